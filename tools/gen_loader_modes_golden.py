"""Writes tests/golden/F22_loader_modes.npz: what the libraries that CAN be executed say about the loader-mode cases
(tests/loader_modes_reference.py).  No reference code runs here: PIL resizes the stacking-target masks (the reference's
transforms.Resize is PIL BILINEAR), scipy.ndimage.map_coordinates evaluates a handful of R1 / R2 vectors.

    python tools/gen_loader_modes_golden.py
"""
import os
import sys

import numpy as np
from PIL import Image
from scipy import ndimage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
import loader_modes_reference as L  # noqa: E402


def pil_target(mask, size):
    """loaders.py:355-360 per class: Image.fromarray((mask == k) uint8) -> Resize((H, W)) (BILINEAR) -> convert('L') -> float32"""
    out = []
    for k in (0, 1):
        im = Image.fromarray((mask == k).astype(np.uint8)).resize((size, size), Image.BILINEAR).convert('L')
        out.append(np.asarray(im, dtype=np.uint8))
    return np.stack(out, 0)


def scipy_resize(P, size_out, mode):
    h, w = P.shape
    rr, cc = np.meshgrid(L.src_coords(h, size_out[0]), L.src_coords(w, size_out[1]), indexing='ij')
    return ndimage.map_coordinates(P.astype(np.float64), [rr, cc], order=1, mode=mode, cval=0.0)


def main():
    out = {}
    for n, N in L.MASK_SIZES:
        for kind in L.MASK_KINDS:
            m = L.mask_case(n, kind)
            out['mask_%d_%d_%s' % (n, N, kind)] = m
            out['pil_%d_%d_%s' % (n, N, kind)] = np.stack([pil_target(t, N) for t in m], 0)
    for (hw, HW) in L.STACK_SIZES:
        x = L.stack_case(hw, 5, 1)
        out['r1_%dx%d_%dx%d' % (hw + HW)] = np.stack([scipy_resize(x[0, :, :, m], HW, 'grid-constant') for m in range(5)], 0)[:, L.golden_rows(HW[0])]
    for (HW, hw) in L.PROB_SIZES:
        p = L.prob_case(HW, 2, 1)
        out['r2_%dx%d_%dx%d' % (HW + hw)] = np.stack([scipy_resize(p[0, c], hw, 'constant') for c in range(2)], 0)[:, L.golden_rows(hw[0])]
    path = os.path.join(ROOT, 'tests', 'golden', 'F22_loader_modes.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
