"""Generate tests/golden/F24_lovasz_options.npz by executing the reference's lovasz_hinge / lovasz_softmax with every combination of
their options (build container only; needs the reference checkout, loaded through ref_import.py as make_golden.py does).

    python tests/golden/make_golden_lovasz_options.py

Inputs (seeded, tie-free): logits [3,2,6,5], probabilities [3,3,6,5] (a softmax of seeded logits).  Two label sets each: without
void labels (ignore=None) and with them (ignore=255): image 0 all void, image 1 partly void.  Softmax classes: class 2 is absent from
the whole batch, class 1 from image 2; no class row keeps exactly one valid pixel.  Stored per combination: the loss and the autograd
gradient with respect to the logits / probabilities.

Why the shapes are this small: the reference computes g_k = J_k - J_(k-1) in fp32, an absolute error of about 2^-24 whatever the row
length, while the largest gradient of a row with G positives is about 1 / G.  The float64 closed forms are compared with these fp32
gradients at 1e-5 of the largest one, which only means something while G stays below about a hundred: the batch-flat hinge row here
has 180 elements (a [3,2,12,10] batch gives 720, G = 288, where the reference's own rounding alone is 2e-5)."""
import itertools
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_import as R            # noqa: E402

VOID = 255


def main():
    assert R.reference_available(), 'reference not mounted'
    ll = R.load('lovasz_losses')
    g = torch.Generator().manual_seed(24)
    out = {}
    # ---- hinge: logits [3,2,6,5], labels of the same shape
    z = torch.randn(3, 2, 6, 5, generator=g) * 2
    t = (torch.rand(3, 2, 6, 5, generator=g) < 0.4).long()
    tv = t.clone()
    tv[0] = VOID
    tv[1][torch.rand(2, 6, 5, generator=g) < 0.3] = VOID
    out.update(hinge_z=z, hinge_t=t.float(), hinge_t_void=tv.float())
    for per_image, ig in itertools.product((True, False), (False, True)):
        zz = z.clone().requires_grad_(True)
        loss = ll.lovasz_hinge(zz, tv if ig else t, per_image=per_image, ignore=VOID if ig else None)
        loss.backward()
        tag = 'hinge_pi%d_ig%d' % (per_image, ig)
        out[tag + '_loss'], out[tag + '_grad'] = loss.detach(), zz.grad
    # ---- softmax: probabilities [3,3,6,5], class labels [3,6,5]
    p = torch.softmax(torch.randn(3, 3, 6, 5, generator=g) * 2, 1)
    y = torch.randint(0, 2, (3, 6, 5), generator=g)           # class 2 never occurs
    y[2] = 0                                                    # class 1 is absent from image 2
    yv = y.clone()
    yv[0] = VOID
    yv[1][torch.rand(6, 5, generator=g) < 0.3] = VOID
    assert all(int((yv[b] != VOID).sum()) != 1 for b in range(3)) and int((yv != VOID).sum()) != 1
    out.update(softmax_p=p, softmax_y=y, softmax_y_void=yv)
    for only_present, per_image, ig in itertools.product((False, True), (True, False), (False, True)):
        pp = p.clone().requires_grad_(True)
        loss = ll.lovasz_softmax(pp, yv if ig else y, only_present=only_present, per_image=per_image, ignore=VOID if ig else None)
        loss.backward()
        tag = 'softmax_op%d_pi%d_ig%d' % (only_present, per_image, ig)
        out[tag + '_loss'], out[tag + '_grad'] = loss.detach(), pp.grad
    arrays = {k: np.asarray(v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in out.items()}
    for k, v in arrays.items():
        assert np.isfinite(v).all(), k
    path = os.path.join(HERE, 'F24_lovasz_options.npz')
    np.savez_compressed(path, **arrays)
    print('wrote %s %.1f KB, %d arrays' % (path, os.path.getsize(path) / 1024, len(arrays)))


if __name__ == '__main__':
    main()
