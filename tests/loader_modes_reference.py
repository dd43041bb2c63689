"""numpy float64 restatements of the loader-mode semantics (include/saltnet.h) and the case table the CPU and GPU tests share.

    R1  resize_map          ResizeArray: skimage 0.14 resize(order 1, mode 'constant', cval 0), no anti-aliasing     (loaders.py:786-795)
    R2  resize_back         postprocessing.resize_image on (C,H,W) -> (C,h,w): map_coordinates(order 1), down-scale only
    R3  mask_target         the PIL BILINEAR two-pass 8-bit resize of (mask == k), k in (0, 1)                      (loaders.py:355-360)
    R5  reflect_index/pad   cv2.BORDER_REFLECT_101 = np.pad(mode='reflect')

None of the reference's own libraries (skimage, imgaug, cv2) can be executed here; test_loader_modes_cpu.py pins R1 / R2 against
scipy.ndimage.map_coordinates, R3 against PIL and R5 against np.pad.  Importable without a GPU and without the built library."""
import numpy as np

from oracle.inputs import resize_cubic_u8_fixed  # noqa: F401  (the R4 / R5 compositions of the GPU tests resize with the existing oracle)

SWEEP = np.linspace(0.5, 0.3, 21)
THRESHOLDS = {1: np.array([0.5]), 21: SWEEP, 32: np.concatenate([SWEEP, np.linspace(0.29, 0.19, 11)])}

# (h, w) -> (H, W)
STACK_SIZES = [((101, 101), (128, 128)), ((5, 7), (8, 16)), ((7, 7), (16, 16)), ((32, 32), (32, 32)), ((9, 9), (8, 8))]
PROB_SIZES = [((128, 128), (101, 101)), ((16, 16), (11, 11)), ((8, 16), (5, 7)), ((32, 32), (32, 32))]
MASK_SIZES = [(101, 128), (7, 16), (5, 8), (32, 32)]
MASK_KINDS = ('empty', 'full', 'noise')
STACK_MAPS = (1, 5, 16, 64)
BATCHES = (1, 3)


def golden_rows(n):
    """the output rows of an R1 / R2 case that tests/golden/F22_loader_modes.npz stores (scipy's values): both borders and the middle"""
    return sorted({0, 1, n // 2, n - 2, n - 1})


def _seed(*key):
    import zlib
    return zlib.crc32(repr(key).encode())


def stack_case(size_in, M, B):
    """first-level probability maps [B, h, w, M] float32 in [0, 1)"""
    h, w = size_in
    return np.random.RandomState(_seed('stack', h, w, M, B)).random_sample((B, h, w, M)).astype(np.float32)


def prob_case(size_in, C, B):
    """network probabilities [B, C, H, W] float32 in [0, 1) and the original-size ground truth is drawn by gt_case"""
    H, W = size_in
    return np.random.RandomState(_seed('prob', H, W, C, B)).random_sample((B, C, H, W)).astype(np.float32)


def gt_case(size_out, B):
    h, w = size_out
    return (np.random.RandomState(_seed('gt', h, w, B)).random_sample((B, h, w)) < 0.4).astype(np.uint8)


def mask_case(n, kind, B=2):
    """[B, n, n] uint8 masks in {0, 1}"""
    if kind == 'empty':
        return np.zeros((B, n, n), np.uint8)
    if kind == 'full':
        return np.ones((B, n, n), np.uint8)
    return (np.random.RandomState(_seed('mask', n, B)).random_sample((B, n, n)) < 0.5).astype(np.uint8)


# ----------------------------------------------------------------------------- R1 / R2
def src_coords(n_in, n_out):
    """r(i) = s (i + 0.5) - 0.5 with s = n_in / n_out, float64, every operation rounded on its own"""
    s = np.float64(n_in) / np.float64(n_out)
    return s * (np.arange(n_out, dtype=np.float64) + 0.5) - 0.5


def bilinear64(P, r, c):
    """the four-tap interpolant of saltnet.h on the last two axes of P at the grid r x c; P reads 0 outside"""
    P = np.asarray(P, np.float64)
    h, w = P.shape[-2:]
    r0, c0 = np.floor(r).astype(np.int64), np.floor(c).astype(np.int64)
    dr, dc = (r - r0)[:, None], (c - c0)[None, :]
    Z = np.zeros(P.shape[:-2] + (h + 2, w + 2))
    Z[..., 1:-1, 1:-1] = P
    if r0.min() < -1 or r0.max() > h - 1 or c0.min() < -1 or c0.max() > w - 1:
        raise ValueError('bilinear64: coordinates further than one pixel outside the map')
    tap = lambda y, x: Z[..., (y + 1)[:, None], (x + 1)[None, :]]
    top = (1.0 - dc) * tap(r0, c0) + dc * tap(r0, c0 + 1)
    bot = (1.0 - dc) * tap(r0 + 1, c0) + dc * tap(r0 + 1, c0 + 1)
    return (1.0 - dr) * top + dr * bot


def resize_map(P, size_out):
    """R1 on the last two axes (float64 result; the loader rounds it once to float32)"""
    h, w = np.shape(P)[-2:]
    return bilinear64(P, src_coords(h, size_out[0]), src_coords(w, size_out[1]))


def stack_resize(x, size_out):
    """[B, h, w, M] -> float64 [B, M, H, W]: ResizeArray per map + to_tensor_stacking"""
    return resize_map(np.transpose(np.asarray(x, np.float64), (0, 3, 1, 2)), size_out)


def resize_back(P, size_out):
    """R2 on the last two axes: down-scale (or equal size) only"""
    H, W = np.shape(P)[-2:]
    if size_out[0] > H or size_out[1] > W:
        raise ValueError('resize_back: %dx%d -> %dx%d is an up-scale' % (H, W, size_out[0], size_out[1]))
    return bilinear64(P, src_coords(H, size_out[0]), src_coords(W, size_out[1]))


def counts(v64, gt, thresholds):
    """(inter [B,T], pred [B,T], gt [B]) of pred_t = v64 > t, integers"""
    g = np.asarray(gt) != 0
    pr = v64[:, None] > np.asarray(thresholds, np.float64)[None, :, None, None]
    return (pr & g[:, None]).sum((2, 3)).astype(np.int64), pr.sum((2, 3)).astype(np.int64), g.sum((1, 2)).astype(np.int64)


# ----------------------------------------------------------------------------- R3
def pil_axis_table(n_in, n_out):
    """PIL's precompute_coeffs for BILINEAR in float64: (start [n_out] int32, length [n_out] int32, weights [n_out, taps] float64)"""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = 1.0 * fs
    taps = int(np.ceil(support)) * 2 + 1
    start, length, weights = np.zeros(n_out, np.int32), np.zeros(n_out, np.int32), np.zeros((n_out, taps), np.float64)
    ss = 1.0 / fs
    for x in range(n_out):
        centre = (x + 0.5) * scale
        lo = max(int(centre - support + 0.5), 0)
        hi = min(int(centre + support + 0.5), n_in)
        k = np.array([max(1.0 - abs((t + lo - centre + 0.5) * ss), 0.0) for t in range(hi - lo)], np.float64)
        ww = 0.0
        for v in k:
            ww += v
        if ww != 0.0:
            k = k * (1.0 / ww)
        start[x], length[x] = lo, hi - lo
        weights[x, :hi - lo] = k
    return start, length, weights


def _pass(a, table):
    """one 8-bit pass along the LAST axis of a (values on the uint8 grid, float64): (rounded result, weighted sums)"""
    start, length, weights = table
    acc = np.zeros(a.shape[:-1] + (len(start),), np.float64)
    for t in range(weights.shape[1]):
        on = t < length
        idx = np.where(on, start + t, 0)
        acc = acc + np.where(on, weights[:, t], 0.0) * a[..., idx]
    return np.floor(acc + 0.5), acc


def mask_target(mask, size_out, with_sums=False):
    """R3: [B, h, w] uint8 -> float32 [B, 2, H, W]; ``with_sums``: also the weighted sums of both passes (the fitness check)"""
    mask = np.asarray(mask)
    tr, tc = pil_axis_table(mask.shape[1], size_out[0]), pil_axis_table(mask.shape[2], size_out[1])
    out, sums = [], []
    for k in (0, 1):
        hor, s1 = _pass((mask == k).astype(np.float64), tc)                       # horizontal first
        ver, s2 = _pass(np.swapaxes(hor, 1, 2), tr)                               # then vertical
        out.append(np.swapaxes(ver, 1, 2))
        sums += [s1, s2]
    res = np.stack(out, 1).astype(np.float32)
    return (res, sums) if with_sums else res


def tie_distance(sums):
    """smallest distance of any weighted sum to k + 0.5"""
    return min(float(np.abs(s - np.floor(s) - 0.5).min()) for s in sums)


# ----------------------------------------------------------------------------- R5
def reflect_index(i, n):
    """reflect-101 of index i on an axis of n pixels, one reflection"""
    i = np.abs(np.asarray(i))
    return np.where(i >= n, 2 * n - 2 - i, i) if n > 1 else np.zeros_like(i)


def reflect_pad(a, top, bottom, left, right):
    """pad the last two axes; raises where a side is wider than n - 1"""
    h, w = a.shape[-2:]
    if max(top, bottom) > h - 1 or max(left, right) > w - 1:
        raise ValueError('reflect pad needs pad <= n - 1')
    yy = reflect_index(np.arange(-top, h + bottom), h)
    xx = reflect_index(np.arange(-left, w + right), w)
    return a[..., yy[:, None], xx[None, :]]


def edge_pad(a, top, bottom, left, right):
    h, w = a.shape[-2:]
    yy = np.clip(np.arange(-top, h + bottom), 0, h - 1)
    xx = np.clip(np.arange(-left, w + right), 0, w - 1)
    return a[..., yy[:, None], xx[None, :]]


def normalise(gray_u8, H, channels=3, mean=0.485, std=0.229):
    """Grayscale + ToTensor + Normalize + AddDepthChannels of a padded uint8 tile [B, H, W] -> float64 [B, channels, H, W]"""
    c0 = (np.asarray(gray_u8, np.float64) / 255.0 - mean) / std
    if channels == 1:
        return c0[:, None]
    ramp = np.linspace(0, 1, H)[None, :, None] * np.ones_like(c0)
    return np.stack([c0, ramp, c0 * ramp], 1)
