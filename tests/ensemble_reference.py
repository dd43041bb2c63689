"""numpy restatements of the ensembling operators (include/saltnet.h) and the case tables the CPU and GPU tests share.
Nothing here imports the product; the float64 interpolant is the one of tests/loader_modes_reference.py.

    E1  fold_mean           np.mean(np.array(maps), axis=0) as ONE fixed order: start at member 0, add members in ascending k in the
                            accumulator's type, one division by K (main.py:893; the notebook's float64 accumulator)
    E2  crop / resized      postprocessing.crop_image with utils.get_crop_pad_sequence; postprocessing.resize_image (R2)
    E3  stack               np.stack of every member's class map, [B,h,w,M] (utils.py:580) or [B,M,h,w]
    E4  fold_split          KFoldBySortedValue under BaseCrossValidator.split (utils.py:371-389)
    E5  rle / submission    utils.run_length_encoding, create_submission's rows (utils.py:68-75, 99-111)

Importable without a GPU and without the built library."""
import zlib

import numpy as np

import loader_modes_reference as L

KS = (2, 3, 7, 8, 9, 33, 64)                       # member counts of the np.mean == sequential-sum check
# (H, W, top, left, h, w)
CROP_CASES = [(16, 16, 0, 0, 16, 16), (16, 20, 3, 5, 9, 11), (128, 128, 13, 14, 101, 101)]
# (H, W, h, w)
RESIZE_CASES = [(128, 128, 101, 101), (16, 12, 7, 5), (8, 8, 8, 8)]
ENSEMBLE_KS = (1, 2, 7, 64)
THRESHOLDS = (0.5, 0.47)                           # 0.47 is no fp32 value: float32(0.47) < 0.47
RLE_SHAPES = [(1, 1), (3, 7), (101, 101), (128, 128), (64, 200), (256, 256)]
RLE_PATTERNS = ('empty', 'full', 'first', 'last', 'checker', 'columns', 'random10', 'random50', 'random90')


def _seed(*key):
    return zlib.crc32(repr(key).encode())


# ----------------------------------------------------------------------------- E1 / E2
def crop_window(H, W, target_size):
    """utils.get_crop_pad_sequence as postprocessing.crop_image uses it: (top, left) of the window"""
    vertical, horizontal = H - target_size[0], W - target_size[1]
    top, right = int(vertical / 2), int(horizontal / 2)
    return top, horizontal - right


def crop(p, top, left, h, w):
    return p[..., top:top + h, left:left + w]


def fold_mean(values, dtype):
    """values: K arrays; the accumulator starts at member 0 and adds in ascending k in ``dtype``; ONE division by K in ``dtype``"""
    s = np.array(values[0], dtype=dtype)
    for v in values[1:]:
        s = s + np.asarray(v, dtype)
    return s / dtype(len(values))


def decide(mean, threshold):
    """binarize: a float32 mean is compared with float32(threshold), a float64 mean with the threshold itself"""
    return (mean > mean.dtype.type(threshold)).astype(np.uint8)


def resized(p, size_out):
    """float64 interpolant of every [H,W] plane of a float32 map"""
    return L.resize_back(np.asarray(p, np.float64), size_out)


def stack(values, layout):
    """values: K maps [B,h,w] -> float32 [B,h,w,K] ('hwm', np.stack(axis=-1)) or [B,K,h,w] ('mhw')"""
    return np.stack([np.asarray(v).astype(np.float32) for v in values], axis=-1 if layout == 'hwm' else 1)


# ----------------------------------------------------------------------------- E4
def fold_split(values, n_splits):
    """[(train, test)]: a stable sort by value, fold s holds every n_splits-th of the sorted samples from s; both index arrays ascend"""
    values = np.asarray(values)
    order = [i for i, _ in sorted(zip(range(len(values)), values.tolist()), key=lambda t: t[1])]      # Python's sort is stable
    out = []
    for s in range(n_splits):
        test = sorted(order[s::n_splits])
        out.append((np.array([i for i in range(len(values)) if i not in set(test)], np.int64), np.array(test, np.int64)))
    return out


# ----------------------------------------------------------------------------- E5
def run_length_encoding(x):
    """utils.py:99-111 by its definition: maximal runs of the column-major order, (1-based start, length)"""
    flat = (np.asarray(x).T.reshape(-1) != 0)
    rle, p, n = [], 0, flat.size
    while p < n:
        if flat[p]:
            q = p
            while q + 1 < n and flat[q + 1]:
                q += 1
            rle += [p + 1, q - p + 1]
            p = q + 1
        else:
            p += 1
    return rle


def run_length_decoding(rle, shape):
    img = np.zeros(shape[0] * shape[1], np.uint8)
    for lo, n in zip(rle[0::2], rle[1::2]):
        img[lo - 1:lo - 1 + n] = 1
    return img.reshape((shape[1], shape[0])).T


def submission_rows(ids, masks):
    return [(str(i), ' '.join(str(v) for v in run_length_encoding(m))) for i, m in zip(ids, masks)]


# ----------------------------------------------------------------------------- cases
def member_maps(K, B, C, H, W, window=None, threshold=None):
    """K float32 maps [B,C,H,W] in [0, 1).  With ``window`` = (top, left, h, w) and a threshold, the first three pixels of the window of
    every channel are planted: EVERY member holds float32(threshold) at the first, the fp32 value one ulp below it at the second and
    one ulp above it at the third.  The float64 mean of K equal fp32 values v is v itself (j v is exact in float64), so it sits on
    the fp32 neighbours of the threshold, on either side of a threshold fp32 cannot represent; the fp32 mean is v while j v stays
    exact (always for v = 0.5) and within a few ulps of it otherwise: the pixels where the accumulator type and the type the
    threshold is compared in decide the mask."""
    r = np.random.RandomState(_seed('members', K, B, C, H, W))
    maps = [r.random_sample((B, C, H, W)).astype(np.float32) for _ in range(K)]
    if window is not None:
        top, left, h, w = window
        t = np.float32(threshold)
        plant = [t, np.nextafter(t, np.float32(0)), np.nextafter(t, np.float32(1))]
        for j, v in enumerate(plant):
            y, x = divmod(j, w)
            if y < h:
                for m in maps:
                    m[:, :, top + y, left + x] = v
    return maps


def rle_mask(shape, pattern):
    h, w = shape
    m = np.zeros((h, w), np.uint8)
    if pattern == 'full':
        m[:] = 1
    elif pattern == 'first':
        m[0, 0] = 1
    elif pattern == 'last':
        m[h - 1, w - 1] = 1
    elif pattern == 'checker':                     # set at every even column-major position: ceil(h w / 2) runs of one pixel
        flat = np.zeros(h * w, np.uint8)
        flat[0::2] = 1
        m = np.ascontiguousarray(flat.reshape(w, h).T)
    elif pattern == 'columns':                     # whole columns, two of them adjacent: runs that cross the column ends
        m[:, 0::3] = 1
        m[:, 1::6] = 1
    elif pattern.startswith('random'):
        m = (np.random.RandomState(_seed('rle', h, w, pattern)).random_sample((h, w)) < int(pattern[6:]) / 100.0).astype(np.uint8)
    return m
