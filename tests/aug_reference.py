"""numpy restatement of the on-device training augmentation (csrc/augment.hip, saltnet.h salt_augment_preprocess): the RNG's integer
and uniform path, every op, the params layout.  float32 arithmetic is rounded per operation in the order the kernel uses, so the
exact ops (flip, Sharpen, Emboss, the intensity ops) agree bit for bit and the warps within the documented tolerance."""
import numpy as np

from oracle.inputs import resize_cubic_u8_fixed

f32 = np.float32
M64 = (1 << 64) - 1
GOLD = 0x9E3779B97F4A7C15
N_PARAMS = 64
S_PIXEL = 1024
PERMS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))


# ------------------------------------------------------------------ RNG (python ints for scalars, uint64 arrays for per-pixel draws)
def mix64(z):
    z = (z + GOLD) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def key(seed, counter, b):
    return mix64(mix64(mix64(int(seed) & M64) ^ int(counter)) ^ int(b))


def bits(k, slot):
    return mix64((k + slot * GOLD) & M64)


def mix64_np(z):
    z = np.asarray(z, np.uint64)
    with np.errstate(over='ignore'):
        z = z + np.uint64(GOLD)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def bits_np(k, slots):
    with np.errstate(over='ignore'):
        return mix64_np(np.uint64(k) + np.asarray(slots, np.uint64) * np.uint64(GOLD))


def uniform_np(b):
    return (b >> np.uint64(40)).astype(f32) * f32(1.0 / 16777216.0)


def int_np(b, lo, hi):
    return lo + (((b >> np.uint64(32)) * np.uint64(hi - lo + 1)) >> np.uint64(32)).astype(np.int64)


def uniform(k, slot):
    return float(uniform_np(np.uint64(bits(k, slot))))


def draw_int(k, slot, lo, hi):
    return lo + (((bits(k, slot) >> 32) * (hi - lo + 1)) >> 32)


def draw_range(k, slot, lo, hi):
    return f32(lo) + f32(uniform(k, slot)) * (f32(hi) - f32(lo))


# ------------------------------------------------------------------ params record
def empty_params(B=1):
    return np.zeros((B, N_PARAMS), np.float32)


def decode(p):
    """row [64] -> dict (the same names as salt_amd.input_pipeline.decode_params, one image)"""
    p = np.asarray(p, np.float32)
    return {'order': int(p[0]), 'n': int(p[1]), 'chosen': p[2:6] != 0, 'flip': bool(p[6]), 'angle': p[7], 'shift': p[8],
            'piecewise': bool(p[9]), 'piecewise_scale': p[10], 'piecewise_jitter': p[11:43].reshape(4, 4, 2), 'perspective': bool(p[43]),
            'perspective_scale': p[44], 'perspective_corners': p[45:53].reshape(4, 2), 'invert': bool(p[53]), 'contrast': bool(p[54]),
            'contrast_alpha': p[55], 'intensity_op': int(p[56]), 'value': p[57]}


# ------------------------------------------------------------------ ops (uint8 planes in, uint8 planes out)
def to_u8(v):
    return np.clip(np.floor(np.asarray(v, f32) + f32(0.5)), 0, 255).astype(np.uint8)


def fliplr(a):
    return a[:, ::-1].copy()


def sharpen_matrix(alpha=0.5, lightness=1.0):
    a = f32(alpha)
    k = np.full((3, 3), a * f32(-1), f32)
    k[1, 1] = (f32(1) - a) + a * (f32(8) + f32(lightness))
    return k


def emboss_matrix(alpha=0.5, strength=1.0):
    a, s = f32(alpha), f32(strength)
    m = np.array([[-1 - s, -s, 0], [-s, 1, s], [0, s, 1 + s]], f32)
    k = (a * m).astype(f32)
    k[1, 1] = (f32(1) - a) + k[1, 1]
    return k


def conv3x3(a, k, binarize=False):
    """cv2.filter2D (correlation), reflect-101 border, products added row by row in float32"""
    h, w = a.shape
    p = np.pad(a.astype(f32), 1, mode='reflect') if min(h, w) > 1 else np.pad(a.astype(f32), 1, mode='edge')
    acc = np.zeros((h, w), f32)
    for dy in range(3):
        for dx in range(3):
            acc = acc + k[dy, dx] * p[dy:dy + h, dx:dx + w]
    v = to_u8(acc)
    return (v != 0).astype(np.uint8) if binarize else v


def bilinear_value(a, sy, sx, edge):
    """float32 bilinear value at float32 coordinates (arrays); edge: clamped taps, else 0 outside"""
    h, w = a.shape
    sy = np.fmin(np.fmax(np.asarray(sy, f32), f32(-2)), f32(h + 1))
    sx = np.fmin(np.fmax(np.asarray(sx, f32), f32(-2)), f32(w + 1))
    y0f, x0f = np.floor(sy), np.floor(sx)
    fy, fx = sy - y0f, sx - x0f
    y0, x0 = y0f.astype(np.int64), x0f.astype(np.int64)
    af = a.astype(f32)

    def tap(yy, xx):
        if edge:
            return af[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)]
        ok = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
        return np.where(ok, af[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)], f32(0))
    gx, gy = f32(1) - fx, f32(1) - fy
    top = gx * tap(y0, x0) + fx * tap(y0, x0 + 1)
    bot = gx * tap(y0 + 1, x0) + fx * tap(y0 + 1, x0 + 1)
    return (gy * top + fy * bot).astype(f32)


def affine_coords(h, w, angle, shift):
    rad = np.float64(f32(angle)) * 0.017453292519943295
    cs, sn = f32(np.cos(rad)), f32(np.sin(rad))
    cx, cy = f32(w) * f32(0.5) - f32(0.5), f32(h) * f32(0.5) - f32(0.5)
    tx = f32(shift) * f32(w)
    y, x = np.mgrid[0:h, 0:w].astype(f32)
    dx, dy = (x - cx) - tx, y - cy
    return (cs * dy - sn * dx) + cy, (cs * dx + sn * dy) + cx


def piecewise_coords(h, w, jitter):
    """jitter [4,4,2] (dy, dx) fractions of h / w -> source coordinates of every output pixel"""
    J = np.asarray(jitter, f32)
    reg_y = np.array([f32(i * h) / f32(3) for i in range(4)], f32)
    reg_x = np.array([f32(j * w) / f32(3) for j in range(4)], f32)
    P = np.empty((4, 4, 2), f32)
    for i in range(4):
        for j in range(4):
            P[i, j, 0] = reg_y[i] + J[i, j, 0] * f32(h)
            P[i, j, 1] = reg_x[j] + J[i, j, 1] * f32(w)
    y, x = np.mgrid[0:h, 0:w]
    ci, cj = np.minimum(3 * y // h, 2), np.minimum(3 * x // w, 2)
    v = (3 * y).astype(f32) / f32(h) - ci.astype(f32)
    u = (3 * x).astype(f32) / f32(w) - cj.astype(f32)
    out = []
    for q in range(2):
        tl, tr, bl, br = P[ci, cj, q], P[ci, cj + 1, q], P[ci + 1, cj, q], P[ci + 1, cj + 1, q]
        upper = (tl + u * (tr - tl)) + v * (br - tr)
        lower = (tl + v * (bl - tl)) + u * (br - bl)
        out.append(np.where(u >= v, upper, lower).astype(f32))
    return out[0], out[1]


def perspective_quad(h, w, corners):
    q = np.asarray(corners, f32).reshape(8)
    fw, fh = f32(w), f32(h)
    x0, y0 = q[0] * fw, q[1] * fh
    x1, y1 = fw - q[2] * fw, q[3] * fh
    x2, y2 = fw - q[4] * fw, fh - q[5] * fh
    x3, y3 = q[6] * fw, fh - q[7] * fh

    def ln(ax, ay, bx, by):
        dx, dy = ax - bx, ay - by
        return int(np.sqrt(dx * dx + dy * dy))
    mw = max(ln(x2, y2, x3, y3), ln(x1, y1, x0, y0))
    mh = max(ln(x3, y3, x0, y0), ln(x2, y2, x1, y1))
    sx, sy = ((x0 - x1) + x2) - x3, ((y0 - y1) + y2) - y3
    dx1, dx2, dy1, dy2 = x1 - x2, x3 - x2, y1 - y2, y3 - y2
    den = dx1 * dy2 - dx2 * dy1
    g = (sx * dy2 - dx2 * sy) / den if den != 0 else f32(0)
    hh = (dx1 * sy - sx * dy1) / den if den != 0 else f32(0)
    H = [(x1 - x0) + g * x1, (x3 - x0) + hh * x3, x0, (y1 - y0) + g * y1, (y3 - y0) + hh * y3, y0, g, hh]
    return [f32(v) for v in H], min(max(mw, 2), 182), min(max(mh, 2), 182)


def perspective_rect_coords(H, mw, mh):
    is_, it = f32(1) / f32(mw - 1), f32(1) / f32(mh - 1)
    v, u = np.mgrid[0:mh, 0:mw].astype(f32)
    s, t = u * is_, v * it
    z = (H[6] * s + H[7] * t) + f32(1)
    return ((H[3] * s + H[4] * t) + H[5]) / z, ((H[0] * s + H[1] * t) + H[2]) / z


def cubic_w(t):
    A = f32(-0.75)
    t = np.asarray(t, f32)
    x1 = t + f32(1)
    c0 = (((A * x1 - f32(5) * A) * x1 + f32(8) * A) * x1) - f32(4) * A
    c1 = (((A + f32(2)) * t - (A + f32(3))) * t) * t + f32(1)
    u = f32(1) - t
    c2 = (((A + f32(2)) * u - (A + f32(3))) * u) * u + f32(1)
    c3 = ((f32(1) - c0) - c1) - c2
    return [c0.astype(f32), c1.astype(f32), c2.astype(f32), c3.astype(f32)]


def resize_cubic_float(a, oh, ow):
    """the float cubic back from the rectified quad: separable taps, replicated border, per-operation float32 rounding"""
    ih, iw = a.shape
    scy, scx = f32(ih) / f32(oh), f32(iw) / f32(ow)
    af = a.astype(f32)
    fy = (np.arange(oh).astype(f32) + f32(0.5)) * scy - f32(0.5)
    fx = (np.arange(ow).astype(f32) + f32(0.5)) * scx - f32(0.5)
    y0f, x0f = np.floor(fy), np.floor(fx)
    wy, wx = cubic_w(fy - y0f), cubic_w(fx - x0f)
    y0, x0 = y0f.astype(np.int64) - 1, x0f.astype(np.int64) - 1
    acc = np.zeros((oh, ow), f32)
    for i in range(4):
        yy = np.clip(y0 + i, 0, ih - 1)
        row = np.zeros((oh, ow), f32)
        for j in range(4):
            xx = np.clip(x0 + j, 0, iw - 1)
            row = row + wx[j][None, :] * af[yy][:, xx]
        acc = acc + wy[i][:, None] * row
    return acc


def warp(img, msk, kind, d):
    """one warp stage -> (img, mask, mask's float value before rounding: the tolerance band of the tests)"""
    h, w = img.shape
    if kind in ('affine', 'piecewise'):
        sy, sx = affine_coords(h, w, d['angle'], d['shift']) if kind == 'affine' else piecewise_coords(h, w, d['piecewise_jitter'])
        edge = kind == 'affine'
        mv = bilinear_value(msk, sy, sx, edge)
        return to_u8(bilinear_value(img, sy, sx, edge)), (to_u8(mv) != 0).astype(np.uint8), mv
    H, mw, mh = perspective_quad(h, w, d['perspective_corners'])
    ry, rx = perspective_rect_coords(H, mw, mh)
    ri = to_u8(bilinear_value(img, ry, rx, False))
    mv_rect = bilinear_value(msk, ry, rx, False)
    rm = (to_u8(mv_rect) != 0).astype(np.uint8)
    mv = resize_cubic_float(rm, h, w)
    return to_u8(resize_cubic_float(ri, h, w)), (to_u8(mv) != 0).astype(np.uint8), mv


def geometric(img, msk, p, sharpen=(0.5, 1.0), emboss=(0.5, 1.0)):
    """the affine_seq stages of one params row on one image / binarised mask; also the list of mask float values of the warps"""
    d = decode(p)
    img, msk = img.copy(), (msk != 0).astype(np.uint8)
    bands = []
    for stage in PERMS[min(max(d['order'], 0), 5)]:
        if stage == 0:
            if d['chosen'][0] and d['flip']:
                img, msk = fliplr(img), fliplr(msk)
            if d['chosen'][1]:
                k = sharpen_matrix(*sharpen)
                img, msk = conv3x3(img, k), conv3x3(msk, k, True)
            if d['chosen'][2]:
                k = emboss_matrix(*emboss)
                img, msk = conv3x3(img, k), conv3x3(msk, k, True)
            if d['chosen'][3]:
                img, msk, mv = warp(img, msk, 'affine', d)
                bands.append(mv)
        elif stage == 1 and d['piecewise']:
            img, msk, mv = warp(img, msk, 'piecewise', d)
            bands.append(mv)
        elif stage == 2 and d['perspective']:
            img, msk, mv = warp(img, msk, 'perspective', d)
            bands.append(mv)
    return img, msk, bands


def resize_pad(a, resize=102, pad=13):
    r = resize_cubic_u8_fixed(a, resize, resize) if resize != a.shape[0] else a
    return np.pad(r, pad, mode='edge')


def intensity(g, p, seed, counter, b, add=(-10, 10), multiply=(0.95, 1.05)):
    """intensity_seq of one params row on the padded uint8 grid [H, W]"""
    d = decode(p)
    v = g.astype(np.int64)
    if d['invert']:
        v = 255 - v
    if d['contrast']:
        v = to_u8(d['contrast_alpha'] * (v - 128).astype(f32) + f32(128)).astype(np.int64)
    op = d['intensity_op']
    if op in (2, 4):
        pix = bits_np(key(seed, counter, b), S_PIXEL + np.arange(v.size, dtype=np.uint64)).reshape(v.shape)
    if op == 1:
        v = np.clip(v + int(d['value']), 0, 255)
    elif op == 2:
        v = np.clip(v + int_np(pix, add[0], add[1]), 0, 255)
    elif op == 3:
        v = to_u8(v.astype(f32) * f32(d['value'])).astype(np.int64)
    elif op == 4:
        m = f32(multiply[0]) + uniform_np(pix) * (f32(multiply[1]) - f32(multiply[0]))
        v = to_u8(v.astype(f32) * m).astype(np.int64)
    return v.astype(np.uint8)


def normalise(g, mean=0.485, std=0.229):
    """x[:, 0] of the kernel from the gray uint8 grid"""
    return ((g.astype(f32) * f32(1.0 / 255.0)) - f32(mean)) * (f32(1) / f32(std))
