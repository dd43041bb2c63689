"""The thin-channel entry points of csrc/conv_small.hip through the C-ABI for the tests: salt_conv_first, salt_conv_first_wgrad,
salt_head1x1, salt_head1x1_bwd, salt_s2d, salt_pack_stem_weight and salt_stem_grad_unfold.  One place that fills their argument
structs, asks which kernel a launch takes (salt_head1x1_kernel_id, salt_head1x1_bwd_kernel_id, salt_conv_first_wgrad_kernel_id: host
only, no launch), and holds the float64 reference of the same operands with a per-element error bound.
test_small_reference_cpu.py pins the references against torch on the CPU, test_gpu_small_abi.py holds every kernel to them.

References (from the definitions in include/saltnet.h, as loops over taps; float64, never rounded):
    conv_first        v[b, oy, ox, n] = sum_{c, kh, kw} X[b, c, oy s - p + kh, ox s - p + kw] W[n][c][kh][kw]   (zero outside the image)
                      y = store(relu?((v + bias) scale + shift)); per 16 x 16 tile: sum, M2 about the tile mean and count of the
                      epilogue values BEFORE their storage rounding (the kernel takes them from its accumulators)
    conv_first_wgrad  dW[n][c][kh][kw] = sum_{b, oy, ox} dY[b, oy, ox, n] X[b, c, oy s - p + kh, ox s - p + kw]  (+ old with accumulate)
    head1x1           y[b, h, w, o] = sum_c X[b, h, w, c] W[o][c] + bias[o], fp32 NCHW or an NHWC view of the activation dtype
    head1x1_bwd       dx[b, h, w, c] = sum_o dY[b, o, h, w] W[o][c] (+ old), gw[o][c] = sum_pixels dY X, gb[o] = sum_pixels dY
    s2d / pack_stem_weight / stem_grad_unfold: index maps (s2d_ref, pack_stem_ref, stem_unfold_ref), compared bit for bit.

Operands come from wgrad_abi.mk / conv_abi.master_weight: values that bf16 holds exactly, in both dtypes.  Every product then has at
most 16 significant bits and is exact in fp32; a kernel differs from the float64 sum only by the order and rounding of its additions.

The bounds, per element (derived here as DESIGN 15 does, not tuned to a kernel; u = 2^-23, a whole ulp, so that adders that truncate
- the matrix cores - are covered):
  * conv_first, head1x1: K - 1 fp32 additions of exact products in any order, each off by at most u |partial sum| <= u A with
    A = sum |x| |w| of the element: t_acc = K u A, K = Cin K K (conv_first) or C (head1x1).  Additions of the exact zeros of the
    padding add nothing.
  * epilogue in fp32 (bias, scale, shift; the head's bias): the error passes through the affine part with gain |scale|, and every
    fp32 operation adds at most half an ulp of its result: tol = t_acc |scale| + 4 u (largest intermediate of the element).
  * weight gradients, gb: the same argument with the N = B OH OW pixels (head: B H W) of the sum in place of K, whatever the tree
    (per-thread runs, tiles, parts, the reduction kernels): N - 1 additions of non-zero terms, the rest add exact zeros.
    tol = N u sum |dy| |x| (gb: N u sum |dy|).  `accumulate` is one more fp32 addition: + 4 u max(|dW|, |dW + old|).
  * dx of the head: K = Cout terms.  With `accumulate` the old value is read back from the activation dtype: the bound allows the new
    term to be rounded to that dtype before the addition (2^-8 (|dx| + tol)), then the fp32 addition (u |dx + old|), then the store.
  * bf16 storage: a value e' = e + d, |d| <= tol, stored as bf16 lands within tol + 2^-8 (|e| + tol) of e (conv_abi._store); one
    such term per storage rounding on the path.  The reference never rounds its intermediates (DESIGN 15 explains why).
  * tile statistics, n = the tile's valid pixels, e_i the unrounded epilogue values known to t_i (the bound before the store):
      sum:  n additions of values off by t_i:           tS = sum t_i + n u (sum |e_i| + sum t_i)
      mean: m' = fl(S' / n):                            tm = tS / n + u |m|
      d_i' = fl(e_i' - m'), off by                      q_i = t_i + tm + u (|d_i| + t_i + tm)
      M2 = sum fl(d_i'^2): (d + q)^2 - d^2 = 2 d q + q^2, one rounding per square and n additions of non-negative terms:
                                                        tM = sum (2 |d_i| q_i + q_i^2) + (n + 2) u sum (|d_i| + q_i)^2
    Counts are exact.
A dropped tap moves an element by about |x w| ~ A / K, i.e. >= 2^23 / K^2 times t_acc (390 bounds at the 7x7 stem); a dropped
pixel of a weight gradient by 2^23 / N^2 bounds: 80 at the base shape of the tables (N = 17 x 19), which is where a wrong tile loop
shows; the cases with 10^4 pixels exist for the reduction kernels, where a wrong part is a whole tile."""
import ctypes

import pytest
import torch

from conv_abi import U32, UBF, _store, bits, last_error, master_weight, mk, ratio           # noqa: F401  (re-exported for the tests)
from op_reference import F64, GUARD, Placed, guard_fill, round_to, torch_dtype            # noqa: F401

DT = {'f32': 0, 'bf16': 1}
VE = {'f32': 4, 'bf16': 8}                # elements of a 16-byte piece
KC = {'f32': 16, 'bf16': 32}              # channels of a packed weight chunk
FT = 16                                   # conv_first's output tile edge
HEAD_SCALAR, HEAD_VEC, HEAD_VEC_CO2 = 1, 2, 3          # salt_head1x1_kernel_id / salt_head1x1_bwd_kernel_id
WIDE = 256                                # salt_conv_first_wgrad_kernel_id: + 256 = partial_sum_wide_kernel; low byte 0 MFMA, else PER


def cdiv(a, b):
    return -(-a // b)


def first_geom(H, W, K, stride, pad):
    return (H + 2 * pad - K) // stride + 1, (W + 2 * pad - K) // stride + 1


def _gather(xd, ci, kh, kw, stride, pad, OH, OW):
    """xd [B,Cin,H,W] float64 -> [B,OH,OW]: X[b, ci, oy s - p + kh, ox s - p + kw], zero outside the image."""
    H, W = xd.shape[2], xd.shape[3]
    iy, ix = torch.arange(OH) * stride - pad + kh, torch.arange(OW) * stride - pad + kw
    ok = ((iy >= 0) & (iy < H)).double()[:, None] * ((ix >= 0) & (ix < W)).double()[None, :]
    return xd[:, ci][:, iy.clamp(0, H - 1)][:, :, ix.clamp(0, W - 1)] * ok


# ---------------------------------------------------------------- float64 references
def conv_first_sum(x, w, stride, pad):
    """x [B,Cin,H,W], w [Cout,Cin,K,K] -> (v, A) [B,OH,OW,Cout] float64."""
    B, Cin, H, W = x.shape
    Cout, _, K, _ = w.shape
    OH, OW = first_geom(H, W, K, stride, pad)
    xd, wd = x.double(), w.double()
    v = torch.zeros(B, OH, OW, Cout, dtype=F64)
    A = torch.zeros_like(v)
    for ci in range(Cin):
        for kh in range(K):
            for kw in range(K):
                g = _gather(xd, ci, kh, kw, stride, pad, OH, OW)[..., None]
                v += g * wd[:, ci, kh, kw]
                A += g.abs() * wd[:, ci, kh, kw].abs()
    return v, A


def epilogue(v, tol, bias=None, scale=None, shift=None, relu=False):
    """relu?((v + bias) scale + shift) of values known to tol -> (e, tol after the fp32 epilogue)."""
    big, e = v.abs(), v
    if bias is not None:
        e = e + bias
        big = torch.maximum(big, e.abs())
    if scale is not None:
        e = e * scale
        tol = tol * scale.abs()
        big = torch.maximum(big, e.abs())
    if shift is not None:
        e = e + shift
        big = torch.maximum(big, e.abs())
    if relu:
        e = e.clamp_min(0)
    return e, tol + 4 * U32 * big


def conv_first_ref(x, w, stride, pad, dtype, bias=None, scale=None, shift=None, relu=False):
    """-> dict(exact, tol: of the stored output; pre_tol: of the epilogue value before its storage rounding; v, A)."""
    v, A = conv_first_sum(x, w, stride, pad)
    K = w.shape[1] * w.shape[2] * w.shape[3]
    e, pre = epilogue(v, K * U32 * A, bias, scale, shift, relu)
    tol, _ = _store(e, pre, dtype)
    return dict(exact=e, tol=tol, pre_tol=pre, v=v, A=A)


def first_stats_ref(e, t):
    """e, t [B,OH,OW,C]: the unrounded epilogue values and their bound -> dict(stats, tol [tiles,2,C], cnt [tiles]) in the launch's tile
    order (image, tile row, tile column)."""
    B, OH, OW, C = e.shape
    stats, tols, cnt = [], [], []
    for b in range(B):
        for i in range(cdiv(OH, FT)):
            for j in range(cdiv(OW, FT)):
                blk = e[b, FT * i:FT * i + FT, FT * j:FT * j + FT].reshape(-1, C)
                tb = t[b, FT * i:FT * i + FT, FT * j:FT * j + FT].reshape(-1, C)
                n = blk.shape[0]
                s = blk.sum(0)
                tS = tb.sum(0) + n * U32 * (blk.abs().sum(0) + tb.sum(0))
                m = s / n
                tm = tS / n + U32 * m.abs()
                d = blk - m
                q = tb + tm + U32 * (d.abs() + tb + tm)
                tM = (2 * d.abs() * q + q * q).sum(0) + (n + 2) * U32 * ((d.abs() + q) ** 2).sum(0)
                stats.append(torch.stack([s, (d * d).sum(0)]))
                tols.append(torch.stack([tS, tM]))
                cnt.append(float(n))
    return dict(stats=torch.stack(stats), tol=torch.stack(tols), cnt=torch.tensor(cnt, dtype=F64))


def conv_first_wgrad_ref(x, dy, K, stride, pad, old=None):
    """x [B,Cin,H,W], dy [B,OH,OW,Cout] (its zero padding is the tile's business, not the definition's), old [Cout,Cin,K,K] or None
    -> dict(exact, tol) [Cout,Cin,K,K]."""
    B, Cin, H, W = x.shape
    _, OH, OW, Cout = dy.shape
    assert (OH, OW) == first_geom(H, W, K, stride, pad)
    xd, gd = x.double(), dy.double()
    dW = torch.zeros(Cout, Cin, K, K, dtype=F64)
    A = torch.zeros_like(dW)
    for ci in range(Cin):
        for kh in range(K):
            for kw in range(K):
                g = _gather(xd, ci, kh, kw, stride, pad, OH, OW)
                dW[:, ci, kh, kw] = torch.einsum('bhw,bhwn->n', g, gd)
                A[:, ci, kh, kw] = torch.einsum('bhw,bhwn->n', g.abs(), gd.abs())
    tol = B * OH * OW * U32 * A
    e = dW
    if old is not None:
        e = dW + old
        tol = tol + 4 * U32 * torch.maximum(dW.abs(), e.abs())
    return dict(exact=e, tol=tol, A=A)


def head_ref(x, w, bias, dtype=None):
    """x [B,H,W,C], w [Cout,C], bias [Cout] | None, float64.  dtype None: the fp32 NCHW logits (returned NHWC all the same), else the
    NHWC view output of that dtype -> dict(exact, tol) [B,H,W,Cout]."""
    v = torch.einsum('bhwc,oc->bhwo', x, w)
    A = torch.einsum('bhwc,oc->bhwo', x.abs(), w.abs())
    e, tol = epilogue(v, x.shape[3] * U32 * A, bias)
    if dtype is not None:
        tol, _ = _store(e, tol, dtype)
    return dict(exact=e, tol=tol, A=A)


def head_bwd_ref(x, w, dy, dtype, old=None):
    """x [B,H,W,C], w [Cout,C], dy [B,Cout,H,W], old [B,H,W,C] | None (accumulate), float64 -> dict(dx, gw, gb: dict(exact, tol))."""
    g = dy.permute(0, 2, 3, 1)
    N = g.shape[0] * g.shape[1] * g.shape[2]
    dx = torch.einsum('bhwo,oc->bhwc', g, w)
    tol = w.shape[0] * U32 * torch.einsum('bhwo,oc->bhwc', g.abs(), w.abs())
    if old is not None:
        tol, _ = _store(dx, tol, dtype)                # a kernel may round the new term before it reads the old one back
        dx = dx + old
        tol = tol + U32 * dx.abs()
    tol, _ = _store(dx, tol, dtype)
    gw = torch.einsum('bhwo,bhwc->oc', g, x)
    tw = N * U32 * torch.einsum('bhwo,bhwc->oc', g.abs(), x.abs())
    gb = g.sum((0, 1, 2))
    return dict(dx=dict(exact=dx, tol=tol), gw=dict(exact=gw, tol=tw), gb=dict(exact=gb, tol=N * U32 * g.abs().sum((0, 1, 2))))


def head_parts(npix):
    """salt_head1x1_bwd_parts: parts of at most 64 pixels, at most 1024 of them (longer ones then), equal lengths."""
    parts = min(max(cdiv(npix, 64), 1), 1024)
    return cdiv(npix, cdiv(npix, parts))


# ---------------------------------------------------------------- the stem's index maps
def s2d_ref(x):
    """x [B,Cin,H,W] fp32 -> z [B,H/2,W/2,16] fp32: z[b, Y, X, (ph 2 + pw) Cin + c] = x[b, c, 2 Y + ph, 2 X + pw], the rest zero."""
    B, Cin, H, W = x.shape
    z = torch.zeros(B, H // 2, W // 2, 16, dtype=x.dtype)
    for ph in range(2):
        for pw in range(2):
            for c in range(Cin):
                z[..., (ph * 2 + pw) * Cin + c] = x[:, c, ph::2, pw::2]
    return z


def stem_taps(K):
    """[(dh, dw)] of the ((K + 1) / 2)^2-tap stride-1 convolution over the space-to-depth image, in packed order."""
    T, half = (K + 1) // 2, (K + 1) // 4
    return [(i - half, j - half) for i in range(T) for j in range(T)]


def pack_stem_ref(w, kc=16):
    """w [Cout,Cin,K,K] -> [T T][Cout][kc] of w's dtype: tap (dh, dw), channel (ph 2 + pw) Cin + c holds W[n][c][2 dh + ph + K/2][2 dw + pw + K/2]
    where that lies inside the kernel, else zero."""
    Cout, Cin, K, _ = w.shape
    taps = stem_taps(K)
    out = torch.zeros(len(taps), Cout, kc, dtype=w.dtype)
    for t, (dh, dw) in enumerate(taps):
        for ph in range(2):
            for pw in range(2):
                kh, kw = 2 * dh + ph + K // 2, 2 * dw + pw + K // 2
                if 0 <= kh < K and 0 <= kw < K:
                    for c in range(Cin):
                        out[t, :, (ph * 2 + pw) * Cin + c] = w[:, c, kh, kw]
    return out


def stem_unfold_ref(g16, Cin, K):
    """g16 [Cout,16,T,T] -> [Cout,Cin,K,K]: the adjoint of pack_stem_ref (every kernel element lies in exactly one (tap, phase))."""
    Cout, T, half = g16.shape[0], (K + 1) // 2, (K + 1) // 4
    out = torch.zeros(Cout, Cin, K, K, dtype=g16.dtype)
    for kh in range(K):
        for kw in range(K):
            eh, ew = kh - K // 2, kw - K // 2
            ph, pw = eh % 2, ew % 2                    # Python's %: 0 or 1 for negative offsets too
            dh, dw = (eh - ph) // 2, (ew - pw) // 2
            for c in range(Cin):
                out[:, c, kh, kw] = g16[:, (ph * 2 + pw) * Cin + c, dh + half, dw + half]
    return out


# ---------------------------------------------------------------- C-ABI
def _abi():
    import salt_amd  # noqa: F401
    from salt_amd import _abi as A
    return A


def view(ptr, B, H, W, C, cs):
    from salt_amd.engine import shaped_view
    return shaped_view(ptr, B, H, W, C, cs)


def first_args(dtype, x, shape, w, K, stride, pad, y, **kw):
    """x, w and the optional bias / scale / shift / stats / stats_cnt: device pointers (any number for the host-only queries)."""
    A = _abi()
    B, Cin, H, W = shape
    return A.fill(A.STRUCTS['salt_conv_first_args'](), dtype=DT[dtype], x=x, B=B, Cin=Cin, H=H, W=W, w=w, K=K, stride=stride, pad=pad, y=y, **kw)


def first_wgrad_args(dtype, x, shape, K, stride, pad, dy, partials, nparts, grad, accumulate=0):
    A = _abi()
    B, Cin, H, W = shape
    return A.fill(A.STRUCTS['salt_conv_first_wgrad_args'](), dtype=DT[dtype], x=x, B=B, Cin=Cin, H=H, W=W, K=K, stride=stride, pad=pad, dy=dy,
                  partials=partials, nparts=nparts, grad=grad, accumulate=accumulate)


def head_args(dtype, x, w, bias, Cout, y_nchw=None, y=None):
    A = _abi()
    S = A.fill(A.STRUCTS['salt_head1x1_args'](), dtype=DT[dtype], x=x, w=w, bias=bias, Cout=Cout, y_nchw=y_nchw)
    if y is not None:
        S.y = y
    return S


def head_bwd_args(dtype, x, w, Cout, dy_nchw, dx, accumulate, partials, nparts, gw, gb):
    A = _abi()
    return A.fill(A.STRUCTS['salt_head1x1_bwd_args'](), dtype=DT[dtype], x=x, w=w, Cout=Cout, dy_nchw=dy_nchw, dx=dx, accumulate=accumulate,
                  partials=partials, nparts=nparts, gw=gw, gb=gb)


def query(name, S):
    """A host-only entry point: int salt_X(const salt_X_args*)."""
    return getattr(_abi().lib, name)(ctypes.byref(S))


def call(name, S):
    """Launch and wait -> the return code (0, a SALT_E_* code or a hipError_t)."""
    rc = getattr(_abi().lib, name)(ctypes.byref(S), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc


def run(name, S):
    rc = call(name, S)
    assert rc == 0, '%s failed (%d): %s' % (name, rc, last_error())


# ---------------------------------------------------------------- guarded flat buffers
class Guarded:
    """n elements that a launch must write (NaN, or `values`) followed by `tail` elements that must keep GUARD's bit pattern."""

    def __init__(self, n, dtype, device, values=None, tail=64):
        self.n = n
        self.buf = guard_fill(torch.empty(n + tail, dtype=dtype, device=device))
        self.buf[:n] = float('nan') if values is None else values.reshape(-1).to(dtype).to(device)

    def ptr(self):
        return self.buf.data_ptr()

    def get(self, what=''):
        """The n elements on the CPU; asserts the tail first."""
        out = self.buf.cpu()
        assert bool((bits(out[self.n:]) == GUARD[out.dtype]).all()), '%s: elements past the end of the buffer were overwritten' % what
        return out[:self.n]


def worst(got, ref):
    """ratio() for a dict(exact, tol) of any shape."""
    return ratio(got.reshape(ref['exact'].shape), ref)


# ================================================================ the case tables and operand builders of test_gpu_small_abi.py /
# test_small_reference_cpu.py (host only)
DTYPES = ('f32', 'bf16')
FAKE = 1 << 24                            # a 16-byte aligned made-up address for the host-only queries


def _vec(C, seed, kind='bias'):
    """bf16-representable per-channel vectors; scale in [0.5, 2] with both signs."""
    g = torch.Generator().manual_seed(seed)
    if kind == 'scale':
        v = (0.5 + 1.5 * torch.rand(C, generator=g)) * torch.where(torch.rand(C, generator=g) < 0.25, -1.0, 1.0)
    else:
        v = torch.randn(C, generator=g)
    return v.bfloat16().double()


def _ids(cases):
    return [pytest.param(c, id=c['name']) for c in cases]


# ---------------------------------------------------------------- salt_conv_first
def first_case(name, dtype, Cin, H, W, K, s, p, Cout, B=2, yv=None, **kw):
    c = dict(name='%s-%s' % (dtype, name), dtype=dtype, B=B, Cin=Cin, H=H, W=W, K=K, s=s, p=p, Cout=Cout, yv=yv or (0, Cout), bias=False,
             scale=False, relu=False, stats=False, vec=None)
    c.update(kw)
    return c


FIRST_CASES = []
for _dt in DTYPES:
    _ve = VE[_dt]
    FIRST_CASES += [
        # the ResNet stem on 2 x 2 ragged tiles (17 x 19 outputs): whole 16-channel blocks, a ragged second block, a single ragged block
        first_case('7x7s2-cout64', _dt, 3, 34, 38, 7, 2, 3, 64, vec=True),
        first_case('7x7s2-cout24', _dt, 3, 34, 38, 7, 2, 3, 24, vec=True),           # (block 0 is whole: vector stores; block 1 scalar)
        first_case('7x7s2-cout10', _dt, 3, 34, 38, 7, 2, 3, 10, vec=False),
        # the remaining K / stride / pad / Cin forms
        first_case('3x3s1p1-cin1', _dt, 1, 19, 21, 3, 1, 1, 16, vec=True),
        first_case('3x3s1p1-cin4', _dt, 4, 19, 21, 3, 1, 1, 10, vec=False),
        first_case('1x1s1', _dt, 2, 17, 19, 1, 1, 0, 16, vec=True),
        first_case('1x1s2', _dt, 2, 33, 37, 1, 2, 0, 16, vec=True),
        first_case('5x5s2p2', _dt, 3, 33, 37, 5, 2, 2, 24, vec=True),
        first_case('3x3s1p0', _dt, 2, 19, 21, 3, 1, 0, 16, vec=True),
        # y as a channel slice of a wider buffer: the three terms of the vector-store predicate, one at a time
        first_case('y-slice-aligned', _dt, 3, 34, 38, 7, 2, 3, 32, yv=(16, 56), vec=True),
        first_case('y-slice-cs-odd', _dt, 3, 34, 38, 7, 2, 3, 32, yv=(0, 37), vec=False),
        first_case('y-slice-misaligned', _dt, 3, 34, 38, 7, 2, 3, 32, yv=(2, 40), vec=False),
        # each epilogue combination on its own (none: the cases above), on the ragged second block
        first_case('bias', _dt, 3, 34, 38, 7, 2, 3, 24, bias=True, vec=True),
        first_case('bias-cout10', _dt, 3, 34, 38, 7, 2, 3, 10, bias=True, vec=False),
        first_case('scale-shift-relu', _dt, 3, 34, 38, 7, 2, 3, 24, scale=True, relu=True, vec=True),
        first_case('bias-scale-shift', _dt, 3, 34, 38, 7, 2, 3, 24, bias=True, scale=True, vec=True),
        # tile statistics on ragged tiles: counts 256, 48, 16 and 3 per image
        first_case('stats', _dt, 3, 34, 38, 7, 2, 3, 24, stats=True, vec=True),
        first_case('stats-epilogue', _dt, 3, 34, 38, 7, 2, 3, 24, bias=True, scale=True, relu=True, stats=True, vec=True),
        first_case('stats-3x3', _dt, 1, 19, 21, 3, 1, 1, 10, bias=True, stats=True, vec=False, B=3),
    ]


def first_vec(c):
    """conv_first_kernel's vector-store predicate for block 0 of the case, from the view alone."""
    es = 4 if c['dtype'] == 'f32' else 2
    c0, cs = c['yv']
    return c['Cout'] >= 16 and cs % VE[c['dtype']] == 0 and (c0 * es) % 16 == 0


def first_build(c):
    x = mk(c['B'], c['Cin'], c['H'], c['W'], 11)
    w = master_weight(c['Cout'], c['Cin'], c['K'], c['K'], c['Cin'], c['K'] * c['K'], 12)
    o = dict(x=x, w=w, bias=_vec(c['Cout'], 3) if c['bias'] else None, scale=_vec(c['Cout'], 4, 'scale') if c['scale'] else None,
             shift=_vec(c['Cout'], 5) if c['scale'] else None)
    o['ref'] = conv_first_ref(x, w, c['s'], c['p'], c['dtype'], o['bias'], o['scale'], o['shift'], c['relu'])
    return o


# ---------------------------------------------------------------- salt_conv_first_wgrad
MFMA = 0


def wg_case(name, Cin, K, Cout, kid, B=1, H=None, W=None, s=1, p=None, OH=17, OW=19, dyv=None, rc=0, per=None, wrong_nparts=False):
    """Default geometry: one image whose output is 17 x 19 (2 x 2 ragged tiles).  kid: salt_conv_first_wgrad_kernel_id, or -1 for a
    refusal with return code rc."""
    p = K // 2 if p is None else p
    if H is None:
        H, W = (OH - 1) * s + K - 2 * p, (OW - 1) * s + K - 2 * p
    assert first_geom(H, W, K, s, p) == (OH, OW), name
    return dict(name=name, B=B, Cin=Cin, H=H, W=W, K=K, s=s, p=p, Cout=Cout, kid=kid, OH=OH, OW=OW, dyv=dyv or (0, Cout), rc=rc, per=per,
                wrong_nparts=wrong_nparts)


WGRAD_CASES = [
    wg_case('mfma-cin1-k3-cout16', 1, 3, 16, MFMA),
    wg_case('mfma-cin1-k3-cout32', 1, 3, 32, MFMA),                          # two cb passes
    wg_case('mfma-cin1-k4-cout16', 1, 4, 16, MFMA, p=1),                     # K K Cin exactly 16
    wg_case('mfma-cin4-k2-cout48', 4, 2, 48, MFMA, p=0),
    wg_case('mfma-cin3-k1-cout16', 3, 1, 16, MFMA),                          # 3 taps on, 13 off
    wg_case('per1-cout10-cin1-k3', 1, 3, 10, 1, per=1),
    wg_case('per4-cout24-cin3-k3', 3, 3, 24, 4, per=3),
    wg_case('per12-cout64-cin1-k5', 1, 5, 64, 12, per=7),
    wg_case('per40-cout64-cin3-k7', 3, 7, 64, 40, per=37),
    wg_case('per40-cout50-cin4-k7', 4, 7, 50, 40, per=40),                   # per exactly MAXKK
    # one group of threads (Cout > 128).  256 pixels x Cout floats of dy live in LDS: 160 KiB end at Cout 159, so Cout 200 and 256 (one
    # group with 56 / no idle threads) are refused with SALT_E_LDS, and 144 / 128 are the widest forms that run
    wg_case('one-group-cout200', 4, 3, 200, -1, rc=-3),
    wg_case('one-group-cout256', 4, 3, 256, -1, rc=-3),
    wg_case('one-group-cout144-112-idle', 4, 3, 144, 40, per=36),
    wg_case('two-groups-cout128-none-idle', 4, 3, 128, 40, per=18),
    wg_case('cout257', 4, 3, 257, -1, rc=-2),
    wg_case('per49-cout64-cin4-k7', 4, 7, 64, -1, rc=-2),
    # the reduction of the partials: narrow below 64 parts or above 4096 outputs, wide otherwise
    wg_case('nparts63-narrow', 1, 3, 10, 1, B=7, OH=33, OW=35, per=1),
    wg_case('nparts64-wide', 1, 3, 10, 1 | WIDE, B=4, OH=49, OW=51, per=1),
    wg_case('nparts64-wide-mfma', 1, 3, 16, MFMA | WIDE, B=4, OH=49, OW=51),
    wg_case('nparts320-wide', 1, 3, 10, 1 | WIDE, B=20, OH=49, OW=51, per=1),  # thread t adds parts t and t + 256
    wg_case('nparts64-n9408-narrow', 3, 7, 64, 40, B=4, OH=49, OW=51, per=37),
    wg_case('stride2-mfma', 1, 3, 16, MFMA, s=2, H=34, W=38),
    wg_case('stride2-per40', 3, 7, 64, 40, s=2, H=34, W=38, per=37),
    wg_case('dy-slice', 3, 3, 24, 4, dyv=(8, 40), per=3),
    wg_case('dy-slice-mfma', 1, 3, 32, MFMA, dyv=(3, 37)),
    wg_case('wrong-nparts', 1, 3, 16, -1, rc=-1, wrong_nparts=True),
]


def wg_nparts(c):
    return c['B'] * cdiv(c['OH'], 16) * cdiv(c['OW'], 16)


def wg_plan(c, dtype, x=FAKE, dy=FAKE, partials=FAKE, grad=FAKE, acc=0):
    es = 4 if dtype == 'f32' else 2
    dyv = view(dy + (c['dyv'][0] * es if dy == FAKE else 0), c['B'], c['OH'], c['OW'], c['Cout'], c['dyv'][1])
    return first_wgrad_args(dtype, x, (c['B'], c['Cin'], c['H'], c['W']), c['K'], c['s'], c['p'], dyv, partials,
                            wg_nparts(c) + int(c['wrong_nparts']), grad, acc)


def wg_build(c, acc):
    x = mk(c['B'], c['Cin'], c['H'], c['W'], 21)
    dy = mk(c['B'], c['Cout'], c['OH'], c['OW'], 22).permute(0, 2, 3, 1).contiguous()
    old = mk(c['Cout'], c['Cin'], c['K'], c['K'], 23).double() if acc else None
    o = dict(x=x, dy=dy, old=old)
    if c['kid'] >= 0:
        o['ref'] = conv_first_wgrad_ref(x, dy, c['K'], c['s'], c['p'], old)
    return o


# ---------------------------------------------------------------- salt_head1x1
def head_case(name, dtype, C, Cout, kid, B=2, H=7, W=9, xv=None):
    return dict(name='%s-%s' % (dtype, name), dtype=dtype, B=B, H=H, W=W, C=C, Cout=Cout, kid=kid, xv=xv or (0, C))


HEAD_CASES = []
for _dt in DTYPES:
    _ve = VE[_dt]
    HEAD_CASES += [
        head_case('co2-8x8-shift', _dt, 8 * _ve, 2, HEAD_VEC_CO2, H=8, W=8),              # H W a power of two: no division per pixel
        head_case('co2-7x9-divide', _dt, 8 * _ve, 2, HEAD_VEC_CO2),
        head_case('co2-units-below-256', _dt, 8 * _ve, 2, HEAD_VEC_CO2, B=1, H=3, W=5),   # the second pixel in flight is past the end
        head_case('co2-cpv1', _dt, _ve, 2, HEAD_VEC_CO2),
        head_case('co2-cpv64', _dt, 64 * _ve, 2, HEAD_VEC_CO2),
        head_case('co2-x-slice', _dt, 8 * _ve, 2, HEAD_VEC_CO2, xv=(2 * _ve, 12 * _ve)),
        head_case('vec-cout1', _dt, 8 * _ve, 1, HEAD_VEC),
        head_case('vec-cout3', _dt, 8 * _ve, 3, HEAD_VEC),
        head_case('vec-cout4', _dt, 8 * _ve, 4, HEAD_VEC, H=8, W=8),
        head_case('vec-cpv1-cout3', _dt, _ve, 3, HEAD_VEC),
        head_case('vec-cpv64-cout4', _dt, 64 * _ve, 4, HEAD_VEC),
        head_case('scalar-c10-cout1', _dt, 10, 1, HEAD_SCALAR),
        head_case('scalar-c10-cout2', _dt, 10, 2, HEAD_SCALAR),
        head_case('scalar-c10-cout3', _dt, 10, 3, HEAD_SCALAR),
        head_case('scalar-c10-cout4', _dt, 10, 4, HEAD_SCALAR),
        head_case('scalar-cs-odd', _dt, 8 * _ve, 2, HEAD_SCALAR, xv=(0, 8 * _ve + 3)),
        head_case('scalar-misaligned', _dt, 8 * _ve, 2, HEAD_SCALAR, xv=(2, 10 * _ve)),
    ]
HEAD_CASES += [
    head_case('scalar-c24-cpv3', 'bf16', 24, 2, HEAD_SCALAR),                              # whole pieces, but not a power of two of them
    head_case('scalar-c12-cpv3', 'f32', 12, 3, HEAD_SCALAR),
    head_case('scalar-c512-cpv128', 'f32', 512, 2, HEAD_SCALAR),                           # more than 64 pieces
    head_case('scalar-c1024-cpv128', 'bf16', 1024, 4, HEAD_SCALAR),
]
# above the 4096-block grid cap: 16640 pixels x 64 pieces = 4160 blocks' worth of units (17 MB of input)
HEAD_GRID_CAP = head_case('co2-grid-cap', 'bf16', 512, 2, HEAD_VEC_CO2, B=1, H=128, W=130)


def head_plan(c, out, x=FAKE, w=FAKE, bias=None, y=FAKE, gap=3):
    es = 4 if c['dtype'] == 'f32' else 2
    xv = view(x + (c['xv'][0] * es if x == FAKE else 0), c['B'], c['H'], c['W'], c['C'], c['xv'][1])
    if out == 'nchw':
        return head_args(c['dtype'], xv, w, bias, c['Cout'], y_nchw=y)
    return head_args(c['dtype'], xv, w, bias, c['Cout'], y=view(y, c['B'], c['H'], c['W'], c['Cout'], c['Cout'] + 2 * gap))


def head_build(c, seed=31):
    x = mk(c['B'], c['C'], c['H'], c['W'], seed).permute(0, 2, 3, 1).contiguous()
    w = master_weight(c['Cout'], c['C'], 1, 1, c['C'], 1, seed + 1).reshape(c['Cout'], c['C'])
    return dict(x=x, w=w, bias=_vec(c['Cout'], seed + 2))


# ---------------------------------------------------------------- salt_head1x1_bwd
def hb_case(name, dtype, C, Cout, kid, B=1, H=4, W=5, xv=None, dxv=None):
    return dict(name='%s-%s' % (dtype, name), dtype=dtype, B=B, H=H, W=W, C=C, Cout=Cout, kid=kid, xv=xv or (0, C), dxv=dxv or (0, C))


HEAD_BWD_CASES = []
for _dt in DTYPES:
    _ve = VE[_dt]
    HEAD_BWD_CASES += [
        hb_case('vec-cpv1', _dt, _ve, 2, HEAD_VEC, B=2, H=7, W=9),
        hb_case('vec-cpv3-r85', _dt, 3 * _ve, 3, HEAD_VEC, B=2, H=20, W=17),                 # one idle thread; 680 pixels in 11 parts of 62
        hb_case('vec-cpv256-r1', _dt, 256 * _ve, 1, HEAD_VEC, H=3, W=5),
        # R <= 21 rows of threads: a part of at most 64 pixels reaches the fourth pixel in flight (126 pixels: 2 parts of 63)
        hb_case('vec-cpv16-r16', _dt, 16 * _ve, 4, HEAD_VEC, B=2, H=7, W=9),
        hb_case('vec-cpv64-r4', _dt, 64 * _ve, 3, HEAD_VEC, B=2, H=7, W=9),
        hb_case('vec-cpv8-ragged-part', _dt, 8 * _ve, 4, HEAD_VEC),                          # 20 pixels: no multiple of 4 R = 128
        hb_case('vec-slices', _dt, 8 * _ve, 2, HEAD_VEC, xv=(_ve, 10 * _ve), dxv=(2 * _ve, 11 * _ve)),
        hb_case('vec-129-pixels', _dt, 8 * _ve, 2, HEAD_VEC, H=3, W=43),                     # 64 k + 1 pixels: 3 parts of 43
        hb_case('vec-260x260', _dt, _ve, 2, HEAD_VEC, H=260, W=260),                         # the cap: 1009 parts of 67 pixels
        hb_case('scalar-c10', _dt, 10, 3, HEAD_SCALAR, B=2, H=7, W=9),
        hb_case('scalar-dx-cs-odd', _dt, 8 * _ve, 2, HEAD_SCALAR, dxv=(0, 8 * _ve + 3)),
        hb_case('scalar-x-misaligned', _dt, 8 * _ve, 4, HEAD_SCALAR, xv=(2, 10 * _ve)),
        hb_case('scalar-260x260', _dt, 10, 1, HEAD_SCALAR, H=260, W=260),
    ]
HEAD_BWD_CASES += [
    hb_case('scalar-c300-two-passes', 'bf16', 300, 2, HEAD_SCALAR, B=2, H=7, W=9),           # cn 256, then 44 (R = 5)
    hb_case('scalar-c1028-cpv257', 'f32', 1028, 3, HEAD_SCALAR),                             # whole pieces, one too many
    hb_case('scalar-c302-two-passes', 'f32', 302, 4, HEAD_SCALAR),                           # cn 256, then 46
]


def hb_plan(c, acc, gb, x=FAKE, dx=FAKE + (1 << 22), nparts=None):
    es = 4 if c['dtype'] == 'f32' else 2
    f = (lambda p, v: p + v[0] * es) if x == FAKE else (lambda p, v: p)
    xv = view(f(x, c['xv']), c['B'], c['H'], c['W'], c['C'], c['xv'][1])
    dxv = view(f(dx, c['dxv']), c['B'], c['H'], c['W'], c['C'], c['dxv'][1])
    S = head_bwd_args(c['dtype'], xv, FAKE, c['Cout'], FAKE, dxv, acc, FAKE, 0, FAKE, FAKE if gb else None)
    S.nparts = query('salt_head1x1_bwd_parts', S) if nparts is None else nparts
    return S


def hb_build(c, acc):
    x = mk(c['B'], c['C'], c['H'], c['W'], 41).permute(0, 2, 3, 1).contiguous()
    w = master_weight(c['Cout'], c['C'], 1, 1, c['Cout'], 1, 42).reshape(c['Cout'], c['C'])
    dy = mk(c['B'], c['Cout'], c['H'], c['W'], 43)
    old = mk(c['B'], c['C'], c['H'], c['W'], 44).permute(0, 2, 3, 1).contiguous() if acc else None
    ref = head_bwd_ref(x.double(), w.double(), dy.double(), c['dtype'], old.double() if acc else None)
    return dict(x=x, w=w, dy=dy, old=old, ref=ref)


def _arbitrary(shape, seed):
    """fp32 values with full mantissas (no two alike in practice), so that bf16 outputs exercise the rounding."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * (1.0 + torch.rand(*shape, generator=g))
