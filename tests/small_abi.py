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
