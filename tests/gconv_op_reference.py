"""Float64 reference of the grouped 3x3 convolution (include/saltnet.h: salt_gconv / salt_gconv_dgrad / salt_gconv_wgrad), written from
the definition: a loop over the groups and the nine taps with zero-masked gathers, NHWC, together with A = sum |x| |w| of the same terms
for the per-element bound.  test_seresnext_cpu.py pins it against F.conv2d(groups=32) and autograd in double; test_gpu_seresnext.py
holds the kernels to it.

Operands (make_case) are normal values that bf16 holds exactly, in both dtypes, so every product x w has at most 16 significant bits and
is exact in fp32: a kernel differs from the float64 sum only by the order and rounding of its K additions.  The bound per element is
tests/conv_abi.py's, restated for this operator (derived, not tuned to a kernel):
  * accumulation: tol = K 2^-23 A, K = 9 Cg terms for the forward and the data gradient, K = the number of summed pixels B OH OW for the
    weight gradient (each of the K - 1 fp32 additions is off by at most one ulp of a partial sum that A bounds);
  * eval epilogue in fp32: tol |scale| + 4 * 2^-23 * (largest intermediate of the element);
  * bf16 storage: + 2^-8 (|value| + tol) per storage rounding - one for a plain store, two with accumulate (the stored old value is
    itself exact; the two roundings are the kernel's own freedom: sum then round, or round then sum then round).
No element is excluded."""
import math

import torch

from conv_abi import ratio_strict as ratio, store_tol as _store          # noqa: F401  (ratio is the tests' entry point)

F64 = torch.float64
GROUPS = 32
U32, UBF = 2.0 ** -23, 2.0 ** -8

# (B, H, W, width, stride): a map smaller than a tile; odd, non-square, B = 3; several tiles with ragged edges on both axes; stride 2;
# stride 2 on an odd map; Cg = 16; Cg = 16 with stride 2; only the centre tap in range; Cg = 32; Cg = 32 with stride 2
SHAPES = [(2, 4, 4, 128, 1), (3, 5, 7, 128, 1), (1, 34, 18, 128, 1), (2, 6, 10, 256, 2), (2, 7, 9, 256, 2), (2, 8, 8, 512, 1),
          (1, 16, 16, 512, 2), (1, 1, 1, 1024, 1), (2, 2, 2, 1024, 1), (2, 4, 4, 1024, 2)]


def out_size(n, stride):
    return (n + 2 - 3) // stride + 1


def _bf(t):
    return t.bfloat16().double()


def make_case(B, H, W, C, stride, seed):
    """x, dy, old values (for accumulate), w [C][Cg][3][3], scale / shift: float64 tensors holding bf16-representable values."""
    g = torch.Generator().manual_seed(seed)
    Cg = C // GROUPS
    OH, OW = out_size(H, stride), out_size(W, stride)
    rn = lambda *s: torch.randn(*s, generator=g)
    return dict(x=_bf(rn(B, H, W, C)), dy=_bf(rn(B, OH, OW, C)), dx_old=_bf(rn(B, H, W, C)), gw_old=_bf(rn(C, Cg, 3, 3)),
                w=_bf(rn(C, Cg, 3, 3) * math.sqrt(2.0 / (9 * Cg))), scale=_bf(0.5 + torch.rand(C, generator=g)) * torch.where(torch.rand(C, generator=g) < 0.2, -1.0, 1.0).double(),
                shift=_bf(0.3 * rn(C)), stride=stride)


def _gather(t, k, stride, n_out, axis):
    """rows (axis 1) or columns (axis 2) o stride + k - 1 of t for o < n_out, zero where that lies outside t"""
    n = t.shape[axis]
    idx = torch.arange(n_out) * stride + k - 1
    ok = ((idx >= 0) & (idx < n)).double()
    g = t.index_select(axis, idx.clamp(0, n - 1))
    shape = [1] * t.dim()
    shape[axis] = n_out
    return g * ok.reshape(shape)


def gconv(x, w, stride):
    """x [B,H,W,C], w [C][Cg][3][3] float64 -> (v, A) [B,OH,OW,C]"""
    B, H, W, C = x.shape
    Cg = C // GROUPS
    OH, OW = out_size(H, stride), out_size(W, stride)
    v = torch.zeros(B, OH, OW, C, dtype=F64)
    A = torch.zeros_like(v)
    for g in range(GROUPS):
        xs = x[..., g * Cg:(g + 1) * Cg]
        for kh in range(3):
            rows = _gather(xs, kh, stride, OH, 1)
            for kw in range(3):
                t = _gather(rows, kw, stride, OW, 2)                       # [B,OH,OW,Cg]
                wk = w[g * Cg:(g + 1) * Cg, :, kh, kw]                       # [n][k]
                v[..., g * Cg:(g + 1) * Cg] += torch.einsum('bhwk,nk->bhwn', t, wk)
                A[..., g * Cg:(g + 1) * Cg] += torch.einsum('bhwk,nk->bhwn', t.abs(), wk.abs())
    return v, A


def gconv_dgrad(dy, w, stride, H, W):
    """dy [B,OH,OW,C] -> (dx, A) [B,H,W,C]: the scatter of the definition (each output pixel adds to the inputs it read)"""
    B, OH, OW, C = dy.shape
    Cg = C // GROUPS
    dx = torch.zeros(B, (OH - 1) * stride + 3, (OW - 1) * stride + 3, C, dtype=F64)      # the grid padded by 1: every tap of every output pixel
    A = torch.zeros_like(dx)
    for g in range(GROUPS):
        ds = dy[..., g * Cg:(g + 1) * Cg]
        for kh in range(3):
            for kw in range(3):
                wk = w[g * Cg:(g + 1) * Cg, :, kh, kw]                       # [n][k]
                sl = (slice(None), slice(kh, kh + (OH - 1) * stride + 1, stride), slice(kw, kw + (OW - 1) * stride + 1, stride),
                      slice(g * Cg, (g + 1) * Cg))
                dx[sl] += torch.einsum('bhwn,nk->bhwk', ds, wk)
                A[sl] += torch.einsum('bhwn,nk->bhwk', ds.abs(), wk.abs())
    # padded coordinate p = input coordinate + 1; rows / columns the padded grid does not reach (stride 2, even map) got nothing
    out, outA = torch.zeros(B, H, W, C, dtype=F64), torch.zeros(B, H, W, C, dtype=F64)
    h, w_ = min(H, dx.shape[1] - 1), min(W, dx.shape[2] - 1)
    out[:, :h, :w_] = dx[:, 1:1 + h, 1:1 + w_]
    outA[:, :h, :w_] = A[:, 1:1 + h, 1:1 + w_]
    return out, outA


def gconv_wgrad(x, dy, stride):
    """-> (gw, A) [C][Cg][3][3]"""
    B, H, W, C = x.shape
    Cg = C // GROUPS
    OH, OW = dy.shape[1], dy.shape[2]
    gw = torch.zeros(C, Cg, 3, 3, dtype=F64)
    A = torch.zeros_like(gw)
    for g in range(GROUPS):
        xs, ds = x[..., g * Cg:(g + 1) * Cg], dy[..., g * Cg:(g + 1) * Cg]
        for kh in range(3):
            rows = _gather(xs, kh, stride, OH, 1)
            for kw in range(3):
                t = _gather(rows, kw, stride, OW, 2)
                gw[g * Cg:(g + 1) * Cg, :, kh, kw] = torch.einsum('bhwn,bhwk->nk', ds, t)
                A[g * Cg:(g + 1) * Cg, :, kh, kw] = torch.einsum('bhwn,bhwk->nk', ds.abs(), t.abs())
    return gw, A


# ---------------------------------------------------------------- bounds
def forward_ref(c, dtype, eval_epilogue, relu):
    """-> dict(exact, tol): eval_epilogue: relu?(v scale + shift); else the raw output"""
    v, A = gconv(c['x'], c['w'], c['stride'])
    K = 9 * (c['x'].shape[3] // GROUPS)
    tol = K * U32 * A
    e = v
    if eval_epilogue:
        e = v * c['scale']
        big = torch.maximum(v.abs(), e.abs())
        e = e + c['shift']
        big = torch.maximum(big, e.abs())
        tol = tol * c['scale'].abs() + 4 * U32 * big
    if relu:
        e = e.clamp_min(0)
    return dict(exact=e, tol=_store(e, tol, dtype))


def dgrad_ref(c, dtype, accumulate):
    dx, A = gconv_dgrad(c['dy'], c['w'], c['stride'], c['x'].shape[1], c['x'].shape[2])
    K = 9 * (c['x'].shape[3] // GROUPS)
    tol = K * U32 * A
    e = dx
    if accumulate:
        tol = _store(e, tol, dtype)                                          # the kernel may round before it adds
        e = e + c['dx_old']
        tol = tol + U32 * e.abs()
    return dict(exact=e, tol=_store(e, tol, dtype))


def wgrad_ref(c, accumulate):
    gw, A = gconv_wgrad(c['x'], c['dy'], c['stride'])
    K = c['dy'].shape[0] * c['dy'].shape[1] * c['dy'].shape[2]
    tol = K * U32 * A
    e = gw
    if accumulate:
        e = e + c['gw_old']
        tol = tol + U32 * e.abs()
    return dict(exact=e, tol=tol)
