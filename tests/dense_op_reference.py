"""Float64 references of the pre-activated 1x1 convolution (include/saltnet.h: salt_dense_conv / salt_dense_conv_dgrad /
salt_dense_conv_wgrad), written from the definitions, NHWC, each with A = sum |a| |w| of the same terms for the per-element bound.
test_densenet_cpu.py pins them against F.batch_norm(training=True) -> ReLU -> 1x1 F.conv2d and autograd in double;
test_gpu_densenet.py holds the kernels to them.

The transformed operand is reproduced EXACTLY (transform): t = x in_scale + in_shift as a float64 multiply-add rounded once to fp32 (the
operands of make_case are bf16-representable, so the float64 value is the exact one and the rounding is the kernel's fmaf), ReLU, one
rounding to the storage dtype; the mask is [t > 0] of the same t.  So kernel and reference contract the same numbers under the same
mask and differ only by the order and rounding of the additions.  The bound per element is tests/gconv_op_reference.py's, restated
(derived, not tuned to a kernel; u = 2^-23):
  * accumulation: tol = K u A.  K = Cin for the forward, the number of summed pixels B H W for the weight gradient.  For the data
    gradient the issue sets K = Cin while the sum has Cout terms: the SMALLER of the two is used, which asks no less than either.
  * eval epilogue in fp32: tol |scale| + 4 u (largest intermediate of the element);
  * bf16 storage: + 2^-8 (|value| + tol) per storage rounding - one for a plain store, two with accumulate.
BatchNorm backward inside the data gradient (dgrad_ref).  With g = m G, G the contraction (|dG| <= tolG = K u A_G, masked elements are 0
on both sides), xhat = (x - mean) invstd computed by the kernel as one fp32 subtraction and one fp32 product (|dxhat| <= 2 u |xhat|):
  * s1 = sum_p g:       tol_s1 = sum_p tolG m + N u sum_p |g|                     (N = B H W additions in any order, each off by at
    most u of a partial sum that sum |g| bounds - conv_abi.moments' argument)
  * s2 = sum_p g xhat:  tol_s2 = sum_p (tolG m |xhat| + |g| 2 u |xhat| + u |g xhat|) + N u sum_p |g xhat|
  * dbeta / dgamma are s1 / s2 rounded once more: + u |s|.
  * t1 = s1 / N (the reciprocal and the product round):  d1 = tol_s1 / N + 2 u |s1| / N
  * t2 = xhat s2 / N:  d2 = |xhat| (tol_s2 / N + 2 u |s2| / N) + 2 u |xhat| |s2| / N + u |xhat s2 / N|
  * inner = (g - t1) - t2:  tol_i = tolG m + d1 + d2 + 2 u (|g| + |t1| + |t2|)
  * dx = k inner, k = gamma invstd rounded:  tol = |k| tol_i + 2 u |k inner|, then the storage / accumulate terms above.
No element is excluded."""
import math

import torch

from conv_abi import ratio_strict as ratio, store_tol as _store          # noqa: F401  (ratio is the tests' entry point)

F64 = torch.float64
U32, UBF = 2.0 ** -23, 2.0 ** -8

# (B, H, W, Cin, Cout): smaller than a tile; odd, non-square, an odd number of K chunks; several tiles, ragged on both axes; the longest
# prefix of depth 121; the longest of the contract's growth-32 family; transition 1; transition 3; Cout not a power of two
SHAPES = [(2, 3, 3, 64, 128), (3, 5, 7, 96, 128), (1, 34, 18, 160, 128), (1, 8, 8, 992, 128), (1, 4, 4, 1888, 128), (2, 6, 10, 256, 128),
          (1, 4, 4, 1024, 512), (1, 3, 3, 1280, 640)]


def _bf(t):
    return t.bfloat16().double()


def make_case(B, H, W, Cin, Cout, seed):
    """float64 tensors holding bf16-representable values.  20 % of in_scale are negative; in_shift = 0.3 N(0,1) against |in_scale| in
    [0.5, 1.5) and x ~ N(0,1) masks about half of the elements (test_densenet_cpu.py asserts 30 .. 70 %)."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    sign = lambda n: torch.where(torch.rand(n, generator=g) < 0.2, -1.0, 1.0).double()
    return dict(x=_bf(rn(B, H, W, Cin)), dy=_bf(rn(B, H, W, Cout)), dx_old=_bf(rn(B, H, W, Cin)), gw_old=_bf(rn(Cout, Cin)),
                w=_bf(rn(Cout, Cin) * math.sqrt(2.0 / Cin)), in_scale=_bf(0.5 + torch.rand(Cin, generator=g)) * sign(Cin), in_shift=_bf(0.3 * rn(Cin)),
                scale=_bf(0.5 + torch.rand(Cout, generator=g)) * sign(Cout), shift=_bf(0.3 * rn(Cout)),
                mean=_bf(0.2 * rn(Cin)), invstd=_bf(0.5 + torch.rand(Cin, generator=g)), gamma=_bf(0.5 + torch.rand(Cin, generator=g)) * sign(Cin))


def transform(x, in_scale, in_shift, dtype):
    """-> (a, m).  dtype 'f32' | 'bf16': the pinned rule of the header; None: the plain float64 values (the autograd comparison)."""
    t = x * in_scale + in_shift
    if dtype is not None:
        t = t.float().double()                                   # ONE rounding to fp32: the kernel's fmaf
    a = t.clamp_min(0)
    if dtype == 'bf16':
        a = a.float().bfloat16().double()                        # one rounding to the storage type
    return a, (t > 0).double()


def masked_fraction(c):
    return 1.0 - float(transform(c['x'], c['in_scale'], c['in_shift'], 'f32')[1].mean())


def dense_conv(a, w):
    """a [B,H,W,Cin], w [Cout][Cin] -> (v, A) [B,H,W,Cout]"""
    return torch.einsum('bhwc,nc->bhwn', a, w), torch.einsum('bhwc,nc->bhwn', a.abs(), w.abs())


def dense_dgrad(dy, w, m, x, mean, invstd, gamma):
    """-> dict(G, A, g, xhat, s1, s2, dx): the definition in float64"""
    G = torch.einsum('bhwn,nc->bhwc', dy, w)
    A = torch.einsum('bhwn,nc->bhwc', dy.abs(), w.abs())
    g = m * G
    xhat = (x - mean) * invstd
    N = x.shape[0] * x.shape[1] * x.shape[2]
    s1, s2 = g.sum((0, 1, 2)), (g * xhat).sum((0, 1, 2))
    dx = gamma * invstd * (g - s1 / N - xhat * s2 / N)
    return dict(G=G, A=A, g=g, xhat=xhat, s1=s1, s2=s2, dx=dx, N=N)


def dense_wgrad(dy, a):
    """-> (gw, A) [Cout][Cin]"""
    return torch.einsum('bhwn,bhwc->nc', dy, a), torch.einsum('bhwn,bhwc->nc', dy.abs(), a.abs())


# ---------------------------------------------------------------- bounds
def forward_ref(c, dtype, eval_epilogue, relu):
    """-> dict(exact, tol).  eval_epilogue: relu?(v scale + shift); else relu?(v) (the raw output of the train form, or a transition)"""
    a, _ = transform(c['x'], c['in_scale'], c['in_shift'], dtype)
    v, A = dense_conv(a, c['w'])
    tol = c['x'].shape[3] * U32 * A
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
    """-> dict(exact, tol) of dx plus dbeta / dgamma as dict(exact, tol) under 'dbeta' / 'dgamma' (derivation: the module docstring)"""
    _, m = transform(c['x'], c['in_scale'], c['in_shift'], dtype)
    d = dense_dgrad(c['dy'], c['w'], m, c['x'], c['mean'], c['invstd'], c['gamma'])
    N, g, xh, s1, s2 = d['N'], d['g'], d['xhat'], d['s1'], d['s2']
    K = min(c['x'].shape[3], c['dy'].shape[3])
    tolG = K * U32 * d['A'] * m
    red = lambda t: t.sum((0, 1, 2))
    tol_s1 = red(tolG) + N * U32 * red(g.abs())
    tol_s2 = red(tolG * xh.abs() + g.abs() * 2 * U32 * xh.abs() + U32 * (g * xh).abs()) + N * U32 * red((g * xh).abs())
    t1, t2 = s1 / N, xh * s2 / N
    d1 = tol_s1 / N + 2 * U32 * s1.abs() / N
    d2 = xh.abs() * (tol_s2 / N + 2 * U32 * s2.abs() / N) + 2 * U32 * xh.abs() * s2.abs() / N + U32 * t2.abs()
    tol_i = tolG + d1 + d2 + 2 * U32 * (g.abs() + t1.abs() + t2.abs())
    k = c['gamma'] * c['invstd']
    inner = g - t1 - t2
    e = k * inner
    tol = k.abs() * tol_i + 2 * U32 * e.abs()
    if accumulate:
        tol = _store(e, tol, dtype)                                          # the kernel may round before it adds
        e = e + c['dx_old']
        tol = tol + U32 * e.abs()
    return dict(exact=e, tol=_store(e, tol, dtype), dbeta=dict(exact=s1, tol=tol_s1 + U32 * s1.abs()), dgamma=dict(exact=s2, tol=tol_s2 + U32 * s2.abs()))


def wgrad_ref(c, dtype, accumulate):
    a, _ = transform(c['x'], c['in_scale'], c['in_shift'], dtype)
    gw, A = dense_wgrad(c['dy'], a)
    K = c['x'].shape[0] * c['x'].shape[1] * c['x'].shape[2]
    tol = K * U32 * A
    e = gw
    if accumulate:
        e = e + c['gw_old']
        tol = tol + U32 * e.abs()
    return dict(exact=e, tol=tol)
