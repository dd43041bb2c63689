"""Float64 references of the six pyramid-pooling operators (include/saltnet.h: salt_psp_pool / salt_psp_pool_bwd / salt_psp_merge /
salt_psp_merge_bwd / salt_bn_prelu / salt_bn_prelu_bwd), written from the definitions, NHWC, each with a derived per-element bound.
test_psp_cpu.py pins them against torch's own adaptive_avg_pool2d / interpolate / prelu and autograd in double and the index tables
against hand-computed values; test_gpu_psp.py holds the kernels to them, elementwise, no element excluded.

Operands are bf16-representable (make_*), so every product of two of them is exact in float64 and the only differences between kernel
and reference are the fp32 roundings counted below (u = 2^-23) and the storage rounding (2^-8 per bf16 store, conv_abi.store_tol).
What is PINNED by the header is reproduced, not bounded:
  * the bilinear source index and the two weights of a destination are formed here with the same fp32 operations in the same order
    (resize_taps: numpy float32), the dense resize matrix adds the two weights of a clamped destination in fp32 as the backward kernel
    does, and a tap's weight is the fp32 product of its row and column weight;
  * the PReLU pre-activation u = fmaf(y, scale, shift) is the float64 multiply-add (exact for these operands) rounded once to fp32,
    and the mask is [u > 0] of that same u: a mask that flipped on a near-zero u would change du by a whole value.
Bounds (A = the sum of the absolute values of the same terms; "K u A" = K fp32 additions in any order, each off by at most u of a partial
sum that A bounds):
  pool       p = (sum of `area` pixels) / area:   tol = area u A / area + u |p|                       (the division rounds once)
  pool_bwd   dx = sum of T terms dp / area:       tol = u A (the T divisions) + T u A, + u |dx + old| with accumulate
  merge      v = f + bias + sum_k sum_taps w q:   the forward kernel adds the two taps of a clamped destination separately where the
             matrix holds their rounded sum (<= 2 u per axis, 1 u for the product: 3 u A), a stage's four products and three additions
             (<= 4 u A_k), five additions into v (<= 5 u A): tol = 12 u A; the ReLU is 1-Lipschitz
  merge_bwd  df = dy [y > 0] is exact;  dq = sum over at most h w pixels of w g: tol = (h w + 1) u A (products and additions; the
             weights are the reference's own);  dbias: h w additions per image, B over the images, one more with accumulate
  bn_prelu   a = u or alpha u: tol = u |a|;       bn_prelu_bwd  du = da or alpha da: tol = u |du|;  dalpha = sum of N products da u:
             tol = (N + 1) u A (N = every element of the tensor, whatever the kernel's tree)."""
import numpy as np
import torch

from conv_abi import ratio_strict as ratio, store_tol as _store          # noqa: F401  (ratio is the tests' entry point)

F64 = torch.float64
U32 = 2.0 ** -23
SIZES = (1, 2, 3, 6)

# (B, h, w, C): the depth-34 shape class; s > h (repeated bins), one ragged channel block; odd, non-square, C no multiple of 16 or 64;
# more pixels than threads per pass
PSP_SHAPES = [(2, 8, 8, 64), (1, 4, 4, 32), (3, 5, 7, 40), (1, 16, 16, 64)]
MERGE_COUT = (64, 160)          # one channel block; three, the last one ragged
PRELU_SHAPES = [(2, 6, 10, 16), (3, 5, 7, 24), (4, 32, 32, 64)]
ALPHAS = (0.25, 0.0, 1.0, -0.5)


def _bf(t):
    return t.bfloat16().double()


# ---------------------------------------------------------------- index tables
def bins(n, s):
    """torch's adaptive pooling windows along an axis of n elements: [(first, one past the last)] for the s bins"""
    return [((i * n) // s, -((-(i + 1) * n) // s)) for i in range(s)]


def resize_taps(n, s, ac):
    """size-based bilinear resize from s sources to n destinations -> [(i0, i1, w0, w1)] with the weights as fp32 values, formed by
    the header's pinned sequence"""
    f = np.float32
    out = []
    for d in range(n):
        if ac:
            src = (f(s - 1) / f(n - 1)) * f(d) if n > 1 else f(0)
        else:
            src = (f(s) / f(n)) * (f(d) + f(0.5)) - f(0.5)
            src = f(0) if src < 0 else src
        src = f(src)
        i0 = min(int(src), s - 1)
        i1 = min(i0 + 1, s - 1)
        w1 = f(src - f(i0))
        w0 = f(f(1) - w1)
        out.append((i0, i1, float(w0), float(w1)))
    return out


def resize_matrix(n, s, ac):
    """[n][s] float64 holding fp32 values: row d has w0 at i0 and w1 at i1, added in fp32 where the two coincide"""
    M = np.zeros((n, s), dtype=np.float32)
    for d, (i0, i1, w0, w1) in enumerate(resize_taps(n, s, ac)):
        M[d, i0] += np.float32(w0)
        M[d, i1] += np.float32(w1)
    return torch.from_numpy(M.astype(np.float64))


def tap_weights(h, w, s, ac):
    """[h][w][s][s]: fp32 product of the row and the column weight, as float64"""
    My, Mx = resize_matrix(h, s, ac), resize_matrix(w, s, ac)
    return torch.einsum('yi,xj->yxij', My, Mx).float().double()


def pool_indicator(n, s):
    P = torch.zeros(s, n, dtype=F64)
    for i, (lo, hi) in enumerate(bins(n, s)):
        P[i, lo:hi] = 1.0
    return P


# ---------------------------------------------------------------- definitions (float64, also what test_psp_cpu.py compares with torch)
def pool(x, sizes=SIZES):
    """x [B,h,w,C] -> [p_k [B,s,s,C]]"""
    out = []
    for s in sizes:
        Py, Px = pool_indicator(x.shape[1], s), pool_indicator(x.shape[2], s)
        area = Py.sum(1)[:, None] * Px.sum(1)[None, :]
        out.append(torch.einsum('iy,jx,byxc->bijc', Py, Px, x) / area[None, :, :, None])
    return out


def pool_bwd(dps, h, w, sizes=SIZES):
    """[dp_k [B,s,s,C]] -> dx [B,h,w,C] and A, T for the bound"""
    dx = A = 0.0
    T = torch.zeros(h, w, dtype=F64)
    for s, dp in zip(sizes, dps):
        Py, Px = pool_indicator(h, s), pool_indicator(w, s)
        area = Py.sum(1)[:, None] * Px.sum(1)[None, :]
        t = dp / area[None, :, :, None]
        dx = dx + torch.einsum('iy,jx,bijc->byxc', Py, Px, t)
        A = A + torch.einsum('iy,jx,bijc->byxc', Py, Px, t.abs())
        T = T + torch.einsum('iy,jx->yx', Py, Px)
    return dx, A, T


def merge(f, bias, qs, ac, sizes=SIZES):
    """-> (v before the ReLU, A)"""
    v = f + (bias if bias is not None else 0.0)
    A = f.abs() + (bias.abs() if bias is not None else 0.0)
    for s, q in zip(sizes, qs):
        Wt = tap_weights(f.shape[1], f.shape[2], s, ac)
        v = v + torch.einsum('yxij,bijc->byxc', Wt, q)
        A = A + torch.einsum('yxij,bijc->byxc', Wt, q.abs())
    return v, A


def merge_bwd(dy, y, ac, sizes=SIZES):
    """-> (g, [dq_k], [A_k], dbias, A_bias)"""
    g = dy * (y > 0).double()
    dqs, As = [], []
    for s in sizes:
        Wt = tap_weights(y.shape[1], y.shape[2], s, ac)
        dqs.append(torch.einsum('yxij,byxc->bijc', Wt, g))
        As.append(torch.einsum('yxij,byxc->bijc', Wt, g.abs()))
    return g, dqs, As, g.sum((0, 1, 2)), g.abs().sum((0, 1, 2))


def pre_activation(y, scale, shift, pinned=True):
    """u = y scale + shift (u = y without them); pinned: rounded once to fp32 - the kernel's fmaf"""
    if scale is None:
        return y
    u = y * scale + shift
    return u.float().double() if pinned else u


def prelu(u, alpha):
    return torch.where(u > 0, u, alpha * u)


# ---------------------------------------------------------------- cases
def make_psp_case(B, h, w, C, Cout, seed, sizes=SIZES):
    """float64 tensors holding bf16-representable values; y is a ReLU output with about half of its elements zero"""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: _bf(torch.randn(*s, generator=g))
    return dict(x=rn(B, h, w, C), dp=[rn(B, s, s, C) for s in sizes], dx_old=rn(B, h, w, C),
                f=rn(B, h, w, Cout), bias=rn(Cout), q=[rn(B, s, s, Cout) for s in sizes],
                dy=rn(B, h, w, Cout), y=rn(B, h, w, Cout).clamp_min(0), dbias_old=rn(Cout))


def make_prelu_case(B, H, W, C, seed):
    """20 % of the scales negative; shift = 0.3 N(0,1) against |scale| in [0.5, 1.5): about half of the pre-activations are negative"""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: _bf(torch.randn(*s, generator=g))
    sign = torch.where(torch.rand(C, generator=g) < 0.2, -1.0, 1.0).double()
    return dict(y=rn(B, H, W, C), da=rn(B, H, W, C), scale=_bf(0.5 + torch.rand(C, generator=g)) * sign, shift=_bf(0.3 * torch.randn(C, generator=g)),
                dalpha_old=rn(1))


# ---------------------------------------------------------------- bounds: dict(exact, tol)
def pool_ref(c, dtype, sizes=SIZES):
    """-> [dict(exact, tol)] per stage"""
    h, w = c['x'].shape[1:3]
    out = []
    for s, p, a in zip(sizes, pool(c['x'], sizes), pool(c['x'].abs(), sizes)):
        area = torch.tensor([[(y1 - y0) * (x1 - x0) for x0, x1 in bins(w, s)] for y0, y1 in bins(h, s)], dtype=F64)[None, :, :, None]
        tol = area * U32 * a + U32 * p.abs()                # a = A / area
        out.append(dict(exact=p, tol=_store(p, tol, dtype)))
    return out


def pool_bwd_ref(c, dtype, accumulate, sizes=SIZES):
    h, w = c['dx_old'].shape[1:3]
    dx, A, T = pool_bwd(c['dp'], h, w, sizes)
    tol = (1 + T)[None, :, :, None] * U32 * A
    if accumulate:
        dx = dx + c['dx_old']
        tol = tol + U32 * dx.abs()
    return dict(exact=dx, tol=_store(dx, tol, dtype))


def merge_ref(c, dtype, ac, bias=True, sizes=SIZES):
    v, A = merge(c['f'], c['bias'] if bias else None, c['q'], ac, sizes)
    e = v.clamp_min(0)
    return dict(exact=e, tol=_store(e, 12 * U32 * A, dtype))


def merge_bwd_ref(c, dtype, ac, accumulate, sizes=SIZES):
    """-> dict(df, dq [per stage], dbias), each dict(exact, tol)"""
    B, h, w, _ = c['y'].shape
    g, dqs, As, db, Ab = merge_bwd(c['dy'], c['y'], ac, sizes)
    tol_b = (h * w + B) * U32 * Ab
    if accumulate:
        db = db + c['dbias_old']
        tol_b = tol_b + U32 * db.abs()
    return dict(df=dict(exact=g, tol=torch.zeros_like(g)),
                dq=[dict(exact=q, tol=_store(q, (h * w + 1) * U32 * a, dtype)) for q, a in zip(dqs, As)],
                dbias=dict(exact=db, tol=tol_b))


def bn_prelu_ref(c, dtype, alpha, affine=True):
    u = pre_activation(c['y'], c['scale'] if affine else None, c['shift'] if affine else None)
    a = prelu(u, alpha)
    return dict(exact=a, tol=_store(a, U32 * a.abs(), dtype))


def bn_prelu_bwd_ref(c, dtype, alpha, accumulate, affine=True):
    """-> dict(du, dalpha)"""
    u = pre_activation(c['y'], c['scale'] if affine else None, c['shift'] if affine else None)
    du = torch.where(u > 0, c['da'], alpha * c['da'])
    t = c['da'] * u.clamp_max(0)
    da, tol_a = t.sum().reshape(1), (t.numel() + 1) * U32 * t.abs().sum().reshape(1)
    if accumulate:
        da = da + c['dalpha_old']
        tol_a = tol_a + U32 * da.abs()
    return dict(du=dict(exact=du, tol=_store(du, U32 * du.abs(), dtype)), dalpha=dict(exact=da, tol=tol_a))


def negative_fraction(c, affine=True):
    u = pre_activation(c['y'], c['scale'] if affine else None, c['shift'] if affine else None)
    return float((u <= 0).double().mean())

