"""float64 operator reference for the C-ABI tests of csrc/stacking.hip (TEST INFRASTRUCTURE ONLY).

Every function is written from the operator's definition in saltnet.h, tap by tap with explicit clamped index vectors - not through
F.conv2d / F.pad - so that it is independent of both the kernel and tests/stacking_oracle.py.  Tensors are torch float64, NCHW unless
the name says otherwise."""
import torch


def _f64(t):
    return t.detach().double() if isinstance(t, torch.Tensor) else torch.as_tensor(t, dtype=torch.float64)


def tap_view(x, kh, kw):
    """x[b, m, max(y + kh - 2, 0), min(x + kw, W - 1)]: the input a 3x3 tap reads under the replicate-top-2 / replicate-right-2 pad."""
    H, W = x.shape[-2:]
    rows = (torch.arange(H) + kh - 2).clamp(min=0)
    cols = (torch.arange(W) + kw).clamp(max=W - 1)
    return x[..., rows, :][..., cols]


def conv(x, w, bias=None):
    """-> [B,F,H,W] float64 (differentiable: the CPU tests take dL/dy from autograd)"""
    x, w = x.double(), w.double()
    y = sum(torch.einsum('bmhw,fm->bfhw', tap_view(x, kh, kw), w[:, :, kh, kw]) for kh in range(3) for kw in range(3))
    return y if bias is None else y + bias.double()[None, :, None, None]


def stats(y):
    """-> (mean [F], biased variance [F], unbiased variance [F]) over (B, H, W)"""
    y = _f64(y)
    n = y.shape[0] * y.shape[2] * y.shape[3]
    mean = y.mean(dim=(0, 2, 3))
    m2 = ((y - mean[None, :, None, None]) ** 2).sum(dim=(0, 2, 3))
    return mean, m2 / n, m2 / max(n - 1, 1)


def eval_head(y, scale, shift, relu, gate, head_w, head_b):
    """logits[b,k] = head_b[k] + sum_f head_w[k][f] * relu?(y * scale + shift) * gate[b][f]; ``gate`` [B,F] or None"""
    a = _f64(y) * _f64(scale)[None, :, None, None] + _f64(shift)[None, :, None, None]
    if relu:
        a = a.clamp(min=0)
    if gate is not None:
        a = a * _f64(gate)[:, :, None, None]
    out = torch.einsum('bfhw,kf->bkhw', a, _f64(head_w).reshape(head_w.shape[0], -1))
    return out if head_b is None else out + _f64(head_b)[None, :, None, None]


def xs_nhwc(x, Mpad):
    """the NHWC copy [B,H,W,Mpad] of the input, channels >= M zero"""
    x = _f64(x)
    B, M, H, W = x.shape
    out = torch.zeros(B, H, W, Mpad, dtype=torch.float64)
    out[..., :M] = x.permute(0, 2, 3, 1)
    return out


def wgrad(dy, x, Mpad=None):
    """dW[f,m,kh,kw] = sum_{b,y,x} dy[b,f,y,x] * tap_view(x, kh, kw)[b,m,y,x] -> [F,M,3,3]; with ``Mpad`` the padded [F,Mpad,3,3] form
    whose channels >= M are zero (what the dense weight-gradient kernels produce from xs before salt_stack_grad_unfold drops them)."""
    dy, x = _f64(dy), _f64(x)
    F_, M = dy.shape[1], x.shape[1]
    g = torch.zeros(F_, M if Mpad is None else Mpad, 3, 3, dtype=torch.float64)
    for kh in range(3):
        for kw in range(3):
            g[:, :M, kh, kw] = torch.einsum('bfhw,bmhw->fm', dy, tap_view(x, kh, kw))
    return g


def bn_fold(gamma, beta, mean, var, eps=1e-5):
    scale = _f64(gamma) / torch.sqrt(_f64(var) + eps)
    return scale, _f64(beta) - _f64(mean) * scale
