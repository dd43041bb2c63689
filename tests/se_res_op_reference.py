"""Plain torch reference of the fused SE-ResNet bottleneck tail (salt_se_res / salt_se_res_bwd / salt_se_res_fc_grads, saltnet.h), NHWC,
in whatever dtype its arguments have (float64 for the reference, float32 for the yardstick of the GPU test's bound).  TEST
INFRASTRUCTURE ONLY: forward and the hand-derived backward of the issue's "Backward of the tail", checked against torch autograd of the
plain module composition (tests/test_seresnet_cpu.py)."""
import torch
import torch.nn.functional as F


def z_of(x, scale, shift):
    return x if scale is None else x * scale + shift


def se_res(x, scale, shift, res, w1, b1, w2, b2):
    """x, res [B,H,W,C]; scale, shift [C] or None; w1 [R,C], b1 [R], w2 [C,R], b2 [C] -> dict(gap, hidden, gate, y, z)"""
    z = z_of(x, scale, shift)
    gap = z.mean(dim=(1, 2))
    hidden = torch.relu(gap @ w1.t() + b1)
    gate = torch.sigmoid(hidden @ w2.t() + b2)
    pre = z * gate[:, None, None, :] + res
    return dict(z=z, gap=gap, hidden=hidden, gate=gate, pre=pre, y=torch.relu(pre))


def se_res_bwd(fwd, dy, w1, w2, dres_old=None):
    """fwd: what se_res returned.  -> dict(dx (= dL/dz), dres, g_w1, g_b1, g_w2, g_b2, dgate, du, dh, dgap (already divided by HW))"""
    z, gap, hidden, gate = fwd['z'], fwd['gap'], fwd['hidden'], fwd['gate']
    hw = z.shape[1] * z.shape[2]
    m = torch.where(fwd['y'] > 0, dy, torch.zeros_like(dy))
    dgate = (m * z).sum(dim=(1, 2))
    du = dgate * gate * (1 - gate)
    dh = torch.where(hidden > 0, du @ w2, torch.zeros_like(hidden))
    dgap = dh @ w1
    dx = m * gate[:, None, None, :] + dgap[:, None, None, :] / hw
    return dict(dx=dx, dres=m if dres_old is None else dres_old + m, g_w2=du.t() @ hidden, g_b2=du.sum(0), g_w1=dh.t() @ gap, g_b1=dh.sum(0),
                dgate=dgate, du=du, dh=dh, dgap=dgap / hw)


def module_composition(x, scale, shift, res, w1, b1, w2, b2):
    """The same arithmetic the way the modules spell it (NCHW, 1x1 convolutions, adaptive average pool): the autograd yardstick."""
    xn, rn = x.permute(0, 3, 1, 2), res.permute(0, 3, 1, 2)
    z = xn if scale is None else xn * scale[None, :, None, None] + shift[None, :, None, None]
    s = F.adaptive_avg_pool2d(z, 1)
    s = torch.relu(F.conv2d(s, w1[:, :, None, None], b1))
    s = torch.sigmoid(F.conv2d(s, w2[:, :, None, None], b2))
    return torch.relu(z * s + rn).permute(0, 2, 3, 1)


def make_case(B, H, W, C, seed, affine, dtype='f32'):
    """Inputs of one operator case, float64 holding values exact in ``dtype`` storage: x, res, dy, dres_old [B,H,W,C], scale / shift
    (None without ``affine``), the FC parameters."""
    g = torch.Generator().manual_seed(seed)
    R = C // 16
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    st = (lambda t: t.bfloat16().double()) if dtype == 'bf16' else (lambda t: t.float().double())
    f32 = lambda t: t.float().double()
    c = dict(x=st(rnd(B, H, W, C)), res=st(rnd(B, H, W, C)), dy=st(rnd(B, H, W, C)), dres_old=st(rnd(B, H, W, C)))
    c['scale'] = f32(1.0 + 0.3 * rnd(C)) if affine else None
    c['shift'] = f32(0.3 * rnd(C)) if affine else None
    # normalised to the case's own pooled vector, so that hidden units are alive and the gates spread over (0, 1) at every map size
    gap = z_of(c['x'], c['scale'], c['shift']).mean(dim=(1, 2))
    c['w1'] = f32(rnd(R, C) / (C ** 0.5 * float(gap.pow(2).mean().sqrt())))
    c['b1'] = f32(0.2 * rnd(R))
    c['w2'] = f32(rnd(C, R) * (1.5 / (0.5 * R) ** 0.5))
    c['b2'] = f32(0.3 * rnd(C))
    return c
