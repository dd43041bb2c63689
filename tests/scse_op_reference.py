"""Plain torch reference of the concurrent spatial + channel squeeze-excitation operator (salt_scse / salt_scse_bwd / salt_scse_fc_grads,
saltnet.h; csrc/se.hip), NHWC, in whatever dtype its arguments have (float64 for the reference, float32 for the yardstick of the GPU
test's bound).  TEST INFRASTRUCTURE ONLY: forward, the hand-derived backward, the consumer-side BatchNorm finalize in front of the
operator, the bit-exact prediction of the element the operator sees behind its input transform, the BatchNorm-backward sums the
backward also takes, and the case table of tests/test_gpu_scse.py with the seeds tests/test_scse_cpu.py proves fit for the bound."""
from collections import namedtuple

import torch
import torch.nn.functional as F

from oracle import blocks as OB

Fwd = namedtuple('Fwd', 'gap hidden_pre hidden gate_c gate_s y')
Fin = namedtuple('Fin', 'mean var invstd scale shift running_mean running_var')
Seen = namedtuple('Seen', 'a pre doubtful')


def scse(a, w1, b1, w2, b2, ws, bs):
    """a [B,H,W,C]; w1 [R,C], b1 [R], w2 [C,R], b2 [C], ws [C], bs [1] -> Fwd(gap [B,C], hidden_pre, hidden [B,R], gate_c [B,C],
    gate_s [B,H,W], y = relu(a (gate_c + gate_s)))"""
    gap = a.mean(dim=(1, 2))
    hidden_pre = gap @ w1.t() + b1
    hidden = torch.relu(hidden_pre)
    gate_c = torch.sigmoid(hidden @ w2.t() + b2)
    gate_s = torch.sigmoid(a @ ws + bs)
    y = torch.relu(a * (gate_c[:, None, None, :] + gate_s[..., None]))
    return Fwd(gap, hidden_pre, hidden, gate_c, gate_s, y)


def scse_bwd(fwd, dy, a, w1, w2, ws, skip_bcast=False, dx_old=None):
    """fwd: what scse returned (its y is the STORED output: the ReLU mask is taken there).  -> dict(g, dgate_c, ds, dx_direct, du, dh,
    dgap (already divided by HW), g_w1, g_b1, g_w2, g_b2, g_ws, g_bs, dx = dx_direct (+ dgap unless skip_bcast) (+ dx_old))"""
    gc, gs = fwd.gate_c, fwd.gate_s
    hw = a.shape[1] * a.shape[2]
    g = torch.where(fwd.y > 0, dy, torch.zeros_like(dy))
    dgate_c = (g * a).sum(dim=(1, 2))
    ds = (g * a).sum(dim=3) * gs * (1 - gs)
    dx_direct = g * (gc[:, None, None, :] + gs[..., None]) + ds[..., None] * ws
    du = dgate_c * gc * (1 - gc)
    dh = torch.where(fwd.hidden > 0, du @ w2, torch.zeros_like(fwd.hidden))
    dgap = (dh @ w1) / hw
    dx = dx_direct if skip_bcast else dx_direct + dgap[:, None, None, :]
    if dx_old is not None:
        dx = dx + dx_old
    return dict(g=g, dgate_c=dgate_c, ds=ds, dx_direct=dx_direct, du=du, dh=dh, dgap=dgap, g_w2=du.t() @ fwd.hidden, g_b2=du.sum(0),
                g_w1=dh.t() @ fwd.gap, g_b1=dh.sum(0), g_ws=(ds[..., None] * a).sum(dim=(0, 1, 2)), g_bs=ds.sum().reshape(1), dx=dx)


def module_composition(a, w1, b1, w2, b2, ws, bs):
    """The same arithmetic through the oracle's ChannelSELayer and SpatialSELayer (NCHW): the autograd yardstick."""
    sd = {'c.fc.0.weight': w1, 'c.fc.0.bias': b1, 'c.fc.2.weight': w2, 'c.fc.2.bias': b2, 's.fc.weight': ws[None, :, None, None], 's.fc.bias': bs}
    x = a.permute(0, 3, 1, 2)
    return F.relu(OB.channel_se(sd, 'c.', x) + OB.spatial_se(sd, 's.', x)).permute(0, 2, 3, 1)


def bn_finalize64(S, Q, N, gamma, beta, eps, momentum, running):
    """The arithmetic of fin_forward_consumer (csrc/common.h) in the dtype of S: S, Q [C] = sum and sum of squares over N elements per
    channel, running = (running_mean, running_var) -> Fin(mean, biased variance clamped at 0, invstd, scale = gamma invstd,
    shift = beta - mean scale, the updated running statistics (unbiased variance))"""
    mean = S / N
    M2 = (Q - S * mean).clamp_min(0)
    var = M2 / N
    invstd = 1 / torch.sqrt(var + eps)
    scale = gamma * invstd
    unb = M2 / (N - 1) if N > 1 else var
    return Fin(mean, var, invstd, scale, beta - mean * scale, (1 - momentum) * running[0] + momentum * mean, (1 - momentum) * running[1] + momentum * unb)


def transform_exact(x, scale32, shift32, relu, dtype):
    """The element the operator sees behind its input transform, round_to_storage(relu?(fma_f32(x, scale, shift))), bit for bit.
    x [..., C] float64 holding values exact in ``dtype`` storage; scale32, shift32 [C] float32.  -> Seen(a float64, pre = the float32
    multiply-add before the ReLU as float64 (the sign the backward's BatchNorm sums go by), doubtful = elements not decided here).
    bf16: x has 8 significant bits and scale 24, so the product (32 bits) and its sum with shift are exact in float64 for operands of
    comparable magnitude; ONE rounding to float32 is __fmaf_rn, one more to bf16 is pack16.  f32: the product (48 bits) is exact, the sum
    is rounded once to float64 (2**-53 relative) before the rounding to float32 - the two roundings differ from the single one only if
    the float64 value lies that close to a midpoint of two neighbouring float32 values; elements whose float64 sum was inexact and lies
    within 2**-50 relative of one are reported as doubtful (a killed element is decided whatever its rounding)."""
    assert x.dtype == torch.float64 and scale32.dtype == torch.float32 and shift32.dtype == torch.float32
    v = x * scale32.double() + shift32.double()
    pre = v.float()
    doubtful = torch.zeros_like(v, dtype=torch.bool)
    if dtype != 'bf16':
        inf = torch.full_like(pre, float('inf'))
        up, dn = (pre.double() + torch.nextafter(pre, inf).double()) / 2, (pre.double() + torch.nextafter(pre, -inf).double()) / 2
        p, h = x * scale32.double(), shift32.double().expand_as(v)
        t = v - p
        lost = (p - (v - t)) + (h - t)                     # two-sum: what the float64 addition dropped (0: v is the exact value, ties included)
        doubtful = (torch.minimum((v - up).abs(), (v - dn).abs()) <= 2.0 ** -50 * v.abs()) & (lost != 0)
        if relu:
            doubtful &= v > 0
    a = torch.relu(pre) if relu else pre
    if dtype == 'bf16':
        a = a.bfloat16()
    return Seen(a.double(), pre.double(), doubtful)


def bnb_sums(x_raw, a_pre_sign, dx_stored, dgap, mean, invstd, per_image=False):
    """The sums the BatchNorm backward of the layer in front reduces, da = dx_stored + dgap (broadcast over the image) where the layer's
    ReLU was on: a_pre_sign [B,H,W,C] bool (pre-activation > 0), or None without in_relu.  -> s1 = sum da, s2 = sum da xhat, [C]
    (per_image: [B,C])"""
    xhat = (x_raw - mean) * invstd
    da = dx_stored + dgap[:, None, None, :]
    if a_pre_sign is not None:
        da = torch.where(a_pre_sign, da, torch.zeros_like(da))
    dims = (1, 2) if per_image else (0, 1, 2)
    return da.sum(dim=dims), (da * xhat).sum(dim=dims)


EPS, MOMENTUM = 1e-5, 0.1
MODES = ('plain', 'fin0', 'fin1')          # the operator's input: a = x as stored; a = bn(x_raw); a = relu(bn(x_raw))


def stats64(x_raw):
    """(sum, sum of squares, count) of a raw tensor per channel, float64"""
    flat = x_raw.reshape(-1, x_raw.shape[-1])
    return flat.sum(0), (flat * flat).sum(0), flat.shape[0]


def make_case(B, H, W, C, R, seed, dtype):
    """Inputs of one operator case, float64 holding values exact in ``dtype`` storage (x, dy, dx_old, x_raw) or in float32 (parameters).
    'w1' is a dict over MODES: each normalised to the pooled vector of the input that mode's operator sees, so that hidden units are
    alive and the gates spread over (0, 1) at every map size; ws ~ N(0, 1 / C); gamma, beta, running statistics and a raw x for the
    input transform."""
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    st = (lambda t: t.bfloat16().double()) if dtype == 'bf16' else (lambda t: t.float().double())
    f32 = lambda t: t.float().double()
    c = dict(x=st(rnd(B, H, W, C)), dy=st(rnd(B, H, W, C)), dx_old=st(rnd(B, H, W, C)))
    c['x_raw'] = st(0.3 * rnd(C) + (0.5 + torch.rand(C, generator=g, dtype=torch.float64)) * rnd(B, H, W, C))
    c['gamma'], c['beta'] = f32(1.0 + 0.3 * rnd(C)), f32(0.3 * rnd(C))
    c['running_mean'], c['running_var'] = f32(0.2 * rnd(C)), f32(0.5 + torch.rand(C, generator=g, dtype=torch.float64))
    unit = rnd(R, C) / C ** 0.5
    c['b1'] = f32(0.2 * rnd(R))
    c['w2'] = f32(rnd(C, R) * (1.5 / max(0.5 * R, 1.0) ** 0.5))
    c['b2'] = f32(0.3 * rnd(C))
    c['ws'] = f32(rnd(C) / C ** 0.5)
    c['bs'] = f32(0.3 * rnd(1))
    S, Q, N = stats64(c['x_raw'])
    fin = bn_finalize64(S, Q, N, c['gamma'], c['beta'], EPS, MOMENTUM, (c['running_mean'], c['running_var']))
    c['a'] = {'plain': c['x']}
    for relu in (0, 1):
        c['a']['fin%d' % relu] = transform_exact(c['x_raw'], fin.scale.float(), fin.shift.float(), relu, dtype).a
    c['w1'] = {m: f32(unit / float(c['a'][m].mean(dim=(1, 2)).pow(2).mean().sqrt())) for m in MODES}
    return c


def params(c, mode, dtype=torch.float64):
    return [c[k][mode].to(dtype) if k == 'w1' else c[k].to(dtype) for k in ('w1', 'b1', 'w2', 'b2', 'ws', 'bs')]


def hidden_band(a, p64):
    """(smallest |hidden pre-activation|, the band 4 e32 + 1e-6 max of the hidden layer) of input ``a`` under parameters p64"""
    f64 = scse(a, *p64)
    f32 = scse(a.float(), *[t.float() for t in p64])
    band = 4 * float((f32.hidden_pre.double() - f64.hidden_pre).abs().max()) + 1e-6 * float(f64.hidden_pre.abs().max())
    return float(f64.hidden_pre.abs().min()), band


def fitness(c):
    """What makes a drawn case fit for a bound without exclusions (tests/test_scse_cpu.py): dict of the figures, and ``ok``."""
    out = dict(zeros=int((c['x'] == 0).sum()), margin=float('inf'), live=True, dead=True, spread_c=1.0, spread_s=1.0)
    for m in MODES:
        p = params(c, m)
        f = scse(c['a'][m], *p)
        lo, band = hidden_band(c['a'][m], p)
        out['margin'] = min(out['margin'], lo / band)
        out['live'] = out['live'] and bool((f.hidden_pre > 0).any())
        out['dead'] = out['dead'] and bool((f.hidden_pre < 0).any())
        out['spread_c'] = min(out['spread_c'], float(((f.gate_c > 0.1) & (f.gate_c < 0.9)).double().mean()))
        out['spread_s'] = min(out['spread_s'], float(((f.gate_s > 0.1) & (f.gate_s < 0.9)).double().mean()))
    out['ok'] = (out['zeros'] == 0 and out['margin'] >= 100 and out['live'] and out['dead'] and out['spread_c'] >= 0.5 and out['spread_s'] >= 0.5)
    return out


# (B, H, W, C, R) per dtype, the smallest shapes at which each branch of csrc/se.hip is live (the issue's table), and the seed of
# make_case that tests/test_scse_cpu.py proves fit.  A shape with R = 1 has one hidden unit: live in one image, dead in the other.
CASES = {
    'one-pixel': {'bf16': (2, 1, 1, 16, 1), 'f32': (2, 1, 1, 16, 1)},
    'one-lane': {'bf16': (3, 3, 5, 8, 3), 'f32': (3, 3, 5, 4, 3)},
    'ragged-parts': {'bf16': (2, 17, 19, 64, 4), 'f32': (2, 17, 19, 64, 4)},
    'whole-wave': {'bf16': (2, 4, 4, 512, 32), 'f32': (2, 4, 4, 256, 16)},
    'part-cap': {'bf16': (1, 66, 66, 16, 2), 'f32': (1, 66, 66, 16, 2)},
    'strided-fc': {'bf16': (2, 2, 3, 32, 260), 'f32': (2, 2, 3, 32, 260)},
    'batch-tiles': {'bf16': (27, 2, 2, 512, 32), 'f32': (53, 2, 2, 256, 16)},
}
SEEDS = {('one-pixel', 'bf16'): 0, ('one-pixel', 'f32'): 0, ('one-lane', 'bf16'): 0, ('one-lane', 'f32'): 0, ('ragged-parts', 'bf16'): 0,
         ('ragged-parts', 'f32'): 0, ('whole-wave', 'bf16'): 0, ('whole-wave', 'f32'): 0, ('part-cap', 'bf16'): 26, ('part-cap', 'f32'): 26,
         ('strided-fc', 'bf16'): 3, ('strided-fc', 'f32'): 2, ('batch-tiles', 'bf16'): 0, ('batch-tiles', 'f32'): 3}      # the first fit seed of find_seed


def storage_allowance(ref, stored_before=None):
    """What round-to-nearest bf16 storage may cost per element: 2**-8 |ref| (8 significant bits) for a value stored once - and 2**-8 of
    the intermediate value as well where the output was stored, read back and stored again (``stored_before``: salt_scse_bwd's
    broadcast pass, which adds dgap to the dx the first pass stored)."""
    return 2.0 ** -8 * (ref.abs() + (stored_before.abs() if stored_before is not None else 0.0))


def find_seed(name, dtype, tries=200):
    for seed in range(tries):
        if fitness(make_case(*CASES[name][dtype], seed, dtype))['ok']:
            return seed
    return None
