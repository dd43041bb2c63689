"""conv_abi.py's float64 convolution reference and its error bound, on the CPU (no library needed): the reference is pinned against
torch.nn.functional.conv2d / conv_transpose2d and autograd's input gradient in float64 for every launch form test_gpu_conv_abi.py
uses; an fp32 stand-in for a kernel (per-tap fp32 sums, fp32 epilogue, the storage roundings where the kernels have them) passes
the bound on every case of that file's table; three reference-side mutations are rejected by it."""
import pytest
import torch
import torch.nn.functional as F

import conv_abi as CA
from conv_abi import k3_taps
from op_reference import pad_fold, round_to

K3, K3R = k3_taps(0), k3_taps(1)


def _nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _ops(B, Cin, Cout, H, W, KH, KW, transposed=False, seed=1):
    x = _nhwc(CA.mk(B, Cin, H, W, seed))
    w = CA.master_weight(Cin if transposed else Cout, Cout if transposed else Cin, KH, KW, Cin, KH * KW, seed + 1)
    return x, w


def _sum(x, w, taps, transpose, in_step, pad_mode, OH, OW):
    wt = CA.tap_weights(w, [(t[0], t[1]) for t in taps], transpose)
    return CA.conv_sum(x, wt, [(t[2], t[3]) for t in taps], in_step, pad_mode, OH, OW)[0]


def _close(a, b):
    assert a.shape == b.shape
    assert float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))


@pytest.mark.parametrize('stride', [1, 2])
@pytest.mark.parametrize('k', [3, 1])
def test_zero_pad_forward_is_conv2d(stride, k):
    x, w = _ops(2, 5, 7, 9, 6, k, k)
    taps = K3 if k == 3 else CA.K1
    OH, OW = (9 - 1) // stride + 1, (6 - 1) // stride + 1
    want = F.conv2d(_nchw(x).double(), w.double(), stride=stride, padding=k // 2)
    _close(_sum(x, w, taps, 0, stride, 0, OH, OW), _nhwc(want))


def test_row_kernel_is_conv2d():
    x, w = _ops(2, 5, 7, 9, 6, 1, 3)
    _close(_sum(x, w, CA.K13, 0, 1, 0, 9, 6), _nhwc(F.conv2d(_nchw(x).double(), w.double(), padding=(0, 1))))


def test_replicate_pad_forward_is_pad_plus_valid_conv2d():
    x, w = _ops(2, 5, 7, 9, 6, 3, 3)
    want = F.conv2d(F.pad(_nchw(x).double(), (0, 2, 2, 0), mode='replicate'), w.double())
    _close(_sum(x, w, K3R, 0, 1, 1, 9, 6), _nhwc(want))


@pytest.mark.parametrize('K', [4, 3])
def test_conv_transpose_phases(K):
    x, w = _ops(2, 5, 7, 6, 4, K, K, transposed=True)
    want = _nhwc(F.conv_transpose2d(_nchw(x).double(), w.double(), stride=2, padding=1, output_padding=K % 2))
    assert want.shape[1:3] == (12, 8)
    counts = []
    for fy, fx, sel in CA.convt_phases(K):
        counts.append(len(sel))
        _close(_sum(x, w, sel, 1, 1, 0, 6, 4), want[:, fy::2, fx::2])
    assert sorted(counts) == ([4, 4, 4, 4] if K == 4 else [1, 2, 2, 4])


def _input_grad(fn, x, dy):
    xr = _nchw(x).double().requires_grad_(True)
    fn(xr).backward(_nchw(dy).double())
    return _nhwc(xr.grad)


def test_dgrad_mirrored_taps_are_the_input_gradient():
    x, w = _ops(2, 5, 7, 9, 6, 3, 3)
    dy = _nhwc(CA.mk(2, 7, 9, 6, 5))
    want = _input_grad(lambda t: F.conv2d(t, w.double(), padding=1), x, dy)
    _close(_sum(dy, w, CA.dgrad_taps(K3), 1, 1, 0, 9, 6), want)


@pytest.mark.parametrize('K', [3, 5])
def test_dgrad_stride2_phases_and_their_unified_form(K):
    """k3 (padding 1): the four phases have 1, 2, 2 and 4 taps over 4 unified offsets, the form the graph builder emits; k5 (padding 2):
    4, 6, 6 and 9 taps over 9 unified offsets."""
    x, w = _ops(2, 5, 7, 10, 6, K, K)
    dy = _nhwc(CA.mk(2, 7, 5, 3, 5))
    want = _input_grad(lambda t: F.conv2d(t, w.double(), stride=2, padding=K // 2), x, dy)
    phases = CA.dgrad_s2_phases(CA.kk_taps(K))
    offs, rows = CA.unify_phases(phases)
    assert len(offs) == (4 if K == 3 else 9)
    assert sorted(sum(k is not None for k in row) for row in rows) == ([1, 2, 2, 4] if K == 3 else [4, 6, 6, 9])
    for (ay, ax, sel), row in zip(phases, rows):
        _close(_sum(dy, w, sel, 1, 1, 0, 5, 3), want[:, ay::2, ax::2])
        v = CA.conv_sum(dy, CA.tap_weights(w, row, 1), offs, 1, 0, 5, 3)[0]          # the unified offsets, zero taps
        _close(v, want[:, ay::2, ax::2])


def test_extended_grid_dgrad_then_pad_fold_is_the_replicate_pad_input_gradient():
    x, w = _ops(2, 5, 7, 9, 6, 3, 3)
    dy = _nhwc(CA.mk(2, 7, 9, 6, 5))
    want = _input_grad(lambda t: F.conv2d(F.pad(t, (0, 2, 2, 0), mode='replicate'), w.double()), x, dy)
    ext = _sum(dy, w, CA.dgrad_taps_extended(K3R, 2), 1, 1, 0, 11, 8)
    _close(pad_fold(ext, 2, 0, 0, 2), want)
    wt = CA.tap_weights(w, [(t[0], t[1]) for t in K3R], 1)
    ref = CA.conv_ref(dy, wt, [(t[2], t[3]) for t in CA.dgrad_taps_extended(K3R, 2)], 1, 0, 11, 8, 'f32', fold=(2, 2))
    _close(ref['exact'], want)


def test_epilogue_order_and_storage_roundings():
    x, w = _ops(2, 5, 7, 9, 6, 3, 3)
    wt, offs = CA.tap_weights(w, [(t[0], t[1]) for t in K3], 0), [(t[2], t[3]) for t in K3]
    b, s, h = CA._vec(7, 3, 'bias'), CA._vec(7, 4, 'scale'), CA._vec(7, 5, 'shift')
    res, old = _nhwc(CA.mk(2, 7, 9, 6, 8)).double(), _nhwc(CA.mk(2, 7, 9, 6, 9)).double()
    v = CA.conv_sum(x, wt, offs, 1, 0, 9, 6)[0]
    e = (v + b) * s + h
    r = CA.conv_ref(x, wt, offs, 1, 0, 9, 6, 'bf16', b, s, h, True)
    _close(r['exact'], e.clamp_min(0))
    assert torch.equal(r['stored'], round_to(e.clamp_min(0), 'bf16'))
    r = CA.conv_ref(x, wt, offs, 1, 0, 9, 6, 'bf16', b, s, h, True, res=res)
    _close(r['exact'], (e + res).clamp_min(0))                              # the ReLU follows the add
    assert torch.equal(r['stored'], round_to((round_to(e, 'bf16') + res).clamp_min(0), 'bf16'))
    r = CA.conv_ref(x, wt, offs, 1, 0, 9, 6, 'bf16', b, old=old)
    _close(r['exact'], v + b + old)
    assert torch.equal(r['stored'], round_to(round_to(v + b, 'bf16') + old, 'bf16'))
    assert bool((r['tol'] > 0).all())


# ---------------------------------------------------------------- the bound lets an fp32 implementation pass
def _standin(c, o):
    """What a kernel computes, in torch fp32: per-tap fp32 sums (another order than the reference's), fp32 epilogue, storage roundings."""
    st = (lambda t: t.bfloat16().float()) if c['dtype'] == 'bf16' else (lambda t: t)
    x, wt = o['x'].float(), o['wt'].float()
    if c['in_tf']:
        x = x * o['in_tf'][0].float() + o['in_tf'][1].float()
        x = st(x.clamp_min(0) if o['in_tf'][2] else x)
    B, H, W, _ = x.shape
    v = torch.zeros(B, c['OH'], c['OW'], c['Cout'])
    for t, (dy, dx) in reversed(list(enumerate(o['offs']))):
        iy, ix = torch.arange(c['OH']) * c['in_step'] + dy, torch.arange(c['OW']) * c['in_step'] + dx
        g = x[:, iy.clamp(0, H - 1)][:, :, ix.clamp(0, W - 1)]
        if not c['pad_mode']:
            ok = ((iy >= 0) & (iy < H)).float()[:, None] * ((ix >= 0) & (ix < W)).float()[None, :]
            g = g * ok[None, :, :, None]
        v = v + g.reshape(-1, g.shape[3]).matmul(wt[t].t()).reshape(v.shape)
    if o['bias'] is not None:
        v = v + o['bias'].float()
    if o['scale'] is not None:
        v = v * o['scale'].float()
    if o['shift'] is not None:
        v = v + o['shift'].float()
    if c['relu'] and o['res'] is None:
        v = v.clamp_min(0)
    if c['fold'] and c['fold'][0] == 'fused':
        v = st(pad_fold(st(v), c['fold'][1], 0, 0, c['fold'][2]))
    if o['res'] is not None:
        v = st(v) + o['res'].float()
        v = v.clamp_min(0) if c['relu'] else v
    if o['old'] is not None:
        v = st(v) + o['old'].float()
    return st(v)


@pytest.mark.parametrize('c', CA.CASES)
def test_bound_lets_fp32_pass(c):
    o = CA.build(c)
    r = CA.ratio(_standin(c, o), o['ref'])
    assert r <= 1.0, 'fp32 stand-in at %.3f of the bound' % r


# ---------------------------------------------------------------- ... and rejects a wrong result
SHAPES = [(3, 13, 7, 5, 10), (2, 64, 16, 16, 64), (5, 160, 8, 8, 64), (2, 96, 33, 17, 96)]


def _mutation_ops(shape, pad_mode):
    B, Cin, H, W, Cout = shape
    x, w = _ops(B, Cin, Cout, H, W, 3, 3, seed=40)
    taps = K3R if pad_mode else K3
    return x, CA.tap_weights(w, [(t[0], t[1]) for t in taps], 0), [(t[2], t[3]) for t in taps]


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
@pytest.mark.parametrize('shape', SHAPES)
def test_bound_rejects_one_dropped_border_tap(shape, dtype):
    x, wt, offs = _mutation_ops(shape, 0)
    B, Cin, H, W, Cout = shape
    ref = CA.conv_ref(x, wt, offs, 1, 0, H, W, dtype)
    got = ref['exact'].clone()
    got[0, 0, 0] -= wt[8].matmul(x[0, 1, 1].double())                       # tap (+1, +1) of the corner pixel, one image
    r = CA.ratio(round_to(got, dtype), ref)
    assert r > 1.0, r
    assert CA.ratio(round_to(ref['exact'], dtype), ref) <= 1.0              # the same values without the mutation pass


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
@pytest.mark.parametrize('shape', SHAPES)
def test_bound_rejects_a_clamp_one_row_off(shape, dtype):
    x, wt, offs = _mutation_ops(shape, 1)
    B, Cin, H, W, Cout = shape
    ref = CA.conv_ref(x, wt, offs, 1, 1, H, W, dtype)
    xm = torch.cat([x[:, :1], x], 1)                                        # reads above the image land on row 1 instead of row 0 ...
    xm[:, 0] = x[:, 1]
    got = CA.conv_sum(xm, wt, [(dy + 1, dx) for dy, dx in offs], 1, 1, H, W)[0]      # ... every in-range read is the same
    assert torch.equal(got[:, 2:], ref['exact'][:, 2:])
    assert CA.ratio(round_to(got, dtype), ref) > 1.0


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
@pytest.mark.parametrize('shape', SHAPES)
def test_bound_rejects_bias_applied_after_scale(shape, dtype):
    x, wt, offs = _mutation_ops(shape, 0)
    B, Cin, H, W, Cout = shape
    b, s, h = CA._vec(Cout, 3, 'bias'), CA._vec(Cout, 4, 'scale'), CA._vec(Cout, 5, 'shift')
    ref = CA.conv_ref(x, wt, offs, 1, 0, H, W, dtype, b, s, h, True)
    got = (ref['v'] * s + b + h).clamp_min(0)
    assert CA.ratio(round_to(got, dtype), ref) > 1.0
