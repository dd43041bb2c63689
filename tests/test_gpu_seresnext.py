"""GPU tests of UNetSeResNetXt (SE-ResNeXt encoders on csrc/conv_group.hip): the grouped 3x3 convolution, its data gradient and its
weight gradient through the C-ABI against the float64 reference of gconv_op_reference.py, elementwise and with no element excluded
(both dtypes; eval epilogue, raw output + statistics in both protocols; accumulate 0 and 1; contiguous views and channel-slice views
between sentinels), bit-identical runs under the fixed summation order, the F18 bottleneck and network fixtures, hipGraph replay and
the trainer.

Operator bound (gconv_op_reference.py; derived, not measured): operands are bf16-representable, every product is exact in fp32,
tol = K 2^-23 sum |x||w| per element with K = 9 Cg (forward, data gradient) or the number of summed pixels (weight gradient), scaled by
|scale| plus 4 * 2^-23 * (largest epilogue intermediate) for the eval epilogue, plus 2^-8 (|value| + tol) per bf16 storage rounding.
Statistics are held to the float64 moments of the stored output (conv_abi.moments)."""
import ctypes
import functools

import pytest
import torch

from helpers import golden, T, assert_close, rel_err
import abi_ops
import closed_form as CF
import gconv_op_reference as GR
import net_checks as NC
import seresnext_oracle as SX
from abi_ops import Act, Vec, raw, call, _abi, merge_partials, check_moments, DEV, F64, SENTINEL

pytestmark = pytest.mark.gpu
TOL32, TOLBF = 5e-5, 4e-2                   # tests/test_gpu_blocks.py: the F2 / F4 block bounds
CODE = {'f32': 0, 'bf16': 1}
_CASES = {}
RATIOS = {}          # {(shape, dtype): {output: worst error / bound}}: the table of DESIGN 17
held = functools.partial(abi_ops.held, ratio=GR.ratio, ratios=RATIOS)


def case_of(shape):
    if shape not in _CASES:
        B, H, W, C, stride = shape
        _CASES[shape] = GR.make_case(B, H, W, C, stride, seed=100 + C + 7 * H + stride)
    return _CASES[shape]


_REFS = {}


def ref_of(shape, dtype, what, flag):
    """the float64 reference of one (shape, dtype, output, variant): computed once, shared, left unchanged"""
    key = (shape, dtype, what, flag)
    if key not in _REFS:
        c = case_of(shape)
        _REFS[key] = (GR.forward_ref(c, dtype, flag, flag) if what == 'fwd' else GR.dgrad_ref(c, dtype, flag) if what == 'dgrad'
                      else GR.wgrad_ref(c, flag))
    return _REFS[key]


def run_forward(shape, dtype, sliced, form):
    """form: 'eval' (scale / shift / relu), 'partials', 'shards' -> the stored output (float64) and what the launch reported"""
    abi = _abi()
    B, H, W, C, stride = shape
    c = case_of(shape)
    OH, OW = GR.out_size(H, stride), GR.out_size(W, stride)
    what = 'gconv %s %s sliced=%d %s' % (shape, dtype, sliced, form)
    x = Act(c['x'], dtype, sliced)
    y = Act(torch.full((B, OH, OW, C), float('nan'), dtype=F64), dtype, sliced)
    w = c['w'].float().contiguous().to(DEV)
    x0 = x.buf.clone()
    kw = dict(dtype=CODE[dtype], x=x.view, w=w.data_ptr(), groups=32, stride=stride, y=y.view)
    nparts = abi.lib.salt_gconv_stats_parts(ctypes.byref(abi.fill(abi.STRUCTS['salt_gconv_args'](), **kw)))
    assert nparts == B * -(-OH // 8) * -(-OW // 8)
    out = {}
    if form == 'eval':
        sc, sh = c['scale'].float().to(DEV), c['shift'].float().to(DEV)
        call('salt_gconv', scale=sc.data_ptr(), shift=sh.data_ptr(), relu=1, **kw)
    elif form == 'partials':
        nf = abi.lib.salt_bn_stats_floats(nparts, C)
        assert nf >= nparts * 2 * C
        stats, cnt = Vec(nf), Vec(nparts)
        call('salt_gconv', stats=stats.ptr(), stats_cnt=cnt.ptr(), **kw)
        out['stats'] = stats.get((nf,))[:nparts * 2 * C].reshape(nparts, 2, C)
        out['cnt'] = cnt.get((nparts,))
    else:
        acc = Vec(8 * (2 * C + 1), fill=0.0, dtype=F64)
        call('salt_gconv', fin_acc=acc.ptr(), **kw)
        out['acc'] = acc.get((8, 2 * C + 1))
    y.check(what + ' y')
    assert torch.equal(x.buf.view(torch.int16), x0.view(torch.int16)), what + ': input changed'
    got = y.get()
    held(got, ref_of(shape, dtype, 'fwd', form == 'eval'), what, (shape, dtype), 'y eval' if form == 'eval' else 'y')
    if form == 'partials':
        check_moments(what, got, dtype, *merge_partials(out['stats'], out['cnt']))
    elif form == 'shards':
        a = out['acc'].sum(0)
        check_moments(what, got, dtype, float(a[2 * C]), a[:C], a[C:2 * C])
    out['y'] = got
    return out


def run_dgrad(shape, dtype, sliced, accumulate):
    B, H, W, C, stride = shape
    c = case_of(shape)
    what = 'gconv_dgrad %s %s sliced=%d acc=%d' % (shape, dtype, sliced, accumulate)
    dy = Act(c['dy'], dtype, sliced)
    dx = Act(c['dx_old'] if accumulate else torch.full((B, H, W, C), float('nan'), dtype=F64), dtype, sliced)
    w = c['w'].float().contiguous().to(DEV)
    d0 = dy.buf.clone()
    call('salt_gconv_dgrad', dtype=CODE[dtype], dy=dy.view, w=w.data_ptr(), groups=32, stride=stride, dx=dx.view, accumulate=accumulate)
    dx.check(what)
    assert torch.equal(dy.buf.view(torch.int16), d0.view(torch.int16)), what + ': dy changed'
    got = dx.get()
    held(got, ref_of(shape, dtype, 'dgrad', accumulate), what, (shape, dtype), 'dx acc' if accumulate else 'dx')
    return got


def run_wgrad(shape, dtype, sliced, accumulate):
    abi = _abi()
    B, H, W, C, stride = shape
    Cg = C // 32
    c = case_of(shape)
    what = 'gconv_wgrad %s %s sliced=%d acc=%d' % (shape, dtype, sliced, accumulate)
    x, dy = Act(c['x'], dtype, sliced), Act(c['dy'], dtype, sliced)
    kw = dict(dtype=CODE[dtype], x=x.view, dy=dy.view, groups=32, stride=stride)
    ns = abi.lib.salt_gconv_wgrad_parts(ctypes.byref(abi.fill(abi.STRUCTS['salt_gconv_wgrad_args'](), **kw)))
    assert ns >= 1
    part = Vec(ns * C * Cg * 9)
    grad = Vec(C * Cg * 9)
    if accumulate:
        grad.win.copy_(c['gw_old'].float().reshape(-1))
    call('salt_gconv_wgrad', partials=part.ptr(), nsplit=ns, grad=grad.ptr(), accumulate=accumulate, **kw)
    x.check(what + ' x')
    dy.check(what + ' dy')
    assert bool(torch.isfinite(part.get((ns, C * Cg * 9))).all()), what + ': a slab element was not written'
    got = grad.get((C, Cg, 3, 3))
    held(got, ref_of(shape, 'f32', 'wgrad', accumulate), what, (shape, dtype), 'gw acc' if accumulate else 'gw')
    return got


@pytest.mark.parametrize('shape', GR.SHAPES, ids=['x'.join(str(v) for v in s) for s in GR.SHAPES])
@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_gconv_vs_fp64_reference(dtype, shape):
    for sliced in (0, 1):
        for form in ('eval', 'partials', 'shards'):
            run_forward(shape, dtype, sliced, form)
        for accumulate in (0, 1):
            run_dgrad(shape, dtype, sliced, accumulate)
            run_wgrad(shape, dtype, sliced, accumulate)
    per = RATIOS[(shape, dtype)]
    print('worst error / bound of %s %s: %.3f  per output:' % (shape, dtype, max(per.values())), {k: round(v, 3) for k, v in sorted(per.items())})


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_fixed_order_sums_are_bit_identical(dtype, deterministic_sums):
    """the weight gradient (slabs added in ascending split order) and the statistics by partials: two runs, the same bits"""
    for shape in ((1, 34, 18, 128, 1), (1, 16, 16, 512, 2)):
        a, b = run_wgrad(shape, dtype, 1, 0), run_wgrad(shape, dtype, 1, 0)
        assert torch.equal(a, b), shape
        p, q = run_forward(shape, dtype, 0, 'partials'), run_forward(shape, dtype, 0, 'partials')
        assert torch.equal(p['stats'], q['stats']) and torch.equal(p['cnt'], q['cnt']) and torch.equal(p['y'], q['y']), shape


def test_unsupported_shapes_fail_loudly_and_launch_nothing():
    abi = _abi()
    from salt_amd.engine import shaped_view
    UNS, BAD = abi.CONSTS['SALT_E_UNSUPPORTED'], abi.CONSTS['SALT_E_BADARG']

    def attempt(C, stride=1, groups=32, dtype=0, off=0, **over):
        B, H, W = 2, 3, 3
        x = torch.randn(B * H * W * C + 64, device=DEV)
        y = torch.full((B, H, W, C), SENTINEL, device=DEV)
        w = torch.randn(C * max(C // 32, 1) * 9, device=DEV)
        kw = dict(dtype=dtype, x=shaped_view(x.data_ptr() + off, B, H, W, C), w=w.data_ptr(), groups=groups, stride=stride,
                  y=shaped_view(y.data_ptr(), B, (H - 1) // max(stride, 1) + 1, (W - 1) // max(stride, 1) + 1, C))
        kw.update(over)
        rc = raw('salt_gconv', **kw)
        return rc, bool((y == SENTINEL).all())
    assert attempt(128) == (0, False)
    for args in ((96,), (2048,), (128, 3), (128, 1, 16)):
        rc, untouched = attempt(*args)
        assert rc == UNS and untouched and abi.lib.salt_last_error(), args
    assert attempt(128, off=4) == (BAD, True)
    assert attempt(128, w=None) == (BAD, True)
    assert attempt(128, dtype=7) == (BAD, True)
    assert attempt(128, relu=1, fin_acc=1 << 20) == (BAD, True)


# ------------------------------------------------------------------------------------------------ the bottleneck through the graph
BLOCKS = {'F18_sx_bottleneck': (64, 64, 1, 256, 'f18a'), 'F18_sx_bottleneck_s2': (256, 128, 2, 512, 'f18b')}


def _block(name, fx):
    from torch import nn
    from salt_amd import architectures as A
    cin, planes, stride, cout, _ = BLOCKS[name]
    down = nn.Sequential(nn.Conv2d(cin, cout, kernel_size=1, stride=stride, padding=0, bias=False), nn.BatchNorm2d(cout))
    m = A.SEResNeXtBottleneck(cin, planes, 32, 16, stride, down)
    sd = {k: CF.tensor_for(k, v.shape).to(v.dtype) for k, v in m.state_dict().items()}
    sd['se_module.fc2.weight'] = sd['se_module.fc2.weight'] * float(fx['fc2_scale'])
    m.load_state_dict(sd)
    return m, sd


def _block_io(name, fx):
    shape = tuple(int(v) for v in fx['x_shape'])
    x = T(fx['x']) if 'x' in fx else CF.input_for(BLOCKS[name][4], shape)
    gy = T(fx['gy']) if 'gy' in fx else CF.input_for('gy:%s' % (tuple(fx['y'].shape),), fx['y'].shape)
    return x, gy


def _emulated_block(name, sd, x, gy):
    """the test-side oracle block with bf16 storage emulated: the yardstick of the bf16 backward bound (tests/test_gpu_blocks.py)"""
    from oracle import blocks as OB
    s2 = {k: v.clone() for k, v in sd.items()}
    leaves = [k for k, v in s2.items() if v.dtype.is_floating_point and not k.endswith(('running_mean', 'running_var'))]
    for k in leaves:
        s2[k].requires_grad_(True)
    xr = x.clone().requires_grad_(True)
    with OB.bf16_storage():
        y = SX.sx_bottleneck(s2, '', OB._st(xr), True, BLOCKS[name][2])
        y.backward(gy)
    out = {'gx': xr.grad}
    for k in leaves:
        out['g:' + k] = s2[k].grad if s2[k].grad is not None else torch.zeros_like(s2[k])
    return out


@pytest.mark.parametrize('name', sorted(BLOCKS))
@pytest.mark.parametrize('mode', ['train', 'eval'])
@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_bottleneck_vs_golden(name, mode, dtype):
    """forward, input gradient, parameter gradients and running statistics with the bounds of
    tests/test_gpu_blocks.py::test_block_vs_reference_golden (5e-5 f32, 4e-2 bf16)"""
    from gpu_harness import BlockRun
    fx = SX.block_fixture(golden, '%s_%s' % (name, mode))
    m, sd = _block(name, fx)
    x, gy = _block_io(name, fx)
    train = mode == 'train'
    m.train(train)
    run = BlockRun(m, [x], lambda g, a: m.emit(g, a), train=train, dtype=dtype)
    tol = TOL32 if dtype == 'f32' else TOLBF
    y = run.forward()
    assert_close(y, fx['y'], tol, 'y')
    ops = [o[0] for o in run.g.fwd.ops]
    assert ops.count('gconv') == 1 and ops.count('se_res') == 1
    if not train:
        return
    bops = [(o[0], s) for o, s in zip(run.g.bwd.ops, run.g.bwd.streams)]
    assert [o for o, _ in bops].count('gconv_dgrad') == 1 and ('gconv_wgrad', 1) in bops          # the weight gradient rides the side stream
    gx, grads = run.backward(gy.to(DEV))
    emu = None if dtype == 'f32' else _emulated_block(name, sd, x, gy)

    def check(got, ref, key, f32_tol):
        if emu is None:
            assert_close(got, ref, f32_tol, key)
        else:
            e_hip, e_emu = rel_err(got, ref), rel_err(emu[key], ref)
            assert e_hip <= 1.5 * e_emu + 2e-2, '%s: HIP bf16 %.3e from the golden, bf16-storage emulation %.3e' % (key, e_hip, e_emu)
    check(gx[0], fx['gx'], 'gx', tol * 2)
    assert set(grads) == {k for k, _ in m.named_parameters()}
    for k, g in grads.items():
        check(g, fx['g:' + k], 'g:' + k, tol * 3)
    sd2 = m.state_dict()
    for k in sd2:
        if k.endswith(('running_mean', 'running_var')):
            assert_close(sd2[k].cpu(), fx['s:' + k], tol, k)


@pytest.mark.parametrize('fin', ['0', '1'])
def test_bottleneck_partials_protocols_agree_with_golden(fin, monkeypatch):
    """SALT_BN_FIN=0 / =1: the grouped layer's statistics travel as per-tile partials + bn_finalize; same fixture, same bounds; under
    the fixed order a second backward run gives the same bits"""
    from gpu_harness import BlockRun
    monkeypatch.setenv('SALT_BN_FIN', fin)
    monkeypatch.setenv('SALT_SE_SHARDS', '0')
    name = 'F18_sx_bottleneck_s2'
    fx = SX.block_fixture(golden, name + '_train')
    m, sd = _block(name, fx)
    x, gy = _block_io(name, fx)
    m.train()
    run = BlockRun(m, [x], lambda g, a: m.emit(g, a), train=True, dtype='f32')
    assert_close(run.forward(), fx['y'], TOL32, 'y')
    ops = [o[0] for o in run.g.fwd.ops]
    assert ops[ops.index('gconv') + 1] == 'bn_finalize'
    gx, grads = run.backward(gy.to(DEV))
    assert_close(gx[0], fx['gx'], 2 * TOL32, 'gx')
    for k, g in grads.items():
        assert_close(g, fx['g:' + k], 3 * TOL32, 'g:' + k)
    if fin == '0':
        gx2, grads2 = run.backward(gy.to(DEV))
        assert torch.equal(gx[0], gx2[0]) and all(torch.equal(grads[k], grads2[k]) for k in grads)


# ------------------------------------------------------------------------------------------------ whole network
def _net(depth, fx, dtype='f32'):
    from salt_amd import architectures as A
    net = NC.fill_closed_form(A.UNetSeResNetXt(depth, 2, dropout_2d=0.0, pretrained=False, use_hypercolumn=True))
    with torch.no_grad():
        for k, p in net.named_parameters():
            if k.endswith(SX.SO.FC2_KEY):
                p.mul_(float(fx['fc2_scale']))
    return net.set_compute_dtype(dtype).to(DEV)


@pytest.mark.parametrize('name,depth', [('F18_unet_seresnext50_hyper', 50), ('F18_unet_seresnext101_hyper', 101)])
def test_eval_logits_and_masks_match_reference(name, depth):
    fx = golden(name)
    x = T(fx['x']).to(DEV)
    net = _net(depth, fx).eval()
    with torch.no_grad():
        logits = net(x).cpu()
    NC.check_eval_masks(logits, fx, 'seresnext eval ' + name, logits_tol=1e-3)
    cn = net.engine().net(tuple(x.shape), False)
    ops = [o[0] for o in cn.fwd.ops]
    assert ops.count('gconv') == ops.count('se_res') == sum(SX.COUNTS[depth])
    if depth != 50:
        return
    NC.check_eval_graph_replay(cn, x, logits)
    NC.check_bf16_eval_guard(_net(depth, fx, 'bf16').eval(), x, logits, fx, 'seresnext eval bf16 ' + name, guard_factor=4)


def test_one_training_step_matches_reference():
    """zero_grad -> forward -> lovasz -> backward -> Adam(lr 1e-4, L2 1e-4) as models.py:105-136, by the procedures of
    tests/net_checks.py with the bounds tests/test_gpu_seresnet.py uses for F17: gradient norms (and sums) of tensors with 16 elements
    and more within 1e-2 relative, tensors under 16 elements within 1e-6 of the largest gradient norm."""
    fx = golden('F18_unet_seresnext50_hyper')
    assert float(fx['ref_f32_vs_f64_gradnorm_rel']) <= 2.5e-3 and float(fx['ref_f32_vs_f64_small_abs']) <= 2.5e-7
    net = _net(50, fx)
    net.train()
    opt, out, eng, own, idx = NC.train_step_prologue(net, [T(fx['x']).to(DEV)], fx, logits_tol=2e-3, loss_tol=2e-3)
    cn = eng.net(tuple(fx['x'].shape), True)
    ops = [o[0] for o in cn.fwd.ops]
    bops = [o[0] for o in cn.bwd.ops]
    assert ops.count('gconv') == 16 and ops.count('se_res') == 16 and bops.count('gconv_dgrad') == 16 and bops.count('gconv_wgrad') == 16
    # small tensors (every one under 16 elements: the absolute bound needs no norm): five spatial-SE biases and the two-element head bias
    NC.check_grad_tally(net, eng, own, idx, fx, 'seresnext train:', include_small_below_norm_floor=True, min_checked=200, n_small=6,
                        norm_tol=1e-2, sum_tol=1e-2, small_tol=1e-6, verbose=False)
    full = [k[9:] for k in fx if k.startswith('fullgrad:')]
    assert len(full) == 8
    NC.check_full_grads(eng, own, fx, full, tol=2e-2, verbose=False)
    NC.check_after_adam(opt, net, own, idx, fx, norm_tol=1e-4, sum_tol=1e-4, bn_tol=1e-3, skip_bn=None)


# ------------------------------------------------------------------------------------------------ trainer
def _model(dtype='bf16', lr=1e-3, cfg=None):
    return NC.family_model('UNetSeResNetXt', dtype, lr, 1, cfg)


def test_step_graph_replay_equals_eager_steps(deterministic_sums):
    """the procedure of tests/net_checks.py::step_graph_equals_eager at [2,3,64,64]: the training step with its 48 grouped-convolution
    entries captured into ONE hipGraph (two-stream forward and backward, loss, Adam) and replayed reproduces the eagerly launched steps
    bit for bit under the fixed summation order"""
    NC.step_graph_equals_eager(_model, lambda: NC.noise_batch(5, 2, 64), steps=4)


def test_fit_two_steps():
    """SegmentationModel.fit for two steps at [2,3,64,64]: the unchanged trainer (fused step) on the new architecture"""
    from salt_amd import architectures as A
    m, values = NC.fit_steps(lambda cfg: _model(cfg=cfg), A.UNetSeResNetXt, NC.square_batch(3), 2)
    print('seresnext fit losses', values)
