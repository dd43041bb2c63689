"""GPU tests of the pre-activated 1x1 convolution of the DenseNet encoders (csrc/dense.hip): salt_dense_conv, its data gradient
(with the BatchNorm backward of the consumer-owned norm) and its weight gradient through the C-ABI against the float64 references
of dense_op_reference.py, elementwise and with no element excluded (both dtypes; eval epilogue, raw output + statistics partials,
no epilogue; accumulate 0 and 1; contiguous views and prefix / slice views of a wider buffer between sentinels, inputs verified
unchanged), bit-identical reruns under the fixed summation order, the shapes the contract refuses, and UNetDenseNet(121) against the F19 fixture the
reference produced (eval logits and masks, hipGraph replay, bf16 storage, one training step, the step graph, the trainer).

Operator bound (dense_op_reference.py; derived, not measured): operands are bf16-representable and the transformed operand is
reproduced exactly, tol = K 2^-23 sum |a||w| per element, scaled by |scale| plus 4 * 2^-23 * (largest epilogue intermediate) for the
eval epilogue, plus 2^-8 (|value| + tol) per bf16 storage rounding; the BatchNorm-backward terms of the data gradient follow from
the two sums' own bounds (derivation in that file).  Statistics are held to the float64 moments of the stored output
(conv_abi.moments)."""
import ctypes
import functools

import pytest
import torch

from helpers import golden, T, assert_close
import abi_ops
import closed_form as CF
import dense_op_reference as DR
import densenet_oracle as DO
import net_checks as NC
from abi_ops import Act, Vec, raw, call, _abi, merge_partials, check_moments, DEV, F64, SENTINEL

pytestmark = pytest.mark.gpu
TOL32, TOLBF = 5e-5, 4e-2                   # tests/test_gpu_blocks.py: the F2 / F4 block bounds
CODE = {'f32': 0, 'bf16': 1}
_CASES, _REFS = {}, {}
RATIOS = {}          # {(shape, dtype): {output: worst error / bound}}: the table of DESIGN 19
held = functools.partial(abi_ops.held, ratio=DR.ratio, ratios=RATIOS)


def case_of(shape):
    if shape not in _CASES:
        B, H, W, Cin, Cout = shape
        _CASES[shape] = DR.make_case(B, H, W, Cin, Cout, seed=300 + Cin + 7 * H + Cout)
    return _CASES[shape]


def ref_of(shape, dtype, what, flag):
    """the float64 reference of one (shape, dtype, output, variant): computed once, shared, left unchanged"""
    key = (shape, dtype, what, flag)
    if key not in _REFS:
        c = case_of(shape)
        if what == 'fwd':
            _REFS[key] = DR.forward_ref(c, dtype, flag == 'eval', flag == 'eval')
        elif what == 'dgrad':
            _REFS[key] = DR.dgrad_ref(c, dtype, flag)
        else:
            _REFS[key] = DR.wgrad_ref(c, dtype, flag)
    return _REFS[key]


def dev(c, name):
    return c[name].float().contiguous().to(DEV)


def same_bits(t, t0):
    return torch.equal(t.view(torch.int16), t0.view(torch.int16))


def run_forward(shape, dtype, sliced, form):
    """form: 'eval' (scale / shift / relu), 'partials' (raw output + statistics), 'plain' (no epilogue: a transition in eval mode)"""
    abi = _abi()
    B, H, W, Cin, Cout = shape
    c = case_of(shape)
    what = 'dense_conv %s %s sliced=%d %s' % (shape, dtype, sliced, form)
    x = Act(c['x'], dtype, sliced)
    y = Act(torch.full((B, H, W, Cout), float('nan'), dtype=F64), dtype, sliced)
    w, isc, ish = dev(c, 'w'), dev(c, 'in_scale'), dev(c, 'in_shift')
    x0 = x.buf.clone()
    kw = dict(dtype=CODE[dtype], x=x.view, in_scale=isc.data_ptr(), in_shift=ish.data_ptr(), w=w.data_ptr(), y=y.view)
    nparts = abi.lib.salt_dense_conv_stats_parts(ctypes.byref(abi.fill(abi.STRUCTS['salt_dense_conv_args'](), **kw)))
    assert nparts == -(-(B * H * W) // 128)
    out = {}
    if form == 'eval':
        sc, sh = dev(c, 'scale'), dev(c, 'shift')
        call('salt_dense_conv', scale=sc.data_ptr(), shift=sh.data_ptr(), relu=1, **kw)
    elif form == 'partials':
        nf = abi.lib.salt_bn_stats_floats(nparts, Cout)
        assert nf >= nparts * 2 * Cout
        stats, cnt = Vec(nf), Vec(nparts)
        call('salt_dense_conv', stats=stats.ptr(), stats_cnt=cnt.ptr(), **kw)
        out['stats'] = stats.get((nf,))[:nparts * 2 * Cout].reshape(nparts, 2, Cout)
        out['cnt'] = cnt.get((nparts,))
    else:
        call('salt_dense_conv', **kw)
    y.check(what + ' y')
    x.check(what + ' x')
    assert same_bits(x.buf, x0), what + ': input changed'
    got = y.get()
    held(got, ref_of(shape, dtype, 'fwd', 'eval' if form == 'eval' else 'raw'), what, (shape, dtype), 'y eval' if form == 'eval' else 'y')
    if form == 'partials':
        check_moments(what, got, dtype, *merge_partials(out['stats'], out['cnt']))
    out['y'] = got
    return out


def run_dgrad(shape, dtype, sliced, accumulate):
    abi = _abi()
    B, H, W, Cin, Cout = shape
    c = case_of(shape)
    what = 'dense_conv_dgrad %s %s sliced=%d acc=%d' % (shape, dtype, sliced, accumulate)
    dy, x = Act(c['dy'], dtype, sliced), Act(c['x'], dtype, sliced)
    dx = Act(c['dx_old'] if accumulate else torch.full((B, H, W, Cin), float('nan'), dtype=F64), dtype, sliced)
    keep = [dev(c, k) for k in ('w', 'in_scale', 'in_shift', 'mean', 'invstd', 'gamma')]
    d0, x0 = dy.buf.clone(), x.buf.clone()
    kw = dict(dtype=CODE[dtype], dy=dy.view, w=keep[0].data_ptr(), x=x.view, in_scale=keep[1].data_ptr(), in_shift=keep[2].data_ptr(),
              mean=keep[3].data_ptr(), invstd=keep[4].data_ptr(), gamma=keep[5].data_ptr(), dx=dx.view, accumulate=accumulate)
    nparts = abi.lib.salt_dense_conv_dgrad_parts(ctypes.byref(abi.fill(abi.STRUCTS['salt_dense_conv_dgrad_args'](), **kw)))
    assert nparts == -(-(B * H * W) // 128)
    part, sums, dgam, dbet = Vec(nparts * 2 * Cin), Vec(2 * Cin), Vec(Cin), Vec(Cin)
    call('salt_dense_conv_dgrad', partials=part.ptr(), nparts=nparts, sums=sums.ptr(), dgamma=dgam.ptr(), dbeta=dbet.ptr(), accumulate_param_grads=0, **kw)
    dx.check(what)
    dy.check(what + ' dy')
    x.check(what + ' x')
    assert same_bits(dy.buf, d0) and same_bits(x.buf, x0), what + ': an input changed'
    assert bool(torch.isfinite(part.get((nparts, 2, Cin))).all()), what + ': a partial was not written'
    ref = ref_of(shape, dtype, 'dgrad', accumulate)
    out = dict(dx=dx.get(), dbeta=dbet.get((Cin,)), dgamma=dgam.get((Cin,)))
    held(out['dbeta'], ref['dbeta'], what + ' dbeta', (shape, dtype), 'dbeta')
    held(out['dgamma'], ref['dgamma'], what + ' dgamma', (shape, dtype), 'dgamma')
    assert torch.equal(sums.get((2, Cin)), torch.stack([out['dbeta'], out['dgamma']])), what + ': sums and the parameter gradients differ'
    held(out['dx'], ref, what, (shape, dtype), 'dx acc' if accumulate else 'dx')
    return out


def run_wgrad(shape, dtype, sliced, accumulate):
    abi = _abi()
    B, H, W, Cin, Cout = shape
    c = case_of(shape)
    what = 'dense_conv_wgrad %s %s sliced=%d acc=%d' % (shape, dtype, sliced, accumulate)
    x, dy = Act(c['x'], dtype, sliced), Act(c['dy'], dtype, sliced)
    isc, ish = dev(c, 'in_scale'), dev(c, 'in_shift')
    x0, d0 = x.buf.clone(), dy.buf.clone()
    kw = dict(dtype=CODE[dtype], x=x.view, in_scale=isc.data_ptr(), in_shift=ish.data_ptr(), dy=dy.view)
    ns = abi.lib.salt_dense_conv_wgrad_parts(ctypes.byref(abi.fill(abi.STRUCTS['salt_dense_conv_wgrad_args'](), **kw)))
    assert ns >= 1
    part, grad = Vec(ns * Cout * Cin), Vec(Cout * Cin)
    if accumulate:
        grad.win.copy_(c['gw_old'].float().reshape(-1))
    call('salt_dense_conv_wgrad', partials=part.ptr(), nsplit=ns, grad=grad.ptr(), accumulate=accumulate, **kw)
    x.check(what + ' x')
    dy.check(what + ' dy')
    assert same_bits(x.buf, x0) and same_bits(dy.buf, d0), what + ': an input changed'
    assert bool(torch.isfinite(part.get((ns, Cout * Cin))).all()), what + ': a slab element was not written'
    got = grad.get((Cout, Cin))
    held(got, ref_of(shape, dtype, 'wgrad', accumulate), what, (shape, dtype), 'gw acc' if accumulate else 'gw')
    return got


@pytest.mark.parametrize('shape', DR.SHAPES, ids=['x'.join(str(v) for v in s) for s in DR.SHAPES])
@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_dense_conv_vs_fp64_reference(dtype, shape):
    for sliced in (0, 1):
        for form in ('eval', 'partials', 'plain'):
            run_forward(shape, dtype, sliced, form)
        for accumulate in (0, 1):
            run_dgrad(shape, dtype, sliced, accumulate)
            run_wgrad(shape, dtype, sliced, accumulate)
    per = RATIOS[(shape, dtype)]
    print('worst error / bound of %s %s: %.3f  per output:' % (shape, dtype, max(per.values())), {k: round(v, 3) for k, v in sorted(per.items())})


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_fixed_order_sums_are_bit_identical(dtype, deterministic_sums):
    """weight gradient (slabs added in ascending split order), the data gradient's sums and the statistics partials: two runs, the same bits"""
    for shape in ((1, 34, 18, 160, 128), (2, 6, 10, 256, 128)):
        a, b = run_wgrad(shape, dtype, 1, 0), run_wgrad(shape, dtype, 1, 0)
        assert torch.equal(a, b), shape
        p, q = run_dgrad(shape, dtype, 1, 0), run_dgrad(shape, dtype, 1, 0)
        assert all(torch.equal(p[k], q[k]) for k in ('dx', 'dbeta', 'dgamma')), shape
        p, q = run_forward(shape, dtype, 0, 'partials'), run_forward(shape, dtype, 0, 'partials')
        assert torch.equal(p['stats'], q['stats']) and torch.equal(p['cnt'], q['cnt']) and torch.equal(p['y'], q['y']), shape


def test_unsupported_shapes_fail_loudly_and_launch_nothing():
    abi = _abi()
    from salt_amd.engine import shaped_view
    UNS, BAD = abi.CONSTS['SALT_E_UNSUPPORTED'], abi.CONSTS['SALT_E_BADARG']

    def attempt(Cin, Cout, dtype=0, off=0, **over):
        B, H, W = 2, 3, 3
        x = torch.randn(B * H * W * Cin + 64, device=DEV)
        y = torch.full((B, H, W, Cout), SENTINEL, device=DEV)
        w = torch.randn(Cout * Cin, device=DEV)
        sc, sh = torch.ones(Cin, device=DEV), torch.zeros(Cin, device=DEV)
        kw = dict(dtype=dtype, x=shaped_view(x.data_ptr() + off, B, H, W, Cin), in_scale=sc.data_ptr(), in_shift=sh.data_ptr(), w=w.data_ptr(),
                  y=shaped_view(y.data_ptr(), B, H, W, Cout))
        kw.update(over)
        parts = abi.lib.salt_dense_conv_stats_parts(ctypes.byref(abi.fill(abi.STRUCTS['salt_dense_conv_args'](), **kw)))
        rc = raw('salt_dense_conv', **kw)
        return rc, bool((y == SENTINEL).all()), parts
    assert attempt(64, 128) == (0, False, 1)
    for args in ((48, 128), (2080, 128), (64, 96), (64, 1088), (16, 128)):
        rc, untouched, parts = attempt(*args)
        assert rc == UNS and untouched and parts < 0 and abi.lib.salt_last_error(), args
    assert attempt(64, 128, off=4)[:2] == (BAD, True)
    assert attempt(64, 128, w=None)[:2] == (BAD, True)
    assert attempt(64, 128, in_scale=None)[:2] == (BAD, True)
    assert attempt(64, 128, dtype=7)[:2] == (BAD, True)
    assert attempt(64, 128, relu=1, stats=1 << 20, stats_cnt=1 << 20)[:2] == (BAD, True)

    # the gradients refuse the same shapes before they touch anything
    for name, extra in (('salt_dense_conv_dgrad', {}), ('salt_dense_conv_wgrad', {})):
        S = abi.STRUCTS[name + '_args']
        for Cin, Cout in ((48, 128), (2080, 128), (64, 96)):
            a = abi.fill(S(), dtype=0, x=shaped_view(1 << 20, 2, 3, 3, Cin), dy=shaped_view(1 << 20, 2, 3, 3, Cout))
            assert getattr(abi.lib, name + '_parts')(ctypes.byref(a)) < 0
            assert raw(name, dtype=0, x=shaped_view(1 << 20, 2, 3, 3, Cin), dy=shaped_view(1 << 20, 2, 3, 3, Cout)) == UNS


# ------------------------------------------------------------------------------------------------ denseblock1 + transition1 through the graph
class _BlockT(torch.nn.Module):
    """denseblock1 + transition1 of depth 121 from the package's own modules, keys as the fixture generator's DenseBlockT"""

    def __init__(self):
        from salt_amd import architectures as A
        super().__init__()
        self.block = A._DenseBlock(6, 64, 4, 32, 0)
        self.transition = A._Transition(256, 128)

    def emit(self, g, a):
        buf = g.new_act(a.B, a.H, a.W, 256, 'block')
        g.copy(a, buf.slice(0, 64))
        table = g.dense_table(buf) if g.train else None
        if g.train:
            g.dense_moments(buf.slice(0, 64), table, 0)
        c = 64
        for layer in self.block.children():
            layer.emit(g, buf, c, table)
            c += 32
        return self.transition.emit(g, buf, table, None)


def _block_state(m):
    return {k: CF.tensor_for(k, v.shape).to(v.dtype) for k, v in m.state_dict().items()}


def _emulated_dense_block(sd, x, gy):
    """the test-side oracle block with bf16 storage emulated: the yardstick of the bf16 backward bound (tests/test_gpu_blocks.py)"""
    from oracle import blocks as OB
    s2 = {k: v.clone() for k, v in sd.items()}
    leaves = [k for k, v in s2.items() if v.dtype.is_floating_point and not k.endswith(('running_mean', 'running_var'))]
    for k in leaves:
        s2[k].requires_grad_(True)
    xr = x.clone().requires_grad_(True)
    with OB.bf16_storage():
        y = DO.transition(s2, 'transition.', DO.dense_block(s2, 'block.', OB._st(xr), True, 6), True)
        y.backward(gy)
    out = {'gx': xr.grad}
    for k in leaves:
        out['g:' + k] = s2[k].grad if s2[k].grad is not None else torch.zeros_like(s2[k])
    return out


@pytest.mark.parametrize('mode', ['train', 'eval'])
@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_dense_block_vs_golden(mode, dtype):
    """six layers that share one statistics table and accumulate into one gradient buffer, then the 256 -> 128 transition and the pool:
    forward, input gradient, parameter gradients and every layer's running statistics with the bounds of
    tests/test_gpu_blocks.py::test_block_vs_reference_golden (5e-5 f32, 2x / 3x for input / parameter gradients; bf16 against the
    bf16-storage emulation by the 1.5 e_emu + 2e-2 rule)"""
    from gpu_harness import BlockRun
    from helpers import rel_err
    fx = golden('F19_dense_block_%s' % mode)
    m = _BlockT()
    sd = _block_state(m)
    m.load_state_dict(sd)
    x = CF.input_for(str(fx['input_tag']), tuple(int(v) for v in fx['x_shape']))
    gy = CF.input_for('gy:%s' % (tuple(fx['y'].shape),), fx['y'].shape)
    train = mode == 'train'
    m.train(train)
    run = BlockRun(m, [x], lambda g, a: m.emit(g, a), train=train, dtype=dtype)
    tol = TOL32 if dtype == 'f32' else TOLBF
    assert_close(run.forward(), fx['y'], tol, 'y')
    ops = [o[0] for o in run.g.fwd.ops]
    assert ops.count('dense_conv') == 7                                  # one per layer and one for the transition
    assert ops.count('affine_act') == (6 if train else 0)                # norm2 of the six layers only: no normalised prefix copy
    if not train:
        assert 'bn_finalize' not in ops and 'dense_moments' not in ops
        return
    assert ops.count('dense_moments') == 1 and ops.count('dense_bn_prep') == 7
    bops = [(o[0], s) for o, s in zip(run.g.bwd.ops, run.g.bwd.streams)]
    assert [o for o, _ in bops].count('dense_conv_dgrad') == 7 and [s for o, s in bops if o == 'dense_conv_wgrad'] == [1] * 7      # side stream
    gx, grads = run.backward(gy.to(DEV))
    emu = None if dtype == 'f32' else _emulated_dense_block(sd, x, gy)

    def check(got, ref, key, f32_tol):
        if emu is None:
            assert_close(got, ref, f32_tol, key)
        else:
            e_hip, e_emu = rel_err(got, ref), rel_err(emu[key], ref)
            assert e_hip <= 1.5 * e_emu + 2e-2, '%s: HIP bf16 %.3e from the golden, bf16-storage emulation %.3e' % (key, e_hip, e_emu)
    check(gx[0], fx['gx'], 'gx', tol * 2)
    assert set(grads) == {k for k, _ in m.named_parameters()}
    full = 0
    for k, g in grads.items():
        if 'g:' + k in fx:
            check(g, fx['g:' + k], 'g:' + k, tol * 3)
            full += 1
        else:                                                            # conv2.weight of the layers 2 .. 5: norm and sum (the fixture stays under 1 MiB)
            gn, gs, n = float(fx['gn:' + k]), float(fx['gs:' + k]), g.numel()
            dn, ds = abs(float(g.double().norm()) - gn) / gn, abs(float(g.double().sum()) - gs) / (gn * n ** 0.5)
            if emu is None:
                assert dn <= 3 * tol and ds <= 3 * tol, (k, dn, ds)
            else:                                                        # the emulation's norm and sum against the FIXTURE's, as the elementwise branch does
                e = emu['g:' + k].double()
                en, es = abs(float(e.norm()) - gn) / gn, abs(float(e.sum()) - gs) / (gn * n ** 0.5)
                assert dn <= 1.5 * en + 2e-2 and ds <= 1.5 * es + 2e-2, (k, dn, en, ds, es)
    assert full == len(grads) - 4
    sd2 = m.state_dict()
    seen = 0
    for k in sd2:
        if k.endswith(('running_mean', 'running_var')):
            assert_close(sd2[k].cpu(), fx['s:' + k], tol, k)
            seen += 1
    assert seen == 2 * 13                                                # norm1 and norm2 of six layers, the transition's norm


# ------------------------------------------------------------------------------------------------ one layer on a 96-channel prefix
def _emit_layer(m):
    """the layer's output IS the 128-wide buffer: its input in the first 96 channels, the 32 new ones behind them.  The statistics table
    and the gradient buffer are wider than the prefix, and 96 is no multiple of the kernels' 64-channel tile."""
    def emit(g, a):
        buf = g.new_act(a.B, a.H, a.W, 128, 'block')
        g.copy(a, buf.slice(0, 96))
        table = g.dense_table(buf) if g.train else None
        if g.train:
            g.dense_moments(buf.slice(0, 96), table, 0)
        m.emit(g, buf, 96, table)
        return buf
    return emit


def _emulated_dense_layer(sd, x, gy):
    from oracle import blocks as OB
    s2 = {k: v.clone() for k, v in sd.items()}
    leaves = [k for k, v in s2.items() if v.dtype.is_floating_point and not k.endswith(('running_mean', 'running_var'))]
    for k in leaves:
        s2[k].requires_grad_(True)
    xr = x.clone().requires_grad_(True)
    with OB.bf16_storage():
        xs = OB._st(xr)
        y = torch.cat([xs, DO.dense_layer(s2, '', xs, True)], 1)
        y.backward(gy)
    out = {'gx': xr.grad}
    for k in leaves:
        out['g:' + k] = s2[k].grad if s2[k].grad is not None else torch.zeros_like(s2[k])
    return out


@pytest.mark.parametrize('mode', ['train', 'eval'])
@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_dense_layer_on_a_prefix_vs_golden(mode, dtype):
    """F19_dense_layer: one layer on a 96-channel prefix of a 128-wide buffer, 189 pixels (two pixel tiles, the second ragged), at the
    bounds of tests/test_gpu_blocks.py::test_block_vs_reference_golden (5e-5 f32, 2x / 3x for input / parameter gradients, running
    statistics; bf16 against the bf16-storage emulation by the 1.5 e_emu + 2e-2 rule)"""
    from gpu_harness import BlockRun
    from helpers import rel_err
    from salt_amd import architectures as A
    fx = golden('F19_dense_layer_%s' % mode)
    m = A._DenseLayer(96, 32, 4, 0)
    sd = _block_state(m)
    m.load_state_dict(sd)
    x = CF.input_for(str(fx['input_tag']), tuple(int(v) for v in fx['x_shape']))
    assert tuple(fx['y'].shape) == (3, 128, 9, 7)
    gy = CF.input_for('gy:%s' % (tuple(fx['y'].shape),), fx['y'].shape)
    train = mode == 'train'
    m.train(train)
    run = BlockRun(m, [x], _emit_layer(m), train=train, dtype=dtype)
    tol = TOL32 if dtype == 'f32' else TOLBF
    assert_close(run.forward(), fx['y'], tol, 'y')
    ops = [o[0] for o in run.g.fwd.ops]
    assert ops.count('dense_conv') == 1 and ops.count('affine_act') == (1 if train else 0)
    if not train:
        return
    assert ops.count('dense_moments') == 1 and ops.count('dense_bn_prep') == 1 and ops.count('bn_finalize') == 3      # two table fills and norm2
    bops = [(o[0], s) for o, s in zip(run.g.bwd.ops, run.g.bwd.streams)]
    assert ('dense_conv_wgrad', 1) in bops and [o for o, _ in bops].count('dense_conv_dgrad') == 1
    dg = [s for (o, _, s) in run.g.bwd.ops if o == 'dense_conv_dgrad'][0]
    assert dg.accumulate == 1 and dg.dx.C == 96 and dg.dx.cs == 128       # adds to the prefix of a wider gradient buffer that the consumer wrote first
    gx, grads = run.backward(gy.to(DEV))
    emu = None if dtype == 'f32' else _emulated_dense_layer(sd, x, gy)

    def check(got, ref, key, f32_tol):
        if emu is None:
            assert_close(got, ref, f32_tol, key)
        else:
            e_hip, e_emu = rel_err(got, ref), rel_err(emu[key], ref)
            assert e_hip <= 1.5 * e_emu + 2e-2, '%s: HIP bf16 %.3e from the golden, bf16-storage emulation %.3e' % (key, e_hip, e_emu)
    check(gx[0], fx['gx'], 'gx', tol * 2)
    assert set(grads) == {k for k, _ in m.named_parameters()} and len(grads) == 6
    for k, g in grads.items():
        check(g, fx['g:' + k], 'g:' + k, tol * 3)
    sd2 = m.state_dict()
    for k in ('norm1.running_mean', 'norm1.running_var', 'norm2.running_mean', 'norm2.running_var'):
        assert_close(sd2[k].cpu(), fx['s:' + k], tol, k)
    assert int(sd2['norm1.num_batches_tracked']) == int(sd['norm1.num_batches_tracked']) + 1


# ------------------------------------------------------------------------------------------------ whole network (F19, closed-form weights)
NET_FX = 'F19_unet_densenet121_hyper'
N_DENSE = sum(DO.CFG[121]) + 3          # one dense_conv per layer and per transition


def _net(dtype='f32'):
    from salt_amd import architectures as A
    net = NC.fill_closed_form(A.UNetDenseNet(121, 2, dropout_2d=0.0, pretrained=False, use_hypercolumn=True))
    return net.set_compute_dtype(dtype).to(DEV)


def _no_prefix_copy(net, cn):
    """no affine_act applies a norm1 or a transition norm, i.e. no normalised copy of a block prefix is ever stored"""
    eng, f = net.engine(), net.encoders.encoder.features
    norms = [l.norm1 for i in (1, 2, 3, 4) for l in getattr(f, 'denseblock%d' % i).children()] + [getattr(f, 'transition%d' % i).norm for i in (1, 2, 3)]
    ptrs = {eng.bn_work(n)['scale'].data_ptr() for n in norms}
    assert len(ptrs) == N_DENSE
    for (op, _, s) in cn.fwd.ops:
        if op == 'affine_act':
            assert s.scale not in ptrs


def test_eval_logits_and_masks_match_reference():
    fx = golden(NET_FX)
    x = T(fx['x']).to(DEV)
    net = _net().eval()
    with torch.no_grad():
        logits = net(x).cpu()
    ref = NC.check_eval_masks(logits, fx, 'densenet eval', logits_tol=1e-3)
    assert ref.any() and not ref.all()
    cn = net.engine().net(tuple(x.shape), False)
    ops = [o[0] for o in cn.fwd.ops]
    assert ops.count('dense_conv') == N_DENSE and 'dense_moments' not in ops and 'dense_bn_prep' not in ops and 'bn_finalize' not in ops
    _no_prefix_copy(net, cn)
    NC.check_eval_graph_replay(cn, x, logits)
    NC.check_bf16_eval_guard(_net('bf16').eval(), x, logits, fx, 'densenet eval bf16', guard_factor=4)


def test_one_training_step_matches_reference():
    """zero_grad -> forward -> lovasz -> backward -> Adam(lr 1e-4, L2 1e-4) as models.py:105-136, by the procedures of
    tests/net_checks.py with the bounds tests/test_gpu_seresnext.py uses for F18: gradient norms (and sums) of tensors with 16 elements
    and more within 1e-2 relative, tensors under 16 elements within 1e-6 of the largest gradient norm."""
    fx = golden(NET_FX)
    assert float(fx['ref_f32_vs_f64_gradnorm_rel']) <= 2.5e-3 and float(fx['ref_f32_vs_f64_small_abs']) <= 2.5e-7
    net = _net()
    net.train()
    opt, out, eng, own, idx = NC.train_step_prologue(net, [T(fx['x']).to(DEV)], fx, logits_tol=2e-3, loss_tol=2e-3)
    cn = eng.net(tuple(fx['x'].shape), True)
    ops = [o[0] for o in cn.fwd.ops]
    bops = [(o[0], s) for o, s in zip(cn.bwd.ops, cn.bwd.streams)]
    names = [o for o, _ in bops]
    assert ops.count('dense_conv') == ops.count('dense_bn_prep') == N_DENSE and ops.count('dense_moments') == 4
    assert names.count('dense_conv_dgrad') == names.count('dense_conv_wgrad') == N_DENSE
    assert all(s == 1 for o, s in bops if o == 'dense_conv_wgrad')          # the weight gradient rides the side stream
    _no_prefix_copy(net, cn)
    # under 16 elements (every one of them: the absolute bound needs no norm): five spatial-SE biases, the five 8-element channel-SE
    # biases of the 128-wide decoder, the two-element head bias
    NC.check_grad_tally(net, eng, own, idx, fx, 'densenet train:', include_small_below_norm_floor=True, min_checked=300, n_small=11,
                        norm_tol=1e-2, sum_tol=1e-2, small_tol=1e-6, verbose=False)
    # full gradients at 2e-2, for every tensor the generator recorded: those whose reference gradient is itself within 5e-3 of float64
    # (the early encoder's are not: transition1.conv.weight of the reference is 1.3e-2 off in fp32, this library 1.9e-2)
    full = fx['fullgrad_keys'].tolist()
    assert len(full) >= 8 and float(fx['fullgrad_ref_f32_vs_f64'].max()) <= 5e-3
    assert any('denselayer' in k and k.endswith('conv1.weight') for k in full) and any(k.endswith('norm1.weight') for k in full)
    assert any(k.endswith('norm1.bias') for k in full) and any('transition' in k and k.endswith('conv.weight') for k in full)
    NC.check_full_grads(eng, own, fx, full, tol=2e-2, verbose=True)
    # every layer's running statistics come out as if it had computed them itself; norm5 is dead in the U-Net: the reference never
    # runs it either
    assert len(fx['bn_keys']) > 2 * N_DENSE
    sd = NC.check_after_adam(opt, net, own, idx, fx, norm_tol=1e-4, sum_tol=1e-4, bn_tol=1e-3, skip_bn='norm5')
    assert int(sd['encoders.encoder.features.denseblock3.denselayer24.norm1.num_batches_tracked']) == 1


# ------------------------------------------------------------------------------------------------ trainer
def _model(dtype='bf16', lr=1e-3, cfg=None):
    return NC.family_model('UNetDenseNet', dtype, lr, 1, cfg)


def test_step_graph_replay_equals_eager_steps(deterministic_sums):
    """the procedure of tests/net_checks.py::step_graph_equals_eager at [2,3,64,64]: the training step captured into ONE hipGraph
    (two-stream forward and backward, loss, Adam) and replayed reproduces the eagerly launched steps bit for bit under the fixed
    summation order"""
    NC.step_graph_equals_eager(_model, lambda: NC.noise_batch(5, 2, 64), steps=4)


def test_fit_two_steps():
    """SegmentationModel.fit for two steps at [2,3,64,64]: the unchanged trainer (fused step) on the new architecture"""
    from salt_amd import architectures as A
    m, values = NC.fit_steps(lambda cfg: _model(cfg=cfg), A.UNetDenseNet, NC.square_batch(3), 2)
    print('densenet fit losses', values)


