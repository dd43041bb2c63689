"""GPU tests of the pyramid-pooling operators (csrc/psp.hip): salt_psp_pool, salt_psp_pool_bwd, salt_psp_merge, salt_psp_merge_bwd,
salt_bn_prelu and salt_bn_prelu_bwd through the C-ABI against the float64 references of psp_op_reference.py, elementwise and with no
element excluded: both dtypes, contiguous views and channel-slice views of a wider buffer between sentinels, inputs verified
unchanged, accumulate 0 and 1, both align_corners values, in-place forms, bit-identical reruns, and the shapes the contract refuses;
then PSPModule and PSPUpsample through the graph against the F20 block fixtures, and PSPNet(34) against the F20 network fixture the
reference produced (eval logits and masks, hipGraph replay, bf16 storage, one training step, the step graph, the trainer).

The bounds are derived in psp_op_reference.py (operands bf16-representable, 2^-23 sum |terms| per fp32 accumulation, 2^-8 per bf16
store; the resize weights and the PReLU pre-activation are pinned and reproduced exactly)."""
import ctypes
import functools

import pytest
import torch

import abi_ops
import psp_op_reference as PR
from abi_ops import Act, Vec, raw, call, _abi, DEV, F64, SENTINEL

pytestmark = pytest.mark.gpu
CODE = {'f32': 0, 'bf16': 1}
SIZES = list(PR.SIZES)
_CASES, _REFS = {}, {}
RATIOS = {}          # {(shape, dtype): {output: worst error / bound}}: the table of DESIGN 20
held = functools.partial(abi_ops.held, ratio=PR.ratio, ratios=RATIOS)
ids = lambda shapes: ['x'.join(str(v) for v in s) for s in shapes]


def psp_case(shape, Cout):
    if (shape, Cout) not in _CASES:
        B, h, w, C = shape
        _CASES[(shape, Cout)] = PR.make_psp_case(B, h, w, C, Cout, seed=500 + 11 * h + C + Cout)
    return _CASES[(shape, Cout)]


def prelu_case(shape):
    if shape not in _CASES:
        _CASES[shape] = PR.make_prelu_case(*shape, seed=700 + shape[1] + shape[3])
    return _CASES[shape]


def ref_of(key, make):
    """one float64 reference per (case, dtype, variant): computed once, shared, left unchanged"""
    if key not in _REFS:
        _REFS[key] = make()
    return _REFS[key]


def nan(*shape):
    return torch.full(shape, float('nan'), dtype=F64)


def same_bits(a, a0):
    return torch.equal(a.buf.view(torch.int16), a0.view(torch.int16))


def dev(t):
    return t.float().contiguous().to(DEV)


def run_pool(shape, dtype, sliced):
    B, h, w, C = shape
    c = psp_case(shape, 64)
    what = 'psp_pool %s %s sliced=%d' % (shape, dtype, sliced)
    x = Act(c['x'], dtype, sliced)
    ps = [Act(nan(B, s, s, C), dtype, sliced) for s in SIZES]
    x0 = x.buf.clone()
    call('salt_psp_pool', dtype=CODE[dtype], x=x.view, nsizes=4, sizes=SIZES, p=[p.view for p in ps])
    x.check(what + ' x')
    assert same_bits(x, x0), what + ': input changed'
    refs = ref_of(('pool', shape, dtype), lambda: PR.pool_ref(c, dtype))
    out = []
    for s, p, r in zip(SIZES, ps, refs):
        p.check(what + ' p%d' % s)
        out.append(p.get())
        held(out[-1], r, what + ' p%d' % s, (shape, dtype), 'pool')
    return out


def run_pool_bwd(shape, dtype, sliced, accumulate):
    B, h, w, C = shape
    c = psp_case(shape, 64)
    what = 'psp_pool_bwd %s %s sliced=%d acc=%d' % (shape, dtype, sliced, accumulate)
    dps = [Act(d, dtype, sliced) for d in c['dp']]
    dx = Act(c['dx_old'] if accumulate else nan(B, h, w, C), dtype, sliced)
    d0 = [d.buf.clone() for d in dps]
    call('salt_psp_pool_bwd', dtype=CODE[dtype], nsizes=4, sizes=SIZES, dp=[d.view for d in dps], dx=dx.view, accumulate=accumulate)
    dx.check(what)
    for d, b in zip(dps, d0):
        d.check(what + ' dp')
        assert same_bits(d, b), what + ': input changed'
    got = dx.get()
    held(got, ref_of(('pool_bwd', shape, dtype, accumulate), lambda: PR.pool_bwd_ref(c, dtype, accumulate)), what, (shape, dtype),
         'pool_bwd acc' if accumulate else 'pool_bwd')
    return got


def run_merge(shape, Cout, dtype, sliced, ac, bias=True):
    B, h, w, _ = shape
    c = psp_case(shape, Cout)
    what = 'psp_merge %s Cout=%d %s sliced=%d ac=%d bias=%d' % (shape, Cout, dtype, sliced, ac, bias)
    f = Act(c['f'], dtype, sliced)
    qs = [Act(q, dtype, sliced) for q in c['q']]
    y = Act(nan(B, h, w, Cout), dtype, sliced)
    bv = dev(c['bias'])
    ins = [f] + qs
    i0 = [a.buf.clone() for a in ins]
    call('salt_psp_merge', dtype=CODE[dtype], f=f.view, bias=bv.data_ptr() if bias else None, nsizes=4, sizes=SIZES, q=[q.view for q in qs],
         align_corners=ac, y=y.view)
    y.check(what)
    for a, b in zip(ins, i0):
        a.check(what + ' input')
        assert same_bits(a, b), what + ': input changed'
    got = y.get()
    held(got, ref_of(('merge', shape, Cout, dtype, ac, bias), lambda: PR.merge_ref(c, dtype, ac, bias)), what, (shape, dtype), 'merge')
    frac = float((got > 0).double().mean())
    assert 0.2 <= frac <= 0.8, (what, frac)
    return got


def run_merge_bwd(shape, Cout, dtype, sliced, ac, accumulate, inplace=False):
    abi = _abi()
    B, h, w, _ = shape
    c = psp_case(shape, Cout)
    what = 'psp_merge_bwd %s Cout=%d %s sliced=%d ac=%d acc=%d inplace=%d' % (shape, Cout, dtype, sliced, ac, accumulate, inplace)
    dy, y = Act(c['dy'], dtype, sliced), Act(c['y'], dtype, sliced)
    df = dy if inplace else Act(nan(B, h, w, Cout), dtype, sliced)
    dqs = [Act(nan(B, s, s, Cout), dtype, sliced) for s in SIZES]
    d0, y0 = dy.buf.clone(), y.buf.clone()
    kw = dict(dtype=CODE[dtype], dy=dy.view, y=y.view, nsizes=4, sizes=SIZES, align_corners=ac, df=df.view, dq=[q.view for q in dqs])
    nparts = abi.lib.salt_psp_merge_bwd_parts(ctypes.byref(abi.fill(abi.STRUCTS['salt_psp_merge_bwd_args'](), **kw)))
    assert nparts == B
    part, dbias = Vec(nparts * Cout), Vec(Cout)
    if accumulate:
        dbias.win.copy_(c['dbias_old'].float())
    call('salt_psp_merge_bwd', partials=part.ptr(), nparts=nparts, dbias=dbias.ptr(), accumulate_dbias=accumulate, **kw)
    y.check(what + ' y')
    assert same_bits(y, y0), what + ': y changed'
    if not inplace:
        dy.check(what + ' dy')
        assert same_bits(dy, d0), what + ': dy changed'
    df.check(what + ' df')
    assert bool(torch.isfinite(part.get((nparts, Cout))).all()), what + ': a partial was not written'
    ref = ref_of(('merge_bwd', shape, Cout, dtype, ac, accumulate), lambda: PR.merge_bwd_ref(c, dtype, ac, accumulate))
    out = dict(df=df.get(), dq=[q.get() for q in dqs], dbias=dbias.get((Cout,)))
    assert torch.equal(out['df'], ref['df']['exact']), what + ': df is not dy [y > 0]'
    for s, q, got, r in zip(SIZES, dqs, out['dq'], ref['dq']):
        q.check(what + ' dq%d' % s)
        held(got, r, what + ' dq%d' % s, (shape, dtype), 'merge_bwd dq')
    held(out['dbias'], ref['dbias'], what + ' dbias', (shape, dtype), 'merge_bwd dbias acc' if accumulate else 'merge_bwd dbias')
    return out


@pytest.mark.parametrize('shape', PR.PSP_SHAPES, ids=ids(PR.PSP_SHAPES))
@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_psp_operators_vs_fp64_reference(dtype, shape):
    for sliced in (0, 1):
        run_pool(shape, dtype, sliced)
        for accumulate in (0, 1):
            run_pool_bwd(shape, dtype, sliced, accumulate)
        for Cout in PR.MERGE_COUT:
            for ac in (0, 1):
                run_merge(shape, Cout, dtype, sliced, ac)
                run_merge_bwd(shape, Cout, dtype, sliced, ac, accumulate=ac)
    run_merge(shape, 64, dtype, 1, 0, bias=False)
    run_merge_bwd(shape, 160, dtype, 1, 0, 0, inplace=True)
    per = RATIOS[(shape, dtype)]
    print('worst error / bound of %s %s: %.3f  per output:' % (shape, dtype, max(per.values())), {k: round(v, 3) for k, v in sorted(per.items())})


def run_bn_prelu(shape, dtype, sliced, alpha, affine, inplace=False):
    c = prelu_case(shape)
    what = 'bn_prelu %s %s sliced=%d alpha=%g affine=%d inplace=%d' % (shape, dtype, sliced, alpha, affine, inplace)
    y = Act(c['y'], dtype, sliced)
    a = y if inplace else Act(nan(*shape), dtype, sliced)
    sc, sh, al = dev(c['scale']), dev(c['shift']), torch.tensor([alpha], device=DEV)
    y0 = y.buf.clone()
    call('salt_bn_prelu', dtype=CODE[dtype], y=y.view, scale=sc.data_ptr() if affine else None, shift=sh.data_ptr() if affine else None,
         alpha=al.data_ptr(), a=a.view)
    a.check(what)
    if not inplace:
        y.check(what + ' y')
        assert same_bits(y, y0), what + ': input changed'
    got = a.get()
    held(got, ref_of(('prelu', shape, dtype, alpha, affine), lambda: PR.bn_prelu_ref(c, dtype, alpha, affine)), what, (shape, dtype), 'bn_prelu')
    return got


def run_bn_prelu_bwd(shape, dtype, sliced, alpha, affine, accumulate, inplace=True):
    abi = _abi()
    c = prelu_case(shape)
    what = 'bn_prelu_bwd %s %s sliced=%d alpha=%g affine=%d acc=%d inplace=%d' % (shape, dtype, sliced, alpha, affine, accumulate, inplace)
    y, da = Act(c['y'], dtype, sliced), Act(c['da'], dtype, sliced)
    du = da if inplace else Act(nan(*shape), dtype, sliced)
    sc, sh, al = dev(c['scale']), dev(c['shift']), torch.tensor([alpha], device=DEV)
    y0, d0 = y.buf.clone(), da.buf.clone()
    kw = dict(dtype=CODE[dtype], da=da.view, y=y.view, scale=sc.data_ptr() if affine else None, shift=sh.data_ptr() if affine else None,
              alpha=al.data_ptr(), du=du.view)
    nparts = abi.lib.salt_bn_prelu_bwd_parts(ctypes.byref(abi.fill(abi.STRUCTS['salt_bn_prelu_bwd_args'](), **kw)))
    assert 1 <= nparts <= 1024
    part, dal = Vec(nparts), Vec(1)
    if accumulate:
        dal.win.copy_(c['dalpha_old'].float())
    call('salt_bn_prelu_bwd', partials=part.ptr(), nparts=nparts, dalpha=dal.ptr(), accumulate_dalpha=accumulate, **kw)
    y.check(what + ' y')
    du.check(what + ' du')
    assert same_bits(y, y0), what + ': y changed'
    if not inplace:
        da.check(what + ' da')
        assert same_bits(da, d0), what + ': da changed'
    assert bool(torch.isfinite(part.get((nparts,))).all()), what + ': a partial was not written'
    ref = ref_of(('prelu_bwd', shape, dtype, alpha, affine, accumulate), lambda: PR.bn_prelu_bwd_ref(c, dtype, alpha, accumulate, affine))
    out = dict(du=du.get(), dalpha=dal.get((1,)))
    held(out['du'], ref['du'], what + ' du', (shape, dtype), 'bn_prelu_bwd du')
    held(out['dalpha'], ref['dalpha'], what + ' dalpha', (shape, dtype), 'bn_prelu_bwd dalpha acc' if accumulate else 'bn_prelu_bwd dalpha')
    return out


@pytest.mark.parametrize('shape', PR.PRELU_SHAPES, ids=ids(PR.PRELU_SHAPES))
@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_bn_prelu_vs_fp64_reference(dtype, shape):
    assert 0.2 <= PR.negative_fraction(prelu_case(shape)) <= 0.8 and 0.2 <= PR.negative_fraction(prelu_case(shape), affine=False) <= 0.8
    for i, alpha in enumerate(PR.ALPHAS):
        sliced, affine = i % 2, i != 2                                  # alpha = 1 without scale / shift: the eval form
        run_bn_prelu(shape, dtype, sliced, alpha, affine)
        run_bn_prelu(shape, dtype, 1 - sliced, alpha, affine, inplace=True)
        run_bn_prelu_bwd(shape, dtype, sliced, alpha, affine, accumulate=i % 2)
        run_bn_prelu_bwd(shape, dtype, 1 - sliced, alpha, affine, accumulate=1 - i % 2, inplace=False)
    per = RATIOS[(shape, dtype)]
    print('worst error / bound of %s %s: %.3f  per output:' % (shape, dtype, max(per.values())), {k: round(v, 3) for k, v in sorted(per.items())})


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_reruns_are_bit_identical(dtype):
    """no atomics anywhere: two runs of every operator give the same bits"""
    shape = (3, 5, 7, 40)
    for a, b in ((run_pool(shape, dtype, 1), run_pool(shape, dtype, 1)),
                 (run_merge_bwd(shape, 160, dtype, 1, 0, 0)['dq'], run_merge_bwd(shape, 160, dtype, 1, 0, 0)['dq'])):
        assert all(torch.equal(p, q) for p, q in zip(a, b))
    assert torch.equal(run_pool_bwd(shape, dtype, 1, 1), run_pool_bwd(shape, dtype, 1, 1))
    assert torch.equal(run_merge(shape, 160, dtype, 0, 1), run_merge(shape, 160, dtype, 0, 1))
    assert torch.equal(run_merge_bwd(shape, 160, dtype, 0, 1, 1)['dbias'], run_merge_bwd(shape, 160, dtype, 0, 1, 1)['dbias'])
    big = (4, 32, 32, 64)
    p, q = run_bn_prelu_bwd(big, dtype, 0, 0.25, True, 0), run_bn_prelu_bwd(big, dtype, 0, 0.25, True, 0)
    assert torch.equal(p['du'], q['du']) and torch.equal(p['dalpha'], q['dalpha'])


def test_unsupported_shapes_fail_loudly_and_launch_nothing():
    abi = _abi()
    from salt_amd.engine import shaped_view
    UNS, BAD = abi.CONSTS['SALT_E_UNSUPPORTED'], abi.CONSTS['SALT_E_BADARG']

    def pool(B=1, h=8, w=8, C=64, sizes=(1, 2, 3, 6), dtype=0, off=0, cs=None):
        x = torch.randn(B * h * w * (cs or C) + 64, device=DEV)
        ps = [torch.full((B, s, s, C), SENTINEL, device=DEV) for s in sizes]
        rc = raw('salt_psp_pool', dtype=dtype, x=shaped_view(x.data_ptr() + off, B, h, w, C, cs), nsizes=len(sizes), sizes=list(sizes),
                 p=[shaped_view(p.data_ptr(), B, s, s, C) for p, s in zip(ps, sizes)])
        return rc, all(bool((p == SENTINEL).all()) for p in ps)
    assert pool() == (0, False)
    assert pool(sizes=(2, 4)) == (0, False)
    for kw in (dict(h=33), dict(w=40), dict(C=36), dict(C=4), dict(sizes=(1, 2, 3, 7)), dict(sizes=(0,)), dict(sizes=())):
        assert pool(**kw) == (UNS, True) and abi.lib.salt_last_error(), kw
    for kw in (dict(dtype=5), dict(off=4), dict(cs=66)):
        assert pool(**kw) == (BAD, True) and abi.lib.salt_last_error(), kw

    def merge(name, h=8, C=64, sizes=(1, 2, 3, 6), qC=None, **over):
        B = 2
        t = lambda *s: torch.full(s, SENTINEL, device=DEV)
        full, out = t(B, h, h, C), t(B, h, h, C)
        qs = [t(B, s, s, qC or C) for s in sizes]
        v = lambda a: shaped_view(a.data_ptr(), *a.shape)
        part, db = t(B * C), t(C)
        if name == 'salt_psp_merge':
            kw = dict(dtype=0, f=v(full), nsizes=len(sizes), sizes=list(sizes), q=[v(q) for q in qs], y=v(out))
        else:
            kw = dict(dtype=0, dy=v(full), y=v(full), nsizes=len(sizes), sizes=list(sizes), df=v(out), dq=[v(q) for q in qs], partials=part.data_ptr(),
                      nparts=B, dbias=db.data_ptr())
        kw.update(over)
        rc = raw(name, **kw)
        return rc, bool((out == SENTINEL).all()) and bool((db == SENTINEL).all())
    for name in ('salt_psp_merge', 'salt_psp_merge_bwd'):
        assert merge(name) == (0, False)
        assert merge(name, h=64) == (UNS, True)
        assert merge(name, C=20) == (UNS, True)
        assert merge(name, sizes=(1, 8)) == (UNS, True)
        assert merge(name, qC=32) == (BAD, True)
    assert merge('salt_psp_merge_bwd', nparts=1) == (BAD, True)
    assert merge('salt_psp_merge_bwd', partials=None) == (BAD, True)

    def prelu(C=16, alpha=True, shift=True, off=0):
        y = torch.randn(2 * 3 * 3 * C + 64, device=DEV)
        a = torch.full((2, 3, 3, C), SENTINEL, device=DEV)
        sc, al = torch.ones(C, device=DEV), torch.ones(1, device=DEV)
        rc = raw('salt_bn_prelu', dtype=0, y=shaped_view(y.data_ptr() + off, 2, 3, 3, C), scale=sc.data_ptr(), shift=sc.data_ptr() if shift else None,
                 alpha=al.data_ptr() if alpha else None, a=shaped_view(a.data_ptr(), 2, 3, 3, C))
        return rc, bool((a == SENTINEL).all())
    assert prelu() == (0, False)
    assert prelu(C=12) == (UNS, True)
    assert prelu(alpha=False) == (BAD, True) and prelu(shift=False) == (BAD, True) and prelu(off=8) == (BAD, True)
    S = abi.STRUCTS['salt_bn_prelu_bwd_args']
    v = shaped_view(1 << 20, 2, 3, 3, 16)
    assert raw('salt_bn_prelu_bwd', dtype=0, da=v, y=v, du=v, alpha=1 << 20, partials=None, nparts=1, dalpha=1 << 20) == BAD
    assert raw('salt_bn_prelu_bwd', dtype=0, da=v, y=v, du=v, alpha=1 << 20, partials=1 << 20, nparts=7, dalpha=1 << 20) == BAD
    assert abi.lib.salt_bn_prelu_bwd_parts(ctypes.byref(abi.fill(S(), dtype=0, y=v))) == 1


# ------------------------------------------------------------------------------------------------ the two blocks through the graph (F20)
TOL32, TOLBF = 5e-5, 4e-2                   # tests/test_gpu_blocks.py: the F2 / F4 block bounds


def _block_state(m):
    import closed_form as CF
    return {k: CF.tensor_for(k, v.shape).to(v.dtype) for k, v in m.state_dict().items()}


def _emulated(fn, sd, x, gy):
    """the test-side oracle block with bf16 storage emulated: the yardstick of the bf16 backward bound (tests/test_gpu_blocks.py)"""
    from oracle import blocks as OB
    s2 = {k: v.clone() for k, v in sd.items()}
    leaves = [k for k, v in s2.items() if v.dtype.is_floating_point and not k.endswith(('running_mean', 'running_var'))]
    for k in leaves:
        s2[k].requires_grad_(True)
    xr = x.clone().requires_grad_(True)
    with OB.bf16_storage():
        fn(s2, OB._st(xr)).backward(gy)
    out = {'gx': xr.grad}
    for k in leaves:
        out['g:' + k] = s2[k].grad if s2[k].grad is not None else torch.zeros_like(s2[k])
    return out


def _block_vs_golden(fxname, make, emit, oracle, mode, dtype, alpha=False):
    """forward, input gradient, parameter gradients and running statistics with the bounds of
    tests/test_gpu_blocks.py::test_block_vs_reference_golden (5e-5 f32, 2x / 3x for input / parameter gradients; bf16 4e-2 forward and
    the 1.5 e_emu + 2e-2 rule against the bf16-storage emulation backward) -> the BlockRun"""
    import numpy as np
    import closed_form as CF
    from gpu_harness import BlockRun
    from helpers import golden, assert_close, rel_err
    fx = golden('%s_%s' % (fxname, mode))
    assert 0.2 <= float(fx['fraction']) <= 0.8 and float(fx['ref_f32_vs_f64']) <= TOL32 / 4
    m = make()
    sd = _block_state(m)
    if alpha:
        sd['conv.2.weight'] = torch.full((1,), float(fx['alpha']))
    m.load_state_dict(sd)
    x = CF.input_for(str(fx['input_tag']), tuple(int(v) for v in fx['x_shape']))
    gy = CF.input_for('gy:%s' % (tuple(fx['y'].shape),), fx['y'].shape)
    train = mode == 'train'
    m.train(train)
    run = BlockRun(m, [x], lambda g, a: emit(m, g, a), train=train, dtype=dtype)
    tol = TOL32 if dtype == 'f32' else TOLBF
    assert_close(run.forward(), fx['y'], tol, 'y')
    if not train:
        return run
    gx, grads = run.backward(gy.to(DEV))
    emu = None if dtype == 'f32' else _emulated(lambda s, a: oracle(s, a, True), sd, x, gy)

    def check(got, ref, key, f32_tol):
        if emu is None:
            e = assert_close(got, ref, f32_tol, key)
            print('  %s %s %s: %.2e of %.1e' % (fxname, dtype, key, e, f32_tol))
        else:
            e_hip, e_emu = rel_err(got, ref), rel_err(emu[key], ref)
            print('  %s %s %s: HIP %.2e, emulation %.2e' % (fxname, dtype, key, e_hip, e_emu))
            assert e_hip <= 1.5 * e_emu + 2e-2, '%s: HIP bf16 %.3e from the golden, bf16-storage emulation %.3e' % (key, e_hip, e_emu)
    check(gx[0], fx['gx'], 'gx', tol * 2)
    assert set(grads) == {k for k, _ in m.named_parameters()} == {k[2:] for k in fx if k.startswith('g:')}
    gscale = max(float(np.abs(fx['g:' + k]).max()) for k in grads)
    for k, g in grads.items():
        if float(g.abs().max()) == 0.0:      # the convolution's bias in front of a train-mode BatchNorm: analytically zero, rounding noise in the fixture
            assert k == 'conv.0.bias' and np.abs(fx['g:' + k]).max() < 1e-4 * gscale, k
        else:
            check(g, fx['g:' + k], 'g:' + k, tol * 3)
    sd2 = m.state_dict()
    for k in sd2:
        if k.endswith(('running_mean', 'running_var')):
            assert_close(sd2[k].cpu(), fx['s:' + k], tol, k)
    return run


@pytest.mark.parametrize('mode', ['train', 'eval'])
@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_psp_module_vs_golden(mode, dtype):
    """F20_psp_module: PSPModule(64, 128) on [2,64,8,8] - the factored path against the reference's concatenated one, the gradient of
    every block of bottleneck.weight, the bias gradient out of the merge's adjoint, the input gradient from two sources"""
    import psp_oracle as PO
    from salt_amd import architectures as A
    run = _block_vs_golden('F20_psp_module', lambda: A.PSPModule(64, 128), lambda m, g, a: m.emit(g, a),
                           lambda s, a, tr: PO.psp_module(s, '', a), mode, dtype)
    ops = [o[0] for o in run.g.fwd.ops]
    assert ops.count('psp_pool') == 1 and ops.count('psp_merge') == 1 and ops.count('conv') == 9         # 4 stages, 4 + 1 slices
    assert max(t.shape[-1] for t in run.g.keep if isinstance(t, torch.Tensor) and t.dim() == 4) == 128                                   # nothing 5 C = 320 channels wide
    if mode == 'train':
        bops = [o[0] for o in run.g.bwd.ops]
        assert bops.count('psp_merge_bwd') == 1 and bops.count('psp_pool_bwd') == 1 and bops.count('conv_wgrad') == 9
        pb = [s for (o, _, s) in run.g.bwd.ops if o == 'psp_pool_bwd'][0]
        assert pb.accumulate == 1                                          # adds to what the feats block's data gradient wrote first


@pytest.mark.parametrize('mode', ['train', 'eval'])
@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_psp_upsample_vs_golden(mode, dtype):
    """F20_psp_upsample: PSPUpsample(32, 16) on [2,32,5,7] with a slope that is not 0, 1 or 0.25: the slope's gradient, the BatchNorm
    backward behind the in-place PReLU backward, the running statistics"""
    import psp_oracle as PO
    from salt_amd import architectures as A
    run = _block_vs_golden('F20_psp_upsample', lambda: A.PSPUpsample(32, 16), lambda m, g, a: m.emit(g, a),
                           lambda s, a, tr: PO.psp_upsample(s, '', a, tr), mode, dtype, alpha=True)
    ops = [o[0] for o in run.g.fwd.ops]
    assert ops.count('bn_prelu') == 1 and 'affine_act' not in ops
    pr = [s for (o, _, s) in run.g.fwd.ops if o == 'bn_prelu'][0]
    assert bool(pr.scale) == (mode == 'train') and (mode == 'train' or pr.y.p == pr.a.p)      # eval: folded BatchNorm in the convolution, PReLU in place
    if mode == 'train':
        bops = [o[0] for o in run.g.bwd.ops]
        assert bops.index('bn_prelu_bwd') < bops.index('bn_bwd') and bops.count('bn_prelu_bwd') == 1


# ------------------------------------------------------------------------------------------------ whole network (F20, closed-form weights)
NET_FX = 'F20_pspnet34_hyper'


def _net(fx, dtype='f32'):
    import net_checks as NC
    from helpers import T
    from salt_amd import architectures as A
    net = NC.fill_closed_form(A.PSPNet(34, 2, dropout_2d=0.0, pretrained=False, use_hypercolumn=True))
    net.final[1].bias.data.copy_(T(fx['final_1_bias']))           # the class-1 bias the generator moved so that both classes occur
    return net.set_compute_dtype(dtype).to(DEV)


def _no_wide_activation(cn):
    """the 2560-channel concatenation of the reference's PSPModule is never allocated: the widest activation is the bottleneck's 1024"""
    assert max(t.shape[-1] for t in cn.g.keep if isinstance(t, torch.Tensor) and t.dim() == 4) == 1024


def test_eval_logits_and_masks_match_reference():
    import net_checks as NC
    from helpers import golden, T
    fx = golden(NET_FX)
    x = T(fx['x']).to(DEV)
    net = _net(fx).eval()
    with torch.no_grad():
        logits = net(x).cpu()
    ref = NC.check_eval_masks(logits, fx, 'pspnet eval', logits_tol=1e-3)
    assert 0.2 <= ref.mean() <= 0.8
    cn = net.engine().net(tuple(x.shape), False)
    ops = [o[0] for o in cn.fwd.ops]
    assert ops.count('psp_pool') == 1 and ops.count('psp_merge') == 1 and ops.count('bn_prelu') == 4 and 'bn_finalize' not in ops
    pool = [s for (o, _, s) in cn.fwd.ops if o == 'psp_pool'][0]
    assert (pool.x.H, pool.x.W, pool.x.C) == (4, 4, 512) and list(pool.sizes) == [1, 2, 3, 6]          # s = 6 on 4 x 4: repeated bins
    _no_wide_activation(cn)
    NC.check_eval_graph_replay(cn, x, logits)
    NC.check_bf16_eval_guard(_net(fx, 'bf16').eval(), x, logits, fx, 'pspnet eval bf16', guard_factor=4)


def test_one_training_step_matches_reference():
    """zero_grad -> forward -> lovasz -> backward -> Adam(lr 1e-4, L2 1e-4) as models.py:105-136, by the procedures of
    tests/net_checks.py with the bounds tests/test_gpu_densenet.py uses for F19: gradient norms (and sums) of tensors with 16 elements
    and more within 1e-2 relative, tensors under 16 elements within 1e-6 of the largest gradient norm, full gradients at 2e-2."""
    import net_checks as NC
    from helpers import golden, T
    fx = golden(NET_FX)
    assert float(fx['ref_f32_vs_f64_gradnorm_rel']) <= 2.5e-3 and float(fx['ref_f32_vs_f64_small_abs']) <= 2.5e-7
    net = _net(fx)
    net.train()
    opt, out, eng, own, idx = NC.train_step_prologue(net, [T(fx['x']).to(DEV)], fx, logits_tol=2e-3, loss_tol=2e-3)
    cn = eng.net(tuple(fx['x'].shape), True)
    ops = [o[0] for o in cn.fwd.ops]
    bops = [o[0] for o in cn.bwd.ops]
    assert ops.count('psp_pool') == 1 and ops.count('psp_merge') == 1 and ops.count('bn_prelu') == 4
    assert bops.count('psp_merge_bwd') == 1 and bops.count('psp_pool_bwd') == 1 and bops.count('bn_prelu_bwd') == 4
    assert ops.count('bilinear') == 6                                  # up x2(up2) once: the hypercolumn's slice is up1's input
    _no_wide_activation(cn)
    # under 16 elements: the four PReLU slopes and the two-element head bias
    NC.check_grad_tally(net, eng, own, idx, fx, 'pspnet train:', include_small_below_norm_floor=True, min_checked=120, n_small=5,
                        norm_tol=1e-2, sum_tol=1e-2, small_tol=1e-6, verbose=True)
    full = fx['fullgrad_keys'].tolist()
    assert len(full) == 17 and float(fx['fullgrad_ref_f32_vs_f64'].max()) <= 5e-3
    assert 'psp.bottleneck.bias' in full and sum(k.endswith('conv.2.weight') for k in full) == 4
    NC.check_full_grads(eng, own, fx, full, tol=2e-2, verbose=True)
    sd = NC.check_after_adam(opt, net, own, idx, fx, norm_tol=1e-4, sum_tol=1e-4, bn_tol=1e-3, skip_bn=None)
    assert int(sd['up1.conv.1.num_batches_tracked']) == 1


def _model(dtype='bf16', lr=1e-3, cfg=None):
    import net_checks as NC
    return NC.family_model('PSPNet', dtype, lr, 1, cfg)


def test_step_graph_replay_equals_eager_steps(deterministic_sums):
    """the procedure of tests/net_checks.py::step_graph_equals_eager at [2,3,64,64]: the training step captured into ONE hipGraph and
    replayed reproduces the eagerly launched steps bit for bit under the fixed summation order"""
    import net_checks as NC
    NC.step_graph_equals_eager(_model, lambda: NC.noise_batch(5, 2, 64), steps=4)


def test_fit_two_steps():
    """SegmentationModel.fit for two steps at [2,3,64,64]: the unchanged trainer (fused step) on the new architecture"""
    import net_checks as NC
    from salt_amd import architectures as A
    m, values = NC.fit_steps(lambda cfg: _model(cfg=cfg), A.PSPNet, NC.square_batch(3), 2)
    print('pspnet fit losses', values)
