"""GPU tests of UNetSeResNet (SE-ResNet encoders on csrc/se_res.hip): the fused SE-residual tail through the C-ABI against the plain
fp64 reference of se_res_op_reference.py (both dtypes, both summation protocols, eval and training scale / shift, strided channel-slice
views with guard patterns, both accumulate settings), bit-identical backward runs under the fixed summation order, the F17 bottleneck
and network fixtures, and the trainer surface.

Operator bound (none of it measured on the kernels): a float32 torch evaluation of the SAME case sits e32 from the float64 reference;
the kernel may sit at most 4 e32 + 1e-6 max|ref| from it.  The bf16 activations (y, dx, dres) are compared the way
tests/test_gpu_blocks.py earns its bf16 bound: a float32 evaluation with the outputs rounded to bf16 storage sits e_emu (max error
relative to max|ref|) from the reference, the kernel may sit at most 1.5 e_emu + 2e-2.  Inputs are drawn (seed by seed, on the CPU) so
that the float32 evaluation takes every ReLU decision like float64 and no pre-activation lies within the bound of zero; elements
that do are excluded, capped at 0.5 %."""
import ctypes

import pytest
import torch

from helpers import golden, T, assert_close, rel_err
import closed_form as CF
import se_res_op_reference as SR
import seresnet_oracle as SO
import net_checks as NC
from abi_ops import Act, Vec, raw, call, _abi, DEV, F64, SENTINEL

pytestmark = pytest.mark.gpu
TOL32, TOLBF = 5e-5, 4e-2                   # tests/test_gpu_blocks.py: the F2 / F4 block bounds

# (B, H, W, C): fewer pixels than pixel rows of a workgroup; an odd, non-square map; a 1x1 map and a 2x2 map at C = 2048 (four channel
# chunks per pixel part, the FC streaming its 1 MB matrices); several row groups per workgroup; 256 pixels (one part) at C = 1024
SHAPES = [(2, 4, 4, 256), (3, 3, 5, 256), (1, 1, 1, 2048), (2, 2, 2, 2048), (2, 8, 8, 512), (2, 16, 16, 1024)]
_CASES = {}


def reference_case(shape, dtype, affine):
    """One set of inputs per (shape, dtype, affine) with its float64 reference, its float32 evaluation and (bf16) the storage
    emulation - computed once, shared by every placement / protocol / accumulate setting and left unchanged."""
    key = (shape, dtype, affine)
    if key in _CASES:
        return _CASES[key]
    B, H, W, C = shape
    rt = (lambda t: t.bfloat16().float()) if dtype == 'bf16' else (lambda t: t)
    for seed in range(100):
        c = SR.make_case(B, H, W, C, 1000 * seed + C + H, affine, dtype)
        p64 = [c[k] for k in ('w1', 'b1', 'w2', 'b2')]
        f64 = SR.se_res(c['x'], c['scale'], c['shift'], c['res'], *p64)
        b64 = {acc: SR.se_res_bwd(f64, c['dy'], c['w1'], c['w2'], c['dres_old'] if acc else None) for acc in (0, 1)}
        c32 = {k: (v.float() if v is not None else None) for k, v in c.items()}
        p32 = [c32[k] for k in ('w1', 'b1', 'w2', 'b2')]
        f32 = SR.se_res(c32['x'], c32['scale'], c32['shift'], c32['res'], *p32)
        band = 4 * float((f32['pre'].double() - f64['pre']).abs().max()) + 1e-6 * float(f64['pre'].abs().max())
        if dtype == 'bf16':
            f32['y'] = rt(f32['y'])
        b32 = {acc: SR.se_res_bwd(f32, c32['dy'], c32['w1'], c32['w2'], c32['dres_old'] if acc else None) for acc in (0, 1)}
        if dtype == 'bf16':
            for acc in (0, 1):
                b32[acc]['dx'], b32[acc]['dres'] = rt(b32[acc]['dx']), rt(b32[acc]['dres'])
        near = f64['pre'].abs() <= band
        flips = (f32['pre'] > 0) != (f64['pre'] > 0)
        gates = f64['gate']
        spread = float(((gates > 0.1) & (gates < 0.9)).double().mean())
        if int(near.sum()) == 0 and int(flips.sum()) == 0 and spread >= 0.5:
            break
    assert int(near.sum()) <= 0.005 * near.numel() and spread >= 0.5, (shape, dtype, affine, int(near.sum()), spread)
    _CASES[key] = dict(c=c, f64=f64, b64=b64, f32=f32, b32=b32, keep=~near, seed=seed)
    return _CASES[key]


RATIOS = {}          # {(shape, dtype): {output: worst error / bound}}, the table of DESIGN 16


def within(got, ref64, ev32, what, dtype, keep=None, activation=False, case=None):
    """the module docstring's bound; records the worst error ratio per output under RATIOS[case], case = (shape, dtype)"""
    if keep is not None:
        got, ref64, ev32 = got[keep], ref64[keep], ev32[keep]
    assert bool(torch.isfinite(got).all()), '%s: non-finite output' % what
    mx = float(ref64.abs().max()) if ref64.numel() else 0.0
    err, e32 = float((got - ref64).abs().max()), float((ev32.double() - ref64).abs().max())
    if activation and dtype == 'bf16':
        bound = (1.5 * e32 / max(mx, 1e-30) + 2e-2) * mx
    else:
        bound = 4 * e32 + 1e-6 * mx
    ratio = err / bound if bound > 0 else (0.0 if err == 0 else float('inf'))
    if case is not None:
        per = RATIOS.setdefault(case, {})
        per[what.split(' | ')[-1]] = max(per.get(what.split(' | ')[-1], 0.0), ratio)
    print('%s [%s]: err %.3e  yardstick %.3e  bound %.3e  ratio %.3f' % (what, dtype, err, e32, bound, ratio))
    assert err <= bound, '%s [%s]: err %.3e > bound %.3e (yardstick %.3e, max|ref| %.3e)' % (what, dtype, err, bound, e32, mx)


def run_case(shape, dtype, affine, shards, sliced, accumulate, inplace=False):
    abi = _abi()
    B, H, W, C = shape
    R = C // 16
    rc = reference_case(shape, dtype, affine)
    c, f64, b64, f32, b32, keep = rc['c'], rc['f64'], rc['b64'][accumulate], rc['f32'], rc['b32'][accumulate], rc['keep']
    what = 'se_res %s %s affine=%d shards=%d sliced=%d acc=%d inplace=%d' % (shape, dtype, affine, shards, sliced, accumulate, inplace)
    dev = lambda t: t.float().contiguous().to(DEV)
    w1, b1, w2, b2 = dev(c['w1']), dev(c['b1']), dev(c['w2']), dev(c['b2'])
    sc, sh = (dev(c['scale']), dev(c['shift'])) if affine else (None, None)
    x, res = Act(c['x'], dtype, sliced), Act(c['res'], dtype, sliced)
    y = Act(torch.full(shape, float('nan'), dtype=F64), dtype, sliced)
    code = 1 if dtype == 'bf16' else 0
    nparts = abi.lib.salt_se_res_parts(ctypes.byref(abi.fill(abi.STRUCTS['salt_se_res_args'](), dtype=code, x=x.view)))
    assert nparts >= 1
    gap, hid, gate = Vec(B * C), Vec(B * R), Vec(B * C)
    acc = Vec(B * C, fill=0.0, dtype=F64) if shards else None
    part = None if shards else Vec(B * nparts * C)
    x0, r0 = x.buf.clone(), res.buf.clone()
    call('salt_se_res', dtype=code, x=x.view, in_scale=sc.data_ptr() if affine else None, in_shift=sh.data_ptr() if affine else None, res=res.view,
         w1=w1.data_ptr(), b1=b1.data_ptr(), w2=w2.data_ptr(), b2=b2.data_ptr(), R=R, gap_partials=part.ptr() if part else None, nparts=nparts,
         gap_acc=acc.ptr() if acc else None, gap=gap.ptr(), hidden=hid.ptr(), gate=gate.ptr(), y=y.view)
    y.check(what + ' y')
    assert torch.equal(x.buf.view(torch.int16), x0.view(torch.int16)) and torch.equal(res.buf.view(torch.int16), r0.view(torch.int16)), what + ': inputs changed'
    within(gap.get((B, C)), f64['gap'], f32['gap'], what + ' | gap', dtype, case=(shape, dtype))
    within(hid.get((B, R)), f64['hidden'], f32['hidden'], what + ' | hidden', dtype, case=(shape, dtype))
    within(gate.get((B, C)), f64['gate'], f32['gate'], what + ' | gate', dtype, case=(shape, dtype))
    got_y = y.get()
    within(got_y, f64['y'], f32['y'], what + ' | y', dtype, keep, activation=True, case=(shape, dtype))
    assert bool(((got_y > 0) == (f64['y'] > 0))[keep].all()), what + ': ReLU decisions'
    # backward
    dy = Act(c['dy'], dtype, sliced)
    old = c['dres_old'] if accumulate else torch.full(shape, float('nan'), dtype=F64)
    dres = Act(old, dtype, sliced)
    dx = dy if inplace else Act(torch.full(shape, float('nan'), dtype=F64), dtype, sliced)
    du, dh, dgap = Vec(B * C), Vec(B * R), Vec(B * C)
    gw1, gb1, gw2, gb2 = Vec(R * C), Vec(R), Vec(C * R), Vec(C)
    acc2 = Vec(B * C, fill=0.0, dtype=F64) if shards else None
    part2 = None if shards else Vec(B * nparts * C)
    kw = dict(dtype=code, x=x.view, in_scale=sc.data_ptr() if affine else None, in_shift=sh.data_ptr() if affine else None, y=y.view, dy=dy.view,
              w1=w1.data_ptr(), w2=w2.data_ptr(), R=R, gap=gap.ptr(), hidden=hid.ptr(), gate=gate.ptr(), partials=part2.ptr() if part2 else None,
              nparts=nparts, acc=acc2.ptr() if acc2 else None, du=du.ptr(), dh=dh.ptr(), dgap=dgap.ptr(), dx=dx.view, dres=dres.view,
              accumulate_dres=accumulate, g_w1=gw1.ptr(), g_b1=gb1.ptr(), g_w2=gw2.ptr(), g_b2=gb2.ptr())
    # the split form first (the engine's): the deferred launch alone must leave the parameter gradients
    call('salt_se_res_bwd', defer_param_grads=1, **kw)
    assert bool(torch.isnan(gw1.get((R, C))).all()) and bool(torch.isnan(gb2.get((C,))).all()), what + ': defer_param_grads wrote parameter gradients'
    call('salt_se_res_fc_grads', **kw)
    for a, name in ((dx, 'dx'), (dres, 'dres'), (y, 'y after backward')):
        a.check(what + ' ' + name)
    within(dx.get(), b64['dx'], b32['dx'], what + ' | dx', dtype, keep, activation=True, case=(shape, dtype))
    within(dres.get(), b64['dres'], b32['dres'], what + ' | dres', dtype, keep, activation=True, case=(shape, dtype))
    for v, k, shp in ((du, 'du', (B, C)), (dh, 'dh', (B, R)), (dgap, 'dgap', (B, C))):
        within(v.get(shp), b64[k], b32[k], what + ' | ' + k, dtype, case=(shape, dtype))
    for v, k, shp in ((gw1, 'g_w1', (R, C)), (gb1, 'g_b1', (R,)), (gw2, 'g_w2', (C, R)), (gb2, 'g_b2', (C,))):
        within(v.get(shp), b64[k], b32[k], what + ' | ' + k, dtype, case=(shape, dtype))
    return dict(dx=dx.get(), dres=dres.get(), gw1=gw1.get((R, C)), gb1=gb1.get((R,)), gw2=gw2.get((C, R)), gb2=gb2.get((C,)), du=du.get((B, C)),
                dh=dh.get((B, R)), dgap=dgap.get((B, C)), y=got_y, gate=gate.get((B, C)), kw=kw)


@pytest.mark.parametrize('shape', SHAPES, ids=['x'.join(str(v) for v in s) for s in SHAPES])
@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_se_res_vs_fp64_reference(dtype, shape):
    n = 0
    for affine in (0, 1):
        for shards in (1, 0):
            for sliced, accumulate in ((0, 0), (1, 1), (1, 0), (0, 1)):
                run_case(shape, dtype, affine, shards, sliced, accumulate)
                n += 1
        run_case(shape, dtype, affine, 1, 0, 0, inplace=True)          # dL/dz written over dL/dy
        n += 1
    assert n == 18
    per = RATIOS[(shape, dtype)]
    print('worst error / bound of %s %s: %.3f  per output:' % (shape, dtype, max(per.values())), {k: round(v, 3) for k, v in sorted(per.items())})


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_deterministic_backward_is_bit_identical(dtype):
    """per-part partials added in a fixed order: two runs of salt_se_res_bwd + salt_se_res_fc_grads give the same bits"""
    for shape in ((2, 16, 16, 1024), (3, 3, 5, 256)):
        a = run_case(shape, dtype, 1, 0, 1, 0)
        b = run_case(shape, dtype, 1, 0, 1, 0)
        for k in a:
            if k != 'kw':
                assert torch.equal(a[k], b[k]), (shape, k)


def test_unsupported_shapes_fail_loudly_and_launch_nothing():
    abi = _abi()
    from salt_amd.engine import shaped_view
    UNS, BAD = abi.CONSTS['SALT_E_UNSUPPORTED'], abi.CONSTS['SALT_E_BADARG']

    def attempt(C, R, dtype=0, off=0, **over):
        B, H, W = 2, 3, 3
        x = torch.randn(B * H * W * C + 64, device=DEV)
        res = torch.randn(B, H, W, C, device=DEV)
        y = torch.full((B, H, W, C), SENTINEL, device=DEV)
        w1, b1, w2, b2 = torch.randn(max(R, 1), C, device=DEV), torch.randn(max(R, 1), device=DEV), torch.randn(C, max(R, 1), device=DEV), torch.randn(C, device=DEV)
        gap, hid, gate, part = (torch.full((n,), SENTINEL, device=DEV) for n in (B * C, B * max(R, 1), B * C, B * 16 * C))
        kw = dict(dtype=dtype, x=shaped_view(x.data_ptr() + off, B, H, W, C), res=shaped_view(res.data_ptr(), B, H, W, C), w1=w1.data_ptr(), b1=b1.data_ptr(),
                  w2=w2.data_ptr(), b2=b2.data_ptr(), R=R, gap_partials=part.data_ptr(), nparts=1, gap=gap.data_ptr(), hidden=hid.data_ptr(),
                  gate=gate.data_ptr(), y=shaped_view(y.data_ptr(), B, H, W, C))
        kw.update(over)
        rc = raw('salt_se_res', **kw)
        untouched = all(bool((t == SENTINEL).all()) for t in (y, gap, hid, gate))
        return rc, untouched
    assert attempt(256, 16) == (0, False)
    for what, args, want in (('C = 96', (96, 6), UNS), ('C = 4096', (4096, 256), UNS), ('R = C / 8', (256, 32), UNS), ('C = 32', (32, 2), UNS)):
        rc, untouched = attempt(*args)
        assert rc == want and untouched and abi.lib.salt_last_error(), (what, rc)
    assert attempt(256, 16, off=4) == (UNS, True)                      # x 4 bytes off the 16-byte grid
    assert attempt(256, 16, nparts=3) == (BAD, True)
    assert attempt(256, 16, w1=None) == (BAD, True)
    assert attempt(256, 16, dtype=7) == (BAD, True)
    probe = abi.fill(abi.STRUCTS['salt_se_res_args'](), dtype=0, x=shaped_view(1 << 20, 2, 3, 3, 96))
    assert abi.lib.salt_se_res_parts(ctypes.byref(probe)) == UNS


# ------------------------------------------------------------------------------------------------ the bottleneck through the graph
BLOCKS = {'F17_se_bottleneck': (64, 64, 1, 256, 'f17a'), 'F17_se_bottleneck_s2': (256, 128, 2, 512, 'f17b')}


def _block(name, fx):
    from torch import nn
    from salt_amd import architectures as A
    cin, planes, stride, cout, _ = BLOCKS[name]
    down = nn.Sequential(nn.Conv2d(cin, cout, kernel_size=1, stride=stride, padding=0, bias=False), nn.BatchNorm2d(cout))
    m = A.SEResNetBottleneck(cin, planes, 1, 16, stride, down)
    sd = {k: CF.tensor_for(k, v.shape).to(v.dtype) for k, v in m.state_dict().items()}
    sd['se_module.fc2.weight'] = sd['se_module.fc2.weight'] * float(fx['fc2_scale'])
    m.load_state_dict(sd)
    return m, sd


def _block_io(name, fx):
    shape = tuple(int(v) for v in fx['x_shape'])
    x = T(fx['x']) if 'x' in fx else CF.input_for(BLOCKS[name][4], shape)
    gy = T(fx['gy']) if 'gy' in fx else CF.input_for('gy:%s' % (tuple(fx['y'].shape),), fx['y'].shape)
    return x, gy


def _emulated_block(name, fx, sd, x, gy):
    """the test-side oracle block with bf16 storage emulated: the yardstick of the bf16 backward bound (tests/test_gpu_blocks.py)"""
    from oracle import blocks as OB
    s2 = {k: v.clone() for k, v in sd.items()}
    leaves = [k for k, v in s2.items() if v.dtype.is_floating_point and not k.endswith(('running_mean', 'running_var'))]
    for k in leaves:
        s2[k].requires_grad_(True)
    xr = x.clone().requires_grad_(True)
    with OB.bf16_storage():
        y = SO.se_bottleneck(s2, '', OB._st(xr), True, BLOCKS[name][2])
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
    tests/test_gpu_blocks.py::test_block_vs_reference_golden"""
    from gpu_harness import BlockRun
    fx = SO.block_fixture(golden, '%s_%s' % (name, mode))
    assert float(fx['gate_frac_mid'][0]) >= 0.5
    m, sd = _block(name, fx)
    x, gy = _block_io(name, fx)
    train = mode == 'train'
    m.train(train)
    run = BlockRun(m, [x], lambda g, a: m.emit(g, a), train=train, dtype=dtype)
    tol = TOL32 if dtype == 'f32' else TOLBF
    y = run.forward()
    assert_close(y, fx['y'], tol, 'y')
    ops = [o[0] for o in run.g.fwd.ops]
    assert ops.count('se_res') == 1
    if not train:
        return
    # default protocol: the BatchNorm output in front of the tail is never stored (the tail applies scale / shift itself)
    assert ops.count('affine_act') == 3 and [o[0] for o in run.g.bwd.ops].count('se_res_bwd') == 1
    gx, grads = run.backward(gy.to(DEV))
    emu = None if dtype == 'f32' else _emulated_block(name, fx, sd, x, gy)

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


@pytest.mark.parametrize('env', [{'SALT_SE_RES_IN_BN': '0'}, {'SALT_BN_FIN': '0', 'SALT_SE_SHARDS': '0'}, {'SALT_SE_SHARDS': '0'}],
                         ids=['stored', 'deterministic', 'fin-partials'])
def test_bottleneck_protocols_agree_with_golden(env, monkeypatch):
    """the stored-activation form, the deterministic protocol and consumer-finalize with per-part partials: same fixture, same bounds"""
    from gpu_harness import BlockRun
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    name = 'F17_se_bottleneck'
    fx = golden(name + '_train')
    m, sd = _block(name, fx)
    x, gy = _block_io(name, fx)
    m.train()
    run = BlockRun(m, [x], lambda g, a: m.emit(g, a), train=True, dtype='f32')
    assert_close(run.forward(), fx['y'], TOL32, 'y')
    taken = [o[0] for o in run.g.fwd.ops].count('affine_act') == 3
    assert taken == (env == {'SALT_SE_SHARDS': '0'})
    gx, grads = run.backward(gy.to(DEV))
    assert_close(gx[0], fx['gx'], 2 * TOL32, 'gx')
    for k, g in grads.items():
        assert_close(g, fx['g:' + k], 3 * TOL32, 'g:' + k)
    if 'SALT_BN_FIN' in env:                     # the fixed summation order: a second backward run gives the same bits
        gx2, grads2 = run.backward(gy.to(DEV))
        assert torch.equal(gx[0], gx2[0]) and all(torch.equal(grads[k], grads2[k]) for k in grads)


# ------------------------------------------------------------------------------------------------ whole network
def _net(depth, fx, dtype='f32'):
    from salt_amd import architectures as A
    net = NC.fill_closed_form(A.UNetSeResNet(depth, 2, dropout_2d=0.0, pretrained=False, use_hypercolumn=True))
    with torch.no_grad():
        for k, p in net.named_parameters():
            if k.endswith(SO.FC2_KEY):
                p.mul_(float(fx['fc2_scale']))
    return net.set_compute_dtype(dtype).to(DEV)


@pytest.mark.parametrize('name,depth', [('F17_unet_seresnet50_hyper', 50), ('F17_unet_seresnet101_hyper', 101)])
def test_eval_logits_and_masks_match_reference(name, depth):
    fx = golden(name)
    x = T(fx['x']).to(DEV)
    net = _net(depth, fx).eval()
    with torch.no_grad():
        logits = net(x).cpu()
    NC.check_eval_masks(logits, fx, 'seresnet eval ' + name, logits_tol=1e-3)
    ops = [o[0] for o in net.engine().net(tuple(x.shape), False).fwd.ops]
    assert ops.count('se_res') == sum(SO.COUNTS[depth])
    if depth != 50:
        return
    # bf16 storage: within 4 x what bf16 storage costs the test-side oracle (the guard factor of tests/test_gpu_emptiness.py), and the same
    # masks wherever the fp32 logit clears that
    NC.check_bf16_eval_guard(_net(depth, fx, 'bf16').eval(), x, logits, fx, 'seresnet eval bf16 ' + name, guard_factor=4)


@pytest.mark.parametrize('form', ['default', 'stored'])
def test_one_training_step_matches_reference(form, monkeypatch):
    """zero_grad -> forward -> lovasz -> backward -> Adam(lr 1e-4, L2 1e-4) as models.py:105-136, by the procedures of
    tests/net_checks.py.  Gradient norms (and sums) of tensors with 16 elements and more: within 1e-2 relative, four times what the
    fixture records for the reference's own float32 run against float64.  Tensors under 16 elements - the one-element spatial-SE
    biases (and the two-element head bias), sums over every pixel that cancel almost completely (norm 6e-4 next to 35 for the stem) -
    are bounded absolutely, within 1e-6 of the largest gradient norm, as the deep branch of
    tests/test_gpu_models.py::test_one_training_step_matches_reference bounds them; the fixture records the reference's own figure
    for them as well and it has to be a quarter of that.
    form 'stored' (SALT_SE_RES_IN_BN=0: the SE tail reads the materialised BatchNorm output): the same step, the same bounds."""
    if form == 'stored':
        monkeypatch.setenv('SALT_SE_RES_IN_BN', '0')
    fx = golden('F17_unet_seresnet50_hyper')
    assert float(fx['ref_f32_vs_f64_gradnorm_rel']) <= 2.5e-3             # the reference's own error: a quarter of the 1e-2 below
    assert float(fx['ref_f32_vs_f64_small_abs']) <= 2.5e-7                # likewise, of the 1e-6 of the largest norm below
    net = _net(50, fx)
    net.train()
    opt, out, eng, own, idx = NC.train_step_prologue(net, [T(fx['x']).to(DEV)], fx, logits_tol=2e-3, loss_tol=2e-3)
    ops = [o[0] for o in eng.net(tuple(fx['x'].shape), True).fwd.ops]
    print('seresnet train [%s]: forward program: %d se_res, %d affine_act' % (form, ops.count('se_res'), ops.count('affine_act')))
    assert ops.count('se_res') == 16
    # small tensors: five spatial-SE biases and the two-element head bias
    NC.check_grad_tally(net, eng, own, idx, fx, 'seresnet train [%s]:' % form, include_small_below_norm_floor=False, min_checked=200, n_small=6,
                        norm_tol=1e-2, sum_tol=1e-2, small_tol=1e-6, verbose=True)
    full = [k[9:] for k in fx if k.startswith('fullgrad:')]
    assert len(full) == 8
    NC.check_full_grads(eng, own, fx, full, tol=2e-2, verbose=True)
    NC.check_after_adam(opt, net, own, idx, fx, norm_tol=1e-4, sum_tol=1e-4, bn_tol=1e-3, skip_bn=None)


# ------------------------------------------------------------------------------------------------ trainer
def _model(dtype='bf16', lr=1e-3, epochs=1, cfg=None):
    return NC.family_model('UNetSeResNet', dtype, lr, epochs, cfg)


def test_fit_persist_load_and_tta(tmp_path):
    """SegmentationModel.fit for 3 steps at [2,3,64,64] (the fused step, unchanged trainer), persist -> load with and without the
    'module.' prefix -> same outputs, predict_tta = mean of the four flips done by hand."""
    from salt_amd import architectures as A, inference as I
    X, Tt = NC.square_batch(3)
    m, values = NC.fit_steps(lambda cfg: _model(dtype='f32', cfg=cfg), A.UNetSeResNet, (X, Tt), 3)
    assert m.model.encoders.encoder.layer3[5].se_module.fc1.weight.shape == (64, 1024, 1, 1)
    print('seresnet fit losses', values)
    assert values[2] < values[0]
    ck = str(tmp_path / 'ck.torch')
    m.persist(ck)
    sd = torch.load(ck, map_location='cpu')
    assert list(sd.keys()) == ['module.' + k for k in golden('F17_unet_seresnet50_hyper')['keys'].tolist()]
    net = m.model.eval()
    with torch.no_grad():
        a = net(X.to(DEV)).float().cpu()
    bare = str(tmp_path / 'bare.torch')
    torch.save({k[len('module.'):]: v for k, v in sd.items()}, bare)
    for path in (ck, bare):
        m2 = _model(dtype='f32').load(path)
        m2.model.eval()
        with torch.no_grad():
            assert torch.equal(m2.model(X.to(DEV)).float().cpu(), a), path
    prob = I.predict_tta(net, X.to(DEV), flip_ud=True, flip_lr=True).cpu()
    acc = torch.zeros_like(prob)
    with torch.no_grad():
        for ud, lr in I.tta_variants(True, True):
            dims = [k for k, f in ((2, ud), (3, lr)) if f]
            xb = torch.flip(X.to(DEV), dims).contiguous() if dims else X.to(DEV)
            p = torch.sigmoid(net(xb).float())
            acc += (torch.flip(p, dims) if dims else p).cpu()
    assert_close(prob, acc / 4, 1e-5, 'predict_tta')
