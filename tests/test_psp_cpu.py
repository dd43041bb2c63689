"""CPU tests of PSPNet: the adaptive-bin and resize index tables of tests/psp_op_reference.py against hand-computed values, its float64
references against torch's own adaptive_avg_pool2d / interpolate / prelu and autograd in double, the host surface of csrc/psp.hip, the
comparator tests/psp_oracle.py against the F20 fixtures the reference produced, and the architecture's keys, registry entry, error
paths and state-dict round trip."""
import ctypes
import re
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import psp_op_reference as PR

NEW_SYMBOLS = ['salt_psp_pool', 'salt_psp_pool_bwd', 'salt_psp_merge', 'salt_psp_merge_bwd', 'salt_psp_merge_bwd_parts', 'salt_bn_prelu',
               'salt_bn_prelu_bwd', 'salt_bn_prelu_bwd_parts']
NET_FX = 'F20_pspnet34_hyper'
nchw = lambda t: t.permute(0, 3, 1, 2)
nhwc = lambda t: t.permute(0, 2, 3, 1)


# ------------------------------------------------------------------------------------------------ index tables, by hand
def test_adaptive_bins_match_hand_computed_tables():
    # rows [floor(i h / s), ceil((i + 1) h / s))
    assert PR.bins(8, 3) == [(0, 3), (2, 6), (5, 8)]                                   # overlapping: rows 2 and 5 are in two bins
    assert PR.bins(8, 6) == [(0, 2), (1, 3), (2, 4), (4, 6), (5, 7), (6, 8)]
    assert PR.bins(4, 6) == [(0, 1), (0, 2), (1, 2), (2, 3), (2, 4), (3, 4)]           # s > h: bins repeat pixels
    assert PR.bins(5, 1) == [(0, 5)]
    for n, s in ((8, 3), (8, 6), (4, 6), (5, 1)):
        x = torch.arange(float(n), dtype=torch.float64).reshape(1, 1, n, 1)
        ref = F.adaptive_avg_pool2d(x, (s, 1)).flatten().tolist()
        assert ref == [sum(range(lo, hi)) / (hi - lo) for lo, hi in PR.bins(n, s)]


def test_resize_taps_match_hand_computed_tables():
    # align_corners = 0: src = max(0, (d + 0.5) s / h - 0.5)
    assert PR.resize_taps(8, 3, 0) == [(0, 1, 1.0, 0.0), (0, 1, 0.9375, 0.0625), (0, 1, 0.5625, 0.4375), (0, 1, 0.1875, 0.8125),
                                       (1, 2, 0.8125, 0.1875), (1, 2, 0.4375, 0.5625), (1, 2, 0.0625, 0.9375), (2, 2, 0.6875, 0.3125)]
    assert PR.resize_taps(8, 6, 0) == [(0, 1, 1.0, 0.0), (0, 1, 0.375, 0.625), (1, 2, 0.625, 0.375), (2, 3, 0.875, 0.125),
                                       (2, 3, 0.125, 0.875), (3, 4, 0.375, 0.625), (4, 5, 0.625, 0.375), (5, 5, 0.875, 0.125)]
    assert PR.resize_taps(4, 6, 0) == [(0, 1, 0.75, 0.25), (1, 2, 0.25, 0.75), (3, 4, 0.75, 0.25), (4, 5, 0.25, 0.75)]
    # s = 1: both taps are source 0 whatever src is (0, 0, 0, 0.1, 0.3 for d = 0 .. 4): their weights add up to 1
    assert [(a, b) for a, b, _, _ in PR.resize_taps(5, 1, 0)] == [(0, 0)] * 5
    assert np.allclose([w1 for _, _, _, w1 in PR.resize_taps(5, 1, 0)], [0, 0, 0, 0.2, 0.4], atol=2e-7)
    assert np.allclose(PR.resize_matrix(5, 1, 0).numpy(), 1.0, atol=2e-7)
    # align_corners = 1: src = d (s - 1) / (h - 1), and 0 when s = 1
    t = PR.resize_taps(8, 3, 1)
    assert [(a, b) for a, b, _, _ in t] == [(0, 1)] * 4 + [(1, 2)] * 3 + [(2, 2)]
    assert np.allclose([w1 for _, _, _, w1 in t], [0, 2 / 7, 4 / 7, 6 / 7, 1 / 7, 3 / 7, 5 / 7, 0], atol=2e-7)
    t = PR.resize_taps(8, 6, 1)
    assert [(a, b) for a, b, _, _ in t] == [(0, 1), (0, 1), (1, 2), (2, 3), (2, 3), (3, 4), (4, 5), (5, 5)]
    assert np.allclose([w1 for _, _, _, w1 in t], [0, 5 / 7, 3 / 7, 1 / 7, 6 / 7, 4 / 7, 2 / 7, 0], atol=2e-7)
    t = PR.resize_taps(4, 6, 1)
    assert [(a, b) for a, b, _, _ in t] == [(0, 1), (1, 2), (3, 4), (5, 5)]
    assert np.allclose([w1 for _, _, _, w1 in t], [0, 2 / 3, 1 / 3, 0], atol=2e-7)
    assert PR.resize_taps(5, 1, 1) == [(0, 0, 1.0, 0.0)] * 5
    assert PR.resize_taps(1, 3, 1) == [(0, 1, 1.0, 0.0)]
    for n, s in ((8, 3), (8, 6), (4, 6), (5, 1)):
        for ac in (0, 1):
            M = PR.resize_matrix(n, s, ac)
            assert np.allclose(M.sum(1).numpy(), 1.0, atol=2e-7)
            ref = F.interpolate(torch.eye(s).reshape(1, s, s, 1), size=(n, 1), mode='bilinear', align_corners=bool(ac))[0, :, :, 0].T
            assert float((M - ref.double()).abs().max()) <= 2e-7, (n, s, ac)


# ------------------------------------------------------------------------------------------------ operator references against torch in double
@pytest.mark.parametrize('shape', PR.PSP_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_psp_references_equal_torch_and_autograd_in_double(shape):
    B, h, w, C = shape
    c = PR.make_psp_case(B, h, w, C, 64, seed=3)
    for k, t in c.items():
        for v in (t if isinstance(t, list) else [t]):
            assert torch.equal(v, v.bfloat16().double()), k
    x = nchw(c['x']).clone().requires_grad_(True)
    ps = [F.adaptive_avg_pool2d(x, s) for s in PR.SIZES]
    for s, p, mine in zip(PR.SIZES, ps, PR.pool(c['x'])):
        assert float((nhwc(p.detach()) - mine).abs().max()) <= 1e-13, s
    torch.autograd.backward(ps, [nchw(d) for d in c['dp']])
    dx, A, T = PR.pool_bwd(c['dp'], h, w)
    assert float((dx - nhwc(x.grad)).abs().max()) <= 1e-12 and bool((A >= dx.abs() - 1e-12).all())
    assert T.min() >= 4 and (T.max() > 4) == (h % 6 != 0 or w % 6 != 0)           # every pixel is in at least one bin per stage
    # the resize weights are fp32 values: the source index (up to s - 1 = 5) carries three fp32 roundings per axis, so torch in double
    # agrees to about 2 * 3 * 5 * 2^-24 = 2e-6 of the summed magnitudes
    for ac in (0, 1):
        f = nchw(c['f']).clone().requires_grad_(True)
        qs = [nchw(q).clone().requires_grad_(True) for q in c['q']]
        bias = c['bias'].clone().requires_grad_(True)
        v = f + bias[None, :, None, None]
        for q in qs:
            v = v + F.interpolate(q, size=(h, w), mode='bilinear', align_corners=bool(ac))
        y = F.relu(v)
        mine, A = PR.merge(c['f'], c['bias'], c['q'], ac)
        assert float((mine - nhwc(v.detach())).abs().max()) <= 3e-6 * float(A.max())
        dy = nchw(c['dy'])
        y.backward(dy)
        g, dqs, As, db, Ab = PR.merge_bwd(c['dy'], nhwc(y.detach()), ac)
        assert torch.equal(g, nhwc(f.grad))
        assert float((db - bias.grad).abs().max()) <= 1e-12 * float(Ab.max())
        for q, d, a in zip(qs, dqs, As):
            assert float((d - nhwc(q.grad)).abs().max()) <= 3e-6 * float(a.max())
    for dtype in ('f32', 'bf16'):
        r = PR.merge_ref(c, dtype, 0)
        assert PR.ratio(r['exact'], r) == 0.0 and PR.ratio(r['exact'] + 1.0, r) > 1.0
        for r in PR.pool_ref(c, dtype):
            assert bool((r['tol'] >= 0).all()) and PR.ratio(r['exact'] * 1.01 + 1e-3, r) > 1.0
        b = PR.merge_bwd_ref(c, dtype, 1, 1)
        assert float(b['df']['tol'].max()) == 0.0 and PR.ratio(b['dbias']['exact'] + 1.0, b['dbias']) > 1.0
        assert 0.2 <= float((c['y'] > 0).double().mean()) <= 0.8


@pytest.mark.parametrize('shape', PR.PRELU_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_bn_prelu_references_equal_torch_and_autograd_in_double(shape):
    c = PR.make_prelu_case(*shape, seed=5)
    assert 0.2 <= PR.negative_fraction(c) <= 0.8
    for alpha in PR.ALPHAS:
        y = nchw(c['y']).clone().requires_grad_(True)
        al = torch.tensor([alpha], dtype=torch.float64, requires_grad=True)
        u = y * c['scale'][None, :, None, None] + c['shift'][None, :, None, None]
        a = F.prelu(u, al)
        a.backward(nchw(c['da']))
        u0 = PR.pre_activation(c['y'], c['scale'], c['shift'], pinned=False)
        assert torch.equal(PR.prelu(u0, alpha), nhwc(a.detach()))
        pinned = PR.pre_activation(c['y'], c['scale'], c['shift'])
        assert torch.equal(pinned, pinned.float().double()) and float((pinned - u0).abs().max()) <= 2.0 ** -23 * float(u0.abs().max())
        # the gradients through the pinned pre-activation differ from autograd only where the fp32 rounding moved u across zero: nowhere here
        assert torch.equal(pinned > 0, u0 > 0)
        r = PR.bn_prelu_bwd_ref(c, 'f32', alpha, 0)
        assert float((r['du']['exact'] * c['scale'] - nhwc(y.grad)).abs().max()) <= 1e-12
        assert abs(float(r['dalpha']['exact']) - float(al.grad)) <= 2e-7 * float(r['dalpha']['tol'] / PR.U32 / c['y'].numel())


# ------------------------------------------------------------------------------------------------ host surface
def test_new_symbols_are_in_the_header_and_the_library():
    from salt_amd import _abi as abi
    from salt_amd.engine import shaped_view
    with open(abi.HEADER) as f:
        header = f.read()
    out = subprocess.run(['nm', '-D', '--defined-only', abi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r'\b(salt_\w+)$', out, flags=re.M))
    for s in NEW_SYMBOLS:
        assert re.search(r'^int %s\(' % s, header, flags=re.M), s
        assert s in abi.DECLARED_SYMBOLS and s in exported, s
    assert abi.lib.salt_abi_version() >= 31
    order = list(abi.STRUCTS)
    assert order[-6:] == ['salt_psp_pool_args', 'salt_psp_pool_bwd_args', 'salt_psp_merge_args', 'salt_psp_merge_bwd_args', 'salt_bn_prelu_args',
                          'salt_bn_prelu_bwd_args']                                  # appended last: salt_abi_struct_sizes keeps its order
    # the host-side rules answer without a GPU: nothing is launched for a refused shape
    UNS, BAD = abi.CONSTS['SALT_E_UNSUPPORTED'], abi.CONSTS['SALT_E_BADARG']
    v = lambda h, C, B=2: shaped_view(1 << 20, B, h, h, C)
    fn, S = abi.OP_FUNCS['salt_psp_pool']
    pool = lambda h, C, sizes: fn(ctypes.byref(abi.fill(S(), dtype=1, x=v(h, C), nsizes=len(sizes), sizes=list(sizes),
                                                        p=[v(s, C) for s in sizes])), None)
    assert pool(33, 64, (1, 2, 3, 6)) == UNS and b'at most 32 x 32' in abi.lib.salt_last_error()
    assert pool(8, 36, (1, 2, 3, 6)) == UNS and b'multiple of 8' in abi.lib.salt_last_error()
    assert pool(8, 64, (1, 2, 3, 7)) == UNS and b'pyramid size 7' in abi.lib.salt_last_error()
    assert pool(8, 64, (1, 1, 1, 1, 1)[:0]) == UNS
    parts = lambda B: abi.lib.salt_psp_merge_bwd_parts(ctypes.byref(abi.fill(abi.STRUCTS['salt_psp_merge_bwd_args'](), dtype=1, dy=v(8, 64, B))))
    assert parts(2) == 2 and parts(32) == 32
    pparts = lambda B, H, C, dt: abi.lib.salt_bn_prelu_bwd_parts(ctypes.byref(abi.fill(abi.STRUCTS['salt_bn_prelu_bwd_args'](), dtype=dt,
                                                                                     y=shaped_view(1 << 20, B, H, H, C))))
    assert pparts(2, 3, 16, 0) == 1 and pparts(4, 32, 64, 0) == 64 and pparts(4, 32, 64, 1) == 32 and pparts(32, 128, 64, 1) == 1024
    fn, S = abi.OP_FUNCS['salt_bn_prelu']
    assert fn(ctypes.byref(abi.fill(S(), dtype=0, y=v(3, 12), a=v(3, 12), alpha=1 << 20)), None) == UNS
    assert fn(ctypes.byref(abi.fill(S(), dtype=0, y=v(3, 16), a=v(3, 16), alpha=None)), None) == BAD


# ------------------------------------------------------------------------------------------------ oracle == fixtures
def _run_block(fn, sd, fx):
    import closed_form as CF
    x = CF.input_for(str(fx['input_tag']), tuple(int(v) for v in fx['x_shape'])).requires_grad_(True)
    gy = CF.input_for('gy:%s' % (tuple(fx['y'].shape),), fx['y'].shape)
    leaves = [k for k, v in sd.items() if v.dtype.is_floating_point and not k.endswith(('running_mean', 'running_var'))]
    for k in leaves:
        sd[k].requires_grad_(True)
    y = fn(sd, x)
    y.backward(gy)
    return x, y, leaves


def test_oracle_reproduces_the_psp_module_fixture():
    from helpers import golden, assert_close
    import psp_oracle as PO
    for mode in ('train', 'eval'):
        fx = golden('F20_psp_module_%s' % mode)
        assert tuple(fx['x_shape']) == (2, 64, 8, 8) and 0.2 <= float(fx['fraction']) <= 0.8 and float(fx['ref_f32_vs_f64']) <= 5e-5 / 4
        assert not any(k.startswith('s:') for k in fx)                                        # no weights in the fixture
        sd = PO.closed_form_state(PO.spec_psp_module(64, 128))
        passed = []
        x, y, leaves = _run_block(lambda s, a: PO.psp_module(s, '', a, passed=passed), sd, fx)
        assert_close(y, fx['y'], 2e-5, 'y')
        assert abs(passed[0] - float(fx['fraction'])) < 1e-3
        assert_close(x.grad, fx['gx'], 1e-4, 'gx')
        assert sorted(leaves) == sorted(k[2:] for k in fx if k.startswith('g:')) and len(leaves) == 6
        for k in leaves:
            assert_close(sd[k].grad, fx['g:' + k], 2e-4, k)


def test_oracle_reproduces_the_psp_upsample_fixture():
    from helpers import golden, assert_close
    import psp_oracle as PO
    for mode in ('train', 'eval'):
        fx = golden('F20_psp_upsample_%s' % mode)
        alpha = float(fx['alpha'])
        assert tuple(fx['x_shape']) == (2, 32, 5, 7) and alpha not in (0.0, 1.0, 0.25) and 0.2 <= float(fx['fraction']) <= 0.8
        assert float(fx['ref_f32_vs_f64']) <= 5e-5 / 4
        sd = PO.closed_form_state(PO.spec_psp_upsample(32, 16))
        sd['conv.2.weight'] = torch.full((1,), alpha)
        passed = []
        x, y, leaves = _run_block(lambda s, a: PO.psp_upsample(s, '', a, mode == 'train', passed), sd, fx)
        assert_close(y, fx['y'], 2e-5, 'y')
        assert abs(passed[0] - float(fx['fraction'])) < 1e-3
        assert_close(x.grad, fx['gx'], 1e-4, 'gx')
        assert sorted(leaves) == sorted(k[2:] for k in fx if k.startswith('g:')) and len(leaves) == 5
        for k in leaves:
            if k == 'conv.0.bias' and mode == 'train':          # in front of a train-mode BatchNorm: analytically zero, rounding noise in the fixture
                assert float(np.abs(fx['g:' + k]).max()) <= 1e-5 * float(np.abs(fx['g:conv.0.weight']).max())
                continue
            assert_close(sd[k].grad, fx['g:' + k], 2e-4, k)
        if mode == 'train':
            for k in ('conv.1.running_mean', 'conv.1.running_var'):
                assert_close(sd[k], fx['s:' + k], 1e-5, k)


def test_oracle_reproduces_reference_network():
    """tests/psp_oracle.py against what the reference's own PSPNet produced (tolerances of tests/test_densenet_cpu.py for F19: logits
    1e-4, gradient norms 2e-3, full gradients 2e-3, statistics 1e-4), and the conditions the generator recorded"""
    from helpers import golden, T, assert_close
    import closed_form as CF
    import psp_oracle as PO
    from oracle import losses as OL, specs as OS
    fx = golden(NET_FX)
    spec = PO.spec_pspnet(34)
    assert set(PO.expand_aliases({k: None for k in spec})) == set(fx['keys'].tolist())
    sd = PO.closed_form_state(spec)
    sd['final.1.bias'] = T(fx['final_1_bias']).clone()
    assert torch.equal(sd['final.1.bias'][:1], CF.tensor_for('final.1.bias', (2,))[:1])          # only the class-1 bias was moved
    x = CF.input_for(str(fx['input_tag']), tuple(int(v) for v in fx['x_shape']))
    assert np.array_equal(x.numpy(), fx['x']) and tuple(x.shape) == (2, 3, 64, 64)               # encoder5 is 4x4: the s = 6 stage repeats bins
    passed = []
    with torch.no_grad():
        logits = PO.pspnet(sd, x, False, passed=passed)
    assert_close(logits, fx['eval_logits'], 1e-4, 'eval logits')
    under = np.abs(fx['eval_logits'][:, 1]) < 10 * float(fx['ref_f32_vs_f64_maxabs'])
    assert int(under.sum()) == int(fx['margin_pixels']) <= 0.001 * under.size
    ref_mask = fx['eval_logits'][:, 1] > 0
    assert 0.2 <= ref_mask.mean() <= 0.8                                                         # both classes, in bulk
    assert np.array_equal((logits[:, 1] > 0).numpy()[~under], ref_mask[~under])
    assert len(passed) == 5 and all(0.2 <= f <= 0.8 for f in passed)
    assert all(abs(a - b) < 1e-3 for a, b in zip(passed, fx['fractions_eval'].tolist()))
    assert all(0.2 <= f <= 0.8 for f in fx['fractions_train'].tolist())
    assert 0 < float(fx['ref_f32_vs_f64_gradnorm_rel']) <= 2.5e-3 and 0 < float(fx['ref_f32_vs_f64_small_abs']) <= 2.5e-7
    assert 0 < float(fx['ref_bf16_storage_vs_f32_maxabs']) < float(np.abs(fx['eval_logits']).max())
    assert not any(k.startswith(('w:', 'p:', 's:')) for k in fx) and 'state' not in fx         # no weights but the two bias values
    # one training step
    t = T(fx['t'])
    train_keys = [k for k in OS.trainable_keys(spec) if '.fc.' not in k]
    for k in train_keys:
        sd[k].requires_grad_(True)
    out = PO.pspnet(sd, x, True)
    assert_close(out, fx['train_logits'], 1e-4, 'train logits')
    loss = OL.lovasz_loss(out, t)
    loss.backward()
    assert abs(float(loss.detach()) - float(fx['train_loss'])) < 1e-4 * max(1.0, abs(float(fx['train_loss'])))
    idx = {n: i for i, n in enumerate(fx['param_names'].tolist())}
    assert int(fx['param_has_grad'].sum()) == len(train_keys) == 140
    checked = 0
    for k in train_keys:
        i = idx[k]
        assert bool(fx['param_has_grad'][i]), k
        if fx['grad_norm'][i] <= 1e-4 or sd[k].numel() < 16:
            continue
        gn = float(sd[k].grad.double().norm())
        assert abs(gn - fx['grad_norm'][i]) <= 2e-3 * fx['grad_norm'][i], (k, gn, fx['grad_norm'][i])
        checked += 1
    assert checked > 120
    import make_golden_psp as MG
    assert fx['fullgrad_keys'].tolist() == list(MG.FULL_REQUIRED) and len(MG.FULL_REQUIRED) == 17
    assert float(fx['fullgrad_ref_f32_vs_f64'].max()) <= 5e-3      # a quarter of the GPU test's 2e-2
    for k in fx['fullgrad_keys'].tolist():
        assert_close(sd[k].grad, fx['fullgrad:' + k], 2e-3, k)
    for k, s in zip(fx['bn_keys'].tolist(), fx['bn_sum'].tolist()):
        assert abs(float(sd[k].double().sum()) - s) <= 1e-4 * max(1.0, abs(s)), k


# ------------------------------------------------------------------------------------------------ architecture, registry, error paths
def test_state_dict_layout_registry_and_signature():
    import inspect
    from helpers import golden
    from salt_amd import architectures as A, models
    fx = golden(NET_FX)
    net = A.PSPNet(34, 2, use_hypercolumn=True)
    sd = net.state_dict()
    assert list(sd.keys()) == fx['keys'].tolist()
    assert ['x'.join(str(d) for d in v.shape) for v in sd.values()] == fx['key_shapes'].tolist()
    for k in ['psp.stages.%d.1.weight' % i for i in range(4)] + ['psp.bottleneck.weight', 'psp.bottleneck.bias', 'final.0.conv.weight', 'final.1.bias'] \
            + ['up%d.conv.%s' % (n, leaf) for n in (4, 3, 2, 1) for leaf in ('0.weight', '0.bias', '1.weight', '1.running_var', '2.weight')]:
        assert k in sd, k
    assert tuple(sd['up4.conv.2.weight'].shape) == (1,) and tuple(sd['psp.bottleneck.weight'].shape) == (1024, 2560, 1, 1)
    assert tuple(sd['final.0.conv.weight'].shape) == (64, 960, 3, 3)
    assert net.dead_parameter_names() == ['encoders.encoder.fc.weight', 'encoders.encoder.fc.bias']
    assert net.output_shape((4, 3, 128, 128)) == (4, 2, 128, 128) and not net.uses_depth
    assert list(inspect.signature(A.PSPNet.__init__).parameters) == ['self', 'encoder_depth', 'num_classes', 'sizes', 'deep_features_size', 'dropout_2d',
                                                                      'pretrained', 'use_hypercolumn', 'pool0']
    d = {k: v.default for k, v in inspect.signature(A.PSPNet.__init__).parameters.items() if v.default is not inspect.Parameter.empty}
    assert d == dict(num_classes=2, sizes=(1, 2, 3, 6), deep_features_size=1024, dropout_2d=0.2, pretrained=False, use_hypercolumn=False, pool0=False)
    assert list(inspect.signature(A.PSPModule.__init__).parameters) == ['self', 'features', 'out_features', 'sizes']
    assert list(inspect.signature(A.PSPUpsample.__init__).parameters) == ['self', 'in_channels', 'out_channels']
    assert models.ARCHITECTURES['PSPNet'] == {'model': A.PSPNet,
                                              'model_config': {'encoder_depth': 34, 'pretrained': False, 'use_hypercolumn': True, 'pool0': False},
                                              'init_weights': False}
    assert list(A.PSPNet(18, 2, use_hypercolumn=True).state_dict())[-12:] == list(sd)[-12:]
    # load_state_dict round trip on CPU tensors, keys as the reference spells them (no translation)
    before = {k: v.clone() for k, v in sd.items()}
    net.load_state_dict({k: (v + 1 if v.dtype.is_floating_point else v) for k, v in before.items()})
    assert all(torch.equal(net.state_dict()[k], before[k] + 1) for k in before if before[k].dtype.is_floating_point)
    old = {k: v for k, v in before.items() if not k.endswith('num_batches_tracked')}          # a torch 0.3.1 checkpoint
    net.load_state_dict(old)
    assert all(torch.equal(net.state_dict()[k], before[k]) for k in old)


def test_error_paths():
    from salt_amd import architectures as A
    from salt_amd._abi import SaltError
    for depth in (50, 101, 152):
        with pytest.raises(NotImplementedError, match='3840'):
            A.PSPNet(depth, 2, use_hypercolumn=True)
    with pytest.raises(NotImplementedError, match='only 18, 34, 50, 101, 152 version of Resnet are implemented'):
        A.PSPNet(121, 2, use_hypercolumn=True)
    with pytest.raises(SaltError, match='use_hypercolumn=False does not run in the reference either'):
        A.PSPNet(34, 2)
    with pytest.raises(SaltError, match='download'):
        A.PSPNet(34, 2, use_hypercolumn=True, pretrained=True)
    with pytest.raises(SaltError, match='pool0'):
        A.PSPNet(34, 2, use_hypercolumn=True, pool0=True)
    with pytest.raises(SaltError, match='sizes'):
        A.PSPNet(34, 2, sizes=(1, 2, 4), use_hypercolumn=True)
    net = A.PSPNet(34, 2, dropout_2d=0.5, use_hypercolumn=True)         # accepted and ignored: an identity under the reference's torch
    assert net.dropout_2d == 0.5
    with pytest.raises(SaltError):
        net(torch.zeros(1, 3, 64, 64))                    # CPU tensor: no fallback
    with pytest.raises(SaltError):
        net.psp(torch.zeros(1, 512, 4, 4))
    with pytest.raises(SaltError, match='multiples of 16'):
        net.output_shape((1, 3, 72, 64))


def test_segmentation_model_construction():
    from salt_amd import architectures as A, models
    arch = {'model_params': {'architecture': 'PSPNet', 'out_channels': 2, 'activation': 'sigmoid', 'loss': 'lovasz', 'compute_dtype': 'bf16'},
            'optimizer_params': {'lr': 1e-4}, 'regularizer_params': {'regularize': True, 'weight_decay_conv2d': 1e-4}}
    m = models.SegmentationModel(arch, {'epochs': 1}, {})
    assert isinstance(m.model, A.PSPNet) and m.model.compute_dtype == 'bf16' and m.model.use_hypercolumn and m.model.dropout_2d == 0.2
    # every parameter the reference trains is in the one group the optimizer steps, with its weight decay: the four slopes among them
    from salt_amd.optim import weight_regularization
    groups = weight_regularization(m.model, True, 1e-4)
    ids = {id(p) for p in groups[0]['params']}
    assert groups[0]['weight_decay'] == 1e-4 and all(id(getattr(m.model, u).conv[2].weight) in ids for u in ('up4', 'up3', 'up2', 'up1'))
