"""CPU tests of LargeKernelMatters: the float64 operator references of gcn_op_reference.py against torch's own ReplicationPad2d + conv2d
and autograd in double (both branches, and the closed-form adjoint with its two edge terms), the host-side shape rules of
salt_gcn_pair (no GPU is touched), the architecture's state dict, signatures, registry entry and error paths, and tests/lkm_oracle.py
against the F21 fixtures the reference produced."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gcn_op_reference as GR

NEW_SYMBOLS = ['salt_gcn_pair', 'salt_gcn_pair_stats_parts', 'salt_gcn_pair_dgrad']
NET_FX = 'F21_lkm34'
F64 = torch.float64
nchw = lambda t: t.permute(0, 3, 1, 2)
nhwc = lambda t: t.permute(0, 2, 3, 1)


# ------------------------------------------------------------------------------------------------ the references against torch
@pytest.mark.parametrize('H,W,K', [(6, 11, 9), (4, 4, 9), (1, 17, 9), (33, 20, 3), (16, 16, 2), (5, 7, 4)], ids=lambda v: str(v))
def test_references_match_torch_and_autograd(H, W, K):
    """pair_fwd is ReplicationPad2d((0, 0, K-1, 0)) + conv2d(K x 1) and ReplicationPad2d((0, K-1, 0, 0)) + conv2d(1 x K); pair_dgrad - the
    closed form with the prefix / suffix edge terms - is autograd's gradient of both, in double"""
    g = torch.Generator().manual_seed(100 * H + 10 * W + K)
    B, C, N = 2, 8, 5
    x = torch.randn(B, H, W, C, generator=g, dtype=F64, requires_grad=True)
    wv, wh = torch.randn(N, C, K, generator=g, dtype=F64), torch.randn(N, C, K, generator=g, dtype=F64)
    v, h = GR.pair_fwd(x.detach(), wv, wh)
    tv = F.conv2d(torch.nn.ReplicationPad2d((0, 0, K - 1, 0))(nchw(x)), wv[:, :, :, None])
    th = F.conv2d(torch.nn.ReplicationPad2d((0, K - 1, 0, 0))(nchw(x)), wh[:, :, None, :])
    assert tuple(tv.shape) == (B, N, H, W) == tuple(th.shape)
    scale = float(tv.abs().max())
    assert float((v - nhwc(tv).detach()).abs().max()) <= 1e-13 * scale and float((h - nhwc(th).detach()).abs().max()) <= 1e-13 * scale
    gv, gh = torch.randn(B, H, W, N, generator=g, dtype=F64), torch.randn(B, H, W, N, generator=g, dtype=F64)
    ((tv * nchw(gv)).sum() + (th * nchw(gh)).sum()).backward()
    dx = GR.pair_dgrad(gv, gh, wv, wh)
    assert float((dx - x.grad).abs().max()) <= 1e-13 * float(x.grad.abs().max())
    # each branch alone, so that a compensating error between the two edge terms cannot hide
    zero = torch.zeros_like(gv)
    xv = x.detach().clone().requires_grad_(True)
    F.conv2d(torch.nn.ReplicationPad2d((0, 0, K - 1, 0))(nchw(xv)), wv[:, :, :, None]).backward(nchw(gv).contiguous())
    assert float((GR.pair_dgrad(gv, zero, wv, wh) - xv.grad).abs().max()) <= 1e-13 * float(xv.grad.abs().max())
    xh = x.detach().clone().requires_grad_(True)
    F.conv2d(torch.nn.ReplicationPad2d((0, K - 1, 0, 0))(nchw(xh)), wh[:, :, None, :]).backward(nchw(gh).contiguous())
    assert float((GR.pair_dgrad(zero, gh, wv, wh) - xh.grad).abs().max()) <= 1e-13 * float(xh.grad.abs().max())
    # the term count of the bound: 2 K inside, more on row 0 and on column W - 1
    T = GR.dgrad_terms(H, W, N, K)
    assert float(T.max()) <= N * (2 * K + K * (K - 1)) and float(T.min()) >= N * min(K, 2)
    assert float(T.sum()) == N * 2 * K * H * W          # every (pixel, tap) of the forward pass lands on exactly one element of dx


def test_reference_bounds_are_positive_and_cover_the_storage_rounding():
    c = GR.make_case(2, 6, 10, 64, 21, 9, seed=1)
    for k in ('x', 'wv', 'wh', 'dyv', 'dyh', 'dx_old'):
        assert torch.equal(c[k], c[k].bfloat16().double()), k          # bf16-representable operands
    for dtype in ('f32', 'bf16'):
        for r in GR.fwd_ref(c, dtype, 'eval', (1, 0)) + GR.fwd_ref(c, dtype, 'train') + [GR.dgrad_ref(c, dtype, 0), GR.dgrad_ref(c, dtype, 1)]:
            assert bool((r['tol'] > 0).all()) and float(r['tol'].max()) < 0.1 * float(r['exact'].abs().max())
            assert GR.ratio(r['exact'], r) == 0.0
            if dtype == 'bf16':
                assert GR.ratio(r['exact'].bfloat16().double(), r) <= 1.0


# ------------------------------------------------------------------------------------------------ host surface
def test_new_symbols_and_host_side_shape_rules():
    from salt_amd import _abi as abi
    from salt_amd.engine import shaped_view
    with open(abi.HEADER) as f:
        header = f.read()
    out = subprocess.run(['nm', '-D', '--defined-only', abi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r'\b(salt_\w+)$', out, flags=re.M))
    for s in NEW_SYMBOLS:
        assert re.search(r'^int %s\(' % s, header, flags=re.M), s
        assert s in abi.DECLARED_SYMBOLS and s in exported, s
    assert abi.lib.salt_abi_version() >= 32
    assert 'gcn.hip' in open(os.path.join(os.path.dirname(abi.LIB_PATH), 'csrc', 'build.py')).read()
    UNS = abi.CONSTS['SALT_E_UNSUPPORTED']
    S = abi.STRUCTS['salt_gcn_pair_args']

    def parts(B=2, H=6, W=10, Cin=64, Cout=21, K=9, dtype=1, xoff=0, ycs=24):
        x = shaped_view((1 << 20) + xoff, B, H, W, Cin)
        y = lambda p: shaped_view(p, B, H, W, Cout, ycs)
        return abi.lib.salt_gcn_pair_stats_parts(ctypes.byref(abi.fill(S(), dtype=dtype, x=x, K=K, yv=y(1 << 21), yh=y(1 << 22))))
    assert parts() == 2 and parts(H=9, W=17) == 2 * 2 * 2 and parts(B=32, H=64, W=64) == 32 * 8 * 4          # 8 x 16 pixel tiles
    assert parts(H=1, W=1, Cin=8, Cout=1, K=2, ycs=8) == 2 and parts(Cin=2048, Cout=32, ycs=32, dtype=0) == 2 and parts(K=4) == 2
    for kw, text in ((dict(Cin=20), b'20 input channels'), (dict(Cout=33, ycs=40), b'33'), (dict(K=10), b'kernel size 10'),
                     (dict(xoff=8), b'16-byte aligned'), (dict(ycs=21), b'16-byte aligned'), (dict(K=1), b'kernel size 1'),
                     (dict(Cin=2056), b'2056 input channels'), (dict(dtype=7), b'dtype')):
        assert parts(**kw) == UNS and text in abi.lib.salt_last_error(), (kw, abi.lib.salt_last_error())
    fn, D = abi.OP_FUNCS['salt_gcn_pair_dgrad']
    v = shaped_view(1 << 20, 2, 6, 10, 20)
    y = shaped_view(1 << 21, 2, 6, 10, 21, 24)
    assert fn(ctypes.byref(abi.fill(D(), dtype=1, dyv=y, dyh=y, wv=1 << 22, wh=1 << 22, K=9, dx=v)), None) == UNS      # refused on the host: nothing launched


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


@pytest.mark.parametrize('fxname,mode', [('F21_gcn', 'train'), ('F21_gcn', 'eval'), ('F21_gcn_norelu', 'train'), ('F21_br', 'train'), ('F21_br', 'eval')])
def test_oracle_reproduces_the_block_fixtures(fxname, mode):
    from helpers import golden, assert_close
    import lkm_oracle as LO
    fx = golden('%s_%s' % (fxname, mode))
    gcn, relu = fxname != 'F21_br', fxname == 'F21_gcn'
    assert tuple(fx['x_shape']) == ((2, 64, 6, 10) if gcn else (2, 21, 5, 7)) and float(fx['ref_f32_vs_f64']) <= 5e-5 / 4
    assert len(fx['fractions']) == (4 if relu else 0 if gcn else 1) and all(0.2 <= f <= 0.8 for f in fx['fractions'].tolist())
    assert os.path.getsize(os.path.join(os.path.dirname(__file__), 'golden', '%s_%s.npz' % (fxname, mode))) < 1 << 20
    sd = LO.closed_form_state(LO.spec_gcn(64, 21, 9) if gcn else LO.spec_br(21, 3))
    passed = []
    fn = (lambda s, a: LO.gcn(s, '', a, mode == 'train', relu, passed)) if gcn else (lambda s, a: LO.boundary_refinement(s, '', a, mode == 'train', passed))
    x, y, leaves = _run_block(fn, sd, fx)
    assert_close(y, fx['y'], 2e-5, 'y')
    assert len(passed) == len(fx['fractions']) and all(abs(a - b) < 1e-3 for a, b in zip(passed, fx['fractions'].tolist()))
    assert_close(x.grad, fx['gx'], 1e-4, 'gx')
    assert sorted(leaves) == sorted(k[2:] for k in fx if k.startswith('g:')) and len(leaves) == (16 if gcn else 8)
    wmax = max(float(np.abs(fx['g:' + k]).max()) for k in leaves)
    for k in leaves:
        if k.endswith('conv.bias') and mode == 'train':          # in front of a train-mode BatchNorm: analytically zero, rounding noise in the fixture
            assert float(np.abs(fx['g:' + k]).max()) <= 1e-5 * wmax
            continue
        assert_close(sd[k].grad, fx['g:' + k], 2e-4, k)
    if mode == 'train':
        for k in sd:
            if k.endswith(('running_mean', 'running_var')):
                assert_close(sd[k], fx['s:' + k], 1e-5, k)


def test_oracle_reproduces_reference_network():
    """tests/lkm_oracle.py against what the reference's own LargeKernelMatters produced (tolerances of tests/test_psp_cpu.py for F20:
    logits 1e-4, gradient norms 2e-3, full gradients 2e-3, statistics 1e-4), and the conditions the generator recorded"""
    from helpers import golden, T, assert_close
    import closed_form as CF
    import lkm_oracle as LO
    import make_golden_lkm as MG
    from oracle import losses as OL, specs as OS
    fx = golden(NET_FX)
    big = golden(NET_FX + '_gcn5_grads')
    for name in (NET_FX, NET_FX + '_gcn5_grads'):
        assert os.path.getsize(os.path.join(os.path.dirname(__file__), 'golden', name + '.npz')) < 1 << 20
    spec = LO.spec_lkm(34)
    assert set(LO.expand_aliases({k: None for k in spec})) == set(fx['keys'].tolist()) and len(fx['keys']) == 688
    sd = LO.closed_form_state(spec)
    sd['final.bias'] = T(fx['final_bias']).clone()
    assert torch.equal(sd['final.bias'][:1], CF.tensor_for('final.bias', (2,))[:1])          # at most the class-1 bias was moved
    x = CF.input_for(str(fx['input_tag']), tuple(int(v) for v in fx['x_shape']))
    assert np.array_equal(x.numpy(), fx['x']) and tuple(x.shape) == (2, 3, 64, 64)           # encoder5 is 4x4: every vertical tap of gcn5 clamps
    passed = []
    with torch.no_grad():
        logits = LO.lkm(sd, x, False, passed=passed)
    assert_close(logits, fx['eval_logits'], 1e-4, 'eval logits')
    under = np.abs(fx['eval_logits'][:, 1]) < 10 * float(fx['ref_f32_vs_f64_maxabs'])
    assert int(under.sum()) == int(fx['margin_pixels']) <= 0.001 * under.size
    ref_mask = fx['eval_logits'][:, 1] > 0
    assert 0.2 <= ref_mask.mean() <= 0.8                                                      # both classes, in bulk
    assert np.array_equal((logits[:, 1] > 0).numpy()[~under], ref_mask[~under])
    assert len(fx['fractions_eval']) == 28 == len(fx['fractions_train'])                      # 16 in the GCN blocks, 8 in the refinements, 4 deconvs
    assert all(0.2 <= f <= 0.8 for f in fx['fractions_eval'].tolist() + fx['fractions_train'].tolist())
    assert len(passed) == 24 and all(0.2 <= f <= 0.8 for f in passed)                         # the oracle reports the GCN and refinement ReLUs
    assert 0 < float(fx['ref_f32_vs_f64_gradnorm_rel']) <= 2.5e-3 and 0 < float(fx['ref_f32_vs_f64_small_abs']) <= 2.5e-7
    assert 0 <= float(fx['ref_post_step_stability']) <= 0.25e-4
    # how the input was chosen is part of the fixture: the tags tried before it, each with the guard that refused it
    assert fx['refused_tags'].tolist() == ['f21', 'f21:1', 'f21:2'] and str(fx['input_tag']) == 'f21:3'
    assert len(fx['refused_why']) == 3 and all('Adam step' in w for w in fx['refused_why'].tolist())
    assert 0 < float(fx['ref_bf16_storage_vs_f32_maxabs']) < float(np.abs(fx['eval_logits']).max())
    assert not any(k.startswith(('w:', 'p:', 's:')) for k in fx) and 'state' not in fx       # no weights but the two bias values
    # one training step
    t = T(fx['t'])
    train_keys = [k for k in OS.trainable_keys(spec) if '.fc.' not in k]
    for k in train_keys:
        sd[k].requires_grad_(True)
    out = LO.lkm(sd, x, True)
    assert_close(out, fx['train_logits'], 1e-4, 'train logits')
    loss = OL.lovasz_loss(out, t)
    loss.backward()
    assert abs(float(loss.detach()) - float(fx['train_loss'])) < 1e-4 * max(1.0, abs(float(fx['train_loss'])))
    idx = {n: i for i, n in enumerate(fx['param_names'].tolist())}
    assert int(fx['param_has_grad'].sum()) == len(train_keys) == 254
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
    assert fx['fullgrad_keys'].tolist() == list(MG.FULL_REQUIRED) and sorted(k[9:] for k in big) == sorted(MG.BIG)
    for k in ('gcn5.conv1.0.conv.weight', 'gcn5.conv2.0.conv.weight', 'encoders.encoder.layer4.2.bn2.weight'):
        assert k in MG.FULL_REQUIRED
    assert float(fx['fullgrad_ref_f32_vs_f64'].max()) <= 5e-3      # a quarter of the GPU test's 2e-2
    for k in fx['fullgrad_keys'].tolist():
        assert_close(sd[k].grad, (big if k in MG.BIG else fx)['fullgrad:' + k], 2e-3, k)
    for k, s in zip(fx['bn_keys'].tolist(), fx['bn_sum'].tolist()):
        assert abs(float(sd[k].double().sum()) - s) <= 1e-4 * max(1.0, abs(s)), k


# ------------------------------------------------------------------------------------------------ architecture, registry, error paths
def test_state_dict_layout_registry_and_signature():
    import inspect
    from helpers import golden
    from salt_amd import architectures as A, models
    fx = golden(NET_FX)
    net = A.LargeKernelMatters(34, 2)
    sd = net.state_dict()
    assert list(sd.keys()) == fx['keys'].tolist() and len(sd) == 688
    assert ['x'.join(str(d) for d in v.shape) for v in sd.values()] == fx['key_shapes'].tolist()
    keys = list(sd)
    assert keys.index('gcn2.conv1.0.batch_norm.weight') < keys.index('gcn2.conv1.0.conv.weight')          # batch_norm.* before conv.*
    assert tuple(sd['gcn5.conv1.0.conv.weight'].shape) == (21, 512, 9, 1) and tuple(sd['gcn5.conv2.0.conv.weight'].shape) == (21, 512, 1, 9)
    assert tuple(sd['gcn2.conv1.1.conv.weight'].shape) == (21, 21, 1, 9) and tuple(sd['deconv5.deconv.weight'].shape) == (21, 21, 3, 3)
    assert tuple(sd['enc_br2.conv.1.conv.weight'].shape) == (21, 21, 3, 3) and tuple(sd['final.weight'].shape) == (2, 21, 1, 1)
    assert net.dead_parameter_names() == ['encoders.encoder.fc.weight', 'encoders.encoder.fc.bias']
    assert net.output_shape((4, 3, 128, 128)) == (4, 2, 128, 128) and not net.uses_depth
    sig = lambda f: list(inspect.signature(f).parameters)
    dflt = lambda f: {k: v.default for k, v in inspect.signature(f).parameters.items() if v.default is not inspect.Parameter.empty}
    assert sig(A.LargeKernelMatters.__init__) == ['self', 'encoder_depth', 'num_classes', 'kernel_size', 'internal_channels', 'use_relu', 'pretrained',
                                                  'dropout_2d', 'pool0']
    assert dflt(A.LargeKernelMatters.__init__) == dict(kernel_size=9, internal_channels=21, use_relu=False, pretrained=False, dropout_2d=0.0, pool0=False)
    assert sig(A.GlobalConvolutionalNetwork.__init__) == ['self', 'in_channels', 'out_channels', 'kernel_size', 'use_relu']
    assert dflt(A.GlobalConvolutionalNetwork.__init__) == dict(use_relu=False)
    assert sig(A.BoundaryRefinement.__init__) == ['self', 'in_channels', 'out_channels', 'kernel_size'] and dflt(A.BoundaryRefinement.__init__) == {}
    assert models.ARCHITECTURES['LargeKernelMatters'] == {
        'model': A.LargeKernelMatters,
        'model_config': {'encoder_depth': 34, 'pretrained': False, 'kernel_size': 9, 'internal_channels': 21, 'dropout_2d': 0.0, 'use_relu': True,
                         'pool0': False},
        'init_weights': False}
    for depth, widths in ((18, (64, 128, 256, 512)), (50, (256, 512, 1024, 2048))):
        n = A.LargeKernelMatters(depth, 2)
        assert tuple(getattr(n, 'gcn%d' % i).conv1[0].conv.weight.shape[1] for i in (2, 3, 4, 5)) == widths
        assert tuple(getattr(n, 'gcn%d' % i).conv2[0].conv.weight.shape[1] for i in (2, 3, 4, 5)) == widths
        assert [k for k in n.state_dict() if not k.startswith('encoders.')] == [k for k in keys if not k.startswith('encoders.')]
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
    with pytest.raises(SaltError, match='download'):
        A.LargeKernelMatters(34, 2, pretrained=True)
    with pytest.raises(SaltError, match='pool0'):
        A.LargeKernelMatters(34, 2, pool0=True)
    with pytest.raises(NotImplementedError, match='only 18, 34, 50, 101, 152 version of Resnet are implemented'):
        A.LargeKernelMatters(121, 2)
    for kw in (dict(kernel_size=10), dict(kernel_size=1), dict(kernel_size=11), dict(internal_channels=33)):
        with pytest.raises(SaltError, match='salt_gcn_pair'):
            A.LargeKernelMatters(34, 2, **kw)
    with pytest.raises(SaltError, match='salt_gcn_pair'):
        A.GlobalConvolutionalNetwork(64, 21, 10)
    for depth in (101, 152):
        assert A.LargeKernelMatters(depth, 2).gcn5.conv1[0].conv.weight.shape[1] == 2048
    A.LargeKernelMatters(18, 2, kernel_size=4, internal_channels=8)                            # even K is legal: the pad is one-sided
    net = A.LargeKernelMatters(34, 2, dropout_2d=0.5)          # accepted and ignored: an identity under the reference's torch
    assert net.dropout_2d == 0.5
    with pytest.raises(SaltError):
        net(torch.zeros(1, 3, 64, 64))                    # CPU tensor: no fallback
    with pytest.raises(SaltError):
        net.gcn5(torch.zeros(1, 512, 4, 4))
    with pytest.raises(SaltError, match='multiples of 16'):
        net.output_shape((1, 3, 72, 64))


def test_segmentation_model_construction():
    from salt_amd import architectures as A, models
    arch = {'model_params': {'architecture': 'LargeKernelMatters', 'out_channels': 2, 'activation': 'sigmoid', 'loss': 'lovasz', 'compute_dtype': 'bf16'},
            'optimizer_params': {'lr': 1e-4}, 'regularizer_params': {'regularize': True, 'weight_decay_conv2d': 1e-4}}
    m = models.SegmentationModel(arch, {'epochs': 1}, {})
    assert isinstance(m.model, A.LargeKernelMatters) and m.model.compute_dtype == 'bf16' and m.model.paired is None
    assert all(blk.conv1[0].use_relu for blk in (m.model.gcn2, m.model.gcn5))               # the registry turns the ReLUs on
    # every parameter the reference trains is in the one group the optimizer steps, with its weight decay
    from salt_amd.optim import weight_regularization
    groups = weight_regularization(m.model, True, 1e-4)
    ids = {id(p) for p in groups[0]['params']}
    dead = set(m.model.dead_parameter_names())
    assert groups[0]['weight_decay'] == 1e-4
    assert all(id(p) in ids for k, p in m.model.named_parameters() if k not in dead)


def test_shape_rule_of_the_pair_follows_the_table_in_both_directions():
    """Graph.gcn_pair_composed against profiles/lkm_bench.json, the table tools/lkm_bench.py measured with the pair FORCED on its paired
    side: a shape takes the composed route if and only if the block with the pair measured slower, forward + backward, by more than the
    spread of the two figures.  Today that is every row."""
    import json
    from types import SimpleNamespace as V
    from salt_amd.engine import Graph
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'lkm_bench.json')) as f:
        doc = json.load(f)
    assert doc['commit'] and set(doc['train_step_ms']) == {'lkm34', 'lkm34_pair_everywhere', 'unet_resnet34'} == set(doc['eval_forward_ms'])
    rows = {tuple(r['shape']): r for r in doc['block']}
    assert set(rows) == {(32, 64, 64, 64), (32, 128, 32, 32), (32, 256, 16, 16), (32, 512, 8, 8), (32, 2048, 8, 8),
                         (2, 64, 32, 32), (2, 128, 16, 16), (2, 256, 8, 8), (2, 512, 4, 4)}
    for (B, C, h, w), r in rows.items():
        assert r['entries_ms']['paired'].get('fwd:gcn_pair', 0) > 0 and r['entries_ms']['paired'].get('bwd:gcn_pair_dgrad', 0) > 0, (B, C, h)   # the paired side ran the pair
        spread = r['paired_fwd_bwd_spread_ms'] + r['composed_fwd_bwd_spread_ms']
        slower = r['paired_fwd_bwd_ms'] > r['composed_fwd_bwd_ms'] + spread
        assert Graph.gcn_pair_composed(V(B=B, H=h, W=w, C=C), 9) == slower, ((B, C, h, w), r['paired_fwd_bwd_ms'], r['composed_fwd_bwd_ms'], spread)


def test_fused_fold_question_of_the_composed_data_gradient():
    """Graph._dgrad asks salt_conv_stats_parts whether the fused fold of a long line kernel's data gradient has tiles larger than its pad
    of 8, and takes the strip fold only on THAT refusal.  The host side of the question, without a GPU: the [2,64,32,32] map of the F21
    network refuses the (9, 1) kernel with exactly that text and accepts the (1, 9) one; the benchmark maps accept both; [8,64,64,64] refuses the (9, 1) kernel again."""
    from salt_amd import _abi as abi
    from salt_amd.engine import shaped_view
    K = 9

    def ask(B, H, W, C, vertical):
        t, r = (K - 1, 0) if vertical else (0, K - 1)
        td = [(-(k - (K - 1)) - t, 0) for k in range(K)] if vertical else [(0, -k) for k in range(K)]
        S = abi.fill(abi.STRUCTS['salt_conv_args'](), dtype=1, x=shaped_view(1 << 20, B, H, W, 21, 24), w=1 << 22, ntaps=K, tap_dy=[a for a, _ in td],
                     tap_dx=[b for _, b in td], in_step=1, pad_mode=0, y=shaped_view(1 << 21, B, H, W, C), OH=H + t, OW=W + r, out_step=1, fold_top=t,
                     fold_right=r)
        n = abi.lib.salt_conv_stats_parts(ctypes.byref(S))
        return n, abi.lib.salt_last_error().decode(errors='replace')
    n, text = ask(2, 32, 32, 64, True)
    assert n < 0 and 'fused fold needs tiles larger than the pad' in text
    assert ask(2, 32, 32, 64, False)[0] > 0
    for shape in ((32, 64, 64, 64), (32, 8, 8, 512)):
        assert ask(*shape, True)[0] > 0 and ask(*shape, False)[0] > 0, shape
    assert ask(8, 64, 64, 64, True)[0] < 0 and ask(8, 64, 64, 64, False)[0] > 0          # the plan's tile follows the batch as well
