"""CPU tests of the DenseNet operator (csrc/dense.hip): the float64 references of tests/dense_op_reference.py against
F.batch_norm(training=True) -> ReLU -> 1x1 F.conv2d and autograd in double (including the gamma / beta gradients and a prefix input), the
conditions make_case promises, and the host surface (exported symbols, struct mirror, the host-side shape rules)."""
import ctypes
import re
import subprocess

import pytest
import torch
import torch.nn.functional as F

import dense_op_reference as DR

NEW_SYMBOLS = ['salt_dense_conv', 'salt_dense_conv_stats_parts', 'salt_dense_conv_dgrad', 'salt_dense_conv_dgrad_parts',
               'salt_dense_conv_wgrad', 'salt_dense_conv_wgrad_parts', 'salt_dense_moments', 'salt_dense_moments_parts', 'salt_dense_bn_prep']
EPS = 1e-5


# ------------------------------------------------------------------------------------------------ operator reference
@pytest.mark.parametrize('shape', DR.SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_op_reference_equals_batchnorm_relu_conv_and_autograd_in_double(shape):
    """x is a PREFIX of a wider buffer; gamma / beta are leaves; in_scale / in_shift / mean / invstd are what train-mode BatchNorm derives"""
    B, H, W, Cin, Cout = shape
    c = DR.make_case(B, H, W, Cin, Cout, seed=11)
    g = torch.Generator().manual_seed(5)
    wide = torch.randn(B, H, W, Cin + 32, generator=g, dtype=torch.float64)
    wide[..., :Cin] = c['x']
    buf = wide.permute(0, 3, 1, 2).clone().requires_grad_(True)
    gamma = c['gamma'].clone().requires_grad_(True)
    beta = c['in_shift'].clone().requires_grad_(True)
    w = c['w'].clone().requires_grad_(True)
    y = F.conv2d(F.relu(F.batch_norm(buf[:, :Cin], None, None, gamma, beta, True, 0.1, EPS)), w[:, :, None, None])
    y.backward(c['dy'].permute(0, 3, 1, 2))
    x = c['x']
    mean = x.mean((0, 1, 2))
    invstd = 1.0 / torch.sqrt(x.var((0, 1, 2), unbiased=False) + EPS)
    in_scale = gamma.detach() * invstd
    in_shift = beta.detach() - mean * in_scale
    a, m = DR.transform(x, in_scale, in_shift, None)
    tol = lambda ref: 1e-11 * float(ref.abs().max())
    v, A = DR.dense_conv(a, c['w'])
    ref = y.detach().permute(0, 2, 3, 1)
    assert float((v - ref).abs().max()) <= tol(ref) and bool((A >= v.abs() - 1e-12).all())
    d = DR.dense_dgrad(c['dy'], c['w'], m, x, mean, invstd, gamma.detach())
    gx = buf.grad.permute(0, 2, 3, 1)
    assert float((d['dx'] - gx[..., :Cin]).abs().max()) <= tol(gx) and float(gx[..., Cin:].abs().max()) == 0.0
    assert float((d['s1'] - beta.grad).abs().max()) <= tol(beta.grad) and float((d['s2'] - gamma.grad).abs().max()) <= tol(gamma.grad)
    gw, _ = DR.dense_wgrad(c['dy'], a)
    assert float((gw - w.grad).abs().max()) <= tol(w.grad)
    assert min(float(t.abs().max()) for t in (v, d['dx'], d['s1'], d['s2'], gw)) > 0


@pytest.mark.parametrize('shape', DR.SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_make_case_keeps_its_promises(shape):
    c = DR.make_case(*shape, seed=300 + shape[3] + 7 * shape[1] + shape[4])          # the seed of tests/test_gpu_densenet.py
    for k, t in c.items():
        assert torch.equal(t, t.bfloat16().double()), k                            # bf16-representable operands
    neg = float((c['in_scale'] < 0).double().mean())
    assert 0.05 <= neg <= 0.4, neg                                                 # 20 % of in_scale negative (a draw of Cin >= 64 values)
    assert 0.3 <= DR.masked_fraction(c) <= 0.7
    # the pinned transform: fp32 t, mask of the same t, bf16 a is a rounding of the fp32 a
    a32, m = DR.transform(c['x'], c['in_scale'], c['in_shift'], 'f32')
    a16, m16 = DR.transform(c['x'], c['in_scale'], c['in_shift'], 'bf16')
    t32 = torch.addcmul(c['in_shift'].float(), c['x'].float(), c['in_scale'].float())      # not necessarily fused: compared through the mask only where clear
    assert torch.equal(m, m16) and torch.equal(a32, a32.float().double()) and torch.equal(a16, a32.float().bfloat16().double())
    clear = t32.abs() > 1e-3
    assert bool(((t32 > 0).double() == m)[clear].all())
    for dtype in ('f32', 'bf16'):
        r = DR.forward_ref(c, dtype, True, True)
        assert bool((r['tol'] >= 0).all()) and DR.ratio(r['exact'], r) == 0.0
        d = DR.dgrad_ref(c, dtype, 1)
        assert bool((d['tol'] > 0).all()) and DR.ratio(d['exact'] + 1.0, d) > 1.0
        assert bool((d['dbeta']['tol'] >= 0).all()) and bool((d['dgamma']['tol'] >= 0).all())      # 0 only where a channel is masked at every pixel
        g = DR.wgrad_ref(c, dtype, 0)
        assert DR.ratio(g['exact'], g) == 0.0 and DR.ratio(g['exact'] * 1.01 + 1e-3, g) > 1.0


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
    assert abi.lib.salt_abi_version() >= 30
    for s in ('salt_dense_conv', 'salt_dense_conv_dgrad', 'salt_dense_conv_wgrad'):
        assert s in abi.OP_FUNCS and s + '_args' in abi.STRUCTS
    # the host-side shape rules answer without a GPU
    UNS = abi.CONSTS['SALT_E_UNSUPPORTED']
    v = lambda C, B=2: shaped_view(1 << 20, B, 34, 18, C)
    parts = lambda Cin, Cout, B=2: abi.lib.salt_dense_conv_stats_parts(ctypes.byref(abi.fill(abi.STRUCTS['salt_dense_conv_args'](), dtype=1, x=v(Cin, B), y=v(Cout, B))))
    assert parts(64, 128) == 10 and parts(2048, 1024, B=1) == 5 and parts(32, 64) == 10
    assert parts(48, 128) == UNS and b'48 input channels' in abi.lib.salt_last_error()
    assert parts(2080, 128) == UNS and parts(64, 96) == UNS and b'96 output channels' in abi.lib.salt_last_error()
    dparts = lambda Cin, Cout: abi.lib.salt_dense_conv_dgrad_parts(ctypes.byref(abi.fill(abi.STRUCTS['salt_dense_conv_dgrad_args'](), dtype=1, x=v(Cin), dy=v(Cout))))
    assert dparts(96, 128) == 10 and dparts(48, 128) == UNS and dparts(64, 1088) == UNS
    splits = lambda Cin, Cout, B=2: abi.lib.salt_dense_conv_wgrad_parts(ctypes.byref(abi.fill(abi.STRUCTS['salt_dense_conv_wgrad_args'](), dtype=1, x=v(Cin, B), dy=v(Cout, B))))
    assert splits(160, 128, B=1) == 3 and splits(64, 128, B=1) == 3 and splits(48, 128) == UNS and splits(64, 96) == UNS
    # one split per 8 chunks of 32 pixels at the least, about 512 workgroups per launch at the most
    assert splits(1024, 128, B=64) == 16 and splits(64, 128, B=64) == 153


# ------------------------------------------------------------------------------------------------ architecture, registry, fixtures
NET_FX = 'F19_unet_densenet121_hyper'


def test_oracle_reproduces_reference_network():
    """tests/densenet_oracle.py against what the reference's own UNetDenseNet produced (tolerances of tests/test_seresnext_cpu.py for F18:
    logits 1e-4, gradient norms 2e-3, full gradients 2e-3, statistics 1e-4), and the conditions the generator recorded"""
    import numpy as np
    from helpers import golden, T, assert_close
    import closed_form as CF
    import densenet_oracle as DO
    from oracle import losses as OL, specs as OS
    fx = golden(NET_FX)
    spec = DO.spec_unet_densenet(121)
    assert set(DO.expand_aliases({k: None for k in spec})) == set(fx['keys'].tolist())
    sd = DO.closed_form_state(spec)
    x = CF.input_for(str(fx['input_tag']), tuple(int(v) for v in fx['x_shape']))
    assert np.array_equal(x.numpy(), fx['x'])
    passed = []
    with torch.no_grad():
        logits = DO.unet_densenet(sd, x, False, passed=passed)
    assert_close(logits, fx['eval_logits'], 1e-4, 'eval logits')
    # the fixture's own conditions: the masks have a margin, both classes occur, the middle norm1 ReLU of every block is half open
    under = np.abs(fx['eval_logits'][:, 1]) < 10 * float(fx['ref_f32_vs_f64_maxabs'])
    assert int(under.sum()) == int(fx['margin_pixels']) <= 0.001 * under.size
    ref_mask = fx['eval_logits'][:, 1] > 0
    assert ref_mask.any() and not ref_mask.all()
    assert np.array_equal((logits[:, 1] > 0).numpy()[~under], ref_mask[~under])
    assert len(passed) == 4 and all(0.2 <= f <= 0.8 for f in passed)
    assert all(abs(a - b) < 1e-3 for a, b in zip(passed, fx['relu_pass_mid_eval'].tolist()))
    assert all(0.2 <= f <= 0.8 for f in fx['relu_pass_mid_train'].tolist())
    assert 0 < float(fx['ref_f32_vs_f64_gradnorm_rel']) <= 2.5e-3 and 0 < float(fx['ref_f32_vs_f64_small_abs']) <= 2.5e-7
    assert 0 < float(fx['ref_bf16_storage_vs_f32_maxabs']) < float(np.abs(fx['eval_logits']).max())
    assert not any(k.startswith(('w:', 'p:')) for k in fx) and 'state' not in fx             # no weights in the fixture
    # one training step
    t = T(fx['t'])
    dead = ('last_linear', 'norm5')
    train_keys = [k for k in OS.trainable_keys(spec) if not any(d in k for d in dead)]
    for k in train_keys:
        sd[k].requires_grad_(True)
    out = DO.unet_densenet(sd, x, True)
    assert_close(out, fx['train_logits'], 1e-4, 'train logits')
    loss = OL.lovasz_loss(out, t)
    loss.backward()
    assert abs(float(loss.detach()) - float(fx['train_loss'])) < 1e-4 * max(1.0, abs(float(fx['train_loss'])))
    idx = {n: i for i, n in enumerate(fx['param_names'].tolist())}
    assert int(fx['param_has_grad'].sum()) == len(train_keys)
    checked = 0
    for k in train_keys:
        i = idx[k]
        assert bool(fx['param_has_grad'][i]), k
        if fx['grad_norm'][i] <= 1e-4 or sd[k].numel() < 16:
            continue
        gn = float(sd[k].grad.double().norm())
        assert abs(gn - fx['grad_norm'][i]) <= 2e-3 * fx['grad_norm'][i], (k, gn, fx['grad_norm'][i])
        checked += 1
    assert checked > 300
    import make_golden_densenet as MG
    assert fx['fullgrad_keys'].tolist() == list(MG.FULL_REQUIRED) and len(MG.FULL_REQUIRED) == 19      # the generator's fixed, required list
    assert float(fx['fullgrad_ref_f32_vs_f64'].max()) <= 5e-3      # a quarter of the GPU test's 2e-2
    for k in fx['fullgrad_keys'].tolist():
        assert_close(sd[k].grad, fx['fullgrad:' + k], 2e-3, k)
    for k, s in zip(fx['bn_keys'].tolist(), fx['bn_sum'].tolist()):
        assert abs(float(sd[k].double().sum()) - s) <= 1e-4 * max(1.0, abs(s)), k


def test_state_dict_layout_registry_and_signature():
    import inspect
    from helpers import golden
    from salt_amd import architectures as A, models
    fx = golden(NET_FX)
    net = A.UNetDenseNet(121, 2, use_hypercolumn=True)
    sd = net.state_dict()
    assert list(sd.keys()) == fx['keys'].tolist()
    assert ['x'.join(str(d) for d in v.shape) for v in sd.values()] == fx['key_shapes'].tolist()
    assert net.dead_parameter_names() == ['encoders.encoder.features.norm5.weight', 'encoders.encoder.features.norm5.bias',
                                          'encoders.encoder.last_linear.weight', 'encoders.encoder.last_linear.bias']
    assert net.output_shape((4, 3, 128, 128)) == (4, 2, 128, 128) and not net.uses_depth
    assert list(inspect.signature(A.UNetDenseNet.__init__).parameters) == ['self', 'encoder_depth', 'num_classes', 'dropout_2d', 'pretrained', 'use_hypercolumn', 'pool0']
    assert list(inspect.signature(A.DenseNetEncoders.__init__).parameters) == ['self', 'encoder_depth', 'pretrained', 'pool0']
    assert models.ARCHITECTURES['UNetDenseNet'] == {
        'model': A.UNetDenseNet,
        'model_config': {'encoder_depth': 121, 'use_hypercolumn': True, 'dropout_2d': 0.0, 'pretrained': False, 'pool0': False},
        'init_weights': False}
    # decoder widths from the four encoder widths: center[1] outputs enc[2], dec5 takes enc[3] + enc[2]
    assert tuple(sd['center.1.conv.weight'].shape) == (1024, 1024, 3, 3) and tuple(sd['dec5.conv1.conv.weight'].shape) == (1024, 2048, 3, 3)
    assert tuple(sd['dec4.conv1.conv.weight'].shape) == (512, 1024 + 128, 3, 3) and tuple(sd['dec2.conv1.conv.weight'].shape) == (128, 256 + 128, 3, 3)
    # the dotted keys of torchvision 0.2.0 checkpoints round-trip
    dotted = A.UNetDenseNet.translate_keys(sd, dotted=True)
    assert 'encoders.encoder.features.denseblock1.denselayer1.norm.1.weight' in dotted and 'encoders.encoder2.denselayer6.conv.2.weight' in dotted
    assert not any('.norm1.' in k or '.conv2.' in k for k in dotted if 'denselayer' in k)
    assert list(A.UNetDenseNet.translate_keys(dotted)) == list(sd)
    before = {k: v.clone() for k, v in sd.items()}
    net.load_state_dict({k: (v + 1 if v.dtype.is_floating_point else v) for k, v in dotted.items()})
    assert all(torch.equal(net.state_dict()[k], before[k] + 1) for k in before if before[k].dtype.is_floating_point)


def test_error_paths():
    from salt_amd import architectures as A
    from salt_amd._abi import SaltError
    with pytest.raises(NotImplementedError, match='161'):
        A.UNetDenseNet(161, 2)
    for depth in (169, 201):
        with pytest.raises(NotImplementedError, match='dec5.channel_se.*power of two'):
            A.UNetDenseNet(depth, 2)
    with pytest.raises(NotImplementedError, match='only 121, 161, 169, 201 version of Densenet are implemented'):
        A.UNetDenseNet(50, 2)
    with pytest.raises(SaltError, match='download'):
        A.UNetDenseNet(121, 2, pretrained='imagenet')
    with pytest.raises(SaltError, match='pool0'):
        A.UNetDenseNet(121, 2, pool0=True)
    net = A.UNetDenseNet(121, 2)
    with pytest.raises(SaltError):
        net(torch.zeros(1, 3, 64, 64))                    # CPU tensor: no fallback
    with pytest.raises(SaltError):
        net.encoders.encoder.features.denseblock1.denselayer1(torch.zeros(1, 64, 8, 8))


def test_segmentation_model_construction():
    from salt_amd import architectures as A, models
    arch = {'model_params': {'architecture': 'UNetDenseNet', 'out_channels': 2, 'activation': 'sigmoid', 'loss': 'lovasz', 'compute_dtype': 'bf16'},
            'optimizer_params': {'lr': 1e-4}, 'regularizer_params': {'regularize': True, 'weight_decay_conv2d': 1e-4}}
    m = models.SegmentationModel(arch, {'epochs': 1}, {})
    assert isinstance(m.model, A.UNetDenseNet) and m.model.compute_dtype == 'bf16' and m.model.use_hypercolumn


def test_oracle_reproduces_the_dense_block_fixture():
    """denseblock1 + transition1: tests/densenet_oracle.py against what the stub's modules produced; the fixture holds no weights"""
    from helpers import golden, assert_close
    import closed_form as CF
    import densenet_oracle as DO
    from salt_amd import architectures as A
    fx, ev = golden('F19_dense_block_train'), golden('F19_dense_block_eval')
    assert not any(k.startswith('s:') and not k.endswith(('running_mean', 'running_var')) for k in fx) and set(ev) == {'y', 'gx', 'x_shape', 'input_tag'}
    m = torch.nn.Module()
    m.block, m.transition = A._DenseBlock(6, 64, 4, 32, 0), A._Transition(256, 128)
    state = lambda: {k: CF.tensor_for(k, v.shape).to(v.dtype) for k, v in m.state_dict().items()}
    sd = state()
    x = CF.input_for(str(fx['input_tag']), tuple(int(v) for v in fx['x_shape'])).requires_grad_(True)
    gy = CF.input_for('gy:%s' % (tuple(fx['y'].shape),), fx['y'].shape)
    leaves = [k for k, v in sd.items() if v.dtype.is_floating_point and not k.endswith(('running_mean', 'running_var'))]
    for k in leaves:
        sd[k].requires_grad_(True)
    passed = []
    y = DO.transition(sd, 'transition.', DO.dense_block(sd, 'block.', x, True, 6, passed), True)
    assert_close(y, fx['y'], 2e-5, 'y')
    assert 0.2 <= passed[0] <= 0.8
    y.backward(gy)
    assert_close(x.grad, fx['gx'], 1e-4, 'gx')
    full = [k for k in leaves if 'g:' + k in fx]
    assert len(full) == len(leaves) - 4 == 35
    for k in full:
        assert_close(sd[k].grad, fx['g:' + k], 2e-4, k)
    for k in sd:
        if k.endswith(('running_mean', 'running_var')):
            assert_close(sd[k], fx['s:' + k], 1e-5, k)
    with torch.no_grad():
        ye = DO.transition(state(), 'transition.', DO.dense_block(state(), 'block.', x.detach(), False, 6), False)
    assert_close(ye, ev['y'], 2e-5, 'eval y')


def test_oracle_reproduces_the_dense_layer_fixture():
    """one layer on a 96-channel prefix: tests/densenet_oracle.py against what the stub's _DenseLayer produced; the fixture holds no weights"""
    from helpers import golden, assert_close
    import closed_form as CF
    import densenet_oracle as DO
    from salt_amd import architectures as A
    fx, ev = golden('F19_dense_layer_train'), golden('F19_dense_layer_eval')
    assert not any(k.startswith('s:') and not k.endswith(('running_mean', 'running_var')) for k in fx) and set(ev) == {'y', 'gx', 'x_shape', 'input_tag'}
    m = A._DenseLayer(96, 32, 4, 0)
    state = lambda: {k: CF.tensor_for(k, v.shape).to(v.dtype) for k, v in m.state_dict().items()}
    sd = state()
    shape = tuple(int(v) for v in fx['x_shape'])
    assert shape == (3, 96, 9, 7) and shape[0] * shape[2] * shape[3] > 128 and (shape[0] * shape[2] * shape[3]) % 128       # two pixel tiles, the second ragged
    x = CF.input_for(str(fx['input_tag']), shape).requires_grad_(True)
    gy = CF.input_for('gy:%s' % (tuple(fx['y'].shape),), fx['y'].shape)
    leaves = [k for k, v in sd.items() if v.dtype.is_floating_point and not k.endswith(('running_mean', 'running_var'))]
    for k in leaves:
        sd[k].requires_grad_(True)
    passed = []
    y = torch.cat([x, DO.dense_layer(sd, '', x, True, passed)], 1)
    assert_close(y, fx['y'], 2e-5, 'y')
    assert 0.2 <= passed[0] <= 0.8
    y.backward(gy)
    assert_close(x.grad, fx['gx'], 1e-4, 'gx')
    assert len(leaves) == 6
    for k in leaves:
        assert_close(sd[k].grad, fx['g:' + k], 2e-4, k)
    for k in sd:
        if k.endswith(('running_mean', 'running_var')):
            assert_close(sd[k], fx['s:' + k], 1e-5, k)
    with torch.no_grad():
        s2 = state()
        ye = torch.cat([x.detach(), DO.dense_layer(s2, '', x.detach(), False)], 1)
    assert_close(ye, ev['y'], 2e-5, 'eval y')
