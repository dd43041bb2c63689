"""CPU tests of UNetSeResNet: the operator reference tests/se_res_op_reference.py against torch autograd of the plain module
composition, the comparator tests/seresnet_oracle.py against the F17 fixtures the reference produced, and the host surface (state_dict
layout, registry, error paths, trainer construction, exported symbols)."""
import os
import re
import subprocess
from collections import OrderedDict

import numpy as np
import pytest
import torch

from helpers import golden, T, assert_close
import closed_form as CF
import se_res_op_reference as SR
import seresnet_oracle as SO
from oracle import losses as OL, specs as OS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ['salt_se_res', 'salt_se_res_parts', 'salt_se_res_bwd', 'salt_se_res_fc_grads']


# ------------------------------------------------------------------------------------------------ operator reference
@pytest.mark.parametrize('shape', [(2, 4, 4, 256), (3, 3, 5, 256), (1, 1, 1, 2048), (2, 2, 2, 64)])
@pytest.mark.parametrize('affine', [0, 1])
def test_op_reference_equals_autograd_in_double(shape, affine):
    c = SR.make_case(*shape, seed=7, affine=affine)
    leaves = {k: c[k].clone().requires_grad_(True) for k in ('x', 'res', 'w1', 'b1', 'w2', 'b2')}
    y = SR.module_composition(leaves['x'], c['scale'], c['shift'], leaves['res'], leaves['w1'], leaves['b1'], leaves['w2'], leaves['b2'])
    y.backward(c['dy'])
    f = SR.se_res(c['x'], c['scale'], c['shift'], c['res'], c['w1'], c['b1'], c['w2'], c['b2'])
    b = SR.se_res_bwd(f, c['dy'], c['w1'], c['w2'])
    tol = lambda ref: 1e-12 * max(1.0, float(ref.abs().max()))
    assert float((f['y'] - y.detach()).abs().max()) <= tol(y.detach())
    # dL/dx of the composition = scale * dL/dz (the BatchNorm in front is outside the operator)
    dz = leaves['x'].grad / c['scale'] if affine else leaves['x'].grad
    assert float((b['dx'] - dz).abs().max()) <= tol(dz)
    assert float((b['dres'] - leaves['res'].grad).abs().max()) <= tol(leaves['res'].grad)
    for k, leaf in (('g_w1', 'w1'), ('g_b1', 'b1'), ('g_w2', 'w2'), ('g_b2', 'b2')):
        assert float((b[k] - leaves[leaf].grad).abs().max()) <= tol(leaves[leaf].grad), k
    assert float(b['g_w1'].abs().max()) > 0 and float(((f['gate'] > 0.1) & (f['gate'] < 0.9)).double().mean()) >= 0.5
    old = torch.full_like(c['dy'], 3.0)
    assert torch.equal(SR.se_res_bwd(f, c['dy'], c['w1'], c['w2'], old)['dres'], b['dres'] + 3.0)


# ------------------------------------------------------------------------------------------------ fixtures vs the comparator
BLOCKS = {'F17_se_bottleneck': (64, 64, 1, 256, 'f17a'), 'F17_se_bottleneck_s2': (256, 128, 2, 512, 'f17b')}


def _block_state(name, fx):
    cin, planes, stride, cout, _ = BLOCKS[name]
    shapes = OrderedDict([('conv1.weight', (planes, cin, 1, 1)), ('conv2.weight', (planes, planes, 3, 3)), ('conv3.weight', (cout, planes, 1, 1)),
                             ('se_module.fc1.weight', (cout // 16, cout, 1, 1)), ('se_module.fc1.bias', (cout // 16,)),
                             ('se_module.fc2.weight', (cout, cout // 16, 1, 1)), ('se_module.fc2.bias', (cout,)),
                             ('downsample.0.weight', (cout, cin, 1, 1))])
    for p, ch in (('bn1.', planes), ('bn2.', planes), ('bn3.', cout), ('downsample.1.', cout)):
        for leaf in ('weight', 'bias', 'running_mean', 'running_var'):
            shapes[p + leaf] = (ch,)
        shapes[p + 'num_batches_tracked'] = ()
    sd = CF.state_for(shapes.items())
    sd['se_module.fc2.weight'] = sd['se_module.fc2.weight'] * float(fx['fc2_scale'])
    return sd


@pytest.mark.parametrize('name', sorted(BLOCKS))
def test_oracle_block_reproduces_the_bottleneck_fixture(name):
    fx = SO.block_fixture(golden, name + '_train')
    assert int(fx['companions']) == (2 if name.endswith('s2') else 0)
    sd = _block_state(name, fx)
    shape = tuple(int(v) for v in fx['x_shape'])
    x = (T(fx['x']) if 'x' in fx else CF.input_for(BLOCKS[name][4], shape)).requires_grad_(True)
    gy = T(fx['gy']) if 'gy' in fx else CF.input_for('gy:%s' % (tuple(fx['y'].shape),), fx['y'].shape)
    leaves = [k for k, v in sd.items() if v.dtype.is_floating_point and not k.endswith(('running_mean', 'running_var'))]
    for k in leaves:
        sd[k].requires_grad_(True)
    gates = []
    y = SO.se_bottleneck(sd, '', x, True, BLOCKS[name][2], gates)
    assert_close(y, fx['y'], 2e-5, 'y')
    y.backward(gy)
    assert_close(x.grad, fx['gx'], 1e-4, 'gx')
    n = 0
    for k in leaves:
        assert_close(sd[k].grad, fx['g:' + k], 2e-4, k)
        n += 1
    assert n == 16
    for k in sd:
        if k.endswith(('running_mean', 'running_var')):
            assert_close(sd[k], fx['s:' + k], 1e-5, k)
    frac = float(((gates[0] >= 0.1) & (gates[0] <= 0.9)).float().mean())
    assert frac >= 0.5 and abs(frac - float(fx['gate_frac_mid'][0])) < 1e-6
    ev = golden(name + '_eval')
    with torch.no_grad():
        ye = SO.se_bottleneck(_block_state(name, ev), '', x.detach(), False, BLOCKS[name][2])
    assert_close(ye, ev['y'], 2e-5, 'eval y')


@pytest.mark.parametrize('name,depth,trains', [('F17_unet_seresnet50_hyper', 50, True), ('F17_unet_seresnet101_hyper', 101, False)])
def test_oracle_reproduces_reference_network(name, depth, trains):
    """logits <= 1e-3 relative as for F8 (measured far below: asserted at the 1e-4 of the F14 / F15 CPU tests), gradient norms within
    the 2e-3 of tests/test_depth_cpu.py / tests/test_emptiness_cpu.py"""
    fx = golden(name)
    spec = SO.spec_unet_seresnet(depth, with_last_linear=True)
    assert list(SO.expand_aliases({k: None for k in spec})) != [] and set(SO.expand_aliases({k: None for k in spec})) == set(fx['keys'].tolist())
    sd = SO.closed_form_state(spec, float(fx['fc2_scale']))
    x = CF.input_for(str(fx['input_tag']), tuple(int(v) for v in fx['x_shape']))
    assert np.array_equal(x.numpy(), fx['x'])
    gates = []
    with torch.no_grad():
        logits = SO.unet_seresnet(sd, x, False, depth=depth, gates=gates)
    assert_close(logits, fx['eval_logits'], 1e-4, 'eval logits')
    for stage, rec in zip(gates, fx['gate_frac_mid_eval'].tolist()):
        g = torch.cat([t.reshape(-1) for t in stage])
        frac = float(((g >= 0.1) & (g <= 0.9)).float().mean())
        assert frac >= 0.5 and abs(frac - rec) < 1e-3, (frac, rec)
    under = np.abs(fx['eval_logits'][:, 1]) < 10 * float(fx['ref_f32_vs_f64_maxabs'])
    assert int(under.sum()) == int(fx['margin_pixels']) <= 0.001 * under.size
    assert np.array_equal((logits[:, 1] > 0).numpy()[~under], (fx['eval_logits'][:, 1] > 0)[~under])
    if not trains:
        assert 'train_loss' not in fx
        return
    t = T(fx['t'])
    train_keys = [k for k in OS.trainable_keys(spec) if 'last_linear' not in k]
    for k in train_keys:
        sd[k].requires_grad_(True)
    out = SO.unet_seresnet(sd, x, True, depth=depth)
    assert_close(out, fx['train_logits'], 1e-4, 'train logits')
    loss = OL.lovasz_loss(out, t)
    loss.backward()
    assert abs(float(loss) - float(fx['train_loss'])) < 1e-4 * max(1.0, abs(float(fx['train_loss'])))
    idx = {n: i for i, n in enumerate(fx['param_names'].tolist())}
    assert int(fx['param_has_grad'].sum()) == len(train_keys)
    assert not fx['param_has_grad'][idx['encoders.encoder.last_linear.weight']]
    checked = 0
    for k in train_keys:
        i = idx[k]
        assert bool(fx['param_has_grad'][i]), k
        if fx['grad_norm'][i] <= 1e-4:            # a convolution bias in front of a train-mode BatchNorm: analytically zero
            assert k.endswith('conv.bias'), k
            continue
        gn = float(sd[k].grad.double().norm())
        assert abs(gn - fx['grad_norm'][i]) <= 2e-3 * fx['grad_norm'][i], (k, gn, fx['grad_norm'][i])
        checked += 1
    assert checked == len(train_keys) - 13          # center (2), five decoder blocks (2 each), final.0
    for k in fx:
        if k.startswith('fullgrad:'):
            assert_close(sd[k[9:]].grad, fx[k], 2e-3, k)
    for k, s in zip(fx['bn_keys'].tolist(), fx['bn_sum'].tolist()):
        assert abs(float(sd[k].double().sum()) - s) <= 1e-4 * max(1.0, abs(s)), k


def test_fixture_guards_are_the_references_own_error():
    fx = golden('F17_unet_seresnet50_hyper')
    assert 0 < float(fx['ref_f32_vs_f64_maxabs']) < 1e-3 * float(np.abs(fx['eval_logits']).max()) / 10
    assert 0 < float(fx['ref_f32_vs_f64_gradnorm_rel']) <= 2.5e-3             # a quarter of the GPU test's 1e-2 (tensors of 16 elements and more)
    # tensors under 16 elements (the one-element spatial-SE biases): a quarter of the GPU test's 1e-6 of the largest gradient norm
    assert 0 < float(fx['ref_f32_vs_f64_small_abs']) <= 2.5e-7
    small = [k for k, h, n in zip(fx['param_names'].tolist(), fx['param_has_grad'], fx['grad_norm']) if h and n > 1e-4 and k.endswith('spatial_se.fc.bias')]
    assert len(small) == 5
    assert 0 < float(fx['ref_bf16_storage_vs_f32_maxabs']) < float(np.abs(fx['eval_logits']).max())
    assert min(fx['gate_frac_mid_eval'].tolist() + fx['gate_frac_mid_train'].tolist()) >= 0.5


# ------------------------------------------------------------------------------------------------ host surface
def test_registry_entry_is_the_references():
    from salt_amd import architectures as A, models
    assert models.ARCHITECTURES['UNetSeResNet'] == {
        'model': A.UNetSeResNet,
        'model_config': {'encoder_depth': 50, 'use_hypercolumn': True, 'dropout_2d': 0.0, 'pretrained': False, 'pool0': False},
        'init_weights': False}


@pytest.mark.parametrize('depth', [50, 101, 152])
def test_state_dict_layout_matches_the_stub(depth):
    from salt_amd import architectures as A
    net = A.UNetSeResNet(depth, 2, use_hypercolumn=True)
    sd = net.state_dict()
    spec = SO.spec_unet_seresnet(depth, with_last_linear=True)
    if depth in (50, 101):
        fx = golden('F17_unet_seresnet%d_hyper' % depth)
        assert list(sd.keys()) == fx['keys'].tolist()
        assert ['x'.join(str(d) for d in v.shape) for v in sd.values()] == fx['key_shapes'].tolist()
    # the canonical spellings come first and in the spec's order; every alias shares its tensor
    canon = [k for k in sd if k in spec]
    assert canon == list(spec) and all(tuple(sd[k].shape) == spec[k][0] for k in spec)
    assert set(sd) == set(SO.expand_aliases({k: None for k in spec}))
    for a, c in SO.ALIASES.items():
        k = next(k for k in spec if k.startswith(c))
        assert sd[a + k[len(c):]].data_ptr() == sd[k].data_ptr()
    blk = net.encoders.encoder.layer2[0]
    assert blk.conv1.stride == (2, 2) and blk.conv2.stride == (1, 1) and blk.downsample[0].stride == (2, 2)      # the 1x1 carries the stride
    assert tuple(sd['encoders.encoder.layer4.2.se_module.fc1.weight'].shape) == (128, 2048, 1, 1)
    assert net.dead_parameter_names() == ['encoders.encoder.last_linear.weight', 'encoders.encoder.last_linear.bias']
    assert net.output_shape((4, 3, 128, 128)) == (4, 2, 128, 128) and not net.uses_depth


def test_error_paths():
    from salt_amd import architectures as A
    from salt_amd._abi import SaltError
    with pytest.raises(NotImplementedError, match='only 50, 101, 152 version of Resnet are implemented'):
        A.UNetSeResNet(34, 2)
    with pytest.raises(SaltError, match='download'):
        A.UNetSeResNet(50, 2, pretrained='imagenet')
    with pytest.raises(SaltError, match='pool0'):
        A.UNetSeResNet(50, 2, pool0=True)
    with pytest.raises(SaltError, match='grouped'):
        A.SEResNetBottleneck(64, 64, 32, 16)
    net = A.UNetSeResNet(50, 2)
    with pytest.raises(SaltError):
        net(torch.zeros(1, 3, 64, 64))                    # CPU tensor: no fallback
    with pytest.raises(SaltError):
        net.encoders.encoder.layer1[0](torch.zeros(1, 64, 8, 8))
    assert net.set_compute_dtype('bf16').compute_dtype == 'bf16' and net.set_align_corners(True).align_corners is True


def test_segmentation_model_construction():
    from salt_amd import architectures as A, models
    arch = {'model_params': {'architecture': 'UNetSeResNet', 'out_channels': 2, 'activation': 'sigmoid', 'loss': 'lovasz', 'compute_dtype': 'bf16'},
            'optimizer_params': {'lr': 1e-4}, 'regularizer_params': {'regularize': True, 'weight_decay_conv2d': 1e-4}}
    m = models.SegmentationModel(arch, {'epochs': 1}, {})
    assert isinstance(m.model, A.UNetSeResNet) and m.model.compute_dtype == 'bf16' and m.model.use_hypercolumn
    ids = {id(p) for g in m.optimizer.param_groups for p in g['params']}
    fc = m.model.encoders.encoder.layer3[2].se_module
    assert all(id(p) in ids for p in (fc.fc1.weight, fc.fc1.bias, fc.fc2.weight, fc.fc2.bias))


def test_new_symbols_are_in_the_header_and_the_library():
    from salt_amd import _abi as abi
    with open(abi.HEADER) as f:
        header = f.read()
    out = subprocess.run(['nm', '-D', '--defined-only', abi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r'\b(salt_\w+)$', out, flags=re.M))
    for s in NEW_SYMBOLS:
        assert re.search(r'^int %s\(' % s, header, flags=re.M), s
        assert s in abi.DECLARED_SYMBOLS and s in exported, s
    assert abi.lib.salt_abi_version() >= 28
    assert 'salt_se_res_args' in abi.STRUCTS and 'salt_se_res_bwd_args' in abi.STRUCTS
    # the host-side shape rules answer without a GPU
    import ctypes
    from salt_amd.engine import shaped_view
    probe = lambda C, dt=0: abi.lib.salt_se_res_parts(ctypes.byref(abi.fill(abi.STRUCTS['salt_se_res_args'](), dtype=dt, x=shaped_view(1 << 20, 2, 40, 40, C))))
    assert probe(256) == 7 and probe(2048, 1) == 7 and probe(96) == abi.CONSTS['SALT_E_UNSUPPORTED'] and probe(4096) == abi.CONSTS['SALT_E_UNSUPPORTED']
