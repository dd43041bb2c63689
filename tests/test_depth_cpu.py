"""CPU tests of the depth-conditioned network: the comparator tests/depth_oracle.py against the F14 fixtures the reference produced,
and the host surface (state_dict layout, registry, trainer construction) that needs no GPU."""
import numpy as np
import pytest
import torch

from helpers import golden, T, assert_close
import closed_form as CF
import depth_oracle as DO
from oracle import losses as OL, specs as OS


@pytest.mark.parametrize('train', [True, False])
def test_depth_gate_block_matches_reference(train):
    fx = golden('F14_depth_channel_excitation_' + ('train' if train else 'eval'))
    sd = {'fc.0.weight': CF.tensor_for('fc.0.weight', fx['s:fc.0.weight'].shape).requires_grad_(True),
          'fc.0.bias': CF.tensor_for('fc.0.bias', fx['s:fc.0.bias'].shape).requires_grad_(True)}
    x = T(fx['x']).requires_grad_(True)
    y = x * DO.depth_gate(sd, T(fx['d']), '')[:, :, None, None]
    assert_close(y, fx['y'], 2e-5, 'y')
    y.backward(T(fx['gy']))
    assert_close(x.grad, fx['gx'], 2e-5, 'gx')
    assert_close(sd['fc.0.weight'].grad, fx['g:fc.0.weight'], 2e-5, 'dw')
    assert_close(sd['fc.0.bias'].grad, fx['g:fc.0.bias'], 2e-5, 'db')


@pytest.mark.parametrize('tag,hyper', [('hyper', True), ('nohyper', False)])
def test_depth_oracle_reproduces_reference_network(tag, hyper):
    """Same checks and tolerances as tests/test_oracle_golden.py applies to the F8 networks."""
    fx = golden('F14_unet_resnet34_depth_' + tag)
    spec = DO.spec_unet_resnet_with_depth(34, use_hypercolumn=hyper, with_fc=True)
    assert set(OS.expand_aliases('UNetResNet', {k: None for k in spec})) == set(fx['keys'].tolist())
    sd = CF.state_for((k, s) for k, (s, _) in spec.items())
    x, d, t = T(fx['x']), T(fx['d']), T(fx['t'])
    with torch.no_grad():
        logits = DO.unet_resnet_with_depth(sd, x, d, False, use_hypercolumn=hyper)
    assert_close(logits, fx['eval_logits'], 1e-4, 'eval logits')
    assert np.array_equal((logits[:, 1] > 0).numpy().astype(np.uint8), fx['eval_mask'])
    train_keys = OS.trainable_keys(spec)
    assert 'depth_channel_excitation.fc.0.weight' in train_keys and 'depth_channel_excitation.fc.0.bias' in train_keys
    for k in train_keys:
        sd[k].requires_grad_(True)
    out = DO.unet_resnet_with_depth(sd, x, d, True, use_hypercolumn=hyper)
    loss = OL.lovasz_loss(out, t)
    loss.backward()
    assert abs(float(loss) - float(fx['train_loss'])) < 1e-4 * max(1.0, abs(float(fx['train_loss'])))
    idx = {n: i for i, n in enumerate(fx['param_names'].tolist())}
    checked = 0
    for k in train_keys:
        i = idx[k]
        has = bool(fx['param_has_grad'][i])
        assert (sd[k].grad is not None) == has, k
        if has and fx['grad_norm'][i] > 1e-4:
            gn = float(sd[k].grad.double().norm())
            assert abs(gn - fx['grad_norm'][i]) <= 2e-3 * fx['grad_norm'][i], (k, gn, fx['grad_norm'][i])
            checked += 1
    assert checked > 20
    full = [k for k in fx if k.startswith('fullgrad:')]
    assert 'fullgrad:depth_channel_excitation.fc.0.weight' in full and 'fullgrad:depth_channel_excitation.fc.0.bias' in full
    for k in full:
        assert_close(sd[k[9:]].grad, fx[k], 2e-3, k)
    params = [sd[k] for k in train_keys]
    with torch.no_grad():
        ps = [p.detach() for p in params]
        OL.adam_l2_step(ps, [p.grad for p in params], [torch.zeros_like(p) for p in ps], [torch.zeros_like(p) for p in ps], 1)
    for k, p in zip(train_keys, params):
        i = idx[k]
        if fx['param_has_grad'][i] and fx['grad_norm'][i] > 1e-4:
            assert abs(float(p.detach().double().norm()) - fx['post_norm'][i]) <= 1e-5 * max(fx['post_norm'][i], 1e-3), k
    for k, s in zip(fx['bn_keys'].tolist(), fx['bn_sum'].tolist()):
        assert abs(float(sd[k].double().sum()) - s) <= 1e-4 * max(1.0, abs(s)), k


def test_fixture_guard_is_the_references_own_error():
    """The mask guard of the GPU test is 4 x the fp32 reference's distance from float64; with D = [[0.2], [0.6]] no pixel sits under it."""
    for tag in ('hyper', 'nohyper'):
        fx = golden('F14_unet_resnet34_depth_' + tag)
        assert fx['d'].tolist() == [[np.float32(0.2)], [np.float32(0.6)]]
        guard = 4 * float(fx['ref_f32_vs_f64_maxabs'])
        assert 0 < guard < 5e-3 and int((np.abs(fx['eval_logits'][:, 1]) <= guard).sum()) == 0
        assert int(fx['ref_f32_mask_flips_vs_f64']) == 0


def _arch(loss='lovasz'):
    return {'model_params': {'architecture': 'UNetResNetWithDepth', 'out_channels': 2, 'activation': 'sigmoid', 'loss': loss},
            'optimizer_params': {'lr': 1e-4}, 'regularizer_params': {'regularize': True, 'weight_decay_conv2d': 1e-4}}


@pytest.mark.parametrize('tag,hyper', [('hyper', True), ('nohyper', False)])
def test_state_dict_layout_matches_reference(tag, hyper):
    from salt_amd import architectures as A
    fx = golden('F14_unet_resnet34_depth_' + tag)
    net = A.UNetResNetWithDepth(34, 2, use_hypercolumn=hyper)
    sd = net.state_dict()
    assert list(sd.keys()) == fx['keys'].tolist()
    assert tuple(sd['depth_channel_excitation.fc.0.weight'].shape) == ((320 if hyper else 64), 1)
    assert [k for k in sd if k.startswith('depth_')] == list(sd.keys())[-2:]
    assert not hasattr(net.encoders, 'pool0') or net.encoders.pool0 is False


def test_segmentation_model_with_depth_constructs_without_gpu():
    from salt_amd import architectures as A, models
    from salt_amd._abi import SaltError
    assert models.ARCHITECTURES['UNetResNetWithDepth']['model_config'] == {'encoder_depth': 34, 'use_hypercolumn': True, 'dropout_2d': 0.0,
                                                                          'pretrained': False}
    m = models.SegmentationModelWithDepth(_arch(), {'epochs': 1}, {'validation_monitor': {'epoch_every': 1, 'use_depth': True}})
    assert isinstance(m.model, A.UNetResNetWithDepth) and m.model.uses_depth
    assert list(m.model.state_dict().keys()) == golden('F14_unet_resnet34_depth_hyper')['keys'].tolist()
    group = m.optimizer.param_groups[0]
    ids = {id(p) for p in group['params']}
    fc = m.model.depth_channel_excitation.fc[0]
    assert id(fc.weight) in ids and id(fc.bias) in ids and group['weight_decay'] == 1e-4
    bad = _arch()
    bad['model_params']['architecture'] = 'UNetResNet'
    with pytest.raises(SaltError):
        models.SegmentationModelWithDepth(bad, {'epochs': 1}, {})
    # the callback's use_depth must agree with the network
    from salt_amd import callbacks as C
    with pytest.raises(SaltError):
        C.ValidationMonitor(use_depth=False).set_params(m, validation_datagen=None)
    C.ValidationMonitor(use_depth=True).set_params(m, validation_datagen=None)


def test_depth_networks_need_a_gpu_and_a_depth():
    from salt_amd import architectures as A
    from salt_amd._abi import SaltError
    net = A.UNetResNetWithDepth(18, 2)
    with pytest.raises(SaltError):
        net(torch.zeros(1, 3, 64, 64), torch.zeros(1, 1))            # CPU tensor: no fallback
    for depth in (18, 34, 50, 101, 152):
        n = A.UNetResNetWithDepth(depth, 2, use_hypercolumn=True)
        b = 512 if depth in (18, 34) else 2048
        assert n.depth_channel_excitation.fc[0].weight.shape == (5 * b // 8, 1)
    with pytest.raises(NotImplementedError):
        A.UNetResNetWithDepth(20, 2)
    with pytest.raises(SaltError):
        A.UNetResNet(34, 2)._check_depth(torch.zeros(2, 3, 64, 64), torch.zeros(2, 1))
    with pytest.raises(SaltError):
        net._check_depth(torch.zeros(2, 3, 64, 64), None)
    with pytest.raises(SaltError):
        net._check_depth(torch.zeros(2, 3, 64, 64), torch.zeros(2))
