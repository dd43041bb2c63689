"""CPU tests of the second-level (stacking) networks: the comparator tests/stacking_oracle.py and the float64 operator reference
tests/stacking_op_reference.py against the F16 fixtures the reference's own misc.StackingFCN / misc.StackingFCNWithDepth produced, and
the host surface (state_dict layout, registry, trainer pairing, shape limits) - nothing here touches a GPU."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import golden, T, assert_close
import closed_form as CF
import stacking_oracle as SO
import stacking_op_reference as SR

FIXTURES = [('F16_stacking_fcn', 5, False), ('F16_stacking_fcn_depth', 5, True), ('F16_stacking_fcn_m32', 32, False)]


def closed_form_state(fx):
    """the state the generator loaded into the reference module: closed-form by state-dict key"""
    shapes = {'conv.0.batch_norm.num_batches_tracked': ()}
    for k in fx:
        if k.startswith('post:'):
            shapes[k[5:]] = fx[k].shape
        if k.startswith('bn:'):
            shapes[k[3:]] = fx[k].shape
    return {k: CF.tensor_for(k, shapes[k]) for k in fx['keys'].tolist()}


def fixture_inputs(fx):
    return T(fx['x']), (T(fx['d']) if 'd' in fx else None), T(fx['t'])


# ------------------------------------------------------------------------------------------------ fixtures vs comparators
@pytest.mark.parametrize('name,M,with_depth', FIXTURES)
def test_fixture_records_the_references_own_error(name, M, with_depth):
    fx = golden(name)
    assert fx['x'].shape[1] == M and fx['eval_logits'].shape == (2, 2) + fx['x'].shape[2:]
    assert 0 < float(fx['ref_f32_vs_f64_maxabs']) < 1e-5
    assert 0 < float(fx['ref_f32_vs_f64_gradnorm_rel']) < 2.5e-3
    assert 1e-4 < float(fx['ref_bf16_storage_vs_f32_maxabs']) < 5e-2
    thr = 1e-3 * float(np.abs(fx['eval_logits']).max())
    assert abs(float(fx['near_zero_thr']) - thr) <= 1e-6 * thr
    share = float((np.abs(fx['eval_logits'][:, 1]) < thr).mean())
    assert share == pytest.approx(float(fx['near_zero_share'])) and share <= 1e-3
    assert fx['zero_grad_names'].tolist() == ['conv.0.conv.bias']
    assert fx['keys'].tolist() == SO.state_keys(with_depth)


@pytest.mark.parametrize('name,M,with_depth', FIXTURES)
def test_oracle_reproduces_reference_network(name, M, with_depth):
    """eval logits 1e-4; one training step: loss, every gradient 2e-5 relative, post-Adam parameters, running statistics"""
    fx = golden(name)
    sd = closed_form_state(fx)
    x, d, t = fixture_inputs(fx)
    with torch.no_grad():
        logits = SO.stacking_fcn(sd, x, False, d=d)
    assert_close(logits, fx['eval_logits'], 1e-4, 'eval logits')
    assert np.array_equal((logits[:, 1] > 0).numpy(), fx['eval_logits'][:, 1] > 0)
    names = fx['param_names'].tolist()
    params = {k: sd[k].clone().requires_grad_(True) for k in names}
    live = dict(sd, **params)
    out = SO.stacking_fcn(live, x, True, d=d)
    assert_close(out, fx['train_logits'], 1e-4, 'train logits')
    loss = SO.lovasz_loss(out, t)
    assert abs(float(loss.detach()) - float(fx['train_loss'])) <= 2e-5 * abs(float(fx['train_loss']))
    loss.backward()
    gmax = max(float(np.abs(fx['fullgrad:' + k]).max()) for k in names)
    for k in names:
        if k in fx['zero_grad_names'].tolist():
            assert float(params[k].grad.abs().max()) <= 1e-5 * gmax, k          # exactly zero in exact arithmetic
        else:
            assert_close(params[k].grad, fx['fullgrad:' + k], 2e-5, 'grad ' + k)
    opt = torch.optim.Adam([{'params': list(params.values()), 'weight_decay': 1e-4}], lr=1e-4)
    opt.step()
    for k in names:
        assert_close(params[k], fx['post:' + k], 1e-5, 'post ' + k)
    for k in ('running_mean', 'running_var'):
        assert_close(live['conv.0.batch_norm.' + k], fx['bn:conv.0.batch_norm.' + k], 1e-5, k)


@pytest.mark.parametrize('name,M,with_depth', FIXTURES)
def test_op_reference_reproduces_reference_network(name, M, with_depth):
    """The float64 operator reference composed into the network: eval logits, the training-mode statistics (through the running
    statistics the reference module left behind), the training logits and the weight gradient from the reference's own dL/dy
    ('train_dy'), all to 2e-6.  dL/dy recomputed in float64 differs from the reference's fp32 one by up to 3e-5 of its maximum (the
    BatchNorm backward cancels), so the operator is checked on the gradient the reference itself contracted; and torch's fp32
    contraction of it is off by 'ref_wgrad_f32_vs_f64_maxrel' (8e-6) itself, so the 2e-6 is against the reference's modules run in
    float64 ('wgrad_f64_from_train_dy') and the fp32 gradient is met within 2e-6 plus that recorded error."""
    fx = golden(name)
    sd = closed_form_state(fx)
    x, d, t = fixture_inputs(fx)
    p = 'conv.0.batch_norm.'
    y = SR.conv(x, sd['conv.0.conv.weight'], sd['conv.0.conv.bias'])
    scale, shift = SR.bn_fold(sd[p + 'weight'], sd[p + 'bias'], sd[p + 'running_mean'], sd[p + 'running_var'])
    gate = SO.depth_gate({k: v.double() for k, v in sd.items() if k.startswith('depth_')}, d.double()) if with_depth else None
    logits = SR.eval_head(y, scale, shift, True, gate, sd['final.0.weight'], sd['final.0.bias'])
    assert_close(logits.float(), fx['eval_logits'], 2e-6, 'op reference eval logits')
    mean, var, unb = SR.stats(y)
    assert_close((0.9 * sd[p + 'running_mean'].double() + 0.1 * mean).float(), fx['bn:' + p + 'running_mean'], 2e-6, 'running mean')
    assert_close((0.9 * sd[p + 'running_var'].double() + 0.1 * unb).float(), fx['bn:' + p + 'running_var'], 2e-6, 'running var')
    # training mode: the same head over the batch statistics
    sc, sh = SR.bn_fold(sd[p + 'weight'], sd[p + 'bias'], mean, var)
    out = SR.eval_head(y, sc, sh, True, gate, sd['final.0.weight'], sd['final.0.bias'])
    assert_close(out.float(), fx['train_logits'], 2e-6, 'op reference train logits')
    dy = T(fx['train_dy'])
    gw = SR.wgrad(dy, x)
    assert fx['wgrad_f64_from_train_dy'].dtype == np.float64
    assert_close(gw.numpy(), fx['wgrad_f64_from_train_dy'], 2e-6, 'op reference weight gradient')
    own = float(fx['ref_wgrad_f32_vs_f64_maxrel'])
    assert 0 < own < 5e-5
    assert_close(gw.numpy(), fx['fullgrad:conv.0.conv.weight'], 2e-6 + own, 'op reference weight gradient vs the fp32 module')
    Mpad = (M + 15) // 16 * 16
    gp = SR.wgrad(dy, x, Mpad)
    assert gp.shape == (32, Mpad, 3, 3) and torch.equal(gp[:, :M], gw) and bool((gp[:, M:] == 0).all())
    xs = SR.xs_nhwc(x, Mpad)
    assert torch.equal(xs[..., :M], x.double().permute(0, 2, 3, 1)) and bool((xs[..., M:] == 0).all())


def test_op_reference_taps_are_not_symmetric():
    """a kh/kw swap or a row/column swap of the reference itself would pass a symmetric test: one hot tap at a time against F.conv2d"""
    x = torch.arange(2 * 3 * 5 * 7, dtype=torch.float64).reshape(2, 3, 5, 7)
    for kh in range(3):
        for kw in range(3):
            w = torch.zeros(4, 3, 3, 3, dtype=torch.float64)
            w[:, :, kh, kw] = torch.arange(12, dtype=torch.float64).reshape(4, 3) + 1
            ref = F.conv2d(F.pad(x, (0, 2, 2, 0), mode='replicate'), w)
            assert torch.equal(SR.conv(x, w), ref), (kh, kw)


# ------------------------------------------------------------------------------------------------ host surface
@pytest.mark.parametrize('name,M,with_depth', FIXTURES)
def test_state_dict_layout_matches_reference(name, M, with_depth):
    from salt_amd import architectures as A
    fx = golden(name)
    net = (A.StackingFCNWithDepth if with_depth else A.StackingFCN)(M, 2, filter_nr=32, dropout_2d=0.0)
    sd = net.state_dict()
    assert list(sd.keys()) == fx['keys'].tolist()
    assert [k for k, _ in net.named_parameters()] == fx['param_names'].tolist()
    for k in fx['param_names'].tolist():
        assert tuple(sd[k].shape) == fx['post:' + k].shape, k
    assert net.uses_depth == with_depth and net.dead_parameter_names() == []
    assert net.output_shape((4, M, 19, 37)) == (4, 2, 19, 37)


def test_registry_entries_are_the_references():
    from salt_amd import architectures as A, models
    cfg = {'input_model_nr': 32, 'filter_nr': 32, 'dropout_2d': 0.0}
    assert models.ARCHITECTURES['StackingFCN'] == {'model': A.StackingFCN, 'model_config': cfg, 'init_weights': True}
    assert models.ARCHITECTURES['StackingFCNWithDepth'] == {'model': A.StackingFCNWithDepth, 'model_config': cfg, 'init_weights': True}


def _arch(name, **extra):
    return {'model_params': dict({'architecture': name, 'out_channels': 2, 'activation': 'sigmoid', 'loss': 'lovasz'}, **extra),
            'optimizer_params': {'lr': 1e-4}, 'regularizer_params': {'regularize': True, 'weight_decay_conv2d': 1e-4}}


def test_trainers_pair_with_their_networks_and_take_overrides():
    from salt_amd import architectures as A, models
    from salt_amd._abi import SaltError
    m = models.SegmentationModel(_arch('StackingFCN'), {'epochs': 1}, {})
    assert isinstance(m.model, A.StackingFCN) and tuple(m.model.conv[0].conv.weight.shape) == (32, 32, 3, 3)
    ids = {id(p) for p in m.optimizer.param_groups[0]['params']}
    assert all(id(p) in ids for p in m.model.parameters())
    md = models.SegmentationModelWithDepth(_arch('StackingFCNWithDepth', input_model_nr=5, filter_nr=16), {'epochs': 1}, {})
    assert isinstance(md.model, A.StackingFCNWithDepth) and tuple(md.model.conv[0].conv.weight.shape) == (16, 5, 3, 3)
    assert tuple(md.model.depth_channel_excitation.fc[0].weight.shape) == (16, 1)
    assert models.ARCHITECTURES['StackingFCNWithDepth']['model_config']['input_model_nr'] == 32          # the registry itself is untouched
    with pytest.raises(SaltError):
        models.SegmentationModelWithDepth(_arch('StackingFCN'), {'epochs': 1}, {})
    with pytest.raises(SaltError):
        models.SegmentationModel(_arch('StackingFCNWithDepth'), {'epochs': 1}, {})
    # an override a network does not know is not forced on it
    u = models.SegmentationModel(_arch('VanillaUNet', input_model_nr=7), {'epochs': 1}, {})
    assert not hasattr(u.model, 'input_model_nr')


def test_unsupported_shapes_raise_from_host_side_checks():
    from salt_amd import architectures as A
    from salt_amd import engine as E
    from salt_amd._abi import SaltError, STRUCTS, check, fill, lib
    with pytest.raises(SaltError, match='65 input maps'):
        A.StackingFCN(65, 2)
    with pytest.raises(SaltError, match='48 filters'):
        A.StackingFCN(5, 2, filter_nr=48)
    with pytest.raises(SaltError):
        A.StackingFCN(5, 5)                                   # the fused head takes at most 4 classes
    assert E.stack_conv_parts(2, 5, 19, 37, 32) == 2 * 3 * 3          # 16 x 8 pixel tiles
    # the C entry point itself refuses before it looks at a pointer or the device
    for bad in (dict(M=65, F=32), dict(M=5, F=48), dict(M=0, F=32)):
        S = fill(STRUCTS['salt_stack_conv_args'](), dtype=0, B=1, H=8, W=8, x=16, w=16, K=2, **bad)
        with pytest.raises(SaltError, match='stack_conv'):
            check(lib.salt_stack_conv(ctypes.byref(S), None), 'stack_conv')
    net = A.StackingFCN(5, 2)
    with pytest.raises(SaltError, match='5 stacked maps'):
        net.output_shape((2, 6, 8, 8))
    with pytest.raises(SaltError):
        net(torch.zeros(1, 5, 8, 8))                          # CPU tensor: no fallback
