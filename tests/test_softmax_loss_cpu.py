"""The softmax head without a GPU: model_params['activation'] = 'softmax' constructs with both losses, and the float64 references of
tests/softmax_loss_reference.py (which the GPU tests compare the kernels with) agree with float64 torch autograd."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import softmax_loss_reference as SR

F64 = torch.float64


def _arch(architecture, **extra):
    return {'model_params': dict({'architecture': architecture, 'out_channels': 2, 'activation': 'softmax', 'compute_dtype': 'f32'}, **extra),
            'optimizer_params': {'lr': 1e-4}, 'regularizer_params': {'regularize': True, 'weight_decay_conv2d': 1e-4}}


# ------------------------------------------------------------------------------------------------ the public surface
@pytest.mark.parametrize('kind', ['lovasz_softmax', 'dice_ce'])
@pytest.mark.parametrize('with_depth', [False, True])
def test_softmax_models_construct_with_a_native_loss(with_depth, kind):
    from salt_amd import models, losses
    cls = models.SegmentationModelWithDepth if with_depth else models.SegmentationModel
    m = cls(_arch('UNetResNetWithDepth' if with_depth else 'UNetResNet', loss=kind), {'epochs': 1}, {})
    (name, fn, weight), = m.loss_function
    assert (name, weight) == ('mask', 1.0) and fn.native_kind == kind
    assert fn is {'lovasz_softmax': losses.lovasz_softmax_loss, 'dice_ce': losses.mixed_dice_cross_entropy_loss}[kind]
    assert m.activation_func == 'softmax' and m.loss_params is None


def test_softmax_loss_choices_and_parameters():
    from salt_amd import models, losses
    from salt_amd._abi import SaltError
    m = models.SegmentationModel(_arch('UNetResNet', loss='dice_ce', loss_params={'dice_weight': 0.2, 'smooth': 1}), {'epochs': 1}, {})
    assert m.loss_function[0][1].native_kind == 'dice_ce' and m.loss_params == {'dice_weight': 0.2, 'smooth': 1}
    assert losses.dice_ce_params(m.loss_params) == (0.2, 0.5, 1.0) and losses.dice_ce_params(None) == (0.5, 0.5, 0.0)
    with pytest.raises(SaltError):
        models.SegmentationModel(_arch('UNetResNet', loss='lovasz'), {'epochs': 1}, {})                 # a sigmoid loss
    with pytest.raises(SaltError):
        models.SegmentationModel(_arch('UNetResNet', loss='dice_ce', loss_params={'bce_weight': 1.0}), {'epochs': 1}, {})
    with pytest.raises(SaltError):
        models.SegmentationModel(_arch('UNetResNet', loss='dice_ce', out_channels=1), {'epochs': 1}, {})
    with pytest.raises(NotImplementedError, match='lovasz_softmax . dice_ce'):                          # no loss is chosen on the user's behalf
        models.SegmentationModel(_arch('UNetResNet'), {'epochs': 1}, {})
    # the sigmoid surface is what it was
    s = models.SegmentationModel(_arch('UNetResNet', activation='sigmoid'), {'epochs': 1}, {})
    assert s.loss_function[0][1] is losses.lovasz_loss
    for kw in ({'dice_activation': 'sigmoid'}, {'dice_loss': F.mse_loss}, {'cross_entropy_loss': F.mse_loss}):
        with pytest.raises(NotImplementedError):
            losses.mixed_dice_cross_entropy_loss(torch.zeros(1, 2, 2, 2), torch.zeros(1, 2, 2, 2), **kw)


def test_a_classifier_with_softmax_is_refused():
    from salt_amd import models
    from salt_amd._abi import SaltError
    with pytest.raises(SaltError, match='sigmoid-only'):
        models.SegmentationModel(_arch('EmptinessClassifier'), {'epochs': 1}, {})


def test_new_symbols_are_declared_and_exported():
    from salt_amd import _abi as abi
    for s in ('salt_softmax', 'salt_softmax_bwd', 'salt_lovasz_softmax', 'salt_dice_ce', 'salt_dice_ce_parts'):
        assert s in abi.DECLARED_SYMBOLS and hasattr(abi.lib, s), s
    assert abi.lib.salt_abi_version() >= 34
    assert [f for f, _ in abi.STRUCTS['salt_tta_mean_args']._fields_][-2:] == ['method', 'activation']      # a zeroed tail is today's sigmoid


# ------------------------------------------------------------------------------------------------ references vs autograd
@pytest.mark.parametrize('shape', [(1, 2, 1), (2, 3, 37), (3, 4, 130)])
def test_softmax_reference_vs_autograd(shape):
    g = SR.gen('softmax', shape)
    z = (torch.randn(shape, generator=g, dtype=F64) * 3).requires_grad_(True)
    dp = torch.randn(shape, generator=g, dtype=F64)
    p = F.softmax(z, 1)
    p.backward(dp)
    assert float((SR.softmax(z.detach()) - p.detach()).abs().max()) <= 1e-15
    assert float((SR.softmax_bwd(p.detach(), dp) - z.grad).abs().max()) <= 1e-15
    big = SR.softmax(SR.large_logits(shape, g))
    assert bool(torch.isfinite(big).all()) and float((big.sum(1) - 1).abs().max()) <= 1e-15


@pytest.mark.parametrize('kind', ['random', 'background'])
@pytest.mark.parametrize('params', [(0.5, 0.5, 0.0, 1.0), (0.2, 0.9, 1.0, 0.25)])
@pytest.mark.parametrize('shape', [(1, 2, 1), (2, 2, 61), (3, 3, 200), (1, 4, 97)])
def test_dice_ce_reference_vs_cross_entropy_and_dice_through_autograd(shape, params, kind):
    g = SR.gen('dice_ce cpu', shape, kind)
    z = (torch.randn(shape, generator=g, dtype=F64) * 3).requires_grad_(True)
    t = SR.random_target(shape, g, kind)
    auto = SR.dice_ce_autograd(z, t, *params)
    auto.backward()
    loss, dz, sums = SR.dice_ce(z.detach(), t, *params)
    assert abs(loss - float(auto.detach())) <= 1e-13 * max(1.0, abs(loss))
    assert float((dz - z.grad).abs().max()) <= 1e-13 * max(float(z.grad.abs().max()), 1e-30)
    p = F.softmax(z.detach(), 1)
    assert torch.allclose(sums[:-1].reshape(-1, 3)[:, 1], p.sum((0, 2)), rtol=1e-13, atol=0)


def test_stable_order_keeps_ascending_indices_in_ties():
    e = torch.tensor([0.5, 1.0, 0.5, 0.0, 1.0, 0.5], dtype=F64)
    assert SR.stable_order(e).tolist() == [1, 4, 0, 2, 5, 3]
    assert SR.stable_order(e).tolist() == np.argsort(-e.numpy(), kind='stable').tolist()


@pytest.mark.parametrize('shape', [(1, 2, 1), (2, 2, 50), (2, 3, 333)])
def test_lovasz_softmax_closed_form_vs_autograd_without_ties(shape):
    g = SR.gen('lovasz_softmax cpu', shape)
    p = torch.rand(shape, generator=g, dtype=F64).requires_grad_(True)             # distinct values: no ties, no zero error
    t = SR.random_target(shape, g)
    t[0] = 0
    t[0, 0] = 1                                                                    # image 0 is all background
    assert SR.tie_groups(p.detach(), t) == (0, 0)
    auto = SR.lovasz_softmax_autograd(p, t, 0.5)
    auto.backward()
    loss, grad, rows = SR.lovasz_softmax(p.detach(), t, 0.5)
    assert abs(loss - float(auto.detach())) <= 1e-14 and abs(float(rows.mean()) * 0.5 - loss) <= 1e-15
    assert float((grad - p.grad).abs().max()) <= 1e-15


def test_lovasz_softmax_gradient_follows_the_stable_order_at_ties_and_is_zero_at_zero_error():
    # one row of class 1 (foreground): errors [.5, .5, 0, .5, 1]; the three tied elements keep their index order 0, 1, 3
    p = torch.tensor([[[0.5, 0.5, 1.0, 0.5, 0.0], [0.5, 0.5, 0.0, 0.5, 1.0]]], dtype=F64)
    t = torch.tensor([[[1.0, 0.0, 0.0, 1.0, 1.0], [0.0, 1.0, 1.0, 0.0, 0.0]]], dtype=F64)
    loss, grad, rows = SR.lovasz_softmax(p, t)
    # row (0, 1): fg = [0, 1, 1, 0, 0], e = [.5, .5, 1, .5, 1] -> stable order 2, 4, 0, 1, 3 with labels 1, 0, 0, 1, 0
    order = [2, 4, 0, 1, 3]
    gk = SR.jaccard_gradient(torch.tensor([1.0, 0.0, 0.0, 1.0, 0.0], dtype=F64))
    want = torch.zeros(5, dtype=F64)
    for k, i in enumerate(order):
        want[i] = (-1.0 if t[0, 1, i] > 0.5 else 1.0) * gk[k] / 2
    assert torch.equal(grad[0, 1], want)
    # swapping the tied elements 0 and 1 would move gradient between them: the order is observable
    assert abs(float(gk[2]) - float(gk[3])) > 0.1
    # row (0, 0): fg = [1, 0, 0, 1, 1], e = [.5, .5, 1, .5, 1]; make one error exactly 0 and its gradient vanishes
    p0 = p.clone()
    p0[0, 0, 0] = 1.0
    _, grad0, _ = SR.lovasz_softmax(p0, t)
    assert float(grad0[0, 0, 0]) == 0.0 and float(grad[0, 0, 0]) != 0.0
    # autograd (torch's abs backward is 0 at 0) agrees on the zero
    q = p0.clone().requires_grad_(True)
    SR.lovasz_softmax_autograd(q, t).backward()
    assert float(q.grad[0, 0, 0]) == 0.0 and float((q.grad - grad0).abs().max()) <= 1e-15


@pytest.mark.parametrize('C', SR.LOVASZ_C)
@pytest.mark.parametrize('HW', SR.LOVASZ_HW)
def test_dyadic_lovasz_cases_hold_ties_a_zero_error_and_an_empty_foreground(HW, C):
    p, t = SR.lovasz_case(C, HW)
    assert p.shape == t.shape == (SR.LOVASZ_B, C, HW)
    assert torch.equal(p * 32, torch.round(p * 32)) and float(p.min()) >= 0 and float(p.max()) <= 1
    assert torch.equal(p.float().double(), p) and torch.equal(t.sum(1), torch.ones(SR.LOVASZ_B, HW, dtype=F64))
    e32 = ((t > 0.5).float() - p.float()).abs()
    assert torch.equal(e32.double(), ((t > 0.5).double() - p).abs())                       # every error is exact in fp32
    assert float(t[0, 1:].sum()) == 0                                                      # an all-zero foreground channel
    rows, zeros = SR.tie_groups(p, t)
    assert zeros >= 1
    assert rows >= 1 if HW >= 2 else rows == 0                                             # a row of one element cannot tie
