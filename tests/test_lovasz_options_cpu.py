"""CPU checks of the float64 closed forms of lovasz_options_reference.py (what the GPU tests of the Lovasz options compare against):
against the reference's own results for every option combination (F24_lovasz_options, tests/golden/make_golden_lovasz_options.py), the
batch-flat values of F6_lovasz, the known answer of the oracle's batch-flat hinge, and float64 autograd.  Also: the GPU case table
holds what its names claim, and lovasz_params refuses what it must."""
import itertools
import math

import pytest
import torch

import lovasz_options_reference as LR
from helpers import golden, T, assert_close
from oracle import losses as OL

F64 = torch.float64
COMBOS_HINGE = list(itertools.product((True, False), (False, True)))
COMBOS_SOFTMAX = list(itertools.product((False, True), (True, False), (False, True)))


def _onehot_with_void(y, C):
    """class labels [B,H,W] with 255 = void -> one-hot [B,C,HW] float64 with the void value in every plane"""
    B = y.shape[0]
    void = (y == 255).reshape(B, 1, -1)
    t = torch.stack([(y == c).to(F64) for c in range(C)], 1).reshape(B, C, -1)
    return torch.where(void, torch.full_like(t, LR.VOID), t)


@pytest.mark.parametrize('per_image,ig', COMBOS_HINGE)
def test_hinge_closed_form_matches_reference(per_image, ig):
    fx = golden('F24_lovasz_options')
    z = T(fx['hinge_z']).to(F64).reshape(3, -1)
    t = T(fx['hinge_t_void' if ig else 'hinge_t']).to(F64).reshape(3, -1)
    if ig:
        assert bool((t[0] == 255).all()) and 0 < int((t[1] == 255).sum()) < t[1].numel(), 'an all-void and a partly void image'
    loss, grad = LR.hinge(z, t, per_image, 255.0 if ig else None)
    tag = 'hinge_pi%d_ig%d' % (per_image, ig)
    ref = float(fx[tag + '_loss'])
    assert abs(loss - ref) <= 2e-6 * max(1.0, abs(ref)), (tag, loss, ref)
    assert_close(grad.float().reshape(fx[tag + '_grad'].shape), fx[tag + '_grad'], 1e-5, tag + ' grad')
    if ig:
        assert bool((grad[t == 255] == 0).all()) and bool((T(fx[tag + '_grad']).reshape(3, -1)[t == 255] == 0).all())


@pytest.mark.parametrize('only_present,per_image,ig', COMBOS_SOFTMAX)
def test_softmax_closed_form_matches_reference(only_present, per_image, ig):
    fx = golden('F24_lovasz_options')
    p = T(fx['softmax_p']).to(F64).reshape(3, 3, -1)
    y = T(fx['softmax_y_void' if ig else 'softmax_y'])
    assert not bool((y == 2).any()) and not bool((y[2] == 1).any()), 'class 2 absent from the batch, class 1 from image 2'
    t = _onehot_with_void(y, 3)
    loss, grad = LR.softmax(p, t, only_present, per_image, 255.0 if ig else None)
    tag = 'softmax_op%d_pi%d_ig%d' % (only_present, per_image, ig)
    ref = float(fx[tag + '_loss'])
    assert abs(loss - ref) <= 2e-6 * max(1.0, abs(ref)), (tag, loss, ref)
    assert_close(grad.float().reshape(fx[tag + '_grad'].shape), fx[tag + '_grad'], 1e-5, tag + ' grad')
    if only_present:
        assert bool((grad[:, 2] == 0).all()), 'the class absent from the batch is skipped'


@pytest.mark.parametrize('case', ['random', 'all0', 'all1', 'p1', 'ties', 'big'])
def test_hinge_batch_flat_matches_f6(case):
    fx = golden('F6_lovasz')
    z, t = T(fx[case + '_z']).to(F64), T(fx[case + '_t']).to(F64)
    B = z.shape[0]
    loss, _ = LR.hinge(z.reshape(B, -1), t.reshape(B, -1), per_image=False)
    ref = float(fx[case + '_loss_batch'])
    assert abs(loss - ref) <= 2e-6 * max(1.0, abs(ref)), (case, loss, ref)


def test_hinge_batch_flat_known_answer():
    logits = torch.linspace(-2, 2, 64).view(2, 2, 4, 4)
    labels = (torch.arange(64) % 3 == 0).float().view(2, 2, 4, 4)
    assert abs(float(OL.lovasz_hinge(logits, labels.long(), per_image=False)) - 1.70986664) < 2e-6
    loss, _ = LR.hinge(logits.to(F64).reshape(2, -1), labels.to(F64).reshape(2, -1), per_image=False)
    assert abs(loss - 1.70986664) < 2e-6
    l32, _ = LR.hinge(logits.to(F64).reshape(2, -1), labels.to(F64).reshape(2, -1), per_image=False, dtype=torch.float32)
    assert abs(l32 - 1.70986664) < 2e-6


def _tie_free(shape, g, lo=0.0, hi=1.0):
    n = math.prod(shape)
    return (lo + (hi - lo) * (torch.randperm(n, generator=g).to(F64) + 0.5) / n).reshape(shape)


@pytest.mark.parametrize('per_image,ig', COMBOS_HINGE)
def test_hinge_gradient_is_autograd(per_image, ig):
    g = LR.gen('hinge autograd', per_image, ig)
    z = _tie_free((3, 150), g, -3.0, 3.0).requires_grad_(True)
    t = LR.put_void(torch.randint(0, 2, (3, 150), generator=g).to(F64), 'some' if ig else None, g)
    ignore = LR.VOID if ig else None
    la = LR.hinge_autograd(z, t, per_image, ignore)
    la.backward()
    loss, grad = LR.hinge(z.detach(), t, per_image, ignore)
    assert abs(loss - float(la)) <= 1e-12 * max(1.0, abs(loss))
    assert float((grad - z.grad).abs().max()) <= 1e-12


@pytest.mark.parametrize('only_present,per_image,ig', COMBOS_SOFTMAX)
def test_softmax_gradient_is_autograd(only_present, per_image, ig):
    g = LR.gen('softmax autograd', only_present, per_image, ig)
    p = _tie_free((3, 3, 90), g).requires_grad_(True)
    _, t = LR.softmax_case(3, 3, 90, 'some' if ig else None, 'image')
    ignore = LR.VOID if ig else None
    la = LR.softmax_autograd(p, t, only_present, per_image, ignore)
    la.backward()
    loss, grad = LR.softmax(p.detach(), t, only_present, per_image, ignore)
    assert abs(loss - float(la)) <= 1e-12 * max(1.0, abs(loss))
    assert float((grad - p.grad).abs().max()) <= 1e-12


def test_gpu_cases_hold_what_their_names_claim():
    for N, B, P in LR.FLAT_SIZES:
        assert B * P == N
        z, t = LR.hinge_case(B, P)
        assert not bool((t == LR.VOID).any())
        assert bool((z * 2 == (z * 2).round()).all()) and float(z.abs().max()) <= 4
        if P >= 2:
            e = 1 - z * (2 * t - 1)
            assert LR.has_tie(e[-1]) and bool((e == 0).any()), 'a forced tie and a zero error'
        p, ts = LR.softmax_case(B, LR.SOFTMAX_C, P)
        assert bool((p * 32 == (p * 32).round()).all()) and bool((ts.sum(1) == 1).all())
    z, t = LR.hinge_case(2, 2049, 'some')
    frac = float((t[0] == LR.VOID).double().mean())
    assert 0.2 < frac < 0.4 and bool(t[1, -1] == LR.VOID) and int((t[1] == LR.VOID).sum()) == 1
    _, t = LR.hinge_case(4, 300, 'image')
    assert bool((t[0] == LR.VOID).all()) and not bool((t[1:] == LR.VOID).any())
    _, t = LR.hinge_case(2, 300, 'single')
    assert int((t[0] != LR.VOID).sum()) == 1
    _, t = LR.hinge_case(1, 4098, 'three')
    assert int((t != LR.VOID).sum()) == 4095, 'the valid count crosses the segment boundary at 4096'
    _, t = LR.softmax_case(2, 2, 300, 'some', 'image')
    assert not bool((t[0, 1] == 1).any()) and bool((t[1, 1] == 1).any()), 'class 1 is absent from image 0 only'
    void = t[:, 0] == LR.VOID
    assert bool(void.any()) and bool(((t[:, 1] == LR.VOID) == void).all()), 'the void value sits in every plane of the pixel'
    _, t = LR.softmax_case(2, 2, 300, None, 'batch')
    assert not bool((t[:, 1] == 1).any())
    _, t = LR.softmax_case(2, 2, 300, 'image')
    assert bool((t[0] == LR.VOID).all())


def test_lovasz_params_refusals():
    from salt_amd import losses
    from salt_amd._abi import SaltError
    assert losses.lovasz_params('lovasz', None) == (True, None)
    assert losses.lovasz_params('lovasz_softmax', {'ignore': 255, 'only_present': True}) == (True, True, 255.0)
    for kind, bad in (('lovasz', {'only_present': True}), ('lovasz', {'per_img': False}), ('lovasz_softmax', {'ignore': float('nan')}),
                      ('lovasz', {'ignore': 'void'}), ('lovasz', {'ignore': True}), ('lovasz_softmax', {'per_image': 0}),
                      ('bce_dice', {})):
        with pytest.raises(SaltError) as ei:
            losses.lovasz_params(kind, bad)
        if 'only_present' in bad or 'per_img' in bad:
            assert 'per_image' in str(ei.value) and 'ignore' in str(ei.value), 'an unknown key names the choices'
