"""Operator-level parity of the softmax head's kernels through the C-ABI against the float64 references of softmax_loss_reference.py:
salt_softmax / salt_softmax_bwd, salt_lovasz_softmax (unsplit and split sort) and salt_dice_ce.  Every output has a NaN guard word one
past its end, and a forward-only call leaves the gradient buffer alone.

Tolerances (none measured on the kernels):
  salt_lovasz_softmax   those of the hinge test of the same operation sequence (test_gpu_ops_loss.py::test_lovasz_small_sizes): loss
                        2e-5 max(1, |ref|); gradient 5e-3 max|ref|, the fp32 cancellation of g_k = J_k - J_(k-1).  The probabilities are
                        multiples of 1/32, so every error is exact in fp32 and the stable order is the only valid one.
  salt_softmax (_bwd)   the fp32 elementwise bar of test_gpu_ops_loss.py, 5e-5 max|ref|.
  salt_dice_ce          salt_bce_dice's: loss 2e-5 max(1, |ref|), gradient 5e-5 max|ref|, sums 1.5e-4 of the vector's max."""
import ctypes
import math

import pytest
import torch

import softmax_loss_reference as SR
from abi_ops import _abi, call, raw, close, DEV, F64, NAN

pytestmark = pytest.mark.gpu


def _rel(got, ref, tol, what):
    got, ref = got.to(F64).cpu().reshape(-1), ref.to(F64).reshape(-1)
    mx, err = float(ref.abs().max()), float((got - ref).abs().max())
    print('%s: max err %.3e, max|ref| %.3e' % (what, err, mx))
    assert bool(torch.isfinite(got).all()) and err <= tol * mx, '%s: max err %.3e > %.1e x %.3e' % (what, err, tol, mx)


def _guarded(n):
    return torch.full((n + 1,), NAN, device=DEV)


# ---------------------------------------------------------------- softmax and its Jacobian
SOFTMAX_SHAPES = [(1, 2, 1), (2, 3, 255), (2, 4, 4097)]


def _softmax(z):
    B, C, HW = z.shape
    x, y = z.float().to(DEV).contiguous(), _guarded(B * C * HW)
    call('salt_softmax', x=x.data_ptr(), y=y.data_ptr(), B=B, C=C, HW=HW)
    assert bool(torch.isnan(y[-1])), 'one past the end'
    return y[:-1].reshape(B, C, HW).cpu().to(F64)


@pytest.mark.parametrize('shape', SOFTMAX_SHAPES)
def test_softmax(shape):
    from op_reference import round_to
    z = round_to(torch.randn(shape, generator=SR.gen('softmax', shape), dtype=F64) * 3, 'f32')
    close(_softmax(z), SR.softmax(z), 'f32', 'softmax %s' % (shape,))


def test_softmax_large_logits():
    shape = (2, 4, 4097)
    z = SR.large_logits(shape, SR.gen('softmax large'))
    got = _softmax(z)
    assert bool(torch.isfinite(got).all())
    close(got, SR.softmax(z), 'f32', 'softmax, logits of +-80')


@pytest.mark.parametrize('shape', SOFTMAX_SHAPES)
def test_softmax_bwd(shape):
    from op_reference import round_to
    B, C, HW = shape
    g = SR.gen('softmax_bwd', shape)
    p = round_to(SR.softmax(torch.randn(shape, generator=g, dtype=F64) * 3), 'f32')
    dp = round_to(torch.randn(shape, generator=g, dtype=F64), 'f32')
    pd, dpd, dz = p.float().to(DEV).contiguous(), dp.float().to(DEV).contiguous(), _guarded(B * C * HW)
    call('salt_softmax_bwd', p=pd.data_ptr(), dp=dpd.data_ptr(), dz=dz.data_ptr(), B=B, C=C, HW=HW)
    assert bool(torch.isnan(dz[-1])), 'one past the end'
    close(dz[:-1].reshape(shape).cpu().to(F64), SR.softmax_bwd(p, dp), 'f32', 'softmax_bwd %s' % (shape,))
    # in place, as the loss programs run it (dz = dp)
    call('salt_softmax_bwd', p=pd.data_ptr(), dp=dpd.data_ptr(), dz=dpd.data_ptr(), B=B, C=C, HW=HW)
    assert torch.equal(dpd.reshape(-1), dz[:-1])


def test_softmax_refusals_come_from_host_code_and_launch_nothing():
    abi = _abi()
    BAD = abi.CONSTS['SALT_E_BADARG']
    x = torch.randn(2 * 5 * 8, device=DEV)
    y = torch.full((2 * 5 * 8,), NAN, device=DEV)
    ok = dict(x=x.data_ptr(), y=y.data_ptr(), B=2, C=3, HW=8)
    for bad in (dict(C=1), dict(C=5), dict(x=None), dict(y=None), dict(B=0), dict(HW=0)):
        assert raw('salt_softmax', **dict(ok, **bad)) == BAD, bad
        assert b'softmax' in abi.lib.salt_last_error()
    okb = dict(p=x.data_ptr(), dp=x.data_ptr(), dz=y.data_ptr(), B=2, C=3, HW=8)
    for bad in (dict(C=1), dict(C=5), dict(p=None), dict(dp=None), dict(dz=None), dict(B=0), dict(HW=0)):
        assert raw('salt_softmax_bwd', **dict(okb, **bad)) == BAD, bad
    assert bool(torch.isnan(y).all()), 'a refused call wrote its output'
    fn, S = abi.OP_FUNCS['salt_softmax']
    assert fn(None, None) == BAD
    # the losses refuse the same channel counts
    assert abi.lib.salt_dice_ce_parts(ctypes.byref(abi.fill(abi.STRUCTS['salt_dice_ce_args'](), B=2, C=1, HW=8))) == -1
    assert abi.lib.salt_dice_ce_parts(ctypes.byref(abi.fill(abi.STRUCTS['salt_dice_ce_args'](), B=2, C=5, HW=8))) == -1
    w = torch.zeros(64, dtype=torch.int32, device=DEV)
    for C in (1, 5):
        assert raw('salt_lovasz_softmax', probas=x.data_ptr(), target=x.data_ptr(), B=2, C=C, HW=8, ws_keys=w.data_ptr(), ws_vals=w.data_ptr(),
                   loss_per_row=y.data_ptr(), loss=y.data_ptr(), dprobas=None, loss_scale=1.0, ws_split=None) == BAD
        assert raw('salt_dice_ce', logits=x.data_ptr(), target=x.data_ptr(), B=2, C=C, HW=8, dice_weight=0.5, cross_entropy_weight=0.5, smooth=0.0,
                   partials=y.data_ptr(), nparts=2, sums=y.data_ptr(), loss=y.data_ptr(), dlogits=None, loss_scale=1.0) == BAD
    assert bool(torch.isnan(y).all())


# ---------------------------------------------------------------- Lovasz-softmax
_LOVASZ_REF = {}


def _lovasz_ref(C, HW):
    """the case and its float64 result, computed once and shared (never modified)"""
    if (C, HW) not in _LOVASZ_REF:
        p, t = SR.lovasz_case(C, HW)
        _LOVASZ_REF[(C, HW)] = (p, t) + SR.lovasz_softmax(p, t, 0.5)
    return _LOVASZ_REF[(C, HW)]


def _lovasz_softmax(p, t, with_grad, split):
    abi = _abi()
    B, C, HW = p.shape
    pd, td = p.float().to(DEV).contiguous(), t.float().to(DEV).contiguous()
    wk = torch.empty(2 * B * C * HW, dtype=torch.int32, device=DEV)
    wv = torch.empty(2 * B * C * HW, dtype=torch.int32, device=DEV)
    sw = int(abi.lib.salt_lovasz_split_words(HW))
    assert (sw > 0) == (HW >= 4096)
    ws = torch.empty(max(1, B * C * sw), dtype=torch.int32, device=DEV) if split else None     # below 4096 a given workspace is not used
    rows, loss, dp = _guarded(B * C), _guarded(1), _guarded(B * C * HW)
    call('salt_lovasz_softmax', probas=pd.data_ptr(), target=td.data_ptr(), B=B, C=C, HW=HW, ws_keys=wk.data_ptr(), ws_vals=wv.data_ptr(),
         loss_per_row=rows.data_ptr(), loss=loss.data_ptr(), dprobas=dp.data_ptr() if with_grad else None, loss_scale=0.5,
         ws_split=ws.data_ptr() if split else None)
    assert bool(torch.isnan(rows[-1])) and bool(torch.isnan(loss[-1])) and bool(torch.isnan(dp[-1])), 'one past the end'
    if not with_grad:
        assert bool(torch.isnan(dp).all()), 'forward-only call leaves dprobas alone'
    return float(loss[0]), rows[:-1].cpu().to(F64), dp[:-1].reshape(B, C, HW)


@pytest.mark.parametrize('with_grad', [1, 0])
@pytest.mark.parametrize('C', SR.LOVASZ_C)
@pytest.mark.parametrize('HW', SR.LOVASZ_HW)
def test_lovasz_softmax(HW, C, with_grad):
    """ws_split NULL and given for every size; from 4096 on the given workspace selects the split sort, whose gradients are bit-identical
    to the unsplit form's"""
    p, t, lref, gref, rref = _lovasz_ref(C, HW)
    B = p.shape[0]
    got = {}
    for split in (False, True):
        loss, rows, dp = _lovasz_softmax(p, t, with_grad, split)
        what = 'lovasz_softmax C=%d HW=%d %s' % (C, HW, 'split' if split else 'unsplit')
        print('%s: loss %.8f ref %.8f' % (what, loss, lref))
        assert abs(loss - lref) <= 2e-5 * max(1.0, abs(lref)), (what, loss, lref)
        assert abs(float(rows.mean()) - float(rref.mean())) <= 2e-5 * max(1.0, abs(float(rref.mean()))), what
        if with_grad:
            _rel(dp, gref, 5e-3, what + ' dprobas (stable ties)')
            e0 = ((t > 0.5).to(F64) - p) == 0
            assert bool((dp.cpu()[e0] == 0).all()), 'the gradient is exactly 0 where the error is 0'
        got[split] = dp
    if with_grad:
        assert torch.equal(got[False], got[True]), 'split and unsplit gradients differ'


# ---------------------------------------------------------------- Dice + cross entropy
def _dice_ce(z, t, scale, with_grad, dw=0.5, cw=0.5, smooth=0.0):
    abi = _abi()
    B, C, HW = z.shape
    zd, td = z.float().to(DEV).contiguous(), t.float().to(DEV).contiguous()
    args = abi.fill(abi.STRUCTS['salt_dice_ce_args'](), B=B, C=C, HW=HW)
    nparts = int(abi.lib.salt_dice_ce_parts(ctypes.byref(args)))
    # parts per image (salt_bce_dice's rule per plane): one up to 4096 positions, two from 4097 on, never more than 16
    assert nparts == B * {1: 1, 255: 1, 4096: 1, 4097: 2, 65537: 16}[HW]
    partials, sums, loss, dz = _guarded(nparts * (3 * C + 1)), _guarded(3 * C + 1), _guarded(1), _guarded(B * C * HW)
    kw = dict(logits=zd.data_ptr(), target=td.data_ptr(), B=B, C=C, HW=HW, dice_weight=dw, cross_entropy_weight=cw, smooth=smooth,
              partials=partials.data_ptr(), nparts=nparts, sums=sums.data_ptr(), loss=loss.data_ptr(), dlogits=dz.data_ptr() if with_grad else None,
              loss_scale=scale)
    call('salt_dice_ce', **kw)
    assert bool(torch.isnan(partials[-1])) and bool(torch.isnan(sums[-1])) and bool(torch.isnan(loss[-1])) and bool(torch.isnan(dz[-1])), 'one past the end'
    if not with_grad:
        assert bool(torch.isnan(dz).all()), 'forward-only call leaves dlogits alone'
    first = (loss.clone(), sums.clone(), dz.clone())
    call('salt_dice_ce', **kw)                                      # fixed-order sums, no floating-point atomics: a rerun gives the same bits
    for a, b in zip(first, (loss, sums, dz)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), 'two runs differ'
    assert raw('salt_dice_ce', **dict(kw, nparts=nparts + 1)) == abi.CONSTS['SALT_E_BADARG']
    return float(loss[0]), sums[:-1], dz[:-1].reshape(B, C, HW)


def _check_dice_ce(z, t, scale, with_grad, what, **weights):
    lref, gref, sref = SR.dice_ce(z, t, weights.get('dw', 0.5), weights.get('cw', 0.5), weights.get('smooth', 0.0), scale)
    loss, sums, dz = _dice_ce(z, t, scale, with_grad, **weights)
    print('%s: loss %.8f ref %.8f' % (what, loss, lref))
    assert math.isfinite(loss) and abs(loss - lref) <= 2e-5 * max(1.0, abs(lref)), (what, loss, lref)
    _rel(sums, sref, 1.5e-4, what + ' sums')
    if with_grad:
        _rel(dz, gref, 5e-5, what + ' dlogits')


@pytest.mark.parametrize('with_grad', [1, 0])
@pytest.mark.parametrize('scale', [1.0, 0.25])
@pytest.mark.parametrize('kind', ['random', 'background'])
@pytest.mark.parametrize('shape', [(1, 2, 1), (2, 2, 255), (3, 3, 4096), (2, 2, 4097), (1, 4, 65537)])
def test_dice_ce(shape, kind, scale, with_grad):
    from op_reference import round_to
    g = SR.gen('dice_ce', shape, kind)
    z = round_to(torch.randn(shape, generator=g, dtype=F64) * 3, 'f32')
    _check_dice_ce(z, SR.random_target(shape, g, kind), scale, with_grad, 'dice_ce %s %s' % (shape, kind))


@pytest.mark.parametrize('scale', [1.0, 0.25])
def test_dice_ce_large_logits(scale):
    g = SR.gen('dice_ce large')
    shape = (2, 2, 4097)
    _check_dice_ce(SR.large_logits(shape, g), SR.random_target(shape, g), scale, 1, 'dice_ce, logits of +-80')


def test_dice_ce_weights_and_smooth():
    from op_reference import round_to
    g = SR.gen('dice_ce weights')
    shape = (3, 3, 4096)
    z = round_to(torch.randn(shape, generator=g, dtype=F64) * 3, 'f32')
    _check_dice_ce(z, SR.random_target(shape, g), 1.0, 1, 'dice_ce 0.2 / 0.9 / smooth 1', dw=0.2, cw=0.9, smooth=1.0)
