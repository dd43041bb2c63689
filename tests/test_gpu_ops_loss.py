"""Operator-level parity of salt_bce_dice, the small sizes of salt_lovasz_hinge, salt_adam and salt_adam_tick through the C-ABI against
the fp64 references of op_reference.py (oracle.losses through autograd, torch.optim semantics in double).

Tolerances (none measured on the kernels): losses 2e-5 (test_gpu_loss_optim.py); `sums` 1.5e-4 of the vector's max (fp32 tiles);
gradients 5e-5 of max|ref| (f32 elementwise); Adam moments 1e-6 of their max, the update p_after - p_before at 1e-4 of max|update|
(with |p| <= 0.1 an fp32 ulp of p is 7.5e-9, two orders below 1e-4 x lr = 1e-6)."""
import ctypes
import math

import numpy as np
import pytest
import torch

import op_reference as R
from abi_ops import _abi, call, gen, DEV, F64, NAN

pytestmark = pytest.mark.gpu


def _rel(got, ref, tol, what):
    got, ref = got.to(F64).cpu().reshape(-1), ref.to(F64).reshape(-1)
    mx, err = float(ref.abs().max()), float((got - ref).abs().max())
    print('%s: max err %.3e, max|ref| %.3e' % (what, err, mx))
    assert bool(torch.isfinite(got).all()) and err <= tol * mx, '%s: max err %.3e > %.1e x %.3e' % (what, err, tol, mx)


# ---------------------------------------------------------------- BCE + Dice
def _bce_dice(z, t, scale, with_grad):
    abi = _abi()
    B, C, HW = z.shape
    zd, td = z.float().to(DEV).contiguous(), t.float().to(DEV).contiguous()
    S = abi.STRUCTS['salt_bce_dice_args']
    args = abi.fill(S(), logits=zd.data_ptr(), target=td.data_ptr(), B=B, C=C, HW=HW, dice_weight=0.2, bce_weight=0.9, loss_scale=scale)
    nparts = int(abi.lib.salt_bce_dice_parts(ctypes.byref(args)))
    # parts per plane: one up to 4096 positions, two from 4097 on, never more than 16
    assert nparts == B * C * {1: 1, 255: 1, 4096: 1, 4097: 2, 65537: 16}[HW]
    partials = torch.full((nparts * 4 + 1,), NAN, device=DEV)
    sums = torch.full((3 * C + 2,), NAN, device=DEV)
    loss = torch.full((2,), NAN, device=DEV)
    dz = torch.full((B * C * HW + 1,), NAN, device=DEV)
    call('salt_bce_dice', logits=zd.data_ptr(), target=td.data_ptr(), B=B, C=C, HW=HW, dice_weight=0.2, bce_weight=0.9, partials=partials.data_ptr(),
         nparts=nparts, sums=sums.data_ptr(), loss=loss.data_ptr(), dlogits=dz.data_ptr() if with_grad else None, loss_scale=scale)
    assert bool(torch.isnan(partials[-1])) and bool(torch.isnan(sums[-1])) and bool(torch.isnan(loss[1])) and bool(torch.isnan(dz[-1])), 'one past the end'
    if not with_grad:
        assert bool(torch.isnan(dz).all()), 'forward-only call leaves dlogits alone'
    return float(loss[0]), sums[:3 * C + 1], dz[:-1].reshape(B, C, HW)


@pytest.mark.parametrize('with_grad', [1, 0])
@pytest.mark.parametrize('scale', [1.0, 0.25])
@pytest.mark.parametrize('kind', ['random', 'empty'])
@pytest.mark.parametrize('shape', [(1, 1, 1), (2, 2, 255), (3, 2, 4096), (2, 1, 4097), (1, 2, 65537)])
def test_bce_dice(shape, kind, scale, with_grad):
    g = gen('bce_dice', shape, kind)
    z = R.round_to(torch.randn(shape, generator=g, dtype=F64) * 3, 'f32')
    t = (torch.rand(shape, generator=g) < 0.3).to(F64) if kind == 'random' else torch.zeros(shape, dtype=F64)
    lref, gref, sref = R.bce_dice(z, t, 0.2, 0.9, scale)
    loss, sums, dz = _bce_dice(z, t, scale, with_grad)
    assert abs(loss - lref) <= 2e-5 * max(1.0, abs(lref)), (loss, lref)
    _rel(sums, sref, 1.5e-4, 'bce_dice sums')
    if with_grad:
        _rel(dz, gref, 5e-5, 'bce_dice dlogits')


@pytest.mark.parametrize('scale', [1.0, 0.25])
def test_bce_dice_large_logits(scale):
    g = gen('bce_dice large')
    shape = (2, 2, 4097)
    z = torch.tensor([-80.0, -15.0, 0.0, 15.0, 80.0], dtype=F64)[torch.randint(0, 5, shape, generator=g)]
    t = (torch.rand(shape, generator=g) < 0.4).to(F64)
    lref, gref, sref = R.bce_dice(z, t, 0.2, 0.9, scale)
    loss, sums, dz = _bce_dice(z, t, scale, 1)
    assert math.isfinite(loss) and abs(loss - lref) <= 2e-5 * max(1.0, abs(lref)), (loss, lref)
    _rel(sums, sref, 1.5e-4, 'bce_dice sums (large logits)')
    _rel(dz, gref, 5e-5, 'bce_dice dlogits (large logits)')


# ---------------------------------------------------------------- Lovasz hinge, small sizes
@pytest.mark.parametrize('with_grad', [1, 0])
@pytest.mark.parametrize('P', [1, 2, 255, 4095, 4096])
def test_lovasz_small_sizes(P, with_grad):
    from oracle import losses as OL
    B = 3
    g = gen('lovasz', P)
    z = torch.round(torch.randn(B, P, generator=g) * 4) / 2                # multiples of 0.5: tie groups, whose order must be the stable one
    t = (torch.rand(B, P, generator=g) < 0.4).float()
    t[0] = 0
    lref, gref = OL.lovasz_hinge_grad_closed_form(z, t)
    zd, td = z.to(DEV).contiguous(), t.to(DEV).contiguous()
    wk = torch.empty(2 * B * P, dtype=torch.int32, device=DEV)
    wv = torch.empty(2 * B * P, dtype=torch.int32, device=DEV)
    lpi, loss, dl = torch.full((B + 1,), NAN, device=DEV), torch.full((2,), NAN, device=DEV), torch.full((B * P + 1,), NAN, device=DEV)
    call('salt_lovasz_hinge', logits=zd.data_ptr(), target=td.data_ptr(), B=B, P=P, ws_keys=wk.data_ptr(), ws_vals=wv.data_ptr(),
         loss_per_image=lpi.data_ptr(), loss=loss.data_ptr(), dlogits=dl.data_ptr() if with_grad else None, loss_scale=0.5, ws_split=None)
    assert bool(torch.isnan(lpi[B])) and bool(torch.isnan(loss[1])) and bool(torch.isnan(dl[-1]))
    assert abs(float(loss[0]) - 0.5 * lref) <= 2e-5 * max(1.0, abs(0.5 * lref)), (float(loss[0]), 0.5 * lref)
    assert abs(float(lpi[:B].sum()) / B - lref) <= 2e-5 * max(1.0, abs(lref))
    if with_grad:
        # test_gpu_loss_optim.py: against the float64 closed form the bar is the fp32 cancellation of g_k = J_k - J_(k-1), 5e-3
        _rel(dl[:-1].reshape(B, P), 0.5 * gref, 5e-3, 'lovasz dlogits (stable ties)')
    else:
        assert bool(torch.isnan(dl).all())


# ---------------------------------------------------------------- Adam
def _hyper(lr, wd, t, gs):
    bc1, bc2 = R.tick(0.9, 0.999, t)
    return [lr, 0.9, 0.999, 1e-8, wd, bc1, bc2, gs]


@pytest.mark.parametrize('t', [1, 1000])
@pytest.mark.parametrize('wd', [0.0, 1e-4])
@pytest.mark.parametrize('gs', [1.0, 1.0 / 64])
@pytest.mark.parametrize('n', [1, 3, 4, 5, 1023, 4194311])
def test_adam(n, gs, wd, t):
    g = gen('adam', n)
    hyper = R.round_to(torch.tensor(_hyper(1e-2, wd, t, gs), dtype=F64), 'f32')          # the kernel reads fp32 hyper-parameters: same values
    p = R.round_to((torch.rand(n, generator=g, dtype=F64) - 0.5) * 0.2, 'f32')            # |p| <= 0.1
    gr = R.round_to(torch.randn(n, generator=g, dtype=F64) * 0.1 / gs, 'f32')
    m = R.round_to(torch.randn(n, generator=g, dtype=F64) * 0.05, 'f32') if t > 1 else torch.zeros(n, dtype=F64)
    v = R.round_to(torch.rand(n, generator=g, dtype=F64) * 0.01, 'f32') if t > 1 else torch.zeros(n, dtype=F64)
    pr, mr, vr = R.adam(p, gr, m, v, hyper)

    def dev(x):                                                        # one guard element past the end
        return torch.cat([x.float(), torch.full((1,), 12345.0)]).to(DEV)
    dp, dg, dm, dv = dev(p), dev(gr), dev(m), dev(v)
    dh = hyper.float().to(DEV)
    call('salt_adam', param=dp.data_ptr(), grad=dg.data_ptr(), exp_avg=dm.data_ptr(), exp_avg_sq=dv.data_ptr(), n=n, hyper=dh.data_ptr())
    for x in (dp, dg, dm, dv):
        assert float(x[n]) == 12345.0, 'element past the end'
    assert torch.equal(dg[:n].cpu().to(F64), gr) and torch.equal(dh.cpu().to(F64), hyper)
    if n == 1 and t == 1000:
        # one element whose new moment cancels: b1 m = -8.747e-3, (1 - b1) g = 8.843e-3, result 9.5e-5 - "1e-6 of the max" is then 1e-10,
        # below one rounding of the operands.  By the rule for a failed bound: plain fp32 torch on the CPU is 2.911e-10 (weight decay 0)
        # and 1.157e-10 (1e-4) from the fp64 reference -> 4 x 2.911e-10
        assert abs(float(dm[0]) - float(mr[0])) <= 4 * 2.911e-10, (float(dm[0]), float(mr[0]))
    else:
        _rel(dm[:n], mr, 1e-6, 'adam exp_avg')
    _rel(dv[:n], vr, 1e-6, 'adam exp_avg_sq')
    if n == 1 and t == 1000:
        # the same element: its update is 7.9e-6 (not ~ lr), and p = 0.0574 is stored in fp32 (half an ulp: 3.4e-9), so 1e-4 of the update
        # is below the representation of p.  Plain fp32 torch on the CPU is 1.208e-9 (weight decay 0) / 4.356e-10 (1e-4) from the fp64
        # update -> 4 x 1.208e-9
        assert abs((float(dp[0]) - float(p[0])) - float(pr[0] - p[0])) <= 4 * 1.208e-9
    else:
        _rel(dp[:n].cpu().to(F64) - p, pr - p, 1e-4, 'adam update')


@pytest.mark.parametrize('step', [0, 1, 999])
def test_adam_tick(step):
    hyper = torch.tensor([1e-2, 0.9, 0.999, 1e-8, 1e-4, -1.0, -1.0, 1.0 / 64], dtype=torch.float32)
    dh = torch.cat([hyper, torch.full((1,), 777.0)]).to(DEV)
    ds = torch.tensor([55, step, 55], dtype=torch.int64, device=DEV)
    call('salt_adam_tick', hyper=dh.data_ptr(), step=ds.data_ptr() + 8)
    assert ds.cpu().tolist() == [55, step + 1, 55]
    got = dh.cpu()
    keep = [0, 1, 2, 3, 4, 7]
    assert torch.equal(got[keep], hyper[keep]) and float(got[8]) == 777.0, 'the other six words are unchanged'
    for k, beta in ((5, hyper[1]), (6, hyper[2])):
        ref = np.float32(R.tick(float(beta), float(beta), step + 1)[0])            # the beta the kernel reads (fp32), the power in double
        ulp = float(np.spacing(ref))
        assert abs(float(got[k]) - float(ref)) <= ulp, (k, float(got[k]), float(ref))
