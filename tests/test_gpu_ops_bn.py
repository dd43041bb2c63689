"""Operator-level parity of the BatchNorm kernels of csrc/elementwise.hip through the C-ABI against the fp64 references of
op_reference.py: salt_bn_finalize fed with partials directly (batch boundaries 64 / 1024, unequal counts, a large-offset channel,
N == 1), salt_bn_fold, the consumer-side finalize of salt_affine_act (fin_acc) and every mode of salt_bn_bwd (partials, fp64 shards
with and without ticket, caller-written partials / shards), its mask sources, da_bias, dres, the accumulate flags, the two channel
blocks of a 301-channel scalar reduction, the grid-stride loop of the apply pass and the secondary sums.

Tolerances (none measured on the kernels): elementwise outputs as in test_gpu_ops_streaming.py (close() of abi_ops.py); per-channel reductions 1.5e-4 of the
vector's max where sums are formed in fp32 tiles (tol * 3 of test_gpu_blocks.py for dgamma / dbeta), 1e-6 where the kernels work in fp64
from caller-given partials or shards."""
import ctypes

import pytest
import torch

import op_reference as R
from op_reference import Placed, VIEW_CASES, VARIANTS
from abi_ops import _abi, call, code, gen, rnd, close, null_view, DEV, F64, NAN, VIEWS_IDS

pytestmark = pytest.mark.gpu
TOL_TILE, TOL_F64 = 1.5e-4, 1e-6


def vec_close(got, ref, tol, what):
    got, ref = got.to(F64).cpu().reshape(-1), ref.to(F64).reshape(-1)
    mx = float(ref.abs().max())
    err = float((got - ref).abs().max())
    print('%s: max err %.3e, max|ref| %.3e, bound %.3e' % (what, err, mx, tol * mx))
    assert bool(torch.isfinite(got).all()) and err <= tol * mx, '%s: max err %.3e > %.1e x max|ref| %.3e' % (what, err, tol, mx)


def dev32(t):
    return t.to(torch.float32).to(DEV).contiguous()


# ---------------------------------------------------------------- bn_finalize fed directly
def _partials(nparts, C, g, n_is_one=False):
    """(partials [nparts, 2, C] as fp32 holds them, counts [nparts]); first and last partial smaller; channel 0 has mean 100, std 0.05."""
    if n_is_one:
        counts = torch.ones(1, dtype=F64)
    else:
        counts = torch.full((nparts,), 32.0, dtype=F64)
        counts[0], counts[-1] = 5.0, 7.0 if nparts > 1 else 5.0
        if nparts > 4:
            counts[3] = 17.0
    means = torch.randn(nparts, C, generator=g, dtype=F64) * 0.5 + torch.linspace(-1, 1, C, dtype=F64)
    m2 = (torch.rand(nparts, C, generator=g, dtype=F64) + 0.5) * (counts - 1).reshape(-1, 1)
    means[:, 0] = 100 + 0.05 * torch.randn(nparts, generator=g, dtype=F64) / counts.sqrt()
    m2[:, 0] = 0.0025 * (counts - 1)
    sums = means * counts.reshape(-1, 1)
    return R.round_to(torch.stack([sums, m2], 1), 'f32'), counts


@pytest.mark.parametrize('nbt', [0, 1])
@pytest.mark.parametrize('running', [1, 0])
@pytest.mark.parametrize('C', [1, 5, 64])
@pytest.mark.parametrize('nparts', [1, 63, 64, 65, 1024, 1025, 'N=1'])
def test_bn_finalize_from_partials(nparts, C, running, nbt):
    n1 = nparts == 'N=1'
    nparts = 1 if n1 else nparts
    g = gen('bn_finalize', nparts, C, n1)
    partials, counts = _partials(nparts, C, g, n1)
    gamma, beta = R.round_to(torch.rand(C, generator=g, dtype=F64) + 0.5, 'f32'), R.round_to(torch.randn(C, generator=g, dtype=F64), 'f32')
    rm, rv = R.round_to(torch.randn(C, generator=g, dtype=F64), 'f32'), R.round_to(torch.rand(C, generator=g, dtype=F64) + 0.5, 'f32')
    ref = R.bn_finalize(partials, counts, gamma, beta, rm if running else None, rv if running else None, 0.1, 1e-5)
    d = {k: dev32(v) for k, v in dict(stats=partials, cnt=counts, gamma=gamma, beta=beta, rm=rm, rv=rv).items()}
    out = {k: torch.full((C,), NAN, device=DEV) for k in ('mean', 'invstd', 'scale', 'shift')}
    steps = torch.full((3,), 41, dtype=torch.int64, device=DEV)
    call('salt_bn_finalize', stats=d['stats'].data_ptr(), stats_cnt=d['cnt'].data_ptr(), nparts=nparts, C=C, gamma=d['gamma'].data_ptr(),
         beta=d['beta'].data_ptr(), running_mean=d['rm'].data_ptr() if running else None, running_var=d['rv'].data_ptr() if running else None,
         num_batches_tracked=steps.data_ptr() + 8 if nbt else None, momentum=0.1, eps=1e-5,
         **{k: v.data_ptr() for k, v in out.items()})
    for k in out:
        vec_close(out[k], ref[k], TOL_F64, 'bn_finalize %s' % k)
    if running:
        vec_close(d['rm'], ref['running_mean'], TOL_F64, 'running_mean')
        vec_close(d['rv'], ref['running_var'], TOL_F64, 'running_var')
    else:
        assert torch.equal(d['rm'].cpu().to(F64), rm) and torch.equal(d['rv'].cpu().to(F64), rv)
    assert steps.cpu().tolist() == [41, 42 if nbt else 41, 41]
    assert torch.equal(d['stats'].cpu().to(F64), partials)


@pytest.mark.parametrize('C', [1, 65])
def test_bn_fold(C):
    g = gen('bn_fold', C)
    gamma, beta, rm = (R.round_to(torch.randn(C, generator=g, dtype=F64), 'f32') for _ in range(3))
    rv = R.round_to(torch.rand(C, generator=g, dtype=F64) + 0.1, 'f32')
    scale, shift = torch.full((C + 1,), NAN, device=DEV), torch.full((C + 1,), NAN, device=DEV)
    dg, db, dm, dv = dev32(gamma), dev32(beta), dev32(rm), dev32(rv)
    call('salt_bn_fold', C=C, gamma=dg.data_ptr(), beta=db.data_ptr(), running_mean=dm.data_ptr(), running_var=dv.data_ptr(), eps=1e-5,
         scale=scale.data_ptr(), shift=shift.data_ptr())
    rs, rh = R.bn_fold(gamma, beta, rm, rv, 1e-5)
    vec_close(scale[:C], rs, 5e-5, 'bn_fold scale')
    vec_close(shift[:C], rh, 5e-5, 'bn_fold shift')
    assert bool(torch.isnan(scale[C])) and bool(torch.isnan(shift[C])), 'one past the end untouched'


# ---------------------------------------------------------------- affine_act with the consumer-side finalize
def _fin_struct(keep, C, gamma, beta, rm, rv, steps, momentum=0.1, eps=1e-5):
    abi = _abi()
    out = {k: torch.full((C,), NAN, device=DEV) for k in ('mean', 'invstd', 'scale', 'shift')}
    f = abi.fill(abi.STRUCTS['salt_bn_finalize_args'](), stats=None, stats_cnt=None, nparts=0, C=C, gamma=gamma.data_ptr(), beta=beta.data_ptr(),
                 running_mean=rm.data_ptr(), running_var=rv.data_ptr(), num_batches_tracked=steps.data_ptr(), momentum=momentum, eps=eps,
                 **{k: v.data_ptr() for k, v in out.items()})
    keep.append(f)
    return f, out


def _fin_problem(dtype, views, with_res, relu):
    """Inputs and fp64 reference of the consumer-finalize case: the statistics of the values as stored, split unevenly over the 8 shards
    (two of them empty); channel 3 has mean 100 and standard deviation 0.05."""
    vin, vout = views
    shape = (2, 6, 8)
    C = VARIANTS[vin][dtype][1]
    g = gen('affine fin', dtype, vin, vout, with_res, relu)
    y = torch.randn(shape + (C,), generator=g, dtype=F64) * 1.5 + torch.linspace(-1, 1, C, dtype=F64)
    y[..., 3] = 100 + 0.05 * torch.randn(shape, generator=g, dtype=F64)
    y = R.round_to(y, dtype)
    res = rnd(shape + (C,), g, dtype) if with_res else None
    gamma, beta = R.round_to(torch.rand(C, generator=g, dtype=F64) + 0.5, 'f32'), R.round_to(torch.randn(C, generator=g, dtype=F64) * 0.3, 'f32')
    rm, rv = R.round_to(torch.randn(C, generator=g, dtype=F64), 'f32'), R.round_to(torch.rand(C, generator=g, dtype=F64) + 0.5, 'f32')
    flat = y.reshape(-1, C)
    cuts = [0, 1, 30, 30, 31, 70, 70, 95, flat.shape[0]]
    shards = torch.zeros(8, 2 * C + 1, dtype=F64)
    for s in range(8):
        p = flat[cuts[s]:cuts[s + 1]]
        shards[s, :C], shards[s, C:2 * C], shards[s, 2 * C] = p.sum(0), (p * p).sum(0), p.shape[0]
    assert float(shards[2, 2 * C]) == 0 and float(shards[5, 2 * C]) == 0
    ref = R.bn_finalize_shards(shards, gamma, beta, rm, rv, 0.1, 1e-5)
    aref = R.affine_act(y, ref['scale'], ref['shift'], res, relu)
    return shape, C, y, res, gamma, beta, rm, rv, shards, ref, aref


@pytest.mark.parametrize('with_res,relu', [(0, 1), (1, 0)])
@pytest.mark.parametrize('views', [('a', 'a'), ('d', 'd'), ('b', 'c'), ('c', 'b')], ids=['a-a', 'd-d', 'b-c', 'c-b'])      # C = 16 and 13
@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_affine_act_consumer_finalize(dtype, views, with_res, relu):
    vin, vout = views
    shape, C, y, res, gamma, beta, rm, rv, shards, ref, aref = _fin_problem(dtype, views, with_res, relu)
    keep = []
    dgam, dbet, drm, drv = dev32(gamma), dev32(beta), dev32(rm), dev32(rv)
    steps = torch.full((3,), 7, dtype=torch.int64, device=DEV)
    f, out = _fin_struct(keep, C, dgam, dbet, drm, drv, steps[1:])
    acc = shards.to(DEV).contiguous()
    py = Placed(shape, vin, dtype, DEV, y)
    pr = Placed(shape, vin, dtype, DEV, res) if with_res else None
    pa = Placed(shape, vout, dtype, DEV, torch.full(shape + (C,), NAN, dtype=F64))
    call('salt_affine_act', dtype=code(dtype), y=py.view, scale=None, shift=None, res=pr.view if with_res else null_view(), relu=relu, a=pa.view,
         fin=ctypes.addressof(f), fin_acc=acc.data_ptr())
    pa.check('affine_act fin_acc')
    for k in out:
        vec_close(out[k], ref[k], TOL_F64, 'affine_act fin_acc %s' % k)
    vec_close(drm, ref['running_mean'], TOL_F64, 'running_mean')
    vec_close(drv, ref['running_var'], TOL_F64, 'running_var')
    assert steps.cpu().tolist() == [7, 8, 7], 'num_batches_tracked advanced once'
    assert torch.equal(acc.cpu(), shards), 'the shards are left as they were'
    got = pa.get()
    if dtype == 'bf16':
        # Channel 3 (every stored value is 100, variance 0, scale = gamma / sqrt(eps) ~ 300) misses the common bound: shift ~ -3e4 is an
        # fp32 number (half an ulp: 1e-3) and y scale + shift cancels to beta.  By the rule for a failed bound: the same operation in plain
        # fp32 torch on the CPU, before the bf16 rounding, is up to 9.444e-4 from the fp64 reference on this channel (the case a-a, no
        # residual, relu; 6.6e-4 .. 6.9e-4 in the residual cases) -> 4 x 9.444e-4 replaces 5e-5 max|ref| there.  Every other channel
        # keeps the common bound.
        rest = [c for c in range(C) if c != 3]
        close(got[..., rest], aref[..., rest], dtype, 'affine_act fin_acc output')
        err3 = (got[..., 3] - aref[..., 3]).abs()
        print('affine_act fin_acc output, large-offset channel [bf16]: max err %.3e' % float(err3.max()))
        assert bool((err3 <= 2.0 ** -8 * aref[..., 3].abs() + 4 * 9.444e-4).all()), float(err3.max())
    else:
        close(got, aref, dtype, 'affine_act fin_acc output')


# ---------------------------------------------------------------- bn_bwd
MODES = ['p0', 'p0_ticket', 'p0_acc', 'p1_n1', 'p1_n7', 'p3', 'p3_bias']


def _split(total, n, g):
    """total [C] -> [n, C] pieces of one sign that add up to it (uneven fractions)."""
    fr = torch.rand(n, 1, generator=g, dtype=F64) + 0.1
    return total.reshape(1, -1) * (fr / fr.sum())


def run_bn_bwd(dtype, views, shape_bhwc, mode, mask, dres, acc_pg, bias, seed=0, sec=False):
    """One salt_bn_bwd call against R.bn_bwd.  mask: 'none' / 'a' / 'y';  dres: 'none' / 'fresh' / 'acc'."""
    abi = _abi()
    vin, vout = views
    B, H, W, C = shape_bhwc
    shape = (B, H, W)
    M = B * H * W
    g = gen('bn_bwd', dtype, str(vin), str(vout), shape_bhwc, mode, mask, dres, acc_pg, bias, seed, sec)
    relu = 0 if mask == 'none' else 1
    y = torch.randn(shape_bhwc, generator=g, dtype=F64) * 1.5 + torch.linspace(-1, 1, C, dtype=F64)
    gamma = R.round_to(torch.rand(C, generator=g, dtype=F64) + 0.5, 'f32')
    beta = R.round_to(torch.randn(C, generator=g, dtype=F64) * 0.3, 'f32')
    y = R.round_to(y, dtype)
    # mean / invstd are arguments of the operator: near the batch statistics, not equal to them
    mean = R.round_to(y.mean((0, 1, 2)) + 0.05 * torch.randn(C, generator=g, dtype=F64), 'f32')
    invstd = R.round_to((1 + 0.03 * torch.randn(C, generator=g, dtype=F64)) / torch.sqrt(y.var((0, 1, 2), unbiased=False) + 1e-5), 'f32')
    if mask == 'y':
        y = R.avoid_zero_crossings(y, lambda v: (v - mean) * invstd * gamma + beta, 1e-3, dtype)
        assert float(((y - mean) * invstd * gamma + beta).abs().min()) >= 1e-3       # condition of the element-wise comparison below
    res = rnd(shape_bhwc, g, dtype) if dres != 'none' else None
    a = R.round_to(R.affine_act(y, gamma * invstd, beta - mean * gamma * invstd, res, 1), dtype) if mask == 'a' else None
    da = R.round_to(torch.randn(shape_bhwc, generator=g, dtype=F64) + 0.3, dtype)
    da_bias = R.round_to(torch.randn(B, C, generator=g, dtype=F64) * 0.5, 'f32') if bias else None
    old_dres = rnd(shape_bhwc, g, dtype) if dres == 'acc' else None
    old_dg, old_db = R.round_to(torch.randn(C, generator=g, dtype=F64), 'f32'), R.round_to(torch.randn(C, generator=g, dtype=F64), 'f32')
    # sums the caller supplies (partials_ready 1 / 3): the test's own fp64 sums, as the buffers hold them
    pure = R.bn_bwd(da, a, y, relu, mean, invstd, gamma, beta, da_bias)
    sums, partials, nparts, fin_acc, ticket, pready = None, None, 0, None, None, 0
    if mode in ('p1_n1', 'p1_n7'):
        nparts, pready = (1 if mode == 'p1_n1' else 7), 1
        pp = R.round_to(torch.stack([_split(pure[3], nparts, g), _split(pure[2], nparts, g)], 1), 'f32')          # [nparts][2][C]: (sum gg, sum gg xhat)
        partials = dev32(pp)
        sums = (pp[:, 0].sum(0), pp[:, 1].sum(0))
    elif mode in ('p3', 'p3_bias'):
        pready = 3
        sh = torch.stack([_split(pure[3], 8, g), _split(pure[2], 8, g)], 1)                                          # [8][2][C] fp64
        sh[2] = 0
        fin_acc = sh.to(DEV).contiguous()
        sums = (sh[:, 0].sum(0), sh[:, 1].sum(0))
    dy_ref, dres_ref, dg_ref, db_ref, coef_ref = R.bn_bwd(da, a, y, relu, mean, invstd, gamma, beta, da_bias, old_dres, dres == 'acc',
                                                          old_dg, old_db, bool(acc_pg), sums)
    pda, py = Placed(shape, vin, dtype, DEV, da), Placed(shape, vin, dtype, DEV, y)
    pa = Placed(shape, vin, dtype, DEV, a) if mask == 'a' else None
    pdy = Placed(shape, vout, dtype, DEV, torch.full(shape_bhwc, NAN, dtype=F64))
    pdres = Placed(shape, vout, dtype, DEV, old_dres if dres == 'acc' else torch.full(shape_bhwc, NAN, dtype=F64)) if dres != 'none' else None
    dmean, dinv, dgam, dbet = dev32(mean), dev32(invstd), dev32(gamma), dev32(beta)
    dgamma, dbeta = dev32(old_dg), dev32(old_db)
    coef = torch.full((3 * C + 1,), NAN, device=DEV)
    dbias = dev32(da_bias) if bias else None
    S = abi.STRUCTS['salt_bn_bwd_args']
    args = abi.fill(S(), dtype=code(dtype), da=pda.view, a=pa.view if pa else null_view(), y=py.view, relu=relu, mean=dmean.data_ptr(),
                    invstd=dinv.data_ptr(), gamma=dgam.data_ptr(), beta=dbet.data_ptr(), dgamma=dgamma.data_ptr(), dbeta=dbeta.data_ptr(),
                    accumulate_param_grads=acc_pg, coef=coef.data_ptr(), dy=pdy.view, dres=pdres.view if pdres else null_view(),
                    accumulate_dres=1 if dres == 'acc' else 0, partials_ready=pready, da_bias=dbias.data_ptr() if bias else None)
    if mode.startswith('p0'):
        nparts = int(abi.lib.salt_bn_bwd_parts(ctypes.byref(args)))
        assert nparts >= 1
        if mode == 'p0':
            partials = torch.full((nparts * 2 * C,), NAN, device=DEV)
        else:
            fin_acc = torch.zeros(8, 2, C, dtype=F64, device=DEV)
            if mode == 'p0_ticket':
                ticket = torch.zeros(3, dtype=torch.int32, device=DEV)
    abi.fill(args, partials=partials.data_ptr() if partials is not None else None, nparts=nparts,
             fin_acc=fin_acc.data_ptr() if fin_acc is not None else None, fin_ticket=ticket.data_ptr() + 4 if ticket is not None else None)
    sec_ref = None
    if sec:
        sec_y = rnd(shape_bhwc, g, dtype)
        sec_mean = R.round_to(torch.randn(C, generator=g, dtype=F64) * 0.2, 'f32')
        sec_inv = R.round_to(torch.rand(C, generator=g, dtype=F64) + 0.5, 'f32')
        psec = Placed(shape, vin, dtype, DEV, sec_y)
        dsm, dsi = dev32(sec_mean), dev32(sec_inv)
        sec_acc = torch.zeros(8, 2, C, dtype=F64, device=DEV)
        abi.fill(args, sec_y=psec.view, sec_mean=dsm.data_ptr(), sec_invstd=dsi.data_ptr(), sec_acc=sec_acc.data_ptr())
    fn = abi.OP_FUNCS['salt_bn_bwd'][0]
    abi.check(fn(ctypes.byref(args), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), 'salt_bn_bwd')
    torch.cuda.synchronize()
    what = 'bn_bwd %s mask=%s dres=%s acc_pg=%d bias=%d' % (mode, mask, dres, acc_pg, bias)
    pdy.check(what)
    tol = TOL_F64 if pready else TOL_TILE
    vec_close(coef[:3 * C].reshape(3, C)[0], coef_ref[0], 5e-5, what + ' coef k')
    vec_close(coef[:3 * C].reshape(3, C)[1], coef_ref[1], tol, what + ' coef c1')
    vec_close(coef[:3 * C].reshape(3, C)[2], coef_ref[2], tol, what + ' coef c2')
    assert bool(torch.isnan(coef[3 * C])), 'coef: one past the end untouched'
    vec_close(dgamma, dg_ref, tol, what + ' dgamma')
    vec_close(dbeta, db_ref, tol, what + ' dbeta')
    close(pdy.get(), dy_ref, dtype, what + ' dy')
    if pdres:
        pdres.check(what + ' dres')
        close(pdres.get(), dres_ref, dtype, what + ' dres')
    if mode == 'p0_ticket':
        assert ticket.cpu().tolist() == [0, 0, 0] and float(fin_acc.abs().max()) == 0.0, 'ticket and shards are left zero'
    if mode == 'p0_acc':
        vec_close(fin_acc.sum(0)[0], pure[3], TOL_TILE, what + ' shards: sum gg')
        vec_close(fin_acc.sum(0)[1], pure[2], TOL_TILE, what + ' shards: sum gg xhat')
    if pready == 3:
        assert torch.equal(fin_acc.cpu(), sh), 'caller-written shards are left as they were'
    if sec:
        stored = pdres.get()                                          # the sums are those of dres AS STORED
        xs = (sec_y - sec_mean) * sec_inv
        got = sec_acc.cpu().sum(0)
        vec_close(got[0], stored.sum((0, 1, 2)), TOL_TILE, what + ' sec: sum dres')
        vec_close(got[1], (stored * xs).sum((0, 1, 2)), TOL_TILE, what + ' sec: sum dres xhat_sec')


def _bwd_cases():
    cases, i = [], 0
    for shape in ((3, 5, 7), (2, 4, 8)):
        for mode in MODES:
            for mask in ('none', 'a', 'y'):
                dres = 'none' if mask == 'y' else ('none', 'fresh', 'acc')[i % 3]
                bias = 1 if mode == 'p3_bias' else (((i // 2) % 2) if mode.startswith('p0') else 0)
                views = VIEW_CASES[i % len(VIEW_CASES)]
                cases.append(pytest.param(('f32', 'bf16')[i % 2], views, shape, mode, mask, dres, (i // 3) % 2, bias,
                                          id='%dx%dx%d-%s-mask_%s-dres_%s-pg%d-bias%d-%s-%s%s' % (shape + (mode, mask, dres, (i // 3) % 2, bias, ('f32', 'bf16')[i % 2]) + views)))
                i += 1
    return cases


@pytest.mark.parametrize('dtype,views,shape,mode,mask,dres,acc_pg,bias', _bwd_cases())
def test_bn_bwd_modes(dtype, views, shape, mode, mask, dres, acc_pg, bias):
    run_bn_bwd(dtype, views, shape + (VARIANTS[views[0]][dtype][1],), mode, mask, dres, acc_pg, bias)


@pytest.mark.parametrize('mode', ['p0', 'p0_acc'])
@pytest.mark.parametrize('views', VIEW_CASES, ids=VIEWS_IDS)
@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_bn_bwd_view_variants(dtype, views, mode):
    C = VARIANTS[views[0]][dtype][1]
    run_bn_bwd(dtype, views, (3, 5, 7, C), mode, 'a', 'fresh', 0, 1, seed=1)
    run_bn_bwd(dtype, views, (2, 4, 8, C), mode, 'a', 'acc', 1, 1, seed=2)


@pytest.mark.parametrize('mode', ['p0', 'p0_ticket', 'p0_acc'])
def test_bn_bwd_two_channel_blocks(mode):
    """C = 301 f32 contiguous -> scalar path, 301 pieces per pixel: the reduction runs a 256-piece block and a 45-piece block (5 rows,
    31 idle threads)."""
    v = (0, 301, 301)
    run_bn_bwd('f32', (v, v), (2, 5, 7, 301), mode, 'a', 'fresh', 0, 1)


@pytest.mark.parametrize('mode,mask,dres', [('p0', 'a', 'acc'), ('p0_acc', 'y', 'none'), ('p3', 'none', 'fresh')])
def test_bn_bwd_apply_grid_stride_loop(mode, mask, dres):
    v = (0, 16, 16)
    run_bn_bwd('f32', (v, v), (2, 192, 192, 16), mode, mask, dres, 0, 0)


@pytest.mark.parametrize('mode', ['p0_acc', 'p3'])
@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_bn_bwd_secondary_sums(dtype, mode):
    v = (0, 32, 32)
    run_bn_bwd(dtype, (v, v), (3, 8, 8, 32), mode, 'a', 'fresh', 0, 0, sec=True)
