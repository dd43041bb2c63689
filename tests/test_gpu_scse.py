"""GPU tests of the scSE kernels (csrc/se.hip: salt_scse, salt_scse_bwd, salt_scse_fc_grads) through the C-ABI against the plain fp64
reference of scse_op_reference.py, on guarded operands: both dtypes, both summation protocols (per-part partials / fp64 atomics), the
input transform with its in-launch BatchNorm finalize, the BatchNorm-backward sums of the layer in front (bnb_acc), the split FC
backward (defer_param_grads + salt_scse_fc_grads), skip_bcast, accumulate, contiguous and channel-slice views - at the smallest shapes
at which each branch of the kernels is live (scse_op_reference.CASES).

Bounds (none of them measured on the kernels).  A float32 torch evaluation of the SAME case sits e32 (largest absolute error over the
tensor) from the float64 reference; every fp32 / fp64 output and every f32 activation may sit at most 4 e32 + 1e-6 max|ref| from it.  A
bf16 activation (y, dx) gets, per element, the storage allowance on top: 2**-8 |ref| - bf16 keeps 8 significant bits, so ONE
round-to-nearest costs up to 2**-8 of the value rounded.  With the broadcast pass (skip_bcast = 0) dx is stored by the first pass, read
back and stored again with dgap added: two roundings, the first of the intermediate value dx - dgap, hence 2**-8 (|ref| + |ref - dgap|)
there (tests/test_scse_cpu.py shows on these very cases that exact arithmetic with the two roundings exceeds 2**-8 |ref| where dgap
cancels part of the direct term - 2341 of the 41344 elements of the ragged case, by up to 82 x - and reaches 0.5 - 1.0 of the sum).  The bnb_acc sums are compared with the float64 sums over the
kernel's OWN stored dx and dgap ("the value salt_bn_bwd will read"), the yardstick being the same sums in float32.

No element is excluded in the plain modes: the case table's seeds keep every hidden pre-activation 100 bands from zero and x free of
zeros, and gate_c + gate_s > 0 makes every ReLU decision of y the sign of the input.  In the transform modes the input the operator
sees is predicted bit for bit from the float32 scale / shift the kernel stored (transform_exact); only float32 elements whose
multiply-add cannot be decided in float64 are dropped, capped at 0.01 % of a tensor (none is expected).

The gates use __expf, exp2 of t log2(e) in float32: the rounding of the product moves the exponent by |t| log2(e) 2**-24, i.e. the
result by |t| 2**-24 relative, and the hardware exp2 adds 1 ulp (2**-23), so e = exp(-t) carries at most (2 + |t|) 2**-24 relative.
The sigmoid 1 / (1 + e) turns a relative error r of e into s (1 - s) r absolute, and s (1 - s) (2 + |t|) <= 0.6 for every t (largest
near |t| = 0.8): under 4e-8 whatever the argument (these cases: |t| < 13), a twenty-fifth of the 1e-6 max|ref| term the gates' bound
already has - no extra allowance is taken."""
import ctypes

import pytest
import torch

import scse_op_reference as SR
from abi_ops import Act, Vec, Frozen, vec_of, raw, call, _abi, code, DEV, F64, NAN
from abi_ops import within as bound_within

pytestmark = pytest.mark.gpu
NAMES = ['one-pixel', 'one-lane', 'ragged-parts', 'whole-wave', 'part-cap', 'strided-fc', 'batch-tiles']
NPARTS = {'ragged-parts': 2, 'part-cap': 16}            # every other case: one part
RATIOS = {}          # {(shape, dtype): {output: worst error / bound}}, the table of DESIGN 22
_CASES = {}
_PLAIN = {}


def case_of(name, dtype):
    key = (name, dtype)
    if key not in _CASES:
        _CASES[key] = SR.make_case(*SR.CASES[name][dtype], SR.SEEDS[key], dtype)
    return _CASES[key]


def references(c, a, mode, skip, accumulate, cache=None):
    """float64 reference and float32 yardstick of forward and backward for input ``a`` - computed once per plain case and shared"""
    key = (cache, skip, accumulate)
    if cache is not None and key in _PLAIN:
        return _PLAIN[key]
    out = []
    for dt in (F64, torch.float32):
        p = SR.params(c, mode, dt)
        f = SR.scse(a.to(dt), *p)
        b = SR.scse_bwd(f, c['dy'].to(dt), a.to(dt), p[0], p[2], p[4], skip_bcast=bool(skip), dx_old=c['dx_old'].to(dt) if accumulate else None)
        out.append((f, b))
    if cache is not None:
        _PLAIN[key] = out
    return out


def fc_tiles(B, C, R):
    """launch_se_fc's rule (csrc/se.hip): images per tile of the single-workgroup FC backward"""
    img, w = (3 * C + 2 * R + 1) * 4, 2 * R * C * 4
    return B if img * B <= 160 * 1024 else (160 * 1024 - w) // img


def within(got, ref64, ev32, what, case, key, allowance=None, keep=None):
    """the module docstring's bound (abi_ops.within), recorded in RATIOS"""
    bound_within(got, ref64, ev32, what, RATIOS, case, key, allowance, keep)


def split_shards(S, Q, N, C, g):
    """[8][2 C + 1] fp64: the true (sum, sum of squares, count), split unevenly over the eight shards (two of them empty)"""
    frac = torch.rand(8, generator=g, dtype=F64) + 0.05
    frac[2], frac[5] = 0.0, 0.0
    frac = frac / frac.sum()
    sh = torch.zeros(8, 2 * C + 1, dtype=F64)
    sh[:, :C], sh[:, C:2 * C] = frac[:, None] * S, frac[:, None] * Q
    cnt = torch.floor(frac * N)
    sh[:, 2 * C] = cnt
    sh[7, :C] += S - sh[:, :C].sum(0)
    sh[7, C:2 * C] += Q - sh[:, C:2 * C].sum(0)
    sh[7, 2 * C] += N - float(cnt.sum())
    return sh


def run(name, dtype, sliced, fwd_acc, fin, bwd_acc, defer, skip, accumulate, bnb):
    """One forward + backward of one case in one combination of the operator's modes; returns every output for the determinism test.
    fin: None (x is the operator's input), or the in_relu of the input transform (x is the raw output of the layer in front)."""
    abi = _abi()
    B, H, W, C, R = shape = SR.CASES[name][dtype]
    hw, case = H * W, (SR.CASES[name][dtype], dtype)
    c = case_of(name, dtype)
    mode = 'plain' if fin is None else 'fin%d' % fin
    what = 'scse %s %s sliced=%d fwd_acc=%d fin=%s bwd_acc=%d defer=%d skip=%d acc=%d bnb=%d' % (shape, dtype, sliced, fwd_acc, fin, bwd_acc, defer, skip, accumulate, bnb)
    g = torch.Generator().manual_seed(B * 1000 + C)
    P = {k: t.float().contiguous().to(DEV) for k, t in zip(('w1', 'b1', 'w2', 'b2', 'ws', 'bs'), SR.params(c, mode))}
    x = Act(c['x'] if fin is None else c['x_raw'], dtype, sliced)
    y = Act(torch.full((B, H, W, C), NAN, dtype=F64), dtype, sliced)
    nparts = abi.lib.salt_scse_parts(ctypes.byref(abi.fill(abi.STRUCTS['salt_scse_args'](), x=x.view)))
    assert nparts == NPARTS.get(name, 1) and (fc_tiles(B, C, R) < B) == (name == 'batch-tiles')
    gap, hid, gc, gs = Vec(B * C), Vec(B * R), Vec(B * C), Vec(B * hw)
    parts = Vec(B * nparts * C)
    gacc = Vec(B * C, fill=0.0, dtype=F64) if fwd_acc else None
    kw = dict(dtype=code(dtype), x=x.view, R=R, gap_partials=parts.ptr(), nparts=nparts, gap=gap.ptr(), hidden=hid.ptr(), gate_c=gc.ptr(), gate_s=gs.ptr(),
              y=y.view, gap_acc=gacc.ptr() if gacc else None, **{k: t.data_ptr() for k, t in P.items()})
    frozen = Frozen(x=x.buf, **P)
    if fin is not None:
        S, Q, N = SR.stats64(c['x_raw'])
        shards = vec_of(split_shards(S, Q, N, C, g), F64)
        gamma, beta = c['gamma'].float().to(DEV), c['beta'].float().to(DEV)
        rmean, rvar = vec_of(c['running_mean']), vec_of(c['running_var'])
        nbt = torch.tensor([-7, 41, -7], dtype=torch.int64, device=DEV)
        mean, invstd, scale, shift = Vec(C), Vec(C), Vec(C), Vec(C)
        Fbn = abi.fill(abi.STRUCTS['salt_bn_finalize_args'](), C=C, gamma=gamma.data_ptr(), beta=beta.data_ptr(), running_mean=rmean.ptr(), running_var=rvar.ptr(),
                       num_batches_tracked=nbt.data_ptr() + 8, momentum=SR.MOMENTUM, eps=SR.EPS, mean=mean.ptr(), invstd=invstd.ptr(), scale=scale.ptr(), shift=shift.ptr())
        kw.update(in_fin=ctypes.addressof(Fbn), in_fin_acc=shards.ptr(), in_relu=fin)
        frozen = Frozen(x=x.buf, shards=shards.buf, gamma=gamma, beta=beta, **P)
    call('salt_scse', **kw)
    frozen.check(what + ' forward')
    y.check(what + ' y')
    if fwd_acc:
        assert bool(torch.isnan(parts.get((-1,))).all()), what + ': the partials workspace was touched on the gap_acc path'
    keep = None
    if fin is None:
        a = c['x']
    else:
        # the finalize against bn_finalize64; the yardstick is the same arithmetic from float32 sums
        run64 = (c['running_mean'], c['running_var'])
        f64 = SR.bn_finalize64(S, Q, N, c['gamma'], c['beta'], SR.EPS, SR.MOMENTUM, run64)
        f32 = SR.bn_finalize64(S.float(), Q.float(), N, c['gamma'].float(), c['beta'].float(), SR.EPS, SR.MOMENTUM, [t.float() for t in run64])
        got = dict(mean=mean.get((C,)), invstd=invstd.get((C,)), scale=scale.get((C,)), shift=shift.get((C,)), running_mean=rmean.get((C,)), running_var=rvar.get((C,)))
        for k, v in got.items():
            within(v, getattr(f64, k), getattr(f32, k), what, case, 'fin.' + k)
        assert nbt.tolist() == [-7, 42, -7], what + ': num_batches_tracked'
        seen = SR.transform_exact(c['x_raw'], got['scale'].float(), got['shift'].float(), fin, dtype)
        a, dropped = seen.a, int(seen.doubtful.sum())
        assert dropped <= 1e-4 * a.numel(), '%s: %d elements of the transform undecided' % (what, dropped)
        keep = ~seen.doubtful if dropped else None
        lo, band = SR.hidden_band(a, SR.params(c, mode))
        assert lo >= 10 * band, '%s: a hidden pre-activation of the REFERENCE lies %.1f bands from zero' % (what, lo / band)
    (f64, b64), (f32, b32) = references(c, a, mode, skip, accumulate, cache=(name, dtype) if fin is None else None)
    fwd = dict(gap=gap.get((B, C)), hidden=hid.get((B, R)), gate_c=gc.get((B, C)), gate_s=gs.get((B, H, W)), y=y.get())
    for k in ('gap', 'hidden', 'gate_c', 'gate_s'):
        within(fwd[k], getattr(f64, k), getattr(f32, k), what, case, k)
    assert bool(((fwd['hidden'] > 0) == (f64.hidden > 0)).all()), what + ': hidden ReLU decisions'
    bf = dtype == 'bf16'
    within(fwd['y'], f64.y, f32.y, what, case, 'y', SR.storage_allowance(f64.y) if bf else None, keep)
    decided = (fwd['y'] > 0) == (a > 0)
    assert bool((decided if keep is None else decided[keep]).all()), what + ': ReLU decisions of y'

    # ---- backward
    dy = Act(c['dy'], dtype, sliced)
    dx = Act(c['dx_old'] if accumulate else torch.full((B, H, W, C), NAN, dtype=F64), dtype, sliced)
    AW = (6 if bnb else 2) * C + 1
    bparts = Vec(B * nparts * (2 * C + 1))
    acc = Vec(B * AW, fill=0.0, dtype=F64) if bwd_acc else None
    bnb_acc = Vec(8 * 2 * C, fill=0.0, dtype=F64) if bnb else None
    G = dict(g_w1=Vec(R * C), g_b1=Vec(R), g_w2=Vec(C * R), g_b2=Vec(C), g_ws=Vec(C), g_bs=Vec(1))
    gshape = dict(g_w1=(R, C), g_b1=(R,), g_w2=(C, R), g_b2=(C,), g_ws=(C,), g_bs=(1,))
    dgap = Vec(B * C)
    bkw = dict(dtype=code(dtype), x=x.view, y=y.view, dy=dy.view, w1=P['w1'].data_ptr(), w2=P['w2'].data_ptr(), R=R, ws=P['ws'].data_ptr(), gap=gap.ptr(),
               hidden=hid.ptr(), gate_c=gc.ptr(), gate_s=gs.ptr(), partials=bparts.ptr(), nparts=nparts, dgap=dgap.ptr(), dx=dx.view, accumulate=accumulate,
               acc=acc.ptr() if acc else None, skip_bcast=skip, defer_param_grads=defer, **{k: v.ptr() for k, v in G.items()})
    inputs = dict(x=x.buf, y=y.buf, dy=dy.buf, gap=gap.buf, hidden=hid.buf, gate_c=gc.buf, gate_s=gs.buf, **P)
    if fin is not None:
        bkw.update(in_scale=scale.ptr(), in_shift=shift.ptr(), in_relu=fin)
        inputs.update(scale=scale.buf, shift=shift.buf, mean=mean.buf, invstd=invstd.buf)
    if bnb:
        bkw.update(bn_mean=mean.ptr(), bn_invstd=invstd.ptr(), bnb_acc=bnb_acc.ptr())
    frozen = Frozen(**inputs)
    call('salt_scse_bwd', **bkw)
    if defer:
        # the critical half alone: dgap, dx (and the sums) final, no parameter gradient written; then the deferred half changes neither
        for k, v in G.items():
            assert bool(torch.isnan(v.get(gshape[k])).all()), '%s: defer_param_grads wrote %s' % (what, k)
        first = Frozen(dx=dx.buf, dgap=dgap.buf, **({'bnb_acc': bnb_acc.buf} if bnb else {}))
        assert bool(torch.isfinite(dgap.get((B, C))).all()) and bool(torch.isfinite(dx.get()).all())
        call('salt_scse_fc_grads', **bkw)
        first.check(what + ' salt_scse_fc_grads')
    frozen.check(what + ' backward')
    dx.check(what + ' dx')
    if bwd_acc:
        assert bool(torch.isnan(bparts.get((-1,))).all()), what + ': the partials workspace was touched on the acc path'
    out = dict(fwd, dx=dx.get(), dgap=dgap.get((B, C)), **{k: v.get(gshape[k]) for k, v in G.items()})
    within(out['dgap'], b64['dgap'], b32['dgap'], what, case, 'dgap')
    for k in G:
        within(out[k], b64[k], b32[k], what, case, k)
    allowance = None
    if bf:
        allowance = SR.storage_allowance(b64['dx'], None if skip else b64['dx'] - b64['dgap'][:, None, None, :])
    within(out['dx'], b64['dx'], b32['dx'], what, case, 'dx' if skip else 'dx+dgap', allowance, keep)
    if bnb:
        # the sums salt_bn_bwd will read, over the kernel's own stored dx and dgap; with defer spread over the shards by image
        on = (seen.pre > 0) if fin else None
        want = []
        for dt in (F64, torch.float32):
            i1, i2 = SR.bnb_sums(c['x_raw'].to(dt), on, out['dx'].to(dt), out['dgap'].to(dt), got['mean'].to(dt), got['invstd'].to(dt), per_image=True)
            w = torch.zeros(8, 2, C, dtype=dt)
            for b in range(B):
                s = (b & 7) if defer else 0
                w[s, 0] += i1[b]
                w[s, 1] += i2[b]
            want.append(w)
        sums = bnb_acc.get((8, 2, C))
        out['bnb'] = sums
        within(sums, want[0], want[1], what, case, 'bnb shards')
        within(sums.sum(0), want[0].sum(0), want[1].sum(0), what, case, 'bnb sums')
        if not defer:
            assert bool((sums[1:] == 0).all()), what + ': a shard other than 0 was written without defer_param_grads'
        else:
            assert bool((sums[min(B, 8):] == 0).all()), what + ': a shard no image maps to was written'
    return out


MODES = {
    # name: [(sliced, fwd_acc, fin, bwd_acc, defer, skip, accumulate, bnb)]
    'partials': [(0, 0, None, 0, 0, 0, 0, 0), (1, 0, None, 0, 0, 0, 1, 0)],
    'atomics': [(1, 1, None, 1, 0, 1, 0, 0)],
    'deferred': [(0, 1, None, 1, 1, 0, 0, 0), (1, 1, None, 1, 1, 1, 0, 0)],
    'transform': [(0, 1, 0, 1, 1, 1, 0, 0), (1, 1, 1, 1, 1, 1, 0, 0)],
    'bnb': [(0, 1, 1, 1, 0, 1, 0, 1), (1, 1, 1, 1, 1, 1, 0, 1), (1, 1, 0, 1, 0, 1, 0, 1), (0, 1, 0, 1, 1, 1, 0, 1)],
}


@pytest.mark.parametrize('mode', list(MODES))
@pytest.mark.parametrize('name', NAMES)
@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_scse_vs_fp64_reference(dtype, name, mode):
    for args in MODES[mode]:
        run(name, dtype, *args)
    case = (SR.CASES[name][dtype], dtype)
    print('RATIOS %s %s after %s:' % (case[0], dtype, mode), {k: round(v, 3) for k, v in sorted(RATIOS[case].items())})


@pytest.mark.parametrize('name', ['ragged-parts', 'part-cap'])
@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_partials_protocol_is_bit_identical_between_runs(dtype, name):
    """per-part partials summed in a fixed order: two runs give the same bits in every output"""
    a = run(name, dtype, *MODES['partials'][1])
    b = run(name, dtype, *MODES['partials'][1])
    assert set(a) == set(b) and len(a) >= 13
    for k in a:
        assert torch.equal(a[k], b[k]), (name, dtype, k)


def test_refusals_come_from_host_code_and_launch_nothing():
    """every one of these is rejected before any launch (csrc/se.hip: the checks ahead of the first salt_launch): an error code, a reason
    in salt_last_error, every output still NaN"""
    abi = _abi()
    from salt_amd.engine import shaped_view
    UNS, BAD = abi.CONSTS['SALT_E_UNSUPPORTED'], abi.CONSTS['SALT_E_BADARG']

    def attempt(op, want, reason, C=16, dtype='f32', cs=None, off=0, **over):
        B, H, W, R = 2, 2, 3, 2
        el = 2 if dtype == 'bf16' else 4
        cs = C if cs is None else cs
        mk = lambda fill: torch.full((B * H * W * cs + 64,), fill, dtype=torch.float32 if el == 4 else torch.bfloat16, device=DEV)
        x, yv, dy, dx = mk(0.5), mk(NAN), mk(0.25), mk(NAN)
        view = lambda t, o=0: shaped_view(t.data_ptr() + o, B, H, W, C, cs)
        P = {k: torch.full((n,), 0.1, device=DEV) for k, n in (('w1', R * C), ('b1', R), ('w2', C * R), ('b2', C), ('ws', C), ('bs', 1))}
        outs = {k: torch.full((n,), NAN, device=DEV) for k, n in (('gap', B * C), ('hidden', B * R), ('gate_c', B * C), ('gate_s', B * H * W), ('dgap', B * C),
                                                                  ('g_w1', R * C), ('g_b1', R), ('g_w2', C * R), ('g_b2', C), ('g_ws', C), ('g_bs', 1))}
        work = torch.full((B * (2 * C + 1),), NAN, device=DEV)
        acc = torch.zeros(B * (6 * C + 1) + 16 * C, dtype=F64, device=DEV)
        if op == 'salt_scse':
            kw = dict(dtype=code(dtype), x=view(x, off), R=R, gap_partials=work.data_ptr(), nparts=1, y=view(yv), **{k: t.data_ptr() for k, t in P.items()},
                      **{k: outs[k].data_ptr() for k in ('gap', 'hidden', 'gate_c', 'gate_s')})
        else:
            kw = dict(dtype=code(dtype), x=view(x, off), y=view(x), dy=view(dy), dx=view(dx), R=R, partials=work.data_ptr(), nparts=1, w1=P['w1'].data_ptr(),
                      w2=P['w2'].data_ptr(), ws=P['ws'].data_ptr(), **{k: t.data_ptr() for k, t in outs.items()})
        for k, v in over.items():
            kw[k] = acc.data_ptr() + 8 * v if k in ('acc', 'bnb_acc', 'gap_acc', 'in_fin_acc') and v is not None else v
        rc = raw(op, **kw)
        msg = abi.lib.salt_last_error().decode()
        touched = [k for k, t in list(outs.items()) + [('y', yv), ('dx', dx), ('work', work)] if not bool(torch.isnan(t.float()).all())]
        assert rc == want and reason in msg and not touched and float(acc.abs().max()) == 0, (op, over, rc, msg, touched)

    C = 16
    fbn = abi.STRUCTS['salt_bn_finalize_args']()
    attempt('salt_scse', BAD, 'nparts', nparts=2)
    attempt('salt_scse_bwd', BAD, 'nparts', nparts=3)
    attempt('salt_scse', UNS, 'power of two', C=24)
    attempt('salt_scse_bwd', UNS, 'layout', C=24)
    attempt('salt_scse', UNS, 'power of two', C=24, dtype='bf16')
    attempt('salt_scse', UNS, 'power of two', C=1024, dtype='bf16')
    attempt('salt_scse_bwd', UNS, 'layout', C=1024, dtype='bf16')
    attempt('salt_scse', UNS, 'power of two', cs=C + 2)
    attempt('salt_scse', UNS, 'power of two', cs=C + 4, dtype='bf16')
    attempt('salt_scse_bwd', UNS, 'layout', cs=C + 2)
    attempt('salt_scse', UNS, 'power of two', off=4)
    attempt('salt_scse_bwd', UNS, 'layout', off=8, dtype='bf16')
    attempt('salt_scse', BAD, 'in_fin needs gap_acc', in_fin=ctypes.addressof(fbn), in_fin_acc=0)
    p = torch.zeros(4 * C, device=DEV)
    tr = dict(in_scale=p.data_ptr(), in_shift=p.data_ptr() + 4 * C, bn_mean=p.data_ptr() + 8 * C, bn_invstd=p.data_ptr() + 12 * C)
    attempt('salt_scse_bwd', BAD, 'bnb_acc needs', acc=0, bnb_acc=2 * (6 * C + 1), skip_bcast=0, **tr)
    attempt('salt_scse_bwd', BAD, 'defer_param_grads needs', defer_param_grads=1)
    attempt('salt_scse_fc_grads', BAD, 'scse_fc_grads: bad args')


def test_ratio_table():
    """prints the worst error / bound per output and per (shape, dtype) of this session (DESIGN 22 holds the table of a full run)"""
    for case in sorted(RATIOS, key=str):
        print('RATIOS', case, {k: round(v, 3) for k, v in sorted(RATIOS[case].items())})
    assert all(v <= 1.0 for per in RATIOS.values() for v in per.values())
