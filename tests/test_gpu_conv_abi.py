"""salt_conv (forward convolutions, transposed-convolution phases, data gradients) per kernel through the C-ABI: every case names the
kernel it is meant for (`kid`: salt_conv_kernel_id, 1-5 conv_mfma_kernel tile configs, 6-8 conv_glds_kernel, 9 conv_ws_kernel, 10
conv_ls_kernel, 12 conv_thin_kernel, 13 conv_stem16_kernel), some the loader instantiation (`regime`) or the general tile (`gen`),
and is held ELEMENTWISE to the float64 reference of conv_abi.py with the bound derived there (max err / tol <= 1).  Outputs are
guard-prefilled: everything outside the written region (gap channels of a view, the other output parities, pixels outside the grid)
must keep its bit pattern; gap channels of the input views hold NaN, so a stray read shows as well.

ReLU is 1-Lipschitz, so the value bound holds through it whatever the sign decision; only the BatchNorm-backward masks need
pre-activations kept away from zero (op_reference.avoid_zero_crossings).

The table and build() live in conv_abi.py, importable without a GPU: test_conv_reference_cpu.py runs an fp32 stand-in over the same
cases."""
import pytest
import torch

import conv_abi as CA
from conv_abi import BM, CASES, K3, K3R, STEM, _vec, build, case


def _view(c, which):
    c0, cs = c[which]
    return c0, (c['Cin'] if which == 'xv' else c['Cout']), cs


def plan_args(c, x_ptr=1 << 20, y_ptr=1 << 24, extra=None):
    """salt_conv_args of a case on made-up 16-byte aligned addresses (+ the views' channel offsets): the planner reads no memory."""
    from salt_amd.engine import shaped_view
    es = 2 if c['dtype'] == 'bf16' else 4
    xc0, Cin, xcs = _view(c, 'xv')
    yc0, Cout, ycs = _view(c, 'yv')
    f = dict(in_step=c['in_step'], pad_mode=c['pad_mode'], out_step=c['out_step'], out_oy=c['out_oy'], out_ox=c['out_ox'], relu=int(c['relu']),
             accumulate=int(c['acc']), cfg=c['cfg'])
    for k in ('bias', 'scale', 'shift'):
        if c[k]:
            f[k] = 1 << 28
    if c['fold']:
        f.update(fold_top=c['fold'][1], fold_right=c['fold'][2])
        if c['fold'][0] == 'strip':
            f.update(strip=1 << 29, strip_cs=_round_up(Cout, 8))
    if c['in_tf']:
        f.update(in_scale=1 << 26, in_shift=(1 << 26) + 4096, in_relu=int(c['in_tf'] == 'relu'))
    f.update(extra or {})
    S = CA.conv_args(c['dtype'], shaped_view(x_ptr + xc0 * es, c['B'], c['H'], c['W'], Cin, xcs), 1 << 27, [(t[2], t[3]) for t in c['taps']],
                     shaped_view(y_ptr + yc0 * es, c['B'], c['yH'], c['yW'], Cout, ycs), c['OH'], c['OW'], **f)
    if c['res']:
        S.res = shaped_view(1 << 30, c['B'], c['yH'], c['yW'], Cout, Cout)
    return S


def _round_up(a, b):
    return (a + b - 1) // b * b


def regime(c, kid, tile):
    """The conv_mfma_kernel instantiation launch_cfg picks: 'ilv9-3' / 'ilv9-9' / 'ilv9-6' / 'ilv4' (interleaved loader, MAXA_T) or
    'nt9' / 'nt4' / 'nt0' (register-staged generic loader, tap count known at compile time or not)."""
    tw, th, nb, _ = tile
    dys, dxs = [t[2] for t in c['taps']], [t[3] for t in c['taps']]
    s = c['in_step']
    hh, hw = (th - 1) * s + max(dys) - min(dys) + 1, (tw - 1) * s + max(dxs) - min(dxs) + 1
    kce = 32 if c['dtype'] == 'bf16' else 16
    vt = 4 if len(c['taps']) == 1 and s == 1 and c['Cin'] % (4 * kce) == 0 else 1
    npa = -(-nb * hh * hw * vt * 4 // 256)
    nt = vt if vt > 1 else len(c['taps'])
    xc0, Cin, xcs = _view(c, 'xv')
    ok = c['dtype'] == 'bf16' and BM[kid] != 64 and xcs % 8 == 0 and Cin % 8 == 0 and (xc0 * 2) % 16 == 0
    if ok and nt == 9:
        if BM[kid] == 256:
            if npa <= 6:
                return 'ilv9-6'
        else:
            return 'ilv9-3' if npa <= 3 else 'ilv9-9'
    if ok and nt == 4 and BM[kid] != 256:
        return 'ilv4'
    return 'nt%d' % (nt if nt in (9, 4) else 0)


def test_cases_land_on_the_kernel_they_name():
    """Host only (no launch): the plan of every case, before any of them runs - kernel id, general tile and loader regime."""
    names = set()
    for p in CASES:
        c = p.values[0]
        assert c['name'] not in names, c['name']
        names.add(c['name'])
        S = plan_args(c)
        kid = CA.conv_kernel_id(S)
        assert kid == c['kid'], '%s: the plan runs kernel %d (%s)' % (c['name'], kid, CA.last_error() if kid < 0 else 'ok')
        if kid <= 8:
            tile = CA.tile_shape(S)
            assert tile is not None
            if c['gen'] is not None:
                assert tile[3] == c['gen'], '%s: tile %r' % (c['name'], tile)
            if kid <= 5 and c['regime'] is not None:
                assert regime(c, kid, tile) == c['regime'], '%s: %s, tile %r' % (c['name'], regime(c, kid, tile), tile)


def test_glds_refuses_4x4_maps():
    """A 128-pixel tile of 4 x 4 maps is 8 images, each with its own halo ring: asked for by id, conv_glds_kernel refuses."""
    for kid in (6, 7, 8):
        c = case('x', kid, 'bf16', 16, 64, 64, 4, 4, K3).values[0]
        S = plan_args(c)
        assert CA.conv_kernel_id(S) == -1
        assert 'too large for the LDS ring' in CA.last_error()


def _written(c, buf_shape):
    yc0, Cout, _ = _view(c, 'yv')
    m = torch.zeros(buf_shape, dtype=torch.bool)
    if c['fold']:
        m[..., yc0:yc0 + Cout] = True
    else:
        s = c['out_step']
        m[:, c['out_oy']::s, c['out_ox']::s][:, :c['OH'], :c['OW'], yc0:yc0 + Cout] = True
    return m


def run_case(c, o, setup=None):
    """Launch a case -> (values of the written region [B, gH, gW, Cout] float64, the strip or None).  setup(S, dev, keep) sets further
    fields of the arguments before the plan is asked."""
    dev = 'cuda:0'
    dt = c['dtype']
    B, Cout = c['B'], c['Cout']
    X = CA.Placed((B, c['H'], c['W']), _view(c, 'xv'), dt, dev, o['x'])
    Y = CA.Placed((B, c['yH'], c['yW']), _view(c, 'yv'), dt, dev)
    m = _written(c, Y.buf.shape)
    if c['acc']:
        tmp = Y.buf.cpu()
        tmp[m] = o['old'].to(tmp.dtype).reshape(-1)
        Y.buf.copy_(tmp)
    before = Y.buf.cpu().clone()
    wp = CA.pack(o['w'].to(dev), dt, o['tap_k'], c['transpose'])
    extra = {}
    keep = [wp]
    for k in ('bias', 'scale', 'shift'):
        if c[k]:
            keep.append(o[k].float().to(dev))
            extra[k] = keep[-1].data_ptr()
    strip = None
    if c['fold'] and c['fold'][0] == 'strip':
        from salt_amd._abi import lib
        ring = lib.salt_fold_strip_pixels(c['yH'], c['yW'], c['fold'][1], 0, 0, c['fold'][2])
        strip = CA.guard_fill(torch.empty(B, ring, _round_up(Cout, 8), dtype=Y.buf.dtype, device=dev))
        extra.update(strip=strip.data_ptr(), strip_cs=strip.shape[2])
    S = plan_args(c, X.buf.data_ptr(), Y.buf.data_ptr(), extra)
    S.w = wp.data_ptr()
    if c['res']:
        R = CA.Placed((B, c['yH'], c['yW']), (0, Cout, Cout), dt, dev, o['res'])
        S.res = R.view
    if c['in_tf']:
        keep += [o['in_tf'][0].float().to(dev), o['in_tf'][1].float().to(dev)]
        S.in_scale, S.in_shift, S.in_relu = keep[-2].data_ptr(), keep[-1].data_ptr(), int(o['in_tf'][2])
    if setup is not None:
        setup(S, dev, keep)
    kid = CA.conv_kernel_id(S)
    assert kid == c['kid'], 'the plan runs kernel %d, this case is meant for %d (%s)' % (kid, c['kid'], CA.last_error() if kid < 0 else '')
    out = CA.conv_hip(S, Y.buf)
    assert torch.equal(CA.bits(out)[~m], CA.bits(before)[~m]), 'elements outside the written region changed'
    gH, gW = (c['yH'], c['yW']) if c['fold'] else (c['OH'], c['OW'])
    got = out[m].reshape(B, gH, gW, Cout).double()
    return got, (None if strip is None else strip.cpu())


@pytest.mark.gpu
@pytest.mark.parametrize('c', CASES)
def test_conv_kernel_vs_float64(c):
    o = build(c)
    got, strip = run_case(c, o)
    assert torch.isfinite(got).all()
    ref = o['ref']
    if strip is None:
        r = CA.ratio(got, ref)
    else:
        # strip mode: the interior of the extended grid in y, the ring in strip order
        from op_reference import ring_from_padded
        top, right = c['fold'][1], c['fold'][2]
        inner = {k: ref[k][:, top:, :c['yW']] for k in ('exact', 'tol')}
        ring = {k: ring_from_padded(ref[k], top, 0, 0, right) for k in ('exact', 'tol')}
        got_ring = strip[:, :, :c['Cout']].double()
        assert torch.isfinite(got_ring).all()
        assert bool((CA.bits(strip[:, :, c['Cout']:]) == CA.GUARD[strip.dtype]).all())
        r = max(CA.ratio(got, inner), CA.ratio(got_ring, ring))
    print('kernel %d %s max err / tol = %.3f' % (c['kid'], c['dtype'], r))
    assert r <= 1.0, 'max err / tol = %.3f' % r


@pytest.mark.gpu
@pytest.mark.parametrize('K', [3, 5])
@pytest.mark.parametrize('dt,kid', [('f32', 1), ('f32', 4), ('bf16', 1), ('bf16', 4), ('bf16', 5)])
def test_phase_fused_dgrad_equals_reference_and_four_launches(dt, kid, K):
    """The nphase = 4 single-launch form of a stride-2 data gradient (unified offsets, zero taps, one packed block per phase at
    w_phase_elems) against the reference, and bit for bit against four out_step = 2 launches on the same kernel id.  K = 3: the
    form the graph builder emits (1, 2, 2 and 4 real taps over 4 unified offsets); K = 5: 9 unified offsets."""
    dev = 'cuda:0'
    B, Ci, Co, H, W = 2, 24, 40, 10, 12                                     # gradient of conv(24 -> 40, K, s2) over a 10 x 12 input
    phases = CA.dgrad_s2_phases(CA.kk_taps(K))
    offs, rows = CA.unify_phases(phases)
    assert len(offs) == (4 if K == 3 else 9)
    dy = CA.mk(B, Co, H // 2, W // 2, 31).permute(0, 2, 3, 1).contiguous()
    w = CA.master_weight(Co, Ci, K, K, Co, len(offs), 32)
    X = CA.Placed((B, H // 2, W // 2), (0, Co, Co), dt, dev, dy)
    outs = []
    for fused in (True, False):
        Y = CA.Placed((B, H, W), (8, Ci, 40), dt, dev)
        if fused:
            wp, elems = CA.pack_phases(w.to(dev), dt, rows, 1)
            S = CA.conv_args(dt, X.view, wp.data_ptr(), offs, Y.view, H // 2, W // 2, out_step=2, nphase=4, w_phase_elems=elems, cfg=kid)
            assert CA.conv_kernel_id(S) == kid
            out = CA.conv_hip(S, Y.buf)
        else:
            for (ay, ax, sel), row in zip(phases, rows):
                wp = CA.pack(w.to(dev), dt, row, 1)                         # the same offsets and zero taps: the same MFMA sequence
                S = CA.conv_args(dt, X.view, wp.data_ptr(), offs, Y.view, H // 2, W // 2, out_step=2, out_oy=ay, out_ox=ax, cfg=kid)
                assert CA.conv_kernel_id(S) == kid
                out = CA.conv_hip(S, Y.buf)
        Y.check('phase-fused dgrad' if fused else 'four launches')
        outs.append(out[..., 8:8 + Ci])
    assert torch.equal(CA.bits(outs[0]), CA.bits(outs[1]))
    worst = 0.0
    for (ay, ax, sel), row in zip(phases, rows):
        ref = CA.conv_ref(dy, CA.tap_weights(w, row, 1), offs, 1, 0, H // 2, W // 2, dt)      # K counts the zero taps: A does not
        got = outs[0][:, ay::2, ax::2].double()
        assert torch.isfinite(got).all()
        worst = max(worst, CA.ratio(got, ref))
    print('kernel %d %s max err / tol = %.3f' % (kid, dt, worst))
    assert worst <= 1.0, worst


# ---------------------------------------------------------------- statistics of the stored values
def _lib():
    from salt_amd._abi import lib
    return lib


def _byref(S):
    import ctypes
    return ctypes.byref(S)


def C_(name, kid, dt, B, Cin, Cout, H, W, taps, **kw):
    return case(name, kid, dt, B, Cin, Cout, H, W, taps, **kw).values[0]


EPI = dict(bias=True, scale=True, shift=True, relu=True)
STATS_CASES = [pytest.param(c, id=c['name']) for c in [
    C_('f32-cfg1-ragged', 1, 'f32', 3, 13, 10, 7, 5, K3), C_('bf16-cfg1-ragged', 1, 'bf16', 3, 13, 10, 7, 5, K3),
    C_('f32-cfg4-epilogue', 4, 'f32', 2, 24, 37, 9, 11, K3, **EPI), C_('bf16-cfg4-epilogue', 4, 'bf16', 2, 24, 37, 9, 11, K3, **EPI),
    C_('f32-cfg5-b5', 5, 'f32', 5, 24, 40, 8, 8, K3R, pad_mode=1), C_('bf16-cfg5-b5', 5, 'bf16', 5, 24, 40, 8, 8, K3R, pad_mode=1),
    C_('bf16-cfg2-33x17', 2, 'bf16', 2, 40, 72, 33, 17, K3), C_('f32-cfg3-33x17', 3, 'f32', 2, 40, 72, 33, 17, K3),
    C_('bf16-glds7-17x9', 7, 'bf16', 2, 64, 40, 17, 9, K3), C_('bf16-glds6-33x17', 6, 'bf16', 2, 32, 72, 33, 17, K3, bias=True),
    C_('bf16-glds8-17x9', 8, 'bf16', 2, 96, 40, 17, 9, K3R, pad_mode=1),
]]
# the fp64 shards without a ticket: every kernel that has them
SHARD_CASES = STATS_CASES + [pytest.param(c, id=c['name']) for c in [
    C_('ws-64-64', 9, 'bf16', 2, 64, 64, 16, 32, K3, cfg=9 | (1 << 8)), C_('ws-32-64-epilogue', 9, 'bf16', 2, 32, 64, 16, 16, K3R, pad_mode=1, **EPI),
    C_('ls-64-32', 10, 'bf16', 2, 64, 32, 16, 16, K3, cfg=10 | (1 << 8)), C_('ls-128-64-ni2', 10, 'bf16', 2, 128, 64, 16, 32, K3, cfg=10 | (2 << 16), bias=True),
    C_('thin-16-32-zero', 12, 'f32', 2, 16, 32, 16, 16, K3), C_('thin-32-16-replicate', 12, 'f32', 3, 32, 16, 16, 32, K3R, pad_mode=1, **EPI),
    C_('thin-32-32', 12, 'f32', 2, 32, 32, 16, 16, K3), C_('thin-16-16', 12, 'f32', 2, 16, 16, 16, 16, K3R, pad_mode=1),
    C_('stem16', 13, 'bf16', 2, 16, 64, 16, 16, STEM), C_('stem16-epilogue', 13, 'bf16', 1, 16, 64, 16, 32, STEM, **EPI),
]]


def _check_moments(what, got, dtype, n, s, q):
    """n, s [C], q [C]: count, sum and sum of squares a launch reported, against the float64 moments of the values it stored."""
    y = got.reshape(-1, got.shape[-1])
    assert n == y.shape[0], '%s: count %r for %d pixels' % (what, n, y.shape[0])
    rs, rq, ts, tq = CA.moments(y, dtype)
    r1, r2 = float(((s - rs).abs() / ts).max()), float(((q - rq).abs() / tq).max())
    print('%s: sum at %.3f, sum of squares at %.3f of the bound' % (what, r1, r2))
    assert r1 <= 1.0 and r2 <= 1.0, '%s: sum at %.3f, sum of squares at %.3f of the bound' % (what, r1, r2)


def _merge(partials, counts):
    """[nparts][2][C] (sum, M2 about the partial's own mean), [nparts] -> (N, sum, sum of squares), exact in float64."""
    n = float(counts.sum())
    s = partials[:, 0].sum(0)
    m2 = torch.zeros_like(s)
    for k in range(partials.shape[0]):
        if counts[k] > 0:
            m2 = m2 + partials[k, 1] + counts[k] * (partials[k, 0] / counts[k] - s / n) ** 2
    return n, s, m2 + s * s / n


@pytest.mark.gpu
@pytest.mark.parametrize('c', STATS_CASES)
def test_stats_partials_are_the_moments_of_the_stored_output(c):
    """stats / stats_cnt: per-tile (sum, M2 about the tile's mean, count), merged here in float64 (Chan): the counts sum exactly to the
    pixel count, the merged sum and sum of squares match the stored output within one storage rounding per element (conv_abi.moments:
    M2 + S^2 / N is the sum of squares)."""
    lib = _lib()
    o, st = build(c), {}

    def setup(S, dev, keep):
        n = lib.salt_conv_stats_parts(_byref(S))
        assert n >= 1
        st['n'] = n
        st['stats'] = torch.full((lib.salt_bn_stats_floats(n, c['Cout']),), float('nan'), device=dev)
        st['cnt'] = torch.full((n,), float('nan'), device=dev)
        S.stats, S.stats_cnt = st['stats'].data_ptr(), st['cnt'].data_ptr()
    got, _ = run_case(c, o, setup)
    assert CA.ratio(got, o['ref']) <= 1.0
    parts = st['stats'][:st['n'] * 2 * c['Cout']].reshape(st['n'], 2, c['Cout']).double().cpu()
    cnt = st['cnt'].double().cpu()
    assert torch.isfinite(parts).all() and torch.isfinite(cnt).all()
    assert bool((parts[:, 1] >= 0).all())
    _check_moments(c['name'], got, c['dtype'], *_merge(parts, cnt))


def _shards(S, dev, keep, C, key='fin_acc', width=None):
    keep.append(torch.zeros(8, width or 2 * C + 1, dtype=torch.float64, device=dev))
    setattr(S, key, keep[-1].data_ptr())
    return keep[-1]


@pytest.mark.gpu
@pytest.mark.parametrize('c', SHARD_CASES)
def test_fin_acc_shards_are_the_moments_of_the_stored_output(c):
    """fin_acc without a ticket: the launch adds (sum, sum of squares, count) to the 8 fp64 shards and nothing else."""
    o, st = build(c), {}

    def setup(S, dev, keep):
        st['acc'] = _shards(S, dev, keep, c['Cout'])
    got, _ = run_case(c, o, setup)
    assert CA.ratio(got, o['ref']) <= 1.0
    C = c['Cout']
    acc = st['acc'].cpu().sum(0)
    _check_moments(c['name'], got, c['dtype'], float(acc[2 * C]), acc[:C], acc[C:2 * C])


@pytest.mark.gpu
@pytest.mark.parametrize('c', [STATS_CASES[i] for i in (0, 1, 3, 6, 8, 10)])
def test_fin_acc_with_ticket_finalizes_in_the_launch(c):
    """fin_acc + fin_ticket + fin: the last workgroup computes what salt_bn_finalize would have from the shards
    (op_reference.bn_finalize_shards of the stored output's moments) and leaves shards and ticket zero.  Bounds: the moments carry
    conv_abi.moments' tolerances; mean, variance and the derived vectors are evaluated at both ends of those intervals, plus 8 fp32 ulps
    for the fp32 results."""
    import op_reference as R
    from salt_amd._abi import STRUCTS, fill
    import ctypes
    o, st = build(c), {}
    C = c['Cout']
    g = torch.Generator().manual_seed(5)
    gamma, beta = R.round_to(torch.rand(C, generator=g, dtype=R.F64) + 0.5, 'f32'), R.round_to(torch.randn(C, generator=g, dtype=R.F64), 'f32')
    rm, rv = R.round_to(torch.randn(C, generator=g, dtype=R.F64), 'f32'), R.round_to(torch.rand(C, generator=g, dtype=R.F64) + 0.5, 'f32')

    def setup(S, dev, keep):
        st['acc'] = _shards(S, dev, keep, C)
        st['ticket'] = torch.zeros(3, dtype=torch.int32, device=dev)
        st['out'] = {k: torch.full((C,), float('nan'), device=dev) for k in ('mean', 'invstd', 'scale', 'shift')}
        st['in'] = {k: v.float().to(dev) for k, v in dict(gamma=gamma, beta=beta, running_mean=rm, running_var=rv).items()}
        st['steps'] = torch.full((1,), 41, dtype=torch.int64, device=dev)
        f = fill(STRUCTS['salt_bn_finalize_args'](), C=C, momentum=0.1, eps=1e-5, num_batches_tracked=st['steps'].data_ptr(),
                 **{k: v.data_ptr() for k, v in list(st['out'].items()) + list(st['in'].items())})
        keep.append(f)
        S.fin, S.fin_ticket = ctypes.addressof(f), st['ticket'].data_ptr() + 4
    got, _ = run_case(c, o, setup)
    assert st['ticket'].cpu().tolist() == [0, 0, 0] and float(st['acc'].abs().max()) == 0.0, 'ticket and shards are left zero'
    assert int(st['steps'].cpu()) == 42
    y = got.reshape(-1, C)
    s, q, ts, tq = CA.moments(y, c['dtype'])
    n = y.shape[0]

    def fin(ds, dq):
        sh = torch.zeros(8, 2 * C + 1, dtype=R.F64)
        sh[0, :C], sh[0, C:2 * C], sh[0, 2 * C] = s + ds, (q + dq).clamp_min(0), n
        return R.bn_finalize_shards(sh, gamma, beta, rm, rv, 0.1, 1e-5)
    ref = fin(0, 0)
    corners = [fin(a * ts, b * tq) for a in (-1, 1) for b in (-1, 1)]
    outs = dict(st['out'], running_mean=st['in']['running_mean'], running_var=st['in']['running_var'])
    for k, v in outs.items():
        tol = torch.stack([(cn[k] - ref[k]).abs() for cn in corners]).max(0).values + 8 * CA.U32 * ref[k].abs()
        r = float(((v.double().cpu() - ref[k]).abs() / tol).max())
        print('%s %s at %.3f of the bound' % (c['name'], k, r))
        assert r <= 1.0, '%s %s at %.3f of the bound' % (c['name'], k, r)


@pytest.mark.gpu
@pytest.mark.parametrize('dt,kid', [('f32', 1), ('bf16', 1), ('bf16', 4), ('f32', 5)])
def test_stats_part0_chains_the_partials_of_four_phase_launches(dt, kid):
    """The four out_step = 2 launches of ConvTranspose2d(k4, s2, p1) write their partials one after the other (stats_part0): together
    they are the moments of the whole stored output."""
    lib = _lib()
    dev = 'cuda:0'
    B, Ci, Co, H, W = 2, 32, 40, 9, 5
    x = CA.mk(B, Ci, H, W, 51).permute(0, 2, 3, 1).contiguous()
    w = CA.master_weight(Ci, Co, 4, 4, Ci, 4, 52)
    bias = _vec(Co, 3, 'bias').float()
    X = CA.Placed((B, H, W), (0, Ci, Ci), dt, dev, x)
    Y = CA.Placed((B, 2 * H, 2 * W), (0, Co, Co), dt, dev)
    bd = bias.to(dev)
    part0, stats, cnt, worst = 0, None, None, 0.0
    for fy, fx, sel in CA.convt_phases(4):
        tap_k, offs = [(t[0], t[1]) for t in sel], [(t[2], t[3]) for t in sel]
        wp = CA.pack(w.to(dev), dt, tap_k, 1)
        S = CA.conv_args(dt, X.view, wp.data_ptr(), offs, Y.view, H, W, out_step=2, out_oy=fy, out_ox=fx, bias=bd.data_ptr(), cfg=kid)
        n = lib.salt_conv_stats_parts(_byref(S))
        if stats is None:
            stats = torch.full((lib.salt_bn_stats_floats(4 * n, Co),), float('nan'), device=dev)
            cnt = torch.full((4 * n,), float('nan'), device=dev)
        S.stats, S.stats_cnt, S.stats_part0 = stats.data_ptr(), cnt.data_ptr(), part0
        assert CA.conv_kernel_id(S) == kid
        out = CA.conv_hip(S, Y.buf)
        part0 += n
        ref = CA.conv_ref(x, CA.tap_weights(w, tap_k, 1), offs, 1, 0, H, W, dt, bias.double())
        worst = max(worst, CA.ratio(out[:, fy::2, fx::2].double(), ref))
    assert worst <= 1.0, worst
    parts = stats[:part0 * 2 * Co].reshape(part0, 2, Co).double().cpu()
    _check_moments('%s cfg%d' % (dt, kid), out.double(), dt, *_merge(parts, cnt.double().cpu()))


# ---------------------------------------------------------------- BatchNorm-backward sums of the stored gradient
def _bnb_problem(B, H, W, C, dtype, seed):
    """yc (the producer's output, pre-activations kept 1e-2 from zero), a (a forward output for the mask), per-channel statistics."""
    import op_reference as R
    g = torch.Generator().manual_seed(seed)
    mean, invstd = R.round_to(0.3 * torch.randn(C, generator=g, dtype=R.F64), 'f32'), R.round_to(0.5 + torch.rand(C, generator=g, dtype=R.F64), 'f32')
    gamma, beta = R.round_to(0.5 + torch.rand(C, generator=g, dtype=R.F64), 'f32'), R.round_to(0.3 * torch.randn(C, generator=g, dtype=R.F64), 'f32')
    yc = torch.randn(B, H, W, C, generator=g, dtype=R.F64)
    yc = R.avoid_zero_crossings(yc, lambda t: (t - mean) * invstd * gamma + beta, 1e-2, dtype)
    a = R.round_to(torch.randn(B, H, W, C, generator=g, dtype=R.F64), dtype)
    a = torch.where(a.abs() < 1e-2, torch.ones_like(a), a)
    return dict(mean=mean, invstd=invstd, gamma=gamma, beta=beta, yc=yc, a=a)


def _bnb_check(what, got, pr, mask_from, s1, s2):
    """sum g m and sum g m xhat of the STORED gradient g: the products are formed and added in fp32, N + 8 roundings per channel."""
    import op_reference as R
    C = got.shape[-1]
    xhat = (pr['yc'] - pr['mean']) * pr['invstd']
    m = ((pr['a'] > 0) if mask_from == 'a' else (xhat * pr['gamma'] + pr['beta'] > 0)).to(R.F64)
    gm = (got * m).reshape(-1, C)
    gx = gm * xhat.reshape(-1, C)
    u = (gm.shape[0] + 8) * CA.U32
    r1 = float(((s1 - gm.sum(0)).abs() / (u * gm.abs().sum(0))).max())
    r2 = float(((s2 - gx.sum(0)).abs() / (u * gx.abs().sum(0))).max())
    print('%s: sum g m at %.3f, sum g m xhat at %.3f of the bound' % (what, r1, r2))
    assert r1 <= 1.0 and r2 <= 1.0, '%s: sum g m at %.3f, sum g m xhat at %.3f of the bound' % (what, r1, r2)


DG = CA.dgrad_taps(K3)
DGX = CA.dgrad_taps_extended(K3R, 2)
BNB_CASES = [pytest.param(c, id=c['name']) for c in [
    C_('f32-cfg1-plain', 1, 'f32', 2, 40, 24, 9, 11, DG, transpose=1), C_('bf16-cfg1-plain', 1, 'bf16', 2, 40, 24, 9, 11, DG, transpose=1),
    C_('bf16-cfg4-plain-accumulate', 4, 'bf16', 2, 40, 24, 9, 11, DG, transpose=1, acc=True),
    C_('f32-cfg5-plain', 5, 'f32', 5, 24, 40, 8, 8, DG, transpose=1), C_('bf16-cfg2-full-tiles', 2, 'bf16', 1, 64, 64, 16, 16, DG, transpose=1),
    C_('f32-cfg1-fold-fused-18x18', 1, 'f32', 2, 40, 24, 16, 16, DGX, transpose=1, fold=('fused', 2, 2), gen=1),
    C_('bf16-cfg1-fold-fused-14x22', 1, 'bf16', 2, 40, 24, 12, 20, DGX, transpose=1, fold=('fused', 2, 2), gen=1, acc=True),
    C_('bf16-cfg4-fold-fused-7x9', 4, 'bf16', 3, 40, 24, 5, 7, DGX, transpose=1, fold=('fused', 2, 2), gen=1),
    C_('bf16-cfg5-fold-fused-10x10', 5, 'bf16', 2, 40, 24, 8, 8, DGX, transpose=1, fold=('fused', 2, 2)),
    C_('bf16-glds7-plain', 7, 'bf16', 2, 64, 40, 17, 9, DG, transpose=1), C_('bf16-glds8-plain-accumulate', 8, 'bf16', 2, 96, 40, 17, 9, DG, transpose=1, acc=True),
    C_('bf16-glds6-plain', 6, 'bf16', 2, 32, 72, 33, 17, DG, transpose=1),
    C_('bf16-glds7-fold-fused-14x22', 7, 'bf16', 2, 64, 40, 12, 20, DGX, transpose=1, fold=('fused', 2, 2), gen=1),
]]
BNB_SHARD_ONLY = [pytest.param(c, id=c['name']) for c in [
    C_('ws-64-64', 9, 'bf16', 2, 64, 64, 16, 32, DG, transpose=1, cfg=9 | (1 << 8)), C_('ws-accumulate-ragged-grid', 9, 'bf16', 2, 32, 64, 24, 20, DG, transpose=1, acc=True),
    C_('ws-fold-fused-18x18', 9, 'bf16', 2, 64, 64, 16, 16, DGX, transpose=1, fold=('fused', 2, 2)),
    C_('ls-64-32', 10, 'bf16', 2, 64, 32, 16, 16, DG, transpose=1, cfg=10 | (1 << 8)), C_('ls-128-64-accumulate', 10, 'bf16', 2, 128, 64, 16, 32, DG, transpose=1, acc=True),
    C_('thin-32-16', 12, 'f32', 2, 32, 16, 16, 16, DG, transpose=1), C_('thin-16-32-accumulate', 12, 'f32', 3, 16, 32, 16, 32, DG, transpose=1, acc=True),
]]


def _bnb_setup(c, pr, mask_from, st, shards):
    lib = _lib()

    def setup(S, dev, keep):
        C, dt = c['Cout'], c['dtype']
        YC = CA.Placed((c['B'], c['yH'], c['yW']), (0, C, C), dt, dev, pr['yc'])
        keep.append(YC)
        S.bnb_y = YC.view
        if mask_from == 'a':
            A = CA.Placed((c['B'], c['yH'], c['yW']), (8, C, C + 16), dt, dev, pr['a'])
            keep.append(A)
            S.bnb_a = A.view
        for k in ('mean', 'invstd', 'gamma', 'beta'):
            keep.append(pr[k].float().to(dev))
            setattr(S, 'bnb_' + k, keep[-1].data_ptr())
        S.bnb_relu = 1
        if shards:
            st['acc'] = _shards(S, dev, keep, C, 'bnb_acc', 2 * C)
        else:
            n = lib.salt_conv_stats_parts(_byref(S))
            assert n >= 1
            st['parts'] = torch.full((n, 2, C), float('nan'), device=dev)
            S.bnb_partials = st['parts'].data_ptr()
    return setup


@pytest.mark.gpu
@pytest.mark.parametrize('mask_from', ['y', 'a'])
@pytest.mark.parametrize('c', BNB_CASES)
def test_bnb_partials(c, mask_from):
    o, st = build(c), {}
    pr = _bnb_problem(c['B'], c['yH'], c['yW'], c['Cout'], c['dtype'], 61)
    got, _ = run_case(c, o, _bnb_setup(c, pr, mask_from, st, False))
    assert CA.ratio(got, o['ref']) <= 1.0
    parts = st['parts'].double().cpu()
    assert torch.isfinite(parts).all()
    _bnb_check(c['name'], got, pr, mask_from, parts[:, 0].sum(0), parts[:, 1].sum(0))


@pytest.mark.gpu
@pytest.mark.parametrize('mask_from', ['y', 'a'])
@pytest.mark.parametrize('c', BNB_CASES + BNB_SHARD_ONLY)
def test_bnb_acc_shards(c, mask_from):
    o, st = build(c), {}
    pr = _bnb_problem(c['B'], c['yH'], c['yW'], c['Cout'], c['dtype'], 62)
    got, _ = run_case(c, o, _bnb_setup(c, pr, mask_from, st, True))
    assert CA.ratio(got, o['ref']) <= 1.0
    C = c['Cout']
    acc = st['acc'].cpu().reshape(8, 2, C).sum(0)
    _bnb_check(c['name'], got, pr, mask_from, acc[0], acc[1])


@pytest.mark.gpu
@pytest.mark.parametrize('shards', [False, True])
@pytest.mark.parametrize('dt,kid', [('f32', 1), ('bf16', 4), ('bf16', 5)])
def test_bnb_sums_of_an_all_phases_stride2_launch(dt, kid, shards):
    """nphase = 4 over an even grid writes every pixel of y once: the launch may carry the BatchNorm-backward sums."""
    lib = _lib()
    dev = 'cuda:0'
    B, Ci, Co, H, W = 2, 24, 40, 10, 12
    phases = CA.dgrad_s2_phases(K3)
    offs, rows = CA.unify_phases(phases)
    dy = CA.mk(B, Co, H // 2, W // 2, 71).permute(0, 2, 3, 1).contiguous()
    w = CA.master_weight(Co, Ci, 3, 3, Co, 4, 72)
    pr = _bnb_problem(B, H, W, Ci, dt, 73)
    X = CA.Placed((B, H // 2, W // 2), (0, Co, Co), dt, dev, dy)
    Y = CA.Placed((B, H, W), (0, Ci, Ci), dt, dev)
    wp, elems = CA.pack_phases(w.to(dev), dt, rows, 1)
    S = CA.conv_args(dt, X.view, wp.data_ptr(), offs, Y.view, H // 2, W // 2, out_step=2, nphase=4, w_phase_elems=elems, cfg=kid)
    st, keep = {}, []
    c = dict(Cout=Ci, dtype=dt, B=B, yH=H, yW=W)
    _bnb_setup(c, pr, 'y', st, shards)(S, dev, keep)
    assert CA.conv_kernel_id(S) == kid, CA.last_error()
    got = CA.conv_hip(S, Y.buf).double()
    for (ay, ax, sel), row in zip(phases, rows):
        assert CA.ratio(got[:, ay::2, ax::2], CA.conv_ref(dy, CA.tap_weights(w, row, 1), offs, 1, 0, H // 2, W // 2, dt)) <= 1.0
    if shards:
        acc = st['acc'].cpu().reshape(8, 2, Ci).sum(0)
        _bnb_check('all phases', got, pr, 'y', acc[0], acc[1])
    else:
        parts = st['parts'].double().cpu()
        assert torch.isfinite(parts).all()
        _bnb_check('all phases', got, pr, 'y', parts[:, 0].sum(0), parts[:, 1].sum(0))


# ---------------------------------------------------------------- planar layouts, the in-launch finalize of the input transform
def _planar_run(c, o, side, gap):
    """The case with its x (conv_ls_kernel) or y (conv_ws_kernel) stored as C / 64 dense planes [B, H, W, 64], `gap` guard elements
    between the planes -> values [B, H, W, Cout] float64."""
    from salt_amd.engine import shaped_view
    dev, dt = 'cuda:0', c['dtype']
    B, H, W, Cin, Cout = c['B'], c['H'], c['W'], c['Cin'], c['Cout']
    tdt = torch.bfloat16
    wp = CA.pack(o['w'].to(dev), dt, o['tap_k'], c['transpose'])
    keep, f = [wp], dict(pad_mode=c['pad_mode'], relu=int(c['relu']), accumulate=int(c['acc']), cfg=c['cfg'])
    for k in ('bias', 'scale', 'shift'):
        if c[k]:
            keep.append(o[k].float().to(dev))
            f[k] = keep[-1].data_ptr()
    n = B * H * W * 64
    if side == 'x':
        planes = Cin // 64
        xb = CA.guard_fill(torch.empty(planes, n + gap, dtype=tdt, device=dev))
        for p in range(planes):
            xb[p, :n] = o['x'][..., 64 * p:64 * p + 64].reshape(-1).to(tdt).to(dev)
        Y = CA.Placed((B, H, W), (0, Cout, Cout), dt, dev)
        yb = Y.buf
        S = CA.conv_args(dt, shaped_view(xb.data_ptr(), B, H, W, Cin, 64), wp.data_ptr(), o['offs'], Y.view, H, W, x_plane=n + gap, **f)
    else:
        planes = Cout // 64
        X = CA.Placed((B, H, W), (0, Cin, Cin), dt, dev, o['x'])
        yb = CA.guard_fill(torch.empty(planes, n + gap, dtype=tdt, device=dev))
        if c['acc']:
            for p in range(planes):
                yb[p, :n] = o['old'][..., 64 * p:64 * p + 64].reshape(-1).to(tdt).to(dev)
        S = CA.conv_args(dt, X.view, wp.data_ptr(), o['offs'], shaped_view(yb.data_ptr(), B, H, W, Cout, 64), H, W, y_plane=n + gap, **f)
    kid = CA.conv_kernel_id(S)
    assert kid == c['kid'], 'the plan runs kernel %d (%s)' % (kid, CA.last_error() if kid < 0 else '')
    out = CA.conv_hip(S, yb)
    if side == 'x':
        return out.double()
    assert bool((CA.bits(out[:, n:]) == CA.GUARD[tdt]).all()), 'the gap between the planes was written'
    return torch.cat([out[p, :n].reshape(B, H, W, 64) for p in range(planes)], 3).double()


@pytest.mark.gpu
@pytest.mark.parametrize('c,side', [
    (C_('ws-planar-y-64-128', 9, 'bf16', 2, 64, 128, 16, 16, K3), 'y'),
    (C_('ws-planar-y-32-128-accumulate', 9, 'bf16', 2, 32, 128, 16, 32, CA.dgrad_taps(K3), transpose=1, acc=True, cfg=9 | (1 << 8)), 'y'),
    (C_('ls-planar-x-128-64', 10, 'bf16', 2, 128, 64, 16, 16, K3, cfg=10 | (2 << 16)), 'x'),
    (C_('ls-planar-x-128-32-epilogue', 10, 'bf16', 2, 128, 32, 16, 32, K3R, pad_mode=1, cfg=10 | (1 << 8), bias=True, scale=True, shift=True, relu=True), 'x'),
], ids=lambda v: v['name'] if isinstance(v, dict) else v)
def test_planar_layouts(c, side):
    o = build(c)
    got = _planar_run(c, o, side, 64)
    assert torch.isfinite(got).all()
    r = CA.ratio(got, o['ref'])
    print('kernel %d %s max err / tol = %.3f' % (c['kid'], c['dtype'], r))
    assert r <= 1.0, r


def test_planar_layouts_are_refused_elsewhere():
    """Host only: y_plane / x_plane on a launch the one kernel that knows the layout does not take has no plan."""
    from salt_amd.engine import shaped_view
    for key, cfg in (('y_plane', 1), ('x_plane', 9)):
        S = CA.conv_args('bf16', shaped_view(1 << 20, 2, 16, 16, 128, 64 if key == 'x_plane' else 128), 1 << 27, [(t[2], t[3]) for t in K3],
                         shaped_view(1 << 24, 2, 16, 16, 128, 64 if key == 'y_plane' else 128), 16, 16, cfg=cfg, **{key: 2 * 16 * 16 * 64})
        assert CA.conv_kernel_id(S) == -1


@pytest.mark.gpu
@pytest.mark.parametrize('kid,B,Cin,H,W', [(1, 2, 40, 33, 17), (4, 2, 64, 16, 16), (2, 1, 64, 16, 16)])
def test_input_transform_finalized_in_the_launch(kid, B, Cin, H, W):
    """in_fin_acc: every workgroup finalizes the producer's fp64 shards itself, workgroup 0 stores mean / invstd / scale / shift (fp64
    arithmetic on given shards, one fp32 rounding of each result: 8 ulps with the cancellation in shift counted by its terms).  The
    convolution is then held to the reference over the transform with the scale / shift the launch stored."""
    import ctypes
    import op_reference as R
    from salt_amd._abi import STRUCTS, fill
    c = C_('in-fin', kid, 'bf16', B, Cin, 40, H, W, K3)
    o, st = build(c), {}
    g = torch.Generator().manual_seed(9)
    gamma, beta = R.round_to(torch.rand(Cin, generator=g, dtype=R.F64) + 0.5, 'f32'), R.round_to(torch.randn(Cin, generator=g, dtype=R.F64) * 0.5, 'f32')
    flat = o['x'].double().reshape(-1, Cin)
    cuts = [0, 1, 30, 30, 31, 70, 70, 95, flat.shape[0]]
    shards = torch.zeros(8, 2 * Cin + 1, dtype=R.F64)
    for s in range(8):
        p = flat[cuts[s]:cuts[s + 1]]
        shards[s, :Cin], shards[s, Cin:2 * Cin], shards[s, 2 * Cin] = p.sum(0), (p * p).sum(0), p.shape[0]
    ref = R.bn_finalize_shards(shards, gamma, beta, None, None, 0.1, 1e-5)

    def setup(S, dev, keep):
        st['sh'] = shards.to(dev)
        st['out'] = {k: torch.full((Cin,), float('nan'), device=dev) for k in ('mean', 'invstd', 'scale', 'shift')}
        st['in'] = {k: v.float().to(dev) for k, v in dict(gamma=gamma, beta=beta).items()}
        f = fill(STRUCTS['salt_bn_finalize_args'](), C=Cin, momentum=0.1, eps=1e-5,
                 **{k: v.data_ptr() for k, v in list(st['out'].items()) + list(st['in'].items())})
        keep.append(f)
        S.in_fin, S.in_fin_acc, S.in_relu = ctypes.addressof(f), st['sh'].data_ptr(), 1
    # the launch first: the reference needs the scale / shift it stored
    dev = 'cuda:0'
    X = CA.Placed((B, H, W), (0, Cin, Cin), 'bf16', dev, o['x'])
    Y = CA.Placed((B, H, W), (0, 40, 40), 'bf16', dev)
    wp = CA.pack(o['w'].to(dev), 'bf16', o['tap_k'], 0)
    S = CA.conv_args('bf16', X.view, wp.data_ptr(), o['offs'], Y.view, H, W, cfg=kid)
    keep = []
    setup(S, dev, keep)
    assert CA.conv_kernel_id(S) == kid, CA.last_error()
    got = CA.conv_hip(S, Y.buf).double()
    assert torch.equal(st['sh'].cpu(), shards), 'the shards are read only'
    for k in ('mean', 'invstd', 'scale'):
        assert bool(((st['out'][k].double().cpu() - ref[k]).abs() <= 8 * CA.U32 * ref[k].abs()).all()), k
    assert bool(((st['out']['shift'].double().cpu() - ref['shift']).abs() <= 8 * CA.U32 * (beta.abs() + (ref['mean'] * ref['scale']).abs())).all())
    tf = (st['out']['scale'].double().cpu(), st['out']['shift'].double().cpu(), True)
    r = CA.ratio(got, CA.conv_ref(o['x'], o['wt'], o['offs'], 1, 0, H, W, 'bf16', in_tf=tf))
    print('kernel %d bf16 max err / tol = %.3f' % (kid, r))
    assert torch.isfinite(got).all() and r <= 1.0, r
