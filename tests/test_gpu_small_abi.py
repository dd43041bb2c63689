"""The kernels of csrc/conv_small.hip one by one through the C-ABI: salt_conv_first, salt_conv_first_wgrad, salt_head1x1,
salt_head1x1_bwd (ELEMENTWISE against the float64 references of small_abi.py with the bounds derived there: max err / tol <= 1) and
salt_s2d, salt_pack_stem_weight, salt_stem_grad_unfold (bit for bit).  Every case names the kernel it is meant for and asserts it
before the launch (salt_head1x1_kernel_id, salt_head1x1_bwd_kernel_id, salt_conv_first_wgrad_kernel_id: host only).  Whatever a launch
must write starts as NaN; gap channels of views and the tails of partials / statistics / gradient buffers hold a bit pattern that must
survive.

The tables and the operand builders live in small_abi.py, importable without a GPU: test_small_reference_cpu.py asserts the tables' claims (kernel ids,
part counts, PER, which predicate a view fails) on the host and runs an fp32 stand-in over them."""
import pytest
import torch

import small_abi as SA
from small_abi import (DTYPES, FIRST_CASES, HEAD_BWD_CASES, HEAD_CASES, HEAD_GRID_CAP, WGRAD_CASES, _arbitrary, _ids, first_build, first_case,
                       first_vec, hb_build, hb_case, hb_plan, head_build, head_plan, wg_build, wg_nparts, wg_plan)

DEV = 'cuda:0'


def _report(what, r):
    print('%s max err / tol = %.3f' % (what, r))
    assert r <= 1.0, '%s: max err / tol = %.3f' % (what, r)


# ================================================================ salt_conv_first
def first_launch(c, o, **override):
    """-> (rc, Placed y, stats Guarded | None, cnt Guarded | None, tiles)."""
    OH, OW = SA.first_geom(c['H'], c['W'], c['K'], c['s'], c['p'])
    Y = SA.Placed((c['B'], OH, OW), (c['yv'][0], c['Cout'], c['yv'][1]), c['dtype'], DEV)
    keep = {k: o[k].float().to(DEV) for k in ('x', 'w')}
    kw = {}
    for k in ('bias', 'scale', 'shift'):
        if o.get(k) is not None:
            keep[k] = o[k].float().to(DEV)
            kw[k] = keep[k].data_ptr()
    S = SA.first_args(c['dtype'], keep['x'].data_ptr(), (c['B'], c['Cin'], c['H'], c['W']), keep['w'].data_ptr(), c['K'], c['s'], c['p'], Y.view,
                      relu=int(c['relu']), **kw)
    for k, v in override.items():
        setattr(S, k, v)
    st = cn = None
    tiles = SA.query('salt_conv_first_stats_parts', S)
    if c['stats']:
        st = SA.Guarded(tiles * 2 * c['Cout'], torch.float32, DEV)
        cn = SA.Guarded(tiles, torch.float32, DEV)
        S.stats, S.stats_cnt = st.ptr(), cn.ptr()
    return SA.call('salt_conv_first', S), Y, st, cn, tiles


@pytest.mark.gpu
@pytest.mark.parametrize('c', _ids(FIRST_CASES))
def test_conv_first_vs_float64(c):
    o = first_build(c)
    assert first_vec(c) == c['vec']
    rc, Y, st, cn, tiles = first_launch(c, o)
    assert rc == 0, SA.last_error()
    Y.check(c['name'])
    ref = o['ref']
    OH, OW = ref['exact'].shape[1:3]
    assert tiles == c['B'] * SA.cdiv(OH, 16) * SA.cdiv(OW, 16)
    got = Y.get()
    assert torch.isfinite(got).all()
    _report('conv_first %s' % c['dtype'], SA.ratio(got, ref))
    if c['stats']:
        sr = SA.first_stats_ref(ref['exact'], ref['pre_tol'])
        cnt = cn.get('stats_cnt').double()
        assert torch.equal(cnt, sr['cnt']), 'tile counts %r' % cnt.tolist()
        assert sorted(set(cnt.tolist())) == sorted({256.0, 16.0 * (OW - 16), 16.0 * (OH - 16), 1.0 * (OH - 16) * (OW - 16)})
        parts = st.get('stats').double().reshape(tiles, 2, c['Cout'])
        assert torch.isfinite(parts).all()
        r = (parts - sr['stats']).abs() / sr['tol']
        print('conv_first %s stats: sum at %.3f, M2 at %.3f of the bound' % (c['dtype'], float(r[:, 0].max()), float(r[:, 1].max())))
        assert float(r.max()) <= 1.0, 'sum at %.3f, M2 at %.3f of the bound' % (float(r[:, 0].max()), float(r[:, 1].max()))


FIRST_REFUSALS = [('cin5', dict(Cin=5)), ('k8', dict(K=8)), ('stride3', dict(stride=3)), ('scale-without-shift', dict(shift=None)),
                  ('y-view-size', dict())]


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('what,override', FIRST_REFUSALS, ids=[r[0] for r in FIRST_REFUSALS])
def test_conv_first_refuses(what, override, dtype):
    """SALT_E_BADARG with a message, and nothing written."""
    c = first_case('refuse', dtype, 3, 34, 38, 7, 2, 3, 24, scale=True)
    if what == 'y-view-size':
        c['H'] += 2                                                         # the view is built for 18 x 19 outputs, the launch says 34 rows
        o = first_build(c)
        rc, Y, _, _, _ = first_launch(c, o, H=c['H'] - 2)
    else:
        o = first_build(c)
        if what == 'cin5':
            o['x'] = SA.mk(c['B'], 5, c['H'], c['W'], 11)                   # memory for what the arguments claim, although nothing may read it
            o['w'] = SA.master_weight(c['Cout'], 5, 8, 8, 5, 64, 12)
        if what == 'k8':
            o['w'] = SA.master_weight(c['Cout'], 5, 8, 8, 5, 64, 12)
        rc, Y, _, _, _ = first_launch(c, o, **override)
    assert rc == -1, rc
    assert 'conv_first' in SA.last_error()
    assert bool((SA.bits(Y.buf.cpu()) == SA.GUARD[Y.buf.dtype]).all()), 'a refused launch wrote to y'


# ================================================================ salt_conv_first_wgrad
@pytest.mark.gpu
@pytest.mark.parametrize('acc', [0, 1], ids=['store', 'accumulate'])
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('c', _ids(WGRAD_CASES))
def test_conv_first_wgrad_vs_float64(c, dtype, acc):
    o = wg_build(c, acc)
    n = c['Cout'] * c['Cin'] * c['K'] * c['K']
    nparts = wg_nparts(c)
    xd = o['x'].to(DEV)
    DY = SA.Placed((c['B'], c['OH'], c['OW']), (c['dyv'][0], c['Cout'], c['dyv'][1]), dtype, DEV, o['dy'])
    part = SA.Guarded(nparts * n, torch.float32, DEV)
    grad = SA.Guarded(n, torch.float32, DEV, o['old'])
    S = wg_plan(c, dtype, xd.data_ptr(), DY.buf.data_ptr(), part.ptr(), grad.ptr(), acc)
    S.dy = DY.view
    assert SA.query('salt_conv_first_wgrad_parts', S) == nparts
    kid = SA.query('salt_conv_first_wgrad_kernel_id', S)
    assert kid == c['kid'], 'the launch takes instantiation %d, this case is meant for %d (%s)' % (kid, c['kid'], SA.last_error() if kid < 0 else '')
    rc = SA.call('salt_conv_first_wgrad', S)
    assert rc == c['rc'], (rc, SA.last_error())
    got, slab = grad.get('grad'), part.get('partials')
    if rc != 0:
        assert 'conv_first_wgrad' in SA.last_error()
        assert bool(torch.isnan(slab).all()) and (bool(torch.isnan(got).all()) if not acc else torch.equal(got.double(), o['old'].reshape(-1)))
        return
    assert torch.isfinite(slab).all(), 'the launch left elements of the partials unwritten'
    assert torch.isfinite(got).all()
    _report('conv_first_wgrad %s id %d' % (dtype, kid), SA.worst(got.double(), o['ref']))


# ================================================================ salt_head1x1
def head_run(c, out, bias):
    o = head_build(c)
    b = o['bias'] if bias else None
    X = SA.Placed((c['B'], c['H'], c['W']), (c['xv'][0], c['C'], c['xv'][1]), c['dtype'], DEV, o['x'])
    wd = o['w'].to(DEV)
    bd = b.float().to(DEV) if bias else None
    bp = bd.data_ptr() if bias else None
    npix = c['B'] * c['H'] * c['W']
    if out == 'nchw':
        Y = SA.Guarded(npix * c['Cout'], torch.float32, DEV)
        S = head_plan(c, out, 0, wd.data_ptr(), bp, Y.ptr())
    else:
        Y = SA.Placed((c['B'], c['H'], c['W']), (3, c['Cout'], c['Cout'] + 6), c['dtype'], DEV)
        S = head_plan(c, out, 0, wd.data_ptr(), bp)
        S.y = Y.view
    S.x = X.view
    kid = SA.query('salt_head1x1_kernel_id', S)
    assert kid == c['kid'], 'the launch takes kernel %d, this case is meant for %d' % (kid, c['kid'])
    SA.run('salt_head1x1', S)
    if out == 'nchw':
        got = Y.get('y_nchw').double().reshape(c['B'], c['Cout'], c['H'], c['W']).permute(0, 2, 3, 1)
    else:
        Y.check(c['name'])
        got = Y.get()
    assert torch.isfinite(got).all()
    ref = SA.head_ref(o['x'].double(), o['w'].double(), b, None if out == 'nchw' else c['dtype'])
    _report('head1x1 %s kernel %d %s' % (c['dtype'], kid, out), SA.ratio(got, ref))


@pytest.mark.gpu
@pytest.mark.parametrize('bias', [True, False], ids=['bias', 'nobias'])
@pytest.mark.parametrize('out', ['nchw', 'view'])
@pytest.mark.parametrize('c', _ids(HEAD_CASES))
def test_head1x1_vs_float64(c, out, bias):
    head_run(c, out, bias)


@pytest.mark.gpu
def test_head1x1_above_the_grid_cap():
    """4160 blocks' worth of units on 4096 blocks: the grid-stride loop runs a second time for the first 64 blocks, with both pixels in
    flight in the first pass."""
    head_run(HEAD_GRID_CAP, 'nchw', True)


# ================================================================ salt_head1x1_bwd
def hb_launch(c, o, acc, gb, wrong_nparts=False):
    npix = c['B'] * c['H'] * c['W']
    X = SA.Placed((c['B'], c['H'], c['W']), (c['xv'][0], c['C'], c['xv'][1]), c['dtype'], DEV, o['x'])
    DX = SA.Placed((c['B'], c['H'], c['W']), (c['dxv'][0], c['C'], c['dxv'][1]), c['dtype'], DEV, o['old'])
    wd, dyd = o['w'].to(DEV), o['dy'].to(DEV)
    S = hb_plan(c, acc, gb, 0, 0)
    S.x, S.dx, S.w, S.dy_nchw = X.view, DX.view, wd.data_ptr(), dyd.data_ptr()
    nparts = SA.query('salt_head1x1_bwd_parts', S)
    assert nparts == SA.head_parts(npix), (nparts, npix)
    part = SA.Guarded(nparts * c['Cout'] * (c['C'] + 1), torch.float32, DEV)
    gw = SA.Guarded(c['Cout'] * c['C'], torch.float32, DEV)
    gbb = SA.Guarded(c['Cout'], torch.float32, DEV)
    S.partials, S.gw, S.gb, S.nparts = part.ptr(), gw.ptr(), gbb.ptr() if gb else None, nparts + int(wrong_nparts)
    kid = SA.query('salt_head1x1_bwd_kernel_id', S)
    return S, kid, DX, part, gw, gbb


@pytest.mark.gpu
@pytest.mark.parametrize('gb', [True, False], ids=['gb', 'nogb'])
@pytest.mark.parametrize('acc', [0, 1], ids=['store', 'accumulate'])
@pytest.mark.parametrize('c', _ids(HEAD_BWD_CASES))
def test_head1x1_bwd_vs_float64(c, acc, gb):
    o = hb_build(c, acc)
    S, kid, DX, part, gw, gbb = hb_launch(c, o, acc, gb)
    assert kid == c['kid'], 'the launch takes kernel %d, this case is meant for %d (%s)' % (kid, c['kid'], SA.last_error() if kid < 0 else '')
    SA.run('salt_head1x1_bwd', S)
    DX.check(c['name'])
    dx, slab, w_, b_ = DX.get(), part.get('partials'), gw.get('gw'), gbb.get('gb')
    assert torch.isfinite(dx).all() and torch.isfinite(slab).all() and torch.isfinite(w_).all()
    ref = o['ref']
    r = {'dx': SA.ratio(dx, ref['dx']), 'gw': SA.worst(w_.double(), ref['gw'])}
    if gb:
        assert torch.isfinite(b_).all()
        r['gb'] = SA.worst(b_.double(), ref['gb'])
    else:
        assert bool(torch.isnan(b_).all())
    print('head1x1_bwd %s kernel %d %s max err / tol: %s' % (c['dtype'], kid, 'accumulate' if acc else 'store', ', '.join('%s %.3f' % kv for kv in sorted(r.items()))))
    assert max(r.values()) <= 1.0, r


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', DTYPES)
def test_head1x1_bwd_refuses_a_wrong_part_count(dtype):
    c = hb_case('refuse', dtype, 8 * SA.VE[dtype], 2, -1, B=2, H=7, W=9)
    o = hb_build(c, 0)
    S, kid, DX, part, gw, gbb = hb_launch(c, o, 0, True, wrong_nparts=True)
    assert kid == -1
    assert SA.call('salt_head1x1_bwd', S) == -1 and 'nparts' in SA.last_error()
    assert bool(torch.isnan(part.get()).all()) and bool(torch.isnan(gw.get()).all()) and bool(torch.isnan(gbb.get()).all())
    assert bool((SA.bits(DX.buf.cpu()) == SA.GUARD[DX.buf.dtype]).all())


# ================================================================ the stem's index maps (bit for bit)
def s2d_launch(x, dtype, zv=(0, 16), **override):
    B, Cin, H, W = x.shape
    Z = SA.Placed((B, H // 2, W // 2), (zv[0], 16, zv[1]), dtype, DEV)
    xd = x.to(DEV)
    A = SA._abi()
    S = A.fill(A.STRUCTS['salt_s2d_args'](), dtype=SA.DT[dtype], x=xd.data_ptr(), B=B, Cin=Cin, H=H, W=W, z=Z.view)
    for k, v in override.items():
        setattr(S, k, v)
    return SA.call('salt_s2d', S), Z


@pytest.mark.gpu
@pytest.mark.parametrize('zv', [(0, 16), (16, 32)], ids=['whole', 'slice'])
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('Cin', [1, 2, 3, 4])
def test_s2d_bit_for_bit(Cin, dtype, zv):
    x = _arbitrary((3, Cin, 10, 14), 50 + Cin)
    rc, Z = s2d_launch(x, dtype, zv)
    assert rc == 0, SA.last_error()
    Z.check('s2d')
    want = SA.s2d_ref(x).to(Z.buf.dtype)
    got = Z.win.cpu()
    assert torch.equal(SA.bits(got), SA.bits(want))
    assert bool((SA.bits(got[..., 4 * Cin:]) == 0).all()), 'channels 4 Cin .. 15 are +0'


@pytest.mark.gpu
@pytest.mark.parametrize('what', ['odd-h', 'odd-w', 'cin5'])
def test_s2d_refuses(what):
    x = _arbitrary((2, 4, 10, 14), 59)
    over = {'odd-h': dict(H=9), 'odd-w': dict(W=13), 'cin5': dict(Cin=5)}[what]
    rc, Z = s2d_launch(x, 'bf16', **over)
    assert rc == -1 and 's2d' in SA.last_error()
    assert bool((SA.bits(Z.buf.cpu()) == SA.GUARD[Z.buf.dtype]).all())


def pack_stem_launch(w, dtype, **override):
    Cout, Cin, K, _ = w.shape
    T = (K + 1) // 2
    n = T * T * Cout * SA.KC[dtype]
    wp = SA.Guarded(n, SA.torch_dtype(dtype), DEV)
    wd = w.to(DEV)
    A = SA._abi()
    S = A.fill(A.STRUCTS['salt_pack_stem_weight_args'](), dtype=SA.DT[dtype], w=wd.data_ptr(), Cout=Cout, Cin=Cin, K=K, wp=wp.ptr())
    for k, v in override.items():
        setattr(S, k, v)
    return SA.call('salt_pack_stem_weight', S), wp


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('K', [3, 5, 7])
@pytest.mark.parametrize('Cin', [1, 2, 3, 4])
def test_pack_stem_weight_bit_for_bit(Cin, K, dtype):
    """The whole [T T][Cout][KC] block, zeros included (KC = 16 channels in fp32, 32 in bf16)."""
    w = _arbitrary((24, Cin, K, K), 60 + Cin)
    assert SA._abi().lib.salt_packed_weight_elems(SA.DT[dtype], ((K + 1) // 2) ** 2, 24, 16) == ((K + 1) // 2) ** 2 * 24 * SA.KC[dtype]
    rc, wp = pack_stem_launch(w, dtype)
    assert rc == 0, SA.last_error()
    want = SA.pack_stem_ref(w, SA.KC[dtype]).to(SA.torch_dtype(dtype)).reshape(-1)
    assert torch.equal(SA.bits(wp.get('wp')), SA.bits(want))


def unfold_launch(g16, Cin, K, old, **override):
    Cout = g16.shape[0]
    grad = SA.Guarded(Cout * Cin * K * K, torch.float32, DEV, old)
    gd = g16.to(DEV)
    A = SA._abi()
    S = A.fill(A.STRUCTS['salt_stem_grad_unfold_args'](), g16=gd.data_ptr(), Cout=Cout, Cin=Cin, K=K, grad=grad.ptr(), accumulate=int(old is not None))
    for k, v in override.items():
        setattr(S, k, v)
    return SA.call('salt_stem_grad_unfold', S), grad


@pytest.mark.gpu
@pytest.mark.parametrize('acc', [0, 1], ids=['store', 'accumulate'])
@pytest.mark.parametrize('K', [3, 5, 7])
@pytest.mark.parametrize('Cin', [1, 2, 3, 4])
def test_stem_grad_unfold_bit_for_bit(Cin, K, acc):
    T = (K + 1) // 2
    g16 = _arbitrary((24, 16, T, T), 70 + Cin)
    old = _arbitrary((24, Cin, K, K), 75) if acc else None
    rc, grad = unfold_launch(g16, Cin, K, old)
    assert rc == 0, SA.last_error()
    want = SA.stem_unfold_ref(g16, Cin, K)
    if acc:
        want = old + want                                                    # one fp32 addition, old first: the same bits on any IEEE adder
    assert torch.equal(SA.bits(grad.get('grad')), SA.bits(want.reshape(-1)))


@pytest.mark.gpu
@pytest.mark.parametrize('what', ['even-k', 'cin5'])
def test_stem_helpers_refuse(what):
    over = dict(K=4) if what == 'even-k' else dict(Cin=5)
    rc, wp = pack_stem_launch(_arbitrary((8, 4, 7, 7), 80), 'bf16', **over)
    assert rc == -1 and 'pack_stem_weight' in SA.last_error() and bool(torch.isnan(wp.get()).all())
    rc, grad = unfold_launch(_arbitrary((8, 16, 4, 4), 81), over.get('Cin', 4), over.get('K', 7), None)
    assert rc == -1 and 'stem_grad_unfold' in SA.last_error() and bool(torch.isnan(grad.get()).all())


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('K', [3, 5, 7])
def test_stem_composition_vs_float64(K, dtype):
    """salt_s2d, salt_pack_stem_weight and salt_conv on z against the float64 STRIDED convolution of x (DESIGN 15's bound with the
    K = T T 16 additions of the launch), then salt_conv_wgrad + salt_wgrad_reduce + salt_stem_grad_unfold against the float64
    [Cout][Cin][K][K] gradient."""
    import conv_abi as CA
    import wgrad_abi as WA
    B, Cin, H, W, Cout = 2, 3, 20, 28, 64
    taps = SA.stem_taps(K)
    x = SA.mk(B, Cin, H, W, 90)
    w = SA.master_weight(Cout, Cin, K, K, Cin, K * K, 91)
    rc, Z = s2d_launch(x, dtype)
    assert rc == 0, SA.last_error()
    rc, wp = pack_stem_launch(w, dtype)
    assert rc == 0, SA.last_error()
    OH, OW = H // 2, W // 2
    Y = SA.Placed((B, OH, OW), (8, Cout, Cout + 16), dtype, DEV)
    S = CA.conv_args(dtype, Z.view, wp.ptr(), taps, Y.view, OH, OW)
    assert CA.conv_kernel_id(S) > 0, CA.last_error()
    CA.conv_hip(S, Y.buf)
    Y.check('stem conv')
    v, A = SA.conv_first_sum(x, w, 2, K // 2)
    tol, _ = SA._store(v, len(taps) * 16 * SA.U32 * A + 4 * SA.U32 * v.abs(), dtype)
    _report('stem K %d %s forward (conv kernel %d)' % (K, dtype, CA.conv_kernel_id(S)), SA.ratio(Y.get(), dict(exact=v, tol=tol)))
    # weight gradient: P = dY (a = cout), Q = z (b = the 16 space-to-depth channels), at most 9 taps per launch
    dy = SA.mk(B, Cout, OH, OW, 92)
    dyd = WA.nhwc(dy, SA.torch_dtype(dtype)).to(DEV)
    T = (K + 1) // 2
    g16 = torch.full((Cout, 16, T, T), float('nan'))
    per = 8 if len(taps) > 9 else 9
    for i in range(0, len(taps), per):
        ch = list(range(i, min(i + per, len(taps))))
        g, _ = WA.wgrad_hip(dyd, Z.win, [taps[j] for j in ch], 0, Ca=Cout, Cb=16, KH=T, KW=T, tap_k=[(j // T, j % T) for j in ch])
        g16 = torch.where(torch.isnan(g16), g, g16)
    assert torch.isfinite(g16).all()
    rc, grad = unfold_launch(g16, Cin, K, None)
    assert rc == 0, SA.last_error()
    ref = SA.conv_first_wgrad_ref(x, dy.permute(0, 2, 3, 1), K, 2, K // 2)
    _report('stem K %d %s weight gradient' % (K, dtype), SA.worst(grad.get('grad').double(), ref))
