"""small_abi.py's float64 references and bounds, on the CPU: every reference is pinned against torch in double (F.conv2d, autograd,
F.pixel_unshuffle), the stem's three index maps against each other exactly on integer values (the space-to-depth identity and the
adjoint property), the case tables of small_abi.py (run on the GPU by test_gpu_small_abi.py) against the library's host-only queries (which kernel every case takes, part
counts, taps per thread), and an fp32 stand-in for a kernel passes the bounds on every case while six result-side mutations do not."""
import pytest
import torch
import torch.nn.functional as F

import conv_abi as CA
import small_abi as SA

F64 = torch.float64


def _close(a, b, rel=1e-12):
    assert a.shape == b.shape, (a.shape, b.shape)
    assert float((a - b).abs().max()) <= rel * max(1.0, float(b.abs().max()))


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


FIRST_FORMS = sorted({(c['K'], c['s'], c['p'], c['Cin'], c['H'], c['W']) for c in SA.FIRST_CASES})
WGRAD_FORMS = sorted({(c['K'], c['s'], c['p'], c['Cin'], c['H'], c['W']) for c in SA.WGRAD_CASES if c['kid'] >= 0 and c['B'] == 1})


# ---------------------------------------------------------------- references against torch
@pytest.mark.parametrize('K,s,p,Cin,H,W', FIRST_FORMS)
def test_conv_first_sum_is_conv2d(K, s, p, Cin, H, W):
    x, w = SA.mk(2, Cin, H, W, 1), SA.master_weight(7, Cin, K, K, Cin, K * K, 2)
    want = F.conv2d(x.double(), w.double(), stride=s, padding=p)
    v, A = SA.conv_first_sum(x, w, s, p)
    assert v.shape[1:3] == SA.first_geom(H, W, K, s, p)
    _close(v, _nhwc(want))
    _close(A, _nhwc(F.conv2d(x.double().abs(), w.double().abs(), stride=s, padding=p)))


def test_conv_first_epilogue_order_and_statistics():
    x, w = SA.mk(2, 3, 34, 38, 1), SA.master_weight(24, 3, 7, 7, 3, 49, 2)
    b, sc, sh = SA._vec(24, 3), SA._vec(24, 4, 'scale'), SA._vec(24, 5)
    v = _nhwc(F.conv2d(x.double(), w.double(), stride=2, padding=3))
    r = SA.conv_first_ref(x, w, 2, 3, 'bf16', b, sc, sh, True)
    _close(r['exact'], ((v + b) * sc + sh).clamp_min(0))
    assert bool((r['tol'] > r['pre_tol']).all()) and bool((r['pre_tol'] > 0).all())
    assert torch.equal(SA.conv_first_ref(x, w, 2, 3, 'f32', b)['tol'], SA.conv_first_ref(x, w, 2, 3, 'f32', b)['pre_tol'])
    st = SA.first_stats_ref(r['exact'], r['pre_tol'])
    assert st['cnt'].tolist() == [256.0, 48.0, 16.0, 3.0] * 2                # 17 x 19 outputs: image, tile row, tile column
    e = r['exact']
    for k, (b_, ys, xs) in enumerate((b_, ys, xs) for b_ in range(2) for ys in (slice(0, 16), slice(16, 17)) for xs in (slice(0, 16), slice(16, 19))):
        blk = e[b_, ys, xs].reshape(-1, 24)
        _close(st['stats'][k, 0], blk.sum(0))
        _close(st['stats'][k, 1], blk.var(0, unbiased=False) * blk.shape[0])
    assert bool((st['tol'] > 0).all())


@pytest.mark.parametrize('acc', [False, True])
@pytest.mark.parametrize('K,s,p,Cin,H,W', WGRAD_FORMS)
def test_conv_first_wgrad_is_autograd(K, s, p, Cin, H, W, acc):
    x = SA.mk(2, Cin, H, W, 3)
    OH, OW = SA.first_geom(H, W, K, s, p)
    dy = SA.mk(2, 6, OH, OW, 4)
    w = torch.zeros(6, Cin, K, K, dtype=F64, requires_grad=True)
    F.conv2d(x.double(), w, stride=s, padding=p).backward(dy.double())
    old = SA.mk(6, Cin, K, K, 5).double() if acc else None
    r = SA.conv_first_wgrad_ref(x, _nhwc(dy), K, s, p, old)
    _close(r['exact'], w.grad + old if acc else w.grad)
    assert bool((r['tol'] > 0).all())


@pytest.mark.parametrize('Cout', [1, 2, 3, 4])
def test_head_references_are_autograd(Cout):
    B, H, W, C = 2, 5, 7, 12
    x = _nhwc(SA.mk(B, C, H, W, 6)).double()
    w = SA.master_weight(Cout, C, 1, 1, C, 1, 7).reshape(Cout, C).double()
    bias, dy, old = SA._vec(Cout, 8), SA.mk(B, Cout, H, W, 9).double(), _nhwc(SA.mk(B, C, H, W, 10)).double()
    xr, wr, br = x.clone().requires_grad_(True), w.clone().requires_grad_(True), bias.clone().requires_grad_(True)
    y = F.conv2d(xr.permute(0, 3, 1, 2), wr.reshape(Cout, C, 1, 1), br)
    _close(SA.head_ref(x, w, bias)['exact'], _nhwc(y.detach()))
    _close(SA.head_ref(x, w, None, 'bf16')['exact'], _nhwc(y.detach()) - bias)
    y.backward(dy)
    r = SA.head_bwd_ref(x, w, dy, 'bf16')
    _close(r['dx']['exact'], xr.grad)
    _close(r['gw']['exact'], wr.grad)
    _close(r['gb']['exact'], br.grad)
    r2 = SA.head_bwd_ref(x, w, dy, 'bf16', old)
    _close(r2['dx']['exact'], xr.grad + old)
    assert bool((r2['dx']['tol'] > r['dx']['tol']).all())                    # the second storage rounding and the fp32 addition
    for k in ('dx', 'gw', 'gb'):
        assert bool((r[k]['tol'] > 0).all())


def test_head_parts_arithmetic():
    """At most 1024 parts, of at most 64 pixels until that cap binds; equal lengths, every pixel in exactly one part."""
    assert SA.head_parts(20) == 1 and SA.head_parts(64) == 1 and SA.head_parts(65) == 2 and SA.head_parts(129) == 3
    assert SA.head_parts(260 * 260) == 1009                                  # 1057 parts of 64 capped to 1024 -> 67 pixels each -> 1009
    for npix in (1, 63, 64, 65, 129, 680, 65536, 65537, 67600, 10 ** 6):
        n = SA.head_parts(npix)
        per = SA.cdiv(npix, n)
        assert n <= 1024 and (n - 1) * per < npix <= n * per and (per <= 64 or npix > 64 * 1024)


# ---------------------------------------------------------------- the stem's index maps
@pytest.mark.parametrize('Cin', [1, 2, 3, 4])
def test_s2d_is_pixel_unshuffle_with_the_headers_channel_order(Cin):
    x = SA._arbitrary((2, Cin, 6, 10), 11)
    z = SA.s2d_ref(x)
    pu = F.pixel_unshuffle(x, 2)                                             # channel c 4 + ph 2 + pw
    for c in range(Cin):
        for q in range(4):
            assert torch.equal(z[..., q * Cin + c], pu[:, c * 4 + q])       # header: (ph 2 + pw) Cin + c
    assert bool((z[..., 4 * Cin:] == 0).all())


def _ints(shape, seed, lo=-4, hi=5):
    return torch.randint(lo, hi, shape, generator=torch.Generator().manual_seed(seed)).double()


@pytest.mark.parametrize('K', [3, 5, 7])
@pytest.mark.parametrize('Cin', [1, 2, 3, 4])
def test_stem_identity_is_exact_on_integers(Cin, K):
    """conv (K + 1) / 2 squared taps, stride 1, with pack(w) over s2d(x) == conv2d(x, w, stride 2, padding K / 2)."""
    x, w = _ints((2, Cin, 12, 16), 12), _ints((5, Cin, K, K), 13)
    taps = SA.stem_taps(K)
    assert len(taps) == ((K + 1) // 2) ** 2
    v, _ = CA.conv_sum(SA.s2d_ref(x), SA.pack_stem_ref(w), taps, 1, 0, 6, 8)
    assert torch.equal(v, _nhwc(F.conv2d(x, w, stride=2, padding=K // 2)))
    assert torch.equal(v, SA.conv_first_sum(x, w, 2, K // 2)[0])
    wide = SA.pack_stem_ref(w, 32)
    assert torch.equal(wide[..., :16], SA.pack_stem_ref(w)) and bool((wide[..., 16:] == 0).all())


@pytest.mark.parametrize('K', [3, 5, 7])
@pytest.mark.parametrize('Cin', [1, 2, 3, 4])
def test_unfold_is_the_adjoint_of_pack(Cin, K):
    """<pack(w), g> == <w, unfold(g)>, and unfold(pack(w)) == w: every kernel element lies in exactly one (tap, phase)."""
    T_ = (K + 1) // 2
    w, g = _ints((5, Cin, K, K), 14), _ints((5, 16, T_, T_), 15)
    packed = SA.pack_stem_ref(w)                                             # [T T][Cout][16]
    as_g16 = packed.reshape(T_, T_, 5, 16).permute(2, 3, 0, 1)               # the gradient's [Cout][16][T][T] layout
    assert float((as_g16 * g).sum()) == float((w * SA.stem_unfold_ref(g, Cin, K)).sum())
    assert torch.equal(SA.stem_unfold_ref(as_g16.contiguous(), Cin, K), w)


# ---------------------------------------------------------------- the tables' own claims (host only, no launch)
def _unique(cases):
    names = [c['name'] for c in cases]
    assert len(names) == len(set(names))


def test_first_cases_take_the_store_path_they_name():
    _unique(SA.FIRST_CASES)
    for c in SA.FIRST_CASES:
        assert SA.first_vec(c) == c['vec'], c['name']
        y = SA.view(SA.FAKE, c['B'], 1, 1, c['Cout'], c['yv'][1])
        S = SA.first_args(c['dtype'], SA.FAKE, (c['B'], c['Cin'], c['H'], c['W']), SA.FAKE, c['K'], c['s'], c['p'], y)
        OH, OW = SA.first_geom(c['H'], c['W'], c['K'], c['s'], c['p'])
        assert 16 < OH <= 32 and 16 < OW <= 32, 'ragged 2 x 2 tiles'
        assert SA.query('salt_conv_first_stats_parts', S) == 4 * c['B']
    # the predicate's three terms fail one at a time
    by = {c['name']: c for c in SA.FIRST_CASES}
    for dt, es in (('f32', 4), ('bf16', 2)):
        c0, cs = by[dt + '-y-slice-cs-odd']['yv']
        assert cs % SA.VE[dt] != 0 and c0 == 0
        c0, cs = by[dt + '-y-slice-misaligned']['yv']
        assert cs % SA.VE[dt] == 0 and (c0 * es) % 16 != 0
        c0, cs = by[dt + '-y-slice-aligned']['yv']
        assert cs % SA.VE[dt] == 0 and (c0 * es) % 16 == 0 and c0 > 0


@pytest.mark.parametrize('dtype', SA.DTYPES)
def test_wgrad_cases_land_on_the_instantiation_they_name(dtype):
    _unique(SA.WGRAD_CASES)
    seen = set()
    for c in SA.WGRAD_CASES:
        S = SA.wg_plan(c, dtype)
        kid = SA.query('salt_conv_first_wgrad_kernel_id', S)
        assert kid == c['kid'], '%s: id %d (%s)' % (c['name'], kid, SA.last_error() if kid < 0 else 'ok')
        if kid < 0:
            continue
        seen.add(kid)
        nparts, n = SA.wg_nparts(c), c['Cout'] * c['Cin'] * c['K'] * c['K']
        assert SA.query('salt_conv_first_wgrad_parts', S) == nparts
        assert bool(kid & SA.WIDE) == (nparts >= 64 and n <= 4096), c['name']
        kkc = c['Cin'] * c['K'] * c['K']
        if kid & 255 == SA.MFMA:
            assert c['Cout'] % 16 == 0 and kkc <= 16
        else:
            groups = 256 // c['Cout']
            assert SA.cdiv(kkc, groups) == c['per'] <= (kid & 255), c['name']
            assert c['per'] > {1: 0, 4: 1, 12: 4, 40: 12}[kid & 255], 'the smallest instantiation that holds `per`'
    assert seen == {0, 1, 4, 12, 40, 256, 257}
    by = {c['name']: c for c in SA.WGRAD_CASES}
    assert SA.wg_nparts(by['nparts63-narrow']) == 63 and SA.wg_nparts(by['nparts64-wide']) == 64 and SA.wg_nparts(by['nparts320-wide']) == 320
    assert 256 - 144 == 112 and 256 // 144 == 1 and 256 // 128 == 2 and 256 % 128 == 0


def test_head_cases_land_on_the_kernel_they_name():
    _unique(SA.HEAD_CASES)
    seen = set()
    for c in SA.HEAD_CASES + [SA.HEAD_GRID_CAP]:
        for out in ('nchw', 'view'):
            kid = SA.query('salt_head1x1_kernel_id', SA.head_plan(c, out))
            assert kid == c['kid'], '%s: kernel %d' % (c['name'], kid)
        cpv = c['C'] // SA.VE[c['dtype']] if c['C'] % SA.VE[c['dtype']] == 0 else None
        seen.add((c['dtype'], c['kid'], cpv))
    for dt in SA.DTYPES:
        for kid in (SA.HEAD_VEC, SA.HEAD_VEC_CO2):
            assert {(dt, kid, 1), (dt, kid, 8), (dt, kid, 64)} <= seen
        assert (dt, SA.HEAD_SCALAR, 3) in seen and (dt, SA.HEAD_SCALAR, 128) in seen and (dt, SA.HEAD_SCALAR, None) in seen
    c = SA.HEAD_GRID_CAP
    units = c['B'] * c['H'] * c['W'] * (c['C'] // 8)
    assert 4096 < SA.cdiv(units, 256) < 2 * 4096 and c['B'] * c['H'] * c['W'] * c['C'] * 2 < 20 << 20
    assert SA.query('salt_head1x1_kernel_id', SA.head_args('f32', SA.view(SA.FAKE, 1, 2, 2, 8, 8), SA.FAKE, None, 5, y_nchw=SA.FAKE)) == -1


def test_head_bwd_cases_land_on_the_kernel_they_name():
    _unique(SA.HEAD_BWD_CASES)
    parts = set()
    for c in SA.HEAD_BWD_CASES:
        S = SA.hb_plan(c, 0, True)
        npix = c['B'] * c['H'] * c['W']
        assert S.nparts == SA.head_parts(npix), c['name']
        parts.add(S.nparts)
        kid = SA.query('salt_head1x1_bwd_kernel_id', S)
        assert kid == c['kid'], '%s: kernel %d (%s)' % (c['name'], kid, SA.last_error() if kid < 0 else 'ok')
        assert SA.query('salt_head1x1_bwd_kernel_id', SA.hb_plan(c, 1, False, nparts=S.nparts + 1)) == -1
        if kid == SA.HEAD_VEC:
            assert c['C'] % SA.VE[c['dtype']] == 0 and c['C'] // SA.VE[c['dtype']] <= 256
    assert {1, 3, 11, 1009} <= parts


# ---------------------------------------------------------------- the bounds let an fp32 implementation pass ...
def _st(dtype):
    return (lambda t: t.bfloat16().float()) if dtype == 'bf16' else (lambda t: t)


@pytest.mark.parametrize('c', SA._ids(SA.FIRST_CASES))
def test_conv_first_bound_lets_fp32_pass(c):
    """torch's fp32 convolution (another order than the reference's), fp32 epilogue, one storage rounding; the statistics from the
    unrounded fp32 values with torch's fp32 sums."""
    o = SA.first_build(c)
    y = F.conv2d(o['x'], o['w'], stride=c['s'], padding=c['p']).permute(0, 2, 3, 1)
    if c['bias']:
        y = y + o['bias'].float()
    if c['scale']:
        y = y * o['scale'].float() + o['shift'].float()
    if c['relu']:
        y = y.clamp_min(0)
    assert SA.ratio(_st(c['dtype'])(y), o['ref']) <= 1.0
    if c['stats']:
        sr = SA.first_stats_ref(o['ref']['exact'], o['ref']['pre_tol'])
        k = 0
        for b in range(c['B']):
            for i in range(2):
                for j in range(2):
                    blk = y[b, 16 * i:16 * i + 16, 16 * j:16 * j + 16].reshape(-1, c['Cout'])
                    s = blk.sum(0)
                    d = blk - s / blk.shape[0]
                    got = torch.stack([s, (d * d).sum(0)]).double()
                    assert float(((got - sr['stats'][k]).abs() / sr['tol'][k]).max()) <= 1.0
                    k += 1


@pytest.mark.parametrize('dtype', SA.DTYPES)
@pytest.mark.parametrize('c', SA._ids([c for c in SA.WGRAD_CASES if c['kid'] >= 0]))
def test_conv_first_wgrad_bound_lets_fp32_pass(c, dtype):
    o = SA.wg_build(c, 1)
    w = torch.zeros(c['Cout'], c['Cin'], c['K'], c['K'], requires_grad=True)
    F.conv2d(o['x'], w, stride=c['s'], padding=c['p']).backward(o['dy'].permute(0, 3, 1, 2))
    assert SA.worst((w.grad + o['old'].float()).double(), o['ref']) <= 1.0


@pytest.mark.parametrize('c', SA._ids(SA.HEAD_CASES))
def test_head_bound_lets_fp32_pass(c):
    o = SA.head_build(c)
    y = o['x'].matmul(o['w'].t()) + o['bias'].float()
    assert SA.ratio(y, SA.head_ref(o['x'].double(), o['w'].double(), o['bias'])) <= 1.0
    assert SA.ratio(_st(c['dtype'])(y), SA.head_ref(o['x'].double(), o['w'].double(), o['bias'], c['dtype'])) <= 1.0


@pytest.mark.parametrize('c', SA._ids([c for c in SA.HEAD_BWD_CASES if c['H'] < 100]))
def test_head_bwd_bound_lets_fp32_pass(c):
    o = SA.hb_build(c, 1)
    st = _st(c['dtype'])
    g = o['dy'].permute(0, 2, 3, 1)
    dx = st(st(g.matmul(o['w'])) + o['old'])                                 # the new term rounded before the old one is added: allowed
    assert SA.ratio(dx, o['ref']['dx']) <= 1.0
    assert SA.ratio(st(g.matmul(o['w']) + o['old']), o['ref']['dx']) <= 1.0  # ... and added in fp32, as the kernels do
    assert SA.worst(torch.einsum('bhwo,bhwc->oc', g, o['x']).double(), o['ref']['gw']) <= 1.0
    assert SA.worst(g.sum((0, 1, 2)).double(), o['ref']['gb']) <= 1.0


# ---------------------------------------------------------------- ... and reject a wrong result
@pytest.mark.parametrize('dtype', SA.DTYPES)
def test_bounds_reject_wrong_results(dtype):
    st = _st(dtype)
    c = next(c for c in SA.FIRST_CASES if c['name'] == dtype + '-bias-cout10')
    o = SA.first_build(c)
    ref = o['ref']
    assert SA.ratio(st(ref['exact'].float()), ref) <= 1.0
    got = ref['exact'].clone()
    got[..., 9] -= o['bias'][9]                                              # the bias of the last channel of the ragged block
    assert SA.ratio(st(got.float()), ref) > 1.0
    got = ref['exact'].clone()
    got[0, 0, 0] -= o['w'][:, 2, 6, 6].double() * float(o['x'][0, 2, 3, 3])  # the last tap at the corner pixel
    assert SA.ratio(st(got.float()), ref) > 1.0
    # weight gradient: pixel 255 of the first tile left out
    c = next(c for c in SA.WGRAD_CASES if c['name'] == 'per4-cout24-cin3-k3')
    o = SA.wg_build(c, 0)
    dy = o['dy'].clone()
    dy[0, 15, 15] = 0
    bad = SA.conv_first_wgrad_ref(o['x'], dy, c['K'], c['s'], c['p'])['exact']
    assert SA.worst(bad.float().double(), o['ref']) > 1.0 and SA.worst(o['ref']['exact'].float().double(), o['ref']) <= 1.0
    # head backward: every fourth pixel missing from gb; one output's term missing from dx at one pixel
    c = next(c for c in SA.HEAD_BWD_CASES if c['name'] == dtype + '-vec-cpv8-ragged-part')
    o = SA.hb_build(c, 0)
    g = o['dy'].double().permute(0, 2, 3, 1).reshape(-1, c['Cout'])
    assert SA.worst((g.sum(0) - g[3::4].sum(0)).float().double(), o['ref']['gb']) > 1.0
    dx = o['ref']['dx']['exact'].clone()
    dx[0, 0, 0] -= g[0, 3] * o['w'][3].double()
    assert SA.ratio(st(dx.float()), o['ref']['dx']) > 1.0
