"""GPU tests of the paired line convolution (csrc/gcn.hip): salt_gcn_pair and salt_gcn_pair_dgrad through the C-ABI against the float64
references of gcn_op_reference.py, elementwise and with no element excluded: both dtypes, x / dx contiguous and as the channel slice at
c0 = 8 of a wider buffer, yv / yh (dyv / dyh) as the [0, Cout) and [c1, c1 + Cout) slices of ONE buffer (c1 = Cout rounded up to 8: [0, 21)
and [24, 45) of 48 channels for the registry's 21) between sentinels, inputs verified unchanged, the eval epilogue with every part and
with none, ReLU on and off, the train form with its statistics partials, accumulate 0 and 1, bit-identical reruns, and the shapes the
contract refuses.

The kernel's tile is GCN_TH x GCN_TW = 8 x 16 pixels and 32 channels per contraction chunk / data-gradient workgroup: the last case of
gcn_op_reference.CASES spans 3 x 3 tiles with a ragged chunk, (2, 40, 36, ...) 5 x 3.  The bounds are derived in gcn_op_reference.py
(operands bf16-representable, 2^-23 sum |terms| per fp32 accumulation, 2^-8 per bf16 store)."""
import ctypes
import functools

import pytest
import torch

import abi_ops
import gcn_op_reference as GR
from abi_ops import Vec, raw, call, _abi, DEV, F64, SENTINEL
from gcn_op_reference import Wide

pytestmark = pytest.mark.gpu
CODE = {'f32': 0, 'bf16': 1}
_CASES, _REFS = {}, {}
RATIOS = {}          # {(case, dtype): {output: worst error / bound}}: the table of DESIGN 21
held = functools.partial(abi_ops.held, ratio=GR.ratio, ratios=RATIOS)
ids = ['x'.join(str(v) for v in s) for s in GR.CASES]


def case(shape):
    if shape not in _CASES:
        _CASES[shape] = GR.make_case(*shape, seed=900 + 7 * shape[1] + shape[3] + shape[5])
    return _CASES[shape]


def ref_of(key, make):
    """one float64 reference per (case, dtype, variant): computed once, shared, left unchanged"""
    if key not in _REFS:
        _REFS[key] = make()
    return _REFS[key]


def nan(*shape):
    return torch.full(shape, float('nan'), dtype=F64)


def dev(t):
    return t.float().contiguous().to(DEV)


def wide_x(data, dtype, sliced):
    """the wide operand: contiguous, or channels [8, 8 + C) of rows C + 16 wide"""
    B, H, W, C = data.shape
    return Wide(B, H, W, C + 16 if sliced else C, dtype, {'x': (8 if sliced else 0, data)})


def pair_y(a, b, dtype):
    """the two thin operands as slices [0, C) and [c1, c1 + C) of one buffer 2 c1 wide"""
    B, H, W, C = a.shape
    c1 = (C + 7) // 8 * 8
    return Wide(B, H, W, 2 * c1, dtype, {'v': (0, a), 'h': (c1, b)})


def run_fwd(shape, dtype, sliced, mode, relu=(0, 0)):
    abi = _abi()
    B, H, W, Cin, Cout, K = shape
    c = case(shape)
    what = 'gcn_pair %s %s sliced=%d %s relu=%s' % (shape, dtype, sliced, mode, relu)
    x, y = wide_x(c['x'], dtype, sliced), pair_y(nan(B, H, W, Cout), nan(B, H, W, Cout), dtype)
    x0 = x.buf.clone()
    wv, wh = dev(c['wv']), dev(c['wh'])
    vec = lambda key: [dev(t) for t in c[key]]
    kw = dict(dtype=CODE[dtype], x=x.view('x'), wv=wv.data_ptr(), wh=wh.data_ptr(), K=K, yv=y.view('v'), yh=y.view('h'), relu_v=relu[0], relu_h=relu[1])
    nparts = abi.lib.salt_gcn_pair_stats_parts(ctypes.byref(abi.fill(abi.STRUCTS['salt_gcn_pair_args'](), **kw)))
    assert nparts == B * -(-H // GR.GCN_TH) * -(-W // GR.GCN_TW), (what, nparts)
    keep = [wv, wh]
    stats = None
    if mode != 'plain':
        b = vec('bias'); keep += b
        kw.update(bias_v=b[0].data_ptr(), bias_h=b[1].data_ptr())
    if mode == 'eval':
        sc, sh = vec('scale'), vec('shift'); keep += sc + sh
        kw.update(scale_v=sc[0].data_ptr(), shift_v=sh[0].data_ptr(), scale_h=sc[1].data_ptr(), shift_h=sh[1].data_ptr())
    if mode == 'train':
        nfl = abi.lib.salt_bn_stats_floats(nparts, Cout)
        stats = [(Vec(nfl), Vec(nparts)) for _ in range(2)]
        kw.update(stats_v=stats[0][0].ptr(), stats_cnt_v=stats[0][1].ptr(), stats_h=stats[1][0].ptr(), stats_cnt_h=stats[1][1].ptr())
    call('salt_gcn_pair', **kw)
    x.check(what + ' x')
    y.check(what + ' y')
    assert torch.equal(x.buf.view(torch.int16), x0.view(torch.int16)), what + ': input changed'
    refs = ref_of(('fwd', shape, dtype, mode, relu), lambda: GR.fwd_ref(c, dtype, mode, relu))
    out = [y.get('v'), y.get('h')]
    for br, name in enumerate(('yv', 'yh')):
        held(out[br], refs[br], '%s %s' % (what, name), (shape, dtype), '%s %s' % (name, mode))
        if relu[br] and Cout >= 8:
            frac = float((out[br] > 0).double().mean())
            assert 0.2 <= frac <= 0.8, (what, name, frac)
        if stats is not None:
            st = stats[br][0].get((nfl,))[:nparts * 2 * Cout].reshape(nparts, 2, Cout)
            cnt = stats[br][1].get((nparts,))
            assert bool(torch.isfinite(st).all()) and bool((cnt > 0).all()), what + ': a partial was not written'
            n, s, q = abi_ops.merge_partials(st, cnt)
            abi_ops.check_moments('%s %s statistics' % (what, name), out[br], dtype, n, s, q)
            out.append(st)
    return out


def run_dgrad(shape, dtype, sliced, accumulate):
    B, H, W, Cin, Cout, K = shape
    c = case(shape)
    what = 'gcn_pair_dgrad %s %s sliced=%d acc=%d' % (shape, dtype, sliced, accumulate)
    dy = pair_y(c['dyv'], c['dyh'], dtype)
    dx = wide_x(c['dx_old'] if accumulate else nan(B, H, W, Cin), dtype, sliced)
    d0 = dy.buf.clone()
    wv, wh = dev(c['wv']), dev(c['wh'])
    call('salt_gcn_pair_dgrad', dtype=CODE[dtype], dyv=dy.view('v'), dyh=dy.view('h'), wv=wv.data_ptr(), wh=wh.data_ptr(), K=K, dx=dx.view('x'),
         accumulate=accumulate)
    dy.check(what + ' dy')
    dx.check(what + ' dx')
    assert torch.equal(dy.buf.view(torch.int16), d0.view(torch.int16)), what + ': input changed'
    got = dx.get('x')
    held(got, ref_of(('dgrad', shape, dtype, accumulate), lambda: GR.dgrad_ref(c, dtype, accumulate)), what, (shape, dtype),
         'dx acc' if accumulate else 'dx')
    return got


@pytest.mark.parametrize('shape', GR.CASES, ids=ids)
@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_gcn_pair_vs_fp64_reference(dtype, shape):
    for sliced in (0, 1):
        run_fwd(shape, dtype, sliced, 'eval', relu=(1, 0))
        run_fwd(shape, dtype, sliced, 'plain', relu=(0, 1))
        run_fwd(shape, dtype, sliced, 'train')
        for accumulate in (0, 1):
            run_dgrad(shape, dtype, sliced, accumulate)
    per = RATIOS[(shape, dtype)]
    print('worst error / bound of %s %s: %.3f  per output:' % (shape, dtype, max(per.values())), {k: round(v, 3) for k, v in sorted(per.items())})


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_reruns_are_bit_identical(dtype):
    """no atomics anywhere: two runs of both operators give the same bits, the statistics partials included"""
    shape = GR.CASES[-1]
    for a, b in ((run_fwd(shape, dtype, 1, 'train'), run_fwd(shape, dtype, 1, 'train')),
                 (run_fwd(shape, dtype, 0, 'eval', (1, 1)), run_fwd(shape, dtype, 0, 'eval', (1, 1)))):
        assert len(a) == len(b) and all(torch.equal(p, q) for p, q in zip(a, b))
    for accumulate in (0, 1):
        assert torch.equal(run_dgrad(shape, dtype, 1, accumulate), run_dgrad(shape, dtype, 1, accumulate))


def test_unsupported_shapes_fail_loudly_and_launch_nothing():
    abi = _abi()
    from salt_amd.engine import shaped_view
    UNS, BAD = abi.CONSTS['SALT_E_UNSUPPORTED'], abi.CONSTS['SALT_E_BADARG']

    def pair(op, Cin=32, Cout=21, K=9, dtype=0, off=0, ycs=48, h_cout=None, w=True):
        B, H, W = 1, 5, 6
        t = lambda n: torch.full((n,), SENTINEL, device=DEV)
        wide, thin, wt = t(B * H * W * Cin + 64), t(B * H * W * max(ycs, 2 * Cout) + 64), torch.zeros(33 * 2048 * 10, device=DEV)
        xv = shaped_view(wide.data_ptr() + off, B, H, W, Cin)
        yv, yh = shaped_view(thin.data_ptr(), B, H, W, Cout, ycs), shaped_view(thin.data_ptr() + 96, B, H, W, h_cout or Cout, ycs)
        wp = wt.data_ptr() if w else None
        if op == 'salt_gcn_pair':
            rc = raw(op, dtype=dtype, x=xv, wv=wp, wh=wp, K=K, yv=yv, yh=yh)
            return rc, bool((thin == SENTINEL).all())
        rc = raw(op, dtype=dtype, dyv=yv, dyh=yh, wv=wp, wh=wp, K=K, dx=xv, accumulate=0)
        return rc, bool((wide == SENTINEL).all())
    for op in ('salt_gcn_pair', 'salt_gcn_pair_dgrad'):
        assert pair(op) == (0, False)
        for kw in (dict(Cin=20), dict(Cin=2056), dict(Cout=33), dict(K=10), dict(K=1), dict(off=4), dict(ycs=46), dict(h_cout=16), dict(dtype=5)):
            assert pair(op, **kw) == (UNS, True) and abi.lib.salt_last_error(), (op, kw)
        assert pair(op, w=False) == (BAD, True)
    v, y = shaped_view(1 << 20, 2, 3, 3, 32), shaped_view(1 << 20, 2, 3, 3, 21, 24)
    st = dict(stats_v=1 << 20, stats_cnt_v=1 << 20, stats_h=1 << 20)
    assert raw('salt_gcn_pair', dtype=0, x=v, wv=1 << 20, wh=1 << 20, K=9, yv=y, yh=y, **st) == BAD                       # three of the four
    assert raw('salt_gcn_pair', dtype=0, x=v, wv=1 << 20, wh=1 << 20, K=9, yv=y, yh=y, stats_cnt_h=1 << 20, relu_v=1, **st) == BAD
    assert raw('salt_gcn_pair', dtype=0, x=v, wv=1 << 20, wh=1 << 20, K=9, yv=y, yh=y, scale_v=1 << 20) == BAD
