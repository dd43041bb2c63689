"""CPU tests of the scSE operator reference tests/scse_op_reference.py, the yardstick of tests/test_gpu_scse.py: the hand-derived backward
against float64 autograd of the oracle's module composition, the BatchNorm-backward sums against autograd of a BatchNorm(+ReLU) layer in
front, the bit-exact input transform against integer arithmetic, the fitness of the GPU case table for a bound without exclusions, and
the storage allowance of a dx that is stored twice."""
from fractions import Fraction

import pytest
import torch
import torch.nn.functional as F

import scse_op_reference as SR

F64 = torch.float64
tol = lambda ref: 1e-12 * max(1.0, float(ref.abs().max()))


@pytest.mark.parametrize('shape', [(2, 1, 1, 16, 1), (3, 3, 5, 8, 3), (2, 4, 6, 32, 5)], ids=lambda s: 'x'.join(str(v) for v in s))
@pytest.mark.parametrize('old', [0, 1])
def test_backward_equals_autograd_of_the_module_composition_in_double(shape, old):
    c = SR.make_case(*shape, seed=7, dtype='f32')
    p = SR.params(c, 'plain')
    a = c['x'].clone().requires_grad_(True)
    leaves = [t.clone().requires_grad_(True) for t in p]
    y = SR.module_composition(a, *leaves)
    y.backward(c['dy'])
    f = SR.scse(c['x'], *p)
    assert float((f.y - y.detach()).abs().max()) <= tol(y.detach())
    b = SR.scse_bwd(f, c['dy'], c['x'], p[0], p[2], p[4], dx_old=c['dx_old'] if old else None)
    want = a.grad + c['dx_old'] if old else a.grad
    assert float((b['dx'] - want).abs().max()) <= tol(want)
    for k, leaf in zip(('g_w1', 'g_b1', 'g_w2', 'g_b2', 'g_ws', 'g_bs'), leaves):
        assert b[k].shape == leaf.grad.shape and float((b[k] - leaf.grad).abs().max()) <= tol(leaf.grad), k
    # the pieces the operator stores separately add up: dx = dx_direct + dgap (+ old), and skip_bcast leaves exactly dgap out
    s = SR.scse_bwd(f, c['dy'], c['x'], p[0], p[2], p[4], skip_bcast=True, dx_old=c['dx_old'] if old else None)
    assert float((s['dx'] + s['dgap'][:, None, None, :] - b['dx']).abs().max()) <= tol(b['dx'])
    assert float(b['g_w1'].abs().max()) > 0 and float(b['dgap'].abs().max()) > 0


@pytest.mark.parametrize('relu', [0, 1])
@pytest.mark.parametrize('shape', [(2, 1, 1, 16, 1), (3, 3, 5, 8, 3), (2, 4, 6, 32, 5)], ids=lambda s: 'x'.join(str(v) for v in s))
def test_finalize_and_bnb_sums_equal_autograd_of_a_batchnorm_in_front(shape, relu):
    c = SR.make_case(*shape, seed=11, dtype='f32')
    mode = 'fin%d' % relu
    p = SR.params(c, mode)
    S, Q, N = SR.stats64(c['x_raw'])
    fin = SR.bn_finalize64(S, Q, N, c['gamma'], c['beta'], SR.EPS, SR.MOMENTUM, (c['running_mean'], c['running_var']))
    x = c['x_raw'].clone().requires_grad_(True)
    gamma, beta = c['gamma'].clone().requires_grad_(True), c['beta'].clone().requires_grad_(True)
    rm, rv = c['running_mean'].clone(), c['running_var'].clone()
    z = F.batch_norm(x.permute(0, 3, 1, 2), rm, rv, gamma, beta, True, SR.MOMENTUM, SR.EPS).permute(0, 2, 3, 1)
    a = torch.relu(z) if relu else z
    SR.module_composition(a, *p).backward(c['dy'])
    ad = a.detach()
    assert float((c['x_raw'] * fin.scale + fin.shift - z.detach()).abs().max()) <= tol(z.detach())
    assert float((fin.running_mean - rm).abs().max()) <= tol(rm) and float((fin.running_var - rv).abs().max()) <= tol(rv)
    assert float((fin.invstd - 1 / torch.sqrt(c['x_raw'].reshape(-1, shape[3]).var(0, unbiased=False) + SR.EPS)).abs().max()) <= 1e-9 * float(fin.invstd.max())
    f = SR.scse(ad, *p)
    b = SR.scse_bwd(f, c['dy'], ad, p[0], p[2], p[4], skip_bcast=True)
    on = (z.detach() > 0) if relu else None
    s1, s2 = SR.bnb_sums(c['x_raw'], on, b['dx'], b['dgap'], fin.mean, fin.invstd)
    assert float((s1 - beta.grad).abs().max()) <= tol(beta.grad) and float((s2 - gamma.grad).abs().max()) <= 1e-10 * max(1.0, float(gamma.grad.abs().max()))
    i1, i2 = SR.bnb_sums(c['x_raw'], on, b['dx'], b['dgap'], fin.mean, fin.invstd, per_image=True)
    assert i1.shape == (shape[0], shape[3]) and float((i1.sum(0) - s1).abs().max()) <= tol(s1) and float((i2.sum(0) - s2).abs().max()) <= tol(s2)
    assert float(s1.abs().max()) > 0 and float(s2.abs().max()) > 0


def _rne(v, p):
    """Fraction -> the nearest value of p significant bits (ties to even; exponents stay far from the format's limits here)"""
    if v == 0:
        return v
    m = abs(v)
    e = m.numerator.bit_length() - m.denominator.bit_length()
    e -= 1 if Fraction(2) ** e > m else 0
    q = Fraction(2) ** (e - p + 1)
    n = m / q
    fl = n.numerator // n.denominator
    rem = n - fl
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and fl % 2 == 1):
        fl += 1
    return (fl * q) * (1 if v > 0 else -1)


def _exact(x, sc, sh, relu, dtype):
    v = _rne(Fraction(x) * Fraction(sc) + Fraction(sh), 24)
    pre = v
    if relu and v < 0:
        v = Fraction(0)
    return float(_rne(v, 8) if dtype == 'bf16' else v), float(pre)


def test_transform_exact_agrees_with_integer_arithmetic():
    f = lambda v: float(torch.tensor(v, dtype=F64).float())
    crafted = [
        (3.0, 1 + 2.0 ** -23, 0.0),                    # the product sits on a float32 tie: to even (down)
        (3.0, 1 + 3 * 2.0 ** -23, 0.0),                # the next tie: to even (up)
        (1.0, 1.0, 2.0 ** -8), (1.0, 1.0, 2.0 ** -7 + 2.0 ** -8),       # bf16 ties, down and up
        (1.0, 1 + 2.0 ** -8, 2.0 ** -30),              # rounds to a bf16 tie in float32 first: 1.0, where ONE rounding to bf16 gives 1 + 2**-7
        (-0.0, 1.5, -0.0), (-0.0, 1.5, 0.25), (2.0, 0.5, -1.0),          # negative zero, and an exact cancellation
        (1.0, 1.0, -1 + 2.0 ** -20), (1.0, 1.0, -1 - 2.0 ** -20),        # a hair above and below zero at the ReLU
        (-1.5, 0.75, 1.125), (1.5, -0.75, 1.125), (0.5, 2.0 ** -100, -2.0 ** -100),
    ]
    g = torch.Generator().manual_seed(5)
    for dtype in ('bf16', 'f32'):
        st = (lambda t: t.bfloat16().double()) if dtype == 'bf16' else (lambda t: t.float().double())
        rx, rs, rh = st(torch.randn(400, generator=g, dtype=F64)), torch.randn(400, generator=g, dtype=F64).float(), torch.randn(400, generator=g, dtype=F64).float()
        xs = torch.cat([st(torch.tensor([t[0] for t in crafted], dtype=F64)), rx])
        sc = torch.cat([torch.tensor([t[1] for t in crafted], dtype=F64).float(), rs])
        sh = torch.cat([torch.tensor([t[2] for t in crafted], dtype=F64).float(), rh])
        for relu in (0, 1):
            a, pre, doubt = [], [], []
            for i in range(xs.numel()):                                     # one channel per operand triple
                s = SR.transform_exact(xs[i].reshape(1, 1), sc[i].reshape(1), sh[i].reshape(1), relu, dtype)
                a.append(float(s.a)), pre.append(float(s.pre)), doubt.append(bool(s.doubtful))
            assert not any(doubt), (dtype, relu)
            for i in range(xs.numel()):
                wa, wp = _exact(float(xs[i]), float(sc[i]), float(sh[i]), relu, dtype)
                assert a[i] == wa and pre[i] == wp and (pre[i] > 0) == (wp > 0), (dtype, relu, i, a[i], wa)
    assert SR.transform_exact(torch.tensor([[1.0]], dtype=F64), torch.tensor([1 + 2.0 ** -8]), torch.tensor([2.0 ** -30]), 0, 'bf16').a.item() == 1.0
    # float32 operands whose exact multiply-add needs more than 53 bits and sits a hair above a float32 midpoint: the float64 evaluation
    # lands ON the midpoint and rounds to even (1.0) where the fused multiply-add gives 1 + 2**-23 - reported, not decided
    x, s, h = -2.0 ** -24 * (1 + 2.0 ** -23), 1 - 2.0 ** -23, 1 + 2.0 ** -23
    assert f(x) == x and f(s) == s and f(h) == h
    seen = SR.transform_exact(torch.tensor([[x]], dtype=F64), torch.tensor([s], dtype=F64).float(), torch.tensor([h], dtype=F64).float(), 0, 'f32')
    assert _exact(x, s, h, 0, 'f32')[0] == 1 + 2.0 ** -23 and seen.a.item() == 1.0 and bool(seen.doubtful)
    killed = SR.transform_exact(torch.tensor([[-x]], dtype=F64), torch.tensor([s], dtype=F64).float(), torch.tensor([-h], dtype=F64).float(), 1, 'f32')
    assert killed.a.item() == 0.0 and not bool(killed.doubtful)


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
@pytest.mark.parametrize('name', sorted(SR.CASES))
def test_case_table_is_fit_for_a_bound_without_exclusions(name, dtype):
    """No zero in x, every hidden pre-activation at least 100 bands (4 e32 + 1e-6 max) from zero, a live and a dead hidden unit over the
    batch, half of either gate inside (0.1, 0.9) - for the plain input and for both transformed ones - at the table's seed, which is the
    first such seed.  With gate_c + gate_s > 0 the sign of y is the sign of the input: every ReLU decision follows from the input alone."""
    B, H, W, C, R = SR.CASES[name][dtype]
    ve = 8 if dtype == 'bf16' else 4
    assert C % ve == 0 and (C // ve) & (C // ve - 1) == 0 and C // ve <= 64 and B * H * W * C <= 70000
    c = SR.make_case(B, H, W, C, R, SR.SEEDS[(name, dtype)], dtype)
    fit = SR.fitness(c)
    print(name, dtype, fit)
    assert fit['ok'] and fit['margin'] >= 100, fit
    assert SR.find_seed(name, dtype, SR.SEEDS[(name, dtype)] + 1) == SR.SEEDS[(name, dtype)]
    st = (lambda t: t.bfloat16().double()) if dtype == 'bf16' else (lambda t: t.float().double())
    for k in ('x', 'dy', 'dx_old', 'x_raw'):
        assert torch.equal(st(c[k]), c[k]), k
    for m in SR.MODES:
        p = SR.params(c, m)
        assert all(torch.equal(t.float().double(), t) for t in p)
        f = SR.scse(c['a'][m], *p)
        assert bool(((f.y > 0) == (c['a'][m] > 0)).all())


def test_a_dx_stored_twice_needs_the_allowance_of_both_roundings():
    """bf16 keeps 8 significant bits: one round-to-nearest costs up to 2**-8 of the value ROUNDED.  With the broadcast pass dx is stored
    as round(dx_direct), read back and stored again as round(. + dgap), so in exact arithmetic the error reaches
    2**-8 (|dx - dgap| + |dx|) - more than 2**-8 |dx| wherever dgap cancels part of dx_direct.  storage_allowance is that sum; the
    single-rounding form holds for every output stored once."""
    worst = 0.0
    for name in ('one-lane', 'ragged-parts', 'whole-wave'):
        c = SR.make_case(*SR.CASES[name]['bf16'], SR.SEEDS[(name, 'bf16')], 'bf16')
        p = SR.params(c, 'plain')
        f = SR.scse(c['x'], *p)
        b = SR.scse_bwd(f, c['dy'], c['x'], p[0], p[2], p[4])
        once = b['dx_direct'].bfloat16().double()
        twice = (once + b['dgap'][:, None, None, :]).bfloat16().double()
        err = (twice - b['dx']).abs()
        assert bool(((once - b['dx_direct']).abs() <= SR.storage_allowance(b['dx_direct'])).all())
        assert int((err > SR.storage_allowance(b['dx'])).sum()) > 0                        # the single-rounding form cannot hold here
        both = SR.storage_allowance(b['dx'], b['dx'] - b['dgap'][:, None, None, :])
        assert bool((err <= both).all())
        worst = max(worst, float((err / both).max()))
    assert 0.5 < worst <= 1.0                       # and the allowance of both is not slack
