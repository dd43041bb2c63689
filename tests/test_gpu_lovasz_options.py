"""Operator-level tests of the Lovasz options through the C-ABI (salt_lovasz_hinge / salt_lovasz_softmax with `flags`, `ignore`,
`ws_flat`, `ws_present`): batch-flat rows, the long-row sort, void labels, only-present.  Every output has a NaN guard word one past its
end and a forward-only call leaves the gradient buffer alone.  Inputs are dyadic (lovasz_options_reference.py), so every error is exact
in fp32 and the stable order is the only valid one.

Bars: against float64 the project's own for this operation sequence (test_gpu_ops_loss.py, test_gpu_softmax_loss.py) - loss
2e-5 max(1, |ref|), gradient 5e-3 max|ref| (the fp32 cancellation of g_k = J_k - J_(k-1)).  Nobody measured the loss bar on rows above
32768 elements: there it is the larger of 2e-5 max(1, |ref|) and 4 x the error of the fp32 closed form evaluated on the CPU (the factor
covers a different summation tree); both errors are printed.

The gradient bar can hold only while 2^-23 G <= 5e-3 (G the positives of a row: g_k = J_k - J_(k-1) is off by up to 2^-23 in fp32 whatever
the row length, the largest gradient is 1 / G), so the cases carry one positive label in eight (lovasz_options_reference.POSITIVE_ONE_IN,
with the reasoning); with one in two, rows of 131072 elements and more sat at 5.8e-3 in every form of the sort, the old ones included.
Between two forms of the sort: gradients bit for bit, losses within 2e-6
(test_lovasz_split_sort_equals_single_workgroup_sort)."""
import pytest
import torch

import lovasz_options_reference as LR
from abi_ops import _abi, call, raw, DEV, F64, NAN

pytestmark = pytest.mark.gpu

FLAT, PRESENT, IGNORE = 1, 2, 4
SCALE = 0.5
GARBAGE = 0x55555555
_REF = {}


def ref(key, fn):
    """a float64 (or fp32 yardstick) result computed once and shared between the tests (never modified)"""
    if key not in _REF:
        _REF[key] = fn()
    return _REF[key]


def _guarded(n):
    return torch.full((n + 1,), NAN, device=DEV)


def _words(n):
    return torch.full((max(1, n),), GARBAGE, dtype=torch.int32, device=DEV)


def _shape(kind, flags, B, C, HW):
    if kind == 'hinge':
        return (1, B * C * HW) if flags & FLAT else (B, C * HW)
    return (C, B * HW) if flags & FLAT else (B * C, HW)


class Op:
    """one launch configuration of salt_lovasz_hinge (x, t [B,P]) or salt_lovasz_softmax (x, t [B,C,HW]) on device copies of x and t"""

    def __init__(self, kind, x, t, flags=0, ignore=0.0, scale=SCALE, split=True, flat_ws=True):
        abi = _abi()
        self.kind, self.flags = kind, flags
        self.xd, self.td = x.float().to(DEV).contiguous(), t.float().to(DEV).contiguous()
        if kind == 'hinge':
            B, P = x.shape
            C, HW = 1, P
        else:
            B, C, HW = x.shape
        n_el = B * C * HW
        rows, n = _shape(kind, flags, B, C, HW)
        self.wk, self.wv = _words(2 * n_el), _words(2 * n_el)
        sw, fw = int(abi.lib.salt_lovasz_split_words(n)), int(abi.lib.salt_lovasz_flat_words(n))
        assert (sw > 0) == (4096 <= n <= 131072) and (fw > 0) == (n > 131072), 'the shortest form that fits the row'
        self.ws = _words(rows * sw) if split else None
        self.wf = _words(rows * fw) if flat_ws else None
        self.wp = _words(B * C)
        self.rows_out, self.loss, self.grad = _guarded(B * C if kind == 'softmax' else B), _guarded(1), _guarded(n_el)
        kw = dict(B=B, ws_keys=self.wk.data_ptr(), ws_vals=self.wv.data_ptr(), loss=self.loss.data_ptr(), loss_scale=scale,
                  ws_split=self.ws.data_ptr() if split else None, flags=flags, ignore=ignore, ws_flat=self.wf.data_ptr() if flat_ws else None)
        if kind == 'hinge':
            kw.update(logits=self.xd.data_ptr(), target=self.td.data_ptr(), P=P, loss_per_image=self.rows_out.data_ptr())
        else:
            kw.update(probas=self.xd.data_ptr(), target=self.td.data_ptr(), C=C, HW=HW, loss_per_row=self.rows_out.data_ptr(),
                      ws_present=self.wp.data_ptr())
        self.kw, self.name = kw, 'salt_lovasz_hinge' if kind == 'hinge' else 'salt_lovasz_softmax'
        self.gkey = 'dlogits' if kind == 'hinge' else 'dprobas'

    def run(self, with_grad=True):
        """-> (loss, gradient on the device in the shape of x, or None)"""
        self.grad.fill_(NAN)
        call(self.name, **dict(self.kw, **{self.gkey: self.grad.data_ptr() if with_grad else None}))
        assert bool(torch.isnan(self.rows_out[-1])) and bool(torch.isnan(self.loss[-1])) and bool(torch.isnan(self.grad[-1])), 'one past the end'
        if not with_grad:
            assert bool(torch.isnan(self.grad).all()), 'a forward-only call leaves the gradient alone'
            return float(self.loss[0]), None
        return float(self.loss[0]), self.grad[:-1].reshape(self.xd.shape).clone()


def _check64(what, loss, grad, lref, gref, n, l32=None):
    bar = 2e-5 * max(1.0, abs(lref))
    if n > 32768:
        e32 = abs(l32 - lref)
        print('%s: fp32 closed form on the CPU is %.3e from float64' % (what, e32))
        bar = max(bar, 4 * e32)
    gerr, gmx = float((grad.cpu().to(F64) - gref).abs().max()), float(gref.abs().max())
    print('%s: loss %.8f ref %.8f err %.3e (bar %.3e); gradient err %.3e, max|ref| %.3e, ratio %.3e' % (
        what, loss, lref, abs(loss - lref), bar, gerr, gmx, gerr / gmx if gmx else 0.0))
    assert abs(loss - lref) <= bar, (what, loss, lref, bar)
    assert bool(torch.isfinite(grad).all()) and gerr <= 5e-3 * gmx, '%s: gradient err %.3e > 5e-3 x %.3e' % (what, gerr, gmx)


# ---------------------------------------------------------------- 1, 2: batch-flat rows against float64 and against the predecessor
@pytest.mark.parametrize('N,B,P', LR.FLAT_SIZES)
def test_flat_hinge(N, B, P):
    z, t = LR.hinge_case(B, P)
    lref, gref = ref(('hinge flat', N), lambda: LR.hinge(z, t, per_image=False, loss_scale=SCALE))
    l32 = ref(('hinge flat 32', N), lambda: LR.hinge(z, t, per_image=False, loss_scale=SCALE, dtype=torch.float32)[0]) if N > 32768 else None
    op = Op('hinge', z, t, FLAT)
    loss, grad = op.run()
    assert op.run(False)[0] == loss
    _check64('flat hinge N=%d' % N, loss, grad, lref, gref, N, l32)


@pytest.mark.parametrize('N,B,P', LR.FLAT_SIZES)
def test_flat_hinge_equals_one_workgroup(N, B, P):
    """the parent's only route for this row: one workgroup over the same memory"""
    z, t = LR.hinge_case(B, P)
    loss, grad = Op('hinge', z, t, FLAT).run()
    old = Op('hinge', z.reshape(1, N), t.reshape(1, N), 0, split=False, flat_ws=False)
    lold, gold = old.run()
    assert torch.equal(grad.reshape(-1), gold.reshape(-1)), 'N=%d: gradients differ from the one-workgroup kernel' % N
    assert abs(loss - lold) <= 2e-6 * max(1.0, abs(lold)), (loss, lold)
    if B == 1:                                                   # a per-image call of a long row takes the long-row form too
        lpi, gpi = Op('hinge', z, t, 0).run()
        assert lpi == loss and torch.equal(gpi, grad)


@pytest.mark.parametrize('N,B,HW', LR.FLAT_SIZES)
def test_flat_softmax(N, B, HW):
    C = LR.SOFTMAX_C
    p, t = LR.softmax_case(B, C, HW)
    lref, gref = ref(('softmax flat', N), lambda: LR.softmax(p, t, per_image=False, loss_scale=SCALE))
    l32 = ref(('softmax flat 32', N), lambda: LR.softmax(p, t, per_image=False, loss_scale=SCALE, dtype=torch.float32)[0]) if N > 32768 else None
    loss, grad = Op('softmax', p, t, FLAT).run()
    e0 = ((t > 0.5).to(F64) - p) == 0
    assert bool((grad.cpu()[e0] == 0).all()), 'the gradient is exactly 0 where the error is 0'
    _check64('flat softmax N=%d' % N, loss, grad, lref, gref, N, l32)


@pytest.mark.parametrize('N,B,HW', LR.FLAT_SIZES)
def test_flat_softmax_equals_one_workgroup(N, B, HW):
    """the rows of class c gathered into contiguous planes [1,C,N], per image, one workgroup each"""
    C = LR.SOFTMAX_C
    p, t = LR.softmax_case(B, C, HW)
    loss, grad = Op('softmax', p, t, FLAT).run()
    gather = lambda a: a.permute(1, 0, 2).reshape(1, C, N)
    lold, gold = Op('softmax', gather(p), gather(t), 0, split=False, flat_ws=False).run()
    assert torch.equal(gather(grad), gold), 'N=%d: gradients differ from the one-workgroup kernel on the gathered rows' % N
    assert abs(loss - lold) <= 2e-6 * max(1.0, abs(lold)), (loss, lold)


# ---------------------------------------------------------------- 3: void handling equals compaction
def _compacted(z, t, flat, scale=SCALE):
    """the operator without `ignore` on the host-compacted valid elements of every row -> (loss, gradient scattered back, zeros elsewhere)"""
    B, P = z.shape
    zr, tr = (z.reshape(1, -1), t.reshape(1, -1)) if flat else (z, t)
    R = zr.shape[0]
    grad = torch.zeros(zr.shape, dtype=torch.float32)
    total = 0.0
    for r in range(R):
        valid = tr[r] != LR.VOID
        nv = int(valid.sum())
        if nv == 0:
            continue
        l, g = Op('hinge', zr[r][valid].reshape(1, nv), tr[r][valid].reshape(1, nv), 0, scale=scale / R).run()
        total += l
        grad[r, valid] = g.cpu().reshape(-1)
    return total, grad.reshape(B, P)


@pytest.mark.parametrize('B,P,void,flat', [(2, 300, None, 0), (2, 300, 'some', 0), (4, 300, 'image', 0), (2, 300, 'single', 0), (2, 4098, 'three', 0),
                                           (4, 5000, 'some', 0), (2, 2049, 'some', 1), (2, 66000, 'some', 1)])
def test_void_equals_compaction(B, P, void, flat):
    z, t = LR.hinge_case(B, P, void)
    flags = IGNORE | (FLAT if flat else 0)
    op = Op('hinge', z, t, flags, LR.VOID)
    loss, grad = op.run()
    lref, gref = LR.hinge(z, t, not flat, LR.VOID, SCALE)
    what = 'void %s B=%d P=%d flat=%d' % (void, B, P, flat)
    n = B * P if flat else P
    _check64(what, loss, grad, lref, gref, n, LR.hinge(z, t, not flat, LR.VOID, SCALE, dtype=torch.float32)[0] if n > 32768 else None)
    lc, gc = _compacted(z, t, flat)
    g = grad.cpu()
    isvoid = t == LR.VOID
    assert torch.equal(g[~isvoid], gc[~isvoid]), what + ': valid gradients differ from the compacted run'
    assert bool((g[isvoid] == 0).all()), what + ': a void element has a gradient'
    assert abs(loss - lc) <= 2e-6 * max(1.0, abs(lc)), (what, loss, lc)
    if void in ('image',):
        assert float(op.rows_out[0]) == 0.0, 'a row without a valid element has loss 0 (and counts in the mean)'
    assert op.run(False)[0] == loss


def test_void_softmax_against_float64():
    for flags, per_image in ((IGNORE, True), (IGNORE | FLAT, False)):
        p, t = LR.softmax_case(2, 3, 4500, 'some')
        loss, grad = Op('softmax', p, t, flags, LR.VOID).run()
        lref, gref = LR.softmax(p, t, False, per_image, LR.VOID, SCALE)
        _check64('void softmax per_image=%d' % per_image, loss, grad, lref, gref, 9000)
        assert bool((grad.cpu()[t == LR.VOID] == 0).all())


# ---------------------------------------------------------------- 4: only-present
@pytest.mark.parametrize('HW', [300, 4500])
def test_only_present(HW):
    # C = 2, class 1 absent from image 0: C / present = 2 there and 1 in image 1, both exact
    p, t = LR.softmax_case(2, 2, HW, None, 'image')
    lall, gall = Op('softmax', p, t, 0).run()
    op = Op('softmax', p, t, PRESENT)
    loss, grad = op.run()
    lref, gref = LR.softmax(p, t, True, True, None, SCALE)
    _check64('only-present per image HW=%d' % HW, loss, grad, lref, gref, HW)
    assert bool((grad[0, 1] == 0).all()), 'the skipped row has a gradient'
    assert torch.equal(grad[0, 0], gall[0, 0] * 2) and torch.equal(grad[1], gall[1])
    assert float(op.rows_out[1]) == 0.0
    # absent from the whole batch, batch-flat
    p, t = LR.softmax_case(2, 2, HW, None, 'batch')
    lall, gall = Op('softmax', p, t, FLAT).run()
    loss, grad = Op('softmax', p, t, FLAT | PRESENT).run()
    lref, gref = LR.softmax(p, t, True, False, None, SCALE)
    _check64('only-present batch-flat HW=%d' % HW, loss, grad, lref, gref, 2 * HW)
    assert bool((grad[:, 1] == 0).all()) and torch.equal(grad[:, 0], gall[:, 0] * 2)
    # an all-void image: no class is present in it, its loss is 0
    p, t = LR.softmax_case(2, 2, HW, 'image')
    op = Op('softmax', p, t, PRESENT | IGNORE, LR.VOID)
    loss, grad = op.run()
    lref, gref = LR.softmax(p, t, True, True, LR.VOID, SCALE)
    _check64('only-present, image 0 void HW=%d' % HW, loss, grad, lref, gref, HW)
    assert bool((op.rows_out[:2] == 0).all()) and bool((grad[0] == 0).all())


# ---------------------------------------------------------------- 5: reruns into a garbage-filled workspace
@pytest.mark.parametrize('kind,flags', [('hinge', FLAT), ('hinge', FLAT | IGNORE), ('softmax', FLAT | PRESENT | IGNORE)])
def test_reruns_are_bit_identical(kind, flags):
    if kind == 'hinge':
        x, t = LR.hinge_case(3, 44374, 'some' if flags & IGNORE else None)
    else:
        x, t = LR.softmax_case(3, 2, 44374, 'some', 'image')
    op = Op(kind, x, t, flags, LR.VOID)                          # every workspace word starts as 0x55555555
    first = op.run()
    rows = op.rows_out.clone()
    second = op.run()                                            # the workspace as the first run left it
    assert first[0] == second[0] and torch.equal(first[1].view(torch.int32), second[1].view(torch.int32))
    assert torch.equal(rows.view(torch.int32), op.rows_out.view(torch.int32))
    again = Op(kind, x, t, flags, LR.VOID).run()
    assert first[0] == again[0] and torch.equal(first[1].view(torch.int32), again[1].view(torch.int32))


# ---------------------------------------------------------------- 6: refusals
def test_refusals_come_from_host_code_and_launch_nothing():
    abi = _abi()
    BAD = abi.CONSTS['SALT_E_BADARG']
    z, t = LR.hinge_case(2, 300)
    op = Op('hinge', z, t, 0)
    for bad in (dict(flags=8), dict(flags=-1), dict(flags=PRESENT), dict(flags=IGNORE, ignore=NAN), dict(flags=FLAT, B=2, P=2 ** 30),
                dict(flags=IGNORE, B=1, P=2 ** 30 + 1), dict(flags=0, B=1, P=2 ** 31 - 4095)):
        assert raw(op.name, **dict(op.kw, dlogits=op.grad.data_ptr(), **bad)) == BAD, bad
        assert b'lovasz' in abi.lib.salt_last_error()
    assert bool(torch.isnan(op.grad).all()) and bool(torch.isnan(op.loss).all()) and bool(torch.isnan(op.rows_out).all())
    p, t = LR.softmax_case(2, 2, 300)
    op = Op('softmax', p, t, 0)
    for bad in (dict(flags=8), dict(flags=IGNORE, ignore=NAN), dict(flags=PRESENT, ws_present=None), dict(flags=FLAT, B=2 ** 11, HW=2 ** 20),
                dict(flags=IGNORE, B=1, HW=2 ** 30 + 1)):
        assert raw(op.name, **dict(op.kw, dprobas=op.grad.data_ptr(), **bad)) == BAD, bad
    assert bool(torch.isnan(op.grad).all()) and bool(torch.isnan(op.loss).all()) and bool(torch.isnan(op.rows_out).all())
    assert abi.lib.salt_lovasz_flat_words(131072) == 0 and abi.lib.salt_lovasz_flat_words(131073) > 0 and abi.lib.salt_lovasz_flat_words(2 ** 31) == 0


# ---------------------------------------------------------------- 7: the default call
@pytest.mark.parametrize('kind', ['lovasz', 'lovasz_softmax'])
def test_default_call_and_explicit_defaults_give_identical_bits(kind):
    from salt_amd import losses
    g = LR.gen('default call', kind)
    z = (torch.randn(2, 2, 48, 48, generator=g) * 2).to(DEV)
    t = (torch.rand(2, 1, 48, 48, generator=g) < 0.4).float()
    t = torch.cat([1 - t, t], 1).to(DEV)
    l0, g0 = losses.native_loss(z, t, kind)
    explicit = dict(losses.LOVASZ_DEFAULTS[kind])
    l1, g1 = losses.native_loss(z, t, kind, params=explicit)
    assert torch.equal(l0.view(torch.int32), l1.view(torch.int32)) and torch.equal(g0.view(torch.int32), g1.view(torch.int32))
    fn = losses.lovasz_loss if kind == 'lovasz' else losses.lovasz_softmax_loss
    zz = z.clone().requires_grad_(True)
    l2 = fn(zz, t, per_image=True, ignore=None)
    l2.backward()
    assert float(l2) == float(l0) and torch.equal(zz.grad, g0)
    # and a keyword reaches the kernel: the batch-flat loss is another number
    l3 = fn(z, t, per_image=False)
    assert float(l3) != float(l0)
