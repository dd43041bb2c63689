"""Launching one operator through the C-ABI on guarded operands, for the operator-level GPU tests: the lazy ABI handle, raw / call,
seeded fp64 operands rounded to the compute dtype, the close() bound of the streaming kernels, guarded fp32 vectors (Vec) and guarded
NHWC activations (Act), and the statistics / error-ratio checks the grouped and dense convolution tests share.

Importable without a GPU and without the built library: salt_amd is imported on first use only."""
import ctypes
import zlib

import torch

import conv_abi as CA
import op_reference as R
from op_reference import Placed, VARIANTS, VIEW_CASES

DEV = 'cuda:0'
F64 = torch.float64
NAN = float('nan')
SENTINEL = -12345.5
TDT = {'f32': torch.float32, 'bf16': torch.bfloat16}
VIEWS_IDS = ['%s-%s' % v for v in VIEW_CASES]


def _abi():
    import salt_amd  # noqa: F401
    from salt_amd import _abi
    return _abi


def raw(name, **kw):
    abi = _abi()
    fn, S = abi.OP_FUNCS[name]
    args = abi.fill(S(), **kw)
    rc = fn(ctypes.byref(args), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc


def call(name, **kw):
    rc = raw(name, **kw)
    _abi().check(rc, name)


def null_view():
    return _abi().STRUCTS['salt_view']()


def code(dtype):
    return 1 if dtype == 'bf16' else 0


def gen(*seed):
    return torch.Generator().manual_seed(zlib.crc32(repr(seed).encode()))


def rnd(shape, g, dtype, scale=1.0):
    return R.round_to(torch.randn(shape, generator=g, dtype=F64) * scale, dtype)


def close(got, ref, dtype, what=''):
    """f32: |got - ref| <= 5e-5 max|ref|;  bf16: <= 2**-8 |ref| + 5e-5 max|ref| per element."""
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), '%s: non-finite output' % what
    mx = float(ref.abs().max()) if ref.numel() else 0.0
    bound = 5e-5 * mx + (2.0 ** -8 * ref.abs() if dtype == 'bf16' else 0.0)
    err = (got - ref).abs()
    print('%s [%s]: max err %.3e, max|ref| %.3e' % (what, dtype, float(err.max()), mx))
    assert bool((err <= bound).all()), '%s [%s]: max err %.3e (max|ref| %.3e), %d elements over the bound' % (
        what, dtype, float(err.max()), mx, int((err > bound).sum()))


def shape_c(shape, variant, dtype):
    return tuple(shape) + (VARIANTS[variant][dtype][1],)


def out_buf(shape, variant, dtype, accumulate, g):
    """Output window: random contents for accumulate = 1 (returned as `old`), NaN for accumulate = 0."""
    old = rnd(shape_c(shape, variant, dtype), g, dtype) if accumulate else torch.full(shape_c(shape, variant, dtype), NAN, dtype=F64)
    return Placed(shape, variant, dtype, DEV, old), old


class Vec:
    """n fp32 (or fp64) values on the device between two runs of 64 sentinel values."""

    def __init__(self, n, fill=float('nan'), dtype=torch.float32):
        self.buf = torch.full((n + 128,), SENTINEL, dtype=dtype, device=DEV)
        self.win = self.buf[64:64 + n]
        self.win.fill_(fill)

    def ptr(self):
        return self.win.data_ptr()

    def get(self, shape):
        b = self.buf.cpu()
        assert bool((b[:64] == SENTINEL).all()) and bool((b[-64:] == SENTINEL).all()), 'write outside an fp32 output'
        return b[64:-64].reshape(shape).to(F64)


class Act:
    """[B,H,W,C] activation in ``dtype`` storage on the device: contiguous, or (``sliced``) channels [32, 32 + C) of rows C + 96 wide whose
    other channels hold a sentinel.  ``check`` asserts that nothing outside the window changed."""

    def __init__(self, data, dtype, sliced, layout=None):
        """layout: (c0, cs) of a window the two standard placements do not give (rows that are no multiple of 16 bytes)"""
        from salt_amd.engine import shaped_view
        B, H, W, C = data.shape
        self.C, self.c0, self.cs = C, (32 if sliced else 0), (C + 96 if sliced else C)
        if layout is not None:
            self.c0, self.cs = layout
        self.sentinel = float(torch.tensor(SENTINEL, dtype=TDT[dtype]).float())          # as the storage dtype holds it
        self.buf = torch.full((B * H * W * self.cs + 128,), SENTINEL, dtype=TDT[dtype], device=DEV)
        self.rows = self.buf[64:64 + B * H * W * self.cs].view(B, H, W, self.cs)
        self.rows[..., self.c0:self.c0 + C] = data.to(TDT[dtype]).to(DEV)
        self.view = shaped_view(self.rows.data_ptr() + self.c0 * self.buf.element_size(), B, H, W, C, self.cs)

    def get(self):
        return self.rows[..., self.c0:self.c0 + self.C].cpu().to(F64)

    def check(self, what):
        b, r = self.buf.cpu().float(), self.rows.cpu().float()
        ok = bool((b[:64] == self.sentinel).all()) and bool((b[-64:] == self.sentinel).all())
        ok = ok and bool((r[..., :self.c0] == self.sentinel).all()) and bool((r[..., self.c0 + self.C:] == self.sentinel).all())
        assert ok, '%s: write outside the view' % what


def vec_of(t, dtype=torch.float32):
    """a Vec holding t"""
    v = Vec(t.numel(), dtype=dtype)
    v.win.copy_(t.reshape(-1).to(dtype))
    return v


def bits(t):
    return t.view({1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


class Frozen:
    """device buffers that a launch must leave bit-unchanged"""

    def __init__(self, **bufs):
        self.bufs = bufs
        self.was = {k: v.clone() for k, v in bufs.items()}

    def check(self, what):
        for k, v in self.bufs.items():
            assert torch.equal(bits(v), bits(self.was[k])), '%s: %s changed' % (what, k)


def within(got, ref64, ev32, what, ratios, case, key, allowance=None, keep=None):
    """The bound of the fp64 operator suites of scSE and the channel gate: a float32 evaluation ``ev32`` of the same case sits e32 (largest
    absolute error over the tensor) from the float64 reference, ``got`` may sit 4 e32 + 1e-6 max|ref| from it, plus a per-element
    ``allowance`` (the rounding of 16-bit storage).  ``keep``: the elements compared.  The worst error / bound goes to ratios[case][key]."""
    assert got.shape == ref64.shape, (what, got.shape, ref64.shape)
    assert bool(torch.isfinite(got).all()), '%s: non-finite output' % what
    ev32 = ev32.double()
    if keep is not None:
        got, ref64, ev32 = got[keep], ref64[keep], ev32[keep]
        allowance = allowance[keep] if allowance is not None else None
    mx = float(ref64.abs().max())
    e32 = float((ev32 - ref64).abs().max())
    bound = 4 * e32 + 1e-6 * mx + (allowance if allowance is not None else 0.0)
    err = (got - ref64).abs()
    ratio = float((err / bound).max()) if mx > 0 else (0.0 if float(err.max()) == 0 else float('inf'))
    per = ratios.setdefault(case, {})
    per[key] = max(per.get(key, 0.0), ratio)
    print('%s | %s: err %.3e  yardstick %.3e  max|ref| %.3e  ratio %.3f' % (what, key, float(err.max()), e32, mx, ratio))
    assert ratio <= 1.0, '%s | %s: error at %.3f of the bound (err %.3e, yardstick %.3e, max|ref| %.3e)' % (what, key, ratio, float(err.max()), e32, mx)


def merge_partials(stats, cnt):
    """Chan's merge of per-tile (sum, M2 about the tile mean, count) in float64 -> (N, S, Q = M2 + S^2 / N)"""
    N = float(cnt.sum())
    S = stats[:, 0].sum(0)
    mean = S / N
    M2 = (stats[:, 1] + cnt[:, None] * (stats[:, 0] / cnt[:, None] - mean) ** 2).sum(0)
    return N, S, M2 + S * S / N


def check_moments(what, got, dtype, n, s, q):
    y = got.reshape(-1, got.shape[-1])
    assert n == y.shape[0], '%s: count %r for %d pixels' % (what, n, y.shape[0])
    rs, rq, ts, tq = CA.moments(y, dtype)
    r1, r2 = float(((s - rs).abs() / ts.clamp_min(1e-300)).max()), float(((q - rq).abs() / tq.clamp_min(1e-300)).max())
    print('%s: sum at %.3f, sum of squares at %.3f of the bound' % (what, r1, r2))
    assert r1 <= 1.0 and r2 <= 1.0, '%s: sum at %.3f, sum of squares at %.3f of the bound' % (what, r1, r2)


def held(got, ref, what, case, key, ratio, ratios):
    """ratio(got, ref) <= 1, recorded as the worst of ratios[case][key]"""
    r = ratio(got, ref)
    per = ratios.setdefault(case, {})
    per[key] = max(per.get(key, 0.0), r)
    print('%s: worst error / bound %.3f' % (what, r))
    assert r <= 1.0, '%s: error at %.3f of the bound' % (what, r)
