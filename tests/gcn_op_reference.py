"""Float64 references of the paired line convolution (include/saltnet.h: salt_gcn_pair / salt_gcn_pair_dgrad), written from the
definitions, NHWC, each with a derived per-element bound.  test_lkm_cpu.py pins them against torch's own ReplicationPad2d + conv2d and
against autograd in double (both branches, and the closed-form adjoint with its two edge terms); test_gpu_gcn.py holds the kernels to
them, elementwise, no element excluded.

Operands are bf16-representable (make_case), so every product of two of them is exact in fp32 and in float64, and the only differences
between kernel and reference are the fp32 roundings counted below (u = 2^-23) and the storage rounding (2^-8 per bf16 store,
conv_abi.store_tol) - the bound of tests/psp_op_reference.py, restated for these sums.  A = the sum of the absolute values of the same
terms; "T u A" = T fp32 additions in any order, each off by at most u of a partial sum that A bounds.
  forward    v = sum over K taps and Cin channels of w x: T = K Cin products, all exact: |v' - v| <= T u A.
             eval   y = relu?((v + bias) scale + shift): one addition, one product, one addition (or one fused step) more:
                    tol = |scale| (T + 1) u (A + |bias|) + 2 u (|scale| (A + |bias|) + |shift|); the ReLU is 1-Lipschitz
             train  y = v + bias: tol = (T + 1) u (A + |bias|)
             statistics: conv_abi.moments (the sums of the STORED values, N fp32 additions in any order)
  dgrad      dx = sum over the taps that reach the pixel (the regular 2 K, and for row 0 / column W - 1 the clamp taps of the
             formula, each applied term by term on the original weight) and Cout channels of w dy: T = Cout x (taps at this pixel),
             counted per pixel by running the same formula on ones: tol = T u A; with accumulate one more addition, u |dx + old|."""
import torch

from conv_abi import ratio_strict as ratio, store_tol          # noqa: F401  (ratio is the tests' entry point)

F64 = torch.float64
U32 = 2.0 ** -23
GCN_TH, GCN_TW = 8, 16          # the kernel's pixel tile (csrc/gcn.hip)

# (B, H, W, Cin, Cout, K)
CASES = [(2, 6, 10, 64, 21, 9),          # H < K - 1 < W: the F21 block's shape
         (3, 4, 4, 96, 21, 9),           # H and W both below K - 1, odd batch, Cin no multiple of 64
         (2, 1, 17, 32, 32, 9),          # a single row, the full N tile, two tiles along W
         (1, 33, 20, 64, 8, 3),
         (2, 40, 36, 32, 21, 4),         # even K
         (1, 16, 16, 64, 1, 2),
         (1, 19, 37, 40, 21, 9)]         # 3 x 3 tiles of GCN_TH x GCN_TW = 8 x 16, a ragged 32-channel chunk (Cin = 40)


def _bf(t):
    return t.bfloat16().double()


def make_case(B, H, W, Cin, Cout, K, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    sc = (K * Cin) ** -0.5
    return dict(shape=(B, H, W, Cin, Cout, K), x=_bf(r(B, H, W, Cin)), wv=_bf(r(Cout, Cin, K) * sc), wh=_bf(r(Cout, Cin, K) * sc),
                bias=[r(Cout).float().double() * 0.5 for _ in range(2)], scale=[(1.0 + 0.25 * r(Cout)).float().double() for _ in range(2)],
                shift=[r(Cout).float().double() * 0.25 for _ in range(2)], dyv=_bf(r(B, H, W, Cout)), dyh=_bf(r(B, H, W, Cout)),
                dx_old=_bf(r(B, H, W, Cin)))


# ---------------------------------------------------------------- definitions (float64, also what test_lkm_cpu.py compares with torch)
def pair_fwd(x, wv, wh):
    """x [B,H,W,C], wv / wh [N,C,K] -> (v, h) [B,H,W,N]: the K x 1 convolution with K - 1 replicated rows on top, the 1 x K convolution
    with K - 1 replicated columns on the right"""
    B, H, W, C = x.shape
    K = wv.shape[2]
    v = torch.zeros(B, H, W, wv.shape[0], dtype=x.dtype)
    h = torch.zeros_like(v)
    for k in range(K):
        rows = (torch.arange(H) - (K - 1) + k).clamp_min(0)
        cols = (torch.arange(W) + k).clamp_max(W - 1)
        v += torch.einsum('bijc,nc->bijn', x[:, rows], wv[:, :, k])
        h += torch.einsum('bijc,nc->bijn', x[:, :, cols], wh[:, :, k])
    return v, h


def pair_dgrad(dyv, dyh, wv, wh):
    """the closed-form adjoint of pair_fwd (saltnet.h): dyv / dyh [B,H,W,N] -> dx [B,H,W,C]"""
    B, H, W, N = dyv.shape
    K = wv.shape[2]
    dx = torch.zeros(B, H, W, wv.shape[1], dtype=dyv.dtype)
    mm = lambda g, w, k: torch.einsum('b...n,nc->b...c', g, w[:, :, k])
    for k in range(K):
        s = K - 1 - k
        if s < H:
            dx[:, :H - s] += mm(dyv[:, s:], wv, k)                  # rows outside [0, H) contribute nothing
        if k < W:
            dx[:, :, k:] += mm(dyh[:, :, :W - k], wh, k)            # columns outside [0, W) contribute nothing
    for i in range(min(K - 2, H - 1) + 1):                          # row 0: the taps that reached above it
        for k in range(K - 2 - i + 1):
            dx[:, 0] += mm(dyv[:, i], wv, k)
    for j in range(max(W - K + 1, 0), W):                           # column W - 1: the taps that reached past it
        for k in range(W - j, K):
            dx[:, :, W - 1] += mm(dyh[:, :, j], wh, k)
    return dx


def dgrad_terms(H, W, N, K):
    """[H][W]: how many products enter an element of dx at that pixel"""
    one = torch.ones(1, H, W, 1, dtype=F64)
    return pair_dgrad(one, one, torch.ones(1, 1, K, dtype=F64), torch.ones(1, 1, K, dtype=F64))[0, :, :, 0] * N


# ---------------------------------------------------------------- references with bounds
def _ref(e, tol, dtype):
    return dict(exact=e, tol=store_tol(e, tol, dtype))


def fwd_ref(c, dtype, mode, relu=(0, 0)):
    """mode 'eval': relu?((v + bias) scale + shift) per branch;  'plain': relu?(v);  'train': v + bias -> [ref of yv, ref of yh]"""
    Cin, K = c['shape'][3], c['shape'][5]
    T = K * Cin
    raw = pair_fwd(c['x'], c['wv'], c['wh'])
    mag = pair_fwd(c['x'].abs(), c['wv'].abs(), c['wh'].abs())
    out = []
    for br in range(2):
        v, A = raw[br], mag[br]
        if mode == 'plain':
            e, tol = v, T * U32 * A
        elif mode == 'train':
            e, tol = v + c['bias'][br], (T + 1) * U32 * (A + c['bias'][br].abs())
        else:
            sc, sh, Ab = c['scale'][br], c['shift'][br], A + c['bias'][br].abs()
            e = (v + c['bias'][br]) * sc + sh
            tol = sc.abs() * (T + 1) * U32 * Ab + 2 * U32 * (sc.abs() * Ab + sh.abs())
        if relu[br]:
            e = e.clamp_min(0)
        out.append(_ref(e, tol, dtype))
    return out


def dgrad_ref(c, dtype, accumulate):
    B, H, W, Cin, Cout, K = c['shape']
    e = pair_dgrad(c['dyv'], c['dyh'], c['wv'], c['wh'])
    A = pair_dgrad(c['dyv'].abs(), c['dyh'].abs(), c['wv'].abs(), c['wh'].abs())
    tol = dgrad_terms(H, W, Cout, K)[None, :, :, None] * U32 * A
    if accumulate:
        e = e + c['dx_old']
        tol = tol + U32 * e.abs()
    return _ref(e, tol, dtype)


# ---------------------------------------------------------------- guarded device storage
class Wide:
    """[B,H,W,cs] rows of ``dtype`` storage on the device between two runs of 64 sentinel values.  ``windows`` = {name: (c0, data)}:
    channels [c0, c0 + C) hold ``data`` [B,H,W,C]; every other channel holds the sentinel.  ``check`` asserts that nothing outside the
    windows changed."""

    def __init__(self, B, H, W, cs, dtype, windows):
        from abi_ops import SENTINEL, TDT, DEV
        self.dt = TDT[dtype]
        self.sentinel = float(torch.tensor(SENTINEL, dtype=self.dt).float())
        self.buf = torch.full((B * H * W * cs + 128,), SENTINEL, dtype=self.dt, device=DEV)
        self.rows = self.buf[64:64 + B * H * W * cs].view(B, H, W, cs)
        self.win = {}
        for name, (c0, data) in windows.items():
            C = data.shape[-1]
            assert c0 + C <= cs
            self.rows[..., c0:c0 + C] = data.to(self.dt).to(DEV)
            self.win[name] = (c0, C)
        self.shape, self.cs = (B, H, W), cs

    def view(self, name):
        from salt_amd.engine import shaped_view
        c0, C = self.win[name]
        return shaped_view(self.rows.data_ptr() + c0 * self.buf.element_size(), *self.shape, C, self.cs)

    def get(self, name):
        c0, C = self.win[name]
        return self.rows[..., c0:c0 + C].cpu().to(F64)

    def check(self, what):
        b, r = self.buf.cpu().float(), self.rows.cpu().float().clone()
        ok = bool((b[:64] == self.sentinel).all()) and bool((b[-64:] == self.sentinel).all())
        for c0, C in self.win.values():
            r[..., c0:c0 + C] = self.sentinel
        assert ok and bool((r == self.sentinel).all()), '%s: write outside the view' % what
