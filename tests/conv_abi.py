"""salt_conv through the C-ABI for the tests: one place that fills salt_conv_args / salt_pack_conv_weight_args, asks the planner
(salt_conv_kernel_id / salt_conv_tile_shape: host only, no launch), launches on guard-prefilled buffers, and the float64 reference of
the same operands with a per-element error bound.  test_conv_reference_cpu.py pins the reference against torch on the CPU,
test_gpu_conv_abi.py holds every kernel family to it.

The reference (conv_sum) is the definition in include/saltnet.h:
    v[b, oy, ox, n] = sum_t sum_c X[b, pad(oy in_step + tap_dy[t]), pad(ox in_step + tap_dx[t]), c] W[t][n][c]
as a loop over the taps with clamped (pad_mode 1) or zero-masked (pad_mode 0) gathers, in float64, together with
A = sum |X| |W| of the same terms.  The epilogue (conv_ref) follows the header: epi(v) = relu?((v + bias) scale + shift), with a
residual relu?(store(epi) + res), with accumulate store(store(epi) + old).

Operands come from mk(): normal values that bf16 holds exactly, in both dtypes.  Every product x w then has at most 16 significant
bits and is exact in fp32; a kernel differs from the float64 sum only by the order and rounding of its K = ntaps Cin additions.

The bound, per element (derived here, not tuned to a kernel):
  * accumulation: K - 1 fp32 additions of exact products, in any order, each off by at most u |partial sum| <= u A with
    u = 2^-23 (a whole ulp, so that adders that truncate are covered): |v' - v| <= t_acc = K 2^-23 A.
  * epilogue in fp32: the error passes through the affine part with gain g = |scale| (else 1), and each fp32 operation of the
    epilogue (bias, scale, shift, + res / + old) adds at most half an ulp of its result: tol = t_acc g + 4 * 2^-23 * (largest
    intermediate of the element) covers eight of them.
  * bf16 storage: a value e' = e + d, |d| <= tol, stored as bf16 (8 significant bits: half an ulp is at most 2^-8 |e'|) lands within
    tol + 2^-8 (|e| + tol) of e.  Every storage rounding on the path adds that term for the value IT rounds: one for a plain launch,
    two with `res` (the stored epilogue value, then the sum) or `accumulate` (the same), one more per level of the fused fold.
The reference itself never rounds: a reference that rounds its intermediate where the kernel does agrees exactly on most elements, but
where d moves e across a rounding boundary the two are a whole ulp apart, which one 2^-8 term per rounding does not cover.  `stored`
in the result is the reference WITH the storage roundings at the header's places (before + res, before +=, at the store): what an
exact kernel would hold, used by the CPU stand-in and for decisions (ReLU / mask signs), never with the bound.
A dropped corner tap moves an element by about |x w| ~ A / K, i.e. >= 2^23 / K^2 times t_acc: hundreds of bounds on these shapes."""
import ctypes
import math

import torch

from op_reference import F64, GUARD, Placed, guard_fill, make_view, pad_fold, round_to    # noqa: F401  (re-exported for the tests)
from wgrad_abi import RASTER, RASTER_REP, mk, nhwc                                  # noqa: F401

_DTYPE = {'f32': 0, 'bf16': 1}
U32, UBF = 2.0 ** -23, 2.0 ** -8
PHASE4 = [(0, 0), (0, 1), (1, 0), (1, 1)]


def k3_taps(pad_mode=0):
    """(kh, kw, dy, dx) of nn.Conv2d(k3, padding 1) / ReplicationPad2d((0, 2, 2, 0)) + valid convolution."""
    return [(kh, kw, kh - 2, kw) if pad_mode else (kh, kw, kh - 1, kw - 1) for kh in range(3) for kw in range(3)]


def kk_taps(K):
    """(kh, kw, dy, dx) of nn.Conv2d(K, padding K // 2), K odd."""
    return [(kh, kw, kh - K // 2, kw - K // 2) for kh in range(K) for kw in range(K)]


def master_weight(D0, D1, KH, KW, cin, ntaps, seed):
    """fp32 master weight [D0][D1][KH][KW]: mk() * sqrt(2 / (ntaps cin)), re-rounded to bf16 (exact in both dtypes)."""
    return (mk(D0, D1, KH, KW, seed) * math.sqrt(2.0 / (ntaps * cin))).bfloat16().float()


def tap_weights(w, tap_k, transpose):
    """salt_pack_conv_weight's meaning as plain indexing: [ntaps][N][C] float64, Wp[t][n][c] = W[n][c][kh][kw] (transpose 0) or
    W[c][n][kh][kw] (transpose 1); tap_k[t] = (kh, kw), None or kh < 0: a zero tap."""
    N, C = (w.shape[1], w.shape[0]) if transpose else (w.shape[0], w.shape[1])
    out = torch.zeros(len(tap_k), N, C, dtype=F64)
    for t, k in enumerate(tap_k):
        if k is not None and k[0] >= 0:
            m = w[:, :, k[0], k[1]].double()
            out[t] = m.t() if transpose else m
    return out


# ---------------------------------------------------------------- launch forms (engine.py emits these)
def dgrad_taps(taps):
    """Stride-1 data gradient of a convolution with taps (kh, kw, dy, dx): mirrored offsets, transposed weights."""
    return [(kh, kw, -dy, -dx) for kh, kw, dy, dx in taps]


def dgrad_taps_extended(taps, top):
    """Data gradient w.r.t. the replicate-padded input on the extended grid (top pad rows above, the pad columns to the right)."""
    return [(kh, kw, -dy - top, -dx) for kh, kw, dy, dx in taps]


def dgrad_s2_phases(taps):
    """Stride-2 data gradient = four output-parity phases: [(ay, ax, [(kh, kw, dy, dx)])] over dy of the phase's own grid."""
    out = []
    for ay in range(2):
        for ax in range(2):
            out.append((ay, ax, [(kh, kw, (ay - dy) // 2, (ax - dx) // 2) for kh, kw, dy, dx in taps if (dy - ay) % 2 == 0 and (dx - ax) % 2 == 0]))
    return out


def convt_phases(K, p=1):
    """nn.ConvTranspose2d(K, stride 2, padding p): [(fy, fx, [(kh, kw, dy, dx)])], output (2 oy + fy, 2 ox + fx) reads x[oy + dy, ox + dx]."""
    out = []
    for fy in range(2):
        for fx in range(2):
            out.append((fy, fx, [(u, v, (fy + p - u) // 2, (fx + p - v) // 2) for u in range(K) for v in range(K)
                                 if (fy + p - u) % 2 == 0 and (fx + p - v) % 2 == 0]))
    return out


def unify_phases(phases):
    """The nphase = 4 form: (unified offsets padded to 4 or 9 with a repeated zero tap, per phase [(kh, kw) | None])."""
    offs = sorted({(t[2], t[3]) for _, _, sel in phases for t in sel})
    offs = offs + [offs[0]] * ((4 if len(offs) <= 4 else 9) - len(offs))
    rows = []
    for _, _, sel in phases:
        d = {(t[2], t[3]): (t[0], t[1]) for t in sel}
        row, used = [], set()
        for o in offs:
            row.append(d[o] if o in d and o not in used else None)
            used.add(o)
        rows.append(row)
    return offs, rows


# ---------------------------------------------------------------- float64 reference
def conv_sum(x, wt, offs, in_step, pad_mode, OH, OW):
    """x [B,H,W,Cin], wt [ntaps][Cout][Cin] float64, offs [(dy, dx)] -> (v, A) [B,OH,OW,Cout] float64."""
    B, H, W, _ = x.shape
    xd = x.double()
    v = torch.zeros(B, OH, OW, wt.shape[1], dtype=F64)
    A = torch.zeros_like(v)
    for t, (dy, dx) in enumerate(offs):
        iy = torch.arange(OH) * in_step + dy
        ix = torch.arange(OW) * in_step + dx
        g = xd[:, iy.clamp(0, H - 1)][:, :, ix.clamp(0, W - 1)]
        if not pad_mode:
            ok = ((iy >= 0) & (iy < H)).double()[:, None] * ((ix >= 0) & (ix < W)).double()[None, :]
            g = g * ok[None, :, :, None]
        v += torch.einsum('bhwc,nc->bhwn', g, wt[t])
        A += torch.einsum('bhwc,nc->bhwn', g.abs(), wt[t].abs())
    return v, A


def _store(e, tol, dtype, stored=None):
    """One storage rounding of the value e (known to tol): -> (tol after it, the rounded reference)."""
    if dtype == 'bf16':
        tol = tol + UBF * (e.abs() + tol)
    return tol, round_to(e if stored is None else stored, dtype)


def conv_ref(x, wt, offs, in_step, pad_mode, OH, OW, dtype, bias=None, scale=None, shift=None, relu=False, res=None, old=None,
             fold=None, in_tf=None):
    """-> dict(exact, tol, stored, v, A).  bias / scale / shift [Cout] float64, res / old [B,OH,OW,Cout] float64 (old: accumulate = 1
    onto these values).  fold = (top, right): the launch's grid is the extended one; the result is on the unpadded grid, every ring
    pixel added onto its edge pixel (op_reference.pad_fold) after its own storage rounding, `old` added after the fold.
    in_tf = (in_scale, in_shift, in_relu): x' = round(relu?(x in_scale + in_shift)) for in-range elements (zero padding stays zero; a
    clamped read takes the transformed border element)."""
    flip = None
    if in_tf is not None:
        xs = x.double() * in_tf[0] + in_tf[1]
        t = xs.clamp_min(0) if in_tf[2] else xs
        # the kernel forms t in fp32 (two roundings, or one fused): where t lies that close to a tie of the storage rounding the two may
        # round to different neighbours - such an element is known to one storage ulp only, and sum ulp |w| joins the bound
        ulp = 2.0 ** (torch.floor(torch.log2(t.abs().clamp_min(2.0 ** -126))) - (7 if dtype == 'bf16' else 23))
        f = t / ulp
        near = ((f - f.floor()) - 0.5).abs() * ulp <= 4 * U32 * ((x.double() * in_tf[0]).abs() + in_tf[1].abs())
        flip = torch.where(near, ulp, torch.zeros_like(ulp))
        x = round_to(t, dtype)
    v, A = conv_sum(x, wt, offs, in_step, pad_mode, OH, OW)
    K = len(offs) * x.shape[3]
    tol = K * U32 * A
    if flip is not None and bool(flip.any()):
        tol = tol + conv_sum(flip, wt.abs(), offs, in_step, pad_mode, OH, OW)[0]
    big = v.abs()
    e = v
    if bias is not None:
        e = e + bias
        big = torch.maximum(big, e.abs())
    if scale is not None:
        e = e * scale
        tol = tol * scale.abs()
        big = torch.maximum(big, e.abs())
    if shift is not None:
        e = e + shift
        big = torch.maximum(big, e.abs())
    if relu and res is None:
        e = e.clamp_min(0)
    tol = tol + 4 * U32 * big
    s = e
    staged = fold is not None or res is not None or old is not None
    if staged:
        tol, s = _store(e, tol, dtype)                                     # the stored epilogue value (the staged tile of a fold)
    if fold is not None:
        top, right = fold
        edge = pad_fold(torch.ones_like(e), top, 0, 0, right) > 1          # pixels that take ring pixels: summed, rounded again
        absum = pad_fold(e.abs(), top, 0, 0, right)
        e, s, tol = pad_fold(e, top, 0, 0, right), pad_fold(s, top, 0, 0, right), pad_fold(tol, top, 0, 0, right)
        tol_e, s_e = _store(e, tol + 4 * U32 * absum, dtype, s)            # up to 8 fp32 additions of the ring
        tol, s = torch.where(edge, tol_e, tol), torch.where(edge, s_e, s)
    if res is not None:
        e, s = e + res, s + res
        tol = tol + U32 * e.abs()
        if relu:
            e, s = e.clamp_min(0), s.clamp_min(0)
        tol, s = _store(e, tol, dtype, s)
    if old is not None:
        e, s = e + old, s + old
        tol, s = _store(e, tol + U32 * e.abs(), dtype, s)
    if not staged:
        tol, s = _store(e, tol, dtype)
    return dict(exact=e, tol=tol, stored=s, v=v, A=A)


def ratio(got, ref):
    """max |got - exact| / tol over the elements (NaN / inf in `got` -> inf)."""
    r = (got.double() - ref['exact']).abs() / ref['tol'].clamp_min(1e-300)
    return float(torch.nan_to_num(r, nan=float('inf'), posinf=float('inf')).max())


# ---------------------------------------------------------------- C-ABI
def pack(w, dtype, tap_k, transpose=0):
    """w: fp32 master [D0][D1][KH][KW] on the device; tap_k [(kh, kw) | None] -> packed device tensor."""
    import salt_amd  # noqa: F401
    from salt_amd._abi import STRUCTS, lib, fill, check
    D0, D1, KH, KW = w.shape
    N, C = (D1, D0) if transpose else (D0, D1)
    n = lib.salt_packed_weight_elems(_DTYPE[dtype], len(tap_k), N, C)
    wp = guard_fill(torch.empty(n, dtype=torch.bfloat16 if dtype == 'bf16' else torch.float32, device=w.device))
    A = fill(STRUCTS['salt_pack_conv_weight_args'](), dtype=_DTYPE[dtype], w=w.data_ptr(), D0=D0, D1=D1, KH=KH, KW=KW, ntaps=len(tap_k),
             tap_kh=[-1 if k is None else k[0] for k in tap_k], tap_kw=[0 if k is None else k[1] for k in tap_k], transpose=transpose,
             wp=wp.data_ptr())
    check(lib.salt_pack_conv_weight(ctypes.byref(A), torch.cuda.current_stream().cuda_stream), 'salt_pack_conv_weight')
    return wp


def pack_phases(w, dtype, rows, transpose=0):
    """The nphase = 4 weight: one packed block per phase, back to back -> (tensor, w_phase_elems)."""
    blocks = [pack(w, dtype, row, transpose) for row in rows]
    return torch.cat(blocks), blocks[0].numel()


def conv_args(dtype, x, wp, offs, y, OH, OW, **kw):
    """x / y: salt_view; wp: device pointer (any 16-byte aligned number for the host-only planner queries)."""
    import salt_amd  # noqa: F401
    from salt_amd._abi import STRUCTS, fill
    f = dict(in_step=1, pad_mode=0, out_step=1)
    f.update(kw)
    return fill(STRUCTS['salt_conv_args'](), dtype=_DTYPE[dtype], x=x, w=wp, ntaps=len(offs), tap_dy=[o[0] for o in offs],
                tap_dx=[o[1] for o in offs], y=y, OH=OH, OW=OW, **f)


def conv_kernel_id(S):
    from salt_amd._abi import lib
    return lib.salt_conv_kernel_id(ctypes.byref(S))


def tile_shape(S):
    """-> (tw, th, images per tile, general) or None when there is no plan."""
    from salt_amd._abi import lib
    t = lib.salt_conv_tile_shape(ctypes.byref(S))
    return None if t < 0 else (t & 0xff, (t >> 8) & 0xff, (t >> 16) & 0xff, (t >> 24) & 0xff)


def last_error():
    from salt_amd._abi import lib
    return lib.salt_last_error().decode(errors='replace')


def conv_hip(S, ybuf):
    """Launch and wait; -> the whole output buffer on the CPU (its storage dtype: the caller compares bits outside the window)."""
    from salt_amd._abi import lib, check
    check(lib.salt_conv(ctypes.byref(S), torch.cuda.current_stream().cuda_stream), 'salt_conv')
    torch.cuda.synchronize()
    return ybuf.cpu()


def bits(t):
    return t.view({4: torch.int32, 2: torch.int16, 8: torch.int64}[t.element_size()])


def moments(y, dtype):
    """y [N, C] float64, the values a launch STORED -> (sum, sum of squares, tol of the sum, tol of the sum of squares) per channel for
    statistics that a kernel forms in fp32 from the values BEFORE their storage rounding: |v - y| <= eps |y| with eps = 2^-8 (1 + 2^-7)
    in bf16 and 0 in fp32 (one storage rounding per element), plus N fp32 additions in any order, each off by at most 2^-23 of a
    partial result that sum |y| (sum y^2) bounds: |S' - S| <= (eps + N u) sum |y|, |Q' - Q| <= (2 eps + eps^2 + 2 N u) sum y^2 (the
    second N u: kernels that form Q as M2 + S^2 / N inherit 2 |S| dS / N <= 2 N u sum y^2)."""
    N = y.shape[0]
    eps = UBF * (1 + 2 * UBF) if dtype == 'bf16' else 0.0
    q = (y * y).sum(0)
    return y.sum(0), q, (eps + N * U32) * y.abs().sum(0), (2 * eps + eps * eps + 2 * N * U32) * q
