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

import pytest
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


def ratio_strict(got, ref):
    """max |got - exact| / tol over ALL elements (NaN / inf in `got` -> inf; an element with tol = 0 must be exact)"""
    d = (got.double() - ref['exact']).abs()
    r = torch.where(ref['tol'] > 0, d / ref['tol'].clamp_min(1e-300), torch.where(d == 0, torch.zeros_like(d), torch.full_like(d, float('inf'))))
    return float(torch.nan_to_num(r, nan=float('inf'), posinf=float('inf')).max())


def store_tol(e, tol, dtype):
    """tol of the value e after one storage rounding (the grouped and dense convolution references; _store above also rounds)"""
    return tol + UBF * (e.abs() + tol) if dtype == 'bf16' else tol


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


# ---------------------------------------------------------------- the case table of test_gpu_conv_abi.py / test_conv_reference_cpu.py
BM = {1: 128, 2: 256, 3: 128, 4: 128, 5: 64}
K3, K3R = k3_taps(0), k3_taps(1)
K1 = [(0, 0, 0, 0)]
K13 = [(0, kw, 0, kw - 1) for kw in range(3)]                     # a (1, 3) kernel, padding (0, 1)


def case(name, kid, dtype, B, Cin, Cout, H, W, taps, **kw):
    c = dict(name=name, kid=kid, dtype=dtype, B=B, Cin=Cin, Cout=Cout, H=H, W=W, taps=taps, transpose=0, in_step=1, pad_mode=0, OH=None, OW=None,
             out_step=1, out_oy=0, out_ox=0, yH=None, yW=None, cfg=kid, xv=None, yv=None, bias=False, scale=False, shift=False, relu=False,
             res=False, acc=False, fold=None, gen=None, regime=None, tile=None, seed=1, KH=None, KW=None, in_tf=None)
    c.update(kw)
    s = c['in_step']
    if c['OH'] is None:
        c['OH'], c['OW'] = ((H - 1) // s + 1, (W - 1) // s + 1) if not c['fold'] else (H + c['fold'][1], W + c['fold'][2])
    if c['yH'] is None:
        if c['fold']:
            c['yH'], c['yW'] = H, W
        else:
            c['yH'], c['yW'] = c['OH'] * c['out_step'], c['OW'] * c['out_step']
    if c['KH'] is None:
        c['KH'], c['KW'] = max(t[0] for t in taps) + 1, max(t[1] for t in taps) + 1
    c['xv'] = c['xv'] or (0, Cin)
    c['yv'] = c['yv'] or (0, Cout)
    return pytest.param(c, id=name)


# forced configs whose halo does not fit the tile's loader budget fall back to config 5 (64-pixel tiles): asserted, not assumed
HALO_FALLBACK = {(2, 'ragged'), (2, 'ragged-replicate'), (2, 'accumulate-ragged'), (2, '160-64-8x8-b5'), (2, 's2-k1-32-48'), (2, '4x4-b16'),
                 (2, '2x2-b5'), (2, '3x4-b3'), (2, 's2-k3-17x31'), (1, 's2-k3-15x13')}
CASES = []
for dt in ('f32', 'bf16'):
    for kid in (1, 2, 3, 4, 5):
        def add(shape, *a, **kw):
            k = kw.pop('runs', 5 if (kid, shape) in HALO_FALLBACK else kid)
            CASES.append(case('%s-cfg%d-%s' % (dt, kid, shape), k, dt, *a, cfg=kid, **kw))
        # ragged: scalar load_piece path (cs 13 / 10), partial tiles, partial batch tile
        add('ragged', 3, 13, 10, 7, 5, K3, regime='nt9')
        add('ragged-replicate', 3, 13, 10, 7, 5, K3R, pad_mode=1, regime='nt9')
        add('ragged-1tap', 3, 13, 10, 7, 5, K1, regime='nt0')
        # whole 16-byte pieces
        add('40-72-33x17', 2, 40, 72, 33, 17, K3)
        add('64-64-16x16', 2, 64, 64, 16, 16, K3)
        add('160-64-8x8-b5', 5, 160, 64, 8, 8, K3R, pad_mode=1)
        add('1x3-24-40', 2, 24, 40, 9, 11, K13, regime='nt0')
        # stride 2: a 16 x 8 tile reads a 33 x 17 halo, the most a 128-pixel tile's loader holds; 8 x 8 tiles x 2 images do not fit
        add('s2-k3-17x31', 2, 32, 48, 17, 31, K3, in_step=2)
        if kid in (1, 5):
            add('s2-k3-15x13', 2, 32, 48, 15, 13, K3, in_step=2)
        add('s2-k1-32-48', 2, 32, 48, 8, 8, K1, in_step=2, regime='nt0')
        # 1x1: Cin a multiple of four chunks -> 4 virtual taps (config 2 falls back to 1), else 1
        add('1x1-vt4', 2, 128 if dt == 'bf16' else 64, 40, 9, 11, K1, runs=1 if kid == 2 else kid, regime='nt4' if dt == 'f32' or kid == 5 else 'ilv4')
        add('1x1-vt1', 2, 96, 40, 9, 11, K1, regime='nt0')
        # many images per tile
        add('4x4-b16', 16, 24, 40, 4, 4, K3)
        add('2x2-b5', 5, 24, 40, 2, 2, K3)
        add('3x4-b3', 3, 24, 40, 3, 4, K3R, pad_mode=1)
        # views: x at channel offset 4 of a wider buffer (bf16: 8 bytes past a 16-byte boundary), y a window with guard channels
        add('x-misaligned', 2, 40, 24, 9, 11, K3, xv=(4, 56), regime='nt9')
        add('y-window', 2, 40, 24, 9, 11, K3, yv=(8, 48))
        add('y-window-ragged', 2, 24, 13, 9, 11, K3, yv=(3, 21))
        # epilogue: the header's combinations, with scale in [0.5, 2] (both signs) and shift of the order of the output
        add('bias-relu', 2, 24, 37, 9, 11, K3, bias=True, relu=True)
        add('scale-shift', 2, 24, 37, 9, 11, K3, scale=True, shift=True)
        add('bias-scale-shift-relu', 2, 24, 37, 9, 11, K3, bias=True, scale=True, shift=True, relu=True)
        add('res-relu', 2, 24, 40, 9, 11, K3, scale=True, shift=True, relu=True, res=True)
        add('res-full-tiles', 2, 32, 64, 16, 16, K3, bias=True, res=True)
        add('accumulate', 2, 24, 40, 9, 11, K3, acc=True)
        add('accumulate-ragged', 3, 13, 10, 7, 5, K3, acc=True)
        add('accumulate-full-tiles', 2, 32, 64, 16, 16, K3, acc=True)

# the interleaved loader's three halo budgets on config 2 (256-pixel tiles, MAXA_T 6) and 1 / 3 / 4 (128-pixel tiles, MAXA_T 3 | 9)
CASES += [
    case('bf16-cfg2-ilv6', 2, 'bf16', 1, 64, 64, 16, 16, K3, regime='ilv9-6'),
    case('bf16-cfg1-ilv9', 1, 'bf16', 5, 160, 64, 8, 8, K3, regime='ilv9-9'),
    case('bf16-cfg1-ilv3', 1, 'bf16', 2, 40, 72, 33, 17, K3, regime='ilv9-3'),
    case('bf16-cfg4-ilv3', 4, 'bf16', 2, 64, 64, 16, 16, K3, regime='ilv9-3'),
    case('bf16-cfg3-ilv9', 3, 'bf16', 16, 24, 40, 4, 4, K3, regime='ilv9-9'),
]

# ---- output placement: the four out_step = 2 launches of ConvTranspose2d k4 (4 taps each) and k3 (4, 2, 2, 1 taps)
for dt in ('f32', 'bf16'):
    for K in (4, 3):
        for kid in ((1, 4, 5) if dt == 'f32' else (1, 4, 5, 6, 7, 8)):
            for fy, fx, sel in convt_phases(K):
                if kid >= 6 and len(sel) != 4:
                    continue                                               # conv_glds_kernel: 9 or 4 taps
                CASES.append(case('%s-cfg%d-convt-k%d-phase%d%d' % (dt, kid, K, fy, fx), kid, dt, 2, 32, 40, 9, 5, sel, transpose=1, KH=K, KW=K,
                                  out_step=2, out_oy=fy, out_ox=fx, bias=True, seed=7))
    # stride-2 data gradient of a k3 convolution, phase by phase, onto random y
    for ay, ax, sel in dgrad_s2_phases(K3):
        CASES.append(case('%s-cfg4-dgrad-s2-phase%d%d-accumulate' % (dt, ay, ax), 4, dt, 2, 40, 24, 5, 6, sel, transpose=1, KH=3, KW=3,
                          out_step=2, out_oy=ay, out_ox=ax, acc=True, seed=9))
    # stride-1 data gradient (mirrored taps, transposed weights) and the strip / fused folds of the replicate-padded one
    CASES.append(case('%s-cfg1-dgrad-s1' % dt, 1, dt, 2, 40, 24, 9, 11, dgrad_taps(K3), transpose=1, acc=True))
    for kid in (1, 4, 5):
        CASES.append(case('%s-cfg%d-fold-strip' % (dt, kid), kid, dt, 2, 40, 24, 9, 7, dgrad_taps_extended(K3R, 2), transpose=1,
                          fold=('strip', 2, 2)))
    for kid, H_, W_, B_, gen in ((1, 8, 8, 2, 1), (1, 16, 16, 2, 1), (4, 16, 16, 2, 1), (1, 12, 20, 2, 1), (2, 12, 20, 1, None), (4, 5, 7, 3, 1),
                                 (5, 8, 8, 2, None), (3, 16, 16, 2, 1)):
        for acc in (False, True):
            CASES.append(case('%s-cfg%d-fold-fused-%dx%d%s' % (dt, kid, H_ + 2, W_ + 2, '-accumulate' if acc else ''), kid, dt, B_, 40, 24,
                              H_, W_, dgrad_taps_extended(K3R, 2), transpose=1, fold=('fused', 2, 2), gen=gen, acc=acc))

# ---- input transform (bf16, 9 taps, whole aligned pieces; configs 1 - 4): the producer's BatchNorm apply (+ ReLU) in the loader
for kid, B_, Ci, H_, W_, reg in ((1, 2, 40, 33, 17, 'ilv9-3'), (1, 5, 64, 8, 8, 'ilv9-9'), (2, 1, 64, 16, 16, 'ilv9-6'), (3, 2, 40, 9, 11, 'ilv9-3'),
                                 (4, 2, 64, 16, 16, 'ilv9-3'), (4, 16, 24, 4, 4, 'ilv9-9')):
    for tf in ('relu', 'affine'):
        CASES.append(case('bf16-cfg%d-in-%s-%d-%dx%d' % (kid, tf, Ci, H_, W_), kid, 'bf16', B_, Ci, 40, H_, W_, K3, in_tf=tf, regime=reg))
CASES.append(case('bf16-cfg1-in-relu-replicate', 1, 'bf16', 2, 40, 40, 9, 11, K3R, pad_mode=1, in_tf='relu', bias=True, relu=True))

# ---- conv_glds_kernel (ids 6 - 8, bf16): 1, 2, 3 chunks of input channels against 2 | 4 K-slices; a ragged channel tile
for kid in (6, 7, 8):
    n = 'bf16-glds%d-' % kid
    for Cin in (32, 64, 96):
        CASES.append(case(n + '%d-40-17x9' % Cin, kid, 'bf16', 2, Cin, 40, 17, 9, K3))
    CASES.append(case(n + '64-72-33x17-replicate', kid, 'bf16', 2, 64, 72, 33, 17, K3R, pad_mode=1))
    CASES.append(case(n + 'accumulate', kid, 'bf16', 2, 64, 40, 17, 9, K3, acc=True))
    CASES.append(case(n + 'res', kid, 'bf16', 2, 96, 40, 17, 9, K3, bias=True, scale=True, shift=True, relu=True, res=True))
    CASES.append(case(n + 'bias-scale-shift-relu', kid, 'bf16', 2, 32, 40, 17, 9, K3, bias=True, scale=True, shift=True, relu=True))
    CASES.append(case(n + 'y-window', kid, 'bf16', 2, 64, 40, 17, 9, K3, yv=(8, 56), xv=(8, 80)))
    CASES.append(case(n + 'fold-fused-14x22', kid, 'bf16', 2, 64, 40, 12, 20, dgrad_taps_extended(K3R, 2), transpose=1, fold=('fused', 2, 2),
                      gen=None if kid == 6 else 1))

# ---- conv_ws_kernel (id 9): cfg = 9 | cap << 8
CASES += [
    case('ws-64-64-16x16-b1', 9, 'bf16', 1, 64, 64, 16, 16, K3),
    case('ws-32-64-16x32', 9, 'bf16', 2, 32, 64, 16, 32, K3R, pad_mode=1),
    case('ws-64-32-32x16-b3-cap1', 9, 'bf16', 3, 64, 32, 32, 16, K3, cfg=9 | (1 << 8)),
    case('ws-64-128-two-blocks', 9, 'bf16', 2, 64, 128, 16, 16, K3, bias=True, scale=True, shift=True, relu=True),
    case('ws-res', 9, 'bf16', 2, 64, 64, 16, 16, K3, scale=True, shift=True, relu=True, res=True),
    case('ws-accumulate-ragged-grid', 9, 'bf16', 2, 64, 64, 24, 20, dgrad_taps(K3), transpose=1, acc=True, cfg=9 | (1 << 8)),
    case('ws-views', 9, 'bf16', 2, 32, 64, 16, 16, K3, xv=(8, 48), yv=(16, 96)),
    case('ws-64-64-replicate-24x20', 9, 'bf16', 2, 64, 64, 24, 20, K3R, pad_mode=1, bias=True, relu=True),
    case('ws-64-32-replicate-cap1', 9, 'bf16', 3, 64, 32, 32, 16, K3R, pad_mode=1, cfg=9 | (1 << 8)),
    case('ws-64-128-replicate-res', 9, 'bf16', 2, 64, 128, 16, 16, K3R, pad_mode=1, scale=True, shift=True, relu=True, res=True),
    case('ws-32-64-replicate-accumulate', 9, 'bf16', 2, 32, 64, 16, 16, K3R, pad_mode=1, acc=True),
    case('ws-fold-fused-18x18', 9, 'bf16', 2, 64, 64, 16, 16, dgrad_taps_extended(K3R, 2), transpose=1, fold=('fused', 2, 2)),
    case('ws-fold-fused-18x18-accumulate', 9, 'bf16', 2, 32, 64, 16, 16, dgrad_taps_extended(K3R, 2), transpose=1, fold=('fused', 2, 2),
         acc=True),
]
# ---- conv_ls_kernel (id 10): cfg = 10 | cap << 8 | NI << 16 | bit 20 two-tile items | bit 21 single tiles only
CASES += [
    case('ls-64-32-16x16-cap1', 10, 'bf16', 2, 64, 32, 16, 16, K3, cfg=10 | (1 << 8)),
    case('ls-128-64-16x32-ni2', 10, 'bf16', 2, 128, 64, 16, 32, K3R, pad_mode=1, cfg=10 | (2 << 16)),
    case('ls-128-64-ni1', 10, 'bf16', 2, 128, 64, 16, 16, K3, cfg=10 | (1 << 16), bias=True, relu=True),
    case('ls-two-tile-items', 10, 'bf16', 4, 128, 64, 16, 32, K3, cfg=10 | (1 << 8) | (2 << 16) | (1 << 20), bias=True, scale=True, shift=True, relu=True),
    case('ls-single-tiles-only', 10, 'bf16', 4, 128, 64, 16, 32, K3, cfg=10 | (1 << 8) | (2 << 16) | (1 << 21), bias=True, scale=True, shift=True, relu=True),
    case('ls-res', 10, 'bf16', 2, 96, 96, 16, 16, K3, scale=True, shift=True, relu=True, res=True),
    case('ls-accumulate', 10, 'bf16', 2, 64, 96, 16, 16, dgrad_taps(K3), transpose=1, acc=True),
    case('ls-64-32-replicate-cap1', 10, 'bf16', 2, 64, 32, 16, 16, K3R, pad_mode=1, cfg=10 | (1 << 8)),
    case('ls-96-96-replicate-res', 10, 'bf16', 2, 96, 96, 16, 16, K3R, pad_mode=1, scale=True, shift=True, relu=True, res=True),
    case('ls-two-tile-items-replicate', 10, 'bf16', 4, 128, 64, 16, 32, K3R, pad_mode=1, cfg=10 | (1 << 8) | (2 << 16) | (1 << 20), bias=True, relu=True),
    case('ls-views', 10, 'bf16', 2, 64, 32, 16, 16, K3, xv=(8, 80), yv=(16, 64)),
]
# ---- conv_thin_kernel (id 12, fp32)
for ci, co in ((16, 16), (16, 32), (32, 16), (32, 32)):
    CASES.append(case('thin-%d-%d-zero' % (ci, co), 12, 'f32', 2, ci, co, 16, 16, K3, bias=True))
    CASES.append(case('thin-%d-%d-replicate' % (ci, co), 12, 'f32', 3, ci, co, 16, 32, K3R, pad_mode=1, scale=True, shift=True, relu=True))
CASES.append(case('thin-accumulate', 12, 'f32', 2, 32, 16, 16, 16, dgrad_taps(K3), transpose=1, acc=True))
# ---- conv_stem16_kernel (id 13): 16 taps over the 16 channels of the space-to-depth image -> 64
STEM = [(kh, kw, kh - 2, kw - 2) for kh in range(4) for kw in range(4)]
CASES.append(case('stem16-eval', 13, 'bf16', 1, 16, 64, 16, 16, STEM, scale=True, shift=True, relu=True))
CASES.append(case('stem16-plain-b3', 13, 'bf16', 3, 16, 64, 16, 32, STEM))


def _vec(C, seed, kind):
    g = torch.Generator().manual_seed(seed)
    if kind == 'scale':                                                    # [0.5, 2], both signs
        return ((0.5 + 1.5 * torch.rand(C, generator=g)) * torch.where(torch.rand(C, generator=g) < 0.25, -1.0, 1.0)).double()
    return torch.randn(C, generator=g).double()


def build(c):
    """Operands (CPU) and the float64 reference of a case."""
    B, Cin, Cout, H, W = c['B'], c['Cin'], c['Cout'], c['H'], c['W']
    taps = c['taps']
    x = mk(B, Cin, H, W, 10 * c['seed']).permute(0, 2, 3, 1).contiguous()
    D0, D1 = (Cin, Cout) if c['transpose'] else (Cout, Cin)
    w = master_weight(D0, D1, c['KH'], c['KW'], Cin, len(taps), 10 * c['seed'] + 1)
    tap_k, offs = [(t[0], t[1]) for t in taps], [(t[2], t[3]) for t in taps]
    wt = tap_weights(w, tap_k, c['transpose'])
    o = dict(x=x, w=w, tap_k=tap_k, offs=offs, wt=wt)
    o['bias'] = _vec(Cout, 3, 'bias').float().double() if c['bias'] else None
    o['scale'] = _vec(Cout, 4, 'scale').float().double() if c['scale'] else None
    o['shift'] = _vec(Cout, 5, 'shift').float().double() if c['shift'] else None
    fold = c['fold']
    gH, gW = (c['yH'], c['yW']) if fold and fold[0] == 'fused' else (c['OH'], c['OW'])
    o['res'] = mk(B, Cout, gH, gW, 10 * c['seed'] + 2).permute(0, 2, 3, 1).double() if c['res'] else None
    o['old'] = mk(B, Cout, gH, gW, 10 * c['seed'] + 3).permute(0, 2, 3, 1).double() if c['acc'] else None
    old = o['old']
    if fold and fold[0] == 'strip' and old is not None:
        raise AssertionError('strip cases here do not accumulate')
    if c['in_tf']:
        # multiples of 1/8 and 1/4: x in_scale + in_shift is exact in fp32 (no double rounding in the kernel's transform), in_shift != 0
        # so that a transformed pad value would show
        g = torch.Generator().manual_seed(77)
        o['in_tf'] = (torch.randint(4, 17, (Cin,), generator=g).double() / 8, torch.randint(1, 9, (Cin,), generator=g).double() / 4 - 1.125,
                      c['in_tf'] == 'relu')
    o['ref'] = conv_ref(x, wt, offs, c['in_step'], c['pad_mode'], c['OH'], c['OW'], c['dtype'], o['bias'], o['scale'], o['shift'], c['relu'],
                        o['res'], old, (fold[1], fold[2]) if fold and fold[0] == 'fused' else None, o.get('in_tf'))
    return o
