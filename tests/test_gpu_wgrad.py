"""The split-K weight-gradient kernels of csrc/conv_wgrad.hip, each asked for directly through the C-ABI: salt_conv_wgrad +
salt_wgrad_reduce against the float64 weight gradient of the same operands (autograd of common_blocks/models.py:133 over
architectures/base.py:7-57 / unet_models.py:21-60 in the reference).  Every case names the kernel family it is meant for and
asserts it through salt_conv_wgrad_kernel_id, so a change of the planner that moves a case elsewhere is a test error and not a
silent loss of coverage.  Operands are bf16-representable in both dtypes: products are exact in fp32, only the summation order
differs from the reference, hence the rel-L2 bound of test_gpu_wgrad_ls.py.  Slab and gradient start as NaN.

The bf16 kernels that conv_wgrad_ls_kernel replaced by default (conv_wgrad_fast8_kernel, conv_wgrad_fast_kernel<9, *> on aligned
raster 3x3 launches) are reached with SALT_WGRAD_LS=0 in test_gpu_wgrad_ls.py's child process."""
import pytest
import torch

from wgrad_abi import FAST, FAST32, GENERIC, RASTER, RASTER_REP, mk, nhwc, rel_l2, wgrad_args, wgrad_hip, wgrad_kernel_id, wgrad_ref

BF16, F32 = torch.bfloat16, torch.float32
PHASE4 = [(0, 0), (0, 1), (1, 0), (1, 1)]                                   # one output-parity phase of ConvTranspose2d(k4, s2)
DILATED = [(2 * dy - 2, 2 * dx - 2) for dy in range(3) for dx in range(3)]     # 3x3, dilation 2
RASTER8 = RASTER[:8]                                                        # a stem half: 8 taps of the 3x3 window
RASTER8_REP = RASTER_REP[:8]


def case(name, kid, dtype, B, H, W, Ca, Cb, taps, q_step=1, pad_mode=0, p_cs=None, p_off=0, planar=False):
    return pytest.param(dict(kid=kid, dtype=dtype, B=B, H=H, W=W, Ca=Ca, Cb=Cb, taps=taps, q_step=q_step, pad_mode=pad_mode, p_cs=p_cs,
                             p_off=p_off, planar=planar), id=name)


CASES = [
    # ---- conv_wgrad_kernel<bf16_t, NT> (generic)
    case('generic-bf16-nt9-ragged', GENERIC, BF16, 3, 7, 5, 10, 13, RASTER),          # scalar load_piece path (cs 10 / 13), partial batch tile
    case('generic-bf16-nt1-ragged', GENERIC, BF16, 3, 7, 5, 10, 13, [(0, 0)]),
    case('generic-bf16-nt3', GENERIC, BF16, 2, 9, 11, 16, 24, [(0, -1), (0, 0), (0, 1)]),     # a (1, 3) kernel, whole pieces
    case('generic-bf16-nt4-ragged', GENERIC, BF16, 2, 6, 9, 12, 20, PHASE4),
    case('generic-bf16-step2', GENERIC, BF16, 3, 5, 4, 24, 13, RASTER, q_step=2),           # 64-pixel K tiles: the 17 x 9 halo
    case('generic-bf16-replicate', GENERIC, BF16, 3, 7, 5, 10, 13, RASTER_REP, pad_mode=1),
    case('generic-bf16-halo-not-pipelined', GENERIC, BF16, 2, 8, 8, 72, 40, DILATED, q_step=2),
    # ---- conv_wgrad_kernel<float, 9>: 8 x 8 maps (tw_log2 = 3 keeps fast32 away); ksplit 4, 2, 3, 0
    case('generic-f32-ksplit4', GENERIC, F32, 3, 8, 8, 24, 16, RASTER),
    case('generic-f32-ksplit2', GENERIC, F32, 3, 8, 8, 24, 72, RASTER),
    case('generic-f32-ksplit3', GENERIC, F32, 3, 8, 8, 72, 24, RASTER_REP, pad_mode=1),
    case('generic-f32-ksplit0', GENERIC, F32, 3, 8, 8, 72, 40, RASTER),
    case('generic-f32-b5', GENERIC, F32, 5, 8, 8, 24, 72, RASTER),
    case('generic-f32-b5-two-images-per-tile', GENERIC, F32, 5, 4, 8, 24, 72, RASTER),        # fp32 rows: nb = 2 needs the 4 x 8 map
    # ---- conv_wgrad_fast_kernel<NT, KS, PAD>
    case('fast-1x1', FAST, BF16, 3, 8, 8, 24, 40, [(0, 0)]),                                 # <1, 8, false>, two images per tile
    case('fast-1x1-step2', FAST, BF16, 2, 5, 9, 24, 40, [(0, 0)], q_step=2),                 # <1, 4, false>
    case('fast-8taps', FAST, BF16, 3, 9, 11, 24, 40, RASTER8),                               # <9, 8, false>: slot 8 repeats tap 0, never stored
    case('fast-8taps-replicate', FAST, BF16, 3, 9, 11, 24, 40, RASTER8_REP, pad_mode=1),     # <9, 8, true>
    case('fast-step2-replicate', FAST, BF16, 3, 5, 7, 72, 40, RASTER_REP, q_step=2, pad_mode=1),      # <9, 4, true>: ls declines it
    case('fast-p-slice', FAST, BF16, 3, 8, 8, 24, 40, [(0, 0)], p_cs=48, p_off=8),           # P = channels [8, 32) of a 48-channel buffer
    case('fast-planar-q', FAST, BF16, 2, 9, 11, 24, 128, RASTER8, planar=True),              # two 64-channel planes
]
# ---- conv_wgrad_fast32_kernel<PAD, KSPLIT, SIDE>: 1/0, 4/0, 2/0, 2/1; sizes conv_wgrad_thin declines
for (H_, W_) in ((9, 11), (33, 17)):
    for (Ca_, Cb_) in ((40, 72), (24, 16), (24, 40), (40, 24)):
        for pad_ in (0, 1):
            CASES.append(case('fast32-%dx%d-%d-%d-%s' % (H_, W_, Ca_, Cb_, 'replicate' if pad_ else 'zero'), FAST32, F32, 3, H_, W_, Ca_, Cb_,
                              RASTER_REP if pad_ else RASTER, pad_mode=pad_))


def _tap_k(taps):
    """Kernel position of every tap in the smallest kernel that holds the list."""
    y0, x0 = min(t[0] for t in taps), min(t[1] for t in taps)
    k = [(t[0] - y0, t[1] - x0) for t in taps]
    return k, max(a for a, _ in k) + 1, max(b for _, b in k) + 1


def test_cases_land_on_the_kernel_they_name():
    """Host only (no launch): the plan of every case, before any of them runs."""
    for c in CASES:
        c = c.values[0]
        qs = c['q_step']
        S = wgrad_args(c['dtype'], 4096, (c['B'], c['H'], c['W'], c['Ca'], c['p_cs'] or c['Ca']), 8192,
                       (c['B'], c['H'] * qs, c['W'] * qs, c['Cb'], 64 if c['planar'] else c['Cb']), c['taps'], qs, c['pad_mode'],
                       c['B'] * c['H'] * qs * c['W'] * qs * 64 if c['planar'] else 0)
        assert wgrad_kernel_id(S) == c['kid'], c


@pytest.mark.gpu
@pytest.mark.parametrize('c', CASES)
def test_wgrad_kernel_vs_float64(c):
    """generic-bf16-halo-not-pipelined: an 8 x 8 tile of a stride-2 convolution with a dilated 3x3 window reads a 19 x 19 halo = 2888
    pieces > MAXQ * 256, which 64-pixel K tiles still hold in LDS - the one legal plan here whose halo takes the generic kernel's
    non-pipelined branch."""
    B, H, W, Ca, Cb, taps, qs = c['B'], c['H'], c['W'], c['Ca'], c['Cb'], c['taps'], c['q_step']
    p, q = mk(B, Ca, H, W, 21), mk(B, Cb, H * qs, W * qs, 22)
    pd, qd = nhwc(p, c['dtype']).cuda(), nhwc(q, c['dtype']).cuda()
    if c['p_cs']:
        buf = torch.randn(B, H, W, c['p_cs']).to(c['dtype']).cuda()
        buf[..., c['p_off']:c['p_off'] + Ca] = pd
        pd = buf[..., c['p_off']:]
    if c['planar']:
        qd = torch.stack([qd[..., i:i + 64] for i in range(0, Cb, 64)]).contiguous().view(-1, H * qs, W * qs, 64)[:B]
    tap_k, KH, KW = _tap_k(taps)
    got, ns = wgrad_hip(pd, qd, taps, c['pad_mode'], q_planar=c['planar'], Ca=Ca, Cb=Cb, q_step=qs, KH=KH, KW=KW, tap_k=tap_k, expect_id=c['kid'])
    got = torch.stack([got[:, :, kh, kw] for kh, kw in tap_k])                # the kernel positions of the launch's taps
    ref = wgrad_ref(p, q, taps, qs, c['pad_mode'])
    err = rel_l2(got, ref)
    print('rel-L2 %.3e nsplit %d' % (err, ns))
    assert torch.isfinite(got).all()
    assert err <= 2e-5, 'rel-L2 %.3e (nsplit %d)' % (err, ns)          # exact products, fp32 accumulation in another order
