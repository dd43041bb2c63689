"""The weight-gradient C-ABI for the tests: salt_conv_wgrad + salt_wgrad_reduce on device tensors, which kernel family the plan
picks (salt_conv_wgrad_kernel_id: host only, no launch), and the float64 weight gradient of the same operands.  One place that fills
salt_conv_wgrad_args / salt_wgrad_reduce_args for test_gpu_wgrad.py, test_gpu_wgrad_ls.py and test_gpu_conv_thin.py."""
import ctypes

import torch

LS, THIN, FAST, FAST32, GENERIC = 1, 2, 3, 4, 5          # salt_conv_wgrad_kernel_id (include/saltnet.h)
RASTER = [(dy - 1, dx - 1) for dy in range(3) for dx in range(3)]          # nn.Conv2d(k3, padding 1)
RASTER_REP = [(dy - 2, dx) for dy in range(3) for dx in range(3)]          # ReplicationPad2d((0, 2, 2, 0)) + valid conv, clamped reads
_DTYPE = {torch.float32: 0, torch.bfloat16: 1}


def mk(B, C, H, W, seed):
    """[B,C,H,W] fp32 normal values that bf16 represents exactly: every product is exact in fp32 on both dtypes' kernels."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, C, H, W, generator=g).bfloat16().float()


def nhwc(x, dtype):
    return x.permute(0, 2, 3, 1).contiguous().to(dtype)


def wgrad_args(dtype, p_ptr, p_shape, q_ptr, q_shape, taps, q_step=1, pad_mode=0, q_plane=0):
    """p_shape / q_shape = (B, H, W, C, cs).  dtype: a torch dtype."""
    import salt_amd  # noqa: F401
    from salt_amd._abi import STRUCTS, fill
    from salt_amd.engine import shaped_view
    return fill(STRUCTS['salt_conv_wgrad_args'](), dtype=_DTYPE[dtype], p=shaped_view(p_ptr, *p_shape), q=shaped_view(q_ptr, *q_shape),
                ntaps=len(taps), tap_dy=[t[0] for t in taps], tap_dx=[t[1] for t in taps], q_step=q_step, pad_mode=pad_mode, q_plane=q_plane)


def wgrad_kernel_id(S):
    from salt_amd._abi import lib
    return lib.salt_conv_wgrad_kernel_id(ctypes.byref(S))


def wgrad_hip(p_nhwc, q_nhwc, taps, pad_mode, nsplit=None, q_planar=False, Ca=None, Cb=None, q_step=1, KH=3, KW=3, tap_k=None, expect_id=None):
    """p_nhwc [B,H,W,Csa] / q_nhwc [B,QH,QW,Csb] bf16 or fp32 device tensors (views of the Ca / Cb leading channels of their pixel
    stride); tap t of `taps` lands at tap_k[t] = (kh, kw) of the [Ca][Cb][KH][KW] fp32 gradient (default: raster order).  Slab and
    gradient are NaN-prefilled: whatever the launch does not write stays NaN.  Returns (gradient on the CPU, nsplit)."""
    from salt_amd._abi import STRUCTS, lib, fill, check
    B, H, W, _ = p_nhwc.shape
    _, QH, QW, _ = q_nhwc.shape
    csa, csb = p_nhwc.stride(2), q_nhwc.stride(2)                 # pixel stride of a channel slice of a wider buffer
    Ca = csa if Ca is None else Ca
    Cb = csb if Cb is None else Cb
    nt = len(taps)
    tap_k = [(t // KW, t % KW) for t in range(nt)] if tap_k is None else tap_k
    # planar: q_nhwc is [planes][B,QH,QW,64] - the view names one plane's pixel stride, q_plane the plane stride
    S = wgrad_args(p_nhwc.dtype, p_nhwc.data_ptr(), (B, H, W, Ca, csa), q_nhwc.data_ptr(), (B, QH, QW, Cb, 64 if q_planar else csb), taps,
                   q_step, pad_mode, B * QH * QW * 64 if q_planar else 0)
    if expect_id is not None:
        kid = wgrad_kernel_id(S)
        assert kid == expect_id, 'the plan runs kernel family %d, this case is meant for %d' % (kid, expect_id)
    ns = lib.salt_conv_wgrad_nsplit(ctypes.byref(S))
    assert ns >= 1, lib.salt_last_error()
    if nsplit is not None:
        ns = nsplit
    part = torch.full((ns, nt, Ca, Cb), float('nan'), device='cuda:0')
    S.partials = part.data_ptr()
    S.nsplit = ns
    st = torch.cuda.current_stream().cuda_stream
    check(lib.salt_conv_wgrad(ctypes.byref(S), st), 'salt_conv_wgrad')
    grad = torch.full((Ca, Cb, KH, KW), float('nan'), device='cuda:0')
    R = fill(STRUCTS['salt_wgrad_reduce_args'](), partials=part.data_ptr(), nsplit=ns, ntaps=nt, Ca=Ca, Cb=Cb, KH=KH, KW=KW,
             tap_kh=[k[0] for k in tap_k], tap_kw=[k[1] for k in tap_k], grad=grad.data_ptr(), accumulate=0)
    check(lib.salt_wgrad_reduce(ctypes.byref(R), st), 'salt_wgrad_reduce')
    torch.cuda.synchronize()
    return grad.cpu(), ns


def wgrad_ref(p, q, taps, q_step=1, pad_mode=0):
    """p [B,Ca,PH,PW], q [B,Cb,QH,QW] -> float64 dW [ntaps][Ca][Cb], dW[t][a][b] = sum_p P[p, a] Q[pad(p q_step + tap_t), b]
    (include/saltnet.h): reads outside Q are zero (pad_mode 0) or clamped to the border (pad_mode 1)."""
    B, Ca, PH, PW = p.shape
    _, Cb, QH, QW = q.shape
    pd, qd = p.double(), q.double()
    out = torch.zeros(len(taps), Ca, Cb, dtype=torch.float64)
    for t, (dy, dx) in enumerate(taps):
        iy = torch.arange(PH) * q_step + dy
        ix = torch.arange(PW) * q_step + dx
        g = qd[:, :, iy.clamp(0, QH - 1)][:, :, :, ix.clamp(0, QW - 1)]
        if not pad_mode:
            ok = ((iy >= 0) & (iy < QH)).double()[:, None] * ((ix >= 0) & (ix < QW)).double()[None, :]
            g = g * ok
        out[t] = torch.einsum('bahw,bchw->ac', pd, g)
    return out


def rel_l2(got, ref):
    return float((got.double() - ref.double()).norm() / ref.double().norm())


# bf16 3x3 shapes that conv_wgrad_ls_kernel takes by default and the previous kernels (conv_wgrad_fast8_kernel /
# conv_wgrad_fast_kernel) with SALT_WGRAD_LS=0.  (B, QH, QW, Ca, Cb, q_step, pad_mode)
PREVIOUS_KERNEL_SHAPES = [
    (2, 32, 32, 64, 64, 1, 0),        # fast8
    (3, 33, 17, 72, 40, 1, 0),        # fast8: ragged rows, columns and channel blocks
    (3, 33, 17, 72, 40, 1, 1),
    (5, 8, 8, 160, 64, 1, 0),         # fast<9, 8>: two images per tile, partial batch tile
    (3, 17, 9, 72, 40, 2, 0),         # nn.Conv2d(k3, s2, p1): fast<9, 4, false>
]


def previous_shape_operands(shape, i):
    B, QH, QW, Ca, Cb, q_step, pad_mode = shape
    PH, PW = (QH - 1) // q_step + 1, (QW - 1) // q_step + 1
    return mk(B, Ca, PH, PW, 100 + 2 * i), mk(B, Cb, QH, QW, 101 + 2 * i), (RASTER_REP if pad_mode else RASTER)


def run_previous_shapes(expect_id):
    """[gradient] of PREVIOUS_KERNEL_SHAPES on whatever kernels this process' library picks (the library reads SALT_WGRAD_LS once)."""
    outs = []
    for i, shape in enumerate(PREVIOUS_KERNEL_SHAPES):
        p, q, taps = previous_shape_operands(shape, i)
        got, _ = wgrad_hip(nhwc(p, torch.bfloat16).cuda(), nhwc(q, torch.bfloat16).cuda(), taps, shape[6], q_step=shape[5], expect_id=expect_id)
        outs.append(got)
    return outs
