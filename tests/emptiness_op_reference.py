"""Plain float64 reference of the classifier head (salt_pool_head / salt_pool_head_bwd), in the style of op_reference.py: the textbook
definition with loops over the windows, NHWC ``torch.float64`` activations, NOT a transcription of the kernel.  The view / guard
helpers come from op_reference.py; ``test_emptiness_cpu.py`` pins these functions against the reference's own F15_pool_head fixture."""
import torch

from op_reference import F64, Placed, VARIANTS, VIEW_CASES, guard_check, guard_fill, make_view, round_to, torch_dtype  # noqa: F401

POOL = 8


def pool_head(x, w, bias=None):
    """x [B,H,W,C], w [K,C], bias [K] or None -> (pooled [B,OH,OW,C], logits NCHW [B,K,OH,OW]); OH = H // 8, OW = W // 8."""
    B, H, W, C = x.shape
    OH, OW, K = H // POOL, W // POOL, w.shape[0]
    pooled = torch.zeros(B, OH, OW, C, dtype=F64)
    logits = torch.zeros(B, K, OH, OW, dtype=F64)
    for oh in range(OH):
        for ow in range(OW):
            for iy in range(POOL * oh, POOL * oh + POOL):
                for ix in range(POOL * ow, POOL * ow + POOL):
                    pooled[:, oh, ow] += x[:, iy, ix]
            pooled[:, oh, ow] /= POOL * POOL
            for j in range(K):
                logits[:, j, oh, ow] = (pooled[:, oh, ow] * w[j]).sum(-1) + (bias[j] if bias is not None else 0.0)
    return pooled, logits


def pool_head_bwd(dlogits, w, pooled, H, W, old=None, accumulate=False):
    """dlogits NCHW [B,K,OH,OW] -> (dx [B,H,W,C], gw [K,C], gb [K]).  Pixels that belong to no window get no gradient: zero, or with
    ``accumulate`` their old value."""
    B, K, OH, OW = dlogits.shape
    C = w.shape[1]
    dx = torch.zeros(B, H, W, C, dtype=F64)
    gw = torch.zeros(K, C, dtype=F64)
    gb = torch.zeros(K, dtype=F64)
    for oh in range(OH):
        for ow in range(OW):
            for j in range(K):
                d = dlogits[:, j, oh, ow]                                         # [B]
                gb[j] += d.sum()
                gw[j] += (d[:, None] * pooled[:, oh, ow]).sum(0)
                for iy in range(POOL * oh, POOL * oh + POOL):
                    for ix in range(POOL * ow, POOL * ow + POOL):
                        dx[:, iy, ix] += d[:, None] * w[j][None, :] / (POOL * POOL)
    return (dx + old if accumulate else dx), gw, gb


def in_window_mask(H, W):
    """[H,W] bool: the pixels some 8x8 window covers."""
    m = torch.zeros(H, W, dtype=torch.bool)
    m[:H // POOL * POOL, :W // POOL * POOL] = True
    return m
