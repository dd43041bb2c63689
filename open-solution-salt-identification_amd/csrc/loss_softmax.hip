// loss_softmax.hip — the softmax head: softmax / its Jacobian, Lovasz-softmax and Dice + cross entropy.
//
// Everything here streams fp32 NCHW logits [B,C,HW] with 2 <= C <= 4: one thread owns a pixel, holds its C values in registers and
// reads / writes every channel plane coalesced along HW.  The Lovasz-softmax is the sort of loss_common.h instantiated with the
// absolute-error policy over the B*C planes (a plane is a contiguous row of HW floats, exactly an image of the hinge form).  Dice +
// cross entropy follows salt_bce_dice: per-part partial sums, a fixed-order finalize in double, a gradient pass; no floating-point
// atomics anywhere, so reruns are bit-identical.
#include "loss_common.h"

namespace {

// p_c and (optionally) logsumexp of one pixel's C logits, the maximum subtracted first: exp arguments are <= 0, the sum is >= 1
template <int C>
__device__ __forceinline__ float softmax_px(const float (&z)[C], float (&p)[C]) {
    float m = z[0];
#pragma unroll
    for (int c = 1; c < C; ++c) m = fmaxf(m, z[c]);
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) { p[c] = expf(z[c] - m); s += p[c]; }
    const float inv = 1.f / s;
#pragma unroll
    for (int c = 0; c < C; ++c) p[c] *= inv;
    return m + logf(s);
}

template <int C>
__global__ __launch_bounds__(256) void softmax_kernel(const float* x, float* y, int B, int HW) {      // y may alias x
    const int64_t n = (int64_t)B * HW;
    for (int64_t q = blockIdx.x * 256LL + threadIdx.x; q < n; q += gridDim.x * 256LL) {
        const int64_t b = q / HW, o = b * C * HW + (q - b * HW);
        float z[C], p[C];
#pragma unroll
        for (int c = 0; c < C; ++c) z[c] = x[o + (int64_t)c * HW];
        softmax_px<C>(z, p);
#pragma unroll
        for (int c = 0; c < C; ++c) y[o + (int64_t)c * HW] = p[c];
    }
}

template <int C>
__global__ __launch_bounds__(256) void softmax_bwd_kernel(const float* p, const float* dp, float* dz, int B, int HW) {      // dz may alias dp
    const int64_t n = (int64_t)B * HW;
    for (int64_t q = blockIdx.x * 256LL + threadIdx.x; q < n; q += gridDim.x * 256LL) {
        const int64_t b = q / HW, o = b * C * HW + (q - b * HW);
        float pp[C], dd[C], dot = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) { pp[c] = p[o + (int64_t)c * HW]; dd[c] = dp[o + (int64_t)c * HW]; dot += pp[c] * dd[c]; }
#pragma unroll
        for (int c = 0; c < C; ++c) dz[o + (int64_t)c * HW] = pp[c] * (dd[c] - dot);
    }
}

// ---------------------------------------------------------------- Dice + cross entropy
// block = (image b, part k of the plane); partials [block][3C+1]: per class (sum p t, sum p, sum t), then sum (logsumexp - z_y)
template <int C>
__global__ __launch_bounds__(256) void dice_ce_partial_kernel(const float* __restrict__ z, const float* __restrict__ t, int HW, int ppp, int per,
                                                              float* __restrict__ partials) {
    __shared__ float sm4[4];
    const int b = blockIdx.x / ppp, part = blockIdx.x % ppp;
    const int i0 = part * per, i1 = min(i0 + per, HW);
    float s_pt[C], s_p[C], s_t[C], s_ce = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) { s_pt[c] = 0.f; s_p[c] = 0.f; s_t[c] = 0.f; }
    for (int i = i0 + threadIdx.x; i < i1; i += 256) {
        const int64_t o = (int64_t)b * C * HW + i;
        float zz[C], tt[C], p[C];
#pragma unroll
        for (int c = 0; c < C; ++c) { zz[c] = z[o + (int64_t)c * HW]; tt[c] = t[o + (int64_t)c * HW]; }
        const float lse = softmax_px<C>(zz, p);
        float zy = zz[0], tmax = tt[0];                          // y = argmax_c t, first maximum
#pragma unroll
        for (int c = 1; c < C; ++c) if (tt[c] > tmax) { tmax = tt[c]; zy = zz[c]; }
        s_ce += lse - zy;
#pragma unroll
        for (int c = 0; c < C; ++c) { s_pt[c] += p[c] * tt[c]; s_p[c] += p[c]; s_t[c] += tt[c]; }
    }
    float* o = partials + (int64_t)blockIdx.x * (3 * C + 1);
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const float r0 = block_sum_256(s_pt[c], sm4), r1 = block_sum_256(s_p[c], sm4), r2 = block_sum_256(s_t[c], sm4);
        if (threadIdx.x == 0) { o[3 * c] = r0; o[3 * c + 1] = r1; o[3 * c + 2] = r2; }
    }
    const float r3 = block_sum_256(s_ce, sm4);
    if (threadIdx.x == 0) o[3 * C] = r3;
}

__global__ void dice_ce_finalize_kernel(const float* partials, int nparts, int B, int C, int HW, float dw, float cw, float smooth, float scale,
                                        float* sums, float* loss) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const int W = 3 * C + 1;
    double dice = 0.0, ce = 0.0;
    for (int k = 0; k < nparts; ++k) ce += partials[(int64_t)k * W + 3 * C];
    for (int c = 0; c < C; ++c) {
        double pt = 0.0, p = 0.0, t = 0.0;
        for (int k = 0; k < nparts; ++k) {
            const float* o = partials + (int64_t)k * W + 3 * c;
            pt += o[0]; p += o[1]; t += o[2];
        }
        sums[c * 3 + 0] = (float)pt; sums[c * 3 + 1] = (float)p; sums[c * 3 + 2] = (float)t;
        if (c > 0) dice += 1.0 - (2.0 * pt + smooth) / (p + t + smooth + 1e-7);
    }
    sums[3 * C] = (float)ce;
    loss[0] = (float)((dw * dice / (C - 1) + cw * ce / ((double)B * HW)) * scale);
}

// dp_c = dw / (C-1) d dice_c / d p_c = dw / (C-1) (-(2 t_c) / D_c + (2 I_c + smooth) / D_c^2) for c >= 1, 0 for the background;
// dz_j = scale (p_j (dp_j - sum_c p_c dp_c) + cw / N (p_j - [j == y]))
template <int C>
__global__ __launch_bounds__(256) void dice_ce_grad_kernel(const float* __restrict__ z, const float* __restrict__ t, int B, int HW,
                                                           const float* __restrict__ sums, float dw, float cw, float smooth, float scale,
                                                           float* __restrict__ dz) {
    const int64_t n = (int64_t)B * HW;
    float ka[C], kb[C];                                          // dp_c = kb_c - t_c ka_c
    ka[0] = 0.f; kb[0] = 0.f;
#pragma unroll
    for (int c = 1; c < C; ++c) {
        const float D = sums[c * 3 + 1] + sums[c * 3 + 2] + smooth + 1e-7f, w = dw / (float)(C - 1);
        ka[c] = w * 2.f / D;
        kb[c] = w * (2.f * sums[c * 3] + smooth) / (D * D);
    }
    const float cn = cw / (float)n;
    for (int64_t q = blockIdx.x * 256LL + threadIdx.x; q < n; q += gridDim.x * 256LL) {
        const int64_t b = q / HW, o = b * C * HW + (q - b * HW);
        float zz[C], tt[C], p[C], dp[C], dot = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) { zz[c] = z[o + (int64_t)c * HW]; tt[c] = t[o + (int64_t)c * HW]; }
        softmax_px<C>(zz, p);
        int y = 0; float tmax = tt[0];
#pragma unroll
        for (int c = 1; c < C; ++c) if (tt[c] > tmax) { tmax = tt[c]; y = c; }
#pragma unroll
        for (int c = 0; c < C; ++c) { dp[c] = kb[c] - tt[c] * ka[c]; dot += p[c] * dp[c]; }
#pragma unroll
        for (int c = 0; c < C; ++c) dz[o + (int64_t)c * HW] = scale * (p[c] * (dp[c] - dot) + cn * (p[c] - (c == y ? 1.f : 0.f)));
    }
}

int stream_blocks(int64_t n) { return (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096); }
bool shape_ok(int B, int C, int HW) { return B >= 1 && C >= 2 && C <= 4 && HW >= 1; }

// launch kern<C> for the run-time C in 2 .. 4 (checked by the caller)
#define SALT_SOFTMAX_C(C_, KERN, ...) \
    ((C_) == 2 ? salt_launch(KERN<2>, __VA_ARGS__) : (C_) == 3 ? salt_launch(KERN<3>, __VA_ARGS__) : salt_launch(KERN<4>, __VA_ARGS__))

}  // namespace

extern "C" int salt_softmax(const salt_softmax_args* a, void* stream) {
    if (!a || !a->x || !a->y || !shape_ok(a->B, a->C, a->HW)) SALT_FAIL(SALT_E_BADARG, "softmax: needs x, y, B >= 1, HW >= 1 and 2 <= C <= 4");
    const int64_t n = (int64_t)a->B * a->HW;
    return SALT_SOFTMAX_C(a->C, softmax_kernel, dim3(stream_blocks(n)), dim3(256), 0, (hipStream_t)stream, a->x, a->y, a->B, a->HW);
}

extern "C" int salt_softmax_bwd(const salt_softmax_bwd_args* a, void* stream) {
    if (!a || !a->p || !a->dp || !a->dz || !shape_ok(a->B, a->C, a->HW))
        SALT_FAIL(SALT_E_BADARG, "softmax_bwd: needs p, dp, dz, B >= 1, HW >= 1 and 2 <= C <= 4");
    const int64_t n = (int64_t)a->B * a->HW;
    return SALT_SOFTMAX_C(a->C, softmax_bwd_kernel, dim3(stream_blocks(n)), dim3(256), 0, (hipStream_t)stream, a->p, a->dp, a->dz, a->B, a->HW);
}

extern "C" int salt_lovasz_softmax(const salt_lovasz_softmax_args* a, void* stream) {
    if (!a || !a->probas || !a->target || !shape_ok(a->B, a->C, a->HW) || !a->ws_keys || !a->ws_vals || !a->loss_per_row || !a->loss)
        SALT_FAIL(SALT_E_BADARG, "lovasz_softmax: needs probas, target, workspaces, loss_per_row, loss, B >= 1, HW >= 1 and 2 <= C <= 4");
    if ((int64_t)a->B * a->C > (1 << 20)) SALT_FAIL(SALT_E_BADARG, "lovasz_softmax: %d x %d rows", a->B, a->C);
    // rows (b, c) of HW contiguous floats: the hinge's images with B' = B C, P' = HW
    salt_lovasz_args r{};
    r.logits = a->probas; r.target = a->target; r.B = a->B * a->C; r.P = a->HW; r.ws_keys = a->ws_keys; r.ws_vals = a->ws_vals;
    r.loss_per_image = a->loss_per_row; r.loss = a->loss; r.dlogits = a->dprobas; r.loss_scale = a->loss_scale; r.ws_split = a->ws_split;
    r.ws_flat = a->ws_flat;
    if (const char* why = lovasz_flags_refusal(a->flags, a->ignore, true)) SALT_FAIL(SALT_E_BADARG, "lovasz_softmax: %s (flags 0x%x)", why, a->flags);
    if ((a->flags & SALT_LOVASZ_ONLY_PRESENT) && !a->ws_present) SALT_FAIL(SALT_E_BADARG, "lovasz_softmax: only-present needs ws_present");
    const bool flat = a->flags & SALT_LOVASZ_BATCH_FLAT;
    const int64_t N = flat ? (int64_t)a->B * a->HW : a->HW;
    if (N > (a->flags ? LOVASZ_MAX_ROW_VOID : LOVASZ_MAX_ROW)) SALT_FAIL(SALT_E_BADARG, "lovasz_softmax: a row of %lld elements", (long long)N);
    if (!a->flags) return lovasz_launch<AbsError>(&r, (hipStream_t)stream);
    LovaszX x{};
    x.ignore = a->ignore; x.HW = a->HW; x.C = a->C;
    x.flags = ((a->flags & SALT_LOVASZ_HAS_IGNORE) ? XF_VOID : 0) | (flat ? XF_GATHER : 0);
    if (flat) { r.B = a->C; r.P = (int)N; }                          // C rows of B HW elements gathered across the images
    return lovasz_launch_x<AbsError, XOpt>(&r, x, (a->flags & SALT_LOVASZ_ONLY_PRESENT) ? a->ws_present : nullptr, (hipStream_t)stream);
}

extern "C" int salt_dice_ce_parts(const salt_dice_ce_args* a) {
    if (!a || !shape_ok(a->B, a->C, a->HW)) return -1;
    return a->B * bce_ppp(a->HW, nullptr);
}

extern "C" int salt_dice_ce(const salt_dice_ce_args* a, void* stream) {
    if (!a || !a->logits || !a->target || !shape_ok(a->B, a->C, a->HW) || !a->partials || !a->sums || !a->loss)
        SALT_FAIL(SALT_E_BADARG, "dice_ce: needs logits, target, partials, sums, loss, B >= 1, HW >= 1 and 2 <= C <= 4");
    int per = 0;
    const int ppp = bce_ppp(a->HW, &per);
    if (a->nparts != a->B * ppp) SALT_FAIL(SALT_E_BADARG, "dice_ce: nparts %d, expected %d", a->nparts, a->B * ppp);
    hipStream_t st = (hipStream_t)stream;
    SALT_TRY(SALT_SOFTMAX_C(a->C, dice_ce_partial_kernel, dim3(a->nparts), dim3(256), 0, st, a->logits, a->target, a->HW, ppp, per, a->partials));
    SALT_TRY(salt_launch(dice_ce_finalize_kernel, dim3(1), dim3(64), 0, st, a->partials, a->nparts, a->B, a->C, a->HW, a->dice_weight,
                         a->cross_entropy_weight, a->smooth, a->loss_scale, a->sums, a->loss));
    if (a->dlogits) {
        const int64_t n = (int64_t)a->B * a->HW;
        SALT_TRY(SALT_SOFTMAX_C(a->C, dice_ce_grad_kernel, dim3(stream_blocks(n)), dim3(256), 0, st, a->logits, a->target, a->B, a->HW, a->sums,
                                a->dice_weight, a->cross_entropy_weight, a->smooth, a->loss_scale, a->dlogits));
    }
    return SALT_OK;
}
