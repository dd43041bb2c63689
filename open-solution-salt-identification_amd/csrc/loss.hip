// loss.hip — Lovasz hinge and BCE+Dice on the GPU.
//
// Lovasz hinge (lovasz_losses.py:81-115,21-33 via models.py:326-328): the reference loops over the B
// images in Python and issues ~10 small torch kernels per image (sort, gather, cumsum x2, ...).  Here
// ONE launch does the whole batch: one 1024-thread workgroup per image runs a stable LSD radix sort
// (4 x 8-bit digits) of the hinge errors with a (flat index, label) payload through a ping-pong
// workspace that stays L2-resident (P = 2*H*W = 32768 keys = 256 KB per image), then a single fused
// pass does the label scan, the Jaccard gradient g_k, the dot with elu(errors) and the scatter of
// d loss / d logit back to NCHW order.  Ties keep flat-index order (stable sort), so results are
// deterministic; the loss value itself is tie-order invariant.  The sort and the final pass live in loss_common.h as kernels
// templated on an error policy (HingeElu here; loss_softmax.hip instantiates AbsError for the Lovasz-softmax).
#include "loss_common.h"

namespace {

// ---------------------------------------------------------------- BCE + Dice
__global__ __launch_bounds__(256) void bce_dice_partial_kernel(const float* z, const float* t, int HW, int ppp, int per, float* partials) {
    __shared__ float sm4[4];
    const int plane = blockIdx.x / ppp, part = blockIdx.x % ppp;
    const int i0 = part * per, i1 = min(i0 + per, HW);
    float s_pt = 0.f, s_p = 0.f, s_t = 0.f, s_b = 0.f;
    for (int i = i0 + threadIdx.x; i < i1; i += 256) {
        const float zz = z[(int64_t)plane * HW + i], tt = t[(int64_t)plane * HW + i];
        const float p = 1.f / (1.f + expf(-zz));
        s_pt += p * tt; s_p += p; s_t += tt;
        s_b += fmaxf(zz, 0.f) - zz * tt + log1pf(expf(-fabsf(zz)));
    }
    const float r0 = block_sum_256(s_pt, sm4), r1 = block_sum_256(s_p, sm4), r2 = block_sum_256(s_t, sm4), r3 = block_sum_256(s_b, sm4);
    if (threadIdx.x == 0) { float* o = partials + (int64_t)blockIdx.x * 4; o[0] = r0; o[1] = r1; o[2] = r2; o[3] = r3; }
}

__global__ void bce_dice_finalize_kernel(const float* partials, int B, int C, int ppp, int HW, float dw, float bw, float scale, float* sums, float* loss) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double bce = 0.0, dice = 0.0;
    for (int c = 0; c < C; ++c) {
        double pt = 0.0, p = 0.0, t = 0.0;
        for (int b = 0; b < B; ++b)
            for (int k = 0; k < ppp; ++k) {
                const float* o = partials + ((int64_t)(b * C + c) * ppp + k) * 4;
                pt += o[0]; p += o[1]; t += o[2]; bce += o[3];
            }
        sums[c * 3 + 0] = (float)pt; sums[c * 3 + 1] = (float)p; sums[c * 3 + 2] = (float)t;
        dice += 1.0 - 2.0 * pt / (p + t + 1e-7);
    }
    sums[3 * C] = (float)bce;
    loss[0] = (float)((dw * dice / C + bw * bce / ((double)B * C * HW)) * scale);
}

__global__ void bce_dice_grad_kernel(const float* z, const float* t, int B, int C, int HW, const float* sums, float dw, float bw, float scale, float* dz) {
    const int64_t n = (int64_t)B * C * HW;
    for (int64_t i = blockIdx.x * 256LL + threadIdx.x; i < n; i += gridDim.x * 256LL) {
        const int c = (int)((i / HW) % C);
        const float pt = sums[c * 3], S = sums[c * 3 + 1] + sums[c * 3 + 2] + 1e-7f;
        const float zz = z[i], tt = t[i];
        const float p = 1.f / (1.f + expf(-zz));
        const float dD = -2.f * (tt * S - pt) / (S * S);
        dz[i] = scale * (dw / (float)C * dD * p * (1.f - p) + bw / (float)n * (p - tt));
    }
}

// ---------------------------------------------------------------- Adam (+L2), flat buffer
__global__ void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v, int64_t n,
                            const float* __restrict__ hyper) {
    const float lr = hyper[0], b1 = hyper[1], b2 = hyper[2], eps = hyper[3], wd = hyper[4], bc1 = hyper[5], bc2 = hyper[6], gs = hyper[7];
    const float step_size = lr / bc1, rs = 1.f / sqrtf(bc2);
    const int64_t n4 = n >> 2;
    for (int64_t i = blockIdx.x * 256LL + threadIdx.x; i < n4; i += gridDim.x * 256LL) {
        f32x4 pp = reinterpret_cast<const f32x4*>(p)[i], mm = reinterpret_cast<const f32x4*>(m)[i], vv = reinterpret_cast<const f32x4*>(v)[i];
        const f32x4 gg = reinterpret_cast<const f32x4*>(g)[i];
        adam4(pp, gg, mm, vv, b1, b2, eps, wd, gs, step_size, rs);             // (common.h: shared with adam_pack_kernel - same bits)
        reinterpret_cast<f32x4*>(p)[i] = pp; reinterpret_cast<f32x4*>(m)[i] = mm; reinterpret_cast<f32x4*>(v)[i] = vv;
    }
    for (int64_t i = (n4 << 2) + blockIdx.x * 256LL + threadIdx.x; i < n; i += gridDim.x * 256LL) {
        const float gr = g[i] * gs + wd * p[i];
        const float m1 = b1 * m[i] + (1.f - b1) * gr, v1 = b2 * v[i] + (1.f - b2) * gr * gr;
        m[i] = m1; v[i] = v1;
        p[i] -= step_size * m1 / (sqrtf(v1) * rs + eps);
    }
}

__global__ void adam_tick_kernel(float* hyper, int64_t* step) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        const int64_t t = step[0] + 1;
        step[0] = t;
        hyper[5] = (float)(1.0 - pow((double)hyper[1], (double)t));
        hyper[6] = (float)(1.0 - pow((double)hyper[2], (double)t));
    }
}

// ---------------------------------------------------------------- TTA: sigmoid -> inverse flip -> mean
struct TtaKP { const float* logits; float* prob; int V, B, C, H, W; int ud[16], lr[16], rq[16]; int method, act; };
__global__ void tta_mean_kernel(TtaKP p) {
    const int64_t hw = (int64_t)p.H * p.W, n = (int64_t)p.B * p.C * hw;
    for (int64_t i = blockIdx.x * 256LL + threadIdx.x; i < n; i += gridDim.x * 256LL) {
        const int x = (int)(i % p.W); int64_t r = i / p.W; const int y = (int)(r % p.H); const int64_t plane = r / p.H;
        float s = p.method == 1 ? -1.f : (p.method == 2 ? 2.f : 0.f);
        for (int v = 0; v < p.V; ++v) {
            // out = flipud?(fliplr?(rot90(pred, -k))): undo the flips on the output coordinate, then read through the rotation
            // (np.rot90(m, q)[i, j] for q = 1, 2, 3: m[j, n-1-i], m[n-1-i, n-1-j], m[n-1-j, i]; rq = (-k) mod 4, square maps)
            const int yf = p.ud[v] ? p.H - 1 - y : y, xf = p.lr[v] ? p.W - 1 - x : x;
            int yy = yf, xx = xf;
            const int q = p.rq[v];
            if (q == 1) { yy = xf; xx = p.W - 1 - yf; }
            else if (q == 2) { yy = p.H - 1 - yf; xx = p.W - 1 - xf; }
            else if (q == 3) { yy = p.H - 1 - xf; xx = yf; }
            const float zz = p.logits[((int64_t)v * p.B * p.C + plane) * hw + (int64_t)yy * p.W + xx];
            const float pr = p.act ? zz : 1.f / (1.f + expf(-zz));     // act 1: the input holds probabilities already
            if (p.method == 0) s += pr;
            else if (p.method == 1) s = fmaxf(s, pr);
            else if (p.method == 2) s = fminf(s, pr);
            else s += logf(pr);
        }
        p.prob[i] = p.method == 0 ? s / (float)p.V : (p.method == 3 ? expf(s / (float)p.V) : s);
    }
}
__global__ void flip_kernel(salt_flip_args a) {
    const int64_t hw = (int64_t)a.H * a.W, n = (int64_t)a.B * a.C * hw;
    for (int64_t i = blockIdx.x * 256LL + threadIdx.x; i < n; i += gridDim.x * 256LL) {
        const int x = (int)(i % a.W); int64_t r = i / a.W; const int y = (int)(r % a.H); const int64_t plane = r / a.H;
        const int yy = a.flip_ud ? a.H - 1 - y : y, xx = a.flip_lr ? a.W - 1 - x : x;
        a.y[i] = a.x[plane * hw + (int64_t)yy * a.W + xx];
    }
}

// ---------------------------------------------------------------- inference epilogue: crop + threshold, metric counts
__global__ void crop_threshold_kernel(salt_crop_threshold_args a) {
    const int64_t n = (int64_t)a.B * a.h * a.w;
    for (int64_t i = blockIdx.x * 256LL + threadIdx.x; i < n; i += gridDim.x * 256LL) {
        const int x = (int)(i % a.w); int64_t r = i / a.w; const int y = (int)(r % a.h); const int b = (int)(r / a.h);
        const float p = a.prob[(((int64_t)b * a.C + a.cls) * a.H + a.top + y) * a.W + a.left + x];
        a.mask[i] = p > a.threshold ? 1 : 0;
    }
}

struct IouKP { salt_iou_sweep_args a; double th[SALT_MAX_THRESHOLDS]; };
__global__ __launch_bounds__(256) void iou_sweep_kernel(IouKP k) {
    __shared__ int s_inter[SALT_MAX_THRESHOLDS], s_pred[SALT_MAX_THRESHOLDS], s_gt;
    const salt_iou_sweep_args& a = k.a;
    const int b = blockIdx.x, tid = threadIdx.x;
    if (tid < SALT_MAX_THRESHOLDS) { s_inter[tid] = 0; s_pred[tid] = 0; }
    if (tid == 0) s_gt = 0;
    __syncthreads();
    int ci[SALT_MAX_THRESHOLDS], cp[SALT_MAX_THRESHOLDS], cg = 0;
#pragma unroll
    for (int t = 0; t < SALT_MAX_THRESHOLDS; ++t) { ci[t] = 0; cp[t] = 0; }
    const int n = a.h * a.w;
    for (int i = tid; i < n; i += 256) {
        const int y = i / a.w, x = i - y * a.w;
        const double p = (double)a.prob[(((int64_t)b * a.C + a.cls) * a.H + a.top + y) * a.W + a.left + x];
        const int g = a.gt[(int64_t)b * n + i] ? 1 : 0;
        cg += g;
#pragma unroll
        for (int t = 0; t < SALT_MAX_THRESHOLDS; ++t) {
            const int pr = (t < a.T && p > k.th[t]) ? 1 : 0;
            cp[t] += pr; ci[t] += pr & g;
        }
    }
#pragma unroll
    for (int t = 0; t < SALT_MAX_THRESHOLDS; ++t) {
        if (t < a.T) {                                   // uniform
            int vi = ci[t], vp = cp[t];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) { vi += __shfl_xor(vi, o); vp += __shfl_xor(vp, o); }
            if ((tid & 63) == 0) { atomicAdd(&s_inter[t], vi); atomicAdd(&s_pred[t], vp); }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cg += __shfl_xor(cg, o);
    if ((tid & 63) == 0) atomicAdd(&s_gt, cg);
    __syncthreads();
    if (tid < a.T) { a.inter[b * a.T + tid] = s_inter[tid]; a.pred[b * a.T + tid] = s_pred[tid]; }
    if (tid == 0) a.gt_count[b] = s_gt;
}

}  // namespace

extern "C" int64_t salt_lovasz_split_words(int P) { return lovasz_split_words(P); }

extern "C" int64_t salt_lovasz_flat_words(int64_t N) { return lovasz_flat_words(N); }

extern "C" int salt_lovasz_hinge(const salt_lovasz_args* a, void* stream) {
    if (!a || !a->logits || !a->target || a->B < 1 || a->P < 0 || !a->ws_keys || !a->ws_vals || !a->loss_per_image || !a->loss)
        SALT_FAIL(SALT_E_BADARG, "lovasz: bad args");
    if (const char* why = lovasz_flags_refusal(a->flags, a->ignore, false)) SALT_FAIL(SALT_E_BADARG, "lovasz: %s (flags 0x%x)", why, a->flags);
    const bool has_void = a->flags & SALT_LOVASZ_HAS_IGNORE;
    const int64_t N = (a->flags & SALT_LOVASZ_BATCH_FLAT) ? (int64_t)a->B * a->P : a->P;
    if (N > (has_void ? LOVASZ_MAX_ROW_VOID : LOVASZ_MAX_ROW)) SALT_FAIL(SALT_E_BADARG, "lovasz: a row of %lld elements", (long long)N);
    salt_lovasz_args r = *a;
    if (a->flags & SALT_LOVASZ_BATCH_FLAT) { r.B = 1; r.P = (int)N; }        // the batch as it lies in memory is the one row
    if (!has_void) return lovasz_launch<HingeElu>(&r, (hipStream_t)stream);
    LovaszX x{};
    x.ignore = a->ignore; x.flags = XF_VOID;
    return lovasz_launch_x<HingeElu, XOpt>(&r, x, nullptr, (hipStream_t)stream);
}

extern "C" int salt_bce_dice_parts(const salt_bce_dice_args* a) {
    if (!a || a->B < 1 || a->C < 1 || a->HW < 1) return -1;
    return a->B * a->C * bce_ppp(a->HW, nullptr);
}

extern "C" int salt_bce_dice(const salt_bce_dice_args* a, void* stream) {
    if (!a || !a->logits || !a->target || a->B < 1 || a->C < 1 || a->HW < 1 || !a->partials || !a->sums || !a->loss) SALT_FAIL(SALT_E_BADARG, "bce_dice: bad args");
    int per = 0;
    const int ppp = bce_ppp(a->HW, &per);
    if (a->nparts != a->B * a->C * ppp) SALT_FAIL(SALT_E_BADARG, "bce_dice: nparts %d, expected %d", a->nparts, a->B * a->C * ppp);
    hipStream_t st = (hipStream_t)stream;
    SALT_TRY(salt_launch(bce_dice_partial_kernel, dim3(a->nparts), dim3(256), 0, st, a->logits, a->target, a->HW, ppp, per, a->partials));
    SALT_TRY(salt_launch(bce_dice_finalize_kernel, dim3(1), dim3(64), 0, st, a->partials, a->B, a->C, ppp, a->HW, a->dice_weight, a->bce_weight, a->loss_scale, a->sums, a->loss));
    if (a->dlogits) {
        const int64_t n = (int64_t)a->B * a->C * a->HW;
        const int blocks = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
        SALT_TRY(salt_launch(bce_dice_grad_kernel, dim3(blocks), dim3(256), 0, st, a->logits, a->target, a->B, a->C, a->HW, a->sums, a->dice_weight, a->bce_weight, a->loss_scale, a->dlogits));
    }
    return SALT_OK;
}

extern "C" int salt_adam(const salt_adam_args* a, void* stream) {
    if (!a || !a->param || !a->grad || !a->exp_avg || !a->exp_avg_sq || !a->hyper || a->n < 0) SALT_FAIL(SALT_E_BADARG, "adam: bad args");
    if (a->n == 0) return SALT_OK;
    if (!aligned16(a->param, a->grad, a->exp_avg, a->exp_avg_sq))
        SALT_FAIL(SALT_E_BADARG, "adam: buffers must be 16-byte aligned");
    const int64_t n4 = (a->n + 3) / 4;
    const int blocks = (int)((n4 + 255) / 256 < 4096 ? (n4 + 255) / 256 : 4096);
    return salt_launch(adam_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, a->param, a->grad, a->exp_avg, a->exp_avg_sq, a->n, a->hyper);
}

extern "C" int salt_adam_tick(const salt_adam_tick_args* a, void* stream) {
    if (!a || !a->hyper || !a->step) SALT_FAIL(SALT_E_BADARG, "adam_tick: bad args");
    return salt_launch(adam_tick_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, a->hyper, a->step);
}

extern "C" int salt_tta_mean(const salt_tta_mean_args* a, void* stream) {
    if (!a || !a->logits || !a->prob || a->V < 1 || a->V > 16 || !a->flip_ud || !a->flip_lr) SALT_FAIL(SALT_E_BADARG, "tta_mean: bad args");
    TtaKP p;
    p.logits = a->logits; p.prob = a->prob; p.V = a->V; p.B = a->B; p.C = a->C; p.H = a->H; p.W = a->W;
    if (a->method < 0 || a->method > 3) SALT_FAIL(SALT_E_BADARG, "tta_mean: method %d (0 mean, 1 max, 2 min, 3 gmean)", a->method);
    p.method = a->method;
    if (a->activation < 0 || a->activation > 1) SALT_FAIL(SALT_E_BADARG, "tta_mean: activation %d (0 sigmoid, 1 none)", a->activation);
    p.act = a->activation;
    for (int v = 0; v < a->V; ++v) {
        p.ud[v] = a->flip_ud[v]; p.lr[v] = a->flip_lr[v];
        const int k = a->rot ? ((a->rot[v] % 4) + 4) % 4 : 0;
        if (k && a->H != a->W) SALT_FAIL(SALT_E_BADARG, "tta_mean: rotated variants need square maps");
        p.rq[v] = (4 - k) % 4;
    }
    const int64_t n = (int64_t)a->B * a->C * a->H * a->W;
    const int blocks = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
    return salt_launch(tta_mean_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, p);
}

extern "C" int salt_flip(const salt_flip_args* a, void* stream) {
    if (!a || !a->x || !a->y) SALT_FAIL(SALT_E_BADARG, "flip: bad args");
    const int64_t n = (int64_t)a->B * a->C * a->H * a->W;
    const int blocks = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
    return salt_launch(flip_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, *a);
}

static bool crop_ok(int B, int C, int H, int W, int cls, int top, int left, int h, int w) {
    return B >= 1 && C >= 1 && cls >= 0 && cls < C && h >= 1 && w >= 1 && top >= 0 && left >= 0 && top + h <= H && left + w <= W;
}

extern "C" int salt_crop_threshold(const salt_crop_threshold_args* a, void* stream) {
    if (!a || !a->prob || !a->mask || !crop_ok(a->B, a->C, a->H, a->W, a->cls, a->top, a->left, a->h, a->w)) SALT_FAIL(SALT_E_BADARG, "crop_threshold: bad args");
    const int64_t n = (int64_t)a->B * a->h * a->w;
    const int blocks = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
    return salt_launch(crop_threshold_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, *a);
}

extern "C" int salt_iou_sweep(const salt_iou_sweep_args* a, void* stream) {
    if (!a || !a->prob || !a->gt || !a->thresholds || !a->inter || !a->pred || !a->gt_count || a->T < 1 || a->T > SALT_MAX_THRESHOLDS ||
        !crop_ok(a->B, a->C, a->H, a->W, a->cls, a->top, a->left, a->h, a->w)) SALT_FAIL(SALT_E_BADARG, "iou_sweep: bad args");
    IouKP k;
    k.a = *a;
    for (int t = 0; t < SALT_MAX_THRESHOLDS; ++t) k.th[t] = t < a->T ? a->thresholds[t] : 2.0;
    return salt_launch(iou_sweep_kernel, dim3(a->B), dim3(256), 0, (hipStream_t)stream, k);
}
