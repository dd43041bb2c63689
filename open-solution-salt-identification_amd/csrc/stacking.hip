// stacking.hip — the reference's second-level networks (architectures/misc.py:8-36: StackingFCN / StackingFCNWithDepth) are ONE
// Conv2dBnRelu(M, F, (3,3)) over the stacked out-of-fold probability maps plus a 1x1 logit head.  salt_stack_conv runs that
// convolution on the matrix cores straight from the fp32 NCHW batch [B,M,H,W] the stacking loader hands over:
//   loader     a workgroup stages the halo of its 16 x 8 output tile (rows y-2 .. y, columns x .. x+2, clamped to the IMAGE edges:
//              the clamp is the replication pad of base.py:26) from the M input planes into LDS as [pixel][Kp] in the compute dtype,
//              channels >= M zero.  The NCHW -> pixel-major transposition happens here and nowhere else; a plane row of the halo is
//              one 72-byte run.  The weights of all nine taps sit in LDS as [tap][F][Kp] (k contiguous: the MFMA A fragment is one
//              16-byte read), converted from the fp32 master weight - no packed copy to keep fresh.  Workgroups are persistent: the
//              weights are staged once per workgroup (per tile only where fp32 with M > 32 and F = 64 needs two channel chunks
//              to stay inside 160 KB).
//   contract   bf16 mfma_f32_16x16x32_bf16, fp32 mfma_f32_16x16x4f32; A = W^T (row = output channel), B = pixels (column = pixel of
//              a 16-pixel tile row), so a lane ends up with 4 consecutive channels of one pixel.
//   eval       (acc + bias) * scale + shift, ReLU, per-image channel gate, 1x1 head F -> K <= 4, fp32 NCHW logits.  Nothing else
//              is written.
//   train      raw y (NHWC, compute dtype), its per-tile BatchNorm partials (sum, M2 about the tile mean, count: the protocol of
//              salt_conv_first), and xs: the staged tile's own pixels as NHWC [B,H,W,Mpad] - the Q operand of the weight gradient.
// salt_stack_grad_unfold drops the padded input channels of the weight gradient ([F][Mpad][3][3] -> [F][M][3][3]).
#include "common.h"

namespace {

constexpr int TW = 16, TH = 8;                  // output tile: 16 pixels of a row x 8 rows (4 waves, 2 rows each)
constexpr int HX = TW + 2, HY = TH + 2, NHALO = HX * HY;

template <typename T> struct StackT;
template <> struct StackT<float> { static constexpr int KS = 16, PAD = 4; };       // k step of the loops, LDS row padding (elements)
template <> struct StackT<bf16_t> { static constexpr int KS = 32, PAD = 8; };

struct StackKP {
    const float* x; const float* w; const float* bias;
    void* y; void* xs; float* stats; float* stats_cnt;
    const float* scale; const float* shift; const float* gate; const float* head_w; const float* head_b; float* logits;
    int B, M, H, W, F, Kp, Mpad, MC, SIN, SWT, y_cs, xs_cs, relu, gate_cs, K, tiles_y, tiles_x, ntiles;
};

template <typename T>
__device__ __forceinline__ void stage_weights(const StackKP& p, T* s_w, int c0, int mc, int tid) {
    // global order (f, m, tap): coalesced reads of the fp32 master weight [F][M][3][3]; channels >= M are zero
    const int n = p.F * mc * 9;
    for (int i = tid; i < n; i += 256) {
        const int tap = i % 9; int r = i / 9; const int ml = r % mc; const int f = r / mc;
        const int m = c0 + ml;
        const float v = m < p.M ? p.w[((int64_t)f * p.M + m) * 9 + tap] : 0.f;
        Elem<T>::st(s_w + ((int64_t)tap * p.F + f) * p.SWT + ml, v);
    }
}

template <typename T, int NF, bool TRAIN>
__global__ __launch_bounds__(256) void stack_conv_kernel(StackKP p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sm_raw[];
    constexpr int KS = StackT<T>::KS;
    constexpr int F = NF * 16;
    T* s_in = reinterpret_cast<T*>(sm_raw);                                 // [NHALO][SIN]
    T* s_w = s_in + NHALO * p.SIN;                                          // [9][F][SWT]
    float* s_red = reinterpret_cast<float*>(s_w + 9 * F * p.SWT);           // [4][F]
    float* s_par = s_red + 4 * F;                                           // [2 + 4][F]: scale | shift' (train: - | bias) | head rows
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lp = lane & 15, lq = lane >> 4;
    const int nchunks = (p.Kp + p.MC - 1) / p.MC;

    for (int f = tid; f < F; f += 256) {
        const float b = p.bias ? p.bias[f] : 0.f;
        if (TRAIN) { s_par[f] = 1.f; s_par[F + f] = b; }
        else {
            const float sc = p.scale ? p.scale[f] : 1.f;
            s_par[f] = sc; s_par[F + f] = b * sc + (p.shift ? p.shift[f] : 0.f);
            for (int k = 0; k < 4; ++k) s_par[(2 + k) * F + f] = k < p.K ? p.head_w[k * F + f] : 0.f;
        }
    }
    if (nchunks == 1) stage_weights<T>(p, s_w, 0, p.Kp, tid);

    for (int tile = blockIdx.x; tile < p.ntiles; tile += gridDim.x) {
        int t = tile;
        const int txi = t % p.tiles_x; t /= p.tiles_x;
        const int tyi = t % p.tiles_y; const int b = t / p.tiles_y;
        const int y0 = tyi * TH, x0 = txi * TW;
        __syncthreads();                                                     // the previous tile's readers of s_in / s_w are done
        // ---- loader: halo of the tile from the M planes, clamped to the image (top / right clamp = the replication pad; the bottom
        //      clamp only keeps the reads of a ragged last tile inside the image, those rows feed masked outputs)
        {
            const int n = p.Kp * NHALO;
            const float* xb = p.x + (int64_t)b * p.M * p.H * p.W;
#pragma unroll 4
            for (int i = tid; i < n; i += 256) {
                const int hx = i % HX; int r = i / HX; const int hy = r % HY; const int m = r / HY;
                int iy = y0 - 2 + hy; iy = iy < 0 ? 0 : (iy > p.H - 1 ? p.H - 1 : iy);
                int ix = x0 + hx; ix = ix > p.W - 1 ? p.W - 1 : ix;
                const float v = m < p.M ? xb[((int64_t)m * p.H + iy) * p.W + ix] : 0.f;
                Elem<T>::st(s_in + (hy * HX + hx) * p.SIN + m, v);
            }
        }
        __syncthreads();
        if (TRAIN) {
            // xs: the tile's own pixels (halo rows 2.., columns 0..15), whole 16-byte pieces; every image pixel belongs to one tile
            constexpr int VE = Elem<T>::VE;
            const int ppp = p.Mpad / VE;
            for (int i = tid; i < TW * TH * ppp; i += 256) {
                const int pc = i % ppp; const int px = i / ppp; const int c = px % TW, r = px / TW;
                const int oy = y0 + r, ox = x0 + c;
                if (oy < p.H && ox < p.W) {
                    const u32x4 v = *reinterpret_cast<const u32x4*>(s_in + ((r + 2) * HX + c) * p.SIN + pc * VE);
                    *reinterpret_cast<u32x4*>(reinterpret_cast<T*>(p.xs) + (((int64_t)b * p.H + oy) * p.W + ox) * p.xs_cs + pc * VE) = v;
                }
            }
        }
        f32x4 acc[2][NF];
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int fb = 0; fb < NF; ++fb) acc[r][fb] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int c0 = 0; c0 < p.Kp; c0 += p.MC) {
            const int mc = p.Kp - c0 < p.MC ? p.Kp - c0 : p.MC;
            if (nchunks > 1) {
                if (c0 > 0) __syncthreads();
                stage_weights<T>(p, s_w, c0, mc, tid);
                __syncthreads();
            }
            for (int tap = 0; tap < 9; ++tap) {
                const int kh = tap / 3, kw = tap - 3 * kh;
                const T* bi0 = s_in + ((wave * 2 + kh) * HX + lp + kw) * p.SIN + c0;       // output row r reads halo row r + kh
                const T* bi1 = bi0 + HX * p.SIN;
                const T* wa = s_w + (tap * F + lp) * p.SWT;
                for (int kk = 0; kk < mc; kk += KS) {
                    if constexpr (sizeof(T) == 2) {
                        const bf16x8 b0 = *reinterpret_cast<const bf16x8*>(bi0 + kk + 8 * lq);
                        const bf16x8 b1 = *reinterpret_cast<const bf16x8*>(bi1 + kk + 8 * lq);
#pragma unroll
                        for (int fb = 0; fb < NF; ++fb) {
                            const bf16x8 a = *reinterpret_cast<const bf16x8*>(wa + fb * 16 * p.SWT + kk + 8 * lq);
                            acc[0][fb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b0, acc[0][fb], 0, 0, 0);
                            acc[1][fb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b1, acc[1][fb], 0, 0, 0);
                        }
                    } else {
#pragma unroll
                        for (int k4 = 0; k4 < KS; k4 += 4) {
                            const float b0 = bi0[kk + k4 + lq], b1 = bi1[kk + k4 + lq];
#pragma unroll
                            for (int fb = 0; fb < NF; ++fb) {
                                const float a = wa[fb * 16 * p.SWT + kk + k4 + lq];
                                acc[0][fb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b0, acc[0][fb], 0, 0, 0);
                                acc[1][fb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b1, acc[1][fb], 0, 0, 0);
                            }
                        }
                    }
                }
            }
        }
        // ---- epilogue: the lane holds channels fb 16 + 4 lq + j (j = 0..3) of pixel (y0 + 2 wave + r, x0 + lp)
        const int ox = x0 + lp;
        bool valid[2];
#pragma unroll
        for (int r = 0; r < 2; ++r) valid[r] = (y0 + wave * 2 + r) < p.H && ox < p.W;
        if constexpr (TRAIN) {
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const int oy = y0 + wave * 2 + r;
                T* yrow = reinterpret_cast<T*>(p.y) + (((int64_t)b * p.H + (valid[r] ? oy : 0)) * p.W + (valid[r] ? ox : 0)) * p.y_cs;
#pragma unroll
                for (int fb = 0; fb < NF; ++fb) {
                    const int f0 = fb * 16 + 4 * lq;
                    const f32x4 b4 = *reinterpret_cast<const f32x4*>(s_par + F + f0);
                    f32x4 v = acc[r][fb] + b4;
                    if constexpr (sizeof(T) == 2) {
                        const unsigned lo = f2bf_pk(v.x, v.y), hi = f2bf_pk(v.z, v.w);
                        if (valid[r]) *reinterpret_cast<uint2*>(yrow + f0) = make_uint2(lo, hi);
                        v.x = __uint_as_float(lo << 16); v.y = __uint_as_float(lo & 0xffff0000u);      // statistics of the STORED value
                        v.z = __uint_as_float(hi << 16); v.w = __uint_as_float(hi & 0xffff0000u);
                    } else {
                        if (valid[r]) *reinterpret_cast<f32x4*>(yrow + f0) = v;
                    }
                    acc[r][fb] = valid[r] ? v : f32x4{0.f, 0.f, 0.f, 0.f};
                }
            }
            const int vh = p.H - y0 < TH ? p.H - y0 : TH, vw = p.W - x0 < TW ? p.W - x0 : TW;
            const float cnt = (float)(vh * vw);
            float mean[NF][4];
            // pass 1: tile sums (lanes of a 16-group, then the wave's two rows, then the four waves in a fixed order)
#pragma unroll
            for (int fb = 0; fb < NF; ++fb)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float s = acc[0][fb][j] + acc[1][fb][j];
#pragma unroll
                    for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o);
                    if (lp == 0) s_red[wave * F + fb * 16 + 4 * lq + j] = s;
                }
            __syncthreads();
#pragma unroll
            for (int fb = 0; fb < NF; ++fb)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int f = fb * 16 + 4 * lq + j;
                    mean[fb][j] = (((s_red[f] + s_red[F + f]) + s_red[2 * F + f]) + s_red[3 * F + f]) / cnt;
                }
            if (tid < F) p.stats[((int64_t)tile * 2) * F + tid] = ((s_red[tid] + s_red[F + tid]) + s_red[2 * F + tid]) + s_red[3 * F + tid];
            __syncthreads();
            // pass 2: M2 about the tile mean
#pragma unroll
            for (int fb = 0; fb < NF; ++fb)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float d0 = valid[0] ? acc[0][fb][j] - mean[fb][j] : 0.f, d1 = valid[1] ? acc[1][fb][j] - mean[fb][j] : 0.f;
                    float s = d0 * d0 + d1 * d1;
#pragma unroll
                    for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o);
                    if (lp == 0) s_red[wave * F + fb * 16 + 4 * lq + j] = s;
                }
            __syncthreads();
            if (tid < F) p.stats[((int64_t)tile * 2 + 1) * F + tid] = ((s_red[tid] + s_red[F + tid]) + s_red[2 * F + tid]) + s_red[3 * F + tid];
            if (tid == 0) p.stats_cnt[tile] = cnt;
        } else {
            f32x4 g4[NF];
#pragma unroll
            for (int fb = 0; fb < NF; ++fb) {
                const int f0 = fb * 16 + 4 * lq;
                if (p.gate) {
                    const float* gp = p.gate + (int64_t)b * p.gate_cs + f0;
                    g4[fb] = f32x4{gp[0], gp[1], gp[2], gp[3]};
                } else g4[fb] = f32x4{1.f, 1.f, 1.f, 1.f};
            }
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                float lg[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int fb = 0; fb < NF; ++fb) {
                    const int f0 = fb * 16 + 4 * lq;
                    const f32x4 sc = *reinterpret_cast<const f32x4*>(s_par + f0);
                    const f32x4 sh = *reinterpret_cast<const f32x4*>(s_par + F + f0);
                    f32x4 v;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        float u = __fmaf_rn(acc[r][fb][j], sc[j], sh[j]);
                        if (p.relu) u = fmaxf(u, 0.f);
                        v[j] = u * g4[fb][j];
                    }
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const f32x4 hw = *reinterpret_cast<const f32x4*>(s_par + (2 + k) * F + f0);
#pragma unroll
                        for (int j = 0; j < 4; ++j) lg[k] = __fmaf_rn(v[j], hw[j], lg[k]);
                    }
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) { lg[k] += __shfl_xor(lg[k], 16); lg[k] += __shfl_xor(lg[k], 32); }
                if (lq == 0 && valid[r]) {
                    const int oy = y0 + wave * 2 + r;
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (k < p.K) p.logits[(((int64_t)b * p.K + k) * p.H + oy) * p.W + ox] = lg[k] + (p.head_b ? p.head_b[k] : 0.f);
                }
            }
        }
    }
}

__global__ void stack_grad_unfold_kernel(const float* gpad, int F, int M, int Mpad, float* grad, int accumulate) {
    const int total = F * M * 9;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
        const int r = i % (M * 9), f = i / (M * 9);
        const float v = gpad[(int64_t)f * Mpad * 9 + r];
        grad[i] = accumulate ? grad[i] + v : v;
    }
}

int stack_cus() {
    static int cus = 0;
    if (!cus) {
        hipDeviceProp_t pr; int dev = 0;
        if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&pr, dev) == hipSuccess) cus = pr.multiProcessorCount;
        if (cus < 8) cus = 256;
    }
    return cus;
}

// shape rules shared by the launch and the partial count: 0 = fine (message set otherwise)
int stack_shape_check(const salt_stack_conv_args* a) {
    if (!a) SALT_FAIL(SALT_E_BADARG, "stack_conv: null args");
    if (a->M < 1 || a->M > 64) SALT_FAIL(SALT_E_UNSUPPORTED, "stack_conv: %d input maps (supported: 1 .. 64)", a->M);
    if (a->F != 16 && a->F != 32 && a->F != 64) SALT_FAIL(SALT_E_UNSUPPORTED, "stack_conv: %d filters (supported: 16, 32, 64)", a->F);
    if (a->B < 1 || a->H < 1 || a->W < 1) SALT_FAIL(SALT_E_BADARG, "stack_conv: empty batch %d x %d x %d", a->B, a->H, a->W);
    if ((int64_t)a->B * cdiv(a->H, TH) * cdiv(a->W, TW) >= (1ll << 31)) SALT_FAIL(SALT_E_UNSUPPORTED, "stack_conv: too many tiles");
    return SALT_OK;
}

template <typename T>
int stack_launch(const salt_stack_conv_args* a, StackKP p, hipStream_t st) {
    constexpr int KS = StackT<T>::KS, PAD = StackT<T>::PAD;
    const size_t es = sizeof(T);
    const bool train = a->y.p != nullptr;
    p.Kp = (a->M + KS - 1) / KS * KS;
    p.Mpad = (a->M + 15) / 16 * 16;
    p.SIN = p.Kp + PAD;
    const size_t fixed = (size_t)NHALO * p.SIN * es + (size_t)(4 + 6) * a->F * sizeof(float);
    // the largest channel chunk (a multiple of the k step) whose nine taps fit beside the halo
    p.MC = 0;
    for (int mc = p.Kp; mc >= KS; mc -= KS)
        if (fixed + (size_t)9 * a->F * (mc + PAD) * es <= 160 * 1024) { p.MC = mc; break; }
    if (!p.MC) SALT_FAIL(SALT_E_LDS, "stack_conv: halo + one weight chunk exceed 160 KB of LDS");
    p.SWT = p.MC + PAD;
    const size_t lds = fixed + (size_t)9 * a->F * p.SWT * es;
    if (lds > 160 * 1024) SALT_FAIL(SALT_E_LDS, "stack_conv: needs %zu bytes of LDS", lds);
    if (train) {
        SALT_TRY(view_check16("stack_conv", "y", a->y, a->dtype, a->B, a->H, a->W, a->F));
        SALT_TRY(view_check16("stack_conv", "xs", a->xs, a->dtype, a->B, a->H, a->W, p.Mpad));
        if (!a->stats || !a->stats_cnt) SALT_FAIL(SALT_E_BADARG, "stack_conv: the train form needs the stats workspaces");
        p.y_cs = a->y.cs; p.xs_cs = a->xs.cs;
    }
    int wgs = (int)((160 * 1024) / lds);
    wgs = wgs < 1 ? 1 : (wgs > 4 ? 4 : wgs);
    const int64_t cap = (int64_t)stack_cus() * wgs;
    const dim3 grid((unsigned)(p.ntiles < cap ? p.ntiles : cap));
#define SALT_STACK_GO(NF) (train ? salt_launch(stack_conv_kernel<T, NF, true>, grid, dim3(256), lds, st, p) \
                                 : salt_launch(stack_conv_kernel<T, NF, false>, grid, dim3(256), lds, st, p))
    return a->F == 16 ? SALT_STACK_GO(1) : a->F == 32 ? SALT_STACK_GO(2) : SALT_STACK_GO(4);
#undef SALT_STACK_GO
}

}  // namespace

extern "C" int salt_stack_conv_stats_parts(const salt_stack_conv_args* a) {
    const int rc = stack_shape_check(a);
    if (rc) return rc;
    return a->B * cdiv(a->H, TH) * cdiv(a->W, TW);
}

extern "C" int salt_stack_conv(const salt_stack_conv_args* a, void* stream) {
    const int rc = stack_shape_check(a);
    if (rc) return rc;
    if (!a->x || !a->w) SALT_FAIL(SALT_E_BADARG, "stack_conv: x / w");
    const bool train = a->y.p != nullptr, eval = a->logits_nchw != nullptr;
    if (train == eval) SALT_FAIL(SALT_E_BADARG, "stack_conv: exactly one of y (train form) and logits_nchw (eval form)");
    if (eval) {
        if (a->K < 1 || a->K > 4) SALT_FAIL(SALT_E_UNSUPPORTED, "stack_conv: head with %d classes (supported: 1 .. 4)", a->K);
        if (!a->head_w) SALT_FAIL(SALT_E_BADARG, "stack_conv: the eval form needs the head weight");
        if ((a->scale == nullptr) != (a->shift == nullptr)) SALT_FAIL(SALT_E_BADARG, "stack_conv: scale/shift");
        if (a->gate && a->gate_cs < a->F) SALT_FAIL(SALT_E_BADARG, "stack_conv: gate rows of %d < %d channels", a->gate_cs, a->F);
    }
    StackKP p;
    p.x = a->x; p.w = a->w; p.bias = a->bias; p.y = a->y.p; p.xs = a->xs.p; p.stats = a->stats; p.stats_cnt = a->stats_cnt;
    p.scale = a->scale; p.shift = a->shift; p.gate = a->gate; p.head_w = a->head_w; p.head_b = a->head_b; p.logits = a->logits_nchw;
    p.B = a->B; p.M = a->M; p.H = a->H; p.W = a->W; p.F = a->F; p.y_cs = 0; p.xs_cs = 0; p.relu = a->relu; p.gate_cs = a->gate_cs; p.K = a->K;
    p.tiles_y = cdiv(a->H, TH); p.tiles_x = cdiv(a->W, TW); p.ntiles = a->B * p.tiles_y * p.tiles_x;
    SALT_DISPATCH_DTYPE(a->dtype, T, return stack_launch<T>(a, p, (hipStream_t)stream))
}

extern "C" int salt_stack_grad_unfold(const salt_stack_grad_unfold_args* a, void* stream) {
    if (!a || !a->gpad || !a->grad || a->F < 1 || a->M < 1 || a->Mpad < a->M) SALT_FAIL(SALT_E_BADARG, "stack_grad_unfold: bad args");
    const int total = a->F * a->M * 9;
    return salt_launch(stack_grad_unfold_kernel, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream, a->gpad, a->F, a->M, a->Mpad, a->grad, a->accumulate);
}
