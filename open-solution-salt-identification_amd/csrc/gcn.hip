// gcn.hip — the entry of a GlobalConvolutionalNetwork block (saltnet.h: salt_gcn_pair, salt_gcn_pair_dgrad): the K x 1 and the 1 x K
// convolution that read the same wide encoder map, from ONE staged tile of it, and the gradient of that map from both branches in ONE
// launch that stores it once.  The reference pads one-sided by replication (K - 1 rows on top, K - 1 columns on the right): the loader
// clamps the source index, so there is no padded copy going in and no fold ring coming back.
// Weights come from the fp32 masters [Cout][Cin][K] (no packed copy, nothing to refresh); bf16 rounds them on the way into LDS.
//   GEMMs          forward  Dv[n][p] = sum_k sum_c Wv[n][c][k] x[p + (k - (K-1)) rows][c]     A rows = output channels (padded to 32 with
//                           Dh[n][p] = sum_k sum_c Wh[n][c][k] x[p + k columns][c]            zero rows), B columns = pixels, K-dim = channels
//                  dgrad    D[c][p]  = sum_taps sum_n W[n][c][k] dy[p'][n]                     A = W transposed while staged, K-dim = Cout
//                                                                                              (padded to 32 with zero columns)
//   tile           GCN_TH x GCN_TW = 8 x 16 pixels per 256-thread workgroup; a wave owns two tile rows (32 pixels).  Forward: two
//                  32 x 32 accumulators per wave (one per branch), channels move in chunks of 32.  Data gradient: 32 input channels per
//                  workgroup, one accumulator per wave, the two branches run one after the other through the same LDS.
//   staged x       L-shaped: rows i0 - (K-1) .. i0 + 7 of the tile's 16 columns (the K x 1 taps; the 1 x K taps of a pixel that stay inside
//                  the tile's columns read its last 8 rows), then the K - 1 columns right of the tile for the tile's 8 rows.  No corner.
//                  At K = 9: 320 pixel rows + 2 x 9 x 32 weight rows of 80 bytes (bf16) = 72 KB, two workgroups per CU.
//   operands       LDS rows are [row][32 k] of the storage type padded to 80 (bf16) / 144 (f32) bytes, the layout of dense.hip.  bf16:
//                  v_mfma_f32_32x32x16_bf16.  f32: the exact v_mfma_f32_32x32x2_f32, as salt_conv does.
//   sums           the forward statistics are reduced over the tile in a fixed order (lane butterflies, then the four waves ascending)
//                  and leave as one partial per tile: no atomics, the same bits every run.
//   dgrad order    PINNED: the K regular K x 1 taps (k ascending), for a tile that holds image row 0 the clamp taps of that row (k
//                  ascending, then the source row descending), then the K regular 1 x K taps, for a tile that holds image column W - 1
//                  the clamp taps of that column (k ascending, then the source column ascending); inside a tap the matrix core's own
//                  order over the 32 output channels.  The clamp taps use the ORIGINAL weights, one tap per (k, source) pair, so every
//                  operand is the stored value: no prefix-summed weight is ever rounded to bf16.
#include "common.h"

namespace {

constexpr int GCN_TH = 8, GCN_TW = 16;      // pixel tile
constexpr int KC = 32;                      // contraction chunk = LDS row width
constexpr int GCN_MAX_K = 9, GCN_MAX_COUT = 32, GCN_MAX_CIN = 2048;

template <typename T> struct Lds {
    static constexpr int RS = sizeof(T) == 2 ? 40 : 36;           // row stride in elements: 80 / 144 bytes, 16-byte aligned
    static constexpr int NS = sizeof(T) == 2 ? 2 : 4;             // Mma steps per 32-wide row
};
// the 16-byte fragment of lane half h for step s of row `row`
template <typename T>
__device__ __forceinline__ u32x4 frag(const T* tile, int row, int s, int h) {
    const int piece = sizeof(T) == 2 ? 2 * s + h : 4 * h + s;
    return *reinterpret_cast<const u32x4*>(tile + row * Lds<T>::RS + piece * Elem<T>::VE);
}
__device__ __forceinline__ void zero_acc(f32x16& a) {
#pragma unroll
    for (int i = 0; i < 16; ++i) a[i] = 0.f;
}
template <typename T> __device__ __forceinline__ f32x4 load4(const T* p);
template <> __device__ __forceinline__ f32x4 load4<float>(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
template <> __device__ __forceinline__ f32x4 load4<bf16_t>(const bf16_t* p) {
    const uint2 v = *reinterpret_cast<const uint2*>(p);
    return f32x4{__uint_as_float(v.x << 16), __uint_as_float(v.x & 0xffff0000u), __uint_as_float(v.y << 16), __uint_as_float(v.y & 0xffff0000u)};
}
template <typename T> __device__ __forceinline__ void store4(T* p, f32x4 v);
template <> __device__ __forceinline__ void store4<float>(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }
template <> __device__ __forceinline__ void store4<bf16_t>(bf16_t* p, f32x4 v) {
    *reinterpret_cast<uint2*>(p) = make_uint2(f2bf_pk(v.x, v.y), f2bf_pk(v.z, v.w));
}
// the value a store of v leaves in memory
template <typename T> __device__ __forceinline__ float stored(float v);
template <> __device__ __forceinline__ float stored<float>(float v) { return v; }
template <> __device__ __forceinline__ float stored<bf16_t>(float v) { return bf2f(f2bf(v)); }

// Sum of v over the 32 lanes of a half-wave (one pixel each), same result in all of them; fixed order
__device__ __forceinline__ float half_sum(float v) {
#pragma unroll
    for (int o = 1; o < 32; o <<= 1) v += __shfl_xor(v, o);
    return v;
}
// Per-channel sums of a 128-pixel x 32-channel tile held as v[4 g + e] = channel 8 g + 4 h + e of the lane's pixel
__device__ __forceinline__ void tile_sums_to_lds(const f32x16& v, float* s_red, int r, int h, int wave) {
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const float s = half_sum(v[q]);
        if (r == 0) s_red[wave * 32 + 8 * (q >> 2) + 4 * h + (q & 3)] = s;
    }
}
__device__ __forceinline__ float waves_sum(const float* s_red, int t) { return ((s_red[t] + s_red[32 + t]) + s_red[64 + t]) + s_red[96 + t]; }

// ---------------------------------------------------------------- forward
struct PairKP {
    const void* x; void* y[2]; const float* w[2];
    const float* bias[2]; const float* scale[2]; const float* shift[2]; float* stats[2]; float* cnt[2];
    int relu[2], y_cs[2];
    int B, H, W, Cin, Cout, K, x_cs, tiles_y, tiles_x;
};
inline size_t pair_lds_bytes(int K, size_t es) {
    const int rs = es == 2 ? 40 : 36, nx = (GCN_TH + K - 1) * GCN_TW + GCN_TH * (K - 1);
    return (size_t)(nx + 2 * K * 32) * rs * es + (4 * 32 + 32) * sizeof(float);
}

template <typename T>
__global__ __launch_bounds__(256) void gcn_pair_kernel(PairKP p) {
    constexpr int VE = Elem<T>::VE, RS = Lds<T>::RS, NS = Lds<T>::NS, PPR = KC / VE;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int K = p.K, K1 = K - 1;
    const int nv = (GCN_TH + K1) * GCN_TW, nx = nv + GCN_TH * K1;
    T* s_x = reinterpret_cast<T*>(smem);                          // [nx][RS]: the L-shaped region
    T* s_w = s_x + nx * RS;                                       // [2][K][32][RS]: Wv then Wh, rows = output channels
    float* s_red = reinterpret_cast<float*>(s_w + 2 * K * 32 * RS);   // [4][32]
    float* s_mean = s_red + 128;                                  // [32]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    const int tj = blockIdx.x % p.tiles_x, ti = (blockIdx.x / p.tiles_x) % p.tiles_y, b = blockIdx.x / (p.tiles_x * p.tiles_y);
    const int i0 = ti * GCN_TH, j0 = tj * GCN_TW;
    const T* x = reinterpret_cast<const T*>(p.x);
    // rows Cout .. 31 of every weight block stay zero for the whole kernel (the loop's first barrier orders this before the fill)
    for (int i = tid; i < 2 * K * 32 * RS * (int)sizeof(T) / 16; i += 256) reinterpret_cast<u32x4*>(s_w)[i] = u32x4{0u, 0u, 0u, 0u};
    f32x16 acc[2];
    zero_acc(acc[0]); zero_acc(acc[1]);
    const int pix = wave * 32 + r, tr = pix / GCN_TW, tc = pix % GCN_TW;
    for (int k0 = 0; k0 < p.Cin; k0 += KC) {
        __syncthreads();                                           // the previous chunk's fragment reads
        for (int i = tid; i < nx * PPR; i += 256) {
            const int pc = i % PPR, px = i / PPR;
            int gi, gj;
            if (px < nv) { gi = i0 - K1 + px / GCN_TW; gj = j0 + px % GCN_TW; }
            else { const int q = px - nv; gi = i0 + q / K1; gj = j0 + GCN_TW + q % K1; }
            gi = gi < 0 ? 0 : (gi < p.H ? gi : p.H - 1);           // the replicated rows on top (and the tile's overhang: never stored)
            gj = gj < p.W ? gj : p.W - 1;                          // the replicated columns on the right
            u32x4 v = u32x4{0u, 0u, 0u, 0u};
            if (k0 + pc * VE < p.Cin) v = *reinterpret_cast<const u32x4*>(x + ((int64_t)(b * p.H + gi) * p.W + gj) * p.x_cs + k0 + pc * VE);
            *reinterpret_cast<u32x4*>(s_x + px * RS + pc * VE) = v;
        }
        // a thread owns one (output channel, input channel) pair of a branch: its K taps are contiguous in the master
        for (int br = 0; br < 2; ++br)
            for (int i = tid; i < p.Cout * KC; i += 256) {
                const int n = i >> 5, c = i & 31;
                const bool ok = k0 + c < p.Cin;
                const float* src = p.w[br] + ((int64_t)n * p.Cin + k0 + c) * K;
                T* dst = s_w + (br * K * 32 + n) * RS + c;
                for (int k = 0; k < K; ++k) Elem<T>::st(dst + k * 32 * RS, ok ? src[k] : 0.f);
            }
        __syncthreads();
        for (int k = 0; k < K; ++k) {
            const int rv = (tr + k) * GCN_TW + tc, cj = tc + k;
            const int rh = cj < GCN_TW ? (tr + K1) * GCN_TW + cj : nv + tr * K1 + cj - GCN_TW;
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                Mma<T>::step(frag<T>(s_w, k * 32 + r, s, h), frag<T>(s_x, rv, s, h), acc[0]);
                Mma<T>::step(frag<T>(s_w, (K + k) * 32 + r, s, h), frag<T>(s_x, rh, s, h), acc[1]);
            }
        }
    }
    // ---- epilogue: the lane holds pixel (i0 + tr, j0 + tc), output channels 8 g + 4 h .. + 3 of both branches
    const int gi = i0 + tr, gj = j0 + tc;
    const bool valid = gi < p.H && gj < p.W;
    const int64_t m = (int64_t)(b * p.H + gi) * p.W + gj;
#pragma unroll
    for (int br = 0; br < 2; ++br) {
        T* y = reinterpret_cast<T*>(p.y[br]);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int ch = 8 * g + 4 * h;
            f32x4 v;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int n = ch + e;
                float t = acc[br][4 * g + e];
                if (n < p.Cout) {
                    if (p.bias[br]) t += p.bias[br][n];
                    if (p.scale[br]) t = t * p.scale[br][n] + p.shift[br][n];
                    if (p.relu[br]) t = fmaxf(t, 0.f);
                }
                v[e] = (valid && n < p.Cout) ? t : 0.f;
            }
            if (valid && ch + 4 <= p.Cout) store4<T>(y + m * p.y_cs[br] + ch, v);
            else if (valid) {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (ch + e < p.Cout) Elem<T>::st(y + m * p.y_cs[br] + ch + e, v[e]);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[br][4 * g + e] = stored<T>(v[e]);          // statistics of the STORED value
        }
    }
    if (!p.stats[0]) return;
    const int th = p.H - i0 < GCN_TH ? p.H - i0 : GCN_TH, tw = p.W - j0 < GCN_TW ? p.W - j0 : GCN_TW;
    const float cnt = (float)(th * tw);
    for (int br = 0; br < 2; ++br) {
        __syncthreads();
        tile_sums_to_lds(acc[br], s_red, r, h, wave);
        __syncthreads();
        if (tid < 32) {
            const float tot = waves_sum(s_red, tid);
            s_mean[tid] = tot / cnt;
            if (tid < p.Cout) p.stats[br][((int64_t)blockIdx.x * 2) * p.Cout + tid] = tot;
        }
        __syncthreads();
        f32x16 d2;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const float d = valid ? acc[br][q] - s_mean[8 * (q >> 2) + 4 * h + (q & 3)] : 0.f;
            d2[q] = d * d;
        }
        tile_sums_to_lds(d2, s_red, r, h, wave);
        __syncthreads();
        if (tid < p.Cout) p.stats[br][((int64_t)blockIdx.x * 2 + 1) * p.Cout + tid] = waves_sum(s_red, tid);
        if (tid == 0) p.cnt[br][blockIdx.x] = cnt;
    }
}

// ---------------------------------------------------------------- data gradient
struct PairDgKP {
    const void* dy[2]; const float* w[2]; void* dx;
    int dy_cs[2], dy_vec[2];
    int B, H, W, Cin, Cout, K, dx_cs, accumulate, tiles_y, tiles_x, c_tiles;
};
inline int dgrad_zero_row(int K) {
    const int nvr = (GCN_TH + K - 1) * GCN_TW, nhr = GCN_TH * (GCN_TW + K - 1);
    return nvr > nhr ? nvr : nhr;
}
inline size_t dgrad_lds_bytes(int K, size_t es) { return (size_t)(dgrad_zero_row(K) + 1 + K * 32) * (es == 2 ? 40 : 36) * es; }

template <typename T>
__global__ __launch_bounds__(256) void gcn_pair_dgrad_kernel(PairDgKP p) {
    constexpr int VE = Elem<T>::VE, RS = Lds<T>::RS, NS = Lds<T>::NS, PPR = KC / VE;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int K = p.K, K1 = K - 1, HW = GCN_TW + K1;
    const int nvr = (GCN_TH + K1) * GCN_TW, nhr = GCN_TH * HW, zrow = nvr > nhr ? nvr : nhr;
    T* s_dy = reinterpret_cast<T*>(smem);                         // [zrow + 1][RS]: the branch's gradient region, then one row of zeros
    T* s_w = s_dy + (zrow + 1) * RS;                              // [K][32 c][RS over n]: the branch's weight, transposed
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    int bid = blockIdx.x;
    const int ct = bid % p.c_tiles; bid /= p.c_tiles;
    const int tj = bid % p.tiles_x, ti = (bid / p.tiles_x) % p.tiles_y, b = bid / (p.tiles_x * p.tiles_y);
    const int i0 = ti * GCN_TH, j0 = tj * GCN_TW, c0 = ct * 32;
    const int pix = wave * 32 + r, tr = pix / GCN_TW, tc = pix % GCN_TW, gi = i0 + tr, gj = j0 + tc;
    f32x16 acc;
    zero_acc(acc);
    for (int ph = 0; ph < 2; ++ph) {                               // 0: the K x 1 branch, 1: the 1 x K branch
        const T* dy = reinterpret_cast<const T*>(p.dy[ph]);
        const int rows = ph ? nhr : nvr, cs = p.dy_cs[ph];
        const bool vec = p.dy_vec[ph] != 0;
        __syncthreads();                                           // the previous branch's fragment reads
        for (int i = tid; i < (zrow + 1) * PPR; i += 256) {
            const int pc = i % PPR, px = i / PPR;
            u32x4 v = u32x4{0u, 0u, 0u, 0u};
            if (px < rows && pc * VE < p.Cout) {
                // K x 1: image rows i0 .. i0 + 7 + (K-1) of the tile's columns;  1 x K: the tile's rows, image columns j0 - (K-1) .. j0 + 15
                const int si = i0 + (ph ? px / HW : px / GCN_TW), sj = ph ? j0 - K1 + px % HW : j0 + px % GCN_TW;
                if (si < p.H && sj >= 0 && sj < p.W)
                    v = load_piece<T>(dy, ((int64_t)(b * p.H + si) * p.W + sj) * cs + pc * VE, pc * VE, p.Cout, vec);
            }
            *reinterpret_cast<u32x4*>(s_dy + px * RS + pc * VE) = v;
        }
        for (int i = tid; i < 32 * KC; i += 256) {                  // one (output channel, input channel) pair per thread, K contiguous taps
            const int n = i >> 5, c = i & 31;
            const bool ok = n < p.Cout && c0 + c < p.Cin;
            const float* src = p.w[ph] + ((int64_t)n * p.Cin + c0 + c) * K;
            for (int k = 0; k < K; ++k) Elem<T>::st(s_w + (k * 32 + c) * RS + n, ok ? src[k] : 0.f);
        }
        __syncthreads();
        for (int k = 0; k < K; ++k) {
            const int row = ph ? tr * HW + tc + K1 - k : (tr + K1 - k) * GCN_TW + tc;
#pragma unroll
            for (int s = 0; s < NS; ++s) Mma<T>::step(frag<T>(s_w, k * 32 + r, s, h), frag<T>(s_dy, row, s, h), acc);
        }
        // the adjoint of the clamp: image row 0 also received the taps that reached above it, image column W - 1 those that reached past
        // it.  A lane whose pixel is not on that edge reads the row of zeros.
        if (ph == 0 ? i0 == 0 : j0 + GCN_TW >= p.W) {
            const bool on = ph ? gj == p.W - 1 : gi == 0;
            for (int k = 0; k < K; ++k)
                for (int e = 1; e <= (ph ? k : K1 - k); ++e) {
                    const int row = !on ? zrow : (ph ? tr * HW + tc + K1 - k + e : (K1 - k - e) * GCN_TW + tc);
#pragma unroll
                    for (int s = 0; s < NS; ++s) Mma<T>::step(frag<T>(s_w, k * 32 + r, s, h), frag<T>(s_dy, row, s, h), acc);
                }
        }
    }
    // ---- epilogue: the lane holds pixel (gi, gj), input channels c0 + 8 g + 4 h .. + 3
    if (gi >= p.H || gj >= p.W) return;
    T* dx = reinterpret_cast<T*>(p.dx) + ((int64_t)(b * p.H + gi) * p.W + gj) * p.dx_cs;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int ch = c0 + 8 * g + 4 * h;
        if (ch >= p.Cin) continue;
        f32x4 v = f32x4{acc[4 * g], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]};
        if (p.accumulate) v += load4<T>(dx + ch);
        store4<T>(dx + ch, v);
    }
}

// ---------------------------------------------------------------- host
int pair_shape_check(const char* op, int dtype, const salt_view& x, const salt_view& yv, const salt_view& yh, int K) {
    if (dtype != SALT_F32 && dtype != SALT_BF16) SALT_FAIL(SALT_E_UNSUPPORTED, "%s: bad dtype %d", op, dtype);
    const int ve = dtype == SALT_F32 ? 4 : 8;
    if (K < 2 || K > GCN_MAX_K) SALT_FAIL(SALT_E_UNSUPPORTED, "%s: kernel size %d (supported: 2 .. %d)", op, K, GCN_MAX_K);
    if (x.C < 8 || x.C > GCN_MAX_CIN || x.C % 8) SALT_FAIL(SALT_E_UNSUPPORTED, "%s: %d input channels (supported: multiples of 8 up to %d)", op, x.C, GCN_MAX_CIN);
    if (yv.C < 1 || yv.C > GCN_MAX_COUT || yh.C != yv.C)
        SALT_FAIL(SALT_E_UNSUPPORTED, "%s: %d / %d output channels (supported: 1 .. %d, the same for both branches)", op, yv.C, yh.C, GCN_MAX_COUT);
    if (x.B < 1 || x.H < 1 || x.W < 1) SALT_FAIL(SALT_E_UNSUPPORTED, "%s: empty batch %d x %d x %d", op, x.B, x.H, x.W);
    const salt_view* vs[3] = {&x, &yv, &yh};
    const char* names[3] = {"x", "yv", "yh"};
    for (int i = 0; i < 3; ++i) {
        const salt_view& v = *vs[i];
        if (!v.p || v.B != x.B || v.H != x.H || v.W != x.W || v.cs < v.C || v.cs % ve || !aligned16(v.p))
            SALT_FAIL(SALT_E_UNSUPPORTED, "%s: %s must be a 16-byte aligned [%d,%d,%d,C] view with cs >= C a multiple of %d", op, names[i], x.B, x.H, x.W, ve);
        if (view_pixels(v) * v.cs >= (1ll << 31)) SALT_FAIL(SALT_E_UNSUPPORTED, "%s: %s holds 2^31 elements or more", op, names[i]);
    }
    if ((int64_t)x.B * cdiv(x.H, GCN_TH) * cdiv(x.W, GCN_TW) * cdiv(x.C, 32) >= (1ll << 31)) SALT_FAIL(SALT_E_UNSUPPORTED, "%s: too many tiles", op);
    return SALT_OK;
}
inline int pair_tiles(const salt_view& x) { return x.B * cdiv(x.H, GCN_TH) * cdiv(x.W, GCN_TW); }

}  // namespace

extern "C" int salt_gcn_pair_stats_parts(const salt_gcn_pair_args* a) {
    if (!a) SALT_FAIL(SALT_E_BADARG, "gcn_pair: null args");
    const int rc = pair_shape_check("gcn_pair", a->dtype, a->x, a->yv, a->yh, a->K);
    if (rc) return rc;
    return pair_tiles(a->x);
}

extern "C" int salt_gcn_pair(const salt_gcn_pair_args* a, void* stream) {
    if (!a) SALT_FAIL(SALT_E_BADARG, "gcn_pair: null args");
    SALT_TRY(pair_shape_check("gcn_pair", a->dtype, a->x, a->yv, a->yh, a->K));
    if (!a->wv || !a->wh) SALT_FAIL(SALT_E_BADARG, "gcn_pair: wv / wh");
    if ((a->scale_v == nullptr) != (a->shift_v == nullptr) || (a->scale_h == nullptr) != (a->shift_h == nullptr))
        SALT_FAIL(SALT_E_BADARG, "gcn_pair: scale / shift go together");
    const bool train = a->stats_v || a->stats_h || a->stats_cnt_v || a->stats_cnt_h;
    if (train && !(a->stats_v && a->stats_h && a->stats_cnt_v && a->stats_cnt_h))
        SALT_FAIL(SALT_E_BADARG, "gcn_pair: the train form needs stats and stats_cnt of both branches");
    if (train && (a->scale_v || a->scale_h || a->relu_v || a->relu_h))
        SALT_FAIL(SALT_E_BADARG, "gcn_pair: the train form stores the raw outputs (no scale / shift / relu)");
    PairKP p;
    p.x = a->x.p; p.y[0] = a->yv.p; p.y[1] = a->yh.p; p.w[0] = a->wv; p.w[1] = a->wh;
    p.bias[0] = a->bias_v; p.bias[1] = a->bias_h; p.scale[0] = a->scale_v; p.scale[1] = a->scale_h; p.shift[0] = a->shift_v; p.shift[1] = a->shift_h;
    p.stats[0] = a->stats_v; p.stats[1] = a->stats_h; p.cnt[0] = a->stats_cnt_v; p.cnt[1] = a->stats_cnt_h;
    p.relu[0] = a->relu_v ? 1 : 0; p.relu[1] = a->relu_h ? 1 : 0; p.y_cs[0] = a->yv.cs; p.y_cs[1] = a->yh.cs;
    p.B = a->x.B; p.H = a->x.H; p.W = a->x.W; p.Cin = a->x.C; p.Cout = a->yv.C; p.K = a->K; p.x_cs = a->x.cs;
    p.tiles_y = cdiv(p.H, GCN_TH); p.tiles_x = cdiv(p.W, GCN_TW);
    const dim3 grid((unsigned)pair_tiles(a->x));
    SALT_DISPATCH_DTYPE(a->dtype, T, return salt_launch(gcn_pair_kernel<T>, grid, dim3(256), pair_lds_bytes(p.K, sizeof(T)), (hipStream_t)stream, p))
}

extern "C" int salt_gcn_pair_dgrad(const salt_gcn_pair_dgrad_args* a, void* stream) {
    if (!a) SALT_FAIL(SALT_E_BADARG, "gcn_pair_dgrad: null args");
    SALT_TRY(pair_shape_check("gcn_pair_dgrad", a->dtype, a->dx, a->dyv, a->dyh, a->K));
    if (!a->wv || !a->wh) SALT_FAIL(SALT_E_BADARG, "gcn_pair_dgrad: wv / wh");
    PairDgKP p;
    p.dy[0] = a->dyv.p; p.dy[1] = a->dyh.p; p.w[0] = a->wv; p.w[1] = a->wh; p.dx = a->dx.p;
    p.dy_cs[0] = a->dyv.cs; p.dy_cs[1] = a->dyh.cs; p.dy_vec[0] = 1; p.dy_vec[1] = 1;      // pair_shape_check: aligned, cs in whole pieces
    p.B = a->dx.B; p.H = a->dx.H; p.W = a->dx.W; p.Cin = a->dx.C; p.Cout = a->dyv.C; p.K = a->K; p.dx_cs = a->dx.cs;
    p.accumulate = a->accumulate ? 1 : 0;
    p.tiles_y = cdiv(p.H, GCN_TH); p.tiles_x = cdiv(p.W, GCN_TW); p.c_tiles = cdiv(p.Cin, 32);
    const dim3 grid((unsigned)(pair_tiles(a->dx) * p.c_tiles));
    SALT_DISPATCH_DTYPE(a->dtype, T, return salt_launch(gcn_pair_dgrad_kernel<T>, grid, dim3(256), dgrad_lds_bytes(p.K, sizeof(T)), (hipStream_t)stream, p))
}
