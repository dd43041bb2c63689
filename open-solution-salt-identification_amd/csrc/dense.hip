// dense.hip — the pre-activated 1x1 convolution of a DenseNet layer / transition (saltnet.h: salt_dense_conv, salt_dense_conv_dgrad,
// salt_dense_conv_wgrad): conv(relu(norm(x))) where x is a channel prefix of the block's concatenation buffer and norm belongs to the
// consumer.  The normalised copy of x is never stored: a register-staged loader applies the PINNED transform of the header
//     t = fmaf(x, in_scale[c], in_shift[c]);  a = round_to_dtype(max(0, t));  m = [t > 0]
// between the global load and the LDS store, and the matrix cores read their fragments from LDS.
// Weights come from the fp32 master [Cout][Cin] (no packed copy); bf16 rounds them on the way into LDS.
//   GEMMs          forward  D[n][p] = sum_c W[n][c] a[p][c]      K = Cin   A rows = output channels, B columns = pixels
//                  dgrad    D[c][p] = sum_n W[n][c] dy[p][n]     K = Cout  A = W transposed while staged, B = dy as stored
//                  wgrad    D[n][c] = sum_p dy[p][n] a[p][c]     K = pixels: both operands are transposed while staged
//   tiles          128 pixels x 64 channels per 256-thread workgroup, a wave owns 32 pixels x 64 channels (two 32 x 32 accumulators);
//                  the weight gradient 64 x 64 outputs, one 32 x 32 accumulator per wave.  K moves in chunks of 32.
//   operands       LDS rows are [row][32 k] of the storage type, padded to 80 (bf16) / 144 (f32) bytes.  bf16: v_mfma_f32_32x32x16_bf16,
//                  lane (r, h) reads k = 8 h .. 8 h + 7 of row r per 16-wide step.  f32: v_mfma_f32_32x32x2_f32 (exact f32), lane half h
//                  reads k = 16 h + 4 q .. + 3 and feeds one element per instruction - the k order inside a chunk is permuted the
//                  same way for both operands.
//   accumulators   column = lane & 31 (pixel; weight gradient: input channel), row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5): a lane
//                  holds 4 consecutive channels per register quad, stored as one 8 / 16-byte piece.
//   sums           every per-channel sum (forward statistics, dbeta / dgamma) is reduced over the tile in a fixed order (lane
//                  butterflies, then the four waves ascending) and leaves as a per-tile partial: no atomics, the same bits every run.
#include "common.h"

namespace {

constexpr int BMP = 128;              // pixels of a forward / data-gradient tile
constexpr int BC = 64;                // channels of a tile
constexpr int KC = 32;                // contraction chunk
constexpr int DW_TARGET_WGS = 512, DW_MIN_CHUNKS = 8;   // weight gradient: workgroups per launch, fewest 32-pixel chunks of a split

template <typename T> struct Lds {
    static constexpr int RS = sizeof(T) == 2 ? 40 : 36;           // row stride in elements: 80 / 144 bytes, 16-byte aligned
    static constexpr int NS = sizeof(T) == 2 ? 2 : 4;             // Mma steps per 32-wide chunk
};
// the 16-byte fragment of lane (r = row, h) for step s of a chunk
template <typename T>
__device__ __forceinline__ u32x4 frag(const T* tile, int row, int s, int h) {
    const int piece = sizeof(T) == 2 ? 2 * s + h : 4 * h + s;
    return *reinterpret_cast<const u32x4*>(tile + row * Lds<T>::RS + piece * Elem<T>::VE);
}
// the pinned transform on one 16-byte piece of x at channel c (a multiple of 4): floats in, floats out (rounded by the caller's pack)
template <int VE>
__device__ __forceinline__ void transform(float* f, const float* in_scale, const float* in_shift, int c) {
#pragma unroll
    for (int j = 0; j < VE; j += 4) {
        const f32x4 sc = *reinterpret_cast<const f32x4*>(in_scale + c + j), sh = *reinterpret_cast<const f32x4*>(in_shift + c + j);
#pragma unroll
        for (int e = 0; e < 4; ++e) f[j + e] = fmaxf(__fmaf_rn(f[j + e], sc[e], sh[e]), 0.f);
    }
}
template <typename T> __device__ __forceinline__ void zero_acc(f32x16& a) {
#pragma unroll
    for (int i = 0; i < 16; ++i) a[i] = 0.f;
}
// 4 consecutive elements of the storage type <-> floats
template <typename T> __device__ __forceinline__ f32x4 load4(const T* p);
template <> __device__ __forceinline__ f32x4 load4<float>(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
template <> __device__ __forceinline__ f32x4 load4<bf16_t>(const bf16_t* p) {
    const uint2 v = *reinterpret_cast<const uint2*>(p);
    return f32x4{__uint_as_float(v.x << 16), __uint_as_float(v.x & 0xffff0000u), __uint_as_float(v.y << 16), __uint_as_float(v.y & 0xffff0000u)};
}
// stores v and returns the STORED value
template <typename T> __device__ __forceinline__ f32x4 store4(T* p, f32x4 v);
template <> __device__ __forceinline__ f32x4 store4<float>(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; return v; }
template <> __device__ __forceinline__ f32x4 store4<bf16_t>(bf16_t* p, f32x4 v) {
    const unsigned lo = f2bf_pk(v.x, v.y), hi = f2bf_pk(v.z, v.w);
    *reinterpret_cast<uint2*>(p) = make_uint2(lo, hi);
    return f32x4{__uint_as_float(lo << 16), __uint_as_float(lo & 0xffff0000u), __uint_as_float(hi << 16), __uint_as_float(hi & 0xffff0000u)};
}
// 4 fp32 weights -> 4 elements of the storage type in LDS (contiguous)
template <typename T> __device__ __forceinline__ void put4(T* p, f32x4 v);
template <> __device__ __forceinline__ void put4<float>(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }
template <> __device__ __forceinline__ void put4<bf16_t>(bf16_t* p, f32x4 v) { *reinterpret_cast<uint2*>(p) = make_uint2(f2bf_pk(v.x, v.y), f2bf_pk(v.z, v.w)); }

// Sum of v over the 32 lanes of a half-wave (one pixel each), same result in all of them; fixed order
__device__ __forceinline__ float half_sum(float v) {
#pragma unroll
    for (int o = 1; o < 32; o <<= 1) v += __shfl_xor(v, o);
    return v;
}
// Per-channel sums of a 128-pixel x 64-channel tile held as acc[i][4 g + e] = channel 32 i + 8 g + 4 h + e of the lane's pixel:
// s_red [4][BC] receives each wave's sums; after the barrier thread t < 64 adds the four waves in ascending order.
__device__ __forceinline__ void tile_sums_to_lds(const f32x16* v, float (*s_red)[BC], int r, int h, int wave) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const float s = half_sum(v[i][q]);
            if (r == 0) s_red[wave][32 * i + 8 * (q >> 2) + 4 * h + (q & 3)] = s;
        }
}
__device__ __forceinline__ float waves_sum(float (*s_red)[BC], int t) { return ((s_red[0][t] + s_red[1][t]) + s_red[2][t]) + s_red[3][t]; }

// ---------------------------------------------------------------- forward
struct DenseKP {
    const void* x; void* y; const float* w; const float* in_scale; const float* in_shift;
    const float* scale; const float* shift; float* stats; float* stats_cnt;
    int64_t M; int Cin, Cout, x_cs, y_cs, relu, n_tiles;
};

template <typename T>
__global__ __launch_bounds__(256) void dense_fwd_kernel(DenseKP p) {
    constexpr int VE = Elem<T>::VE, RS = Lds<T>::RS, NS = Lds<T>::NS, PPR = KC / VE;
    __shared__ __attribute__((aligned(16))) T s_a[BMP * RS];
    __shared__ __attribute__((aligned(16))) T s_w[BC * RS];
    __shared__ float s_red[4][BC];
    __shared__ float s_mean[BC];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    const int nt = blockIdx.x % p.n_tiles, mt = blockIdx.x / p.n_tiles, n0 = nt * BC;
    const int64_t m0 = (int64_t)mt * BMP;
    const T* x = reinterpret_cast<const T*>(p.x);
    T* y = reinterpret_cast<T*>(p.y);
    f32x16 acc[2];
    zero_acc<T>(acc[0]); zero_acc<T>(acc[1]);
    for (int k0 = 0; k0 < p.Cin; k0 += KC) {
        __syncthreads();                                           // the previous chunk's fragment reads
        for (int i = tid; i < BMP * PPR; i += 256) {
            const int pc = i % PPR, px = i / PPR;
            const int64_t m = m0 + px;
            float f[VE];
            if (m < p.M) {
                unpack16<T>(*reinterpret_cast<const u32x4*>(x + m * p.x_cs + k0 + pc * VE), f);
                transform<VE>(f, p.in_scale, p.in_shift, k0 + pc * VE);
            } else {
#pragma unroll
                for (int j = 0; j < VE; ++j) f[j] = 0.f;
            }
            *reinterpret_cast<u32x4*>(s_a + px * RS + pc * VE) = pack16<T>(f);
        }
        for (int i = tid; i < BC * (KC / 4); i += 256) {
            const int q = i % (KC / 4), n = i / (KC / 4);
            put4<T>(s_w + n * RS + 4 * q, *reinterpret_cast<const f32x4*>(p.w + (int64_t)(n0 + n) * p.Cin + k0 + 4 * q));
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const u32x4 b = frag<T>(s_a, wave * 32 + r, s, h);
#pragma unroll
            for (int i = 0; i < 2; ++i) Mma<T>::step(frag<T>(s_w, i * 32 + r, s, h), b, acc[i]);
        }
    }
    // ---- epilogue: the lane holds pixel m0 + 32 wave + r, channels n0 + 32 i + 8 g + 4 h .. + 3
    const int64_t m = m0 + wave * 32 + r;
    const bool valid = m < p.M;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int ch = n0 + 32 * i + 8 * g + 4 * h;
            f32x4 v = f32x4{acc[i][4 * g], acc[i][4 * g + 1], acc[i][4 * g + 2], acc[i][4 * g + 3]};
            if (p.scale) {
                const f32x4 sc = *reinterpret_cast<const f32x4*>(p.scale + ch), sh = *reinterpret_cast<const f32x4*>(p.shift + ch);
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = __fmaf_rn(v[e], sc[e], sh[e]);
            }
            if (p.relu) {
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
            }
            if (valid) v = store4<T>(y + m * p.y_cs + ch, v);
            else v = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[i][4 * g + e] = v[e];          // statistics of the STORED value
        }
    if (!p.stats) return;
    const int64_t left = p.M - m0;
    const float cnt = (float)(left < BMP ? left : BMP);
    tile_sums_to_lds(acc, s_red, r, h, wave);
    __syncthreads();
    if (tid < BC) {
        const float tot = waves_sum(s_red, tid);
        s_mean[tid] = tot / cnt;
        p.stats[((int64_t)mt * 2) * p.Cout + n0 + tid] = tot;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const float d = valid ? acc[i][q] - s_mean[32 * i + 8 * (q >> 2) + 4 * h + (q & 3)] : 0.f;
            acc[i][q] = d * d;
        }
    tile_sums_to_lds(acc, s_red, r, h, wave);
    __syncthreads();
    if (tid < BC) p.stats[((int64_t)mt * 2 + 1) * p.Cout + n0 + tid] = waves_sum(s_red, tid);
    if (nt == 0 && tid == 0) p.stats_cnt[mt] = cnt;
}

// ---------------------------------------------------------------- data gradient (+ BatchNorm backward of the consumer-owned norm)
struct DgradKP {
    const void* dy; const void* x; void* dx; const float* w; const float* in_scale; const float* in_shift;
    const float* mean; const float* invstd; const float* gamma; float* partials; const float* sums;
    int64_t M; int Cin, Cout, dy_cs, x_cs, dx_cs, accumulate, c_tiles; float inv_n;
};

// PASS 0: the two sums of the tile -> partials.  PASS 1: the apply.
template <typename T, int PASS>
__global__ __launch_bounds__(256) void dense_dgrad_kernel(DgradKP p) {
    constexpr int VE = Elem<T>::VE, RS = Lds<T>::RS, NS = Lds<T>::NS, PPR = KC / VE;
    __shared__ __attribute__((aligned(16))) T s_a[BMP * RS];      // dy [pixel][n]
    __shared__ __attribute__((aligned(16))) T s_w[BC * RS];       // W transposed [c][n]
    __shared__ float s_red[4][BC];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    const int ct = blockIdx.x % p.c_tiles, mt = blockIdx.x / p.c_tiles, c0 = ct * BC;
    const int nblk = c0 + 32 < p.Cin ? 2 : 1;                      // Cin is a multiple of 32: the tile's second half may lie past it
    const int64_t m0 = (int64_t)mt * BMP;
    const T* dy = reinterpret_cast<const T*>(p.dy);
    const T* x = reinterpret_cast<const T*>(p.x);
    T* dx = reinterpret_cast<T*>(p.dx);
    f32x16 acc[2];
    zero_acc<T>(acc[0]); zero_acc<T>(acc[1]);
    for (int n0 = 0; n0 < p.Cout; n0 += KC) {
        __syncthreads();
        for (int i = tid; i < BMP * PPR; i += 256) {
            const int pc = i % PPR, px = i / PPR;
            const int64_t m = m0 + px;
            u32x4 v = u32x4{0u, 0u, 0u, 0u};
            if (m < p.M) v = *reinterpret_cast<const u32x4*>(dy + m * p.dy_cs + n0 + pc * VE);
            *reinterpret_cast<u32x4*>(s_a + px * RS + pc * VE) = v;
        }
        for (int i = tid; i < KC * (BC / 4); i += 256) {
            const int q = i % (BC / 4), n = i / (BC / 4);
            f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
            if (c0 + 4 * q < p.Cin) v = *reinterpret_cast<const f32x4*>(p.w + (int64_t)(n0 + n) * p.Cin + c0 + 4 * q);
#pragma unroll
            for (int e = 0; e < 4; ++e) Elem<T>::st(s_w + (4 * q + e) * RS + n, v[e]);
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const u32x4 b = frag<T>(s_a, wave * 32 + r, s, h);
#pragma unroll
            for (int i = 0; i < 2; ++i)
                if (i < nblk) Mma<T>::step(frag<T>(s_w, i * 32 + r, s, h), b, acc[i]);
        }
    }
    // ---- epilogue: the lane holds pixel m0 + 32 wave + r, input channels c0 + 32 i + 8 g + 4 h .. + 3
    const int64_t m = m0 + wave * 32 + r;
    const bool valid = m < p.M;
    f32x16 s2[2];                                                  // PASS 0: g xhat (acc keeps g)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int ch = c0 + 32 * i + 8 * g + 4 * h;
            const bool ok = valid && i < nblk;
            f32x4 gv = f32x4{0.f, 0.f, 0.f, 0.f}, xh = gv;
            if (ok) {
                const f32x4 xv = load4<T>(x + m * p.x_cs + ch);
                const f32x4 sc = *reinterpret_cast<const f32x4*>(p.in_scale + ch), sh = *reinterpret_cast<const f32x4*>(p.in_shift + ch);
                const f32x4 mu = *reinterpret_cast<const f32x4*>(p.mean + ch), is = *reinterpret_cast<const f32x4*>(p.invstd + ch);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    gv[e] = __fmaf_rn(xv[e], sc[e], sh[e]) > 0.f ? acc[i][4 * g + e] : 0.f;
                    xh[e] = __fmul_rn(__fsub_rn(xv[e], mu[e]), is[e]);
                }
            }
            if (PASS == 0) {
#pragma unroll
                for (int e = 0; e < 4; ++e) { acc[i][4 * g + e] = gv[e]; s2[i][4 * g + e] = __fmul_rn(gv[e], xh[e]); }
            } else if (ok) {
                const f32x4 s1 = *reinterpret_cast<const f32x4*>(p.sums + ch), sx = *reinterpret_cast<const f32x4*>(p.sums + p.Cin + ch);
                const f32x4 ga = *reinterpret_cast<const f32x4*>(p.gamma + ch), is = *reinterpret_cast<const f32x4*>(p.invstd + ch);
                f32x4 v;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float k = __fmul_rn(ga[e], is[e]);
                    const float t = __fsub_rn(__fsub_rn(gv[e], __fmul_rn(s1[e], p.inv_n)), __fmul_rn(xh[e], __fmul_rn(sx[e], p.inv_n)));
                    v[e] = __fmul_rn(k, t);
                }
                T* o = dx + m * p.dx_cs + ch;
                if (p.accumulate) v += load4<T>(o);
                store4<T>(o, v);
            }
        }
    if (PASS == 0) {
        tile_sums_to_lds(acc, s_red, r, h, wave);
        __syncthreads();
        if (tid < BC && c0 + tid < p.Cin) p.partials[((int64_t)mt * 2) * p.Cin + c0 + tid] = waves_sum(s_red, tid);
        __syncthreads();
        tile_sums_to_lds(s2, s_red, r, h, wave);
        __syncthreads();
        if (tid < BC && c0 + tid < p.Cin) p.partials[((int64_t)mt * 2 + 1) * p.Cin + c0 + tid] = waves_sum(s_red, tid);
    }
}

// partials [nparts][2][C] -> sums [2][C] (and dbeta / dgamma): 64 channels x 4 part-rows per workgroup; a row adds its parts
// k = row, row + 4, ... in ascending order in fp64, the rows meet in ascending order, one rounding to fp32
__global__ __launch_bounds__(256) void dense_dgrad_finalize_kernel(const float* partials, int nparts, int C, float* sums, float* dgamma, float* dbeta, int accumulate) {
    __shared__ double sm[2][4][64];
    const int cl = threadIdx.x & 63, row = threadIdx.x >> 6, c = blockIdx.x * 64 + cl;
    double a1 = 0.0, a2 = 0.0;
    if (c < C)
        for (int k = row; k < nparts; k += 4) { a1 += (double)partials[((int64_t)k * 2) * C + c]; a2 += (double)partials[((int64_t)k * 2 + 1) * C + c]; }
    sm[0][row][cl] = a1; sm[1][row][cl] = a2;
    __syncthreads();
    if (row == 0 && c < C) {
        const float s1 = (float)(((sm[0][0][cl] + sm[0][1][cl]) + sm[0][2][cl]) + sm[0][3][cl]);
        const float s2 = (float)(((sm[1][0][cl] + sm[1][1][cl]) + sm[1][2][cl]) + sm[1][3][cl]);
        sums[c] = s1; sums[C + c] = s2;
        if (dbeta) dbeta[c] = accumulate ? dbeta[c] + s1 : s1;
        if (dgamma) dgamma[c] = accumulate ? dgamma[c] + s2 : s2;
    }
}

// ---------------------------------------------------------------- weight gradient
struct DwKP {
    const void* x; const void* dy; const float* in_scale; const float* in_shift; float* partials;
    int64_t M; int Cin, Cout, x_cs, dy_cs, n_tiles, c_tiles, nchunks, cps;
};

template <typename T>
__global__ __launch_bounds__(256) void dense_wgrad_kernel(DwKP p) {
    constexpr int VE = Elem<T>::VE, RS = Lds<T>::RS, NS = Lds<T>::NS, PPT = BC / VE;
    __shared__ __attribute__((aligned(16))) T s_a[BC * RS];       // dy transposed [n][pixel]
    __shared__ __attribute__((aligned(16))) T s_w[BC * RS];       // a(x) transposed [c][pixel]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    int bid = blockIdx.x;
    const int ct = bid % p.c_tiles; bid /= p.c_tiles;
    const int nt = bid % p.n_tiles, split = bid / p.n_tiles;
    const int n0 = nt * BC, c0 = ct * BC, nb = wave & 1, cb = wave >> 1;
    const bool mine = c0 + 32 * cb < p.Cin;                        // this wave's 32 input channels exist
    const T* x = reinterpret_cast<const T*>(p.x);
    const T* dy = reinterpret_cast<const T*>(p.dy);
    f32x16 acc;
    zero_acc<T>(acc);
    const int ch_end = (split + 1) * p.cps < p.nchunks ? (split + 1) * p.cps : p.nchunks;
    for (int chunk = split * p.cps; chunk < ch_end; ++chunk) {
        const int64_t m0 = (int64_t)chunk * KC;
        __syncthreads();
        for (int i = tid; i < KC * PPT; i += 256) {
            const int pc = i % PPT, px = i / PPT;
            const int64_t m = m0 + px;
            float f[VE], d[VE];
            const bool okx = m < p.M && c0 + pc * VE < p.Cin;
            if (m < p.M) unpack16<T>(*reinterpret_cast<const u32x4*>(dy + m * p.dy_cs + n0 + pc * VE), d);
            if (okx) {
                unpack16<T>(*reinterpret_cast<const u32x4*>(x + m * p.x_cs + c0 + pc * VE), f);
                transform<VE>(f, p.in_scale, p.in_shift, c0 + pc * VE);
            }
#pragma unroll
            for (int j = 0; j < VE; ++j) {
                Elem<T>::st(s_a + (pc * VE + j) * RS + px, m < p.M ? d[j] : 0.f);
                Elem<T>::st(s_w + (pc * VE + j) * RS + px, okx ? f[j] : 0.f);
            }
        }
        __syncthreads();
        if (mine) {
#pragma unroll
            for (int s = 0; s < NS; ++s) Mma<T>::step(frag<T>(s_a, nb * 32 + r, s, h), frag<T>(s_w, cb * 32 + r, s, h), acc);
        }
    }
    if (!mine) return;
    // the lane holds column c0 + 32 cb + r, rows n0 + 32 nb + (q & 3) + 8 (q >> 2) + 4 h
    float* slab = p.partials + (int64_t)split * p.Cout * p.Cin;
#pragma unroll
    for (int q = 0; q < 16; ++q)
        slab[(int64_t)(n0 + 32 * nb + (q & 3) + 8 * (q >> 2) + 4 * h) * p.Cin + c0 + 32 * cb + r] = acc[q];
}

// ---------------------------------------------------------------- moments of a stored view / per-layer BatchNorm coefficients
// Per-tile (sum, M2 about the tile's own mean, count) of a [pixels][C] view, salt_bn_finalize's protocol: a workgroup owns 128 pixels x
// 64 channels, thread (row, channel) walks pixels row, row + 4, ... in ascending order, the four rows meet in ascending order.
template <typename T>
__global__ __launch_bounds__(256) void dense_moments_kernel(const T* x, int64_t M, int C, int cs, int c_tiles, float* stats, float* stats_cnt) {
    __shared__ float sm[4][64];
    const int cl = threadIdx.x & 63, row = threadIdx.x >> 6;
    const int ct = blockIdx.x % c_tiles, mt = blockIdx.x / c_tiles, c = ct * 64 + cl;
    const int64_t m0 = (int64_t)mt * BMP;
    const int64_t left = M - m0;
    const int n = (int)(left < BMP ? left : BMP);
    const bool ok = c < C;
    float s = 0.f;
    if (ok) for (int i = row; i < n; i += 4) s += Elem<T>::ld(x + (m0 + i) * cs + c);
    sm[row][cl] = s;
    __syncthreads();
    const float tot = ((sm[0][cl] + sm[1][cl]) + sm[2][cl]) + sm[3][cl];
    const float mean = tot / (float)n;
    __syncthreads();
    float q = 0.f;
    if (ok) for (int i = row; i < n; i += 4) { const float d = Elem<T>::ld(x + (m0 + i) * cs + c) - mean; q = __fmaf_rn(d, d, q); }
    sm[row][cl] = q;
    __syncthreads();
    if (row == 0 && ok) {
        stats[((int64_t)mt * 2) * C + c] = tot;
        stats[((int64_t)mt * 2 + 1) * C + c] = ((sm[0][cl] + sm[1][cl]) + sm[2][cl]) + sm[3][cl];
    }
    if (ct == 0 && threadIdx.x == 0) stats_cnt[mt] = (float)n;
}

// the arithmetic of bn_finalize_kernel's last step, from a statistics table instead of partials
__global__ __launch_bounds__(256) void dense_bn_prep_kernel(salt_dense_bn_prep_args a) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c < a.C) {
        const float mean = a.mean[c], sc = a.gamma[c] * a.invstd[c];
        a.in_scale[c] = sc; a.in_shift[c] = a.beta[c] - mean * sc;
        if (a.running_mean) {
            a.running_mean[c] = (1.f - a.momentum) * a.running_mean[c] + a.momentum * mean;
            a.running_var[c] = (1.f - a.momentum) * a.running_var[c] + a.momentum * a.unbiased_var[c];
        }
    }
    if (c == 0 && a.num_batches_tracked) *a.num_batches_tracked += 1;
}

// ---------------------------------------------------------------- host
int dense_shape_check(const char* op, const salt_view& x, int Cout) {
    if (x.C < 32 || x.C > 2048 || x.C % 32) SALT_FAIL(SALT_E_UNSUPPORTED, "%s: %d input channels (supported: multiples of 32 in [32, 2048])", op, x.C);
    if (Cout < 64 || Cout > 1024 || Cout % 64) SALT_FAIL(SALT_E_UNSUPPORTED, "%s: %d output channels (supported: multiples of 64 in [64, 1024])", op, Cout);
    if (x.B < 1 || x.H < 1 || x.W < 1) SALT_FAIL(SALT_E_BADARG, "%s: empty batch %d x %d x %d", op, x.B, x.H, x.W);
    if (view_pixels(x) >= (1ll << 31) / 64) SALT_FAIL(SALT_E_UNSUPPORTED, "%s: too many pixels", op);
    return SALT_OK;
}
int dense_vec_check(const char* op, const char* what, const void* p) {
    if (!p || !aligned16(p)) SALT_FAIL(SALT_E_BADARG, "%s: %s must be a 16-byte aligned device pointer", op, what);
    return SALT_OK;
}
inline int m_tiles(const salt_view& x) { return (int)((view_pixels(x) + BMP - 1) / BMP); }

// pixel splits of the weight gradient: a function of the shape alone
void dwgrad_plan(DwKP& p, int& nsplit) {
    p.n_tiles = p.Cout / BC; p.c_tiles = cdiv(p.Cin, BC);
    p.nchunks = (int)((p.M + KC - 1) / KC);
    const int want = DW_TARGET_WGS / (p.n_tiles * p.c_tiles) > 0 ? DW_TARGET_WGS / (p.n_tiles * p.c_tiles) : 1;
    p.cps = cdiv(p.nchunks, want);
    if (p.cps < DW_MIN_CHUNKS) p.cps = DW_MIN_CHUNKS;
    nsplit = cdiv(p.nchunks, p.cps);
}

}  // namespace

extern "C" int salt_dense_conv_stats_parts(const salt_dense_conv_args* a) {
    if (!a) SALT_FAIL(SALT_E_BADARG, "dense_conv: null args");
    const int rc = dense_shape_check("dense_conv", a->x, a->y.C);
    if (rc) return rc;
    return m_tiles(a->x);
}

extern "C" int salt_dense_conv(const salt_dense_conv_args* a, void* stream) {
    if (!a) SALT_FAIL(SALT_E_BADARG, "dense_conv: null args");
    int rc = dense_shape_check("dense_conv", a->x, a->y.C);
    if (rc) return rc;
    if (a->dtype != SALT_F32 && a->dtype != SALT_BF16) SALT_FAIL(SALT_E_BADARG, "dense_conv: bad dtype %d", a->dtype);
    if ((rc = view_check16("dense_conv", "x", a->x, a->dtype, a->x.B, a->x.H, a->x.W, a->x.C))) return rc;
    if ((rc = view_check16("dense_conv", "y", a->y, a->dtype, a->x.B, a->x.H, a->x.W, a->y.C))) return rc;
    if ((rc = dense_vec_check("dense_conv", "w", a->w))) return rc;
    if ((rc = dense_vec_check("dense_conv", "in_scale", a->in_scale))) return rc;
    if ((rc = dense_vec_check("dense_conv", "in_shift", a->in_shift))) return rc;
    if ((a->scale == nullptr) != (a->shift == nullptr)) SALT_FAIL(SALT_E_BADARG, "dense_conv: scale/shift");
    if (a->scale && (!aligned16(a->scale) || !aligned16(a->shift))) SALT_FAIL(SALT_E_BADARG, "dense_conv: scale / shift must be 16-byte aligned");
    if ((a->stats == nullptr) != (a->stats_cnt == nullptr)) SALT_FAIL(SALT_E_BADARG, "dense_conv: stats/stats_cnt");
    if (a->stats && (a->scale || a->relu)) SALT_FAIL(SALT_E_BADARG, "dense_conv: the train form stores the raw output (no scale / shift / relu)");
    DenseKP p;
    p.x = a->x.p; p.y = a->y.p; p.w = a->w; p.in_scale = a->in_scale; p.in_shift = a->in_shift; p.scale = a->scale; p.shift = a->shift;
    p.stats = a->stats; p.stats_cnt = a->stats_cnt;
    p.M = view_pixels(a->x); p.Cin = a->x.C; p.Cout = a->y.C; p.x_cs = a->x.cs; p.y_cs = a->y.cs; p.relu = a->relu ? 1 : 0; p.n_tiles = p.Cout / BC;
    const dim3 grid((unsigned)(m_tiles(a->x) * p.n_tiles));
    SALT_DISPATCH_DTYPE(a->dtype, T, return salt_launch(dense_fwd_kernel<T>, grid, dim3(256), 0, (hipStream_t)stream, p))
}

extern "C" int salt_dense_conv_dgrad_parts(const salt_dense_conv_dgrad_args* a) {
    if (!a) SALT_FAIL(SALT_E_BADARG, "dense_conv_dgrad: null args");
    const int rc = dense_shape_check("dense_conv_dgrad", a->x, a->dy.C);
    if (rc) return rc;
    return m_tiles(a->x);
}

extern "C" int salt_dense_conv_dgrad(const salt_dense_conv_dgrad_args* a, void* stream) {
    if (!a) SALT_FAIL(SALT_E_BADARG, "dense_conv_dgrad: null args");
    int rc = dense_shape_check("dense_conv_dgrad", a->x, a->dy.C);
    if (rc) return rc;
    if (a->dtype != SALT_F32 && a->dtype != SALT_BF16) SALT_FAIL(SALT_E_BADARG, "dense_conv_dgrad: bad dtype %d", a->dtype);
    if ((rc = view_check16("dense_conv_dgrad", "x", a->x, a->dtype, a->x.B, a->x.H, a->x.W, a->x.C))) return rc;
    if ((rc = view_check16("dense_conv_dgrad", "dy", a->dy, a->dtype, a->x.B, a->x.H, a->x.W, a->dy.C))) return rc;
    if ((rc = view_check16("dense_conv_dgrad", "dx", a->dx, a->dtype, a->x.B, a->x.H, a->x.W, a->x.C))) return rc;
    if ((rc = dense_vec_check("dense_conv_dgrad", "w", a->w))) return rc;
    if ((rc = dense_vec_check("dense_conv_dgrad", "in_scale", a->in_scale))) return rc;
    if ((rc = dense_vec_check("dense_conv_dgrad", "in_shift", a->in_shift))) return rc;
    if ((rc = dense_vec_check("dense_conv_dgrad", "mean", a->mean))) return rc;
    if ((rc = dense_vec_check("dense_conv_dgrad", "invstd", a->invstd))) return rc;
    if ((rc = dense_vec_check("dense_conv_dgrad", "gamma", a->gamma))) return rc;
    if ((rc = dense_vec_check("dense_conv_dgrad", "sums", a->sums))) return rc;
    if (!a->partials) SALT_FAIL(SALT_E_BADARG, "dense_conv_dgrad: partials");
    const int nparts = m_tiles(a->x);
    if (a->nparts != nparts) SALT_FAIL(SALT_E_BADARG, "dense_conv_dgrad: nparts %d, salt_dense_conv_dgrad_parts says %d", a->nparts, nparts);
    DgradKP p;
    p.dy = a->dy.p; p.x = a->x.p; p.dx = a->dx.p; p.w = a->w; p.in_scale = a->in_scale; p.in_shift = a->in_shift;
    p.mean = a->mean; p.invstd = a->invstd; p.gamma = a->gamma; p.partials = a->partials; p.sums = a->sums;
    p.M = view_pixels(a->x); p.Cin = a->x.C; p.Cout = a->dy.C; p.dy_cs = a->dy.cs; p.x_cs = a->x.cs; p.dx_cs = a->dx.cs;
    p.accumulate = a->accumulate ? 1 : 0; p.c_tiles = cdiv(p.Cin, BC); p.inv_n = 1.0f / (float)p.M;
    const dim3 grid((unsigned)(nparts * p.c_tiles));
    hipStream_t st = (hipStream_t)stream;
    SALT_DISPATCH_DTYPE(a->dtype, T, rc = salt_launch(dense_dgrad_kernel<T, 0>, grid, dim3(256), 0, st, p))
    if (rc) return rc;
    rc = salt_launch(dense_dgrad_finalize_kernel, dim3(cdiv(p.Cin, 64)), dim3(256), 0, st, (const float*)a->partials, nparts, p.Cin, a->sums, a->dgamma, a->dbeta,
                     a->accumulate_param_grads ? 1 : 0);
    if (rc) return rc;
    SALT_DISPATCH_DTYPE(a->dtype, T, return salt_launch(dense_dgrad_kernel<T, 1>, grid, dim3(256), 0, st, p))
}

extern "C" int salt_dense_conv_wgrad_parts(const salt_dense_conv_wgrad_args* a) {
    if (!a) SALT_FAIL(SALT_E_BADARG, "dense_conv_wgrad: null args");
    const int rc = dense_shape_check("dense_conv_wgrad", a->x, a->dy.C);
    if (rc) return rc;
    DwKP p; int nsplit = 0;
    p.M = view_pixels(a->x); p.Cin = a->x.C; p.Cout = a->dy.C;
    dwgrad_plan(p, nsplit);
    return nsplit;
}

extern "C" int salt_dense_conv_wgrad(const salt_dense_conv_wgrad_args* a, void* stream) {
    if (!a) SALT_FAIL(SALT_E_BADARG, "dense_conv_wgrad: null args");
    int rc = dense_shape_check("dense_conv_wgrad", a->x, a->dy.C);
    if (rc) return rc;
    if (a->dtype != SALT_F32 && a->dtype != SALT_BF16) SALT_FAIL(SALT_E_BADARG, "dense_conv_wgrad: bad dtype %d", a->dtype);
    if ((rc = view_check16("dense_conv_wgrad", "x", a->x, a->dtype, a->x.B, a->x.H, a->x.W, a->x.C))) return rc;
    if ((rc = view_check16("dense_conv_wgrad", "dy", a->dy, a->dtype, a->x.B, a->x.H, a->x.W, a->dy.C))) return rc;
    if ((rc = dense_vec_check("dense_conv_wgrad", "in_scale", a->in_scale))) return rc;
    if ((rc = dense_vec_check("dense_conv_wgrad", "in_shift", a->in_shift))) return rc;
    if (!a->partials || !a->grad) SALT_FAIL(SALT_E_BADARG, "dense_conv_wgrad: partials / grad");
    DwKP p; int nsplit = 0;
    p.x = a->x.p; p.dy = a->dy.p; p.in_scale = a->in_scale; p.in_shift = a->in_shift; p.partials = a->partials;
    p.M = view_pixels(a->x); p.Cin = a->x.C; p.Cout = a->dy.C; p.x_cs = a->x.cs; p.dy_cs = a->dy.cs;
    dwgrad_plan(p, nsplit);
    if (a->nsplit != nsplit) SALT_FAIL(SALT_E_BADARG, "dense_conv_wgrad: nsplit %d, salt_dense_conv_wgrad_parts says %d", a->nsplit, nsplit);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)(nsplit * p.n_tiles * p.c_tiles));
    SALT_DISPATCH_DTYPE(a->dtype, T, rc = salt_launch(dense_wgrad_kernel<T>, grid, dim3(256), 0, st, p))
    if (rc) return rc;
    const int total = p.Cout * p.Cin;
    return salt_launch(slab_sum_kernel<>, dim3(cdiv(total, 256)), dim3(256), 0, st, (const float*)a->partials, nsplit, total, a->grad, a->accumulate ? 1 : 0);
}

extern "C" int salt_dense_moments_parts(const salt_dense_moments_args* a) {
    if (!a) SALT_FAIL(SALT_E_BADARG, "dense_moments: null args");
    if (a->x.B < 1 || a->x.H < 1 || a->x.W < 1 || a->x.C < 1 || view_pixels(a->x) >= (1ll << 31) / 64) SALT_FAIL(SALT_E_UNSUPPORTED, "dense_moments: shape");
    return m_tiles(a->x);
}

extern "C" int salt_dense_moments(const salt_dense_moments_args* a, void* stream) {
    if (!a) SALT_FAIL(SALT_E_BADARG, "dense_moments: null args");
    if (a->dtype != SALT_F32 && a->dtype != SALT_BF16) SALT_FAIL(SALT_E_BADARG, "dense_moments: bad dtype %d", a->dtype);
    if (!view_ok(a->x) || view_pixels(a->x) >= (1ll << 31) / 64) SALT_FAIL(SALT_E_BADARG, "dense_moments: x");
    if (!a->stats || !a->stats_cnt) SALT_FAIL(SALT_E_BADARG, "dense_moments: stats / stats_cnt");
    const int c_tiles = cdiv(a->x.C, 64);
    const dim3 grid((unsigned)(m_tiles(a->x) * c_tiles));
    SALT_DISPATCH_DTYPE(a->dtype, T, return salt_launch(dense_moments_kernel<T>, grid, dim3(256), 0, (hipStream_t)stream, (const T*)a->x.p, view_pixels(a->x),
                                                        a->x.C, a->x.cs, c_tiles, a->stats, a->stats_cnt))
}

extern "C" int salt_dense_bn_prep(const salt_dense_bn_prep_args* a, void* stream) {
    if (!a || a->C < 1 || !a->mean || !a->invstd || !a->gamma || !a->beta || !a->in_scale || !a->in_shift) SALT_FAIL(SALT_E_BADARG, "dense_bn_prep: bad args");
    if ((a->running_mean == nullptr) != (a->running_var == nullptr) || (a->running_mean && !a->unbiased_var))
        SALT_FAIL(SALT_E_BADARG, "dense_bn_prep: running_mean / running_var / unbiased_var go together");
    return salt_launch(dense_bn_prep_kernel, dim3(cdiv(a->C, 256)), dim3(256), 0, (hipStream_t)stream, *a);
}
