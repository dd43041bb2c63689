// conv_wgrad.hip — the split-K weight-gradient kernels of the convolution family (conv_mfma.hip) on the CDNA4 matrix cores (gfx950).
//
//   dW[t][a][b] = sum_p P[p,a] * Q[pad(p*q_step + tap_t), b]        (saltnet.h, salt_conv_wgrad_args)
//
// Workgroup = 64(a) x 64(b) block for all taps of the launch over a slice of the pixel tiles (split-K); 4 waves as 2(a) x 2(b), each
// 32x32 per tap.  Every split writes a partial slab [ntaps][Ca][Cb]; salt_wgrad_reduce sums the slabs in fixed order.  Four kernels
// share that decomposition and the pieces below (workgroup decode, tile walk, per-tile loader origin, slab store):
//   conv_wgrad_kernel         any dtype / tap list / alignment (its own scalar-capable loader)
//   conv_wgrad_fast_kernel    bf16, whole aligned pieces, 1 or 5 - 9 taps
//   conv_wgrad_fast8_kernel   bf16, raster 3x3 on 16 x 8 row tiles, 8 waves
//   conv_wgrad_fast32_kernel  fp32, raster 3x3 on 16 x 8 row tiles
// conv_wgrad_ls.hip and conv_thin.hip hold the two kernels with other decompositions; salt_conv_wgrad tries them first.
#include <cstdlib>
#include <type_traits>
#include "common.h"

namespace {

struct WgradKP {
    const void* P; const void* Q; float* partials;
    int B, PH, PW, Ca, p_cs;        // P view (output-grid pixels)
    int QH, QW, Cb, q_cs;
    int ntaps; int tap_off[SALT_MAX_TAPS];
    int q_step, pad_mode, min_dy, min_dx;
    int th_log2, tw_log2, nb, hh, hw;
    int tiles_y, tiles_x, ntiles, nsplit;
    int a_blocks, b_blocks;
    int bmp;                        // pixels per K tile (64 | 128)
    long long q_plane;              // salt_conv_wgrad_args.q_plane: b-block bb reads the dense plane Q + bb * q_plane (0: channel-interleaved rows)
    int ksplit;                     // conv_wgrad_kernel<float>: 0 off; 4: Ca, Cb <= 32 - the four waves share block (0, 0) and a quarter of the k-steps each;
                                    // 2: Ca <= 32 - waves (wa, wb) work on block (0, wb), k-step pairs of parity wa; 3: Cb <= 32 - block (wa, 0), parity wb
};

__device__ __forceinline__ void slab_put4(float* dst, const f32x4& v) { *reinterpret_cast<f32x4*>(dst) = v; }   // 64 channels per pixel row

// 16 zero bytes in device memory: a masked-out piece of the branch-free loader reads them instead of zero-initialising its
// destination registers under a branch (see conv_wgrad_fast_kernel)
__device__ __attribute__((aligned(16))) unsigned int g_wg_zero[4] = {0u, 0u, 0u, 0u};

// ---- workgroup decode: channel block (ab, bb) and split of this workgroup, its first channels and operand bases
template <typename T> struct WgBlock { int ab, bb, split, a0, c0, hhw; const T* Pg; const T* Qg; };      // hhw: pixels of one image's halo
template <typename T>
__device__ __forceinline__ WgBlock<T> wg_block(const WgradKP& p) {
    WgBlock<T> w;
    const int blk = blockIdx.x;
    w.ab = blk % p.a_blocks;
    w.bb = (blk / p.a_blocks) % p.b_blocks;
    w.split = blk / (p.a_blocks * p.b_blocks);
    w.a0 = w.ab * 64; w.c0 = w.bb * 64;
    w.hhw = p.hh * p.hw;
    w.Pg = reinterpret_cast<const T*>(p.P);
    w.Qg = reinterpret_cast<const T*>(p.Q) + (p.q_plane ? (long long)w.bb * p.q_plane - w.c0 : 0);   // planar Q: channel c0 + j of block bb is element j of plane bb
    return w;
}

// ---- tile walk without divisions: tile = (tbi, tyi, txi), advanced by nsplit with carries
struct TileC { int tbi, tyi, txi; };
struct TileWalk {
    int tiles_x, tiles_y; TileC step;
    __device__ __forceinline__ explicit TileWalk(const WgradKP& p) : tiles_x(p.tiles_x), tiles_y(p.tiles_y) { step = decode(p.nsplit); }
    __device__ __forceinline__ TileC decode(int tile) const {
        TileC c; c.txi = tile % tiles_x; const int tt = tile / tiles_x; c.tyi = tt % tiles_y; c.tbi = tt / tiles_y; return c;
    }
    __device__ __forceinline__ void advance(TileC& c) const {
        c.txi += step.txi; if (c.txi >= tiles_x) { c.txi -= tiles_x; ++c.tyi; }
        c.tyi += step.tyi; if (c.tyi >= tiles_y) { c.tyi -= tiles_y; ++c.tbi; }
        c.tbi += step.tbi;
    }
};

// ---- per-tile origin of the fast kernels' branch-free piece loaders: a handful of uniform values, while every piece keeps only
// tile-invariant lane constants.  rowQ = QW * q_cs.  Without PAD, baseQ may point in front of the image: in-range pieces only.
template <typename T> struct TileCtx { const T* baseP; const T* baseQ; int iy0, ix0, limB, limY, limX; };
template <typename T, bool PAD>
__device__ __forceinline__ TileCtx<T> tile_ctx(const WgradKP& p, const WgBlock<T>& w, int rowQ, const TileC& c, bool live) {
    TileCtx<T> x;
    x.limB = live ? p.B - c.tbi * p.nb : 0;                          // no next tile: every piece is masked out
    x.limY = p.PH - (c.tyi << p.th_log2); x.limX = p.PW - (c.txi << p.tw_log2);
    x.baseP = w.Pg + (((int64_t)c.tbi * p.nb * p.PH + (c.tyi << p.th_log2)) * p.PW + (c.txi << p.tw_log2)) * p.p_cs;
    x.iy0 = (c.tyi << p.th_log2) * p.q_step + p.min_dy; x.ix0 = (c.txi << p.tw_log2) * p.q_step + p.min_dx;
    x.baseQ = w.Qg + (int64_t)c.tbi * p.nb * p.QH * rowQ;
    if (!PAD) x.baseQ += (int64_t)x.iy0 * rowQ + (int64_t)x.ix0 * p.q_cs;
    return x;
}

// ---- slab store of the swapped-operand (D^T) accumulator: lane = a-row, 4 consecutive registers = 4 consecutive b, so tap t of the
// partial slab partials[split][t][a][b] takes 16-byte stores.  The caller tests t < ntaps and a < Ca.
template <typename T>
__device__ __forceinline__ void slab_store(const WgradKP& p, const WgBlock<T>& w, const f32x16& acc, int t, int a, int wb, int khalf) {
    float* row = p.partials + (((int64_t)w.split * p.ntaps + t) * p.Ca + a) * p.Cb;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int b = w.c0 + wb * 32 + 8 * g + 4 * khalf;
        if (b < p.Cb) slab_put4(row + b, f32x4{acc[4 * g], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]});
    }
}

template <typename T, int NT>
__global__ __launch_bounds__(256) void conv_wgrad_kernel(WgradKP p) {
    constexpr int VE = Elem<T>::VE;
    constexpr int PPR = 64 / VE;                                // 16-byte pieces per pixel row
    constexpr int ROWB = (sizeof(T) == 2) ? 192 : 256;           // bf16 rows padded to 192 B: conflict-free tr reads
    constexpr bool PIPE = sizeof(T) == 2;                        // register-prefetch pipeline (fits the VGPR budget for bf16)
    constexpr int MAXP = 128 * PPR / 256, MAXQ = 10;
    const int BMP = p.bmp;                                       // pixels per K tile
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* sP = smem;
    unsigned char* sQ = smem + BMP * ROWB;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wa = wave >> 1, wb = wave & 1;
    const WgBlock<T> w = wg_block<T>(p);
    const int split = w.split, a0 = w.a0, c0 = w.c0;
    const int hhw = w.hhw, phalo = p.nb * hhw;
    const T* Pg = w.Pg;
    const T* Qg = w.Qg;
    const bool p_vec = ((p.p_cs % VE) == 0) && ((reinterpret_cast<uintptr_t>(p.P) & 15) == 0);
    const bool q_vec = ((p.q_cs % VE) == 0) && ((reinterpret_cast<uintptr_t>(p.Q) & 15) == 0);

    f32x16 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

    const TileWalk walk(p);
    // ---- tile-invariant piece descriptors.  Piece q = tid + 256 k covers 16 bytes of pixel row q / PPR; 256 % PPR == 0, so the
    // channel piece (tid % PPR) is the same for every k and only the pixel coordinates (packed bl:ty:tx / bl:hy:hx) differ.
    const int pcx = tid % PPR;
    const int chP = a0 + pcx * VE, chQ = c0 + pcx * VE;
    const int np = BMP * PPR, nq = phalo * PPR;
    auto descP = [&](int q) -> unsigned {
        if (q >= np || chP >= p.Ca) return 0xffffffffu;
        const int m = q / PPR;
        const int tx = m & ((1 << p.tw_log2) - 1);
        const int ty = (m >> p.tw_log2) & ((1 << p.th_log2) - 1);
        const int bl = m >> (p.tw_log2 + p.th_log2);
        return (unsigned)((bl << 16) | (ty << 8) | tx);
    };
    auto descQ = [&](int q) -> unsigned {
        if (q >= nq || chQ >= p.Cb) return 0xffffffffu;
        const int pix = q / PPR;
        const int bl = pix / hhw;
        const int r = pix - bl * hhw;
        const int hy = r / p.hw, hx = r - hy * p.hw;
        return (unsigned)((bl << 16) | (hy << 8) | hx);
    };
    auto fetchP = [&](const TileC& c, unsigned d) -> u32x4 {
        u32x4 v = {0u, 0u, 0u, 0u};
        if (d == 0xffffffffu) return v;
        const int oy = (c.tyi << p.th_log2) + (int)((d >> 8) & 255u), ox = (c.txi << p.tw_log2) + (int)(d & 255u), b = c.tbi * p.nb + (int)(d >> 16);
        if (b < p.B && oy < p.PH && ox < p.PW)
            v = load_piece<T>(Pg, (((int64_t)b * p.PH + oy) * p.PW + ox) * p.p_cs + chP, chP, p.Ca, p_vec);
        return v;
    };
    auto fetchQ = [&](const TileC& c, unsigned d) -> u32x4 {
        u32x4 v = {0u, 0u, 0u, 0u};
        if (d == 0xffffffffu) return v;
        int iy = (c.tyi << p.th_log2) * p.q_step + p.min_dy + (int)((d >> 8) & 255u);
        int ix = (c.txi << p.tw_log2) * p.q_step + p.min_dx + (int)(d & 255u);
        const int b = c.tbi * p.nb + (int)(d >> 16);
        bool valid = b < p.B;
        if (p.pad_mode) { iy = min(max(iy, 0), p.QH - 1); ix = min(max(ix, 0), p.QW - 1); }
        else valid = valid && iy >= 0 && iy < p.QH && ix >= 0 && ix < p.QW;
        if (valid) v = load_piece<T>(Qg, (((int64_t)b * p.QH + iy) * p.QW + ix) * p.q_cs + chQ, chQ, p.Cb, q_vec);
        return v;
    };
    auto lds_p = [&](int q) -> u32x4* { return reinterpret_cast<u32x4*>(sP + (q / PPR) * ROWB + pcx * 16); };
    auto lds_q = [&](int q) -> u32x4* { return reinterpret_cast<u32x4*>(sQ + (q / PPR) * ROWB + pcx * 16); };

    int tob[NT];                                                // tap offsets in LDS bytes (uniform)
#pragma unroll
    for (int t = 0; t < NT; ++t) tob[t] = p.tap_off[t] * ROWB;  // the plan repeats tap 0 in the slots ntaps..NT-1 (never stored)

    auto compute_tile = [&]() {
        if constexpr (sizeof(T) == 4) {
            // f32: v_mfma_f32_32x32x2_f32, A[i=a][k=pixel], B[k=pixel][j=b]; one dword per lane per operand.
            const int khalf = lane >> 5, l31 = lane & 31;
            // K-split (round 4): a layer with <= 32 output or input channels fills a quarter / half of the 64 x 64 block and the exact-f32
            // MFMA takes 64 cycles per 2 pixels - the waves of the empty quadrants take a share of the k-steps of the real one instead
            const int ks = p.ksplit;
            const int wa_e = (ks == 4 || ks == 2) ? 0 : wa, wb_e = (ks == 4 || ks == 3) ? 0 : wb;
            const int kmod = ks == 4 ? 3 : (ks ? 1 : 0), kidx = ks == 4 ? wave : (ks == 2 ? wa : (ks == 3 ? wb : 0));
            const int aoff = (wa_e * 32 + l31) * 4, boff = (wb_e * 32 + l31) * 4;
            for (int k0 = 0; k0 < BMP; k0 += 2) {
                if (((k0 >> 1) & kmod) != kidx) continue;
                const int m = k0 + khalf;
                const int tx = m & ((1 << p.tw_log2) - 1);
                const int ty = (m >> p.tw_log2) & ((1 << p.th_log2) - 1);
                const int bl = m >> (p.tw_log2 + p.th_log2);
                const int qb = (bl * hhw + ty * p.q_step * p.hw + tx * p.q_step) * ROWB + boff;
                const float av = *reinterpret_cast<const float*>(sP + m * ROWB + aoff);
                float bv[NT];
#pragma unroll
                for (int t = 0; t < NT; ++t) bv[t] = *reinterpret_cast<const float*>(sQ + qb + tob[t]);
#pragma unroll
                for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv[t], acc[t], 0, 0, 0);
            }
        } else {
            // bf16: v_mfma_f32_32x32x16_bf16 needs 8 k(=pixel)-consecutive values per lane while LDS rows are
            // channel-contiguous: ds_read_b64_tr_b16 transposes a [4 pixel][16 channel] block per 16-lane group.
            // All 2 + 2 NT transposed reads of a k-step are issued before the first MFMA (no control flow in between).
            typedef short s16x4 __attribute__((ext_vector_type(4)));
            typedef short s16x8 __attribute__((ext_vector_type(8)));
            typedef __attribute__((address_space(3))) s16x4* lds_s16x4_ptr;
            const int khalf = lane >> 5;
            const int g16 = (lane >> 4) & 1;                     // which 16-row half of the 32-row operand
            const int i16 = lane & 15;
            const int prow = i16 >> 2;                           // pixel within the k-quad this lane fetches
            const int pcol = (i16 & 3) * 4;                      // channel offset of its 4 contiguous elements
            const int acol = (wa * 32 + g16 * 16 + pcol) * 2;
            const int bcol = (wb * 32 + g16 * 16 + pcol) * 2;
            for (int k0 = 0; k0 < BMP; k0 += 16) {
                int pa[2], qb[2];
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int m = k0 + khalf * 8 + h * 4 + prow;
                    const int tx = m & ((1 << p.tw_log2) - 1);
                    const int ty = (m >> p.tw_log2) & ((1 << p.th_log2) - 1);
                    const int bl = m >> (p.tw_log2 + p.th_log2);
                    pa[h] = m * ROWB + acol;
                    qb[h] = (bl * hhw + ty * p.q_step * p.hw + tx * p.q_step) * ROWB + bcol;
                }
                const s16x4 alo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(sP + pa[0]));
                const s16x4 ahi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(sP + pa[1]));
                s16x4 blo[NT], bhi[NT];
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    blo[t] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(sQ + qb[0] + tob[t]));
                    bhi[t] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(sQ + qb[1] + tob[t]));
                }
                const s16x8 av = {alo[0], alo[1], alo[2], alo[3], ahi[0], ahi[1], ahi[2], ahi[3]};
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    const s16x8 bv = {blo[t][0], blo[t][1], blo[t][2], blo[t][3], bhi[t][0], bhi[t][1], bhi[t][2], bhi[t][3]};
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, av), __builtin_bit_cast(bf16x8, bv), acc[t], 0, 0, 0);
                }
            }
        }
    };

    if (PIPE && nq <= MAXQ * 256) {
        // software pipeline: next tile's global loads fly while the matrix cores work on the current one.
        // Per piece only tile-invariant lane constants are kept (packed coordinates for the bounds test, a 32-bit element offset
        // relative to the tile); per tile the origin is a handful of uniform values - no per-piece 64-bit index arithmetic.
        unsigned dp[MAXP], dq[MAXQ];
        int offP[MAXP], offQ[MAXQ];
        const int rowP = p.PW * p.p_cs, rowQ = p.QW * p.q_cs;
#pragma unroll
        for (int k = 0; k < MAXP; ++k) {
            dp[k] = descP(tid + (k << 8));
            const int bl = (int)(dp[k] >> 16), ty = (int)((dp[k] >> 8) & 255u), tx = (int)(dp[k] & 255u);
            offP[k] = (bl * p.PH + ty) * rowP + tx * p.p_cs + chP;
        }
#pragma unroll
        for (int k = 0; k < MAXQ; ++k) {
            dq[k] = descQ(tid + (k << 8));
            offQ[k] = (int)(dq[k] >> 16) * p.QH * rowQ + chQ;                 // image part only: rows / columns may be clamped
        }
        u32x4 rp[MAXP], rq[MAXQ];
        auto load_tile = [&](const TileC& c) {
            const int limB = p.B - c.tbi * p.nb, limY = p.PH - (c.tyi << p.th_log2), limX = p.PW - (c.txi << p.tw_log2);
            const T* baseP = Pg + (((int64_t)c.tbi * p.nb * p.PH + (c.tyi << p.th_log2)) * p.PW + (c.txi << p.tw_log2)) * p.p_cs;
            const T* baseQ = Qg + (int64_t)c.tbi * p.nb * p.QH * rowQ;
            const int iy0 = (c.tyi << p.th_log2) * p.q_step + p.min_dy, ix0 = (c.txi << p.tw_log2) * p.q_step + p.min_dx;
#pragma unroll
            for (int k = 0; k < MAXP; ++k) {
                rp[k] = u32x4{0u, 0u, 0u, 0u};
                const unsigned d = dp[k];
                if (d != 0xffffffffu && (int)(d >> 16) < limB && (int)((d >> 8) & 255u) < limY && (int)(d & 255u) < limX)
                    rp[k] = load_piece<T>(baseP, offP[k], chP, p.Ca, p_vec);
            }
#pragma unroll
            for (int k = 0; k < MAXQ; ++k) {
                rq[k] = u32x4{0u, 0u, 0u, 0u};
                const unsigned d = dq[k];
                if (d == 0xffffffffu) continue;
                int iy = iy0 + (int)((d >> 8) & 255u), ix = ix0 + (int)(d & 255u);
                bool valid = (int)(d >> 16) < limB;
                if (p.pad_mode) { iy = min(max(iy, 0), p.QH - 1); ix = min(max(ix, 0), p.QW - 1); }
                else valid = valid && (unsigned)iy < (unsigned)p.QH && (unsigned)ix < (unsigned)p.QW;
                if (valid) rq[k] = load_piece<T>(baseQ, offQ[k] + iy * rowQ + ix * p.q_cs, chQ, p.Cb, q_vec);
            }
        };
        TileC cur = walk.decode(split);
        if (split < p.ntiles) load_tile(cur);
        for (int tile = split; tile < p.ntiles; tile += p.nsplit) {
            __syncthreads();
#pragma unroll
            for (int k = 0; k < MAXP; ++k) { const int q = tid + (k << 8); if (q < np) *lds_p(q) = rp[k]; }
#pragma unroll
            for (int k = 0; k < MAXQ; ++k) { const int q = tid + (k << 8); if (q < nq) *lds_q(q) = rq[k]; }
            __syncthreads();
            walk.advance(cur);
            if (tile + p.nsplit < p.ntiles) load_tile(cur);
            compute_tile();
        }
    } else {
        TileC cur = walk.decode(split);
        for (int tile = split; tile < p.ntiles; tile += p.nsplit) {
            __syncthreads();
            for (int q = tid; q < np; q += 256) *lds_p(q) = fetchP(cur, descP(q));
            for (int q = tid; q < nq; q += 256) *lds_q(q) = fetchQ(cur, descQ(q));
            __syncthreads();
            compute_tile();
            walk.advance(cur);
        }
    }
    // K-split (fp32): the waves that shared a channel block meet in LDS tap by tap, fixed order (leader + partner 1 [+ 2 + 3])
    int wa_o = wa, wb_o = wb;
    bool leader = true;
    if (sizeof(T) == 4 && p.ksplit) {
        const int ks = p.ksplit;
        const int step = ks == 4 ? 1 : (ks == 2 ? 2 : 1), cnt = ks == 4 ? 4 : 2;          // partners of leader w: w + step, w + 2 step, ...
        leader = ks == 4 ? wave == 0 : (ks == 2 ? wa == 0 : wb == 0);
        wa_o = (ks == 4 || ks == 2) ? 0 : wa; wb_o = (ks == 4 || ks == 3) ? 0 : wb;
        float* red = reinterpret_cast<float*>(smem);                                       // [wave][16][64] floats: 4 KB per wave
        __syncthreads();                                                                   // every wave is done with the tile buffers
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            if (!leader) {
#pragma unroll
                for (int r = 0; r < 16; ++r) red[(wave * 16 + r) * 64 + lane] = acc[t][r];
            }
            __syncthreads();
            if (leader) {
                for (int q = 1; q < cnt; ++q) {
                    const int w2 = wave + q * step;
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[t][r] += red[(w2 * 16 + r) * 64 + lane];
                }
            }
            __syncthreads();
        }
    }
    // write the partial slab: partials[split][t][a][b]
    const int khalf = lane >> 5, l31 = lane & 31;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        if (t < p.ntaps && leader) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int a = a0 + wa_o * 32 + (r & 3) + 8 * (r >> 2) + 4 * khalf;
                const int b = c0 + wb_o * 32 + l31;
                if (a < p.Ca && b < p.Cb) {
                    float* d = p.partials + (((int64_t)split * p.ntaps + t) * p.Ca + a) * p.Cb + b;
                    *d = acc[t][r];
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------ weight gradient, fast path
// Same decomposition and partial-slab format as conv_wgrad_kernel, for the shapes that dominate training: bf16, 3x3 (NT taps in
// one launch), KS*16-pixel K tiles, 16-byte aligned views whose channel counts are multiples of 8, halo of at most MAXQ*256
// pieces (the host checks all of it).  A weight-gradient workgroup is alone on its CU (144 accumulator registers per lane), so
// nothing hides latency unless the instruction stream does it itself:
//   * the k-step loop is fully unrolled and software pipelined: the transposed LDS reads of k-step j+1 and the global loads of
//     the NEXT pixel tile are issued between the MFMAs of k-step j (sched_group_barrier pins the interleave);
//   * the loader is branch free: a masked-out piece loads 16 zero bytes from g_wg_zero instead of zero-initialising its
//     destination registers (which made the compiler wait for the loads already in flight) - per piece a few VALU instructions;
//   * the MFMA operands are swapped (D^T): a lane then owns 4 consecutive b-channels of one a-row, the slab is written with
//     16-byte stores instead of 4-byte ones.
template <int NT, int KS, bool PAD>
__global__ __launch_bounds__(256) void conv_wgrad_fast_kernel(WgradKP p) {
    typedef bf16_t T;
    constexpr int PPR = 8, ROWB = 192, BMP = KS * 16;
    constexpr int MAXP = BMP * PPR / 256, MAXQ = 10, NPIECE = MAXP + MAXQ;
    constexpr int LSTEPS = KS / 2;                               // the next tile's loads are issued during the first k-steps
    constexpr int LPS = (NPIECE + LSTEPS - 1) / LSTEPS;
    typedef short s16x4 __attribute__((ext_vector_type(4)));
    typedef short s16x8 __attribute__((ext_vector_type(8)));
    typedef __attribute__((address_space(3))) s16x4* lds_s16x4_ptr;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* sP = smem;
    unsigned char* sQ = smem + BMP * ROWB;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wa = wave >> 1, wb = wave & 1;
    const WgBlock<T> w = wg_block<T>(p);
    const int split = w.split, a0 = w.a0, c0 = w.c0;
    const int hhw = w.hhw, phalo = p.nb * hhw;
    const T* zp = reinterpret_cast<const T*>(g_wg_zero);

    f32x16 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

    const TileWalk walk(p);

    // ---- tile-invariant piece constants.  Piece q = tid + 256 k is 16 bytes (8 channels) of pixel row q / 8.
    const int pcx = tid % PPR;
    const int chP = a0 + pcx * 8, chQ = c0 + pcx * 8;
    const int np = BMP * PPR, nq = phalo * PPR;
    const int rowP = p.PW * p.p_cs, rowQ = p.QW * p.q_cs;
    int offP[MAXP], pby[MAXP], pxx[MAXP];                          // element offset in the tile, (image << 8 | row), column
    int offQ[MAXQ], hyq[MAXQ], hxq[MAXQ], blq[MAXQ];
#pragma unroll
    for (int k = 0; k < MAXP; ++k) {
        const int q = tid + (k << 8), m = q / PPR;
        const int tx = m & ((1 << p.tw_log2) - 1), ty = (m >> p.tw_log2) & ((1 << p.th_log2) - 1), bl = m >> (p.tw_log2 + p.th_log2);
        const bool ok = q < np && chP < p.Ca;
        offP[k] = (bl * p.PH + ty) * rowP + tx * p.p_cs + chP;
        pby[k] = ok ? bl : (1 << 20); pxx[k] = tx | (ty << 16);
    }
#pragma unroll
    for (int k = 0; k < MAXQ; ++k) {
        const int q = tid + (k << 8), pix = q / PPR;
        const int bl = pix / hhw, r = pix - bl * hhw, hy = r / p.hw, hx = r - hy * p.hw;
        const bool ok = q < nq && chQ < p.Cb;
        blq[k] = ok ? bl : (1 << 20);                                // fails "image < limB" for every tile
        hyq[k] = hy; hxq[k] = hx;
        offQ[k] = bl * p.QH * rowQ + chQ + (PAD ? 0 : hy * rowQ + hx * p.q_cs);
    }
    u32x4 rp[MAXP], rq[MAXQ];
    typedef TileCtx<T> Ctx;
    auto make_ctx = [&](const TileC& c, bool live) { return tile_ctx<T, PAD>(p, w, rowQ, c, live); };
    auto issue_piece = [&](int K, const Ctx& x) {                // K is a constant after unrolling
        if (K < MAXP) {
            const int k = K;
            const bool ok = pby[k] < x.limB && (pxx[k] >> 16) < x.limY && (pxx[k] & 0xffff) < x.limX;
            rp[k] = *reinterpret_cast<const u32x4*>(ok ? x.baseP + offP[k] : zp);
        } else {
            const int k = K - MAXP;
            if (!PAD) {
                const bool ok = (unsigned)(x.iy0 + hyq[k]) < (unsigned)p.QH && (unsigned)(x.ix0 + hxq[k]) < (unsigned)p.QW && blq[k] < x.limB;
                rq[k] = *reinterpret_cast<const u32x4*>(ok ? x.baseQ + offQ[k] : zp);
            } else {
                const int iy = min(max(x.iy0 + hyq[k], 0), p.QH - 1), ix = min(max(x.ix0 + hxq[k], 0), p.QW - 1);
                rq[k] = *reinterpret_cast<const u32x4*>(blq[k] < x.limB ? x.baseQ + (offQ[k] + iy * rowQ + ix * p.q_cs) : zp);
            }
        }
    };

    // ---- fragment addressing: ds_read_b64_tr_b16 transposes a [4 pixel][16 channel] block per 16-lane group (conv_wgrad_kernel)
    const int khalf = lane >> 5, g16 = (lane >> 4) & 1, i16 = lane & 15, prow = i16 >> 2, pcol = (i16 & 3) * 4;
    const int pa_base = (khalf * 8 + prow) * ROWB + (wa * 32 + g16 * 16 + pcol) * 2;     // + (16 j + 4 h) rows: an immediate
    int qaddr[KS * 2];                                                // halo-row byte address of pixel 16 j + 8 khalf + 4 h + prow
#pragma unroll
    for (int i = 0; i < KS * 2; ++i) {
        const int m = (i >> 1) * 16 + khalf * 8 + (i & 1) * 4 + prow;
        const int tx = m & ((1 << p.tw_log2) - 1), ty = (m >> p.tw_log2) & ((1 << p.th_log2) - 1), bl = m >> (p.tw_log2 + p.th_log2);
        qaddr[i] = (bl * hhw + ty * p.q_step * p.hw + tx * p.q_step) * ROWB + (wb * 32 + g16 * 16 + pcol) * 2;
    }
    int tob[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) tob[t] = p.tap_off[t] * ROWB;
    struct Frag { s16x4 alo, ahi, blo[NT], bhi[NT]; };
    auto read_frags = [&](int j, Frag& fr) {
        fr.alo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(sP + pa_base + (j * 16) * ROWB));
        fr.ahi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(sP + pa_base + (j * 16 + 4) * ROWB));
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            fr.blo[t] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(sQ + qaddr[2 * j] + tob[t]));
            fr.bhi[t] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(sQ + qaddr[2 * j + 1] + tob[t]));
        }
    };
    auto b_operand = [&](const Frag& fr, int t) -> bf16x8 {
        const s16x8 bv = {fr.blo[t][0], fr.blo[t][1], fr.blo[t][2], fr.blo[t][3], fr.bhi[t][0], fr.bhi[t][1], fr.bhi[t][2], fr.bhi[t][3]};
        return __builtin_bit_cast(bf16x8, bv);
    };

    TileC cur = walk.decode(split);
    {
        const Ctx x = make_ctx(cur, split < p.ntiles);
#pragma unroll
        for (int K = 0; K < NPIECE; ++K) issue_piece(K, x);
    }
    Frag f0, f1;
    for (int tile = split; tile < p.ntiles; tile += p.nsplit) {
        __syncthreads();
#pragma unroll
        for (int k = 0; k < MAXP; ++k) { const int q = tid + (k << 8); if (q < np) *reinterpret_cast<u32x4*>(sP + (q / PPR) * ROWB + pcx * 16) = rp[k]; }
#pragma unroll
        for (int k = 0; k < MAXQ; ++k) { const int q = tid + (k << 8); if (q < nq) *reinterpret_cast<u32x4*>(sQ + (q / PPR) * ROWB + pcx * 16) = rq[k]; }
        __syncthreads();
        walk.advance(cur);
        const Ctx x = make_ctx(cur, tile + p.nsplit < p.ntiles);
        read_frags(0, f0);
#pragma unroll
        for (int j = 0; j < KS; ++j) {
            Frag& fc = (j & 1) ? f1 : f0;
            Frag& fn = (j & 1) ? f0 : f1;
            if (j + 1 < KS) read_frags(j + 1, fn);
            int nld = 0;
            if (j < LSTEPS) {
#pragma unroll
                for (int u = 0; u < LPS; ++u)
                    if (j * LPS + u < NPIECE) { issue_piece(j * LPS + u, x); ++nld; }
            }
            const s16x8 av = {fc.alo[0], fc.alo[1], fc.alo[2], fc.alo[3], fc.ahi[0], fc.ahi[1], fc.ahi[2], fc.ahi[3]};
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const bf16x8 bv = b_operand(fc, t);
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bv, __builtin_bit_cast(bf16x8, av), acc[t], 0, 0, 0);
            }
            if (j + 1 < KS) {                                        // pin: 2 LDS reads (+ a global load) behind every MFMA
                __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
                    if (t < nld) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
                }
            }
        }
    }
    // ---- partial slab partials[split][t][a][b]
    const int a = a0 + wa * 32 + (lane & 31);
#pragma unroll
    for (int t = 0; t < NT; ++t)
        if (t < p.ntaps && a < p.Ca) slab_store(p, w, acc[t], t, a, wb, khalf);
}

// 8-wave 3x3 weight gradient on row tiles: every k-step is one 16-pixel tile row (tw = 16, th = 8, one image per tile, 18-pixel
// halo rows, unit step), so the halo address of a fragment read is a per-row lane constant plus a compile-time multiple of the
// halo row - no address arithmetic.  The workgroup tile, LDS layout, branch-free loader and slab stores are those of
// conv_wgrad_fast_kernel, but two waves share a SIMD - waves 0-3 accumulate taps 0-4, waves 4-7 taps 5-8 (80 / 64 accumulator
// registers per lane instead of 144) - so that one wave's VMEM / LDS issue stalls (a global_load_dwordx4 costs ~115 cycles of
// issue time) overlap with the other wave's MFMAs.  The three taps of a kernel row read overlapping pixel runs, so one run of
// 12 pixels (three transposed quads per lane) serves all three: tap dx is the run shifted by dx pixels = dx 16-bit elements
// (dx = 1: four v_alignbit, dx = 2: a register offset).  Each half reads the runs of the two kernel rows its taps touch (8 LDS
// reads per k-step; the LDS return path, not the MFMA, bounds this kernel) and moves half of the tile pieces.
template <bool PAD>
__global__ __launch_bounds__(512) void conv_wgrad_fast8_kernel(WgradKP p) {
    typedef bf16_t T;
    constexpr int KS = 8, NTH = 512, PPR = 8, ROWB = 192, BMP = KS * 16, NTA = 5;
    constexpr int MAXP = BMP * PPR / NTH, MAXQ = 5, NPIECE = MAXP + MAXQ;
    constexpr int LSTEPS = KS / 2, LPS = (NPIECE + LSTEPS - 1) / LSTEPS;
    typedef short s16x4 __attribute__((ext_vector_type(4)));
    typedef short s16x8 __attribute__((ext_vector_type(8)));
    typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
    typedef __attribute__((address_space(3))) s16x4* lds_s16x4_ptr;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* sP = smem;
    unsigned char* sQ = smem + BMP * ROWB;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int grp = wave >> 2, wa = (wave >> 1) & 1, wb = wave & 1;
    const WgBlock<T> w = wg_block<T>(p);
    const int split = w.split, a0 = w.a0, c0 = w.c0;
    const int hhw = w.hhw, phalo = p.nb * hhw;
    const T* zp = reinterpret_cast<const T*>(g_wg_zero);

    f32x16 acc[NTA];
#pragma unroll
    for (int t = 0; t < NTA; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

    const TileWalk walk(p);

    // ---- tile-invariant piece constants.  Piece q = tid + 512 k is 16 bytes (8 channels) of pixel row q / 8.
    const int pcx = tid % PPR;
    const int chP = a0 + pcx * 8, chQ = c0 + pcx * 8;
    const int np = BMP * PPR, nq = phalo * PPR;
    const int rowP = p.PW * p.p_cs, rowQ = p.QW * p.q_cs;
    int offP[MAXP], pby[MAXP], pxx[MAXP];
    int offQ[MAXQ], hyq[MAXQ], hxq[MAXQ], blq[MAXQ];
#pragma unroll
    for (int k = 0; k < MAXP; ++k) {
        const int q = tid + k * NTH, m = q / PPR;
        const int tx = m & ((1 << p.tw_log2) - 1), ty = (m >> p.tw_log2) & ((1 << p.th_log2) - 1), bl = m >> (p.tw_log2 + p.th_log2);
        const bool ok = q < np && chP < p.Ca;
        offP[k] = (bl * p.PH + ty) * rowP + tx * p.p_cs + chP;
        pby[k] = ok ? bl : (1 << 20); pxx[k] = tx | (ty << 16);
    }
#pragma unroll
    for (int k = 0; k < MAXQ; ++k) {
        const int q = tid + k * NTH, pix = q / PPR;
        const int bl = pix / hhw, r = pix - bl * hhw, hy = r / p.hw, hx = r - hy * p.hw;
        const bool ok = q < nq && chQ < p.Cb;
        blq[k] = ok ? bl : (1 << 20);
        hyq[k] = hy; hxq[k] = hx;
        offQ[k] = bl * p.QH * rowQ + chQ + (PAD ? 0 : hy * rowQ + hx * p.q_cs);
    }
    u32x4 rp[MAXP], rq[MAXQ];
    typedef TileCtx<T> Ctx;
    auto make_ctx = [&](const TileC& c, bool live) { return tile_ctx<T, PAD>(p, w, rowQ, c, live); };
    auto issue_piece = [&](int K, const Ctx& x) {
        if (K < MAXP) {
            const int k = K;
            const bool ok = pby[k] < x.limB && (pxx[k] >> 16) < x.limY && (pxx[k] & 0xffff) < x.limX;
            rp[k] = *reinterpret_cast<const u32x4*>(ok ? x.baseP + offP[k] : zp);
        } else {
            const int k = K - MAXP;
            if (!PAD) {
                const bool ok = (unsigned)(x.iy0 + hyq[k]) < (unsigned)p.QH && (unsigned)(x.ix0 + hxq[k]) < (unsigned)p.QW && blq[k] < x.limB;
                rq[k] = *reinterpret_cast<const u32x4*>(ok ? x.baseQ + offQ[k] : zp);
            } else {
                const int iy = min(max(x.iy0 + hyq[k], 0), p.QH - 1), ix = min(max(x.ix0 + hxq[k], 0), p.QW - 1);
                rq[k] = *reinterpret_cast<const u32x4*>(blq[k] < x.limB ? x.baseQ + (offQ[k] + iy * rowQ + ix * p.q_cs) : zp);
            }
        }
    };

    // ---- fragment addressing: this wave half reads the 12-pixel runs of kernel rows grp and grp + 1
    const int khalf = lane >> 5, g16 = (lane >> 4) & 1, i16 = lane & 15, prow = i16 >> 2, pcol = (i16 & 3) * 4;
    const int pa_base = (khalf * 8 + prow) * ROWB + (wa * 32 + g16 * 16 + pcol) * 2;
    int tq[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) tq[i] = (khalf * 8 + prow) * ROWB + (wb * 32 + g16 * 16 + pcol) * 2 + (grp + i) * (18 * ROWB);
    struct Frag { s16x4 alo, ahi; u32x2 q[2][3]; };
    auto read_frags = [&](int j, Frag& fr) {
        fr.alo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(sP + pa_base + (j * 16) * ROWB));
        fr.ahi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(sP + pa_base + (j * 16 + 4) * ROWB));
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int u = 0; u < 3; ++u)
                fr.q[i][u] = __builtin_bit_cast(u32x2, __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(sQ + tq[i] + (j * 18 + u * 4) * ROWB)));
    };
    auto b_operand = [&](const Frag& fr, int row, int dx) -> bf16x8 {       // row, dx constants after unrolling
        const unsigned w0 = fr.q[row][0].x, w1 = fr.q[row][0].y, w2 = fr.q[row][1].x, w3 = fr.q[row][1].y, w4 = fr.q[row][2].x;
        u32x4 v;
        if (dx == 0) v = u32x4{w0, w1, w2, w3};
        else if (dx == 1) v = u32x4{__builtin_amdgcn_alignbit(w1, w0, 16), __builtin_amdgcn_alignbit(w2, w1, 16),
                                    __builtin_amdgcn_alignbit(w3, w2, 16), __builtin_amdgcn_alignbit(w4, w3, 16)};
        else v = u32x4{w1, w2, w3, w4};
        return __builtin_bit_cast(bf16x8, v);
    };
    Frag f0, f1;
    // the k-steps of one tile for wave half G (taps 5 G ... 5 G + CNT - 1): static register indices need G at compile time
    auto ksteps = [&](auto gc, const Ctx& x) {
        constexpr int G = decltype(gc)::value, CNT = G ? 4 : 5;
        read_frags(0, f0);
#pragma unroll
        for (int j = 0; j < KS; ++j) {
            Frag& fc = (j & 1) ? f1 : f0;
            Frag& fn = (j & 1) ? f0 : f1;
            if (j + 1 < KS) read_frags(j + 1, fn);
            int nld = 0;
            if (j < LSTEPS) {
#pragma unroll
                for (int u = 0; u < LPS; ++u)
                    if (j * LPS + u < NPIECE) { issue_piece(j * LPS + u, x); ++nld; }
            }
            const s16x8 av = {fc.alo[0], fc.alo[1], fc.alo[2], fc.alo[3], fc.ahi[0], fc.ahi[1], fc.ahi[2], fc.ahi[3]};
#pragma unroll
            for (int tl = 0; tl < CNT; ++tl) {
                const int t = G * 5 + tl;
                acc[tl] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(b_operand(fc, t / 3 - G, t % 3), __builtin_bit_cast(bf16x8, av), acc[tl], 0, 0, 0);
            }
            if (j + 1 < KS) {                                        // pin: the 8 LDS reads (+ the global loads) between the MFMAs
                __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
#pragma unroll
                for (int tl = 0; tl < CNT; ++tl) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    if (tl < 6 - CNT) __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
                    else __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                    if (tl < nld) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
                }
            }
        }
    };

    TileC cur = walk.decode(split);
    {
        const Ctx x = make_ctx(cur, split < p.ntiles);
#pragma unroll
        for (int K = 0; K < NPIECE; ++K) issue_piece(K, x);
    }
    for (int tile = split; tile < p.ntiles; tile += p.nsplit) {
        __syncthreads();
#pragma unroll
        for (int k = 0; k < MAXP; ++k) { const int q = tid + k * NTH; if (q < np) *reinterpret_cast<u32x4*>(sP + (q / PPR) * ROWB + pcx * 16) = rp[k]; }
#pragma unroll
        for (int k = 0; k < MAXQ; ++k) { const int q = tid + k * NTH; if (q < nq) *reinterpret_cast<u32x4*>(sQ + (q / PPR) * ROWB + pcx * 16) = rq[k]; }
        __syncthreads();
        walk.advance(cur);
        const Ctx x = make_ctx(cur, tile + p.nsplit < p.ntiles);
        if (grp == 0) ksteps(std::integral_constant<int, 0>{}, x);     // wave-uniform: no barrier inside
        else ksteps(std::integral_constant<int, 1>{}, x);
    }
    // ---- partial slab partials[split][t][a][b]: this wave half's taps 5 grp ...
    const int a = a0 + wa * 32 + (lane & 31);
    const int cnt = grp ? 4 : 5;
#pragma unroll
    for (int tl = 0; tl < NTA; ++tl)
        if (tl < cnt && a < p.Ca) slab_store(p, w, acc[tl], grp * 5 + tl, a, wb, khalf);
}

// fp32 3x3 weight gradient on row tiles (tw = 16, th = 8, one image per tile, 18-pixel halo rows, unit step; exact fp32: v_mfma_f32_32x32x2_f32, two pixels per k-step, 64 k-steps per 128-pixel tile).
// LDS rows are 64 channels x 4 B; a fragment read is one dword per lane (lanes = consecutive channels: conflict free) at a per-tap
// lane constant plus a compile-time offset of the k-step, so the unrolled loop has no address arithmetic; the branch-free loader and
// the 16-byte slab stores are those of conv_wgrad_fast_kernel.  The generic kernel spent ~34 us per tile here, most of it on one
// global load in flight at a time.
// KSPLIT / SIDE: a layer with <= 32 output or input channels fills a quarter / half of the 64 x 64 channel block, and the exact-f32
// MFMA (64 cycles for K = 2) makes the idle waves expensive (vanilla U-Net, 16-64 channels: 200 us per launch whatever the layer).
// KSPLIT = 4 (both sides <= 32): all four waves work on the SAME 32 x 32 channel block and take a quarter of the tile's 64 k-steps
// each; KSPLIT = 2 (SIDE 0: the a side <= 32, SIDE 1: the b side <= 32): the two waves that would idle split the k-steps with their
// partners.  The partial accumulators meet in LDS after the tile loop (fixed order: k-slice 0 + 1 + 2 + 3).
template <bool PAD, int KSPLIT = 1, int SIDE = 0>
__global__ __launch_bounds__(256) void conv_wgrad_fast32_kernel(WgradKP p) {
    typedef float T;
    constexpr int NT = 9, KS = 64, PPR = 16, ROWB = 256, BMP = 128;
    constexpr int JN = KS / KSPLIT;                                   // k-steps per wave and tile
    constexpr int MAXP = BMP * PPR / 256, MAXQ = 12, NPIECE = MAXP + MAXQ;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* sP = smem;
    unsigned char* sQ = smem + BMP * ROWB;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // wave roles: channel sub-block (wa, wb) and k-slice ks
    const int wa = KSPLIT == 4 ? 0 : (KSPLIT == 2 && SIDE == 0 ? 0 : wave >> 1);
    const int wb = KSPLIT == 4 ? 0 : (KSPLIT == 2 && SIDE == 1 ? 0 : wave & 1);
    const int ks = KSPLIT == 4 ? wave : (KSPLIT == 2 ? (SIDE == 0 ? wave >> 1 : wave & 1) : 0);
    const WgBlock<T> w = wg_block<T>(p);
    const int split = w.split, a0 = w.a0, c0 = w.c0;
    const int hhw = w.hhw, phalo = p.nb * hhw;
    const T* zp = reinterpret_cast<const T*>(g_wg_zero);

    f32x16 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

    const TileWalk walk(p);

    // ---- tile-invariant piece constants.  Piece q = tid + 256 k is 16 bytes (4 channels) of pixel row q / 16.
    const int pcx = tid % PPR;
    const int chP = a0 + pcx * 4, chQ = c0 + pcx * 4;
    const int np = BMP * PPR, nq = phalo * PPR;
    const int rowP = p.PW * p.p_cs, rowQ = p.QW * p.q_cs;
    int offP[MAXP], offQ[MAXQ];
    unsigned dp[MAXP], dq[MAXQ];                                      // packed (image << 16 | row << 8 | column); 0xffffffff: no piece
#pragma unroll
    for (int k = 0; k < MAXP; ++k) {
        const int q = tid + (k << 8), m = q / PPR;
        const int tx = m & 15, ty = (m >> 4) & 7, bl = m >> 7;
        const bool ok = q < np && chP < p.Ca;
        offP[k] = (bl * p.PH + ty) * rowP + tx * p.p_cs + chP;
        dp[k] = ok ? (unsigned)((bl << 16) | (ty << 8) | tx) : 0xffffffffu;
    }
#pragma unroll
    for (int k = 0; k < MAXQ; ++k) {
        const int q = tid + (k << 8), pix = q / PPR;
        const int bl = pix / hhw, r = pix - bl * hhw, hy = r / p.hw, hx = r - hy * p.hw;
        const bool ok = q < nq && chQ < p.Cb;
        dq[k] = ok ? (unsigned)((bl << 16) | (hy << 8) | hx) : 0xffffffffu;
        offQ[k] = bl * p.QH * rowQ + chQ + (PAD ? 0 : hy * rowQ + hx * p.q_cs);
    }
    u32x4 rp[MAXP], rq[MAXQ];
    typedef TileCtx<T> Ctx;
    auto make_ctx = [&](const TileC& c, bool live) { return tile_ctx<T, PAD>(p, w, rowQ, c, live); };
    auto issue_piece = [&](int K, const Ctx& x) {
        if (K < MAXP) {
            const int k = K;
            const unsigned d = dp[k];
            const bool ok = (int)(d >> 16) < x.limB && (int)((d >> 8) & 255u) < x.limY && (int)(d & 255u) < x.limX;    // no piece: image 65535
            rp[k] = *reinterpret_cast<const u32x4*>(ok ? x.baseP + offP[k] : zp);
        } else {
            const int k = K - MAXP;
            const unsigned d = dq[k];
            const int bl = (int)(d >> 16), hy = (int)((d >> 8) & 255u), hx = (int)(d & 255u);
            if (!PAD) {
                const bool ok = (unsigned)(x.iy0 + hy) < (unsigned)p.QH && (unsigned)(x.ix0 + hx) < (unsigned)p.QW && bl < x.limB;
                rq[k] = *reinterpret_cast<const u32x4*>(ok ? x.baseQ + offQ[k] : zp);
            } else {
                const int iy = min(max(x.iy0 + hy, 0), p.QH - 1), ix = min(max(x.ix0 + hx, 0), p.QW - 1);
                rq[k] = *reinterpret_cast<const u32x4*>(bl < x.limB ? x.baseQ + (offQ[k] + iy * rowQ + ix * p.q_cs) : zp);
            }
        }
    };

    // ---- fragment addressing: k-step j covers pixels 2 j + khalf = (row j >> 3, column (2 j & 15) + khalf) of the 8 x 16 tile
    const int khalf = lane >> 5, l31 = lane & 31;
    // k-slice ks starts at k-step ks * JN = pixel row 2 ks JN of the tile (JN is a multiple of 8: whole 16-pixel tile rows)
    const int pa_lane = (khalf + 2 * JN * ks) * ROWB + (wa * 32 + l31) * 4;            // + 2 j rows: an immediate
    int qt[NT];                                                        // per-tap lane constant; + ((j >> 3) * 18 + (2 j & 15)) rows: an immediate
#pragma unroll
    for (int t = 0; t < NT; ++t) qt[t] = (khalf + p.tap_off[t] + (ks * JN / 8) * 18) * ROWB + (wb * 32 + l31) * 4;
    struct Frag { float a, b[NT]; };
    auto read_frags = [&](int j, Frag& fr) {
        fr.a = *reinterpret_cast<const float*>(sP + pa_lane + (2 * j) * ROWB);
#pragma unroll
        for (int t = 0; t < NT; ++t) fr.b[t] = *reinterpret_cast<const float*>(sQ + qt[t] + ((j >> 3) * 18 + ((2 * j) & 15)) * ROWB);
    };

    TileC cur = walk.decode(split);
    {
        const Ctx x = make_ctx(cur, split < p.ntiles);
#pragma unroll
        for (int K = 0; K < NPIECE; ++K) issue_piece(K, x);
    }
    Frag f0, f1;
    for (int tile = split; tile < p.ntiles; tile += p.nsplit) {
        __syncthreads();
#pragma unroll
        for (int k = 0; k < MAXP; ++k) { const int q = tid + (k << 8); if (q < np) *reinterpret_cast<u32x4*>(sP + (q / PPR) * ROWB + pcx * 16) = rp[k]; }
#pragma unroll
        for (int k = 0; k < MAXQ; ++k) { const int q = tid + (k << 8); if (q < nq) *reinterpret_cast<u32x4*>(sQ + (q / PPR) * ROWB + pcx * 16) = rq[k]; }
        __syncthreads();
        walk.advance(cur);
        const Ctx x = make_ctx(cur, tile + p.nsplit < p.ntiles);
        read_frags(0, f0);
        constexpr int LEVERY = JN >= 3 * NPIECE ? 3 : 1;              // next tile's 20 pieces: one every third k-step (every step when k is split)
        constexpr int LPS = (NPIECE * LEVERY + JN - 1) / JN;          // pieces per loading k-step
#pragma unroll
        for (int j = 0; j < JN; ++j) {
            Frag& fc = (j & 1) ? f1 : f0;
            Frag& fn = (j & 1) ? f0 : f1;
            if (j + 1 < JN) read_frags(j + 1, fn);
            const bool ld = (j % LEVERY == 0) && ((j / LEVERY) * LPS < NPIECE);
            if (ld) {
#pragma unroll
                for (int u = 0; u < LPS; ++u) if ((j / LEVERY) * LPS + u < NPIECE) issue_piece((j / LEVERY) * LPS + u, x);
            }
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(fc.b[t], fc.a, acc[t], 0, 0, 0);
            if (j + 1 < JN) {
                __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                    if (ld && t < LPS) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
                }
            }
        }
    }
    if constexpr (KSPLIT > 1) {
        // sum the k-slices of every (wa, wb) sub-block tap by tap through LDS: slice s > 0 parks its accumulator, slice 0 adds them in
        // ascending slice order.  Waves of the same sub-block: KSPLIT 4: all four; KSPLIT 2: the pair that shares (wa, wb).
        float* red = reinterpret_cast<float*>(smem);                  // [pair][slice - 1][16][64]
        const int pair = KSPLIT == 4 ? 0 : (SIDE == 0 ? (wave & 1) : (wave >> 1));
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            __syncthreads();                                           // tile loop / previous tap done with this LDS
            if (ks > 0) {
                float* dst = red + ((pair * (KSPLIT - 1) + ks - 1) * 16) * 64 + lane * 4;
#pragma unroll
                for (int g = 0; g < 4; ++g) *reinterpret_cast<f32x4*>(dst + g * 256) = f32x4{acc[t][4 * g], acc[t][4 * g + 1], acc[t][4 * g + 2], acc[t][4 * g + 3]};
            }
            __syncthreads();
            if (ks == 0) {
#pragma unroll
                for (int s2 = 1; s2 < KSPLIT; ++s2) {
                    const float* src = red + ((pair * (KSPLIT - 1) + s2 - 1) * 16) * 64 + lane * 4;
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const f32x4 v = *reinterpret_cast<const f32x4*>(src + g * 256);
                        acc[t][4 * g] += v.x; acc[t][4 * g + 1] += v.y; acc[t][4 * g + 2] += v.z; acc[t][4 * g + 3] += v.w;
                    }
                }
            }
        }
        if (ks > 0) return;
    }
    // ---- partial slab partials[split][t][a][b]
    const int a = a0 + wa * 32 + l31;
#pragma unroll
    for (int t = 0; t < NT; ++t)
        if (t < p.ntaps && a < p.Ca) slab_store(p, w, acc[t], t, a, wb, khalf);
}

int wgrad_plan(const salt_conv_wgrad_args* a, WgradKP* k, int* nsplit_out) {
    if (!a) SALT_FAIL(SALT_E_BADARG, "wgrad: null args");
    {
        salt_view qv = a->q;
        if (a->q_plane) {                         // planar q: planes of one 64-channel b-block
            if (a->q.cs != 64 || a->q.C % 64 || a->q_plane % 8 || a->q_plane < (int64_t)a->q.B * a->q.H * a->q.W * 64)
                SALT_FAIL(SALT_E_BADARG, "wgrad: q_plane needs dense planes of 64 channels");
            qv.cs = qv.C;
        }
        if (!view_ok(a->p) || !view_ok(qv)) SALT_FAIL(SALT_E_BADARG, "wgrad: bad view");
    }
    if (a->ntaps < 1 || a->ntaps > 9) SALT_FAIL(SALT_E_BADARG, "wgrad: ntaps %d (max 9 per launch)", a->ntaps);
    if (a->p.B != a->q.B) SALT_FAIL(SALT_E_BADARG, "wgrad: batch mismatch");
    const TapBox tb = tap_box(a->tap_dy, a->tap_dx, a->ntaps);
    const int min_dy = tb.min_dy, max_dy = tb.max_dy, min_dx = tb.min_dx, max_dx = tb.max_dx;
    const int rowb = a->dtype == SALT_F32 ? 256 : 192;
    int th = 1, tw = 1;
    for (int bmp = 128; bmp >= 32; bmp >>= 1) {
        k->bmp = bmp;
        k->tw_log2 = ilog2_ceil(a->p.W) < 4 ? ilog2_ceil(a->p.W) : 4;
        int rem = ilog2_ceil(bmp) - k->tw_log2;
        k->th_log2 = ilog2_ceil(a->p.H) < rem ? ilog2_ceil(a->p.H) : rem;
        k->nb = bmp >> (k->tw_log2 + k->th_log2);
        th = 1 << k->th_log2; tw = 1 << k->tw_log2;
        k->hh = (th - 1) * a->q_step + (max_dy - min_dy) + 1;
        k->hw = (tw - 1) * a->q_step + (max_dx - min_dx) + 1;
        if ((size_t)(bmp + k->nb * k->hh * k->hw) * rowb <= 80 * 1024) break;     // keep >= 2 workgroups per CU
    }
    k->P = a->p.p; k->Q = a->q.p; k->partials = a->partials;
    k->q_plane = a->q_plane; k->ksplit = 0;
    k->B = a->p.B; k->PH = a->p.H; k->PW = a->p.W; k->Ca = a->p.C; k->p_cs = a->p.cs;
    k->QH = a->q.H; k->QW = a->q.W; k->Cb = a->q.C; k->q_cs = a->q.cs;
    k->ntaps = a->ntaps; k->q_step = a->q_step; k->pad_mode = a->pad_mode; k->min_dy = min_dy; k->min_dx = min_dx;
    for (int t = 0; t < a->ntaps; ++t) k->tap_off[t] = (a->tap_dy[t] - min_dy) * k->hw + (a->tap_dx[t] - min_dx);
    for (int t = a->ntaps; t < SALT_MAX_TAPS; ++t) k->tap_off[t] = k->tap_off[0];      // padding slots of the NT-tap kernel instance
    k->tiles_y = cdiv(a->p.H, th); k->tiles_x = cdiv(a->p.W, tw);
    k->ntiles = cdiv(a->p.B, k->nb) * k->tiles_y * k->tiles_x;
    k->a_blocks = cdiv(a->p.C, 64); k->b_blocks = cdiv(a->q.C, 64);
    const WgradBudget bud = wgrad_split_budget(a->dtype);             // workgroups per launch, pixel tiles per split (common.h)
    const int min_tiles = bud.min_tiles;
    int ns = bud.target_wgs / (k->a_blocks * k->b_blocks);
    // the stem (64 x 16 channels, launched on the MAIN stream at the very end of backward, nothing left to overlap with): finer
    // split.  NOT for the other single-block layers: their launches share the chip with the data-gradient chain, and 256 instead
    // of 128 weight-gradient workgroups cost 6.17 -> 6.24 ms per step (and halving the tiles per split wherever a launch has fewer than
    // 256 workgroups 6.17 -> 6.30)
    const int mt = (k->a_blocks * k->b_blocks == 1 && a->q.C <= 16 && min_tiles >= 2) ? min_tiles / 2 : min_tiles;
    if (ns > k->ntiles / mt) ns = k->ntiles / mt;
    if (ns < 1) ns = 1;
    if (ns > k->ntiles) ns = k->ntiles;
    *nsplit_out = ns;
    k->nsplit = ns;
    return SALT_OK;
}

struct ReduceKP {
    const float* partials; float* grad; int nsplit, ntaps, Ca, Cb, KH, KW, accumulate;
    int ldb, a_mod;                                // slice of a wider tensor / tap-GEMM slab (salt_wgrad_reduce_args)
    int tap_kh[SALT_MAX_TAPS], tap_kw[SALT_MAX_TAPS];
};
// 256 threads = 4 split-rows x 64 consecutive slab elements: coalesced 256-B reads, 4x the parallelism of one thread
// per element (the slab is small - 36 K floats for a 64->64 3x3 - while nsplit can be 512), fixed summation order.
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(ReduceKP p) {
    __shared__ float sm[4][64];
    const int64_t slab = (int64_t)p.ntaps * p.Ca * p.Cb;
    const int e = threadIdx.x & 63, row = threadIdx.x >> 6;
    const int64_t i = (int64_t)blockIdx.x * 64 + e;
    float s0 = 0.f, s1 = 0.f;
    if (i < slab) {
        int k = row;
        for (; k + 4 < p.nsplit; k += 8) { s0 += p.partials[k * slab + i]; s1 += p.partials[(k + 4) * slab + i]; }
        for (; k < p.nsplit; k += 4) s0 += p.partials[k * slab + i];
    }
    sm[row][e] = s0 + s1;
    __syncthreads();
    if (row != 0 || i >= slab) return;
    const float s = sm[0][e] + sm[1][e] + sm[2][e] + sm[3][e];
    const int b = (int)(i % p.Cb);
    int64_t r = i / p.Cb;
    int a = (int)(r % p.Ca);
    int t = (int)(r / p.Ca);
    if (p.a_mod) { t = a / p.a_mod; a -= t * p.a_mod; }               // tap-GEMM slab: row = (tap, reference row)
    float* dst = p.grad + (((int64_t)a * p.ldb + b) * p.KH + p.tap_kh[t]) * p.KW + p.tap_kw[t];
    *dst = p.accumulate ? (*dst + s) : s;
}

// nsplit <= 8 (every 3x3 layer of the networks here): one thread per element with all split loads in flight, no LDS round trip;
// same summation order as wgrad_reduce_kernel for nsplit <= 8: (((v0 + v4) + (v1 + v5)) + (v2 + v6)) + (v3 + v7)
__global__ __launch_bounds__(256) void wgrad_reduce8_kernel(ReduceKP p) {
    const int64_t slab = (int64_t)p.ntaps * p.Ca * p.Cb;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= slab) return;
    float v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = k < p.nsplit ? p.partials[k * slab + i] : 0.f;
    const float s = (((v[0] + v[4]) + (v[1] + v[5])) + (v[2] + v[6])) + (v[3] + v[7]);
    const int b = (int)(i % p.Cb);
    int64_t r = i / p.Cb;
    int a = (int)(r % p.Ca);
    int t = (int)(r / p.Ca);
    if (p.a_mod) { t = a / p.a_mod; a -= t * p.a_mod; }               // tap-GEMM slab: row = (tap, reference row)
    float* dst = p.grad + (((int64_t)a * p.ldb + b) * p.KH + p.tap_kh[t]) * p.KW + p.tap_kw[t];
    *dst = p.accumulate ? (*dst + s) : s;
}

}  // namespace

extern "C" int salt_conv_wgrad_nsplit(const salt_conv_wgrad_args* a) {
    WgradKP k; int ns = 0;
    if (wgrad_plan(a, &k, &ns)) return -1;
    const int th = conv_wgrad_thin(a, false, nullptr, nullptr);     // fp32, 16 / 32 channels on both sides: one slab per persistent workgroup
    if (th > 0) return th;
    const int ls = conv_wgrad_ls(a, false, nullptr, nullptr);       // the loader-specialised row-streaming kernel has its own split rule
    return ls > 0 ? ls : ns;
}

// salt_conv_wgrad_kernel_id: when set, launch_wgrad records which kernel family it would run (3 fast, 4 fast32, 5 generic) and returns
static thread_local int* g_wgrad_probe = nullptr;
#define SALT_WGRAD_PROBE(ID) if (g_wgrad_probe) { *g_wgrad_probe = (ID); return SALT_OK; }

// the fast kernels' branch-free loaders: whole aligned 16-byte pieces of `ve` channels in both views, an aligned slab, and a halo of
// at most maxq pieces for each of 256 threads
static bool wgrad_whole_pieces(const WgradKP& k, int ve, int maxq) {
    return k.p_cs % ve == 0 && k.q_cs % ve == 0 && k.Ca % ve == 0 && k.Cb % ve == 0 &&
           aligned16(k.P, k.Q, k.partials) &&
           k.nb * k.hh * k.hw * (64 / ve) <= maxq * 256;
}

template <typename T>
static int launch_wgrad(const WgradKP& k, hipStream_t st) {
    constexpr int ROWB = (sizeof(T) == 2) ? 192 : 256;
    const size_t lds = (size_t)(k.bmp + k.nb * k.hh * k.hw) * ROWB;
    if (lds > 160 * 1024) SALT_FAIL(SALT_E_LDS, "wgrad: needs %zu bytes of LDS", lds);
    const dim3 grid((unsigned)(k.a_blocks * k.b_blocks * k.nsplit));
    if constexpr (sizeof(T) == 2) {
        // fast path: whole aligned 16-byte pieces, 3x3, 128-pixel K tiles (conv_wgrad_fast_kernel)
        // (5..8 taps - the two 8-tap halves of the 4x4 space-to-depth stem - run the 9-tap instance: the padding tap re-reads tap 0's rows
        //  and is never stored)
        const bool pieces = wgrad_whole_pieces(k, 8, 10);
        const bool fast = pieces && k.ntaps >= 5 && k.ntaps <= 9 && k.bmp == 128;
        if (fast) {
            SALT_WGRAD_PROBE(3)
            bool row16 = k.ntaps == 9 && k.tw_log2 == 4 && k.th_log2 == 3 && k.nb == 1 && k.q_step == 1 && k.hw == 18;
            for (int t = 0; t < 9; ++t) row16 = row16 && k.tap_off[t] == (t / 3) * 18 + t % 3;       // raster tap order
            if (row16) {
                auto kern8 = k.pad_mode ? conv_wgrad_fast8_kernel<true> : conv_wgrad_fast8_kernel<false>;
                return salt_launch(kern8, grid, dim3(512), lds, st, k);
            }
            auto kern = k.pad_mode ? conv_wgrad_fast_kernel<9, 8, true> : conv_wgrad_fast_kernel<9, 8, false>;
            return salt_launch(kern, grid, dim3(256), lds, st, k);
        }
        // round 3: the stride-2 3x3 layers (ResNet layer2-4 conv1): their halo (17 x 17 pixels for an 8 x 8 tile) only leaves room for
        // 64-pixel K tiles, which used to send them to the generic kernel (51 us at 94 TFLOP/s); the fast kernel with 4 k-steps per tile
        const bool fast64 = pieces && k.ntaps == 9 && k.bmp == 64;
        // ... and the 1x1 stride-2 projection shortcuts (one tap; 33 us at 16 TFLOP/s on the generic kernel)
        const bool fast1 = pieces && k.ntaps == 1 && !k.pad_mode && (k.bmp == 64 || k.bmp == 128);
        if (fast1) {
            SALT_WGRAD_PROBE(3)
            auto kern = k.bmp == 64 ? conv_wgrad_fast_kernel<1, 4, false> : conv_wgrad_fast_kernel<1, 8, false>;
            return salt_launch(kern, grid, dim3(256), lds, st, k);
        }
        if (fast64) {
            SALT_WGRAD_PROBE(3)
            auto kern = k.pad_mode ? conv_wgrad_fast_kernel<9, 4, true> : conv_wgrad_fast_kernel<9, 4, false>;
            return salt_launch(kern, grid, dim3(256), lds, st, k);
        }
    }
    if constexpr (sizeof(T) == 4) {
        bool fast = wgrad_whole_pieces(k, 4, 12) && k.ntaps == 9 && k.bmp == 128 &&
                    k.tw_log2 == 4 && k.th_log2 == 3 && k.nb == 1 && k.q_step == 1 && k.hw == 18 && k.hh == 10;
        for (int t = 0; t < 9 && fast; ++t) fast = k.tap_off[t] == (t / 3) * 18 + t % 3;
        if (fast) {
            SALT_WGRAD_PROBE(4)
            const bool a32 = k.Ca <= 32, b32 = k.Cb <= 32;
            auto kern = k.pad_mode ? conv_wgrad_fast32_kernel<true> : conv_wgrad_fast32_kernel<false>;
            if (a32 && b32) kern = k.pad_mode ? conv_wgrad_fast32_kernel<true, 4, 0> : conv_wgrad_fast32_kernel<false, 4, 0>;
            else if (a32) kern = k.pad_mode ? conv_wgrad_fast32_kernel<true, 2, 0> : conv_wgrad_fast32_kernel<false, 2, 0>;
            else if (b32) kern = k.pad_mode ? conv_wgrad_fast32_kernel<true, 2, 1> : conv_wgrad_fast32_kernel<false, 2, 1>;
            return salt_launch(kern, grid, dim3(256), lds, st, k);
        }
    }
    SALT_WGRAD_PROBE(5)
    WgradKP kg = k;
    if constexpr (sizeof(T) == 4) {
        if (lds >= 4 * 16 * 64 * sizeof(float)) {
            const bool a32 = k.Ca <= 32, b32 = k.Cb <= 32;
            kg.ksplit = (a32 && b32) ? 4 : (a32 ? 2 : (b32 ? 3 : 0));
        }
    }
    auto kern = k.ntaps == 1 ? conv_wgrad_kernel<T, 1> : k.ntaps <= 3 ? conv_wgrad_kernel<T, 3> : k.ntaps == 4 ? conv_wgrad_kernel<T, 4> : conv_wgrad_kernel<T, 9>;
    return salt_launch(kern, grid, dim3(256), lds, st, kg);
}

extern "C" int salt_conv_wgrad_kernel_id(const salt_conv_wgrad_args* a) {
    WgradKP k; int ns = 0;
    if (wgrad_plan(a, &k, &ns)) return -1;
    if (conv_wgrad_thin(a, false, nullptr, nullptr) > 0) return 2;
    if (conv_wgrad_ls(a, false, nullptr, nullptr) > 0) return 1;
    int id = 0;
    g_wgrad_probe = &id;
    const int rc = a->dtype == SALT_F32 ? launch_wgrad<float>(k, nullptr) : launch_wgrad<bf16_t>(k, nullptr);
    g_wgrad_probe = nullptr;
    return rc ? -1 : id;
}

extern "C" int salt_conv_wgrad(const salt_conv_wgrad_args* a, void* stream) {
    WgradKP k; int ns = 0;
    int rc = wgrad_plan(a, &k, &ns);
    if (rc) return rc;
    if (!a->partials) SALT_FAIL(SALT_E_BADARG, "wgrad: partials workspace missing");
    { int lrc = SALT_OK; if (conv_wgrad_thin(a, true, (hipStream_t)stream, &lrc) > 0) return lrc; }
    { int lrc = SALT_OK; if (conv_wgrad_ls(a, true, (hipStream_t)stream, &lrc) > 0) return lrc; }
    if (a->nsplit != ns) SALT_FAIL(SALT_E_BADARG, "wgrad: nsplit %d, expected %d", a->nsplit, ns);
    if (a->dtype == SALT_F32) return launch_wgrad<float>(k, (hipStream_t)stream);
    if (a->dtype == SALT_BF16) return launch_wgrad<bf16_t>(k, (hipStream_t)stream);
    SALT_FAIL(SALT_E_BADARG, "wgrad: dtype");
}

extern "C" int salt_wgrad_reduce(const salt_wgrad_reduce_args* a, void* stream) {
    if (!a || !a->partials || !a->grad || a->ntaps < 1 || a->ntaps > SALT_MAX_TAPS) SALT_FAIL(SALT_E_BADARG, "wgrad_reduce: bad args");
    ReduceKP p;
    p.partials = a->partials; p.grad = a->grad; p.nsplit = a->nsplit; p.ntaps = a->ntaps; p.Ca = a->Ca; p.Cb = a->Cb;
    p.KH = a->KH; p.KW = a->KW; p.accumulate = a->accumulate;
    p.ldb = a->ldb > 0 ? a->ldb : a->Cb; p.a_mod = a->a_mod;
    int nt_tab = a->ntaps;
    if (a->a_mod) {
        if (a->a_mod < 0 || a->ntaps != 1 || a->Ca % a->a_mod || a->Ca / a->a_mod > SALT_MAX_TAPS) SALT_FAIL(SALT_E_BADARG, "wgrad_reduce: tap-GEMM slab");
        nt_tab = a->Ca / a->a_mod;
    }
    if (a->ldb && a->ldb < a->Cb) SALT_FAIL(SALT_E_BADARG, "wgrad_reduce: ldb < Cb");
    for (int t = 0; t < nt_tab; ++t) {
        if (a->tap_kh[t] < 0 || a->tap_kh[t] >= a->KH || a->tap_kw[t] < 0 || a->tap_kw[t] >= a->KW) SALT_FAIL(SALT_E_BADARG, "wgrad_reduce: tap");
        p.tap_kh[t] = a->tap_kh[t]; p.tap_kw[t] = a->tap_kw[t];
    }
    const int64_t slab = (int64_t)a->ntaps * a->Ca * a->Cb;
    if (a->nsplit <= 8) return salt_launch(wgrad_reduce8_kernel, dim3((unsigned)((slab + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p);
    return salt_launch(wgrad_reduce_kernel, dim3((unsigned)((slab + 63) / 64)), dim3(256), 0, (hipStream_t)stream, p);
}
