// conv_group.hip — the grouped 3x3 convolution in the middle of every SE-ResNeXt bottleneck (senet.py SEResNeXtBottleneck.conv2:
// nn.Conv2d(C, C, 3, stride, padding 1, groups 32, bias=False); C = 128 .. 1024, Cg = C / 32 = 4 .. 32), its data gradient and its
// weight gradient.  A streaming layer: 9 Cg multiply-adds per output element next to one read and one write of the tensor, so the
// kernels contract with the TRUE Cg in fp32 on the vector ALU from the fp32 master weight [C][Cg][3][3] (no packed copy):
//   gconv_kernel   a workgroup owns a 32-channel block (32 / Cg whole groups) and walks 8 x 8 output tiles with it: the block's
//                  weights are staged once as [tap][n][Cg] floats, per tile the halo of the 32 input channels as [pixel][32] floats
//                  (zero outside the image; bf16 is widened here).  A thread holds 2 pixels x 4 consecutive output channels (one
//                  group: 4 | Cg) and reads 16-byte pieces of both operands: 6 LDS reads per 32 multiply-adds.  Forward (stride 1 | 2)
//                  and data gradient are ONE kernel: the data gradient stages dy and the transposed weights, stride 2 as the gather
//                  form - a dx pixel takes the taps whose parity matches, from a 5 x 5 halo of dy.
//   epilogues      eval: relu?(v scale + shift).  train: raw y and the BatchNorm statistics of the stored values, per tile (sum, M2
//                  about the tile mean, count: fixed order) or as fp64 shard adds without a ticket.  dgrad: dx (+)= v.
//   gconv_wgrad    a workgroup owns (pixel split, 32-channel block); 256 threads = 8 Cg (channel, 4 inputs) quads x 32 / Cg pixel
//                  sub-sets, 36 accumulators each; the sub-sets meet in LDS in ascending order, the split's slab goes out in the
//                  reference layout, and slab_sum_kernel (common.h) adds the slabs in ascending split order.
#include "common.h"

namespace {

constexpr int GT = 8;                 // output tile edge (pixels)
constexpr int GCB = 32;               // channels of a workgroup's block
constexpr int XS = GCB + 4;           // LDS pixel stride in floats (144 bytes: 16-byte aligned, not a multiple of the 128-byte bank row)
constexpr int G_TARGET_WGS = 2048;    // workgroups of a forward / data-gradient launch (a shape rule: no device query)
constexpr int GW_TARGET_WGS = 1024, GW_MIN_TILES = 4;   // weight gradient: workgroups per launch, fewest tiles of a split

enum { G_FWD1 = 0, G_FWD2 = 1, G_DG1 = 2, G_DG2 = 3 };
// halo edge of a tile: forward (GT - 1) stride + 3; data gradient 10 (stride 1) or the 5 dy rows of even parity (stride 2)
constexpr int halo_edge(int mode) { return mode == G_FWD1 ? GT + 2 : mode == G_FWD2 ? 2 * GT + 1 : mode == G_DG1 ? GT + 2 : GT / 2 + 1; }

struct GconvKP {
    const void* in; void* out; const float* w;
    const float* scale; const float* shift; float* stats; float* stats_cnt; double* fin_acc;
    int B, IH, IW, OH, OW, C, in_cs, out_cs, relu, accumulate, tiles_y, tiles_x, ntiles, ncb, nchunks;
};

// one 16-byte piece of the halo / tile: global (or zero) -> floats in LDS
template <typename T>
__device__ __forceinline__ void stage_piece(const T* src, bool ok, float* dst) {
    constexpr int VE = Elem<T>::VE;
    float f[VE];
    if (ok) unpack16<T>(*reinterpret_cast<const u32x4*>(src), f);
    else {
#pragma unroll
        for (int j = 0; j < VE; ++j) f[j] = 0.f;
    }
#pragma unroll
    for (int j = 0; j < VE; j += 4) *reinterpret_cast<f32x4*>(dst + j) = f32x4{f[j], f[j + 1], f[j + 2], f[j + 3]};
}

// sum over the 32 pixel slots that share a channel quad (lanes 8 apart, then the four waves in a fixed order); s_red: [4][32]
__device__ __forceinline__ float slot_sum(float s, float* s_red, int n, int lane, int wave) {
#pragma unroll
    for (int o = 8; o < 64; o <<= 1) s += __shfl_xor(s, o);
    __syncthreads();                                               // the previous use of s_red
    if (lane < 8) s_red[wave * GCB + n] = s;
    __syncthreads();
    return ((s_red[n] + s_red[GCB + n]) + s_red[2 * GCB + n]) + s_red[3 * GCB + n];
}

template <typename T, int CG, int MODE>
__global__ __launch_bounds__(256) void gconv_kernel(GconvKP p) {
    constexpr bool DG = MODE >= G_DG1;
    constexpr int S = (MODE & 1) + 1, HL = halo_edge(MODE), WS = CG + 4, VE = Elem<T>::VE, PPP = GCB / VE;
    extern __shared__ __attribute__((aligned(16))) float sm_g[];
    float* s_w = sm_g;                               // [9][GCB][WS]: k (the contraction index inside the group) contiguous
    float* s_x = s_w + 9 * GCB * WS;                 // [HL * HL][XS]
    float* s_red = s_x + HL * HL * XS;               // [4][GCB]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, cq = tid & 7, pp = tid >> 3;
    const int cb = blockIdx.x % p.ncb, chunk = blockIdx.x / p.ncb, c0 = cb * GCB;
    const T* in = reinterpret_cast<const T*>(p.in);
    T* out = reinterpret_cast<T*>(p.out);

    // ---- the block's weights, read in the master weight's own order ((n, k, tap) contiguous for the 32 channels of the block)
    for (int i = tid; i < GCB * CG * 9; i += 256) {
        const int tap = i % 9, r = i / 9, k = r % CG, n = r / CG;
        const float v = p.w[(int64_t)c0 * CG * 9 + i];
        // forward: row = output channel n, column = input k.  data gradient: w[c0 + n][k] feeds dx channel (group base of n) + k from
        // dy channel n, whose index inside the group is n % CG (c0 is a multiple of 32 and CG divides 32)
        if (DG) s_w[(tap * GCB + (n / CG) * CG + k) * WS + n % CG] = v;
        else s_w[(tap * GCB + n) * WS + k] = v;
    }
    const int gbase = (4 * cq / CG) * CG;            // first channel (inside the block) of this quad's group

    for (int tile = chunk; tile < p.ntiles; tile += p.nchunks) {
        int t = tile;
        const int txi = t % p.tiles_x; t /= p.tiles_x;
        const int tyi = t % p.tiles_y, b = t / p.tiles_y;
        const int oy0 = tyi * GT, ox0 = txi * GT;
        const int hy0 = DG ? (S == 1 ? oy0 - 1 : oy0 / 2) : oy0 * S - 1, hx0 = DG ? (S == 1 ? ox0 - 1 : ox0 / 2) : ox0 * S - 1;
        __syncthreads();                             // the previous tile's readers of s_x are done (first tile: s_w is complete)
        for (int i = tid; i < HL * HL * PPP; i += 256) {
            const int pc = i % PPP, hp = i / PPP, hx = hp % HL, hy = hp / HL;
            const int iy = hy0 + hy, ix = hx0 + hx;
            const bool ok = iy >= 0 && iy < p.IH && ix >= 0 && ix < p.IW;
            stage_piece<T>(in + (((int64_t)b * p.IH + (ok ? iy : 0)) * p.IW + (ok ? ix : 0)) * p.in_cs + c0 + pc * VE, ok, s_x + hp * XS + pc * VE);
        }
        __syncthreads();
        f32x4 acc[2];
        acc[0] = acc[1] = f32x4{0.f, 0.f, 0.f, 0.f};
        // the tap loop stays rolled: unrolled, the compiler hoists every LDS read of the 9 taps and runs out of registers
#pragma unroll 1
        for (int tap = 0; tap < 9; ++tap) {
            const int kh = tap / 3, kw = tap - 3 * kh;
            const float* xr[2]; bool ok[2];
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int px = pp & 7, py = (pp >> 3) + 4 * j;         // pixel slots pp and pp + 32 of the tile
                int hy, hx;
                ok[j] = true;
                if (!DG) { hy = py * S + kh; hx = px * S + kw; }
                else if (S == 1) { hy = py + 2 - kh; hx = px + 2 - kw; }
                else {
                    // iy + 1 - kh = 2 oy: the tile origin is even, so the parity is that of ty = py + 1 - kh (-1 .. 8)
                    const int ty = py + 1 - kh, tx = px + 1 - kw;
                    ok[j] = !((ty | tx) & 1);
                    hy = ok[j] ? ty >> 1 : 0; hx = ok[j] ? tx >> 1 : 0;
                }
                xr[j] = s_x + (hy * HL + hx) * XS + gbase;
            }
            const float* wr = s_w + (tap * GCB + 4 * cq) * WS;
#pragma unroll
            for (int k4 = 0; k4 < CG; k4 += 4) {
                f32x4 wv[4];
#pragma unroll
                for (int n = 0; n < 4; ++n) wv[n] = *reinterpret_cast<const f32x4*>(wr + n * WS + k4);
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    if (DG && S == 2 && !ok[j]) continue;
                    const f32x4 xv = *reinterpret_cast<const f32x4*>(xr[j] + k4);
#pragma unroll
                    for (int n = 0; n < 4; ++n) {
                        float a = acc[j][n];
                        a = __fmaf_rn(xv.x, wv[n].x, a); a = __fmaf_rn(xv.y, wv[n].y, a); a = __fmaf_rn(xv.z, wv[n].z, a); a = __fmaf_rn(xv.w, wv[n].w, a);
                        acc[j][n] = a;
                    }
                }
            }
        }
        // ---- epilogue: the thread holds channels c0 + 4 cq .. + 3 of pixels (oy0 + (pp >> 3) + 4 j, ox0 + (pp & 7))
        const bool train = p.stats != nullptr || p.fin_acc != nullptr;
        const int ch = c0 + 4 * cq;
        f32x4 sc4 = f32x4{1.f, 1.f, 1.f, 1.f}, sh4 = f32x4{0.f, 0.f, 0.f, 0.f};
        if (p.scale) {
#pragma unroll
            for (int n = 0; n < 4; ++n) { sc4[n] = p.scale[ch + n]; sh4[n] = p.shift[ch + n]; }
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int oy = oy0 + (pp >> 3) + 4 * j, ox = ox0 + (pp & 7);
            const bool valid = oy < p.OH && ox < p.OW;
            f32x4 v = acc[j];
            if (valid) {
                T* o = out + (((int64_t)b * p.OH + oy) * p.OW + ox) * p.out_cs + ch;
                if (!DG) {
                    if (p.scale) {
#pragma unroll
                        for (int n = 0; n < 4; ++n) v[n] = __fmaf_rn(v[n], sc4[n], sh4[n]);
                    }
                    if (p.relu) {
#pragma unroll
                        for (int n = 0; n < 4; ++n) v[n] = fmaxf(v[n], 0.f);
                    }
                }
                if constexpr (sizeof(T) == 2) {
                    if (DG && p.accumulate) {
                        const uint2 old = *reinterpret_cast<const uint2*>(o);
                        v.x += __uint_as_float(old.x << 16); v.y += __uint_as_float(old.x & 0xffff0000u);
                        v.z += __uint_as_float(old.y << 16); v.w += __uint_as_float(old.y & 0xffff0000u);
                    }
                    const unsigned lo = f2bf_pk(v.x, v.y), hi = f2bf_pk(v.z, v.w);
                    *reinterpret_cast<uint2*>(o) = make_uint2(lo, hi);
                    v.x = __uint_as_float(lo << 16); v.y = __uint_as_float(lo & 0xffff0000u);          // statistics of the STORED value
                    v.z = __uint_as_float(hi << 16); v.w = __uint_as_float(hi & 0xffff0000u);
                } else {
                    if (DG && p.accumulate) v += *reinterpret_cast<const f32x4*>(o);
                    *reinterpret_cast<f32x4*>(o) = v;
                }
            }
            acc[j] = valid ? v : f32x4{0.f, 0.f, 0.f, 0.f};
        }
        if (!DG && train) {
            const int vh = p.OH - oy0 < GT ? p.OH - oy0 : GT, vw = p.OW - ox0 < GT ? p.OW - ox0 : GT;
            const float cnt = (float)(vh * vw);
            bool valid[2];
#pragma unroll
            for (int j = 0; j < 2; ++j) valid[j] = (oy0 + (pp >> 3) + 4 * j) < p.OH && (ox0 + (pp & 7)) < p.OW;
            if (p.stats) {
                // per-tile partial: sum, then M2 about the tile's own mean (two passes over the 8 values the thread holds)
#pragma unroll
                for (int n = 0; n < 4; ++n) {
                    const float tot = slot_sum(acc[0][n] + acc[1][n], s_red, 4 * cq + n, lane, wave);
                    const float mean = tot / cnt;
                    const float d0 = valid[0] ? acc[0][n] - mean : 0.f, d1 = valid[1] ? acc[1][n] - mean : 0.f;
                    const float m2 = slot_sum(d0 * d0 + d1 * d1, s_red, 4 * cq + n, lane, wave);
                    if (pp == 0) {
                        p.stats[((int64_t)tile * 2) * p.C + ch + n] = tot;
                        p.stats[((int64_t)tile * 2 + 1) * p.C + ch + n] = m2;
                    }
                }
                if (cb == 0 && tid == 0) p.stats_cnt[tile] = cnt;
            } else {
                double* shard = p.fin_acc + (size_t)(blockIdx.x & 7) * (2 * p.C + 1);
#pragma unroll
                for (int n = 0; n < 4; ++n) {
                    const float tot = slot_sum(acc[0][n] + acc[1][n], s_red, 4 * cq + n, lane, wave);
                    const float sq = slot_sum(acc[0][n] * acc[0][n] + acc[1][n] * acc[1][n], s_red, 4 * cq + n, lane, wave);
                    if (pp == 0) { fin_add(shard + ch + n, (double)tot); fin_add(shard + p.C + ch + n, (double)sq); }
                }
                if (cb == 0 && tid == 0) fin_add(shard + 2 * p.C, (double)cnt);
            }
        }
    }
}

// ---------------------------------------------------------------- weight gradient
struct GwKP {
    const void* x; const void* dy; float* partials;
    int B, H, W, OH, OW, C, x_cs, dy_cs, tiles_y, tiles_x, ntiles, ncb, tps;
};

template <typename T, int CG, int S>
__global__ __launch_bounds__(256) void gconv_wgrad_kernel(GwKP p) {
    constexpr int HL = (GT - 1) * S + 3, VE = Elem<T>::VE, PPP = GCB / VE;
    constexpr int NQ = 8 * CG, NPS = 256 / NQ, Q4 = CG / 4;        // (channel, 4 inputs) quads; pixel sub-sets; quads per channel
    constexpr int SLAB = GCB * CG * 9;                             // the block's slab: [n][k][tap], the master weight's layout
    constexpr int NX = HL * HL * XS > NPS * SLAB ? HL * HL * XS : NPS * SLAB;
    extern __shared__ __attribute__((aligned(16))) float sm_g[];
    float* s_dy = sm_g;                              // [GT * GT][XS]
    float* s_x = s_dy + GT * GT * XS;                // [HL * HL][XS]; afterwards [NPS][SLAB]
    (void)NX;
    const int tid = threadIdx.x, qi = tid % NQ, ps = tid / NQ, n = qi / Q4, k4 = (qi % Q4) * 4;
    const int cb = blockIdx.x % p.ncb, split = blockIdx.x / p.ncb, c0 = cb * GCB;
    const int gbase = (n / CG) * CG;
    const T* x = reinterpret_cast<const T*>(p.x);
    const T* dy = reinterpret_cast<const T*>(p.dy);
    f32x4 acc[9];
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) acc[tap] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int t_end = (split + 1) * p.tps < p.ntiles ? (split + 1) * p.tps : p.ntiles;
    for (int tile = split * p.tps; tile < t_end; ++tile) {
        int t = tile;
        const int txi = t % p.tiles_x; t /= p.tiles_x;
        const int tyi = t % p.tiles_y, b = t / p.tiles_y;
        const int oy0 = tyi * GT, ox0 = txi * GT, hy0 = oy0 * S - 1, hx0 = ox0 * S - 1;
        __syncthreads();
        for (int i = tid; i < GT * GT * PPP; i += 256) {
            const int pc = i % PPP, px = i / PPP, oy = oy0 + px / GT, ox = ox0 + px % GT;
            const bool ok = oy < p.OH && ox < p.OW;
            stage_piece<T>(dy + (((int64_t)b * p.OH + (ok ? oy : 0)) * p.OW + (ok ? ox : 0)) * p.dy_cs + c0 + pc * VE, ok, s_dy + px * XS + pc * VE);
        }
        for (int i = tid; i < HL * HL * PPP; i += 256) {
            const int pc = i % PPP, hp = i / PPP, iy = hy0 + hp / HL, ix = hx0 + hp % HL;
            const bool ok = iy >= 0 && iy < p.H && ix >= 0 && ix < p.W;
            stage_piece<T>(x + (((int64_t)b * p.H + (ok ? iy : 0)) * p.W + (ok ? ix : 0)) * p.x_cs + c0 + pc * VE, ok, s_x + hp * XS + pc * VE);
        }
        __syncthreads();
        for (int px = ps; px < GT * GT; px += NPS) {
            const int py = px / GT, pxx = px % GT;
            const float d = s_dy[px * XS + n];
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                const int kh = tap / 3, kw = tap - 3 * kh;
                const f32x4 xv = *reinterpret_cast<const f32x4*>(s_x + ((py * S + kh) * HL + pxx * S + kw) * XS + gbase + k4);
                acc[tap].x = __fmaf_rn(d, xv.x, acc[tap].x); acc[tap].y = __fmaf_rn(d, xv.y, acc[tap].y);
                acc[tap].z = __fmaf_rn(d, xv.z, acc[tap].z); acc[tap].w = __fmaf_rn(d, xv.w, acc[tap].w);
            }
        }
    }
    // ---- the pixel sub-sets meet in LDS, ascending; the slab leaves in the reference layout
    __syncthreads();
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
        for (int j = 0; j < 4; ++j) s_x[ps * SLAB + (n * CG + k4 + j) * 9 + tap] = acc[tap][j];
    __syncthreads();
    float* slab = p.partials + ((int64_t)split * p.C + c0) * CG * 9;
    for (int i = tid; i < SLAB; i += 256) {
        float s = s_x[i];
#pragma unroll
        for (int q = 1; q < NPS; ++q) s += s_x[q * SLAB + i];
        slab[i] = s;
    }
}

// ---------------------------------------------------------------- host
int gconv_shape_check(const char* op, const salt_view& x, int groups, int stride) {
    if (groups != 32) SALT_FAIL(SALT_E_UNSUPPORTED, "%s: %d groups (supported: 32)", op, groups);
    if (stride != 1 && stride != 2) SALT_FAIL(SALT_E_UNSUPPORTED, "%s: stride %d (supported: 1, 2)", op, stride);
    if (x.C != 128 && x.C != 256 && x.C != 512 && x.C != 1024) SALT_FAIL(SALT_E_UNSUPPORTED, "%s: %d channels (supported: 128, 256, 512, 1024)", op, x.C);
    if (x.B < 1 || x.H < 1 || x.W < 1) SALT_FAIL(SALT_E_BADARG, "%s: empty batch %d x %d x %d", op, x.B, x.H, x.W);
    if ((int64_t)x.B * cdiv(x.H, GT) * cdiv(x.W, GT) >= (1ll << 31) / 64) SALT_FAIL(SALT_E_UNSUPPORTED, "%s: too many tiles", op);
    return SALT_OK;
}
inline int out_size(int n, int stride) { return (n - 1) / stride + 1; }

template <typename T, int CG>
int gconv_launch_cg(int mode, const GconvKP& p, hipStream_t st) {
    const int hl = halo_edge(mode);
    const size_t lds = ((size_t)9 * GCB * (CG + 4) + (size_t)hl * hl * XS + 4 * GCB) * sizeof(float);
    const dim3 grid((unsigned)(p.ncb * p.nchunks));
    switch (mode) {
        case G_FWD1: return salt_launch(gconv_kernel<T, CG, G_FWD1>, grid, dim3(256), lds, st, p);
        case G_FWD2: return salt_launch(gconv_kernel<T, CG, G_FWD2>, grid, dim3(256), lds, st, p);
        case G_DG1: return salt_launch(gconv_kernel<T, CG, G_DG1>, grid, dim3(256), lds, st, p);
        default: return salt_launch(gconv_kernel<T, CG, G_DG2>, grid, dim3(256), lds, st, p);
    }
}
template <typename T>
int gconv_launch(int mode, const GconvKP& p, hipStream_t st) {
    switch (p.C / 32) {
        case 4: return gconv_launch_cg<T, 4>(mode, p, st);
        case 8: return gconv_launch_cg<T, 8>(mode, p, st);
        case 16: return gconv_launch_cg<T, 16>(mode, p, st);
        default: return gconv_launch_cg<T, 32>(mode, p, st);
    }
}
// tiles of the launch's output grid [B, OH, OW] and the workgroup shape over them
void gconv_grid(GconvKP& p) {
    p.tiles_y = cdiv(p.OH, GT); p.tiles_x = cdiv(p.OW, GT); p.ntiles = p.B * p.tiles_y * p.tiles_x;
    p.ncb = p.C / GCB;
    const int want = G_TARGET_WGS / p.ncb;
    p.nchunks = p.ntiles < want ? p.ntiles : want;
}

template <typename T, int CG>
int gwgrad_launch_cg(int stride, const GwKP& p, int nsplit, hipStream_t st) {
    constexpr int NPS = 32 / CG, SLAB = GCB * CG * 9;
    const int hl = (GT - 1) * stride + 3;
    const size_t nx = (size_t)hl * hl * XS > (size_t)NPS * SLAB ? (size_t)hl * hl * XS : (size_t)NPS * SLAB;
    const size_t lds = ((size_t)GT * GT * XS + nx) * sizeof(float);
    const dim3 grid((unsigned)(p.ncb * nsplit));
    return stride == 1 ? salt_launch(gconv_wgrad_kernel<T, CG, 1>, grid, dim3(256), lds, st, p)
                       : salt_launch(gconv_wgrad_kernel<T, CG, 2>, grid, dim3(256), lds, st, p);
}
template <typename T>
int gwgrad_launch(int stride, const GwKP& p, int nsplit, hipStream_t st) {
    switch (p.C / 32) {
        case 4: return gwgrad_launch_cg<T, 4>(stride, p, nsplit, st);
        case 8: return gwgrad_launch_cg<T, 8>(stride, p, nsplit, st);
        case 16: return gwgrad_launch_cg<T, 16>(stride, p, nsplit, st);
        default: return gwgrad_launch_cg<T, 32>(stride, p, nsplit, st);
    }
}
// pixel splits of the weight gradient: tiles per split -> nsplit (a function of the shape alone)
void gwgrad_plan(GwKP& p, int& nsplit) {
    p.tiles_y = cdiv(p.OH, GT); p.tiles_x = cdiv(p.OW, GT); p.ntiles = p.B * p.tiles_y * p.tiles_x;
    p.ncb = p.C / GCB;
    const int want = GW_TARGET_WGS / p.ncb;
    p.tps = cdiv(p.ntiles, want);
    if (p.tps < GW_MIN_TILES) p.tps = GW_MIN_TILES;
    nsplit = cdiv(p.ntiles, p.tps);
}

}  // namespace

extern "C" int salt_gconv_stats_parts(const salt_gconv_args* a) {
    if (!a) SALT_FAIL(SALT_E_BADARG, "gconv: null args");
    const int rc = gconv_shape_check("gconv", a->x, a->groups, a->stride);
    if (rc) return rc;
    return a->x.B * cdiv(out_size(a->x.H, a->stride), GT) * cdiv(out_size(a->x.W, a->stride), GT);
}

extern "C" int salt_gconv(const salt_gconv_args* a, void* stream) {
    if (!a) SALT_FAIL(SALT_E_BADARG, "gconv: null args");
    int rc = gconv_shape_check("gconv", a->x, a->groups, a->stride);
    if (rc) return rc;
    if (a->dtype != SALT_F32 && a->dtype != SALT_BF16) SALT_FAIL(SALT_E_BADARG, "gconv: bad dtype %d", a->dtype);
    const int OH = out_size(a->x.H, a->stride), OW = out_size(a->x.W, a->stride);
    if ((rc = view_check16("gconv", "x", a->x, a->dtype, a->x.B, a->x.H, a->x.W, a->x.C))) return rc;
    if ((rc = view_check16("gconv", "y", a->y, a->dtype, a->x.B, OH, OW, a->x.C))) return rc;
    if (!a->w) SALT_FAIL(SALT_E_BADARG, "gconv: w");
    if ((a->scale == nullptr) != (a->shift == nullptr)) SALT_FAIL(SALT_E_BADARG, "gconv: scale/shift");
    if (a->stats && a->fin_acc) SALT_FAIL(SALT_E_BADARG, "gconv: statistics go to the partials or to the shards, not both");
    if ((a->stats == nullptr) != (a->stats_cnt == nullptr)) SALT_FAIL(SALT_E_BADARG, "gconv: stats/stats_cnt");
    if ((a->stats || a->fin_acc) && (a->scale || a->relu)) SALT_FAIL(SALT_E_BADARG, "gconv: the train form stores the raw output (no scale / shift / relu)");
    GconvKP p;
    p.in = a->x.p; p.out = a->y.p; p.w = a->w; p.scale = a->scale; p.shift = a->shift; p.stats = a->stats; p.stats_cnt = a->stats_cnt; p.fin_acc = a->fin_acc;
    p.B = a->x.B; p.IH = a->x.H; p.IW = a->x.W; p.OH = OH; p.OW = OW; p.C = a->x.C; p.in_cs = a->x.cs; p.out_cs = a->y.cs; p.relu = a->relu; p.accumulate = 0;
    gconv_grid(p);
    const int mode = a->stride == 1 ? G_FWD1 : G_FWD2;
    SALT_DISPATCH_DTYPE(a->dtype, T, return gconv_launch<T>(mode, p, (hipStream_t)stream))
}

extern "C" int salt_gconv_dgrad(const salt_gconv_dgrad_args* a, void* stream) {
    if (!a) SALT_FAIL(SALT_E_BADARG, "gconv_dgrad: null args");
    int rc = gconv_shape_check("gconv_dgrad", a->dx, a->groups, a->stride);
    if (rc) return rc;
    if (a->dtype != SALT_F32 && a->dtype != SALT_BF16) SALT_FAIL(SALT_E_BADARG, "gconv_dgrad: bad dtype %d", a->dtype);
    const int OH = out_size(a->dx.H, a->stride), OW = out_size(a->dx.W, a->stride);
    if ((rc = view_check16("gconv_dgrad", "dx", a->dx, a->dtype, a->dx.B, a->dx.H, a->dx.W, a->dx.C))) return rc;
    if ((rc = view_check16("gconv_dgrad", "dy", a->dy, a->dtype, a->dx.B, OH, OW, a->dx.C))) return rc;
    if (!a->w) SALT_FAIL(SALT_E_BADARG, "gconv_dgrad: w");
    GconvKP p;
    p.in = a->dy.p; p.out = a->dx.p; p.w = a->w; p.scale = nullptr; p.shift = nullptr; p.stats = nullptr; p.stats_cnt = nullptr; p.fin_acc = nullptr;
    p.B = a->dx.B; p.IH = OH; p.IW = OW; p.OH = a->dx.H; p.OW = a->dx.W; p.C = a->dx.C; p.in_cs = a->dy.cs; p.out_cs = a->dx.cs; p.relu = 0;
    p.accumulate = a->accumulate ? 1 : 0;
    gconv_grid(p);
    const int mode = a->stride == 1 ? G_DG1 : G_DG2;
    SALT_DISPATCH_DTYPE(a->dtype, T, return gconv_launch<T>(mode, p, (hipStream_t)stream))
}

extern "C" int salt_gconv_wgrad_parts(const salt_gconv_wgrad_args* a) {
    if (!a) SALT_FAIL(SALT_E_BADARG, "gconv_wgrad: null args");
    const int rc = gconv_shape_check("gconv_wgrad", a->x, a->groups, a->stride);
    if (rc) return rc;
    GwKP p; int nsplit = 0;
    p.B = a->x.B; p.OH = out_size(a->x.H, a->stride); p.OW = out_size(a->x.W, a->stride); p.C = a->x.C;
    gwgrad_plan(p, nsplit);
    return nsplit;
}

extern "C" int salt_gconv_wgrad(const salt_gconv_wgrad_args* a, void* stream) {
    if (!a) SALT_FAIL(SALT_E_BADARG, "gconv_wgrad: null args");
    int rc = gconv_shape_check("gconv_wgrad", a->x, a->groups, a->stride);
    if (rc) return rc;
    if (a->dtype != SALT_F32 && a->dtype != SALT_BF16) SALT_FAIL(SALT_E_BADARG, "gconv_wgrad: bad dtype %d", a->dtype);
    const int OH = out_size(a->x.H, a->stride), OW = out_size(a->x.W, a->stride);
    if ((rc = view_check16("gconv_wgrad", "x", a->x, a->dtype, a->x.B, a->x.H, a->x.W, a->x.C))) return rc;
    if ((rc = view_check16("gconv_wgrad", "dy", a->dy, a->dtype, a->x.B, OH, OW, a->x.C))) return rc;
    if (!a->partials || !a->grad) SALT_FAIL(SALT_E_BADARG, "gconv_wgrad: partials / grad");
    GwKP p; int nsplit = 0;
    p.x = a->x.p; p.dy = a->dy.p; p.partials = a->partials;
    p.B = a->x.B; p.H = a->x.H; p.W = a->x.W; p.OH = OH; p.OW = OW; p.C = a->x.C; p.x_cs = a->x.cs; p.dy_cs = a->dy.cs;
    gwgrad_plan(p, nsplit);
    if (a->nsplit != nsplit) SALT_FAIL(SALT_E_BADARG, "gconv_wgrad: nsplit %d, salt_gconv_wgrad_parts says %d", a->nsplit, nsplit);
    hipStream_t st = (hipStream_t)stream;
    SALT_DISPATCH_DTYPE(a->dtype, T, rc = gwgrad_launch<T>(a->stride, p, nsplit, st))
    if (rc) return rc;
    const int total = a->x.C * (a->x.C / 32) * 9;
    return salt_launch(slab_sum_kernel<>, dim3(cdiv(total, 256)), dim3(256), 0, st, (const float*)a->partials, nsplit, total, a->grad, a->accumulate ? 1 : 0);
}
