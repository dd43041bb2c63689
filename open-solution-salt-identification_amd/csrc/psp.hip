// psp.hip — the low-resolution middle of PSPNet (saltnet.h: salt_psp_pool / salt_psp_pool_bwd / salt_psp_merge / salt_psp_merge_bwd /
// salt_bn_prelu / salt_bn_prelu_bwd).  Six bandwidth operators over at most 32 x 32 pixels per image: 16-byte pieces, fp32 sums in a
// fixed order, no atomics - a rerun produces the same bits.
#include "common.h"

#define PSP_MAX_HW 32          // h, w of the pooled feature map
#define PSP_MAX_S 6            // largest pyramid size
#define PSP_CB 64              // channels per workgroup of the merge kernels

struct PspGeom { int n; int s[SALT_PSP_MAX_STAGES]; int off[SALT_PSP_MAX_STAGES]; int bins; };      // off: first bin of a stage
struct PspPtrs { void* p[SALT_PSP_MAX_STAGES]; int cs[SALT_PSP_MAX_STAGES]; };

// torch's adaptive pooling window along an axis of n elements: [floor(i n / s), ceil((i + 1) n / s))
__device__ __forceinline__ int bin_lo(int i, int n, int s) { return (i * n) / s; }
__device__ __forceinline__ int bin_hi(int i, int n, int s) { return ((i + 1) * n + s - 1) / s; }

// torch's size-based bilinear source index of destination d along an axis resized from s to n elements.  PINNED in fp32 - one
// division, one product, one subtraction, no contraction - so that tests/psp_op_reference.py forms the same weights bit for bit.
__device__ __forceinline__ void psp_src(int d, int n, int s, int ac, int& i0, int& i1, float& w0, float& w1) {
    float src;
    if (ac) src = n > 1 ? __fmul_rn(__fdiv_rn((float)(s - 1), (float)(n - 1)), (float)d) : 0.f;
    else { src = __fsub_rn(__fmul_rn(__fdiv_rn((float)s, (float)n), (float)d + 0.5f), 0.5f); src = src < 0.f ? 0.f : src; }
    i0 = (int)src;
    i0 = i0 < s - 1 ? i0 : s - 1;
    i1 = i0 < s - 1 ? i0 + 1 : i0;
    w1 = __fsub_rn(src, (float)i0);
    w0 = __fsub_rn(1.f, w1);
}

__device__ __forceinline__ int psp_stage_of(const PspGeom& g, int bin) {
    int k = 0;
#pragma unroll
    for (int q = 1; q < SALT_PSP_MAX_STAGES; ++q) k = (q < g.n && bin >= g.off[q]) ? q : k;
    return k;
}

// ---------------------------------------------------------------------------------------------------------------- pooling
// one thread per (image, bin, 16-byte piece): the window's pixels in row-major order, one division by the window's area
template <typename T>
__global__ __launch_bounds__(256) void psp_pool_kernel(const T* x, int B, int h, int w, int C, int xcs, PspGeom g, PspPtrs out) {
    constexpr int N = Elem<T>::VE;
    const int cpv = C / N;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)B * g.bins * cpv) return;
    const int pc = (int)(idx % cpv), bin = (int)((idx / cpv) % g.bins), b = (int)(idx / ((int64_t)cpv * g.bins));
    const int k = psp_stage_of(g, bin), s = g.s[k], i = (bin - g.off[k]) / s, j = (bin - g.off[k]) % s;
    const int y0 = bin_lo(i, h, s), y1 = bin_hi(i, h, s), x0 = bin_lo(j, w, s), x1 = bin_hi(j, w, s);
    float acc[N];
#pragma unroll
    for (int e = 0; e < N; ++e) acc[e] = 0.f;
    for (int yy = y0; yy < y1; ++yy)
        for (int xx = x0; xx < x1; ++xx) {
            float v[N];
            Piece<T, true>::ld(x + ((int64_t)(b * h + yy) * w + xx) * xcs + pc * N, v);
#pragma unroll
            for (int e = 0; e < N; ++e) acc[e] += v[e];
        }
    const float area = (float)((y1 - y0) * (x1 - x0));
#pragma unroll
    for (int e = 0; e < N; ++e) acc[e] = __fdiv_rn(acc[e], area);
    Piece<T, true>::st((T*)out.p[k] + ((int64_t)(b * s + i) * s + j) * out.cs[k] + pc * N, acc);
}

// one thread per (pixel, 16-byte piece): a gather over the bins that contain the pixel - stages, rows, columns ascending
template <typename T>
__global__ __launch_bounds__(256) void psp_pool_bwd_kernel(PspPtrs dp, int B, int h, int w, int C, PspGeom g, T* dx, int dcs, int accumulate) {
    constexpr int N = Elem<T>::VE;
    const int cpv = C / N;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)B * h * w * cpv) return;
    const int pc = (int)(idx % cpv);
    const int64_t pix = idx / cpv;
    const int xx = (int)(pix % w), yy = (int)((pix / w) % h), b = (int)(pix / ((int64_t)w * h));
    float acc[N];
#pragma unroll
    for (int e = 0; e < N; ++e) acc[e] = 0.f;
    for (int k = 0; k < g.n; ++k) {
        const int s = g.s[k];
        for (int i = 0; i < s; ++i) {
            const int y0 = bin_lo(i, h, s), y1 = bin_hi(i, h, s);
            if (yy < y0 || yy >= y1) continue;
            for (int j = 0; j < s; ++j) {
                const int x0 = bin_lo(j, w, s), x1 = bin_hi(j, w, s);
                if (xx < x0 || xx >= x1) continue;
                const float area = (float)((y1 - y0) * (x1 - x0));
                float v[N];
                Piece<T, true>::ld((const T*)dp.p[k] + ((int64_t)(b * s + i) * s + j) * dp.cs[k] + pc * N, v);
#pragma unroll
                for (int e = 0; e < N; ++e) acc[e] += __fdiv_rn(v[e], area);
            }
        }
    }
    T* o = dx + pix * dcs + pc * N;
    if (accumulate) {
        float old[N];
        Piece<T, true>::ld(o, old);
#pragma unroll
        for (int e = 0; e < N; ++e) acc[e] += old[e];
    }
    Piece<T, true>::st(o, acc);
}

// ---------------------------------------------------------------------------------------------------------------- merge
// LDS of the merge kernels: the resize tables of both axes, then (forward) the image's q values of the channel block as fp32
struct PspTab {
    int i0[2][SALT_PSP_MAX_STAGES][PSP_MAX_HW];            // [axis: 0 rows, 1 columns][stage][destination]
    int i1[2][SALT_PSP_MAX_STAGES][PSP_MAX_HW];
    float w0[2][SALT_PSP_MAX_STAGES][PSP_MAX_HW];
    float w1[2][SALT_PSP_MAX_STAGES][PSP_MAX_HW];
};
__device__ __forceinline__ void psp_fill_tab(PspTab* t, const PspGeom& g, int h, int w, int ac) {
    for (int q = threadIdx.x; q < 2 * SALT_PSP_MAX_STAGES * PSP_MAX_HW; q += 256) {
        const int d = q % PSP_MAX_HW, k = (q / PSP_MAX_HW) % SALT_PSP_MAX_STAGES, ax = q / (PSP_MAX_HW * SALT_PSP_MAX_STAGES);
        const int n = ax ? w : h;
        if (k < g.n && d < n) psp_src(d, n, g.s[k], ac, t->i0[ax][k][d], t->i1[ax][k][d], t->w0[ax][k][d], t->w1[ax][k][d]);
    }
}

// y = relu(f + bias + sum_k resize(q_k)): one workgroup per (image, 64-channel block)
template <typename T>
__global__ __launch_bounds__(256) void psp_merge_kernel(const T* f, int fcs, const float* bias, PspPtrs q, PspGeom g, int h, int w, int C, int ac, T* y, int ycs) {
    constexpr int N = Elem<T>::VE;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    PspTab* tab = reinterpret_cast<PspTab*>(smem);
    float* sq = reinterpret_cast<float*>(smem + sizeof(PspTab));              // [bins][PSP_CB]
    const int nblk = (C + PSP_CB - 1) / PSP_CB;
    const int b = blockIdx.x / nblk, c0 = (blockIdx.x % nblk) * PSP_CB;
    const int cb = C - c0 < PSP_CB ? C - c0 : PSP_CB, pieces = cb / N;
    psp_fill_tab(tab, g, h, w, ac);
    for (int it = threadIdx.x; it < g.bins * pieces; it += 256) {
        const int pc = it % pieces, bin = it / pieces, k = psp_stage_of(g, bin), s = g.s[k];
        Piece<T, true>::ld((const T*)q.p[k] + ((int64_t)b * s * s + (bin - g.off[k])) * q.cs[k] + c0 + pc * N, sq + bin * PSP_CB + pc * N);
    }
    __syncthreads();
    for (int it = threadIdx.x; it < h * w * pieces; it += 256) {
        const int pc = it % pieces, pix = it / pieces, yy = pix / w, xx = pix % w;
        const int64_t p = (int64_t)b * h * w + pix;
        float v[N];
        Piece<T, true>::ld(f + p * fcs + c0 + pc * N, v);
        if (bias) {
#pragma unroll
            for (int e = 0; e < N; ++e) v[e] += bias[c0 + pc * N + e];
        }
        for (int k = 0; k < g.n; ++k) {
            const int s = g.s[k];
            const float wy0 = tab->w0[0][k][yy], wy1 = tab->w1[0][k][yy], wx0 = tab->w0[1][k][xx], wx1 = tab->w1[1][k][xx];
            const float* r0 = sq + (g.off[k] + tab->i0[0][k][yy] * s) * PSP_CB + pc * N;
            const float* r1 = sq + (g.off[k] + tab->i1[0][k][yy] * s) * PSP_CB + pc * N;
            const int j0 = tab->i0[1][k][xx] * PSP_CB, j1 = tab->i1[1][k][xx] * PSP_CB;
            const float w00 = __fmul_rn(wy0, wx0), w01 = __fmul_rn(wy0, wx1), w10 = __fmul_rn(wy1, wx0), w11 = __fmul_rn(wy1, wx1);
#pragma unroll
            for (int e = 0; e < N; ++e) v[e] += w00 * r0[j0 + e] + w01 * r0[j1 + e] + w10 * r1[j0 + e] + w11 * r1[j1 + e];
        }
#pragma unroll
        for (int e = 0; e < N; ++e) v[e] = v[e] > 0.f ? v[e] : 0.f;
        Piece<T, true>::st(y + p * ycs + c0 + pc * N, v);
    }
}

// g = dy [y > 0] -> df;  dq_k[bin] = sum_pixels weight_k(pixel, bin) g[pixel] (a gather per bin, pixels in row-major order);  per-image
// partial of dbias.  One workgroup per (image, 64-channel block).  The gathers read dy and y BEFORE anything is written (the barrier
// in between), so df may be dy itself.
template <typename T>
__global__ __launch_bounds__(256) void psp_merge_bwd_kernel(const T* dy, int dycs, const T* y, int ycs, PspGeom g, int h, int w, int C, int ac,
                                                            T* df, int dfcs, PspPtrs dq, float* partials) {
    constexpr int N = Elem<T>::VE;
    __shared__ PspTab tab;
    __shared__ float wt[2][SALT_PSP_MAX_STAGES][PSP_MAX_HW][PSP_MAX_S];            // dense resize matrices [axis][stage][destination][source]
    const int nblk = (C + PSP_CB - 1) / PSP_CB;
    const int b = blockIdx.x / nblk, c0 = (blockIdx.x % nblk) * PSP_CB;
    const int cb = C - c0 < PSP_CB ? C - c0 : PSP_CB, pieces = cb / N;
    psp_fill_tab(&tab, g, h, w, ac);
    __syncthreads();
    for (int q = threadIdx.x; q < 2 * SALT_PSP_MAX_STAGES * PSP_MAX_HW; q += 256) {
        const int d = q % PSP_MAX_HW, k = (q / PSP_MAX_HW) % SALT_PSP_MAX_STAGES, ax = q / (PSP_MAX_HW * SALT_PSP_MAX_STAGES);
        if (k < g.n && d < (ax ? w : h)) {
            float* row = wt[ax][k][d];
#pragma unroll
            for (int i = 0; i < PSP_MAX_S; ++i) row[i] = 0.f;
            row[tab.i0[ax][k][d]] += tab.w0[ax][k][d];
            row[tab.i1[ax][k][d]] += tab.w1[ax][k][d];
        }
    }
    __syncthreads();
    const int64_t p0 = (int64_t)b * h * w;
    for (int it = threadIdx.x; it < (g.bins + 1) * pieces; it += 256) {
        const int pc = it % pieces, bin = it / pieces;
        const bool all = bin == g.bins;                                  // the pseudo-bin of dbias: every pixel, weight 1
        const int k = all ? 0 : psp_stage_of(g, bin), s = g.s[k], i = all ? 0 : (bin - g.off[k]) / s, j = all ? 0 : (bin - g.off[k]) % s;
        float acc[N];
#pragma unroll
        for (int e = 0; e < N; ++e) acc[e] = 0.f;
        for (int yy = 0; yy < h; ++yy) {
            const float wy = all ? 1.f : wt[0][k][yy][i];
            if (wy == 0.f) continue;
            for (int xx = 0; xx < w; ++xx) {
                const float wx = all ? 1.f : wt[1][k][xx][j];
                if (wx == 0.f) continue;
                const float wgt = __fmul_rn(wy, wx);
                float gv[N], yv[N];
                Piece<T, true>::ld(dy + (p0 + yy * w + xx) * dycs + c0 + pc * N, gv);
                Piece<T, true>::ld(y + (p0 + yy * w + xx) * ycs + c0 + pc * N, yv);
#pragma unroll
                for (int e = 0; e < N; ++e) acc[e] += wgt * (yv[e] > 0.f ? gv[e] : 0.f);
            }
        }
        if (all) {
#pragma unroll
            for (int e = 0; e < N; ++e) partials[(int64_t)b * C + c0 + pc * N + e] = acc[e];
        } else {
            Piece<T, true>::st((T*)dq.p[k] + ((int64_t)b * s * s + (bin - g.off[k])) * dq.cs[k] + c0 + pc * N, acc);
        }
    }
    __syncthreads();
    for (int it = threadIdx.x; it < h * w * pieces; it += 256) {
        const int pc = it % pieces, pix = it / pieces;
        float gv[N], yv[N];
        Piece<T, true>::ld(dy + (p0 + pix) * dycs + c0 + pc * N, gv);
        Piece<T, true>::ld(y + (p0 + pix) * ycs + c0 + pc * N, yv);
#pragma unroll
        for (int e = 0; e < N; ++e) gv[e] = yv[e] > 0.f ? gv[e] : 0.f;
        Piece<T, true>::st(df + (p0 + pix) * dfcs + c0 + pc * N, gv);
    }
}

// out[c] (+)= sum_r partials[r][c], rows ascending
__global__ __launch_bounds__(256) void psp_rowsum_kernel(const float* partials, int rows, int C, float* out, int accumulate) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    float s = partials[c];
    for (int r = 1; r < rows; ++r) s += partials[(int64_t)r * C + c];
    out[c] = accumulate ? out[c] + s : s;
}

// ---------------------------------------------------------------------------------------------------------------- BatchNorm apply + PReLU
// THE PRE-ACTIVATION IS PINNED: u = fmaf(y, scale[c], shift[c]) (u = y without scale / shift); forward and backward see the same u
template <typename T>
__device__ __forceinline__ void bnp_u(const T* yp, const float* scale, const float* shift, int c, float* u) {
    constexpr int N = Elem<T>::VE;
    Piece<T, true>::ld(yp, u);
    if (scale) {
#pragma unroll
        for (int e = 0; e < N; ++e) u[e] = __fmaf_rn(u[e], scale[c + e], shift[c + e]);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void bn_prelu_kernel(const T* y, int ycs, int64_t pixels, int C, const float* scale, const float* shift, const float* alpha,
                                                       T* a, int acs) {
    constexpr int N = Elem<T>::VE;
    const int cpv = C / N;
    const float al = *alpha;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < pixels * cpv; idx += (int64_t)gridDim.x * 256) {
        const int c = (int)(idx % cpv) * N;
        const int64_t p = idx / cpv;
        float u[N];
        bnp_u<T>(y + p * ycs + c, scale, shift, c, u);
#pragma unroll
        for (int e = 0; e < N; ++e) u[e] = u[e] > 0.f ? u[e] : __fmul_rn(al, u[e]);
        Piece<T, true>::st(a + p * acs + c, u);
    }
}

// du = da (u > 0 ? 1 : alpha);  partials[workgroup] = sum da min(u, 0): per-thread chains over the grid-stride loop, then the block tree
template <typename T>
__global__ __launch_bounds__(256) void bn_prelu_bwd_kernel(const T* da, int dacs, const T* y, int ycs, int64_t pixels, int C, const float* scale, const float* shift,
                                                           const float* alpha, T* du, int ducs, float* partials) {
    constexpr int N = Elem<T>::VE;
    __shared__ float sm4[4];
    const int cpv = C / N;
    const float al = *alpha;
    float part = 0.f;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < pixels * cpv; idx += (int64_t)gridDim.x * 256) {
        const int c = (int)(idx % cpv) * N;
        const int64_t p = idx / cpv;
        float u[N], g[N];
        bnp_u<T>(y + p * ycs + c, scale, shift, c, u);
        Piece<T, true>::ld(da + p * dacs + c, g);
#pragma unroll
        for (int e = 0; e < N; ++e) {
            if (!(u[e] > 0.f)) { part += g[e] * u[e]; g[e] = __fmul_rn(g[e], al); }
        }
        Piece<T, true>::st(du + p * ducs + c, g);
    }
    const float s = block_sum_256(part, sm4);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

__global__ __launch_bounds__(256) void bn_prelu_dalpha_kernel(const float* partials, int nparts, float* dalpha, int accumulate) {
    __shared__ float sm4[4];
    float part = 0.f;
    for (int i = threadIdx.x; i < nparts; i += 256) part += partials[i];
    const float s = block_sum_256(part, sm4);
    if (threadIdx.x == 0) *dalpha = accumulate ? *dalpha + s : s;
}

// ---------------------------------------------------------------------------------------------------------------- host
static int psp_geom(const char* op, int nsizes, const int* sizes, PspGeom* g) {
    if (nsizes < 1 || nsizes > SALT_PSP_MAX_STAGES) SALT_FAIL(SALT_E_UNSUPPORTED, "%s: %d pyramid sizes (1..%d)", op, nsizes, SALT_PSP_MAX_STAGES);
    *g = PspGeom{};
    g->n = nsizes;
    for (int k = 0; k < nsizes; ++k) {
        if (sizes[k] < 1 || sizes[k] > PSP_MAX_S) SALT_FAIL(SALT_E_UNSUPPORTED, "%s: pyramid size %d (1..%d)", op, sizes[k], PSP_MAX_S);
        g->s[k] = sizes[k];
        g->off[k] = g->bins;
        g->bins += sizes[k] * sizes[k];
    }
    return SALT_OK;
}
static int psp_dtype(const char* op, int dtype) {
    if (dtype != SALT_F32 && dtype != SALT_BF16) SALT_FAIL(SALT_E_BADARG, "%s: bad dtype %d", op, dtype);
    return SALT_OK;
}
// the full-resolution view fixes B, h, w, C: h, w <= 32, C a multiple of 8
static int psp_shape(const char* op, const salt_view& v) {
    if (!view_ok(v)) SALT_FAIL(SALT_E_BADARG, "%s: bad view", op);
    if (v.H > PSP_MAX_HW || v.W > PSP_MAX_HW) SALT_FAIL(SALT_E_UNSUPPORTED, "%s: %d x %d pixels (at most %d x %d)", op, v.H, v.W, PSP_MAX_HW, PSP_MAX_HW);
    if (v.C % 8) SALT_FAIL(SALT_E_UNSUPPORTED, "%s: %d channels (a multiple of 8)", op, v.C);
    if ((int64_t)v.B * v.H * v.W * v.cs >= (1ll << 31)) SALT_FAIL(SALT_E_UNSUPPORTED, "%s: view of 2^31 elements or more", op);
    return SALT_OK;
}
static int psp_stage_views(const char* op, const char* what, const salt_view* v, int dtype, const PspGeom& g, int B, int C, PspPtrs* out) {
    for (int k = 0; k < g.n; ++k) {
        SALT_TRY(view_check16(op, what, v[k], dtype, B, g.s[k], g.s[k], C));
        out->p[k] = v[k].p;
        out->cs[k] = v[k].cs;
    }
    return SALT_OK;
}

extern "C" int salt_psp_pool(const salt_psp_pool_args* a, void* stream) {
    if (!a) SALT_FAIL(SALT_E_BADARG, "psp_pool: null args");
    PspGeom g; PspPtrs out = {};
    SALT_TRY(psp_dtype("psp_pool", a->dtype));
    SALT_TRY(psp_geom("psp_pool", a->nsizes, a->sizes, &g));
    SALT_TRY(psp_shape("psp_pool", a->x));
    SALT_TRY(view_check16("psp_pool", "x", a->x, a->dtype, a->x.B, a->x.H, a->x.W, a->x.C));
    SALT_TRY(psp_stage_views("psp_pool", "p", a->p, a->dtype, g, a->x.B, a->x.C, &out));
    const int ve = a->dtype == SALT_F32 ? 4 : 8;
    const int64_t items = (int64_t)a->x.B * g.bins * (a->x.C / ve);
    SALT_DISPATCH_DTYPE(a->dtype, T, return salt_launch(psp_pool_kernel<T>, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                                                        (const T*)a->x.p, a->x.B, a->x.H, a->x.W, a->x.C, a->x.cs, g, out))
}

extern "C" int salt_psp_pool_bwd(const salt_psp_pool_bwd_args* a, void* stream) {
    if (!a) SALT_FAIL(SALT_E_BADARG, "psp_pool_bwd: null args");
    PspGeom g; PspPtrs dp = {};
    SALT_TRY(psp_dtype("psp_pool_bwd", a->dtype));
    SALT_TRY(psp_geom("psp_pool_bwd", a->nsizes, a->sizes, &g));
    SALT_TRY(psp_shape("psp_pool_bwd", a->dx));
    SALT_TRY(view_check16("psp_pool_bwd", "dx", a->dx, a->dtype, a->dx.B, a->dx.H, a->dx.W, a->dx.C));
    SALT_TRY(psp_stage_views("psp_pool_bwd", "dp", a->dp, a->dtype, g, a->dx.B, a->dx.C, &dp));
    const int ve = a->dtype == SALT_F32 ? 4 : 8;
    const int64_t items = view_pixels(a->dx) * (a->dx.C / ve);
    SALT_DISPATCH_DTYPE(a->dtype, T, return salt_launch(psp_pool_bwd_kernel<T>, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                                                        dp, a->dx.B, a->dx.H, a->dx.W, a->dx.C, g, (T*)a->dx.p, a->dx.cs, a->accumulate))
}

extern "C" int salt_psp_merge(const salt_psp_merge_args* a, void* stream) {
    if (!a) SALT_FAIL(SALT_E_BADARG, "psp_merge: null args");
    PspGeom g; PspPtrs q = {};
    SALT_TRY(psp_dtype("psp_merge", a->dtype));
    SALT_TRY(psp_geom("psp_merge", a->nsizes, a->sizes, &g));
    SALT_TRY(psp_shape("psp_merge", a->y));
    const int B = a->y.B, h = a->y.H, w = a->y.W, C = a->y.C;
    SALT_TRY(view_check16("psp_merge", "y", a->y, a->dtype, B, h, w, C));
    SALT_TRY(view_check16("psp_merge", "f", a->f, a->dtype, B, h, w, C));
    SALT_TRY(psp_stage_views("psp_merge", "q", a->q, a->dtype, g, B, C, &q));
    const size_t lds = sizeof(PspTab) + (size_t)g.bins * PSP_CB * sizeof(float);
    SALT_DISPATCH_DTYPE(a->dtype, T, return salt_launch(psp_merge_kernel<T>, dim3((unsigned)(B * cdiv(C, PSP_CB))), dim3(256), lds, (hipStream_t)stream,
                                                        (const T*)a->f.p, a->f.cs, a->bias, q, g, h, w, C, a->align_corners ? 1 : 0, (T*)a->y.p, a->y.cs))
}

extern "C" int salt_psp_merge_bwd_parts(const salt_psp_merge_bwd_args* a) {
    if (!a || a->dy.B < 1) SALT_FAIL(SALT_E_BADARG, "psp_merge_bwd: bad args");
    return a->dy.B;
}

extern "C" int salt_psp_merge_bwd(const salt_psp_merge_bwd_args* a, void* stream) {
    if (!a) SALT_FAIL(SALT_E_BADARG, "psp_merge_bwd: null args");
    PspGeom g; PspPtrs dq = {};
    SALT_TRY(psp_dtype("psp_merge_bwd", a->dtype));
    SALT_TRY(psp_geom("psp_merge_bwd", a->nsizes, a->sizes, &g));
    SALT_TRY(psp_shape("psp_merge_bwd", a->dy));
    const int B = a->dy.B, h = a->dy.H, w = a->dy.W, C = a->dy.C;
    SALT_TRY(view_check16("psp_merge_bwd", "dy", a->dy, a->dtype, B, h, w, C));
    SALT_TRY(view_check16("psp_merge_bwd", "y", a->y, a->dtype, B, h, w, C));
    SALT_TRY(view_check16("psp_merge_bwd", "df", a->df, a->dtype, B, h, w, C));
    SALT_TRY(psp_stage_views("psp_merge_bwd", "dq", a->dq, a->dtype, g, B, C, &dq));
    if (!a->partials || a->nparts != B) SALT_FAIL(SALT_E_BADARG, "psp_merge_bwd: partials [%d][%d] (salt_psp_merge_bwd_parts), nparts %d", B, C, a->nparts);
    SALT_DISPATCH_DTYPE(a->dtype, T, SALT_TRY(salt_launch(psp_merge_bwd_kernel<T>, dim3((unsigned)(B * cdiv(C, PSP_CB))), dim3(256), 0, (hipStream_t)stream,
                                                          (const T*)a->dy.p, a->dy.cs, (const T*)a->y.p, a->y.cs, g, h, w, C, a->align_corners ? 1 : 0,
                                                          (T*)a->df.p, a->df.cs, dq, a->partials)))
    if (!a->dbias) return SALT_OK;
    return salt_launch(psp_rowsum_kernel, dim3(cdiv(C, 256)), dim3(256), 0, (hipStream_t)stream, (const float*)a->partials, B, C, a->dbias, a->accumulate_dbias);
}

// any B, H, W; C a multiple of 8; 16-byte addressable views
static int bnp_views(const char* op, int dtype, const salt_view& y, const salt_view& o, const char* oname) {
    SALT_TRY(psp_dtype(op, dtype));
    if (!view_ok(y)) SALT_FAIL(SALT_E_BADARG, "%s: bad view", op);
    if (y.C % 8) SALT_FAIL(SALT_E_UNSUPPORTED, "%s: %d channels (a multiple of 8)", op, y.C);
    SALT_TRY(view_check16(op, "y", y, dtype, y.B, y.H, y.W, y.C));
    return view_check16(op, oname, o, dtype, y.B, y.H, y.W, y.C);
}
static int bnp_grid(const salt_view& y, int dtype) {
    const int64_t items = view_pixels(y) * (y.C / (dtype == SALT_F32 ? 4 : 8));
    const int64_t wgs = (items + 1023) / 1024;                          // four pieces per thread
    return (int)(wgs < 1 ? 1 : wgs > 1024 ? 1024 : wgs);
}

extern "C" int salt_bn_prelu(const salt_bn_prelu_args* a, void* stream) {
    if (!a) SALT_FAIL(SALT_E_BADARG, "bn_prelu: null args");
    SALT_TRY(bnp_views("bn_prelu", a->dtype, a->y, a->a, "a"));
    if (!a->alpha || (a->scale == nullptr) != (a->shift == nullptr)) SALT_FAIL(SALT_E_BADARG, "bn_prelu: alpha is required, scale / shift go together");
    SALT_DISPATCH_DTYPE(a->dtype, T, return salt_launch(bn_prelu_kernel<T>, dim3(bnp_grid(a->y, a->dtype)), dim3(256), 0, (hipStream_t)stream,
                                                        (const T*)a->y.p, a->y.cs, view_pixels(a->y), a->y.C, a->scale, a->shift, a->alpha, (T*)a->a.p, a->a.cs))
}

extern "C" int salt_bn_prelu_bwd_parts(const salt_bn_prelu_bwd_args* a) {
    if (!a || !view_ok(a->y) || (a->dtype != SALT_F32 && a->dtype != SALT_BF16)) SALT_FAIL(SALT_E_BADARG, "bn_prelu_bwd: bad args");
    return bnp_grid(a->y, a->dtype);
}

extern "C" int salt_bn_prelu_bwd(const salt_bn_prelu_bwd_args* a, void* stream) {
    if (!a) SALT_FAIL(SALT_E_BADARG, "bn_prelu_bwd: null args");
    SALT_TRY(bnp_views("bn_prelu_bwd", a->dtype, a->y, a->da, "da"));
    SALT_TRY(view_check16("bn_prelu_bwd", "du", a->du, a->dtype, a->y.B, a->y.H, a->y.W, a->y.C));
    if (!a->alpha || (a->scale == nullptr) != (a->shift == nullptr)) SALT_FAIL(SALT_E_BADARG, "bn_prelu_bwd: alpha is required, scale / shift go together");
    const int nparts = bnp_grid(a->y, a->dtype);
    if (!a->partials || !a->dalpha || a->nparts != nparts)
        SALT_FAIL(SALT_E_BADARG, "bn_prelu_bwd: partials [%d] (salt_bn_prelu_bwd_parts) and dalpha are required, nparts %d", nparts, a->nparts);
    SALT_DISPATCH_DTYPE(a->dtype, T, SALT_TRY(salt_launch(bn_prelu_bwd_kernel<T>, dim3(nparts), dim3(256), 0, (hipStream_t)stream, (const T*)a->da.p, a->da.cs,
                                                          (const T*)a->y.p, a->y.cs, view_pixels(a->y), a->y.C, a->scale, a->shift, a->alpha, (T*)a->du.p, a->du.cs,
                                                          a->partials)))
    return salt_launch(bn_prelu_dalpha_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)a->partials, nparts, a->dalpha, a->accumulate_dalpha);
}
