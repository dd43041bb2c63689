// classifier.hip — the head of EmptinessClassifier (architectures/misc.py:70-71,80): nn.AvgPool2d(8) followed by a 1x1 convolution to
// K <= 8 logits on the pooled map.  salt_pool_head is ONE launch: a workgroup per 8x8 window averages the window per channel
// and contracts the pooled vector with the fp32 weight; the logits come out as fp32 NCHW, the layout the loss kernels read.  Training
// keeps the pooled vector ([B,OH,OW,C] fp32, 1/64 of the layer4 map), so salt_pool_head_bwd never reads the activation again: its one
// launch spreads W^T dlogits / 64 over the windows (dx), zeroes what no window covers, and sums gW / gb in a fixed order (no atomics:
// the same bits on every run).
// The window sums, the K dot products and the gW / gb sums are carried in fp64 and rounded to fp32 ONCE where they are stored: a logit
// is a signed sum over up to 2048 channels and may cancel to far below its terms, and a [B,2,1,1] output has no larger neighbour to
// hide an fp32 accumulation error behind.  The operator is launch-bound (it reads 2 MB at the workload's shape), so the fp64 adds
// cost nothing that can be measured.
#include "common.h"

namespace {

constexpr int POOL = 8;                 // nn.AvgPool2d(8): window side, window step
constexpr int NPIX = POOL * POOL;
constexpr int KMAX = 8;

// One workgroup per window (b, oh, ow).  `lanes` = min(C / N, 256) threads share a pixel (consecutive 16-byte pieces), 256 / lanes pixel
// rows walk the 64 pixels; the rows' partial sums meet in LDS in ascending row order, then every thread owns channels c = tid, tid + 256,
// ...: pooled value, K partial dot products, wave shuffles, one LDS step.
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void pool_head_kernel(salt_view x, const float* w, const float* bias, int K, int OH, int OW, float* logits,
                                                        float* pooled) {
    typedef Piece<T, VEC> P;
    constexpr int N = P::N;
    extern __shared__ double sm[];                     // [R][C]
    __shared__ double red[4][KMAX];
    const int C = x.C, cpv = C / N;
    const int lanes = cpv < 256 ? cpv : 256, R = 256 / lanes;
    const int wid = blockIdx.x;
    const int ow = wid % OW, oh = (wid / OW) % OH, b = wid / (OW * OH);
    const int row = threadIdx.x / lanes, cv = threadIdx.x % lanes;
    const T* base = (const T*)x.p + (((int64_t)b * x.H + oh * POOL) * x.W + ow * POOL) * x.cs;
    if (row < R) {
        for (int piece = cv; piece < cpv; piece += lanes) {
            double acc[N];
#pragma unroll
            for (int j = 0; j < N; ++j) acc[j] = 0.0;
            for (int pix = row; pix < NPIX; pix += R) {
                float f[N];
                P::ld(base + ((int64_t)(pix / POOL) * x.W + (pix % POOL)) * x.cs + piece * N, f);
#pragma unroll
                for (int j = 0; j < N; ++j) acc[j] += (double)f[j];
            }
#pragma unroll
            for (int j = 0; j < N; ++j) sm[row * C + piece * N + j] = acc[j];
        }
    }
    __syncthreads();
    double part[KMAX];
#pragma unroll
    for (int j = 0; j < KMAX; ++j) part[j] = 0.0;
    for (int c = threadIdx.x; c < C; c += 256) {
        double t = 0.0;
        for (int r = 0; r < R; ++r) t += sm[r * C + c];
        t *= 1.0 / NPIX;
        if (pooled) pooled[(int64_t)wid * C + c] = (float)t;
#pragma unroll
        for (int j = 0; j < KMAX; ++j)
            if (j < K) part[j] = fma((double)w[j * C + c], t, part[j]);
    }
#pragma unroll
    for (int j = 0; j < KMAX; ++j) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) part[j] += __shfl_xor(part[j], o);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int j = 0; j < KMAX; ++j) red[threadIdx.x >> 6][j] = part[j];
    }
    __syncthreads();
    if (threadIdx.x < K) {
        const int j = threadIdx.x;
        const double v = (red[0][j] + red[1][j]) + (red[2][j] + red[3][j]);
        logits[(((int64_t)b * K + j) * OH + oh) * OW + ow] = (float)(v + (bias ? (double)bias[j] : 0.0));
    }
}

// Backward, one launch, three kinds of workgroup:
//   [0, nwin)                  one window each: g[c] = (1/64) sum_j W[j][c] dlogits[b][j][oh][ow] per piece in registers, stored to (or
//                              added to) the window's 64 pixels
//   [nwin, nwin + nedge)       accumulate == 0 only: zero the pixels below / right of the last whole window
//   [nwin + nedge, +ngw)       256 channels each: gW[j][c] = sum over the windows in ascending order of dlogits pooled
//   last                       gb[j] = sum over the windows in ascending order of dlogits
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void pool_head_bwd_kernel(salt_view dx, const float* w, int K, int OH, int OW, const float* dl, const float* pooled,
                                                            int accumulate, float* gw, float* gb, int nwin, int nedge, int edge_per_image, int ngw) {
    typedef Piece<T, VEC> P;
    constexpr int N = P::N;
    const int C = dx.C, cpv = C / N;
    int blk = blockIdx.x;
    if (blk < nwin) {
        const int lanes = cpv < 256 ? cpv : 256, R = 256 / lanes;
        const int ow = blk % OW, oh = (blk / OW) % OH, b = blk / (OW * OH);
        const int row = threadIdx.x / lanes, cv = threadIdx.x % lanes;
        if (row >= R) return;
        float dv[KMAX];
#pragma unroll
        for (int j = 0; j < KMAX; ++j) dv[j] = j < K ? dl[(((int64_t)b * K + j) * OH + oh) * OW + ow] : 0.f;
        T* base = (T*)dx.p + (((int64_t)b * dx.H + oh * POOL) * dx.W + ow * POOL) * dx.cs;
        for (int piece = cv; piece < cpv; piece += lanes) {
            float g[N];
#pragma unroll
            for (int i = 0; i < N; ++i) {
                float a = 0.f;
#pragma unroll
                for (int j = 0; j < KMAX; ++j)
                    if (j < K) a = __fmaf_rn(w[j * C + piece * N + i], dv[j], a);
                g[i] = a * (1.f / NPIX);
            }
            for (int pix = row; pix < NPIX; pix += R) {
                T* q = base + ((int64_t)(pix / POOL) * dx.W + (pix % POOL)) * dx.cs + piece * N;
                float o[N];
                if (accumulate) {
                    P::ld(q, o);
#pragma unroll
                    for (int i = 0; i < N; ++i) o[i] += g[i];
                } else {
#pragma unroll
                    for (int i = 0; i < N; ++i) o[i] = g[i];
                }
                P::st(q, o);
            }
        }
        return;
    }
    blk -= nwin;
    if (blk < nedge) {
        // the pixels no window covers: rows [8 OH, H) whole, then columns [8 OW, W) of the rows above
        const int b = blk / edge_per_image, part = blk % edge_per_image;
        const int h0 = OH * POOL, w0 = OW * POOL;
        const int nb = (dx.H - h0) * dx.W, nr = h0 * (dx.W - w0);
        const int64_t units = (int64_t)(nb + nr) * cpv;
        float z[N];
#pragma unroll
        for (int i = 0; i < N; ++i) z[i] = 0.f;
        for (int64_t u = (int64_t)part * 256 + threadIdx.x; u < units; u += (int64_t)edge_per_image * 256) {
            const int e = (int)(u / cpv), piece = (int)(u % cpv);
            int h, x0;
            if (e < nb) { h = h0 + e / dx.W; x0 = e % dx.W; }
            else { const int e2 = e - nb, rw = dx.W - w0; h = e2 / rw; x0 = w0 + e2 % rw; }
            P::st((T*)dx.p + (((int64_t)b * dx.H + h) * dx.W + x0) * dx.cs + piece * N, z);
        }
        return;
    }
    blk -= nedge;
    const int NW = (dx.B * OH) * OW;
    if (blk < ngw) {
        const int c = blk * 256 + threadIdx.x;
        if (c >= C) return;
        double a[KMAX];
#pragma unroll
        for (int j = 0; j < KMAX; ++j) a[j] = 0.0;
        const int hw = OH * OW;
        for (int n = 0; n < NW; ++n) {
            const double pv = (double)pooled[(int64_t)n * C + c];
            const int b = n / hw, r = n - b * hw;
#pragma unroll
            for (int j = 0; j < KMAX; ++j)
                if (j < K) a[j] = fma((double)dl[((int64_t)b * K + j) * hw + r], pv, a[j]);
        }
#pragma unroll
        for (int j = 0; j < KMAX; ++j)
            if (j < K) gw[j * C + c] = (float)a[j];
        return;
    }
    if (gb && threadIdx.x < K) {
        const int j = threadIdx.x, hw = OH * OW;
        double s = 0.0;
        for (int n = 0; n < NW; ++n) {
            const int b = n / hw, r = n - b * hw;
            s += (double)dl[((int64_t)b * K + j) * hw + r];
        }
        gb[j] = (float)s;
    }
}

// LDS of the forward kernel: [R][C] doubles, R C <= 256 N when C / N < 256, one row otherwise
size_t pool_lds(int C, int N) {
    const int cpv = C / N, lanes = cpv < 256 ? cpv : 256;
    return (size_t)(256 / lanes) * C * sizeof(double);
}

bool shape_ok(const salt_view& v) { return v.B > 0 && v.H >= POOL && v.W >= POOL && v.C > 0 && v.cs >= v.C; }

}  // namespace

extern "C" int salt_pool_head(const salt_pool_head_args* a, void* stream) {
    if (!a || !a->x.p || !shape_ok(a->x) || !a->w || !a->logits_nchw || a->K < 1 || a->K > KMAX)
        SALT_FAIL(SALT_E_BADARG, "pool_head: bad args (x [B,H>=8,W>=8,C], 1 <= K <= 8, w and logits required)");
    const int OH = a->x.H / POOL, OW = a->x.W / POOL;
    if ((int64_t)a->x.B * OH * OW > 0x7fffffffLL) SALT_FAIL(SALT_E_BADARG, "pool_head: too many windows");
    const dim3 grid(a->x.B * OH * OW);
    hipStream_t st = (hipStream_t)stream;
    SALT_DISPATCH_DTYPE(a->dtype, T, {
        const bool vec = view_vec(a->x, Elem<T>::VE);
        const size_t lds = pool_lds(a->x.C, vec ? Elem<T>::VE : 1);
        if (lds > 48 * 1024) SALT_FAIL(SALT_E_UNSUPPORTED, "pool_head: %d channels", a->x.C);
        if (vec) return salt_launch(pool_head_kernel<T, true>, grid, dim3(256), lds, st, a->x, a->w, a->bias, a->K, OH, OW, a->logits_nchw, a->pooled);
        return salt_launch(pool_head_kernel<T, false>, grid, dim3(256), lds, st, a->x, a->w, a->bias, a->K, OH, OW, a->logits_nchw, a->pooled);
    });
}

extern "C" int salt_pool_head_bwd(const salt_pool_head_bwd_args* a, void* stream) {
    if (!a || !shape_ok(a->dx) || !a->w || !a->dlogits_nchw || !a->pooled || !a->gw || a->K < 1 || a->K > KMAX)
        SALT_FAIL(SALT_E_BADARG, "pool_head_bwd: bad args (dx shape [B,H>=8,W>=8,C], 1 <= K <= 8, w, dlogits, pooled and gw required)");
    const salt_view& v = a->dx;
    const int OH = v.H / POOL, OW = v.W / POOL;
    if ((int64_t)v.B * OH * OW > 0x3fffffffLL) SALT_FAIL(SALT_E_BADARG, "pool_head_bwd: too many windows");
    hipStream_t st = (hipStream_t)stream;
    SALT_DISPATCH_DTYPE(a->dtype, T, {
        const bool vec = v.p && view_vec(v, Elem<T>::VE);
        const int N = vec ? Elem<T>::VE : 1;
        const int nwin = v.p ? v.B * OH * OW : 0;
        const int64_t edge_units = (int64_t)(v.H * v.W - OH * OW * NPIX) * (v.C / N);
        int per_image = 0;
        if (v.p && !a->accumulate && edge_units > 0) per_image = (int)(edge_units < 64 * 256 ? (edge_units + 255) / 256 : 64);
        const int nedge = per_image * v.B, ngw = cdiv(v.C, 256);
        const dim3 grid(nwin + nedge + ngw + 1);
        if (vec) return salt_launch(pool_head_bwd_kernel<T, true>, grid, dim3(256), 0, st, v, a->w, a->K, OH, OW, a->dlogits_nchw, a->pooled,
                                    a->accumulate, a->gw, a->gb, nwin, nedge, per_image, ngw);
        return salt_launch(pool_head_bwd_kernel<T, false>, grid, dim3(256), 0, st, v, a->w, a->K, OH, OW, a->dlogits_nchw, a->pooled,
                           a->accumulate, a->gw, a->gb, nwin, nedge, per_image, ngw);
    });
}
