// depth.hip — the depth-conditioned channel gate of UNetResNetWithDepth (architectures/base.py:120-131,
// architectures/models_with_depth.py:56-76): s = sigmoid(Linear(1, C)(D)), hypercolumn * s[:, :, None, None].
// salt_depth_gate is the tiny [B][C] gate and its parameter gradients; salt_channel_gate scales ONE hypercolumn level at that level's
// own resolution (a per-image, per-channel factor commutes with bilinear up-sampling) and, backward, reduces dL/ds per image.
// The dL/ds reduction follows se.hip's protocol for the pooled channel sums: fp64 atomics into a zeroed [B][C] row (default) or
// per-part partials summed in a fixed order by a second launch (SALT_BN_FIN=0 / SALT_SE_SHARDS=0: bit-reproducible training).
#include "common.h"

namespace {

constexpr int UNR = 4;          // pixels in flight per thread (one 16-byte load each)

__global__ void depth_gate_fwd_kernel(const float* d, const float* w, const float* bias, int B, int C, float* s) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * C) return;
    const int b = i / C, j = i - b * C;
    const float t = __fmaf_rn(w[j], d[b], bias[j]);
    s[i] = 1.f / (1.f + expf(-t));
}

// one thread per channel, images in ascending order: the same bits on every run
__global__ void depth_gate_bwd_kernel(const float* d, const float* s, const float* ds, const double* ds_acc, int B, int C, float* gw, float* gb,
                                      int accumulate) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= C) return;
    float aw = 0.f, ab = 0.f;
    for (int b = 0; b < B; ++b) {
        const float g = ds ? ds[b * C + j] : (float)ds_acc[(int64_t)b * C + j];
        const float sv = s[b * C + j];
        const float t = g * sv * (1.f - sv);
        aw = __fmaf_rn(t, d[b], aw);
        ab += t;
    }
    gw[j] = accumulate ? gw[j] + aw : aw;
    gb[j] = accumulate ? gb[j] + ab : ab;
}

// y = x * s[b][c0 + c]: one workgroup per (image, pixel part); C / N lanes share a pixel (a wave reads 64 consecutive 16-byte pieces
// of a dense level), the gate of the lane's channels sits in registers
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void gate_fwd_kernel(salt_view x, salt_view y, const float* s, int sC, int c0, int nparts, int pix_per_part) {
    typedef Piece<T, VEC> P;
    constexpr int N = P::N;
    const int cpv = x.C / N, R = 256 / cpv;
    const int b = blockIdx.x / nparts, part = blockIdx.x % nparts;
    const int hw = x.H * x.W;
    const int p0 = part * pix_per_part, p1 = min(p0 + pix_per_part, hw);
    const int row = threadIdx.x / cpv, cv = threadIdx.x % cpv;
    if (row >= R) return;
    float sv[N];
#pragma unroll
    for (int j = 0; j < N; ++j) sv[j] = s[(int64_t)b * sC + c0 + cv * N + j];
    for (int pix = p0 + row; pix < p1; pix += UNR * R) {
        float f[UNR][N];
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            const int p = pix + u * R;
            if (p < p1) P::ld((const T*)x.p + ((int64_t)b * hw + p) * x.cs + cv * N, f[u]);
        }
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            const int p = pix + u * R;
            if (p < p1) {
#pragma unroll
                for (int j = 0; j < N; ++j) f[u][j] *= sv[j];
                P::st((T*)y.p + ((int64_t)b * hw + p) * y.cs + cv * N, f[u]);
            }
        }
    }
}

// dx (+)= dy * s; per (image, part): sum_pixels dy * x per channel (inplace: x holds x s, the sum is divided by s), rows combined in
// ascending order through LDS, then one fp64 atomic per channel (acc) or one partials row
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void gate_bwd_kernel(salt_view x, salt_view dy, salt_view dx, const float* s, int sC, int c0, int accumulate,
                                                       int inplace, float* partials, double* acc, int nparts, int pix_per_part) {
    typedef Piece<T, VEC> P;
    constexpr int N = P::N;
    extern __shared__ float sm[];                      // [R][C]
    const int C = x.C, cpv = C / N, R = 256 / cpv;
    const int b = blockIdx.x / nparts, part = blockIdx.x % nparts;
    const int hw = x.H * x.W;
    const int p0 = part * pix_per_part, p1 = min(p0 + pix_per_part, hw);
    const int row = threadIdx.x / cpv, cv = threadIdx.x % cpv;
    const bool live = row < R;
    float sv[N], sum[N];
#pragma unroll
    for (int j = 0; j < N; ++j) { sv[j] = live ? s[(int64_t)b * sC + c0 + cv * N + j] : 0.f; sum[j] = 0.f; }
    if (live) {
        for (int pix = p0 + row; pix < p1; pix += UNR * R) {
            float g[UNR][N], xv[UNR][N], old[UNR][N];
#pragma unroll
            for (int u = 0; u < UNR; ++u) {
                const int p = pix + u * R;
                if (p < p1) {
                    const int64_t gp = (int64_t)b * hw + p;
                    P::ld((const T*)dy.p + gp * dy.cs + cv * N, g[u]);
                    P::ld((const T*)x.p + gp * x.cs + cv * N, xv[u]);
                    if (accumulate) P::ld((const T*)dx.p + gp * dx.cs + cv * N, old[u]);
                }
            }
#pragma unroll
            for (int u = 0; u < UNR; ++u) {
                const int p = pix + u * R;
                if (p < p1) {
                    float o[N];
#pragma unroll
                    for (int j = 0; j < N; ++j) {
                        sum[j] = __fmaf_rn(g[u][j], xv[u][j], sum[j]);
                        o[j] = g[u][j] * sv[j];
                        if (accumulate) o[j] += old[u][j];
                    }
                    P::st((T*)dx.p + ((int64_t)b * hw + p) * dx.cs + cv * N, o);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < N; ++j) sm[row * C + cv * N + j] = sum[j];
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += 256) {
        float t = 0.f;
        for (int r = 0; r < R; ++r) t += sm[r * C + c];
        if (inplace) t = t / s[(int64_t)b * sC + c0 + c];
        if (acc) unsafeAtomicAdd(acc + (int64_t)b * sC + c0 + c, (double)t);
        else partials[((int64_t)b * nparts + part) * C + c] = t;
    }
}

// ds[b][c0 + c] = sum over the parts in ascending order
__global__ void gate_parts_reduce_kernel(const float* partials, int nparts, int C, float* ds, int sC, int c0) {
    const int b = blockIdx.x;
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
        float t = 0.f;
        for (int k = 0; k < nparts; ++k) t += partials[((int64_t)b * nparts + k) * C + c];
        ds[(int64_t)b * sC + c0 + c] = t;
    }
}

void gate_plan(const salt_view& x, int N, int* nparts, int* per) {
    const int cpv = x.C / N, R = 256 / cpv, hw = x.H * x.W;
    int np = cdiv(1024, x.B);                          // ~4 workgroups per CU over the batch
    const int most = cdiv(hw, R * UNR);                // at least one full sweep of the block per part
    if (np > most) np = most;
    if (np > 64) np = 64;                              // <= 64 atomic arrivals per address (se.hip)
    if (np < 1) np = 1;
    *per = cdiv(hw, np);
    *nparts = cdiv(hw, *per);
}

}  // namespace

extern "C" int salt_depth_gate(const salt_depth_gate_args* a, void* stream) {
    if (!a || !a->d || !a->s || a->B < 1 || a->C < 1) SALT_FAIL(SALT_E_BADARG, "depth_gate: bad args");
    hipStream_t st = (hipStream_t)stream;
    if (!a->backward) {
        if (!a->w || !a->bias) SALT_FAIL(SALT_E_BADARG, "depth_gate: no parameters");
        return salt_launch(depth_gate_fwd_kernel, dim3(cdiv(a->B * a->C, 256)), dim3(256), 0, st, a->d, a->w, a->bias, a->B, a->C, a->s);
    }
    if ((!a->ds && !a->ds_acc) || !a->gw || !a->gb) SALT_FAIL(SALT_E_BADARG, "depth_gate: backward needs ds or ds_acc, gw and gb");
    return salt_launch(depth_gate_bwd_kernel, dim3(cdiv(a->C, 64)), dim3(64), 0, st, a->d, a->s, a->ds, a->ds_acc, a->B, a->C, a->gw, a->gb, a->accumulate);
}

static int gate_check(const salt_channel_gate_args* a) {
    if (!a || !view_ok(a->x) || !view_ok(a->y) || !a->s || a->c0 < 0 || a->c0 + a->x.C > a->sC) SALT_FAIL(SALT_E_BADARG, "channel_gate: bad args");
    if (a->y.B != a->x.B || a->y.H != a->x.H || a->y.W != a->x.W || a->y.C != a->x.C) SALT_FAIL(SALT_E_BADARG, "channel_gate: x / y shapes differ");
    if (a->x.C > 2048) SALT_FAIL(SALT_E_UNSUPPORTED, "channel_gate: %d channels", a->x.C);
    return SALT_OK;
}

template <typename T> static int gate_n(const salt_channel_gate_args* a) {
    constexpr int VE = Elem<T>::VE;
    const bool vec = view_vec(a->x, VE) && view_vec(a->y, VE) && (!a->backward || view_vec(a->dx, VE)) && a->x.C / VE <= 256;
    if (!vec && a->x.C > 256) return 0;
    return vec ? VE : 1;
}

extern "C" int salt_channel_gate_parts(const salt_channel_gate_args* a) {
    if (!a || a->x.B < 1 || a->x.H < 1 || a->x.W < 1 || a->x.C < 1) return -1;
    int N = 1;
    if (a->dtype == SALT_F32) N = (a->x.C % 4 == 0 && a->x.cs % 4 == 0 && a->x.C / 4 <= 256) ? 4 : 1;
    else N = (a->x.C % 8 == 0 && a->x.cs % 8 == 0 && a->x.C / 8 <= 256) ? 8 : 1;
    if (N == 1 && a->x.C > 256) return -1;
    int nparts, per;
    gate_plan(a->x, N, &nparts, &per);
    return nparts;
}

extern "C" int salt_channel_gate(const salt_channel_gate_args* a, void* stream) {
    const int rc = gate_check(a);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    SALT_DISPATCH_DTYPE(a->dtype, T, {
        const int N = gate_n<T>(a);
        if (!N) SALT_FAIL(SALT_E_UNSUPPORTED, "channel_gate: %d channels without 16-byte rows", a->x.C);
        int nparts, per;
        gate_plan(a->x, N, &nparts, &per);
        const dim3 grid(a->x.B * nparts);
        if (!a->backward) {
            if (N > 1) return salt_launch(gate_fwd_kernel<T, true>, grid, dim3(256), 0, st, a->x, a->y, a->s, a->sC, a->c0, nparts, per);
            return salt_launch(gate_fwd_kernel<T, false>, grid, dim3(256), 0, st, a->x, a->y, a->s, a->sC, a->c0, nparts, per);
        } else {
            if (!view_ok(a->dx) || a->dx.B != a->x.B || a->dx.H != a->x.H || a->dx.W != a->x.W || a->dx.C != a->x.C)
                SALT_FAIL(SALT_E_BADARG, "channel_gate: dx shape");
            if (a->ds ? (!a->partials || a->nparts != nparts) : !a->ds_acc)
                SALT_FAIL(SALT_E_BADARG, "channel_gate: backward needs ds + partials (nparts %d, expected %d) or ds_acc", a->nparts, nparts);
            if (a->inplace && a->accumulate) SALT_FAIL(SALT_E_BADARG, "channel_gate: inplace backward overwrites dy");
            const int R = 256 / (a->x.C / N);
            const size_t lds = (size_t)R * a->x.C * sizeof(float);
            float* parts = a->ds ? a->partials : nullptr;
            double* acc = a->ds ? nullptr : a->ds_acc;
            if (N > 1) SALT_TRY(salt_launch(gate_bwd_kernel<T, true>, grid, dim3(256), lds, st, a->x, a->y, a->dx, a->s, a->sC, a->c0, a->accumulate,
                                            a->inplace, parts, acc, nparts, per));
            else SALT_TRY(salt_launch(gate_bwd_kernel<T, false>, grid, dim3(256), lds, st, a->x, a->y, a->dx, a->s, a->sC, a->c0, a->accumulate,
                                      a->inplace, parts, acc, nparts, per));
            if (a->ds) SALT_TRY(salt_launch(gate_parts_reduce_kernel, dim3(a->x.B), dim3(256), 0, st, a->partials, nparts, a->x.C, a->ds, a->sC, a->c0));
        }
    });
    return SALT_OK;
}
