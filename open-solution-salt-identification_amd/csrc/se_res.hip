// se_res.hip — tail of the SE-ResNet bottleneck (public pretrainedmodels senet.py, SEResNetBottleneck.forward, reached through the
// reference's architectures/encoders.py:48-83):  y = relu(gate * bn3(conv3(a)) + shortcut),  gate = sigmoid(fc2(relu(fc1(mean_hw z)))).
// Bandwidth-bound: forward = pooling pass over the RAW convolution output (mean z = scale mean(x) + shift), a per-image FC launch
// that streams w1 / w2 from global memory (1 MB each at C = 2048: never staged in LDS), one apply pass.  Backward = one reduction
// pass (sum_hw m z), the per-image FC backward, one apply pass (dL/dz and dL/dshortcut), and a parameter-gradient launch that the
// engine puts on the weight-gradient queue.  Every streaming kernel uses one decomposition: a workgroup owns (image, pixel part,
// channel chunk of `cw` channels), cw the largest power of two <= 512 that divides C; a thread owns one 16-byte piece of a pixel row.
#include "common.h"

namespace {

// the one expression for z in the three kernels that need it (the FC on the pooled mean, the forward apply, the backward reduction): they
// must agree on the value
__device__ __forceinline__ float z_of(float x, float sc, float sh) { return __fmaf_rn(x, sc, sh); }

struct Tile {            // (image, pixel range, first channel) of a workgroup and (row, piece) of a thread
    int b, p0, p1, c, row, rows;
};
__device__ __forceinline__ Tile tile_of(int nparts, int nchunks, int pix_per_part, int hw, int pc_log2, int N) {
    Tile t;
    const int chunk = blockIdx.x % nchunks, bp = blockIdx.x / nchunks;
    t.b = bp / nparts;
    const int part = bp % nparts;
    t.p0 = part * pix_per_part;
    t.p1 = min(t.p0 + pix_per_part, hw);
    t.row = threadIdx.x >> pc_log2;
    t.rows = 256 >> pc_log2;
    t.c = ((chunk << pc_log2) + (threadIdx.x & ((1 << pc_log2) - 1))) * N;
    return t;
}

// Cross-row sums of the per-thread channel sums s[N] (rows in ascending order), then ONE fp64 atomic per channel (acc) or one
// partial per channel (partials[b][part][C]) per workgroup.  sm: 256 * N floats.
template <int N>
__device__ __forceinline__ void block_channel_sums(const float* s, float* sm, const Tile& t, int pc_log2, int C, int nparts, int nchunks, double* acc,
                                                   float* partials) {
    const int cw = N << pc_log2;
#pragma unroll
    for (int j = 0; j < N; ++j) sm[t.row * cw + (threadIdx.x & ((1 << pc_log2) - 1)) * N + j] = s[j];
    __syncthreads();
    const int chunk = blockIdx.x % nchunks, part = (blockIdx.x / nchunks) % nparts;
    for (int k = threadIdx.x; k < cw; k += 256) {
        float v = 0.f;
        for (int r = 0; r < t.rows; ++r) v += sm[r * cw + k];
        const int c = chunk * cw + k;
        if (acc) unsafeAtomicAdd(acc + (int64_t)t.b * C + c, (double)v);
        else partials[((int64_t)t.b * nparts + part) * C + c] = v;
    }
}

// forward pass 1: per-image channel sums of the raw x
template <typename T>
__global__ __launch_bounds__(256) void se_res_pool_kernel(salt_view x, int nparts, int nchunks, int pix_per_part, int pc_log2, double* acc, float* partials) {
    constexpr int N = Piece<T, true>::N;
    __shared__ float sm[256 * N];
    const int hw = x.H * x.W;
    const Tile t = tile_of(nparts, nchunks, pix_per_part, hw, pc_log2, N);
    float s[N];
#pragma unroll
    for (int j = 0; j < N; ++j) s[j] = 0.f;
    for (int pix = t.p0 + t.row; pix < t.p1; pix += t.rows) {
        float f[N];
        Piece<T, true>::ld((const T*)x.p + ((int64_t)t.b * hw + pix) * x.cs + t.c, f);
#pragma unroll
        for (int j = 0; j < N; ++j) s[j] += f[j];
    }
    block_channel_sums<N>(s, sm, t, pc_log2, x.C, nparts, nchunks, acc, partials);
}

// forward pass 2, one workgroup per image: [finalize the BatchNorm in front] gap -> hidden -> gate.  sm: [C] gap, [R] hidden, and with
// FIN [C] scale, [C] shift.
template <bool FIN>
__global__ __launch_bounds__(256) void se_res_fc_kernel(const double* acc, const float* partials, int nparts, int C, int R, float inv_hw, const float* in_scale,
                                                        const float* in_shift, BnFin fin, const float* w1, const float* b1, const float* w2, const float* b2,
                                                        float* gap, float* hidden, float* gate) {
    extern __shared__ float sm[];
    float* sg = sm; float* shid = sm + C;
    const int b = blockIdx.x, tid = threadIdx.x;
    if constexpr (FIN) {
        float* ssc = sm + C + R;
        fin_forward_consumer(fin, C, ssc, ssc + C, blockIdx.x == 0);
        __syncthreads();
        in_scale = ssc; in_shift = ssc + C;
    }
    for (int c = tid; c < C; c += 256) {
        float t;
        if (acc) t = (float)(acc[(int64_t)b * C + c] * (double)inv_hw);
        else {
            t = 0.f;
            for (int k = 0; k < nparts; ++k) t += partials[((int64_t)b * nparts + k) * C + c];
            t *= inv_hw;
        }
        if (in_scale) t = z_of(t, in_scale[c], in_shift[c]);
        sg[c] = t; gap[(int64_t)b * C + c] = t;
    }
    __syncthreads();
    // hidden: one wave per r, lanes across c (w1 rows are read as whole lines)
    const int lane = tid & 63, wave = tid >> 6;
    for (int r = wave; r < R; r += 4) {
        float t = 0.f;
        for (int c = lane; c < C; c += 64) t = __fmaf_rn(w1[(int64_t)r * C + c], sg[c], t);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o);
        if (lane == 0) { t = fmaxf(t + b1[r], 0.f); shid[r] = t; hidden[(int64_t)b * R + r] = t; }
    }
    __syncthreads();
    // gate: one thread per c, its w2 row as 16-byte loads (R is a multiple of 4)
    for (int c = tid; c < C; c += 256) {
        float t = b2[c];
        const f32x4* row = reinterpret_cast<const f32x4*>(w2 + (int64_t)c * R);
        for (int r4 = 0; r4 < R / 4; ++r4) {
            const f32x4 w = row[r4];
            t = __fmaf_rn(w.x, shid[4 * r4], t); t = __fmaf_rn(w.y, shid[4 * r4 + 1], t);
            t = __fmaf_rn(w.z, shid[4 * r4 + 2], t); t = __fmaf_rn(w.w, shid[4 * r4 + 3], t);
        }
        gate[(int64_t)b * C + c] = 1.f / (1.f + expf(-t));      // (expf, not __expf: B x C values, and the gate multiplies every element)
    }
}

// forward pass 3: y = relu(gate z + res)
template <typename T>
__global__ __launch_bounds__(256) void se_res_apply_kernel(salt_view x, salt_view res, salt_view y, const float* in_scale, const float* in_shift, const float* gate,
                                                           int nparts, int nchunks, int pix_per_part, int pc_log2) {
    constexpr int N = Piece<T, true>::N;
    const int hw = x.H * x.W;
    const Tile t = tile_of(nparts, nchunks, pix_per_part, hw, pc_log2, N);
    float g[N], sc[N], sh[N];
#pragma unroll
    for (int j = 0; j < N; ++j) {
        g[j] = gate[(int64_t)t.b * x.C + t.c + j];
        sc[j] = in_scale ? in_scale[t.c + j] : 1.f; sh[j] = in_scale ? in_shift[t.c + j] : 0.f;
    }
    for (int pix = t.p0 + t.row; pix < t.p1; pix += t.rows) {
        const int64_t gp = (int64_t)t.b * hw + pix;
        float f[N], r[N];
        Piece<T, true>::ld((const T*)x.p + gp * x.cs + t.c, f);
        Piece<T, true>::ld((const T*)res.p + gp * res.cs + t.c, r);
#pragma unroll
        for (int j = 0; j < N; ++j) f[j] = fmaxf(__fmaf_rn(g[j], in_scale ? z_of(f[j], sc[j], sh[j]) : f[j], r[j]), 0.f);
        Piece<T, true>::st((T*)y.p + gp * y.cs + t.c, f);
    }
}

// backward pass 1: per-image sums of m z, m = dy [y > 0]
template <typename T>
__global__ __launch_bounds__(256) void se_res_bwd_reduce_kernel(salt_view x, salt_view y, salt_view dy, const float* in_scale, const float* in_shift, int nparts,
                                                                int nchunks, int pix_per_part, int pc_log2, double* acc, float* partials) {
    constexpr int N = Piece<T, true>::N;
    __shared__ float sm[256 * N];
    const int hw = x.H * x.W;
    const Tile t = tile_of(nparts, nchunks, pix_per_part, hw, pc_log2, N);
    float s[N], sc[N], sh[N];
#pragma unroll
    for (int j = 0; j < N; ++j) { s[j] = 0.f; sc[j] = in_scale ? in_scale[t.c + j] : 1.f; sh[j] = in_scale ? in_shift[t.c + j] : 0.f; }
    for (int pix = t.p0 + t.row; pix < t.p1; pix += t.rows) {
        const int64_t gp = (int64_t)t.b * hw + pix;
        float f[N], o[N], d[N];
        Piece<T, true>::ld((const T*)x.p + gp * x.cs + t.c, f);
        Piece<T, true>::ld((const T*)y.p + gp * y.cs + t.c, o);
        Piece<T, true>::ld((const T*)dy.p + gp * dy.cs + t.c, d);
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const float z = in_scale ? z_of(f[j], sc[j], sh[j]) : f[j];
            s[j] += o[j] > 0.f ? d[j] * z : 0.f;
        }
    }
    block_channel_sums<N>(s, sm, t, pc_log2, x.C, nparts, nchunks, acc, partials);
}

// backward pass 2, one workgroup per image: dgate -> du -> dh -> dgap (scaled by 1 / HW).  sm: [C] du, [R] dh, [256] partial sums
__global__ __launch_bounds__(256) void se_res_fc_bwd_kernel(const double* acc, const float* partials, int nparts, int C, int R, float inv_hw, const float* w1,
                                                            const float* w2, const float* hidden, const float* gate, float* du, float* dh, float* dgap) {
    extern __shared__ float sm[];
    float* sdu = sm; float* sdh = sm + C; float* sp = sm + C + R;
    const int b = blockIdx.x, tid = threadIdx.x;
    for (int c = tid; c < C; c += 256) {
        float t;
        if (acc) t = (float)acc[(int64_t)b * C + c];
        else {
            t = 0.f;
            for (int k = 0; k < nparts; ++k) t += partials[((int64_t)b * nparts + k) * C + c];
        }
        const float g = gate[(int64_t)b * C + c];
        t = t * g * (1.f - g);
        sdu[c] = t; du[(int64_t)b * C + c] = t;
    }
    __syncthreads();
    // dh[r] = sum_c du[c] w2[c][r]: threads across r (adjacent addresses), 256 / R slices of c, slices combined in ascending order
    const int nsl = 256 / R, r = tid % R, sl = tid / R;
    if (sl < nsl) {
        float t = 0.f;
        for (int c = sl; c < C; c += nsl) t = __fmaf_rn(sdu[c], w2[(int64_t)c * R + r], t);
        sp[sl * R + r] = t;
    }
    __syncthreads();
    if (tid < R) {
        float t = 0.f;
        for (int k = 0; k < nsl; ++k) t += sp[k * R + tid];
        t = hidden[(int64_t)b * R + tid] > 0.f ? t : 0.f;
        sdh[tid] = t; dh[(int64_t)b * R + tid] = t;
    }
    __syncthreads();
    for (int c = tid; c < C; c += 256) {
        float t = 0.f;
        for (int k = 0; k < R; ++k) t = __fmaf_rn(sdh[k], w1[(int64_t)k * C + c], t);
        dgap[(int64_t)b * C + c] = t * inv_hw;
    }
}

// backward pass 3: dx = m gate + dgap, dres (+)= m.  dx may alias dy (a thread reads its piece of dy before it writes it).
template <typename T>
__global__ __launch_bounds__(256) void se_res_bwd_apply_kernel(salt_view y, salt_view dy, const float* gate, const float* dgap, salt_view dx, salt_view dres,
                                                               int accumulate_dres, int nparts, int nchunks, int pix_per_part, int pc_log2) {
    constexpr int N = Piece<T, true>::N;
    const int hw = y.H * y.W;
    const Tile t = tile_of(nparts, nchunks, pix_per_part, hw, pc_log2, N);
    float g[N], dg[N];
#pragma unroll
    for (int j = 0; j < N; ++j) { g[j] = gate[(int64_t)t.b * y.C + t.c + j]; dg[j] = dgap[(int64_t)t.b * y.C + t.c + j]; }
    for (int pix = t.p0 + t.row; pix < t.p1; pix += t.rows) {
        const int64_t gp = (int64_t)t.b * hw + pix;
        float o[N], d[N], q[N];
        Piece<T, true>::ld((const T*)y.p + gp * y.cs + t.c, o);
        Piece<T, true>::ld((const T*)dy.p + gp * dy.cs + t.c, d);
#pragma unroll
        for (int j = 0; j < N; ++j) d[j] = o[j] > 0.f ? d[j] : 0.f;
        T* pr = (T*)dres.p + gp * dres.cs + t.c;
        if (accumulate_dres) {
            Piece<T, true>::ld(pr, q);
#pragma unroll
            for (int j = 0; j < N; ++j) q[j] += d[j];
            Piece<T, true>::st(pr, q);
        } else Piece<T, true>::st(pr, d);
#pragma unroll
        for (int j = 0; j < N; ++j) q[j] = __fmaf_rn(d[j], g[j], dg[j]);
        Piece<T, true>::st((T*)dx.p + gp * dx.cs + t.c, q);
    }
}

// parameter gradients, one thread per output, images in ascending order: [C R] g_w2, [C] g_b2, [R C] g_w1, [R] g_b1
__global__ __launch_bounds__(256) void se_res_fc_grads_kernel(int B, int C, int R, const float* du, const float* dh, const float* gap, const float* hidden,
                                                              float* g_w1, float* g_b1, float* g_w2, float* g_b2) {
    const int n = 2 * C * R + C + R;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        float t = 0.f;
        if (i < C * R) {
            const int c = i / R, r = i - c * R;
            for (int b = 0; b < B; ++b) t = __fmaf_rn(du[(int64_t)b * C + c], hidden[(int64_t)b * R + r], t);
            g_w2[i] = t;
        } else if (i < C * R + C) {
            const int c = i - C * R;
            for (int b = 0; b < B; ++b) t += du[(int64_t)b * C + c];
            g_b2[c] = t;
        } else if (i < 2 * C * R + C) {
            const int k = i - C * R - C, r = k / C, c = k - r * C;
            for (int b = 0; b < B; ++b) t = __fmaf_rn(dh[(int64_t)b * R + r], gap[(int64_t)b * C + c], t);
            g_w1[k] = t;
        } else {
            const int r = i - 2 * C * R - C;
            for (int b = 0; b < B; ++b) t += dh[(int64_t)b * R + r];
            g_b1[r] = t;
        }
    }
}

struct Plan { int nparts, nchunks, per, pc_log2; };

// host-side shape rules of every entry point; false: unsupported (the error text is set)
template <typename T> bool plan_of(const salt_view& x, Plan* p, const char* who) {
    constexpr int VE = Elem<T>::VE;
    const int C = x.C;
    if (C % 64 || C > 2048) { salt_set_error("%s: C = %d (a multiple of 64 up to 2048 is supported)", who, C); return false; }
    const int64_t hw = (int64_t)x.H * x.W;
    if (hw * x.B >= (1LL << 31)) { salt_set_error("%s: 2^31 pixels or more are not supported", who); return false; }
    int cw = C & -C;
    if (cw > 512) cw = 512;
    p->pc_log2 = ilog2_ceil(cw / VE);
    p->nchunks = C / cw;
    // pixel parts of about 256 pixels, 16 per image at most (the FC launch adds them up)
    int parts = cdiv((int)hw, 256);
    if (parts > 16) parts = 16;
    if (parts < 1) parts = 1;
    p->per = cdiv((int)hw, parts);
    p->nparts = cdiv((int)hw, p->per);
    return true;
}

template <typename T> bool layout_ok(const salt_view& v, const salt_view& like) {
    constexpr int VE = Elem<T>::VE;
    return view_ok(v) && v.B == like.B && v.H == like.H && v.W == like.W && v.C == like.C && (v.cs % VE) == 0 && aligned16(v.p) &&
           (int64_t)v.B * v.H * v.W * v.cs < (1LL << 31);
}

int launch_fc_grads(const salt_se_res_bwd_args* a, hipStream_t st) {
    const int C = a->x.C, n = 2 * C * a->R + C + a->R;
    return salt_launch(se_res_fc_grads_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, a->x.B, C, a->R, (const float*)a->du, (const float*)a->dh, a->gap, a->hidden,
                       a->g_w1, a->g_b1, a->g_w2, a->g_b2);
}

}  // namespace

extern "C" int salt_se_res_parts(const salt_se_res_args* a) {
    if (!a || a->x.B < 1 || a->x.H < 1 || a->x.W < 1 || a->x.C < 1) { salt_set_error("se_res_parts: bad args"); return SALT_E_BADARG; }
    Plan p;
    const bool ok = a->dtype == SALT_BF16 ? plan_of<bf16_t>(a->x, &p, "se_res") : plan_of<float>(a->x, &p, "se_res");
    return ok ? p.nparts : SALT_E_UNSUPPORTED;
}

extern "C" int salt_se_res(const salt_se_res_args* a, void* stream) {
    if (!a || !view_ok(a->x) || !view_ok(a->res) || !view_ok(a->y) || !a->w1 || !a->b1 || !a->w2 || !a->b2 || (!a->gap_partials && !a->gap_acc) || !a->gap ||
        !a->hidden || !a->gate || ((a->in_scale == nullptr) != (a->in_shift == nullptr)))
        SALT_FAIL(SALT_E_BADARG, "se_res: bad args");
    hipStream_t st = (hipStream_t)stream;
    const int C = a->x.C, B = a->x.B, R = a->R;
    SALT_DISPATCH_DTYPE(a->dtype, T, {
        Plan p;
        if (!plan_of<T>(a->x, &p, "se_res")) return SALT_E_UNSUPPORTED;
        if (R != C / 16) SALT_FAIL(SALT_E_UNSUPPORTED, "se_res: R = %d, C / 16 = %d is supported", R, C / 16);
        if (!aligned16(a->w2)) SALT_FAIL(SALT_E_UNSUPPORTED, "se_res: w2 must be 16-byte aligned");
        if (!layout_ok<T>(a->x, a->x) || !layout_ok<T>(a->res, a->x) || !layout_ok<T>(a->y, a->x))
            SALT_FAIL(SALT_E_UNSUPPORTED, "se_res: x / res / y must be 16-byte aligned views of one shape, cs a multiple of the 16-byte piece");
        if (a->nparts != p.nparts) SALT_FAIL(SALT_E_BADARG, "se_res: nparts %d, expected %d", a->nparts, p.nparts);
        const salt_bn_finalize_args* f = static_cast<const salt_bn_finalize_args*>(a->in_fin);
        if (f && (!a->in_fin_acc || f->C != C || !f->gamma || !f->beta || !f->mean || !f->invstd || !f->scale || !f->shift))
            SALT_FAIL(SALT_E_BADARG, "se_res: in_fin needs in_fin_acc and the complete salt_bn_finalize arguments of a %d-channel layer", C);
        const dim3 grid(B * p.nparts * p.nchunks);
        const float inv_hw = 1.0f / (float)(a->x.H * a->x.W);
        int rc = salt_launch(se_res_pool_kernel<T>, grid, dim3(256), 0, st, a->x, p.nparts, p.nchunks, p.per, p.pc_log2, a->gap_acc, a->gap_partials);
        if (rc) return rc;
        const float* sc = a->in_scale; const float* sh = a->in_shift;
        if (f) {
            const BnFin fin{const_cast<double*>(a->in_fin_acc), nullptr, f->gamma, f->beta, f->running_mean, f->running_var, f->num_batches_tracked,
                            f->momentum, f->eps, f->mean, f->invstd, f->scale, f->shift};
            rc = salt_launch(se_res_fc_kernel<true>, dim3(B), dim3(256), (size_t)(3 * C + R) * sizeof(float), st, (const double*)a->gap_acc, (const float*)a->gap_partials,
                             p.nparts, C, R, inv_hw, (const float*)nullptr, (const float*)nullptr, fin, a->w1, a->b1, a->w2, a->b2, a->gap, a->hidden, a->gate);
            sc = f->scale; sh = f->shift;
        } else {
            rc = salt_launch(se_res_fc_kernel<false>, dim3(B), dim3(256), (size_t)(C + R) * sizeof(float), st, (const double*)a->gap_acc, (const float*)a->gap_partials,
                             p.nparts, C, R, inv_hw, sc, sh, BnFin{}, a->w1, a->b1, a->w2, a->b2, a->gap, a->hidden, a->gate);
        }
        if (rc) return rc;
        return salt_launch(se_res_apply_kernel<T>, grid, dim3(256), 0, st, a->x, a->res, a->y, sc, sh, (const float*)a->gate, p.nparts, p.nchunks, p.per, p.pc_log2);
    })
    return SALT_OK;
}

static int se_res_bwd_check(const salt_se_res_bwd_args* a, const char* who) {
    if (!a || !view_ok(a->x) || !a->w1 || !a->w2 || !a->gap || !a->hidden || !a->gate || !a->du || !a->dh || !a->dgap || !a->g_w1 || !a->g_b1 || !a->g_w2 ||
        !a->g_b2 || ((a->in_scale == nullptr) != (a->in_shift == nullptr)))
        SALT_FAIL(SALT_E_BADARG, "%s: bad args", who);
    if (a->x.C % 64 || a->x.C > 2048 || a->R != a->x.C / 16) SALT_FAIL(SALT_E_UNSUPPORTED, "%s: C = %d, R = %d (C a multiple of 64 up to 2048, R = C / 16)", who, a->x.C, a->R);
    return SALT_OK;
}

extern "C" int salt_se_res_fc_grads(const salt_se_res_bwd_args* a, void* stream) {
    const int rc = se_res_bwd_check(a, "se_res_fc_grads");
    if (rc) return rc;
    return launch_fc_grads(a, (hipStream_t)stream);
}

extern "C" int salt_se_res_bwd(const salt_se_res_bwd_args* a, void* stream) {
    int rc = se_res_bwd_check(a, "se_res_bwd");
    if (rc) return rc;
    if (!view_ok(a->y) || !view_ok(a->dy) || !view_ok(a->dx) || !view_ok(a->dres) || (!a->partials && !a->acc)) SALT_FAIL(SALT_E_BADARG, "se_res_bwd: bad args");
    hipStream_t st = (hipStream_t)stream;
    const int C = a->x.C, B = a->x.B, R = a->R;
    SALT_DISPATCH_DTYPE(a->dtype, T, {
        Plan p;
        if (!plan_of<T>(a->x, &p, "se_res_bwd")) return SALT_E_UNSUPPORTED;
        if (!layout_ok<T>(a->x, a->x) || !layout_ok<T>(a->y, a->x) || !layout_ok<T>(a->dy, a->x) || !layout_ok<T>(a->dx, a->x) || !layout_ok<T>(a->dres, a->x))
            SALT_FAIL(SALT_E_UNSUPPORTED, "se_res_bwd: x / y / dy / dx / dres must be 16-byte aligned views of one shape, cs a multiple of the 16-byte piece");
        if (a->nparts != p.nparts) SALT_FAIL(SALT_E_BADARG, "se_res_bwd: nparts %d, expected %d", a->nparts, p.nparts);
        const dim3 grid(B * p.nparts * p.nchunks);
        rc = salt_launch(se_res_bwd_reduce_kernel<T>, grid, dim3(256), 0, st, a->x, a->y, a->dy, a->in_scale, a->in_shift, p.nparts, p.nchunks, p.per, p.pc_log2,
                         a->acc, a->partials);
        if (rc) return rc;
        rc = salt_launch(se_res_fc_bwd_kernel, dim3(B), dim3(256), (size_t)(C + R + 256) * sizeof(float), st, (const double*)a->acc, (const float*)a->partials, p.nparts, C, R,
                         1.0f / (float)(a->x.H * a->x.W), a->w1, a->w2, a->hidden, a->gate, a->du, a->dh, a->dgap);
        if (rc) return rc;
        rc = salt_launch(se_res_bwd_apply_kernel<T>, grid, dim3(256), 0, st, a->y, a->dy, a->gate, (const float*)a->dgap, a->dx, a->dres, a->accumulate_dres, p.nparts,
                         p.nchunks, p.per, p.pc_log2);
        if (rc) return rc;
    })
    return a->defer_param_grads ? SALT_OK : launch_fc_grads(a, st);
}
