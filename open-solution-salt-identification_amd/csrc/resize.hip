// resize.hip — the reference's loader modes 'stacking' and 'resize' on the device (saltnet.h has the pinned formulas).
//
//   salt_stack_resize       ResizeArray + to_tensor_stacking (loaders.py:786-795, 772-775): [B,h,w,M] first-level maps -> NCHW [B,M,H,W],
//                           skimage's order-1 'constant' resize in float64, one rounding.  A TRANSPOSING resampler: the input runs along
//                           M, the output along W, so a workgroup stages the source patch of its output tile in LDS.
//   salt_mask_resize        the PIL-resized two-class stacking target (loaders.py:355-360, 572-575), two 8-bit passes
//   salt_resize_prob / _threshold / _iou_sweep
//                           postprocessing.resize_image (128 -> 101) and what follows it: the map, one class's mask, the metric counts
#include "common.h"
#include "resample64.h"    // src_coord, floor_int, lerp2, frac_of, bilinear64: shared with ensemble.hip

namespace {

// ---- salt_stack_resize ------------------------------------------------------------------------------------------------------------
// One workgroup: image b, MC consecutive maps, an output tile of th x tw pixels.  Its source patch - rows floor(r(Y0)) .. floor(r(Y1)) + 1,
// columns likewise, zero where the source ends - goes to LDS as [patch row][patch column][MC + 1] (the odd pixel stride keeps lanes
// that walk along x off each other's banks); then every thread owns output pixels and walks the MC maps, so a wavefront stores a run
// along W per map.  The [B,h,w,M] layout is read along M (MC floats = 64 bytes per pixel, neighbouring pixels of a patch row follow
// at sc), the plane layout along the patch row.
constexpr int SR_NT = 256;
constexpr int SR_MC = 16;
constexpr int SR_LDS_FLOATS = 12 * 1024;            // 48 KB

struct StackKP {
    salt_stack_resize_args a;
    int th, tw, pr, pc;                               // output tile; patch rows / columns the LDS array is laid out for
    double sr, sc;                                    // h / H, w / W
};

__global__ __launch_bounds__(SR_NT) void stack_resize_kernel(StackKP k) {
    extern __shared__ float s_patch[];
    const salt_stack_resize_args& a = k.a;
    const int tid = threadIdx.x;
    const int tiles_x = (a.W + k.tw - 1) / k.tw;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int m0 = blockIdx.y * SR_MC, b = blockIdx.z;
    const int mc = min(SR_MC, a.M - m0);
    const int Y0 = ty * k.th, X0 = tx * k.tw;
    const int Y1 = min(Y0 + k.th, a.H) - 1, X1 = min(X0 + k.tw, a.W) - 1;          // last output row / column of the tile
    const int rlo = floor_int(src_coord(k.sr, Y0)), clo = floor_int(src_coord(k.sc, X0));
    const int pr = min(floor_int(src_coord(k.sr, Y1)) + 2 - rlo, k.pr), pc = min(floor_int(src_coord(k.sc, X1)) + 2 - clo, k.pc);
    constexpr int PS = SR_MC + 1;
    const float* xb = a.x + (int64_t)b * a.sb + (int64_t)m0 * a.sm;
    const int npix = pr * pc;
    if (a.sm == 1) {                                                                // maps innermost
        for (int i = tid; i < npix * SR_MC; i += SR_NT) {
            const int m = i % SR_MC, q = i / SR_MC;
            const int y = rlo + q / pc, x = clo + q % pc;
            const bool in = m < mc && y >= 0 && y < a.h && x >= 0 && x < a.w;
            s_patch[q * PS + m] = in ? xb[(int64_t)y * a.sr + (int64_t)x * a.sc + m] : 0.f;
        }
    } else {                                                                        // planes: columns innermost
        for (int i = tid; i < npix * SR_MC; i += SR_NT) {
            const int q = i % npix, m = i / npix;
            const int y = rlo + q / pc, x = clo + q % pc;
            const bool in = m < mc && y >= 0 && y < a.h && x >= 0 && x < a.w;
            s_patch[q * PS + m] = in ? xb[(int64_t)m * a.sm + (int64_t)y * a.sr + (int64_t)x * a.sc] : 0.f;
        }
    }
    __syncthreads();
    const int64_t HW = (int64_t)a.H * a.W;
    float* yb = a.y + ((int64_t)b * a.M + m0) * HW;
    for (int i = tid; i < k.th * k.tw; i += SR_NT) {
        const int Y = Y0 + i / k.tw, X = X0 + i % k.tw;
        if (Y > Y1 || X > X1) continue;
        const double r = src_coord(k.sr, Y), c = src_coord(k.sc, X);
        const int r0 = floor_int(r), c0 = floor_int(c);
        const double dr = frac_of(r, r0), dc = frac_of(c, c0);
        const int py = min(max(r0 - rlo, 0), pr - 2), px = min(max(c0 - clo, 0), pc - 2);   // inside the patch by construction
        const float* q = s_patch + (py * pc + px) * PS;
        float* yo = yb + (int64_t)Y * a.W + X;
        for (int m = 0; m < mc; ++m)
            yo[m * HW] = (float)lerp2((double)q[m], (double)q[PS + m], (double)q[pc * PS + m], (double)q[(pc + 1) * PS + m], dr, dc);
    }
}

// patch extent (rows or columns) of the largest tile of `t` outputs along an axis of n outputs
int patch_extent(double scale, int n, int t) {
    int worst = 2;
    for (int o = 0; o < n; o += t) {
        const int last = (o + t < n ? o + t : n) - 1;
        const int e = floor_int(src_coord(scale, last)) + 2 - floor_int(src_coord(scale, o));
        worst = e > worst ? e : worst;
    }
    return worst;
}

// ---- salt_mask_resize ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mask_resize_kernel(salt_mask_resize_args a) {
#pragma clang fp contract(off)
    const int64_t n = (int64_t)a.B * a.H * a.W, HW = (int64_t)a.H * a.W;
    for (int64_t i = blockIdx.x * 256LL + threadIdx.x; i < n; i += gridDim.x * 256LL) {
        const int X = (int)(i % a.W); const int64_t q = i / a.W; const int Y = (int)(q % a.H); const int b = (int)(q / a.H);
        const int rs = min(max(a.row_start[Y], 0), a.h - 1), cs = min(max(a.col_start[X], 0), a.w - 1);          // a table never leaves the mask
        const int rl = min(a.row_len[Y], min(a.row_taps, a.h - rs)), cl = min(a.col_len[X], min(a.col_taps, a.w - cs));
        const double* wr = a.row_w + (int64_t)Y * a.row_taps;
        const double* wc = a.col_w + (int64_t)X * a.col_taps;
        const unsigned char* mk = a.mask + (int64_t)b * a.h * a.w;
        double v0 = 0.0, v1 = 0.0;
        for (int t = 0; t < rl; ++t) {
            const unsigned char* row = mk + (int64_t)(rs + t) * a.w + cs;
            double h0 = 0.0, h1 = 0.0;
            for (int u = 0; u < cl; ++u) {
                const unsigned char v = row[u];
                h0 += v == 0 ? wc[u] : 0.0;
                h1 += v == 1 ? wc[u] : 0.0;
            }
            v0 += wr[t] * floor(h0 + 0.5);                  // the horizontal pass lands on the uint8 grid
            v1 += wr[t] * floor(h1 + 0.5);
        }
        float* to = a.target + (int64_t)b * 2 * HW + (int64_t)Y * a.W + X;
        to[0] = (float)floor(v0 + 0.5);
        to[HW] = (float)floor(v1 + 0.5);
    }
}

// ---- salt_resize_prob / threshold / iou sweep -----------------------------------------------------------------------------------------
struct DownKP { const float* prob; int B, C, H, W, h, w; double sr, sc; };

__global__ __launch_bounds__(256) void resize_prob_kernel(DownKP k, float* out) {
    const int64_t n = (int64_t)k.B * k.C * k.h * k.w;
    for (int64_t i = blockIdx.x * 256LL + threadIdx.x; i < n; i += gridDim.x * 256LL) {
        const int x = (int)(i % k.w); const int64_t q = i / k.w; const int y = (int)(q % k.h); const int64_t plane = q / k.h;
        out[i] = (float)bilinear64(k.prob + plane * k.H * k.W, k.H, k.W, src_coord(k.sr, y), src_coord(k.sc, x));
    }
}

__global__ __launch_bounds__(256) void resize_threshold_kernel(DownKP k, int cls, double threshold, unsigned char* mask) {
    const int64_t n = (int64_t)k.B * k.h * k.w;
    for (int64_t i = blockIdx.x * 256LL + threadIdx.x; i < n; i += gridDim.x * 256LL) {
        const int x = (int)(i % k.w); const int64_t q = i / k.w; const int y = (int)(q % k.h); const int64_t b = q / k.h;
        const double v = bilinear64(k.prob + (b * k.C + cls) * k.H * k.W, k.H, k.W, src_coord(k.sr, y), src_coord(k.sc, x));
        mask[i] = v > threshold ? 1 : 0;
    }
}

struct SweepKP { DownKP d; int cls, T; const unsigned char* gt; int* inter; int* pred; int* gt_count; double th[SALT_MAX_THRESHOLDS]; };

// Threshold-sweep counts of one image by one 256-thread workgroup, the protocol of salt_iou_sweep (loss.hip): every thread counts its
// pixels in registers, add() once per pixel; store() reduces over the workgroup and writes inter[b][T], pred[b][T] and gt_count[b].
// th[t] for t >= T must be a value no probability exceeds.
struct IouSweepCounts {
    int ci[SALT_MAX_THRESHOLDS], cp[SALT_MAX_THRESHOLDS], cg;
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int t = 0; t < SALT_MAX_THRESHOLDS; ++t) { ci[t] = 0; cp[t] = 0; }
        cg = 0;
    }
    __device__ __forceinline__ void add(double p, int g, const double (&th)[SALT_MAX_THRESHOLDS], int T) {
        cg += g;
#pragma unroll
        for (int t = 0; t < SALT_MAX_THRESHOLDS; ++t) {
            const int pr = (t < T && p > th[t]) ? 1 : 0;
            cp[t] += pr; ci[t] += pr & g;
        }
    }
    __device__ __forceinline__ void store(int T, int b, int* inter, int* pred, int* gt_count) {
        __shared__ int s_inter[SALT_MAX_THRESHOLDS], s_pred[SALT_MAX_THRESHOLDS], s_gt;
        const int tid = threadIdx.x;
        if (tid < SALT_MAX_THRESHOLDS) { s_inter[tid] = 0; s_pred[tid] = 0; }
        if (tid == 0) s_gt = 0;
        __syncthreads();
#pragma unroll
        for (int t = 0; t < SALT_MAX_THRESHOLDS; ++t) {
            if (t < T) {                                   // uniform
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
        if (tid < T) { inter[b * T + tid] = s_inter[tid]; pred[b * T + tid] = s_pred[tid]; }
        if (tid == 0) gt_count[b] = s_gt;
    }
};

// one workgroup per image
__global__ __launch_bounds__(256) void resize_iou_sweep_kernel(SweepKP k) {
    const DownKP& d = k.d;
    const int b = blockIdx.x;
    IouSweepCounts c;
    c.clear();
    const int n = d.h * d.w;
    const float* pl = d.prob + ((int64_t)b * d.C + k.cls) * d.H * d.W;
    for (int i = threadIdx.x; i < n; i += 256) {
        const int y = i / d.w, x = i - y * d.w;
        const double p = bilinear64(pl, d.H, d.W, src_coord(d.sr, y), src_coord(d.sc, x));
        c.add(p, k.gt[(int64_t)b * n + i] ? 1 : 0, k.th, k.T);
    }
    c.store(k.T, b, k.inter, k.pred, k.gt_count);
}

bool side_ok(int v) { return v >= 1 && v <= SALT_RESIZE_MAX_SIDE; }

int down_args(const char* op, const float* prob, int B, int C, int H, int W, int h, int w, DownKP& k) {
    if (!prob || B < 1 || C < 1 || !side_ok(H) || !side_ok(W) || !side_ok(h) || !side_ok(w))
        SALT_FAIL(SALT_E_BADARG, "%s: bad args (sides 1 .. %d)", op, SALT_RESIZE_MAX_SIDE);
    if (h > H || w > W)
        SALT_FAIL(SALT_E_BADARG, "%s: %dx%d -> %dx%d is an up-scale; resize_image is pinned for h <= H and w <= W only", op, H, W, h, w);
    k.prob = prob; k.B = B; k.C = C; k.H = H; k.W = W; k.h = h; k.w = w;
    k.sr = (double)H / (double)h; k.sc = (double)W / (double)w;
    return SALT_OK;
}

int grid_for(int64_t n) { return (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096); }

}  // namespace

extern "C" int salt_stack_resize(const salt_stack_resize_args* a, void* stream) {
    if (!a || !a->x || !a->y || a->B < 1 || a->B > 65535 || !side_ok(a->h) || !side_ok(a->w) || !side_ok(a->H) || !side_ok(a->W))
        SALT_FAIL(SALT_E_BADARG, "stack_resize: bad args (sides 1 .. %d, B <= 65535)", SALT_RESIZE_MAX_SIDE);
    if (a->M < 1 || a->M > SALT_STACK_RESIZE_MAX_MAPS) SALT_FAIL(SALT_E_BADARG, "stack_resize: 1 <= M <= %d maps (got %d)", SALT_STACK_RESIZE_MAX_MAPS, a->M);
    if (a->sb < 1 || a->sr < 1 || a->sc < 1 || a->sm < 1 || (a->sm != 1 && a->sc != 1))
        SALT_FAIL(SALT_E_BADARG, "stack_resize: strides must be positive with the maps ([B,h,w,M]) or the columns ([B,M,h,w]) innermost");
    StackKP k;
    k.a = *a;
    k.sr = (double)a->h / (double)a->H; k.sc = (double)a->w / (double)a->W;
    // 8 x 64 outputs per map: a wavefront stores 256-byte runs and the patch of the 101 -> 128 case (9 x 53 pixels x 17 floats) is 32 KB;
    // strong down-scales shrink the tile until its patch fits
    k.th = 8; k.tw = 64;
    for (;;) {
        k.pr = patch_extent(k.sr, a->H, k.th); k.pc = patch_extent(k.sc, a->W, k.tw);
        if ((int64_t)k.pr * k.pc * (SR_MC + 1) <= SR_LDS_FLOATS) break;
        if (k.tw > 1 && k.tw >= k.th) k.tw /= 2; else if (k.th > 1) k.th /= 2;
        else SALT_FAIL(SALT_E_UNSUPPORTED, "stack_resize: no tile fits");          // a 1 x 1 tile has a 2 x 2 patch: not reached
    }
    const int tiles = cdiv(a->H, k.th) * cdiv(a->W, k.tw);
    const size_t lds = (size_t)k.pr * k.pc * (SR_MC + 1) * sizeof(float);
    return salt_launch(stack_resize_kernel, dim3(tiles, cdiv(a->M, SR_MC), a->B), dim3(SR_NT), lds, (hipStream_t)stream, k);
}

extern "C" int salt_mask_resize(const salt_mask_resize_args* a, void* stream) {
    if (!a || !a->mask || !a->target || a->B < 1 || !side_ok(a->h) || !side_ok(a->w) || !side_ok(a->H) || !side_ok(a->W))
        SALT_FAIL(SALT_E_BADARG, "mask_resize: bad args (sides 1 .. %d)", SALT_RESIZE_MAX_SIDE);
    if (!a->row_start || !a->row_len || !a->row_w || !a->col_start || !a->col_len || !a->col_w || a->row_taps < 1 || a->col_taps < 1 ||
        a->row_taps > a->h + 1 || a->col_taps > a->w + 1)
        SALT_FAIL(SALT_E_BADARG, "mask_resize: the per-axis weight tables are required (start, length, weights [n][taps])");
    return salt_launch(mask_resize_kernel, dim3(grid_for((int64_t)a->B * a->H * a->W)), dim3(256), 0, (hipStream_t)stream, *a);
}

extern "C" int salt_resize_prob(const salt_resize_prob_args* a, void* stream) {
    if (!a || !a->out) SALT_FAIL(SALT_E_BADARG, "resize_prob: bad args");
    DownKP k;
    SALT_TRY(down_args("resize_prob", a->prob, a->B, a->C, a->H, a->W, a->h, a->w, k));
    return salt_launch(resize_prob_kernel, dim3(grid_for((int64_t)a->B * a->C * a->h * a->w)), dim3(256), 0, (hipStream_t)stream, k, a->out);
}

extern "C" int salt_resize_threshold(const salt_resize_threshold_args* a, void* stream) {
    if (!a || !a->mask || a->cls < 0 || a->cls >= a->C) SALT_FAIL(SALT_E_BADARG, "resize_threshold: bad args");
    DownKP k;
    SALT_TRY(down_args("resize_threshold", a->prob, a->B, a->C, a->H, a->W, a->h, a->w, k));
    return salt_launch(resize_threshold_kernel, dim3(grid_for((int64_t)a->B * a->h * a->w)), dim3(256), 0, (hipStream_t)stream, k, a->cls,
                       a->threshold, a->mask);
}

extern "C" int salt_resize_iou_sweep(const salt_resize_iou_sweep_args* a, void* stream) {
    if (!a || !a->gt || !a->thresholds || !a->inter || !a->pred || !a->gt_count || a->T < 1 || a->T > SALT_MAX_THRESHOLDS || a->cls < 0 ||
        a->cls >= a->C) SALT_FAIL(SALT_E_BADARG, "resize_iou_sweep: bad args");
    SweepKP k;
    SALT_TRY(down_args("resize_iou_sweep", a->prob, a->B, a->C, a->H, a->W, a->h, a->w, k.d));
    k.cls = a->cls; k.T = a->T; k.gt = a->gt; k.inter = a->inter; k.pred = a->pred; k.gt_count = a->gt_count;
    for (int t = 0; t < SALT_MAX_THRESHOLDS; ++t) k.th[t] = t < a->T ? a->thresholds[t] : 2.0;
    return salt_launch(resize_iou_sweep_kernel, dim3(a->B), dim3(256), 0, (hipStream_t)stream, k);
}
