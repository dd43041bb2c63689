// ensemble.hip — what the reference does BETWEEN models, on the device (saltnet.h has the pinned formulas).
//
//   salt_ensemble      one pass over K member maps: the fold mean (main.py:892-912, np.mean over float32 maps; the float64 accumulator of
//                      notebooks/prediction_average.ipynb), its binarized class map, and the first-level stack of every member's own class
//                      map (utils.py:560-581), on the crop window or through the float64 interpolant of resize.hip
//   salt_rle_encode    utils.run_length_encoding (utils.py:99-111) of a batch of masks, the runs packed across the batch
#include "common.h"
#include "resample64.h"
#include <type_traits>

namespace {

// ---- salt_ensemble ------------------------------------------------------------------------------------------------------------------
// A thread owns an output pixel (b, y, x) and walks the channels and, inside, the members in ascending k: consecutive threads read
// consecutive columns of every member, and the sm = 1 stack store is K consecutive floats per thread.
struct EnsKP {
    const float* m[SALT_MAX_MEMBERS];
    int K, B, C, H, W, top, left, h, w, cls, m0;
    double threshold, sr, sc;                         // sr = H / h, sc = W / w (mode 1)
    float* mean; uint8_t* mask; float* stack;
    int64_t sb, srow, scol, sm;
};

template <int MODE, int ACC>
__global__ __launch_bounds__(256) void ensemble_kernel(EnsKP k) {
#pragma clang fp contract(off)
    typedef typename std::conditional<ACC == 1, double, float>::type acc_t;
    const int64_t n = (int64_t)k.B * k.h * k.w, HW = (int64_t)k.H * k.W, hw = (int64_t)k.h * k.w;
    const int c_lo = k.mean ? 0 : k.cls, c_hi = k.mean ? k.C : k.cls + 1;
    for (int64_t i = blockIdx.x * 256LL + threadIdx.x; i < n; i += gridDim.x * 256LL) {
        const int x = (int)(i % k.w); const int64_t q = i / k.w; const int y = (int)(q % k.h); const int64_t b = q / k.h;
        double r = 0.0, c = 0.0;
        if (MODE == 1) { r = src_coord(k.sr, y); c = src_coord(k.sc, x); }
        float* so = k.stack ? k.stack + b * k.sb + (int64_t)y * k.srow + (int64_t)x * k.scol + (int64_t)k.m0 * k.sm : nullptr;
        for (int ch = c_lo; ch < c_hi; ++ch) {
            const int64_t plane = (b * k.C + ch) * HW;
            const bool is_cls = ch == k.cls;
            acc_t s = 0;
            for (int j = 0; j < k.K; ++j) {
                acc_t v;
                if (MODE == 1) v = (acc_t)bilinear64(k.m[j] + plane, k.H, k.W, r, c);
                else v = (acc_t)k.m[j][plane + (int64_t)(k.top + y) * k.W + (k.left + x)];
                if (so && is_cls) so[(int64_t)j * k.sm] = (float)v;
                if (ACC == 1) s = j ? (acc_t)__dadd_rn((double)s, (double)v) : v;
                else s = j ? (acc_t)__fadd_rn((float)s, (float)v) : v;
            }
            if (ACC == 1) {
                const double v = __ddiv_rn((double)s, (double)k.K);
                if (k.mean) k.mean[(b * k.C + ch) * hw + (int64_t)y * k.w + x] = (float)v;
                if (k.mask && is_cls) k.mask[i] = v > k.threshold ? 1 : 0;
            } else {
                const float v = __fdiv_rn((float)s, (float)k.K);
                if (k.mean) k.mean[(b * k.C + ch) * hw + (int64_t)y * k.w + x] = v;
                if (k.mask && is_cls) k.mask[i] = v > (float)k.threshold ? 1 : 0;
            }
        }
    }
}

// ---- salt_rle_encode ----------------------------------------------------------------------------------------------------------------
// One 256-thread workgroup per image.  The mask goes row-major into LDS (coalesced), is read back in column-major order p = x h + y, and
// thread t owns the positions [t n, (t + 1) n), n = ceil(h w / 256).  A run is emitted by the thread that owns its END; the run's start
// is the latest start at or before it: the thread's own, or - for a run that is open where the range begins - the largest start
// position of the threads before it (an exclusive max-scan).  The rank of a thread's first end is the exclusive sum-scan of the end
// counts.  Both scans: wave64 shuffles, then LDS across the four waves.  No atomics: every pair has one writer and one place.
constexpr int RLE_NT = 256;
constexpr int RLE_SCRATCH = 128;                      // bytes of scan scratch behind the staged mask

__device__ __forceinline__ void wave_scan(int& sum, int& mx) {          // inclusive, over the 64 lanes
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int ts = __shfl_up(sum, o), tm = __shfl_up(mx, o);
        if (lane >= o) { sum += ts; mx = max(mx, tm); }
    }
}

template <bool PLACE>
__global__ __launch_bounds__(RLE_NT) void rle_kernel(salt_rle_encode_args a, int lds_mask_bytes) {
    extern __shared__ unsigned char s_m[];
    int* s_sum = reinterpret_cast<int*>(s_m + lds_mask_bytes);           // [4] end counts of the waves
    int* s_max = s_sum + 4;                                              // [4] latest start of the waves
    long long* s_off = reinterpret_cast<long long*>(s_max + 4);          // [4] partial sums of counts[0 .. b)
    const int tid = threadIdx.x, b = blockIdx.x, h = a.h, w = a.w, hw = h * w;
    const uint8_t* mk = a.mask + (int64_t)b * hw;
    for (int i = tid; i < hw; i += RLE_NT) s_m[i] = mk[i] ? 1 : 0;
    long long off = 0;
    if (PLACE) {
        for (int j = tid; j < b; j += RLE_NT) off += a.counts[j];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) off += __shfl_xor(off, o);
        if ((tid & 63) == 0) s_off[tid >> 6] = off;
    }
    __syncthreads();
    if (PLACE) off = s_off[0] + s_off[1] + s_off[2] + s_off[3];
    const int per = (hw + RLE_NT - 1) / RLE_NT;
    const int lo = min(tid * per, hw), hi = min(lo + per, hw);
    auto at = [&](int p) -> int { const int x = p / h; return s_m[(p - x * h) * w + x]; };
    const int before = lo > 0 && lo < hw ? at(lo - 1) : 0;
    // pass 1: this range's run ends and its latest run start
    int ends = 0, last_start = -1;
    if (lo < hi) {
        int x = lo / h, y = lo - x * h, idx = y * w + x, prev = before, cur = s_m[idx];
        for (int p = lo; p < hi; ++p) {
            if (++y == h) { y = 0; ++x; idx = x; } else idx += w;
            const int next = p + 1 < hw ? s_m[idx] : 0;
            ends += cur & (next ^ 1);
            if (cur & (prev ^ 1)) last_start = p;
            prev = cur; cur = next;
        }
    }
    int sum = ends, mx = last_start;
    wave_scan(sum, mx);
    if ((tid & 63) == 63) { s_sum[tid >> 6] = sum; s_max[tid >> 6] = mx; }
    __syncthreads();
    int rank = sum - ends, carry = __shfl_up(mx, 1);                      // exclusive within the wave
    if ((tid & 63) == 0) carry = -1;
    for (int v = 0; v < (tid >> 6); ++v) { rank += s_sum[v]; carry = max(carry, s_max[v]); }
    const int count = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
    if (!PLACE) {
        if (tid == 0) a.counts[b] = count;
        return;
    }
    if (tid == 0 && b == (int)gridDim.x - 1) a.total[0] = off + count;
    // pass 2: emit (start + 1, length) for every run that ends in this range
    if (lo < hi) {
        int x = lo / h, y = lo - x * h, idx = y * w + x, prev = before, cur = s_m[idx], start = carry;
        int64_t pair = off + rank;
        for (int p = lo; p < hi; ++p) {
            if (++y == h) { y = 0; ++x; idx = x; } else idx += w;
            const int next = p + 1 < hw ? s_m[idx] : 0;
            if (cur & (prev ^ 1)) start = p;
            if (cur & (next ^ 1)) {
                if (pair < a.cap_pairs) { a.runs[2 * pair] = start + 1; a.runs[2 * pair + 1] = p - start + 1; }
                ++pair;
            }
            prev = cur; cur = next;
        }
    }
}

int grid_for(int64_t n) { return (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096); }

}  // namespace

extern "C" int salt_ensemble(const salt_ensemble_args* a, void* stream) {
    if (!a || !a->members || a->K < 1 || a->K > SALT_MAX_MEMBERS)
        SALT_FAIL(SALT_E_BADARG, "ensemble: bad args (members is a HOST array of 1 <= K <= %d device pointers)", SALT_MAX_MEMBERS);
    if (a->B < 1 || a->C < 1 || a->H < 1 || a->W < 1 || a->h < 1 || a->w < 1) SALT_FAIL(SALT_E_BADARG, "ensemble: bad shape");
    if (a->mode != 0 && a->mode != 1) SALT_FAIL(SALT_E_BADARG, "ensemble: mode %d (0 crop | 1 resize)", a->mode);
    if (a->acc != 0 && a->acc != 1) SALT_FAIL(SALT_E_BADARG, "ensemble: acc %d (0 fp32 | 1 float64)", a->acc);
    if (a->mode == 1 && a->acc == 0)
        SALT_FAIL(SALT_E_UNSUPPORTED, "ensemble: the resized maps of the reference are float64: mode 1 needs acc 1");
    if (a->mode == 0 && (a->top < 0 || a->left < 0 || (int64_t)a->top + a->h > a->H || (int64_t)a->left + a->w > a->W))
        SALT_FAIL(SALT_E_BADARG, "ensemble: window [%d,+%d) x [%d,+%d) outside the %dx%d map", a->top, a->h, a->left, a->w, a->H, a->W);
    if (a->mode == 1 && (a->h > a->H || a->w > a->W))
        SALT_FAIL(SALT_E_BADARG, "ensemble: %dx%d -> %dx%d is an up-scale; resize_image is pinned for h <= H and w <= W only", a->H, a->W, a->h, a->w);
    if (a->cls < 0 || a->cls >= a->C) SALT_FAIL(SALT_E_BADARG, "ensemble: cls %d of %d channels", a->cls, a->C);
    if (!a->mean && !a->mask && !a->stack) SALT_FAIL(SALT_E_BADARG, "ensemble: no output requested (mean, mask, stack)");
    if (a->stack && (a->sb < 1 || a->sr < 1 || a->sc < 1 || a->sm < 1 || a->m0 < 0))
        SALT_FAIL(SALT_E_BADARG, "ensemble: the stack needs positive element strides and m0 >= 0");
    EnsKP k;
    for (int j = 0; j < SALT_MAX_MEMBERS; ++j) {
        k.m[j] = j < a->K ? a->members[j] : nullptr;
        if (j < a->K && !k.m[j]) SALT_FAIL(SALT_E_BADARG, "ensemble: member %d is NULL", j);
    }
    k.K = a->K; k.B = a->B; k.C = a->C; k.H = a->H; k.W = a->W; k.top = a->top; k.left = a->left; k.h = a->h; k.w = a->w;
    k.cls = a->cls; k.m0 = a->m0; k.threshold = a->threshold;
    k.sr = (double)a->H / (double)a->h; k.sc = (double)a->W / (double)a->w;
    k.mean = a->mean; k.mask = a->mask; k.stack = a->stack;
    k.sb = a->sb; k.srow = a->sr; k.scol = a->sc; k.sm = a->sm;
    const dim3 grid(grid_for((int64_t)a->B * a->h * a->w));
    if (a->mode == 1) return salt_launch(ensemble_kernel<1, 1>, grid, dim3(256), 0, (hipStream_t)stream, k);
    if (a->acc == 1) return salt_launch(ensemble_kernel<0, 1>, grid, dim3(256), 0, (hipStream_t)stream, k);
    return salt_launch(ensemble_kernel<0, 0>, grid, dim3(256), 0, (hipStream_t)stream, k);
}

extern "C" int salt_rle_encode(const salt_rle_encode_args* a, void* stream) {
    if (!a || !a->mask || !a->counts || !a->runs || !a->total || a->B < 1 || a->h < 1 || a->w < 1 || a->cap_pairs < 0)
        SALT_FAIL(SALT_E_BADARG, "rle_encode: bad args");
    if ((int64_t)a->h * a->w > 65536) SALT_FAIL(SALT_E_BADARG, "rle_encode: h w <= 65536 (the mask is staged in LDS), got %dx%d", a->h, a->w);
    const int mask_bytes = (a->h * a->w + 15) / 16 * 16;
    const size_t lds = (size_t)mask_bytes + RLE_SCRATCH;
    SALT_TRY(salt_launch(rle_kernel<false>, dim3(a->B), dim3(RLE_NT), lds, (hipStream_t)stream, *a, mask_bytes));
    return salt_launch(rle_kernel<true>, dim3(a->B), dim3(RLE_NT), lds, (hipStream_t)stream, *a, mask_bytes);
}
