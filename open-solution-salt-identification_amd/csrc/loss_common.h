// loss_common.h — the stable radix sort behind every Lovasz loss, as kernels templated on an error policy, and the parts-per-plane
// rule of the partial-sum losses.  Included by loss.hip (Lovasz hinge: HingeElu) and loss_softmax.hip (Lovasz-softmax: AbsError).
//
// A policy supplies the three places where the losses differ; everything else - keys, ranking, scatter, label scan, the fp32
// operation sequence of the Jaccard gradient g_k - is one piece of code:
//   error(x, lab)    the sorted quantity of an element with input x and label lab in {0.f, 1.f}
//   value(e)         what enters the dot product with g_k
//   dvalue(e, lab)   d value(error(x, lab)) / d x; the stored gradient is dvalue * g_k * loss_scale / rows
// Rows are `B` contiguous runs of `P` floats of salt_lovasz_args (an image of the hinge, a (b, c) plane of the softmax form).
#pragma once
#include "common.h"

namespace {

struct HingeElu {                        // lovasz_losses.py:81-115 with F.elu: e = 1 - z * sign, elu(e) . g
    static __device__ __forceinline__ float error(float z, float lab) { return 1.f - z * (2.f * lab - 1.f); }
    static __device__ __forceinline__ float value(float e) { return e > 0.f ? e : expm1f(e); }
    static __device__ __forceinline__ float dvalue(float e, unsigned lab) {
        const float d = e > 0.f ? 1.f : __expf(e);
        const float sg = lab ? 1.f : -1.f;
        return -sg * d;
    }
};

struct AbsError {                        // lovasz_losses.py:173-210: e = |fg - p|, e . g; torch's abs backward is 0 at 0
    static __device__ __forceinline__ float error(float p, float lab) { return fabsf(lab - p); }
    static __device__ __forceinline__ float value(float e) { return e; }
    static __device__ __forceinline__ float dvalue(float e, unsigned lab) { return e == 0.f ? 0.f : (lab ? -1.f : 1.f); }
};

// The options of a row are a second policy.  XPlain is the call without options: contiguous rows, no void label,
// every class; its kernels hold no trace of the rest.  XOpt reads LovaszX at run time:
//   void     an element whose target equals `ignore` gets the largest key (no finite error maps to it) and bit 1 of the payload, so it
//            is sorted behind every valid element and the valid ones keep the positions of the compacted list; it counts in neither
//            k, c_k nor G and its gradient is written as 0
//   gather   row c of the batch-flat softmax form: flat index j = b HW + i lives at ((b C + c) HW + i)
//   present  rowpos[row] = positives of the row (lovasz_rowpos_kernel); rows come in groups of C classes, a row without positives is
//            skipped (loss 0, gradient 0) and the others scale by loss_scale / (groups * present classes of the group)
// The payload is (index << 1 | label) for XPlain and (index << 2 | void << 1 | label) for XOpt.
__device__ __forceinline__ unsigned desc_key(float e);
constexpr int XF_VOID = 1, XF_GATHER = 2;
struct LovaszX { float ignore; int flags; int HW; int C; const unsigned* rowpos; };
struct XPlain { static constexpr bool on = false; static constexpr int shift = 1; };
struct XOpt { static constexpr bool on = true; static constexpr int shift = 2; };

// offset of element i of row b in logits / target / dlogits
template <class X>
__device__ __forceinline__ int64_t x_off(const salt_lovasz_args& a, const LovaszX& x, int b, int64_t i) {
    if constexpr (X::on) {
        if (x.flags & XF_GATHER) { const int64_t im = i / x.HW; return (im * x.C + b) * x.HW + (i - im * x.HW); }
    }
    return (int64_t)b * a.P + i;
}

template <class Pol, class X>
__device__ __forceinline__ void x_keyval(float zi, float yi, unsigned i, const LovaszX& x, unsigned& key, unsigned& val, float& lab) {
    if constexpr (X::on) {
        if ((x.flags & XF_VOID) && yi == x.ignore) { key = 0xffffffffu; val = (i << 2) | 2u; lab = 0.f; return; }   // before the > 0.5 test
    }
    lab = yi > 0.5f ? 1.f : 0.f;                                  // target.long() of a {0.,1.} mask
    key = desc_key(Pol::error(zi, lab));
    val = (i << X::shift) | (lab > 0.5f ? 1u : 0u);
}

// gradient scale of row b; *skip: the row is left out (only-present and no positives)
template <class X>
__device__ __forceinline__ float x_gscale(const salt_lovasz_args& a, const LovaszX& x, int b, bool* skip) {
    *skip = false;
    if constexpr (X::on) {
        if (x.rowpos) {
            const int g0 = (b / x.C) * x.C;
            int present = 0;
            for (int c = 0; c < x.C; ++c) present += x.rowpos[g0 + c] > 0u ? 1 : 0;
            *skip = x.rowpos[b] == 0u;
            return *skip ? 0.f : a.loss_scale / (float)((a.B / x.C) * present);
        }
    }
    return a.loss_scale / (float)a.B;
}

constexpr int LT = 1024;                 // threads per image
constexpr int LW = LT / 64;              // waves

__device__ __forceinline__ unsigned desc_key(float e) {          // ascending uint order == descending float order
    unsigned u = __float_as_uint(e);
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ~u;
}
__device__ __forceinline__ float key_to_float(unsigned k) {
    unsigned u = ~k;
    u = (u & 0x80000000u) ? (u & 0x7fffffffu) : ~u;
    return __uint_as_float(u);
}

// One workgroup per image.  Chunk c is the elements c*1024 + tid; every pass ranks and scatters the chunks in ascending order, which
// is what makes the sort stable.  Two things keep the per-chunk critical path LDS-only:
//   * the (key, payload) pairs of the next group of 4 chunks are loaded while the current group is ranked and scattered (the
//     ping-pong workspace is L2-resident), and
//   * the digit histogram of pass p+1 is accumulated while pass p scatters (a histogram does not depend on element order), so
//     there are no separate counting sweeps.
// Final pass over the sorted sequence, with k = rank + 1, c_k = positives up to rank k (inclusive), G = all positives, in fp32:
//   J_k = 1 - (G - c_k) / (G + (k - c_k))    (__fsub_rn / __fdiv_rn: one correctly rounded division, one subtraction from 1)
//   g_k = J_k - J_(k-1)  (g_1 = J_1),  loss += value(e_k) g_k,  d loss / d input = dvalue g_k loss_scale / B
//   (hinge: value = elu, dvalue = -sign d).
constexpr int LG = 4;                    // chunks per prefetch group
template <class Pol, class X>
__global__ __launch_bounds__(LT) void lovasz_pf_kernel(salt_lovasz_args a, LovaszX x) {
    __shared__ unsigned hist[2][256];
    __shared__ unsigned base[256];
    __shared__ unsigned wcount[LW][256];
    __shared__ float red[LW];
    __shared__ unsigned scan_w[LW];
    __shared__ unsigned carry_s;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int P = a.P;
    const float* z = a.logits + (int64_t)b * P;
    const float* y = a.target + (int64_t)b * P;
    unsigned* k0 = a.ws_keys + (int64_t)b * P;
    unsigned* v0 = a.ws_vals + (int64_t)b * P;
    unsigned* k1 = a.ws_keys + ((int64_t)a.B + b) * P;
    unsigned* v1 = a.ws_vals + ((int64_t)a.B + b) * P;
    const int nchunks = (P + LT - 1) / LT, ngroups = (nchunks + LG - 1) / LG;

    // ---- keys + total positives + histogram of the first digit
    if (tid < 256) { hist[0][tid] = 0; hist[1][tid] = 0; }
    __syncthreads();
    float gsum = 0.f;
    for (int i = tid; i < P; i += LT) {
        unsigned key, val; float lab;
        if constexpr (X::on) { const int64_t o = x_off<X>(a, x, b, i); x_keyval<Pol, X>(a.logits[o], a.target[o], (unsigned)i, x, key, val, lab); }
        else x_keyval<Pol, X>(z[i], y[i], (unsigned)i, x, key, val, lab);
        k0[i] = key;
        v0[i] = val;
        atomicAdd(&hist[0][key & 255u], 1u);
        gsum += lab;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) gsum += __shfl_xor(gsum, o);
    if (lane == 0) red[wave] = gsum;
    __syncthreads();
    float G = 0.f;
    for (int w = 0; w < LW; ++w) G += red[w];
    __syncthreads();

    // ---- stable LSD radix sort, 8 bits per pass
    const unsigned long long lt_mask = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    for (int pass = 0; pass < 4; ++pass) {
        const unsigned* ki = (pass & 1) ? k1 : k0; const unsigned* vi = (pass & 1) ? v1 : v0;
        unsigned* ko = (pass & 1) ? k0 : k1; unsigned* vo = (pass & 1) ? v0 : v1;
        const int shift = pass * 8;
        unsigned* hcur = hist[pass & 1];
        unsigned* hnext = hist[(pass + 1) & 1];
        unsigned ck[LG], cv[LG], nk[LG], nv[LG];
#pragma unroll
        for (int u = 0; u < LG; ++u) { const int i = u * LT + tid; ck[u] = i < P ? ki[i] : 0u; cv[u] = i < P ? vi[i] : 0u; }
        if (tid < 64) {                                           // exclusive scan of 256 counters by one wave
            unsigned c[4], s = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) { c[j] = hcur[tid * 4 + j]; s += c[j]; }
            unsigned incl = s;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) { const unsigned t = __shfl_up(incl, o); if (lane >= o) incl += t; }
            unsigned run = incl - s;
#pragma unroll
            for (int j = 0; j < 4; ++j) { base[tid * 4 + j] = run; run += c[j]; }
        }
        __syncthreads();
        if (tid < 256) hcur[tid] = 0;                             // becomes the histogram of pass+2 (written from pass+1 on)
        for (int g = 0; g < ngroups; ++g) {
            const int cn = (g + 1) * LG;
#pragma unroll
            for (int u = 0; u < LG; ++u) { const int i = (cn + u) * LT + tid; nk[u] = i < P ? ki[i] : 0u; nv[u] = i < P ? vi[i] : 0u; }
#pragma unroll
            for (int u = 0; u < LG; ++u) {
                const int c0 = (g * LG + u) * LT;
                if (c0 >= P) break;                               // uniform
                for (int i = tid; i < LW * 256; i += LT) (&wcount[0][0])[i] = 0;
                __syncthreads();
                const bool ok = c0 + tid < P;
                const unsigned key = ck[u];
                const unsigned d = ok ? ((key >> shift) & 255u) : 256u;
                unsigned long long m = __ballot(ok);              // lanes of this wave holding the same digit
#pragma unroll
                for (int bit = 0; bit < 8; ++bit) {
                    const unsigned long long bm = __ballot((d >> bit) & 1u);
                    m &= ((d >> bit) & 1u) ? bm : ~bm;
                }
                const unsigned rank = (unsigned)__popcll(m & lt_mask);
                if (ok && rank == 0) wcount[wave][d] = (unsigned)__popcll(m);
                __syncthreads();
                if (tid < 256) {                                  // digit tid: prefix over waves, advance base
                    unsigned run = base[tid];
                    for (int w = 0; w < LW; ++w) { const unsigned c = wcount[w][tid]; wcount[w][tid] = run; run += c; }
                    base[tid] = run;
                }
                __syncthreads();
                if (ok) {
                    const unsigned dst = wcount[wave][d] + rank;
                    ko[dst] = key; vo[dst] = cv[u];
                    if (pass < 3) atomicAdd(&hnext[(key >> (shift + 8)) & 255u], 1u);
                }
                __syncthreads();
            }
#pragma unroll
            for (int u = 0; u < LG; ++u) { ck[u] = nk[u]; cv[u] = nv[u]; }
        }
        __syncthreads();
    }
    // after 4 passes the sorted sequence is back in (k0, v0)

    // ---- fused scan + Jaccard gradient + dot + scatter
    if (tid == 0) carry_s = 0;
    __syncthreads();
    float lsum = 0.f;
    bool skip;
    const float gscale = x_gscale<X>(a, x, b, &skip);
    float* dz = a.dlogits ? a.dlogits + (int64_t)b * P : nullptr;
    unsigned ck[LG], cv[LG], nk[LG], nv[LG];
#pragma unroll
    for (int u = 0; u < LG; ++u) { const int i = u * LT + tid; ck[u] = i < P ? k0[i] : 0u; cv[u] = i < P ? v0[i] : 0u; }
    for (int g = 0; g < ngroups; ++g) {
        const int cn = (g + 1) * LG;
#pragma unroll
        for (int u = 0; u < LG; ++u) { const int i = (cn + u) * LT + tid; nk[u] = i < P ? k0[i] : 0u; nv[u] = i < P ? v0[i] : 0u; }
#pragma unroll
        for (int u = 0; u < LG; ++u) {
            const int c0 = (g * LG + u) * LT;
            if (c0 >= P) break;
            const int i = c0 + tid;
            const bool ok = i < P;
            const unsigned val = ok ? cv[u] : 0u;
            const unsigned lab = val & 1u;
            unsigned incl = ok ? lab : 0u;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) { const unsigned t = __shfl_up(incl, o); if (lane >= o) incl += t; }
            if (lane == 63) scan_w[wave] = incl;
            __syncthreads();
            unsigned woff = carry_s;
            for (int w = 0; w < wave; ++w) woff += scan_w[w];
            const unsigned c_k = woff + incl;                     // inclusive count of positives up to rank k
            __syncthreads();
            if (tid == LT - 1) carry_s = c_k;
            if (ok) {
                const float e = key_to_float(ck[u]);
                const float kf = (float)(i + 1), ckf = (float)c_k, ckm = (float)(c_k - lab);
                // exactly the reference's fp32 sequence (lovasz_losses.py:27-32): one correctly rounded division, one
                // subtraction from 1, one first difference; no fma contraction (the difference cancels ~3 digits)
                const float jk = __fsub_rn(1.f, __fdiv_rn(G - ckf, G + (kf - ckf)));
                float jm = 0.f;
                if (i > 0) jm = __fsub_rn(1.f, __fdiv_rn(G - ckm, G + ((kf - 1.f) - ckm)));
                const float gk = (i > 0) ? __fsub_rn(jk, jm) : jk;
                const float el = Pol::value(e);
                if constexpr (X::on) {
                    const bool live = !(val & 2u) && !skip;       // a void element or a skipped row: no loss, a gradient of exactly 0
                    if (live) lsum += el * gk;
                    if (a.dlogits && (val >> 2) < (unsigned)P) a.dlogits[x_off<X>(a, x, b, val >> 2)] = live ? Pol::dvalue(e, lab) * gk * gscale : 0.f;
                } else {
                    lsum += el * gk;
                    if (dz) dz[val >> 1] = Pol::dvalue(e, lab) * gk * gscale;
                }
            }
            __syncthreads();
        }
#pragma unroll
        for (int u = 0; u < LG; ++u) { ck[u] = nk[u]; cv[u] = nv[u]; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) lsum += __shfl_xor(lsum, o);
    if (lane == 0) red[wave] = lsum;
    __syncthreads();
    if (tid == 0) {
        float t = 0.f;
        for (int w = 0; w < LW; ++w) t += red[w];
        if (P == 0) t = 0.f;
        a.loss_per_image[b] = t;
    }
}

// ---------------------------------------------------------------- split over several workgroups per image
// The one-workgroup-per-image kernel above is a chain of ~500 barriers on 32 of the 256 CUs (265 us for B = 32).  The split form
// gives every image S segments of SL = 2048 consecutive positions, one 256-thread workgroup each, and runs the SAME stable LSD
// radix sort as 1 + 4 launches - the launch boundary is the only cross-workgroup synchronisation:
//   keys    : keys / payload of the segment, histogram of digit 0 per segment              -> H0[b][seg][256]
//   pass p  : digit base of the segment = (keys of all segments with a smaller digit) + (same digit in earlier segments), from
//             H_p; stable ranking chunk by chunk exactly as above (4 waves instead of 16); scatter; the histogram of digit p+1 is
//             collected per DESTINATION segment in LDS and flushed with integer atomics into H_(p+1) (three rotating buffers: the
//             one read in the previous pass is cleared for the next); the last pass counts the positives per destination segment
//   scan    : label scan with the carry of the earlier segments, Jaccard gradient, dot, scatter; per-segment loss partials that
//             lovasz_mean_split_kernel adds in fixed order.
// Integer atomics only: results do not depend on scheduling.  Positions, ties and the fp32 operation sequence of g_k are those of
// lovasz_pf_kernel, so gradients are bit-identical to it; the loss differs in the last bits (different summation tree).
// Only the keys and the scan kernel see the policy; the passes move (key, payload) pairs.
constexpr int ST = 256, SWV = ST / 64, SL = 2048, SCH = SL / ST, SMAXSEG = 64;
struct LovaszSplit {                                                            // hist [3][B][S][256], pos [B][S], part [B][S]
    int S; unsigned* hist; unsigned* pos; float* part;
    static constexpr bool guard = false;
    __device__ __forceinline__ void first_histogram(int B, int b, int seg, int tid, unsigned count) const {
        const int64_t slot = ((int64_t)b * S + seg) * 256 + tid, hb = (int64_t)B * S * 256;
        hist[slot] = count;
        hist[hb + slot] = 0;                                      // buffer 1 collects digit 1 during pass 0
        if (tid == 0) pos[b * S + seg] = 0;
    }
    // positives of the row in the segments before `seg`, and in the whole row
    __device__ __forceinline__ void positives(int b, int seg, unsigned* carry, unsigned* gtot) const {
        unsigned g = 0, c = 0;
        for (int s2 = 0; s2 < S; ++s2) { const unsigned v = pos[b * S + s2]; g += v; if (s2 < seg) c += v; }
        *carry = c; *gtot = g;
    }
};
// The long-row form (rows above SMAXSEG segments): the histograms live in global memory, digit-major so that one digit's counts over
// the segments are contiguous - hist [rows][256][S], tot [rows][256], pos [rows][S], postot [rows], part [rows][S].
struct LovaszLong {
    int S; unsigned* hist; unsigned* tot; unsigned* pos; unsigned* postot; float* part;
    static constexpr bool guard = true;                           // new code checks a payload's index before it stores through it
    __device__ __forceinline__ void first_histogram(int, int b, int seg, int tid, unsigned count) const {
        hist[((int64_t)b * 256 + tid) * S + seg] = count;
    }
    __device__ __forceinline__ void positives(int b, int seg, unsigned* carry, unsigned* gtot) const {
        *carry = pos[(int64_t)b * S + seg];                       // exclusive prefix (lovasz_segscan_kernel)
        *gtot = postot[b];
    }
};

template <class Pol, class X, class SP>
__global__ __launch_bounds__(ST) void lovasz_keys_kernel(salt_lovasz_args a, SP sp, LovaszX x) {
    __shared__ unsigned h[256];
    const int b = blockIdx.x / sp.S, seg = blockIdx.x % sp.S, tid = threadIdx.x;
    const int P = a.P, i0 = seg * SL, i1 = min(i0 + SL, P);
    const float* z = a.logits + (int64_t)b * P;
    const float* y = a.target + (int64_t)b * P;
    unsigned* k0 = a.ws_keys + (int64_t)b * P;
    unsigned* v0 = a.ws_vals + (int64_t)b * P;
    h[tid] = 0;
    __syncthreads();
    for (int i = i0 + tid; i < i1; i += ST) {
        unsigned key, val; float lab;
        if constexpr (X::on) { const int64_t o = x_off<X>(a, x, b, i); x_keyval<Pol, X>(a.logits[o], a.target[o], (unsigned)i, x, key, val, lab); }
        else x_keyval<Pol, X>(z[i], y[i], (unsigned)i, x, key, val, lab);
        k0[i] = key;
        v0[i] = val;
        atomicAdd(&h[key & 255u], 1u);
    }
    __syncthreads();
    sp.first_histogram(a.B, b, seg, tid, h[tid]);
}

__global__ __launch_bounds__(ST) void lovasz_pass_kernel(salt_lovasz_args a, LovaszSplit sp, int pass) {
    extern __shared__ unsigned nh[];                              // [S][256] next digit per destination segment (+ [S] positives)
    __shared__ unsigned base[256];
    __shared__ unsigned wcount2[2][SWV][256];                     // double buffered: no barrier between a chunk's scatter and the next chunk's reset
    __shared__ unsigned scan_w[SWV];
    const int b = blockIdx.x / sp.S, seg = blockIdx.x % sp.S, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int P = a.P, S = sp.S, i0 = seg * SL;
    const unsigned* ki = a.ws_keys + ((int64_t)((pass & 1) ? a.B : 0) + b) * P;
    const unsigned* vi = a.ws_vals + ((int64_t)((pass & 1) ? a.B : 0) + b) * P;
    unsigned* ko = a.ws_keys + ((int64_t)((pass & 1) ? 0 : a.B) + b) * P;
    unsigned* vo = a.ws_vals + ((int64_t)((pass & 1) ? 0 : a.B) + b) * P;
    const int64_t hb = (int64_t)a.B * S * 256;
    const unsigned* Hc = sp.hist + (pass % 3) * hb + (int64_t)b * S * 256;
    unsigned* Hn = sp.hist + ((pass + 1) % 3) * hb + (int64_t)b * S * 256;
    unsigned* Hz = sp.hist + ((pass + 2) % 3) * hb + (int64_t)b * S * 256;
    const int shift = pass * 8;
    // the segment's keys: all SCH chunks in registers before the first barrier
    unsigned ck[SCH], cv[SCH];
#pragma unroll
    for (int u = 0; u < SCH; ++u) { const int i = i0 + u * ST + tid; ck[u] = i < P ? ki[i] : 0u; cv[u] = i < P ? vi[i] : 0u; }
    // ---- digit bases of this segment
    {
        unsigned tot = 0, before = 0;
        for (int s2 = 0; s2 < S; ++s2) { const unsigned c = Hc[s2 * 256 + tid]; tot += c; if (s2 < seg) before += c; }
        unsigned incl = tot;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const unsigned t = __shfl_up(incl, o); if (lane >= o) incl += t; }
        if (lane == 63) scan_w[wave] = incl;
        for (int e = tid; e < S * 256 + S; e += ST) nh[e] = 0;
        __syncthreads();
        unsigned woff = 0;
        for (int w = 0; w < wave; ++w) woff += scan_w[w];
        base[tid] = woff + incl - tot + before;
        Hz[seg * 256 + tid] = 0;                                  // read in the previous pass, collects digit pass+2 in the next
    }
    const unsigned long long lt_mask = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
#pragma unroll
    for (int u = 0; u < SCH; ++u) {
        const int c0 = i0 + u * ST;
        if (c0 >= P) break;                                       // uniform
        unsigned (*wcount)[256] = wcount2[u & 1];
#pragma unroll
        for (int w = 0; w < SWV; ++w) wcount[w][tid] = 0;
        __syncthreads();                                          // also publishes base[] / nh[] on the first round
        const bool ok = c0 + tid < P;
        const unsigned key = ck[u];
        const unsigned d = ok ? ((key >> shift) & 255u) : 256u;
        unsigned long long m = __ballot(ok);
#pragma unroll
        for (int bit = 0; bit < 8; ++bit) {
            const unsigned long long bm = __ballot((d >> bit) & 1u);
            m &= ((d >> bit) & 1u) ? bm : ~bm;
        }
        const unsigned rank = (unsigned)__popcll(m & lt_mask);
        if (ok && rank == 0) wcount[wave][d] = (unsigned)__popcll(m);
        __syncthreads();
        {
            unsigned run = base[tid];
#pragma unroll
            for (int w = 0; w < SWV; ++w) { const unsigned c = wcount[w][tid]; wcount[w][tid] = run; run += c; }
            base[tid] = run;
        }
        __syncthreads();
        if (ok) {
            const unsigned dst = wcount[wave][d] + rank;
            ko[dst] = key; vo[dst] = cv[u];
            const unsigned ds = dst / SL;
            if (pass < 3) atomicAdd(&nh[ds * 256 + ((key >> (shift + 8)) & 255u)], 1u);
            else if (cv[u] & 1u) atomicAdd(&nh[S * 256 + ds], 1u);
        }
    }
    __syncthreads();
    if (pass < 3) {
        for (int e = tid; e < S * 256; e += ST) { const unsigned c = nh[e]; if (c) atomicAdd(&Hn[e], c); }
    } else if (tid < S) {
        const unsigned c = nh[S * 256 + tid];
        if (c) atomicAdd(&sp.pos[b * S + tid], c);
    }
}

template <class Pol, class X, class SP>
__global__ __launch_bounds__(ST) void lovasz_scan_kernel(salt_lovasz_args a, SP sp, LovaszX x) {
    __shared__ unsigned scan_w[SWV];
    __shared__ float red[SWV];
    const int b = blockIdx.x / sp.S, seg = blockIdx.x % sp.S, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int P = a.P, S = sp.S, i0 = seg * SL;
    const unsigned* k0 = a.ws_keys + (int64_t)b * P;              // after 4 passes the sorted sequence is back in buffer 0
    const unsigned* v0 = a.ws_vals + (int64_t)b * P;
    unsigned ck[SCH], cv[SCH];
#pragma unroll
    for (int u = 0; u < SCH; ++u) { const int i = i0 + u * ST + tid; ck[u] = i < P ? k0[i] : 0u; cv[u] = i < P ? v0[i] : 0u; }
    unsigned gtot = 0, carry = 0;
    sp.positives(b, seg, &carry, &gtot);
    const float G = (float)gtot;
    bool skip;
    const float gscale = x_gscale<X>(a, x, b, &skip);
    float* dz = a.dlogits ? a.dlogits + (int64_t)b * P : nullptr;
    float lsum = 0.f;
#pragma unroll
    for (int u = 0; u < SCH; ++u) {
        const int i = i0 + u * ST + tid;
        if (i0 + u * ST >= P) break;
        const bool ok = i < P;
        const unsigned val = ok ? cv[u] : 0u;
        const unsigned lab = val & 1u;
        unsigned incl = ok ? lab : 0u;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const unsigned t = __shfl_up(incl, o); if (lane >= o) incl += t; }
        __syncthreads();                                          // scan_w of the previous chunk has been read
        if (lane == 63) scan_w[wave] = incl;
        __syncthreads();
        unsigned woff = carry, ctot = 0;
        for (int w = 0; w < SWV; ++w) { if (w < wave) woff += scan_w[w]; ctot += scan_w[w]; }
        const unsigned c_k = woff + incl;
        carry += ctot;
        if (ok) {
            const float e = key_to_float(ck[u]);
            const float kf = (float)(i + 1), ckf = (float)c_k, ckm = (float)(c_k - lab);
            // the reference's fp32 sequence (lovasz_losses.py:27-32): one correctly rounded division, one subtraction from 1, one
            // first difference; no fma contraction (the difference cancels ~3 digits)
            const float jk = __fsub_rn(1.f, __fdiv_rn(G - ckf, G + (kf - ckf)));
            float jm = 0.f;
            if (i > 0) jm = __fsub_rn(1.f, __fdiv_rn(G - ckm, G + ((kf - 1.f) - ckm)));
            const float gk = (i > 0) ? __fsub_rn(jk, jm) : jk;
            const float el = Pol::value(e);
            if constexpr (X::on) {
                const bool live = !(val & 2u) && !skip;           // a void element or a skipped row: no loss, a gradient of exactly 0
                if (live) lsum += el * gk;
                if (a.dlogits && (val >> 2) < (unsigned)P) a.dlogits[x_off<X>(a, x, b, val >> 2)] = live ? Pol::dvalue(e, lab) * gk * gscale : 0.f;
            } else {
                lsum += el * gk;
                if (dz && (!SP::guard || (val >> 1) < (unsigned)P)) dz[val >> 1] = Pol::dvalue(e, lab) * gk * gscale;
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) lsum += __shfl_xor(lsum, o);
    __syncthreads();
    if (lane == 0) red[wave] = lsum;
    __syncthreads();
    if (tid == 0) {
        float t = 0.f;
        for (int w = 0; w < SWV; ++w) t += red[w];
        sp.part[(int64_t)b * S + seg] = t;
    }
}

__global__ void lovasz_mean_split_kernel(const float* part, int B, int S, float scale, float* per_image, float* out) {
    __shared__ float sm[1024];
    const int tid = threadIdx.x;
    for (int b = tid; b < B; b += blockDim.x) {
        float t = 0.f;
        for (int s2 = 0; s2 < S; ++s2) t += part[b * S + s2];
        per_image[b] = t;
        if (b < 1024) sm[b] = t;
    }
    __syncthreads();
    if (tid == 0) {
        float t = 0.f;
        for (int b = 0; b < B; ++b) t += (b < 1024) ? sm[b] : per_image[b];
        out[0] = t * scale / (float)B;
    }
}

__global__ void mean_kernel(const float* v, int n, float scale, float* out) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        float s = 0.f;
        for (int i = 0; i < n; ++i) s += v[i];
        out[0] = s * scale / (float)n;
    }
}

// ---------------------------------------------------------------- long rows: more than SMAXSEG segments
// The [S][256] next-digit table of lovasz_pass_kernel does not fit LDS beyond 64 segments (512 segments: 512 KB), so the long-row form
// keeps the SAME stable LSD radix sort and moves the histograms to global memory, digit-major (LovaszLong).  Per pass:
//   count    (pass 0: the keys kernel) digit histogram of every source segment                  -> hist[row][digit][seg]
//   segscan  one workgroup per (row, digit): exclusive prefix over the segments in place, the digit's total -> tot[row][digit]
//   scatter  digit base = (exclusive prefix of tot over the digits) + hist[row][digit][seg]; ranking chunk by chunk exactly as
//            lovasz_pass_kernel
// then poscount (positives per sorted segment, plain stores), segscan over them (carry of the earlier segments and G), and
// lovasz_scan_kernel.  Launch boundaries are the only cross-workgroup synchronisation; there is no floating-point atomic and no
// global atomic at all, every sum has a fixed order: reruns are bit-identical.  Positions, ties and the fp32 sequence of g_k are
// lovasz_pf_kernel's, so the gradients equal it bit for bit.
__global__ __launch_bounds__(ST) void lovasz_count_kernel(salt_lovasz_args a, LovaszLong sp, int pass) {
    __shared__ unsigned h[256];
    const int b = blockIdx.x / sp.S, seg = blockIdx.x % sp.S, tid = threadIdx.x;
    const int P = a.P, i0 = seg * SL, i1 = min(i0 + SL, P);
    const unsigned* ki = a.ws_keys + ((int64_t)((pass & 1) ? a.B : 0) + b) * P;
    h[tid] = 0;
    __syncthreads();
    for (int i = i0 + tid; i < i1; i += ST) atomicAdd(&h[(ki[i] >> (pass * 8)) & 255u], 1u);
    __syncthreads();
    sp.first_histogram(a.B, b, seg, tid, h[tid]);
}

// workgroup w: arr[w][0 .. S) becomes its exclusive prefix, tot[w] its sum
__global__ __launch_bounds__(ST) void lovasz_segscan_kernel(unsigned* arr, unsigned* tot, int S) {
    __shared__ unsigned scan_w[SWV];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned* v = arr + (int64_t)blockIdx.x * S;
    unsigned carry = 0;
    for (int c0 = 0; c0 < S; c0 += ST) {
        const int i = c0 + tid;
        const unsigned c = i < S ? v[i] : 0u;
        unsigned incl = c;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const unsigned t = __shfl_up(incl, o); if (lane >= o) incl += t; }
        __syncthreads();                                          // scan_w of the previous chunk has been read
        if (lane == 63) scan_w[wave] = incl;
        __syncthreads();
        unsigned woff = carry, ctot = 0;
        for (int w = 0; w < SWV; ++w) { if (w < wave) woff += scan_w[w]; ctot += scan_w[w]; }
        if (i < S) v[i] = woff + incl - c;
        carry += ctot;
    }
    if (tid == 0) tot[blockIdx.x] = carry;
}

__global__ __launch_bounds__(ST) void lovasz_scatter_kernel(salt_lovasz_args a, LovaszLong sp, int pass) {
    __shared__ unsigned base[256];
    __shared__ unsigned wcount2[2][SWV][256];
    __shared__ unsigned scan_w[SWV];
    const int b = blockIdx.x / sp.S, seg = blockIdx.x % sp.S, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int P = a.P, S = sp.S, i0 = seg * SL;
    const unsigned* ki = a.ws_keys + ((int64_t)((pass & 1) ? a.B : 0) + b) * P;
    const unsigned* vi = a.ws_vals + ((int64_t)((pass & 1) ? a.B : 0) + b) * P;
    unsigned* ko = a.ws_keys + ((int64_t)((pass & 1) ? 0 : a.B) + b) * P;
    unsigned* vo = a.ws_vals + ((int64_t)((pass & 1) ? 0 : a.B) + b) * P;
    const int shift = pass * 8;
    unsigned ck[SCH], cv[SCH];
#pragma unroll
    for (int u = 0; u < SCH; ++u) { const int i = i0 + u * ST + tid; ck[u] = i < P ? ki[i] : 0u; cv[u] = i < P ? vi[i] : 0u; }
    {
        const unsigned tot = sp.tot[(int64_t)b * 256 + tid], before = sp.hist[((int64_t)b * 256 + tid) * S + seg];
        unsigned incl = tot;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const unsigned t = __shfl_up(incl, o); if (lane >= o) incl += t; }
        if (lane == 63) scan_w[wave] = incl;
        __syncthreads();
        unsigned woff = 0;
        for (int w = 0; w < wave; ++w) woff += scan_w[w];
        base[tid] = woff + incl - tot + before;
    }
    const unsigned long long lt_mask = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
#pragma unroll
    for (int u = 0; u < SCH; ++u) {
        const int c0 = i0 + u * ST;
        if (c0 >= P) break;                                       // uniform
        unsigned (*wcount)[256] = wcount2[u & 1];
#pragma unroll
        for (int w = 0; w < SWV; ++w) wcount[w][tid] = 0;
        __syncthreads();                                          // also publishes base[] on the first round
        const bool ok = c0 + tid < P;
        const unsigned key = ck[u];
        const unsigned d = ok ? ((key >> shift) & 255u) : 256u;
        unsigned long long m = __ballot(ok);
#pragma unroll
        for (int bit = 0; bit < 8; ++bit) {
            const unsigned long long bm = __ballot((d >> bit) & 1u);
            m &= ((d >> bit) & 1u) ? bm : ~bm;
        }
        const unsigned rank = (unsigned)__popcll(m & lt_mask);
        if (ok && rank == 0) wcount[wave][d] = (unsigned)__popcll(m);
        __syncthreads();
        {
            unsigned run = base[tid];
#pragma unroll
            for (int w = 0; w < SWV; ++w) { const unsigned c = wcount[w][tid]; wcount[w][tid] = run; run += c; }
            base[tid] = run;
        }
        __syncthreads();
        if (ok) {
            const unsigned dst = wcount[wave][d] + rank;
            if (dst < (unsigned)P) { ko[dst] = key; vo[dst] = cv[u]; }       // always true for consistent histograms; never write outside the row
        }
    }
}

__global__ __launch_bounds__(ST) void lovasz_poscount_kernel(salt_lovasz_args a, LovaszLong sp) {
    __shared__ unsigned cnt[SWV];
    const int b = blockIdx.x / sp.S, seg = blockIdx.x % sp.S, tid = threadIdx.x;
    const int P = a.P, i0 = seg * SL, i1 = min(i0 + SL, P);
    const unsigned* v0 = a.ws_vals + (int64_t)b * P;
    unsigned c = 0;
    for (int i = i0 + tid; i < i1; i += ST) c += v0[i] & 1u;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
    if ((tid & 63) == 0) cnt[tid >> 6] = c;
    __syncthreads();
    if (tid == 0) { unsigned t = 0; for (int w = 0; w < SWV; ++w) t += cnt[w]; sp.pos[(int64_t)b * sp.S + seg] = t; }
}

// ---------------------------------------------------------------- only-present: positives of every row before anything is sorted
constexpr int RPL = 8192;                // elements per workgroup of lovasz_rowpos_kernel
__global__ void lovasz_zero_kernel(unsigned* v, int n) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) v[i] = 0u;
}
__global__ __launch_bounds__(ST) void lovasz_rowpos_kernel(salt_lovasz_args a, LovaszX x, unsigned* rowpos, int parts) {
    const int b = blockIdx.x / parts, part = blockIdx.x % parts, tid = threadIdx.x;
    const int P = a.P, i0 = part * RPL, i1 = min(i0 + RPL, P);
    unsigned c = 0;
    for (int i = i0 + tid; i < i1; i += ST) {
        const float yi = a.target[x_off<XOpt>(a, x, b, i)];
        if (!((x.flags & XF_VOID) && yi == x.ignore) && yi > 0.5f) ++c;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
    if ((tid & 63) == 0 && c) atomicAdd(&rowpos[b], c);           // integer: the sum does not depend on the order
}

// Row losses from the per-segment partials (`part` NULL: per_row holds them already), then the mean in fixed order: over all rows, or
// (rowpos given) over the groups of C classes of the mean over each group's present classes, 0 for a group with none.
__global__ __launch_bounds__(ST) void lovasz_mean_x_kernel(const float* part, int S, float* per_row, int rows, int C, const unsigned* rowpos,
                                                           float scale, float* out) {
    __shared__ float red[ST];
    const int tid = threadIdx.x;
    if (part && S <= SMAXSEG) {
        for (int b = tid; b < rows; b += ST) {
            float t = 0.f;
            for (int s2 = 0; s2 < S; ++s2) t += part[(int64_t)b * S + s2];
            per_row[b] = t;
        }
    } else if (part) {
        for (int b = 0; b < rows; ++b) {
            float t = 0.f;
            for (int j = tid; j < S; j += ST) t += part[(int64_t)b * S + j];
            red[tid] = t;
            __syncthreads();
            for (int o = ST / 2; o > 0; o >>= 1) { if (tid < o) red[tid] += red[tid + o]; __syncthreads(); }
            if (tid == 0) per_row[b] = red[0];
            __syncthreads();
        }
    }
    __syncthreads();
    if (tid != 0) return;
    float t = 0.f;
    if (!rowpos) {
        for (int b = 0; b < rows; ++b) t += per_row[b];
        out[0] = t * scale / (float)rows;
        return;
    }
    const int groups = rows / C;
    for (int g = 0; g < groups; ++g) {
        float lg = 0.f; int present = 0;
        for (int c = 0; c < C; ++c) if (rowpos[g * C + c] > 0u) { lg += per_row[g * C + c]; ++present; }
        if (present) t += lg / (float)present;
    }
    out[0] = t * scale / (float)groups;
}

// words per row of salt_lovasz_args.ws_split (0: the split form does not apply to this size)
inline int64_t lovasz_split_words(int P) {
    const int S = (P + SL - 1) / SL;
    if (P < 2 * SL || S > SMAXSEG) return 0;
    return (int64_t)3 * S * 256 + 2 * S;
}

// words per row of salt_lovasz_args.ws_flat (0: the long-row form does not apply to this size)
constexpr int64_t LOVASZ_MAX_ROW = ((int64_t)1 << 31) - 2 * SL, LOVASZ_MAX_ROW_VOID = (int64_t)1 << 30;
inline int64_t lovasz_flat_words(int64_t N) {
    const int64_t S = (N + SL - 1) / SL;
    if (N < 1 || N > LOVASZ_MAX_ROW || S <= SMAXSEG) return 0;
    return 258 * S + 257;
}

// The launches of one Lovasz loss with row options (X) and / or long rows; `rowpos`: NULL, or [a->B] words for only-present.
template <class Pol, class X>
int lovasz_launch_x(const salt_lovasz_args* a, LovaszX x, unsigned* rowpos, hipStream_t st) {
    const int S = (int)(((int64_t)a->P + SL - 1) / SL), R = a->B;
    if ((int64_t)R * S > 0x7fffffff) SALT_FAIL(SALT_E_BADARG, "lovasz: %d rows of %d segments", R, S);
    x.rowpos = nullptr;
    if constexpr (X::on) {
        if (rowpos) {
            const int parts = a->P > 0 ? (a->P + RPL - 1) / RPL : 1;
            SALT_TRY(salt_launch(lovasz_zero_kernel, dim3((R + 255) / 256), dim3(256), 0, st, rowpos, R));
            SALT_TRY(salt_launch(lovasz_rowpos_kernel, dim3(R * parts), dim3(ST), 0, st, *a, x, rowpos, parts));
            x.rowpos = rowpos;
        }
    }
    const int C = x.rowpos ? x.C : 1;
    const dim3 grid(R * S);
    if (a->ws_flat && S > SMAXSEG) {
        unsigned* w = a->ws_flat;
        LovaszLong sp;
        sp.S = S;
        sp.hist = w; w += (int64_t)R * 256 * S;
        sp.tot = w; w += (int64_t)R * 256;
        sp.pos = w; w += (int64_t)R * S;
        sp.postot = w; w += R;
        sp.part = reinterpret_cast<float*>(w);
        SALT_TRY(salt_launch(lovasz_keys_kernel<Pol, X, LovaszLong>, grid, dim3(ST), 0, st, *a, sp, x));
        for (int pass = 0; pass < 4; ++pass) {
            if (pass) SALT_TRY(salt_launch(lovasz_count_kernel, grid, dim3(ST), 0, st, *a, sp, pass));
            SALT_TRY(salt_launch(lovasz_segscan_kernel, dim3(R * 256), dim3(ST), 0, st, sp.hist, sp.tot, S));
            SALT_TRY(salt_launch(lovasz_scatter_kernel, grid, dim3(ST), 0, st, *a, sp, pass));
        }
        SALT_TRY(salt_launch(lovasz_poscount_kernel, grid, dim3(ST), 0, st, *a, sp));
        SALT_TRY(salt_launch(lovasz_segscan_kernel, dim3(R), dim3(ST), 0, st, sp.pos, sp.postot, S));
        SALT_TRY(salt_launch(lovasz_scan_kernel<Pol, X, LovaszLong>, grid, dim3(ST), 0, st, *a, sp, x));
        return salt_launch(lovasz_mean_x_kernel, dim3(1), dim3(ST), 0, st, (const float*)sp.part, S, a->loss_per_image, R, C, x.rowpos, a->loss_scale, a->loss);
    }
    if (a->ws_split && a->P >= 2 * SL && S <= SMAXSEG) {
        LovaszSplit sp{S, a->ws_split, a->ws_split + (int64_t)3 * R * S * 256, reinterpret_cast<float*>(a->ws_split + (int64_t)3 * R * S * 256 + (int64_t)R * S)};
        SALT_TRY(salt_launch(lovasz_keys_kernel<Pol, X, LovaszSplit>, grid, dim3(ST), 0, st, *a, sp, x));
        const size_t lds = (size_t)(S * 256 + S) * sizeof(unsigned);
        for (int pass = 0; pass < 4; ++pass) SALT_TRY(salt_launch(lovasz_pass_kernel, grid, dim3(ST), lds, st, *a, sp, pass));
        SALT_TRY(salt_launch(lovasz_scan_kernel<Pol, X, LovaszSplit>, grid, dim3(ST), 0, st, *a, sp, x));
        return salt_launch(lovasz_mean_x_kernel, dim3(1), dim3(ST), 0, st, (const float*)sp.part, S, a->loss_per_image, R, C, x.rowpos, a->loss_scale, a->loss);
    }
    SALT_TRY(salt_launch(lovasz_pf_kernel<Pol, X>, dim3(R), dim3(LT), 0, st, *a, x));
    return salt_launch(lovasz_mean_x_kernel, dim3(1), dim3(ST), 0, st, (const float*)nullptr, 0, a->loss_per_image, R, C, x.rowpos, a->loss_scale, a->loss);
}

// The launches of one Lovasz loss without row options over a->B rows of a->P elements (arguments already checked by the entry point):
// the shortest form that fits the row - one workgroup, the split form, the long-row form.
template <class Pol>
int lovasz_launch(const salt_lovasz_args* a, hipStream_t st) {
    const int S = (int)(((int64_t)a->P + SL - 1) / SL);
    if (a->ws_flat && S > SMAXSEG) return lovasz_launch_x<Pol, XPlain>(a, LovaszX{}, nullptr, st);
    if (a->ws_split && a->P >= 2 * SL && S <= SMAXSEG) {
        LovaszSplit sp{S, a->ws_split, a->ws_split + (int64_t)3 * a->B * S * 256, reinterpret_cast<float*>(a->ws_split + (int64_t)3 * a->B * S * 256 + (int64_t)a->B * S)};
        const dim3 grid(a->B * S);
        SALT_TRY(salt_launch(lovasz_keys_kernel<Pol, XPlain, LovaszSplit>, grid, dim3(ST), 0, st, *a, sp, LovaszX{}));
        const size_t lds = (size_t)(S * 256 + S) * sizeof(unsigned);
        for (int pass = 0; pass < 4; ++pass) SALT_TRY(salt_launch(lovasz_pass_kernel, grid, dim3(ST), lds, st, *a, sp, pass));
        SALT_TRY(salt_launch(lovasz_scan_kernel<Pol, XPlain, LovaszSplit>, grid, dim3(ST), 0, st, *a, sp, LovaszX{}));
        return salt_launch(lovasz_mean_split_kernel, dim3(1), dim3(256), 0, st, sp.part, a->B, S, a->loss_scale, a->loss_per_image, a->loss);
    }
    SALT_TRY(salt_launch(lovasz_pf_kernel<Pol, XPlain>, dim3(a->B), dim3(LT), 0, st, *a, LovaszX{}));
    return salt_launch(mean_kernel, dim3(1), dim3(64), 0, st, a->loss_per_image, a->B, a->loss_scale, a->loss);
}

// The option fields shared by salt_lovasz_args and salt_lovasz_softmax_args, checked on the host: 0 or the reason of the refusal.
inline const char* lovasz_flags_refusal(int flags, float ignore, bool softmax) {
    if (flags & ~(SALT_LOVASZ_BATCH_FLAT | SALT_LOVASZ_ONLY_PRESENT | SALT_LOVASZ_HAS_IGNORE)) return "unknown flag bit";
    if ((flags & SALT_LOVASZ_ONLY_PRESENT) && !softmax) return "only-present is an option of the softmax form";
    if ((flags & SALT_LOVASZ_HAS_IGNORE) && ignore != ignore) return "the ignore value is NaN";
    return nullptr;
}

// parts per plane of the partial-sum losses: one up to 4096 positions, never more than 16; *per = positions per part
inline int bce_ppp(int HW, int* per) {
    int ppp = cdiv(HW, 4096);
    if (ppp > 16) ppp = 16;
    if (ppp < 1) ppp = 1;
    const int pp = cdiv(HW, ppp);
    if (per) *per = pp;
    return cdiv(HW, pp);
}

}  // namespace
