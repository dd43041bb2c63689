// augment.hip — on-device training augmentation fused with the train-branch preprocessing (salt_augment_preprocess).
//
// The reference augments every training tile on the CPU with imgaug (main.py:130-133, loaders.py:124-150, augmentation.py:34-65):
// affine_seq on the 101x101 uint8 image and the mask planes, resize + pad, intensity_seq on the padded image.  Here one workgroup
// takes one image: the image and mask planes sit in LDS and ping-pong between the geometric stages (each stage writes the uint8
// grid, as imgaug does between augmenters), then every thread produces output pixels: the fixed-point cubic resize + edge pad of
// salt_preprocess, the intensity ops on the padded grid, normalisation, depth channels and the one-hot target.  The conventions
// imgaug / cv2 / skimage cannot pin here (border modes, rounding, grids) are the ones documented in saltnet.h and DESIGN.md.
#include "preprocess_common.h"

namespace {

constexpr int MAXT = SALT_AUG_MAX_TILE;
constexpr int RMAX = SALT_AUG_RECT_MAX;
constexpr int NP = SALT_AUG_PARAMS;
constexpr int NT = 256;

// params record slots (saltnet.h)
enum : int {
    P_ORDER = 0, P_N = 1, P_CHOSEN = 2, P_FLIP = 6, P_ANGLE = 7, P_SHIFT = 8, P_PW_ON = 9, P_PW_SCALE = 10, P_PW_JIT = 11,
    P_PS_ON = 43, P_PS_SCALE = 44, P_PS_CORNER = 45, P_INVERT = 53, P_CONTRAST_ON = 54, P_CONTRAST = 55, P_OP = 56, P_VALUE = 57
};

// RNG draw slots
enum : uint64_t {
    S_ORDER = 0, S_N = 1, S_PICK1 = 2, S_PICK2 = 3, S_FLIP = 4, S_ANGLE = 5, S_SHIFT = 6, S_PW_ON = 7, S_PW_SCALE = 8, S_PS_ON = 10,
    S_PS_SCALE = 11, S_INVERT = 12, S_CONTRAST_ON = 13, S_CONTRAST = 14, S_NOOP = 15, S_OP = 16, S_VALUE = 17, S_NORMAL = 64,
    S_PIXEL = 1024
};

struct AugKP {
    const unsigned char* img; const unsigned char* mask; float* x; float* target;
    int B, h, w, rh, rw, top, left, H, W, channels, pad_mode;
    float mean[3], inv_std[3];
    salt_augment_config cfg;
    uint64_t seed, counter;
    float* params; int params_given;
    unsigned char* geo_img; unsigned char* geo_mask; unsigned char* gray;
};

__device__ __forceinline__ uint64_t mix64(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__device__ __forceinline__ uint64_t draw_bits(uint64_t key, uint64_t slot) { return mix64(key + slot * 0x9E3779B97F4A7C15ull); }
__device__ __forceinline__ float draw_u(uint64_t key, uint64_t slot) { return (float)(draw_bits(key, slot) >> 40) * (1.f / 16777216.f); }
__device__ __forceinline__ int draw_int(uint64_t key, uint64_t slot, int lo, int hi) {
    return lo + (int)(((draw_bits(key, slot) >> 32) * (uint64_t)(hi - lo + 1)) >> 32);
}
__device__ __forceinline__ float draw_range(uint64_t key, uint64_t slot, float lo, float hi) {
    return __fadd_rn(lo, __fmul_rn(draw_u(key, slot), __fsub_rn(hi, lo)));
}
__device__ __forceinline__ float draw_normal(uint64_t key, int k) {
    const float u1 = (float)((draw_bits(key, S_NORMAL + 2 * k) >> 40) + 1) * (1.f / 16777216.f);
    const float u2 = draw_u(key, S_NORMAL + 2 * k + 1);
    return sqrtf(-2.f * logf(u1)) * cosf(6.28318530717958647f * u2);
}

// uint8 write-back of every stage: round half up, clip to [0, 255]
__device__ __forceinline__ unsigned char to_u8(float v) {
    return (unsigned char)fminf(fmaxf(floorf(__fadd_rn(v, 0.5f)), 0.f), 255.f);
}

// bilinear sample of a uint8 plane at (sy, sx); edge: indices clamped (mode 'edge'), else taps outside read 0 (constant 0)
__device__ __forceinline__ float bilinear(const unsigned char* pl, int h, int w, float sy, float sx, bool edge) {
    sy = fminf(fmaxf(sy, -2.f), (float)h + 1.f);                   // far outside: every tap is out (or clamped) either way
    sx = fminf(fmaxf(sx, -2.f), (float)w + 1.f);
    const float y0f = floorf(sy), x0f = floorf(sx);
    const float fy = __fsub_rn(sy, y0f), fx = __fsub_rn(sx, x0f);
    const int y0 = (int)y0f, x0 = (int)x0f;
    auto tap = [&](int yy, int xx) -> float {
        if (edge) return (float)pl[min(max(yy, 0), h - 1) * w + min(max(xx, 0), w - 1)];
        return (yy >= 0 && yy < h && xx >= 0 && xx < w) ? (float)pl[yy * w + xx] : 0.f;
    };
    const float gx = __fsub_rn(1.f, fx), gy = __fsub_rn(1.f, fy);
    const float top = __fadd_rn(__fmul_rn(gx, tap(y0, x0)), __fmul_rn(fx, tap(y0, x0 + 1)));
    const float bot = __fadd_rn(__fmul_rn(gx, tap(y0 + 1, x0)), __fmul_rn(fx, tap(y0 + 1, x0 + 1)));
    return __fadd_rn(__fmul_rn(gy, top), __fmul_rn(fy, bot));
}

// v / 255 as salt_preprocess rounds it: a product of its own, never fused with the mean subtraction that follows
__device__ __forceinline__ float u8_to_unit(int v) {
#pragma clang fp contract(off)
    return (float)v * (1.f / 255.f);
}

using salt_pre::reflect101;

// cv2.filter2D (correlation) with a reflect-101 border, the 9 products summed row by row, each operation rounded on its own
__device__ void conv3x3(const unsigned char* src, unsigned char* dst, int h, int w, const float (&k)[9], bool binarize) {
    for (int i = threadIdx.x; i < h * w; i += NT) {
        const int y = i / w, x = i - (i / w) * w;
        float acc = 0.f;
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
            for (int dx = 0; dx < 3; ++dx)
                acc = __fadd_rn(acc, __fmul_rn(k[dy * 3 + dx], (float)src[reflect101(y + dy - 1, h) * w + reflect101(x + dx - 1, w)]));
        const unsigned char v = to_u8(acc);
        dst[i] = binarize ? (unsigned char)(v != 0) : v;
    }
}

__device__ __forceinline__ float pw_point(const float* J, int h, int w, int i, int j, int c) {   // jittered control point, c 0: y, 1: x
    const float reg = c == 0 ? __fdiv_rn((float)(i * h), 3.f) : __fdiv_rn((float)(j * w), 3.f);
    return __fadd_rn(reg, __fmul_rn(J[2 * (4 * i + j) + c], (float)(c == 0 ? h : w)));
}

__global__ __launch_bounds__(NT) void augment_kernel(AugKP p) {
    __shared__ unsigned char s_img[2][MAXT * MAXT];
    __shared__ unsigned char s_msk[2][MAXT * MAXT];
    __shared__ unsigned char s_rect[RMAX * RMAX];
    __shared__ float s_prm[NP];
    __shared__ float s_geo[10];                                   // affine: cos, sin; perspective: homography a..h

    const int b = blockIdx.x, tid = threadIdx.x, h = p.h, w = p.w, n = h * w;
    const bool has_mask = p.mask != nullptr;
    const uint64_t key = mix64(mix64(mix64(p.seed) ^ p.counter) ^ (uint64_t)b);
    const salt_augment_config& c = p.cfg;

    // ---- the parameters of this image: drawn by one thread, or the given record
    if (p.params_given) {
        if (tid < NP) s_prm[tid] = p.params[(int64_t)b * NP + tid];
    } else if (tid == 0) {
        float* q = s_prm;
        for (int i = 0; i < NP; ++i) q[i] = 0.f;
        q[P_ORDER] = (float)draw_int(key, S_ORDER, 0, 5);
        int en[4], k = 0;
        const int bits[4] = {SALT_AUG_FLIPLR, SALT_AUG_SHARPEN, SALT_AUG_EMBOSS, SALT_AUG_AFFINE};
        for (int i = 0; i < 4; ++i)
            if (c.enable & bits[i]) en[k++] = i;
        if (k > 0) {
            const int nn = min(draw_int(key, S_N, 1, 2), k);
            q[P_N] = (float)nn;
            const int a = draw_int(key, S_PICK1, 0, k - 1);
            q[P_CHOSEN + en[a]] = 1.f;
            if (nn == 2) {
                int bb = draw_int(key, S_PICK2, 0, k - 2);
                bb += bb >= a ? 1 : 0;                            // the second pick among the remaining ones
                q[P_CHOSEN + en[bb]] = 1.f;
            }
        }
        if (q[P_CHOSEN + 0] != 0.f) q[P_FLIP] = draw_u(key, S_FLIP) < c.p_fliplr ? 1.f : 0.f;
        if (q[P_CHOSEN + 3] != 0.f) {
            q[P_ANGLE] = draw_range(key, S_ANGLE, c.rotate_min, c.rotate_max);
            q[P_SHIFT] = draw_range(key, S_SHIFT, c.shift_min, c.shift_max);
        }
        if ((c.enable & SALT_AUG_PIECEWISE) && draw_u(key, S_PW_ON) < c.p_piecewise) {
            const float s = draw_range(key, S_PW_SCALE, c.piecewise_scale_min, c.piecewise_scale_max);
            q[P_PW_ON] = 1.f; q[P_PW_SCALE] = s;
            for (int i = 0; i < 32; ++i) q[P_PW_JIT + i] = draw_normal(key, i) * s;
        }
        if ((c.enable & SALT_AUG_PERSPECTIVE) && draw_u(key, S_PS_ON) < c.p_perspective) {
            const float s = draw_range(key, S_PS_SCALE, c.perspective_scale_min, c.perspective_scale_max);
            q[P_PS_ON] = 1.f; q[P_PS_SCALE] = s;
            for (int i = 0; i < 8; ++i) q[P_PS_CORNER + i] = fmodf(fabsf(draw_normal(key, 32 + i) * s), 1.f);
        }
        if ((c.enable & SALT_AUG_INVERT) && draw_u(key, S_INVERT) < c.p_invert) q[P_INVERT] = 1.f;
        if ((c.enable & SALT_AUG_CONTRAST) && draw_u(key, S_CONTRAST_ON) < c.p_contrast) {
            q[P_CONTRAST_ON] = 1.f;
            q[P_CONTRAST] = draw_range(key, S_CONTRAST, c.contrast_min, c.contrast_max);
        }
        int ops[4], ko = 0;
        const int obits[4] = {SALT_AUG_ADD, SALT_AUG_ADD_ELEMENTWISE, SALT_AUG_MULTIPLY, SALT_AUG_MULTIPLY_ELEMENTWISE};
        for (int i = 0; i < 4; ++i)
            if (c.enable & obits[i]) ops[ko++] = i + 1;
        if (ko > 0 && !(draw_u(key, S_NOOP) < c.p_intensity_noop)) {
            const int op = ops[draw_int(key, S_OP, 0, ko - 1)];
            q[P_OP] = (float)op;
            if (op == 1) q[P_VALUE] = (float)draw_int(key, S_VALUE, c.add_min, c.add_max);
            if (op == 3) q[P_VALUE] = draw_range(key, S_VALUE, c.mul_min, c.mul_max);
        }
    }
    // ---- the tile into LDS (mask binarised)
    const unsigned char* im = p.img + (int64_t)b * n;
    const unsigned char* mk = has_mask ? p.mask + (int64_t)b * n : nullptr;
    for (int i = tid; i < n; i += NT) {
        s_img[0][i] = im[i];
        s_msk[0][i] = has_mask ? (unsigned char)(mk[i] != 0) : 0;
    }
    __syncthreads();
    if (p.params && !p.params_given && tid < NP) p.params[(int64_t)b * NP + tid] = s_prm[tid];   // the record, one float per thread

    int cur = 0;
    auto flip = [&]() {
        __syncthreads();
        cur ^= 1;
    };
    const int order = min(max((int)s_prm[P_ORDER], 0), 5);
    const int perm[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
    for (int st = 0; st < 3; ++st) {
        const int stage = perm[order][st];
        if (stage == 0) {                                                  // A: the chosen children in list order
            if (s_prm[P_CHOSEN + 0] != 0.f && s_prm[P_FLIP] != 0.f) {
                for (int i = tid; i < n; i += NT) {
                    const int y = i / w, x = i - (i / w) * w, j = y * w + (w - 1 - x);
                    s_img[cur ^ 1][i] = s_img[cur][j];
                    s_msk[cur ^ 1][i] = s_msk[cur][j];
                }
                flip();
            }
            for (int e = 1; e <= 2; ++e) {
                if (s_prm[P_CHOSEN + e] == 0.f) continue;
                float k[9];
                if (e == 1) {                                              // Sharpen
                    const float a = c.sharpen_alpha, L = c.sharpen_lightness;
                    for (int t = 0; t < 9; ++t) k[t] = __fmul_rn(a, -1.f);
                    k[4] = __fadd_rn(__fsub_rn(1.f, a), __fmul_rn(a, __fadd_rn(8.f, L)));
                } else {                                                   // Emboss
                    const float a = c.emboss_alpha, s = c.emboss_strength;
                    const float m[9] = {-1.f - s, -s, 0.f, -s, 1.f, s, 0.f, s, 1.f + s};
                    for (int t = 0; t < 9; ++t) k[t] = __fmul_rn(a, m[t]);
                    k[4] = __fadd_rn(__fsub_rn(1.f, a), k[4]);
                }
                conv3x3(s_img[cur], s_img[cur ^ 1], h, w, k, false);
                conv3x3(s_msk[cur], s_msk[cur ^ 1], h, w, k, true);
                flip();
            }
            if (s_prm[P_CHOSEN + 3] != 0.f) {                              // Affine: rotate about the centre, shift x, mode 'edge'
                if (tid == 0) {
                    const double rad = (double)s_prm[P_ANGLE] * 0.017453292519943295;   // in double: cos / sin rounded once to float
                    s_geo[0] = (float)cos(rad); s_geo[1] = (float)sin(rad);
                }
                __syncthreads();
                const float cs = s_geo[0], sn = s_geo[1];
                const float cx = __fsub_rn(__fmul_rn((float)w, 0.5f), 0.5f), cy = __fsub_rn(__fmul_rn((float)h, 0.5f), 0.5f);
                const float tx = __fmul_rn(s_prm[P_SHIFT], (float)w);
                for (int i = tid; i < n; i += NT) {
                    const int y = i / w, x = i - (i / w) * w;
                    const float dx = __fsub_rn(__fsub_rn((float)x, cx), tx), dy = __fsub_rn((float)y, cy);
                    const float sx = __fadd_rn(__fadd_rn(__fmul_rn(cs, dx), __fmul_rn(sn, dy)), cx);
                    const float sy = __fadd_rn(__fsub_rn(__fmul_rn(cs, dy), __fmul_rn(sn, dx)), cy);
                    s_img[cur ^ 1][i] = to_u8(bilinear(s_img[cur], h, w, sy, sx, true));
                    s_msk[cur ^ 1][i] = to_u8(bilinear(s_msk[cur], h, w, sy, sx, true)) != 0;
                }
                flip();
            }
        } else if (stage == 1 && s_prm[P_PW_ON] != 0.f) {                 // B: PiecewiseAffine
            const float* J = s_prm + P_PW_JIT;
            for (int i = tid; i < n; i += NT) {
                const int y = i / w, x = i - (i / w) * w;
                const int ci = min(3 * y / h, 2), cj = min(3 * x / w, 2);
                const float v = __fsub_rn(__fdiv_rn((float)(3 * y), (float)h), (float)ci);   // local coordinates in the regular cell
                const float u = __fsub_rn(__fdiv_rn((float)(3 * x), (float)w), (float)cj);
                float sp[2];
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    const float tl = pw_point(J, h, w, ci, cj, q), br = pw_point(J, h, w, ci + 1, cj + 1, q);
                    if (u >= v) {                                        // triangle TL, TR, BR
                        const float tr = pw_point(J, h, w, ci, cj + 1, q);
                        sp[q] = __fadd_rn(__fadd_rn(tl, __fmul_rn(u, __fsub_rn(tr, tl))), __fmul_rn(v, __fsub_rn(br, tr)));
                    } else {                                             // triangle TL, BL, BR
                        const float bl = pw_point(J, h, w, ci + 1, cj, q);
                        sp[q] = __fadd_rn(__fadd_rn(tl, __fmul_rn(v, __fsub_rn(bl, tl))), __fmul_rn(u, __fsub_rn(br, bl)));
                    }
                }
                s_img[cur ^ 1][i] = to_u8(bilinear(s_img[cur], h, w, sp[0], sp[1], false));
                s_msk[cur ^ 1][i] = to_u8(bilinear(s_msk[cur], h, w, sp[0], sp[1], false)) != 0;
            }
            flip();
        } else if (stage == 2 && s_prm[P_PS_ON] != 0.f) {                 // C: PerspectiveTransform onto the rectified quad, cubic back
            if (tid == 0) {
                const float* q = s_prm + P_PS_CORNER;
                const float fw = (float)w, fh = (float)h;
                const float x0 = __fmul_rn(q[0], fw), y0 = __fmul_rn(q[1], fh);                                   // tl
                const float x1 = __fsub_rn(fw, __fmul_rn(q[2], fw)), y1 = __fmul_rn(q[3], fh);                    // tr
                const float x2 = __fsub_rn(fw, __fmul_rn(q[4], fw)), y2 = __fsub_rn(fh, __fmul_rn(q[5], fh));     // br
                const float x3 = __fmul_rn(q[6], fw), y3 = __fsub_rn(fh, __fmul_rn(q[7], fh));                    // bl
                auto len = [](float ax, float ay, float bx, float by) {
                    const float dx = __fsub_rn(ax, bx), dy = __fsub_rn(ay, by);
                    return (int)__fsqrt_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)));
                };
                const int mw = max(len(x2, y2, x3, y3), len(x1, y1, x0, y0));
                const int mh = max(len(x3, y3, x0, y0), len(x2, y2, x1, y1));
                // unit square (s, t) -> quad tl, tr, br, bl (Heckbert's square-to-quad projective map)
                const float sx = __fsub_rn(__fadd_rn(__fsub_rn(x0, x1), x2), x3), sy = __fsub_rn(__fadd_rn(__fsub_rn(y0, y1), y2), y3);
                const float dx1 = __fsub_rn(x1, x2), dx2 = __fsub_rn(x3, x2), dy1 = __fsub_rn(y1, y2), dy2 = __fsub_rn(y3, y2);
                const float den = __fsub_rn(__fmul_rn(dx1, dy2), __fmul_rn(dx2, dy1));
                const float g = den != 0.f ? __fdiv_rn(__fsub_rn(__fmul_rn(sx, dy2), __fmul_rn(dx2, sy)), den) : 0.f;
                const float hh = den != 0.f ? __fdiv_rn(__fsub_rn(__fmul_rn(dx1, sy), __fmul_rn(sx, dy1)), den) : 0.f;
                s_geo[0] = __fadd_rn(__fsub_rn(x1, x0), __fmul_rn(g, x1)); s_geo[1] = __fadd_rn(__fsub_rn(x3, x0), __fmul_rn(hh, x3)); s_geo[2] = x0;
                s_geo[3] = __fadd_rn(__fsub_rn(y1, y0), __fmul_rn(g, y1)); s_geo[4] = __fadd_rn(__fsub_rn(y3, y0), __fmul_rn(hh, y3)); s_geo[5] = y0;
                s_geo[6] = g; s_geo[7] = hh;
                s_geo[8] = (float)min(max(mw, 2), RMAX); s_geo[9] = (float)min(max(mh, 2), RMAX);
            }
            __syncthreads();
            const int mw = (int)s_geo[8], mh = (int)s_geo[9];
            const float is = __fdiv_rn(1.f, (float)(mw - 1)), it = __fdiv_rn(1.f, (float)(mh - 1));
            for (int plane = 0; plane < (has_mask ? 2 : 1); ++plane) {
                const unsigned char* src = plane ? s_msk[cur] : s_img[cur];
                unsigned char* dst = plane ? s_msk[cur ^ 1] : s_img[cur ^ 1];
                for (int i = tid; i < mw * mh; i += NT) {
                    const int v = i / mw, u = i - (i / mw) * mw;
                    const float s = __fmul_rn((float)u, is), t = __fmul_rn((float)v, it);
                    const float z = __fadd_rn(__fadd_rn(__fmul_rn(s_geo[6], s), __fmul_rn(s_geo[7], t)), 1.f);
                    const float X = __fdiv_rn(__fadd_rn(__fadd_rn(__fmul_rn(s_geo[0], s), __fmul_rn(s_geo[1], t)), s_geo[2]), z);
                    const float Y = __fdiv_rn(__fadd_rn(__fadd_rn(__fmul_rn(s_geo[3], s), __fmul_rn(s_geo[4], t)), s_geo[5]), z);
                    const unsigned char r = to_u8(bilinear(src, h, w, Y, X, false));
                    s_rect[i] = plane ? (unsigned char)(r != 0) : r;
                }
                __syncthreads();
                const float scy = __fdiv_rn((float)mh, (float)h), scx = __fdiv_rn((float)mw, (float)w);
                for (int i = tid; i < n; i += NT) {
                    const int y = i / w, x = i - (i / w) * w;
                    const float fy = __fsub_rn(__fmul_rn(__fadd_rn((float)y, 0.5f), scy), 0.5f);
                    const float fx = __fsub_rn(__fmul_rn(__fadd_rn((float)x, 0.5f), scx), 0.5f);
                    const float y0f = floorf(fy), x0f = floorf(fx);
                    float wy[4], wx[4];
                    salt_pre::cubic_w_rn(__fsub_rn(fy, y0f), wy);
                    salt_pre::cubic_w_rn(__fsub_rn(fx, x0f), wx);
                    const int y0 = (int)y0f - 1, x0 = (int)x0f - 1;
                    float acc = 0.f;
                    for (int a = 0; a < 4; ++a) {
                        const int yy = min(max(y0 + a, 0), mh - 1);
                        float row = 0.f;
                        for (int bb = 0; bb < 4; ++bb)
                            row = __fadd_rn(row, __fmul_rn(wx[bb], (float)s_rect[yy * mw + min(max(x0 + bb, 0), mw - 1)]));
                        acc = __fadd_rn(acc, __fmul_rn(wy[a], row));
                    }
                    const unsigned char r = to_u8(acc);
                    dst[i] = plane ? (unsigned char)(r != 0) : r;
                }
                __syncthreads();
            }
            cur ^= 1;
        }
    }
    if (p.geo_img || p.geo_mask) {
        for (int i = tid; i < n; i += NT) {
            if (p.geo_img) p.geo_img[(int64_t)b * n + i] = s_img[cur][i];
            if (p.geo_mask) p.geo_mask[(int64_t)b * n + i] = s_msk[cur][i];
        }
    }

    // ---- resize + pad (edge | reflect-101) (salt_preprocess interpolation 2), intensity, normalisation, one-hot target
    const bool invert = s_prm[P_INVERT] != 0.f, contrast = s_prm[P_CONTRAST_ON] != 0.f;
    const float alpha = s_prm[P_CONTRAST], value = s_prm[P_VALUE];
    const int op = (int)s_prm[P_OP];
    const bool resize = p.rh != h || p.rw != w;
    const double sy = 1.0 / ((double)p.rh / (double)h), sx = 1.0 / ((double)p.rw / (double)w);
    const int HW = p.H * p.W;
    for (int i = tid; i < HW; i += NT) {
        const int Y = i / p.W, X = i - (i / p.W) * p.W;
        const int ry = salt_pre::pad_index(Y, p.top, p.rh, p.pad_mode), rx = salt_pre::pad_index(X, p.left, p.rw, p.pad_mode);
        int v, m;
        if (resize) {
            int y0, x0, cy[4], cx[4];
            salt_pre::cubic_coef_fixed(ry, sy, y0, cy);
            salt_pre::cubic_coef_fixed(rx, sx, x0, cx);
            v = salt_pre::fixed_to_u8(salt_pre::cubic_fixed_acc(s_img[cur], h, w, y0, cy, x0, cx, false));
            m = has_mask ? (salt_pre::fixed_to_u8(salt_pre::cubic_fixed_acc(s_msk[cur], h, w, y0, cy, x0, cx, true)) > 0 ? 1 : 0) : 0;
        } else {
            v = s_img[cur][ry * w + rx];
            m = s_msk[cur][ry * w + rx];
        }
        if (invert) v = 255 - v;
        if (contrast) v = to_u8(__fadd_rn(__fmul_rn(alpha, (float)(v - 128)), 128.f));
        if (op == 1) {
            v = min(max(v + (int)value, 0), 255);
        } else if (op == 2) {
            v = min(max(v + draw_int(key, S_PIXEL + (uint64_t)i, p.cfg.add_min, p.cfg.add_max), 0), 255);
        } else if (op == 3) {
            v = to_u8(__fmul_rn((float)v, value));
        } else if (op == 4) {
            v = to_u8(__fmul_rn((float)v, draw_range(key, S_PIXEL + (uint64_t)i, p.cfg.mul_min, p.cfg.mul_max)));
        }
        if (p.gray) p.gray[(int64_t)b * HW + i] = (unsigned char)v;
        salt_pre::store_x_target(p.x, has_mask ? p.target : nullptr, b, Y, X, p.H, p.W, p.channels, p.mean, p.inv_std,
                                 u8_to_unit(v), (float)m);
    }
}

}  // namespace

extern "C" int salt_augment_preprocess(const salt_augment_preprocess_args* a, void* stream) {
    if (!a || !a->img || !a->x || a->B < 1 || a->h < 1 || a->w < 1 || a->H < 1 || a->W < 1 || (a->channels != 1 && a->channels != 3) ||
        a->top < 0 || a->left < 0 || (a->mask && !a->target))
        SALT_FAIL(SALT_E_BADARG, "augment_preprocess: bad args");
    if (a->h > SALT_AUG_MAX_TILE || a->w > SALT_AUG_MAX_TILE)
        SALT_FAIL(SALT_E_BADARG, "augment_preprocess: tiles up to %dx%d (got %dx%d)", SALT_AUG_MAX_TILE, SALT_AUG_MAX_TILE, a->h, a->w);
    if (a->params_given && !a->params) SALT_FAIL(SALT_E_BADARG, "augment_preprocess: params_given without a params record");
    const salt_augment_config& c = a->cfg;
    if (c.add_min > c.add_max || c.add_min < -255 || c.add_max > 255) SALT_FAIL(SALT_E_BADARG, "augment_preprocess: add range");
    AugKP p;
    p.img = a->img; p.mask = a->mask; p.x = a->x; p.target = a->target;
    p.B = a->B; p.h = a->h; p.w = a->w;
    p.rh = a->resize_h > 0 ? a->resize_h : a->h; p.rw = a->resize_w > 0 ? a->resize_w : a->w;
    p.top = a->top; p.left = a->left; p.H = a->H; p.W = a->W; p.channels = a->channels;
    if (p.top + p.rh > p.H || p.left + p.rw > p.W) SALT_FAIL(SALT_E_BADARG, "augment_preprocess: resized tile + pad offset exceeds the output");
    if ((int64_t)p.H * p.W >= (1ll << 30)) SALT_FAIL(SALT_E_BADARG, "augment_preprocess: output too large");
    p.pad_mode = a->pad_mode;
    if (const char* why = salt_pre::pad_mode_error(a->pad_mode, p.top, p.left, p.rh, p.rw, p.H, p.W)) SALT_FAIL(SALT_E_BADARG, "augment_preprocess: %s", why);
    for (int i = 0; i < 3; ++i) {
        if (a->std[i] <= 0.f) SALT_FAIL(SALT_E_BADARG, "augment_preprocess: std must be positive");
        p.mean[i] = a->mean[i]; p.inv_std[i] = 1.f / a->std[i];
    }
    p.cfg = c; p.seed = a->seed; p.counter = a->counter; p.params = a->params; p.params_given = a->params_given;
    p.geo_img = a->geo_img; p.geo_mask = a->geo_mask; p.gray = a->gray;
    return salt_launch(augment_kernel, dim3(a->B), dim3(NT), 0, (hipStream_t)stream, p);
}
