// preprocess_common.h — resize / normalise pieces shared by salt_preprocess (input.hip) and salt_augment_preprocess (augment.hip).
#pragma once
#include "common.h"

namespace salt_pre {

// cv2.BORDER_REFLECT_101 = np.pad(mode='reflect'): the border pixel is not repeated; one reflection (|overhang| <= n - 1)
__device__ __forceinline__ int reflect101(int i, int n) {
    if (n == 1) return 0;
    i = i < 0 ? -i : i;
    return i >= n ? 2 * n - 2 - i : i;
}

// padded output index -> index on the (resized) tile axis of n pixels that starts `before` pixels in: pad_mode 0 edge, 1 reflect-101
__device__ __forceinline__ int pad_index(int out, int before, int n, int pad_mode) {
    const int i = out - before;
    return pad_mode ? reflect101(i, n) : min(max(i, 0), n - 1);
}

// host side of pad_mode: a value that exists, and for reflect-101 a pad of at most n - 1 pixels on every side
static inline const char* pad_mode_error(int pad_mode, int top, int left, int rh, int rw, int H, int W) {
    if (pad_mode != 0 && pad_mode != 1) return "pad_mode must be 0 (edge) or 1 (reflect-101)";
    if (pad_mode == 1 && (top > rh - 1 || H - top - rh > rh - 1 || left > rw - 1 || W - left - rw > rw - 1))
        return "reflect-101 needs a pad of at most n - 1 pixels on every side";
    return nullptr;
}

// cv2.INTER_CUBIC / imgaug 0.2.5 iaa.Scale default: Keys cubic convolution, a = -0.75, taps at floor(s) - 1 .. floor(s) + 2 of the
// half-pixel-centred source coordinate s = (dst + 0.5) * in / out - 0.5, indices clamped to the image (BORDER_REPLICATE)
__device__ __forceinline__ void cubic_w(float t, float (&w)[4]) {
    const float A = -0.75f;
    w[0] = ((A * (t + 1.f) - 5.f * A) * (t + 1.f) + 8.f * A) * (t + 1.f) - 4.f * A;
    w[1] = ((A + 2.f) * t - (A + 3.f)) * t * t + 1.f;
    w[2] = ((A + 2.f) * (1.f - t) - (A + 3.f)) * (1.f - t) * (1.f - t) + 1.f;
    w[3] = 1.f - w[0] - w[1] - w[2];
}

// the same four coefficients, every operation rounded on its own (no FMA contraction): cv2's interpolateCubic in float32
__device__ __forceinline__ void cubic_w_rn(float t, float (&c)[4]) {
    const float A = -0.75f;
    const float x1 = __fadd_rn(t, 1.f);
    c[0] = __fsub_rn(__fmul_rn(__fadd_rn(__fmul_rn(__fsub_rn(__fmul_rn(A, x1), __fmul_rn(5.f, A)), x1), __fmul_rn(8.f, A)), x1), __fmul_rn(4.f, A));
    c[1] = __fadd_rn(__fmul_rn(__fmul_rn(__fsub_rn(__fmul_rn(__fadd_rn(A, 2.f), t), __fadd_rn(A, 3.f)), t), t), 1.f);
    const float u = __fsub_rn(1.f, t);
    c[2] = __fadd_rn(__fmul_rn(__fmul_rn(__fsub_rn(__fmul_rn(__fadd_rn(A, 2.f), u), __fadd_rn(A, 3.f)), u), u), 1.f);
    c[3] = __fsub_rn(__fsub_rn(__fsub_rn(1.f, c[0]), c[1]), c[2]);
}

// cv2.resize(..., INTER_CUBIC) on CV_8U as opencv_python 3.4.0.12 (environment.yml:16) evaluates it (modules/imgproc/src/resize.cpp:
// resizeGeneric_<HResizeCubic<uchar, int, short>, VResizeCubic<uchar, int, short, FixedPtCast<int, uchar, 22>, ...>>), restated:
//   per axis   fx = (float)((d + 0.5) * scale - 0.5) with scale = 1 / ((double)out / in);  s = floor(fx);  t = fx - s   (float)
//              coefficients interpolateCubic(t) in float32 (A = -0.75f, the four expressions below, no FMA contraction), each
//              rounded on its own to a short: cvRound(c * 2048)   (their sum is 2047 .. 2049)
//   horizontal int sums of uchar x short over taps s - 1 .. s + 2 (indices clamped = BORDER_REPLICATE)
//   vertical   int sum of those x short, then saturate_cast<uchar>((v + (1 << 21)) >> 22)
// (the SSE2 build of that release runs the vertical pass of whole 8-pixel groups in float32 with round-to-nearest-even: the same
//  value except where v / 2^22 sits within float rounding of a tie - the integer form is the documented one and is what is restated.)
__device__ __forceinline__ void cubic_coef_fixed(int d, double scale, int& s0, int (&c)[4]) {
    const float fx = (float)(((double)d + 0.5) * scale - 0.5);
    const float sf = floorf(fx);
    const float t = __fsub_rn(fx, sf);
    s0 = (int)sf - 1;
    float cf[4];
    cubic_w_rn(t, cf);
#pragma unroll
    for (int i = 0; i < 4; ++i) c[i] = __float2int_rn(__fmul_rn(cf[i], 2048.f));
}

// the integer sum of the fixed-point cubic over one uint8 plane [h, w] (row stride w); `binarize`: each tap is (v != 0) - the uint8
// {0,1} mask goes through the same resize, binarised first (a 0 / 255 mask must not dilate)
__device__ __forceinline__ int cubic_fixed_acc(const unsigned char* pl, int h, int w, int y0, const int (&cy)[4], int x0, const int (&cx)[4],
                                               bool binarize) {
    int acc = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int yy = min(max(y0 + i, 0), h - 1);
        int row = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int xx = min(max(x0 + j, 0), w - 1);
            const int v = (int)pl[yy * w + xx];
            row += cx[j] * (binarize ? (int)(v != 0) : v);
        }
        acc += cy[i] * row;
    }
    return acc;
}

__device__ __forceinline__ int fixed_to_u8(int acc) { return min(max((acc + (1 << 21)) >> 22, 0), 255); }

// Grayscale(3) + ToTensor + Normalize + AddDepthChannels of one gray value g in [0, 1] at output pixel (Y, X) of image b; the mask
// value m (when target != NULL) -> one-hot {1 - m, m}
__device__ __forceinline__ void store_x_target(float* x, float* target, int b, int Y, int X, int H, int W, int channels,
                                               const float (&mean)[3], const float (&inv_std)[3], float g, float m) {
    const int64_t hw = (int64_t)H * W;
    float* xo = x + (int64_t)b * channels * hw + (int64_t)Y * W + X;
    const float c0 = (g - mean[0]) * inv_std[0];
    xo[0] = c0;
    if (channels == 3) {
        const float depth = H > 1 ? (float)((double)Y / (double)(H - 1)) : 0.f;              // np.linspace(0, 1, H)[Y]
        xo[hw] = depth;
        xo[2 * hw] = c0 * depth;
    }
    if (target) {
        float* to = target + (int64_t)b * 2 * hw + (int64_t)Y * W + X;
        to[0] = 1.f - m;
        to[hw] = m;
    }
}

}  // namespace salt_pre
