// resample64.h — the float64 order-1 interpolant of saltnet.h (BILINEAR64): resize.hip and ensemble.hip evaluate the SAME source text,
// so a resized map and a resized ensemble member are the same bits.
#pragma once
#include "common.h"

namespace {

// ---- float64 source coordinates and the four-tap interpolant: every operation rounded on its own, on the host and on the device
__host__ __device__ inline double src_coord(double scale, int i) {
#pragma clang fp contract(off)
    const double t = (double)i + 0.5;
    const double u = scale * t;
    return u - 0.5;
}
__host__ __device__ inline int floor_int(double v) { const int i = (int)v; return (double)i > v ? i - 1 : i; }

__device__ __forceinline__ double lerp2(double p00, double p01, double p10, double p11, double dr, double dc) {
#pragma clang fp contract(off)
    const double gc = 1.0 - dc, gr = 1.0 - dr;
    const double a = gc * p00, b = dc * p01, c = gc * p10, d = dc * p11;
    const double top = a + b, bot = c + d;
    const double e = gr * top, f = dr * bot;
    return e + f;
}
__device__ __forceinline__ double frac_of(double v, int v0) {
#pragma clang fp contract(off)
    return v - (double)v0;
}

// BILINEAR64 of one contiguous [h, w] fp32 plane, 0 outside
__device__ __forceinline__ double bilinear64(const float* pl, int h, int w, double r, double c) {
    const int r0 = floor_int(r), c0 = floor_int(c);
    auto tap = [&](int y, int x) -> double { return (y >= 0 && y < h && x >= 0 && x < w) ? (double)pl[(int64_t)y * w + x] : 0.0; };
    return lerp2(tap(r0, c0), tap(r0, c0 + 1), tap(r0 + 1, c0), tap(r0 + 1, c0 + 1), frac_of(r, r0), frac_of(c, c0));
}

}  // namespace
