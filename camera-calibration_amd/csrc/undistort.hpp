// Undistortion (device code, gfx950): the inverse of the per-point distortion model, the map an undistorted image
// reads from, and the bilinear resampling through such a map. Everything the LM kernels do with the model runs it
// forward; these three kernels are what applies a finished calibration to pixels. One thread per output element, no
// LDS, no atomics; the model and its 2 x 2 derivative come from point_model.hpp (distort<MODEL, double>).
#pragma once
#include "point_model.hpp"

#include <stdint.h>

namespace calib {

// A = [[al, ga, uc], [0, be, vc], [0, 0, 1]] as a kernel argument
struct Pinhole { double al, be, ga, uc, vc; };

constexpr int kUndistortMaxIters = 30;                  // Newton iterations of the inverse, at most
constexpr double kUlp = 2.220446049250313e-16;          // 2^-52
constexpr double kStepUlps = 4.0, kResidualUlps = 64.0; // stop rule / acceptance bar of the inverse (calib_lm.h)

template <int MODEL>
__device__ __forceinline__ void distort_jac(const double* __restrict__ k, double x, double y,
                                            double& xd, double& yd, double& a, double& b, double& c) {
    double dkx[ModelTraits<MODEL>::NK], dky[ModelTraits<MODEL>::NK];
    distort<MODEL, double>(k, x, y, xd, yd, a, b, c, dkx, dky);
}

// ---------------------------------------------------------------- inverse of the model, N points
// in (n): distorted NORMALISED points (the host entry has taken the pixels through A^-1); out (n): the ideal
// normalised points, status (n): 0 = solved, 1 = no solution on the principal branch (out is NaN).
//   radtan   Newton on distort(x, y) = (xd, yd) from (xd, yd); the Jacobian [[a, b], [b, c]] is symmetric, the 2 x 2
//            system is solved in closed form.
//   fisheye  the model is radial: 1-D Newton on theta (1 + k1 theta^2 + .. + k4 theta^8) = theta_d = |(xd, yd)| from
//            theta = theta_d, then (x, y) = (xd, yd) tan(theta) / theta_d; (x, y) = (xd, yd) below theta_d = 1e-8, the
//            limit the forward model takes at r -> 0.
// The loop is bounded: at most kUndistortMaxIters iterations, a lane whose step has fallen to 4 ulp of max(1, |x|)
// leaves it. Whether a point is SOLVED is decided afterwards and by the forward model alone: the residual
// |distort(x) - (xd, yd)|_inf is at most 64 ulp of max(1, |(xd, yd)|_inf) and the model preserves orientation at x
// (radtan: J positive definite; fisheye: d theta_d / d theta > 0 and 0 <= theta < pi / 2). A target without a
// preimage, a root on a folded-over branch and a non-finite input all fail one of the two (every comparison with a NaN
// is false) and come out as status 1 / NaN.
template <int MODEL>
__global__ __launch_bounds__(256) void undistort_points_kernel(const double2* __restrict__ in, const double* __restrict__ k,
                                                               int64_t n, double2* __restrict__ out,
                                                               int32_t* __restrict__ status) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    constexpr int NK = ModelTraits<MODEL>::NK;
    double kk[NK];
#pragma unroll
    for (int j = 0; j < NK; ++j) kk[j] = k[j];
    const double2 target = in[i];
    const double xd = target.x, yd = target.y;
    double x = xd, y = yd;
    bool branch;                                        // the model preserves orientation at (x, y)
    if constexpr (MODEL == kRadtan) {
        bool done = false;
        for (int it = 0; it < kUndistortMaxIters && !done; ++it) {
            double fx, fy, a, b, c;
            distort_jac<MODEL>(kk, x, y, fx, fy, a, b, c);
            const double rx = fx - xd, ry = fy - yd;
            const double idet = 1.0 / (a * c - b * b);
            const double dx = (c * rx - b * ry) * idet, dy = (a * ry - b * rx) * idet;
            x -= dx;
            y -= dy;
            done = fmax(fabs(dx), fabs(dy)) <= kStepUlps * kUlp * fmax(1.0, fmax(fabs(x), fabs(y)));
        }
        branch = true;                                  // read off the Jacobian of the final evaluation below
    } else {
        const double k1 = kk[0], k2 = kk[1], k3 = kk[2], k4 = kk[3];
        const double td = sqrt(xd * xd + yd * yd);
        if (td < 1e-8) {
            branch = true;                              // (x, y) = (xd, yd)
        } else {
            double th = td;
            bool done = false;
            for (int it = 0; it < kUndistortMaxIters && !done; ++it) {
                const double t2 = th * th;
                const double poly = 1.0 + t2 * (k1 + t2 * (k2 + t2 * (k3 + t2 * k4)));
                const double dpoly = 1.0 + t2 * (3.0 * k1 + t2 * (5.0 * k2 + t2 * (7.0 * k3 + t2 * 9.0 * k4)));
                const double step = (th * poly - td) / dpoly;
                th -= step;
                done = fabs(step) <= kStepUlps * kUlp * fmax(1.0, fabs(th));
            }
            const double t2 = th * th;
            const double dpoly = 1.0 + t2 * (3.0 * k1 + t2 * (5.0 * k2 + t2 * (7.0 * k3 + t2 * 9.0 * k4)));
            branch = dpoly > 0.0 && th >= 0.0 && th < 1.5707963267948966;
            const double sc = branch ? tan(th) / td : __builtin_nan("");
            x = xd * sc;
            y = yd * sc;
        }
    }
    double fx, fy, a, b, c;
    distort_jac<MODEL>(kk, x, y, fx, fy, a, b, c);
    if constexpr (MODEL == kRadtan) branch = a > 0.0 && a * c - b * b > 0.0;
    const double res = fmax(fabs(fx - xd), fabs(fy - yd));
    const bool ok = branch && res <= kResidualUlps * kUlp * fmax(1.0, fmax(fabs(xd), fabs(yd)));
    const double nan = __builtin_nan("");
    out[i] = ok ? make_double2(x, y) : make_double2(nan, nan);
    status[i] = ok ? 0 : 1;
}

// ---------------------------------------------------------------- the map of an undistorted image
// Destination pixel (col j, row i) of a pinhole image with matrix `dst` looks along the ray y = (i - vc') / be',
// x = (j - uc' - ga' y) / al'; the source image shows that ray at cam(distort(x, y)). fp64 throughout, stored as two
// fp32 planes (h, w), rounded to nearest. The planes are walked as ONE flat array of h w floats: a thread owns
// kMapCols consecutive elements -- a 16-byte store per plane, aligned whatever w is -- and steps (j, i) across the row
// ends itself (one integer division per thread). Only the last thread of the array can hold fewer than kMapCols
// elements; it stores them one by one. Writes 8 B per pixel and reads nothing of size.
constexpr int kMapCols = 4;
template <int MODEL>
__global__ __launch_bounds__(256) void undistort_map_kernel(Pinhole cam, Pinhole dst, const double* __restrict__ k,
                                                            unsigned w, unsigned total /* h w < 2^31 */,
                                                            float* __restrict__ mapx, float* __restrict__ mapy) {
    const unsigned base = (blockIdx.x * 256u + threadIdx.x) * (unsigned)kMapCols;
    if (base >= total) return;
    constexpr int NK = ModelTraits<MODEL>::NK;
    double kk[NK];
#pragma unroll
    for (int j = 0; j < NK; ++j) kk[j] = k[j];
    const double ial = fast_rcp(dst.al), ibe = fast_rcp(dst.be);
    unsigned i = base / w, j = base - i * w;
    float sx[kMapCols], sy[kMapCols];
#pragma unroll
    for (int q = 0; q < kMapCols; ++q) {
        const double y = ((double)i - dst.vc) * ibe;
        const double x = ((double)j - dst.uc - dst.ga * y) * ial;
        double xd, yd, a, b, c;
        distort_jac<MODEL>(kk, x, y, xd, yd, a, b, c);
        sx[q] = (float)(cam.al * xd + cam.ga * yd + cam.uc);
        sy[q] = (float)(cam.be * yd + cam.vc);
        if (++j == w) { j = 0; ++i; }
    }
    if (total - base >= (unsigned)kMapCols) {
        *reinterpret_cast<float4*>(mapx + base) = make_float4(sx[0], sx[1], sx[2], sx[3]);
        *reinterpret_cast<float4*>(mapy + base) = make_float4(sy[0], sy[1], sy[2], sy[3]);
    } else {
#pragma unroll
        for (int q = 0; q < kMapCols; ++q)
            if (base + (unsigned)q < total) { mapx[base + q] = sx[q]; mapy[base + q] = sy[q]; }
    }
}

// ---------------------------------------------------------------- bilinear resampling through a map
// dst(row, col, :) = the source (H, W, C interleaved) at (sx, sy) = (mapx, mapy)(row, col), in fp32:
//   x0 = floor(sx), fx = sx - x0 (exact in fp32), likewise y;  taps a (y0, x0), b (y0, x0 + 1), c (y0 + 1, x0), d
//   top = a + fx (b - a),  bot = c + fx (d - c),  out = top + fy (bot - top)      (each a fused multiply-add)
// A tap outside the source is the constant `border` -- the other taps of the pixel still count -- and a map entry that
// is NaN or infinite gives `border`. Every tap is bounds-checked on its own, so no map value can make a load leave the
// source. uint8 output is rint (ties to even) saturated to [0, 255]; float output is the fp32 value.
// Block (64, 4): a wave is 64 consecutive columns of one row, so the map loads and the output stores coalesce; the
// four-tap gather is not coalesced but neighbouring pixels share taps, which the L2 serves.
template <typename T> __device__ __forceinline__ T pixel_from_float(float v);
template <> __device__ __forceinline__ float pixel_from_float<float>(float v) { return v; }
template <> __device__ __forceinline__ uint8_t pixel_from_float<uint8_t>(float v) {
    return (uint8_t)rintf(fminf(fmaxf(v, 0.0f), 255.0f));
}

// one pixel's C channels, as one load / store where C elements are a power-of-two number of bytes
template <typename T, int C>
__device__ __forceinline__ void load_pixel(const T* __restrict__ p, float (&v)[C]) {
    if constexpr (C == 4 && sizeof(T) == 4) {
        const float4 t = *reinterpret_cast<const float4*>(p);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else if constexpr (C == 4) {
        const uchar4 t = *reinterpret_cast<const uchar4*>(p);
        v[0] = (float)t.x; v[1] = (float)t.y; v[2] = (float)t.z; v[3] = (float)t.w;
    } else if constexpr (C == 2 && sizeof(T) == 4) {
        const float2 t = *reinterpret_cast<const float2*>(p);
        v[0] = t.x; v[1] = t.y;
    } else if constexpr (C == 2) {
        const uchar2 t = *reinterpret_cast<const uchar2*>(p);
        v[0] = (float)t.x; v[1] = (float)t.y;
    } else {
#pragma unroll
        for (int ch = 0; ch < C; ++ch) v[ch] = (float)p[ch];
    }
}

template <typename T, int C>
__device__ __forceinline__ void store_pixel(T* __restrict__ p, const float (&v)[C]) {
    if constexpr (C == 4 && sizeof(T) == 4) {
        *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    } else if constexpr (C == 4) {
        *reinterpret_cast<uchar4*>(p) = make_uchar4(pixel_from_float<uint8_t>(v[0]), pixel_from_float<uint8_t>(v[1]),
                                                    pixel_from_float<uint8_t>(v[2]), pixel_from_float<uint8_t>(v[3]));
    } else if constexpr (C == 2 && sizeof(T) == 4) {
        *reinterpret_cast<float2*>(p) = make_float2(v[0], v[1]);
    } else if constexpr (C == 2) {
        *reinterpret_cast<uchar2*>(p) = make_uchar2(pixel_from_float<uint8_t>(v[0]), pixel_from_float<uint8_t>(v[1]));
    } else {
#pragma unroll
        for (int ch = 0; ch < C; ++ch) p[ch] = pixel_from_float<T>(v[ch]);
    }
}

constexpr int kRemapRows = 4;       // rows (waves) of a block
template <typename T, int C>
__global__ __launch_bounds__(64 * kRemapRows) void remap_kernel(const T* __restrict__ src, int H, int W,
                                                                const float* __restrict__ mapx,
                                                                const float* __restrict__ mapy, int h, int w,
                                                                float border, T* __restrict__ dst) {
    const int col = (int)blockIdx.y * 64 + (int)threadIdx.x;
    const int64_t row = (int64_t)blockIdx.x * kRemapRows + threadIdx.y;
    if (col >= w || row >= h) return;
    const int64_t p = row * w + col;
    const float sx = mapx[p], sy = mapy[p];
    float v[C];
#pragma unroll
    for (int ch = 0; ch < C; ++ch) v[ch] = border;
    // outside (-1, W) x (-1, H) all four taps are border (and the interpolation of four equal values is that value);
    // NaN fails the comparisons, and inside the range the conversions to int below cannot overflow
    if (sx > -1.0f && sx < (float)W && sy > -1.0f && sy < (float)H) {
        const float x0f = floorf(sx), y0f = floorf(sy);
        const float fx = sx - x0f, fy = sy - y0f;
        const int x0 = (int)x0f, y0 = (int)y0f;
        const bool xl = x0 >= 0 && x0 < W, xr = x0 + 1 >= 0 && x0 + 1 < W;
        const bool yt = y0 >= 0 && y0 < H, yb = y0 + 1 >= 0 && y0 + 1 < H;
        const int64_t rowStride = (int64_t)W * C;
        const int64_t at = ((int64_t)y0 * W + x0) * C;      // element offset of tap a (negative where it is outside)
        float a[C], b[C], c[C], d[C];
#pragma unroll
        for (int ch = 0; ch < C; ++ch) a[ch] = b[ch] = c[ch] = d[ch] = border;
        if (yt && xl) load_pixel<T, C>(src + at, a);
        if (yt && xr) load_pixel<T, C>(src + at + C, b);
        if (yb && xl) load_pixel<T, C>(src + at + rowStride, c);
        if (yb && xr) load_pixel<T, C>(src + at + rowStride + C, d);
#pragma unroll
        for (int ch = 0; ch < C; ++ch) {
            const float top = __builtin_fmaf(fx, b[ch] - a[ch], a[ch]);
            const float bot = __builtin_fmaf(fx, d[ch] - c[ch], c[ch]);
            v[ch] = __builtin_fmaf(fy, bot - top, top);
        }
    }
    store_pixel<T, C>(dst + p * C, v);
}

}  // namespace calib
