// Using a calibrated rig (device code, gfx950): the map a RECTIFIED image reads from, and the 3-D point two matched
// pixels see. Both are per-element evaluations of the per-point camera model (point_model.hpp) with the helpers of
// undistort.hpp; one thread per output element (the map kernel: four), no LDS, no atomics, no sums across lanes -- two
// calls agree bit for bit. Both kernels are templates: they are emitted where they are first launched, at the end of the
// module, so the module's other kernels keep their place and labels.
#pragma once
#include "undistort.hpp"

namespace calib {

struct Rot3 { double m[9]; };               // row-major rotation, as a kernel argument
struct Rigid { double R[9], t[3]; };        // Xb = R Xa + t

// ---------------------------------------------------------------- the map of a rectified image
// undistort_map_kernel with a rotation between the destination's ray and the source camera: destination pixel
// (col j, row i) of the pinhole image `dst` looks along r = ((j - uc' - ga' y) / al', y = (i - vc') / be', 1) in the
// ROTATED frame; in the camera's own frame that is X = R^T r, which the source image shows at
// cam(distort(X.x / X.z, X.y / X.z)). A ray that does not point into the camera's front half space (X.z <= 0), or whose
// normalised point is not finite, has no pixel: both planes get NaN, which remap turns into `border`. The flat walk,
// the 16-byte stores and the tail rule are undistort_map_kernel's; with R = I the arithmetic reduces to that kernel's
// (x 1 + y 0 + 0 and x / 1 are exact), so the two maps are equal bit for bit.
template <int MODEL>
__global__ __launch_bounds__(256) void rectify_map_kernel(Pinhole cam, Pinhole dst, Rot3 R, const double* __restrict__ k,
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
    const float nanf_ = __builtin_nanf("");
#pragma unroll
    for (int q = 0; q < kMapCols; ++q) {
        const double ry = ((double)i - dst.vc) * ibe;
        const double rx = ((double)j - dst.uc - dst.ga * ry) * ial;
        const double X = R.m[0] * rx + R.m[3] * ry + R.m[6];                  // R^T r
        const double Y = R.m[1] * rx + R.m[4] * ry + R.m[7];
        const double Z = R.m[2] * rx + R.m[5] * ry + R.m[8];
        const double iz = fast_rcp(Z);
        const double x = X * iz, y = Y * iz;
        const bool ok = Z > 0.0 && fabs(x) <= 1.79769313486231571e308 && fabs(y) <= 1.79769313486231571e308;
        double xd, yd, a, b, c;
        distort_jac<MODEL>(kk, x, y, xd, yd, a, b, c);
        sx[q] = ok ? (float)(cam.al * xd + cam.ga * yd + cam.uc) : nanf_;
        sy[q] = ok ? (float)(cam.be * yd + cam.vc) : nanf_;
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

// ---------------------------------------------------------------- triangulation of matched pixels
constexpr int kTriMaxIters = 20;
constexpr double kTriLambda0 = 1e-3;        // the project's LM damping rule: / 10 on accept, * 10 on reject
constexpr double kTriParallel = 1e-12;      // sin^2 of the angle between the rays below which they count as parallel
constexpr double kTriStepLeave = 1e-14;     // a lane leaves the loop at a step <= this * |X|
constexpr double kTriStepDone = 1e-9;       // status 3: the last accepted step was still larger than this * |X|
constexpr double kTriPixelUlps = 0x1p-44;   // a projected pixel is trusted to 256 ulp of the largest pixel coordinate

// One camera's two rows at the point (X, Y, Z) of ITS frame: residual uv - cam(distort(X / Z, Y / Z)) and the rows
// d(u, v) / d(X, Y, Z) = A2x2 [[a, b], [b, c]] d(x, y)/d(X, Y, Z), [[a, b], [b, c]] the model's own symmetric derivative.
template <int MODEL>
__device__ __forceinline__ void tri_rows(const Pinhole& cam, const double* __restrict__ kk, double X, double Y, double Z,
                                         double2 uv, double& ru, double& rv, double (&Ju)[3], double (&Jv)[3]) {
    const double iz = fast_rcp(Z);
    const double x = X * iz, y = Y * iz;
    double xd, yd, a, b, c;
    distort_jac<MODEL>(kk, x, y, xd, yd, a, b, c);
    ru = uv.x - (cam.al * xd + cam.ga * yd + cam.uc);
    rv = uv.y - (cam.be * yd + cam.vc);
    const double ux = (cam.al * a + cam.ga * b) * iz, uy = (cam.al * b + cam.ga * c) * iz;
    const double vx = cam.be * b * iz, vy = cam.be * c * iz;
    Ju[0] = ux; Ju[1] = uy; Ju[2] = -(ux * x + uy * y);
    Jv[0] = vx; Jv[1] = vy; Jv[2] = -(vx * x + vy * y);
}

// The four residuals at X (camera a's frame): their squared sum, N = J^T J (lower triangle: 00 10 11 20 21 22),
// g = J^T r, and whether X lies in front of both cameras.
struct TriEval { double err, N[6], g[3]; bool front; };

template <int MODEL_A, int MODEL_B>
__device__ __forceinline__ void tri_eval(const Pinhole& ca, const double* __restrict__ ka, const Pinhole& cb,
                                         const double* __restrict__ kb, const Rigid& rig, const double (&X)[3],
                                         double2 uva, double2 uvb, TriEval& e) {
    double r[4], J[4][3], Ju[3], Jv[3];
    tri_rows<MODEL_A>(ca, ka, X[0], X[1], X[2], uva, r[0], r[1], J[0], J[1]);
    const double Xb = rig.R[0] * X[0] + rig.R[1] * X[1] + rig.R[2] * X[2] + rig.t[0];
    const double Yb = rig.R[3] * X[0] + rig.R[4] * X[1] + rig.R[5] * X[2] + rig.t[1];
    const double Zb = rig.R[6] * X[0] + rig.R[7] * X[1] + rig.R[8] * X[2] + rig.t[2];
    tri_rows<MODEL_B>(cb, kb, Xb, Yb, Zb, uvb, r[2], r[3], Ju, Jv);
#pragma unroll
    for (int m = 0; m < 3; ++m) {                                               // d / dXa = (d / dXb) R
        J[2][m] = Ju[0] * rig.R[m] + Ju[1] * rig.R[3 + m] + Ju[2] * rig.R[6 + m];
        J[3][m] = Jv[0] * rig.R[m] + Jv[1] * rig.R[3 + m] + Jv[2] * rig.R[6 + m];
    }
    e.err = ((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]) + r[3] * r[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int b = 0; b <= a; ++b)
            e.N[a * (a + 1) / 2 + b] = ((J[0][a] * J[0][b] + J[1][a] * J[1][b]) + J[2][a] * J[2][b]) + J[3][a] * J[3][b];
        e.g[a] = ((J[0][a] * r[0] + J[1][a] * r[1]) + J[2][a] * r[2]) + J[3][a] * r[3];
    }
    e.front = X[2] > 0.0 && Zb > 0.0;
}

// xa, xb (n): the IDEAL normalised points of the two pixels (undistort_points_kernel's output, NaN where its status is 1)
// with their statuses sa, sb; uva, uvb (n): the pixels themselves. X (n, 3) in camera a's frame, sse (n) or null: the
// four residuals squared and summed at X, status (n) or null.
//   start   the midpoint of the common perpendicular of the rays s da and c + u R^T db, c = -R^T t (a 2 x 2 solve)
//   refine  at most kTriMaxIters steps delta = (N + lambda diag N)^-1 g on the four PIXEL residuals through each camera's
//           full forward model; lambda from 1e-3, / 10 when the step is accepted, * 10 when not. A step is accepted when
//           it lowers the error. The error is a sum of squares of ROUNDED pixels: with eta = 2^-44 max(1, |uv|_inf) the
//           trust in a projected pixel, two errors closer than flat = eta (2 sqrt(err) + eta) cannot be told apart. A
//           step whose PREDICTED decrease delta . g is below flat is judged at that resolution instead (accepted unless
//           the error grows by more than flat) -- without this the last Newton step, the one that takes the gradient
//           from 1e-7 of its scale to rounding, is a coin toss, and a pair whose pixels happen to agree to 1e-4 px never
//           sees a step accepted again once its error is below 1e-7. A candidate behind a camera is rejected. A lane
//           leaves the loop at a step <= 1e-14 |X|.
//   status  0 ok; 1 a pixel without an inverse in either camera (or not finite); 2 degenerate geometry: rays parallel
//           (sin^2 < 1e-12), the start or the end point behind a camera, N + lambda diag N not positive definite;
//           3 the last accepted step was still > 1e-9 |X|. Decided after the loop; X and sse are NaN unless it is 0.
template <int MODEL_A, int MODEL_B>
__global__ __launch_bounds__(256) void triangulate_kernel(Pinhole ca, const double* __restrict__ ka, Pinhole cb,
                                                          const double* __restrict__ kb, Rigid rig, int64_t n,
                                                          const double2* __restrict__ xa, const int32_t* __restrict__ sa,
                                                          const double2* __restrict__ xb, const int32_t* __restrict__ sb,
                                                          const double2* __restrict__ uva, const double2* __restrict__ uvb,
                                                          double* __restrict__ outX, double* __restrict__ outSse,
                                                          int32_t* __restrict__ outStatus) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    constexpr int NA = ModelTraits<MODEL_A>::NK, NB = ModelTraits<MODEL_B>::NK;
    double kka[NA], kkb[NB];
#pragma unroll
    for (int j = 0; j < NA; ++j) kka[j] = ka[j];
#pragma unroll
    for (int j = 0; j < NB; ++j) kkb[j] = kb[j];
    const bool solved = sa[i] == 0 && sb[i] == 0;
    const double2 pa = xa[i], pb = xb[i], ma = uva[i], mb = uvb[i];

    // the midpoint of the common perpendicular
    const double da[3] = {pa.x, pa.y, 1.0};
    double db[3], cc[3];
#pragma unroll
    for (int m = 0; m < 3; ++m) {
        db[m] = rig.R[m] * pb.x + rig.R[3 + m] * pb.y + rig.R[6 + m];           // R^T (xb, yb, 1)
        cc[m] = -(rig.R[m] * rig.t[0] + rig.R[3 + m] * rig.t[1] + rig.R[6 + m] * rig.t[2]);
    }
    const double aa = da[0] * da[0] + da[1] * da[1] + da[2] * da[2];
    const double bb = db[0] * db[0] + db[1] * db[1] + db[2] * db[2];
    const double ab = da[0] * db[0] + da[1] * db[1] + da[2] * db[2];
    const double ac = da[0] * cc[0] + da[1] * cc[1] + da[2] * cc[2];
    const double bc = db[0] * cc[0] + db[1] * cc[1] + db[2] * cc[2];
    const double det = aa * bb - ab * ab;
    bool geometry = det >= kTriParallel * (aa * bb);                            // false for NaN
    const double idet = 1.0 / det;
    const double s = (ac * bb - ab * bc) * idet, u = (ab * ac - aa * bc) * idet;
    double X[3];
#pragma unroll
    for (int m = 0; m < 3; ++m) X[m] = 0.5 * (s * da[m] + (cc[m] + u * db[m]));

    const double eta = kTriPixelUlps * fmax(fmax(1.0, fmax(fabs(ma.x), fabs(ma.y))), fmax(fabs(mb.x), fabs(mb.y)));
    TriEval cur;
    tri_eval<MODEL_A, MODEL_B>(ca, kka, cb, kkb, rig, X, ma, mb, cur);
    geometry = geometry && cur.front;
    double lam = kTriLambda0, lastAccepted = 0.0;
    bool live = solved && geometry;
    for (int it = 0; it < kTriMaxIters && live; ++it) {
        // L L^T = N + lam diag N, delta = its inverse applied to g
        const double d0 = cur.N[0] + lam * cur.N[0], d1 = cur.N[2] + lam * cur.N[2], d2 = cur.N[5] + lam * cur.N[5];
        const double l00 = sqrt(d0), i00 = 1.0 / l00;
        const double l10 = cur.N[1] * i00, l20 = cur.N[3] * i00;
        const double p1 = d1 - l10 * l10;
        const double l11 = sqrt(p1), i11 = 1.0 / l11;
        const double l21 = (cur.N[4] - l20 * l10) * i11;
        const double p2 = d2 - l20 * l20 - l21 * l21;
        if (!(d0 > 0.0 && p1 > 0.0 && p2 > 0.0)) { geometry = false; break; }
        const double i22 = 1.0 / sqrt(p2);
        const double z0 = cur.g[0] * i00, z1 = (cur.g[1] - l10 * z0) * i11, z2 = (cur.g[2] - l20 * z0 - l21 * z1) * i22;
        double dl[3];
        dl[2] = z2 * i22;
        dl[1] = (z1 - l21 * dl[2]) * i11;
        dl[0] = (z0 - l10 * dl[1] - l20 * dl[2]) * i00;
        const double Xn[3] = {X[0] + dl[0], X[1] + dl[1], X[2] + dl[2]};
        TriEval cand;
        tri_eval<MODEL_A, MODEL_B>(ca, kka, cb, kkb, rig, Xn, ma, mb, cand);
        const double pred = dl[0] * cur.g[0] + dl[1] * cur.g[1] + dl[2] * cur.g[2];
        const double flat = eta * (2.0 * sqrt(cur.err) + eta);
        const bool accept = cand.front && (cand.err < cur.err || (pred <= flat && cand.err <= cur.err + flat));
        const double step = sqrt(dl[0] * dl[0] + dl[1] * dl[1] + dl[2] * dl[2]);
        if (accept) {
            X[0] = Xn[0]; X[1] = Xn[1]; X[2] = Xn[2];
            cur = cand;
            lastAccepted = step;
            lam *= 0.1;
        } else {
            lam *= 10.0;
        }
        live = !(step <= kTriStepLeave * sqrt(X[0] * X[0] + X[1] * X[1] + X[2] * X[2]));
    }
    geometry = geometry && cur.front;
    const double norm = sqrt(X[0] * X[0] + X[1] * X[1] + X[2] * X[2]);
    const int st = !solved ? 1 : !geometry ? 2 : !(lastAccepted <= kTriStepDone * norm) ? 3 : 0;
    const double nan = __builtin_nan("");
    outX[3 * i] = st ? nan : X[0];
    outX[3 * i + 1] = st ? nan : X[1];
    outX[3 * i + 2] = st ? nan : X[2];
    if (outSse) outSse[i] = st ? nan : cur.err;
    if (outStatus) outStatus[i] = st;
}

}  // namespace calib
