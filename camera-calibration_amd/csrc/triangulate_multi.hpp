// N-view triangulation (device code, gfx950): the 3-D point that the pixels of up to kRigMaxCams cameras of a rig see.
// triangulate_kernel (rectify.hpp) for any number of cameras and a per-point mask of the cameras that saw the point: one
// thread per point, no LDS, no atomics, no sums across lanes -- two calls agree bit for bit. The number of cameras and each
// camera's model are run-time, wave-uniform values -- there is one kernel for every rig -- and the cameras are visited in
// index order in one loop that is never unrolled. The kernel's only template argument is its block size: like
// rectify.hpp's kernels it is emitted where it is first launched, at the end of the module, so the module's other
// kernels keep their place and labels.
#pragma once
#include "rectify.hpp"
#include "rig.hpp"

namespace calib {

// One camera of a call: X_c = T.R X + T.t takes the caller's frame into the camera's. The table is a kernel argument:
// every read of it has a wave-uniform index, so it arrives by scalar loads and lives in scalar registers.
struct TriCamera {
    Pinhole cam;
    Rigid T;
    double k[5];                                 // the model's coefficients (fisheye: four)
    int model, pad;
};
struct TriCameras {
    TriCamera c[kRigMaxCams];
    int n, pad;
};

// What the seen cameras add at X, in index order: the squared residuals, N = J^T J (lower triangle: 00 10 11 20 21 22),
// g = J^T r, and whether X lies in front of every seen camera. An unseen camera adds nothing and its pixel is not read.
// res (camera-major, like uv) or null: the residuals themselves.
__device__ __forceinline__ void tri_multi_eval(const TriCameras& cs, uint32_t seen, const double2* __restrict__ uv,
                                               int64_t n, int64_t i, const double (&X)[3], TriEval& e,
                                               double2* __restrict__ res) {
    e.err = 0.0;
#pragma unroll
    for (int j = 0; j < 6; ++j) e.N[j] = 0.0;
#pragma unroll
    for (int j = 0; j < 3; ++j) e.g[j] = 0.0;
    e.front = true;
    __builtin_assume(cs.n >= 2 && cs.n <= kRigMaxCams);
#pragma unroll 1
    for (int c = 0; c < cs.n; ++c) {
        if (!((seen >> c) & 1u)) continue;
        const TriCamera& cm = cs.c[c];
        const double2 m = uv[(int64_t)c * n + i];
        const double Xc = cm.T.R[0] * X[0] + cm.T.R[1] * X[1] + cm.T.R[2] * X[2] + cm.T.t[0];
        const double Yc = cm.T.R[3] * X[0] + cm.T.R[4] * X[1] + cm.T.R[5] * X[2] + cm.T.t[1];
        const double Zc = cm.T.R[6] * X[0] + cm.T.R[7] * X[1] + cm.T.R[8] * X[2] + cm.T.t[2];
        double ru, rv, Ju[3], Jv[3];
        if (cm.model == kRadtan) tri_rows<kRadtan>(cm.cam, cm.k, Xc, Yc, Zc, m, ru, rv, Ju, Jv);
        else tri_rows<kFisheye>(cm.cam, cm.k, Xc, Yc, Zc, m, ru, rv, Ju, Jv);
        double Ku[3], Kv[3];                                                        // d / dX = (d / dX_c) R
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            Ku[q] = Ju[0] * cm.T.R[q] + Ju[1] * cm.T.R[3 + q] + Ju[2] * cm.T.R[6 + q];
            Kv[q] = Jv[0] * cm.T.R[q] + Jv[1] * cm.T.R[3 + q] + Jv[2] * cm.T.R[6 + q];
        }
        e.err = (e.err + ru * ru) + rv * rv;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
#pragma unroll
            for (int b = 0; b <= a; ++b) e.N[a * (a + 1) / 2 + b] = (e.N[a * (a + 1) / 2 + b] + Ku[a] * Ku[b]) + Kv[a] * Kv[b];
            e.g[a] = (e.g[a] + Ku[a] * ru) + Kv[a] * rv;
        }
        e.front = e.front && Zc > 0.0;
        if (res) res[(int64_t)c * n + i] = make_double2(ru, rv);
    }
}

// the ray of camera c's ideal normalised point p in the caller's frame: R^T (x, y, 1)
__device__ __forceinline__ void tri_multi_ray(const TriCamera& cm, double2 p, double (&d)[3]) {
#pragma unroll
    for (int q = 0; q < 3; ++q) d[q] = cm.T.R[q] * p.x + cm.T.R[3 + q] * p.y + cm.T.R[6 + q];
}

// L L^T = the symmetric 3 x 3 matrix A (lower triangle, diagonal d0 d1 d2 given apart); false where a pivot is not
// positive. L = (l00 l10 l11 l20 l21 l22) as the reciprocals i00 i11 i22 of its diagonal and its three other entries.
struct Chol3 { double i00, i11, i22, l10, l20, l21; };
__device__ __forceinline__ bool cholesky3(double d0, double d1, double d2, double a10, double a20, double a21, Chol3& L) {
    const double l00 = sqrt(d0);
    L.i00 = 1.0 / l00;
    L.l10 = a10 * L.i00;
    L.l20 = a20 * L.i00;
    const double p1 = d1 - L.l10 * L.l10;
    const double l11 = sqrt(p1);
    L.i11 = 1.0 / l11;
    L.l21 = (a21 - L.l20 * L.l10) * L.i11;
    const double p2 = d2 - L.l20 * L.l20 - L.l21 * L.l21;
    L.i22 = 1.0 / sqrt(p2);
    return d0 > 0.0 && p1 > 0.0 && p2 > 0.0;
}
__device__ __forceinline__ void solve3(const Chol3& L, const double (&b)[3], double (&x)[3]) {
    const double z0 = b[0] * L.i00, z1 = (b[1] - L.l10 * z0) * L.i11, z2 = (b[2] - L.l20 * z0 - L.l21 * z1) * L.i22;
    x[2] = z2 * L.i22;
    x[1] = (z1 - L.l21 * x[2]) * L.i11;
    x[0] = (z0 - L.l10 * x[1] - L.l20 * x[2]) * L.i00;
}

// uv, xy, status: camera-major (N, n): camera c's pixel of point i, the IDEAL normalised point undistort_points_kernel
// found for it and that kernel's status, at c n + i. seen (n): bit c set where camera c saw point i (bits at or above N
// are the host's to refuse). X (n, 3) in the frame the cameras' T map from; sse (n) or null; status (n) or null;
// cov (n, 6) or null: the lower triangle (00 10 11 20 21 22) of the UNDAMPED (J^T J)^-1 at X, NaN where a pivot is not
// positive; res (N, n) or null: the residuals at X, NaN for an unseen camera.
//   start   the point closest in least squares to the seen rays o_c + s d_c, o_c = -R_c^T t_c, d_c = R_c^T (x_c, y_c, 1):
//           sum_c (I - d_c d_c^T / |d_c|^2) (X - o_c) = 0 by a 3 x 3 Cholesky (two rays: the midpoint of their common
//           perpendicular)
//   refine  triangulate_kernel's loop on the 2 m pixel residuals of the m seen cameras: the same constants, the same
//           accept rule with eta = 2^-44 max(1, |uv|_inf) over the seen pixels, the same leave threshold; a candidate
//           must lie in front of every seen camera
//   status  the first that applies: 4 fewer than two cameras saw the point; 1 a seen pixel is not finite or has no
//           inverse; 2 degenerate geometry: the largest sin^2 of the angle between two seen rays < kTriParallel (two
//           cameras: triangulate_kernel's rule), the start's system not positive definite, the start or the end point
//           behind a seen camera, a damped pivot that is not positive; 3 the last accepted step was still > 1e-9 |X|; 0.
//           X, sse, cov and res are NaN unless it is 0.
// Which of the optional outputs are asked for changes no arithmetic that reaches another output.
template <int THREADS>
__global__ __launch_bounds__(THREADS) void triangulate_multi_kernel(TriCameras cs, int64_t n, const double2* __restrict__ uv,
                                                                const double2* __restrict__ xy,
                                                                const int32_t* __restrict__ inv,
                                                                const uint32_t* __restrict__ seenMask,
                                                                double* __restrict__ outX, double* __restrict__ outSse,
                                                                int32_t* __restrict__ outStatus,
                                                                double* __restrict__ outCov, double2* __restrict__ outRes) {
    const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (i >= n) return;
    __builtin_assume(cs.n >= 2 && cs.n <= kRigMaxCams);                             // the host's check: no loop is empty
    const uint32_t seen = seenMask[i] & ((1u << cs.n) - 1u);
    const bool enough = __builtin_popcount(seen) >= 2;

    // the seen cameras in index order: the inverse's statuses, the largest pixel coordinate, the closest point's system
    bool solved = true;
    double big = 1.0;
    double M[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, b[3] = {0.0, 0.0, 0.0};
    bool apart = false;                                                             // two seen rays are not parallel
#pragma unroll 1
    for (int c = 0; c < cs.n; ++c) {
        if (!((seen >> c) & 1u)) continue;
        const TriCamera& cm = cs.c[c];
        const int64_t at = (int64_t)c * n + i;
        solved = solved && inv[at] == 0;
        const double2 m = uv[at];
        big = fmax(big, fmax(fabs(m.x), fabs(m.y)));
        double d[3], o[3];
        tri_multi_ray(cm, xy[at], d);
#pragma unroll
        for (int q = 0; q < 3; ++q) o[q] = -(cm.T.R[q] * cm.T.t[0] + cm.T.R[3 + q] * cm.T.t[1] + cm.T.R[6 + q] * cm.T.t[2]);
        const double dd = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
        const double idd = 1.0 / dd;
        const double w = (d[0] * o[0] + d[1] * o[1] + d[2] * o[2]) * idd;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
#pragma unroll
            for (int q = 0; q <= a; ++q) M[a * (a + 1) / 2 + q] += (a == q ? 1.0 : 0.0) - d[a] * d[q] * idd;
            b[a] += o[a] - d[a] * w;
        }
        // sin^2 of the angle to every seen ray before this one: aa bb - ab^2 against kTriParallel aa bb
#pragma unroll 1
        for (int c2 = 0; c2 < c; ++c2) {
            if (!((seen >> c2) & 1u)) continue;
            double f[3];
            tri_multi_ray(cs.c[c2], xy[(int64_t)c2 * n + i], f);
            const double ff = f[0] * f[0] + f[1] * f[1] + f[2] * f[2];
            const double fd = f[0] * d[0] + f[1] * d[1] + f[2] * d[2];
            apart = apart || ff * dd - fd * fd >= kTriParallel * (ff * dd);         // false for NaN
        }
    }
    Chol3 L;
    bool geometry = cholesky3(M[0], M[2], M[5], M[1], M[3], M[4], L) && apart;
    double X[3];
    solve3(L, b, X);

    const double eta = kTriPixelUlps * big;
    TriEval cur;
    tri_multi_eval(cs, seen, uv, n, i, X, cur, nullptr);
    geometry = geometry && cur.front;
    int st = !enough ? 4 : !solved ? 1 : !geometry ? 2 : 0;                         // the first rule that applies
    double lam = kTriLambda0, lastAccepted = 0.0;
    bool live = st == 0;
    for (int it = 0; it < kTriMaxIters && live; ++it) {
        // L L^T = N + lam diag N, delta = its inverse applied to g
        if (!cholesky3(cur.N[0] + lam * cur.N[0], cur.N[2] + lam * cur.N[2], cur.N[5] + lam * cur.N[5], cur.N[1], cur.N[3],
                       cur.N[4], L)) { st = 2; break; }
        double dl[3];
        solve3(L, cur.g, dl);
        const double Xn[3] = {X[0] + dl[0], X[1] + dl[1], X[2] + dl[2]};
        TriEval cand;
        tri_multi_eval(cs, seen, uv, n, i, Xn, cand, nullptr);
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
    const double norm = sqrt(X[0] * X[0] + X[1] * X[1] + X[2] * X[2]);
    if (st == 0) st = !cur.front ? 2 : !(lastAccepted <= kTriStepDone * norm) ? 3 : 0;
    const double nan = __builtin_nan("");
    outX[3 * i] = st ? nan : X[0];
    outX[3 * i + 1] = st ? nan : X[1];
    outX[3 * i + 2] = st ? nan : X[2];
    if (outSse) outSse[i] = st ? nan : cur.err;
    if (outStatus) outStatus[i] = st;
    if (outCov) {
        // (L L^T)^-1 = W^T W, W = L^-1 (lower triangular)
        const bool pd = cholesky3(cur.N[0], cur.N[2], cur.N[5], cur.N[1], cur.N[3], cur.N[4], L);
        const double w10 = -L.l10 * L.i00 * L.i11;
        const double w21 = -L.l21 * L.i11 * L.i22;
        const double w20 = -(L.l20 * L.i00 + L.l21 * w10) * L.i22;
        const bool ok = st == 0 && pd;
        double* __restrict__ o = outCov + 6 * i;
        o[0] = ok ? L.i00 * L.i00 + w10 * w10 + w20 * w20 : nan;
        o[1] = ok ? w10 * L.i11 + w20 * w21 : nan;
        o[2] = ok ? L.i11 * L.i11 + w21 * w21 : nan;
        o[3] = ok ? w20 * L.i22 : nan;
        o[4] = ok ? w21 * L.i22 : nan;
        o[5] = ok ? L.i22 * L.i22 : nan;
    }
    if (outRes) {
        const double2 nan2 = make_double2(nan, nan);
#pragma unroll 1
        for (int c = 0; c < cs.n; ++c) outRes[(int64_t)c * n + i] = nan2;            // this lane's entries only
        if (st == 0) {
            TriEval at;
            tri_multi_eval(cs, seen, uv, n, i, X, at, outRes);
        }
    }
}

}  // namespace calib
