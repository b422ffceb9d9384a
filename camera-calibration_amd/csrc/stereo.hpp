// Stereo calibration with both cameras known: the rig transform between two calibrated cameras (device code, gfx950).
//
// Unknowns Ps = (rig[6], pose_0[6], .., pose_{M-1}[6]), every 6-tuple Euler angles in DEGREES then t, the convention of
// the view blocks of P (pose_view_constants). pose_i takes board points into camera a's frame, Xa = R_i X + t_i; the
// rig takes camera a's frame into camera b's, Xb = R_rig Xa + t_rig. Residuals uv_a - project_a(Xa) and
// uv_b - project_b(Xb). The normal equations have the block-arrow shape of the mono problem with the rig in the place
// of the shared parameters: B (6x6, rig), E_i (rig x view), V_i (6x6, view).
//
// The Jacobian is jacobian_point twice. A camera-a row: the six view columns of jacobian_point<MODEL_A> at (pose_i, X).
// A camera-b row: jacobian_point<MODEL_B> at (rig, Xa) -- Xa as the model point, the rig as the pose -- gives d(uv)/d(rig)
// in its six view columns, whose translation columns are G = d(uv)/dXb; the view columns are G R_rig [dXa/drho_i | I].
//
// One LM round (src/calibrate.py:143-171) is five launches, all fixed-order sums, no floating-point atomics:
//   stereo_blocks_kernel   per view (16 lanes), at the CANDIDATE: V_i, E_i, B_i, g and the view's errors -> record;
//                          B_i, g_rig and the two errors summed over the workgroup's 16 views -> one partial
//   stereo_decide_kernel   one workgroup: the partials in one fixed order, then accept / lambda / stop (round 0: bootstrap)
//   stereo_schur_kernel    per view (16 lanes), blocks of the ACCEPTED point: Cholesky of V_i + lam diag V_i, lane c < 6
//                          row c of E_i V_i^-1 E_i^T and of E_i V_i^-1 g_i; summed over the workgroup -> one partial
//   stereo_rig_kernel      one workgroup: the partials in one fixed order, S = B + lam diag B - sum, Cholesky, delta_rig
//   stereo_backsub_kernel  one lane per view: delta_i = (V_i + lam diag V_i)^-1 (g_i - E_i^T delta_rig), next candidate
//                          (stereo_loop.hpp's, on this file's record with S = 6)
// The state, the decision, the end of the loop and the sum of the partials are stereo_loop.hpp's, shared with the joint
// solver. All kernels are templates (those that need no model take the width they sum or launch with): a template is
// emitted where it is first launched, at the end of the module, so the module's other kernels keep their place and labels.
#pragma once
#include "stereo_loop.hpp"

namespace calib {

// per-view record (doubles): V lower triangle, E row-major (rig row, view column), B_i lower triangle, g_rig, g_view, errors
constexpr int kStV = 0, kStE = 21, kStB = 57, kStGr = 78, kStGv = 84, kStErr = 90, kStAcc = 92;
constexpr int kStRecord = 96;
constexpr int kStTot = 29;            // what is summed over the views at once: B (21), g_rig (6), sse_a, sse_b = record [kStB, kStAcc) minus g_view
constexpr int kStSchur = 43;          // rows c < 6 of (E V^-1 E^T | E V^-1 g) (42), number of failed views

// the record as stereo_backsub_kernel reads it
struct StereoRecord {
    static constexpr int kV = kStV, kE = kStE, kGv = kStGv, kStride = kStRecord;
};

// slot of record entry j in [kStB, kStAcc) among the kStTot summed ones, or -1 (g_view is per view)
__device__ __forceinline__ constexpr int stTotSlot(int j) {
    return j < kStB ? -1 : j < kStGv ? j - kStB : j < kStErr ? -1 : j - kStErr + 27;
}

template <int MODEL_A, int MODEL_B>
__global__ __launch_bounds__(256) void stereo_blocks_kernel(StereoCam ca, const double* shared_a, StereoCam cb,
                                                            const double* shared_b, StereoBufs bf) {
    constexpr int LA = ModelTraits<MODEL_A>::L, CA = ModelTraits<MODEL_A>::C;
    constexpr int LB = ModelTraits<MODEL_B>::L, CB = ModelTraits<MODEL_B>::C;
    __shared__ double sh[16][kStTot];
    if (bf.st->done) return;
    const int cand = bf.st->cur ^ 1;
    const double* __restrict__ Ps = bf.P[cand];
    const int tid = threadIdx.x, i = tid & 15, grp = tid >> 4;
    const int64_t view = (int64_t)blockIdx.x * 16 + grp;
    double acc[kStAcc];
#pragma unroll
    for (int j = 0; j < kStAcc; ++j) acc[j] = 0.0;
    if (view < bf.M) {                         // whole 16-lane group together
        double e[6], rg[6], vc[kViewStride], vr[kViewStride];
#pragma unroll
        for (int j = 0; j < 6; ++j) { rg[j] = Ps[j]; e[j] = Ps[6 + 6 * view + j]; }
        pose_view_constants(e, vc);
        pose_view_constants(rg, vr);
        {
            Shared<MODEL_A, double> sp;
            sp.load(shared_a);
            const int64_t p0 = ca.offs[view];
            const int n = (int)(ca.offs[view + 1] - p0);
            for (int q = i; q < n; q += 16) {
                const double2 m = ca.uv[p0 + q];
                const double* X = ca.xyz + 3 * (p0 + q);
                double u, v;
                double2 J[CA];
                jacobian_point<MODEL_A, double>(sp, vc, X[0], X[1], X[2], u, v, J);
                const double ru = m.x - u, rv = m.y - v;
#pragma unroll
                for (int a = 0; a < 6; ++a) {
#pragma unroll
                    for (int b = 0; b <= a; ++b) acc[kStV + tri(a, b)] += J[LA + a].x * J[LA + b].x + J[LA + a].y * J[LA + b].y;
                    acc[kStGv + a] += J[LA + a].x * ru + J[LA + a].y * rv;
                }
                acc[kStErr] += ru * ru + rv * rv;
            }
        }
        {
            Shared<MODEL_B, double> sp;
            sp.load(shared_b);
            const int64_t p0 = cb.offs[view];
            const int n = (int)(cb.offs[view + 1] - p0);
            for (int q = i; q < n; q += 16) {
                const double2 m = cb.uv[p0 + q];
                const double* X = cb.xyz + 3 * (p0 + q);
                const double q0 = vc[0] * X[0] + vc[1] * X[1] + vc[2] * X[2];       // R_i X
                const double q1 = vc[3] * X[0] + vc[4] * X[1] + vc[5] * X[2];
                const double q2 = vc[6] * X[0] + vc[7] * X[1] + vc[8] * X[2];
                double u, v;
                double2 J[CB];
                jacobian_point<MODEL_B, double>(sp, vr, q0 + vc[9], q1 + vc[10], q2 + vc[11], u, v, J);
                const double ru = m.x - u, rv = m.y - v;
                // G R_rig (2 x 3), G = d(uv)/dXb = the translation columns
                double2 GR[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    GR[k].x = J[LB + 3].x * vr[k] + J[LB + 4].x * vr[3 + k] + J[LB + 5].x * vr[6 + k];
                    GR[k].y = J[LB + 3].y * vr[k] + J[LB + 4].y * vr[3 + k] + J[LB + 5].y * vr[6 + k];
                }
                // dXa/drho_i = (pi/180) a. x q (jacobian_stage_b), dXa/dt_i = I
                const double ax0 = vc[12], ax1 = vc[13], ax2 = vc[14], ay0 = vc[15], ay1 = vc[16];
                const double deg = 0.017453292519943295;
                const double dx[3] = {ax1 * q2 - ax2 * q1, ax2 * q0 - ax0 * q2, ax0 * q1 - ax1 * q0};
                const double dy[3] = {ay1 * q2, -ay0 * q2, ay0 * q1 - ay1 * q0};
                const double dz[3] = {-deg * q1, deg * q0, 0.0};
                double2 Jv[6];
                Jv[0].x = GR[0].x * dx[0] + GR[1].x * dx[1] + GR[2].x * dx[2];
                Jv[0].y = GR[0].y * dx[0] + GR[1].y * dx[1] + GR[2].y * dx[2];
                Jv[1].x = GR[0].x * dy[0] + GR[1].x * dy[1] + GR[2].x * dy[2];
                Jv[1].y = GR[0].y * dy[0] + GR[1].y * dy[1] + GR[2].y * dy[2];
                Jv[2].x = GR[0].x * dz[0] + GR[1].x * dz[1];
                Jv[2].y = GR[0].y * dz[0] + GR[1].y * dz[1];
                Jv[3] = GR[0]; Jv[4] = GR[1]; Jv[5] = GR[2];
#pragma unroll
                for (int a = 0; a < 6; ++a) {
                    const double2 Jr = J[LB + a];
#pragma unroll
                    for (int b = 0; b <= a; ++b) {
                        acc[kStV + tri(a, b)] += Jv[a].x * Jv[b].x + Jv[a].y * Jv[b].y;
                        acc[kStB + tri(a, b)] += Jr.x * J[LB + b].x + Jr.y * J[LB + b].y;
                    }
#pragma unroll
                    for (int b = 0; b < 6; ++b) acc[kStE + a * 6 + b] += Jr.x * Jv[b].x + Jr.y * Jv[b].y;
                    acc[kStGr + a] += Jr.x * ru + Jr.y * rv;
                    acc[kStGv + a] += Jv[a].x * ru + Jv[a].y * rv;
                }
                acc[kStErr + 1] += ru * ru + rv * rv;
            }
        }
#pragma unroll
        for (int j = 0; j < kStAcc; ++j) acc[j] = group_sum16(acc[j]);
        double* __restrict__ rec = bf.rec[cand] + view * kStRecord;
#pragma unroll
        for (int j = 0; j < kStAcc; ++j)
            if ((j & 15) == i) rec[j] = acc[j];
    }
    // the workgroup's 16 views in index order (a group past the last view adds zeros)
#pragma unroll
    for (int j = kStB; j < kStAcc; ++j)
        if (stTotSlot(j) >= 0 && (j & 15) == i) sh[grp][stTotSlot(j)] = acc[j];
    __syncthreads();
    if (tid < kStTot) {
        double s = 0.0;
#pragma unroll
        for (int g = 0; g < 16; ++g) s += sh[g][tid];
        bf.partA[cand][(int64_t)blockIdx.x * kStTot + tid] = s;
    }
}

// The candidate's totals, then the decision (stereo_decide).
template <int NTOT>
__global__ __launch_bounds__(256) void stereo_decide_kernel(StereoBufs bf, int nwg) {
    static_assert(NTOT == kStTot && NTOT <= 64, "one lane per summed entry");
    __shared__ double sh[4][64];
    if (bf.st->done) return;
    const int cand = bf.st->cur ^ 1, tid = threadIdx.x;
    joint_sum_partials<NTOT>(bf.partA[cand], nwg, sh);
    if (tid < NTOT) bf.tot[cand][tid] = joint_total(sh, tid);
    if (tid == 0) stereo_decide<6>(bf, cand, joint_total(sh, 27) + joint_total(sh, 28));
}

// Per view: Lc Lc^T = V + lam diag V; lane c < 6 substitutes row c of E, lane 6 the view gradient; row c of
// E V^-1 E^T and of E V^-1 g are dot products of lane c's z with every lane's. A view with fewer than three points in
// total, or with a pivot that is not positive, counts as failed (pose_lm_kernel's rule).
template <int VIEWS>
__global__ __launch_bounds__(16 * VIEWS) void stereo_schur_kernel(StereoCam ca, StereoCam cb, StereoBufs bf) {
    static_assert(VIEWS == 16, "16 lanes per view, 16 views per workgroup");
    __shared__ double sh[VIEWS][kStSchur];
    const StereoState* st = bf.st;
    if (st->done) return;
    const int tid = threadIdx.x, i = tid & 15, grp = tid >> 4;
    const int64_t view = (int64_t)blockIdx.x * 16 + grp;
    double t[7];
#pragma unroll
    for (int c = 0; c < 7; ++c) t[c] = 0.0;
    bool failed = false;
    if (view < bf.M) {                         // whole 16-lane group together
        const double* __restrict__ rec = bf.rec[st->cur] + view * kStRecord;
        const int64_t n = (ca.offs[view + 1] - ca.offs[view]) + (cb.offs[view + 1] - cb.offs[view]);
        double V[21], b[6], invd[6], z[6];
#pragma unroll
        for (int j = 0; j < 21; ++j) V[j] = rec[kStV + j];
        const int boff = i < 6 ? kStE + i * 6 : kStGv;
#pragma unroll
        for (int m = 0; m < 6; ++m) b[m] = rec[boff + m];
        failed = !eliminate(V, b, st->lam, invd, z) || n < 3;
        auto dots = [&](auto cc) {
            constexpr int c = decltype(cc)::value;
            double s = 0.0;
#pragma unroll
            for (int m = 0; m < 6; ++m) s += z[m] * row_bcast<c>(z[m]);
            t[c] = s;
        };
        dots(std::integral_constant<int, 0>{}); dots(std::integral_constant<int, 1>{});
        dots(std::integral_constant<int, 2>{}); dots(std::integral_constant<int, 3>{});
        dots(std::integral_constant<int, 4>{}); dots(std::integral_constant<int, 5>{});
        dots(std::integral_constant<int, 6>{});
    }
    if (i < 6) {
#pragma unroll
        for (int c = 0; c < 7; ++c) sh[grp][i * 7 + c] = t[c];
    } else if (i == 6) {
        sh[grp][42] = failed ? 1.0 : 0.0;
    }
    __syncthreads();
    if (tid < kStSchur) {
        double s = 0.0;
#pragma unroll
        for (int g = 0; g < 16; ++g) s += sh[g][tid];
        bf.partC[(int64_t)blockIdx.x * kStSchur + tid] = s;
    }
}

// S = B + lam diag B - sum_i E_i V_i^-1 E_i^T, s = g_rig - sum_i E_i V_i^-1 g_i, delta_rig = S^-1 s (Cholesky).
// A failed view or a pivot of S that is not positive ends the loop with CALIB_E_SINGULAR (-3).
template <int NSUM>
__global__ __launch_bounds__(256) void stereo_rig_kernel(StereoBufs bf, int nwg) {
    static_assert(NSUM == kStSchur && NSUM <= 64, "one lane per summed entry");
    __shared__ double sh4[4][64];
    __shared__ double sh[NSUM];
    StereoState* st = bf.st;
    if (st->done) return;
    const int tid = threadIdx.x;
    joint_sum_partials<NSUM>(bf.partC, nwg, sh4);
    if (tid < NSUM) sh[tid] = joint_total(sh4, tid);
    __syncthreads();
    if (tid != 0) return;
    bool ok = !(sh[42] != 0.0);
    const double* __restrict__ tot = bf.tot[st->cur];
    const double lam = st->lam;
    double S[21], s[6], invd[6], z[6], d[6];
#pragma unroll
    for (int a = 0; a < 6; ++a) {
#pragma unroll
        for (int b = 0; b <= a; ++b) {
            const double B = tot[tri(a, b)];
            S[tri(a, b)] = (a == b ? B + lam * B : B) - sh[a * 7 + b];
        }
        s[a] = tot[21 + a] - sh[a * 7 + 6];
    }
    ok = eliminate(S, s, 0.0, invd, z) && ok;
    backward6(S, invd, z, d);
    if (!ok) {
        stereo_stop(st, -3);
        return;
    }
#pragma unroll
    for (int a = 0; a < 6; ++a) st->dsh[a] = d[a];
}

}  // namespace calib
