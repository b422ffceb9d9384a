// Multi-camera rig calibration: N known cameras, one board (device code, gfx950).
//
// Unknowns Pr = (rig_1[6], .., rig_{N-1}[6], pose_0[6], .., pose_{M-1}[6]), every 6-tuple Euler angles in DEGREES then t
// (pose_view_constants). pose_i takes board points into camera 0's frame, X0 = R_i X + t_i; rig_c takes camera 0's frame
// into camera c's, Xc = R_c X0 + t_c. Residuals uv_c - project_c(Xc); every camera's shared vector is held fixed. The
// S = 6 (N - 1) <= 42 leading unknowns are shared by all views: B (S x S) is block diagonal, one 6 x 6 block per camera
// c >= 1 (no row touches two rigs), E_i (S x 6) has a zero 6 x 6 block for every camera that did not see view i, V_i
// (6 x 6). A camera-0 row is stereo_blocks_kernel's camera-a row, a camera-c row its camera-b row with rig_c as the rig.
//
// One LM round (src/calibrate.py:143-171) is the five launches of stereo.hpp, every sum in one fixed order, no
// floating-point atomics:
//   rig_blocks_kernel      per view (16 lanes), at the CANDIDATE, the cameras in index order: V_i and g_view accumulate
//                          over the cameras; E_c, B_c, g_c and the camera's error are summed over the 16 lanes and stored
//                          after each camera (the accumulators do not grow with N) -> the view's record (V, E, g_view);
//                          B_c, g_c and the N errors summed over the workgroup's 16 views in index order -> one partial
//   rig_decide_kernel      one workgroup: the partials in one order, then accept / lambda / stop (round 0: bootstrap)
//   rig_schur_kernel       16 lanes per view at the ACCEPTED point: Z = Lc^-1 E_i^T (6 x S) and Lc^-1 g_i with cholesky6 /
//                          forward6, lane i the right-hand sides i, i + 16, i + 32; the workgroup's 16 views' Z^T Z and
//                          Z^T z_g summed in view order -> one partial (zero blocks are multiplied like any other)
//   rig_solve_kernel       one workgroup: partials in one order, B + lam diag B - sum, Cholesky of the S x S system in
//                          one wave's registers (lane i holds row i), substitution -> delta_shared
//   stereo_backsub_kernel  one lane per view (stereo_loop.hpp's, on RigLayout's record with this S)
// The buffers, the state, the decision, the end of the loop and the sum of the partials are stereo_loop.hpp's. All
// kernels are templates on the number of cameras: they are emitted where they are first launched, at the end of the
// module.
#pragma once
#include "stereo_joint.hpp"

namespace calib {

constexpr int kRigMaxCams = 8;
static_assert(6 * (kRigMaxCams - 1) <= kJMaxS, "StereoState::dsh holds the shared part of the step");

// the cameras of a call: correspondences, the known shared vector and the model id of each
struct RigCams {
    StereoCam cam[kRigMaxCams];
    const double* shared[kRigMaxCams];
    int model[kRigMaxCams];
};

template <int NC>
struct RigLayout {
    static_assert(NC >= 2 && NC <= kRigMaxCams, "2 to 8 cameras");
    static constexpr int S = 6 * (NC - 1);
    // view record: V lower triangle, E row-major (shared row, view column; camera c's block at 36 (c - 1)), g_view
    static constexpr int kV = 0, kE = 21, kGv = 21 + 6 * S, kRec = kGv + 6, kStride = (kRec + 7) / 8 * 8;
    // what is summed over the views: per camera c >= 1 the lower triangle of B_c (21) and g_c (6), then the N errors
    static constexpr int kCam = 27, kErr = kCam * (NC - 1), kTot = kErr + NC;
    // Schur partial: lower triangle of sum Z^T Z (S x S), sum E V^-1 g (S), number of failed views
    static constexpr int kZZ = 0, kEg = S * (S + 1) / 2, kFail = kEg + S, kSchur = kFail + 1;
    // slot of B(i, j), i >= j, among the summed entries; -1: a zero block
    static __host__ __device__ constexpr int slotB(int i, int j) {
        return i / 6 == j / 6 ? kCam * (i / 6) + (i % 6) * (i % 6 + 1) / 2 + j % 6 : -1;
    }
};

// what one camera adds to a view, per lane: its part of V and g_view (kept over the cameras), E_c, B_c, g_c, its error
struct RigAcc {
    double V[21], gv[6], E[36], B[21], g[6], err;
};

// camera 0's points q = i, i + 16, .. of a view: stereo_blocks_kernel's camera-a rows
template <int MODEL>
__device__ __forceinline__ void rig_rows_cam0(const StereoCam& cm, const double* __restrict__ shared, int64_t view, int i,
                                              const double (&vc)[kViewStride], RigAcc& acc) {
    constexpr int L = ModelTraits<MODEL>::L, C = ModelTraits<MODEL>::C;
    Shared<MODEL, double> sp;
    sp.load(shared);
    const int64_t p0 = cm.offs[view];
    const int n = (int)(cm.offs[view + 1] - p0);
    for (int q = i; q < n; q += 16) {
        const double2 m = cm.uv[p0 + q];
        const double* X = cm.xyz + 3 * (p0 + q);
        double u, v;
        double2 J[C];
        jacobian_point<MODEL, double>(sp, vc, X[0], X[1], X[2], u, v, J);
        const double ru = m.x - u, rv = m.y - v;
#pragma unroll
        for (int a = 0; a < 6; ++a) {
#pragma unroll
            for (int b = 0; b <= a; ++b) acc.V[tri(a, b)] += J[L + a].x * J[L + b].x + J[L + a].y * J[L + b].y;
            acc.gv[a] += J[L + a].x * ru + J[L + a].y * rv;
        }
        acc.err += ru * ru + rv * rv;
    }
}

// camera c >= 1: stereo_blocks_kernel's camera-b rows with rig_c (constants vr) as the rig
template <int MODEL>
__device__ __forceinline__ void rig_rows_camc(const StereoCam& cm, const double* __restrict__ shared, int64_t view, int i,
                                              const double (&vc)[kViewStride], const double (&vr)[kViewStride], RigAcc& acc) {
    constexpr int L = ModelTraits<MODEL>::L, C = ModelTraits<MODEL>::C;
    Shared<MODEL, double> sp;
    sp.load(shared);
    const int64_t p0 = cm.offs[view];
    const int n = (int)(cm.offs[view + 1] - p0);
    for (int q = i; q < n; q += 16) {
        const double2 m = cm.uv[p0 + q];
        const double* X = cm.xyz + 3 * (p0 + q);
        const double q0 = vc[0] * X[0] + vc[1] * X[1] + vc[2] * X[2];       // R_i X
        const double q1 = vc[3] * X[0] + vc[4] * X[1] + vc[5] * X[2];
        const double q2 = vc[6] * X[0] + vc[7] * X[1] + vc[8] * X[2];
        double u, v;
        double2 J[C];
        jacobian_point<MODEL, double>(sp, vr, q0 + vc[9], q1 + vc[10], q2 + vc[11], u, v, J);
        const double ru = m.x - u, rv = m.y - v;
        // G R_rig (2 x 3), G = d(uv)/dXc = the translation columns
        double2 GR[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            GR[k].x = J[L + 3].x * vr[k] + J[L + 4].x * vr[3 + k] + J[L + 5].x * vr[6 + k];
            GR[k].y = J[L + 3].y * vr[k] + J[L + 4].y * vr[3 + k] + J[L + 5].y * vr[6 + k];
        }
        // dX0/drho_i = (pi/180) a. x q (jacobian_stage_b), dX0/dt_i = I
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
            const double2 Jr = J[L + a];
#pragma unroll
            for (int b = 0; b <= a; ++b) {
                acc.V[tri(a, b)] += Jv[a].x * Jv[b].x + Jv[a].y * Jv[b].y;
                acc.B[tri(a, b)] += Jr.x * J[L + b].x + Jr.y * J[L + b].y;
            }
#pragma unroll
            for (int b = 0; b < 6; ++b) acc.E[a * 6 + b] += Jr.x * Jv[b].x + Jr.y * Jv[b].y;
            acc.g[a] += Jr.x * ru + Jr.y * rv;
            acc.gv[a] += Jv[a].x * ru + Jv[a].y * rv;
        }
        acc.err += ru * ru + rv * rv;
    }
}

template <int NC>
__global__ __launch_bounds__(256) void rig_blocks_kernel(RigCams rc, StereoBufs bf) {
    using Y = RigLayout<NC>;
    __shared__ double sh[16][Y::kTot];
    if (bf.st->done) return;
    const int cand = bf.st->cur ^ 1;
    const double* __restrict__ Pr = bf.P[cand];
    const int tid = threadIdx.x, i = tid & 15, grp = tid >> 4;
    const int64_t view = (int64_t)blockIdx.x * 16 + grp;
    const bool live = view < bf.M;                 // whole 16-lane group together
    double* __restrict__ rec = bf.rec[cand] + (live ? view : 0) * Y::kStride;
    RigAcc acc;
#pragma unroll
    for (int j = 0; j < 21; ++j) acc.V[j] = 0.0;
#pragma unroll
    for (int j = 0; j < 6; ++j) acc.gv[j] = 0.0;
    double vc[kViewStride];
    if (live) {
        double e[6];
#pragma unroll
        for (int j = 0; j < 6; ++j) e[j] = Pr[Y::S + 6 * view + j];
        pose_view_constants(e, vc);
        acc.err = 0.0;
        if (rc.model[0] == kRadtan) rig_rows_cam0<kRadtan>(rc.cam[0], rc.shared[0], view, i, vc, acc);
        else rig_rows_cam0<kFisheye>(rc.cam[0], rc.shared[0], view, i, vc, acc);
        acc.err = group_sum16(acc.err);
    } else {
        acc.err = 0.0;
    }
    if (i == 0) sh[grp][Y::kErr] = acc.err;
#pragma unroll 1
    for (int c = 1; c < NC; ++c) {           // one body for every camera
#pragma unroll
        for (int j = 0; j < 36; ++j) acc.E[j] = 0.0;
#pragma unroll
        for (int j = 0; j < 21; ++j) acc.B[j] = 0.0;
#pragma unroll
        for (int j = 0; j < 6; ++j) acc.g[j] = 0.0;
        acc.err = 0.0;
        if (live) {
            double rg[6], vr[kViewStride];
#pragma unroll
            for (int j = 0; j < 6; ++j) rg[j] = Pr[6 * (c - 1) + j];
            pose_view_constants(rg, vr);
            if (rc.model[c] == kRadtan) rig_rows_camc<kRadtan>(rc.cam[c], rc.shared[c], view, i, vc, vr, acc);
            else rig_rows_camc<kFisheye>(rc.cam[c], rc.shared[c], view, i, vc, vr, acc);
            // the camera's own blocks leave the registers here (a camera without points in the view: exact zeros)
#pragma unroll
            for (int j = 0; j < 36; ++j) {
                const double s = group_sum16(acc.E[j]);
                if ((j & 15) == i) rec[Y::kE + 36 * (c - 1) + j] = s;
            }
#pragma unroll
            for (int j = 0; j < 21; ++j) acc.B[j] = group_sum16(acc.B[j]);
#pragma unroll
            for (int j = 0; j < 6; ++j) acc.g[j] = group_sum16(acc.g[j]);
            acc.err = group_sum16(acc.err);
        }
        double* o = &sh[grp][Y::kCam * (c - 1)];
#pragma unroll
        for (int j = 0; j < 21; ++j)
            if ((j & 15) == i) o[j] = acc.B[j];
#pragma unroll
        for (int j = 0; j < 6; ++j)
            if (((21 + j) & 15) == i) o[21 + j] = acc.g[j];
        if (i == 0) sh[grp][Y::kErr + c] = acc.err;
    }
    if (live) {
#pragma unroll
        for (int j = 0; j < 21; ++j) {
            const double s = group_sum16(acc.V[j]);
            if ((j & 15) == i) rec[Y::kV + j] = s;
        }
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            const double s = group_sum16(acc.gv[j]);
            if (j == i) rec[Y::kGv + j] = s;
        }
    }
    __syncthreads();
    // the workgroup's 16 views in index order (a group past the last view adds zeros)
    if (tid < Y::kTot) {
        double s = 0.0;
#pragma unroll
        for (int g = 0; g < 16; ++g) s += sh[g][tid];
        bf.partA[cand][(int64_t)blockIdx.x * Y::kTot + tid] = s;
    }
}

// The candidate's totals, then the decision (stereo_decide, with S trace columns): the error is the cameras' in index order.
template <int NC>
__global__ __launch_bounds__(256) void rig_decide_kernel(StereoBufs bf, int nwg) {
    using Y = RigLayout<NC>;
    static_assert(Y::kTot <= 256, "one lane per summed entry");
    __shared__ double sh[4][Y::kTot + 1];
    if (bf.st->done) return;
    const int cand = bf.st->cur ^ 1, tid = threadIdx.x;
    joint_sum_partials<Y::kTot>(bf.partA[cand], nwg, sh);
    if (tid < Y::kTot) bf.tot[cand][tid] = joint_total(sh, tid);
    if (tid == 0) {
        double err = joint_total(sh, Y::kErr);
        for (int c = 1; c < NC; ++c) err += joint_total(sh, Y::kErr + c);
        stereo_decide<Y::S>(bf, cand, err);
    }
}

// Per view: Lc Lc^T = V + lam diag V; lane i substitutes right-hand sides i, i + 16, i + 32 of the S + 1 (rows of E, then
// the view gradient) into the workgroup's LDS; then entry e of (Z^T Z | Z^T z_g) is summed over the 16 views in index
// order by thread e, e + 256, .. A view with fewer than three points over all cameras, or with a pivot that is not
// positive, counts as failed.
template <int NC>
__global__ __launch_bounds__(256) void rig_schur_kernel(RigCams rc, StereoBufs bf) {
    using Y = RigLayout<NC>;
    constexpr int S = Y::S, ZS = (S + 1) * 6;
    __shared__ double zs[16][ZS];
    __shared__ double sfail[16];
    const StereoState* st = bf.st;
    if (st->done) return;
    const int tid = threadIdx.x, i = tid & 15, grp = tid >> 4;
    const int64_t view = (int64_t)blockIdx.x * 16 + grp;
    if (view < bf.M) {                         // whole 16-lane group together
        const double* __restrict__ rec = bf.rec[st->cur] + view * Y::kStride;
        int64_t n = 0;
        for (int c = 0; c < NC; ++c) n += rc.cam[c].offs[view + 1] - rc.cam[c].offs[view];
        double V[21], invd[6];
#pragma unroll
        for (int j = 0; j < 21; ++j) V[j] = rec[Y::kV + j];
        const bool failed = !cholesky6(V, st->lam, invd) || n < 3;
        for (int r = i; r <= S; r += 16) {                                       // row r of E, or g_view (kGv = kE + 6 S)
            double b[6], z[6];
#pragma unroll
            for (int m = 0; m < 6; ++m) b[m] = rec[Y::kE + r * 6 + m];
            forward6(V, invd, b, z);
#pragma unroll
            for (int m = 0; m < 6; ++m) zs[grp][r * 6 + m] = z[m];
        }
        if (i == 0) sfail[grp] = failed ? 1.0 : 0.0;
    } else {
        for (int j = i; j < ZS; j += 16) zs[grp][j] = 0.0;
        if (i == 0) sfail[grp] = 0.0;
    }
    __syncthreads();
    for (int e = tid; e < Y::kSchur; e += 256) {
        double s = 0.0;
        if (e < Y::kFail) {
            int a, b;
            if (e < Y::kEg) { a = tri_row(e); b = e - a * (a + 1) / 2; } else { a = e - Y::kEg; b = S; }
#pragma unroll
            for (int g = 0; g < 16; ++g) {
                const double* za = &zs[g][a * 6];
                const double* zb = &zs[g][b * 6];
                double d = 0.0;
#pragma unroll
                for (int m = 0; m < 6; ++m) d += za[m] * zb[m];
                s += d;
            }
        } else {
#pragma unroll
            for (int g = 0; g < 16; ++g) s += sfail[g];
        }
        bf.partC[(int64_t)blockIdx.x * Y::kSchur + e] = s;
    }
}

// A = B + lam diag B - sum Z^T Z, b = g_shared - sum E V^-1 g, then delta_shared = A^-1 b: Cholesky in the registers of
// wave 0, lane i holding row i (S <= 42 lanes), pivots and multipliers passed by v_readlane. A failed view or a pivot that
// is not positive -- a camera c >= 1 that sees nothing, for one -- ends the loop with CALIB_E_SINGULAR (-3).
template <int NC>
__global__ __launch_bounds__(256) void rig_solve_kernel(StereoBufs bf, int nwg) {
    using Y = RigLayout<NC>;
    constexpr int S = Y::S;
    static_assert(S <= 64, "one lane per row");
    __shared__ double sh[4][Y::kSchur + 1];
    __shared__ double Lsh[S][S + 1];
    StereoState* st = bf.st;
    if (st->done) return;
    const int tid = threadIdx.x;
    joint_sum_partials<Y::kSchur>(bf.partC, nwg, sh);
    if (tid >= 64) return;
    const int i = tid < S ? tid : S - 1;                     // lanes past S repeat the last row; nothing reads them
    const double* __restrict__ tot = bf.tot[st->cur];
    const double lam = st->lam;
    double row[S];
#pragma unroll
    for (int cI = 0; cI < S; ++cI) {
        const int hi = i > cI ? i : cI, lo = i > cI ? cI : i;
        const int slot = Y::slotB(hi, lo);
        const double B = slot >= 0 ? tot[slot >= 0 ? slot : 0] : 0.0;
        row[cI] = (cI == i ? B + lam * B : B) - joint_total(sh, Y::kZZ + hi * (hi + 1) / 2 + lo);
    }
    double y = tot[Y::kCam * (i / 6) + 21 + i % 6] - joint_total(sh, Y::kEg + i);
    bool ok = !(joint_total(sh, Y::kFail) != 0.0);
    double invs[S];
#pragma unroll
    for (int j = 0; j < S; ++j) {
        const double d = readlane_d(row[j], j);
        if (!(d > 0.0)) ok = false;
        const double inv = rsqrt_nr(d);
        invs[j] = inv;
        const double lij = row[j] * inv;
        row[j] = lij;
#pragma unroll
        for (int cI = j + 1; cI < S; ++cI) row[cI] -= lij * readlane_d(lij, cI);
    }
    if (!ok) {                                               // the same for every lane
        if (tid == 0) stereo_stop(st, -3);
        return;
    }
    // forward: z_j = y_j / L_jj, y_i -= L_ij z_j (i > j); lane j keeps z_j
    double t = 0.0;
#pragma unroll
    for (int j = 0; j < S; ++j) {
        const double zj = readlane_d(y, j) * invs[j];
        t = tid == j ? zj : t;
        y -= row[j] * zj;
    }
    // backward needs column j of L in lane order: through LDS
    if (tid < S) {
#pragma unroll
        for (int cI = 0; cI < S; ++cI) Lsh[tid][cI] = row[cI];
    }
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int j = S - 1; j >= 0; --j) {
        const double xj = readlane_d(t, j) * invs[j];
        if (tid < j) t -= Lsh[j][tid] * xj;
        if (tid == 0) st->dsh[j] = xj;
    }
}

}  // namespace calib
