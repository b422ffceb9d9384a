// What the rig-only (stereo.hpp) and the joint (stereo_joint.hpp) stereo solver share (device code, gfx950): the
// buffers, the loop state, the decision and the end of the loop, the fixed-order sum of the workgroup partials and the
// back-substitution. (Camera b's chain rule into the columns of a view's pose is NOT here: as a shared function the
// compiler contracts it differently in stereo_joint_blocks_kernel, so each blocks kernel keeps its text.)
//
// Both solve a block-arrow problem P = (shared[S], pose_0[6], .., pose_{M-1}[6]) -- S = 6 (the rig) or LA + LB + 6 -- in
// rounds of five launches: blocks at the CANDIDATE, decide, Schur at the ACCEPTED point, solve of the shared system,
// back-substitution into the next candidate. Every kernel returns at once when the state says the loop is over, so
// the host may run ahead.
#pragma once
#include "kernels.hpp"

namespace calib {

constexpr int kJMaxS = 42;            // shared unknowns at most: the seven rigs of eight cameras (rig.hpp; the joint problem has 26)

// one camera's correspondences (the rig-only solver's known cameras travel beside them: stereo_blocks_kernel)
struct StereoCam {
    const int64_t* offs; const double2* uv; const double* xyz;
};

struct StereoState {
    double lam, err_cur, last_err, lam_min, lam_max, err_min;
    double dsh[kJMaxS];             // the shared part of the step (rig-only: [0, 6))
    unsigned long long fixed;       // bit s: shared unknown s is held fixed (rig-only: 0)
    int cur;        // index of the buffers holding the accepted point; the candidate lives in cur ^ 1
    int round;      // 0: the next decide is the bootstrap (the candidate IS the start point)
    int iters, max_iters, done, error;
    int* notify;    // host-visible word set when the loop is over (or null)
};

struct StereoBufs {
    double* P[2];         // S + 6 M
    double* rec[2];       // M * the solver's record stride
    double* partA[2];     // workgroups of the blocks kernel * its summed entries
    double* tot[2];       // the summed entries
    double* partC;        // workgroups of the Schur kernel * its summed entries
    double* delta;        // S + 6 M: the last step
    double* trace;        // max_iters * (CALIB_TRACE_HEADER + S), or null
    StereoState* st;
    int64_t M;
};

// the loop is over, with an error code (CALIB_E_*) or 0
__device__ __forceinline__ void stereo_stop(StereoState* st, int error) {
    if (error) st->error = error;
    st->done = 1;
    if (st->notify) __hip_atomic_store(st->notify, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// Lane 0 of a decide kernel, err1 the candidate's error: the decision of src/calibrate.py:161-168. Round 0 is the
// bootstrap (the candidate is the start point). Then accept iff err(P + delta) < err(P) strictly (NaN rejects), lambda
// / 10 or * 10, the trace row with the NSH shared unknowns of the point the step left from, stop when lambda leaves
// (lam_min, lam_max) or err(P) < err_min or max_iters ran.
template <int NSH>
__device__ __forceinline__ void stereo_decide(const StereoBufs& bf, int cand, double err1) {
    StereoState* st = bf.st;
    if (st->round == 0) {
        st->err_cur = err1;
        st->cur = cand;
        st->round = 1;
        return;
    }
    const int it = st->iters;
    const double err0 = st->err_cur, lam = st->lam;
    const bool accepted = err1 < err0;
    if (bf.trace) {
        double* row = bf.trace + (int64_t)it * (5 + NSH);
        row[0] = it; row[1] = err0; row[2] = err1; row[3] = lam; row[4] = accepted ? 1.0 : 0.0;
        for (int j = 0; j < NSH; ++j) row[5 + j] = bf.P[cand ^ 1][j];
    }
    const double lam1 = accepted ? lam / 10 : lam * 10;
    if (accepted) { st->cur = cand; st->err_cur = err1; }
    st->lam = lam1;
    st->last_err = err0;
    st->iters = it + 1;
    st->round = st->round + 1;
    if (!(st->lam_min < lam1 && lam1 < st->lam_max) || err0 < st->err_min || it + 1 >= st->max_iters) stereo_stop(st, 0);
}

// Entry j < N (any N <= NP) of the nwg workgroup partials (rows of N doubles), summed in one fixed order by 256 lanes:
// lane (seg, j) adds its quarter of the rows of entries j, j + 64, .. in index order -- eight loads in flight at a time,
// a chain of dependent loads is what a one-wave sum of 625 rows spent 150 us on -- and after the barrier
// total j = ((q0 + q1) + q2) + q3 from sh.
template <int N, int NP>
__device__ __forceinline__ void joint_sum_partials(const double* __restrict__ p, int nwg, double (&sh)[4][NP]) {
    const int seg = threadIdx.x >> 6;
    const int q = (nwg + 3) / 4, w0 = seg * q, w1 = min(nwg, (seg + 1) * q);
    for (int j = threadIdx.x & 63; j < N; j += 64) {
        double s = 0.0;
        int w = w0;
        for (; w + 8 <= w1; w += 8) {
            double v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = p[(int64_t)(w + u) * N + j];
#pragma unroll
            for (int u = 0; u < 8; ++u) s += v[u];
        }
        for (; w < w1; ++w) s += p[(int64_t)w * N + j];
        sh[seg][j] = s;
    }
    __syncthreads();
}
template <int NP>
__device__ __forceinline__ double joint_total(const double (&sh)[4][NP], int j) {
    return ((sh[0][j] + sh[1][j]) + sh[2][j]) + sh[3][j];
}

// One lane per view: delta_i = (V_i + lam diag V_i)^-1 (g_i - E_i^T delta_shared); the next candidate = accepted point +
// delta. REC places V, E (shared row, view column) and g_view in the view's record of REC::kStride doubles. A fixed
// shared unknown is copied, not added to: its bits are kept (-0.0 + 0.0 is +0.0).
template <typename REC, int S>
__global__ __launch_bounds__(64) void stereo_backsub_kernel(StereoBufs bf) {
    const StereoState* st = bf.st;
    if (st->done) return;
    const int64_t view = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (view >= bf.M) return;
    const int cur = st->cur;
    const double* __restrict__ rec = bf.rec[cur] + view * REC::kStride;
    const double* __restrict__ Pc = bf.P[cur];
    double* __restrict__ Pn = bf.P[cur ^ 1];
    double V[21], b[6], invd[6], z[6], d[6];
#pragma unroll
    for (int j = 0; j < 21; ++j) V[j] = rec[REC::kV + j];
#pragma unroll
    for (int m = 0; m < 6; ++m) b[m] = rec[REC::kGv + m];
    for (int s = 0; s < S; ++s) {
        const double ds = st->dsh[s];
#pragma unroll
        for (int m = 0; m < 6; ++m) b[m] -= rec[REC::kE + s * 6 + m] * ds;
    }
    eliminate(V, b, st->lam, invd, z);
    backward6(V, invd, z, d);
#pragma unroll
    for (int m = 0; m < 6; ++m) {
        const int64_t o = S + 6 * view + m;
        bf.delta[o] = d[m];
        Pn[o] = Pc[o] + d[m];
    }
    if (view == 0) {
        const unsigned long long fixed = st->fixed;
        for (int s = 0; s < S; ++s) {
            const double ds = st->dsh[s];
            bf.delta[s] = ds;
            Pn[s] = ((fixed >> s) & 1) ? Pc[s] : Pc[s] + ds;
        }
    }
}

}  // namespace calib
