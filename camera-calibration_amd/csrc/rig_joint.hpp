// Joint rig calibration: N cameras, their rigs and the board poses in one problem (device code, gfx950).
//
// Unknowns, camera-major: Pq = (shared_0[L0] | shared_1[L1], rig_1[6] | .. | shared_{N-1}, rig_{N-1}[6] | pose_0[6], ..,
// pose_{M-1}[6]); the shared vectors in the order of P, the 6-tuples, frames and residuals those of rig.hpp. The
// S = sum L_c + 6 (N - 1) <= 122 leading unknowns are shared by all views. No row touches two cameras, so in this order B
// is block diagonal with contiguous blocks (L0 wide for camera 0, L_c + 6 <= 16 for camera c >= 1); E_i (S x 6) has a zero
// band for every camera that missed view i; V_i is 6 x 6; the reduced system is dense S x S. At N = 2 Pq is
// stereo_joint.hpp's Pj.
//
// The model of a camera, L_c and every offset are run-time, launch-uniform values (RigJointDesc): the kernels are
// instantiated once, not per number of cameras or mix of models. One LM round is the five launches of stereo_loop.hpp,
// every sum in one fixed order, no floating-point atomics:
//   rig_joint_blocks_kernel   one wave per view at the CANDIDATE, two waves per workgroup, a grid of at most
//                             kRjBlocksGrid workgroups whose waves loop over their views. Per view the cameras in index
//                             order: camera 0 is stereo_joint_blocks_kernel's camera-a pass (tile T00 = J0^T J0), camera
//                             c >= 1 its camera-b pass (T00, T10 = J1^T J0, T11 = J1^T J1), through the odd-stride LDS slab
//                             into v_mfma_f64_16x16x4_f64. After each camera the tiles are parked in LDS: its E band goes
//                             to the view's record, V and g_view add up in one register per lane, its B block, g and error
//                             add to the wave's resident partial (LDS). The workgroup's two waves summed -> one partial.
//   rig_joint_decide_kernel   one workgroup: the <= kRjBlocksGrid partials in index order, then accept / lambda / stop
//   rig_joint_schur_kernel    64 lanes per view, four views per pass at the ACCEPTED point, a grid of at most
//                             kRjSchurGrid workgroups that loop over their passes: Z = Lc^-1 E_i^T (6 x S) and Lc^-1 g_i
//                             into LDS, then thread t adds the views' parts of entries t, t + 256, .. of (Z^T Z | Z^T z_g)
//                             to 30 resident registers, in view order -> one partial per workgroup
//   rig_joint_solve_kernel    one workgroup: the <= kRjSchurGrid partials in index order into the packed lower triangle
//                             of B + lam diag B - sum (LDS, 59 KiB), the fixed mask, Cholesky, both substitutions
//   rig_joint_backsub_kernel  one lane per view (stereo_backsub_kernel with a run-time S, the step and the 128-bit mask in
//                             this solver's own arguments: StereoState::dsh holds 42 entries and stays as it is)
// Under a robust loss (the end of this file) rig_joint_robust_blocks_kernel takes the place of the first launch; the
// other four run unchanged on its totals and records. rig_residuals_kernel writes every point's residual.
// The buffers, the state and the end of the loop are stereo_loop.hpp's. The kernels need no compile-time argument; they
// are templates on the largest number of cameras all the same: a template is emitted where it is first launched, at the
// end of the module, so the module's other kernels keep their place and labels.
//
// Tile maps: stereo_joint.hpp's, with T00 in the place of Ta for camera 0.
#pragma once
#include "rig.hpp"

namespace calib {

constexpr int kRjMaxS = 16 + 16 * (kRigMaxCams - 1) - 6;            // 122: eight radtan cameras
constexpr int kRjMaxTri = kRjMaxS * (kRjMaxS + 1) / 2;              // 7503
constexpr int kRjMaxSchur = kRjMaxTri + kRjMaxS + 1;                // 7626
constexpr int kRjAcc = (kRjMaxSchur + 255) / 256;                   // resident sums per thread of the Schur kernel: 30
constexpr int kRjMaxTot = 55 + 136 * (kRigMaxCams - 1) + kRjMaxS + kRigMaxCams;    // 1137
constexpr int kRjWaves = 2;                                         // views in flight per workgroup of the blocks kernel
// partial rows the one-workgroup kernels read at most, whatever M. 512 two-wave workgroups of 63.4 KiB LDS are two per
// CU and one wave per SIMD of the 256 CUs: all resident at once (at 256 the blocks kernel took 1483 us instead of 786 on
// 10 000 views x 4 cameras x 200 points)
constexpr int kRjBlocksGrid = 512, kRjSchurGrid = 128;
constexpr int kRjSchurViews = 4;                                    // views per pass of the Schur kernel
// a wave's parked tiles (doubles): three 16 x 16 tiles, two J^T r vectors, the camera's error
constexpr int kRjT00 = 0, kRjT10 = 256, kRjT11 = 512, kRjG0 = 768, kRjG1 = 784, kRjE = 800, kRjPark = 808;

// The layout of one call: where camera c's unknowns, B block and sums live. Filled on the host, once per call.
struct RigJointDesc {
    int nc, S;
    int model[kRigMaxCams], L[kRigMaxCams];
    int off[kRigMaxCams];         // first unknown of camera c: shared_c, then (c >= 1) rig_c
    int bo[kRigMaxCams];          // first total of camera c's B block: the lower triangle, L_0 or L_c + 6 wide
    int kG, kErr, kTot;           // totals: the blocks, g_shared (S), the cameras' errors (nc)
    int kGv, kRec, kStride;       // view record: V lower triangle at 0, E (shared row, view column) at 21, g_view
    int kEg, kFail, kSchur;       // Schur partial: lower triangle of sum Z^T Z, sum E V^-1 g (S), failed views
    __host__ __device__ int width(int c) const { return c == 0 ? L[0] : L[c] + 6; }
};
constexpr int kRjE0 = 21;

struct RigJointArgs {
    RigJointDesc d;
    StereoCam cam[kRigMaxCams];
    double* dsh;                  // S: the shared part of the step
    unsigned long long fixed[2];  // bit s: shared unknown s is held fixed
    __device__ bool isFixed(int s) const { return (fixed[s >> 6] >> (s & 63)) & 1; }
};

// row of entry e of a lower triangle stored row by row, without tri_row's loop (e < 2^24)
__device__ __forceinline__ int tri_row_big(int e) {
    int a = (int)((__builtin_sqrt(8.0 * e + 1.0) - 1.0) * 0.5);
    while ((a + 1) * (a + 2) / 2 <= e) ++a;
    while (a * (a + 1) / 2 > e) --a;
    return a;
}

// stereo_decide with a run-time number of trace columns (the template is kept as it is: its kernels must not move)
__device__ __forceinline__ void rig_joint_decide(const StereoBufs& bf, int cand, double err1, int nsh) {
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
        double* row = bf.trace + (int64_t)it * (5 + nsh);
        row[0] = it; row[1] = err0; row[2] = err1; row[3] = lam; row[4] = accepted ? 1.0 : 0.0;
        for (int j = 0; j < nsh; ++j) row[5 + j] = bf.P[cand ^ 1][j];
    }
    const double lam1 = accepted ? lam / 10 : lam * 10;
    if (accepted) { st->cur = cand; st->err_cur = err1; }
    st->lam = lam1;
    st->last_err = err0;
    st->iters = it + 1;
    st->round = st->round + 1;
    if (!(st->lam_min < lam1 && lam1 < st->lam_max) || err0 < st->err_min || it + 1 >= st->max_iters) stereo_stop(st, 0);
}

// A robust loss of one launch (rig_joint_robust_blocks_kernel): CALIB_LOSS_HUBER or CALIB_LOSS_CAUCHY and its scale delta
// in pixels. A kernel argument of its own: RigJointArgs and StereoBufs keep their kernarg offsets.
constexpr int kLossHuber = 1, kLossCauchy = 2;
struct RigLoss {
    int kind;
    double scale;
};

// the tiles of one camera of one view, per lane
struct RigJointTiles {
    d4 t00U, t00V, t10U, t10V, t11U, t11V;
    double g0, g1, err;
};

// One camera's points of one view through the slab into the tiles. RIG = false: camera 0, columns [view 6 | shared | pad]
// (stereo_joint_blocks_kernel's camera a). RIG = true: camera c >= 1 with vr the constants of rig_c, J0 = [view 6 | shared |
// pad], J1 = [rig 6 | pad] (its camera b; the chain rule is written out as there).
// ROBUST: with s = |res|^2 the point's rows and residual are scaled by sqrt(w), w = rho'(s), before they reach the slab --
// the tiles are those of the re-weighted problem -- and t.err is the lane's own sum of rho(s) over its points, not the
// slab's sum of squares: the caller adds up all 64 lanes. A tail lane has s = 0: w = 1, rho = 0.
template <int MODEL, bool RIG, bool ROBUST = false>
__device__ __forceinline__ void rig_joint_pass(const StereoCam& cm, const double* __restrict__ shared, int64_t view, int lane,
                                               const double (&vc)[kViewStride], const double (&vr)[kViewStride],
                                               double2* slab, RigJointTiles& t, int lossKind = 0, double lossScale = 0.0) {
    constexpr int L = ModelTraits<MODEL>::L, C = ModelTraits<MODEL>::C;
    const int k = lane >> 4, c = lane & 15;
    const double2 zero2 = {0.0, 0.0};
    double2* const myRow = slab + (lane & (kJRows - 1)) * kJRowChunks;
    const double2* const src = slab + k * kJRowChunks + c;
    Shared<MODEL, double> sp;
    sp.load(shared);
    const int64_t p0 = cm.offs[view];
    const int n = (int)(cm.offs[view + 1] - p0);
    for (int q0 = 0; q0 < n; q0 += 64) {                                         // a camera that missed the view: zero trips
        const int q = q0 + lane;
        const bool live = q < n;
        const int64_t p = p0 + (live ? q : n - 1);                               // tail lanes: a clamped point, zeroed below
        const double2 m = cm.uv[p];
        const double* X = cm.xyz + 3 * p;
        double u, v;
        double2 J[C];
        double2 Jv[6];
        if constexpr (RIG) {
            const double qx = vc[0] * X[0] + vc[1] * X[1] + vc[2] * X[2];       // R_i X
            const double qy = vc[3] * X[0] + vc[4] * X[1] + vc[5] * X[2];
            const double qz = vc[6] * X[0] + vc[7] * X[1] + vc[8] * X[2];
            jacobian_point<MODEL, double>(sp, vr, qx + vc[9], qy + vc[10], qz + vc[11], u, v, J);
            // G R_rig (2 x 3), G = d(uv)/dXc = the translation columns
            double2 GR[3];
#pragma unroll
            for (int s = 0; s < 3; ++s) {
                GR[s].x = J[L + 3].x * vr[s] + J[L + 4].x * vr[3 + s] + J[L + 5].x * vr[6 + s];
                GR[s].y = J[L + 3].y * vr[s] + J[L + 4].y * vr[3 + s] + J[L + 5].y * vr[6 + s];
            }
            // dX0/drho_i = (pi/180) a. x q (jacobian_stage_b), dX0/dt_i = I
            const double ax0 = vc[12], ax1 = vc[13], ax2 = vc[14], ay0 = vc[15], ay1 = vc[16];
            const double deg = 0.017453292519943295;
            const double dx[3] = {ax1 * qz - ax2 * qy, ax2 * qx - ax0 * qz, ax0 * qy - ax1 * qx};
            const double dy[3] = {ay1 * qz, -ay0 * qz, ay0 * qy - ay1 * qx};
            const double dz[3] = {-deg * qy, deg * qx, 0.0};
            Jv[0].x = GR[0].x * dx[0] + GR[1].x * dx[1] + GR[2].x * dx[2];
            Jv[0].y = GR[0].y * dx[0] + GR[1].y * dx[1] + GR[2].y * dx[2];
            Jv[1].x = GR[0].x * dy[0] + GR[1].x * dy[1] + GR[2].x * dy[2];
            Jv[1].y = GR[0].y * dy[0] + GR[1].y * dy[1] + GR[2].y * dy[2];
            Jv[2].x = GR[0].x * dz[0] + GR[1].x * dz[1];
            Jv[2].y = GR[0].y * dz[0] + GR[1].y * dz[1];
            Jv[3] = GR[0]; Jv[4] = GR[1]; Jv[5] = GR[2];
        } else {
            jacobian_point<MODEL, double>(sp, vc, X[0], X[1], X[2], u, v, J);
#pragma unroll
            for (int s = 0; s < 6; ++s) Jv[s] = J[L + s];
        }
        double2 res;
        res.x = live ? m.x - u : 0.0;
        res.y = live ? m.y - v : 0.0;
        if constexpr (ROBUST) {
            const double s = res.x * res.x + res.y * res.y, d2 = lossScale * lossScale;
            double w, rho;
            if (lossKind == kLossHuber) {                                       // launch-uniform
                const double r = sqrt(s);
                w = s <= d2 ? 1.0 : lossScale / r;
                rho = s <= d2 ? s : 2.0 * lossScale * r - d2;
            } else {
                w = 1.0 / (1.0 + s / d2);
                rho = d2 * log1p(s / d2);
            }
            const double sw = sqrt(w);
#pragma unroll
            for (int cc = 0; cc < 6; ++cc) { Jv[cc].x *= sw; Jv[cc].y *= sw; }
#pragma unroll
            for (int cc = 0; cc < (RIG ? L + 6 : L); ++cc) { J[cc].x *= sw; J[cc].y *= sw; }
            res.x *= sw; res.y *= sw;
            t.err += rho;
        }
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            if (q0 + kJRows * half >= n) break;                                  // wave-uniform
            __builtin_amdgcn_wave_barrier();
            if ((lane >> 5) == half) {
#pragma unroll
                for (int cc = 0; cc < 16; ++cc) {
                    const double2 col = cc < 6 ? Jv[cc < 6 ? cc : 0] : (cc < 6 + L ? J[cc < 6 + L ? cc - 6 : 0] : zero2);
                    myRow[cc] = live_or_zero(live, col);
                }
                if constexpr (RIG) {
#pragma unroll
                    for (int cc = 0; cc < 6; ++cc) myRow[16 + cc] = live_or_zero(live, J[L + cc]);
                }
                myRow[kJResChunk] = res;
            }
            __builtin_amdgcn_wave_barrier();
            const int rows = min(kJRows, n - (q0 + kJRows * half));
            const int ng = (rows + 3) >> 2;                                      // rows past the end of the last group are zeros
            for (int s = 0; s < ng; ++s) {
                const double2 j0 = src[s * 4 * kJRowChunks];
                const double2 rr = slab[(4 * s + k) * kJRowChunks + kJResChunk];
                t.t00U = __builtin_amdgcn_mfma_f64_16x16x4f64(j0.x, j0.x, t.t00U, 0, 0, 0);
                t.t00V = __builtin_amdgcn_mfma_f64_16x16x4f64(j0.y, j0.y, t.t00V, 0, 0, 0);
                t.g0 += j0.x * rr.x + j0.y * rr.y;
                if constexpr (RIG) {
                    const double2 j1 = src[s * 4 * kJRowChunks + 16];
                    t.t10U = __builtin_amdgcn_mfma_f64_16x16x4f64(j1.x, j0.x, t.t10U, 0, 0, 0);
                    t.t10V = __builtin_amdgcn_mfma_f64_16x16x4f64(j1.y, j0.y, t.t10V, 0, 0, 0);
                    t.t11U = __builtin_amdgcn_mfma_f64_16x16x4f64(j1.x, j1.x, t.t11U, 0, 0, 0);
                    t.t11V = __builtin_amdgcn_mfma_f64_16x16x4f64(j1.y, j1.y, t.t11V, 0, 0, 0);
                    t.g1 += j1.x * rr.x + j1.y * rr.y;
                }
                if constexpr (!ROBUST) t.err += rr.x * rr.x + rr.y * rr.y;
            }
        }
    }
}

template <int NCMAX>
__global__ __launch_bounds__(64 * kRjWaves) void rig_joint_blocks_kernel(RigJointArgs a, StereoBufs bf) {
    __shared__ __attribute__((aligned(16))) double2 smem[kRjWaves * kJSlab];
    __shared__ double park[kRjWaves][kRjPark];
    __shared__ double part[kRjWaves][kRjMaxTot];
    static_assert(NCMAX == kRigMaxCams, "the partial holds eight cameras' blocks");
    if (bf.st->done) return;
    const RigJointDesc& d = a.d;
    const int cand = bf.st->cur ^ 1;
    const double* __restrict__ Pq = bf.P[cand];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int k = lane >> 4, c16 = lane & 15;
    double2* slab = smem + wave * kJSlab;
    double* T = park[wave];
    double* mine = part[wave];
    const double2 zero2 = {0.0, 0.0};
    // chunks no pass stores (J1's pad columns) stay zero from here on; camera 0 leaves J1 as the last camera wrote it
    // and does not read it
    for (int j = lane; j < kJSlab; j += 64) slab[j] = zero2;
    for (int j = lane; j < d.kTot; j += 64) mine[j] = 0.0;
    // this lane's entry of (V | g_view): its row and column in T00, or its place in g0
    const int va = lane < 21 ? tri_row(lane) : 0, vb = lane < 21 ? lane - va * (va + 1) / 2 : 0;
    const int64_t stride = (int64_t)gridDim.x * kRjWaves;
    for (int64_t view = (int64_t)blockIdx.x * kRjWaves + wave; view < bf.M; view += stride) {     // wave-uniform
        double e[6], vc[kViewStride];
#pragma unroll
        for (int j = 0; j < 6; ++j) e[j] = Pq[d.S + 6 * view + j];
        pose_view_constants(e, vc);
        // one view per wave: the constants are the same in every lane and live in scalar registers
#pragma unroll
        for (int j = 0; j < kViewStride; ++j) vc[j] = readlane_d(vc[j], 0);
        double* __restrict__ rec = bf.rec[cand] + view * d.kStride;
        double vacc = 0.0;                                                       // lane j < 27: entry j of (V | g_view)
#pragma unroll 1
        for (int c = 0; c < d.nc; ++c) {                                         // one body for every camera
            const int L = d.L[c], off = d.off[c];
            RigJointTiles t;
            t.t00U = d4{0.0, 0.0, 0.0, 0.0};
            t.t00V = t.t00U; t.t10U = t.t00U; t.t10V = t.t00U; t.t11U = t.t00U; t.t11V = t.t00U;
            t.g0 = 0.0; t.g1 = 0.0; t.err = 0.0;
            if (c == 0) {
                if (d.model[0] == kRadtan) rig_joint_pass<kRadtan, false>(a.cam[0], Pq + off, view, lane, vc, vc, slab, t);
                else rig_joint_pass<kFisheye, false>(a.cam[0], Pq + off, view, lane, vc, vc, slab, t);
            } else {
                double rg[6], vr[kViewStride];
#pragma unroll
                for (int j = 0; j < 6; ++j) rg[j] = Pq[off + L + j];
                pose_view_constants(rg, vr);
#pragma unroll
                for (int j = 0; j < kViewStride; ++j) vr[j] = readlane_d(vr[j], 0);
                if (d.model[c] == kRadtan) rig_joint_pass<kRadtan, true>(a.cam[c], Pq + off, view, lane, vc, vr, slab, t);
                else rig_joint_pass<kFisheye, true>(a.cam[c], Pq + off, view, lane, vc, vr, slab, t);
            }
            // the four points of a group sit in the four 16-lane rows of the wave
            t.g0 += __shfl_xor(t.g0, 16, 64);   t.g0 += __shfl_xor(t.g0, 32, 64);
            t.g1 += __shfl_xor(t.g1, 16, 64);   t.g1 += __shfl_xor(t.g1, 32, 64);
            t.err += __shfl_xor(t.err, 16, 64); t.err += __shfl_xor(t.err, 32, 64);
            __builtin_amdgcn_wave_barrier();                                     // the last camera's readers are through
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int o = (k + 4 * reg) * 16 + c16;
                T[kRjT00 + o] = t.t00U[reg] + t.t00V[reg];
                T[kRjT10 + o] = t.t10U[reg] + t.t10V[reg];
                T[kRjT11 + o] = t.t11U[reg] + t.t11V[reg];
            }
            if (k == 0) { T[kRjG0 + c16] = t.g0; T[kRjG1 + c16] = t.g1; }
            if (lane == 0) T[kRjE] = t.err;
            __builtin_amdgcn_wave_barrier();
            // V and g_view over the cameras in index order
            if (lane < 21) vacc += T[kRjT00 + va * 16 + vb];
            else if (lane < 27) vacc += T[kRjG0 + lane - 21];
            // the camera's band of E (a camera without points in the view: exact zeros)
            const int W = d.width(c);
            for (int j = lane; j < 6 * W; j += 64) {
                const int s = j / 6, v = j - 6 * s;
                rec[kRjE0 + (off + s) * 6 + v] = s < L ? T[kRjT00 + (6 + s) * 16 + v] : T[kRjT10 + (s - L) * 16 + v];
            }
            // its B block, g and error into the wave's resident partial: the wave's views in index order
            const int nb = W * (W + 1) / 2;
            for (int eI = lane; eI < nb; eI += 64) {
                const int i = tri_row(eI), j = eI - i * (i + 1) / 2;
                mine[d.bo[c] + eI] += i < L ? T[kRjT00 + (6 + i) * 16 + 6 + j]
                                            : j < L ? T[kRjT10 + (i - L) * 16 + 6 + j] : T[kRjT11 + (i - L) * 16 + (j - L)];
            }
            if (lane < W) mine[d.kG + off + lane] += lane < L ? T[kRjG0 + 6 + lane] : T[kRjG1 + lane - L];
            if (lane == 0) mine[d.kErr + c] += T[kRjE];
        }
        if (lane < 21) rec[lane] = vacc;
        else if (lane < 27) rec[d.kGv + lane - 21] = vacc;
    }
    __syncthreads();
    // the workgroup's waves in index order
    for (int eI = threadIdx.x; eI < d.kTot; eI += 64 * kRjWaves) {
        double s = part[0][eI];
#pragma unroll
        for (int w = 1; w < kRjWaves; ++w) s += part[w][eI];
        bf.partA[cand][(int64_t)blockIdx.x * d.kTot + eI] = s;
    }
}

// entry j of the nrows partial rows (n doubles each) in index order, eight loads in flight
__device__ __forceinline__ double rig_joint_sum_rows(const double* __restrict__ p, int nrows, int n, int j) {
    double s = 0.0;
    int w = 0;
    for (; w + 8 <= nrows; w += 8) {
        double v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = p[(int64_t)(w + u) * n + j];
#pragma unroll
        for (int u = 0; u < 8; ++u) s += v[u];
    }
    for (; w < nrows; ++w) s += p[(int64_t)w * n + j];
    return s;
}

// The candidate's totals, then the decision: the error is the cameras' in index order.
template <int NCMAX>
__global__ __launch_bounds__(256) void rig_joint_decide_kernel(RigJointArgs a, StereoBufs bf, int nwg) {
    __shared__ double serr[kRigMaxCams];
    if (bf.st->done) return;
    const RigJointDesc& d = a.d;
    const int cand = bf.st->cur ^ 1, tid = threadIdx.x;
    for (int j = tid; j < d.kTot; j += 256) {
        const double s = rig_joint_sum_rows(bf.partA[cand], nwg, d.kTot, j);
        bf.tot[cand][j] = s;
        if (j >= d.kErr) serr[j - d.kErr] = s;
    }
    __syncthreads();
    if (tid == 0) {
        double err = serr[0];
        for (int c = 1; c < d.nc; ++c) err += serr[c];
        rig_joint_decide(bf, cand, err, d.S);
    }
}

// Per view: Lc Lc^T = V + lam diag V; lane i of the view's wave substitutes right-hand sides i, i + 64 of the S + 1 (rows
// of E, then the view gradient) into LDS. Then thread t adds the pass's four views, in index order, to its resident
// entries t, t + 256, .. of (Z^T Z | Z^T z_g | failed); zero bands are multiplied like any other. A view with fewer than
// three points over all cameras, or with a pivot that is not positive, counts as failed. Workgroup w takes passes w,
// w + grid, ..: the order of every sum depends on M and the grid alone.
template <int NCMAX>
__global__ __launch_bounds__(256) void rig_joint_schur_kernel(RigJointArgs a, StereoBufs bf) {
    __shared__ double zs[kRjSchurViews][(kRjMaxS + 1) * 6];
    __shared__ double sfail[kRjSchurViews];
    const StereoState* st = bf.st;
    if (st->done) return;
    const RigJointDesc& d = a.d;
    const int S = d.S, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double acc[kRjAcc];
    int ab[kRjAcc];                                          // (a << 8 | b) of entry tid + 256 k; -1 the failed count; -2 none
#pragma unroll
    for (int kk = 0; kk < kRjAcc; ++kk) {
        acc[kk] = 0.0;
        const int e = tid + 256 * kk;
        int code = -2;
        if (e < d.kEg) { const int r = tri_row_big(e); code = r << 8 | (e - r * (r + 1) / 2); }
        else if (e < d.kFail) code = (e - d.kEg) << 8 | S;
        else if (e == d.kFail) code = -1;
        ab[kk] = code;
    }
    const double lam = st->lam;
    const int64_t passes = (bf.M + kRjSchurViews - 1) / kRjSchurViews;
    for (int64_t pass = blockIdx.x; pass < passes; pass += gridDim.x) {
        const int64_t view = pass * kRjSchurViews + wave;
        if (view < bf.M) {                                   // whole wave together
            const double* __restrict__ rec = bf.rec[st->cur] + view * d.kStride;
            int64_t n = 0;
            for (int c = 0; c < d.nc; ++c) n += a.cam[c].offs[view + 1] - a.cam[c].offs[view];
            double V[21], invd[6];
#pragma unroll
            for (int j = 0; j < 21; ++j) V[j] = rec[j];
            const bool failed = !cholesky6(V, lam, invd) || n < 3;
            for (int r = lane; r <= S; r += 64) {            // row r of E, or g_view (kGv = 21 + 6 S)
                double b[6], z[6];
#pragma unroll
                for (int m = 0; m < 6; ++m) b[m] = rec[kRjE0 + r * 6 + m];
                forward6(V, invd, b, z);
#pragma unroll
                for (int m = 0; m < 6; ++m) zs[wave][r * 6 + m] = z[m];
            }
            if (lane == 0) sfail[wave] = failed ? 1.0 : 0.0;
        } else {
            for (int j = lane; j < (S + 1) * 6; j += 64) zs[wave][j] = 0.0;
            if (lane == 0) sfail[wave] = 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < kRjAcc; ++kk) {
            const int code = ab[kk];
            if (code >= 0) {
                const int ra = code >> 8, rb = code & 255;
#pragma unroll
                for (int g = 0; g < kRjSchurViews; ++g) {
                    const double* za = &zs[g][ra * 6];
                    const double* zb = &zs[g][rb * 6];
                    double s = 0.0;
#pragma unroll
                    for (int m = 0; m < 6; ++m) s += za[m] * zb[m];
                    acc[kk] += s;
                }
            } else if (code == -1) {
#pragma unroll
                for (int g = 0; g < kRjSchurViews; ++g) acc[kk] += sfail[g];
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int kk = 0; kk < kRjAcc; ++kk) {
        const int e = tid + 256 * kk;
        if (e < d.kSchur) bf.partC[(int64_t)blockIdx.x * d.kSchur + e] = acc[kk];
    }
}

// A = B + lam diag B - sum Z^T Z, b = g_shared - sum E V^-1 g, edited by the fixed mask (a fixed row is the unit row with
// right-hand side 0, fixed columns are zero elsewhere), then delta_shared = A^-1 b. The lower triangle of A is packed row
// by row in LDS (entry (i, j) at i (i + 1) / 2 + j, the order of the Schur partial): a right-looking Cholesky by the
// whole workgroup, two barriers a column, then the two substitutions, one barrier a row. A failed view or a pivot that is
// not positive -- a free camera that sees nothing, for one -- ends the loop with CALIB_E_SINGULAR (-3).
template <int NCMAX>
__global__ __launch_bounds__(256) void rig_joint_solve_kernel(RigJointArgs a, StereoBufs bf, int nwg) {
    __shared__ double A[kRjMaxTri];
    __shared__ double y[kRjMaxS], z[kRjMaxS], invs[kRjMaxS];
    __shared__ int sbad;
    StereoState* st = bf.st;
    if (st->done) return;
    const RigJointDesc& d = a.d;
    const int S = d.S, tid = threadIdx.x;
    const double* __restrict__ tot = bf.tot[st->cur];
    const double lam = st->lam;
    if (tid == 0) sbad = 0;
    __syncthreads();
    for (int e = tid; e < d.kSchur; e += 256) {
        const double s = rig_joint_sum_rows(bf.partC, nwg, d.kSchur, e);
        if (e < d.kEg) {
            const int i = tri_row_big(e), j = e - i * (i + 1) / 2;
            int cI = 0;
            while (cI + 1 < d.nc && i >= d.off[cI + 1]) ++cI;                    // the camera of row i
            const double B = j >= d.off[cI] ? tot[d.bo[cI] + tri(i - d.off[cI], j - d.off[cI])] : 0.0;
            const double v = (i == j ? B + lam * B : B) - s;
            A[e] = (a.isFixed(i) || a.isFixed(j)) ? (i == j ? 1.0 : 0.0) : v;
        } else if (e < d.kFail) {
            const int i = e - d.kEg;
            y[i] = a.isFixed(i) ? 0.0 : tot[d.kG + i] - s;
        } else if (s != 0.0) {
            sbad = 1;
        }
    }
    bool ok = true;
    for (int j = 0; j < S; ++j) {
        __syncthreads();
        const double dj = A[tri(j, j)];
        if (!(dj > 0.0)) ok = false;
        const double inv = rsqrt_nr(dj);
        for (int i = j + 1 + tid; i < S; i += 256) A[tri(i, j)] *= inv;
        if (tid == 0) invs[j] = inv;
        __syncthreads();
        for (int i = j + 1 + (tid >> 4); i < S; i += 16) {
            const double lij = A[tri(i, j)];
            for (int kI = j + 1 + (tid & 15); kI <= i; kI += 16) A[tri(i, kI)] -= lij * A[tri(kI, j)];
        }
    }
    __syncthreads();
    if (sbad) ok = false;
    if (!ok) {                                               // the same for every thread
        if (tid == 0) stereo_stop(st, -3);
        return;
    }
    // forward: z_j = y_j / L_jj, y_i -= L_ij z_j (i > j)
    for (int j = 0; j < S; ++j) {
        const double zj = y[j] * invs[j];
        for (int i = j + 1 + tid; i < S; i += 256) y[i] -= A[tri(i, j)] * zj;
        if (tid == 0) z[j] = zj;
        __syncthreads();
    }
    // backward: x_j = z_j / L_jj, z_i -= L_ji x_j (i < j)
    for (int j = S - 1; j >= 0; --j) {
        const double xj = z[j] * invs[j];
        for (int i = tid; i < j; i += 256) z[i] -= A[tri(j, i)] * xj;
        if (tid == 0) a.dsh[j] = xj;
        __syncthreads();
    }
}

// stereo_backsub_kernel with a run-time S, the shared step and the mask from this solver's arguments
template <int NCMAX>
__global__ __launch_bounds__(64) void rig_joint_backsub_kernel(RigJointArgs a, StereoBufs bf) {
    const StereoState* st = bf.st;
    if (st->done) return;
    const int64_t view = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (view >= bf.M) return;
    const int S = a.d.S, cur = st->cur;
    const double* __restrict__ rec = bf.rec[cur] + view * a.d.kStride;
    const double* __restrict__ Pc = bf.P[cur];
    double* __restrict__ Pn = bf.P[cur ^ 1];
    double V[21], b[6], invd[6], z[6], dl[6];
#pragma unroll
    for (int j = 0; j < 21; ++j) V[j] = rec[j];
#pragma unroll
    for (int m = 0; m < 6; ++m) b[m] = rec[a.d.kGv + m];
    for (int s = 0; s < S; ++s) {
        const double ds = a.dsh[s];
#pragma unroll
        for (int m = 0; m < 6; ++m) b[m] -= rec[kRjE0 + s * 6 + m] * ds;
    }
    eliminate(V, b, st->lam, invd, z);
    backward6(V, invd, z, dl);
#pragma unroll
    for (int m = 0; m < 6; ++m) {
        const int64_t o = S + 6 * view + m;
        bf.delta[o] = dl[m];
        Pn[o] = Pc[o] + dl[m];
    }
    if (view == 0) {
        for (int s = 0; s < S; ++s) {
            const double ds = a.dsh[s];
            bf.delta[s] = ds;
            Pn[s] = a.isFixed(s) ? Pc[s] : Pc[s] + ds;      // copied, not added to: the bits stay (-0.0 + 0.0 is +0.0)
        }
    }
}

// ---- robust losses -----------------------------------------------------------------------------------------
// rig_joint_blocks_kernel on the problem re-weighted at the candidate: sum rho(|r_p|^2) instead of sum |r_p|^2, every
// point's rows and residual times sqrt(rho') (first order: Triggs' second-order term is left out). Same slab, tiles,
// parking, record and partial; the cameras' sums of rho stand where their errors stand, so the other four kernels of a
// round run unchanged. Huber or Cauchy is a run-time, launch-uniform value: the kernel exists once.
template <int NCMAX>
__global__ __launch_bounds__(64 * kRjWaves) void rig_joint_robust_blocks_kernel(RigJointArgs a, StereoBufs bf, RigLoss loss) {
    __shared__ __attribute__((aligned(16))) double2 smem[kRjWaves * kJSlab];
    __shared__ double park[kRjWaves][kRjPark];
    __shared__ double part[kRjWaves][kRjMaxTot];
    static_assert(NCMAX == kRigMaxCams, "the partial holds eight cameras' blocks");
    if (bf.st->done) return;
    const RigJointDesc& d = a.d;
    const int cand = bf.st->cur ^ 1;
    const double* __restrict__ Pq = bf.P[cand];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int k = lane >> 4, c16 = lane & 15;
    double2* slab = smem + wave * kJSlab;
    double* T = park[wave];
    double* mine = part[wave];
    const double2 zero2 = {0.0, 0.0};
    // chunks no pass stores (J1's pad columns) stay zero from here on; camera 0 leaves J1 as the last camera wrote it
    // and does not read it
    for (int j = lane; j < kJSlab; j += 64) slab[j] = zero2;
    for (int j = lane; j < d.kTot; j += 64) mine[j] = 0.0;
    // this lane's entry of (V | g_view): its row and column in T00, or its place in g0
    const int va = lane < 21 ? tri_row(lane) : 0, vb = lane < 21 ? lane - va * (va + 1) / 2 : 0;
    const int64_t stride = (int64_t)gridDim.x * kRjWaves;
    for (int64_t view = (int64_t)blockIdx.x * kRjWaves + wave; view < bf.M; view += stride) {     // wave-uniform
        double e[6], vc[kViewStride];
#pragma unroll
        for (int j = 0; j < 6; ++j) e[j] = Pq[d.S + 6 * view + j];
        pose_view_constants(e, vc);
        // one view per wave: the constants are the same in every lane and live in scalar registers
#pragma unroll
        for (int j = 0; j < kViewStride; ++j) vc[j] = readlane_d(vc[j], 0);
        double* __restrict__ rec = bf.rec[cand] + view * d.kStride;
        double vacc = 0.0;                                                       // lane j < 27: entry j of (V | g_view)
#pragma unroll 1
        for (int c = 0; c < d.nc; ++c) {                                         // one body for every camera
            const int L = d.L[c], off = d.off[c];
            RigJointTiles t;
            t.t00U = d4{0.0, 0.0, 0.0, 0.0};
            t.t00V = t.t00U; t.t10U = t.t00U; t.t10V = t.t00U; t.t11U = t.t00U; t.t11V = t.t00U;
            t.g0 = 0.0; t.g1 = 0.0; t.err = 0.0;
            if (c == 0) {
                if (d.model[0] == kRadtan) rig_joint_pass<kRadtan, false, true>(a.cam[0], Pq + off, view, lane, vc, vc, slab, t, loss.kind, loss.scale);
                else rig_joint_pass<kFisheye, false, true>(a.cam[0], Pq + off, view, lane, vc, vc, slab, t, loss.kind, loss.scale);
            } else {
                double rg[6], vr[kViewStride];
#pragma unroll
                for (int j = 0; j < 6; ++j) rg[j] = Pq[off + L + j];
                pose_view_constants(rg, vr);
#pragma unroll
                for (int j = 0; j < kViewStride; ++j) vr[j] = readlane_d(vr[j], 0);
                if (d.model[c] == kRadtan) rig_joint_pass<kRadtan, true, true>(a.cam[c], Pq + off, view, lane, vc, vr, slab, t, loss.kind, loss.scale);
                else rig_joint_pass<kFisheye, true, true>(a.cam[c], Pq + off, view, lane, vc, vr, slab, t, loss.kind, loss.scale);
            }
            // the sum of rho: every lane holds points of its own, all 64 in one fixed order
            t.err += __shfl_xor(t.err, 1, 64);  t.err += __shfl_xor(t.err, 2, 64);
            t.err += __shfl_xor(t.err, 4, 64);  t.err += __shfl_xor(t.err, 8, 64);
            // the four points of a group sit in the four 16-lane rows of the wave
            t.g0 += __shfl_xor(t.g0, 16, 64);   t.g0 += __shfl_xor(t.g0, 32, 64);
            t.g1 += __shfl_xor(t.g1, 16, 64);   t.g1 += __shfl_xor(t.g1, 32, 64);
            t.err += __shfl_xor(t.err, 16, 64); t.err += __shfl_xor(t.err, 32, 64);
            __builtin_amdgcn_wave_barrier();                                     // the last camera's readers are through
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int o = (k + 4 * reg) * 16 + c16;
                T[kRjT00 + o] = t.t00U[reg] + t.t00V[reg];
                T[kRjT10 + o] = t.t10U[reg] + t.t10V[reg];
                T[kRjT11 + o] = t.t11U[reg] + t.t11V[reg];
            }
            if (k == 0) { T[kRjG0 + c16] = t.g0; T[kRjG1 + c16] = t.g1; }
            if (lane == 0) T[kRjE] = t.err;
            __builtin_amdgcn_wave_barrier();
            // V and g_view over the cameras in index order
            if (lane < 21) vacc += T[kRjT00 + va * 16 + vb];
            else if (lane < 27) vacc += T[kRjG0 + lane - 21];
            // the camera's band of E (a camera without points in the view: exact zeros)
            const int W = d.width(c);
            for (int j = lane; j < 6 * W; j += 64) {
                const int s = j / 6, v = j - 6 * s;
                rec[kRjE0 + (off + s) * 6 + v] = s < L ? T[kRjT00 + (6 + s) * 16 + v] : T[kRjT10 + (s - L) * 16 + v];
            }
            // its B block, g and error into the wave's resident partial: the wave's views in index order
            const int nb = W * (W + 1) / 2;
            for (int eI = lane; eI < nb; eI += 64) {
                const int i = tri_row(eI), j = eI - i * (i + 1) / 2;
                mine[d.bo[c] + eI] += i < L ? T[kRjT00 + (6 + i) * 16 + 6 + j]
                                            : j < L ? T[kRjT10 + (i - L) * 16 + 6 + j] : T[kRjT11 + (i - L) * 16 + (j - L)];
            }
            if (lane < W) mine[d.kG + off + lane] += lane < L ? T[kRjG0 + 6 + lane] : T[kRjG1 + lane - L];
            if (lane == 0) mine[d.kErr + c] += T[kRjE];
        }
        if (lane < 21) rec[lane] = vacc;
        else if (lane < 27) rec[d.kGv + lane - 21] = vacc;
    }
    __syncthreads();
    // the workgroup's waves in index order
    for (int eI = threadIdx.x; eI < d.kTot; eI += 64 * kRjWaves) {
        double s = part[0][eI];
#pragma unroll
        for (int w = 1; w < kRjWaves; ++w) s += part[w][eI];
        bf.partA[cand][(int64_t)blockIdx.x * d.kTot + eI] = s;
    }
}

// one camera's points of one view: sensor - projection into res (the camera's own rows)
template <int MODEL, bool RIG>
__device__ __forceinline__ void rig_residuals_pass(const StereoCam& cm, const double* __restrict__ shared, int64_t view, int lane,
                                                   const double (&vc)[kViewStride], const double (&vr)[kViewStride],
                                                   double2* __restrict__ res) {
    Shared<MODEL, double> sp;
    sp.load(shared);
    const int64_t p0 = cm.offs[view];
    const int n = (int)(cm.offs[view + 1] - p0);
    for (int q = lane; q < n; q += 64) {
        const int64_t p = p0 + q;
        const double2 m = cm.uv[p];
        const double* X = cm.xyz + 3 * p;
        double u, v;
        if constexpr (RIG) {
            const double qx = vc[0] * X[0] + vc[1] * X[1] + vc[2] * X[2];       // R_i X
            const double qy = vc[3] * X[0] + vc[4] * X[1] + vc[5] * X[2];
            const double qz = vc[6] * X[0] + vc[7] * X[1] + vc[8] * X[2];
            project_point<MODEL, double>(sp, vr, qx + vc[9], qy + vc[10], qz + vc[11], u, v);
        } else {
            project_point<MODEL, double>(sp, vc, X[0], X[1], X[2], u, v);
        }
        res[p] = double2{m.x - u, m.y - v};
    }
}

// Every point's residual at Pq, one wave per view, the cameras in index order: out holds camera 0's n_0 rows, then camera
// 1's, .. (2 doubles a point, nothing else). Four waves per workgroup; the grid's waves loop over the views.
constexpr int kRjResidualWaves = 4, kRjResidualGrid = 1024;
template <int NCMAX>
__global__ __launch_bounds__(64 * kRjResidualWaves) void rig_residuals_kernel(RigJointArgs a, const double* __restrict__ Pq,
                                                                               int64_t M, double2* __restrict__ out) {
    const RigJointDesc& d = a.d;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t stride = (int64_t)gridDim.x * kRjResidualWaves;
    for (int64_t view = (int64_t)blockIdx.x * kRjResidualWaves + wave; view < M; view += stride) {     // wave-uniform
        double e[6], vc[kViewStride];
#pragma unroll
        for (int j = 0; j < 6; ++j) e[j] = Pq[d.S + 6 * view + j];
        pose_view_constants(e, vc);
#pragma unroll
        for (int j = 0; j < kViewStride; ++j) vc[j] = readlane_d(vc[j], 0);
        double2* res = out;
#pragma unroll 1
        for (int c = 0; c < d.nc; ++c) {
            const int L = d.L[c], off = d.off[c];
            if (c == 0) {
                if (d.model[0] == kRadtan) rig_residuals_pass<kRadtan, false>(a.cam[0], Pq + off, view, lane, vc, vc, res);
                else rig_residuals_pass<kFisheye, false>(a.cam[0], Pq + off, view, lane, vc, vc, res);
            } else {
                double rg[6], vr[kViewStride];
#pragma unroll
                for (int j = 0; j < 6; ++j) rg[j] = Pq[off + L + j];
                pose_view_constants(rg, vr);
#pragma unroll
                for (int j = 0; j < kViewStride; ++j) vr[j] = readlane_d(vr[j], 0);
                if (d.model[c] == kRadtan) rig_residuals_pass<kRadtan, true>(a.cam[c], Pq + off, view, lane, vc, vr, res);
                else rig_residuals_pass<kFisheye, true>(a.cam[c], Pq + off, view, lane, vc, vr, res);
            }
            res += a.cam[c].offs[M];                                             // the camera's points over all views
        }
    }
}

}  // namespace calib
