// Joint stereo calibration: both cameras, the rig and the board poses in one problem (device code, gfx950).
//
// Unknowns Pj = (shared_a[LA], shared_b[LB], rig[6], pose_0[6], .., pose_{M-1}[6]); the shared vectors in the order of P,
// every 6-tuple Euler angles in DEGREES then t (pose_view_constants). Residuals and correspondences are those of
// stereo.hpp. The S = LA + LB + 6 <= 26 leading unknowns are shared by all views, so the normal equations keep the
// block-arrow shape: B (S x S), E_i (S x 6), V_i (6 x 6). A camera-a row is jacobian_point<MODEL_A> at (pose_i, X) as it
// comes; a camera-b row is jacobian_point<MODEL_B> at (rig, Xa): its shared columns are d/d shared_b, its six view
// columns d/d rig, and the columns of pose_i are G R_rig [dXa/drho_i | I] as in stereo_blocks_kernel. No row touches
// both shared_a and (shared_b, rig): that block of B is zero and has no slot anywhere below.
//
// One LM round (src/calibrate.py:143-171) is five launches, every sum in one fixed order, no floating-point atomics:
//   stereo_joint_blocks_kernel   one wave per view, four views per workgroup, at the CANDIDATE: the view's rows go
//                                through the wave's LDS slab into v_mfma_f64_16x16x4_f64 tiles -> the view's record
//                                (V, E, g_view) and the workgroup's partial of B_aa, B_(b,rig)(b,rig), g_shared, errors
//   stereo_joint_decide_kernel   one workgroup: the partials in one order, then accept / lambda / stop (round 0: bootstrap)
//   stereo_joint_schur_kernel    16 lanes per view at the ACCEPTED point: Z = Lc^-1 E_i^T (6 x S) and Lc^-1 g_i with
//                                eliminate(); the workgroup's 16 views' Z^T Z and Z^T z_g summed in view order -> partial
//   stereo_joint_solve_kernel    one workgroup: partials in one order, B + lam diag B - sum, the fixed mask, Cholesky of
//                                the S x S system in one wave's registers, substitution -> delta_shared
//   stereo_backsub_kernel        one lane per view: delta_i, the next candidate, the step (stereo_loop.hpp's, on
//                                JointLayout's record with this S)
// The buffers, the state, the decision, the end of the loop and the sum of the partials are stereo_loop.hpp's, shared
// with the rig-only solver. All kernels are templates: they are emitted where they are first launched, at the end of
// the module.
//
// Tile maps (C/D layout of the fp64 MFMA: lane (k, c) = (lane >> 4, lane & 15) holds rows k + 4 reg of column c):
//   camera a   columns [view 6 | shared_a | pad]                     Ta  = J^T J
//   camera b   J0 = [view 6 | shared_b | pad], J1 = [rig 6 | pad]    T00 = J0^T J0, T10 = J1^T J0, T11 = J1^T J1
//   V = Ta[0:6, 0:6] + T00[0:6, 0:6];  E rows: shared_a Ta[6 + s][v], shared_b T00[6 + s][v], rig T10[r][v]
//   B_aa = Ta[6 + i][6 + j];  B_bb = T00[6 + i][6 + j];  B_rig,b = T10[r][6 + j];  B_rig,rig = T11[r][r']
#pragma once
#include "stereo.hpp"

namespace calib {

constexpr int kJRowChunks = 33;                    // 32 columns (J0 | J1) + 1 chunk: odd => conflict-free 16-byte accesses;
constexpr int kJResChunk = 32;                     // the odd chunk carries the point's residual
constexpr int kJRows = 32;                         // points transposed per pass: two passes per 64-point batch
constexpr int kJSlab = kJRows * kJRowChunks;       // chunks (double2) per wave: 16.5 KiB
constexpr int kJWaves = 4;                         // views per workgroup
constexpr int kJRecord = 184;                      // doubles per view record (21 + 6 * 26 + 6 = 183 used at most)
// a wave's parked results (doubles, in its dead slab): four 16 x 16 tiles, three J^T r vectors, two errors
constexpr int kJTa = 0, kJT00 = 256, kJT10 = 512, kJT11 = 768, kJGa = 1024, kJGb0 = 1040, kJGb1 = 1056, kJErr = 1072;
static_assert(kJErr + 2 <= 2 * kJSlab, "the parked results must fit the wave's slab");

template <int LA, int LB>
struct JointLayout {
    static constexpr int S = LA + LB + 6, LR = LB + 6;
    // view record: V lower triangle, E row-major (shared row, view column), g_view
    static constexpr int kV = 0, kE = 21, kGv = 21 + 6 * S, kRec = kGv + 6, kStride = kJRecord;
    // what is summed over the views: lower triangles of B_aa and of B over (b, rig), g_shared, sse_a, sse_b
    static constexpr int kBa = 0, kBr = LA * (LA + 1) / 2, kG = kBr + LR * (LR + 1) / 2, kErr = kG + S, kTot = kErr + 2;
    // Schur partial: lower triangle of sum Z^T Z (S x S), sum E V^-1 g (S), number of failed views
    static constexpr int kZZ = 0, kEg = S * (S + 1) / 2, kFail = kEg + S, kSchur = kFail + 1;
    static_assert(kRec <= kJRecord && S <= kJMaxS, "record stride");
    // slot of B(i, j), i >= j in the order (a, b, rig), among the summed entries; -1: the zero block
    static __host__ __device__ constexpr int slotB(int i, int j) {
        return i < LA ? kBa + i * (i + 1) / 2 + j : (j >= LA ? kBr + (i - LA) * (i - LA + 1) / 2 + (j - LA) : -1);
    }
};
constexpr int kJMaxTot = 219, kJMaxSchur = 378;    // JointLayout<10, 10>

// row of entry e of a lower triangle stored row by row
__device__ __forceinline__ int tri_row(int e) {
    int i = 0;
    while ((i + 1) * (i + 2) / 2 <= e) ++i;
    return i;
}

// a row of a batch's tail lane is stored as exact zeros (selected per component: a select of the pair goes through memory)
__device__ __forceinline__ double2 live_or_zero(bool live, double2 v) {
    double2 o;
    o.x = live ? v.x : 0.0;
    o.y = live ? v.y : 0.0;
    return o;
}

// entry j of a view's record / entry e of the workgroup partial, from one wave's parked results
template <int LA, int LB>
__device__ __forceinline__ double joint_record_entry(const double* __restrict__ T, int j) {
    using Y = JointLayout<LA, LB>;
    if (j < Y::kE) {
        const int a = tri_row(j), b = j - a * (a + 1) / 2;
        return T[kJTa + a * 16 + b] + T[kJT00 + a * 16 + b];
    }
    if (j < Y::kGv) {
        const int s = (j - Y::kE) / 6, v = (j - Y::kE) % 6;
        return s < LA ? T[kJTa + (6 + s) * 16 + v]
                      : s < LA + LB ? T[kJT00 + (6 + s - LA) * 16 + v] : T[kJT10 + (s - LA - LB) * 16 + v];
    }
    return T[kJGa + j - Y::kGv] + T[kJGb0 + j - Y::kGv];
}
template <int LA, int LB>
__device__ __forceinline__ double joint_partial_entry(const double* __restrict__ T, int e) {
    using Y = JointLayout<LA, LB>;
    if (e < Y::kBr) {
        const int i = tri_row(e), j = e - i * (i + 1) / 2;
        return T[kJTa + (6 + i) * 16 + 6 + j];
    }
    if (e < Y::kG) {
        const int i = tri_row(e - Y::kBr), j = e - Y::kBr - i * (i + 1) / 2;
        return i < LB ? T[kJT00 + (6 + i) * 16 + 6 + j]
                      : j < LB ? T[kJT10 + (i - LB) * 16 + 6 + j] : T[kJT11 + (i - LB) * 16 + (j - LB)];
    }
    if (e < Y::kErr) {
        const int s = e - Y::kG;
        return s < LA ? T[kJGa + 6 + s] : s < LA + LB ? T[kJGb0 + 6 + s - LA] : T[kJGb1 + s - LA - LB];
    }
    return T[kJErr + e - Y::kErr];
}

template <int MODEL_A, int MODEL_B>
__global__ __launch_bounds__(64 * kJWaves) void stereo_joint_blocks_kernel(StereoCam ca, StereoCam cb, StereoBufs bf) {
    constexpr int LA = ModelTraits<MODEL_A>::L, CA = ModelTraits<MODEL_A>::C;
    constexpr int LB = ModelTraits<MODEL_B>::L, CB = ModelTraits<MODEL_B>::C;
    using Y = JointLayout<LA, LB>;
    __shared__ __attribute__((aligned(16))) double2 smem[kJWaves * kJSlab];
    if (bf.st->done) return;
    const int cand = bf.st->cur ^ 1;
    const double* __restrict__ Pj = bf.P[cand];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int k = lane >> 4, c = lane & 15;
    const int64_t view = (int64_t)blockIdx.x * kJWaves + wave;
    double2* slab = smem + wave * kJSlab;
    const double2 zero2 = {0.0, 0.0};
    // chunks no pass stores (J1's pad columns) stay zero from here on
    for (int j = lane; j < kJSlab; j += 64) slab[j] = zero2;
    d4 aU = {0.0, 0.0, 0.0, 0.0}, aV = aU, b00U = aU, b00V = aU, b10U = aU, b10V = aU, b11U = aU, b11V = aU;
    double ga = 0.0, gb0 = 0.0, gb1 = 0.0, ea = 0.0, eb = 0.0;
    double2* const myRow = slab + (lane & (kJRows - 1)) * kJRowChunks;           // the row this lane stores in its pass
    const double2* const src = slab + k * kJRowChunks + c;                       // rows 4 s + k: + 4 rows per group
    if (view < bf.M) {                           // wave-uniform
        double e[6], rg[6], vc[kViewStride], vr[kViewStride];
#pragma unroll
        for (int j = 0; j < 6; ++j) { rg[j] = Pj[LA + LB + j]; e[j] = Pj[Y::S + 6 * view + j]; }
        pose_view_constants(e, vc);
        pose_view_constants(rg, vr);
        // one view per wave: the constants are the same in every lane and live in scalar registers
#pragma unroll
        for (int j = 0; j < kViewStride; ++j) { vc[j] = readlane_d(vc[j], 0); vr[j] = readlane_d(vr[j], 0); }
        {
            Shared<MODEL_A, double> sp;
            sp.load(Pj);
            const int64_t p0 = ca.offs[view];
            const int n = (int)(ca.offs[view + 1] - p0);
            for (int q0 = 0; q0 < n; q0 += 64) {                                 // an empty side: zero trips
                const int q = q0 + lane;
                const bool live = q < n;
                const int64_t p = p0 + (live ? q : n - 1);                       // tail lanes: a clamped point, zeroed below
                const double2 m = ca.uv[p];
                const double* X = ca.xyz + 3 * p;
                double u, v;
                double2 J[CA];
                jacobian_point<MODEL_A, double>(sp, vc, X[0], X[1], X[2], u, v, J);
                double2 res;
                res.x = live ? m.x - u : 0.0;
                res.y = live ? m.y - v : 0.0;
#pragma unroll
                for (int half = 0; half < 2; ++half) {
                    if (q0 + kJRows * half >= n) break;                          // wave-uniform
                    __builtin_amdgcn_wave_barrier();
                    if ((lane >> 5) == half) {
#pragma unroll
                        for (int cc = 0; cc < 16; ++cc) {
                            const double2 col = cc < 6 ? J[LA + cc] : (cc < 6 + LA ? J[cc < 6 + LA ? cc - 6 : 0] : zero2);
                            myRow[cc] = live_or_zero(live, col);
                        }
                        myRow[kJResChunk] = res;
                    }
                    __builtin_amdgcn_wave_barrier();
                    const int rows = min(kJRows, n - (q0 + kJRows * half));
                    const int ng = (rows + 3) >> 2;                              // rows past the end of the last group are zeros
                    for (int s = 0; s < ng; ++s) {
                        const double2 ja = src[s * 4 * kJRowChunks];
                        const double2 rr = slab[(4 * s + k) * kJRowChunks + kJResChunk];
                        aU = __builtin_amdgcn_mfma_f64_16x16x4f64(ja.x, ja.x, aU, 0, 0, 0);
                        aV = __builtin_amdgcn_mfma_f64_16x16x4f64(ja.y, ja.y, aV, 0, 0, 0);
                        ga += ja.x * rr.x + ja.y * rr.y;
                        ea += rr.x * rr.x + rr.y * rr.y;
                    }
                }
            }
        }
        {
            Shared<MODEL_B, double> sp;
            sp.load(Pj + LA);
            const int64_t p0 = cb.offs[view];
            const int n = (int)(cb.offs[view + 1] - p0);
            for (int q0 = 0; q0 < n; q0 += 64) {
                const int q = q0 + lane;
                const bool live = q < n;
                const int64_t p = p0 + (live ? q : n - 1);
                const double2 m = cb.uv[p];
                const double* X = cb.xyz + 3 * p;
                const double qx = vc[0] * X[0] + vc[1] * X[1] + vc[2] * X[2];   // R_i X
                const double qy = vc[3] * X[0] + vc[4] * X[1] + vc[5] * X[2];
                const double qz = vc[6] * X[0] + vc[7] * X[1] + vc[8] * X[2];
                double u, v;
                double2 J[CB];
                jacobian_point<MODEL_B, double>(sp, vr, qx + vc[9], qy + vc[10], qz + vc[11], u, v, J);
                double2 res;
                res.x = live ? m.x - u : 0.0;
                res.y = live ? m.y - v : 0.0;
                // stereo_blocks_kernel's chain rule, written out here as there: moved into a function the two kernels
                // share, the compiler contracts Jv[1] the other way round here (bits change) and reschedules that kernel
                // G R_rig (2 x 3), G = d(uv)/dXb = the translation columns
                double2 GR[3];
#pragma unroll
                for (int t = 0; t < 3; ++t) {
                    GR[t].x = J[LB + 3].x * vr[t] + J[LB + 4].x * vr[3 + t] + J[LB + 5].x * vr[6 + t];
                    GR[t].y = J[LB + 3].y * vr[t] + J[LB + 4].y * vr[3 + t] + J[LB + 5].y * vr[6 + t];
                }
                // dXa/drho_i = (pi/180) a. x q (jacobian_stage_b), dXa/dt_i = I
                const double ax0 = vc[12], ax1 = vc[13], ax2 = vc[14], ay0 = vc[15], ay1 = vc[16];
                const double deg = 0.017453292519943295;
                const double dx[3] = {ax1 * qz - ax2 * qy, ax2 * qx - ax0 * qz, ax0 * qy - ax1 * qx};
                const double dy[3] = {ay1 * qz, -ay0 * qz, ay0 * qy - ay1 * qx};
                const double dz[3] = {-deg * qy, deg * qx, 0.0};
                double2 Jv[6];
                Jv[0].x = GR[0].x * dx[0] + GR[1].x * dx[1] + GR[2].x * dx[2];
                Jv[0].y = GR[0].y * dx[0] + GR[1].y * dx[1] + GR[2].y * dx[2];
                Jv[1].x = GR[0].x * dy[0] + GR[1].x * dy[1] + GR[2].x * dy[2];
                Jv[1].y = GR[0].y * dy[0] + GR[1].y * dy[1] + GR[2].y * dy[2];
                Jv[2].x = GR[0].x * dz[0] + GR[1].x * dz[1];
                Jv[2].y = GR[0].y * dz[0] + GR[1].y * dz[1];
                Jv[3] = GR[0]; Jv[4] = GR[1]; Jv[5] = GR[2];
#pragma unroll
                for (int half = 0; half < 2; ++half) {
                    if (q0 + kJRows * half >= n) break;                          // wave-uniform
                    __builtin_amdgcn_wave_barrier();
                    if ((lane >> 5) == half) {
#pragma unroll
                        for (int cc = 0; cc < 16; ++cc) {
                            const double2 col = cc < 6 ? Jv[cc < 6 ? cc : 0] : (cc < 6 + LB ? J[cc < 6 + LB ? cc - 6 : 0] : zero2);
                            myRow[cc] = live_or_zero(live, col);
                        }
#pragma unroll
                        for (int cc = 0; cc < 6; ++cc) myRow[16 + cc] = live_or_zero(live, J[LB + cc]);
                        myRow[kJResChunk] = res;
                    }
                    __builtin_amdgcn_wave_barrier();
                    const int rows = min(kJRows, n - (q0 + kJRows * half));
                    const int ng = (rows + 3) >> 2;
                    for (int s = 0; s < ng; ++s) {
                        const double2 j0 = src[s * 4 * kJRowChunks];
                        const double2 j1 = src[s * 4 * kJRowChunks + 16];
                        const double2 rr = slab[(4 * s + k) * kJRowChunks + kJResChunk];
                        b00U = __builtin_amdgcn_mfma_f64_16x16x4f64(j0.x, j0.x, b00U, 0, 0, 0);
                        b00V = __builtin_amdgcn_mfma_f64_16x16x4f64(j0.y, j0.y, b00V, 0, 0, 0);
                        b10U = __builtin_amdgcn_mfma_f64_16x16x4f64(j1.x, j0.x, b10U, 0, 0, 0);
                        b10V = __builtin_amdgcn_mfma_f64_16x16x4f64(j1.y, j0.y, b10V, 0, 0, 0);
                        b11U = __builtin_amdgcn_mfma_f64_16x16x4f64(j1.x, j1.x, b11U, 0, 0, 0);
                        b11V = __builtin_amdgcn_mfma_f64_16x16x4f64(j1.y, j1.y, b11V, 0, 0, 0);
                        gb0 += j0.x * rr.x + j0.y * rr.y;
                        gb1 += j1.x * rr.x + j1.y * rr.y;
                        eb += rr.x * rr.x + rr.y * rr.y;
                    }
                }
            }
        }
    }
    // the four points of a group sit in the four 16-lane rows of the wave
    ga += __shfl_xor(ga, 16, 64);   ga += __shfl_xor(ga, 32, 64);
    gb0 += __shfl_xor(gb0, 16, 64); gb0 += __shfl_xor(gb0, 32, 64);
    gb1 += __shfl_xor(gb1, 16, 64); gb1 += __shfl_xor(gb1, 32, 64);
    ea += __shfl_xor(ea, 16, 64);   ea += __shfl_xor(ea, 32, 64);
    eb += __shfl_xor(eb, 16, 64);   eb += __shfl_xor(eb, 32, 64);
    // every wave parks its results in its dead slab (zeros for a wave without a view)
    double* T = reinterpret_cast<double*>(slab);
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
        const int o = (k + 4 * reg) * 16 + c;
        T[kJTa + o] = aU[reg] + aV[reg];
        T[kJT00 + o] = b00U[reg] + b00V[reg];
        T[kJT10 + o] = b10U[reg] + b10V[reg];
        T[kJT11 + o] = b11U[reg] + b11V[reg];
    }
    if (k == 0) { T[kJGa + c] = ga; T[kJGb0 + c] = gb0; T[kJGb1 + c] = gb1; }
    if (lane == 0) { T[kJErr] = ea; T[kJErr + 1] = eb; }
    __syncthreads();
    if (view < bf.M) {
        double* __restrict__ rec = bf.rec[cand] + view * kJRecord;
        for (int j = lane; j < Y::kRec; j += 64) rec[j] = joint_record_entry<LA, LB>(T, j);
    }
    // the workgroup's four views in index order
    const double* T0 = reinterpret_cast<const double*>(smem);
    for (int e = threadIdx.x; e < Y::kTot; e += 64 * kJWaves) {
        double s = joint_partial_entry<LA, LB>(T0, e);
#pragma unroll
        for (int w = 1; w < kJWaves; ++w) s += joint_partial_entry<LA, LB>(T0 + w * 2 * kJSlab, e);
        bf.partA[cand][(int64_t)blockIdx.x * Y::kTot + e] = s;
    }
}

// The candidate's totals, then the decision (stereo_decide, with S trace columns).
template <int LA, int LB>
__global__ __launch_bounds__(256) void stereo_joint_decide_kernel(StereoBufs bf, int nwg) {
    using Y = JointLayout<LA, LB>;
    __shared__ double sh[4][kJMaxTot + 1];
    if (bf.st->done) return;
    const int cand = bf.st->cur ^ 1, tid = threadIdx.x;
    joint_sum_partials<Y::kTot>(bf.partA[cand], nwg, sh);
    if (tid < Y::kTot) bf.tot[cand][tid] = joint_total(sh, tid);
    if (tid == 0) stereo_decide<Y::S>(bf, cand, joint_total(sh, Y::kErr) + joint_total(sh, Y::kErr + 1));
}

// Per view: Lc Lc^T = V + lam diag V; lane i substitutes right-hand sides i and i + 16 of the S + 1 (rows of E, then the
// view gradient) into the workgroup's LDS; then entry e of (Z^T Z | Z^T z_g) is summed over the 16 views in index order by
// thread e, e + 256. A view with fewer than three points in total, or with a pivot that is not positive, counts as failed.
template <int LA, int LB>
__global__ __launch_bounds__(256) void stereo_joint_schur_kernel(StereoCam ca, StereoCam cb, StereoBufs bf) {
    using Y = JointLayout<LA, LB>;
    constexpr int S = Y::S, ZS = (S + 1) * 6;
    __shared__ double zs[16][ZS];
    __shared__ double sfail[16];
    const StereoState* st = bf.st;
    if (st->done) return;
    const int tid = threadIdx.x, i = tid & 15, grp = tid >> 4;
    const int64_t view = (int64_t)blockIdx.x * 16 + grp;
    bool failed = false;
    double z[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, z2[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const int r2 = i + 16;
    if (view < bf.M) {                         // whole 16-lane group together
        const double* __restrict__ rec = bf.rec[st->cur] + view * kJRecord;
        const int64_t n = (ca.offs[view + 1] - ca.offs[view]) + (cb.offs[view + 1] - cb.offs[view]);
        double V[21], b[6], invd[6];
#pragma unroll
        for (int j = 0; j < 21; ++j) V[j] = rec[Y::kV + j];
#pragma unroll
        for (int m = 0; m < 6; ++m) b[m] = rec[Y::kE + i * 6 + m];               // S >= 16: row i of E
        failed = !eliminate(V, b, st->lam, invd, z) || n < 3;
        if (r2 <= S) {                                                           // row r2 of E, or g_view (kGv = kE + 6 S)
#pragma unroll
            for (int m = 0; m < 6; ++m) b[m] = rec[Y::kE + r2 * 6 + m];
            forward6(V, invd, b, z2);
        }
    }
#pragma unroll
    for (int m = 0; m < 6; ++m) zs[grp][i * 6 + m] = z[m];
    if (r2 <= S) {
#pragma unroll
        for (int m = 0; m < 6; ++m) zs[grp][r2 * 6 + m] = z2[m];
    }
    if (i == 0) sfail[grp] = failed ? 1.0 : 0.0;
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

// A = B + lam diag B - sum Z^T Z, b = g_shared - sum E V^-1 g, edited by the fixed mask (a fixed row is the unit row with
// right-hand side 0, fixed columns are zero elsewhere), then delta_shared = A^-1 b: Cholesky in the registers of wave 0,
// lane i holding row i, pivots and multipliers passed by v_readlane. A failed view or a pivot that is not positive ends
// the loop with CALIB_E_SINGULAR (-3).
template <int LA, int LB>
__global__ __launch_bounds__(256) void stereo_joint_solve_kernel(StereoBufs bf, int nwg) {
    using Y = JointLayout<LA, LB>;
    constexpr int S = Y::S;
    __shared__ double sh[4][kJMaxSchur + 1];
    __shared__ double Lsh[S][S + 1];
    StereoState* st = bf.st;
    if (st->done) return;
    const int tid = threadIdx.x;
    joint_sum_partials<Y::kSchur>(bf.partC, nwg, sh);
    if (tid >= 64) return;
    const int i = tid < S ? tid : S - 1;                     // lanes past S repeat the last row; nothing reads them
    const double* __restrict__ tot = bf.tot[st->cur];
    const double lam = st->lam;
    const unsigned long long fixed = st->fixed;
    const bool fi = (fixed >> i) & 1;
    double row[S];
#pragma unroll
    for (int cI = 0; cI < S; ++cI) {
        const int hi = i > cI ? i : cI, lo = i > cI ? cI : i;
        const int slot = Y::slotB(hi, lo);
        const double B = slot >= 0 ? tot[slot >= 0 ? slot : 0] : 0.0;
        const double a = (cI == i ? B + lam * B : B) - joint_total(sh, Y::kZZ + hi * (hi + 1) / 2 + lo);
        row[cI] = (fi || ((fixed >> cI) & 1)) ? (cI == i ? 1.0 : 0.0) : a;
    }
    double y = fi ? 0.0 : tot[Y::kG + i] - joint_total(sh, Y::kEg + i);
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
