/*
 * calib_lm.h -- C-ABI of the MI355X (gfx950) Levenberg-Marquardt refinement engine.
 *
 * Drop-in boundary for the nonlinear stage of pvphan/camera-calibration. The
 * reference has no FFI layer; its seam is the duck-typed Python surface of
 *   Calibrator.refineCalibrationParameters   src/calibrate.py:117-171
 *   ProjectionJacobian.compute               src/jacobian.py:48-85
 *   Calibrator.projectAllPoints              src/calibrate.py:190-197
 *   Calibrator._computeReprojectionError     src/calibrate.py:178-188
 *   DistortionModel.projectWithDistortion    src/distortion.py:42-59
 * The Python host in camera-calibration_amd/ binds these entry points with
 * ctypes (INTEGRATION.md shows the stub a maintainer adds to src/calibrate.py).
 *
 * Conventions
 *  - Every function returns 0 on success, <0 on error (CALIB_E_*);
 *    calib_last_error() returns a thread-local message. No C++ exception
 *    crosses the boundary.
 *  - All pointer arguments are caller-owned HOST memory unless the name ends
 *    in _dev. The library owns all device memory of a handle.
 *  - One handle = one GPU = one host thread (one process per GPU; shards of a
 *    multi-GPU job are separate handles in separate processes). Every entry point that takes a handle makes
 *    the handle's device the calling thread's current HIP device (hipSetDevice) and leaves it so.
 *  - Parameter vector P (fp64, length K = L + 6*M), exactly the reference's
 *    (src/calibrate.py:199-229):
 *      P = (alpha, beta, gamma, uc, vc, k[0..|k|),  then per view i:
 *           rho_x, rho_y, rho_z [DEGREES], t_x, t_y, t_z)
 *    L = 10 radial-tangential (k1,k2,p1,p2,k3), 9 fisheye (k1..k4).
 *  - Views are a CSR over points: view i owns points [view_offsets[i], view_offsets[i+1]).
 */
#ifndef CALIB_LM_H
#define CALIB_LM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct calib_handle_s* calib_handle_t;

enum { CALIB_MODEL_RADTAN = 0, CALIB_MODEL_FISHEYE = 1 };   /* src/main.py:28-33 */
enum { CALIB_DTYPE_F64 = 0, CALIB_DTYPE_F32 = 1 };          /* storage/eval type of points, J, r;
                                                               normal equations + solve are always fp64 */
enum {
    CALIB_OK = 0,
    CALIB_E_INVALID = -1,   /* bad argument / shape (reference: ValueError, src/mathutils.py:102-105) */
    CALIB_E_HIP = -2,       /* HIP runtime error, no device, kernel failure */
    CALIB_E_SINGULAR = -3,  /* damped normal equations singular (reference: numpy LinAlgError, src/calibrate.py:152) */
    CALIB_E_STATE = -4      /* call sequence error (e.g. lm_local before lm_begin) */
};

/* trace row written per LM iteration (backs shouldPrint, src/calibrate.py:158-159,269-274):
 *   [0] iter  [1] err(P) [2] err(P+delta) [3] lambda used  [4] accepted (0/1)
 *   [5 .. 5+L) the shared parameters of P before the update                       */
#define CALIB_TRACE_HEADER 5

int         calib_version(void);
const char* calib_last_error(void);
int         calib_device_count(int* out_count);

int calib_create(int model, int dtype, int device_id, calib_handle_t* out_handle);
int calib_destroy(calib_handle_t h);

/* Launch all work of this handle on an existing HIP stream (e.g. the stream a
 * torch.distributed all-reduce is ordered against). use_own != 0: back to the handle's own
 * (non-blocking) stream; otherwise hip_stream is used as given, NULL being the HIP default
 * stream (which is what torch.cuda.current_stream().cuda_stream is unless the caller changed it). */
int calib_set_stream(calib_handle_t h, void* hip_stream, int use_own);
/* Wait until everything enqueued on the handle's stream has run (hipStreamSynchronize); an asynchronous fault of an
 * earlier launch is reported here with the names of the kernels enqueued since the last successful wait. */
int calib_synchronize(calib_handle_t h);

/* Upload the correspondences once (replaces getSensorPoints' vstack, src/calibrate.py:277-282).
 * sensor_uv: (MN,2) row-major as numpy, may be NULL (projection-only use);
 * model_xyz: (MN,3) row-major. Packs to SoA on the device. */
int calib_set_problem(calib_handle_t h, int64_t num_views, const int64_t* view_offsets,
                      const double* sensor_uv, const double* model_xyz);
/* The same upload from PER-VIEW arrays, as the reference's callers hold them -- allDetections is a list of
 * (sensorPoints (N_i,2), modelPoints (N_i,3)) pairs (src/calibrate.py:117-118) that getSensorPoints stacks with np.vstack on
 * every call (src/calibrate.py:277-282). sensor_uv_views[i] / model_xyz_views[i] point at view i's C-contiguous rows
 * (view_offsets[i+1] - view_offsets[i] of them; NULL allowed for an empty view; sensor_uv_views itself may be NULL).
 * Nothing is stacked on the host: the staged upload gathers from the views straight into its pinned buffers. */
int calib_set_problem_views(calib_handle_t h, int64_t num_views, const int64_t* view_offsets,
                            const double* const* sensor_uv_views, const double* const* model_xyz_views);

/* How an LM round forms the per-view normal equations:
 *   CALIB_LM_FUSED       one kernel evaluates the 2 x C Jacobian blocks and contracts them with
 *                        MFMA without writing them to HBM (default; fastest);
 *   CALIB_LM_TWO_KERNEL  the jacobian kernel materialises the compact J in HBM (the layout
 *                        calib_eval returns) and the gram kernel reads it back.
 * Both produce the same blocks up to summation order. Every sum is fixed-order, so a run is bitwise reproducible for a
 * given shard, mode and device. Bit-identity ACROSS modes, shard splits and devices holds for the one-view-per-wave
 * forms only: the stream form of the fused kernel (calib_fused_form) sums a view that a wave start cuts in two parts,
 * and where the cuts fall depends on the launch width (CU count, CALIB_STREAM_WAVES) -- "same sums, order fixed per
 * (shard shape, launch width)", 1e-13 relative between forms. CALIB_FUSED_STREAM=0 keeps the one-view-per-wave forms
 * for callers who need bit-reproducibility across devices. */
enum { CALIB_LM_FUSED = 0, CALIB_LM_TWO_KERNEL = 1 };
int calib_set_lm_mode(calib_handle_t h, int mode);
/* Which form of the fused kernel the loaded problem's rounds run in (decided by calib_set_problem from the shard's
 * shape; CALIB_FUSED_STREAM=0|1 and CALIB_STREAM_WAVES override it for tests and tuning).
 *   *out_share  > 0: stream form -- uniform fp64 shards (every view n points, n % 4 == 0, n >= 64, at least two views
 *               per wave slot of the chip): the shard's 4-point groups are dealt out to `*out_waves` waves in equal
 *               shares of `*out_share` groups, batches run across view boundaries, and a view cut by a wave start has
 *               a second (overflow) record; 0: one view item per wave (or several whole items per wave). */
int calib_fused_form(calib_handle_t h, int* out_share, int* out_waves);

int calib_num_shared(calib_handle_t h, int* out_L);          /* L                          */
int calib_num_params(calib_handle_t h, int64_t* out_K);       /* K = L + 6*num_views        */

/* Hold chosen SHARED parameters fixed in the LM loop (the reference refines all of them; this is surface beside the
 * drop-in one). Bit i of mask = shared parameter i in the order of P (bit 0 alpha, 1 beta, 2 gamma, 3 uc, 4 vc, 5.. the
 * distortion coefficients); a bit >= L is CALIB_E_INVALID. Every LM step is then the step of the problem whose
 * Jacobian has those columns deleted -- delta_free = (Jf^T Jf + lambda diag(Jf^T Jf))^-1 Jf^T r, delta_fixed = 0 -- and a
 * fixed parameter keeps the bits of the start point; error, accept rule, lambda schedule and stop rule are unchanged.
 * The mask takes effect at the next calib_lm_begin (hence calib_refine, calib_refine_awk, calib_lm_step_delta and the
 * sharded loop, where every rank must set the same mask) and stays on the handle across problems. All L bits set is
 * legal: only the poses move (calib_refine_poses does that per view, without the global loop). Mask 0, the default,
 * is bit for bit the loop without this call. calib_eval and calib_normal_eq are not affected. */
int calib_set_fixed_shared(calib_handle_t h, uint32_t mask);
int calib_get_fixed_shared(calib_handle_t h, uint32_t* out_mask);

/* One evaluation at P. Any output may be NULL.
 *   out_y   (MN,2)    projection            -> Calibrator.projectAllPoints
 *   out_r   (MN,2)    sensor - projection   -> residual of src/calibrate.py:151
 *   out_Jc  (MN,2,C)  compact Jacobian, C = L+6: per point rows (du, dv), columns
 *                     [shared L | the point's own view's 6]  -> ProjectionJacobian.compute
 *   out_sse           sum of squared residual norms -> _computeReprojectionError           */
int calib_eval(calib_handle_t h, const double* P, double* out_y, double* out_r,
               double* out_Jc, double* out_sse);

/* Block-arrow normal equations at P (J^T J and J^T r of src/calibrate.py:146,152):
 *   out_B (L,L), out_E (M,L,6), out_V (M,6,6), out_g (K).  Any may be NULL. */
int calib_normal_eq(calib_handle_t h, const double* P, double* out_B, double* out_E,
                    double* out_V, double* out_g);

/* delta = (J^T J + lambda diag(J^T J))^-1 J^T r at P (src/calibrate.py:152), solved on the
 * device through the Schur complement of the 6x6 view blocks. out_delta (K). */
int calib_lm_step_delta(calib_handle_t h, const double* P, double lambda, double* out_delta);

/* The whole refinement loop of src/calibrate.py:143-171 on the device.
 * P_inout (K): start point in, refined parameters out.
 * out_sse: the reference's return value = err(P) evaluated BEFORE the last update.
 * out_trace: max_iters * (CALIB_TRACE_HEADER + L) doubles or NULL.
 * max_iters <= 0 is CALIB_E_INVALID (the reference raises UnboundLocalError). */
int calib_refine(calib_handle_t h, double* P_inout, int max_iters,
                 double lam_init, double lam_min, double lam_max, double err_min,
                 double* out_sse, int* out_iters, double* out_trace);

/* Parameter vector (de)composition behind the boundary: Calibrator._composeParameterVector /
 * _decomposeParameterVector (src/calibrate.py:199-267). A (3,3) row-major, W (M,4,4) board poses in the
 * camera frame, k (5 radtan | 4 fisheye) <-> P (L + 6 M). Rotations become Euler angles in DEGREES with the
 * gimbal-lock branches of rotationMatrixToEuler (src/mathutils.py:13-33) and back through
 * eulerToRotationMatrix (src/mathutils.py:36-51); one device thread per view. Needs no handle.
 * calib_refine_awk = compose -> calib_refine -> decompose on the handle's problem: the signature of
 * Calibrator.refineCalibrationParameters (src/calibrate.py:117) for a C caller. */
int calib_compose_params(int model, int64_t num_views, const double* A, const double* W, const double* k,
                         double* P_out, int device_id);
int calib_decompose_params(int model, int64_t num_views, const double* P, double* A_out, double* W_out,
                           double* k_out, int device_id);
int calib_refine_awk(calib_handle_t h, double* A_inout, double* W_inout, double* k_inout, int max_iters,
                     double lam_init, double lam_min, double lam_max, double err_min,
                     double* out_sse, int* out_iters, double* out_trace);

/* ---- stepping form of the same loop (multi-GPU shards, benchmarks) ----------------
 * One LM round = calib_lm_local (per-shard kernels, fills the reduce buffer)
 *              -> [all-reduce(sum) of the reduce buffer across shards]
 *              -> calib_lm_update (accept/reject, lambda, solve, back-substitute).
 * Round 0 bootstraps (evaluates P0); rounds 1..max_iters are the LM iterations.
 * All calls only enqueue work on the handle's stream. */
int calib_lm_begin(calib_handle_t h, const double* P0, int max_iters,
                   double lam_init, double lam_min, double lam_max, double err_min);
int calib_lm_reduce_size(calib_handle_t h, int64_t* out_num_doubles);
/* Use a caller-owned DEVICE buffer of calib_lm_reduce_size doubles as the reduce buffer
 * (e.g. the storage of a torch tensor handed to torch.distributed.all_reduce). NULL restores
 * the library's own buffer. */
int calib_lm_bind_reduce_buffer(calib_handle_t h, void* reduce_dev);
int calib_lm_local(calib_handle_t h);
int calib_lm_update(calib_handle_t h);
/* rounds x (local, update) without a collective (single shard) -- also on a handle that owns a
 * communicator: calib_refine, calib_lm_step_delta and calib_normal_eq, which are built on it, never take part
 * in a collective. If check_every > 0 the host reads the device's done flag every check_every rounds and
 * stops early. */
int calib_lm_run(calib_handle_t h, int rounds, int check_every);
/* rounds x (local, exchange, update) with the exchange done by the library: summed inside the reduce kernel
 * over xGMI when peers are connected (calib_peer_connect), else an ncclAllReduce (calib_rccl_init). Every rank
 * must make the same call. CALIB_E_STATE when the handle has neither. */
int calib_lm_run_sharded(calib_handle_t h, int rounds, int check_every);

/* ---- peer exchange over xGMI (optional; the fastest form of the one exchange) -----------------------
 * The sum over the ranks happens INSIDE the kernel that finishes a shard's reduce buffer: each wave stores its
 * element point-to-point into every other rank's slot memory and polls its own for theirs (kernels.hpp,
 * "peer exchange"); no collective is launched, no stream is handed over, and every rank adds in rank order,
 * so the reduced system -- hence every accept/reject decision -- is bitwise identical everywhere. It replaces
 * the all-reduce torch.distributed / RCCL would launch per LM round. One process per GPU, ranks on one node:
 *   every rank: calib_peer_prepare(h, nranks, rank, handle64)       allocates its slot memory, exports it (HIP IPC)
 *   all-gather the CALIB_PEER_HANDLE_BYTES-byte handles by any means (rank order)
 *   every rank: calib_peer_connect(h, handles, timeout_s)            maps the peers' slot memory
 *   every rank: calib_peer_selftest(h, rounds, timeout_s)            exchanges known values, checks the sums
 * then calib_lm_run_sharded runs whole rounds. A rank that waits longer than timeout_s (<= 0: 60 s) for a
 * contribution stops waiting: the step is rejected, and calib_lm_done / calib_lm_end (and the self-test)
 * return CALIB_E_HIP -- the kernels never spin without bound. Handles of one exchange must call
 * calib_lm_run_sharded in lockstep (same number of rounds; they stop together because the done flag is derived
 * from the identical sums). calib_lm_run and everything built on it stay single-shard on a connected handle.
 * calib_peer_shutdown (or calib_destroy) unmaps and frees. nranks <= 64.
 * Exercised with one rank per process on ONE GPU (tests/test_gpu_multiproc.py); callers should keep the
 * self-test and fall back to calib_rccl_* / their own all-reduce when it fails on any rank. */
#define CALIB_PEER_HANDLE_BYTES 64
int calib_peer_prepare(calib_handle_t h, int nranks, int rank, void* out_handle64);
int calib_peer_connect(calib_handle_t h, const void* handles, double timeout_s);
int calib_peer_selftest(calib_handle_t h, int rounds, double timeout_s);
int calib_peer_shutdown(calib_handle_t h);

/* ---- in-library all-reduce (optional) -------------------------------------------------------------
 * The ONE exchange of the sharded loop can also be issued by the library itself, as ncclAllReduce on
 * the engine's own stream (no hand-off to another framework's stream, and calib_lm_run then drives
 * whole rounds -- local, all-reduce, update -- from C). RCCL is not linked: calib_rccl_load dlopens the
 * librccl.so the process already uses (path given by the caller, e.g. the one PyTorch ships) and
 * resolves ncclGetUniqueId / ncclCommInitRank / ncclAllReduce / ncclCommDestroy / ncclCommAbort.
 *   rank 0: calib_rccl_unique_id(id) -> broadcast the 128 bytes by any means -> every rank:
 *   calib_rccl_init(h, nranks, rank, id)   (collective)  -> calib_rccl_selftest(h, timeout_s)
 * calib_rccl_init blocks until every rank has joined, for at most 120 s (calib_rccl_init_deadline: a
 * caller-chosen limit); past the deadline it returns CALIB_E_HIP and the handle has no communicator.
 * The self-test all-reduces a rank-dependent vector and checks the sums, polling the stream against the
 * deadline; on a wrong answer or a timeout it ABORTS the communicator (ncclCommAbort) and returns
 * CALIB_E_HIP, and the caller falls back to its own all-reduce (calib_lm_bind_reduce_buffer). The collective is
 * never implicit: calib_lm_run_sharded runs whole rounds (local, all-reduce, update) and calib_lm_allreduce is
 * that step alone for callers that drive the three steps themselves; calib_lm_run and everything built on it
 * stay single-shard. Exercised with one rank per process on one GPU (tests/test_gpu_multiproc.py); more than
 * one GPU has not been available to this build. */
int calib_rccl_load(const char* librccl_path);
int calib_rccl_unique_id(void* out_id128);
int calib_rccl_init(calib_handle_t h, int nranks, int rank, const void* id128);
int calib_rccl_init_deadline(calib_handle_t h, int nranks, int rank, const void* id128, double timeout_s);
int calib_rccl_selftest(calib_handle_t h, double timeout_s);
int calib_rccl_shutdown(calib_handle_t h);
int calib_lm_allreduce(calib_handle_t h);
int calib_lm_done(calib_handle_t h, int* out_done);           /* synchronises */
/* Synchronise and copy trace row `iter` (CALIB_TRACE_HEADER + L doubles) of the running loop;
 * out_iters = LM iterations executed so far (rows >= that are not written yet). */
int calib_lm_peek_trace(calib_handle_t h, int iter, double* out_row, int* out_iters);
/* Synchronise, return refined P (K), reference-style sse, iterations executed, trace. */
int calib_lm_end(calib_handle_t h, double* P_out, double* out_sse, int* out_iters,
                 double* out_trace);

/* ---- uncertainty of an estimate: per-view reprojection errors and the parameter covariance -----------------
 * Surface beside the drop-in one (the reference returns neither). Evaluated at a parameter vector P, normally the
 * refinement's result. With n the total number of points, r the (n,2) residuals at P, F the fixed shared
 * parameters of the handle (calib_set_fixed_shared), Jf the Jacobian with the columns in F deleted and
 * K_free = L - |F| + 6 M:
 *   dof = 2 n - K_free (dof <= 0: CALIB_E_INVALID),   sigma2 = sse(P) / dof,   C = sigma2 (Jf^T Jf)^-1
 * -- no damping, no pseudo-inverse; rows and columns of fixed parameters are exactly 0.0 in every output. C is never
 * formed densely: with S the Schur complement of the shared block, V_i / E_i view i's blocks and Y_i = V_i^-1 E_i^T,
 *   C_ss = sigma2 S_free^-1,   C_vv,i = sigma2 V_i^-1 + Y_i C_ss Y_i^T,   C_sv,i = -C_ss Y_i^T.
 * A view whose V_i has a pivot that is not positive (e.g. fewer than three points), or an S_free that has one, is
 * CALIB_E_SINGULAR: the condition under which the LM step fails. The blocks come from one LM round at lambda = 0 in the
 * handle's LM mode and storage type (fp32 storage: the Jacobian the fp32 path evaluates; sums and all that follows
 * are fp64). UNITS: pose parameters are those of P -- Euler angles in DEGREES, then t -- and standard deviations and
 * covariances are of those quantities. Sums are fixed-order: results are bitwise reproducible for a given shard, mode
 * and device.
 *
 * calib_view_errors: for view i with n_i points, view_sse = sum |r|^2, view_rms = sqrt(view_sse / n_i) (per-point RMS;
 *   NaN for an empty view), view_max = max |r| (0 for an empty view). Each output (M) or NULL. One kernel, nothing is
 *   written per point. CALIB_E_STATE while a stepping LM run is active (it owns the view constants).
 * calib_cov_local: enqueues the lambda = 0 round at P; the handle's reduce buffer (calib_lm_bind_reduce_buffer) then
 *   holds this shard's sums. Sharded: all-reduce that buffer by any carrier (calib_lm_allreduce is the library's),
 *   then every rank calls
 * calib_cov_finish with the GLOBAL totals: the L x L step is host arithmetic on the all-reduced buffer, so
 *   out_cov_shared is bitwise equal on every rank. out_cov_views (M,6,6) and out_cov_cross (M,L,6) are this shard's
 *   views; out_std (K, the shard's K) = sqrt of the diagonal. Any output may be NULL.
 * calib_covariance = calib_cov_local + calib_cov_finish with the handle's own totals (single shard).
 * All three calib_cov_* calls return CALIB_E_STATE while a stepping LM run is active on the handle. */
int calib_view_errors(calib_handle_t h, const double* P,
                      double* out_view_sse, double* out_view_rms, double* out_view_max);
int calib_cov_local(calib_handle_t h, const double* P);
int calib_cov_finish(calib_handle_t h, int64_t total_points, int64_t total_views,
                     double* out_sigma2, int64_t* out_dof,
                     double* out_cov_shared, double* out_cov_views, double* out_cov_cross, double* out_std);
int calib_covariance(calib_handle_t h, const double* P, double* out_sigma2, int64_t* out_dof,
                     double* out_cov_shared, double* out_cov_views, double* out_cov_cross, double* out_std);

/* Numeric forward model on caller points (no problem needed):
 *   calib_distort_points            DistortionModel.distortPoints          src/distortion.py:78-108,198-220
 *   calib_project_with_distortion   DistortionModel.projectWithDistortion  src/distortion.py:42-59
 * x_norm (N,2) normalised points; cam_xyz (N,3) camera-frame points; A (3,3) row-major. */
int calib_distort_points(int model, int64_t n, const double* x_norm, const double* k,
                         double* out_xd);
int calib_project_with_distortion(int model, int64_t n, const double* A, const double* cam_xyz,
                                  const double* k, double* out_uv);

/* ---- undistortion: the inverse of the camera model, rectify maps, image remap -----------------------------------
 * Surface beside the drop-in one (the reference runs its model forward only). Stateless: no handle, host pointers, the
 * work runs on device_id. A and newA are (3,3) row-major, A = [[alpha, gamma, uc], [0, beta, vc], [0, 0, 1]]; k is the
 * model's coefficient vector (5 radtan | 4 fisheye). alpha or beta equal to 0, in A or in newA, is CALIB_E_INVALID.
 *
 * calib_undistort_points: uv (n,2) pixels of the distorted image -> out_xy (n,2), the IDEAL point of each: normalised
 *   (x, y) when newA is NULL, else the pixel newA (x, y, 1). A pixel becomes the distorted normalised point
 *   yd = (v - vc) / beta, xd = (u - uc - gamma yd) / alpha, and distort(x, y) = (xd, yd) is solved by Newton in fp64
 *   with the model's own 2 x 2 Jacobian (radtan) or in one dimension on theta (fisheye, which is radial; theta_d < 1e-8
 *   returns (xd, yd), the forward model's r -> 0 limit). At most 30 iterations; an iteration stops at a step of 4 ulp of
 *   max(1, |x|). out_status (n) or NULL, per point:
 *     0  solved: |distort(x, y) - (xd, yd)|_inf <= 64 * 2^-52 * max(1, |(xd, yd)|_inf) AND the model preserves
 *        orientation at (x, y) -- radtan: its Jacobian is positive definite; fisheye: d theta_d / d theta > 0 and
 *        theta < pi / 2. This is the root on the branch that contains the optical axis.
 *     1  not solved, out_xy is NaN: the target has no preimage (past the turning point of the radial polynomial), the
 *        iteration ended on a folded-over branch, or the input is not finite. The call itself still returns CALIB_OK.
 *   n == 0 is CALIB_OK.
 * calib_undistort_maps: the maps an undistorted image of width x height pixels and camera matrix newA (NULL: A itself,
 *   gamma kept) reads from: destination pixel (col j, row i) looks along y = (i - vc') / beta',
 *   x = (j - uc' - gamma' y) / alpha' and finds it in the source at (mapx, mapy)(i, j) = A distort(x, y). Evaluated in
 *   fp64, STORED AS FP32 (rounded to nearest), two (height, width) planes: half a ulp of fp32 is 3e-5 px at 1000 px.
 *   width * height < 2^31.
 * calib_remap: dst (dst_h, dst_w, channels) = src (src_h, src_w, channels; interleaved, 1 <= channels <= 4) sampled
 *   bilinearly at (mapx, mapy) (dst_h, dst_w), fp32 arithmetic: x0 = floor(sx), fx = sx - x0, likewise y, taps a (y0, x0),
 *   b (y0, x0 + 1), c (y0 + 1, x0), d (y0 + 1, x0 + 1); top = a + fx (b - a), bot = c + fx (d - c), out = top + fy (bot - top).
 *   A TAP outside the source takes the constant `border` (the pixel's other taps still count; nothing is clamped or
 *   reflected), and a map entry that is NaN or infinite yields `border`. CALIB_IMAGE_U8: rint (ties to even), saturated to
 *   [0, 255]; CALIB_IMAGE_F32: the fp32 value. src, dst and the maps must not overlap. */
enum { CALIB_IMAGE_U8 = 0, CALIB_IMAGE_F32 = 1 };
int calib_undistort_points(int model, int64_t n, const double* A, const double* k, const double* uv,
                           const double* newA, double* out_xy, int32_t* out_status, int device_id);
int calib_undistort_maps(int model, const double* A, const double* k, const double* newA, int width, int height,
                         float* out_mapx, float* out_mapy, int device_id);
int calib_remap(int dtype, const void* src, int src_h, int src_w, int channels, const float* mapx, const float* mapy,
                int dst_h, int dst_w, double border, void* dst, int device_id);

/* Per-view homography polish of the initialisation stage: Calibrator._refineHomographies
 * (src/calibrate.py:60-111, HomographyJacobian src/jacobian.py:88-121), all views in one launch.
 * H_inout (M,3,3) row-major: DLT homographies in, LM-refined (H[2,2] = 1) out. model_xyz (MN,3):
 * only X, Y are used. max_iters = 20 in the reference. */
int calib_refine_homographies(int64_t num_views, const int64_t* view_offsets, const double* sensor_uv,
                              const double* model_xyz, double* H_inout, int max_iters, int device_id);

/* Pose-only refinement with a KNOWN camera: every view runs the loop of src/calibrate.py:143-171 on its own six
 * parameters, with its own lambda, accept decision and stop, all views in one launch. shared (L): the camera in the
 * order of P; poses_inout (M,6): per view rho_x, rho_y, rho_z [DEGREES], t -- start values in, refined out.
 * Per view (each may be NULL): out_sse = the view's error before its last update (the reference's return
 * convention; NaN when no iteration ran), out_iters = iterations executed, out_status = 0 or CALIB_E_SINGULAR (fewer
 * than three points, or V + lambda diag V has a pivot that is not positive); such a view keeps its input pose and
 * does not fail the call. max_iters <= 0 is CALIB_E_INVALID. Needs no handle. */
int calib_refine_poses(int model, int64_t num_views, const int64_t* view_offsets, const double* sensor_uv,
                       const double* model_xyz, const double* shared, double* poses_inout, int max_iters,
                       double lam_init, double lam_min, double lam_max, double err_min, double* out_sse,
                       int* out_iters, int* out_status, int device_id);

/* HomographyJacobian.compute (src/jacobian.py:88-121): the (2N, 9) Jacobian of the projection of the
 * model points (X, Y, 1) through H = h.reshape(3,3) with respect to h, rows (u_j, v_j) interleaved.
 * h9 (9), model_xyz (N,3): only X, Y are used; out_J (2N,9) row-major. */
int calib_homography_jacobian(int64_t n, const double* h9, const double* model_xyz, double* out_J,
                              int device_id);

/* ---- closed-form initialisation stage on the device (Calibrator.estimateCalibrationParameters,
 * src/calibrate.py:41-58). The 6-unknown intrinsics fit and the <= 5-unknown distortion solve stay on
 * the host; everything that is per view / per point runs here. ------------------------------------
 * calib_estimate_homographies: normalised DLT (src/linearcalibrate.py:7-90) for every view, followed by
 *   refine_iters LM iterations (0 = DLT only). H_out (M,3,3), H[2,2] = 1.
 * calib_compute_extrinsics: world-to-camera poses from A (3,3) and the homographies
 *   (src/linearcalibrate.py:306-371). W_out (M,4,4).
 * calib_distortion_normal_equations: D^T D (n,n) and D^T Ddot (n) of the linear distortion estimate
 *   D k = Ddot (src/distortion.py:110-191, 222-271), n = 5 radtan / 4 fisheye; W (M,4,4). */
int calib_estimate_homographies(int64_t num_views, const int64_t* view_offsets, const double* sensor_uv,
                                const double* model_xyz, double* H_out, int refine_iters, int device_id);
int calib_compute_extrinsics(int64_t num_views, const double* A, const double* H, double* W_out, int device_id);
int calib_distortion_normal_equations(int model, int64_t num_views, const int64_t* view_offsets,
                                      const double* sensor_uv, const double* model_xyz, const double* A,
                                      const double* W, double* out_DtD, double* out_Dtd, int device_id);

/* HIP-event timing of the dominant kernels over the rounds enqueued since the last
 * calib_profile_enable(h, on). on = 0: off; on = 1: every launch is bracketed by an event pair;
 * on = N > 1: every N-th launch of each kernel (an event pair keeps a launch from being dispatched
 * back to back with its neighbours, so timing every launch slows the loop it measures).
 * which: 0 = jacobian kernel, 1 = J^T J (MFMA) kernel, 2 = fused jacobian + J^T J kernel;
 * out_launches = launches timed, out_total_ms = their summed duration. */
int calib_profile_enable(calib_handle_t h, int on);
int calib_profile_read(calib_handle_t h, int which, double* out_total_ms, int64_t* out_launches);

/* ---- stereo calibration with both cameras KNOWN: the rig between two calibrated cameras --------------------------
 * Cameras a and b, each radtan or fisheye with its shared vector (alpha beta gamma uc vc k.., the order of P) held
 * fixed, see M views of one board; each camera's correspondences are a CSR of their own (the cameras may see
 * different corners, either side of a view may be empty). Unknowns Ps (6 + 6 M) = (rig, pose_0, .., pose_{M-1}), every
 * 6-tuple rho_x, rho_y, rho_z [DEGREES], t as the view blocks of P: pose_i takes board points into camera a's frame,
 * Xa = R_i X + t_i; the rig takes camera a's frame into camera b's, Xb = R_rig Xa + t_rig. Residuals
 * uv_a - project_a(Xa) and uv_b - project_b(Xb); the error is the sum of their squared norms over both cameras.
 * Stateless: host pointers in and out, no handle. Any output may be NULL. Every sum is fixed-order: a call is bitwise
 * reproducible. A bad model id, num_views < 1, max_iters <= 0, a NULL input or an offset array that does not start at 0
 * or decreases is CALIB_E_INVALID before any device call.
 *
 * calib_stereo_normal_eq: the block-arrow normal equations at Ps -- out_B (6,6) rig block, out_E (M,6,6) rig row x view
 *   column, out_V (M,6,6), out_g (6 + 6 M) = J^T r in the order of Ps, out_sse_ab (2) the error per camera.
 * calib_stereo_step_delta: delta = (J^T J + lambda diag J^T J)^-1 J^T r at Ps through the Schur complement of the view
 *   blocks. CALIB_E_SINGULAR when a view has fewer than three points in total or a pivot of V_i + lambda diag V_i that
 *   is not positive (an empty view), or when the rig's Schur complement has such a pivot (no view with points in b).
 * calib_refine_stereo: the loop of src/calibrate.py:143-171 on Ps with the rules of calib_refine. out_sse = err(Ps)
 *   before the last update; out_sse_ab (2) = the error per camera AT the returned Ps; out_trace rows are
 *   CALIB_TRACE_HEADER + 6 doubles, the six rig parameters before the update in the place of the shared ones.
 *   On CALIB_E_SINGULAR Ps_inout is left as it was. */
typedef struct {
    int model_a, model_b;
    int64_t num_views;
    const int64_t* offs_a; const double *uv_a, *xyz_a, *shared_a;
    const int64_t* offs_b; const double *uv_b, *xyz_b, *shared_b;
} calib_stereo_problem_t;

int calib_stereo_normal_eq(const calib_stereo_problem_t* problem, const double* Ps, double* out_B, double* out_E,
                           double* out_V, double* out_g, double* out_sse_ab, int device_id);
int calib_stereo_step_delta(const calib_stereo_problem_t* problem, const double* Ps, double lambda, double* out_delta,
                            int device_id);
int calib_refine_stereo(const calib_stereo_problem_t* problem, double* Ps_inout, int max_iters, double lam_init,
                        double lam_min, double lam_max, double err_min, double* out_sse, double* out_sse_ab,
                        int* out_iters, double* out_trace, int device_id);

/* ---- joint stereo calibration: both cameras, the rig and the board poses in one problem ---------------------------
 * The problem of calib_refine_stereo with the two cameras free. Unknowns Pj (S + 6 M) = (shared_a[La], shared_b[Lb],
 * rig[6], pose_0[6], .., pose_{M-1}[6]), S = La + Lb + 6 <= 26, the shared vectors in the order of P, the 6-tuples as in
 * Ps. The struct's shared_a / shared_b are not read and may be NULL: the cameras travel in Pj. fixed_mask: bit s set
 * holds shared unknown s (camera a's, then camera b's, then the rig's) fixed by the rule of calib_lm_begin's mask -- the
 * reduced S x S system is edited, the parameter keeps its bits; a bit at or above S is CALIB_E_INVALID. With all
 * La + Lb camera bits set the problem is calib_refine_stereo's. Stateless, fixed-order sums, argument checks before
 * any device call as for the calls above.
 *
 * calib_stereo_joint_normal_eq: out_B (S,S) -- its shared_a x (shared_b, rig) block is exactly zero --, out_E (M,S,6)
 *   shared row x view column, out_V (M,6,6), out_g (S + 6 M) = J^T r in the order of Pj, out_sse_ab (2).
 * calib_stereo_joint_step_delta: delta (S + 6 M) = the LM step at Pj through the Schur complement of the view blocks;
 *   0 at fixed parameters.
 * calib_refine_stereo_joint: the loop of calib_refine_stereo on Pj; out_trace rows are CALIB_TRACE_HEADER + S doubles,
 *   the shared unknowns before the update.
 * CALIB_E_SINGULAR (Pj_inout left as it was): a view with fewer than three points in total, an empty view, a pivot of
 *   a view block or of the reduced system that is not positive -- a free camera that sees nothing, for one; the same
 *   problem with that camera's bits all set succeeds. */
int calib_stereo_joint_normal_eq(const calib_stereo_problem_t* problem, const double* Pj, double* out_B, double* out_E,
                                 double* out_V, double* out_g, double* out_sse_ab, int device_id);
int calib_stereo_joint_step_delta(const calib_stereo_problem_t* problem, const double* Pj, uint64_t fixed_mask,
                                  double lambda, double* out_delta, int device_id);
int calib_refine_stereo_joint(const calib_stereo_problem_t* problem, double* Pj_inout, uint64_t fixed_mask, int max_iters,
                              double lam_init, double lam_min, double lam_max, double err_min, double* out_sse,
                              double* out_sse_ab, int* out_iters, double* out_trace, int device_id);

/* ---- multi-camera rig calibration: N KNOWN cameras, one board -----------------------------------------------------
 * N cameras, 2 <= N <= CALIB_RIG_MAX_CAMERAS, each radtan or fisheye with its shared vector held fixed, see M views of
 * one board; each camera's correspondences are a CSR of its own (the cameras may see different corners, any camera's
 * side of a view may be empty). Camera 0 is the reference frame. Unknowns Pr (S + 6 M) = (rig_1, .., rig_{N-1}, pose_0,
 * .., pose_{M-1}), S = 6 (N - 1) <= 42, the 6-tuples as in Ps: pose_i takes board points into camera 0's frame, rig_c takes
 * camera 0's frame into camera c's, Xc = R_c X0 + t_c. Residuals uv_c - project_c(Xc); the error is the sum of their
 * squared norms over all cameras. With N = 2 the problem is calib_refine_stereo's. Stateless, host pointers, any output
 * may be NULL, fixed-order sums (a call is bitwise reproducible). N outside [2, 8], a bad model id, num_views < 1,
 * max_iters <= 0, a NULL input or an offset array that does not start at 0 or decreases is CALIB_E_INVALID before any
 * device call.
 *
 * calib_rig_normal_eq: out_B (S,S) block diagonal, one 6 x 6 block per camera c >= 1; out_E (M,S,6) shared row x view
 *   column, the 6 x 6 block of a camera that did not see the view exactly zero; out_V (M,6,6); out_g (S + 6 M) = J^T r in
 *   the order of Pr; out_sse_cam (N) the error per camera.
 * calib_rig_step_delta: delta (S + 6 M) = the LM step at Pr through the Schur complement of the view blocks.
 * calib_refine_rig: the loop of calib_refine_stereo on Pr; out_sse = err(Pr) before the last update, out_sse_cam (N) the
 *   error per camera AT the returned Pr, out_trace rows are CALIB_TRACE_HEADER + S doubles, the rigs before the update.
 * CALIB_E_SINGULAR (Pr_inout left as it was): a view with fewer than three points over all cameras, an empty view, a
 *   pivot of a view block or of the reduced system that is not positive -- a camera c >= 1 that sees nothing. Camera 0
 *   seeing nothing is a solvable problem. */
#define CALIB_RIG_MAX_CAMERAS 8
typedef struct {
    int model;
    const int64_t* offs; const double *uv, *xyz, *shared;
} calib_rig_camera_t;
typedef struct {
    int num_cameras;
    int64_t num_views;
    const calib_rig_camera_t* cameras;
} calib_rig_problem_t;

int calib_rig_normal_eq(const calib_rig_problem_t* problem, const double* Pr, double* out_B, double* out_E, double* out_V,
                        double* out_g, double* out_sse_cam, int device_id);
int calib_rig_step_delta(const calib_rig_problem_t* problem, const double* Pr, double lambda, double* out_delta,
                         int device_id);
int calib_refine_rig(const calib_rig_problem_t* problem, double* Pr_inout, int max_iters, double lam_init, double lam_min,
                     double lam_max, double err_min, double* out_sse, double* out_sse_cam, int* out_iters, double* out_trace,
                     int device_id);

/* ---- joint rig calibration: N cameras, their rigs and the board poses in one problem --------------------------------
 * calib_refine_rig with the cameras free as well. Unknowns, camera-major: Pq (S + 6 M) = (shared_0[L0] | shared_1[L1],
 * rig_1[6] | .. | shared_{N-1}, rig_{N-1}[6] | pose_0[6], .., pose_{M-1}[6]), the shared vectors in the order of P (alpha
 * beta gamma uc vc k..; L = 10 radtan, 9 fisheye), the 6-tuples, frames and residuals as in Pr; S = sum L_c + 6 (N - 1)
 * <= 122. At N = 2 Pq is calib_refine_stereo_joint's Pj. The problem is calib_rig_problem_t; cameras[c].shared is not
 * read and may be NULL (the cameras travel in Pq). fixed_mask: two 64-bit words over all S unknowns, rigs included (bit
 * s of word s / 64 holds unknown s fixed, by the rule of calib_lm_begin's mask: the step is 0 there and the value keeps
 * its bits), NULL = none. With every camera bit set the problem is calib_refine_rig's. Stateless, host pointers, any
 * output may be NULL, fixed-order sums (a call is bitwise reproducible). What calib_refine_rig rejects (but a NULL
 * shared), and a mask bit at or above S, is CALIB_E_INVALID before any device call.
 *
 * calib_rig_joint_normal_eq: out_B (S,S) dense, exactly zero outside its diagonal blocks (L0 wide for camera 0, L_c + 6
 *   for camera c >= 1); out_E (M,S,6), the band of a camera that did not see the view exactly zero; out_V (M,6,6); out_g
 *   (S + 6 M) in the order of Pq; out_sse_cam (N).
 * calib_rig_joint_step_delta: delta (S + 6 M), the LM step at Pq through the Schur complement; 0 at fixed unknowns.
 * calib_refine_rig_joint: the loop of calib_refine_rig on Pq; out_trace rows are CALIB_TRACE_HEADER + S doubles.
 * CALIB_E_SINGULAR (Pq_inout left as it was): a view with fewer than three points over all cameras, an empty view, a
 *   pivot of a view block or of the reduced system that is not positive -- a free camera that sees nothing, camera 0
 *   included; the same problem succeeds with that camera's bits (and for c >= 1 its rig's) set. */
int calib_rig_joint_normal_eq(const calib_rig_problem_t* problem, const double* Pq, double* out_B, double* out_E,
                              double* out_V, double* out_g, double* out_sse_cam, int device_id);
int calib_rig_joint_step_delta(const calib_rig_problem_t* problem, const double* Pq, const uint64_t* fixed_mask /* [2] */,
                               double lambda, double* out_delta, int device_id);
int calib_refine_rig_joint(const calib_rig_problem_t* problem, double* Pq_inout, const uint64_t* fixed_mask /* [2] */,
                           int max_iters, double lam_init, double lam_min, double lam_max, double err_min, double* out_sse,
                           double* out_sse_cam, int* out_iters, double* out_trace, int device_id);

/* ---- robust losses on the joint rig problem ---------------------------------------------------------------------------
 * The joint rig entry points above with sum_p rho(s_p) in the place of sum_p s_p, s_p = rx^2 + ry^2 the squared length
 * of point p's 2-vector residual (a loss is per point, not per coordinate), over all points of all cameras:
 *   CALIB_LOSS_NONE    rho(s) = s
 *   CALIB_LOSS_HUBER   rho(s) = s for s <= d^2, 2 d sqrt(s) - d^2 above;   w = rho'(s) = 1, d / sqrt(s) above
 *   CALIB_LOSS_CAUCHY  rho(s) = d^2 log1p(s / d^2);                        w = 1 / (1 + s / d^2)
 * d = scale, in pixels, finite and > 0. The step is the LM step of the re-weighted problem: a point's two Jacobian rows
 * and its residual are multiplied by sqrt(w) at the current point (first order, IRLS; the second-order term of Triggs'
 * correction is left out). Accept rule, lambda schedule, stop rule and trace are calib_refine_rig_joint's, on sum rho.
 * Problem, Pq, fixed_mask, outputs and errors are those of the joint rig entry points; with every camera bit set the
 * problem is the robust rig-only one. loss == NULL or kind CALIB_LOSS_NONE IS the plain entry point, bit for bit. Any
 * other kind, or a scale that is not finite and > 0, is CALIB_E_INVALID before any device call.
 *
 * calib_rig_robust_normal_eq: the blocks of the weighted problem at Pq; out_cost_cam (N) = sum rho per camera.
 * calib_rig_robust_step_delta, calib_refine_rig_robust: out_cost = sum rho before the last update, out_cost_cam at the
 *   returned Pq, trace columns 1 and 2 = sum rho.
 * calib_rig_residuals: out_res (sum_c n_c, 2) = sensor - projection of every point at Pq, camera 0's n_0 rows first, then
 *   camera 1's, .., each in the order of its uv; no loss, no mask. */
#define CALIB_LOSS_NONE 0
#define CALIB_LOSS_HUBER 1
#define CALIB_LOSS_CAUCHY 2
typedef struct {
    int kind;       /* CALIB_LOSS_* */
    double scale;   /* d, pixels */
} calib_loss_t;

int calib_rig_robust_normal_eq(const calib_rig_problem_t* problem, const double* Pq, const calib_loss_t* loss, double* out_B,
                               double* out_E, double* out_V, double* out_g, double* out_cost_cam, int device_id);
int calib_rig_robust_step_delta(const calib_rig_problem_t* problem, const double* Pq, const uint64_t* fixed_mask /* [2] */,
                                const calib_loss_t* loss, double lambda, double* out_delta, int device_id);
int calib_refine_rig_robust(const calib_rig_problem_t* problem, double* Pq_inout, const uint64_t* fixed_mask /* [2] */,
                            const calib_loss_t* loss, int max_iters, double lam_init, double lam_min, double lam_max,
                            double err_min, double* out_cost, double* out_cost_cam, int* out_iters, double* out_trace,
                            int device_id);
int calib_rig_residuals(const calib_rig_problem_t* problem, const double* Pq, double* out_res, int device_id);

/* ---- using a calibrated rig: rectify maps, rectified points, triangulation ---------------------------------------
 * Stateless, host pointers, the work runs on device_id; cameras as in the undistortion entries (A (3,3) row-major, k the
 * model's coefficients). R is a (3,3) row-major rotation; |det R - 1| > 1e-6 is CALIB_E_INVALID, as are a bad model id, a
 * NULL input and alpha or beta equal to 0 in a camera matrix -- all before any device call.
 *
 * calib_rectify_maps: calib_undistort_maps with a rotation between the destination and the camera. R (NULL = identity)
 *   takes the camera's frame into the rectified one, P is the (3,3) camera matrix of the destination (the left block of
 *   a rectification's projection matrix). Destination pixel (col j, row i) looks along r = (x, y, 1),
 *   y = (i - vc') / beta', x = (j - uc' - gamma' y) / alpha', that is along X = R^T r in the camera's own frame, and finds
 *   it in the source at (mapx, mapy)(i, j) = A distort(X.x / X.z, X.y / X.z). A ray with X.z <= 0 (it does not enter the
 *   camera's front half space) or a normalised point that is not finite gives NaN in BOTH planes, which calib_remap turns
 *   into `border`. fp64, stored as fp32 rounded to nearest; width * height < 2^31. With R = NULL and P = A the maps equal
 *   calib_undistort_maps' bit for bit.
 * calib_rectify_points: uv (n,2) pixels of the distorted image -> out_uv (n,2) pixels of the rectified one: the inverse
 *   of the model as calib_undistort_points finds it, then P (R (x, y, 1)) on the host. out_status (n) or NULL: 0, or 1
 *   (out_uv NaN) where calib_undistort_points reports 1 or the rotated point has Z <= 0. n == 0 is CALIB_OK.
 * calib_triangulate: the point X (camera a's frame) that the pixel pair uv_a[i], uv_b[i] sees, cameras a and b joined by
 *   Xb = R Xa + t. Both pixels are inverted as calib_undistort_points does; the start is the midpoint of the common
 *   perpendicular of the two rays; then at most 20 damped Gauss-Newton steps minimise the four PIXEL residuals
 *   uv_a - project_a(X), uv_b - project_b(R X + t) through each camera's full forward model, with the damping rule of
 *   calib_refine (lambda from 1e-3, / 10 on an accepted step, * 10 on a rejected one). A step is accepted when it lowers
 *   the error; with eta = 2^-44 max(1, |uv|_inf) the trust in a projected pixel, a step whose predicted decrease is
 *   below flat = eta (2 sqrt(error) + eta) -- less than two errors of rounded pixels can show -- is accepted unless the
 *   error grows by more than flat. A point leaves the loop at a step <= 1e-14 |X|.
 *   out_X (n,3); out_sse (n) or NULL: the four residuals squared and summed at X; out_status (n) or NULL, per pair:
 *     0  ok
 *     1  a pixel has no inverse in its camera (calib_undistort_points' status 1), or is not finite
 *     2  degenerate geometry: the rays are parallel (sin^2 of their angle < 1e-12), or the start point or the end point
 *        has Z <= 0 in either camera, or the damped 3 x 3 system has a pivot that is not positive
 *     3  the last accepted step was still > 1e-9 |X|
 *   out_X and out_sse are NaN wherever the status is not 0; the call itself still returns CALIB_OK. n == 0 is CALIB_OK.
 *   One thread per pair, no atomics, no sums across threads: two calls agree bit for bit. */
int calib_rectify_maps(int model, const double* A, const double* k, const double* R, const double* P, int width,
                       int height, float* out_mapx, float* out_mapy, int device_id);
int calib_rectify_points(int model, int64_t n, const double* A, const double* k, const double* uv, const double* R,
                         const double* P, double* out_uv, int32_t* out_status, int device_id);
int calib_triangulate(int model_a, const double* Aa, const double* ka, int model_b, const double* Ab, const double* kb,
                      const double* R, const double* t, int64_t n, const double* uv_a, const double* uv_b, double* out_X,
                      double* out_sse, int32_t* out_status, int device_id);

/* ---- N-view triangulation: one point from every camera of a rig that saw it ----------------------------------------
 * calib_triangulate for N cameras, 2 <= N <= CALIB_RIG_MAX_CAMERAS, and a per-point mask of the cameras that saw the
 * point. Camera c is (model, A, k) as above and a rigid transform X_c = R_c X + t_c (R (3,3) row-major, NULL = identity;
 * t (3), NULL = 0) from the frame in which X is wanted -- camera 0's with the transforms of a rig calibration. No camera
 * is special: every one goes through its R_c, t_c. uv (N,n,2) is camera-major: the pixel of point i in camera c is at
 * uv[2 (c n + i)]. seen (n) or NULL: bit c of seen[i] is set where camera c saw point i; NULL = every camera saw every
 * point. An unseen camera contributes nothing to the point: its pixel is never read, whatever it holds.
 *   inverse  every seen pixel is inverted as calib_undistort_points does (the same ideal normalised point, bit for bit).
 *   start    the point closest in least squares to the seen rays o_c + s d_c, o_c = -R_c^T t_c, d_c = R_c^T (x_c, y_c, 1):
 *            sum_c (I - d_c d_c^T / |d_c|^2) (X - o_c) = 0, a 3 x 3 Cholesky. Two rays: the midpoint of their common
 *            perpendicular, calib_triangulate's start.
 *   refine   calib_triangulate's loop on the 2 m PIXEL residuals uv_c - project_c(R_c X + t_c) of the m seen cameras: at
 *            most 20 damped Gauss-Newton steps, lambda from 1e-3, / 10 on an accepted step, * 10 on a rejected one, the
 *            same accept rule with eta = 2^-44 max(1, |uv|_inf) over the seen pixels and flat = eta (2 sqrt(error) + eta),
 *            a candidate must lie in front of EVERY seen camera, a point leaves the loop at a step <= 1e-14 |X|. J^T J,
 *            J^T r and the error are summed over the seen cameras in index order.
 *   out_X (n,3); out_sse (n) or NULL: the 2 m residuals squared and summed at X; out_status (n) or NULL, per point the
 *   first that applies:
 *     4  fewer than two cameras saw the point
 *     1  a seen pixel has no inverse in its camera (calib_undistort_points' status 1), or is not finite
 *     2  degenerate geometry: the largest sin^2 of the angle between any two seen rays is < 1e-12 (N = 2:
 *        calib_triangulate's rule), or the start's 3 x 3 system is not positive definite, or the start point or the end
 *        point has Z <= 0 in a seen camera, or the damped 3 x 3 system has a pivot that is not positive
 *     3  the last accepted step was still > 1e-9 |X|
 *     0  ok
 *   out_cov (n,6) or NULL: the lower triangle, in the order 00 10 11 20 21 22, of the UNDAMPED (J^T J)^-1 at the returned
 *     X -- the covariance of X for unit pixel variance; NaN where a pivot is not positive (the status stays as it is).
 *   out_res (N,n,2) or NULL, camera-major like uv: the residuals at X, NaN for an unseen camera.
 *   out_X, out_sse, out_cov and out_res are NaN wherever the status is not 0; the call itself still returns CALIB_OK.
 *   Which optional outputs are requested does not change a bit of the others.
 * Stateless, host pointers. CALIB_E_INVALID before any device call: N outside [2, 8], a NULL cameras, A, k, uv or out_X, a
 * bad model id, alpha or beta equal to 0, |det R_c - 1| > 1e-6, n < 0, a bit of seen at or above N. n == 0 is CALIB_OK
 * without touching a device. One thread per point, no atomics, no sums across threads: two calls agree bit for bit, and a
 * point's result does not depend on the cameras that did not see it, nor on how many there are. */
typedef struct {
    int model;
    const double *A, *k, *R, *t;
} calib_view_camera_t;
int calib_triangulate_multi(int num_cameras, const calib_view_camera_t* cameras, int64_t n, const double* uv,
                            const uint32_t* seen, double* out_X, double* out_sse, int32_t* out_status, double* out_cov,
                            double* out_res, int device_id);

#ifdef __cplusplus
}
#endif
#endif /* CALIB_LM_H */
