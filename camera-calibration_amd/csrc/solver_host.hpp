// Host front end of the four solvers on the LM loop of stereo_loop.hpp: the rig between two known cameras (stereo.hpp),
// joint stereo (stereo_joint.hpp), the rig of N known cameras (rig.hpp) and the joint rig (rig_joint.hpp). Included once
// by calib_lm.hip, after the kernel headers and its own helpers (fail, HIP_TRY, LAUNCHED, DevBuf, dispatch_model,
// check_views, use_device). What a solver is on the host is one descriptor (solver_desc); one checker, one begin and
// three drivers (solver_normal_eq, solver_step_delta, solver_refine) serve all four. A robust loss (the joint rig's) is a
// member of the run: begin() then takes the solver's evaluate_robust; the drivers are the same.
#pragma once
#include "block_map.hpp"

namespace {

enum SolverKind { kSolveStereo, kSolveStereoJoint, kSolveRig, kSolveRigJoint };
constexpr bool solver_is_pair(SolverKind k) { return k == kSolveStereo || k == kSolveStereoJoint; }
constexpr bool solver_is_joint(SolverKind k) { return k == kSolveStereoJoint || k == kSolveRigJoint; }

// The one internal form of a problem: the rig entry points' camera array. A stereo problem becomes two such cameras.
struct SolverProblem {
    calib_rig_camera_t pair[2];
    const calib_rig_camera_t* cams = nullptr;
    int ncam = 0;
    int64_t M = 0;
    SolverProblem(const calib_stereo_problem_t* p) {
        if (!p) return;
        pair[0] = calib_rig_camera_t{p->model_a, p->offs_a, p->uv_a, p->xyz_a, p->shared_a};
        pair[1] = calib_rig_camera_t{p->model_b, p->offs_b, p->uv_b, p->xyz_b, p->shared_b};
        cams = pair; ncam = 2; M = p->num_views;
    }
    SolverProblem(const calib_rig_problem_t* p) {
        if (p) { cams = p->cameras; ncam = p->num_cameras; M = p->num_views; }
    }
    SolverProblem(const SolverProblem&) = delete;
    SolverProblem& operator=(const SolverProblem&) = delete;
};

// The fixed mask over the shared unknowns, two words everywhere on the host: none, joint stereo's word, the joint rig's two
struct SolverMask {
    uint64_t w[2] = {0, 0};
    SolverMask() = default;
    explicit SolverMask(uint64_t m) : w{m, 0} {}
    explicit SolverMask(const uint64_t* m) { if (m) { w[0] = m[0]; w[1] = m[1]; } }
    bool beyond(int S) const {          // a bit at or above S
        const uint64_t lo = S >= 64 ? 0 : w[0] >> S;
        const uint64_t hi = S >= 128 ? 0 : (S > 64 ? w[1] >> (S - 64) : w[1]);
        return lo || hi;
    }
};

struct StereoRun;

// Everything the host knows about a solver at given models and camera count.
struct StereoSolver {
    int S;                  // shared unknowns: the rig's 6, LA + LB + 6, 6 (N - 1), or sum L_c + 6 (N - 1)
    int record;             // doubles per view record
    int ntot, nschur;       // entries per workgroup partial of the blocks / of the Schur kernel
    int views_a;            // views per workgroup of the blocks kernel
    int (*evaluate)(const StereoRun&);      // blocks at the candidate, then its totals and the decision
    int (*step)(const StereoRun&);          // at the accepted point: Schur complement, shared solve, back-substitution
    const char* singular;                   // the text of the solver's CALIB_E_SINGULAR
    int views_c = 16;                       // views per workgroup pass of the Schur kernel
    int grid_a = 0, grid_c = 0;             // > 0: the blocks / Schur kernel's grid loops over its views, at most so many partials
    bool known_cameras = false;             // the cameras' shared vectors are required and uploaded (else they travel in P)
    bool rig_joint = false;                 // the joint rig's extras: rj, the step's shared part, both mask words as arguments
    int (*evaluate_robust)(const StereoRun&) = nullptr;     // evaluate under the run's loss (the joint rig alone has one)
    int (*residuals)(const StereoRun&, const double*, double*) = nullptr;   // every point's residual at a device P
    RigJointDesc rj{};
    BlockMap map;
};
StereoSolver solver_desc(SolverKind kind, const int* model, int num_cameras);

// One checker. Every entry point keeps the order of its checks: the stereo ones test both models, the view count, the
// shared vectors and the mask before any view; the rig ones the view count, then camera by camera, the mask last.
int check_problem(SolverKind kind, const SolverProblem& pb, const double* P, const SolverMask& mask, StereoSolver& sv) {
    if (!pb.cams || !P) return fail(CALIB_E_INVALID, "null argument");
    if (pb.ncam < 2 || pb.ncam > CALIB_RIG_MAX_CAMERAS) return fail(CALIB_E_INVALID, "a rig has 2 to 8 cameras");
    const bool pair = solver_is_pair(kind);
    auto some_views = [&] {
        return pb.M >= 1 ? CALIB_OK : fail(CALIB_E_INVALID, std::string(pair ? "stereo" : "rig") + " calibration needs at least one view");
    };
    auto model_ok = [&](int c) { return known_model(pb.cams[c].model) ? CALIB_OK : fail(CALIB_E_INVALID, "unknown distortion model"); };
    auto shared_ok = [&](int c) { return solver_is_joint(kind) || pb.cams[c].shared ? CALIB_OK : fail(CALIB_E_INVALID, "null argument"); };
    auto views_ok = [&](int c) { return check_views(pb.M, pb.cams[c].offs, pb.cams[c].uv, pb.cams[c].xyz); };
    auto mask_ok = [&] {                // the models are known by now: S is
        int model[CALIB_RIG_MAX_CAMERAS];
        for (int c = 0; c < pb.ncam; ++c) model[c] = pb.cams[c].model;
        sv = solver_desc(kind, model, pb.ncam);
        return mask.beyond(sv.S) ? fail(CALIB_E_INVALID, "fixed_mask has a bit at or above the number of shared unknowns") : CALIB_OK;
    };
    int rc = CALIB_OK;
    if (pair) {
        for (int c = 0; c < pb.ncam && !rc; ++c) rc = model_ok(c);
        if (!rc) rc = some_views();
        for (int c = 0; c < pb.ncam && !rc; ++c) rc = shared_ok(c);
        if (!rc) rc = mask_ok();
        for (int c = 0; c < pb.ncam && !rc; ++c) rc = views_ok(c);
    } else {
        rc = some_views();
        for (int c = 0; c < pb.ncam && !rc; ++c) {
            rc = model_ok(c);
            if (!rc) rc = shared_ok(c);
            if (!rc) rc = views_ok(c);
        }
        if (!rc) rc = mask_ok();
    }
    return rc;
}

// A word in pinned memory that the device sets when the loop is over. Best effort: without it (or without its device
// address) the host looks at the state instead.
struct DoneWord {
    int* host = nullptr;
    int* dev = nullptr;
    DoneWord() = default;
    DoneWord(const DoneWord&) = delete;
    DoneWord& operator=(const DoneWord&) = delete;
    ~DoneWord() { if (host) (void)hipHostFree(host); }
    void create() {
        void* hp = nullptr; void* dp = nullptr;
        if (hipHostMalloc(&hp, sizeof(int), hipHostMallocMapped) == hipSuccess) {
            host = static_cast<int*>(hp);
            *host = 0;
            if (hipHostGetDevicePointer(&dp, hp, 0) == hipSuccess) dev = static_cast<int*>(dp);
        }
        (void)hipGetLastError();
    }
    bool set() const { return *static_cast<volatile int*>(host) != 0; }
};

// Device side of one call: the problem's cameras (up to CALIB_RIG_MAX_CAMERAS), the two (point, record, total) buffer
// sets the loop alternates between, the state. Released with the scope of the entry point.
struct StereoRun {
    struct Cam {
        DevBuf<int64_t> offs;
        DevBuf<double2> uv;
        DevBuf<double> xyz, shared;         // shared: a known camera (not the joint solvers')
        StereoCam view() const { return StereoCam{offs.p, uv.p, xyz.p}; }
    };
    StereoSolver sv{};
    Cam cam[CALIB_RIG_MAX_CAMERAS];
    DevBuf<double> P[2], rec[2], partA[2], tot, partC, delta, trace;
    DevBuf<double> dshq;                    // the joint rig solver's shared step (StereoState::dsh holds kJMaxS entries)
    SolverMask fixed;                       // over all S shared unknowns
    RigLoss loss{CALIB_LOSS_NONE, 0.0};     // a robust loss: begin() then takes the solver's evaluate_robust
    DevBuf<StereoState> st;
    DoneWord done;
    int64_t M = 0;
    int nwgA = 0, nwgC = 0, ncam = 0, model[CALIB_RIG_MAX_CAMERAS] = {};
    StereoBufs bufs{};

    size_t params() const { return (size_t)sv.S + 6 * (size_t)M; }
    size_t trace_width() const { return (size_t)(CALIB_TRACE_HEADER + sv.S); }

    int upload_cam(int index, const calib_rig_camera_t& cm, int64_t M, bool with_shared) {
        Cam& c = cam[index];
        model[index] = cm.model;
        const int64_t n = cm.offs[M];
        const size_t L = 5 + (size_t)num_distortion(cm.model);
        HIP_TRY(c.offs.alloc((size_t)M + 1));
        HIP_TRY(c.uv.alloc((size_t)std::max<int64_t>(n, 1)));
        HIP_TRY(c.xyz.alloc((size_t)std::max<int64_t>(n, 1) * 3));
        HIP_TRY(hipMemcpy(c.offs.p, cm.offs, ((size_t)M + 1) * 8, hipMemcpyHostToDevice));
        if (n) HIP_TRY(hipMemcpy(c.uv.p, cm.uv, (size_t)n * 16, hipMemcpyHostToDevice));
        if (n) HIP_TRY(hipMemcpy(c.xyz.p, cm.xyz, (size_t)n * 24, hipMemcpyHostToDevice));
        if (with_shared) {
            HIP_TRY(c.shared.alloc(L));
            HIP_TRY(hipMemcpy(c.shared.p, cm.shared, L * 8, hipMemcpyHostToDevice));
        }
        return CALIB_OK;
    }

    // After the cameras: the start point goes into buffer 0, which the bootstrap round evaluates as its candidate (cur = 1)
    int begin(StereoSolver solver, int64_t num_views, const double* P0, const SolverMask& mask, int max_iters, double lam,
              double lam_min, double lam_max, double err_min, bool want_trace, bool want_notify) {
        sv = std::move(solver);
        if (loss.kind != CALIB_LOSS_NONE) {
            if (!sv.evaluate_robust) return fail(CALIB_E_INVALID, "this solver has no robust loss");
            sv.evaluate = sv.evaluate_robust;
        }
        fixed = mask;
        M = num_views;
        nwgA = (int)((M + sv.views_a - 1) / sv.views_a);
        nwgC = (int)((M + sv.views_c - 1) / sv.views_c);
        if (sv.grid_a) nwgA = std::min(nwgA, sv.grid_a);
        if (sv.grid_c) nwgC = std::min(nwgC, sv.grid_c);
        if (sv.rig_joint) {
            HIP_TRY(dshq.alloc((size_t)sv.S));
            HIP_TRY(hipMemset(dshq.p, 0, (size_t)sv.S * 8));
        }
        const size_t K = params();
        for (int s = 0; s < 2; ++s) {
            HIP_TRY(P[s].alloc(K));
            HIP_TRY(rec[s].alloc((size_t)M * sv.record));
            HIP_TRY(partA[s].alloc((size_t)nwgA * sv.ntot));
        }
        HIP_TRY(tot.alloc(2 * (size_t)sv.ntot));
        HIP_TRY(partC.alloc((size_t)nwgC * sv.nschur));
        HIP_TRY(delta.alloc(K));
        HIP_TRY(st.alloc(1));
        HIP_TRY(hipMemcpy(P[0].p, P0, K * 8, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(P[1].p, P0, K * 8, hipMemcpyHostToDevice));
        HIP_TRY(hipMemset(tot.p, 0, 2 * (size_t)sv.ntot * 8));
        if (want_trace) {
            HIP_TRY(trace.alloc((size_t)max_iters * trace_width()));
            HIP_TRY(hipMemset(trace.p, 0, (size_t)max_iters * trace_width() * 8));
        }
        StereoState s{};
        s.lam = lam; s.lam_min = lam_min; s.lam_max = lam_max; s.err_min = err_min;
        s.err_cur = s.last_err = std::nan("");
        s.fixed = sv.rig_joint ? 0 : fixed.w[0];    // the joint rig's kernels take both words as an argument
        s.cur = 1; s.max_iters = max_iters;
        if (want_notify) {
            done.create();
            s.notify = done.dev;
        }
        HIP_TRY(hipMemcpy(st.p, &s, sizeof s, hipMemcpyHostToDevice));
        bufs = StereoBufs{{P[0].p, P[1].p}, {rec[0].p, rec[1].p}, {partA[0].p, partA[1].p}, {tot.p, tot.p + sv.ntot},
                          partC.p, delta.p, trace.p, st.p, M};
        return CALIB_OK;
    }

    int state(StereoState& s) const {
        HIP_TRY(hipMemcpy(&s, st.p, sizeof s, hipMemcpyDeviceToHost));
        return CALIB_OK;
    }
};

// A loss as the robust entry points take it: NULL or CALIB_LOSS_NONE is no loss (the plain entry point serves it, whatever
// the scale says); otherwise the kind is Huber or Cauchy and the scale finite and > 0.
int check_loss(const calib_loss_t* loss) {
    if (loss->kind != CALIB_LOSS_HUBER && loss->kind != CALIB_LOSS_CAUCHY) return fail(CALIB_E_INVALID, "unknown loss kind");
    if (!(std::isfinite(loss->scale) && loss->scale > 0.0)) return fail(CALIB_E_INVALID, "the scale of a loss must be finite and > 0");
    return CALIB_OK;
}
bool loss_is_plain(const calib_loss_t* loss) { return !loss || loss->kind == CALIB_LOSS_NONE; }

// One begin: checks, device, the cameras and the run's buffers with P as the start point
int solver_begin(StereoRun& run, SolverKind kind, const SolverProblem& pb, const double* P, const SolverMask& mask, int max_iters,
                 double lam, double lam_min, double lam_max, double err_min, bool want_trace, bool want_notify, int device_id,
                 const calib_loss_t* loss = nullptr) {
    StereoSolver sv{};
    int rc = loss_is_plain(loss) ? CALIB_OK : check_loss(loss);
    if (rc) return rc;
    if (!loss_is_plain(loss)) run.loss = RigLoss{loss->kind, loss->scale};
    rc = check_problem(kind, pb, P, mask, sv);
    if (rc) return rc;
    rc = use_device(device_id);
    if (rc) return rc;
    run.ncam = pb.ncam;
    for (int c = 0; c < pb.ncam; ++c) {
        rc = run.upload_cam(c, pb.cams[c], pb.M, sv.known_cameras);
        if (rc) return rc;
    }
    return run.begin(std::move(sv), pb.M, P, mask, max_iters, lam, lam_min, lam_max, err_min, want_trace, want_notify);
}

// the blocks at P on the host: every view's record and the totals
int run_blocks(StereoRun& run, std::vector<double>& rec, std::vector<double>& tot) {
    int rc = run.sv.evaluate(run);
    if (rc) return rc;
    rec.resize((size_t)run.M * run.sv.record);
    tot.resize((size_t)run.sv.ntot);
    HIP_TRY(hipMemcpy(rec.data(), run.rec[0].p, rec.size() * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(tot.data(), run.tot.p, tot.size() * 8, hipMemcpyDeviceToHost));
    return CALIB_OK;
}

// one step from a run begun with lambda
int run_step_delta(StereoRun& run, double* out_delta) {
    int rc = run.sv.evaluate(run);
    if (rc) return rc;
    rc = run.sv.step(run);
    if (rc) return rc;
    StereoState s;
    rc = run.state(s);
    if (rc) return rc;
    if (s.error) return fail(CALIB_E_SINGULAR, run.sv.singular);
    if (out_delta) HIP_TRY(hipMemcpy(out_delta, run.delta.p, run.params() * 8, hipMemcpyDeviceToHost));
    return CALIB_OK;
}

// the loop of a run begun with its start point; out_sse_cam: the error per camera at the returned point
int run_refine(StereoRun& run, double* P_inout, int max_iters, double* out_sse, double* out_sse_cam, int* out_iters,
               double* out_trace) {
    int rc;
    // round 0 evaluates the start point; round r >= 1 decides iteration r - 1. The host runs ahead of the device: the
    // done word in pinned memory stops the enqueueing (rounds already in the queue return at once); without such a word,
    // a synchronised look at the state every 8 rounds.
    StereoState s;
    for (int r = 0; r <= max_iters; ++r) {
        rc = run.sv.evaluate(run);
        if (rc) return rc;
        rc = run.sv.step(run);
        if (rc) return rc;
        if (run.done.host) {
            if (run.done.set()) break;
        } else if ((r + 1) % 8 == 0) {
            rc = run.state(s);
            if (rc) return rc;
            if (s.done) break;
        }
    }
    rc = run.state(s);
    if (rc) return rc;
    if (s.error) return fail(CALIB_E_SINGULAR, run.sv.singular);
    HIP_TRY(hipMemcpy(P_inout, run.P[s.cur].p, run.params() * 8, hipMemcpyDeviceToHost));
    if (out_sse) *out_sse = s.last_err;
    if (out_iters) *out_iters = s.iters;
    if (out_sse_cam)    // the cameras' errors end the totals
        HIP_TRY(hipMemcpy(out_sse_cam, run.tot.p + (size_t)s.cur * run.sv.ntot + (run.sv.ntot - run.ncam), (size_t)run.ncam * 8,
                          hipMemcpyDeviceToHost));
    if (out_trace && s.iters > 0)
        HIP_TRY(hipMemcpy(out_trace, run.trace.p, (size_t)s.iters * run.trace_width() * 8, hipMemcpyDeviceToHost));
    return CALIB_OK;
}

// ---- the three drivers behind the twelve entry points ------------------------------------------------------------------
int solver_normal_eq(SolverKind kind, const SolverProblem& pb, const double* P, double* out_B, double* out_E, double* out_V,
                     double* out_g, double* out_sse_cam, int device_id, const calib_loss_t* loss = nullptr) {
    StereoRun run;
    std::vector<double> rec, tot;
    int rc = solver_begin(run, kind, pb, P, SolverMask(), 1, 0.0, 0.0, 0.0, 0.0, false, false, device_id, loss);
    if (rc) return rc;
    rc = run_blocks(run, rec, tot);
    if (rc) return rc;
    unpack_blocks(run.sv.map, run.M, tot.data(), rec.data(), out_B, out_E, out_V, out_g, out_sse_cam);
    return CALIB_OK;
}

int solver_step_delta(SolverKind kind, const SolverProblem& pb, const double* P, const SolverMask& mask, double lambda,
                      double* out_delta, int device_id, const calib_loss_t* loss = nullptr) {
    StereoRun run;
    const int rc = solver_begin(run, kind, pb, P, mask, 1, lambda, 0.0, 0.0, 0.0, false, false, device_id, loss);
    return rc ? rc : run_step_delta(run, out_delta);
}

int solver_refine(SolverKind kind, const SolverProblem& pb, double* P_inout, const SolverMask& mask, int max_iters,
                  double lam_init, double lam_min, double lam_max, double err_min, double* out_sse, double* out_sse_cam,
                  int* out_iters, double* out_trace, int device_id, const calib_loss_t* loss = nullptr) {
    if (max_iters <= 0) return fail(CALIB_E_INVALID, "max_iters must be >= 1");
    StereoRun run;
    const int rc = solver_begin(run, kind, pb, P_inout, mask, max_iters, lam_init, lam_min, lam_max, err_min,
                                out_trace != nullptr, true, device_id, loss);
    return rc ? rc : run_refine(run, P_inout, max_iters, out_sse, out_sse_cam, out_iters, out_trace);
}

// every point's residual at P, the cameras one after the other: no loop, no buffers but the cameras, P and the result
int solver_residuals(SolverKind kind, const SolverProblem& pb, const double* P, double* out_res, int device_id) {
    StereoRun run;
    int rc = check_problem(kind, pb, P, SolverMask(), run.sv);
    if (rc) return rc;
    if (!out_res) return fail(CALIB_E_INVALID, "null argument");
    if (!run.sv.residuals) return fail(CALIB_E_INVALID, "this solver has no residual kernel");
    rc = use_device(device_id);
    if (rc) return rc;
    run.ncam = pb.ncam;
    run.M = pb.M;
    size_t n = 0;
    for (int c = 0; c < pb.ncam; ++c) {
        rc = run.upload_cam(c, pb.cams[c], pb.M, run.sv.known_cameras);
        if (rc) return rc;
        n += (size_t)pb.cams[c].offs[pb.M];
    }
    if (!n) return CALIB_OK;
    DevBuf<double> res;
    HIP_TRY(run.P[0].alloc(run.params()));
    HIP_TRY(res.alloc(2 * n));
    HIP_TRY(hipMemcpy(run.P[0].p, P, run.params() * 8, hipMemcpyHostToDevice));
    rc = run.sv.residuals(run, run.P[0].p, res.p);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(out_res, res.p, 2 * n * 8, hipMemcpyDeviceToHost));
    return CALIB_OK;
}

}  // namespace
