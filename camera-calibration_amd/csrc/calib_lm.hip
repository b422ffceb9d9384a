// C-ABI host side of the LM refinement engine (see include/calib_lm.h).
// Owns device memory, packs correspondences to SoA, sequences the kernels of kernels.hpp.
#include "../../include/calib_lm.h"
#include "kernels.hpp"
#include "undistort.hpp"
#include "stereo.hpp"
#include "stereo_joint.hpp"
#include "rig.hpp"
#include "rig_joint.hpp"
#include "rectify.hpp"
#include "triangulate_multi.hpp"
#include "host_rows.hpp"
#include "launch_plan.hpp"
#include "shard_layout.hpp"

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <dlfcn.h>
#include <chrono>
#include <future>
#include <memory>
#include <mutex>
#include <thread>
#include <cstring>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

using namespace calib;

namespace {

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

#define HIP_TRY(expr)                                                                         \
    do {                                                                                      \
        hipError_t e__ = (expr);                                                              \
        if (e__ != hipSuccess)                                                                \
            return fail(CALIB_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e__));     \
    } while (0)

// after a kernel launch: a launch-time failure is reported with the kernel's name, and the name is remembered so
// that an ASYNCHRONOUS fault -- seen only at a later synchronisation -- can say what was in flight
#define LAUNCHED(h, name)                                                                     \
    do {                                                                                      \
        if (h) (h)->noteKernel(name);                                                         \
        hipError_t e__ = hipGetLastError();                                                   \
        if (e__ != hipSuccess)                                                                \
            return fail(CALIB_E_HIP, std::string("launch of ") + (name) + ": " + hipGetErrorString(e__)); \
    } while (0)

#define SYNC_H(h)                                                                             \
    do {                                                                                      \
        hipError_t e__ = hipStreamSynchronize((h)->stream);                                   \
        if (e__ != hipSuccess)                                                                \
            return fail(CALIB_E_HIP, std::string("hipStreamSynchronize: ") + hipGetErrorString(e__) + \
                                     " (kernels enqueued since the last successful synchronisation: " + (h)->recentKernels() + ")"); \
        (h)->kernels_since_sync.clear();                                                      \
    } while (0)

#define CHECK_H(h)                                                                            \
    if (!(h)) return fail(CALIB_E_INVALID, "null handle");                                    \
    HIP_TRY(hipSetDevice((h)->device))

// Device allocation owned by its scope: every early return of an entry point (HIP_TRY) releases it.
template <typename U>
struct DevBuf {
    U* p = nullptr;
    size_t n = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    hipError_t alloc(size_t count) {
        if (count <= n && p) return hipSuccess;
        release();
        if (count == 0) return hipSuccess;
        const hipError_t e = hipMalloc((void**)&p, count * sizeof(U));
        if (e != hipSuccess) return e;
        n = count;
        return hipSuccess;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
};

constexpr int kEventPool = 32768;

}  // namespace

struct calib_handle_s {
    // names of the kernels enqueued since the last successful synchronisation (distinct, in first-use order)
    std::vector<const char*> kernels_since_sync;
    void noteKernel(const char* name) {
        for (const char* k : kernels_since_sync) if (k == name) return;
        if (kernels_since_sync.size() < 16) kernels_since_sync.push_back(name);
    }
    std::string recentKernels() const {
        std::string r;
        for (const char* k : kernels_since_sync) { if (!r.empty()) r += ", "; r += k; }
        return r.empty() ? "none" : r;
    }
    int model = 0, dtype = 0, device = 0;
    int L = 10, C = 16;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;

    // problem
    bool has_problem = false;
    int64_t M = 0, MN = 0;        // external views, points
    int nv = 0;                   // non-empty views
    int n_items = 0;
    int64_t n_tiles = 0;
    int max_views_per_tile = 1;
    int uniform_n = 0;            // > 0: every item is one whole view of exactly this many points, in order (item i = view i = points [i n, (i+1) n))
    Knobs knobs;                  // CALIB_* tuning variables (calib_create)
    LaunchPlan plan;              // kernel forms and grids of this problem's LM rounds (plan_of)
    std::vector<ShardChunk> chunks;   // of the two-kernel rounds (shard_layout.hpp)
    int64_t max_chunk_points = 0;
    DevBuf<unsigned char> uv, XY, Z, VC, J, r, y;   // typed by dtype: the launches read them through the accessors
    template <typename U> static U* as(const DevBuf<unsigned char>& b) { return reinterpret_cast<U*>(b.p); }
    template <typename U> U* uv_as() const { return as<U>(uv); }
    template <typename U> U* XY_as() const { return as<U>(XY); }
    template <typename U> U* Z_as() const { return as<U>(Z); }
    template <typename U> U* VC_as() const { return as<U>(VC); }
    template <typename U> U* J_as() const { return as<U>(J); }
    template <typename U> U* r_as() const { return as<U>(r); }
    template <typename U> U* y_as() const { return as<U>(y); }
    DevBuf<int> pt_view, view_ext, item_n, view_item0, item_view;
    DevBuf<uint32_t> emit_tab;    // fused kernel's record assembly table (buildEmitTable)
    DevBuf<int32_t> stream_ops;   // fused_stream_kernel's per-lane record offsets (buildStreamOps)
    int lm_mode = CALIB_LM_FUSED;
    uint32_t fixed_mask = 0;      // shared parameters the LM holds fixed (calib_set_fixed_shared); read by calib_lm_begin
    int num_cus = 256;
    DevBuf<int64_t> item_pt0;
    DevBuf<double> sse_part, G[2], bpart, part, red_own, P[2], Peval, trace;
    int n_bpart = 0;              // workgroup partials of the shared block written by this round's pass
    DevBuf<LMState> st, st_eval;
    double* red = nullptr;        // active reduce buffer (own or bound)
    void* comm = nullptr;         // RCCL communicator of the in-library all-reduce (calib_rccl_init), or null
    DevBuf<double> rccl_test;     // operand of calib_rccl_selftest: outlives a collective that timed out
    int comm_ranks = 0, comm_rank = 0;
    // peer exchange over xGMI (calib_peer_*): the reduce kernel sums over the ranks itself
    void* peer_mem = nullptr;             // this rank's slot memory (uncached / fine-grained device memory)
    std::vector<void*> peer_open;         // IPC mappings of the other ranks' slot memory
    DevBuf<unsigned long long*> peer_slots;
    std::vector<unsigned long long*> peer_slot_host;     // the same pointers, for the kernel arguments
    DevBuf<int> peer_flags;               // [0] a spin timed out, [1] self-test mismatches
    int peer_world = 0, peer_rank = 0;
    unsigned peer_epoch = 0;
    double peer_timeout_s = 60.0;
    bool peer_connected = false;
    bool exchange_round = false;          // the round being enqueued belongs to a sharded run
    int* host_done = nullptr;             // pinned, device-visible: 1 = the update kernel says the LM loop is over, 2 = a peer exchange gave up
    int* host_done_dev = nullptr;         // the same word as the device sees it
    bool lm_active = false;
    int lm_max_iters = 0;
    int rounds_enqueued = 0;

    // uncertainty (calib_view_errors, calib_cov_*)
    bool cov_pending = false;             // calib_cov_local has run its lambda = 0 round; calib_cov_finish is due
    std::vector<int64_t> ext_offsets;     // the caller's view_offsets (M + 1), uploaded by the first calib_view_errors
    bool ext_offsets_on_device = false;
    DevBuf<int64_t> ext_offsets_dev;
    DevBuf<double> view_err, cov_css, cov_views, cov_cross;
    DevBuf<int> cov_flag;

    // pinned staging of calib_set_problem's uploads (upload_staged)
    bool stage_ready = false;
    void* stage_pinned = nullptr;
    hipStream_t stage_stream[4] = {nullptr, nullptr, nullptr, nullptr};
    void* stage_buf[4][2] = {{nullptr, nullptr}, {nullptr, nullptr}, {nullptr, nullptr}, {nullptr, nullptr}};
    hipEvent_t stage_ev[4][2] = {{nullptr, nullptr}, {nullptr, nullptr}, {nullptr, nullptr}, {nullptr, nullptr}};

    // profiling
    bool prof = false;
    int prof_stride = 1;          // every prof_stride-th launch of a kernel kind is timed
    int64_t prof_seen[3] = {0, 0, 0};
    std::vector<hipEvent_t> ev;   // pairs
    std::vector<int> ev_kind;
    size_t ev_used = 0;
};

namespace {

size_t tsize(const calib_handle_s* h) { return h->dtype == CALIB_DTYPE_F64 ? 8 : 4; }

// Profiled launches (calib_profile_enable): every prof_stride-th launch of a kernel kind gets a HIP event pair that
// rides on the kernel's own dispatch (hipExtLaunchKernelGGL: the events take the kernel's begin and end timestamps).
// Recording stream markers around the launch instead put two more packets into the queue, kept the launch from
// being dispatched back to back with its neighbours and read ~3 us long on a 45 us kernel.
int prof_reserve(calib_handle_s* h, int kind) {
    if (!h->prof || h->ev_used + 2 > h->ev.size()) return -1;
    if (h->prof_seen[kind]++ % h->prof_stride != 0) return -1;
    int idx = (int)h->ev_used;
    h->ev_used += 2;
    h->ev_kind[idx / 2] = kind;
    return idx;
}

template <typename F, typename... Args>
void launch_kind(calib_handle_s* h, int kind, F kernel, dim3 grid, dim3 block, size_t shmem, Args... args) {
    const int idx = prof_reserve(h, kind);
    if (idx >= 0)
        hipExtLaunchKernelGGL(kernel, grid, block, (uint32_t)shmem, h->stream, h->ev[(size_t)idx], h->ev[(size_t)idx + 1], 0, args...);
    else
        hipLaunchKernelGGL(kernel, grid, block, shmem, h->stream, args...);
}

calib_handle_s* const kNoHandle = nullptr;      // LAUNCHED of the entry points that take no handle

// ---- form dispatch -----------------------------------------------------------------------
// A run-time (model, dtype) as compile-time arguments: f is a generic lambda that gets a Form value and reads MODEL,
// L, C, T and T2 from its type. A launch names only what its kernel takes, so the kernels instantiated are the ones a
// ladder at the site would spell out -- in the ladders' order (storage type, then model), which keeps the module's
// kernels, and the numbering of their labels, where they were. The stream form of the per-view kernels (plan.stream())
// stays a branch at its three sites for the same reason: there it alternates inside a (model, dtype) form.
static_assert(CALIB_MODEL_RADTAN == kRadtan && CALIB_MODEL_FISHEYE == kFisheye, "the C ABI's model ids are the kernels'");
template <int MODEL_, typename T_>
struct Form {
    static constexpr int MODEL = MODEL_, L = ModelTraits<MODEL_>::L, C = ModelTraits<MODEL_>::C;
    using T = T_;
    using T2 = typename Pair<T_>::type;
};

template <typename F>
int dispatch(int model, int dtype, F&& f) {
    auto byModel = [&](auto t) -> int { return model == kRadtan ? f(Form<kRadtan, decltype(t)>{}) : f(Form<kFisheye, decltype(t)>{}); };
    return dtype == CALIB_DTYPE_F64 ? byModel(double{}) : byModel(float{});
}
template <typename F>
int dispatch(const calib_handle_s* h, F&& f) { return dispatch(h->model, h->dtype, f); }
// entry points without a handle: fp64, the model alone
template <typename F>
int dispatch_model(int model, F&& f) { return dispatch(model, CALIB_DTYPE_F64, f); }

bool known_model(int model) { return model == CALIB_MODEL_RADTAN || model == CALIB_MODEL_FISHEYE; }
int num_distortion(int model) { return model == CALIB_MODEL_RADTAN ? 5 : 4; }

// ---- undistortion entry points' helpers ----------------------------------------------------
// alpha, beta, gamma, uc, vc of a row-major (3,3) camera matrix; false when it cannot be inverted
bool pinhole_of(const double* A, Pinhole& p) {
    p.al = A[0]; p.ga = A[1]; p.uc = A[2]; p.be = A[4]; p.vc = A[5];
    return p.al != 0.0 && p.be != 0.0;
}

template <typename T>
int remap_typed(const void* src, int src_h, int src_w, int channels, const float* mapx, const float* mapy, int dst_h,
                int dst_w, double border, void* dst) {
    const size_t nsrc = (size_t)src_h * src_w * channels, npix = (size_t)dst_h * dst_w, ndst = npix * channels;
    DevBuf<T> dsrc, ddst;
    DevBuf<float> dmx, dmy;
    HIP_TRY(dsrc.alloc(nsrc)); HIP_TRY(ddst.alloc(ndst)); HIP_TRY(dmx.alloc(npix)); HIP_TRY(dmy.alloc(npix));
    HIP_TRY(hipMemcpy(dsrc.p, src, nsrc * sizeof(T), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dmx.p, mapx, npix * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dmy.p, mapy, npix * 4, hipMemcpyHostToDevice));
    const dim3 grid((unsigned)((dst_h + kRemapRows - 1) / kRemapRows), (unsigned)((dst_w + 63) / 64)), block(64, kRemapRows);
    auto launch = [&](auto c) -> int {
        hipLaunchKernelGGL((remap_kernel<T, decltype(c)::value>), grid, block, 0, 0, (const T*)dsrc.p, src_h, src_w,
                           (const float*)dmx.p, (const float*)dmy.p, dst_h, dst_w, (float)border, ddst.p);
        LAUNCHED(kNoHandle, "remap_kernel");
        return CALIB_OK;
    };
    const int rc = channels == 1 ? launch(std::integral_constant<int, 1>{})
                 : channels == 2 ? launch(std::integral_constant<int, 2>{})
                 : channels == 3 ? launch(std::integral_constant<int, 3>{})
                                 : launch(std::integral_constant<int, 4>{});
    if (rc) return rc;
    HIP_TRY(hipMemcpy(dst, ddst.p, ndst * sizeof(T), hipMemcpyDeviceToHost));
    return CALIB_OK;
}

// ---- RCCL, resolved at run time (calib_rccl_load) ------------------------------------------
// Only the handful of entry points the one all-reduce needs; types as in rccl.h (ncclUniqueId is 128
// opaque bytes passed by value, ncclDouble = 8, ncclSum = 0, ncclSuccess = 0).
struct RcclId { char internal[128]; };
struct RcclApi {
    void* lib = nullptr;
    int (*getUniqueId)(RcclId*) = nullptr;
    int (*commInitRank)(void**, int, RcclId, int) = nullptr;
    int (*allReduce)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
    int (*commDestroy)(void*) = nullptr;
    int (*commAbort)(void*) = nullptr;
    const char* (*getErrorString)(int) = nullptr;
};
RcclApi g_rccl;                 // written once under g_rccl_mutex (calib_rccl_load), read-only afterwards
std::mutex g_rccl_mutex;
constexpr int kNcclDouble = 8, kNcclSum = 0;

int rccl_fail(const char* what, int rc) {
    return fail(CALIB_E_HIP, std::string(what) + ": " +
                             (g_rccl.getErrorString ? g_rccl.getErrorString(rc) : "RCCL error") + " (" + std::to_string(rc) + ")");
}

// ---- host -> device copies of large caller arrays --------------------------------------------
// Pageable memory goes over PCIe at ~8 GB/s through hipMemcpy. Here kUploadThreads host threads copy
// alternating 1 MiB chunks into their own pair of pinned buffers and DMA them from there on the handle's stream:
// the host memcpy of one chunk overlaps the DMA of the previous ones (measured: 31-40 GB/s). The pinned memory
// is one 8 MiB allocation per handle -- pinning costs ~0.3 ms per MiB, paid by the handle's first upload.
constexpr int kUploadThreads = 4;
constexpr size_t kUploadChunk = (size_t)1 << 20;

int upload_staged(calib_handle_s* h, void* dst, const HostRows& src, size_t bytes) {
    if (bytes == 0) return CALIB_OK;
    if (bytes < 2 * kUploadChunk) {
        if (src.flat) {
            HIP_TRY(hipMemcpy(dst, src.flat, bytes, hipMemcpyHostToDevice));
        } else {
            std::vector<char> tmp(bytes);
            src.copy(tmp.data(), 0, bytes);
            HIP_TRY(hipMemcpy(dst, tmp.data(), bytes, hipMemcpyHostToDevice));
        }
        return CALIB_OK;
    }
    if (!h->stage_ready) {
        HIP_TRY(hipHostMalloc(&h->stage_pinned, 2 * kUploadThreads * kUploadChunk, hipHostMallocDefault));
        for (int t = 0; t < kUploadThreads; ++t) {
            h->stage_stream[t] = h->own_stream;       // one DMA queue saturates the link; creating streams costs ms each
            for (int b = 0; b < 2; ++b) {
                h->stage_buf[t][b] = static_cast<char*>(h->stage_pinned) + (size_t)(2 * t + b) * kUploadChunk;
                HIP_TRY(hipEventCreateWithFlags(&h->stage_ev[t][b], hipEventDisableTiming));
            }
        }
        h->stage_ready = true;
    }
    const size_t nchunks = (bytes + kUploadChunk - 1) / kUploadChunk;
    auto copyShare = [&](int t) -> hipError_t {       // thread t: chunks t, t + kUploadThreads, ...
        if (hipError_t e = hipSetDevice(h->device)) return e;
        size_t use = 0;
        for (size_t c = (size_t)t; c < nchunks; c += kUploadThreads, ++use) {
            const int b = (int)(use & 1);
            const size_t off = c * kUploadChunk, n = std::min(kUploadChunk, bytes - off);
            if (use >= 2)                                                       // this buffer's previous DMA is done
                if (hipError_t e = hipEventSynchronize(h->stage_ev[t][b])) return e;
            src.copy(static_cast<char*>(h->stage_buf[t][b]), off, n);
            if (hipError_t e = hipMemcpyAsync(static_cast<char*>(dst) + off, h->stage_buf[t][b], n, hipMemcpyHostToDevice,
                                              h->stage_stream[t])) return e;
            if (hipError_t e = hipEventRecord(h->stage_ev[t][b], h->stage_stream[t])) return e;
        }
        return hipStreamSynchronize(h->stage_stream[t]);
    };
    hipError_t errs[kUploadThreads];
    std::thread workers[kUploadThreads];
    for (int t = 0; t < kUploadThreads; ++t) workers[t] = std::thread([&errs, &copyShare, t]() { errs[t] = copyShare(t); });
    for (auto& w : workers) w.join();
    for (int t = 0; t < kUploadThreads; ++t)
        if (errs[t] != hipSuccess) return fail(CALIB_E_HIP, std::string("staged upload: ") + hipGetErrorString(errs[t]));
    return CALIB_OK;
}

// ---- launches ---------------------------------------------------------------------------
int launch_jacobian(calib_handle_s* h, const double* P0, const double* P1, const LMState* st, int sel,
                    bool wantJ, bool wantR, bool wantY, bool wantSse, int64_t p_begin, int64_t p_end) {
    if (p_end <= p_begin) return CALIB_OK;
    return dispatch(h, [&](auto form) -> int {
        using F = decltype(form);
        using T = typename F::T;
        using T2 = typename F::T2;
        JacArgs<T> a;
        a.P0 = P0; a.P1 = P1; a.st = st; a.sel = sel;
        a.uv = h->uv_as<const T2>();
        a.XY = h->XY_as<const T2>();
        a.Z = h->Z_as<const T>();
        a.pt_view = h->pt_view.p;
        a.p_begin = p_begin;
        a.p_end = p_end;
        a.VC = h->VC_as<const T>();
        a.J = wantJ ? h->J_as<T2>() : nullptr;
        a.r = wantR ? h->r_as<T2>() : nullptr;
        a.y = wantY ? h->y_as<T2>() : nullptr;
        a.sse_part = wantSse ? h->sse_part.p : nullptr;
        const size_t lds = 32 + (size_t)h->max_views_per_tile * kViewStride * sizeof(T);
        const unsigned tiles = (unsigned)((p_end - p_begin + kTile - 1) / kTile);
        launch_kind(h, 0, jacobian_kernel<F::MODEL, T>, dim3(tiles), dim3(kTile), lds, a);
        LAUNCHED(h, "jacobian_kernel");
        return CALIB_OK;
    });
}

int launch_view_setup(calib_handle_s* h, const double* P0, const double* P1, const LMState* st, int sel) {
    if (h->nv == 0) return CALIB_OK;
    const int threads = 64;
    const int blocks = (h->nv + threads - 1) / threads;
    return dispatch(h, [&](auto form) -> int {
        using T = typename decltype(form)::T;
        hipLaunchKernelGGL((view_setup_kernel<T>), dim3(blocks), dim3(threads), 0, h->stream, P0, P1, st, sel,
                           h->L, h->view_ext.p, h->nv, h->VC_as<T>());
        LAUNCHED(h, "view_setup_kernel");
        return CALIB_OK;
    });
}

int launch_gram(calib_handle_s* h, const LMState* st, int sel, int item0, int item1, int64_t origin) {
    if (item1 <= item0) return CALIB_OK;
    const int ipb = 4 / h->plan.gram_wpi;  // items per workgroup
    const int blocks = (item1 - item0 + ipb - 1) / ipb;
    return dispatch(h, [&](auto form) -> int {
        using F = decltype(form);
        using T2 = typename F::T2;
        launch_kind(h, 1, gram_kernel<typename F::T, F::C>, dim3(blocks), dim3(256), 0, h->J_as<const T2>(), h->r_as<const T2>(),
                    (const int64_t*)h->item_pt0.p, (const int*)h->item_n.p, item0, item1, origin, h->plan.gram_wpi, st, sel, h->G[0].p,
                    h->G[1].p, h->bpart.p, h->n_bpart);
        h->n_bpart += blocks;                  // the chunk's workgroups append their partials
        LAUNCHED(h, "gram_kernel");
        return CALIB_OK;
    });
}

// records of this problem's fused rounds: stream form (view records + one overflow record per wave) or one per item
StreamMap stream_map(const calib_handle_s* h) {
    StreamMap sm;
    sm.share = h->plan.stream_share;
    sm.n4 = h->uniform_n / 4;
    sm.nv = h->nv;
    return sm;
}
int num_records(const calib_handle_s* h) { return std::max(h->n_items, 1) + h->plan.stream_waves; }

int launch_fused(calib_handle_s* h, const LMState* st, int sel) {
    const LaunchPlan& p = h->plan;
    if (p.fused == FusedForm::Stream)           // fp64 only (makePlan)
        return dispatch(h, [&](auto form) -> int {
            launch_kind(h, 2, fused_stream_kernel<decltype(form)::MODEL>, dim3(p.fused_blocks), dim3(256), 0,
                        (const double*)h->P[0].p, (const double*)h->P[1].p, h->uv_as<const double2>(), h->XY_as<const double2>(),
                        h->Z_as<const double>(), h->VC_as<const double>(), h->uniform_n, h->nv, p.stream_share,
                        (const uint32_t*)h->emit_tab.p, (const int32_t*)h->stream_ops.p, st, sel, h->G[0].p, h->G[1].p, h->bpart.p);
            h->n_bpart = p.fused_blocks;
            LAUNCHED(h, "fused_stream_kernel");
            return CALIB_OK;
        });
    if (p.fused_blocks == 0) return CALIB_OK;
    return dispatch(h, [&](auto form) -> int {
        using F = decltype(form);
        using T = typename F::T;
        using T2 = typename F::T2;
        auto launch = [&](auto kernel) {
            launch_kind(h, 2, kernel, dim3(p.fused_blocks), dim3(256), 0, (const double*)h->P[0].p, (const double*)h->P[1].p,
                        h->uv_as<const T2>(), h->XY_as<const T2>(), h->Z_as<const T>(), h->VC_as<const T>(),
                        (const int64_t*)h->item_pt0.p, (const int*)h->item_n.p, (const int*)h->item_view.p, h->n_items,
                        h->uniform_n, p.ipw, p.fused_wpi, (const uint32_t*)h->emit_tab.p, st, sel, h->G[0].p, h->G[1].p,
                        h->bpart.p);
        };
        if (p.fused == FusedForm::Tile) launch(fused_kernel<F::MODEL, T, false, false>);
        else if (p.fused == FusedForm::TileMulti) launch(fused_kernel<F::MODEL, T, false, true>);
        else if constexpr (sizeof(T) == 8) launch(fused_kernel<F::MODEL, T, true, false>);    // Block44: fp64 only
        h->n_bpart = p.fused_blocks;
        LAUNCHED(h, "fused_kernel");
        return CALIB_OK;
    });
}

// per-view kernels skip the view -> item indirection when every view is a single item
const int* view_items(const calib_handle_s* h) { return h->n_items == h->nv ? nullptr : h->view_item0.p; }

// arguments of the next peer exchange: every rank enqueues the same sequence of exchanges, so the epoch
// counters advance in lockstep
PeerExchange next_exchange(calib_handle_s* h) {
    PeerExchange x;
    x.slots = h->peer_slots.p;
    for (int r = 0; r < kPeerInline; ++r) x.slot8[r] = r < (int)h->peer_slot_host.size() ? h->peer_slot_host[(size_t)r] : nullptr;
    x.fault = h->peer_flags.p;
    x.notify = h->host_done_dev;
    x.timeout_ticks = (unsigned long long)(h->peer_timeout_s * 1e8);      // wall_clock64 counts at 100 MHz
    x.epoch = ++h->peer_epoch;
    x.world = h->peer_world;
    x.rank = h->peer_rank;
    return x;
}

int launch_schur(calib_handle_s* h, const LMState* st) {
    const LaunchPlan& p = h->plan;
    return dispatch(h, [&](auto form) -> int {
        using F = decltype(form);
        auto launch = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, dim3(p.schur_blocks, 3), dim3(kSchurBlock), 0, h->stream, h->G[0].p, h->G[1].p, st,
                               view_items(h), h->nv, stream_map(h), h->bpart.p, h->n_bpart, h->part.p);
        };
        if (p.stream()) { if (p.wide_heads) launch(schur_kernel<F::L, true, true>); else launch(schur_kernel<F::L, false, true>); }
        else { if (p.wide_heads) launch(schur_kernel<F::L, true, false>); else launch(schur_kernel<F::L, false, false>); }
        LAUNCHED(h, "schur_kernel");
        return CALIB_OK;
    });
}

int launch_schur_reduce(calib_handle_s* h, const LMState* st, double* red) {
    const int VA = variantSize(h->L);
    if (h->nv > 0) {
        const int rc = launch_schur(h, st);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(reduce_kernel, dim3(2 * VA), dim3(64), 0, h->stream, h->part.p,
                       h->nv > 0 ? h->plan.schur_blocks : 0, VA, st, red,
                       h->exchange_round ? next_exchange(h) : PeerExchange{});
    LAUNCHED(h, "reduce_kernel");
    return CALIB_OK;
}

// the LM state is double-buffered per round: kernels of round r read st[r & 1], the update kernel
// writes st[(r + 1) & 1]
LMState* st_cur(calib_handle_s* h) { return h->st.p + (h->rounds_enqueued & 1); }
LMState* st_next(calib_handle_s* h) { return h->st.p + ((h->rounds_enqueued + 1) & 1); }

int launch_update_backsub(calib_handle_s* h) {
    const LaunchPlan& p = h->plan;
    return dispatch(h, [&](auto form) -> int {
        using F = decltype(form);
        using T = typename F::T;
        UpdArgs<T> a;
        a.G0 = h->G[0].p; a.G1 = h->G[1].p;
        a.st_in = st_cur(h); a.st_out = st_next(h);
        a.red = h->red;
        a.view_item0 = view_items(h);
        a.view_ext = h->view_ext.p;
        a.nv = h->nv;
        a.sm = stream_map(h);
        a.P0 = h->P[0].p; a.P1 = h->P[1].p;
        a.trace = h->trace.p;
        a.VC = h->VC_as<T>();
        auto launch = [&](auto kernel, int threads, const char* name) -> int {
            hipLaunchKernelGGL(kernel, dim3(p.update_blocks), dim3(threads), 0, h->stream, a);
            LAUNCHED(h, name);
            return CALIB_OK;
        };
        constexpr int L = F::L;
        if (p.update == UpdateForm::Small)
            return p.stream() ? launch(update_backsub_small_kernel<L, T, true>, kUpdThreads, "update_backsub_small_kernel")
                              : launch(update_backsub_small_kernel<L, T, false>, kUpdThreads, "update_backsub_small_kernel");
        if (p.update == UpdateForm::Lane)
            return p.stream() ? launch(update_backsub_lane_kernel<L, T, true>, kSchurThreads, "update_backsub_lane_kernel")
                              : launch(update_backsub_lane_kernel<L, T, false>, kSchurThreads, "update_backsub_lane_kernel");
        return p.stream() ? launch(update_backsub_kernel<L, T, true>, kSchurThreads, "update_backsub_kernel")
                          : launch(update_backsub_kernel<L, T, false>, kSchurThreads, "update_backsub_kernel");
    });
}

LaunchPlan plan_of(const calib_handle_s* h) {
    ShardShape s;
    s.nv = h->nv; s.n_items = h->n_items; s.uniform_n = h->uniform_n; s.MN = h->MN;
    return makePlan(s, h->dtype, h->lm_mode, h->knobs, h->num_cus);
}

int need_problem(calib_handle_s* h) {
    if (!h->has_problem) return fail(CALIB_E_STATE, "calib_set_problem has not been called");
    return CALIB_OK;
}

int64_t numParams(const calib_handle_s* h) { return h->L + 6 * h->M; }

// ---- calib_set_problem -------------------------------------------------------------------
// CALIB_TIMING: stage times of calib_set_problem on stderr
struct Laps {
    bool on;
    double mark = now();
    static double now() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
    void operator()(const char* what) {
        if (!on) return;
        const double t = now();
        std::fprintf(stderr, "  set_problem %-28s %.3f ms\n", what, t - mark);
        mark = t;
    }
};

int upload(void* dst, const void* src, size_t bytes) {
    if (bytes) HIP_TRY(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
    return CALIB_OK;
}

// Everything O(points) -- the AoS -> SoA split, the storage-type conversion, the point -> view index -- happens on
// the device, from the caller's arrays uploaded as they are.
int pack_points(calib_handle_s* h, const ShardLayout& lay, const HostRows& sensor_uv, const HostRows& model_xyz, Laps& lap) {
    const int64_t MN = h->MN;
    DevBuf<double> xyz_stage, uv_stage;
    DevBuf<int64_t> dvoffs;
    HIP_TRY(xyz_stage.alloc((size_t)MN * 3));
    HIP_TRY(dvoffs.alloc(lay.voffs.size()));
    int rc = upload(dvoffs.p, lay.voffs.data(), lay.voffs.size() * 8);
    if (rc) return rc;
    lap("small uploads + stage alloc");
    rc = upload_staged(h, xyz_stage.p, model_xyz, (size_t)MN * 24);
    if (rc) return rc;
    lap("staged upload xyz");
    int uv_mode = 2;
    const double* uv_in = nullptr;
    if (sensor_uv.present() && h->dtype == CALIB_DTYPE_F64) {   // already in the device layout
        rc = upload_staged(h, h->uv.p, sensor_uv, (size_t)MN * 16);
        if (rc) return rc;
        uv_mode = 0;
    } else if (sensor_uv.present()) {
        HIP_TRY(uv_stage.alloc((size_t)MN * 2));
        rc = upload_staged(h, uv_stage.p, sensor_uv, (size_t)MN * 16);
        if (rc) return rc;
        uv_in = uv_stage.p;
        uv_mode = 1;
    }
    lap("staged upload uv");
    const unsigned blocks = (unsigned)((MN + 255) / 256);
    rc = dispatch(h, [&](auto form) -> int {
        using T = typename decltype(form)::T;
        using T2 = typename decltype(form)::T2;
        hipLaunchKernelGGL((pack_points_kernel<T>), dim3(blocks), dim3(256), 0, h->stream, xyz_stage.p, uv_in, uv_mode,
                           dvoffs.p, h->nv, MN, h->XY_as<T2>(), h->Z_as<T>(), h->uv_as<T2>(), h->pt_view.p);
        LAUNCHED(h, "pack_points_kernel");
        return CALIB_OK;
    });
    if (rc) return rc;
    SYNC_H(h);                   // the staging buffers go out of scope
    lap("pack kernel");
    return CALIB_OK;
}

int set_problem_impl(calib_handle_t h, int64_t num_views, const int64_t* view_offsets, const HostRows& sensor_uv,
                     const HostRows& model_xyz) {
    CHECK_H(h);
    if (num_views < 0 || !view_offsets) return fail(CALIB_E_INVALID, "bad view_offsets");
    if (view_offsets[0] != 0) return fail(CALIB_E_INVALID, "view_offsets[0] must be 0");
    for (int64_t i = 0; i < num_views; ++i)
        if (view_offsets[i + 1] < view_offsets[i])
            return fail(CALIB_E_INVALID, "view_offsets must be non-decreasing");
    const int64_t MN = view_offsets[num_views];
    if (MN > 0 && !model_xyz.present()) return fail(CALIB_E_INVALID, "model_xyz is null");
    if (num_views > 0x7fffffffLL / 8 || MN > (int64_t)1 << 40)
        return fail(CALIB_E_INVALID, "problem too large for one shard");
    SYNC_H(h);
    h->has_problem = false;
    h->lm_active = false;
    h->cov_pending = false;
    h->ext_offsets.assign(view_offsets, view_offsets + num_views + 1);
    h->ext_offsets_on_device = false;
    h->M = num_views;
    h->MN = MN;

    Laps lap{h->knobs.timing};
    ShardLayout lay = makeShardLayout(num_views, view_offsets, h->knobs.chunk_points);
    h->nv = lay.nv;
    h->n_items = lay.n_items;
    h->n_tiles = lay.n_tiles;
    h->max_views_per_tile = lay.max_views_per_tile;
    h->uniform_n = lay.uniform_n;
    h->chunks = std::move(lay.chunks);
    h->max_chunk_points = lay.max_chunk_points;
    lap("host view/item lists");

    const size_t ts = tsize(h);
    HIP_TRY(h->uv.alloc((size_t)MN * 2 * ts));
    HIP_TRY(h->XY.alloc((size_t)MN * 2 * ts));
    HIP_TRY(h->Z.alloc((size_t)MN * ts));
    HIP_TRY(h->pt_view.alloc((size_t)MN));
    HIP_TRY(h->view_ext.alloc((size_t)h->nv));
    HIP_TRY(h->item_n.alloc((size_t)h->n_items));
    HIP_TRY(h->item_view.alloc((size_t)h->n_items));
    HIP_TRY(h->item_pt0.alloc((size_t)h->n_items));
    HIP_TRY(h->view_item0.alloc((size_t)h->nv + 1));
    HIP_TRY(h->VC.alloc((size_t)std::max(h->nv, 1) * kViewStride * ts));
    HIP_TRY(h->r.alloc((size_t)MN * 2 * ts));
    HIP_TRY(h->sse_part.alloc((size_t)std::max<int64_t>(h->n_tiles, 1)));
    HIP_TRY(h->st_eval.alloc(1));
    HIP_TRY(hipMemsetAsync(h->st_eval.p, 0, sizeof(LMState), h->stream));
    HIP_TRY(h->Peval.alloc((size_t)numParams(h)));
    lap("device allocations");

    h->plan = plan_of(h);
    const struct { void* dst; const void* src; size_t bytes; } tables[] = {
        {h->view_ext.p, lay.view_ext.data(), lay.view_ext.size() * 4},
        {h->item_n.p, lay.item_n.data(), lay.item_n.size() * 4},
        {h->item_view.p, lay.item_view.data(), lay.item_view.size() * 4},
        {h->item_pt0.p, lay.item_pt0.data(), lay.item_pt0.size() * 8},
        {h->view_item0.p, lay.view_item0.data(), lay.view_item0.size() * 4},
    };
    for (const auto& t : tables) {
        const int rc = upload(t.dst, t.src, t.bytes);
        if (rc) return rc;
    }
    if (MN > 0) {
        const int rc = pack_points(h, lay, sensor_uv, model_xyz, lap);
        if (rc) return rc;
    }
    h->has_problem = true;
    return CALIB_OK;
}

// ---- peer exchange, LM run ---------------------------------------------------------------------
// Slot memory exported by handles of THIS process (one process driving several handles / GPUs): HIP IPC
// cannot open a handle in the process that made it, so calib_peer_connect looks here first.
struct LocalSlots { hipIpcMemHandle_t ipc; void* mem; int device; };
std::vector<LocalSlots> g_local_slots;
std::mutex g_local_slots_mutex;

void peer_release(calib_handle_s* h) {
    for (void* m : h->peer_open)
        if (m) (void)hipIpcCloseMemHandle(m);
    h->peer_open.clear();
    if (h->peer_mem) {
        std::lock_guard<std::mutex> lock(g_local_slots_mutex);
        for (size_t i = 0; i < g_local_slots.size(); ++i)
            if (g_local_slots[i].mem == h->peer_mem) { g_local_slots.erase(g_local_slots.begin() + (long)i); break; }
    }
    if (h->peer_mem) (void)hipFree(h->peer_mem);
    h->peer_mem = nullptr;
    h->peer_slots.release();
    h->peer_slot_host.clear();
    h->peer_flags.release();
    h->peer_connected = false;
    h->peer_world = 0;
}

// after a synchronisation: did a peer exchange of this handle give up waiting for a rank?
int peer_fault_check(calib_handle_s* h) {
    if (!h->peer_connected) return CALIB_OK;
    int fault = 0;
    HIP_TRY(hipMemcpy(&fault, h->peer_flags.p, sizeof(int), hipMemcpyDeviceToHost));
    if (fault)
        return fail(CALIB_E_HIP, "peer exchange: a rank's contribution did not arrive before the deadline "
                                 "(the ranks no longer run in lockstep, or a peer died)");
    return CALIB_OK;
}

// the end of a run: wait for it, read the LM state, then the peer-fault check and the singular check
int lm_finish(calib_handle_s* h, LMState* s) {
    SYNC_H(h);
    HIP_TRY(hipMemcpy(s, st_cur(h), sizeof(*s), hipMemcpyDeviceToHost));
    h->lm_active = false;
    const int prc = peer_fault_check(h);
    if (prc) return prc;
    if (s->error == CALIB_E_SINGULAR)
        return fail(CALIB_E_SINGULAR, "Singular matrix: damped normal equations are not invertible");
    return CALIB_OK;
}

int lm_run(calib_handle_t h, int rounds, int check_every, bool sharded) {
    CHECK_H(h);
    if (!h->lm_active) return fail(CALIB_E_STATE, "calib_lm_begin has not been called");
    const bool peers = sharded && h->peer_connected;      // the reduce kernel sums over the ranks itself
    for (int i = 0; i < rounds; ++i) {
        h->exchange_round = peers;
        int rc = calib_lm_local(h);
        h->exchange_round = false;
        if (rc) return rc;
        if (sharded && !peers) {
            rc = calib_lm_allreduce(h);
            if (rc) return rc;
        }
        rc = calib_lm_update(h);
        if (rc) return rc;
        if (peers && h->host_done && *static_cast<volatile int*>(h->host_done) == 2)
            return fail(CALIB_E_HIP, "peer exchange: a rank's contribution did not arrive before the deadline "
                                     "(the ranks no longer run in lockstep, or a peer died); no further rounds are enqueued");
        if (check_every > 0 && !sharded && h->host_done) {
            // single shard: the device says so in host-visible memory when the loop is over -- no synchronisation, the
            // host simply stops enqueueing (rounds already in the queue exit at once)
            if (*static_cast<volatile int*>(h->host_done)) break;
        } else if (check_every > 0 && (i + 1) % check_every == 0 && i + 1 < rounds) {
            // sharded: every rank must enqueue the same rounds, so all of them look at the (replicated) flag at the
            // same round numbers
            int done = 0;
            rc = calib_lm_done(h, &done);
            if (rc) return rc;
            if (done) break;
        }
    }
    return CALIB_OK;
}

// ---- entry points without a handle: the closed-form stages -------------------------------------
int check_views(int64_t num_views, const int64_t* view_offsets, const double* sensor_uv, const double* model_xyz) {
    if (num_views < 0 || !view_offsets) return fail(CALIB_E_INVALID, "null argument");
    if (num_views == 0) return CALIB_OK;
    const int64_t MN = view_offsets[num_views];
    if (view_offsets[0] != 0 || MN < 0 || (MN > 0 && (!sensor_uv || !model_xyz)))
        return fail(CALIB_E_INVALID, "bad view_offsets / point arrays");
    for (int64_t i = 0; i < num_views; ++i)
        if (view_offsets[i + 1] < view_offsets[i]) return fail(CALIB_E_INVALID, "view_offsets must be non-decreasing");
    return CALIB_OK;
}

int use_device(int device_id) {
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (device_id < 0 || device_id >= ndev) return fail(CALIB_E_HIP, "no such HIP device (no CPU fallback)");
    HIP_TRY(hipSetDevice(device_id));
    return CALIB_OK;
}

// DLT and / or LM polish of every view's homography
int homography_pipeline(int64_t num_views, const int64_t* view_offsets, const double* sensor_uv,
                        const double* model_xyz, double* H, bool dlt, int refine_iters, int device_id) {
    if (!H) return fail(CALIB_E_INVALID, "null argument");
    int rc = check_views(num_views, view_offsets, sensor_uv, model_xyz);
    if (rc || num_views == 0) return rc;
    rc = use_device(device_id);
    if (rc) return rc;
    const int64_t MN = view_offsets[num_views];
    std::vector<double> xy((size_t)MN * 2);
    for (int64_t p = 0; p < MN; ++p) { xy[2 * p] = model_xyz[3 * p]; xy[2 * p + 1] = model_xyz[3 * p + 1]; }
    DevBuf<int64_t> doffs;
    DevBuf<double2> duv, dxy;
    DevBuf<double> dH;
    HIP_TRY(doffs.alloc((size_t)num_views + 1));
    HIP_TRY(duv.alloc((size_t)std::max<int64_t>(MN, 1)));
    HIP_TRY(dxy.alloc((size_t)std::max<int64_t>(MN, 1)));
    HIP_TRY(dH.alloc((size_t)num_views * 9));
    HIP_TRY(hipMemcpy(doffs.p, view_offsets, ((size_t)num_views + 1) * 8, hipMemcpyHostToDevice));
    if (MN) HIP_TRY(hipMemcpy(duv.p, sensor_uv, (size_t)MN * 16, hipMemcpyHostToDevice));
    if (MN) HIP_TRY(hipMemcpy(dxy.p, xy.data(), (size_t)MN * 16, hipMemcpyHostToDevice));
    if (!dlt) HIP_TRY(hipMemcpy(dH.p, H, (size_t)num_views * 72, hipMemcpyHostToDevice));
    const unsigned blocks = (unsigned)((num_views + 15) / 16);
    if (dlt) {
        hipLaunchKernelGGL(dlt_kernel, dim3(blocks), dim3(256), 0, 0, doffs.p, (const double2*)duv.p, (const double2*)dxy.p,
                           num_views, dH.p);
        LAUNCHED(kNoHandle, "dlt_kernel");
    }
    if (refine_iters > 0) {
        hipLaunchKernelGGL(homography_lm_kernel, dim3(blocks), dim3(256), 0, 0, doffs.p, (const double2*)duv.p,
                           (const double2*)dxy.p, num_views, refine_iters, dH.p);
        LAUNCHED(kNoHandle, "homography_lm_kernel");
    }
    HIP_TRY(hipMemcpy(H, dH.p, (size_t)num_views * 72, hipMemcpyDeviceToHost));
    return CALIB_OK;
}

// ---- uncertainty (calib_cov_finish) ------------------------------------------------------------
// sigma2 (S_free)^-1 of the reduced system S = Bsum - Ssub, zero-padded to L x L for the fixed parameters: Cholesky of
// the free sub-matrix (lower triangle), its inverse by substitution, mirrored so that the result is exactly symmetric.
// Pure host arithmetic on the all-reduced buffer: every rank of a sharded run gets the same bits.
bool shared_covariance(const double* red, int L, uint32_t fixed_mask, double sigma2, double* Css /* L*L */) {
    int idx[kMaxL], n = 0;
    for (int i = 0; i < L; ++i) if (!((fixed_mask >> i) & 1)) idx[n++] = i;
    double S[kMaxL][kMaxL], X[kMaxL][kMaxL];
    for (int a = 0; a < n; ++a)
        for (int b = 0; b <= a; ++b) S[a][b] = red[idx[a] * L + idx[b]] - red[L * L + idx[a] * L + idx[b]];
    for (int j = 0; j < n; ++j) {                        // S = Lc Lc^T, in place
        double d = S[j][j];
        for (int q = 0; q < j; ++q) d -= S[j][q] * S[j][q];
        if (!(d > 0.0)) return false;
        S[j][j] = std::sqrt(d);
        for (int i = j + 1; i < n; ++i) {
            double t = S[i][j];
            for (int q = 0; q < j; ++q) t -= S[i][q] * S[j][q];
            S[i][j] = t / S[j][j];
        }
    }
    for (int c = 0; c < n; ++c) {                        // column c of the inverse
        double z[kMaxL];
        for (int i = 0; i < n; ++i) {
            double t = i == c ? 1.0 : 0.0;
            for (int q = 0; q < i; ++q) t -= S[i][q] * z[q];
            z[i] = t / S[i][i];
        }
        for (int i = n - 1; i >= 0; --i) {
            double t = z[i];
            for (int q = i + 1; q < n; ++q) t -= S[q][i] * X[q][c];
            X[i][c] = t / S[i][i];
        }
    }
    std::fill(Css, Css + L * L, 0.0);
    for (int a = 0; a < n; ++a)
        for (int b = 0; b <= a; ++b) {
            const double v = sigma2 * X[a][b];
            Css[idx[a] * L + idx[b]] = v;
            Css[idx[b] * L + idx[a]] = v;
        }
    return true;
}
}  // namespace

// ============================================================================ C-ABI
extern "C" {

int calib_version(void) { return 500; }   // 5.0: calib_rig_robust_*, calib_refine_rig_robust, calib_rig_residuals

const char* calib_last_error(void) { return g_err.c_str(); }

int calib_device_count(int* out_count) {
    if (!out_count) return fail(CALIB_E_INVALID, "out_count is null");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        *out_count = 0;
        return fail(CALIB_E_HIP, std::string("hipGetDeviceCount: ") + hipGetErrorString(e));
    }
    *out_count = n;
    return CALIB_OK;
}


int calib_create(int model, int dtype, int device_id, calib_handle_t* out_handle) {
    if (!out_handle) return fail(CALIB_E_INVALID, "out_handle is null");
    *out_handle = nullptr;
    if (!known_model(model)) return fail(CALIB_E_INVALID, "unknown distortion model");
    if (dtype != CALIB_DTYPE_F64 && dtype != CALIB_DTYPE_F32)
        return fail(CALIB_E_INVALID, "unknown dtype");
    int n = 0;
    HIP_TRY(hipGetDeviceCount(&n));
    if (device_id < 0 || device_id >= n)
        return fail(CALIB_E_HIP, "no such HIP device (this library has no CPU fallback)");
    HIP_TRY(hipSetDevice(device_id));
    // the half-built handle is owned here: every early return below destroys what it holds
    std::unique_ptr<calib_handle_s, int (*)(calib_handle_t)> h(new (std::nothrow) calib_handle_s(), calib_destroy);
    if (!h) return fail(CALIB_E_INVALID, "out of host memory");
    h->model = model;
    h->dtype = dtype;
    h->device = device_id;
    h->L = 5 + num_distortion(model);
    h->C = h->L + 6;
    HIP_TRY(hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking));
    h->stream = h->own_stream;
    {
        uint32_t tab[kEmitTabSize];
        buildEmitTable(h->C, tab);
        HIP_TRY(h->emit_tab.alloc(kEmitTabSize));
        HIP_TRY(hipMemcpy(h->emit_tab.p, tab, sizeof(tab), hipMemcpyHostToDevice));
    }
    {
        int32_t ops[64 * kStreamOps];
        if (!buildStreamOps(h->C, ops)) return fail(CALIB_E_HIP, "stream record table: inconsistent");
        HIP_TRY(h->stream_ops.alloc(64 * kStreamOps));
        HIP_TRY(hipMemcpy(h->stream_ops.p, ops, sizeof(ops), hipMemcpyHostToDevice));
    }
    h->knobs = readKnobs();
    h->lm_mode = h->knobs.lm_mode;
    {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device_id) == hipSuccess && cus > 0)
            h->num_cus = cus;
    }
    *out_handle = h.release();
    return CALIB_OK;
}

// What the members' destructors cannot do, in this order: the stream is drained before anything is freed; the
// device buffers (DevBuf) go with `delete`.
int calib_destroy(calib_handle_t h) {
    if (!h) return CALIB_OK;
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
    if (h->comm && g_rccl.commDestroy) { (void)g_rccl.commDestroy(h->comm); h->comm = nullptr; }
    peer_release(h);
    for (auto& e : h->ev) (void)hipEventDestroy(e);
    if (h->stage_ready)
        for (int t = 0; t < 4; ++t) {
            for (int b = 0; b < 2; ++b) {
                if (h->stage_ev[t][b]) (void)hipEventDestroy(h->stage_ev[t][b]);
            }
        }
    if (h->stage_pinned) (void)hipHostFree(h->stage_pinned);
    if (h->host_done) (void)hipHostFree(h->host_done);
    if (h->own_stream) (void)hipStreamDestroy(h->own_stream);
    delete h;
    return CALIB_OK;
}

int calib_set_stream(calib_handle_t h, void* hip_stream, int use_own) {
    CHECK_H(h);
    SYNC_H(h);
    h->stream = use_own ? h->own_stream : reinterpret_cast<hipStream_t>(hip_stream);
    return CALIB_OK;
}

int calib_synchronize(calib_handle_t h) {
    CHECK_H(h);
    SYNC_H(h);
    return CALIB_OK;
}

int calib_set_lm_mode(calib_handle_t h, int mode) {
    CHECK_H(h);
    if (mode != CALIB_LM_FUSED && mode != CALIB_LM_TWO_KERNEL) return fail(CALIB_E_INVALID, "unknown LM mode");
    if (h->lm_active) return fail(CALIB_E_STATE, "cannot change the LM mode inside a run");
    h->lm_mode = mode;
    if (h->has_problem) h->plan = plan_of(h);      // the stream form exists in fused mode only
    return CALIB_OK;
}

int calib_fused_form(calib_handle_t h, int* out_share, int* out_waves) {
    if (!h || !out_share || !out_waves) return fail(CALIB_E_INVALID, "null argument");
    *out_share = h->plan.stream_share;
    *out_waves = h->plan.stream_waves;
    return CALIB_OK;
}

int calib_num_shared(calib_handle_t h, int* out_L) {
    if (!h || !out_L) return fail(CALIB_E_INVALID, "null argument");
    *out_L = h->L;
    return CALIB_OK;
}

int calib_set_fixed_shared(calib_handle_t h, uint32_t mask) {
    CHECK_H(h);
    if (mask >> h->L) return fail(CALIB_E_INVALID, "fixed mask has a bit at or above the number of shared parameters");
    h->fixed_mask = mask;
    return CALIB_OK;
}

int calib_get_fixed_shared(calib_handle_t h, uint32_t* out_mask) {
    CHECK_H(h);
    if (!out_mask) return fail(CALIB_E_INVALID, "out_mask is null");
    *out_mask = h->fixed_mask;
    return CALIB_OK;
}

int calib_num_params(calib_handle_t h, int64_t* out_K) {
    if (!h || !out_K) return fail(CALIB_E_INVALID, "null argument");
    *out_K = numParams(h);
    return CALIB_OK;
}

int calib_set_problem(calib_handle_t h, int64_t num_views, const int64_t* view_offsets,
                      const double* sensor_uv, const double* model_xyz) {
    HostRows s, m;
    s.flat = sensor_uv; s.width = 2;
    m.flat = model_xyz; m.width = 3;
    return set_problem_impl(h, num_views, view_offsets, s, m);
}

int calib_set_problem_views(calib_handle_t h, int64_t num_views, const int64_t* view_offsets,
                            const double* const* sensor_uv_views, const double* const* model_xyz_views) {
    if (num_views < 0 || !view_offsets) return fail(CALIB_E_INVALID, "bad view_offsets");
    if (num_views > 0 && !model_xyz_views) return fail(CALIB_E_INVALID, "model_xyz_views is null");
    for (int64_t i = 0; i < num_views; ++i)
        if (view_offsets[i + 1] > view_offsets[i] && (!model_xyz_views[i] || (sensor_uv_views && !sensor_uv_views[i])))
            return fail(CALIB_E_INVALID, "a view with points has a null array");
    HostRows s, m;
    s.views = sensor_uv_views; s.offs = view_offsets; s.nviews = num_views; s.width = 2;
    m.views = model_xyz_views; m.offs = view_offsets; m.nviews = num_views; m.width = 3;
    return set_problem_impl(h, num_views, view_offsets, s, m);
}

int calib_eval(calib_handle_t h, const double* P, double* out_y, double* out_r, double* out_Jc,
               double* out_sse) {
    CHECK_H(h);
    int rc = need_problem(h);
    if (rc) return rc;
    if (!P) return fail(CALIB_E_INVALID, "P is null");
    const size_t ts = tsize(h);
    const int64_t MN = h->MN;
    const size_t MN4 = (size_t)((MN + 3) / 4 * 4);     // J is stored in groups of 4 points
    if (out_Jc) HIP_TRY(h->J.alloc(MN4 * h->C * 2 * ts));
    if (out_y) HIP_TRY(h->y.alloc((size_t)MN * 2 * ts));
    HIP_TRY(h->red_own.alloc((size_t)reduceSize(h->L)));
    HIP_TRY(hipMemcpyAsync(h->Peval.p, P, (size_t)numParams(h) * 8, hipMemcpyHostToDevice, h->stream));
    rc = launch_view_setup(h, h->Peval.p, nullptr, h->st_eval.p, 0);
    if (rc) return rc;
    rc = launch_jacobian(h, h->Peval.p, nullptr, h->st_eval.p, 0, out_Jc != nullptr, out_r != nullptr,
                         out_y != nullptr, true, 0, MN);
    if (rc) return rc;
    hipLaunchKernelGGL(sse_reduce_kernel, dim3(1), dim3(256), 0, h->stream, h->sse_part.p, h->n_tiles,
                       h->red_own.p);
    LAUNCHED(h, "sse_reduce_kernel");
    SYNC_H(h);
    if (out_sse) HIP_TRY(hipMemcpy(out_sse, h->red_own.p, 8, hipMemcpyDeviceToHost));

    auto fetch2 = [&](const void* dev, double* out) -> int {   // (MN,2) of T -> double
        if (h->dtype == CALIB_DTYPE_F64) {
            HIP_TRY(hipMemcpy(out, dev, (size_t)MN * 16, hipMemcpyDeviceToHost));
        } else {
            std::vector<float> tmp((size_t)MN * 2);
            HIP_TRY(hipMemcpy(tmp.data(), dev, tmp.size() * 4, hipMemcpyDeviceToHost));
            for (size_t i = 0; i < tmp.size(); ++i) out[i] = tmp[i];
        }
        return CALIB_OK;
    };
    if (out_y && MN) { rc = fetch2(h->y.p, out_y); if (rc) return rc; }
    if (out_r && MN) { rc = fetch2(h->r.p, out_r); if (rc) return rc; }
    if (out_Jc && MN) {
        // device layout jIndex(p, c)(du,dv) -> caller layout (MN,2,C)
        const int C = h->C;
        const size_t cnt = MN4 * C * 2;
        std::vector<double> tmp(cnt);
        if (h->dtype == CALIB_DTYPE_F64) {
            HIP_TRY(hipMemcpy(tmp.data(), h->J.p, cnt * 8, hipMemcpyDeviceToHost));
        } else {
            std::vector<float> tf(cnt);
            HIP_TRY(hipMemcpy(tf.data(), h->J.p, cnt * 4, hipMemcpyDeviceToHost));
            for (size_t i = 0; i < cnt; ++i) tmp[i] = tf[i];
        }
        for (int64_t p = 0; p < MN; ++p)
            for (int c = 0; c < C; ++c) {
                out_Jc[(p * 2 + 0) * C + c] = tmp[(size_t)jIndex(p, c, C) * 2 + 0];
                out_Jc[(p * 2 + 1) * C + c] = tmp[(size_t)jIndex(p, c, C) * 2 + 1];
            }
    }
    return CALIB_OK;
}

int calib_lm_reduce_size(calib_handle_t h, int64_t* out_num_doubles) {
    if (!h || !out_num_doubles) return fail(CALIB_E_INVALID, "null argument");
    *out_num_doubles = reduceSize(h->L);
    return CALIB_OK;
}

int calib_lm_bind_reduce_buffer(calib_handle_t h, void* reduce_dev) {
    CHECK_H(h);
    SYNC_H(h);
    HIP_TRY(h->red_own.alloc((size_t)reduceSize(h->L)));
    h->red = reduce_dev ? reinterpret_cast<double*>(reduce_dev) : h->red_own.p;
    return CALIB_OK;
}

int calib_lm_begin(calib_handle_t h, const double* P0, int max_iters, double lam_init, double lam_min,
                   double lam_max, double err_min) {
    CHECK_H(h);
    int rc = need_problem(h);
    if (rc) return rc;
    if (!P0) return fail(CALIB_E_INVALID, "P0 is null");
    h->cov_pending = false;
    if (max_iters <= 0)
        return fail(CALIB_E_INVALID, "max_iters must be >= 1 (the reference raises UnboundLocalError "
                                     "for maxIters=0, src/calibrate.py:171)");
    // A shard WITHOUT views is legal (ranks of a sharded run may own none): it contributes zeros to the
    // reduce buffer and still takes every decision. Alone, it ends as the reference does on an empty system:
    // CALIB_E_SINGULAR from the L x L solve.
    if (h->nv != h->M)
        return fail(CALIB_E_SINGULAR, "a view without points makes J^T J + lambda diag(J^T J) singular");
    const size_t ts = tsize(h);
    const int64_t K = numParams(h);
    if (h->lm_mode == CALIB_LM_TWO_KERNEL)
        HIP_TRY(h->J.alloc((size_t)((h->max_chunk_points + 3) / 4 * 4) * h->C * 2 * ts));
    for (int b = 0; b < 2; ++b) {
        // fused_stream_kernel writes only the record entries the per-view kernels read: start from zeros
        const bool fresh = !h->G[b].p || h->G[b].n < (size_t)num_records(h) * kGStride;
        HIP_TRY(h->G[b].alloc((size_t)num_records(h) * kGStride));
        if (fresh) HIP_TRY(hipMemsetAsync(h->G[b].p, 0, h->G[b].n * 8, h->stream));
    }
    HIP_TRY(h->bpart.alloc(((size_t)std::max(h->n_items, 1) + h->chunks.size()) * kPartStride));   // <= 1 per item (+1 per chunk)
    HIP_TRY(h->part.alloc((size_t)2 * h->plan.schur_blocks * variantSize(h->L)));
    HIP_TRY(h->red_own.alloc((size_t)reduceSize(h->L)));
    if (!h->red) h->red = h->red_own.p;
    HIP_TRY(h->P[0].alloc((size_t)K));
    HIP_TRY(h->P[1].alloc((size_t)K));
    HIP_TRY(h->st.alloc(2));
    HIP_TRY(h->trace.alloc((size_t)max_iters * (CALIB_TRACE_HEADER + h->L)));
    HIP_TRY(hipMemsetAsync(h->trace.p, 0, (size_t)max_iters * (CALIB_TRACE_HEADER + h->L) * 8, h->stream));
    HIP_TRY(hipMemcpyAsync(h->P[0].p, P0, (size_t)K * 8, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(h->P[1].p, P0, (size_t)K * 8, hipMemcpyHostToDevice, h->stream));
    LMState s;
    std::memset(&s, 0, sizeof(s));
    s.lam = lam_init; s.lam_min = lam_min; s.lam_max = lam_max; s.err_min = err_min;
    if (!h->host_done) {
        void* p = nullptr;
        if (hipHostMalloc(&p, sizeof(int), hipHostMallocMapped) == hipSuccess) h->host_done = static_cast<int*>(p);
        else (void)hipGetLastError();        // without the word the host falls back to synchronising checks
        void* dp = nullptr;
        if (h->host_done && hipHostGetDevicePointer(&dp, h->host_done, 0) == hipSuccess) h->host_done_dev = static_cast<int*>(dp);
        else (void)hipGetLastError();
    }
    if (h->host_done) {
        // a run that was begun and never ended (an exception between lmBegin and lmEnd) may still have update kernels
        // in flight that would set the word AFTER this reset: drain them first
        if (h->lm_active) SYNC_H(h);
        *h->host_done = 0;
        s.notify = h->host_done_dev;
    }
    s.cur = 1;            // round 0 evaluates the "candidate" buffer 0 == P0
    s.fixed_mask = (int)h->fixed_mask;     // the update kernel carries it from round to round
    s.max_iters = max_iters;
    HIP_TRY(hipMemsetAsync(h->st.p, 0, 2 * sizeof(LMState), h->stream));
    HIP_TRY(hipMemcpyAsync(h->st.p, &s, sizeof(s), hipMemcpyHostToDevice, h->stream));
    SYNC_H(h);     // s and P0 are host stack / caller memory
    h->lm_active = true;
    h->lm_max_iters = max_iters;
    h->rounds_enqueued = 0;
    return CALIB_OK;
}

int calib_lm_local(calib_handle_t h) {
    CHECK_H(h);
    if (!h->lm_active) return fail(CALIB_E_STATE, "calib_lm_begin has not been called");
    LMState* st = st_cur(h);
    int rc = CALIB_OK;
    if (h->rounds_enqueued == 0) {      // later rounds: the update kernel already wrote the candidate's constants
        rc = launch_view_setup(h, h->P[0].p, h->P[1].p, st, 1);
        if (rc) return rc;
    }
    if (h->lm_mode == CALIB_LM_FUSED) {
        rc = launch_fused(h, st, 1);
        if (rc) return rc;
        return launch_schur_reduce(h, st, h->red);
    }
    h->n_bpart = 0;
    for (const auto& c : h->chunks) {
        rc = launch_jacobian(h, h->P[0].p, h->P[1].p, st, 1, true, true, false, false, c.p0, c.p1);
        if (rc) return rc;
        rc = launch_gram(h, st, 1, c.item0, c.item1, c.p0);
        if (rc) return rc;
    }
    return launch_schur_reduce(h, st, h->red);
}

int calib_lm_update(calib_handle_t h) {
    CHECK_H(h);
    if (!h->lm_active) return fail(CALIB_E_STATE, "calib_lm_begin has not been called");
    const int rc = launch_update_backsub(h);
    h->rounds_enqueued += 1;
    return rc;
}

int calib_lm_done(calib_handle_t h, int* out_done) {
    CHECK_H(h);
    if (!h->lm_active || !out_done) return fail(CALIB_E_STATE, "no LM run active");
    LMState s;
    HIP_TRY(hipMemcpyAsync(&s, st_cur(h), sizeof(s), hipMemcpyDeviceToHost, h->stream));
    SYNC_H(h);
    *out_done = s.done;
    return peer_fault_check(h);
}

int calib_lm_peek_trace(calib_handle_t h, int iter, double* out_row, int* out_iters) {
    CHECK_H(h);
    if (!h->lm_active || !out_row || !out_iters) return fail(CALIB_E_STATE, "no LM run active");
    if (iter < 0 || iter >= h->lm_max_iters) return fail(CALIB_E_INVALID, "trace row out of range");
    LMState s;
    const size_t w = (size_t)(CALIB_TRACE_HEADER + h->L);
    HIP_TRY(hipMemcpyAsync(&s, st_cur(h), sizeof(s), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(out_row, h->trace.p + (size_t)iter * w, w * 8, hipMemcpyDeviceToHost, h->stream));
    SYNC_H(h);
    *out_iters = s.iters;
    return CALIB_OK;
}

int calib_lm_run(calib_handle_t h, int rounds, int check_every) { return lm_run(h, rounds, check_every, false); }

int calib_lm_run_sharded(calib_handle_t h, int rounds, int check_every) {
    if (h && !h->comm && !h->peer_connected)
        return fail(CALIB_E_STATE, "neither calib_peer_connect nor calib_rccl_init has been called");
    return lm_run(h, rounds, check_every, true);
}

int calib_rccl_load(const char* librccl_path) {
    std::lock_guard<std::mutex> lock(g_rccl_mutex);
    if (g_rccl.lib) return CALIB_OK;
    if (!librccl_path) return fail(CALIB_E_INVALID, "librccl path is null");
    void* lib = dlopen(librccl_path, RTLD_NOW | RTLD_GLOBAL);
    if (!lib) return fail(CALIB_E_HIP, std::string("dlopen librccl: ") + dlerror());
    RcclApi a;
    a.lib = lib;
    a.getUniqueId = reinterpret_cast<decltype(a.getUniqueId)>(dlsym(lib, "ncclGetUniqueId"));
    a.commInitRank = reinterpret_cast<decltype(a.commInitRank)>(dlsym(lib, "ncclCommInitRank"));
    a.allReduce = reinterpret_cast<decltype(a.allReduce)>(dlsym(lib, "ncclAllReduce"));
    a.commDestroy = reinterpret_cast<decltype(a.commDestroy)>(dlsym(lib, "ncclCommDestroy"));
    a.commAbort = reinterpret_cast<decltype(a.commAbort)>(dlsym(lib, "ncclCommAbort"));
    a.getErrorString = reinterpret_cast<decltype(a.getErrorString)>(dlsym(lib, "ncclGetErrorString"));
    if (!a.getUniqueId || !a.commInitRank || !a.allReduce || !a.commDestroy || !a.commAbort) {
        (void)dlclose(lib);
        return fail(CALIB_E_HIP, "librccl lacks ncclGetUniqueId / ncclCommInitRank / ncclAllReduce / ncclCommDestroy / ncclCommAbort");
    }
    g_rccl = a;
    return CALIB_OK;
}

int calib_rccl_unique_id(void* out_id128) {
    if (!g_rccl.lib) return fail(CALIB_E_STATE, "calib_rccl_load has not been called");
    if (!out_id128) return fail(CALIB_E_INVALID, "null argument");
    RcclId id;
    const int rc = g_rccl.getUniqueId(&id);
    if (rc) return rccl_fail("ncclGetUniqueId", rc);
    std::memcpy(out_id128, id.internal, sizeof(id.internal));
    return CALIB_OK;
}

int calib_rccl_init(calib_handle_t h, int nranks, int rank, const void* id128) {
    return calib_rccl_init_deadline(h, nranks, rank, id128, 120.0);
}

int calib_rccl_init_deadline(calib_handle_t h, int nranks, int rank, const void* id128, double timeout_s) {
    CHECK_H(h);
    if (!g_rccl.lib) return fail(CALIB_E_STATE, "calib_rccl_load has not been called");
    if (!id128 || nranks < 1 || rank < 0 || rank >= nranks) return fail(CALIB_E_INVALID, "bad communicator arguments");
    if (h->comm) return fail(CALIB_E_STATE, "this handle already has a communicator");
    // ncclCommInitRank blocks until every rank has joined; a peer that never calls it would hang this thread
    // for good. It runs on a helper thread; past the deadline the caller gets an error and the helper, should
    // it ever return, destroys the communicator it made.
    struct Job { RcclId id; int nranks, rank, device; void* comm = nullptr; int rc = 0; std::atomic<bool> abandoned{false}; };
    auto job = std::make_shared<Job>();
    std::memcpy(job->id.internal, id128, sizeof(job->id.internal));
    job->nranks = nranks; job->rank = rank; job->device = h->device;
    std::promise<void> donePromise;
    std::future<void> done = donePromise.get_future();
    std::thread([job, p = std::move(donePromise)]() mutable {
        (void)hipSetDevice(job->device);
        job->rc = g_rccl.commInitRank(&job->comm, job->nranks, job->id, job->rank);
        if (job->abandoned.load() && job->rc == 0 && job->comm) (void)g_rccl.commAbort(job->comm);
        p.set_value();
    }).detach();
    if (done.wait_for(std::chrono::duration<double>(timeout_s > 0 ? timeout_s : 120.0)) != std::future_status::ready) {
        job->abandoned.store(true);
        return fail(CALIB_E_HIP, "ncclCommInitRank did not return before the deadline (a peer rank is missing)");
    }
    if (job->rc) return rccl_fail("ncclCommInitRank", job->rc);
    h->comm = job->comm;
    h->comm_ranks = nranks;
    h->comm_rank = rank;
    return CALIB_OK;
}

int calib_rccl_shutdown(calib_handle_t h) {
    CHECK_H(h);
    if (!h->comm) return CALIB_OK;
    (void)hipStreamSynchronize(h->stream);
    const int rc = g_rccl.commDestroy(h->comm);
    h->comm = nullptr;
    h->comm_ranks = 0;
    if (rc) return rccl_fail("ncclCommDestroy", rc);
    return CALIB_OK;
}

int calib_rccl_selftest(calib_handle_t h, double timeout_s) {
    CHECK_H(h);
    if (!h->comm) return fail(CALIB_E_STATE, "calib_rccl_init has not been called");
    // rank r contributes (r + 1, 1, 2^r, 4): the sums must come back as (n (n + 1) / 2, n, 2^n - 1, 4 n).
    // The operand lives in the handle: a collective that timed out may still refer to it.
    const int n = h->comm_ranks, r = h->comm_rank;
    HIP_TRY(h->rccl_test.alloc(4));
    const double mine[4] = {r + 1.0, 1.0, std::ldexp(1.0, r), 4.0};
    const double want[4] = {0.5 * n * (n + 1.0), (double)n, std::ldexp(1.0, n) - 1.0, 4.0 * n};
    HIP_TRY(hipMemcpy(h->rccl_test.p, mine, sizeof(mine), hipMemcpyHostToDevice));
    auto giveUp = [&]() {                   // the communicator cannot be trusted: abort it, never destroy it
        (void)g_rccl.commAbort(h->comm);
        h->comm = nullptr;
        h->comm_ranks = 0;
    };
    int rc = g_rccl.allReduce(h->rccl_test.p, h->rccl_test.p, 4, kNcclDouble, kNcclSum, h->comm, h->stream);
    if (rc) { giveUp(); return rccl_fail("ncclAllReduce (self-test)", rc); }
    const auto deadline = std::chrono::steady_clock::now() + std::chrono::duration<double>(timeout_s > 0 ? timeout_s : 30.0);
    for (hipError_t e; (e = hipStreamQuery(h->stream)) != hipSuccess;) {
        if (e != hipErrorNotReady) { giveUp(); return fail(CALIB_E_HIP, hipGetErrorString(e)); }
        if (std::chrono::steady_clock::now() > deadline) {
            giveUp();
            return fail(CALIB_E_HIP, "in-library all-reduce self-test timed out");
        }
        std::this_thread::sleep_for(std::chrono::microseconds(200));
    }
    double got[4] = {0, 0, 0, 0};
    HIP_TRY(hipMemcpy(got, h->rccl_test.p, sizeof(got), hipMemcpyDeviceToHost));
    for (int i = 0; i < 4; ++i)
        if (got[i] != want[i]) {
            giveUp();
            return fail(CALIB_E_HIP, "in-library all-reduce self-test returned wrong sums");
        }
    return CALIB_OK;
}

int calib_lm_allreduce(calib_handle_t h) {
    CHECK_H(h);
    if (!h->lm_active && !h->cov_pending) return fail(CALIB_E_STATE, "calib_lm_begin has not been called");
    if (!h->comm) return fail(CALIB_E_STATE, "calib_rccl_init has not been called");
    const int rc = g_rccl.allReduce(h->red, h->red, (size_t)reduceSize(h->L), kNcclDouble, kNcclSum, h->comm, h->stream);
    if (rc) return rccl_fail("ncclAllReduce", rc);
    return CALIB_OK;
}

// ---- peer exchange over xGMI ----------------------------------------------------------------
int calib_peer_prepare(calib_handle_t h, int nranks, int rank, void* out_handle64) {
    CHECK_H(h);
    static_assert(sizeof(hipIpcMemHandle_t) == CALIB_PEER_HANDLE_BYTES, "hipIpcMemHandle_t is 64 bytes");
    if (!out_handle64 || nranks < 1 || nranks > kPeerMaxRanks || rank < 0 || rank >= nranks)
        return fail(CALIB_E_INVALID, "bad peer exchange arguments (1 <= nranks <= 64, 0 <= rank < nranks)");
    if (h->peer_mem) return fail(CALIB_E_STATE, "this handle already takes part in a peer exchange");
    if (h->lm_active) return fail(CALIB_E_STATE, "cannot set up a peer exchange inside an LM run");
    // Cells are written by other GPUs while this one polls them: the memory must not be held in this
    // device's L2 (uncached; fine-grained where the runtime has no uncached pool).
    const size_t bytes = (size_t)nranks * 2 * kPeerStride * 2 * sizeof(unsigned long long);
    void* mem = nullptr;
    if (hipExtMallocWithFlags(&mem, bytes, hipDeviceMallocUncached) != hipSuccess) {
        (void)hipGetLastError();
        const hipError_t e = hipExtMallocWithFlags(&mem, bytes, hipDeviceMallocFinegrained);
        if (e != hipSuccess) return fail(CALIB_E_HIP, std::string("peer slot memory: ") + hipGetErrorString(e));
    }
    h->peer_mem = mem;
    h->peer_world = nranks;
    h->peer_rank = rank;
    auto undo = [&](const char* what, hipError_t e) {
        peer_release(h);
        return fail(CALIB_E_HIP, std::string(what) + ": " + hipGetErrorString(e));
    };
    if (hipError_t e = hipMemset(mem, 0, bytes)) return undo("peer slot memory", e);          // epoch 0 is never sent
    if (hipError_t e = hipDeviceSynchronize()) return undo("peer slot memory", e);
    hipIpcMemHandle_t ipc;
    if (hipError_t e = hipIpcGetMemHandle(&ipc, mem)) return undo("hipIpcGetMemHandle", e);
    std::memcpy(out_handle64, &ipc, sizeof(ipc));
    {
        std::lock_guard<std::mutex> lock(g_local_slots_mutex);
        g_local_slots.push_back(LocalSlots{ipc, mem, h->device});
    }
    return CALIB_OK;
}

int calib_peer_connect(calib_handle_t h, const void* handles, double timeout_s) {
    CHECK_H(h);
    if (!handles) return fail(CALIB_E_INVALID, "null argument");
    if (!h->peer_mem) return fail(CALIB_E_STATE, "calib_peer_prepare has not been called");
    if (h->peer_connected) return fail(CALIB_E_STATE, "peers are already connected");
    const int n = h->peer_world;
    std::vector<unsigned long long*> slots((size_t)n, nullptr);
    h->peer_open.assign((size_t)n, nullptr);
    for (int r = 0; r < n; ++r) {
        if (r == h->peer_rank) { slots[(size_t)r] = static_cast<unsigned long long*>(h->peer_mem); continue; }
        hipIpcMemHandle_t ipc;
        std::memcpy(&ipc, static_cast<const char*>(handles) + (size_t)r * sizeof(ipc), sizeof(ipc));
        void* m = nullptr;
        hipError_t pe = hipSuccess;
        {
            std::lock_guard<std::mutex> lock(g_local_slots_mutex);
            for (const LocalSlots& ls : g_local_slots)
                if (std::memcmp(&ls.ipc, &ipc, sizeof(ipc)) == 0) {
                    if (ls.device != h->device) {
                        pe = hipDeviceEnablePeerAccess(ls.device, 0);
                        if (pe == hipErrorPeerAccessAlreadyEnabled) { (void)hipGetLastError(); pe = hipSuccess; }
                    }
                    m = ls.mem;
                }
        }
        if (pe != hipSuccess) {
            (void)hipGetLastError();
            for (void*& o : h->peer_open) { if (o) (void)hipIpcCloseMemHandle(o); o = nullptr; }
            return fail(CALIB_E_HIP, "hipDeviceEnablePeerAccess (device of rank " + std::to_string(r) + "): " + hipGetErrorString(pe));
        }
        if (m) { slots[(size_t)r] = static_cast<unsigned long long*>(m); continue; }
        const hipError_t e = hipIpcOpenMemHandle(&m, ipc, hipIpcMemLazyEnablePeerAccess);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            for (void*& o : h->peer_open) { if (o) (void)hipIpcCloseMemHandle(o); o = nullptr; }
            return fail(CALIB_E_HIP, "hipIpcOpenMemHandle (slot memory of rank " + std::to_string(r) + "): " + hipGetErrorString(e));
        }
        h->peer_open[(size_t)r] = m;
        slots[(size_t)r] = static_cast<unsigned long long*>(m);
    }
    h->peer_slot_host = slots;
    HIP_TRY(h->peer_slots.alloc((size_t)n));
    HIP_TRY(h->peer_flags.alloc(2));
    HIP_TRY(hipMemcpy(h->peer_slots.p, slots.data(), (size_t)n * sizeof(slots[0]), hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(h->peer_flags.p, 0, 2 * sizeof(int)));
    h->peer_timeout_s = timeout_s > 0 ? timeout_s : 60.0;
    h->peer_epoch = 0;
    h->peer_connected = true;
    return CALIB_OK;
}

int calib_peer_selftest(calib_handle_t h, int rounds, double timeout_s) {
    CHECK_H(h);
    if (!h->peer_connected) return fail(CALIB_E_STATE, "calib_peer_connect has not been called");
    if (rounds < 1) rounds = 1;
    const double keep = h->peer_timeout_s;
    h->peer_timeout_s = timeout_s > 0 ? timeout_s : 10.0;       // each spin of the test gives up after this long
    for (int r = 0; r < rounds; ++r) {
        hipLaunchKernelGGL(peer_selftest_kernel, dim3(kPeerStride), dim3(64), 0, h->stream, next_exchange(h), r,
                           h->peer_flags.p + 1);
        LAUNCHED(h, "peer_selftest_kernel");
    }
    h->peer_timeout_s = keep;
    SYNC_H(h);
    int flags[2] = {0, 0};
    HIP_TRY(hipMemcpy(flags, h->peer_flags.p, sizeof(flags), hipMemcpyDeviceToHost));
    if (flags[0] || flags[1]) {
        HIP_TRY(hipMemset(h->peer_flags.p, 0, sizeof(flags)));
        return fail(CALIB_E_HIP, flags[0] ? "peer exchange self-test: a rank's contribution did not arrive in time"
                                          : "peer exchange self-test: wrong sums (" + std::to_string(flags[1]) + " elements)");
    }
    return CALIB_OK;
}

int calib_peer_shutdown(calib_handle_t h) {
    CHECK_H(h);
    if (h->lm_active) return fail(CALIB_E_STATE, "cannot drop the peer exchange inside an LM run");
    (void)hipStreamSynchronize(h->stream);
    peer_release(h);
    return CALIB_OK;
}

int calib_lm_end(calib_handle_t h, double* P_out, double* out_sse, int* out_iters, double* out_trace) {
    CHECK_H(h);
    if (!h->lm_active) return fail(CALIB_E_STATE, "no LM run active");
    LMState s;
    const int rc = lm_finish(h, &s);
    if (rc) return rc;
    // after the bootstrap round cur points at the current parameters
    const int cur = s.round == 0 ? 0 : s.cur;
    if (P_out) HIP_TRY(hipMemcpy(P_out, h->P[cur].p, (size_t)numParams(h) * 8, hipMemcpyDeviceToHost));
    if (out_sse) *out_sse = s.last_err;
    if (out_iters) *out_iters = s.iters;
    if (out_trace && s.iters > 0)
        HIP_TRY(hipMemcpy(out_trace, h->trace.p, (size_t)s.iters * (CALIB_TRACE_HEADER + h->L) * 8,
                          hipMemcpyDeviceToHost));
    return CALIB_OK;
}

int calib_refine(calib_handle_t h, double* P_inout, int max_iters, double lam_init, double lam_min,
                 double lam_max, double err_min, double* out_sse, int* out_iters, double* out_trace) {
    int rc = calib_lm_begin(h, P_inout, max_iters, lam_init, lam_min, lam_max, err_min);
    if (rc) return rc;
    rc = calib_lm_run(h, max_iters + 1, 8);
    if (rc) return rc;
    return calib_lm_end(h, P_inout, out_sse, out_iters, out_trace);
}

int calib_lm_step_delta(calib_handle_t h, const double* P, double lambda, double* out_delta) {
    if (!out_delta) return fail(CALIB_E_INVALID, "out_delta is null");
    int rc = calib_lm_begin(h, P, 1, lambda, 0.0, INFINITY, -INFINITY);
    if (rc) return rc;
    rc = calib_lm_run(h, 1, 0);     // bootstrap round: evaluates P, solves, writes P + delta
    if (rc) return rc;
    LMState s;
    rc = lm_finish(h, &s);
    if (rc) return rc;
    const int64_t K = numParams(h);
    std::vector<double> cand((size_t)K);
    HIP_TRY(hipMemcpy(cand.data(), h->P[s.cur ^ 1].p, (size_t)K * 8, hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < K; ++i) out_delta[i] = cand[(size_t)i] - P[i];
    return CALIB_OK;
}

int calib_normal_eq(calib_handle_t h, const double* P, double* out_B, double* out_E, double* out_V,
                    double* out_g) {
    // bootstrap round with lambda = 0: variant A of the reduce buffer carries sum B and g_c,
    // the per-view Gram blocks carry E_i, V_i, g_i.
    int rc = calib_lm_begin(h, P, 1, 0.0, 0.0, INFINITY, -INFINITY);
    if (rc) return rc;
    rc = calib_lm_local(h);
    if (rc) return rc;
    SYNC_H(h);
    h->lm_active = false;
    const int L = h->L;
    std::vector<double> red((size_t)reduceSize(L));
    HIP_TRY(hipMemcpy(red.data(), h->red, red.size() * 8, hipMemcpyDeviceToHost));
    if (out_B) std::memcpy(out_B, red.data(), (size_t)L * L * 8);
    if (out_g) std::memcpy(out_g, red.data() + 2 * L * L, (size_t)L * 8);
    if (out_E || out_V || out_g) {
        std::vector<double> G((size_t)num_records(h) * kGStride);
        std::vector<int> vi0((size_t)h->nv + 1);
        const StreamMap sm = stream_map(h);
        HIP_TRY(hipMemcpy(G.data(), h->G[0].p, G.size() * 8, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(vi0.data(), h->view_item0.p, vi0.size() * 4, hipMemcpyDeviceToHost));
        for (int v = 0; v < h->nv; ++v) {       // nv == M here (calib_lm_begin checked)
            double blk[kGStride];
            std::fill(blk, blk + kGStride, 0.0);
            for (int it = vi0[v]; it < vi0[v + 1]; ++it)
                for (int i = 0; i < kGStride; ++i) blk[i] += G[(size_t)it * kGStride + i];
            const int extra = stream_extra_item(sm, v);     // stream form: the part of the view summed by a second wave
            if (extra >= 0)
                for (int i = 0; i < kGStride; ++i) blk[i] += G[(size_t)extra * kGStride + i];
            for (int a = 0; a < 6; ++a) {
                if (out_g) out_g[L + 6 * (int64_t)v + a] = blk[gvSlot(L, a)];
                for (int b = 0; b < 6; ++b)     // V is symmetric; the record holds its lower triangle (g_v rides in the upper)
                    if (out_V) out_V[((int64_t)v * 6 + a) * 6 + b] = blk[kGRows + (a >= b ? a * 16 + L + b : b * 16 + L + a)];
                for (int c = 0; c < L; ++c)
                    if (out_E) out_E[((int64_t)v * L + c) * 6 + a] = blk[kGRows + a * 16 + c];
            }
        }
    }
    return CALIB_OK;
}

int calib_distort_points(int model, int64_t n, const double* x_norm, const double* k, double* out_xd) {
    if (n < 0 || (n > 0 && (!x_norm || !out_xd)) || !k) return fail(CALIB_E_INVALID, "null argument");
    if (!known_model(model)) return fail(CALIB_E_INVALID, "unknown distortion model");
    if (n == 0) return CALIB_OK;
    const int nk = num_distortion(model);
    DevBuf<double> dx, dk, dout;
    HIP_TRY(dx.alloc((size_t)n * 2)); HIP_TRY(dk.alloc(nk)); HIP_TRY(dout.alloc((size_t)n * 2));
    HIP_TRY(hipMemcpy(dx.p, x_norm, (size_t)n * 16, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dk.p, k, (size_t)nk * 8, hipMemcpyHostToDevice));
    const unsigned blocks = (unsigned)((n + 255) / 256);
    const int rc = dispatch_model(model, [&](auto form) -> int {
        hipLaunchKernelGGL((distort_points_kernel<decltype(form)::MODEL>), dim3(blocks), dim3(256), 0, 0, dx.p, dk.p, n, dout.p);
        LAUNCHED(kNoHandle, "distort_points_kernel");
        return CALIB_OK;
    });
    if (rc) return rc;
    HIP_TRY(hipMemcpy(out_xd, dout.p, (size_t)n * 16, hipMemcpyDeviceToHost));
    return CALIB_OK;
}

int calib_project_with_distortion(int model, int64_t n, const double* A, const double* cam_xyz,
                                  const double* k, double* out_uv) {
    if (n < 0 || (n > 0 && (!cam_xyz || !out_uv)) || !k || !A) return fail(CALIB_E_INVALID, "null argument");
    if (!known_model(model)) return fail(CALIB_E_INVALID, "unknown distortion model");
    if (n == 0) return CALIB_OK;
    const int nk = num_distortion(model);
    DevBuf<double> dA, dc, dk, dout;
    HIP_TRY(dA.alloc(9)); HIP_TRY(dc.alloc((size_t)n * 3)); HIP_TRY(dk.alloc(nk)); HIP_TRY(dout.alloc((size_t)n * 2));
    HIP_TRY(hipMemcpy(dA.p, A, 72, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dc.p, cam_xyz, (size_t)n * 24, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dk.p, k, (size_t)nk * 8, hipMemcpyHostToDevice));
    const unsigned blocks = (unsigned)((n + 255) / 256);
    const int rc = dispatch_model(model, [&](auto form) -> int {
        hipLaunchKernelGGL((project_cam_kernel<decltype(form)::MODEL>), dim3(blocks), dim3(256), 0, 0, dA.p, dc.p, dk.p, n, dout.p);
        LAUNCHED(kNoHandle, "project_cam_kernel");
        return CALIB_OK;
    });
    if (rc) return rc;
    HIP_TRY(hipMemcpy(out_uv, dout.p, (size_t)n * 16, hipMemcpyDeviceToHost));
    return CALIB_OK;
}

int calib_refine_homographies(int64_t num_views, const int64_t* view_offsets, const double* sensor_uv,
                              const double* model_xyz, double* H_inout, int max_iters, int device_id) {
    return homography_pipeline(num_views, view_offsets, sensor_uv, model_xyz, H_inout, false, max_iters, device_id);
}

int calib_estimate_homographies(int64_t num_views, const int64_t* view_offsets, const double* sensor_uv,
                                const double* model_xyz, double* H_out, int refine_iters, int device_id) {
    if (num_views > 0 && view_offsets)
        for (int64_t i = 0; i < num_views; ++i)
            if (view_offsets[i + 1] - view_offsets[i] < 4)
                return fail(CALIB_E_INVALID, "a homography needs at least 4 point correspondences per view");
    return homography_pipeline(num_views, view_offsets, sensor_uv, model_xyz, H_out, true, refine_iters, device_id);
}

int calib_refine_poses(int model, int64_t num_views, const int64_t* view_offsets, const double* sensor_uv,
                       const double* model_xyz, const double* shared, double* poses_inout, int max_iters,
                       double lam_init, double lam_min, double lam_max, double err_min, double* out_sse,
                       int* out_iters, int* out_status, int device_id) {
    if (!known_model(model)) return fail(CALIB_E_INVALID, "unknown distortion model");
    if (max_iters <= 0) return fail(CALIB_E_INVALID, "max_iters must be >= 1");
    if (!shared || (num_views > 0 && !poses_inout)) return fail(CALIB_E_INVALID, "null argument");
    int rc = check_views(num_views, view_offsets, sensor_uv, model_xyz);
    if (rc || num_views == 0) return rc;
    rc = use_device(device_id);
    if (rc) return rc;
    const int L = 5 + num_distortion(model);
    const int64_t MN = view_offsets[num_views];
    const size_t M = (size_t)num_views;
    DevBuf<int64_t> doffs;
    DevBuf<double2> duv;
    DevBuf<double> dxyz, dshared, dposes, dsse;
    DevBuf<int> dint;             // iterations [0, M), status [M, 2 M)
    HIP_TRY(doffs.alloc(M + 1));
    HIP_TRY(duv.alloc((size_t)std::max<int64_t>(MN, 1)));
    HIP_TRY(dxyz.alloc((size_t)std::max<int64_t>(MN, 1) * 3));
    HIP_TRY(dshared.alloc((size_t)L));
    HIP_TRY(dposes.alloc(M * 6));
    HIP_TRY(dsse.alloc(M));
    HIP_TRY(dint.alloc(2 * M));
    HIP_TRY(hipMemcpy(doffs.p, view_offsets, (M + 1) * 8, hipMemcpyHostToDevice));
    if (MN) HIP_TRY(hipMemcpy(duv.p, sensor_uv, (size_t)MN * 16, hipMemcpyHostToDevice));
    if (MN) HIP_TRY(hipMemcpy(dxyz.p, model_xyz, (size_t)MN * 24, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dshared.p, shared, (size_t)L * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dposes.p, poses_inout, M * 48, hipMemcpyHostToDevice));
    rc = dispatch_model(model, [&](auto form) -> int {
        hipLaunchKernelGGL((pose_lm_kernel<decltype(form)::MODEL>), dim3((unsigned)((num_views + 15) / 16)), dim3(256), 0, 0,
                           doffs.p, (const double2*)duv.p, dxyz.p, dshared.p, num_views, max_iters, lam_init, lam_min, lam_max,
                           err_min, dposes.p, dsse.p, dint.p, dint.p + M);
        LAUNCHED(kNoHandle, "pose_lm_kernel");
        return CALIB_OK;
    });
    if (rc) return rc;
    HIP_TRY(hipMemcpy(poses_inout, dposes.p, M * 48, hipMemcpyDeviceToHost));
    if (out_sse) HIP_TRY(hipMemcpy(out_sse, dsse.p, M * 8, hipMemcpyDeviceToHost));
    if (out_iters) HIP_TRY(hipMemcpy(out_iters, dint.p, M * 4, hipMemcpyDeviceToHost));
    if (out_status) HIP_TRY(hipMemcpy(out_status, dint.p + M, M * 4, hipMemcpyDeviceToHost));
    return CALIB_OK;
}

int calib_homography_jacobian(int64_t n, const double* h9, const double* model_xyz, double* out_J, int device_id) {
    if (n < 0 || !h9 || (n > 0 && (!model_xyz || !out_J))) return fail(CALIB_E_INVALID, "null argument");
    if (n == 0) return CALIB_OK;
    int rc = use_device(device_id);
    if (rc) return rc;
    DevBuf<double> dh, dx, dJ;
    HIP_TRY(dh.alloc(9));
    HIP_TRY(dx.alloc((size_t)n * 3));
    HIP_TRY(dJ.alloc((size_t)n * 18));
    HIP_TRY(hipMemcpy(dh.p, h9, 72, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dx.p, model_xyz, (size_t)n * 24, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(homography_jacobian_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, dh.p, dx.p, n, dJ.p);
    LAUNCHED(kNoHandle, "homography_jacobian_kernel");
    HIP_TRY(hipMemcpy(out_J, dJ.p, (size_t)n * 18 * 8, hipMemcpyDeviceToHost));
    return CALIB_OK;
}

int calib_compute_extrinsics(int64_t num_views, const double* A, const double* H, double* W_out, int device_id) {
    if (num_views < 0 || !A || (num_views > 0 && (!H || !W_out))) return fail(CALIB_E_INVALID, "null argument");
    if (num_views == 0) return CALIB_OK;
    int rc = use_device(device_id);
    if (rc) return rc;
    // A = [[a, g, uc], [0, b, vc], [0, 0, 1]] (src/calibrate.py:252-256): closed-form inverse
    const double a = A[0], g = A[1], uc = A[2], b = A[4], vc = A[5];
    if (!(a != 0.0) || !(b != 0.0)) return fail(CALIB_E_SINGULAR, "Singular matrix: intrinsic matrix is not invertible");
    const double Ainv[9] = {1.0 / a, -g / (a * b), (g * vc - uc * b) / (a * b), 0.0, 1.0 / b, -vc / b, 0.0, 0.0, 1.0};
    DevBuf<double> dA, dH, dW;
    HIP_TRY(dA.alloc(9));
    HIP_TRY(dH.alloc((size_t)num_views * 9));
    HIP_TRY(dW.alloc((size_t)num_views * 16));
    HIP_TRY(hipMemcpy(dA.p, Ainv, 72, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dH.p, H, (size_t)num_views * 72, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(extrinsics_kernel, dim3((unsigned)((num_views + 255) / 256)), dim3(256), 0, 0, dA.p, dH.p, num_views, dW.p);
    LAUNCHED(kNoHandle, "extrinsics_kernel");
    HIP_TRY(hipMemcpy(W_out, dW.p, (size_t)num_views * 128, hipMemcpyDeviceToHost));
    return CALIB_OK;
}

int calib_distortion_normal_equations(int model, int64_t num_views, const int64_t* view_offsets,
                                      const double* sensor_uv, const double* model_xyz, const double* A,
                                      const double* W, double* out_DtD, double* out_Dtd, int device_id) {
    if (!known_model(model)) return fail(CALIB_E_INVALID, "unknown distortion model");
    if (!A || !out_DtD || !out_Dtd || (num_views > 0 && !W)) return fail(CALIB_E_INVALID, "null argument");
    int rc = check_views(num_views, view_offsets, sensor_uv, model_xyz);
    if (rc) return rc;
    const int nk = num_distortion(model);
    const int ns = nk * (nk + 1) / 2 + nk;
    std::fill(out_DtD, out_DtD + nk * nk, 0.0);
    std::fill(out_Dtd, out_Dtd + nk, 0.0);
    const int64_t MN = num_views ? view_offsets[num_views] : 0;
    if (MN == 0) return CALIB_OK;
    rc = use_device(device_id);
    if (rc) return rc;
    std::vector<double> xy((size_t)MN * 2), z((size_t)MN);
    std::vector<int> pv((size_t)MN);
    for (int64_t v = 0; v < num_views; ++v)
        for (int64_t p = view_offsets[v]; p < view_offsets[v + 1]; ++p) pv[(size_t)p] = (int)v;
    for (int64_t p = 0; p < MN; ++p) { xy[2 * p] = model_xyz[3 * p]; xy[2 * p + 1] = model_xyz[3 * p + 1]; z[p] = model_xyz[3 * p + 2]; }
    const int blocks = (int)std::min<int64_t>(1024, (MN + 255) / 256);
    DevBuf<double> dA, dW, dz, dpart;
    DevBuf<double2> duv, dxy;
    DevBuf<int> dpv;
    HIP_TRY(dA.alloc(9));
    HIP_TRY(dW.alloc((size_t)num_views * 16));
    HIP_TRY(duv.alloc((size_t)MN));
    HIP_TRY(dxy.alloc((size_t)MN));
    HIP_TRY(dz.alloc((size_t)MN));
    HIP_TRY(dpv.alloc((size_t)MN));
    HIP_TRY(dpart.alloc((size_t)blocks * ns));
    HIP_TRY(hipMemcpy(dA.p, A, 72, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dW.p, W, (size_t)num_views * 128, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(duv.p, sensor_uv, (size_t)MN * 16, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dxy.p, xy.data(), (size_t)MN * 16, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dz.p, z.data(), (size_t)MN * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dpv.p, pv.data(), (size_t)MN * 4, hipMemcpyHostToDevice));
    rc = dispatch_model(model, [&](auto form) -> int {
        hipLaunchKernelGGL((distortion_normal_kernel<decltype(form)::MODEL>), dim3(blocks), dim3(256), 0, 0, dA.p, dW.p, dpv.p,
                           (const double2*)duv.p, (const double2*)dxy.p, dz.p, MN, dpart.p);
        LAUNCHED(kNoHandle, "distortion_normal_kernel");
        return CALIB_OK;
    });
    if (rc) return rc;
    std::vector<double> part((size_t)blocks * ns);
    HIP_TRY(hipMemcpy(part.data(), dpart.p, part.size() * 8, hipMemcpyDeviceToHost));
    std::vector<double> sum((size_t)ns, 0.0);
    for (int bidx = 0; bidx < blocks; ++bidx)
        for (int j = 0; j < ns; ++j) sum[(size_t)j] += part[(size_t)bidx * ns + j];
    int idx = 0;
    for (int a2 = 0; a2 < nk; ++a2)
        for (int b2 = a2; b2 < nk; ++b2) { out_DtD[a2 * nk + b2] = sum[(size_t)idx]; out_DtD[b2 * nk + a2] = sum[(size_t)idx]; ++idx; }
    for (int a2 = 0; a2 < nk; ++a2) out_Dtd[a2] = sum[(size_t)idx++];
    return CALIB_OK;
}

int calib_compose_params(int model, int64_t num_views, const double* A, const double* W, const double* k,
                         double* P_out, int device_id) {
    if (!known_model(model)) return fail(CALIB_E_INVALID, "unknown distortion model");
    if (num_views < 0 || !A || !k || !P_out || (num_views > 0 && !W)) return fail(CALIB_E_INVALID, "null argument");
    const int nk = num_distortion(model), L = 5 + nk;
    // shared part: (alpha, beta, gamma, uc, vc, k...) from A = [[alpha, gamma, uc], [0, beta, vc], [0, 0, 1]]
    P_out[0] = A[0]; P_out[1] = A[4]; P_out[2] = A[1]; P_out[3] = A[2]; P_out[4] = A[5];
    for (int j = 0; j < nk; ++j) P_out[5 + j] = k[j];
    if (num_views == 0) return CALIB_OK;
    int rc = use_device(device_id);
    if (rc) return rc;
    DevBuf<double> dW, dP;
    HIP_TRY(dW.alloc((size_t)num_views * 16));
    HIP_TRY(dP.alloc((size_t)L + 6 * (size_t)num_views));
    HIP_TRY(hipMemcpy(dW.p, W, (size_t)num_views * 128, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(compose_views_kernel, dim3((unsigned)((num_views + 255) / 256)), dim3(256), 0, 0, dW.p, num_views, L, dP.p);
    LAUNCHED(kNoHandle, "compose_views_kernel");
    HIP_TRY(hipMemcpy(P_out + L, dP.p + L, (size_t)num_views * 48, hipMemcpyDeviceToHost));
    return CALIB_OK;
}

int calib_decompose_params(int model, int64_t num_views, const double* P, double* A_out, double* W_out,
                           double* k_out, int device_id) {
    if (!known_model(model)) return fail(CALIB_E_INVALID, "unknown distortion model");
    if (num_views < 0 || !P || (num_views > 0 && !W_out)) return fail(CALIB_E_INVALID, "null argument");
    const int nk = num_distortion(model), L = 5 + nk;
    if (A_out) {
        const double a[9] = {P[0], P[2], P[3], 0.0, P[1], P[4], 0.0, 0.0, 1.0};
        std::memcpy(A_out, a, sizeof(a));
    }
    if (k_out) for (int j = 0; j < nk; ++j) k_out[j] = P[5 + j];
    if (num_views == 0) return CALIB_OK;
    int rc = use_device(device_id);
    if (rc) return rc;
    DevBuf<double> dW, dP;
    HIP_TRY(dW.alloc((size_t)num_views * 16));
    HIP_TRY(dP.alloc((size_t)L + 6 * (size_t)num_views));
    HIP_TRY(hipMemcpy(dP.p, P, ((size_t)L + 6 * (size_t)num_views) * 8, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(decompose_views_kernel, dim3((unsigned)((num_views + 255) / 256)), dim3(256), 0, 0, dP.p, num_views, L, dW.p);
    LAUNCHED(kNoHandle, "decompose_views_kernel");
    HIP_TRY(hipMemcpy(W_out, dW.p, (size_t)num_views * 128, hipMemcpyDeviceToHost));
    return CALIB_OK;
}

int calib_refine_awk(calib_handle_t h, double* A_inout, double* W_inout, double* k_inout, int max_iters,
                     double lam_init, double lam_min, double lam_max, double err_min, double* out_sse,
                     int* out_iters, double* out_trace) {
    CHECK_H(h);
    int rc = need_problem(h);
    if (rc) return rc;
    if (!A_inout || !k_inout || (h->M > 0 && !W_inout)) return fail(CALIB_E_INVALID, "null argument");
    std::vector<double> P((size_t)numParams(h));
    rc = calib_compose_params(h->model, h->M, A_inout, W_inout, k_inout, P.data(), h->device);
    if (rc) return rc;
    rc = calib_refine(h, P.data(), max_iters, lam_init, lam_min, lam_max, err_min, out_sse, out_iters, out_trace);
    if (rc) return rc;
    return calib_decompose_params(h->model, h->M, P.data(), A_inout, W_inout, k_inout, h->device);
}

int calib_profile_enable(calib_handle_t h, int on) {
    CHECK_H(h);
    SYNC_H(h);
    if (on && h->ev.empty()) {
        h->ev.resize(kEventPool);
        h->ev_kind.assign(kEventPool / 2, 0);
        for (auto& e : h->ev) HIP_TRY(hipEventCreate(&e));
    }
    h->prof = on != 0;
    h->prof_stride = on > 1 ? on : 1;
    h->prof_seen[0] = h->prof_seen[1] = h->prof_seen[2] = 0;
    h->ev_used = 0;
    return CALIB_OK;
}

int calib_profile_read(calib_handle_t h, int which, double* out_total_ms, int64_t* out_launches) {
    CHECK_H(h);
    if (!out_total_ms || !out_launches) return fail(CALIB_E_INVALID, "null argument");
    SYNC_H(h);
    double total = 0.0;
    int64_t count = 0;
    for (size_t i = 0; i + 1 < h->ev_used; i += 2) {
        if (h->ev_kind[i / 2] != which) continue;
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, h->ev[i], h->ev[i + 1]));
        total += ms;
        count += 1;
    }
    *out_total_ms = total;
    *out_launches = count;
    return CALIB_OK;
}

int calib_view_errors(calib_handle_t h, const double* P, double* out_view_sse, double* out_view_rms,
                      double* out_view_max) {
    CHECK_H(h);
    int rc = need_problem(h);
    if (rc) return rc;
    if (!P) return fail(CALIB_E_INVALID, "P is null");
    if (h->lm_active)       // the running loop owns the view constants this evaluation would overwrite
        return fail(CALIB_E_STATE, "a stepping LM run is active on this handle (calib_lm_end it first)");
    const int64_t M = h->M;
    if (M == 0) return CALIB_OK;
    if (!h->ext_offsets_on_device) {
        HIP_TRY(h->ext_offsets_dev.alloc((size_t)M + 1));
        HIP_TRY(hipMemcpy(h->ext_offsets_dev.p, h->ext_offsets.data(), ((size_t)M + 1) * 8, hipMemcpyHostToDevice));
        h->ext_offsets_on_device = true;
    }
    HIP_TRY(h->view_err.alloc((size_t)M * 3));
    HIP_TRY(hipMemcpyAsync(h->Peval.p, P, (size_t)numParams(h) * 8, hipMemcpyHostToDevice, h->stream));
    rc = launch_view_setup(h, h->Peval.p, nullptr, h->st_eval.p, 0);
    if (rc) return rc;
    rc = dispatch(h, [&](auto form) -> int {
        using F = decltype(form);
        using T = typename F::T;
        using T2 = typename F::T2;
        const unsigned blocks = (unsigned)((M + kViewErrWaves - 1) / kViewErrWaves);
        hipLaunchKernelGGL((view_errors_kernel<F::MODEL, T>), dim3(blocks), dim3(64 * kViewErrWaves), 0, h->stream,
                           (const double*)h->Peval.p, h->uv_as<const T2>(), h->XY_as<const T2>(), h->Z_as<const T>(),
                           h->VC_as<const T>(), (const int*)h->pt_view.p, (const int64_t*)h->ext_offsets_dev.p, M,
                           h->view_err.p);
        LAUNCHED(h, "view_errors_kernel");
        return CALIB_OK;
    });
    if (rc) return rc;
    std::vector<double> tmp((size_t)M * 3);
    HIP_TRY(hipMemcpyAsync(tmp.data(), h->view_err.p, tmp.size() * 8, hipMemcpyDeviceToHost, h->stream));
    SYNC_H(h);
    for (int64_t i = 0; i < M; ++i) {
        if (out_view_sse) out_view_sse[i] = tmp[(size_t)3 * i];
        if (out_view_rms) out_view_rms[i] = tmp[(size_t)3 * i + 1];
        if (out_view_max) out_view_max[i] = tmp[(size_t)3 * i + 2];
    }
    return CALIB_OK;
}

int calib_cov_local(calib_handle_t h, const double* P) {
    CHECK_H(h);
    if (h->lm_active) return fail(CALIB_E_STATE, "a stepping LM run is active on this handle (calib_lm_end it first)");
    // the bootstrap round at lambda = 0, as calib_normal_eq runs it: variant A of the reduce buffer then holds Bsum,
    // Ssub = sum E V^-1 E^T, the count of views whose V has a pivot that is not positive, and sse(P)
    int rc = calib_lm_begin(h, P, 1, 0.0, 0.0, INFINITY, -INFINITY);
    if (rc) return rc;
    rc = calib_lm_local(h);
    h->lm_active = false;
    if (rc) return rc;
    h->cov_pending = true;
    return CALIB_OK;
}

int calib_cov_finish(calib_handle_t h, int64_t total_points, int64_t total_views, double* out_sigma2, int64_t* out_dof,
                     double* out_cov_shared, double* out_cov_views, double* out_cov_cross, double* out_std) {
    CHECK_H(h);
    if (h->lm_active) return fail(CALIB_E_STATE, "a stepping LM run is active on this handle (calib_lm_end it first)");
    if (!h->cov_pending) return fail(CALIB_E_STATE, "calib_cov_local has not been called");
    h->cov_pending = false;
    const int L = h->L;
    const int64_t M = h->M;
    if (total_points < h->MN || total_views < M) return fail(CALIB_E_INVALID, "totals are smaller than this shard");
    int nfree = 0;
    for (int i = 0; i < L; ++i) nfree += !((h->fixed_mask >> i) & 1);
    const int64_t dof = 2 * total_points - (nfree + 6 * total_views);
    if (dof <= 0) { SYNC_H(h); return fail(CALIB_E_INVALID, "no degrees of freedom left: 2 n <= number of free parameters"); }
    std::vector<double> red((size_t)variantSize(L));
    HIP_TRY(hipMemcpyAsync(red.data(), h->red, red.size() * 8, hipMemcpyDeviceToHost, h->stream));
    SYNC_H(h);
    if (red[(size_t)2 * L * L + 2 * L] > 0.0)
        return fail(CALIB_E_SINGULAR, "Singular matrix: a view's 6 x 6 block has a pivot that is not positive");
    const double sigma2 = red[(size_t)2 * L * L + 2 * L + 1] / (double)dof;
    double Css[kMaxL * kMaxL];
    if (!shared_covariance(red.data(), L, h->fixed_mask, sigma2, Css))
        return fail(CALIB_E_SINGULAR, "Singular matrix: the reduced system of the shared parameters is not positive definite");
    if (out_sigma2) *out_sigma2 = sigma2;
    if (out_dof) *out_dof = dof;
    if (out_cov_shared) std::memcpy(out_cov_shared, Css, (size_t)L * L * 8);
    if (out_std) for (int i = 0; i < L; ++i) out_std[i] = std::sqrt(Css[i * L + i]);
    if (M == 0 || !(out_cov_views || out_cov_cross || out_std)) return CALIB_OK;
    HIP_TRY(h->cov_css.alloc((size_t)kMaxL * kMaxL));
    HIP_TRY(h->cov_flag.alloc(1));
    HIP_TRY(h->cov_views.alloc((size_t)M * 36));
    if (out_cov_cross) HIP_TRY(h->cov_cross.alloc((size_t)M * L * 6));
    HIP_TRY(hipMemcpyAsync(h->cov_css.p, Css, (size_t)L * L * 8, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemsetAsync(h->cov_flag.p, 0, sizeof(int), h->stream));
    const int rc = dispatch(h, [&](auto form) -> int {
        constexpr int LL = decltype(form)::L;
        const int blocks = std::max(1, std::min((h->nv + kSchurThreads - 1) / kSchurThreads, 4 * h->num_cus));
        auto launch = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kSchurThreads), 0, h->stream, (const double*)h->G[0].p, view_items(h),
                               (const int*)h->view_ext.p, h->nv, stream_map(h), (const double*)h->cov_css.p, sigma2,
                               h->cov_views.p, out_cov_cross ? h->cov_cross.p : nullptr, h->cov_flag.p);
        };
        if (h->plan.stream()) launch(covariance_views_kernel<LL, true>); else launch(covariance_views_kernel<LL, false>);
        LAUNCHED(h, "covariance_views_kernel");
        return CALIB_OK;
    });
    if (rc) return rc;
    int flag = 0;
    HIP_TRY(hipMemcpyAsync(&flag, h->cov_flag.p, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    SYNC_H(h);
    if (flag)
        return fail(CALIB_E_SINGULAR, "Singular matrix: a view's 6 x 6 block has a pivot that is not positive");
    std::vector<double> tmp;
    double* cv = out_cov_views;
    if (!cv) { tmp.resize((size_t)M * 36); cv = tmp.data(); }
    HIP_TRY(hipMemcpy(cv, h->cov_views.p, (size_t)M * 36 * 8, hipMemcpyDeviceToHost));
    if (out_cov_cross) HIP_TRY(hipMemcpy(out_cov_cross, h->cov_cross.p, (size_t)M * L * 6 * 8, hipMemcpyDeviceToHost));
    if (out_std)
        for (int64_t v = 0; v < M; ++v)
            for (int a = 0; a < 6; ++a) out_std[L + 6 * v + a] = std::sqrt(cv[(size_t)v * 36 + a * 7]);
    return CALIB_OK;
}

int calib_covariance(calib_handle_t h, const double* P, double* out_sigma2, int64_t* out_dof, double* out_cov_shared,
                     double* out_cov_views, double* out_cov_cross, double* out_std) {
    const int rc = calib_cov_local(h, P);
    if (rc) return rc;
    return calib_cov_finish(h, h->MN, h->M, out_sigma2, out_dof, out_cov_shared, out_cov_views, out_cov_cross, out_std);
}

// ---- undistortion (undistort.hpp): the inverse model on points, the rectify maps, the bilinear remap -----------------
int calib_undistort_points(int model, int64_t n, const double* A, const double* k, const double* uv,
                           const double* newA, double* out_xy, int32_t* out_status, int device_id) {
    if (n < 0 || (n > 0 && (!uv || !out_xy)) || !k || !A) return fail(CALIB_E_INVALID, "null argument");
    if (!known_model(model)) return fail(CALIB_E_INVALID, "unknown distortion model");
    Pinhole cam, out;
    if (!pinhole_of(A, cam) || (newA && !pinhole_of(newA, out)))
        return fail(CALIB_E_INVALID, "alpha and beta of a camera matrix must not be 0");
    if (n == 0) return CALIB_OK;
    int rc = use_device(device_id);
    if (rc) return rc;
    const int nk = num_distortion(model);
    std::vector<double> xy((size_t)n * 2);                  // pixels -> distorted normalised points
    for (int64_t i = 0; i < n; ++i) {
        const double yd = (uv[2 * i + 1] - cam.vc) / cam.be;
        xy[2 * i] = (uv[2 * i] - cam.uc - cam.ga * yd) / cam.al;
        xy[2 * i + 1] = yd;
    }
    DevBuf<double2> din, dout;
    DevBuf<double> dk;
    DevBuf<int32_t> dstatus;
    HIP_TRY(din.alloc((size_t)n)); HIP_TRY(dout.alloc((size_t)n)); HIP_TRY(dk.alloc(nk)); HIP_TRY(dstatus.alloc((size_t)n));
    HIP_TRY(hipMemcpy(din.p, xy.data(), (size_t)n * 16, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dk.p, k, (size_t)nk * 8, hipMemcpyHostToDevice));
    const unsigned blocks = (unsigned)((n + 255) / 256);
    rc = dispatch_model(model, [&](auto form) -> int {
        hipLaunchKernelGGL((undistort_points_kernel<decltype(form)::MODEL>), dim3(blocks), dim3(256), 0, 0,
                           (const double2*)din.p, (const double*)dk.p, n, dout.p, dstatus.p);
        LAUNCHED(kNoHandle, "undistort_points_kernel");
        return CALIB_OK;
    });
    if (rc) return rc;
    HIP_TRY(hipMemcpy(out_xy, dout.p, (size_t)n * 16, hipMemcpyDeviceToHost));
    if (out_status) HIP_TRY(hipMemcpy(out_status, dstatus.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    if (newA)                                               // ideal normalised points -> pixels of the new camera
        for (int64_t i = 0; i < n; ++i) {
            const double x = out_xy[2 * i], y = out_xy[2 * i + 1];
            out_xy[2 * i] = out.al * x + out.ga * y + out.uc;
            out_xy[2 * i + 1] = out.be * y + out.vc;
        }
    return CALIB_OK;
}

int calib_undistort_maps(int model, const double* A, const double* k, const double* newA, int width, int height,
                         float* out_mapx, float* out_mapy, int device_id) {
    if (!A || !k || !out_mapx || !out_mapy) return fail(CALIB_E_INVALID, "null argument");
    if (!known_model(model)) return fail(CALIB_E_INVALID, "unknown distortion model");
    if (width <= 0 || height <= 0) return fail(CALIB_E_INVALID, "width and height must be positive");
    if ((int64_t)width * height > (int64_t)INT32_MAX) return fail(CALIB_E_INVALID, "a map has at most 2^31 - 1 pixels");
    Pinhole cam, dst;
    if (!pinhole_of(A, cam) || !pinhole_of(newA ? newA : A, dst))
        return fail(CALIB_E_INVALID, "alpha and beta of a camera matrix must not be 0");
    int rc = use_device(device_id);
    if (rc) return rc;
    const int nk = num_distortion(model);
    const unsigned total = (unsigned)width * (unsigned)height;
    DevBuf<double> dk;
    DevBuf<float> dmaps;                                    // mapx, then mapy from the next 16-byte boundary
    const size_t plane = ((size_t)total + 3) / 4 * 4;
    HIP_TRY(dk.alloc(nk)); HIP_TRY(dmaps.alloc(2 * plane));
    HIP_TRY(hipMemcpy(dk.p, k, (size_t)nk * 8, hipMemcpyHostToDevice));
    const unsigned perBlock = 256u * (unsigned)kMapCols;
    const unsigned blocks = (unsigned)(((uint64_t)total + perBlock - 1) / perBlock);
    rc = dispatch_model(model, [&](auto form) -> int {
        hipLaunchKernelGGL((undistort_map_kernel<decltype(form)::MODEL>), dim3(blocks), dim3(256), 0, 0, cam, dst,
                           (const double*)dk.p, (unsigned)width, total, dmaps.p, dmaps.p + plane);
        LAUNCHED(kNoHandle, "undistort_map_kernel");
        return CALIB_OK;
    });
    if (rc) return rc;
    HIP_TRY(hipMemcpy(out_mapx, dmaps.p, (size_t)total * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out_mapy, dmaps.p + plane, (size_t)total * 4, hipMemcpyDeviceToHost));
    return CALIB_OK;
}

int calib_remap(int dtype, const void* src, int src_h, int src_w, int channels, const float* mapx, const float* mapy,
                int dst_h, int dst_w, double border, void* dst, int device_id) {
    if (!src || !mapx || !mapy || !dst) return fail(CALIB_E_INVALID, "null argument");
    if (dtype != CALIB_IMAGE_U8 && dtype != CALIB_IMAGE_F32) return fail(CALIB_E_INVALID, "unknown image dtype");
    if (channels < 1 || channels > 4) return fail(CALIB_E_INVALID, "an image has 1 to 4 channels");
    if (src_h <= 0 || src_w <= 0 || dst_h <= 0 || dst_w <= 0) return fail(CALIB_E_INVALID, "image sizes must be positive");
    if ((dst_w + 63) / 64 > 65535) return fail(CALIB_E_INVALID, "destination too wide (at most 4194240 columns)");
    const int rc = use_device(device_id);
    if (rc) return rc;
    return dtype == CALIB_IMAGE_U8
               ? remap_typed<uint8_t>(src, src_h, src_w, channels, mapx, mapy, dst_h, dst_w, border, dst)
               : remap_typed<float>(src, src_h, src_w, channels, mapx, mapy, dst_h, dst_w, border, dst);
}

}  // extern "C"

// ---- the four solvers on the LM loop of stereo_loop.hpp: two known cameras (calib_stereo_*), joint stereo
// ---- (calib_stereo_joint_*), N known cameras (calib_rig_*), the joint rig (calib_rig_joint_*). Their host side is
// ---- solver_host.hpp, which needs this file's helpers above; what is left here is each solver's two launch functions,
// ---- the descriptor that names them and, at the end of the file, the twelve entry points. The launch functions stay
// ---- where they were among the sections that follow: the module emits a kernel template where it is first launched,
// ---- and a kernel that changes its place changes every label after it (tools/isa_diff.py).
#include "solver_host.hpp"

namespace {

// ---- the rig between two known cameras (stereo.hpp) --------------------------------------------------------------------
int rig_evaluate(const StereoRun& r) {
    const StereoCam ca = r.cam[0].view(), cb = r.cam[1].view();
    const StereoBufs bf = r.bufs;
    const unsigned grid = (unsigned)r.nwgA;
    const int rc = dispatch_model(r.model[0], [&](auto fa) -> int {
        return dispatch_model(r.model[1], [&](auto fb) -> int {
            hipLaunchKernelGGL((stereo_blocks_kernel<decltype(fa)::MODEL, decltype(fb)::MODEL>), dim3(grid), dim3(256),
                               0, 0, ca, r.cam[0].shared.p, cb, r.cam[1].shared.p, bf);
            LAUNCHED(kNoHandle, "stereo_blocks_kernel");
            return CALIB_OK;
        });
    });
    if (rc) return rc;
    hipLaunchKernelGGL(stereo_decide_kernel<kStTot>, dim3(1), dim3(256), 0, 0, bf, r.nwgA);
    LAUNCHED(kNoHandle, "stereo_decide_kernel");
    return CALIB_OK;
}

int rig_step(const StereoRun& r) {
    const StereoBufs bf = r.bufs;
    hipLaunchKernelGGL(stereo_schur_kernel<16>, dim3((unsigned)r.nwgC), dim3(256), 0, 0, r.cam[0].view(), r.cam[1].view(), bf);
    LAUNCHED(kNoHandle, "stereo_schur_kernel");
    hipLaunchKernelGGL(stereo_rig_kernel<kStSchur>, dim3(1), dim3(256), 0, 0, bf, r.nwgC);
    LAUNCHED(kNoHandle, "stereo_rig_kernel");
    hipLaunchKernelGGL((stereo_backsub_kernel<StereoRecord, 6>), dim3((unsigned)((r.M + 63) / 64)), dim3(64), 0, 0, bf);
    LAUNCHED(kNoHandle, "stereo_backsub_kernel");
    return CALIB_OK;
}

}  // namespace

// ---- using a calibrated rig (rectify.hpp): rectify maps, rectified points, triangulation -------------------------
namespace {

// a (3,3) row-major rotation, NULL = identity; false unless |det R - 1| <= 1e-6
bool rotation_of(const double* R, double (&m)[9]) {
    static const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    for (int j = 0; j < 9; ++j) m[j] = R ? R[j] : I[j];
    const double det = m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) +
                       m[2] * (m[3] * m[7] - m[4] * m[6]);
    return std::fabs(det - 1.0) <= 1e-6;                    // false for NaN
}

// One camera's side of calib_triangulate: the pixels and the ideal normalised points undistort_points_kernel finds for
// them, all on the device.
struct TriSide {
    DevBuf<double2> uv, xd, xy;
    DevBuf<double> k;
    DevBuf<int32_t> status;

    int run(int model, const Pinhole& cam, const double* kHost, int64_t n, const double* uvHost) {
        const int nk = num_distortion(model);
        std::vector<double> norm((size_t)n * 2);            // pixels -> distorted normalised points
        for (int64_t i = 0; i < n; ++i) {
            const double yd = (uvHost[2 * i + 1] - cam.vc) / cam.be;
            norm[2 * i] = (uvHost[2 * i] - cam.uc - cam.ga * yd) / cam.al;
            norm[2 * i + 1] = yd;
        }
        HIP_TRY(uv.alloc((size_t)n)); HIP_TRY(xd.alloc((size_t)n)); HIP_TRY(xy.alloc((size_t)n));
        HIP_TRY(k.alloc(nk)); HIP_TRY(status.alloc((size_t)n));
        HIP_TRY(hipMemcpy(uv.p, uvHost, (size_t)n * 16, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(xd.p, norm.data(), (size_t)n * 16, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(k.p, kHost, (size_t)nk * 8, hipMemcpyHostToDevice));
        const unsigned blocks = (unsigned)((n + 255) / 256);
        return dispatch_model(model, [&](auto form) -> int {
            hipLaunchKernelGGL((undistort_points_kernel<decltype(form)::MODEL>), dim3(blocks), dim3(256), 0, 0,
                               (const double2*)xd.p, (const double*)k.p, n, xy.p, status.p);
            LAUNCHED(kNoHandle, "undistort_points_kernel");
            return CALIB_OK;
        });
    }
};

}  // namespace

extern "C" {

int calib_rectify_maps(int model, const double* A, const double* k, const double* R, const double* P, int width,
                       int height, float* out_mapx, float* out_mapy, int device_id) {
    if (!A || !k || !P || !out_mapx || !out_mapy) return fail(CALIB_E_INVALID, "null argument");
    if (!known_model(model)) return fail(CALIB_E_INVALID, "unknown distortion model");
    if (width <= 0 || height <= 0) return fail(CALIB_E_INVALID, "width and height must be positive");
    if ((int64_t)width * height > (int64_t)INT32_MAX) return fail(CALIB_E_INVALID, "a map has at most 2^31 - 1 pixels");
    Pinhole cam, dst;
    if (!pinhole_of(A, cam) || !pinhole_of(P, dst))
        return fail(CALIB_E_INVALID, "alpha and beta of a camera matrix must not be 0");
    Rot3 rot;
    if (!rotation_of(R, rot.m)) return fail(CALIB_E_INVALID, "R is not a rotation (|det R - 1| > 1e-6)");
    int rc = use_device(device_id);
    if (rc) return rc;
    const int nk = num_distortion(model);
    const unsigned total = (unsigned)width * (unsigned)height;
    DevBuf<double> dk;
    DevBuf<float> dmaps;                                    // mapx, then mapy from the next 16-byte boundary
    const size_t plane = ((size_t)total + 3) / 4 * 4;
    HIP_TRY(dk.alloc(nk)); HIP_TRY(dmaps.alloc(2 * plane));
    HIP_TRY(hipMemcpy(dk.p, k, (size_t)nk * 8, hipMemcpyHostToDevice));
    const unsigned perBlock = 256u * (unsigned)kMapCols;
    const unsigned blocks = (unsigned)(((uint64_t)total + perBlock - 1) / perBlock);
    rc = dispatch_model(model, [&](auto form) -> int {
        hipLaunchKernelGGL((rectify_map_kernel<decltype(form)::MODEL>), dim3(blocks), dim3(256), 0, 0, cam, dst, rot,
                           (const double*)dk.p, (unsigned)width, total, dmaps.p, dmaps.p + plane);
        LAUNCHED(kNoHandle, "rectify_map_kernel");
        return CALIB_OK;
    });
    if (rc) return rc;
    HIP_TRY(hipMemcpy(out_mapx, dmaps.p, (size_t)total * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out_mapy, dmaps.p + plane, (size_t)total * 4, hipMemcpyDeviceToHost));
    return CALIB_OK;
}

int calib_rectify_points(int model, int64_t n, const double* A, const double* k, const double* uv, const double* R,
                         const double* P, double* out_uv, int32_t* out_status, int device_id) {
    if (n < 0 || (n > 0 && (!uv || !out_uv)) || !k || !A || !P) return fail(CALIB_E_INVALID, "null argument");
    if (!known_model(model)) return fail(CALIB_E_INVALID, "unknown distortion model");
    Pinhole cam, dst;
    if (!pinhole_of(A, cam) || !pinhole_of(P, dst))
        return fail(CALIB_E_INVALID, "alpha and beta of a camera matrix must not be 0");
    double m[9];
    if (!rotation_of(R, m)) return fail(CALIB_E_INVALID, "R is not a rotation (|det R - 1| > 1e-6)");
    if (n == 0) return CALIB_OK;
    std::vector<int32_t> status((size_t)n);
    const int rc = calib_undistort_points(model, n, A, k, uv, nullptr, out_uv, status.data(), device_id);
    if (rc) return rc;
    const double nan = std::nan("");
    for (int64_t i = 0; i < n; ++i) {                       // ideal normalised points -> the rotated frame -> pixels of P
        const double x = out_uv[2 * i], y = out_uv[2 * i + 1];
        const double X = m[0] * x + m[1] * y + m[2], Y = m[3] * x + m[4] * y + m[5], Z = m[6] * x + m[7] * y + m[8];
        const bool ok = status[(size_t)i] == 0 && Z > 0.0;
        const double px = X / Z, py = Y / Z;
        out_uv[2 * i] = ok ? dst.al * px + dst.ga * py + dst.uc : nan;
        out_uv[2 * i + 1] = ok ? dst.be * py + dst.vc : nan;
        status[(size_t)i] = ok ? 0 : 1;
    }
    if (out_status) std::copy(status.begin(), status.end(), out_status);
    return CALIB_OK;
}

int calib_triangulate(int model_a, const double* Aa, const double* ka, int model_b, const double* Ab, const double* kb,
                      const double* R, const double* t, int64_t n, const double* uv_a, const double* uv_b, double* out_X,
                      double* out_sse, int32_t* out_status, int device_id) {
    if (n < 0 || (n > 0 && (!uv_a || !uv_b || !out_X)) || !Aa || !ka || !Ab || !kb || !R || !t)
        return fail(CALIB_E_INVALID, "null argument");
    if (!known_model(model_a) || !known_model(model_b)) return fail(CALIB_E_INVALID, "unknown distortion model");
    Pinhole ca, cb;
    if (!pinhole_of(Aa, ca) || !pinhole_of(Ab, cb))
        return fail(CALIB_E_INVALID, "alpha and beta of a camera matrix must not be 0");
    Rigid rig;
    if (!rotation_of(R, rig.R)) return fail(CALIB_E_INVALID, "R is not a rotation (|det R - 1| > 1e-6)");
    for (int j = 0; j < 3; ++j) rig.t[j] = t[j];
    if (n == 0) return CALIB_OK;
    int rc = use_device(device_id);
    if (rc) return rc;
    TriSide a, b;
    rc = a.run(model_a, ca, ka, n, uv_a);
    if (rc) return rc;
    rc = b.run(model_b, cb, kb, n, uv_b);
    if (rc) return rc;
    DevBuf<double> dX, dsse;
    DevBuf<int32_t> dstatus;
    HIP_TRY(dX.alloc((size_t)n * 3)); HIP_TRY(dsse.alloc((size_t)n)); HIP_TRY(dstatus.alloc((size_t)n));
    const unsigned blocks = (unsigned)((n + 255) / 256);
    rc = dispatch_model(model_a, [&](auto fa) -> int {
        return dispatch_model(model_b, [&](auto fb) -> int {
            hipLaunchKernelGGL((triangulate_kernel<decltype(fa)::MODEL, decltype(fb)::MODEL>), dim3(blocks), dim3(256), 0, 0,
                               ca, (const double*)a.k.p, cb, (const double*)b.k.p, rig, n, (const double2*)a.xy.p,
                               (const int32_t*)a.status.p, (const double2*)b.xy.p, (const int32_t*)b.status.p,
                               (const double2*)a.uv.p, (const double2*)b.uv.p, dX.p, dsse.p, dstatus.p);
            LAUNCHED(kNoHandle, "triangulate_kernel");
            return CALIB_OK;
        });
    });
    if (rc) return rc;
    HIP_TRY(hipMemcpy(out_X, dX.p, (size_t)n * 24, hipMemcpyDeviceToHost));
    if (out_sse) HIP_TRY(hipMemcpy(out_sse, dsse.p, (size_t)n * 8, hipMemcpyDeviceToHost));
    if (out_status) HIP_TRY(hipMemcpy(out_status, dstatus.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    return CALIB_OK;
}

}  // extern "C"

namespace {

// ---- joint stereo: both cameras, the rig and the poses (stereo_joint.hpp) ----------------------------------------------
// the two models of a joint call as compile-time shared counts
template <typename F>
int dispatch_joint(int model_a, int model_b, F&& f) {
    return dispatch_model(model_a, [&](auto fa) -> int {
        return dispatch_model(model_b, [&](auto fb) -> int { return f(fa, fb); });
    });
}

int joint_evaluate(const StereoRun& r) {
    const StereoCam ca = r.cam[0].view(), cb = r.cam[1].view();
    const StereoBufs bf = r.bufs;
    const unsigned grid = (unsigned)r.nwgA;
    const int nwg = r.nwgA;
    return dispatch_joint(r.model[0], r.model[1], [&](auto fa, auto fb) -> int {
        constexpr int MA = decltype(fa)::MODEL, MB = decltype(fb)::MODEL;
        hipLaunchKernelGGL((stereo_joint_blocks_kernel<MA, MB>), dim3(grid), dim3(64 * kJWaves), 0, 0, ca, cb, bf);
        LAUNCHED(kNoHandle, "stereo_joint_blocks_kernel");
        hipLaunchKernelGGL((stereo_joint_decide_kernel<ModelTraits<MA>::L, ModelTraits<MB>::L>), dim3(1), dim3(256), 0, 0,
                           bf, nwg);
        LAUNCHED(kNoHandle, "stereo_joint_decide_kernel");
        return CALIB_OK;
    });
}

int joint_step(const StereoRun& r) {
    const StereoCam ca = r.cam[0].view(), cb = r.cam[1].view();
    const StereoBufs bf = r.bufs;
    const int nwg = r.nwgC;
    const unsigned gridB = (unsigned)((r.M + 63) / 64);
    return dispatch_joint(r.model[0], r.model[1], [&](auto fa, auto fb) -> int {
        constexpr int LA = ModelTraits<decltype(fa)::MODEL>::L, LB = ModelTraits<decltype(fb)::MODEL>::L;
        using Y = JointLayout<LA, LB>;
        hipLaunchKernelGGL((stereo_joint_schur_kernel<LA, LB>), dim3((unsigned)nwg), dim3(256), 0, 0, ca, cb, bf);
        LAUNCHED(kNoHandle, "stereo_joint_schur_kernel");
        hipLaunchKernelGGL((stereo_joint_solve_kernel<LA, LB>), dim3(1), dim3(256), 0, 0, bf, nwg);
        LAUNCHED(kNoHandle, "stereo_joint_solve_kernel");
        hipLaunchKernelGGL((stereo_backsub_kernel<Y, Y::S>), dim3(gridB), dim3(64), 0, 0, bf);
        LAUNCHED(kNoHandle, "stereo_joint_backsub_kernel");
        return CALIB_OK;
    });
}

// ---- the rig of N known cameras (rig.hpp) ------------------------------------------------------------------------------
// the number of cameras of a rig call as a compile-time argument
template <typename F>
int dispatch_cameras(int n, F&& f) {
    switch (n) {
        case 2: return f(std::integral_constant<int, 2>{});
        case 3: return f(std::integral_constant<int, 3>{});
        case 4: return f(std::integral_constant<int, 4>{});
        case 5: return f(std::integral_constant<int, 5>{});
        case 6: return f(std::integral_constant<int, 6>{});
        case 7: return f(std::integral_constant<int, 7>{});
        case 8: return f(std::integral_constant<int, 8>{});
    }
    return fail(CALIB_E_INVALID, "a rig has 2 to 8 cameras");
}
static_assert(CALIB_RIG_MAX_CAMERAS == kRigMaxCams, "the C ABI's camera count is the kernels'");

RigCams rig_cams(const StereoRun& r) {
    RigCams rc{};
    for (int c = 0; c < r.ncam; ++c) {
        rc.cam[c] = r.cam[c].view();
        rc.shared[c] = r.cam[c].shared.p;
        rc.model[c] = r.model[c];
    }
    return rc;
}

int multi_evaluate(const StereoRun& r) {
    const RigCams rc = rig_cams(r);
    const StereoBufs bf = r.bufs;
    const int nwg = r.nwgA;
    return dispatch_cameras(r.ncam, [&](auto nc) -> int {
        constexpr int NC = decltype(nc)::value;
        hipLaunchKernelGGL(rig_blocks_kernel<NC>, dim3((unsigned)nwg), dim3(256), 0, 0, rc, bf);
        LAUNCHED(kNoHandle, "rig_blocks_kernel");
        hipLaunchKernelGGL(rig_decide_kernel<NC>, dim3(1), dim3(256), 0, 0, bf, nwg);
        LAUNCHED(kNoHandle, "rig_decide_kernel");
        return CALIB_OK;
    });
}

int multi_step(const StereoRun& r) {
    const RigCams rc = rig_cams(r);
    const StereoBufs bf = r.bufs;
    const int nwg = r.nwgC;
    const unsigned gridB = (unsigned)((r.M + 63) / 64);
    return dispatch_cameras(r.ncam, [&](auto nc) -> int {
        constexpr int NC = decltype(nc)::value;
        using Y = RigLayout<NC>;
        hipLaunchKernelGGL(rig_schur_kernel<NC>, dim3((unsigned)nwg), dim3(256), 0, 0, rc, bf);
        LAUNCHED(kNoHandle, "rig_schur_kernel");
        hipLaunchKernelGGL(rig_solve_kernel<NC>, dim3(1), dim3(256), 0, 0, bf, nwg);
        LAUNCHED(kNoHandle, "rig_solve_kernel");
        hipLaunchKernelGGL((stereo_backsub_kernel<Y, Y::S>), dim3(gridB), dim3(64), 0, 0, bf);
        LAUNCHED(kNoHandle, "rig_backsub_kernel");
        return CALIB_OK;
    });
}

}  // namespace

// ---- N-view triangulation: one point from every camera of a rig that saw it (triangulate_multi.hpp) ----------------
extern "C" {

int calib_triangulate_multi(int num_cameras, const calib_view_camera_t* cameras, int64_t n, const double* uv,
                            const uint32_t* seen, double* out_X, double* out_sse, int32_t* out_status, double* out_cov,
                            double* out_res, int device_id) {
    if (num_cameras < 2 || num_cameras > CALIB_RIG_MAX_CAMERAS) return fail(CALIB_E_INVALID, "a rig has 2 to 8 cameras");
    if (!cameras || n < 0 || (n > 0 && (!uv || !out_X))) return fail(CALIB_E_INVALID, "null argument");
    const size_t N = (size_t)num_cameras;
    TriCameras cs{};
    cs.n = num_cameras;
    for (size_t c = 0; c < N; ++c) {
        const calib_view_camera_t& in = cameras[c];
        TriCamera& cm = cs.c[c];
        if (!in.A || !in.k) return fail(CALIB_E_INVALID, "null argument");
        if (!known_model(in.model)) return fail(CALIB_E_INVALID, "unknown distortion model");
        if (!pinhole_of(in.A, cm.cam)) return fail(CALIB_E_INVALID, "alpha and beta of a camera matrix must not be 0");
        if (!rotation_of(in.R, cm.T.R)) return fail(CALIB_E_INVALID, "R is not a rotation (|det R - 1| > 1e-6)");
        for (int j = 0; j < 3; ++j) cm.T.t[j] = in.t ? in.t[j] : 0.0;
        for (int j = 0; j < num_distortion(in.model); ++j) cm.k[j] = in.k[j];
        cm.model = in.model;
    }
    const uint32_t all = (1u << num_cameras) - 1u;
    if (seen)
        for (int64_t i = 0; i < n; ++i)
            if (seen[i] & ~all) return fail(CALIB_E_INVALID, "seen: a bit at or above the number of cameras is set");
    if (n == 0) return CALIB_OK;
    int rc = use_device(device_id);
    if (rc) return rc;

    // pixels -> distorted normalised points, camera-major like uv; an unseen pixel is not read: its slot holds 0
    const size_t cnt = (size_t)n;
    std::vector<double> norm(N * cnt * 2, 0.0);
    std::vector<uint32_t> mask(cnt, all);
    if (seen) std::copy(seen, seen + cnt, mask.begin());
    for (size_t c = 0; c < N; ++c) {
        const Pinhole& cam = cs.c[c].cam;
        const double* src = uv + c * cnt * 2;
        double* dst = norm.data() + c * cnt * 2;
        for (size_t i = 0; i < cnt; ++i) {
            if (!((mask[i] >> c) & 1u)) continue;
            const double yd = (src[2 * i + 1] - cam.vc) / cam.be;
            dst[2 * i] = (src[2 * i] - cam.uc - cam.ga * yd) / cam.al;
            dst[2 * i + 1] = yd;
        }
    }
    DevBuf<double2> duv, dxd, dxy, dres;
    DevBuf<double> dk, dX, dsse, dcov;
    DevBuf<int32_t> dinv, dstatus;
    DevBuf<uint32_t> dseen;
    HIP_TRY(duv.alloc(N * cnt)); HIP_TRY(dxd.alloc(N * cnt)); HIP_TRY(dxy.alloc(N * cnt)); HIP_TRY(dinv.alloc(N * cnt));
    HIP_TRY(dk.alloc(N * 5)); HIP_TRY(dseen.alloc(cnt));
    HIP_TRY(dX.alloc(cnt * 3)); HIP_TRY(dsse.alloc(cnt)); HIP_TRY(dstatus.alloc(cnt));
    if (out_cov) HIP_TRY(dcov.alloc(cnt * 6));
    if (out_res) HIP_TRY(dres.alloc(N * cnt));
    std::vector<double> kAll(N * 5, 0.0);
    for (size_t c = 0; c < N; ++c) std::copy(cs.c[c].k, cs.c[c].k + 5, kAll.begin() + 5 * c);
    HIP_TRY(hipMemcpy(duv.p, uv, N * cnt * 16, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dxd.p, norm.data(), N * cnt * 16, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dk.p, kAll.data(), N * 5 * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dseen.p, mask.data(), cnt * 4, hipMemcpyHostToDevice));
    const unsigned blocks = (unsigned)((n + 255) / 256);
    for (size_t c = 0; c < N; ++c) {            // the ideal normalised points, as calib_undistort_points finds them
        rc = dispatch_model(cs.c[c].model, [&](auto form) -> int {
            hipLaunchKernelGGL((undistort_points_kernel<decltype(form)::MODEL>), dim3(blocks), dim3(256), 0, 0,
                               (const double2*)(dxd.p + c * cnt), (const double*)(dk.p + 5 * c), n, dxy.p + c * cnt,
                               dinv.p + c * cnt);
            LAUNCHED(kNoHandle, "undistort_points_kernel");
            return CALIB_OK;
        });
        if (rc) return rc;
    }
    hipLaunchKernelGGL(triangulate_multi_kernel<256>, dim3(blocks), dim3(256), 0, 0, cs, n, (const double2*)duv.p,
                       (const double2*)dxy.p, (const int32_t*)dinv.p, (const uint32_t*)dseen.p, dX.p, dsse.p, dstatus.p,
                       dcov.p, dres.p);
    LAUNCHED(kNoHandle, "triangulate_multi_kernel");
    HIP_TRY(hipMemcpy(out_X, dX.p, cnt * 24, hipMemcpyDeviceToHost));
    if (out_sse) HIP_TRY(hipMemcpy(out_sse, dsse.p, cnt * 8, hipMemcpyDeviceToHost));
    if (out_status) HIP_TRY(hipMemcpy(out_status, dstatus.p, cnt * 4, hipMemcpyDeviceToHost));
    if (out_cov) HIP_TRY(hipMemcpy(out_cov, dcov.p, cnt * 48, hipMemcpyDeviceToHost));
    if (out_res) HIP_TRY(hipMemcpy(out_res, dres.p, N * cnt * 16, hipMemcpyDeviceToHost));
    return CALIB_OK;
}

}  // extern "C"

namespace {

// ---- the joint rig: N cameras, their rigs and the poses in one problem (rig_joint.hpp) ---------------------------------
static_assert(kRjMaxS == 16 * CALIB_RIG_MAX_CAMERAS - 6, "eight radtan cameras");

RigJointArgs rig_joint_args(const StereoRun& r) {
    RigJointArgs a{};
    a.d = r.sv.rj;
    for (int c = 0; c < r.ncam; ++c) a.cam[c] = r.cam[c].view();
    a.dsh = r.dshq.p;
    a.fixed[0] = r.fixed.w[0]; a.fixed[1] = r.fixed.w[1];
    return a;
}

int rig_joint_evaluate(const StereoRun& r) {
    const RigJointArgs a = rig_joint_args(r);
    const StereoBufs bf = r.bufs;
    hipLaunchKernelGGL(rig_joint_blocks_kernel<kRigMaxCams>, dim3((unsigned)r.nwgA), dim3(64 * kRjWaves), 0, 0, a, bf);
    LAUNCHED(kNoHandle, "rig_joint_blocks_kernel");
    hipLaunchKernelGGL(rig_joint_decide_kernel<kRigMaxCams>, dim3(1), dim3(256), 0, 0, a, bf, r.nwgA);
    LAUNCHED(kNoHandle, "rig_joint_decide_kernel");
    return CALIB_OK;
}

int rig_joint_step(const StereoRun& r) {
    const RigJointArgs a = rig_joint_args(r);
    const StereoBufs bf = r.bufs;
    hipLaunchKernelGGL(rig_joint_schur_kernel<kRigMaxCams>, dim3((unsigned)r.nwgC), dim3(256), 0, 0, a, bf);
    LAUNCHED(kNoHandle, "rig_joint_schur_kernel");
    hipLaunchKernelGGL(rig_joint_solve_kernel<kRigMaxCams>, dim3(1), dim3(256), 0, 0, a, bf, r.nwgC);
    LAUNCHED(kNoHandle, "rig_joint_solve_kernel");
    hipLaunchKernelGGL(rig_joint_backsub_kernel<kRigMaxCams>, dim3((unsigned)((r.M + 63) / 64)), dim3(64), 0, 0, a, bf);
    LAUNCHED(kNoHandle, "rig_joint_backsub_kernel");
    return CALIB_OK;
}

// the blocks of the problem re-weighted by the run's loss; the decision runs on the sums of rho
int rig_joint_robust_evaluate(const StereoRun& r) {
    const RigJointArgs a = rig_joint_args(r);
    const StereoBufs bf = r.bufs;
    hipLaunchKernelGGL(rig_joint_robust_blocks_kernel<kRigMaxCams>, dim3((unsigned)r.nwgA), dim3(64 * kRjWaves), 0, 0, a, bf,
                       r.loss);
    LAUNCHED(kNoHandle, "rig_joint_robust_blocks_kernel");
    hipLaunchKernelGGL(rig_joint_decide_kernel<kRigMaxCams>, dim3(1), dim3(256), 0, 0, a, bf, r.nwgA);
    LAUNCHED(kNoHandle, "rig_joint_decide_kernel");
    return CALIB_OK;
}

int rig_joint_residuals(const StereoRun& r, const double* Pq, double* out) {
    const RigJointArgs a = rig_joint_args(r);
    const unsigned grid = (unsigned)std::min<int64_t>((r.M + kRjResidualWaves - 1) / kRjResidualWaves, kRjResidualGrid);
    hipLaunchKernelGGL(rig_residuals_kernel<kRigMaxCams>, dim3(grid), dim3(64 * kRjResidualWaves), 0, 0, a, Pq, r.M,
                       reinterpret_cast<double2*>(out));
    LAUNCHED(kNoHandle, "rig_residuals_kernel");
    return CALIB_OK;
}

// ---- one descriptor per solver -----------------------------------------------------------------------------------------
StereoSolver solver_desc(SolverKind kind, const int* model, int num_cameras) {
    StereoSolver sv{};
    switch (kind) {
        case kSolveStereo:
            sv = StereoSolver{6, kStRecord, kStTot, kStSchur, 16, rig_evaluate, rig_step,
                              "stereo normal equations singular: a view with fewer than three points in total or a pivot that "
                              "is not positive, or a rig that no view with points in camera b constrains"};
            sv.map = stereo_block_map();
            break;
        case kSolveStereoJoint:
            dispatch_joint(model[0], model[1], [&](auto fa, auto fb) -> int {
                constexpr int LA = ModelTraits<decltype(fa)::MODEL>::L, LB = ModelTraits<decltype(fb)::MODEL>::L;
                using Y = JointLayout<LA, LB>;
                sv = StereoSolver{Y::S, kJRecord, Y::kTot, Y::kSchur, kJWaves, joint_evaluate, joint_step,
                                  "joint stereo normal equations singular: a view with fewer than three points in total, or a "
                                  "pivot of a view block or of the shared system that is not positive (a free parameter that "
                                  "no point constrains)"};
                sv.map = joint_block_map<LA, LB>();
                return CALIB_OK;
            });
            break;
        case kSolveRig:
            dispatch_cameras(num_cameras, [&](auto nc) -> int {
                using Y = RigLayout<decltype(nc)::value>;
                sv = StereoSolver{Y::S, Y::kStride, Y::kTot, Y::kSchur, 16, multi_evaluate, multi_step,
                                  "rig normal equations singular: a view with fewer than three points over all cameras, or a "
                                  "pivot of a view block or of the reduced system that is not positive (a camera other than "
                                  "camera 0 that sees nothing)"};
                sv.map = rig_block_map<decltype(nc)::value>();
                return CALIB_OK;
            });
            break;
        case kSolveRigJoint: {
            const RigJointDesc y = rig_joint_desc(model, num_cameras);
            sv = StereoSolver{y.S, y.kStride, y.kTot, y.kSchur, kRjWaves, rig_joint_evaluate, rig_joint_step,
                              "joint rig normal equations singular: a view with fewer than three points over all cameras, or a "
                              "pivot of a view block or of the reduced system that is not positive (a free parameter that no "
                              "point constrains, such as a free camera that sees nothing)"};
            sv.views_c = kRjSchurViews;
            sv.grid_a = kRjBlocksGrid;
            sv.grid_c = kRjSchurGrid;
            sv.rig_joint = true;
            sv.evaluate_robust = rig_joint_robust_evaluate;
            sv.residuals = rig_joint_residuals;
            sv.rj = y;
            sv.map = rig_joint_block_map(y);
            break;
        }
    }
    sv.known_cameras = !solver_is_joint(kind);
    return sv;
}

}  // namespace

// ---- the entry points of the four solvers
extern "C" {

int calib_stereo_normal_eq(const calib_stereo_problem_t* problem, const double* Ps, double* out_B, double* out_E,
                           double* out_V, double* out_g, double* out_sse_ab, int device_id) {
    return solver_normal_eq(kSolveStereo, problem, Ps, out_B, out_E, out_V, out_g, out_sse_ab, device_id);
}

int calib_stereo_step_delta(const calib_stereo_problem_t* problem, const double* Ps, double lambda, double* out_delta,
                            int device_id) {
    return solver_step_delta(kSolveStereo, problem, Ps, SolverMask(), lambda, out_delta, device_id);
}

int calib_refine_stereo(const calib_stereo_problem_t* problem, double* Ps_inout, int max_iters, double lam_init,
                        double lam_min, double lam_max, double err_min, double* out_sse, double* out_sse_ab,
                        int* out_iters, double* out_trace, int device_id) {
    return solver_refine(kSolveStereo, problem, Ps_inout, SolverMask(), max_iters, lam_init, lam_min, lam_max, err_min, out_sse,
                         out_sse_ab, out_iters, out_trace, device_id);
}

int calib_stereo_joint_normal_eq(const calib_stereo_problem_t* problem, const double* Pj, double* out_B, double* out_E,
                                 double* out_V, double* out_g, double* out_sse_ab, int device_id) {
    return solver_normal_eq(kSolveStereoJoint, problem, Pj, out_B, out_E, out_V, out_g, out_sse_ab, device_id);
}

int calib_stereo_joint_step_delta(const calib_stereo_problem_t* problem, const double* Pj, uint64_t fixed_mask,
                                  double lambda, double* out_delta, int device_id) {
    return solver_step_delta(kSolveStereoJoint, problem, Pj, SolverMask(fixed_mask), lambda, out_delta, device_id);
}

int calib_refine_stereo_joint(const calib_stereo_problem_t* problem, double* Pj_inout, uint64_t fixed_mask, int max_iters,
                              double lam_init, double lam_min, double lam_max, double err_min, double* out_sse,
                              double* out_sse_ab, int* out_iters, double* out_trace, int device_id) {
    return solver_refine(kSolveStereoJoint, problem, Pj_inout, SolverMask(fixed_mask), max_iters, lam_init, lam_min, lam_max,
                         err_min, out_sse, out_sse_ab, out_iters, out_trace, device_id);
}

int calib_rig_normal_eq(const calib_rig_problem_t* problem, const double* Pr, double* out_B, double* out_E, double* out_V,
                        double* out_g, double* out_sse_cam, int device_id) {
    return solver_normal_eq(kSolveRig, problem, Pr, out_B, out_E, out_V, out_g, out_sse_cam, device_id);
}

int calib_rig_step_delta(const calib_rig_problem_t* problem, const double* Pr, double lambda, double* out_delta,
                         int device_id) {
    return solver_step_delta(kSolveRig, problem, Pr, SolverMask(), lambda, out_delta, device_id);
}

int calib_refine_rig(const calib_rig_problem_t* problem, double* Pr_inout, int max_iters, double lam_init, double lam_min,
                     double lam_max, double err_min, double* out_sse, double* out_sse_cam, int* out_iters, double* out_trace,
                     int device_id) {
    return solver_refine(kSolveRig, problem, Pr_inout, SolverMask(), max_iters, lam_init, lam_min, lam_max, err_min, out_sse,
                         out_sse_cam, out_iters, out_trace, device_id);
}

int calib_rig_joint_normal_eq(const calib_rig_problem_t* problem, const double* Pq, double* out_B, double* out_E,
                              double* out_V, double* out_g, double* out_sse_cam, int device_id) {
    return solver_normal_eq(kSolveRigJoint, problem, Pq, out_B, out_E, out_V, out_g, out_sse_cam, device_id);
}

int calib_rig_joint_step_delta(const calib_rig_problem_t* problem, const double* Pq, const uint64_t* fixed_mask,
                               double lambda, double* out_delta, int device_id) {
    return solver_step_delta(kSolveRigJoint, problem, Pq, SolverMask(fixed_mask), lambda, out_delta, device_id);
}

int calib_refine_rig_joint(const calib_rig_problem_t* problem, double* Pq_inout, const uint64_t* fixed_mask, int max_iters,
                           double lam_init, double lam_min, double lam_max, double err_min, double* out_sse,
                           double* out_sse_cam, int* out_iters, double* out_trace, int device_id) {
    return solver_refine(kSolveRigJoint, problem, Pq_inout, SolverMask(fixed_mask), max_iters, lam_init, lam_min, lam_max,
                         err_min, out_sse, out_sse_cam, out_iters, out_trace, device_id);
}

// robust losses on the joint rig: the same three drivers with the loss in the run; no loss is the plain entry point
int calib_rig_robust_normal_eq(const calib_rig_problem_t* problem, const double* Pq, const calib_loss_t* loss, double* out_B,
                               double* out_E, double* out_V, double* out_g, double* out_cost_cam, int device_id) {
    if (loss_is_plain(loss)) return calib_rig_joint_normal_eq(problem, Pq, out_B, out_E, out_V, out_g, out_cost_cam, device_id);
    return solver_normal_eq(kSolveRigJoint, problem, Pq, out_B, out_E, out_V, out_g, out_cost_cam, device_id, loss);
}

int calib_rig_robust_step_delta(const calib_rig_problem_t* problem, const double* Pq, const uint64_t* fixed_mask,
                                const calib_loss_t* loss, double lambda, double* out_delta, int device_id) {
    if (loss_is_plain(loss)) return calib_rig_joint_step_delta(problem, Pq, fixed_mask, lambda, out_delta, device_id);
    return solver_step_delta(kSolveRigJoint, problem, Pq, SolverMask(fixed_mask), lambda, out_delta, device_id, loss);
}

int calib_refine_rig_robust(const calib_rig_problem_t* problem, double* Pq_inout, const uint64_t* fixed_mask,
                            const calib_loss_t* loss, int max_iters, double lam_init, double lam_min, double lam_max,
                            double err_min, double* out_cost, double* out_cost_cam, int* out_iters, double* out_trace,
                            int device_id) {
    if (loss_is_plain(loss))
        return calib_refine_rig_joint(problem, Pq_inout, fixed_mask, max_iters, lam_init, lam_min, lam_max, err_min, out_cost,
                                      out_cost_cam, out_iters, out_trace, device_id);
    return solver_refine(kSolveRigJoint, problem, Pq_inout, SolverMask(fixed_mask), max_iters, lam_init, lam_min, lam_max,
                         err_min, out_cost, out_cost_cam, out_iters, out_trace, device_id, loss);
}

int calib_rig_residuals(const calib_rig_problem_t* problem, const double* Pq, double* out_res, int device_id) {
    return solver_residuals(kSolveRigJoint, problem, Pq, out_res, device_id);
}

}  // extern "C"
