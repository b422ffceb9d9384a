// Knobs and LaunchPlan: which compiled form of each LM-round kernel a shard runs, and on what grid (host code only;
// included by calib_lm.hip and by tests/host_cpp/launch_plan_check.cpp). makePlan is the one place that decides;
// the launches only switch on what it recorded.
#pragma once
#include "../../include/calib_lm.h"
#include "kernels.hpp"

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>

namespace calib {

// shards of at most this many views take the latency-oriented form of the update kernel (kernels.hpp)
constexpr int kUpdSmallViews = 4096;
// shards of at least this many views take the one-lane-per-view form (a wave per 64 views: it needs many to fill the chip).
// tools/sweep_upd_lane.sh, update kernel us, 16 lanes per view / one lane per view: 10 000 views 8.9 / 15.0 - 12 500 (fp32)
// 10.0 / 11.5 - 16 384: 11.2 / 12.4 - 32 768: 19.0 / 13.3 - 65 536: 29.7 / 17.6 - 125 000: 47.5 / 30.5
constexpr int kUpdLaneViews = 24576;
// shards above this many views load record heads in the coalesced, DPP-broadcast form (kernels.hpp: load_view_head).
// Round 4: since a record is six rows (768 B) the broadcast chain behind the loads is 48 DPP moves instead of 54, and on
// c4's 12 500-view shard the wide update kernel (122 VGPRs, no scratch) is as fast as the narrow one was WITH its 12-byte
// spill (10.1 vs 10.3 us; the narrow one without the spill, at three workgroups per CU: 12.3 us -- 782 workgroups on 768
// slots are two rounds). So every shard the small update kernel does not take (> 4 096 views) loads wide; the narrow
// schur form remains for the small shards and on request (CALIB_HEAD_LOADS=narrow).
constexpr int kWideHeadViews = 4096;

// The CALIB_* tuning variables, read once per engine (calib_create)
struct Knobs {
    int lm_mode = CALIB_LM_FUSED;          // CALIB_LM_MODE: the engine's first LM mode (non-zero: two-kernel)
    int head_loads = 0;                    // CALIB_HEAD_LOADS: schur record-head loads, 0 = by shard size, 1 = narrow, 2 = wide
    int items_per_wave = 0;                // CALIB_ITEMS_PER_WAVE: fused kernel, short uniform items; 0 = chosen per shard
    int upd_lane_views = kUpdLaneViews;    // CALIB_UPD_LANE_VIEWS: shards from this many views on take the lane update kernel
    int upd_small_views = kUpdSmallViews;  // CALIB_UPD_SMALL_VIEWS: shards up to this many views take the small update kernel
    int gram_form = 0;                     // CALIB_GRAM_FORM: fp64 fused kernel, 0 = chosen per shard, 1 = 16x16x4 tiles, 2 = 4x4x4 blocks
    int stream_mode = -1;                  // CALIB_FUSED_STREAM: -1 = chosen per shard, 0 = never, 1 = whenever the shard allows it
    int stream_waves = 0;                  // CALIB_STREAM_WAVES: > 0: waves of the stream launch; 0 = the chip's wave slots
    int gram_wpi = 0;                      // CALIB_GRAM_WPI: waves per item (1, 2, 4) of the gram and fused kernels; 0 = per shard
    int64_t chunk_points = (int64_t)1 << 26;   // CALIB_CHUNK_POINTS: points per chunk of the two-kernel mode
    bool timing = false;                   // CALIB_TIMING: stage times of calib_set_problem on stderr
};

inline Knobs readKnobs() {
    Knobs k;
    if (const char* e = std::getenv("CALIB_LM_MODE")) k.lm_mode = std::atoi(e) ? CALIB_LM_TWO_KERNEL : CALIB_LM_FUSED;
    if (const char* e = std::getenv("CALIB_HEAD_LOADS")) k.head_loads = std::strcmp(e, "narrow") == 0 ? 1 : (std::strcmp(e, "wide") == 0 ? 2 : 0);
    if (const char* e = std::getenv("CALIB_ITEMS_PER_WAVE")) k.items_per_wave = std::max(0, std::min(16, std::atoi(e)));
    if (const char* e = std::getenv("CALIB_UPD_LANE_VIEWS")) k.upd_lane_views = std::max(1, std::atoi(e));
    if (const char* e = std::getenv("CALIB_UPD_SMALL_VIEWS")) k.upd_small_views = std::max(0, std::atoi(e));
    if (const char* e = std::getenv("CALIB_GRAM_FORM")) k.gram_form = std::strcmp(e, "tile") == 0 ? 1 : (std::strcmp(e, "block") == 0 ? 2 : 0);
    if (const char* e = std::getenv("CALIB_FUSED_STREAM")) k.stream_mode = std::atoi(e) > 0 ? 1 : (std::atoi(e) == 0 ? 0 : -1);
    if (const char* e = std::getenv("CALIB_STREAM_WAVES")) k.stream_waves = std::max(0, std::atoi(e));
    if (const char* e = std::getenv("CALIB_GRAM_WPI")) {
        const int w = std::atoi(e);
        if (w == 1 || w == 2 || w == 4) k.gram_wpi = w;
    }
    if (const char* e = std::getenv("CALIB_CHUNK_POINTS")) k.chunk_points = std::max<int64_t>(1, std::atoll(e));
    k.timing = std::getenv("CALIB_TIMING") != nullptr;
    return k;
}

// what the form choices depend on: the shard's views (non-empty), work items and points; uniform_n > 0 when every
// item is one whole view of exactly that many points, in order
struct ShardShape {
    int nv = 0, n_items = 0, uniform_n = 0;
    int64_t MN = 0;
};

enum class FusedForm {
    TwoKernel,   // jacobian_kernel + gram_kernel per chunk (CALIB_LM_TWO_KERNEL)
    Tile,        // fused_kernel<.., G44 = false, MULTI = false>: J^T J from 16x16x4 tiles
    TileMulti,   // fused_kernel<.., false, true>: tiles, `ipw` short uniform items per wave
    Block44,     // fused_kernel<.., true, false>: fp64, J^T J from 4x4x4 blocks
    Stream,      // fused_stream_kernel: equal shares of 4-point groups per wave, view records + overflow records
};
enum class UpdateForm {
    Small,       // update_backsub_small_kernel: one trip, the solver wave beside the view waves
    Lane,        // update_backsub_lane_kernel: one lane per view
    Wide16,      // update_backsub_kernel: 16 lanes per view, grid-stride
};

struct LaunchPlan {
    FusedForm fused = FusedForm::Tile;
    int fused_wpi = 1;          // waves per item of the tile / block forms
    int ipw = 1;                // items per wave of the tile forms
    int fused_blocks = 0;       // workgroups of the fused launch (0: none -- two-kernel mode, or no items)
    int gram_wpi = 1;           // waves per gram item (two-kernel mode)
    int stream_share = 0;       // > 0 (Stream only): `stream_share` 4-point groups per wave
    int stream_waves = 0;       // Stream: waves that have work = overflow records behind the nv view records
    bool wide_heads = false;    // schur_kernel loads record heads coalesced + DPP (the narrow form: one load per value)
    UpdateForm update = UpdateForm::Small;
    int schur_blocks = 1;       // grid (schur_blocks, 3)
    int update_blocks = 1;
    bool stream() const { return stream_share > 0; }
};

inline LaunchPlan makePlan(const ShardShape& s, int dtype, int lm_mode, const Knobs& k, int num_cus) {
    LaunchPlan p;
    // waves per gram item from the mean points per item: a wave wants >= 2 trips of 16 points. The fused kernel: one
    // wave per item is fastest (measured c3: 84 us vs 102 us at 4) as long as there are enough items to fill the chip;
    // few big items are split over more waves
    const double avg = s.n_items ? (double)s.MN / s.n_items : 0.0;
    p.gram_wpi = avg >= 128 ? 4 : (avg >= 64 ? 2 : 1);
    p.fused_wpi = s.n_items >= 2048 ? 1 : p.gram_wpi;
    if (k.gram_wpi > 0) p.gram_wpi = p.fused_wpi = k.gram_wpi;

    // Stream form of the fused kernel (kernels.hpp: fused_stream_kernel): uniform fp64 shards whose views are whole
    // 4-point groups and at least one batch long. One wave per wave slot of the chip (4 per SIMD), every wave the
    // same share of groups; a share is at least two views, so a view is cut by at most one wave start. By default
    // only where a wave gets two views or more anyway (below that, a view per wave fills the chip better).
    const int un = s.uniform_n;
    const bool can = dtype == CALIB_DTYPE_F64 && un >= 64 && (un & 3) == 0 && s.MN < ((int64_t)1 << 31) && s.nv >= 1;
    if (lm_mode == CALIB_LM_FUSED && can && k.stream_mode != 0) {
        const int slots = k.stream_waves > 0 ? k.stream_waves : kFusedWaves * kStreamMinBlocks * num_cus;
        const int waves = std::max(1, std::min(slots, s.nv));
        if (k.stream_mode == 1 || s.nv >= 2 * slots) {
            const int64_t groups = (int64_t)s.nv * (un / 4);
            p.stream_share = (int)((groups + waves - 1) / waves);
            p.stream_waves = (int)((groups + p.stream_share - 1) / p.stream_share);
        }
    }

    if (p.stream()) {
        p.fused = FusedForm::Stream;
        p.fused_blocks = (p.stream_waves + 3) / 4;
    } else if (lm_mode == CALIB_LM_TWO_KERNEL) {
        p.fused = FusedForm::TwoKernel;
    } else {
        // ROWS = 32, 4 waves per workgroup: the 64-row / 2-wave variants measured 1-6 % slower (c3, c5, c2).
        // fp64 items of more than two batches build J^T J from 4x4 blocks (v_mfma_f64_4x4x4_4b, symmetric half only;
        // c3 -4.5 %); shorter items stay on the 16x16x4 form, whose record goes to HBM straight from the accumulators
        // (one-batch items: c2 +4 % on the block form; two batches, c5: no difference)
        p.fused_wpi = std::min(p.fused_wpi, 4);
        const bool g44 = dtype == CALIB_DTYPE_F64 && (k.gram_form == 2 || (k.gram_form == 0 && s.MN > (int64_t)128 * s.n_items));
        // short uniform items (tile forms, one wave each): on shards large enough to leave every workgroup slot of the
        // chip (4 per CU) four workgroups even so, a wave takes up to four items in a row -- one prologue, one partial,
        // one barrier, the next item's points requested early (c5 shard -7 %; c4's 12 500 items: no gain, c2: slower)
        if (!g44 && p.fused_wpi == 1 && un > 0) {
            if (k.items_per_wave > 0) p.ipw = k.items_per_wave;
            else while (p.ipw < 4 && s.n_items / (8 * p.ipw) >= 16 * num_cus) p.ipw *= 2;
        }
        p.fused = g44 ? FusedForm::Block44 : (p.ipw > 1 ? FusedForm::TileMulti : FusedForm::Tile);
        const int ipb = (4 / p.fused_wpi) * p.ipw;
        p.fused_blocks = (s.n_items + ipb - 1) / ipb;
    }

    // Larger shards, and shards whose views can be two records (stream form: the second record doubles the 27 per-value
    // loads of the narrow form; c3 schur +2.1 us, update +3 us -- six coalesced rows per record cost nothing extra)
    p.wide_heads = k.head_loads == 2 || (k.head_loads == 0 && (s.nv > kWideHeadViews || p.stream()));
    p.schur_blocks = std::max(1, std::min(kMaxSchurBlocks, (s.nv + kSchurViewsPerBlock - 1) / kSchurViewsPerBlock));

    if (s.nv <= k.upd_small_views) {
        p.update = UpdateForm::Small;
        p.update_blocks = std::max(1, (s.nv + kUpdViewsPerBlock - 1) / kUpdViewsPerBlock);      // one view per 16-lane group
    } else if (s.nv >= k.upd_lane_views && k.head_loads == 0) {
        p.update = UpdateForm::Lane;
        p.update_blocks = std::max(1, std::min(12 * num_cus, (s.nv + kSchurThreads - 1) / kSchurThreads));
    } else {
        p.update = UpdateForm::Wide16;
        const int per = kSchurThreads / 16;
        p.update_blocks = std::max(1, std::min(2048, (s.nv + per - 1) / per));                  // grid-stride over views
    }
    return p;
}

}  // namespace calib
