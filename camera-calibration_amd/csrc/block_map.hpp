// Where the block-arrow normal equations of a solver on the LM loop of stereo_loop.hpp live on the device, and their way
// into the caller's arrays (host code, no HIP call; tests/host_cpp/block_map_check.cpp runs it against a restatement).
//
// A blocks kernel leaves two things: the totals, summed over the views (the entries of B that some row touches, g_shared,
// one error per camera), and one record per view (V's lower triangle, E row-major as (shared row, view column), g_view).
// The four layouts -- kSt* (stereo.hpp), JointLayout (stereo_joint.hpp), RigLayout (rig.hpp), RigJointDesc (rig_joint.hpp)
// -- differ only in where a slot is; each fills one BlockMap, and unpack_blocks reads them all.
#pragma once
#include "rig_joint.hpp"

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace calib {

struct BlockMap {
    int S = 0, ncam = 0;
    std::vector<int> slotB;     // B(r, c), c <= r, at r (r + 1) / 2 + c: its slot in the totals; -1: no row touches it
    std::vector<int> slotG;     // g_shared[s]: its slot in the totals
    int err = 0;                // slot of camera 0's error, the other cameras' follow
    int kV = 0, kE = 0, kGv = 0, stride = 0;    // the view record: offsets of V (21), E (6 S), g_view (6); doubles per view
};

// slotB(r, c) and slotG(s) as the layout states them
template <typename SlotB, typename SlotG>
BlockMap make_block_map(int S, int ncam, int err, int kV, int kE, int kGv, int stride, SlotB slotB, SlotG slotG) {
    BlockMap m;
    m.S = S; m.ncam = ncam; m.err = err; m.kV = kV; m.kE = kE; m.kGv = kGv; m.stride = stride;
    m.slotB.reserve((size_t)S * (S + 1) / 2);
    for (int r = 0; r < S; ++r)
        for (int c = 0; c <= r; ++c) m.slotB.push_back(slotB(r, c));
    for (int s = 0; s < S; ++s) m.slotG.push_back(slotG(s));
    return m;
}

// the rig between two known cameras: the totals are the record's [kStB, kStAcc) without g_view
inline BlockMap stereo_block_map() {
    return make_block_map(6, 2, kStTot - 2, kStV, kStE, kStGv, kStRecord, [](int r, int c) { return r * (r + 1) / 2 + c; },
                          [](int s) { return kStGr - kStB + s; });
}

template <int LA, int LB>
BlockMap joint_block_map() {
    using Y = JointLayout<LA, LB>;
    return make_block_map(Y::S, 2, Y::kErr, Y::kV, Y::kE, Y::kGv, Y::kStride, [](int r, int c) { return Y::slotB(r, c); },
                          [](int s) { return Y::kG + s; });
}

template <int NC>
BlockMap rig_block_map() {
    using Y = RigLayout<NC>;
    return make_block_map(Y::S, NC, Y::kErr, Y::kV, Y::kE, Y::kGv, Y::kStride, [](int r, int c) { return Y::slotB(r, c); },
                          [](int s) { return Y::kCam * (s / 6) + 21 + s % 6; });
}

// S, the per-camera offsets, the slots of the totals and the record stride of a joint rig call
inline RigJointDesc rig_joint_desc(const int* model, int num_cameras) {
    RigJointDesc y{};
    y.nc = num_cameras;
    int s = 0, b = 0;
    for (int c = 0; c < y.nc; ++c) {
        y.model[c] = model[c];
        y.L[c] = model[c] == kRadtan ? ModelTraits<kRadtan>::L : ModelTraits<kFisheye>::L;
        y.off[c] = s;
        y.bo[c] = b;
        const int w = y.width(c);
        s += w;
        b += w * (w + 1) / 2;
    }
    y.S = s;
    y.kG = b; y.kErr = b + s; y.kTot = y.kErr + y.nc;
    y.kGv = kRjE0 + 6 * s; y.kRec = y.kGv + 6; y.kStride = (y.kRec + 7) / 8 * 8;
    y.kEg = s * (s + 1) / 2; y.kFail = y.kEg + s; y.kSchur = y.kFail + 1;
    return y;
}

inline BlockMap rig_joint_block_map(const RigJointDesc& y) {
    int cam[kRjMaxS];           // the camera of every shared unknown
    for (int c = 0; c < y.nc; ++c) std::fill(cam + y.off[c], cam + y.off[c] + y.width(c), c);
    return make_block_map(y.S, y.nc, y.kErr, 0, kRjE0, y.kGv, y.kStride,
                          [&](int r, int c) {
                              const int q = cam[r], i = r - y.off[q], j = c - y.off[q];
                              return cam[c] == q ? y.bo[q] + i * (i + 1) / 2 + j : -1;
                          },
                          [&](int s) { return y.kG + s; });
}

// a 6 x 6 lower triangle stored row by row -> the full symmetric matrix
inline void sym6(const double* t, double* o) {
    for (int r = 0; r < 6; ++r)
        for (int c = 0; c <= r; ++c) o[r * 6 + c] = o[c * 6 + r] = t[r * (r + 1) / 2 + c];
}

// (totals, M records) -> B (S, S) dense and symmetric, exact zeros where no slot exists; E (M, S, 6); V (M, 6, 6);
// g (S + 6 M); one error per camera. Every output may be null.
inline void unpack_blocks(const BlockMap& m, int64_t M, const double* tot, const double* rec, double* out_B, double* out_E,
                          double* out_V, double* out_g, double* out_sse_cam) {
    const size_t S = (size_t)m.S;
    if (out_B)
        for (size_t r = 0, e = 0; r < S; ++r)
            for (size_t c = 0; c <= r; ++c, ++e) out_B[r * S + c] = out_B[c * S + r] = m.slotB[e] >= 0 ? tot[m.slotB[e]] : 0.0;
    if (out_g)
        for (size_t s = 0; s < S; ++s) out_g[s] = tot[m.slotG[s]];
    if (out_sse_cam) std::copy(tot + m.err, tot + m.err + m.ncam, out_sse_cam);
    for (size_t v = 0; v < (size_t)M; ++v) {
        const double* r = rec + v * (size_t)m.stride;
        if (out_V) sym6(r + m.kV, out_V + v * 36);
        if (out_E) std::copy(r + m.kE, r + m.kE + 6 * S, out_E + v * 6 * S);
        if (out_g) std::copy(r + m.kGv, r + m.kGv + 6, out_g + S + v * 6);
    }
}

}  // namespace calib
