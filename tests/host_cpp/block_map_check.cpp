// Host-side check of the block maps of the four solvers on the shared LM loop (csrc/block_map.hpp) and of unpack_blocks:
// totals and view records whose every value names its own slot are unpacked and compared, entry by entry, with a
// restatement written from the record tables of DESIGN.md (sections 11, 13, 15 and 17) that calls none of the fill
// functions. Compiled and run by tests/test_block_map.py with hipcc; only host code runs.
#include "../../camera-calibration_amd/csrc/block_map.hpp"
#include <cmath>
#include <cstdio>
#include <string>

using namespace calib;

namespace {

int cases = 0, bad = 0;

#define EXPECT(cond)                                                                                                 \
    do {                                                                                                             \
        if (!(cond)) { if (bad++ < 20) std::printf("case %d (%s): %s fails\n", cases, name.c_str(), #cond); return; } \
    } while (0)

// What the tables say, in the tables' own terms: B's diagonal blocks, where g_shared and the errors are, the record.
struct Block { int first, width, slot; };       // unknowns [first, first + width): lower triangle, row by row, from `slot`
struct Stated {
    int S, ncam;
    std::vector<Block> blocks;
    std::vector<int> g;         // slot of g_shared[s]
    int err, ntot;              // slot of camera 0's error; number of totals
    int gv, stride;             // view record: V [0, 21) | E [21, 21 + 6 S) | .. | g_view [gv, gv + 6); doubles per record
};

int roundUp8(int n) { return (n + 7) / 8 * 8; }

// section 11: totals B (21), g_rig (6), sse_a, sse_b; a record of 96 doubles: V | E | B_i [57, 78) | g_rig [78, 84) |
// g_view [84, 90) | the two errors
Stated statedStereo() {
    Stated t{6, 2, {{0, 6, 0}}, {}, 27, 29, 84, 96};
    for (int s = 0; s < 6; ++s) t.g.push_back(21 + s);
    return t;
}

// section 13: unknowns (a | b | rig); totals B_aa, B over (b, rig), g_shared (S), sse_a, sse_b; records 184 doubles apart
Stated statedJoint(int LA, int LB) {
    const int S = LA + LB + 6, LR = LB + 6, baa = LA * (LA + 1) / 2, g0 = baa + LR * (LR + 1) / 2;
    Stated t{S, 2, {{0, LA, 0}, {LA, LR, baa}}, {}, g0 + S, g0 + S + 2, 21 + 6 * S, 184};
    for (int s = 0; s < S; ++s) t.g.push_back(g0 + s);
    return t;
}

// section 15: per camera c >= 1 B_c (21) and g_c (6) at 27 (c - 1), then the N errors; stride a multiple of 8
Stated statedRig(int N) {
    const int S = 6 * (N - 1);
    Stated t{S, N, {}, {}, 27 * (N - 1), 27 * (N - 1) + N, 21 + 6 * S, roundUp8(27 + 6 * S)};
    for (int c = 1; c < N; ++c) {
        t.blocks.push_back({6 * (c - 1), 6, 27 * (c - 1)});
        for (int k = 0; k < 6; ++k) t.g.push_back(27 * (c - 1) + 21 + k);
    }
    return t;
}

// section 17: camera-major unknowns (shared_0 | shared_1, rig_1 | ..); totals: the blocks' lower triangles | g (S) | errors
Stated statedRigJoint(const std::vector<int>& L) {
    const int N = (int)L.size();
    Stated t{0, N, {}, {}, 0, 0, 0, 0};
    int slot = 0;
    for (int c = 0; c < N; ++c) {
        const int w = L[(size_t)c] + (c ? 6 : 0);
        t.blocks.push_back({t.S, w, slot});
        t.S += w;
        slot += w * (w + 1) / 2;
    }
    for (int s = 0; s < t.S; ++s) t.g.push_back(slot + s);
    t.err = slot + t.S;
    t.ntot = t.err + N;
    t.gv = 21 + 6 * t.S;
    t.stride = roundUp8(27 + 6 * t.S);
    return t;
}

double totValue(int slot) { return 1000.0 + slot; }
double recValue(int view, int at) { return 1e6 * (view + 1) + at; }

void check(const std::string& name, const BlockMap& m, const Stated& t) {
    ++cases;
    const int M = 3;
    const size_t S = (size_t)t.S;
    EXPECT(m.S == t.S && m.ncam == t.ncam && m.stride == t.stride);
    EXPECT(m.slotB.size() == S * (S + 1) / 2 && m.slotG.size() == S);
    std::vector<double> tot((size_t)t.ntot), rec((size_t)M * (size_t)t.stride);
    for (size_t i = 0; i < tot.size(); ++i) tot[i] = totValue((int)i);
    for (int v = 0; v < M; ++v)
        for (int j = 0; j < t.stride; ++j) rec[(size_t)v * (size_t)t.stride + (size_t)j] = recValue(v, j);
    const double nan = std::nan("");
    std::vector<double> B(S * S, nan), E((size_t)M * S * 6, nan), V((size_t)M * 36, nan), g(S + 6 * (size_t)M, nan),
        sse((size_t)t.ncam, nan);
    unpack_blocks(m, M, tot.data(), rec.data(), B.data(), E.data(), V.data(), g.data(), sse.data());

    // B: the stated blocks, an exact +0 everywhere else, symmetric
    std::vector<double> wantB(S * S, 0.0);
    for (const Block& b : t.blocks)
        for (int i = 0; i < b.width; ++i)
            for (int j = 0; j <= i; ++j) {
                const double x = totValue(b.slot + i * (i + 1) / 2 + j);
                wantB[(size_t)(b.first + i) * S + (size_t)(b.first + j)] = wantB[(size_t)(b.first + j) * S + (size_t)(b.first + i)] = x;
            }
    for (size_t r = 0; r < S; ++r)
        for (size_t c = 0; c < S; ++c) {
            EXPECT(B[r * S + c] == wantB[r * S + c] && !std::signbit(B[r * S + c]));
            EXPECT(B[r * S + c] == B[c * S + r]);
        }
    for (size_t s = 0; s < S; ++s) EXPECT(g[s] == totValue(t.g[s]));
    for (int c = 0; c < t.ncam; ++c) EXPECT(sse[(size_t)c] == totValue(t.err + c));
    for (int v = 0; v < M; ++v) {
        for (int a = 0; a < 6; ++a)
            for (int b = 0; b < 6; ++b) {
                const int hi = a > b ? a : b, lo = a > b ? b : a;
                EXPECT(V[(size_t)v * 36 + (size_t)a * 6 + (size_t)b] == recValue(v, hi * (hi + 1) / 2 + lo));
            }
        for (size_t s = 0; s < S; ++s)
            for (size_t k = 0; k < 6; ++k) EXPECT(E[((size_t)v * S + s) * 6 + k] == recValue(v, 21 + (int)(6 * s + k)));
        for (size_t k = 0; k < 6; ++k) EXPECT(g[S + 6 * (size_t)v + k] == recValue(v, t.gv + (int)k));
    }

    // null outputs are skipped
    unpack_blocks(m, M, tot.data(), rec.data(), nullptr, nullptr, nullptr, nullptr, nullptr);
}

template <int LA, int LB>
void checkJoint() {
    check("joint " + std::to_string(LA) + " " + std::to_string(LB), joint_block_map<LA, LB>(), statedJoint(LA, LB));
}

void checkRigJoint(const std::vector<int>& model) {
    std::string name = "rig joint";
    std::vector<int> L;
    for (int m : model) {
        L.push_back(m == kRadtan ? 10 : 9);         // shared parameters of a radtan / a fisheye camera
        name += m == kRadtan ? " r" : " f";
    }
    const RigJointDesc y = rig_joint_desc(model.data(), (int)model.size());
    const Stated t = statedRigJoint(L);
    check(name, rig_joint_block_map(y), t);
    if (y.S != t.S || y.kTot != t.ntot || y.kStride != t.stride || y.kStride > 760) {
        if (bad++ < 20) std::printf("%s: RigJointDesc S %d kTot %d kStride %d\n", name.c_str(), y.S, y.kTot, y.kStride);
    }
}

}  // namespace

int main() {
    check("stereo", stereo_block_map(), statedStereo());
    checkJoint<10, 10>();
    checkJoint<10, 9>();
    checkJoint<9, 10>();
    checkJoint<9, 9>();
    check("rig 2", rig_block_map<2>(), statedRig(2));
    check("rig 3", rig_block_map<3>(), statedRig(3));
    check("rig 8", rig_block_map<8>(), statedRig(8));
    if (statedRig(2).stride != 64 || statedRig(8).stride != 280 || statedRig(8).ntot != 197) { ++bad; std::printf("rig: the documented sizes\n"); }
    const int r = kRadtan, f = kFisheye;
    for (int a : {r, f})
        for (int b : {r, f}) {
            checkRigJoint({a, b});
            for (int c : {r, f}) checkRigJoint({a, b, c});
        }
    checkRigJoint({r, r, r, r, r, r, r, r});
    checkRigJoint({f, f, f, f, f, f, f, f});
    checkRigJoint({r, f, f, r, r, f, r, f});
    checkRigJoint({f, r, f, r, f, r, f, r});
    if (statedRigJoint({10, 10, 10, 10, 10, 10, 10, 10}).S != 122) { ++bad; std::printf("eight radtan cameras: S\n"); }
    std::printf("%d cases, %d mismatches\n", cases, bad);
    std::printf(bad ? "FAILED\n" : "ok\n");
    return bad ? 1 : 0;
}
