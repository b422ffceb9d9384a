// Host-side check of makeShardLayout (csrc/shard_layout.hpp) against a brute-force restatement of every field: a
// per-point view index, items and chunks rebuilt point by point, and for the tile span a count of the distinct views
// in every tile of every chunk. Compiled and run by tests/test_shard_layout.py with hipcc; only host code runs.
#include "../../camera-calibration_amd/csrc/shard_layout.hpp"
#include <cstdio>
#include <random>
#include <set>

using namespace calib;

namespace {

int cases = 0, bad = 0;

#define EXPECT(cond)                                                                                       \
    do {                                                                                                   \
        if (!(cond)) { if (bad++ < 20) std::printf("case %d (%s): %s fails\n", cases, name, #cond); return; } \
    } while (0)

// distinct views among the points [a, b)
int viewsIn(const std::vector<int>& pv, int64_t a, int64_t b) {
    return (int)std::set<int>(pv.begin() + a, pv.begin() + b).size();
}

void check(const char* name, const std::vector<int64_t>& sizes, int64_t chunk_points) {
    ++cases;
    const int64_t M = (int64_t)sizes.size();
    std::vector<int64_t> offs(1, 0);
    for (int64_t n : sizes) offs.push_back(offs.back() + n);
    const int64_t MN = offs.back();
    const ShardLayout s = makeShardLayout(M, offs.data(), chunk_points);

    // compact views and the view of every point
    std::vector<int> ext, pv;
    std::vector<int64_t> first;
    for (int64_t i = 0; i < M; ++i) {
        if (sizes[(size_t)i] == 0) continue;
        first.push_back(offs[(size_t)i]);
        pv.insert(pv.end(), (size_t)sizes[(size_t)i], (int)ext.size());
        ext.push_back((int)i);
    }
    first.push_back(MN);
    EXPECT((int64_t)pv.size() == MN);
    EXPECT(s.nv == (int)ext.size() && s.view_ext == ext && s.voffs == first);

    // items, point by point: a new one at a view's first point and after every kGramChunk points of a view
    std::vector<int64_t> pt0;
    std::vector<int> n, view, item0((size_t)s.nv + 1, 0);
    for (int64_t p = 0; p < MN; ++p) {
        const int v = pv[(size_t)p];
        if ((p - first[(size_t)v]) % kGramChunk == 0) { pt0.push_back(p); n.push_back(0); view.push_back(v); }
        ++n.back();
    }
    for (int v : view) for (int w = v + 1; w <= s.nv; ++w) ++item0[(size_t)w];      // items of the views before w
    EXPECT(s.n_items == (int)pt0.size() && s.item_pt0 == pt0 && s.item_n == n && s.item_view == view);
    EXPECT(s.view_item0 == item0);

    // uniform: every non-empty view has the same number of points, at most one item's worth
    int un = s.nv ? (int)(first[1] - first[0]) : 0;
    for (int v = 0; v < s.nv; ++v)
        if (first[(size_t)v + 1] - first[(size_t)v] != un || un > kGramChunk) un = 0;
    EXPECT(s.uniform_n == un);
    if (un > 0) for (int i = 0; i < s.n_items; ++i) EXPECT(pt0[(size_t)i] == (int64_t)i * un && view[(size_t)i] == i);

    // chunks: whole views, back to back over [0, MN); closed by the view that brings them to chunk_points
    int64_t at = 0, longest = 0;
    for (size_t c = 0; c < s.chunks.size(); ++c) {
        const ShardChunk& k = s.chunks[c];
        EXPECT(k.p0 == at && k.p1 > k.p0 && k.p1 <= MN);
        EXPECT(pv[(size_t)k.p0] != (k.p0 ? pv[(size_t)k.p0 - 1] : -1));                      // starts a view
        EXPECT(k.p1 == MN || pv[(size_t)k.p1] != pv[(size_t)k.p1 - 1]);                       // ends one
        const int64_t lastView = first[(size_t)pv[(size_t)k.p1 - 1]];
        EXPECT(lastView - k.p0 < chunk_points);                                              // open before its last view
        EXPECT(k.p1 - k.p0 >= chunk_points || c + 1 == s.chunks.size());
        int i0 = 0, i1 = 0;
        for (int64_t q : pt0) { i0 += q < k.p0; i1 += q < k.p1; }
        EXPECT(k.item0 == i0 && k.item1 == i1);
        at = k.p1;
        longest = std::max(longest, k.p1 - k.p0);
    }
    EXPECT(at == MN && s.max_chunk_points == longest && (MN > 0) == !s.chunks.empty());

    // tiles: kTile points from 0 (one evaluation over all points) and, with several chunks, from each chunk's start
    EXPECT(s.n_tiles == (MN + kTile - 1) / kTile);
    int span = 1;
    for (int64_t a = 0; a < MN; a += kTile) span = std::max(span, viewsIn(pv, a, std::min<int64_t>(MN, a + kTile)));
    if (s.chunks.size() > 1)
        for (const ShardChunk& k : s.chunks)
            for (int64_t a = k.p0; a < k.p1; a += kTile) span = std::max(span, viewsIn(pv, a, std::min<int64_t>(k.p1, a + kTile)));
    EXPECT(s.max_views_per_tile == span);
}

}  // namespace

int main() {
    const std::vector<int64_t> ones(300, 1);
    std::vector<int64_t> onesThenBig(ones);
    onesThenBig.push_back(700);
    const struct { const char* name; std::vector<int64_t> sizes; } fixed[] = {
        {"no views", {}},
        {"all views empty", {0, 0, 0}},
        {"empty views between non-empty ones", {0, 5, 0, 0, 300, 0, 17, 0}},
        {"a view of exactly 512 points", {3, 512, 4}},
        {"a view of 513 points", {3, 513, 4}},
        {"a view of 1024 points", {1024}},
        {"views of 6, 513, 7, 1024, 257, 9 points", {6, 513, 7, 1024, 257, 9}},
        {"300 views of one point", ones},
        {"300 views of one point and a big one", onesThenBig},
        {"uniform views", {54, 54, 54, 54, 54, 54, 54, 54, 54, 54, 54, 54}},
        {"uniform views, one shortened", {54, 54, 54, 54, 54, 53, 54, 54, 54, 54, 54, 54}},
        {"uniform views with empty ones among them", {88, 0, 88, 88, 0, 88}},
        {"uniform views of one item's worth", {512, 512, 512}},
        {"equal views of two items", {600, 600, 600}},
    };
    for (const auto& f : fixed)
        for (int64_t chunk_points : {(int64_t)1, (int64_t)300, (int64_t)1 << 26}) check(f.name, f.sizes, chunk_points);

    std::mt19937_64 rng(20240611);
    const int64_t chunkChoices[] = {1, 2, 100, 255, 256, 257, 300, 513, 2000, 10000, (int64_t)1 << 26};
    for (int rep = 0; rep < 400; ++rep) {
        const int M = (int)(rng() % 41);
        const int kind = (int)(rng() % 4);                  // mostly small / mixed / large views / many empty
        std::vector<int64_t> sizes((size_t)M);
        for (auto& n : sizes) {
            const uint64_t r = rng();
            n = kind == 0 ? (int64_t)(r % 8) : kind == 1 ? (int64_t)(r % 1501) : kind == 2 ? 200 + (int64_t)(r % 1301)
                                                                                            : ((r >> 20) % 3 ? 0 : (int64_t)(r % 600));
        }
        check("random", sizes, chunkChoices[rng() % (sizeof(chunkChoices) / sizeof(chunkChoices[0]))]);
    }
    std::printf("%d cases, %d mismatches\n%s\n", cases, bad, bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
