// ShardLayout: the O(views) host arithmetic of calib_set_problem (host code only; included by calib_lm.hip and by
// tests/host_cpp/shard_layout_check.cpp). From the caller's view offsets: the compact list of non-empty views, the
// gram / fused work items, the chunks of the two-kernel rounds, and what the kernels' tables and LDS sizes follow from.
// Everything O(points) happens on the device (pack_points_kernel).
#pragma once
#include "kernels.hpp"

#include <algorithm>
#include <cstdint>
#include <vector>

namespace calib {

// Two-kernel LM rounds walk the points in chunks of whole views, so that a chunk's compact J (written by the jacobian
// kernel, read once by the gram kernel) is bounded: points [p0, p1), items [item0, item1). A chunk's 256-point
// jacobian tiles start at p0.
// Measured on MI355X (c3, 2 M points): chunks small enough for the 256 MiB Infinity Cache do NOT make the J round
// trip cheaper (0.33 ms/iter at one chunk, 0.45 at 262 k points, 1.1 at 65 k), so the chunk only bounds the J buffer:
// 64 M points = 17 GB at C = 16, fp64.
struct ShardChunk { int64_t p0, p1; int item0, item1; };

struct ShardLayout {
    int nv = 0, n_items = 0;            // non-empty views, work items
    std::vector<int> view_ext;          // [nv] the caller's index of each non-empty view
    std::vector<int64_t> voffs;         // [nv + 1] first point of each non-empty view (their points are contiguous), then MN
    std::vector<int64_t> item_pt0;      // [n_items] work items: at most kGramChunk points of one view each, in point order
    std::vector<int> item_n, item_view; // [n_items] an item's points and its (compact) view
    std::vector<int> view_item0;        // [nv + 1] first item of each view
    std::vector<ShardChunk> chunks;     // whole views, closed once they hold chunk_points points
    int64_t max_chunk_points = 0;
    int64_t n_tiles = 0;                // kTile-point tiles of [0, MN)
    int max_views_per_tile = 1;         // most views one tile touches (what jacobian_kernel stages in LDS), over the tiles
                                        // of [0, MN) and, with several chunks, the tiles of each chunk
    int uniform_n = 0;                  // > 0: item i is the whole view i, points [i n, (i + 1) n), for every i
};

// view_offsets: num_views + 1 non-decreasing offsets from 0 (the caller has checked them)
inline ShardLayout makeShardLayout(int64_t num_views, const int64_t* view_offsets, int64_t chunk_points) {
    ShardLayout s;
    const int64_t MN = view_offsets[num_views];
    s.view_item0.push_back(0);
    for (int64_t i = 0; i < num_views; ++i) {
        const int64_t a = view_offsets[i], b = view_offsets[i + 1];
        if (b == a) continue;
        const int cv = (int)s.view_ext.size();
        s.view_ext.push_back((int)i);
        s.voffs.push_back(a);
        for (int64_t p = a; p < b; p += kGramChunk) {
            s.item_pt0.push_back(p);
            s.item_n.push_back((int)std::min<int64_t>(kGramChunk, b - p));
            s.item_view.push_back(cv);
        }
        s.view_item0.push_back((int)s.item_pt0.size());
    }
    s.voffs.push_back(MN);
    s.nv = (int)s.view_ext.size();
    s.n_items = (int)s.item_pt0.size();

    // uniform shards (every view fully detected: the usual case) need no item tables in the fused kernel
    s.uniform_n = s.n_items ? s.item_n[0] : 0;
    for (int i = 0; i < s.n_items && s.uniform_n > 0; ++i)
        if (s.item_n[(size_t)i] != s.uniform_n || s.item_pt0[(size_t)i] != (int64_t)i * s.uniform_n || s.item_view[(size_t)i] != i)
            s.uniform_n = 0;

    // most views one tile of [p0, p1) touches; the tiles start at p0, a point of view `va`: one sweep over the offsets
    auto tileSpan = [&s](int64_t p0, int64_t p1, int va) {
        int span = 1, vb = va;
        for (int64_t a = p0; a < p1; a += kTile) {
            const int64_t b = std::min<int64_t>(p1, a + kTile) - 1;
            while (s.voffs[(size_t)va + 1] <= a) ++va;      // the view of the tile's first point
            while (s.voffs[(size_t)vb + 1] <= b) ++vb;      // ... and of its last one
            span = std::max(span, vb - va + 1);
        }
        return span;
    };
    s.n_tiles = (MN + kTile - 1) / kTile;
    s.max_views_per_tile = tileSpan(0, MN, 0);        // calib_eval's one launch over all points

    for (int v = 0; v < s.nv;) {
        const int v0 = v;
        ShardChunk c;
        c.p0 = c.p1 = s.voffs[(size_t)v];
        while (v < s.nv && c.p1 - c.p0 < chunk_points) c.p1 = s.voffs[(size_t)++v];
        c.item0 = s.view_item0[(size_t)v0];
        c.item1 = s.view_item0[(size_t)v];
        s.chunks.push_back(c);
        s.max_chunk_points = std::max(s.max_chunk_points, c.p1 - c.p0);
        if (v0 > 0 || v < s.nv)                       // a single chunk has the tiles counted above
            s.max_views_per_tile = std::max(s.max_views_per_tile, tileSpan(c.p0, c.p1, v0));
    }
    return s;
}

}  // namespace calib
