// pt_nn_tiles.h -- host only, no hip* call: the network denoiser's memory model and its tile plan (pt_nn.hip allocates and runs by
// them; the public side and the definition are include/mi355x_pathtracer.h, "network denoiser", Tiles).
//
// Memory model: the activations of one tile of tw x th pixels (padded to multiples of 16) with a plan's channel counts -- the network's
// input, the three pooled skips each in a place of their own, every other tensor in one of two arenas (pt_nn.h).  pt_nn_scratch is the
// one computation of it: the allocation and the tile rule both read it.
//
// Tile rule (OIDN's UNetFilter, restated): split the taller or wider side, one more tile at a time, until a tile's scratch fits the
// limit and the tile fits the one-tile cap, never below 3 x the overlap.  Tiles overlap by PTX_NN_TILE_OVERLAP = 96 pixels (half the
// receptive field of 174, rounded up to the alignment of 16), their origins are multiples of 16, and each keeps its interior.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <algorithm>

#include "../../include/mi355x_pathtracer.h"
#include "pt_tza.h"

// where each layer's output lives: 0 .. 2 = the skips pool1 .. pool3, 3 / 4 = the two arenas
constexpr int PT_NN_PLACE[PT_NN_LAYERS] = {3, 0, 1, 2, 3, 4, 3, 4, 3, 4, 3, 4, 3, 4, 3, 4};

struct PtNnScratch {
    size_t in_offset = 0, out_offset[PT_NN_LAYERS] = {};      // bytes into the scratch
    size_t total = 0;
    uint64_t macs = 0;                                        // of one run over the padded tile
};

inline int pt_nn_pad16(int c) { return (c + 15) / 16 * 16; }
inline size_t pt_nn_align256(size_t v) { return (v + 255) / 256 * 256; }

// multiply-adds of one run over a padded wp x hp tile
inline uint64_t pt_nn_macs(const PtNnPlan &plan, int wp, int hp) {
    uint64_t macs = 0;
    for (int i = 0; i < PT_NN_LAYERS; i++) {
        const PtNnLayer &P = plan.layers[i];
        macs += (uint64_t)(hp >> P.level) * (uint64_t)(wp >> P.level) * 9u * (uint64_t)(P.cin0 + P.cin1) * (uint64_t)P.cout;
    }
    return macs;
}

// The scratch of a tile of w x h pixels (any w, h >= 1; padded here)
inline PtNnScratch pt_nn_scratch(const PtNnPlan &plan, int w, int h) {
    PtNnScratch s;
    const int wp = pt_nn_pad16(w), hp = pt_nn_pad16(h);
    size_t skip[3] = {0, 0, 0}, arena[2] = {0, 0};
    for (int i = 0; i < PT_NN_LAYERS; i++) {
        const PtNnLayer &P = plan.layers[i];
        const size_t px = (size_t)(hp >> P.level) * (size_t)(wp >> P.level);
        const size_t bytes = i == PT_NN_LAYERS - 1 ? px * 4 * sizeof(float) : (P.pool ? px / 4 : px) * (size_t)pt_nn_pad16(P.cout) * 2;
        if (PT_NN_PLACE[i] < 3) skip[PT_NN_PLACE[i]] = pt_nn_align256(bytes);
        else arena[PT_NN_PLACE[i] - 3] = std::max(arena[PT_NN_PLACE[i] - 3], pt_nn_align256(bytes));
    }
    s.macs = pt_nn_macs(plan, wp, hp);
    size_t at = 0;
    s.in_offset = at; at += pt_nn_align256((size_t)hp * wp * 16 * 2);
    size_t skip_at[3], arena_at[2];
    for (int k = 0; k < 3; k++) { skip_at[k] = at; at += skip[k]; }
    for (int k = 0; k < 2; k++) { arena_at[k] = at; at += arena[k]; }
    for (int i = 0; i < PT_NN_LAYERS; i++) s.out_offset[i] = PT_NN_PLACE[i] < 3 ? skip_at[PT_NN_PLACE[i]] : arena_at[PT_NN_PLACE[i] - 3];
    s.total = at;
    return s;
}

// The plan of a W x H frame: tile_width x tile_height (multiples of 16) is the buffer every tile fits in
struct PtNnTiling {
    int width = 0, height = 0, tile_width = 0, tile_height = 0, tiles_x = 1, tiles_y = 1, max_memory_mb = 0;
    int count() const { return tiles_x * tiles_y; }
};

// One side of the rule's step: the tile size with `tiles` tiles along a side of `size` pixels
inline int pt_nn_tile_side(int size, int tiles) {
    const int inner = size - 2 * PTX_NN_TILE_OVERLAP;
    return std::max(pt_nn_pad16((inner + tiles - 1) / tiles) + 2 * PTX_NN_TILE_OVERLAP, PTX_NN_MIN_TILE);
}

// The rule.  The caller has checked 1 <= width, height <= PTX_NN_MAX_FRAME and max_memory_mb >= 0 (0: no memory limit).
inline PtNnTiling pt_nn_tiling(const PtNnPlan &plan, int width, int height, int max_memory_mb) {
    PtNnTiling t;
    t.width = width; t.height = height; t.max_memory_mb = max_memory_mb;
    const uint64_t limit = (uint64_t)max_memory_mb << 20;
    int ty = 1, tx = 1, th = pt_nn_pad16(height), tw = pt_nn_pad16(width);
    while (tw > PTX_NN_MAX_WIDTH || th > PTX_NN_MAX_HEIGHT || (max_memory_mb > 0 && (uint64_t)pt_nn_scratch(plan, tw, th).total > limit)) {
        if (th > PTX_NN_MIN_TILE && th > tw) th = pt_nn_tile_side(height, ++ty);
        else if (tw > PTX_NN_MIN_TILE) tw = pt_nn_tile_side(width, ++tx);
        else break;                                           // a minimum tile above the limit is accepted
    }
    const int O2 = 2 * PTX_NN_TILE_OVERLAP;
    t.tile_width = tw; t.tile_height = th;
    t.tiles_y = height > th ? (height - O2 + (th - O2) - 1) / (th - O2) : 1;
    t.tiles_x = width > tw ? (width - O2 + (tw - O2) - 1) / (tw - O2) : 1;
    return t;
}

// Tile k in execution order (row-major): the window read and the rectangle kept, in frame coordinates
inline ptx_nn_tile pt_nn_tile_at(const PtNnTiling &t, int k) {
    const int i = k / t.tiles_x, j = k - i * t.tiles_x, O = PTX_NN_TILE_OVERLAP;
    ptx_nn_tile r;
    r.y = i * (t.tile_height - 2 * O); r.h = std::min(t.height - r.y, t.tile_height);
    r.x = j * (t.tile_width - 2 * O); r.w = std::min(t.width - r.x, t.tile_width);
    const int top = i > 0 ? O : 0, bottom = i < t.tiles_y - 1 ? O : 0, left = j > 0 ? O : 0, right = j < t.tiles_x - 1 ? O : 0;
    r.out_x = r.x + left; r.out_w = r.w - left - right;
    r.out_y = r.y + top; r.out_h = r.h - top - bottom;
    return r;
}

// multiply-adds of one run: the sum over the tiles' padded windows
inline uint64_t pt_nn_tiling_macs(const PtNnPlan &plan, const PtNnTiling &t) {
    uint64_t macs = 0;
    for (int k = 0; k < t.count(); k++) {
        const ptx_nn_tile r = pt_nn_tile_at(t, k);
        macs += pt_nn_macs(plan, pt_nn_pad16(r.w), pt_nn_pad16(r.h));
    }
    return macs;
}
