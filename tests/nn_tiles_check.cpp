// nn_tiles_check.cpp -- csrc/pt_nn_tiles.h, the network denoiser's tile plan, as a stand-alone program for AddressSanitizer and
// UndefinedBehaviorSanitizer (tests/test_nn_tiles_cpu.py compiles and runs it; host only, no device).  Two plans are filled in code (the
// standard channel table with 9 inputs, and one channel everywhere); the tile rule runs over every W, H of 1, 8, 15 .. 700 (step 7: every
// residue mod 16) with both sides of 288 added, and over the large sizes up to 16384, each with the limits 0, 1, 2, 4 .. MiB up to the
// first that gives one tile.  Checked per plan, in C++: the kept rectangles cover the frame exactly once; every window lies inside the
// frame, begins at a multiple of 16 and fits the tile buffer; the buffer is at most 7680 x 4320; a kept pixel is at least 96 pixels from
// every window edge that is not a frame edge; one tile, or both tile dimensions at least 288; a tile's scratch is within the buffer's;
// limit 0 within the cap is one tile; the limit is kept unless the tile is at its minimum; the summed macs.
#include <stdint.h>
#include <stdio.h>
#include <vector>

#include "pt_nn_tiles.h"

static long failures = 0, plans = 0;
#define CHECK(cond, what) do { if (!(cond)) { if (failures++ < 40) printf("FAIL %s (line %d): %d x %d limit %d\n", what, __LINE__, W, H, mb); } } while (0)

static PtNnPlan make_plan(int ic, const int *c) {      // c: e1 e2 e3 e4 e5 d4 d3 d2 d1a d1b
    static const struct { const char *name; int level; bool pool, up; int s0, s1; } G[PT_NN_LAYERS] = {
        {"enc_conv0", 0, false, false, -1, -2}, {"enc_conv1", 0, true, false, 0, -2},  {"enc_conv2", 1, true, false, 1, -2},
        {"enc_conv3", 2, true, false, 2, -2},   {"enc_conv4", 3, true, false, 3, -2},  {"enc_conv5a", 4, false, false, 4, -2},
        {"enc_conv5b", 4, false, false, 5, -2}, {"dec_conv4a", 3, false, true, 6, 3},  {"dec_conv4b", 3, false, false, 7, -2},
        {"dec_conv3a", 2, false, true, 8, 2},   {"dec_conv3b", 2, false, false, 9, -2}, {"dec_conv2a", 1, false, true, 10, 1},
        {"dec_conv2b", 1, false, false, 11, -2}, {"dec_conv1a", 0, false, true, 12, -1}, {"dec_conv1b", 0, false, false, 13, -2},
        {"dec_conv0", 0, false, false, 14, -2}};
    const int cout[PT_NN_LAYERS] = {c[0], c[0], c[1], c[2], c[3], c[4], c[4], c[5], c[5], c[6], c[6], c[7], c[7], c[8], c[9], 3};
    PtNnPlan p;
    p.ic = ic;
    for (int i = 0; i < PT_NN_LAYERS; i++) {
        PtNnLayer &L = p.layers[i];
        L.name = G[i].name; L.level = G[i].level; L.pool = G[i].pool; L.upsample = G[i].up; L.src0 = G[i].s0; L.src1 = G[i].s1;
        L.relu = i != PT_NN_LAYERS - 1;
        L.cout = cout[i];
        L.cin0 = L.src0 == -1 ? ic : cout[L.src0];
        L.cin1 = L.src1 == -2 ? 0 : L.src1 == -1 ? ic : cout[L.src1];
    }
    return p;
}

// one plan checked; returns its tile count
static int check(const PtNnPlan &plan, int W, int H, int mb) {
    const int O = PTX_NN_TILE_OVERLAP, A = PTX_NN_TILE_ALIGN;
    const PtNnTiling t = pt_nn_tiling(plan, W, H, mb);
    plans++;
    const int n = t.count();
    CHECK(t.tiles_x >= 1 && t.tiles_y >= 1 && t.width == W && t.height == H && t.max_memory_mb == mb, "the plan's own fields");
    CHECK(t.tile_width % A == 0 && t.tile_height % A == 0, "the tile buffer is aligned");
    CHECK(t.tile_width <= PTX_NN_MAX_WIDTH && t.tile_height <= PTX_NN_MAX_HEIGHT, "the tile buffer is within the cap");
    CHECK(n == 1 || (t.tile_width >= PTX_NN_MIN_TILE || t.tiles_x == 1), "tiles in x only of at least the minimum width");
    CHECK(n == 1 || (t.tile_height >= PTX_NN_MIN_TILE || t.tiles_y == 1), "tiles in y only of at least the minimum height");
    if (mb == 0 && W <= PTX_NN_MAX_WIDTH && H <= PTX_NN_MAX_HEIGHT)
        CHECK(n == 1 && t.tile_width == pt_nn_pad16(W) && t.tile_height == pt_nn_pad16(H), "no limit within the cap is one tile: the padded frame");
    const PtNnScratch whole = pt_nn_scratch(plan, t.tile_width, t.tile_height);
    if (mb > 0 && (t.tile_width > PTX_NN_MIN_TILE || t.tile_height > PTX_NN_MIN_TILE))
        CHECK((uint64_t)whole.total <= ((uint64_t)mb << 20), "the limit is kept above the minimum tile");
    std::vector<ptx_nn_tile> tiles((size_t)n);
    uint64_t macs = 0;
    for (int k = 0; k < n; k++) tiles[(size_t)k] = pt_nn_tile_at(t, k);
    for (int i = 0; i < t.tiles_y; i++)
        for (int j = 0; j < t.tiles_x; j++) {
            const ptx_nn_tile &T = tiles[(size_t)i * t.tiles_x + j];
            CHECK(T.x >= 0 && T.y >= 0 && T.w >= 1 && T.h >= 1 && T.x + T.w <= W && T.y + T.h <= H, "the window lies inside the frame");
            CHECK(T.x % A == 0 && T.y % A == 0, "the window begins at a multiple of 16");
            CHECK(T.w <= t.tile_width && T.h <= t.tile_height, "the window fits the tile buffer");
            // the kept rectangles are a grid: each begins where its left / upper neighbour ends, the first at 0, the last ends at W / H
            const int want_x = j ? tiles[(size_t)i * t.tiles_x + j - 1].out_x + tiles[(size_t)i * t.tiles_x + j - 1].out_w : 0;
            const int want_y = i ? tiles[(size_t)(i - 1) * t.tiles_x + j].out_y + tiles[(size_t)(i - 1) * t.tiles_x + j].out_h : 0;
            CHECK(T.out_x == want_x && T.out_y == want_y && T.out_w >= 1 && T.out_h >= 1, "the kept rectangles join without gap or overlap");
            if (j == t.tiles_x - 1) CHECK(T.out_x + T.out_w == W, "the last column's kept rectangle ends at the frame's edge");
            if (i == t.tiles_y - 1) CHECK(T.out_y + T.out_h == H, "the last row's kept rectangle ends at the frame's edge");
            if (i) CHECK(T.out_x == tiles[(size_t)j].out_x && T.out_w == tiles[(size_t)j].out_w, "a column's kept rectangles share x");
            if (j) CHECK(T.out_y == tiles[(size_t)i * t.tiles_x].out_y && T.out_h == tiles[(size_t)i * t.tiles_x].out_h, "a row's kept rectangles share y");
            CHECK(T.out_x >= T.x && T.out_y >= T.y && T.out_x + T.out_w <= T.x + T.w && T.out_y + T.out_h <= T.y + T.h, "the kept rectangle lies in the window");
            // a window edge that is not a frame edge is at least the overlap away from every kept pixel
            if (T.x > 0) CHECK(T.out_x - T.x >= O, "left overlap");
            if (T.y > 0) CHECK(T.out_y - T.y >= O, "top overlap");
            if (T.x + T.w < W) CHECK(T.x + T.w - (T.out_x + T.out_w) >= O, "right overlap");
            if (T.y + T.h < H) CHECK(T.y + T.h - (T.out_y + T.out_h) >= O, "bottom overlap");
            const PtNnScratch s = pt_nn_scratch(plan, T.w, T.h);
            CHECK(s.total <= whole.total && s.in_offset == whole.in_offset, "a tile's scratch is within the buffer's");
            for (int l = 0; l < PT_NN_LAYERS; l++) CHECK(s.out_offset[l] <= whole.out_offset[l], "a tile's tensors are prefixes of the buffer's");
            macs += s.macs;
        }
    CHECK(macs == pt_nn_tiling_macs(plan, t), "macs are summed over the tiles");
    return n;
}

int main() {
    static const int standard[10] = {32, 48, 64, 80, 96, 112, 96, 64, 64, 32}, ones[10] = {1, 1, 1, 1, 1, 1, 1, 1, 1, 1};
    const PtNnPlan plans2[2] = {make_plan(9, standard), make_plan(3, ones)};
    std::vector<int> small, large = {1, 17, 288, 289, 1920, 3840, 4320, 4321, 7680, 7681, PTX_NN_MAX_FRAME};
    for (int v = 1; v <= 700; v += 7) small.push_back(v);
    for (int v : {16, 287, 288, 289, 304, 305, 480, 481}) small.push_back(v);
    int most = 0;
    for (const PtNnPlan &plan : plans2)
        for (const std::vector<int> *sizes : {&small, &large})
            for (int W : *sizes)
                for (int H : *sizes)
                    for (int mb = 0;; mb = mb ? 2 * mb : 1) {
                        const int n = check(plan, W, H, mb);
                        most = n > most ? n : most;
                        if ((mb > 0 && n == 1) || mb >= (1 << 20)) break;      // (frames above the cap never reach one tile)
                    }
    printf("nn_tiles_check: %ld plans, at most %d tiles\n", plans, most);
    printf("nn_tiles_check: %ld failures\n", failures);
    return failures ? 1 : 0;
}
