// CPU check of the local index's plan (csrc/pt_plan.hip, plan_local_index): linked with that unit alone and run under the sanitizers by
// tests/test_loop_index_plan.py.  Over a grid of frame sizes, bins, launch-set sizes, budgets and switches it holds the plan to the rule
// as pt_plan.h states it, restated here: N2 is the smallest power of two >= the stage's slots; the bound an entry is checked against
// (nbins x N2) times the words per entry is what one segment's allocation holds; the bytes per path the memory rule counts are 176 - 24 +
// the index of two stages; and the plan falls back to the tail's index exactly where a term of the predicate fails, naming the first.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "pt_plan.h"

using namespace ptd;

static int failures = 0, loops = 0, fallbacks[7] = {0, 0, 0, 0, 0, 0, 0}, two_words = 0;
#define CHECK(cond) do { if (!(cond)) { failures++; printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); } } while (0)

static PlanFacts facts(int cus, int owned, int nbins, int lanes, bool split) {
    PlanFacts f;
    f.cus = cus; f.maxTiles = (owned + 255) / 256; f.nbins = nbins; f.nmats = nbins; f.ngeoms = 7; f.lanes = lanes;
    f.split_mesh = split; f.uses_uv = 0; f.sort_by_material = nbins > 1; f.cull = 1; f.tri_lds = 1; f.bump_bits = 0; f.ntri_lds = 0; f.ntri = 0;
    f.has_bvh = split; f.bvh_stack = 32;
    f.dbg = read_debug_switches();
    plan_grids(f);
    return f;
}

static void check_one(const PlanFacts &f, int owned, int kmax, long long budget) {
    const int slots = f.maxTiles * 256;
    const IndexPlan x = plan_local_index(f, slots, owned, kmax, budget);
    // N2: a power of two, >= slots, the smallest
    const size_t n2 = (size_t)1 << x.n2_log2;
    CHECK(n2 >= (size_t)slots && (n2 == 1 || n2 / 2 < (size_t)slots));
    // words: 2 exactly where some launch set the tracer can plan keeps the two-word form
    int words = 1;
    for (int K = 1; K <= kmax; K++)
        for (int v = 0; v < 4; v++) {
            const BatchPlan p = plan_batch(f, K, v & 1, (v & 2) != 0);
            if (!p.idx16_first || !p.idx16_later) words = 2;
        }
    const size_t entries = (size_t)f.nbins * n2;
    const long long bytes = 176 - 24 + (long long)((2 * 4 * entries * words + slots - 1) / slots);
    int why = 0;
    if (f.dbg.tail_index) why = 1;
    else if (f.split_mesh) why = 2;
    else if (f.nbins > 64) why = 3;
    else if (entries > ((size_t)1 << 30)) why = 5;      // (4, no direct epilogue, is a build option: not reachable here)
    else if (bytes * f.lanes * owned * kmax > budget) why = 6;
    CHECK(x.why_code == why && x.loop == (why == 0));
    if (x.loop) {
        loops++;
        CHECK(x.words == words && x.entries == entries && x.seg_words == entries * (size_t)words && x.bytes_per_path == bytes);
        CHECK(x.entries * sizeof(int32_t) <= ((size_t)1 << 32));                       // an entry's byte offset fits 32 bits
        CHECK(x.bytes_per_path * f.lanes * owned * kmax <= budget);                     // the bytes-per-path rule holds
        if (words == 2) two_words++;
    } else {
        fallbacks[why]++;
        CHECK(x.entries == 0 && x.seg_words == 0 && x.words == 1 && x.bytes_per_path == 176 && x.why[0] != 0);
    }
}

int main() {
    const int sizes[] = {1, 255, 256, 257, 96 * 64, 300 * 130, 520 * 254, 1920 * 1080 / 8, 1920 * 1080, 3840 * 2160, 7680 * 4320};
    const int bins[] = {1, 2, 7, 8, 63, 64, 65, 200};
    const long long budgets[] = {8LL << 20, 1LL << 30, 64LL << 30};
    const char *envs[][2] = {{nullptr, nullptr}, {"PTX_DEBUG_TAIL_INDEX", "1"}, {"PTX_DEBUG_NO_IDX16", "1"}, {"PTX_DEBUG_TOTAL_WG_PER_CU", "1"}};
    for (const auto &e : envs) {
        if (e[0]) setenv(e[0], e[1], 1);
        for (int owned : sizes) for (int nb : bins) for (int lanes : {1, 3}) for (int split = 0; split < 2; split++) {
            const PlanFacts f = facts(256, owned, nb, lanes, split != 0);
            for (int kmax : {1, 2, 12, 64}) for (long long b : budgets) check_one(f, owned, kmax, b);
        }
        if (e[0]) unsetenv(e[0]);
    }
    // the bench's shape: 1920 x 1080, seven bins, three lanes of twelve iterations, a quarter of 288 GB capped at 64 GB
    {
        const PlanFacts f = facts(256, 1920 * 1080, 7, 3, false);
        const IndexPlan x = plan_local_index(f, 8100 * 256, 1920 * 1080, 12, launch_budget_bytes((size_t)280 << 30, (size_t)288 << 30, 0));
        CHECK(x.loop && x.n2_log2 == 21 && x.words == 1 && x.entries == (size_t)7 << 21 && x.bytes_per_path == 152 + 57);
    }
    CHECK(launch_budget_bytes(0, 0, 0) == 64LL << 30 && launch_budget_bytes((size_t)8 << 30, (size_t)16 << 30, 0) == 2LL << 30 && launch_budget_bytes(1, 2, 8) == 8LL << 20);
    // every branch was taken
    CHECK(loops > 0 && two_words > 0 && fallbacks[1] > 0 && fallbacks[2] > 0 && fallbacks[3] > 0 && fallbacks[5] > 0 && fallbacks[6] > 0);
    printf("loop_index_check: %d failures (%d plans bin-major, %d of them two words; fallbacks %d %d %d %d %d)\n", failures, loops, two_words, fallbacks[1], fallbacks[2],
           fallbacks[3], fallbacks[5], fallbacks[6]);
    return failures != 0;
}
