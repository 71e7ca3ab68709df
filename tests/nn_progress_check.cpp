// nn_progress_check.cpp -- csrc/pt_nn_progress.h (host only) as a stand-alone program under -fsanitize=address,undefined, run by
// tests/test_nn_progress_cpu.py: the unit counts, the report sequence of the tile loop with a fake device (enqueue and wait are
// recorded, nothing runs), the lead of the enqueue over the reports, and a cancel at every report index.
#include <stdio.h>
#include <stdlib.h>
#include <vector>

#include "pt_nn_progress.h"

static long long failures = 0, checks = 0;
#define CHECK(cond) do { checks++; if (!(cond)) { failures++; printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); } } while (0)

struct Log {
    std::vector<double> said;
    long long cancel_at = -1;                 // the report index that answers 0; -1: none
    static int hear(void *user, double n) {
        Log *l = static_cast<Log *>(user);
        l->said.push_back(n);
        return (long long)l->said.size() - 1 == l->cancel_at ? 0 : 1;
    }
};

// One call as the units make it: begin, the tile loop, the copy-out's unit.  Returns the code the call would return.
static int run(PtNnProgress &pg, int tiles, bool copy_out, int *enqueued_out, int *max_lead_out) {
    int enqueued = 0, delivering = -1, max_lead = 0;
    long long waited = 0;
    if (!pg.begin(tiles, copy_out)) { *enqueued_out = 0; *max_lead_out = 0; return PTX_ERR_CANCELLED; }
    int rc = pt_nn_progress_tiles(pg, tiles,
        [&](int k) { CHECK(k == enqueued); CHECK(pg.running); enqueued++; return PTX_OK; },
        [&](int k, int s) {
            CHECK(k < enqueued);                                   // only what was enqueued is waited for
            CHECK(k * (long long)PT_NN_TILE_UNITS + s == waited);  // in order, each stage once
            waited++;
            delivering = k;
            if (enqueued - 1 - delivering > max_lead) max_lead = enqueued - 1 - delivering;
            return PTX_OK;
        });
    if (rc == PTX_OK && copy_out && !pg.unit()) rc = PTX_ERR_CANCELLED;
    pg.end();
    *enqueued_out = enqueued; *max_lead_out = max_lead;
    return rc;
}

int main() {
    CHECK(PT_NN_TILE_UNITS == 18);
    CHECK(pt_nn_progress_units(1, false) == 18 && pt_nn_progress_units(1, true) == 19);
    CHECK(pt_nn_progress_units(2, false) == 36 && pt_nn_progress_units(2, true) == 37);
    CHECK(pt_nn_progress_units(28, false) == 504 && pt_nn_progress_units(28, true) == 505);
    CHECK(pt_nn_progress_units(1 << 20, true) == 18ll * (1 << 20) + 1);

    const int tile_counts[] = {1, 2, 3, 28};
    for (const int tiles : tile_counts)
        for (int copy = 0; copy < 2; copy++) {
            const long long units = pt_nn_progress_units(tiles, copy != 0);
            // complete
            {
                Log log;
                PtNnProgress pg;
                pg.fn = Log::hear; pg.user = &log;
                int enq, lead;
                CHECK(run(pg, tiles, copy != 0, &enq, &lead) == PTX_OK);
                CHECK(enq == tiles && lead <= 1 && (tiles == 1 || lead == 1));
                CHECK((long long)log.said.size() == units + 1);
                CHECK(log.said.front() == 0.0 && log.said.back() == 1.0);
                for (size_t i = 1; i < log.said.size(); i++) CHECK(log.said[i] > log.said[i - 1]);
                for (size_t i = 1; i + 1 < log.said.size(); i++) CHECK(log.said[i] > 0.0 && log.said[i] < 1.0);
                CHECK(!pg.running && pg.done == units && pg.total == units);
                if (tiles == 1) CHECK((long long)log.said.size() - 2 >= 17 && (long long)log.said.size() - 1 >= 18);
            }
            // a cancel at every report index: that report is the last, nothing beyond one tile ahead was enqueued
            for (long long at = 0; at <= units; at++) {
                Log log;
                log.cancel_at = at;
                PtNnProgress pg;
                pg.fn = Log::hear; pg.user = &log;
                int enq, lead;
                CHECK(run(pg, tiles, copy != 0, &enq, &lead) == PTX_ERR_CANCELLED);
                CHECK((long long)log.said.size() == at + 1);
                CHECK(!pg.running);
                if (at == 0) CHECK(enq == 0);
                else {
                    const int tile = (int)((at - 1) / PT_NN_TILE_UNITS);          // the tile whose unit was reported last
                    CHECK(enq <= (tile < tiles ? tile + 2 : tiles) && enq <= tiles && enq >= (tile < tiles ? tile + 1 : tiles));
                }
                if (at == units) CHECK(log.said.back() == 1.0);                   // a 0 on the last report cancels too
                // the same state runs a whole call afterwards
                Log again;
                pg.user = &again;
                CHECK(run(pg, tiles, copy != 0, &enq, &lead) == PTX_OK && (long long)again.said.size() == units + 1 && again.said.back() == 1.0);
            }
        }
    printf("nn_progress_check: %lld failures in %lld checks\n", failures, checks);
    return failures ? 1 : 0;
}
