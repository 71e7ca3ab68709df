// pt_nn_progress.h -- host only, no hip* call: the bookkeeping of the network denoiser's progress monitor (ptx_nn_set_progress of
// include/mi355x_pathtracer.h, "progress"; pt_nn.hip and the image units run by it, tests/nn_progress_check.cpp holds it under the
// sanitizers).  A call's work is counted in units: per tile its input stage, each of its sixteen layers and its output stage, and one
// more for the frame where the in-place copy-out runs.  The monitor hears 0 before anything is enqueued, then (finished units) / (all
// units) after each unit has finished on the device, the last report exactly 1.  A monitor that returns 0 cancels: no report follows.
#pragma once
#include "../../include/mi355x_pathtracer.h"

constexpr int PT_NN_TILE_UNITS = 18;          // input, sixteen layers, output (PT_NN_LAYERS + 2; pt_nn.hip asserts it)

inline long long pt_nn_progress_units(int tiles, bool copy_out) { return (long long)tiles * PT_NN_TILE_UNITS + (copy_out ? 1 : 0); }

struct PtNnProgress {
    ptx_nn_progress_fn fn = nullptr;          // NULL: no monitor
    void *user = nullptr;
    long long total = 0, done = 0;
    bool running = false;                     // between a call's first report and its end: the tile loop reports

    bool say(double v) {
        if (fn(user, v)) return true;
        running = false;
        return false;
    }
    // the first report; false: cancelled
    bool begin(int tiles, bool copy_out) {
        total = pt_nn_progress_units(tiles, copy_out); done = 0; running = true;
        return say(0.0);
    }
    // one more unit has finished on the device; false: cancelled (at the last unit too)
    bool unit() {
        done++;
        return say(done >= total ? 1.0 : (double)done / (double)total);
    }
    void end() { running = false; }
};

// The tile loop under a monitor.  enqueue(k) enqueues tile k's eighteen stages with a marker behind each; wait(k, s) returns once stage
// s of tile k has finished.  The host enqueues at most one tile beyond the tile whose reports it is delivering, so a cancel leaves at
// most two tiles in flight.  PTX_OK, PTX_ERR_CANCELLED (nothing further was enqueued; what is in flight is the caller's to wait for),
// or what enqueue / wait returned.
template <class Enqueue, class Wait> int pt_nn_progress_tiles(PtNnProgress &pg, int tiles, Enqueue enqueue, Wait wait) {
    auto deliver = [&](int k) {
        for (int s = 0; s < PT_NN_TILE_UNITS; s++) {
            if (const int rc = wait(k, s)) return rc;
            if (!pg.unit()) return PTX_ERR_CANCELLED;
        }
        return PTX_OK;
    };
    for (int k = 0; k < tiles; k++) {
        if (const int rc = enqueue(k)) return rc;
        if (k >= 1)
            if (const int rc = deliver(k - 1)) return rc;
    }
    return tiles > 0 ? deliver(tiles - 1) : PTX_OK;
}
