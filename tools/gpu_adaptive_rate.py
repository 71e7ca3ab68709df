"""Adaptive sampling by tiles on C4 (cornellObj.txt, 1920x1080, depth 8), three figures for DESIGN.md 10:
  1. the cost of one round's bookkeeping -- ptx_adaptive_add + ptx_adaptive_select (tile errors, decision, status, mask, the one read
     back) -- on the host clock around the two calls with the stream drained before, median over the rounds; beside ptx_moments_add +
     ptx_moments_summarize, the same pair of the --until-error loop;
  2. ms per iteration (ptx_render of 16, hipEvents through ptx_last_loop_ms) against the fraction of active tiles, with masks that
     keep the tiles of largest error first, as the select does;
  3. --adaptive E against --until-error run to the same worst-tile error: pixel-samples and wall time.  The uniform run goes on in
     batches of the same size until the largest tile error, measured by the same kernel on its own moments (every tile kept active:
     min_batches above any count), is at E.
    python tools/gpu_adaptive_rate.py [--target E] [--batch K] [--res W H] [--cap N]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mygpuraytracer_amd as pt  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--target", type=float, default=0.02)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--res", type=int, nargs=2, default=(1920, 1080))
    ap.add_argument("--cap", type=int, default=32768)
    args = ap.parse_args()
    W, H = args.res
    K = args.batch
    s = pt.Scene(os.path.join(ROOT, "scenes", "cornellObj.txt"), res=(W, H), depth=8)
    s.apply_runcuda_camera()
    with pt.Tracer(s) as T, pt.Moments(0, W, H) as m, pt.Adaptive(0, W, H) as a:
        nt = T.num_tiles
        # 3a. the adaptive run, its rounds timed as they go (1.)
        T.render(1, K)                                               # warm-up: code objects, buffers
        T.reset_image()
        T.synchronize()
        t0 = time.perf_counter()
        done, book, rounds = 0, [], []
        while done < args.cap:
            T.render(done + 1, K)
            done += K
            T.synchronize()
            b0 = time.perf_counter()
            a.add(m, T, K)
            st = a.select(m, T, target=args.target)
            book.append((time.perf_counter() - b0) * 1e3)
            rounds.append(st)
            if st["tiles_active"] == 0:
                break
        a.resolve(T)
        r = a.read()
        wall_adaptive = time.perf_counter() - t0
        last = rounds[-1]
        print(json.dumps(dict(what="adaptive", res="%dx%d" % (W, H), target=args.target, batch=K, rounds=len(rounds), iterations=done,
                              ended="every tile at its target" if last["tiles_active"] == 0 else "cap", tiles=nt,
                              pixel_samples=last["samples_total"], per_pixel=round(last["samples_total"] / (W * H), 1),
                              samples_min=last["samples_min"], samples_max=last["samples_max"], worst_error=last["worst_error"],
                              wall_s=round(wall_adaptive, 3), round_bookkeeping_ms_median=round(float(np.median(book)), 4),
                              round_bookkeeping_ms_max=round(max(book), 4))), flush=True)
        print(json.dumps(dict(what="active tiles by round", every=8, tiles_active=[x["tiles_active"] for x in rounds][::8])), flush=True)
        order = np.argsort(-r["tile_error"])                         # largest error first
        # 2. ms per iteration against the active fraction
        for frac in (1.0, 0.75, 0.5, 0.25, 0.1, 0.03, 0.0):
            mask = np.zeros(nt, np.uint8)
            mask[order[:int(round(frac * nt))]] = 1
            T.set_active_tiles(mask)
            T.render(100001, K)                                      # warm-up under this mask
            T.synchronize()
            ms = []
            for rep in range(3):
                before = T.stats()["loop_ms_total"]
                T.render(100001 + K * (rep + 1), K)
                T.synchronize()
                ms.append((T.stats()["loop_ms_total"] - before) / K)
            print(json.dumps(dict(what="ms per iteration", active_fraction=frac, tiles_active=int(mask.sum()),
                                  ms_per_iteration=round(sorted(ms)[1], 4))), flush=True)
        # 1b. the --until-error pair, and 3b. the uniform run to the same worst-tile error
        T.clear_active_tiles()
        T.reset_image()
        m.reset()
        a.reset()
        T.synchronize()
        t0 = time.perf_counter()
        done, pair, worst = 0, [], None
        while done < args.cap:
            T.render(done + 1, K)
            done += K
            T.synchronize()
            b0 = time.perf_counter()
            a.add(m, T, K)                                           # (every tile stays active: the plain add's arithmetic and traffic)
            st = a.select(m, T, target=args.target, min_batches=1 << 30)
            pair.append((time.perf_counter() - b0) * 1e3)
            worst = st["worst_error"]
            if done >= 4 * K and worst <= args.target:
                break
        wall_uniform = time.perf_counter() - t0
        print(json.dumps(dict(what="uniform to the same worst-tile error", iterations=done, pixel_samples=done * W * H, worst_error=worst,
                              ended="worst tile at the target" if worst <= args.target else "cap", wall_s=round(wall_uniform, 3),
                              pixel_samples_ratio_adaptive=round(last["samples_total"] / (done * W * H), 4),
                              wall_ratio_adaptive=round(wall_adaptive / wall_uniform, 4))), flush=True)
        m.reset()
        T.reset_image()
        T.render(1, K)
        T.synchronize()
        plain = []
        for i in range(2, 12):
            b0 = time.perf_counter()
            m.add(T, K * i)                                          # (the frame does not change: the batches are zeros, the traffic is the same)
            m.summary()
            plain.append((time.perf_counter() - b0) * 1e3)
        print(json.dumps(dict(what="ptx_moments_add + ptx_moments_summarize, host clock", ms_median=round(float(np.median(plain)), 4))), flush=True)


if __name__ == "__main__":
    main()
