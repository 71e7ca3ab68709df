"""Device time of the denoiser's guide pass at 1920x1080: k_gbuffer (the pixel-centre guides, count 0) and k_guides (the sampled guides,
ptx_set_guide_samples) for K = 1, 4, 16 with antialiasing and depth of field on, on cornellObj.txt and the 20k-triangle scene.
Neither kernel has an entry point that enqueues it alone, so each figure is a difference: `reps` back-to-back ptx_denoise calls of one
pass with the guides marked stale before every call (ptx_set_guide_samples with another iter_first, or count 0 <-> 1 -> 0: host work
only, nothing is enqueued and the stream is not waited for) minus the same calls with the guides left valid, between hipEvents on the
tracer's stream.  Three runs of each, alternated: the median difference and the spread (max - min) of the three are printed.
k_gbuffer is the parent commit's kernel unchanged (pt_engine.hip's code object holds the same kernel), so its line is the parent's
time on the same box in the same process.
    python tools/gpu_guides_time.py [--reps N]      (the lines go to profiles/guides_time.txt)"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mygpuraytracer_amd as pt  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    args = ap.parse_args()
    import torch
    from conftest import ensure_standin_assets
    ensure_standin_assets()
    W, H = 1920, 1080
    for scene in ("cornellObj.txt", "cornellSpaceship20k.txt"):
        s = pt.Scene(os.path.join(ROOT, "scenes", scene), res=(W, H), depth=8)
        s.apply_runcuda_camera()
        with pt.Tracer(s, antialiasing=1, depth_of_field=1) as T:
            T.render(1, 2)
            T.denoise(2, passes=1)                       # warm-up: buffers, code objects
            st = torch.cuda.ExternalStream(T.stream_ptr())
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

            def timed(stale):
                T.synchronize()
                e0.record(st)
                for r in range(args.reps):
                    stale(r)
                    T.denoise(2, read=False, passes=1)
                e1.record(st)
                e1.synchronize()
                return e0.elapsed_time(e1) / args.reps

            def centre_stale(r):
                T.set_guide_samples(1)
                T.set_guide_samples(0)

            row = dict(scene=scene, res="%dx%d" % (W, H), reps=args.reps)
            for K in (0, 1, 4, 16):
                T.set_guide_samples(K)
                stale = centre_stale if K == 0 else (lambda r, K=K: T.set_guide_samples(K, 3 - T.guide_samples()[1]))      # iter_first 1 <-> 2
                T.denoise(2, passes=1)
                runs = []
                for _ in range(3):                       # alternated: filter alone, guides + filter
                    base = timed(lambda r: None)
                    runs.append(timed(stale) - base)
                name = "k_gbuffer" if K == 0 else "k_guides_K%d" % K
                row[name + "_ms"] = round(sorted(runs)[1], 4)
                row[name + "_spread_ms"] = round(max(runs) - min(runs), 4)
                row[name + "_runs_ms"] = [round(x, 4) for x in runs]
            for K in (1, 4, 16):
                row["K%d_over_K_gbuffer" % K] = round(row["k_guides_K%d_ms" % K] / (K * row["k_gbuffer_ms"]), 3)
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
