"""Device time of the denoiser's guide pass with the guide rays followed through mirrors and glass (ptx_set_guide_bounces) at 1920x1080
on cornell.txt and cornellGlass.txt: the pixel-centre mode (K = 0) and K = 16 sampled guides with antialiasing and depth of field on,
at bounces = 0, 1, 8.  bounces = 0 launches the parent commit's kernels unchanged (k_gbuffer, k_guides), in the same process on the
same box: that is the yardstick, and its spread the yardstick's run-to-run spread.  As in tools/gpu_guides_time.py each figure is a
difference: `reps` back-to-back one-pass ptx_denoise calls with the guides marked stale before every call (ptx_set_guide_samples to
another value and back, or another iter_first: host work only) minus the same calls with the guides left valid, between hipEvents on
the tracer's stream; three runs of each, alternated: the median difference and the spread (max - min) of the three.
The expectation printed next to each ratio is 1 + the mean number of continuations per guide ray, counted by the restatement
(tests/guide_bounces_ref.py) on the CPU oracle's pixel-centre rays of the same view at 480x270.
    python tools/gpu_guide_bounces_time.py [--reps N]      (the lines go to profiles/guide_bounces_time.txt)"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mygpuraytracer_amd as pt  # noqa: E402


def mean_continuations(scene, bounces):
    """per pixel-centre guide ray of the view at 480x270, from the restatement on the CPU oracle"""
    from cpulibs import OracleLib
    from guide_bounces_ref import effective_bounces, follow
    s = pt.Scene(os.path.join(ROOT, "scenes", scene), res=(480, 270), depth=8)
    s.apply_runcuda_camera()
    d = s.dump()
    O = OracleLib()
    O.set_libm(1)
    O.create(d, d["textures"])
    O.set_options(aa=0, dof=0)
    O.pt_init()
    O.pt_generate(1)
    paths = O.paths()
    out = {B: float(follow(O, d, paths, effective_bounces(d, B))["continuations"].mean()) for B in bounces}
    O.set_libm(0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    args = ap.parse_args()
    import torch
    W, H = 1920, 1080
    BOUNCES = (0, 1, 8)
    for scene in ("cornell.txt", "cornellGlass.txt"):
        cont = mean_continuations(scene, BOUNCES)
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

            for K in (0, 16):
                T.set_guide_samples(K)
                stale = centre_stale if K == 0 else (lambda r, K=K: T.set_guide_samples(K, 3 - T.guide_samples()[1]))      # iter_first 1 <-> 2
                row = dict(scene=scene, res="%dx%d" % (W, H), reps=args.reps, K=K)
                runs = {B: [] for B in BOUNCES}
                for _ in range(3):                       # alternated: every bounces value in turn; filter alone, guides + filter
                    for B in BOUNCES:
                        T.set_guide_bounces(B)
                        T.denoise(2, passes=1)
                        base = timed(lambda r: None)
                        runs[B].append(timed(stale) - base)
                T.set_guide_bounces(0)
                for B in BOUNCES:
                    row["B%d_ms" % B] = round(sorted(runs[B])[1], 4)
                    row["B%d_spread_ms" % B] = round(max(runs[B]) - min(runs[B]), 4)
                    row["B%d_runs_ms" % B] = [round(x, 4) for x in runs[B]]
                for B in BOUNCES[1:]:
                    row["B%d_over_B0" % B] = round(row["B%d_ms" % B] / row["B0_ms"], 3)
                    row["B%d_expected" % B] = round(1.0 + cont[B], 3)
                print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
