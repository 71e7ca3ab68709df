"""Device time of the network denoiser's prefiltered guides (ptx_nn_prefilter_*, ptx_denoise_nn_prefiltered) at 1920x1080 and 3840x2160,
by tools/gpu_nn_rate.py's method: hipEvents on one stream around `inner` back-to-back calls, the calls alternated within a round, the
figure the median over the rounds (minimum and maximum next to it).  Synthetic weights on the standard channel table: time does not
depend on the weights' values.
    prefilter_ms     one ptx_nn_prefilter_run_device with both networks on W*H*3 images
    plain_ms         Tracer.denoise_nn on a 9-input network, the guides as the G-buffer has them
    first_ms         the same with a prefilter whose clean guides were invalidated before each call: both prefilter networks, then the main one
    cached_ms        the same with the clean guides of this G-buffer cached: the main network alone
The tracer renders one iteration of scenes/cornell.txt at the size; the G-buffer is computed before the timed calls.
    --other-lib SO   another build of the library (the parent commit's): a tracer and a one-tile 9-input handle of its own from the same
                     scene and blob, its ptx_denoise_nn alternated with this tree's plain call in the same rounds (other_plain_ms);
                     --other-first: the other build's call goes first in every round
    python tools/gpu_nn_prefilter_rate.py [--rounds N] [--inner M] [--sizes WxH,..] [--max-memory-mb L] [--other-lib SO [--other-first]] [--out FILE]"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mygpuraytracer_amd as pt  # noqa: E402
import unet_ref as U  # noqa: E402


class OtherTracer:
    """a tracer on `stream` and a one-tile network handle of another build of the library, through entry points every build has"""

    def __init__(self, path, scene_path, w, h, depth, blob, stream):
        L = self.L = ctypes.CDLL(os.path.abspath(path))
        vp, i = ctypes.c_void_p, ctypes.c_int
        L.ptx_last_error.restype = ctypes.c_char_p
        L.ptx_scene_load.restype, L.ptx_scene_load.argtypes = i, [ctypes.c_char_p, ctypes.c_char_p, ctypes.POINTER(vp)]
        L.ptx_scene_free.argtypes = L.ptx_destroy.argtypes = L.ptx_scene_apply_runcuda_camera.argtypes = [vp]
        L.ptx_scene_set_resolution.argtypes, L.ptx_scene_set_trace_depth.argtypes = [vp, i, i], [vp, i]
        L.ptx_default_options.argtypes = [ctypes.POINTER(pt.Options)]
        L.ptx_create_from_scene.restype, L.ptx_create_from_scene.argtypes = i, [vp, ctypes.POINTER(pt.Options), vp, vp, ctypes.POINTER(vp)]
        L.ptx_render_strided.restype, L.ptx_render_strided.argtypes = i, [vp, i, i, i]
        L.ptx_nn_create.restype, L.ptx_nn_create.argtypes = i, [i, i, i, vp, ctypes.c_size_t, ctypes.POINTER(vp)]
        L.ptx_nn_destroy.restype, L.ptx_nn_destroy.argtypes = None, [vp]
        L.ptx_denoise_nn.restype, L.ptx_denoise_nn.argtypes = i, [vp, vp, ctypes.POINTER(pt.NNParams), i]
        self.scene, self.t, self.nn = vp(), vp(), vp()
        self.ok(L.ptx_scene_load(scene_path.encode(), None, ctypes.byref(self.scene)))
        L.ptx_scene_set_resolution(self.scene, w, h)
        L.ptx_scene_set_trace_depth(self.scene, depth)
        L.ptx_scene_apply_runcuda_camera(self.scene)
        opt = pt.Options()
        L.ptx_default_options(ctypes.byref(opt))
        self.ok(L.ptx_create_from_scene(self.scene, ctypes.byref(opt), None, vp(stream), ctypes.byref(self.t)))
        self.ok(L.ptx_render_strided(self.t, 1, 1, 1))
        self.ok(L.ptx_nn_create(0, w, h, ctypes.cast(ctypes.c_char_p(blob), vp), len(blob), ctypes.byref(self.nn)))
        self.params = pt.default_nn_params()

    def ok(self, rc):
        if rc:
            raise RuntimeError(self.L.ptx_last_error().decode())

    def denoise(self):
        self.ok(self.L.ptx_denoise_nn(self.t, self.nn, ctypes.byref(self.params), 1))

    def close(self):
        self.L.ptx_nn_destroy(self.nn)
        self.L.ptx_destroy(self.t)
        self.L.ptx_scene_free(self.scene)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--sizes", default="1920x1080,3840x2160")
    ap.add_argument("--max-memory-mb", type=int, default=None)
    ap.add_argument("--other-lib", default=None)
    ap.add_argument("--other-first", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    pt.load_library()
    st = torch.cuda.Stream()
    aux, main9 = U.weights_blob(U.synthetic_weights(3, 1)), U.weights_blob(U.synthetic_weights(9, 1))
    rows = []
    for W, H in (tuple(int(v) for v in s.split("x")) for s in args.sizes.split(",")):
        s = pt.Scene(os.path.join(ROOT, "scenes", "cornell.txt"), res=(W, H), depth=4)
        s.apply_runcuda_camera()
        rng = np.random.default_rng(W)
        img = [torch.from_numpy(rng.random((H, W, 3), dtype=np.float32)).to("cuda:0") for _ in range(2)]
        with pt.Tracer(s, stream_ptr=st.cuda_stream) as T, pt.NN(W, H, main9, max_memory_mb=args.max_memory_mb) as nn, \
                pt.NNPrefilter(W, H, aux, aux, max_memory_mb=args.max_memory_mb) as alone, \
                pt.NNPrefilter(W, H, aux, aux, max_memory_mb=args.max_memory_mb) as pf:
            T.render(1, 1)

            def first():
                pf.invalidate()
                T.denoise_nn(nn, 1, read=False, prefilter=pf)

            calls = dict(prefilter=lambda: alone.device(img[0].data_ptr(), img[1].data_ptr(), stream=st.cuda_stream),
                         plain=lambda: T.denoise_nn(nn, 1, read=False),
                         first=first,
                         cached=lambda: T.denoise_nn(nn, 1, read=False, prefilter=pf))
            other = None
            if args.other_lib:                                       # (after torch and this tree's library: one HIP runtime in the process)
                other = OtherTracer(args.other_lib, os.path.join(ROOT, "scenes", "cornell.txt"), W, H, 4, main9, st.cuda_stream)
                calls = dict(other_plain=other.denoise, plain=calls["plain"]) if args.other_first else dict(plain=calls["plain"], other_plain=other.denoise)
            for f in calls.values():
                for _ in range(3):
                    f()
            st.synchronize()
            runs0 = pf.info()["runs"]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ms = {k: [] for k in calls}
            for _ in range(args.rounds):
                for k, f in calls.items():
                    if k == "cached":
                        f()                                          # (the call before the timed ones fills the cache: `first` left it filled too)
                        st.synchronize()
                    e0.record(st)
                    for _ in range(args.inner):
                        f()
                    e1.record(st)
                    e1.synchronize()
                    ms[k].append(e0.elapsed_time(e1) / args.inner)
            info = pf.info()
            assert info["runs"] - runs0 == (args.rounds * args.inner if "first" in calls else 0), "the cached calls ran a prefilter network"
            row = dict(res="%dx%d" % (W, H), calls_each=args.rounds * args.inner, max_memory_mb=args.max_memory_mb,
                       prefilter_scratch_mib=round(info["scratch_bytes"] / 2 ** 20, 1), main_scratch_mib=round(nn.info()["scratch_bytes"] / 2 ** 20, 1))
            for k in calls:
                row[k + "_ms"] = round(float(np.median(ms[k])), 3)
                row[k + "_min_ms"] = round(float(np.min(ms[k])), 3)
                row[k + "_max_ms"] = round(float(np.max(ms[k])), 3)
            if other:
                st.synchronize()
                other.close()
            rows.append(row)
            print(json.dumps(row), flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(json.dumps(row) + "\n")
    return rows


if __name__ == "__main__":
    main()
