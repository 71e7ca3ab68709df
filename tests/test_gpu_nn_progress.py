"""GPU: the network denoiser's progress monitor (ptx_nn_set_progress; csrc/pt_nn_progress.h, pt_nn.hip).  The report sequence -- 0 first,
exactly 1 last, never decreasing, eighteen reports per tile and one for the in-place copy-out -- with the bytes of the run without a
monitor; a cancel at the first report, in the middle and on the last report, after which a host output keeps every sentinel byte and
the next call gives the uncancelled bytes; the device form, which returns only after completion."""
import numpy as np
import pytest

from conftest import beq
from test_gpu_nn_image import _blob, _gauss, _layout, _same

pytestmark = pytest.mark.gpu

NAN = float("nan")
CALLS = ["host", "images", "lightmap_hdr", "lightmap_dir"]


def _run(nn, call, rgb, out):
    if call == "host":
        out[...] = nn.host(rgb, hdr=1, input_scale=0.5)
    elif call == "images":
        nn.images_host(rgb, out, hdr=1, input_scale=0.5)
    elif call == "lightmap_hdr":
        nn.lightmap_host(rgb, out, input_scale=0.5)
    else:
        nn.lightmap_host(rgb, out, directional=True, input_scale=0.5)


class Monitor:
    def __init__(self, cancel_at=None):
        self.said, self.cancel_at = [], cancel_at

    def __call__(self, n):
        self.said.append(n)
        return self.cancel_at is None or n < self.cancel_at


def _check_sequence(said, tiles, copy_out=False):
    units = 18 * tiles + (1 if copy_out else 0)
    assert said[0] == 0.0 and said[-1] == 1.0 and len(said) == units + 1, (len(said), units)
    assert all(b > a for a, b in zip(said, said[1:]))
    assert len([n for n in said if 0 < n < 1]) >= 18 * tiles - 1 and len(said) - 1 >= 18 * tiles
    assert said[1:-1] == [k / units for k in range(1, units)]


@pytest.mark.parametrize("w,h,mb", [(33, 17, None), (289, 17, 1)])
def test_reports_and_the_bytes_of_the_run_without_a_monitor(gpu_product, w, h, mb):
    pt = gpu_product
    rgb = np.abs(_gauss(w, h, 11 + w, 2.0))
    with pt.NN(w, h, _blob(3, "narrow", 2), max_memory_mb=mb) as nn:
        t = nn.tiling(tiles=False)
        tiles = t["tiles_x"] * t["tiles_y"]
        assert tiles == (1 if mb is None else 2)
        for call in CALLS:
            want = np.full((h, w, 3), -7.0, np.float32)
            _run(nn, call, rgb, want)
            m = Monitor()
            nn.set_progress(m)
            got = np.full((h, w, 3), -7.0, np.float32)
            _run(nn, call, rgb, got)
            _check_sequence(m.said, tiles)
            assert beq(got, want), call
            if call != "host":                                     # in place: with more than one tile the copy-out is a unit of its own
                m = Monitor()
                nn.set_progress(m)
                same = rgb.copy()
                _run(nn, call, same, same)
                _check_sequence(m.said, tiles, copy_out=tiles > 1)
                assert beq(same, want), call
            nn.set_progress(None)
            again = np.full((h, w, 3), -7.0, np.float32)
            _run(nn, call, rgb, again)
            assert beq(again, want) and len(m.said) in (18 * tiles + 1, 18 * tiles + 2)      # no report after the monitor was taken off
        assert want.std() > 0


@pytest.mark.parametrize("w,h,mb", [(33, 17, None), (289, 17, 1)])
def test_cancel_leaves_the_host_output_untouched_and_the_handle_usable(gpu_product, w, h, mb):
    pt = gpu_product
    rgb = np.abs(_gauss(w, h, 21 + w, 2.0))
    with pt.NN(w, h, _blob(3, "narrow", 2), max_memory_mb=mb) as nn:
        for call in CALLS[1:]:
            want = np.full((h, w, 3), -7.0, np.float32)
            _run(nn, call, rgb, want)
            for at in (0.0, 0.5, 1.0):
                m = Monitor(cancel_at=at)
                nn.set_progress(m)
                obuf, oview = _layout(np.full((h, w, 3), -7.0, np.float32), "offset")
                with pytest.raises(pt.Cancelled, match="cancelled"):
                    _run(nn, call, rgb, oview)
                assert m.said[-1] >= at and all(n < at for n in m.said[:-1]), (call, at, m.said[-3:])
                assert (at != 0.0 or m.said == [0.0]) and (at != 1.0 or m.said[-1] == 1.0)
                assert (obuf == -7).all(), (call, at)                                  # every sentinel byte, the pixels' too
                same = rgb.copy()                                                      # in place: the colour is as it was
                m2 = Monitor(cancel_at=at)
                nn.set_progress(m2)
                with pytest.raises(pt.Cancelled):
                    _run(nn, call, same, same)
                assert beq(same, rgb), (call, at)
                nn.set_progress(None)
                got = np.full((h, w, 3), -7.0, np.float32)
                _run(nn, call, rgb, got)
                assert beq(got, want), (call, at)
        # NN.host returns a new array: the call raises before it
        nn.set_progress(Monitor(cancel_at=0.5))
        with pytest.raises(pt.Cancelled):
            nn.host(rgb)
        nn.set_progress(None)


def test_the_device_form_returns_only_after_completion(gpu_product):
    """images_device and lightmap_device on a stream with a monitor: when the call returns the last report was 1 and the result is in
    memory -- read back through another stream that does not wait for the first.  A cancel writes nothing but output channels."""
    import torch
    pt = gpu_product
    w, h = 289, 17
    rgb = np.abs(_gauss(w, h, 5, 2.0))
    with pt.NN(w, h, _blob(3, "narrow", 2), max_memory_mb=1) as nn:
        want = np.full((h, w, 3), -7.0, np.float32)
        nn.images_host(rgb, want, hdr=1, input_scale=0.5)
        lwant = np.full((h, w, 3), -7.0, np.float32)
        nn.lightmap_host(rgb, lwant, input_scale=0.5)
        stream, other = torch.cuda.Stream(device="cuda:0"), torch.cuda.Stream(device="cuda:0")
        d = torch.from_numpy(rgb).to("cuda:0")
        obuf, _ = _layout(np.full((h, w, 3), -7.0, np.float32), "x4")
        torch.cuda.synchronize()
        for lightmap, expect in ((False, want), (True, lwant)):
            o = torch.from_numpy(obuf).to("cuda:0")
            torch.cuda.synchronize()
            m = Monitor()
            nn.set_progress(m)
            color = pt.nn_image_of(d.data_ptr(), format=pt.NN_FORMAT_FLOAT3)
            out = pt.nn_image_of(o.data_ptr(), format=pt.NN_FORMAT_FLOAT3, pixel_stride=16)
            if lightmap:
                nn.lightmap_device(color, out, input_scale=0.5, stream=stream.cuda_stream)
            else:
                nn.images_device(color, out, hdr=1, input_scale=0.5, stream=stream.cuda_stream)
            assert m.said[-1] == 1.0 and len(m.said) == 37
            with torch.cuda.stream(other):                          # no wait for `stream`: the work is over
                got = o.cpu().numpy()
            assert _same(got[..., :3].copy(), expect) and (got[..., 3] == -7).all(), lightmap
            # cancelled in the middle: the alpha channel and the colour are untouched
            o2 = torch.from_numpy(obuf).to("cuda:0")
            torch.cuda.synchronize()
            m = Monitor(cancel_at=0.5)
            nn.set_progress(m)
            out2 = pt.nn_image_of(o2.data_ptr(), format=pt.NN_FORMAT_FLOAT3, pixel_stride=16)
            with pytest.raises(pt.Cancelled):
                if lightmap:
                    nn.lightmap_device(color, out2, input_scale=0.5, stream=stream.cuda_stream)
                else:
                    nn.images_device(color, out2, hdr=1, input_scale=0.5, stream=stream.cuda_stream)
            with torch.cuda.stream(other):
                got2 = o2.cpu().numpy()
            assert (got2[..., 3] == -7).all() and beq(d.cpu().numpy(), rgb)
            written = got2[..., :3] != -7
            assert (got2[..., :3][written] == expect[written]).all()                # what a finished tile wrote is the result's
            nn.set_progress(None)
        torch.cuda.synchronize()
