"""GPU: the record primitives of the compaction library -- sc_sort_records_by_key_device, sc_partition_records_device,
sc_compact_records_device (thrust::sort_by_key(.., sortByMaterial()) and thrust::stable_partition(.., isTerminate()) of the
reference's src/pathtrace.cu:418-428, 518, 541) -- against numpy's stable argsort / flatnonzero.  Every result is an integer
permutation, so every comparison is array_equal; torch only holds the device memory."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT, golden

pytestmark = pytest.mark.gpu

SENT = -0x2152ACE3                                             # what every output holds before a call
INT_MIN = -2 ** 31
# struct ShadeableIntersection / struct PathSegment of the reference's src/sceneStructs.h, field for field
ISECT = np.dtype([("t", "<f4"), ("surfaceNormal", "<f4", (3,)), ("materialId", "<i4"), ("texcoord", "<f4", (2,)), ("geomId", "<i4")])
PATH = np.dtype([("origin", "<f4", (3,)), ("direction", "<f4", (3,)), ("color", "<f4", (3,)), ("pixelIndex", "<i4"), ("remainingBounces", "<i4")])
assert ISECT.itemsize == 32 and ISECT.fields["materialId"][1] == 16
assert PATH.itemsize == 44 and PATH.fields["remainingBounces"][1] == 40


def _torch():
    import torch
    return torch, torch.device("cuda", 0)


class Buf:
    """`nbytes` of device memory at a 16-byte-aligned address + `shift` (0 or 4), sentinel words in front, behind and inside"""

    def __init__(self, nbytes=0, data=None, shift=0):
        torch, dev = _torch()
        if data is not None:
            nbytes = data.nbytes
        self.words, self.off = nbytes // 4, 4 + shift // 4
        self.t = torch.full((self.words + 12,), SENT, dtype=torch.int32, device=dev)
        assert self.t.data_ptr() % 16 == 0
        if data is not None and nbytes:
            self.t[self.off:self.off + self.words].copy_(torch.from_numpy(np.frombuffer(np.ascontiguousarray(data).tobytes(), np.int32).copy()))

    @property
    def ptr(self):
        return self.t.data_ptr() + 4 * self.off

    def words_host(self):
        """(the body's words, True if every word around the body is still the sentinel)"""
        h = self.t.cpu().numpy()
        return h[self.off:self.off + self.words], bool(np.all(h[:self.off] == SENT) and np.all(h[self.off + self.words:] == SENT))

    def body(self, like):
        w, guards = self.words_host()
        assert guards, "a word outside the buffer was written"
        return np.frombuffer(w.tobytes(), like.dtype).reshape(like.shape)


def workspace(sc, n, nkeys):
    """a workspace with arbitrary contents"""
    torch, dev = _torch()
    return torch.full(((sc.records_workspace_bytes(n, nkeys) + 7) // 8,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=dev)


def mapped_keys(keys, nkeys, descending):
    k = np.clip(np.asarray(keys, np.int64), 0, nkeys - 1)
    return nkeys - 1 - k if descending else k


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8).reshape(-1), b.view(np.uint8).reshape(-1))


def check_sort(sc, keys, arrays, nkeys, descending, shift=0, key_field=None, ws=None, stream=0, outputs=True):
    """one sc_sort_records_by_key_device call on fresh sentinel-filled buffers, compared with numpy's stable argsort"""
    torch, _ = _torch()
    n = len(keys)
    ins = [Buf(data=a, shift=shift) for a in arrays]
    outs = [Buf(a.nbytes, shift=shift) for a in arrays]
    if key_field is None:
        kbuf = Buf(data=np.asarray(keys, np.int32))
        kptr, stride = kbuf.ptr, 4
    else:                                                       # the key is a field of the first record array
        kptr, stride = ins[0].ptr + arrays[0].dtype.fields[key_field][1], arrays[0].dtype.itemsize
    perm, tot = Buf(4 * n), Buf(4 * nkeys)
    ws = workspace(sc, n, nkeys) if ws is None else ws
    rb = [a.nbytes // n for a in arrays]
    b = (outs[1].ptr, ins[1].ptr, rb[1]) if len(arrays) == 2 else (0, 0, 0)
    sc.sort_records_by_key_device(n, nkeys, descending, kptr, stride, outs[0].ptr, ins[0].ptr, rb[0], b[0], b[1], b[2],
                                  perm.ptr if outputs else 0, tot.ptr if outputs else 0, ws.data_ptr(), stream)
    torch.cuda.synchronize()
    mk = mapped_keys(keys, nkeys, descending)
    want = np.argsort(mk, kind="stable")
    for a, o, i in zip(arrays, outs, ins):
        assert same_bytes(o.body(a), a[want])
        assert same_bytes(i.body(a), a)                         # the input is only read
    pw, pg = perm.words_host()
    tw, tg = tot.words_host()
    assert pg and tg
    if outputs:
        assert np.array_equal(pw, want.astype(np.int32))
        assert np.array_equal(tw, np.bincount(mk, minlength=nkeys).astype(np.int32))
    else:
        assert np.all(pw == SENT) and np.all(tw == SENT)


def check_split(sc, records, flags, compact, shift=0, flag_field=None, ws=None, stream=0):
    """one sc_partition_records_device / sc_compact_records_device call, compared with numpy"""
    torch, _ = _torch()
    n = len(flags)
    src, out, count = Buf(data=records, shift=shift), Buf(records.nbytes, shift=shift), Buf(4)
    if flag_field is None:
        fbuf = Buf(data=np.asarray(flags, np.int32))
        fptr, stride = fbuf.ptr, 4
    else:
        fptr, stride = src.ptr + records.dtype.fields[flag_field][1], records.dtype.itemsize
    ws = workspace(sc, n, 2) if ws is None else ws
    fn = sc.compact_records_device if compact else sc.partition_records_device
    fn(n, records.nbytes // n, out.ptr, src.ptr, fptr, stride, count.ptr, ws.data_ptr(), stream)
    torch.cuda.synchronize()
    f = np.asarray(flags)
    kept, dropped = np.flatnonzero(f != 0), np.flatnonzero(f == 0)
    cw, cg = count.words_host()
    assert cg and cw[0] == len(kept)
    got = out.body(records)
    if compact:
        assert same_bytes(got[:len(kept)], records[kept])
        rest = np.ascontiguousarray(got[len(kept):]).view(np.int32)
        assert np.all(rest == SENT)                             # nothing at or after count
    else:
        assert same_bytes(got, records[np.concatenate([kept, dropped])])


def key_patterns(rng, n, nkeys):
    u = rng.integers(0, nkeys, n).astype(np.int32)
    last = np.zeros(n, np.int32)
    last[-1:] = nkeys - 1
    return {"uniform": u, "equal": np.full(n, nkeys // 2, np.int32), "sorted": np.sort(u), "reverse": np.sort(u)[::-1].copy(),
            "only the last key": np.full(n, nkeys - 1, np.int32), "the last key once, at the end": last}


@pytest.fixture(scope="module")
def sc(gpu_product):
    return gpu_product.StreamCompaction()


@pytest.fixture(scope="module")
def T(sc):
    return sc.records_tile()


@pytest.mark.parametrize("nkeys", [1, 2, 7, 64, 65, 256])
@pytest.mark.parametrize("size", ["1", "63", "64", "65", "T-1", "T", "T+1", "3*T+5"])
def test_sizes_and_keys(sc, T, size, nkeys):
    """1. every size around a wave and a tile x every key count around a wave of keys, six key patterns, both directions, one
    12-byte record array: the permuted records, d_perm and d_key_totals."""
    n = eval(size, {"T": T})
    rng = np.random.default_rng(1000 * nkeys + n)
    rec = rng.integers(-2 ** 31, 2 ** 31, (n, 3), dtype=np.int64).astype(np.int32)
    for name, keys in key_patterns(rng, n, nkeys).items():
        for descending in (False, True):
            check_sort(sc, keys, [rec], nkeys, descending)


def test_the_scan_inside_crosses_its_own_tile(sc, T):
    """2. nkeys = 256, n = 70 T + 1: a table of 71 x 256 = 18 176 entries, more than the scan's 16 384-element tile (and, tile for
    tile, more than its look-back window of 64 would cover in one step)."""
    n, nkeys = 70 * T + 1, 256
    assert nkeys * ((n + T - 1) // T) > 16384
    rng = np.random.default_rng(2)
    rec = rng.integers(0, 2 ** 31, (n, 3), dtype=np.int64).astype(np.int32)
    check_sort(sc, rng.integers(0, nkeys, n).astype(np.int32), [rec], nkeys, False)
    check_sort(sc, rng.integers(0, nkeys, n).astype(np.int32), [rec], nkeys, True)


@pytest.mark.parametrize("shift", [0, 4])
@pytest.mark.parametrize("record_bytes", [4, 12, 32, 44, 48, 256])
def test_record_shapes(sc, T, record_bytes, shift):
    """3. every record size from 16-byte-aligned buffers (the 16-byte path for 32, 48, 256) and from views shifted by 4 bytes (the
    dword path for all): sort, partition and compaction."""
    n = 3 * T + 5
    rng = np.random.default_rng(record_bytes + shift)
    rec = rng.integers(-2 ** 31, 2 ** 31, (n, record_bytes // 4), dtype=np.int64).astype(np.int32)
    check_sort(sc, rng.integers(0, 7, n).astype(np.int32), [rec], 7, True, shift=shift)
    flags = (rng.random(n) < 0.46) * rng.integers(1, 9, n)
    check_split(sc, rec, flags, compact=False, shift=shift)
    check_split(sc, rec, flags, compact=True, shift=shift)


def bounce_records(rng, n, materials):
    isect, path = np.zeros(n, ISECT), np.zeros(n, PATH)
    isect["t"] = rng.random(n, np.float32)
    isect["surfaceNormal"] = rng.standard_normal((n, 3)).astype(np.float32)
    isect["materialId"] = rng.integers(0, materials, n)
    isect["texcoord"] = rng.random((n, 2), np.float32)
    isect["geomId"] = rng.integers(0, 40, n)
    for f in ("origin", "direction", "color"):
        path[f] = rng.standard_normal((n, 3)).astype(np.float32)
    path["pixelIndex"] = rng.permutation(n)
    path["remainingBounces"] = (rng.random(n) < 0.46) * rng.integers(1, 8, n)
    return isect, path


@pytest.mark.parametrize("shift", [0, 4])
def test_keys_and_flags_read_out_of_the_records(sc, T, shift):
    """3. two arrays in one call (32-byte ShadeableIntersection + 44-byte PathSegment) with the key read out of the first at
    materialId's offset and stride; partition with the flag read at remainingBounces' offset inside the 44-byte records."""
    n = 3 * T + 5
    isect, path = bounce_records(np.random.default_rng(3 + shift), n, 7)
    check_sort(sc, isect["materialId"], [isect, path], 7, True, shift=shift, key_field="materialId")
    check_split(sc, path, path["remainingBounces"], compact=False, shift=shift, flag_field="remainingBounces")
    check_split(sc, path, path["remainingBounces"], compact=True, shift=shift, flag_field="remainingBounces")


def test_nothing_else_is_written(sc, T):
    """4. sentinel-filled outputs: compaction leaves everything from count on untouched, partition and sort write exactly n records
    and the guard words around every buffer survive (check_sort / check_split assert both on every call of this file); d_perm = NULL
    and d_key_totals = NULL are accepted."""
    n = 3 * T + 5
    rng = np.random.default_rng(4)
    rec = rng.integers(0, 2 ** 31, (n, 11), dtype=np.int64).astype(np.int32)
    check_sort(sc, rng.integers(0, 64, n).astype(np.int32), [rec], 64, False, outputs=False)
    for frac in (0.46, 0.001, 0.999):
        flags = (rng.random(n) < frac).astype(np.int32)
        check_split(sc, rec, flags, compact=True)
        check_split(sc, rec, flags, compact=False)


@pytest.mark.parametrize("nkeys", [1, 7, 256])
def test_out_of_range_keys_are_clamped(sc, T, nkeys):
    """5. keys of -1, nkeys, nkeys + 5 and INT_MIN among random ones: the result of the clamped keys, no HIP error."""
    torch, _ = _torch()
    n = 3 * T + 5
    rng = np.random.default_rng(5 + nkeys)
    keys = rng.integers(0, nkeys, n).astype(np.int64)
    bad = rng.choice(n, n // 3, replace=False)
    keys[bad] = rng.choice([-1, nkeys, nkeys + 5, INT_MIN, 2 ** 31 - 1], len(bad))
    rec = rng.integers(0, 2 ** 31, (n, 3), dtype=np.int64).astype(np.int32)
    for descending in (False, True):
        check_sort(sc, keys.astype(np.int32), [rec], nkeys, descending)
    torch.cuda.synchronize()                                   # raises if a kernel faulted


def test_one_workspace_reused(sc, T):
    """6. one workspace back to back: n = 3T+5 with 64 keys, then n = 65 with 2 keys (the stale table must not matter), then a side
    stream; afterwards the int scan_device / compact_device on the same workspace are still exact."""
    torch, dev = _torch()
    rng = np.random.default_rng(6)
    big, small = 3 * T + 5, 65
    ws = workspace(sc, big, 64)
    assert sc.records_workspace_bytes(small, 2) <= sc.records_workspace_bytes(big, 64)
    rec = rng.integers(0, 2 ** 31, (big, 3), dtype=np.int64).astype(np.int32)
    side = torch.cuda.Stream(device=dev)
    for stream in (0, side.cuda_stream):
        check_sort(sc, rng.integers(0, 64, big).astype(np.int32), [rec], 64, True, ws=ws, stream=stream)
        check_sort(sc, rng.integers(0, 2, small).astype(np.int32), [rec[:small]], 2, False, ws=ws, stream=stream)
        check_split(sc, rec[:small], rng.integers(0, 2, small), compact=False, ws=ws, stream=stream)
        check_split(sc, rec, rng.integers(0, 2, big), compact=True, ws=ws, stream=stream)
    m = big
    assert sc.workspace_bytes(m) <= ws.numel() * 8
    a = (rng.integers(-4, 9, m) * (rng.random(m) < 0.4)).astype(np.int32)
    d_in, d_out, count = torch.from_numpy(a).to(dev), torch.zeros(m, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    sc.scan_device(m, d_out.data_ptr(), d_in.data_ptr(), ws.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(d_out.cpu().numpy(), np.concatenate([[0], np.cumsum(a, dtype=np.int64)[:-1]]).astype(np.int32))
    sc.compact_device(m, d_out.data_ptr(), d_in.data_ptr(), count.data_ptr(), ws.data_ptr())
    torch.cuda.synchronize()
    k = int(count.item())
    assert k == np.count_nonzero(a) and np.array_equal(d_out.cpu().numpy()[:k], a[a != 0])


def test_degenerate(sc, T):
    """7. n = 0 gives count and totals 0 and nothing else; all-kept and none-kept partitions."""
    torch, _ = _torch()
    ws = workspace(sc, 0, 7)
    out, src, tot, count, perm = Buf(64), Buf(64), Buf(4 * 7), Buf(4), Buf(64)
    sc.sort_records_by_key_device(0, 7, 1, src.ptr, 4, out.ptr, src.ptr + 32, 12, 0, 0, 0, perm.ptr, tot.ptr, ws.data_ptr())
    sc.partition_records_device(0, 12, out.ptr, src.ptr, src.ptr, 4, count.ptr, ws.data_ptr())
    torch.cuda.synchronize()
    assert np.all(tot.words_host()[0] == 0) and tot.words_host()[1] and count.words_host()[0][0] == 0
    count = Buf(4)
    sc.compact_records_device(0, 12, out.ptr, src.ptr, src.ptr, 4, count.ptr, ws.data_ptr())
    sc.sort_records_by_key_device(0, 7, 0, 0, 4, 0, 0, 12, 0, 0, 0, 0, 0, 0)          # nothing to touch, nothing to write
    torch.cuda.synchronize()
    assert count.words_host()[0][0] == 0
    assert np.all(out.words_host()[0] == SENT) and np.all(perm.words_host()[0] == SENT)
    n = T + 1
    rec = np.arange(3 * n, dtype=np.int32).reshape(n, 3)
    for flags in (np.full(n, 5, np.int32), np.zeros(n, np.int32), np.full(n, INT_MIN, np.int32)):
        check_split(sc, rec, flags, compact=False)
        check_split(sc, rec, flags, compact=True)


def test_refused_calls_enqueue_nothing(gpu_product, sc, T):
    """7. nkeys 0 and 257, record_bytes 0, 6 and 260, stride 2, NULL and misaligned workspace, d_out == d_in: PathTracerError, and
    every output is still the sentinel."""
    torch, _ = _torch()
    n = 65
    rec = np.arange(3 * n, dtype=np.int32).reshape(n, 3)
    keys = Buf(data=np.zeros(n, np.int32))
    src, out, perm, tot, count = Buf(data=rec), Buf(rec.nbytes), Buf(4 * n), Buf(4 * 256), Buf(4)
    ws = workspace(sc, n, 256)

    def sort(nkeys=7, rb=12, stride=4, w=ws.data_ptr(), o=out.ptr):
        sc.sort_records_by_key_device(n, nkeys, 0, keys.ptr, stride, o, src.ptr, rb, 0, 0, 0, perm.ptr, tot.ptr, w)

    def split(fn, rb=12, stride=4, w=ws.data_ptr(), o=out.ptr):
        fn(n, rb, o, src.ptr, keys.ptr, stride, count.ptr, w)

    bad = [dict(nkeys=0), dict(nkeys=257), dict(rb=0), dict(rb=6), dict(rb=260), dict(stride=2), dict(w=0), dict(w=ws.data_ptr() + 4),
           dict(o=src.ptr)]
    for kw in bad:
        with pytest.raises(gpu_product.PathTracerError):
            sort(**kw)
        for fn in (sc.partition_records_device, sc.compact_records_device):
            if "nkeys" in kw:
                continue
            with pytest.raises(gpu_product.PathTracerError):
                split(fn, **kw)
    with pytest.raises(gpu_product.PathTracerError):            # a second array without its size
        sc.sort_records_by_key_device(n, 7, 0, keys.ptr, 4, out.ptr, src.ptr, 12, perm.ptr, src.ptr, 0, 0, 0, ws.data_ptr())
    torch.cuda.synchronize()
    for b in (out, perm, tot, count):
        w, guards = b.words_host()
        assert guards and np.all(w == SENT)
    assert same_bytes(src.body(rec), rec)
    sort()                                                      # and the same buffers are accepted with good arguments
    torch.cuda.synchronize()
    assert same_bytes(out.body(rec), rec)


def test_one_reference_bounce_tail(sc, T):
    """8. the sequence src/pathtrace.cu:518,541 runs, through the host-array conveniences: sort_records_by_key(descending, nkeys =
    materials) of 32-byte / 44-byte record pairs, then partition_records (and compact_records) of the result by remainingBounces --
    against numpy doing the same two stable steps.

    The committed tests/golden/render_*.npz fixtures hold, per bounce, the pixel index and material id of every path in the
    order AFTER the reference's sort (stream_pix_b*, stream_mat_b*).  Before bounce 0's sort the paths are in pixel order, so that
    bounce carries both sides: the material ids before the sort are stream_mat_b0 scattered to stream_pix_b0, and the permutation
    the sort must find is stream_pix_b0 itself.  Those are fed as well (configs 3 and 4, which sort)."""
    materials, n = 7, 3 * T + 5
    isect, path = bounce_records(np.random.default_rng(8), n, materials)
    (s_isect, s_path), perm, totals = sc.sort_records_by_key(isect["materialId"], isect, path, nkeys=materials, descending=True)
    order = np.argsort(materials - 1 - isect["materialId"], kind="stable")
    assert same_bytes(s_isect, isect[order]) and same_bytes(s_path, path[order]) and np.array_equal(perm, order)
    assert np.array_equal(totals, np.bincount(isect["materialId"], minlength=materials)[::-1])
    parted, live = sc.partition_records(s_path, s_path["remainingBounces"])
    rb = path[order]["remainingBounces"]
    want = path[order][np.concatenate([np.flatnonzero(rb != 0), np.flatnonzero(rb == 0)])]
    assert live == np.count_nonzero(rb) and same_bytes(parted, want)
    assert same_bytes(sc.compact_records(s_path, s_path["remainingBounces"]), want[:live])

    for name in ("render_c4_obj.npz", "render_c3_glass.npz"):
        g = golden(name)
        pix, mat = g["stream_pix_b0"], g["stream_mat_b0"]
        before = np.empty_like(mat)
        before[pix] = mat
        nk = int(mat.max()) + 1
        (s_mat, s_pix), perm, totals = sc.sort_records_by_key(before, before, np.arange(len(pix), dtype=np.int32), nkeys=nk, descending=True)
        assert np.array_equal(s_mat, mat) and np.array_equal(s_pix, pix) and np.array_equal(perm, pix)


def test_records_through_the_cpp_veneer(gpu_product, tmp_path):
    """9. tests/sc_records_check.cpp: StreamCompaction::Records::sortByKey / stablePartition / compact (csrc/stream_compaction_api.h)
    on a struct of its own at sizes around the tile, against std::stable_sort / std::stable_partition."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    lib_dir = os.path.join(ROOT, "mygpuraytracer_amd")
    exe = tmp_path / "sc_records_check"
    subprocess.check_call([hipcc, "-std=c++17", "-O1", "-Wall", "--offload-arch=gfx950", "-o", str(exe),
                           os.path.join(ROOT, "tests", "sc_records_check.cpp"), "-L" + lib_dir, "-lmi355x_pathtracer", "-Wl,-rpath," + lib_dir])
    out = subprocess.check_output([str(exe)], text=True)
    assert "all: 0 mismatches" in out
