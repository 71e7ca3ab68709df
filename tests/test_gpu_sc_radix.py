"""GPU: sc_radix_sort_records_device / sc_radix_sort_records -- the stable LSD radix sort of records by bits of full 32-bit keys (int32,
uint32, float32; thrust::sort_by_key for keys of any value) -- against its restatement, tests/radix_ref.py: the key map in numpy and
numpy's stable argsort of the field.  Every output array, perm and keys_out are compared as raw bytes (so a NaN key never reaches
==); there is no tolerance anywhere.  torch only holds the device memory."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import radix_ref
from conftest import ROOT
from radix_ref import KEY_DTYPES, KEY_FLOAT32, KEY_INT32, KEY_UINT32

pytestmark = pytest.mark.gpu

SENT = -0x2152ACE3                                             # what every output holds before a call
KEY_TYPES = (KEY_INT32, KEY_UINT32, KEY_FLOAT32)
# struct ShadeableIntersection / struct PathSegment of the reference's src/sceneStructs.h, field for field
ISECT = np.dtype([("t", "<f4"), ("surfaceNormal", "<f4", (3,)), ("materialId", "<i4"), ("texcoord", "<f4", (2,)), ("geomId", "<i4")])
PATH = np.dtype([("origin", "<f4", (3,)), ("direction", "<f4", (3,)), ("color", "<f4", (3,)), ("pixelIndex", "<i4"), ("remainingBounces", "<i4")])
assert ISECT.itemsize == 32 and ISECT.fields["materialId"][1] == 16 and PATH.itemsize == 44 and PATH.fields["pixelIndex"][1] == 36


def _torch():
    import torch
    return torch, torch.device("cuda", 0)


class Buf:
    """`nbytes` of device memory at a 16-byte-aligned address + `shift` (0 or 4), sentinel words in front and behind (and inside)"""

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


class Workspace:
    """exactly `nbytes` (a multiple of 8) filled with 0xFF, and a guard band of 0x5A bytes behind"""
    GUARD = 64

    def __init__(self, nbytes):
        torch, dev = _torch()
        assert nbytes % 8 == 0
        self.nbytes = nbytes
        self.t = torch.full((nbytes // 8 + self.GUARD,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=dev)
        self.t[:nbytes // 8] = -1

    @property
    def ptr(self):
        return self.t.data_ptr()

    def guard_intact(self):
        return bool((self.t[self.nbytes // 8:] == 0x5A5A5A5A5A5A5A5A).all().item())


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8).reshape(-1), b.view(np.uint8).reshape(-1))


def random_bits(rng, n):
    return rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)


def records(rng, n, record_bytes):
    return rng.integers(-2 ** 31, 2 ** 31, (n, record_bytes // 4), dtype=np.int64).astype(np.int32)


def check_radix(sc, key_type, bits, arrays, descending=False, begin_bit=0, end_bit=32, shift=0, key_at=None, ws=None, stream=0,
                want_perm=True, want_keys_out=True):
    """one sc_radix_sort_records_device call on fresh sentinel-filled buffers, compared byte for byte with the restatement.
    bits: the keys' 32-bit patterns; key_at = (offset, stride): the keys are read out of the first record array.  Returns the bytes of
    everything the call wrote."""
    torch, _ = _torch()
    bits = np.ascontiguousarray(bits, np.uint32)
    n = len(bits)
    ins = [Buf(data=a, shift=shift) for a in arrays]
    outs = [Buf(a.nbytes, shift=shift) for a in arrays]
    if key_at is None:
        kbuf = Buf(data=bits)
        kptr, stride = kbuf.ptr, 4
    else:
        kptr, stride = ins[0].ptr + key_at[0], key_at[1]
    perm, kout = Buf(4 * n), Buf(4 * n)
    ws = Workspace(sc.radix_workspace_bytes(n)) if ws is None else ws
    assert ws.nbytes >= sc.radix_workspace_bytes(n)
    rb = [a.nbytes // n for a in arrays]
    b = (outs[1].ptr, ins[1].ptr, rb[1]) if len(arrays) == 2 else (0, 0, 0)
    sc.radix_sort_records_device(n, key_type, descending, begin_bit, end_bit, kptr, stride, outs[0].ptr, ins[0].ptr, rb[0], b[0], b[1], b[2],
                                 perm.ptr if want_perm else 0, kout.ptr if want_keys_out else 0, ws.ptr, stream)
    torch.cuda.synchronize()
    want = radix_ref.order(key_type, descending, bits, begin_bit, end_bit)
    got = []
    for a, o, i in zip(arrays, outs, ins):
        assert same_bytes(o.body(a), a[want])
        assert same_bytes(i.body(a), a)                         # the input is only read
        got.append(o.body(a).tobytes())
    pw, pg = perm.words_host()
    kw, kg = kout.words_host()
    assert pg and kg and ws.guard_intact()
    if want_perm:
        assert same_bytes(pw, want.astype(np.int32))
    else:
        assert np.all(pw == SENT)
    if want_keys_out:
        assert same_bytes(kw.view(np.uint32), bits[want])
    else:
        assert np.all(kw == SENT)
    return got + [pw.tobytes(), kw.tobytes()]


@pytest.fixture(scope="module")
def sc(gpu_product):
    return gpu_product.StreamCompaction()


@pytest.fixture(scope="module")
def T(sc):
    return sc.records_tile()


def float_edge_keys(rng, n=5000):
    """radix_ref's edge set (the +-0 pair, denormals, infinities, NaNs of both signs) shuffled into random floats"""
    bits = rng.standard_normal(n).astype(np.float32).view(np.uint32).copy()
    where = rng.choice(n, 4 * len(radix_ref.EDGES), replace=False)
    bits[where] = np.tile(radix_ref.EDGES, 4)
    return bits


@pytest.mark.parametrize("key_type", KEY_TYPES)
@pytest.mark.parametrize("size", ["1", "63", "64", "65", "T-1", "T", "T+1", "3*T+17", "64*T", "65*T+3"])
def test_sizes(sc, T, size, key_type):
    """1. every size around a wave and a tile, and 64 and 65 tiles (at 65 the 256-row table is 16 640 ints and crosses the scan's own
    16 384-element tile), random full-range key bits of each type, one 12-byte record array, all 32 bits."""
    n = eval(size, {"T": T})
    if size == "65*T+3":
        assert 256 * ((n + T - 1) // T) > 16384
    rng = np.random.default_rng(100 * n + key_type)
    check_radix(sc, key_type, random_bits(rng, n), [records(rng, n, 12)])


@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("key_type", KEY_TYPES)
def test_stability_and_degenerate_keys(sc, T, key_type, descending):
    """2. all keys equal (perm is arange), already sorted, reversed, only the top byte varies, only the bottom byte varies, two distinct
    values: equal keys keep input order, ascending and descending."""
    n = 3 * T + 17
    rng = np.random.default_rng(20 + key_type)
    base = random_bits(rng, n)
    in_order = base[radix_ref.order(key_type, False, base)]
    patterns = {"equal": np.full(n, 0x40490fdb, np.uint32), "sorted": in_order, "reversed": in_order[::-1].copy(),
                "top byte": (base & np.uint32(0xff000000)) | np.uint32(0x00345678), "bottom byte": (base & np.uint32(0xff)) | np.uint32(0x12345600),
                "two values": np.where(base & np.uint32(1), np.uint32(0xc0000000), np.uint32(0x00000005)).astype(np.uint32)}
    rec = records(rng, n, 12)
    for name, bits in patterns.items():
        got = check_radix(sc, key_type, bits, [rec], descending=descending)
        if name == "equal":
            assert got[1] == np.arange(n, dtype=np.int32).tobytes()


@pytest.mark.parametrize("descending", [False, True])
def test_float_order(sc, descending):
    """3. the CPU test's edge set shuffled into 5000 random floats: -0 before +0, denormals, infinities, and NaNs of both signs at the
    two ends, by payload."""
    rng = np.random.default_rng(3)
    bits = float_edge_keys(rng)
    got = check_radix(sc, KEY_FLOAT32, bits, [records(rng, len(bits), 12)], descending=descending)
    out = np.frombuffer(got[2], np.uint32)
    if descending:
        out = out[::-1]
    f = out.view(np.float32)
    nan = np.isnan(f)
    lead, trail = np.flatnonzero(~nan)[0], len(f) - 1 - np.flatnonzero(~nan)[-1]
    assert lead == trail == np.count_nonzero(nan) // 2 > 0 and np.all(out[:lead] >> 31 == 1) and np.all(out[len(f) - trail:] >> 31 == 0)
    mid = f[lead:len(f) - trail]
    assert np.all(mid[:-1] <= mid[1:]) and np.isneginf(mid[0]) and np.isposinf(mid[-1])
    z = np.flatnonzero(mid == 0)
    assert np.array_equal(np.signbit(mid[z]), np.arange(len(z)) < np.count_nonzero(np.signbit(mid[z])))      # every -0 before every +0


@pytest.mark.parametrize("key_type", KEY_TYPES)
@pytest.mark.parametrize("bit_range", [(0, 8), (8, 16), (4, 13), (24, 32), (0, 32), (0, 1), (7, 7), (0, 16), (3, 32), (32, 32), (0, 0)])
def test_bit_ranges(sc, T, key_type, bit_range):
    """4. the stable sort by the field of every range: one, two and four passes, a narrow last pass, one bit, and the empty ranges, which
    copy."""
    n = 3 * T + 17
    rng = np.random.default_rng(40 + key_type)
    rec = records(rng, n, 12)
    for descending in (False, True):
        got = check_radix(sc, key_type, random_bits(rng, n), [rec], descending=descending, begin_bit=bit_range[0], end_bit=bit_range[1])
        if bit_range[0] == bit_range[1]:
            assert got[0] == rec.tobytes() and got[1] == np.arange(n, dtype=np.int32).tobytes()


def test_low_byte_equals_the_counting_sort(sc, T):
    """4. bits [0, 8) of keys below 256 against sc_sort_records_by_key_device with nkeys = 256 on the same records: the same bytes."""
    torch, dev = _torch()
    n = 3 * T + 17
    rng = np.random.default_rng(41)
    keys = rng.integers(0, 256, n).astype(np.int32)
    rec = records(rng, n, 44)
    for descending in (False, True):
        got = check_radix(sc, KEY_INT32, keys.view(np.uint32), [rec], descending=descending, begin_bit=0, end_bit=8)
        kbuf, src, out, perm = Buf(data=keys), Buf(data=rec), Buf(rec.nbytes), Buf(4 * n)
        ws = torch.zeros((sc.records_workspace_bytes(n, 256) + 7) // 8, dtype=torch.int64, device=dev)
        sc.sort_records_by_key_device(n, 256, descending, kbuf.ptr, 4, out.ptr, src.ptr, 44, 0, 0, 0, perm.ptr, 0, ws.data_ptr())
        torch.cuda.synchronize()
        assert out.body(rec).tobytes() == got[0] and perm.words_host()[0].tobytes() == got[1]


@pytest.mark.parametrize("shift", [0, 4])
@pytest.mark.parametrize("record_bytes", [4, 12, 32, 44, 48, 256])
def test_record_shapes(sc, T, record_bytes, shift):
    """5. every record size with one and with two arrays (the second of 44 bytes, or of 48 beside the 44), from 16-byte-aligned buffers
    (the 16-byte path for 32, 48, 256) and from pointers shifted by 4 bytes (the dword path for all)."""
    n = 3 * T + 17
    rng = np.random.default_rng(500 + record_bytes + shift)
    a, b = records(rng, n, record_bytes), records(rng, n, 48 if record_bytes == 44 else 44)
    check_radix(sc, KEY_UINT32, random_bits(rng, n), [a], shift=shift)
    check_radix(sc, KEY_FLOAT32, random_bits(rng, n), [a, b], shift=shift, descending=True)


@pytest.mark.parametrize("shift", [0, 4])
def test_keys_read_out_of_the_records(sc, T, shift):
    """5. the key read out of record array a: at offset 16 with stride 32 (materialId inside a ShadeableIntersection, here shifted over a
    geom id), and at offset 36 with stride 44 (pixelIndex inside a PathSegment)."""
    n = 3 * T + 17
    rng = np.random.default_rng(55 + shift)
    isect, path = np.zeros(n, ISECT), np.zeros(n, PATH)
    isect["t"] = rng.random(n, np.float32)
    isect["materialId"] = (rng.integers(0, 40, n) << 8) | rng.integers(0, 7, n)
    isect["geomId"] = rng.integers(0, 40, n)
    path["origin"] = rng.standard_normal((n, 3)).astype(np.float32)
    path["pixelIndex"] = rng.permutation(n) * 977 - 5 * n
    check_radix(sc, KEY_INT32, isect["materialId"].view(np.uint32), [isect, path], shift=shift, key_at=(16, 32), begin_bit=0, end_bit=16)
    check_radix(sc, KEY_INT32, path["pixelIndex"].view(np.uint32), [path, isect], shift=shift, key_at=(36, 44))
    check_radix(sc, KEY_FLOAT32, isect["t"].view(np.uint32), [isect], shift=shift, key_at=(0, 32), descending=True)


def test_nothing_else_is_written(sc, T):
    """6. guard words around every output and behind the workspace (check_radix asserts them on every call of this file); d_perm and
    d_keys_out NULL one at a time and together: the other is written, the absent one's buffer keeps its sentinels."""
    n = 3 * T + 17
    rng = np.random.default_rng(6)
    a, b = records(rng, n, 44), records(rng, n, 32)
    for want_perm, want_keys_out in ((False, True), (True, False), (False, False)):
        check_radix(sc, KEY_INT32, random_bits(rng, n), [a, b], want_perm=want_perm, want_keys_out=want_keys_out)
        check_radix(sc, KEY_FLOAT32, random_bits(rng, n), [a], want_perm=want_perm, want_keys_out=want_keys_out, begin_bit=7, end_bit=7)
    out, src, perm, kout = Buf(64), Buf(64), Buf(64), Buf(64)
    sc.radix_sort_records_device(0, KEY_INT32, 0, 0, 32, src.ptr, 4, out.ptr, src.ptr + 32, 12, 0, 0, 0, perm.ptr, kout.ptr, 0)
    sc.radix_sort_records_device(0, KEY_INT32, 0, 0, 32, 0, 4, 0, 0, 12, 0, 0, 0, 0, 0, 0)            # n = 0: nothing to touch, nothing written
    _torch()[0].cuda.synchronize()
    for buf in (out, perm, kout):
        w, guards = buf.words_host()
        assert guards and np.all(w == SENT)


def test_refused_calls_enqueue_nothing(gpu_product, sc):
    """6. a refused call (bad key type, bit range, stride, record size, aliasing, workspace) raises and leaves every output untouched."""
    torch, _ = _torch()
    n = 65
    rec = np.arange(3 * n, dtype=np.int32).reshape(n, 3)
    keys, src, out, perm, kout = Buf(data=np.zeros(n, np.int32)), Buf(data=rec), Buf(rec.nbytes), Buf(4 * n), Buf(4 * n)
    ws = Workspace(sc.radix_workspace_bytes(n))

    def sort(kt=0, bb=0, eb=32, stride=4, rb=12, o=out.ptr, w=ws.ptr):
        sc.radix_sort_records_device(n, kt, 0, bb, eb, keys.ptr, stride, o, src.ptr, rb, 0, 0, 0, perm.ptr, kout.ptr, w)

    for kw in (dict(kt=3), dict(bb=9, eb=8), dict(eb=33), dict(bb=-1), dict(stride=2), dict(stride=6), dict(rb=0), dict(rb=6), dict(rb=260),
               dict(o=src.ptr), dict(w=0), dict(w=ws.ptr + 4)):
        with pytest.raises(gpu_product.PathTracerError):
            sort(**kw)
    torch.cuda.synchronize()
    for b in (out, perm, kout):
        w, guards = b.words_host()
        assert guards and np.all(w == SENT)
    sort()                                                      # and the same buffers are accepted with good arguments
    torch.cuda.synchronize()
    assert same_bytes(out.body(rec), rec) and ws.guard_intact()


def test_one_workspace_reused(sc, T):
    """7. one workspace of exactly sc_radix_workspace_bytes(big) bytes, filled with 0xFF, guard band behind: calls of different n, key
    type and bit range back to back, on the null stream and on a side stream (8.)."""
    torch, dev = _torch()
    rng = np.random.default_rng(7)
    big, small = 5 * T + 17, 65
    ws = Workspace(sc.radix_workspace_bytes(big))
    assert sc.radix_workspace_bytes(small) <= ws.nbytes
    rec = records(rng, big, 32)
    side = torch.cuda.Stream(device=dev)
    for stream in (0, side.cuda_stream):
        check_radix(sc, KEY_INT32, random_bits(rng, big), [rec], ws=ws, stream=stream)
        check_radix(sc, KEY_FLOAT32, random_bits(rng, small), [rec[:small]], ws=ws, stream=stream, descending=True)
        check_radix(sc, KEY_UINT32, random_bits(rng, T + 1), [rec[:T + 1]], ws=ws, stream=stream, begin_bit=4, end_bit=13)
        check_radix(sc, KEY_UINT32, random_bits(rng, big), [rec], ws=ws, stream=stream, begin_bit=20, end_bit=21)
        check_radix(sc, KEY_INT32, random_bits(rng, 1), [rec[:1]], ws=ws, stream=stream)
    ws.t[:ws.nbytes // 8] = -1                                  # and scribbled over again between two calls
    check_radix(sc, KEY_FLOAT32, float_edge_keys(rng), [rec[:5000]], ws=ws)


def test_two_runs_give_the_same_bytes(sc, T):
    """8. the same call twice, heavy duplicates included: every output byte equal (check_radix holds both to the one restatement, and
    the two to each other)."""
    n = 7 * T + 3
    rng = np.random.default_rng(8)
    bits = np.where(rng.random(n) < 0.5, random_bits(rng, n) & np.uint32(0x00030003), random_bits(rng, n)).astype(np.uint32)
    a, b = records(rng, n, 32), records(rng, n, 44)
    first = check_radix(sc, KEY_INT32, bits, [a, b])
    second = check_radix(sc, KEY_INT32, bits, [a, b])
    assert first == second


def test_the_counting_sort_and_partition_after_a_radix_call(sc, T):
    """9. after a radix call, sc_sort_records_by_key_device and sc_partition_records_device on the same workspace are what they were:
    one case each of tests/test_gpu_sc_records.py's checks, against numpy's stable argsort / flatnonzero."""
    torch, _ = _torch()
    n, nkeys = 3 * T + 5, 7
    rng = np.random.default_rng(9)
    ws = Workspace(sc.radix_workspace_bytes(n))
    assert sc.records_workspace_bytes(n, nkeys) <= ws.nbytes
    rec = records(rng, n, 44)
    check_radix(sc, KEY_INT32, random_bits(rng, n), [rec], ws=ws)
    keys = rng.integers(-1, nkeys + 1, n).astype(np.int32)      # (one below and one above the range: clamped)
    kbuf, src, out, perm, tot = Buf(data=keys), Buf(data=rec), Buf(rec.nbytes), Buf(4 * n), Buf(4 * nkeys)
    sc.sort_records_by_key_device(n, nkeys, 1, kbuf.ptr, 4, out.ptr, src.ptr, 44, 0, 0, 0, perm.ptr, tot.ptr, ws.ptr)
    torch.cuda.synchronize()
    mk = nkeys - 1 - np.clip(keys.astype(np.int64), 0, nkeys - 1)
    want = np.argsort(mk, kind="stable")
    assert same_bytes(out.body(rec), rec[want]) and np.array_equal(perm.words_host()[0], want.astype(np.int32))
    assert np.array_equal(tot.words_host()[0], np.bincount(mk, minlength=nkeys).astype(np.int32)) and perm.words_host()[1] and tot.words_host()[1]
    flags = ((rng.random(n) < 0.46) * rng.integers(1, 9, n)).astype(np.int32)
    fbuf, out, count = Buf(data=flags), Buf(rec.nbytes), Buf(4)
    sc.partition_records_device(n, 44, out.ptr, src.ptr, fbuf.ptr, 4, count.ptr, ws.ptr)
    torch.cuda.synchronize()
    kept, dropped = np.flatnonzero(flags != 0), np.flatnonzero(flags == 0)
    assert count.words_host()[0][0] == len(kept) and same_bytes(out.body(rec), rec[np.concatenate([kept, dropped])])
    assert ws.guard_intact()
    check_radix(sc, KEY_FLOAT32, random_bits(rng, n), [rec], ws=ws, descending=True)       # and the radix sort after them


def test_host_arrays(sc, T):
    """the host-array convenience, sc_radix_sort_records: each key type by its dtype, two arrays, a bit range, descending."""
    n = 2 * T + 9
    rng = np.random.default_rng(11)
    a, b = records(rng, n, 32).view(ISECT).reshape(n), records(rng, n, 44)
    for key_type in KEY_TYPES:
        keys = random_bits(rng, n).view(KEY_DTYPES[key_type])
        for kw in (dict(), dict(descending=True, begin_bit=5, end_bit=27)):
            (oa, ob), perm, keys_out = sc.radix_sort_records(keys, a, b, **kw)
            want = radix_ref.order(key_type, kw.get("descending", False), keys.view(np.uint32), kw.get("begin_bit", 0), kw.get("end_bit", 32))
            assert same_bytes(oa, a[want]) and same_bytes(ob, b[want]) and same_bytes(perm, want.astype(np.int32)) and same_bytes(keys_out, keys[want])
            assert keys_out.dtype == keys.dtype and sc.last_gpu_ms() > 0


def test_radix_through_the_cpp_veneer(gpu_product, tmp_path):
    """10. tests/sc_radix_check.cpp: StreamCompaction::Records::radixSortByKey (csrc/stream_compaction_api.h) for int, unsigned and float
    keys on structs of its own at sizes around the tile, against std::stable_sort."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    lib_dir = os.path.join(ROOT, "mygpuraytracer_amd")
    exe = tmp_path / "sc_radix_check"
    subprocess.check_call([hipcc, "-std=c++17", "-O1", "-Wall", "--offload-arch=gfx950", "-o", str(exe),
                           os.path.join(ROOT, "tests", "sc_radix_check.cpp"), "-L" + lib_dir, "-lmi355x_pathtracer", "-Wl,-rpath," + lib_dir])
    out = subprocess.check_output([str(exe)], text=True)
    assert "all: 0 mismatches" in out
