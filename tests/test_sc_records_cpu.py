"""CPU: the record primitives of the compaction library (sc_sort_records_by_key*, sc_partition_records*, sc_compact_records*)
as far as they go without a GPU: the argument checks, which come before the device check; no CPU fallback behind them; the
workspace size; and what the compiler made of the two kernels."""
import numpy as np
import pytest

from resource_usage import kernels_named, resource_usage

INVALID, NODEVICE = "(code 1)", "(code 4)"


@pytest.fixture(scope="module")
def sc(product):
    return product.StreamCompaction()


def test_host_conveniences_have_no_cpu_fallback(product, sc):
    """Without a device the three host-array conveniences raise PathTracerError (PTX_ERR_NODEVICE); with one they give numpy's
    stable result (the GPU tier checks them at length)."""
    rng = np.random.default_rng(0)
    n = 300
    keys = rng.integers(0, 5, n).astype(np.int32)
    rec = np.zeros(n, np.dtype([("a", "<f4", (2,)), ("id", "<i4")]))
    rec["id"] = np.arange(n)
    flags = rng.integers(0, 2, n).astype(np.int32)
    if product.load_library().ptx_device_count() < 1:
        for call in (lambda: sc.sort_records_by_key(keys, rec, nkeys=5), lambda: sc.sort_records_by_key(keys, rec, keys, nkeys=5, descending=True),
                     lambda: sc.partition_records(rec, flags), lambda: sc.compact_records(rec, flags)):
            with pytest.raises(product.PathTracerError, match=r"\(code 4\)"):
                call()
    else:
        (out,), perm, totals = sc.sort_records_by_key(keys, rec, nkeys=5)
        assert np.array_equal(perm, np.argsort(keys, kind="stable")) and np.array_equal(out["id"], perm)
        assert np.array_equal(totals, np.bincount(keys, minlength=5))
        out, kept = sc.partition_records(rec, flags)
        assert kept == flags.sum() and np.array_equal(out["id"], np.concatenate([np.flatnonzero(flags), np.flatnonzero(flags == 0)]))
        assert np.array_equal(sc.compact_records(rec, flags)["id"], np.flatnonzero(flags))


def test_refusals_come_before_the_device_check(product, sc):
    """nkeys 0 and 257, record_bytes 0, 6 and 260, stride 2, NULL and misaligned workspace, d_out == d_in: PTX_ERR_INVALID with the
    offending value in the message, device or not (made-up addresses: a refused call touches nothing)."""
    n, keys, src, out, ws = 65, 0x10000, 0x20000, 0x30000, 0x40000

    def sort(nkeys=7, rb=12, stride=4, w=ws, o=out):
        sc.sort_records_by_key_device(n, nkeys, 0, keys, stride, o, src, rb, 0, 0, 0, 0, 0, w)

    def split(fn, rb=12, stride=4, w=ws, o=out):
        fn(n, rb, o, src, keys, stride, 0x50000, w)

    bad = [(dict(nkeys=0), "nkeys = 0"), (dict(nkeys=257), "nkeys = 257"), (dict(rb=0), "record_bytes = 0"), (dict(rb=6), "record_bytes = 6"),
           (dict(rb=260), "record_bytes = 260"), (dict(stride=2), "key_stride_bytes = 2"), (dict(w=0), "null"), (dict(w=ws + 4), "d_workspace"),
           (dict(o=src), "d_out")]
    for kw, what in bad:
        with pytest.raises(product.PathTracerError, match=r"\(code 1\)") as e:
            sort(**kw)
        assert what in str(e.value)
        if "nkeys" in kw:
            continue
        for fn in (sc.partition_records_device, sc.compact_records_device):
            with pytest.raises(product.PathTracerError, match=r"\(code 1\)") as e:
                split(fn, **kw)
            assert what in str(e.value)
    with pytest.raises(product.PathTracerError, match=r"\(code 1\)"):
        sc.sort_records_by_key_device(-1, 7, 0, keys, 4, out, src, 12, 0, 0, 0, 0, 0, ws)
    with pytest.raises(product.PathTracerError, match=r"\(code 1\)"):      # a second array without a size, and with a bad one
        sc.sort_records_by_key_device(n, 7, 0, keys, 4, out, src, 12, 0x60000, 0x70000, 0, 0, 0, ws)
    with pytest.raises(product.PathTracerError, match=r"\(code 1\)"):
        sc.sort_records_by_key_device(n, 7, 0, keys, 4, out, src, 12, 0x60000, 0x70000, 46, 0, 0, ws)
    with pytest.raises(product.PathTracerError, match=r"\(code 1\)"):      # the count is not optional
        sc.partition_records_device(n, 12, out, src, keys, 4, 0, ws)
    for call in (lambda: sc.sort_records_by_key(np.zeros(4, np.int32), np.zeros((4, 3), np.int32), nkeys=0),
                 lambda: sc.sort_records_by_key(np.zeros(4, np.int32), np.zeros((4, 3), np.int32), nkeys=257),
                 lambda: sc.partition_records(np.zeros((4, 65), np.int32), np.ones(4, np.int32)),
                 lambda: sc.compact_records(np.zeros((4, 3), np.int16), np.ones(4, np.int32))):
        with pytest.raises(product.PathTracerError, match=r"\(code 1\)"):
            call()
    if product.load_library().ptx_device_count() < 1:           # after the checks: no device
        with pytest.raises(product.PathTracerError, match=r"\(code 4\)"):
            sort()


def test_workspace_size(sc):
    """records_workspace_bytes is monotone in n and in nkeys, a multiple of 8, and at least the table (one int per key and tile) plus
    the int scan's own workspace for that many elements."""
    T = sc.records_tile()
    assert T >= 64 and T % 64 == 0
    sizes = [0, 1, T - 1, T, T + 1, 3 * T + 5, 70 * T + 1, 1920 * 1080, 3840 * 2160, 2 ** 31 - 1]
    keys = [1, 2, 7, 64, 65, 256]
    grid = np.array([[sc.records_workspace_bytes(n, k) for k in keys] for n in sizes], dtype=np.int64)
    assert np.all(grid > 0) and np.all(grid % 8 == 0)
    assert np.all(np.diff(grid, axis=0) >= 0) and np.all(np.diff(grid, axis=1) >= 0)
    for i, n in enumerate(sizes):
        for j, k in enumerate(keys):
            m = k * max(1, -(-n // T))
            assert grid[i, j] >= 4 * m + sc.workspace_bytes(m)
    assert sc.records_workspace_bytes(10, 0) == 0 and sc.records_workspace_bytes(10, 257) == 0 and sc.records_workspace_bytes(-1, 7) == 0


def test_record_kernels_do_not_spill():
    """compile-only for gfx950 (`make resource-usage-records`): the two kernels use no scratch, and their LDS leaves room for at
    least four workgroups per CU."""
    usage = kernels_named(resource_usage("resource-usage-records"), ("k_records_count", "k_records_move"))
    for k, v in usage.items():
        assert v["scratch"] == 0, (k, v)
        assert v["lds"] <= 160 * 1024 // 4, (k, v)
