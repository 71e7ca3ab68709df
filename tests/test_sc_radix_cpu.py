"""CPU: the radix sort of records by full 32-bit keys (sc_radix_sort_records*, sc_radix_map_key, sc_radix_workspace_bytes) as far as it
goes without a GPU: the order-preserving key map against its numpy restatement (tests/radix_ref.py), the argument checks, which come
before the device check, no CPU fallback behind them, the workspace size, and what the compiler made of the three kernels."""
import numpy as np
import pytest

import radix_ref
from resource_usage import kernels_named, resource_usage

KEY_TYPES = (radix_ref.KEY_INT32, radix_ref.KEY_UINT32, radix_ref.KEY_FLOAT32)


@pytest.fixture(scope="module")
def sc(product):
    return product.StreamCompaction()


def lib_map(sc, key_type, descending, bits):
    return np.array([sc.radix_map_key(key_type, descending, int(b)) for b in bits], np.uint32)


@pytest.mark.parametrize("key_type", KEY_TYPES)
def test_map_key_is_the_restatement_and_keeps_the_order(sc, key_type):
    """sc_radix_map_key on the edge set and on 10^5 random bit patterns: equal to the numpy map, ascending and descending, and for
    keys that are not NaN map(a) < map(b) exactly when numpy says a < b (every pair of the edge set, the random patterns as
    neighbours)."""
    rng = np.random.default_rng(key_type)
    bits = np.concatenate([radix_ref.EDGES, rng.integers(0, 2 ** 32, 100000, dtype=np.uint64).astype(np.uint32)])
    got = lib_map(sc, key_type, False, bits)
    assert np.array_equal(got, radix_ref.map_key(key_type, False, bits))
    assert np.array_equal(lib_map(sc, key_type, True, bits), ~got)
    assert np.array_equal(~got, radix_ref.map_key(key_type, True, bits))
    keys = bits.view(radix_ref.KEY_DTYPES[key_type])
    ok = ~np.isnan(keys) if key_type == radix_ref.KEY_FLOAT32 else np.ones(len(keys), bool)
    keys, u = keys[ok], got[ok]
    ne = int(np.count_nonzero(ok[:len(radix_ref.EDGES)]))
    a, b = np.meshgrid(np.arange(ne), np.arange(ne))           # every pair of the edge set, and the random patterns as neighbours
    a, b = np.concatenate([a.ravel(), np.arange(ne, len(keys) - 1)]), np.concatenate([b.ravel(), np.arange(ne + 1, len(keys))])
    # (-0.0 and +0.0 are one number to numpy and two keys to the map, -0 first: test_float_total_order; no other pair is left out)
    zeros = (keys[a] == 0) & (keys[b] == 0)
    assert np.array_equal((u[a] < u[b])[~zeros], (keys[a] < keys[b])[~zeros])
    assert np.array_equal((u[b] < u[a])[~zeros], (keys[b] < keys[a])[~zeros])


def test_float_total_order(sc):
    """negative NaNs < -inf < -FLT_MAX < -FLT_MIN < -denormal < -0 < +0 < +denormal < +FLT_MIN < +FLT_MAX < +inf < positive NaNs, the
    NaNs by payload."""
    chain = [0xffffffff, 0xffc12345, 0xffc00000, 0xff800001, 0xff800000, 0xff7fffff, 0x80800000, 0x80000001, 0x80000000,
             0x00000000, 0x00000001, 0x00800000, 0x7f7fffff, 0x7f800000, 0x7f800001, 0x7fc00000, 0x7fc12345, 0x7fffffff]
    assert sorted(chain) != chain and set(chain) == set(radix_ref.FLOAT_EDGES.tolist())
    u = [sc.radix_map_key(radix_ref.KEY_FLOAT32, False, b) for b in chain]
    assert all(x < y for x, y in zip(u[:-1], u[1:])), u
    d = [sc.radix_map_key(radix_ref.KEY_FLOAT32, True, b) for b in chain]
    assert all(x > y for x, y in zip(d[:-1], d[1:])), d


def test_refusals_come_before_the_device_check(product, sc):
    """bad key_type, begin_bit > end_bit and bits outside 0..32, stride 2 and 6, record_bytes 0, 6 and 260, an output that is an input,
    a misaligned workspace, null pointers with n > 0: PTX_ERR_INVALID with the argument's name in the message, device or not (made-up
    addresses: a refused call touches nothing); with good arguments and no device, PTX_ERR_NODEVICE."""
    n, keys, src, out, ws = 65, 0x10000, 0x20000, 0x30000, 0x40000

    def sort(n=n, kt=0, bb=0, eb=32, k=keys, stride=4, o=out, s=src, rb=12, ob=0, sb=0, rbb=0, perm=0, kout=0, w=ws):
        sc.radix_sort_records_device(n, kt, 0, bb, eb, k, stride, o, s, rb, ob, sb, rbb, perm, kout, w)

    bad = [(dict(kt=3), "key_type = 3"), (dict(kt=-1), "key_type = -1"), (dict(bb=9, eb=8), "begin_bit = 9"), (dict(bb=-1), "begin_bit = -1"),
           (dict(eb=33), "end_bit = 33"), (dict(bb=33, eb=33), "begin_bit = 33"), (dict(stride=2), "key_stride_bytes = 2"),
           (dict(stride=6), "key_stride_bytes = 6"), (dict(rb=0), "record_bytes = 0"), (dict(rb=6), "record_bytes = 6"),
           (dict(rb=260), "record_bytes = 260"), (dict(ob=0x60000, sb=0x70000, rbb=6), "record_bytes_b = 6"),
           (dict(ob=0x60000, sb=0x70000, rbb=0), "record_bytes_b = 0"), (dict(o=src), "d_out"), (dict(ob=src, sb=0x70000, rbb=12), "d_out"),
           (dict(kout=keys), "d_keys_out"), (dict(perm=out), "d_perm"), (dict(w=ws + 4), "d_workspace"), (dict(w=0), "null"),
           (dict(k=0), "null"), (dict(o=0), "null"), (dict(s=0), "null"), (dict(ob=0x60000, sb=0, rbb=12), "null"), (dict(n=-1), "n = -1"),
           (dict(k=keys + 2), "4-byte aligned")]
    for kw, what in bad:
        with pytest.raises(product.PathTracerError, match=r"\(code 1\)") as e:
            sort(**kw)
        assert what in str(e.value), (kw, str(e.value))
    z = np.zeros((4, 3), np.int32)
    for call in (lambda: sc.radix_sort_records(np.zeros(4, np.int32), z, begin_bit=5, end_bit=4),
                 lambda: sc.radix_sort_records(np.zeros(4, np.int32), z, end_bit=40),
                 lambda: sc.radix_sort_records(np.zeros(4, np.int32), z, key_type=7),
                 lambda: sc.radix_sort_records(np.zeros(4, np.float32), np.zeros((4, 65), np.int32)),
                 lambda: sc.radix_sort_records(np.zeros(4, np.uint32), np.zeros((4, 3), np.int16))):
        with pytest.raises(product.PathTracerError, match=r"\(code 1\)"):
            call()
    for keys_of_another_type in (np.zeros(4, np.int64), np.zeros(4, np.float64), np.zeros(4, np.int16)):
        with pytest.raises(product.PathTracerError, match="int32, uint32 or float32"):
            sc.radix_sort_records(keys_of_another_type, z)
    if product.load_library().ptx_device_count() < 1:           # after the checks: no device
        with pytest.raises(product.PathTracerError, match=r"\(code 4\)"):
            sort()
        with pytest.raises(product.PathTracerError, match=r"\(code 4\)"):
            sort(bb=7, eb=7)


def test_host_convenience_has_no_cpu_fallback(product, sc):
    """Without a device sc_radix_sort_records raises PTX_ERR_NODEVICE; with one it gives the restatement's stable result."""
    rng = np.random.default_rng(0)
    n = 300
    keys = rng.standard_normal(n).astype(np.float32)
    rec = np.zeros(n, np.dtype([("a", "<f4", (2,)), ("id", "<i4")]))
    rec["id"] = np.arange(n)
    if product.load_library().ptx_device_count() < 1:
        for call in (lambda: sc.radix_sort_records(keys, rec), lambda: sc.radix_sort_records(keys, rec, keys, descending=True, begin_bit=3, end_bit=9)):
            with pytest.raises(product.PathTracerError, match=r"\(code 4\)"):
                call()
    else:
        (out,), perm, keys_out = sc.radix_sort_records(keys, rec)
        want = radix_ref.order(radix_ref.KEY_FLOAT32, False, radix_ref.key_bits(keys))
        assert np.array_equal(perm, want) and np.array_equal(out["id"], want) and np.array_equal(keys_out.view(np.uint32), keys[want].view(np.uint32))


def test_workspace_size(sc):
    """radix_workspace_bytes is 0 for negative n, monotone in n, a multiple of 8, and holds two (u, index) pair buffers, the 256-row
    table and the int scan's own workspace for it."""
    T = sc.records_tile()
    sizes = [0, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 17, 64 * T, 65 * T + 3, 1920 * 1080, 3840 * 2160, 2 ** 31 - 1]
    got = np.array([sc.radix_workspace_bytes(n) for n in sizes], dtype=np.int64)
    assert np.all(got > 0) and np.all(got % 8 == 0) and np.all(np.diff(got) >= 0)
    for n, b in zip(sizes, got):
        m = 256 * max(1, -(-n // T))
        assert b >= 16 * n + 4 * m + sc.workspace_bytes(m)
    assert sc.radix_workspace_bytes(-1) == 0 and sc.radix_workspace_bytes(-2 ** 31) == 0


def test_radix_kernels_do_not_spill():
    """compile-only for gfx950 (`make resource-usage-radix`): the three kernels use no scratch, and their LDS leaves room for at least
    four workgroups per CU."""
    usage = kernels_named(resource_usage("resource-usage-radix"), ("k_radix_count", "k_radix_move", "k_radix_gather"))
    for k, v in usage.items():
        assert v["scratch"] == 0, (k, v)
        assert v["lds"] <= 160 * 1024 // 4, (k, v)
