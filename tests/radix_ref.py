"""The restatement the radix sort of the compaction library (sc_radix_sort_records*) is held to: the order-preserving key map of
include/mi355x_stream_compaction.h in numpy, and numpy's stable argsort of the field.  Nothing here touches the library."""
import numpy as np

KEY_INT32, KEY_UINT32, KEY_FLOAT32 = 0, 1, 2
KEY_DTYPES = {KEY_INT32: np.dtype(np.int32), KEY_UINT32: np.dtype(np.uint32), KEY_FLOAT32: np.dtype(np.float32)}

INT_EDGES = np.array([0, 1, 0xffffffff, 0x80000000, 0x7fffffff, 0x7fffffff, 0x80000000, 0xffffffff], np.uint32)     # 0, +-1, INT_MIN, INT_MAX, ...
FLOAT_EDGES = np.array([0x00000000, 0x80000000,                 # +-0.0
                        0x00000001, 0x80000001,                 # +-denormal min
                        0x00800000, 0x80800000,                 # +-FLT_MIN
                        0x7f7fffff, 0xff7fffff,                 # +-FLT_MAX
                        0x7f800000, 0xff800000,                 # +-inf
                        0x7fc00000, 0x7f800001, 0x7fffffff, 0x7fc12345,         # four NaN payloads of each sign
                        0xffc00000, 0xff800001, 0xffffffff, 0xffc12345], np.uint32)
EDGES = np.concatenate([INT_EDGES, FLOAT_EDGES])


def key_bits(keys):
    """the 32 bits of every key, whatever its dtype"""
    keys = np.ascontiguousarray(keys)
    assert keys.dtype.itemsize == 4
    return keys.view(np.uint32)


def map_key(key_type, descending, bits):
    bits = np.asarray(bits, np.uint32)
    if key_type == KEY_INT32:
        u = bits ^ np.uint32(0x80000000)
    elif key_type == KEY_UINT32:
        u = bits.copy()
    else:
        u = np.where(bits >> np.uint32(31) != 0, ~bits, bits | np.uint32(0x80000000))
    return ~u if descending else u


def field(key_type, descending, bits, begin_bit=0, end_bit=32):
    u = map_key(key_type, descending, bits).astype(np.uint64)
    return (u >> np.uint64(begin_bit)) & np.uint64((1 << (end_bit - begin_bit)) - 1)


def order(key_type, descending, bits, begin_bit=0, end_bit=32):
    """perm: the source index of every output row"""
    return np.argsort(field(key_type, descending, bits, begin_bit, end_bit), kind="stable")
