"""The network denoiser's image descriptor restated (include/mi355x_pathtracer.h, "images"; csrc/pt_nn_image.h / .hip), for its tests.

    typedef struct ptx_nn_image {
        const void *ptr;        /* NULL: no such image */
        int    format;          /* PTX_NN_FORMAT_FLOAT3 = 1, PTX_NN_FORMAT_HALF3 = 2 */
        size_t byte_offset;     /* of pixel (0,0) from ptr */
        size_t pixel_stride;    /* bytes; 0 = the pixel's size (12 / 6) */
        size_t row_stride;      /* bytes; 0 = width * pixel_stride */
    } ptx_nn_image;

Channel c of pixel (x, y) is the `size` bytes at ptr + byte_offset + y * row_stride + x * pixel_stride + c * size, size = 4 or 2.  No
other byte is written.  Here a descriptor is (ptr, format, byte_offset, pixel_stride, row_stride) with ptr an integer, and memory is
a numpy uint8 array whose first byte stands at address `origin`."""
import numpy as np

FLOAT3, HALF3 = 1, 2
SIZE = {FLOAT3: 4, HALF3: 2}
DTYPE = {FLOAT3: np.float32, HALF3: np.float16}
RULES = ("unknown format", "below the pixel's size", "below width * pixel stride", "not a multiple of the pixel stride",
         "not a multiple of the channel size")


def view(desc, width):
    """(base, pixel_stride, row_stride, size) with the defaults filled in"""
    ptr, fmt, off, ps, rs = desc
    size = SIZE[fmt]
    ps = ps or 3 * size
    return ptr + off, ps, rs or width * ps, size


def problem(desc, width, height):
    """None, or the rule of RULES that refuses the descriptor, in the header's order"""
    if desc[1] not in SIZE:
        return RULES[0]
    base, ps, rs, size = view(desc, width)
    if ps < 3 * size:
        return RULES[1]
    if rs < width * ps:
        return RULES[2]
    if rs % ps:
        return RULES[3]
    if base % size or ps % size or rs % size:
        return RULES[4]
    return None


def address(desc, width, x, y, c):
    base, ps, rs, size = view(desc, width)
    return base + y * rs + x * ps + c * size


def interval(desc, width, height):
    """[lo, hi): the first channel byte of (0, 0) to the last channel byte of (W - 1, H - 1), + 1"""
    return address(desc, width, 0, 0, 0), address(desc, width, width - 1, height - 1, 2) + SIZE[desc[1]]


def meet(a, b):
    return a[0] < b[1] and b[0] < a[1]


def _index(desc, width, height, origin):
    """(H, W, 3) element indices into memory seen as the format's dtype (aligned by the rules)"""
    base, ps, rs, size = view(desc, width)
    y, x, c = np.meshgrid(np.arange(height), np.arange(width), np.arange(3), indexing="ij")
    byte = base - origin + y * rs + x * ps + c * size
    assert (byte % size == 0).all()
    return byte // size


def read(memory, origin, desc, width, height):
    """the image's pixels widened exactly to float32, (H, W, 3)"""
    return memory.view(DTYPE[desc[1]])[_index(desc, width, height, origin)].astype(np.float32)


def to_half(v):
    """fp16_rne(min(v, 65504)), numpy's own statement of it"""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.minimum(np.asarray(v, np.float32), np.float32(65504)).astype(np.float16)


def write(memory, origin, desc, width, height, values):
    """memory with the image's pixels replaced by `values` ((H, W, 3) float32) -- a half image by to_half -- and every other byte kept"""
    out = memory.copy()
    flat = out.view(DTYPE[desc[1]])
    flat[_index(desc, width, height, origin)] = values if desc[1] == FLOAT3 else to_half(values)
    return out
