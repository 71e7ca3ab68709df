"""The network denoiser's tile plan restated (include/mi355x_pathtracer.h, "Tiles"; csrc/pt_nn_tiles.h), for its tests
(tests/test_nn_tiles_cpu.py, tests/test_gpu_nn_tiles.py).  The rule and the tiles are written from the definition, with the scratch of
a tile taken from a function of the caller's (the tests hand in the library's own figure for one tile, and scratch_model below, which
restates that figure too); tiled_unet runs tests/unet_ref.py's network window by window and pastes the kept rectangles together."""
import numpy as np

import unet_ref as U

ALIGN, OVERLAP, MIN_TILE, MAX_TILE_W, MAX_TILE_H, MAX_FRAME = 16, 96, 288, 7680, 4320, 16384
POOLED = (1, 2, 3, 4)                                      # enc_conv1 .. 4 write only their pooled output
PLACE = (3, 0, 1, 2, 3, 4, 3, 4, 3, 4, 3, 4, 3, 4, 3, 4)   # 0 .. 2: the skips, each in its own place; 3 / 4: the two arenas

pad16 = lambda v: (v + 15) // 16 * 16
align256 = lambda v: (v + 255) // 256 * 256
ceil_div = lambda a, b: -(-a // b)


def scratch_model(couts, w, h):
    """bytes of the activations of one w x h tile, from the sixteen layers' output channel counts: the fp16 input (16 channels), the
    three skips, and two arenas each as large as its largest tenant (dec_conv0's tenant is four floats per pixel); every tensor
    rounded up to 256 bytes"""
    wp, hp = pad16(w), pad16(h)
    skip, arena = [0, 0, 0], [0, 0]
    for i, (cout, lv) in enumerate(zip(couts, U.LEVELS)):
        px = (hp >> lv) * (wp >> lv)
        size = align256(px * 16 if i == 15 else (px // 4 if i in POOLED else px) * pad16(cout) * 2)
        if PLACE[i] < 3:
            skip[PLACE[i]] = size
        else:
            arena[PLACE[i] - 3] = max(arena[PLACE[i] - 3], size)
    return align256(hp * wp * 32) + sum(skip) + sum(arena)


def macs_model(layers, w, h):
    """multiply-adds of one run over the padded w x h tile; layers = [(name, cin, cout)] with cin summed"""
    wp, hp = pad16(w), pad16(h)
    return sum(9 * cin * cout * (wp >> lv) * (hp >> lv) for (_, cin, cout), lv in zip(layers, U.LEVELS))


def plan(width, height, max_memory_mb, scratch):
    """the rule: (tile_width, tile_height, tiles_x, tiles_y); scratch(tw, th) -> bytes of one tile within the cap"""
    limit = max_memory_mb * 2 ** 20
    ty = tx = 1
    th, tw = pad16(height), pad16(width)
    side = lambda size, tiles: max(pad16(ceil_div(size - 2 * OVERLAP, tiles)) + 2 * OVERLAP, MIN_TILE)
    while tw > MAX_TILE_W or th > MAX_TILE_H or (max_memory_mb > 0 and scratch(tw, th) > limit):
        if th > MIN_TILE and th > tw:
            ty += 1
            th = side(height, ty)
        elif tw > MIN_TILE:
            tx += 1
            tw = side(width, tx)
        else:
            break
    tiles_y = ceil_div(height - 2 * OVERLAP, th - 2 * OVERLAP) if height > th else 1
    tiles_x = ceil_div(width - 2 * OVERLAP, tw - 2 * OVERLAP) if width > tw else 1
    return tw, th, tiles_x, tiles_y


FIELDS = ("x", "y", "w", "h", "out_x", "out_y", "out_w", "out_h")       # ptx_nn_tile's


def tiles_array(width, height, tw, th, tiles_x, tiles_y, overlap=OVERLAP):
    """the tiles in execution order (row-major) as an (n, 8) int32 array with FIELDS as columns (overlap: the definition's 96; a test
    that shows the comparison can fail cuts it)"""
    i, j = np.divmod(np.arange(tiles_x * tiles_y), tiles_x)
    y, x = i * (th - 2 * overlap), j * (tw - 2 * overlap)
    h, w = np.minimum(height - y, th), np.minimum(width - x, tw)
    top, left = np.where(i > 0, overlap, 0), np.where(j > 0, overlap, 0)
    bottom, right = np.where(i < tiles_y - 1, overlap, 0), np.where(j < tiles_x - 1, overlap, 0)
    return np.stack([x, y, w, h, x + left, y + top, w - left - right, h - top - bottom], axis=1).astype(np.int32)


def tiles(width, height, tw, th, tiles_x, tiles_y, overlap=OVERLAP):
    """the same as dicts with ptx_nn_tile's fields"""
    return [dict(zip(FIELDS, (int(v) for v in r))) for r in tiles_array(width, height, tw, th, tiles_x, tiles_y, overlap)]


def tiled_unet(x_in, weights, tile_list, dtype_name="float64"):
    """unet_ref.unet on every tile's window (the window at the top left of its own padded tensor), the kept rectangles pasted together"""
    h, w, _ = x_in.shape
    out = np.full((h, w, 3), np.nan)
    for t in tile_list:
        net = U.unet(x_in[t["y"]:t["y"] + t["h"], t["x"]:t["x"] + t["w"]], weights, dtype_name)
        iy, ix = t["out_y"] - t["y"], t["out_x"] - t["x"]
        out[t["out_y"]:t["out_y"] + t["out_h"], t["out_x"]:t["out_x"] + t["out_w"]] = net[iy:iy + t["out_h"], ix:ix + t["out_w"]]
    return out
