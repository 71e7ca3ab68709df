"""GPU: the per-tile kernels of adaptive sampling (csrc/pt_adaptive.hip) beyond 256 tiles.  k_tile_mask and k_adaptive_advance run one
thread per tile in workgroups of 256, k_adaptive_status one workgroup in which thread t takes ceil(ntiles / 256) tiles; the other tests
stop at 72 tiles.  A 300 x 220 frame has 258: a second workgroup of two threads, runs of two tiles, and a last tile of 208 pixels."""
import numpy as np
import pytest

from conftest import beq
from adaptive_ref import decide, num_tiles, resolve, status, tile_of, tile_sizes
from test_gpu_active_tiles import _drive, _scene, tile_of_pixel
from test_gpu_adaptive import _restated, _target_in_the_widest_gap
from test_gpu_lit_planes import aux_nonzero

pytestmark = pytest.mark.gpu

MANY = (300, 220)
NT, LAST = 258, 208


def _shape_is_as_stated(pt):
    W, H = MANY
    tp = pt.tile_pixels()
    assert (tp, W * H, num_tiles(H, W, tp), W * H - (NT - 1) * tp) == (256, 66000, NT, LAST)
    return tp


def masks():
    """{name: off}.  Both switch off a pseudo-random third of the tiles below 254 and leave tile 0 on.  `around_256`: 254, 255, 256 and
    257 off -- both sides of the workgroup boundary, the partial tile among them.  `above_256_on`: 255 and 256 off, 254 and 257 on, so
    that a tile of the second workgroup, the partial one, is traced between switched-off neighbours.  (258 tiles: no one mask does both.)"""
    out = {}
    for name, top in (("around_256", (True, True, True, True)), ("above_256_on", (False, True, True, False))):
        off = np.zeros(NT, bool)
        off[:254] = np.random.default_rng(258).random(254) < 1.0 / 3.0
        off[0] = False
        off[254:] = top
        out[name] = off
    return out


def _lit(img, tile):
    """per tile: at least 8 of its pixels hold light, so that 8 more iterations change the tile for certain"""
    return np.bincount(tile, weights=img.reshape(-1, 3).any(1), minlength=NT) >= 8


def _view_lighting_the_tiles_around_256(pt):
    """cornell.txt at 300 x 220, zoomed in until tiles 254 .. 257 (the last four rows) receive light within 4 iterations, as
    tests/test_gpu_active_tiles.py's _view_with_a_lit_last_tile does for its last tile"""
    for zoom in (0, -40, -80, -160, -320):
        s = _scene(pt, "cornell.txt", MANY)
        if zoom:
            s.orbit_events(s.orbit_init(), [("right", zoom)])
        with pt.Tracer(s) as T:
            T.render(1, 4)
            if _lit(T.read_image(), tile_of_pixel(pt, T))[254:].all():
                return s
    raise AssertionError("no view lights tiles 254 .. 257")


@pytest.mark.parametrize("how", ["render", "ahead"])
def test_a_mask_of_all_ones_changes_no_bit_at_258_tiles(gpu_product, how):
    pt = gpu_product
    _shape_is_as_stated(pt)
    s = _scene(pt, "cornell.txt", MANY)
    with pt.Tracer(s) as N, pt.Tracer(s) as A:
        assert A.num_tiles == NT
        A.set_active_tiles(np.ones(NT, np.uint8))
        for T in (N, A):
            _drive(T, 1, 4, how)
        img, st = N.read_image(), N.stats()
        assert img.any() and beq(A.read_image(), img)
        assert A.stats()["rays_per_bounce"] == st["rays_per_bounce"] and A.stats()["iterations"] == st["iterations"]


@pytest.mark.parametrize("name", ["around_256", "above_256_on"])
def test_inactive_tiles_keep_their_bits_beyond_the_first_workgroup(gpu_product, name):
    """tests/test_gpu_active_tiles.py's test_inactive_tiles_keep_their_bits_and_clearing_restores_the_tracer with masks around tile 256:
    4 iterations unmasked, 8 under the mask -- the inactive tiles hold their bits, every active tile that had light has changed, the
    camera bounce counts every pixel -- and after clearing the mask and resetting the image the tracer is a fresh one."""
    pt = gpu_product
    _shape_is_as_stated(pt)
    off = masks()[name]
    assert not off[0] and off[255] and off[256] and NT // 3 < off.sum() < NT // 2
    s = _view_lighting_the_tiles_around_256(pt)
    with pt.Tracer(s) as T, pt.Tracer(s) as N:
        tile = tile_of_pixel(pt, T)
        for X in (T, N):
            _drive(X, 1, 4, "render")
        before = T.read_image()
        assert beq(before, N.read_image())
        lit = _lit(before, tile)
        assert lit[254:].all() and (lit & ~off)[:254].sum() >= 8     # the tiles on both sides of 256 receive light: a mask there shows
        T.set_active_tiles(~off)
        for X in (T, N):
            _drive(X, 5, 8, "render")
        after = T.read_image()
        assert beq(after[off[tile]], before[off[tile]]) and all(before[tile == t].any() for t in np.flatnonzero(off[254:]) + 254)
        for t in np.flatnonzero(lit & ~off):
            assert not beq(after[tile == t], before[tile == t]), t
        st, sn = T.stats(), N.stats()
        assert st["rays_per_bounce"][0] == sn["rays_per_bounce"][0] > 0 and st["iterations"] == sn["iterations"] == 12
        assert st["rays_per_bounce"][1] < sn["rays_per_bounce"][1]
        assert aux_nonzero(T)[:2] == [0, 0]
        T.clear_active_tiles()
        T.reset_image()
        _drive(T, 1, 4, "render")
        with pt.Tracer(s) as F:
            _drive(F, 1, 4, "render")
            assert beq(T.read_image(), F.read_image()) and T.stats()["rays_per_bounce"] == F.stats()["rays_per_bounce"]


KS = (8, 8, 48, 192)


def noise_scales():
    """Per-tile noise levels in three groups a factor 10 and a factor 7 apart, each spread by +-8 %.  LOW: odd tiles 1, 7, 13, ...; HIGH:
    odd tiles 3, 9, 15, ... and tile 257, which holds the largest; MID: the rest, every even tile among them.  With KS the widest gap
    between the tiles' errors is LOW | MID after the second add (LOW stops at 16 samples), MID | HIGH after the third (MID stops at 64)
    and LOW | MID again after the fourth, where max_samples stops HIGH at 256: the smallest and the largest count sit in odd tiles
    only, the worst error in the partial tile 257, and tiles 256 (MID) and 257 (HIGH) differ in everything the status tallies."""
    t = np.arange(NT)
    group = np.where(t % 6 == 1, 0, np.where(t % 6 == 3, 2, 1))
    group[257] = 2
    scale = np.array([0.02, 0.2, 1.4])[group] * (0.92 + 0.16 * np.random.default_rng(7).random(NT))
    scale[257] = 1.4 * 1.15
    return group, scale


def buffers(H, W, tile, scale, seed=11):
    """generator over KS of (k, gain (H, W, 3) float32): tests/test_gpu_adaptive.py's synthetic batches, the caller masks them"""
    rng = np.random.default_rng(seed)
    f = np.float32
    c = (0.05 + 0.95 * rng.random((H, W, 3))).astype(f)
    for k in KS:
        z = (0.5 * rng.standard_normal((H, W, 1)) + 0.2 * rng.standard_normal((H, W, 3))) * scale[tile].reshape(H, W, 1)
        yield k, (k * c * np.maximum(1 + z / np.sqrt(k), 0)).astype(f)


def test_advance_select_status_and_resolve_at_258_tiles(gpu_product):
    """The flow of test_select_matches_the_restatement at 258 tiles (a fourth add, because three leave only two sample counts and the
    smallest and the largest cannot both avoid the even tiles): per-tile samples, batches and decisions exactly, e_T within 1e-5,
    every integer of the status exactly and worst_error within 1e-5, the same bits from a second select, the resolve bit for bit."""
    pt = gpu_product
    W, H = MANY
    tp = _shape_is_as_stated(pt)
    s = _scene(pt, "cornell.txt", MANY)
    group, scale = noise_scales()
    tile = tile_of(H, W, tp).ravel()
    n_t = tile_sizes(H, W, tp)
    odd = np.arange(NT) % 2 == 1
    assert n_t[-1] == LAST and odd[group != 1].all()
    with pt.Tracer(s) as T, pt.Moments(0, W, H) as m, pt.Adaptive(0, W, H) as a:
        assert a.num_tiles == T.num_tiles == NT
        samples, batches, active = np.zeros(NT, np.int64), np.zeros(NT, np.int64), np.ones(NT, bool)
        acc = np.zeros((H, W, 3), np.float32)
        selects = 0
        history = []
        worst_te = 0.0
        for rnd, (k, gain) in enumerate(buffers(H, W, tile, scale), 1):
            acc = (acc + np.where(active[tile].reshape(H, W, 1), gain, np.float32(0))).astype(np.float32)
            T.write_image(acc)
            a.add(m, T, k)
            samples += k * active
            batches += active
            assert beq(m.read_samples().ravel(), samples[tile].astype(np.int32)) and beq(m.read()["batches"].ravel(), batches[tile].astype(np.int32))
            e, has = _restated(m, 0.05, tp)
            assert has.all() == (rnd >= 2)
            target = _target_in_the_widest_gap(e) if rnd >= 2 else 0.02
            cap = int(samples.max()) if rnd == 4 else 1 << 20
            st = a.select(m, T, target=target, min_batches=2, max_samples=cap)
            selects += 1
            rd = a.read()
            want_active = decide(samples, batches, e, target, 2, cap)
            print("round %d: target %.6g, %s" % (rnd, target, st))
            te = float((np.abs(rd["tile_error"] - e) / np.maximum(e, 1e-30)).max()) if rnd >= 2 else 0.0
            worst_te = max(worst_te, te)
            assert (np.abs(rd["tile_error"] - e) <= 1e-5 * e).all(), (rd["tile_error"], e)
            assert (rd["tile_active"] == want_active).all()
            want = status(samples, want_active, e, has, H, W, tp, selects)
            for key, v in want.items():
                assert (abs(st[key] - v) <= 1e-5 * v) if key == "worst_error" else (st[key] == v), (rnd, key, st[key], v)
            assert beq(rd["samples"].ravel(), samples[tile].astype(np.int32))
            if rnd >= 2:                                             # the same bits from a second run
                st2, rd2 = a.select(m, T, target=target, min_batches=2, max_samples=cap), a.read()
                selects += 1
                assert {**st2, "rounds": 0} == {**st, "rounds": 0} and st2["rounds"] == st["rounds"] + 1
                assert beq(rd2["tile_error"], rd["tile_error"]) and beq(rd2["tile_active"], rd["tile_active"])
                assert int(np.argmax(np.where(has, e, 0.0))) == NT - 1                # the worst error sits in the partial tile, above 256
            history.append((samples.copy(), want_active.copy(), e.copy()))
            active = want_active
        print("largest relative error of tile_error: %.3g" % worst_te)
        # the schedule did what noise_scales says
        (s2, a2, _), (s3, a3, _), (s4, a4, e4) = history[1:]
        assert (a2 == (group != 0)).all() and (a3 == (group == 2)).all() and (a4 == (group == 1)).all()
        assert a3[NT - 1] and not a4[NT - 1]                          # the partial tile: active in one round, stopped in another
        assert sorted(set(s4.tolist())) == [16, 64, 256]
        assert odd[s4 == s4.min()].all() and odd[s4 == s4.max()].all()
        # tiles 256 and 257 are one thread's run: they differ in samples, pixels, decision and error
        assert s4[256] != s4[257] and a4[256] != a4[257] and e4[256] != e4[257] and n_t[256] != n_t[257]
        assert s4[256] * n_t[256] != s4[257] * n_t[257]
        a.resolve(T)
        assert beq(a.read()["mean"], resolve(acc, samples, H, W, tp))
        assert a.read()["mean"].reshape(-1, 3)[tile == NT - 1].any()
