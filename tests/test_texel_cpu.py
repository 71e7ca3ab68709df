"""CPU: the oracle's texel lookups against the plain-numpy rule (tests/texel_ref.py) over the whole grid the GPU tier shades
(tests/test_gpu_texels.py): odd and non-square map sizes, 3 and 4 channels, every subset of kd / ks / ke on the mesh, texture coordinates
on every texel boundary, outside [0, 1] and tiled.  Proves on the reference side alone that the grid reaches what it is meant to reach
-- every class of lookup at every size -- before a GPU sees it."""
import numpy as np
import pytest

import texel_ref as TR
import texelcases as TC
from conftest import beq, dump_from_golden, golden


@pytest.fixture(scope="module")
def ship():
    return dump_from_golden(golden("loader_cornellSpaceship.npz"))


@pytest.fixture()
def O(oracle_lib):
    oracle_lib.set_libm(1)
    yield oracle_lib
    oracle_lib.set_libm(0)


def test_rule_on_hand_worked_lookups():
    """The restatement itself, on a 3 x 2 map whose bytes are their own index: u == 1 is the next row's first texel, v == 1 and beyond
    read the last byte three times, a negative index reads byte 0 three times, -0.1 truncates to texel 0, alpha is skipped."""
    for ch in (3, 4):
        img = np.arange(2 * 3 * ch, dtype=np.uint8).reshape(2, 3, ch)
        last = 2 * 3 * ch - 1
        u = np.float32([0.0, 0.34, 1.0, 0.99, 0.0, -0.4, -0.1, 1.0, np.nextafter(np.float32(1), np.float32(0))])
        v = np.float32([0.0, 0.0, 0.0, 0.99, 1.0, 0.0, -0.1, 0.5, 0.49])
        want = [[0, 1, 2], [ch, ch + 1, ch + 2], [3 * ch, 3 * ch + 1, 3 * ch + 2], [5 * ch, 5 * ch + 1, 5 * ch + 2], [last] * 3, [0] * 3,
                [0, 1, 2], [last] * 3, [2 * ch, 2 * ch + 1, 2 * ch + 2]]
        assert TR.fetch(img, u, v).tolist() == want
        assert TR.classes(u, v, 3, 2, ch).tolist() == [TR.INTERIOR, TR.INTERIOR, TR.WRAP_ROW, TR.LAST_TEXEL, TR.CLAMPED_HIGH, TR.CLAMPED_LOW,
                                                       TR.INTERIOR, TR.CLAMPED_HIGH, TR.INTERIOR]
    assert TR.admitted(1, 1) == {TR.LAST_TEXEL, TR.CLAMPED_HIGH} and TR.INTERIOR not in TR.admitted(5, 1)
    assert TR.admitted(64, 33) == set(range(7))
    c = np.float32([[0.5, 0.25, 1.0]])
    assert beq(TR.emission_colour(c, np.uint8([[255, 51, 0]])), np.float32([[2.5, np.float32(0.25) * (np.float32(51) / np.float32(255) * np.float32(5)), 0]]))
    assert beq(TR.tint(c, np.uint8([[255, 0, 51]])), np.float32([[0.5, 0, np.float32(51) / np.float32(255)]]))


@pytest.mark.parametrize("name,spec", TC.shade_grid(), ids=[c[0] for c in TC.shade_grid()])
def test_oracle_shades_by_the_rule(O, ship, name, spec):
    gi = TC.mesh_index(ship)
    seed = TC.case_seed(name)
    uv = TC.uv_grid(sorted({(w, h) for w, h, ch in spec.values()}), seed)
    TC.grid_conditions(uv, spec)
    maps = TC.make_maps(spec, seed)
    d = TC.with_maps(ship, gi, maps)
    idx, isects, paths = TC.shade_inputs(d, gi, uv, seed + 1)
    O.create(d, d["textures"])
    TC.assert_shaded_by_rule(O.shade(3, 1, idx, isects, paths), paths, uv, maps, d["materials"][d["geom_ints"][gi][1]])


def test_grid_covers_every_size_channel_count_and_subset():
    seen = [(w, h, ch, tuple(sorted(spec))) for _, spec in TC.shade_grid() for w, h, ch in spec.values()]
    for w, h in TC.SIZES:
        assert {ch for a, b, ch, s in seen if (a, b) == (w, h)} == {3, 4}
        assert {s for a, b, ch, s in seen if (a, b) == (w, h)} >= set(TC.SUBSETS) | {(TC.KD, TC.KS, TC.KE)}
    for sub in TC.SUBSETS:
        assert {ch for a, b, ch, s in seen if s == sub} == {3, 4}
    assert len(TC.shade_grid()) <= 48


def test_large_map_case_reaches_the_last_row_and_texel(O, ship):
    """The large-map case of the GPU tier on the oracle: kd 4096 x 1400 x 3 ahead of a 9 x 5 ke map, so that ke's bytes lie beyond 2^24 in a blob that
    stores the maps in order; the coordinates reach kd's last row and last texel."""
    spec = TC.LARGE_SPEC
    uv = TC.uv_grid([(4096, 1400), (9, 5)], 77)
    TC.grid_conditions(uv, spec)
    assert 4096 * 1400 * 3 > 1 << 24
    maps = TC.make_maps(spec, 77)
    gi = TC.mesh_index(ship)
    d = TC.with_maps(ship, gi, maps)
    idx, isects, paths = TC.shade_inputs(d, gi, uv, 78)
    O.create(d, d["textures"])
    TC.assert_shaded_by_rule(O.shade(3, 1, idx, isects, paths), paths, uv, maps, d["materials"][d["geom_ints"][gi][1]])


@pytest.mark.parametrize("tname", list(TC.UV_TRANSFORMS))
def test_transformed_mesh_uvs_reach_what_the_bump_test_needs(O, ship, tname):
    """What the GPU tier's bump test needs, on the oracle alone: about 6000 rays aimed at the mesh give at least 500 mesh hits, and with the face UVs
    tiled (uv' = 3 uv - 1) at least 100 clamped and at least 100 interior bump lookups at every map size."""
    gi = TC.mesh_index(ship)
    a, b = TC.UV_TRANSFORMS[tname]
    d = TC.with_uv_transform(TC.with_maps(ship, gi, TC.make_maps({TC.BUMP: (7, 3, 3)}, 5)), gi, a, b)
    O.create(d, d["textures"])
    oi = O.compute_intersections(TC.mesh_rays(d, gi, 6000, 77))
    mesh = (oi["t"] > 0) & (oi["geomId"] == gi)
    assert mesh.sum() >= 500
    uv = oi["texcoord"][mesh]
    assert np.abs(uv).max() <= 8
    for w, h in TC.BUMP_SIZES:
        cls = TR.classes(uv[:, 0], uv[:, 1], w, h)
        if tname == "tiled":
            assert TR.clamped(cls).sum() >= 100 and TC.inner_count(cls, w, h) >= 100, (w, h)
        elif tname == "identity":
            assert not TR.clamped(cls).any()


@pytest.mark.parametrize("key", sorted({c[1] for c in TC.FRAME_CASES}))
def test_frame_scenes_show_their_maps(O, ship, key):
    """What the GPU tier's frame cases need, on the oracle alone (96 x 54, depth 8, 3 iterations): every scene's frame differs from the frame of the
    same scene without its maps; tiled, the first bounce holds at least 50 clamped lookups; the 34-geom scene has a bump-mapped mesh
    beyond index 31 and one at index 0."""
    cornell_obj = dump_from_golden(golden("loader_cornellObj.npz"))
    frames = []
    d = TC.frame_scene(O, key, ship, cornell_obj)
    for scene in (d, TC.without_maps(d)):
        scene = dict(scene, cam_ints=np.array([96, 54, scene["cam_ints"][2], 8], np.int32))
        O.create(scene, scene["textures"])
        O.set_camera(scene["cam_ints"], O.camera_from_loader(96, 54, 45.0, [0, 5, 10.5], [0, 5, 0], [0, 1, 0]))
        O.apply_runcuda_camera()
        O.pt_init()
        if key == "tiled" and not frames:
            O.pt_generate(1)
            assert TC.clamped_lookups(d, O.compute_intersections(O.paths())) >= 50
        for it in (1, 2, 3):
            O.iterate(it)
        frames.append(O.image())
    assert frames[0].shape == (96 * 54, 3) and not beq(frames[0], frames[1])
    if key == "34":
        assert len(d["geom_ints"]) == 34 and (33, TC.BUMP) in d["textures"] and (0, TC.BUMP) in d["textures"]
    if key in ("two", "34"):
        assert len({img.shape for img in d["textures"].values()}) == 8


@pytest.mark.parametrize("front", [False, True], ids=["appended", "as-geom-0"])
def test_rays_reach_both_of_two_meshes(O, ship, front):
    """... and with the second mesh behind every cube and sphere no hit on those carries a texcoord; as geom 0 it leaves its own on
    cubes that win after it (computeIntersections copies tmp_uv with every new nearest hit): the value the GPU tier does not compare."""
    gi = TC.mesh_index(ship)
    d = TC.with_second_mesh(O, TC.with_maps(ship, gi, TC.make_maps({TC.BUMP: (7, 3, 3)}, 21)), gi, TC.TWIN_TRS, {}, front)
    first, second = (0, gi + 1) if front else (gi, gi + 1)
    O.create(d, d["textures"])
    oi = O.compute_intersections(np.concatenate([TC.mesh_rays(d, first, 3000, 78), TC.mesh_rays(d, second, 3000, 79)]))
    for g in (first, second):
        assert ((oi["t"] > 0) & (oi["geomId"] == g)).sum() >= 500
    other = (oi["t"] > 0) & (d["geom_ints"][oi["geomId"], 0] != 3)
    assert other.sum() >= 100 and oi["texcoord"][other].any() == front
