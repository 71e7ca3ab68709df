"""CPU: the material parameter space of tests/materialcases.py.  The oracle (glibc libm mode = the reference's host semantics) against
the two zoo fixtures that tests/golden/make_golden.py wrote with the reference's own functions, and -- where oracle/_ref exists --
against the live reference on every single-material case, bit for bit; the condition that makes the zoo a test of every material (each
is hit often enough); and the host tables the kernels key off a material's fields (light_bits, the record masks) against their rules
restated over the dumped floats.  tests/test_gpu_materials.py then holds the device to the oracle on the same scenes."""
import numpy as np
import pytest

from conftest import beq, golden
import materialcases as MC
from test_loader import product_dump_from_text
from test_record_masks import masks, runs


@pytest.fixture()
def O(oracle_lib):
    oracle_lib.set_libm(0)
    yield oracle_lib
    oracle_lib.set_libm(0)


def zoo_dump(res=(96, 72), depth=8):
    return product_dump_from_text(MC.zoo_text(res, depth), runcuda=True)


def test_every_material_of_the_zoo_is_hit(O):
    """In the sorted streams of iteration 1 at 96x72, depth 8, every material 0-17 and the mesh's own is the hit material of at least 50
    records, summed over the bounces (the rarest: 135, material 16)."""
    d = zoo_dump()
    assert len(d["materials"]) == MC.ZOO_OBJ_MATERIAL + 1 and len(d["geom_ints"]) == 32
    assert beq(d["materials"][: len(MC.ZOO_MATERIALS)], np.array(MC.ZOO_MATERIALS, np.float32))       # the file fields arrive as written
    O.create(d); O.set_options(aa=1, dof=0, sort=1, cache=1); O.pt_init()
    counts = MC.hit_counts(O, len(d["materials"]))
    print("records per material:", counts.tolist(), "rarest:", int(counts.min()), "material", int(counts.argmin()))
    assert counts.min() >= MC.ZOO_MIN_RECORDS, counts.tolist()


def test_zoo_placement_covers_both_kinds_of_geom():
    """Among the non-diffuse materials one sits on cubes only, one on spheres only, one on both; the same among the diffuse ones."""
    d = zoo_dump()
    gi, m = d["geom_ints"], d["materials"]
    on = lambda mat, typ: bool(((gi[:, 1] == mat) & (gi[:, 0] == typ)).any())
    kinds = {(bool(m[k, 7] > 0 or m[k, 8] > 0), on(k, 1), on(k, 0)) for k in range(len(MC.ZOO_MATERIALS))}
    for nondiffuse in (False, True):
        assert {(nondiffuse, True, False), (nondiffuse, False, True), (nondiffuse, True, True)} <= kinds
    assert (gi[:, 0] == 3).sum() == 1 and gi[gi[:, 0] == 3, 1][0] == MC.ZOO_OBJ_MATERIAL


def test_zoo_shade_kat(O):
    """shadeFakeMaterial + scatterRay of the oracle on the (path, intersection) pairs captured from the reference's render of the zoo:
    every branch the zoo's materials select, bit for bit."""
    k = golden("shade_kat_zoo.npz")
    text = bytes(k["scene_text"]).decode()
    assert text == MC.zoo_text((48, 36), 8)
    d = product_dump_from_text(text)
    O.create(d)
    keys = sorted(x[:-6] for x in k.files if x.endswith("_paths"))
    assert keys == ["it1_b%d" % b for b in range(4)]
    seen = np.zeros(len(d["materials"]), np.int64)
    for key in keys:
        out = O.shade(1, 1, k[key + "_idx"], k[key + "_isects"], k[key + "_paths"])
        assert beq(out, k[key + "_shaded"]), key
        s = k[key + "_isects"]
        seen += np.bincount(s["materialId"][s["t"] > 0], minlength=len(seen))
    assert seen.sum() > 3000 and seen.min() >= 10, seen.tolist()          # hits among the 4478 records; every material among them


def test_zoo_render(O):
    """Whole iterations of the zoo: the sorted streams of iteration 1, image and counts after 1, 2 and 4 iterations, and the apps
    variant's image (x PI gather) and albedo after 3, as the reference's functions gave them."""
    r = golden("render_zoo.npz")
    assert bytes(r["scene_text"]).decode() == MC.zoo_text((96, 72), 8)
    d = zoo_dump()
    aa, dof, sort, cache = map(int, r["options"])
    O.create(d); O.set_options(aa=aa, dof=dof, sort=sort, cache=cache); O.pt_init()
    O.pt_generate(1)
    b = 0
    while True:
        n = O.num_paths()
        O.pt_bounce(1, 3)
        assert beq(O.paths()["pixelIndex"][:n], r["stream_pix_b%d" % b])
        assert beq(O.isects()["materialId"][:n], r["stream_mat_b%d" % b])
        assert beq(O.isects()["t"][:n], r["stream_t_b%d" % b])
        if O.pt_bounce(1, 12) == 0:
            break
        b += 1
    assert "stream_pix_b%d" % (b + 1) not in r.files
    O.pt_final_gather()
    for it in (1, 2, 3, 4):
        if it > 1:
            O.iterate(it)
        if it != 3:
            assert beq(O.live_counts(), r["counts_it%d" % it]) and beq(O.image(), r["image_spp%d" % it]), it
    assert np.isfinite(O.image()).all()
    O.create(d); O.set_apps_variant(1); O.pt_init()
    for it in (1, 2, 3):
        O.iterate(it)
    assert beq(O.image(), r["apps_image_spp3"]) and beq(O.albedo(), r["apps_albedo"]) and beq(O.live_counts(), r["apps_counts_it3"])


def _against_the_reference(R, O, mat, **opt):
    import os
    from conftest import ROOT
    text = MC.single_text(mat, (48, 36), 8)
    R.load_text(text, cwd=os.path.join(ROOT, "scenes"))
    rd = R.dump()
    assert beq(product_dump_from_text(text)["materials"], rd["materials"])      # both loaders read the fields alike (1e6, 1e-30, -1.5)
    assert beq(rd["materials"][4], np.array(mat, np.float32))
    O.create(rd)
    R.apply_runcuda_camera(); O.apply_runcuda_camera()
    R.set_options(**opt); O.set_options(**opt)
    R.pt_init(); O.pt_init()
    for it in (1, 2, 3):
        R.iterate(it); O.iterate(it)
        assert beq(R.live_counts(), O.live_counts()), it
    assert beq(R.image(), O.image())
    assert beq(R.paths(), O.paths())
    return O.image()


@pytest.mark.parametrize("name,mat", MC.GRID, ids=[n for n, _ in MC.GRID])
def test_grid_case_equals_the_reference(ref_lib, O, name, mat):
    """One material of the grid on a sphere, a rotated cube and a second sphere: 3 iterations at 48x36, depth 8 -- counts, image and the
    final stream of the oracle equal the reference's bit for bit, and the frame is finite."""
    img = _against_the_reference(ref_lib, O, mat, aa=1, dof=0, sort=1, cache=1)
    assert np.isfinite(img).all()


@pytest.mark.parametrize("name,mat", MC.NONFINITE, ids=[n for n, _ in MC.NONFINITE])
def test_nonfinite_case_equals_the_reference(ref_lib, O, name, mat):
    """A negative exponent: pow(0, e < 0) = inf reaches the colour, never a ray.  Counts, image and final stream equal the reference's,
    NaN == NaN through beq; the frame is not finite (else the case would not belong here)."""
    img = _against_the_reference(ref_lib, O, mat, aa=1, dof=0, sort=1, cache=1)
    assert not np.isfinite(img).all()


def test_light_bits_of_the_zoo(product):
    """ptx_create's light_bits: a geom's bit is set iff its material has emittance > 0 -- the light, the emitting mirror (12) and the dim
    light (14); not the negative emitter (13)."""
    d = zoo_dump()
    mats, gm = np.asarray(d["materials"], np.float32).reshape(-1, 11), np.asarray(d["geom_ints"])[:, 1]
    want = 0
    for g, m in enumerate(gm):
        if mats[m][10] > 0:
            want |= 1 << g
    got = product.api.debug_light_bits(mats, gm)
    assert got == want
    for g, m in enumerate(gm):
        assert bool(got >> g & 1) == (int(m) in (0, 12, 14)), (g, int(m))
    assert all((gm == m).any() for m in (12, 13, 14))


def test_record_masks_of_the_zoo(product):
    """ptx_create's record masks over the zoo's bins (bin = number of materials - 1 - material): the direction rule (reflective > 0 or
    refractive > 0 over the dumped floats, or the material of a mesh) asks for 4-12, 15, 16 and the mesh's -- three runs, so the
    gap-filling loop runs; the mask holds all of them in at most two.  The normal-code mask marks only materials that cubes alone have,
    in at most two runs, and both of its outcomes occur among the diffuse materials."""
    d = zoo_dump()
    mats, gi = np.asarray(d["materials"], np.float32).reshape(-1, 11), np.asarray(d["geom_ints"])
    nm = len(mats)
    bit = lambda m: 1 << (nm - 1 - m)
    need = cubes_only = 0
    for m in range(nm):
        on = gi[gi[:, 1] == m, 0]
        if mats[m, 7] > 0 or mats[m, 8] > 0 or (on == 3).any():
            need |= bit(m)
        if len(on) and (on == 1).all():
            cubes_only |= bit(m)
    assert need == sum(bit(m) for m in MC.ZOO_DIRECTION_MATERIALS)
    assert runs(need, nm) == 3
    dmask, nmask = masks(mats, gi[:, 0], gi[:, 1])
    assert dmask & need == need and runs(dmask, nm) <= 2 and dmask >> nm == 0
    assert dmask != (1 << nm) - 1                                  # (filled, not given up: some diffuse bin still travels light)
    assert cubes_only == sum(bit(m) for m in (0, 1, 2, 3, 15, 16)) and nmask == cubes_only          # two runs: nothing to drop
    diffuse = [m for m in range(nm) if not need & bit(m)]
    assert any(nmask & bit(m) for m in diffuse) and any(not nmask & bit(m) for m in diffuse)
    assert any(nmask & bit(m) for m in MC.ZOO_DIRECTION_MATERIALS)                                  # a record with a code AND a direction
    dmask, nmask = masks(mats, gi[:, 0], gi[:, 1], sort=0)
    assert dmask == 1 and nmask == 0


@pytest.mark.parametrize("name,mat", MC.GRID + MC.NONFINITE, ids=[n for n, _ in MC.GRID + MC.NONFINITE])
def test_host_tables_of_a_grid_case(product, name, mat):
    """The single-material scenes have one run of bins at the most, so nothing is filled or dropped: the direction mask IS the rule
    (reflective > 0 or refractive > 0 -- not != 0: REFL -1 REFR -1 is diffuse), the code mask the box's four materials, and light_bits
    the ceiling light plus the three geoms of an emitter (emittance > 0: not -2, but 1e-30)."""
    d = product_dump_from_text(MC.single_text(mat, (48, 36), 8))
    mats, gi = np.asarray(d["materials"], np.float32).reshape(-1, 11), np.asarray(d["geom_ints"])
    assert len(mats) == 5 and beq(mats[4], np.array(mat, np.float32)) and gi[:, 1].tolist() == [0, 1, 1, 1, 2, 3, 4, 4, 4]
    dmask, nmask = masks(mats, gi[:, 0], gi[:, 1])
    assert dmask == (1 if mats[4, 7] > 0 or mats[4, 8] > 0 else 0)
    assert nmask == 0b11110
    assert product.api.debug_light_bits(mats, gi[:, 1]) == (0x1c1 if mats[4, 10] > 0 else 0x001)
