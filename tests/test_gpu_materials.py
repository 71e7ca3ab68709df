"""GPU: the bounce kernels across the material parameter space (tests/materialcases.py), against the CPU oracle in its portable-libm
mode, bit for bit.

Everything the kernels key off a material's fields -- the record masks (a record's direction and normal code), light_bits (the
light-only last bounce), scatterRayT's branches in every k_bounce mode, write_albedo -- meets here what the stock scenes never hold:
specular exponents other than 0 (powf_own with a real argument), fractional and negative REFL / REFR, indices of refraction <= 1 and 0,
an emitting mirror, a negative emitter.  tests/test_materials_cpu.py pins the oracle to the reference on the same scenes."""
import numpy as np
import pytest

from conftest import beq, golden
import materialcases as MC
from test_gpu_parity import O, fences_stay_silent, _scene_from_text, _vs_oracle, check_sorted_streams  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

ZOO_RES, ZOO_DEPTH = (96, 72), 8          # 27 tiles of 256 paths; the grid's 48 x 36 is 7 with a ragged last one


def _zoo(pt, tmp_path, res=ZOO_RES, depth=ZOO_DEPTH):
    return _scene_from_text(pt, MC.zoo_text(res, depth), tmp_path)


def _oracle(O, s, **opt):
    d = s.dump()
    O.set_libm(1); O.create(d, d["textures"])
    O.set_options(aa=opt.get("antialiasing", 1), dof=opt.get("depth_of_field", 0), sort=opt.get("sort_by_material", 1), cache=opt.get("cache_first_bounce", 1))
    O.pt_init()
    return d


# ---- a. the shade KAT -------------------------------------------------------------------------------------------------------

def test_zoo_shade_kat_on_device(gpu_product, O, tmp_path):
    """k_kat_shade on the (path, intersection) pairs captured from the reference's render of the zoo: bit for bit the oracle's
    (portable libm); against the fixture (glibc's libm) remainingBounces and pixelIndex exactly, origin / direction / colour within
    rtol = atol = 2e-6.  Measured share of identical values per bounce and field: origin and colour 1.0, direction 0.9944 at the least
    (bounce 2), 0.99845 over all values -- powf_own and the portable sin / cos round as glibc does nearly everywhere; the floor is 0.99."""
    k = golden("shade_kat_zoo.npz")
    s = _scene_from_text(gpu_product, bytes(k["scene_text"]).decode(), tmp_path)
    O.set_libm(1); O.create(s.dump())
    same = total = 0
    with gpu_product.Tracer(s) as T:
        for key in sorted(x[:-6] for x in k.files if x.endswith("_paths")):
            got = T.shade(1, k[key + "_idx"], k[key + "_isects"], k[key + "_paths"])
            assert beq(got, O.shade(1, 1, k[key + "_idx"], k[key + "_isects"], k[key + "_paths"])), key
            want = k[key + "_shaded"]
            assert beq(got["remainingBounces"], want["remainingBounces"]) and beq(got["pixelIndex"], want["pixelIndex"])
            for f in ("origin", "direction", "color"):
                share = float((got[f] == want[f]).mean())
                print("%s %-9s identical to the glibc fixture: %.5f" % (key, f, share))
                same += int((got[f] == want[f]).sum()); total += got[f].size
                assert np.allclose(got[f], want[f], rtol=2e-6, atol=2e-6), (key, f)
                assert share > 0.99, (key, f, share)
    print("all values: %.5f" % (same / total))


# ---- b. the zoo on the production path ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("opt", [{}, dict(batch=1), dict(batch=1, lanes=1), dict(no_cull=1), dict(sort_by_material=0, cache_first_bounce=0),
                                 dict(depth_of_field=1), dict(depth_of_field=1, antialiasing=0)],
                         ids=lambda o: ",".join("%s=%s" % kv for kv in o.items()) or "defaults")
def test_zoo_frames(gpu_product, O, tmp_path, opt):
    """4 iterations of the zoo at 96x72, depth 8: image and rays per bounce equal the oracle's."""
    img = _vs_oracle(gpu_product, O, _zoo(gpu_product, tmp_path), iters=4, **opt)
    assert np.isfinite(img).all() and img.any()
    if not opt:
        # ... and the reference's own frame: exactly where glibc's pow and the portable one agree on every path (they differ in 3 of
        # 20736 values after 4 iterations, on pixels around 1e-25), within the libm swap's rtol = atol = 2e-6 everywhere
        assert np.allclose(img, golden("render_zoo.npz")["image_spp4"], rtol=2e-6, atol=2e-6)


def test_zoo_apps_variant(gpu_product, O, tmp_path):
    """apps_variant = 1 on the zoo: image (x PI) and albedo AOV equal the oracle's bit for bit and the counts too; against the fixture
    (glibc's libm) the albedo and the counts exactly, the image within the libm swap's rtol = atol = 2e-6 (3 values differ, around 1e-25)."""
    r = golden("render_zoo.npz")
    s = _zoo(gpu_product, tmp_path)
    _oracle(O, s)
    O.set_apps_variant(1); O.pt_init()
    try:
        for it in (1, 2, 3):
            O.iterate(it)
        with gpu_product.Tracer(s, apps_variant=1) as T:
            T.render(1, 3)
            img, alb, st = T.read_image(), T.read_albedo(), T.stats()
        assert beq(img, O.image()) and beq(alb, O.albedo())
        assert st["rays_per_bounce"][: len(O.live_counts())] == O.live_counts().tolist() == r["apps_counts_it3"].tolist()
        assert beq(alb, r["apps_albedo"])
        assert np.allclose(img, r["apps_image_spp3"], rtol=2e-6, atol=2e-6)
    finally:
        O.set_apps_variant(0)


@pytest.mark.parametrize("depth", [1, 2])
def test_zoo_shortest_paths(gpu_product, O, tmp_path, depth):
    """Depth 1 and 2: the light-only last bounce is the camera bounce itself, or follows it directly -- on a scene where a mirror emits
    (its geoms are in light_bits and its bin carries a direction) and an emitter is negative (no light)."""
    s = _zoo(gpu_product, tmp_path, depth=depth)
    img = _vs_oracle(gpu_product, O, s, iters=4)
    assert img.any()
    _vs_oracle(gpu_product, O, s, iters=4, batch=1, lanes=1)


# ---- c. every record after every bounce -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("as_run", [False, True], ids=["captured", "as-run"])
def test_zoo_sorted_streams(gpu_product, O, tmp_path, monkeypatch, as_run):
    """After each bounce the device stream holds the oracle's sorted survivors, field by field: once with every record complete (a
    capture's own mode), once with the kernels running as they do otherwise (PTX_DEBUG_KEEP_DIR_SKIP): records of diffuse hits without
    their direction, records of materials that only cubes have -- the box's, and mirrors 15 and 16 -- with a code for their normal."""
    if as_run:
        monkeypatch.setenv("PTX_DEBUG_KEEP_DIR_SKIP", "1")
    s = _zoo(gpu_product, tmp_path)
    d = _oracle(O, s)
    with gpu_product.Tracer(s) as T:
        check_sorted_streams(T, O, d, ZOO_DEPTH, directions_where_needed_only=as_run)


def test_zoo_records_weigh_what_the_host_tables_say(gpu_product, O, tmp_path):
    """ptx_stats counts the stored paths of a frame by what their records carry.  Over iteration 1 of the zoo: the oracle's pending
    paths, bounce by bounce, through the masks ptx_create keeps (ptx_debug_record_masks; tests/test_materials_cpu.py holds them to
    their rules) -- with a direction where the filled mask says so, with a normal code on the box and on mirrors 15 and 16."""
    from test_gpu_parity import oracle_pending_stream
    from test_record_masks import masks
    s = _zoo(gpu_product, tmp_path)
    d = _oracle(O, s)
    mats, gi = d["materials"], d["geom_ints"]
    nm = len(mats)
    dmask, nmask = masks(mats, gi[:, 0], gi[:, 1])
    with_dir = np.array([bool(dmask >> (nm - 1 - m) & 1) for m in range(nm)])
    with_code = np.array([bool(nmask >> (nm - 1 - m) & 1) for m in range(nm)])
    want = np.zeros(3, np.int64)
    for b in range(ZOO_DEPTH - 1):
        n, paths, isects = oracle_pending_stream(O, 1, b)
        m = isects["materialId"][(isects["t"] > 0) & (mats[isects["materialId"], 10] <= 0)]
        want += (len(m), int(with_dir[m].sum()), int(with_code[m].sum()))
    with gpu_product.Tracer(s) as T:
        T.render(1, 1)
        st = T.stats()
    assert (st["stored_paths"], st["stored_with_direction"], st["stored_with_normal_code"]) == tuple(int(x) for x in want)
    assert 0 < want[2] < want[0] and 0 < want[1] < want[0]


# ---- d. full grids --------------------------------------------------------------------------------------------------------------

def test_zoo_on_a_frame_of_many_workgroups(gpu_product, O, tmp_path):
    """320x200: 250 tiles, every material bin spans more than one workgroup and the run search moves on."""
    s = _zoo(gpu_product, tmp_path, res=(320, 200))
    O.set_threads(16)
    try:
        _vs_oracle(gpu_product, O, s, iters=3)
        _vs_oracle(gpu_product, O, s, iters=3, batch=1, lanes=1)
    finally:
        O.set_threads(1)


# ---- e. the variants agree ------------------------------------------------------------------------------------------------------

_DEFAULT = {}


def _default_zoo_frame(pt, tmp_path):
    if not _DEFAULT:
        with pt.Tracer(_zoo(pt, tmp_path)) as T:
            T.render(1, 5)
            img = T.read_image()
            img.setflags(write=False)
            _DEFAULT["img"], _DEFAULT["rays"] = img, T.stats()["rays_total"]
    return _DEFAULT["img"], _DEFAULT["rays"]


@pytest.mark.parametrize("switch", ["PTX_DEBUG_NO_FAST", "PTX_DEBUG_NO_LAST", "PTX_DEBUG_LAST_INPLACE", "PTX_DEBUG_NO_DIR_SKIP",
                                    "PTX_DEBUG_NO_NORMAL_CODES", "PTX_DEBUG_NO_TANGENTS", "PTX_DEBUG_NO_TILE_GEOMS"])
def test_zoo_kernel_variants_agree(gpu_product, tmp_path, monkeypatch, switch):
    """5 iterations of the zoo with one optimisation switched off (general instead of specialised kernel, no light-only last bounce or
    its in-place form, every record with its direction / its normal, tangent frames per ray, no per-tile geom masks): the same image
    and the same number of rays as the default."""
    img, rays = _default_zoo_frame(gpu_product, tmp_path)
    monkeypatch.setenv(switch, "1")
    with gpu_product.Tracer(_zoo(gpu_product, tmp_path)) as T:
        T.render(1, 5)
        assert beq(T.read_image(), img) and T.stats()["rays_total"] == rays


# ---- f. the grid ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,mat", MC.GRID, ids=[n for n, _ in MC.GRID])
def test_grid_case(gpu_product, O, tmp_path, name, mat):
    """One material on a sphere, a rotated cube and a second sphere in the lit box, 48x36, depth 8, 3 iterations."""
    s = _scene_from_text(gpu_product, MC.single_text(mat, (48, 36), 8), tmp_path)
    img = _vs_oracle(gpu_product, O, s, iters=3)
    assert np.isfinite(img).all()
    _vs_oracle(gpu_product, O, s, iters=3, batch=1, sort_by_material=0)


# ---- g. non-finite colour -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,mat", MC.NONFINITE, ids=[n for n, _ in MC.NONFINITE])
def test_nonfinite_colour(gpu_product, O, tmp_path, name, mat):
    """A negative exponent makes pow(0, e) = inf, and inf x 0 = NaN, in a path's colour.  No index or branch of k_bounce, k_finish or
    k_gather derives from a colour (classifyPath tests the material's emittance, deposit and the gather add), so the rays are the
    oracle's: same rays per bounce, the same pixels NaN, +inf and -inf, every other pixel bit-equal.  NaN sign and payload are not
    compared: the host's and the device's default NaNs differ."""
    s = _scene_from_text(gpu_product, MC.single_text(mat, (48, 36), 8), tmp_path)
    _oracle(O, s)
    for it in (1, 2, 3):
        O.iterate(it)
    want = O.image()
    with gpu_product.Tracer(s) as T:
        T.render(1, 3)
        got, st = T.read_image(), T.stats()
    assert st["rays_per_bounce"][: len(O.live_counts())] == O.live_counts().tolist()
    assert not np.isfinite(want).all()
    for cls in (np.isnan, np.isposinf, np.isneginf):
        assert np.array_equal(cls(got), cls(want)), cls.__name__
    fin = np.isfinite(want)
    assert beq(got[fin], want[fin])


# ---- h. guides ------------------------------------------------------------------------------------------------------------------

def test_zoo_pixel_centre_guides(gpu_product, O, tmp_path):
    """k_gbuffer on the zoo against the oracle's pixel-centre rays and first hits, bit for bit; the albedo against write_albedo's rule
    restated over the dumped floats (guides_ref.untextured_albedo): an emitter's colour x emittance before a refractive material's
    specular colour -- materials 7, 10, 12, 13, 14 tell the orders apart -- and against the apps variant's AOV."""
    from guides_ref import untextured_albedo
    pt = gpu_product
    W, H = ZOO_RES
    s = _zoo(pt, tmp_path)
    d = s.dump()
    O.set_libm(1); O.create(d, d["textures"])
    O.set_options(aa=0, dof=0)
    O.pt_init()
    O.pt_generate(1)
    op = O.paths()
    oi = O.compute_intersections(op)
    with pt.Tracer(s) as T:
        g = T.gbuffer()
    hit = (oi["t"] > 0).reshape(H, W)
    assert np.array_equal(g["hit"], hit) and hit.sum() > H * W // 2
    assert beq(g["t"][hit], oi["t"].reshape(H, W)[hit]) and beq(g["normal"][hit], oi["normal"].reshape(H, W, 3)[hit])
    assert beq(g["material"][hit], oi["materialId"].reshape(H, W)[hit]) and beq(g["geom"][hit], oi["geomId"].reshape(H, W)[hit])
    pos = (op["origin"] + oi["t"][:, None] * op["direction"]).astype(np.float32).reshape(H, W, 3)
    assert beq(g["position"][hit], pos[hit])
    seen = set(np.unique(oi["materialId"][oi["t"] > 0]).tolist())
    assert {7, 10, 12, 13, 14} <= seen, sorted(seen)
    assert beq(g["albedo"].reshape(-1, 3), untextured_albedo(d, oi["materialId"], oi["geomId"], oi["t"] > 0))
    O.set_apps_variant(1)
    try:
        O.set_depth(1); O.pt_init(); O.iterate(1)
        assert beq(g["albedo"].reshape(-1, 3), O.albedo())
    finally:
        O.set_apps_variant(0)


def test_zoo_sampled_guides(gpu_product, O, tmp_path):
    """k_guides over the camera rays of iterations 1-4 (antialiasing on) against the numpy restatement, bit for bit."""
    from guides_ref import oracle_samples, sampled_guides
    from test_gpu_guides import _same_as_the_restatement
    pt = gpu_product
    W, H = ZOO_RES
    s = _zoo(pt, tmp_path)
    d = s.dump()
    O.set_libm(1); O.create(d, d["textures"])
    O.set_options(aa=1, dof=0)
    O.pt_init()
    ref = sampled_guides(oracle_samples(O, d, 1, 4))
    with pt.Tracer(s, antialiasing=1) as T:
        T.set_guide_samples(4)
        _same_as_the_restatement(T, ref, W, H, "zoo")
    assert ref["mixed"].any() and ref["hit"].sum() > W * H // 2


# ---- i. the render the device never saw -----------------------------------------------------------------------------------------

def test_mirror20_render_matches_reference_golden(gpu_product, O, tmp_path):
    """render_mirror20.npz (exponent 20.5 on a sphere and a cube) on the device as tests/test_gpu_parity.py compares the other seven
    renders: the accumulated radiance after 1, 2 and 16 iterations equals the golden frames and the oracle's bit for bit; so do the
    per-bounce ray counts and the 8-bit preview."""
    r = golden("render_mirror20.npz")
    aa, dof, sort, cache = map(int, r["options"])
    s = _scene_from_text(gpu_product, bytes(golden("shade_kat_mirror20.npz")["scene_text"]).decode(), tmp_path)
    assert s.resolution == (64, 64) and s.trace_depth == 8
    opt = dict(antialiasing=aa, depth_of_field=dof, sort_by_material=sort, cache_first_bounce=cache)
    _oracle(O, s, **opt)
    with gpu_product.Tracer(s, **opt) as T:
        for it in range(1, 17):
            O.iterate(it)
            T.pathtrace(it)
            if it in (1, 2, 16):
                img = T.read_image()
                assert beq(img, O.image())
                assert np.array_equal(img, r["image_spp%d" % it])
                counts = r["counts_it%d" % it]
                assert T.stats()["rays_per_bounce"][: len(counts)] == counts.tolist()
        assert np.array_equal(T.pbo(16), r["pbo_spp16"])
