"""The denoiser's sampled guides (include/mi355x_pathtracer.h: ptx_set_guide_samples; DESIGN.md 10 "Sampled guides") restated in numpy
float32 from per-iteration camera rays and their first hits.  Every operation is one fp32 operation on fp32 arrays -- numpy neither
contracts nor reorders -- so the result is the definition's, bit for bit.

A sample is a dict of per-pixel arrays in the frame's order (pixelIndex = x + y*W): origin, direction (N, 3), t (N,), normal (N, 3),
material, geom (N,) int32, albedo (N, 3).  oracle_samples() takes them from the CPU oracle the way tests/test_gpu_denoise.py takes the
pixel-centre guides: pt_generate(i) with the scene's antialiasing / depth-of-field options, then compute_intersections."""
import numpy as np

G_OBJ = 3          # csrc/pt_device.h: enum { G_SPHERE, G_CUBE, G_TRIANGLE, G_OBJ }
f32 = np.float32


def untextured_albedo(dump, material, geom, hit):
    """write_albedo (csrc/pt_kernels.h) for scenes without textures, from the dumped materials (colour 3, exponent, specular colour 3,
    reflective, refractive, ior, emittance): the colour; on a geom that is not a mesh an emitter's colour x emittance, else a refractive
    material's specular colour.  Misses: 0."""
    m = np.ascontiguousarray(dump["materials"], f32).reshape(-1, 11)
    gtype = np.asarray(dump["geom_ints"], np.int32).reshape(-1, 3)[:, 0]
    mat = np.where(hit, material, 0)
    mm = m[mat]
    a = mm[:, 0:3].copy()
    prim = gtype[np.where(hit, geom, 0)] != G_OBJ
    emit = prim & (mm[:, 10] > 0)
    a[emit] = (mm[emit, 0:3] * mm[emit, 10:11]).astype(f32)
    refr = prim & ~emit & (mm[:, 8] > 0)
    a[refr] = mm[refr, 4:7]
    a[~hit] = 0
    return a.astype(f32)


def oracle_samples(O, dump, iter_first, count, albedo=untextured_albedo):
    """the camera rays of iterations iter_first .. iter_first + count - 1 and their first hits, from an oracle that holds the scene
    with its options set and pt_init() done; albedo(dump, material, geom, hit) -> (N, 3), or None to leave it out"""
    for it in range(iter_first, iter_first + count):
        O.pt_generate(it)
        p = O.paths()
        assert np.array_equal(p["pixelIndex"], np.arange(len(p), dtype=np.int32))
        s = O.compute_intersections(p)
        hit = s["t"] > 0
        yield dict(origin=p["origin"].copy(), direction=p["direction"].copy(), t=s["t"].copy(), normal=s["normal"].copy(),
                   material=s["materialId"].copy(), geom=s["geomId"].copy(),
                   albedo=None if albedo is None else albedo(dump, s["materialId"], s["geomId"], hit))


def sampled_guides(samples):
    """The definition.  samples: the K samples in iteration order.  Returns per-pixel arrays: normal, position, albedo (N, 3), t,
    coverage (N,) float32, hit (N,) bool, material, geom (N,) int32 -- and, for the tests' masks, hits (N,) = H and mixed (N,) bool =
    more than one geom id among the samples that hit."""
    K = 0
    for s in samples:
        t = np.asarray(s["t"], f32)
        if K == 0:
            n = len(t)
            Sn, Sx, Sa = (np.zeros((n, 3), f32) for _ in range(3))
            St = np.zeros(n, f32)
            H = np.zeros(n, np.int32)
            mat, geom = np.zeros(n, np.int32), np.zeros(n, np.int32)
            mixed = np.zeros(n, bool)
            have_albedo = s["albedo"] is not None
        K += 1
        m = t > 0
        first, later = m & (H == 0), m & (H > 0)
        x = (np.asarray(s["origin"], f32) + t[:, None] * np.asarray(s["direction"], f32)).astype(f32)      # o + t*d, as k_gbuffer forms it
        nrm = np.asarray(s["normal"], f32)
        alb = np.asarray(s["albedo"], f32) if have_albedo else np.zeros((n, 3), f32)
        # the sums begin with the first hit sample (an assignment: its -0 survives) and add the later ones in order
        for S, v in ((Sn, nrm), (Sx, x), (Sa, alb)):
            S[first] = v[first]
            S[later] = (S[later] + v[later]).astype(f32)
        St[first] = t[first]
        St[later] = (St[later] + t[later]).astype(f32)
        mat[first], geom[first] = s["material"][first], s["geom"][first]
        mixed |= later & (np.asarray(s["geom"]) != geom)
        H += m
    assert K >= 1
    hit = H > 0
    fh = np.where(hit, H, 1).astype(f32)
    fk = f32(K)
    out = dict(normal=(Sn / fh[:, None]).astype(f32), position=(Sx / fh[:, None]).astype(f32), t=(St / fh).astype(f32),
               albedo=(Sa / fk).astype(f32), coverage=(H.astype(f32) / fk).astype(f32), hit=hit, material=mat, geom=geom, hits=H, mixed=mixed)
    for k in ("normal", "position", "albedo", "t", "coverage", "material", "geom"):
        out[k][~hit] = 0
    return out
