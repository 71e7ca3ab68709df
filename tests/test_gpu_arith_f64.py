"""GPU: arithmetic levels 0, 1 and 2 against the float64 reference of the same operation (tests/isect_f64.py), on the ray families of
tests/arithcases.py -- what tests/test_arith_f64_cpu.py establishes for the oracle and its contracted build on the host, here for the
three code objects of the device.  tests/test_gpu_arith.py bounds a level's distance to level 0; this module asks whether a level is
further from the TRUTH than level 0 is.

A = the float64 reference, B = the oracle (level 0's bits), L0 / L1 / L2 = Tracer.geom_test of a tracer of that level on a one-geom scene.

Stage level (test_levels_against_the_float64_reference), per subject and family:
  guard      L0 equals B bit for bit: the three tracers see the scene the reference sees.
  decisions  where B has no exception against A over the whole family (the host tier prints which: "zero"), L1 and L2 agree with A on
             hit or miss, on the face or side and on the outside flag for every ray; elsewhere a level's disagreements with A number at
             most 2 x level 0's + 4.
  accuracy   on S_L (A, L0 and L report the same hit; at least 98 % of A's hits, 50 % in the ill-conditioned families), for t relative
             to |t_A|, point and normal against their scales (isect_f64.scales):
                 rms(|L - A|) <= m_L max(rms(|L0 - A|), 1 u)      and the same for the 99th percentile,
             m_1 = 2: contraction only removes roundings, every remaining operation rounds as before, so the budget is level 0's and
             the factor is for different error draws;  m_2 = 8: pt_device.h states one ulp for the hardware's seeds against half an ulp
             and 2.5 ulp for a * rcp(b) against half an ulp, so 5, with margin.  Maxima are printed, not asserted.

Mesh routes (test_mesh_routes_at_every_level): the same rays through compute_intersections, tile_intersect(split=False) and
tile_intersect(split=True) under the four plans of tests/test_gpu_mesh_walks.py, the plan asserted against that module's EXPECT, at
levels 0, 1 and 2 -- every single-lane walk (loop, skip, ordered, wide) at every level.  Per walk and family:
  face rule  the walk returns A's face, or one whose float64 distance is within 64 u (relative) of A's winner;
  miss rule  the walk reports no miss where A has a hit with a margin of at least 1e-4 whose runner-up is not within 64 u -- what a
             too-small slack of the tree's boxes would break.
Both hold without exception where B has none against A.  Elsewhere -- from 1e3 sizes away the fp32 origin no longer resolves the faces,
and level 0 breaks both rules itself: it takes a neighbour where another arithmetic misses, so the two kinds trade -- a level's
violations of both kinds together number at most 2 x level 0's on the same route + 4, and the miss rule is held against the level's
OWN loop over all faces (the same tracer under no_bvh): on no ray of any family, at any level, does a walk through the tree miss a
solid hit of A that the loop of that level finds.  That is "the tree equals the loop" where the arithmetic is not IEEE.  (Under no_bvh
there is no tree, and tile_intersect's loop, chunked over lanes, is another instantiation than the single-lane one: at level 2 the two
round differently from 1e5 sizes away, where one ulp of a direction is a hundredth of a size -- measured 9 and 4 of 4096 rays of
hull_cut24 / hull_cut25 lost by one and as many found by the other; the rule on the totals covers them.)"""
import numpy as np
import pytest

import arithcases as ac
import isect_f64 as f64
import test_gpu_mesh_walks as mw
from conftest import beq
from test_gpu_parity import O, fences_stay_silent      # noqa: F401  (fixtures; the fence check is autouse)

pytestmark = pytest.mark.gpu

M = {1: 2.0, 2: 8.0}
assert (mw.TRS_ROT, mw.TRS_SMALL, mw.TRS_FLAT) == (ac.TRANSFORMS["rot"], ac.TRANSFORMS["small"], ac.TRANSFORMS["flat"])

_REF = {}        # per subject: the scene, the families and, per family, A, its scales and B's answers -- computed once, read only


def reference(O, kind, which):
    if (kind, which) not in _REF:
        s = ac.subject(O, kind, which)
        O.create(s["d"], {})
        s["ref"] = {}
        for name, rays in s["families"].items():
            A = f64.intersect(kind, s["gm"], rays, s["faces"])
            b10 = O.geom_test(0, rays)
            agree, S = f64.decisions(kind, s["gm"], A, b10)
            s["ref"][name] = dict(A=A, sc=f64.scales(kind, s["gm"], A, rays), b10=b10, zero=bool(agree.all()), exc_b=int((~agree).sum()))
        _REF[(kind, which)] = s
    return _REF[(kind, which)]


@pytest.mark.parametrize("kind,which", ac.SUBJECTS, ids=["%s-%s" % s for s in ac.SUBJECTS])
def test_levels_against_the_float64_reference(gpu_product, O, kind, which):
    s = reference(O, kind, which)
    tracers = {lv: gpu_product.Tracer.from_pod(s["d"], arith=lv) for lv in (0, 1, 2)}
    bad = []
    try:
        for name, rays in s["families"].items():
            r = s["ref"][name]
            A, sc = r["A"], r["sc"]
            got = {lv: T.geom_test(0, rays) for lv, T in tracers.items()}
            assert beq(got[0], r["b10"]), "%s: level 0 on the device is not the oracle on %d rays" % (
                name, int((got[0].view(np.uint32) != r["b10"].view(np.uint32)).any(axis=1).sum()))
            hits = int(A["hit"].sum())
            dec = {lv: f64.decisions(kind, s["gm"], A, got[lv]) for lv in got}
            exc = {lv: int((~dec[lv][0]).sum()) for lv in got}
            line = "%-6s %-16s %-13s hits %4d  exceptions B/L0/L1/L2 %d/%d/%d/%d%s" % (kind, which, name, hits, r["exc_b"], exc[0], exc[1], exc[2], " zero" if r["zero"] else "")
            for lv in (1, 2):
                if r["zero"]:
                    if exc[lv]:
                        bad.append("%s level %d: %d decisions differ from A in a zero-exception family, first rays %s" % (
                            name, lv, exc[lv], np.nonzero(~dec[lv][0])[0][:6].tolist()))
                elif exc[lv] > 2 * exc[0] + 4:
                    bad.append("%s level %d: %d decisions differ from A, level 0 has %d" % (name, lv, exc[lv], exc[0]))
                SL = dec[0][1] & dec[lv][1]
                e0, eL = f64.errors(A, got[0], rays, SL, sc), f64.errors(A, got[lv], rays, SL, sc)
                ratios = ac.accuracy_ratios(e0, eL)
                line += "  | L%d |S| %4d (%.1f %%)" % (lv, int(SL.sum()), 100.0 * SL.sum() / max(hits, 1))
                line += " " + " ".join("%s %.2f/%.2f max %.3g/%.3g u" % (q, *ratios[q], ac.spread(eL[q])[2], ac.spread(e0[q])[2]) for q in ac.QUANTITIES)
                if (kind, which, name) in ac.ACCURACY_NOT_ASSERTED:
                    continue
                cap = ac.CAP_ILL if ac.ill_conditioned(kind, name) else ac.CAP
                if SL.sum() < cap * hits:
                    bad.append("%s level %d: |S| = %d of %d hits, below %.0f %%" % (name, lv, int(SL.sum()), hits, 100 * cap))
                for q, (r_rms, r_99) in ratios.items():
                    if max(r_rms, r_99) > M[lv]:
                        bad.append("%s level %d: the error of %s is %.2f (rms) / %.2f (99th percentile) x level 0's, above m = %g" % (name, lv, q, r_rms, r_99, M[lv]))
            print("\n" + line, end="")
    finally:
        for T in tracers.values():
            T.close()
    assert not bad, "\n".join(bad)


def _violations(A, isects):
    """-> (face rule violations, miss rule violations, A's solid hits) of one route's answers, boolean per ray"""
    out10 = np.zeros((len(isects), 10))
    out10[:, 0], out10[:, 4:7] = isects["t"], isects["normal"]
    side = f64.side_of("mesh", None, A, out10)
    rows = np.arange(len(side))
    with np.errstate(invalid="ignore"):
        k = (A["near_face"] == side[:, None]).argmax(axis=1)
        known = (A["near_face"] == side[:, None]).any(axis=1) & (side >= 0)
        near_enough = known & (A["near_t"][rows, k] <= A["near_t"][:, 0] * (1 + 64 * f64.U))
        face_bad = (side != -1) & ~near_enough
        solid = A["hit"] & (A["margin"] >= 1e-4) & ~(A["near_t"][:, 1] <= A["near_t"][:, 0] * (1 + 64 * f64.U))
    return face_bad, (side == -1) & solid, solid


_LOOP = {}       # per (case, level, family): the level's loop over all faces (the tracer under no_bvh), computed once


def loop_answers(pt, monkeypatch, s, case, lv):
    if (case, lv) not in _LOOP:
        with mw.open_tracer(pt, monkeypatch, s["d"], "no_bvh", arith=lv) as T:
            assert T.mesh_plan(0)["frame_walk"] == "loop"
            _LOOP[(case, lv)] = {name: T.compute_intersections(mw.kat_paths(rays))["t"] for name, rays in s["families"].items()}
    return _LOOP[(case, lv)]


@pytest.mark.parametrize("plan", list(mw.PLANS))
@pytest.mark.parametrize("case", ac.MESH_CASES)
def test_mesh_routes_at_every_level(gpu_product, O, monkeypatch, case, plan):
    s = reference(O, "mesh", case)
    split, frame_walk, stack_walk = mw.EXPECT[(case, plan)]
    counts, bad = {}, []
    for lv in (0, 1, 2):
        loop = loop_answers(gpu_product, monkeypatch, s, case, lv)
        with mw.open_tracer(gpu_product, monkeypatch, s["d"], plan, arith=lv) as T:
            pl = T.mesh_plan(0)
            assert (bool(pl["split"]), pl["frame_walk"], pl["stack_walk"]) == (split, frame_walk, stack_walk), (lv, pl)
            for name, rays in s["families"].items():
                p = mw.kat_paths(rays)
                routes = {"compute_intersections [%s]" % ("skip" if pl["root"] >= 0 else "loop"): T.compute_intersections(p),
                          "tile_intersect(split=False) [%s]" % ("skip" if pl["root"] >= 0 else "loop"): T.tile_intersect(p, split=False)}
                if pl["root"] >= 0:
                    routes["tile_intersect(split=True) [%s]" % stack_walk] = T.tile_intersect(p, split=True)
                for route, got in routes.items():
                    if lv == 0:                                         # (level 0: every route is the oracle's loop, bit for bit)
                        assert beq(got["t"], s["ref"][name]["b10"][:, 0]), (name, route)
                    assert ((got["t"] > 0) <= (got["geomId"] == 0)).all()
                    f, m, solid = _violations(s["ref"][name]["A"], got)
                    counts[(name, route, lv)] = (int(f.sum()), int(m.sum()), np.nonzero(f | m)[0][:6].tolist())
                    lost = (got["t"] <= 0) & (loop[name] > 0) & solid
                    if lost.any() and pl["root"] >= 0:                  # (a walk through a tree; under no_bvh there is none)
                        bad.append("%s %s level %d: the walk misses %d solid hits that the level's loop over all faces finds, first rays %s" % (
                            name, route, lv, int(lost.sum()), np.nonzero(lost)[0][:6].tolist()))
    for (name, route, lv), (nf, nm, first) in sorted(counts.items()):
        f0, m0, _ = counts[(name, route, 0)]
        print("\n%-16s %-13s %-13s %-40s level %d  face rule %4d  miss rule %4d%s" % (case, plan, name, route, lv, nf, nm, "  zero" if s["ref"][name]["zero"] else ""), end="")
        if lv == 0:
            continue
        if s["ref"][name]["zero"]:
            if nf or nm:
                bad.append("%s %s level %d: %d face / %d miss violations where the oracle has none, first rays %s" % (name, route, lv, nf, nm, first))
        elif nf + nm > 2 * (f0 + m0) + 4:
            bad.append("%s %s level %d: %d face + %d miss violations, level 0 has %d + %d" % (name, route, lv, nf, nm, f0, m0))
    assert not bad, "\n".join(bad)
