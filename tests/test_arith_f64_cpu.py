"""CPU: the float64 reference of the intersection tests (tests/isect_f64.py) against the oracle, and the oracle against its contracted
build, on the ray families of tests/arithcases.py -- everything the device tier (tests/test_gpu_arith_f64.py) rests on that can be
established without a GPU.

  A = isect_f64: float64, written from the mathematics
  B = the oracle (oracle/libptoracle.so): the bits of arithmetic level 0
  C = the oracle's contracted build (-ffp-contract=fast -mfma): the kind of arithmetic level 1 runs; skipped on a CPU without FMA

Asserted, per subject (a geom under a transform) and family:
  1  A is right.  In the well-conditioned families (arithcases.well_conditioned), on every ray whose decision is clear (isect_f64: margin
     of at least 1e-2, for a miss too; a mesh's runner-up not within 64 u) and that starts within 100 sizes, B agrees with A on hit or
     miss, on the face or side and on the outside flag, and |B - A| in t, point and normal stays within 64 u of the quantity's scale (isect_f64.scales: what the quantity
     is computed from, worked out from the inputs alone).
  2  Which families have ZERO exceptions of B against A over all their rays, clear or not: printed per family ("zero"), because the
     device tier demands zero exceptions of levels 1 and 2 exactly there (it recomputes the same predicate from the same B).
  3  The usable subset S (A and B report the same hit) holds at least 98 % of A's hits, 50 % in the ill-conditioned families
     (arithcases.ill_conditioned), for every family whose accuracy the device tier asserts (all but arithcases.ACCURACY_NOT_ASSERTED,
     where it asserts the opposite: the oracle alone is below the cap, which is the exemption's reason).
  4  The device tier's accuracy rule, C against B with m = 2: on the rays where A, B and C report the same hit, the rms and the 99th
     percentile of |C - A| are at most 2 x max(those of |B - A|, 1 u of the scale), for t (relative to |t_A|), point and normal.

Printed per family: rays, A's hits, clear rays, B's exceptions, |S|, then rms / 99th percentile / maximum of |B - A| in u for t_fwd (t
against its scale), t (relative), point and normal, then C's ratios.

The sphere's far families are left out of rule 1 (arithcases.well_conditioned says why) and printed: the oracle's root formula loses
about R^2 u there, 1e3 u of the scale at 300 sizes."""
import numpy as np
import pytest

import arithcases as ac
import fp_tolerance
import isect_f64 as f64
from cpulibs import OracleLib


@pytest.fixture(scope="module")
def contracted():
    if not fp_tolerance.cpu_has_fma():
        return None
    return OracleLib(fp_tolerance.build_fma_oracle())


def _fmt(s):
    return "%.3g/%.3g/%.3g" % s


@pytest.mark.parametrize("kind,which", ac.SUBJECTS, ids=["%s-%s" % s for s in ac.SUBJECTS])
def test_reference_oracle_and_contracted_oracle(oracle_lib, contracted, kind, which):
    B, C = oracle_lib, contracted
    s = ac.subject(B, kind, which)
    B.create(s["d"], {})
    if C is not None:
        C.create(s["d"], {})
    bad = []
    for name, rays in s["families"].items():
        A = f64.intersect(kind, s["gm"], rays, s["faces"])
        sc = f64.scales(kind, s["gm"], A, rays)
        b10 = B.geom_test(0, rays)
        agree, S = f64.decisions(kind, s["gm"], A, b10)
        hits, exc = int(A["hit"].sum()), int((~agree).sum())
        e = f64.errors(A, b10, rays, S, sc)
        line = "%-6s %-16s %-13s rays %d hits %4d clear %4d exc %4d %s |S| %4d (%.1f %%)  t_fwd %s  t %s  point %s  normal %s" % (
            kind, which, name, len(rays), hits, int(A["clear"].sum()), exc, "zero" if exc == 0 else "    ", int(S.sum()), 100.0 * S.sum() / max(hits, 1),
            _fmt(ac.spread(e["t_fwd"])), _fmt(ac.spread(e["t"])), _fmt(ac.spread(e["point"])), _fmt(ac.spread(e["normal"])))
        assert hits >= 100, (name, hits)                                           # no family passes vacuously
        # 1: A is right
        if ac.well_conditioned(kind, name):
            clear = A["clear"] & (A["away"] <= 100.0)
            assert clear.sum() >= 400, (name, int(clear.sum()))               # (the 1e-2 families sit on the line: about a quarter of theirs)
            if not agree[clear].all():
                bad.append("%s: B disagrees with A on %d clear rays, first %s" % (name, int((~agree[clear]).sum()), np.nonzero(clear & ~agree)[0][:6].tolist()))
            ec = f64.errors(A, b10, rays, S & clear, sc)
            for q in ("t_fwd", "point", "normal"):
                worst = ac.spread(ec[q])[2]
                if not worst <= ac.BOUND_U:
                    bad.append("%s: |B - A| in %s reaches %.3g u of its scale on the clear rays (bound %g)" % (name, q, worst, ac.BOUND_U))
        # 3: S is large enough
        if (kind, which, name) not in ac.ACCURACY_NOT_ASSERTED:
            cap = ac.CAP_ILL if ac.ill_conditioned(kind, name) else ac.CAP
            if S.sum() < cap * hits:
                bad.append("%s: |S| = %d of %d hits, below %.0f %%" % (name, int(S.sum()), hits, 100 * cap))
        else:
            # (the exemption's premise: the oracle alone is below the cap here.  Should that stop being so, the family is to be asserted)
            assert S.sum() < ac.CAP_ILL * hits, "%s: the oracle keeps %d of %d hits: accuracy can be asserted on this family" % (name, int(S.sum()), hits)
        # 4: the accuracy rule, C against B, m = 2
        if C is not None:
            c10 = C.geom_test(0, rays)
            _, Sc = f64.decisions(kind, s["gm"], A, c10)
            both = S & Sc
            ratios = ac.accuracy_ratios(f64.errors(A, b10, rays, both, sc), f64.errors(A, c10, rays, both, sc))
            line += "  C/B " + " ".join("%s %.2f/%.2f" % (q, *ratios[q]) for q in ac.QUANTITIES)
            if (kind, which, name) not in ac.ACCURACY_NOT_ASSERTED:
                for q, (r_rms, r_99) in ratios.items():
                    if max(r_rms, r_99) > 2.0:
                        bad.append("%s: C's %s error is %.2f (rms) / %.2f (99th percentile) x B's, above m = 2" % (name, q, r_rms, r_99))
        print(line)
    assert not bad, "\n".join(bad)


def test_the_reference_is_not_the_oracle_restated():
    """Known answers worked by hand: a unit cube and a unit-diameter sphere at the identity, one triangle."""
    gm = np.concatenate([np.eye(4).ravel()] * 3).astype(np.float32)
    rays = np.float32([[0, 0, 3, 0, 0, -2], [0, 0, 0, 1, 0, 0], [2, 2, 3, 0, 0, -1], [0.25, 0.1, 3, 0, 0, -1]])
    c = f64.cube(gm, rays)
    assert c["hit"].tolist() == [True, True, False, True] and c["outside"].tolist()[:2] == [True, False]
    assert np.allclose(c["t"][[0, 1, 3]], [2.5 - f64.NUDGE, 0.5 - f64.NUDGE, 2.5 - f64.NUDGE], rtol=0, atol=1e-15)
    assert np.allclose(c["normal"][0], [0, 0, 1]) and np.allclose(c["normal"][1], [-1, 0, 0])            # (from inside: against the ray)
    assert np.isclose(c["margin"][3], 0.25) and c["side"].tolist() == [5, 0, -1, 5]
    sp = f64.sphere(gm, rays)
    assert sp["hit"].tolist() == [True, True, False, True] and sp["outside"].tolist()[:2] == [True, False]
    assert np.allclose(sp["t"][:2], [2.5 - f64.NUDGE, 0.5 - f64.NUDGE], rtol=0, atol=1e-15)
    assert np.allclose(sp["normal"][1], [-1, 0, 0])                                                      # (from inside: reversed)
    b = np.hypot(0.25, 0.1)
    assert np.isclose(sp["margin"][3], 1 - b / 0.5) and np.isclose(sp["t"][3], 3 - np.sqrt(0.25 - b * b) - f64.NUDGE)
    # one triangle in the plane z = 0, counter-clockwise seen from +z, texcoords (0,0) (1,0) (0,1); a second one behind it
    tri = np.float32([[0, 0, 0, 0, 0, 1, 0, 0, 1, 0, 0, 1, 0, 0, 1], [0, 0, -1, 0, 0, 1, 0, -1, 1, 0, 0, 1, -1, 0, 1]])
    m = f64.mesh(gm, tri, rays[[3, 2]])
    assert m["hit"].tolist() == [True, False] and m["side"][0] == 0 and np.isclose(m["t"][0], 3.0)
    assert np.allclose(m["uv"][0], [0.25, 0.1]) and np.isclose(m["margin"][0], 0.1) and np.isclose(m["near_t"][0, 1], 4.0)
    assert np.allclose(m["point"][0], [0.25, 0.1, f64.NUDGE]) and np.allclose(m["normal"][0], [0, 0, 1]) and m["outside"][0]
    back = f64.mesh(gm, tri, np.float32([[0.25, 0.1, -3, 0, 0, 1]]))                                    # single-sided: from behind, nothing
    assert not back["hit"][0]
