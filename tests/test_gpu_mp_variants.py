"""The device-resident engine's multiphase pass (pair_compute_mp, csrc/sph_engine_step.h) on
jittered two- and three-phase boxes, every gather family and style subset, under the strict
bar of mp_variants_util (1e-10 normwise and per element, the oracle's reordering / one-ulp
spread only, exact zeros where the oracle's field is zero).

pair_compute_mp picks one of three gather families -- k_mp2_gather_w4 (symmetric styles, every
gamma 1), k_mp2_gather<POW> (symmetric, one gamma != 1), k_mp_gather (unequal gammas, or a type
pinned to Tc against its own type) -- each instantiated for the seven non-empty subsets of
taitwater / surfacetension / heatconduction, and sums rhosum/multiphase either inside the list
fill (rebuild steps) or in k_mp2_rhosum.  The C5 tests (bubble_physics) reach one of those 21
gathers, with every cutoff equal, no background pressure, Tc 0, nstep 1, two types and atoms
at rest on a lattice.  Here every case states its premise on the oracle or the tables first,
then asserts the path through Engine.stats()["flags"] (STAT_MP_*), then the fields.

Which instantiations an engine can reach: the gammas reach the engine only with taitwater on
(mp_config / coef_mp), so without taitwater every gamma is 0 there -- equal, not 1 -- and the
pass takes k_mp2_gather<POW> with TAIT = false (pow is never evaluated); k_mp_gather without
taitwater needs the own-type pin and so heatconduction.  Reached here: w4 x {T, TS, TH, TSH},
POW x all seven, k_mp_gather x {T, TS, TH, TSH, H, SH}: 17 of 21.  k_mp2_gather_w4 x {S, H,
SH} and k_mp_gather x {S} cannot be launched by any configuration.

Every case is compared at setup, after step 1 (a forward-comm step: skin 0.3, rebuild every 2)
and after step 3 (past a rebuild); `nstep` at every step to 6."""
import functools

import numpy as np
import pytest

from c5_util import bricks_step, mp_bricks, mp_collect, mp_engine, mp_state
from mp_variants_util import (CUTS, FIELDS, GAMMAS, check_fields_strict, mp_box, mp_physics,
                              oracle_caps, oracle_run)

import pyoracle as po

AT = (0, 1, 3)
# name -> (box, physics, compared steps, gather family)
CASES = {
    "g1": (dict(), dict(), AT, "W4"),
    "uneqcut": (dict(), dict(cuts="uneq"), AT, "W4"),
    "uneqcut2": (dict(), dict(cuts="uneq2"), AT, "W4"),
    "pow": (dict(), dict(gamma="pow"), AT, "POW"),
    "asym": (dict(), dict(gamma="asym"), AT, "ROW"),
    "diag": (dict(), dict(diag=True), AT, "ROW"),
    "nstep": (dict(), dict(rhosum_nstep=2, cg_nstep=3), tuple(range(7)), "W4"),
    "nt3": (dict(ntypes=3), dict(ntypes=3, cuts="uneq"), AT, "W4"),
    "2d-g1": (dict(dim=2), dict(), AT, "W4"),
    "2d-asym": (dict(dim=2), dict(gamma="asym"), AT, "ROW"),
}
SUBSETS = [(t, s, h) for t in (True, False) for s in (True, False) for h in (True, False)
           if (t or s or h) and not (t and s and h)]


def _sub_id(sub):
    return "".join(c for c, on in zip("TSH", sub) if on)


for _sub in SUBSETS:
    for _g, _fam in (("g1", "W4"), ("pow", "POW"), ("asym", "ROW")):
        # (without taitwater the engine holds no gammas: equal, not 1 -> POW; module doc)
        CASES[f"sub-{_sub_id(_sub)}-{_g}"] = (
            dict(), dict(gamma=_g, tait=_sub[0], st=_sub[1], heat=_sub[2]), (0, 1),
            _fam if _sub[0] else "POW")
    if _sub[2] and not _sub[0]:   # k_mp_gather without taitwater: the own-type pin
        CASES[f"sub-{_sub_id(_sub)}-diag"] = (
            dict(), dict(diag=True, tait=False, st=_sub[1], heat=True), (0, 1), "ROW")
BRICKS = {"bricks-asym": (dict(), dict(gamma="asym"), AT, "ROW"),
          "bricks-uneqcut": (dict(), dict(cuts="uneq"), AT, "W4")}
PG = (2, 1, 1)


@functools.lru_cache(maxsize=None)
def case(name):
    """(system, physics, the oracle's frozen snapshots, family) of a case, computed once"""
    box, phys, at, fam = (BRICKS if name in BRICKS else CASES)[name]
    s = mp_box(**box)
    ph = mp_physics(**phys)
    snaps = oracle_run(s, ph, at, procgrid=PG if name in BRICKS else None)
    return s, ph, snaps, fam


def premises(name, s, ph, snaps):
    """What the case is about, read off the tables and the oracle's pairs."""
    _, phys, _, fam = (BRICKS if name in BRICKS else CASES)[name]
    nt = s.ntypes
    assert s.n == (343 if s.dim == 3 else 144) and nt == phys.get("ntypes", 2)
    assert sorted(set(s.type.tolist())) == list(range(1, nt + 1))
    assert np.abs(s.v).max() > 0.05 and np.ptp(s.rmass / s.rho) > 0.05
    assert (ph.rbg[1:] != 0).all() and ph.skin == 0.3 and ph.every == 2 and ph.pc is None
    g = ph.gamma[1:]
    gk = phys.get("gamma", "g1")
    if gk == "g1":
        assert (g == 1.0).all()
    elif gk == "pow":
        assert (g == g[0]).all() and g[0] != 1.0
    else:
        assert len(set(g.tolist())) == nt
    # the engine's family by its own rule (mp2_symmetric / mp2_gamma1) on what it is given
    eg = g if ph.tait else np.zeros(nt)
    pin = any(ph.heat_fixflag[t, t] == t for t in range(1, nt + 1))
    want = "ROW" if (len(set(eg.tolist())) > 1 or pin) else "W4" if (eg == 1.0).all() else "POW"
    assert want == fam, (name, want, fam)
    assert pin == bool(phys.get("diag"))
    cuts = CUTS[phys.get("cuts", "eq")]
    if phys.get("cuts") == "uneq":
        assert cuts[3] != cuts[2] and cuts[4] != cuts[2] and cuts[0] == max(cuts)
    if phys.get("cuts") == "uneq2":
        assert cuts[2] == min(cuts)
        assert all(sn.st_not_tait > 100 for sn in snaps.values())   # cs && !ct pairs
    else:
        assert all(sn.st_not_tait == 0 for sn in snaps.values())
    if ph.heat:   # the pinned temperature is taken by some pair at every compared step
        assert ph.heat_fixflag[1, 2] == 2 and ph.heat_tc[1, 2] == 0.5
        assert all(sn.pinned >= 1 for sn in snaps.values()), name
    for sn in snaps.values():   # a style that is off leaves its field exactly zero
        assert (not sn.field("de").any()) == (not ph.heat)
        assert (not sn.field("f").any()) == (not (ph.tait or ph.st))
    if "nstep" in name:
        assert ph.rhosum_nstep == 2 and ph.cg_nstep == 3 and max(snaps) == 6
        # between two due steps rho and the colour gradient stand still
        assert np.array_equal(snaps[0].field("rho"), snaps[1].field("rho"))
        assert np.array_equal(snaps[3].field("cg"), snaps[5].field("cg"))
        assert not np.array_equal(snaps[0].field("rho"), snaps[2].field("rho"))
        assert not np.array_equal(snaps[0].field("cg"), snaps[3].field("cg"))


ALL = sorted(CASES) + sorted(BRICKS)


def test_case_list():
    """every row of the case table: 10 named cases, 6 subsets x 3 gammas (+ the two own-type
    pins that reach k_mp_gather without taitwater), two brick cases"""
    subs = [n for n in CASES if n.startswith("sub-")]
    assert len(SUBSETS) == 6 and len(subs) == 20 and len(CASES) == 30 and len(BRICKS) == 2
    reached = {(CASES[n][3], _sub_id((CASES[n][1].get("tait", True), CASES[n][1].get("st", True),
                                      CASES[n][1].get("heat", True)))) for n in CASES}
    assert len(reached) == 17, sorted(reached)


@pytest.mark.parametrize("name", ALL)
def test_oracle_caps(po, name):
    """The inputs keep the strict bar meaningful (mp_variants_util.oracle_caps), and every
    case's premise holds -- on the oracle alone, so a bad seed shows without a GPU."""
    s, ph, snaps, fam = case(name)
    premises(name, s, ph, snaps)
    for step, sn in snaps.items():
        caps = oracle_caps(sn, FIELDS, (name, step))
        for k, c in caps.items():
            if not c.get("zero"):
                print(f"[mp caps] {name} step {step} {k}: spread {c['spread']:.1e} "
                      f"wide {c['wide']} worst bar {c['worst_bar']:.1e}")


def fam_of(eng, flags):
    return "|".join(n for n in ("W4", "POW", "ROW") if flags & getattr(eng, "STAT_MP_" + n))


def check_path(eng, ph, fam, step, where):
    """the family bit, and where rhosum was summed: inside the list fill when it is due on a
    rebuild step (every 2 from setup), by k_mp2_rhosum when due on a forward-comm step"""
    fl = eng.stats()["flags"]
    assert fam_of(eng, fl) == fam, (where, fam_of(eng, fl))
    due = step % ph.rhosum_nstep == 0
    last_due = step - step % ph.rhosum_nstep
    assert bool(fl & eng.STAT_RHO_FUSED) == (due and step % ph.every == 0), (where, fl)
    assert bool(fl & eng.STAT_MP_RHO_LISTFILL) == (last_due % ph.every == 0), (where, fl)
    return fl


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_mp_variant(gpu, sph_amd, name):
    s, ph, snaps, fam = case(name)
    premises(name, s, ph, snaps)
    eng = mp_engine(sph_amd, s, ph)
    try:
        seen = []
        for step in range(max(snaps) + 1):
            if step == 0:
                eng.setup()
            else:
                eng.run(1)
            seen.append(check_path(eng, ph, fam, step, (name, step)))
            if step not in snaps:
                continue
            sn = snaps[step]
            g = mp_state(eng)
            assert g["x"].shape[0] == sn.n and np.array_equal(g["type"], sn.type)
            assert np.array_equal(eng.neighbor_counts(), sn.counts), (name, step)
            check_fields_strict(g, sn, FIELDS, (name, step))
        print(f"[mp variants] {name}: {fam} flags by step {[hex(f) for f in seen]}")
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(BRICKS))
def test_mp_variant_bricks(gpu, sph_amd, name):
    """procgrid (2,1,1): a neighbour across the brick face is a ghost with its rho and colour
    gradient as communicated where one process sees it fresh (the oracle's per-rank view), so
    the gather's fresh / stale choice and forward_fresh's pack / unpack carry the result."""
    s, ph, snaps, fam = case(name)
    premises(name, s, ph, snaps)
    one = case(name[len("bricks-"):])[2]   # (the same physics on one process differs)
    assert not np.array_equal(one[1].field("f"), snaps[1].field("f"))
    world, engines = mp_bricks(sph_amd, s, ph, PG, po.brick_owner(s, s.x, PG))
    try:
        for step in range(max(snaps) + 1):
            bricks_step(engines, (lambda e: e.setup()) if step == 0 else (lambda e: e.run(1)))
            for e in engines:
                assert fam_of(e, e.stats()["flags"]) == fam, (name, step)
            if step not in snaps:
                continue
            sn = snaps[step]
            out = mp_collect(engines, sn.n)
            assert np.array_equal(out["type"], sn.type)
            assert np.array_equal(out["counts"], sn.counts), (name, step)
            check_fields_strict(out, sn, FIELDS, (name, step))
    finally:
        for e in engines:
            e.close()
        world.close()


@pytest.mark.gpu
def test_mp_zero_gamma_rejected(gpu, sph_amd):
    """taitwater/multiphase divides by gamma (B = c0^2 rho0 / gamma): a zero is refused at
    create, not carried into the tables."""
    s = mp_box()
    ph = mp_physics()
    ph.gamma = np.array([0.0, 1.0, 0.0])
    with pytest.raises(sph_amd.HipError, match="gamma and rho0 must be non-zero"):
        mp_engine(sph_amd, s, ph)
