"""fix setforce / fix addforce and the layer profiles on the device-resident engine, against
the oracle's Verlet drivers with the fixes applied in numpy where LAMMPS runs post_force
(forcefix_util.forced_oracle; its preconditions are test_forcefix_cpu.py's).

Bars: conftest.check_fields at 1e-10 (normwise, and elementwise against the oracle's
reordering / one-ulp shadows, every shadow with the fixes armed), atom counts, insertions,
types and neighbour counts exact, set force components bit for bit.  Profiles and reductions
against numpy on the engine's own arrays: counts exact, |sum - fsum| <= 1e-13 sum|q| per
layer (a fold of N <= 2^24 doubles in any fixed shape is within ~24 * 1.1e-16 sum|q|), two
calls identical bits.  Tallies: the ranks' totals added against the oracle's pre-fix force
summed over the selection, within 1e-10 sum|f|."""
import math

import numpy as np
import pytest

import pyoracle as po
from c5_util import bricks_step, mp_bricks, mp_collect, mp_engine, mp_state
from conftest import check_fields
from forcefix_util import (BRICKS_PG, C3_ADD, C3_G, ORDER_ADD, ORDER_SET, POISEUILLE_DELTA, arm,
                           bricks_case, buoyancy_case, c3_walls_case, forced_oracle, foriginal,
                           nevery_case, np_layer, order_case, poiseuille_case)
from setmeso_util import arm as arm_clamps
from setmeso_util import c3_engine, np_selected

pytestmark = pytest.mark.gpu
TOL = 1e-10
C3_FIELDS = ("x", "v", "rho", "e", "f", "drho", "de")
MP_FIELDS = ("x", "v", "rho", "e", "rmass", "cv", "cg", "f", "de")


def _compare_mp(g, ref, counts, where=""):
    s = ref.s
    assert g["x"].shape[0] == s.n and g["ninserted"] == ref.ninserted
    assert np.array_equal(g["type"], s.type)
    assert np.array_equal(counts, ref.numneigh_full()), where
    check_fields(g, ref, MP_FIELDS, TOL, where=where)


# ---- 1. single-phase frozen walls and body forces -------------------------------------------
@pytest.mark.parametrize("path", [0, 1])
@pytest.mark.parametrize("nsteps", [5, 12])
def test_c3_walls_and_body_forces(gpu, sph_amd, path, nsteps):
    """setforce 0 0 0 on the walls, setforce NULL 0 0 in a block, a constant addforce in a
    sphere and a per-mass body force on the fluid, in one launch; both pair paths; 5 steps
    cross no rebuild, 12 cross one"""
    s, ph, fixes = c3_walls_case(sph_amd)
    ref = forced_oracle(s, ph, fixes)
    ref.setup()
    eng = c3_engine(sph_amd, s, ph, path)
    arm(eng, fixes)
    eng.setup()
    check_fields(eng.get_atoms(), ref, C3_FIELDS, TOL, where="setup")
    ref.run(nsteps)
    eng.run(nsteps)
    g = eng.get_atoms()
    assert np.array_equal(eng.neighbor_counts(), ref.numneigh_full())
    check_fields(g, ref, C3_FIELDS, TOL, where=f"step {nsteps}")   # (drho: fo.w left alone)
    if path == 0:
        assert eng.stats()["staged"] == 1
    wall = s.type == 2
    assert np.array_equal(g["x"][wall], s.x[wall]) and np.array_equal(g["v"][wall], s.v[wall])
    assert wall.any() and not g["f"][wall].any()
    # fluid in the block and outside the sphere: NULL 0 0, then mass * g on top, bit for bit
    blk = np_selected(fixes[1], g["x"], s.type)
    m = blk & ~np_selected(fixes[2], g["x"], s.type)
    assert m.any()
    assert np.all(g["f"][m, 1] == 0.0 + s.mass[1] * C3_G[1])
    assert np.all(g["f"][m, 2] == 0.0 + s.mass[1] * C3_G[2])
    # ... and inside the sphere the constant force as well, in call order
    m = blk & np_selected(fixes[2], g["x"], s.type)
    assert m.any()
    assert np.all(g["f"][m, 1] == (0.0 + C3_ADD[1]) + s.mass[1] * C3_G[1])
    assert np.all(g["f"][m, 2] == (0.0 + C3_ADD[2]) + s.mass[1] * C3_G[2])


# ---- 2. order -------------------------------------------------------------------------------
@pytest.mark.parametrize("set_first", [True, False])
def test_call_order(gpu, sph_amd, set_first):
    """overlapping selections: set then add leaves value + add, add then set leaves value"""
    s, ph, fixes = order_case(sph_amd, set_first)
    ref = forced_oracle(s, ph, fixes)
    ref.setup()
    eng = c3_engine(sph_amd, s, ph, 0)
    arm(eng, fixes)
    eng.setup()
    for step in (0, 2):
        if step:
            ref.run(step)
            eng.run(step)
        g = eng.get_atoms()
        check_fields(g, ref, C3_FIELDS, TOL, where=f"step {step}")
        a = np_selected(fixes[0 if set_first else 1], g["x"], s.type)   # the setforce
        b = np_selected(fixes[1 if set_first else 0], g["x"], s.type)   # the addforce
        both, only_set = a & b, a & ~b
        assert both.any() and only_set.any()
        want = (np.array(ORDER_SET) + np.array(ORDER_ADD)) if set_first else np.array(ORDER_SET)
        assert np.all(g["f"][both] == want), step
        assert np.all(g["f"][only_set] == np.array(ORDER_SET)), step


# ---- 3. nevery ------------------------------------------------------------------------------
def test_addforce_every_three(gpu, sph_amd):
    """the fix acts in the steps with ntimestep % 3 == 0, setup's step 0 included: the oracle
    applies it at 0, 3 and 6 only, and f is compared after every step"""
    s, ph, fixes = nevery_case(sph_amd)
    ref = forced_oracle(s, ph, fixes)
    ref.setup()
    eng = c3_engine(sph_amd, s, ph, 0)
    arm(eng, fixes)
    eng.setup()
    for step in range(8):
        if step:
            ref.run(1)
            eng.run(1)
        check_fields(eng.get_atoms(), ref, C3_FIELDS, TOL, where=f"step {step}")
    assert ref.ff_applied == [(0, 0), (3, 0), (6, 0)]


# ---- 4. Poiseuille-shaped multiphase run, profiles ------------------------------------------
def _check_profile(eng, g, axis, lo, delta, n, box, sel=None):
    sel = sel or {}
    quant = dict(vx=g["v"][:, 0], rho=g["rho"])
    count, sums = eng.profile(axis, lo, delta, n, ["vx", "rho"], **sel)
    count2, sums2 = eng.profile(axis, lo, delta, n, ["vx", "rho"], **sel)
    assert np.array_equal(count, count2) and sums.tobytes() == sums2.tobytes()
    m = np_selected(sel, g["x"], g["type"])
    lay = np_layer(g["x"][:, axis], lo, delta, n, box[0], box[1], True)
    assert np.array_equal(count, np.bincount(lay[m], minlength=n))
    for k, name in enumerate(("vx", "rho")):
        for L in range(n):
            q = quant[name][m & (lay == L)]
            assert abs(sums[k, L] - math.fsum(q)) <= 1e-13 * math.fsum(np.abs(q)), (name, L)
    return count, sums


@pytest.mark.parametrize("dim", [2, 3])
def test_poiseuille_multiphase_and_profiles(gpu, sph_amd, dim):
    s, ph, fixes = poiseuille_case(sph_amd, dim)
    ref = forced_oracle(s, ph, fixes, builds=False)
    ref.setup()
    eng = mp_engine(sph_amd, s, ph)
    arm(eng, fixes)
    with pytest.raises(sph_amd.HipError) as ei:     # (valid after setup only)
        eng.profile(1, 0.0, 1.0, 4, ["vx"])
    assert ei.value.code == -1
    eng.setup()
    _compare_mp(mp_state(eng), ref, eng.neighbor_counts(), "setup")
    for step in range(1, 7):
        ref.run(1)
        eng.run(1)
        _compare_mp(mp_state(eng), ref, eng.neighbor_counts(), f"step {step}")
    g = mp_state(eng)
    assert not g["f"][g["type"] == 2].any()
    box = (s.boxlo[1], s.boxhi[1])
    lo, n = sph_amd.layers("lower", POISEUILLE_DELTA, *box)
    count, sums = _check_profile(eng, g, 1, lo, POISEUILLE_DELTA, n, box)
    assert count.sum() == s.n and count.min() > 0
    _check_profile(eng, g, 1, lo, POISEUILLE_DELTA, n, box, dict(types=[1]))
    _check_profile(eng, g, 1, lo, POISEUILLE_DELTA, n, box, dict(types=[1], region=fixes[0]["region"]))
    c1, s1 = eng.profile("y", lo, POISEUILLE_DELTA, n, ["vx"], types=[1])   # (axis by name)
    c2, s2 = eng.profile(1, lo, POISEUILLE_DELTA, n, ["vx"], types=[1])
    assert np.array_equal(c1, c2) and s1.tobytes() == s2.tobytes()
    # compute reduce ave vx (poiseuille.lmp:65) and its siblings against numpy
    out = eng.reduce([dict(quantity=q, types=[1]) for q in ("vx", "vy", "vz")])
    fl = g["type"] == 1
    for d, o in enumerate(out):
        q = g["v"][fl, d]
        assert o["count"] == int(fl.sum()) and o["min"] == q.min() and o["max"] == q.max()
        assert abs(o["sum"] - math.fsum(q)) <= 1e-13 * math.fsum(np.abs(q))
    # layers that stop short of the box: an atom outside [lo, lo + nlayers delta) counts in
    # the edge layer.  One atom above the window and one below it, each picked alone by a
    # small sphere around it
    wlo, wn = 2.0, 3
    for i, edge in ((int(np.argmax(g["x"][:, 1])), wn - 1), (int(np.argmin(g["x"][:, 1])), 0)):
        assert not wlo <= g["x"][i, 1] < wlo + wn * 1.0
        alone = sph_amd.sphere(g["x"][i], 1e-3)
        assert np_selected(dict(region=alone), g["x"], g["type"]).sum() == 1
        c, sm = eng.profile(1, wlo, 1.0, wn, ["vx"], region=alone)
        want = np.zeros(wn, dtype=np.int64)
        want[edge] = 1
        assert np.array_equal(c, want) and sm[0, edge] == g["v"][i, 0]
    c, _ = _check_profile(eng, g, 1, wlo, 1.0, wn, box)
    assert c.sum() == s.n
    # argument checks
    for bad in (dict(axis=3), dict(delta=0.0), dict(delta=-1.0), dict(nlayers=0),
                dict(quantities=["vx"] * 9), dict(quantities=[10]), dict(quantities=[-1])):
        kw = dict(axis=1, lo=0.0, delta=1.0, nlayers=4, quantities=["vx"])
        kw.update(bad)
        with pytest.raises(sph_amd.HipError) as ei:
            eng.profile(**kw)
        assert ei.value.code == -1, bad


# ---- 5. the C5 stack with fix phase_change --------------------------------------------------
def test_c5_buoyancy_with_phase_change(gpu, sph_amd):
    """bubble.lmp:188's buoyancy on the gas beside the far-field clamp and fix phase_change:
    an atom created in a step carries mass * g in that step's f"""
    s, ph, clamps, fixes, _ = buoyancy_case(sph_amd)
    ref = forced_oracle(s, ph, fixes, clamps=clamps)
    ref.setup()
    eng = mp_engine(sph_amd, s, ph)
    arm_clamps(eng, clamps)
    arm(eng, fixes)
    eng.setup()
    _compare_mp(mp_state(eng), ref, eng.neighbor_counts(), "setup")
    seen_new = 0
    for step in range(1, 6):
        n0 = ref.s.n
        ref.run(1)
        eng.run(1)
        g = mp_state(eng)
        _compare_mp(g, ref, eng.neighbor_counts(), f"step {step}")
        new = np.arange(n0, ref.s.n)
        if new.size:    # created in this step: of the gas type, selected, and carrying the force
            seen_new += new.size
            assert (g["type"][new] == 2).all()
            # (check_fields above holds f to the oracle's; this says what that f contains: the
            # oracle's pre-fix force plus mass * g, which a missing fix would leave out whole)
            add = ref.s.rmass[new, None] * np.array(fixes[0]["value"])
            assert np.array_equal(ref.f[new], ref.ff_pre[0][new] + add)
            assert np.abs(g["f"][new, 1] - ref.f[new, 1]).max() <= 1e-3 * np.abs(add[:, 1]).min()
    assert ref.ninserted >= 1 and seen_new == ref.ninserted


# ---- 6. two bricks --------------------------------------------------------------------------
def _bricks_run(sph_amd, s, ph, fixes, ref=None, nsteps=3):
    world, engines = mp_bricks(sph_amd, s, ph, BRICKS_PG, po.brick_owner(s, s.x, BRICKS_PG))
    totals = []
    try:
        ids = [arm(e, fixes) for e in engines][0]
        for step in range(nsteps + 1):
            bricks_step(engines, (lambda e: e.setup()) if step == 0 else (lambda e: e.run(1)))
            if ref is not None:
                if step:
                    ref.run(1)
                out = mp_collect(engines, ref.s.n)
                _compare_mp(out, ref, out["counts"], f"step {step}")
            totals.append([[e.force_total(i) for i in ids] for e in engines])
    finally:
        for e in engines:
            e.close()
        world.close()
    return np.array(totals)     # (step, rank, fix, 3)


def test_two_bricks_tally(gpu, sph_amd):
    """2x1x1 bricks, the setforce sphere across the cut, the oracle on the same procgrid: the
    fields, and the ranks' foriginal totals added together against the oracle's pre-fix force
    over the selection; a second identical run returns the same bits"""
    s, ph, fixes = bricks_case(sph_amd)
    ref = forced_oracle(s, ph, fixes, procgrid=BRICKS_PG, builds=False)
    ref.setup()
    # (the oracle's per-step foriginal, kept as the run goes)
    want = []
    orig_force = ref._force

    def force_and_keep():
        orig_force()
        want.append([foriginal(ref, k) for k in range(len(fixes))])

    ref._force = force_and_keep
    want.append([foriginal(ref, k) for k in range(len(fixes))])   # setup's
    totals = _bricks_run(sph_amd, s, ph, fixes, ref)
    assert len(want) == totals.shape[0] == 4
    for step in range(4):
        assert np.abs(totals[step, :, 0]).max(axis=1).min() > 0   # both ranks hold a share
        for k in range(len(fixes)):
            tot, mag = want[step][k]
            got = np.array([math.fsum(totals[step, :, k, d]) for d in range(3)])
            assert np.abs(got - tot).max() <= TOL * mag, (step, k, got, tot)
    again = _bricks_run(sph_amd, s, ph, fixes)
    assert again.tobytes() == totals.tobytes()


# ---- 7. rejected calls ----------------------------------------------------------------------
def test_forcefix_validation(gpu, sph_amd):
    """every rejected call raises EINVAL and leaves the engine as it was"""
    s, ph, fixes = c3_walls_case(sph_amd)
    eng = c3_engine(sph_amd, s, ph, 0)
    ok = sph_amd.sphere((4.0, 4.0, 4.0), 2.0)

    def rejected(fn, *a, **kw):
        with pytest.raises(sph_amd.HipError) as ei:
            fn(*a, **kw)
        assert ei.value.code == -1

    def raw(**kw):
        """a sph_forcefix that the Python helpers would not build"""
        f = sph_amd.ForceFix()
        f.kind, f.comp_mask, f.nevery = sph_amd.SPH_FF_ADD, 7, 1
        for k, v in kw.items():
            setattr(f, k, v)
        import ctypes
        sph_amd._chk(eng.L.sph_engine_forcefix(eng.h, ctypes.byref(f), None))

    rejected(raw, kind=2)                                              # unknown kind
    bad = sph_amd.sphere((4.0, 4.0, 4.0), 2.0)
    bad.style = 5
    rejected(eng.setforce, 0, 0, 0, region=bad)                        # unknown region style
    rejected(eng.addforce, 0, 0, 1, region=sph_amd.sphere((4, 4, 4), -0.5))   # negative radius
    rejected(raw, kind=sph_amd.SPH_FF_SET, per_mass=1)                 # per_mass on SET
    rejected(raw, kind=sph_amd.SPH_FF_SET, nevery=2)                   # nevery on SET
    rejected(raw, comp_mask=5)                                         # ADD with a NULL
    rejected(eng.addforce, 0, None, 1)
    rejected(eng.addforce, 0, 0, 1, every=0)                           # nevery < 1
    rejected(eng.addforce, 0, 0, 1, every=-2)
    ids = arm(eng, fixes)
    assert ids == [0, 1, 2, 3]
    rejected(eng.force_total, ids[0])                                  # before setup
    for k in range(sph_amd.SPH_MAX_FORCEFIX - len(fixes)):
        last = eng.addforce(0.0, 0.0, 0.0, types=[1], region=ok, tally=(k == 0))   # (no-ops)
    assert last == sph_amd.SPH_MAX_FORCEFIX - 1
    rejected(eng.setforce, 0, 0, 0)                                    # too many fixes
    rejected(eng.force_total, len(fixes))                              # (tallying, but) before setup
    ref = forced_oracle(s, ph, fixes, shadows=False)
    ref.setup()
    ref.run(1)
    eng.setup()
    rejected(eng.setforce, 0, 0, 0)                                    # after setup
    rejected(eng.force_total, ids[0])                                  # armed without tally
    rejected(eng.force_total, 8)                                       # no such fix
    assert eng.force_total(len(fixes)).shape == (3,)
    eng.run(1)
    check_fields(eng.get_atoms(), ref, ("x", "v", "rho", "f", "drho"), TOL)
