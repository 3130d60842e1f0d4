"""fix setmeso / setmesode clamps and the group reductions on the device-resident engine,
against the oracle's Verlet drivers with the clamps applied in numpy where LAMMPS runs
post_force (setmeso_util.clamped_oracle; its preconditions are test_setmeso_cpu.py's).

Bars: fields 1e-10 normwise and conftest.check_fields' elementwise bar (the shadows clamped
like the run), atom counts, insertions, types and neighbour counts exact, clamped values bit
for bit.  Reductions against numpy on the engine's own arrays: count exact; min / max exact
for stored fields and 1e-14 relative for derived ones (T = e / cv, KE: their last bits depend
on contraction); |sum - fsum| <= 1e-13 sum|q| (a tree sum of N <= 2^24 doubles is within
~24 * 1.1e-16 = 2.7e-15 sum|q|; the rest is the derived quantities' own rounding)."""
import math

import numpy as np
import pytest

import pyoracle as po
from c5_util import bricks_step, mp_bricks, mp_collect, mp_engine, mp_state
from conftest import check_fields
from setmeso_util import (arm, bubble_case, c3_case, c3_engine, clamped_oracle, far_field,
                          np_selected)

pytestmark = pytest.mark.gpu
TOL = 1e-10
MP_FIELDS = ("x", "v", "rho", "e", "rmass", "cv", "cg", "f", "de")


def _compare_mp(g, ref, counts):
    s = ref.s
    assert g["x"].shape[0] == s.n and g["ninserted"] == ref.ninserted
    assert np.array_equal(g["type"], s.type)
    assert np.array_equal(counts, ref.numneigh_full())
    check_fields(g, ref, MP_FIELDS, TOL)


def _clamped_exactly(g, clamp):
    """after setup (a step's final integrate then adds dtf * de): e = cv * T bit for bit"""
    m = np_selected(clamp, g["x"], g["type"])
    assert 0 < m.sum() < m.size
    assert np.array_equal(g["e"][m], g["cv"][m] * clamp["value"])


@pytest.mark.parametrize("nx,dim,pc", [(10, 3, False), (10, 3, True), (16, 2, True)])
def test_c5_far_field_clamp(gpu, sph_amd, nx, dim, pc):
    """bubble.lmp:94-96 on the C5 stack, alone and with fix phase_change creating atoms that
    meet the clamp in the step they are created"""
    s, ph, clamps, _ = bubble_case(sph_amd, nx, dim, pc)
    ref = clamped_oracle(s, ph, clamps)
    ref.setup()
    eng = mp_engine(sph_amd, s, ph)
    arm(eng, clamps)
    eng.setup()
    g = mp_state(eng)
    _compare_mp(g, ref, eng.neighbor_counts())
    _clamped_exactly(g, clamps[0])
    for _ in range(5):
        ref.run(1)
        eng.run(1)
        _compare_mp(mp_state(eng), ref, eng.neighbor_counts())
    if pc:
        assert ref.ninserted >= 1


@pytest.mark.parametrize("path", [0, 1])
@pytest.mark.parametrize("nsteps", [5, 12])
def test_c3_three_fixes(gpu, sph_amd, path, nsteps):
    """single-phase engine, both pair paths, three fixes in one launch: meso_e on a type in a
    block, setmesode on a type outside a sphere, meso_rho in a block; 5 steps cross no
    rebuild, 12 cross one"""
    s, ph, clamps, _ = c3_case(sph_amd)
    ref = clamped_oracle(s, ph, clamps)
    ref.setup()
    eng = c3_engine(sph_amd, s, ph, path)
    arm(eng, clamps)
    eng.setup()
    fields = ("x", "v", "rho", "e", "f", "drho", "de")
    g = eng.get_atoms()
    check_fields(g, ref, fields, TOL, where="setup")
    m = np_selected(clamps[0], g["x"], s.type)     # (the clamped values, bit for bit)
    assert m.any() and np.all(g["e"][m] == 1.5)
    m = np_selected(clamps[2], g["x"], s.type)
    assert m.any() and np.all(g["rho"][m] == 0.8)
    ref.run(nsteps)
    eng.run(nsteps)
    g = eng.get_atoms()
    assert np.array_equal(eng.neighbor_counts(), ref.numneigh_full())
    check_fields(g, ref, fields, TOL, where=f"step {nsteps}")
    assert eng.stats()["staged"] == (1 if path == 0 else 0)
    m = np_selected(clamps[1], g["x"], s.type)     # (de is not integrated: still the clamp's)
    assert m.any() and np.all(g["de"][m] == 0.0)


def _bricks(sph_amd, pg=(2, 1, 1)):
    s, ph, clamps, _ = bubble_case(sph_amd, 10, 3, False)
    world, engines = mp_bricks(sph_amd, s, ph, pg, po.brick_owner(s, s.x, pg))
    for e in engines:
        arm(e, clamps)
    return s, ph, clamps, world, engines


def test_c5_far_field_clamp_two_bricks(gpu, sph_amd):
    """The sphere straddles the cut at x = 0.5 of 2x1x1 bricks (0.5 wide against a 0.3
    cutoff).  The oracle runs the same decomposition (MpRefRun procgrid), as the brick tests
    of the stack do: the multiphase styles leave the ghosts' rho and colour gradient as
    communicated, so which neighbours are ghosts changes the reference's own results."""
    pg = (2, 1, 1)
    s, ph, clamps, world, engines = _bricks(sph_amd, pg)
    ref = clamped_oracle(s, ph, clamps, procgrid=pg)
    ref.setup()
    try:
        bricks_step(engines, lambda e: e.setup())
        out = mp_collect(engines, ref.s.n)
        _compare_mp(out, ref, out["counts"])
        _clamped_exactly(out, clamps[0])
        for _ in range(5):
            ref.run(1)
            bricks_step(engines, lambda e: e.run(1))
            out = mp_collect(engines, ref.s.n)
            _compare_mp(out, ref, out["counts"])
    finally:
        for e in engines:
            e.close()
        world.close()


def test_setmeso_validation(gpu, sph_amd):
    """every rejected call raises EINVAL and leaves the engine as it was"""
    s, ph, clamps, _ = c3_case(sph_amd)
    eng = c3_engine(sph_amd, s, ph, 0)
    ok = sph_amd.sphere((4.0, 4.0, 4.0), 2.0)

    def rejected(*a, **kw):
        with pytest.raises(sph_amd.HipError) as ei:
            eng.setmeso(*a, **kw)
        assert ei.value.code == -1

    rejected(7, 1.0)                                              # unknown field
    bad = sph_amd.sphere((4.0, 4.0, 4.0), 2.0)
    bad.style = 5
    rejected("e", 1.0, region=bad)                                # unknown region style
    rejected("e", 1.0, region=sph_amd.sphere((4, 4, 4), -0.5))    # negative radius
    rejected("de", 0.0, noregion=ok)                              # setmesode has no noregion
    arm(eng, clamps)
    for _ in range(sph_amd.SPH_MAX_SETMESO - len(clamps)):
        eng.setmeso("de", 0.0, types=[1], region=clamps[1]["region"])   # (repeats of a fix)
    rejected("e", 1.0)                                            # too many fixes
    ref = clamped_oracle(s, ph, clamps, shadows=False)
    ref.setup()
    ref.run(1)
    eng.setup()
    rejected("e", 1.0)                                            # after setup
    eng.run(1)
    check_fields(eng.get_atoms(), ref, ("x", "rho", "e", "de"), TOL)


QUANT = ("one", "rho", "e", "t", "de", "mass", "ke")
STORED = ("one", "rho", "e", "de", "mass")


def _quantities(g):
    m = g["rmass"]
    return dict(one=np.ones_like(m), rho=g["rho"], e=g["e"], t=g["e"] / g["cv"], de=g["de"],
                mass=m, ke=0.5 * m * (g["v"] * g["v"]).sum(1))


def _selections(sph):
    groups = [dict(), dict(types=[1]), dict(types=[2]), dict(region=sph), dict(noregion=sph)]
    return [dict(quantity=q, **grp) for q in QUANT for grp in groups]


def _reduce_all(eng, sels):
    out = []
    for k in range(0, len(sels), 16):
        out += eng.reduce(sels[k:k + 16])
    return out


def _check_reduction(sel, o, g):
    m = np_selected(sel, g["x"], g["type"])
    q = _quantities(g)[sel["quantity"]][m]
    assert o["count"] == int(m.sum()), sel
    if not q.size:
        assert (o["sum"], o["min"], o["max"]) == (0.0, math.inf, -math.inf), sel
        return
    if sel["quantity"] in STORED:
        assert o["min"] == q.min() and o["max"] == q.max(), sel
    else:
        assert abs(o["min"] - q.min()) <= 1e-14 * abs(q.min()), sel
        assert abs(o["max"] - q.max()) <= 1e-14 * abs(q.max()), sel
    assert abs(o["sum"] - math.fsum(q)) <= 1e-13 * math.fsum(np.abs(q)), (sel, o["sum"])


def _combine(parts):
    return dict(sum=math.fsum(p["sum"] for p in parts), min=min(p["min"] for p in parts),
                max=max(p["max"] for p in parts), count=sum(p["count"] for p in parts))


def test_reduce_c5(gpu, sph_amd):
    """end state of the far-field scenario: seven quantities x {all, each type, inside the
    sphere, noregion sphere}, twice (identical bits)"""
    s, ph, clamps, _ = bubble_case(sph_amd, 10, 3, False)
    eng = mp_engine(sph_amd, s, ph)
    arm(eng, clamps)
    with pytest.raises(sph_amd.HipError) as ei:     # (valid after setup only)
        eng.reduce([dict(quantity="one")])
    assert ei.value.code == -1
    eng.setup()
    eng.run(5)
    g = mp_state(eng)
    sels = _selections(far_field(sph_amd, 10, 3))
    out = _reduce_all(eng, sels)
    assert out == _reduce_all(eng, sels)
    for sel, o in zip(sels, out):
        _check_reduction(sel, o, g)
    assert out[0]["count"] == s.n and out[2]["count"] == int((s.type == 2).sum()) > 0
    # an empty selection: type 2 outside the far-field sphere; 17 selections: EINVAL
    empty = eng.reduce([dict(quantity="e", types=[2], noregion=far_field(sph_amd, 10, 3)),
                        dict(quantity="one", types=[5])])
    for o in empty:
        assert o == dict(sum=0.0, min=math.inf, max=-math.inf, count=0)
    with pytest.raises(sph_amd.HipError) as ei:
        eng.reduce([dict(quantity="one")] * 17)
    assert ei.value.code == -1
    assert eng.reduce([]) == []


def test_reduce_c3(gpu, sph_amd):
    """end state of the three-fix scenario on a single-phase engine (mass[type], one cv)"""
    s, ph, clamps, _ = c3_case(sph_amd)
    eng = c3_engine(sph_amd, s, ph, 0)
    arm(eng, clamps)
    eng.setup()
    eng.run(12)
    g = eng.get_atoms()
    g.update(eng.get_atoms_multiphase())
    sels = _selections(sph_amd.sphere((4.0, 4.0, 4.0), 2.77))
    out = _reduce_all(eng, sels)
    assert out == _reduce_all(eng, sels)
    for sel, o in zip(sels, out):
        _check_reduction(sel, o, g)


def test_reduce_two_bricks_combine(gpu, sph_amd):
    """each brick reduces its owned atoms; sum / min / max / count combined over the bricks
    (the caller's Allreduce) meet the same bars on the collected atoms"""
    s, ph, clamps, world, engines = _bricks(sph_amd)
    try:
        bricks_step(engines, lambda e: e.setup())
        bricks_step(engines, lambda e: e.run(5))
        g = mp_collect(engines, s.n)
        sels = _selections(far_field(sph_amd, 10, 3))
        per = [_reduce_all(e, sels) for e in engines]
        assert sum(e.nlocal for e in engines) == s.n
        for k, sel in enumerate(sels):
            _check_reduction(sel, _combine([p[k] for p in per]), g)
    finally:
        for e in engines:
            e.close()
        world.close()
