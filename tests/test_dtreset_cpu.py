"""fix dt/reset on the oracle side (dtreset_util.py), no GPU: the restated Verlet loops against
the unmodified pyoracle loops, the corners of FixDtReset::end_of_step (fix_dt_reset.cpp:131-186)
worked out by hand, and -- on the oracle alone -- that every scenario of test_gpu_dtreset.py
exercises what it is there for: dt changes at every reset, stays strictly inside (tmin, tmax)
there, and the `delr > xmax` rescale decides the minimum at least once."""
import math

import numpy as np
import pytest

import pyoracle as po
from dtreset_util import (BIG, CASES, Clock, DtMpRefRun, DtRefRun, bounded, case_inputs,
                          dt_oracle, np_dt_reset, oracle_for)
from forcefix_util import wrapped
from mp_variants_util import mp_box, mp_physics
from scenarios import c3_system

REF_FIELDS = ("x", "v", "rho", "e")


def _same(a, b, fields):
    for k in fields:
        assert np.array_equal(a.field(k), b.field(k)), k
    for k in ("f", "drho", "de", "vest"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k


@pytest.mark.parametrize("how", ["unarmed", "unbound", "pinned"])
def test_restated_loop_equals_refrun(how):
    """without the fix; with an xmax no atom comes near, so that MIN with tmax = dt holds dt;
    and with a tiny xmax under tmin = dt (tmax one ulp above: tmin >= tmax is an error), so
    that MAX with tmin holds it -- each time the unmodified RefRun bit for bit, over two runs,
    with a meso/stationary type"""
    s = wrapped(c3_system(8))
    ph = po.c3_physics()
    ph.stationary_mask = 1 << 2
    dt = ph.dt
    if how == "unarmed":
        fix = None
    elif how == "unbound":
        fix = dict(nevery=1, tmin=None, tmax=dt, xmax=1e3)
    else:
        ph.dt = dt = math.nextafter(ph.dt, 0.0)
        fix = dict(nevery=1, tmin=dt, tmax=math.nextafter(dt, 1.0), xmax=1e-12)
    a = dt_oracle(DtRefRun, s, ph, fix, shadows=False)
    b = po.RefRun(s, ph)
    for r in (a, b):
        r.setup()
        r.run(7)
        r.run(6)
    _same(a, b, REF_FIELDS)
    assert a.dt_steps == [dt] * 13 and a.dt_stats()["changes"] == 0
    assert a.dt_stats()["laststep"] == 0
    assert np.array_equal(a.numneigh_full(), b.numneigh_full())


def test_restated_loop_equals_mprefrun():
    s, ph = mp_box(dim=3), mp_physics()
    a = dt_oracle(DtMpRefRun, s, ph, dict(nevery=2, tmin=None, tmax=ph.dt, xmax=1e3),
                  shadows=False)
    b = po.MpRefRun(s, ph)
    for r in (a, b):
        r.setup()
        r.run(5)
    _same(a, b, ("x", "v", "rho", "e", "rmass", "cv"))
    assert a.dt_stats() == dict(dt=ph.dt, time=5 * ph.dt, laststep=0, changes=0)


def test_formula_corners():
    one = np.ones(1, bool)
    z = np.zeros((1, 3))
    # at rest without force: BIG (fix_dt_reset.cpp:155)
    assert np_dt_reset(z, z, [1.0], one, 0.1) == (np.array([BIG]), BIG)
    # velocity alone: xmax / |v|, exactly
    v = np.array([[3.0, 0.0, 4.0]])
    assert np_dt_reset(v, z, [1.0], one, 0.5)[1] == 0.1
    # force alone: sqrt(2 xmax m / |f|)
    f = np.array([[0.0, 8.0, 0.0]])
    assert np_dt_reset(z, f, [0.25], one, 0.25)[1] == math.sqrt(2 * 0.25 / (8.0 * 0.25))
    # v and f aligned: dt = dtv = 0.1 moves 0.5 + 0.5 0.01 2 = 0.51 > xmax: rescaled by 0.5/0.51
    f = np.array([[1.2, 0.0, 1.6]])
    dt, dtmin, resc = np_dt_reset(v, f, [1.0], one, 0.5, detail=True)
    d0 = 0.5 / math.sqrt(3.0 * 3.0 + 0.0 * 0.0 + 4.0 * 4.0)
    dx, dz = d0 * 3.0 + 0.5 * (d0 * d0) * 1.0 * 1.2 * 1.0, d0 * 4.0 + 0.5 * (d0 * d0) * 1.0 * 1.6 * 1.0
    assert resc[0] and dtmin == d0 * (0.5 / math.sqrt(dx * dx + 0.0 * 0.0 + dz * dz))
    assert abs(dtmin - 0.1 * 0.5 / 0.51) < 1e-15
    # opposed: the force shortens the move, no rescale
    dt, dtmin, resc = np_dt_reset(v, -f, [1.0], one, 0.5, detail=True)
    assert not resc[0] and dtmin == 0.1
    # an atom outside the group is ignored, however fast
    v2 = np.array([[3.0, 0.0, 4.0], [300.0, 0.0, 400.0]])
    z2 = np.zeros((2, 3))
    dt, dtmin = np_dt_reset(v2, z2, [1.0, 1.0], [True, False], 0.5)
    assert dtmin == 0.1 and dt[1] == BIG
    assert np_dt_reset(v2, z2, [1.0, 1.0], [False, False], 0.5)[1] == BIG
    # MAX with tmin first, then MIN with tmax (:170-171)
    assert bounded(0.05, 0.2, 0.1) == 0.1      # (the other order would give 0.2)
    assert bounded(0.05, 0.01, 0.1) == 0.05 and bounded(5.0, None, 0.1) == 0.1
    assert bounded(0.001, 0.01, None) == 0.01 and bounded(BIG, None, None) == BIG


def test_clock_unchanged_dt_leaves_time_alone():
    c = Clock(0.5)
    c.change(0, 0.5)
    c.change(3, 0.5)
    assert (c.atime, c.atimestep, c.laststep, c.changes) == (0.0, 0, 0, 0)
    assert c.time(4) == 2.0
    c.change(4, 0.25)             # update_time: atime += (4 - 0) * 0.5
    assert (c.atime, c.atimestep, c.laststep, c.changes, c.dt) == (2.0, 4, 4, 1, 0.25)
    c.change(6, 0.25)
    assert c.laststep == 4 and c.time(8) == 2.0 + 4 * 0.25


# the scenarios whose deciding atom is never rescaled: the fastest atom of these boxes is
# decelerating (v . f < 0) throughout, asserted below
NO_RESCALE = {"c3"}


@pytest.mark.parametrize("name", sorted(CASES))
def test_scenarios_exercise_the_fix(name):
    cls, s, ph, kw, dtfix, nm, steps = case_inputs(name)
    ref = oracle_for(name, shadows=False)
    dts = np.asarray(ref.dt_steps)
    assert len(dts) == steps and len(ref.eos) == 1 + steps // dtfix["nevery"]
    tmin = dtfix["tmin"] if dtfix["tmin"] is not None else 0.0
    tmax = dtfix["tmax"] if dtfix["tmax"] is not None else BIG
    changed = np.concatenate([[dts[0] != ph.dt], dts[1:] != dts[:-1]])
    inside = (dts > tmin) & (dts < tmax)
    print(name, "changed", int(changed.sum()), "of", steps, "rescaled at",
          [e[0] for e in ref.eos if e[3]])
    if dtfix["nevery"] == 1:
        assert (changed & inside).sum() * 2 >= steps
    else:
        # dt can only change after a reset step: every one of them changes it here, which is
        # one step in nevery
        resets = [k for k in range(steps) if k % dtfix["nevery"] == 0]
        assert all(changed[k] and inside[k] for k in resets)
        assert not any(changed[k] for k in range(steps) if k not in resets)
    # the raw minimum itself is inside the bounds: they never did the work
    assert all(tmin < e[1] < tmax for e in ref.eos)
    if name in NO_RESCALE:
        assert not any(e[3] for e in ref.eos)
    else:
        assert any(e[3] for e in ref.eos)
    if nm is not None and nm[2]:
        # no displacement check of a check-yes case is near a tie
        assert all(abs(m - 1.0) > 1e-6 for m in ref.check_max)
