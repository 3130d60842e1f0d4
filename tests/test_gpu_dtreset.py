"""GPU tests of fix dt/reset (sph_engine_dt_reset, fix_dt_reset.cpp:131-186): the scan behind the
final integrate, the one-block fold and the integrate kernels that read {dtv, dtf} from the
device record, against dtreset_util.py's numpy restatement of FixDtReset::end_of_step and its
oracle runs.

* the dt the engine holds after every step equals, bit for bit, np_dt_reset + the bounds applied
  to the v and f the engine itself reports (no force tolerance enters), and time / laststep /
  changes equal Update::update_time replayed over the engine's own dt sequence;
* against the oracle: fields at test_gpu_engine.compare's bars (1e-10 normwise, elementwise
  bounded by the oracle's reordering spread), the per-step dt within max(1e-10 dt, the spread of
  dt between the oracle and its own reordered shadow runs), neighbour counts exact.
test_dtreset_cpu.py shows on the oracle that these scenarios change dt at every reset, keep it
strictly inside the bounds and let the delr rescale decide the minimum."""
import threading

import numpy as np
import pytest

import pyoracle as po
from c5_util import mp_engine, mp_state
from conftest import check_fields
from dtreset_util import (BRICKS_PG, Clock, arm_dt, bounded, case_inputs, fast_c2, np_dt_reset,
                          oracle_for, type_mask)
from forcefix_util import arm, wrapped
from idealgas_util import gas_engine
from neighcheck_util import single_engine
from scenarios import c3_system, water_collapse_physics, water_collapse_system

pytestmark = pytest.mark.gpu
TOL = 1e-10
FIELDS = ("rho", "f", "drho", "de", "x", "v", "e")
MP_FIELDS = ("x", "v", "rho", "e", "rmass", "cv", "cg", "f", "de")


def bits(x):
    return np.float64(x).tobytes()


# ---- 1. the scan and the fold, bit for bit ----------------------------------------------------
def _scan_cases():
    return {
        "n1000": lambda: (fast_c2(10), po.c2_physics(), None),          # 3 full blocks + 232
        "n49_2d": lambda: (fast_c2(7, dim=2), po.c2_physics(), None),   # one partial wave
        "n512_type1": lambda: (wrapped(c3_system(8)), po.c3_physics(), [1]),
    }


@pytest.mark.parametrize("path", [0, 1])
@pytest.mark.parametrize("name", ["n1000", "n49_2d", "n512_type1"])
def test_scan_and_fold_bit_exact(gpu, sph_amd, name, path):
    s, ph, types = _scan_cases()[name]()
    tmin, tmax, xmax = 2e-4, 5e-3, 1.5e-4 if name != "n512_type1" else 5e-5
    eng = single_engine(sph_amd, s, ph, path)
    eng.dt_reset(1, tmin, tmax, xmax, type_mask(types))
    eng.setup()
    clock = Clock(float(ph.dt))
    nchanged = 0
    for step in range(0, 11):
        if step:
            eng.run(1)
        got = eng.get_atoms()
        t = s.type[got["tag"]]
        minv = 1.0 / s.mass[t]
        dti, dtmin = np_dt_reset(got["v"], got["f"], minv,
                                 np.ones(t.size, bool) if types is None else np.isin(t, types),
                                 xmax)
        want = bounded(dtmin, tmin, tmax)
        st = eng.dt_stats()
        print(name, path, step, st, "host", want, "raw", dtmin)
        assert bits(st["dt"]) == bits(want), (step, st["dt"], want)
        nchanged += want != clock.dt
        clock.change(step, want)
        ws = clock.stats(step)
        assert bits(st["time"]) == bits(ws["time"]), step
        assert st["laststep"] == ws["laststep"] and st["changes"] == ws["changes"], step
    assert nchanged >= 6 and tmin < want < tmax   # the bounds did not do the work
    eng.close()


# ---- 2. parity with the oracle ----------------------------------------------------------------
def check_dt_sequence(dts, ref, where):
    want = np.asarray(ref.dt_steps)
    bar = np.maximum(1e-10 * want, ref.dt_spread())
    err = np.abs(np.asarray(dts) - want)
    print(where, "dt err / bar max", float((err / bar).max()), "spread max", float(ref.dt_spread().max()))
    assert (err <= bar).all(), (where, err, bar)


def run_case(sph, name, make, path=0, fields=FIELDS, arm_with=None, chunks=None):
    """the engine stepped one step at a time (its dt read before every step), or in chunks"""
    cls, s, ph, kw, dtfix, nm, steps = case_inputs(name)
    ref = oracle_for(name)
    eng = make(sph, s, ph, path)
    if arm_with is not None:
        arm(eng, arm_with)
    if nm is not None:
        eng.neigh_modify(*nm)
    arm_dt(eng, dtfix)
    eng.setup()
    dts = []
    if chunks is None:
        for _ in range(steps):
            dts.append(eng.dt_stats()["dt"])
            eng.run(1)
    else:
        for c in chunks:
            eng.run(c)
    return eng, ref, dts


def finish_single(eng, ref, dts, name, path, fields=FIELDS):
    if dts:
        check_dt_sequence(dts, ref, name)
    st, want = eng.dt_stats(), ref.dt_stats()
    assert st["laststep"] == want["laststep"] and st["changes"] == want["changes"]
    assert abs(st["time"] - want["time"]) <= 1e-9 * want["time"]
    assert eng.stats()["staged"] == (1 if path == 0 else 0)
    assert np.array_equal(eng.neighbor_counts(), ref.numneigh_full())
    check_fields(eng.get_atoms(), ref, fields, TOL, where=name)


@pytest.mark.parametrize("path", [0, 1])
def test_parity_c2(gpu, sph_amd, path):
    eng, ref, dts = run_case(sph_amd, "c2", single_engine, path)
    finish_single(eng, ref, dts, "c2", path)
    eng.close()


def test_parity_c3_morris_heat(gpu, sph_amd):
    eng, ref, dts = run_case(sph_amd, "c3", single_engine)
    finish_single(eng, ref, dts, "c3", 0)
    eng.close()


def test_parity_shock_tube_setforce(gpu, sph_amd):
    """idealgas + setforce NULL 0 0 from rest: at setup v = 0, so dtf alone sets the step, from
    the force the setforce fix has already cleared in y"""
    cls, s, ph, kw, dtfix, nm, steps = case_inputs("shock")
    eng, ref, dts = run_case(sph_amd, "shock", gas_engine, arm_with=kw["fixes"])
    finish_single(eng, ref, dts, "shock", 0, fields=("f", "drho", "de", "x", "v", "rho", "e"))
    eng.close()


def test_parity_multiphase(gpu, sph_amd):
    """the two-phase box: massinv from rmass"""
    cls, s, ph, kw, dtfix, nm, steps = case_inputs("mp")
    ref = oracle_for("mp")
    eng = mp_engine(sph_amd, s, ph)
    arm_dt(eng, dtfix)
    eng.setup()
    dts = []
    for _ in range(steps):
        dts.append(eng.dt_stats()["dt"])
        eng.run(1)
    check_dt_sequence(dts, ref, "mp")
    g = mp_state(eng)
    assert np.array_equal(eng.neighbor_counts(), ref.numneigh_full())
    check_fields(g, ref, MP_FIELDS, TOL, where="mp")
    eng.close()


# ---- 3. nevery = 3 ------------------------------------------------------------------------------
def _state(eng):
    g = eng.get_atoms()
    st = eng.dt_stats()
    return (b"".join(g[k].tobytes() for k in FIELDS), bits(st["dt"]), bits(st["time"]),
            st["laststep"], st["changes"], eng.neighbor_counts().tobytes())


def test_nevery3_fused_steps_and_split_runs(gpu, sph_amd):
    """between resets the fused final+initial kernel runs in its dt-from-record form; a reset
    at the end of a run is the trailing final integrate's: run(7) = run(3); run(4) = 7 x run(1)"""
    res = []
    for chunks in ((7,), (3, 4), (1,) * 7):
        eng, ref, _ = run_case(sph_amd, "c2_every3", single_engine, chunks=chunks)
        res.append(_state(eng))
        st = eng.dt_stats()
        eng.close()
    assert res[0] == res[1] == res[2]
    assert st["laststep"] == 6 and st["changes"] == 3   # setup, 3, 6
    eng, ref, dts = run_case(sph_amd, "c2_every3", single_engine)
    finish_single(eng, ref, dts, "c2_every3", 0)
    assert dts[0] == dts[1] == dts[2] != dts[3] == dts[4]
    eng.close()


# ---- 4. water collapse as scripted --------------------------------------------------------------
def test_water_collapse_as_scripted(gpu, sph_amd):
    """fix dtfix all dt/reset 1 NULL ${dt} 0.0005 units box with neigh_modify every 5 delay 0
    check no: from rest the reset holds tmax over the 20 steps, and the run is the fixed-dt
    engine's bit for bit"""
    s, ph = water_collapse_system(), water_collapse_physics()
    res = []
    for armed in (True, False):
        eng = single_engine(sph_amd, s, ph, 0)
        eng.neigh_modify(5, 0, False)
        if armed:
            eng.dt_reset(1, None, ph.dt, 0.0005)
        eng.setup()
        for _ in range(4):
            eng.run(5)
            assert bits(eng.dt_stats()["dt"]) == bits(ph.dt)
        g = eng.get_atoms()
        res.append(b"".join(g[k].tobytes() for k in FIELDS))
        st = eng.dt_stats()
        assert st["laststep"] == 0 and st["changes"] == 0
        assert abs(st["time"] - 20 * ph.dt) < 1e-15
        eng.close()
    assert res[0] == res[1]


def test_water_collapse_moving(gpu, sph_amd):
    """the same fixture with a small random velocity on the water: dt drops below tmax at
    setup and changes every step; the group is `all`, so the stationary boundary takes part"""
    eng, ref, dts = run_case(sph_amd, "water", single_engine)
    assert max(dts) < 3e-4
    finish_single(eng, ref, dts, "water", 0)
    eng.close()


# ---- 5. two bricks ----------------------------------------------------------------------------
def test_two_bricks_share_one_dt(gpu, sph_amd):
    """2x1x1 bricks from rest, only rank 1's atoms fall: both ranks hold the same dt after every
    step, bit for bit, and the run keeps the one-brick oracle's bars"""
    cls, s, ph, kw, dtfix, nm, steps = case_inputs("bricks")
    ref = oracle_for("bricks")
    world = sph_amd.LocalWorld(2)
    owner = po.brick_owner(s, s.x, BRICKS_PG)
    assert all(owner[e[2]] == 1 for e in ref.eos)   # the deciding atom is one of rank 1's
    engines = []
    for r in range(2):
        eng = single_engine(sph_amd, s, ph, 0, procgrid=BRICKS_PG, rank=r,
                            sel=np.nonzero(owner == r)[0])
        eng.comm_local(world, r)
        arm_dt(eng, dtfix)
        engines.append(eng)
    errors, seq = [], [[], []]

    def work(r):
        try:
            engines[r].setup()
            for _ in range(steps):
                seq[r].append(engines[r].dt_stats())
                engines[r].run(1)
            seq[r].append(engines[r].dt_stats())
        except Exception as ex:  # surfaced below
            errors.append(ex)

    th = [threading.Thread(target=work, args=(r,)) for r in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=300)
    try:
        assert not any(t.is_alive() for t in th), "brick threads hung"
        assert not errors, errors
        assert seq[0] == seq[1]
        assert all(bits(a["dt"]) == bits(b["dt"]) for a, b in zip(*seq))
        check_dt_sequence([d["dt"] for d in seq[0][:-1]], ref, "bricks")
        assert seq[0][-1]["changes"] == ref.dt_stats()["changes"]
        out = {k: np.zeros((s.n, 3)) for k in ("x", "v", "f")}
        out.update({k: np.zeros(s.n) for k in ("rho", "e", "drho", "de")})
        counts = np.zeros(s.n, dtype=np.int32)
        for eng in engines:
            got = eng.get_atoms()
            for k in out:
                out[k][got["tag"]] = got[k]
            counts[got["tag"]] = eng.neighbor_counts()
        assert np.array_equal(counts, ref.numneigh_full())
        check_fields(out, ref, FIELDS, TOL, where="bricks")
    finally:
        for e in engines:
            e.close()
        world.close()


# ---- 6. with neigh_modify check yes -------------------------------------------------------------
@pytest.mark.parametrize("path", [0, 1])
def test_with_neigh_check(gpu, sph_amd, path):
    """check yes and dt/reset together (the kernels' CHK and DTR forms at once): the builds
    come where the oracle's do, which with a smaller dt is later than at the fixed step"""
    eng, ref, dts = run_case(sph_amd, "c2_check", single_engine, path)
    ns = eng.neigh_stats()
    print("c2_check", ns, ref.build_steps)
    assert ns == dict(builds=len(ref.build_steps), dangerous=ref.ndanger,
                      checks=len(ref.eligible_steps), last_build=ref.build_steps[-1])
    assert len(ref.build_steps) > 1
    finish_single(eng, ref, dts, "c2_check", path)
    eng.close()


def test_with_neigh_check_between_resets(gpu, sph_amd):
    """the same with a reset every 3 steps: the steps between two resets take the fused
    final + initial integrate in its CHK and DTR form (k_final_initial<true, true>), which a
    reset at every step never launches"""
    eng, ref, dts = run_case(sph_amd, "c2_check_every3", single_engine)
    ns = eng.neigh_stats()
    print("c2_check_every3", ns, ref.build_steps)
    assert ns == dict(builds=len(ref.build_steps), dangerous=ref.ndanger,
                      checks=len(ref.eligible_steps), last_build=ref.build_steps[-1])
    assert len(ref.build_steps) > 1 and len(ref.eligible_steps) == 16
    finish_single(eng, ref, dts, "c2_check_every3", 0)
    assert dts[0] == dts[1] == dts[2] != dts[3]
    eng.close()


# ---- 7. argument errors and calling time ----------------------------------------------------------
def test_argument_errors_and_calling_time(gpu, sph_amd):
    cls, s, ph, kw, dtfix, nm, steps = case_inputs("c2")
    eng = single_engine(sph_amd, s, ph, 1)
    for args in ((0, 1e-4, 1e-3, 1e-3), (-2, None, None, 1e-3), (1, -1e-4, 1e-3, 1e-3),
                 (1, None, -1e-3, 1e-3), (1, 1e-3, 1e-3, 1e-3), (1, 2e-3, 1e-3, 1e-3),
                 (1, None, None, 0.0), (1, None, None, -1.0)):
        with pytest.raises(sph_amd.HipError) as ei:
            eng.dt_reset(*args)
        assert ei.value.code == -1 and len(str(ei.value)) > 20, args
    with pytest.raises(sph_amd.HipError) as ei:
        eng.dt_stats()                              # before setup
    assert ei.value.code == -1
    eng.dt_reset(2, None, 1e-3, 1e-3)
    with pytest.raises(sph_amd.HipError, match="armed already"):
        eng.dt_reset(1, None, 1e-3, 1e-3)           # a second call
    eng.setup()
    with pytest.raises(sph_amd.HipError, match="before sph_engine_setup"):
        eng.dt_reset(1, None, 1e-3, 1e-3)           # after setup
    eng.close()
    # an engine without the fix reports its fixed step
    eng = single_engine(sph_amd, s, ph, 1)
    eng.setup()
    eng.run(3)
    assert eng.dt_stats() == dict(dt=ph.dt, time=3 * ph.dt, laststep=0, changes=0)
    eng.close()
    # fix phase_change reads update->dt: rejected in either order
    ms, mph = case_inputs("mp")[1:3]
    pc = dict(Tc=0.5, Tt=0.1, Hwv=1.0, dr=0.5, to_mass=0.3, cutoff=3.0, from_type=1, to_type=2)
    eng = mp_engine(sph_amd, ms, mph)
    eng.dt_reset(1, None, 1e-3, 1e-3)
    with pytest.raises(sph_amd.HipError, match="dt_reset"):
        eng.phase_change(pc["Tc"], pc["Tt"], pc["Hwv"], pc["dr"], pc["to_mass"], pc["cutoff"],
                         pc["from_type"], pc["to_type"], nevery=1, seed=12345)
    eng.close()
    eng = mp_engine(sph_amd, ms, mph)
    eng.phase_change(pc["Tc"], pc["Tt"], pc["Hwv"], pc["dr"], pc["to_mass"], pc["cutoff"],
                     pc["from_type"], pc["to_type"], nevery=1, seed=12345)
    with pytest.raises(sph_amd.HipError, match="phase_change"):
        eng.dt_reset(1, None, 1e-3, 1e-3)
    eng.close()


# ---- 8. identical runs, identical bits ------------------------------------------------------------
def test_identical_runs_identical_bits(gpu, sph_amd):
    res = []
    for _ in range(2):
        eng, ref, _ = run_case(sph_amd, "c2", single_engine, chunks=(20,))
        res.append(_state(eng))
        eng.close()
    assert res[0] == res[1]
