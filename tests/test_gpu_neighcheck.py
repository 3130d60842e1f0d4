"""GPU parity of neigh_modify every / delay / check (sph_engine_neigh_modify, Neighbor::decide,
neighbor.cpp:1332-1410) against the oracle runs of neighcheck_util.py, whose rebuild decision
is the reference's.  The schedule is exact: builds, dangerous builds, checks and the last build
step equal the oracle's; since the builds then happen at the same steps from the same positions,
the fields keep the bars of the helper each case comes from (conftest.check_fields: 1e-10
normwise, elementwise bounded by the oracle's reordering spread) and the neighbour counts after
the last build are bit-exact.  test_neighcheck_cpu.py shows that no check of these cases is
within 1e-6 of a tie and works their schedules out by hand."""
import threading

import numpy as np
import pytest

import pyoracle as po
from c5_util import mp_engine, mp_state
from conftest import check_fields
from forcefix_util import arm
from idealgas_util import gas_engine
from neighcheck_util import BRICKS_PG, case_inputs, oracle_for, single_engine

pytestmark = pytest.mark.gpu
TOL = 1e-10
FIELDS = ("rho", "f", "drho", "de", "x", "v", "e")
MP_FIELDS = ("x", "v", "rho", "e", "rmass", "cv", "cg", "f", "de")


def want_stats(ref):
    nm = ref.nm
    return dict(builds=len(ref.build_steps), dangerous=ref.ndanger,
                checks=len(ref.eligible_steps) if nm is not None and nm[2] else 0,
                last_build=ref.build_steps[-1])


def run_single(sph, name, path, make=single_engine, fields=FIELDS, arm_with=None):
    cls, s, ph, kw, nm, steps = case_inputs(name)
    ref = oracle_for(name)
    eng = make(sph, s, ph, path)
    if arm_with is not None:
        arm(eng, arm_with)
    if nm is not None:
        eng.neigh_modify(*nm)
    eng.setup()
    assert eng.neigh_stats() == dict(builds=1, dangerous=0, checks=0, last_build=0)
    eng.run(steps)
    ns, st = eng.neigh_stats(), eng.stats()
    print(name, path, ns, "oracle builds", ref.build_steps, "check max",
          [f"{m:.3f}" for m in ref.check_max])
    assert ns == want_stats(ref)
    assert st["staged"] == (1 if path == 0 else 0) and st["step"] == steps
    assert np.array_equal(eng.neighbor_counts(), ref.numneigh_full())
    check_fields(eng.get_atoms(), ref, fields, TOL, where=name)
    return eng, ref, st


@pytest.mark.parametrize("path", [0, 1])
@pytest.mark.parametrize("name", ["c2_every5", "c2_every1", "c2_delay5", "c2_delay_nocheck",
                                  "c2_still"])
def test_c2_schedules(gpu, sph_amd, name, path):
    """every 5 with the crossing off the grid (builds at 10 and 20, not 7 or 5), every 1
    (builds at 7 and 14 only), every 1 delay 5 (the dangerous build at 5), every 2 delay 4
    check no (delay alone), and the box nothing crosses in (the setup's build alone)"""
    eng, ref, st = run_single(sph_amd, name, path)
    if name == "c2_still":
        assert eng.neigh_stats()["builds"] == 1 and st["nbr_builds"] == 1
    eng.close()


def test_inner_rows_with_skipped_rebuilds(gpu, sph_amd):
    """the block path's inner rows under check yes: the drift retires them between builds
    (inner_refresh > 0) while the eligible steps 5 and 15 skip their rebuild; an engine that
    rebuilds every step without neigh_modify stays within the same bars of the same oracle"""
    eng, ref, st = run_single(sph_amd, "c2_every5", 0)
    assert st["inner_rows"] == 1 and st["inner_refresh"] > 0
    assert eng.neigh_stats()["checks"] > eng.neigh_stats()["builds"] - 1
    eng.close()
    cls, s, ph, kw, nm, steps = case_inputs("c2_every5")
    every1 = single_engine(sph_amd, s, ph, 0, every=1)
    every1.setup()
    every1.run(steps)
    assert every1.neigh_stats() == dict(builds=steps + 1, dangerous=0, checks=0,
                                        last_build=steps)
    check_fields(every1.get_atoms(), ref, FIELDS, TOL, where="neigh_every 1")
    every1.close()


def test_shock_tube_as_scripted(gpu, sph_amd):
    """shock2d.lmp's neighbor 0.5 bin, neigh_modify every 5 delay 0 check yes with fix
    setforce NULL 0 0: the first rebuild comes at step 20, two of the later ones are
    dangerous"""
    cls, s, ph, kw, nm, steps = case_inputs("shock_tube")
    eng, ref, st = run_single(sph_amd, "shock_tube", 0, make=gas_engine,
                              fields=("f", "drho", "de", "x", "v", "rho", "e"),
                              arm_with=kw["fixes"])
    ns = eng.neigh_stats()
    assert 1 < ns["builds"] < 1 + steps // 5 and ns["dangerous"] >= 1
    eng.close()


def test_stationary_type_never_triggers(gpu, sph_amd):
    """a meso/stationary type whose velocity would cross skin/2 at step 2: the builds come at
    4 and 8, from the moving type alone"""
    eng, ref, _ = run_single(sph_amd, "stationary", 0)
    assert ref.build_steps == [0, 4, 8]
    eng.close()


def _compare_mp(eng, ref, where):
    g = mp_state(eng)
    assert g["x"].shape[0] == ref.s.n and g["ninserted"] == ref.ninserted
    assert np.array_equal(g["type"], ref.s.type)
    assert np.array_equal(eng.neighbor_counts(), ref.numneigh_full()), where
    check_fields(g, ref, MP_FIELDS, TOL, where=where)


@pytest.mark.parametrize("name", ["mp_3d", "mp_2d", "c5_pc"])
def test_multiphase(gpu, sph_amd, name):
    """the multiphase engine, every 1 check yes on the jittered two-phase boxes (builds at 3
    and 6); and C5 with fix phase_change every 3 steps, every 2 check yes: the due steps 1, 4,
    7 rebuild although nothing crossed, and ago restarts there (checks at 3 and 6 only)"""
    cls, s, ph, kw, nm, steps = case_inputs(name)
    ref = oracle_for(name)
    eng = mp_engine(sph_amd, s, ph)
    eng.neigh_modify(*nm)
    eng.setup()
    eng.run(steps)
    print(name, eng.neigh_stats(), ref.build_steps)
    assert eng.neigh_stats() == want_stats(ref)
    _compare_mp(eng, ref, name)
    if name == "c5_pc":
        assert ref.ninserted >= 1 and ref.build_steps == [0, 1, 4, 7]
    eng.close()


def _bricks_run(sph, s, ph, nm, steps):
    world = sph.LocalWorld(2)
    owner = po.brick_owner(s, s.x, BRICKS_PG)
    engines = []
    for r in range(2):
        eng = single_engine(sph, s, ph, 0, procgrid=BRICKS_PG, rank=r,
                            sel=np.nonzero(owner == r)[0])
        eng.comm_local(world, r)
        eng.neigh_modify(*nm)
        engines.append(eng)
    n0 = [e.nlocal for e in engines]
    errors = []

    def work(eng):
        try:
            eng.setup()
            eng.run(steps)
        except Exception as ex:  # surfaced below
            errors.append(ex)

    th = [threading.Thread(target=work, args=(e,)) for e in engines]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=300)
    try:
        assert not any(t.is_alive() for t in th), "brick threads hung"
        assert not errors, errors
        out = {k: np.zeros((s.n, 3)) for k in ("x", "v", "f")}
        out.update({k: np.zeros(s.n) for k in ("rho", "e", "drho", "de")})
        counts, seen = np.zeros(s.n, dtype=np.int32), np.zeros(s.n, dtype=np.int64)
        for eng in engines:
            got = eng.get_atoms()
            seen[got["tag"]] += 1
            for k in out:
                out[k][got["tag"]] = got[k]
            counts[got["tag"]] = eng.neighbor_counts()
        assert (seen == 1).all(), "every atom owned by exactly one brick"
        return out, counts, n0, [e.nlocal for e in engines], [e.neigh_stats() for e in engines]
    finally:
        for e in engines:
            e.close()
        world.close()


def test_two_bricks_flag_crosses_the_ranks(gpu, sph_amd):
    """2x1x1 bricks from rest, only rank 1's atoms fall: both ranks rebuild at the oracle's
    steps and report the same stats, so rank 0 took its decision from rank 1's flag; atoms
    migrate across the face at x = 8 within the run; a second run returns the same bits"""
    cls, s, ph, kw, nm, steps = case_inputs("bricks")
    ref = oracle_for("bricks")
    out, counts, n0, n1, stats = _bricks_run(sph_amd, s, ph, nm, steps)
    print("bricks", stats, n0, n1, ref.build_steps)
    assert stats[0] == stats[1] == want_stats(ref)
    assert ref.ndanger >= 1 and len(ref.build_steps) < 1 + steps // 5 + 1
    assert n1[0] > n0[0] and n1[1] < n0[1] and sum(n1) == sum(n0) == s.n
    assert np.array_equal(counts, ref.numneigh_full())
    check_fields(out, ref, ("rho", "f", "drho", "de", "x", "v"), TOL, where="bricks")
    again = _bricks_run(sph_amd, s, ph, nm, steps)
    assert all(again[0][k].tobytes() == out[k].tobytes() for k in out)
    assert again[4] == stats and np.array_equal(again[1], counts)


def test_argument_errors_and_calling_time(gpu, sph_amd):
    cls, s, ph, kw, nm, steps = case_inputs("c2_still")
    eng = single_engine(sph_amd, s, ph, 1)
    for args in ((0, 0, 1), (-1, 0, 1), (5, -5, 1), (5, 7, 1), (4, 6, 0), (5, 0, 2), (5, 0, -1)):
        with pytest.raises(sph_amd.HipError) as ei:
            eng.neigh_modify(*args)
        assert ei.value.code == -1 and len(str(ei.value)) > 20, args
    with pytest.raises(sph_amd.HipError, match="multiple of every"):
        eng.neigh_modify(5, 7, 1)
    eng.neigh_modify(5, 10, True)     # accepted; the last accepted call holds
    eng.neigh_modify(3, 0, False)
    eng.setup()
    with pytest.raises(sph_amd.HipError, match="before sph_engine_setup") as ei:
        eng.neigh_modify(5, 0, 1)
    assert ei.value.code == -1
    eng.run(7)                        # ... and the rejected calls left it as it was
    assert eng.neigh_stats() == dict(builds=3, dangerous=0, checks=0, last_build=6)
    eng.close()


def test_identical_runs_identical_bits(gpu, sph_amd):
    cls, s, ph, kw, nm, steps = case_inputs("c2_every1")
    res = []
    for _ in range(2):
        eng = single_engine(sph_amd, s, ph, 0)
        eng.neigh_modify(*nm)
        eng.setup()
        eng.run(steps)
        g = eng.get_atoms()
        res.append((b"".join(g[k].tobytes() for k in FIELDS), eng.neigh_stats(),
                    eng.neighbor_counts().tobytes()))
        eng.close()
    assert res[0] == res[1]


@pytest.mark.parametrize("path", [0, 1])
def test_without_neigh_modify(gpu, sph_amd, path):
    """an engine that never calls neigh_modify rebuilds by neigh_every alone and reports it"""
    eng, ref, _ = run_single(sph_amd, "c2_default", path)
    assert ref.nm is None and ref.build_steps == [0, 10]
    assert eng.neigh_stats() == dict(builds=2, dangerous=0, checks=0, last_build=10)
    eng.close()
