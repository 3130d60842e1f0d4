"""fix phase_change on the device-resident engine (sph_engine::phase_change, csrc/sph_pc.h)
beyond the periodic bubble of test_c5_engine.py: ENERGY mode (the threshold reads the engine's
own dt), Tt and Tc deciding per atom, walls (the placement ladder's retries, its second ladder
and the give-up exit; the ghost slots of a box with non-periodic swaps), three types with
from 3 to 2, calls every other step between forward-comm steps, two ranks between walls, and
a restart read into an armed engine and continued.  The cases, and the premises each is
asserted to meet on the oracle, are in pc_engine_util.py (test_pc_engine_cpu.py runs them
without a GPU).

Engine against po.MpRefRun(s, ph, spread=True) at setup and after every step: atom count,
ninserted, types and full-list neighbour counts exact; x v rho e rmass cv cg f de through
conftest.check_fields at 1e-10 (normwise, and per element up to the oracle's own spread).

Measured on an MI355X: profiles/pc_engine/README.md."""
import numpy as np
import pytest

import pyoracle as po
from c5_util import bricks_step, mp_collect, mp_state
from conftest import check_fields, elem_ratio, rel_err
from pc_engine_util import (CASES, PG_WALLS, RESTART_AT, case, oracle_records, pc_bricks,
                            pc_engine, premises, procgrid, restart_ref, restart_system)

TOL = 1e-10
FIELDS = ("x", "v", "rho", "e", "rmass", "cv", "cg", "f", "de")


def _figures(name, step, g, ref, fig):
    """the worst plain normwise error and bar ratio so far (printed; the asserts are
    check_fields')"""
    for k in FIELDS:
        want = ref.field(k)
        if np.abs(np.asarray(want)).max() == 0:
            continue
        br = ref.build_rel(k)
        fig["normwise"] = max(fig["normwise"], rel_err(g[k], want))
        fig["bar_ratio"] = max(fig["bar_ratio"],
                               elem_ratio(g[k], want, ref.spread(k),
                                          tol=max(TOL, br) if br is not None else TOL))


def _compare(name, step, g, counts, ref, fig):
    s = ref.s
    assert g["x"].shape[0] == s.n, (name, step, g["x"].shape[0], s.n)
    assert g["ninserted"] == ref.ninserted, (name, step, g["ninserted"], ref.ninserted)
    assert np.array_equal(g["type"], s.type), (name, step)
    assert np.array_equal(counts, ref.numneigh_full()), (name, step)
    _figures(name, step, g, ref, fig)
    check_fields(g, ref, FIELDS, TOL, where=(name, step))


def _flags(eng):
    return hex(eng.stats()["flags"])


SINGLE = [n for n in CASES if n not in ("bricks-walls", "restart")]


@pytest.mark.gpu
@pytest.mark.parametrize("name", SINGLE)
def test_pc_engine(gpu, sph_amd, name):
    s, ph, steps = case(name)
    premises(name)
    ref = po.MpRefRun(s, ph, spread=True)
    ref.setup()
    eng = pc_engine(sph_amd, s, ph)
    fig = dict(normwise=0.0, bar_ratio=0.0)
    try:
        eng.setup()
        _compare(name, 0, mp_state(eng), eng.neighbor_counts(), ref, fig)
        seen = []
        for step in range(1, steps + 1):
            ref.run(1)
            eng.run(1)
            _compare(name, step, mp_state(eng), eng.neighbor_counts(), ref, fig)
            seen.append(ref.ninserted)
        print(f"[pc engine] {name}: ninserted by step {seen} normwise {fig['normwise']:.2e} "
              f"bar ratio {fig['bar_ratio']:.3f} flags {_flags(eng)}")
    finally:
        eng.close()
    assert ref.ninserted >= 1


@pytest.mark.gpu
def test_pc_engine_bricks_walls(gpu, sph_amd):
    """walls-y over two ranks in y: each rank's own Park-Miller stream, pc_owns rejecting at
    the brick face and at the walls, the created atoms' tags rank by rank"""
    name = "bricks-walls"
    s, ph, steps = case(name)
    out = premises(name)
    assert procgrid(name) == PG_WALLS and min(out["per_rank"]) >= 1
    ref = po.MpRefRun(s, ph, procgrid=PG_WALLS, spread=True)
    ref.setup()
    world, engines = pc_bricks(sph_amd, s, ph, PG_WALLS, po.brick_owner(s, s.x, PG_WALLS))
    fig = dict(normwise=0.0, bar_ratio=0.0)
    try:
        per = None
        for step in range(steps + 1):
            if step:
                ref.run(1)
            bricks_step(engines, (lambda e: e.run(1)) if step else (lambda e: e.setup()))
            g = mp_collect(engines, ref.s.n)
            _compare(name, step, g, g["counts"], ref, fig)
            per = [int(mp_state(e)["ninserted"]) for e in engines]
        assert per == out["per_rank"], (per, out["per_rank"])
        print(f"[pc engine] {name}: ninserted per rank {per} normwise {fig['normwise']:.2e} "
              f"bar ratio {fig['bar_ratio']:.3f}")
    finally:
        for e in engines:
            e.close()
        world.close()


@pytest.mark.gpu
def test_pc_engine_restart(gpu, sph_amd):
    """three steps with the fix armed, write_restart; a fresh engine with the fix armed reads
    the records, sets up and runs three more -- against the oracle restarted from the same
    records (their atoms in tag order, cg and vest as the records carry them)"""
    name = "restart"
    s, ph, steps = case(name)
    premises(name)
    fig = dict(normwise=0.0, bar_ratio=0.0)
    ref = po.MpRefRun(s, ph, spread=True)
    ref.setup()
    ref.run(RESTART_AT)
    eng = pc_engine(sph_amd, s, ph)
    eng2 = None
    try:
        eng.setup()
        eng.run(RESTART_AT)
        _compare(name, RESTART_AT, mp_state(eng), eng.neighbor_counts(), ref, fig)
        rec = eng.write_restart()
        assert ref.ninserted >= 1 and rec.shape == (s.n + ref.ninserted, 21)
        s2, cg, vest = restart_system(s, rec)
        ref2 = restart_ref(s2, ph, cg, vest, spread=True)
        ref2.setup()
        eng2 = pc_engine(sph_amd, s, ph)   # (armed, holding the first atoms until the read)
        eng2.read_restart(rec)
        assert np.array_equal(eng2.write_restart(), rec)
        eng2.setup()
        _compare(name, "0'", mp_state(eng2), eng2.neighbor_counts(), ref2, fig)
        for step in range(1, steps - RESTART_AT + 1):
            ref2.run(1)
            eng2.run(1)
            _compare(name, f"{step}'", mp_state(eng2), eng2.neighbor_counts(), ref2, fig)
        assert ref2.ninserted >= 1 and eng2.nlocal > rec.shape[0]
        print(f"[pc engine] {name}: ninserted {ref.ninserted} + {ref2.ninserted} normwise "
              f"{fig['normwise']:.2e} bar ratio {fig['bar_ratio']:.3f} flags {_flags(eng2)}")
    finally:
        eng.close()
        if eng2 is not None:
            eng2.close()
