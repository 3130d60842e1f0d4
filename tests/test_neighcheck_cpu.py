"""neigh_modify every / delay / check without a device: the oracle-side restatement of the two
Verlet loops pinned to pyoracle's own, the margin of every GPU case's displacement checks, the
schedules those cases were built to have, and sph_engine_neigh_modify's argument errors."""
import dataclasses

import numpy as np
import pytest

import pyoracle as po
from neighcheck_util import (BRICKS_PG, CASES, EXPECTED, NcMpRefRun, NcRefRun, case_inputs,
                             oracle_for)
from scenarios import bubble_physics, bubble_system, c2_system

FIELDS = ("x", "v", "rho", "e", "f", "drho", "de")


def _same(a, b, fields):
    for k in fields:
        assert np.array_equal(np.asarray(a.field(k)), np.asarray(b.field(k))), k
    assert np.array_equal(a.numneigh_full(), b.numneigh_full())


def test_restated_loop_is_refrun():
    """check off, delay 0, every = ph.every: bit for bit RefRun.run, builds at the same steps"""
    s = c2_system(6)
    ph = po.c2_physics()
    ph.every = 5
    want = po.RefRun(s, ph)
    want.setup()
    builds = [0]
    for step in range(1, 13):
        want.run(1)
        if want.last_build == step:
            builds.append(step)
    for nm in (None, (ph.every, 0, 0)):
        got = NcRefRun(s, ph)
        got.nm = nm
        got.setup()
        got.run(12)
        _same(got, want, FIELDS)
        assert got.build_steps == builds == [0, 5, 10] and got.last_build == want.last_build


def test_restated_loop_is_mprefrun():
    """the same for MpRefRun on the smallest C5 box, fix phase_change armed (every step) and
    not (every 2)"""
    for pc in (True, False):
        s = bubble_system(8)
        ph = bubble_physics(8, prob=0.5, Tt=-1.0, pc=pc)
        if not pc:
            ph = dataclasses.replace(ph, every=2)
        want = po.MpRefRun(s, ph)
        want.setup()
        builds = [0]
        for step in range(1, 13):
            want.run(1)
            if want.last_build == step:
                builds.append(step)
        got = NcMpRefRun(s, ph)
        got.setup()
        got.run(12)
        _same(got, want, FIELDS + ("rmass", "cv", "cg"))
        assert got.ninserted == want.ninserted and (not pc or want.ninserted >= 1)
        assert got.build_steps == builds


@pytest.mark.parametrize("name", sorted(CASES))
def test_input_margin(name):
    """no displacement check of a GPU case comes within 1e-6 of a tie: the engine's positions
    differ from the oracle's at the 1e-10 level, and a tie could decide either way"""
    ref = oracle_for(name, shadows=False)
    nm = case_inputs(name)[4]
    if nm is not None and nm[2]:
        assert ref.checks, "a check-yes case without a check"
    for step, ratio in ref.checks:
        assert not (np.abs(ratio - 1.0) <= 1e-6).any(), (name, step)
    print(name, "builds", ref.build_steps, "danger", ref.ndanger, "check max",
          [f"{m:.3f}" for m in ref.check_max])


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_expected_schedule(name):
    ref = oracle_for(name, shadows=False)
    builds, danger, eligible = EXPECTED[name]
    assert ref.build_steps == builds
    assert ref.ndanger == danger
    assert ref.eligible_steps == eligible
    nm = case_inputs(name)[4]
    assert len(ref.checks) == (len(eligible) if nm is not None and nm[2] else 0)


def test_stationary_atoms_never_trigger():
    ref = oracle_for("stationary", shadows=False)
    st = ref.s.type == 2
    assert st.any() and np.abs(ref.s.v[st]).max() > 10.0
    for _, ratio in ref.checks:
        assert not ratio[st].any()


def test_bricks_case_only_rank1_triggers_and_migrates():
    """the premise of the bricks test: every check that fires is raised by atoms rank 1 owns
    alone, rank 0's stay far below the trigger, and atoms cross the brick face in the run"""
    cls, s, ph, kw, nm, steps = case_inputs("bricks")
    ref = oracle_for("bricks", shadows=False)
    own0 = po.brick_owner(s, s.x, BRICKS_PG)
    assert (own0 == (s.type - 1)).all() and (own0 == 0).any() and (own0 == 1).any()
    fired = [(st, r) for st, r in ref.checks if (r > 1.0).any()]
    assert len(fired) >= 2 and len(ref.build_steps) == 1 + len(fired)
    assert len(fired) < len(ref.checks), "no skipped rebuild"
    for _, r in ref.checks:
        assert r[s.type == 1].max() < 0.5
    own1 = po.brick_owner(ref.s, ref.s.x, BRICKS_PG)
    assert ((own0 == 1) & (own1 == 0)).sum() >= 1


def test_argument_errors(sph_amd):
    """the arguments are judged before the engine is touched, so a NULL engine reaches every
    argument error without a device; a live engine and the calling-time rule are in
    test_gpu_neighcheck.py"""
    L = sph_amd.load()
    for args, text in (((0, 0, 1), b"every"), ((-3, 0, 0), b"every"), ((5, -1, 1), b"delay"),
                       ((5, 7, 1), b"Neighbor delay must be 0 or multiple of every setting"),
                       ((2, 3, 0), b"Neighbor delay must be 0 or multiple of every setting"),
                       ((5, 0, 2), b"check"), ((5, 10, -1), b"check"),
                       ((5, 10, 1), b"NULL"), ((1, 0, 0), b"NULL")):
        assert L.sph_engine_neigh_modify(None, *args) == -1, args      # SPH_HIP_EINVAL
        assert text in L.sph_hip_last_error(), (args, L.sph_hip_last_error())
    st = sph_amd.NeighStats()
    assert L.sph_engine_neigh_stats(None, st) == -1
    assert b"NULL" in L.sph_hip_last_error()
