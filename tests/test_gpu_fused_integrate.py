"""The block force pass that integrates each row in its epilogue (sph_engine_tune
SPH_TUNE_FUSEINT, the default) against the step that launches the integrate kernel: the same
seeded input run on two engines, the default and one with SPH_TUNE_FUSEINT 0, must leave
every array of get_atoms() bit for bit the same, and the build statistics equal.

Each case first asserts its premise: both engines are on the block path (staged == 1), the
default engine's last run() fused at least one step (STAT_FUSEINT) and the other none.  The
last test arms, one at a time, what keeps a step from fusing and asserts that the flag stays
clear.
"""
import threading

import numpy as np
import pytest

import pyoracle as po
from forcefix_util import wrapped
from neighcheck_util import single_engine
from scenarios import c2_system, c3_system
from test_gpu_engine import engine_for

pytestmark = pytest.mark.gpu

STATS = ("nbr_full", "nghost", "staged", "blk_nbig")   # (as test_gpu_csort.py compares)


def raw(a):
    return np.ascontiguousarray(a).view(np.uint8)


def two_type_physics(stationary_mask=0):
    """rhosum + taitwater on two types with per-pair viscosities (the kernels' several-types
    instantiation: coefficient tables in LDS), one cut"""
    t = np.zeros((3, 3))
    t[1:, 1:] = 3.0
    v = np.zeros((3, 3))
    v[1, 1], v[1, 2], v[2, 2] = 0.1, 0.07, 0.05
    return po.Physics(rhosum_cut=t.copy(), rho0=np.array([0.0, 1.0, 0.5]),
                      c0=np.array([0.0, 10.0, 10.0]), visc=v, tait_cut=t.copy(),
                      stationary_mask=stationary_mask)


def _c2(visc=None, morris=False, gravity=None):
    ph = po.c2_physics()
    if visc is not None:
        ph.visc[1, 1] = visc
    ph.morris = morris
    if gravity is not None:
        ph.gravity = gravity
    return ph


def _fast():
    s = c2_system(12)
    s.v *= 300.0     # sigma 3: at dt 1e-3 an atom passes skin/32 = 0.0094 within a few steps
    return s


# name -> (system, physics, run() calls, BLKUMF)
CASES = {
    "c2_12": (lambda: c2_system(12), _c2, (25,), 0),
    "c2_11_gravity": (lambda: c2_system(11), lambda: _c2(gravity=(0.3, -9.81, 1.7)), (25,), 0),
    "fast_atoms": (_fast, _c2, (25,), 0),
    # (wrapped into the box beforehand: the rebuild's pbc leaves a resting atom where it was)
    "two_types_stationary": (lambda: wrapped(c3_system(10)), lambda: two_type_physics(1 << 2),
                             (25,), 0),
    "no_viscosity": (lambda: c2_system(12), lambda: _c2(visc=0.0), (12,), 0),
    "morris": (lambda: c2_system(12), lambda: _c2(morris=True), (12,), 0),
    "windowed": (lambda: c2_system(12), _c2, (12,), 64),
}


def run_engine(sph, make_s, make_ph, runs, umf, fuse):
    eng = engine_for(sph, make_s(), make_ph())
    if umf:
        eng.tune(eng.TUNE_BLKUMF, umf)
    if fuse is not None:
        eng.tune(eng.TUNE_FUSEINT, fuse)
    eng.setup()
    flags = []
    for n in runs:
        eng.run(n)
        flags.append(eng.stats()["flags"] & eng.STAT_FUSEINT)
    return eng, eng.stats(), eng.get_atoms(), flags


def assert_same(got, want, st, st0):
    assert sorted(got) == sorted(want)
    for k in want:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.shape == b.shape and a.dtype == b.dtype, k
        assert np.array_equal(raw(a), raw(b)), k
    for k in STATS:
        assert st[k] == st0[k], (k, st[k], st0[k])


@pytest.mark.parametrize("name", list(CASES))
def test_fused_equals_unfused(gpu, sph_amd, name):
    make_s, make_ph, runs, umf = CASES[name]
    eng, st, got, fl = run_engine(sph_amd, make_s, make_ph, runs, umf, None)
    eng0, st0, want, fl0 = run_engine(sph_amd, make_s, make_ph, runs, umf, 0)
    print(f"[fuseint] {name}: n {st['nlocal']} builds {st['nbr_builds']} flags {st['flags']:#x} "
          f"/ {st0['flags']:#x} nbig {st['blk_nbig']} refresh {st['inner_refresh']} / "
          f"{st0['inner_refresh']}")
    assert st["staged"] == 1 and st0["staged"] == 1
    assert all(f == eng.STAT_FUSEINT for f in fl), fl
    assert all(f == 0 for f in fl0), fl0
    assert st["nbr_builds"] == st0["nbr_builds"] >= 2
    if name == "c2_11_gravity":
        assert st["nlocal"] % 64 != 0            # the last block of 64 rows is partly dead
    if name == "fast_atoms":
        assert st["inner_refresh"] > 0, "no refresh: the atoms did not pass the margin"
        assert st["inner_refresh"] == st0["inner_refresh"]
    if name == "windowed":
        assert st["blk_nbig"] > 0
    assert_same(got, want, st, st0)
    if name == "two_types_stationary":
        s = make_s()
        fixed = s.type == 2
        assert fixed.any() and not fixed.all()
        assert np.array_equal(got["tag"], np.arange(s.n))    # (one brick: set_atoms order)
        assert np.array_equal(raw(got["x"][fixed]), raw(s.x[fixed]))
        assert np.array_equal(raw(got["v"][fixed]), raw(s.v[fixed]))
        assert not np.array_equal(got["x"][~fixed], s.x[~fixed])


def test_run_splits(gpu, sph_amd):
    """run(7); run(1); run(9) against run(17): the last step of every run() integrates on its
    own (the caller reads its force), a single-step run never fuses"""
    args = (lambda: c2_system(12), _c2)
    eng, st, got, fl = run_engine(sph_amd, *args, (7, 1, 9), 0, None)
    assert fl == [eng.STAT_FUSEINT, 0, eng.STAT_FUSEINT], fl
    eng1, st1, one, fl1 = run_engine(sph_amd, *args, (17,), 0, None)
    assert fl1 == [eng.STAT_FUSEINT] and st["staged"] == 1 and st1["staged"] == 1
    assert_same(got, one, st, st1)
    eng0, st0, want, fl0 = run_engine(sph_amd, *args, (17,), 0, 0)
    assert fl0 == [0] and st0["staged"] == 1
    assert_same(got, want, st, st0)


def _two_bricks(sph):
    s, ph = c2_system(12), po.c2_physics()
    pg = (2, 1, 1)
    world = sph.LocalWorld(2)
    owner = po.brick_owner(s, s.x, pg)
    engines = []
    for r in range(2):
        eng = single_engine(sph, s, ph, 0, procgrid=pg, rank=r, sel=np.nonzero(owner == r)[0])
        eng.comm_local(world, r)
        engines.append(eng)
    errors = []

    def work(eng):
        try:
            eng.setup()
            eng.run(5)
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
        return [e.stats() for e in engines]
    finally:
        for e in engines:
            e.close()
        world.close()


def _armed(sph, what):
    if what == "c3_heat":
        ph = po.c3_physics()
        ph.every = 5
        return engine_for(sph, c3_system(10), ph)
    eng = engine_for(sph, c2_system(12), po.c2_physics())
    if what == "setmeso":
        eng.setmeso("rho", 1.0, region=sph.sphere((6.0, 6.0, 6.0), 2.0))
    elif what == "setforce":
        eng.setforce(0.0, None, None, region=sph.sphere((6.0, 6.0, 6.0), 2.0))
    elif what == "dt_reset":
        eng.dt_reset(2, None, None, 0.01)
    elif what == "check_yes":
        eng.neigh_modify(2, 0, True)
    return eng


@pytest.mark.parametrize("what", ["setmeso", "setforce", "dt_reset", "check_yes", "c3_heat",
                                  "two_bricks"])
def test_does_not_engage(gpu, sph_amd, what):
    """each of these reads or changes f, de, x or dt between the force pass and the next
    integrate (or stages e, or is not one brick): the step runs as it did"""
    if what == "two_bricks":
        sts = _two_bricks(sph_amd)
    else:
        eng = _armed(sph_amd, what)
        eng.setup()
        eng.run(6)
        sts = [eng.stats()]
    for st in sts:
        assert st["staged"] == 1, what
        assert st["flags"] & sph_amd.Engine.STAT_FUSEINT == 0, (what, hex(st["flags"]))
