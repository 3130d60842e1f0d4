"""The neighbour rebuild's counting sorts (bin copy: bin_q; row order: sort_owned) against
the radix sorts they replace: the same engine run twice, once with the default and once with
sph_engine_tune(SPH_TUNE_CSORT, 0), must leave every array bit for bit the same.

Each case first asserts its premise through Engine.csort_paths() and Engine.stats(): the
default run's last build took both counting paths (STAT_CSORT_BINS, STAT_CSORT_ROWS), the
forced run neither.  (On the single-phase row path stats()["flags"] keeps bit 0 alone, as
test_gpu_block_paths asserts; csort_paths() answers on every path.)  The last test packs more
atoms into one bin than the counting path's segment cap allows and asserts that the build
then takes the radix path, with the same results.
"""
import numpy as np
import pytest

import pyoracle as po
from c5_util import mp_engine, mp_state
from scenarios import bubble_physics, bubble_system, c2_system, c3_system
from test_gpu_engine import engine_for

pytestmark = pytest.mark.gpu

CS_CAP = 64            # csrc/sph_engine_kernels.h: the longest segment the counting path orders
STATS = ("nbr_full", "nghost", "staged", "blk_nbig")
BLK_BITS = 0x3e        # flags bits 1 to 5: what the last block build did


def _padded(s, pad=2.0):
    s.periodic = (0, 0, 0)
    s.boxlo = s.boxlo - pad
    s.boxhi = s.boxhi + pad
    return s


def _subset(s, keep):
    for k in ("x", "v", "type", "rho", "e", "cv"):
        setattr(s, k, np.ascontiguousarray(getattr(s, k)[keep]))
    return s


def _cluster(n):
    if n == 27:
        return _padded(c2_system(3))
    return _padded(_subset(c2_system(6), np.arange(n)))


def _sp(make_s, make_ph, every, path=0):
    def build(sph, csort):
        ph = make_ph()
        ph.every = every
        eng = engine_for(sph, make_s(), ph, kernel_path=path)
        if csort is not None:
            eng.tune(eng.TUNE_CSORT, csort)
        return eng
    return build


def _mp(sph, csort):
    """a small C5 box, phase change armed and firing (prob 0.5, Tt below every T), rebuilt
    every step"""
    ph = bubble_physics(8, prob=0.5, Tt=-1.0)
    eng = mp_engine(sph, bubble_system(8), ph)
    if csort is not None:
        eng.tune(eng.TUNE_CSORT, csort)
    return eng


# name -> (engine factory, steps, multiphase)
CASES = {
    "c2_periodic": (_sp(lambda: c2_system(12), po.c2_physics, 10), 25, False),
    "c2_open": (_sp(lambda: _padded(c2_system(12)), po.c2_physics, 10), 25, False),
    "n27": (_sp(lambda: _cluster(27), po.c2_physics, 2), 5, False),
    "n65": (_sp(lambda: _cluster(65), po.c2_physics, 2), 5, False),
    "n129": (_sp(lambda: _cluster(129), po.c2_physics, 2), 5, False),
    "c2_2d": (_sp(lambda: c2_system(30, dim=2), lambda: po.c2_physics(2.5), 10), 25, False),
    "c3_two_types": (_sp(lambda: c3_system(10), po.c3_physics, 5), 12, False),
    "c5_phase_change": (_mp, 12, True),
    "c2_row_path": (_sp(lambda: c2_system(12), po.c2_physics, 10, path=1), 25, False),
}


def raw(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8)


def run_case(sph, make, steps, mp, csort):
    eng = make(sph, csort)
    eng.setup()
    eng.run(steps)
    st = eng.stats()
    got = mp_state(eng) if mp else eng.get_atoms()
    return eng, st, got


def assert_same(got, want, st, st0):
    assert sorted(got) == sorted(want)
    for k in want:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.shape == b.shape and a.dtype == b.dtype, k
        assert np.array_equal(raw(a), raw(b)), k
    for k in STATS:
        assert st[k] == st0[k], (k, st[k], st0[k])
    assert st["flags"] & BLK_BITS == st0["flags"] & BLK_BITS


@pytest.mark.parametrize("name", list(CASES))
def test_counting_equals_radix(gpu, sph_amd, name):
    make, steps, mp = CASES[name]
    eng, st, got = run_case(sph_amd, make, steps, mp, None)
    both = eng.STAT_CSORT_BINS | eng.STAT_CSORT_ROWS
    print(f"[csort] {name}: n {st['nlocal']} ghosts {st['nghost']} builds {st['nbr_builds']} "
          f"flags {st['flags']:#x}")
    assert st["nbr_builds"] >= 3                      # setup and at least two rebuilds
    assert eng.csort_paths() == both, hex(eng.csort_paths())
    if st["staged"] == 1 or mp:   # (the row path's flags carry bit 0 alone)
        assert st["flags"] & both == both, hex(st["flags"])
    eng0, st0, want = run_case(sph_amd, make, steps, mp, 0)
    assert eng0.csort_paths() == 0 and st0["flags"] & both == 0, hex(st0["flags"])
    assert st0["nbr_builds"] == st["nbr_builds"]
    assert_same(got, want, st, st0)


def clumped():
    """the open 12^3 box with 600 more atoms inside a cube of edge 0.5 at its centre: every
    bin edge is at least (h + skin) / 2 = 1.65, so the cube meets at most 8 bins and one of
    them holds more than 600 / 8 = 75 atoms"""
    s = _padded(c2_system(12))
    rng = np.random.default_rng(77)
    m = 600
    c = 0.5 * (s.boxlo + s.boxhi)
    x = c + rng.uniform(-0.25, 0.25, (m, 3))
    s.x = np.ascontiguousarray(np.concatenate([s.x, x]))
    s.v = np.ascontiguousarray(np.concatenate([s.v, np.zeros((m, 3))]))
    for k in ("type", "rho", "e", "cv"):
        a = getattr(s, k)
        setattr(s, k, np.ascontiguousarray(np.concatenate([a, np.full(m, a[0], a.dtype)])))
    return s, x


def test_long_segment_takes_the_radix_path(gpu, sph_amd):
    s, x = clumped()
    size = 0.5 * (3.0 + 0.3)   # the half-size bins' smallest edge: cutneighmax / 2
    # whatever the bins' origin, the clump's largest bin count exceeds the cap
    worst = min(int(np.unique(np.floor((x - o) / size), axis=0, return_counts=True)[1].max())
                for o in np.random.default_rng(5).uniform(0.0, size, (64, 3)))
    assert len(x) / 8 > CS_CAP and worst > CS_CAP, worst

    def make(sph, csort):
        ph = po.c2_physics()
        ph.every = 2
        ph.dt = 1e-9          # (the clump's forces are huge: nothing moves in five steps)
        eng = engine_for(sph, s.copy(), ph)
        if csort is not None:
            eng.tune(eng.TUNE_CSORT, csort)
        return eng

    eng, st, got = run_case(sph_amd, make, 5, False, None)
    print(f"[csort] clump: largest bin >= {worst}, flags {st['flags']:#x} staged {st['staged']}")
    assert st["nbr_builds"] >= 3
    assert eng.csort_paths() & eng.STAT_CSORT_BINS == 0, hex(eng.csort_paths())
    assert st["flags"] & eng.STAT_CSORT_BINS == 0, hex(st["flags"])
    eng0, st0, want = run_case(sph_amd, make, 5, False, 0)
    assert eng0.csort_paths() == 0
    assert_same(got, want, st, st0)
