"""The block-staged pair path's variants that the small engine tests do not reach (every one
of them is a jittered lattice at h = 3, skin 0.3: rows of 147-163 entries in a 256-entry
stride, unions inside the LDS image, constant density):

A. the force pass's windowed walk (blk_force_body, nwin > 1) per physics of blk_force,
   through a rebuild, with the inner rows live;
B. rows past the register preload (BlkArgs::pre() false: the NCH = 0 instantiations);
C. the rebuild's retries (a row outgrows the slot-row stride, a block the small candidate
   image, both in one build) under a compression that grows the rows by ~1.6x;
D. degenerate blocks: n < R, a last block with one live row, a row without neighbours;
E. a build without inner rows (skin = 0).

The reference is always pyoracle.RefRun(spread=True); the bars are test_gpu_engine's: counts
bit-exact per particle, rho f drho de x v e at 1e-10 normwise + conftest.check_fields'
elementwise bar.  Every test first asserts its premise on the oracle alone, and then through
Engine.stats() (staged, blk_nbig, inner_*, the STAT_BLK_* flags) that the path it is about
ran.  What each case reported is printed (pytest -s / -rP shows it).
"""
import numpy as np
import pytest

import pyoracle as po
from scenarios import c2_system, c3_system
from test_gpu_engine import FIELDS, compare, engine_for

pytestmark = pytest.mark.gpu

PRELOAD = 256  # BLK_NCH * U * G: the longest slot row the pair passes preload into registers


class Snap:
    """An oracle run's compared state at one step, frozen (the references are computed once
    and shared between the cases of a test): what compare / check_fields read of a RefRun."""

    def __init__(self, ref):
        self._f = {k: np.array(ref.field(k), copy=True) for k in FIELDS}
        self._s = {k: np.array(ref.spread(k), copy=True) for k in FIELDS}
        self.nn = ref.numneigh_full().copy()
        self.step = ref.step
        for a in list(self._f.values()) + list(self._s.values()) + [self.nn]:
            a.setflags(write=False)

    def field(self, k):
        return self._f[k]

    def spread(self, k):
        return self._s[k]

    def numneigh_full(self):
        return self.nn


def oracle_snaps(s, ph, at):
    """RefRun(spread=True) of (s, ph): snapshots at setup (key 0) and after the steps `at`,
    and the largest displacement at the last step since the last rebuild before it"""
    ref = po.RefRun(s, ph, spread=True)
    ref.setup()
    out = {0: Snap(ref)}
    xb = ref.s.x.copy()
    for k in sorted(at):
        while ref.step < k:
            ref.run(1)
            if ref.last_build == ref.step:
                xb = ref.s.x.copy()
        out[k] = Snap(ref)
    moved = float(np.sqrt(((ref.s.x - xb) ** 2).sum(1)).max())
    for v in out.values():
        for k in FIELDS:
            assert np.isfinite(v.field(k)).all() and np.isfinite(v.spread(k)).all()
    return out, moved


def flag_names(eng, flags):
    names = ("STAT_BLK_R32", "STAT_BLK_BIGIMG", "STAT_BLK_NOPRE", "STAT_BLK_ROWRETRY",
             "STAT_BLK_IMGRETRY")
    return "|".join(n[9:] for n in names if flags & getattr(eng, n)) or "-"


def report(what, eng, st, flags=None):
    flags = st["flags"] if flags is None else flags
    print(f"[block paths] {what}: staged {st['staged']} flags {flag_names(eng, flags)} "
          f"blk_nbig {st['blk_nbig']} stage_max {st['stage_max']} inner_rows "
          f"{st['inner_rows']} inner_live {st['inner_live']}")


def check_step(eng, snap, path=0):
    assert np.array_equal(eng.neighbor_counts(), snap.numneigh_full()), snap.step
    compare(eng, snap, path=path)


# ---- the physics of A (make_config level) ------------------------------------------------
def _one_type_e(s):
    """a one-type lattice carries e = 0 everywhere: give the heat term differences to sum"""
    s.e = 1.0 + 0.1 * np.random.default_rng(99).uniform(-1.0, 1.0, s.n)
    return s


def _with_heat(ph, nt, h):
    a = np.zeros((nt + 1, nt + 1))
    a[1:, 1:] = 0.1
    t = np.zeros((nt + 1, nt + 1))
    t[1:, 1:] = h
    ph.heat, ph.alpha, ph.heat_cut = True, a, t
    return ph


def _c2():
    return c2_system(12), po.c2_physics(), 10, 12


def _c2_novisc():
    ph = po.c2_physics()
    ph.visc = np.zeros_like(ph.visc)
    return c2_system(12), ph, 10, 12


def _morris1():
    ph = po.c2_physics()
    ph.morris = True
    return c2_system(12), ph, 10, 12


def _morris1_heat():
    ph = _with_heat(po.c2_physics(), 1, 3.0)
    ph.morris = True
    return _one_type_e(c2_system(12)), ph, 10, 12


def _c3():
    return c3_system(10), po.c3_physics(), 5, 7


def _monaghan2():
    """two types, rhosum + Monaghan taitwater in 3-D (3x3 tables, masses 1.0 / 0.5)"""
    t = np.zeros((3, 3))
    t[1:, 1:] = 3.0
    v = np.zeros((3, 3))
    v[1:, 1:] = 0.1
    ph = po.Physics(rhosum_cut=t.copy(), rho0=np.array([0.0, 1.0, 0.5]),
                    c0=np.array([0.0, 10.0, 10.0]), visc=v, tait_cut=t.copy())
    return c3_system(10), ph, 5, 7


def _heat_only():
    ph = po.c3_physics()
    ph.tait = False
    return c3_system(10), ph, 5, 7


def _c2_2d():
    return c2_system(30, dim=2), po.c2_physics(2.5), 10, 12


PHYSICS = {"c2": _c2, "c2_novisc": _c2_novisc, "morris1": _morris1,
           "morris1_heat": _morris1_heat, "c3": _c3, "monaghan2": _monaghan2,
           "heat_only": _heat_only, "c2_2d": _c2_2d}
NEW_PHYSICS = ("heat_only", "morris1", "morris1_heat", "monaghan2")

# B: h = 4, rows past the preload
LONG = {"c2_long": lambda: (c2_system(12), po.c2_physics(4.0), 10, 12),
        "c3_long": lambda: (c3_system(10), po.c3_physics(4.0), 5, 12)}

_CACHE = {}


def scenario(name):
    """(system, physics with its rebuild period set, steps, snapshots, displacement since the
    last rebuild) of a named scenario; the oracle runs once per session"""
    if name not in _CACHE:
        s, ph, every, steps = {**PHYSICS, **LONG}[name]()
        ph.every = every
        snaps, moved = oracle_snaps(s, ph, (1, steps))
        _CACHE[name] = (s, ph, steps, snaps, moved)
    return _CACHE[name]


def premise_common(ph, steps, snaps, moved):
    # a rebuild inside the run and at least two steps past it (every < steps - 1): the block
    # force pass and the passes on the inner rows of a rebuild are both compared
    assert ph.every + 2 <= steps
    # no atom moves past half the inner rows' margin (skin / 16) after the last rebuild: the
    # run ends on inner rows
    assert moved < 0.5 * 0.0625 * ph.skin, moved
    end = snaps[steps]
    if ph.tait:
        assert np.abs(end.field("f")).max() > 0 and np.abs(end.field("drho")).max() > 0
    else:  # heat conduction alone moves nothing but e
        assert np.abs(end.field("f")).max() == 0 and np.abs(end.field("drho")).max() == 0
    if ph.heat or ph.tait:
        assert np.abs(end.field("de")).max() > 0


A_CASES = [(n, u) for n in PHYSICS for u in (0, 64)] + [("c2", 16), ("c2", 640)]


@pytest.mark.parametrize("name,umf", A_CASES)
def test_windowed_force_walk(gpu, sph_amd, name, umf):
    """A. setup, one step, then across a rebuild to the end, the force pass's LDS image capped
    at umf records (0: the engine's own choice, no window at these sizes)."""
    s, ph, steps, snaps, moved = scenario(name)
    premise_common(ph, steps, snaps, moved)
    # rows inside the register preload: these are the NCH = BLK_NCH walks (B has the others)
    assert max(v.numneigh_full().max() for v in snaps.values()) <= PRELOAD
    if ph.heat and s.ntypes == 1:
        assert np.ptp(s.e) > 0
    eng = engine_for(sph_amd, s, ph)
    if umf:
        eng.tune(eng.TUNE_BLKUMF, umf)
    eng.setup()
    check_step(eng, snaps[0])
    eng.run(1)
    st = eng.stats()
    report(f"A {name} umf {umf} step 1", eng, st)
    assert st["staged"] == 1 and st["inner_rows"] == 1 and st["inner_live"] == 1
    if umf:
        assert st["blk_nbig"] > 0
    check_step(eng, snaps[1])
    eng.run(steps - 1)
    st = eng.stats()
    report(f"A {name} umf {umf} step {steps}", eng, st)
    assert st["step"] == steps and st["staged"] == 1
    assert st["nbr_builds"] >= 2                       # (the rebuild inside the run)
    assert not st["flags"] & eng.STAT_BLK_NOPRE
    if umf:
        assert st["blk_nbig"] > 0
    assert st["inner_rows"] == 1 and st["inner_live"] == 1
    check_step(eng, snaps[steps])


@pytest.mark.parametrize("name", NEW_PHYSICS)
def test_new_physics_on_the_row_path(gpu, sph_amd, name):
    """The physics A adds to the suite, on the row path (where a wide union falls back to)."""
    s, ph, steps, snaps, moved = scenario(name)
    premise_common(ph, steps, snaps, moved)
    eng = engine_for(sph_amd, s, ph, kernel_path=1)
    eng.setup()
    check_step(eng, snaps[0], path=1)
    eng.run(1)
    check_step(eng, snaps[1], path=1)
    eng.run(steps - 1)
    st = eng.stats()
    assert st["staged"] == 0 and st["flags"] & ~eng.STAT_RHO_FUSED == 0
    check_step(eng, snaps[steps], path=1)


# ---- B: rows past the preload -----------------------------------------------------------
@pytest.mark.parametrize("name,umf", [(n, u) for n in LONG for u in (0, 64)])
def test_long_rows(gpu, sph_amd, name, umf):
    """B. h = 4: rows of ~330 entries, which no 256-entry stride holds, so the rho, force and
    inner passes run their NCH = 0 instantiations (BlkSlots::walk with the chunk prefetch)."""
    s, ph, steps, snaps, moved = scenario(name)
    premise_common(ph, steps, snaps, moved)
    assert all(v.numneigh_full().max() > PRELOAD for v in snaps.values())
    eng = engine_for(sph_amd, s, ph)
    if umf:
        eng.tune(eng.TUNE_BLKUMF, umf)
    eng.setup()
    check_step(eng, snaps[0])
    eng.run(1)
    st = eng.stats()
    report(f"B {name} umf {umf} step 1", eng, st)
    assert st["staged"] == 1 and st["flags"] & eng.STAT_BLK_NOPRE
    assert st["inner_rows"] == 1 and st["inner_live"] == 1
    if umf:
        assert st["blk_nbig"] > 0
    check_step(eng, snaps[1])
    eng.run(steps - 1)
    st = eng.stats()
    report(f"B {name} umf {umf} step {steps}", eng, st)
    assert st["staged"] == 1 and st["flags"] & eng.STAT_BLK_NOPRE
    assert st["nbr_builds"] >= 2
    if umf:
        assert st["blk_nbig"] > 0
    assert st["inner_rows"] == 1 and st["inner_live"] == 1
    check_step(eng, snaps[steps])


# ---- C: the rebuild's retries -----------------------------------------------------------
def _padded(s, pad=2.0):
    s.periodic = (0, 0, 0)
    s.boxlo = s.boxlo - pad
    s.boxhi = s.boxhi + pad
    return s


def _collapsing_cluster():
    """the free cluster collapsing on its centre: v -= 15 (x - <x>)"""
    s = _padded(c2_system(12))
    s.v -= 15.0 * (s.x - s.x.mean(0))
    return s


def _converging_box():
    """the periodic box with a flow converging on its centre,
    v -= 20 L / (2 pi) sin(2 pi (x - c) / L) per axis: the bulk, ghosts around every block"""
    s = c2_system(12)
    ell = s.boxhi - s.boxlo
    s.v -= 20.0 * ell / (2 * np.pi) * np.sin(2 * np.pi * (s.x - 0.5 * (s.boxlo + s.boxhi)) / ell)
    return s


# (system, h, steps per rebuild, the flags the run must raise, ... in ONE build)
RETRY = {"cluster": (_collapsing_cluster, 3.0, 2, ("NOPRE", "ROWRETRY"), ()),
         "box": (_converging_box, 3.2, 3, ("NOPRE", "ROWRETRY", "IMGRETRY"),
                 ("ROWRETRY", "IMGRETRY"))}


@pytest.mark.parametrize("case", list(RETRY))
def test_retry_ladder_under_compression(gpu, sph_amd, case):
    """C. Rebuilds under a compression that outruns what each build sized from the one before;
    12 steps, the block path must hold through all of them: counts and staged after every
    step, fields after steps 1, 6 and 12.

    cluster (every 2): the longest row grows 162 -> 267, past the build's slack over the
    setup's rows (1.25 n0 + 16 = 218, a 256-entry stride: the stride doubles, ROWRETRY) and
    past the preload (NOPRE).  Its candidate sets (the atoms within the neighbour cutoff of a
    block's bounding box, k_blk_build) hardly grow, 1024 -> 1089 of the small image's 1536: a
    free cluster has nothing around it.

    box (h = 3.2, every 3): the periodic bulk, rows 185 -> 288, rho up to 2.0.  The candidate
    sets stay at 1350-1385 through four builds, which keep the small image, and reach 1552 at
    the build of step 12: that build overflows the small image (IMGRETRY), repeats with the
    large one, overflows the 256-entry stride (ROWRETRY), repeats with 512 and succeeds --
    both causes in one build, each with its own budget (build_blk_shape).

    The 32-row and large-image (k_blk_neigh) rungs are reported, not required: neither case
    reaches them."""
    make, h, every, need, together = RETRY[case]
    s = make()
    ph = po.c2_physics(h)
    ph.every = every
    ref = po.RefRun(s, ph, spread=True)
    ref.setup()
    snaps = [Snap(ref)]
    for k in range(1, 13):
        ref.run(1)
        snaps.append(Snap(ref))
    # the premise, on the oracle alone: the rows outgrow the slack a build leaves over the
    # setup's (and with them the density that fills the candidate sets), and the preload
    rows = [int(v.numneigh_full().max()) for v in snaps]
    assert rows[-1] > 1.25 * rows[0] + 16 and rows[-1] > PRELOAD, rows
    assert all(np.isfinite(v.field(k)).all() for v in snaps for k in FIELDS)

    eng = engine_for(sph_amd, s, ph)
    eng.setup()
    st = eng.stats()
    report(f"C {case} setup (oracle's longest row {rows[0]})", eng, st)
    assert st["staged"] == 1
    check_step(eng, snaps[0])
    seen = both = 0
    want_both = sum(getattr(eng, "STAT_BLK_" + n) for n in together)
    for k in range(1, 13):
        eng.run(1)
        st = eng.stats()
        seen |= st["flags"]
        if want_both and st["flags"] & want_both == want_both:
            both += 1
        report(f"C {case} step {k} (oracle's longest row {rows[k]})", eng, st)
        assert np.array_equal(eng.neighbor_counts(), snaps[k].numneigh_full()), k
        assert st["staged"] == 1, k
        if k in (1, 6, 12):
            compare(eng, snaps[k], path=0)
    report(f"C {case} all steps", eng, st, seen)
    for n in need:
        assert seen & getattr(eng, "STAT_BLK_" + n), flag_names(eng, seen)
    if together:  # (the per-cause budget: one build that repeats for both causes and stays)
        assert both > 0, "no build repeated for " + " and ".join(together)


# ---- E: a build without inner rows ------------------------------------------------------
def test_zero_skin_builds_no_inner_rows(gpu, sph_amd):
    """E. skin = 0 (a rebuild every step): the inner rows' margin, a sixteenth of the skin, is
    zero, so k_blk_build runs its instantiation without the inner ballot and the passes walk
    the full rows -- every other engine test has a skin and with it inner rows."""
    s = c2_system(10)
    ph = po.c2_physics()
    ph.skin, ph.every = 0.0, 1
    snaps, _ = oracle_snaps(s, ph, (1, 3))
    assert np.abs(snaps[3].field("f")).max() > 0
    eng = engine_for(sph_amd, s, ph)
    eng.setup()
    for k, steps in ((0, 0), (1, 1), (3, 2)):
        if steps:
            eng.run(steps)
        st = eng.stats()
        report(f"E skin 0 step {k}", eng, st)
        assert st["step"] == k and st["staged"] == 1
        assert st["inner_rows"] == 0 and st["inner_live"] == 0 and st["inner_refresh"] == 0
        check_step(eng, snaps[k])
    assert st["nbr_builds"] >= 4


# ---- D: degenerate blocks ---------------------------------------------------------------
def _subset(s, keep):
    for k in ("x", "v", "type", "rho", "e", "cv"):
        setattr(s, k, np.ascontiguousarray(getattr(s, k)[keep]))
    return s


def _cluster(n):
    if n == 27:
        return _padded(c2_system(3))
    if n == 65:
        return _padded(_subset(c2_system(5), np.arange(65)))
    s = _subset(c2_system(6), np.arange(129))
    s.x[128] = s.x[:128].max(0) + 10.0      # >= 10 from every other atom along each axis
    s.boxhi = np.maximum(s.boxhi, s.x[128] + 0.5)
    return _padded(s)


@pytest.mark.parametrize("n", [27, 65, 129])
def test_degenerate_blocks(gpu, sph_amd, n):
    """D. Free clusters: 27 atoms (one partial block), 65 (a second block with one live
    row), 129 with one atom 10 away from the rest (a row without neighbours: its rho is the
    self term, its f, drho and de exact zeros)."""
    s = _cluster(n)
    assert s.n == n
    ph = po.c2_physics()
    ph.every = 1
    ref = po.RefRun(s, ph, spread=True)
    ref.setup()
    lone = None
    if n == 129:
        lone = 128
        d = np.sqrt(((s.x[:128] - s.x[128]) ** 2).sum(1))
        assert d.min() >= 10.0
        assert ref.numneigh_full()[lone] == 0 and ref.numneigh_full()[:128].min() > 0
    eng = engine_for(sph_amd, s, ph)
    eng.setup()
    for k in range(4):
        if k:
            ref.run(1)
            eng.run(1)
        st = eng.stats()
        report(f"D n {n} step {k}", eng, st)
        # (n < R, a one-row block and an empty row are all block-path shapes: no fallback is
        # documented for them)
        assert st["staged"] == 1
        assert np.array_equal(eng.neighbor_counts(), ref.numneigh_full()), k
        got = compare(eng, ref, path=0)
        if lone is not None:
            assert eng.neighbor_counts()[lone] == 0
            for f in ("f", "drho", "de"):
                assert np.all(ref.field(f)[lone] == 0.0)
                assert np.all(got[f][lone] == 0.0), (k, f, got[f][lone])
