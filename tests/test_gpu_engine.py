"""GPU parity of the device-resident engine (sph_engine_* C ABI) against the oracle's
reference-faithful Verlet driver (pyoracle.RefRun: half lists, Newton scatter, reverse
comm -- src/verlet.cpp:88-139, 222-308 around the USER-SPH styles).

* neighbor counts within cut+skin: bit-exact per particle (Neighbor::full_bin membership)
* rho / f / drho / de / x / v / e: 1e-10 normwise relative (north_star tolerance)
"""
import numpy as np
import pytest

import pyoracle as po
from conftest import check_fields, elem_rel_err, rel_err
from scenarios import c2_system, c3_system

pytestmark = pytest.mark.gpu
TOL = 1e-10


def engine_for(sph_amd, s, ph: po.Physics, sort=1, every=None, kernel_path=0):
    nt = s.ntypes
    kw = {}
    if ph.rhosum_nstep > 0:
        kw["rhosum"] = dict(nstep=ph.rhosum_nstep, cut=ph.rhosum_cut)
    if ph.tait:
        kw["tait"] = dict(rho0=ph.rho0, c0=ph.c0, visc=ph.visc, cut=ph.tait_cut, morris=ph.morris)
    if ph.heat:
        kw["heat"] = dict(alpha=ph.alpha, cut=ph.heat_cut)
    cfg = sph_amd.make_config(s.dim, nt, s.boxlo, s.boxhi, s.periodic, s.mass, ph.skin, ph.dt,
                              neigh_every=every or ph.every, sort=sort,
                              kernel_path=kernel_path, stationary_mask=ph.stationary_mask,
                              gravity=ph.gravity, gravity_mask=ph.gravity_mask, **kw)
    eng = sph_amd.Engine(cfg)
    eng.set_atoms(s.x, s.v, s.type, s.rho, s.e, s.cv)
    return eng


FIELDS = ("rho", "f", "drho", "de", "x", "v", "e")


def compare(eng, ref, tol=TOL, path=None):
    """normwise 1e-10 and SURVEY 8(d)'s elementwise bar (conftest.elem_ratio: 1e-10 per
    element, or k x the oracle's own reordering spread where an element's sum cancels --
    the RefRuns here carry their shadow runs, spread=True)"""
    if path is not None:  # the requested pair path really ran (no silent fallback)
        assert eng.stats()["staged"] == (1 if path == 0 else 0)
    got = eng.get_atoms()
    check_fields(got, ref, FIELDS, tol)
    return got


PATHS = [0, 1]   # 0 = block-staged LDS unions (production), 1 = row path (global gathers)


@pytest.mark.parametrize("sort,path,umf", [(1, 0, 0), (1, 0, 64), (0, 0, 0), (1, 1, 0),
                                           (0, 1, 0)])
def test_setup_c2(gpu, sph_amd, sort, path, umf):
    """path 0 = block-staged passes (LDS unions, 16-bit slot rows built from the bins), 1 =
    the row path.  umf = 64 caps the force pass's LDS image at 64 records (sph_engine_tune
    SPH_TUNE_BLKUMF), so the build counts nearly every block as windowed (blk_nbig) -- setup
    itself runs the block rhosum and the CSR setup force (setup_forces_full), not the windowed
    force walk: test_gpu_block_paths.py steps such engines --; unsorted rows
    (sort 0) make blocks too wide for the build's candidate image, so the build takes its
    large-image variant."""
    s = c2_system(12)
    ph = po.c2_physics()
    ref = po.RefRun(s, ph, spread=True)
    ref.setup()
    eng = engine_for(sph_amd, s, ph, sort=sort, kernel_path=path)
    if umf:
        eng.tune(eng.TUNE_BLKUMF, umf)
    eng.setup()
    if umf:
        assert eng.stats()["blk_nbig"] > 0
    assert eng.stats()["staged"] == (1 if path == 0 else 0)
    # neighbor membership: bit-exact counts per particle
    assert np.array_equal(eng.neighbor_counts(), ref.numneigh_full())
    st = eng.stats()
    assert st["nghost"] == ref.g.nghost
    assert st["nbr_full"] == int(ref.foff[-1])
    got = compare(eng, ref)
    assert elem_rel_err(got["rho"], ref.s.rho) < 1e-13


@pytest.mark.parametrize("path", PATHS)
def test_run_c2_with_rebuilds(gpu, sph_amd, path):
    s = c2_system(12)
    ph = po.c2_physics()
    ref = po.RefRun(s, ph, spread=True)
    ref.setup()
    ref.run(25)                                # rebuilds at steps 10 and 20
    eng = engine_for(sph_amd, s, ph, kernel_path=path)
    eng.setup()
    eng.run(25)
    assert np.array_equal(eng.neighbor_counts(), ref.numneigh_full())
    compare(eng, ref, path=path)
    assert eng.stats()["step"] == 25


def test_inner_rows_refresh(gpu, sph_amd):
    """Between rebuilds the inner rows (pairs within cut + skin/16 at the time they were
    written) are derived again once an atom has moved past half that margin (refresh_inner,
    a per-step moved flag): with 3x the lattice's velocities and 20 steps per build the
    refresh runs several times; fields stay at 1e-10 and counts exact at every compared step,
    and the passes end on inner rows (inner_live)."""
    s = c2_system(12)
    s.v *= 3.0
    ph = po.c2_physics()
    ph.every = 20
    ref = po.RefRun(s, ph, spread=True)
    ref.setup()
    eng = engine_for(sph_amd, s, ph)
    eng.setup()
    done = 0
    for k in (6, 13, 19, 27):
        ref.run(k - done)
        eng.run(k - done)
        done = k
        assert np.array_equal(eng.neighbor_counts(), ref.numneigh_full()), k
        compare(eng, ref, path=0)
    st = eng.stats()
    assert st["inner_refresh"] > 0, "no refresh: the atoms did not move past the margin"
    assert st["inner_rows"] == 1 and st["inner_live"] == 1


@pytest.mark.parametrize("path", PATHS)
def test_run_c3_morris_heat(gpu, sph_amd, path):
    s = c3_system(10)
    ph = po.c3_physics()
    ph.every = 5
    ref = po.RefRun(s, ph, spread=True)
    ref.setup()
    ref.run(12)
    eng = engine_for(sph_amd, s, ph, kernel_path=path)
    eng.setup()
    eng.run(12)
    assert np.array_equal(eng.neighbor_counts(), ref.numneigh_full())
    compare(eng, ref, path=path)


@pytest.mark.parametrize("path", PATHS)
def test_run_2d(gpu, sph_amd, path):
    s = c2_system(30, dim=2)
    ph = po.c2_physics(2.5)
    ph.every = 4
    ref = po.RefRun(s, ph, spread=True)
    ref.setup()
    ref.run(9)
    eng = engine_for(sph_amd, s, ph, kernel_path=path)
    eng.setup()
    eng.run(9)
    assert np.array_equal(eng.neighbor_counts(), ref.numneigh_full())
    compare(eng, ref, path=path)


@pytest.mark.parametrize("path", PATHS)
def test_every_step_rebuild_and_nstep(gpu, sph_amd, path):
    s = c2_system(9)
    ph = po.c2_physics()
    ph.every = 1
    ph.rhosum_nstep = 3          # rhosum gated on ntimestep % nstep (pair_sph_rhosum.cpp:112)
    ref = po.RefRun(s, ph, spread=True)
    ref.setup()
    ref.run(7)
    eng = engine_for(sph_amd, s, ph, kernel_path=path)
    eng.setup()
    eng.run(7)
    compare(eng, ref, path=path)


@pytest.mark.parametrize("path", PATHS)
def test_nonperiodic_box(gpu, sph_amd, path):
    """No ghosts across non-periodic boundaries (sendneed = 0, comm_brick.cpp:226-274)."""
    s = c2_system(9)
    s.periodic = (1, 0, 1)
    s.boxlo[1] -= 2.0
    s.boxhi[1] += 2.0
    ph = po.c2_physics()
    ref = po.RefRun(s, ph, spread=True)
    ref.setup()
    ref.run(3)
    eng = engine_for(sph_amd, s, ph, kernel_path=path)
    eng.setup()
    eng.run(3)
    assert np.array_equal(eng.neighbor_counts(), ref.numneigh_full())
    compare(eng, ref, path=path)


@pytest.mark.parametrize("path", PATHS)
def test_full_size_properties(gpu, sph_amd, path):
    """BASELINE C2 size (1M particles): size-independent checks -- total neighbor count
    equals the oracle's full_bin count, momentum is conserved by the pair forces
    (sum f = 0 up to roundoff), density is positive and near rho0."""
    s = c2_system(100)
    ph = po.c2_physics()
    eng = engine_for(sph_amd, s, ph, kernel_path=path)
    eng.setup()
    nc = eng.neighbor_counts()
    cns, cmax = po.cutneighsq(1, ph.cutmax(1), ph.skin)
    g = po.borders(s, cmax)
    off = np.zeros(g.nlocal + 1, dtype=np.int64)
    tot = po.lib().orc_neigh_full(3, g.nlocal, g.nall, g.x, g.type, 1, cns, off, None, 0)
    assert int(nc.sum()) == tot
    assert np.array_equal(nc, np.diff(off).astype(np.int32))
    got = eng.get_atoms()
    fsum = np.abs(got["f"].sum(0)).max()
    assert fsum < 1e-9 * np.abs(got["f"]).sum()
    assert (got["rho"] > 0.5).all() and (got["rho"] < 1.5).all()
    eng.run(3)
    got = eng.get_atoms()
    assert np.isfinite(got["x"]).all() and np.isfinite(got["f"]).all()


def test_timing_classes(gpu, sph_amd):
    """sph_engine_set_timing's class mask (bench.py's timed region): only the asked classes
    are timed, the results do not depend on it, and "all" times every class."""
    s = c2_system(12)
    ph = po.c2_physics()
    ref = po.RefRun(s, ph, spread=True)
    ref.setup()
    ref.run(12)
    eng = engine_for(sph_amd, s, ph)
    eng.setup()
    eng.set_timing(True, classes=(eng.T_RHO, eng.T_TAIT))
    eng.run(12)                                # (a rebuild at step 10)
    eng.sync()
    st = eng.stats()
    assert st["n_rhosum"] >= 12 and st["n_tait"] >= 12
    assert st["ms_rhosum"] > 0 and st["ms_tait"] > 0
    assert st["n_neigh"] == 0 and st["ms_neigh"] == 0 and st["ms_integrate"] == 0
    compare(eng, ref, path=0)
    eng.set_timing(True)
    eng.run(2)
    eng.sync()
    st = eng.stats()
    assert st["ms_integrate"] > 0


def test_wide_union_takes_the_row_path(gpu, sph_amd):
    """A block union too large for the rho / inner passes' LDS image (8000 atoms, every pair
    within the cutoff, > 160 KiB at 24 B per slot): the block build reports the overflow and
    the step runs on the row path (before, the rho pass's launch failed once a union passed
    ~6.8k atoms), with parity as everywhere."""
    s = c2_system(20)
    s.periodic = (0, 0, 0)
    s.boxlo = s.boxlo - 2.0
    s.boxhi = s.boxhi + 2.0
    ph = po.c2_physics(40.0)
    ref = po.RefRun(s, ph, spread="lean")
    ref.setup()
    ref.run(1)
    eng = engine_for(sph_amd, s, ph)
    eng.setup()
    eng.run(1)
    assert eng.stats()["staged"] == 0
    assert np.array_equal(eng.neighbor_counts(), ref.numneigh_full())
    compare(eng, ref, path=1)


def test_no_viscosity_c2(gpu, sph_amd):
    """sph/taitwater with nu = 0 (Monaghan viscC = 0): the block pass takes its no-viscosity
    variant (BLK_VISC_NONE) -- before, a 1e300 scale stood in for 1 / viscC, which overflowed
    for large h or rho and left a ~1e-300 term in place of the reference's exact 0."""
    s = c2_system(12)
    ph = po.c2_physics()
    ph.visc = np.zeros_like(ph.visc)
    ref = po.RefRun(s, ph, spread=True)
    ref.setup()
    ref.run(12)
    eng = engine_for(sph_amd, s, ph)
    eng.setup()
    assert eng.stats()["staged"] == 1
    eng.run(12)
    assert np.array_equal(eng.neighbor_counts(), ref.numneigh_full())
    compare(eng, ref, path=0)
