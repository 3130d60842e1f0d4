"""sph/idealgas on the GPU: the pair-style layer against the numpy restatement of
PairSPHIdealGas::compute (idealgas_util.np_idealgas: FULL list, HALF list with newton on and
off, the device-built list, the twice-tallied virial), and the device-resident engine against
the oracle run built on it (idealgas_util.gas_oracle; its preconditions are
test_idealgas_cpu.py's).

Bars: the pair layer at 1e-10 normwise, as test_gpu_pair.py; the engine through
conftest.check_fields at 1e-10 normwise and elementwise against the oracle's own spread (two
row reorderings, the one-ulp input); the engine's momentum and energy sums at 1e-10 of the
sums of absolute terms; neighbour counts exact; identical runs identical bits."""
import dataclasses
import math
import threading

import numpy as np
import pytest

import pyoracle as po
from conftest import check_fields, rel_err
from forcefix_util import arm
from idealgas_util import (HOT_GRAVITY, gas_box, gas_config, gas_engine, gas_oracle,
                           ghosted_inputs, hot_box, np_idealgas, shock_tube_case)
from test_gpu_bricks import brick_index, collect

pytestmark = pytest.mark.gpu
TOL = 1e-10
FIELDS = ("f", "drho", "de", "x", "v", "rho", "e")   # (the pass's own outputs first)


# ---- pair layer -----------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[3, 2])
def boxed(request, po):
    s, ph = gas_box(request.param)
    return s, ph, ghosted_inputs(s, ph)


def _ctx(sph, s, ph, d, newton=1, e=True):
    g = d["g"]
    ctx = sph.PairContext(s.dim, s.ntypes, newton)
    ctx.idealgas_coeff(ph.gas_visc, ph.gas_cut, s.mass)
    ctx.atoms(g.nlocal, g.nghost, g.x, g.type, vest=d["vest"], rho=d["rho"],
              e=d["e"] if e else None)
    return ctx


def _want(s, ph, d, newton, off, nb, **kw):
    g = d["g"]
    return np_idealgas(s.dim, g.nlocal, newton, g.x, g.type, d["vest"], d["rho"], d["e"], s.mass,
                       ph.gas_visc, ph.gas_cut, off, nb, **kw)


def _zeros(nall):
    return np.zeros((nall, 3)), np.zeros(nall), np.zeros(nall), np.zeros(6)


def test_pair_full_list(gpu, sph_amd, boxed):
    s, ph, d = boxed
    n, nall = s.n, d["g"].nall
    ctx = _ctx(sph_amd, s, ph, d)
    ctx.list_csr(sph_amd.SPH_LIST_FULL, d["foff"], d["fnb"])
    f, drho, de, vir = _zeros(nall)
    ctx.idealgas(f, drho, de, virial=vir)
    wf, wd, we = _want(s, ph, d, 0, d["foff"], d["fnb"], gather=True)
    assert rel_err(f[:n], wf[:n]) < TOL and rel_err(drho[:n], wd[:n]) < TOL
    assert rel_err(de[:n], we[:n]) < TOL
    assert not f[n:].any() and not drho[n:].any() and not de[n:].any()   # ghosts untouched
    # every row tallies half of each of its pairs, twice.  The half list's newton-on virial
    # is the same sum: an owned-owned pair once with two whole tallies, and of the two images
    # of an owned-ghost pair (the box is periodic: each has both) the one the half list keeps
    wv = _want(s, ph, d, 1, d["hoff"], d["hnb"], virial=True)[3]
    assert rel_err(vir, wv) < TOL
    # accumulated, not overwritten
    ctx.idealgas(f, drho, de)
    assert rel_err(f[:n], 2 * wf[:n]) < TOL


@pytest.mark.parametrize("newton", [1, 0])
def test_pair_half_list(gpu, sph_amd, boxed, newton):
    """the reference's Newton-3 shares, ghosts included under newton_pair, and the virial of
    two ev_tally calls per pair"""
    s, ph, d = boxed
    n, nall = s.n, d["g"].nall
    ctx = _ctx(sph_amd, s, ph, d, newton)
    ctx.list_csr(sph_amd.SPH_LIST_HALF, d["hoff"], d["hnb"])
    f, drho, de, vir = _zeros(nall)
    ctx.idealgas(f, drho, de, virial=vir)
    wf, wd, we, wv = _want(s, ph, d, newton, d["hoff"], d["hnb"], virial=True)
    assert rel_err(f, wf) < TOL and rel_err(drho, wd) < TOL and rel_err(de, we) < TOL
    assert rel_err(vir, wv) < TOL
    assert f[n:].any() == bool(newton)


def test_pair_viscosity_read_by_row_type(gpu, sph_amd, boxed):
    """a viscosity table that differs from its transpose, as LAMMPS holds one whose
    pair_coeff lines set visc[1][2] only: the pair is evaluated with visc[itype][jtype], i the
    row atom.  HALF: one evaluation per pair, so the list takes the atomics path (the reverse
    list's gather would read the transposed entry); FULL: each row its own entry"""
    s, ph, d = boxed
    n, nall = s.n, d["g"].nall
    visc = ph.gas_visc.copy()
    visc[2, 1] = 3.0 * visc[1, 2]
    ph2 = dataclasses.replace(ph, gas_visc=visc)
    ctx = _ctx(sph_amd, s, ph2, d)
    ctx.list_csr(sph_amd.SPH_LIST_HALF, d["hoff"], d["hnb"])
    f, drho, de, vir = _zeros(nall)
    ctx.idealgas(f, drho, de, virial=vir)
    wf, wd, we, wv = _want(s, ph2, d, 1, d["hoff"], d["hnb"], virial=True)
    assert rel_err(f, wf) < TOL and rel_err(drho, wd) < TOL and rel_err(de, we) < TOL
    assert rel_err(vir, wv) < TOL
    # (the transposed reading, and the symmetric table, are far away)
    sf = _want(s, ph, d, 1, d["hoff"], d["hnb"])[0]
    tf = _want(s, dataclasses.replace(ph, gas_visc=visc.T.copy()), d, 1, d["hoff"], d["hnb"])[0]
    assert rel_err(sf, wf) > 1e-4 and rel_err(tf, wf) > 1e-4
    ctx.list_csr(sph_amd.SPH_LIST_FULL, d["foff"], d["fnb"])
    f, drho, de, _ = _zeros(nall)
    ctx.idealgas(f, drho, de)
    wf, wd, we = _want(s, ph2, d, 0, d["foff"], d["fnb"], gather=True)
    assert rel_err(f[:n], wf[:n]) < TOL and rel_err(de[:n], we[:n]) < TOL


def test_pair_device_built_list_and_update(gpu, sph_amd, boxed):
    s, ph, d = boxed
    g, n, nall = d["g"], s.n, d["g"].nall
    ctx = _ctx(sph_amd, s, ph, d)
    ctx.set_timing(True)
    ctx.build_list(sph_amd.SPH_LIST_HALF, np.asarray(d["cns"], dtype=np.float64), key=1)
    assert np.array_equal(ctx.numneigh(n), np.diff(d["hoff"]).astype(np.int32))
    f, drho, de, _ = _zeros(nall)
    ctx.idealgas(f, drho, de)
    wf, wd, we = _want(s, ph, d, 1, d["hoff"], d["hnb"])
    assert rel_err(f, wf) < TOL and rel_err(drho, wd) < TOL and rel_err(de, we) < TOL
    assert ctx.last_kernel_ms() > 0
    # a step between rebuilds: e and rho restaged, the list kept
    d2 = dict(d, e=d["e"] * 1.25, rho=d["rho"] * 0.8)
    ctx.atoms_update(g.x, vest=d2["vest"], rho=d2["rho"], e=d2["e"])
    f, drho, de, _ = _zeros(nall)
    ctx.idealgas(f, drho, de)
    wf2, wd2, we2 = _want(s, ph, d2, 1, d["hoff"], d["hnb"])
    assert rel_err(f, wf2) < TOL and rel_err(de, we2) < TOL and rel_err(f, wf) > 1e-3


def test_pair_needs_e_and_coefficients(gpu, sph_amd, boxed):
    s, ph, d = boxed
    nall = d["g"].nall
    f, drho, de, _ = _zeros(nall)
    ctx = _ctx(sph_amd, s, ph, d, e=False)
    ctx.list_csr(sph_amd.SPH_LIST_FULL, d["foff"], d["fnb"])
    with pytest.raises(sph_amd.HipError) as ei:
        ctx.idealgas(f, drho, de)
    assert ei.value.code == -1 and not f.any()
    ctx2 = sph_amd.PairContext(s.dim, s.ntypes, 1)
    ctx2.atoms(d["g"].nlocal, d["g"].nghost, d["g"].x, d["g"].type, vest=d["vest"], rho=d["rho"],
               e=d["e"])
    ctx2.list_csr(sph_amd.SPH_LIST_FULL, d["foff"], d["fnb"])
    with pytest.raises(sph_amd.HipError) as ei:
        ctx2.idealgas(f, drho, de)
    assert ei.value.code == -1


# ---- engine ---------------------------------------------------------------------------------
def _run_case(sph, s, ph, path=0, fixes=(), steps=20, umf=0):
    ref = gas_oracle(s, ph, fixes)
    ref.setup()
    eng = gas_engine(sph, s, ph, path)
    arm(eng, fixes)
    if umf:
        eng.tune(eng.TUNE_BLKUMF, umf)
    eng.setup()
    check_fields(eng.get_atoms(), ref, FIELDS, TOL, where="setup")
    assert np.array_equal(eng.neighbor_counts(), ref.numneigh_full())
    ref.run(steps)
    eng.run(steps)
    st = eng.stats()
    assert st["step"] == steps and st["staged"] == (1 if path == 0 else 0)
    assert st["nbr_builds"] >= 1 + steps // ph.every
    assert np.array_equal(eng.neighbor_counts(), ref.numneigh_full())
    check_fields(eng.get_atoms(), ref, FIELDS, TOL, where=f"step {steps}")
    assert ref.e_min > 0
    return eng, ref, st


@pytest.mark.parametrize("path", [0, 1])
def test_engine_gas_box_3d(gpu, sph_amd, path):
    s, ph = gas_box(3)
    eng, ref, _ = _run_case(sph_amd, s, ph, path)
    assert np.abs(ref.s.e - s.e).max() > 1e-6


@pytest.mark.parametrize("path", [0, 1])
def test_engine_one_type(gpu, sph_amd, path):
    """NT1: the uniform factors applied once per row"""
    s, ph = gas_box(3, ntypes=1)
    _run_case(sph_amd, s, ph, path)


@pytest.mark.parametrize("path,nstep", [(0, 0), (1, 0), (0, 3), (1, 3)])
def test_engine_rhosum_nstep(gpu, sph_amd, path, nstep):
    """nstep 0: rho integrated from drho, the EOS term refreshed without a rhosum pass; nstep 3:
    refreshed in the steps between two rhosum passes too (e moves every step)"""
    s, ph = gas_box(3, rhosum_nstep=nstep)
    _run_case(sph_amd, s, ph, path)


@pytest.mark.parametrize("path", [0, 1])
def test_engine_gas_box_2d(gpu, sph_amd, path):
    s, ph = gas_box(2)
    _run_case(sph_amd, s, ph, path)


@pytest.mark.parametrize("path,nstep,gravity", [(0, 1, False), (1, 1, False), (0, 3, False),
                                                (1, 3, False), (0, 1, True), (1, 0, True)])
def test_engine_unequal_sound_speeds(gpu, sph_amd, path, nstep, gravity):
    """hot_box: e differs from atom to atom, so c_j differs from c_i by tens of per cent on
    every pair from the setup pass on (the block path's staged c_j, the row path's gathered
    e_j, the setup CSR pass), and the EOS term of a step without rhosum differs from the last
    rhosum step's; with fix gravity on all types"""
    s, ph = hot_box(3, rhosum_nstep=nstep, gravity=gravity)
    c = np.sqrt(0.4 * s.e / s.mass[s.type])
    assert c.max() / c.min() > 1.5
    eng, ref, _ = _run_case(sph_amd, s, ph, path)
    assert (np.abs(ref.f).max() > 0) and (not gravity or ph.gravity == HOT_GRAVITY)


def test_engine_shock_tube_with_setforce(gpu, sph_amd):
    s, ph, fixes = shock_tube_case()
    eng, ref, _ = _run_case(sph_amd, s, ph, 0, fixes, steps=40)
    g = eng.get_atoms()
    assert ref.all_inside
    assert not g["f"][:, 1].any() and not g["f"][:, 2].any()
    assert np.abs(g["v"][:, 0]).max() > 0.05


def test_engine_windowed_walk(gpu, sph_amd):
    """the force image capped at 64 records: every block walks its union in windows, in the
    gas mode's 80-byte image"""
    s, ph = gas_box(3)
    _, _, st = _run_case(sph_amd, s, ph, 0, umf=64)
    assert st["staged"] == 1 and st["blk_nbig"] > 0


def test_engine_bricks(gpu, sph_amd):
    """2x1x1 bricks in a local world, from rest (the reference's setup forces depend on the
    decomposition otherwise: test_gpu_bricks.py)"""
    s, ph = gas_box(3, at_rest=True)
    pg, steps = (2, 1, 1), 20
    ref = gas_oracle(s, ph)
    ref.setup()
    ref.run(steps)
    world = sph_amd.LocalWorld(2)
    owner = brick_index(s.x, s.boxlo, s.boxhi, pg)
    engines = []
    for r in range(2):
        eng = sph_amd.Engine(gas_config(sph_amd, s, ph, 0, procgrid=pg, rank=r))
        eng.idealgas(ph.gas_visc, ph.gas_cut)
        sel = np.nonzero(owner == r)[0]
        eng.set_atoms(s.x[sel], s.v[sel], s.type[sel], s.rho[sel], s.e[sel], s.cv[sel])
        eng.set_tags(sel)
        eng.comm_local(world, r)
        engines.append(eng)
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
        t.join(timeout=120)
    try:
        assert not any(t.is_alive() for t in th), "brick threads hung"
        assert not errors, errors
        out, counts, nloc = collect(engines, s)
        assert min(nloc) > 0 and np.array_equal(counts, ref.numneigh_full())
        check_fields(out, ref, FIELDS, TOL, where="bricks")
    finally:
        for e in engines:
            e.close()
        world.close()


def test_engine_invariants(gpu, sph_amd):
    """momentum and energy of the engine's own output on the periodic box, independent of the
    restatement: |sum f| at setup, and |sum de + sum f . vest| after one step, within 1e-10 of
    the sums of absolute terms.  The energy sum is taken after a step, not at setup: Verlet::
    setup runs borders before FixMeso::setup_pre_force, so the setup pass pairs an owned
    atom's vest = v with its ghosts' vest = 0 and the reference's own setup terms do not
    cancel; from step 1 on ghosts carry their owners' vest.  vest comes from the restart
    records (get_atoms has none)."""
    s, ph = gas_box(3)
    for path in (0, 1):
        eng = gas_engine(sph_amd, s, ph, path)
        eng.setup()
        f = eng.get_atoms()["f"]
        assert np.abs(f).max() > 0
        for k in range(3):
            assert abs(math.fsum(f[:, k])) <= 1e-10 * math.fsum(np.abs(f[:, k]))
        eng.run(1)
        g = eng.get_atoms()
        f, de = g["f"], g["de"]
        vest = po.unpack_restart(eng.write_restart())["vest"]
        assert np.abs(de).max() > 0 and np.abs(vest).max() > 0
        for k in range(3):
            assert abs(math.fsum(f[:, k])) <= 1e-10 * math.fsum(np.abs(f[:, k]))
        work = (f * vest).sum(axis=1)
        scale = math.fsum(np.abs(de)) + math.fsum(np.abs(f * vest).ravel())
        print(f"path {path}: sum de + sum f.vest = {math.fsum(de) + math.fsum(work):.3e}, "
              f"scale {scale:.3e}")
        assert abs(math.fsum(de) + math.fsum(work)) <= 1e-10 * scale


@pytest.mark.parametrize("path", [0, 1])
def test_engine_energy_invariant_at_setup(gpu, sph_amd, path):
    """the setup pass (the CSR kernel with its ghost-vest rule) under the energy invariant:
    |sum de + sum f . vest| <= 1e-10 of the sums of absolute terms AT SETUP, on a state in
    which the ghosts' bordered vest is their owners' -- the restart records of an engine just
    set up (vest = v), read into a fresh engine: borders carry the restored vest, setup_pre_force
    sets the owned atoms' to the same v, and every pair of the setup pass sees vest = v"""
    s, ph = hot_box(3)
    eng = gas_engine(sph_amd, s, ph, path)
    eng.setup()
    rec = eng.write_restart()
    assert np.array_equal(po.unpack_restart(rec)["vest"], s.v)
    eng2 = gas_engine(sph_amd, s, ph, path, atoms=False)
    eng2.read_restart(rec)
    eng2.setup()
    g = eng2.get_atoms()
    f, de, v = g["f"], g["de"], s.v
    assert np.abs(de).max() > 0
    for k in range(3):
        assert abs(math.fsum(f[:, k])) <= 1e-10 * math.fsum(np.abs(f[:, k]))
    work = (f * v).sum(axis=1)
    scale = math.fsum(np.abs(de)) + math.fsum(np.abs(f * v).ravel())
    print(f"path {path}: setup sum de + sum f.vest = {math.fsum(de) + math.fsum(work):.3e}, "
          f"scale {scale:.3e}")
    assert abs(math.fsum(de) + math.fsum(work)) <= 1e-10 * scale
    # ... and the first engine's own setup, ghosts at vest = 0, does not cancel: the two
    # setups differ, which is why the sum above is taken on the restarted one
    f1, de1 = eng.get_atoms()["f"], eng.get_atoms()["de"]
    assert abs(math.fsum(de1) + math.fsum((f1 * v).sum(axis=1))) > 1e-6 * scale


def test_engine_einval(gpu, sph_amd):
    s, ph = gas_box(3)
    H = sph_amd.HipError

    def code(fn):
        with pytest.raises(H) as ei:
            fn()
        return ei.value.code

    eng = gas_engine(sph_amd, s, ph)
    assert code(lambda: eng.idealgas(ph.gas_visc, ph.gas_cut)) == -1        # a second call
    eng.setup()
    eng2 = sph_amd.Engine(gas_config(sph_amd, s, ph))
    eng2.set_atoms(s.x, s.v, s.type, s.rho, s.e, s.cv)
    eng2.setup()
    assert code(lambda: eng2.idealgas(ph.gas_visc, ph.gas_cut)) == -1       # after setup
    bad = ph.gas_cut.copy()
    bad[1, 2] = 0.0
    eng3 = sph_amd.Engine(gas_config(sph_amd, s, ph))
    assert code(lambda: eng3.idealgas(ph.gas_visc, bad)) == -1              # cut <= 0
    bad[1, 2] = -1.0
    assert code(lambda: eng3.idealgas(ph.gas_visc, bad)) == -1
    eng3.idealgas(ph.gas_visc, ph.gas_cut)                                   # (still armable)
    t = dict(rho0=[0, 1, 1], c0=[0, 10, 10], visc=ph.gas_visc, cut=ph.gas_cut)
    eng4 = sph_amd.Engine(gas_config(sph_amd, s, ph, tait=t))
    assert code(lambda: eng4.idealgas(ph.gas_visc, ph.gas_cut)) == -1       # tait_on
    eng5 = sph_amd.Engine(gas_config(sph_amd, s, ph, heat=dict(alpha=ph.gas_visc,
                                                                  cut=ph.gas_cut)))
    assert code(lambda: eng5.idealgas(ph.gas_visc, ph.gas_cut)) == -1       # heat_on
    # no style at all: the engine is created, setup insists on a cut
    s0, ph0 = gas_box(3, rhosum_nstep=0)
    eng6 = sph_amd.Engine(gas_config(sph_amd, s0, ph0))
    eng6.set_atoms(s0.x, s0.v, s0.type, s0.rho, s0.e, s0.cv)
    assert code(eng6.setup) == -1


def test_engine_mp_refuses_gas(gpu, sph_amd):
    from c5_util import mp_engine
    from mp_variants_util import mp_box, mp_physics
    s, ph = mp_box(dim=3), mp_physics()
    eng = mp_engine(sph_amd, s, ph)
    visc = np.full((s.ntypes + 1, s.ntypes + 1), 0.5)
    with pytest.raises(sph_amd.HipError) as ei:
        eng.idealgas(visc, np.full_like(visc, 3.0))
    assert ei.value.code == -1


def test_engine_restart_round_trip(gpu, sph_amd):
    """write at step 10, read into a fresh engine: the same bytes again; at step 20 the
    restarted engine equals the oracle restarted from that state (tests/test_restart.py's
    engine case) and the first engine, run on, the oracle that never stopped"""
    s, ph = hot_box(3)
    ref = gas_oracle(s, ph)
    ref.setup()
    ref.run(20)
    eng = gas_engine(sph_amd, s, ph)
    eng.setup()
    eng.run(10)
    rec = eng.write_restart()
    eng.run(10)
    check_fields(eng.get_atoms(), ref, FIELDS, TOL, where="run on, step 20")
    eng2 = gas_engine(sph_amd, s, ph, atoms=False)
    eng2.read_restart(rec)
    assert np.array_equal(eng2.write_restart(), rec)
    d = po.unpack_restart(rec)
    s2 = s.copy()
    s2.x, s2.v, s2.rho, s2.e = d["x"].copy(), d["v"].copy(), d["rho"].copy(), d["e"].copy()

    def restarted(sysm):
        r = gas_oracle(sysm, ph, shadows=False)
        r.vest = d["vest"].copy()
        return r

    ref2 = restarted(s2)
    for how in po.SPREAD_ORDERS:
        a = restarted(s2)
        a.rev = how
        ref2.alts.append(a)
    ref2.alts.append(restarted(po.ulp_perturbed(s2, planar=True)))
    ref2.setup()
    ref2.run(10)
    eng2.setup()
    eng2.run(10)
    check_fields(eng2.get_atoms(), ref2, FIELDS, TOL, where="restarted, step 20")


def test_engine_identical_runs_identical_bits(gpu, sph_amd):
    s, ph = gas_box(3)
    outs = []
    for _ in range(2):
        eng = gas_engine(sph_amd, s, ph)
        eng.setup()
        eng.run(12)
        eng.pair_passes(2)
        outs.append(eng.get_atoms())
        eng.close()
    for k in FIELDS:
        assert outs[0][k].tobytes() == outs[1][k].tobytes(), k


def test_engine_pair_passes_and_timing(gpu, sph_amd):
    """sph_engine_pair_passes recomputes the same forces from the same state, and the gas pass
    is timed under the taitwater class (set_timing bit 1)"""
    s, ph = gas_box(3, ntypes=1)
    eng = gas_engine(sph_amd, s, ph)
    eng.setup()
    eng.run(3)
    eng.pair_passes(1)
    g0 = eng.get_atoms()
    eng.set_timing(True, classes=[eng.T_TAIT])   # (bit 1: the taitwater class)
    eng.pair_passes(3)
    eng.sync()
    st = eng.stats()
    assert st["n_tait"] == 3 and st["ms_tait"] > 0 and st["n_rhosum"] == 0
    g1 = eng.get_atoms()
    for k in ("f", "drho", "de", "rho"):
        assert g1[k].tobytes() == g0[k].tobytes(), k
