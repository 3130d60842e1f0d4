"""The VIR instantiations of the force passes that test_gpu_thermo.py does not reach, each
against the oracle's fp64 pair tally (virial_variants_util.py): one type (the NT1 epilogue
scale) on the block path, the row path and the setup step's k_force; the windowed walk
(SPH_TUNE_BLKUMF 64); rows past the register preload (h = 4, NCH = 0); BLK_VISC_NONE; Morris
with one type; M_TAIT | M_HEAT; 2-D with one type; the engine with heat conduction alone,
which has nothing to tally; a due step behind fused steps and a rebuild; 1x2x2 and 2x2x2
bricks.  And per case and pass: an engine that never asked for the virial leaves the same
bytes in every array of get_atoms().

The systems are test_gpu_block_paths.py's (900 to 1728 atoms) with v 30 times theirs, so that
the viscous term is a visible share of fpair.  Every engine is armed with virial_every(1000):
the due steps are the setup step and the last step of each run().

Bars (thermo_util's): every virial component within 1e-10 S_ab, ke / ke_tensor / egrav within
1e-12 of the sum of their terms' absolute values, press within the bar of its parts.  Every
test first asserts its premise on the oracle, and through Engine.stats() that the path it is
about ran; one line per case and step is printed (pytest -s / -rP shows it).
"""
import math
import threading

import numpy as np
import pytest

import pyoracle as po
from test_gpu_block_paths import PRELOAD, flag_names
from thermo_util import STOL, VTOL, dump_parity, engine, ratio
from virial_variants_util import (BLOCK, BRICK_GRIDS, BRICK_STEPS, HEAT_ONLY_CASES, NEVERY,
                                  SPECS, VALUE_CASES, brick_case, brick_history, case_id,
                                  history, make_case, steps_of)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _parity_file():
    yield
    dump_parity()


def raw(a):
    return np.ascontiguousarray(a).view(np.uint8)


def label(name, path, umf):
    return f"{name} {'row' if path else 'block'}" + (f" umf {umf}" if umf else "")


def check_virial(tag, th, h):
    r = ratio(f"vv:{tag}:virial", th["virial"] - h["virial"], VTOL * h["vscale"])
    assert r <= 1.0, (tag, th["virial"], h["virial"], h["vscale"])
    return r


def check_sums(tag, th, want):
    re = ratio(f"vv:{tag}:egrav", th["egrav"] - want["egrav"], STOL * want["egrav_scale"])
    rk = ratio(f"vv:{tag}:ke", th["ke"] - want["ke"], STOL * want["ke"])
    rt = ratio(f"vv:{tag}:ke_tensor", th["ke_tensor"] - want["ke_tensor"],
               STOL * want["ke_tensor_scale"])
    rp = ratio(f"vv:{tag}:press", th["press"] - want["press"], want["press_bar"])
    assert th["volume"] == want["volume"]
    assert max(re, rk, rt, rp) <= 1.0, (tag, dict(egrav=re, ke=rk, ke_tensor=rt, press=rp), th,
                                        want)
    return dict(egrav=re, ke=rk, ke_tensor=rt, press=rp)


def premise(name, c, hist):
    """on the oracle alone: what the case is about is there to be seen"""
    sp, dim = SPECS[name], c.s.dim
    ks = steps_of(c.ph)
    assert c.ph.every + 2 == ks[2] and NEVERY > ks[2]       # one rebuild, two steps behind it
    for k in ks:
        h = hist[k]
        rows = h["nn_max"]
        assert (rows > PRELOAD) if sp.long else (rows <= PRELOAD), (name, k, rows)
        assert h["sums"]["ke"] > 0.0
        assert (h["sums"]["egrav"] != 0.0) == sp.gravity
    if sp.gravity:
        assert len(set(c.ph.gravity)) == 3
    # no atom moves past half the inner rows' margin (skin / 16) behind the build it is read
    # after: steps 1 and every + 2 end on inner rows (test_gpu_block_paths.premise_common)
    assert hist[ks[1]]["moved"] < 0.5 * 0.0625 * c.ph.skin
    assert hist[ks[2]]["moved"] < 0.5 * 0.0625 * c.ph.skin
    if not c.ph.tait:
        return
    for k in ks:
        h = hist[k]
        bar = VTOL * h["vscale"]
        if k == 0 and c.ph.rhosum_nstep == 0 and c.ph.morris:
            # no rhosum: at setup every rho is its type's rho0, the Tait pressure an exact 0,
            # and Morris' viscosity is not part of fpair -- every tallied term is 0, S_ab is 0
            # and so is the bar: the engine's six components must be exact zeros
            assert not np.any(h["vscale"]) and not np.any(h["virial"])
            continue
        # a tally off by a factor, or short of a share of its pairs, is far outside the bar
        assert np.all(np.abs(h["virial"][:dim]) > 1e3 * bar[:dim]), (name, k)
        if dim == 2:  # S_zz = S_xz = S_yz = 0: those components are exact zeros
            assert np.all(h["vscale"][[2, 4, 5]] == 0.0) and np.all(h["virial"][[2, 4, 5]] == 0.0)
        else:
            assert np.all(h["vscale"] > 0.0)
        if sp.monaghan:
            # the Monaghan term changes S_ab by more than 1e3 bars: a tally of the pressure
            # part alone would not pass
            assert np.all(np.abs(h["vscale"] - h["vscale_novisc"])[:dim] > 1e3 * bar[:dim]), \
                (name, k, h["vscale"], h["vscale_novisc"])
    if c.ph.heat and c.s.ntypes == 1:
        assert np.ptp(c.s.e) > 0


def tuned_engine(sph, c, path, umf, nevery, fuse=None):
    eng = engine(sph, c, path, virial_every=nevery)
    if umf:
        eng.tune(eng.TUNE_BLKUMF, umf)
    if fuse is not None:
        eng.tune(eng.TUNE_FUSEINT, fuse)
    return eng


def check_path(eng, st, name, path, umf, k):
    """through Engine.stats(): the pass the case names ran"""
    sp = SPECS[name]
    assert st["step"] == k
    assert st["staged"] == (1 if path == BLOCK else 0)
    if umf:
        assert st["blk_nbig"] > 0
    assert bool(st["flags"] & eng.STAT_BLK_NOPRE) == sp.long
    if path == BLOCK and k > 0:
        assert st["inner_rows"] == 1 and st["inner_live"] == 1


# ---- values: setup (k_force), step 1, the due step behind fused steps and a rebuild ---------
@pytest.mark.parametrize("name,path,umf", VALUE_CASES, ids=map(case_id, VALUE_CASES))
def test_virial_values(gpu, sph_amd, name, path, umf):
    c, hist, sp = make_case(name), history(name), SPECS[name]
    premise(name, c, hist)
    k1, k2 = steps_of(c.ph)[1:]
    fuses = sp.fuses and path == BLOCK
    eng = tuned_engine(sph_amd, c, path, umf, NEVERY)
    try:
        eng.setup()
        for k, nrun in ((0, 0), (k1, 1), (k2, k2 - k1)):
            if nrun:
                eng.run(nrun)
            st, th = eng.stats(), eng.thermo()
            check_path(eng, st, name, path, umf, k)
            if k == k1:  # (a one-step run never fuses)
                assert st["flags"] & eng.STAT_FUSEINT == 0
            if k == k2:  # the steps before the due last one fused, or could not
                assert bool(st["flags"] & eng.STAT_FUSEINT) == fuses
                assert st["nbr_builds"] >= 2
            assert th["virial_step"] == k
            tag = f"{case_id((name, path, umf))}:step{k}"
            rv = check_virial(tag, th, hist[k])
            rs = check_sums(tag, th, hist[k]["sums"])
            print(f"[virial variants] {label(name, path, umf)} step {k} ({sp.inst}): staged "
                  f"{st['staged']} flags {flag_names(eng, st['flags'])}"
                  f"{'|FUSEINT' if st['flags'] & eng.STAT_FUSEINT else ''} nbig "
                  f"{st['blk_nbig']} inner_live {st['inner_live']} ratio virial {rv:.3e} ke "
                  f"{rs['ke']:.3e} ke_tensor {rs['ke_tensor']:.3e} egrav {rs['egrav']:.3e} press "
                  f"{rs['press']:.3e}")
    finally:
        eng.close()


# ---- heat conduction alone: nothing to tally --------------------------------------------------
@pytest.mark.parametrize("name,path,umf", HEAT_ONLY_CASES, ids=map(case_id, HEAT_ONLY_CASES))
def test_heat_only_has_no_virial(gpu, sph_amd, name, path, umf):
    """force_body() is false: a due step launches no VIR pass and virial_fold() writes zeros.
    After setup and after each run virial_step is current, the six components are exactly 0.0
    and press is its kinetic part, within 2 STOL ke / (dim volume)."""
    c, hist = make_case(name), history(name)
    assert not c.ph.tait and c.ph.heat and c.ph.rhosum_nstep == 0
    premise(name, c, hist)
    k1, k2 = steps_of(c.ph)[1:]
    eng = tuned_engine(sph_amd, c, path, umf, NEVERY)
    try:
        eng.setup()
        for k, nrun in ((0, 0), (k1, 1), (k2, k2 - k1)):
            if nrun:
                eng.run(nrun)
            st, th = eng.stats(), eng.thermo()
            check_path(eng, st, name, path, umf, k)
            assert st["flags"] & eng.STAT_FUSEINT == 0
            assert th["virial_step"] == k
            assert th["virial"].shape == (6,)
            assert np.array_equal(raw(th["virial"]), raw(np.zeros(6))), th["virial"]
            want = hist[k]["sums"]
            dim, vol = c.s.dim, want["volume"]
            assert math.isfinite(th["press"])
            kinetic = 2.0 * want["ke"] / (dim * vol)
            assert want["press"] == kinetic      # (nothing tallied: the oracle's press is that)
            assert want["press_bar"] == 2.0 * STOL * want["ke"] / (dim * vol)
            tag = f"{case_id((name, path, umf))}:step{k}"
            rs = check_sums(tag, th, want)
            print(f"[virial variants] {label(name, path, umf)} step {k} ({SPECS[name].inst}): "
                  f"staged {st['staged']} flags {flag_names(eng, st['flags'])} virial "
                  f"{th['virial'].tolist()} ratio ke {rs['ke']:.3e} ke_tensor "
                  f"{rs['ke_tensor']:.3e} press {rs['press']:.3e}")
        got = eng.get_atoms()
        assert np.abs(got["f"]).max() == 0.0 and np.abs(got["de"]).max() > 0.0
    finally:
        eng.close()


# ---- the fields do not depend on the virial ---------------------------------------------------
ALL_CASES = VALUE_CASES + HEAT_ONLY_CASES


@pytest.mark.parametrize("name,path,umf", ALL_CASES, ids=map(case_id, ALL_CASES))
def test_fields_unchanged(gpu, sph_amd, name, path, umf):
    """an engine armed with virial_every and one that never asked, through the same calls, both
    with SPH_TUNE_FUSEINT 0 (fusion is shown not to change bits by test_gpu_fused_integrate.py,
    and the armed engine's due steps would otherwise be the only difference in what fused):
    every array of get_atoms() is the same bytes after setup (k_force<VIR> against k_force),
    after run(1) and after run(every + 1) (the VIR block or row pass against the plain one)"""
    c = make_case(name)
    k1, k2 = steps_of(c.ph)[1:]
    got = []
    for nevery in (NEVERY, None):
        eng = tuned_engine(sph_amd, c, path, umf, nevery, fuse=0)
        try:
            eng.setup()
            out = [eng.get_atoms()]
            for k, nrun in ((k1, 1), (k2, k2 - k1)):
                eng.run(nrun)
                st = eng.stats()
                check_path(eng, st, name, path, umf, k)
                assert st["flags"] & eng.STAT_FUSEINT == 0
                assert eng.thermo()["virial_step"] == (k if nevery else -1)
                out.append(eng.get_atoms())
            got.append(out)
        finally:
            eng.close()
    for k, a, b in zip((0, k1, k2), *got):
        assert sorted(a) == sorted(b)
        for f in a:
            x, y = np.asarray(a[f]), np.asarray(b[f])
            assert x.shape == y.shape and x.dtype == y.dtype, (k, f)
            same = np.array_equal(raw(x), raw(y))
            assert same, (label(name, path, umf), k, f, int((x != y).sum()),
                          float(np.abs(x.astype(np.float64) - y).max()))
    print(f"[virial variants] {label(name, path, umf)} fields: {len(got[0][0])} arrays x 3 "
          f"steps, the same bytes")


# ---- bricks -----------------------------------------------------------------------------------
@pytest.mark.parametrize("pg", list(BRICK_GRIDS), ids=lambda pg: "x".join(map(str, pg)))
def test_bricks_add_up(gpu, sph_amd, pg):
    """c2_system(12), one type, from rest under a gravity vector with three different
    components (virial_variants_util.brick_case), one thread per brick: the ranks' sums against
    the one-brick oracle at the setup step and at step 5, behind the rebuild of step 3"""
    path = BRICK_GRIDS[pg]
    hist, c = brick_history(), brick_case()
    last = hist[BRICK_STEPS]
    # premise: the atoms move, and pairs reach across the brick faces (each tallied half by
    # either brick)
    assert c.ph.every < BRICK_STEPS and last["sums"]["ke"] > 0.0 and hist[0]["sums"]["ke"] == 0.0
    assert last["face_pairs"][pg] > 0 and len(set(c.ph.gravity)) == 3
    P = int(np.prod(pg))
    world = sph_amd.LocalWorld(P)
    owner = po.brick_owner(c.s, c.s.x, pg)
    engines = []
    for r in range(P):
        eng = engine(sph_amd, c, path, virial_every=NEVERY, procgrid=pg, rank=r,
                     sel=np.nonzero(owner == r)[0])
        eng.comm_local(world, r)
        engines.append(eng)
    out, errors = [{} for _ in range(P)], []

    def work(r):
        try:
            engines[r].setup()
            out[r][0] = engines[r].thermo()
            engines[r].run(BRICK_STEPS)
            out[r][BRICK_STEPS] = engines[r].thermo()
        except Exception as ex:  # surfaced below
            errors.append(ex)

    th = [threading.Thread(target=work, args=(r,)) for r in range(P)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=300)
    try:
        assert not any(t.is_alive() for t in th), "brick threads hung"
        assert not errors, errors
        sts = [e.stats() for e in engines]
        assert all(st["staged"] == (1 if path == BLOCK else 0) for st in sts)
        assert all(st["flags"] & e.STAT_FUSEINT == 0 for st, e in zip(sts, engines))
        assert all(st["nbr_builds"] >= 2 for st in sts)
        assert sum(st["nlocal"] for st in sts) == c.s.n
        for k in (0, BRICK_STEPS):
            assert all(o[k]["virial_step"] == k for o in out)
            tot = {f: sum(o[k][f] for o in out) for f in ("virial", "ke_tensor", "ke", "egrav")}
            want = hist[k]["sums"]
            tag = f"bricks{'x'.join(map(str, pg))}:step{k}"
            rv = check_virial(tag, tot, hist[k])
            rt = ratio(f"vv:{tag}:ke_tensor", tot["ke_tensor"] - want["ke_tensor"],
                       STOL * want["ke_tensor_scale"])
            rk = ratio(f"vv:{tag}:ke", tot["ke"] - want["ke"], STOL * want["ke"])
            assert want["egrav"] != 0.0
            re = ratio(f"vv:{tag}:egrav", tot["egrav"] - want["egrav"], STOL * want["egrav_scale"])
            print(f"[virial variants] bricks {pg} {'row' if path else 'block'} step {k}: "
                  f"nlocal {[st['nlocal'] for st in sts]} face pairs {last['face_pairs'][pg]} "
                  f"ratio virial {rv:.3e} ke_tensor {rt:.3e} ke {rk:.3e} egrav {re:.3e}")
            assert max(rt, rk, re) <= 1.0, (tag, rt, rk, re)
    finally:
        for e in engines:
            e.close()
        world.close()
