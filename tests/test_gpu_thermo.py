"""sph_engine_virial_every / sph_engine_thermo on the device against the oracle
(thermo_util.py): the pair virial of the due steps on the block path, the row path and the
setup step's CSR pass, for Monaghan, Morris and sph/idealgas; fix gravity's scalar, ke and
press on a small water_collapse; the last step of a run; two bricks; determinism; the fields
of a run that asks for the virial against one that does not; the refused calls.

Bars: every virial component within 1e-10 S_ab (S_ab: the sum of the tallied terms' absolute
values); egrav, ke and ke_tensor within 1e-12 of the sum of their terms' absolute values;
press within the bar of its parts (thermo_util.sums)."""
import math
import threading

import numpy as np
import pytest

import pyoracle as po
from thermo_util import (MVV2E, NKTV2P, STOL, VTOL, dump_parity, engine, make_case,
                         oracle_history, ratio)

pytestmark = pytest.mark.gpu

NSTEPS = 7


@pytest.fixture(scope="module", autouse=True)
def _parity_file():
    yield
    dump_parity()


def raw(a):
    return np.ascontiguousarray(a).view(np.uint8)


def check_virial(tag, th, h):
    r = ratio(f"{tag}:virial", th["virial"] - h["virial"], VTOL * h["vscale"])
    print(f"[thermo] {tag}: virial ratio {r:.3e}")
    assert r <= 1.0, (tag, th["virial"], h["virial"], h["vscale"])


def check_sums(tag, th, want):
    re = ratio(f"{tag}:egrav", th["egrav"] - want["egrav"], STOL * want["egrav_scale"])
    rk = ratio(f"{tag}:ke", th["ke"] - want["ke"], STOL * want["ke"])
    rt = ratio(f"{tag}:ke_tensor", th["ke_tensor"] - want["ke_tensor"],
               STOL * want["ke_tensor_scale"])
    rp = ratio(f"{tag}:press", th["press"] - want["press"], want["press_bar"])
    print(f"[thermo] {tag}: egrav {re:.3e} ke {rk:.3e} ke_tensor {rt:.3e} press {rp:.3e}")
    assert th["volume"] == want["volume"]
    assert max(re, rk, rt, rp) <= 1.0, (tag, th, want)


# ---- a: 3-D periodic, two types with unequal cuts, both paths, both viscosities --------------
@pytest.mark.parametrize("path", [0, 1])
@pytest.mark.parametrize("name", ["monaghan", "morris"])
def test_virial_due_steps(gpu, sph_amd, name, path):
    hist = oracle_history(name, NSTEPS)
    eng = engine(sph_amd, make_case(name), path, virial_every=2)
    eng.setup()
    assert eng.stats()["staged"] == (1 if path == 0 else 0)
    for k in range(NSTEPS + 1):
        if k:
            eng.run(1)
        th = eng.thermo()
        # (run(1): every step is the last of its run, so every step is due)
        assert th["virial_step"] == k
        check_virial(f"a:{name}:path{path}:step{k}", th, hist[k])
        check_sums(f"a:{name}:path{path}:step{k}", th, hist[k]["sums"])
    assert eng.stats()["staged"] == (1 if path == 0 else 0)
    eng.close()


@pytest.mark.parametrize("path", [0, 1])
def test_stale_steps_are_nan(gpu, sph_amd, path):
    """The last step of every run() is due, so an armed engine cannot show a stale virial after
    run() returns (the steps inside a run that are not due are seen in test_fields_unchanged:
    they fuse); an engine that never asked (virial_every 0, the default) has none: virial_step
    -1 and press NaN, the other fields valid"""
    hist = oracle_history("monaghan", NSTEPS)
    eng = engine(sph_amd, make_case("monaghan"), path, virial_every=0)
    eng.setup()
    th = eng.thermo()
    assert th["virial_step"] == -1 and math.isnan(th["press"])       # never asked
    eng.run(1)
    th = eng.thermo()
    assert th["virial_step"] == -1 and math.isnan(th["press"])
    want = hist[1]["sums"]
    assert abs(th["ke"] - want["ke"]) <= STOL * want["ke"]
    eng.close()


# ---- b: the small 2-D water_collapse: egrav, ke, press ---------------------------------------
@pytest.mark.parametrize("path", [0, 1])
def test_dam2d_sums(gpu, sph_amd, path):
    hist = oracle_history("dam2d", 3)
    c = make_case("dam2d")
    assert c.s.dim == 2 and tuple(c.s.periodic)[:2] == (0, 0)
    assert c.ph.gravity_mask == 1 << 1 and c.ph.stationary_mask == 1 << 2
    eng = engine(sph_amd, c, path, virial_every=1)
    eng.setup()
    for k in range(4):
        if k:
            eng.run(1)
        th = eng.thermo()
        assert th["virial_step"] == k
        check_virial(f"b:path{path}:step{k}", th, hist[k])
        check_sums(f"b:path{path}:step{k}", th, hist[k]["sums"])
        assert hist[k]["sums"]["egrav"] != 0.0 and (k == 0 or hist[k]["sums"]["ke"] > 0.0)
        # two non-trivial factors: each applied once
        check_sums(f"b:path{path}:step{k}:factors", eng.thermo(MVV2E, NKTV2P), hist[k]["sums2"])
    eng.close()


# ---- c: sph/idealgas: each pair once ---------------------------------------------------------
@pytest.mark.parametrize("path", [0, 1])
def test_gas_virial_once_per_pair(gpu, sph_amd, path):
    hist = oracle_history("shock", 2)
    eng = engine(sph_amd, make_case("shock"), path, virial_every=1)
    eng.setup()
    for k in range(3):
        if k:
            eng.run(1)
        th = eng.thermo()
        assert th["virial_step"] == k
        check_virial(f"c:path{path}:step{k}", th, hist[k])
        # (a twice-tallied virial is off by the whole value, far outside the bar)
        assert np.abs(hist[k]["virial"][:2]).min() > 1e3 * VTOL * hist[k]["vscale"][:2].max()
    eng.close()


# ---- d: the last step of a run ----------------------------------------------------------------
@pytest.mark.parametrize("path", [0, 1])
def test_last_step_of_run(gpu, sph_amd, path):
    hist = oracle_history("monaghan", NSTEPS)
    eng = engine(sph_amd, make_case("monaghan"), path, virial_every=4)
    eng.setup()
    eng.run(5)
    th = eng.thermo()
    assert th["virial_step"] == 5 and not math.isnan(th["press"])
    check_virial(f"d:path{path}:step5", th, hist[5])
    check_sums(f"d:path{path}:step5", th, hist[5]["sums"])
    eng.close()


def test_stale_inside_cadence(gpu, sph_amd):
    """virial_every 4, run(5), run(1), run(2): thermo names the last step of each run (5 and 6
    as last steps, 8 as both)"""
    eng = engine(sph_amd, make_case("monaghan"), 0, virial_every=4)
    eng.setup()
    seen = []
    for n in (5, 1, 2):
        eng.run(n)
        seen.append(eng.thermo()["virial_step"])
    assert seen == [5, 6, 8]
    eng.close()


# ---- e: two bricks ----------------------------------------------------------------------------
def test_two_bricks_add_up(gpu, sph_amd):
    """the `rest` case (thermo_util.make_case says why): the ranks' sums against the one-brick
    oracle at the setup step and two steps on, where the atoms move"""
    hist = oracle_history("rest", 2)
    c = make_case("rest")
    pg = (2, 1, 1)
    world = sph_amd.LocalWorld(2)
    owner = po.brick_owner(c.s, c.s.x, pg)
    engines = []
    for r in range(2):
        eng = engine(sph_amd, c, 0, virial_every=2, procgrid=pg, rank=r,
                     sel=np.nonzero(owner == r)[0])
        eng.comm_local(world, r)
        engines.append(eng)
    out, errors = [{}, {}], []

    def work(r):
        try:
            engines[r].setup()
            out[r][0] = engines[r].thermo()
            engines[r].run(2)
            out[r][2] = engines[r].thermo()
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
        for k in (0, 2):
            tot = {f: out[0][k][f] + out[1][k][f] for f in ("virial", "ke_tensor", "ke", "egrav")}
            assert out[0][k]["virial_step"] == out[1][k]["virial_step"] == k
            want = hist[k]["sums"]
            check_virial(f"e:step{k}", tot, hist[k])
            assert ratio(f"e:step{k}:ke_tensor", tot["ke_tensor"] - want["ke_tensor"],
                         STOL * want["ke_tensor_scale"]) <= 1.0
            assert ratio(f"e:step{k}:ke", tot["ke"] - want["ke"], STOL * want["ke"]) <= 1.0
            assert (want["ke"] > 0.0) == (k == 2) and want["egrav"] != 0.0
            assert ratio(f"e:step{k}:egrav", tot["egrav"] - want["egrav"],
                         STOL * want["egrav_scale"]) <= 1.0
    finally:
        for e in engines:
            e.close()
        world.close()


# ---- f: determinism ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,path", [("monaghan", 0), ("monaghan", 1), ("morris", 0),
                                       ("shock", 0), ("shock", 1)])
def test_same_bits_twice(gpu, sph_amd, name, path):
    outs = []
    for _ in range(2):
        eng = engine(sph_amd, make_case(name), path, virial_every=2)
        eng.setup()
        o = [eng.thermo()]
        eng.run(3)
        o.append(eng.thermo())
        outs.append(o)
        eng.close()
    for a, b in zip(*outs):
        assert sorted(a) == sorted(b)
        for k in a:
            assert np.array_equal(raw(np.asarray(a[k])), raw(np.asarray(b[k]))), (name, path, k)


# ---- g: the fields do not depend on the virial ------------------------------------------------
@pytest.mark.parametrize("name,path,fuse,every", [
    ("monaghan", 0, None, 1), ("monaghan", 1, None, 1), ("morris", 0, None, 1),
    ("morris", 0, 0, 1), ("morris", 1, None, 1), ("c2", 0, 1, 1),
    # every 3 over run(6): fused steps, a due step, fused steps, the due last step
    ("c2", 0, 1, 3), ("monaghan", 0, 1, 3)])
def test_fields_unchanged(gpu, sph_amd, name, path, fuse, every):
    from scenarios import c2_system
    from thermo_util import Case
    got = []
    for nevery in (every, 0):
        c = (Case("c2", c2_system(12), po.c2_physics()) if name == "c2" else make_case(name))
        eng = engine(sph_amd, c, path, virial_every=nevery)
        if fuse is not None:
            eng.tune(eng.TUNE_FUSEINT, fuse)
        eng.setup()
        eng.run(6)
        st = eng.stats()
        assert st["staged"] == (1 if path == 0 else 0)
        if fuse and nevery == 0:
            assert st["flags"] & eng.STAT_FUSEINT     # the plain run did fuse its steps
        if nevery == 1:
            assert st["flags"] & eng.STAT_FUSEINT == 0  # every step due: none fused
        if fuse and nevery == 3:
            assert st["flags"] & eng.STAT_FUSEINT     # the steps between the due ones fused
            assert eng.thermo()["virial_step"] == 6
        got.append(eng.get_atoms())
        eng.close()
    a, b = got
    assert sorted(a) == sorted(b)
    for k in a:
        assert np.array_equal(raw(np.asarray(a[k])), raw(np.asarray(b[k]))), (name, path, k)


def _bricks_overlap(sph, nevery):
    """the two bricks of case e's split of `monaghan`, halo / compute overlap on: 7 steps"""
    c = make_case("monaghan")
    pg = (2, 1, 1)
    world = sph.LocalWorld(2)
    owner = po.brick_owner(c.s, c.s.x, pg)
    engines = []
    for r in range(2):
        eng = engine(sph, c, 0, virial_every=nevery, procgrid=pg, rank=r,
                     sel=np.nonzero(owner == r)[0])
        eng.comm_local(world, r)
        eng.tune(eng.TUNE_OVERLAP, 1)
        engines.append(eng)
    out, errors = [None, None], []

    def work(r):
        try:
            engines[r].setup()
            engines[r].run(7)
            out[r] = engines[r].get_atoms()
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
        return out
    finally:
        for e in engines:
            e.close()
        world.close()


def test_fields_unchanged_bricks_overlap(gpu, sph_amd):
    """a due step takes the serial pair compute where a plain step of these bricks overlaps the
    halos with the interior rows: the fields are the same bits"""
    a, b = _bricks_overlap(sph_amd, 2), _bricks_overlap(sph_amd, 0)
    for r in range(2):
        assert sorted(a[r]) == sorted(b[r])
        for k in a[r]:
            assert np.array_equal(raw(np.asarray(a[r][k])), raw(np.asarray(b[r][k]))), (r, k)


# ---- h: refused calls -------------------------------------------------------------------------
def test_einval(gpu, sph_amd):
    from c5_util import mp_engine
    from scenarios import bubble_physics, bubble_system
    eng = engine(sph_amd, make_case("monaghan"), 0)
    with pytest.raises(sph_amd.HipError, match="nevery"):
        eng.virial_every(-1)
    with pytest.raises(sph_amd.HipError, match="sph_engine_setup"):
        eng.thermo()
    eng.virial_every(3)
    eng.setup()
    with pytest.raises(sph_amd.HipError, match="before sph_engine_setup"):
        eng.virial_every(2)
    rc = eng.L.sph_engine_thermo(eng.h, 1.0, 1.0, None)
    assert rc != 0
    assert eng.L.sph_engine_virial_every(None, 1) != 0
    eng.close()
    # a multiphase engine: no virial, the kinetic and gravity sums with rmass as the mass
    s = bubble_system(6)
    s.v = np.random.default_rng(5).normal(0.0, 0.01, s.v.shape)
    mp = mp_engine(sph_amd, s, bubble_physics(6, pc=False))
    with pytest.raises(sph_amd.HipError, match="multiphase"):
        mp.virial_every(1)
    mp.setup()
    th = mp.thermo()
    ke = 0.5 * (s.rmass * (s.v * s.v).sum(1)).sum()
    assert th["virial_step"] == -1 and math.isnan(th["press"])
    assert abs(th["ke"] - ke) <= STOL * ke and th["egrav"] == 0.0 and th["volume"] == 1.0
    mp.close()
