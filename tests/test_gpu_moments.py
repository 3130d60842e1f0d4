"""sph_engine_moments / sph_engine_gyration on the device-resident engine against the numpy
reference of tests/moments_util.py, whose docstring derives the bar: every sum within
n 2^-52 fsum|t_i| of the correctly rounded sum of the reference's own per-atom terms (n = the
atoms selected); count, lo and hi exact; a repeated call bit-identical."""
import ctypes
import dataclasses

import numpy as np
import pytest

import pyoracle as po
from c5_util import bricks_step, mp_engine, mp_state
from forcefix_util import wrapped
from moments_util import (CROSS_STEPS, CROSS_VX, check_gyration, check_moments, counted_system,
                          crossing_system, engine_inputs, gyration_terms, moment_terms,
                          restart_records, same_bits, subset, sum_and_bound)
from mp_variants_util import mp_box, mp_physics
from neighcheck_util import single_engine
from pc_engine_util import case as pc_case
from pc_engine_util import pc_engine
from scenarios import c2_system, c3_system

pytestmark = pytest.mark.gpu


def _prd(s):
    return np.asarray(s.boxhi, dtype=np.float64) - np.asarray(s.boxlo, dtype=np.float64)


def _check_all(sph, eng, s, sels, where, inp=None):
    """moments and gyration of every selection against the reference, and the repeat call"""
    inp = inp or engine_inputs(eng, sph)
    prd = _prd(s)
    mom = eng.moments(sels)
    same_bits(mom, eng.moments(sels))
    cm = [m["xcm"] for m in mom]
    gyr = eng.gyration(sels, cm=cm, mass=[m["mass"] for m in mom])
    same_bits(gyr, eng.gyration(sels, cm=cm, mass=[m["mass"] for m in mom]))
    same_bits(gyr, eng.gyration(sels))      # (one brick: its own moments are the group's)
    for k, sel in enumerate(sels):
        sub = check_moments(mom[k], inp, sel, prd, f"{where} sel {k}")
        check_gyration(gyr[k]["sums"], sub, prd, cm[k], f"{where} sel {k}")
        if mom[k]["mass"] > 0:
            assert np.array_equal(mom[k]["xcm"], mom[k]["mx"] / mom[k]["mass"])
            assert gyr[k]["rg"] == np.sqrt(gyr[k]["sums"][0] / mom[k]["mass"])
            assert np.array_equal(gyr[k]["tensor"], gyr[k]["sums"][1:] / mom[k]["mass"])
    return inp, mom, gyr


def _restart_engine(sph, s, images, path=0):
    ph = po.c3_physics()
    eng = single_engine(sph, s, ph, path=path)
    eng.read_restart(restart_records(s, images))
    return eng


# ---- 1. sizes -------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 37, 64, 256 * 2 + 3, 512 * 256 + 77])
def test_small_counts(gpu, sph_amd, n):
    """one atom, under a wave, one wave, three blocks with a tail, and past RED_MAXBLOCKS
    blocks of 256 (the grid stride wraps); images -3 .. 3 drawn per atom and dimension"""
    s = counted_system(n)
    images = np.random.default_rng(n).integers(-3, 4, (n, 3))
    eng = _restart_engine(sph_amd, s, images)
    eng.setup()
    c = 0.5 * s.boxhi
    sels = [dict(), dict(types=[2], region=sph_amd.sphere(c, 0.45 * s.boxhi[0]))]
    inp, mom, _ = _check_all(sph_amd, eng, s, sels, f"n={n}")
    assert np.array_equal(inp["image"], images)      # (the positions were wrapped already)
    assert mom[0]["count"] == n


# ---- 2. images ------------------------------------------------------------------------------
def test_images(gpu, sph_amd):
    """300 atoms whose images are -2, 0 and +3, a different one per dimension and per third of
    the atoms: mx and the gyration follow the unwrapped positions, lo / hi the wrapped ones"""
    full = wrapped(c3_system(7))
    s = dataclasses.replace(full.copy(), **{k: getattr(full, k)[:300].copy()
                                            for k in ("x", "v", "type", "rho", "e", "cv")})
    images = np.zeros((300, 3), dtype=np.int64)
    images[:100] = (-2, 0, 3)
    images[100:200] = (0, 3, -2)
    images[200:] = (3, -2, 0)
    eng = _restart_engine(sph_amd, s, images)
    eng.setup()
    sels = [dict(), dict(types=[1])]
    inp, mom, gyr = _check_all(sph_amd, eng, s, sels, "images")
    assert np.array_equal(inp["image"], images)
    prd = _prd(s)
    assert np.array_equal(mom[0]["lo"], s.x.min(0)) and np.array_equal(mom[0]["hi"], s.x.max(0))
    # a reference that ignores the images is far outside the bound in every dimension
    plain = moment_terms(inp, prd, images=False)["mx"]
    plain_g = gyration_terms(inp, prd, mom[0]["xcm"], images=False)
    for d in range(3):
        want, bound = sum_and_bound(plain[:, d])
        print(f"images: mx[{d}] without images off by {abs(mom[0]['mx'][d] - want):.3e}, "
              f"bound {bound:.3e}")
        assert abs(mom[0]["mx"][d] - want) > 1e6 * bound
    want, bound = sum_and_bound(plain_g[:, 0])
    assert abs(gyr[0]["sums"][0] - want) > 1e6 * bound


# ---- 3. crossing the periodic face ----------------------------------------------------------
def _crossing_engine(sph, path=0, sort=1, freeze=(1,), **kw):
    """freeze: the types under `fix setforce 0 0 0`"""
    s, ph = crossing_system()
    eng = single_engine(sph, s, ph, path=path, every=2, sort=sort, **kw)
    for t in freeze:
        eng.setforce(0.0, 0.0, 0.0, types=[t])
    return s, ph, eng


@pytest.mark.parametrize("path", [0, 1])
@pytest.mark.parametrize("sort", [0, 1])
def test_crossing(gpu, sph_amd, path, sort):
    """the force-free slab (type 1) at constant velocity: a third of it crosses the periodic x
    face in 20 steps with a rebuild every 2; xcm advances by v t, vcm is the velocity.
    The bar of xcm(t) - xcm(0) - v t: every step adds dtv * v to x with one rounding of at most
    2^-53 |x| <= 2^-53 * 17.5 (the stored x stays inside [0, 16 + 1.5]), twenty of them per
    atom and so at most that in the mass-weighted mean; plus the two sums' own bounds over the
    mass; plus the rounding of the unwrapping add, of v t and of the two divisions,
    4 * 2^-53 * 17.5."""
    s, ph, eng = _crossing_engine(sph_amd, path, sort)
    eng.setup()
    sels = [dict(types=[1]), dict()]
    inp0, mom0, _ = _check_all(sph_amd, eng, s, sels, "step 0")
    eng.run(CROSS_STEPS)
    inp, mom, _ = _check_all(sph_amd, eng, s, sels, f"step {CROSS_STEPS}")
    slab = inp["type"] == 1
    first = slab & (s.x[:, 0] >= 12.5)       # the slab at the periodic face
    crossed = inp["image"][first, 0] == 1
    assert first.sum() // 4 < crossed.sum() < first.sum() // 2
    assert not inp["image"][slab & ~first].any()
    assert not inp0["image"][slab].any() and not inp["image"][slab, 1:].any()
    prd = _prd(s)
    bound = 0.0
    for m_, i_ in ((mom0[0], inp0), (mom[0], inp)):
        bound += sum_and_bound(moment_terms(subset(i_, slab), prd)["mx"][:, 0])[1] / m_["mass"]
    bound += (CROSS_STEPS + 4) * 2.0 ** -53 * 17.5
    adv = mom[0]["xcm"] - mom0[0]["xcm"]
    want = np.array([CROSS_VX * (CROSS_STEPS * ph.dt), 0.0, 0.0])
    print(f"crossing: xcm advance {adv!r} want {want!r} bound {bound:.3e}")
    assert np.abs(adv - want).max() <= bound
    vb = sum_and_bound(moment_terms(subset(inp, slab), prd)["mv"][:, 0])[1] / mom[0]["mass"]
    assert abs(mom[0]["vcm"][0] - CROSS_VX) <= vb + 2.0 ** -53 * CROSS_VX
    assert mom[0]["vcm"][1] == 0.0 and mom[0]["vcm"][2] == 0.0
    # lo / hi are those of the stored positions: the slab's x bounds wrap with the atoms
    assert mom[0]["lo"][0] < 1.0 and mom[0]["hi"][0] > 15.0


# ---- 4. empty selections and rejected calls -------------------------------------------------
def test_empty_and_errors(gpu, sph_amd):
    s = counted_system(37)
    eng = single_engine(sph_amd, s, po.c3_physics())
    L = eng.L
    sel1 = (sph_amd.GroupSel * 1)()
    out1 = (sph_amd.MomentsOut * 1)()
    cm1, g1 = np.zeros(3), np.zeros(7)

    def rc_moments(n, sel=sel1, out=out1):
        return L.sph_engine_moments(eng.h, n, ctypes.cast(sel, ctypes.c_void_p),
                                    ctypes.cast(out, ctypes.c_void_p))

    def rc_gyration(n, sel=sel1, cm=cm1, out=g1):
        return L.sph_engine_gyration(eng.h, n, ctypes.cast(sel, ctypes.c_void_p),
                                     None if cm is None else cm.ctypes.data,
                                     None if out is None else out.ctypes.data)

    def rejected(fn, *a, **kw):
        with pytest.raises(sph_amd.HipError) as ei:
            fn(*a, **kw)
        assert ei.value.code == -1

    assert rc_moments(1) == -1 and rc_gyration(1) == -1          # before setup
    rejected(eng.moments, [dict()])
    rejected(eng.gyration, [dict()], cm=[(0, 0, 0)], mass=[1.0])
    eng.setup()
    assert rc_moments(1) == 0 and rc_gyration(1) == 0
    assert rc_moments(0, None, None) == 0 and rc_gyration(0, None, None, None) == 0   # nsel 0
    assert eng.moments([]) == [] and eng.gyration([]) == []
    assert rc_moments(1, None) == -1 and rc_moments(1, sel1, None) == -1      # NULL, nsel > 0
    assert rc_gyration(1, None) == -1 and rc_gyration(1, sel1, None) == -1
    assert rc_gyration(1, sel1, cm1, None) == -1
    assert L.sph_engine_moments(None, 1, None, None) == -1
    assert rc_moments(-1) == -1 and rc_gyration(-1) == -1                     # nsel range
    many = [dict()] * (sph_amd.SPH_MAX_MOMENTS + 1)
    rejected(eng.moments, many)
    rejected(eng.gyration, many, cm=np.zeros((len(many), 3)), mass=np.ones(len(many)))
    bad = sph_amd.sphere((3.5, 3.5, 3.5), 2.0)
    bad.style = 5
    for sel in (dict(region=bad), dict(noregion=bad),                         # unknown style
                dict(region=sph_amd.sphere((3.5, 3.5, 3.5), -0.5))):         # negative radius
        rejected(eng.moments, [dict(), sel])
        rejected(eng.gyration, [dict(), sel], cm=np.zeros((2, 3)), mass=np.ones(2))
    sel1[0].region_mode = 3
    assert rc_moments(1) == -1 and rc_gyration(1) == -1                       # region_mode
    # empty selections beside a full one, and a full set of SPH_MAX_MOMENTS
    far = sph_amd.sphere((100.0, 100.0, 100.0), 0.5)
    sels = [dict(types=[3]), dict(), dict(region=far)] + [dict(types=[1])] * 5
    mom = eng.moments(sels)
    gyr = eng.gyration(sels)
    for k in (0, 2):
        m = mom[k]
        assert m["count"] == 0 and m["mass"] == 0.0 and m["volume"] == 0.0
        assert not m["mx"].any() and not m["mv"].any() and not m["xcm"].any()
        assert np.all(m["lo"] == np.inf) and np.all(m["hi"] == -np.inf)
        assert gyr[k]["rg"] == 0.0 and not gyr[k]["sums"].any()
    _check_all(sph_amd, eng, s, sels, "eight")
    same_bits(mom[3:4], mom[7:8])


# ---- 5. multiphase: rmass, rho, created atoms -----------------------------------------------
def test_multiphase_rmass(gpu, sph_amd):
    """the jittered two-phase box with unequal per-atom rmass after 5 steps; then the smallest
    creating case of pc_engine_util (2-D, 144 atoms) with fix phase_change armed"""
    s, ph = mp_box(dim=3), mp_physics()
    assert np.unique(s.rmass).size > s.n // 2
    eng = mp_engine(sph_amd, s, ph)
    eng.setup()
    eng.run(5)
    sels = [dict(), dict(types=[2]), dict(types=[1], noregion=sph_amd.sphere((3.5, 3.4, 3.6), 1.93))]
    inp, mom, _ = _check_all(sph_amd, eng, s, sels, "mp_box")
    g = mp_state(eng)
    assert np.array_equal(inp["m"], g["rmass"]) and np.array_equal(inp["rho"], g["rho"])
    assert not np.array_equal(g["rho"], s.rho)
    eng.close()
    # fix phase_change armed: the created atoms carry to_type, so the type mask is the group
    s, ph, steps = pc_case("energy-2d")
    eng = pc_engine(sph_amd, s, ph)
    eng.setup()
    eng.run(steps)
    g = mp_state(eng)
    assert g["ninserted"] > 0 and g["x"].shape[0] == s.n + g["ninserted"]
    to = ph.pc["to_type"]
    sels = [dict(types=[to]), dict(types=[ph.pc["from_type"]]), dict()]
    inp, mom, _ = _check_all(sph_amd, eng, s, sels, "energy-2d")
    assert mom[0]["count"] == int((g["type"] == to).sum()) > int((s.type == to).sum())
    assert mom[2]["count"] == g["x"].shape[0]


# ---- 6. two bricks --------------------------------------------------------------------------
def test_bricks(gpu, sph_amd):
    """2x1x1 bricks on the crossing case: type 1 straddles the brick face at x = 8 and the
    periodic face; the ranks' results folded by combine_moments against the reference of the
    one-brick engine's state, the gyration about the combined centre likewise.  Both types
    are force-free here, so positions and velocities are bit for bit the same on one brick and
    on two, and rho (sph/rhosum) differs by the order of its sum alone."""
    s, ph, one = _crossing_engine(sph_amd, freeze=(1, 2))
    one.setup()
    one.run(CROSS_STEPS)
    inp = engine_inputs(one, sph_amd)
    prd = _prd(s)
    pg = (2, 1, 1)
    owner = po.brick_owner(s, s.x, pg)
    world = sph_amd.LocalWorld(2)
    engines = []
    try:
        for r in range(2):
            sel = np.nonzero(owner == r)[0]
            e = single_engine(sph_amd, s, ph, every=2, procgrid=pg, rank=r, sel=sel)
            for t in (1, 2):
                e.setforce(0.0, 0.0, 0.0, types=[t])
            e.comm_local(world, r)
            engines.append(e)
        bricks_step(engines, lambda e: e.setup())
        bricks_step(engines, lambda e: e.run(CROSS_STEPS))
        block = sph_amd.block((-1e20, 1.0, -1e20), (1e20, 7.0, 1e20))
        sels = [dict(types=[1]), dict(types=[1], region=block)]
        per_rank = [e.moments(sels) for e in engines]
        for again, e in zip(per_rank, engines):
            same_bits(again, e.moments(sels))
        with pytest.raises(ValueError):
            engines[0].gyration(sels)
        for k, sel in enumerate(sels):
            assert all(r[k]["count"] > 0 for r in per_rank)      # both ranks hold a share
            tot = sph_amd.combine_moments([r[k] for r in per_rank])
            sub = check_moments(tot, inp, sel, prd, f"bricks sel {k}")
            cm, mass = tot["xcm"], tot["mass"]
            parts = [e.gyration([sel], cm=[cm], mass=[mass])[0]["sums"] for e in engines]
            sums = parts[0] + parts[1]
            # (the fold of the two ranks adds one rounding to each of their sums' bounds)
            check_gyration(sums, sub, prd, cm, f"bricks sel {k}")
            g = sph_amd.gyration_dict(sums, mass)
            assert g["rg"] == np.sqrt(sums[0] / mass)
        # atoms of the group migrated across the brick face and wrapped across the periodic one
        tags = [e.get_atoms()["tag"] for e in engines]
        assert np.intersect1d(tags[1], np.nonzero((owner == 0) & (s.type == 1))[0]).size > 0
        assert np.intersect1d(tags[0], np.nonzero((owner == 1) & (s.type == 1))[0]).size > 0
    finally:
        for e in engines:
            e.close()
        world.close()


# ---- 7. two dimensions ----------------------------------------------------------------------
def test_2d(gpu, sph_amd):
    s = wrapped(c2_system(12, dim=2))
    images = np.random.default_rng(12).integers(-2, 3, (s.n, 3))
    images[:, 2] = 0
    eng = single_engine(sph_amd, s, po.c2_physics())
    eng.read_restart(restart_records(s, images))
    eng.setup()
    eng.run(3)
    sels = [dict(), dict(region=sph_amd.sphere((6.0, 6.0, 0.0), 4.0))]
    inp, mom, gyr = _check_all(sph_amd, eng, s, sels, "2d")
    assert inp["image"][:, :2].any()
    for m, g in zip(mom, gyr):
        assert m["count"] > 0
        assert m["mx"][2] == 0.0 and m["mv"][2] == 0.0 and m["lo"][2] == 0.0 == m["hi"][2]
        assert g["sums"][3] == 0.0 and g["sums"][5] == 0.0 and g["sums"][6] == 0.0
        assert g["sums"][4] != 0.0 and g["sums"][0] == g["sums"][0]
