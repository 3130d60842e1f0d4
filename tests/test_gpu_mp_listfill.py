"""The multiphase engine's list build (sph_engine::list_q, launch_neigh3) where the other
multiphase tests do not take it: a rebuild in a step whose rhosum/multiphase is NOT due, so the
fill pass runs without the fused rhosum (k_neigh3 <FILL, RHO = false, TP>), and an engine with
ONE type (NT1 with packed types: the count pass, the fill with the fused rhosum and the fill
without).  Elsewhere rhosum is due at every rebuild (nstep 1, or nstep 2 with rebuilds every 2)
and there are two or three types.

rhosum every 3 steps, rebuilds every 2: step 0 builds with the fused rhosum, step 2 rebuilds
without any rhosum, step 3 sums it in k_mp2_rhosum on the list of step 2.  The boxes, the bar
(mp_variants_util: 1e-10 normwise and per element, the oracle's reordering spread only, exact
zeros) and the path flags are those of test_gpu_mp_variants; with one type the colour gradient
and with it the surface tension are exactly zero in the oracle, and must be here."""
import functools

import numpy as np
import pytest

from c5_util import mp_engine, mp_state
from mp_variants_util import FIELDS, check_fields_strict, mp_box, mp_physics, oracle_caps, oracle_run

import pyoracle as po

AT = (0, 2, 3)


def one_type():
    s = mp_box()
    s.type = np.ones_like(s.type)
    s.ntypes = 1
    s.mass = np.array([0.0, 1.0])

    def tab(c):
        t = np.zeros((2, 2))
        t[1, 1] = c
        return t

    ph = po.MpPhysics(skin=0.3, dt=2e-3, every=2, rhosum_nstep=3, rhosum_cut=tab(3.0), cg_nstep=1,
                      cg_alpha=tab(0.0), cg_cut=tab(3.0), tait=True, rho0=np.array([0.0, 1.0]),
                      c0=np.array([0.0, 10.0]), gamma=np.array([0.0, 1.0]),
                      rbg=np.array([0.0, 0.5]), visc=tab(0.05), tait_cut=tab(3.0), st=True,
                      st_cut=tab(3.0), heat=True, heat_alpha=tab(0.2), heat_cut=tab(3.0),
                      heat_fixflag=np.zeros((2, 2), dtype=np.int32), heat_tc=tab(0.0), pc=None)
    return s, ph


@functools.lru_cache(maxsize=None)
def case(name):
    s, ph = one_type() if name == "one_type" else (mp_box(), mp_physics(rhosum_nstep=3))
    return s, ph, oracle_run(s, ph, AT)


NAMES = ("one_type", "two_types")


@pytest.mark.parametrize("name", NAMES)
def test_oracle_caps(po, name):
    """the premises, on the oracle alone: the types, rhosum's schedule against the rebuilds',
    and inputs that keep the strict bar meaningful"""
    s, ph, snaps = case(name)
    assert s.n == 343 and sorted(set(s.type.tolist())) == ([1] if name == "one_type" else [1, 2])
    assert ph.rhosum_nstep == 3 and ph.every == 2 and ph.skin == 0.3
    # rho stands still over the rebuild of step 2 and moves at step 3
    assert not np.array_equal(snaps[2].field("rho"), snaps[3].field("rho"))
    assert not np.array_equal(snaps[0].counts, snaps[2].counts)
    for step, sn in snaps.items():
        oracle_caps(sn, FIELDS, (name, step))
        assert sn.field("f").any() and sn.field("de").any()
        assert sn.field("cg").any() == (name == "two_types")


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_mp_listfill(gpu, sph_amd, name):
    s, ph, snaps = case(name)
    eng = mp_engine(sph_amd, s, ph)
    try:
        for step in range(max(snaps) + 1):
            if step == 0:
                eng.setup()
            else:
                eng.run(1)
            fl = eng.stats()["flags"]
            # W4: symmetric styles, every gamma 1; rhosum inside the list fill at step 0 only
            assert fl & eng.STAT_MP_W4 and not fl & (eng.STAT_MP_POW | eng.STAT_MP_ROW)
            assert bool(fl & eng.STAT_RHO_FUSED) == (step == 0), (name, step, hex(fl))
            assert bool(fl & eng.STAT_MP_RHO_LISTFILL) == (step < 3), (name, step, hex(fl))
            if step not in snaps:
                continue
            sn = snaps[step]
            g = mp_state(eng)
            assert g["x"].shape[0] == sn.n and np.array_equal(g["type"], sn.type)
            assert np.array_equal(eng.neighbor_counts(), sn.counts), (name, step)
            check_fields_strict(g, sn, FIELDS, (name, step))
    finally:
        eng.close()
