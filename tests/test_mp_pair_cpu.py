"""The inputs and the numpy reference of test_gpu_mp_pair.py, on the oracle alone: the case
list, mp_pair_util.premises per case (a bad seed shows here, without a GPU), and the numpy
restatement of the five pair terms pinned to the C oracle -- half list with newton on and off,
full list for rhosum and colorgradient -- at 1e-12 normwise."""
import numpy as np
import pytest

import mp_pair_util as mp
import mp_variants_util as mv
from conftest import rel_err

PIN = 1e-12
ALL = list(mp.CASES)


def test_case_list():
    """the table of the module: nine cases, 3-D and 2-D, two and three types, every cut set
    and gamma set of mp_variants_util, both extra heat_fixflag placements"""
    assert len(mp.CASES) == 9
    rows = list(mp.CASES.values())
    assert {r[0] for r in rows} == {2, 3} and {r[1] for r in rows} == {2, 3}
    assert {r[2] for r in rows} == set(mv.CUTS) | {"t3"}
    assert {r[3] for r in rows} == set(mv.GAMMAS)
    assert mp.CASES["diag"][4][:3] == (2, 2, 2) and mp.CASES["ff1"][4][:3] == (1, 2, 1)
    for d in (2, 3):
        assert sum(r[0] == d and r[2] == "t3" for r in rows) == 1
    # three types: cuts differ within each style, one absent pair per half-list style, each
    # another pair, none in rhosum / colorgradient
    for k, v in mp.T3.items():
        pos = [x for x in v if x > 0]
        assert len(set(pos)) == len(pos) and max(pos) == 3.0, k
        assert v.count(0.0) == (1 if k[:-4] in mp.HALF_STYLES else 0), k
    assert len(set(mp.ABSENT3.values())) == 3
    for name in ALL:
        c = mp.case(name)
        assert (c.dim, c.nt) == mp.CASES[name][:2]
        assert c.n == (343 if c.dim == 3 else 144)
        for k, u in c.U.items():   # what coeff() gets: no lower-triangle entry is a real one
            lo = np.tril(np.ones_like(u, dtype=bool), -1)
            lo[:, 0] = False
            assert (u[lo] == (7 if k == "heat_fixflag" else 9.75)).all()
            assert np.array_equal(np.triu(u), np.triu(c.T[k]))
    c = mp.case("3d-3types")
    for st, (a, b) in mp.ABSENT3.items():
        assert c.T[mp.CUT_OF[st]][a, b] == 0 and c.T[mp.CUT_OF[st]][b, a] == 0
    assert c.T["visc"][2, 3] == 0 and c.T["heat_alpha"][3, 3] == 0
    assert mp.case("diag").T["heat_fixflag"][2, 2] == 2
    assert mp.case("ff1").T["heat_fixflag"][1, 2] == 1 == mp.case("ff1").T["heat_fixflag"][2, 1]


@pytest.mark.parametrize("name", ALL)
def test_premises(po, name):
    out = mp.premises(name)
    print(f"[mp pair premises] {name}: n {out['n']} ghosts {out['nghost']} full {out['full']} "
          f"half {out['half']} pinned {out['pinned']} chained {out['chained']} owned-ghost {out['owned_ghost']}")
    print(f"[mp pair premises] {name}: pieces {out['pieces']}")
    print(f"[mp pair premises] {name}: bands {out['bands']} absent {out['absent']}")
    for k, v in out["caps"].items():
        print(f"[mp pair premises] {name} {k}: spread {v['spread']:.1e} wide {v['wide']} "
              f"worst bar {v['worst_bar']:.1e}")
    print(f"[mp pair premises] {name}: ghost slots under the floor {out['ghost_floor']}")


@pytest.mark.parametrize("name", ALL)
def test_numpy_restatement_vs_oracle(po, name):
    """np_style against the C oracle on the oracle's own lists"""
    c = mp.case(name)
    for st in mp.STYLES:
        off, nb = c.lists(st)
        for newton in ((1,) if st in ("rhosum", "cg") else (1, 0)):
            want, _ = c.want(st, newton)
            got = mp.np_style(c, st, off, nb, newton)
            err = rel_err(got, want)
            print(f"[mp pair numpy] {name} {st} newton {newton}: {err:.2e}")
            assert err < PIN, (name, st, newton, err)
            assert np.array_equal(got == 0, want == 0), (name, st, newton)


@pytest.mark.parametrize("name", ["3d-uneq-asym", "diag", "ff1", "2d-uneq-asym"])
def test_gather_differs_from_folded_half_list(po, name):
    """what the FULL-list tests rely on: with gamma[itype] in p_j (asym), or a temperature
    pinned on a same-type pair (diag), the pair term depends on which atom is the row's, so the
    gather over the full list is not the half-list result folded onto its owners;
    surfacetension's is (antisymmetric)"""
    c = mp.case(name)
    for st in mp.HALF_STYLES:
        ga = mp.np_style(c, st, c.foff, c.fnb, gather=True)
        assert not ga[c.n:].any()
        fo = mp.fold(c, c.want(st, 1)[0])
        d = rel_err(ga[:c.n], fo)
        print(f"[mp pair gather] {name} {st}: gather vs folded {d:.2e}")
        # (a flag on an unlike pair names one atom whichever the row is: symmetric; on a
        # same-type pair the second clamp sees the first one's result, and the row decides)
        if st == "st" or (st == "heat" and name != "diag"):
            assert d < PIN, (name, st, d)
        else:
            assert d > 1e-3, (name, st, d)
