"""GPU parity of the pair-style layer's multiphase styles (sph_hip_rhosum_multiphase,
_colorgradient, _taitwater_multiphase, _heatconduction_phasechange, _surfacetension: k_mp_rhosum,
k_mp_colorgradient, k_mp_half<STYLE, REV>, sph_hip_ctx::build_rev) beyond the one 3-D two-type
configuration of test_gpu_multiphase.py: mp_pair_util's nine cases (2-D, three types, per-pair
and per-style cuts with absent pairs, every gamma set, heat_fixflag on a same-type pair and
naming the lower type), newton_pair on and off, the FULL-list gather of the two asymmetric
styles against the numpy restatement, skip lists through list_lammps, accumulation into
pre-filled arrays, one context over many calls, and the argument errors that launch nothing.

Bars are mp_pair_util's: 1e-10 normwise (rhosum 1e-13), per element max(1e-10 |b_i|,
SPREAD_K s_i) with the oracle's reordering spread, exact zeros where the oracle holds zeros.
Every case asserts mp_pair_util.premises on the oracle before it touches the GPU."""
import numpy as np
import pytest

import mp_pair_util as mp
import tables_util as tu
from conftest import elem_ratio, record_parity, rel_err

pytestmark = pytest.mark.gpu
ALL = list(mp.CASES)
EINVAL = -1   # SPH_HIP_EINVAL (include/sph_hip.h)
_PREM = {}


def scene(name):
    if name not in _PREM:
        _PREM[name] = mp.premises(name)
    return mp.case(name)


def soft(missed, *args, **kw):
    """mp.check, a miss kept for the end of the test (every style and list is looked at)"""
    try:
        mp.check(*args, **kw)
    except AssertionError as err:
        missed.append(err.args[0] if err.args else str(err))


def _kind(sph_amd, style):
    return sph_amd.SPH_LIST_FULL if style in ("rhosum", "cg") else sph_amd.SPH_LIST_HALF


def all_styles(sph_amd, ctx, c, fill=None):
    """the five styles on the case's own lists (full, then half) -> {style: array}"""
    out = {}
    for st in mp.STYLES:
        if st in ("rhosum", "tait"):
            mp.stage_list(ctx, sph_amd, c, st)
        out[st] = mp.run(ctx, c, st, mp.blank(c, st, fill))
    return out


@pytest.mark.parametrize("newton", [1, 0])
@pytest.mark.parametrize("name", ALL)
def test_parity(gpu, sph_amd, name, newton):
    """all five styles against the C oracle: rhosum and colorgradient on the full list (ghost
    slots untouched), the three half-list styles on the half list, ghost slots compared; every
    style called twice returns the same bits (no atomics on this path).

    With newton on the ghost slots that hold one or two pairs next to the cutoff are sums
    without reordering spread: their bar is 1e-10 |b_i| alone, which the kernels' quintic meets
    only while its powers are the reference's to the last bit."""
    c = scene(name)
    ctx = mp.context(sph_amd, c, newton)
    got = all_styles(sph_amd, ctx, c)
    again = all_styles(sph_amd, ctx, c)
    ctx.close()
    missed = []
    for st in mp.STYLES:
        assert np.array_equal(got[st], again[st]), (name, st, "second call differs")
        if st in ("rhosum", "cg"):
            assert not got[st][c.n:].any(), (name, st, "ghost slots written")
        soft(missed, got[st], c, st, newton, (name, newton))
    assert not missed, missed


@pytest.mark.parametrize("name", ["3d-uneq-asym", "diag", "2d-uneq-asym"])
def test_full_list_gather(gpu, sph_amd, name):
    """taitwater/multiphase, heatconduction/phasechange and surfacetension on the FULL list:
    every owned row gathers its pairs with itself as i (p_j's gamma[itype], the chained clamps
    of a same-type pin), against the numpy restatement, which the oracle pins
    (test_mp_pair_cpu); f and de are added into, ghost slots keep the caller's values.  It is not the half-list result
    folded onto its owners where the pair term is asymmetric, and is where it is not."""
    c = scene(name)
    ctx = mp.context(sph_amd, c, 1)
    ctx.list_csr(sph_amd.SPH_LIST_FULL, c.foff, c.fnb)
    for st in mp.HALF_STYLES:
        want, sp = mp.want_on(c, st, c.foff, c.fnb,
                              fn=lambda c_, s_, o_, n_, nw: mp.np_style(c_, s_, o_, n_, gather=True))
        assert not want[c.n:].any()
        zero = mp.run(ctx, c, st, mp.blank(c, st))
        assert not zero[c.n:].any(), (name, st, "ghost slots written")
        a, b = zero[:c.n], want[:c.n]
        record_parity(st + "_gather", a, b, sp[:c.n], mp.TOL)
        if c.dim == 2 and a.ndim == 2:
            assert not a[:, 2].any()
        print(f"[mp pair gather] {name} {st}: normwise {rel_err(a, b):.2e}")
        assert rel_err(a, b) < mp.TOL, (name, st, rel_err(a, b))
        assert elem_ratio(a, b, sp[:c.n], tol=mp.TOL) <= 1.0, (name, st)
        # every slot pre-filled with values of the result's size: owned rows come back as
        # prefill + result to the bit, ghost slots as they were
        pre = mp.blank(c, st, float(np.abs(want).max()), seed=5)
        assert (pre != 0).all()
        out = mp.run(ctx, c, st, pre.copy())
        assert np.array_equal(out[:c.n], pre[:c.n] + zero[:c.n]), (name, st, "not prefill + result")
        assert np.array_equal(out[c.n:], pre[c.n:]), (name, st, "ghost slots touched")
        d = rel_err(a, mp.fold(c, c.want(st, 1)[0]))
        if st == "st" or (st == "heat" and name != "diag"):
            assert d < mp.TOL, (name, st, d)
        else:
            assert d > 1e-3, (name, st, d)
    ctx.close()


def test_2d_colorgradient_leaves_z_out(gpu, sph_amd):
    """2-D atoms that carry a z coordinate (the pair layer takes any x): the reference adds
    nothing to the colour gradient's z in 2-D (pair_sph_colorgradient.cpp:176-180) although
    e_z is not zero then, and rsq holds dz^2.  On the lattice's own z = 0 a gz that is
    accumulated stays zero and nothing shows."""
    c = mp.with_z(scene("2d-uneq-asym"))
    ref = mp.want_on(c, "cg", c.foff, c.fnb)
    P = mp._Pairs(c, c.foff, c.fnb, c.T["cg_cut"])
    assert (np.abs(P.d[:, 2]) > 0.01).sum() > 1000 and not ref[0][:, 2].any()
    assert (ref[0][:c.n, :2] != 0).all()
    ctx = mp.context(sph_amd, c, 1)
    ctx.list_csr(sph_amd.SPH_LIST_FULL, c.foff, c.fnb)
    out = mp.run(ctx, c, "cg", mp.blank(c, "cg"))
    ctx.close()
    assert not out[:, 2].any(), np.abs(out[:, 2]).max()
    mp.check(out, c, "cg", 1, "2d-z", ref=ref)


def _lammps_rows(c, off, nb):
    off = np.asarray(off, dtype=np.int64)
    return np.diff(off).astype(np.int32), [nb[off[i]:off[i + 1]] for i in range(c.n)]


@pytest.mark.parametrize("newton", [1, 0])
def test_skip_list_one_type(gpu, sph_amd, newton):
    """list_lammps with inum < nlocal and a shuffled ilist: the rows of type 2, and ten rows of
    type 1 that are listed but hold no entry.  The oracle gets the same list with every other
    row empty.  rho / cg of the rows that are not listed keep the caller's values; a listed
    row without entries gets rhosum's self term and a zero colour gradient."""
    c = scene("3d-uneq-asym")
    t = c.type[:c.n]
    bare = np.nonzero(t == 1)[0][3:33:3]
    rows = np.concatenate([np.nonzero(t == 2)[0], bare]).astype(np.int32)
    np.random.default_rng(11).shuffle(rows)
    assert 0 < rows.size < c.n and (np.diff(rows) < 0).any() and bare.size == 10
    keep = t == 2
    listed = np.zeros(c.n, dtype=bool)
    listed[rows] = True
    ctx = mp.context(sph_amd, c, newton)
    missed = []
    for st in mp.STYLES:
        off, nb = mp.emptied(*c.lists(st), keep)
        ref = mp.want_on(c, st, off, nb, newton)
        numneigh, fr = _lammps_rows(c, *c.lists(st))
        numneigh[~keep] = 0
        ctx.list_lammps(_kind(sph_amd, st), rows, numneigh, fr)
        if st in ("rhosum", "cg"):
            out = mp.blank(c, st, 1.0, seed=3)
            pre = out.copy()
            mp.run(ctx, c, st, out)
            soft(missed, out, c, st, newton, ("skip", newton), rows=rows, ref=ref)
            assert np.array_equal(out[:c.n][~listed], pre[:c.n][~listed]), (st, "unlisted rows")
            assert np.array_equal(out[c.n:], pre[c.n:]), (st, "ghost slots")
            if st == "cg":
                assert not out[bare].any()
            else:
                assert (out[bare] > 0).all()
        else:
            out = mp.run(ctx, c, st, mp.blank(c, st))
            soft(missed, out, c, st, newton, ("skip", newton), ref=ref)
            assert out[:c.n][~listed].any()       # (unlisted rows still take their j share)
    ctx.close()
    assert not missed, missed


@pytest.mark.parametrize("name", ["3d-3types", "2d-3types"])
def test_skip_list_style_lists(gpu, sph_amd, name):
    """hybrid/overlay's per-style lists (tables_util.style_list) of the three-type cases: the
    pairs a style has no coefficients for are not in its list.  Same result as the oracle's on
    that list -- and, those pairs carrying nothing, as on the whole list."""
    c = scene(name)
    ctx = mp.context(sph_amd, c, 1)
    missed = []
    for st in mp.HALF_STYLES:
        off, nb = tu.style_list(c.g, c.hoff, c.hnb[:c.hoff[-1]], c.T[mp.CUT_OF[st]])
        assert off[-1] < c.hoff[-1]
        numneigh, fr = _lammps_rows(c, off, nb)
        ctx.list_lammps(sph_amd.SPH_LIST_HALF, np.arange(c.n, dtype=np.int32), numneigh, fr)
        out = mp.run(ctx, c, st, mp.blank(c, st))
        soft(missed, out, c, st, 1, (name, "style_list"), ref=mp.want_on(c, st, off, nb, 1))
        soft(missed, out, c, st, 1, (name, "style_list/whole"))
    ctx.close()
    assert not missed, missed


@pytest.mark.parametrize("newton", [1, 0])
def test_accumulation(gpu, sph_amd, newton):
    """every output array pre-filled with seeded nonzero values of the result's own size: f
    and de come back as prefill + what a zeroed array receives, to the bit, and within the bar
    of the oracle; rho / cg are overwritten on the owned rows and nothing else is touched"""
    c = scene("3d-3types")
    ctx = mp.context(sph_amd, c, newton)
    zero = all_styles(sph_amd, ctx, c)
    fill = {st: float(np.abs(c.want(st, newton)[0]).max()) for st in mp.STYLES}
    for st in mp.STYLES:
        mp.stage_list(ctx, sph_amd, c, st)
        pre = mp.blank(c, st, fill[st], seed=21)
        assert (pre != 0).all()
        out = mp.run(ctx, c, st, pre.copy())
        if st in ("rhosum", "cg"):
            assert np.array_equal(out[:c.n], zero[st][:c.n]), (st, "owned rows not overwritten")
            assert np.array_equal(out[c.n:], pre[c.n:]), (st, "ghost slots touched")
        else:
            assert np.array_equal(out, pre + zero[st]), (st, "not prefill + result")
            assert rel_err(out - pre, c.want(st, newton)[0]) < mp.TOL
            if not newton:
                assert np.array_equal(out[c.n:], pre[c.n:]), (st, "ghost slots with newton off")
    ctx.close()


@pytest.mark.parametrize("newton", [1, 0])
def test_one_context_many_calls(gpu, sph_amd, newton):
    """case A, then B (other atom and ghost counts, lists and every coefficient table), then A
    again on one context; the half list, the full list, another half list, the first again:
    every result is bit-identical to a fresh context's"""
    A, B = scene("3d-uneq-asym"), mp.case("3d-uneq2-pow", drop=43)
    assert (A.n, A.g.nghost) != (B.n, B.g.nghost) and A.n != B.n and A.g.nghost != B.g.nghost
    fresh = {}
    for k, c in (("A", A), ("B", B)):
        ctx = mp.context(sph_amd, c, newton)
        fresh[k] = all_styles(sph_amd, ctx, c)
        ctx.close()
    missed = []
    for st in mp.STYLES:     # (B's results are results: within the bar of the oracle)
        soft(missed, fresh["B"][st], B, st, newton, ("B", newton))
    ctx = mp.context(sph_amd, A, newton)
    for k, c in (("A", A), ("B", B), ("A", A)):
        mp.stage_atoms(ctx, c)
        mp.set_coeffs(ctx, c)
        got = all_styles(sph_amd, ctx, c)
        for st in mp.STYLES:
            assert np.array_equal(got[st], fresh[k][st]), (k, st, "differs from a fresh context")
    # half -> full -> a shorter half list -> the first half list, atoms and tables unchanged
    keep = A.type[:A.n] == 2
    soff, snb = mp.emptied(A.hoff, A.hnb, keep)
    f2 = sph_amd.PairContext(A.dim, A.nt, newton)
    mp.stage_atoms(f2, A)
    mp.set_coeffs(f2, A)
    want_full, want_short = {}, {}
    f2.list_csr(sph_amd.SPH_LIST_FULL, A.foff, A.fnb)
    for st in mp.HALF_STYLES:
        want_full[st] = mp.run(f2, A, st, mp.blank(A, st))
    f2.close()
    f3 = mp.context(sph_amd, A, newton)
    f3.list_csr(sph_amd.SPH_LIST_HALF, soff, snb)
    for st in mp.HALF_STYLES:
        want_short[st] = mp.run(f3, A, st, mp.blank(A, st))
        soft(missed, want_short[st], A, st, newton, ("short", newton),
             ref=mp.want_on(A, st, soff, snb, newton))
    f3.close()
    for kind, off, nb, want in ((sph_amd.SPH_LIST_FULL, A.foff, A.fnb, want_full),
                                (sph_amd.SPH_LIST_HALF, soff, snb, want_short),
                                (sph_amd.SPH_LIST_HALF, A.hoff, A.hnb, fresh["A"])):
        ctx.list_csr(kind, off, nb)
        for st in mp.HALF_STYLES:
            out = mp.run(ctx, A, st, mp.blank(A, st))
            assert np.array_equal(out, want[st]), (st, "after a list change")
    ctx.close()
    assert not missed, missed


def test_rejected_coefficients_leave_tables(gpu, sph_amd):
    """a taitwater/multiphase coeff call that is refused (gamma = 0 for the last type) changes
    no table: the next call, after another style's coefficients were set again and the tables
    uploaded, returns the same bits"""
    c = scene("3d-3types")
    ctx = mp.context(sph_amd, c, 1)
    mp.stage_list(ctx, sph_amd, c, "tait")
    before = mp.run(ctx, c, "tait", mp.blank(c, "tait"))
    bad = c.gamma.copy()
    bad[c.nt] = 0.0
    with pytest.raises(sph_amd.HipError, match="type 3: gamma and rho0 must be non-zero") as ei:
        ctx.taitwater_multiphase_coeff(2.0 * c.rho0, c.c0, bad, c.rbg, c.U["visc"], c.U["tait_cut"])
    assert ei.value.code == EINVAL
    ctx.surfacetension_coeff(c.U["st_cut"])
    after = mp.run(ctx, c, "tait", mp.blank(c, "tait"))
    assert np.array_equal(before, after)
    ctx.close()


def test_argument_errors(gpu, sph_amd):
    """SPH_HIP_EINVAL with its message, before anything is launched: a style before its
    coefficients, before a list, before atoms_multiphase; rmass <= 0 (after which the atoms
    count as not staged); gamma or rho0 of 0"""
    c = scene("3d-eq")
    E = sph_amd.HipError
    calls = {"rhosum": "sph_hip_rhosum_multiphase", "cg": "sph_hip_colorgradient",
             "tait": "sph_hip_taitwater_multiphase", "st": "sph_hip_surfacetension",
             "heat": "sph_hip_heatconduction_phasechange"}

    def refused(ctx, st, msg):
        out = mp.blank(c, st, 1.0, seed=9)
        pre = out.copy()
        with pytest.raises(E, match=msg) as ei:
            mp.run(ctx, c, st, out)
        assert ei.value.code == EINVAL and calls[st] + ":" in str(ei.value)
        assert np.array_equal(out, pre)

    ctx = sph_amd.PairContext(c.dim, c.nt, 1)
    mp.stage_atoms(ctx, c)
    ctx.list_csr(sph_amd.SPH_LIST_HALF, c.hoff, c.hnb)
    for st in mp.STYLES:
        refused(ctx, st, "coefficients not set")
    ctx.close()
    ctx = sph_amd.PairContext(c.dim, c.nt, 1)
    mp.stage_atoms(ctx, c)
    mp.set_coeffs(ctx, c)
    for st in mp.STYLES:
        refused(ctx, st, "no neighbor list staged")
    ctx.close()
    ctx = sph_amd.PairContext(c.dim, c.nt, 1)
    ctx.atoms(c.n, c.g.nghost, c.x, c.type, vest=c.v_all, rho=c.rho_all, e=c.e_all)
    mp.set_coeffs(ctx, c)
    ctx.list_csr(sph_amd.SPH_LIST_HALF, c.hoff, c.hnb)
    for st in mp.STYLES:
        refused(ctx, st, "per-atom rmass/cv not staged")
    for bad in (0.0, -1.0):
        rm = c.rm_all.copy()
        rm[c.n + 2] = bad
        with pytest.raises(E, match=f"atom {c.n + 2} has rmass {bad:g} <= 0") as ei:
            ctx.atoms_multiphase(rm, c.cv_all)
        assert ei.value.code == EINVAL
        for st in mp.STYLES:   # (nothing was staged by the refused call)
            refused(ctx, st, "per-atom rmass/cv not staged")
    ctx.close()
    ctx = sph_amd.PairContext(c.dim, c.nt, 1)
    for k, t in (("gamma", 1), ("gamma", 2), ("rho0", 1), ("rho0", 2)):
        v = dict(gamma=c.gamma.copy(), rho0=c.rho0.copy())
        v[k][t] = 0.0
        with pytest.raises(E, match=f"type {t}: gamma and rho0 must be non-zero") as ei:
            ctx.taitwater_multiphase_coeff(v["rho0"], c.c0, v["gamma"], c.rbg, c.U["visc"],
                                           c.U["tait_cut"])
        assert ei.value.code == EINVAL
    mp.stage_atoms(ctx, c)
    ctx.list_csr(sph_amd.SPH_LIST_HALF, c.hoff, c.hnb)
    refused(ctx, "tait", "coefficients not set")
    ctx.close()
