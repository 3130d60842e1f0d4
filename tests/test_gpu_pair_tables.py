"""GPU parity of the pair-style layer with per-pair coefficient tables whose entries all differ
(tables_util: unequal cuts per type pair and per style, pairs a style has no coefficients
for, per-type mass / rho0 / c0 distinct, 3 and 8 types, 3-D and 2-D).  Every other pair-layer
test feeds the `!NT1` kernels tables with equal entries, where a transposed index, another
style's record, a membership test against the largest cutoff or 2 c0[i] for c0[i] + c0[j]
changes no compared number.

Bars are test_gpu_pair's: rhosum 1e-13 normwise and elementwise, forces 1e-10 normwise,
list row lengths bit-exact.  The oracle is pinned to the reference on these tables by
test_oracle_golden.test_oracle_vs_reference_pair_tables.  Each case asserts
tables_util.premises on the oracle before it touches the GPU.
"""
import dataclasses

import numpy as np
import pytest

import pyoracle as po
import tables_util as tu
from conftest import elem_rel_err, rel_err
from scenarios import oracle_forces, prepared
from test_gpu_pair import _ctx

pytestmark = pytest.mark.gpu
TOL = 1e-10

CASES = [("mixed3", 8), ("mixed8", 8), ("mixed3_2d", 30)]
_CACHE = {}


def scene(name, n, morris=False):
    """(system, physics, prepared) of a case; the premises are asserted once per case"""
    if (name, n) not in _CACHE:
        s, ph = tu.case(name, n)
        prem = tu.premises(s, ph)
        P = prepared(s, ph)
        for a in P.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _CACHE[(name, n)] = (s, ph, P, prem)
    s, ph, P, prem = _CACHE[(name, n)]
    return s, dataclasses.replace(ph, morris=morris), P


def _zeros(nall):
    return np.zeros((nall, 3)), np.zeros(nall), np.zeros(nall)


def _check_rhosum(s, ph, P, rho, rows):
    with np.errstate(all="ignore"):              # (skipped types' self terms: h = 0)
        want = po.rhosum(s.dim, P["g"], s.ntypes, s.mass, ph.rhosum_cut, P["foff"], P["fnb"])
    assert rel_err(rho[rows], want[rows]) < 1e-13
    assert elem_rel_err(rho[rows], want[rows]) < 1e-13


@pytest.mark.parametrize("name,n", CASES)
def test_rhosum_full_list(gpu, sph_amd, name, n):
    """sph/rhosum's list under hybrid/overlay holds the rows of the types it has a pair for
    (mixed8: not tables_util.KEEP8's); here with every neighbour of those rows left in, so the
    pairs without coefficients meet the kernel's zero-weight records.  The other rows' rho is
    not touched."""
    s, ph, P = scene(name, n)
    g, nall = P["g"], P["g"].nall
    keep = ph.rho_keep(s.ntypes)[s.type]
    assert keep.any() == (name == "mixed8")
    rows = np.nonzero(~keep)[0].astype(np.int32)
    ctx = _ctx(sph_amd, s, ph, P)
    numneigh = np.diff(P["foff"]).astype(np.int32)
    fr = [P["fnb"][P["foff"][i]:P["foff"][i + 1]] for i in range(s.n)]
    ctx.list_lammps(sph_amd.SPH_LIST_FULL, rows, numneigh, fr)
    rho = ctx.rhosum(np.full(nall, -7.0))
    _check_rhosum(s, ph, P, rho[:s.n], rows)
    assert np.all(rho[:s.n][keep] == -7.0) and np.all(rho[s.n:] == -7.0)
    ctx.close()


@pytest.mark.parametrize("morris", [False, True])
@pytest.mark.parametrize("name,n", CASES)
def test_taitwater_heat_full_list(gpu, sph_amd, name, n, morris):
    """taitwater (Monaghan / Morris) alone, then with heatconduction added, on the FULL list:
    each pair gathered from both sides with its own record; ghost rows exactly zero"""
    s, ph, P = scene(name, n, morris)
    nall = P["g"].nall
    ctx = _ctx(sph_amd, s, ph, P)
    ctx.list_csr(sph_amd.SPH_LIST_FULL, P["foff"], P["fnb"])
    f, drho, de = _zeros(nall)
    ctx.taitwater(f, drho, de)
    wf, wd, we = oracle_forces(s, dataclasses.replace(ph, heat=False), P)
    n_ = s.n
    assert rel_err(f[:n_], wf[:n_]) < TOL
    assert rel_err(drho[:n_], wd[:n_]) < TOL
    assert rel_err(de[:n_], we[:n_]) < TOL
    ctx.heatconduction(de)
    wf, wd, we = oracle_forces(s, ph, P)
    assert np.abs(we[:n_]).max() > 0
    assert rel_err(de[:n_], we[:n_]) < TOL
    assert not f[n_:].any() and not drho[n_:].any() and not de[n_:].any()
    ctx.close()


@pytest.mark.parametrize("newton", [1, 0])
@pytest.mark.parametrize("morris", [False, True])
@pytest.mark.parametrize("name,n", CASES)
def test_half_list_newton(gpu, sph_amd, name, n, morris, newton):
    """HALF list before reverse comm, newton_pair on and off (both on the oracle's
    half_from_full list, as test_gpu_idealgas.test_pair_half_list): off, a ghost j takes no
    share and its pair half the virial (k_force's newton tests)."""
    s, ph, P = scene(name, n, morris)
    g, nall, nt = P["g"], P["g"].nall, s.ntypes
    ctx = _ctx(sph_amd, s, ph, P, newton)
    ctx.list_csr(sph_amd.SPH_LIST_HALF, P["hoff"], P["hnb"])
    f, drho, de = _zeros(nall)
    vir = np.zeros(6)
    ctx.taitwater(f, drho, de, virial=vir)
    wf, wd, we, wv = po.taitwater(s.dim, g, nt, newton, P["vest_all"], P["rho_all"], s.mass,
                                  ph.rho0, ph.c0, ph.visc, ph.tait_cut, P["hoff"], P["hnb"],
                                  morris=morris, virial=True)
    assert rel_err(f, wf) < TOL and rel_err(drho, wd) < TOL and rel_err(de, we) < TOL
    assert rel_err(vir, wv) < TOL
    assert f[s.n:].any() == bool(newton) and drho[s.n:].any() == bool(newton)
    if morris:     # (one heat pass per case is enough: it does not read the viscosity form)
        ctx.close()
        return
    dh = np.zeros(nall)
    ctx.heatconduction(dh)
    wh = po.heatconduction(s.dim, g, nt, newton, P["e_all"], P["rho_all"], s.mass, ph.alpha,
                           ph.heat_cut, P["hoff"], P["hnb"])
    assert rel_err(dh, wh) < TOL
    assert dh[s.n:].any() == bool(newton)
    ctx.close()


@pytest.mark.parametrize("newton", [1, 0])
def test_half_list_newton_atomics_scatter(gpu, sph_amd, newton):
    """k_force's own Newton-3 scatter (atomics onto j, `newton || j < nlocal`).  taitwater,
    morris and heat conduction never take it: their HALF lists go through the reverse half
    list, whose rows end at nlocal without newton (the cases above).  The one configuration
    that scatters is sph/idealgas with a viscosity table that differs from its transpose
    (test_gpu_idealgas.test_pair_viscosity_read_by_row_type, newton on only); here on mixed3
    with rhosum's cuts, newton on and off, against idealgas_util.np_idealgas."""
    from idealgas_util import np_idealgas
    s, ph, P = scene("mixed3", 8)
    g, nall = P["g"], P["g"].nall
    visc = ph.visc.copy()
    visc[2, 1], visc[3, 1], visc[3, 2] = 3.0 * visc[1, 2], 0.5 * visc[1, 3], 0.07
    assert (visc != visc.T).any() and (P["e_all"] > 0).all()
    ctx = sph_amd.PairContext(s.dim, s.ntypes, newton)
    ctx.idealgas_coeff(visc, ph.rhosum_cut, s.mass)
    ctx.atoms(g.nlocal, g.nghost, g.x, g.type, vest=P["vest_all"], rho=P["rho_all"],
              e=P["e_all"])
    ctx.list_csr(sph_amd.SPH_LIST_HALF, P["hoff"], P["hnb"])
    f, drho, de = _zeros(nall)
    vir = np.zeros(6)
    ctx.idealgas(f, drho, de, virial=vir)
    wf, wd, we, wv = np_idealgas(s.dim, g.nlocal, newton, g.x, g.type, P["vest_all"],
                                 P["rho_all"], P["e_all"], s.mass, visc, ph.rhosum_cut,
                                 P["hoff"], P["hnb"], virial=True)
    assert rel_err(f, wf) < TOL and rel_err(drho, wd) < TOL and rel_err(de, we) < TOL
    assert rel_err(vir, wv) < TOL
    assert f[s.n:].any() == bool(newton) and de[s.n:].any() == bool(newton)
    ctx.close()


@pytest.mark.parametrize("morris", [False, True])
@pytest.mark.parametrize("name,n", CASES)
def test_device_built_lists(gpu, sph_amd, name, n, morris):
    """sph_hip_build_list with the per-pair cutneighsq: FULL then HALF, row lengths bit-exact
    against the oracle's lists (a build that tests against the largest cutoff differs on
    every row, tables_util.premises), the styles on them at the bars above.  (The built FULL
    list holds every owned row, so rhosum writes mixed8's skipped type too; under
    hybrid/overlay such rows are not in its list.  They are left out of the comparison.)"""
    s, ph, P = scene(name, n, morris)
    g, nall = P["g"], P["g"].nall
    cns = np.asarray(P["cns"], dtype=np.float64).reshape(s.ntypes + 1, s.ntypes + 1)
    ctx = _ctx(sph_amd, s, ph, P)
    ctx.build_list(sph_amd.SPH_LIST_FULL, cns, key=1)
    assert np.array_equal(ctx.numneigh(s.n), np.diff(P["foff"]).astype(np.int32))
    rho = ctx.rhosum(np.zeros(nall))[:s.n]
    _check_rhosum(s, ph, P, rho, np.nonzero(~ph.rho_keep(s.ntypes)[s.type])[0])
    f, drho, de = _zeros(nall)
    ctx.taitwater(f, drho, de)
    ctx.heatconduction(de)
    wf, wd, we = oracle_forces(s, ph, P)
    for got, want in ((f, wf), (drho, wd), (de, we)):
        assert rel_err(got[:s.n], want[:s.n]) < TOL
        assert not got[s.n:].any()
    ctx.build_list(sph_amd.SPH_LIST_HALF, cns, key=1)
    assert np.array_equal(ctx.numneigh(s.n), np.diff(P["hoff"]).astype(np.int32))
    f, drho, de = _zeros(nall)
    ctx.taitwater(f, drho, de)
    ctx.heatconduction(de)
    wf, wd, we = oracle_forces(s, ph, P, reverse=False)
    assert rel_err(f, wf) < TOL
    assert rel_err(drho, wd) < TOL
    assert rel_err(de, we) < TOL
    ctx.close()


def test_mapped_host_arrays(gpu, sph_amd):
    """the host_arrays path with mixed3: the staging kernels read x / vest / rho / e from
    mapped host memory, rhosum writes rho and taitwater / heat add into f / drho / de, which
    hold nonzero values beforehand"""
    s, ph, P = scene("mixed3", 8)
    g, n, nall = P["g"], s.n, P["g"].nall
    cns = np.asarray(P["cns"], dtype=np.float64)
    x = np.ascontiguousarray(g.x).copy()
    vest, rho, e = (np.ascontiguousarray(P[k]).copy() for k in ("vest_all", "rho_all", "e_all"))
    f, drho, de = np.full((nall, 3), 0.25), np.full(nall, -0.5), np.full(nall, 2.0)
    ctx = sph_amd.PairContext(3, 3, 1)
    ctx.host_arrays(nall, x=x, vest=vest, rho=rho, e=e, f=f, drho=drho, de=de)
    ctx.atoms(g.nlocal, g.nghost, x, g.type, vest=vest, rho=rho, e=e)
    ctx.rhosum_coeff(ph.rhosum_cut, s.mass)
    ctx.taitwater_coeff(ph.rho0, ph.c0, ph.c0 * ph.c0 * ph.rho0 / 7.0, ph.visc, ph.tait_cut,
                        s.mass, morris=ph.morris)
    ctx.heatconduction_coeff(ph.alpha, ph.heat_cut, s.mass)
    ctx.build_list(sph_amd.SPH_LIST_HALF, cns, key=3)
    assert np.array_equal(ctx.numneigh(n), np.diff(P["hoff"]).astype(np.int32))
    ctx.taitwater(f, drho, de)
    ctx.heatconduction(de)
    wf, wd, we = oracle_forces(s, ph, P, reverse=False)
    assert rel_err(f - 0.25, wf) < TOL
    assert rel_err(drho + 0.5, wd) < TOL
    assert rel_err(de - 2.0, we) < TOL
    # rhosum into the mapped rho (owned rows; the ghosts keep what they held)
    ctx.build_list(sph_amd.SPH_LIST_FULL, cns, key=3)
    ctx.rhosum(rho)
    _check_rhosum(s, ph, P, rho[:n], np.arange(n))
    assert np.array_equal(rho[n:], P["rho_all"][n:])
    ctx.host_arrays(0)
    ctx.close()
