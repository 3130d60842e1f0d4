"""CPU side of sph/idealgas: the C ABI declares and exports it, the ctypes mirror of
sph_engine_gas matches the header, the numpy restatement of PairSPHIdealGas::compute
(idealgas_util.np_idealgas) gives hand-worked values on two atoms and keeps the loop's
invariants on the jittered gas_box, the oracle-side preconditions of test_gpu_idealgas.py
hold, and without a device the new entry points fail with ENODEV."""
import ctypes
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

import pyoracle as po
from idealgas_util import (K2, K3, gas_box, gas_engine, gas_oracle, ghosted_inputs, np_idealgas,
                           shock_tube_case)
from test_capi import HEADER, declared_functions, lib_built  # noqa: F401

NEW = ("sph_hip_idealgas_coeff", "sph_hip_idealgas", "sph_engine_idealgas")


def test_header_and_bindings_declare_the_functions(sph_amd):
    names = declared_functions()
    for n in NEW:
        assert n in names and n in sph_amd.EXPORTS
    for m in ("idealgas_coeff", "idealgas"):
        assert callable(getattr(sph_amd.PairContext, m))
    assert callable(sph_amd.Engine.idealgas)


def test_library_exports_the_functions(lib_built):  # noqa: F811
    out = subprocess.run(["nm", "-D", "--defined-only", lib_built], capture_output=True,
                         text=True, check=True).stdout
    exported = set(l.split()[-1] for l in out.splitlines() if " T " in l)
    assert set(NEW) <= exported


def test_engine_gas_layout_matches_header(sph_amd):
    cls = sph_amd.EngineGas
    lines = ['printf("%zu\\n", sizeof(sph_engine_gas));']
    want = [ctypes.sizeof(cls)]
    for f, _ in cls._fields_:
        lines.append(f'printf("%zu\\n", offsetof(sph_engine_gas, {f}));')
        want.append(getattr(cls, f).offset)
    lines.append('printf("%d\\n", SPH_HIP_ABI_VERSION);')
    want.append(2)
    probe = ("#include <stdio.h>\n#include <stddef.h>\n#include \"sph_hip.h\"\n"
             "int main(void){\n" + "\n".join(lines) + "\nreturn 0;}\n")
    d = tempfile.mkdtemp()
    src, exe = os.path.join(d, "probe.c"), os.path.join(d, "probe")
    open(src, "w").write(probe)
    subprocess.run(["gcc", "-I", os.path.dirname(HEADER), src, "-o", exe], check=True)
    got = list(map(int, subprocess.run([exe], capture_output=True, text=True,
                                       check=True).stdout.split()))
    assert got == want
    assert want[0] == 2 * 8 * (sph_amd.SPH_MAXTYPES + 1) ** 2


# ---- the restatement on two atoms -----------------------------------------------------------
H, VISC = 2.0, 0.5
MASS = np.array([0.0, 1.0, 0.25])
E = np.array([2.0, 0.5])          # atom 0 (type 1), atom 1 (type 2)
RHO = np.array([1.0, 0.25])


def _two_atoms(dim, x1, v0, v1, newton=1, nlocal=2):
    x = np.array([[0.0, 0.0, 0.0], x1])
    vest = np.array([v0, v1], dtype=np.float64)
    cut = np.zeros((3, 3))
    cut[1:, 1:] = H
    visc = np.zeros((3, 3))
    visc[1, 2] = VISC                     # (the row atom is type 1: visc[1][2] is read)
    visc[2, 1] = 123.0                    # (... and its transpose is not)
    return np_idealgas(dim, nlocal, newton, x, np.array([1, 2], dtype=np.int32), vest, RHO, E,
                       MASS, visc, cut, np.array([0, 1, 1][:nlocal + 1]), np.array([1]),
                       virial=True)


def _hand(dim, r, dvdr):
    """the pair (0, 1) at distance r along x, by hand: fi = 0.4*2/1/1 = 0.8, fj = 0.4*0.5/0.25/
    0.25 = 3.2, ci = sqrt(0.8), cj = sqrt(0.8) (0.4*0.5/0.25), h = 2"""
    fi, fj, c = 0.8, 3.2, math.sqrt(0.8)
    wfd = (K3 / 128.0 if dim == 3 else K2 / 64.0) * (H - r) ** 2
    fvisc = 0.0
    if dvdr < 0:
        mu = H * dvdr / (r * r + 0.04)
        fvisc = -VISC * (c + c) * mu / 1.25
    fpair = -1.0 * 0.25 * (fi + fj + fvisc) * wfd
    return fpair, wfd


@pytest.mark.parametrize("dim", [3, 2])
def test_two_atoms_hand_worked(dim):
    # approaching: atom 1 at x = 1 moving towards atom 0 at rest: delx = -1, dv = +0.5 ->
    # dvdr = -0.5; the viscosity term counts
    f, drho, de, vir = _two_atoms(dim, [1.0, 0.0, 0.0], [0, 0, 0], [-0.5, 0, 0])
    fpair, wfd = _hand(dim, 1.0, -0.5)
    assert fpair != _hand(dim, 1.0, 0.5)[0]
    np.testing.assert_allclose(f[0], [-1.0 * fpair, 0, 0], rtol=1e-15, atol=0)
    np.testing.assert_allclose(f[1], [1.0 * fpair, 0, 0], rtol=1e-15, atol=0)
    np.testing.assert_allclose(drho, [0.25 * -0.5 * wfd, 1.0 * -0.5 * wfd], rtol=1e-15)
    np.testing.assert_allclose(de, [-0.5 * fpair * -0.5] * 2, rtol=1e-15)
    # two ev_tally calls: 2 * delx^2 * fpair in xx, nothing elsewhere
    np.testing.assert_allclose(vir, [2.0 * fpair, 0, 0, 0, 0, 0], rtol=1e-15)
    # receding: no viscosity term
    f, drho, de, vir = _two_atoms(dim, [1.0, 0.0, 0.0], [0, 0, 0], [0.5, 0, 0])
    fpair, wfd = _hand(dim, 1.0, 0.5)
    assert abs(fpair - -0.25 * 4.0 * wfd) <= 1e-15 * abs(fpair)
    np.testing.assert_allclose(f[0], [-fpair, 0, 0], rtol=1e-15)
    np.testing.assert_allclose(de, [-0.25 * fpair] * 2, rtol=1e-15)
    np.testing.assert_allclose(drho, [0.25 * 0.5 * wfd, 0.5 * wfd], rtol=1e-15)
    # r = h exactly and r > h: outside (the test is rsq < cutsq)
    for r in (2.0, 2.5):
        f, drho, de, vir = _two_atoms(dim, [r, 0.0, 0.0], [0, 0, 0], [-0.5, 0, 0])
        assert not f.any() and not drho.any() and not de.any() and not vir.any()
    # newton off with atom 1 a ghost: the i share only, half the virial (of two tallies)
    f, drho, de, vir = _two_atoms(dim, [1.0, 0.0, 0.0], [0, 0, 0], [-0.5, 0, 0], newton=0,
                                  nlocal=1)
    fpair, wfd = _hand(dim, 1.0, -0.5)
    assert not f[1].any() and drho[1] == 0 and de[1] == 0
    np.testing.assert_allclose(f[0], [-fpair, 0, 0], rtol=1e-15)
    np.testing.assert_allclose(vir[0], 2 * 0.5 * fpair, rtol=1e-15)


# ---- invariants on gas_box ------------------------------------------------------------------
@pytest.fixture(scope="module", params=[3, 2])
def boxed(request, po):
    s, ph = gas_box(request.param)
    return s, ph, ghosted_inputs(s, ph)


def _half(s, ph, d, newton, **kw):
    g = d["g"]
    return np_idealgas(s.dim, g.nlocal, newton, g.x, g.type, d["vest"], d["rho"], d["e"], s.mass,
                       ph.gas_visc, ph.gas_cut, d["hoff"], d["hnb"], **kw)


def test_restatement_invariants(boxed):
    s, ph, d = boxed
    g, n = d["g"], s.n
    f, drho, de = _half(s, ph, d, 1)
    fa, _, dea = _half(s, ph, d, 1, absolute=True)
    po.reverse_comm(g, f, drho, de)
    po.reverse_comm(g, fa, None, dea)
    assert (d["e"] > 0).all() and np.abs(f[:n]).max() > 0
    # about half of the pairs approach (the viscosity branch is exercised both ways)
    i = np.repeat(np.arange(n), np.diff(d["hoff"]))
    j = d["hnb"][:d["hoff"][-1]]
    dv = ((g.x[i] - g.x[j]) * (d["vest"][i] - d["vest"][j])).sum(axis=1)
    assert 0.3 < (dv < 0).mean() < 0.7
    # momentum: sum f = 0
    for k in range(3):
        assert abs(math.fsum(f[:n, k])) <= 1e-12 * math.fsum(fa[:n, k])
    # energy: sum de + sum f . vest = 0
    work = (f[:n] * d["vest"][:n]).sum(axis=1)
    scale = math.fsum(dea[:n]) + math.fsum((fa[:n] * np.abs(d["vest"][:n])).sum(axis=1))
    assert abs(math.fsum(de[:n]) + math.fsum(work)) <= 1e-12 * scale
    # the half list with newton on, after reverse comm = the full list's gather
    ff, df, ef = np_idealgas(s.dim, n, 0, g.x, g.type, d["vest"], d["rho"], d["e"], s.mass,
                             ph.gas_visc, ph.gas_cut, d["foff"], d["fnb"], gather=True)
    _, da, _ = np_idealgas(s.dim, n, 0, g.x, g.type, d["vest"], d["rho"], d["e"], s.mass,
                           ph.gas_visc, ph.gas_cut, d["foff"], d["fnb"], gather=True,
                           absolute=True)
    assert np.all(np.abs(f[:n] - ff[:n]) <= 1e-12 * fa[:n])
    assert np.all(np.abs(de[:n] - ef[:n]) <= 1e-12 * dea[:n])
    assert np.all(np.abs(drho[:n] - df[:n]) <= 1e-12 * da[:n])


def test_newton_off_leaves_ghosts_alone(boxed):
    s, ph, d = boxed
    n = s.n
    f, drho, de, vir0 = _half(s, ph, d, 0, virial=True)
    assert not f[n:].any() and not drho[n:].any() and not de[n:].any()
    f1, _, _, vir1 = _half(s, ph, d, 1, virial=True)
    assert f1[n:].any()
    # (the list is the newton-on half list, which names an owned-ghost pair once: with newton
    # off that pair's tally is halved, so the virial is smaller, never equal)
    assert np.all(np.abs(vir0[:s.dim]) < np.abs(vir1[:s.dim]))


# ---- preconditions of the GPU cases ---------------------------------------------------------
def test_gas_box_oracle_keeps_e_positive(po):
    s, ph = gas_box(3)
    ref = gas_oracle(s, ph, shadows=False)
    ref.setup()
    e0 = ref.s.e.copy()
    ref.run(20)
    assert ref.e_min > 0
    assert np.abs(ref.s.e - e0).max() > 1e-6      # (e moves: the EOS term must follow it)


def test_shock_tube_oracle_stays_in_the_box(po):
    s, ph, fixes = shock_tube_case()
    assert s.n == 480 and (s.type == 2).sum() == 230
    ref = gas_oracle(s, ph, fixes, shadows=False)
    ref.setup()
    ref.run(40)
    assert ref.all_inside and ref.e_min > 0
    assert not ref.f[:, 1].any() and not ref.f[:, 2].any()    # setforce NULL 0 0
    assert np.abs(ref.s.v[:, 0]).max() > 0.05                  # the shock runs


# ---- no silent CPU fallback -----------------------------------------------------------------
def test_no_device_no_gas(sph_amd):
    """Without a device the gas entry points fail with ENODEV (GPU box: skipped)."""
    if sph_amd.device_count() > 0:
        pytest.skip("a HIP device is present")
    s, ph = gas_box(3)
    with pytest.raises(sph_amd.HipError) as ei:
        gas_engine(sph_amd, s, ph).setup()
    assert ei.value.code == -2
    with pytest.raises(sph_amd.HipError) as ei:
        pc = sph_amd.PairContext(3, 2, 1)
        pc.idealgas_coeff(ph.gas_visc, ph.gas_cut, s.mass)
        pc.idealgas(np.zeros((1, 3)), np.zeros(1), np.zeros(1))
    assert ei.value.code == -2


def test_entry_points_refuse_a_null_handle(sph_amd, lib_built):  # noqa: F811
    """the three new C entry points themselves (no context or engine can exist without a
    device, so the bindings above stop in the constructors): called with the NULL handle a
    failed create leaves, each returns SPH_HIP_EINVAL, names itself in sph_hip_last_error and
    writes nothing -- there is no path that computes on the host"""
    L = sph_amd.load()
    tab = np.full(9, 3.0)
    f, drho, de = np.zeros((4, 3)), np.zeros(4), np.zeros(4)
    assert L.sph_hip_idealgas_coeff(None, tab, tab, np.ones(3)) == -1
    assert b"sph_hip_idealgas_coeff" in L.sph_hip_last_error()
    assert L.sph_hip_idealgas(None, f, drho, de, None) == -1
    assert b"sph_hip_idealgas" in L.sph_hip_last_error()
    assert not f.any() and not drho.any() and not de.any()
    assert L.sph_engine_idealgas(None, ctypes.byref(sph_amd.EngineGas())) == -1
    assert b"sph_engine_idealgas" in L.sph_hip_last_error()
