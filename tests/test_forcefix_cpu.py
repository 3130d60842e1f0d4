"""CPU side of fix setforce / addforce and the layer profiles: the C ABI declares and exports
them, the ctypes mirrors match the header, layers() restates fix ave/spatial's layer set-up on
hand-worked cases, and the oracle-side preconditions of tests/test_gpu_forcefix.py hold --
every selection is a non-empty proper subset, no atom sits within 1e-6 of a region surface or
a layer boundary in any step the GPU cases run (a last-bit difference in x then cannot flip a
membership), the fixes change the run, and the phase-change scenario creates an atom."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

import pyoracle as po
from conftest import rel_err
from forcefix_util import (BRICKS_PG, POISEUILLE_DELTA, boundary_distance, bricks_case,
                           buoyancy_case, c3_walls_case, fix_region, forced_oracle, foriginal,
                           nevery_case, np_layer, order_case, poiseuille_case)
from setmeso_util import np_selected, surface_distance
from test_capi import HEADER, declared_functions, lib_built  # noqa: F401

NEW = ("sph_engine_forcefix", "sph_engine_forcefix_total", "sph_engine_profile")


def test_header_and_bindings_declare_the_functions(sph_amd):
    names = declared_functions()
    for n in NEW:
        assert n in names and n in sph_amd.EXPORTS
    for m in ("setforce", "addforce", "force_total", "profile"):
        assert callable(getattr(sph_amd.Engine, m))
    assert (sph_amd.SPH_Q_VX, sph_amd.SPH_Q_VY, sph_amd.SPH_Q_VZ) == (7, 8, 9)
    assert (sph_amd.SPH_FF_SET, sph_amd.SPH_FF_ADD) == (0, 1)


def test_library_exports_the_functions(lib_built):  # noqa: F811
    out = subprocess.run(["nm", "-D", "--defined-only", lib_built], capture_output=True,
                         text=True, check=True).stdout
    exported = set(l.split()[-1] for l in out.splitlines() if " T " in l)
    assert set(NEW) <= exported


def test_struct_layouts_match_header(sph_amd):
    """sizeof / offsetof of sph_forcefix and sph_profile from a probe compiled against the
    header = their ctypes mirrors; the limits and constants too"""
    structs = {"sph_forcefix": sph_amd.ForceFix, "sph_profile": sph_amd.Profile}
    lines, want = [], []
    for cname, cls in structs.items():
        lines.append(f'printf("%zu\\n", sizeof({cname}));')
        want.append(ctypes.sizeof(cls))
        for f, _ in cls._fields_:
            lines.append(f'printf("%zu\\n", offsetof({cname}, {f}));')
            want.append(getattr(cls, f).offset)
    for c in ("SPH_MAX_FORCEFIX", "SPH_MAX_PROFILE_Q", "SPH_FF_SET", "SPH_FF_ADD", "SPH_Q_VX",
              "SPH_Q_VY", "SPH_Q_VZ"):
        lines.append(f'printf("%d\\n", {c});')
        want.append(getattr(sph_amd, c))
    probe = ("#include <stdio.h>\n#include <stddef.h>\n#include \"sph_hip.h\"\n"
             "int main(void){\n" + "\n".join(lines) + "\nreturn 0;}\n")
    d = tempfile.mkdtemp()
    src, exe = os.path.join(d, "probe.c"), os.path.join(d, "probe")
    open(src, "w").write(probe)
    subprocess.run(["gcc", "-I", os.path.dirname(HEADER), src, "-o", exe], check=True)
    got = list(map(int, subprocess.run([exe], capture_output=True, text=True,
                                       check=True).stdout.split()))
    assert got == want


# ---- layers() -------------------------------------------------------------------------------
@pytest.mark.parametrize("origin,delta,boxlo,boxhi,lo,n", [
    # origin lower, box 0..10: layers 0, 2.5, .. 10
    ("lower", 2.5, 0.0, 10.0, 0.0, 4),
    # origin center (5): down 5 - 2*2 = 1 > 0 so one more, lo = -1; up 5 + 2*2 = 9 < 10 so
    # hi = 11: six layers of 2 from -1
    ("center", 2.0, 0.0, 10.0, -1.0, 6),
    # origin upper (10): down 10 - 3*3 = 1 > 0, lo = -2; hi = 10: four layers of 3
    ("upper", 3.0, 0.0, 10.0, -2.0, 4),
    # origin below the box (-3.5): n = (int)(3.5 / 2) = 1, lo = -1.5; up (int)(13.5 / 2) = 6,
    # hi = 8.5 < 10 so 10.5: six layers of 2 from -1.5
    (-3.5, 2.0, 0.0, 10.0, -1.5, 6),
    # origin above the box (12.25): down (int)(12.25 / 4) = 3, lo = 0.25 > 0 so -3.75; hi:
    # (int)(2.25 / 4) = 0, hi = 12.25: four layers of 4
    (12.25, 4.0, 0.0, 10.0, -3.75, 4),
    # a box length (7) that is no multiple of delta (0.9): eight layers from 0, the last one
    # reaching to 7.2
    ("lower", 0.9, 0.0, 7.0, 0.0, 8),
    # a box that does not start at 0, origin inside: 1.0 - 3*0.5 = -0.5 == boxlo; up
    # 1.0 + 6*0.5 = 4.0 == boxhi: nine layers
    (1.0, 0.5, -0.5, 4.0, -0.5, 9),
])
def test_layers_hand_worked(sph_amd, origin, delta, boxlo, boxhi, lo, n):
    got_lo, got_n = sph_amd.layers(origin, delta, boxlo, boxhi)
    assert got_n == n and abs(got_lo - lo) < 1e-12
    # the layers cover the box
    assert got_lo <= boxlo and got_lo + got_n * delta >= boxhi - 1e-12


def test_layers_rejects_bad_delta(sph_amd):
    with pytest.raises(ValueError):
        sph_amd.layers("lower", 0.0, 0.0, 1.0)


def test_np_layer_rule():
    """the layer rule on hand-worked coordinates: remap once, truncate, clamp"""
    c = np.array([-0.5, 0.0, 0.89, 0.95, 6.99, 7.0, 7.3, 3.0])
    # periodic box 0..7: -0.5 -> 6.5 (layer 7), 7.0 -> 0.0 (layer 0), 7.3 -> 0.3 (layer 0)
    assert np_layer(c, 0.0, 0.9, 8, 0.0, 7.0, True).tolist() == [7, 0, 0, 1, 7, 0, 0, 3]
    # not periodic: below lo clamps to 0, past the last layer to nlayers - 1
    assert np_layer(c, 1.0, 2.0, 2, 0.0, 7.0, False).tolist() == [0, 0, 0, 0, 1, 1, 1, 1]


# ---- preconditions of the GPU cases ---------------------------------------------------------
def _walk(s, ph, fixes, nsteps, dx, clamps=(), procgrid=None, moves=True):
    """After setup and each step: every fix that was applied selects a non-empty proper subset
    at more than 1e-6 dx from its region's surface; the fixes change f against a plain run of
    the same physics."""
    ref = forced_oracle(s, ph, fixes, clamps=clamps, procgrid=procgrid, shadows=False)
    plain = forced_oracle(s, ph, (), clamps=clamps, procgrid=procgrid, shadows=False)
    ref.setup()
    plain.setup()
    for step in range(nsteps + 1):
        if step:
            ref.run(1)
            plain.run(1)
        for k, c in enumerate(fixes):
            m = np_selected(c, ref.s.x, ref.s.type)
            assert 0 < m.sum() < ref.s.n, (step, k)
            r = fix_region(c)
            if r is not None:
                assert surface_distance(r, ref.s.x).min() > 1e-6 * dx, (step, k)
        if moves and ref.f.shape == plain.f.shape:
            assert rel_err(ref.f, plain.f) > 1e-3, step
    return ref


@pytest.mark.parametrize("nsteps", [12])
def test_c3_walls_preconditions(sph_amd, nsteps):
    s, ph, fixes = c3_walls_case(sph_amd)
    assert (s.x >= s.boxlo).all() and (s.x < s.boxhi).all()   # (no first-rebuild wrap)
    assert not s.v[s.type == 2].any() and s.v[s.type == 1].any()
    ref = _walk(s, ph, fixes, nsteps, 1.0)
    assert ref.last_build == 10   # (the 12 steps cross a rebuild, the first 5 none)
    w = s.type == 2               # the walls never moved
    assert np.array_equal(ref.s.x[w], s.x[w]) and not ref.s.v[w].any()
    # fluid inside the block and outside the sphere: the set components, then the body force
    m = (np_selected(fixes[1], ref.s.x, ref.s.type) & ~np_selected(fixes[2], ref.s.x, ref.s.type))
    assert m.any()


def test_order_preconditions(sph_amd):
    for set_first in (True, False):
        s, ph, fixes = order_case(sph_amd, set_first)
        ref = _walk(s, ph, fixes, 2, 1.0)
        a, b = (np_selected(c, ref.s.x, ref.s.type) for c in fixes)
        assert (a & b).any() and (a & ~b).any() and (b & ~a).any()   # (they overlap, properly)


def test_nevery_preconditions(sph_amd):
    s, ph, fixes = nevery_case(sph_amd)
    ref = _walk(s, ph, fixes, 7, 1.0, moves=False)
    assert ref.ff_applied == [(0, 0), (3, 0), (6, 0)]   # ntimestep % 3, step 0 included


@pytest.mark.parametrize("dim", [2, 3])
def test_poiseuille_preconditions(sph_amd, dim):
    s, ph, fixes = poiseuille_case(sph_amd, dim)
    assert ph.every == 1 and ph.tait and not ph.st and not ph.heat and ph.cg_nstep == 0
    ref = _walk(s, ph, fixes, 6, 1.0)
    assert not ref.de.any() and not ref.cg.any()
    lo, n = sph_amd.layers("lower", POISEUILLE_DELTA, s.boxlo[1], s.boxhi[1])
    assert n * POISEUILLE_DELTA > s.boxhi[1] - s.boxlo[1]   # (no multiple of delta)
    assert boundary_distance(ref.s.x[:, 1], lo, POISEUILLE_DELTA, n).min() > 1e-6
    lay = np_layer(ref.s.x[:, 1], lo, POISEUILLE_DELTA, n, s.boxlo[1], s.boxhi[1], True)
    assert np.bincount(lay, minlength=n).min() > 0
    # no atom on the shared closed plane, where the two fixes would both apply
    lower, upper = (np_selected(c, ref.s.x, ref.s.type) for c in fixes[:2])
    assert not (lower & upper).any() and ((lower | upper) == (ref.s.type == 1)).all()


def test_buoyancy_preconditions(sph_amd):
    s, ph, clamps, fixes, dx = buoyancy_case(sph_amd)
    ref = _walk(s, ph, fixes, 5, dx, clamps=clamps, moves=False)
    assert ref.ninserted >= 1      # (a created atom meets the fix)
    new = np.arange(s.n, ref.s.n)
    assert (ref.s.type[new] == 2).all() and ref.ff_sel[0][new].all()
    # the step an atom is created in is one the walk compared; its f carries mass * g
    assert np.array_equal(ref.f[new], ref.ff_pre[0][new] + ref.s.rmass[new, None] *
                          np.array(fixes[0]["value"]))


def test_bricks_preconditions(sph_amd):
    s, ph, fixes = bricks_case(sph_amd)
    ref = _walk(s, ph, fixes, 3, 1.0, procgrid=BRICKS_PG)
    r = fixes[0]["region"]
    cut = 0.5 * (s.boxlo[0] + s.boxhi[0])
    assert r.xc - r.radius < cut < r.xc + r.radius            # the sphere straddles the cut
    own = po.brick_owner(ref.s, ref.s.x, BRICKS_PG)
    m = ref.ff_sel[0]
    assert (m & (own == 0)).any() and (m & (own == 1)).any()
    tot, mag = foriginal(ref, 0)
    assert mag > 0 and np.abs(tot).max() > 1e-6 * mag   # (a drag that does not cancel away)
