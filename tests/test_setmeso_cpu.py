"""CPU side of fix setmeso / setmesode and the on-device reductions: the C ABI declares and
exports them, the ctypes mirrors match the header, and the oracle-side preconditions of the
GPU tests (tests/test_setmeso_gpu.py) hold -- the clamps change the run, select a proper
subset, and no atom sits on a region surface where engine and oracle could legitimately
disagree."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

import pyoracle as po
from conftest import ROOT, rel_err
from setmeso_util import (FIELD_OF, bubble_case, c3_case, clamp_region, clamped_oracle,
                          np_selected, surface_distance)
from test_capi import HEADER, declared_functions, lib_built  # noqa: F401

NEW = ("sph_engine_setmeso", "sph_engine_reduce")


def test_header_and_bindings_declare_the_functions(sph_amd):
    names = declared_functions()
    for n in NEW:
        assert n in names and n in sph_amd.EXPORTS
    assert sph_amd.Engine.setmeso and sph_amd.Engine.reduce


def test_library_exports_the_functions(lib_built):  # noqa: F811
    out = subprocess.run(["nm", "-D", "--defined-only", lib_built], capture_output=True,
                         text=True, check=True).stdout
    exported = set(l.split()[-1] for l in out.splitlines() if " T " in l)
    assert set(NEW) <= exported


def test_struct_layouts_match_header(sph_amd):
    """sizeof / offsetof of sph_region, sph_setmeso, sph_reduce_sel, sph_reduce_out from a
    probe compiled against the header = their ctypes mirrors"""
    structs = {"sph_region": sph_amd.Region, "sph_setmeso": sph_amd.SetMeso,
               "sph_reduce_sel": sph_amd.ReduceSel, "sph_reduce_out": sph_amd.ReduceOut}
    lines, want = [], []
    for cname, cls in structs.items():
        lines.append(f'printf("%zu\\n", sizeof({cname}));')
        want.append(ctypes.sizeof(cls))
        for f, _ in cls._fields_:
            lines.append(f'printf("%zu\\n", offsetof({cname}, {f}));')
            want.append(getattr(cls, f).offset)
    probe = ("#include <stdio.h>\n#include <stddef.h>\n#include \"sph_hip.h\"\n"
             "int main(void){\n" + "\n".join(lines) + "\nreturn 0;}\n")
    d = tempfile.mkdtemp()
    src, exe = os.path.join(d, "probe.c"), os.path.join(d, "probe")
    open(src, "w").write(probe)
    subprocess.run(["gcc", "-I", os.path.dirname(HEADER), src, "-o", exe], check=True)
    got = list(map(int, subprocess.run([exe], capture_output=True, text=True,
                                       check=True).stdout.split()))
    assert got == want
    assert (sph_amd.SPH_MAX_SETMESO, sph_amd.SPH_MAX_REDUCE) == (8, 16)


def test_region_helpers(sph_amd):
    r = sph_amd.sphere((0.5, 0.25, 0.0), 0.2, side="out")
    assert (r.style, r.interior, r.xc, r.yc, r.zc, r.radius) == (0, 0, 0.5, 0.25, 0.0, 0.2)
    b = sph_amd.block((0, 1, 2), (3, 4, 5))
    assert (b.style, b.interior) == (1, 1)
    assert (b.xlo, b.xhi, b.ylo, b.yhi, b.zlo, b.zhi) == (0, 3, 1, 4, 2, 5)
    with pytest.raises(ValueError):
        sph_amd.sphere((0, 0, 0), 1.0, side="up")


def _preconditions(s, ph, clamps, dx, nsteps):
    """After setup and each step: every clamp moves its field by more than 1e-3 normwise
    against the unclamped run, selects a non-empty set with a non-empty complement, and no
    atom lies within 1e-6 dx of a region surface."""
    ref = clamped_oracle(s, ph, clamps, shadows=False)
    plain = clamped_oracle(s, ph, (), shadows=False)
    ref.setup()
    plain.setup()
    for step in range(nsteps + 1):
        if step:
            ref.run(1)
            plain.run(1)
        for c in clamps:
            m = np_selected(c, ref.s.x, ref.s.type)
            assert 0 < m.sum() < ref.s.n, (step, c["what"])
            assert surface_distance(clamp_region(c), ref.s.x).min() > 1e-6 * dx, (step, c["what"])
            k = FIELD_OF[c["what"]]
            a, b = ref.field(k), plain.field(k)
            assert a.shape != b.shape or rel_err(a, b) > 1e-3, (step, c["what"])
    return ref


@pytest.mark.parametrize("nx,dim,pc", [(10, 3, False), (10, 3, True), (16, 2, True)])
def test_bubble_clamp_preconditions(sph_amd, nx, dim, pc):
    s, ph, clamps, dx = bubble_case(sph_amd, nx, dim, pc)
    if (nx, dim) == (10, 3):
        # (R/dx)^2 = 5.76; the sites' squared distances from the centre are k/4 with k a sum
        # of three odd squares: none on the surface
        assert abs((clamps[0]["noregion"].radius / dx) ** 2 - 5.76) < 1e-12
    ref = _preconditions(s, ph, clamps, dx, 5)
    if pc:
        assert ref.ninserted >= 1   # (a created atom meets the clamp)
    # after setup the clamped atoms carry e = cv * Tinf exactly (a step's final integrate
    # then adds dtf * de)
    ref = clamped_oracle(s, ph, clamps, shadows=False)
    ref.setup()
    m = np_selected(clamps[0], ref.s.x, ref.s.type)
    assert np.array_equal(ref.s.e[m], ref.s.cv[m] * clamps[0]["value"])


def test_c3_clamp_preconditions(sph_amd):
    s, ph, clamps, dx = c3_case(sph_amd)
    ref = _preconditions(s, ph, clamps, dx, 12)
    assert ref.last_build == 10   # (the 12 steps cross a rebuild, the first 5 none)
