"""CPU side of sph_engine_moments / sph_engine_gyration: the C ABI declares and exports them,
the ctypes mirrors match the header, and the numpy reference of the GPU tests
(tests/moments_util.py) decodes the image flags and bounds its sums as it says."""
import ctypes
import math
import os
import subprocess
import tempfile

import numpy as np

import pyoracle as po
from moments_util import (counted_system, crossing_system, gyration_terms, moment_terms,
                          sum_and_bound, unpack_images, unwrapped, CROSS_SLABS, CROSS_STEPS,
                          CROSS_VX)
from test_capi import HEADER, declared_functions, lib_built  # noqa: F401

NEW = ("sph_engine_moments", "sph_engine_gyration")


def test_header_and_bindings_declare_the_functions(sph_amd):
    names = declared_functions()
    for n in NEW:
        assert n in names and n in sph_amd.EXPORTS
    assert sph_amd.Engine.moments and sph_amd.Engine.gyration and sph_amd.combine_moments


def test_library_exports_the_functions(lib_built):  # noqa: F811
    out = subprocess.run(["nm", "-D", "--defined-only", lib_built], capture_output=True,
                         text=True, check=True).stdout
    exported = set(l.split()[-1] for l in out.splitlines() if " T " in l)
    assert set(NEW) <= exported


def test_struct_layouts_match_header(sph_amd):
    """sizeof / offsetof of sph_group_sel and sph_moments_out from a probe compiled against the
    header = their ctypes mirrors"""
    structs = {"sph_group_sel": sph_amd.GroupSel, "sph_moments_out": sph_amd.MomentsOut}
    lines, want = ['printf("%d\\n", SPH_MAX_MOMENTS);'], [sph_amd.SPH_MAX_MOMENTS]
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
    # (the device writes a result as fifteen 8-byte slots)
    assert ctypes.sizeof(sph_amd.MomentsOut) == 15 * 8 and sph_amd.SPH_MAX_MOMENTS == 8


def test_unwrapping_decodes_every_field():
    """negative and positive counts in each of the three bit fields, alone and together, and
    the round trip through the oracle's packing"""
    cases = np.array([[0, 0, 0], [-2, 0, 0], [3, 0, 0], [0, -2, 0], [0, 3, 0], [0, 0, -2],
                      [0, 0, 3], [-2, 3, -1], [3, -2, 5], [-512, 511, -512], [511, -512, 511]])
    packed = po.img_pack(cases)
    assert packed[0] == (512 << 20) | (512 << 10) | 512
    assert packed[1] == (512 << 20) | (512 << 10) | 510          # x field: the low ten bits
    assert packed[4] == (512 << 20) | (515 << 10) | 512          # y field: the middle ten
    assert packed[5] == (510 << 20) | (512 << 10) | 512          # z field: the top
    assert np.array_equal(unpack_images(packed), cases)
    prd = np.array([7.0, 0.3, 1.0e-3])
    x = np.full((len(cases), 3), 0.1)
    u = unwrapped(x, unpack_images(packed), prd)
    for i, c in enumerate(cases):
        for d in range(3):
            assert u[i, d] == 0.1 + float(c[d]) * prd[d]     # the product, then the add
    assert u[1, 0] == 0.1 - 14.0 and u[4, 1] == 0.1 + 3 * 0.3


def test_fsum_bound_is_self_consistent():
    """a cancelling sum (pairs +-t around a small remainder): its fsum is the remainder's,
    and every shuffled left-to-right or pairwise summation lies inside the bound, though far
    outside 2^-52 of the result itself"""
    rng = np.random.default_rng(5)
    big = rng.uniform(1.0, 2.0, 4000) * 10.0 ** rng.integers(0, 12, 4000)
    small = rng.uniform(-1e-3, 1e-3, 200)
    t = np.concatenate([big, -big, small])
    want, bound = sum_and_bound(t)
    assert want == math.fsum(small)
    assert bound == t.size * 2.0 ** -52 * math.fsum(np.abs(t))
    worst = 0.0
    for k in range(20):
        p = rng.permutation(t)
        naive = 0.0
        for v in p:
            naive += v
        for got in (naive, float(np.sum(p)), float(p.reshape(-1, 100).sum(1).sum())):
            worst = max(worst, abs(got - want))
            assert abs(got - want) <= bound
    assert worst > 2.0 ** -52 * abs(want)      # (the bound is about sum |t|, not the result)


def test_reference_terms_and_scenarios():
    """the terms are the reference's expressions; the crossing case crosses what it says"""
    inp = dict(x=np.array([[0.25, 0.5, 0.75]]), v=np.array([[1.0, -2.0, 0.5]]),
               rho=np.array([0.3]), m=np.array([0.7]), image=np.array([[1, -1, 2]]))
    prd = np.array([2.0, 3.0, 5.0])
    t = moment_terms(inp, prd)
    assert t["mx"][0, 0] == (0.25 + 1 * 2.0) * 0.7 and t["mx"][0, 1] == (0.5 - 3.0) * 0.7
    assert t["mv"][0, 1] == -2.0 * 0.7 and t["volume"][0] == 0.7 / 0.3
    assert moment_terms(inp, prd, images=False)["mx"][0, 2] == 0.75 * 0.7
    cm = np.array([1.0, 1.0, 1.0])
    dx, dy, dz = 2.25 - 1.0, -2.5 - 1.0, 10.75 - 1.0
    g = gyration_terms(inp, prd, cm)[0]
    assert g[0] == (dx * dx + dy * dy + dz * dz) * 0.7
    assert list(g[1:]) == [dx * dx * 0.7, dy * dy * 0.7, dz * dz * 0.7, dx * dy * 0.7,
                           dx * dz * 0.7, dy * dz * 0.7]
    s, ph = crossing_system()
    slab = s.type == 1
    assert np.all(s.v[slab] == np.array([CROSS_VX, 0.0, 0.0]))
    move = CROSS_STEPS * ph.dt * CROSS_VX
    xs = s.x[slab, 0]
    for (lo, hi), face in zip(CROSS_SLABS, (16.0, 8.0)):
        part = xs[(xs >= lo - 0.5) & (xs < hi - 0.5)]
        crossed = (part + move >= face).sum()
        assert 0.25 * part.size < crossed < 0.5 * part.size      # a third of the slab
    for n in (1, 37, 64, 515, 131149):
        c = counted_system(n)
        assert c.n == n and (c.x >= 0).all() and (c.x < c.boxhi).all()
        assert c.boxhi[0] >= 7.0
