"""CPU side of sph_engine_virial_every / sph_engine_thermo: the C ABI declares and exports
them at ABI version 2, the ctypes mirror matches the header, and on the scenarios of
test_gpu_thermo.py the reference's fdotr form of the virial (x . f over owned and ghost atoms
before reverse comm, what a newton-on run prints) agrees with the pair tally the GPU tests
compare against, within their bar."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

from test_capi import HEADER, declared_functions, lib_built  # noqa: F401
from thermo_util import CASES, VTOL, oracle_history

NEW = ("sph_engine_virial_every", "sph_engine_thermo")


def test_header_and_bindings_declare_the_functions(sph_amd):
    names = declared_functions()
    for n in NEW:
        assert n in names and n in sph_amd.EXPORTS
    assert sph_amd.Engine.virial_every and sph_amd.Engine.thermo
    with open(HEADER) as fh:
        assert "#define SPH_HIP_ABI_VERSION 2" in fh.read()


def test_library_exports_the_functions(lib_built):  # noqa: F811
    out = subprocess.run(["nm", "-D", "--defined-only", lib_built], capture_output=True,
                         text=True, check=True).stdout
    exported = set(l.split()[-1] for l in out.splitlines() if " T " in l)
    assert set(NEW) <= exported
    L = ctypes.CDLL(lib_built)
    L.sph_hip_abi_version.restype = ctypes.c_int
    assert L.sph_hip_abi_version() == 2


def test_struct_layout_matches_header(sph_amd):
    src = ('#include <stddef.h>\n#include <stdio.h>\n#include "sph_hip.h"\n'
           'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(sph_thermo_out),'
           ' offsetof(sph_thermo_out, virial_step), offsetof(sph_thermo_out, virial),'
           ' offsetof(sph_thermo_out, ke_tensor), offsetof(sph_thermo_out, ke),'
           ' offsetof(sph_thermo_out, egrav), offsetof(sph_thermo_out, volume),'
           ' offsetof(sph_thermo_out, press)); return 0; }\n')
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "p.c"), os.path.join(d, "p")
        with open(c, "w") as fh:
            fh.write(src)
        subprocess.run(["cc", "-I", os.path.dirname(HEADER), c, "-o", exe], check=True)
        got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True,
                                              check=True).stdout.split()]
    T = sph_amd.ThermoOut
    want = [ctypes.sizeof(T)] + [getattr(T, f).offset for f in
                                 ("virial_step", "virial", "ke_tensor", "ke", "egrav", "volume",
                                  "press")]
    assert got == want


def test_null_arguments_need_no_device(sph_amd):
    L = sph_amd.load()
    assert L.sph_engine_virial_every(None, 1) != 0
    assert L.sph_engine_thermo(None, 1.0, 1.0, None) != 0


@pytest.mark.parametrize("name", CASES)
def test_fdotr_agrees_with_pair_tally(name):
    """virial_fdotr_compute's sum against the pair tally, per component within 1e-10 S_ab, at
    the setup step and two steps on.  sph/taitwater/morris' force has the part velx * fvisc
    that is not along del: its x . f carries sum del_a vel_b fvisc besides (thermo_util
    fdotr_visc, restated in numpy), which is taken off before the comparison and must itself
    be far above the bar -- the tally is what the engine is held to."""
    hist = oracle_history(name, {"monaghan": 7, "morris": 7, "dam2d": 3}.get(name, 2))
    for k in (0, 2):
        h = hist[k]
        err = np.abs(h["fdotr"] - h["fdotr_visc"] - h["virial"])
        bar = VTOL * h["vscale"]
        print(f"[thermo-cpu] {name} step {k}: worst fdotr/tally ratio "
              f"{np.max(err / np.where(bar > 0, bar, 1e-300)):.3e}")
        assert (err <= bar).all(), (name, k, err, bar)
        if name == "morris":
            assert np.abs(h["fdotr_visc"][:3]).max() > 1e3 * bar[:3].max()
        else:
            assert not h["fdotr_visc"].any()
