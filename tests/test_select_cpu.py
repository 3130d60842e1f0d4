"""csrc/sph_select.h, the helpers that turn the launchers' run-time selectors into template
arguments, checked on the CPU: tests/select_cpu_main.cpp includes that header and nothing else
of the project, is built with a host compiler under AddressSanitizer + UndefinedBehaviorSanitizer
and run once.  It checks that each listed value reaches the lambda as its own constant, an
unlisted one as the declared fall-back, true / false as theirs, and that nested helpers
compose (bool x int x shape)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lammps-sph-multiphase_amd", "csrc")


def _cxx():
    for name in ("g++", "c++", "clang++"):
        if shutil.which(name):
            return name
    return None


@pytest.mark.skipif(_cxx() is None, reason="needs a host C++ compiler")
def test_select_helpers(tmp_path):
    exe = tmp_path / "select_check"
    b = subprocess.run([_cxx(), "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-o", str(exe),
                        os.path.join(ROOT, "tests", "select_cpu_main.cpp")],
                       capture_output=True, text=True, timeout=120)
    assert b.returncode == 0, b.stderr
    env = dict(os.environ, ASAN_OPTIONS="verify_asan_link_order=0:detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 0, r.stdout + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
    assert "select: all checks passed" in r.stdout
