"""The pair-layer workloads of bench.py (c2pair, c5pair) and the layer's kernel timing
(sph_hip_set_timing / sph_hip_last_kernel_ms) on small blocks: they run, time something,
and report consistent JSON.  Parity of the styles themselves is test_gpu_pair.py /
test_gpu_multiphase.py."""
import argparse
import contextlib
import importlib.util
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_bench():
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("workload", ["c2pair", "c5pair"])
def test_pair_layer_workload(gpu, sph_amd, workload):
    bench = load_bench()
    args = argparse.Namespace(edge=14, steps=2, warmup=1, no_cpu=True, full=True)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        (bench.c2_pair_main if workload == "c2pair" else bench.c5_pair_main)(args, sph_amd)
    out = json.loads(buf.getvalue().strip().splitlines()[-1])
    assert out["value"] > 0 and out["ms_per_step"] > 0
    for k, v in out["kernels"].items():
        assert v["ms_per_call"] > 0, k
    assert 0 < out["roofline"]["frac"] < 1


def _run_bench(argv):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + argv,
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def _load_dump(d):
    return {fn[:-4]: np.load(os.path.join(d, fn)) for fn in sorted(os.listdir(d))}


def _close(got, want):
    """1e-10 normwise, the suite's parity bar: what a changed summation
    order may move in fp64; another seed or another number of steps moves the fields by
    orders of magnitude more (asserted below)."""
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k].dtype == np.float64 and got[k].shape == want[k].shape, k
        den = max(np.abs(want[k]).max(), 1e-300)
        assert np.abs(got[k] - want[k]).max() / den < 1e-10, k


def test_plain_run_full_run_and_dump(gpu, sph_amd, tmp_path):
    """A plain run carries the headline figures only; --full adds the per-class times of its
    further steps.  --dump-outputs writes the state after the last timed step as float64
    arrays: the same from run to run (seeded inputs), and equal to the state of an engine
    this test drives itself for warmup + steps steps -- so --steps sets the steps run."""
    n, fields = 24, ("x", "v", "f", "rho", "e", "drho", "de")
    base = ["--gpus", "1", "--edge", str(n), "--warmup", "1"]
    a, b, c = (str(tmp_path / k) for k in "abc")
    plain = _run_bench(base + ["--steps", "3", "--dump-outputs", a])
    again = _run_bench(base + ["--steps", "3", "--dump-outputs", b])
    full = _run_bench(base + ["--steps", "5", "--full", "--no-cpu", "--dump-outputs", c])
    for out, steps in ((plain, 3), (again, 3), (full, 5)):
        assert out["steps"] == steps and out["warmup"] == 1 and out["n_gpus"] == 1
        assert out["ms_per_step"] > 0 and out["unit"] == "particle-steps/s"
        assert out["value"] == pytest.approx(n ** 3 / (out["ms_per_step"] * 1e-3))
        assert out["higher_is_better"] is True and out["dtype"] == "f64"
        assert "cpu_baseline" not in out
    assert "neighbor_build_ms" not in plain["kernels"]
    assert full["kernels"]["neighbor_build_ms"] > 0
    bench = load_bench()
    eng = sph_amd.Engine(bench.c2_config(sph_amd, n))
    eng.set_atoms(*bench.make_system(n, 12345))
    eng.setup()
    want = {}
    for total, more in ((4, 4), (6, 2)):
        eng.run(more)
        eng.sync()
        g = eng.get_atoms()
        order = np.argsort(g["tag"], kind="stable")
        want[total] = {k: g[k][order] for k in fields}
    eng.close()
    for k in ("x", "v", "f"):   # two more steps move the state 100x the bar and more
        assert np.abs(want[6][k] - want[4][k]).max() > 1e-8 * np.abs(want[4][k]).max(), k
    da, db, dc = _load_dump(a), _load_dump(b), _load_dump(c)
    assert all(np.isfinite(v).all() for v in da.values())
    _close(da, want[4])
    _close(db, da)
    _close(dc, want[6])


@pytest.mark.parametrize("workload,edge,key", [
    ("c3", "24", "neighbor_build_ms"), ("c5", "30", "neighbor_build_and_phase_change_ms")])
def test_full_run_other_workloads(gpu, workload, edge, key):
    """--full on the other engine workloads: the further steps' per-class times are in the
    line, and absent from a plain run's."""
    base = ["--workload", workload, "--edge", edge, "--steps", "3", "--warmup", "1"]
    plain = _run_bench(base)
    full = _run_bench(base + ["--full", "--no-cpu"])
    assert key not in plain.get("kernels", {}) and "cpu_baseline" not in plain
    assert full["kernels"][key] > 0 and full["kernels"]["integrate_ms_per_step"] > 0
    assert plain["value"] > 0 and full["value"] > 0 and full["steps"] == 3


def test_kernel_timing_api(gpu, sph_amd):
    x = np.array([[0.0, 0, 0], [0.5, 0, 0], [0, 0.5, 0]])
    t = np.ones(3, dtype=np.int32)
    ctx = sph_amd.PairContext(3, 1, 1)
    ctx.atoms(3, 0, x, t, vest=np.zeros((3, 3)), rho=np.ones(3), e=np.zeros(3))
    cut = np.array([[0.0, 0.0], [0.0, 1.0]])
    ctx.rhosum_coeff(cut, np.array([0.0, 1.0]))
    ctx.list_csr(sph_amd.SPH_LIST_FULL, np.array([0, 2, 4, 6]), np.array([1, 2, 0, 2, 0, 1]))
    ctx.rhosum(np.zeros(3))
    assert ctx.last_kernel_ms() == 0.0          # timing off
    ctx.set_timing(True)
    ctx.rhosum(np.zeros(3))
    assert ctx.last_kernel_ms() > 0.0
    ctx.close()
