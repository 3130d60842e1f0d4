#!/usr/bin/env python3
"""Cost of the force-fix post_force launch and of one layer profile on bench.py's C2 system.

    python tools/forcefix_cost.py [--edge 100]

Runs the C2 engine (edge^3 atoms) with no force fix, with one (a per-mass body force on all
atoms) and with eight (seven more over half-box blocks and a sphere, one of them tallying),
with the engine's event timers on the integrate class alone -- the class the post_force launch
is timed under -- and prints the class's time per step for each; the differences against the
unarmed engine are the launch's cost.  Then one `profile` call (vx and rho over the layers
along y, sort and fold, the copy and the sync included) timed on the host."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from __graft_entry__ import _import_pkg  # noqa: E402


def engine(sph, n, nfix):
    x, v, t, rho, e, cv = bench.make_system(n, 12345)
    eng = sph.Engine(bench.c2_config(sph, n))
    eng.set_atoms(x, v, t, rho, e, cv)
    L = float(n)
    if nfix >= 1:
        eng.addforce(1e-3, 0.0, 0.0, per_mass=True)
    for k in range(1, nfix):
        if k == 7:
            eng.setforce(None, 0.0, None, region=sph.sphere((L / 2,) * 3, L / 8), tally=True)
        else:
            lo, hi = (0.0, L / 2) if k % 2 else (L / 2, L)
            eng.addforce(0.0, 1e-3 * k, 0.0, per_mass=bool(k & 2),
                         region=sph.block((-1e20, lo, -1e20), (1e20, hi, 1e20)))
    eng.setup()
    return eng


def integrate_ms(eng, warmup, steps):
    eng.run(warmup)
    eng.sync()
    eng.set_timing(True, classes=(eng.T_INT,))
    t0 = time.perf_counter()
    eng.run(steps)
    eng.sync()
    wall = (time.perf_counter() - t0) / steps * 1e3
    return eng.stats()["ms_integrate"] / steps, wall


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--edge", type=int, default=100)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    sph = _import_pkg()
    n = args.edge
    out = {"atoms": n ** 3, "steps": args.steps}
    for nfix in (0, 1, 8):
        eng = engine(sph, n, nfix)
        ms, wall = integrate_ms(eng, args.warmup, args.steps)
        out[f"integrate_class_ms_per_step_{nfix}fix"] = ms
        out[f"step_ms_{nfix}fix"] = wall
        if nfix == 8:
            lo, nl = sph.layers("lower", 2.5, 0.0, float(n))
            eng.profile(1, lo, 2.5, nl, ["vx", "rho"])
            reps = 20
            t0 = time.perf_counter()
            for _ in range(reps):
                eng.profile(1, lo, 2.5, nl, ["vx", "rho"])
            out["profile_layers"] = nl
            out["profile_call_ms"] = (time.perf_counter() - t0) / reps * 1e3
        eng.close()
    for nfix in (1, 8):
        out[f"post_force_ms_{nfix}fix"] = (out[f"integrate_class_ms_per_step_{nfix}fix"] -
                                           out["integrate_class_ms_per_step_0fix"])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
