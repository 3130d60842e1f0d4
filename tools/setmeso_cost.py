#!/usr/bin/env python3
"""Cost of the armed far-field clamp and of one 16-selection reduction at C5's own size.

    rocprofv3 --kernel-trace --stats -d OUT -- python tools/setmeso_cost.py [--edge 159]

runs bench.py's C5 system (159^3 = 4.02M atoms, fix phase_change armed) with bubble.lmp:94-96's
`fix setmeso meso_t Tinf noregion sphere` armed; the kernel stats then hold k_setmeso's and
k_reduce_part's averages.  Without the profiler it prints the host-timed figures alone: the
step with and without the clamp, and the reduce call (launches, copy and sync included)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from __graft_entry__ import _import_pkg  # noqa: E402


def engine(sph, n, clamp):
    x, v, t, rho, e, cv, rmass = bench.c5_system(n)
    mp, dt, pc = bench.c5_physics(n)
    cfg = sph.make_config(3, 2, [0.0] * 3, [1.0] * 3, [1, 1, 1], [0.0, 1.0, 1.0], 0.0, dt,
                          neigh_every=1, mp=mp)
    eng = sph.Engine(cfg)
    eng.set_atoms(x, v, t, rho, e, cv)
    eng.set_atoms_multiphase(rmass, cv)
    eng.phase_change(pc["Tc"], pc["Tt"], pc["Hwv"], pc["dr"], pc["to_mass"], pc["cutoff"],
                     pc["from_type"], pc["to_type"], nevery=pc["nevery"], seed=pc["seed"],
                     prob=pc["prob"])
    if clamp:
        eng.setmeso("t", 1.0, noregion=sph.sphere((0.5, 0.5, 0.5), 0.5 - 2.6 / n))
    eng.setup()
    return eng


def step_ms(eng, warmup, steps):
    eng.run(warmup)
    eng.sync()
    t0 = time.perf_counter()
    eng.run(steps)
    eng.sync()
    return (time.perf_counter() - t0) / steps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--edge", type=int, default=159)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    sph = _import_pkg()
    n = args.edge
    out = {"atoms": n ** 3}
    eng = engine(sph, n, clamp=False)
    out["step_ms_plain"] = step_ms(eng, args.warmup, args.steps)
    eng.close()
    eng = engine(sph, n, clamp=True)
    out["step_ms_clamped"] = step_ms(eng, args.warmup, args.steps)
    far = sph.sphere((0.5, 0.5, 0.5), 0.5 - 2.6 / n)
    groups = [dict(), dict(types=[1]), dict(types=[2]), dict(noregion=far)]
    sels = [dict(quantity=q, **g) for q in ("one", "rho", "e", "t") for g in groups]
    eng.reduce(sels)
    reps = 20
    t0 = time.perf_counter()
    for _ in range(reps):
        eng.reduce(sels)
    out["reduce16_call_ms"] = (time.perf_counter() - t0) / reps * 1e3
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
