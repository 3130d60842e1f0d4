#!/usr/bin/env python3
"""What neigh_modify check yes costs and buys on bench.py's C2 box.

    python tools/neighcheck_cost.py [--edge 100] [--out profiles/neighcheck/neighcheck_cost.json]

edge^3 atoms of the C2 lattice (h = 3, skin 0.3, rhosum every step), four engines on the same
box in one session:
  every10        neigh_every 10, no neigh_modify call (bench.py's setting)
  every10_check  neigh_modify every 10 delay 0 check yes
  every1_check   neigh_modify every 1 delay 0 check yes
  never          neigh_modify every 10^6 check no: plain steps only, no rebuild, no check
Each runs `warmup` steps once; then the four alternate, `rounds` times `steps` steps each.
Per engine and round: wall ms per step (host clock around run + sync), builds and checks of the
round.  A second pass with the event timers on the integrate class alone (class T_INT) gives
the integrate kernel's ms per step: every1_check runs the checking instantiation on every step,
never the plain one.  While every1_check builds nothing, each of its steps is an eligible step
that does not rebuild, so its wall time less never's is what such a step costs over a plain one,
the host synchronise included.  Prints one JSON line and writes it to --out."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from __graft_entry__ import _import_pkg  # noqa: E402

KINDS = {"every10": None, "every10_check": (10, 0, True), "every1_check": (1, 0, True),
         "never": (1000000, 0, False)}


def engine(sph, n, nm):
    x, v, t, rho, e, cv = bench.make_system(n, 12345)
    cut = np.zeros((2, 2))
    cut[1, 1] = 3.0
    visc = np.zeros((2, 2))
    visc[1, 1] = 0.1
    cfg = sph.make_config(3, 1, [0.0] * 3, [float(n)] * 3, [1, 1, 1], [0.0, 1.0], 0.3, 1e-3,
                          neigh_every=10, rhosum=dict(nstep=1, cut=cut),
                          tait=dict(rho0=np.array([0.0, 1.0]), c0=np.array([0.0, 10.0]),
                                    visc=visc, cut=cut))
    eng = sph.Engine(cfg)
    if nm is not None:
        eng.neigh_modify(*nm)
    eng.set_atoms(x, v, t, rho, e, cv)
    eng.setup()
    return eng


def summary(v):
    return dict(runs=v, median=statistics.median(v), min=min(v), max=max(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--edge", type=int, default=100)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sph = _import_pkg()
    engs = {k: engine(sph, args.edge, nm) for k, nm in KINDS.items()}
    for eng in engs.values():
        eng.run(args.warmup)
        eng.sync()
    wall = {k: [] for k in KINDS}
    integ = {k: [] for k in KINDS}
    builds = {k: [] for k in KINDS}
    checks = {k: [] for k in KINDS}
    for timed in (False, True):
        for _ in range(args.rounds):
            for k, eng in engs.items():
                before = eng.neigh_stats()
                if timed:
                    eng.set_timing(True, classes=(eng.T_INT,))
                eng.sync()
                t0 = time.perf_counter()
                eng.run(args.steps)
                eng.sync()
                dt = time.perf_counter() - t0
                after = eng.neigh_stats()
                if timed:
                    integ[k].append(eng.stats()["ms_integrate"] / args.steps)
                    eng.set_timing(False)
                else:
                    wall[k].append(1e3 * dt / args.steps)
                    builds[k].append(after["builds"] - before["builds"])
                    checks[k].append(after["checks"] - before["checks"])
    out = {"atoms": args.edge ** 3, "steps": args.steps, "warmup": args.warmup,
           "rounds": args.rounds, "skin": 0.3}
    for k in KINDS:
        out[k] = dict(wall_ms_per_step=summary(wall[k]), integrate_ms_per_step=summary(integ[k]),
                      builds=builds[k], checks=checks[k])
    out["check_integrate_over_plain"] = (out["every1_check"]["integrate_ms_per_step"]["median"] /
                                         out["never"]["integrate_ms_per_step"]["median"])
    if not any(builds["every1_check"]):
        out["eligible_step_without_rebuild_ms"] = out["every1_check"]["wall_ms_per_step"]["median"]
        out["plain_step_ms"] = out["never"]["wall_ms_per_step"]["median"]
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
