#!/usr/bin/env python3
"""What fix dt/reset costs per step on bench.py's C2 box.

    python tools/dtreset_cost.py [--edge 100] [--out profiles/dtreset/dtreset_cost.json]

edge^3 atoms of the C2 lattice (h = 3, skin 0.3, rhosum every step, rebuild every 10), three
engines on the same box in one session:
  plain     no dt_reset call (bench.py's setting): the fused final+initial integrate
  every1    dt_reset(1, None, dt, xmax) with an xmax no atom comes near: every step is a reset
            step (final+scan, fold, initial: three launches), MIN with tmax = dt holds dt, so
            the physics is plain's
  every10   dt_reset(10, ...): nine steps in ten run the fused kernel in its dt-from-record form
Each runs `warmup` steps once; then the three alternate, `rounds` times `steps` steps each.
Per engine and round: wall ms per step (host clock around run + sync).  A second pass with the
event timers on the integrate class alone (class T_INT: the integrate, scan and fold kernels
and the post_force fixes, none here) gives that class's ms per step; every1's less plain's is
what un-fusing the integrate, the scan and the fold cost on the device.  The armed engines must
end with dt unchanged and the plain engine's positions bit for bit.  Prints one JSON line and
writes it to --out."""
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

DT = 1e-3
KINDS = {"plain": None, "every1": 1, "every10": 10}


def engine(sph, n, nevery):
    x, v, t, rho, e, cv = bench.make_system(n, 12345)
    cut = np.zeros((2, 2))
    cut[1, 1] = 3.0
    visc = np.zeros((2, 2))
    visc[1, 1] = 0.1
    cfg = sph.make_config(3, 1, [0.0] * 3, [float(n)] * 3, [1, 1, 1], [0.0, 1.0], 0.3, DT,
                          neigh_every=10, rhosum=dict(nstep=1, cut=cut),
                          tait=dict(rho0=np.array([0.0, 1.0]), c0=np.array([0.0, 10.0]),
                                    visc=visc, cut=cut))
    eng = sph.Engine(cfg)
    if nevery is not None:
        eng.dt_reset(nevery, None, DT, 1.0e3)
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
    engs = {k: engine(sph, args.edge, nevery) for k, nevery in KINDS.items()}
    for eng in engs.values():
        eng.run(args.warmup)
        eng.sync()
    wall = {k: [] for k in KINDS}
    integ = {k: [] for k in KINDS}
    for timed in (False, True):
        for _ in range(args.rounds):
            for k, eng in engs.items():
                if timed:
                    eng.set_timing(True, classes=(eng.T_INT,))
                eng.sync()
                t0 = time.perf_counter()
                eng.run(args.steps)
                eng.sync()
                dt = time.perf_counter() - t0
                if timed:
                    integ[k].append(eng.stats()["ms_integrate"] / args.steps)
                    eng.set_timing(False)
                else:
                    wall[k].append(1e3 * dt / args.steps)
    out = {"atoms": args.edge ** 3, "steps": args.steps, "warmup": args.warmup,
           "rounds": args.rounds}
    x0 = engs["plain"].get_atoms()["x"]
    for k in KINDS:
        st = engs[k].dt_stats()
        out[k] = dict(wall_ms_per_step=summary(wall[k]), integrate_ms_per_step=summary(integ[k]),
                      dt=st["dt"], changes=st["changes"],
                      same_bits_as_plain=bool(engs[k].get_atoms()["x"].tobytes() == x0.tobytes()))
    for k in ("every1", "every10"):
        out[k + "_wall_over_plain"] = (out[k]["wall_ms_per_step"]["median"] /
                                       out["plain"]["wall_ms_per_step"]["median"])
        out[k + "_integrate_extra_ms"] = (out[k]["integrate_ms_per_step"]["median"] -
                                          out["plain"]["integrate_ms_per_step"]["median"])
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
