#!/usr/bin/env python3
"""Cost of the sph/idealgas force pass against the two passes it is built beside.

    python tools/idealgas_cost.py [--edge 100] [--out profiles/idealgas/idealgas_cost.json]

One type on bench.py's C2 lattice (edge^3 atoms, h = 3, rhosum every step, rebuild every 10),
three engines on the same box in one session:
  gas    sph/rhosum + sph/idealgas (visc 0.5, e = 2.5, gas_box's physics)
  tait   sph/rhosum + sph/taitwater (C2; the 64-byte image, 6 waves per SIMD)
  heat   sph/rhosum + sph/taitwater/morris + sph/heatconduction (the other 80-byte image)
Each runs `warmup` steps once; then the three alternate, `rounds` times `steps` steps each,
with the event timers on the force class alone (class 1, which times all three passes).
Prints, and writes to --out, per engine the force pass's ms per step of every round, the
median and the range, and the ratios of the gas median to the other two."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from __graft_entry__ import _import_pkg  # noqa: E402


def tables(v):
    cut = np.zeros((2, 2))
    cut[1, 1] = 3.0
    t = np.zeros((2, 2))
    t[1, 1] = v
    return t, cut


def engine(sph, n, kind):
    x, v, t, rho, e, cv = bench.make_system(n, 12345)
    e = np.full_like(rho, 2.5)
    visc, cut = tables(0.5 if kind == "gas" else 0.1)
    kw = dict(rhosum=dict(nstep=1, cut=cut))
    if kind != "gas":
        kw["tait"] = dict(rho0=np.array([0.0, 1.0]), c0=np.array([0.0, 10.0]), visc=visc,
                          cut=cut, morris=kind == "heat")
    if kind == "heat":
        kw["heat"] = dict(alpha=tables(0.1)[0], cut=cut)
    cfg = sph.make_config(3, 1, [0.0] * 3, [float(n)] * 3, [1, 1, 1], [0.0, 1.0], 0.3, 1e-3,
                          neigh_every=10, **kw)
    eng = sph.Engine(cfg)
    if kind == "gas":
        eng.idealgas(visc, cut)
    eng.set_atoms(x, v, t, rho, e, cv)
    eng.setup()
    return eng


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--edge", type=int, default=100)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sph = _import_pkg()
    kinds = ("gas", "tait", "heat")
    engs = {k: engine(sph, args.edge, k) for k in kinds}
    for eng in engs.values():
        eng.run(args.warmup)
        eng.sync()
    ms = {k: [] for k in kinds}
    for _ in range(args.rounds):
        for k in kinds:
            eng = engs[k]
            eng.set_timing(True, classes=(eng.T_TAIT,))
            eng.run(args.steps)
            eng.sync()
            st = eng.stats()
            assert st["staged"] == 1 and st["n_tait"] == args.steps
            ms[k].append(st["ms_tait"] / args.steps)
            eng.set_timing(False)
    out = {"atoms": args.edge ** 3, "steps": args.steps, "warmup": args.warmup,
           "rounds": args.rounds}
    for k in kinds:
        out[k] = dict(ms_per_step=ms[k], median=statistics.median(ms[k]), min=min(ms[k]),
                      max=max(ms[k]))
    out["gas_over_tait"] = out["gas"]["median"] / out["tait"]["median"]
    out["gas_over_heat"] = out["gas"]["median"] / out["heat"]["median"]
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
