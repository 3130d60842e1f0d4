#!/usr/bin/env python3
"""Cost of the on-device group diagnostics at C5's own size, beside the copy-back they replace.

    python tools/moments_cost.py [--edge 159] [--out profiles/moments/moments_cost.json]

runs bench.py's C5 system (159^3 = 4.02M atoms, fix phase_change armed) a few steps and times,
host side (launches, the copy of the results and the stream synchronise included):
one Engine.moments call with four selections (the droplet's type, the liquid's, all atoms and
the far field outside a sphere: what bubble_on_wall's print line reads of its groups), one
Engine.gyration call with the same four about given centres, one of each with
SPH_MAX_MOMENTS selections, and a get_atoms + get_atoms_multiphase round trip."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.setmeso_cost import engine, step_ms  # noqa: E402
from __graft_entry__ import _import_pkg  # noqa: E402


def call_ms(fn, reps):
    fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) / reps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--edge", type=int, default=159)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sph = _import_pkg()
    n = args.edge
    out = {"atoms": n ** 3}
    eng = engine(sph, n, clamp=False)
    out["step_ms"] = step_ms(eng, args.warmup, args.steps)
    far = sph.sphere((0.5, 0.5, 0.5), 0.5 - 2.6 / n)
    four = [dict(types=[2]), dict(types=[1]), dict(), dict(noregion=far)]
    eight = four + [dict(region=far), dict(types=[2], region=far), dict(types=[1], region=far),
                    dict(types=[1], noregion=far)]
    mom = eng.moments(four)
    out["droplet_count"] = mom[0]["count"]
    for name, sels in (("4", four), ("8", eight)):
        m = eng.moments(sels)
        cm, mass = [r["xcm"] for r in m], [r["mass"] for r in m]
        out[f"moments{name}_call_ms"] = call_ms(lambda: eng.moments(sels), 20)
        out[f"gyration{name}_call_ms"] = call_ms(lambda: eng.gyration(sels, cm=cm, mass=mass), 20)
    out["copy_back_ms"] = call_ms(lambda: (eng.get_atoms(), eng.get_atoms_multiphase()), 3)
    eng.close()
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
