"""The oracle side of test_gpu_virial_variants.py: the block-path scenarios of
test_gpu_block_paths.py (PHYSICS / LONG) with velocities 30 times theirs, run once per case by
thermo_util.TaitThermoRun (the plain fp64 pair tally, po.taitwater(virial=True)) and kept at
the three steps the engine is read at: setup, step 1 and step every + 2 (one rebuild, at step
`every`, and two steps behind it).

Per kept step: the tally, S_ab (the bar's scale), thermo_util.sums, the longest full-list row,
the largest displacement since the last build and, for Monaghan viscosity, S_ab of the same
pairs with the viscosity taken out (how much of the tally the viscous term is).
"""
import dataclasses
import functools

import numpy as np

import pyoracle as po
from scenarios import c2_system
from test_gpu_block_paths import LONG, PHYSICS
from thermo_util import Case, TaitThermoRun, _pairs, _six_abs, sums, tait_pair_terms

VSCALE = 30.0                    # thermo_util.box3d's factor
GRAVITY = (0.3, -0.2, 0.1)       # three different components
NEVERY = 1000                    # virial_every(N), N larger than any run here

BLOCK, ROW = 0, 1


@dataclasses.dataclass(frozen=True)
class Spec:
    passes: tuple            # (kernel_path, SPH_TUNE_BLKUMF) per pass
    long: bool = False       # rows past the register preload: the NCH = 0 instantiations
    fuses: bool = False      # one type, taitwater alone: the block path fuses its inner steps
    monaghan: bool = False   # Monaghan viscosity with a coefficient: fpair has a viscous term
    gravity: bool = False
    inst: str = ""           # VISC, MODE, NT1 of the case's force pass (for the printed line)


# the issue's table, row for row
SPECS = {
    "c2": Spec(((BLOCK, 0), (BLOCK, 64), (ROW, 0)), fuses=True, monaghan=True, gravity=True,
               inst="MONAGHAN M_TAIT NT1"),
    "c2_novisc": Spec(((BLOCK, 0), (ROW, 0)), fuses=True, inst="BLK_VISC_NONE M_TAIT NT1"),
    "morris1": Spec(((BLOCK, 0), (ROW, 0)), fuses=True, inst="MORRIS M_TAIT NT1"),
    "morris1_heat": Spec(((BLOCK, 0), (BLOCK, 64), (ROW, 0)), inst="MORRIS M_TAIT|M_HEAT NT1"),
    "c3": Spec(((BLOCK, 0), (ROW, 0)), inst="MORRIS M_TAIT|M_HEAT two types"),
    "c2_2d": Spec(((BLOCK, 0), (ROW, 0)), fuses=True, monaghan=True,
                  inst="MONAGHAN M_TAIT NT1 2-D"),
    "c2_long": Spec(((BLOCK, 0), (BLOCK, 64)), long=True, fuses=True, monaghan=True,
                    inst="MONAGHAN M_TAIT NT1 NCH 0"),
    "c3_long": Spec(((BLOCK, 0),), long=True, inst="MORRIS M_TAIT|M_HEAT two types NCH 0"),
    "heat_only": Spec(((BLOCK, 0), (ROW, 0)), inst="M_HEAT two types (no force body)"),
}

VALUE_CASES = [(n, p, u) for n, sp in SPECS.items() if n != "heat_only" for p, u in sp.passes]
HEAT_ONLY_CASES = [("heat_only", p, u) for p, u in SPECS["heat_only"].passes]


def case_id(v):
    name, path, umf = v
    return f"{name}-{'row' if path else 'block'}" + (f"-umf{umf}" if umf else "")


def make_case(name):
    """(system, physics) of a named case: test_gpu_block_paths' scenario, v scaled"""
    s, ph, every, _ = {**PHYSICS, **LONG}[name]()
    ph.every = every
    s.v = s.v * VSCALE
    if SPECS[name].gravity:
        ph.gravity = GRAVITY
    return Case(name, s, ph)


def steps_of(ph):
    """the steps the engine is read at: setup, run(1), run(every + 1)"""
    return (0, 1, ph.every + 2)


class VariantRun(TaitThermoRun):
    """TaitThermoRun that tallies at the steps `at` alone (the steps between are RefRun's own,
    the same trajectory without the second pass and the numpy pair terms) and keeps there, for
    Monaghan viscosity, S_ab without the viscous term"""
    at = ()

    def _force(self):
        if self.step not in self.at:
            po.RefRun._force(self)
            return
        super()._force()
        s, g, ph = self.s, self.g, self.ph
        if not ph.morris and np.any(ph.visc):
            dx, dy, dz, fp = tait_pair_terms(
                s.dim, g, self.vest_all, self.rho_all, s.mass, ph.rho0, ph.c0, self.B,
                np.zeros_like(ph.visc), ph.tait_cut, self.hoff, self.hnb, False)[:4]
            self.vir_by_step[self.step]["vscale_novisc"] = _six_abs(dx, dy, dz, fp)


class HeatOnlyRun(po.RefRun):
    """heat conduction alone: no pair style with a force, so nothing is tallied (the engine's
    virial_fold() writes zeros); thermo_util.sums then gives press = its kinetic part with the
    bar 2 STOL ke / (dim volume)"""
    virial = np.zeros(6)
    vscale = np.zeros(6)


def _keep(ref, xb):
    h = dict(sums=sums(ref), nn_max=int(ref.numneigh_full().max()),
             moved=float(np.sqrt(((ref.s.x - xb) ** 2).sum(1)).max()))
    if isinstance(ref, TaitThermoRun):
        h.update(ref.vir_by_step[ref.step])
    for v in h.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return h


def _run(ref, at):
    """the run's record at setup and at the steps `at`"""
    ref.setup()
    xb = ref.s.x.copy()
    hist = {0: _keep(ref, xb)}
    for k in sorted(at):
        while ref.step < k:
            ref.run(1)
            if ref.last_build == ref.step:
                xb = ref.s.x.copy()
        hist[k] = _keep(ref, xb)
    return hist


@functools.lru_cache(maxsize=None)
def history(name):
    """the case's oracle run, computed once per session, shared by its passes, never changed"""
    c = make_case(name)
    ref = (VariantRun if c.ph.tait else HeatOnlyRun)(c.s, c.ph)
    ref.at = steps_of(c.ph)
    return _run(ref, ref.at[1:])


# ---- bricks -----------------------------------------------------------------------------------
BRICK_EVERY, BRICK_STEPS = 3, 5
BRICK_GRIDS = {(1, 2, 2): BLOCK, (2, 2, 2): ROW}     # processor grid -> pair path


def brick_case():
    """c2_system(12), one type, at rest under GRAVITY (thermo_util.make_case("rest") says why
    only a start from rest has the one-brick run's setup forces), rebuilt every 3 steps"""
    s = c2_system(12)
    s.v[:] = 0.0
    ph = po.c2_physics()
    ph.every = BRICK_EVERY
    ph.gravity = GRAVITY
    return Case("rest1", s, ph)


def face_pairs(ref, pg):
    """the pairs of the oracle's current half list, inside the cut, whose two atoms lie in
    different bricks of the grid pg (a ghost counts as the atom it images)"""
    s, g = ref.s, ref.g
    i, j = _pairs(g.nlocal, ref.hoff, ref.hnb)
    d = g.x[i] - g.x[j]
    h = float(np.asarray(ref.ph.tait_cut).max())
    inside = (d * d).sum(1) < h * h
    atom = np.concatenate([np.arange(g.nlocal), np.asarray(g.owner[:g.nghost], dtype=np.int64)])
    brick = po.brick_owner(s, s.x, pg)
    return int((inside & (brick[atom[i]] != brick[atom[j]])).sum())


@functools.lru_cache(maxsize=None)
def brick_history():
    c = brick_case()
    ref = VariantRun(c.s, c.ph)
    ref.at = (0, BRICK_STEPS)
    hist = _run(ref, ref.at[1:])
    hist[BRICK_STEPS]["face_pairs"] = {pg: face_pairs(ref, pg) for pg in BRICK_GRIDS}
    return hist
