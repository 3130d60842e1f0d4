"""fix setforce / fix addforce and fix ave/spatial's layers on the oracle side, shared by
test_forcefix_cpu.py and test_gpu_forcefix.py: the reference's post_force loops and layer rule
restated in numpy, oracle runs that apply them where LAMMPS runs post_force (after the pair
compute and its reverse comm, setup included), and the scenarios both files use.

A force fix is a dict(kind="set"|"add", value=(fx, fy, fz), per_mass=False, every=1,
types=None|[t..], region=R | noregion=R, tally=False); a None component of a "set" is NULL.
R = sph_amd.sphere(...) | sph_amd.block(...): the arguments of Engine.setforce / addforce."""
import dataclasses
import math

import numpy as np

import pyoracle as po
from mp_variants_util import mp_box, mp_physics
from scenarios import c3_system
from setmeso_util import apply_clamps, bubble_case, np_selected

BIG = 1.0e20   # an open side of a block (LAMMPS' INF)


def atom_mass(s):
    """rmass of atom_style meso/multiphase, else mass[type]"""
    return s.rmass if s.rmass is not None else s.mass[s.type]


def apply_forcefixes(run, fixes):
    """FixSetForce::post_force (fix_setforce.cpp:241-251) and FixAddForce::post_force
    (fix_addforce.cpp:238, 269-282), constant style, in the order given, on an oracle run's
    tag-ordered f.  per_mass: the atom-style variable mass*g is evaluated on its own, then
    added.  Keeps, per fix, what the last application found: run.ff_sel[k] (the selection),
    run.ff_pre[k] (f of all atoms just before the fix), and run.ff_applied (step, k) pairs."""
    s = run.s
    f = run.f
    for name in ("ff_sel", "ff_pre"):
        if not hasattr(run, name):
            setattr(run, name, {})
    if not hasattr(run, "ff_applied"):
        run.ff_applied = []
    for k, c in enumerate(fixes):
        if run.step % c.get("every", 1):
            continue
        m = np_selected(c, s.x, s.type)
        run.ff_sel[k] = m
        run.ff_pre[k] = f.copy()
        run.ff_applied.append((run.step, k))
        for d, v in enumerate(c["value"]):
            if c["kind"] == "set":
                if v is not None:
                    f[m, d] = v
            elif c.get("per_mass"):
                f[m, d] += atom_mass(s)[m] * v
            else:
                f[m, d] += v


def foriginal(run, k):
    """the fix's foriginal force sums of its last application, and sum |f| over the selection"""
    pre = run.ff_pre[k][run.ff_sel[k]]
    return (np.array([math.fsum(pre[:, d]) for d in range(3)]),
            math.fsum(np.abs(pre).ravel()))


class _Forced:
    clamps = ()
    fixes = ()

    def _force(self):   # (post_force: the clamps touch other fields, their order is immaterial)
        super()._force()
        apply_clamps(self, self.clamps)
        apply_forcefixes(self, self.fixes)


class ForcedMpRefRun(_Forced, po.MpRefRun):
    pass


class ForcedRefRun(_Forced, po.RefRun):
    pass


def forced_oracle(s, ph, fixes, clamps=(), procgrid=None, shadows=True, builds=True):
    """The oracle run with the fixes (and setmeso clamps) armed, and check_fields' shadow runs
    -- two reorderings, one ulp, and for a lattice input (builds) the FMA build -- every one of
    them with the fixes armed too."""
    mp = isinstance(ph, po.MpPhysics)

    def make(sysm):
        r = (ForcedMpRefRun(sysm, ph, procgrid=procgrid) if mp else ForcedRefRun(sysm, ph))
        r.fixes, r.clamps = tuple(fixes), tuple(clamps)
        return r

    ref = make(s)
    if shadows:
        for how in po.SPREAD_ORDERS:
            a = make(s)
            a.rev = how
            ref.alts.append(a)
        ref.alts.append(make(po.ulp_perturbed(s, planar=not builds)))
        if mp and builds:
            a = make(s)
            a.build = "fma"
            ref.alts.append(a)
    return ref


def arm(eng, fixes):
    """the fixes on an engine, in order -> their ids"""
    ids = []
    for c in fixes:
        kw = dict(types=c.get("types"), region=c.get("region"), noregion=c.get("noregion"),
                  tally=c.get("tally", False))
        if c["kind"] == "set":
            ids.append(eng.setforce(*c["value"], **kw))
        else:
            ids.append(eng.addforce(*c["value"], per_mass=c.get("per_mass", False),
                                    every=c.get("every", 1), **kw))
    return ids


def fix_region(c):
    return c.get("region") if c.get("region") is not None else c.get("noregion")


# ---- layers (fix ave/spatial) ---------------------------------------------------------------
def np_layer(c, lo, delta, nlayers, boxlo, boxhi, periodic):
    """fix_ave_spatial.cpp:1006-1013: the coordinate remapped once into a periodic box, then
    (int)((c - lo) * (1 / delta)) clamped to [0, nlayers - 1]"""
    c = np.array(c, dtype=np.float64)
    if periodic:
        prd = boxhi - boxlo
        c = np.where(c < boxlo, c + prd, c)
        c = np.where(c >= boxhi, c - prd, c)
    b = np.trunc((c - lo) * (1.0 / delta))
    return np.clip(b, 0, nlayers - 1).astype(np.int64)


def boundary_distance(c, lo, delta, nlayers):
    """distance of every coordinate to the nearest layer boundary lo + k delta"""
    t = (np.asarray(c) - lo) / delta
    return np.abs(t - np.rint(t)) * delta


# ---- scenarios ------------------------------------------------------------------------------
def wrapped(s):
    """positions wrapped into the periodic box beforehand, so that the first rebuild's pbc
    leaves an atom that never moves bit for bit where it was"""
    for d in range(s.dim):
        L = s.boxhi[d] - s.boxlo[d]
        s.x[:, d] = np.where(s.x[:, d] < s.boxlo[d], s.x[:, d] + L, s.x[:, d])
        s.x[:, d] = np.where(s.x[:, d] >= s.boxhi[d], s.x[:, d] - L, s.x[:, d])
    return s


def c3_walls_system():
    """the jittered two-type C3 box (edge 8, 512 atoms), type 2 at rest: the frozen walls"""
    s = wrapped(c3_system(8))
    s.v[s.type == 2] = 0.0
    return s


C3_BLOCK = ((1.03, 1.03, 1.03), (5.07, 6.11, 4.9))
C3_SPHERE = ((4.0, 4.0, 4.0), 2.77)
C3_G = (0.5, -0.25, 0.0)
C3_ADD = (0.7, -0.4, 0.25)


def c3_walls_case(sph):
    """case 1: setforce 0 0 0 on the walls, setforce NULL 0 0 on the fluid inside a block, a
    constant addforce on the fluid inside a sphere, a per-mass body force on the fluid"""
    fixes = [
        dict(kind="set", value=(0.0, 0.0, 0.0), types=[2]),
        dict(kind="set", value=(None, 0.0, 0.0), types=[1], region=sph.block(*C3_BLOCK)),
        dict(kind="add", value=C3_ADD, types=[1], region=sph.sphere(*C3_SPHERE)),
        dict(kind="add", value=C3_G, per_mass=True, types=[1]),
    ]
    return c3_walls_system(), po.c3_physics(), fixes


ORDER_SET = (1.0, 2.0, 3.0)
ORDER_ADD = (0.1, 0.2, 0.3)


def order_case(sph, set_first):
    """case 2: a setforce in the block and an addforce in the sphere, which overlap"""
    a = dict(kind="set", value=ORDER_SET, region=sph.block(*C3_BLOCK))
    b = dict(kind="add", value=ORDER_ADD, region=sph.sphere(*C3_SPHERE))
    return c3_walls_system(), po.c3_physics(), [a, b] if set_first else [b, a]


def nevery_case(sph):
    """case 3: an addforce every 3 steps on the fluid outside the sphere"""
    fixes = [dict(kind="add", value=(0.9, 0.3, -0.6), every=3, types=[1],
                  noregion=sph.sphere(*C3_SPHERE))]
    return c3_walls_system(), po.c3_physics(), fixes


POISEUILLE_G = 0.5
POISEUILLE_DELTA = 0.9     # (neither box edge, 7 or 12, is a multiple of it)


def poiseuille_case(sph, dim):
    """case 4: mp_box with rhosum/multiphase + taitwater/multiphase alone, rebuilt every
    step; mass * g along x on type 1 below y = Ly/2 and mass * -g above it (poiseuille.lmp:
    57-58 as two half-box fixes), type 2 frozen"""
    s = mp_box(dim=dim)
    ph = dataclasses.replace(mp_physics(st=False, heat=False, cg_nstep=0), every=1)
    mid = 0.5 * (s.boxlo[1] + s.boxhi[1])
    lower = sph.block((-BIG, -BIG, -BIG), (BIG, mid, BIG))
    upper = sph.block((-BIG, mid, -BIG), (BIG, BIG, BIG))
    fixes = [
        dict(kind="add", value=(POISEUILLE_G, 0.0, 0.0), per_mass=True, types=[1], region=lower),
        dict(kind="add", value=(-POISEUILLE_G, 0.0, 0.0), per_mass=True, types=[1],
             region=upper),
        dict(kind="set", value=(0.0, 0.0, 0.0), types=[2]),
    ]
    return s, ph, fixes


BUOYANCY = (0.0, 40.0, 0.0)


def buoyancy_case(sph):
    """case 5: the C5 stack with fix phase_change and the far-field clamp
    (setmeso_util.bubble_case), buoyancy mass * g on the gas (bubble.lmp:188)"""
    s, ph, clamps, dx = bubble_case(sph, nx=10, pc=True)
    fixes = [dict(kind="add", value=BUOYANCY, per_mass=True, types=[2])]
    return s, ph, clamps, fixes, dx


BRICKS_PG = (2, 1, 1)


def bricks_case(sph):
    """case 6: the jittered three-style mp_box on 2x1x1 bricks (cut at x = 3.5); a tallying
    setforce in a sphere across the cut (the drag on a body), then a tallying body force"""
    s = mp_box(dim=3)
    ph = mp_physics()
    fixes = [
        dict(kind="set", value=(0.0, 0.0, 0.0), region=sph.sphere((3.5, 3.4, 3.6), 1.93),
             tally=True),
        dict(kind="add", value=(0.0, -0.4, 0.0), per_mass=True, types=[1], tally=True),
    ]
    return s, ph, fixes
