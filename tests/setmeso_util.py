"""fix setmeso / setmesode on the oracle side, shared by the clamp and reduction tests: the
reference's region predicates and post_force clamps restated in numpy, oracle runs that
apply them where LAMMPS runs post_force, and the scenarios both test files use.

A clamp is a dict(what="rho"|"e"|"t"|"de", value, types=None|[t..], region=R | noregion=R)
with R = sph_amd.sphere(...) | sph_amd.block(...) -- the arguments of Engine.setmeso."""
import numpy as np

import pyoracle as po
from scenarios import bubble_physics, bubble_system, c3_system

TINF = 1.25   # the far field held hotter than the liquid's initial T = 1 (bubble.lmp:94-96)


def np_inside(r, x):
    """RegSphere::inside (region_sphere.cpp:96-105) / RegBlock::inside (region_block.cpp:
    114-119), closed boundaries"""
    if r.style == 0:
        dx, dy, dz = x[:, 0] - r.xc, x[:, 1] - r.yc, x[:, 2] - r.zc
        return np.sqrt(dx * dx + dy * dy + dz * dz) <= r.radius
    return ((x[:, 0] >= r.xlo) & (x[:, 0] <= r.xhi) & (x[:, 1] >= r.ylo) & (x[:, 1] <= r.yhi) &
            (x[:, 2] >= r.zlo) & (x[:, 2] <= r.zhi))


def np_match(r, x):
    """Region::match (region.cpp:127-131): !(inside ^ interior)"""
    return ~(np_inside(r, x) ^ bool(r.interior))


def np_selected(c, x, type_):
    """the atoms a clamp / reduction selection dict picks: group and region"""
    m = np.ones(x.shape[0], dtype=bool)
    if c.get("types") is not None:
        m &= np.isin(type_, np.atleast_1d(c["types"]))
    if c.get("region") is not None:
        m &= np_match(c["region"], x)
    if c.get("noregion") is not None:
        m &= ~np_match(c["noregion"], x)
    return m


def surface_distance(r, x):
    """distance of every atom to the region's surface (block: to its nearest face plane)"""
    if r.style == 0:
        d = x - np.array([r.xc, r.yc, r.zc])
        return np.abs(np.sqrt((d * d).sum(1)) - r.radius)
    lo = np.array([r.xlo, r.ylo, r.zlo])
    hi = np.array([r.xhi, r.yhi, r.zhi])
    return np.minimum(np.abs(x - lo), np.abs(x - hi)).min(1)


def clamp_region(c):
    return c.get("region") if c.get("region") is not None else c.get("noregion")


FIELD_OF = {"rho": "rho", "e": "e", "t": "e", "de": "de"}


def apply_clamps(run, clamps):
    """FixSetMeso::post_force (fix_setmeso.cpp:180-233) / FixSetMesodE::post_force
    (fix_setmesode.cpp:171-198), constant style, on an oracle run's tag-ordered arrays"""
    s = run.s
    for c in clamps:
        m = np_selected(c, s.x, s.type)
        if c["what"] == "rho":
            s.rho[m] = c["value"]
        elif c["what"] == "e":
            s.e[m] = c["value"]
        elif c["what"] == "t":
            s.e[m] = s.cv[m] * c["value"]
        else:
            run.de[m] = c["value"]


class _Clamped:
    clamps = ()

    def _force(self):   # (post_force follows the pair compute and its reverse comm, setup too)
        super()._force()
        apply_clamps(self, self.clamps)


class ClampedMpRefRun(_Clamped, po.MpRefRun):
    pass


class ClampedRefRun(_Clamped, po.RefRun):
    pass


def clamped_oracle(s, ph, clamps, procgrid=None, shadows=True):
    """The oracle run with the clamps armed; shadows: the reordering, one-ulp and (C5) FMA-build
    shadow runs of check_fields' bar, every one of them clamped too (the built-in
    spread=True shadows would be plain runs)."""
    mp = isinstance(ph, po.MpPhysics)

    def make(sysm):
        r = (ClampedMpRefRun(sysm, ph, procgrid=procgrid) if mp else ClampedRefRun(sysm, ph))
        r.clamps = tuple(clamps)
        return r

    ref = make(s)
    if shadows:
        for how in po.SPREAD_ORDERS:
            a = make(s)
            a.rev = how
            ref.alts.append(a)
        ref.alts.append(make(po.ulp_perturbed(s)))
        if mp:
            a = make(s)
            a.build = "fma"
            ref.alts.append(a)
    return ref


# ---- scenarios ----------------------------------------------------------------------------
def far_field(sph, nx, dim):
    """bubble.lmp:94-96: everything outside a sphere of radius 0.5 - 2.6 dx at the box centre"""
    dx = 1.0 / nx
    c = (0.5, 0.5, 0.5 if dim == 3 else 0.0)
    return sph.sphere(c, 0.5 - 2.6 * dx)


def bubble_case(sph, nx=10, dim=3, pc=False):
    """scenarios 1 / 2 / 4: the C5 stack with `fix setmeso meso_t TINF noregion sphere`"""
    s = bubble_system(nx, dim=dim)
    ph = (bubble_physics(nx, dim=dim, prob=0.5, Tt=-1.0) if pc
          else bubble_physics(nx, dim=dim, pc=False))
    clamps = [dict(what="t", value=TINF, noregion=far_field(sph, nx, dim))]
    return s, ph, clamps, 1.0 / nx


def c3_case(sph):
    """scenario 3: the jittered two-type C3 box (edge 8, spacing 1) with three fixes at once"""
    s = c3_system(8)
    ph = po.c3_physics()
    clamps = [
        dict(what="e", value=1.5, types=[2], region=sph.block((1.03, 1.03, 1.03), (5.07, 6.11, 4.9))),
        dict(what="de", value=0.0, types=[1], region=sph.sphere((4.0, 4.0, 4.0), 2.77, side="out")),
        dict(what="rho", value=0.8, region=sph.block((2.2, 2.3, 2.1), (4.4, 4.6, 4.3))),
    ]
    return s, ph, clamps, 1.0


def arm(eng, clamps):
    for c in clamps:
        eng.setmeso(c["what"], c["value"], types=c.get("types"), region=c.get("region"),
                    noregion=c.get("noregion"))


def c3_engine(sph, s, ph, path):
    cfg = sph.make_config(s.dim, s.ntypes, s.boxlo, s.boxhi, s.periodic, s.mass, ph.skin, ph.dt,
                          neigh_every=ph.every, kernel_path=path,
                          tait=dict(rho0=ph.rho0, c0=ph.c0, visc=ph.visc, cut=ph.tait_cut,
                                    morris=ph.morris),
                          heat=dict(alpha=ph.alpha, cut=ph.heat_cut))
    eng = sph.Engine(cfg)
    eng.set_atoms(s.x, s.v, s.type, s.rho, s.e, s.cv)
    return eng
