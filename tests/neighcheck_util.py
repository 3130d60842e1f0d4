"""neigh_modify every / delay / check on the oracle side, shared by test_neighcheck_cpu.py and
test_gpu_neighcheck.py.

pyoracle.RefRun.run and MpRefRun._run decide a rebuild with `(step - last_build) % every == 0`
inside their loops and offer no hook, so the two loops are restated here step for step
(pyoracle.py:866-890 and :1638-1655) with only that line replaced by Neighbor::decide
(neighbor.cpp:1332-1410); test_neighcheck_cpu.py pins the restatement, with check off, to the
unmodified loops bit for bit.  The mixins sit over RefRun, MpRefRun and the forced / gas
oracles of forcefix_util.py and idealgas_util.py.

nm = (every, delay, check) or None (every = ph.every, delay 0, check no: the oracle's own
rule).  Every run records build_steps (setup's 0 included), ndanger, eligible_steps, and per
displacement check (step, rsq / deltasq of every atom)."""
import dataclasses
import functools

import numpy as np

import pyoracle as po
from forcefix_util import ForcedMpRefRun, ForcedRefRun, wrapped
from idealgas_util import GasRefRun, shock_tube_case
from mp_variants_util import mp_box, mp_physics
from scenarios import bubble_physics, bubble_system, c2_system, c3_system


class _NeighCheck:
    nm = None

    def _nm(self):
        if self.nm is None:
            return int(self.ph.every), 0, False
        every, delay, check = self.nm
        return int(every), int(delay), bool(check)

    def setup(self):
        self.ago = 0
        self.build_steps, self.eligible_steps, self.checks = [], [], []
        self.ndanger = 0
        super().setup()

    def _build(self):
        super()._build()
        # Neighbor::build (neighbor.cpp:1428-1441): xhold = x of the owned atoms after the pbc
        # wrap, ago = 0
        self.xhold = self.s.x.copy()
        self.ago = 0
        self.build_steps.append(self.step)

    def _decide(self):
        """Neighbor::decide (neighbor.cpp:1332-1347) and check_distance (:1385-1410) of a step
        that no fix forces to reneighbor; the box is fixed, so deltasq = triggersq"""
        every, delay, check = self._nm()
        self.ago += 1
        if not (self.ago >= delay and self.ago % every == 0):
            return False
        self.eligible_steps.append(self.step)
        if not check:
            return True
        x, xh = self.s.x, self.xhold
        delx, dely, delz = x[:, 0] - xh[:, 0], x[:, 1] - xh[:, 1], x[:, 2] - xh[:, 2]
        rsq = delx * delx + dely * dely + delz * delz
        deltasq = 0.25 * self.ph.skin * self.ph.skin
        self.checks.append((self.step, rsq / deltasq if deltasq > 0 else np.where(rsq > 0, np.inf, 0.0)))
        flag = bool((rsq > deltasq).any())
        if flag and self.ago == max(every, delay):
            self.ndanger += 1
        return flag

    @property
    def check_max(self):
        """per check: the largest rsq / deltasq"""
        return [float(r.max()) for _, r in self.checks]


class _NeighCheckRef(_NeighCheck):
    def run(self, nsteps):   # pyoracle.py:866-890, the decision at :877 replaced
        s, L = self.s, po.lib()
        mm, sm = self._meso_mask(), self.ph.stationary_mask
        for _ in range(nsteps):
            self.step += 1
            if mm or not sm:
                L.orc_meso_initial_g(s.n, self.ph.dt, self.dtf, s.type, mm, s.mass, None, s.x,
                                     s.v, self.f, self.vest, s.rho, self.drho, s.e, self.de)
            if sm:
                L.orc_meso_stationary(s.n, self.dtf, s.type, sm, s.rho, self.drho, s.e,
                                      self.de)
            if self._decide():
                self._build()
                self.last_build = self.step
            else:
                self._forward()
            self._force()
            if mm or not sm:
                L.orc_meso_final_g(s.n, self.dtf, s.type, mm, s.mass, None, s.v, self.f,
                                   s.rho, self.drho, s.e, self.de)
            if sm:
                L.orc_meso_stationary(s.n, self.dtf, s.type, sm, s.rho, self.drho, s.e,
                                      self.de)
        for a in self.alts:
            a.run(nsteps)


class _NeighCheckMp(_NeighCheck):
    def _run(self, nsteps):   # pyoracle.py:1638-1655, the decision at :1645 replaced
        s, L, ph = self.s, po.lib(), self.ph
        for _ in range(nsteps):
            self.step += 1
            L.orc_meso_initial_g(s.n, ph.dt, self.dtf, s.type, 0, s.mass, s.rmass.ctypes.data,
                                 s.x, s.v, self.f, self.vest, s.rho, self.drho, s.e, self.de)
            # (a due fix phase_change is must_check: decide() returns before ago counts)
            pc_due = ph.pc is not None and self.step == self.next_pc
            if pc_due or self._decide():
                if pc_due:
                    self._phase_change()
                    self.next_pc += int(ph.pc.get("nevery", 1))
                self._build()
                self.last_build = self.step
            else:
                self._forward()
            self._force()
            L.orc_meso_final_g(s.n, self.dtf, s.type, 0, s.mass, s.rmass.ctypes.data, s.v,
                               self.f, s.rho, self.drho, s.e, self.de)


class NcRefRun(_NeighCheckRef, po.RefRun):
    pass


class NcForcedRefRun(_NeighCheckRef, ForcedRefRun):
    pass


class NcGasRefRun(_NeighCheckRef, GasRefRun):
    pass


class NcMpRefRun(_NeighCheckMp, po.MpRefRun):
    pass


class NcForcedMpRefRun(_NeighCheckMp, ForcedMpRefRun):
    pass


def neigh_oracle(cls, s, ph, nm, shadows=True, planar=True, builds=False, fixes=None, **kw):
    """cls(s, ph, **kw) deciding by nm, with check_fields' shadow runs attached as
    forcefix_util.forced_oracle attaches them: two row reorderings, the one-ulp input, and for
    a lattice C5 input (builds) the same source in its two other builds; every shadow decides
    by nm on its own positions"""
    def make(sysm, **more):
        r = cls(sysm, ph, **kw)
        r.nm = nm
        if fixes is not None:
            r.fixes = tuple(fixes)
        for k, v in more.items():
            setattr(r, k, v)
        return r

    ref = make(s)
    if shadows:
        for how in po.SPREAD_ORDERS:
            ref.alts.append(make(s, rev=how))
        ref.alts.append(make(po.ulp_perturbed(s, planar=planar)))
        if builds:
            for b in ("fma", "fastmath"):
                ref.alts.append(make(s, build=b))
    return ref


# ---- scenarios ------------------------------------------------------------------------------
def drift_speed(skin, dt, cross):
    """the uniform speed that carries an atom skin/2 in `cross` steps: with cross = k - 0.5 the
    displacement first exceeds skin/2 at step k = ceil(skin / (2 v dt))"""
    return skin / (2.0 * cross * dt)


def with_drift(s, speed, axis=0):
    """the upper half of the box along its last dimension drifts along `axis` (a shear: the
    density stays what it was)"""
    d = s.dim - 1
    up = s.x[:, d] >= 0.5 * (s.boxlo[d] + s.boxhi[d])
    s.v[up, axis] += speed
    return s


def c2_drift(n=10, cross=None, dim=3, skin=0.3, h=3.0):
    s = wrapped(c2_system(n, dim=dim))
    ph = po.c2_physics(h)
    ph.skin = skin
    if cross is not None:
        with_drift(s, drift_speed(ph.skin, ph.dt, cross))
    return s, ph


def stationary_case():
    """C1-style mixed integrators: type 2 under fix meso/stationary with a velocity that would
    carry it past skin/2 in two steps were it integrated; type 1 drifts past it at step 4"""
    s = wrapped(c3_system(10))
    ph = po.c3_physics()
    ph.skin = 0.3
    ph.stationary_mask = 1 << 2
    s.v[s.type == 2] = 0.0
    s.v[s.type == 2, 1] = drift_speed(ph.skin, ph.dt, 1.5)
    s.v[s.type == 1, 0] += drift_speed(ph.skin, ph.dt, 3.5)
    return s, ph


def mp_drift(dim):
    s = mp_box(dim=dim)
    ph = dataclasses.replace(mp_physics(), skin=0.06)
    with_drift(s, drift_speed(ph.skin, ph.dt, 2.5))
    return s, ph


C5_NX = 8


def c5_pc_case():
    """the smallest C5 box with fix phase_change every 3 steps (due at 1, 4, 7) and a skin no
    atom crosses in the run: every build is the fix's, and ago restarts from each"""
    s = bubble_system(C5_NX)
    ph = bubble_physics(C5_NX, prob=0.5, Tt=-1.0, nevery=3)
    return s, dataclasses.replace(ph, skin=0.1 / C5_NX)


BRICKS_PG = (2, 1, 1)
BRICKS_G = -350.0


def bricks_case():
    """16x8x8 jittered, from rest (test_gpu_bricks.py: the reference's setup forces depend on
    the decomposition otherwise), C3 physics; the atoms of rank 1 (x >= 8) are type 2 and fall
    along -x under a body force on their type alone, so only rank 1 ever raises the flag and
    the atoms just above x = 8 migrate to rank 0"""
    n = 8
    a = wrapped(c3_system(n, seed=12345))
    b = wrapped(c3_system(n, seed=54321))
    x = np.concatenate([a.x, b.x + np.array([float(n), 0.0, 0.0])])
    N = x.shape[0]
    t = np.where(x[:, 0] >= float(n), 2, 1).astype(np.int32)
    rho_t, e_t = np.array([0.0, 1.0, 0.5]), np.array([0.0, 1.0, 2.0])
    boxhi = a.boxhi.copy()
    boxhi[0] = a.boxlo[0] + 2.0 * (a.boxhi[0] - a.boxlo[0])
    s = po.System(3, a.boxlo.copy(), boxhi, (1, 1, 1), x, np.zeros((N, 3)), t, rho_t[t].copy(),
                  e_t[t].copy(), np.ones(N), 2, a.mass.copy())
    ph = po.c3_physics()
    ph.skin = 0.02
    ph.gravity = (BRICKS_G, 0.0, 0.0)
    ph.gravity_mask = 1 << 2
    return s, ph


# name -> (builder of (cls, s, ph, kw), nm, steps); the GPU tests run exactly these
def _c2(cross):
    return lambda: (NcRefRun,) + c2_drift(10, cross) + ({},)


def _shock():
    s, ph, fixes = shock_tube_case()
    assert ph.skin == 0.5
    return NcGasRefRun, s, ph, dict(fixes=fixes)


CASES = {
    "c2_every5": (_c2(6.5), (5, 0, 1), 22),
    "c2_every1": (_c2(6.5), (1, 0, 1), 16),
    "c2_delay5": (_c2(3.5), (1, 5, 1), 9),
    "c2_delay_nocheck": (_c2(6.5), (2, 4, 0), 11),
    "c2_still": (_c2(None), (5, 0, 1), 12),
    "c2_default": (_c2(6.5), None, 12),
    "shock_tube": (_shock, (5, 0, 1), 40),
    "stationary": (lambda: (NcRefRun,) + stationary_case() + ({},), (1, 0, 1), 9),
    "mp_3d": (lambda: (NcMpRefRun,) + mp_drift(3) + ({},), (1, 0, 1), 7),
    "mp_2d": (lambda: (NcMpRefRun,) + mp_drift(2) + ({},), (1, 0, 1), 7),
    "c5_pc": (lambda: (NcMpRefRun,) + c5_pc_case() + (dict(builds=True, planar=False),),
              (2, 0, 1), 8),
    "bricks": (lambda: (NcRefRun,) + bricks_case() + ({},), (5, 0, 1), 22),
}

# the schedules worked out by hand from the constructions above: builds (setup's 0 first),
# dangerous builds, eligible steps
EXPECTED = {
    # crossing at step 7 after each build, off the every-5 grid: eligible 5 10 15 20
    "c2_every5": ([0, 10, 20], 0, [5, 10, 15, 20]),
    # every step is eligible; a build at ago == 1 would be dangerous, these come at ago == 7
    "c2_every1": ([0, 7, 14], 0, list(range(1, 17))),
    # crossing at step 4, first eligible at ago == 5 == max(every, delay): dangerous
    "c2_delay5": ([0, 5], 1, [5]),
    # check no: ago >= 4 && ago % 2 == 0
    "c2_delay_nocheck": ([0, 4, 8], 0, [4, 8]),
    # thermal motion alone: 12 steps x 1e-3 x ~0.04 << 0.15
    "c2_still": ([0], 0, [5, 10]),
    "c2_default": ([0, 10], 0, [10]),
    # type 1 crosses at step 4, 8; the stationary type would at 2 if it moved
    "stationary": ([0, 4, 8], 0, list(range(1, 10))),
    "mp_3d": ([0, 3, 6], 0, list(range(1, 8))),
    "mp_2d": ([0, 3, 6], 0, list(range(1, 8))),
    # fix phase_change due at 1 4 7; ago restarts there, so the checks fall on 3 and 6
    "c5_pc": ([0, 1, 4, 7], 0, [3, 6]),
}


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    make, nm, steps = CASES[name]
    cls, s, ph, kw = make()
    return cls, s, ph, kw, nm, steps


@functools.lru_cache(maxsize=None)
def oracle_for(name, shadows=True):
    """the case's oracle after setup() and run(steps), computed once per session; tests read
    it and leave it as it is"""
    cls, s, ph, kw, nm, steps = case_inputs(name)
    kw = dict(kw)
    if not shadows:
        kw.pop("builds", None)
    ref = neigh_oracle(cls, s, ph, nm, shadows=shadows, **kw)
    ref.setup()
    ref.run(steps)
    return ref


def single_engine(sph, s, ph, path=0, every=None, **kw):
    """a single-phase engine for a po.Physics case (atoms set, before setup)"""
    if ph.rhosum_nstep > 0:
        kw["rhosum"] = dict(nstep=ph.rhosum_nstep, cut=ph.rhosum_cut)
    if ph.tait:
        kw["tait"] = dict(rho0=ph.rho0, c0=ph.c0, visc=ph.visc, cut=ph.tait_cut, morris=ph.morris)
    if ph.heat:
        kw["heat"] = dict(alpha=ph.alpha, cut=ph.heat_cut)
    sel = kw.pop("sel", None)
    cfg = sph.make_config(s.dim, s.ntypes, s.boxlo, s.boxhi, s.periodic, s.mass, ph.skin, ph.dt,
                          neigh_every=every or ph.every, kernel_path=path,
                          stationary_mask=ph.stationary_mask, gravity=ph.gravity,
                          gravity_mask=ph.gravity_mask, **kw)
    eng = sph.Engine(cfg)
    if sel is None:
        eng.set_atoms(s.x, s.v, s.type, s.rho, s.e, s.cv)
    else:
        eng.set_atoms(s.x[sel], s.v[sel], s.type[sel], s.rho[sel], s.e[sel], s.cv[sel])
        eng.set_tags(np.asarray(sel, dtype=np.int32))
    return eng
