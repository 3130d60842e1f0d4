"""fix dt/reset on the oracle side, shared by test_dtreset_cpu.py and test_gpu_dtreset.py.

oracle/build_ref.sh does not compile fix_dt_reset.cpp, so FixDtReset::end_of_step
(fix_dt_reset.cpp:131-186) is restated here in numpy, left to right as the reference writes it,
one rounding per operation (numpy never contracts a product into a sum), and the two Verlet
loops (pyoracle.py:866-890 and :1638-1655) are restated once more with a per-step dt / dtf, the
way neighcheck_util.py restates them for Neighbor::decide; the mixins here sit on top of those,
so fix dt/reset and neigh_modify can be armed together.  test_dtreset_cpu.py pins the
restatement to the unmodified loops bit for bit.

A dt fix is a dict(nevery=N, tmin=None|t, tmax=None|t, xmax=x, types=None|[t..]) (None = NULL;
units box).  It is the last fix of the script: end_of_step reads v after the final integrate
and f after every post_force fix (gravity, setforce, addforce).  The oracle's units are lj:
ftm2v = 1."""
import functools

import numpy as np

import pyoracle as po
from forcefix_util import ForcedMpRefRun, ForcedRefRun, wrapped
from idealgas_util import GasRefRun, shock_tube_case
from mp_variants_util import mp_box, mp_physics
from neighcheck_util import BRICKS_PG, _NeighCheckMp, _NeighCheckRef, c2_drift
from neighcheck_util import bricks_case as nc_bricks_case
from scenarios import c2_system, c3_system, water_collapse_physics, water_collapse_system

BIG = 1.0e20   # fix_dt_reset.cpp:33


def np_dt_reset(v, f, massinv, group, xmax, ftm2v=1.0, detail=False):
    """fix_dt_reset.cpp:149-166 over all atoms at once -> (dt per atom, BIG outside the group;
    their minimum, BIG for an empty group).  detail: also the mask of the atoms whose dt the
    `delr > xmax` rescale (:164) changed."""
    v = np.asarray(v, dtype=np.float64)
    f = np.asarray(f, dtype=np.float64)
    massinv = np.asarray(massinv, dtype=np.float64)
    with np.errstate(all="ignore"):   # (the branches not taken divide by zero)
        vsq = v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2]          # :153
        fsq = f[:, 0] * f[:, 0] + f[:, 1] * f[:, 1] + f[:, 2] * f[:, 2]          # :154
        dtv = np.where(vsq > 0.0, xmax / np.sqrt(vsq), BIG)                      # :156
        dtf = np.where(fsq > 0.0,
                       np.sqrt(2.0 * xmax / (ftm2v * np.sqrt(fsq) * massinv)), BIG)  # :157
        dt = np.where(dtv < dtf, dtv, dtf)                                       # :158 MIN
        dtsq = dt * dt
        delx = dt * v[:, 0] + 0.5 * dtsq * massinv * f[:, 0] * ftm2v             # :160-162
        dely = dt * v[:, 1] + 0.5 * dtsq * massinv * f[:, 1] * ftm2v
        delz = dt * v[:, 2] + 0.5 * dtsq * massinv * f[:, 2] * ftm2v
        delr = np.sqrt(delx * delx + dely * dely + delz * delz)                  # :163
        resc = delr > xmax
        dt = np.where(resc, dt * (xmax / delr), dt)                              # :164
    group = np.asarray(group, dtype=bool)
    dt = np.where(group, dt, BIG)
    dtmin = float(dt.min()) if dt.size else BIG
    dtmin = dtmin if dtmin < BIG else BIG                                        # :147, :165
    if detail:
        return dt, dtmin, resc & group
    return dt, dtmin


def bounded(dt, tmin, tmax):
    """fix_dt_reset.cpp:170-171: MAX with tmin first, then MIN with tmax"""
    if tmin is not None:
        dt = dt if dt > tmin else tmin
    if tmax is not None:
        dt = dt if dt < tmax else tmax
    return dt


def massinv_of(s):
    return 1.0 / (s.rmass if s.rmass is not None else s.mass[s.type])            # :151-152


def group_of(s, types):
    return np.ones(s.n, dtype=bool) if types is None else np.isin(s.type, list(types))


def type_mask(types):
    return 0 if types is None else sum(1 << t for t in types)


class Clock:
    """Update::update_time (update.cpp:482-483), update->dt and the fix's laststep, replayed
    over a dt sequence: change(step, dt) where an end_of_step call found another dt"""

    def __init__(self, dt):
        self.dt, self.atime, self.atimestep, self.laststep, self.changes = dt, 0.0, 0, 0, 0

    def change(self, step, dt):
        if dt == self.dt:                                                        # :177
            return
        self.laststep = step                                                     # :179
        self.atime += (step - self.atimestep) * self.dt                          # update_time
        self.atimestep = step
        self.dt = dt
        self.changes += 1

    def time(self, step):
        return self.atime + (step - self.atimestep) * self.dt                    # thermo.cpp:1500

    def stats(self, step):
        return dict(dt=self.dt, time=self.time(step), laststep=self.laststep,
                    changes=self.changes)


class _DtReset:
    dtfix = None

    def setup(self):
        self.clock = Clock(float(self.ph.dt))
        self.dt = float(self.ph.dt)
        self.dtf = 0.5 * self.dt
        self.dt_steps = []     # the dt every step ran with
        self.eos = []          # per end_of_step: (step, raw minimum, its atom, rescaled?, dt)
        super().setup()
        self._end_of_step()    # FixDtReset::setup

    def _end_of_step(self):
        c = self.dtfix
        if c is None:
            return
        s = self.s
        dti, dtmin, resc = np_dt_reset(s.v, self.f, massinv_of(s), group_of(s, c.get("types")),
                                       c["xmax"], detail=True)
        k = int(np.argmin(dti))
        dt = bounded(dtmin, c.get("tmin"), c.get("tmax"))
        self.eos.append((self.step, dtmin, k, bool(resc[k]), dt))
        self.clock.change(self.step, dt)
        if dt != self.dt:
            self.dt = dt
            self.dtf = 0.5 * dt   # FixMeso::reset_dt (fix_meso.cpp:184-187), ftm2v = 1

    def _due(self):
        return self.dtfix is not None and self.step % int(self.dtfix.get("nevery", 1)) == 0

    def dt_stats(self):
        return self.clock.stats(self.step)

    def dt_spread(self):
        """per step: the largest distance of the shadow runs' dt from this run's"""
        mine = np.asarray(self.dt_steps)
        out = np.zeros_like(mine)
        for a in self.alts:
            out = np.maximum(out, np.abs(np.asarray(a.dt_steps) - mine))
        return out


class _DtResetRef(_DtReset):
    def run(self, nsteps):   # pyoracle.py:866-890 with ph.dt -> self.dt, and end_of_step
        s, L = self.s, po.lib()
        mm, sm = self._meso_mask(), self.ph.stationary_mask
        for _ in range(nsteps):
            self.step += 1
            self.dt_steps.append(self.dt)
            if mm or not sm:
                L.orc_meso_initial_g(s.n, self.dt, self.dtf, s.type, mm, s.mass, None, s.x,
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
            if self._due():   # Modify::end_of_step (modify.cpp:404-408, verlet.cpp:299)
                self._end_of_step()
        for a in self.alts:
            a.run(nsteps)


class _DtResetMp(_DtReset):
    def _run(self, nsteps):   # pyoracle.py:1638-1655 with ph.dt -> self.dt, and end_of_step
        s, L, ph = self.s, po.lib(), self.ph
        assert self.dtfix is None or ph.pc is None, "fix phase_change reads update->dt"
        for _ in range(nsteps):
            self.step += 1
            self.dt_steps.append(self.dt)
            L.orc_meso_initial_g(s.n, self.dt, self.dtf, s.type, 0, s.mass, s.rmass.ctypes.data,
                                 s.x, s.v, self.f, self.vest, s.rho, self.drho, s.e, self.de)
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
            if self._due():
                self._end_of_step()


class DtRefRun(_DtResetRef, _NeighCheckRef, po.RefRun):
    pass


class DtForcedRefRun(_DtResetRef, _NeighCheckRef, ForcedRefRun):
    pass


class DtGasRefRun(_DtResetRef, _NeighCheckRef, GasRefRun):
    pass


class DtMpRefRun(_DtResetMp, _NeighCheckMp, po.MpRefRun):
    pass


class DtForcedMpRefRun(_DtResetMp, _NeighCheckMp, ForcedMpRefRun):
    pass


def dt_oracle(cls, s, ph, dtfix, nm=None, shadows=True, planar=True, fixes=None, **kw):
    """cls(s, ph, **kw) with the dt fix (and neigh_modify nm, post_force fixes) armed, and
    check_fields' shadow runs -- two row reorderings and the one-ulp input -- built from the
    same class with the same fix: each resets its own dt from its own v and f"""
    def make(sysm, **more):
        r = cls(sysm, ph, **kw)
        r.dtfix, r.nm = dtfix, nm
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
    return ref


# ---- scenarios ------------------------------------------------------------------------------
# Each names its xmax and bounds outright; test_dtreset_cpu.py shows on the oracle that with
# them dt changes at (at least) every other step, stays strictly inside (tmin, tmax) there and
# that the rescale of :164 decides the minimum at least once.
def fast_c2(n=10, dim=3, scale=1.0, seed=102):
    """the C2 jittered lattice with gaussian velocities of its own (sigma 0.05 x scale)"""
    s = wrapped(c2_system(n, dim=dim))
    s.v[:, :dim] = np.random.default_rng(seed).normal(0.0, 0.05 * scale, (s.n, dim))
    return s


def _c2():
    return DtRefRun, fast_c2(10), po.c2_physics(), {}


def _c3():
    return DtRefRun, wrapped(c3_system(8)), po.c3_physics(), {}


def _shock():
    s, ph, fixes = shock_tube_case()
    return DtGasRefRun, s, ph, dict(fixes=fixes)


def _mp():
    return DtMpRefRun, mp_box(dim=3), mp_physics(), {}


def _c2_check():
    s, ph = c2_drift(10, 6.5)
    return DtRefRun, s, ph, {}


WATER_V = 0.02


def water_moving():
    """the water_collapse fixture with a small random velocity on the water (type 1)"""
    s = water_collapse_system()
    w = s.type == 1
    s.v[w, :2] = np.random.default_rng(5).normal(0.0, WATER_V, (int(w.sum()), 2))
    return s


def _water():
    return DtRefRun, water_moving(), water_collapse_physics(), {}


def bricks_case():
    """neighcheck_util.bricks_case: 16x8x8 from rest (the reference's setup forces depend on
    the decomposition otherwise), the atoms of rank 1 (x >= 8, type 2) fall along -x under a
    body force on their type alone -- at setup their force, afterwards their speed sets the
    step, so rank 0 can only learn it from rank 1"""
    return nc_bricks_case()


def _bricks():
    s, ph = bricks_case()
    return DtRefRun, s, ph, {}


# name -> (builder of (cls, s, ph, kw), dt fix, nm, steps)
CASES = {
    "c2": (_c2, dict(nevery=1, tmin=1e-4, tmax=2e-3, xmax=1.5e-4), None, 20),
    "c2_every3": (_c2, dict(nevery=3, tmin=1e-4, tmax=2e-3, xmax=1.5e-4), None, 20),
    "c3": (_c3, dict(nevery=1, tmin=None, tmax=2e-3, xmax=5e-5), None, 20),
    "shock": (_shock, dict(nevery=1, tmin=1e-3, tmax=0.1, xmax=2e-3), None, 20),
    "mp": (_mp, dict(nevery=1, tmin=1e-4, tmax=4e-3, xmax=2e-4), None, 20),
    "c2_check": (_c2_check, dict(nevery=1, tmin=1e-4, tmax=2e-3, xmax=2e-2), (1, 0, 1), 16),
    "c2_check_every3": (_c2_check, dict(nevery=3, tmin=1e-4, tmax=2e-3, xmax=2e-2), (1, 0, 1), 16),
    "water": (_water, dict(nevery=1, tmin=None, tmax=3e-4, xmax=1e-5), (5, 0, 0), 20),
    "bricks": (_bricks, dict(nevery=1, tmin=1e-5, tmax=2e-3, xmax=6.3e-5), None, 12),
}


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    make, dtfix, nm, steps = CASES[name]
    cls, s, ph, kw = make()
    return cls, s, ph, kw, dtfix, nm, steps


@functools.lru_cache(maxsize=None)
def oracle_for(name, shadows=True):
    """the case's oracle after setup() and run(steps), computed once per session; tests read
    it and leave it as it is"""
    cls, s, ph, kw, dtfix, nm, steps = case_inputs(name)
    ref = dt_oracle(cls, s, ph, dtfix, nm=nm, shadows=shadows, **kw)
    ref.setup()
    ref.run(steps)
    return ref


def arm_dt(eng, dtfix):
    eng.dt_reset(dtfix.get("nevery", 1), dtfix.get("tmin"), dtfix.get("tmax"), dtfix["xmax"],
                 type_mask(dtfix.get("types")))
