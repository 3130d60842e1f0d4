"""Thermo pressure, pair virial and gravity energy on the oracle side, shared by
test_thermo_cpu.py and test_gpu_thermo.py.

The reference's newton-on run prints the fdotr virial (Verlet passes vflag = 2, Pair::ev_setup
turns it into vflag_fdotr, virial_fdotr_compute sums x . f over owned and ghost atoms before
reverse comm: pair.cpp:1403-1420), which for a pair force along del is each pair's
del (x) del fpair once.  The oracle states that as the pair tally of its half list
(po.taitwater(virial=True): Pair::ev_tally, pair.cpp:770-850, each pair once under newton);
sph/idealgas' restatement tallies twice as PairSPHIdealGas::compute does (:164-169) and is
halved here.  The runs below keep, at every force pass: `virial` (the tally), `fdotr` (x . f of
the same pass, owned + ghost, before reverse comm) and `vscale` (S_ab, the sum of the absolute
values of the tallied terms -- the scale of the 1e-10 bar).

sph/taitwater/morris adds velx * fvisc to the force, which is not along del: the fdotr form
then carries sum del_a vel_b fvisc on top of the tally (`fdotr_visc`); the engine tallies the
fpair part, as the pair tally does.
"""
import dataclasses
import functools
import json
import os

import numpy as np

import pyoracle as po
from idealgas_util import GasRefRun, K2, K3, np_idealgas, shock_tube_case
from scenarios import c3_system, water_collapse_physics

VTOL = 1e-10     # virial: per component, of S_ab
STOL = 1e-12     # egrav, ke, ke_tensor: of the sum of the terms' absolute values


# ---- the bar's scales -------------------------------------------------------------------------
def _pairs(nlocal, hoff, hnb):
    hoff = np.asarray(hoff, dtype=np.int64)
    i = np.repeat(np.arange(nlocal, dtype=np.int64), np.diff(hoff))
    return i, np.asarray(hnb[:hoff[-1]], dtype=np.int64)


def _six(dx, dy, dz, s):
    """sum over pairs of (xx yy zz xy xz yz) of del (x) del s"""
    return np.array([(dx * dx * s).sum(), (dy * dy * s).sum(), (dz * dz * s).sum(),
                     (dx * dy * s).sum(), (dx * dz * s).sum(), (dy * dz * s).sum()])


def _six_abs(dx, dy, dz, s):
    """S_ab: the same sums over the terms' absolute values"""
    return _six(np.abs(dx), np.abs(dy), np.abs(dz), np.abs(s))


def tait_pair_terms(dim, g, vest, rho, mass, rho0, c0, B, visc, cut, hoff, hnb, morris):
    """pair_sph_taitwater.cpp:117-178 / pair_sph_taitwater_morris.cpp:160-177 per pair of the
    half list in numpy: (delx, dely, delz, fpair, velx, vely, velz, fvisc) -- fvisc the Morris
    viscous factor (0 for Monaghan).  For the bar's scale and the Morris fdotr term only: the
    virial compared is the oracle's."""
    i, j = _pairs(g.nlocal, hoff, hnb)
    x, t = g.x, g.type
    it, jt = t[i], t[j]
    d = x[i] - x[j]
    rsq = (d * d).sum(1)
    h = np.asarray(cut, dtype=np.float64)[it, jt]
    keep = rsq < h * h
    i, j, it, jt, d, rsq, h = (a[keep] for a in (i, j, it, jt, d, rsq, h))
    ih = 1.0 / h
    wfd = h - np.sqrt(rsq)
    wfd = (K3 * wfd * wfd * ih ** 7) if dim == 3 else (K2 * wfd * wfd * ih ** 6)

    def eos(a, ty):
        q = rho[a] / rho0[ty]
        return B[ty] * (q ** 7 - 1.0) / (rho[a] * rho[a])

    vel = vest[i] - vest[j]
    dvdr = (d * vel).sum(1)
    mm = mass[it] * mass[jt]
    v = np.asarray(visc, dtype=np.float64)[it, jt]
    if morris:
        fvisc = 2 * v / (rho[i] * rho[j]) * mm * wfd
        fpair = -mm * (eos(i, it) + eos(j, jt)) * wfd
    else:
        mu = h * dvdr / (rsq + 0.01 * h * h)
        fv = np.where(dvdr < 0.0, -v * (c0[it] + c0[jt]) * mu / (rho[i] + rho[j]), 0.0)
        fpair = -mm * (eos(i, it) + eos(j, jt) + fv) * wfd
        fvisc = np.zeros_like(fpair)
    return d[:, 0], d[:, 1], d[:, 2], fpair, vel[:, 0], vel[:, 1], vel[:, 2], fvisc


def gas_pair_terms(dim, g, vest, rho, e, mass, visc, cut, hoff, hnb):
    """pair_sph_idealgas.cpp:94-144 per pair of the half list (np_idealgas' expressions), for
    the bar's scale only"""
    i, j = _pairs(g.nlocal, hoff, hnb)
    x, t = g.x, g.type
    it, jt = t[i], t[j]
    d = x[i] - x[j]
    rsq = (d * d).sum(1)
    h = np.asarray(cut, dtype=np.float64)[it, jt]
    keep = rsq < h * h
    i, j, it, jt, d, rsq, h = (a[keep] for a in (i, j, it, jt, d, rsq, h))
    ih = 1.0 / h
    wfd = h - np.sqrt(rsq)
    wfd = (K3 * wfd * wfd * ih ** 7) if dim == 3 else (K2 * wfd * wfd * ih ** 6)
    im, jm = mass[it], mass[jt]
    fi, fj = 0.4 * e[i] / im / rho[i], 0.4 * e[j] / jm / rho[j]
    ci, cj = np.sqrt(0.4 * e[i] / im), np.sqrt(0.4 * e[j] / jm)
    dvdr = (d * (vest[i] - vest[j])).sum(1)
    mu = h * dvdr / (rsq + 0.01 * h * h)
    v = np.asarray(visc, dtype=np.float64)[it, jt]
    fv = np.where(dvdr < 0.0, -v * (ci + cj) * mu / (rho[i] + rho[j]), 0.0)
    return d[:, 0], d[:, 1], d[:, 2], -im * jm * (fi + fj + fv) * wfd


def fdotr(g, f):
    """virial_fdotr_compute (pair.cpp:1403-1420): sum over owned + ghost atoms of
    x0 f0, x1 f1, x2 f2, x1 f0, x2 f0, x2 f1, from f before reverse comm"""
    x = g.x
    return np.array([(x[:, 0] * f[:, 0]).sum(), (x[:, 1] * f[:, 1]).sum(),
                     (x[:, 2] * f[:, 2]).sum(), (x[:, 1] * f[:, 0]).sum(),
                     (x[:, 2] * f[:, 0]).sum(), (x[:, 2] * f[:, 1]).sum()])


# ---- oracle runs that keep the virial of every force pass -----------------------------------
class _Thermo:
    """record(): the thermo sums of the current state, by step"""

    def _keep(self):
        self.vir_by_step = getattr(self, "vir_by_step", {})
        self.vir_by_step[self.step] = dict(virial=self.virial.copy(), fdotr=self.fdotr.copy(),
                                           fdotr_visc=self.fdotr_visc.copy(),
                                           vscale=self.vscale.copy())


class TaitThermoRun(_Thermo, po.RefRun):
    def _force(self):
        super()._force()
        s, g, ph = self.s, self.g, self.ph
        f, drho, de, vir = po.taitwater(s.dim, g, s.ntypes, 1, self.vest_all, self.rho_all,
                                        s.mass, ph.rho0, ph.c0, ph.visc, ph.tait_cut, self.hoff,
                                        self.hnb, morris=ph.morris, B=self.B, virial=True)
        dx, dy, dz, fp, vx, vy, vz, fv = tait_pair_terms(
            s.dim, g, self.vest_all, self.rho_all, s.mass, ph.rho0, ph.c0, self.B, ph.visc,
            ph.tait_cut, self.hoff, self.hnb, ph.morris)
        self.virial, self.fdotr = vir, fdotr(g, f)
        self.vscale = _six_abs(dx, dy, dz, fp)
        # the Morris shear term of x . f: del_a (vel_b fvisc), in fdotr's component order
        self.fdotr_visc = np.array([(dx * vx * fv).sum(), (dy * vy * fv).sum(),
                                    (dz * vz * fv).sum(), (dy * vx * fv).sum(),
                                    (dz * vx * fv).sum(), (dz * vy * fv).sum()])
        self.vscale_visc = np.array([np.abs(dx * vx * fv).sum(), np.abs(dy * vy * fv).sum(),
                                     np.abs(dz * vz * fv).sum(), np.abs(dy * vx * fv).sum(),
                                     np.abs(dz * vx * fv).sum(), np.abs(dz * vy * fv).sum()])
        self._keep()


class GasThermoRun(_Thermo, GasRefRun):
    def _force(self):
        super()._force()
        s, g, ph = self.s, self.g, self.ph
        f, drho, de, vir = np_idealgas(s.dim, g.nlocal, 1, g.x, g.type, self.vest_all,
                                       self.rho_all, self.e_all, s.mass, ph.gas_visc, ph.gas_cut,
                                       self.hoff, self.hnb, virial=True)
        dx, dy, dz, fp = gas_pair_terms(s.dim, g, self.vest_all, self.rho_all, self.e_all, s.mass,
                                        ph.gas_visc, ph.gas_cut, self.hoff, self.hnb)
        self.virial = 0.5 * vir      # (two ev_tally calls per pair: the fdotr value is one)
        self.fdotr = fdotr(g, f)
        self.fdotr_visc = np.zeros(6)
        self.vscale = _six_abs(dx, dy, dz, fp)
        self._keep()


def sums(ref, mvv2e=1.0, nktv2p=1.0):
    """egrav, ke, ke_tensor, volume and press of the oracle's current state with the bars'
    scales.  fix_gravity.cpp:272-291: egrav -= massone * (xacc x + yacc y + zacc z) over the
    fix's group; compute_temp.cpp:71-91 / compute_pressure.cpp:193-207: dof boltz t =
    sum m |v|^2 mvv2e, press = (that + virial trace) / (dim volume) * nktv2p; ke
    (compute_ke.cpp:56-75) = 0.5 sum m |v|^2 mvv2e"""
    s, ph = ref.s, ref.ph
    m = s.mass[s.type]
    gm = ph.gravity_mask
    ing = np.ones(s.n, bool) if gm == 0 else ((gm >> s.type) & 1).astype(bool)
    gx = s.x @ np.asarray(ph.gravity, dtype=np.float64)
    v = s.v
    ket = np.array([(m * v[:, a] * v[:, b]).sum() for a, b in
                    ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))]) * mvv2e
    kets = np.array([np.abs(m * v[:, a] * v[:, b]).sum() for a, b in
                     ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))]) * mvv2e
    ke = 0.5 * (m * (v * v).sum(1)).sum() * mvv2e
    prd = np.asarray(s.boxhi) - np.asarray(s.boxlo)
    vol = float(prd[0] * prd[1] * (prd[2] if s.dim == 3 else 1.0))
    w, ws = ref.virial, ref.vscale
    tr, trs = w[:s.dim].sum(), ws[:s.dim].sum()
    press = (2.0 * ke + tr) / (s.dim * vol) * nktv2p
    # the bar that follows from press' parts: 2 ke within STOL of itself (its terms are all
    # positive), each diagonal virial component within VTOL of its S_aa
    press_bar = (2.0 * STOL * ke + VTOL * trs) / (s.dim * vol) * abs(nktv2p)
    return dict(egrav=-(m * gx)[ing].sum(), egrav_scale=np.abs(m * gx)[ing].sum(), ke=ke,
                ke_tensor=ket, ke_tensor_scale=kets, volume=vol, press=press,
                press_bar=press_bar)


# ---- parity record (profiles/thermo/parity.json) --------------------------------------------------
_RATIOS = {}


def ratio(name, err, bar):
    """the worst error / bar of the check `name` (0 / 0 = 0), kept for dump_parity"""
    err, bar = np.abs(np.asarray(err, dtype=np.float64)), np.asarray(bar, dtype=np.float64)
    r = float(np.max(np.where(err == 0.0, 0.0, err / np.where(bar > 0, bar, 1e-300))))
    _RATIOS[name] = max(_RATIOS.get(name, 0.0), r)
    return r


def dump_parity():
    """SPH_THERMO_PARITY=<path>: the worst error / bar of every check of this session"""
    path = os.environ.get("SPH_THERMO_PARITY")
    if not path or not _RATIOS:
        return
    old = {}
    if os.path.exists(path):
        with open(path) as fh:
            old = json.load(fh).get("ratios", {})
    old.update(_RATIOS)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(dict(note="worst |error| / bar per check (<= 1 passes): virial components "
                            "against 1e-10 S_ab, egrav / ke / ke_tensor against 1e-12 of the "
                            "sum of |terms|, press against the bar of its parts",
                       ratios=dict(sorted(old.items()))), fh, indent=1)


# ---- scenarios --------------------------------------------------------------------------------
def uneq_physics(morris=False):
    """rhosum + taitwater[/morris] on two types with unequal cuts (11: 3.0, 12: 2.6, 22: 2.2)
    and per-pair viscosities; the list is rebuilt every 3 steps"""
    t = np.zeros((3, 3))
    t[1, 1], t[1, 2], t[2, 2] = 3.0, 2.6, 2.2
    t[2, 1] = t[1, 2]
    v = np.zeros((3, 3))
    v[1, 1], v[1, 2], v[2, 2] = 0.1, 0.07, 0.05
    v[2, 1] = v[1, 2]
    return po.Physics(every=3, rhosum_cut=t.copy(), morris=morris,
                      rho0=np.array([0.0, 1.0, 0.5]), c0=np.array([0.0, 10.0, 10.0]), visc=v,
                      tait_cut=t.copy())


def box3d():
    """the jittered periodic two-type box of test_gpu_fused_integrate.py: 1000 atoms"""
    s = c3_system(10)
    s.v = s.v * 30.0     # (approaching pairs with a viscous share that is not negligible)
    return s


def dam2d(nx=28, ny=18, wall=3, dx=0.01):
    """water_collapse in small: a 2-D non-periodic box (boundary f f p) lined with `wall`
    layers of resting boundary atoms (type 2, fix meso/stationary) around a block of water
    (type 1) filling the left two thirds, scenarios.water_collapse_physics with the example's
    h = 3 dx: rhosum on the water alone, gravity on type 1 only.  The water is jittered and
    moves (so ke and the viscous terms are not zero)."""
    ix, iy = np.meshgrid(np.arange(nx), np.arange(ny), indexing="xy")
    ix, iy = ix.ravel(), iy.ravel()
    bc = (ix < wall) | (ix >= nx - wall) | (iy < wall)
    water = ~bc & (ix < wall + 2 * (nx - 2 * wall) // 3)
    keep = bc | water
    n = int(keep.sum())
    x = np.zeros((n, 3))
    x[:, 0], x[:, 1] = (ix[keep] + 0.5) * dx, (iy[keep] + 0.5) * dx
    t = np.where(bc[keep], 2, 1).astype(np.int32)
    rng = np.random.default_rng(2718)
    w = t == 1
    x[w, :2] += rng.uniform(-0.1, 0.1, (int(w.sum()), 2)) * dx
    v = np.zeros((n, 3))
    v[w, :2] = rng.normal(0.0, 0.05, (int(w.sum()), 2))
    m = 1000.0 * dx * dx
    s = po.System(2, np.zeros(3), np.array([nx * dx, (ny + 6) * dx, 0.5 * dx]), (0, 0, 1), x, v,
                  t, np.full(n, 1000.0), np.zeros(n), np.ones(n), 2, np.array([0.0, m, m]))
    return s, water_collapse_physics(h=3 * dx)


@dataclasses.dataclass
class Case:
    name: str
    s: po.System
    ph: po.Physics
    fixes: tuple = ()
    gas: bool = False


def make_case(name):
    if name in ("monaghan", "morris"):
        return Case(name, box3d(), uneq_physics(morris=name == "morris"))
    if name == "rest":
        # atoms at rest under gravity: with two bricks the setup step's force pass sees a
        # neighbour across the brick face with its vest as borders() left it (0: Verlet::setup
        # runs borders before setup_pre_force), so only a start from rest has the one-brick
        # run's setup forces -- and from there its trajectory
        s = box3d()
        s.v[:] = 0.0
        return Case(name, s, dataclasses.replace(uneq_physics(), gravity=(0.3, -0.2, 0.1)))
    if name == "dam2d":
        s, ph = dam2d()
        return Case(name, s, ph)
    assert name == "shock"
    s, ph, fixes = shock_tube_case()
    return Case(name, s, ph, fixes, True)


CASES = ("monaghan", "morris", "rest", "dam2d", "shock")


@functools.lru_cache(maxsize=None)
def oracle_history(name, nsteps):
    """the case's oracle run, setup and nsteps single steps: per step the virial record
    (vir_by_step) and the thermo sums; computed once, shared, never changed"""
    c = make_case(name)
    if c.gas:
        ref = GasThermoRun(c.s, c.ph)
        ref.fixes = tuple(c.fixes)
    else:
        ref = TaitThermoRun(c.s, c.ph)
    ref.setup()
    hist = {0: dict(sums=sums(ref), sums2=sums(ref, MVV2E, NKTV2P), **ref.vir_by_step[0])}
    for k in range(1, nsteps + 1):
        ref.run(1)
        hist[k] = dict(sums=sums(ref), sums2=sums(ref, MVV2E, NKTV2P), **ref.vir_by_step[k])
    return hist


MVV2E, NKTV2P = 48.88821291 ** 2, 68568.415      # LAMMPS' `units real` values: non-trivial


def engine(sph, c, path=0, virial_every=None, **kw):
    """the case's engine, atoms set and fixes armed, before setup (kw: procgrid / rank / sel of
    neighcheck_util.single_engine)"""
    from forcefix_util import arm
    from idealgas_util import gas_engine
    from neighcheck_util import single_engine
    if c.gas:
        eng = gas_engine(sph, c.s, c.ph, path)
    else:
        eng = single_engine(sph, c.s, c.ph, path, **kw)
    arm(eng, c.fixes)
    if virial_every is not None:
        eng.virial_every(virial_every)
    return eng
