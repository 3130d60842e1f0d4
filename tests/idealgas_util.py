"""sph/idealgas on the oracle side, shared by test_idealgas_cpu.py and test_gpu_idealgas.py:
PairSPHIdealGas::compute (pair_sph_idealgas.cpp:48-175) restated in numpy over a half list in
list order and in the reference's operation order -- newton_pair, j < nlocal and the doubled
ev_tally included --, an oracle run whose force step is rhosum when due, that restatement,
reverse comm, gravity and the post_force fixes, and the scenarios both files use.

Per-pair terms are vectorised (numpy evaluates each expression left to right, one rounding
per operation, no contraction: the reference's x86-64 arithmetic); the accumulation into f,
drho and de walks the pairs in list order, i share then j share, so every atom receives its
terms in the reference's order."""
import dataclasses

import numpy as np

import pyoracle as po
from forcefix_util import _Forced

K3 = -25.066903536973515383e0   # Lucy kernel, 3-D (:121)
K2 = -19.098593171027440292e0   # 2-D (:124)


def np_idealgas(dim, nlocal, newton, x, type_, vest, rho, e, mass, visc, cut, hoff, hnb,
                virial=False, gather=False, absolute=False):
    """-> f (nall, 3), drho, de (nall) [, virial (6)] of one compute over the half list
    hoff/hnb (row r = owned atom r); all per-atom arrays over owned + ghost atoms; visc and cut
    (nt+1, nt+1), read as [itype][jtype] with i the row atom (init_one mirrors cut only).
    gather: hoff/hnb is a FULL list and every row keeps its own share only (no j share);
    absolute: the sums of the terms' absolute values instead (the scale of a cancelling sum)"""
    nall = x.shape[0]
    hoff = np.asarray(hoff, dtype=np.int64)
    i = np.repeat(np.arange(nlocal, dtype=np.int64), np.diff(hoff))
    j = np.asarray(hnb[:hoff[-1]], dtype=np.int64)
    it, jt = type_[i], type_[j]
    imass, jmass = mass[it], mass[jt]
    fi = 0.4 * e[i] / imass / rho[i]
    ci = np.sqrt(0.4 * e[i] / imass)
    delx, dely, delz = x[i, 0] - x[j, 0], x[i, 1] - x[j, 1], x[i, 2] - x[j, 2]
    rsq = delx * delx + dely * dely + delz * delz
    cutm = np.asarray(cut, dtype=np.float64)
    h = cutm[it, jt]
    keep = rsq < h * h                       # cutsq = cut * cut (pair.cpp init)
    i, j, it, jt, imass, jmass, fi, ci, delx, dely, delz, rsq, h = (
        a[keep] for a in (i, j, it, jt, imass, jmass, fi, ci, delx, dely, delz, rsq, h))
    ih = 1. / h
    ihsq = ih * ih
    wfd = h - np.sqrt(rsq)
    if dim == 3:
        wfd = K3 * wfd * wfd * ihsq * ihsq * ihsq * ih
    else:
        wfd = K2 * wfd * wfd * ihsq * ihsq * ihsq
    fj = 0.4 * e[j] / jmass / rho[j]
    dvdr = (delx * (vest[i, 0] - vest[j, 0]) + dely * (vest[i, 1] - vest[j, 1])
            + delz * (vest[i, 2] - vest[j, 2]))
    cj = np.sqrt(0.4 * e[j] / jmass)
    mu = h * dvdr / (rsq + 0.01 * h * h)
    v = np.asarray(visc, dtype=np.float64)[it, jt]
    fvisc = np.where(dvdr < 0., -v * (ci + cj) * mu / (rho[i] + rho[j]), 0.)
    fpair = -imass * jmass * (fi + fj + fvisc) * wfd
    deltaE = -0.5 * fpair * dvdr
    jside = np.ones(i.size, dtype=bool) if newton else j < nlocal
    if gather:
        jside = np.zeros(i.size, dtype=bool)
    # events in the reference's order: pair k's i share, then its j share
    npair = i.size
    tgt = np.empty(2 * npair, dtype=np.int64)
    tgt[0::2], tgt[1::2] = i, j
    on = np.ones(2 * npair, dtype=bool)
    on[1::2] = jside

    def scatter(vi, vj, width=None):
        ev = np.empty((2 * npair,) + (() if width is None else (width,)))
        ev[0::2], ev[1::2] = vi, vj
        if absolute:
            ev = np.abs(ev)
        out = np.zeros((nall,) + (() if width is None else (width,)))
        np.add.at(out, tgt[on], ev[on])      # (unbuffered: applied in index order)
        return out

    fv = np.stack([delx * fpair, dely * fpair, delz * fpair], axis=1)
    f = scatter(fv, -fv, 3)
    drho = scatter(jmass * dvdr * wfd, imass * dvdr * wfd)
    de = scatter(deltaE, deltaE)
    if not virial:
        return f, drho, de
    # Pair::ev_tally (pair.cpp:770-850), called twice per pair (:164-169)
    v6 = np.stack([delx * delx * fpair, dely * dely * fpair, delz * delz * fpair,
                   delx * dely * fpair, delx * delz * fpair, dely * delz * fpair], axis=1)
    if newton:
        ev = np.repeat(v6, 2, axis=0)
    else:
        half = 0.5 * v6
        ev = np.zeros((4 * npair, 6))
        for c in (0, 2):
            ev[c::4] = np.where((i < nlocal)[:, None], half, 0.0)
            ev[c + 1::4] = np.where((j < nlocal)[:, None], half, 0.0)
    vir = np.zeros(6)
    for d in range(6):
        vir[d] = np.cumsum(ev[:, d])[-1] if ev.shape[0] else 0.0   # (in list order)
    return f, drho, de, vir


@dataclasses.dataclass
class GasPhysics(po.Physics):
    """hybrid/overlay sph/rhosum N sph/idealgas (rhosum_nstep 0: sph/idealgas alone)"""
    gas_visc: np.ndarray | None = None
    gas_cut: np.ndarray | None = None
    tait: bool = False

    def cutmax(self, nt):
        cm = super().cutmax(nt)
        g = np.asarray(self.gas_cut, dtype=np.float64)
        for i in range(nt + 1):
            for j in range(i, nt + 1):
                cm[i, j] = cm[j, i] = max(cm[i, j], g[i, j])
        return cm


class _GasRun(po.RefRun):
    def _force(self):
        s, g, ph = self.s, self.g, self.ph
        nt = s.ntypes
        g.x[:s.n] = s.x
        if ph.rhosum_nstep > 0 and self.step % ph.rhosum_nstep == 0:
            with np.errstate(all="ignore"):
                rho = po.rhosum(s.dim, g, nt, s.mass, ph.rhosum_cut, self.foff, self.fnb)
            upd = ~ph.rho_keep(nt)[s.type]
            s.rho[upd] = rho[upd]
            self.rho_all = g.gather(s.rho)       # forward_comm_pair
        f, drho, de = np_idealgas(s.dim, g.nlocal, 1, g.x, g.type, self.vest_all, self.rho_all,
                                  self.e_all, s.mass, ph.gas_visc, ph.gas_cut, self.hoff,
                                  self.hnb)
        po.reverse_comm(g, f, drho, de)
        if any(a != 0.0 for a in ph.gravity):    # post_force
            po.lib().orc_gravity(s.n, s.type, ph.gravity_mask, s.mass, None,
                                 np.asarray(ph.gravity, dtype=np.float64), f)
        self.f = f[:s.n].copy()
        self.drho = drho[:s.n].copy()
        self.de = de[:s.n].copy()
        self.e_min = min(getattr(self, "e_min", np.inf), float(s.e.min()))
        lo, hi = np.asarray(s.boxlo), np.asarray(s.boxhi)
        inside = bool(((s.x[:, :s.dim] >= lo[:s.dim]) & (s.x[:, :s.dim] <= hi[:s.dim])).all())
        self.all_inside = getattr(self, "all_inside", True) and inside


class GasRefRun(_Forced, _GasRun):
    """rhosum when due, the restatement, reverse comm, gravity, then the post_force fixes"""


def gas_oracle(s, ph, fixes=(), shadows=True):
    """the oracle run and check_fields' shadow runs, attached as forcefix_util.forced_oracle
    attaches them: two row reorderings and the one-ulp input"""
    def make(sysm):
        r = GasRefRun(sysm, ph)
        r.fixes = tuple(fixes)
        return r

    ref = make(s)
    if shadows:
        for how in po.SPREAD_ORDERS:
            a = make(s)
            a.rev = how
            ref.alts.append(a)
        ref.alts.append(make(po.ulp_perturbed(s, planar=True)))
    return ref


# ---- scenarios ------------------------------------------------------------------------------
GAS_H = 3.0


def gas_tables(nt, h=GAS_H):
    cut = np.zeros((nt + 1, nt + 1))
    cut[1:, 1:] = h
    visc = np.zeros((nt + 1, nt + 1))
    vals = {(1, 1): 0.5, (1, 2): 0.75, (2, 2): 1.0}
    for i in range(1, nt + 1):
        for j in range(i, nt + 1):
            visc[i, j] = visc[j, i] = vals[(i, j)]
    return visc, cut


def gas_box(dim, ntypes=2, rhosum_nstep=1, at_rest=False):
    """po.cubic_lattice(8) jittered; two types with mass (1, 0.25), rho (1, 0.25), e (2.5,
    0.625) (one type: the first of each); gaussian velocities, so about half the pairs
    approach; h = 3 for rhosum and the gas, visc 0.5 | 0.75 | 1.0 for pairs 11 | 12 | 22"""
    s = po.cubic_lattice(8, dim=dim, ntypes=ntypes, type2_frac=0.4 if ntypes > 1 else 0.0,
                         vel_sigma=0.1, mass=(1.0, 0.25), rho=(1.0, 0.25), e=(2.5, 0.625))
    if at_rest:
        s.v[:] = 0.0
    visc, cut = gas_tables(ntypes)
    ph = GasPhysics(skin=0.3, dt=1e-3, every=5, rhosum_nstep=rhosum_nstep,
                    rhosum_cut=cut.copy() if rhosum_nstep > 0 else None, gas_visc=visc,
                    gas_cut=cut)
    return s, ph


HOT_GRAVITY = (0.3, -0.2, 0.1)


def hot_box(dim, rhosum_nstep=1, gravity=False):
    """gas_box with a per-atom e: in gas_box 0.4 e/m is exactly 1.0 for both types (2.5/1,
    0.625/0.25), so every atom has the same sound speed and c_j cannot be told from c_i.  Here
    e is scaled per atom by U(0.5, 1.5): neighbours differ in c by tens of per cent, from the
    setup pass on.  gravity: fix gravity on all types (cfg.gravity, inside the pass)"""
    s, ph = gas_box(dim, rhosum_nstep=rhosum_nstep)
    s.e = s.e * np.random.default_rng(20240).uniform(0.5, 1.5, s.n)
    if gravity:
        ph = dataclasses.replace(ph, gravity=HOT_GRAVITY)
    return s, ph


SHOCK_FIXES = (dict(kind="set", value=(None, 0.0, 0.0)),)   # fix setforce NULL 0.0 0.0


def shock_tube_case():
    """examples/USER/sph/shock_tube/shock2d.lmp scaled down: lattice sq 1.0, atoms on x in
    [-24, 24), y in [-5, 5), box x in [-30, 30] (fixed) and y periodic; type 2 where x >= 1;
    the example's mass (1, 0.25), e (2.5, 0.625), rho (1, 0.25); sph/rhosum 1 with h = 4,
    sph/idealgas 0.75 4.0; skin 0.5, rebuild every 5, dt 0.05; setforce NULL 0 0 on all"""
    xs, ys = np.meshgrid(np.arange(-24, 24), np.arange(-5, 5), indexing="xy")
    x = np.zeros((xs.size, 3))
    x[:, 0], x[:, 1] = xs.ravel(), ys.ravel()
    n = x.shape[0]
    t = np.where(x[:, 0] >= 1.0, 2, 1).astype(np.int32)
    mass = np.array([0.0, 1.0, 0.25])
    e_t = np.array([0.0, 2.5, 0.625])
    rho_t = np.array([0.0, 1.0, 0.25])
    s = po.System(2, np.array([-30.0, -5.0, -0.5]), np.array([30.0, 5.0, 0.5]), (0, 1, 0), x,
                  np.zeros((n, 3)), t, rho_t[t].copy(), e_t[t].copy(), np.ones(n), 2, mass)
    cut = np.zeros((3, 3))
    cut[1:, 1:] = 4.0
    visc = np.zeros((3, 3))
    visc[1:, 1:] = 0.75
    ph = GasPhysics(skin=0.5, dt=0.05, every=5, rhosum_nstep=1, rhosum_cut=cut.copy(),
                    gas_visc=visc, gas_cut=cut)
    return s, ph, SHOCK_FIXES


# ---- the engine and the pair layer ----------------------------------------------------------
def gas_config(sph, s, ph, path=0, **kw):
    if ph.rhosum_nstep > 0:
        kw["rhosum"] = dict(nstep=ph.rhosum_nstep, cut=ph.rhosum_cut)
    return sph.make_config(s.dim, s.ntypes, s.boxlo, s.boxhi, s.periodic, s.mass, ph.skin,
                           ph.dt, neigh_every=ph.every, kernel_path=path, gravity=ph.gravity,
                           gravity_mask=ph.gravity_mask, stationary_mask=ph.stationary_mask,
                           **kw)


def gas_engine(sph, s, ph, path=0, atoms=True):
    eng = sph.Engine(gas_config(sph, s, ph, path))
    eng.idealgas(ph.gas_visc, ph.gas_cut)
    if atoms:
        eng.set_atoms(s.x, s.v, s.type, s.rho, s.e, s.cv)
    return eng


def ghosted_inputs(s, ph, seed=7):
    """gas_box with ghosts from po.borders, its full and half lists, and per-atom vest, rho, e
    over owned + ghost atoms (vest = v; rho and e jittered so that no two atoms agree)"""
    nt = s.ntypes
    cns, cutneighmax = po.cutneighsq(nt, ph.cutmax(nt), ph.skin)
    g = po.borders(s, cutneighmax)
    foff, fnb = po.neigh_full(s.dim, g, nt, cns)
    hoff, hnb = po.half_from_full(g, foff, fnb)
    rng = np.random.default_rng(seed)
    rho = s.rho * rng.uniform(0.9, 1.1, s.n)
    e = s.e * rng.uniform(0.9, 1.1, s.n)
    return dict(g=g, cns=cns, foff=foff, fnb=fnb, hoff=hoff, hnb=hnb, vest=g.gather(s.v),
                rho=g.gather(rho), e=g.gather(e))
