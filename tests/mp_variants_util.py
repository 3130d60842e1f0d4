"""Jittered two- and three-phase boxes for the multiphase engine pass, and the strict bar they
are held to (tests/test_gpu_mp_variants.py).

The bubble lattice of the C5 tests makes the reference's own sums cancel pairwise, which is why
those tests widen their bars by the oracle's build spread.  Here every coordinate is jittered,
every atom moves, and rho / e / rmass vary per atom: nothing cancels, the oracle's own spread
stays below 1e-12 of each field, and the bar is the project's plain one --

  * normwise ||a-b||inf / ||b||inf < 1e-10, never widened;
  * per element |a_i - b_i| <= max(1e-10 |b_i|, 16 s_i), s_i the oracle's reordering and
    one-ulp spread alone (MpRefRun spread="nobuild": no build shadows, never build_rel);
  * a field the oracle holds at exactly zero is exactly zero.

That such a bar means something is a property of the INPUT, so it is asserted on the oracle's
numbers before the engine's are looked at (oracle_caps): the floor |b| <= 1e-6 ||b||inf leaves
out nothing (2-D: exactly the z components), the oracle's normwise spread is <= 1e-12, and at
most 0.5 % of a field's elements have a bar wider than 1e-9 |b_i|.  A seed that breaks a cap
is a bad seed: change the seed, not the cap."""
import numpy as np

import pyoracle as po
from conftest import SPREAD_K, elem_ratio, record_parity, rel_err

TOL = 1e-10
FLOOR = 1e-6
CAP_SPREAD = 1e-12     # (b) the oracle's own normwise spread
CAP_WIDE = 0.005       # (c) share of elements whose bar is wider than CAP_WIDE_AT |b_i|
CAP_WIDE_AT = 1e-9
FIELDS = ("x", "v", "rho", "e", "rmass", "cv", "cg", "f", "de")
SEED = 1   # (20240611 and 7 each put one element of one case under the floor, cap (a))

# the five styles' cutoffs (rhosum, cg, tait, st, heat)
CUTS = {"eq": (3.0, 3.0, 3.0, 3.0, 3.0),
        # per-style h: the gather's q.sih / q.hih differ from q.tih; rhosum cut = list cut
        "uneq": (3.0, 2.6, 3.0, 2.4, 2.8),
        # taitwater the smallest: pairs inside surfacetension's cut but outside taitwater's
        "uneq2": (3.0, 2.6, 2.4, 3.0, 2.8)}
GAMMAS = {"g1": (1.0, 1.0, 1.0), "pow": (2.0, 2.0, 2.0), "asym": (7.0, 1.4, 3.0)}


def mp_box(dim=3, ntypes=2, seed=SEED):
    """343 atoms (2-D: 144) on a jittered lattice in a periodic box of 7 (12) >= 2 x (3.0 +
    0.3), 40 % type 2 (three types: a further 20 % of all atoms relabelled 3), gaussian
    velocities, and a seeded per-atom spread of rho (2 %), e (30 %) and rmass = rho (1 +- 5 %).
    Positions are wrapped into the box (brick ownership reads them as given)."""
    n = 7 if dim == 3 else 12
    s = po.cubic_lattice(n, jitter=0.1, ntypes=2, type2_frac=0.4, vel_sigma=0.05,
                         rho=(1.0, 0.3), e=(0.04, 0.09), cv=(0.04, 0.06), dim=dim)
    rng = np.random.default_rng(seed)
    N = s.n
    s.rho = s.rho * (1.0 + 0.02 * rng.uniform(-1, 1, N))
    s.e = s.e * (1.0 + 0.30 * rng.uniform(-1, 1, N))
    s.rmass = s.rho * (1.0 + 0.05 * rng.uniform(-1, 1, N))
    if ntypes == 3:
        s.type = s.type.copy()
        s.type[rng.random(N) < 0.2] = 3
        s.ntypes = 3
        s.mass = np.array([0.0, 1.0, 1.0, 1.0])
    for d in range(dim):
        L = s.boxhi[d] - s.boxlo[d]
        s.x[:, d] = np.where(s.x[:, d] < s.boxlo[d], s.x[:, d] + L, s.x[:, d])
        s.x[:, d] = np.where(s.x[:, d] >= s.boxhi[d], s.x[:, d] - L, s.x[:, d])
    return s


def _table(nt, diag, off):
    """(nt+1)^2 table, upper triangle: diag[i-1] on (i, i), off[(i, j)] above it"""
    t = np.zeros((nt + 1, nt + 1))
    for i in range(1, nt + 1):
        t[i, i] = diag[i - 1]
        for j in range(i + 1, nt + 1):
            t[i, j] = off[(i, j)]
    return t


def mp_physics(ntypes=2, cuts="eq", gamma="g1", tait=True, st=True, heat=True, diag=False,
               rhosum_nstep=1, cg_nstep=1):
    """The five-style stack with everything the bubble physics leaves at a trivial value set
    to something that shows: skin 0.3 and rebuilds every 2 steps (forward-comm steps between),
    a background pressure, viscosity / heat / colour coefficients that differ per type pair
    (colour: off the diagonal only), type 2 pinned to Tc = 0.5 against type 1, no fix
    phase_change.  cuts / gamma: keys of CUTS / GAMMAS; diag: type 2 also pinned against its
    own type (heat_fixflag[2,2] = 2), which makes heatconduction asymmetric."""
    nt = ntypes
    rc, cc, tc, sc, hc = CUTS[cuts]

    def full(c):
        t = np.zeros((nt + 1, nt + 1))
        t[1:, 1:] = c
        return t

    visc = _table(nt, (0.05, 0.02, 0.035), {(1, 2): 0.03, (1, 3): 0.04, (2, 3): 0.025})
    hal = _table(nt, (0.2, 0.6, 0.4), {(1, 2): 0.3, (1, 3): 0.25, (2, 3): 0.5})
    cga = _table(nt, (0.0, 0.0, 0.0), {(1, 2): 1.0, (1, 3): 0.7, (2, 3): 0.4})
    ff = np.zeros((nt + 1, nt + 1), dtype=np.int32)
    htc = np.zeros((nt + 1, nt + 1))
    ff[1, 2], htc[1, 2] = 2, 0.5
    if diag:
        ff[2, 2], htc[2, 2] = 2, 0.5
    per = lambda v: np.array((0.0,) + tuple(v[:nt]))
    return po.MpPhysics(skin=0.3, dt=2e-3, every=2, rhosum_nstep=rhosum_nstep,
                        rhosum_cut=full(rc), cg_nstep=cg_nstep, cg_alpha=cga, cg_cut=full(cc),
                        tait=tait, rho0=per((1.0, 0.3, 0.6)), c0=per((10.0, 8.0, 9.0)),
                        gamma=per(GAMMAS[gamma]), rbg=per((0.5, 0.2, 0.1)), visc=visc,
                        tait_cut=full(tc), st=st, st_cut=full(sc), heat=heat, heat_alpha=hal,
                        heat_cut=full(hc), heat_fixflag=ff, heat_tc=htc, pc=None)


def pinned_pairs(ref):
    """How many pairs of the oracle's half list, inside heatconduction's cutoff, take the
    pinned temperature (pair_sph_heatconduction_phasechange.cpp:124-129: the pair's type is
    flagged for one of its atoms and that atom is the colder one)."""
    T = ref.tabs
    i, j, ti, tj, rsq = half_pairs(ref)
    temp = ref.e_all / ref.cv_all
    inside = rsq < T["heat_cut"][ti, tj] ** 2
    ff = T["heat_fixflag"][ti, tj]
    Ti, Tj = temp[i], temp[j]
    fire_i = (ff == ti) & (Ti < Tj)
    fire_j = (ff == tj) & (Tj < np.where(fire_i, T["heat_tc"][ti, tj], Ti))
    return int((inside & (fire_i | fire_j)).sum())


def half_pairs(ref):
    """The pairs of the oracle's half list (one process' view): row atom i, entry j (owned or
    ghost), their types and rsq at the positions of the last build or forward comm."""
    g = ref.g
    i = np.repeat(np.arange(ref.s.n), np.diff(ref.hoff))
    j = np.asarray(ref.hnb[:i.size], dtype=np.int64)
    d = g.x[i] - g.x[j]
    return i, j, g.type[i], g.type[j], (d * d).sum(axis=1)


def pairs_between(ref, inner, outer):
    """pairs with inner cut <= r < outer cut (tables of ref.tabs by name)"""
    _, _, ti, tj, rsq = half_pairs(ref)
    T = ref.tabs
    return int(((rsq >= T[inner][ti, tj] ** 2) & (rsq < T[outer][ti, tj] ** 2)).sum())


class Snap:
    """One compared moment of an oracle run, frozen: the fields and their reordering / one-ulp
    spread, types, neighbour counts, and what the premises read (pinned pairs, pairs between
    taitwater's and surfacetension's cutoffs)."""

    def __init__(self, ref, fields):
        assert ref.alts and not any(a.build for a in ref.alts)
        self.dim, self.n, self.step = ref.s.dim, ref.s.n, ref.step
        self.s = ref.s.copy()
        self.alts = ()
        self._f = {k: np.array(ref.field(k), dtype=np.float64) for k in fields}
        self._s = {k: np.array(ref.spread(k, builds=False)) for k in fields}
        self.type = ref.s.type.copy()
        self.counts = ref.numneigh_full().copy()
        self.pinned = pinned_pairs(ref) if ref.ph.heat else 0
        self.st_not_tait = pairs_between(ref, "tait_cut", "st_cut") if ref.ph.st and ref.ph.tait else 0
        for a in list(self._f.values()) + list(self._s.values()) + [self.type, self.counts]:
            a.setflags(write=False)

    def field(self, k):
        return self._f[k]

    def spread(self, k, builds=False):
        assert not builds
        return self._s[k]


def oracle_run(s, ph, at, procgrid=None, fields=FIELDS):
    """MpRefRun of (s, ph) with the reordering and one-ulp shadows only; Snaps at the steps
    `at` (0 = setup)."""
    ref = po.MpRefRun(s, ph, procgrid=procgrid, spread="nobuild")
    ref.setup()
    out = {}
    for step in range(max(at) + 1):
        if step:
            ref.run(1)
        if step in at:
            out[step] = Snap(ref, fields)
    return out


def _bar(want, sp):
    return np.maximum(TOL * np.abs(want), SPREAD_K * sp)


def oracle_caps(ref, fields, where):
    """The caps (a)-(c) of the module doc on the oracle's own numbers; returns, per field, the
    figures it found (for the record)."""
    dim = ref.s.dim
    out = {}
    for k in fields:
        want = np.asarray(ref.field(k), dtype=np.float64)
        big = float(np.abs(want).max()) if want.size else 0.0
        if big == 0.0:
            out[k] = dict(zero=True)
            continue
        sp = ref.spread(k, builds=False)
        assert sp is not None, (where, k, "the oracle run carries no shadows")
        assert not any(a.build for a in ref.alts), (where, "build shadows present")
        m = np.abs(want) > FLOOR * big
        if dim == 2 and want.ndim == 2:   # (a) the z components, exactly a third
            assert m[:, :2].all() and not m[:, 2].any(), (where, k, "floor", 1.0 - m.mean())
            assert not want[:, 2].any(), (where, k, "2-D z component not zero in the oracle")
        else:                              # (a) nothing
            assert m.all(), (where, k, "floor leaves out", int((~m).sum()), "of", m.size)
        nsp = float(sp.max()) / big       # (b)
        assert nsp <= CAP_SPREAD, (where, k, "oracle normwise spread", nsp)
        wide = _bar(want, sp)[m] > CAP_WIDE_AT * np.abs(want[m])   # (c)
        assert wide.mean() <= CAP_WIDE, (where, k, "elements with a bar over 1e-9",
                                         int(wide.sum()), "of", int(m.sum()))
        out[k] = dict(floor_out=float(1.0 - m.mean()), spread=nsp, wide=int(wide.sum()),
                      worst_bar=float((_bar(want, sp)[m] / np.abs(want[m])).max()))
    return out


def check_fields_strict(got, ref, fields, where):
    """oracle_caps, then the strict bar of the module doc on the engine's fields `got`."""
    caps = oracle_caps(ref, fields, where)
    for k in fields:
        want = np.asarray(ref.field(k), dtype=np.float64)
        a = np.asarray(got[k], dtype=np.float64)
        assert a.shape == want.shape, (where, k, a.shape, want.shape)
        if caps[k].get("zero"):
            record_parity(k, a, want, None, TOL)
            assert not a.any(), (where, k, "the oracle's field is exactly zero", np.abs(a).max())
            continue
        sp = ref.spread(k, builds=False)
        record_parity(k, a, want, sp, TOL)
        if ref.s.dim == 2 and want.ndim == 2:   # (every term carries an exact zero factor)
            assert not a[:, 2].any(), (where, k, "2-D z component", np.abs(a[:, 2]).max())
        nerr = rel_err(a, want)
        assert nerr < TOL, (where, k, "normwise", nerr)
        r = elem_ratio(a, want, sp, tol=TOL)
        if r > 1.0:   # (the worst element, for the record)
            q = np.abs(a - want).ravel() / np.where(_bar(want, sp) > 0, _bar(want, sp), 1.0).ravel()
            q = np.where(np.abs(want).ravel() > FLOOR * np.abs(want).max(), q, 0.0)
            i = int(np.argmax(q))
            detail = dict(i=i, got=a.ravel()[i], want=want.ravel()[i],
                          spread=float(sp.ravel()[i]), maxabs=float(np.abs(want).max()))
            assert r <= 1.0, (where, k, "elementwise", r, detail)
    return caps
