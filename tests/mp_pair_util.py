"""The pair-style layer's multiphase styles (sph_hip_rhosum_multiphase, _colorgradient,
_taitwater_multiphase, _heatconduction_phasechange, _surfacetension) beyond their one 3-D
two-type configuration: named cases on mp_variants_util's jittered boxes, the oracle's results
with their reordering spread, a numpy restatement of the five pair terms (the FULL-list gather
of the two asymmetric styles, which the C oracle's scatter cannot express), premises() on the
oracle alone, and the few lines that drive a PairContext.  Shared by test_mp_pair_cpu.py and
test_gpu_mp_pair.py.

Bars (never widened): normwise ||a-b||inf / ||b||inf < 1e-10 (rhosum 1e-13), per element
|a_i - b_i| <= max(1e-10 |b_i|, SPREAD_K s_i) with s_i the oracle's own reordering spread (the
same list with every row's entries reversed, and in one seeded permutation of the entries and
of the order the rows are visited in: relabelled), a field the oracle holds at zero exactly
zero."""
import numpy as np

import pyoracle as po
import mp_variants_util as mv
from conftest import SPREAD_K, elem_ratio, record_parity, rel_err

TOL = 1e-10
TOL_RHO = 1e-13
SKIN = 0.3
PERM_SEED = 77
STYLES = ("rhosum", "cg", "tait", "st", "heat")
HALF_STYLES = ("tait", "st", "heat")
CUT_OF = dict(rhosum="rhosum_cut", cg="cg_cut", tait="tait_cut", st="st_cut", heat="heat_cut")
NORM = {3: 0.0716197243913529, 2: 0.04195297663091802}   # sph_kernel_quintic.cpp

# three types, upper triangle in the order 11 12 13 22 23 33: cuts that differ within each
# style; 0 = the style has no coefficients for the pair (one per half-list style, each a
# different pair; every pair keeps a cut in rhosum and colorgradient)
T3 = dict(rhosum_cut=(3.0, 2.8, 2.6, 2.9, 2.7, 2.5),
          cg_cut=(2.6, 3.0, 2.4, 2.8, 2.5, 2.7),
          tait_cut=(2.8, 3.0, 2.5, 2.6, 0.0, 2.9),
          st_cut=(2.7, 2.5, 0.0, 3.0, 2.6, 2.4),
          heat_cut=(2.5, 2.9, 2.7, 2.8, 3.0, 0.0))
ABSENT3 = dict(tait=(2, 3), st=(1, 3), heat=(3, 3))

# name -> dim, types, cuts (key of mp_variants_util.CUTS, or "t3"), gamma, and one more
# heat_fixflag entry (i, j, flag, Tc)
CASES = {
    "3d-eq": (3, 2, "eq", "g1", None),
    "3d-uneq-asym": (3, 2, "uneq", "asym", None),
    "3d-uneq2-pow": (3, 2, "uneq2", "pow", None),
    "3d-3types": (3, 3, "t3", "asym", None),
    "2d-eq": (2, 2, "eq", "g1", None),
    "2d-uneq-asym": (2, 2, "uneq", "asym", None),
    "2d-3types": (2, 3, "t3", "asym", None),
    # the flag on a same-type pair, Tc inside that type's temperatures (1.05 .. 1.95): where
    # both atoms are colder the two clamps chain -- Ti is replaced, then Tj meets the new Ti
    "diag": (3, 2, "uneq", "asym", (2, 2, 2, 1.5)),
    "ff1": (3, 2, "uneq", "asym", (1, 2, 1, 0.5)),    # the flag names the row's (lower) type
}
BASE_OF = {"diag": "3d-uneq-asym", "ff1": "3d-uneq-asym"}


def _upper(nt, vals):
    t = np.zeros((nt + 1, nt + 1))
    k = 0
    for i in range(1, nt + 1):
        for j in range(i, nt + 1):
            t[i, j] = vals[k]
            k += 1
    return t


class Case:
    """One named case: system, ghosts, lists, per-atom arrays over owned + ghost atoms (ghosts
    copy their owner), the tables mirrored as init_one does (T, what the oracle reads) and as
    coeff() holds them (U: upper triangle, the lower one filled with values no pair may see)."""

    def __init__(self, name, drop=0):
        dim, nt, cuts, gamma, ffx = CASES[name]
        self.name, self.dim, self.nt = name, dim, nt
        s = mv.mp_box(dim, nt)
        if drop:     # (another atom count, ghost count and list: the last owned atoms left out)
            left = s.n - drop
            for k in ("x", "v", "type", "rho", "e", "cv", "rmass"):
                setattr(s, k, np.ascontiguousarray(getattr(s, k)[:left]))
        ph = mv.mp_physics(nt, cuts if cuts != "t3" else "eq", gamma)
        if cuts == "t3":
            for k, v in T3.items():
                setattr(ph, k, _upper(nt, v))
            a, b = ABSENT3["tait"]
            ph.visc[a, b] = 0.0
            a, b = ABSENT3["heat"]
            ph.heat_alpha[a, b] = 0.0
        if ffx is not None:
            a, b, t, tc = ffx
            ph.heat_fixflag[a, b], ph.heat_tc[a, b] = t, tc
        self.s, self.ph = s, ph
        names = ("rhosum_cut", "cg_cut", "cg_alpha", "tait_cut", "visc", "st_cut", "heat_cut",
                 "heat_alpha", "heat_tc", "heat_fixflag")
        self.T = {k: po._sym(np.triu(getattr(ph, k))) for k in names}
        self.U = {}
        for k in names:
            u = np.triu(getattr(ph, k)).astype(self.T[k].dtype)
            lo = np.tril(np.ones((nt + 1, nt + 1), dtype=bool), -1)
            lo[:, 0] = False
            u[lo] = 7 if k == "heat_fixflag" else 9.75
            self.U[k] = np.ascontiguousarray(u)
        self.rho0, self.c0, self.gamma, self.rbg = (np.ascontiguousarray(getattr(ph, k), dtype=float)
                                                    for k in ("rho0", "c0", "gamma", "rbg"))
        self.B = self.c0 ** 2 * self.rho0 / np.where(self.gamma > 0, self.gamma, 1.0)
        self.cns, cmax = po.cutneighsq(nt, ph.cutmax(nt), SKIN)
        g = self.g = po.borders(s, cmax)
        self.n, self.nall = g.nlocal, g.nall
        self.foff, self.fnb = po.neigh_full(dim, g, nt, self.cns)
        self.hoff, self.hnb = po.half_from_full(g, self.foff, self.fnb)
        self.x, self.type = np.ascontiguousarray(g.x), np.ascontiguousarray(g.type)
        for k, a in (("v_all", s.v), ("rho_all", s.rho), ("e_all", s.e), ("cv_all", s.cv),
                     ("rm_all", s.rmass)):
            setattr(self, k, np.ascontiguousarray(g.gather(a)))
        # colorgradient of every atom, from the oracle (ghosts copy their owner)
        cg = orc(self, "cg", self.foff, self.fnb)
        self.cg_all = np.ascontiguousarray(np.concatenate([cg[:self.n], cg[:self.n][g.owner]]))
        self.tabs = self.T                  # (what mp_variants_util.pinned_pairs reads)
        self._want = {}
        for a in (self.x, self.type, self.v_all, self.rho_all, self.e_all, self.cv_all,
                  self.rm_all, self.cg_all, self.foff, self.fnb, self.hoff, self.hnb):
            a.setflags(write=False)

    def lists(self, style):
        return (self.foff, self.fnb) if style in ("rhosum", "cg") else (self.hoff, self.hnb)

    def want(self, style, newton=1):
        """(oracle result, reordering spread) of a style on its list; full-list styles ignore
        newton.  Frozen."""
        key = (style, 1 if style in ("rhosum", "cg") else newton)
        if key not in self._want:
            self._want[key] = want_on(self, style, *self.lists(style), key[1])
        return self._want[key]


_CASES = {}


def case(name, drop=0):
    if (name, drop) not in _CASES:
        _CASES[(name, drop)] = Case(name, drop)
    return _CASES[(name, drop)]


def with_z(c, amp=0.2, seed=5):
    """a view of a 2-D case whose owned atoms carry a seeded z in (-amp, amp); ghosts copy
    their owner's (z is not periodic in 2-D).  Lists and tables are the case's own."""
    import copy
    assert c.dim == 2
    z = np.random.default_rng(seed).uniform(-amp, amp, c.n)
    x = np.array(c.x)
    x[:, 2] = c.g.gather(z)
    c2 = copy.copy(c)
    c2.x = np.ascontiguousarray(x)
    c2.x.setflags(write=False)
    c2._want = {}
    return c2


def want_on(c, style, off, nb, newton=1, fn=None):
    """(result, reordering spread) of a style on the list off/nb: the oracle -- or fn, a
    function with orc's arguments -- on the list as given, with every row's entries reversed,
    and in one seeded permutation (relabelled: of every row's entries and of the order the rows
    are visited in).  Frozen."""
    fn = fn or orc
    nb = np.asarray(nb)[:int(np.asarray(off)[-1])]
    base = fn(c, style, off, nb, newton)
    c2, off2, nb2, new = relabelled(c, off, nb)
    alts = (fn(c, style, off, po._reverse_rows(off, nb), newton),
            fn(c2, style, off2, nb2, newton)[new])
    sp = np.zeros_like(base)
    for alt in alts:
        sp = np.maximum(sp, np.abs(alt - base))
    base.setflags(write=False)
    sp.setflags(write=False)
    return base, sp


def relabelled(c, off, nb, seed=PERM_SEED):
    """The same atoms, pairs and pair orientations with every row's entries in one seeded
    order and the owned atoms renumbered by one seeded permutation, so that the rows are
    visited in another order.  A slot's j shares arrive in row order: reordering inside the
    rows alone moves no ghost slot and no j share, while a gather over the reverse list sums
    them in an order of its own.  -> (the case's view, off, nb, new index of every atom)"""
    import copy
    n = c.n
    new = np.arange(c.nall)
    new[:n] = np.random.default_rng(seed + 1).permutation(n)
    old = np.empty_like(new)
    old[new] = np.arange(c.nall)
    c2 = copy.copy(c)
    for k in ("x", "type", "v_all", "rho_all", "e_all", "cv_all", "rm_all", "cg_all"):
        setattr(c2, k, np.ascontiguousarray(getattr(c, k)[old]))
    off = np.asarray(off, dtype=np.int64)
    cnt2 = np.diff(off)[old[:n]]
    off2 = np.zeros(n + 1, dtype=np.int64)
    off2[1:] = np.cumsum(cnt2)
    idx = np.repeat(off[old[:n]] - off2[:-1], cnt2) + np.arange(off2[-1])
    nb2 = new[permuted_rows(off, nb, seed)[idx]]
    return c2, off2, np.ascontiguousarray(nb2, dtype=np.int32), new


def emptied(off, nb, keep):
    """the list with the rows outside `keep` (bool per row) emptied"""
    off = np.asarray(off, dtype=np.int64)
    cnt = np.where(keep, np.diff(off), 0)
    row = np.repeat(np.arange(len(off) - 1), np.diff(off))
    off2 = np.zeros(len(off), dtype=np.int64)
    off2[1:] = np.cumsum(cnt)
    return off2, np.ascontiguousarray(np.asarray(nb)[:row.size][keep[row]])


def permuted_rows(off, nb, seed=PERM_SEED):
    """every CSR row's entries in one seeded order"""
    off = np.asarray(off, dtype=np.int64)
    row = np.repeat(np.arange(len(off) - 1), np.diff(off))
    key = np.random.default_rng(seed).random(row.size)
    return np.ascontiguousarray(np.asarray(nb)[:row.size][np.lexsort((key, row))])


def orc(c, style, off, nb, newton=1, cg_all=None):
    """The C oracle's compute() of one style over the list off/nb (row r = owned atom r; a row
    that a skip list leaves out is empty) -> rho (nall), cg / f (nall, 3) or de (nall), from
    zero."""
    L, T, n, nt, dim = po.lib(), c.T, c.n, c.nt, c.dim
    off = np.ascontiguousarray(off, dtype=np.int64)
    nb = np.ascontiguousarray(nb if len(nb) else np.zeros(1), dtype=np.int32)
    cut = T[CUT_OF[style]]
    if style == "rhosum":
        out = np.zeros(c.nall)
        L.orc_rhosum_multiphase(dim, n, c.x, c.type, nt, c.rm_all, cut, cut * cut, off, nb, out)
    elif style == "cg":
        out = np.zeros((c.nall, 3))
        L.orc_colorgradient(dim, n, c.x, c.rho_all, c.rm_all, c.type, nt, T["cg_alpha"], cut,
                            cut * cut, off, nb, out)
    elif style == "tait":
        out = np.zeros((c.nall, 3))
        L.orc_taitwater_multiphase(dim, n, newton, c.x, c.v_all, c.rho_all, c.type, nt, c.rm_all,
                                   c.rho0, c.c0, c.B, c.gamma, c.rbg, T["visc"], cut, cut * cut,
                                   off, nb, out)
    elif style == "st":
        out = np.zeros((c.nall, 3))
        L.orc_surfacetension(dim, n, newton, c.x, c.rho_all, c.rm_all, c.type, nt,
                             c.cg_all if cg_all is None else cg_all, cut, cut * cut, off, nb, out)
    else:
        assert style == "heat"
        out = np.zeros(c.nall)
        L.orc_heatconduction_phasechange(dim, n, newton, c.x, c.e_all, c.cv_all, c.rho_all,
                                         c.rm_all, c.type, nt, T["heat_alpha"],
                                         T["heat_fixflag"].ctypes.data, T["heat_tc"].ctypes.data,
                                         cut, cut * cut, off, nb, out)
    return out


# ---- the five pair terms in numpy ------------------------------------------------------------
def _w(dim, r):
    """sph_kernel_quintic.cpp:17-43, s = 3 r"""
    s = 3.0 * r
    a = np.where(s < 3.0, (3 - s) ** 5, 0.0)
    b = np.where(s < 2.0, (2 - s) ** 5, 0.0)
    cc = np.where(s < 1.0, (1 - s) ** 5, 0.0)
    return NORM[dim] * np.where(s < 1.0, a - 6 * b + 15 * cc, np.where(s < 2.0, a - 6 * b, a))


def _dw(dim, r):
    """sph_kernel_quintic.cpp:45-73: the expanded pieces of dW/ds, times 3 norm"""
    s = 3.0 * r
    p1 = -50 * s ** 4 + 120 * s ** 3 - 120 * s
    p2 = 25 * s ** 4 - 180 * s ** 3 + 450 * s ** 2 - 420 * s + 75
    p3 = -5 * s ** 4 + 60 * s ** 3 - 270 * s ** 2 + 540 * s - 405
    return 3.0 * NORM[dim] * np.where(s < 1, p1, np.where(s < 2, p2, np.where(s < 3.0, p3, 0.0)))


class _Pairs:
    """the list's pairs inside a style's cut: i (row atom), j, types, separation, r, h"""

    def __init__(self, c, off, nb, cut):
        off = np.asarray(off, dtype=np.int64)
        i = np.repeat(np.arange(c.n, dtype=np.int64), np.diff(off))
        j = np.asarray(nb[:off[-1]], dtype=np.int64)
        d = c.x[i] - c.x[j]
        rsq = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
        h = cut[c.type[i], c.type[j]]
        k = rsq < h * h
        self.i, self.j, self.d, self.h = i[k], j[k], d[k], h[k]
        self.ti, self.tj = c.type[self.i], c.type[self.j]
        self.r = np.sqrt(rsq[k])
        self.ih = 1.0 / self.h

    def wfd(self, dim):
        ih = self.ih
        w = _dw(dim, self.r * ih)
        return w * ih * ih * ih * ih if dim == 3 else w * ih * ih * ih


def _scatter(c, P, vi, vj, newton, gather):
    """pair k's i share, then its j share (newton_pair || j < nlocal), in list order; gather:
    a FULL list, every row keeps its own share only"""
    npair = P.i.size
    tgt = np.empty(2 * npair, dtype=np.int64)
    tgt[0::2], tgt[1::2] = P.i, P.j
    on = np.ones(2 * npair, dtype=bool)
    on[1::2] = False if gather else (True if newton else P.j < c.n)
    ev = np.empty((2 * npair,) + vi.shape[1:])
    ev[0::2], ev[1::2] = vi, vj
    out = np.zeros((c.nall,) + vi.shape[1:])
    np.add.at(out, tgt[on], ev[on])
    return out


def _st_vec(dim, cg, e):
    """pair_sph_surfacetension.cpp:135-168"""
    c0, c1, c2 = cg[:, 0], cg[:, 1], cg[:, 2]
    e0, e1, e2 = e[:, 0], e[:, 1], e[:, 2]
    third, two3 = 0.3333333333333333, 0.6666666666666666
    if dim == 2:
        absc = np.sqrt(c0 * c0 + c1 * c1)
        S = np.stack([e0 * ((c1 * c1 + c0 * c0) / 2 - c0 * c0) - c0 * e1 * c1,
                      e1 * ((c1 * c1 + c0 * c0) / 2 - c1 * c1) - e0 * c0 * c1,
                      np.zeros_like(c0)], axis=1)
    else:
        absc = np.sqrt(c0 * c0 + c1 * c1 + c2 * c2)
        S = np.stack([e0 * (third * c2 * c2 + third * c1 * c1 - two3 * c0 * c0)
                      - c0 * e2 * c2 - c0 * e1 * c1,
                      e1 * (third * c2 * c2 - two3 * c1 * c1 + third * c0 * c0)
                      - c1 * e2 * c2 - e0 * c0 * c1,
                      e2 * (-two3 * c2 * c2 + third * c1 * c1 + third * c0 * c0)
                      - e1 * c1 * c2 - e0 * c0 * c2], axis=1)
    ok = absc > 1.0e-12
    return np.where(ok[:, None], S / np.where(ok, absc, 1.0)[:, None], 0.0)


def np_style(c, style, off, nb, newton=1, gather=False, cg_all=None):
    """One compute() of a style over off/nb, per pair in float64 from the reference's formulas
    (pair_sph_rhosum_multiphase.cpp:112-167, pair_sph_colorgradient.cpp:118-187,
    pair_sph_taitwater_multiphase.cpp:95-183 with p_j's gamma[itype],
    pair_sph_heatconduction_phasechange.cpp:81-138 with the two chained clamps,
    pair_sph_surfacetension.cpp:50-192).  gather: off/nb is a FULL list and the half-list
    styles add each pair, evaluated with the row atom as i, to the row atom only."""
    T, dim, n = c.T, c.dim, c.n
    P = _Pairs(c, off, nb, T[CUT_OF[style]])
    i, j, ti, tj = P.i, P.j, P.ti, P.tj
    rho, rm = c.rho_all, c.rm_all
    if style == "rhosum":
        h = T["rhosum_cut"][c.type[:n], c.type[:n]]
        self_ = _w(dim, np.zeros(n)) / (h * h * h if dim == 3 else h * h)
        ih = P.ih
        wf = _w(dim, P.r * ih) * (ih * ih * ih if dim == 3 else ih * ih)
        out = np.zeros(c.nall)
        out[:n] = self_
        np.add.at(out, i, wf)
        out[:n] *= rm[:n]
        return out
    wfd = P.wfd(dim)
    if style == "cg":
        e = P.d / P.r[:, None]
        sigi, sigj = rho[i] / rm[i], rho[j] / rm[j]
        dphi = -wfd * T["cg_alpha"][ti, tj] / (sigj * sigj) * sigi
        v = dphi[:, None] * e
        if dim == 2:
            v[:, 2] = 0.0
        out = np.zeros((c.nall, 3))
        np.add.at(out, i, v)
        return out
    if style == "tait":
        w = wfd / P.r
        Vi, Vj = rm[i] / rho[i], rm[j] / rho[j]
        V2 = Vi * Vi + Vj * Vj
        pi = c.B[ti] * ((rho[i] / c.rho0[ti]) ** c.gamma[ti] - c.rbg[ti])
        pj = c.B[tj] * ((rho[j] / c.rho0[tj]) ** c.gamma[ti] - c.rbg[tj])   # (:148, the quirk)
        pij = (rho[j] * pi + rho[i] * pj) / (rho[i] + rho[j])
        fvisc = V2 * T["visc"][ti, tj] * w
        fpair = -V2 * pij * w
        F = P.d * fpair[:, None] + (c.v_all[i] - c.v_all[j]) * fvisc[:, None]
        return _scatter(c, P, F, -F, newton, gather)
    if style == "st":
        cg = c.cg_all if cg_all is None else cg_all
        e = P.d / P.r[:, None]
        if dim == 2:
            e[:, 2] = 0.0
        Si, Sj = _st_vec(dim, cg[i], e), _st_vec(dim, cg[j], e)
        Vi, Vj = rm[i] / rho[i], rm[j] / rho[j]
        F = (Si * (Vi * Vi)[:, None] + Sj * (Vj * Vj)[:, None]) * wfd[:, None]
        return _scatter(c, P, F, -F, newton, gather)
    assert style == "heat"
    w = wfd / P.r
    Ti, Tj = c.e_all[i] / c.cv_all[i], c.e_all[j] / c.cv_all[j]
    ff, tc = T["heat_fixflag"][ti, tj], T["heat_tc"][ti, tj]
    Ti = np.where((ff == ti) & (Ti < Tj), tc, Ti)
    Tj = np.where((ff == tj) & (Tj < Ti), tc, Tj)      # (against the replaced Ti)
    dE = 2.0 * T["heat_alpha"][ti, tj] * (Ti - Tj) * w / (rho[i] * rho[j])
    return _scatter(c, P, dE * rm[j], -dE * rm[i], newton, gather)


def fold(c, a):
    """a half-list result with its ghost slots added to their owners (reverse comm)"""
    out = np.array(a[:c.n])
    np.add.at(out, c.g.owner, a[c.n:])
    return out


# ---- premises ---------------------------------------------------------------------------------
class _Capped:
    """what mp_variants_util.oracle_caps reads: one field with its spread"""
    alts = ()

    def __init__(self, c, base, sp):
        self.s, self._b, self._s = c.s, base, sp

    def field(self, k):
        return self._b

    def spread(self, k, builds=False):
        return self._s


def premises(name):
    """Conditions on the inputs, on the oracle's numbers alone; returns what it found.

    bands: per style and type pair with a cut, the atom pairs between that cut and the style's
    largest; for the pair that holds the largest cut itself, between the style's smallest cut
    and it (tables_util.premises does the same); a style with one cut for every pair has no
    such band and is left out.  Across styles, the pairs between two styles' cuts."""
    c = case(name)
    dim, nt, cuts = c.dim, c.nt, CASES[name][2]
    out = dict(n=c.n, nghost=c.g.nghost, full=int(c.foff[-1]), half=int(c.hoff[-1]),
               pieces={}, bands={}, absent={}, caps={}, ghost_floor={})
    for st in STYLES:
        off, nb = c.lists(st)
        cut = c.T[CUT_OF[st]]
        P = _Pairs(c, off, nb, cut)
        s3 = 3.0 * P.r * P.ih
        out["pieces"][st] = tuple(int(((s3 >= k) & (s3 < k + 1)).sum()) for k in range(3))
        if cuts == "eq":
            assert min(out["pieces"][st]) > 0, (name, st, out["pieces"][st])
        # every pair of the list, whatever the cut: the bands between table entries
        A = _Pairs(c, off, nb, np.full_like(cut, 1e9))
        pos = cut[1:, 1:][cut[1:, 1:] > 0]
        cmax, cmin = float(pos.max()), float(pos.min())
        for a in range(1, nt + 1):
            for b in range(a, nt + 1):
                m = ((A.ti == a) & (A.tj == b)) | ((A.ti == b) & (A.tj == a))
                if cut[a, b] == 0:
                    k = int((m & (A.r < cmax)).sum())
                    out["absent"][(st, a, b)] = k
                elif cmin < cmax:
                    lo, hi = (cut[a, b], cmax) if cut[a, b] < cmax else (cmin, cmax)
                    k = int((m & (A.r > lo) & (A.r < hi)).sum())
                    out["bands"][(st, a, b)] = k
                else:
                    continue                      # (one cut for the whole style: no band)
                assert k > 0, (name, st, a, b)
    if cuts == "t3":
        assert sorted(k[0] for k in out["absent"]) == ["heat", "st", "tait"], out["absent"]
    # two styles with different cuts: pairs between them (a style reading the other's table)
    H = _Pairs(c, c.hoff, c.hnb, np.full_like(c.T["tait_cut"], 1e9))
    for a, b in (("tait", "st"), ("tait", "heat"), ("st", "heat")):
        ca, cb = c.T[CUT_OF[a]][H.ti, H.tj], c.T[CUT_OF[b]][H.ti, H.tj]
        k = int(((H.r < np.maximum(ca, cb)) & (H.r >= np.minimum(ca, cb))).sum())
        out["bands"][(a, b)] = k
        assert (k > 0) == (cuts != "eq"), (name, a, b, k)
    if cuts == "uneq2":
        k = int(((H.r < c.T["st_cut"][H.ti, H.tj]) & (H.r >= c.T["tait_cut"][H.ti, H.tj])).sum())
        out["st_not_tait"] = k
        assert k > 0
    out["pinned"] = mv.pinned_pairs(c)
    assert out["pinned"] > 0, name
    if name in BASE_OF:
        assert out["pinned"] != mv.pinned_pairs(case(BASE_OF[name])), name
    # pairs whose second clamp fires only because the first one replaced Ti
    Q = _Pairs(c, c.hoff, c.hnb, c.T["heat_cut"])
    Ti, Tj = c.e_all[Q.i] / c.cv_all[Q.i], c.e_all[Q.j] / c.cv_all[Q.j]
    ff, tc = c.T["heat_fixflag"][Q.ti, Q.tj], c.T["heat_tc"][Q.ti, Q.tj]
    out["chained"] = int(((ff == Q.ti) & (Ti < Tj) & (ff == Q.tj) & (Tj < tc)).sum())
    assert (out["chained"] > 0) == (name == "diag"), (name, out["chained"])
    out["owned_ghost"] = int((c.hnb[:c.hoff[-1]] >= c.n).sum())
    assert out["owned_ghost"] > 0
    assert set(np.unique(c.type[:c.n])) == set(range(1, nt + 1))
    for st in STYLES:
        for newton in ((1,) if st in ("rhosum", "cg") else (1, 0)):
            base, sp = c.want(st, newton)
            own, ghost = base[:c.n], base[c.n:]
            assert np.isfinite(base).all(), (name, st)
            if base.ndim == 2 and dim == 2:
                assert not base[:, 2].any(), (name, st, "2-D z component")
                assert (own[:, :2] != 0).all(), (name, st)
            else:
                assert (own != 0).all(), (name, st)
            if st in ("rhosum", "cg") or not newton:
                assert not ghost.any(), (name, st, newton, "ghost slots")
            else:     # ghost slots: their share under the floor is left out of the per-element bar
                big = np.abs(base).max()
                g2 = ghost[:, :2] if (ghost.ndim == 2 and dim == 2) else ghost
                out["ghost_floor"][st] = float((np.abs(g2) <= mv.FLOOR * big).mean())
                assert ghost.any(), (name, st)
            out["caps"][(st, newton)] = mv.oracle_caps(_Capped(c, own, sp[:c.n]), ("f",),
                                                       (name, st, newton))["f"]
    return out


# ---- the strict bar ---------------------------------------------------------------------------
def check(got, c, style, newton, where, rows=None, ref=None):
    """got against the oracle at the bars of the module doc; rows: the compared owned rows of
    a full-list style (default all).  Half-list styles compare the ghost slots too.  ref:
    (result, spread) of want_on for another list than the case's own."""
    base, sp = ref if ref is not None else c.want(style, newton)
    full = style in ("rhosum", "cg")
    tol = TOL_RHO if style == "rhosum" else TOL
    a = np.asarray(got, dtype=np.float64)
    assert a.shape == base.shape, (where, style, a.shape)
    if full:
        sel = np.arange(c.n) if rows is None else np.asarray(rows)
        a, b, s = a[sel], base[sel], sp[sel]
    else:
        b, s = base, sp
    record_parity(style, a, b, s, tol)
    assert np.isfinite(a).all(), (where, style)
    if c.dim == 2 and b.ndim == 2:
        assert not a[:, 2].any(), (where, style, "2-D z component", np.abs(a[:, 2]).max())
    if not full and not newton:
        assert not a[c.n:].any(), (where, style, "ghost slots with newton off")
    zero = b == 0
    assert not a[zero].any(), (where, style, "the oracle holds these at zero")
    nerr = rel_err(a, b)
    print(f"[mp pair] {where} {style}: normwise {nerr:.2e} "
          f"bar ratio {elem_ratio(a, b, s, tol=tol):.3f}")
    assert nerr < tol, (where, style, "normwise", nerr)
    r = elem_ratio(a, b, s, tol=tol)
    assert r <= 1.0, (where, style, "elementwise", r, SPREAD_K)


# ---- driving a PairContext --------------------------------------------------------------------
def context(sph_amd, c, newton=1):
    ctx = sph_amd.PairContext(c.dim, c.nt, newton)
    stage_atoms(ctx, c)
    set_coeffs(ctx, c)
    return ctx


def stage_atoms(ctx, c):
    ctx.atoms(c.n, c.g.nghost, c.x, c.type, vest=c.v_all, rho=c.rho_all, e=c.e_all)
    ctx.atoms_multiphase(c.rm_all, c.cv_all)


def set_coeffs(ctx, c):
    U = c.U
    ctx.rhosum_multiphase_coeff(U["rhosum_cut"])
    ctx.colorgradient_coeff(U["cg_alpha"], U["cg_cut"])
    ctx.taitwater_multiphase_coeff(c.rho0, c.c0, c.gamma, c.rbg, U["visc"], U["tait_cut"])
    ctx.heatconduction_phasechange_coeff(U["heat_alpha"], U["heat_cut"],
                                         fixflag=U["heat_fixflag"], tc=U["heat_tc"])
    ctx.surfacetension_coeff(U["st_cut"])


def blank(c, style, fill=None, seed=0):
    """an output array of a style: zeros, or seeded nonzero values"""
    shape = (c.nall,) if style in ("rhosum", "heat") else (c.nall, 3)
    if fill is None:
        return np.zeros(shape)
    return np.random.default_rng(seed).uniform(0.5, 1.5, shape) * fill


def run(ctx, c, style, out, cg_all=None):
    """one style call into `out` (rhosum / colorgradient write, the others add)"""
    if style == "rhosum":
        ctx.rhosum_multiphase(out)
    elif style == "cg":
        ctx.colorgradient(out)
    elif style == "tait":
        ctx.taitwater_multiphase(out)
    elif style == "st":
        ctx.surfacetension(c.cg_all if cg_all is None else cg_all, out)
    else:
        ctx.heatconduction_phasechange(out)
    return out


def stage_list(ctx, sph_amd, c, style):
    off, nb = c.lists(style)
    ctx.list_csr(sph_amd.SPH_LIST_FULL if style in ("rhosum", "cg") else sph_amd.SPH_LIST_HALF,
                 off, nb)
