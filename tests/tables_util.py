"""Systems and physics whose per-pair coefficient tables differ in every entry, for the
single-phase kernels (k_rhosum / k_force, the row2 and block passes, sph_hip_build_list and
the engine's rebuild): unequal cuts per type pair and per style, pairs a style has no
coefficients for (cut 0: hybrid/overlay's skip lists), per-type mass / rho / e / rho0 / c0 all
distinct, 3 types or SPH_MAXTYPES = 8 (the typed list entries' three type bits), 3-D and 2-D.

premises() states, on the oracle alone, that the inputs can tell a wrong table entry from the
right one; every test asserts it before it touches the GPU.
"""
from __future__ import annotations

import numpy as np

import pyoracle as po

# per-type values, types 1..8 (index 0 unused): all distinct within each row
MASS = (0.0, 1.0, 0.8, 1.2, 0.9, 1.1, 0.7, 1.3, 0.95)
RHO = (0.0, 1.0, 0.85, 1.15, 0.9, 1.1, 0.8, 1.2, 0.95)
E = (0.0, 1.0, 2.0, 1.5, 2.5, 0.5, 3.0, 1.25, 1.75)
RHO0 = (0.0, 1.0, 0.9, 1.1, 0.95, 1.05, 0.85, 1.15, 0.97)
C0 = (0.0, 10.0, 8.0, 12.0, 9.0, 11.0, 7.0, 13.0, 10.5)

# nt = 3, upper triangle in the order 11 12 13 22 23 33; 0 = the style has no coefficients
# for the pair (every pair keeps a coefficient in another style)
T3 = dict(rhosum_cut=(2.6, 2.4, 2.2, 2.8, 2.0, 2.5),
          tait_cut=(3.0, 2.7, 2.3, 2.5, 0.0, 2.9),
          heat_cut=(2.0, 3.0, 0.0, 2.2, 2.6, 2.4),
          visc=(0.1, 0.05, 0.2, 0.15, 0.0, 0.08),
          alpha=(0.1, 0.2, 0.0, 0.05, 0.15, 0.12))
# nt = 8: cuts and coefficients from this seed; the pairs below are absent, and KEEP8 has no
# rhosum pair at all (its rows keep their rho: the rho_keep bit of a type above 2)
SEED8 = 20260
ABSENT8 = dict(tait_cut=((2, 7), (4, 8)), heat_cut=((1, 8), (3, 5)))
KEEP8 = 6


def _upper(nt, vals):
    t = np.zeros((nt + 1, nt + 1))
    k = 0
    for i in range(1, nt + 1):
        for j in range(i, nt + 1):
            t[i, j] = t[j, i] = vals[k]          # mirrored, as init_one does
            k += 1
    return t


def mixed_system(n, nt, dim=3, seed=4711):
    """po.cubic_lattice(n) with the types drawn uniformly from 1..nt and per-type mass, rho, e
    (MASS, RHO, E)"""
    s = po.cubic_lattice(n, seed=seed, ntypes=nt, dim=dim, mass=MASS[1:nt + 1],
                         rho=RHO[1:nt + 1], e=E[1:nt + 1])
    t = np.random.default_rng(seed + 1).integers(1, nt + 1, s.n).astype(np.int32)
    s.type = t
    s.rho = np.asarray(RHO)[t].copy()
    s.e = np.asarray(E)[t].copy()
    return s


def mixed_physics(nt, morris, heat=True, rhosum=True, scale=1.0):
    """rhosum + taitwater (Monaghan or Morris) + heatconduction with the tables above, cuts
    times `scale` (2.5 / 3 for the 2-D variant)"""
    if nt == 3:
        tab = {k: _upper(3, v) for k, v in T3.items()}
    else:
        assert nt == 8
        rng = np.random.default_rng(SEED8)
        npair = nt * (nt + 1) // 2
        tab = {k: _upper(nt, rng.uniform(2.0, 3.0, npair))
               for k in ("rhosum_cut", "tait_cut", "heat_cut")}
        tab["visc"] = _upper(nt, rng.uniform(0.02, 0.2, npair))
        tab["alpha"] = _upper(nt, rng.uniform(0.02, 0.2, npair))
        for k, pairs in ABSENT8.items():
            for i, j in pairs:
                tab[k][i, j] = tab[k][j, i] = 0.0
                c = "visc" if k == "tait_cut" else "alpha"
                tab[c][i, j] = tab[c][j, i] = 0.0
        tab["rhosum_cut"][KEEP8, :] = 0.0
        tab["rhosum_cut"][:, KEEP8] = 0.0
    for k in ("rhosum_cut", "tait_cut", "heat_cut"):
        tab[k] = tab[k] * scale
    ph = po.Physics(every=5, rhosum_nstep=1 if rhosum else 0,
                    rhosum_cut=tab["rhosum_cut"] if rhosum else None, morris=morris,
                    rho0=np.array(RHO0[:nt + 1]), c0=np.array(C0[:nt + 1]), visc=tab["visc"],
                    tait_cut=tab["tait_cut"], heat=heat, alpha=tab["alpha"] if heat else None,
                    heat_cut=tab["heat_cut"] if heat else None)
    # hybrid/overlay: every pair has coefficients in at least one style that is on
    assert (ph.cutmax(nt)[1:, 1:] > 0).all()
    return ph


def styles(ph):
    """(name, cut table) of the styles that are on"""
    out = []
    if ph.rhosum_nstep > 0:
        out.append(("rhosum", np.asarray(ph.rhosum_cut)))
    if ph.tait:
        out.append(("tait", np.asarray(ph.tait_cut)))
    if ph.heat:
        out.append(("heat", np.asarray(ph.heat_cut)))
    return out


def pair_census(s, ph):
    """every (owned i, owned or ghost j) pair within the largest neighbour cutoff: types and
    distance; and the per-row counts of the per-pair build and of a uniform-cutmax build"""
    nt = s.ntypes
    cns, cmax = po.cutneighsq(nt, ph.cutmax(nt), ph.skin)
    g = po.borders(s, cmax)
    uni = np.zeros_like(cns)
    uni[1:, 1:] = cns.max()
    uoff, unb = po.neigh_full(s.dim, g, nt, uni)
    foff, _ = po.neigh_full(s.dim, g, nt, cns)
    i = np.repeat(np.arange(s.n), np.diff(uoff))
    r = np.sqrt(((g.x[i] - g.x[unb]) ** 2).sum(1))
    return dict(ti=g.type[i], tj=g.type[unb], r=r, rows=np.diff(foff), urows=np.diff(uoff),
                cns=cns)


def premises(s, ph, ref=None, steps=1):
    """Conditions on the inputs, checked on the oracle alone; returns the numbers.

    * per style and type pair with a cut: at least one pair of atoms between that pair's cut
      and the style's largest (the band where another entry of the table changes a term) --
      for the pair that holds the largest cut itself, between the style's smallest cut and it;
    * per absent pair of a style: at least one pair of atoms inside the style's largest cut;
    * the per-row neighbour counts differ from a uniform-cutmax build's on more than half of
      the rows;
    * every type occurs, the last one included;
    * f, drho and de are nonzero and every field is finite, at setup and after `steps` steps
      of an oracle run made here -- or in `ref`, the oracle states a test compares with (one
      or a list of RefRun / snapshots with .field(k))."""
    nt = s.ntypes
    c = pair_census(s, ph)
    out = dict(bands={}, absent={}, rows=(int(c["rows"].min()), int(c["rows"].max())))
    for name, cut in styles(ph):
        pos = cut[1:, 1:][cut[1:, 1:] > 0]
        cmax, cmin = float(pos.max()), float(pos.min())
        for a in range(1, nt + 1):
            for b in range(a, nt + 1):
                m = ((c["ti"] == a) & (c["tj"] == b)) | ((c["ti"] == b) & (c["tj"] == a))
                if cut[a, b] > 0:
                    lo, hi = ((cut[a, b], cmax) if cut[a, b] < cmax else (cmin, cmax))
                    k = int((m & (c["r"] > lo) & (c["r"] < hi)).sum())
                    out["bands"][(name, a, b)] = k
                else:
                    k = int((m & (c["r"] < cmax)).sum())
                    out["absent"][(name, a, b)] = k
                assert k > 0, (name, a, b, float(cut[a, b]))
    out["rows_differ"] = float((c["rows"] != c["urows"]).mean())
    assert out["rows_differ"] > 0.5, out["rows_differ"]
    assert set(np.unique(s.type)) == set(range(1, nt + 1))
    if ref is None:
        ref = po.RefRun(s, ph)
        ref.setup()
        _fields_ok(ref)
        ref.run(steps)
    for r in (ref if isinstance(ref, (list, tuple)) else [ref]):
        _fields_ok(r)
        out["fmax"] = float(np.abs(r.field("f")).max())
    return out


def _fields_ok(r):
    for k in ("f", "drho", "de"):
        assert np.abs(r.field(k)).max() > 0, k
    for k in ("rho", "f", "drho", "de", "x", "v", "e"):
        assert np.isfinite(r.field(k)).all(), k


# ---- the named cases of the pair-layer, engine and oracle-pinning tests ----------------------
def case(name, n=None, rhosum=True):
    """(system, physics) of mixed3 / mixed3_morris / mixed8 / mixed3_2d; n: lattice edge"""
    if name in ("mixed3", "mixed3_morris"):
        return (mixed_system(n or 10, 3, seed=4711),
                mixed_physics(3, morris=name.endswith("morris"), rhosum=rhosum))
    if name in ("mixed8", "mixed8_morris"):
        return (mixed_system(n or 10, 8, seed=4811),
                mixed_physics(8, morris=name.endswith("morris"), rhosum=rhosum))
    assert name == "mixed3_2d"
    return (mixed_system(n or 30, 3, dim=2, seed=4911),
            mixed_physics(3, morris=False, rhosum=rhosum, scale=2.5 / 3.0))


def style_list(g, off, nb, cut):
    """the list a hybrid/overlay sub-style sees (pair_hybrid.cpp:428-485, the SKIP list): of a
    list over all owned rows, the pairs the style has coefficients for, in the list's order;
    the rows of a type without any pair come out empty"""
    off = np.asarray(off, dtype=np.int64)
    cut = np.asarray(cut)
    i = np.repeat(np.arange(len(off) - 1), np.diff(off))
    keep = cut[g.type[i], g.type[nb]] > 0
    cnt = np.bincount(i[keep], minlength=len(off) - 1)
    off2 = np.zeros(len(off), dtype=np.int64)
    off2[1:] = np.cumsum(cnt)
    return off2, np.ascontiguousarray(nb[keep])
