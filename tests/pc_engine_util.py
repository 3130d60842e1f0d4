"""fix phase_change on the device-resident engine beyond the periodic bubble: the cases of
tests/test_gpu_pc_engine.py, their premises (tests/test_pc_engine_cpu.py) and an engine
builder that hands the whole ph.pc dict to Engine.phase_change.

Every other engine test arms the fix through c5_util.mp_engine on bubble_physics: a fully
periodic box, probability mode, Tt = -1, Tc = 0 with all the vapour at T = 0, from 1 to 2 of
two types, atoms at rest, nevery 1.  The cases here each move one of those, and each states
on the oracle alone (premises) that it reaches what it is about -- a premise that fails is a
broken case, to be mended by its seed, dr, rate or Tt, never skipped.

Axis restriction.  insert_one_atom's ownership test (fix_phase_change.cpp:441-452; pc_owns in
csrc/sph_pc.h, pc_mine in the oracle) accepts a coordinate at or beyond boxhi on the top rank
in z (3-D) and in y (2-D).  In a periodic direction the next Domain::pbc wraps such an atom;
in a non-periodic one it would sit outside a fixed box, where LAMMPS loses the atom and the
engine has no defined behaviour.  So every 3-D case keeps z periodic and every 2-D case keeps
y periodic (asserted in premises), and the premises also assert that every atom of the
oracle's run stays inside the box in every non-periodic direction at every step."""
import dataclasses
import functools

import numpy as np

import pyoracle as po
from c5_util import mp_engine
from mp_variants_util import mp_box, mp_physics
from scenarios import bubble_physics, bubble_system

MAX_STEPS = 6
PG_WALLS = (1, 2, 1)


# ------------------------------------------------------------------------------------------
# the engine
# ------------------------------------------------------------------------------------------
def pc_engine(sph, s, ph, procgrid=(1, 1, 1), rank=0, sel=None):
    """c5_util.mp_engine's engine for (s, ph), with fix phase_change armed from the WHOLE
    ph.pc dict: energy_chance, rate and maxattempt too (mp_engine passes prob, nevery and seed
    only).  The defaults are Engine.phase_change's own, so a dict without the three keys arms
    exactly what mp_engine arms."""
    eng = mp_engine(sph, s, dataclasses.replace(ph, pc=None), procgrid=procgrid, rank=rank,
                    sel=sel)
    p = ph.pc
    if p:
        eng.phase_change(p["Tc"], p["Tt"], p["Hwv"], p["dr"], p["to_mass"], p["cutoff"],
                         p["from_type"], p["to_type"], nevery=p.get("nevery", 1),
                         seed=p["seed"], prob=p.get("prob", 0.0),
                         energy_chance=p.get("energy_chance", 0), rate=p.get("rate", 0.0),
                         maxattempt=p.get("maxattempt", 10))
        eng.atom_sort(getattr(ph, "sortfreq", 1000), getattr(ph, "sort_binsize", 0.0))
    return eng


def pc_bricks(sph, s, ph, pg, owner):
    """c5_util.mp_bricks over pc_engine: one engine per brick on a LocalWorld"""
    P = int(np.prod(pg))
    world = sph.LocalWorld(P)
    engines = []
    for r in range(P):
        sel = np.nonzero(owner == r)[0]
        eng = pc_engine(sph, s, ph, procgrid=pg, rank=r, sel=sel)
        eng.comm_local(world, r)
        engines.append(eng)
    return world, engines


# ------------------------------------------------------------------------------------------
# the oracle, with what the premises read
# ------------------------------------------------------------------------------------------
class Probe(po.MpRefRun):
    """MpRefRun that notes, per call of the fix: the step, the owned to_type atoms, the
    flagged candidates (type == to_type and not T < Tc: one Park-Miller draw each) and the
    atoms created; and per step whether every atom was inside the box in the non-periodic
    directions."""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.calls = []

    def _phase_change(self):
        s, p = self.s, self.ph.pc
        n0 = s.n
        to = s.type == p["to_type"]
        flagged = to & ~(s.e / s.cv < p["Tc"])
        nins = super()._phase_change()
        self.calls.append(dict(step=self.step, n_to=int(to.sum()), flagged=int(flagged.sum()),
                               nins=int(nins), x_new=self.s.x[n0:].copy()))
        return nins

    def inside(self):
        s = self.s
        ok = True
        for d in range(s.dim):
            if not s.periodic[d]:
                ok = ok and bool(((s.x[:, d] >= s.boxlo[d]) & (s.x[:, d] < s.boxhi[d])).all())
        return ok


def probe_run(s, ph, steps, procgrid=None):
    ref = Probe(s, ph, procgrid=procgrid)
    ref.setup()
    ref.always_inside = ref.inside()
    for _ in range(steps):
        ref.run(1)
        ref.always_inside = ref.always_inside and ref.inside()
    return ref


def with_pc(ph, **kw):
    """ph with entries of its pc dict replaced"""
    return dataclasses.replace(ph, pc=dict(ph.pc, **kw))


# ------------------------------------------------------------------------------------------
# the cases
# ------------------------------------------------------------------------------------------
def _slab(nx, dim, periodic=None, Tv=None, seed=0, axis=0):
    """bubble_system's jittered slab: vapour in the last layer along `axis` (bubble_system's
    own is x).  Tv: the vapour's temperature, a number or a (lo, hi) range drawn per atom;
    e = cv T (bubble_system: T = Tc = 0, where the sign of the first heat flow decides whether
    an atom is a candidate at all)."""
    s = bubble_system(nx, dim=dim, slab=True)
    if periodic is not None:
        s.periodic = tuple(periodic)
    if axis != 0:
        dx = 1.0 / nx
        vap = s.x[:, axis] > 1.0 - dx
        s.type = np.where(vap, 2, 1).astype(np.int32)
        s.rho = np.where(vap, 0.1, 1.0)
        s.cv = np.where(vap, 0.06, 0.04)
        s.e = np.where(vap, 0.0, 0.04)
        s.rmass = s.rho * dx ** dim
    if Tv is not None:
        vap = s.type == 2
        if np.ndim(Tv):
            T = np.random.default_rng(seed).uniform(Tv[0], Tv[1], int(vap.sum()))
        else:
            T = float(Tv)
        s.e = s.e.copy()
        s.e[vap] = s.cv[vap] * T
    return s


def _rate(ph, e, threshold):
    """the ENERGY rate at which an atom of energy e has `threshold` = (e - Tc cv)/Hwv dt rate
    (Tc = 0 in these cases)"""
    return threshold * ph.pc["Hwv"] / (e * ph.dt)


# the fix's seed per case (default: bubble_physics' 123456), chosen with the other knobs until
# the case's premise holds on the oracle
SEEDS = {"walls-y": 29, "bricks-walls": 29, "giveup": 4711, "walls-2d": 7}


def _types_pc(**kw):
    """fix phase_change on mp_box(ntypes=3): type 3 evaporates into type 2, type 1 inert; Hwv
    small enough that an atom that changed stays above Tc = 0 and draws again.  cutoff 1 = dx:
    the fix hands r * cutoff to the quintic (not r / h), whose support ends at
    r * cutoff = 1, while isfromphasearound asks for r <= cutoff -- with cutoff > 1 a
    candidate can pass that test with no donor of any weight, and W = 0 divides (in the
    reference too).  At 1 about half the candidates have a type-3 atom that near, and those
    have one to three donors; to_mass 0.05 keeps a donor's rmass (>= 0.28) positive."""
    d = dict(Tc=0.0, Tt=-1.0, Hwv=0.05, dr=0.5, to_mass=0.05, cutoff=1.0, from_type=3,
             to_type=2, nevery=1, seed=4711, prob=0.06)
    d.update(kw)
    return d


def _energy(dim):
    nx = 8 if dim == 3 else 12
    s = _slab(nx, dim, Tv=0.5)
    ph = bubble_physics(nx, dim=dim, prob=0.0, Tt=-1.0)
    return s, with_pc(ph, energy_chance=1, rate=_rate(ph, 0.06 * 0.5, 0.3)), 4


def _walls_y(**kw):
    """3-D slab between walls in y, vapour (T = 0.5 > Tc) in the last x layer; dr = 1.5 dx:
    a first placement from the two layers next to a wall can leave the box"""
    s = _slab(8, 3, periodic=(1, 0, 1), Tv=0.5)
    ph = bubble_physics(8, prob=kw.pop("prob", 0.5), Tt=-1.0)
    return s, with_pc(ph, dr=1.5 / 8, **kw), 3


def _make(name):
    if name == "energy":
        return _energy(3)
    if name == "energy-2d":
        return _energy(2)
    if name == "tt":
        return (_slab(8, 3, Tv=(0.2, 0.8), seed=5),
                bubble_physics(8, prob=0.5, Tt=0.5), 4)
    if name == "tc":
        return (_slab(8, 3, Tv=(0.2, 0.8), seed=5),
                with_pc(bubble_physics(8, prob=0.5, Tt=-1.0), Tc=0.5), 4)
    if name in ("walls-y", "bricks-walls"):
        return _walls_y()
    if name == "giveup":
        return _walls_y(maxattempt=1, prob=0.9)
    if name == "walls-2d":
        # walls in x; the vapour in the last y layer, so that the colour gradient points
        # along y and create_newpos (2-D: +-dr across the gradient) places along x
        s = _slab(12, 2, periodic=(0, 1, 0), Tv=0.5, axis=1)
        ph = bubble_physics(12, dim=2, prob=0.5, Tt=-1.0)
        return s, with_pc(ph, dr=1.25 / 12), 3
    if name == "types":
        ph = mp_physics(ntypes=3)
        ph.pc = _types_pc()
        return mp_box(ntypes=3), ph, 6
    if name == "types-to1":
        # (beyond the issue's table: every case above creates type 2, so a walk that held a
        # literal 2 for to_type would pass them all -- here type 3 evaporates into type 1)
        ph = mp_physics(ntypes=3)
        ph.pc = _types_pc(to_type=1, prob=0.04)
        return mp_box(ntypes=3), ph, 4
    if name == "nevery2":
        ph = mp_physics(ntypes=3)
        ph.pc = _types_pc(nevery=2, prob=0.1)
        return mp_box(ntypes=3), ph, 6
    if name == "restart":
        # (Hwv 0.01: an atom that changed keeps T = 1/6 > Tc, so both halves have candidates)
        return (_slab(8, 3, Tv=0.5),
                with_pc(bubble_physics(8, prob=0.1, Tt=-1.0), Hwv=0.01), 6)
    raise KeyError(name)


CASES = ("energy", "energy-2d", "tt", "tc", "walls-y", "giveup", "walls-2d", "types",
         "types-to1", "nevery2", "bricks-walls", "restart")
RESTART_AT = 3


@functools.lru_cache(maxsize=None)
def case(name):
    """(system, physics, steps) of a case, made once; nobody writes to them"""
    s, ph, steps = _make(name)
    if name in SEEDS:
        ph = with_pc(ph, seed=SEEDS[name])
    assert steps <= MAX_STEPS
    return s, ph, steps


def procgrid(name):
    return PG_WALLS if name == "bricks-walls" else None


def restart_system(s, rec):
    """The System an oracle restarts from: the records' atoms in tag order, and the cg and
    vest they carry (read_restart restores both; borders carry vest at setup)."""
    d = po.unpack_restart(rec)
    assert np.array_equal(d["tag"], np.arange(1, rec.shape[0] + 1))
    s2 = s.copy()
    for k in ("x", "v", "rho", "e", "cv", "rmass"):
        setattr(s2, k, np.ascontiguousarray(d[k], dtype=np.float64).copy())
    s2.type = d["type"].astype(np.int32)
    return s2, d["cg"].copy(), d["vest"].copy()


def restart_ref(s2, ph, cg, vest, spread=False, cls=po.MpRefRun):
    ref = cls(s2, ph, cg=cg, spread=spread)
    for r in [ref] + list(ref.alts):
        r.vest = vest.copy()
    return ref


def oracle_records(ref):
    """the oracle's state as restart records (tests/test_restart.py _oracle_records)"""
    s = ref.s
    return po.pack_restart_multiphase(s.x, np.arange(1, s.n + 1), s.type, po.img_pack(ref.image),
                                      s.v, s.rho, ref.cg, s.rmass, s.e, s.cv, ref.vest)


# ------------------------------------------------------------------------------------------
# the premises
# ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _run(name, **kw):
    """the oracle's probe run of a case, with entries of its pc dict replaced by kw"""
    s, ph, steps = case(name)
    return probe_run(s, with_pc(ph, **kw) if kw else ph, steps, procgrid=procgrid(name))


def _differs(a, b):
    return a.s.n != b.s.n or not np.array_equal(a.s.x, b.s.x)


def premises(name):
    """What the case claims to exercise, asserted on the oracle alone.  Returns the figures
    (for the record)."""
    s, ph, steps = case(name)
    p = ph.pc
    ref = _run(name)
    out = dict(n=s.n, ninserted=ref.ninserted, draws=sum(c["flagged"] for c in ref.calls))
    # the axis restriction of the module doc
    assert s.periodic[2 if s.dim == 3 else 1], (name, "z (3-D) / y (2-D) must be periodic")
    assert ref.always_inside, (name, "an atom left the box in a non-periodic direction")
    assert s.n <= 512 and steps <= MAX_STEPS
    assert np.all(np.isfinite(ref.f)) and np.all(ref.s.rmass > 0), name
    assert np.all(ref.s.type[s.n:] == p["to_type"]), name
    if name in ("energy", "energy-2d"):
        assert p["energy_chance"] == 1 and p.get("prob", 0.0) == 0.0
        vap = s.type == p["to_type"]
        thr = (s.e[vap] - p["Tc"] * s.cv[vap]) / p["Hwv"] * ph.dt * p["rate"]
        assert (s.e[vap] / s.cv[vap] > p["Tc"]).all() and 0.2 <= thr.min() <= thr.max() <= 0.5
        assert 1 <= ref.ninserted < out["draws"], (name, out)
        more = _run(name, rate=2.0 * p["rate"])
        assert more.ninserted > ref.ninserted, (name, more.ninserted, ref.ninserted)
        out["ninserted_rate2"] = more.ninserted
    elif name == "tt":
        vap = s.type == 2
        T = s.e[vap] / s.cv[vap]
        assert (T > p["Tt"]).any() and (T < p["Tt"]).any() and (T > p["Tc"]).all()
        free = _run(name, Tt=-1.0)
        assert 1 <= ref.ninserted < free.ninserted, (name, ref.ninserted, free.ninserted)
        out["ninserted_free"] = free.ninserted
    elif name == "tc":
        c0 = ref.calls[0]
        assert p["Tc"] > 0 and c0["step"] == 1
        assert 0 < c0["flagged"] < c0["n_to"], (name, c0)
        assert ref.ninserted >= 1
        out.update(flagged0=c0["flagged"], n_to0=c0["n_to"])
    elif name in ("walls-y", "walls-2d", "giveup", "bricks-walls"):
        assert tuple(s.periodic) == ((1, 0, 1) if s.dim == 3 else (0, 1, 0))
        assert p["dr"] * (8 if s.dim == 3 else 12) >= 1.0 and p.get("energy_chance", 0) == 0
        assert ref.ninserted >= 1
        if name == "giveup":
            assert p["maxattempt"] == 1 and p["prob"] >= 0.5
            full = _run(name, maxattempt=10)
            assert 1 <= ref.ninserted < full.ninserted, (name, ref.ninserted, full.ninserted)
            out["ninserted_attempt10"] = full.ninserted
        else:
            one = _run(name, maxattempt=1)
            assert p.get("maxattempt", 10) == 10 and _differs(one, ref), name
            out["ninserted_attempt1"] = one.ninserted
        if name == "bricks-walls":
            per = np.zeros(int(np.prod(PG_WALLS)), dtype=np.int64)
            for c in ref.calls:
                if c["nins"]:
                    per += np.bincount(po.brick_owner(s, c["x_new"], PG_WALLS),
                                       minlength=per.size)
            assert (per >= 1).all() and per.sum() == ref.ninserted, (name, per)
            out["per_rank"] = per.tolist()
    elif name in ("types", "types-to1", "nevery2"):
        assert s.ntypes == 3 and p["from_type"] == 3
        assert p["to_type"] == (1 if name == "types-to1" else 2)
        assert ph.every == 2 and ph.skin == 0.3 and (ph.rbg[1:] != 0).all()
        assert np.abs(s.v).max() > 0.05
        # a candidate's row holding all three types: the full list at setup
        seen = False
        ref0 = po.MpRefRun(s, dataclasses.replace(ph, pc=None))
        ref0.setup()
        g = ref0.g
        for i in np.nonzero(s.type == p["to_type"])[0][:20]:
            js = ref0.fnb[ref0.foff[i]:ref0.foff[i + 1]]
            seen = seen or set(g.type[js].tolist()) == {1, 2, 3}
        assert seen, name
        if name == "types":
            assert ref.ninserted >= 2
            swapped = _run(name, from_type=1)
            assert _differs(swapped, ref) or not np.array_equal(swapped.s.rmass, ref.s.rmass)
        elif name == "types-to1":
            assert ref.ninserted >= 2 and _differs(_run(name, to_type=2), ref)
        else:
            assert p["nevery"] == 2 and ref.ninserted >= 1
            assert [c["step"] for c in ref.calls] == [1, 3, 5]
            # a call every step meets other candidates
            assert [c["step"] for c in _run(name, nevery=1).calls] == [1, 2, 3, 4, 5, 6]
    elif name == "restart":
        half = probe_run(s, ph, RESTART_AT)
        s2, cg, vest = restart_system(s, oracle_records(half))
        second = restart_ref(s2, ph, cg, vest, cls=Probe)
        second.setup()
        second.run(steps - RESTART_AT)
        assert half.ninserted >= 1 and second.ninserted >= 1
        assert s2.n == s.n + half.ninserted and second.s.n > s2.n
        out.update(ninserted_first=half.ninserted, ninserted_second=second.ninserted)
    else:
        raise KeyError(name)
    return out
