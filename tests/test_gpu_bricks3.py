"""Brick grids with three or more bricks along a dimension, bricks as threads of one process
(tests/test_gpu_bricks.py's driver), against the single-process oracle from rest.

With two bricks along a periodic dimension a brick's lower and upper neighbour are one rank
and every brick sits on a box edge, so these run only here:
  * CommBrick::exchange's two sends per dimension (comm_brick.cpp:634-672: the leavers go to
    both neighbours, each keeps its own; sph_engine::exchange_multi, pg[d] >= 3);
  * borders with sendproc != recvproc: one count exchange and one record exchange carrying two
    different peers, an interior brick (no periodic shift on either side), and in a
    non-periodic dimension a brick that sends both ways between two that send one way;
  * the direct forward's peer grouping with distinct face neighbours (and, on 3x3x1, corner
    ghosts whose origin is a diagonal rank that is no swap neighbour: eight peers);
  * the setup step's reverse comm over swaps with distinct peers;
  * the halo overlap with two different peers in flight.

Bars (the project's): neighbour counts exact, every atom owned by exactly one brick,
sum(nlocal) == n, fields 1e-10 normwise plus conftest.check_fields with the oracle's spread.

Ghost cut = h + skin (3.3, plus the inner rows' margin) at unit spacing: a 12-wide box cut in
3 gives bricks 4 wide, the narrowest whole-plane brick CommBrick's maxneed = 1 allows; cut in 4
it is refused (test_thin_brick_is_refused)."""
import numpy as np
import pytest

import pyoracle as po
from conftest import rel_err
from scenarios import c2_system, c3_system
from test_gpu_bricks import LAST_STATS, TOL, at_rest, compare, run_bricks

pytestmark = pytest.mark.gpu
EINVAL = -1   # SPH_HIP_EINVAL (include/sph_hip.h)


def wrapped(s):
    """s.x wrapped into the box (the lattice's jitter leaves some atoms below 0)"""
    prd = s.boxhi - s.boxlo
    x = s.x.copy()
    for d in range(3):
        if s.periodic[d]:
            x[:, d] = s.boxlo[d] + np.mod(x[:, d] - s.boxlo[d], prd[d])
    return x


def peers(s, cut, pg):
    """Per rank, from the oracle's CommBrick::borders alone: the ranks owning the atoms its
    ghosts image (the direct forward's peers; the rank itself where a ghost images an own
    atom across a dimension with one brick, is left out)."""
    sw = s.copy()
    sw.x = wrapped(s)
    views = po.borders_bricks(sw, cut, pg)
    own = po.brick_owner(sw, sw.x, pg)
    return [sorted(set(own[v.gid[v.nlocal:]].tolist()) - {v.rank}) for v in views]


def ghost_cut(s, ph):
    return po.cutneighsq(s.ntypes, ph.cutmax(s.ntypes), ph.skin)[1]


def reference(s, ph, nsteps):
    ref = po.RefRun(s, ph, spread=True)
    ref.setup()
    ref.run(nsteps)
    return ref


_REF = {}


def c2_ref(n, every=4, nsteps=9):
    """The 9-step C2 reference from rest on the n^3 lattice, computed once per n (the
    single-process oracle does not depend on the grid) and left unchanged."""
    if n not in _REF:
        s = at_rest(c2_system(n))
        ph = po.c2_physics()
        ph.every = every
        _REF[n] = (s, ph, reference(s, ph, nsteps))
    return _REF[n]


def check(sph_amd, s, ph, ref, pg, nsteps, path=0, overlap=False, e=False):
    out, counts, nloc = run_bricks(sph_amd, s, ph, pg, nsteps, path=path, overlap=overlap)
    print(f"PREMISE pg={pg} path={path} n={s.n} nlocal={nloc}")
    assert sum(nloc) == s.n
    assert all(n > 0 for n in nloc)
    assert np.array_equal(counts, ref.numneigh_full())
    compare(out, ref)
    if e:
        assert rel_err(out["e"], ref.s.e) < TOL
    return nloc


@pytest.mark.parametrize("pg,path", [((3, 1, 1), 0), ((1, 1, 3), 0), ((3, 1, 1), 1),
                                     ((1, 1, 3), 1)])
def test_bricks3_periodic_three_along_one_axis(gpu, sph_amd, pg, path):
    """12^3 from rest, rebuilds (and migrations through both exchanges) at steps 4 and 8:
    every brick has two distinct neighbours, brick 1 shifts nothing (interior)."""
    s, ph, ref = c2_ref(12)
    pr = peers(s, ghost_cut(s, ph), pg)
    print(f"PREMISE pg={pg} peers per rank {pr}")
    assert all(len(p) == 2 for p in pr), pr      # lower != upper for every brick
    check(sph_amd, s, ph, ref, pg, 9, path=path)


def test_bricks3_3x3x1_eight_peers(gpu, sph_amd):
    """Nine bricks: a corner ghost's origin is a diagonal rank that no swap reaches directly
    (it arrives forwarded by the y swap), so build_direct groups eight distinct peers."""
    s, ph, ref = c2_ref(12)
    pg = (3, 3, 1)
    pr = peers(s, ghost_cut(s, ph), pg)
    print(f"PREMISE pg={pg} peers per rank {[len(p) for p in pr]}")
    assert all(len(p) == 8 for p in pr), pr
    check(sph_amd, s, ph, ref, pg, 9)


def test_bricks3_four_bricks(gpu, sph_amd):
    """4x1x1 on 16^3: two interior bricks side by side."""
    s, ph, ref = c2_ref(16)
    pg = (4, 1, 1)
    pr = peers(s, ghost_cut(s, ph), pg)
    print(f"PREMISE pg={pg} peers per rank {pr}")
    assert pr == [[1, 3], [0, 2], [1, 3], [0, 2]]
    check(sph_amd, s, ph, ref, pg, 9)


def test_bricks3_uneven_overlap(gpu, sph_amd):
    """3x1x1 on 20^3 with the halo overlap: the faces (20/3, 40/3) fall between lattice
    planes, the bricks hold 7, 7 and 6 of them; bricks 6.67 wide have interior blocks, whose
    passes run while the halos of two different peers are in flight."""
    s, ph, ref = c2_ref(20)
    pg = (3, 1, 1)
    x = wrapped(s)[:, 0]
    planes = [sum(1 for k in range(20) if b["lo"][0] <= k < b["hi"][0])
              for b in po.brick_grid(s, pg)]
    print(f"PREMISE pg={pg} lattice planes per brick {planes}")
    assert planes == [7, 7, 6]
    for face in (20.0 / 3.0, 40.0 / 3.0):
        assert np.abs(x - face).min() > 0.2     # (no plane sits on an inner face)
    nloc = check(sph_amd, s, ph, ref, pg, 9, overlap=True)
    assert len(set(nloc)) > 1
    assert LAST_STATS[0]["staged"] == 1


@pytest.mark.parametrize("pg", [(1, 3, 1), (2, 3, 1)])
def test_bricks3_nonperiodic_interior(gpu, sph_amd, pg):
    """Non-periodic y cut in three: the middle brick sends both ways (sendflag true in both
    directions, no shift), the bricks at the y faces send one way only."""
    s = at_rest(c2_system(12))
    s.periodic = (1, 0, 1)
    s.boxlo[1] -= 2.0
    s.boxhi[1] += 2.0
    ph = po.c2_physics()
    ph.every = 4
    key = "np12"
    if key not in _REF:
        _REF[key] = reference(s, ph, 9)
    ref = _REF[key]
    pr = peers(s, ghost_cut(s, ph), pg)
    print(f"PREMISE pg={pg} nonperiodic y, peers per rank {pr}")
    for r, p in enumerate(pr):   # (rank = y * pg[0] + x)
        rows = {q // pg[0] for q in p}
        if r // pg[0] == 1:
            assert {0, 2} <= rows, (r, p)            # the middle brick meets both edge bricks
        else:
            assert 1 in rows and 2 - r // pg[0] not in rows, (r, p)   # nothing across a y face
    check(sph_amd, s, ph, ref, pg, 9)


@pytest.mark.parametrize("path", [0, 1])
def test_bricks3_c3_heat_two_types(gpu, sph_amd, path):
    """Morris viscosity + heat conduction, two types, on 3x2x1 (three distinct along x, the
    degenerate pair along y in the same run)."""
    if "c3" not in _REF:
        s = at_rest(c3_system(12))
        ph = po.c3_physics()
        ph.every = 3
        _REF["c3"] = (s, ph, reference(s, ph, 7))
    s, ph, ref = _REF["c3"]
    check(sph_amd, s, ph, ref, (3, 2, 1), 7, path=path, e=True)


def test_bricks3_2d(gpu, sph_amd):
    s = at_rest(c2_system(30, dim=2))
    ph = po.c2_physics(2.5)
    ph.every = 4
    ref = reference(s, ph, 9)
    pg = (3, 3, 1)
    pr = peers(s, ghost_cut(s, ph), pg)
    print(f"PREMISE pg={pg} 2d peers per rank {[len(p) for p in pr]}")
    assert all(len(p) == 8 for p in pr), pr
    check(sph_amd, s, ph, ref, pg, 9)


def migration_case():
    """test_bricks_migration's run: pressure-driven motion from rest, dt 5e-3, rebuilds every
    5 of 40 steps.  Returns the reference and, per atom, its brick along x on 3x1x1 at the
    start (after the setup's wrap) and at the end."""
    if "mig" not in _REF:
        s = at_rest(c2_system(12))
        ph = po.c2_physics()
        ph.dt = 5e-3
        ph.every = 5
        ref = po.RefRun(s, ph, spread=True)
        ref.setup()
        b0 = po.brick_owner(s, ref.s.x.copy(), (3, 1, 1))
        ref.run(40)
        b1 = po.brick_owner(s, ref.s.x, (3, 1, 1))
        _REF["mig"] = (s, ph, ref, b0, b1)
    return _REF["mig"]


@pytest.mark.parametrize("path", [0, 1])
def test_bricks3_migration_both_directions(gpu, sph_amd, path):
    """Atoms of the lattice planes on the faces x = 0, 4, 8 cross them between rebuilds, some
    upwards and some downwards: a brick's leavers go to both neighbours in one
    exchange_multi, each of which keeps its own and nothing else."""
    s, ph, ref, b0, b1 = migration_case()
    d = (b1 - b0) % 3
    up, down = int((d == 1).sum()), int((d == 2).sum())
    wrap = int((((b0 == 0) & (b1 == 2)) | ((b0 == 2) & (b1 == 0))).sum())
    print(f"PREMISE migration 3x1x1: {up} up, {down} down, {wrap} across the periodic face")
    assert up >= 1, "no atom moved to its upper neighbour"
    assert down >= 1, "no atom moved to its lower neighbour"
    assert wrap >= 1, "no atom crossed the periodic face between brick 0 and brick 2"
    check(sph_amd, s, ph, ref, (3, 1, 1), 40, path=path)
    if path == 0:  # the inner rows were derived again between rebuilds (ghosts' x0 too)
        assert sum(st["inner_refresh"] for st in LAST_STATS) > 0


def test_thin_brick_is_refused(gpu, sph_amd):
    """CommBrick with maxneed = 1 needs bricks wider than the ghost cut: 12 / 4 = 3 < 3.3 is
    refused at create with SPH_HIP_EINVAL and its message, before anything is launched; the
    same grid on a 16-wide box is accepted (test_bricks3_four_bricks)."""
    s = at_rest(c2_system(12))
    ph = po.c2_physics()
    cfg = sph_amd.make_config(s.dim, s.ntypes, s.boxlo, s.boxhi, s.periodic, s.mass, ph.skin,
                              ph.dt, neigh_every=ph.every, procgrid=(4, 1, 1), rank=0,
                              rhosum=dict(nstep=ph.rhosum_nstep, cut=ph.rhosum_cut),
                              tait=dict(rho0=ph.rho0, c0=ph.c0, visc=ph.visc, cut=ph.tait_cut,
                                        morris=ph.morris))
    with pytest.raises(sph_amd.HipError, match="multi-hop swaps unsupported") as ei:
        sph_amd.Engine(cfg)
    assert ei.value.code == EINVAL
    assert "brick width 3 in dim 0" in str(ei.value)
