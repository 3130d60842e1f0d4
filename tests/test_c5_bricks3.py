"""C5 (bubble_growth stack + fix phase_change) on grids with three bricks along a dimension,
against the oracle's per-rank emulation (pyoracle.MpRefRun(procgrid=...)); the driver and
the bars are tests/test_c5_bricks.py's.

Three bricks along a periodic dimension give every brick two different neighbours, which the
2-brick grids cannot: CommBrick::exchange then sends a rank's leavers to both (comm_brick.cpp:
634-672) and appends what it keeps of the UPPER neighbour's buffer before the lower one's, so
the arrivals' local order -- the order fix phase_change meets its candidates in, and the
order of the ghost slots on the neighbours -- tells the two exchanges apart; the dmass reverse
comm and the slot keys run over swaps with distinct peers and an interior brick.

The unit box has h = 3 / nx and skin 0: a third of the box exceeds h from nx = 10 (0.333 >
0.3); nx = 12 (3D) and 16 (2D) leave margin."""
import dataclasses

import numpy as np
import pytest

import pyoracle as po
from c5_util import bricks_step, mp_bricks, mp_collect
from scenarios import bubble_physics, bubble_system, shuffled
from test_c5_bricks import _compare


def counterflow(s, vx, dx0):
    """The lower half in y moving along +x at vx and shifted by +dx0, the upper half along -x
    and shifted by -dx0, both wrapped into the box: every brick face is crossed upwards and
    downwards in the same CommBrick::exchange (scenarios.drifting moves everything one way)."""
    s = s.copy()
    lo, hi = s.boxlo[0], s.boxhi[0]
    up = s.x[:, 1] < 0.5 * (s.boxlo[1] + s.boxhi[1])
    x = s.x[:, 0] + np.where(up, dx0, -dx0)
    x = np.where(x >= hi, x - (hi - lo), x)
    s.x[:, 0] = np.where(x < lo, x + (hi - lo), x)
    s.v[:, 0] += np.where(up, vx, -vx)
    return s


def arrivals_by_side(ref, before, pg, d=0):
    """From the oracle's local orders before and after a step: per rank, how many of its
    arrivals were owned by its lower and by its upper neighbour along d (created atoms, which
    no rank owned before, are neither)."""
    grid = po.brick_grid(ref.s, pg)
    was = {}
    for r, l in enumerate(before):
        for i in l:
            was[int(i)] = r
    out = []
    for r, l in enumerate(ref.local):
        src = [was.get(int(i), -1) for i in l]
        out.append((sum(1 for q in src if q == grid[r]["neigh"][d, 0] and q != r),
                    sum(1 for q in src if q == grid[r]["neigh"][d, 1] and q != r)))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("nx,dim,slab,pg,strict", [
    (12, 3, False, (3, 1, 1), False), (16, 2, False, (3, 3, 1), False),
    (12, 3, True, (3, 1, 1), True), (16, 2, True, (3, 3, 1), True)])
def test_c5_bricks3_vs_oracle(gpu, sph_amd, nx, dim, slab, pg, strict):
    """test_c5_bricks_vs_oracle's shapes (the lattice bubble; the jittered slab under the
    plain 1e-10) on 3x1x1 and 3x3x1: setup + 4 single steps, compared after each."""
    s = bubble_system(nx, dim=dim, slab=slab)
    ph = bubble_physics(nx, dim=dim, prob=0.3 if slab else 0.5, Tt=-1.0)
    ref = po.MpRefRun(s, ph, procgrid=pg, spread=True)
    ref.setup()
    owner = po.brick_owner(s, s.x, pg)
    world, engines = mp_bricks(sph_amd, s, ph, pg, owner)
    try:
        bricks_step(engines, lambda e: e.setup())
        _compare(mp_collect(engines, ref.s.n), ref, strict)
        for _ in range(4):
            ref.run(1)
            bricks_step(engines, lambda e: e.run(1))
            _compare(mp_collect(engines, ref.s.n), ref, strict)
        print(f"PREMISE c5 nx={nx} dim={dim} slab={slab} pg={pg} ninserted={ref.ninserted} "
              f"nlocal={[e.nlocal for e in engines]}")
        assert ref.ninserted >= 2
    finally:
        for e in engines:
            e.close()
        world.close()


def counterflow_case(sortfreq, nx=12):
    """A vapour sphere of radius 0.25 reaching across both inner faces of 3x1x1 (x = 1/3, 2/3),
    read in a shuffled order, its halves in y flowing against each other.  Tc = Tt = -1000
    keeps every vapour atom a candidate at every step (at the bubble's Tc = 0 the first
    insertions cool all of them below Tc and nothing is drawn after step 1), so the ranks'
    RanPark streams meet the arrivals of the first exchange, vapour atoms from both sides,
    in local order at every later step: with the two received buffers appended the other
    way round the oracle itself creates other atoms from step 3 on
    (tests/test_pc_bricks_oracle.py::test_counterflow_depends_on_arrival_order)."""
    s = counterflow(shuffled(bubble_system(nx, rv=0.25), 3), 200.0, 0.49 / nx)
    ph = bubble_physics(nx, prob=0.05, Tt=-1000.0)
    ph.pc["Tc"] = -1000.0
    return s, dataclasses.replace(ph, sortfreq=sortfreq)


@pytest.mark.gpu
@pytest.mark.parametrize("sortfreq", [4, 0])
def test_c5_bricks3_migration_local_order(gpu, sph_amd, sortfreq):
    """Counter-flowing halves on 3x1x1: in one exchange a rank receives atoms from its lower
    and from its upper neighbour, appended upper first; fix phase_change then meets them in
    that order (with sortfreq 0 for good, with 4 until and within the bins of Atom::sort)."""
    pg = (3, 1, 1)
    s, ph = counterflow_case(sortfreq)
    ref = po.MpRefRun(s, ph, procgrid=pg, spread=True)
    ref.setup()
    own0 = po.brick_owner(s, s.x, pg)
    world, engines = mp_bricks(sph_amd, s, ph, pg, own0)
    both, nins = [], []
    try:
        bricks_step(engines, lambda e: e.setup())
        _compare(mp_collect(engines, ref.s.n), ref)
        for _ in range(8):
            before = [l.copy() for l in ref.local]
            ref.run(1)
            both.append(arrivals_by_side(ref, before, pg))
            nins.append(ref.ninserted)
            bricks_step(engines, lambda e: e.run(1))
            _compare(mp_collect(engines, ref.s.n), ref)
        print(f"PREMISE c5 counterflow sortfreq={sortfreq} arrivals (lower, upper) per rank "
              f"per step {both} ninserted by step {nins}")
        # the first exchange carried arrivals from both sides to one rank (to every rank: 72
        # and 72), and atoms were created at the steps after it
        assert any(lo > 0 and up > 0 for lo, up in both[0])
        assert nins[-1] > nins[1] >= 2
        moved = po.brick_owner(s, ref.s.x[:s.n], pg) != own0
        assert moved.sum() >= 10
    finally:
        for e in engines:
            e.close()
        world.close()
