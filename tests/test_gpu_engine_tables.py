"""GPU parity of the single-phase engine, both pair paths, with per-pair coefficient tables
whose entries all differ (tables_util: unequal cuts per type pair and per style, absent
pairs, 3 and 8 types, per-type mass / rho / e / rho0 / c0 distinct, 3-D and 2-D).  The engine
re-lays the caller's tables from the (SPH_MAXTYPES+1)^2 ABI layout into the (ntypes+1)^2 one
the kernels index, tests list membership per type pair at every rebuild (k_blk_build /
k_blk_neigh, the inner rows' cutinsq) and packs type - 1 into three bits of a list entry;
every other engine test runs with at most two types and equal entries.

The reference is pyoracle.RefRun(spread=True), pinned to the reference's compiled styles on
these tables by test_oracle_golden.test_oracle_vs_reference_pair_tables.  Bars are
test_gpu_engine's: neighbour counts bit-exact per particle, rho f drho de x v e at 1e-10
normwise plus conftest.check_fields' elementwise bar.  Every case asserts
tables_util.premises on the oracle before it touches the GPU; what the block path reported
is printed (pytest -rP shows it).
"""
import numpy as np
import pytest

import pyoracle as po
import tables_util as tu
from conftest import rel_err
from test_gpu_block_paths import check_step, flag_names, oracle_snaps, report
from test_gpu_bricks import at_rest, run_bricks
from test_gpu_bricks import compare as compare_bricks
from test_gpu_engine import engine_for

pytestmark = pytest.mark.gpu

STEPS = 7    # every = 5: a rebuild at step 5, compared two steps past it
_CACHE = {}


def scenario(name, rhosum=True):
    """(system, physics, oracle snapshots at setup / step 1 / step STEPS, the largest
    displacement since the last rebuild); the oracle runs once per session and the premises
    are asserted on it"""
    key = (name, rhosum)
    if key not in _CACHE:
        s, ph = tu.case(name, rhosum=rhosum)
        assert ph.every + 2 <= STEPS
        snaps, moved = oracle_snaps(s, ph, (1, STEPS))
        tu.premises(s, ph, ref=[snaps[0], snaps[1], snaps[STEPS]])
        _CACHE[key] = (s, ph, snaps, moved)
    return _CACHE[key]


def run_case(sph_amd, what, s, ph, snaps, path, at, sort=1, umf=0):
    eng = engine_for(sph_amd, s, ph, sort=sort, kernel_path=path)
    if umf:
        eng.tune(eng.TUNE_BLKUMF, umf)
    eng.setup()
    seen = 0
    done = 0
    for k in at:
        if k > done:
            eng.run(k - done)
            done = k
        st = eng.stats()
        seen |= st["flags"]
        if path == 0:
            report(f"{what} path 0 sort {sort} umf {umf} step {k}", eng, st)
            assert st["staged"] == 1
            if umf:
                assert st["blk_nbig"] > 0
        check_step(eng, snaps[k], path=path)
    assert st["step"] == at[-1]
    if at[-1] > ph.every:
        assert st["nbr_builds"] >= 2               # (the rebuild inside the run)
    return eng, st, seen


@pytest.mark.parametrize("path", [0, 1])
@pytest.mark.parametrize("name", ["mixed3", "mixed3_morris"])
def test_mixed3(gpu, sph_amd, name, path):
    """three types, rhosum + taitwater (Monaghan / Morris) + heat conduction: setup, step 1
    and step 7, two steps past the rebuild.  The Monaghan case must end on the inner rows
    (cutinsq per type pair): no atom of the oracle moves past half their margin after the
    rebuild."""
    s, ph, snaps, moved = scenario(name)
    assert moved < 0.5 * 0.0625 * ph.skin, moved
    eng, st, _ = run_case(sph_amd, name, s, ph, snaps, path, (0, 1, STEPS))
    if path == 0 and name == "mixed3":
        assert st["inner_rows"] == 1 and st["inner_live"] == 1


@pytest.mark.parametrize("path", [0, 1])
def test_mixed3_without_rhosum(gpu, sph_amd, path):
    """rhosum_nstep = 0: rho evolves by drho from the per-type initial values, the neighbour
    cutoffs come from the taitwater and heat tables alone"""
    s, ph, snaps, moved = scenario("mixed3", rhosum=False)
    assert ph.rhosum_nstep == 0
    run_case(sph_amd, "mixed3 no rhosum", s, ph, snaps, path, (0, 1, STEPS))


@pytest.mark.parametrize("path", [0, 1])
def test_mixed8(gpu, sph_amd, path):
    """SPH_MAXTYPES types (type 8 fills the list entries' three type bits), two absent pairs
    each in taitwater and heat conduction, one type without any rhosum pair, whose rows keep
    their rho"""
    s, ph, snaps, moved = scenario("mixed8")
    keep = ph.rho_keep(8)[s.type]
    assert keep.any() and s.type.max() == 8
    run_case(sph_amd, "mixed8", s, ph, snaps, path, (0, STEPS))


@pytest.mark.parametrize("path", [0, 1])
def test_mixed3_2d(gpu, sph_amd, path):
    s, ph, snaps, moved = scenario("mixed3_2d")
    assert s.dim == 2
    run_case(sph_amd, "mixed3 2-D", s, ph, snaps, path, (0, STEPS))


def test_mixed3_windowed_walk(gpu, sph_amd):
    """the force pass's LDS image capped at 64 records: the windowed walk reads the per-pair
    records too"""
    s, ph, snaps, moved = scenario("mixed3")
    eng, st, _ = run_case(sph_amd, "mixed3", s, ph, snaps, 0, (0, 1, STEPS), umf=64)
    assert st["blk_nbig"] > 0


def test_mixed3_unsorted(gpu, sph_amd):
    """sort = 0: blocks of rows far apart, too wide for the build's small candidate image --
    the large-image bitmap build (k_blk_neigh) tests membership per type pair too"""
    s, ph, snaps, moved = scenario("mixed3")
    eng, st, seen = run_case(sph_amd, "mixed3", s, ph, snaps, 0, (0, 1, STEPS), sort=0)
    print(f"[pair tables] mixed3 sort 0: flags over the run {flag_names(eng, seen)}")
    assert seen & eng.STAT_BLK_BIGIMG, flag_names(eng, seen)


@pytest.mark.parametrize("path", [0, 1])
def test_bricks_mixed3(gpu, sph_amd, path):
    """two bricks (a local world): the halo atoms of every type reach the tables"""
    s, ph = tu.case("mixed3")
    s = at_rest(s)
    ph.every = 3
    ref = po.RefRun(s, ph, spread=True)
    ref.setup()
    ref.run(7)
    tu.premises(s, ph, ref=ref)
    half = s.x[:, 0] < 0.5 * (s.boxlo[0] + s.boxhi[0])
    for t in (1, 2, 3):     # every type on both sides of the face
        assert (s.type[half] == t).any() and (s.type[~half] == t).any()
    out, counts, nloc = run_bricks(sph_amd, s, ph, (2, 1, 1), 7, path=path)
    assert sum(nloc) == s.n
    assert np.array_equal(counts, ref.numneigh_full())
    compare_bricks(out, ref)
    assert rel_err(out["e"], ref.s.e) < 1e-10
