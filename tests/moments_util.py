"""Reference side of sph_engine_moments / sph_engine_gyration (tests/test_moments_cpu.py,
tests/test_gpu_moments.py): the reference's per-atom terms restated in numpy, one rounding per
operation, and correctly rounded sums of them.

Inputs of one brick: x, v and rho from get_atoms, the images from write_restart's records, the
type and the mass (rmass, or mass[type] on a single-phase engine) from get_atoms_multiphase.

Terms, as the reference writes them (group.cpp, compute_gyration.cpp, domain.cpp:1307-1316):
unwrap = x + xbox * prd, then unwrap * m, v * m, m / rho; for the gyration d = unwrap - cm,
(dx*dx + dy*dy + dz*dz) * m, dx*dx * m ... dy*dz * m.  numpy rounds every one of these
operations on its own, which is what the kernels must reproduce.

Bound of a sum.  The reference value is math.fsum of the terms, the correctly rounded sum.
Any order of summing n terms t_i lies within (n - 1) 2^-53 sum|t_i| of the exact sum to first
order (Higham, Accuracy and Stability of Numerical Algorithms, eq. 4.4); the tests allow
n 2^-52 fsum|t_i|, twice that, for the second-order terms and the rounding of the fsum itself.
count, lo and hi are exact."""
import math

import numpy as np

import pyoracle as po
from forcefix_util import wrapped
from scenarios import c3_system
from setmeso_util import np_selected

IMG_MASK, IMG_MAX, IMG_BITS = 1023, 512, 10   # lmptype.h, LAMMPS_SMALLBIG
SUMS = ("mass", "mx", "mv", "volume")


def unpack_images(packed):
    """packed imageint -> (n, 3) image counts, as Domain::unmap decodes them"""
    p = np.asarray(packed, dtype=np.int64)
    return np.stack([(p & IMG_MASK) - IMG_MAX, ((p >> IMG_BITS) & IMG_MASK) - IMG_MAX,
                     (p >> (2 * IMG_BITS)) - IMG_MAX], 1)


def unwrapped(x, image_xyz, prd):
    """Domain::unmap, orthogonal box: the product rounded, then the add"""
    shift = np.asarray(image_xyz, dtype=np.float64) * np.asarray(prd, dtype=np.float64)
    return np.asarray(x, dtype=np.float64) + shift


def sum_and_bound(terms):
    """(fsum of the terms, n 2^-52 fsum |terms|)"""
    t = np.asarray(terms, dtype=np.float64).ravel()
    return math.fsum(t), t.size * 2.0 ** -52 * math.fsum(np.abs(t))


def moment_terms(inp, prd, images=True):
    """per-atom terms of every sum of sph_moments_out; images=False: a reference that ignores
    the image flags (what the engine must NOT compute)"""
    m = inp["m"]
    u = unwrapped(inp["x"], inp["image"], prd) if images else inp["x"]
    return dict(mass=m, mx=u * m[:, None], mv=inp["v"] * m[:, None], volume=m / inp["rho"])


def gyration_terms(inp, prd, cm, images=True):
    """(n, 7): Group::gyration's term, then compute gyration's xx yy zz xy xz yz"""
    m = inp["m"]
    u = unwrapped(inp["x"], inp["image"], prd) if images else inp["x"]
    dx, dy, dz = u[:, 0] - cm[0], u[:, 1] - cm[1], u[:, 2] - cm[2]
    return np.stack([(dx * dx + dy * dy + dz * dz) * m, dx * dx * m, dy * dy * m, dz * dz * m,
                     dx * dy * m, dx * dz * m, dy * dz * m], 1)


def engine_inputs(eng, sph):
    """one brick's state in set_atoms order: x, v, rho, type, m, image (n, 3)"""
    g = eng.get_atoms()
    mpf = eng.get_atoms_multiphase()
    rec = sph.unpack_restart_records(eng.write_restart())
    assert np.array_equal(rec["x"], g["x"])
    return dict(x=g["x"], v=g["v"], rho=g["rho"], type=mpf["type"], m=mpf["rmass"],
                image=unpack_images(rec["image"]))


def subset(inp, mask):
    return {k: v[mask] for k, v in inp.items()}


def check_moments(got, inp, sel, prd, where=""):
    """one selection's Engine.moments() result against the reference; -> the selected atoms'
    inputs.  Every figure is printed before it is asserted."""
    mask = np_selected(sel, inp["x"], inp["type"])
    sub = subset(inp, mask)
    n = int(mask.sum())
    print(f"{where}: count {got['count']} (want {n})")
    assert got["count"] == n, where
    terms = moment_terms(sub, prd)
    for k in SUMS:
        t = terms[k] if terms[k].ndim == 2 else terms[k][:, None]
        g = np.atleast_1d(got[k])
        for d in range(t.shape[1]):
            want, bound = sum_and_bound(t[:, d])
            print(f"{where}: {k}[{d}] got {g[d]!r} want {want!r} err {abs(g[d] - want):.3e} "
                  f"bound {bound:.3e}")
            assert abs(g[d] - want) <= bound, (where, k, d)
    if n:
        assert np.array_equal(got["lo"], sub["x"].min(0)), where
        assert np.array_equal(got["hi"], sub["x"].max(0)), where
    else:
        assert np.all(got["lo"] == np.inf) and np.all(got["hi"] == -np.inf), where
    return sub


def check_gyration(sums, sub, prd, cm, where=""):
    """sph_engine_gyration's seven sums of one selection about cm against the reference"""
    t = gyration_terms(sub, prd, cm)
    for k in range(7):
        want, bound = sum_and_bound(t[:, k])
        print(f"{where}: gyration[{k}] got {sums[k]!r} want {want!r} "
              f"err {abs(sums[k] - want):.3e} bound {bound:.3e}")
        assert abs(sums[k] - want) <= bound, (where, k)


def same_bits(a, b):
    """two Engine.moments() / Engine.gyration() results, bit for bit"""
    assert len(a) == len(b)
    for p, q in zip(a, b):
        assert p.keys() == q.keys()
        for k in p:
            assert np.asarray(p[k]).tobytes() == np.asarray(q[k]).tobytes(), k


# ---- scenarios ------------------------------------------------------------------------------
def restart_records(s, images, rmass=None):
    """meso restart records (17 doubles) of System s with the given (n, 3) image counts"""
    n = s.n
    return po.pack_restart_meso(s.x, np.arange(1, n + 1), s.type, po.img_pack(images), s.v,
                                s.rho, s.e, s.cv, s.v)


def counted_system(n, seed=2024):
    """n atoms of two types (30 % type 2; masses 1 and 0.5) on the first n sites, in a seeded
    random order, of a jittered cubic lattice in a periodic box of max(7, k) with k^3 >= n
    sites of spacing 1, wrapped into the box; gaussian velocities; rho 1 | 0.5 with a 2 %
    spread"""
    k = 1
    while k ** 3 < n:
        k += 1
    full = wrapped(c3_system(k, seed=seed))
    rng = np.random.default_rng(seed + n)
    pick = np.sort(rng.permutation(full.n)[:n])
    L = float(max(7, k))
    t = np.where(rng.random(n) < 0.3, 2, 1).astype(np.int32)
    rho = np.array([0.0, 1.0, 0.5])[t] * (1.0 + 0.02 * rng.uniform(-1, 1, n))
    return po.System(3, np.zeros(3), np.array([L, L, L]), (1, 1, 1), full.x[pick].copy(),
                     rng.normal(0.0, 0.05, (n, 3)), t, rho, np.array([0.0, 1.0, 2.0])[t],
                     np.ones(n), 2, full.mass.copy())


CROSS_STEPS = 20
CROSS_VX = 75.0          # 20 steps of dt = 1e-3: 1.5 lattice spacings
CROSS_SLABS = ((13.0, 16.0), (5.0, 8.0))


def crossing_system():
    """16x8x8 jittered lattice (two 8^3 halves), all of it translating along +x at CROSS_VX.
    Type 1: the planes x = 13, 14, 15 and x = 5, 6, 7 without thermal motion -- under
    `setforce 0 0 0` they move at exactly (CROSS_VX, 0, 0), the plane x = 15 crosses the
    periodic face at 16 and the plane x = 7 the brick face at 8 of a 2x1x1 decomposition
    within CROSS_STEPS steps (1.5 spacings; the jitter is 0.1).  Type 2: everything else,
    with its thermal velocities on top of the translation."""
    n = 8
    a = wrapped(c3_system(n, seed=12345))
    b = wrapped(c3_system(n, seed=54321))
    x = np.concatenate([a.x, b.x + np.array([float(n), 0.0, 0.0])])
    v = np.concatenate([a.v, b.v])
    N = x.shape[0]
    slab = np.zeros(N, dtype=bool)
    for lo, hi in CROSS_SLABS:
        slab |= (x[:, 0] >= lo - 0.5) & (x[:, 0] < hi - 0.5)
    t = np.where(slab, 1, 2).astype(np.int32)
    v[slab] = 0.0
    v[:, 0] += CROSS_VX
    boxhi = a.boxhi.copy()
    boxhi[0] = 2.0 * n
    rho_t, e_t = np.array([0.0, 1.0, 0.5]), np.array([0.0, 1.0, 2.0])
    s = po.System(3, a.boxlo.copy(), boxhi, (1, 1, 1), x, v, t, rho_t[t].copy(), e_t[t].copy(),
                  np.ones(N), 2, a.mass.copy())
    return s, crossing_physics()


def crossing_physics():
    """sph/rhosum every step + sph/taitwater on both types (C2's physics on two types): rho is
    a function of the positions alone, so a run whose atoms are all force-free has the same
    state on one brick and on several (with rho integrated from drho, setup's forces on moving
    atoms depend on the decomposition in the reference itself)"""
    t = np.zeros((3, 3))
    t[1:, 1:] = 3.0
    v = np.zeros((3, 3))
    v[1:, 1:] = 0.1
    return po.Physics(rhosum_cut=t.copy(), rho0=np.array([0.0, 1.0, 1.0]),
                      c0=np.array([0.0, 10.0, 10.0]), visc=v, tait_cut=t.copy())
