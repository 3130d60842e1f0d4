// sph_fix_kernels.h -- streaming kernels of the engine beside the integrator: the fix
// setmeso / setmesode clamps (one pass over the owned rows after the pair compute), the
// group reductions of the thermo output (a fixed-shape two-stage reduction, no atomics), the
// fix setforce / addforce pass of the same post_force slot with its foriginal tallies, and
// fix ave/spatial's layer profiles (rows sorted by layer, each layer folded in a fixed shape).
// Layout as in sph_kernels.h: rho lives in vr[i].w; xf[i].w is the single-phase Tait term
// p/rho^2 derived from it, which the clamp keeps in step with a clamped rho.
#pragma once
#include <hip/hip_runtime.h>

#include "sph_kernels.h"

namespace sph {

// Region::match (region.cpp:127-131) over RegSphere::inside (region_sphere.cpp:96-105) and
// RegBlock::inside (region_block.cpp:114-119), closed boundaries as there
__device__ __forceinline__ bool region_match(const sph_region &r, double x, double y, double z) {
  bool inside;
  if (r.style == SPH_REGION_SPHERE) {
    const double dx = x - r.xc, dy = y - r.yc, dz = z - r.zc;
    inside = sqrt(dx * dx + dy * dy + dz * dz) <= r.radius;
  } else {
    inside = x >= r.xlo && x <= r.xhi && y >= r.ylo && y <= r.yhi && z >= r.zlo && z <= r.zhi;
  }
  return !(inside ^ (r.interior != 0));
}

// group (type_mask, 0 = all) and region (mode 0 none, 1 where match, 2 where !match)
__device__ __forceinline__ bool selected(int type_mask, int region_mode, const sph_region &r,
                                         int t, const double4 &x) {
  if (type_mask && !((type_mask >> t) & 1)) return false;
  if (region_mode == 0) return true;
  const bool m = region_match(r, x.x, x.y, x.z);
  return region_mode == 1 ? m : !m;
}

struct SetMesoArgs {
  int nfix;
  sph_setmeso fix[SPH_MAX_SETMESO];
};

// FixSetMeso::post_force / FixSetMesodE::post_force (constant style) of every armed fix, in
// call order, on the owned rows.  cv == nullptr: cv_const for every atom (single-phase
// engines).  eos != nullptr (single-phase taitwater): xf.w follows a clamped rho.  A thread
// whose atom no fix selects stores nothing.
static __global__ void __launch_bounds__(256)
k_setmeso(int n, SetMesoArgs a, double4 *__restrict__ xf, double4 *__restrict__ vr,
          double *__restrict__ en, double *__restrict__ de, const int *__restrict__ ty,
          const double *__restrict__ cv, double cv_const, const Coefs *__restrict__ eos) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int t = ty[i];
  const double4 x = xf[i];
  bool set_rho = false, set_e = false, set_de = false;
  double rho = 0.0, e = 0.0, dei = 0.0;
  for (int k = 0; k < a.nfix; k++) {
    const sph_setmeso &f = a.fix[k];
    if (!selected(f.type_mask, f.region_mode, f.region, t, x)) continue;
    switch (f.what) {
      case SPH_SET_RHO:
        rho = f.value;
        set_rho = true;
        break;
      case SPH_SET_E:
        e = f.value;
        set_e = true;
        break;
      case SPH_SET_T:
        e = (cv ? cv[i] : cv_const) * f.value;
        set_e = true;
        break;
      default:
        dei = f.value;
        set_de = true;
        break;
    }
  }
  if (set_rho) {
    vr[i].w = rho;
    if (eos) xf[i].w = tait_p_over_rho2(rho, eos->rho0[t], eos->B[t]);
  }
  if (set_e) en[i] = e;
  if (set_de) de[i] = dei;
}

// ---- group reductions -------------------------------------------------------------------
struct ReduceArgs {
  int nsel;
  sph_reduce_sel sel[SPH_MAX_REDUCE];
};
struct StepMass {  // per-type mass (engines without per-atom rmass)
  double mass[MAXT + 1];
};
struct ReducePart {
  double sum, mn, mx;
  long long cnt;
};
constexpr int SPH_NQ = SPH_Q_VZ + 1;  // the SPH_Q_* quantities
constexpr int RED_THREADS = 256;  // four wave64
constexpr int RED_MAXBLOCKS = 512;

__device__ __forceinline__ void red_fold(ReducePart &a, const ReducePart &b) {
  a.sum += b.sum;
  a.mn = fmin(a.mn, b.mn);
  a.mx = fmax(a.mx, b.mx);
  a.cnt += b.cnt;
}

// Stage 1: each thread folds its grid-stride slice of the owned atoms in index order, the
// wave folds by cross-lane shuffles (lane l takes lane l + d, d = 32 .. 1), the block's
// four waves through LDS in wave order; part[block * SPH_MAX_REDUCE + s] takes the block's
// partial of selection s.  The shape depends on (n, grid) alone, so the result's bits do too.
static __global__ void __launch_bounds__(RED_THREADS)
k_reduce_part(int n, ReduceArgs a, const double4 *__restrict__ xf,
              const double4 *__restrict__ vr, const double *__restrict__ en,
              const double *__restrict__ de, const int *__restrict__ ty,
              const double4 *__restrict__ vel, const double *__restrict__ rm,
              const double *__restrict__ cv, double cv_const, StepMass sm,
              ReducePart *__restrict__ part) {
  __shared__ ReducePart s_p[RED_THREADS / 64][SPH_MAX_REDUCE];
  ReducePart acc[SPH_MAX_REDUCE];
#pragma unroll
  for (int s = 0; s < SPH_MAX_REDUCE; s++) acc[s] = ReducePart{0.0, HUGE_VAL, -HUGE_VAL, 0};
  const int stride = gridDim.x * blockDim.x;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const int t = ty[i];
    const double4 x = xf[i];
    const double4 v = vel[i];
    const double m = rm ? rm[i] : sm.mass[t];
    const double ei = en[i];
    double q[SPH_NQ];
    q[SPH_Q_ONE] = 1.0;
    q[SPH_Q_RHO] = vr[i].w;
    q[SPH_Q_E] = ei;
    q[SPH_Q_T] = ei / (cv ? cv[i] : cv_const);
    q[SPH_Q_DE] = de[i];
    q[SPH_Q_MASS] = m;
    q[SPH_Q_KE] = 0.5 * m * (v.x * v.x + v.y * v.y + v.z * v.z);
    q[SPH_Q_VX] = v.x;
    q[SPH_Q_VY] = v.y;
    q[SPH_Q_VZ] = v.z;
#pragma unroll
    for (int s = 0; s < SPH_MAX_REDUCE; s++) {
      if (s >= a.nsel) continue;
      const sph_reduce_sel &c = a.sel[s];
      if (!selected(c.type_mask, c.region_mode, c.region, t, x)) continue;
      double val = q[0];
#pragma unroll
      for (int k = 1; k < SPH_NQ; k++) val = c.quantity == k ? q[k] : val;
      acc[s].sum += val;
      acc[s].mn = fmin(acc[s].mn, val);
      acc[s].mx = fmax(acc[s].mx, val);
      acc[s].cnt += 1;
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int s = 0; s < SPH_MAX_REDUCE; s++) {
    if (s >= a.nsel) continue;  // (uniform over the grid)
    ReducePart p = acc[s];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      ReducePart o;
      o.sum = __shfl_down(p.sum, d, 64);
      o.mn = __shfl_down(p.mn, d, 64);
      o.mx = __shfl_down(p.mx, d, 64);
      o.cnt = __shfl_down(p.cnt, d, 64);
      red_fold(p, o);
    }
    if (lane == 0) s_p[wave][s] = p;
  }
  __syncthreads();
  if ((int)threadIdx.x < a.nsel) {
    ReducePart p = s_p[0][threadIdx.x];
    for (int w = 1; w < RED_THREADS / 64; w++) red_fold(p, s_p[w][threadIdx.x]);
    part[(size_t)blockIdx.x * SPH_MAX_REDUCE + threadIdx.x] = p;
  }
}

// Stage 2 (one block): thread s folds selection s over the blocks' partials in block order
static __global__ void k_reduce_final(int nblocks, int nsel, const ReducePart *__restrict__ part,
                                      sph_reduce_out *__restrict__ out) {
  const int s = threadIdx.x;
  if (s >= nsel) return;
  ReducePart p{0.0, HUGE_VAL, -HUGE_VAL, 0};
  for (int b = 0; b < nblocks; b++) red_fold(p, part[(size_t)b * SPH_MAX_REDUCE + s]);
  out[s].sum = p.sum;
  out[s].min = p.mn;
  out[s].max = p.mx;
  out[s].count = p.cnt;
}

// ---- thermo sums (sph_engine_thermo) -----------------------------------------------------------
// The pair virial of a due step and the kinetic and gravity sums, in k_reduce_part's fixed
// shape: stage 1 leaves part[block * NS + j], the one-block stage 2 folds the blocks in block
// order.  No atomics; the bits depend on (n, grid) alone.
constexpr int VIR_NS = 6;  // xx yy zz xy xz yz
constexpr int TH_NS = 8;   // sum m v_a v_b (the same six), sum m |v|^2 / 2, -sum m (g . x)

// the block's fold of each thread's NS accumulators: shuffles, then the waves through LDS
template <int NS>
__device__ __forceinline__ void slots_block_fold(const double (&acc)[NS],
                                                 double *__restrict__ part) {
  __shared__ double s_p[RED_THREADS / 64][NS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < NS; j++) {
    double p = acc[j];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) p += __shfl_down(p, d, 64);
    if (lane == 0) s_p[wave][j] = p;
  }
  __syncthreads();
  if ((int)threadIdx.x < NS) {
    double p = s_p[0][threadIdx.x];
    for (int w = 1; w < RED_THREADS / 64; w++) p += s_p[w][threadIdx.x];
    part[(size_t)blockIdx.x * NS + threadIdx.x] = p;
  }
}

// stage 1 of the virial: the owned rows' shares w[6 i ..] as the force pass stored them
// (k_force / k_row2_force / blk_force_body VIR), each thread its grid-stride slice in row order
static __global__ void __launch_bounds__(RED_THREADS)
k_virial_part(int n, const double *__restrict__ w, double *__restrict__ part) {
  double acc[VIR_NS] = {};
  const int stride = gridDim.x * blockDim.x;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
#pragma unroll
    for (int j = 0; j < VIR_NS; j++) acc[j] += w[(size_t)i * VIR_NS + j];
  }
  slots_block_fold<VIR_NS>(acc, part);
}

// stage 1 of the kinetic and gravity sums over the owned atoms: v is atom->v (not vest), x the
// wrapped position, m = rmass (rm != nullptr) or mass[type]; gmask: the types of the gravity
// fix's group (cfg.gravity_mask, 0 = every type).  FixGravity::compute_scalar
// (fix_gravity.cpp:272-291): egrav -= massone * (xacc x + yacc y + zacc z).
static __global__ void __launch_bounds__(RED_THREADS)
k_thermo_part(int n, const double4 *__restrict__ xf, const int *__restrict__ ty,
              const double4 *__restrict__ vel, const double *__restrict__ rm, StepMass sm,
              int gmask, double gx, double gy, double gz, double *__restrict__ part) {
  double acc[TH_NS] = {};
  const int stride = gridDim.x * blockDim.x;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const int t = ty[i];
    const double4 x = xf[i];
    const double4 v = vel[i];
    const double m = rm ? rm[i] : sm.mass[t];
    const double mg = (gmask == 0 || ((gmask >> t) & 1)) ? m : 0.0;
    acc[0] += m * v.x * v.x;
    acc[1] += m * v.y * v.y;
    acc[2] += m * v.z * v.z;
    acc[3] += m * v.x * v.y;
    acc[4] += m * v.x * v.z;
    acc[5] += m * v.y * v.z;
    acc[6] += 0.5 * m * (v.x * v.x + v.y * v.y + v.z * v.z);
    acc[7] -= mg * (gx * x.x + gy * x.y + gz * x.z);
  }
  slots_block_fold<TH_NS>(acc, part);
}

// stage 2 (one block): thread j folds slot j over the blocks' partials in block order
static __global__ void k_slots_final(int nblocks, int ns, double scale,
                                     const double *__restrict__ part, double *__restrict__ out) {
  const int j = threadIdx.x;
  if (j >= ns) return;
  double p = 0.0;
  for (int b = 0; b < nblocks; b++) p += part[(size_t)b * ns + j];
  out[j] = scale * p;
}

// ---- fix setforce / fix addforce ------------------------------------------------------------
struct ForceFixArgs {
  int nfix;
  int active;  // bit k: fix k applies in this step (ntimestep % nevery == 0)
  sph_forcefix fix[SPH_MAX_FORCEFIX];
};
constexpr int FF_NT = SPH_MAX_FORCEFIX * 3;  // the tallies: (fix, component)

// FixSetForce::post_force / FixAddForce::post_force (constant style) of every active fix, in
// call order, on one atom's force; TALLY: acc[3 k + d] += the force as fix k found it
// (foriginal).  Returns whether a fix selected the atom.  per_mass: the product is rounded on
// its own (`variable bodyfx atom mass*${gx}`, then f += sforce), never contracted into the add.
template <bool TALLY>
__device__ __forceinline__ bool forcefix_chain(const ForceFixArgs &a, int t, const double4 &x,
                                               double m, double &fx, double &fy, double &fz,
                                               double *acc) {
  bool hit = false;
#pragma unroll
  for (int k = 0; k < SPH_MAX_FORCEFIX; k++) {
    if (k >= a.nfix || !((a.active >> k) & 1)) continue;
    const sph_forcefix &f = a.fix[k];
    if (!selected(f.type_mask, f.region_mode, f.region, t, x)) continue;
    hit = true;
    if (TALLY && f.tally) {
      acc[3 * k] += fx;
      acc[3 * k + 1] += fy;
      acc[3 * k + 2] += fz;
    }
    if (f.kind == SPH_FF_SET) {
      if (f.comp_mask & 1) fx = f.value[0];
      if (f.comp_mask & 2) fy = f.value[1];
      if (f.comp_mask & 4) fz = f.value[2];
    } else if (f.per_mass) {
      fx += __dmul_rn(m, f.value[0]);
      fy += __dmul_rn(m, f.value[1]);
      fz += __dmul_rn(m, f.value[2]);
    } else {
      fx += f.value[0];
      fy += f.value[1];
      fz += f.value[2];
    }
  }
  return hit;
}

// the fixes on the owned rows: f's x, y, z only (fo.w is a single-phase engine's drho); a
// thread whose atom no fix selects stores nothing.  rm == nullptr: mass[type]
static __global__ void __launch_bounds__(256)
k_forcefix(int n, ForceFixArgs a, const double4 *__restrict__ xf, const int *__restrict__ ty,
           const double *__restrict__ rm, StepMass sm, double4 *__restrict__ fo) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int t = ty[i];
  const double4 f = fo[i];
  double fx = f.x, fy = f.y, fz = f.z;
  if (!forcefix_chain<false>(a, t, xf[i], rm ? rm[i] : sm.mass[t], fx, fy, fz, nullptr)) return;
  fo[i].x = fx;
  fo[i].y = fy;
  fo[i].z = fz;
}

// foriginal of the tallying fixes, before k_forcefix changes f: the chain again on a copy of
// each atom's force, summed in k_reduce_part's fixed shape (grid-stride slices in index order,
// cross-lane shuffles, the waves through LDS); part[block * FF_NT + 3 k + d]
static __global__ void __launch_bounds__(RED_THREADS)
k_forcefix_tally(int n, ForceFixArgs a, const double4 *__restrict__ xf,
                 const int *__restrict__ ty, const double *__restrict__ rm, StepMass sm,
                 const double4 *__restrict__ fo, double *__restrict__ part) {
  __shared__ double s_p[RED_THREADS / 64][FF_NT];
  double acc[FF_NT];
#pragma unroll
  for (int j = 0; j < FF_NT; j++) acc[j] = 0.0;
  const int stride = gridDim.x * blockDim.x;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const int t = ty[i];
    const double4 f = fo[i];
    double fx = f.x, fy = f.y, fz = f.z;
    forcefix_chain<true>(a, t, xf[i], rm ? rm[i] : sm.mass[t], fx, fy, fz, acc);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < FF_NT; j++) {
    double p = acc[j];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) p += __shfl_down(p, d, 64);
    if (lane == 0) s_p[wave][j] = p;
  }
  __syncthreads();
  if ((int)threadIdx.x < FF_NT) {
    double p = s_p[0][threadIdx.x];
    for (int w = 1; w < RED_THREADS / 64; w++) p += s_p[w][threadIdx.x];
    part[(size_t)blockIdx.x * FF_NT + threadIdx.x] = p;
  }
}

// one block: thread 3 k + d folds the blocks' partials in block order; only the fixes that
// tallied in this post_force are written (the others keep their last sums)
static __global__ void k_forcefix_final(int nblocks, ForceFixArgs a,
                                        const double *__restrict__ part,
                                        double *__restrict__ tot) {
  const int j = threadIdx.x;
  if (j >= FF_NT) return;
  const int k = j / 3;
  if (k >= a.nfix || !((a.active >> k) & 1) || !a.fix[k].tally) return;
  double p = 0.0;
  for (int b = 0; b < nblocks; b++) p += part[(size_t)b * FF_NT + j];
  tot[j] = p;
}

// ---- layer profiles (fix ave/spatial) ---------------------------------------------------------
struct ProfileArgs {
  sph_profile p;
  double boxlo, boxhi, prd;  // along p.axis
  int periodic;
};

// the layer of each owned atom (fix_ave_spatial.cpp:1006-1013), nlayers for an atom the group
// or region does not select; idx = the atom's row
static __global__ void k_profile_keys(int n, ProfileArgs a, const double4 *__restrict__ xf,
                                      const int *__restrict__ ty, unsigned *__restrict__ key,
                                      int *__restrict__ idx) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double4 x = xf[i];
  idx[i] = i;
  if (!selected(a.p.type_mask, a.p.region_mode, a.p.region, ty[i], x)) {
    key[i] = (unsigned)a.p.nlayers;
    return;
  }
  double c = a.p.axis == 0 ? x.x : a.p.axis == 1 ? x.y : x.z;
  if (a.periodic) {
    if (c < a.boxlo) c += a.prd;
    if (c >= a.boxhi) c -= a.prd;
  }
  // (clamped as a double first: the cast of a value past int's range is undefined)
  const double b = (c - a.p.lo) * (1.0 / a.p.delta);
  const int ibin = b >= (double)a.p.nlayers ? a.p.nlayers - 1 : b < 1.0 ? 0 : (int)b;
  key[i] = (unsigned)ibin;
}

// one SPH_Q_* quantity of owned atom i, k_reduce_part's expressions
__device__ __forceinline__ double atom_quantity(int which, int i, const double4 *vr,
                                                const double *en, const double *de,
                                                const int *ty, const double4 *vel,
                                                const double *rm, const double *cv,
                                                double cv_const, const StepMass &sm) {
  switch (which) {
    case SPH_Q_RHO: return vr[i].w;
    case SPH_Q_E: return en[i];
    case SPH_Q_T: return en[i] / (cv ? cv[i] : cv_const);
    case SPH_Q_DE: return de[i];
    case SPH_Q_MASS: return rm ? rm[i] : sm.mass[ty[i]];
    case SPH_Q_KE: {
      const double4 v = vel[i];
      const double m = rm ? rm[i] : sm.mass[ty[i]];
      return 0.5 * m * (v.x * v.x + v.y * v.y + v.z * v.z);
    }
    case SPH_Q_VX: return vel[i].x;
    case SPH_Q_VY: return vel[i].y;
    case SPH_Q_VZ: return vel[i].z;
    default: return 1.0;
  }
}

// Block L folds layer L: its atoms are the run [lower_bound(L), lower_bound(L + 1)) of the
// keys sorted stably, so in row order.  Thread t sums the run's elements t, t + 256, ... in
// that order, the wave folds by shuffles, the four waves through LDS in wave order: the shape
// depends on the run alone.
static __global__ void __launch_bounds__(RED_THREADS)
k_profile_fold(int n, ProfileArgs a, const unsigned *__restrict__ key,
               const int *__restrict__ idx, const double4 *__restrict__ vr,
               const double *__restrict__ en, const double *__restrict__ de,
               const int *__restrict__ ty, const double4 *__restrict__ vel,
               const double *__restrict__ rm, const double *__restrict__ cv, double cv_const,
               StepMass sm, long long *__restrict__ count, double *__restrict__ sum) {
  __shared__ double s_p[RED_THREADS / 64][SPH_MAX_PROFILE_Q];
  const unsigned L = blockIdx.x;
  auto lower = [&](unsigned k) {  // first position whose key >= k
    int lo = 0, hi = n;
    while (lo < hi) {
      const int mid = lo + (hi - lo) / 2;
      if (key[mid] < k) lo = mid + 1;
      else hi = mid;
    }
    return lo;
  };
  const int beg = lower(L), end = lower(L + 1);
  double acc[SPH_MAX_PROFILE_Q];
#pragma unroll
  for (int q = 0; q < SPH_MAX_PROFILE_Q; q++) acc[q] = 0.0;
  for (int p = beg + (int)threadIdx.x; p < end; p += RED_THREADS) {
    const int i = idx[p];
#pragma unroll
    for (int q = 0; q < SPH_MAX_PROFILE_Q; q++)
      if (q < a.p.nq)
        acc[q] += atom_quantity(a.p.quantity[q], i, vr, en, de, ty, vel, rm, cv, cv_const, sm);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int q = 0; q < SPH_MAX_PROFILE_Q; q++) {
    double p = acc[q];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) p += __shfl_down(p, d, 64);
    if (lane == 0) s_p[wave][q] = p;
  }
  __syncthreads();
  if ((int)threadIdx.x < a.p.nq) {
    double p = s_p[0][threadIdx.x];
    for (int w = 1; w < RED_THREADS / 64; w++) p += s_p[w][threadIdx.x];
    sum[(size_t)threadIdx.x * a.p.nlayers + L] = p;
  }
  if (threadIdx.x == 0) count[L] = end - beg;
}

}  // namespace sph
