// sph_fix_kernels.h -- streaming kernels of the engine beside the integrator: the fix
// setmeso / setmesode clamps (one pass over the owned rows after the pair compute) and the
// group reductions of the thermo output (a fixed-shape two-stage reduction, no atomics).
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
    double q[7];
    q[SPH_Q_ONE] = 1.0;
    q[SPH_Q_RHO] = vr[i].w;
    q[SPH_Q_E] = ei;
    q[SPH_Q_T] = ei / (cv ? cv[i] : cv_const);
    q[SPH_Q_DE] = de[i];
    q[SPH_Q_MASS] = m;
    q[SPH_Q_KE] = 0.5 * m * (v.x * v.x + v.y * v.y + v.z * v.z);
#pragma unroll
    for (int s = 0; s < SPH_MAX_REDUCE; s++) {
      if (s >= a.nsel) continue;
      const sph_reduce_sel &c = a.sel[s];
      if (!selected(c.type_mask, c.region_mode, c.region, t, x)) continue;
      double val = q[0];
#pragma unroll
      for (int k = 1; k < 7; k++) val = c.quantity == k ? q[k] : val;
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

}  // namespace sph
