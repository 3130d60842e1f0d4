// sph_moments_kernels.h -- group diagnostics of the owned atoms beside sph_fix_kernels.h's
// reductions: mass, centre-of-mass and momentum sums, bounds, sum m / rho and the count
// (sph_engine_moments: Group::mass / xcm / vcm / bounds, compute reduce sum of mass / c_rho)
// and the gyration sums about a given centre (sph_engine_gyration: Group::gyration,
// ComputeGyration::compute_vector).  The reduction has k_reduce_part's fixed shape: grid-stride
// slices in index order, the wave folded by shuffles at 32 .. 1, the waves through LDS in wave
// order, one block folding the blocks' partials in block order; no atomics.
// Coordinates are unwrapped as Domain::unmap does (domain.cpp:1307-1316, orthogonal box) with
// the image flags of vel[i].w; every product, sum and quotient of a per-atom term is rounded
// on its own, in the reference's order (no contraction into an FMA).
#pragma once
#include <hip/hip_runtime.h>

#include "sph_engine_kernels.h"
#include "sph_fix_kernels.h"

namespace sph {

// A selection's partial is MOM_SLOTS 8-byte slots laid out as sph_moments_out (one pad slot):
// 0 count (an int64's bits), 1 mass, 2-4 mx, 5-7 mv, 8-10 lo, 11-13 hi, 14 volume
constexpr int MOM_SLOTS = 16;
constexpr int MOM_OUT = 15;   // sizeof(sph_moments_out) / 8
constexpr int GYR_SLOTS = 8;  // sph_engine_gyration's seven sums and a pad slot
constexpr int GYR_OUT = 7;
static_assert(sizeof(sph_moments_out) == MOM_OUT * sizeof(double), "slot layout");
static_assert(SPH_MAX_MOMENTS * MOM_SLOTS <= RED_THREADS, "one thread per slot in the folds");

struct MomentsArgs {
  int nsel;
  sph_group_sel sel[SPH_MAX_MOMENTS];
  double prd[3];
};
struct GyrationArgs {
  int nsel;
  sph_group_sel sel[SPH_MAX_MOMENTS];
  double prd[3];
  double cm[SPH_MAX_MOMENTS][3];
};

// slot k of two partials folded: the count as an integer, lo by min, hi by max, else a sum
__device__ __forceinline__ double mom_fold(int k, double a, double b) {
  if (k == 0) return __longlong_as_double(__double_as_longlong(a) + __double_as_longlong(b));
  if (k >= 8 && k <= 10) return fmin(a, b);
  if (k >= 11 && k <= 13) return fmax(a, b);
  return a + b;
}
__device__ __forceinline__ double mom_identity(int k) {
  return (k >= 8 && k <= 10) ? HUGE_VAL : (k >= 11 && k <= 13) ? -HUGE_VAL : 0.0;
}

// Domain::unmap: x[d] + xbox[d] * prd[d], the image counts decoded from the packed imageint
__device__ __forceinline__ void unmap(const double4 &x, int img, const double *prd, double &ux,
                                      double &uy, double &uz) {
#pragma clang fp contract(off)
  const int xbox = (img & IMG_MASK) - IMG_MAX;
  const int ybox = ((img >> IMG_BITS) & IMG_MASK) - IMG_MAX;
  const int zbox = (img >> (2 * IMG_BITS)) - IMG_MAX;
  ux = x.x + xbox * prd[0];
  uy = x.y + ybox * prd[1];
  uz = x.z + zbox * prd[2];
}

struct MomAcc {
  long long cnt;
  double sum[8];  // mass, mx[3], mv[3], volume
  double lo[3], hi[3];
};

// Stage 1 of sph_engine_moments for up to NS selections (the accumulators of all of them stay
// in registers: 15 per selection); part[(block * SPH_MAX_MOMENTS + s) * MOM_SLOTS + slot]
template <int NS>
static __global__ void __launch_bounds__(RED_THREADS)
k_moments_part(int n, MomentsArgs a, const double4 *__restrict__ xf,
               const double4 *__restrict__ vr, const int *__restrict__ ty,
               const double4 *__restrict__ vel, const double *__restrict__ rm, StepMass sm,
               double *__restrict__ part) {
#pragma clang fp contract(off)
  __shared__ double s_p[RED_THREADS / 64][NS][MOM_SLOTS];
  MomAcc acc[NS];
#pragma unroll
  for (int s = 0; s < NS; s++) {
    acc[s].cnt = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) acc[s].sum[k] = 0.0;
#pragma unroll
    for (int d = 0; d < 3; d++) {
      acc[s].lo[d] = HUGE_VAL;
      acc[s].hi[d] = -HUGE_VAL;
    }
  }
  const int stride = gridDim.x * blockDim.x;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const int t = ty[i];
    const double4 x = xf[i];
    const double4 v = vel[i];
    const double m = rm ? rm[i] : sm.mass[t];
    double ux, uy, uz;
    unmap(x, (int)v.w, a.prd, ux, uy, uz);
    double term[8];
    term[0] = m;
    term[1] = ux * m;
    term[2] = uy * m;
    term[3] = uz * m;
    term[4] = v.x * m;
    term[5] = v.y * m;
    term[6] = v.z * m;
    term[7] = m / vr[i].w;
#pragma unroll
    for (int s = 0; s < NS; s++) {
      if (s >= a.nsel) continue;
      const sph_group_sel &c = a.sel[s];
      if (!selected(c.type_mask, c.region_mode, c.region, t, x)) continue;
      acc[s].cnt += 1;
#pragma unroll
      for (int k = 0; k < 8; k++) acc[s].sum[k] += term[k];
      acc[s].lo[0] = fmin(acc[s].lo[0], x.x);
      acc[s].lo[1] = fmin(acc[s].lo[1], x.y);
      acc[s].lo[2] = fmin(acc[s].lo[2], x.z);
      acc[s].hi[0] = fmax(acc[s].hi[0], x.x);
      acc[s].hi[1] = fmax(acc[s].hi[1], x.y);
      acc[s].hi[2] = fmax(acc[s].hi[2], x.z);
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int s = 0; s < NS; s++) {
    if (s >= a.nsel) continue;  // (uniform over the grid)
    MomAcc p = acc[s];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      p.cnt += __shfl_down(p.cnt, d, 64);
#pragma unroll
      for (int k = 0; k < 8; k++) p.sum[k] += __shfl_down(p.sum[k], d, 64);
#pragma unroll
      for (int k = 0; k < 3; k++) {
        p.lo[k] = fmin(p.lo[k], __shfl_down(p.lo[k], d, 64));
        p.hi[k] = fmax(p.hi[k], __shfl_down(p.hi[k], d, 64));
      }
    }
    if (lane == 0) {
      double *o = s_p[wave][s];
      o[0] = __longlong_as_double(p.cnt);
#pragma unroll
      for (int k = 0; k < 7; k++) o[1 + k] = p.sum[k];
#pragma unroll
      for (int k = 0; k < 3; k++) {
        o[8 + k] = p.lo[k];
        o[11 + k] = p.hi[k];
      }
      o[14] = p.sum[7];
      o[15] = 0.0;
    }
  }
  __syncthreads();
  const int s = threadIdx.x / MOM_SLOTS, k = threadIdx.x % MOM_SLOTS;
  if (s < a.nsel && s < NS) {
    double p = s_p[0][s][k];
    for (int w = 1; w < RED_THREADS / 64; w++) p = mom_fold(k, p, s_p[w][s][k]);
    part[((size_t)blockIdx.x * SPH_MAX_MOMENTS + s) * MOM_SLOTS + k] = p;
  }
}

// Stage 2 (one block): thread (s, slot) folds its slot over the blocks' partials in block
// order; out: nsel sph_moments_out, as their 8-byte slots
static __global__ void k_moments_final(int nblocks, int nsel, const double *__restrict__ part,
                                       double *__restrict__ out) {
  const int s = threadIdx.x / MOM_SLOTS, k = threadIdx.x % MOM_SLOTS;
  if (s >= nsel || k >= MOM_OUT) return;
  double p = mom_identity(k);
  for (int b = 0; b < nblocks; b++)
    p = mom_fold(k, p, part[((size_t)b * SPH_MAX_MOMENTS + s) * MOM_SLOTS + k]);
  out[s * MOM_OUT + k] = p;
}

// Stage 1 of sph_engine_gyration: per selection, with d = unwrap(x) - cm of that selection,
// (dx*dx + dy*dy + dz*dz) * m (Group::gyration, group.cpp:1327-1336) and dx*dx * m, dy*dy * m,
// dz*dz * m, dx*dy * m, dx*dz * m, dy*dz * m (compute_gyration.cpp:92-108);
// part[(block * SPH_MAX_MOMENTS + s) * GYR_SLOTS + slot]
static __global__ void __launch_bounds__(RED_THREADS)
k_gyration_part(int n, GyrationArgs a, const double4 *__restrict__ xf,
                const int *__restrict__ ty, const double4 *__restrict__ vel,
                const double *__restrict__ rm, StepMass sm, double *__restrict__ part) {
#pragma clang fp contract(off)
  __shared__ double s_p[RED_THREADS / 64][SPH_MAX_MOMENTS][GYR_SLOTS];
  double acc[SPH_MAX_MOMENTS][GYR_OUT];
#pragma unroll
  for (int s = 0; s < SPH_MAX_MOMENTS; s++)
#pragma unroll
    for (int k = 0; k < GYR_OUT; k++) acc[s][k] = 0.0;
  const int stride = gridDim.x * blockDim.x;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const int t = ty[i];
    const double4 x = xf[i];
    const double m = rm ? rm[i] : sm.mass[t];
    double ux, uy, uz;
    unmap(x, (int)vel[i].w, a.prd, ux, uy, uz);
#pragma unroll
    for (int s = 0; s < SPH_MAX_MOMENTS; s++) {
      if (s >= a.nsel) continue;
      const sph_group_sel &c = a.sel[s];
      if (!selected(c.type_mask, c.region_mode, c.region, t, x)) continue;
      const double dx = ux - a.cm[s][0], dy = uy - a.cm[s][1], dz = uz - a.cm[s][2];
      acc[s][0] += (dx * dx + dy * dy + dz * dz) * m;
      acc[s][1] += dx * dx * m;
      acc[s][2] += dy * dy * m;
      acc[s][3] += dz * dz * m;
      acc[s][4] += dx * dy * m;
      acc[s][5] += dx * dz * m;
      acc[s][6] += dy * dz * m;
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int s = 0; s < SPH_MAX_MOMENTS; s++) {
    if (s >= a.nsel) continue;  // (uniform over the grid)
#pragma unroll
    for (int k = 0; k < GYR_OUT; k++) {
      double p = acc[s][k];
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) p += __shfl_down(p, d, 64);
      if (lane == 0) s_p[wave][s][k] = p;
    }
  }
  __syncthreads();
  const int s = threadIdx.x / GYR_SLOTS, k = threadIdx.x % GYR_SLOTS;
  if (s < a.nsel && k < GYR_OUT) {
    double p = s_p[0][s][k];
    for (int w = 1; w < RED_THREADS / 64; w++) p += s_p[w][s][k];
    part[((size_t)blockIdx.x * SPH_MAX_MOMENTS + s) * GYR_SLOTS + k] = p;
  }
}

// Stage 2 (one block): thread (s, slot) folds in block order; out[s * 7 + slot]
static __global__ void k_gyration_final(int nblocks, int nsel, const double *__restrict__ part,
                                        double *__restrict__ out) {
  const int s = threadIdx.x / GYR_SLOTS, k = threadIdx.x % GYR_SLOTS;
  if (s >= nsel || k >= GYR_OUT) return;
  double p = 0.0;
  for (int b = 0; b < nblocks; b++)
    p += part[((size_t)b * SPH_MAX_MOMENTS + s) * GYR_SLOTS + k];
  out[s * GYR_OUT + k] = p;
}

}  // namespace sph
