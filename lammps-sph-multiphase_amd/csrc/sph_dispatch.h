// sph_dispatch.h -- runtime -> template dispatch for the CSR pair kernels (sph_select.h).
#pragma once
#include "sph_kernels.h"
#include "sph_select.h"
#include "sph_util.h"

namespace sph {

// lanes per neighbor-list row; SPH_GROUP env var overrides (tuning), default 8
int group_lanes();

inline unsigned grid_for_rows(long rows, int G, int block = 256) {
  return (unsigned)((rows * (long)G + block - 1) / block);
}

struct RhoArgs {
  int inum;
  const int *ilist, *off, *nbr;
  double4 *xf;
  const int *ty;
  double4 *vr;
  double *rho_out;
  const Coefs *cf;
};

inline void launch_rhosum(int dim, bool eos, bool nt1, hipStream_t s, const RhoArgs &a) {
  if (a.inum <= 0) return;
  select_int<8, 4, 16>(group_lanes(), [&](auto g) {
    constexpr int G = g;
    select_int<2, 3>(dim, [&](auto d) {
      constexpr int DIM = d;
      select_bool(eos, [&](auto e) {
        constexpr bool EOS = e;
        select_bool(nt1, [&](auto t) {
          constexpr bool NT1 = t;
          hipLaunchKernelGGL((k_rhosum<G, DIM, EOS, NT1>), dim3(grid_for_rows(a.inum, G)),
                             dim3(256), 0, s, a.inum, a.ilist, a.off, a.nbr, a.xf, a.ty, a.vr,
                             a.rho_out, a.cf);
        });
      });
    });
  });
}

struct ForceArgs {
  int inum, nlocal, newton;
  const int *ilist, *off, *nbr;
  const double4 *xf, *vr;
  const int *ty;
  const double *en;
  double4 *fo;
  double *de;
  int accum;
  const Coefs *cf;
  double gx, gy, gz;
  double *virial;
  int nojside = 0;  // HALF: i share only, no atomics (two-pass reverse-list mode)
  // setup step, full list: owned atoms' vest before setup_pre_force, ghosts' vest as
  // borders() left it (k_force's setup comment); nullptr otherwise
  const double4 *vso = nullptr, *vsg = nullptr;
};

// vir (the engine's due steps; full lists with a force body): a.virial is the per-row scratch
// of k_force's VIR
inline void launch_force(int dim, bool nt1, hipStream_t s, int visc, int mode,
                         const ForceArgs &a, bool vir = false) {
  if (a.inum <= 0) return;
  select_int<8, 4, 16>(group_lanes(), [&](auto g) {
    constexpr int G = g;
    select_int<2, 3>(dim, [&](auto d) {
      constexpr int DIM = d;
      select_bool(nt1, [&](auto t) {
        constexpr bool NT1 = t;
        select_int<-1, M_TAIT, M_TAIT | M_HEAT, M_HEAT, M_GAS, M_TAIT | M_HALF,
                   M_TAIT | M_HEAT | M_HALF, M_HEAT | M_HALF, M_GAS | M_HALF>(mode, [&](auto m) {
          constexpr int MODE = m;
          if constexpr (MODE < 0) {
            SPH_REQUIRE(false, SPH_HIP_EINVAL, "unsupported force mode %d", mode);
          } else {
            select_bool(visc == SPH_VISC_MORRIS, [&](auto mor) {
              // Morris viscosity exists only for the modes with M_TAIT
              constexpr int VISC = (mor && (MODE & M_TAIT)) ? 1 : 0;
              constexpr bool CANVIR = (MODE & (M_TAIT | M_GAS)) != 0 && (MODE & M_HALF) == 0;
              SPH_REQUIRE(!vir || CANVIR, SPH_HIP_EINVAL, "no virial variant of force mode %d",
                          mode);
              select_bool(vir, [&](auto vi) {
                constexpr bool VIR = vi && CANVIR;
                hipLaunchKernelGGL((k_force<G, DIM, VISC, MODE, NT1, VIR>),
                                   dim3(grid_for_rows(a.inum, G)), dim3(256), 0, s, a.inum,
                                   a.nlocal, a.newton, a.ilist, a.off, a.nbr, a.xf, a.vr, a.ty,
                                   a.en, a.fo, a.de, a.accum, a.cf, a.gx, a.gy, a.gz, a.virial,
                                   a.nojside, a.vso, a.vsg);
              });
            });
          }
        });
      });
    });
  });
}

}  // namespace sph
