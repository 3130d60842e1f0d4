// sph_engine.hip -- device-resident engine of the C ABI (include/sph_hip.h, section 2).
//
// One engine = one rank's share of an SPH run, resident in HBM.  A step is Verlet::run's
// sequence (src/verlet.cpp:222-308) specialised to the USER-SPH hot path:
//   initial_integrate -> [rebuild: pbc, spatial sort, borders, bins, full list]
//   | forward comm -> rhosum (+EOS) -> forward rho -> taitwater[/morris][+heat] ->
//   final_integrate
// Full lists are walked gather-only, so the reverse communication of the reference
// (comm->reverse_comm, verlet.cpp:290-293) has nothing to carry and is skipped.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <rocprofiler-sdk-roctx/roctx.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <cmath>
#include <utility>
#include <vector>

#include "sph_coef.h"
#include "sph_comm.h"
#include "sph_dispatch.h"
#include "sph_blk_kernels.h"
#include "sph_engine_kernels.h"
#include "sph_engine_mp.h"
#include "sph_fix_kernels.h"
#include "sph_ipc.h"
#include "sph_moments_kernels.h"
#include "sph_mp2_kernels.h"
#include "sph_pc.h"
#include "sph_row2_kernels.h"
#include "sph_util.h"

using namespace sph;

#include "sph_engine_state.h"
#include "sph_engine_comm.h"
#include "sph_engine_pc.h"
#include "sph_engine_neigh.h"
#include "sph_engine_step.h"

// MpCoefs of the multiphase stack from the engine's (SPH_MAXTYPES+1)^2 tables (upper
// triangle mirrored like init_one; the coeff() formulas as sph_multiphase.hip's), and the
// stack's cutoffs into cutmax ((nt+1)^2, upper triangle)
static void coef_mp(MpCoefs &m, const sph_engine_mp_config &c, int dim, int nt,
                    std::vector<double> &cutmax) {
  const int n1 = nt + 1, M1 = SPH_MAXTYPES + 1;
  m = MpCoefs{};
  m.ntypes = nt;
  m.dim = dim;
  auto up = [&](const double *t, int i, int j) { return j >= i ? t[i * M1 + j] : t[j * M1 + i]; };
  auto upi = [&](const int *t, int i, int j) { return j >= i ? t[i * M1 + j] : t[j * M1 + i]; };
  auto cut = [&](bool on, const double *t) {
    if (!on) return;
    for (int i = 0; i <= nt; i++)
      for (int j = i; j <= nt; j++) cutmax[i * n1 + j] = std::max(cutmax[i * n1 + j], t[i * M1 + j]);
  };
  for (int i = 0; i <= nt; i++)
    for (int j = 0; j <= nt; j++) {
      const int k = i * n1 + j;
      m.rcut[k] = up(c.rhosum_cut, i, j);
      m.rcutsq[k] = m.rcut[k] * m.rcut[k];
      m.calpha[k] = up(c.cg_alpha, i, j);
      m.ccut[k] = up(c.cg_cut, i, j);
      m.ccutsq[k] = m.ccut[k] * m.ccut[k];
      m.tvisc[k] = up(c.tait_visc, i, j);
      m.tcut[k] = up(c.tait_cut, i, j);
      m.tcutsq[k] = m.tcut[k] * m.tcut[k];
      m.scut[k] = up(c.st_cut, i, j);
      m.scutsq[k] = m.scut[k] * m.scut[k];
      m.halpha[k] = up(c.heat_alpha, i, j);
      m.hcut[k] = up(c.heat_cut, i, j);
      m.hcutsq[k] = m.hcut[k] * m.hcut[k];
      m.htc[k] = up(c.heat_tc, i, j);
      m.hfix[k] = upi(c.heat_fixflag, i, j);
    }
  if (c.tait_on)
    for (int t = 1; t <= nt; t++) {
      SPH_REQUIRE(c.gamma[t] != 0.0 && c.rho0[t] != 0.0, SPH_HIP_EINVAL,
                  "type %d: gamma and rho0 must be non-zero", t);
      m.rho0[t] = c.rho0[t];
      m.gamma[t] = c.gamma[t];
      m.rbg[t] = c.rbackground[t];
      // B = c^2 rho0 / gamma, pair_sph_taitwater_multiphase.cpp:243-250
      m.B[t] = c.soundspeed[t] * c.soundspeed[t] * c.rho0[t] / c.gamma[t];
    }
  cut(c.rhosum_nstep > 0, c.rhosum_cut);
  cut(c.cg_nstep > 0, c.cg_cut);
  cut(c.tait_on != 0, c.tait_cut);
  cut(c.st_on != 0, c.st_cut);
  cut(c.heat_on != 0, c.heat_cut);
}

extern "C" {

int sph_engine_create(int device, const sph_engine_config *cfg, sph_engine **out) {
  SPH_API_BEGIN
  SPH_REQUIRE(cfg && out, SPH_HIP_EINVAL, "sph_engine_create: NULL argument");
  g_alloc_log = env_int("SPH_ALLOC_LOG", 0);
  SPH_REQUIRE(cfg->dim == 2 || cfg->dim == 3, SPH_HIP_EINVAL, "dimension must be 2 or 3");
  SPH_REQUIRE(cfg->ntypes >= 1 && cfg->ntypes <= SPH_MAXTYPES, SPH_HIP_EINVAL,
              "ntypes %d outside [1,%d]", cfg->ntypes, SPH_MAXTYPES);
  const int pgn = cfg->procgrid[0] * cfg->procgrid[1] * cfg->procgrid[2];
  SPH_REQUIRE(pgn == 0 || (cfg->procgrid[0] >= 1 && cfg->procgrid[1] >= 1 &&
                           cfg->procgrid[2] >= 1 && cfg->rank >= 0 && cfg->rank < pgn),
              SPH_HIP_EINVAL, "bad procgrid %dx%dx%d / rank %d", cfg->procgrid[0],
              cfg->procgrid[1], cfg->procgrid[2], cfg->rank);
  SPH_REQUIRE(pgn <= 1 || cfg->dim == 3 || cfg->procgrid[2] == 1, SPH_HIP_EINVAL,
              "2-D runs cannot split z");
  require_device(device);
  sph_engine *e = new sph_engine;
  try {
    e->device = device;
    e->cfg = *cfg;
    const int nt = cfg->ntypes;
    Coefs &c = e->hc;
    c.ntypes = nt;
    c.dim = cfg->dim;
    // the body-force mass: the types of the gravity fix's group (gravity_mask, 0 = all)
    for (int t = 0; t <= nt; t++)
      c.mass[t] = (cfg->gravity_mask == 0 || ((cfg->gravity_mask >> t) & 1)) ? cfg->mass[t] : 0.0;
    // per-type-pair tables are passed in the engine's fixed (SPH_MAXTYPES+1)^2 layout
    auto repack = [&](const double *src, std::vector<double> &dst) {
      dst.assign((nt + 1) * (nt + 1), 0.0);
      for (int i = 0; i <= nt; i++)
        for (int j = 0; j <= nt; j++) dst[i * (nt + 1) + j] = src[i * (SPH_MAXTYPES + 1) + j];
    };
    std::vector<double> cutmax((nt + 1) * (nt + 1), 0.0), tmpv, tmpc;
    if (cfg->rhosum_nstep > 0) {
      repack(cfg->rhosum_cut, tmpc);
      coef_rhosum(c, cfg->dim, nt, tmpc.data(), cfg->mass);
      for (size_t k = 0; k < cutmax.size(); k++) cutmax[k] = std::max(cutmax[k], tmpc[k]);
    }
    if (cfg->tait_on) {
      repack(cfg->tait_cut, tmpc);
      repack(cfg->tait_visc_coef, tmpv);
      coef_tait(c, cfg->dim, nt, cfg->tait_visc, cfg->rho0, cfg->soundspeed, cfg->B,
                tmpv.data(), tmpc.data(), cfg->mass);
      for (size_t k = 0; k < cutmax.size(); k++) cutmax[k] = std::max(cutmax[k], tmpc[k]);
      e->force_mode |= M_TAIT;
    }
    if (cfg->heat_on) {
      repack(cfg->heat_cut, tmpc);
      repack(cfg->heat_alpha, tmpv);
      coef_heat(c, cfg->dim, nt, tmpv.data(), tmpc.data(), cfg->mass);
      for (size_t k = 0; k < cutmax.size(); k++) cutmax[k] = std::max(cutmax[k], tmpc[k]);
      e->force_mode |= M_HEAT;
    }
    if (cfg->mp) {
      SPH_REQUIRE(cfg->rhosum_nstep == 0 && !cfg->tait_on && !cfg->heat_on, SPH_HIP_EINVAL,
                  "the multiphase stack replaces the single-phase styles (turn them off)");
      e->mp = true;
      e->mpc = *cfg->mp;
      e->cfg.mp = nullptr;
      coef_mp(e->hm, e->mpc, cfg->dim, nt, cutmax);
    }
    if (pgn > 1) {
      for (int k = 0; k < 3; k++) e->pg[k] = cfg->procgrid[k];
      e->nprocs = pgn;
      e->me = cfg->rank;
    }
    // brick of this rank, x fastest (Domain::set_local_box with uniform xsplit, domain.cpp)
    e->myloc[0] = e->me % e->pg[0];
    e->myloc[1] = (e->me / e->pg[0]) % e->pg[1];
    e->myloc[2] = e->me / (e->pg[0] * e->pg[1]);
    for (int k = 0; k < 3; k++) {
      e->box.lo[k] = cfg->boxlo[k];
      e->box.hi[k] = cfg->boxhi[k];
      e->box.prd[k] = cfg->boxhi[k] - cfg->boxlo[k];
      e->box.periodic[k] = (k < cfg->dim) ? cfg->periodic[k] : 0;
      const double lo = (double)e->myloc[k] / e->pg[k], hi = (double)(e->myloc[k] + 1) / e->pg[k];
      e->sublo[k] = cfg->boxlo[k] + e->box.prd[k] * lo;
      e->subhi[k] = (e->myloc[k] + 1 == e->pg[k]) ? cfg->boxhi[k]
                                                   : cfg->boxlo[k] + e->box.prd[k] * hi;
      auto at = [&](int dx, int dy, int dz) {
        const int l[3] = {(e->myloc[0] + dx + e->pg[0]) % e->pg[0],
                          (e->myloc[1] + dy + e->pg[1]) % e->pg[1],
                          (e->myloc[2] + dz + e->pg[2]) % e->pg[2]};
        return (l[2] * e->pg[1] + l[1]) * e->pg[0] + l[0];
      };
      e->procneigh[k][0] = at(k == 0 ? -1 : 0, k == 1 ? -1 : 0, k == 2 ? -1 : 0);
      e->procneigh[k][1] = at(k == 0 ? 1 : 0, k == 1 ? 1 : 0, k == 2 ? 1 : 0);
    }
    e->cutmax_tab = cutmax;
    // (no style yet: sph_engine_idealgas brings the first cut; setup insists on one)
    if (*std::max_element(cutmax.begin(), cutmax.end()) > 0.0) e->set_cutoffs();
    e->sc.dtv = cfg->dt;
    e->sc.dtf = 0.5 * cfg->dt * (cfg->ftm2v > 0 ? cfg->ftm2v : 1.0);  // fix_meso.cpp:63-66
    for (int t = 0; t <= nt; t++) e->sc.mass[t] = cfg->mass[t];
    e->sc.stationary_mask = cfg->stationary_mask;
    SPH_HIP_TRY(hipStreamCreateWithFlags(&e->s, hipStreamNonBlocking));
    SPH_HIP_TRY(hipMalloc(&e->dc, sizeof(Coefs)));
    SPH_HIP_TRY(hipMemcpy(e->dc, &e->hc, sizeof(Coefs), hipMemcpyHostToDevice));
    if (e->mp) {
      SPH_HIP_TRY(hipMalloc(&e->dm, sizeof(MpCoefs)));
      mp_inverses(e->hm);
      SPH_HIP_TRY(hipMemcpy(e->dm, &e->hm, sizeof(MpCoefs), hipMemcpyHostToDevice));
    }
    SPH_HIP_TRY(hipHostMalloc(&e->h_scalar, sizeof(int)));
    SPH_HIP_TRY(hipHostMalloc(&e->h_small, 16 * sizeof(int)));
    SPH_HIP_TRY(hipHostMalloc(&e->h_cs, 2 * sizeof(int)));
    SPH_HIP_TRY(hipHostMalloc(&e->h_nm, sizeof(int)));
    SPH_HIP_TRY(hipHostMalloc(&e->h_dt, sizeof(DtRecord)));
    for (auto &ev : e->cs_ev) SPH_HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  } catch (...) {
    delete e;
    throw;
  }
  e->overlap = false;
  *out = e;
  SPH_API_END
}

int sph_engine_destroy(sph_engine *e) {
  if (!e) return SPH_HIP_OK;
  (void)hipSetDevice(e->device);
  if (e->s) (void)hipStreamSynchronize(e->s);
  if (e->s2) (void)hipStreamSynchronize(e->s2);
  for (auto *b : {&e->xf, &e->vr, &e->vel, &e->fo, &e->xf2, &e->vr2, &e->vel2, &e->xb}) b->release();
  for (auto *b : {&e->en, &e->en2, &e->de, &e->rm, &e->cvv, &e->rho_tmp, &e->dmass, &e->xbuf,
                  &e->xbuf2})
    b->release();
  for (auto *b : {&e->rhoS, &e->rhoF}) b->release();
  for (auto *b : {&e->cg, &e->cgS, &e->cgF, &e->recA, &e->recK, &e->recF, &e->recS}) b->release();
  if (e->dm) (void)hipFree(e->dm);
  for (auto *b : {&e->nbs, &e->gorank, &e->goidx, &e->dr_sidx, &e->dr_rslot, &e->dr_self, &e->dr_req, &e->dr_byq, &e->dr_byg, &e->dr_hist, &e->pc_flag,
                  &e->pc_cand, &e->pc_otag, &e->pc_idx})
    b->release();
  for (auto *b : {&e->pc_rec, &e->pc_gat, &e->pc_Wd, &e->pc_vals, &e->pc_nrec, &e->pc_v0,
                  &e->pc_v1})
    b->release();
  e->pc_k0.release();
  e->pc_k1.release();
  e->pc_cnt.release();
  e->red_part.release();
  e->red_out.release();
  e->ff_part.release();
  e->ff_tot.release();
  e->pf_key.release();
  e->pf_key2.release();
  e->pf_idx.release();
  e->pf_idx2.release();
  e->pf_cnt.release();
  e->pf_sum.release();
  e->mom_buf.release();
  for (auto *b : {&e->ty, &e->ty2, &e->tag, &e->tag2, &e->gowner, &e->gimg, &e->sel, &e->nsel,
                  &e->bidx, &e->bidx2, &e->cnt, &e->off, &e->nbr, &e->mx,
                  &e->ccnt, &e->qbeg, &e->tb, &e->xpos, &e->sel2, &e->rows_in, &e->rows_bd,
                  &e->ulist, &e->ucnt, &e->kcnt, &e->uilist, &e->uicnt})
    b->release();
  for (auto *b : {&e->bkey, &e->bkey2}) b->release();
  for (auto *b : {&e->cs_cnt, &e->cs_beg, &e->cs_mx}) b->release();
  for (auto ev : e->cs_ev)
    if (ev) (void)hipEventDestroy(ev);
  if (e->h_cs) (void)hipHostFree(e->h_cs);
  if (e->h_nm) (void)hipHostFree(e->h_nm);
  if (e->h_dt) (void)hipHostFree(e->h_dt);
  e->dt_rec.release();
  e->dt_part.release();
  for (auto *b : {&e->flags, &e->tmp, &e->cbs, &e->cbr, &e->flag2, &e->fl_in, &e->fl_bd}) b->release();
  e->snbr.release();
  e->snbi.release();
  e->icnt.release();
  e->moved.release();
  e->xhold.release();
  e->nm_flag.release();
  e->x0.release();
  e->blen.release();
  for (auto &sw : e->swaps) sw.list.release();
  for (auto &p : e->pending) {
    (void)hipEventDestroy(p.a);
    (void)hipEventDestroy(p.b);
  }
  for (auto ev : e->evpool) (void)hipEventDestroy(ev);
  if (e->h_scalar) (void)hipHostFree(e->h_scalar);
  if (e->h_small) (void)hipHostFree(e->h_small);
  delete e->tr;
  if (e->dc) (void)hipFree(e->dc);
  if (e->ev_fork) (void)hipEventDestroy(e->ev_fork);
  if (e->ev_join) (void)hipEventDestroy(e->ev_join);
  if (e->s2) (void)hipStreamDestroy(e->s2);
  if (e->s) (void)hipStreamDestroy(e->s);
  delete e;
  return SPH_HIP_OK;
}

int sph_engine_set_atoms(sph_engine *e, int n, const double *x, const double *v,
                         const int *type, const double *rho, const double *en,
                         const double *cv) {
  SPH_API_BEGIN
  SPH_REQUIRE(e && n >= 0 && (n == 0 || (x && v && type && rho)), SPH_HIP_EINVAL,
              "sph_engine_set_atoms: bad argument");
  SPH_HIP_TRY(hipSetDevice(e->device));
  for (int i = 0; i < n; i++)
    SPH_REQUIRE(type[i] >= 1 && type[i] <= e->cfg.ntypes, SPH_HIP_EINVAL,
                "atom %d has type %d outside [1,%d]", i, type[i], e->cfg.ntypes);
  e->nlocal = n;
  e->nghost = 0;
  e->tag_next = n;
  e->pc_tags_agreed = false;
  e->pc_inserted = 0;
  e->cv_by_tag.assign(n, 1.0);
  if (cv)
    for (int i = 0; i < n; i++) e->cv_by_tag[i] = cv[i];
  e->ensure_atoms(n > 0 ? n : 1, false);
  e->vel.reserve_min1(n);
  e->fo.reserve_min1(n);
  e->de.reserve_min1(n);
  e->tag.reserve_min1(n);
  std::vector<double4> hx(n), hv(n), hvel(n);
  std::vector<double> he(n);
  std::vector<int> ht(n), hty(n);
  for (int i = 0; i < n; i++) {
    hx[i] = make_double4(x[3 * i], x[3 * i + 1], x[3 * i + 2], 0.0);
    hv[i] = make_double4(0.0, 0.0, 0.0, rho[i]);  // vest = 0 until setup_pre_force
    hvel[i] = make_double4(v[3 * i], v[3 * i + 1], v[3 * i + 2], (double)IMG_ZERO);
    he[i] = en ? en[i] : 0.0;
    ht[i] = i;
    hty[i] = type[i];
  }
  if (n > 0) {
    e->to_dev(e->xf.p, hx.data(), n);
    e->to_dev(e->vr.p, hv.data(), n);
    e->to_dev(e->vel.p, hvel.data(), n);
    e->to_dev(e->en.p, he.data(), n);
    e->to_dev(e->ty.p, hty.data(), n);
    e->to_dev(e->tag.p, ht.data(), n);
    SPH_HIP_TRY(hipMemsetAsync(e->fo.p, 0, n * sizeof(double4), e->s));
    SPH_HIP_TRY(hipMemsetAsync(e->de.p, 0, n * sizeof(double), e->s));
  }
  // LAMMPS' local order starts as the read order (data-file lines / create_atoms), which is
  // the order handed here -- not necessarily tag order (sph_engine_set_tags may permute)
  e->lidx.reserve_min1(n);
  if (n > 0) e->launch(k_lidx_iota, n, n, 0, e->lidx.p);
  e->lidx_valid = true;
  if (e->mp && n > 0) {  // per-type mass, cv (default 1, create_atom), colorgradient 0
    std::vector<double> hm(n), hc(n);
    for (int i = 0; i < n; i++) {
      hm[i] = e->cfg.mass[type[i]];
      hc[i] = cv ? cv[i] : 1.0;
    }
    e->to_dev(e->rm.p, hm.data(), n);
    e->to_dev(e->cvv.p, hc.data(), n);
    SPH_HIP_TRY(hipMemsetAsync(e->cg.p, 0, n * sizeof(double4), e->s));
  }
  SPH_HIP_TRY(hipStreamSynchronize(e->s));
  e->setup_done = false;
  SPH_API_END
}

int sph_engine_set_atoms_multiphase(sph_engine *e, const double *rmass, const double *cv,
                                    const double *cg) {
  SPH_API_BEGIN
  SPH_REQUIRE(e && e->mp, SPH_HIP_EINVAL,
              "sph_engine_set_atoms_multiphase: not a multiphase engine (cfg.mp)");
  const int n = e->nlocal;
  SPH_REQUIRE(n == 0 || rmass, SPH_HIP_EINVAL, "sph_engine_set_atoms_multiphase: NULL rmass");
  SPH_HIP_TRY(hipSetDevice(e->device));
  if (n == 0) return SPH_HIP_OK;
  for (int i = 0; i < n; i++)
    SPH_REQUIRE(rmass[i] > 0.0, SPH_HIP_EINVAL, "atom %d has rmass %g <= 0", i, rmass[i]);
  std::vector<double> hc(n, 1.0);
  std::vector<double4> hg(n, make_double4(0.0, 0.0, 0.0, 0.0));
  for (int i = 0; i < n; i++) {
    if (cv) hc[i] = cv[i];
    if (cg) hg[i] = make_double4(cg[3 * i], cg[3 * i + 1], cg[3 * i + 2], 0.0);
  }
  e->to_dev(e->rm.p, rmass, n);
  e->to_dev(e->cvv.p, hc.data(), n);
  e->to_dev(e->cg.p, hg.data(), n);
  SPH_HIP_TRY(hipStreamSynchronize(e->s));
  e->setup_done = false;
  SPH_API_END
}

int sph_engine_phase_change(sph_engine *e, const sph_phasechange_params *p, int nevery,
                            int seed) {
  SPH_API_BEGIN
  SPH_REQUIRE(e && p, SPH_HIP_EINVAL, "sph_engine_phase_change: NULL argument");
  SPH_REQUIRE(e->mp, SPH_HIP_EINVAL,
              "fix phase_change needs atom_style meso/multiphase (a multiphase engine)");
  SPH_REQUIRE(seed > 0, SPH_HIP_EINVAL, "Invalid seed for Park random # generator");
  SPH_REQUIRE(!e->setup_done, SPH_HIP_EINVAL,
              "sph_engine_phase_change: arm the fix before sph_engine_setup (its local-order "
              "bookkeeping starts at set_atoms)");
  SPH_REQUIRE(!e->dtr_on, SPH_HIP_EINVAL,
              "sph_engine_phase_change: not together with sph_engine_dt_reset (the fix's "
              "ENERGY-rate threshold reads update->dt, which then lives on the device)");
  SPH_REQUIRE(nevery >= 1, SPH_HIP_EINVAL, "sph_engine_phase_change: nevery < 1");
  SPH_REQUIRE(p->to_mass > 0.0 && p->maxattempt >= 1 && p->cutoff > 0.0, SPH_HIP_EINVAL,
              "sph_engine_phase_change: bad parameters");
  SPH_REQUIRE(p->from_type >= 1 && p->from_type <= e->cfg.ntypes && p->to_type >= 1 &&
                  p->to_type <= e->cfg.ntypes,
              SPH_HIP_EINVAL, "sph_engine_phase_change: type outside [1,%d]", e->cfg.ntypes);
  e->pc = true;
  e->pcp = *p;
  e->pcp.dt = e->cfg.dt;
  e->pc_nevery = nevery;
  e->pc_seed = seed;
  e->pc_next = e->step + 1;  // next_reneighbor = ntimestep + 1 (fix_phase_change.cpp:120)
  SPH_API_END
}

static void check_region(const char *who, int region_mode, const sph_region &r) {
  SPH_REQUIRE(region_mode >= 0 && region_mode <= 2, SPH_HIP_EINVAL, "%s: region_mode %d", who,
              region_mode);
  if (region_mode == 0) return;
  SPH_REQUIRE(r.style == SPH_REGION_SPHERE || r.style == SPH_REGION_BLOCK, SPH_HIP_EINVAL,
              "%s: unknown region style %d", who, r.style);
  if (r.style == SPH_REGION_SPHERE)  // "Illegal region sphere command" (region_sphere.cpp:70)
    SPH_REQUIRE(r.radius >= 0.0, SPH_HIP_EINVAL, "%s: sphere radius %g < 0", who, r.radius);
}

int sph_engine_setmeso(sph_engine *e, const sph_setmeso *fix) {
  SPH_API_BEGIN
  SPH_REQUIRE(e && fix, SPH_HIP_EINVAL, "sph_engine_setmeso: NULL argument");
  SPH_REQUIRE(!e->setup_done, SPH_HIP_EINVAL,
              "sph_engine_setmeso: arm the fix before sph_engine_setup");
  SPH_REQUIRE(fix->what >= SPH_SET_RHO && fix->what <= SPH_SET_DE, SPH_HIP_EINVAL,
              "sph_engine_setmeso: unknown field %d", fix->what);
  check_region("sph_engine_setmeso", fix->region_mode, fix->region);
  SPH_REQUIRE(!(fix->what == SPH_SET_DE && fix->region_mode == 2), SPH_HIP_EINVAL,
              "sph_engine_setmeso: fix setmesode has no noregion");
  SPH_REQUIRE(e->sm.nfix < SPH_MAX_SETMESO, SPH_HIP_EINVAL,
              "sph_engine_setmeso: more than %d fixes", SPH_MAX_SETMESO);
  e->sm.fix[e->sm.nfix++] = *fix;
  if (fix->what == SPH_SET_T) e->sm_needs_cv = true;
  SPH_API_END
}

int sph_engine_reduce(sph_engine *e, int nsel, const sph_reduce_sel *sel, sph_reduce_out *out) {
  SPH_API_BEGIN
  SPH_REQUIRE(e && nsel >= 0 && (nsel == 0 || (sel && out)), SPH_HIP_EINVAL,
              "sph_engine_reduce: bad argument");
  SPH_REQUIRE(nsel <= SPH_MAX_REDUCE, SPH_HIP_EINVAL,
              "sph_engine_reduce: %d selections > %d", nsel, SPH_MAX_REDUCE);
  SPH_REQUIRE(e->setup_done, SPH_HIP_EINVAL, "sph_engine_reduce: call sph_engine_setup first");
  ReduceArgs a{};
  a.nsel = nsel;
  bool needs_cv = false;
  for (int k = 0; k < nsel; k++) {
    SPH_REQUIRE(sel[k].quantity >= SPH_Q_ONE && sel[k].quantity <= SPH_Q_VZ, SPH_HIP_EINVAL,
                "sph_engine_reduce: selection %d: unknown quantity %d", k, sel[k].quantity);
    check_region("sph_engine_reduce", sel[k].region_mode, sel[k].region);
    a.sel[k] = sel[k];
    needs_cv = needs_cv || sel[k].quantity == SPH_Q_T;
  }
  if (nsel == 0) return SPH_HIP_OK;
  const double cvc = (!e->mp && needs_cv) ? e->uniform_cv("SPH_Q_T") : 1.0;
  const int n = e->nlocal;
  if (n == 0) {
    for (int k = 0; k < nsel; k++) out[k] = sph_reduce_out{0.0, HUGE_VAL, -HUGE_VAL, 0};
    return SPH_HIP_OK;
  }
  SPH_HIP_TRY(hipSetDevice(e->device));
  const int nb = (int)std::min<long>(blocks(n), RED_MAXBLOCKS);
  e->red_part.reserve((size_t)RED_MAXBLOCKS * SPH_MAX_REDUCE);
  e->red_out.reserve(SPH_MAX_REDUCE);
  StepMass sm;
  for (int t = 0; t <= MAXT; t++) sm.mass[t] = e->sc.mass[t];
  hipLaunchKernelGGL(k_reduce_part, dim3(nb), dim3(RED_THREADS), 0, e->s, n, a, e->xf.p, e->vr.p,
                     e->en.p, e->de.p, e->ty.p, e->vel.p, e->mp ? (const double *)e->rm.p : nullptr,
                     e->mp ? (const double *)e->cvv.p : nullptr, cvc, sm, e->red_part.p);
  hipLaunchKernelGGL(k_reduce_final, dim3(1), dim3(64), 0, e->s, nb, nsel, e->red_part.p,
                     e->red_out.p);
  SPH_HIP_TRY(hipGetLastError());
  e->to_host(out, e->red_out.p, nsel);
  SPH_HIP_TRY(hipStreamSynchronize(e->s));
  SPH_API_END
}

int sph_engine_forcefix(sph_engine *e, const sph_forcefix *fix, int *id) {
  SPH_API_BEGIN
  SPH_REQUIRE(e && fix, SPH_HIP_EINVAL, "sph_engine_forcefix: NULL argument");
  SPH_REQUIRE(!e->setup_done, SPH_HIP_EINVAL,
              "sph_engine_forcefix: arm the fix before sph_engine_setup");
  SPH_REQUIRE(fix->kind == SPH_FF_SET || fix->kind == SPH_FF_ADD, SPH_HIP_EINVAL,
              "sph_engine_forcefix: unknown kind %d", fix->kind);
  check_region("sph_engine_forcefix", fix->region_mode, fix->region);
  SPH_REQUIRE(fix->nevery >= 1, SPH_HIP_EINVAL, "sph_engine_forcefix: nevery %d < 1",
              fix->nevery);
  SPH_REQUIRE((fix->comp_mask & ~7) == 0, SPH_HIP_EINVAL, "sph_engine_forcefix: comp_mask %d",
              fix->comp_mask);
  if (fix->kind == SPH_FF_SET)
    SPH_REQUIRE(!fix->per_mass && fix->nevery == 1, SPH_HIP_EINVAL,
                "sph_engine_forcefix: fix setforce has neither a per-mass value nor nevery");
  else
    SPH_REQUIRE(fix->comp_mask == 7, SPH_HIP_EINVAL,
                "sph_engine_forcefix: fix addforce needs all three components (comp_mask 7)");
  SPH_REQUIRE(e->ff.nfix < SPH_MAX_FORCEFIX, SPH_HIP_EINVAL,
              "sph_engine_forcefix: more than %d fixes", SPH_MAX_FORCEFIX);
  if (id) *id = e->ff.nfix;
  e->ff.fix[e->ff.nfix++] = *fix;
  if (fix->tally) e->ff_tally = true;
  SPH_API_END
}

int sph_engine_idealgas(sph_engine *e, const sph_engine_gas *gas) {
  SPH_API_BEGIN
  SPH_REQUIRE(e && gas, SPH_HIP_EINVAL, "sph_engine_idealgas: NULL argument");
  SPH_REQUIRE(!e->setup_done, SPH_HIP_EINVAL,
              "sph_engine_idealgas: arm the style before sph_engine_setup");
  SPH_REQUIRE(!(e->force_mode & M_GAS), SPH_HIP_EINVAL, "sph_engine_idealgas: already armed");
  SPH_REQUIRE(!e->cfg.tait_on && !e->cfg.heat_on && !e->mp, SPH_HIP_EINVAL,
              "sph_engine_idealgas: one force style per engine (tait_on, heat_on and mp off)");
  const int nt = e->cfg.ntypes, n1 = nt + 1, M1 = SPH_MAXTYPES + 1;
  std::vector<double> visc(n1 * n1, 0.0), cut(n1 * n1, 0.0);
  for (int i = 1; i <= nt; i++)
    for (int j = i; j <= nt; j++) {
      SPH_REQUIRE(gas->cut[i * M1 + j] > 0.0, SPH_HIP_EINVAL,
                  "sph_engine_idealgas: cut %g of types %d %d is not positive",
                  gas->cut[i * M1 + j], i, j);
      visc[i * n1 + j] = gas->viscosity[i * M1 + j];
      cut[i * n1 + j] = gas->cut[i * M1 + j];
    }
  SPH_HIP_TRY(hipSetDevice(e->device));
  // (the cutoffs first: a cut the box cannot take leaves the engine as it was)
  const std::vector<double> old = e->cutmax_tab;
  for (size_t k = 0; k < cut.size(); k++) e->cutmax_tab[k] = std::max(old[k], cut[k]);
  try {
    e->set_cutoffs();
  } catch (...) {
    e->cutmax_tab = old;
    if (*std::max_element(old.begin(), old.end()) > 0.0) e->set_cutoffs();
    throw;
  }
  coef_gas(e->hc, e->cfg.dim, nt, visc.data(), cut.data(), e->cfg.mass, /*mirror_visc=*/true);
  // (the rhosum epilogue still writes a Tait term, which k_eos_gas replaces: keep it finite)
  for (int t = 0; t <= nt; t++) {
    e->hc.rho0[t] = 1.0;
    e->hc.B[t] = 0.0;
  }
  e->force_mode = M_GAS;
  SPH_HIP_TRY(hipMemcpy(e->dc, &e->hc, sizeof(Coefs), hipMemcpyHostToDevice));
  SPH_API_END
}

int sph_engine_forcefix_total(sph_engine *e, int id, double out[3]) {
  SPH_API_BEGIN
  SPH_REQUIRE(e && out, SPH_HIP_EINVAL, "sph_engine_forcefix_total: NULL argument");
  SPH_REQUIRE(id >= 0 && id < e->ff.nfix, SPH_HIP_EINVAL,
              "sph_engine_forcefix_total: no fix %d", id);
  SPH_REQUIRE(e->ff.fix[id].tally, SPH_HIP_EINVAL,
              "sph_engine_forcefix_total: fix %d was armed without tally", id);
  SPH_REQUIRE(e->setup_done, SPH_HIP_EINVAL,
              "sph_engine_forcefix_total: call sph_engine_setup first");
  SPH_HIP_TRY(hipSetDevice(e->device));
  e->to_host(out, e->ff_tot.p + 3 * id, 3);
  SPH_HIP_TRY(hipStreamSynchronize(e->s));
  SPH_API_END
}

int sph_engine_profile(sph_engine *e, const sph_profile *p, int64_t *count, double *sum) {
  SPH_API_BEGIN
  SPH_REQUIRE(e && p && count, SPH_HIP_EINVAL, "sph_engine_profile: NULL argument");
  SPH_REQUIRE(p->axis >= 0 && p->axis <= 2, SPH_HIP_EINVAL, "sph_engine_profile: axis %d",
              p->axis);
  SPH_REQUIRE(p->delta > 0.0, SPH_HIP_EINVAL, "sph_engine_profile: delta %g <= 0", p->delta);
  SPH_REQUIRE(p->nlayers >= 1, SPH_HIP_EINVAL, "sph_engine_profile: nlayers %d < 1",
              p->nlayers);
  SPH_REQUIRE(p->nq >= 0 && p->nq <= SPH_MAX_PROFILE_Q && (p->nq == 0 || sum), SPH_HIP_EINVAL,
              "sph_engine_profile: nq %d outside [0,%d]", p->nq, SPH_MAX_PROFILE_Q);
  bool needs_cv = false;
  for (int q = 0; q < p->nq; q++) {
    SPH_REQUIRE(p->quantity[q] >= SPH_Q_ONE && p->quantity[q] <= SPH_Q_VZ, SPH_HIP_EINVAL,
                "sph_engine_profile: unknown quantity %d", p->quantity[q]);
    needs_cv = needs_cv || p->quantity[q] == SPH_Q_T;
  }
  check_region("sph_engine_profile", p->region_mode, p->region);
  SPH_REQUIRE(e->setup_done, SPH_HIP_EINVAL, "sph_engine_profile: call sph_engine_setup first");
  const double cvc = (!e->mp && needs_cv) ? e->uniform_cv("SPH_Q_T") : 1.0;
  const int n = e->nlocal, nl = p->nlayers;
  for (int l = 0; l < nl; l++) count[l] = 0;
  for (size_t k = 0; k < (size_t)p->nq * nl; k++) sum[k] = 0.0;
  if (n == 0) return SPH_HIP_OK;
  SPH_HIP_TRY(hipSetDevice(e->device));
  ProfileArgs a{};
  a.p = *p;
  a.boxlo = e->box.lo[p->axis];
  a.boxhi = e->box.hi[p->axis];
  a.prd = e->box.prd[p->axis];
  a.periodic = e->box.periodic[p->axis];
  hipStream_t s = e->s;
  e->pf_key.reserve(n);
  e->pf_key2.reserve(n);
  e->pf_idx.reserve(n);
  e->pf_idx2.reserve(n);
  e->pf_cnt.reserve(nl);
  e->pf_sum.reserve((size_t)std::max(p->nq, 1) * nl);
  e->launch(k_profile_keys, n, n, a, e->xf.p, e->ty.p, e->pf_key.p, e->pf_idx.p);
  int eb = 1;  // (keys 0 .. nlayers; the radix sort is stable, so rows stay in order)
  while (eb < 32 && (1u << eb) <= (unsigned)nl) eb++;
  e->cub([&](void *t, size_t &tb) {
    return hipcub::DeviceRadixSort::SortPairs(t, tb, e->pf_key.p, e->pf_key2.p, e->pf_idx.p,
                                              e->pf_idx2.p, n, 0, eb, s);
  });
  hipLaunchKernelGGL(k_profile_fold, dim3(nl), dim3(RED_THREADS), 0, s, n, a, e->pf_key2.p,
                     e->pf_idx2.p, e->vr.p, e->en.p, e->de.p, e->ty.p, e->vel.p,
                     e->mp ? (const double *)e->rm.p : nullptr,
                     e->mp ? (const double *)e->cvv.p : nullptr, cvc, e->type_mass(),
                     e->pf_cnt.p, e->pf_sum.p);
  SPH_HIP_TRY(hipGetLastError());
  static_assert(sizeof(long long) == sizeof(int64_t), "count copy");
  SPH_HIP_TRY(hipMemcpyAsync(count, e->pf_cnt.p, nl * sizeof(int64_t), hipMemcpyDeviceToHost, s));
  if (p->nq)
    e->to_host(sum, e->pf_sum.p, (size_t)p->nq * nl);
  SPH_HIP_TRY(hipStreamSynchronize(s));
  SPH_API_END
}

// the checks sph_engine_moments and sph_engine_gyration share; -> the selections as given
static void check_group_sels(const char *who, sph_engine *e, int nsel, const sph_group_sel *sel,
                             const void *in, const void *out, sph_group_sel *to) {
  SPH_REQUIRE(e, SPH_HIP_EINVAL, "%s: NULL engine", who);
  SPH_REQUIRE(nsel >= 0 && nsel <= SPH_MAX_MOMENTS, SPH_HIP_EINVAL,
              "%s: %d selections outside [0,%d]", who, nsel, SPH_MAX_MOMENTS);
  SPH_REQUIRE(nsel == 0 || (sel && in && out), SPH_HIP_EINVAL, "%s: NULL argument", who);
  SPH_REQUIRE(e->setup_done, SPH_HIP_EINVAL, "%s: call sph_engine_setup first", who);
  for (int k = 0; k < nsel; k++) {
    check_region(who, sel[k].region_mode, sel[k].region);
    to[k] = sel[k];
  }
}

int sph_engine_moments(sph_engine *e, int nsel, const sph_group_sel *sel, sph_moments_out *out) {
  SPH_API_BEGIN
  MomentsArgs a{};
  check_group_sels("sph_engine_moments", e, nsel, sel, sel, out, a.sel);
  if (nsel == 0) return SPH_HIP_OK;
  a.nsel = nsel;
  for (int d = 0; d < 3; d++) a.prd[d] = e->box.prd[d];
  const int n = e->nlocal;
  if (n == 0) {
    for (int k = 0; k < nsel; k++) {
      out[k] = sph_moments_out{};
      for (int d = 0; d < 3; d++) {
        out[k].lo[d] = HUGE_VAL;
        out[k].hi[d] = -HUGE_VAL;
      }
    }
    return SPH_HIP_OK;
  }
  SPH_HIP_TRY(hipSetDevice(e->device));
  const int nb = (int)std::min<long>(blocks(n), RED_MAXBLOCKS);
  const size_t npart = (size_t)RED_MAXBLOCKS * SPH_MAX_MOMENTS * MOM_SLOTS;
  e->mom_buf.reserve(npart + SPH_MAX_MOMENTS * MOM_SLOTS);
  double *part = e->mom_buf.p, *res = e->mom_buf.p + npart;
  const double *rm = e->mp ? (const double *)e->rm.p : nullptr;
  // (up to four selections keep a smaller register file: more waves per SIMD)
  auto stage1 = nsel <= 4 ? k_moments_part<4> : k_moments_part<SPH_MAX_MOMENTS>;
  hipLaunchKernelGGL(stage1, dim3(nb), dim3(RED_THREADS), 0, e->s, n, a, e->xf.p, e->vr.p,
                     e->ty.p, e->vel.p, rm, e->type_mass(), part);
  hipLaunchKernelGGL(k_moments_final, dim3(1), dim3(SPH_MAX_MOMENTS * MOM_SLOTS), 0, e->s, nb,
                     nsel, part, res);
  SPH_HIP_TRY(hipGetLastError());
  e->to_host((double *)out, res, (size_t)nsel * MOM_OUT);
  SPH_HIP_TRY(hipStreamSynchronize(e->s));
  SPH_API_END
}

int sph_engine_gyration(sph_engine *e, int nsel, const sph_group_sel *sel, const double *cm,
                        double *out) {
  SPH_API_BEGIN
  GyrationArgs a{};
  check_group_sels("sph_engine_gyration", e, nsel, sel, cm, out, a.sel);
  if (nsel == 0) return SPH_HIP_OK;
  a.nsel = nsel;
  for (int d = 0; d < 3; d++) a.prd[d] = e->box.prd[d];
  for (int k = 0; k < nsel; k++)
    for (int d = 0; d < 3; d++) a.cm[k][d] = cm[3 * k + d];
  const int n = e->nlocal;
  if (n == 0) {
    for (int k = 0; k < nsel * GYR_OUT; k++) out[k] = 0.0;
    return SPH_HIP_OK;
  }
  SPH_HIP_TRY(hipSetDevice(e->device));
  const int nb = (int)std::min<long>(blocks(n), RED_MAXBLOCKS);
  const size_t npart = (size_t)RED_MAXBLOCKS * SPH_MAX_MOMENTS * MOM_SLOTS;
  e->mom_buf.reserve(npart + SPH_MAX_MOMENTS * MOM_SLOTS);
  double *part = e->mom_buf.p, *res = e->mom_buf.p + npart;
  hipLaunchKernelGGL(k_gyration_part, dim3(nb), dim3(RED_THREADS), 0, e->s, n, a, e->xf.p,
                     e->ty.p, e->vel.p, e->mp ? (const double *)e->rm.p : nullptr,
                     e->type_mass(), part);
  hipLaunchKernelGGL(k_gyration_final, dim3(1), dim3(SPH_MAX_MOMENTS * GYR_SLOTS), 0, e->s, nb,
                     nsel, part, res);
  SPH_HIP_TRY(hipGetLastError());
  e->to_host(out, res, (size_t)nsel * GYR_OUT);
  SPH_HIP_TRY(hipStreamSynchronize(e->s));
  SPH_API_END
}

int sph_engine_get_atoms_multiphase(sph_engine *e, double *rmass, double *cv, double *cg,
                                    double *vest, int *type, int64_t *ninserted) {
  SPH_API_BEGIN
  SPH_REQUIRE(e, SPH_HIP_EINVAL, "sph_engine_get_atoms_multiphase: NULL engine");
  SPH_HIP_TRY(hipSetDevice(e->device));
  if (ninserted) *ninserted = e->pc_inserted;
  const int n = e->nlocal;
  if (n == 0) return SPH_HIP_OK;
  std::vector<double> hm(n, 0.0), hc(n, 1.0);
  std::vector<double4> hg(n, make_double4(0, 0, 0, 0)), hv(n);
  std::vector<int> ht(n), hty(n);
  if (e->mp) {
    e->to_host(hm.data(), e->rm.p, n);
    e->to_host(hc.data(), e->cvv.p, n);
    e->to_host(hg.data(), e->cg.p, n);
  }
  e->to_host(hv.data(), e->vr.p, n);
  e->to_host(hty.data(), e->ty.p, n);
  e->to_host(ht.data(), e->tag.p, n);
  SPH_HIP_TRY(hipStreamSynchronize(e->s));
  const bool local_order = e->multi() || e->global_tags;
  for (int i = 0; i < n; i++) {
    const int t = local_order ? i : ht[i];
    SPH_REQUIRE(t >= 0 && t < n, SPH_HIP_ERUNTIME, "corrupt tag %d", t);
    if (rmass) rmass[t] = e->mp ? hm[i] : e->cfg.mass[hty[i]];
    if (cv) cv[t] = hc[i];
    if (cg) {
      cg[3 * t] = hg[i].x;
      cg[3 * t + 1] = hg[i].y;
      cg[3 * t + 2] = hg[i].z;
    }
    if (vest) {
      vest[3 * t] = hv[i].x;
      vest[3 * t + 1] = hv[i].y;
      vest[3 * t + 2] = hv[i].z;
    }
    if (type) type[t] = hty[i];
  }
  SPH_API_END
}

// LAMMPS ubuf (lmptype.h): an integer stored as the bit pattern of an int64 in a double
static double ubuf_d(int64_t v) {
  double d;
  memcpy(&d, &v, sizeof d);
  return d;
}
static int64_t ubuf_i(double d) {
  int64_t v;
  memcpy(&v, &d, sizeof v);
  return v;
}

int sph_engine_write_restart(sph_engine *e, double *buf, int64_t cap, int *rec_size) {
  SPH_API_BEGIN
  SPH_REQUIRE(e, SPH_HIP_EINVAL, "sph_engine_write_restart: NULL engine");
  SPH_REQUIRE(!e->multi() && !e->global_tags, SPH_HIP_EINVAL,
              "sph_engine_write_restart: one brick with implicit tags");
  const int rec = e->mp ? 21 : 17;
  if (rec_size) *rec_size = rec;
  if (!buf) return SPH_HIP_OK;
  const int n = e->nlocal;
  SPH_REQUIRE(cap >= (int64_t)n * rec, SPH_HIP_EINVAL,
              "sph_engine_write_restart: buffer of %lld doubles < %lld", (long long)cap,
              (long long)n * rec);
  if (n == 0) return SPH_HIP_OK;
  SPH_HIP_TRY(hipSetDevice(e->device));
  std::vector<double4> hx(n), hv(n), hr(n), hg(n, make_double4(0, 0, 0, 0));
  std::vector<double> he(n), hm(n, 0.0), hc(n, 1.0);
  std::vector<int> ht(n), hty(n);
  e->to_host(hx.data(), e->xf.p, n);
  e->to_host(hv.data(), e->vel.p, n);
  e->to_host(hr.data(), e->vr.p, n);
  e->to_host(he.data(), e->en.p, n);
  e->to_host(hty.data(), e->ty.p, n);
  e->to_host(ht.data(), e->tag.p, n);
  if (e->mp) {
    e->to_host(hm.data(), e->rm.p, n);
    e->to_host(hc.data(), e->cvv.p, n);
    e->to_host(hg.data(), e->cg.p, n);
  }
  SPH_HIP_TRY(hipStreamSynchronize(e->s));
  for (int i = 0; i < n; i++) {
    const int t = ht[i];
    SPH_REQUIRE(t >= 0 && t < n, SPH_HIP_ERUNTIME, "corrupt tag %d", t);
    const double cv = e->mp ? hc[i] : (t < (int)e->cv_by_tag.size() ? e->cv_by_tag[t] : 1.0);
    double *o = buf + (size_t)rec * t;
    const int img = (int)hv[i].w;
    int m = 0;
    o[m++] = rec;
    o[m++] = hx[i].x;
    o[m++] = hx[i].y;
    o[m++] = hx[i].z;
    if (e->mp) {  // plain doubles (atom_vec_meso_multiphase.cpp:892-895)
      o[m++] = t + 1;
      o[m++] = hty[i];
      o[m++] = 1;
      o[m++] = img;
    } else {  // ubuf bit patterns (atom_vec_meso.cpp:731-734)
      o[m++] = ubuf_d(t + 1);
      o[m++] = ubuf_d(hty[i]);
      o[m++] = ubuf_d(1);
      o[m++] = ubuf_d(img);
    }
    o[m++] = hv[i].x;
    o[m++] = hv[i].y;
    o[m++] = hv[i].z;
    o[m++] = hr[i].w;
    if (e->mp) {
      o[m++] = hg[i].x;
      o[m++] = hg[i].y;
      o[m++] = hg[i].z;
      o[m++] = hm[i];
    }
    o[m++] = he[i];
    o[m++] = cv;
    o[m++] = hr[i].x;
    o[m++] = hr[i].y;
    o[m++] = hr[i].z;
  }
  SPH_API_END
}

int sph_engine_read_restart(sph_engine *e, int n, const double *buf) {
  SPH_API_BEGIN
  SPH_REQUIRE(e && n >= 0 && (n == 0 || buf), SPH_HIP_EINVAL,
              "sph_engine_read_restart: bad argument");
  SPH_REQUIRE(!e->multi(), SPH_HIP_EINVAL, "sph_engine_read_restart: one brick");
  const int rec = e->mp ? 21 : 17;
  std::vector<double> x(3 * (size_t)n), v(3 * (size_t)n), vest(3 * (size_t)n), rho(n), en(n),
      cv(n), rm(n), cg(3 * (size_t)n);
  std::vector<int> type(n), img(n), seen(n, 0);
  for (int k = 0; k < n; k++) {
    const double *o = buf + (size_t)rec * k;
    SPH_REQUIRE((int)o[0] == rec, SPH_HIP_EINVAL,
                "record %d has %g values, this engine's layout has %d", k, o[0], rec);
    int64_t tg, ty, im;
    if (e->mp) {
      tg = (int64_t)o[4];
      ty = (int64_t)o[5];
      im = (int64_t)o[7];
    } else {
      tg = ubuf_i(o[4]);
      ty = ubuf_i(o[5]);
      im = ubuf_i(o[7]);
    }
    SPH_REQUIRE(tg >= 1 && tg <= n && !seen[tg - 1], SPH_HIP_EINVAL,
                "record %d: tag %lld is not a new one of 1..%d", k, (long long)tg, n);
    const int i = (int)tg - 1;
    seen[i] = 1;
    type[i] = (int)ty;
    img[i] = (int)im;
    int m = 8;
    for (int d = 0; d < 3; d++) {
      x[3 * i + d] = o[1 + d];
      v[3 * i + d] = o[m++];
    }
    rho[i] = o[m++];
    if (e->mp) {
      for (int d = 0; d < 3; d++) cg[3 * i + d] = o[m++];
      rm[i] = o[m++];
    }
    en[i] = o[m++];
    cv[i] = o[m++];
    for (int d = 0; d < 3; d++) vest[3 * i + d] = o[m++];
  }
  int rc = sph_engine_set_atoms(e, n, x.data(), v.data(), type.data(), rho.data(), en.data(),
                                cv.data());
  if (rc != SPH_HIP_OK) return rc;
  if (e->mp) {
    rc = sph_engine_set_atoms_multiphase(e, rm.data(), cv.data(), cg.data());
    if (rc != SPH_HIP_OK) return rc;
  }
  if (n > 0) {  // vest and the image flags, which set_atoms does not take
    std::vector<double4> hr(n), hv(n);
    for (int i = 0; i < n; i++) {
      hr[i] = make_double4(vest[3 * i], vest[3 * i + 1], vest[3 * i + 2], rho[i]);
      hv[i] = make_double4(v[3 * i], v[3 * i + 1], v[3 * i + 2], (double)img[i]);
    }
    e->to_dev(e->vr.p, hr.data(), n);
    e->to_dev(e->vel.p, hv.data(), n);
    SPH_HIP_TRY(hipStreamSynchronize(e->s));
  }
  SPH_API_END
}

int sph_engine_setup(sph_engine *e) {
  SPH_API_BEGIN
  SPH_REQUIRE(e, SPH_HIP_EINVAL, "sph_engine_setup: NULL engine");
  SPH_REQUIRE(!e->multi() || e->tr, SPH_HIP_ECOMM,
              "brick %d of %d: attach a communicator (sph_engine_comm_init / _comm_local) first",
              e->me, e->nprocs);
  SPH_REQUIRE(e->cutneighmax > 0.0, SPH_HIP_EINVAL, "no pair style enabled / zero cutoff");
  SPH_HIP_TRY(hipSetDevice(e->device));
  e->setup();
  SPH_HIP_TRY(hipGetLastError());
  SPH_API_END
}

int sph_engine_run(sph_engine *e, int nsteps) {
  SPH_API_BEGIN
  SPH_REQUIRE(e && nsteps >= 0, SPH_HIP_EINVAL, "sph_engine_run: bad argument");
  SPH_REQUIRE(e->setup_done, SPH_HIP_EINVAL, "sph_engine_run: call sph_engine_setup first");
  SPH_HIP_TRY(hipSetDevice(e->device));
  e->run(nsteps);
  SPH_API_END
}

int sph_engine_neigh_modify(sph_engine *e, int every, int delay, int check) {
  SPH_API_BEGIN
  // (the arguments first: they are judged the same with or without an engine)
  SPH_REQUIRE(every > 0 && delay >= 0, SPH_HIP_EINVAL,
              "sph_engine_neigh_modify: every %d must be positive, delay %d not negative", every,
              delay);
  SPH_REQUIRE(delay == 0 || delay % every == 0, SPH_HIP_EINVAL,
              "Neighbor delay must be 0 or multiple of every setting (every %d delay %d)", every,
              delay);
  SPH_REQUIRE(check == 0 || check == 1, SPH_HIP_EINVAL,
              "sph_engine_neigh_modify: check %d is neither 0 (no) nor 1 (yes)", check);
  SPH_REQUIRE(e, SPH_HIP_EINVAL, "sph_engine_neigh_modify: NULL engine");
  SPH_REQUIRE(!e->setup_done, SPH_HIP_EINVAL,
              "sph_engine_neigh_modify: before sph_engine_setup (the setup takes the hold "
              "positions)");
  e->nm_set = true;
  e->nm_every = every;
  e->nm_delay = delay;
  e->nm_check = check != 0;
  SPH_API_END
}

int sph_engine_neigh_stats(sph_engine *e, sph_neigh_stats *out) {
  SPH_API_BEGIN
  SPH_REQUIRE(e && out, SPH_HIP_EINVAL, "sph_engine_neigh_stats: NULL argument");
  out->builds = e->nm_builds;
  out->dangerous = e->nm_danger;
  out->checks = e->nm_checks;
  out->last_build = e->last_build;
  SPH_API_END
}

int sph_engine_dt_reset(sph_engine *e, const sph_dtreset *fix) {
  SPH_API_BEGIN
  SPH_REQUIRE(e && fix, SPH_HIP_EINVAL, "sph_engine_dt_reset: NULL argument");
  // "Illegal fix dt/reset command" (fix_dt_reset.cpp:52-67)
  SPH_REQUIRE(fix->nevery >= 1, SPH_HIP_EINVAL, "sph_engine_dt_reset: nevery %d < 1",
              fix->nevery);
  SPH_REQUIRE(!(fix->minbound && fix->tmin < 0.0) && !(fix->maxbound && fix->tmax < 0.0),
              SPH_HIP_EINVAL, "sph_engine_dt_reset: a negative bound (tmin %g, tmax %g)",
              fix->tmin, fix->tmax);
  SPH_REQUIRE(!(fix->minbound && fix->maxbound && fix->tmin >= fix->tmax), SPH_HIP_EINVAL,
              "sph_engine_dt_reset: tmin %g >= tmax %g", fix->tmin, fix->tmax);
  SPH_REQUIRE(fix->xmax > 0.0, SPH_HIP_EINVAL, "sph_engine_dt_reset: xmax %g <= 0", fix->xmax);
  SPH_REQUIRE(fix->type_mask >= 0, SPH_HIP_EINVAL, "sph_engine_dt_reset: type_mask %d",
              fix->type_mask);
  SPH_REQUIRE(!e->setup_done, SPH_HIP_EINVAL,
              "sph_engine_dt_reset: before sph_engine_setup (the setup runs the fix's first "
              "end_of_step)");
  SPH_REQUIRE(!e->dtr_on, SPH_HIP_EINVAL, "sph_engine_dt_reset: the fix is armed already");
  SPH_REQUIRE(!e->pc, SPH_HIP_EINVAL,
              "sph_engine_dt_reset: not together with sph_engine_phase_change (the fix's "
              "ENERGY-rate threshold reads update->dt, which then lives on the device)");
  e->dtr_on = true;
  e->dtr_nevery = fix->nevery;
  e->dtr.minbound = fix->minbound != 0;
  e->dtr.maxbound = fix->maxbound != 0;
  e->dtr.tmin = fix->tmin;
  e->dtr.tmax = fix->tmax;
  e->dtr.xmax = fix->xmax;
  e->dtr.ftm2v = e->cfg.ftm2v > 0 ? e->cfg.ftm2v : 1.0;
  e->dtr.type_mask = fix->type_mask;
  SPH_API_END
}

int sph_engine_dt_stats(sph_engine *e, sph_dt_stats *out) {
  SPH_API_BEGIN
  SPH_REQUIRE(e && out, SPH_HIP_EINVAL, "sph_engine_dt_stats: NULL argument");
  SPH_REQUIRE(e->setup_done, SPH_HIP_EINVAL, "sph_engine_dt_stats: after sph_engine_setup");
  if (!e->dtr_on) {
    out->dt = e->cfg.dt;
    out->time = (double)e->step * e->cfg.dt;
    out->laststep = out->changes = 0;
  } else {
    SPH_HIP_TRY(hipSetDevice(e->device));
    e->to_host(e->h_dt, e->dt_rec.p, 1);
    SPH_HIP_TRY(hipStreamSynchronize(e->s));
    const DtRecord &r = *e->h_dt;
    out->dt = r.dt;
    // Thermo's time (thermo.cpp:1500)
    out->time = r.atime + (double)((long long)e->step - r.atimestep) * r.dt;
    out->laststep = r.laststep;
    out->changes = r.changes;
  }
  SPH_API_END
}

int sph_engine_virial_every(sph_engine *e, int nevery) {
  SPH_API_BEGIN
  SPH_REQUIRE(e, SPH_HIP_EINVAL, "sph_engine_virial_every: NULL engine");
  SPH_REQUIRE(nevery >= 0, SPH_HIP_EINVAL, "sph_engine_virial_every: nevery %d < 0", nevery);
  SPH_REQUIRE(!e->setup_done, SPH_HIP_EINVAL,
              "sph_engine_virial_every: before sph_engine_setup (the setup step's force pass "
              "tallies the first virial)");
  SPH_REQUIRE(!e->mp, SPH_HIP_EINVAL,
              "sph_engine_virial_every: the multiphase styles have no virial here "
              "(sph_engine_thermo still gives their kinetic and gravity sums)");
  e->vir_every = nevery;
  SPH_API_END
}

int sph_engine_thermo(sph_engine *e, double mvv2e, double nktv2p, sph_thermo_out *out) {
  SPH_API_BEGIN
  SPH_REQUIRE(e && out, SPH_HIP_EINVAL, "sph_engine_thermo: NULL argument");
  SPH_REQUIRE(e->setup_done, SPH_HIP_EINVAL, "sph_engine_thermo: call sph_engine_setup first");
  SPH_HIP_TRY(hipSetDevice(e->device));
  const int n = e->nlocal;
  double th[TH_NS] = {}, w[VIR_NS] = {};
  const int nb = (int)std::min<long>(blocks(n), RED_MAXBLOCKS);
  if (nb) {
    e->vir_part.reserve((size_t)RED_MAXBLOCKS * TH_NS);
    e->th_tot.reserve(TH_NS);
    hipLaunchKernelGGL(k_thermo_part, dim3(nb), dim3(RED_THREADS), 0, e->s, n, e->xf.p, e->ty.p,
                       e->vel.p, e->mp ? (const double *)e->rm.p : nullptr, e->type_mass(),
                       e->cfg.gravity_mask, e->cfg.gravity[0], e->cfg.gravity[1],
                       e->cfg.gravity[2], e->vir_part.p);
    hipLaunchKernelGGL(k_slots_final, dim3(1), dim3(64), 0, e->s, nb, TH_NS, 1.0, e->vir_part.p,
                       e->th_tot.p);
    SPH_HIP_TRY(hipGetLastError());
    e->to_host(th, e->th_tot.p, TH_NS);
  }
  if (e->vir_step >= 0) e->to_host(w, e->vir_tot.p, VIR_NS);
  SPH_HIP_TRY(hipStreamSynchronize(e->s));
  out->virial_step = e->vir_step;
  for (int k = 0; k < 6; k++) {
    out->virial[k] = w[k];
    out->ke_tensor[k] = th[k] * mvv2e;
  }
  out->ke = th[6] * mvv2e;
  out->egrav = th[7];
  const int dim = e->cfg.dim;
  out->volume = e->box.prd[0] * e->box.prd[1] * (dim == 3 ? e->box.prd[2] : 1.0);
  // ComputePressure::compute_scalar (compute_pressure.cpp:193-207) with keflag: dof * boltz * t
  // of compute temp is sum m |v|^2 * mvv2e
  const double trace = w[0] + w[1] + (dim == 3 ? w[2] : 0.0);
  out->press = (e->vir_step >= 0 && e->vir_step == e->step)
                   ? (2.0 * out->ke + trace) / ((double)dim * out->volume) * nktv2p
                   : std::nan("");
  SPH_API_END
}

int sph_engine_pair_passes(sph_engine *e, int n) {
  SPH_API_BEGIN
  SPH_REQUIRE(e && n >= 0, SPH_HIP_EINVAL, "sph_engine_pair_passes: bad argument");
  SPH_REQUIRE(e->setup_done, SPH_HIP_EINVAL, "sph_engine_pair_passes: call setup first");
  SPH_HIP_TRY(hipSetDevice(e->device));
  for (int k = 0; k < n; k++) e->pair_compute(e->cfg.rhosum_nstep > 0);
  SPH_HIP_TRY(hipGetLastError());
  SPH_API_END
}

int sph_engine_rebuild_passes(sph_engine *e, int n) {
  SPH_API_BEGIN
  SPH_REQUIRE(e && n >= 0, SPH_HIP_EINVAL, "sph_engine_rebuild_passes: bad argument");
  SPH_REQUIRE(e->setup_done, SPH_HIP_EINVAL, "sph_engine_rebuild_passes: call setup first");
  SPH_HIP_TRY(hipSetDevice(e->device));
  for (int k = 0; k < n; k++) {
    e->force_sort = true;  // (the full rebuild, sort included)
    e->rebuild();
  }
  SPH_HIP_TRY(hipGetLastError());
  SPH_API_END
}

int sph_engine_nlocal(sph_engine *e) { return e ? e->nlocal : 0; }

int sph_engine_get_atoms(sph_engine *e, double *x, double *v, double *rho, double *en,
                         double *f, double *drho, double *de, int *tag) {
  SPH_API_BEGIN
  SPH_REQUIRE(e, SPH_HIP_EINVAL, "sph_engine_get_atoms: NULL engine");
  SPH_HIP_TRY(hipSetDevice(e->device));
  const int n = e->nlocal;
  if (n == 0) return SPH_HIP_OK;
  std::vector<double4> hx(n), hv(n), hvel(n), hf(n);
  std::vector<double> hen(n), hde(n);
  std::vector<int> ht(n);
  e->to_host(hx.data(), e->xf.p, n);
  e->to_host(hv.data(), e->vr.p, n);
  e->to_host(hvel.data(), e->vel.p, n);
  e->to_host(hf.data(), e->fo.p, n);
  e->to_host(hen.data(), e->en.p, n);
  e->to_host(hde.data(), e->de.p, n);
  e->to_host(ht.data(), e->tag.p, n);
  SPH_HIP_TRY(hipStreamSynchronize(e->s));
  // one brick of a decomposition (or caller tags): local slot order, tag[] names the atom;
  // otherwise the set_atoms order
  const bool local_order = e->multi() || e->global_tags;
  for (int i = 0; i < n; i++) {
    const int t = local_order ? i : ht[i];
    SPH_REQUIRE(t >= 0 && t < n, SPH_HIP_ERUNTIME, "corrupt tag %d", t);
    if (x) {
      x[3 * t] = hx[i].x;
      x[3 * t + 1] = hx[i].y;
      x[3 * t + 2] = hx[i].z;
    }
    if (v) {
      v[3 * t] = hvel[i].x;
      v[3 * t + 1] = hvel[i].y;
      v[3 * t + 2] = hvel[i].z;
    }
    if (rho) rho[t] = hv[i].w;
    if (en) en[t] = hen[i];
    if (f) {
      f[3 * t] = hf[i].x;
      f[3 * t + 1] = hf[i].y;
      f[3 * t + 2] = hf[i].z;
    }
    if (drho) drho[t] = hf[i].w;
    if (de) de[t] = hde[i];
    if (tag) tag[t] = ht[i];
  }
  SPH_API_END
}

int sph_engine_neighbor_counts(sph_engine *e, int *numneigh) {
  SPH_API_BEGIN
  SPH_REQUIRE(e && numneigh, SPH_HIP_EINVAL, "sph_engine_neighbor_counts: bad argument");
  SPH_HIP_TRY(hipSetDevice(e->device));
  const int n = e->nlocal;
  if (n == 0) return SPH_HIP_OK;
  std::vector<int> hc(n), ht(n);
  e->to_host(hc.data(), e->ccnt.p, n);
  e->to_host(ht.data(), e->tag.p, n);
  SPH_HIP_TRY(hipStreamSynchronize(e->s));
  const bool local_order = e->multi() || e->global_tags;
  for (int i = 0; i < n; i++) numneigh[local_order ? i : ht[i]] = hc[i];
  SPH_API_END
}

int sph_engine_stats_get(sph_engine *e, sph_engine_stats *st) {
  SPH_API_BEGIN
  SPH_REQUIRE(e && st, SPH_HIP_EINVAL, "sph_engine_stats_get: bad argument");
  SPH_HIP_TRY(hipSetDevice(e->device));
  e->harvest();
  st->step = e->step;
  st->nlocal = e->nlocal;
  st->nghost = e->nghost;
  st->nbr_full = e->list_entries();
  st->nbr_builds = e->nbr_builds;
  st->nbr_maxrow = e->nbr_maxrow;
  st->staged = e->blk ? 1 : 0;
  st->stage_max = e->blk ? e->blk_um : 0;
  st->ms_rhosum = e->ms[T_RHO];
  st->ms_tait = e->ms[T_TAIT];
  st->ms_heat = e->ms[T_HEAT];
  st->ms_integrate = e->ms[T_INT];
  st->ms_comm = e->ms[T_COMM];
  st->ms_neigh = e->ms[T_NEIGH];
  st->n_rhosum = e->nlaunch[T_RHO];
  st->n_tait = e->nlaunch[T_TAIT];
  st->n_heat = e->nlaunch[T_HEAT];
  st->n_neigh = e->nlaunch[T_NEIGH];
  st->blk_nbig = 0;
  if (e->blk && e->mx.p) {  // (k_blk_count_big of the last block build)
    e->to_host(&st->blk_nbig, e->mx.p + 9, 1);
    SPH_HIP_TRY(hipStreamSynchronize(e->s));
  }
  st->inner_rows = e->inner ? 1 : 0;
  st->inner_live = 0;
  if (e->inner && e->moved.p) {
    int mv = 1;
    e->to_host(&mv, e->moved_flag(), 1);
    SPH_HIP_TRY(hipStreamSynchronize(e->s));
    st->inner_live = mv == 0 ? 1 : 0;
  }
  st->flags = (e->rho_fused_step >= 0 && e->rho_fused_step == e->step) ? SPH_STAT_RHO_FUSED : 0;
  if (e->blk) st->flags |= e->blk_flags;
  if (e->mp) st->flags |= e->mp_flags;
  // (like the other families, not on the single-phase row path, whose flags stay bit 0 alone:
  // sph_engine_csort_paths answers there too)
  if (e->blk || e->mp) st->flags |= e->cs_flags;
  st->flags |= e->fuse_flag;  // (only ever set on the block path: fuse_step)
  st->inner_refresh = e->inner_refreshes;
  SPH_API_END
}

int sph_engine_set_timing(sph_engine *e, int on) {
  SPH_API_BEGIN
  SPH_REQUIRE(e, SPH_HIP_EINVAL, "sph_engine_set_timing: NULL engine");
  SPH_HIP_TRY(hipSetDevice(e->device));
  e->harvest();
  // 1: every class; (mask << 1): the classes of mask (a timed run records an event pair per
  // timed scope, which at small sizes is a visible share of a step)
  e->timing_mask = on == 1 ? (1 << T_NCLASS) - 1 : (on > 1 ? (on >> 1) & ((1 << T_NCLASS) - 1) : 0);
  e->timing = e->timing_mask != 0;
  for (int k = 0; k < T_NCLASS; k++) {
    e->ms[k] = 0.0;
    e->nlaunch[k] = 0;
  }
  SPH_API_END
}

int sph_engine_sync(sph_engine *e) {
  SPH_API_BEGIN
  SPH_REQUIRE(e, SPH_HIP_EINVAL, "sph_engine_sync: NULL engine");
  SPH_HIP_TRY(hipSetDevice(e->device));
  SPH_HIP_TRY(hipStreamSynchronize(e->s));
  SPH_API_END
}

int sph_engine_comm_uid(void *uid128) {
  SPH_API_BEGIN
  SPH_REQUIRE(uid128, SPH_HIP_EINVAL, "sph_engine_comm_uid: NULL buffer");
  static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId is 128 bytes");
  ncclUniqueId id;
  SPH_NCCL_TRY(ncclGetUniqueId(&id));
  memcpy(uid128, &id, sizeof(id));
  SPH_API_END
}

static void attach(sph_engine *e, Transport *t) {
  const int sz = t->size(), rk = t->rank();
  if (sz != e->nprocs || rk != e->me) {
    delete t;
    SPH_REQUIRE(false, SPH_HIP_EINVAL,
                "communicator rank %d/%d does not match the engine's brick %d/%d", rk, sz,
                e->me, e->nprocs);
  }
  delete e->tr;
  e->tr = t;
}

int sph_engine_comm_init(sph_engine *e, const void *uid128, int nranks, int rank) {
  SPH_API_BEGIN
  SPH_REQUIRE(e && uid128, SPH_HIP_EINVAL, "sph_engine_comm_init: NULL argument");
  SPH_HIP_TRY(hipSetDevice(e->device));
  ncclUniqueId id;
  memcpy(&id, uid128, sizeof(id));
  attach(e, new RcclTransport(id, nranks, rank));
  SPH_API_END
}

int sph_engine_comm_loopback(sph_engine *e, int on) {
  SPH_API_BEGIN
  SPH_REQUIRE(e, SPH_HIP_EINVAL, "sph_engine_comm_loopback: NULL engine");
  SPH_REQUIRE(e->nprocs == 1 && e->tr, SPH_HIP_ECOMM,
              "sph_engine_comm_loopback: needs a one-brick engine with a communicator attached");
  e->loopback = on != 0;
  e->setup_done = false;
  SPH_API_END
}

int sph_local_world_create(int nranks, sph_local_world **out) {
  SPH_API_BEGIN
  SPH_REQUIRE(out && nranks >= 1, SPH_HIP_EINVAL, "sph_local_world_create: bad argument");
  *out = reinterpret_cast<sph_local_world *>(new LocalWorld(nranks));
  SPH_API_END
}

int sph_local_world_destroy(sph_local_world *w) {
  delete reinterpret_cast<LocalWorld *>(w);
  return SPH_HIP_OK;
}

int sph_engine_comm_local(sph_engine *e, sph_local_world *w, int rank) {
  SPH_API_BEGIN
  SPH_REQUIRE(e && w, SPH_HIP_EINVAL, "sph_engine_comm_local: NULL argument");
  LocalWorld *lw = reinterpret_cast<LocalWorld *>(w);
  SPH_REQUIRE(rank >= 0 && rank < lw->n, SPH_HIP_EINVAL, "rank %d outside [0,%d)", rank, lw->n);
  attach(e, new LocalTransport(lw, rank));
  SPH_API_END
}

int sph_engine_comm_ipc(sph_engine *e, const char *name, int nranks, int rank, int mode) {
  SPH_API_BEGIN
  SPH_REQUIRE(e && name, SPH_HIP_EINVAL, "sph_engine_comm_ipc: NULL argument");
  SPH_HIP_TRY(hipSetDevice(e->device));
  attach(e, new IpcTransport(name, nranks, rank, mode, e->device));
  SPH_API_END
}

int sph_engine_tune(sph_engine *e, int key, int value) {
  SPH_API_BEGIN
  SPH_REQUIRE(e, SPH_HIP_EINVAL, "sph_engine_tune: NULL engine");
  SPH_REQUIRE(!e->setup_done, SPH_HIP_EINVAL, "sph_engine_tune: before sph_engine_setup");
  switch (key) {
    case SPH_TUNE_OVERLAP: e->overlap = value != 0; break;
    case SPH_TUNE_BLKUMF:
      SPH_REQUIRE(value >= 0, SPH_HIP_EINVAL, "sph_engine_tune: BLKUMF %d < 0", value);
      e->blkumf = value;
      break;
    case SPH_TUNE_CSORT:
      SPH_REQUIRE(value >= 0 && value <= 2, SPH_HIP_EINVAL, "sph_engine_tune: CSORT %d", value);
      e->csort = value;
      break;
    case SPH_TUNE_FUSEINT:
      SPH_REQUIRE(value == 0 || value == 1, SPH_HIP_EINVAL, "sph_engine_tune: FUSEINT %d", value);
      e->fuseint = value != 0;
      break;
    default: SPH_REQUIRE(false, SPH_HIP_EINVAL, "sph_engine_tune: unknown key %d", key);
  }
  SPH_API_END
}

int sph_engine_csort_paths(sph_engine *e, int *mask) {
  SPH_API_BEGIN
  SPH_REQUIRE(e && mask, SPH_HIP_EINVAL, "sph_engine_csort_paths: NULL argument");
  *mask = e->cs_flags;
  SPH_API_END
}

int sph_engine_set_tags(sph_engine *e, const int *tags) {
  SPH_API_BEGIN
  SPH_REQUIRE(e && (tags || e->nlocal == 0), SPH_HIP_EINVAL, "sph_engine_set_tags: bad argument");
  SPH_HIP_TRY(hipSetDevice(e->device));
  int mx = -1;
  for (int i = 0; i < e->nlocal; i++) {
    SPH_REQUIRE(tags[i] >= 0 && tags[i] < (1 << 30), SPH_HIP_EINVAL,
                "sph_engine_set_tags: tag %d outside [0, 2^30)", tags[i]);
    mx = std::max(mx, tags[i]);
  }
  if (e->nlocal)
    SPH_HIP_TRY(hipMemcpy(e->tag.p, tags, e->nlocal * sizeof(int), hipMemcpyHostToDevice));
  e->global_tags = true;
  e->tag_next = mx + 1;  // (bricks: the ranks agree on the largest at the first phase change)
  e->pc_tags_agreed = false;
  e->lidx_valid = false;  // (read order = tag order, taken at setup)
  SPH_API_END
}

int sph_engine_atom_sort(sph_engine *e, int sortfreq, double binsize) {
  SPH_API_BEGIN
  SPH_REQUIRE(e, SPH_HIP_EINVAL, "sph_engine_atom_sort: NULL engine");
  SPH_REQUIRE(sortfreq >= 0 && binsize >= 0.0, SPH_HIP_EINVAL, "Illegal atom_modify command");
  e->sortfreq = sortfreq;
  e->sort_binsize = binsize;
  SPH_API_END
}

}  // extern "C"
