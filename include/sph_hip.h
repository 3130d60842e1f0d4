/*
 * sph_hip.h -- C ABI of the MI355X-native USER-SPH pair engine (libsph_hip.so).
 *
 * Two layers, both plain C (pointers + sizes, no torch/HIP types):
 *
 *  1. Pair-style layer (sph_hip_*): what a LAMMPS `sph/<style>/hip` Pair class calls from
 *     its compute(), with LAMMPS' own host arrays and NeighList.  Replaces the CPU loops of
 *       PairSPHRhoSum::compute          src/USER-SPH/pair_sph_rhosum.cpp:66-204
 *       PairSPHTaitwater::compute       src/USER-SPH/pair_sph_taitwater.cpp:53-200
 *       PairSPHTaitwaterMorris::compute src/USER-SPH/pair_sph_taitwater_morris.cpp:52-200
 *       PairSPHHeatConduction::compute  src/USER-SPH/pair_sph_heatconduction.cpp:47-134
 *     (paths relative to the reference tree).  Coefficients follow each style's coeff() /
 *     init_one() semantics (tables already filled and symmetrised by LAMMPS).
 *
 *  2. Device-resident engine (sph_engine_*): the whole Verlet step of an SPH run
 *     (FixMeso integrate, pbc, borders/ghost images, binned neighbor build, rhosum ->
 *     forward comm -> taitwater[/morris] [+heatconduction], integrate) kept in HBM,
 *     optionally sharded over several GPUs by brick decomposition with the halo carried on
 *     RCCL.  Replaces, for device-resident runs, Verlet::run (src/verlet.cpp:207-309)
 *     around the same pair styles; Neighbor::full_bin (src/neigh_full.cpp:241-344);
 *     CommBrick::borders/forward_comm (src/comm_brick.cpp:444-506, 696-864);
 *     FixMeso::initial/final_integrate (src/USER-SPH/fix_meso.cpp:91-180).
 *
 * Every function returns 0 on success and a negative SPH_HIP_E* code on failure;
 * sph_hip_last_error() then describes the failure (thread-local).  As with the GPU
 * package precedent (src/GPU/pair_lj_cut_gpu.cpp:114-115) the caller turns a failure into
 * error->one(FLERR, ...).  There is no CPU fallback: without a usable HIP device every
 * compute entry point fails with SPH_HIP_ENODEV.
 *
 * Array conventions (identical to LAMMPS): per-atom vectors are AoS double[n][3]
 * (atom->x's contiguous backing, src/memory.h:124-137); per-type tables have ntypes+1
 * entries and per-type-pair tables (ntypes+1)^2 entries, row-major, 1-based types.
 */
#ifndef SPH_HIP_H
#define SPH_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SPH_HIP_ABI_VERSION 2

#define SPH_HIP_OK 0
#define SPH_HIP_EINVAL (-1)   /* bad argument / not configured */
#define SPH_HIP_ENODEV (-2)   /* no usable HIP device */
#define SPH_HIP_ERUNTIME (-3) /* HIP runtime / kernel failure */
#define SPH_HIP_ENOMEM (-4)   /* device allocation failed ("Insufficient memory on accelerator") */
#define SPH_HIP_ECOMM (-5)    /* RCCL failure */
#define SPH_HIP_EOVERFLOW (-6)/* neighbor / ghost capacity exceeded */

/* list kinds, as NeighRequest half/full (src/neigh_request.h) */
#define SPH_LIST_FULL 0
#define SPH_LIST_HALF 1

/* viscosity variants of sph/taitwater */
#define SPH_VISC_MONAGHAN 0   /* sph/taitwater        (pair_sph_taitwater.cpp:162-169) */
#define SPH_VISC_MORRIS 1     /* sph/taitwater/morris (pair_sph_taitwater_morris.cpp:163-167) */

const char *sph_hip_last_error(void);
int sph_hip_abi_version(void);
/* number of visible HIP devices (0 without a GPU; never fails) */
int sph_hip_device_count(void);

/* ======================================================================================
 * 1. Pair-style layer
 * ==================================================================================== */
typedef struct sph_hip_ctx sph_hip_ctx;

/* One context per MPI rank / Pair instance set.  dim = domain->dimension, ntypes =
   atom->ntypes, newton_pair = force->newton_pair. */
int sph_hip_create(int device, int dim, int ntypes, int newton_pair, sph_hip_ctx **out);
int sph_hip_destroy(sph_hip_ctx *ctx);
/* Device time of the last style call's kernels, in ms (HIP events recorded around the
   launches on the context's stream; staging and result copies excluded), when enabled by
   sph_hip_set_timing(ctx, 1).  Measurement support; not part of the LAMMPS pair API. */
int sph_hip_set_timing(sph_hip_ctx *ctx, int on);
int sph_hip_last_kernel_ms(sph_hip_ctx *ctx, double *ms);

/* PairSPHRhoSum::coeff/init_one: cut (nt+1)^2 (h per type pair), mass = atom->mass. */
int sph_hip_rhosum_coeff(sph_hip_ctx *ctx, const double *cut, const double *mass);
/* PairSPHTaitwater[Morris]::coeff/init_one: rho0, soundspeed, B per type (nt+1),
   viscosity and cut per pair ((nt+1)^2). visc_variant = SPH_VISC_*. */
int sph_hip_taitwater_coeff(sph_hip_ctx *ctx, int visc_variant, const double *rho0,
                            const double *soundspeed, const double *B,
                            const double *viscosity, const double *cut, const double *mass);
/* PairSPHHeatConduction::coeff/init_one: alpha and cut per pair ((nt+1)^2). */
int sph_hip_heatconduction_coeff(sph_hip_ctx *ctx, const double *alpha, const double *cut,
                                 const double *mass);
/* PairSPHIdealGas::coeff/init_one: viscosity and cut per pair ((nt+1)^2), mass = atom->mass.
   init_one of this style mirrors cut but NOT viscosity (pair_sph_idealgas.cpp:214-225), so
   the viscosity table is taken as LAMMPS holds it and read as viscosity[itype][jtype], i the
   row atom of the staged list.  (With a table that differs from its transpose a HALF list
   takes the atomics path, whose single evaluation per pair is the reference's.) */
int sph_hip_idealgas_coeff(sph_hip_ctx *ctx, const double *viscosity, const double *cut,
                           const double *mass);

/* Stage per-atom inputs: nlocal owned then nghost ghost atoms (atom->x, atom->vest,
   atom->rho, atom->e, atom->type).  vest/rho/e may be NULL when the next compute does
   not read them. */
int sph_hip_atoms(sph_hip_ctx *ctx, int nlocal, int nghost, const double *x,
                  const double *vest, const double *rho, const double *e, const int *type);
/* Restage rho only (nall values; x, vest, e, type, rmass, cv as last staged): the second
   and later pair computes of one step under hybrid/overlay, after forward_comm_pair of the
   density (the shim keys it on ntimestep + neighbor->ncalls + nlocal/nghost). */
int sph_hip_atoms_rho(sph_hip_ctx *ctx, const double *rho);
/* Restage x (and vest, rho, e where non-NULL) of the SAME atom set as the last
   sph_hip_atoms (same nlocal/nghost and types: a step between rebuilds) -- no type upload or
   check, staged lists kept. */
int sph_hip_atoms_update(sph_hip_ctx *ctx, const double *x, const double *vest,
                         const double *rho, const double *e);
/* Register the caller's per-atom arrays (capacity nmax atoms: x, vest, f nmax*3, the others
   nmax; any may be NULL) as mapped host memory: the staging kernels then read x/vest/rho/e
   straight from them over PCIe and the styles write rho / add f, drho, de straight into
   them, instead of a host copy, a PCIe copy and a host loop per call.  Call again whenever
   the arrays move (LAMMPS: atom->nmax or a pointer changed; the shim checks every compute);
   nmax = 0 unregisters.  An array the runtime refuses to register keeps the copy path. */
int sph_hip_host_arrays(sph_hip_ctx *ctx, int nmax, double *x, double *vest, double *rho,
                        double *e, double *f, double *drho, double *de);

/* Stage a LAMMPS NeighList (list->inum, ilist, numneigh, firstneigh; NEIGHMASK bits are
   stripped).  kind = SPH_LIST_FULL (gather-only kernels, nothing written to ghosts) or
   SPH_LIST_HALF (the reference's Newton-3 semantics: the j share of every pair, ghosts
   included when newton_pair is on, is gathered through the reverse of the staged half list,
   built once per upload; SPH_MPREV=0 scatters it with fp64 atomics instead).  Entries are
   checked on the device (0 <= j < nall, ilist owned): SPH_HIP_EINVAL otherwise. */
int sph_hip_list(sph_hip_ctx *ctx, int kind, int inum, const int *ilist,
                 const int *numneigh, const int *const *firstneigh);
/* sph_hip_list with reuse (the device mirror keyed by the list build):
   key >= 0 identifies the build (LAMMPS: neighbor->ncalls).  The context keeps one staged
   list per kind, so hybrid/overlay sub-styles that alternate FULL and HALF lists each keep
   theirs; a call whose (kind, key, inum) matches the staged list of that kind returns
   without touching the host list (no copy, upload or check; the reverse list is kept).
   Restaging atoms with a different nlocal/nghost drops every staged list.  key < 0 always
   uploads (= sph_hip_list). */
int sph_hip_list_keyed(sph_hip_ctx *ctx, int kind, int64_t key, int inum, const int *ilist,
                       const int *numneigh, const int *const *firstneigh);
/* The list built on the DEVICE from the staged atoms (SURVEY 8(b) device-list path; the GPU
   package's GPU_NEIGH, src/GPU/pair_lj_cut_gpu.cpp:97-104): kind SPH_LIST_FULL =
   Neighbor::full_bin membership (neigh_full.cpp:241-344: j != i, rsq <= cutneighsq[it][jt]),
   SPH_LIST_HALF = half_from_full_newton of it (neigh_derive.cpp:83-150); owned rows, ilist
   the identity.  cutneighsq = neighbor->cutneighsq ((nt+1)^2).  key as sph_hip_list_keyed:
   a staged device-built list of this kind with the same key is reused (hybrid/overlay
   sub-styles, the fix's copy).  Replaces the host NeighList copy and upload per rebuild. */
int sph_hip_build_list(sph_hip_ctx *ctx, int kind, int64_t key, const double *cutneighsq);
/* Row lengths of the staged list (inum values, in ilist order): LAMMPS' numneigh. */
int sph_hip_list_numneigh(sph_hip_ctx *ctx, int *numneigh);
/* Same, from a CSR list (row i = neigh[off[i]..off[i+1]) for owned atom i). */
int sph_hip_list_csr(sph_hip_ctx *ctx, int kind, int inum, const int64_t *off,
                     const int *neigh);

/* rho[0..nlocal) <- self term + sum over list (pair_sph_rhosum.cpp:112-195).  The
   forward_comm_pair of ghost rho stays with the caller (comm->forward_comm_pair). */
int sph_hip_rhosum(sph_hip_ctx *ctx, double *rho);
/* f (nall*3), drho, de (nall) are ACCUMULATED into (force_clear semantics stay with the
   caller).  With a FULL list only owned entries change; with a HALF list ghosts receive
   their Newton-3 share exactly as in the reference and need reverse_comm. virial may be
   NULL, else 6 doubles accumulated in the ev_tally convention (pair.cpp:770-850). */
int sph_hip_taitwater(sph_hip_ctx *ctx, double *f, double *drho, double *de,
                      double *virial);
int sph_hip_heatconduction(sph_hip_ctx *ctx, double *de);
/* sph/idealgas (PairSPHIdealGas::compute, pair_sph_idealgas.cpp:48-175): the energy EOS
   p = 0.4 e rho / m, sound speed c = sqrt(0.4 e / m), Lucy kernel, Monaghan viscosity on
   approaching pairs.  f (nall*3), drho, de (nall) ACCUMULATED with the list semantics of
   sph_hip_taitwater; reads the staged x, vest, rho, e, type -- SPH_HIP_EINVAL when the last
   sph_hip_atoms was given no e.  virial may be NULL, else every pair is tallied TWICE, as
   the reference's two ev_tally calls in a row do (:164-169). */
int sph_hip_idealgas(sph_hip_ctx *ctx, double *f, double *drho, double *de, double *virial);

/* ======================================================================================
 * 1b. Multiphase styles (atom_style meso/multiphase: per-atom rmass; quintic kernel).
 *     Tables are (nt+1)^2 row-major; like coeff()+init_one() the upper triangle i <= j is
 *     read and mirrored.  Stage atoms with sph_hip_atoms (x, vest, rho, e, type) and then
 *     sph_hip_atoms_multiphase (rmass, cv: nlocal + nghost each; cv may be NULL).
 * ==================================================================================== */
int sph_hip_atoms_multiphase(sph_hip_ctx *ctx, const double *rmass, const double *cv);

/* PairSPHRhoSumMultiphase (pair_sph_rhosum_multiphase.cpp:112-167, coeff :194-216):
   cut = h per pair; rho[0..nlocal) <- rmass_i (W(0)/h_ii^d + sum_j W(r/h)/h^d).  Full list. */
int sph_hip_rhosum_multiphase_coeff(sph_hip_ctx *ctx, const double *cut);
int sph_hip_rhosum_multiphase(sph_hip_ctx *ctx, double *rho);

/* PairSPHTaitwaterMultiphase (pair_sph_taitwater_multiphase.cpp:95-183, coeff :225-262):
   per type rho0, soundspeed, gamma, rbackground (B = c^2 rho0 / gamma); per pair viscosity
   and cut.  f (nall*3) is ACCUMULATED; HALF lists scatter onto j (newton_pair) exactly as
   the reference, including its p_j = p(rho_j; gamma[itype]) asymmetry. */
int sph_hip_taitwater_multiphase_coeff(sph_hip_ctx *ctx, const double *rho0,
                                       const double *soundspeed, const double *gamma,
                                       const double *rbackground, const double *viscosity,
                                       const double *cut);
int sph_hip_taitwater_multiphase(sph_hip_ctx *ctx, double *f);

/* PairSPHHeatConductionPhaseChange (pair_sph_heatconduction_phasechange.cpp:81-138, coeff
   :177-225): alpha, cut per pair; fixflag (int, the type whose temperature is clamped, 0 =
   none) and tc per pair, either may be NULL (4-argument coeff form).  de (nall) is
   ACCUMULATED. */
int sph_hip_heatconduction_phasechange_coeff(sph_hip_ctx *ctx, const double *alpha,
                                             const int *fixflag, const double *tc,
                                             const double *cut);
int sph_hip_heatconduction_phasechange(sph_hip_ctx *ctx, double *de);

/* PairSPHColorGradient (pair_sph_colorgradient.cpp:118-187): alpha, cut per pair;
   cg[0..nlocal)*3 is OVERWRITTEN (the reference zeroes it first).  Full list. */
int sph_hip_colorgradient_coeff(sph_hip_ctx *ctx, const double *alpha, const double *cut);
int sph_hip_colorgradient(sph_hip_ctx *ctx, double *cg);

/* PairSPHSurfaceTension (pair_sph_surfacetension.cpp:50-192, coeff :222-247): cut = h per
   pair.  cg (nall*3, atom->colorgradient of owned atoms and ghosts) is read; f (nall*3) is
   ACCUMULATED; HALF lists (the style's default request) scatter onto j when newton_pair or
   j < nlocal, as the reference. */
int sph_hip_surfacetension_coeff(sph_hip_ctx *ctx, const double *cut);
int sph_hip_surfacetension(sph_hip_ctx *ctx, const double *cg, double *f);

/* ======================================================================================
 * 1c. fix phase_change (FixPhaseChange::pre_exchange, fix_phase_change.cpp:167-352)
 * ==================================================================================== */
typedef struct {
  double Tc, Tt, Hwv, dr, to_mass, cutoff;   /* required args (fix_phase_change.cpp:58-67) */
  int from_type, to_type;
  int energy_chance;                          /* 1: "ENERGY rate" form (:70-73) */
  double change_chance, rate;                 /* prob, or rate of the ENERGY form */
  double dt;                                  /* update->dt */
  int maxattempt;                             /* option "attempt" (default 10) */
  double sublo[3], subhi[3], boxhi[3];        /* domain->sublo/subhi/boxhi */
  int top[3];                                 /* comm->myloc[d] == comm->procgrid[d]-1 */
} sph_phasechange_params;

/* One pre_exchange on this rank.  Uses the staged atoms (sph_hip_atoms: x, vest, rho, e,
   type; sph_hip_atoms_multiphase: rmass, cv) and the fix's FULL list (sph_hip_list /
   sph_hip_list_csr with SPH_LIST_FULL).  v and cg (atom->v, atom->colorgradient) are nall*3.
   The Park-Miller stream (*seed, RanPark) is consumed in the reference's order, so the
   same seed gives the same insertions.  e[0..nlocal) is updated for atoms that changed
   phase; dmass[0..nall) receives the mass taken from from_type atoms (reverse-communicate
   the ghost part, then call sph_hip_phasechange_finish).  Up to cap new atoms are written
   as 13-double records {x[3], v[3], vest[3], e, rmass, rho, cv}, their parent atom index in
   parent[]; *nins = number inserted (may exceed cap: then call again with more room, the
   seed must be restored by the caller).  The caller creates them (avec->create_atom,
   type to_type) and updates natoms/tags as the reference does (:336-351). */
int sph_hip_phasechange(sph_hip_ctx *ctx, const sph_phasechange_params *p, int *seed,
                        const double *v, const double *cg, double *e, double *dmass, int cap,
                        int *nins, double *new_atoms, int *parent);
/* rmass[i] -= dmass[i]; e[i] *= mold / rmass[i] for i < nlocal (:327-334).  Host only. */
int sph_hip_phasechange_finish(int nlocal, const double *dmass, double *rmass, double *e);

/* ======================================================================================
 * 2. Device-resident engine
 * ==================================================================================== */
#define SPH_MAXTYPES 8

/* Multiphase stack of examples/USER/sph/bubble_growth/bubble.lmp:57-73 (atom_style
   meso/multiphase: per-atom rmass, cv, colorgradient; quintic kernel), run by the engine
   in place of the sph/rhosum, taitwater and heatconduction styles of sph_engine_config.
   Per-pair tables in the (SPH_MAXTYPES+1)^2 layout, upper triangle (i <= j) read and
   mirrored as init_one does.  Sequence per step (hybrid/overlay order): rhosum/multiphase
   and colorgradient over the full list (owned rows; their misnamed pack_comm moves
   nothing, so ghosts keep their comm-time rho and colorgradient), then
   taitwater/multiphase, surfacetension and heatconduction/phasechange over the half list
   with Newton-3 and reverse comm.  fix meso integrates with rmass. */
typedef struct {
  int rhosum_nstep;            /* sph/rhosum/multiphase N (0 = off); cut = h per pair */
  double rhosum_cut[(SPH_MAXTYPES + 1) * (SPH_MAXTYPES + 1)];
  int cg_nstep;                /* sph/colorgradient N (0 = off): alpha, cut per pair */
  double cg_alpha[(SPH_MAXTYPES + 1) * (SPH_MAXTYPES + 1)];
  double cg_cut[(SPH_MAXTYPES + 1) * (SPH_MAXTYPES + 1)];
  int tait_on;                 /* sph/taitwater/multiphase: per type rho0, c, gamma, rbg */
  double rho0[SPH_MAXTYPES + 1], soundspeed[SPH_MAXTYPES + 1], gamma[SPH_MAXTYPES + 1];
  double rbackground[SPH_MAXTYPES + 1];
  double tait_visc[(SPH_MAXTYPES + 1) * (SPH_MAXTYPES + 1)];
  double tait_cut[(SPH_MAXTYPES + 1) * (SPH_MAXTYPES + 1)];
  int st_on;                   /* sph/surfacetension: cut per pair */
  double st_cut[(SPH_MAXTYPES + 1) * (SPH_MAXTYPES + 1)];
  int heat_on;                 /* sph/heatconduction/phasechange: alpha, cut, fixflag, tc */
  double heat_alpha[(SPH_MAXTYPES + 1) * (SPH_MAXTYPES + 1)];
  double heat_cut[(SPH_MAXTYPES + 1) * (SPH_MAXTYPES + 1)];
  double heat_tc[(SPH_MAXTYPES + 1) * (SPH_MAXTYPES + 1)];
  int heat_fixflag[(SPH_MAXTYPES + 1) * (SPH_MAXTYPES + 1)];
} sph_engine_mp_config;

typedef struct {
  int dim;                     /* 2 or 3 */
  int ntypes;                  /* <= SPH_MAXTYPES */
  double boxlo[3], boxhi[3];   /* global box */
  int periodic[3];
  double skin;                 /* neighbor skin */
  int neigh_every;             /* rebuild every N steps (neigh_modify every N delay 0 check no);
                                  sph_engine_neigh_modify replaces it, with delay and check */
  double dt;                   /* timestep (units lj: ftm2v = 1) */
  double ftm2v;                /* force->ftm2v */
  double mass[SPH_MAXTYPES + 1];
  /* integrator: 0 = fix meso for all types, 1 = fix meso/stationary for type 2.. (bc) */
  int stationary_mask;         /* bit t set: type t integrates with meso/stationary */
  /* sph/rhosum: enabled if rhosum_nstep > 0 */
  int rhosum_nstep;
  double rhosum_cut[(SPH_MAXTYPES + 1) * (SPH_MAXTYPES + 1)];
  /* sph/taitwater[/morris]: enabled if tait_on */
  int tait_on;
  int tait_visc;               /* SPH_VISC_* */
  double rho0[SPH_MAXTYPES + 1], soundspeed[SPH_MAXTYPES + 1], B[SPH_MAXTYPES + 1];
  double tait_visc_coef[(SPH_MAXTYPES + 1) * (SPH_MAXTYPES + 1)];
  double tait_cut[(SPH_MAXTYPES + 1) * (SPH_MAXTYPES + 1)];
  /* sph/heatconduction: enabled if heat_on */
  int heat_on;
  double heat_alpha[(SPH_MAXTYPES + 1) * (SPH_MAXTYPES + 1)];
  double heat_cut[(SPH_MAXTYPES + 1) * (SPH_MAXTYPES + 1)];
  /* body force per unit mass (fix gravity style), added in post_force: f += m*g, for the
     types in gravity_mask (bit t set: type t is in the fix's group; 0 = every type).
     Single-phase engines only (the multiphase stack takes no body force from here: use
     sph_engine_forcefix); it acts as a fix defined before every sph_engine_forcefix fix */
  double gravity[3];
  int gravity_mask;
  /* brick decomposition (procgrid[0]*procgrid[1]*procgrid[2] bricks, uniform split; 1 1 1 or
     0 0 0 = one brick).  Bricks are numbered x fastest; each must be wider than the ghost
     cutoff (CommBrick maxneed = 1). */
  int procgrid[3];
  int rank;                    /* my rank in the brick, x fastest */
  /* spatially sort owned particles at every rebuild (atom->sort analogue) */
  int sort;
  /* pair-pass kernels (full lists, gather only, no atomics):
     0 = block-staged (production): blocks of consecutive owned rows stage the union of
         their neighbours in LDS, rows walk 16-bit slot lists built from the bins at every
         rebuild (falls back to 1 for a build whose blocks overflow the LDS image);
     1 = row path: rows gather neighbour records from HBM through a strided global-index
         list (the round-1 production path) */
  int kernel_path;
  /* multiphase stack (NULL: the single-phase styles above); copied at create */
  const sph_engine_mp_config *mp;
} sph_engine_config;

typedef struct {
  int64_t step;
  int nlocal, nghost;
  int64_t nbr_full;            /* entries in the device full list (owned rows) */
  int nbr_builds;
  int nbr_maxrow;              /* longest full-list row of the last CSR build */
  int staged;                  /* 1 if the last build produced block-staged lists */
  int stage_max;               /* block path: largest block union (LDS records) */
  double ms_rhosum, ms_tait, ms_heat, ms_integrate, ms_comm, ms_neigh; /* event-timed */
  int64_t n_rhosum, n_tait, n_heat, n_neigh;  /* launches timed */
  int blk_nbig;                /* block path: blocks of the last build whose union exceeds the
                                  force pass's LDS image (walked by the second launch) */
  int inner_rows;              /* block path: inner rows were built at the last rebuild */
  int inner_live;              /* ... and the last step's passes walked them (no atom had moved
                                  past their margin since they were written) */
  int flags;                   /* SPH_STAT_* bits.  Bit 0: the last rhosum/multiphase was summed
                                  inside the list fill (C5: its time is in ms_neigh, not
                                  ms_rhosum).  Bits 1-5 describe the last block build and are 0
                                  when staged == 0.  Bits 6-9 (SPH_STAT_MP_*) name the gather
                                  family of the last multiphase force pass and where the last
                                  due rhosum was summed */
  int64_t inner_refresh;       /* refresh launches since create (inner rows derived again
                                  between rebuilds when an atom passed their margin) */
} sph_engine_stats;

/* sph_engine_stats.flags */
#define SPH_STAT_RHO_FUSED (1 << 0)    /* rhosum/multiphase summed inside the list fill */
#define SPH_STAT_BLK_R32 (1 << 1)      /* the block build used 32-row blocks (after the 64-row
                                          shape's unions or candidates did not fit) */
#define SPH_STAT_BLK_BIGIMG (1 << 2)   /* ... and the large candidate image (the bitmap build) */
#define SPH_STAT_BLK_NOPRE (1 << 3)    /* the pair passes walk the slot rows chunk by chunk,
                                          without the register preload: the slot-row stride is
                                          past the preload's 256 entries */
#define SPH_STAT_BLK_ROWRETRY (1 << 4) /* the build was repeated with a doubled slot-row stride
                                          after a row outgrew it */
#define SPH_STAT_BLK_IMGRETRY (1 << 5) /* the build was repeated after a block outgrew the small
                                          candidate image */
/* multiphase engines: the gather family the last force pass launched (one of three; none when
   taitwater, surfacetension and heatconduction are all off) ... */
#define SPH_STAT_MP_W4 (1 << 6)        /* k_mp2_gather_w4: symmetric styles, every gamma 1 */
#define SPH_STAT_MP_POW (1 << 7)       /* k_mp2_gather<POW>: symmetric styles, one gamma != 1 */
#define SPH_STAT_MP_ROW (1 << 8)       /* k_mp_gather: unequal gammas, or a type pinned to Tc
                                          against its own type */
/* ... and whether the last rhosum/multiphase that was due was summed inside the list fill
   (bit 0 says so for the current step only; this bit keeps the answer over the steps between
   two due ones, rhosum_nstep > 1) */
#define SPH_STAT_MP_RHO_LISTFILL (1 << 9)
/* the last build's bin copy / the last sort of the owned rows took the counting sort (and not
   the radix sort: SPH_TUNE_CSORT 0, a key space too large for the atoms, or a segment past the
   cap).  In flags on the block path and in multiphase engines; sph_engine_csort_paths gives
   the two bits on every path */
#define SPH_STAT_CSORT_BINS (1 << 10)
#define SPH_STAT_CSORT_ROWS (1 << 11)
/* at least one step of the most recent sph_engine_run had its integrate done by the block
   force pass (SPH_TUNE_FUSEINT) */
#define SPH_STAT_FUSEINT (1 << 12)

typedef struct sph_engine sph_engine;

int sph_engine_create(int device, const sph_engine_config *cfg, sph_engine **out);
int sph_engine_destroy(sph_engine *e);

/* Brick decomposition (cfg.procgrid, cfg.rank; CommBrick's swaps, comm_brick.cpp).  Every
   brick needs a communicator before sph_engine_setup:
   * RCCL, one process per GPU: uid = ncclUniqueId bytes (128) produced by
     sph_engine_comm_uid on rank 0 and distributed by the caller (MPI_Bcast / torch);
   * a local world: several bricks in one process (one host thread per brick, any devices),
     halo exchange by device copies -- for tests and bricks that share a GPU.
   Owned atoms migrate between bricks at rebuilds; sph_engine_get_atoms then returns them in
   local order with their tags (sph_engine_set_tags sets global tags; default = index). */
int sph_engine_comm_uid(void *uid128);
int sph_engine_comm_init(sph_engine *e, const void *uid128, int nranks, int rank);
/* One-brick engine with a communicator attached: on != 0 routes its periodic self swaps
   (borders, forward, rho, reverse) through the communicator -- RCCL send/recv to itself --
   instead of device copies, so the multi-brick data path runs on one GPU.  Before setup. */
int sph_engine_comm_loopback(sph_engine *e, int on);
typedef struct sph_local_world sph_local_world;
int sph_local_world_create(int nranks, sph_local_world **out);
int sph_local_world_destroy(sph_local_world *w);
int sph_engine_comm_local(sph_engine *e, sph_local_world *w, int rank);
/* Node-local world of PROCESSES without RCCL (one process per brick, any devices of the
   node, incl. several processes on one GPU, which RCCL refuses): `name` ("/word", chosen by
   rank 0 and distributed by the caller like the RCCL uid) names a POSIX shared-memory
   control segment; mode 0 moves halos device-to-device through hipIpc-exported outboxes,
   mode 1 stages them through host shared memory.  Same Transport calls, same order, as
   RCCL (comm_brick.cpp:444-506, 696-864, 999-1030).  Collective: every rank calls it. */
int sph_engine_comm_ipc(sph_engine *e, const char *name, int nranks, int rank, int mode);
/* Schedule choices that do not change results (parity-tested both ways), set explicitly
   rather than through the environment; before sph_engine_setup.
   SPH_TUNE_OVERLAP: bricks on the row path overlap interior rows' passes with the halo
   exchange (1) or not (0, default).  SPH_TUNE_BLKUMF: cap the block force pass's LDS image
   at `value` records, blocks with larger unions going to its second launch (0 = auto).
   SPH_TUNE_CSORT: the rebuild orders bins and rows by counting sorts (1, default) or by the
   radix sorts alone (0); 2 = counting, the bin copy as a pass of its own (measurement).
   SPH_TUNE_FUSEINT: the block force pass integrates each row in its epilogue (1, default) on
   the steps that allow it -- one brick, taitwater alone, no post_force fix, fix dt/reset, fix
   phase_change or check yes, not the last step of a run -- or every step launches the
   integrate kernel (0). */
#define SPH_TUNE_OVERLAP 1
#define SPH_TUNE_BLKUMF 2
#define SPH_TUNE_CSORT 3
#define SPH_TUNE_FUSEINT 4
int sph_engine_tune(sph_engine *e, int key, int value);
/* SPH_STAT_CSORT_* of the last build, on every pair path */
int sph_engine_csort_paths(sph_engine *e, int *mask);
int sph_engine_set_tags(sph_engine *e, const int *tags);

/* Owned particles of this rank (tag order is the caller's order; results are returned in
   the same order).  v is the velocity; vest is set from v at setup (FixMeso::setup_pre_force). */
int sph_engine_set_atoms(sph_engine *e, int n, const double *x, const double *v,
                         const int *type, const double *rho, const double *en,
                         const double *cv);
/* Multiphase engines: per-atom rmass and cv (and the initial colorgradient, n*3, may be
   NULL = 0) of the set_atoms atoms, in the same order.  After set_atoms, before setup. */
int sph_engine_set_atoms_multiphase(sph_engine *e, const double *rmass, const double *cv,
                                    const double *cg);
/* fix phase_change on a one-brick multiphase engine (FixPhaseChange::pre_exchange at steps
   1, 1+nevery, ...; the rebuild follows): p's sublo/subhi/boxhi/top are filled by the
   engine, p->dt must be the engine's dt.  Candidates meet the Park-Miller stream (seed) in
   the reference's local atom order, which the engine tracks beside its own row order while
   the fix is armed: read order (ascending tag within the brick), CommBrick::exchange's hole
   fill (comm_brick.cpp:620-632; received atoms appended), Atom::sort at setup and every
   sortfreq steps (sph_engine_atom_sort), created atoms appended.  New atoms get tags n,
   n+1, ... in creation order (atom->tag_extend), type to_type.  Before setup. */
int sph_engine_phase_change(sph_engine *e, const sph_phasechange_params *p, int nevery,
                            int seed);
/* atom_modify sort sortfreq binsize (atom.cpp:540-551; replaces Atom::sortfreq/userbinsize):
   the spatial sort whose order fix phase_change meets its candidates in -- bins of binsize
   (0 = half the neighbor cutoff, Atom::setup_sort_bins) over the brick, at setup and every
   sortfreq steps (0 = never).  Default 1000 / 0, LAMMPS' own.  The engine's rows keep their
   own order; only the tracked LAMMPS order changes. */
int sph_engine_atom_sort(sph_engine *e, int sortfreq, double binsize);

/* neigh_modify every E delay D check yes|no (neighbor.cpp:1332-1347).  Without this call:
   every = cfg.neigh_every, delay 0, check no -- the engine's behaviour so far.
   Neighbor::decide per step, after the initial integrate: a due fix phase_change rebuilds
   first (must_check); otherwise ago (steps since the last build) counts, and a step with
   ago >= D && ago % E == 0 rebuilds -- with check yes only if an owned atom of any brick has
   moved more than skin/2 from where the last build left it (|x - xhold|^2 > 0.25 skin^2,
   strict, fp64).  Only those steps run the checking integrate kernel and read its flag back
   (one stream synchronise each; bricks take the largest flag, so all rebuild together).
   Before sph_engine_setup, like sph_engine_idealgas: the setup takes the first hold positions
   and restarts ago and the counters.
   SPH_HIP_EINVAL: every <= 0, delay < 0, delay > 0 && delay % every != 0 ("Neighbor delay must
   be 0 or multiple of every setting", neighbor.cpp:215), check not 0 or 1, after setup. */
int sph_engine_neigh_modify(sph_engine *e, int every, int delay, int check);

typedef struct {
  int64_t builds;      /* Neighbor::ncalls: builds since sph_engine_setup, setup's included */
  int64_t dangerous;   /* Neighbor::ndanger (neighbor.cpp:1408) */
  int64_t checks;      /* displacement checks evaluated */
  int64_t last_build;  /* step of the last build */
} sph_neigh_stats;
int sph_engine_neigh_stats(sph_engine *e, sph_neigh_stats *out);

/* fix ID group dt/reset N tmin tmax xmax units box (fix_dt_reset.cpp).  At setup (after the
   step-0 forces and the post_force fixes' own setup) and after the final integrate of every
   step with step % nevery == 0, FixDtReset::end_of_step: per owned atom of the group
     dtv = xmax / |v|,  dtf = sqrt(2 xmax / (ftm2v |f| / m)),  dt = MIN(dtv, dtf),
     del = dt v + 0.5 dt^2 f / m ftm2v,  dt *= xmax / |del| if |del| > xmax
   (BIG = 1e20 for an atom at rest without force; every operation rounded on its own, in the
   reference's order), the smallest over atoms and bricks, then MAX with tmin, then MIN with
   tmax.  If that differs from the current dt: Update::update_time, update->dt = dt and
   FixMeso's dtv = dt, dtf = 0.5 dt ftm2v.  v is the velocity after the final integrate, f the
   step's force after every post_force fix: the fix acts as one defined after every
   sph_engine_forcefix and sph_engine_setmeso fix and after cfg.gravity (water_collapse.lmp's
   order: gfix before dtfix).
   The scan runs behind the final integrate in one kernel, a one-block kernel folds its
   per-block minima and keeps dt, {dtv, dtf}, the time and laststep in a device record that
   the integrate kernels of such an engine read; a reset step cannot fuse its final integrate
   with the next initial integrate (three launches where other steps have one).  One brick:
   nothing returns to the host.  Bricks: one stream synchronise per reset step (as
   neigh_modify check yes has per check) -- the brick's minimum is read back and reduced
   over the ranks through the transport.
   Before sph_engine_setup, once.  SPH_HIP_EINVAL: nevery < 1, a negative bound, minbound &&
   maxbound && tmin >= tmax, xmax <= 0 ("Illegal fix dt/reset command", :52-67); after setup;
   a second call; together with sph_engine_phase_change in either order (its ENERGY-rate
   threshold reads update->dt on the host).  Not part of the restart records. */
typedef struct {
  int nevery;            /* >= 1 */
  int minbound; double tmin;   /* minbound 0 = NULL */
  int maxbound; double tmax;   /* maxbound 0 = NULL */
  double xmax;           /* box units (the script's `units box`) */
  int type_mask;         /* the fix's group, as sph_setmeso; 0 = all */
} sph_dtreset;
int sph_engine_dt_reset(sph_engine *e, const sph_dtreset *fix);

/* After setup.  Without the fix: cfg.dt, step * cfg.dt, 0, 0.  With it: one small copy and a
   stream synchronise, as sph_engine_neigh_stats' callers expect of a statistics call. */
typedef struct {
  double dt;             /* update->dt now */
  double time;           /* atime + (step - atimestep) * dt (thermo.cpp:1500) */
  int64_t laststep;      /* f_dtfix: last step at which dt changed (0 if never) */
  int64_t changes;       /* how many end_of_step calls changed dt, setup's included */
} sph_dt_stats;
int sph_engine_dt_stats(sph_engine *e, sph_dt_stats *out);

/* thermo's `press` and fix gravity's scalar (`f_gfix`, so v_etot = c_esph + ke + f_gfix) without
   a sph_engine_get_atoms round trip: the pair virial, the kinetic sums and the gravity energy
   on the device (single-phase engines: sph/taitwater[/morris], + sph/heatconduction, which
   adds no force and so no virial, and sph/idealgas).
   sph_engine_virial_every(e, nevery): the virial is due on the setup step, on every step with
   step % nevery == 0 and on the last step of each sph_engine_run call, as LAMMPS' thermo
   output is; 0 = never (the default).  On a due step the force pass of whichever path runs
   (block, row, generic CSR; the setup step's pass too) is its virial instantiation: each
   owned row i also sums w_i[ab] = sum_j del_a del_b fpair_ij over the neighbours it accepts
   (del = x_i - x_j, fpair as the row's force has it) into a scratch row, and a fixed-shape
   two-stage fold leaves this rank's W = 1/2 sum_i w_i -- every pair once over all bricks,
   the value of the reference's newton-on run (vflag_fdotr: virial_fdotr_compute,
   pair.cpp:1403-1420; sph/idealgas' doubled ev_tally does not reach it).  One exception:
   sph/taitwater/morris' force also has the part vel * fvisc, which is not along del, so the
   reference's x . f carries sum del_a vel_b fvisc besides; the engine tallies the fpair part
   alone (what ev_tally would), and a press formed from it lacks that shear term.  No atomics: two
   runs from one state give the same bits.  A step that is not due launches exactly what an
   engine without this call launches; a due step runs unfused (SPH_TUNE_FUSEINT) and without
   the halo overlap, and the fields after it are bit for bit those of a run that never asked.
   No fix of the package contributes a virial.  Before sph_engine_setup.  SPH_HIP_EINVAL:
   nevery < 0, after setup, a multiphase engine (cfg->mp: those styles' virial is not restated).
   sph_engine_thermo(e, mvv2e, nktv2p, out): after setup, any engine.  The sums run over the
   owned atoms in the state sph_engine_get_atoms would return (v is atom->v, m = mass[type],
   rmass on a multiphase engine).  If virial_step is not the current step, press is NaN; the
   other fields are valid.  Ranks: the caller sums virial, ke_tensor, ke and egrav and forms
   press again, as for sph_engine_reduce.  Not covered: per-atom stress, thermo_modify norm. */
int sph_engine_virial_every(sph_engine *e, int nevery);
typedef struct {
  int64_t virial_step;   /* step whose force pass tallied virial[] (-1: none yet) */
  double virial[6];      /* this rank's share, xx yy zz xy xz yz */
  double ke_tensor[6];   /* sum m v_a v_b * mvv2e over owned atoms (v, not vest) */
  double ke;             /* 0.5 sum m |v|^2 * mvv2e */
  double egrav;          /* this rank's share of f_gfix: -sum m (g . x) over the types of
                            cfg->gravity_mask (fix_gravity.cpp:272-291) */
  double volume;         /* xprd*yprd(*zprd in 3-D) of the global box */
  double press;          /* (sum m v^2 * mvv2e + W_xx + W_yy [+ W_zz]) / (dim * volume) * nktv2p
                            from this rank's sums (compute_pressure.cpp:193-207) */
} sph_thermo_out;
int sph_engine_thermo(sph_engine *e, double mvv2e, double nktv2p, sph_thermo_out *out);

/* Static regions (box units), shared by the clamps and the reductions below.  The
   predicates are LAMMPS' own, closed boundaries included: sphere
   sqrt(dx*dx+dy*dy+dz*dz) <= radius (region_sphere.cpp:96-105), block x >= xlo && x <= xhi
   && ... (region_block.cpp:114-119), match = !(inside ^ interior) (region.cpp:127-131).
   Moving and variable-shape regions cannot be expressed. */
#define SPH_REGION_SPHERE 0
#define SPH_REGION_BLOCK 1
typedef struct {
  int style;                           /* SPH_REGION_* */
  int interior;                        /* 1 = side in (LAMMPS' default), 0 = side out */
  double xc, yc, zc, radius;           /* sphere */
  double xlo, xhi, ylo, yhi, zlo, zhi; /* block */
} sph_region;

/* fix setmeso / fix setmesode, constant style (FixSetMeso::post_force,
   fix_setmeso.cpp:180-233; FixSetMesodE::post_force, fix_setmesode.cpp:171-198): the named
   field of every owned atom of the group (type_mask) that the region selects at its current
   position is overwritten.  Up to SPH_MAX_SETMESO fixes, applied in call order by one
   kernel where LAMMPS runs post_force: at the end of setup and in every step after the
   whole pair compute, before that step's final integrate.  Created and migrated atoms are
   clamped from the step they are owned.  Single-phase and multiphase engines; on a
   single-phase engine SPH_SET_T needs one cv for all atoms (set_atoms' cv, default 1),
   checked at setup.  Before sph_engine_setup.  SPH_HIP_EINVAL: unknown `what` or region
   style, negative radius, after setup, too many fixes, SPH_SET_DE with region_mode 2
   (setmesode has no noregion). */
#define SPH_MAX_SETMESO 8
#define SPH_SET_RHO 0   /* fix setmeso meso_rho : rho = value */
#define SPH_SET_E 1     /* fix setmeso meso_e   : e   = value */
#define SPH_SET_T 2     /* fix setmeso meso_t   : e   = cv * value (sph_t2energy) */
#define SPH_SET_DE 3    /* fix setmesode        : de  = value */
typedef struct {
  int what;            /* SPH_SET_* */
  double value;
  int type_mask;       /* bit t: type t is in the fix's group; 0 = all */
  int region_mode;     /* 0 none, 1 `region` (where match), 2 `noregion` (where !match) */
  sph_region region;
} sph_setmeso;
int sph_engine_setmeso(sph_engine *e, const sph_setmeso *fix);

/* Group reductions on the device (the thermo output of bubble.lmp:77-90 without a
   get_atoms round trip): for each of nsel <= SPH_MAX_REDUCE selections, sum / min / max of
   one per-atom quantity and the atom count over the owned atoms of this rank that the
   group and region select, in the state sph_engine_get_atoms would return; all selections
   in one pass.  An empty selection gives count 0, sum 0, min +inf, max -inf; the average is
   sum / count; combining ranks is the caller's (as the computes' Allreduce).  Fixed-shape
   reduction without atomics: two calls on the same state return identical bits.  After
   setup.  On a single-phase engine SPH_Q_T needs one cv for all atoms. */
#define SPH_MAX_REDUCE 16
#define SPH_Q_ONE 0     /* 1 per atom */
#define SPH_Q_RHO 1
#define SPH_Q_E 2
#define SPH_Q_T 3       /* e / cv */
#define SPH_Q_DE 4
#define SPH_Q_MASS 5    /* rmass, or mass[type] */
#define SPH_Q_KE 6      /* 0.5 m |v|^2 */
#define SPH_Q_VX 7      /* v (not vest): compute reduce ave vx, fix ave/spatial ... vx */
#define SPH_Q_VY 8
#define SPH_Q_VZ 9
typedef struct {
  int quantity;        /* SPH_Q_* */
  int type_mask;
  int region_mode;
  sph_region region;
} sph_reduce_sel;
typedef struct {
  double sum, min, max;
  int64_t count;
} sph_reduce_out;
int sph_engine_reduce(sph_engine *e, int nsel, const sph_reduce_sel *sel, sph_reduce_out *out);

/* fix setforce / fix addforce, constant style (FixSetForce::post_force,
   fix_setforce.cpp:241-251; FixAddForce::post_force, fix_addforce.cpp:238, 269-282) on the
   owned atoms of the group (type_mask) that the region selects at their current position.
   Up to SPH_MAX_FORCEFIX fixes, all applied to each atom in call order by one kernel where
   LAMMPS runs post_force: at the end of setup and in every step after the whole pair compute
   (the engine's gathers leave nothing for a reverse comm to add), before that step's final
   integrate -- the slot of sph_engine_setmeso, whose clamps touch other fields.  Only f's x,
   y, z are written (a single-phase engine's drho is not); an atom no fix selects is not
   stored; with no fix armed nothing is launched.  Created and migrated atoms meet the fixes
   from the step they are owned.
   cfg.gravity (single-phase engines only: the multiphase gathers take no body force) is added
   inside the force pass, so it acts as a fix defined before every force fix: a later
   setforce overwrites it, and a tally sees it.
   per_mass: the added force is m_i * value[d], the product rounded on its own before the
   add -- `variable bodyfx atom mass*${gx}` followed by f += sforce (poiseuille.lmp:57-58).
   The sign change across a plane is two per_mass fixes on the two half-box blocks; regions
   are closed, so an atom exactly on the shared plane gets both, where the reference's one
   expression gives it 0.
   nevery: the fix is applied in the steps with ntimestep % nevery == 0 (setup is step 0).
   tally: the fix keeps foriginal[1..3] of setforce / foriginal[1..3] of addforce -- the
   selected atoms' force just before this fix changed it, summed over this rank by a
   fixed-shape two-stage reduction without atomics (identical runs give identical bits);
   sph_engine_forcefix_total returns the sums of the last post_force that applied the fix
   (combining ranks is the caller's).  Without tally nothing is reduced.  addforce's energy
   foriginal[0] is not kept.
   *id (may be NULL) receives the fix's index, 0, 1, ... in call order.  Before
   sph_engine_setup.  SPH_HIP_EINVAL: after setup, more than SPH_MAX_FORCEFIX fixes, unknown
   kind or region style, negative radius, per_mass or nevery != 1 on SET, ADD with comp_mask
   != 7, nevery < 1; forcefix_total of a fix armed without tally, of an unknown id, or
   before setup. */
#define SPH_MAX_FORCEFIX 8
#define SPH_FF_SET 0   /* fix setforce, constant style */
#define SPH_FF_ADD 1   /* fix addforce, constant style */
typedef struct {
  int kind;            /* SPH_FF_* */
  int comp_mask;       /* bit d set: component d has a value.  SET with a clear bit = NULL
                          (left alone); ADD requires 7 */
  double value[3];
  int per_mass;        /* ADD only: value is per unit mass; added force = m_i * value[d]
                          (m_i = rmass on multiphase engines, mass[type] otherwise) */
  int nevery;          /* ADD only: applied when ntimestep % nevery == 0; >= 1 (SET: 1) */
  int type_mask;       /* the fix's group, as sph_setmeso */
  int region_mode;     /* 0 none, 1 region, 2 noregion (= !match) */
  sph_region region;
  int tally;           /* 1: keep the fix's foriginal force sums of each post_force */
} sph_forcefix;
int sph_engine_forcefix(sph_engine *e, const sph_forcefix *fix, int *id);
int sph_engine_forcefix_total(sph_engine *e, int id, double out[3]);

/* sph/idealgas as the engine's force style (shock_tube/shock2d.lmp: pair_style hybrid/overlay
   sph/rhosum 1 sph/idealgas): it takes the slot of sph/taitwater in the step -- sph/rhosum
   when due, forward comm of rho, the gas pass, post_force (setmeso, forcefix; cfg.gravity
   inside the pass), final integrate -- on both kernel paths, with bricks, sort,
   stationary_mask, rhosum_nstep 0 or N, sph_engine_pair_passes and restarts.  The per-atom
   EOS term 0.4 e / m / rho is recomputed from the current e and rho before every gas pass.
   viscosity and cut are read from the upper triangle (j >= i) and mirrored: the reference
   leaves viscosity[j][i], j > i, unset, and the engine's both-sides gather needs a symmetric
   table.  cut joins the neighbour cutoff (an engine without another style may be created
   with no cut at all; sph_engine_setup then insists on this call).  Before sph_engine_setup.
   SPH_HIP_EINVAL: after setup, a second call, cfg.tait_on, cfg.heat_on or cfg.mp set (one
   force style per engine), a pair of types 1..ntypes with cut <= 0.
   sph_engine_stats ms_tait / n_tait time the gas pass, and sph_engine_set_timing's bit 1
   (taitwater) selects it. */
typedef struct {
  double viscosity[(SPH_MAXTYPES + 1) * (SPH_MAXTYPES + 1)];
  double cut[(SPH_MAXTYPES + 1) * (SPH_MAXTYPES + 1)];
} sph_engine_gas;
int sph_engine_idealgas(sph_engine *e, const sph_engine_gas *gas);

/* Layer profiles (fix ave/spatial ... <axis> origin delta <values>, one dimension, box
   units): per layer, the atom count and the plain sum of each of nq quantities over the
   owned atoms of this rank that the group and region select, in the state
   sph_engine_get_atoms would return.  The layer of an atom (fix_ave_spatial.cpp:1006-1013):
   its coordinate c along `axis`, remapped once if the axis is periodic (c < boxlo: c +=
   prd; c >= boxhi: c -= prd), ibin = (int)((c - lo) * (1.0 / delta)) clamped to [0,
   nlayers - 1] -- atoms outside [lo, lo + nlayers * delta) count in the edge layers.
   count[nlayers]; sum[nq * nlayers], quantity-major (sum[q * nlayers + layer]).  Averaging
   over samples and ranks is the caller's (`norm all` sums and divides).  The selected atoms'
   indices are sorted by layer (stable) and each layer is folded in a fixed shape in index
   order, no atomics: two calls on the same state return identical bits.  After setup.
   SPH_HIP_EINVAL: axis outside 0..2, delta <= 0, nlayers < 1, nq outside [0,
   SPH_MAX_PROFILE_Q] (0: counts only), an unknown quantity or region, before setup. */
#define SPH_MAX_PROFILE_Q 8
typedef struct {
  int axis;            /* 0, 1, 2 */
  double lo, delta;    /* fix ave/spatial's offset[0] and delta[0] */
  int nlayers;
  int type_mask;
  int region_mode;
  sph_region region;
  int nq;
  int quantity[SPH_MAX_PROFILE_Q];   /* SPH_Q_* */
} sph_profile;
int sph_engine_profile(sph_engine *e, const sph_profile *p, int64_t *count, double *sum);

/* Group centre of mass, momentum, bounds, volume and gyration on the device: the diagnostic
   lines of the multiphase examples (bubble.lmp's xcm / vcm / bound(droplet,ymin) /
   `compute dvol droplet reduce sum v_volume` with volume = mass/c_rho / count(droplet);
   `compute rg droplet gyration` of the droplet scripts) without a get_atoms round trip.
   A group is a type mask (0 = all) plus an optional static region tested at the wrapped
   position, as everywhere in the engine; `fix phase_change` gives created atoms the type
   to_type, so a type mask follows `group droplet type d` through the run.
   Both calls work on the owned atoms of this rank in the state sph_engine_get_atoms would
   return, after setup, on single-phase and multiphase engines, both kernel paths, with sort
   and bricks; up to SPH_MAX_MOMENTS selections are evaluated in one pass over the atoms.
   Each rank returns its own partial sums: adding the ranks and dividing by the total mass are
   the caller's (the reference's MPI_Allreduce and the lines after it).
   Arithmetic, every operation rounded on its own in the reference's order (no FMA):
   unwrap[d] = x[d] + xbox[d] * prd[d] with the image counts xbox of the packed imageint
   (Domain::unmap, domain.cpp:1307-1316, orthogonal box); then unwrap[d] * m (Group::xcm,
   group.cpp:1002-1018), v[d] * m (Group::vcm, :1107-1125; v, not vest), m / rho, and for the
   gyration dx = unwrap[0] - cm[0] ..., (dx*dx + dy*dy + dz*dz) * m (Group::gyration,
   :1327-1336), dx*dx * m ... dy*dz * m (compute_gyration.cpp:92-108).  m = rmass on
   multiphase engines, mass[type] otherwise.  lo / hi are the extremes of the stored
   (wrapped) x (Group::bounds, :905-916).
   Fixed-shape two-stage reductions without atomics: two calls on the same state return
   identical bits.  An empty selection gives count 0, sums 0, lo = +inf, hi = -inf (the
   reference's Group::bounds leaves +-BIG = +-1e20 there, a host convention).
   SPH_HIP_EINVAL: a NULL argument with nsel > 0, nsel outside [0, SPH_MAX_MOMENTS], a
   region_mode outside 0..2, an unknown region style, a negative radius, a call before setup.
   nsel == 0 returns SPH_HIP_OK and touches nothing. */
#define SPH_MAX_MOMENTS 8
typedef struct {
  int type_mask;       /* bit t: type t is in the group; 0 = all */
  int region_mode;     /* 0 none, 1 `region` (where match), 2 where !match */
  sph_region region;
} sph_group_sel;
typedef struct {
  int64_t count;       /* atoms selected on this rank */
  double mass;         /* Group::mass: sum m */
  double mx[3];        /* Group::xcm's cmone: sum unwrap(x)[d] * m */
  double mv[3];        /* Group::vcm's p: sum v[d] * m */
  double lo[3], hi[3]; /* Group::bounds: min / max of the wrapped x */
  double volume;       /* sum m / rho (compute reduce sum of mass/c_rho) */
} sph_moments_out;
int sph_engine_moments(sph_engine *e, int nsel, const sph_group_sel *sel, sph_moments_out *out);
/* cm: nsel*3, the caller's (all-rank) centre of mass per selection.
   out: nsel*7 = { sum m*(dx*dx+dy*dy+dz*dz), sum m*dx*dx, dy*dy, dz*dz, dx*dy, dx*dz, dy*dz }
   about it: rg = sqrt(out[0] / masstotal), compute gyration's vector = out[1..6] / masstotal
   (xx yy zz xy xz yz). */
int sph_engine_gyration(sph_engine *e, int nsel, const sph_group_sel *sel, const double *cm,
                        double *out);

/* Multiphase fields of the owned atoms in get_atoms order (any pointer may be NULL):
   rmass, cv, colorgradient (n*3), vest (n*3), type; *ninserted = atoms created so far. */
int sph_engine_get_atoms_multiphase(sph_engine *e, double *rmass, double *cv, double *cg,
                                    double *vest, int *type, int64_t *ninserted);

/* Restart records of the owned atoms (one brick), in get_atoms order, in the reference's
   per-atom restart layout: meso -- AtomVecMeso::pack_restart (atom_vec_meso.cpp:726-757),
   17 doubles {17, x[3], tag, type, mask, image (each an int64 bit pattern, LAMMPS ubuf),
   v[3], rho, e, cv, vest[3]}; multiphase -- AtomVecMesoMultiPhase::pack_restart
   (atom_vec_meso_multiphase.cpp:887-916), 21 doubles {21, x[3], tag, type, mask, image (as
   plain doubles, as that routine writes them), v[3], rho, colorgradient[3], rmass, e, cv,
   vest[3]}.  tag = 1 + the set_atoms index (LAMMPS tags start at 1), mask = 1 (group all),
   image = the packed imageint (lmptype.h, 10 bits per dimension, 512 = zero) counted by
   Domain::pbc.  buf == NULL: only *rec_size (17 or 21) is returned; else cap >= nlocal *
   rec_size doubles. */
int sph_engine_write_restart(sph_engine *e, double *buf, int64_t cap, int *rec_size);
/* Atoms from n restart records of the engine's layout (tags a permutation of 1..n; the
   atom with tag t becomes set_atoms index t-1): x, v, vest, rho, e, cv, type, image (and
   rmass, colorgradient for a multiphase engine).  Replaces set_atoms; before setup (whose
   FixMeso::setup_pre_force sets vest = v again, as a LAMMPS run after read_restart does). */
int sph_engine_read_restart(sph_engine *e, int n, const double *buf);

/* Verlet::setup: forced rebuild + forces at step 0. */
int sph_engine_setup(sph_engine *e);
/* Verlet::run(nsteps). */
int sph_engine_run(sph_engine *e, int nsteps);
/* Copy back owned particles in the set_atoms order (any pointer may be NULL). n is the
   current nlocal (sph_engine_nlocal). */
int sph_engine_nlocal(sph_engine *e);
int sph_engine_get_atoms(sph_engine *e, double *x, double *v, double *rho, double *en,
                         double *f, double *drho, double *de, int *tag);
/* per owned particle (set_atoms order): full-list count within cut+skin at last build */
int sph_engine_neighbor_counts(sph_engine *e, int *numneigh);
int sph_engine_stats_get(sph_engine *e, sph_engine_stats *s);
/* hipEvent timing of the kernel classes (adds an event pair per timed scope): on = 0 off,
   1 every class, (mask << 1) the classes in mask -- bit 0 rhosum, 1 taitwater (or the fused
   multiphase gather, or the sph/idealgas pass of sph_engine_idealgas), 2 heat, 3 integrate, 4 comm, 5 neighbor build / phase change */
int sph_engine_set_timing(sph_engine *e, int on);
/* synchronise the engine's stream */
int sph_engine_sync(sph_engine *e);
/* run only the pair passes (rhosum + forward comm + taitwater [+heat]) n times on the
   current state, no integration or rebuild: the kernel-roofline workload */
int sph_engine_pair_passes(sph_engine *e, int n);
/* run only the neighbour rebuild (pbc, spatial sort, borders, bins, list) n times on the
   current positions: the list-build workload (timed under the neighbour class) */
int sph_engine_rebuild_passes(sph_engine *e, int n);

#ifdef __cplusplus
}
#endif
#endif /* SPH_HIP_H */
