// sph_engine_state.h -- the device-resident engine's state and the plumbing every subsystem
// shares: the study knobs, struct sph_engine (the opaque type of include/sph_hip.h: all of its
// members, and the declaration of every member function under the header that defines it),
// the timing events (get_ev, Scope, harvest), the shorthands on the engine's stream (launch,
// to_host / to_dev / dev_copy, cub), the growth of the atom arrays and the flagged selection.
// Writes: the timing sums and event pool (ms, nlaunch, pending, evpool), the capacities of
// the atom arrays, the scratch tmp, nsel and the pinned h_scalar.
// The sph_engine_*.h headers are the parts of sph_engine.hip's one translation unit: that file
// alone includes them, after its own includes and its `using namespace sph`.
#pragma once

namespace sph {
#ifndef SPH_INNER_FRAC
#define SPH_INNER_FRAC 0.0625
#endif
int g_alloc_log = 0;
static int env_int(const char *name, int dflt) {
  const char *s = getenv(name);
  return s ? atoi(s) : dflt;
}
// Study knobs (tools/kernel_sweep.py, tools/build_sweep.py) exist only in study builds
// (make STUDY=1 -> -DSPH_STUDY); the production library ignores the variables, so no
// environment setting can change its results or run a variant whose outputs are
// meaningless.
#ifdef SPH_STUDY
static int study_int(const char *name, int dflt) { return env_int(name, dflt); }
#else
static int study_int(const char *, int dflt) { return dflt; }
#endif
// SPH_ROW2TILE: shape index of SPH_ROW2_TILES (default 3 = 8 lanes x 4 pairs, the fastest
// with lane-pair gathers on C2 1M: profiles/r01/sweep_row2.log)
int row2_tile() {
  static int t = study_int("SPH_ROW2TILE", 3);
  return t;
}
}  // namespace sph
// SPH_MORTON_DIV (default 4, the fastest of 1/2/4/8 on C2 1M for the row path): cells per
// bin edge of the owned atoms' sort key (Morton for the row path, Hilbert for the block path)
static int morton_div() {
  static int v = std::max(1, study_int("SPH_MORTON_DIV", 4));
  return v;
}
// Row path (kernel_path 1) knobs.  SPH_LP (default 1): lane-pair gathers in the row2
// kernels; SPH_IV (default 1): the strided list is stored chunk-transposed so each lane's
// four indices of a chunk are one 16-B load (sph_row2_kernels.h).
static bool row2_lp() {
  static bool v = study_int("SPH_LP", 1) != 0;
  return v;
}
static bool row2_iv() {
  static bool v = study_int("SPH_IV", 1) != 0;
  return v;
}
// SPH_EXP: study variants of the pair passes (tools/kernel_sweep.py sets it for the timed
// passes only, so it is read per launch); 0 in production
static int row2_exp() { return study_int("SPH_EXP", 0); }
// SPH_TBITS (default 1): with several types, strided list entries carry the neighbour's
// type in their top bits, so the row2 passes skip the per-neighbour type gather
static bool tbits_env() {
  static bool v = study_int("SPH_TBITS", 1) != 0;
  return v;
}
// SPH_BLK (default 0 = 64-row blocks, 8 lanes x 4 slots; the fastest pair passes on C2 1M):
// block shape of the block-staged path (SPH_BLK_SHAPES)
static int blk_shape_env() {
  static int v = study_int("SPH_BLK", 0);
  return v;
}
// SPH_DIRECT (study builds; default 1): bricks forward the per-step halos owner -> ghost in
// one exchange
static bool direct_env() {
  static bool v = study_int("SPH_DIRECT", 1) != 0;
  return v;
}
// SPH_HIL_POW2 (default 1): power-of-two Hilbert cells per axis of the owned sub-box
static bool hil_pow2() {
  static bool v = study_int("SPH_HIL_POW2", 1) != 0;
  return v;
}
// SPH_SORT_EVERY (default 10): steps between spatial sorts of the owned atoms at rebuilds
// (row path and the multiphase stack)
static int sort_every() {
  static int v = study_int("SPH_SORT_EVERY", 10);
  return v;
}

// SPH_MP_TYPED (default 1): the multiphase passes take the neighbour's type from the entry
static bool mp_typed_env() {
  static bool v = study_int("SPH_MP_TYPED", 1) != 0;
  return v;
}
// SPH_INNER_REFRESH (study builds; default 1): derive the inner rows again between rebuilds
// once an atom has moved past their margin (refresh_inner)
static bool refresh_env() {
  static bool v = study_int("SPH_INNER_REFRESH", 1) != 0;
  return v;
}
// SPH_MP_RHOFUSE (default 1): the multiphase engine's list fill sums rhosum/multiphase over
// the hits it finds when the list is built in the step whose forces follow (k_neigh3 RHO)
static bool rhofuse_env() {
  static bool v = study_int("SPH_MP_RHOFUSE", 1) != 0;
  return v;
}

namespace {

constexpr int BLK = 256;
inline unsigned blocks(long n) { return (unsigned)((n + BLK - 1) / BLK); }

enum TimerClass { T_RHO, T_TAIT, T_HEAT, T_INT, T_COMM, T_NEIGH, T_NCLASS };

}  // namespace

struct sph_engine {
  int device = 0;
  hipStream_t s = nullptr;
  sph_engine_config cfg{};
  Coefs hc{};
  Coefs *dc = nullptr;
  Box box{};
  double sublo[3], subhi[3];
  double cutneighmax = 0.0, cutghost = 0.0;
  StepConst sc{};
  int force_mode = 0;  // M_TAIT | M_HEAT, or M_GAS alone (sph_engine_idealgas)
  // the styles' largest cut per type pair ((ntypes+1)^2, upper triangle), kept so that
  // sph_engine_idealgas can add its own before setup (set_cutoffs)
  std::vector<double> cutmax_tab;

  // multiphase stack (cfg.mp, sph_engine_mp.h): per-atom rmass, cv, colorgradient of owned
  // atoms and ghosts, and the ghosts' v (comm vel yes)
  bool mp = false;
  sph_engine_mp_config mpc{};
  MpCoefs hm{};
  MpCoefs *dm = nullptr;
  DBuf<double> rm, cvv, rho_tmp, dmass, xbuf, xbuf2, rhoS, rhoF;
  DBuf<double4> cg, cgS, cgF;
  DBuf<double4> recA, recK, recF, recS;  // k_mp_gather's packed records (k_mp_pack_rec)
  // fix phase_change scratch, kept across calls (no allocation per step)
  DBuf<int> pc_flag, pc_cand, pc_otag, pc_idx, pc_minr, pc_one, pc_grank, pc_key, pc_val, gsrc;
  std::vector<int> gswap_first;  // one brick: first ghost of each swap (+ nghost at the end)
  int gcap_hint = 0;              // one brick: ghost room of the next borders
  DBuf<int> gnall;                // one brick: nall before each swap (+ the overflow word)
  DBuf<int> bcnt;                 // one brick: the swaps' per-block counts (k_brd_*)
  DBuf<double> pc_rec, pc_gat, pc_Wd, pc_vals, pc_nrec, pc_v0, pc_v1;
  DBuf<unsigned long long> pc_k0, pc_k1;  // the donations' (donor, candidate) sort keys
  DBuf<int> pc_cnt;
  int64_t migrations = 0;  // atoms that left this brick at exchanges so far
  // LAMMPS' local order of the owned atoms, tracked while fix phase_change is armed (its
  // candidates meet the random stream in that order): lidx[row] = the atom's index in the
  // reference's arrays -- read order, CommBrick::exchange's hole fill, Atom::sort at setup and
  // every sortfreq steps (atom_modify sort, default 1000 at half the neighbour cutoff)
  DBuf<int> lidx, lidx2, lidx_tab;
  DBuf<unsigned long long> skey, skey2;
  DBuf<int> srow, srow2;
  std::vector<char> h_leave;
  bool lidx_valid = false;
  int sortfreq = 1000;
  double sort_binsize = 0.0;
  int64_t nextsort = 0;
  // fix phase_change (one brick): parameters, stream state, next call, atoms created
  bool pc = false;
  sph_phasechange_params pcp{};
  int pc_nevery = 1, pc_seed = 0;
  int64_t pc_next = 1, pc_inserted = 0;
  int tag_next = 0;  // tag of the next created atom (atom->tag_extend)
  // fix setmeso / setmesode clamps (sph_engine_setmeso), applied in call order by k_setmeso
  // after every pair compute of setup() and run() -- LAMMPS' post_force
  SetMesoArgs sm{};
  bool sm_needs_cv = false;  // a SPH_SET_T clamp is armed
  // sph_engine_reduce: the blocks' partials and the folded results
  DBuf<ReducePart> red_part;
  DBuf<sph_reduce_out> red_out;
  // fix setforce / addforce (sph_engine_forcefix), applied in call order by k_forcefix in
  // the post_force slot; the tallying fixes' foriginal sums of their last post_force
  ForceFixArgs ff{};
  bool ff_tally = false;  // a fix keeps its foriginal sums
  DBuf<double> ff_part, ff_tot;
  // sph_engine_profile: layer keys and rows (sorted twins), the layers' counts and sums
  DBuf<unsigned> pf_key, pf_key2;
  DBuf<int> pf_idx, pf_idx2;
  DBuf<long long> pf_cnt;
  DBuf<double> pf_sum;
  // sph_engine_moments / sph_engine_gyration: the blocks' partials, then the folded results
  DBuf<double> mom_buf;
  // the pair virial (sph_engine_virial_every; single-phase engines): due on the setup step,
  // on steps with step % vir_every == 0 and on the last step of each run().  A due step's
  // force pass stores each owned row's share in vir_w (six doubles per row), virial_fold()
  // leaves this rank's W in vir_tot and names the step in vir_step; sph_engine_thermo's
  // kinetic and gravity sums share vir_part and leave theirs in th_tot
  int vir_every = 0;
  int64_t vir_step = -1;
  DBuf<double> vir_w, vir_part, vir_tot, th_tot;
  bool pc_tags_agreed = false;  // bricks: tag_next agreed over the ranks (first call)
  std::vector<double> cv_by_tag;  // single-phase engines: the constant cv, for restarts

  int nlocal = 0, nghost = 0;
  // brick decomposition (CommBrick): this brick's grid location, face neighbours, swaps
  int pg[3] = {1, 1, 1}, myloc[3] = {0, 0, 0}, procneigh[3][2] = {{0, 0}, {0, 0}, {0, 0}};
  int me = 0, nprocs = 1;
  Transport *tr = nullptr;
  struct Swap {
    int dim = 0, dir = 0, sendproc = 0, recvproc = 0, nsend = 0, nrecv = 0, firstrecv = 0;
    int pbc = 0;
    double lo = 0.0, hi = 0.0, shift = 0.0;
    double lo_sel = 0.0, hi_sel = 0.0;  // (the selection's slab: empty without a send)
    bool remote = false;
    DBuf<int> list;
  };
  Swap swaps[6];
  int nswap = 0;
  DBuf<unsigned char> cbs, cbr, flag2;
  DBuf<int> sel2;
  // loopback: a one-brick run whose periodic self swaps go through the attached
  // communicator (RCCL send/recv to itself) instead of device copies -- the multi-brick
  // data path (slab selection, packing, RCCL groups, unpacking) on one GPU
  bool loopback = false;
  bool multi() const { return pg[0] * pg[1] * pg[2] > 1 || loopback; }
  // halo/compute overlap (multi only): interior and boundary rows of the current list
  hipStream_t s2 = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  DBuf<int> rows_in, rows_bd;
  DBuf<unsigned char> fl_in, fl_bd;
  int n_in = 0, n_bd = 0;
  bool ov_ready = false;  // rows_in / rows_bd describe the current list
  bool overlap = false;   // halo/compute overlap (sph_engine_tune SPH_TUNE_OVERLAP)
  int blkumf = 0;         // force pass LDS image cap in records (SPH_TUNE_BLKUMF; 0 = auto)
  // SPH_TUNE_FUSEINT: the block force pass integrates each row in its epilogue where the step
  // allows it (fuse_step); fuse_flag: SPH_STAT_FUSEINT if a step of the last run() did
  bool fuseint = true;
  int fuse_flag = 0;
  int64_t step = 0;
  int64_t rho_fused_step = -1;  // step whose rhosum/multiphase the list fill summed (k_neigh3 RHO)
  int64_t last_sort = 0;        // step of the last spatial sort of the owned atoms
  bool force_sort = false;  // the next rebuild sorts (sph_engine_rebuild_passes)
  bool setup_done = false;
  bool global_tags = false;
  int last_build = 0;
  // Neighbor::decide (neighbor.cpp:1332-1410): steps since the last build, and neigh_modify's
  // every / delay / check as sph_engine_neigh_modify set them (without the call: every =
  // cfg.neigh_every, delay 0, check no); the builds, dangerous builds and displacement checks
  // since setup.  check yes: the owned positions of the last build (xhold), the word the
  // checking integrate raises and its pinned host copy.
  bool nm_set = false, nm_check = false;
  int nm_every = 1, nm_delay = 0;
  int64_t nm_ago = 0, nm_builds = 0, nm_danger = 0, nm_checks = 0;
  DBuf<double4> xhold;
  DBuf<int> nm_flag;
  int *h_nm = nullptr;
  // fix dt/reset (sph_engine_dt_reset; fix_dt_reset.cpp): the fix as armed, the device record
  // its fold keeps (dt, {dtv, dtf}, time, laststep: sph_engine_kernels.h DtRecord), one
  // partial per block of the scan, and the record's pinned host copy (sph_engine_dt_stats,
  // and the bricks' minimum).  The fix acts as one defined after every forcefix / setmeso fix
  // and after cfg.gravity: it reads the step's force after all of them.
  bool dtr_on = false;
  int dtr_nevery = 1;
  DtFix dtr{};
  DBuf<DtRecord> dt_rec;
  DBuf<double> dt_part;
  DtRecord *h_dt = nullptr;

  // atoms (owned first, then ghosts): layout of sph_kernels.h
  DBuf<double4> xf, vr;
  DBuf<double> en;
  DBuf<int> ty;
  // owned only
  DBuf<double4> vel, fo;
  DBuf<double> de;
  DBuf<int> tag;
  // sort scratch; xf2 / vr2 are also the second xf / vr pair of a fused step (fuse_step): the
  // sort needs them only inside a rebuild, the fused force pass only between two
  DBuf<double4> xf2, vr2, vel2;
  DBuf<double> en2;
  DBuf<int> ty2, tag2;
  // ghosts
  DBuf<int> gowner, gimg;
  DBuf<int> gorank, goidx;  // bricks: each ghost's origin rank and owned index (gimg: image)
  // direct forward comm (build_direct): peers, per-peer record offsets (sends / receives),
  // send lists (owned indices), receiving ghost slots, ghosts imaging own atoms
  bool dr_ok = false;
  std::vector<int> dr_peer;
  std::vector<size_t> dr_soff, dr_roff;
  DBuf<int> dr_sidx, dr_rslot, dr_self, dr_req;
  DBuf<int> dr_byq, dr_byg, dr_hist;  // ghosts grouped by origin rank: owned index, slot
  int dr_nself = 0;
  std::vector<const void *> dr_sb;
  std::vector<void *> dr_rb;
  std::vector<size_t> dr_sbytes, dr_rbytes;
  // borders scratch
  DBuf<unsigned char> flags;
  DBuf<int> sel, nsel;
  // bins
  Bins bn{};
  int nbins = 0;
  QBins qb{};  // the list builders' half-size bins, and the same grid for the binned copy's keys
  Bins qbn{};
  int nqbins = 0;
  DBuf<int> qbeg, tb, xpos;
  DBuf<double4> xb;
  DBuf<unsigned> bkey, bkey2;
  DBuf<int> bidx, bidx2;
  // counting sorts of bin_q (slot 0) and sort_owned (slot 1), cs_count(): the key counts,
  // sort_owned's segment starts, the builds' long-segment words and their pinned host copies
  DBuf<int> cs_cnt, cs_beg, cs_mx;
  int *h_cs = nullptr;
  hipEvent_t cs_ev[2] = {nullptr, nullptr};
  bool cs_pending[2] = {false, false};
  int cs_prev[2] = {-1, -1};  // the last build's longest segment above CS_CAP / 2 (0: none; -1: unknown)
  int csort = 1;              // SPH_TUNE_CSORT: 0 = radix sorts only, 2 = bin copy not fused
  int cs_flags = 0;           // SPH_STAT_CSORT_*: what the last bin copy / row sort took
  // cs_count takes the counting sort up to these key-space sizes (its comment has the rule)
  static constexpr int CS_KFLOOR = 1 << 16, CS_KPERN = 4, CS_KMAX = 1 << 24;
  // neighbor list
  DBuf<int> cnt, off, nbr;
  int64_t nbr_total = 0;   // list entries (-1: strided list, counted on demand)
  int nbr_builds = 0, nbr_maxrow = 0;
  int64_t inner_refreshes = 0;  // refresh_inner launches
  bool strided = false;    // list in fixed-stride rows (row i at i*list_stride, ccnt[i])
  int list_stride = 0;
  int list_perm_g = 0;     // strided rows stored chunk-transposed for G-lane rows (tpos)
  bool list_tbits = false; // strided entries carry the neighbour's type (SPH_TBIT_SHIFT)
  // block-staged path (production, sph_blk_kernels.h): per block of consecutive rows its
  // union of neighbour atoms (ulist, ucnt) and the rows' 16-bit slot rows (snbr)
  bool blk = false;
  int blk_sh = 0, blk_um = 0, blk_umf = 0, blk_sstride = 0, blk_rowcap = 0;
  DBuf<int> ulist, ucnt, kcnt;  // (kcnt: the build's candidates per block, statistics)
  DBuf<unsigned short> snbr;
  // the inner rows' own union (k_blk_build / k_blk_inner): a smaller LDS image for the passes
  DBuf<int> uilist, uicnt;
  bool blk_ksmall = false;  // k_blk_build with the small candidate image (BLK_SCAP_S)
  int blk_kover = 0;        // ... builds it overflowed
  // what the last block build did (sph_engine_stats.flags, SPH_STAT_BLK_*); blk_retry: the
  // repeats of the build_blk call under way (SPH_STAT_BLK_ROWRETRY | SPH_STAT_BLK_IMGRETRY)
  int blk_flags = 0, blk_retry = 0;
  // which gather family the last multiphase force pass launched, and whether the last due
  // rhosum/multiphase came from the list fill (sph_engine_stats.flags, SPH_STAT_MP_*)
  int mp_flags = 0;
  // ... and the inner rows of the build (k_blk_inner: pairs within cut + inner_margin), the
  // owned positions they were written at and the flag that retires them (sc.x0 / sc.moved)
  DBuf<unsigned short> snbi;
  DBuf<int> icnt, moved;
  DBuf<double4> x0;
  double inner_margin = 0.0;
  bool inner = false, inner_written = false;  // (written: by k_blk_build, with the full rows)
  DBuf<int> nbs;  // fixed-stride scratch rows of a CSR build (list_q)
  DBuf<int> mx, ccnt;  // scratch scalars; full-list row counts of the current build
  DBuf<long long> blen;
  // cub scratch
  DBuf<unsigned char> tmp;
  // pinned host scalar
  int *h_scalar = nullptr;
  int *h_small = nullptr;  // pinned: a few device words read back together (borders)

  // timing
  bool timing = false;
  int timing_mask = 0;  // classes timed (bit k = TimerClass k)
  struct EvPair {
    hipEvent_t a, b;
    int cls;
  };
  std::vector<EvPair> pending;
  std::vector<hipEvent_t> evpool;
  double ms[T_NCLASS] = {0, 0, 0, 0, 0, 0};
  int64_t nlaunch[T_NCLASS] = {0, 0, 0, 0, 0, 0};
  // the setup step's force pass (setup_forces_full)
  DBuf<double4> vso, vsg;  // owned vest before setup_pre_force; ghosts' vest as bordered

  // A timed class of the step: a roctx range named after LAMMPS' Timer bucket it stands
  // for (timer.h:19-20: Pair, Neigh, Comm, Modify; seen by rocprofv3 --marker-trace; a few
  // tens of ns without a tool), and where timing asks for it a hipEvent pair
  struct Scope {
    sph_engine *e;
    EvPair p;
    bool on;
    Scope(sph_engine *eng, int cls);
    ~Scope();
  };

  // sph_engine_state.h
  hipEvent_t get_ev();
  void harvest();
  template <class K, class... A>
  void launch(K k, long n, A &&...a);
  template <class T>
  void to_host(T *dst, const T *src, size_t n);
  template <class T>
  void to_dev(T *dst, const T *src, size_t n);
  template <class T>
  void dev_copy(T *dst, const T *src, size_t n);
  template <class Call>
  void cub(Call call);
  void ensure_atoms(size_t nall, bool keep);
  void mpx_copy(int n, const int *src, int first, DBuf<double> &buf);
  bool nt1() const { return cfg.ntypes == 1; }
  int blk_visc() const;
  // the viscosity variant of the row and CSR passes (sph/idealgas has Monaghan's form)
  int row_visc() const { return (force_mode & M_GAS) ? SPH_VISC_MONAGHAN : cfg.tait_visc; }
  // the timer class of the force pass: taitwater's for every style that writes f
  TimerClass force_class() const { return (force_mode & (M_TAIT | M_GAS)) ? T_TAIT : T_HEAT; }
  int read_scalar(const int *dptr);
  template <class F>
  int select_flagged(const F *flag, int n, DBuf<int> &out);

  // sph_engine_comm.h
  void swap_move(bool remote, size_t sbytes, int dest, size_t rbytes, int src);
  template <class Pack, class Unpack>
  void swap_pair(Swap &a, Swap &b, size_t rec, Pack pack, Unpack unpack);
  void borders_multi();
  void build_direct();
  template <class Pack, class Unpack, class Self>
  void forward_direct(size_t rec, Pack pack, Unpack unpack, Self self);
  void mpx_swap_pair(Swap &a, Swap &b);
  template <class Pack, class Unpack>
  void forward_dims(size_t rec, Pack pack, Unpack unpack);
  void forward_multi();
  void reverse1(double *a);
  void forward_rho_multi();
  template <class Pack, class Unpack>
  void reverse_swaps(size_t rec, Pack pack, Unpack unpack);
  void reverse_multi();
  void exchange_multi();
  void borders();
  void forward();
  void forward_fresh();

  // sph_engine_neigh.h
  bool cs_count(int w, int n, long long K0, const Bins &b, int morton, int hdim,
                DBuf<int> &begb);
  void sort_owned();
  void grow_twins();
  bool want_blk() const;
  void set_cutoffs();
  void setup_bins_geometry();
  void bin_q();
  void list_q(bool csr, const double4 *xi = nullptr);
  bool build_blk();
  int build_blk_shape(int shape, bool big);
  int blk_cq() const;
  int choose_umf(int maxu, double meanu) const;
  bool blk_args_pre(const BlkShape &sh) const;
  BlkArgs blk_args() const;
  void build_all(bool need_csr);
  void build_inner();
  int *moved_flag() const;
  void refresh_inner(bool rebuild_next);
  void rebuild();
  int neigh_every() const { return nm_set ? nm_every : (cfg.neigh_every > 0 ? cfg.neigh_every : 1); }
  bool neigh_eligible(int64_t ago) const;
  void neigh_built();
  bool neigh_flag_any();

  // sph_engine_pc.h
  void hole_fill(int n, int nl, int nst);
  void atom_sort();
  void lidx_from_tags();
  void pc_ghost_slots();
  void pc_rank_swap(int ns, int first, int bits);
  void pc_ghost_slots_multi();
  void phase_change();

  // sph_engine_step.h
  bool overlap_on() const;
  void classify_rows();
  void fork();
  void join();
  void pair_compute_overlap();
  void dt_reset_init();
  void dt_end_of_step(bool with_final);
  RowArgs row_args();
  ForceArgs force_args();
  int64_t list_span() const;
  int64_t list_entries();
  Row2Args row2_args();
  bool use_row2() const { return row2_fits((long)nlocal + nghost, (long)list_span()); }
  void pair_compute(bool do_rhosum, bool setup = false, bool fuse = false, bool vir = false);
  bool fuse_step() const;
  void setup_forces_full(double *vw);
  bool force_body() const { return (force_mode & (M_TAIT | M_GAS)) != 0; }
  double *virial_rows();
  void virial_fold();
  static dim3 mp_rows(int rows) { return dim3((unsigned)(((long long)rows * 8 + 255) / 256)); }
  void pair_compute_mp();
  double uniform_cv(const char *who) const;
  void post_force_setmeso();
  StepMass type_mass() const;
  void post_force_forcefix();
  bool rhosum_due() const;
  void setup();
  void launch_integrate(bool first, bool chk);
  void run(int nsteps);
};

inline hipEvent_t sph_engine::get_ev() {
  if (!evpool.empty()) {
    hipEvent_t e = evpool.back();
    evpool.pop_back();
    return e;
  }
  hipEvent_t e;
  SPH_HIP_TRY(hipEventCreate(&e));
  return e;
}
inline sph_engine::Scope::Scope(sph_engine *eng, int cls)
    : e(eng), on(((eng->timing_mask >> cls) & 1) != 0) {
  static const char *const bucket[T_NCLASS] = {"Pair:rhosum", "Pair:taitwater",
                                               "Pair:heatconduction", "Modify:integrate",
                                               "Comm", "Neigh"};
  roctxRangePushA(bucket[cls]);
  if (!on) return;
  p.a = e->get_ev();
  p.b = e->get_ev();
  p.cls = cls;
  SPH_HIP_TRY(hipEventRecord(p.a, e->s));
}
inline sph_engine::Scope::~Scope() {
  roctxRangePop();
  if (!on) return;
  (void)hipEventRecord(p.b, e->s);
  e->pending.push_back(p);
}
inline void sph_engine::harvest() {
  if (pending.empty()) return;
  SPH_HIP_TRY(hipStreamSynchronize(s));
  for (auto &p : pending) {
    float t = 0.f;
    SPH_HIP_TRY(hipEventElapsedTime(&t, p.a, p.b));
    ms[p.cls] += t;
    nlaunch[p.cls] += 1;
    evpool.push_back(p.a);
    evpool.push_back(p.b);
  }
  pending.clear();
}

// Shorthands on the engine's stream.  launch: a 1-D grid of blocks(n) x BLK threads, no
// dynamic LDS (any other geometry or stream spells out hipLaunchKernelGGL); the copies take
// element counts; cub: a hipcub device-wide call over the scratch tmp (with_scratch)
template <class K, class... A>
inline void sph_engine::launch(K k, long n, A &&...a) {
  hipLaunchKernelGGL(k, dim3(blocks(n)), dim3(BLK), 0, s, std::forward<A>(a)...);
}
template <class T>
inline void sph_engine::to_host(T *dst, const T *src, size_t n) {
  SPH_HIP_TRY(hipMemcpyAsync(dst, src, n * sizeof(T), hipMemcpyDeviceToHost, s));
}
template <class T>
inline void sph_engine::to_dev(T *dst, const T *src, size_t n) {
  SPH_HIP_TRY(hipMemcpyAsync(dst, src, n * sizeof(T), hipMemcpyHostToDevice, s));
}
template <class T>
inline void sph_engine::dev_copy(T *dst, const T *src, size_t n) {
  SPH_HIP_TRY(hipMemcpyAsync(dst, src, n * sizeof(T), hipMemcpyDeviceToDevice, s));
}
template <class Call>
inline void sph_engine::cub(Call call) {
  with_scratch(tmp, call);
}

inline void sph_engine::ensure_atoms(size_t nall, bool keep) {
  xf.reserve(nall, keep, s);
  vr.reserve(nall, keep, s);
  en.reserve(nall, keep, s);
  ty.reserve(nall, keep, s);
  if (mp) {
    vel.reserve(nall, keep, s);
    rm.reserve(nall, keep, s);
    cvv.reserve(nall, keep, s);
    cg.reserve(nall, keep, s);
  }
}
// extra multiphase fields: atoms src[0..n) (nullptr: 0..n) -> xbuf -> atoms first..
inline void sph_engine::mpx_copy(int n, const int *src, int first, DBuf<double> &buf) {
  if (!mp || n <= 0) return;
  buf.reserve((size_t)MPX * n, false, s);
  launch(k_mpx_pack, n, n, src, vel.p, rm.p, cvv.p, cg.p, buf.p);
  launch(k_mpx_unpack, n, n, (const int *)nullptr, first, buf.p, vel.p, rm.p, cvv.p, cg.p);
}
// the block force pass's viscosity variant: one type with Monaghan viscosity and viscC = 0
// (nu = 0 or c0 = 0) has no viscosity term at all (BLK_VISC_NONE)
inline int sph_engine::blk_visc() const {
  if (force_mode & M_GAS) return SPH_VISC_MONAGHAN;
  if (nt1() && cfg.tait_visc == SPH_VISC_MONAGHAN && hc.tait[3].viscC == 0.0)
    return BLK_VISC_NONE;
  return cfg.tait_visc;
}

inline int sph_engine::read_scalar(const int *dptr) {
  to_host(h_scalar, dptr, 1);
  SPH_HIP_TRY(hipStreamSynchronize(s));
  return *h_scalar;
}

// ordered indices i in [0, n) with flag[i] != 0 (byte or int flags) -> out (returns the
// count; host sync)
template <class F>
inline int sph_engine::select_flagged(const F *flag, int n, DBuf<int> &out) {
  out.reserve_min1(n);
  nsel.reserve(1);
  if (n == 0) return 0;
  hipcub::CountingInputIterator<int> it(0);
  cub([&](void *t, size_t &tb) {
    return hipcub::DeviceSelect::Flagged(t, tb, it, flag, out.p, nsel.p, n, s);
  });
  return read_scalar(nsel.p);
}
