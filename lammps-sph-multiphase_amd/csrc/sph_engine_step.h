// sph_engine_step.h -- the step (Verlet::setup and Verlet::run, verlet.cpp:88-139, 222-308):
// the pair passes over the current list (block path, row path, generic CSR kernels; the
// multiphase stack; the passes split into interior and boundary rows behind the halos), the
// post_force fixes (setmeso, setforce / addforce), fix dt/reset and the loop that orders them
// with the integrates, the rebuilds and fix phase_change.
// Writes: the forces fo / de (and rho, P in vr through the rhosum passes), the multiphase
// passes' records and partial sums (recA .. recS, rhoS / rhoF, cgS / cgF, rho_tmp), vso / vsg,
// the overlap's row classes (rows_in, rows_bd, n_in, n_bd, ov_ready), ff_part / ff_tot,
// dt_rec / dt_part / h_dt, mp_flags, the nm_* counters, pc_next, step and setup_done.
#pragma once
#include "sph_engine_state.h"

inline bool sph_engine::overlap_on() const {
  return multi() && overlap && (blk || use_row2()) && (force_mode & M_TAIT) != 0 &&
         cfg.rhosum_nstep > 0;
}
// interior rows (no ghost in the list) and boundary rows, each in row order; on the block
// path interior and boundary BLOCKS (no ghost in the union, k_blk_interior)
inline void sph_engine::classify_rows() {
  const int n = nlocal;
  if (!s2) {
    // (a lowest-priority s2 was measured: the interior rows starve, 1.31 -> 2.17 ms per
    // step on the loopback bench)
    SPH_HIP_TRY(hipStreamCreateWithFlags(&s2, hipStreamNonBlocking));
    SPH_HIP_TRY(hipEventCreateWithFlags(&ev_fork, hipEventDisableTiming));
    SPH_HIP_TRY(hipEventCreateWithFlags(&ev_join, hipEventDisableTiming));
  }
  if (blk) {
    const int nb = blk_blocks(n, blk_shape(blk_sh).R);
    fl_in.reserve_min1(nb);
    fl_bd.reserve_min1(nb);
    if (nb)
      hipLaunchKernelGGL(k_blk_interior, dim3(nb), dim3(64), 0, s, nb, ulist.p, ucnt.p,
                         BLK_UCAP, nlocal, fl_in.p, fl_bd.p);
    n_in = select_flagged(fl_in.p, nb, rows_in);
    n_bd = select_flagged(fl_bd.p, nb, rows_bd);
    SPH_REQUIRE(n_in + n_bd == nb, SPH_HIP_ERUNTIME, "block classification lost blocks");
    ov_ready = true;
    return;
  }
  fl_in.reserve_min1(n);
  fl_bd.reserve_min1(n);
  if (n)
    hipLaunchKernelGGL(k_row_ghost_flags, dim3((unsigned)(((long)n * 8 + 255) / 256)),
                       dim3(256), 0, s, n, nlocal, strided ? nullptr : off.p,
                       strided ? list_stride : 0, ccnt.p, nbr.p, list_perm_g,
                       (strided && list_tbits) ? 1 : 0, fl_in.p, fl_bd.p);
  n_in = select_flagged(fl_in.p, n, rows_in);
  n_bd = select_flagged(fl_bd.p, n, rows_bd);
  SPH_REQUIRE(n_in + n_bd == n, SPH_HIP_ERUNTIME, "row classification lost rows");
  ov_ready = true;
}
inline void sph_engine::fork() {  // s2 continues after everything queued on s so far
  SPH_HIP_TRY(hipEventRecord(ev_fork, s));
  SPH_HIP_TRY(hipStreamWaitEvent(s2, ev_fork, 0));
}
inline void sph_engine::join() {  // s continues after everything queued on s2 so far
  SPH_HIP_TRY(hipEventRecord(ev_join, s2));
  SPH_HIP_TRY(hipStreamWaitEvent(s, ev_join, 0));
}

// Forward comm + rhosum + forward rho + taitwater(+heat) of a non-rebuild step with the
// halos overlapped: interior rows read no ghost, so their rhosum runs (on s2) while the
// x/vest/rho/e halo moves, and their force pass while the rho halo moves; boundary rows
// follow each exchange on s.  Same per-row arithmetic as pair_compute (bit-identical).
// The forward pack may read an interior row's rho/EOS term before or after this
// step's rhosum wrote it: ghost rho and P/rho^2 are only read after the rho halo has
// overwritten them, so either value is harmless.
inline void sph_engine::pair_compute_overlap() {
  if (blk) {  // the same on the block path: interior blocks first, on s2
    BlkArgs ka = blk_args(), ki = ka, kb = ka;
    ki.blist = rows_in.p;
    ki.nlist = n_in;
    kb.blist = rows_bd.p;
    kb.nlist = n_bd;
    {
      Scope t(this, T_RHO);  // (this class then includes the forward halo)
      fork();
      blk_rhosum(nt1(), s2, ki, xf.p, ty.p, vr.p, dc);
      forward_multi();
      // (the ghosts' displacement check of forward(): the interior blocks read no ghost,
      // so whether they saw the flag before or after it is harmless)
      if (inner && sc.x0 && nghost)
        launch(k_inner_ghosts, nghost, nghost, nlocal, sc, xf.p);
      blk_rhosum(nt1(), s, kb, xf.p, ty.p, vr.p, dc);
      join();
    }
    {
      Scope t(this, force_class());  // (includes the rho halo)
      fork();
      blk_force(nt1(), blk_visc(), force_mode, s2, ki, row_args());
      forward_rho_multi();
      blk_force(nt1(), blk_visc(), force_mode, s, kb, row_args());
      join();
    }
    return;
  }
  Row2Args b = row2_args(), bi = b, bb = b;
  bi.a.n = n_in;
  bi.rows = rows_in.p;
  bb.a.n = n_bd;
  bb.rows = rows_bd.p;
  {
    Scope t(this, T_RHO);  // (this class then includes the forward halo)
    fork();
    row2_rhosum(nt1(), s2, bi);
    forward_multi();
    row2_rhosum(nt1(), s, bb);
    join();
  }
  {
    Scope t(this, force_class());  // (includes the rho halo)
    fork();
    row2_force(nt1(), row_visc(), force_mode, s2, bi);
    forward_rho_multi();
    row2_force(nt1(), row_visc(), force_mode, s, bb);
    join();
  }
}

// FixDtReset::init at setup: the record starts from cfg.dt at time 0, laststep 0
inline void sph_engine::dt_reset_init() {
  dt_rec.reserve(1);
  DtRecord r{};
  r.dt = r.dtv = cfg.dt;
  r.dtf = sc.dtf;
  r.brick_min = DT_BIG;
  *h_dt = r;
  to_dev(dt_rec.p, h_dt, 1);
  SPH_HIP_TRY(hipStreamSynchronize(s));  // (h_dt is read back into later)
}
// FixDtReset::end_of_step (fix_dt_reset.cpp:131-186) of the current step: the scan over the
// owned atoms -- with_final: behind FixMeso::final_integrate in the same pass -- and the
// one-block fold.  One brick: two launches, nothing returns to the host.  Bricks: the fold
// leaves this brick's minimum in the record; the host reads it back (one stream synchronise
// per reset step, as neigh_flag_any has per check), takes the smallest over the ranks
// (MPI_Allreduce MIN, :168; a rank without atoms takes part with BIG) and launches the
// bounds-and-apply part with it.  The bit pattern of a positive double orders as an
// unsigned 64-bit integer, so it travels as two allgather_int words.
inline void sph_engine::dt_end_of_step(bool with_final) {
  Scope t(this, T_INT);
  const unsigned nb = blocks(nlocal);
  dt_part.reserve_min1(nb);
  const double *m = rm.p;
  if (nb)
    select_bool(with_final, [&](auto f) {
      constexpr bool INT = f;
      hipLaunchKernelGGL(k_dt_scan<INT>, dim3(nb), dim3(BLK), 0, s, nlocal, sc, dtr, dt_rec.p,
                         vr.p, en.p, ty.p, vel.p, fo.p, de.p, m, dt_part.p);
    });
  const bool bricks = multi() && tr;
  select_bool(bricks, [&](auto b) {
    constexpr bool BRICK = b;
    hipLaunchKernelGGL(k_dt_fold<BRICK>, dim3(1), dim3(BLK), 0, s, (int)nb, dt_part.p, dtr,
                       (long long)step, dt_rec.p);
  });
  if (!bricks) return;
  to_host(h_dt, dt_rec.p, 1);
  SPH_HIP_TRY(hipStreamSynchronize(s));
  uint64_t bits;
  std::memcpy(&bits, &h_dt->brick_min, sizeof bits);
  std::vector<int> hi(tr->size()), lo(tr->size());
  tr->allgather_int((int)(uint32_t)(bits >> 32), hi.data(), s);
  tr->allgather_int((int)(uint32_t)(bits & 0xffffffffu), lo.data(), s);
  for (int r = 0; r < tr->size(); r++) {
    const uint64_t b = ((uint64_t)(uint32_t)hi[r] << 32) | (uint64_t)(uint32_t)lo[r];
    bits = std::min(bits, b);
  }
  double dtmin;
  std::memcpy(&dtmin, &bits, sizeof dtmin);
  hipLaunchKernelGGL(k_dt_apply, dim3(1), dim3(64), 0, s, dtmin, dtr, (long long)step,
                     dt_rec.p);
}

inline RowArgs sph_engine::row_args() {
  RowArgs a;
  a.n = nlocal;
  a.off = off.p;
  a.nbr = nbr.p;
  a.xf = xf.p;
  a.vr = vr.p;
  a.ty = ty.p;
  a.en = en.p;
  a.cf = dc;
  a.fo = fo.p;
  a.de = de.p;
  a.gx = cfg.gravity[0];
  a.gy = cfg.gravity[1];
  a.gz = cfg.gravity[2];
  return a;
}
// the generic CSR force kernels' arguments over the same arrays: every owned row of the
// full list, gathered (no ilist, no accumulation into f, no virial)
inline ForceArgs sph_engine::force_args() {
  ForceArgs a{};
  a.inum = nlocal;
  a.nlocal = nlocal;
  a.newton = 1;
  a.ilist = nullptr;
  a.off = off.p;
  a.nbr = nbr.p;
  a.xf = xf.p;
  a.vr = vr.p;
  a.ty = ty.p;
  a.en = en.p;
  a.fo = fo.p;
  a.de = de.p;
  a.accum = 0;
  a.cf = dc;
  a.gx = cfg.gravity[0];
  a.gy = cfg.gravity[1];
  a.gz = cfg.gravity[2];
  a.virial = nullptr;
  return a;
}
// extent of the list array the kernels may address
inline int64_t sph_engine::list_span() const {
  return strided ? (int64_t)nlocal * list_stride : nbr_total;
}
// entries of the current list (sum of row counts for a strided list)
inline int64_t sph_engine::list_entries() {
  if (!strided) return nbr_total;
  if (nlocal == 0) return 0;
  blen.reserve(1);
  cub([&](void *t, size_t &tb) {
    return hipcub::DeviceReduce::Sum(t, tb, ccnt.p, blen.p, nlocal, s);
  });
  long long v = 0;
  to_host(&v, blen.p, 1);
  SPH_HIP_TRY(hipStreamSynchronize(s));
  return v;
}
inline Row2Args sph_engine::row2_args() {
  Row2Args b;
  b.a = row_args();
  b.nall = nlocal + nghost;
  b.ntot = (int)list_span();
  if (strided) {
    b.stride = list_stride;
    b.rcnt = ccnt.p;
  }
  b.lp = row2_lp();
  b.iv = strided && list_perm_g > 0 && list_perm_g == row2_iv_g();
  b.exp = row2_exp();
  b.tbits = strided && list_tbits;
  return b;
}

// rhosum (+ the EOS epilogue) -> forward rho -> taitwater[/morris][+heat] on the current
// list: block path, row path (row2 kernels), or the generic CSR kernels for a list past
// the row2 kernels' 32-bit offsets.  The setup step's force pass walks the half list.
// fuse (fuse_step): the block force pass integrates each row in its epilogue -- the next
// step's x and {vest, rho} go to the second pair, which xf and vr name from here on.
// vir (a due step of sph_engine_virial_every, never fused): the force pass is the VIR
// instantiation of whichever path runs, and virial_fold() follows it.
inline void sph_engine::pair_compute(bool do_rhosum, bool setup, bool fuse, bool vir) {
  SPH_REQUIRE(!vir || (!fuse && !mp), SPH_HIP_ERUNTIME, "a virial step is unfused, single-phase");
  if (mp) {
    pair_compute_mp();
    return;
  }
  const int nall = nlocal + nghost;
  if (do_rhosum) {
    {
      Scope t(this, T_RHO);
      if (blk) {
        blk_rhosum(nt1(), s, blk_args(), xf.p, ty.p, vr.p, dc);
      } else if (use_row2()) {
        row2_rhosum(nt1(), s, row2_args());
      } else {
        RhoArgs ra{nlocal, nullptr, off.p, nbr.p, xf.p, ty.p, vr.p, nullptr, dc};
        launch_rhosum(cfg.dim, true, nt1(), s, ra);
      }
    }
    if (multi()) {
      Scope t(this, T_COMM);
      forward_rho_multi();
    } else if (nghost) {
      Scope t(this, T_COMM);
      launch(k_forward_rho, nghost, nghost, nlocal, gowner.p, xf.p, vr.p);
    }
  } else if (force_mode & M_TAIT) {
    launch(k_eos, nall, nall, xf.p, vr.p, ty.p, dc);
  }
  // sph/idealgas: 0.4 e/m/rho of owned atoms and ghosts from the current e and rho (the
  // ghosts' came with the halos), before EVERY gas pass -- e moves every step, whether or
  // not rhosum was due
  if ((force_mode & M_GAS) && nall)
    launch(k_eos_gas, nall, nall, xf.p, vr.p, en.p, ty.p, dc);
  // the rows' shares of a due step (nullptr: not due, or no style with a force body)
  double *const vw = (vir && force_body()) ? virial_rows() : nullptr;
  if (force_mode && setup) {
    setup_forces_full(vw);
  } else if (force_mode && blk && fuse) {
    Scope t(this, force_class());  // (this class then includes the integrate)
    // the second pair at the first's capacity (the sort's twins: grow_twins keeps them so)
    xf2.reserve_exact(xf.cap);
    vr2.reserve_exact(vr.cap);
    BlkFuse<true> fu;
    fu.sc = sc;
    // step k's epilogue checks the positions of step k + 1: that step's slot of the flag
    fu.sc.moved = sc.x0 ? moved.p + ((step + 1) & 1) : nullptr;
    fu.xn = xf2.p;
    fu.vn = vr2.p;
    fu.vel = vel.p;
    fu.en = en.p;
    blk_force(nt1(), blk_visc(), force_mode, s, blk_args(), row_args(), &fu);
    // Everything downstream sees the new pair.  Its ghost records are stale until the next
    // step's forward comm (k_forward rewrites every ghost's xf, vr and e from its owner) or
    // rebuild (borders() makes the ghosts anew): a fused step runs no post_force fix, no
    // refresh and no end-of-step scan behind the pass, and the next step no integrate, so
    // nothing reads a ghost in between.
    std::swap(xf, xf2);
    std::swap(vr, vr2);
  } else if (force_mode && blk) {
    Scope t(this, force_class());
    blk_force(nt1(), blk_visc(), force_mode, s, blk_args(), row_args(), nullptr, vw);
  } else if (force_mode && use_row2()) {
    Scope t(this, force_class());
    row2_force(nt1(), row_visc(), force_mode, s, row2_args(), vw);
  } else if (force_mode) {
    Scope t(this, force_class());
    ForceArgs a = force_args();
    a.virial = vw;
    launch_force(cfg.dim, nt1(), s, row_visc(), force_mode, a, vw != nullptr);
  } else {
    SPH_HIP_TRY(hipMemsetAsync(fo.p, 0, nlocal * sizeof(double4), s));
    SPH_HIP_TRY(hipMemsetAsync(de.p, 0, nlocal * sizeof(double), s));
  }
  if (vir) virial_fold();
}

// the due step's scratch: six doubles per owned row, which the VIR force pass writes whole
inline double *sph_engine::virial_rows() {
  vir_w.reserve_min1((size_t)VIR_NS * nlocal);
  return vir_w.p;
}
// W = 1/2 sum over the owned rows of their shares (each pair is seen from both of its rows,
// on this brick or another: summed over the bricks every pair counts once), folded in
// k_reduce_part's fixed shape into vir_tot; zeros for an engine whose styles have no force
// body (heat conduction alone) or a brick without atoms
inline void sph_engine::virial_fold() {
  vir_tot.reserve(VIR_NS);
  const int nb = (int)std::min<long>(blocks(nlocal), RED_MAXBLOCKS);
  if (!force_body() || nb == 0) {
    SPH_HIP_TRY(hipMemsetAsync(vir_tot.p, 0, VIR_NS * sizeof(double), s));
  } else {
    vir_part.reserve((size_t)RED_MAXBLOCKS * TH_NS);
    hipLaunchKernelGGL(k_virial_part, dim3(nb), dim3(RED_THREADS), 0, s, nlocal, vir_w.p,
                       vir_part.p);
    hipLaunchKernelGGL(k_slots_final, dim3(1), dim3(64), 0, s, nb, VIR_NS, 0.5, vir_part.p,
                       vir_tot.p);
  }
  vir_step = step;
}

// Force pass of Verlet::setup with the reference's half-list ownership (see
// k_half_from_full): exact even though ghost vest is stale at this point.
// The setup step's force pass (Verlet::setup, verlet.cpp:88-139): borders() ran before
// FixMeso::setup_pre_force, so the reference's half-list pass sees a ghost's vest as it
// was bordered.  Walked as a full-list gather (the global-index CSR rows of the setup
// build) that picks, for each ghost pair, the vest pair the reference's one evaluation
// uses (k_force: vso / vsg) -- no half list, no atomics, no reverse comm.
inline void sph_engine::setup_forces_full(double *vw) {
  const int n = nlocal, nall = nlocal + nghost;
  if (force_mode == 0 || n == 0) return;
  vsg.reserve_min1(nghost);
  if (nghost)
    dev_copy(vsg.p, vr.p + n, (size_t)nghost);
  forward();  // the ghosts' vest as setup_pre_force left their owners' (x, rho, e unchanged)
  fo.reserve(nall, true, s);
  de.reserve(nall, true, s);
  ForceArgs a = force_args();
  a.vso = vso.p;
  a.vsg = vsg.p;
  a.virial = vw;  // (the rows' shares of the setup step's virial, or nullptr)
  launch_force(cfg.dim, nt1(), s, row_visc(), force_mode, a, vw != nullptr);
}

// ---- multiphase stack -------------------------------------------------------------
// hybrid/overlay of bubble.lmp:57-73 in order: rhosum/multiphase and colorgradient over
// the full list (owned rows; no forward comm of either, A.6-1), then taitwater/multiphase,
// surfacetension and heatconduction/phasechange fused in one gather over the full list,
// each pair in its half-list orientation (k_mp_gather: the reference's Newton-3 scatter +
// reverse comm, without atomics or comm)
inline void sph_engine::pair_compute_mp() {
  const int n = nlocal, nall = nlocal + nghost;
  fo.reserve_min1(n, true, s);
  de.reserve_min1(n, true, s);
  if (n == 0) return;
  MpArgs a{};
  a.stride = strided ? list_stride : 0;  // (else CSR: off)
  a.cnt = ccnt.p;
  a.inum = n;
  a.nlocal = n;
  a.newton = 1;
  a.dim = cfg.dim;
  a.ilist = nullptr;  // (rows = owned atoms)
  a.off = off.p;
  a.nbr = nbr.p;
  a.xf = xf.p;
  a.vr = vr.p;
  a.ty = ty.p;
  a.rm = rm.p;
  a.en = en.p;
  a.cv = cvv.p;
  a.mc = dm;
  a.typed = mp_typed_env() ? 1 : 0;  // (k_neigh3 tbits 2 writes the types)
  // the stale version: rho and colorgradient as communicated (k_mp_gather)
  rhoS.reserve(nall);
  cgS.reserve(nall);
  launch(k_mp_snap, nall, nall, vr.p, cg.p, rhoS.p, cgS.p);
  const bool rdue = mpc.rhosum_nstep > 0 && step % mpc.rhosum_nstep == 0;
  const bool cdue = mpc.cg_nstep > 0 && step % mpc.cg_nstep == 0;
  {
    Scope t(this, T_RHO);
    if (rdue) {
      rho_tmp.reserve(nall);
      a.rho = rho_tmp.p;
      if (rho_fused_step != step)  // (else the list fill of this step summed it)
        hipLaunchKernelGGL(k_mp2_rhosum<8>, mp_rows(n), dim3(256), 0, s, a);
      mp_flags = (mp_flags & ~SPH_STAT_MP_RHO_LISTFILL) |
                 (rho_fused_step == step ? SPH_STAT_MP_RHO_LISTFILL : 0);
      launch(k_mp_rho_store, n, n, rho_tmp.p, vr.p);
    }
    if (cdue) {
      a.cg = cg.p;
      recA.reserve(nall);  // (free until the force pass packs its records)
      launch(k_mp_pack_sigma, nall, nall, xf.p, vr.p, rm.p, recA.p);
      a.xs = recA.p;
      hipLaunchKernelGGL(k_mp2_colorgradient<8>, mp_rows(n), dim3(256), 0, s, a);
      a.xs = nullptr;
    }
  }
  // the fresh version: the owned atoms' new values, forwarded to the ghosts
  const double *rF = rhoS.p;
  const double4 *cF = cgS.p;
  if (rdue || cdue) {
    Scope t(this, T_COMM);
    rhoF.reserve(nall);
    cgF.reserve(nall);
    launch(k_mp_snap, n, n, vr.p, cg.p, rhoF.p, cgF.p);
    forward_fresh();
    rF = rhoF.p;
    cF = cgF.p;
  }
  Scope t(this, T_TAIT);
  if (!mpc.tait_on && !mpc.st_on)
    SPH_HIP_TRY(hipMemsetAsync(fo.p, 0, n * sizeof(double4), s));
  if (!mpc.heat_on) SPH_HIP_TRY(hipMemsetAsync(de.p, 0, n * sizeof(double), s));
  MpArgs h = a;
  h.vel = vel.p;
  h.rhoS = rhoS.p;
  h.rhoF = rF;
  h.cgS = cgS.p;
  h.cgF = cF;
  h.fo = fo.p;
  h.de = de.p;
  recA.reserve(nall);
  recK.reserve(nall);
  recF.reserve(nall);
  recS.reserve(nall);
  // symmetric styles (mp2_symmetric): the issue-rate gather of sph_mp2_kernels.h
  const bool sym = mp2_symmetric(hm);
  if (sym)
    launch(k_mp2_pack_rec, nall, nall, cfg.dim, xf.p, vel.p, rm.p, en.p, cvv.p, rF, rhoS.p, cF,
           cgS.p, mpc.heat_on ? 1 : 0, recA.p, recK.p, recF.p, recS.p);
  else
    launch(k_mp_pack_rec, nall, nall, xf.p, vel.p, rm.p, en.p, cvv.p, rF, rhoS.p, cF, cgS.p,
           mpc.heat_on ? 1 : 0, recA.p, recK.p, recF.p, recS.p);
  h.pA = recA.p;
  h.pK = recK.p;
  h.pF = recF.p;
  h.pS = recS.p;
  const int sel = (mpc.tait_on ? 1 : 0) | (mpc.st_on ? 2 : 0) | (mpc.heat_on ? 4 : 0);
  const bool g1 = mp2_gamma1(hm);
  mp_flags = (mp_flags & SPH_STAT_MP_RHO_LISTFILL) |
             (sel == 0 ? 0 : sym && g1 ? SPH_STAT_MP_W4 : sym ? SPH_STAT_MP_POW : SPH_STAT_MP_ROW);
  select_bool(mpc.tait_on, [&](auto ta) {
    constexpr bool T = ta;
    select_bool(mpc.st_on, [&](auto st) {
      constexpr bool S = st;
      select_bool(mpc.heat_on, [&](auto he) {
        constexpr bool H = he;
        if constexpr (T || S || H) {  // (no style enabled: no gather)
          if (sym && g1)
            hipLaunchKernelGGL((k_mp2_gather_w4<8, T, S, H>), mp_rows(n), dim3(256), 0, s, h);
          else if (sym)
            hipLaunchKernelGGL((k_mp2_gather<8, T, S, H, true>), mp_rows(n), dim3(256), 0, s, h);
          else
            hipLaunchKernelGGL((k_mp_gather<8, T, S, H>), mp_rows(n), dim3(256), 0, s, h);
        }
      });
    });
  });
}

// single-phase engines keep no per-atom cv on the device (atom_style meso's cv takes no
// part in its pair styles): meso_t clamps and temperature reductions take the one cv all
// atoms were set with
inline double sph_engine::uniform_cv(const char *who) const {
  double c = cv_by_tag.empty() ? 1.0 : cv_by_tag[0];
  for (double v : cv_by_tag)
    SPH_REQUIRE(v == c, SPH_HIP_EINVAL,
                "%s on a single-phase engine needs one cv for all atoms (got %g and %g); "
                "per-atom cv is the multiphase engine's",
                who, c, v);
  return c;
}

// FixSetMeso / FixSetMesodE post_force of the armed clamps on the owned rows: one launch,
// none without a clamp
inline void sph_engine::post_force_setmeso() {
  if (sm.nfix == 0 || nlocal == 0) return;
  Scope t(this, T_INT);
  const double cvc = (!mp && sm_needs_cv) ? uniform_cv("fix setmeso meso_t") : 1.0;
  launch(k_setmeso, nlocal, nlocal, sm, xf.p, vr.p, en.p, de.p, ty.p,
         mp ? (const double *)cvv.p : nullptr, cvc,
         (!mp && (force_mode & M_TAIT)) ? (const Coefs *)dc : nullptr);
}

// the types' masses as configured (sc.mass is the body-force mass: 0 outside gravity_mask)
inline StepMass sph_engine::type_mass() const {
  StepMass m;
  for (int t = 0; t <= MAXT; t++) m.mass[t] = cfg.mass[t];
  return m;
}

// FixSetForce / FixAddForce post_force of the armed fixes that are due in this step
// (ntimestep % nevery == 0) on the owned rows, after the pair compute has left f whole:
// the tallying fixes' foriginal sums first (k_forcefix_tally reads f as the chain finds
// it), then one launch of k_forcefix; none without a due fix
inline void sph_engine::post_force_forcefix() {
  if (ff.nfix == 0) return;
  ForceFixArgs a = ff;
  a.active = 0;
  bool tally = false;
  for (int k = 0; k < ff.nfix; k++)
    if (step % ff.fix[k].nevery == 0) {
      a.active |= 1 << k;
      tally = tally || ff.fix[k].tally;
    }
  if (a.active == 0) return;
  Scope t(this, T_INT);
  const StepMass tm = type_mass();
  const double *m = mp ? (const double *)rm.p : nullptr;
  if (tally) {
    const int nb = (int)std::min<long>(blocks(nlocal), RED_MAXBLOCKS);
    ff_part.reserve((size_t)RED_MAXBLOCKS * FF_NT);
    if (nb)
      hipLaunchKernelGGL(k_forcefix_tally, dim3(nb), dim3(RED_THREADS), 0, s, nlocal, a, xf.p,
                         ty.p, m, tm, fo.p, ff_part.p);
    hipLaunchKernelGGL(k_forcefix_final, dim3(1), dim3(64), 0, s, nb, a, ff_part.p, ff_tot.p);
  }
  if (nlocal)
    launch(k_forcefix, nlocal, nlocal, a, xf.p, ty.p, m, tm, fo.p);
}

inline bool sph_engine::rhosum_due() const {
  return cfg.rhosum_nstep > 0 && (step % cfg.rhosum_nstep) == 0;
}

// Verlet::setup (verlet.cpp:88-139)
inline void sph_engine::setup() {
  step = 0;
  vir_step = -1;  // (step starts over: no earlier virial may pass for this run's)
  Scope t(this, T_NEIGH);
  if (pc) {  // (every setup sorts: verlet.cpp:106)
    if (!lidx_valid) lidx_from_tags();
    nextsort = 0;
  }
  // borders() runs before setup_pre_force: ghosts carry vest as it was (reference order);
  // the setup force pass needs the global-index list for its half-list walk
  build_all(true);
  vso.reserve_min1(nlocal);  // (vest before setup_pre_force: setup_forces_full)
  if (nlocal)
    dev_copy(vso.p, vr.p, (size_t)nlocal);
  launch(k_vest_from_v, nlocal, nlocal, cfg.stationary_mask, ty.p, vel.p, vr.p);
  pair_compute(rhosum_due(), /*setup=*/true, false, vir_every > 0);
  post_force_setmeso();  // (FixSetMeso::setup calls post_force)
  if (ff_tally) {
    ff_tot.reserve(FF_NT);
    SPH_HIP_TRY(hipMemsetAsync(ff_tot.p, 0, FF_NT * sizeof(double), s));
  }
  post_force_forcefix();  // (FixSetForce::setup / FixAddForce::setup too)
  nm_builds = nm_danger = nm_checks = 0;
  neigh_built();  // (Neighbor::ncalls counts the setup's build)
  if (dtr_on) {  // FixDtReset::setup = end_of_step, after every post_force fix's own setup
    dt_reset_init();
    dt_end_of_step(false);
  }
  setup_done = true;
}

// The step's integrate launch: the initial integrate alone when `first` (the final integrate
// before it has run: the first step of a run, with fix dt/reset also the step after a reset
// step), else fused behind the previous step's final one.  CHK: an eligible step of a check-yes
// engine; DTR: an engine with fix dt/reset takes {dtv, dtf} from the device record.
inline void sph_engine::launch_integrate(bool first, bool chk) {
  Scope t(this, T_INT);
  select_bool(chk, [&](auto c) {
    constexpr bool CHK = c;
    select_bool(dtr_on, [&](auto d) {
      constexpr bool DTR = d;
      StepOpt<CHK, DTR> o{};
      if constexpr (CHK) {
        o.xhold = xhold.p;
        o.trig2 = 0.25 * cfg.skin * cfg.skin;
        o.flag = nm_flag.p;
      }
      if constexpr (DTR) o.rec = &dt_rec.p->dtv;
      if (first)
        launch((k_initial_integrate<CHK, DTR>), nlocal, nlocal, sc, xf.p, vr.p, en.p, ty.p, vel.p,
               fo.p, de.p, rm.p, o);
      else
        launch((k_final_initial<CHK, DTR>), nlocal, nlocal, sc, xf.p, vr.p, en.p, ty.p, vel.p,
               fo.p, de.p, rm.p, o);
    });
  });
}

// Whether a step's force pass may integrate its rows itself (blk_force_body FUSE; the caller
// excludes the last step of a run(), whose force and de the caller reads): one brick on the
// block path with taitwater alone -- the heat and gas modes stage e, which the epilogue writes
// -- and nothing that reads or changes f, de, x or dt between the force pass and the next
// step's integrate: no post_force fix (setmeso, setforce / addforce), no fix dt/reset, no fix
// phase_change, no displacement check (check yes: the integrate raises the flag the host reads
// before it decides on the rebuild).  Asked after the step's rebuild, which decides blk.
inline bool sph_engine::fuse_step() const {
  return fuseint && blk && !multi() && !mp && force_mode == M_TAIT && !pc && !nm_check &&
         !dtr_on && sm.nfix == 0 && ff.nfix == 0 && row2_exp() == 0;
}

// Verlet::run (verlet.cpp:222-308)
inline void sph_engine::run(int nsteps) {
  // the final_integrate of step k-1 runs fused with the initial_integrate of step k;
  // the last step's final_integrate runs on its own after the loop
  bool final_done = false;  // (fix dt/reset: the step's final integrate has run already)
  bool fused = false;       // the previous step's force pass integrated its rows (fuse_step)
  fuse_flag = 0;
  for (int k = 0; k < nsteps; k++) {
    step++;
    if (sc.x0) sc.moved = moved_flag();
    // Neighbor::decide (neighbor.cpp:1332-1410).  A due fix phase_change is must_check: it
    // builds before ago counts.  Otherwise ago counts, and the step is eligible once
    // ago >= delay && ago % every == 0 -- known before the integrate is launched, so only
    // an eligible step of a check-yes engine runs the checking instantiation.  (The box
    // never changes in the engine: the reference's boxcheck branch does not apply.)
    const bool pc_due = pc && step == pc_next;  // (the fix forces this reneighbor)
    const bool elig = !pc_due && neigh_eligible(nm_ago + 1);
    const bool chk = elig && nm_check;
    // (a fused step has integrated already, into the pair xf and vr now name)
    if (!fused) launch_integrate(dtr_on ? (k == 0 || final_done) : k == 0, chk);
    bool build = pc_due;
    if (!pc_due) {
      nm_ago++;
      if (chk) {
        nm_checks++;
        build = neigh_flag_any();
        // (a check that fires at its first opportunity, neighbor.cpp:1408)
        if (build && nm_ago == std::max(neigh_every(), nm_delay)) nm_danger++;
      } else {
        build = elig;
      }
    }
    if (pc_due) {
      phase_change();
      pc_next += pc_nevery;
    }
    // (check yes: whether the next step rebuilds is not known yet -- a refresh that a
    // rebuild then supersedes is harmless, the rebuild clears both slots)
    auto refresh = [&] {
      refresh_inner(nm_check ? (pc && step + 1 == pc_next) : (!pc && neigh_eligible(nm_ago + 1)));
    };
    if (build) {
      rebuild();
      neigh_built();
    }
    // the virial is due as thermo output is (every vir_every steps and on a run's last step);
    // a due step runs unfused and without the halo overlap, whose per-row arithmetic is the
    // same, so the fields do not depend on vir_every
    const bool vdue = vir_every > 0 && (step % vir_every == 0 || k + 1 == nsteps);
    fused = k + 1 < nsteps && fuse_step() && !vdue;
    if (!build && !fused && !vdue && ov_ready && rhosum_due() && overlap_on()) {
      pair_compute_overlap();
    } else {
      if (!build) forward();
      // A fused step refreshes the inner rows BEFORE its passes: the epilogue raises the next
      // step's slot of the moved flag against x0, so that slot's clear and a due x0 := x of
      // this step come first, as the unfused order has them (refresh, then the next step's
      // integrate); and the refresh reads this step's positions, which xf no longer names
      // behind the pass.  This step's positions are final from the forward comm on, and its
      // passes read this step's slot, which the refresh leaves as it is: they walk the rows
      // they would have walked.
      if (fused) refresh();
      pair_compute(rhosum_due(), false, fused, vdue);
    }
    if (fused) fuse_flag = SPH_STAT_FUSEINT;
    post_force_setmeso();
    post_force_forcefix();
    if (!fused) refresh();
    if (timing && pending.size() > 4096) harvest();
    // fix dt/reset: Modify::end_of_step follows the final integrate of a step with
    // ntimestep % nevery == 0 (modify.cpp:404-408, verlet.cpp:299), and the next initial
    // integrate needs the dt it leaves: the final integrate runs here with the scan behind
    // it, then the fold, and the next step (or the next run) integrates on its own -- three
    // launches where the other steps have the fused one
    final_done = dtr_on && step % dtr_nevery == 0;
    if (final_done) dt_end_of_step(true);
  }
  if (nsteps > 0 && !final_done) {
    Scope t(this, T_INT);
    if (dtr_on)
      launch(k_final_integrate_dt, nlocal, nlocal, sc, vr.p, en.p, ty.p, vel.p, fo.p, de.p, rm.p,
             DtFrom<true>{&dt_rec.p->dtv});
    else
      launch(k_final_integrate, nlocal, nlocal, sc, vr.p, en.p, ty.p, vel.p, fo.p, de.p, rm.p);
  }
  SPH_HIP_TRY(hipGetLastError());
}
