// sph_engine_comm.h -- the engine's communication, CommBrick's (comm_brick.cpp) on the device:
// bricks of a procgrid (and the loopback brick) exchange, border, forward and reverse through
// the swaps of the Transport, a periodic self swap by device copies; the per-step halos also
// go owner -> ghost in one exchange (build_direct / forward_direct); one brick alone images
// its own atoms by kernels (borders, forward, forward_fresh).
// Writes: nghost, the ghosts' part of the atom arrays and their origins (gowner, gimg, gorank,
// goidx, gsrc, gswap_first, gnall, gcap_hint), swaps[] / nswap, the dr_* tables of the direct
// forward, the buffers cbs / cbr and the selection scratch; exchange_multi also nlocal, the
// owned arrays, lidx and migrations.
#pragma once
#include "sph_engine_state.h"

// CommBrick::setup slabs (comm_brick.cpp:330-380) + borders (:696-864) on one process

// move the packed send buffer (cbs, sbytes) of swap-like traffic to cbr (rbytes)
inline void sph_engine::swap_move(bool remote, size_t sbytes, int dest, size_t rbytes, int src) {
  if (remote) {
    tr->exchange(cbs.p, sbytes, dest, cbr.p, rbytes, src, s);
  } else if (rbytes) {
    dev_copy(cbr.p, cbs.p, rbytes);
  }
}

// A dimension's two swaps as ONE move of rec-byte records.  Both send from the same atoms
// (owned + earlier dimensions' ghosts, see borders_multi) and receive into disjoint ghost
// ranges: pack(sw, buf) fills each swap's part of one send buffer (b's part 256-byte
// aligned behind a's), one exchange carries both (one RCCL group over xGMI per dimension
// instead of one per swap) and unpack(sw, buf) reads each received part.  pack and unpack
// are called only for a swap that sends / receives.
template <class Pack, class Unpack>
inline void sph_engine::swap_pair(Swap &a, Swap &b, size_t rec, Pack pack, Unpack unpack) {
  const size_t sa = (size_t)a.nsend * rec, sb = (size_t)b.nsend * rec;
  const size_t ra = (size_t)a.nrecv * rec, rb = (size_t)b.nrecv * rec;
  const size_t so = (sa + 255) & ~(size_t)255, ro = (ra + 255) & ~(size_t)255;
  cbs.reserve(std::max<size_t>(so + sb, 1), true, s);
  cbr.reserve(std::max<size_t>(ro + rb, 1), true, s);
  if (a.nsend) pack(a, cbs.p);
  if (b.nsend) pack(b, cbs.p + so);
  if (a.remote) {
    tr->exchange2(cbs.p, sa, a.sendproc, cbr.p, ra, a.recvproc, cbs.p + so, sb, b.sendproc,
                  cbr.p + ro, rb, b.recvproc, s);
  } else {  // this brick is its own neighbour along this dimension (periodic self swap)
    if (ra) dev_copy(cbr.p, cbs.p, ra);
    if (rb) dev_copy(cbr.p + ro, cbs.p + so, rb);
  }
  if (a.nrecv) unpack(a, cbr.p);
  if (b.nrecv) unpack(b, cbr.p + ro);
}

// CommBrick::borders over a procgrid (comm_brick.cpp:690-880, maxneed = 1).  Both swaps
// of a dimension select from the same atoms (owned + earlier dimensions' ghosts), so
// their counts travel in one exchange and their records in another; the ghosts of the
// lower swap are appended before those of the upper one, as in CommBrick.
inline void sph_engine::borders_multi() {
  nghost = 0;
  int nall = nlocal;
  nswap = 0;
  for (int d = 0; d < cfg.dim; d++) {
    const int nlast = nall;
    Swap *pair[2] = {&swaps[nswap], &swaps[nswap + 1]};
    nswap += 2;
    for (int dir = 0; dir < 2; dir++) {
      Swap &sw = *pair[dir];
      sw.dim = d;
      sw.dir = dir;
      sw.sendproc = procneigh[d][dir];
      sw.recvproc = procneigh[d][1 - dir];
      sw.remote = pg[d] > 1 || loopback;
      bool sendflag = true;  // sendneed/recvneed across a non-periodic boundary (:226-274)
      if (!box.periodic[d]) sendflag = dir == 0 ? myloc[d] > 0 : myloc[d] < pg[d] - 1;
      sw.lo = dir == 0 ? -1.0e20 : subhi[d] - cutghost;
      sw.hi = dir == 0 ? sublo[d] + cutghost : 1.0e20;
      int pbc = 0;
      if (dir == 0 && myloc[d] == 0) pbc = 1;
      if (dir == 1 && myloc[d] == pg[d] - 1) pbc = -1;
      sw.shift = pbc * box.prd[d];
      sw.pbc = pbc;
      // the selection's count stays on the device (nsel[dir]); both swaps' counts and the
      // peers' are read back together below: one host sync per dimension
      nsel.reserve(2);
      sw.list.reserve_min1(nlast);
      sw.lo_sel = sendflag ? sw.lo : 1.0;  // (no send: an empty slab)
      sw.hi_sel = sendflag ? sw.hi : 0.0;
    }
    Swap &a = *pair[0], &b = *pair[1];
    {  // both swaps' selections in three launches
      const int nb = (nlast + BRD_CH - 1) / BRD_CH;
      if (nb == 0) {
        SPH_HIP_TRY(hipMemsetAsync(nsel.p, 0, 2 * sizeof(int), s));
      } else {
        bcnt.reserve(2 * (size_t)nb);
        hipLaunchKernelGGL(k_brd_count, dim3(nb), dim3(BRD_T), 0, s, (const int *)nullptr, d,
                           a.lo_sel, a.hi_sel, b.lo_sel, b.hi_sel, xf.p, bcnt.p, nlast);
        hipLaunchKernelGGL(k_brd_scan, dim3(1), dim3(1024), 0, s, nb, bcnt.p, (int *)nullptr,
                           0, (int *)nullptr, nsel.p);
        hipLaunchKernelGGL(k_brd_lists, dim3(nb), dim3(BRD_T), 0, s, nlast, bcnt.p, d,
                           a.lo_sel, a.hi_sel, b.lo_sel, b.hi_sel, xf.p, a.list.p, b.list.p);
      }
    }
    if (a.remote) {
      int h[4];
      tr->exchange_count2_dev(nsel.p, a.sendproc, a.recvproc, b.sendproc, b.recvproc, s, h);
      a.nsend = h[0];
      b.nsend = h[1];
      a.nrecv = h[2];
      b.nrecv = h[3];
    } else {
      int *const h = h_small;  // (pinned)
      to_host(h, nsel.p, 2);
      SPH_HIP_TRY(hipStreamSynchronize(s));
      a.nsend = a.nrecv = h[0];
      b.nsend = b.nrecv = h[1];
    }
    a.firstrecv = nall;
    b.firstrecv = nall + a.nrecv;
    const int nr = a.nrecv + b.nrecv;
    if (nr) {
      ensure_atoms((size_t)nall + nr, true);
      const size_t ngn = (size_t)nall + nr - nlocal;
      gorank.reserve(ngn, true, s);
      goidx.reserve(ngn, true, s);
      gimg.reserve(ngn, true, s);
    }
    swap_pair(
        a, b, sizeof(BorderRec),
        [&](Swap &sw, unsigned char *buf) {
          launch(k_pack_border, sw.nsend, sw.nsend, sw.list.p, d, sw.shift, sw.pbc, tr->rank(),
                 nlocal, xf.p, vr.p, en.p, ty.p, gorank.p, goidx.p, gimg.p, (BorderRec *)buf);
        },
        [&](Swap &sw, unsigned char *buf) {
          launch(k_unpack_border, sw.nrecv, sw.nrecv, sw.firstrecv, nlocal,
                 (const BorderRec *)buf, xf.p, vr.p, en.p, ty.p, gorank.p, goidx.p, gimg.p);
        });
    if (mp) mpx_swap_pair(a, b);
    nall += nr;
  }
  nghost = nall - nlocal;
  build_direct();
}

// Direct forward comm: the per-step halo goes straight from each ghost's owner (its
// origin, carried through the border records) in ONE exchange, instead of one exchange
// per dimension with earlier dimensions' ghosts forwarded again (CommBrick's
// dimension-ordered swaps, comm_brick.cpp:475-530).  Built at every borders: the ghosts
// are grouped by origin rank (ghost order kept), every rank sends its peers the owned
// indices it needs from them (counts first), and what it receives becomes its send lists.
// Ghosts imaging this rank's own atoms are device copies (through the communicator in
// loopback mode).  The swaps stay for the reverse comm of the setup step and of fix
// phase_change.  SPH_DIRECT=0 keeps the dimension-ordered forward.
inline void sph_engine::build_direct() {
  dr_ok = false;
  if (!direct_env() || mp || !tr) return;
  const int P = tr->size(), me = tr->rank(), ng = nghost;
  // the ghosts grouped by origin rank on the device (a stable radix sort of (rank, ghost)
  // keeps the ghost order within a rank), the per-rank counts the only read-back
  std::vector<int> beg(P + 2, 0);
  dr_byq.reserve_min1(ng);
  dr_byg.reserve_min1(ng);
  dr_hist.reserve(P + 2);
  if (ng) {
    bkey.reserve(ng);
    bkey2.reserve(ng);
    bidx.reserve(ng);
    bidx2.reserve(ng);
    launch(k_dr_keys, ng, ng, P, gorank.p, bkey.p, bidx.p);
    int eb = 1;
    while ((1 << eb) <= P) eb++;
    cub([&](void *t, size_t &tb) {
      return hipcub::DeviceRadixSort::SortPairs(t, tb, bkey.p, bkey2.p, bidx.p, bidx2.p, ng, 0,
                                                eb, s);
    });
    launch(k_dr_group, ng, ng, bidx2.p, goidx.p, dr_byq.p, dr_byg.p);
    // beg[r]: the first ghost of rank r (r = 0 .. P + 1; ranks out of range sort as P)
    hipLaunchKernelGGL(k_lower_bound, dim3(1), dim3(64 * ((P + 2 + 63) / 64)), 0, s, P + 1,
                       ng, 0, bkey2.p, dr_hist.p);
    to_host(beg.data(), dr_hist.p, P + 2);
    SPH_HIP_TRY(hipStreamSynchronize(s));
  }
  SPH_REQUIRE(beg[P + 1] == beg[P], SPH_HIP_ERUNTIME,
              "%d ghosts with an origin rank outside [0,%d)", beg[P + 1] - beg[P], P);
  std::vector<int> scnt(P, 0), rcnt(P, 0);
  for (int r = 0; r < P; r++)
    if (r != me) scnt[r] = beg[r + 1] - beg[r];
  tr->exchange_counts_all(scnt.data(), rcnt.data(), s);  // rcnt[r]: what r needs from me
  dr_peer.clear();
  dr_soff.assign(1, 0);
  dr_roff.assign(1, 0);
  for (int r = 0; r < P; r++) {
    if (r == me && !loopback) continue;
    const size_t nin = beg[r + 1] - beg[r], nout = (r == me) ? nin : (size_t)rcnt[r];
    if (nin == 0 && nout == 0) continue;
    dr_peer.push_back(r);
    dr_roff.push_back(dr_roff.back() + nin);
    dr_soff.push_back(dr_soff.back() + nout);
  }
  const int np = (int)dr_peer.size();
  const size_t S = dr_soff.back(), R = dr_roff.back();
  // the peers' groups are the rank-ordered groups without this rank's own (unless the
  // loopback sends those through the communicator): two device copies
  DBuf<int> &req = dr_req;  // (persistent: no hipMalloc / synchronising hipFree per rebuild)
  req.reserve_min1(R);
  dr_sidx.reserve_min1(S);
  dr_rslot.reserve_min1(R);
  {
    const size_t a = loopback ? (size_t)ng : (size_t)beg[me];
    const size_t b0 = loopback ? (size_t)ng : (size_t)beg[me + 1];
    SPH_REQUIRE(a + (ng - b0) == R, SPH_HIP_ERUNTIME, "direct forward: %zu != %zu", a + (ng - b0), R);
    if (a) {
      dev_copy(req.p, dr_byq.p, a);
      dev_copy(dr_rslot.p, dr_byg.p, a);
    }
    if (ng > (int)b0) {
      dev_copy(req.p + a, dr_byq.p + b0, ng - b0);
      dev_copy(dr_rslot.p + a, dr_byg.p + b0, ng - b0);
    }
  }
  dr_sb.resize(np);
  dr_rb.resize(np);
  dr_sbytes.resize(np);
  dr_rbytes.resize(np);
  for (int k = 0; k < np; k++) {  // requests out, the peers' requests in (= my send lists)
    dr_sb[k] = req.p + dr_roff[k];
    dr_sbytes[k] = (dr_roff[k + 1] - dr_roff[k]) * sizeof(int);
    dr_rb[k] = dr_sidx.p + dr_soff[k];
    dr_rbytes[k] = (dr_soff[k + 1] - dr_soff[k]) * sizeof(int);
  }
  tr->exchange_multi(np, dr_peer.data(), dr_sb.data(), dr_sbytes.data(), dr_rb.data(),
                     dr_rbytes.data(), s);
  dr_nself = loopback ? 0 : beg[me + 1] - beg[me];
  dr_self.reserve_min1(dr_nself);
  if (dr_nself)
    dev_copy(dr_self.p, dr_byg.p + beg[me], dr_nself);
  dr_ok = true;
}
// one direct forward of rec-byte records: pack the send lists, one exchange, unpack
template <class Pack, class Unpack, class Self>
inline void sph_engine::forward_direct(size_t rec, Pack pack, Unpack unpack, Self self) {
  const int np = (int)dr_peer.size();
  const size_t S = dr_soff.back(), R = dr_roff.back();
  cbs.reserve(std::max<size_t>(S * rec, 1));
  cbr.reserve(std::max<size_t>(R * rec, 1));
  if (S) pack((int)S, cbs.p);
  for (int k = 0; k < np; k++) {
    dr_sb[k] = cbs.p + dr_soff[k] * rec;
    dr_sbytes[k] = (dr_soff[k + 1] - dr_soff[k]) * rec;
    dr_rb[k] = cbr.p + dr_roff[k] * rec;
    dr_rbytes[k] = (dr_roff[k + 1] - dr_roff[k]) * rec;
  }
  tr->exchange_multi(np, dr_peer.data(), dr_sb.data(), dr_sbytes.data(), dr_rb.data(),
                     dr_rbytes.data(), s);
  if (R) unpack((int)R, cbr.p);
  if (dr_nself) self();
}

// the extra multiphase fields of a dimension's two swaps (pack_border_vel / pack_comm_vel
// of atom_vec_meso_multiphase.cpp): lists -> the peers -> firstrecv..
inline void sph_engine::mpx_swap_pair(Swap &a, Swap &b) {
  swap_pair(
      a, b, MPX * sizeof(double),
      [&](Swap &sw, unsigned char *buf) {
        launch(k_mpx_pack, sw.nsend, sw.nsend, sw.list.p, vel.p, rm.p, cvv.p, cg.p,
               (double *)buf);
      },
      [&](Swap &sw, unsigned char *buf) {
        launch(k_mpx_unpack, sw.nrecv, sw.nrecv, (const int *)nullptr, sw.firstrecv,
               (const double *)buf, vel.p, rm.p, cvv.p, cg.p);
      });
}

// Per-step forward traffic, one dimension at a time (swap_pair)
template <class Pack, class Unpack>
inline void sph_engine::forward_dims(size_t rec, Pack pack, Unpack unpack) {
  for (int k = 0; k + 1 < nswap; k += 2) swap_pair(swaps[k], swaps[k + 1], rec, pack, unpack);
}

// Comm::forward_comm (x, vest, rho, e)
inline void sph_engine::forward_multi() {
  if (dr_ok) {
    forward_direct(
        9 * sizeof(double),
        [&](int n, unsigned char *buf) {
          launch(k_pack_direct, n, n, dr_sidx.p, xf.p, vr.p, en.p, (double *)buf);
        },
        [&](int n, unsigned char *buf) {
          launch(k_unpack_direct, n, n, dr_rslot.p, nlocal, box, gimg.p, (const double *)buf,
                 xf.p, vr.p, en.p);
        },
        [&] {
          launch(k_forward_self, dr_nself, dr_nself, dr_self.p, nlocal, box, goidx.p, gimg.p,
                 xf.p, vr.p, en.p);
        });
    return;
  }
  forward_dims(
      9 * sizeof(double),
      [&](Swap &sw, unsigned char *buf) {
        launch(k_pack_forward, sw.nsend, sw.nsend, sw.list.p, sw.dim, sw.shift, xf.p, vr.p, en.p,
               (double *)buf);
      },
      [&](Swap &sw, unsigned char *buf) {
        launch(k_unpack_forward, sw.nrecv, sw.nrecv, sw.firstrecv, (const double *)buf, xf.p,
               vr.p, en.p);
      });
  if (mp)
    for (int k = 0; k + 1 < nswap; k += 2) mpx_swap_pair(swaps[k], swaps[k + 1]);
}

// comm->reverse_comm_fix of one per-atom double (fix phase_change's dmass)
inline void sph_engine::reverse1(double *a) {
  if (!multi()) {
    if (nghost)
      launch(k_reverse1, nghost, nghost, nlocal, gowner.p, a);
    return;
  }
  reverse_swaps(
      sizeof(double),
      [&](Swap &sw) {
        launch(k_pack_rev1, sw.nrecv, sw.nrecv, sw.firstrecv, a, (double *)cbs.p);
      },
      [&](Swap &sw) {
        launch(k_unpack_rev1, sw.nsend, sw.nsend, sw.list.p, (const double *)cbr.p, a);
      });
}

// comm->forward_comm_pair of sph/rhosum: rho (+ the EOS term)
inline void sph_engine::forward_rho_multi() {
  if (dr_ok) {
    forward_direct(
        sizeof(double2),
        [&](int n, unsigned char *buf) {
          launch(k_pack_rho, n, n, dr_sidx.p, xf.p, vr.p, (double2 *)buf);
        },
        [&](int n, unsigned char *buf) {
          launch(k_unpack_rho_direct, n, n, dr_rslot.p, nlocal, (const double2 *)buf, xf.p, vr.p);
        },
        [&] {
          launch(k_forward_rho_self, dr_nself, dr_nself, dr_self.p, nlocal, goidx.p, xf.p, vr.p);
        });
    return;
  }
  forward_dims(
      sizeof(double2),
      [&](Swap &sw, unsigned char *buf) {
        launch(k_pack_rho, sw.nsend, sw.nsend, sw.list.p, xf.p, vr.p, (double2 *)buf);
      },
      [&](Swap &sw, unsigned char *buf) {
        launch(k_unpack_rho, sw.nrecv, sw.nrecv, sw.firstrecv, (const double2 *)buf, xf.p, vr.p);
      });
}

// The swaps in reverse order, ghosts back to their senders: pack(sw) fills cbs from the
// nrecv ghosts of a swap, unpack(sw) adds cbr to the nsend atoms of its list (rec bytes each)
template <class Pack, class Unpack>
inline void sph_engine::reverse_swaps(size_t rec, Pack pack, Unpack unpack) {
  for (int k = nswap - 1; k >= 0; k--) {
    Swap &sw = swaps[k];
    cbs.reserve((size_t)(sw.nrecv > 0 ? sw.nrecv : 1) * rec, true, s);
    cbr.reserve((size_t)(sw.nsend > 0 ? sw.nsend : 1) * rec, true, s);
    if (sw.nrecv) pack(sw);
    swap_move(sw.remote, (size_t)sw.nrecv * rec, sw.recvproc, (size_t)sw.nsend * rec,
              sw.sendproc);
    if (sw.nsend) unpack(sw);
  }
}

// Comm::reverse_comm (f, drho, de).  No caller today: the step's full lists are gather-only,
// so nothing goes back to the owners; it stays for a half-list (newton) pass on bricks and
// is untested until one exists.
inline void sph_engine::reverse_multi() {
  reverse_swaps(
      5 * sizeof(double),
      [&](Swap &sw) {
        launch(k_pack_reverse, sw.nrecv, sw.nrecv, sw.firstrecv, fo.p, de.p, (double *)cbs.p);
      },
      [&](Swap &sw) {
        launch(k_unpack_reverse, sw.nsend, sw.nsend, sw.list.p, (const double *)cbr.p, fo.p,
               de.p);
      });
}

// CommBrick::exchange (comm_brick.cpp:573-680): atoms that left the brick along each
// split dimension go to the face neighbours, which keep the ones inside their slab
inline void sph_engine::exchange_multi() {
  for (int d = 0; d < cfg.dim; d++) {
    if (pg[d] == 1) continue;
    const int n = nlocal;
    flags.reserve_min1(n);
    flag2.reserve_min1(n);
    if (n)
      launch(k_flag_leave, n, n, d, sublo[d], subhi[d], xf.p, flags.p, flag2.p);
    const int nl = select_flagged(flags.p, n, sel);
    migrations += nl;
    const int nst = select_flagged(flag2.p, n, sel2);
    if (pc && nl) hole_fill(n, nl, nst);  // (leavers put in send order, lidx renumbered)
    cbs.reserve((size_t)(nl > 0 ? nl : 1) * sizeof(MigRec));
    if (nl)
      launch(k_pack_mig, nl, nl, sel.p, xf.p, vr.p, vel.p, en.p, ty.p, tag.p, (MigRec *)cbs.p);
    if (mp && nl) {  // the leavers' extra fields
      xbuf.reserve((size_t)MPX * nl, false, s);
      launch(k_mpx_pack, nl, nl, sel.p, vel.p, rm.p, cvv.p, cg.p, xbuf.p);
    }
    if (nl) {  // compact the staying atoms to the front (order kept)
      DBuf<unsigned char> keep;
      keep.reserve((size_t)(nst > 0 ? nst : 1) * sizeof(MigRec));
      // (every record is packed from the old rows before any row is rewritten: the extra
      // fields' copy rewrites vel, which the records carry whole)
      if (nst)
        launch(k_pack_mig, nst, nst, sel2.p, xf.p, vr.p, vel.p, en.p, ty.p, tag.p,
               (MigRec *)keep.p);
      mpx_copy(nst, sel2.p, 0, xbuf2);
      if (nst)
        launch(k_gather_mig, nst, nst, (const int *)nullptr, (const MigRec *)keep.p, 0, xf.p,
               vr.p, vel.p, en.p, ty.p, tag.p);
      SPH_HIP_TRY(hipStreamSynchronize(s));
      keep.release();
    }
    nlocal = nst;
    // pg == 2: both neighbours are the same brick, one exchange; otherwise send the
    // leavers to both and let each keep its own
    const int nex = (pg[d] == 2) ? 1 : 2;
    for (int x = 0; x < nex; x++) {
      const int dest = procneigh[d][x], src = procneigh[d][1 - x];
      const int nr = tr->exchange_count(nl, dest, src, s);
      cbr.reserve((size_t)(nr > 0 ? nr : 1) * sizeof(MigRec));
      tr->exchange(cbs.p, (size_t)nl * sizeof(MigRec), dest, cbr.p, (size_t)nr * sizeof(MigRec),
                   src, s);
      if (mp) {
        xbuf2.reserve((size_t)MPX * (nr > 0 ? nr : 1), false, s);
        tr->exchange((unsigned char *)xbuf.p, (size_t)nl * MPX * sizeof(double), dest,
                     (unsigned char *)xbuf2.p, (size_t)nr * MPX * sizeof(double), src, s);
      }
      if (nr == 0) continue;
      flags.reserve(nr);
      launch(k_flag_mine, nr, nr, d, sublo[d], subhi[d], (const MigRec *)cbr.p, flags.p);
      const int nm = select_flagged(flags.p, nr, sel2);
      if (nm == 0) continue;
      ensure_atoms((size_t)nlocal + nm, true);
      vel.reserve((size_t)nlocal + nm, true, s);
      tag.reserve((size_t)nlocal + nm, true, s);
      launch(k_gather_mig, nm, nm, sel2.p, (const MigRec *)cbr.p, nlocal, xf.p, vr.p, vel.p, en.p,
             ty.p, tag.p);
      if (pc) {  // unpack_exchange appends in buffer order
        lidx.reserve((size_t)nlocal + nm, true, s);
        launch(k_lidx_iota, nm, nm, nlocal, lidx.p + nlocal);
      }
      if (mp)
        launch(k_mpx_unpack, nm, nm, sel2.p, nlocal, (const double *)xbuf2.p, vel.p, rm.p, cvv.p,
               cg.p);
      nlocal += nm;
    }
  }
  fo.reserve_min1(nlocal, true, s);
  de.reserve_min1(nlocal, true, s);
}

// One brick: CommBrick::borders' self swaps (comm_brick.cpp:696-864) with every count kept
// on the device -- each swap's selection size, and where its ghosts go, is read by the next
// kernels from device words (gnall), so the swaps run back to back with ONE host read at
// the end.  The ghost arrays are sized ahead from the last borders' ghost count (or the
// box geometry); a borders that would outgrow them is redone with twice the room.
inline void sph_engine::borders() {
  if (multi()) {
    borders_multi();
    return;
  }
  const int ndim = cfg.dim;
  int nsw = 0;
  for (int d = 0; d < ndim; d++)
    if (cfg.periodic[d]) nsw += 2;
  if (gcap_hint <= 0) {  // the ghost shell's share of the sub-box, with room
    double in = 1.0, out = 1.0;
    for (int d = 0; d < ndim; d++) {
      const double ext = std::max(subhi[d] - sublo[d], 1e-300);
      in *= ext;
      out *= ext + (cfg.periodic[d] ? 2.0 * cutghost : 0.0);
    }
    gcap_hint = (int)std::min(1.5 * (out / in - 1.0) * nlocal + 4096.0, 2.0e9 - nlocal);
  }
  gnall.reserve(nsw + 2);
  for (;;) {
    const int gcap = gcap_hint, cap = nlocal + gcap;
    ensure_atoms((size_t)cap, true);
    gowner.reserve(gcap, true, s);
    gimg.reserve(gcap, true, s);
    if (pc) gsrc.reserve(gcap, true, s);
    h_small[14] = nlocal;  // (pinned; the read-back below lands in words 0 .. nsw + 1)
    h_small[15] = 0;       // the overflow word
    to_dev(gnall.p, h_small + 14, 1);
    to_dev(gnall.p + nsw + 1, h_small + 15, 1);
    int w = 0;
    // a dimension's two swaps in three launches (k_brd_count / scan / scatter)
    for (int d = 0; d < ndim; d++) {
      if (!cfg.periodic[d]) continue;  // sendneed = 0 across a non-periodic boundary
      const double lo0 = -1.0e20, hi0 = sublo[d] + cutghost;
      const double lo1 = subhi[d] - cutghost, hi1 = 1.0e20;
      const int nb = (cap + BRD_CH - 1) / BRD_CH;
      bcnt.reserve(2 * (size_t)nb);
      hipLaunchKernelGGL(k_brd_count, dim3(nb), dim3(BRD_T), 0, s, gnall.p + w, d, lo0, hi0,
                         lo1, hi1, xf.p, bcnt.p);
      hipLaunchKernelGGL(k_brd_scan, dim3(1), dim3(1024), 0, s, nb, bcnt.p, gnall.p + w, cap,
                         gnall.p + nsw + 1);
      hipLaunchKernelGGL(k_brd_scatter, dim3(nb), dim3(BRD_T), 0, s, gnall.p + w, bcnt.p, cap,
                         nlocal, d, lo0, hi0, lo1, hi1, box.prd[d], xf.p, vr.p, en.p, ty.p,
                         gowner.p, gimg.p, pc ? gsrc.p : (int *)nullptr,
                         mp ? vel.p : (double4 *)nullptr, mp ? rm.p : (double *)nullptr,
                         mp ? cvv.p : (double *)nullptr, mp ? cg.p : (double4 *)nullptr);
      w += 2;
    }
    to_host(h_small, gnall.p, nsw + 2);
    SPH_HIP_TRY(hipStreamSynchronize(s));
    if (h_small[nsw + 1] == 0) break;
    SPH_REQUIRE(gcap < 1000000000, SPH_HIP_EOVERFLOW, "ghost count exceeds 2^30");
    gcap_hint = 2 * gcap;
  }
  gswap_first.clear();
  for (int w = 0; w <= nsw; w++) gswap_first.push_back(h_small[w] - nlocal);
  nghost = h_small[nsw] - nlocal;
  // next time: this count with room (atoms drift between rebuilds)
  gcap_hint = std::max(gcap_hint, nghost + nghost / 8 + 4096);
}

inline void sph_engine::forward() {
  if (multi()) {
    Scope t(this, T_COMM);
    forward_multi();
    if (inner && sc.x0 && nghost)
      launch(k_inner_ghosts, nghost, nghost, nlocal, sc, xf.p);
    return;
  }
  if (nghost == 0) return;
  Scope t(this, T_COMM);
  launch(k_forward, nghost, nghost, nlocal, box, gowner.p, gimg.p, xf.p, vr.p, en.p);
  mpx_copy(nghost, gowner.p, nlocal, xbuf);
}

// rhoF / cgF of the ghosts from their owners (the values the reference's half-list pass
// uses for a pair evaluated in the owner's row, k_mp_gather)
inline void sph_engine::forward_fresh() {
  if (!multi()) {
    if (nghost)
      launch(k_mp_fwd_fresh, nghost, nghost, nlocal, gowner.p, rhoF.p, cgF.p);
    return;
  }
  forward_dims(
      4 * sizeof(double),
      [&](Swap &sw, unsigned char *buf) {
        launch(k_mp_pack_fresh, sw.nsend, sw.nsend, sw.list.p, rhoF.p, cgF.p, (double *)buf);
      },
      [&](Swap &sw, unsigned char *buf) {
        launch(k_mp_unpack_fresh, sw.nrecv, sw.nrecv, sw.firstrecv, (const double *)buf, rhoF.p,
               cgF.p);
      });
}
