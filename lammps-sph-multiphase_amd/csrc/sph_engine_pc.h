// sph_engine_pc.h -- fix phase_change in the engine (FixPhaseChange::pre_exchange,
// fix_phase_change.cpp; kernels and the split of the work: sph_pc.h): LAMMPS' local order of the
// owned atoms that the fix's random stream follows (CommBrick::exchange's hole fill, Atom::sort,
// the order by tag), the ghosts' LAMMPS slots on one brick and on bricks, and the fix itself.
// Writes: lidx and its sort scratch (lidx2, lidx_tab, skey*, srow*, lidx_valid, nextsort), the
// ghost slot ranks (pc_grank, pc_key, pc_val), the pc_* scratch, dmass; phase_change creates
// atoms: nlocal, the owned arrays, tag / tag_next, pc_inserted, pc_tags_agreed.
#pragma once
#include "sph_engine_state.h"

// CommBrick::exchange's scan of one dimension (comm_brick.cpp:620-632) on the LAMMPS
// indices: a departing atom's slot takes the last atom, which is examined next.  The n - nst
// leavers (sel) go into the buffer in that order -- the receivers append them as LAMMPS
// does -- and the stayers' indices are compacted along sel2, the tail atoms that moved
// into holes renumbered.  Host work over the leavers only (the tail atom at LAMMPS index
// m is always the one that started there: moves only go from the tail into lower holes).
inline void sph_engine::hole_fill(int n, int nl, int nst) {
  std::vector<int> hl(nl), hr(nl);
  lidx_tab.reserve(nl);
  launch(k_lidx_take, nl, nl, sel.p, lidx.p, 0, (const int *)nullptr, lidx_tab.p);
  to_host(hl.data(), lidx_tab.p, nl);
  to_host(hr.data(), sel.p, nl);
  SPH_HIP_TRY(hipStreamSynchronize(s));
  std::vector<int> ord(nl);
  for (int k = 0; k < nl; k++) ord[k] = k;
  std::sort(ord.begin(), ord.end(), [&](int a, int b) { return hl[a] < hl[b]; });
  if ((int)h_leave.size() < n) h_leave.resize(n, 0);
  for (int k = 0; k < nl; k++) h_leave[hl[k]] = 1;
  std::vector<int> sent, tab(nl, -1);
  sent.reserve(nl);
  int m = n;
  for (int q = 0; q < nl; q++) {
    const int p = hl[ord[q]];  // the leavers in ascending LAMMPS index
    if (p >= m) break;         // (already sent from the tail)
    sent.push_back(p);
    for (;;) {
      m--;
      if (m == p) break;  // the hole was the last slot
      if (h_leave[m]) {   // the tail atom leaves too: examined in the hole, sent
        sent.push_back(m);
        continue;
      }
      tab[m - nst] = p;
      break;
    }
  }
  for (int k = 0; k < nl; k++) h_leave[hl[k]] = 0;
  SPH_REQUIRE((int)sent.size() == nl && m == nst, SPH_HIP_ERUNTIME,
              "exchange: hole fill sent %zu of %d atoms", sent.size(), nl);
  std::vector<int> rows(nl);  // sel in send order
  for (int k = 0; k < nl; k++) {
    const int v = sent[k];
    const auto it = std::lower_bound(ord.begin(), ord.end(), v,
                                     [&](int a, int val) { return hl[a] < val; });
    rows[k] = hr[*it];
  }
  to_dev(sel.p, rows.data(), nl);
  to_dev(lidx_tab.p, tab.data(), nl);
  if (nst) {
    lidx2.reserve_exact(lidx.cap);
    launch(k_lidx_take, nst, nst, sel2.p, lidx.p, nst, lidx_tab.p, lidx2.p);
    dev_copy(lidx.p, lidx2.p, nst);
  }
  SPH_HIP_TRY(hipStreamSynchronize(s));  // (host vectors)
}

// Atom::sort (atom.cpp:1555-1654) on the LAMMPS indices: the bins of setup_sort_bins
// (:1660-1726) over this brick's sub-box, atoms listed bin by bin and in their current order
// within a bin; one bin = no sort.  nextsort as atom.cpp:1561.
inline void sph_engine::atom_sort() {
  nextsort = (step / sortfreq) * sortfreq + sortfreq;
  const double bs = sort_binsize > 0.0 ? sort_binsize : 0.5 * cutneighmax;
  const double bininv = 1.0 / bs;
  SortBins b{};
  double nbins = 1.0;
  for (int d = 0; d < 3; d++) {
    const double ext = subhi[d] - sublo[d];
    int m = (int)(ext * bininv);
    if (d == 2 && cfg.dim == 2) m = 1;
    if (m == 0) m = 1;
    b.lo[d] = sublo[d];
    b.nb[d] = m;
    b.inv[d] = m / ext;
    nbins *= m;
  }
  SPH_REQUIRE(nbins <= 2147483647.0, SPH_HIP_EINVAL, "Too many atom sorting bins");
  const int n = nlocal;
  if (nbins == 1.0 || n == 0) return;
  skey.reserve(n);
  skey2.reserve(n);
  srow.reserve(n);
  srow2.reserve(n);
  launch(k_lidx_sortkeys, n, n, b, xf.p, lidx.p, skey.p, srow.p);
  int hb = 32;
  while ((double)(1ll << (hb - 32)) < nbins) hb++;
  cub([&](void *t, size_t &tb) {
    return hipcub::DeviceRadixSort::SortPairs(t, tb, skey.p, skey2.p, srow.p, srow2.p, n, 0, hb,
                                              s);
  });
  launch(k_lidx_rank, n, n, srow2.p, lidx.p);
}

// the LAMMPS indices from the tags: read order (tag order) -- set_atoms, read_restart
inline void sph_engine::lidx_from_tags() {
  const int n = nlocal;
  lidx.reserve_min1(n);
  lidx_valid = true;
  if (n == 0) return;
  skey.reserve(n);
  skey2.reserve(n);
  srow.reserve(n);
  srow2.reserve(n);
  launch(k_lidx_tagkeys, n, n, tag.p, skey.p, srow.p);
  cub([&](void *t, size_t &tb) {
    return hipcub::DeviceRadixSort::SortPairs(t, tb, skey.p, skey2.p, srow.p, srow2.p, n, 0, 32,
                                              s);
  });
  launch(k_lidx_rank, n, n, srow2.p, lidx.p);
}

// LAMMPS' index order of this brick's ghosts (one process): CommBrick::borders appends each
// swap's ghosts in the order of the atoms it scans (comm_brick.cpp:741-800), i.e. by the
// LAMMPS index of their source -- tag - 1 for an owned atom (local order = tag order on one
// process without sorting), nlocal + slot for a ghost of an earlier swap.  Our swaps hold
// the same ghosts in our own (Hilbert) order; sort each swap by that key: grank[g] = the
// ghost's LAMMPS slot.  Used only when a created atom may overwrite a slot a candidate reads.
inline void sph_engine::pc_ghost_slots() {
  pc_grank.reserve_min1(nghost);
  for (size_t w = 0; w + 1 < gswap_first.size(); w++) {
    const int first = gswap_first[w], ns = gswap_first[w + 1] - first;
    if (ns == 0) continue;
    pc_key.reserve(2 * (size_t)ns);
    pc_val.reserve(2 * (size_t)ns);
    launch(k_pc_swapkeys, ns, ns, first, gsrc.p, nlocal, lidx.p, pc_grank.p, pc_key.p, pc_val.p);
    pc_rank_swap(ns, first, 32);
  }
}
// a swap's ns ghosts from slot `first` on: pc_key / pc_val sorted by the low `bits` key bits
// (into their upper halves), the ghosts' ranks from that order
inline void sph_engine::pc_rank_swap(int ns, int first, int bits) {
  cub([&](void *t, size_t &tb) {
    return hipcub::DeviceRadixSort::SortPairs(t, tb, pc_key.p, pc_key.p + ns, pc_val.p,
                                              pc_val.p + ns, ns, 0, bits, s);
  });
  launch(k_pc_swaprank, ns, ns, first, pc_val.p + ns, pc_grank.p);
}

// Bricks: the same slot order, but a swap's ghosts come from another rank, whose scan
// order (owned atoms in tag order, then its ghosts in slot order) only it knows -- each
// dimension's two swaps send that key along the send lists (one exchange), the receiver
// sorts each swap by it.  Collective over the ranks (every rank calls it).
inline void sph_engine::pc_ghost_slots_multi() {
  pc_grank.reserve_min1(nghost);
  for (int k = 0; k + 1 < nswap; k += 2)
    swap_pair(
        swaps[k], swaps[k + 1], sizeof(int),
        [&](Swap &sw, unsigned char *buf) {
          launch(k_pc_sendkeys, sw.nsend, sw.nsend, sw.list.p, nlocal, lidx.p, pc_grank.p,
                 (int *)buf);
        },
        [&](Swap &sw, unsigned char *buf) {
          const int ns = sw.nrecv;
          pc_key.reserve(2 * (size_t)ns);
          pc_val.reserve(2 * (size_t)ns);
          launch(k_pc_keys_in, ns, ns, (const int *)buf, pc_key.p, pc_val.p);
          pc_rank_swap(ns, sw.firstrecv - nlocal, 31);
        });
}

// FixPhaseChange::pre_exchange (fix_phase_change.cpp:167-352) on the last build's full
// list, owned atoms as integrated, ghosts as last communicated; the rebuild follows.
// Bricks: every rank runs the call on its own atoms with its own RanPark of the same seed
// (:116), creating atoms only inside its sub-box; the ghosts' dmass goes back over the
// swaps (reverse_comm_fix, :324), and the created atoms take the next tags rank by rank
// (MPI_Allreduce + Atom::tag_extend, :338-351).  A rank with no candidate still takes part
// in the collectives (slot keys, reverse comm, counts) and in the finish loop.
inline void sph_engine::phase_change() {
  Scope t(this, T_NEIGH);
  // (SPH_DEBUG: host time between the stages of this call)
  const bool dbg = env_int("SPH_DEBUG", 0) != 0;
  std::vector<std::pair<const char *, std::chrono::steady_clock::time_point>> tm;
  auto mark = [&](const char *w) {
    if (dbg) tm.emplace_back(w, std::chrono::steady_clock::now());
  };
  mark("start");
  if (!lidx_valid) lidx_from_tags();  // (read_restart: the file's tag order)
  const bool mul = multi();
  const int n = nlocal, nall = nlocal + nghost;
  if (n == 0 && !mul) return;
  sph_phasechange_params p = pcp;
  for (int k = 0; k < 3; k++) {
    p.sublo[k] = sublo[k];
    p.subhi[k] = subhi[k];
    p.boxhi[k] = box.hi[k];
    p.top[k] = myloc[k] == pg[k] - 1;
  }
  const PcDev pd{cfg.dim, p.from_type, p.to_type, p.Tc, p.to_mass, p.cutoff};
  DBuf<int> &flag = pc_flag, &cand = pc_cand, &otag = pc_otag, &idx = pc_idx;
  DBuf<double> &rec = pc_rec, &gat = pc_gat, &Wd = pc_Wd, &vals = pc_vals, &nrec = pc_nrec;
  int ncand = 0;
  if (n > 0) {
    flag.reserve(n);
    launch(k_pc_flags, n, n, (const int *)nullptr, ty.p, en.p, cvv.p, pd, flag.p);
    ncand = select_flagged(flag.p, n, cand);
  }
  if (ncand == 0 && !mul) return;  // (dmass 0: the finish loop leaves rmass and e as they are)
  const int lst = strided ? list_stride : 0;
  PcRank rk{n, 1, nullptr};
  auto walk = [&](const PcRank &r) {
    hipLaunchKernelGGL(k_pc_candidates<8>, mp_rows(ncand), dim3(256), 0, s, ncand, cand.p,
                       (const int *)nullptr, off.p, nbr.p, xf.p, vr.p, (const double *)vel.p,
                       4, ty.p, rm.p, pd, rec.p, lst, ccnt.p, r, 0, 0, pc_minr.p);
  };
  std::vector<int> hm(ncand), hc(ncand), ht(ncand);
  std::vector<double> hr((size_t)8 * ncand), hg((size_t)9 * ncand);
  if (mul) {  // slot ranks first (collective), then one walk with them
    pc_ghost_slots_multi();
    rk = PcRank{n, 2, pc_grank.p};
  }
  if (ncand > 0) {
    rec.reserve((size_t)8 * ncand);
    gat.reserve((size_t)9 * ncand);
    otag.reserve(ncand);
    // one brick: the first pass screens -- every ghost ranks 0, so minr < NORANK flags the
    // candidates whose row holds a from_type ghost at all; only then are LAMMPS' ghost
    // slots worked out
    pc_minr.reserve(ncand);
    walk(rk);
    if (!mul) {
      to_host(hm.data(), pc_minr.p, ncand);
      SPH_HIP_TRY(hipStreamSynchronize(s));
      if (std::any_of(hm.begin(), hm.end(), [](int v) { return v != PC_NORANK; })) {
        pc_ghost_slots();
        rk = PcRank{n, 2, pc_grank.p};
        walk(rk);
      }
    }
    launch(k_pc_gather, ncand, ncand, cand.p, xf.p, vr.p, en.p, cvv.p, cg.p, lidx.p, gat.p,
           otag.p);
    to_host(hm.data(), pc_minr.p, ncand);
    to_host(hc.data(), cand.p, ncand);
    to_host(ht.data(), otag.p, ncand);
    to_host(hr.data(), rec.p, hr.size());
    to_host(hg.data(), gat.p, hg.size());
    SPH_HIP_TRY(hipStreamSynchronize(s));
  }
  mark("readback");
  // the reference meets the candidates in its local order (lidx: read order, exchange hole
  // fill, Atom::sort)
  std::vector<int> ord(ncand);
  for (int k = 0; k < ncand; k++) ord[k] = k;
  std::sort(ord.begin(), ord.end(), [&](int a, int b) { return ht[a] < ht[b]; });
  std::vector<PcCand> cands(ncand);
  for (int q = 0; q < ncand; q++) {
    const int k = ord[q];
    PcCand &c = cands[q];
    const double *g = &hg[(size_t)9 * k];
    for (int d = 0; d < 3; d++) {
      c.x[d] = g[d];
      c.cg[d] = g[3 + d];
    }
    c.e = g[6];
    c.cv = g[7];
    c.rho = g[8];
    for (int d = 0; d < 8; d++) c.rec[d] = hr[(size_t)8 * k + d];
    c.minr = hm[k];
  }
  auto recompute = [&](size_t q, int dead_a, int dead_w, double *out) {
    pc_one.reserve(1);
    to_dev(pc_one.p, &hc[ord[q]], 1);
    hipLaunchKernelGGL(k_pc_candidates<8>, dim3(1), dim3(256), 0, s, 1, pc_one.p,
                       (const int *)nullptr, off.p, nbr.p, xf.p, vr.p, (const double *)vel.p,
                       4, ty.p, rm.p, pd, Wd.p, lst, ccnt.p, rk, dead_a, dead_w, (int *)nullptr);
    to_host(out, Wd.p, 8);
    SPH_HIP_TRY(hipStreamSynchronize(s));
  };
  Wd.reserve(8);
  std::vector<int> ins_k;
  std::vector<double> ins_rec, ins_W;
  mark("candidates");
  pc_replay(p, cfg.dim, pc_seed, cands, ins_k, ins_W, ins_rec, recompute);
  mark("replay");
  const int nins = (int)ins_k.size();
  // MPI_Allreduce(nins) and the tag base of this rank's created atoms (tag_extend: rank
  // order); the first call also agrees on the next free tag
  int ninsall = nins, tag0 = tag_next;
  if (mul) {
    std::vector<int> all(tr->size());
    if (!pc_tags_agreed) {
      tr->allgather_int(tag_next, all.data(), s);
      tag_next = *std::max_element(all.begin(), all.end());
      pc_tags_agreed = true;
    }
    tr->allgather_int(nins, all.data(), s);
    ninsall = 0;
    tag0 = tag_next;
    for (int r = 0; r < (int)all.size(); r++) {
      if (r < tr->rank()) tag0 += all[r];
      ninsall += all[r];
    }
  }
  if (nins == 0 && !mul) return;
  std::vector<int> hidx(nins);
  std::vector<double> hval(nins), hW(nins);
  for (int q = 0; q < nins; q++) {
    const int k = ord[ins_k[q]];
    hidx[q] = hc[k];  // the candidate's row = its atom (identity row list)
    hval[q] = ins_rec[(size_t)13 * q + 9];
    hW[q] = ins_W[q];
  }
  dmass.reserve_min1(nall);
  mark("host");
  if (nall) SPH_HIP_TRY(hipMemsetAsync(dmass.p, 0, nall * sizeof(double), s));
  if (nins) {
    idx.reserve(nins);
    vals.reserve(nins);
    Wd.reserve(nins);
    nrec.reserve((size_t)13 * nins);
    to_dev(idx.p, hidx.data(), nins);
    to_dev(vals.p, hval.data(), nins);
    to_dev(Wd.p, hW.data(), nins);
    to_dev(nrec.p, ins_rec.data(), ins_rec.size());
    // e_i = (e_i - Hwv)/2 of the atoms that changed phase, the donors' dmass
    launch(k_pc_set_e, nins, nins, idx.p, vals.p, en.p);
    // (in candidate order per donor: the reference's sum, fix_phase_change.cpp:289-299)
    const long long cap = (long long)nins * std::max(lst > 0 ? lst : nbr_maxrow, 1);
    pc_dmass_ordered<8>(s, nins, idx.p, Wd.p, (const int *)nullptr, off.p, nbr.p, xf.p, ty.p,
                        rm.p, pd, lst, ccnt.p, rk, cap, pc_k0, pc_k1, pc_v0, pc_v1, pc_cnt,
                        tmp, dmass.p);
  }
  // its reverse comm, rmass -= dmass and e renormalised, then the new atoms
  reverse1(dmass.p);
  if (n)
    launch(k_pc_finish, n, n, dmass.p, rm.p, en.p);
  if (nins) {
    ensure_atoms((size_t)n + nins, true);  // (over the ghost slots: the rebuild follows)
    vel.reserve((size_t)n + nins, true, s);
    tag.reserve((size_t)n + nins, true, s);
    fo.reserve((size_t)n + nins, true, s);
    de.reserve((size_t)n + nins, true, s);
    launch(k_pc_append, nins, nins, nrec.p, n, p.to_type, tag0, xf.p, vr.p, vel.p, en.p, rm.p,
           cvv.p, cg.p, ty.p, tag.p, fo.p, de.p);
    lidx.reserve((size_t)n + nins, true, s);  // (create_atom: at the end, in creation order)
    launch(k_lidx_iota, nins, nins, n, lidx.p + n);
  }
  SPH_HIP_TRY(hipStreamSynchronize(s));  // (the host staging vectors go out of scope)
  mark("end");
  if (dbg) {
    fprintf(stderr, "[sph] phase change: %d candidates, %d inserted;", ncand, nins);
    for (size_t k = 1; k < tm.size(); k++)
      fprintf(stderr, " %s %.1f us", tm[k].first,
              std::chrono::duration<double, std::micro>(tm[k].second - tm[k - 1].second).count());
    fprintf(stderr, "\n");
  }
  if (ninsall == 0) return;  // (natoms unchanged: the ghosts stay, the rebuild follows)
  nlocal = n + nins;
  nghost = 0;
  tag_next += ninsall;
  pc_inserted += nins;
}
