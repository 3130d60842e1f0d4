// sph_engine_neigh.h -- the neighbour rebuild (neighbor.cpp: Neighbor::decide, setup_bins,
// build) on the device: the counting sorts and the spatial sort of the owned atoms, cutoffs and
// bin geometry, the binned copy, the full list (strided rows or CSR), the block build with its
// inner rows and their refresh, and neigh_modify's every / delay / check bookkeeping.
// Writes: the owned arrays' order (sort_owned swaps them with their twins), cutneighmax /
// cutghost, bn / qb / qbn and the bin arrays, the cs_* words of the counting sorts, the list (cnt,
// off, nbr, ccnt, nbr_*, strided, list_*), the block path's state (blk, blk_*, ulist, ucnt,
// snbr, uilist, uicnt, snbi, icnt, moved, x0, inner*), xhold / nm_flag and the nm_* counters,
// last_sort, last_build, rho_fused_step and ov_ready.
#pragma once
#include "sph_engine_state.h"

// ------------------------------------------------------------------------------------
// Counting sort of xf[0, n) by the key of k_bin_keys (sph_engine_kernels.h, k_cs_*), first
// half: histogram (keys -> bkey, arrival numbers -> bkey2) and the exclusive scan of the
// K + 1 counts into beg.  w = 0 (bin_q) | 1 (sort_owned).  False = take the radix sort:
//  * SPH_TUNE_CSORT 0;
//  * a key space the atoms do not fill: counting while K <= CS_KFLOOR or K <= CS_KPERN * n,
//    never past CS_KMAX (the 30-bit curve keys of large boxes, a few atoms in a wide box:
//    clearing and scanning the counts would cost more than the radix passes);
//  * a segment longer than CS_CAP (k_cs_place reads a whole segment per element).
// The longest segment is known on the device after the histogram.  While the build before
// (of the same sort) saw none above CS_CAP / 2, this one goes on without waiting for its
// own word -- bin counts move by a few atoms between rebuilds -- and that word is read
// back behind the build for the next one.  The first build, and any build after one that
// came within a factor two of the cap, waits for the word (one stream synchronisation) and
// decides on its own count.  Whatever the segment lengths, the order is the exact one.
inline bool sph_engine::cs_count(int w, int n, long long K0, const Bins &b, int morton, int hdim,
                                 DBuf<int> &begb) {
  if (!csort || n < 1 || K0 < 1 || K0 > CS_KMAX) return false;
  if (K0 > CS_KFLOOR && K0 > (long long)CS_KPERN * n) return false;
  const int K = (int)K0;
  begb.reserve((size_t)K + 1);
  int *const beg = begb.p;
  int prev = cs_prev[w];
  if (cs_pending[w]) {
    SPH_HIP_TRY(hipEventSynchronize(cs_ev[w]));
    cs_pending[w] = false;
    prev = h_cs[w];
  }
  if (!setup_done) prev = -1;
  cs_cnt.reserve((size_t)K + 1);
  cs_mx.reserve(2);
  SPH_HIP_TRY(hipMemsetAsync(cs_cnt.p, 0, ((size_t)K + 1) * sizeof(int), s));
  SPH_HIP_TRY(hipMemsetAsync(cs_mx.p + w, 0, sizeof(int), s));
  launch(k_cs_hist, n, n, b, xf.p, bkey.p, (int *)bkey2.p, cs_cnt.p, K, cs_mx.p + w, morton,
         hdim);
  to_host(h_cs + w, cs_mx.p + w, 1);
  if (prev != 0) {
    SPH_HIP_TRY(hipStreamSynchronize(s));
    cs_prev[w] = h_cs[w];
    if (cs_prev[w] > CS_CAP) return false;
  } else {
    SPH_HIP_TRY(hipEventRecord(cs_ev[w], s));
    cs_pending[w] = true;
  }
  cub([&](void *t, size_t &tb) {
    return hipcub::DeviceScan::ExclusiveSum(t, tb, cs_cnt.p, beg, K + 1, s);
  });
  return true;
}

inline void sph_engine::sort_owned() {
  if (nlocal < 1) return;
  const int n = nlocal;
  bkey.reserve(n);
  bkey2.reserve(n);
  bidx.reserve(n);
  bidx2.reserve(n);
  // Space-filling-curve order over cells of 1/div of a bin per axis (bins fit 10 bits per
  // axis; else linear bins): consecutive rows are a compact region, so a block's union
  // (block path) or a wave's gathers (row path) stay small and within one XCD's L2
  const int div = morton_div();
  Bins kbn = bn;
  for (int k = 0; k < 3; k++)
    if (bn.nb[k] > 1) {
      kbn.nb[k] = bn.nb[k] * div;
      kbn.inv[k] = bn.inv[k] * div;
    }
  if (want_blk()) {
    // block path: cells of ~1/div of a bin over the OWNED sub-box only, so the Hilbert
    // curve (over the next power of two of cells) leaves the rows' region as rarely as
    // possible -- a block of consecutive rows stays one compact piece of space
    for (int k = 0; k < 3; k++) {
      const double ext = subhi[k] - sublo[k];
      if (k >= cfg.dim || ext <= 0.0) {
        kbn.lo[k] = sublo[k];
        kbn.nb[k] = 1;
        kbn.inv[k] = 0.0;
        continue;
      }
      // a power of two per axis: a cubic sub-box (and the 2x1x1 / 2x2x1 / 2x2x2 bricks
      // of a cubic box) is then whole octants of the curve's cube, which the curve leaves
      // only between octants -- with any other count it exits and re-enters the
      // rows' region, and a block of consecutive rows spanning such a jump outgrows the
      // build's candidate image (seen at 125k particles per brick: the whole build fell
      // back to 32-row blocks)
      const int nc0 = std::max(1, (int)std::ceil(ext / (cutneighmax / div)));
      int nc = 1;
      while (nc < nc0 && nc < 1024) nc *= 2;
      if (!hil_pow2()) nc = std::min(nc0, 1024);
      kbn.lo[k] = sublo[k];
      kbn.nb[k] = nc;
      kbn.inv[k] = nc / ext;
    }
  }
  const bool mort = kbn.nb[0] <= 1024 && kbn.nb[1] <= 1024 && kbn.nb[2] <= 1024;
  if (!mort) kbn = bn;
  // the block path orders rows along a Hilbert curve (its blocks of consecutive rows stay
  // compact), the row path along a Morton curve
  int cb = 1;
  const int mx3 = std::max(kbn.nb[0], std::max(kbn.nb[1], kbn.nb[2]));
  while ((1 << cb) < mx3) cb++;
  const bool hil = mort && want_blk() && cb >= 2;
  const int morton = hil ? cb + 1 : (mort ? 1 : 0);
  // key bits: dim (Hilbert) or 3 (Morton) x bits of the largest cell dimension, else
  // bits(nbins)
  const int kb = mort ? cb * (hil ? cfg.dim : 3) : key_bits(nbins);
  // the permutation bidx2: the counting sort over the 2^kb keys (k_cs_*: the order within a
  // key by index, as the stable radix sort's), else the radix sort
  cs_flags &= ~SPH_STAT_CSORT_ROWS;
  if (cs_count(1, n, 1ll << kb, kbn, morton, cfg.dim, cs_beg)) {
    launch(k_cs_scatter, n, n, bkey.p, (const int *)bkey2.p, cs_beg.p, bidx.p);
    launch(k_cs_place<false>, n, n, bkey.p, cs_beg.p, bidx.p, bidx2.p, (const double4 *)nullptr,
           (const int *)nullptr, (double4 *)nullptr, (int *)nullptr, (int *)nullptr, 0);
    cs_flags |= SPH_STAT_CSORT_ROWS;
  } else {
    launch(k_bin_keys, n, n, 0, kbn, xf.p, bkey.p, bidx.p, morton, cfg.dim);
    cub([&](void *t, size_t &tb) {
      return hipcub::DeviceRadixSort::SortPairs(t, tb, bkey.p, bkey2.p, bidx.p, bidx2.p, n, 0, kb,
                                                s);
    });
  }
  // twins of equal capacity: the swaps below then never reallocate (a growing twin would
  // cost a hipMalloc + a synchronising hipFree at every rebuild)
  if (mp) {  // the extra fields in the new order, packed before the permutation
    xbuf.reserve((size_t)MPX * n, false, s);
    launch(k_mpx_pack, n, n, bidx2.p, vel.p, rm.p, cvv.p, cg.p, xbuf.p);
  }
  grow_twins();
  launch(k_permute, n, n, bidx2.p, xf.p, vr.p, en.p, ty.p, vel.p, tag.p, xf2.p, vr2.p, en2.p,
         ty2.p, vel2.p, tag2.p);
  std::swap(xf, xf2);
  std::swap(vr, vr2);
  std::swap(en, en2);
  std::swap(ty, ty2);
  std::swap(vel, vel2);
  std::swap(tag, tag2);
  if (pc) {  // (the LAMMPS index rides along)
    lidx2.reserve_exact(lidx.cap);
    launch(k_lidx_take, n, n, bidx2.p, lidx.p, 0, (const int *)nullptr, lidx2.p);
    std::swap(lidx, lidx2);
  }
  if (mp)
    launch(k_mpx_unpack, n, n, (const int *)nullptr, 0, xbuf.p, vel.p, rm.p, cvv.p, cg.p);
}

// the sort's twins at the capacity of the arrays they swap with; called again at the end
// of every build, so that the growth borders caused (ghosts) is matched in the same build
// -- at setup -- and not by a hipMalloc + synchronising hipFree in the next one (~1 ms of
// host time in the first rebuild after setup, profiles/r04/first_rebuild)
inline void sph_engine::grow_twins() {
  xf2.reserve_exact(xf.cap);
  vr2.reserve_exact(vr.cap);
  en2.reserve_exact(en.cap);
  ty2.reserve_exact(ty.cap);
  vel2.reserve_exact(vel.cap);
  tag2.reserve_exact(tag.cap);
}

// kernel_path 0: block-staged passes (production; the row path takes over for a build
// whose blocks overflow); 1: the row path (row2 gathers over the strided global list)
inline bool sph_engine::want_blk() const { return cfg.kernel_path == 0; }

// The neighbour and ghost cutoffs from cutmax_tab, the checks that depend on them, and the
// bins: at create, and again when sph_engine_idealgas adds its cut
inline void sph_engine::set_cutoffs() {
  const int nt = cfg.ntypes;
  std::vector<double> cutmax = cutmax_tab;
  // mirror upper triangle into a symmetric max-cut table (init_one semantics)
  for (int i = 1; i <= nt; i++)
    for (int j = 1; j < i; j++) cutmax[i * (nt + 1) + j] = cutmax[j * (nt + 1) + i];
  // inner rows of the block path (sph_blk_kernels.h k_blk_inner): a sixteenth of the skin
  // -- rows of ~110 instead of ~120 entries at C2 (with 16-entry walk chunks 114.5 instead
  // of 128 pair evaluations), valid while no atom has moved skin/32 since the build
  inner_margin = SPH_INNER_FRAC * cfg.skin;
  cutneighmax = coef_cutneigh(hc, nt, cutmax.data(), cfg.skin, inner_margin);
  SPH_REQUIRE(cutneighmax > 0.0, SPH_HIP_EINVAL, "no pair style enabled / zero cutoff");
  cutghost = cutneighmax;  // CommBrick::setup: cutghost = cutneighmax (:166)
  for (int k = 0; k < 3; k++) {
    if (box.periodic[k])
      SPH_REQUIRE(cutghost < box.prd[k], SPH_HIP_EINVAL,
                  "ghost cutoff %g >= box length %g in dim %d (multi-hop borders unsupported)",
                  cutghost, box.prd[k], k);
    if (pg[k] > 1)  // CommBrick maxneed = 1: a brick must be wider than the ghost cut
      SPH_REQUIRE(cutghost < subhi[k] - sublo[k], SPH_HIP_EINVAL,
                  "ghost cutoff %g >= brick width %g in dim %d (multi-hop swaps unsupported)",
                  cutghost, subhi[k] - sublo[k], k);
  }
  setup_bins_geometry();
}

inline void sph_engine::setup_bins_geometry() {
  for (int k = 0; k < 3; k++) {
    double lo = sublo[k], hi = subhi[k];
    if (k < cfg.dim) {
      lo -= cutghost;
      hi += cutghost;
      const double ext = hi - lo;
      int nb = (int)(ext / cutneighmax);
      if (nb < 1) nb = 1;
      if (nb > 4096) nb = 4096;
      bn.lo[k] = lo;
      bn.nb[k] = nb;
      bn.inv[k] = nb / ext;
    } else {
      bn.lo[k] = lo;
      bn.nb[k] = 1;
      bn.inv[k] = 0.0;
    }
  }
  nbins = bn.nb[0] * bn.nb[1] * bn.nb[2];
  // half-size bins of the list builders (k_neigh3, k_blk_neigh: reach 2 in y and z; the
  // x-range of a bin-row is cut to the sphere per row, at the bins' x resolution).  The
  // multiphase engine's per-step list fill (k_neigh3 with the fused rhosum, instruction-
  // bound) takes bins three times finer in x: ~19 % fewer candidates per row, C5 11.54 ->
  // 11.17 ms per step (profiles/r06/qbx/); the block build of C2 gained nothing measurable
  const int fx = mp ? 3 : 1;
  double ext[3];
  int nb[3];
  for (int k = 0; k < 3; k++) {
    ext[k] = bn.nb[k] > 0 && bn.inv[k] > 0.0 ? bn.nb[k] / bn.inv[k] : 0.0;
    nb[k] = 1;
    if (k < cfg.dim)
      nb[k] = std::max(1, std::min((int)(ext[k] / (0.5 * cutneighmax / (k == 0 ? fx : 1))), 8192));
  }
  fill_qbins(qb, qbn, bn.lo, ext, nb, cfg.dim, cutneighmax * cutneighmax);
  nqbins = qb.nb[0] * qb.nb[1] * qb.nb[2];
}

// bin-ordered copy of all atoms over the half-size bins (xb, tb, qbeg)
inline void sph_engine::bin_q() {
  const int nall = nlocal + nghost;
  bkey.reserve(nall);
  bkey2.reserve(nall);
  bidx.reserve(nall);
  bidx2.reserve(nall);
  qbeg.reserve(nqbins + 1);
  xb.reserve(nall);
  tb.reserve(nall);
  // (mp: k_bin_copy packs the type into xb.w above bit 28, the list entries' MP_NMASK)
  SPH_REQUIRE(!mp || (long long)nall < MP_MAXALL, SPH_HIP_EOVERFLOW,
              "multiphase lists index at most 2^28 atoms per rank (%d)", nall);
  xpos.reserve(nall);
  // the counting sort over the nqbins keys: its scan is qbeg itself, and its last pass
  // writes the bin-ordered copy (k_cs_place<true>: k_bin_copy fused; SPH_TUNE_CSORT 2 keeps
  // the two apart); else the radix sort, k_lower_bound and k_bin_copy (bin_copy_radix)
  cs_flags &= ~SPH_STAT_CSORT_BINS;
  if (cs_count(0, nall, nqbins, qbn, 0, 3, qbeg)) {
    launch(k_cs_scatter, nall, nall, bkey.p, (const int *)bkey2.p, qbeg.p, bidx.p);
    if (csort == 2) {
      launch(k_cs_place<false>, nall, nall, bkey.p, qbeg.p, bidx.p, bidx2.p,
             (const double4 *)nullptr, (const int *)nullptr, (double4 *)nullptr, (int *)nullptr,
             (int *)nullptr, 0);
      launch(k_bin_copy, nall, nall, bidx2.p, xf.p, ty.p, xb.p, tb.p, xpos.p, mp ? 1 : 0);
    } else {
      launch(k_cs_place<true>, nall, nall, bkey.p, qbeg.p, bidx.p, (int *)nullptr, xf.p, ty.p,
             xb.p, tb.p, xpos.p, mp ? 1 : 0);
    }
    cs_flags |= SPH_STAT_CSORT_BINS;
    return;
  }
  bin_copy_radix(s, tmp, nall, nqbins, qbn, xf.p, ty.p, bkey.p, bkey2.p, bidx.p, bidx2.p, qbeg.p,
                 xb.p, tb.p, xpos.p, mp ? 1 : 0);
}
// Global-index full list (k_neigh3, Neighbor::full_bin membership) of the owned rows at
// positions xi (default: the current ones, as binned by bin_q): CSR (count pass, scan,
// fill pass) or, when `csr` is false and an earlier build sized the rows, one fill pass
// into fixed-stride rows (ccnt = row counts; `strided` records which).
inline void sph_engine::list_q(bool csr, const double4 *xi) {
  const int n = nlocal, nall = nlocal + nghost;
  const double4 *const xi_src = xi ? xi : xf.p;
  // rhosum/multiphase fused into the fill passes (k_neigh3 RHO): current positions, due now
  const bool rho = mp && !xi && rhofuse_env() && mpc.rhosum_nstep > 0 &&
                   step % mpc.rhosum_nstep == 0;
  SPH_REQUIRE(!mp || (long long)nall < MP_MAXALL, SPH_HIP_EOVERFLOW,
              "multiphase lists index at most 2^28 atoms per rank (%d)", nall);
  if (rho) rho_tmp.reserve(nlocal + nghost);
  rho_fused_step = rho ? step : -1;  // (every path below ends in a fill pass)
  ccnt.reserve(n + 1);
  off.reserve(n + 1);
  auto pass = [&](bool fill, int stride, int *dst = nullptr) {
    if (n == 0) return;
    const bool frho = fill && rho;
    // (mp: xb packs the types, k_bin_copy tpack)
    Neigh3Args a{n, qb, cfg.dim, xi_src, ty.p, xb.p, tb.p, qbeg.p, dc};
    a.cnt = (!fill || stride > 0) ? ccnt.p : nullptr;
    a.off = (fill && stride == 0) ? off.p : nullptr;
    a.nbr = fill ? (dst ? dst : nbr.p) : nullptr;
    a.stride = stride;
    a.ovf = mx.p;
    a.perm_g = stride > 0 ? list_perm_g : 0;
    a.tbits = mp ? 2 : ((stride > 0 && list_tbits) ? 1 : 0);
    if (frho) {
      a.mc = dm;
      a.rm = rm.p;
      a.rho = rho_tmp.p;
    }
    // asymmetric multiphase styles (k_mp_gather): owned pairs take the half-list orientation
    // of the reference's local order, i.e. by tag (k_neigh3 tg); the symmetric gathers
    // never read an owned pair's orientation
    if (mp && !mp2_symmetric(hm)) a.tg = tag.p;
    launch_neigh3<true>(fill, nt1(), mp, frho, s, a);
  };
  mx.reserve(8);
  // single pass into fixed-stride rows when a previous build sized them and nothing
  // needs the CSR form (the setup's half-list pass)
  // (the multiphase passes index rows with 64-bit offsets, MpRow: plain rows, any size)
  const bool sfits = mp ? true : row2_fits((long)nall, (long)n * list_stride);
  bool sover = false;  // the strided fill overflowed: a CSR fill at the same stride would too
  if (!csr && list_stride > 0 && sfits) {
    // rows stored chunk-transposed for the row2 kernels' 16-B index loads; with several
    // types the neighbour's type rides in the entry's top bits
    list_perm_g = (row2_iv() && !mp) ? row2_iv_g() : 0;
    list_tbits = !nt1() && tbits_env() && !mp;
    nbr.reserve((size_t)n * list_stride);
    SPH_HIP_TRY(hipMemsetAsync(mx.p, 0, sizeof(int), s));
    pass(true, list_stride);
    if (read_scalar(mx.p) == 0) {
      strided = true;
      nbr_total = -1;  // entries counted on demand (stats)
      nbr_builds++;
      return;
    }
    sover = true;
  }
  strided = false;
  list_tbits = false;
  // CSR: when an earlier build sized the rows, ONE fill pass into fixed-stride scratch rows
  // (counts as a by-product) compacted into CSR after the scan -- instead of a count pass
  // and a fill pass (the C5 stack rebuilds every step); a row past the stride falls back
  bool filled = false;
  if (!sover && list_stride > 0 && (long)n * list_stride < 0x7fffffffL) {
    list_perm_g = 0;
    nbs.reserve((size_t)n * list_stride);
    SPH_HIP_TRY(hipMemsetAsync(mx.p, 0, sizeof(int), s));
    pass(true, list_stride, nbs.p);
    filled = read_scalar(mx.p) == 0;
  }
  if (!filled) pass(false, 0);
  launch(k_copy_counts, n + 1, n, ccnt.p, off.p);
  cub([&](void *t, size_t &tb) {
    return hipcub::DeviceScan::ExclusiveSum(t, tb, off.p, off.p, n + 1, s);
  });
  if (n > 0)
    cub([&](void *t, size_t &tb) {
      return hipcub::DeviceReduce::Max(t, tb, ccnt.p, mx.p + 1, n, s);
    });
  else SPH_HIP_TRY(hipMemsetAsync(mx.p + 1, 0, sizeof(int), s));
  int hm[2];
  to_host(&hm[0], off.p + n, 1);
  to_host(&hm[1], mx.p + 1, 1);
  SPH_HIP_TRY(hipStreamSynchronize(s));
  const int tot = hm[0];
  SPH_REQUIRE(tot >= 0, SPH_HIP_EOVERFLOW, "neighbor list exceeds 2^31 entries");
  nbr.reserve_min1(tot);
  if (filled) {
    if (n)
      hipLaunchKernelGGL(k_compact_rows, dim3((unsigned)(((long)n * 32 + BLK - 1) / BLK)),
                         dim3(BLK), 0, s, n, list_stride, ccnt.p, off.p, nbs.p, nbr.p);
  } else {
    pass(true, 0);
  }
  // stride of later single-pass builds: this build's longest row + 25% + 16, 64-aligned
  // (whole chunks of the transposed layout, 16-B aligned rows)
  list_stride = ((hm[1] + hm[1] / 4 + 16) + 63) & ~63;
  nbr_maxrow = hm[1];
  nbr_total = tot;
  nbr_builds++;
}

// Block unions + slot rows straight from the bins (k_blk_neigh; bin_q() must have run) in
// the SPH_BLK shape.  The row stride is the last CSR build's (list_stride), doubled if a
// row outgrows it; false (the row path takes over) if a block overflows its LDS image.
inline bool sph_engine::build_blk() {
  const int n = nlocal;
  if (n == 0) return false;
  mx.reserve(10);
  ccnt.reserve(n + 1);
  if (blk_rowcap == 0) blk_rowcap = std::max(list_stride, nbr_maxrow + nbr_maxrow / 4 + 16);
  blk_flags = blk_retry = 0;
  // the SPH_BLK shape, then 32-row blocks (smaller unions), then 32-row blocks with the
  // build's large candidate image, if the blocks do not fit
  const int first = blk_shape_env();
  const int chain[3][2] = {{first, 0}, {1, 0}, {1, 1}};
  for (const auto &c : chain) {
    if (c[0] == 1 && first == 1 && c[1] == 0 && &c != &chain[0]) continue;
    const int r = build_blk_shape(c[0], c[1] != 0);
    if (r == 1) return true;
    if (r != 2) return false;  // (2: a block overflowed: the next, roomier variant)
  }
  return false;
}
// 1 = built, 2 = a block overflowed (candidates, bin table or LDS image), 0 = failed
inline int sph_engine::build_blk_shape(int shape, bool big) {
  const int n = nlocal;
  const BlkShape sh = blk_shape(shape);
  const int chunk = sh.G * sh.U;
  // repeats are counted per cause, so that one cause cannot spend the other's: the small
  // candidate image overflows at most once (the repeat takes BLK_SCAP); the stride is tried
  // at 1x, 2x and 4x the sized row (a third overflow doubles it once more for the next
  // rebuild and this build goes to the row path)
  for (int nrow = 0, nimg = 0; nrow < 3 && nimg < 2;) {
    blk_sstride = (std::max(blk_rowcap, 1) + chunk - 1) / chunk * chunk;
    snbr.reserve((size_t)n * blk_sstride + 2 * chunk);  // + the pair passes' prefetch pad
    const int nb = blk_blocks(n, sh.R);
    ulist.reserve((size_t)nb * BLK_UCAP);
    ucnt.reserve(nb);
    kcnt.reserve(nb);
    SPH_HIP_TRY(hipMemsetAsync(mx.p, 0, 10 * sizeof(int), s));
    // k_blk_build (ballots, inner rows in the same pass); the bitmap walk k_blk_neigh for
    // the large candidate image, with a k_blk_inner pass over the full rows afterwards
    // (build_inner)
    const bool v2 = !big;
    const bool want_inner = inner_margin > 0.0;
    if (want_inner) {
      snbi.reserve((size_t)n * blk_sstride + 2 * chunk);
      icnt.reserve(n);
      uilist.reserve((size_t)nb * BLK_UCAP);
      uicnt.reserve(nb);
    }
    // the inner rows over their own union
    const bool iu = v2 && want_inner;
    BlkBuildArgs a;
    a.n = n;
    a.q = qb;
    a.dim = cfg.dim;
    a.xf = xf.p;
    a.ty = ty.p;
    a.xb = xb.p;
    a.tb = tb.p;
    a.qbeg = qbeg.p;
    a.cf = dc;
    a.ucap = BLK_UCAP;
    a.sstride = blk_sstride;
    a.ulist = ulist.p;
    a.ucnt = ucnt.p;
    a.rcnt = ccnt.p;
    a.snbr = snbr.p;
    a.ovf = mx.p;
    a.umax = mx.p + 1;
    a.cq = blk_cq();
    a.bexp = study_int("SPH_BEXP", 0);
    if (v2) {
      a.icnt = icnt.p;
      a.snbi = snbi.p;
      a.uilist = iu ? uilist.p : nullptr;
      a.uicnt = iu ? uicnt.p : nullptr;
      a.kcnt = kcnt.p;
      a.small = blk_ksmall;
      blk_build(shape, nt1(), want_inner, s, a);
    } else {
      a.xpos = xpos.p;
      blk_neigh(shape, big, nt1(), s, a);
    }
    inner_written = v2 && want_inner;
    // the build's statistics: ONE read-back
    int *const hm = h_small;
    to_host(hm, mx.p, 9);
    SPH_HIP_TRY(hipStreamSynchronize(s));
    if (env_int("SPH_DEBUG", 0))
      fprintf(stderr,
              "[sph] k_blk_neigh shape %d%s n %d rowcap %d: ovf %d union max %d mean %.1f, "
              "candidates max %d mean %.1f\n",
              shape, big ? " (large image)" : "", n, blk_rowcap, hm[0], hm[1], (double)hm[4] / nb, hm[2],
              (double)hm[3] / nb);
    if (hm[0] == (1 << 24)) {  // a block outgrew the small candidate image
      blk_ksmall = false;
      blk_kover++;
      blk_retry |= SPH_STAT_BLK_IMGRETRY;
      nimg++;
      continue;
    }
    if (hm[0] == (1 << 21)) {  // a row outgrew the slot-row stride
      blk_rowcap *= 2;
      blk_retry |= SPH_STAT_BLK_ROWRETRY;
      nrow++;
      continue;
    }
    if (hm[0] != 0) return 2;
    // the rho and inner passes stage the whole largest union (24 B per slot, blk_rho_lds,
    // + their static tables): a union past the CU's 160 KiB takes the next shape or the row
    // path (only the force pass walks windows)
    if (blk_rho_lds(std::max(hm[1], 1), nt1()) + (nt1() ? 0 : sizeof(RhoPair) * NT2) +
            sizeof(double) * sh.R + 1024 > 163840)
      return 2;
    // the next build takes the small candidate image (four workgroups per CU) while this
    // one's largest block fits it (hm[2]: the largest candidate set; the blocks' sets move
    // by a few candidates between rebuilds); after two overflows it stays with the large one
    if (v2) blk_ksmall = blk_kover < 2 && hm[2] <= BLK_SCAP_S - 24;
    // the largest union's force-pass LDS image (+ the static coefficient tables) must fit
    // the CU's 160 KiB
    blk_sh = shape;
    blk_um = std::max(hm[1], 1);
    blk_flags = (shape == 1 ? SPH_STAT_BLK_R32 : 0) | (big ? SPH_STAT_BLK_BIGIMG : 0) |
                (blk_args_pre(sh) ? 0 : SPH_STAT_BLK_NOPRE) | blk_retry;
    // the force pass's LDS image: sized to the union the passes stage (the inner one when
    // the build wrote it), for as many workgroups per CU as fit; larger unions are walked
    // in windows (k_blk_force)
    if (iu)
      blk_umf = choose_umf(hm[7], (double)hm[8] / nb);
    else
      blk_umf = choose_umf(blk_um, (double)hm[4] / nb);
    launch(k_blk_count_big, nb, nb, iu ? uicnt.p : ucnt.p, blk_umf, mx.p + 9);
    if (env_int("SPH_DEBUG", 0))
      fprintf(stderr, "[sph] inner union max %d mean %.1f; force image %d records\n", hm[7],
              (double)hm[8] / nb, blk_umf);
    return 1;
  }
  return 0;
}
// the union image's chunk size / 16 (sph_blk_kernels.h): with the heat term's e array
// or the gas mode's c
inline int sph_engine::blk_cq() const {
  return ((force_mode & (M_HEAT | M_GAS)) ? BLK_CHE : BLK_CH) / 16;
}
// The force pass's LDS image in union records (a multiple of 16) for unions of at most
// maxu records, meanu on average: the whole largest union if it fits three workgroups per
// CU (6 waves per SIMD); else three workgroups' image when the mean union fits it with
// 10 % to spare (the few larger unions walked in windows); else up to two workgroups'
// image.  SPH_TUNE_BLKUMF caps it (tests force the windowed walk that way).
inline int sph_engine::choose_umf(int maxu, double meanu) const {
  const bool one = nt1();
  const int cq = blk_cq();
  const size_t stat = (one ? 0 : (sizeof(TaitPair) + sizeof(HeatPair)) * NT2) + 1024;
  auto fits = [&](int w, int wgs) { return blk_lds(w, cq, one) + stat <= 163840 / wgs; };
  auto cap = [&](int wgs) {
    int w = 16;
    while (w < BLK_UCAP && fits(w + 16, wgs)) w += 16;
    return w;
  };
  const int m16 = std::max(16, (maxu + 15) / 16 * 16);
  int umf;
  if (fits(m16, 3)) umf = m16;
  else if (meanu * 1.10 <= cap(3)) umf = cap(3);
  else umf = std::min(m16, cap(2));
  if (blkumf > 0) umf = std::min(umf, std::max(16, blkumf / 16 * 16));
  return umf;
}
// (BlkArgs::pre of the current stride)
inline bool sph_engine::blk_args_pre(const BlkShape &sh) const {
  BlkArgs k;
  k.sstride = blk_sstride;
  return k.pre(sh);
}
inline BlkArgs sph_engine::blk_args() const {
  BlkArgs k;
  k.cq = blk_cq();
  k.n = nlocal;
  k.shape = blk_sh;
  k.exp = row2_exp();
  k.ucap = BLK_UCAP;
  k.um = blk_um;
  k.umf = blk_umf;
  k.sstride = blk_sstride;
  k.ulist = ulist.p;
  k.ucnt = ucnt.p;
  k.rcnt = ccnt.p;
  k.snbr = snbr.p;
  if (inner) {
    k.snbi = snbi.p;
    k.icnt = icnt.p;
    k.moved = moved_flag();
    k.uilist = uilist.p;
    k.uicnt = uicnt.p;
  }
  return k;
}

// pbc + sort + borders + bins + list(s); `need_csr` also builds the global-index CSR
// list (the setup's half-list pass walks it).  Block path: the block unions + slot rows
// from the bins (no global-index list on a plain rebuild); the row path's strided list
// if a block overflows its LDS image.
inline void sph_engine::build_all(bool need_csr) {
  // (the multiphase passes walk global-index full rows carrying each pair's half-list
  // orientation, k_neigh3: CSR at setup, fixed-stride rows once the setup sized them)
  launch(k_pbc, nlocal, nlocal, box, xf.p, vel.p);
  if (multi()) exchange_multi();
  // Atom::sort between the exchange and borders (verlet.cpp:106, 251): only the LAMMPS
  // indices move -- the rows keep the engine's own order
  if (pc && sortfreq > 0 && step >= nextsort) atom_sort();
  // (at most every sort_every() steps, as atom_modify sort Nevery: the C5 stack rebuilds
  // every step, and its rows keep their locality over a few steps of motion)
  if (cfg.sort && (force_sort || !setup_done || step == 0 || step - last_sort >= sort_every())) {
    sort_owned();
    last_sort = step;
  }
  force_sort = false;
  borders();
  if (cfg.sort) grow_twins();
  bin_q();
  blk = false;
  if (need_csr || !want_blk() || mp) list_q(need_csr);
  if (mp) {
    ov_ready = false;
    return;
  }
  if (want_blk()) {
    blk = build_blk();
    build_inner();
    if (blk && !need_csr) {
      strided = true;  // (ccnt holds the full-list counts; list_entries sums them)
      nbr_total = -1;
      nbr_builds++;
    } else if (!blk && !need_csr) {
      list_q(false);
    }
  }
  ov_ready = false;
  if (overlap_on()) classify_rows();
}

// The block path's inner rows (sph_blk_kernels.h k_blk_inner), written after every block
// build: the pair passes walk them while no atom has moved inner_margin / 2 since (owned
// atoms: checked by the integrate kernels; bricks: the ghosts after each forward comm).
inline void sph_engine::build_inner() {
  inner = blk && inner_margin > 0.0 && nlocal > 0;
  sc.x0 = nullptr;
  if (!inner) return;
  const BlkShape sh = blk_shape(blk_sh);
  snbi.reserve((size_t)nlocal * blk_sstride + 2 * sh.U * sh.G);
  icnt.reserve(nlocal);
  uilist.reserve((size_t)blk_blocks(nlocal, sh.R) * BLK_UCAP);
  uicnt.reserve(blk_blocks(nlocal, sh.R));
  moved.reserve(2);
  const size_t nx0 = (size_t)nlocal + (multi() ? nghost : 0);
  x0.reserve(nx0);
  if (!inner_written)  // (k_blk_inner writes the inner unions too)
    blk_inner(nt1(), s, blk_args(), xf.p, ty.p, dc, snbi.p, icnt.p);
  dev_copy(x0.p, xf.p, nx0);
  SPH_HIP_TRY(hipMemsetAsync(moved.p, 0, 2 * sizeof(int), s));
  sc.x0 = x0.p;
  sc.lim2 = 0.25 * inner_margin * inner_margin;
  sc.moved = moved_flag();
}
// The moved flag of this step (two slots, by step parity: the integrate and the ghost check
// of step k raise slot k & 1 against x0, the passes of step k read it; refresh_inner
// clears the other slot for step k + 1).  Validity of the inner rows depends only on the
// current displacements from x0, so a flag per step, not a sticky one, is exact.
inline int *sph_engine::moved_flag() const { return moved.p ? moved.p + (step & 1) : nullptr; }
// After the passes of a step between rebuilds: if this step's flag is raised, the inner
// rows are derived again from the full rows at the current positions (x0 := them), so the
// next steps walk ~120 instead of ~155 entries per row until the next rebuild; skipped
// when the next step rebuilds anyway.
inline void sph_engine::refresh_inner(bool rebuild_next) {
  if (!inner || !sc.x0 || !refresh_env()) return;
  if (rebuild_next) return;  // (the rebuild clears both slots)
  int *const cur = moved_flag();
  int *const nxt = moved.p + ((step + 1) & 1);
  BlkArgs k = blk_args();
  BlkInnerRefresh rf;
  rf.cond = cur;
  rf.zero = nxt;
  rf.x0 = x0.p;
  blk_inner(nt1(), s, k, xf.p, ty.p, dc, snbi.p, icnt.p, rf);
  if (multi() && nghost)
    launch(k_x0_cond, nghost, nghost, cur, xf.p + nlocal, x0.p + nlocal);
  inner_refreshes++;
}

inline void sph_engine::rebuild() {
  Scope t(this, T_NEIGH);
  build_all(false);
}
// Neighbor::decide's test of a step `ago` steps after the last build (neighbor.cpp:1338)
inline bool sph_engine::neigh_eligible(int64_t ago) const {
  return ago >= nm_delay && ago % neigh_every() == 0;
}
// After a build (setup's included): ago = 0 and, with check yes, xhold = x of the owned
// atoms as the build left them -- wrapped, migrated, sorted (neighbor.cpp:1428-1441); the
// rows keep that order until the next build.  The flag is only ever raised by a check that
// a build follows, so clearing it here keeps it clear for every check.
inline void sph_engine::neigh_built() {
  nm_ago = 0;
  last_build = (int)step;
  nm_builds++;
  if (!nm_check) return;
  xhold.reserve_min1(nlocal);
  nm_flag.reserve(1);
  if (nlocal)
    dev_copy(xhold.p, xf.p, (size_t)nlocal);
  SPH_HIP_TRY(hipMemsetAsync(nm_flag.p, 0, sizeof(int), s));
}
// The check's answer: this brick's flag (one small copy into pinned memory, one stream
// synchronise), over bricks the largest (MPI_Allreduce MAX, neighbor.cpp:1407) -- every
// rank reaches the same eligible steps, a rank without atoms takes part with 0.
inline bool sph_engine::neigh_flag_any() {
  to_host(h_nm, nm_flag.p, 1);
  SPH_HIP_TRY(hipStreamSynchronize(s));
  int flag = nlocal > 0 ? *h_nm : 0;
  if (multi() && tr) {
    std::vector<int> all(tr->size());
    tr->allgather_int(flag, all.data(), s);
    flag = *std::max_element(all.begin(), all.end());
  }
  return flag != 0;
}
