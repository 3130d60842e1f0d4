// sph_bins.h -- the bin grids of the neighbour builds as the kernels take them, and the host
// arithmetic that fills them.  Plain C++: no HIP, a host compiler builds it alone.
#pragma once

namespace sph {

// nb bins per axis from lo, inv = bins per length (k_bin_keys, k_cs_hist)
struct Bins {
  double lo[3];
  double inv[3];
  int nb[3];
};

// the list builders' bins of at least cutneighmax / 2 (k_neigh3, k_blk_build: reach 2)
struct QBins {
  double lo[3], inv[3], size[3];
  int nb[3];
  double cutmaxsq;
};

// q, and the same grid as the Bins b that the binned copy's keys take, from nb bins over
// [lo, lo + ext) per axis; an axis at or past dim is one bin that every coordinate falls into
inline void fill_qbins(QBins &q, Bins &b, const double lo[3], const double ext[3],
                       const int nb[3], int dim, double cutmaxsq) {
  for (int k = 0; k < 3; k++) {
    const bool act = k < dim;
    q.lo[k] = b.lo[k] = lo[k];
    q.nb[k] = b.nb[k] = act ? nb[k] : 1;
    q.inv[k] = b.inv[k] = act ? nb[k] / ext[k] : 0.0;
    q.size[k] = act ? ext[k] / nb[k] : 1.0;
  }
  q.cutmaxsq = cutmaxsq;
}

// bits of a radix sort over the keys [0, nkeys)
inline int key_bits(int nkeys) {
  int bits = 1;
  while ((1u << bits) < (unsigned)nkeys && bits < 32) bits++;
  return bits;
}

}  // namespace sph
