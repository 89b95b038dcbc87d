// The SI-SDR / SNR case analysis of one (reference, estimate) pair from its sums over the row, in
// double: what sdr_finish (sdr.hip) scores a row by and pit_finish / pit_grad (pitsdr.hip) every
// (source, estimate) pair of a mixture.
#pragma once
#include "fsem_common.h"

namespace fsem {

// The scores, and the (centred, with zero_mean) sums the SI-SDR's gradient needs.
struct PairScores {
  double si, snr, ss, sh, nn;
};
// ss = sum s^2, hh = sum h^2, sh = sum s h, dd = sum (h - s)^2, s1 = sum s, h1 = sum h over the
// row's n samples (all finite).  SNR = 10 log10(ss / dd): 0 / 0 is NaN, x / 0 +inf, 0 / x -inf.
// SI-SDR, after removing the means with zero_mean: NaN when either signal has no energy, +inf
// when the estimate equals the reference, else 10 log10(|target|^2 / |noise|^2) with the target
// (sh / ss) s.
__device__ __forceinline__ PairScores pair_scores(double ss, double hh, double sh, double dd, double s1, double h1,
                                                  int n, int zero_mean) {
  PairScores p;
  p.snr = 10.0 * log10(ss / dd);
  if (zero_mean) {
    ss = fmax(ss - s1 * s1 / n, 0.0);
    sh = sh - s1 * h1 / n;
    hh = fmax(hh - h1 * h1 / n, 0.0);
  }
  p.ss = ss, p.sh = sh, p.nn = 0.0;
  if (ss == 0.0 || hh == 0.0) {
    p.si = __builtin_nan("");
  } else if (dd == 0.0) {
    p.si = __builtin_inf();
  } else {
    const double tt = sh / ss * sh;
    p.nn = fmax(hh - tt, 0.0);
    p.si = 10.0 * log10(tt / p.nn);
  }
  return p;
}

}  // namespace fsem
