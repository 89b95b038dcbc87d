// Linear prediction in double for one lane (composite.hip, spectral.hip): R in registers or in LDS.
#pragma once
#include "fsem_common.h"

namespace fsem {

// Prediction-error filter a = [1, a_1 .. a_P] of R by Levinson-Durbin (R[0] == 0: NaN by 0 / 0).
template <int P>
__device__ __forceinline__ void levinson(const double *R, double a[P + 1]) {
  a[0] = 1.0;
#pragma unroll
  for (int i = 1; i <= P; ++i) a[i] = 0.0;
  double E = R[0];
#pragma unroll
  for (int i = 1; i <= P; ++i) {
    double acc = R[i];
#pragma unroll
    for (int j = 1; j < i; ++j) acc = fma(a[j], R[i - j], acc);
    const double k = -acc / E;
#pragma unroll
    for (int j = 1; 2 * j <= i; ++j) {
      const double u = a[j], v = a[i - j];
      a[j] = fma(k, v, u);
      if (j != i - j) a[i - j] = fma(k, u, v);
    }
    a[i] = k;
    E *= 1.0 - k * k;
  }
}

// a Toeplitz(R) a^T = R[0] sum a_i^2 + 2 sum_k R[k] sum_i a_i a_{i+k}.
template <int P>
__device__ __forceinline__ double quadratic(const double a[P + 1], const double *R) {
  double q = 0.0;
#pragma unroll
  for (int k = P; k >= 0; --k) {
    double c = 0.0;
#pragma unroll
    for (int i = 0; i + k <= P; ++i) c = fma(a[i], a[i + k], c);
    q = fma(k ? 2.0 * c : c, R[k], q);
  }
  return q;
}

}  // namespace fsem
