// sift_epipolar.h -- the device helpers that sift_epipolar.hip and sift_pose.hip share: the pinned Sampson test and the
// static-index cyclic Jacobi (sift_pnp.hip takes the Jacobi).  Inline functions only; every expression here is pinned bit for bit by tests/test_epipolar.py.
#pragma once

#include "sift_ransac.h"

namespace cusift {

// Cyclic Jacobi converges quadratically: on the refit matrices of planted scenes of 12 to 3,300 records (float64 numpy
// restatement) the eigenvector stops moving after 6 sweeps of the 9 x 9 matrix; two more are the margin.
constexpr int kEpiSweeps9 = 8, kEpiSweeps3 = 8;

// The inlier test: the Sampson distance without a division or a root, in exactly the expressions of
// include/cusift_amd_extras.h.  *e2 and *den leave for match_error.  A NaN or den == 0 is no inlier.
__device__ __forceinline__ bool epipolar_inlier(const double (&F)[9], double x1, double y1, double x2, double y2,
                                                double t2, double *e2 = nullptr, double *den_out = nullptr) {
  const double l0 = (F[0] * x1 + F[1] * y1) + F[2];
  const double l1 = (F[3] * x1 + F[4] * y1) + F[5];
  const double l2 = (F[6] * x1 + F[7] * y1) + F[8];
  const double m0 = (F[0] * x2 + F[3] * y2) + F[6];
  const double m1 = (F[1] * x2 + F[4] * y2) + F[7];
  const double e = (x2 * l0 + y2 * l1) + l2;
  const double den = ((l0 * l0 + l1 * l1) + m0 * m0) + m1 * m1;
  if (e2) *e2 = e * e;
  if (den_out) *den_out = den;
  return e * e < t2 * den;
}

// Entry (i, j) of a symmetric matrix kept in its upper triangle.
#define EPI_SYM(a, i, j) a[(i) < (j) ? (i) : (j)][(i) < (j) ? (j) : (i)]

// Cyclic Jacobi on the symmetric N x N matrix `a` (upper triangle used): `sweeps` sweeps over the pairs (p, q), p < q, in
// row-major order, whatever the data.  Afterwards a[j][j] are the eigenvalues and column j of v the eigenvectors.  Every
// index is static; a pair whose off-diagonal entry is 0 is rotated by the identity.
template <int N>
__device__ __forceinline__ void epipolar_jacobi(double (&a)[N][N], double (&v)[N][N], int sweeps) {
#pragma unroll
  for (int i = 0; i < N; ++i)
#pragma unroll
    for (int j = 0; j < N; ++j) v[i][j] = i == j ? 1.0 : 0.0;
#pragma unroll 1
  for (int sw = 0; sw < sweeps; ++sw) {
#pragma unroll
    for (int p = 0; p < N - 1; ++p)
#pragma unroll
      for (int q = p + 1; q < N; ++q) {
        const double apq = a[p][q];
        const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
        double t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
        t = theta < 0.0 ? -t : t;
        t = apq == 0.0 ? 0.0 : t;
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
        a[p][p] -= t * apq;
        a[q][q] += t * apq;
        a[p][q] = 0.0;
#pragma unroll
        for (int k = 0; k < N; ++k) {
          if (k != p && k != q) {
            const double akp = EPI_SYM(a, k, p), akq = EPI_SYM(a, k, q);
            EPI_SYM(a, k, p) = c * akp - s * akq;
            EPI_SYM(a, k, q) = s * akp + c * akq;
          }
          const double vkp = v[k][p], vkq = v[k][q];
          v[k][p] = c * vkp - s * vkq;
          v[k][q] = s * vkp + c * vkq;
        }
      }
  }
}

}  // namespace cusift
