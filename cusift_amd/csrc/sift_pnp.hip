// sift_pnp.hip -- absolute pose on the device: from records that carry coords3D (cusift_lift_depth, cusift_register_pose)
// and matches into an ordinary image to that image's pose [R | t], in the unit coords3D is in, without a host decision.
// The reference has no PnP code: the definition is this library's own, written out in include/cusift_amd_extras.h
// (cusift_estimate_pnp), and all of it is fp64.  cusift_estimate_pnp / cusift_register_pnp enqueue, on the context's
// stream, with no host round trip in between:
//
//   pnp_mark_kernel         pair_mark (sift_ransac_chain.h) with the depth condition (three finite coords3D floats,
//                           coords3D[2] != 0); SoA coordinates [X | Y | Z | x2 | y2] of all records; marks and per-block
//                           counts as planar_compact_kernel reads them
//   planar_compact_kernel   (sift_planar.hip, unchanged) the candidates' record indices in ascending order, their number
//   pnp_solve_kernel        one hypothesis per lane: draw_and_gather (sift_ransac_chain.h: the candidates' coordinates
//                           compacted, six samples drawn from the candidate list), the normalised 11 x 12 DLT system, its
//                           null_vector, denormalisation, the nearest rotation, scale, [R | t]
//   pnp_score_kernel        ransac_score (sift_ransac_chain.h) over the candidates with pnp_inlier; grid (loops / 64,
//                           candidate splits)
//   pnp_select_kernel       one workgroup: the winner (ransac_winner<true>: among equals the first), its inlier flags, the
//                           Gauss-Newton rounds (27 sums and the set's size over the current inliers, a 6 x 6 Cholesky
//                           solve on one lane, Rodrigues), then match_error of every record and the candidates that fit
//
// THE POSE is kept in one form everywhere -- hypotheses, winner, refit, outputs: twelve doubles, row-major [R | t] with
// X1 = R X2 + t, the RGB-D calls' direction.  pnp_inlier() is the one test that the scoring, the flags, the refit's
// membership, num_fit and match_error share, so a host can recount every integer of a call from the doubles it returns.
// THE NULL VECTOR of the 11 x 12 system is null_vector's (sift_ransac_chain.h), the elimination epipolar_solve_kernel
// runs on its 8 x 9 system.  132 doubles and 12 ints per lane: 70,656 bytes of static LDS per one-wave workgroup, two
// workgroups per CU.
// THE REFIT's normal matrix is a sum of 2 x 6 Jacobian outer products: positive definite unless the set is degenerate,
// so one lane's Cholesky needs no pivot search -- 6 square roots and 21 divisions where the epipolar refit runs 288
// Jacobi rotations.  A pivot that is not > 0 (NaN included) keeps the previous pose and ends the refit.  The partial
// sums are reduced in a fixed order (wave_tree_sum of sift_ransac.h), so every run gives the same bits.
// A PAIR LIST (cusift_register_pnp_batch).  The solve, scoring and selection kernels have a pair index, blockIdx.z, and
// PlanarBatch's strides like every kernel of sift_epipolar.hip: pair p's arrays lie the strides further, it draws from
// seed + p, and its record count is what sequence_pnp_mark_kernel (sift_sequence.hip, in pnp_mark_kernel's place) left
// in its head; num_pts is then the capacity of a pair.  One pair is gridDim.z == 1 with every stride 0.  A batch's
// pnp_select_kernel writes match_error to an array of its own: the records are read only.
// Kernels use no scratch memory and write with vector stores only.
#include "sift_epipolar.h"
#include "sift_ransac_chain.h"

namespace cusift {

constexpr int kPnPThreads = 256;  // mark / select
constexpr int kPnPTile = 64;      // hypotheses per workgroup of the solve and scoring kernels, candidates per LDS tile
static_assert(kPnPTile == kRansacTile && kPnPThreads == kRansacThreads, "the shared bodies' geometry");
constexpr int kPnPRows = 11, kPnPCols = 12;
constexpr int kPnPSums = 28;      // 21 of J^T J, 6 of J^T r, the size of the set

// The inlier test, in exactly the expressions of include/cusift_amd_extras.h: no division, no root.  xs = x2 - px and
// ys = y2 - py.  *e2 and *den leave for match_error.  A NaN fails; a point that is not in front of the camera fails.
__device__ __forceinline__ bool pnp_inlier(const double (&rt)[12], PnPCam k, double X, double Y, double Z, double xs,
                                           double ys, double t2, double *e2 = nullptr, double *den_out = nullptr,
                                           double *abc = nullptr) {
  const double dx = X - rt[3], dy = Y - rt[7], dz = Z - rt[11];
  const double a = (rt[0] * dx + rt[4] * dy) + rt[8] * dz;
  const double b = (rt[1] * dx + rt[5] * dy) + rt[9] * dz;
  const double c = (rt[2] * dx + rt[6] * dy) + rt[10] * dz;
  const double ex = k.fx * a - xs * c;
  const double ey = k.fy * b - ys * c;
  const double err = ex * ex + ey * ey, den = c * c;
  if (e2) *e2 = err;
  if (den_out) *den_out = den;
  if (abc) abc[0] = a, abc[1] = b, abc[2] = c;
  return c > 0.0 && err < t2 * den;
}

// From the 3 x 4 matrix p (row-major, det of its left block > 0) to [R | t]: R21 the rotation nearest the left block M,
// t21 = p4 / scale, then the returned direction.  false: something is not finite, rt is twelve zeros.
__device__ __forceinline__ bool pnp_finish(const double (&p)[12], double (&rt)[12]) {
  double g[3][3], v[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = i; j < 3; ++j) g[i][j] = (p[i] * p[j] + p[4 + i] * p[4 + j]) + p[8 + i] * p[8 + j];
  epipolar_jacobi<3>(g, v, kEpiSweeps3);
  // the eigenpairs in descending order, the first among equals
  const double l0 = g[0][0], l1 = g[1][1], l2 = g[2][2];
  int i1 = 0;
  i1 = l1 > pick3(i1, l0, l1, l2) ? 1 : i1;
  i1 = l2 > pick3(i1, l0, l1, l2) ? 2 : i1;
  const int ia = i1 == 0 ? 1 : 0, ib = i1 == 2 ? 1 : 2;  // the other two, ascending
  const int i2 = pick3(ib, l0, l1, l2) > pick3(ia, l0, l1, l2) ? ib : ia;
  const double lam1 = pick3(i1, l0, l1, l2), lam2 = pick3(i2, l0, l1, l2);
  const double s1 = sqrt(lam1 > 0.0 ? lam1 : 0.0), s2 = sqrt(lam2 > 0.0 ? lam2 : 0.0);
  double v1[3], v2[3], v3[3], u1[3], u2[3], u3[3], w[3], mv3[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) v1[r] = pick3(i1, v[r][0], v[r][1], v[r][2]), v2[r] = pick3(i2, v[r][0], v[r][1], v[r][2]);
  v3[0] = v1[1] * v2[2] - v1[2] * v2[1];
  v3[1] = v1[2] * v2[0] - v1[0] * v2[2];
  v3[2] = v1[0] * v2[1] - v1[1] * v2[0];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    u1[r] = ((p[4 * r] * v1[0] + p[4 * r + 1] * v1[1]) + p[4 * r + 2] * v1[2]) / s1;
    w[r] = (p[4 * r] * v2[0] + p[4 * r + 1] * v2[1]) + p[4 * r + 2] * v2[2];
    mv3[r] = (p[4 * r] * v3[0] + p[4 * r + 1] * v3[1]) + p[4 * r + 2] * v3[2];
  }
  const double d = (w[0] * u1[0] + w[1] * u1[1]) + w[2] * u1[2];
#pragma unroll
  for (int r = 0; r < 3; ++r) w[r] = w[r] - d * u1[r];
  const double nw = sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]);
#pragma unroll
  for (int r = 0; r < 3; ++r) u2[r] = w[r] / nw;
  u3[0] = u1[1] * u2[2] - u1[2] * u2[1];
  u3[1] = u1[2] * u2[0] - u1[0] * u2[2];
  u3[2] = u1[0] * u2[1] - u1[1] * u2[0];
  const double s3 = fabs((u3[0] * mv3[0] + u3[1] * mv3[1]) + u3[2] * mv3[2]);
  const double scale = ((s1 + s2) + s3) / 3.0;
  double R21[9], t21[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) R21[3 * i + j] = (u1[i] * v1[j] + u2[i] * v2[j]) + u3[i] * v3[j];
    t21[i] = p[4 * i + 3] / scale;
  }
  // X1 = R X2 + t: R = R21^T, t = -R21^T t21
  double out[12];
  bool ok = scale > 0.0;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) out[4 * r + c] = R21[3 * c + r];
    out[4 * r + 3] = -((R21[r] * t21[0] + R21[3 + r] * t21[1]) + R21[6 + r] * t21[2]);
  }
#pragma unroll
  for (int i = 0; i < 12; ++i) ok = ok && finite_d(out[i]);
#pragma unroll
  for (int i = 0; i < 12; ++i) rt[i] = ok ? out[i] : 0.0;
  return ok;
}

// coord [5][num_pts] = [X | Y | Z | x2 | y2], marks, block_counts: pair_mark<true> (sift_ransac_chain.h), planar_mark_kernel's
// body plus the depth condition.
__global__ void __launch_bounds__(kPnPThreads) pnp_mark_kernel(const cusift_point *__restrict__ pts, int num_pts,
                                                               int num_pts2, int rule, float lo, float hi,
                                                               float *__restrict__ coord,
                                                               unsigned char *__restrict__ marks,
                                                               int *__restrict__ block_counts,
                                                               const cusift_point *__restrict__ pts2) {
  __shared__ int s_wave[kPnPThreads / 64];
  pair_mark<true>(pts, num_pts, num_pts2, rule, lo, hi, coord, marks, block_counts, PlanarBatch{}, pts2, s_wave);
}

// drawn [6][num_loops] (record indices), pose [12][num_loops], counts [num_loops] (zeroed here for the scoring kernel),
// ccoord [5][num_pts]: the coordinates of candidate k at column k.  Fewer than 6 candidates: nothing is done.
__global__ void __launch_bounds__(kPnPTile) pnp_solve_kernel(const float *__restrict__ coord, int num_pts,
                                                             const int *__restrict__ cand,
                                                             const int *__restrict__ head, unsigned long long seed,
                                                             int num_loops, PnPCam cam, int *__restrict__ drawn,
                                                             double *__restrict__ pose, int *__restrict__ counts,
                                                             float *__restrict__ ccoord, PlanarBatch nb) {
  __shared__ double s_m[kPnPRows * kPnPCols * kPnPTile];  // the 11 x 12 system, one column of the array per lane
  __shared__ int s_col[kPnPCols * kPnPTile];              // the column permutation of the pivoting
  int idx, rec[6];
  if (!draw_and_gather<6, 5>(coord, num_pts, cand, head, seed, num_loops, drawn, pose, counts, ccoord, nb, idx, rec)) return;
  double X[6], Y[6], Z[6], u[6], v[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    const int r = rec[i];
    X[i] = (double)coord[r], Y[i] = (double)coord[(size_t)num_pts + r], Z[i] = (double)coord[2 * (size_t)num_pts + r];
    u[i] = ((double)coord[3 * (size_t)num_pts + r] - cam.px) / cam.fx;
    v[i] = ((double)coord[4 * (size_t)num_pts + r] - cam.py) / cam.fy;
  }
  // the 3-D samples: centroid to 0, mean distance sqrt(3)
  double cx, cy, cz, s;
  {
    double sx = 0.0, sy = 0.0, sz = 0.0;
#pragma unroll
    for (int i = 0; i < 6; ++i) sx += X[i], sy += Y[i], sz += Z[i];
    cx = sx / 6.0, cy = sy / 6.0, cz = sz / 6.0;
    double d = 0.0;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      const double ax = X[i] - cx, ay = Y[i] - cy, az = Z[i] - cz;
      d += sqrt((ax * ax + ay * ay) + az * az);
    }
    s = sqrt(3.0) / (d / 6.0);
  }
  const LaneSystem<kPnPCols> M{s_m, (int)threadIdx.x};
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    const double xn = (X[i] - cx) * s, yn = (Y[i] - cy) * s, zn = (Z[i] - cz) * s;
    M(2 * i, 0) = xn, M(2 * i, 1) = yn, M(2 * i, 2) = zn, M(2 * i, 3) = 1.0;
    M(2 * i, 4) = 0.0, M(2 * i, 5) = 0.0, M(2 * i, 6) = 0.0, M(2 * i, 7) = 0.0;
    M(2 * i, 8) = -(u[i] * xn), M(2 * i, 9) = -(u[i] * yn), M(2 * i, 10) = -(u[i] * zn), M(2 * i, 11) = -u[i];
    if (i < 5) {  // static: the v row of the sixth sample is not used
      M(2 * i + 1, 0) = 0.0, M(2 * i + 1, 1) = 0.0, M(2 * i + 1, 2) = 0.0, M(2 * i + 1, 3) = 0.0;
      M(2 * i + 1, 4) = xn, M(2 * i + 1, 5) = yn, M(2 * i + 1, 6) = zn, M(2 * i + 1, 7) = 1.0;
      M(2 * i + 1, 8) = -(v[i] * xn), M(2 * i + 1, 9) = -(v[i] * yn), M(2 * i + 1, 10) = -(v[i] * zn);
      M(2 * i + 1, 11) = -v[i];
    }
  }
  double ph[12];
  null_vector<kPnPRows, kPnPCols>(M, s_col, ph);
  // denormalise: P = P^ T with T = [s I | -s c; 0 0 0 1]
  const double tx3 = -(s * cx), ty3 = -(s * cy), tz3 = -(s * cz);
  double P[12];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    P[4 * i] = ph[4 * i] * s, P[4 * i + 1] = ph[4 * i + 1] * s, P[4 * i + 2] = ph[4 * i + 2] * s;
    P[4 * i + 3] = ((ph[4 * i] * tx3 + ph[4 * i + 1] * ty3) + ph[4 * i + 2] * tz3) + ph[4 * i + 3];
  }
  // the sign: det of the left block > 0
  const double det = (P[0] * (P[5] * P[10] - P[6] * P[9]) - P[1] * (P[4] * P[10] - P[6] * P[8])) +
                     P[2] * (P[4] * P[9] - P[5] * P[8]);
#pragma unroll
  for (int i = 0; i < 12; ++i) P[i] = det < 0.0 ? -P[i] : P[i];
  double rt[12];
  pnp_finish(P, rt);
#pragma unroll
  for (int i = 0; i < 12; ++i) pose[(size_t)i * num_loops + idx] = rt[i];
}

// ransac_score's model (sift_ransac_chain.h): 12 doubles per hypothesis, counted over the candidates; the pixel rows are
// staged with the principal point taken off, as pnp_inlier wants them.
struct PnPScore {
  static constexpr int kValues = 12, kRows = 5, kMin = 6, kUnroll = 4;
  static constexpr bool kCandidates = true;
  typedef double value_t;
  PnPCam cam;
  double t2;
  __device__ __forceinline__ void stage(double (*s_pt)[kPnPTile], const float *__restrict__ ccoord, int num_pts, int tile,
                                        int tx) const {
    stage_rows<3>(s_pt, ccoord, num_pts, tile, tx);
    s_pt[3][tx] = (double)ccoord[3 * (size_t)num_pts + tile + tx] - cam.px;
    s_pt[4][tx] = (double)ccoord[4 * (size_t)num_pts + tile + tx] - cam.py;
  }
  __device__ __forceinline__ bool inlier(const double (&rt)[12], const double (*p)[kPnPTile], int j) const {
    return pnp_inlier(rt, cam, p[0][j], p[1][j], p[2][j], p[3][j], p[4][j], t2);
  }
};

__global__ void __launch_bounds__(kPnPTile) pnp_score_kernel(const float *__restrict__ ccoord, int num_pts, int per_split,
                                                             const double *__restrict__ pose, int num_loops, PnPCam cam,
                                                             float thresh, int *__restrict__ counts,
                                                             const int *__restrict__ head, PlanarBatch nb) {
  __shared__ double s_pt[5][kPnPTile];
  ransac_score(PnPScore{cam, (double)thresh * (double)thresh}, ccoord, num_pts, per_split, pose, num_loops, counts, head, nb,
               s_pt);
}

// Solves the 6 x 6 system A p = -g from the 27 sums (A's upper triangle row by row, then g) by cholesky_lower.
// false: a pivot is not > 0 (NaN included) or the step is not finite.
__device__ __forceinline__ bool pnp_step(const double *s_sum, double (&p)[6]) {
  double A[6][6], g[6];
  int q = 0;
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int j = i; j < 6; ++j) A[j][i] = s_sum[q++];  // the lower triangle holds A
#pragma unroll
  for (int i = 0; i < 6; ++i) g[i] = -s_sum[21 + i];
  bool ok = cholesky_lower<6>(A, g, p);
#pragma unroll
  for (int i = 0; i < 6; ++i) ok = ok && finite_d(p[i]);
  return ok;
}

// R <- R exp([w]x)^T, t <- t - R d: the left increment (w, d) of X2 = R21 X1 + t21 in the returned direction.
__device__ __forceinline__ bool pnp_update(const double (&p)[6], const double (&rt)[12], double (&out)[12]) {
  double E[3][3];
  rodrigues_exp(p[0], p[1], p[2], E);
  bool ok = true;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) out[4 * i + j] = (rt[4 * i] * E[j][0] + rt[4 * i + 1] * E[j][1]) + rt[4 * i + 2] * E[j][2];
    out[4 * i + 3] = rt[4 * i + 3] - ((out[4 * i] * p[3] + out[4 * i + 1] * p[4]) + out[4 * i + 2] * p[5]);
  }
#pragma unroll
  for (int i = 0; i < 12; ++i) ok = ok && finite_d(out[i]);
  return ok;
}

// head: words kPlanarHeadCand .. kPlanarHeadLoop as the planar head's (planar_compact_kernel writes the first); then as
// doubles [R | t] refined at kPnPHeadRt and the winner's at kPnPHeadWin.  Fewer than 6 candidates, or a winner that counts
// nothing: the counts are 0 and the records stay as they are; the host reports the degenerate answer.  errors == NULL:
// match_error goes into the records; otherwise into errors[] (a batch, whose records stay as they are).
__global__ void __launch_bounds__(kPnPThreads) pnp_select_kernel(cusift_point *__restrict__ pts, int num_pts,
                                                                 const float *__restrict__ coord,
                                                                 const float *__restrict__ ccoord,
                                                                 const unsigned char *__restrict__ marks,
                                                                 const double *__restrict__ pose,
                                                                 const int *__restrict__ counts, int num_loops,
                                                                 PnPCam cam, float thresh, int refine_loops,
                                                                 float refine_thresh, int *__restrict__ head,
                                                                 char *__restrict__ flags, float *__restrict__ errors,
                                                                 PlanarBatch nb) {
  __shared__ unsigned long long s_key[kPnPThreads];
  __shared__ double s_part[kPnPThreads / 64][kPnPSums];
  __shared__ double s_sum[kPnPSums];
  __shared__ double s_rt[12];
  __shared__ int s_ok;
  __shared__ int s_cnt[kPnPThreads];
  pts += (size_t)blockIdx.z * nb.records;
  coord = pair_ptr(coord, nb.scratch), ccoord = pair_ptr(ccoord, nb.scratch);
  marks = pair_ptr(marks, nb.scratch), pose = pair_ptr(pose, nb.scratch);
  counts = pair_ptr(counts, nb.scratch), head = pair_ptr(head, nb.head);
  flags += (size_t)blockIdx.z * nb.flags;
  if (errors) errors += (size_t)blockIdx.z * nb.flags;
  const float *__restrict__ kX = ccoord, *__restrict__ kY = ccoord + num_pts, *__restrict__ kZ = ccoord + 2 * (size_t)num_pts;
  const float *__restrict__ kx2 = ccoord + 3 * (size_t)num_pts, *__restrict__ ky2 = ccoord + 4 * (size_t)num_pts;
  const int tx = threadIdx.x;
  double *dhead = (double *)head;
  const int n = pair_count(head, num_pts, nb);
  const int n_cand = min(head[kPlanarHeadCand], n);
  int best = 0, best_count = 0;
  if (n_cand >= 6) ransac_winner<true>(counts, num_loops, s_key, best, best_count);  // uniform
  if (best_count == 0) {  // uniform: no inlier, the records stay as they are
    for (int i = tx; i < n; i += kPnPThreads) flags[i] = 0;
    if (tx < 12) dhead[kPnPHeadRt + tx] = 0.0, dhead[kPnPHeadWin + tx] = 0.0;
    if (tx >= kPlanarHeadMatches && tx <= kPlanarHeadLoop) head[tx] = 0;
    return;
  }
  // The current pose travels through LDS, the winner first: read from there it lives in vector registers, where there
  // is room; as 24 scalar registers next to the camera and the pointers it would spill.
  if (tx < 12) s_rt[tx] = pose[(size_t)tx * num_loops + best];
  __syncthreads();
  double rt[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) rt[i] = s_rt[i];
  const double t2 = (double)thresh * (double)thresh, rt2 = (double)refine_thresh * (double)refine_thresh;
  for (int i = tx; i < n; i += kPnPThreads)  // a record that is no candidate is no inlier
    flags[i] = (marks[i] & 1) && pnp_inlier(rt, cam, (double)coord[i], (double)coord[(size_t)num_pts + i],
                                            (double)coord[2 * (size_t)num_pts + i],
                                            (double)coord[3 * (size_t)num_pts + i] - cam.px,
                                            (double)coord[4 * (size_t)num_pts + i] - cam.py, t2)
                   ? 1
                   : 0;
  // ---- the refit: thread tx owns candidates tx, tx + 256, ... ----
#pragma unroll 1
  for (int round = 0; round < refine_loops; ++round) {
    double s[kPnPSums];
#pragma unroll
    for (int q = 0; q < kPnPSums; ++q) s[q] = 0.0;
    for (int k = tx; k < n_cand; k += kPnPThreads) {
      const double xs = (double)kx2[k] - cam.px, ys = (double)ky2[k] - cam.py;
      double abc[3];
      if (!pnp_inlier(rt, cam, (double)kX[k], (double)kY[k], (double)kZ[k], xs, ys, rt2, nullptr, nullptr, abc)) continue;
      const double a = abc[0], b = abc[1], c = abc[2];
      const double ic = 1.0 / c, ua = a * ic, vb = b * ic;
      const double g0 = cam.fx * ic, g2 = -(g0 * ua), h1 = cam.fy * ic, h2 = -(h1 * vb);
      const double ru = cam.fx * ua - xs, rv = cam.fy * vb - ys;
      const double ju[6] = {g2 * b, g0 * c - g2 * a, -(g0 * b), g0, 0.0, g2};
      const double jv[6] = {h2 * b - h1 * c, -(h2 * a), h1 * a, 0.0, h1, h2};
      int q = 0;
#pragma unroll
      for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = i; j < 6; ++j) s[q++] += ju[i] * ju[j] + jv[i] * jv[j];
#pragma unroll
      for (int i = 0; i < 6; ++i) s[21 + i] += ju[i] * ru + jv[i] * rv;
      s[27] += 1.0;
    }
    wave_tree_sum<kPnPSums>(s, s_part, s_sum, tx);
    if (s_sum[27] < 6.0) break;  // uniform: keep the pose
    if (tx == 0) {  // one lane solves, everybody reads the answer
      double p[6], out[12];
      const bool ok = pnp_step(s_sum, p) && pnp_update(p, rt, out);
#pragma unroll
      for (int i = 0; i < 12; ++i) s_rt[i] = out[i];
      s_ok = ok ? 1 : 0;
    }
    __syncthreads();
    if (!s_ok) break;  // uniform: a step that is not finite keeps the previous pose and ends the refit
#pragma unroll
    for (int i = 0; i < 12; ++i) rt[i] = s_rt[i];
  }
  // ---- match_error of every record, the number of candidates that fit ----
  for (int i = tx; i < n; i += kPnPThreads) {
    double e2, den, abc[3];
    pnp_inlier(rt, cam, (double)coord[i], (double)coord[(size_t)num_pts + i], (double)coord[2 * (size_t)num_pts + i],
               (double)coord[3 * (size_t)num_pts + i] - cam.px, (double)coord[4 * (size_t)num_pts + i] - cam.py, rt2, &e2,
               &den, abc);
    const float err = abc[2] > 0.0 ? (float)sqrt(e2 / den) : __builtin_nanf("");
    if (errors)
      errors[i] = err;
    else
      pts[i].match_error = err;
  }
  int fit = 0;
#pragma unroll 1  // unrolled 16 times the loop's addresses and masks spill scalar registers
  for (int k = tx; k < n_cand; k += kPnPThreads)
    fit += pnp_inlier(rt, cam, (double)kX[k], (double)kY[k], (double)kZ[k], (double)kx2[k] - cam.px,
                      (double)ky2[k] - cam.py, rt2)
               ? 1
               : 0;
  fit = block_sum_256(fit, s_cnt);
  if (tx == 0) {
#pragma unroll
    for (int i = 0; i < 12; ++i) {
      dhead[kPnPHeadRt + i] = rt[i];
      dhead[kPnPHeadWin + i] = pose[(size_t)i * num_loops + best];
    }
    head[kPlanarHeadMatches] = best_count;
    head[kPlanarHeadFit] = fit;
    head[kPlanarHeadLoop] = best;
  }
}

}  // namespace cusift
