// sift_pose.hip -- calibrated two-view pose on the device: the stage behind epipolar_select_kernel.  From a fundamental
// matrix and the two cameras' intrinsics to [R | t] and a triangulated point in coords3D of every record, without a host
// decision.  The definition is this library's own, written out in include/cusift_amd_extras.h (cusift_estimate_pose), and
// all of it is fp64.  cusift_estimate_pose / cusift_register_pose enqueue, on the context's stream:
//
//   pose_vote_kernel    one record per lane.  Every lane derives the essential matrix and its four (R21, t21) candidates
//                       from F itself -- uniform work in registers with static indices, 24 Jacobi rotations, cheaper than
//                       a broadcast through memory and a launch of its own -- then, for a record of the fit set, solves the
//                       two depths under each candidate.  The four counts of a workgroup (ballot + popcount per wave,
//                       waves ((0 + 1) + 2) + 3) meet in four integer atomic adds on the pose head, zeroed before
//   pose_write_kernel   the same grid: the winner from the four integers (among equals the first), the record's depths
//                       under it again, coords3D of EVERY record in [0, n); workgroup 0 writes [R | t], sigma and
//                       num_front into the pose head
// F comes from the epipolar head (kEpiHeadF): epipolar_select_kernel left it there, or the staged call uploaded it.  The
// kernels read the SoA coordinates and the mark bytes of the marking kernel, never the 588-byte records, and write three
// floats per record.  Both have a pair index, blockIdx.z, and PlanarBatch's strides like every kernel of sift_epipolar.hip;
// the pose heads of a batch are kPoseHeadBytes apart.  cusift_register_pose_batch launches both with one grid layer per
// pair of its list behind the batched epipolar selection; its triangulated points go to an array, not into the records.
// No scratch memory, 64 bytes of LDS, vector stores only.
// COST (profiles/pose.json): 10 us and 11 us at 4,096 and at 32,768 records alike -- the decomposition's chain of fp64
// divisions and square roots, which every lane walks once per launch; together 2.6 % and 1.5 % of epipolar_select_kernel.
#include "sift_epipolar.h"

namespace cusift {

constexpr int kPoseThreads = 256;

// The decomposition of E = K2^T (F K1): R[0] = U W V^T, R[1] = U W^T V^T (row-major R21), t = u3, the singular values.
// The four candidates are (R[0], +t), (R[0], -t), (R[1], +t), (R[1], -t).  ok == false: a degenerate answer.
struct PoseFrame {
  double R[2][9], t[3], sigma[3];
  bool ok;
};

__device__ __forceinline__ void pose_decompose(const double (&F)[9], const PoseCams &k, PoseFrame &p) {
  bool any = false, fin = true;
#pragma unroll
  for (int i = 0; i < 9; ++i) any = any || F[i] != 0.0, fin = fin && finite_d(F[i]);
  // A = F K1, E = K2^T A
  double A[3][3], E[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    A[i][0] = F[3 * i] * k.fx1;
    A[i][1] = F[3 * i + 1] * k.fy1;
    A[i][2] = (F[3 * i] * k.px1 + F[3 * i + 1] * k.py1) + F[3 * i + 2];
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    E[0][j] = k.fx2 * A[0][j];
    E[1][j] = k.fy2 * A[1][j];
    E[2][j] = (k.px2 * A[0][j] + k.py2 * A[1][j]) + A[2][j];
  }
  // G = E^T E, its eigenpairs in descending order, the first among equals
  double g[3][3], v[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = i; j < 3; ++j) g[i][j] = (E[0][i] * E[0][j] + E[1][i] * E[1][j]) + E[2][i] * E[2][j];
  epipolar_jacobi<3>(g, v, kEpiSweeps3);
  const double l0 = g[0][0], l1 = g[1][1], l2 = g[2][2];
  int i1 = 0;
  i1 = l1 > pick3(i1, l0, l1, l2) ? 1 : i1;
  i1 = l2 > pick3(i1, l0, l1, l2) ? 2 : i1;
  const int ia = i1 == 0 ? 1 : 0, ib = i1 == 2 ? 1 : 2;  // the other two, ascending
  const int i2 = pick3(ib, l0, l1, l2) > pick3(ia, l0, l1, l2) ? ib : ia;
  const int i3 = 3 - i1 - i2;
  const double lam[3] = {pick3(i1, l0, l1, l2), pick3(i2, l0, l1, l2), pick3(i3, l0, l1, l2)};
#pragma unroll
  for (int i = 0; i < 3; ++i) p.sigma[i] = sqrt(lam[i] > 0.0 ? lam[i] : 0.0);
  double v1[3], v2[3], v3[3], u1[3], u2[3], u3[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) v1[r] = pick3(i1, v[r][0], v[r][1], v[r][2]), v2[r] = pick3(i2, v[r][0], v[r][1], v[r][2]);
  v3[0] = v1[1] * v2[2] - v1[2] * v2[1];
  v3[1] = v1[2] * v2[0] - v1[0] * v2[2];
  v3[2] = v1[0] * v2[1] - v1[1] * v2[0];
  double w[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    u1[r] = ((E[r][0] * v1[0] + E[r][1] * v1[1]) + E[r][2] * v1[2]) / p.sigma[0];
    w[r] = (E[r][0] * v2[0] + E[r][1] * v2[1]) + E[r][2] * v2[2];
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
  // sigma_3 from the vectors: l3 is rounding noise of size eps * l1, and its root would keep half the digits only
  double ev3[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) ev3[r] = (E[r][0] * v3[0] + E[r][1] * v3[1]) + E[r][2] * v3[2];
  const double s3 = fabs((u3[0] * ev3[0] + u3[1] * ev3[1]) + u3[2] * ev3[2]);
  p.sigma[2] = finite_d(s3) ? s3 : p.sigma[2];
  bool out = true;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      p.R[0][3 * i + j] = (u2[i] * v1[j] - u1[i] * v2[j]) + u3[i] * v3[j];
      p.R[1][3 * i + j] = (u1[i] * v2[j] - u2[i] * v1[j]) + u3[i] * v3[j];
      out = out && finite_d(p.R[0][3 * i + j]) && finite_d(p.R[1][3 * i + j]);
    }
    p.t[i] = u3[i];
    out = out && finite_d(u3[i]) && finite_d(p.sigma[i]);
  }
  p.ok = any && fin && p.sigma[1] > 0.0 && out;
}

// The depths of one record under (R, +t): the least-squares solution of z1 a + t = z2 d2, a = R d1.  Under (R, -t) both
// depths are these with the sign changed, exactly: at and bt change sign and so do both numerators.
__device__ __forceinline__ void pose_depths(const double (&R)[9], const double (&t)[3], const PoseCams &k, double x1,
                                            double y1, double x2, double y2, double &d1x, double &d1y, double &z1,
                                            double &z2) {
  d1x = (x1 - k.px1) / k.fx1, d1y = (y1 - k.py1) / k.fy1;
  const double d2x = (x2 - k.px2) / k.fx2, d2y = (y2 - k.py2) / k.fy2;
  const double a0 = (R[0] * d1x + R[1] * d1y) + R[2];
  const double a1 = (R[3] * d1x + R[4] * d1y) + R[5];
  const double a2 = (R[6] * d1x + R[7] * d1y) + R[8];
  const double aa = (a0 * a0 + a1 * a1) + a2 * a2;
  const double bb = (d2x * d2x + d2y * d2y) + 1.0;
  const double ab = (a0 * d2x + a1 * d2y) + a2;
  const double at = (a0 * t[0] + a1 * t[1]) + a2 * t[2];
  const double bt = (d2x * t[0] + d2y * t[1]) + t[2];
  const double det = aa * bb - ab * ab;
  z1 = (ab * bt - bb * at) / det;
  z2 = (aa * bt - ab * at) / det;
}

// The epipolar head's F, and whether record i of this pair belongs to the fit set under it (then its coordinates).
__device__ __forceinline__ bool pose_fit(const double (&F)[9], const float *__restrict__ coord,
                                         const unsigned char *__restrict__ marks, int num_pts, int i, int n, float thresh,
                                         double &x1, double &y1, double &x2, double &y2) {
  if (i >= n || !(marks[i] & 1)) return false;
  x1 = (double)coord[i], y1 = (double)coord[(size_t)num_pts + i];
  x2 = (double)coord[2 * (size_t)num_pts + i], y2 = (double)coord[3 * (size_t)num_pts + i];
  return epipolar_inlier(F, x1, y1, x2, y2, (double)thresh * (double)thresh);
}

// pose: the pose head, zeroed before this launch.  Adds the four candidates' votes to its words kPoseHeadVotes .. + 3.
__global__ void __launch_bounds__(kPoseThreads) pose_vote_kernel(const float *__restrict__ coord,
                                                                 const unsigned char *__restrict__ marks, int num_pts,
                                                                 const int *__restrict__ head, PoseCams cams, float thresh,
                                                                 int *__restrict__ pose, PlanarBatch nb) {
  __shared__ int s_wave[4][kPoseThreads / 64];
  coord = pair_ptr(coord, nb.scratch), marks = pair_ptr(marks, nb.scratch);
  head = pair_ptr(head, nb.head), pose = pair_ptr(pose, kPoseHeadBytes);
  const int tx = threadIdx.x;
  const double *dhead = (const double *)head;
  double F[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) F[i] = dhead[kEpiHeadF + i];
  PoseFrame p;
  pose_decompose(F, cams, p);
  if (!p.ok) return;  // uniform: the votes stay 0
  const int n = pair_count(head, num_pts, nb);
  const int i = blockIdx.x * kPoseThreads + tx;
  bool front[4] = {false, false, false, false};
  double x1, y1, x2, y2;
  if (pose_fit(F, coord, marks, num_pts, i, n, thresh, x1, y1, x2, y2)) {
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      double d1x, d1y, z1, z2;
      pose_depths(p.R[r], p.t, cams, x1, y1, x2, y2, d1x, d1y, z1, z2);
      front[2 * r] = z1 > 0.0 && z2 > 0.0;
      front[2 * r + 1] = z1 < 0.0 && z2 < 0.0;  // -z1 > 0 && -z2 > 0
    }
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const unsigned long long m = __ballot(front[c]);
    if ((tx & 63) == 0) s_wave[c][tx >> 6] = __builtin_popcountll(m);
  }
  __syncthreads();
  if (tx < 4) {
    const int v = ((s_wave[tx][0] + s_wave[tx][1]) + s_wave[tx][2]) + s_wave[tx][3];
    if (v) atomicAdd(&pose[kPoseHeadVotes + tx], v);
  }
}

// Reads the four votes, writes coords3D of the records [0, n) of pts and -- workgroup 0 -- the rest of the pose head: as
// doubles [R | t] at kPoseHeadRt and sigma at kPoseHeadSigma, as int num_front at kPoseHeadFront.  xyz == NULL: the points
// go into the records; otherwise into xyz[pair][num_pts][3] (a batch, whose records stay as they are: a frame may be
// frame 1 of many pairs).
__global__ void __launch_bounds__(kPoseThreads) pose_write_kernel(cusift_point *__restrict__ pts,
                                                                  const float *__restrict__ coord,
                                                                  const unsigned char *__restrict__ marks, int num_pts,
                                                                  const int *__restrict__ head, PoseCams cams,
                                                                  float thresh, int *__restrict__ pose,
                                                                  float *__restrict__ xyz, PlanarBatch nb) {
  pts += (size_t)blockIdx.z * nb.records;
  if (xyz) xyz += 3 * (size_t)blockIdx.z * nb.flags;
  coord = pair_ptr(coord, nb.scratch), marks = pair_ptr(marks, nb.scratch);
  head = pair_ptr(head, nb.head), pose = pair_ptr(pose, kPoseHeadBytes);
  const int tx = threadIdx.x;
  const double *dhead = (const double *)head;
  double F[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) F[i] = dhead[kEpiHeadF + i];
  PoseFrame p;
  pose_decompose(F, cams, p);
  int win = 0, votes = pose[kPoseHeadVotes];
#pragma unroll
  for (int c = 1; c < 4; ++c) {
    const int v = pose[kPoseHeadVotes + c];
    win = v > votes ? c : win;
    votes = v > votes ? v : votes;
  }
  const bool ok = p.ok && votes > 0;  // otherwise the degenerate answer
  double R[9];
#pragma unroll
  for (int q = 0; q < 9; ++q) R[q] = win < 2 ? p.R[0][q] : p.R[1][q];
  const double sign = (win & 1) ? -1.0 : 1.0;
  const int n = pair_count(head, num_pts, nb);
  const int i = blockIdx.x * kPoseThreads + tx;
  float X = 0.0f, Y = 0.0f, Z = 0.0f;
  double x1, y1, x2, y2;
  if (ok && pose_fit(F, coord, marks, num_pts, i, n, thresh, x1, y1, x2, y2)) {
    double d1x, d1y, z1, z2;
    pose_depths(R, p.t, cams, x1, y1, x2, y2, d1x, d1y, z1, z2);
    z1 = sign * z1, z2 = sign * z2;
    const float fx = (float)(z1 * d1x), fy = (float)(z1 * d1y), fz = (float)z1;
    const bool keep = z1 > 0.0 && z2 > 0.0 && fabsf(fx) < __builtin_inff() && fabsf(fy) < __builtin_inff() &&
                      fabsf(fz) < __builtin_inff() && fz > 0.0f;
    X = keep ? fx : 0.0f, Y = keep ? fy : 0.0f, Z = keep ? fz : 0.0f;
  }
  if (i < n) {
    float *out = xyz ? xyz + 3 * (size_t)i : pts[i].coords3D;
    out[0] = X, out[1] = Y, out[2] = Z;
  }
  if (blockIdx.x == 0 && tx == 0) {
    // X1 = R X2 + t: R = R21^T, t = -R21^T t21 with t21 = sign * u3
    double *dpose = (double *)pose;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
      for (int c = 0; c < 3; ++c) dpose[kPoseHeadRt + 4 * r + c] = ok ? R[3 * c + r] : (r == c ? 1.0 : 0.0);
      const double t = -((R[r] * (sign * p.t[0]) + R[3 + r] * (sign * p.t[1])) + R[6 + r] * (sign * p.t[2]));
      dpose[kPoseHeadRt + 4 * r + 3] = ok ? t : 0.0;
      dpose[kPoseHeadSigma + r] = p.sigma[r];
    }
    pose[kPoseHeadFront] = ok ? votes : 0;
  }
}

}  // namespace cusift
