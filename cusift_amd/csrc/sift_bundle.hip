// sift_bundle.hip -- bundle adjustment on the device (cusift_bundle_adjust): the per-frame poses and the track points of
// cusift_build_tracks / cusift_triangulate_tracks refined together by Schur-complement Levenberg-Marquardt.  New
// functionality: the reference stops at one model per frame pair.  The contract, expression by expression, is
// include/cusift_amd_extras.h's; tests/bundle_model.py restates it in numpy.
//
// Everything is fp64 and nothing is decided on the host: the damping, the cost, the accept / reject decision and the
// stop live in a BundleState in scratch, every kernel of an iteration reads `stopped` first, and the poses and points
// are double-buffered -- the trial goes to buffer 1 - cur and an accepted step flips cur, nothing is copied.  Enqueued,
// whatever the data holds:
//
//   hipMemsetAsync x 2       node -> track all -1; the state and the per-frame counts zero
//   hipMemcpyAsync           the poses
//   bundle_index_kernel      one thread per track: the entry decisions (which observations are used), node -> track, the
//                            points into both buffers, the entry cost of the track.  Integer atomics count.
//   bundle_decide_kernel     (entry form) the entry cost, the held frames, lambda
//   per iteration, six launches:
//   bundle_track_kernel      one thread per track: V_t and g_t over its members in d_obs order, the damped inverse
//   bundle_frame_kernel      one workgroup per frame: U_f, g_f and e_f = sum W V^-1 g_t over the frame's records
//   bundle_schur_kernel      one workgroup per block pair f <= g: E_fg = sum W_tf V_t^-1 W_tg^T over frame f's records,
//                            the member in frame g by binary search in the track's sorted list; writes S and its
//                            right-hand side.  The W blocks are never stored: the Jacobians are recomputed where they
//                            are consumed, scratch stays at a word per node plus S.
//   bundle_solve_kernel      ONE workgroup of 1024: the Cholesky factorisation of S in global memory, a thread per row and
//                            six columns (a frame's block) per pass, L in both triangles so that every inner loop
//                            reads consecutive words; the two triangular solves through LDS; the trial poses.  One workgroup, so __syncthreads() orders its global
//                            stores and loads; S (at most 18.9 MB) stays in this XCD's L2.
//   bundle_trial_kernel      one thread per track: back-substitution, the trial point, the trial cost of the track
//   bundle_decide_kernel     sums the costs, decides, updates lambda and the state, writes the history row
//   bundle_finish_kernel     the outputs from the accepted buffers
//
// Sums: a track's members in d_obs order from 0; a frame's records and the tracks' costs as 256 strided partials
// (partial k takes index k, k + 256, ... ascending) and a halving tree in LDS (block_tree_sum).  No floating-point
// atomics: the same input gives the same bytes.
#include <cmath>

#include "sift_host.h"
#include "sift_ransac.h"

namespace cusift {

constexpr int kBundleThreads = 256;
constexpr int kBundleSolveThreads = 1024;
constexpr int kBundleMaxFrames = 256;
constexpr int kBundleMaxDim = 6 * kBundleMaxFrames;
constexpr int kBundleSolveRows = kBundleMaxDim / kBundleSolveThreads + 1;  // rows of S a solve thread owns, at most
constexpr int kBundleRound = 12;  // values block_tree_sum reduces per pass: 12 x 256 doubles of LDS

struct BundleCam {
  double fx, fy, px, py;
};
struct BundleOpts {
  double lambda, lambda_min, lambda_max, huber, max_error, min_decrease;
};
struct BundleFixed {
  unsigned char f[kBundleMaxFrames];
};
struct BundleState {
  double cost, lambda, entry_cost;
  int stopped, accepted, ran, cur, sfail, used_tracks, used_obs, free_frames;
};

// c = R^T (X - t), q = (c0 / c2, c1 / c2), r = (fx q0 + px - x, fy q1 + py - y)
struct BundleProj {
  double c0, c1, c2, q0, q1, r0, r1, err2;
};
__device__ __forceinline__ BundleProj bundle_project(const double *__restrict__ P, double X0, double X1, double X2,
                                                     double x, double y, const BundleCam &cam) {
  BundleProj o;
  const double e0 = X0 - P[3], e1 = X1 - P[7], e2 = X2 - P[11];
  o.c0 = (P[0] * e0 + P[4] * e1) + P[8] * e2;
  o.c1 = (P[1] * e0 + P[5] * e1) + P[9] * e2;
  o.c2 = (P[2] * e0 + P[6] * e1) + P[10] * e2;
  o.q0 = o.c0 / o.c2, o.q1 = o.c1 / o.c2;
  o.r0 = (cam.fx * o.q0 + cam.px) - x, o.r1 = (cam.fy * o.q1 + cam.py) - y;
  o.err2 = o.r0 * o.r0 + o.r1 * o.r1;
  return o;
}
__device__ __forceinline__ double bundle_rho(double err2, double huber) {
  if (huber == 0.0 || err2 <= huber * huber) return err2;
  return (2.0 * huber) * sqrt(err2) - huber * huber;
}

// One observation at the current iterate: the residual, the IRLS weight and the two Jacobians.
struct BundleObs {
  double r0, r1, w;
  double JX[2][3], Jc[2][6];
};
__device__ __forceinline__ void bundle_observe(const double *__restrict__ P, const double *__restrict__ X, double x,
                                               double y, const BundleCam &cam, double huber, BundleObs &o) {
  const BundleProj p = bundle_project(P, X[0], X[1], X[2], x, y, cam);
  o.r0 = p.r0, o.r1 = p.r1;
  o.w = (huber == 0.0 || p.err2 <= huber * huber) ? 1.0 : huber / sqrt(p.err2);
  const double a0 = cam.fx / p.c2, a1 = cam.fy / p.c2;
  const double b0 = 0.0 - a0 * p.q0, b1 = 0.0 - a1 * p.q1;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    o.JX[0][k] = a0 * P[4 * k + 0] + b0 * P[4 * k + 2];
    o.JX[1][k] = a1 * P[4 * k + 1] + b1 * P[4 * k + 2];
    o.Jc[0][3 + k] = 0.0 - o.JX[0][k];
    o.Jc[1][3 + k] = 0.0 - o.JX[1][k];
  }
  o.Jc[0][0] = 0.0 - b0 * p.c1, o.Jc[0][1] = b0 * p.c0 - a0 * p.c2, o.Jc[0][2] = a0 * p.c1;
  o.Jc[1][0] = a1 * p.c2 - b1 * p.c1, o.Jc[1][1] = b1 * p.c0, o.Jc[1][2] = 0.0 - a1 * p.c0;
}
// W[a][k] = w (Jc[0][a] JX[0][k] + Jc[1][a] JX[1][k])
__device__ __forceinline__ void bundle_w(const BundleObs &o, double (&W)[6][3]) {
#pragma unroll
  for (int a = 0; a < 6; ++a)
#pragma unroll
    for (int k = 0; k < 3; ++k) W[a][k] = o.w * (o.Jc[0][a] * o.JX[0][k] + o.Jc[1][a] * o.JX[1][k]);
}
// tv: what bundle_track_kernel leaves per track -- the damped inverse (00, 10, 11, 20, 21, 22) and g_t
__device__ __forceinline__ double bundle_vi(const double *__restrict__ tv, int i, int k) {
  const int r = i > k ? i : k, c = i > k ? k : i;
  return tv[r * (r + 1) / 2 + c];
}
// Y = W V^-1
__device__ __forceinline__ void bundle_y(const double (&W)[6][3], const double *__restrict__ tv, double (&Y)[6][3]) {
#pragma unroll
  for (int a = 0; a < 6; ++a)
#pragma unroll
    for (int k = 0; k < 3; ++k)
      Y[a][k] = (W[a][0] * bundle_vi(tv, 0, k) + W[a][1] * bundle_vi(tv, 1, k)) + W[a][2] * bundle_vi(tv, 2, k);
}

// The sum of each of v[0 .. NV) over the 256 threads: partial[k] += partial[k + h] for h = 128, 64 .. 1.  Every thread
// gets the totals.  s: kBundleRound x 256 doubles.
template <int NV>
__device__ __forceinline__ void block_tree_sum(double (&v)[NV], double *s) {
  const int tx = threadIdx.x;
#pragma unroll
  for (int base = 0; base < NV; base += kBundleRound) {  // (unrolled: v[] stays in registers)
    const int cnt = NV - base < kBundleRound ? NV - base : kBundleRound;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kBundleRound; ++j)
      if (base + j < NV) s[j * kBundleThreads + tx] = v[base + j];
    __syncthreads();
    for (int h = kBundleThreads / 2; h >= 1; h >>= 1) {
      if (tx < h)
        for (int j = 0; j < cnt; ++j) s[j * kBundleThreads + tx] += s[j * kBundleThreads + tx + h];
      __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < kBundleRound; ++j)
      if (base + j < NV) v[base + j] = s[j * kBundleThreads];
  }
}

// ---- entry ----------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBundleThreads) bundle_index_kernel(
    const cusift_point *__restrict__ points, int n_images, int max_pts, const int *__restrict__ offsets,
    const int *__restrict__ obs, const unsigned int *__restrict__ stats, int max_tracks,
    const double *__restrict__ poses, BundleCam cam, BundleOpts opt, const double *__restrict__ points3d,
    int *__restrict__ node_track, int *__restrict__ frame_used, int *__restrict__ used, double *__restrict__ X,
    double *__restrict__ tcost, BundleState *state) {
  const long t = (long)blockIdx.x * kBundleThreads + threadIdx.x;
  const long n_tracks = min((long)stats[0], (long)max_tracks);
  if (t >= n_tracks) return;
  const double *row = points3d + 4 * (size_t)t;
  const double X0 = row[0], X1 = row[1], X2 = row[2];
  double *Xa = X + 3 * (size_t)t, *Xb = X + 3 * ((size_t)max_tracks + t);
  Xa[0] = X0, Xa[1] = X1, Xa[2] = X2;
  Xb[0] = X0, Xb[1] = X1, Xb[2] = X2;
  const int first = offsets[t], last = offsets[t + 1];
  const long n_nodes = (long)n_images * max_pts;
  bool alive = !(X0 == 0.0 && X1 == 0.0 && X2 == 0.0 && row[3] == 0.0);
  const double inf = __builtin_inf();
  int n_used = 0;
  for (int e = first; alive && e < last; ++e) {
    const int v = obs[e];
    if (v < 0 || v >= n_nodes) {  // not a node of this batch: the track is left alone
      alive = false;
      break;
    }
    const double x = (double)points[v].coords2D[0], y = (double)points[v].coords2D[1];
    if (!(fabs(x) < inf && fabs(y) < inf)) {
      alive = false;
      break;
    }
    const BundleProj p = bundle_project(poses + 12 * (size_t)(v / max_pts), X0, X1, X2, x, y, cam);
    const bool ok = p.c2 > 0.0 && p.err2 < inf && (opt.max_error == 0.0 || sqrt(p.err2) <= opt.max_error);
    n_used += ok ? 1 : 0;
  }
  alive = alive && n_used >= 2;
  used[t] = alive ? 1 : 0;
  double cost = 0.0;
  for (int e = first; alive && e < last; ++e) {
    const int v = obs[e];
    const double x = (double)points[v].coords2D[0], y = (double)points[v].coords2D[1];
    const BundleProj p = bundle_project(poses + 12 * (size_t)(v / max_pts), X0, X1, X2, x, y, cam);
    const bool ok = p.c2 > 0.0 && p.err2 < inf && (opt.max_error == 0.0 || sqrt(p.err2) <= opt.max_error);
    if (!ok) continue;
    node_track[v] = (int)t;
    frame_used[v / max_pts] = 1;  // (whoever comes first: the value is the same)
    cost += bundle_rho(p.err2, opt.huber);
  }
  tcost[t] = cost;
  if (alive) {
    atomicAdd(&state->used_tracks, 1);
    atomicAdd(&state->used_obs, n_used);
  }
}

// ---- one iteration --------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBundleThreads) bundle_track_kernel(
    const cusift_point *__restrict__ points, int max_pts, const int *__restrict__ offsets, const int *__restrict__ obs,
    const unsigned int *__restrict__ stats, int max_tracks, int n_images, const double *__restrict__ Pbuf,
    const double *__restrict__ Xbuf, BundleCam cam, double huber, const int *__restrict__ node_track,
    const int *__restrict__ used, const BundleState *__restrict__ state, double *__restrict__ tv,
    int *__restrict__ vfail) {
  if (state->stopped) return;
  const long t = (long)blockIdx.x * kBundleThreads + threadIdx.x;
  const long n_tracks = min((long)stats[0], (long)max_tracks);
  if (t >= n_tracks || !used[t]) return;
  const int cur = state->cur;
  const double lambda = state->lambda;
  const double *P = Pbuf + 12 * (size_t)cur * n_images, *X = Xbuf + 3 * ((size_t)cur * max_tracks + t);
  double V00 = 0.0, V10 = 0.0, V11 = 0.0, V20 = 0.0, V21 = 0.0, V22 = 0.0, g0 = 0.0, g1 = 0.0, g2 = 0.0;
  const int first = offsets[t], last = offsets[t + 1];
  for (int e = first; e < last; ++e) {
    const int v = obs[e];
    if (node_track[v] != (int)t) continue;
    BundleObs o;
    bundle_observe(P + 12 * (size_t)(v / max_pts), X, (double)points[v].coords2D[0], (double)points[v].coords2D[1], cam,
                   huber, o);
    V00 += o.w * (o.JX[0][0] * o.JX[0][0] + o.JX[1][0] * o.JX[1][0]);
    V10 += o.w * (o.JX[0][1] * o.JX[0][0] + o.JX[1][1] * o.JX[1][0]);
    V11 += o.w * (o.JX[0][1] * o.JX[0][1] + o.JX[1][1] * o.JX[1][1]);
    V20 += o.w * (o.JX[0][2] * o.JX[0][0] + o.JX[1][2] * o.JX[1][0]);
    V21 += o.w * (o.JX[0][2] * o.JX[0][1] + o.JX[1][2] * o.JX[1][1]);
    V22 += o.w * (o.JX[0][2] * o.JX[0][2] + o.JX[1][2] * o.JX[1][2]);
    g0 += o.w * (o.JX[0][0] * o.r0 + o.JX[1][0] * o.r1);
    g1 += o.w * (o.JX[0][1] * o.r0 + o.JX[1][1] * o.r1);
    g2 += o.w * (o.JX[0][2] * o.r0 + o.JX[1][2] * o.r1);
  }
  const double v00 = V00 + lambda * V00, v11 = V11 + lambda * V11, v22 = V22 + lambda * V22;
  const double v10 = V10, v20 = V20, v21 = V21;
  const double c00 = v11 * v22 - v21 * v21, c10 = v21 * v20 - v10 * v22, c20 = v10 * v21 - v11 * v20;
  const double det = (v00 * c00 + v10 * c10) + v20 * c20;
  const double c11 = v00 * v22 - v20 * v20, c21 = v10 * v20 - v00 * v21, c22 = v00 * v11 - v10 * v10;
  vfail[t] = (v00 > 0.0 && c22 > 0.0 && det > 0.0 && det < __builtin_inf()) ? 0 : 1;
  double *out = tv + 9 * (size_t)t;
  out[0] = c00 / det, out[1] = c10 / det, out[2] = c11 / det, out[3] = c20 / det, out[4] = c21 / det, out[5] = c22 / det;
  out[6] = g0, out[7] = g1, out[8] = g2;
}

// fterms[f]: U_f [36], g_f [6], e_f [6]
__global__ void __launch_bounds__(kBundleThreads) bundle_frame_kernel(
    const cusift_point *__restrict__ points, int max_pts, int max_tracks, int n_images,
    const double *__restrict__ Pbuf, const double *__restrict__ Xbuf, BundleCam cam, double huber,
    const int *__restrict__ node_track, const int *__restrict__ held, const BundleState *__restrict__ state,
    const double *__restrict__ tv, double *__restrict__ fterms) {
  __shared__ double s_red[kBundleRound * kBundleThreads];
  const int f = blockIdx.x;
  if (state->stopped || held[f]) return;
  const int cur = state->cur;
  const double *P = Pbuf + 12 * ((size_t)cur * n_images + f), *X = Xbuf + 3 * (size_t)cur * max_tracks;
  double acc[48];
#pragma unroll
  for (int k = 0; k < 48; ++k) acc[k] = 0.0;
  for (int i = threadIdx.x; i < max_pts; i += kBundleThreads) {
    const size_t v = (size_t)f * max_pts + i;
    const int t = node_track[v];
    if (t < 0) continue;
    BundleObs o;
    bundle_observe(P, X + 3 * (size_t)t, (double)points[v].coords2D[0], (double)points[v].coords2D[1], cam, huber, o);
    double W[6][3], Y[6][3];
    bundle_w(o, W);
    const double *tvt = tv + 9 * (size_t)t;
    bundle_y(W, tvt, Y);
#pragma unroll
    for (int a = 0; a < 6; ++a) {
#pragma unroll
      for (int b = 0; b < 6; ++b) acc[6 * a + b] += o.w * (o.Jc[0][a] * o.Jc[0][b] + o.Jc[1][a] * o.Jc[1][b]);
      acc[36 + a] += o.w * (o.Jc[0][a] * o.r0 + o.Jc[1][a] * o.r1);
      acc[42 + a] += (Y[a][0] * tvt[6] + Y[a][1] * tvt[7]) + Y[a][2] * tvt[8];
    }
  }
  block_tree_sum<48>(acc, s_red);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < 48; ++k) fterms[48 * (size_t)f + k] = acc[k];
  }
}

// grid (g, f); only f <= g works.  S is [M][M] row-major, M = 6 n_images; both triangles are written.
__global__ void __launch_bounds__(kBundleThreads) bundle_schur_kernel(
    const cusift_point *__restrict__ points, int max_pts, const int *__restrict__ offsets, const int *__restrict__ obs,
    int max_tracks, int n_images, const double *__restrict__ Pbuf, const double *__restrict__ Xbuf, BundleCam cam,
    double huber, const int *__restrict__ node_track, const int *__restrict__ held,
    const BundleState *__restrict__ state, const double *__restrict__ tv, const double *__restrict__ fterms,
    double *__restrict__ S, double *__restrict__ rhs) {
  __shared__ double s_red[kBundleRound * kBundleThreads];
  const int g = blockIdx.x, f = blockIdx.y;
  if (f > g || state->stopped) return;
  const size_t M = 6 * (size_t)n_images;
  if (held[f] || held[g]) {  // a held frame: its diagonal block is the identity, everything else of its rows zero
    if (threadIdx.x < 36) {
      const int a = threadIdx.x / 6, b = threadIdx.x % 6;
      const double val = (f == g && a == b) ? 1.0 : 0.0;
      S[(6 * (size_t)f + a) * M + 6 * (size_t)g + b] = val;
      S[(6 * (size_t)g + b) * M + 6 * (size_t)f + a] = val;
      if (f == g && b == 0) rhs[6 * (size_t)f + a] = 0.0;
    }
    return;
  }
  const int cur = state->cur;
  const double lambda = state->lambda;
  const double *Pf = Pbuf + 12 * ((size_t)cur * n_images + f), *Pg = Pbuf + 12 * ((size_t)cur * n_images + g);
  const double *X = Xbuf + 3 * (size_t)cur * max_tracks;
  double acc[36];
#pragma unroll
  for (int k = 0; k < 36; ++k) acc[k] = 0.0;
  for (int i = threadIdx.x; i < max_pts; i += kBundleThreads) {
    const size_t v = (size_t)f * max_pts + i;
    const int t = node_track[v];
    if (t < 0) continue;
    size_t u = v;
    if (g != f) {  // the track's member in frame g: its list is sorted by node, one per frame
      int lo = offsets[t], hi = offsets[t + 1];
      const long want = (long)g * max_pts;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((long)obs[mid] < want) lo = mid + 1;
        else hi = mid;
      }
      if (lo >= offsets[t + 1]) continue;
      const long cand = obs[lo];
      if (cand >= want + max_pts || node_track[cand] != t) continue;
      u = (size_t)cand;
    }
    BundleObs o;
    double Wf[6][3], Wg[6][3], Y[6][3];
    bundle_observe(Pf, X + 3 * (size_t)t, (double)points[v].coords2D[0], (double)points[v].coords2D[1], cam, huber, o);
    bundle_w(o, Wf);
    bundle_y(Wf, tv + 9 * (size_t)t, Y);
    if (g != f) {
      bundle_observe(Pg, X + 3 * (size_t)t, (double)points[u].coords2D[0], (double)points[u].coords2D[1], cam, huber, o);
      bundle_w(o, Wg);
    }
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
      for (int b = 0; b < 6; ++b) {
        const double w0 = g != f ? Wg[b][0] : Wf[b][0], w1 = g != f ? Wg[b][1] : Wf[b][1];
        const double w2 = g != f ? Wg[b][2] : Wf[b][2];
        acc[6 * a + b] += (Y[a][0] * w0 + Y[a][1] * w1) + Y[a][2] * w2;
      }
  }
  block_tree_sum<36>(acc, s_red);
  __shared__ double s_tot[36];
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < 36; ++k) s_tot[k] = acc[k];
  }
  __syncthreads();
  if (threadIdx.x < 36) {
    const int a = threadIdx.x / 6, b = threadIdx.x % 6;
    const double E = s_tot[threadIdx.x];
    if (f == g) {
      const double *ft = fterms + 48 * (size_t)f;
      const double U = ft[6 * a + b];
      S[(6 * (size_t)f + a) * M + 6 * (size_t)f + b] = (a == b ? U + lambda * U : U) - E;
      if (b == 0) rhs[6 * (size_t)f + a] = ft[42 + a] - ft[36 + a];
    } else {
      S[(6 * (size_t)f + a) * M + 6 * (size_t)g + b] = 0.0 - E;
      S[(6 * (size_t)g + b) * M + 6 * (size_t)f + a] = 0.0 - E;
    }
  }
}

// One workgroup.  L = chol(S), every sum from k = 0 ascending:  acc = S[i][j] - sum_k L[i][k] L[j][k]; L[j][j] =
// sqrt(acc_j), L[i][j] = acc_i / L[j][j].  Six columns (one frame) at a time: a thread owns a row i and carries the six
// sums of its row; over the columns k in front of the block every L[i][k] it loads serves all six (rows J .. J + 5 of L,
// the other factor, are staged in LDS), inside the block the factors are its own registers and a 6 x 6 corner in LDS.
// An entry's sum still runs over k = 0 .. j - 1 ascending.  Only the lower triangle of S is read as input; L[i][j] goes
// to both S[i][j] and S[j][i], so the staged rows and a thread's walk down its column are both contiguous.
// L y = rhs (y_j = b_j / L_jj, b_i -= L_ij y_j for i > j, j ascending) is the same recurrence with rhs as row M of S and
// y as row M of L -- the same operations in the same order -- so it rides along as one more row, its factors in LDS.
// Then L^T x = y from the last column (x_j = y_j / L_jj, y_i -= L_ji x_j for i < j), eight rows of L fetched at a time
// so that one wait serves eight steps.
__global__ void __launch_bounds__(kBundleSolveThreads) bundle_solve_kernel(int n_images, double *__restrict__ Pbuf,
                                                                            const int *__restrict__ held,
                                                                            BundleState *state, double *S,
                                                                            const double *__restrict__ rhs,
                                                                            double *__restrict__ delta) {
  __shared__ double s_rows[6][kBundleMaxDim];  // rows J .. J + 5 of L, k < J
  __shared__ double s_blk[6][6];               // L[J + c][J + k], k < c: the block's own corner
  __shared__ double s_b[kBundleMaxDim];        // y, then the right-hand side of the back-substitution
  __shared__ double s_x[kBundleMaxDim];
  __shared__ double s_dg[kBundleMaxDim];  // the diagonal of L
  __shared__ double s_diag;
  __shared__ int s_fail;
  if (state->stopped) return;
  const int tx = threadIdx.x, M = 6 * n_images;
  if (tx == 0) s_fail = 0;
  for (int J = 0; J < M; J += 6) {
    for (int e = tx; e < 6 * J; e += kBundleSolveThreads) {
      const int c = e / J, k = e - c * J;
      s_rows[c][k] = S[(size_t)(J + c) * M + k];
    }
    __syncthreads();
    double acc[kBundleSolveRows][6];
#pragma unroll
    for (int r = 0; r < kBundleSolveRows; ++r) {
      const int i = J + tx + r * kBundleSolveThreads;  // i == M: the right-hand side
#pragma unroll
      for (int c = 0; c < 6; ++c) acc[r][c] = 0.0;
      if (i < M) {
#pragma unroll
        for (int c = 0; c < 6; ++c) acc[r][c] = J + c <= i ? S[(size_t)i * M + J + c] : 0.0;
        const double *col = S + i;  // L[i][k] at col[k * M]
        int k = 0;
        for (; k + 8 <= J; k += 8) {  // eight loads in flight, the subtractions in order
          double l[8];
#pragma unroll
          for (int u = 0; u < 8; ++u) l[u] = col[(size_t)(k + u) * M];
#pragma unroll
          for (int u = 0; u < 8; ++u)
#pragma unroll
            for (int c = 0; c < 6; ++c) acc[r][c] -= l[u] * s_rows[c][k + u];
        }
        for (; k < J; ++k) {
          const double l = col[(size_t)k * M];
#pragma unroll
          for (int c = 0; c < 6; ++c) acc[r][c] -= l * s_rows[c][k];
        }
      } else if (i == M) {
#pragma unroll
        for (int c = 0; c < 6; ++c) acc[r][c] = rhs[J + c];
        for (int k = 0; k < J; ++k) {
          const double l = s_b[k];
#pragma unroll
          for (int c = 0; c < 6; ++c) acc[r][c] -= l * s_rows[c][k];
        }
      }
    }
    // the block's six columns: the factors in front are the thread's own l[r][k] and the corner in LDS
    double l[kBundleSolveRows][6];
#pragma unroll
    for (int c = 0; c < 6; ++c) {
#pragma unroll
      for (int r = 0; r < kBundleSolveRows; ++r) {
        const int i = J + tx + r * kBundleSolveThreads;
        if (i >= J + c && i <= M) {
#pragma unroll
          for (int k = 0; k < 6; ++k)
            if (k < c) acc[r][c] -= l[r][k] * s_blk[c][k];
          if (i == J + c) s_diag = acc[r][c];
        }
      }
      __syncthreads();
      const double q = s_diag, d = sqrt(q);
      if (tx == 0 && !(q > 0.0 && q < __builtin_inf())) s_fail = 1;
#pragma unroll
      for (int r = 0; r < kBundleSolveRows; ++r) {
        const int i = J + tx + r * kBundleSolveThreads;
        l[r][c] = i == J + c ? d : acc[r][c] / d;
        if (i == J + c) s_dg[i] = d;
        if (i > J + c && i < J + 6) s_blk[i - J][c] = l[r][c];
        if (i == M) s_b[J + c] = l[r][c];
      }
      __syncthreads();
    }
#pragma unroll
    for (int r = 0; r < kBundleSolveRows; ++r) {
      const int i = J + tx + r * kBundleSolveThreads;
      if (i < M) {
#pragma unroll
        for (int c = 0; c < 6; ++c)
          if (i >= J + c) {
            S[(size_t)i * M + J + c] = l[r][c];
            S[(size_t)(J + c) * M + i] = l[r][c];
          }
      }
    }
    __syncthreads();
  }
  for (int jb = M - 1; jb >= 0; jb -= 8) {
    double row[8][kBundleSolveRows];  // L[jb - u][i] for the rows i < jb - u this thread owns
#pragma unroll
    for (int u = 0; u < 8; ++u)
#pragma unroll
      for (int r = 0; r < kBundleSolveRows; ++r) {
        const int j = jb - u, i = tx + r * kBundleSolveThreads;
        row[u][r] = (j >= 0 && i < j) ? S[(size_t)j * M + i] : 0.0;
      }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int j = jb - u;
      if (j >= 0) {  // (uniform)
        const double xj = s_b[j] / s_dg[j];
#pragma unroll
        for (int r = 0; r < kBundleSolveRows; ++r) {
          const int i = tx + r * kBundleSolveThreads;
          if (i < j) s_b[i] -= row[u][r] * xj;
        }
        if (tx == 0) s_x[j] = xj;
      }
      __syncthreads();
    }
  }
  for (int i = tx; i < M; i += kBundleSolveThreads) delta[i] = s_x[i];
  if (tx == 0 && s_fail) state->sfail = 1;
  // the trial poses: R <- R Exp(w), t <- t + dt; a held frame keeps its pose
  const int cur = state->cur;
  for (int f = tx; f < n_images; f += kBundleSolveThreads) {
    const double *P = Pbuf + 12 * ((size_t)cur * n_images + f);
    double *Q = Pbuf + 12 * ((size_t)(1 - cur) * n_images + f);
    if (held[f]) {
      for (int k = 0; k < 12; ++k) Q[k] = P[k];
      continue;
    }
    const double *d = s_x + 6 * f;
    double E[3][3];
    rodrigues_exp(d[0], d[1], d[2], E);
    for (int i = 0; i < 3; ++i) {
      for (int k = 0; k < 3; ++k) Q[4 * i + k] = (P[4 * i] * E[0][k] + P[4 * i + 1] * E[1][k]) + P[4 * i + 2] * E[2][k];
      Q[4 * i + 3] = P[4 * i + 3] + d[3 + i];
    }
  }
}

__global__ void __launch_bounds__(kBundleThreads) bundle_trial_kernel(
    const cusift_point *__restrict__ points, int max_pts, const int *__restrict__ offsets, const int *__restrict__ obs,
    const unsigned int *__restrict__ stats, int max_tracks, int n_images, const double *__restrict__ Pbuf,
    double *__restrict__ Xbuf, BundleCam cam, double huber, const int *__restrict__ node_track,
    const int *__restrict__ used, const BundleState *__restrict__ state, const double *__restrict__ tv,
    const int *__restrict__ vfail, const double *__restrict__ delta, double *__restrict__ tcost) {
  if (state->stopped) return;
  const long t = (long)blockIdx.x * kBundleThreads + threadIdx.x;
  const long n_tracks = min((long)stats[0], (long)max_tracks);
  if (t >= n_tracks || !used[t]) return;
  const int cur = state->cur;
  const double *P = Pbuf + 12 * (size_t)cur * n_images, *Q = Pbuf + 12 * (size_t)(1 - cur) * n_images;
  const double *X = Xbuf + 3 * ((size_t)cur * max_tracks + t);
  const double *tvt = tv + 9 * (size_t)t;
  double s0 = tvt[6], s1 = tvt[7], s2 = tvt[8];
  const int first = offsets[t], last = offsets[t + 1];
  for (int e = first; e < last; ++e) {
    const int v = obs[e];
    if (node_track[v] != (int)t) continue;
    const int f = v / max_pts;
    BundleObs o;
    bundle_observe(P + 12 * (size_t)f, X, (double)points[v].coords2D[0], (double)points[v].coords2D[1], cam, huber, o);
    double W[6][3];
    bundle_w(o, W);
    const double *d = delta + 6 * (size_t)f;
    double z[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      double a = W[0][k] * d[0] + W[1][k] * d[1];
#pragma unroll
      for (int c = 2; c < 6; ++c) a = a + W[c][k] * d[c];
      z[k] = a;
    }
    s0 += z[0], s1 += z[1], s2 += z[2];
  }
  double T[3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
    T[i] = X[i] + (0.0 - ((bundle_vi(tvt, i, 0) * s0 + bundle_vi(tvt, i, 1) * s1) + bundle_vi(tvt, i, 2) * s2));
  double *out = Xbuf + 3 * ((size_t)(1 - cur) * max_tracks + t);
  out[0] = T[0], out[1] = T[1], out[2] = T[2];
  double cost = 0.0;
  bool bad = vfail[t] != 0;
  for (int e = first; e < last; ++e) {
    const int v = obs[e];
    if (node_track[v] != (int)t) continue;
    const BundleProj p = bundle_project(Q + 12 * (size_t)(v / max_pts), T[0], T[1], T[2], (double)points[v].coords2D[0],
                                        (double)points[v].coords2D[1], cam);
    bad = bad || !(p.c2 > 0.0);
    cost += bundle_rho(p.err2, huber);
  }
  tcost[t] = (bad || !(cost < __builtin_inf())) ? __builtin_inf() : cost;
}

// One workgroup.  k < 0: the entry form.
__global__ void __launch_bounds__(kBundleThreads) bundle_decide_kernel(
    int k, const unsigned int *__restrict__ stats, int max_tracks, int n_images, BundleOpts opt, BundleFixed fixed,
    const int *__restrict__ used, const double *__restrict__ tcost, const int *__restrict__ frame_used,
    int *__restrict__ held, BundleState *state, double *__restrict__ history) {
  __shared__ double s_red[kBundleRound * kBundleThreads];
  const int tx = threadIdx.x;
  if (k >= 0 && state->stopped) {
    if (tx == 0) {
      double *h = history + 4 * (size_t)k;
      h[0] = state->cost, h[1] = state->cost, h[2] = state->lambda, h[3] = 2.0;
    }
    return;
  }
  const long n_tracks = min((long)stats[0], (long)max_tracks);
  double part[1] = {0.0};
  for (long t = tx; t < n_tracks; t += kBundleThreads)
    if (used[t]) part[0] += tcost[t];
  block_tree_sum<1>(part, s_red);
  if (k < 0) {
    for (int f = tx; f < n_images; f += kBundleThreads) held[f] = (fixed.f[f] != 0 || frame_used[f] == 0) ? 1 : 0;
    __syncthreads();
    if (tx == 0) {
      int n_free = 0;
      for (int f = 0; f < n_images; ++f) n_free += held[f] ? 0 : 1;
      state->free_frames = n_free;
      state->cost = state->entry_cost = part[0];
      state->lambda = opt.lambda;
      state->stopped = state->used_tracks == 0 ? 1 : 0;  // no used track: nothing to do
    }
    return;
  }
  if (tx != 0) return;
  const double inf = __builtin_inf();
  const double cost = state->cost, lambda = state->lambda;
  const double trial = (state->sfail || !(part[0] < inf)) ? inf : part[0];
  const bool accept = trial < cost;
  double *h = history + 4 * (size_t)k;
  h[0] = cost, h[1] = trial, h[2] = lambda, h[3] = accept ? 1.0 : 0.0;
  state->ran += 1;
  state->sfail = 0;
  if (accept) {
    const double gain = (cost - trial) / cost;
    const double next = lambda / 10.0;
    state->cost = trial;
    state->cur = 1 - state->cur;
    state->accepted += 1;
    state->lambda = next > opt.lambda_min ? next : opt.lambda_min;
    if (gain <= opt.min_decrease) state->stopped = 1;
  } else {
    state->lambda = 10.0 * lambda;
    if (state->lambda > opt.lambda_max) state->stopped = 1;
  }
}

__global__ void __launch_bounds__(kBundleThreads) bundle_finish_kernel(
    const cusift_point *__restrict__ points, int max_pts, const int *__restrict__ offsets, const int *__restrict__ obs,
    const unsigned int *__restrict__ stats, int max_tracks, int n_images, const double *__restrict__ Pbuf,
    const double *__restrict__ Xbuf, BundleCam cam, const int *__restrict__ node_track, const int *__restrict__ used,
    const BundleState *__restrict__ state, double *__restrict__ points3d, double *__restrict__ poses_out,
    double *__restrict__ summary) {
  const long t = (long)blockIdx.x * kBundleThreads + threadIdx.x;
  const int cur = state->cur;
  const double *P = Pbuf + 12 * (size_t)cur * n_images;
  if (t < 12 * (long)n_images) poses_out[t] = P[t];
  if (t == 0) {
    summary[0] = state->entry_cost, summary[1] = state->cost, summary[2] = (double)state->accepted;
    summary[3] = (double)state->ran, summary[4] = (double)state->used_tracks, summary[5] = (double)state->used_obs;
    summary[6] = (double)state->free_frames, summary[7] = state->lambda;
  }
  const long n_tracks = min((long)stats[0], (long)max_tracks);
  if (t >= n_tracks || !used[t]) return;
  const double *X = Xbuf + 3 * ((size_t)cur * max_tracks + t);
  double worst = 0.0;
  for (int e = offsets[t]; e < offsets[t + 1]; ++e) {
    const int v = obs[e];
    if (node_track[v] != (int)t) continue;
    const BundleProj p = bundle_project(P + 12 * (size_t)(v / max_pts), X[0], X[1], X[2], (double)points[v].coords2D[0],
                                        (double)points[v].coords2D[1], cam);
    worst = p.err2 > worst ? p.err2 : worst;
  }
  double *out = points3d + 4 * (size_t)t;
  out[0] = X[0], out[1] = X[1], out[2] = X[2], out[3] = sqrt(worst);
}

// max_tracks == 0, or a batch without nodes: nothing is adjusted
__global__ void bundle_empty_kernel(int iterations, double lambda, double *__restrict__ history,
                                    double *__restrict__ summary) {
  const int k = threadIdx.x;
  if (k < 8) summary[k] = 0.0;
  if (k < iterations) {
    double *h = history + 4 * (size_t)k;
    h[0] = 0.0, h[1] = 0.0, h[2] = lambda, h[3] = 2.0;
  }
}

}  // namespace cusift

// ------------------------------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------------------------------
extern "C" void cusift_bundle_default_params(cusift_bundle_params *p) {
  if (!p) return;
  p->iterations = 10;
  p->lambda = 1e-3, p->lambda_min = 1e-9, p->lambda_max = 1e6;
  p->huber = 0.0, p->max_error = 0.0, p->min_decrease = 1e-12;
}

extern "C" int cusift_bundle_adjust(cusift_ctx *ctx, const cusift_point *d_points, int n_images, int max_pts,
                                    const int *d_offsets, const int *d_obs, const unsigned int *d_stats, int max_tracks,
                                    const double *h_poses, const unsigned char *h_fixed, const cusift_camera *camera,
                                    const cusift_bundle_params *params, double *d_points3d, double *d_poses,
                                    double *d_history, double *d_summary) {
  TRY(enter(ctx));
  TRY(check_pair_list(nullptr, 0, n_images, max_pts, "BundleAdjust"));
  if ((long long)n_images * max_pts > 0x7fffffffLL)
    return fail(CUSIFT_ERR_INVALID, "BundleAdjust: %d frames x %d records are more than 2^31 - 1 nodes", n_images, max_pts);
  if (n_images > kBundleMaxFrames)
    return fail(CUSIFT_ERR_INVALID, "BundleAdjust: %d frames, the dense reduced system takes at most %d", n_images,
                kBundleMaxFrames);
  if (!d_points || !d_offsets || !d_obs || !d_stats || !h_poses || !camera || !params || !d_points3d || !d_poses ||
      !d_history || !d_summary)
    return fail(CUSIFT_ERR_INVALID, "BundleAdjust: NULL pointer");
  if (max_tracks < 0) return fail(CUSIFT_ERR_INVALID, "BundleAdjust: max_tracks %d is negative", max_tracks);
  if (!std::isfinite(camera->fx) || !std::isfinite(camera->fy) || camera->fx == 0.0f || camera->fy == 0.0f ||
      !std::isfinite(camera->cx) || !std::isfinite(camera->cy) || !std::isfinite(camera->origin))
    return fail(CUSIFT_ERR_INVALID, "BundleAdjust: fx, fy must be finite and not 0, cx, cy, origin finite");
  for (size_t k = 0; k < 12 * (size_t)n_images; ++k)
    if (!std::isfinite(h_poses[k]))
      return fail(CUSIFT_ERR_INVALID, "BundleAdjust: pose %zu has an entry that is not finite", k / 12);
  const cusift_bundle_params &q = *params;
  if (q.iterations < 1 || q.iterations > 100)
    return fail(CUSIFT_ERR_INVALID, "BundleAdjust: iterations %d outside [1, 100]", q.iterations);
  if (!(q.lambda > 0.0) || !std::isfinite(q.lambda) || !(q.lambda_min > 0.0) || !std::isfinite(q.lambda_min) ||
      !(q.lambda_max > 0.0) || !std::isfinite(q.lambda_max))
    return fail(CUSIFT_ERR_INVALID, "BundleAdjust: lambda, lambda_min and lambda_max must be positive and finite");
  if (!(q.huber >= 0.0) || !std::isfinite(q.huber) || !(q.max_error >= 0.0) || !std::isfinite(q.max_error) ||
      !(q.min_decrease >= 0.0) || !std::isfinite(q.min_decrease))
    return fail(CUSIFT_ERR_INVALID, "BundleAdjust: huber, max_error and min_decrease must be finite and not negative");

  const size_t poses_b = sizeof(double) * 12 * (size_t)n_images;
  const dim3 block(kBundleThreads);
  if (max_tracks == 0 || n_images == 0 || max_pts == 0) {
    if (poses_b) HIP_TRY(hipMemcpyAsync(d_poses, h_poses, poses_b, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(bundle_empty_kernel, dim3(1), block, 0, ctx->stream, q.iterations, q.lambda, d_history, d_summary);
    return check_launch("bundle_empty");
  }

  // scratch: [state | per-frame counts | held | poses x 2 | node -> track | used | V pivots | points x 2 | per-track
  // terms | per-track costs | per-frame terms | S | right-hand side | step]
  const size_t n_nodes = (size_t)n_images * max_pts, M = 6 * (size_t)n_images, T = (size_t)max_tracks;
  ScratchLayout L;
  const size_t state_at = L.take(sizeof(BundleState)), fused_at = L.take(sizeof(int) * n_images);
  const size_t zero_b = L.size;  // the state and the counts: one memset
  const size_t held_at = L.take(sizeof(int) * n_images), poses_at = L.take(2 * poses_b);
  const size_t node_at = L.take(sizeof(int) * n_nodes), used_at = L.take(sizeof(int) * T);
  const size_t vfail_at = L.take(sizeof(int) * T), x_at = L.take(sizeof(double) * 6 * T);
  const size_t tv_at = L.take(sizeof(double) * 9 * T), tcost_at = L.take(sizeof(double) * T);
  const size_t ft_at = L.take(sizeof(double) * 48 * n_images), s_at = L.take(sizeof(double) * M * M);
  const size_t rhs_at = L.take(sizeof(double) * M), delta_at = L.take(sizeof(double) * M);
  TRY(grow_scratch(ctx, ctx->bundle_scratch, ctx->bundle_scratch_bytes, L.size, "BundleAdjust: ", false));
  char *s = ctx->bundle_scratch;
  BundleState *state = at<BundleState>(s, state_at);
  int *frame_used = at<int>(s, fused_at), *held = at<int>(s, held_at), *node_track = at<int>(s, node_at);
  int *used = at<int>(s, used_at), *vfail = at<int>(s, vfail_at);
  double *Pbuf = at<double>(s, poses_at), *Xbuf = at<double>(s, x_at), *tv = at<double>(s, tv_at);
  double *tcost = at<double>(s, tcost_at), *fterms = at<double>(s, ft_at), *S = at<double>(s, s_at);
  double *rhs = at<double>(s, rhs_at), *delta = at<double>(s, delta_at);

  BundleCam cam;
  cam.fx = (double)camera->fx, cam.fy = (double)camera->fy;
  cam.px = (double)camera->cx - (double)camera->origin, cam.py = (double)camera->cy - (double)camera->origin;
  BundleOpts opt = {q.lambda, q.lambda_min, q.lambda_max, q.huber, q.max_error, q.min_decrease};
  BundleFixed fixed;
  for (int f = 0; f < kBundleMaxFrames; ++f) fixed.f[f] = f < n_images ? (h_fixed ? (h_fixed[f] != 0) : (f == 0)) : 0;

  const dim3 tracks(idiv_up(max_tracks, kBundleThreads)), one(1);
  const dim3 finish(std::max(idiv_up(max_tracks, kBundleThreads), idiv_up(12 * n_images, kBundleThreads)));
  HIP_TRY(hipMemsetAsync(s, 0, zero_b, ctx->stream));
  HIP_TRY(hipMemsetAsync(node_track, 0xFF, sizeof(int) * n_nodes, ctx->stream));
  HIP_TRY(hipMemcpyAsync(Pbuf, h_poses, poses_b, hipMemcpyHostToDevice, ctx->stream));
  hipLaunchKernelGGL(bundle_index_kernel, tracks, block, 0, ctx->stream, d_points, n_images, max_pts, d_offsets, d_obs,
                     d_stats, max_tracks, (const double *)Pbuf, cam, opt, (const double *)d_points3d, node_track,
                     frame_used, used, Xbuf, tcost, state);
  hipLaunchKernelGGL(bundle_decide_kernel, one, block, 0, ctx->stream, -1, d_stats, max_tracks, n_images, opt, fixed,
                     (const int *)used, (const double *)tcost, (const int *)frame_used, held, state, d_history);
  for (int k = 0; k < q.iterations; ++k) {
    hipLaunchKernelGGL(bundle_track_kernel, tracks, block, 0, ctx->stream, d_points, max_pts, d_offsets, d_obs, d_stats,
                       max_tracks, n_images, (const double *)Pbuf, (const double *)Xbuf, cam, q.huber,
                       (const int *)node_track, (const int *)used, (const BundleState *)state, tv, vfail);
    hipLaunchKernelGGL(bundle_frame_kernel, dim3(n_images), block, 0, ctx->stream, d_points, max_pts, max_tracks,
                       n_images, (const double *)Pbuf, (const double *)Xbuf, cam, q.huber, (const int *)node_track,
                       (const int *)held, (const BundleState *)state, (const double *)tv, fterms);
    hipLaunchKernelGGL(bundle_schur_kernel, dim3(n_images, n_images), block, 0, ctx->stream, d_points, max_pts,
                       d_offsets, d_obs, max_tracks, n_images, (const double *)Pbuf, (const double *)Xbuf, cam, q.huber,
                       (const int *)node_track, (const int *)held, (const BundleState *)state, (const double *)tv,
                       (const double *)fterms, S, rhs);
    hipLaunchKernelGGL(bundle_solve_kernel, one, dim3(kBundleSolveThreads), 0, ctx->stream, n_images, Pbuf,
                       (const int *)held, state, S, (const double *)rhs, delta);
    hipLaunchKernelGGL(bundle_trial_kernel, tracks, block, 0, ctx->stream, d_points, max_pts, d_offsets, d_obs, d_stats,
                       max_tracks, n_images, (const double *)Pbuf, Xbuf, cam, q.huber, (const int *)node_track,
                       (const int *)used, (const BundleState *)state, (const double *)tv, (const int *)vfail,
                       (const double *)delta, tcost);
    hipLaunchKernelGGL(bundle_decide_kernel, one, block, 0, ctx->stream, k, d_stats, max_tracks, n_images, opt, fixed,
                       (const int *)used, (const double *)tcost, (const int *)frame_used, held, state, d_history);
  }
  hipLaunchKernelGGL(bundle_finish_kernel, finish, block, 0, ctx->stream, d_points, max_pts, d_offsets, d_obs, d_stats,
                     max_tracks, n_images, (const double *)Pbuf, (const double *)Xbuf, cam, (const int *)node_track,
                     (const int *)used, (const BundleState *)state, d_points3d, d_poses, d_summary);
  return check_launch("bundle_adjust");
}
