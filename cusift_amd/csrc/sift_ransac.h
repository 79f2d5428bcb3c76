// sift_ransac.h -- the device helpers that the registration units share (sift_rigid.hip, sift_homography.hip,
// sift_planar.hip, sift_epipolar.hip, sift_pose.hip, sift_pnp.hip, sift_sequence.hip, sift_rgbd.hip).  Inline functions only: the LDS arrays stay
// declared in the kernels and are passed in.  Every rule here is pinned bit for bit by the units' tests.
//
// SAMPLING.  The reference seeds cuRAND with time(0) (extras/rigidTransform.cu:411), which cannot be reproduced.  Here
// draw number k of loop l out of n is
//     u(seed, l, k) = mix(seed ^ mix((l << 32) | k)),         index = (u >> 32) mod n
//     mix(z): z += 0x9E3779B97F4A7C15; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;
//             z = (z ^ (z >> 27)) * 0x94D049BB133111EB; return z ^ (z >> 31)          (all modulo 2^64)
// The N slots of a hypothesis (3 rigid, 4 homography, 6 PnP, 8 fundamental matrix) are draws 0 .. N-1; then, with k counting on
// from N, slots 2 .. N in order: while the slot equals an earlier one, redraw it (extras/rigidTransform.cu:343-349,
// extras/homography.cu:222-235).  A slot redrawn 64 times takes the lowest index not taken yet, so the loop is bounded.
// Integer arithmetic only: tests/test_rigid.py, tests/test_planar.py and tests/test_epipolar.py restate it and demand
// identical indices.  The planar, epipolar and PnP paths draw positions in the candidate list, pair p from seed + p.
#pragma once

#include "sift_device.h"

namespace cusift {

constexpr int kRansacThreads = 256;  // the workgroup of every *_256 helper and of ransac_winner: four waves
constexpr int kRansacRedraws = 64;

__device__ __forceinline__ bool finite_d(double x) { return fabs(x) < __builtin_inf(); }  // a NaN fails

// a_i for a run-time i in {0, 1, 2}: selects, so the three stay in registers
__device__ __forceinline__ double pick3(int i, double a0, double a1, double a2) {
  return i == 0 ? a0 : (i == 1 ? a1 : a2);
}

__device__ __forceinline__ unsigned long long ransac_mix(unsigned long long z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__device__ __forceinline__ int ransac_draw(unsigned long long seed, int loop, unsigned int k, int n) {
  const unsigned long long u = ransac_mix(seed ^ ransac_mix(((unsigned long long)(unsigned int)loop << 32) | k));
  return (int)((unsigned int)(u >> 32) % (unsigned int)n);
}

// The N distinct samples of hypothesis `loop` out of [0, n), n >= N: the recipe above.
template <int N>
__device__ __forceinline__ void ransac_sample(unsigned long long seed, int loop, int n, int (&p)[N]) {
  unsigned int k = N;
#pragma unroll
  for (int s = 0; s < N; ++s) p[s] = ransac_draw(seed, loop, (unsigned int)s, n);
#pragma unroll
  for (int s = 1; s < N; ++s) {
    int tries = 0;
    bool clash = true;
    while (true) {
      clash = false;
#pragma unroll
      for (int q = 0; q < s; ++q) clash = clash || p[s] == p[q];
      if (!clash || tries >= kRansacRedraws) break;
      p[s] = ransac_draw(seed, loop, k++, n);
      ++tries;
    }
    if (clash) {
      int v = 0;
      bool taken = true;
      while (taken) {  // n >= N > s: at most s steps
        taken = false;
#pragma unroll
        for (int q = 0; q < s; ++q) taken = taken || v == p[q];
        v += taken ? 1 : 0;
      }
      p[s] = v;
    }
  }
}

// The hypothesis with the highest count: a 64-bit max over count << 32 | ~loop (kFirst: among equals the FIRST,
// extras/homography.cu:249-254) or count << 32 | loop (the LAST: the reference's `>=`, extras/rigidTransform.cu:450).
// s_key [256].
template <bool kFirst>
__device__ __forceinline__ void ransac_winner(const int *__restrict__ counts, int num_loops, unsigned long long *s_key,
                                              int &best, int &best_count) {
  const int tx = threadIdx.x;
  unsigned long long key = 0;
  for (int l = tx; l < num_loops; l += kRansacThreads) {
    const unsigned int low = kFirst ? ~(unsigned int)l : (unsigned int)l;
    const unsigned long long k = ((unsigned long long)(unsigned int)counts[l] << 32) | low;
    key = k > key ? k : key;
  }
  s_key[tx] = key;
  __syncthreads();
#pragma unroll
  for (int half = kRansacThreads / 2; half > 0; half >>= 1) {
    if (tx < half) s_key[tx] = s_key[tx + half] > s_key[tx] ? s_key[tx + half] : s_key[tx];
    __syncthreads();
  }
  key = s_key[0];
  const unsigned int low = (unsigned int)(key & 0xffffffffull);
  best = (int)(kFirst ? ~low : low), best_count = (int)(unsigned int)(key >> 32);
}

// Sum of one int per thread over the workgroup; every thread gets it.  Integers: any order gives the same value.
// s_red [256].
__device__ __forceinline__ int block_sum_256(int v, int *s_red) {
  const int tx = threadIdx.x;
  s_red[tx] = v;
  __syncthreads();
#pragma unroll
  for (int half = kRansacThreads / 2; half > 0; half >>= 1) {
    if (tx < half) s_red[tx] += s_red[tx + half];
    __syncthreads();
  }
  return s_red[0];
}

// Sums s[0 .. K) over the workgroup in a fixed order -- the lane tree of every wave, then waves ((0 + 1) + 2) + 3 -- into
// s_sum, so every run gives the same bits.  s_part [4][kStride], kStride >= K.
template <int K, int kStride>
__device__ __forceinline__ void wave_tree_sum(double (&s)[K], double (*s_part)[kStride], double *s_sum, int tx) {
#pragma unroll
  for (int q = 0; q < K; ++q) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s[q] += __shfl_down(s[q], off);
  }
  __syncthreads();  // whoever still reads the previous sums is done
  if ((tx & 63) == 0) {
#pragma unroll
    for (int q = 0; q < K; ++q) s_part[tx >> 6][q] = s[q];
  }
  __syncthreads();
  if (tx < K) s_sum[tx] = ((s_part[0][tx] + s_part[1][tx]) + s_part[2][tx]) + s_part[3][tx];
  __syncthreads();
}

// The workgroup's number of keeps (ballot + popcount per wave).  s_wave [4].
__device__ __forceinline__ int keep_count_256(bool keep, int *s_wave) {
  const int tx = threadIdx.x;
  const unsigned long long m = __ballot(keep);
  if ((tx & 63) == 0) s_wave[tx >> 6] = __builtin_popcountll(m);
  __syncthreads();
  return s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
}

// Ordered compaction without atomics: the thread's rank among the workgroup's keeps in ascending thread order (ballot +
// mbcnt inside a wave, a 4-entry scan across the waves) and their number.  s_wave [4]; the caller puts a barrier in
// front of the next call with the same s_wave.
__device__ __forceinline__ int keep_rank_256(bool keep, int *s_wave, int &total) {
  const int tx = threadIdx.x;
  const unsigned long long m = __ballot(keep);
  const int rank = __builtin_amdgcn_mbcnt_hi((unsigned int)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int)m, 0u));
  total = keep_count_256(keep, s_wave);
  int wave_base = 0;
#pragma unroll
  for (int wv = 0; wv < kRansacThreads / 64; ++wv) wave_base += wv < (tx >> 6) ? s_wave[wv] : 0;
  return wave_base + rank;
}

// The array of pair blockIdx.z, `bytes` further per pair.
template <class T>
__device__ __forceinline__ T *pair_ptr(T *p, size_t bytes) {
  return (T *)((char *)p + (size_t)blockIdx.z * bytes);
}

// The number of points of this workgroup's pair: num_pts, or -- batched -- what sequence_mark_kernel left in its head
// (num_pts is then the capacity of a pair and the stride of its coordinate rows).  `head` is the pair's own.
__device__ __forceinline__ int pair_count(const int *__restrict__ head, int num_pts, PlanarBatch nb) {
  return nb.count ? min(head[kPlanarHeadCount], num_pts) : num_pts;
}

// The mark byte of a record, cand | fit << 1.  Candidate: rule 0 score > lo && amb < hi, rule 1 score < lo && amb < hi;
// both finite coordinates and a valid partner.  The refit's set: ImproveHomography's literal predicate
// (extras/homography.cu:286) under rule 0, the candidates under rule 1.  The cross-check takes what is not mutual out of
// both.
__device__ __forceinline__ unsigned char planar_marks(int rule, float score, float amb, float lo, float hi, bool finite,
                                                      bool valid, bool has_cross, bool mutual) {
  bool cand = rule == 0 ? (score > lo && amb < hi) : (score < lo && amb < hi);
  cand = cand && finite && valid;
  bool fit = rule == 0 ? !(score < lo || amb > hi) : cand;
  if (has_cross) cand = cand && mutual, fit = fit && mutual;
  return (unsigned char)((cand ? 1 : 0) | (fit ? 2 : 0));
}

// Selected pair number k: record i of frame 1 and its partner, then their coords3D as one [6] coordinate row.
__device__ __forceinline__ void write_selected(int *__restrict__ pairs, float *__restrict__ coord, int k, int i,
                                               int partner, const float *a, const float *b) {
  pairs[2 * (size_t)k + 0] = i;
  pairs[2 * (size_t)k + 1] = partner;
  float *c = coord + 6 * (size_t)k;
  c[0] = a[0], c[1] = a[1], c[2] = a[2];
  c[3] = b[0], c[4] = b[1], c[5] = b[2];
}

// Exp(w) of a rotation vector, Rodrigues' formula in fp64: E = I + A [w]x + B [w]x^2, A = sin(th) / th, B = (1 - cos(th))
// / th^2, the limits 1 and 1/2 below th^2 = 1e-20.  The PnP refit (sift_pnp.hip) and the bundle adjuster's pose update
// (sift_bundle.hip) both take their increment through this one expression.
__device__ __forceinline__ void rodrigues_exp(double w0, double w1, double w2, double (&E)[3][3]) {
  const double th2 = (w0 * w0 + w1 * w1) + w2 * w2;
  const double th = sqrt(th2);
  const bool tiny = th2 < 1e-20;
  const double A = tiny ? 1.0 : sin(th) / th, B = tiny ? 0.5 : (1.0 - cos(th)) / th2;
  E[0][0] = 1.0 - B * (w1 * w1 + w2 * w2), E[0][1] = B * (w0 * w1) - A * w2, E[0][2] = B * (w0 * w2) + A * w1;
  E[1][0] = B * (w0 * w1) + A * w2, E[1][1] = 1.0 - B * (w0 * w0 + w2 * w2), E[1][2] = B * (w1 * w2) - A * w0;
  E[2][0] = B * (w0 * w2) - A * w1, E[2][1] = B * (w1 * w2) + A * w0, E[2][2] = 1.0 - B * (w0 * w0 + w1 * w1);
}

}  // namespace cusift
