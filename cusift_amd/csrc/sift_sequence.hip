// sift_sequence.hip -- the per-pair stages of the registrations of a whole sequence that read cusift_match_batch's rows.
// The selection stage of the batched RGB-D registration (cusift_register_rgbd_batch): a batch of frames and a pair list
// in, one [R | t] per pair out, in a fixed number of launches:
//
//   rgbd_lift_kernel           (sift_rgbd.hip)   coords3D of every frame, one launch
//   match_batch_kernel         (sift_match.hip)  every pair's best / second-best, grid (row block, column split, pair)
//   match_batch_merge_kernel   (sift_match.hip)  the splits folded in column order -> rows[pair][max_pts]
//   sequence_select_kernel     (here)            the threshold filter of every pair -> pairs / coord / count per pair
//   rigid_solve / score / select (sift_rigid.hip) the RANSAC of every pair, blockIdx.z = pair
//
// THE SELECTION is match_select_*'s rule (sift_rgbd.hip; include/matching.h:43-58) read from the match rows instead of
// the records: row i of pair (f1, f2) is kept iff score < score_thresh2 && ambiguity < ambiguity_thresh2 &&
// 0 <= match < n2 and, for the 3-D type, coords3D[2] != 0 in record i of f1 and in record `match` of f2.  One workgroup
// per pair walks frame 1's records 256 at a time with a running base, ranks its keeps with ballot + mbcnt inside a wave
// and a 4-entry scan across its waves: ascending record order, no atomics, the same output every run.  The record
// counts come from device memory (frame_count); nothing is written past a pair's count.
//
// THE PLANAR MARKING (cusift_register_planar_batch) is planar_mark_kernel (sift_planar.hip) for every pair of a list in
// one launch, grid (record block, 1, pair), reading the pair's match rows instead of the records' match fields:
//
//   match_batch_kernel (+ merge)  (sift_match.hip)   rows[pair][max_pts]
//   sequence_mark_kernel          (here)             coord / marks / block counts of every pair, its count into its head
//   planar_compact / homography_solve / planar_score / planar_select (sift_planar.hip, sift_homography.hip), blockIdx.z = pair
//
// Record i of pair (f1, f2) gives x1, y1 = its coords2D and x2, y2 = coords2D of record `match` of f2 -- of record 0 when
// `match` is outside [0, n2), the value cusift_match puts into match_xpos / match_ypos (sift_match.hip) -- one 16-byte
// row and two coords2D per record.  Candidates and the refit's set follow planar_mark_kernel's predicates with num_pts2
// = n2.  A pair whose frame 2 is empty has no row (the matcher wrote none): no candidate, nothing read.  The records are
// never written.
//
// THE CROSS-CHECK (cusift_ctx_set_cross_check).  Both kernels take rows_back[pair][max_pts], the column side that
// cusift_match_batch_mutual's kernels leave (NULL = off): record i stays only if back row `match` names i.  The matcher
// writes back rows 0 .. n2 - 1 of a pair with n1 > 0 and n2 > 0 and none otherwise; a back row is read only for a record
// i < n1 with 0 <= match < n2, inside the n2 > 0 branch, so no unwritten row is ever read.  In a self pair (a, a) every
// record is its own best in both directions.
// No scratch memory, vector stores only.
#include "sift_device.h"

namespace cusift {

constexpr int kSequenceSelectThreads = 256;

// sel_pairs[pair][max_pts][2], coord[pair][max_pts][6], sel_count[pair]
__global__ void __launch_bounds__(kSequenceSelectThreads) sequence_select_kernel(
    const cusift_point *__restrict__ points, const unsigned int *__restrict__ counters, int max_pts,
    const int *__restrict__ pairs, const cusift_match_row *__restrict__ rows, float score_thresh2,
    float ambiguity_thresh2, int type3d, int *__restrict__ sel_pairs, float *__restrict__ coord,
    int *__restrict__ sel_count, const cusift_match_row *__restrict__ rows_back) {
  __shared__ int s_wave[kSequenceSelectThreads / 64];
  const int tx = threadIdx.x;
  const int pair = blockIdx.x;
  const int f1 = pairs[2 * pair], f2 = pairs[2 * pair + 1];
  const int n1 = frame_count(counters, f1, max_pts), n2 = frame_count(counters, f2, max_pts);
  const cusift_point *__restrict__ sift1 = points + (size_t)f1 * max_pts;
  const cusift_point *__restrict__ sift2 = points + (size_t)f2 * max_pts;
  rows += (size_t)pair * max_pts;
  if (rows_back) rows_back += (size_t)pair * max_pts;
  sel_pairs += 2 * (size_t)pair * max_pts;
  coord += 6 * (size_t)pair * max_pts;
  int base = 0;
  // n2 == 0: the matcher wrote no row of this pair (nothing to match, extras/matching.cu:241-242)
  for (int chunk = 0; n2 > 0 && chunk < n1; chunk += kSequenceSelectThreads) {
    const int i = chunk + tx;
    bool keep = false;
    int partner = -1;
    if (i < n1) {
      const f4 row = *reinterpret_cast<const f4 *>(rows + i);  // score, ambiguity, match, reserved
      const int m = __float_as_int(row[2]);
      keep = row[0] < score_thresh2 && row[1] < ambiguity_thresh2 && m >= 0 && m < n2;
      if (keep && type3d) keep = sift1[i].coords3D[2] != 0.0f && sift2[m].coords3D[2] != 0.0f;
      // the cross-check: back row m was written (n1 > 0, m < n2) and must name record i
      if (keep && rows_back) keep = __float_as_int((*reinterpret_cast<const f4 *>(rows_back + m))[2]) == i;
      partner = keep ? m : -1;
    }
    const unsigned long long mask = __ballot(keep);
    const int rank =
        __builtin_amdgcn_mbcnt_hi((unsigned int)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int)mask, 0u));
    if ((tx & 63) == 0) s_wave[tx >> 6] = __builtin_popcountll(mask);
    __syncthreads();
    int wave_base = 0, total = 0;
#pragma unroll
    for (int wv = 0; wv < kSequenceSelectThreads / 64; ++wv) {
      wave_base += wv < (tx >> 6) ? s_wave[wv] : 0;
      total += s_wave[wv];
    }
    if (keep) {
      const int k = base + wave_base + rank;  // < n1: every keep before this one is a distinct record below i
      sel_pairs[2 * (size_t)k + 0] = i;
      sel_pairs[2 * (size_t)k + 1] = partner;
      const float *a = sift1[i].coords3D, *b = sift2[partner].coords3D;
      float *c = coord + 6 * (size_t)k;
      c[0] = a[0], c[1] = a[1], c[2] = a[2];
      c[3] = b[0], c[4] = b[1], c[5] = b[2];
    }
    base += total;
    __syncthreads();  // s_wave is rewritten by the next chunk
  }
  if (tx == 0) sel_count[pair] = base;
}

// coord [pair][4][max_pts], marks [pair][max_pts], block_counts [pair][ceil(max_pts / 256)] in the pairs' scratch blocks
// (nb.scratch bytes apart); head[kPlanarHeadCount] of pair p (nb.head bytes apart) = its record count
__global__ void __launch_bounds__(kSequenceSelectThreads) sequence_mark_kernel(
    const cusift_point *__restrict__ points, const unsigned int *__restrict__ counters, int max_pts,
    const int *__restrict__ pairs, const cusift_match_row *__restrict__ rows, int rule, float lo, float hi,
    float *__restrict__ coord, unsigned char *__restrict__ marks, int *__restrict__ block_counts, int *__restrict__ head,
    PlanarBatch nb, const cusift_match_row *__restrict__ rows_back) {
  __shared__ int s_wave[kSequenceSelectThreads / 64];
  const int tx = threadIdx.x;
  const int pair = blockIdx.z;
  const int f1 = pairs[2 * pair], f2 = pairs[2 * pair + 1];
  const int n1 = frame_count(counters, f1, max_pts), n2 = frame_count(counters, f2, max_pts);
  const cusift_point *__restrict__ sift1 = points + (size_t)f1 * max_pts;
  const cusift_point *__restrict__ sift2 = points + (size_t)f2 * max_pts;
  rows += (size_t)pair * max_pts;
  coord = (float *)((char *)coord + (size_t)pair * nb.scratch);
  marks = (unsigned char *)((char *)marks + (size_t)pair * nb.scratch);
  block_counts = (int *)((char *)block_counts + (size_t)pair * nb.scratch);
  head = (int *)((char *)head + (size_t)pair * nb.head);
  const int i = blockIdx.x * kSequenceSelectThreads + tx;
  bool cand = false;
  if (i < n1) {
    const float x1 = sift1[i].coords2D[0], y1 = sift1[i].coords2D[1];
    float x2 = 0.0f, y2 = 0.0f;
    bool fit = false;
    if (n2 > 0) {
      const f4 row = *reinterpret_cast<const f4 *>(rows + i);  // score, ambiguity, match, reserved
      const float score = row[0], amb = row[1];
      const int m = __float_as_int(row[2]);
      const bool valid = m >= 0 && m < n2;
      const cusift_point *q = sift2 + (valid ? m : 0);  // the partner cusift_match takes the position from
      x2 = q->coords2D[0], y2 = q->coords2D[1];
      cand = rule == 0 ? (score > lo && amb < hi) : (score < lo && amb < hi);
      cand = cand && planar_finite(x1) && planar_finite(y1) && planar_finite(x2) && planar_finite(y2) && valid;
      fit = rule == 0 ? !(score < lo || amb > hi) : cand;  // as planar_mark_kernel
      if (rows_back) {  // the cross-check, as planar_mark_kernel: back row m was written (i < n1, m < n2)
        const cusift_match_row *back = rows_back + (size_t)pair * max_pts + (valid ? m : 0);
        const bool mutual = valid && __float_as_int((*reinterpret_cast<const f4 *>(back))[2]) == i;
        cand = cand && mutual;
        fit = fit && mutual;
      }
    }
    coord[i] = x1;
    coord[i + max_pts] = y1;
    coord[i + 2 * (size_t)max_pts] = x2;
    coord[i + 3 * (size_t)max_pts] = y2;
    marks[i] = (unsigned char)((cand ? 1 : 0) | (fit ? 2 : 0));
  }
  const unsigned long long mask = __ballot(cand);
  if ((tx & 63) == 0) s_wave[tx >> 6] = __builtin_popcountll(mask);
  __syncthreads();
  if (tx == 0) {
    block_counts[blockIdx.x] = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    if (blockIdx.x == 0) head[kPlanarHeadCount] = n1;
  }
}

}  // namespace cusift
