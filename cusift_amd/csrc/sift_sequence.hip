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
// per pair walks frame 1's records 256 at a time with a running base and ranks its keeps with keep_rank_256
// (sift_ransac.h): ascending record order, no atomics, the same output every run.  The record
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
// THE OTHER MARKINGS.  cusift_register_epipolar_batch and cusift_register_pose_batch launch sequence_mark_kernel as it is:
// the epipolar model takes the same coordinate rows and the same candidates.  cusift_register_pnp_batch launches
// sequence_pnp_mark_kernel, the same reading -- match rows, the partner's coords2D, back rows, the record count into the
// head -- with pnp_mark_kernel's (sift_pnp.hip) five coordinate rows [X | Y | Z | x2 | y2] and its depth condition: three
// finite coords3D floats in frame 1's record and Z != 0.  Both kernels are one device function, sequence_mark<kPnP>.
//
// THE CROSS-CHECK (cusift_ctx_set_cross_check).  Both kernels take rows_back[pair][max_pts], the column side that
// cusift_match_batch_mutual's kernels leave (NULL = off; the markings alike): record i stays only if back row `match` names i.  The matcher
// writes back rows 0 .. n2 - 1 of a pair with n1 > 0 and n2 > 0 and none otherwise; a back row is read only for a record
// i < n1 with 0 <= match < n2, inside the n2 > 0 branch, so no unwritten row is ever read.  In a self pair (a, a) every
// record is its own best in both directions.
// No scratch memory, vector stores only.
#include "sift_ransac_chain.h"

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
    int total;
    const int rank = keep_rank_256(keep, s_wave, total);
    // base + rank < n1: every keep before this one is a distinct record below i
    if (keep) write_selected(sel_pairs, coord, base + rank, i, partner, sift1[i].coords3D, sift2[partner].coords3D);
    base += total;
    __syncthreads();  // s_wave is rewritten by the next chunk
  }
  if (tx == 0) sel_count[pair] = base;
}

// The marking of one record of pair blockIdx.z, shared by the two kernels below: what pair_mark (sift_ransac_chain.h)
// reads from a record's match fields comes from the pair's match rows here; the predicate (mark_record) and the
// coordinate rows (write_coord_rows) are the same.  kPnP: [X | Y | Z | x2 | y2] with (X, Y, Z) = coords3D of frame 1's
// record, and the depth condition.
template <bool kPnP>
__device__ __forceinline__ void sequence_mark(const cusift_point *__restrict__ points,
                                              const unsigned int *__restrict__ counters, int max_pts,
                                              const int *__restrict__ pairs, const cusift_match_row *__restrict__ rows,
                                              int rule, float lo, float hi, float *__restrict__ coord,
                                              unsigned char *__restrict__ marks, int *__restrict__ block_counts,
                                              int *__restrict__ head, PlanarBatch nb,
                                              const cusift_match_row *__restrict__ rows_back, int *s_wave) {
  const int tx = threadIdx.x;
  const int pair = blockIdx.z;
  const int f1 = pairs[2 * pair], f2 = pairs[2 * pair + 1];
  const int n1 = frame_count(counters, f1, max_pts), n2 = frame_count(counters, f2, max_pts);
  const cusift_point *__restrict__ sift1 = points + (size_t)f1 * max_pts;
  const cusift_point *__restrict__ sift2 = points + (size_t)f2 * max_pts;
  rows += (size_t)pair * max_pts;
  coord = pair_ptr(coord, nb.scratch), marks = pair_ptr(marks, nb.scratch);
  block_counts = pair_ptr(block_counts, nb.scratch), head = pair_ptr(head, nb.head);
  const int i = blockIdx.x * kSequenceSelectThreads + tx;
  bool cand = false;
  if (i < n1) {
    const float x1 = sift1[i].coords2D[0], y1 = sift1[i].coords2D[1];
    float X = 0.0f, Y = 0.0f, Z = 0.0f;
    if (kPnP) X = sift1[i].coords3D[0], Y = sift1[i].coords3D[1], Z = sift1[i].coords3D[2];
    float x2 = 0.0f, y2 = 0.0f;
    unsigned char mk = 0;
    if (n2 > 0) {
      const f4 row = *reinterpret_cast<const f4 *>(rows + i);  // score, ambiguity, match, reserved
      const float score = row[0], amb = row[1];
      const int m = __float_as_int(row[2]);
      const bool valid = m >= 0 && m < n2;
      const cusift_point *q = sift2 + (valid ? m : 0);  // the partner cusift_match takes the position from
      x2 = q->coords2D[0], y2 = q->coords2D[1];
      bool mutual = false;
      if (rows_back) {  // the cross-check: back row m was written (i < n1, m < n2)
        const cusift_match_row *back = rows_back + (size_t)pair * max_pts + (valid ? m : 0);
        mutual = valid && __float_as_int((*reinterpret_cast<const f4 *>(back))[2]) == i;
      }
      mk = mark_record<kPnP>(rule, score, amb, lo, hi, x1, y1, x2, y2, X, Y, Z, valid, rows_back != nullptr, mutual);
      cand = mk & 1;
    }
    write_coord_rows<kPnP>(coord, max_pts, i, x1, y1, x2, y2, X, Y, Z);
    marks[i] = mk;
  }
  const int keeps = keep_count_256(cand, s_wave);
  if (tx == 0) {
    block_counts[blockIdx.x] = keeps;
    if (blockIdx.x == 0) head[kPlanarHeadCount] = n1;
  }
}

// coord [pair][4][max_pts], marks [pair][max_pts], block_counts [pair][ceil(max_pts / 256)] in the pairs' scratch blocks
// (nb.scratch bytes apart); head[kPlanarHeadCount] of pair p (nb.head bytes apart) = its record count
__global__ void __launch_bounds__(kSequenceSelectThreads) sequence_mark_kernel(
    const cusift_point *__restrict__ points, const unsigned int *__restrict__ counters, int max_pts,
    const int *__restrict__ pairs, const cusift_match_row *__restrict__ rows, int rule, float lo, float hi,
    float *__restrict__ coord, unsigned char *__restrict__ marks, int *__restrict__ block_counts, int *__restrict__ head,
    PlanarBatch nb, const cusift_match_row *__restrict__ rows_back) {
  __shared__ int s_wave[kSequenceSelectThreads / 64];
  sequence_mark<false>(points, counters, max_pts, pairs, rows, rule, lo, hi, coord, marks, block_counts, head, nb,
                       rows_back, s_wave);
}

// the same for cusift_register_pnp_batch: coord [pair][5][max_pts] = [X | Y | Z | x2 | y2], the depth condition
__global__ void __launch_bounds__(kSequenceSelectThreads) sequence_pnp_mark_kernel(
    const cusift_point *__restrict__ points, const unsigned int *__restrict__ counters, int max_pts,
    const int *__restrict__ pairs, const cusift_match_row *__restrict__ rows, int rule, float lo, float hi,
    float *__restrict__ coord, unsigned char *__restrict__ marks, int *__restrict__ block_counts, int *__restrict__ head,
    PlanarBatch nb, const cusift_match_row *__restrict__ rows_back) {
  __shared__ int s_wave[kSequenceSelectThreads / 64];
  sequence_mark<true>(points, counters, max_pts, pairs, rows, rule, lo, hi, coord, marks, block_counts, head, nb,
                      rows_back, s_wave);
}

}  // namespace cusift
