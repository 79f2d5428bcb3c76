// sift_rgbd.hip -- the two stages that were missing between extraction / matching and the rigid-transform RANSAC of
// sift_rigid.hip, so that an RGB-D frame pair goes from SiftData + depth image to [R | t] without leaving the device:
//
//   rgbd_lift_kernel          coords2D + depth image + pinhole intrinsics -> SiftPoint::coords3D (nothing in the
//                             reference writes that field; its fixtures -- depth1/2.png, INTRINSICS, match/match1_2 --
//                             pin the convention below)
//   match_select_count_kernel / match_select_write_kernel
//                             the host filter of MatchSiftData (extras/matching.cu:318-349; its own note at :318: "move
//                             this to CUDA kernel"): which records of frame 1 are matches, written in ASCENDING record
//                             order as index pairs and as the [n][6] coordinate rows the RANSAC takes, plus their count
//
// THE LIFT, all in fp32 (fx, fy, cx, cy arrive rounded to fp32):
//     u = roundf(x), v = roundf(y)                       nearest pixel, x / y 0-based at base-image scale
//     not finite, or outside [0, w) x [0, h)         ->  (0, 0, 0)
//     r = raw[v][u]; encoding 1: r = (r >> 3) | (r << 13) in 16 bits (SUN3D PNGs); encoding 0: r as it is
//     r == 0                                         ->  (0, 0, 0): z == 0 is the "no depth" mark MatchType3D tests
//     z = float(r) / units_per_metre                     a correctly rounded DIVISION, not a multiplication by 1e-3f:
//                                                        that is what reproduces the fixture's z bit for bit
//     X = ((u + origin) - cx) * z / fx,  Y = ((v + origin) - cy) * z / fy        (the product first, then the division)
// One lane per record, 8 bytes read at offset 0, one 16-bit gather, 12 bytes written at offset 576; no other byte of the
// record is touched.
//
// THE SELECTION keeps record i of frame 1 iff score < score_thresh2 && ambiguity < ambiguity_thresh2 && 0 <= match < n2
// and, for the 3-D type, coords3D[2] != 0 on both sides -- the comparisons of include/matching.h:43-58 in the same
// precision; cusift_select_mutual adds the cross-check sift2[match].match == i.
// Order-preserving compaction without atomics: every 256-record workgroup counts its keeps (keep_count_256 of
// sift_ransac.h), the second launch sums the counts of the workgroups before it, ranks its own keeps (keep_rank_256) and
// writes.  Same input, same output, every run.
// Kernels use no scratch memory and write with vector stores only.
#include "sift_ransac.h"

namespace cusift {

constexpr int kSelectThreads = 256;

__global__ void __launch_bounds__(256) rgbd_lift_kernel(cusift_point *__restrict__ points,
                                                        const unsigned int *__restrict__ counters, int max_pts,
                                                        const unsigned short *__restrict__ depth, int w, int h,
                                                        int pitch, size_t image_stride, cusift_camera cam) {
  const int img = blockIdx.y;
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int n = counters ? (int)min(counters[img], (unsigned int)max_pts) : max_pts;
  if (i >= n) return;
  cusift_point *pt = points + (size_t)img * max_pts + i;
  const float x = pt->coords2D[0], y = pt->coords2D[1];
  const float uf = roundf(x), vf = roundf(y);  // NaN and infinities fail the comparisons below
  float X = 0.0f, Y = 0.0f, Z = 0.0f;
  if (uf >= 0.0f && uf < (float)w && vf >= 0.0f && vf < (float)h) {
    const int u = (int)uf, v = (int)vf;
    unsigned int r = depth[(size_t)img * image_stride + (size_t)v * pitch + u];
    if (cam.encoding == 1) r = ((r >> 3) | (r << 13)) & 0xffffu;
    if (r != 0u) {
      Z = (float)r / cam.units_per_metre;
      X = ((uf + cam.origin) - cam.cx) * Z / cam.fx;
      Y = ((vf + cam.origin) - cam.cy) * Z / cam.fy;
    }
  }
  pt->coords3D[0] = X;
  pt->coords3D[1] = Y;
  pt->coords3D[2] = Z;
}

// include/matching.h:47-49.  `type3d`: bit 0 the 3-D type, bit 1 (cusift_select_mutual) the cross-check -- the partner's
// own match must name record i.
__device__ __forceinline__ bool match_selected(const cusift_point *__restrict__ sift1, int i, int n1,
                                               const cusift_point *__restrict__ sift2, int n2, float score_thresh2,
                                               float ambiguity_thresh2, int type3d, int &partner) {
  partner = -1;
  if (i >= n1) return false;
  const cusift_point *p = sift1 + i;
  if (!(p->score < score_thresh2 && p->ambiguity < ambiguity_thresh2)) return false;
  const int m = p->match;
  if (m < 0 || m >= n2) return false;
  if ((type3d & 1) && !(p->coords3D[2] != 0.0f && sift2[m].coords3D[2] != 0.0f)) return false;
  if ((type3d & 2) && sift2[m].match != i) return false;
  partner = m;
  return true;
}

// block_counts[b] = keeps among records [256 b, 256 b + 256)
__global__ void __launch_bounds__(kSelectThreads) match_select_count_kernel(const cusift_point *__restrict__ sift1,
                                                                            int n1,
                                                                            const cusift_point *__restrict__ sift2,
                                                                            int n2, float score_thresh2,
                                                                            float ambiguity_thresh2, int type3d,
                                                                            int *__restrict__ block_counts) {
  __shared__ int s_wave[kSelectThreads / 64];
  const int tx = threadIdx.x;
  int partner;
  const bool keep = match_selected(sift1, blockIdx.x * kSelectThreads + tx, n1, sift2, n2, score_thresh2,
                                   ambiguity_thresh2, type3d, partner);
  const int keeps = keep_count_256(keep, s_wave);
  if (tx == 0) block_counts[blockIdx.x] = keeps;
}

// pairs[k] = (i, match), coord[k] = coords3D of record i, then of its partner; the last workgroup writes *count.
__global__ void __launch_bounds__(kSelectThreads) match_select_write_kernel(const cusift_point *__restrict__ sift1,
                                                                            int n1,
                                                                            const cusift_point *__restrict__ sift2,
                                                                            int n2, float score_thresh2,
                                                                            float ambiguity_thresh2, int type3d,
                                                                            const int *__restrict__ block_counts,
                                                                            int *__restrict__ pairs,
                                                                            float *__restrict__ coord,
                                                                            int *__restrict__ count) {
  __shared__ int s_red[kSelectThreads];
  __shared__ int s_wave[kSelectThreads / 64];
  const int tx = threadIdx.x;
  int before = 0;  // keeps of the workgroups before this one
  for (int b = tx; b < (int)blockIdx.x; b += kSelectThreads) before += block_counts[b];
  const int base = block_sum_256(before, s_red);
  const int i = blockIdx.x * kSelectThreads + tx;
  int partner;
  const bool keep = match_selected(sift1, i, n1, sift2, n2, score_thresh2, ambiguity_thresh2, type3d, partner);
  int total;
  const int rank = keep_rank_256(keep, s_wave, total);
  // base + rank < n1: every keep before this one is a distinct record below i
  if (keep) write_selected(pairs, coord, base + rank, i, partner, sift1[i].coords3D, sift2[partner].coords3D);
  if (blockIdx.x == gridDim.x - 1 && tx == 0) *count = base + total;
}

}  // namespace cusift
