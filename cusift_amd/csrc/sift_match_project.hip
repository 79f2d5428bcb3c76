// sift_match_project.hip -- nearest neighbours under a known pose (cusift_match_projected, cusift_match_batch_projected):
// the guided search of a tracker.  Image 1's records carry map points in coords3D (cusift_lift_depth,
// cusift_register_pose); [R | t] and camera 2's intrinsics say where each of them lands in image 2; a column of image 2
// counts for a row only within `radius` pixels of that prediction.  The matcher is sift_match.hip's, from the same text
// (match_block, sift_match_block.h): the same grids, staging, LDS tile, sinks and -- with split columns -- the same merge
// kernels.  What is new is the per-row prologue of the guide: fp64, once per row, before the column loop.  The
// definition, expression by expression, is in include/cusift_amd_extras.h.
#include "sift_match_block.h"

namespace cusift {

// X1 = R X2 + t: the row's point in camera 2's frame (a, b, c) as cusift_estimate_pnp's inlier test forms it, then its
// pixel (px, py) and |x2 - p|^2 < r2, GuideH's test.  A row without depth (Z == 0), behind camera 2 or on its principal
// plane (c <= 0, or a NaN) is two NaNs: no pass for the whole row.  Lane (r, g) evaluates row 4g + (r & 3) of its wave
// and the quad exchanges, as in GuideH; the row's record is addressed under row_xy's clamp.
struct GuideP : GuideColumns {
  const ProjectModel *k;
  float px[4], py[4];
  __device__ __forceinline__ void rows(const cusift_point *__restrict__ sift1, int n1, int p1_base, int lane) {
    const float *X1 = sift1[min(p1_base + 4 * (lane >> 4) + (lane & 3), n1 - 1)].coords3D;
    const double X = X1[0], Y = X1[1], Z = X1[2];
    const double *rt = k->rt;
    const double dx = X - rt[3], dy = Y - rt[7], dz = Z - rt[11];
    const double a = (rt[0] * dx + rt[4] * dy) + rt[8] * dz;
    const double b = (rt[1] * dx + rt[5] * dy) + rt[9] * dz;
    const double c = (rt[2] * dx + rt[6] * dy) + rt[10] * dz;
    const bool usable = Z != 0.0 && c > 0.0;
    const float kNaN = __builtin_nanf("");
    const float x = usable ? (float)((k->fx * a) / c + k->px) : kNaN;
    const float y = usable ? (float)((k->fy * b) / c + k->py) : kNaN;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      px[q] = from_quad(x, lane, q);
      py[q] = from_quad(y, lane, q);
    }
  }
  __device__ __forceinline__ bool pass(int q, Column c) const {
    const float dx = c.x - px[q], dy = c.y - py[q];
    return dx * dx + dy * dy < r2;
  }
};

// match_guided_kernel (sift_match.hip) under GuideP: the model is a kernel argument
template <bool kL2>
__global__ void __launch_bounds__(256) match_projected_kernel(cusift_point *__restrict__ sift1, int n1,
                                                             const cusift_point *__restrict__ sift2, int n2,
                                                             int cols_per_split, MatchPartial *__restrict__ partials,
                                                             int n1_pad, ProjectModel model, float r2) {
  __shared__ float sB[kMatchTileCols * kBStride];
  const int col_begin = blockIdx.y * cols_per_split;
  GuideP guide;
  guide.m = model.rt;
  guide.k = &model;
  guide.r2 = r2;
  match_block<kL2>(sift1, n1, sift2, col_begin, min(col_begin + cols_per_split, n2), sB, NoColumnSide{}, guide,
                   point_sink<kL2>(partials, (size_t)blockIdx.y * n1_pad, sift1, sift2, n2));
}

// match_batch_guided_kernel under GuideP: pair blockIdx.z's model from models[pair] (a device copy of the caller's poses
// beside the one camera)
template <bool kL2>
__global__ void __launch_bounds__(256) match_batch_projected_kernel(const cusift_point *__restrict__ points,
                                                                   const unsigned int *__restrict__ counters,
                                                                   int max_pts, const int *__restrict__ pairs,
                                                                   int cols_per_split,
                                                                   MatchPartial *__restrict__ partials, int n1_pad,
                                                                   cusift_match_row *__restrict__ rows,
                                                                   const ProjectModel *__restrict__ models, float r2) {
  __shared__ float sB[kMatchTileCols * kBStride];
  const PairFrame fr(counters, pairs, max_pts, cols_per_split, kMatchRowsPerBlock);
  if (fr.empty) return;
  GuideP guide;
  guide.m = models[fr.pair].rt;
  guide.k = models + fr.pair;
  guide.r2 = r2;
  match_block<kL2>(points + (size_t)fr.f1 * max_pts, fr.n1, points + (size_t)fr.f2 * max_pts, fr.col_begin, fr.col_end,
                   sB, NoColumnSide{}, guide,
                   row_sink<kL2>(partials, ((size_t)fr.pair * gridDim.y + blockIdx.y) * n1_pad,
                                 rows + (size_t)fr.pair * max_pts));
}

#define CUSIFT_PROJECTED_KERNELS(kL2)                                                                                   \
  template __global__ void match_projected_kernel<kL2>(cusift_point *, int, const cusift_point *, int, int,              \
                                                       MatchPartial *, int, ProjectModel, float);                        \
  template __global__ void match_batch_projected_kernel<kL2>(const cusift_point *, const unsigned int *, int,            \
                                                             const int *, int, MatchPartial *, int, cusift_match_row *,  \
                                                             const ProjectModel *, float);
CUSIFT_PROJECTED_KERNELS(false)
CUSIFT_PROJECTED_KERNELS(true)
#undef CUSIFT_PROJECTED_KERNELS

}  // namespace cusift
