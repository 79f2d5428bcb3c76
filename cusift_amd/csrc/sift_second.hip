// sift_second.hip -- second-peak orientations (cusift_second_orientations_batch, cusift_ctx_set_second_orientation): a
// keypoint whose orientation histogram has a second peak above `ratio` of the first gets a second record, described at
// that peak's orientation.  The reference computes the peak and leaves the duplication compiled out
// (ComputeOrientations_D, cuSIFT_D.cu:380); the contract is include/cusift_amd_extras.h's.
// A stage BEHIND the description, three launches on the context's stream whatever the records hold:
//   second_peak_kernel      (sift_second.inc) one wave per record: the orientation stage again, the second peak's
//                           orientation -- or a NaN -- to marks[image][slot]
//   second_scan_kernel      (here) one workgroup per image: ordered prefix over the marks -> parent[image][k], the record
//                           duplicate k repeats, in ascending parent index, cut where max_pts ends; the image's number of
//                           duplicates and its new counter
//   second_describe_kernel  (sift_second.inc) one wave per duplicate: the parent's record with the new orientation,
//                           described at it
// No atomics and no append: the same input gives the same bytes.  The two wave-per-record kernels live in
// sift_keypoints.hip's unit because they call its device functions.
#include "sift_host.h"

#include "sift_ransac.h"  // keep_rank_256: the ordered compaction of the registration units

namespace cusift {

__global__ void __launch_bounds__(kRansacThreads) second_scan_kernel(const float *__restrict__ marks, int max_pts,
                                                                     unsigned int *__restrict__ counters,
                                                                     unsigned int *__restrict__ parent,
                                                                     unsigned int *__restrict__ dup_count) {
  __shared__ int s_wave[kRansacThreads / 64];
  const int i = blockIdx.x, tid = threadIdx.x;
  const unsigned int raw = counters[i];
  const int n = (int)(raw < (unsigned int)max_pts ? raw : (unsigned int)max_pts);
  const int room = max_pts - n;
  const float *mark = marks + (size_t)i * max_pts;
  unsigned int *par = parent + (size_t)i * max_pts;
  int placed = 0;  // (uniform) duplicates found so far, of which those below `room` are placed
  for (int j0 = 0; j0 < n && placed < room; j0 += kRansacThreads) {  // whole workgroups: ballots and barriers inside
    const int j = j0 + tid;
    const bool dup = j < n && (__float_as_uint(mark[j]) & 0x7fffffffu) <= 0x7f800000u;  // not a NaN
    int found;
    const int rank = placed + keep_rank_256(dup, s_wave, found);
    if (dup && rank < room) par[rank] = (unsigned int)j;  // rank < room = max_pts - n: inside the image's row
    placed += found;
    __syncthreads();  // s_wave is free for the next round
  }
  if (tid == 0) {
    const int m = placed < room ? placed : room;
    dup_count[i] = (unsigned int)m;
    counters[i] = (unsigned int)(n + m);
  }
}

}  // namespace cusift

// The stage's scratch: marks [image][max_pts] floats, parent [image][max_pts] words, dup_count [image] words.
size_t second_scratch_bytes(int n_images, int max_pts) {
  const size_t words = align_up_sz((size_t)n_images * max_pts * sizeof(unsigned int), 256);
  return 2 * words + align_up_sz((size_t)n_images * sizeof(unsigned int), 256);
}

// Enqueues the three kernels on the context's stream.  T: the pyramid the records were (or are to be) described on;
// `scratch`: second_scratch_bytes() of the arena.  The caller has checked the arguments and sized ctx->describe_grid.
int second_orientations_impl(cusift_ctx *ctx, const OctaveTable &T, cusift_point *d_points, int max_pts,
                             unsigned int *d_counters, int n_images, const cusift_params *prm, float ratio,
                             unsigned int flags, char *scratch) {
  const size_t words = align_up_sz((size_t)n_images * max_pts * sizeof(unsigned int), 256);
  float *marks = reinterpret_cast<float *>(scratch);
  unsigned int *parent = reinterpret_cast<unsigned int *>(scratch + words);
  unsigned int *dup_count = reinterpret_cast<unsigned int *>(scratch + 2 * words);
  float q, inv_q;
  frac_consts(prm->tex_frac_bits, q, inv_q);
  const dim3 grid = describe_walk_grid(ctx, n_images, max_pts);
  hipLaunchKernelGGL(second_peak_kernel, grid, dim3(64), 0, ctx->stream, T, (const cusift_point *)d_points, max_pts,
                     (const unsigned int *)d_counters, n_images, q, inv_q, ratio, flags, marks);
  TRY(check_launch("second_peak"));
  hipLaunchKernelGGL(second_scan_kernel, dim3(n_images), dim3(kRansacThreads), 0, ctx->stream, (const float *)marks,
                     max_pts, d_counters, parent, dup_count);
  TRY(check_launch("second_scan"));
  hipLaunchKernelGGL(second_describe_kernel, grid, dim3(64), 0, ctx->stream, T, d_points, max_pts,
                     (const unsigned int *)d_counters, (const unsigned int *)dup_count, (const unsigned int *)parent,
                     (const float *)marks, n_images, q, inv_q, prm->root_sift, flags);
  return check_launch("second_describe");
}

// What cusift_ctx_set_second_orientation and the stage call accept: 0 < ratio <= 1 (a NaN fails both comparisons).
static bool ratio_ok(float ratio) { return ratio > 0.0f && ratio <= 1.0f; }

// Sticky per context, read by resolve_plan (sift_driver.hip) on every extraction.
extern "C" int cusift_ctx_set_second_orientation(cusift_ctx *ctx, float ratio) {
  if (!ctx) return fail(CUSIFT_ERR_INVALID, "ctx is NULL");
  if (ratio != 0.0f && !ratio_ok(ratio))
    return fail(CUSIFT_ERR_INVALID, "second_orientation: the ratio must be 0 (off) or lie in (0, 1], got %g", (double)ratio);
  ctx->second_orientation = ratio;
  return CUSIFT_OK;
}
float cusift_second_orientation_of(const cusift_ctx *ctx) { return ctx ? ctx->second_orientation : 0.0f; }

extern "C" int cusift_second_orientations_batch(cusift_ctx *ctx, const float *d_imgs, int n_images, int w, int h, int pitch,
                                                size_t image_stride, const cusift_params *prm, cusift_point *d_points,
                                                unsigned int *d_counters, float ratio, unsigned int flags) {
  TRY(enter(ctx));
  if (!prm) return fail(CUSIFT_ERR_INVALID, "params is NULL");
  if (flags & ~(unsigned int)CUSIFT_DESCRIBE_OCTAVE_FROM_SCALE)
    return fail(CUSIFT_ERR_INVALID, "second_orientations: unknown flag bits 0x%x", flags);
  if (!ratio_ok(ratio))
    return fail(CUSIFT_ERR_INVALID, "second_orientations: the ratio must lie in (0, 1], got %g", (double)ratio);
  if (!d_counters) return fail(CUSIFT_ERR_INVALID, "second_orientations: the counters are read and written, NULL given");
  OctaveTable T;
  char *scratch = nullptr;
  bool nothing = false;
  TRY(describe_pyramid(ctx, "second_orientations", d_imgs, n_images, w, h, pitch, image_stride, prm, d_points,
                       n_images > 0 && prm->max_pts > 0 ? second_scratch_bytes(n_images, prm->max_pts) : 0, T, &scratch,
                       nothing));
  if (nothing) return CUSIFT_OK;
  return second_orientations_impl(ctx, T, d_points, prm->max_pts, d_counters, n_images, prm, ratio, flags, scratch);
}
