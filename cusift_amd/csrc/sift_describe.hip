// sift_describe.hip -- cusift_describe_batch: orientation + descriptor of keypoints the CALLER supplies (a tracker's
// predictions, reprojected map points, a dense grid, another detector's output).  The host side only: it checks the
// arguments, lays the pyramid out in the context's arena, enqueues the extraction's own pyramid launches
// (cusift_scale_up, cusift_scale_down: the same images, bit for bit) and describe_given_kernel (sift_keypoints.hip),
// which chooses every record's octave itself.  The contract is include/cusift_amd_extras.h's.
#include "sift_host.h"

// The pyramid set-up that cusift_describe_batch and cusift_second_orientations_batch (sift_second.hip) share: refuses
// the geometry cusift_extract_batch refuses, lays the octave images out in the arena with `extra_bytes` of the caller's
// scratch behind them (*extra; everything that may allocate or query the device happens before anything is enqueued),
// and enqueues the extraction's own pyramid launches.  `nothing`: n_images == 0 or max_pts == 0, no error, nothing done.
int describe_pyramid(cusift_ctx *ctx, const char *who, const float *d_imgs, int n_images, int w, int h, int pitch,
                     size_t image_stride, const cusift_params *prm, const cusift_point *d_points, size_t extra_bytes,
                     OctaveTable &T, char **extra, bool &nothing) {
  nothing = false;
  if (n_images < 0 || prm->max_pts < 0)
    return fail(CUSIFT_ERR_INVALID, "%s: n_images = %d and max_pts = %d must not be negative", who, n_images, prm->max_pts);
  if (n_images == 0 || prm->max_pts == 0) {  // nothing to do is no error
    nothing = true;
    return CUSIFT_OK;
  }
  // the geometry cusift_extract_batch refuses (resolve_plan, sift_driver.hip)
  if (w < 1 || h < 1 || pitch < w)
    return fail(CUSIFT_ERR_INVALID, "bad geometry n=%d w=%d h=%d pitch=%d", n_images, w, h, pitch);
  if (n_images > 65535) return fail(CUSIFT_ERR_INVALID, "at most 65535 images per batch (grid.y), got %d", n_images);
  if (n_images > 1 && image_stride < (size_t)h * pitch) return fail(CUSIFT_ERR_INVALID, "image_stride too small");
  if (prm->upsample && (w > (1 << 27) || h > 4 * 65535))
    return fail(CUSIFT_ERR_INVALID, "upsample: %dx%d is too large to enlarge", w, h);
  if (!d_imgs || !d_points) return fail(CUSIFT_ERR_INVALID, "%s: missing data", who);

  // the octave images of the extraction (resolve_plan): octave 0 is the caller's image or its enlargement, every
  // further one half of the one before, at a pitch of whole 128 floats, one behind the other in the arena
  memset(&T, 0, sizeof(T));
  size_t off[kMaxOctaves] = {0};
  const bool up = prm->upsample != 0;
  T.w[0] = up ? 2 * w : w;
  T.h[0] = up ? 2 * h : h;
  T.pitch[0] = up ? ialign_up(2 * w, 128) : pitch;
  T.stride[0] = up ? (long)T.h[0] * T.pitch[0] : (long)image_stride;
  T.sub[0] = up ? prm->subsampling * 0.5f : prm->subsampling;
  T.n_oct = 1;
  size_t total = up ? align_up_sz((size_t)n_images * T.stride[0] * sizeof(float), 256) : 0;
  const int n = std::max(1, std::min(prm->num_octaves, kMaxOctaves));
  for (int o = 1; o < n; ++o) {
    const int ww = T.w[o - 1] / 2, hh = T.h[o - 1] / 2;
    if (ww < 1 || hh < 1) break;
    T.w[o] = ww;
    T.h[o] = hh;
    T.pitch[o] = ialign_up(ww, 128);
    T.stride[o] = (long)hh * T.pitch[o];
    T.sub[o] = T.sub[o - 1] * 2.0f;
    off[o] = total;
    total = align_up_sz(total + (size_t)n_images * T.stride[o] * sizeof(float), 256);
    T.n_oct = o + 1;
  }
  // everything that may allocate or query the device, before anything is enqueued
  TRY(ensure_arena(ctx, total + extra_bytes));
  if (ctx->describe_grid == 0) {  // the resident blocks of describe_all_kernel (same LDS, same 4 waves per SIMD): cached
    int per_cu = 0, cus = 0;
    HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, describe_all_kernel, 64, 0));
    HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device));
    ctx->describe_grid = std::max(1, per_cu) * std::max(1, cus);
  }
  ctx->seg_clean_ptr = nullptr;  // the pyramid overwrites whatever the last extraction left in the arena

  T.base[0] = up ? (const float *)ctx->arena : d_imgs;
  for (int o = 1; o < T.n_oct; ++o) T.base[o] = (const float *)(ctx->arena + off[o]);
  if (up)
    TRY(cusift_scale_up(ctx, const_cast<float *>(T.base[0]), T.pitch[0], (size_t)T.stride[0], d_imgs, w, h, pitch,
                        image_stride, n_images));
  for (int o = 1; o < T.n_oct; ++o)
    TRY(cusift_scale_down(ctx, const_cast<float *>(T.base[o]), T.pitch[o], (size_t)T.stride[o], T.base[o - 1], T.w[o - 1],
                          T.h[o - 1], T.pitch[o - 1], (size_t)T.stride[o - 1], n_images, 0.5f));  // cuSIFT.cu:185
  if (extra) *extra = ctx->arena + total;
  return CUSIFT_OK;
}

extern "C" int cusift_describe_batch(cusift_ctx *ctx, const float *d_imgs, int n_images, int w, int h, int pitch,
                                     size_t image_stride, const cusift_params *prm, cusift_point *d_points,
                                     const unsigned int *d_counters, unsigned int flags) {
  TRY(enter(ctx));
  if (!prm) return fail(CUSIFT_ERR_INVALID, "params is NULL");
  if (flags & ~(unsigned int)(CUSIFT_DESCRIBE_KEEP_ORIENTATION | CUSIFT_DESCRIBE_OCTAVE_FROM_SCALE))
    return fail(CUSIFT_ERR_INVALID, "describe: unknown flag bits 0x%x", flags);
  OctaveTable T;
  bool nothing = false;
  TRY(describe_pyramid(ctx, "describe", d_imgs, n_images, w, h, pitch, image_stride, prm, d_points, 0, T, nullptr, nothing));
  if (nothing) return CUSIFT_OK;

  float q, inv_q;
  frac_consts(prm->tex_frac_bits, q, inv_q);
  StageTimer t(ctx, CUSIFT_STAGE_DESCRIBE_ALL);
  hipLaunchKernelGGL(describe_given_kernel, describe_walk_grid(ctx, n_images, prm->max_pts), dim3(64), 0, ctx->stream, T,
                     d_points, prm->max_pts, d_counters, n_images, q, inv_q, prm->root_sift, flags);
  return check_launch("describe_given");
}
