// sift_driver.hip -- the octave driver of the C ABI (include/cusift_amd.h): the launch policy and the plan it resolves to,
// cusift_extract_batch (SiftData::Extract + ExtractSiftLoop, cuSIFT.cu:61-120,175-270, for a batch), which enqueues a plan,
// its recorded hipGraph and the blocking single-image entry points.
#include "sift_host.h"

// ------------------------------------------------------------------------------------------------
// launch policy: what a call asks for, by the context's policy (Knobs) and the size of the call
// ------------------------------------------------------------------------------------------------
// Octave 0 beside the coarser octaves.  One extraction on one stream is a chain of launches of very different sizes:
// octave 0's detection (3/4 of the pixels), then four ScaleDowns and four detections that each fill the chip for a few
// microseconds and end in a tail.  A caller that keeps several batches in flight (cusift_params.concurrent_batches >= 2)
// covers those tails with the other batches' kernels; a lone caller -- ExtractSift as the reference calls it -- cannot.
// For it the driver forks: octave 0's detection goes to a second stream of the context and appends HEADS (64 bytes)
// to a staging list in the arena, the ScaleDown chain and the coarser detections run on the context's stream as
// before, the streams join, and describe_all_kernel moves the staged keypoints behind the coarser ones while it
// describes them -- so SiftData comes out coarsest octave first, and saturates coarsest first, exactly as before.
// Measured on MI355X (one stream, back to back; a later run: profiles/r03/octave_overlap.txt): 64 x 1080p 1.527 ->
// 1.356 ms, 16: 0.478 -> 0.429, 4: 0.213 -> 0.200 -- but ONE frame 0.132 -> 0.138 ms, and its recorded graph 0.148 ->
// 0.187: the two cross-stream waits cost more than a frame's tails.  So the fork is taken from kSideStreamMinPixels up (three 1080p
// frames), never inside a recording, never with the stage timers on (they bracket launches on one stream).
constexpr size_t kSideStreamMinPixels = 6u << 20;
static bool wants_side_stream(const cusift_ctx *ctx, const cusift_params *prm, int n_images, int w, int h) {
  const int mode = ctx->knobs.octave_overlap;  // 0 (default): the context has not been asked to fork
  if (mode == 0 || ctx->timing || ctx->knobs.force_generic || ctx->side_failed) return false;
  if (!prm->fused_detect || n_images > kMaxFlatImages) return false;
  if (mode == 3) return true;  // tests: whatever the size, also inside a recording
  if (ctx->recording) return false;
  return prm->concurrent_batches < 2 && (size_t)n_images * (size_t)w * (size_t)h >= kSideStreamMinPixels;
}

// The pyramid as a by-product of the detection (CUSIFT_POLICY_PYRAMID_IN_DETECT; detect_fused_kernel<.., kDown>): octave
// o's detection writes octave o + 1's image from its own row window, so the ScaleDown launches -- 0.2 ms of HBM-bound
// re-reading per 64 x 1080p, a fifth of a lone caller's step -- disappear for ~5 % more vector instructions in the
// detection, and the octaves are searched finest first (lists per octave).  What it costs is the one-launch detection
// of the coarser octaves: a chain of dependent launches has a tail per octave, which a caller with several batches in
// flight fills with the other batches' kernels and a lone caller does not.  Measured on MI355X
// (profiles/r05/ab_pyramid_by_size.txt; 1080p frames per call, ms per call, ScaleDown chain first -> every octave):
//   four calls in flight  1: 0.0409 -> 0.0390   3: 0.0776 -> 0.0725   8: 0.1645 -> 0.1450   16: 0.288 -> 0.267   64: 1.033 -> 0.976
//   a lone caller         1: 0.0649 -> 0.0973  16: 0.342 -> 0.392    32: 0.645 -> 0.662    48: 0.941 -> 0.932   64: 1.241 -> 1.153
// A lone caller's middle ground is "octave 0 only" (1): octave 0's detection hands octave 1 over -- the large ScaleDown is
// the one worth saving -- and the coarser octaves keep their short ScaleDown chain and their ONE launch: 32 frames
// 0.645 -> 0.640, 48: 0.941 -> 0.910 (every octave: 0.932), 64: 1.241 -> 1.152 (every octave: 1.154); 24: 0.496 -> 0.505.
// So by default: a pipelining caller (concurrent_batches >= 2) every octave from one 1080p frame's worth of pixels up
// (2,000,000: a single 1920 x 1080 frame, 2,073,600 pixels, qualifies -- until round 6 the limit was 2 << 20 = 2,097,152
// and it did not), a lone caller octave 0 only from 64,000,000 pixels per call (31 frames of 1080p).  0: never; 1: octave 0
// only; 2: every octave.
constexpr size_t kPyramidInDetectMinPixelsPipelined = 2000000, kPyramidInDetectMinPixelsLone = 64000000;
static int wants_pyramid_in_detect(const cusift_ctx *ctx, const cusift_params *prm, int n_images, int w, int h) {
  const int mode = ctx->knobs.pyramid_in_detect;
  if (mode == 0 || ctx->knobs.force_generic || ctx->knobs.stage_all == 0) return 0;
  if (!prm->fused_detect || prm->num_octaves < 2 || n_images > kMaxFlatImages) return 0;
  // (the stage timers do not change this: every launch of the finest-first sequence is a detection launch and is
  // bracketed as one -- the ScaleDown stage then simply reports no launches)
  if (mode > 0) return std::min(mode, 2);
  const size_t px = (size_t)n_images * (size_t)w * (size_t)h;
  if (prm->concurrent_batches >= 2) return px >= kPyramidInDetectMinPixelsPipelined ? 2 : 0;
  return px >= kPyramidInDetectMinPixelsLone ? 1 : 0;
}

// Every octave's keypoints to staging lists, joined by describe_all_kernel: detections no longer have to run, or end, in
// list order -- ALL octaves are searched by ONE launch (detect_multi_impl; two with octave 0 on the side stream), the
// large octave's workgroups first and the small ones in its tail.  What it buys is dispatches and tails (MI355X,
// 1080p, ms per call back to back on one stream: 1 frame 0.130 -> 0.082, 4: 0.210 -> 0.145, 16: 0.476 -> 0.389,
// 64: 1.52 -> 1.41; with four calls in flight: 1 frame 0.062 -> 0.043, 4: 0.111 -> 0.106, 16: 0.338 -> 0.343,
// 64: 1.165 -> 1.20 -- there the other batches fill the tails already and octave 0 is better off in its own, tuned
// instantiation).  So: a lone caller whenever the lists fit, a pipelining caller up to eight 1080p frames' worth of
// pixels per call.  Not with the per-octave stage sequence, the generic kernels or the stage timers on.
constexpr size_t kListsMaxPixelsPipelined = 16u << 20;
static bool wants_stage_all(const cusift_ctx *ctx, const cusift_params *prm, int n_images, int w, int h) {
  if (ctx->knobs.stage_all == 0 || ctx->knobs.force_generic) return false;
  if (!prm->fused_detect || n_images > kMaxFlatImages) return false;
  if (ctx->knobs.stage_all > 0) return true;  // tests: whenever the lists fit
  if (wants_pyramid_in_detect(ctx, prm, n_images, w, h) > 0) return true;  // finest first needs a list per octave
  if (ctx->timing) return false;  // the stage timers bracket the reference's launch-per-octave sequence
  return prm->concurrent_batches < 2 || (size_t)n_images * (size_t)w * (size_t)h <= kListsMaxPixelsPipelined;
}

// The ScaleDown chain of a small call -- levels 1 .. n from level 0 -- in ONE launch (pyramid_small_kernel).
// A call takes it up to kPyramidSmallPixels source pixels (one 1080p frame: four launches of 6-10 us become one of
// ~10); beyond that the 2.9x re-reads of the source cost more than the dispatches.  Not with the stage timers on (they
// count one ScaleDown per octave).
constexpr size_t kPyramidSmallPixels = (size_t)5 << 19;  // 2.6 Mpixel
static bool wants_small_pyramid(const cusift_ctx *ctx, int n_images, int w, int h) {
  return !ctx->knobs.force_generic && !ctx->timing && (size_t)n_images * (size_t)w * (size_t)h <= kPyramidSmallPixels;
}

// describe_all_kernel may form the lists' running sums itself (no join_counts_kernel: a small call saves the dispatch) --
// but it then finds every keypoint's list by a walk over the lists' counters, which a large call pays per keypoint
// (64 x 1080p of `blobs`, 581 k keypoints, one stream: 2.066 ms with the self-join against 1.99 with the 5-us join kernel and
// its precomputed ends).  So: small calls only.
static bool wants_self_join(int n_images, int w, int h) {
  return (size_t)n_images * (size_t)w * (size_t)h <= kPyramidSmallPixels;
}

// ------------------------------------------------------------------------------------------------
// the plan: every decision of one extraction, made here and nowhere else
// ------------------------------------------------------------------------------------------------
// The launch sequence of a plan whose geometry and arena layout are made.  `may_fork` false: the sequence of a call that
// found no side stream -- everything that follows from `forked` is decided again, on the same layout.
static void resolve_launches(Plan &pl, const cusift_ctx *ctx, const cusift_params *prm, bool may_fork) {
  const int n_images = pl.n_images, w = pl.w[0], h = pl.h[0];
  const bool generic = ctx->knobs.force_generic;
  // With fused_detect the keypoint stages run once, after the last octave's detection, over the flattened list
  // of all keypoints of the batch (describe_all_kernel); otherwise per octave like the reference.  The DETECTION
  // kernel is chosen per octave: the fused one wherever it applies (16-byte aligned rows, w >= 4, h >= 3), the
  // two-stage pair for an octave where it does not (a 2x1 coarsest octave, a caller's odd pitch) -- one such octave
  // no longer demotes the others.  Octaves >= 1 live in the arena, 256-byte aligned (ensure_arena) at a pitch of whole
  // 128 floats: of the pointers only the caller's decides, so all this is known before anything is allocated.
  pl.flat = prm->fused_detect && n_images <= kMaxFlatImages && !generic;
  pl.dog_bytes = 0;
  bool all_fused = true, any_coarser = false;
  for (int o = 0; o < pl.n_oct; ++o) {
    pl.detect[o] = kNotSearched;
    if (!(prm->lowest_scale < pl.sub[o] * 2.0f)) continue;  // cuSIFT.cu:194
    const size_t plane = (size_t)pl.h[o] * pl.p[o];
    const bool fused = prm->fused_detect && !generic &&
                       detect_fused_ok(o == 0 ? pl.img0 : nullptr, pl.w[o], pl.h[o], pl.p[o], o == 0 ? pl.stride0 : plane);
    pl.detect[o] = fused ? kFused : kTwoStage;
    if (!fused) pl.dog_bytes = std::max(pl.dog_bytes, (size_t)n_images * kNumDog * plane * sizeof(float));
    all_fused = all_fused && fused;
    any_coarser = any_coarser || o > 0;
  }
  // Where the octaves' keypoints go (sift_types.h: SegmentTable).  One stream searching coarsest first leaves SiftData
  // in list order by itself; the moment two detections may overlap -- octave 0 on the side stream, the coarser octaves
  // in one launch -- they append to lists of their own (record heads in the arena) and describe_all_kernel joins them.
  //   stage_all   every searched octave to its own list: needs the fused kernel for every searched octave
  //   forked      octave 0 to a list of its own and to the side stream; the coarser ones in place (or staged too)
  pl.stage_all = pl.flat && pl.staged_octaves == pl.n_oct && all_fused;
  pl.forked = may_fork && pl.flat && pl.fork && pl.staged_octaves >= 1 && pl.detect[0] == kFused && any_coarser;
  pl.concurrent = pl.forked ? 1 : prm->concurrent_batches;
  // The pyramid as a by-product of the detection (CUSIFT_POLICY_PYRAMID_IN_DETECT): octaves [0, chain_end) are searched
  // finest first by detections that also write the next octave's image -- images 1 .. chain_end come from there, not
  // from ScaleDown launches.  Needs a list per octave (the detections no longer run in list order) and octave 0 on the
  // context's own stream (octave 1 waits for it anyway).
  pl.chain_end = 0;
  if (pl.stage_all && !pl.forked) {
    const int mode = wants_pyramid_in_detect(ctx, prm, n_images, w, h);
    while (pl.chain_end < pl.n_oct - 1 && (mode == 2 || (mode == 1 && pl.chain_end == 0)) && pl.detect[pl.chain_end])
      pl.detect[pl.chain_end++] = kChain;
  }
  // A small call's dispatches are most of its time, so its housekeeping rides along: the ScaleDown chain in one launch
  // (which also clears the lists' counters), all octaves in one detection launch (which also clears describe_all's work
  // cursors), and describe_all_kernel joins the lists itself -- pyramid, detection, description: three dispatches.
  const bool small_pyramid = pl.n_oct >= 2 && pl.chain_end == 0 && wants_small_pyramid(ctx, n_images, w, h);
  pl.small_levels = small_pyramid ? std::min(pl.n_oct - 1, kMaxPyramidLevels) : 0;
  if (pl.forked) pl.detect[0] = kSide;
  // With a list per octave the octaves that are left (at most kMaxMultiOctaves) are searched by ONE launch, if it saves one
  const int first_rest = std::max(pl.forked ? 1 : 0, pl.chain_end);
  int n_rest = 0, n_taken = 0;
  for (int o = first_rest; o < pl.n_oct; ++o) n_rest += pl.detect[o] ? 1 : 0;
  const bool one_launch = pl.stage_all && !ctx->knobs.no_multi && n_rest >= 2;
  for (int o = first_rest; o < pl.n_oct && pl.stage_all; ++o)
    if (pl.detect[o]) pl.detect[o] = one_launch && n_taken++ < kMaxMultiOctaves ? kOneLaunch : kStaged;
  pl.self_join = one_launch && wants_self_join(n_images, w, h);
  // join_counts_kernel reads every list's counter exactly once and leaves it zero: when the previous extraction of this
  // context did that for these very counters, nothing has to be cleared now -- in a loop of equal batches no memset is
  // dispatched at all.  (A forked octave 0 may count before the pyramid runs: then the pyramid cannot clear.)
  pl.join_clears = pl.stage_all && !pl.self_join && !pl.forked;
  pl.clear = !(pl.stage_all || pl.forked) ? kNoLists : (small_pyramid && pl.stage_all && !pl.forked) ? kByPyramid : kByMemset;
  pl.n_seg_counts = (size_t)n_images * (pl.stage_all ? pl.n_oct : 1);
  // (a multiple of 64 bytes: the runtime fills an odd size with two dispatches; the region is kMaxOctaves x n_images)
  pl.seg_bytes = std::min(align_up_sz(sizeof(unsigned int) * pl.n_seg_counts, 64), sizeof(unsigned int) * n_images * kMaxOctaves);
}

// One extraction, decided (Plan, sift_host.h).  Nothing here touches the device: `d_imgs` is looked at for its alignment only
// (NULL: not known yet, as aligned as the arena).
// Octave -1 (cusift_params.upsample): octave 0 OF THE PLAN is the 2x enlarged image -- 2w x 2h at a pitch of whole 128
// floats, at the head of the arena, written by cusift_scale_up before anything else runs -- with half the caller's
// subsampling and twice its init_blur (the enlargement stretches the blur the input already has).  Everything below, the
// launch policies included, sees that image as it would see a caller's: the same plan, launch for launch, as for an
// enlarged image handed in with subsampling * 0.5 and init_blur * 2.
static int resolve_plan(Plan &pl, const cusift_ctx *ctx, const cusift_params *prm, int n_images, int w, int h, int pitch,
                        const float *d_imgs, size_t image_stride) {
  if (!prm) return fail(CUSIFT_ERR_INVALID, "params is NULL");
  if (n_images < 1 || w < 1 || h < 1 || pitch < w)
    return fail(CUSIFT_ERR_INVALID, "bad geometry n=%d w=%d h=%d pitch=%d", n_images, w, h, pitch);
  if (n_images > 65535) return fail(CUSIFT_ERR_INVALID, "at most 65535 images per batch (grid.z), got %d", n_images);
  if (prm->max_pts < 1) return fail(CUSIFT_ERR_INVALID, "max_pts must be >= 1");
  // Keep the K strongest keypoints per image (cusift_ctx_set_keep_strongest; sift_select.hip): the selection works on the
  // staged heads, so such a call takes a list per octave whatever the policy or the size of the call says -- or is refused.
  pl.keep = ctx->keep_strongest;
  if (pl.keep < 0 || pl.keep > prm->max_pts)
    return fail(CUSIFT_ERR_INVALID, "keep_strongest: K = %d must lie in 0 .. max_pts = %d", pl.keep, prm->max_pts);
  if (pl.keep && !prm->fused_detect)
    return fail(CUSIFT_ERR_INVALID, "keep_strongest: needs the keypoint lists of fused_detect = 1");
  if (pl.keep && ctx->knobs.force_generic)
    return fail(CUSIFT_ERR_INVALID, "keep_strongest: needs the keypoint lists, which CUSIFT_POLICY_GENERIC_KERNELS rules out");
  if (pl.keep && n_images > kMaxFlatImages)
    return fail(CUSIFT_ERR_INVALID, "keep_strongest: at most %d images per call, got %d", kMaxFlatImages, n_images);
  // Second-peak orientations (cusift_ctx_set_second_orientation; sift_second.hip): the stage runs behind
  // describe_all_kernel, on the pyramid that launch has read, so such a call takes the flat path -- or is refused.
  pl.second = ctx->second_orientation;
  if (pl.second != 0.0f && !prm->fused_detect)
    return fail(CUSIFT_ERR_INVALID, "second_orientation: needs the one description launch of fused_detect = 1");
  if (pl.second != 0.0f && ctx->knobs.force_generic)
    return fail(CUSIFT_ERR_INVALID, "second_orientation: needs the one description launch, which CUSIFT_POLICY_GENERIC_KERNELS rules out");
  if (pl.second != 0.0f && n_images > kMaxFlatImages)
    return fail(CUSIFT_ERR_INVALID, "second_orientation: at most %d images per call, got %d", kMaxFlatImages, n_images);
  int n = std::max(1, std::min(prm->num_octaves, kMaxOctaves));
  pl.upsample = prm->upsample != 0;
  if (pl.upsample) {
    if (w > (1 << 27) || h > 4 * 65535) return fail(CUSIFT_ERR_INVALID, "upsample: %dx%d is too large to enlarge", w, h);
    w *= 2;
    h *= 2;
    pitch = ialign_up(w, 128);
    d_imgs = nullptr;  // in the arena
    image_stride = (size_t)h * pitch;
  }
  pl.img0 = d_imgs;
  pl.stride0 = image_stride;
  pl.n_images = n_images;
  pl.w[0] = w;
  pl.h[0] = h;
  pl.p[0] = pitch;
  pl.blur[0] = pl.upsample ? 2.0 * prm->init_blur : prm->init_blur;
  pl.sub[0] = pl.upsample ? prm->subsampling * 0.5f : prm->subsampling;
  pl.n_oct = 1;
  for (int o = 1; o < n; ++o) {
    int ww = pl.w[o - 1] / 2, hh = pl.h[o - 1] / 2;  // integer division, cuSIFT.cu:182
    if (ww < 1 || hh < 1) break;
    pl.w[o] = ww;
    pl.h[o] = hh;
    pl.p[o] = ialign_up(ww, 128);  // cuSIFT.cu:183
    // cuSIFT.cu:188: float totInitBlur = (float)sqrt(initBlur*initBlur + 0.5f*0.5f) / 2.0f;
    float tot = (float)sqrt(pl.blur[o - 1] * pl.blur[o - 1] + 0.5f * 0.5f) / 2.0f;
    pl.blur[o] = tot;
    pl.sub[o] = pl.sub[o - 1] * 2.0f;
    pl.n_oct = o + 1;
  }
  pl.base_off[0] = 0;
  size_t off = pl.upsample ? align_up_sz((size_t)n_images * image_stride * sizeof(float), 256) : 0;
  for (int o = 1; o < pl.n_oct; ++o) {
    pl.base_off[o] = off;
    off = align_up_sz(off + (size_t)n_images * pl.h[o] * pl.p[o] * sizeof(float), 256);
  }
  pl.first_off = off;  // per-octave snapshots of the counters (fstPts), or the segments' counters
  off = align_up_sz(off + (size_t)n_images * kMaxOctaves * sizeof(unsigned int), 256);
  pl.seg_end_off = off;  // join_counts_kernel's running sums, [image][segment]
  off = align_up_sz(off + (size_t)n_images * kMaxOctaves * sizeof(unsigned int), 256);
  const size_t per_octave = (size_t)n_images * prm->max_pts * kStagedRecBytes;
  pl.fork = wants_side_stream(ctx, prm, n_images, w, h) && pl.n_oct >= 2 && per_octave <= kMaxStagedBytes;
  if (pl.keep && per_octave * pl.n_oct > kMaxStagedAllBytes)
    return fail(CUSIFT_ERR_INVALID, "keep_strongest: the keypoint lists (%d octaves x %d images x max_pts %d heads) exceed %zu bytes",
                pl.n_oct, n_images, prm->max_pts, kMaxStagedAllBytes);
  const bool lists = pl.keep ? true
                             : wants_stage_all(ctx, prm, n_images, w, h) && pl.n_oct >= 2 &&
                                   per_octave * pl.n_oct <= kMaxStagedAllBytes;
  pl.staged_octaves = lists ? pl.n_oct : (pl.fork ? 1 : 0);
  if (pl.staged_octaves) {
    pl.staged_off = off;
    off = align_up_sz(off + per_octave * pl.staged_octaves, 256);
  }
  if (pl.keep) {
    pl.select_off = off;
    off = align_up_sz(off + select_scratch_bytes(pl.n_oct, n_images, prm->max_pts), 256);
  }
  if (pl.second != 0.0f) {
    pl.second_off = off;
    off = align_up_sz(off + second_scratch_bytes(n_images, prm->max_pts), 256);
  }
  pl.total = off;
  resolve_launches(pl, ctx, prm, true);
  if (pl.keep && !pl.stage_all)
    return fail(CUSIFT_ERR_INVALID, "keep_strongest: an octave of this %dx%d call (pitch %d) is not one the fused detection takes, "
                "so its keypoints have no list", w, h, pitch);
  return CUSIFT_OK;
}

// Everything a resolved plan needs that may allocate, synchronise or query the device: the arena, the DoG planes of the
// two-stage octaves (sized once for the largest, before anything is enqueued), the grid of describe_all_kernel.  A second
// call for the same plan does nothing, so cusift_graph_create calls it before its capture starts.
static int prepare(cusift_ctx *ctx, const Plan &pl) {
  TRY(ensure_arena(ctx, pl.total));
  TRY(grow_scratch(ctx, ctx->dog, ctx->dog_bytes, pl.dog_bytes, "DoG ", true));
  // persistent grid = exactly the blocks that are resident at once (a larger static grid would run in
  // rounds and leave the second round's items waiting); items are interleaved over the blocks
  if (pl.flat && ctx->describe_grid == 0) {
    int per_cu = 0, cus = 0;
    HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, describe_all_kernel, 64, 0));
    HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device));
    ctx->describe_grid = std::max(1, per_cu) * std::max(1, cus);
  }
  return CUSIFT_OK;
}

// ------------------------------------------------------------------------------------------------
// the driver: enqueues what the plan says
// ------------------------------------------------------------------------------------------------
extern "C" int cusift_extract_batch(cusift_ctx *ctx, const float *d_imgs, int n_images, int w, int h, int pitch,
                                    size_t image_stride, const cusift_params *prm, cusift_point *d_points,
                                    unsigned int *d_counters) {
  TRY(enter(ctx));
  if (!d_imgs || !d_points || !d_counters) return fail(CUSIFT_ERR_INVALID, "extract: missing data");
  if (n_images > 1 && image_stride < (size_t)h * pitch) return fail(CUSIFT_ERR_INVALID, "image_stride too small");
  Plan pl;
  TRY(resolve_plan(pl, ctx, prm, n_images, w, h, pitch, d_imgs, image_stride));
  TRY(prepare(ctx, pl));
  // no stream runs beside this one: one stream (ensure_side_stream has set side_failed: later calls no longer ask)
  if (pl.forked && ensure_side_stream(ctx) != CUSIFT_OK) resolve_launches(pl, ctx, prm, false);

  StageTimer total(ctx, CUSIFT_STAGE_TOTAL);

  const float *base[kMaxOctaves];
  size_t stride[kMaxOctaves];
  base[0] = pl.upsample ? (const float *)(ctx->arena + pl.base_off[0]) : d_imgs;
  stride[0] = pl.stride0;
  // octave -1: the enlargement first, on the context's stream (a forked octave 0 waits for it through ev_fork)
  if (pl.upsample)
    TRY(cusift_scale_up(ctx, const_cast<float *>(base[0]), pl.p[0], stride[0], d_imgs, w, h, pitch, image_stride, n_images));
  for (int o = 1; o < pl.n_oct; ++o) {
    base[o] = (const float *)(ctx->arena + pl.base_off[o]);
    stride[o] = (size_t)pl.h[o] * pl.p[o];
  }
  unsigned int *first = (unsigned int *)(ctx->arena + pl.first_off);
  const size_t list_bytes = (size_t)n_images * prm->max_pts * kStagedRecBytes;
  char *const lists = ctx->arena + pl.staged_off;
  unsigned int *const seg_counts = first;  // [octave][image]: `first` is free when the keypoint stages run once
  unsigned int *const seg_end = (unsigned int *)(ctx->arena + pl.seg_end_off);
  auto list_of = [&](int o) { return reinterpret_cast<cusift_point *>(lists + (size_t)o * list_bytes); };
  auto counts_of = [&](int o) { return seg_counts + (size_t)o * n_images; };
  // the fused detection of octave o: in place, or heads to the octave's list (on the side stream; + the next octave's image)
  auto detect = [&](int o, bool staged, bool side = false, const DownOut *down = nullptr) {
    return detect_impl(ctx, base[o], pl.w[o], pl.h[o], pl.p[o], stride[o], (float)pl.blur[o], prm->peak_thresh,
                       prm->edge_thresh, pl.sub[o], staged ? list_of(o) : d_points, prm->max_pts,
                       staged ? counts_of(o) : d_counters, n_images, RowWindow{0, pl.h[o]}, 0, pl.h[o], pl.concurrent, staged,
                       side, down);
  };
  SegmentTable G;
  memset(&G, 0, sizeof(G));
  if (pl.stage_all) {
    G.n_seg = pl.n_oct;
    for (int r = 0; r < pl.n_oct; ++r) {  // list order: coarsest octave first
      const int o = pl.n_oct - 1 - r;
      G.base[r] = reinterpret_cast<const char *>(list_of(o));
      G.count[r] = counts_of(o);
    }
  } else if (pl.forked) {
    G.n_seg = 2;
    G.base[0] = nullptr;  // the coarser octaves: in place, the caller's counter
    G.count[0] = d_counters;
    G.base[1] = reinterpret_cast<const char *>(list_of(0));
    G.count[1] = seg_counts;
  }
  // cuSIFT.cu:69: point counter = 0 (with every octave staged the join writes it instead)
  if (!pl.stage_all) HIP_TRY(hipMemsetAsync(d_counters, 0, sizeof(unsigned int) * n_images, ctx->stream));
  // Not relied upon inside a recording (a replay cannot know what ran before it).
  const bool seg_clean = !ctx->recording && ctx->seg_clean_ptr == (const void *)seg_counts && ctx->seg_clean_bytes >= pl.seg_bytes;
  ctx->seg_clean_ptr = nullptr;  // whatever follows writes the arena; set again once the clearing join is enqueued
  if (pl.clear == kByMemset && !seg_clean) HIP_TRY(hipMemsetAsync(seg_counts, 0, pl.seg_bytes, ctx->stream));

  if (pl.forked) {
    ctx->forks++;
    HIP_TRY(hipEventRecord(ctx->ev_fork, ctx->stream));
    HIP_TRY(hipStreamWaitEvent(ctx->side, ctx->ev_fork, 0));
    const int rc = detect(0, true, true);
    const hipError_t e = hipEventRecord(ctx->ev_join, ctx->side);
    if (rc != CUSIFT_OK || e != hipSuccess) {
      (void)hipStreamWaitEvent(ctx->stream, ctx->ev_join, 0);  // never leave the side stream forked (a capture would not end)
      if (rc != CUSIFT_OK) return rc;
      HIP_TRY(e);
    }
  }
  // the side stream rejoins the context's stream however the work in between ends
  auto on_main = [&]() -> int {
    // ExtractSiftLoop, cuSIFT.cu:175-192: build the pyramid finest -> coarsest -- a small call's first levels in one launch
    for (int o = 0; o < pl.chain_end; ++o) {  // finest first: octave o's detection writes octave o + 1
      DownOut dn;
      dn.dst = const_cast<float *>(base[o + 1]);
      dn.pitch = pl.p[o + 1];
      dn.stride = (long)stride[o + 1];
      scale_down_taps(dn.T, 0.5f);  // cuSIFT.cu:185
      TRY(detect(o, true, false, &dn));
    }
    const bool zero = pl.clear == kByPyramid;
    if (pl.small_levels)
      TRY(pyramid_small_impl(ctx, base, pl.w, pl.h, pl.p, stride, pl.small_levels, n_images, 0.5f,
                             zero ? seg_counts : nullptr, zero ? (int)pl.n_seg_counts : 0));
    for (int o = std::max(pl.chain_end, pl.small_levels) + 1; o < pl.n_oct; ++o)
      TRY(cusift_scale_down(ctx, const_cast<float *>(base[o]), pl.p[o], stride[o], base[o - 1], pl.w[o - 1], pl.h[o - 1],
                            pl.p[o - 1], stride[o - 1], n_images, 0.5f));  // cuSIFT.cu:185
    // the one detection launch, largest octave first
    MultiOctave mo[kMaxMultiOctaves];
    int n_mo = 0;
    for (int o = 0; o < pl.n_oct; ++o)
      if (pl.detect[o] == kOneLaunch)
        mo[n_mo++] = MultiOctave{base[o], pl.w[o], pl.h[o], pl.p[o], stride[o], (float)pl.blur[o], pl.sub[o], list_of(o),
                                 counts_of(o)};
    if (n_mo)
      TRY(detect_multi_impl(ctx, mo, n_mo, prm->peak_thresh, prm->edge_thresh, prm->max_pts, n_images, pl.concurrent,
                            ctx->d_queue));
    // ... and the octaves with a launch of their own, coarsest first (the recursion unwinds: cuSIFT.cu:190-196)
    for (int o = pl.n_oct - 1; o >= 0; --o) {
      const Detect how = pl.detect[o];
      if (how != kTwoStage && how != kFused && how != kStaged) continue;
      // ExtractSiftOctave, cuSIFT.cu:204-270
      unsigned int *fst = first + (size_t)o * n_images;  // cuSIFT.cu:243 (fstPts), kept on the device
      if (!pl.flat)
        HIP_TRY(hipMemcpyAsync(fst, d_counters, sizeof(unsigned int) * n_images, hipMemcpyDeviceToDevice, ctx->stream));
      if (how != kTwoStage) {
        TRY(detect(o, how == kStaged));
      } else {
        const size_t dstride = (size_t)kNumDog * pl.h[o] * pl.p[o];
        TRY(cusift_laplace_multi(ctx, base[o], pl.w[o], pl.h[o], pl.p[o], stride[o], (float)pl.blur[o], ctx->dog, dstride,
                                 n_images));
        TRY(cusift_find_points_multi(ctx, ctx->dog, pl.w[o], pl.h[o], pl.p[o], dstride, prm->peak_thresh,
                                     prm->edge_thresh, pl.sub[o], d_points, prm->max_pts, d_counters, n_images));
      }
      if (pl.flat) continue;
      TRY(cusift_compute_orientations(ctx, base[o], pl.w[o], pl.h[o], pl.p[o], stride[o], d_points, prm->max_pts, fst,
                                      d_counters, prm->tex_frac_bits, n_images));
      TRY(descriptors_impl(ctx, base[o], pl.w[o], pl.h[o], pl.p[o], stride[o], d_points, prm->max_pts, fst, d_counters,
                           pl.sub[o], prm->tex_frac_bits, n_images, RowWindow{0, pl.h[o]}, prm->root_sift));
    }
    return CUSIFT_OK;
  };
  const int rc_main = on_main();
  if (pl.forked) {
    const hipError_t e = hipStreamWaitEvent(ctx->stream, ctx->ev_join, 0);
    if (rc_main == CUSIFT_OK) HIP_TRY(e);
  }
  if (rc_main != CUSIFT_OK || !pl.flat) return rc_main;
  // keep_strongest: every detection has appended; the lists shrink to the kept heads and their counters to the kept
  // counts before anything joins or describes them (three launches on this stream, whatever the images hold)
  if (pl.keep)
    TRY(select_strongest_impl(ctx, G, n_images, prm->max_pts, pl.keep, ctx->arena + pl.select_off, nullptr));
  OctaveTable T;
  memset(&T, 0, sizeof(T));
  T.n_oct = pl.n_oct;
  for (int o = 0; o < pl.n_oct; ++o) {
    T.base[o] = base[o];
    T.stride[o] = (long)stride[o];
    T.w[o] = pl.w[o];
    T.h[o] = pl.h[o];
    T.pitch[o] = pl.p[o];
    T.sub[o] = pl.sub[o];
  }
  float q, inv_q;
  frac_consts(prm->tex_frac_bits, q, inv_q);
  const long cap = (long)n_images * prm->max_pts;
  // a multiple of the shard count (the kernel deals items to shards by workgroup index)
  const long want = std::max(1L, std::min(cap, (long)ctx->describe_grid));
  dim3 grid((unsigned int)std::max<long>(kQueueShards, want / kQueueShards * kQueueShards));
  unsigned int *queue = ctx->d_queue;  // the kernel's work cursors, zero at launch
  if (pl.self_join) {
    // (the detection launch cleared the cursors; describe_all_kernel joins the lists itself)
  } else if (G.n_seg) {
    hipLaunchKernelGGL(join_counts_kernel, dim3(1), dim3(256), 0, ctx->stream, d_counters, G, seg_end, n_images,
                       prm->max_pts, queue, pl.join_clears ? 1 : 0);
    TRY(check_launch("join_counts"));
    if (pl.join_clears && !ctx->recording) {  // (a recording enqueues nothing: the counters are as they were)
      ctx->seg_clean_ptr = seg_counts;
      ctx->seg_clean_bytes = pl.seg_bytes;
    }
  } else {
    HIP_TRY(hipMemsetAsync(queue, 0, kQueueShards * 128, ctx->stream));
  }
  {
    StageTimer t(ctx, CUSIFT_STAGE_DESCRIBE_ALL);
    hipLaunchKernelGGL(describe_all_kernel, grid, dim3(64), 0, ctx->stream, T, d_points, prm->max_pts, d_counters,
                       n_images, q, inv_q, prm->root_sift, queue, G,
                       pl.self_join ? (const unsigned int *)nullptr : (const unsigned int *)seg_end);
    TRY(check_launch("describe_all"));
  }
  // second_orientation: the records are complete; the stage duplicates behind them, on the pyramid just read
  if (pl.second != 0.0f)
    TRY(second_orientations_impl(ctx, T, d_points, prm->max_pts, d_counters, n_images, prm, pl.second, 0u,
                                 ctx->arena + pl.second_off));
  return CUSIFT_OK;
}

// ------------------------------------------------------------------------------------------------
// replayable extraction: the launch sequence of cusift_extract_batch recorded once as a hipGraph
// ------------------------------------------------------------------------------------------------
struct cusift_graph {
  cusift_ctx *ctx = nullptr;
  hipGraph_t graph = nullptr;
  hipGraphExec_t exec = nullptr;
  unsigned long scratch_gen = 0;  // the recording refers to the context's scratch (arena, DoG planes of the
                                  // two-stage path) as it was: any later re-allocation invalidates it
  int nodes = 0;
};

extern "C" int cusift_graph_create(cusift_ctx *ctx, cusift_graph **out, const float *d_imgs, int n_images, int w, int h,
                                   int pitch, size_t image_stride, const cusift_params *prm, cusift_point *d_points,
                                   unsigned int *d_counters) {
  if (!ctx || !out) return fail(CUSIFT_ERR_INVALID, "NULL argument");
  TRY(enter(ctx));
  *out = nullptr;
  if (!ctx->stream) return fail(CUSIFT_ERR_INVALID, "graph capture needs a real stream (the context borrows the null stream)");
  // For the length of this call the context is "recording": no stage-timer events (they are not part of a recording)
  // and the one-stream launch sequence (wants_side_stream).
  struct Recording {
    cusift_ctx *c;
    bool timing;
    explicit Recording(cusift_ctx *ctx) : c(ctx), timing(ctx->timing) { c->timing = false; c->recording = true; }
    ~Recording() { c->timing = timing; c->recording = false; }
  } recording(ctx);
  // Everything that allocates or synchronises happens before the capture starts -- the side stream is found (and probed:
  // that waits), the fork and the join become edges -- so that cusift_extract_batch, which resolves the same plan,
  // finds all of it done.
  Plan pl;
  TRY(resolve_plan(pl, ctx, prm, n_images, w, h, pitch, d_imgs, image_stride));
  if (pl.forked && ensure_side_stream(ctx) != CUSIFT_OK)  // (side_failed is set now: the plan of a context that never forks)
    TRY(resolve_plan(pl, ctx, prm, n_images, w, h, pitch, d_imgs, image_stride));
  TRY(prepare(ctx, pl));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  cusift_graph *g = new cusift_graph();
  g->ctx = ctx;
  hipError_t e = hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeThreadLocal);
  if (e != hipSuccess) {
    delete g;
    return fail(CUSIFT_ERR_HIP, "hipStreamBeginCapture failed: %s", hipGetErrorString(e));
  }
  const int rc = cusift_extract_batch(ctx, d_imgs, n_images, w, h, pitch, image_stride, prm, d_points, d_counters);
  e = hipStreamEndCapture(ctx->stream, &g->graph);
  if (rc != CUSIFT_OK || e != hipSuccess || !g->graph) {
    if (g->graph) (void)hipGraphDestroy(g->graph);
    delete g;
    if (rc != CUSIFT_OK) return rc;
    return fail(CUSIFT_ERR_HIP, "hipStreamEndCapture failed: %s", hipGetErrorString(e));
  }
  e = hipGraphInstantiate(&g->exec, g->graph, nullptr, nullptr, 0);
  if (e != hipSuccess) {
    (void)hipGraphDestroy(g->graph);
    delete g;
    return fail(CUSIFT_ERR_HIP, "hipGraphInstantiate failed: %s", hipGetErrorString(e));
  }
  size_t n_nodes = 0;
  (void)hipGraphGetNodes(g->graph, nullptr, &n_nodes);
  g->nodes = (int)n_nodes;
  g->scratch_gen = ctx->scratch_gen;
  *out = g;
  return CUSIFT_OK;
}

extern "C" int cusift_graph_launch(cusift_graph *g) {
  if (!g || !g->exec) return fail(CUSIFT_ERR_INVALID, "graph is NULL");
  if (g->ctx->scratch_gen != g->scratch_gen)
    return fail(CUSIFT_ERR_INVALID,
                "the context's scratch (arena / DoG planes) was re-allocated after this graph was recorded; record it again");
  HIP_TRY(hipSetDevice(g->ctx->device));
  g->ctx->seg_clean_ptr = nullptr;  // the recording may leave its lists' counters in any state
  HIP_TRY(hipGraphLaunch(g->exec, g->ctx->stream));
  return CUSIFT_OK;
}

extern "C" int cusift_graph_nodes(cusift_graph *g) { return g ? g->nodes : 0; }

extern "C" int cusift_graph_destroy(cusift_graph *g) {
  if (!g) return CUSIFT_OK;
  if (g->exec) (void)hipGraphExecDestroy(g->exec);
  if (g->graph) (void)hipGraphDestroy(g->graph);
  delete g;
  return CUSIFT_OK;
}

extern "C" int cusift_extract(cusift_ctx *ctx, const float *d_img, int w, int h, int pitch, const cusift_params *prm,
                              cusift_point *d_points, cusift_point *h_points, int *num_pts) {
  TRY(enter(ctx));
  if (!num_pts) return fail(CUSIFT_ERR_INVALID, "num_pts is NULL");
  *num_pts = 0;
  TRY(cusift_extract_batch(ctx, d_img, 1, w, h, pitch, (size_t)h * pitch, prm, d_points, ctx->d_counter1));
  // The count travels to a pinned word of the context (a pageable destination is a staged copy under a runtime-wide
  // lock: callers on several threads serialise on it), and the records the caller most likely wants travel WITH it: as
  // many as the context's previous call returned plus an eighth, copied before the count is known -- one wait for the
  // device instead of two (the reference's order, cuSIFT.cu:107-114: count, then Synchronize()).  Whatever the guess
  // missed follows in a second copy.  Rows at and beyond numPts of the caller's buffer are unspecified, as after the
  // reference's malloc (cuSIFT.cu:24); never beyond its max_pts rows.
  HIP_TRY(hipMemcpyAsync(ctx->h_counter1, ctx->d_counter1, sizeof(unsigned int), hipMemcpyDeviceToHost, ctx->stream));
  const int guess = h_points ? (ctx->extract_guess < prm->max_pts ? ctx->extract_guess : prm->max_pts) : 0;
  if (guess > 0)
    HIP_TRY(hipMemcpyAsync(h_points, d_points, sizeof(cusift_point) * (size_t)guess, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  const unsigned int cnt = *(volatile unsigned int *)ctx->h_counter1;
  // cuSIFT.cu:107-110
  const int n = cnt < (unsigned int)prm->max_pts ? (int)cnt : prm->max_pts;
  *num_pts = n;
  if (h_points && n > guess) {  // SiftData::Synchronize, cuSIFT.cu:52-59
    HIP_TRY(hipMemcpyAsync(h_points + guess, d_points + guess, sizeof(cusift_point) * (size_t)(n - guess),
                           hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
  }
  if (h_points) ctx->extract_guess = n + n / 8 + 16;
  return CUSIFT_OK;
}

extern "C" int cusift_extract_host(cusift_ctx *ctx, const float *h_img, int w, int h, const cusift_params *prm,
                                   cusift_point *d_points, cusift_point *h_points, int *num_pts) {
  TRY(enter(ctx));
  if (!h_img) return fail(CUSIFT_ERR_INVALID, "image is NULL");
  if (w < 1 || h < 1) return fail(CUSIFT_ERR_INVALID, "bad image size %dx%d", w, h);
  const int pitch = ialign_up(w, 128);  // cuImage::AllocateWithHostMemory, cuImage.cu:11-13
  Plan pl;  // cusift_extract_batch's, but for the image's address: behind the plan's arena, as aligned as the arena is
  TRY(resolve_plan(pl, ctx, prm, 1, w, h, pitch, nullptr, (size_t)h * pitch));
  const size_t img_bytes = align_up_sz((size_t)h * pitch * sizeof(float), 256);
  TRY(ensure_arena(ctx, pl.total + img_bytes));
  float *d_img = (float *)(ctx->arena + pl.total);
  HIP_TRY(hipMemcpy2DAsync(d_img, sizeof(float) * pitch, h_img, sizeof(float) * w, sizeof(float) * w, h,
                           hipMemcpyHostToDevice, ctx->stream));
  return cusift_extract(ctx, d_img, w, h, pitch, prm, d_points, h_points, num_pts);
}

extern "C" int cusift_ctx_reserve(cusift_ctx *ctx, int n_images, int w, int h, const cusift_params *p) {
  TRY(enter(ctx));
  const int pitch = ialign_up(w, 128);
  Plan pl;
  TRY(resolve_plan(pl, ctx, p, n_images, w, h, pitch, nullptr, (size_t)h * pitch));
  // + one pitched upload image for cusift_extract_host
  return ensure_arena(ctx, pl.total + align_up_sz((size_t)h * pitch * sizeof(float), 256));
}
