// sift_register.hip -- the registration host layer of the C ABI: the matcher, FindHomography, rigid RANSAC, RGB-D
// registration, the calibrated pose, planar and epipolar registration, the absolute pose (PnP), the pair-list forms.  An entry point that reads
// results back lays its state out in the context's register_scratch, what travels back first, and ends in one copy and
// one synchronisation.  Shared: match_launch (either pair matcher), match_enqueue (a fused call's matcher), mark_launch
// (the candidate marking), pose_launch (the pose stage) and the two runners of the chain of the homography, of the
// fundamental matrix and of the absolute pose, told apart by data: ransac_run (a pair) and ransac_batch_run (a pair
// list).  The RGB-D calls run the rigid chain (rigid_launch) behind a selection.
#include "sift_host.h"

// the refusals that several entry points share; `who` is the entry point's name in the message
int check_distance(const char *who, int distance) {
  return distance == 0 || distance == 1 ? CUSIFT_OK : fail(CUSIFT_ERR_INVALID, "%s: distance must be 0 or 1", who);
}
static int check_dims(const char *who, const char *name, int type) {
  return type == 0 || type == 1 ? CUSIFT_OK : fail(CUSIFT_ERR_INVALID, "%s: %s must be 0 (2D) or 1 (3D)", who, name);
}
static int check_num_loops(const char *who, int num_loops) {
  if (num_loops >= 1 && num_loops <= (1 << 24)) return CUSIFT_OK;
  return fail(CUSIFT_ERR_INVALID, "%s: num_loops %d outside [1, 2^24]", who, num_loops);
}
static int check_thresh2(const char *who, float thresh2) {
  return thresh2 > 0.0f ? CUSIFT_OK : fail(CUSIFT_ERR_INVALID, "%s: thresh2 must be > 0", who);
}
static int check_not_nan(const char *who, float a, float b) {
  return std::isnan(a) || std::isnan(b) ? fail(CUSIFT_ERR_INVALID, "%s: a threshold is NaN", who) : CUSIFT_OK;
}
// the mutual matcher writes both record sets: their ranges must not overlap
int check_disjoint(const char *who, const cusift_point *d_sift1, int num_pts1, const cusift_point *d_sift2, int num_pts2) {
  const uintptr_t a = (uintptr_t)d_sift1, b = (uintptr_t)d_sift2;
  if (a < b + sizeof(cusift_point) * (size_t)num_pts2 && b < a + sizeof(cusift_point) * (size_t)num_pts1)
    return fail(CUSIFT_ERR_INVALID, "%s: the two record ranges overlap (both are written; match a copy)", who);
  return CUSIFT_OK;
}

// word `word` of a result head that was read back (sift_types.h names the words)
static int head_int(const char *head, int word) {
  int v;
  memcpy(&v, head + sizeof(int) * word, sizeof(v));
  return v;
}
static const float kIdentH[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};             // extras/homography.cu:184-187
static const float kIdentRt[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
static const double kIdentRtD[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};

// ------------------------------------------------------------------------------------------------
// matcher
// ------------------------------------------------------------------------------------------------
// GuideCall, the geometry of a guided match: sift_host.h (the 8-bit guided matchers share it and the four functions here)
ProjectModel project_model(const double *h_rt, const PnPCam &cam) {
  ProjectModel pm;
  memcpy(pm.rt, h_rt, sizeof(pm.rt));
  pm.fx = cam.fx, pm.fy = cam.fy, pm.px = cam.px, pm.py = cam.py;
  return pm;
}
// every refusal the guided calls add to their unguided counterparts'
int check_guide(const char *who, int model, const double *h_models, float radius) {
  if (model != CUSIFT_GUIDE_HOMOGRAPHY && model != CUSIFT_GUIDE_EPIPOLAR)
    return fail(CUSIFT_ERR_INVALID, "%s: model must be 0 (homography) or 1 (epipolar), got %d", who, model);
  if (!h_models) return fail(CUSIFT_ERR_INVALID, "%s: NULL model", who);
  return radius > 0.0f ? CUSIFT_OK : fail(CUSIFT_ERR_INVALID, "%s: radius must be > 0", who);
}

// The matcher of one pair: one launch, plus the row-side merge when the columns are split.  d_back != NULL
// (cusift_match_mutual): image 2's records again, to receive the column side -- folded from the same accumulators
// (sift_match.hip), merged when there are several row blocks.  guide != NULL (cusift_match_guided, never with d_back):
// the guided kernel, its model a kernel argument.  Both counts >= 1, the arguments are checked.
static int match_launch(cusift_ctx *ctx, cusift_point *d_sift1, int num_pts1, const cusift_point *d_sift2, int num_pts2,
                        int distance, cusift_point *d_back, const GuideCall *guide = nullptr) {
  const int row_blocks = idiv_up(num_pts1, 64);
  int splits, cols_per_split;
  TRY(matcher_split_plan(ctx, kMatcher32, num_pts1, num_pts2, 1, &splits, &cols_per_split));
  const int n1_pad = row_blocks * 64;
  MatchPartial *partials = nullptr, *col_partials = nullptr;
  if (splits > 1) {
    const size_t bytes = sizeof(MatchPartial) * (size_t)splits * n1_pad;
    TRY(grow_scratch(ctx, ctx->match_scratch, ctx->match_scratch_bytes, bytes, "", true));
    partials = ctx->match_scratch;
  }
  if (d_back && row_blocks > 1) {
    const size_t bytes = sizeof(MatchPartial) * (size_t)row_blocks * num_pts2;
    TRY(grow_scratch(ctx, ctx->match_col_scratch, ctx->match_col_scratch_bytes, bytes, "", false));
    col_partials = ctx->match_col_scratch;
  }
  const dim3 grid(row_blocks, splits);
  if (d_back)
    hipLaunchKernelGGL(distance ? match_mutual_kernel<true> : match_mutual_kernel<false>, grid, dim3(256), 0,
                       ctx->stream, d_sift1, num_pts1, d_back, num_pts2, cols_per_split, partials, n1_pad,
                       col_partials);
  else if (guide && guide->camera)
    hipLaunchKernelGGL(distance ? match_projected_kernel<true> : match_projected_kernel<false>, grid, dim3(256), 0,
                       ctx->stream, d_sift1, num_pts1, d_sift2, num_pts2, cols_per_split, partials, n1_pad,
                       project_model(guide->h_models, *guide->camera), guide->r2);
  else if (guide) {
    GuideModel model;
    memcpy(model.m, guide->h_models, sizeof(model.m));
    const auto kernel = guide->model == CUSIFT_GUIDE_EPIPOLAR
                            ? (distance ? match_guided_kernel<true, GuideF> : match_guided_kernel<false, GuideF>)
                            : (distance ? match_guided_kernel<true, GuideH> : match_guided_kernel<false, GuideH>);
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, ctx->stream, d_sift1, num_pts1, d_sift2, num_pts2, cols_per_split,
                       partials, n1_pad, model, guide->r2);
  } else
    hipLaunchKernelGGL(distance ? match_kernel<true> : match_kernel<false>, grid, dim3(256), 0, ctx->stream, d_sift1,
                       num_pts1, d_sift2, num_pts2, cols_per_split, partials, n1_pad);
  if (splits > 1)
    hipLaunchKernelGGL(match_merge_kernel, dim3(idiv_up(num_pts1, 256)), dim3(256), 0, ctx->stream, d_sift1, num_pts1,
                       d_sift2, num_pts2, distance, (const MatchPartial *)partials, n1_pad, splits);
  if (col_partials)
    hipLaunchKernelGGL(match_mutual_merge_kernel, dim3(idiv_up(num_pts2, 256)), dim3(256), 0, ctx->stream, d_back,
                       num_pts2, (const cusift_point *)d_sift1, num_pts1, distance, (const MatchPartial *)col_partials,
                       row_blocks);
  return check_launch(d_back ? "match_mutual" : guide ? (guide->camera ? "match_projected" : "match_guided") : "match");
}

extern "C" int cusift_match(cusift_ctx *ctx, cusift_point *d_sift1, int num_pts1, const cusift_point *d_sift2,
                            int num_pts2, int distance) {
  TRY(enter(ctx));
  if (num_pts1 <= 0 || num_pts2 <= 0) return CUSIFT_OK;  // extras/matching.cu:241-242: nothing to match
  if (!d_sift1 || !d_sift2) return fail(CUSIFT_ERR_INVALID, "MatchSiftData: missing data");
  TRY(check_distance("MatchSiftData", distance));
  return match_launch(ctx, d_sift1, num_pts1, d_sift2, num_pts2, distance, nullptr);
}

// cusift_match where a column that fails the geometric test against a row scores the initial value for that row.
extern "C" int cusift_match_guided(cusift_ctx *ctx, cusift_point *d_sift1, int num_pts1, const cusift_point *d_sift2,
                                   int num_pts2, int distance, int model, const double h_model[9], float radius) {
  TRY(enter(ctx));
  if (num_pts1 <= 0 || num_pts2 <= 0) return CUSIFT_OK;  // as cusift_match: nothing to match
  if (!d_sift1 || !d_sift2) return fail(CUSIFT_ERR_INVALID, "MatchGuided: missing data");
  TRY(check_distance("MatchGuided", distance));
  TRY(check_guide("MatchGuided", model, h_model, radius));
  const GuideCall guide{model, radius * radius, h_model};
  return match_launch(ctx, d_sift1, num_pts1, d_sift2, num_pts2, distance, nullptr, &guide);
}

// Both directions from one pass over the scores.  Both record sets are written, so their ranges must not overlap.
extern "C" int cusift_match_mutual(cusift_ctx *ctx, cusift_point *d_sift1, int num_pts1, cusift_point *d_sift2,
                                   int num_pts2, int distance) {
  TRY(enter(ctx));
  if (num_pts1 <= 0 || num_pts2 <= 0) return CUSIFT_OK;  // nothing to match, on either side
  if (!d_sift1 || !d_sift2) return fail(CUSIFT_ERR_INVALID, "MatchMutual: missing data");
  TRY(check_distance("MatchMutual", distance));
  TRY(check_disjoint("MatchMutual", d_sift1, num_pts1, d_sift2, num_pts2));
  return match_launch(ctx, d_sift1, num_pts1, d_sift2, num_pts2, distance, d_sift2);
}

// The matcher of a fused call `who`, behind the refusals that go with it; it stays enqueued with fewer than 8 records
// too.  Cross-check (cusift_ctx_set_cross_check): the mutual matcher, which writes the match fields of d_sift2 as well
// -- the callers' parameter keeps its const spelling -- and refuses overlapping ranges before it enqueues anything.
// *d_cross: what the marking or the selection then takes, the records of image 2 or NULL.
static int match_enqueue(cusift_ctx *ctx, const char *who, cusift_point *d_sift1, int num_pts1,
                         const cusift_point *d_sift2, int num_pts2, int distance, const cusift_point **d_cross) {
  TRY(check_distance(who, distance));
  if (num_pts2 < 0 || (num_pts2 > 0 && !d_sift2)) return fail(CUSIFT_ERR_INVALID, "%s: missing data", who);
  *d_cross = ctx->cross_check ? d_sift2 : nullptr;
  if (ctx->match_bits == 8) {  // cusift_ctx_set_match_bits: quantise both sets into the context, match the bytes
    if (num_pts1 <= 0 || num_pts2 <= 0) return CUSIFT_OK;  // as cusift_match8: nothing to match
    if (!d_sift1) return fail(CUSIFT_ERR_INVALID, "%s: missing data", who);
    if (ctx->cross_check) TRY(check_disjoint(who, d_sift1, num_pts1, d_sift2, num_pts2));
    return match8_pair_enqueue(ctx, d_sift1, num_pts1, d_sift2, num_pts2, distance,
                               ctx->cross_check ? const_cast<cusift_point *>(d_sift2) : nullptr);
  }
  if (ctx->cross_check)
    return cusift_match_mutual(ctx, d_sift1, num_pts1, const_cast<cusift_point *>(d_sift2), num_pts2, distance);
  return cusift_match(ctx, d_sift1, num_pts1, d_sift2, num_pts2, distance);
}

// ------------------------------------------------------------------------------------------------
// RANSAC homography
// ------------------------------------------------------------------------------------------------
extern "C" int cusift_find_homography(cusift_ctx *ctx, const cusift_point *d_sift, int num_pts, const int *h_rand_pts,
                                      int num_loops, float thresh, float h_homography[9], int *num_matches,
                                      float *h_all_homo, int *h_all_counts) {
  TRY(enter(ctx));
  if (!h_homography || !num_matches) return fail(CUSIFT_ERR_INVALID, "FindHomography: NULL output");
  memcpy(h_homography, kIdentH, sizeof(kIdentH));
  *num_matches = 0;
  if (!d_sift || !h_rand_pts) return fail(CUSIFT_ERR_INVALID, "FindHomography: missing data");
  if (num_pts < 1 || num_loops < 1) return fail(CUSIFT_ERR_INVALID, "FindHomography: num_pts and num_loops must be >= 1");
  for (long i = 0; i < 4L * num_loops; ++i)
    if (h_rand_pts[i] < 0 || h_rand_pts[i] >= num_pts)
      return fail(CUSIFT_ERR_INVALID, "FindHomography: sample index %d out of range [0, %d)", h_rand_pts[i], num_pts);
  ScratchLayout s;
  const size_t coord_off = s.take(sizeof(float) * 4 * (size_t)num_pts);
  const size_t rand_off = s.take(sizeof(int) * 4 * (size_t)num_loops);
  const size_t homo_off = s.take(sizeof(float) * 8 * (size_t)num_loops);
  const size_t cnt_off = s.take(sizeof(int) * (size_t)num_loops);
  TRY(grow_scratch(ctx, ctx->register_scratch, ctx->register_scratch_bytes, s.size, "", false));
  char *base = ctx->register_scratch;
  float *d_coord = at<float>(base, coord_off), *d_homo = at<float>(base, homo_off);
  int *d_rand = at<int>(base, rand_off), *d_counts = at<int>(base, cnt_off);
  HIP_TRY(hipMemcpyAsync(d_rand, h_rand_pts, sizeof(int) * 4 * (size_t)num_loops, hipMemcpyHostToDevice, ctx->stream));
  hipLaunchKernelGGL(homography_gather_kernel, dim3(idiv_up(num_pts, 256)), dim3(256), 0, ctx->stream, d_sift, num_pts,
                     d_coord);
  hipLaunchKernelGGL(homography_solve_kernel, dim3(idiv_up(num_loops, 64)), dim3(64), 0, ctx->stream, d_coord, num_pts,
                     d_rand, num_loops, d_homo, 0, 0ull, (const int *)nullptr, (const int *)nullptr, (int *)nullptr,
                     PlanarBatch{});
  hipLaunchKernelGGL(homography_test_kernel, dim3(num_loops), dim3(64), 0, ctx->stream, d_coord, num_pts, d_homo,
                     num_loops, thresh * thresh, d_counts);
  TRY(check_launch("find_homography"));
  std::vector<int> counts((size_t)num_loops);
  std::vector<float> homo(8 * (size_t)num_loops);
  HIP_TRY(hipMemcpyAsync(counts.data(), d_counts, sizeof(int) * (size_t)num_loops, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipMemcpyAsync(homo.data(), d_homo, sizeof(float) * 8 * (size_t)num_loops, hipMemcpyDeviceToHost,
                         ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  int best = -1, best_count = -1;  // extras/homography.cu:249-254: first maximum
  for (int i = 0; i < num_loops; ++i)
    if (counts[i] > best_count) {
      best_count = counts[i];
      best = i;
    }
  *num_matches = best_count;
  for (int j = 0; j < 8; ++j) h_homography[j] = homo[(size_t)j * num_loops + best];
  if (h_all_homo) memcpy(h_all_homo, homo.data(), sizeof(float) * homo.size());
  if (h_all_counts) memcpy(h_all_counts, counts.data(), sizeof(int) * counts.size());
  return CUSIFT_OK;
}

// The point splits of a RANSAC scoring launch (grid.y): `wgs` workgroups before splitting; split the points until the
// launch has ~per_cu workgroups per CU, but keep at least one `tile` of points per split.  round_to_tile: a split is a
// whole number of tiles.
static int score_splits(cusift_ctx *ctx, int num_pts, long wgs, int per_cu, int tile, bool round_to_tile,
                        int *per_split_out) {
  const long target = ((long)per_cu * ctx->num_cus + wgs - 1) / wgs;
  int splits = (int)std::max(1L, std::min(std::min(target, (long)idiv_up(num_pts, tile)), 65535L));
  const int per_split = round_to_tile ? idiv_up(idiv_up(num_pts, splits), tile) * tile : idiv_up(num_pts, splits);
  *per_split_out = per_split;
  return idiv_up(num_pts, per_split);
}

// The marking's thresholds: rule 1 compares squared scores (include/matching.h:43-44).
static float mark_thresh(int rule, float t) { return rule == 1 ? t * t : t; }

// ------------------------------------------------------------------------------------------------
// the marked-RANSAC chain (sift_planar.hip, sift_epipolar.hip, sift_pnp.hip): candidates, seeded RANSAC, refit -- its
// parts up to the planar launches; its run stands behind the pose stage, which it can take
// ------------------------------------------------------------------------------------------------
// What tells the homography, the fundamental matrix and the absolute pose apart, as data: every output is copied by its
// size.
enum RansacLaunch { kPlanarLaunch, kEpipolarLaunch, kPnPLaunch };  // planar_launch, epipolar_launch, pnp_launch
struct RansacModel {
  size_t elem, head_bytes;      // bytes of a model value -- float (H) or double (F, Rt) -- and of the result head
  int samples, values;          // of a hypothesis: the records drawn, the values kept
  int reported, min_pts;        // the values of a reported model; the fewest records or candidates that can be fitted
  int coord_rows;               // coordinate rows per record: x1 y1 x2 y2, or X Y Z x2 y2
  int head_model, head_ransac;  // where the head holds the refined and the winning model, in values (sift_types.h)
  const void *nothing;          // the model reported when there is nothing to fit: the identity, zeros, [I | 0]
  bool ccoord;                  // the block ends in the candidates' own coordinates
  bool needs_support;           // a winner that counts no point is nothing to fit either
  RansacLaunch launch;          // the four launches behind the marking; kPnPLaunch: its own marking as well
  const char *label;            // check_launch's
};
static const double kZeroF[9] = {};
static const RansacModel kHomography{sizeof(float), kPlanarHeadBytes, 4, 8, 9, 8, 4, kPlanarHeadH, kPlanarHeadR, kIdentH,
                                     false, false, kPlanarLaunch, "estimate_homography"};
static const RansacModel kFundamental{sizeof(double), kEpiHeadBytes, 8, 9, 9, 8, 4, kEpiHeadF, kEpiHeadR, kZeroF,
                                      true, false, kEpipolarLaunch, "estimate_fundamental"};
static const RansacModel kPnP{sizeof(double), kPnPHeadBytes, 6, 12, 12, 6, 5, kPnPHeadRt, kPnPHeadWin, kIdentRtD,
                              true, true, kPnPLaunch, "estimate_pnp"};

// The candidate marking over num_pts >= 1 records: coordinates, marks and block counts.  d_cross != NULL: the
// cross-check against the num_pts2 records of image 2, which carry cusift_match_mutual's fields.
static void mark_launch(cusift_ctx *ctx, const RansacModel &m, const cusift_point *d_sift, int num_pts, int num_pts2,
                        int rule, float lo, float hi, float *d_coord, unsigned char *d_marks, int *d_blocks,
                        const cusift_point *d_cross) {
  const dim3 grid(idiv_up(num_pts, 256));
  if (m.launch == kPnPLaunch)  // also wants a finite, non-zero depth, and writes the record's five rows
    hipLaunchKernelGGL(pnp_mark_kernel, grid, dim3(256), 0, ctx->stream, d_sift, num_pts, num_pts2, rule,
                       mark_thresh(rule, lo), mark_thresh(rule, hi), d_coord, d_marks, d_blocks, d_cross);
  else
    hipLaunchKernelGGL(planar_mark_kernel, grid, dim3(256), 0, ctx->stream, d_sift, num_pts, num_pts2, rule,
                       mark_thresh(rule, lo), mark_thresh(rule, hi), d_coord, d_marks, d_blocks, PlanarBatch{}, d_cross);
}

struct RansacOut {
  void *h_model, *h_ransac;  // RansacModel::reported values each
  int *num_candidates, *num_matches, *num_fit, *best_loop;
  char *h_inliers;
  int *h_drawn;
  void *h_all;
  int *h_all_counts;
};

// every refusal of cusift_estimate_homography and cusift_estimate_fundamental, and those that cusift_estimate_pnp shares
// (pnp_check), before anything is enqueued or written; `outputs`: none of the required output pointers is NULL
static int ransac_check(const char *who, bool outputs, const cusift_point *d_sift, int num_pts, int rule, float lo,
                        float hi, int num_loops, float thresh, int refine_loops, float refine_thresh) {
  if (!outputs) return fail(CUSIFT_ERR_INVALID, "%s: NULL output", who);
  if (rule != 0 && rule != 1) return fail(CUSIFT_ERR_INVALID, "%s: rule must be 0 (score > lo) or 1 (score < lo^2)", who);
  TRY(check_not_nan(who, lo, hi));
  TRY(check_num_loops(who, num_loops));
  if (!(thresh > 0.0f) || !(refine_thresh > 0.0f))
    return fail(CUSIFT_ERR_INVALID, "%s: thresh and refine_thresh must be > 0", who);
  if (refine_loops < 0) return fail(CUSIFT_ERR_INVALID, "%s: refine_loops %d < 0", who, refine_loops);
  if (num_pts < 0 || num_pts > (1 << 26)) return fail(CUSIFT_ERR_INVALID, "%s: num_pts %d outside [0, 2^26]", who, num_pts);
  if (num_pts > 0 && !d_sift) return fail(CUSIFT_ERR_INVALID, "%s: missing data", who);
  return CUSIFT_OK;
}
static int precheck(const char *who, const cusift_point *d_sift, int num_pts, int rule, float lo, float hi,
                    int num_loops, float thresh, int refine_loops, float refine_thresh, const RansacOut &o) {
  return ransac_check(who, o.h_model && o.h_ransac && o.num_candidates && o.num_matches && o.num_fit, d_sift, num_pts,
                      rule, lo, hi, num_loops, thresh, refine_loops, refine_thresh);
}

// fewer than the model's min_pts records or candidates: there is nothing to fit
static void ransac_nothing(const RansacModel &m, int num_pts, int num_loops, const RansacOut &o) {
  memcpy(o.h_model, m.nothing, m.elem * m.reported);
  memcpy(o.h_ransac, m.nothing, m.elem * m.reported);
  *o.num_candidates = 0, *o.num_matches = 0, *o.num_fit = 0;
  if (o.best_loop) *o.best_loop = 0;
  if (o.h_inliers && num_pts > 0) memset(o.h_inliers, 0, (size_t)num_pts);
  if (o.h_drawn) memset(o.h_drawn, 0, sizeof(int) * m.samples * (size_t)num_loops);
  if (o.h_all) memset(o.h_all, 0, m.elem * m.values * (size_t)num_loops);
  if (o.h_all_counts) memset(o.h_all_counts, 0, sizeof(int) * (size_t)num_loops);
}

// What one pair keeps on the device, as byte offsets into its block (PlanarBatch::scratch apart in a batch): samples,
// hypotheses and counts -- which the pair call can read back, so they come first -- then all records' coordinates,
// candidates, marks, the marking's block counts and, behind the epipolar and the PnP kernels, the candidates' own
// coordinates.
struct RansacBlock {
  size_t idx, model, counts, coord, cand, marks, blocks, ccoord, bytes;
  RansacBlock(const RansacModel &m, int num_pts, int num_loops) {
    ScratchLayout s;
    idx = s.take(sizeof(int) * m.samples * (size_t)num_loops);
    model = s.take(m.elem * m.values * (size_t)num_loops);
    counts = s.take(sizeof(int) * (size_t)num_loops);
    coord = s.take(sizeof(float) * m.coord_rows * (size_t)num_pts);
    cand = s.take(sizeof(int) * (size_t)num_pts);
    marks = s.take((size_t)num_pts);
    blocks = s.take(sizeof(int) * (size_t)idiv_up(num_pts, 256));
    ccoord = m.ccoord ? s.take(sizeof(float) * m.coord_rows * (size_t)num_pts) : 0;
    bytes = s.size;
  }
};

// The four launches behind the marking, over the block(s) at d_block.  n_pairs > 1: that many independent problems,
// PlanarBatch's strides apart, pair p drawing from seed + p; num_pts is then the capacity of a pair.
static void planar_launch(cusift_ctx *ctx, cusift_point *d_sift, int num_pts, int num_loops, float thresh,
                          int refine_loops, float refine_thresh, uint64_t seed, char *d_block, const RansacBlock &b,
                          float *d_head, char *d_flags, float *d_err, int n_pairs, PlanarBatch nb) {
  const float *d_coord = at<float>(d_block, b.coord), *d_homo = at<float>(d_block, b.model);
  const unsigned char *d_marks = at<unsigned char>(d_block, b.marks);
  int *d_counts = at<int>(d_block, b.counts), *d_cand = at<int>(d_block, b.cand);
  // scoring: 64 hypotheses per one-wave workgroup, ~8 waves per CU over all pairs, whole 64-point tiles
  const int blocks = idiv_up(num_pts, 256), loop_blocks = idiv_up(num_loops, 64);
  int pts_per_split;
  const int splits = score_splits(ctx, num_pts, (long)loop_blocks * n_pairs, 8, 64, true, &pts_per_split);
  hipLaunchKernelGGL(planar_compact_kernel, dim3(blocks, 1, n_pairs), dim3(256), 0, ctx->stream, d_marks, num_pts,
                     (const int *)at<int>(d_block, b.blocks), d_cand, (int *)d_head, nb);
  hipLaunchKernelGGL(homography_solve_kernel, dim3(loop_blocks, 1, n_pairs), dim3(64), 0, ctx->stream, d_coord, num_pts,
                     at<int>(d_block, b.idx), num_loops, at<float>(d_block, b.model), 1, (unsigned long long)seed,
                     (const int *)d_cand, (const int *)d_head + kPlanarHeadCand, d_counts, nb);
  hipLaunchKernelGGL(planar_score_kernel, dim3(loop_blocks, splits, n_pairs), dim3(64), 0, ctx->stream, d_coord, num_pts,
                     pts_per_split, d_homo, num_loops, thresh * thresh, d_counts, (const int *)d_head, nb);
  hipLaunchKernelGGL(planar_select_kernel, dim3(1, 1, n_pairs), dim3(256), 0, ctx->stream, d_sift, num_pts, d_coord,
                     d_marks, d_homo, (const int *)d_counts, num_loops, thresh * thresh, refine_loops,
                     refine_thresh * refine_thresh, d_head, d_flags, d_err, nb);
}

// ------------------------------------------------------------------------------------------------
// RANSAC rigid transform (sift_rigid.hip)
// ------------------------------------------------------------------------------------------------
// The three launches of sift_rigid.hip over d_coord[num_pts][6].  d_count == NULL: num_pts is the number of points;
// otherwise it is their capacity (the grids are sized by it) and the kernels read the number from *d_count.
// n_pairs > 1: that many independent problems, `nb` elements apart in every array, pair p drawing from seed + p.
static void rigid_launch(cusift_ctx *ctx, const float *d_coord, int num_pts, const int *d_count, int *d_idx,
                         int num_loops, int draw, float thresh2, int type, uint64_t seed, float *d_rt, int *d_counts,
                         float *d_head, char *d_flags, int n_pairs = 1, RigidBatch nb = RigidBatch{}) {
  // scoring: 256 hypotheses per workgroup, ~4 workgroups per CU, at least one 256-point tile per split
  const int loop_blocks = idiv_up(num_loops, 256);
  int pts_per_split;
  const int splits = score_splits(ctx, num_pts, (long)loop_blocks * n_pairs, 4, 256, false, &pts_per_split);
  const dim3 solve_grid(idiv_up(num_loops, 64), 1, n_pairs), score_grid(loop_blocks, splits, n_pairs);
  const dim3 select_grid(1, 1, n_pairs);
  hipLaunchKernelGGL(type == 1 ? rigid_solve_kernel<true> : rigid_solve_kernel<false>, solve_grid, dim3(64), 0,
                     ctx->stream, d_coord, num_pts, d_idx, num_loops, draw, (unsigned long long)seed, d_rt, d_counts,
                     d_count, nb);
  hipLaunchKernelGGL(rigid_score_kernel, score_grid, dim3(256), 0, ctx->stream, d_coord, num_pts, pts_per_split, d_rt,
                     num_loops, thresh2, d_counts, d_count, nb);
  hipLaunchKernelGGL(type == 1 ? rigid_select_kernel<true> : rigid_select_kernel<false>, select_grid, dim3(256), 0,
                     ctx->stream, d_coord, num_pts, d_rt, d_counts, num_loops, thresh2, d_head, d_flags, d_count, nb);
}

extern "C" int cusift_estimate_rigid(cusift_ctx *ctx, const float *h_coord, int num_pts, const int *h_indices,
                                     int num_loops, float thresh2, int type, uint64_t seed, float h_rt[12],
                                     int *num_inliers, int *best_loop, char *h_inliers, float *h_all_rt,
                                     int *h_all_counts, int *h_drawn) {
  TRY(enter(ctx));
  if (!h_rt || !num_inliers) return fail(CUSIFT_ERR_INVALID, "EstimateRigidTransform: NULL output");
  if (!h_coord) return fail(CUSIFT_ERR_INVALID, "EstimateRigidTransform: missing data");
  TRY(check_dims("EstimateRigidTransform", "type", type));
  const int used = type == 1 ? 3 : 2;  // the 2-D estimate never reads a hypothesis' third sample
  const int min_pts = h_indices ? used : 3;  // drawing takes three distinct points for either type
  if (num_pts < min_pts || num_pts > (1 << 26))
    return fail(CUSIFT_ERR_INVALID, "EstimateRigidTransform: num_pts %d outside [%d, 2^26]", num_pts, min_pts);
  TRY(check_num_loops("EstimateRigidTransform", num_loops));
  TRY(check_thresh2("EstimateRigidTransform", thresh2));
  if (h_indices)
    for (int l = 0; l < num_loops; ++l)
      for (int i = 0; i < used; ++i) {
        const int v = h_indices[3 * (size_t)l + i];
        if (v < 0 || v >= num_pts)
          return fail(CUSIFT_ERR_INVALID, "EstimateRigidTransform: sample index %d out of range [0, %d)", v, num_pts);
      }
  // [head | flags | hypotheses | counts | samples] is what travels back, in one copy; the coordinates come last
  ScratchLayout s;
  s.take(kRigidHeadBytes);  // the head, at 0
  const size_t flag_off = s.take((size_t)num_pts);
  const size_t rt_off = s.take(sizeof(float) * 12 * (size_t)num_loops);
  const size_t cnt_off = s.take(sizeof(int) * (size_t)num_loops);
  const size_t idx_off = s.take(sizeof(int) * 3 * (size_t)num_loops);
  const size_t coord_off = s.take(sizeof(float) * 6 * (size_t)num_pts);
  TRY(grow_scratch(ctx, ctx->register_scratch, ctx->register_scratch_bytes, s.size, "", false));
  char *base = ctx->register_scratch;
  float *d_coord = at<float>(base, coord_off);
  int *d_idx = at<int>(base, idx_off);
  HIP_TRY(hipMemcpyAsync(d_coord, h_coord, sizeof(float) * 6 * (size_t)num_pts, hipMemcpyHostToDevice, ctx->stream));
  if (h_indices)
    HIP_TRY(hipMemcpyAsync(d_idx, h_indices, sizeof(int) * 3 * (size_t)num_loops, hipMemcpyHostToDevice, ctx->stream));
  rigid_launch(ctx, d_coord, num_pts, nullptr, d_idx, num_loops, h_indices ? 0 : 1, thresh2, type, seed,
               at<float>(base, rt_off), at<int>(base, cnt_off), (float *)base, base + flag_off);
  TRY(check_launch("estimate_rigid"));
  // the one blocking read-back
  const bool all = h_all_rt || h_all_counts || h_drawn;
  std::vector<char> back(all ? coord_off : (h_inliers ? rt_off : flag_off));
  HIP_TRY(hipMemcpyAsync(back.data(), base, back.size(), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  memcpy(h_rt, back.data(), sizeof(float) * 12);
  *num_inliers = head_int(back.data(), kRigidHeadInliers);
  if (best_loop) *best_loop = head_int(back.data(), kRigidHeadLoop);
  if (h_inliers) memcpy(h_inliers, back.data() + flag_off, (size_t)num_pts);
  if (h_all_rt) memcpy(h_all_rt, back.data() + rt_off, sizeof(float) * 12 * (size_t)num_loops);
  if (h_all_counts) memcpy(h_all_counts, back.data() + cnt_off, sizeof(int) * (size_t)num_loops);
  if (h_drawn) memcpy(h_drawn, back.data() + idx_off, sizeof(int) * 3 * (size_t)num_loops);
  return CUSIFT_OK;
}

// ------------------------------------------------------------------------------------------------
// RGB-D registration (sift_rgbd.hip): depth lift, match selection, the fused frame-pair call
// ------------------------------------------------------------------------------------------------
// the intrinsics alone: all that the calibrated pose looks at
static int check_pinhole(const cusift_camera *cam, const char *who) {
  if (!std::isfinite(cam->fx) || !std::isfinite(cam->fy) || cam->fx == 0.0f || cam->fy == 0.0f ||
      !std::isfinite(cam->cx) || !std::isfinite(cam->cy) || !std::isfinite(cam->origin))
    return fail(CUSIFT_ERR_INVALID, "%s: fx and fy must be finite and not 0, cx / cy / origin finite", who);
  return CUSIFT_OK;
}
static int check_camera(const cusift_camera *cam, const char *who) {
  if (!cam) return fail(CUSIFT_ERR_INVALID, "%s: NULL camera", who);
  TRY(check_pinhole(cam, who));
  if (!(cam->units_per_metre > 0.0f) || !std::isfinite(cam->units_per_metre))
    return fail(CUSIFT_ERR_INVALID, "%s: units_per_metre must be > 0", who);
  if (cam->encoding != 0 && cam->encoding != 1)
    return fail(CUSIFT_ERR_INVALID, "%s: encoding must be 0 (plain) or 1 (rotated by 3 bits)", who);
  return CUSIFT_OK;
}

static int check_depth_geometry(int w, int h, int pitch, size_t image_stride, int n_images, const char *who) {
  if (w < 1 || h < 1 || w > (1 << 24) || h > (1 << 24) || pitch < w)
    return fail(CUSIFT_ERR_INVALID, "%s: depth image %d x %d, pitch %d", who, w, h, pitch);
  if (n_images > 1 && image_stride < (size_t)(h - 1) * (size_t)pitch + (size_t)w)
    return fail(CUSIFT_ERR_INVALID, "%s: image stride %zu is smaller than one image", who, image_stride);
  return CUSIFT_OK;
}

extern "C" int cusift_lift_depth(cusift_ctx *ctx, cusift_point *d_points, const unsigned int *d_counters, int n_images,
                                 int max_pts, const uint16_t *d_depth, int width, int height, int pitch_elems,
                                 size_t image_stride_elems, const cusift_camera *camera) {
  TRY(enter(ctx));
  TRY(check_camera(camera, "LiftDepth"));
  if (n_images < 0 || n_images > 65535 || max_pts < 0)
    return fail(CUSIFT_ERR_INVALID, "LiftDepth: n_images %d outside [0, 65535] or max_pts %d < 0", n_images, max_pts);
  if (n_images == 0 || max_pts == 0) return CUSIFT_OK;
  if (!d_points || !d_depth) return fail(CUSIFT_ERR_INVALID, "LiftDepth: missing data");
  TRY(check_depth_geometry(width, height, pitch_elems, image_stride_elems, n_images, "LiftDepth"));
  hipLaunchKernelGGL(rgbd_lift_kernel, dim3(idiv_up(max_pts, 256), n_images), dim3(256), 0, ctx->stream, d_points,
                     d_counters, max_pts, (const unsigned short *)d_depth, width, height, pitch_elems,
                     image_stride_elems, *camera);
  return check_launch("lift_depth");
}

// the two launches of the selection; d_blocks: idiv_up(n1, 256) ints.  n1 >= 1.
static void select_launch(cusift_ctx *ctx, const cusift_point *d_sift1, int n1, const cusift_point *d_sift2, int n2,
                          float score_thresh, float ambiguity_thresh, int type, int *d_blocks, int *d_pairs,
                          float *d_coord, int *d_count) {
  const float s2 = score_thresh * score_thresh, a2 = ambiguity_thresh * ambiguity_thresh;  // include/matching.h:43-44
  const int blocks = idiv_up(n1, 256);
  hipLaunchKernelGGL(match_select_count_kernel, dim3(blocks), dim3(256), 0, ctx->stream, d_sift1, n1, d_sift2, n2, s2,
                     a2, type, d_blocks);
  hipLaunchKernelGGL(match_select_write_kernel, dim3(blocks), dim3(256), 0, ctx->stream, d_sift1, n1, d_sift2, n2, s2,
                     a2, type, d_blocks, d_pairs, d_coord, d_count);
}

// cusift_select_matches and cusift_select_mutual; `who` is the entry point's name in the messages
static int select_impl(cusift_ctx *ctx, const char *who, bool mutual, const cusift_point *d_sift1, int num_pts1,
                       const cusift_point *d_sift2, int num_pts2, float score_thresh, float ambiguity_thresh, int type,
                       int *d_pairs, float *d_coord, int *d_count) {
  TRY(enter(ctx));
  if (!d_count) return fail(CUSIFT_ERR_INVALID, "%s: NULL d_count", who);
  TRY(check_dims(who, "type", type));
  if (num_pts1 < 0 || num_pts2 < 0 || num_pts1 > (1 << 26))
    return fail(CUSIFT_ERR_INVALID, "%s: num_pts1 %d outside [0, 2^26] or num_pts2 %d < 0", who, num_pts1, num_pts2);
  TRY(check_not_nan(who, score_thresh, ambiguity_thresh));
  if (num_pts1 == 0) {
    HIP_TRY(hipMemsetAsync(d_count, 0, sizeof(int), ctx->stream));
    return CUSIFT_OK;
  }
  if (!d_sift1 || (!d_sift2 && num_pts2 > 0) || !d_pairs || !d_coord)
    return fail(CUSIFT_ERR_INVALID, "%s: missing data", who);
  // the per-workgroup keep counts
  TRY(grow_scratch(ctx, ctx->register_scratch, ctx->register_scratch_bytes, sizeof(int) * (size_t)idiv_up(num_pts1, 256),
                   "", false));
  select_launch(ctx, d_sift1, num_pts1, d_sift2, num_pts2, score_thresh, ambiguity_thresh, type | (mutual ? 2 : 0),
                (int *)ctx->register_scratch, d_pairs, d_coord, d_count);
  return check_launch(mutual ? "select_mutual" : "select_matches");
}

extern "C" int cusift_select_matches(cusift_ctx *ctx, const cusift_point *d_sift1, int num_pts1,
                                     const cusift_point *d_sift2, int num_pts2, float score_thresh,
                                     float ambiguity_thresh, int type, int *d_pairs, float *d_coord, int *d_count) {
  return select_impl(ctx, "SelectMatches", false, d_sift1, num_pts1, d_sift2, num_pts2, score_thresh, ambiguity_thresh,
                     type, d_pairs, d_coord, d_count);
}

// cusift_select_matches plus the cross-check: record i is kept only if d_sift2[match].match == i
extern "C" int cusift_select_mutual(cusift_ctx *ctx, const cusift_point *d_sift1, int num_pts1,
                                    const cusift_point *d_sift2, int num_pts2, float score_thresh,
                                    float ambiguity_thresh, int type, int *d_pairs, float *d_coord, int *d_count) {
  return select_impl(ctx, "SelectMutual", true, d_sift1, num_pts1, d_sift2, num_pts2, score_thresh, ambiguity_thresh,
                     type, d_pairs, d_coord, d_count);
}

extern "C" int cusift_register_rgbd(cusift_ctx *ctx, cusift_point *d_sift1, int num_pts1, const uint16_t *d_depth1,
                                    cusift_point *d_sift2, int num_pts2, const uint16_t *d_depth2, int width,
                                    int height, int pitch_elems, const cusift_camera *camera, int distance,
                                    float score_thresh, float ambiguity_thresh, int num_loops, float thresh2,
                                    int rigid_type, uint64_t seed, float h_rt[12], int *num_matches, int *num_inliers,
                                    int *h_pairs, char *h_inliers) {
  TRY(enter(ctx));
  if (!h_rt || !num_matches || !num_inliers) return fail(CUSIFT_ERR_INVALID, "RegisterRGBD: NULL output");
  TRY(check_camera(camera, "RegisterRGBD"));
  TRY(check_dims("RegisterRGBD", "rigid_type", rigid_type));
  TRY(check_distance("RegisterRGBD", distance));
  if (num_pts1 < 0 || num_pts2 < 0 || num_pts1 > (1 << 26))
    return fail(CUSIFT_ERR_INVALID, "RegisterRGBD: num_pts1 %d outside [0, 2^26] or num_pts2 %d < 0", num_pts1, num_pts2);
  TRY(check_num_loops("RegisterRGBD", num_loops));
  TRY(check_thresh2("RegisterRGBD", thresh2));
  TRY(check_not_nan("RegisterRGBD", score_thresh, ambiguity_thresh));
  if ((num_pts1 > 0 && (!d_sift1 || !d_depth1)) || (num_pts2 > 0 && (!d_sift2 || !d_depth2)))
    return fail(CUSIFT_ERR_INVALID, "RegisterRGBD: missing data");
  TRY(check_depth_geometry(width, height, pitch_elems, 0, 1, "RegisterRGBD"));
  const bool cross = ctx->cross_check != 0;  // cusift_ctx_set_cross_check: refuse what the mutual matcher refuses, first
  if (cross && num_pts1 > 0 && num_pts2 > 0) TRY(check_disjoint("RegisterRGBD", d_sift1, num_pts1, d_sift2, num_pts2));
  const int n1 = num_pts1;
  // [head | flags | pairs] is what travels back, in one copy; behind it what stays on the device, the selection's count
  // in a 256-byte slot of its own at the end
  ScratchLayout s;
  s.take(kRigidHeadBytes);  // the head, at 0
  const size_t flag_off = s.take((size_t)std::max(n1, 1));
  const size_t pair_off = s.take(sizeof(int) * 2 * (size_t)n1);
  const size_t rt_off = s.take(sizeof(float) * 12 * (size_t)num_loops);
  const size_t cnt_off = s.take(sizeof(int) * (size_t)num_loops);
  const size_t idx_off = s.take(sizeof(int) * 3 * (size_t)num_loops);
  const size_t coord_off = s.take(sizeof(float) * 6 * (size_t)n1);
  const size_t block_off = s.take(sizeof(int) * (size_t)idiv_up(std::max(n1, 1), 256));
  const size_t count_off = s.take(256);
  TRY(grow_scratch(ctx, ctx->register_scratch, ctx->register_scratch_bytes, s.size, "", false));
  char *base = ctx->register_scratch;
  float *d_coord = at<float>(base, coord_off);
  int *d_count = at<int>(base, count_off);
  if (n1 > 0)
    hipLaunchKernelGGL(rgbd_lift_kernel, dim3(idiv_up(n1, 256), 1), dim3(256), 0, ctx->stream, d_sift1, nullptr, n1,
                       (const unsigned short *)d_depth1, width, height, pitch_elems, (size_t)0, *camera);
  if (num_pts2 > 0)
    hipLaunchKernelGGL(rgbd_lift_kernel, dim3(idiv_up(num_pts2, 256), 1), dim3(256), 0, ctx->stream, d_sift2, nullptr,
                       num_pts2, (const unsigned short *)d_depth2, width, height, pitch_elems, (size_t)0, *camera);
  TRY(check_launch("register_rgbd lift"));
  if (n1 == 0 || num_pts2 == 0) {  // nothing to match (extras/matching.cu:241-242); known from the arguments alone
    memcpy(h_rt, kIdentRt, sizeof(kIdentRt));
    *num_matches = 0;
    *num_inliers = 0;
    HIP_TRY(hipStreamSynchronize(ctx->stream));  // blocking like the full route: the depth images may be freed
    return CUSIFT_OK;
  }
  // the matcher as the other fused calls enqueue it; with the cross-check the selection takes its bit as well
  const cusift_point *d_cross;
  TRY(match_enqueue(ctx, "RegisterRGBD", d_sift1, n1, d_sift2, num_pts2, distance, &d_cross));
  select_launch(ctx, d_sift1, n1, d_sift2, num_pts2, score_thresh, ambiguity_thresh, d_cross ? 1 | 2 : 1,
                at<int>(base, block_off), at<int>(base, pair_off), d_coord, d_count);
  rigid_launch(ctx, d_coord, n1, d_count, at<int>(base, idx_off), num_loops, 1, thresh2, rigid_type, seed,
               at<float>(base, rt_off), at<int>(base, cnt_off), (float *)base, base + flag_off);
  TRY(check_launch("register_rgbd"));
  // the one blocking read-back
  std::vector<char> back(h_pairs ? rt_off : (h_inliers ? pair_off : flag_off));
  HIP_TRY(hipMemcpyAsync(back.data(), base, back.size(), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  const int n = std::min(std::max(head_int(back.data(), kRigidHeadCount), 0), n1);
  memcpy(h_rt, back.data(), sizeof(float) * 12);
  *num_inliers = head_int(back.data(), kRigidHeadInliers);
  *num_matches = n;
  if (h_inliers) memcpy(h_inliers, back.data() + flag_off, (size_t)n);
  if (h_pairs) memcpy(h_pairs, back.data() + pair_off, sizeof(int) * 2 * (size_t)n);
  return CUSIFT_OK;
}

// ------------------------------------------------------------------------------------------------
// calibrated two-view pose (sift_pose.hip): the stage behind the epipolar selection -- [R | t], coords3D -- one read-back
// ------------------------------------------------------------------------------------------------
struct PoseOut {
  double *h_rt;
  int *num_front, *h_votes;
  double *h_sigma;
};
// One call's pose stage: what its two kernels take besides the epipolar state, and the pose head as it was read back.
struct PoseStage {
  PoseCams cams;
  float thresh;
  PoseOut out;
  char back[kPoseHeadBytes];
};

// every refusal that the pose adds to the epipolar calls'; camera2 == NULL: both views use camera1.  units_per_metre and
// encoding belong to the depth image and are not looked at
static int pose_check(const char *who, const cusift_camera *camera1, const cusift_camera *camera2, const PoseOut &o) {
  if (!camera1 || !o.h_rt || !o.num_front) return fail(CUSIFT_ERR_INVALID, "%s: NULL camera or output", who);
  TRY(check_pinhole(camera1, who));
  return camera2 ? check_pinhole(camera2, who) : CUSIFT_OK;
}
static PoseStage pose_stage(const cusift_camera *camera1, const cusift_camera *camera2, float thresh, const PoseOut &o) {
  const cusift_camera *c2 = camera2 ? camera2 : camera1;
  PoseStage st{};
  st.cams = PoseCams{(double)camera1->fx, (double)camera1->fy, (double)camera1->cx - (double)camera1->origin,
                     (double)camera1->cy - (double)camera1->origin, (double)c2->fx, (double)c2->fy,
                     (double)c2->cx - (double)c2->origin, (double)c2->cy - (double)c2->origin};
  st.thresh = thresh;
  st.out = o;
  return st;
}

// The pose heads zeroed and the two launches, n_pairs and nb as planar_launch.  d_head: the epipolar head(s) with F at
// kEpiHeadF.  d_xyz != NULL: the points go there, not into coords3D.  num_pts == 0: one workgroup, which writes the head.
static int pose_launch(cusift_ctx *ctx, cusift_point *d_sift, int num_pts, const float *d_coord,
                       const unsigned char *d_marks, const int *d_head, const PoseCams &cams, float thresh, int *d_pose,
                       float *d_xyz, int n_pairs, PlanarBatch nb) {
  const dim3 grid(std::max(idiv_up(num_pts, 256), 1), 1, n_pairs);
  HIP_TRY(hipMemsetAsync(d_pose, 0, kPoseHeadBytes * (size_t)n_pairs, ctx->stream));
  hipLaunchKernelGGL(pose_vote_kernel, grid, dim3(256), 0, ctx->stream, d_coord, d_marks, num_pts, d_head, cams, thresh,
                     d_pose, nb);
  hipLaunchKernelGGL(pose_write_kernel, grid, dim3(256), 0, ctx->stream, d_sift, d_coord, d_marks, num_pts, d_head, cams,
                     thresh, d_pose, d_xyz, nb);
  return CUSIFT_OK;
}

// The pair call's stage: pose_launch and the head's copy to the host -- adjacent to the caller's one read-back, in front
// of its one synchronisation.
static int pose_enqueue(cusift_ctx *ctx, cusift_point *d_sift, int num_pts, const float *d_coord,
                        const unsigned char *d_marks, const int *d_head, int *d_pose, PoseStage &st) {
  TRY(pose_launch(ctx, d_sift, num_pts, d_coord, d_marks, d_head, st.cams, st.thresh, d_pose, nullptr, 1, PlanarBatch{}));
  HIP_TRY(hipMemcpyAsync(st.back, d_pose, kPoseHeadBytes, hipMemcpyDeviceToHost, ctx->stream));
  return CUSIFT_OK;
}

// after the synchronisation: a pose head that was read back into entry p of the caller's outputs (a pair call: 0)
static void pose_report(const char *head, const PoseOut &o, size_t p = 0) {
  memcpy(o.h_rt + 12 * p, head + sizeof(double) * kPoseHeadRt, sizeof(double) * 12);
  o.num_front[p] = head_int(head, kPoseHeadFront);
  if (o.h_votes) memcpy(o.h_votes + 4 * p, head + sizeof(int) * kPoseHeadVotes, sizeof(int) * 4);
  if (o.h_sigma) memcpy(o.h_sigma + 3 * p, head + sizeof(double) * kPoseHeadSigma, sizeof(double) * 3);
}
static void pose_nothing(const PoseOut &o, size_t p) {  // no frames to look at: [I | 0], nothing in front, no votes
  memcpy(o.h_rt + 12 * p, kIdentRtD, sizeof(kIdentRtD));
  o.num_front[p] = 0;
  if (o.h_votes) memset(o.h_votes + 4 * p, 0, sizeof(int) * 4);
  if (o.h_sigma) memset(o.h_sigma + 3 * p, 0, sizeof(double) * 3);
}

// The staged route: F from the host, the marking, the pose stage; the arguments are checked.
static int pose_run(cusift_ctx *ctx, cusift_point *d_sift, int num_pts, int num_pts2, int rule, float lo, float hi,
                    const double *h_fundamental, PoseStage &st) {
  // [epipolar head | pose head] in front, behind them what stays on the device
  ScratchLayout s;
  s.take(kEpiHeadBytes);  // the head, at 0: only F is filled in
  const size_t pose_off = s.take(kPoseHeadBytes);
  const size_t coord_off = s.take(sizeof(float) * 4 * (size_t)num_pts);
  const size_t mark_off = s.take((size_t)num_pts);
  const size_t block_off = s.take(sizeof(int) * (size_t)idiv_up(num_pts, 256));
  TRY(grow_scratch(ctx, ctx->register_scratch, ctx->register_scratch_bytes, s.size, "", false));
  char *base = ctx->register_scratch;
  HIP_TRY(hipMemcpyAsync(base + sizeof(double) * kEpiHeadF, h_fundamental, sizeof(double) * 9, hipMemcpyHostToDevice,
                         ctx->stream));
  if (num_pts > 0)
    mark_launch(ctx, kFundamental, d_sift, num_pts, num_pts2, rule, lo, hi, at<float>(base, coord_off),
                at<unsigned char>(base, mark_off), at<int>(base, block_off), nullptr);
  TRY(pose_enqueue(ctx, d_sift, num_pts, at<float>(base, coord_off), at<unsigned char>(base, mark_off), (const int *)base,
                   at<int>(base, pose_off), st));
  TRY(check_launch("estimate_pose"));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  pose_report(st.back, st.out);
  return CUSIFT_OK;
}

extern "C" int cusift_estimate_pose(cusift_ctx *ctx, cusift_point *d_sift, int num_pts, int num_pts2, int rule, float lo,
                                    float hi, const double h_fundamental_in[9], float thresh,
                                    const cusift_camera *camera1, const cusift_camera *camera2, double h_rt[12],
                                    int *num_front, int *h_votes, double *h_sigma) {
  TRY(enter(ctx));
  const PoseOut o{h_rt, num_front, h_votes, h_sigma};
  TRY(pose_check("EstimatePose", camera1, camera2, o));
  TRY(ransac_check("EstimatePose", h_fundamental_in != nullptr, d_sift, num_pts, rule, lo, hi, 1, thresh, 0, thresh));
  PoseStage st = pose_stage(camera1, camera2, thresh, o);
  return pose_run(ctx, d_sift, num_pts, num_pts2, rule, lo, hi, h_fundamental_in, st);
}

// ------------------------------------------------------------------------------------------------
// the epipolar and the PnP launches, the run of the marked-RANSAC chain, and planar and epipolar registration on it --
// one read-back
// ------------------------------------------------------------------------------------------------
// The four launches behind the marking, over the block(s) at d_block; n_pairs and nb as planar_launch.
static void epipolar_launch(cusift_ctx *ctx, cusift_point *d_sift, int num_pts, int num_loops, float thresh,
                            int refine_loops, float refine_thresh, uint64_t seed, char *d_block, const RansacBlock &b,
                            int *d_head, char *d_flags, float *d_err, int n_pairs, PlanarBatch nb) {
  const float *d_coord = at<float>(d_block, b.coord);
  float *d_ccoord = at<float>(d_block, b.ccoord);
  const unsigned char *d_marks = at<unsigned char>(d_block, b.marks);
  double *d_fund = at<double>(d_block, b.model);
  int *d_counts = at<int>(d_block, b.counts), *d_cand = at<int>(d_block, b.cand);
  // scoring: as planar_launch, over the candidates -- at most num_pts of them, the number stays on the device
  const int blocks = idiv_up(num_pts, 256), loop_blocks = idiv_up(num_loops, 64);
  int per_split;
  const int splits = score_splits(ctx, num_pts, (long)loop_blocks * n_pairs, 8, 64, true, &per_split);
  hipLaunchKernelGGL(planar_compact_kernel, dim3(blocks, 1, n_pairs), dim3(256), 0, ctx->stream, d_marks, num_pts,
                     (const int *)at<int>(d_block, b.blocks), d_cand, d_head, nb);
  hipLaunchKernelGGL(epipolar_solve_kernel, dim3(loop_blocks, 1, n_pairs), dim3(64), 0, ctx->stream, d_coord, num_pts,
                     (const int *)d_cand, (const int *)d_head, (unsigned long long)seed, num_loops,
                     at<int>(d_block, b.idx), d_fund, d_counts, d_ccoord, nb);
  hipLaunchKernelGGL(epipolar_score_kernel, dim3(loop_blocks, splits, n_pairs), dim3(64), 0, ctx->stream,
                     (const float *)d_ccoord, num_pts, per_split, (const double *)d_fund, num_loops, thresh, d_counts,
                     (const int *)d_head, nb);
  hipLaunchKernelGGL(epipolar_select_kernel, dim3(1, 1, n_pairs), dim3(256), 0, ctx->stream, d_sift, num_pts, d_coord,
                     (const float *)d_ccoord, d_marks, (const double *)d_fund, (const int *)d_counts, num_loops, thresh,
                     refine_loops, refine_thresh, d_head, d_flags, d_err, nb);
}

// The four launches behind the marking, over the block(s) at d_block: the candidates' 3-D points against their matches'
// pixels in the image of `cam` (sift_pnp.hip); n_pairs and nb as planar_launch.
static void pnp_launch(cusift_ctx *ctx, cusift_point *d_sift, int num_pts, int num_loops, float thresh, int refine_loops,
                       float refine_thresh, uint64_t seed, PnPCam cam, char *d_block, const RansacBlock &b, int *d_head,
                       char *d_flags, float *d_err, int n_pairs, PlanarBatch nb) {
  const float *d_coord = at<float>(d_block, b.coord);
  float *d_ccoord = at<float>(d_block, b.ccoord);
  const unsigned char *d_marks = at<unsigned char>(d_block, b.marks);
  double *d_pose = at<double>(d_block, b.model);
  int *d_counts = at<int>(d_block, b.counts), *d_cand = at<int>(d_block, b.cand);
  // scoring: as epipolar_launch, over the candidates of every pair
  const int blocks = idiv_up(num_pts, 256), loop_blocks = idiv_up(num_loops, 64);
  int cand_per_split;
  const int splits = score_splits(ctx, num_pts, (long)loop_blocks * n_pairs, 8, 64, true, &cand_per_split);
  hipLaunchKernelGGL(planar_compact_kernel, dim3(blocks, 1, n_pairs), dim3(256), 0, ctx->stream, d_marks, num_pts,
                     (const int *)at<int>(d_block, b.blocks), d_cand, d_head, nb);
  hipLaunchKernelGGL(pnp_solve_kernel, dim3(loop_blocks, 1, n_pairs), dim3(64), 0, ctx->stream, d_coord, num_pts,
                     (const int *)d_cand, (const int *)d_head, (unsigned long long)seed, num_loops, cam,
                     at<int>(d_block, b.idx), d_pose, d_counts, d_ccoord, nb);
  hipLaunchKernelGGL(pnp_score_kernel, dim3(loop_blocks, splits, n_pairs), dim3(64), 0, ctx->stream,
                     (const float *)d_ccoord, num_pts, cand_per_split, (const double *)d_pose, num_loops, cam, thresh,
                     d_counts, (const int *)d_head, nb);
  hipLaunchKernelGGL(pnp_select_kernel, dim3(1, 1, n_pairs), dim3(256), 0, ctx->stream, d_sift, num_pts, d_coord,
                     (const float *)d_ccoord, d_marks, (const double *)d_pose, (const int *)d_counts, num_loops, cam,
                     thresh, refine_loops, refine_thresh, d_head, d_flags, d_err, nb);
}

// The marking, the model's four launches and the one read-back; the arguments are checked.  d_cross as mark_launch's.
// pose != NULL (cusift_register_pose, on F): its stage behind the selection, at refine_thresh, its head last.
// cam: the matches' camera, which kPnP alone takes.
static int ransac_run(cusift_ctx *ctx, const RansacModel &m, cusift_point *d_sift, int num_pts, int num_pts2, int rule,
                      float lo, float hi, int num_loops, float thresh, int refine_loops, float refine_thresh,
                      uint64_t seed, const RansacOut &o, const cusift_point *d_cross, PoseStage *pose = nullptr,
                      const PnPCam *cam = nullptr) {
  if (num_pts < m.min_pts) {  // fewer than the solver takes (extras/homography.cu:205): the answer needs no device work
    ransac_nothing(m, num_pts, num_loops, o);
    // a pose stage still owes coords3D of the records: the staged route from the nine zeros just reported
    return pose ? pose_run(ctx, d_sift, num_pts, num_pts2, rule, lo, hi, (const double *)o.h_model, *pose) : CUSIFT_OK;
  }
  // [head | flags | samples | hypotheses | counts] is what travels back, in one copy; behind it what stays on the device
  const RansacBlock b(m, num_pts, num_loops);
  ScratchLayout s;
  s.take(m.head_bytes);  // the head, at 0
  const size_t flag_off = s.take((size_t)num_pts);
  const size_t block_off = s.take(b.bytes);
  const size_t pose_off = pose ? s.take(kPoseHeadBytes) : 0;
  TRY(grow_scratch(ctx, ctx->register_scratch, ctx->register_scratch_bytes, s.size, "", false));
  char *base = ctx->register_scratch, *d_block = base + block_off;
  mark_launch(ctx, m, d_sift, num_pts, num_pts2, rule, lo, hi, at<float>(d_block, b.coord),
              at<unsigned char>(d_block, b.marks), at<int>(d_block, b.blocks), d_cross);
  if (m.launch == kPlanarLaunch)
    planar_launch(ctx, d_sift, num_pts, num_loops, thresh, refine_loops, refine_thresh, seed, d_block, b, (float *)base,
                  base + flag_off, nullptr, 1, PlanarBatch{});
  else if (m.launch == kEpipolarLaunch)
    epipolar_launch(ctx, d_sift, num_pts, num_loops, thresh, refine_loops, refine_thresh, seed, d_block, b, (int *)base,
                    base + flag_off, nullptr, 1, PlanarBatch{});
  else
    pnp_launch(ctx, d_sift, num_pts, num_loops, thresh, refine_loops, refine_thresh, seed, *cam, d_block, b, (int *)base,
               base + flag_off, nullptr, 1, PlanarBatch{});
  if (pose)
    TRY(pose_enqueue(ctx, d_sift, num_pts, at<float>(d_block, b.coord), at<unsigned char>(d_block, b.marks),
                     (const int *)base, at<int>(base, pose_off), *pose));
  TRY(check_launch(m.label));
  // the one blocking read-back
  const bool all = o.h_drawn || o.h_all || o.h_all_counts;
  std::vector<char> back(all ? block_off + b.coord : (o.h_inliers ? block_off : flag_off));
  HIP_TRY(hipMemcpyAsync(back.data(), base, back.size(), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  if (pose) pose_report(pose->back, pose->out);
  const char *head = back.data(), *block = back.data() + block_off;
  const int n_cand = head_int(head, kPlanarHeadCand);
  // extras/homography.cu:220; the kernels left the records alone
  if (n_cand < m.min_pts || (m.needs_support && head_int(head, kPlanarHeadMatches) < 1)) {
    ransac_nothing(m, num_pts, num_loops, o);
    *o.num_candidates = n_cand;
    return CUSIFT_OK;
  }
  memcpy(o.h_model, head + m.elem * m.head_model, m.elem * m.reported);
  memcpy(o.h_ransac, head + m.elem * m.head_ransac, m.elem * m.reported);
  *o.num_candidates = n_cand, *o.num_matches = head_int(head, kPlanarHeadMatches);
  *o.num_fit = head_int(head, kPlanarHeadFit);
  if (o.best_loop) *o.best_loop = head_int(head, kPlanarHeadLoop);
  if (o.h_inliers) memcpy(o.h_inliers, back.data() + flag_off, (size_t)num_pts);
  if (o.h_drawn) memcpy(o.h_drawn, block + b.idx, sizeof(int) * m.samples * (size_t)num_loops);
  if (o.h_all) memcpy(o.h_all, block + b.model, m.elem * m.values * (size_t)num_loops);
  if (o.h_all_counts) memcpy(o.h_all_counts, block + b.counts, sizeof(int) * (size_t)num_loops);
  return CUSIFT_OK;
}

extern "C" int cusift_estimate_homography(cusift_ctx *ctx, cusift_point *d_sift, int num_pts, int num_pts2, int rule,
                                          float lo, float hi, int num_loops, float thresh, int refine_loops,
                                          float refine_thresh, uint64_t seed, float h_homography[9], float h_ransac[9],
                                          int *num_candidates, int *num_matches, int *num_fit, int *best_loop,
                                          char *h_inliers, int *h_drawn, float *h_all_homo, int *h_all_counts) {
  TRY(enter(ctx));
  const RansacOut o{h_homography, h_ransac, num_candidates, num_matches, num_fit,
                    best_loop,    h_inliers, h_drawn,       h_all_homo,  h_all_counts};
  TRY(precheck("EstimateHomography", d_sift, num_pts, rule, lo, hi, num_loops, thresh, refine_loops, refine_thresh, o));
  return ransac_run(ctx, kHomography, d_sift, num_pts, num_pts2, rule, lo, hi, num_loops, thresh, refine_loops,
                    refine_thresh, seed, o, nullptr);
}

extern "C" int cusift_register_planar(cusift_ctx *ctx, cusift_point *d_sift1, int num_pts1, const cusift_point *d_sift2,
                                      int num_pts2, int distance, int rule, float lo, float hi, int num_loops,
                                      float thresh, int refine_loops, float refine_thresh, uint64_t seed,
                                      float h_homography[9], float h_ransac[9], int *num_candidates, int *num_matches,
                                      int *num_fit, int *best_loop, char *h_inliers, int *h_drawn, float *h_all_homo,
                                      int *h_all_counts) {
  TRY(enter(ctx));
  const RansacOut o{h_homography, h_ransac, num_candidates, num_matches, num_fit,
                    best_loop,    h_inliers, h_drawn,       h_all_homo,  h_all_counts};
  TRY(precheck("RegisterPlanar", d_sift1, num_pts1, rule, lo, hi, num_loops, thresh, refine_loops, refine_thresh, o));
  const cusift_point *d_cross;
  TRY(match_enqueue(ctx, "RegisterPlanar", d_sift1, num_pts1, d_sift2, num_pts2, distance, &d_cross));
  return ransac_run(ctx, kHomography, d_sift1, num_pts1, num_pts2, rule, lo, hi, num_loops, thresh, refine_loops,
                    refine_thresh, seed, o, d_cross);
}

extern "C" int cusift_estimate_fundamental(cusift_ctx *ctx, cusift_point *d_sift, int num_pts, int num_pts2, int rule,
                                           float lo, float hi, int num_loops, float thresh, int refine_loops,
                                           float refine_thresh, uint64_t seed, double h_fundamental[9],
                                           double h_ransac[9], int *num_candidates, int *num_matches, int *num_fit,
                                           int *best_loop, char *h_inliers, int *h_drawn, double *h_all_f,
                                           int *h_all_counts) {
  TRY(enter(ctx));
  const RansacOut o{h_fundamental, h_ransac, num_candidates, num_matches, num_fit,
                    best_loop,     h_inliers, h_drawn,       h_all_f,     h_all_counts};
  TRY(precheck("EstimateFundamental", d_sift, num_pts, rule, lo, hi, num_loops, thresh, refine_loops, refine_thresh,
               o));
  return ransac_run(ctx, kFundamental, d_sift, num_pts, num_pts2, rule, lo, hi, num_loops, thresh, refine_loops,
                    refine_thresh, seed, o, nullptr);
}

extern "C" int cusift_register_epipolar(cusift_ctx *ctx, cusift_point *d_sift1, int num_pts1,
                                        const cusift_point *d_sift2, int num_pts2, int distance, int rule, float lo,
                                        float hi, int num_loops, float thresh, int refine_loops, float refine_thresh,
                                        uint64_t seed, double h_fundamental[9], double h_ransac[9], int *num_candidates,
                                        int *num_matches, int *num_fit, int *best_loop, char *h_inliers, int *h_drawn,
                                        double *h_all_f, int *h_all_counts) {
  TRY(enter(ctx));
  const RansacOut o{h_fundamental, h_ransac, num_candidates, num_matches, num_fit,
                    best_loop,     h_inliers, h_drawn,       h_all_f,     h_all_counts};
  TRY(precheck("RegisterEpipolar", d_sift1, num_pts1, rule, lo, hi, num_loops, thresh, refine_loops, refine_thresh, o));
  const cusift_point *d_cross;
  TRY(match_enqueue(ctx, "RegisterEpipolar", d_sift1, num_pts1, d_sift2, num_pts2, distance, &d_cross));
  return ransac_run(ctx, kFundamental, d_sift1, num_pts1, num_pts2, rule, lo, hi, num_loops, thresh, refine_loops,
                    refine_thresh, seed, o, d_cross);
}

// ------------------------------------------------------------------------------------------------
// absolute pose from coords3D and the matches' pixels (sift_pnp.hip): the third model of ransac_run -- six samples,
// twelve values, five coordinate rows, a camera, the answer [I | 0] -- one read-back
// ------------------------------------------------------------------------------------------------
// every refusal of cusift_estimate_pnp, before anything is enqueued or written
static int pnp_check(const char *who, const cusift_point *d_sift, int num_pts, int rule, float lo, float hi,
                     const cusift_camera *camera2, int num_loops, float thresh, int refine_loops, float refine_thresh,
                     const RansacOut &o) {
  if (!camera2) return fail(CUSIFT_ERR_INVALID, "%s: NULL camera", who);
  TRY(precheck(who, d_sift, num_pts, rule, lo, hi, num_loops, thresh, refine_loops, refine_thresh, o));
  return check_pinhole(camera2, who);
}
PnPCam pnp_cam(const cusift_camera *c) {
  return PnPCam{(double)c->fx, (double)c->fy, (double)c->cx - (double)c->origin, (double)c->cy - (double)c->origin};
}

extern "C" int cusift_estimate_pnp(cusift_ctx *ctx, cusift_point *d_sift, int num_pts, int num_pts2, int rule, float lo,
                                   float hi, const cusift_camera *camera2, int num_loops, float thresh, int refine_loops,
                                   float refine_thresh, uint64_t seed, double h_rt[12], double h_ransac[12],
                                   int *num_candidates, int *num_matches, int *num_fit, int *best_loop, char *h_inliers,
                                   int *h_drawn, double *h_all_rt, int *h_all_counts) {
  TRY(enter(ctx));
  const RansacOut o{h_rt, h_ransac, num_candidates, num_matches, num_fit, best_loop, h_inliers, h_drawn, h_all_rt, h_all_counts};
  TRY(pnp_check("EstimatePnP", d_sift, num_pts, rule, lo, hi, camera2, num_loops, thresh, refine_loops, refine_thresh, o));
  const PnPCam cam = pnp_cam(camera2);
  return ransac_run(ctx, kPnP, d_sift, num_pts, num_pts2, rule, lo, hi, num_loops, thresh, refine_loops, refine_thresh,
                    seed, o, nullptr, nullptr, &cam);
}

extern "C" int cusift_register_pnp(cusift_ctx *ctx, cusift_point *d_sift1, int num_pts1, const cusift_point *d_sift2,
                                   int num_pts2, int distance, int rule, float lo, float hi,
                                   const cusift_camera *camera2, int num_loops, float thresh, int refine_loops,
                                   float refine_thresh, uint64_t seed, double h_rt[12], double h_ransac[12],
                                   int *num_candidates, int *num_matches, int *num_fit, int *best_loop, char *h_inliers,
                                   int *h_drawn, double *h_all_rt, int *h_all_counts) {
  TRY(enter(ctx));
  const RansacOut o{h_rt, h_ransac, num_candidates, num_matches, num_fit, best_loop, h_inliers, h_drawn, h_all_rt, h_all_counts};
  TRY(pnp_check("RegisterPnP", d_sift1, num_pts1, rule, lo, hi, camera2, num_loops, thresh, refine_loops, refine_thresh, o));
  const cusift_point *d_cross;
  TRY(match_enqueue(ctx, "RegisterPnP", d_sift1, num_pts1, d_sift2, num_pts2, distance, &d_cross));
  const PnPCam cam = pnp_cam(camera2);
  return ransac_run(ctx, kPnP, d_sift1, num_pts1, num_pts2, rule, lo, hi, num_loops, thresh, refine_loops, refine_thresh,
                    seed, o, d_cross, nullptr, &cam);
}

// ------------------------------------------------------------------------------------------------
// the same over a batch of frames and a pair list (sift_sequence.hip)
// ------------------------------------------------------------------------------------------------
int check_pair_list(const int *h_pairs, int n_pairs, int n_images, int max_pts, const char *who) {
  if (n_pairs < 0 || n_pairs > 65535) return fail(CUSIFT_ERR_INVALID, "%s: n_pairs %d outside [0, 65535]", who, n_pairs);
  if (n_images < 0 || n_images > 65535)
    return fail(CUSIFT_ERR_INVALID, "%s: n_images %d outside [0, 65535]", who, n_images);
  if (max_pts < 0 || max_pts > (1 << 20)) return fail(CUSIFT_ERR_INVALID, "%s: max_pts %d outside [0, 2^20]", who, max_pts);
  if (n_pairs > 0 && !h_pairs) return fail(CUSIFT_ERR_INVALID, "%s: NULL pair list", who);
  for (int p = 0; p < 2 * n_pairs; ++p)
    if (h_pairs[p] < 0 || h_pairs[p] >= n_images)
      return fail(CUSIFT_ERR_INVALID, "%s: pair %d names frame %d outside [0, %d)", who, p / 2, h_pairs[p], n_images);
  return CUSIFT_OK;
}

// Uploads the pair list and enqueues the matcher of every pair: one launch, plus the merge when the columns are split.
// *d_pairs_out: the list on the device, for the stages behind it.  n_pairs >= 1, max_pts >= 1, the list is checked.
static int match_batch_launch32(cusift_ctx *ctx, const cusift_point *d_points, const unsigned int *d_counters,
                                int max_pts, const int *h_pairs, int n_pairs, int distance, cusift_match_row *d_rows,
                                const int **d_pairs_out, cusift_match_row *d_rows_back = nullptr,
                                const GuideCall *guide = nullptr) {
  const int row_blocks = idiv_up(max_pts, 64);
  int splits, cols_per_split;
  TRY(matcher_split_plan(ctx, kMatcher32, max_pts, max_pts, n_pairs, &splits, &cols_per_split));
  const int n1_pad = row_blocks * 64;
  const size_t list_b = align_up_sz(sizeof(int) * 2 * (size_t)n_pairs, 256);
  const size_t part_b = align_up_sz(splits > 1 ? sizeof(MatchPartial) * (size_t)n_pairs * splits * n1_pad : 0, 256);
  // the column side (cusift_match_batch_mutual): [pair][row block][max_pts] partials when there is more than one row block
  const size_t col_b = d_rows_back && row_blocks > 1 ? sizeof(MatchPartial) * (size_t)n_pairs * row_blocks * max_pts : 0;
  // the models of a guided call (cusift_match_batch_guided, never with d_rows_back): [pair], behind the partials
  // (cusift_match_batch_projected: ProjectModel [pair] in the same place; col_b is 0 for both, so it is 256-byte aligned)
  const size_t model_b = guide ? (guide->camera ? sizeof(ProjectModel) : sizeof(GuideModel)) * (size_t)n_pairs : 0;
  TRY(grow_scratch(ctx, ctx->pairs_scratch, ctx->pairs_scratch_bytes, list_b + part_b + col_b + model_b, "", false));
  int *d_pairs = (int *)ctx->pairs_scratch;
  MatchPartial *partials = splits > 1 ? (MatchPartial *)(ctx->pairs_scratch + list_b) : nullptr;
  MatchPartial *col_partials = col_b ? (MatchPartial *)(ctx->pairs_scratch + list_b + part_b) : nullptr;
  HIP_TRY(hipMemcpyAsync(d_pairs, h_pairs, sizeof(int) * 2 * (size_t)n_pairs, hipMemcpyHostToDevice, ctx->stream));
  const dim3 grid(row_blocks, splits, n_pairs);
  if (d_rows_back)
    hipLaunchKernelGGL(distance ? match_batch_mutual_kernel<true> : match_batch_mutual_kernel<false>, grid, dim3(256),
                       0, ctx->stream, d_points, d_counters, max_pts, d_pairs, cols_per_split, partials, n1_pad, d_rows,
                       col_partials, d_rows_back);
  else if (guide && guide->camera) {
    ProjectModel *d_models = (ProjectModel *)(ctx->pairs_scratch + list_b + part_b + col_b);
    ctx->project_models.resize(n_pairs);  // stays allocated behind this call, whenever the upload reads it
    for (int p = 0; p < n_pairs; ++p) ctx->project_models[p] = project_model(guide->h_models + 12 * (size_t)p, *guide->camera);
    HIP_TRY(hipMemcpyAsync(d_models, ctx->project_models.data(), model_b, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(distance ? match_batch_projected_kernel<true> : match_batch_projected_kernel<false>, grid,
                       dim3(256), 0, ctx->stream, d_points, d_counters, max_pts, (const int *)d_pairs, cols_per_split,
                       partials, n1_pad, d_rows, (const ProjectModel *)d_models, guide->r2);
  } else if (guide) {
    GuideModel *d_models = (GuideModel *)(ctx->pairs_scratch + list_b + part_b + col_b);
    HIP_TRY(hipMemcpyAsync(d_models, guide->h_models, model_b, hipMemcpyHostToDevice, ctx->stream));
    const auto kernel =
        guide->model == CUSIFT_GUIDE_EPIPOLAR
            ? (distance ? match_batch_guided_kernel<true, GuideF> : match_batch_guided_kernel<false, GuideF>)
            : (distance ? match_batch_guided_kernel<true, GuideH> : match_batch_guided_kernel<false, GuideH>);
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, ctx->stream, d_points, d_counters, max_pts, (const int *)d_pairs,
                       cols_per_split, partials, n1_pad, d_rows, (const GuideModel *)d_models, guide->r2);
  } else
    hipLaunchKernelGGL(distance ? match_batch_kernel<true> : match_batch_kernel<false>, grid, dim3(256), 0, ctx->stream,
                       d_points, d_counters, max_pts, d_pairs, cols_per_split, partials, n1_pad, d_rows);
  if (splits > 1)
    hipLaunchKernelGGL(match_batch_merge_kernel, dim3(idiv_up(max_pts, 256), n_pairs), dim3(256), 0, ctx->stream,
                       d_counters, max_pts, d_pairs, distance, cols_per_split, partials, n1_pad, splits, d_rows);
  if (col_partials)
    hipLaunchKernelGGL(match_batch_mutual_merge_kernel, dim3(idiv_up(max_pts, 256), n_pairs), dim3(256), 0, ctx->stream,
                       d_counters, max_pts, d_pairs, distance, (const MatchPartial *)col_partials, row_blocks,
                       d_rows_back);
  *d_pairs_out = d_pairs;
  return check_launch("match_batch");
}

// The matcher of the pair-list registrations: match_batch_launch32, or -- cusift_ctx_set_match_bits 8 -- ONE quantiser
// launch over the frames the list names (0 .. the highest), honouring the counters, then the batched 8-bit matcher: the
// same rows.
static int match_batch_launch(cusift_ctx *ctx, const cusift_point *d_points, const unsigned int *d_counters, int max_pts,
                              const int *h_pairs, int n_pairs, int distance, cusift_match_row *d_rows,
                              const int **d_pairs_out, cusift_match_row *d_rows_back) {
  if (ctx->match_bits != 8)
    return match_batch_launch32(ctx, d_points, d_counters, max_pts, h_pairs, n_pairs, distance, d_rows, d_pairs_out,
                              d_rows_back);
  int n_frames = 0;
  for (int p = 0; p < 2 * n_pairs; ++p) n_frames = std::max(n_frames, h_pairs[p] + 1);
  return match8_batch_enqueue(ctx, d_points, d_counters, n_frames, max_pts, h_pairs, n_pairs, distance, d_rows,
                              d_rows_back, d_pairs_out);
}

extern "C" int cusift_match_batch(cusift_ctx *ctx, const cusift_point *d_points, const unsigned int *d_counters,
                                  int n_images, int max_pts, const int *h_pairs, int n_pairs, int distance,
                                  cusift_match_row *d_rows) {
  TRY(enter(ctx));
  TRY(check_distance("MatchBatch", distance));
  TRY(check_pair_list(h_pairs, n_pairs, n_images, max_pts, "MatchBatch"));
  if (n_pairs == 0 || max_pts == 0) return CUSIFT_OK;
  if (!d_points || !d_rows) return fail(CUSIFT_ERR_INVALID, "MatchBatch: missing data");
  const int *d_pairs = nullptr;
  return match_batch_launch32(ctx, d_points, d_counters, max_pts, h_pairs, n_pairs, distance, d_rows, &d_pairs);
}

// cusift_match_batch under one model per pair (sift_match.hip: match_batch_guided_kernel)
extern "C" int cusift_match_batch_guided(cusift_ctx *ctx, const cusift_point *d_points, const unsigned int *d_counters,
                                         int n_images, int max_pts, const int *h_pairs, int n_pairs, int distance,
                                         int model, const double *h_models, float radius, cusift_match_row *d_rows) {
  TRY(enter(ctx));
  TRY(check_distance("MatchBatchGuided", distance));
  TRY(check_pair_list(h_pairs, n_pairs, n_images, max_pts, "MatchBatchGuided"));
  TRY(check_guide("MatchBatchGuided", model, h_models, radius));
  if (n_pairs == 0 || max_pts == 0) return CUSIFT_OK;
  if (!d_points || !d_rows) return fail(CUSIFT_ERR_INVALID, "MatchBatchGuided: missing data");
  const GuideCall guide{model, radius * radius, h_models};
  const int *d_pairs = nullptr;
  return match_batch_launch32(ctx, d_points, d_counters, max_pts, h_pairs, n_pairs, distance, d_rows, &d_pairs, nullptr,
                            &guide);
}

// Matching by projection (sift_match_project.hip): cusift_match / cusift_match_batch where a record of image 2 counts for
// a row only within `radius` pixels of where the pose puts the row's coords3D.  Every refusal the two calls add:
int check_project(const char *who, const double *h_rts, const cusift_camera *camera2, float radius) {
  if (!h_rts) return fail(CUSIFT_ERR_INVALID, "%s: NULL pose", who);
  if (!camera2) return fail(CUSIFT_ERR_INVALID, "%s: NULL camera", who);
  TRY(check_pinhole(camera2, who));
  return radius > 0.0f ? CUSIFT_OK : fail(CUSIFT_ERR_INVALID, "%s: radius must be > 0", who);
}

extern "C" int cusift_match_projected(cusift_ctx *ctx, cusift_point *d_sift1, int num_pts1, const cusift_point *d_sift2,
                                      int num_pts2, int distance, const double h_rt[12], const cusift_camera *camera2,
                                      float radius) {
  TRY(enter(ctx));
  if (num_pts1 <= 0 || num_pts2 <= 0) return CUSIFT_OK;  // as cusift_match: nothing to match
  if (!d_sift1 || !d_sift2) return fail(CUSIFT_ERR_INVALID, "MatchProjected: missing data");
  TRY(check_distance("MatchProjected", distance));
  TRY(check_project("MatchProjected", h_rt, camera2, radius));
  const PnPCam cam = pnp_cam(camera2);
  const GuideCall guide{0, radius * radius, h_rt, &cam};
  return match_launch(ctx, d_sift1, num_pts1, d_sift2, num_pts2, distance, nullptr, &guide);
}

extern "C" int cusift_match_batch_projected(cusift_ctx *ctx, const cusift_point *d_points, const unsigned int *d_counters,
                                            int n_images, int max_pts, const int *h_pairs, int n_pairs, int distance,
                                            const double *h_rts, const cusift_camera *camera2, float radius,
                                            cusift_match_row *d_rows) {
  TRY(enter(ctx));
  TRY(check_distance("MatchBatchProjected", distance));
  TRY(check_pair_list(h_pairs, n_pairs, n_images, max_pts, "MatchBatchProjected"));
  TRY(check_project("MatchBatchProjected", h_rts, camera2, radius));
  if (n_pairs == 0 || max_pts == 0) return CUSIFT_OK;
  if (!d_points || !d_rows) return fail(CUSIFT_ERR_INVALID, "MatchBatchProjected: missing data");
  const PnPCam cam = pnp_cam(camera2);
  const GuideCall guide{0, radius * radius, h_rts, &cam};
  const int *d_pairs = nullptr;
  return match_batch_launch32(ctx, d_points, d_counters, max_pts, h_pairs, n_pairs, distance, d_rows, &d_pairs, nullptr,
                            &guide);
}

// cusift_match_batch with the column side of every pair in d_rows_back (sift_match.hip: match_batch_mutual_kernel)
extern "C" int cusift_match_batch_mutual(cusift_ctx *ctx, const cusift_point *d_points, const unsigned int *d_counters,
                                         int n_images, int max_pts, const int *h_pairs, int n_pairs, int distance,
                                         cusift_match_row *d_rows, cusift_match_row *d_rows_back) {
  TRY(enter(ctx));
  TRY(check_distance("MatchBatchMutual", distance));
  TRY(check_pair_list(h_pairs, n_pairs, n_images, max_pts, "MatchBatchMutual"));
  if (!d_rows_back) return fail(CUSIFT_ERR_INVALID, "MatchBatchMutual: NULL d_rows_back");
  if (n_pairs == 0 || max_pts == 0) return CUSIFT_OK;
  if (!d_points || !d_rows) return fail(CUSIFT_ERR_INVALID, "MatchBatchMutual: missing data");
  const int *d_pairs = nullptr;
  return match_batch_launch32(ctx, d_points, d_counters, max_pts, h_pairs, n_pairs, distance, d_rows, &d_pairs,
                            d_rows_back);
}

extern "C" int cusift_register_rgbd_batch(cusift_ctx *ctx, cusift_point *d_points, const unsigned int *d_counters,
                                          int n_images, int max_pts, const uint16_t *d_depth, int width, int height,
                                          int pitch_elems, size_t image_stride_elems, const cusift_camera *camera,
                                          const int *h_pairs, int n_pairs, int distance, float score_thresh,
                                          float ambiguity_thresh, int num_loops, float thresh2, int rigid_type,
                                          uint64_t seed, float *h_rt, int *h_num_matches, int *h_num_inliers,
                                          int *h_sel_pairs, char *h_inliers) {
  TRY(enter(ctx));
  if (!h_rt || !h_num_matches || !h_num_inliers) return fail(CUSIFT_ERR_INVALID, "RegisterRGBDBatch: NULL output");
  TRY(check_camera(camera, "RegisterRGBDBatch"));
  TRY(check_dims("RegisterRGBDBatch", "rigid_type", rigid_type));
  TRY(check_distance("RegisterRGBDBatch", distance));
  TRY(check_num_loops("RegisterRGBDBatch", num_loops));
  TRY(check_thresh2("RegisterRGBDBatch", thresh2));
  TRY(check_not_nan("RegisterRGBDBatch", score_thresh, ambiguity_thresh));
  TRY(check_pair_list(h_pairs, n_pairs, n_images, max_pts, "RegisterRGBDBatch"));
  if (n_images > 0 && max_pts > 0 && (!d_points || !d_depth))
    return fail(CUSIFT_ERR_INVALID, "RegisterRGBDBatch: missing data");
  TRY(check_depth_geometry(width, height, pitch_elems, image_stride_elems, n_images, "RegisterRGBDBatch"));
  if (n_pairs == 0) return CUSIFT_OK;
  if (max_pts == 0) {  // every frame is empty: nothing to match (extras/matching.cu:241-242)
    for (int p = 0; p < n_pairs; ++p) {
      memcpy(h_rt + 12 * (size_t)p, kIdentRt, sizeof(kIdentRt));
      h_num_matches[p] = h_num_inliers[p] = 0;
    }
    return CUSIFT_OK;
  }
  // [heads | flags | selected pairs] is what travels back, in one copy; behind it what stays on the device
  const size_t P = (size_t)n_pairs, M = (size_t)max_pts, L = (size_t)num_loops;
  ScratchLayout s;
  s.take(kRigidHeadBytes * P);  // the heads, at 0
  const size_t flag_off = s.take(P * M);
  const size_t pair_off = s.take(sizeof(int) * 2 * P * M);
  const size_t row_off = s.take(sizeof(cusift_match_row) * P * M);
  const size_t coord_off = s.take(sizeof(float) * 6 * P * M);
  const size_t count_off = s.take(sizeof(int) * P);
  const size_t rt_off = s.take(sizeof(float) * 12 * P * L);
  const size_t cnt_off = s.take(sizeof(int) * P * L);
  const size_t idx_off = s.take(sizeof(int) * 3 * P * L);
  // cross-check (cusift_ctx_set_cross_check): the matcher's back rows, behind everything else
  const size_t back_off = ctx->cross_check ? s.take(sizeof(cusift_match_row) * P * M) : 0;
  TRY(grow_scratch(ctx, ctx->register_scratch, ctx->register_scratch_bytes, s.size, "", false));
  char *base = ctx->register_scratch;
  float *d_coord = at<float>(base, coord_off);
  int *d_count = at<int>(base, count_off);
  cusift_match_row *d_rows = at<cusift_match_row>(base, row_off);
  cusift_match_row *d_rows_back = ctx->cross_check ? at<cusift_match_row>(base, back_off) : nullptr;
  hipLaunchKernelGGL(rgbd_lift_kernel, dim3(idiv_up(max_pts, 256), n_images), dim3(256), 0, ctx->stream, d_points,
                     d_counters, max_pts, (const unsigned short *)d_depth, width, height, pitch_elems,
                     image_stride_elems, *camera);
  const int *d_pairs = nullptr;
  TRY(match_batch_launch(ctx, d_points, d_counters, max_pts, h_pairs, n_pairs, distance, d_rows, &d_pairs, d_rows_back));
  hipLaunchKernelGGL(sequence_select_kernel, dim3(n_pairs), dim3(256), 0, ctx->stream, d_points, d_counters, max_pts,
                     d_pairs, d_rows, score_thresh * score_thresh, ambiguity_thresh * ambiguity_thresh, 1,
                     at<int>(base, pair_off), d_coord, d_count, (const cusift_match_row *)d_rows_back);
  RigidBatch nb;
  nb.coord = 6 * M, nb.indices = 3 * L, nb.rt = 12 * L, nb.counts = L, nb.head = kRigidHeadWords, nb.flags = M, nb.count = 1;
  rigid_launch(ctx, d_coord, max_pts, d_count, at<int>(base, idx_off), num_loops, 1, thresh2, rigid_type, seed,
               at<float>(base, rt_off), at<int>(base, cnt_off), (float *)base, base + flag_off, n_pairs, nb);
  TRY(check_launch("register_rgbd_batch"));
  // the one blocking read-back
  std::vector<char> back(h_sel_pairs ? row_off : (h_inliers ? pair_off : kRigidHeadBytes * P));
  HIP_TRY(hipMemcpyAsync(back.data(), base, back.size(), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  for (size_t p = 0; p < P; ++p) {
    const char *head = back.data() + kRigidHeadBytes * p;
    const size_t n = (size_t)std::min(std::max(head_int(head, kRigidHeadCount), 0), max_pts);
    memcpy(h_rt + 12 * p, head, sizeof(float) * 12);
    h_num_inliers[p] = head_int(head, kRigidHeadInliers);
    h_num_matches[p] = (int)n;
    if (h_inliers) memcpy(h_inliers + p * M, back.data() + flag_off + p * M, n);
    if (h_sel_pairs) memcpy(h_sel_pairs + 2 * p * M, back.data() + pair_off + sizeof(int) * 2 * p * M, sizeof(int) * 2 * n);
  }
  return CUSIFT_OK;
}

// ------------------------------------------------------------------------------------------------
// the fused pose call: matcher, epipolar registration and the pose stage (sift_pose.hip) -- one read-back
// ------------------------------------------------------------------------------------------------
extern "C" int cusift_register_pose(cusift_ctx *ctx, cusift_point *d_sift1, int num_pts1, const cusift_point *d_sift2,
                                    int num_pts2, int distance, int rule, float lo, float hi, int num_loops, float thresh,
                                    int refine_loops, float refine_thresh, uint64_t seed, const cusift_camera *camera1,
                                    const cusift_camera *camera2, double h_fundamental[9], double h_ransac[9],
                                    int *num_candidates, int *num_matches, int *num_fit, int *best_loop, char *h_inliers,
                                    int *h_drawn, double *h_all_f, int *h_all_counts, double h_rt[12], int *num_front,
                                    int *h_votes, double *h_sigma) {
  TRY(enter(ctx));
  const RansacOut o{h_fundamental, h_ransac, num_candidates, num_matches, num_fit,
                    best_loop,     h_inliers, h_drawn,       h_all_f,     h_all_counts};
  const PoseOut po{h_rt, num_front, h_votes, h_sigma};
  TRY(pose_check("RegisterPose", camera1, camera2, po));
  TRY(precheck("RegisterPose", d_sift1, num_pts1, rule, lo, hi, num_loops, thresh, refine_loops, refine_thresh, o));
  const cusift_point *d_cross;
  TRY(match_enqueue(ctx, "RegisterPose", d_sift1, num_pts1, d_sift2, num_pts2, distance, &d_cross));
  PoseStage st = pose_stage(camera1, camera2, refine_thresh, po);
  return ransac_run(ctx, kFundamental, d_sift1, num_pts1, num_pts2, rule, lo, hi, num_loops, thresh, refine_loops,
                    refine_thresh, seed, o, d_cross, &st);
}

// ------------------------------------------------------------------------------------------------
// planar, epipolar, pose and PnP registration of a pair list (sift_sequence.hip, sift_planar.hip, sift_epipolar.hip,
// sift_pose.hip, sift_pnp.hip): the batch counterpart of ransac_run, told apart by the model -- one read-back
// ------------------------------------------------------------------------------------------------
// What a pair-list call returns besides RansacOut's arrays ([P] entries each), and what its model takes: the pose stage's
// outputs and cameras (pose_cams != NULL: cusift_register_pose_batch), the matches' camera (kPnP)
struct BatchExtra {
  float *h_match_error;
  const PoseCams *pose_cams;
  PoseOut pose;
  float *h_points3d;
  const PnPCam *cam;
};

// every refusal that the pair-list calls share, before anything is enqueued or written
static int batch_check(const char *who, const cusift_point *d_points, int n_images, int max_pts, const int *h_pairs,
                       int n_pairs, int distance, int rule, float lo, float hi, int num_loops, float thresh,
                       int refine_loops, float refine_thresh, const RansacOut &o) {
  TRY(check_pair_list(h_pairs, n_pairs, n_images, max_pts, who));
  TRY(precheck(who, d_points, n_images > 0 ? max_pts : 0, rule, lo, hi, num_loops, thresh, refine_loops, refine_thresh,
               o));
  return check_distance(who, distance);
}

// Pair p's slice of the outputs.
static RansacOut batch_pair_out(const RansacModel &m, const RansacOut &o, size_t p) {
  return RansacOut{(char *)o.h_model + m.elem * m.reported * p, (char *)o.h_ransac + m.elem * m.reported * p,
                   o.num_candidates + p, o.num_matches + p, o.num_fit + p, o.best_loop ? o.best_loop + p : nullptr,
                   nullptr, nullptr, nullptr, nullptr};
}

// The matcher, the marking, the model's four launches, the pose stage and the one read-back, every pair of the list in
// the same launches; the arguments are checked, n_pairs >= 1.
static int ransac_batch_run(cusift_ctx *ctx, const RansacModel &m, const cusift_point *d_points,
                            const unsigned int *d_counters, int max_pts, const int *h_pairs, int n_pairs, int distance,
                            int rule, float lo, float hi, int num_loops, float thresh, int refine_loops,
                            float refine_thresh, uint64_t seed, const RansacOut &o, const BatchExtra &x) {
  const size_t P = (size_t)n_pairs, M = (size_t)max_pts;
  const bool pose = x.pose_cams != nullptr;
  if (max_pts == 0) {  // every frame is empty, known from the arguments alone
    for (size_t p = 0; p < P; ++p) {
      ransac_nothing(m, 0, num_loops, batch_pair_out(m, o, p));
      if (pose) pose_nothing(x.pose, p);
    }
    return CUSIFT_OK;
  }
  // [heads | pose heads | flags | errors | points] is what travels back, in one copy; behind it what stays on the device:
  // one RansacBlock per pair, then the match rows and -- with the cross-check (cusift_ctx_set_cross_check) -- the
  // matcher's back rows
  const RansacBlock b(m, max_pts, num_loops);
  ScratchLayout s;
  s.take(m.head_bytes * P);  // the heads, at 0
  const size_t pose_off = pose ? s.take(kPoseHeadBytes * P) : s.size;
  const size_t flag_off = s.take(P * M);
  const size_t err_off = s.take(sizeof(float) * P * M);
  const size_t xyz_off = pose ? s.take(sizeof(float) * 3 * P * M) : s.size;
  const size_t block_off = s.take(b.bytes * P);
  const size_t row_off = s.take(sizeof(cusift_match_row) * P * M);
  const size_t back_off = ctx->cross_check ? s.take(sizeof(cusift_match_row) * P * M) : 0;
  TRY(grow_scratch(ctx, ctx->register_scratch, ctx->register_scratch_bytes, s.size, "", false));
  char *base = ctx->register_scratch, *d_block = base + block_off;
  cusift_match_row *d_rows = at<cusift_match_row>(base, row_off);
  cusift_match_row *d_rows_back = ctx->cross_check ? at<cusift_match_row>(base, back_off) : nullptr;
  PlanarBatch nb;
  nb.records = 0, nb.scratch = b.bytes, nb.head = m.head_bytes, nb.flags = M, nb.count = 1, nb.min_pts = m.min_pts;
  const int *d_pairs = nullptr;
  TRY(match_batch_launch(ctx, d_points, d_counters, max_pts, h_pairs, n_pairs, distance, d_rows, &d_pairs, d_rows_back));
  const dim3 mark_grid(idiv_up(max_pts, 256), 1, n_pairs);
  hipLaunchKernelGGL(m.launch == kPnPLaunch ? sequence_pnp_mark_kernel : sequence_mark_kernel, mark_grid, dim3(256), 0,
                     ctx->stream, d_points, d_counters, max_pts, d_pairs, (const cusift_match_row *)d_rows, rule,
                     mark_thresh(rule, lo), mark_thresh(rule, hi), at<float>(d_block, b.coord),
                     at<unsigned char>(d_block, b.marks), at<int>(d_block, b.blocks), (int *)base, nb,
                     (const cusift_match_row *)d_rows_back);
  if (m.launch == kPlanarLaunch)
    planar_launch(ctx, nullptr, max_pts, num_loops, thresh, refine_loops, refine_thresh, seed, d_block, b, (float *)base,
                  base + flag_off, at<float>(base, err_off), n_pairs, nb);
  else if (m.launch == kEpipolarLaunch)
    epipolar_launch(ctx, nullptr, max_pts, num_loops, thresh, refine_loops, refine_thresh, seed, d_block, b, (int *)base,
                    base + flag_off, at<float>(base, err_off), n_pairs, nb);
  else
    pnp_launch(ctx, nullptr, max_pts, num_loops, thresh, refine_loops, refine_thresh, seed, *x.cam, d_block, b,
               (int *)base, base + flag_off, at<float>(base, err_off), n_pairs, nb);
  if (pose)  // behind the selection, at refine_thresh as in the pair call; the points go to an array of their own
    TRY(pose_launch(ctx, nullptr, max_pts, at<float>(d_block, b.coord), at<unsigned char>(d_block, b.marks),
                    (const int *)base, *x.pose_cams, refine_thresh, at<int>(base, pose_off), at<float>(base, xyz_off),
                    n_pairs, nb));
  TRY(check_launch(m.label));
  // the one blocking read-back
  size_t back_bytes = pose ? pose_off + kPoseHeadBytes * P : m.head_bytes * P;
  if (o.h_inliers) back_bytes = flag_off + P * M;
  if (x.h_match_error) back_bytes = err_off + sizeof(float) * P * M;
  if (pose && x.h_points3d) back_bytes = xyz_off + sizeof(float) * 3 * P * M;
  std::vector<char> back(back_bytes);
  HIP_TRY(hipMemcpyAsync(back.data(), base, back.size(), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  for (size_t p = 0; p < P; ++p) {  // the kernels decided every pair: copies, and the model's answer where nothing was fitted
    const char *head = back.data() + m.head_bytes * p;
    const int n_cand = head_int(head, kPlanarHeadCand);
    const size_t n = (size_t)std::min(std::max(head_int(head, kPlanarHeadCount), 0), max_pts);  // records of frame a
    const RansacOut one = batch_pair_out(m, o, p);
    // a winner that counts no point (needs_support) is nothing to fit either, as ransac_run decides after its read-back
    const bool fitted = n_cand >= m.min_pts && !(m.needs_support && head_int(head, kPlanarHeadMatches) < 1);
    if (fitted) {
      memcpy(one.h_model, head + m.elem * m.head_model, m.elem * m.reported);
      memcpy(one.h_ransac, head + m.elem * m.head_ransac, m.elem * m.reported);
      *one.num_matches = head_int(head, kPlanarHeadMatches), *one.num_fit = head_int(head, kPlanarHeadFit);
      if (one.best_loop) *one.best_loop = head_int(head, kPlanarHeadLoop);
    } else {
      ransac_nothing(m, 0, num_loops, one);
    }
    *one.num_candidates = n_cand;
    if (o.h_inliers) memcpy(o.h_inliers + p * M, back.data() + flag_off + p * M, n);
    // a pair without a fit has no error, as the pair call leaves match_error alone then
    if (x.h_match_error && fitted)
      memcpy(x.h_match_error + p * M, back.data() + err_off + sizeof(float) * p * M, sizeof(float) * n);
    if (!pose) continue;
    pose_report(back.data() + pose_off + kPoseHeadBytes * p, x.pose, p);
    if (x.h_points3d)
      memcpy(x.h_points3d + 3 * p * M, back.data() + xyz_off + sizeof(float) * 3 * p * M, sizeof(float) * 3 * n);
  }
  return CUSIFT_OK;
}

extern "C" int cusift_register_planar_batch(cusift_ctx *ctx, const cusift_point *d_points, const unsigned int *d_counters,
                                            int n_images, int max_pts, const int *h_pairs, int n_pairs, int distance,
                                            int rule, float lo, float hi, int num_loops, float thresh, int refine_loops,
                                            float refine_thresh, uint64_t seed, float *h_homography, float *h_ransac,
                                            int *h_num_candidates, int *h_num_matches, int *h_num_fit, int *h_best_loop,
                                            char *h_inliers, float *h_match_error) {
  TRY(enter(ctx));
  const RansacOut o{h_homography, h_ransac, h_num_candidates, h_num_matches, h_num_fit, h_best_loop,
                    h_inliers,    nullptr,  nullptr,          nullptr};
  TRY(batch_check("RegisterPlanarBatch", d_points, n_images, max_pts, h_pairs, n_pairs, distance, rule, lo, hi, num_loops,
                  thresh, refine_loops, refine_thresh, o));
  if (n_pairs == 0) return CUSIFT_OK;
  const BatchExtra x{h_match_error, nullptr, PoseOut{}, nullptr, nullptr};
  return ransac_batch_run(ctx, kHomography, d_points, d_counters, max_pts, h_pairs, n_pairs, distance, rule, lo, hi,
                          num_loops, thresh, refine_loops, refine_thresh, seed, o, x);
}

extern "C" int cusift_register_epipolar_batch(cusift_ctx *ctx, const cusift_point *d_points,
                                              const unsigned int *d_counters, int n_images, int max_pts,
                                              const int *h_pairs, int n_pairs, int distance, int rule, float lo, float hi,
                                              int num_loops, float thresh, int refine_loops, float refine_thresh,
                                              uint64_t seed, double *h_fundamental, double *h_ransac,
                                              int *h_num_candidates, int *h_num_matches, int *h_num_fit, int *h_best_loop,
                                              char *h_inliers, float *h_match_error) {
  TRY(enter(ctx));
  const RansacOut o{h_fundamental, h_ransac, h_num_candidates, h_num_matches, h_num_fit, h_best_loop,
                    h_inliers,     nullptr,  nullptr,          nullptr};
  TRY(batch_check("RegisterEpipolarBatch", d_points, n_images, max_pts, h_pairs, n_pairs, distance, rule, lo, hi,
                  num_loops, thresh, refine_loops, refine_thresh, o));
  if (n_pairs == 0) return CUSIFT_OK;
  const BatchExtra x{h_match_error, nullptr, PoseOut{}, nullptr, nullptr};
  return ransac_batch_run(ctx, kFundamental, d_points, d_counters, max_pts, h_pairs, n_pairs, distance, rule, lo, hi,
                          num_loops, thresh, refine_loops, refine_thresh, seed, o, x);
}

extern "C" int cusift_register_pose_batch(cusift_ctx *ctx, const cusift_point *d_points, const unsigned int *d_counters,
                                          int n_images, int max_pts, const int *h_pairs, int n_pairs, int distance,
                                          int rule, float lo, float hi, int num_loops, float thresh, int refine_loops,
                                          float refine_thresh, uint64_t seed, const cusift_camera *camera1,
                                          const cusift_camera *camera2, double *h_fundamental, double *h_ransac,
                                          int *h_num_candidates, int *h_num_matches, int *h_num_fit, int *h_best_loop,
                                          char *h_inliers, float *h_match_error, double *h_rt, int *h_num_front,
                                          int *h_votes, double *h_sigma, float *h_points3d) {
  TRY(enter(ctx));
  const RansacOut o{h_fundamental, h_ransac, h_num_candidates, h_num_matches, h_num_fit, h_best_loop,
                    h_inliers,     nullptr,  nullptr,          nullptr};
  const PoseOut po{h_rt, h_num_front, h_votes, h_sigma};
  TRY(pose_check("RegisterPoseBatch", camera1, camera2, po));
  TRY(batch_check("RegisterPoseBatch", d_points, n_images, max_pts, h_pairs, n_pairs, distance, rule, lo, hi, num_loops,
                  thresh, refine_loops, refine_thresh, o));
  if (n_pairs == 0) return CUSIFT_OK;
  const PoseStage st = pose_stage(camera1, camera2, refine_thresh, po);
  const BatchExtra x{h_match_error, &st.cams, po, h_points3d, nullptr};
  return ransac_batch_run(ctx, kFundamental, d_points, d_counters, max_pts, h_pairs, n_pairs, distance, rule, lo, hi,
                          num_loops, thresh, refine_loops, refine_thresh, seed, o, x);
}

extern "C" int cusift_register_pnp_batch(cusift_ctx *ctx, const cusift_point *d_points, const unsigned int *d_counters,
                                         int n_images, int max_pts, const int *h_pairs, int n_pairs, int distance,
                                         int rule, float lo, float hi, const cusift_camera *camera2, int num_loops,
                                         float thresh, int refine_loops, float refine_thresh, uint64_t seed, double *h_rt,
                                         double *h_ransac, int *h_num_candidates, int *h_num_matches, int *h_num_fit,
                                         int *h_best_loop, char *h_inliers, float *h_match_error) {
  TRY(enter(ctx));
  const RansacOut o{h_rt, h_ransac, h_num_candidates, h_num_matches, h_num_fit, h_best_loop, h_inliers, nullptr, nullptr,
                    nullptr};
  if (!camera2) return fail(CUSIFT_ERR_INVALID, "RegisterPnPBatch: NULL camera");
  TRY(batch_check("RegisterPnPBatch", d_points, n_images, max_pts, h_pairs, n_pairs, distance, rule, lo, hi, num_loops,
                  thresh, refine_loops, refine_thresh, o));
  TRY(check_pinhole(camera2, "RegisterPnPBatch"));
  if (n_pairs == 0) return CUSIFT_OK;
  const PnPCam cam = pnp_cam(camera2);
  const BatchExtra x{h_match_error, nullptr, PoseOut{}, nullptr, &cam};
  return ransac_batch_run(ctx, kPnP, d_points, d_counters, max_pts, h_pairs, n_pairs, distance, rule, lo, hi, num_loops,
                          thresh, refine_loops, refine_thresh, seed, o, x);
}
