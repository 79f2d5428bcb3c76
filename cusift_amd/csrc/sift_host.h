// sift_host.h -- what the host-side translation units of libcusift_amd.so share (not installed): the kernels' prototypes,
// the context object, the octave plan and the helpers of the launch wrappers.
//   sift_context.hip  errors, context + arena + policy + stage timers, memory helpers
//   sift_stages.hip   the C ABI's stage entry points and their launch wrappers (front-end, ScaleDown, LaplaceMulti,
//                     FindPointsMulti, fused detection, orientation, descriptors, bands, math-eval, packing)
//   sift_register.hip the registration host layer: matcher, FindHomography, rigid RANSAC, RGB-D registration, the
//                     calibrated pose, planar and epipolar registration on one chain, the absolute pose, the pair-list forms
//   sift_select.hip   keep the K strongest keypoints per image: its three kernels, cusift_select_strongest
//   sift_match8.hip   8-bit descriptors: the quantiser, the int8-MFMA matcher, their entry points (a unit of its own)
//   sift_match8_guided.hip  the int8 matcher's kernels under a geometric guide, on sift_match8_block.h with sift_match8.hip
//   sift_match_common.h  device code of both matchers (sift_match.hip, sift_match8.hip): write-out, pair-list frame,
//                     fold of the partials, the "partial or final" sink
//   sift_driver.hip   the octave driver: launch policy -> Plan (resolve_plan), cusift_extract_batch enqueues it; its
//                     recorded graph, the single-image entry points, cusift_ctx_reserve
//   sift_describe.hip cusift_describe_batch: the pyramid (describe_pyramid) and describe_given_kernel for caller-supplied
//                     keypoints
//   sift_second.hip   second-peak orientations: the scan kernel, the stage's launches, cusift_second_orientations_batch
//                     (its wave-per-record kernels: sift_second.inc, in sift_keypoints.hip's unit, on the frame that unit's
//                     description kernels share; all three are launched on describe_walk_grid, below)
//   sift_tracks.hip   cusift_build_tracks, cusift_triangulate_tracks: their kernels and entry points (a unit of its own)
//   sift_bundle.hip   cusift_bundle_adjust: its kernels and entry point (a unit of its own)
// The device units share sift_device.h (all of them) and sift_ransac.h (the eight registration units: sampling, winner,
// reductions, ordered compaction, pair strides).
#pragma once

#include <hip/hip_runtime.h>

#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "sift_internal.h"
#include "sift_types.h"


namespace cusift {
// kernels (sift_stencils.hip, sift_keypoints.hip)
__global__ void scale_down_kernel(float *, int, long, const float *, int, int, int, long, int, ScaleDownTaps);
__global__ void scale_down_fast_kernel(float *, int, long, const float *, int, int, int, long, int, ScaleDownTaps,
                                       RowWindow, int, int, int);
__global__ void scale_up_kernel(float *, int, long, const float *, int, int, int, long, int);
__global__ void scale_up_fast_kernel(float *, int, long, const float *, int, int, int, long, int);
__global__ void laplace_multi_kernel(const float *, float *, int, int, int, long, long, int, int, LaplaceTaps);
template <int kStoreAux>
__global__ void laplace_multi_fast_kernel(const float *, float *, int, int, int, long, long, int, LaplaceTapsPk);
__global__ void find_points_fast_kernel(const float *, int, int, int, long, cusift_point *, int, unsigned int *, int,
                                        FindParams);
template <bool kIdent0, int kRecBytes, bool kDown>
__global__ void detect_fused_kernel(const float *, int, int, int, long, cusift_point *, int, unsigned int *, int,
                                    LaplaceTapsPk, FindParams, RowWindow, int, int, DownOut);
template <int kRecBytes>
__global__ void detect_multi_kernel(DetectTable, int, unsigned int *);
__global__ void pyramid_small_kernel(PyramidLevels, ScaleDownTaps, unsigned int *, int);
__global__ void find_points_kernel(const float *, int, int, int, long, cusift_point *, int, unsigned int *, int, int,
                                   FindParams);
__global__ void orientations_kernel(const float *, int, int, int, long, cusift_point *, int, const unsigned int *,
                                    const unsigned int *, float, float, RowWindow);
__global__ void descriptors_kernel(const float *, int, int, int, long, cusift_point *, int, const unsigned int *,
                                   const unsigned int *, float, float, float, RowWindow, int, unsigned int *);
__global__ void describe_all_kernel(OctaveTable, cusift_point *, int, unsigned int *, int, float, float, int,
                                    unsigned int *, SegmentTable, const unsigned int *);
__global__ void join_counts_kernel(unsigned int *, SegmentTable, unsigned int *, int, int, unsigned int *, int);
__global__ void describe_bands_kernel(OctaveTable, BandWindows, cusift_point *, int, SegmentTable, const unsigned int *,
                                      float, float, int, unsigned int *);
__global__ void describe_given_kernel(OctaveTable, cusift_point *, int, const unsigned int *, int, float, float, int,
                                      unsigned int);
__global__ void second_peak_kernel(OctaveTable, const cusift_point *, int, const unsigned int *, int, float, float, float,
                                   unsigned int, float *);
__global__ void second_describe_kernel(OctaveTable, cusift_point *, int, const unsigned int *, const unsigned int *,
                                       const unsigned int *, const float *, int, float, float, int, unsigned int);
__global__ void rootsift_kernel(cusift_point *, int);
template <bool kL2>
__global__ void match_kernel(cusift_point *, int, const cusift_point *, int, int, MatchPartial *, int);
__global__ void match_merge_kernel(cusift_point *, int, const cusift_point *, int, int, const MatchPartial *, int, int);
template <bool kL2>
__global__ void match_batch_kernel(const cusift_point *, const unsigned int *, int, const int *, int, MatchPartial *, int,
                                   cusift_match_row *);
__global__ void match_batch_merge_kernel(const unsigned int *, int, const int *, int, int, const MatchPartial *, int, int,
                                         cusift_match_row *);
template <bool kL2>
__global__ void match_mutual_kernel(cusift_point *, int, cusift_point *, int, int, MatchPartial *, int, MatchPartial *);
__global__ void match_mutual_merge_kernel(cusift_point *, int, const cusift_point *, int, int, const MatchPartial *, int);
template <bool kL2>
__global__ void match_batch_mutual_kernel(const cusift_point *, const unsigned int *, int, const int *, int,
                                          MatchPartial *, int, cusift_match_row *, MatchPartial *, cusift_match_row *);
__global__ void match_batch_mutual_merge_kernel(const unsigned int *, int, const int *, int, const MatchPartial *, int,
                                                cusift_match_row *);
struct GuideH;  // the geometric predicates of the guided matchers (sift_match.hip)
struct GuideF;
template <bool kL2, class Guide>
__global__ void match_guided_kernel(cusift_point *, int, const cusift_point *, int, int, MatchPartial *, int, GuideModel,
                                    float);
template <bool kL2, class Guide>
__global__ void match_batch_guided_kernel(const cusift_point *, const unsigned int *, int, const int *, int,
                                          MatchPartial *, int, cusift_match_row *, const GuideModel *, float);
template <bool kL2>  // the matcher under a pose and coords3D (sift_match_project.hip)
__global__ void match_projected_kernel(cusift_point *, int, const cusift_point *, int, int, MatchPartial *, int,
                                       ProjectModel, float);
template <bool kL2>
__global__ void match_batch_projected_kernel(const cusift_point *, const unsigned int *, int, const int *, int,
                                             MatchPartial *, int, cusift_match_row *, const ProjectModel *, float);
struct Match8Partial;  // the int8 matcher's partial (sift_match8_block.h)
struct M8GuideH;        // the same predicates inside the int8 matcher (sift_match8_guided.hip)
struct M8GuideF;
struct M8GuideP;
template <bool kL2, class Guide, class Model>
__global__ void match8_guided_kernel(cusift_point *, int, const unsigned char *, const int *, const cusift_point *, int,
                                     const unsigned char *, const int *, int, Match8Partial *, int, Model, float);
template <bool kL2>
__global__ void match8_guided_merge_kernel(cusift_point *, int, const cusift_point *, int, const Match8Partial *, int, int);
template <bool kL2, class Guide, class Model>
__global__ void match8_batch_guided_kernel(const cusift_point *, const unsigned char *, const int *, const unsigned int *,
                                           int, const int *, int, Match8Partial *, int, cusift_match_row *, const Model *,
                                           float);
template <bool kL2>
__global__ void match8_batch_guided_merge_kernel(const unsigned int *, int, const int *, int, const Match8Partial *, int,
                                                 int, cusift_match_row *);
__global__ void sequence_select_kernel(const cusift_point *, const unsigned int *, int, const int *,
                                       const cusift_match_row *, float, float, int, int *, float *, int *,
                                       const cusift_match_row *);
__global__ void homography_gather_kernel(const cusift_point *, int, float *);
__global__ void homography_solve_kernel(const float *, int, int *, int, float *, int, unsigned long long, const int *,
                                        const int *, int *, PlanarBatch);
__global__ void planar_mark_kernel(const cusift_point *, int, int, int, float, float, float *, unsigned char *, int *,
                                   PlanarBatch, const cusift_point *);
__global__ void planar_compact_kernel(const unsigned char *, int, const int *, int *, int *, PlanarBatch);
__global__ void planar_score_kernel(const float *, int, int, const float *, int, float, int *, const int *, PlanarBatch);
__global__ void planar_select_kernel(cusift_point *, int, const float *, const unsigned char *, const float *, const int *,
                                     int, float, int, float, float *, char *, float *, PlanarBatch);
__global__ void epipolar_solve_kernel(const float *, int, const int *, const int *, unsigned long long, int, int *, double *,
                                      int *, float *, PlanarBatch);
__global__ void epipolar_score_kernel(const float *, int, int, const double *, int, float, int *, const int *, PlanarBatch);
__global__ void epipolar_select_kernel(cusift_point *, int, const float *, const float *, const unsigned char *,
                                       const double *, const int *, int, float, int, float, int *, char *, float *,
                                       PlanarBatch);
__global__ void pose_vote_kernel(const float *, const unsigned char *, int, const int *, PoseCams, float, int *,
                                 PlanarBatch);
__global__ void pose_write_kernel(cusift_point *, const float *, const unsigned char *, int, const int *, PoseCams, float,
                                  int *, float *, PlanarBatch);
__global__ void pnp_mark_kernel(const cusift_point *, int, int, int, float, float, float *, unsigned char *, int *,
                                const cusift_point *);
__global__ void pnp_solve_kernel(const float *, int, const int *, const int *, unsigned long long, int, PnPCam, int *,
                                 double *, int *, float *, PlanarBatch);
__global__ void pnp_score_kernel(const float *, int, int, const double *, int, PnPCam, float, int *, const int *,
                                 PlanarBatch);
__global__ void pnp_select_kernel(cusift_point *, int, const float *, const float *, const unsigned char *, const double *,
                                  const int *, int, PnPCam, float, int, float, int *, char *, float *, PlanarBatch);
__global__ void sequence_mark_kernel(const cusift_point *, const unsigned int *, int, const int *,
                                     const cusift_match_row *, int, float, float, float *, unsigned char *, int *, int *,
                                     PlanarBatch, const cusift_match_row *);
__global__ void sequence_pnp_mark_kernel(const cusift_point *, const unsigned int *, int, const int *,
                                         const cusift_match_row *, int, float, float, float *, unsigned char *, int *,
                                         int *, PlanarBatch, const cusift_match_row *);
__global__ void homography_test_kernel(const float *, int, const float *, int, float, int *);
template <bool k3D>
__global__ void rigid_solve_kernel(const float *, int, int *, int, int, unsigned long long, float *, int *, const int *,
                                   RigidBatch);
__global__ void rigid_score_kernel(const float *, int, int, const float *, int, float, int *, const int *, RigidBatch);
template <bool k3D>
__global__ void rigid_select_kernel(const float *, int, const float *, const int *, int, float, float *, char *,
                                    const int *, RigidBatch);
__global__ void rgbd_lift_kernel(cusift_point *, const unsigned int *, int, const unsigned short *, int, int, int, size_t,
                                 cusift_camera);
__global__ void match_select_count_kernel(const cusift_point *, int, const cusift_point *, int, float, float, int, int *);
__global__ void match_select_write_kernel(const cusift_point *, int, const cusift_point *, int, float, float, int,
                                          const int *, int *, float *, int *);
__global__ void u8_to_f32_kernel(float *, int, long, const unsigned char *, int, int, int, long, int);
__global__ void gaussian3x3_kernel(float *, int, long, const float *, int, int, int, long, float, float);
__global__ void math_eval_kernel(int, const float *, const float *, float *, float *, long);
__global__ void pack_points_kernel(const cusift_point *, const unsigned int *, int, int, cusift_point *, unsigned int,
                                   unsigned int *);
__global__ void pack_points_trimmed_kernel(const cusift_point *, const unsigned int *, int, int, cusift_trimmed_point *,
                                           unsigned int, unsigned int *);
__global__ void expand_trimmed_kernel(const cusift_trimmed_point *, size_t, cusift_point *);
__global__ void pack_points_compact_kernel(const cusift_point *, const unsigned int *, int, int, cusift_compact_point *,
                                           unsigned int, unsigned int *);
}  // namespace cusift

using namespace cusift;

// ------------------------------------------------------------------------------------------------
// errors
// ------------------------------------------------------------------------------------------------
// sets the thread's error text (cusift_last_error) and returns `code` (cusift_fail: sift_internal.h, printf-checked)
#define fail(...) cusift_fail(__VA_ARGS__)

#define HIP_TRY(expr)                                                                                        \
  do {                                                                                                       \
    hipError_t e_ = (expr);                                                                                  \
    if (e_ != hipSuccess)                                                                                    \
      return fail(CUSIFT_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
  } while (0)

#define TRY(expr)              \
  do {                         \
    int rc_ = (expr);          \
    if (rc_ != CUSIFT_OK) return rc_; \
  } while (0)

static inline int idiv_up(int a, int b) { return (a + b - 1) / b; }
static inline int ialign_up(int a, int b) { return idiv_up(a, b) * b; }  // cutils.h:17
static inline size_t align_up_sz(size_t a, size_t b) { return (a + b - 1) / b * b; }

// Lays the arrays of a scratch block out one behind the other, each on a 256-byte boundary: take() returns the offset of
// the next array, `size` is the offset behind the last one (the bytes the block needs).
struct ScratchLayout {
  size_t size = 0;
  size_t take(size_t bytes) {
    const size_t at = size;
    size += align_up_sz(bytes, 256);
    return at;
  }
};
template <class T>
static T *at(char *base, size_t offset) {  // the array at `offset` of a block
  return reinterpret_cast<T *>(base + offset);
}

// ------------------------------------------------------------------------------------------------
// context
// ------------------------------------------------------------------------------------------------
struct TimedSpan {
  hipEvent_t start, stop;
  int stage;
};

// Launch policy of a context, set per context through cusift_ctx_set_policy; a context starts with the defaults
// below.  Nothing here comes from the environment (CUSIFT_OCTAVE_OVERLAP, for an unchanged caller of the C++ shim, is
// read by the shim: include/cuSIFT.h), and nothing on a launch path looks at the environment.
// 0 / negative = "not set".
struct Knobs {
  int octave_overlap = 0;                            // CUSIFT_POLICY_SIDE_STREAM: 0 never (default), 1 eligible calls, 2 eligible calls
                                                     // after the concurrency probe, 3 every call (tests)
  int stage_all = -1;                                // CUSIFT_POLICY_OCTAVE_LISTS: -1 by size (default), 0 never, 1 whenever it fits
  bool force_generic = false;                        // CUSIFT_POLICY_GENERIC_KERNELS
  bool no_multi = false;                             // CUSIFT_POLICY_LAUNCH_PER_OCTAVE: the coarser octaves one launch each, even with lists
  int match_splits = 0;                              // CUSIFT_POLICY_MATCH_SPLITS
  bool tiled_per_octave = false;                     // CUSIFT_POLICY_TILED_PER_OCTAVE (read by cusift_tiled_create)
  int pyramid_in_detect = -1;                        // CUSIFT_POLICY_PYRAMID_IN_DETECT: -1 by size, 0 never, 1 octave 0, 2 every octave
};

struct cusift_ctx {
  int device = 0;
  Knobs knobs;
  int num_cus = 256;
  hipStream_t stream = nullptr;
  bool owns_stream = false;
  // scratch arena (one allocation, grown on demand, never shrunk)
  char *arena = nullptr;
  size_t arena_bytes = 0;
  // DoG planes of the two-stage path ([n][7][h0][p0] floats); allocated only when that path runs
  float *dog = nullptr;
  size_t dog_bytes = 0;
  // per-split partial results of the matcher (cusift_match)
  MatchPartial *match_scratch = nullptr;
  size_t match_scratch_bytes = 0;
  // per-row-block partial results of the column side (cusift_match_mutual): [row blocks][num_pts2]
  MatchPartial *match_col_scratch = nullptr;
  size_t match_col_scratch_bytes = 0;
  // the state of one registration call (sift_register.hip): FindHomography, rigid, RGB-D, pose, planar, epipolar, the
  // selection's block counts, the pair-list forms -- what travels back comes first.  Every call lays it out anew and
  // writes what it reads: nothing is carried from one call to the next.
  char *register_scratch = nullptr;
  size_t register_scratch_bytes = 0;
  // cusift_match_batch / cusift_register_rgbd_batch / cusift_register_planar_batch: the pair list and the matcher's
  // per-split partials (live together with register_scratch in the last two)
  char *pairs_scratch = nullptr;
  size_t pairs_scratch_bytes = 0;
  // cusift_match_batch_projected: the pairs' models as the upload reads them (the caller's poses beside the one camera)
  std::vector<ProjectModel> project_models;
  // the byte tables and sums the registrations quantise into while cusift_ctx_set_match_bits is 8 (sift_match8.hip)
  char *q8_scratch = nullptr;
  size_t q8_scratch_bytes = 0;
  // cusift_build_tracks (pair list, union-find, hash sets, scans) and cusift_triangulate_tracks (the poses): sift_tracks.hip
  char *tracks_scratch = nullptr;
  size_t tracks_scratch_bytes = 0;
  // cusift_bundle_adjust (the state, both pose and point buffers, node -> track, the reduced system): sift_bundle.hip
  char *bundle_scratch = nullptr;
  size_t bundle_scratch_bytes = 0;
  // staging buffer for 8-bit uploads (cusift_image_u8_h2d)
  unsigned char *u8_stage = nullptr;
  size_t u8_stage_bytes = 0;
  // small persistent device scratch for the blocking single-image entry points
  unsigned int *d_counter1 = nullptr;
  unsigned int *h_counter1 = nullptr;  // pinned mailbox the count of cusift_extract is copied to (no staged pageable copy)
  int extract_guess = 0;  // records cusift_extract copies back BEFORE it knows the count (the previous call's, + 1/8)
  unsigned int *d_queue = nullptr;  // kQueueShards work cursors of describe_all_kernel, 128 bytes apart
  int describe_grid = 0;  // resident blocks of describe_all_kernel on this device (occupancy query, cached)
  // octave 0's detection beside the coarser octaves (cusift_extract_batch): a second stream and its fork / join events
  hipStream_t side = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  bool side_failed = false;  // no stream was found that runs beside the context's stream: never fork
  bool side_probed = false;  // `side` passed the concurrency probe (policy value 2 accepts no other)
  bool recording = false;  // inside cusift_graph_create's capture
  int keep_strongest = 0;  // cusift_ctx_set_keep_strongest: K > 0, every extraction keeps the K strongest keypoints per image
  float second_orientation = 0.0f;  // cusift_ctx_set_second_orientation: ratio > 0, every extraction duplicates the keypoints
                                    // whose orientation histogram has a second peak above ratio x the first
  int cross_check = 0;     // cusift_ctx_set_cross_check: 1, the six cusift_register_* calls keep mutual matches only
  int match_bits = 32;     // cusift_ctx_set_match_bits: 8, the registrations quantise and match on the int8 matrix pipe
  unsigned long forks = 0;  // extractions that took the side stream
  // the lists' counters in the arena that the last extraction's join_counts_kernel left zero (stream order): the next
  // extraction that uses exactly them skips its memset.  Anything else that writes the arena resets this.
  const void *seg_clean_ptr = nullptr;
  size_t seg_clean_bytes = 0;
  unsigned long scratch_gen = 0;  // bumped whenever arena / DoG / matcher scratch is re-allocated (recorded graphs check it)
  // timing
  bool timing = false;
  std::vector<TimedSpan> spans;       // recorded, not yet folded
  std::vector<hipEvent_t> event_pool;  // free events
  float ms[CUSIFT_NUM_STAGES] = {0};
  int launches[CUSIFT_NUM_STAGES] = {0};
};


struct StageTimer {
  cusift_ctx *ctx;
  int stage;
  hipEvent_t start = nullptr, stop = nullptr;
  StageTimer(cusift_ctx *c, int s) : ctx(c), stage(s) {
    if (!ctx->timing) return;
    start = take();
    stop = take();
    if (start) (void)hipEventRecord(start, ctx->stream);
  }
  ~StageTimer() {
    if (!ctx->timing || !start || !stop) return;
    (void)hipEventRecord(stop, ctx->stream);
    ctx->spans.push_back({start, stop, stage});
  }
  hipEvent_t take() {
    if (!ctx->event_pool.empty()) {
      hipEvent_t e = ctx->event_pool.back();
      ctx->event_pool.pop_back();
      return e;
    }
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    return e;
  }
};

// How cusift_extract_batch detects one octave's keypoints.
enum Detect : unsigned char {
  kNotSearched,  // below cusift_params.lowest_scale (cuSIFT.cu:194)
  kTwoStage,     // LaplaceMulti + FindPointsMulti: the fused kernel does not apply (a 2x1 octave, a caller's odd pitch)
  kFused,        // the fused detection, appending in place to SiftData
  kStaged,       // the fused detection, heads to the octave's own list
  kSide,         // kStaged on the context's side stream (octave 0 of a forked call)
  kChain,        // kStaged, and it writes the next octave's image (the pyramid as a by-product of the detection)
  kOneLaunch,    // a member of the one multi-octave launch (heads to the octave's own list)
};
// Who zeroes the lists' counters: kByMemset is skipped when the previous extraction's join left these very counters zero.
enum SegClear : unsigned char { kNoLists, kByPyramid, kByMemset };

// One extraction, decided: the octave geometry (cuSIFT.cu:76-91,175-190), the arena layout and the launch sequence.  A pure
// function of the context's policy and flags (timing, recording, side_failed), cusift_params, the batch geometry and the
// alignment of the caller's images (resolve_plan, sift_driver.hip); cusift_extract_batch enqueues what it says.
struct Plan {
  int n_images = 0, n_oct = 0;
  // octave 0: the caller's images, or (cusift_params.upsample) their 2x enlargement in the arena at base_off[0]
  bool upsample = false;
  const float *img0 = nullptr;  // looked at for its alignment only (NULL: as aligned as the arena)
  size_t stride0 = 0;           // floats between the images of octave 0
  int w[kMaxOctaves], h[kMaxOctaves], p[kMaxOctaves];
  double blur[kMaxOctaves];
  float sub[kMaxOctaves];
  // arena offsets in bytes
  size_t base_off[kMaxOctaves];  // octave >= 1 base images (n * h*p floats each); [0]: the enlarged images
  size_t first_off = 0, total = 0;
  // staging lists of keypoint heads ([octave][image][max_pts] x kStagedRecBytes), see cusift_extract_batch:
  // staged_octaves == 0: none; 1: octave 0's (searched on the side stream); n_oct: every octave's
  size_t staged_off = 0, seg_end_off = 0;
  int staged_octaves = 0;
  // keep_strongest = K > 0: the selection's scratch (sift_select.hip) behind the lists; it runs after the last detection
  int keep = 0;
  size_t select_off = 0;
  // second_orientation = ratio > 0: the stage's scratch (sift_second.hip) behind that; it runs after describe_all_kernel
  float second = 0.0f;
  size_t second_off = 0;
  bool fork = false;     // the layout has octave 0's list for the side stream (stays set when no side stream is found)
  size_t dog_bytes = 0;  // DoG planes of the largest kTwoStage octave (0: none)
  // the launch sequence
  Detect detect[kMaxOctaves];
  bool flat = false;       // the keypoint stages run once, over all octaves (describe_all_kernel); else per octave
  bool stage_all = false;  // every searched octave to a list of its own, joined behind the detections
  bool forked = false;     // octave 0 on the side stream (wanted: cusift_extract_batch drops it if it finds no stream)
  int chain_end = 0;       // octaves [0, chain_end) are kChain: images 1 .. chain_end come from detections
  int small_levels = 0;    // levels 1 .. small_levels from ONE ScaleDown launch (pyramid_small_kernel); 0: none
  int concurrent = 1;      // what the detections are told about other batches in flight
  bool self_join = false;  // describe_all_kernel joins the lists itself (no join_counts_kernel)
  bool join_clears = false;  // join_counts_kernel leaves the lists' counters zero for the next extraction
  SegClear clear = kNoLists;
  size_t n_seg_counts = 0, seg_bytes = 0;  // the lists' counters: how many, and the bytes a memset clears
};

// Largest staging a context allocates: for octave 0 alone (the side stream), for all octaves (one detection launch; a
// batch beyond it keeps the in-place lists)
constexpr size_t kMaxStagedBytes = (size_t)1 << 30, kMaxStagedAllBytes = (size_t)1 << 30;

struct MultiOctave {
  const float *img;
  int w, h, pitch;
  size_t img_stride;
  float init_blur, subsampling;
  cusift_point *lists;
  unsigned int *counters;
  // a band of a larger image (cusift_extract_bands): global row of local row 0, global rows, centre rows; -1: whole image
  int row0 = 0, hg = -1, cy_begin = 0, cy_end = 0;
};

// Grows one of the context's device scratch blocks (never shrinks): waits for the stream, frees the old block, allocates.
// `recorded`: recorded graphs refer to the block, so its re-allocation invalidates them (scratch_gen).
template <class T>
static int grow_scratch(cusift_ctx *ctx, T *&ptr, size_t &have, size_t bytes, const char *what, bool recorded) {
  if (bytes <= have) return CUSIFT_OK;
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  if (recorded) ctx->scratch_gen++;
  if (ptr) HIP_TRY(hipFree(ptr));
  ptr = nullptr;
  have = 0;
  hipError_t e = hipMalloc((void **)&ptr, bytes);
  if (e != hipSuccess) return fail(CUSIFT_ERR_NOMEM, "%shipMalloc(%zu) failed: %s", what, bytes, hipGetErrorString(e));
  have = bytes;
  return CUSIFT_OK;
}

// shared between sift_context.hip, sift_stages.hip, sift_register.hip and sift_driver.hip
int enter(cusift_ctx *ctx);
int check_launch(const char *what);
int ensure_arena(cusift_ctx *ctx, size_t bytes);
// sift_register.hip: what every pair-list call refuses of its batch shape and its list (sift_tracks.hip shares it), and
// two refusals of the matchers (sift_match8.hip shares them): the distance, and record ranges that a mutual matcher
// writes both of
int check_pair_list(const int *h_pairs, int n_pairs, int n_images, int max_pts, const char *who);
int check_distance(const char *who, int distance);
int check_disjoint(const char *who, const cusift_point *d_sift1, int num_pts1, const cusift_point *d_sift2, int num_pts2);

// The shape of a brute-force matcher as its split plan sees it.
struct MatcherShape {
  int rows_per_block;  // rows of set 1 per workgroup
  int tile_cols;       // columns of set 2 per LDS tile
  int wgs_per_cu;      // workgroups per CU the grid aims at
  int col_bytes;       // bytes per column behind a split's buffer resource (32-bit byte offsets)
  const char *who;     // in the error text
};
constexpr MatcherShape kMatcher32{64, 32, 4, (int)sizeof(cusift_point), "MatchSiftData"};  // sift_match.hip
constexpr MatcherShape kMatcher8{256, 64, 2, 128, "Match8"};                                // sift_match8.hip
// the same under a guide: the columns' coords2D come through a buffer resource over the split's 588-byte records
constexpr MatcherShape kMatcher8Guided{256, 64, 2, (int)sizeof(cusift_point), "Match8Guided"};

// The column splits of a matcher over n_pairs pairs (a batch: sized from max_pts, the counts stay on the device): aim at
// >= wgs_per_cu workgroups per CU over all pairs, keep >= 4 LDS tiles per split.  CUSIFT_POLICY_MATCH_SPLITS = k > 0: k
// splits, at most one per tile.  A split is a whole number of tiles and spans less than 2^31 bytes (3.65 M of the
// 588-byte records) -- more columns than that force further splits (never a batch: max_pts <= 2^20).
static inline int matcher_split_plan(const cusift_ctx *ctx, const MatcherShape &shape, int num_pts1, int num_pts2,
                                     int n_pairs, int *splits_out, int *cols_per_split_out) {
  const int tile = shape.tile_cols;
  const long blocks = (long)idiv_up(num_pts1, shape.rows_per_block) * n_pairs;
  int splits = (int)std::max(1L, std::min(((long)shape.wgs_per_cu * ctx->num_cus + blocks - 1) / blocks,
                                          (long)idiv_up(num_pts2, 4 * tile)));
  if (ctx->knobs.match_splits > 0) splits = std::min(ctx->knobs.match_splits, idiv_up(num_pts2, tile));
  splits = std::min(splits, 65535);
  const int max_cols_per_split = (int)((0x7fffffffu / (unsigned int)shape.col_bytes) / tile * tile);
  splits = std::max(splits, idiv_up(num_pts2, max_cols_per_split));
  if (splits > 65535) return fail(CUSIFT_ERR_INVALID, "%s: too many records in set 2 (%d)", shape.who, num_pts2);
  const int cols_per_split = idiv_up(idiv_up(num_pts2, splits), tile) * tile;
  *splits_out = idiv_up(num_pts2, cols_per_split);
  *cols_per_split_out = cols_per_split;
  return CUSIFT_OK;
}
// The geometry of a guided match (cusift_match_guided, cusift_match_batch_guided and the 8-bit forms), checked: which test,
// the squared radius and the models as the caller's host array -- one of the pair call, one per pair of the pair-list call.
// camera != NULL (cusift_match_projected, cusift_match_batch_projected and the 8-bit forms): the test is the projection of
// coords3D, h_models holds [R | t], twelve doubles a pair, and `model` is not read.
struct GuideCall {
  int model;
  float r2;
  const double *h_models;
  const PnPCam *camera = nullptr;
};
// sift_register.hip: every refusal the guided and the projected calls add to their unguided counterparts', the camera as
// the kernels take it, and a pose beside it
int check_guide(const char *who, int model, const double *h_models, float radius);
int check_project(const char *who, const double *h_rts, const cusift_camera *camera2, float radius);
PnPCam pnp_cam(const cusift_camera *c);
ProjectModel project_model(const double *h_rt, const PnPCam &cam);
// sift_match8.hip, for the registrations' matcher fronts (sift_register.hip)
int match8_pair_enqueue(cusift_ctx *ctx, cusift_point *d_sift1, int num_pts1, const cusift_point *d_sift2, int num_pts2,
                        int distance, cusift_point *d_back, const GuideCall *guide = nullptr);
int match8_batch_enqueue(cusift_ctx *ctx, const cusift_point *d_points, const unsigned int *d_counters, int n_images,
                         int max_pts, const int *h_pairs, int n_pairs, int distance, cusift_match_row *d_rows,
                         cusift_match_row *d_rows_back, const int **d_pairs_out);
int ensure_side_stream(cusift_ctx *ctx);
size_t bands_arena_bytes(int n_bands, int max_pts);
void scale_down_taps(ScaleDownTaps &T, float variance);
void frac_consts(int frac_bits, float &q, float &inv_q);
bool detect_fused_ok(const float *d_img, int w, int h, int pitch, size_t img_stride);
int pyramid_small_impl(cusift_ctx *ctx, const float *const *base, const int *w, const int *h, const int *pitch,
                       const size_t *stride, int n_levels, int n_images, float variance, unsigned int *d_zero, int n_zero);
int detect_impl(cusift_ctx *ctx, const float *d_img, int w, int h, int pitch, size_t img_stride, float init_blur,
                float peak_thresh, float edge_thresh, float subsampling, cusift_point *d_points, int max_pts,
                unsigned int *d_counters, int n_images, RowWindow rw, int cy_begin, int cy_end, int concurrent = 1,
                bool heads = false, bool side = false, const DownOut *down = nullptr);
int detect_multi_impl(cusift_ctx *ctx, const MultiOctave *octaves, int n_octaves, float peak_thresh, float edge_thresh,
                      int max_pts, int n_images, int concurrent, unsigned int *d_queue);
size_t select_scratch_bytes(int n_lists, int n_images, int capacity);
int select_strongest_impl(cusift_ctx *ctx, const SegmentTable &G, int n_images, int capacity, int keep, char *scratch,
                          unsigned int *d_kept);
// sift_describe.hip: the pyramid of cusift_describe_batch, with `extra_bytes` of the arena behind it
int describe_pyramid(cusift_ctx *ctx, const char *who, const float *d_imgs, int n_images, int w, int h, int pitch,
                     size_t image_stride, const cusift_params *prm, const cusift_point *d_points, size_t extra_bytes,
                     OctaveTable &T, char **extra, bool &nothing);
// The grid of the kernels that walk records with RecordWalk (sift_keypoints.hip: describe_given_kernel, the second-peak
// kernels): as many workgroups as are resident at once (ctx->describe_grid, sized by describe_pyramid), at most one per
// record slot; up to kMaxFlatImages images are walked flat (grid.y == 1), beyond that one row of workgroups per image.
static inline dim3 describe_walk_grid(const cusift_ctx *ctx, int n_images, int max_pts) {
  const bool flat = n_images <= kMaxFlatImages;
  const long cap = flat ? (long)n_images * max_pts : (long)max_pts;
  const long resident = flat ? (long)ctx->describe_grid : std::max(1L, (long)ctx->describe_grid / n_images);
  return dim3((unsigned int)std::max(1L, std::min(cap, resident)), flat ? 1u : (unsigned int)n_images);
}
// sift_second.hip: the second-peak stage on records that were described on the pyramid T
size_t second_scratch_bytes(int n_images, int max_pts);
int second_orientations_impl(cusift_ctx *ctx, const OctaveTable &T, cusift_point *d_points, int max_pts,
                             unsigned int *d_counters, int n_images, const cusift_params *prm, float ratio,
                             unsigned int flags, char *scratch);
int descriptors_impl(cusift_ctx *ctx, const float *d_img, int w, int h, int pitch, size_t img_stride,
                     cusift_point *d_points, int max_pts, const unsigned int *d_first, const unsigned int *d_counters,
                     float subsampling, int tex_frac_bits, int n_images, RowWindow rw, int root_sift = 0,
                     unsigned int *d_flags = nullptr);
