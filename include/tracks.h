// tracks.h -- feature tracks of a sequence and their triangulation, over cusift_build_tracks and
// cusift_triangulate_tracks (cusift_amd_extras.h).  New: the reference returns matches per pair.  Plain C++ over the C
// ABI, like sequence.h: no HIP headers.
//
// BuildTracks matches every pair of a list (cusift_match_batch_mutual, or cusift_match_batch with mutual = false), joins
// the accepted rows into connected components on the device and returns the components that are tracks -- at least
// minViews records, no two of one frame -- as lists of (frame, record), frames ascending, the tracks in ascending order
// of their first observation.  Only the track count, the offsets and the observations travel back.
// TriangulateTracks gives every track its 3-D point from all its views under per-frame poses [R | t] (camera to world,
// 12 doubles a frame) and one camera.
// BundleAdjust refines those poses and points together (cusift_bundle_adjust: Schur-complement Levenberg-Marquardt on
// the device) and returns them in place.
#ifndef CUSIFT_AMD_TRACKS_H
#define CUSIFT_AMD_TRACKS_H

#include <cstddef>
#include <utility>
#include <vector>

#include "cuSIFT.h"
#include "cusift_amd_extras.h"
#include "sequence.h"

typedef std::vector<std::vector<std::pair<int, int> > > SiftTracks;  // [track][view] = (frame, record)

// pairs: (frame a, frame b) rows, an empty list means (i, i + 1) for every consecutive frame.  rule / maxScore /
// maxAmbiguity: the match filter of the registrations (rule 1: score < maxScore^2 && ambiguity < maxAmbiguity^2, for
// the L2 distance; rule 0: score > maxScore && ambiguity < maxAmbiguity).  inliers (optional): [pair][record of frame a]
// flags such as RegisterPlanarSequence's -- only flagged rows can join records; a pair's list may be shorter than the
// frame.  stats (optional): the eight counters of cusift_build_tracks.  The frames are not written.  Returns the
// elapsed milliseconds.
inline double BuildTracks(std::vector<SiftData *> &frames, std::vector<std::pair<int, int> > pairs, SiftTracks &tracks,
                          int minViews = 2, bool mutual = true, float maxScore = 999.0f, float maxAmbiguity = 0.8f,
                          int distance = 1, int rule = 1, const std::vector<std::vector<char> > *inliers = NULL,
                          std::vector<unsigned int> *stats = NULL) {
  TimerGPU timer;
  cusift_ctx *c = cusift_dropin::ctx();
  cusift_dropin::SequencePack pack(frames, pairs);
  const size_t nodes = (size_t)pack.n * pack.max_pts, flat = pack.flat();
  cusift_dropin::device_block rows(sizeof(cusift_match_row) * flat), back(mutual ? sizeof(cusift_match_row) * flat : 0);
  cusift_dropin::device_block keep(inliers ? flat : 0), track(sizeof(int) * nodes), offsets(sizeof(int) * (nodes / 2 + 1));
  cusift_dropin::device_block obs(sizeof(int) * nodes), counters(sizeof(unsigned int) * 8);
  cusift_match_row *d_rows = static_cast<cusift_match_row *>(rows.ptr);
  cusift_match_row *d_back = mutual ? static_cast<cusift_match_row *>(back.ptr) : NULL;
  if (inliers) {
    std::vector<unsigned char> flags(flat > 0 ? flat : 1, 0);
    for (size_t k = 0; k < (size_t)pack.n_pairs && k < inliers->size(); k++)
      for (size_t i = 0; i < (*inliers)[k].size() && i < (size_t)pack.max_pts; i++)
        flags[k * pack.max_pts + i] = (*inliers)[k][i] != 0;
    safeCall(cusift_memcpy_h2d(c, keep.ptr, flags.data(), flat));
  }
  if (mutual)
    safeCall(cusift_match_batch_mutual(c, pack.d_points(), pack.d_counters(), pack.n, pack.max_pts, pack.h_pairs.data(),
                                       pack.n_pairs, distance, d_rows, d_back));
  else
    safeCall(cusift_match_batch(c, pack.d_points(), pack.d_counters(), pack.n, pack.max_pts, pack.h_pairs.data(),
                                pack.n_pairs, distance, d_rows));
  safeCall(cusift_build_tracks(c, pack.d_counters(), pack.n, pack.max_pts, pack.h_pairs.data(), pack.n_pairs, d_rows,
                               d_back, inliers ? static_cast<const unsigned char *>(keep.ptr) : NULL, rule, maxScore,
                               maxAmbiguity, minViews, static_cast<int *>(track.ptr), static_cast<int *>(offsets.ptr),
                               static_cast<int *>(obs.ptr), static_cast<unsigned int *>(counters.ptr)));
  unsigned int h_stats[8];
  safeCall(cusift_memcpy_d2h(c, h_stats, counters.ptr, sizeof(h_stats)));
  std::vector<int> h_offsets((size_t)h_stats[0] + 1), h_obs(h_stats[1] > 0 ? h_stats[1] : 1);
  safeCall(cusift_memcpy_d2h(c, h_offsets.data(), offsets.ptr, sizeof(int) * h_offsets.size()));
  if (h_stats[1] > 0) safeCall(cusift_memcpy_d2h(c, h_obs.data(), obs.ptr, sizeof(int) * (size_t)h_stats[1]));
  tracks.assign(h_stats[0], std::vector<std::pair<int, int> >());
  for (size_t t = 0; t < tracks.size(); t++)
    for (int e = h_offsets[t]; e < h_offsets[t + 1]; e++)
      tracks[t].push_back(std::make_pair(h_obs[e] / pack.max_pts, h_obs[e] % pack.max_pts));
  if (stats) stats->assign(h_stats, h_stats + 8);
  return timer.read();
}

// The 3-D point of every track from all its views: 4 doubles a track, (X, Y, Z, largest reprojection error in pixels),
// in the coordinates of `poses` -- 12 doubles a frame, row-major [R | t], camera to world.  A degenerate track (a pivot
// of its 3 x 3 system not above minPivot: identical or nearly parallel rays, a coordinate that is not finite) has four
// zeros.  front (optional): the views of each track that have the point in front of them.
inline std::vector<double> TriangulateTracks(std::vector<SiftData *> &frames, const SiftTracks &tracks,
                                             const std::vector<double> &poses, const cusift_camera &camera,
                                             double minPivot = 1e-12, std::vector<int> *front = NULL) {
  cusift_ctx *c = cusift_dropin::ctx();
  std::vector<std::pair<int, int> > none;
  cusift_dropin::SequencePack pack(frames, none);
  const size_t n_tracks = tracks.size();
  if (poses.size() < 12 * frames.size()) return std::vector<double>();  // 12 doubles a frame
  std::vector<int> h_offsets(1, 0), h_obs;
  for (size_t t = 0; t < n_tracks; t++) {
    for (size_t e = 0; e < tracks[t].size(); e++) h_obs.push_back(tracks[t][e].first * pack.max_pts + tracks[t][e].second);
    h_offsets.push_back((int)h_obs.size());
  }
  unsigned int h_stats[8] = {(unsigned int)n_tracks, (unsigned int)h_obs.size(), 0, 0, 0, 0, 0, 0};
  cusift_dropin::device_block offsets(sizeof(int) * h_offsets.size()), obs(sizeof(int) * h_obs.size());
  cusift_dropin::device_block counters(sizeof(h_stats)), points(sizeof(double) * 4 * n_tracks), in_front(sizeof(int) * n_tracks);
  safeCall(cusift_memcpy_h2d(c, offsets.ptr, h_offsets.data(), sizeof(int) * h_offsets.size()));
  if (!h_obs.empty()) safeCall(cusift_memcpy_h2d(c, obs.ptr, h_obs.data(), sizeof(int) * h_obs.size()));
  safeCall(cusift_memcpy_h2d(c, counters.ptr, h_stats, sizeof(h_stats)));
  safeCall(cusift_triangulate_tracks(c, pack.d_points(), pack.n, pack.max_pts, static_cast<const int *>(offsets.ptr),
                                     static_cast<const int *>(obs.ptr), static_cast<const unsigned int *>(counters.ptr),
                                     (int)n_tracks, poses.data(), &camera, minPivot, static_cast<double *>(points.ptr),
                                     static_cast<int *>(in_front.ptr)));
  std::vector<double> out(4 * n_tracks);
  if (n_tracks > 0) safeCall(cusift_memcpy_d2h(c, out.data(), points.ptr, sizeof(double) * out.size()));
  if (front) {
    front->assign(n_tracks, 0);
    if (n_tracks > 0) safeCall(cusift_memcpy_d2h(c, front->data(), in_front.ptr, sizeof(int) * n_tracks));
  }
  return out;
}

// Bundle adjustment of what TriangulateTracks returned: `poses` (12 doubles a frame) and `points` (4 doubles a track)
// go in and come back refined -- a track that is not used (four zeros, a coordinate that is not finite, fewer than two
// observations in front of their cameras and inside params->max_error) keeps its row, a frame that is held its pose.
// params: NULL for cusift_bundle_default_params.  fixed (optional): a flag per frame that must not move; NULL holds
// frame 0 only, which leaves the scale to the damping -- fix a second frame to pin it.  history (optional): 4 doubles
// per enqueued iteration (cost, trial cost, lambda, 1 accepted / 0 rejected / 2 not run).  Returns the 8 doubles of the
// summary: entry cost, final cost, accepted steps, iterations run, used tracks, used observations, free frames,
// final lambda; empty if poses or points are too short.
inline std::vector<double> BundleAdjust(std::vector<SiftData *> &frames, const SiftTracks &tracks,
                                        std::vector<double> &poses, const cusift_camera &camera,
                                        std::vector<double> &points, const cusift_bundle_params *params = NULL,
                                        const std::vector<char> *fixed = NULL, std::vector<double> *history = NULL) {
  cusift_ctx *c = cusift_dropin::ctx();
  std::vector<std::pair<int, int> > none;
  cusift_dropin::SequencePack pack(frames, none);
  const size_t n_tracks = tracks.size(), n_frames = frames.size();
  if (poses.size() < 12 * n_frames || points.size() < 4 * n_tracks) return std::vector<double>();
  if (fixed && fixed->size() < n_frames) return std::vector<double>();
  cusift_bundle_params par;
  if (params) par = *params;
  else cusift_bundle_default_params(&par);
  std::vector<int> h_offsets(1, 0), h_obs;
  for (size_t t = 0; t < n_tracks; t++) {
    for (size_t e = 0; e < tracks[t].size(); e++) h_obs.push_back(tracks[t][e].first * pack.max_pts + tracks[t][e].second);
    h_offsets.push_back((int)h_obs.size());
  }
  unsigned int h_stats[8] = {(unsigned int)n_tracks, (unsigned int)h_obs.size(), 0, 0, 0, 0, 0, 0};
  const size_t n_hist = 4 * (size_t)(par.iterations > 0 ? par.iterations : 1);
  cusift_dropin::device_block offsets(sizeof(int) * h_offsets.size()), obs(sizeof(int) * h_obs.size());
  cusift_dropin::device_block counters(sizeof(h_stats)), d_points(sizeof(double) * 4 * n_tracks);
  cusift_dropin::device_block d_poses(sizeof(double) * 12 * n_frames), d_history(sizeof(double) * n_hist);
  cusift_dropin::device_block d_summary(sizeof(double) * 8);
  safeCall(cusift_memcpy_h2d(c, offsets.ptr, h_offsets.data(), sizeof(int) * h_offsets.size()));
  if (!h_obs.empty()) safeCall(cusift_memcpy_h2d(c, obs.ptr, h_obs.data(), sizeof(int) * h_obs.size()));
  safeCall(cusift_memcpy_h2d(c, counters.ptr, h_stats, sizeof(h_stats)));
  if (n_tracks > 0) safeCall(cusift_memcpy_h2d(c, d_points.ptr, points.data(), sizeof(double) * 4 * n_tracks));
  std::vector<unsigned char> flags(n_frames > 0 ? n_frames : 1, 0);
  for (size_t f = 0; fixed && f < n_frames; f++) flags[f] = (*fixed)[f] != 0;
  safeCall(cusift_bundle_adjust(c, pack.d_points(), pack.n, pack.max_pts, static_cast<const int *>(offsets.ptr),
                                static_cast<const int *>(obs.ptr), static_cast<const unsigned int *>(counters.ptr),
                                (int)n_tracks, poses.data(), fixed ? flags.data() : NULL, &camera, &par,
                                static_cast<double *>(d_points.ptr), static_cast<double *>(d_poses.ptr),
                                static_cast<double *>(d_history.ptr), static_cast<double *>(d_summary.ptr)));
  std::vector<double> summary(8);
  safeCall(cusift_memcpy_d2h(c, summary.data(), d_summary.ptr, sizeof(double) * 8));
  if (n_frames > 0) safeCall(cusift_memcpy_d2h(c, poses.data(), d_poses.ptr, sizeof(double) * 12 * n_frames));
  if (n_tracks > 0) safeCall(cusift_memcpy_d2h(c, points.data(), d_points.ptr, sizeof(double) * 4 * n_tracks));
  if (history) {
    history->assign(n_hist, 0.0);
    safeCall(cusift_memcpy_d2h(c, history->data(), d_history.ptr, sizeof(double) * n_hist));
    history->resize(4 * (size_t)par.iterations);
  }
  return summary;
}

#endif  // CUSIFT_AMD_TRACKS_H
