// Bundle adjustment through the drop-in headers (include/tracks.h): BundleAdjust from plain C++ (g++), no HIP headers.
//
//   bundle_dropin scene.bin
//
// scene.bin, little-endian, written by tests/test_cpp_bundle.py: int32 n_frames, max_pts, n_tracks, n_obs, iterations;
// float32 fx, fy, cx, cy; float32 pixels [n_frames][max_pts][2]; int32 offsets [n_tracks + 1]; int32 obs [n_obs] (frame
// * max_pts + record); float64 poses [n_frames][12]; float64 points [n_tracks][4].  The program puts the pixels into
// SiftData frames, runs BundleAdjust and prints "summary <8 values>", "history <k> <4 values>" per iteration,
// "pose <f> <12 values>" per frame, "points <sum of |x| + |y| + |z|> <largest error>" and PASSED when the cost did not
// rise, frame 0 kept its pose and a second call from the result accepts next to nothing.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "cuSIFT.h"
#include "tracks.h"

template <class T>
static bool read_some(FILE *fp, std::vector<T> &v, size_t n) {
  v.resize(n);
  return n == 0 || std::fread(v.data(), sizeof(T), n, fp) == n;
}

int main(int argc, char **argv) {
  if (argc < 2) {
    std::printf("usage: %s scene.bin\n", argv[0]);
    return 2;
  }
  FILE *fp = std::fopen(argv[1], "rb");
  if (!fp) return 2;
  std::vector<int> head, offsets, obs;
  std::vector<float> cam, pixels;
  std::vector<double> poses, points;
  if (!read_some(fp, head, 5) || head[0] < 1 || head[1] < 1 || head[2] < 0 || head[3] < 0) return 2;
  const int n = head[0], max_pts = head[1], n_tracks = head[2], n_obs = head[3];
  if (!read_some(fp, cam, 4) || !read_some(fp, pixels, (size_t)n * max_pts * 2) ||
      !read_some(fp, offsets, (size_t)n_tracks + 1) || !read_some(fp, obs, (size_t)n_obs) ||
      !read_some(fp, poses, (size_t)n * 12) || !read_some(fp, points, (size_t)n_tracks * 4))
    return 2;
  std::fclose(fp);
  if (!deviceInit(0)) return 2;
  int failures = 0;
  {
    std::vector<SiftData *> frames;
    for (int f = 0; f < n; f++) {
      SiftData *d = new SiftData(max_pts, true, true);
      for (int i = 0; i < max_pts; i++) {
        d->h_data[i] = SiftPoint();
        d->h_data[i].coords2D[0] = pixels[2 * ((size_t)f * max_pts + i)];
        d->h_data[i].coords2D[1] = pixels[2 * ((size_t)f * max_pts + i) + 1];
      }
      d->numPts = max_pts;
      safeCall(cusift_memcpy_h2d(cusift_dropin::ctx(), d->d_data, d->h_data, sizeof(SiftPoint) * (size_t)max_pts));
      frames.push_back(d);
    }
    SiftTracks tracks((size_t)n_tracks);
    for (int t = 0; t < n_tracks; t++)
      for (int e = offsets[t]; e < offsets[t + 1]; e++) tracks[t].push_back(std::make_pair(obs[e] / max_pts, obs[e] % max_pts));
    const cusift_camera camera = {cam[0], cam[1], cam[2], cam[3], 0.0f, 1000.0f, 0};
    cusift_bundle_params par;
    cusift_bundle_default_params(&par);
    par.iterations = head[4];
    const std::vector<double> poses_in = poses;
    std::vector<double> history;
    const std::vector<double> summary = BundleAdjust(frames, tracks, poses, camera, points, &par, NULL, &history);
    if (summary.size() != 8 || history.size() != 4 * (size_t)par.iterations) return 1;
    std::printf("summary");
    for (int k = 0; k < 8; k++) std::printf(" %.17g", summary[k]);
    std::printf("\n");
    for (int k = 0; k < par.iterations; k++)
      std::printf("history %d %.17g %.17g %.17g %.17g\n", k, history[4 * k], history[4 * k + 1], history[4 * k + 2],
                  history[4 * k + 3]);
    for (int f = 0; f < n; f++) {
      std::printf("pose %d", f);
      for (int k = 0; k < 12; k++) std::printf(" %.17g", poses[12 * (size_t)f + k]);
      std::printf("\n");
    }
    double sum = 0.0, worst = 0.0;
    for (int t = 0; t < n_tracks; t++) {
      sum += std::fabs(points[4 * (size_t)t]) + std::fabs(points[4 * (size_t)t + 1]) + std::fabs(points[4 * (size_t)t + 2]);
      worst = points[4 * (size_t)t + 3] > worst ? points[4 * (size_t)t + 3] : worst;
    }
    std::printf("points %.17g %.17g\n", sum, worst);
    if (!(summary[1] <= summary[0]) || summary[2] < 1.0) failures++, std::printf("FAILED: the cost did not fall\n");
    for (int k = 0; k < 12; k++)
      if (poses[k] != poses_in[k]) failures++, std::printf("FAILED: frame 0 moved\n");
    // the result goes straight back in: its entry cost is the final cost; all frames fixed, the defaults otherwise
    std::vector<char> fixed((size_t)n, 1);
    std::vector<double> poses2 = poses, points2 = points;
    const std::vector<double> second = BundleAdjust(frames, tracks, poses2, camera, points2, NULL, &fixed);
    if (second.size() != 8 || std::fabs(second[0] - summary[1]) > 1e-9 * (summary[1] > 1.0 ? summary[1] : 1.0) ||
        second[6] != 0.0 || poses2 != poses)
      failures++, std::printf("FAILED: the second call\n");
    std::printf("second %.17g %.17g\n", second.size() == 8 ? second[0] : -1.0, second.size() == 8 ? second[1] : -1.0);
    for (size_t f = 0; f < frames.size(); f++) delete frames[f];
  }
  std::printf(failures ? "FAILED\n" : "PASSED\n");
  return failures ? 1 : 0;
}
