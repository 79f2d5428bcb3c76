// Feature tracks through the drop-in headers (include/tracks.h): BuildTracks and TriangulateTracks from plain C++ (g++),
// no HIP headers.  Four crops of the PGM fixture, each 16 x 8 pixels further along, are four views of a fronto-parallel
// plane at depth 5 from a camera that moves parallel to it: a track is one keypoint of the fixture in up to four crops,
// and its triangulated point lies at depth 5.
//
//   tracks_dropin tests/golden/gray1.pgm
//
// prints "tracks <T> observations <O> accepted <rows> shared <dropped components>", "views <tracks of 2> <of 3> <of 4>",
// "consistent <tracks whose views are one keypoint of the fixture>", "depth <tracks within 0.25 of depth 5>" and PASSED.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "cuImage.h"
#include "cuSIFT.h"
#include "tracks.h"

static bool read_pgm(const char *path, std::vector<float> &img, int &w, int &h) {
  FILE *fp = std::fopen(path, "rb");
  if (!fp) return false;
  int maxv = 0;
  if (std::fscanf(fp, "P5 %d %d %d", &w, &h, &maxv) != 3 || maxv != 255) return false;
  std::fgetc(fp);
  std::vector<unsigned char> raw((size_t)w * h);
  if (std::fread(raw.data(), 1, raw.size(), fp) != raw.size()) return false;
  std::fclose(fp);
  img.assign(raw.begin(), raw.end());
  return true;
}

int main(int argc, char **argv) {
  if (argc < 2) {
    std::printf("usage: %s gray1.pgm\n", argv[0]);
    return 2;
  }
  std::vector<float> im;
  int w = 0, h = 0;
  if (!read_pgm(argv[1], im, w, h)) return 2;
  if (!deviceInit(0)) return 2;
  int failures = 0;
  {
    const int kFrames = 4, kStepX = 16, kStepY = 8;
    const int cw = w - (kFrames - 1) * kStepX, ch = h - (kFrames - 1) * kStepY;
    const double depth = 5.0;
    const cusift_camera camera = {500.0f, 500.0f, 0.5f * cw, 0.5f * ch, 0.0f, 1000.0f, 0};
    std::vector<SiftData *> frames;
    std::vector<double> poses;
    for (int k = 0; k < kFrames; k++) {
      std::vector<float> crop((size_t)cw * ch);
      for (int y = 0; y < ch; y++)
        for (int x = 0; x < cw; x++) crop[(size_t)y * cw + x] = im[(size_t)(y + k * kStepY) * w + x + k * kStepX];
      cuImage img(cw, ch, crop.data());
      frames.push_back(new SiftData(4096, true, true));
      ExtractSift(*frames.back(), img, 4, 0.0, 2.0f);
      // crop k starts kStep * k pixels further along: the camera has moved by that many pixels at the plane's depth
      const double rt[12] = {1, 0, 0, k * kStepX * depth / camera.fx, 0, 1, 0, k * kStepY * depth / camera.fy, 0, 0, 1, 0};
      poses.insert(poses.end(), rt, rt + 12);
    }
    std::vector<std::pair<int, int> > pairs;  // every pair of the four frames
    for (int a = 0; a < kFrames; a++)
      for (int b = a + 1; b < kFrames; b++) pairs.push_back(std::make_pair(a, b));
    SiftTracks tracks;
    std::vector<unsigned int> stats;
    BuildTracks(frames, pairs, tracks, 2, true, 999.0f, 0.8f, 1, 1, NULL, &stats);
    int views[kFrames + 1] = {0}, consistent = 0;
    size_t observations = 0;
    for (size_t t = 0; t < tracks.size(); t++) {
      const std::vector<std::pair<int, int> > &tr = tracks[t];
      observations += tr.size();
      if (tr.size() < 2 || tr.size() > (size_t)kFrames) {
        ++failures;
        continue;
      }
      views[tr.size()]++;
      bool same = true;
      for (size_t e = 0; e < tr.size(); e++) {
        if (e > 0 && tr[e].first <= tr[e - 1].first) ++failures;  // frames ascending, one record per frame
        if (tr[e].second < 0 || tr[e].second >= frames[tr[e].first]->numPts) ++failures;
        const SiftPoint &p = frames[tr[e].first]->h_data[tr[e].second], &q = frames[tr[0].first]->h_data[tr[0].second];
        const float dx = (p.coords2D[0] + tr[e].first * kStepX) - (q.coords2D[0] + tr[0].first * kStepX);
        const float dy = (p.coords2D[1] + tr[e].first * kStepY) - (q.coords2D[1] + tr[0].first * kStepY);
        same = same && std::fabs(dx) < 1.0f && std::fabs(dy) < 1.0f;
      }
      consistent += same;
    }
    if (stats.size() != 8 || stats[0] != tracks.size() || stats[1] != observations) ++failures;
    std::printf("tracks %zu observations %zu accepted %u shared %u\n", tracks.size(), observations, stats[2], stats[3]);
    std::printf("views %d %d %d\n", views[2], views[3], views[4]);
    std::printf("consistent %d\n", consistent);
    if (tracks.size() < 100 || views[4] < 50 || consistent < 0.95 * tracks.size()) ++failures;

    // three views at least, one direction only: fewer or as many tracks, none of two views
    SiftTracks longer;
    BuildTracks(frames, pairs, longer, 3, false);
    for (size_t t = 0; t < longer.size(); t++)
      if (longer[t].size() < 3) ++failures;
    if (longer.empty()) ++failures;

    std::vector<int> front;
    std::vector<double> points = TriangulateTracks(frames, tracks, poses, camera, 1e-12, &front);
    int at_depth = 0;
    if (points.size() != 4 * tracks.size() || front.size() != tracks.size()) ++failures;
    for (size_t t = 0; t < tracks.size() && 4 * t + 3 < points.size(); t++)
      at_depth += std::fabs(points[4 * t + 2] - depth) < 0.25 && front[t] == (int)tracks[t].size();
    std::printf("depth %d\n", at_depth);
    if (at_depth < 0.9 * consistent) ++failures;
    for (size_t k = 0; k < frames.size(); k++) delete frames[k];
  }
  cusift_dropin::shutdown();
  std::printf(failures ? "FAILED (%d)\n" : "PASSED\n", failures);
  return failures ? 1 : 0;
}
