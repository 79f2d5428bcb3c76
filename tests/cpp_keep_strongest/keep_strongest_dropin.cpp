// The K strongest keypoints through the drop-in header: SiftData::keepStrongest and the legacy ExtractSift with its new
// trailing keepStrongest argument, on the PGM fixture.  Plain C++ (g++), no HIP headers.
//
//   keep_strongest_dropin tests/golden/gray1.pgm    prints "kept <K> of <count>: weakest kept <a>, strongest dropped <b>"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <vector>

#include "cuImage.h"
#include "cuSIFT.h"

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

static float strength(const SiftPoint &p) { return std::isfinite(p.sharpness) ? std::fabs(p.sharpness) : 0.0f; }

int main(int argc, char **argv) {
  if (argc < 2) {
    std::printf("usage: %s gray1.pgm\n", argv[0]);
    return 2;
  }
  std::vector<float> im;
  int w = 0, h = 0;
  if (!read_pgm(argv[1], im, w, h)) return 2;
  if (!deviceInit(0)) return 2;
  cuImage img(w, h, im.data());

  int failures = 0;
  const int K = 500;
  SiftData all(8192, true, true), kept(8192, true, true), field(8192, true, true);
  if (kept.keepStrongest != 0) ++failures;  // off by default
  ExtractSift(all, img, 5, 0.0, 1.0f);
  ExtractSift(kept, img, 5, 0.0, 1.0f, 0.0f, 1.0f, false, K);
  if (kept.keepStrongest != K) ++failures;
  if (all.numPts <= K || all.numPts >= all.maxPts || kept.numPts != K) ++failures;
  // the K-th strongest of the unselected run bounds both sides of the cut
  std::vector<float> s;
  for (int i = 0; i < all.numPts; i++) s.push_back(strength(all.h_data[i]));
  std::sort(s.begin(), s.end(), [](float a, float b) { return a > b; });
  const float weakest_allowed = s[(size_t)std::min(K, all.numPts) - 1];
  const float strongest_dropped = all.numPts > K ? s[(size_t)K] : 0.0f;
  float weakest_kept = 1e30f;
  for (int i = 0; i < kept.numPts; i++) {
    weakest_kept = std::min(weakest_kept, strength(kept.h_data[i]));
    if (i > 0 && kept.h_data[i].subsampling > kept.h_data[i - 1].subsampling) ++failures;  // coarsest first
  }
  std::printf("kept %d of %d: weakest kept %g, strongest dropped %g\n", kept.numPts, all.numPts, weakest_kept, strongest_dropped);
  if (!(weakest_kept >= strongest_dropped) || weakest_kept != weakest_allowed) ++failures;
  // the field alone does the same as the argument
  field.numOctaves = 5;
  field.initBlur = 0.0;
  field.peakThresh = 1.0f;
  field.keepStrongest = K;
  field.Extract(img);
  if (field.numPts != K) ++failures;
  // ... and the short ExtractSift turns it off again, on the same SiftData and the same thread's context
  ExtractSift(kept, img, 5, 0.0, 1.0f);
  if (kept.keepStrongest != 0 || kept.numPts != all.numPts) ++failures;
  std::printf(failures ? "FAILED (%d)\n" : "PASSED\n", failures);
  return failures ? 1 : 0;
}
