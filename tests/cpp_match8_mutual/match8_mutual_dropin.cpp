// The mutual 8-bit matcher and the match-bits setting through the drop-in headers (include/matching.h, homography.h), from
// plain C++ (g++), no HIP headers.  The PGM fixture is extracted at two thresholds, which gives two record sets of one
// scene.
//   1. MatchSiftData8Mutual(set 1, set 2), its fields kept, against MatchSiftData8 run in both directions afterwards: the
//      five match fields of every record of both sets are the same bytes, and the returned pairs are the forward call's
//      pairs whose partner points back.
//   2. SetMatchBits(8) + RegisterPlanar against the staged route QuantizeSiftData + MatchSiftData8 + EstimateHomography
//      with the same seed: the same homography, bit for bit, and the same counts.  SetMatchBits(32) afterwards.
//
//   match8_mutual_dropin tests/golden/gray1.pgm
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "cuImage.h"
#include "cuSIFT.h"
#include "homography.h"
#include "matching.h"

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

// the five match fields of every record: score, ambiguity, match, match_xpos, match_ypos
struct Fields {
  float v[5];
};
static std::vector<Fields> fields_of(const SiftData &a) {
  std::vector<Fields> out((size_t)a.numPts);
  for (int i = 0; i < a.numPts; i++) std::memcpy(out[i].v, &a.h_data[i].score, sizeof(Fields));
  return out;
}
static int fields_differ(const std::vector<Fields> &a, const std::vector<Fields> &b) {
  if (a.size() != b.size()) return 1;
  int bad = 0;
  for (size_t i = 0; i < a.size(); i++) bad += std::memcmp(a[i].v, b[i].v, sizeof(Fields)) != 0;
  return bad;
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
    cuImage img(w, h, im.data());
    SiftData data1(8192, true, true), data2(8192, true, true);
    ExtractSift(data1, img, 4, 0.0, 1.0f);
    ExtractSift(data2, img, 4, 0.0, 2.0f);
    if (data1.numPts <= data2.numPts || data2.numPts < 100) ++failures;
    SiftDescriptors8 desc1, desc2;
    QuantizeSiftData(data1, desc1);
    QuantizeSiftData(data2, desc2);

    // 1. both directions from one pass against the two directions one after the other
    std::vector<SiftMatch *> mutual = MatchSiftData8Mutual(data1, desc1, data2, desc2, MatchSiftDistanceL2, 999.0f, 0.8f);
    std::vector<int> got;
    for (SiftMatch *m : mutual) {
      got.push_back((int)(m->pt1 - data1.h_data));
      got.push_back((int)(m->pt2 - data2.h_data));
    }
    const std::vector<Fields> both1 = fields_of(data1), both2 = fields_of(data2);
    std::vector<SiftMatch *> bwd = MatchSiftData8(data2, desc2, data1, desc1, MatchSiftDistanceL2, 999.0f, 0.8f);
    std::vector<SiftMatch *> fwd = MatchSiftData8(data1, desc1, data2, desc2, MatchSiftDistanceL2, 999.0f, 0.8f);
    const int d1 = fields_differ(both1, fields_of(data1)), d2 = fields_differ(both2, fields_of(data2));
    std::printf("fields: %d of %d records of set 1 differ, %d of %d of set 2\n", d1, data1.numPts, d2, data2.numPts);
    failures += d1 + d2;
    std::vector<int> want;
    for (SiftMatch *m : fwd) {
      const int i = (int)(m->pt1 - data1.h_data), j = (int)(m->pt2 - data2.h_data);
      if (data2.h_data[j].match == i) {
        want.push_back(i);
        want.push_back(j);
      }
    }
    std::printf("pairs: %zu forward, %zu backward, %zu mutual, %zu expected\n", fwd.size(), bwd.size(), mutual.size(),
                want.size() / 2);
    if (got != want || mutual.empty() || mutual.size() > fwd.size()) ++failures;
    for (SiftMatch *m : mutual) delete m;
    for (SiftMatch *m : fwd) delete m;
    for (SiftMatch *m : bwd) delete m;

    // 2. the setting: RegisterPlanar at 8 bits against the staged route on set 1, which carries MatchSiftData8's fields
    float staged[9], fused[9];
    int staged_matches = -1, staged_fit = -1, fused_matches = -2, fused_fit = -2;
    EstimateHomography(data1, staged, &staged_matches, &staged_fit, 1008, 999.0f, 0.8f, 5.0f, 5, 3.0f, 5, 1, nullptr,
                       data2.numPts);
    SetMatchBits(8);
    RegisterPlanar(data1, data2, fused, &fused_matches, &fused_fit, 1008, 999.0f, 0.8f, 5.0f, 5, 3.0f, 5, 1, 1);
    SetMatchBits(32);
    std::printf("planar: %d inliers, %d fit (staged %d, %d)\n", fused_matches, fused_fit, staged_matches, staged_fit);
    if (std::memcmp(staged, fused, sizeof(staged)) != 0 || staged_matches != fused_matches || staged_fit != fused_fit)
      ++failures;
    if (fused_matches < 50) ++failures;
  }
  cusift_dropin::shutdown();
  std::printf(failures ? "FAILED (%d)\n" : "PASSED\n", failures);
  return failures ? 1 : 0;
}
