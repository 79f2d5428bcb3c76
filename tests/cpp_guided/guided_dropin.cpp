// MatchSiftDataGuided (include/matching.h) from plain C++ (g++), no HIP headers: VLFeat descriptor dumps in.  Two cases,
// each against MatchSiftData at the same thresholds: under a radius that every pair passes the guided call must leave the
// same bytes in data1's records and return the same pairs, under both kinds of model; under a model of nine zeros, which
// passes nothing, every record must come back with match == -1 and no pair may be returned.
// Usage: guided_dropin <vlfeat_sift1.bin> <vlfeat_sift2.bin> <score threshold> <ambiguity threshold>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "cuSIFT.h"
#include "debug.h"
#include "matching.h"

int main(int argc, char **argv) {
  if (argc < 5) return 2;
  const float score = (float)std::atof(argv[3]), amb = (float)std::atof(argv[4]);
  InitCuda(0);
  int failures = 0;
  {
    SiftData data1, data2;
    if (ReadVLFeatSiftData(data1, argv[1]) < 0 || ReadVLFeatSiftData(data2, argv[2]) < 0) return 2;
    const int n1 = data1.numPts;

    std::vector<SiftMatch *> plain = MatchSiftData(data1, data2, MatchSiftDistanceL2, score, amb);
    std::vector<int> plain_pairs;
    for (SiftMatch *m : plain) {
      plain_pairs.push_back((int)(m->pt1 - data1.h_data));
      plain_pairs.push_back((int)(m->pt2 - data2.h_data));
      delete m;
    }
    const std::vector<SiftPoint> rows(data1.h_data, data1.h_data + n1);
    std::printf("plain: %zu pairs of %d records\n", plain_pairs.size() / 2, n1);
    if (plain_pairs.empty()) ++failures;

    // a huge radius: the same call, under a homography and under a fundamental matrix
    const double ident[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, shift[9] = {0, 0, 0, 0, 0, -1, 0, 1, 0};
    const double *models[2] = {ident, shift};
    for (int model = CUSIFT_GUIDE_HOMOGRAPHY; model <= CUSIFT_GUIDE_EPIPOLAR; ++model) {
      std::memset((void *)&data1.h_data[0].score, 0xCD, 5 * sizeof(float));  // the call must write it again
      std::vector<SiftMatch *> wide = MatchSiftDataGuided(data1, data2, model, models[model], 1e6f, MatchSiftDistanceL2,
                                                          score, amb);
      if (std::memcmp(rows.data(), data1.h_data, sizeof(SiftPoint) * (size_t)n1) != 0) {
        std::printf("model %d, radius 1e6: data1's records differ from MatchSiftData's\n", model);
        ++failures;
      }
      std::vector<int> pairs;
      for (SiftMatch *m : wide) {
        pairs.push_back((int)(m->pt1 - data1.h_data));
        pairs.push_back((int)(m->pt2 - data2.h_data));
        if (m->score != m->pt1->score || m->ambiguity != m->pt1->ambiguity) ++failures;
        delete m;
      }
      if (pairs != plain_pairs) {
        std::printf("model %d, radius 1e6: %zu pairs, MatchSiftData returned %zu\n", model, pairs.size() / 2,
                    plain_pairs.size() / 2);
        ++failures;
      }
    }

    // nine zeros pass nothing
    const double zero[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int model = CUSIFT_GUIDE_HOMOGRAPHY; model <= CUSIFT_GUIDE_EPIPOLAR; ++model) {
      std::vector<SiftMatch *> none = MatchSiftDataGuided(data1, data2, model, zero, 5.0f, MatchSiftDistanceL2, score, amb);
      int unmatched = 0;
      for (int i = 0; i < n1; i++) unmatched += data1.h_data[i].match == -1 && data1.h_data[i].score == 999.0f;
      std::printf("model %d, zero model: %d of %d records unmatched, %zu pairs\n", model, unmatched, n1, none.size());
      if (unmatched != n1 || !none.empty()) ++failures;
      for (SiftMatch *m : none) delete m;
    }
  }
  cusift_dropin::shutdown();
  std::printf(failures ? "FAILED (%d)\n" : "PASSED\n", failures);
  return failures ? 1 : 0;
}
