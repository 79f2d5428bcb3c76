// MatchSiftDataMutual (include/matching.h) from plain C++ (g++), no HIP headers: VLFeat descriptor dumps in, the
// cross-checked pairs out.  Checks made here: every returned pair passes the thresholds and names each other, nothing that
// does is missing, the list is a subset of MatchSiftData's at the same thresholds, and data1's match fields are the ones
// MatchSiftData writes.  The pair list is printed ("pair i j", ascending i) for the caller to compare.
// Usage: mutual_dropin <vlfeat_sift1.bin> <vlfeat_sift2.bin> <score threshold> <ambiguity threshold>
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
    const int n1 = data1.numPts, n2 = data2.numPts;

    // the one-directional call first: its pairs, and data1's fields as it leaves them
    std::vector<SiftMatch *> plain = MatchSiftData(data1, data2, MatchSiftDistanceL2, score, amb);
    std::vector<char> is_plain((size_t)n1, 0);
    for (SiftMatch *m : plain) is_plain[(size_t)(m->pt1 - data1.h_data)] = 1;
    const size_t n_plain = plain.size();
    for (SiftMatch *m : plain) delete m;
    std::vector<SiftPoint> rows(data1.h_data, data1.h_data + n1);

    std::vector<SiftMatch *> mutual = MatchSiftDataMutual(data1, data2, MatchSiftDistanceL2, score, amb);
    if (std::memcmp(rows.data(), data1.h_data, sizeof(SiftPoint) * (size_t)n1) != 0) {
      std::printf("data1's match fields differ from MatchSiftData's\n");
      ++failures;
    }
    const float s2 = score * score, a2 = amb * amb;
    int expected = 0;
    for (int i = 0; i < n1; i++) {
      const SiftPoint &p = data1.h_data[i];
      expected += p.score < s2 && p.ambiguity < a2 && p.match >= 0 && p.match < n2 && data2.h_data[p.match].match == i;
    }
    int last = -1;
    for (SiftMatch *m : mutual) {
      const int i = (int)(m->pt1 - data1.h_data), j = (int)(m->pt2 - data2.h_data);
      const bool ok = i > last && i < n1 && j >= 0 && j < n2 && m->pt1->match == j && m->pt2->match == i &&
                      m->pt1->score < s2 && m->pt1->ambiguity < a2 && is_plain[(size_t)i] &&
                      m->score == m->pt1->score && m->ambiguity == m->pt1->ambiguity;
      if (!ok) ++failures;
      last = i;
      std::printf("pair %d %d\n", i, j);
    }
    std::printf("mutual: %zu of %zu matches are cross-checked (%d expected from the fields)\n", mutual.size(), n_plain,
                expected);
    if ((int)mutual.size() != expected || mutual.empty() || mutual.size() >= n_plain) ++failures;
    // record j's match must be a record of data1 for every j (884 real descriptors: nothing scores 999)
    for (int j = 0; j < n2; j++)
      if (data2.h_data[j].match < 0 || data2.h_data[j].match >= n1) ++failures;
    for (SiftMatch *m : mutual) delete m;
  }
  cusift_dropin::shutdown();
  std::printf(failures ? "FAILED (%d)\n" : "PASSED\n", failures);
  return failures ? 1 : 0;
}
