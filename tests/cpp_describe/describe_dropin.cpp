// Descriptors for records the caller supplies, through the drop-in headers: SiftData::Describe over an extraction's own
// records (wiped first: they must come back byte for byte) and the free DescribeSift over keypoints that AddSiftData put
// on the device (position and scale only), on the PGM fixture.  Plain C++ (g++), no HIP headers.
//
//   describe_dropin tests/golden/gray1.pgm    prints "described <n> records: <a> round-trip mismatches, <b> from AddSiftData"
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "cuImage.h"
#include "cuSIFT.h"
#include "debug.h"

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

static int mismatches(const SiftPoint *a, const SiftPoint *b, int n) {
  int bad = 0;
  for (int i = 0; i < n; i++) bad += std::memcmp(a + i, b + i, sizeof(SiftPoint)) != 0;
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
  cuImage img(w, h, im.data());

  int failures = 0;
  for (int root = 0; root < 2; root++) {
    SiftData data(8192, true, true);
    data.rootSift = root != 0;
    data.numOctaves = 5;
    data.peakThresh = 1.0f;
    data.Extract(img);
    const int n = data.numPts;
    if (n < 500 || n >= data.maxPts) ++failures;
    const std::vector<SiftPoint> want(data.h_data, data.h_data + n);

    // Extract, copy the records, wipe orientation and descriptor, Describe, compare bytes
    std::vector<SiftPoint> wiped(want);
    for (SiftPoint &p : wiped) {
      p.orientation = std::numeric_limits<float>::quiet_NaN();
      for (float &v : p.data) v = std::numeric_limits<float>::quiet_NaN();
    }
    safeCall(cusift_memcpy_h2d(cusift_dropin::ctx(), data.d_data, wiped.data(), sizeof(SiftPoint) * (size_t)n));
    data.Describe(img);
    const int bad_round = mismatches(data.h_data, want.data(), n);

    // keypoints from the host -- position and scale, nothing else -- through AddSiftData, then the free function
    std::vector<SiftPoint> given((size_t)n);
    std::memset(given.data(), 0, sizeof(SiftPoint) * given.size());
    for (int i = 0; i < n; i++) {
      given[(size_t)i].coords2D[0] = want[(size_t)i].coords2D[0];
      given[(size_t)i].coords2D[1] = want[(size_t)i].coords2D[1];
      given[(size_t)i].scale = want[(size_t)i].scale;
    }
    SiftData added(1024, true, true);
    added.rootSift = root != 0;
    AddSiftData(added, given.data(), n);  // grows past 1024
    if (added.numPts != n) ++failures;
    DescribeSift(added, img, 5);
    int bad_added = 0;
    for (int i = 0; i < n; i++) {
      const SiftPoint &a = added.h_data[i], &b = want[(size_t)i];
      bad_added += a.subsampling != b.subsampling || std::memcmp(&a.orientation, &b.orientation, sizeof(float)) != 0 ||
                   std::memcmp(a.data, b.data, sizeof(a.data)) != 0 || a.sharpness != 0.0f || a.coords2D[0] != b.coords2D[0];
    }
    // kept orientations (the previous call's) and the octave from the scale: the same records again
    DescribeSift(added, img, 5, 1.0f, CUSIFT_DESCRIBE_KEEP_ORIENTATION | CUSIFT_DESCRIBE_OCTAVE_FROM_SCALE);
    for (int i = 0; i < n; i++)
      bad_added += std::memcmp(&added.h_data[i].orientation, &want[(size_t)i].orientation, sizeof(float)) != 0 ||
                   std::memcmp(added.h_data[i].data, want[(size_t)i].data, sizeof(want[0].data)) != 0;
    std::printf("described %d records%s: %d round-trip mismatches, %d from AddSiftData\n", n, root ? " (RootSIFT)" : "",
                bad_round, bad_added);
    failures += bad_round + bad_added;
  }
  std::printf(failures ? "FAILED (%d)\n" : "PASSED\n", failures);
  return failures ? 1 : 0;
}
