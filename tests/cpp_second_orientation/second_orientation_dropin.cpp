// Second-peak orientations through the drop-in header: SiftData::secondOrientation on an unchanged-style cuSIFT program,
// and the free SecondOrientationsSift on the records of a plain extraction, on the PGM fixture.  Plain C++ (g++), no HIP
// headers.
//
//   second_orientation_dropin tests/golden/gray1.pgm <keypoints> <records with duplicates>
//   prints "second orientations: <n> keypoints, <m> duplicates, <a> head mismatches, <b> out of order"
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

// a duplicate's record equals its parent's but for the orientation and the descriptor
static bool same_but_orientation(const SiftPoint &a, const SiftPoint &b) {
  SiftPoint x = a, y = b;
  x.orientation = y.orientation = 0.0f;
  std::memset(x.data, 0, sizeof(x.data));
  std::memset(y.data, 0, sizeof(y.data));
  return std::memcmp(&x, &y, sizeof(SiftPoint)) == 0;
}

// the records [n, total) of `d`: each one's parent among [0, n), in ascending parent index, at another orientation
static void check_duplicates(const SiftData &d, int n, int &mismatches, int &disorder) {
  int last = -1;
  for (int k = n; k < d.numPts; k++) {
    int parent = -1;
    for (int j = 0; j < n && parent < 0; j++)
      if (same_but_orientation(d.h_data[k], d.h_data[j])) parent = j;
    if (parent < 0 || d.h_data[k].orientation == d.h_data[parent].orientation) ++mismatches;
    if (parent <= last) ++disorder;
    last = parent;
  }
}

int main(int argc, char **argv) {
  if (argc < 4) {
    std::printf("usage: %s gray1.pgm <keypoints> <records with duplicates>\n", argv[0]);
    return 2;
  }
  const int want_n = std::atoi(argv[2]), want_total = std::atoi(argv[3]);
  std::vector<float> im;
  int w = 0, h = 0;
  if (!read_pgm(argv[1], im, w, h)) return 2;
  if (!deviceInit(0)) return 2;
  cuImage img(w, h, im.data());

  int failures = 0;
  SiftData plain(1024, true, true), data(1024, true, true);
  if (data.secondOrientation != 0.0f) ++failures;  // off by default
  ExtractSift(plain, img, 5, 0.0, 3.0f);
  data.numOctaves = 5;
  data.initBlur = 0.0;
  data.peakThresh = 3.0f;
  data.secondOrientation = 0.8f;
  data.Extract(img);
  const int n = plain.numPts;
  if (n != want_n || data.numPts != want_total) ++failures;
  int mismatches = 0, disorder = 0;
  check_duplicates(data, n, mismatches, disorder);
  std::printf("second orientations: %d keypoints, %d duplicates, %d head mismatches, %d out of order\n", n, data.numPts - n,
              mismatches, disorder);
  if (mismatches || disorder) ++failures;
  // the stage on the records of the plain extraction: the same count, the same layout
  SecondOrientationsSift(plain, img, 5);
  if (plain.numPts != want_total) ++failures;
  check_duplicates(plain, n, mismatches, disorder);
  if (mismatches || disorder) ++failures;
  // ... and the setting off again, on the same SiftData and the same thread's context
  data.secondOrientation = 0.0f;
  data.Extract(img);
  if (data.numPts != want_n) ++failures;
  std::printf(failures ? "FAILED (%d)\n" : "PASSED\n", failures);
  return failures ? 1 : 0;
}
