// Octave -1 through the drop-in header: the legacy ExtractSift with its new trailing scaleUp argument, and the
// SiftData::scaleUp field behind it, on the PGM fixture.  Plain C++ (g++), no HIP headers.
//
//   upsample_dropin tests/golden/gray1.pgm      prints "scaleUp: <count> points, smallest subsampling <s>, ..."
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
  SiftData plain(8192, true, true), up(8192, true, true);
  if (up.scaleUp) ++failures;  // off by default
  ExtractSift(plain, img, 5, 0.0, 1.0f);
  ExtractSift(up, img, 6, 0.0, 1.0f, 0.0f, 1.0f, true);  // octaves -1 .. 4
  if (!up.scaleUp) ++failures;
  float smallest = 1e30f, largest = 0.0f;
  int n_half = 0;
  for (int i = 0; i < up.numPts; i++) {
    const SiftPoint &pt = up.h_data[i];
    smallest = pt.subsampling < smallest ? pt.subsampling : smallest;
    largest = pt.subsampling > largest ? pt.subsampling : largest;
    n_half += pt.subsampling == 0.5f;
    // coordinates are base-image pixels whichever octave found the point
    if (!(pt.coords2D[0] >= 0.0f && pt.coords2D[0] < (float)w && pt.coords2D[1] >= 0.0f && pt.coords2D[1] < (float)h)) ++failures;
    if (i > 0 && pt.subsampling > up.h_data[i - 1].subsampling) ++failures;  // coarsest first, octave -1 last
  }
  float plain_smallest = 1e30f;
  for (int i = 0; i < plain.numPts; i++)
    plain_smallest = plain.h_data[i].subsampling < plain_smallest ? plain.h_data[i].subsampling : plain_smallest;
  std::printf("plain: %d points, smallest subsampling %g\n", plain.numPts, plain_smallest);
  std::printf("scaleUp: %d points, smallest subsampling %g, largest %g, %d at 0.5\n", up.numPts, smallest, largest, n_half);
  if (plain_smallest != 1.0f || smallest != 0.5f || n_half < 1 || up.numPts <= plain.numPts || up.numPts >= up.maxPts) ++failures;
  // the field alone does the same as the argument
  SiftData again(8192, true, true);
  again.numOctaves = 6;
  again.initBlur = 0.0;
  again.peakThresh = 1.0f;
  again.scaleUp = true;
  again.Extract(img);
  if (again.numPts != up.numPts) ++failures;
  std::printf(failures ? "FAILED (%d)\n" : "PASSED\n", failures);
  return failures ? 1 : 0;
}
