// 8-bit descriptors through the drop-in headers (include/matching.h): extract, QuantizeSiftData, MatchSiftData8, from
// plain C++ (g++), no HIP headers.  The PGM fixture is extracted twice, at two thresholds, which gives two different
// record sets of one scene; both are quantised (with a host copy of the bytes) and matched in L2 mode.
//
//   match8_dropin tests/golden/gray1.pgm <records.bin> <score threshold> <ambiguity threshold>
//
// prints  "counts <n1> <n2> <matches>", "bytes <checksum of set 1's bytes> <of set 2's>", "fields <checksum of the five match
// fields of set 1>", "pairs <checksum of the returned (i, j)>" and writes the two record sets as extracted (int n1, int n2,
// n1 records, n2 records) to <records.bin>, from which tests/test_cpp_match8.py recomputes all of it in numpy.  A checksum
// is sum_i (i + 1) * byte_i modulo 2^64.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "cuImage.h"
#include "cuSIFT.h"
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

struct Checksum {
  uint64_t sum = 0, i = 0;
  void add(const void *p, size_t bytes) {
    const unsigned char *b = static_cast<const unsigned char *>(p);
    for (size_t k = 0; k < bytes; k++) sum += ++i * b[k];
  }
};

int main(int argc, char **argv) {
  if (argc < 5) {
    std::printf("usage: %s gray1.pgm records.bin score_threshold ambiguity_threshold\n", argv[0]);
    return 2;
  }
  const float score = (float)std::atof(argv[3]), amb = (float)std::atof(argv[4]);
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
    FILE *fp = std::fopen(argv[2], "wb");
    if (!fp) return 2;
    std::fwrite(&data1.numPts, sizeof(int), 1, fp);
    std::fwrite(&data2.numPts, sizeof(int), 1, fp);
    std::fwrite(data1.h_data, sizeof(SiftPoint), (size_t)data1.numPts, fp);
    std::fwrite(data2.h_data, sizeof(SiftPoint), (size_t)data2.numPts, fp);
    std::fclose(fp);

    SiftDescriptors8 desc1, desc2;
    InitSiftDescriptors8(desc1, data1.numPts, true);
    InitSiftDescriptors8(desc2, 16, true);  // too small: QuantizeSiftData grows it and keeps the host copy
    QuantizeSiftData(data1, desc1);
    QuantizeSiftData(data2, desc2);
    if (desc1.numPts != data1.numPts || desc2.numPts != data2.numPts || !desc2.h_data || desc2.maxPts < data2.numPts)
      ++failures;
    std::vector<SiftMatch *> matches = MatchSiftData8(data1, desc1, data2, desc2, MatchSiftDistanceL2, score, amb);
    Checksum b1, b2, fields, pairs;
    b1.add(desc1.h_data, (size_t)128 * data1.numPts);
    b2.add(desc2.h_data, (size_t)128 * data2.numPts);
    for (int i = 0; i < data1.numPts; i++) fields.add(&data1.h_data[i].score, 5 * sizeof(float));
    for (SiftMatch *m : matches) {
      const int ij[2] = {(int)(m->pt1 - data1.h_data), (int)(m->pt2 - data2.h_data)};
      pairs.add(ij, sizeof(ij));
      if (m->score != m->pt1->score || m->ambiguity != m->pt1->ambiguity) ++failures;
      delete m;
    }
    std::printf("counts %d %d %zu\n", data1.numPts, data2.numPts, matches.size());
    std::printf("bytes %llu %llu\n", (unsigned long long)b1.sum, (unsigned long long)b2.sum);
    std::printf("fields %llu\n", (unsigned long long)fields.sum);
    std::printf("pairs %llu\n", (unsigned long long)pairs.sum);
    if (matches.empty()) ++failures;
    FreeSiftDescriptors8(desc1);
    if (desc1.d_data || desc1.maxPts) ++failures;
  }
  cusift_dropin::shutdown();
  std::printf(failures ? "FAILED (%d)\n" : "PASSED\n", failures);
  return failures ? 1 : 0;
}
