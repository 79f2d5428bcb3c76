// match_tile.inc -- the body shared by match_kernel and match_batch_kernel (sift_match.hip): one workgroup's 64 rows
// (descriptors p1_base .. p1_base + 15 of this wave) against the columns [col_begin, col_end) of sift2.  Included inside
// a kernel that has in scope: kL2, kInit, sB, lane, wv, r, g, p1_base, sift1, n1, sift2, col_begin, col_end, cols and
// guide.  On exit lane r == 0 of every 16-lane group g holds best[q], second[q], bidx[q] of rows p1_base + 4 g + q
// (q = 0..3).
// One text, so that a (row, column) dot product is the same k-ordered MFMA chain whichever kernel computes it.
// `cols` is the column side (sift_match.hip): NoColumnSide in the one-directional kernels, whose three calls below are
// empty inline functions -- no barrier, no LDS, no register (tools/kernel_regs.py: 96 VGPRs, 16,896 B as before);
// ColumnSide in the mutual kernels.
// `guide` is the geometric predicate of the guided kernels (sift_match.hip): NoGuide everywhere else, again nothing but
// empty inline functions; GuideH / GuideF keep the per-row terms of this lane's rows 4g + q in registers (rows()), stage
// coords2D of a tile's 32 columns into floats 128..129 of the columns' LDS rows (fetch() / store(), the descriptors'
// range-checked buffer resource, no new LDS) and turn a (row, column) that fails the test into kInit in the update.
  // A fragments: lane (r, g) holds elements 16u + 4g + j of descriptor p1_base + r (u = 0..7, j = 0..3)
  float a[8][4];
  {
    const float *d1 = sift1[min(p1_base + r, n1 - 1)].data;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const f4u v = *reinterpret_cast<const f4u *>(d1 + 16 * u + 4 * g);
#pragma unroll
      for (int j = 0; j < 4; ++j) a[u][j] = v[j];
    }
  }
  // running top-2 of rows 4g + q for the columns this lane sees (p2 = r mod 16): reference thread tx = r
  float best[4], second[4];
  int bidx[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    best[q] = second[q] = kInit;
    bidx[q] = -1;
  }
  guide.rows(sift1, n1, p1_base, lane);

  // staging: thread t moves four 16-byte chunks per tile; chunk c = t + 256 i -> descriptor c >> 5, floats 4 (c & 31).
  // Raw buffer loads from a descriptor based at this split's first column: the lane offset is computed once, the tile
  // and the chunk row advance in the scalar offset, and columns past col_end read as 0 (their scores are masked below).
  const __amdgpu_buffer_rsrc_t rsrc2 = __builtin_amdgcn_make_buffer_rsrc(
      (void *)(sift2 + col_begin), 0, (int)((col_end > col_begin ? col_end - col_begin : 0) * sizeof(cusift_point)),
      kBufFlags);
  constexpr int kRec = (int)sizeof(cusift_point);
  const int voff = (int)(threadIdx.x >> 5) * kRec + (int)offsetof(cusift_point, data) + 16 * (int)(threadIdx.x & 31);
  u4 stage[4];
  auto fetch = [&](int c0) {
    const int soff = __builtin_amdgcn_readfirstlane((c0 - col_begin) * kRec);
#pragma unroll
    for (int i = 0; i < 4; ++i) stage[i] = __builtin_amdgcn_raw_buffer_load_b128(rsrc2, voff, soff + 8 * i * kRec, 0);
    guide.fetch(rsrc2, soff);
  };
  if (col_begin < col_end) fetch(col_begin);
  const float *brow = sB + r * kBStride + 4 * g;
  for (int c0 = col_begin; c0 < col_end; c0 += kMatchTileCols) {
    __syncthreads();  // the previous tile has been consumed
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = threadIdx.x + 256 * i;
      *reinterpret_cast<u4 *>(sB + (c >> 5) * kBStride + 4 * (c & 31)) = stage[i];
    }
    guide.store(sB);
    __syncthreads();
    if (c0 + kMatchTileCols < col_end) fetch(c0 + kMatchTileCols);  // in flight while this tile is multiplied
    if (c0 > col_begin) cols.drain(c0 - kMatchTileCols, col_begin, col_end, lane, wv);  // the previous tile's columns
    // this lane's two columns' coordinates, read in front of the MFMAs so that the update does not wait for LDS
    const auto xy2a = guide.column(sB, r), xy2b = guide.column(sB, 16 + r);

    // two independent 16x16 accumulators (columns c0 + r and c0 + 16 + r), each a k-ordered chain; the B fragments
    // of step u + 1 are read from LDS before the MFMAs of step u are issued
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    __builtin_amdgcn_s_setprio(1);  // a wave with MFMAs to issue goes before its SIMD's waves that are in the update
    f4 b0 = *reinterpret_cast<const f4 *>(brow);
    f4 b1 = *reinterpret_cast<const f4 *>(brow + 16 * kBStride);
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      f4 n0 = b0, n1v = b1;
      if (u < 7) {
        n0 = *reinterpret_cast<const f4 *>(brow + 16 * (u + 1));
        n1v = *reinterpret_cast<const f4 *>(brow + 16 * kBStride + 16 * (u + 1));
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u][j], b0[j], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u][j], b1[j], acc1, 0, 0, 0);
      }
      b0 = n0;
      b1 = n1v;
    }
    __builtin_amdgcn_s_setprio(0);
    // acc[q] = <descriptor p1_base + 4g + q, descriptor p2>.  (Deferring this update into the next tile's MFMA gaps
    // -- one score per step u -- was built and measured: no change, 110-112 TFLOP/s at 16k either way.)
    {
      const bool full = c0 + kMatchTileCols <= col_end;  // wave-uniform: only a split's last tile can be partial
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const int p2 = c0 + 16 * t + r;
        const bool live = full || p2 < col_end;
        const auto xy2 = t ? xy2b : xy2a;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float dot = t ? acc1[q] : acc0[q];
          // ComputeL2Distance :71-72, 2 - 2*dot (2*dot is exact, so the fused form has the same bits)
          float val = kL2 ? (dot > -1.0f ? __builtin_fmaf(-2.0f, dot, 2.0f) : kMatchFltMax) : dot;
          // `live` stays in the condition: a column past col_end reads as zeros, and (0, 0) can pass a guide
          val = (live && guide.pass(q, xy2)) ? val : kInit;
          top2_update<kL2>(best[q], second[q], bidx[q], val, p2);
        }
      }
    }
    cols.tile(c0, col_begin, acc0, acc1, p1_base, lane, wv);
  }
  cols.finish(col_begin, col_end, lane, wv);
  // tree over tx = r (extras/matching.cu:122-138,201-218): lane r < len takes lane r + len; ties keep the lower r
#pragma unroll
  for (int len = 8; len > 0; len >>= 1) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float ob = __shfl_down(best[q], len, 16);
      const float os = __shfl_down(second[q], len, 16);
      const int oi = __shfl_down(bidx[q], len, 16);
      if (r < len) {
        top2_scan(best[q], second[q], bidx[q], ob, oi, kL2);
        if (beats(os, second[q], kL2)) second[q] = os;
      }
    }
  }
