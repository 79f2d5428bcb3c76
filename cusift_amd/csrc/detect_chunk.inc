// detect_chunk.inc -- the body of the fused detection for ONE wave's chunk: local centre rows [ya, yb) of strip `bx` of
// one image.  Included, not called: detect_fused_kernel's code generation is sensitive to its shape -- as an inlined
// function the same statements compiled to 251 instead of 224 registers and the pipelined benchmark step ran 5 % slower
// (same-box A/B, round 3) -- so the kernels that share it (sift_stencils.hip: detect_fused_kernel, detect_multi_kernel)
// paste the text.  Names the including scope provides:
//   kIdent0, kRecBytes (compile time); img, w, h, pitch (this image); list, max_pts, counter (this image's keypoint
//   list); ya, yb, bx; rw (RowWindow: rw.row0 turns local rows into global ones); T (LaplaceTapsPk), P (FindParams);
//   cands (CandList), lane;  kDown (compile time) and, when it is set, down_img / down_pitch (the next octave's image
//   of this picture), DT (ScaleDownTaps), own_lo / own_hi (the source rows whose output rows this wave writes).
  const int c0 = bx * kDetStrip - kDetHaloLanes * kBlurCols + lane * kBlurCols;
  const EdgeFix4 edge(c0, w);  // any w >= 4
  const __amdgpu_buffer_rsrc_t rin =
      __builtin_amdgcn_make_buffer_rsrc((void *)img, 0, (int)((unsigned int)h * (unsigned int)pitch * 4u), kBufFlags);
  const bool lane_valid = lane >= kDetHaloLanes && lane < 64 - kDetHaloLanes;

  // The load and its border fix-up are separate: the fix-up is the first USE of the loaded registers, and it is
  // written where the row enters the window -- two row steps after the load was issued -- so that the wait for the
  // load sits there too (as one function the compiler fixed the row up, and waited, one row step after the issue).
  auto load_raw = [&](int y) -> f4 {
    // the row is wave-uniform, but the loop counter it derives from lives in a vector register (the compiler's
    // divergence analysis gives up across the candidate branches) and the load's scalar offset then went through a
    // waterfall loop (v_readfirstlane / compare / saveexec per row): say that it is uniform
    const int yc = clampi(__builtin_amdgcn_readfirstlane(y), 0, h - 1);
    return __builtin_bit_cast(f4, __builtin_amdgcn_raw_buffer_load_b128(rin, edge.voff, yc * pitch * 4, 0));
  };
  // Only the waves whose 256 columns reach the image's left or right border replace anything (two strips of eight at
  // 1080p): a wave-uniform branch around the seven selects of the fix-up (round 5, same-box A/B:
  // 64 x 1080p 1.154 -> 1.133 ms for a lone caller, 0.955 -> 0.944 on four streams; profiles/r05/ab_edge_uniform.txt)
  const bool edge_wave = bx == 0 || bx * kDetStrip - kDetHaloLanes * kBlurCols + 64 * kBlurCols > w;
  auto fix = [&](f4 v) -> f4 { return edge_wave ? edge(v) : v; };

  f4 win[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) win[i] = fix(load_raw(ya - 1 - 4 + i));

  // DoG rows yy-2, yy-1, yy live in three register sets whose roles rotate; the row loop is unrolled by
  // three so the rotation costs no moves.
  f4 DA[kNumDog], DB[kNumDog], DC[kNumDog];
#pragma unroll
  for (int p = 0; p < kNumDog; ++p) DA[p] = DB[p] = DC[p] = f4{0.f, 0.f, 0.f, 0.f};

  // kDown: the horizontally filtered source rows 2r-1, 2r, 2r+1 of the next output row r slide through three register
  // pairs, two rows per EVEN row step (scale_down_fast_kernel's scheme).  The first even step of the chunk is ya-1 or ya:
  // its three rows are in the window already.
  f2 hm1 = f2{0.f, 0.f}, h0 = hm1, hp1 = hm1;
  int voff_down = kOobOffset;
  if (kDown) {
    const bool odd0 = ((ya - 1) & 1) != 0;  // wave-uniform
    hm1 = down_hrow(odd0 ? win[4] : win[3], DT.k[0], DT.k[1], DT.k[2]);
    h0 = down_hrow(odd0 ? win[5] : win[4], DT.k[0], DT.k[1], DT.k[2]);
    hp1 = down_hrow(odd0 ? win[6] : win[5], DT.k[0], DT.k[1], DT.k[2]);
    // output columns c0/2, c0/2+1; columns >= w/2 are dropped by num_records = (w/2)*4, per component
    voff_down = (lane_valid && c0 >= 0) ? (c0 >> 1) * 4 : kOobOffset;
  }

  f4 ahead = load_raw(ya - 1 + 5);  // row yy+5 of the first iteration; the loop keeps two rows in flight
  auto row_step = [&](int yy, f4 (&D0)[kNumDog], f4 (&D1)[kNumDog], f4 (&D2)[kNumDog]) {
    const f4 nxt = ahead;        // requested one iteration ago (raw)
    ahead = load_raw(yy + 6);    // needed two iterations from now
    if (kDown) {
      const int yu = __builtin_amdgcn_readfirstlane(yy);
      if ((yu & 1) == 0) {  // wave-uniform: the window holds rows yu-4 .. yu+4, output row r = yu/2 reads yu-1 .. yu+3
        const f2 hp2 = down_hrow(win[6], DT.k[0], DT.k[1], DT.k[2]), hp3 = down_hrow(win[7], DT.k[0], DT.k[1], DT.k[2]);
        const f2 o = down_vcol(hm1, h0, hp1, hp2, hp3, DT.k[0], DT.k[1], DT.k[2]);
        const int r = yu >> 1;
        if (yu >= own_lo && yu < own_hi && r < (h >> 1)) {  // wave-uniform
          const __amdgpu_buffer_rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc(
              (void *)(down_img + (long)r * down_pitch), 0, (w >> 1) * 4, kBufFlags);
          __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u2, o), ro, voff_down, 0, 0);
        }
        hm1 = hp1;
        h0 = hp2;
        hp1 = hp3;
      }
    }
    blur_dog_row<kIdent0>(win, T, D2);

    if (yy >= ya + 1) {
      const int y = yy - 1;  // centre row: D0 = y-1, D1 = y, D2 = y+1
      // Threshold pre-test.  An extremum must have |v| > peakThresh at its centre; for natural images <1 % of the
      // pixels do, so for most wave-rows no lane holds a candidate centre at a given scale (and often at none).
      // measured 73-79 % of the octave-0 wave-rows (240 px x 5 scales) of the 1080p benchmark images hold no such
      // centre at all.  One wave-uniform test skips the whole neighbourhood analysis for them; skipping cannot
      // change the result, because a hit implies |v| > thr.  (Skipping per scale/plane as well was tried: the
      // conditionally live min/max arrays cost 258 VGPRs -> 1 wave per SIMD, slower.)
      // (one running maximum of |v| -- ten v_max3_f32 with |.| modifiers and one compare instead of twenty compares;
      // a NaN never raises the maximum, just as it never passed `|v| > thr`)
      float vmax = 0.0f;
#pragma unroll
      for (int s = 0; s < kNumScales; ++s) {
        const f4 v = D1[s + 1];
        vmax = max3f(vmax, fabsf(v.x), fabsf(v.y));
        vmax = max3f(vmax, fabsf(v.z), fabsf(v.w));
      }
      // halo lanes and lanes right of the image hold no centres (and their DoG values are not meaningful)
      // (folding the lane gate into a per-lane threshold register -- one compare, no mask to reload -- was measured:
      // +0.9 % on four streams, round 5; the kernel has no register to spare for it)
      const bool big = vmax > P.thr_pos && lane_valid && c0 < w;
      unsigned int cand = 0;  // bit (4*s + j)
      if (__builtin_amdgcn_ballot_w64(big) != 0) {  // wave-uniform
        // per plane: 3-row column min/max, then the 3x3 min/max (h*) and the left/right neighbours' columns
        f4 hmn[kNumDog], hmx[kNumDog];
        f4 lmn[kNumScales], rmn[kNumScales], lmx[kNumScales], rmx[kNumScales];  // for the 5 centre planes 1..5
#pragma unroll
        for (int p = 0; p < kNumDog; ++p) {
          f4 cmn, cmx, l_mn, r_mn, l_mx, r_mx;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            cmn[j] = min3f(D0[p][j], D1[p][j], D2[p][j]);
            cmx[j] = max3f(D0[p][j], D1[p][j], D2[p][j]);
          }
          l_mn = f4{from_prev_lane(cmn[3]), cmn[0], cmn[1], cmn[2]};
          r_mn = f4{cmn[1], cmn[2], cmn[3], from_next_lane(cmn[0])};
          l_mx = f4{from_prev_lane(cmx[3]), cmx[0], cmx[1], cmx[2]};
          r_mx = f4{cmx[1], cmx[2], cmx[3], from_next_lane(cmx[0])};
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            hmn[p][j] = min3f(l_mn[j], cmn[j], r_mn[j]);
            hmx[p][j] = max3f(l_mx[j], cmx[j], r_mx[j]);
          }
          if (p >= 1 && p <= kNumScales) {
            lmn[p - 1] = l_mn;
            rmn[p - 1] = r_mn;
            lmx[p - 1] = l_mx;
            rmx[p - 1] = r_mx;
          }
        }
#pragma unroll
        for (int s = 0; s < kNumScales; ++s) {
          const int c = s + 1;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const float v = D1[c][j];
            // v < thr_neg && v < every neighbour  <=>  v < min(thr_neg, neighbours): three 3-input trees, one compare
            const float mn_a = min3f(lmn[s][j], rmn[s][j], D0[c][j]);
            const float mn_b = min3f(D2[c][j], hmn[c - 1][j], hmn[c + 1][j]);
            const float mx_a = max3f(lmx[s][j], rmx[s][j], D0[c][j]);
            const float mx_b = max3f(D2[c][j], hmx[c - 1][j], hmx[c + 1][j]);
            const bool hit = (v < min3f(mn_a, mn_b, P.thr_neg)) || (v > max3f(mx_a, mx_b, P.thr_pos));
            cand |= (hit ? 1u : 0u) << (4 * s + j);
          }
        }
      }
      if (!lane_valid) cand = 0;
      // border pixels are never extrema in the reference (clamped neighbour == centre)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (c0 + j < 1 || c0 + j > w - 2) cand &= ~(0x11111u << j);
      if (__builtin_expect_with_probability(__builtin_amdgcn_ballot_w64(cand != 0) != 0, 0, 1.0)) {  // wave-uniform, rare
        // A candidate's refinement reads 19 DoG values: the 3x3 of its own plane, and the centre with its four
        // neighbours in the planes below and above.  All of them are in the registers of the detecting lane, except
        // the column beyond its float4 (from the lane before for column 0, the lane after for column 3: five DPP
        // moves).  The scale index and the column are made compile-time constants -- one case per (scale, column) --
        // so every value is a named register and the lane stores its entry directly.  (Round 2 first dumped the three
        // planes of the strip into an LDS cube, 9 KB per wave, and copied from there: ~1,750 cycles per
        // row-and-scale with a candidate by the phase stamps.)
        // The cases only PUSH; the check-and-refine behind the switch is the row step's one copy of refine_batch
        // (inside each of the 20 cases it was inlined 60 times per chunk body, ~95 KB of a 112 KB kernel).
        auto push = [&](auto scale_c, auto col_c, float *e) {
          constexpr int k = decltype(scale_c)::value;  // planes k (below), k + 1 (the candidate's), k + 2 (above)
          constexpr int j = decltype(col_c)::value;
          // value of plane p, row set D, column j + dx
          auto at = [&](const f4 (&D)[kNumDog], int p, int dx) -> float {
            const int col = j + dx;
            if (col < 0) return from_prev_lane(D[p][3]);
            if (col > 3) return from_next_lane(D[p][0]);
            return D[p][col];
          };
          // all lanes take part in the DPP moves and in the stores: `e` of a lane without a candidate is its spare words
          const float c00 = at(D0, k + 1, -1), c01 = at(D0, k + 1, 0), c02 = at(D0, k + 1, 1);
          const float c10 = at(D1, k + 1, -1), c11 = at(D1, k + 1, 0), c12 = at(D1, k + 1, 1);
          const float c20 = at(D2, k + 1, -1), c21 = at(D2, k + 1, 0), c22 = at(D2, k + 1, 1);
          const float l0 = at(D1, k, 0), l1 = at(D1, k, -1), l2 = at(D1, k, 1), l3 = at(D0, k, 0), l4 = at(D2, k, 0);
          const float h0 = at(D1, k + 2, 0), h1 = at(D1, k + 2, -1), h2 = at(D1, k + 2, 1), h3 = at(D0, k + 2, 0),
                      h4 = at(D2, k + 2, 0);
          e[0] = c00, e[1] = c01, e[2] = c02, e[3] = c10, e[4] = c11, e[5] = c12, e[6] = c20, e[7] = c21, e[8] = c22;
          e[9] = l0, e[10] = l1, e[11] = l2, e[12] = l3, e[13] = l4;
          e[14] = h0, e[15] = h1, e[16] = h2, e[17] = h3, e[18] = h4;
        };
#define CUSIFT_PUSH_CASE(S, J) \
  case 4 * S + J: push(std::integral_constant<int, S>{}, std::integral_constant<int, J>{}, e); break;
#define CUSIFT_PUSH_SCALE(S) CUSIFT_PUSH_CASE(S, 0) CUSIFT_PUSH_CASE(S, 1) CUSIFT_PUSH_CASE(S, 2) CUSIFT_PUSH_CASE(S, 3)
        // the 20 (scale, column) items of the row, scale ascending, then column ascending: bit 4*s + j of `cand`
        // (one OR over the wave instead of a ballot per item: the loop below visits the non-empty items only)
        unsigned int items = wave_or(cand);
        while (items != 0) {
          const int it = __builtin_ctz(items);
          items &= items - 1;
          const bool mine = (cand >> it) & 1u;
          float *e = cands.reserve(mine, lane);  // at most kDetCandLanes more entries
          e[19] = __builtin_bit_cast(float, c0 + (it & 3));
          e[20] = __builtin_bit_cast(float, ((y + rw.row0) << 3) | (it >> 2));
          switch (it) {
            CUSIFT_PUSH_SCALE(0)
            CUSIFT_PUSH_SCALE(1)
            CUSIFT_PUSH_SCALE(2)
            CUSIFT_PUSH_SCALE(3)
            default: CUSIFT_PUSH_SCALE(4)
          }
          // fewer than 64 were waiting and one item pushes at most 64: never more than kCandCap entries
          if (cands.n >= 64) {
            cands.refine_batch<kRecBytes>(list, max_pts, counter, P, lane);
          }
        }
#undef CUSIFT_PUSH_SCALE
#undef CUSIFT_PUSH_CASE
      }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) win[i] = win[i + 1];
    win[8] = fix(nxt);
  };

  for (int yy = ya - 1; yy <= yb; yy += 3) {
    row_step(yy, DA, DB, DC);
    if (yy + 1 > yb) break;
    row_step(yy + 1, DB, DC, DA);
    if (yy + 2 > yb) break;
    row_step(yy + 2, DC, DA, DB);
  }
  cands.refine_batch<kRecBytes>(list, max_pts, counter, P, lane);  // what is left of the chunk's candidates (fewer than 64)
