// sift_tracks.hip -- feature tracks of a whole sequence on the device (cusift_build_tracks) and their triangulation from
// all views (cusift_triangulate_tracks).  New functionality: the reference stops at one model per frame pair.  The
// contract is include/cusift_amd_extras.h's; tests/tracks_model.py restates it in numpy and the tests demand its bytes.
//
// A NODE is a record of the batch, v = frame * max_pts + record; an EDGE is an accepted row of cusift_match_batch; a
// TRACK is a connected component with at least min_views nodes and no two of them in one frame, numbered in ascending
// order of its smallest node.  Ten enqueued operations, whatever the rows hold and however many pairs there are:
//
//   hipMemsetAsync           the per-frame hash sets, all slots free
//   tracks_init_kernel       parent[v] = v; sizes, shared-frame flags, cursors and d_stats zero
//   tracks_link_kernel       one thread per row (pair, record): a lock-free union-find over parent[].  find() walks
//                            parent[] down to a root; two roots are joined by a compare-and-swap that hooks the LARGER
//                            under the smaller, so parent[v] <= v always holds, every walk descends strictly and ends,
//                            and the last root of a component is its smallest node whatever order the hooks land in.  A
//                            failed compare-and-swap (someone else hooked that root first) finds again and retries; no
//                            thread waits for another.  Every access to parent[] in this launch is an agent-scope atomic:
//                            the XCDs' L2s are private, and a plain load may return a line that another XCD has long
//                            rewritten.
//   tracks_flatten_kernel    root[v] of every live node into an array of its own (plain loads: the kernel boundary made
//                            the links visible), -1 for a dead slot; size[root] += 1
//   tracks_shared_kernel     components of 2 .. n_images nodes (a larger one shares a frame by pigeonhole): every node
//                            puts its root into its FRAME's open-addressing hash set; finding it there already means two
//                            records of that frame in one component: shared[root] = 1.  Which of the two finds it varies,
//                            the flag does not.
//   tracks_sums_kernel       per 256 nodes: kept roots and their sizes; the two drop counts into d_stats
//   tracks_scan_kernel       ONE workgroup: exclusive scan of the block sums in block order; T, the observation count
//   tracks_assign_kernel     track number of a kept root = block base + its rank in the block (ballot + mbcnt),
//                            d_offsets[t] = block base + the sizes in front: ascending node order, no append atomics
//   tracks_label_kernel      d_track[v]; the members of every track behind its offset in arrival order (integer cursor)
//   tracks_order_kernel      a wave per track ranks its short list by node -> d_obs in ascending node order
//
// Integer arithmetic only, and every value that reaches an output is independent of the order of arrival: the same input
// gives the same bytes.
#include <cmath>

#include "sift_host.h"
#include "sift_ransac.h"

namespace cusift {

constexpr int kTrackThreads = 256;  // == kRansacThreads: keep_count_256, keep_rank_256, block_sum_256
static_assert(kTrackThreads == kRansacThreads, "the *_256 helpers of sift_ransac.h");
constexpr int kTrackFree = -1;  // a free slot of a hash set (the memset's 0xFF bytes)

// parent[] while tracks_link_kernel runs: agent scope, relaxed -- the words carry no other data with them
__device__ __forceinline__ int uf_load(int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int uf_find(int *parent, int v) {
  int p = uf_load(parent + v);
  while (p != v) {  // parent[v] <= v: strictly descending
    v = p;
    p = uf_load(parent + v);
  }
  return v;
}
__device__ __forceinline__ void uf_union(int *parent, int a, int b) {
  while (true) {
    a = uf_find(parent, a);
    b = uf_find(parent, b);
    if (a == b) return;
    const int hi = a > b ? a : b, lo = a > b ? b : a;
    int expected = hi;  // still a root: hook it under the smaller one
    if (__hip_atomic_compare_exchange_strong(parent + hi, &expected, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_AGENT))
      return;
    // someone hooked `hi` first: it has a smaller parent now, the next find starts from there
  }
}

__global__ void __launch_bounds__(kTrackThreads) tracks_init_kernel(int n, int *__restrict__ parent, int *__restrict__ size,
                                                                     int *__restrict__ shared, int *__restrict__ cursor,
                                                                     unsigned int *__restrict__ stats) {
  const long v = (long)blockIdx.x * kTrackThreads + threadIdx.x;
  if (v < 8) stats[v] = 0u;
  if (v >= n) return;
  parent[v] = (int)v;
  size[v] = 0;
  shared[v] = 0;
  cursor[v] = 0;
}

// n_pairs == 0 or max_pts == 0: no edge, no track
__global__ void __launch_bounds__(kTrackThreads) tracks_empty_kernel(int n, int *__restrict__ track,
                                                                      int *__restrict__ offsets,
                                                                      unsigned int *__restrict__ stats) {
  const long v = (long)blockIdx.x * kTrackThreads + threadIdx.x;
  if (v < 8) stats[v] = 0u;
  if (v == 0) offsets[0] = 0;
  if (v < n) track[v] = -1;
}

// grid (record block, pair)
__global__ void __launch_bounds__(kTrackThreads) tracks_link_kernel(
    const unsigned int *__restrict__ counters, int max_pts, const int *__restrict__ pairs,
    const cusift_match_row *__restrict__ rows, const cusift_match_row *__restrict__ rows_back,
    const unsigned char *__restrict__ keep, int rule, float lo, float hi, int *parent, unsigned int *__restrict__ stats) {
  __shared__ int s_wave[kTrackThreads / 64];
  const int p = blockIdx.y, i = blockIdx.x * kTrackThreads + threadIdx.x;
  const int a = pairs[2 * p], b = pairs[2 * p + 1];
  const int na = frame_count(counters, a, max_pts), nb = frame_count(counters, b, max_pts);
  bool edge = false;
  int m = -1;
  // nb == 0: the matcher wrote no row of this pair; rows past na are never read
  if (a != b && nb > 0 && i < na) {
    const size_t at = (size_t)p * max_pts + i;
    const f4 row = *reinterpret_cast<const f4 *>(rows + at);  // score, ambiguity, match, reserved
    m = __float_as_int(row[2]);
    edge = m >= 0 && m < nb && (rule == 0 ? (row[0] > lo && row[1] < hi) : (row[0] < lo && row[1] < hi));
    if (edge && keep) edge = keep[at] != 0;
    // the cross-check: back row m was written (na > 0, m < nb) and must name record i
    if (edge && rows_back) edge = rows_back[(size_t)p * max_pts + m].match == i;
  }
  if (edge) uf_union(parent, a * max_pts + i, b * max_pts + m);
  const int accepted = keep_count_256(edge, s_wave);
  if (threadIdx.x == 0 && accepted) atomicAdd(stats + 2, (unsigned int)accepted);
}

__global__ void __launch_bounds__(kTrackThreads) tracks_flatten_kernel(const unsigned int *__restrict__ counters,
                                                                        int max_pts, int n,
                                                                        const int *__restrict__ parent,
                                                                        int *__restrict__ root, int *__restrict__ size) {
  const long v = (long)blockIdx.x * kTrackThreads + threadIdx.x;
  if (v >= n) return;
  const int f = (int)(v / max_pts), i = (int)(v - (long)f * max_pts);
  int r = -1;
  if (i < frame_count(counters, f, max_pts)) {
    r = (int)v;
    for (int q = parent[r]; q != r; q = parent[r]) r = q;
    atomicAdd(size + r, 1);
  }
  root[v] = r;
}

// table[frame][slots], slots = 2^log_slots >= 2 max_pts: never more than half full
__global__ void __launch_bounds__(kTrackThreads) tracks_shared_kernel(int max_pts, int n, int n_images,
                                                                       const int *__restrict__ root,
                                                                       const int *__restrict__ size, int log_slots,
                                                                       int *table, int *__restrict__ shared) {
  const long v = (long)blockIdx.x * kTrackThreads + threadIdx.x;
  if (v >= n) return;
  const int r = root[v];
  if (r < 0) return;
  const int sz = size[r];
  if (sz < 2 || sz > n_images) return;
  int *set = table + ((size_t)(v / max_pts) << log_slots);
  const unsigned int mask = (1u << log_slots) - 1u;
  unsigned int h = ((unsigned int)r * 2654435761u) >> (32 - log_slots);
  while (true) {
    int seen = kTrackFree;
    if (__hip_atomic_compare_exchange_strong(set + h, &seen, r, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_AGENT))
      return;  // the first of this component in this frame
    if (seen == r) {
      shared[r] = 1;
      return;
    }
    h = (h + 1u) & mask;
  }
}

// what becomes of the component whose root is v (sz = size[v]: 0 unless v is a live root)
__device__ __forceinline__ bool track_kept(int sz, int is_shared, int n_images, int min_views, bool &drop_shared,
                                           bool &drop_short) {
  const bool two = sz >= 2, sh = two && (sz > n_images || is_shared != 0);
  drop_shared = sh;
  drop_short = two && !sh && sz < min_views;
  return two && !sh && sz >= min_views;
}

__global__ void __launch_bounds__(kTrackThreads) tracks_sums_kernel(int n, int n_images, int min_views,
                                                                     const int *__restrict__ size,
                                                                     const int *__restrict__ shared,
                                                                     int2 *__restrict__ block_sums,
                                                                     unsigned int *__restrict__ stats) {
  __shared__ int s_red[kTrackThreads];
  __shared__ int s_wave[kTrackThreads / 64];
  const long v = (long)blockIdx.x * kTrackThreads + threadIdx.x;
  const int sz = v < n ? size[v] : 0;
  bool drop_shared, drop_short;
  const bool kept = track_kept(sz, v < n ? shared[v] : 0, n_images, min_views, drop_shared, drop_short);
  const int n_kept = keep_count_256(kept, s_wave);
  __syncthreads();
  const int n_shared = keep_count_256(drop_shared, s_wave);
  __syncthreads();
  const int n_short = keep_count_256(drop_short, s_wave);
  const int n_obs = block_sum_256(kept ? sz : 0, s_red);
  if (threadIdx.x == 0) {
    block_sums[blockIdx.x] = make_int2(n_kept, n_obs);
    if (n_shared) atomicAdd(stats + 3, (unsigned int)n_shared);
    if (n_short) atomicAdd(stats + 4, (unsigned int)n_short);
  }
}

// Exclusive scan of one int per thread over the workgroup in thread order, and the total.  s_wave [4]; a barrier stands
// in front of its reuse.
__device__ __forceinline__ int excl_scan_256(int v, int *s_wave, int &total) {
  const int tx = threadIdx.x, lane = tx & 63;
  int inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int other = __shfl_up(inc, d);
    if (lane >= d) inc += other;
  }
  __syncthreads();
  if (lane == 63) s_wave[tx >> 6] = inc;
  __syncthreads();
  int base = 0;
#pragma unroll
  for (int wv = 0; wv < kTrackThreads / 64; ++wv) base += wv < (tx >> 6) ? s_wave[wv] : 0;
  total = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
  return base + inc - v;
}

// one workgroup: block_sums -> exclusive bases in place, block order
__global__ void __launch_bounds__(kTrackThreads) tracks_scan_kernel(int n_blocks, int2 *__restrict__ block_sums,
                                                                     int *__restrict__ offsets,
                                                                     unsigned int *__restrict__ stats) {
  __shared__ int s_wave[kTrackThreads / 64];
  int base_t = 0, base_o = 0;
  for (int chunk = 0; chunk < n_blocks; chunk += kTrackThreads) {
    const int b = chunk + threadIdx.x;
    const int2 s = b < n_blocks ? block_sums[b] : make_int2(0, 0);
    int total_t, total_o;
    const int t = excl_scan_256(s.x, s_wave, total_t);
    const int o = excl_scan_256(s.y, s_wave, total_o);
    if (b < n_blocks) block_sums[b] = make_int2(base_t + t, base_o + o);
    base_t += total_t;
    base_o += total_o;
  }
  if (threadIdx.x == 0) {
    stats[0] = (unsigned int)base_t;
    stats[1] = (unsigned int)base_o;
    offsets[base_t] = base_o;
  }
}

__global__ void __launch_bounds__(kTrackThreads) tracks_assign_kernel(int n, int n_images, int min_views,
                                                                       const int *__restrict__ size,
                                                                       const int *__restrict__ shared,
                                                                       const int2 *__restrict__ block_base,
                                                                       int *__restrict__ track_of_root,
                                                                       int *__restrict__ offsets) {
  __shared__ int s_wave[kTrackThreads / 64];
  const long v = (long)blockIdx.x * kTrackThreads + threadIdx.x;
  const int sz = v < n ? size[v] : 0;
  bool drop_shared, drop_short;
  const bool kept = track_kept(sz, v < n ? shared[v] : 0, n_images, min_views, drop_shared, drop_short);
  int total;
  const int rank = keep_rank_256(kept, s_wave, total);
  const int front = excl_scan_256(kept ? sz : 0, s_wave, total);  // (its leading barrier frees s_wave)
  const int2 base = block_base[blockIdx.x];
  if (v < n) track_of_root[v] = kept ? base.x + rank : -1;
  if (kept) offsets[base.x + rank] = base.y + front;
}

__global__ void __launch_bounds__(kTrackThreads) tracks_label_kernel(int n, const int *__restrict__ root,
                                                                      const int *__restrict__ track_of_root,
                                                                      const int *__restrict__ offsets,
                                                                      int *__restrict__ cursor, int *__restrict__ track,
                                                                      int *__restrict__ members) {
  const long v = (long)blockIdx.x * kTrackThreads + threadIdx.x;
  if (v >= n) return;
  const int r = root[v];
  const int t = r >= 0 ? track_of_root[r] : -1;
  track[v] = t;
  if (t >= 0) members[offsets[t] + atomicAdd(cursor + r, 1)] = (int)v;
}

// a wave per track, as many tracks per wave as it takes: member e goes to the place its node has among the members
__global__ void __launch_bounds__(kTrackThreads) tracks_order_kernel(const unsigned int *__restrict__ stats,
                                                                      const int *__restrict__ offsets,
                                                                      const int *__restrict__ members,
                                                                      int *__restrict__ obs) {
  const int lane = threadIdx.x & 63;
  const long n_waves = (long)gridDim.x * (kTrackThreads / 64);
  const long n_tracks = (long)stats[0];
  for (long t = (long)blockIdx.x * (kTrackThreads / 64) + (threadIdx.x >> 6); t < n_tracks; t += n_waves) {
    const int first = offsets[t], len = offsets[t + 1] - first;
    for (int e = lane; e < len; e += 64) {
      const int v = members[first + e];
      int rank = 0;
      for (int j = 0; j < len; ++j) rank += members[first + j] < v ? 1 : 0;
      obs[first + rank] = v;
    }
  }
}

// ------------------------------------------------------------------------------------------------
// triangulation: one thread per track, all fp64, every expression in the header's order
// ------------------------------------------------------------------------------------------------
struct TrackCam {
  double fx, fy, px, py;
};

__global__ void __launch_bounds__(kTrackThreads) tracks_triangulate_kernel(
    const cusift_point *__restrict__ points, int max_pts, const int *__restrict__ offsets, const int *__restrict__ obs,
    const unsigned int *__restrict__ stats, int max_tracks, const double *__restrict__ poses, TrackCam cam,
    double min_pivot, double *__restrict__ points3d, int *__restrict__ front) {
  const long t = (long)blockIdx.x * kTrackThreads + threadIdx.x;
  const long n_tracks = min((long)stats[0], (long)max_tracks);
  if (t >= n_tracks) return;
  const int first = offsets[t], last = offsets[t + 1];
  double A00 = 0.0, A10 = 0.0, A11 = 0.0, A20 = 0.0, A21 = 0.0, A22 = 0.0, g0 = 0.0, g1 = 0.0, g2 = 0.0;
  for (int e = first; e < last; ++e) {
    const int v = obs[e];
    const double *P = poses + 12 * (size_t)(v / max_pts);
    const double x = (double)points[v].coords2D[0], y = (double)points[v].coords2D[1];
    const double d0 = (x - cam.px) / cam.fx, d1 = (y - cam.py) / cam.fy;
    const double w0 = (P[0] * d0 + P[1] * d1) + P[2];
    const double w1 = (P[4] * d0 + P[5] * d1) + P[6];
    const double w2 = (P[8] * d0 + P[9] * d1) + P[10];
    const double n = (w0 * w0 + w1 * w1) + w2 * w2;
    const double t0 = P[3], t1 = P[7], t2 = P[11];
    const double M00 = 1.0 - (w0 * w0) / n, M11 = 1.0 - (w1 * w1) / n, M22 = 1.0 - (w2 * w2) / n;
    const double M01 = 0.0 - (w0 * w1) / n, M02 = 0.0 - (w0 * w2) / n, M12 = 0.0 - (w1 * w2) / n;
    const double M10 = 0.0 - (w1 * w0) / n, M20 = 0.0 - (w2 * w0) / n, M21 = 0.0 - (w2 * w1) / n;
    A00 += M00, A10 += M10, A11 += M11, A20 += M20, A21 += M21, A22 += M22;
    g0 += (M00 * t0 + M01 * t1) + M02 * t2;
    g1 += (M10 * t0 + M11 * t1) + M12 * t2;
    g2 += (M20 * t0 + M21 * t1) + M22 * t2;
  }
  const double q00 = A00, l00 = sqrt(q00), l10 = A10 / l00, l20 = A20 / l00;
  const double q11 = A11 - l10 * l10, l11 = sqrt(q11), l21 = (A21 - l20 * l10) / l11;
  const double q22 = A22 - (l20 * l20 + l21 * l21), l22 = sqrt(q22);
  const double y0 = g0 / l00, y1 = (g1 - l10 * y0) / l11, y2 = (g2 - (l20 * y0 + l21 * y1)) / l22;
  const double X2 = y2 / l22, X1 = (y1 - l21 * X2) / l11, X0 = (y0 - (l10 * X1 + l20 * X2)) / l00;
  const double inf = __builtin_inf();
  const bool good = q00 > min_pivot && q11 > min_pivot && q22 > min_pivot && fabs(X0) < inf && fabs(X1) < inf &&
                    fabs(X2) < inf;
  double worst = 0.0;
  int in_front = 0;
  for (int e = first; good && e < last; ++e) {
    const int v = obs[e];
    const double *P = poses + 12 * (size_t)(v / max_pts);
    const double x = (double)points[v].coords2D[0], y = (double)points[v].coords2D[1];
    const double e0 = X0 - P[3], e1 = X1 - P[7], e2 = X2 - P[11];
    const double c0 = (P[0] * e0 + P[4] * e1) + P[8] * e2;
    const double c1 = (P[1] * e0 + P[5] * e1) + P[9] * e2;
    const double c2 = (P[2] * e0 + P[6] * e1) + P[10] * e2;
    in_front += c2 > 0.0 ? 1 : 0;
    const double u = cam.fx * (c0 / c2) + cam.px, w = cam.fy * (c1 / c2) + cam.py;
    const double err2 = (u - x) * (u - x) + (w - y) * (w - y);
    worst = err2 > worst ? err2 : worst;
  }
  double *out = points3d + 4 * (size_t)t;
  out[0] = good ? X0 : 0.0;
  out[1] = good ? X1 : 0.0;
  out[2] = good ? X2 : 0.0;
  out[3] = good ? sqrt(worst) : 0.0;
  front[t] = good ? in_front : 0;
}

}  // namespace cusift

// ------------------------------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------------------------------
static int tracks_shape(const char *who, int n_images, int max_pts) {
  if ((long long)n_images * max_pts > 0x7fffffffLL)
    return fail(CUSIFT_ERR_INVALID, "%s: %d frames x %d records are more than 2^31 - 1 nodes", who, n_images, max_pts);
  return CUSIFT_OK;
}

extern "C" int cusift_build_tracks(cusift_ctx *ctx, const unsigned int *d_counters, int n_images, int max_pts,
                                   const int *h_pairs, int n_pairs, const cusift_match_row *d_rows,
                                   const cusift_match_row *d_rows_back, const unsigned char *d_keep, int rule, float lo,
                                   float hi, int min_views, int *d_track, int *d_offsets, int *d_obs,
                                   unsigned int *d_stats) {
  TRY(enter(ctx));
  TRY(check_pair_list(h_pairs, n_pairs, n_images, max_pts, "BuildTracks"));
  TRY(tracks_shape("BuildTracks", n_images, max_pts));
  if (n_pairs > 0 && !d_rows) return fail(CUSIFT_ERR_INVALID, "BuildTracks: NULL d_rows");
  if (!d_track || !d_offsets || !d_obs || !d_stats) return fail(CUSIFT_ERR_INVALID, "BuildTracks: NULL output");
  if (rule != 0 && rule != 1)
    return fail(CUSIFT_ERR_INVALID, "BuildTracks: rule must be 0 (score > lo) or 1 (score < lo^2)");
  if (lo != lo || hi != hi) return fail(CUSIFT_ERR_INVALID, "BuildTracks: lo / hi is NaN");
  if (min_views < 2) return fail(CUSIFT_ERR_INVALID, "BuildTracks: min_views %d, a track has at least 2 views", min_views);
  if (d_rows_back && d_rows_back == d_rows)
    return fail(CUSIFT_ERR_INVALID, "BuildTracks: d_rows_back is d_rows (it is the column side, or NULL)");
  const int n = n_images * max_pts;
  const int n_blocks = std::max(1, idiv_up(n, kTrackThreads));
  if (n_pairs == 0 || max_pts == 0) {
    hipLaunchKernelGGL(tracks_empty_kernel, dim3(n_blocks), dim3(kTrackThreads), 0, ctx->stream, n, d_track, d_offsets,
                       d_stats);
    return check_launch("tracks_empty");
  }

  // scratch: [pair list | parent | root | size | shared | track of root | cursor | members | block sums | hash sets]
  int log_slots = 1;
  while ((1ll << log_slots) < 2ll * max_pts) ++log_slots;
  ScratchLayout L;
  const size_t words = sizeof(int) * (size_t)n;
  const size_t pairs_at = L.take(sizeof(int) * 2 * (size_t)n_pairs);
  const size_t parent_at = L.take(words), root_at = L.take(words), size_at = L.take(words), shared_at = L.take(words);
  const size_t ids_at = L.take(words), cursor_at = L.take(words), members_at = L.take(words);
  const size_t sums_at = L.take(sizeof(int2) * (size_t)n_blocks);
  const size_t table_b = sizeof(int) * ((size_t)n_images << log_slots);
  const size_t table_at = L.take(table_b);
  TRY(grow_scratch(ctx, ctx->tracks_scratch, ctx->tracks_scratch_bytes, L.size, "BuildTracks: ", false));
  char *s = ctx->tracks_scratch;
  int *d_pairs = at<int>(s, pairs_at), *parent = at<int>(s, parent_at), *root = at<int>(s, root_at);
  int *size = at<int>(s, size_at), *shared = at<int>(s, shared_at), *ids = at<int>(s, ids_at);
  int *cursor = at<int>(s, cursor_at), *members = at<int>(s, members_at), *table = at<int>(s, table_at);
  int2 *sums = at<int2>(s, sums_at);

  const dim3 nodes(n_blocks), block(kTrackThreads);
  HIP_TRY(hipMemcpyAsync(d_pairs, h_pairs, sizeof(int) * 2 * (size_t)n_pairs, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(hipMemsetAsync(table, 0xFF, table_b, ctx->stream));
  hipLaunchKernelGGL(tracks_init_kernel, nodes, block, 0, ctx->stream, n, parent, size, shared, cursor, d_stats);
  hipLaunchKernelGGL(tracks_link_kernel, dim3(idiv_up(max_pts, kTrackThreads), n_pairs), block, 0, ctx->stream,
                     d_counters, max_pts, (const int *)d_pairs, d_rows, d_rows_back, d_keep, rule,
                     rule == 1 ? lo * lo : lo, rule == 1 ? hi * hi : hi, parent, d_stats);
  hipLaunchKernelGGL(tracks_flatten_kernel, nodes, block, 0, ctx->stream, d_counters, max_pts, n, (const int *)parent,
                     root, size);
  hipLaunchKernelGGL(tracks_shared_kernel, nodes, block, 0, ctx->stream, max_pts, n, n_images, (const int *)root,
                     (const int *)size, log_slots, table, shared);
  hipLaunchKernelGGL(tracks_sums_kernel, nodes, block, 0, ctx->stream, n, n_images, min_views, (const int *)size,
                     (const int *)shared, sums, d_stats);
  hipLaunchKernelGGL(tracks_scan_kernel, dim3(1), block, 0, ctx->stream, n_blocks, sums, d_offsets, d_stats);
  hipLaunchKernelGGL(tracks_assign_kernel, nodes, block, 0, ctx->stream, n, n_images, min_views, (const int *)size,
                     (const int *)shared, (const int2 *)sums, ids, d_offsets);
  hipLaunchKernelGGL(tracks_label_kernel, nodes, block, 0, ctx->stream, n, (const int *)root, (const int *)ids,
                     (const int *)d_offsets, cursor, d_track, members);
  // at most n / 2 tracks, four to a workgroup; beyond 4096 workgroups the waves take several tracks each
  const int order_blocks = std::max(1, std::min(4096, idiv_up(n / 2, kTrackThreads / 64)));
  hipLaunchKernelGGL(tracks_order_kernel, dim3(order_blocks), block, 0, ctx->stream, (const unsigned int *)d_stats,
                     (const int *)d_offsets, (const int *)members, d_obs);
  return check_launch("build_tracks");
}

extern "C" int cusift_triangulate_tracks(cusift_ctx *ctx, const cusift_point *d_points, int n_images, int max_pts,
                                         const int *d_offsets, const int *d_obs, const unsigned int *d_stats,
                                         int max_tracks, const double *h_poses, const cusift_camera *camera,
                                         double min_pivot, double *d_points3d, int *d_front) {
  TRY(enter(ctx));
  TRY(check_pair_list(nullptr, 0, n_images, max_pts, "TriangulateTracks"));
  TRY(tracks_shape("TriangulateTracks", n_images, max_pts));
  if (!d_points || !d_offsets || !d_obs || !d_stats || !h_poses || !camera || !d_points3d || !d_front)
    return fail(CUSIFT_ERR_INVALID, "TriangulateTracks: NULL pointer");
  if (max_tracks < 0) return fail(CUSIFT_ERR_INVALID, "TriangulateTracks: max_tracks %d is negative", max_tracks);
  if (!(min_pivot >= 0.0)) return fail(CUSIFT_ERR_INVALID, "TriangulateTracks: min_pivot is negative or NaN");
  if (!std::isfinite(camera->fx) || !std::isfinite(camera->fy) || camera->fx == 0.0f || camera->fy == 0.0f ||
      !std::isfinite(camera->cx) || !std::isfinite(camera->cy) || !std::isfinite(camera->origin))
    return fail(CUSIFT_ERR_INVALID, "TriangulateTracks: fx, fy must be finite and not 0, cx, cy, origin finite");
  for (size_t k = 0; k < 12 * (size_t)n_images; ++k)
    if (!std::isfinite(h_poses[k]))
      return fail(CUSIFT_ERR_INVALID, "TriangulateTracks: pose %zu has an entry that is not finite", k / 12);
  if (max_tracks == 0 || n_images == 0 || max_pts == 0) return CUSIFT_OK;
  const size_t poses_b = sizeof(double) * 12 * (size_t)n_images;
  TRY(grow_scratch(ctx, ctx->tracks_scratch, ctx->tracks_scratch_bytes, poses_b, "TriangulateTracks: ", false));
  double *d_poses = reinterpret_cast<double *>(ctx->tracks_scratch);
  HIP_TRY(hipMemcpyAsync(d_poses, h_poses, poses_b, hipMemcpyHostToDevice, ctx->stream));
  TrackCam cam;
  cam.fx = (double)camera->fx, cam.fy = (double)camera->fy;
  cam.px = (double)camera->cx - (double)camera->origin, cam.py = (double)camera->cy - (double)camera->origin;
  hipLaunchKernelGGL(tracks_triangulate_kernel, dim3(idiv_up(max_tracks, kTrackThreads)), dim3(kTrackThreads), 0,
                     ctx->stream, d_points, max_pts, d_offsets, d_obs, d_stats, max_tracks, (const double *)d_poses, cam,
                     min_pivot, d_points3d, d_front);
  return check_launch("triangulate_tracks");
}
