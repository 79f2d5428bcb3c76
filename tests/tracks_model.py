"""cusift_build_tracks and cusift_triangulate_tracks restated in numpy and plain Python: the definition of
include/cusift_amd_extras.h, which the device has to equal -- exactly for the tracks, to fp64 rounding for the points."""
import numpy as np

ROW = np.dtype([("score", "<f4"), ("ambiguity", "<f4"), ("match", "<i4"), ("reserved", "<i4")])


def build_tracks_model(counts, max_pts, pairs, rows, rows_back=None, keep=None, rule=1, lo=999.0, hi=0.8, min_views=2):
    """counts: the raw counter of every frame (clamped to max_pts here); rows / rows_back: ROW [P, max_pts]; keep:
    [P, max_pts].  Returns (track int32 [n, max_pts], offsets int32 [T + 1], obs int32, stats uint32 [8])."""
    n = len(counts)
    cnt = [min(int(c), max_pts) for c in counts]
    lo, hi = np.float32(lo), np.float32(hi)
    if rule == 1:
        lo, hi = np.float32(lo * lo), np.float32(hi * hi)
    lo, hi = float(lo), float(hi)
    parent = list(range(n * max_pts))

    def find(v):
        while parent[v] != v:
            v = parent[v]
        return v

    accepted = 0
    for p, (a, b) in enumerate(np.asarray(pairs).reshape(-1, 2).tolist()):
        if a == b or cnt[a] == 0 or cnt[b] == 0:
            continue
        # as Python lists: a float32 widens exactly, so the comparisons are the float32 ones
        score, ambiguity, match = (rows[p][f].tolist() for f in ("score", "ambiguity", "match"))
        back = None if rows_back is None else rows_back[p]["match"].tolist()
        for i in range(cnt[a]):
            s, amb, m = score[i], ambiguity[i], match[i]
            ok = 0 <= m < cnt[b] and (s > lo if rule == 0 else s < lo) and amb < hi
            ok = ok and (keep is None or keep[p, i] != 0)
            ok = ok and (back is None or back[m] == i)
            if ok:
                accepted += 1
                ra, rb = find(a * max_pts + i), find(b * max_pts + m)
                parent[max(ra, rb)] = min(ra, rb)
    members = {}
    for f in range(n):
        for i in range(cnt[f]):
            members.setdefault(find(f * max_pts + i), []).append(f * max_pts + i)
    track = np.full((n, max_pts), -1, dtype=np.int32)
    offsets, obs, stats = [0], [], np.zeros(8, dtype=np.uint32)
    for root in sorted(members):  # a root is its component's smallest node
        nodes = members[root]
        if len(nodes) < 2:
            continue
        frames = [v // max_pts for v in nodes]
        if len(set(frames)) < len(frames):
            stats[3] += 1
        elif len(nodes) < min_views:
            stats[4] += 1
        else:
            track.reshape(-1)[nodes] = len(offsets) - 1
            obs += sorted(nodes)
            offsets.append(len(obs))
    stats[0], stats[1], stats[2] = len(offsets) - 1, len(obs), accepted
    return track, np.asarray(offsets, dtype=np.int32), np.asarray(obs, dtype=np.int32), stats


def triangulate_model(xy, max_pts, offsets, obs, poses, fx, fy, cx, cy, origin=0.0, min_pivot=1e-12):
    """xy: float32 [n, max_pts, 2] (coords2D); poses: [n, 3, 4] camera to world; the camera's values as float32.  Returns
    (points3d float64 [T, 4], front int32 [T]): the header's expressions, in float64, in its order."""
    f64 = np.float64
    fx, fy = f64(np.float32(fx)), f64(np.float32(fy))
    px, py = f64(np.float32(cx)) - f64(np.float32(origin)), f64(np.float32(cy)) - f64(np.float32(origin))
    poses = np.asarray(poses, dtype=f64).reshape(-1, 3, 4)
    xy = np.asarray(xy, dtype=np.float32).reshape(-1, 2)
    n_tracks = len(offsets) - 1
    out, front = np.zeros((n_tracks, 4), dtype=f64), np.zeros(n_tracks, dtype=np.int32)
    with np.errstate(all="ignore"):
        for t in range(n_tracks):
            nodes = [int(v) for v in obs[offsets[t]:offsets[t + 1]]]
            A, g = np.zeros((3, 3), dtype=f64), np.zeros(3, dtype=f64)
            for v in nodes:
                R, tr = poses[v // max_pts, :, :3], poses[v // max_pts, :, 3]
                x, y = f64(xy[v, 0]), f64(xy[v, 1])
                d0, d1 = (x - px) / fx, (y - py) / fy
                w = [(R[i, 0] * d0 + R[i, 1] * d1) + R[i, 2] for i in range(3)]
                nn = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]
                M = [[f64(1.0 if i == j else 0.0) - (w[i] * w[j]) / nn for j in range(3)] for i in range(3)]
                for i in range(3):
                    for j in range(3):
                        A[i, j] += M[i][j]
                    g[i] += (M[i][0] * tr[0] + M[i][1] * tr[1]) + M[i][2] * tr[2]
            q00 = A[0, 0]; l00 = np.sqrt(q00); l10 = A[1, 0] / l00; l20 = A[2, 0] / l00
            q11 = A[1, 1] - l10 * l10; l11 = np.sqrt(q11); l21 = (A[2, 1] - l20 * l10) / l11
            q22 = A[2, 2] - (l20 * l20 + l21 * l21); l22 = np.sqrt(q22)
            y0 = g[0] / l00; y1 = (g[1] - l10 * y0) / l11; y2 = (g[2] - (l20 * y0 + l21 * y1)) / l22
            X2 = y2 / l22; X1 = (y1 - l21 * X2) / l11; X0 = (y0 - (l10 * X1 + l20 * X2)) / l00
            if not (q00 > min_pivot and q11 > min_pivot and q22 > min_pivot and np.isfinite([X0, X1, X2]).all()):
                continue
            worst = f64(0.0)
            for v in nodes:
                R, tr = poses[v // max_pts, :, :3], poses[v // max_pts, :, 3]
                x, y = f64(xy[v, 0]), f64(xy[v, 1])
                e = [X0 - tr[0], X1 - tr[1], X2 - tr[2]]
                c = [(R[0, j] * e[0] + R[1, j] * e[1]) + R[2, j] * e[2] for j in range(3)]
                front[t] += 1 if c[2] > 0 else 0
                u, w_ = fx * (c[0] / c[2]) + px, fy * (c[1] / c[2]) + py
                err2 = (u - x) * (u - x) + (w_ - y) * (w_ - y)
                worst = err2 if err2 > worst else worst
            out[t] = (X0, X1, X2, np.sqrt(worst))
    return out, front


def six_camera_scene(n_points, seed=0, n_cams=6):
    """The planted scene of the triangulation tests: n_cams cameras on an arc looking at a cloud of points around the
    origin.  Returns (poses float64 [n_cams, 3, 4] camera to world, planted float64 [n_points, 3], pixels float32
    [n_cams, n_points, 2] -- the exact projections rounded to float32 --, and the camera values fx, fy, cx, cy)."""
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = 700.0, 710.0, 320.0, 240.0
    planted = rng.uniform(-1.0, 1.0, size=(n_points, 3))
    poses = np.zeros((n_cams, 3, 4))
    pixels = np.zeros((n_cams, n_points, 2), dtype=np.float32)
    for k in range(n_cams):
        ang = -0.5 + k / max(n_cams - 1, 1)  # radians around the y axis
        centre = np.array([6.0 * np.sin(ang), 0.3 * (k % 3 - 1), -6.0 * np.cos(ang)])
        z = -centre / np.linalg.norm(centre)  # looks at the origin
        x = np.cross([0.0, 1.0, 0.0], z)
        x /= np.linalg.norm(x)
        R = np.stack([x, np.cross(z, x), z], axis=1)  # columns: the camera's axes in the world
        poses[k, :, :3], poses[k, :, 3] = R, centre
        c = (planted - centre) @ R  # R^T (X - t)
        pixels[k, :, 0] = (fx * c[:, 0] / c[:, 2] + cx).astype(np.float32)
        pixels[k, :, 1] = (fy * c[:, 1] / c[:, 2] + cy).astype(np.float32)
    return poses, planted, pixels, (fx, fy, cx, cy)


FILL = -7  # what device_build_tracks puts into every output entry before the call


def device_build_tracks(ctx, counts, n_images, max_pts, pairs, rows, rows_back=None, keep=None, **opts):
    """Runs cusift_build_tracks on hand-written rows: uploads them, calls capi.Context.build_tracks(**opts) and reads
    every entry of every output back -- (track [n, max_pts], offsets [N // 2 + 1], obs [N], stats [8]), each entry the
    library did not write still FILL.  counts: raw counters or None (d_counters = NULL)."""
    pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    n_nodes = n_images * max_pts
    host = [np.full((n_images, max_pts), FILL, np.int32), np.full(n_nodes // 2 + 1, FILL, np.int32),
            np.full(max(n_nodes, 1), FILL, np.int32), np.full(8, FILL, np.int32)]
    inputs = [None if counts is None else np.asarray(counts, dtype=np.uint32), np.ascontiguousarray(rows),
              None if rows_back is None else np.ascontiguousarray(rows_back),
              None if keep is None else np.ascontiguousarray(keep, dtype=np.uint8)]
    ptrs = []
    try:
        for arr in inputs + host:
            ptrs.append(None if arr is None else ctx.malloc(max(arr.nbytes, 16)))
            if arr is not None and arr.nbytes:
                ctx.h2d(ptrs[-1], arr)
        ctx.synchronize()
        d_counts, d_rows, d_back, d_keep, d_track, d_offsets, d_obs, d_stats = ptrs
        ctx.build_tracks(d_counts, n_images, max_pts, pairs, d_rows, d_track, d_offsets, d_obs, d_stats,
                         d_rows_back=d_back, d_keep=d_keep, **opts)
        ctx.synchronize()
        for arr, ptr in zip(host, ptrs[4:]):
            ctx.d2h(arr, ptr)
    finally:
        for ptr in ptrs:
            if ptr is not None:
                ctx.free(ptr)
    return host[0], host[1], host[2], host[3].view(np.uint32)


def assert_tracks_equal(device, model):
    """Every entry of the four device outputs against the model's: the named ones equal, the others never written."""
    track, offsets, obs, stats = device
    m_track, m_offsets, m_obs, m_stats = model
    np.testing.assert_array_equal(stats, m_stats)
    np.testing.assert_array_equal(track, m_track)
    n_tracks, n_obs = len(m_offsets) - 1, len(m_obs)
    np.testing.assert_array_equal(offsets[: n_tracks + 1], m_offsets)
    assert (offsets[n_tracks + 1:] == FILL).all()
    np.testing.assert_array_equal(obs[:n_obs], m_obs)
    assert (obs[n_obs:] == FILL).all()
