"""tests/tracks_model.py is what pins cusift_build_tracks and cusift_triangulate_tracks, so it has to be right first:
its union-find against an independent breadth-first search, its triangulation against planted points.  No GPU."""
import numpy as np

from tracks_model import ROW, build_tracks_model, six_camera_scene, triangulate_model


def random_graph(rng, n, max_pts):
    counts = rng.integers(0, max_pts + 3, size=n)  # zeros and counters above max_pts included
    n_pairs = int(rng.integers(n, 3 * n))
    pairs = rng.integers(0, n, size=(n_pairs, 2))
    rows = np.zeros((n_pairs, max_pts), dtype=ROW)
    rows["score"] = rng.choice([0.1, 0.5, 2.0, np.nan], size=rows.shape, p=[0.3, 0.4, 0.25, 0.05])
    rows["ambiguity"] = rng.choice([0.3, 0.9, np.nan], size=rows.shape, p=[0.8, 0.15, 0.05])
    rows["match"] = rng.integers(-1, max_pts + 1, size=rows.shape)
    back = np.zeros_like(rows)
    back["match"] = rng.integers(-1, max_pts, size=rows.shape)
    # half of the back rows agree with the forward rows
    for p in range(n_pairs):
        for i in range(max_pts):
            m = rows[p, i]["match"]
            if 0 <= m < max_pts and rng.random() < 0.5:
                back[p, m]["match"] = i
    keep = (rng.random(rows.shape) < 0.8).astype(np.uint8)
    return counts, pairs, rows, back, keep


def bfs_tracks(counts, max_pts, pairs, rows, back, keep, rule, lo, hi, min_views):
    """The definition again, with no union-find: adjacency lists and a breadth-first search from every node in order."""
    n = len(counts)
    cnt = np.minimum(counts, max_pts)
    lo32, hi32 = (np.float32(lo) ** 2, np.float32(hi) ** 2) if rule == 1 else (np.float32(lo), np.float32(hi))
    adj = {(f, i): set() for f in range(n) for i in range(cnt[f])}
    accepted = 0
    for p, (a, b) in enumerate(pairs):
        for i in range(cnt[a]):
            r = rows[p, i]
            passes = (r["score"] > lo32) if rule == 0 else (r["score"] < lo32)
            if a == b or not (0 <= r["match"] < cnt[b]) or not passes or not r["ambiguity"] < hi32:
                continue
            if keep is not None and not keep[p, i]:
                continue
            if back is not None and back[p, r["match"]]["match"] != i:
                continue
            accepted += 1
            adj[(a, i)].add((b, int(r["match"])))
            adj[(b, int(r["match"]))].add((a, i))
    seen, tracks, shared, short = set(), [], 0, 0
    for start in sorted(adj):
        if start in seen:
            continue
        comp, queue = [], [start]
        seen.add(start)
        while queue:
            v = queue.pop(0)
            comp.append(v)
            for u in sorted(adj[v] - seen):
                seen.add(u)
                queue.append(u)
        if len(comp) < 2:
            continue
        if len({f for f, _ in comp}) < len(comp):
            shared += 1
        elif len(comp) < min_views:
            short += 1
        else:
            tracks.append(sorted(comp))
    return tracks, accepted, shared, short


def test_union_find_model_equals_breadth_first_search():
    rng = np.random.default_rng(2026)
    seen_shared = seen_short = seen_tracks = 0
    for g in range(200):
        n, max_pts = int(rng.integers(2, 7)), int(rng.integers(1, 9))
        counts, pairs, rows, back, keep = random_graph(rng, n, max_pts)
        rule, min_views = g % 2, 2 + g % 3
        lo, hi = (0.3, 0.8) if rule == 0 else (1.0, 0.8)
        use_back, use_keep = back if g % 4 < 2 else None, keep if g % 3 else None
        track, offsets, obs, stats = build_tracks_model(counts, max_pts, pairs, rows, use_back, use_keep, rule, lo, hi,
                                                        min_views)
        want, accepted, shared, short = bfs_tracks(counts, max_pts, pairs, rows, use_back, use_keep, rule, lo, hi,
                                                   min_views)
        got = [[(int(v) // max_pts, int(v) % max_pts) for v in obs[offsets[t]:offsets[t + 1]]]
               for t in range(len(offsets) - 1)]
        assert got == want, g
        assert list(stats) == [len(want), sum(len(t) for t in want), accepted, shared, short, 0, 0, 0], g
        expect = np.full((n, max_pts), -1, dtype=np.int32)
        for t, nodes in enumerate(want):
            for f, i in nodes:
                expect[f, i] = t
        np.testing.assert_array_equal(track, expect)
        seen_shared, seen_short, seen_tracks = seen_shared + shared, seen_short + short, seen_tracks + len(want)
    # the graphs hold every kind of component often enough to mean something
    assert seen_shared > 10 and seen_short > 10 and seen_tracks > 50, (seen_shared, seen_short, seen_tracks)


def test_triangulation_model_lands_on_planted_points():
    """2,000 planted points over six cameras, pixels rounded to float32.  The bound is twice the largest distance the
    definition's author found in numpy on such a scene (8.6e-6): float32 pixels at 700-pixel focal lengths and 6 units
    of distance leave about 1e-6 of depth noise; the rest is margin for the scene's geometry, not for the arithmetic."""
    poses, planted, pixels, (fx, fy, cx, cy) = six_camera_scene(2000, seed=7)
    n_cams, n_pts = pixels.shape[:2]
    offsets = np.arange(n_pts + 1, dtype=np.int32) * n_cams
    obs = (np.arange(n_cams)[None, :] * n_pts + np.arange(n_pts)[:, None]).reshape(-1).astype(np.int32)
    out, front = triangulate_model(pixels, n_pts, offsets, obs, poses, fx, fy, cx, cy)
    dist = np.linalg.norm(out[:, :3] - planted, axis=1)
    print("triangulation model: largest distance %.3g, median %.3g, largest reprojection error %.3g px"
          % (dist.max(), np.median(dist), out[:, 3].max()))
    assert dist.max() < 2 * 8.6e-6
    assert out[:, 3].max() < 1e-3
    assert (front == n_cams).all()


def test_triangulation_model_marks_degenerate_tracks():
    poses, planted, pixels, (fx, fy, cx, cy) = six_camera_scene(4, seed=3)
    pixels[1] = pixels[0]  # frame 1 is frame 0 again: same pose, same pixels
    poses[1] = poses[0]
    n_pts = 4
    obs = np.array([0, n_pts, 1, 2 * n_pts + 1], dtype=np.int32)  # track 0: frames 0 and 1 (identical rays)
    offsets = np.array([0, 2, 4], dtype=np.int32)
    out, front = triangulate_model(pixels, n_pts, offsets, obs, poses, fx, fy, cx, cy)
    assert (out[0] == 0).all() and front[0] == 0
    assert np.linalg.norm(out[1, :3] - planted[1]) < 2 * 8.6e-6 and front[1] == 2
