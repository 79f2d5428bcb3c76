"""cusift_build_tracks where tracks_shared_kernel (cusift_amd/csrc/sift_tracks.hip) has to probe in earnest.

Every node of a component of 2 .. n_images nodes puts its root into its FRAME's open-addressing set; finding the root
there already flags the component.  The scenes of the other track tests hardly collide (a restatement of the insertion
over them finds chains of 3 at the most and never a step from the last slot to slot 0), so `h = (h + 1u) & mask` at
h == mask, `seen == r` behind foreign roots and the walk past foreign roots were all but unexecuted.  Here the scenes
are built from nodes chosen by their HOME SLOT ((r * 2654435761) mod 2^32) >> (32 - log_slots): a node of an early frame
that is linked only to later frames is its component's root, so the roots that meet in a late frame's set can be picked.

  * probe_scene(40, 8): 16 slots, met exactly by 2 * max_pts.  The last frame's 8 records hang on 8 roots whose homes
    are the last two slots: the set is exactly half full and its chain runs across the end.  The frame before holds
    three flagged components (two records each) and two clean ones whose five roots all have slot `mask` as home: at
    most one of them can sit at home, so at least two flagged roots are found behind foreign roots whatever the order
    of arrival, and a clean root with a flagged root's home passes over it unflagged.
  * probe_scene(40, 12): 24 slots wanted, 32 taken (max_pts is no power of two); the same construction.
  * one_record_scene(): max_pts = 1, two slots, a shift by 31.
  * twin_scene(): a component of exactly n_images nodes with two records in one frame -- found by the hash route, the
    pigeonhole shortcut `sz > n_images` does not apply --, its clean twin of n_images nodes and a component of
    n_images + 1 nodes beside them.
  * n_images = 0 and n_images = 1 (a self pair only): tracks_empty_kernel with zero nodes, and the whole chain of
    launches without an edge.

The insertion and the table shape are restated here (probe_plan); the model (tests/tracks_model.py) stays the definition
of the outputs.  The occupied slots of linear probing do not depend on the order of arrival, so the premises are asserted
on several orders and must hold in each; every premise test prints its plan, and a scene that does not do what it is for
fails on the CPU.  Every device run must equal the model in all four outputs, and a second run must give the same bytes.

Tried once in a scratch build that was never committed: `shared[r] = 1` only where the root is found at its home slot
(h still the hash).  test_every_output_equals_the_model[pow2] and [not_pow2] fail on d_stats -- 1 flagged component
against the model's 3, and 1 against 5: the one that can sit at home, the others turned into tracks (12 for 10, 18 for
14) --; [one] and [twins] stay green, as they must: their flagged roots are found at home.  Of the older tests
tests/test_tracks_sizes.py's planted scene notices it too (1,341 flagged components for 1,369: its chains reach 3); none
of them steps across the end of a set.
"""
import numpy as np
import pytest

from tracks_model import FILL, ROW, assert_tracks_equal, build_tracks_model, device_build_tracks

OPTS = dict(rule=1, lo=0.8, hi=0.9, min_views=2)
ORDERS = 6  # arrival orders the premises are asserted on: ascending, descending and four random ones


# ---- the restatement: table shape, home slot, insertion ------------------------------------------
def log_slots_of(max_pts):
    log_slots = 1
    while (1 << log_slots) < 2 * max_pts:
        log_slots += 1
    return log_slots


def home_slot(r, log_slots):
    return ((r * 2654435761) & 0xFFFFFFFF) >> (32 - log_slots)


def components(n_nodes, edges):
    """(root [n_nodes], size {root: nodes}) of the graph: the root is the component's smallest node."""
    parent = list(range(n_nodes))

    def find(v):
        while parent[v] != v:
            v = parent[v]
        return v

    for a, b in edges:
        ra, rb = find(a), find(b)
        parent[max(ra, rb)] = min(ra, rb)
    root = [find(v) for v in range(n_nodes)]
    size = {}
    for r in root:
        size[r] = size.get(r, 0) + 1
    return root, size


def probe_plan(n_images, max_pts, root, size, order):
    """tracks_shared_kernel with the nodes of every frame arriving in `order` (a permutation of the records).  Returns
    (per frame: occupied slots, longest probe chain, steps from slot `mask` to slot 0; the flagged roots)."""
    log_slots = log_slots_of(max_pts)
    mask = (1 << log_slots) - 1
    frames, flagged = [], set()
    for f in range(n_images):
        table, chain, wraps = [-1] * (mask + 1), 0, 0
        for i in order:
            r = root[f * max_pts + i]
            if size[r] < 2 or size[r] > n_images:
                continue
            h, steps = home_slot(r, log_slots), 1
            while True:
                if table[h] == -1:
                    table[h] = r
                    break
                if table[h] == r:
                    flagged.add(r)
                    break
                wraps += 1 if h == mask else 0
                h = (h + 1) & mask
                steps += 1
            chain = max(chain, steps)
        frames.append(dict(occupied=frozenset(s for s in range(mask + 1) if table[s] != -1), chain=chain, wraps=wraps))
    return frames, flagged


def plans(n_images, max_pts, root, size):
    rng = np.random.default_rng(2)
    orders = [list(range(max_pts)), list(range(max_pts - 1, -1, -1))]
    orders += [rng.permutation(max_pts).tolist() for _ in range(ORDERS - 2)]
    return [probe_plan(n_images, max_pts, root, size, order) for order in orders]


# ---- scenes: directed edges (node a -> node b) become the row of pair (frame a, frame b) ----------
def rows_of(n_images, max_pts, edges):
    pairs = sorted({(a // max_pts, b // max_pts) for a, b in edges})
    rows = np.zeros((len(pairs), max_pts), ROW)
    rows["score"], rows["ambiguity"], rows["match"] = 0.5, 0.5, -1
    for a, b in edges:
        p = pairs.index((a // max_pts, b // max_pts))
        assert rows["match"][p, a % max_pts] == -1, "two edges in one row"
        rows["match"][p, a % max_pts] = b % max_pts
    return np.asarray(pairs, np.int32), rows


def probe_scene(n_images, max_pts):
    """-> dict(edges, flagged, clean, hung).  Frame n_images - 1: every record hangs on a root of its own whose home is
    one of the last two slots (`hung`).  Frame n_images - 2: (max_pts - 2) // 2 components with two records there
    (`flagged`: root -> first record, second record -> root) and the remaining records on roots of their own (`clean`),
    all of these roots with slot `mask` as home."""
    log_slots = log_slots_of(max_pts)
    mask = (1 << log_slots) - 1
    last, prev = n_images - 1, n_images - 2
    early = range(prev * max_pts)  # nodes of the frames before the two
    at_end = [v for v in early if home_slot(v, log_slots) == mask]
    before_end = [v for v in early if home_slot(v, log_slots) == mask - 1]
    n_flagged = (max_pts - 2) // 2
    n_clean = max_pts - 2 * n_flagged
    assert len(at_end) >= n_flagged + n_clean + max_pts // 2 and len(before_end) >= max_pts - max_pts // 2
    flagged, clean = at_end[:n_flagged], at_end[n_flagged:n_flagged + n_clean]
    hung = at_end[n_flagged + n_clean:][:max_pts // 2] + before_end[:max_pts - max_pts // 2]
    edges = []
    for k, r in enumerate(flagged):
        edges += [(r, prev * max_pts + 2 * k), (prev * max_pts + 2 * k + 1, r)]
    edges += [(r, prev * max_pts + 2 * n_flagged + k) for k, r in enumerate(clean)]
    edges += [(r, last * max_pts + k) for k, r in enumerate(hung)]
    return dict(n_images=n_images, max_pts=max_pts, edges=edges, flagged=flagged, clean=clean, hung=hung)


def one_record_scene():
    """max_pts = 1: a node is a frame.  Components {0, 1}, {2, 3, 4}, {5, 6}, {7, 8}, {9, 10, 11}; frame 12 alone."""
    edges = [(0, 1), (2, 3), (3, 4), (5, 6), (7, 8), (9, 10), (9, 11)]
    return dict(n_images=13, max_pts=1, edges=edges)


TWIN_N, TWIN_PTS = 10, 4


def twin_scene():
    """Record 0: frames 0 .. 8 chained and record 1 of frame 8 on record 0 of frame 7 -- ten nodes, frame 8 twice,
    frame 9 never.  Record 2: frames 0 .. 9 chained, ten nodes, one per frame.  Record 3: frames 0 .. 9 chained and
    record 1 of frame 9 on record 3 of frame 8 -- eleven nodes."""
    m = TWIN_PTS
    edges = [(f * m + 0, (f + 1) * m + 0) for f in range(8)] + [(8 * m + 1, 7 * m + 0)]
    edges += [(f * m + 2, (f + 1) * m + 2) for f in range(9)]
    edges += [(f * m + 3, (f + 1) * m + 3) for f in range(9)] + [(9 * m + 1, 8 * m + 3)]
    return dict(n_images=TWIN_N, max_pts=m, edges=edges)


SCENES = {"pow2": lambda: probe_scene(40, 8), "not_pow2": lambda: probe_scene(40, 12), "one": one_record_scene,
          "twins": twin_scene}


@pytest.fixture(scope="module")
def models():
    out = {}
    for name, make in SCENES.items():
        sc = make()
        n, m = sc["n_images"], sc["max_pts"]
        pairs, rows = rows_of(n, m, sc["edges"])
        out[name] = (sc, pairs, rows, build_tracks_model([m] * n, m, pairs, rows, **OPTS))
    return out


def print_plan(name, n_images, max_pts, frames):
    print("%s: %d frames x %d records, log_slots %d, %d slots" % (name, n_images, max_pts, log_slots_of(max_pts),
                                                                  1 << log_slots_of(max_pts)))
    for f, fr in enumerate(frames):
        if fr["occupied"]:
            print("  frame %2d: slots %s, longest chain %d, wraps %d" % (f, sorted(fr["occupied"]), fr["chain"],
                                                                       fr["wraps"]))


@pytest.mark.parametrize("name,log_slots,slots", [("pow2", 4, 16), ("not_pow2", 5, 32)])
def test_the_scene_fills_a_set_across_its_end(models, name, log_slots, slots):
    sc, pairs, rows, (track, offsets, obs, stats) = models[name]
    n, m = sc["n_images"], sc["max_pts"]
    assert log_slots_of(m) == log_slots and (1 << log_slots) == slots >= 2 * m and slots < 4 * m
    assert (slots == 2 * m) == (name == "pow2")  # 2 * max_pts slots met exactly, and not
    mask, last, prev = slots - 1, n - 1, n - 2
    root, size = components(n * m, sc["edges"])
    # the chosen nodes are roots, of components that go by the hash route
    for r in sc["flagged"] + sc["clean"] + sc["hung"]:
        assert root[r] == r and 2 <= size[r] <= 3 < n
    assert all(size[r] == 3 for r in sc["flagged"]) and all(size[r] == 2 for r in sc["clean"] + sc["hung"])
    all_plans = plans(n, m, root, size)
    print_plan(name, n, m, all_plans[0][0])
    for frames, flagged in all_plans:
        # the occupied slots and the flags do not depend on the order of arrival
        assert [fr["occupied"] for fr in frames] == [fr["occupied"] for fr in all_plans[0][0]]
        assert flagged == set(sc["flagged"])
        for f in (last, prev):
            assert {mask, 0} <= frames[f]["occupied"] and frames[f]["wraps"] >= 1 and frames[f]["chain"] >= 4, (f, frames[f])
        # the last frame's set: exactly half of 2 * max_pts slots, the stated maximum
        assert len(frames[last]["occupied"]) == m and frames[last]["chain"] >= m - 1
        assert len(frames[prev]["occupied"]) == len(sc["flagged"]) + len(sc["clean"])
    # flagged and unflagged roots share a home slot, and two flagged ones do: at most one root sits at home, so a
    # flagged root is found behind a foreign one in every order
    homes = {home_slot(r, log_slots) for r in sc["flagged"] + sc["clean"]}
    assert homes == {mask} and len(sc["flagged"]) >= 2 and len(sc["clean"]) >= 1
    assert {home_slot(r, log_slots) for r in sc["hung"]} == {mask - 1, mask}
    # the model: the flagged components dropped, every other one a track of two nodes
    assert stats[3] == len(sc["flagged"]) and stats[0] == len(sc["clean"]) + len(sc["hung"]) and stats[4] == 0
    assert (np.diff(offsets) == 2).all() and stats[2] == len(sc["edges"])
    assert all(track.reshape(-1)[r] == -1 for r in sc["flagged"]) and all(track.reshape(-1)[r] >= 0 for r in sc["clean"])
    assert (track[last] >= 0).all() and (track[prev, :2 * len(sc["flagged"])] == -1).all()


def test_the_scene_of_one_record_uses_both_slots(models):
    sc, pairs, rows, (track, offsets, obs, stats) = models["one"]
    n = sc["n_images"]
    assert log_slots_of(1) == 1  # two slots, the hash shifted by 31
    root, size = components(n, sc["edges"])
    homes = {home_slot(r, 1) for r in set(root) if size[r] >= 2}
    assert homes == {0, 1}, homes
    frames, flagged = probe_plan(n, 1, root, size, [0])
    print_plan("one", n, 1, frames)
    assert not flagged and {s for fr in frames for s in fr["occupied"]} == {0, 1}
    assert all(len(fr["occupied"]) == (1 if size[root[f]] >= 2 else 0) for f, fr in enumerate(frames))
    assert stats[0] == 5 and stats[3] == 0 and np.diff(offsets).tolist() == [2, 3, 2, 2, 3] and track[12, 0] == -1


def test_the_scene_of_the_twins_goes_by_the_hash_route(models):
    sc, pairs, rows, (track, offsets, obs, stats) = models["twins"]
    n, m = sc["n_images"], sc["max_pts"]
    root, size = components(n * m, sc["edges"])
    shared, clean, large = root[0], root[2], root[3]
    assert (shared, clean, large) == (0, 2, 3)
    assert size[shared] == n and size[clean] == n and size[large] == n + 1  # no pigeonhole for the first two
    for frames, flagged in plans(n, m, root, size):
        assert flagged == {shared}  # by the set of frame 8 alone; the large one is never inserted
        assert all(len(fr["occupied"]) == (1 if f == 9 else 2) for f, fr in enumerate(frames))
    print_plan("twins", n, m, frames)
    assert stats[3] == 2 and stats[0] == 1 and stats[1] == n and stats[4] == 0
    assert (track[:, 2] == 0).all() and (track[:, [0, 1, 3]] == -1).all()
    assert obs.tolist() == [f * m + 2 for f in range(n)]


def edge_cases():
    """n_images = 0: no pair can be named.  n_images = 1: a self pair, never an edge."""
    rows = np.zeros((1, 8), ROW)
    rows["score"], rows["ambiguity"] = 0.5, 0.5
    rows["match"][0] = (np.arange(8) + 1) % 8
    return {"no_frame": (0, np.zeros((0, 2), np.int32), rows), "one_frame": (1, np.array([(0, 0)], np.int32), rows)}


def test_the_edge_scenes_have_no_track():
    for name, (n, pairs, rows) in edge_cases().items():
        track, offsets, obs, stats = build_tracks_model([8] * n, 8, pairs, rows, **OPTS)
        assert track.shape == (n, 8) and (track == -1).all() and offsets.tolist() == [0] and len(obs) == 0
        assert (stats == 0).all(), name
        # the launch: one workgroup of 256 even for zero nodes
        assert max(1, -(-(n * 8) // 256)) == 1


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SCENES))
def test_every_output_equals_the_model(ctx, models, name):
    sc, pairs, rows, model = models[name]
    first = device_build_tracks(ctx, None, sc["n_images"], sc["max_pts"], pairs, rows, **OPTS)
    assert_tracks_equal(first, model)
    second = device_build_tracks(ctx, None, sc["n_images"], sc["max_pts"], pairs, rows, **OPTS)
    for a, b in zip(first, second):
        assert a.tobytes() == b.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["no_frame", "one_frame"])
def test_no_frame_and_one_frame(ctx, name):
    n, pairs, rows = edge_cases()[name]
    model = build_tracks_model([8] * n, 8, pairs, rows, **OPTS)
    for counts in (None, [8] * n):
        got = device_build_tracks(ctx, counts, n, 8, pairs, rows, **OPTS)
        assert_tracks_equal(got, model)
        track, offsets, obs, stats = got
        assert offsets[0] == 0 and (offsets[1:] == FILL).all() and (obs == FILL).all() and (stats == 0).all()
        assert track.size == n * 8 and (track == -1).all()
