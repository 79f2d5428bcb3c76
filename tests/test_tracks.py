"""cusift_build_tracks (cusift_amd/csrc/sift_tracks.hip) on rows written by hand: every output array and all of d_stats
equal tests/tracks_model.py exactly, on one scene of 5 frames x 96 records that holds every kind of component and every
kind of row the contract names; then every refusal, and the answer without pairs."""
import itertools

import numpy as np
import pytest

from tracks_model import FILL, ROW, assert_tracks_equal, build_tracks_model, device_build_tracks

N, MAX_PTS = 5, 96
# both (a, b) and (b, a), a repeated pair, a self pair
PAIRS = np.array([(0, 1), (1, 2), (2, 3), (3, 4), (0, 2), (1, 1), (1, 0), (0, 1), (2, 4), (4, 2)], np.int32)
P01, P12, P23, P34, P02, P11, P10, P01B, P24, P42 = range(len(PAIRS))
RULES = {1: dict(rule=1, lo=0.8, hi=0.9), 0: dict(rule=0, lo=0.3, hi=0.9)}
# d_counters = NULL; a counter above max_pts and short frames; a frame of 0 records
COUNTERS = {"null": None, "clamped": [96, 200, 70, 96, 50], "empty": [96, 200, 0, 96, 50]}


def scene(counters):
    """rows, rows_back, keep of the scene.  A good row (score 0.5, ambiguity 0.5) passes both rules."""
    rng = np.random.default_rng(11)
    rows, back = np.zeros((len(PAIRS), MAX_PTS), ROW), np.zeros((len(PAIRS), MAX_PTS), ROW)
    rows["match"], back["match"] = -1, -1  # match = -1 wherever nothing else is written
    rows["score"], rows["ambiguity"] = 0.5, 0.5
    keep = np.ones((len(PAIRS), MAX_PTS), np.uint8)

    def edge(p, i, m, score=0.5, ambiguity=0.5, mutual=True):
        rows[p, i] = (score, ambiguity, m, 0)
        if mutual and 0 <= m < MAX_PTS:
            back[p, m]["match"] = i

    # chains over 5, 4, 3 and 2 frames
    for p, f in ((P01, 0), (P12, 1), (P23, 2), (P34, 3)):
        edge(p, 3 + f, 4 + f)
    for p, f in ((P01, 0), (P12, 1), (P23, 2)):
        edge(p, 10 + f, 11 + f)
    edge(P12, 15, 16), edge(P23, 16, 17)
    edge(P34, 18, 19)
    # a star around record 20 of frame 2, one ray into every other frame
    edge(P24, 20, 21), edge(P02, 22, 20), edge(P12, 23, 20), edge(P23, 20, 24)
    # two records of frame 0 in one component, only through frames 1 and 2
    edge(P01, 30, 31), edge(P12, 31, 33), edge(P02, 32, 33)
    # ... and through one record of frame 1 (the cross-check lets only one of the two rows through)
    edge(P01, 34, 35), edge(P01, 36, 35)
    # a component of 7 nodes, more than there are frames
    for p in (P01, P12, P23, P34):
        edge(p, 40, 40)
    edge(P02, 41, 40), edge(P10, 42, 41)
    # a self pair: never an edge, whatever its rows say
    for i in range(50, 56):
        edge(P11, i, i + 1)
    # match past the partner's records: 96 and 1000 always, 60 where frame 4 holds 50 records
    edge(P34, 44, 96), edge(P34, 45, 1000), edge(P34, 46, 60), edge(P23, 46, 46)
    # NaN score / ambiguity, and rows that fail one rule, the other, or both
    edge(P01, 47, 47, score=np.nan), edge(P01, 48, 48, ambiguity=np.nan)
    edge(P01, 57, 57, score=0.7), edge(P12, 57, 57)  # 0.7 >= 0.8^2 fails rule 1, passes rule 0: a 2- or 3-chain
    edge(P01, 58, 58, score=0.2), edge(P12, 58, 58)  # fails rule 0 only
    edge(P01, 59, 59, ambiguity=0.85), edge(P12, 59, 59)  # 0.85 >= 0.9^2 fails rule 1 only
    edge(P01, 60, 60, ambiguity=0.95)  # fails both
    # the same edge from both directions and from the repeated pair (counted each time); edges only they bring
    edge(P10, 4, 3), edge(P01B, 3, 4)
    edge(P10, 61, 62), edge(P01B, 63, 64), edge(P12, 64, 65)
    # rows that d_keep takes out: one breaks the 5-chain, one a 2-chain
    edge(P01, 66, 66)
    keep[P01, 66] = 0
    keep[P23, 5] = 0
    # rows the cross-check takes out: the back row names somebody else
    edge(P23, 67, 67, mutual=False), edge(P34, 67, 67)
    back[P23, 67]["match"] = 68
    # behind the records of frame 4 (50 in two settings): a row that is never read there
    edge(P42, 80, 81)
    # and a sprinkling of arbitrary rows among records 68 .. 95 of every pair
    for p in range(len(PAIRS)):
        for i in range(70, MAX_PTS):
            if (p, i) != (P42, 80) and rng.random() < 0.4:
                edge(p, i, int(rng.choice([-1, int(rng.integers(68, MAX_PTS + 2))])), score=float(rng.choice([0.2, 0.5, 0.7])),
                     ambiguity=float(rng.choice([0.5, 0.85])), mutual=bool(rng.random() < 0.7))
    # the matchers leave the rows of a pair with an empty frame unwritten: 0xFF bytes
    if counters is not None:
        for p, (a, b) in enumerate(PAIRS):
            if counters[a] == 0 or counters[b] == 0:
                rows[p].view(np.uint8)[:] = 0xFF
                back[p].view(np.uint8)[:] = 0xFF
    return rows, back, keep


def model_of(counters, rows, back, keep, **opts):
    return build_tracks_model([MAX_PTS] * N if counters is None else counters, MAX_PTS, PAIRS, rows, back, keep, **opts)


def test_the_scene_holds_every_kind_of_component():
    """From the model alone, before any device is looked at."""
    rows, back, keep = scene(None)
    track, offsets, obs, stats = model_of(None, rows, None, None, min_views=2, **RULES[1])
    sizes = set(np.diff(offsets).tolist())
    assert {2, 3, 4, 5} <= sizes, sizes
    assert stats[3] >= 3
    # the star: frames 0 .. 4 around record 20 of frame 2
    star = track[2, 20]
    assert star >= 0 and [int(v) for v in obs[offsets[star]:offsets[star + 1]]] == [22, 96 + 23, 192 + 20, 288 + 24, 384 + 21]
    # the component of 7 nodes and both shared-frame components are dropped; the self pair made nothing
    assert track[0, 40] == -1 and track[0, 30] == -1 and track[0, 34] == -1 and (track[1, 50:57] == -1).all()
    assert track[0, 47] == -1 and track[0, 48] == -1 and track[0, 60] == -1  # NaN, NaN, both rules fail
    assert track[1, 42] == -1 and track[1, 61] >= 0 and track[0, 63] >= 0  # (b, a) and the repeated pair link
    m3 = model_of(None, rows, None, None, min_views=3, **RULES[1])
    assert m3[3][4] > 0 and m3[3][0] == stats[0] - m3[3][4] and m3[3][3] == stats[3]
    # the rules differ, d_keep and d_rows_back each take something out, the counters change the answer
    assert model_of(None, rows, None, None, min_views=2, **RULES[0])[0].tolist() != track.tolist()
    assert track[0, 66] >= 0 and model_of(None, rows, None, keep, min_views=2, **RULES[1])[0][0, 66] == -1
    crossed = model_of(None, rows, back, None, min_views=2, **RULES[1])
    assert track[2, 67] >= 0 and crossed[0][2, 67] == -1 and crossed[0][0, 36] >= 0 and track[0, 36] == -1
    for name in ("clamped", "empty"):
        other = model_of(COUNTERS[name], *scene(COUNTERS[name])[:1], None, None, min_views=2, **RULES[1])
        assert other[3][0] > 0 and other[3].tolist() != stats.tolist(), name
    assert (other[0][2] == -1).all()  # the empty frame


@pytest.mark.gpu
@pytest.mark.parametrize("counters", sorted(COUNTERS))
def test_every_output_equals_the_model(ctx, counters):
    rows, back, keep = scene(COUNTERS[counters])
    for rule, min_views, use_back, use_keep in itertools.product((1, 0), (2, 3), (False, True), (False, True)):
        opts = dict(min_views=min_views, **RULES[rule])
        b, k = back if use_back else None, keep if use_keep else None
        got = device_build_tracks(ctx, COUNTERS[counters], N, MAX_PTS, PAIRS, rows, b, k, **opts)
        assert_tracks_equal(got, model_of(COUNTERS[counters], rows, b, k, **opts))


@pytest.mark.gpu
def test_the_filter_can_be_switched_off(ctx):
    rows, back, keep = scene(None)
    opts = dict(rule=0, lo=-np.inf, hi=np.inf, min_views=2)
    got = device_build_tracks(ctx, None, N, MAX_PTS, PAIRS, rows, **opts)
    model = model_of(None, rows, None, None, **opts)
    assert model[3][2] > model_of(None, rows, None, None, min_views=2, **RULES[0])[3][2]
    assert_tracks_equal(got, model)


@pytest.mark.gpu
def test_without_pairs_every_record_is_alone(ctx):
    rows = np.zeros((1, MAX_PTS), ROW)
    for pairs, max_pts in ((np.zeros((0, 2), np.int32), MAX_PTS), (PAIRS, 0)):
        track, offsets, obs, stats = device_build_tracks(ctx, None, N, max_pts, pairs, rows, min_views=2, **RULES[1])
        assert (track == -1).all() and track.size == N * max_pts
        assert offsets[0] == 0 and (offsets[1:] == FILL).all() and (obs == FILL).all()
        assert (stats == 0).all()


@pytest.mark.gpu
def test_refusals_leave_the_outputs_untouched(ctx):
    from cusift_amd import capi

    rows, back, keep = scene(None)
    n_nodes = N * MAX_PTS
    host = [np.full(n_nodes, FILL, np.int32), np.full(n_nodes // 2 + 1, FILL, np.int32), np.full(n_nodes, FILL, np.int32),
            np.full(8, FILL, np.int32)]
    ptrs = [ctx.malloc(a.nbytes) for a in (rows, back)] + [ctx.malloc(a.nbytes) for a in host]
    try:
        for ptr, arr in zip(ptrs, [rows, back] + host):
            ctx.h2d(ptr, arr)
        d_rows, d_back, d_track, d_offsets, d_obs, d_stats = ptrs
        pairs = np.ascontiguousarray(PAIRS)
        bad_pairs = pairs.copy()
        bad_pairs[3, 1] = N
        good = dict(counters=None, n=N, max_pts=MAX_PTS, pairs=pairs.ctypes.data, n_pairs=len(pairs), rows=d_rows,
                    back=d_back, keep=None, rule=1, lo=0.8, hi=0.9, min_views=2, track=d_track, offsets=d_offsets,
                    obs=d_obs, stats=d_stats)
        cases = [dict(n=-1), dict(n=65536), dict(max_pts=-1), dict(max_pts=(1 << 20) + 1), dict(n_pairs=-1),
                 dict(n_pairs=65536), dict(pairs=None), dict(pairs=bad_pairs.ctypes.data),
                 dict(n=4096, max_pts=1 << 20),  # N = 2^32 > 2^31 - 1
                 dict(rows=None), dict(track=None), dict(offsets=None), dict(obs=None), dict(stats=None),
                 dict(rule=2), dict(rule=-1), dict(lo=np.nan), dict(hi=np.nan), dict(min_views=1), dict(min_views=0),
                 dict(back=d_rows)]
        for case in cases:
            a = dict(good, **case)
            rc = capi.lib().cusift_build_tracks(ctx.handle, a["counters"], a["n"], a["max_pts"], a["pairs"], a["n_pairs"],
                                                a["rows"], a["back"], a["keep"], a["rule"], a["lo"], a["hi"],
                                                a["min_views"], a["track"], a["offsets"], a["obs"], a["stats"])
            assert rc == -1, (case, rc)  # CUSIFT_ERR_INVALID
        ctx.synchronize()
        for ptr, arr in zip(ptrs[2:], host):
            seen = np.empty_like(arr)
            ctx.d2h(seen, ptr)
            assert (seen == FILL).all()
    finally:
        for ptr in ptrs:
            ctx.free(ptr)
