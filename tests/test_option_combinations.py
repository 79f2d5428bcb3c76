"""The per-call options in combination: cusift_params.upsample (octave -1) with cusift_ctx_set_keep_strongest, with
root_sift and lowest_scale, through every driver.

Each option has a file of its own (test_upsample.py, test_keep_strongest.py, test_gpu_parity.py); this one is about their
product, where one arena carries the 2x enlarged images at its head, the coarser octaves, the counters, a staged list per
octave and the selection's scratch (resolve_plan, cusift_amd/csrc/sift_driver.hip), and where the selection's secondary
order meets subsampling = 0.5 for the first time (secondary_words, sift_select.hip).

The yardstick is made of what those files already trust: `up2` enlarges the image in numpy float32 (bit-exact with the
kernel), the CPU oracle extracts it with subsampling * 0.5 and init_blur * 2, `strongest` cuts the oracle's records, and
RootSIFT comes from the oracle.  The second yardstick is the device's own unselected run: the kept set is `strongest` of it,
bit for bit.  The bars are the existing ones (assert_matches_oracle, assert_same_bits, assert_layout); every K and max_pts
below is picked on the CPU from the oracle alone and asserted in test_expected_sets_and_their_preconditions.
"""
import functools

import numpy as np
import pytest

from cusift_amd import capi, synth
from cusift_amd.capi import SIFT_POINT_DTYPE, DeviceBuffer
from oracle_binding import Oracle, pitched
from test_keep_strongest import (assert_layout, assert_matches_oracle, assert_same_bits, check_select, context_with,
                                 heads, kept_ids, run_batch, strength_key, strongest, strongest_order, synthetic_heads, tie_cut)
from test_octave_overlap_gpu import MODES
from test_upsample import oracle_upsampled

gpu = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------------------------
# the cases: images, extraction parameters (upsample = 1 is added for the device, the oracle gets the enlarged image)
# ------------------------------------------------------------------------------------------------------------------
def crop(y, x, h, w):
    return synth.fixture_image()[y:y + h, x:x + w].copy()


GRAY1 = dict(num_octaves=5, init_blur=0.0, peak_thresh=1.0)  # 640x480 -> 1280x960, octaves -1 .. 3
SMALL = dict(num_octaves=4, init_blur=0.0, peak_thresh=0.5)
CASES = {
    # max_pts * 64 B is one image's list: with 4096 the lists follow each other at a stride of 256 KiB, with 2501 the lists
    # of octaves 1 .. 4 start off the 256-byte alignment that the images and the selection's scratch get, and 192 bytes of
    # padding lie between the last list and the scratch
    "gray1/4096": (lambda: [synth.fixture_image()], dict(GRAY1, max_pts=4096)),
    "gray1/2501": (lambda: [synth.fixture_image()], dict(GRAY1, max_pts=2501)),
    # 202x154 enlarged at a pitch of 256: ragged rows, odd sizes in every coarser octave (101, 50, 25 wide)
    "101x77": (lambda: [crop(100, 200, 77, 101)], dict(SMALL, max_pts=512)),
    # three different images: the cuts differ per image, and image 1's lists lie between image 0's and image 2's
    "batch": (lambda: [crop(60 * i, 150 * i, 120, 160) for i in range(3)], dict(SMALL, max_pts=1024)),
    # 128x96 enlarged, halved down to 4x3: the most octaves (6) that K takes on this image, see
    # test_num_octaves_up_to_the_limit_of_the_structure
    "64x48": (lambda: [crop(100, 200, 48, 64)], dict(num_octaves=6, init_blur=0.0, peak_thresh=0.5, max_pts=256)),
    # the enlarged octave (2 * 0.5 = 1.0, not above lowest_scale) is not searched: its list stays empty, K cuts the others
    "lowest_scale": (lambda: [crop(0, 0, 120, 160)], dict(SMALL, lowest_scale=1.0, max_pts=1024)),
    # The one deliberate exception to "no octave reaches max_pts": two octaves of which only the coarser one is searched,
    # and max_pts EXACTLY the oracle's count of it.  The last list of the arena is then full to its last slot without
    # losing a candidate (the result is still defined), no padding follows it (2 * 782 * 64 is a multiple of 256), and the
    # selection's scratch begins at the very next byte: a scratch that began one head too early would overwrite a live head.
    "full list": (lambda: [synth.fixture_image()], dict(num_octaves=2, init_blur=0.0, peak_thresh=1.0, lowest_scale=1.0,
                                                        max_pts=782)),
}
FULL = ("full list",)               # cases whose densest list holds exactly max_pts
UNSEARCHED = ("lowest_scale", "full list")  # cases whose enlarged octave is not searched
K_LABELS = ("one", "mid", "one below the total", "the total", "above the total")


@functools.lru_cache(maxsize=None)
def case(name):
    """(images, params dict, per image the oracle's records, the same with RootSIFT) -- computed once, never written."""
    make, prm = CASES[name]
    imgs = make()
    ora = Oracle()
    want, rooted = [], []
    for img in imgs:
        w = oracle_upsampled(ora, img, **prm).copy()
        r = w.copy()
        ora.rootsift(r, len(r))
        for a in (w, r):
            a.setflags(write=False)
        want.append(w)
        rooted.append(r)
    return imgs, prm, want, rooted


@functools.lru_cache(maxsize=None)
def plain_case(name):
    """The same images without the enlarged octave: the oracle's records of the call with every option off."""
    imgs, prm, _, _ = case(name)
    ora = Oracle()
    out = [ora.extract(img, **prm).view(SIFT_POINT_DTYPE).copy() for img in imgs]
    for a in out:
        a.setflags(write=False)
    return out


def expected(name, root_sift=0):
    return case(name)[3 if root_sift else 2]


def params(name, **kw):
    return capi.default_params(**dict(case(name)[1], **kw))


def keeps(name):
    """label -> K.  The first three cut every image of the case; the last two keep everything (K <= max_pts).  Of several
    images "one below the total" is below the smallest total and "the total" is the largest, so each image's own total
    and the K one below it are added: every image meets K == held and K == held - 1."""
    _, prm, want, _ = case(name)
    lo, hi = min(len(w) for w in want), max(len(w) for w in want)
    ks = dict(zip(K_LABELS, (1, lo // 2, lo - 1, hi, prm["max_pts"])))
    if len(want) > 1:
        for i, w in enumerate(want):
            ks["image %d's total" % i] = len(w)
            ks["one below image %d's total" % i] = len(w) - 1
    if name.startswith("gray1"):
        ks["through a tie"] = tie_cut(want[0])
    return ks


def tie_group(records, k):
    order, key = strongest_order(records), strength_key(records["sharpness"])
    return records[key == key[order[k]]]


# ------------------------------------------------------------------------------------------------------------------
# without a GPU
# ------------------------------------------------------------------------------------------------------------------
def ordered_bits(f):
    b = np.ascontiguousarray(f, dtype=np.float32).view(np.uint32)
    return np.where(b >> 31, ~b, b ^ np.uint32(0x80000000)).astype(np.uint32)


def device_order(records):
    """The five words of sift_select.hip, restated word for word: the key descending, then ~ordered_bits(subsampling),
    ordered_bits(y), (x), (scale) ascending.  Independent of `strongest_order`, which compares floats."""
    s0 = ~ordered_bits(records["subsampling"])
    xy = records["coords2D"]
    return np.lexsort((ordered_bits(records["scale"]), ordered_bits(xy[:, 0]), ordered_bits(xy[:, 1]), s0,
                       -strength_key(records["sharpness"])))


def lists_with_half_pixel_octave(rng, n, **kw):
    """Three lists as the driver lays them: coarsest first, subsampling 2, 1 and 0.5."""
    return [[synthetic_heads(rng, n, sub=s, **kw)] for s in (2.0, 1.0, 0.5)]


def test_restatement_with_the_half_pixel_octave():
    # ties across octaves: 2 before 1 before 0.5, whatever the position
    r = heads([(0, 0, 1, 2.0, 0.5), (99, 99, 9, 2.0, 2), (50, 50, 1, 2.0, 1), (1, 1, 1, 2.5, 0.5), (0, 0, 0.5, -2.0, 0.5)])
    assert kept_ids(r, 5) == [3, 1, 2, 4, 0] and kept_ids(r, 2) == [3, 1]
    assert [int(e) for e in r[device_order(r)]["edgeness"]] == [3, 1, 2, 4, 0]
    # the octave word: smaller for the coarser octave, and 0.5 is the largest of the three
    w = ~ordered_bits(np.float32([2.0, 1.0, 0.5, 0.25]))
    assert np.all(np.diff(w.astype(np.int64)) > 0)
    # the two statements of the order agree on lists full of ties that hold the half-pixel octave
    rng = np.random.default_rng(21)
    for levels in (1, 3, 37):
        for n in (1, 65, 700):
            pool = np.concatenate([l[0] for l in lists_with_half_pixel_octave(rng, n, levels=levels, nonfinite=levels == 3)])
            np.testing.assert_array_equal(strongest_order(pool), device_order(pool))


def test_expected_sets_and_their_preconditions():
    for name in CASES:
        imgs, prm, want, rooted = case(name)
        ks = keeps(name)
        for w, r in zip(want, rooted):
            assert len(w) > 20, name
            # no octave reaches max_pts (the enlarged one is the densest), so the lists hold every keypoint
            if name not in FULL:
                for sub in np.unique(w["subsampling"]):
                    assert (w["subsampling"] == sub).sum() < prm["max_pts"], (name, sub)
                assert len(w) < prm["max_pts"]
            assert all(1 <= k <= prm["max_pts"] for k in ks.values())
            # every cutting K cuts, the others keep everything, all are legal
            assert all(1 <= ks[l] < len(w) for l in K_LABELS[:3]), (name, ks)
            assert all(len(w) <= ks[l] <= prm["max_pts"] for l in K_LABELS[3:]), (name, ks)
            assert ks["one"] < ks["mid"] < ks["one below the total"]
            # RootSIFT touches the descriptors only
            for f in ("coords2D", "scale", "sharpness", "orientation", "subsampling"):
                assert w[f].tobytes() == r[f].tobytes()
            assert not np.array_equal(w["data"], r["data"])
            if name in UNSEARCHED:
                assert w["subsampling"].min() == 1.0  # nothing from the enlarged octave
            else:
                assert (w["subsampling"] == 0.5).sum() > 0.1 * len(w)  # the half-pixel octave holds a good part of every cut
                assert (strongest(w, ks["mid"])["subsampling"] == 0.5).any() and (strongest(w, ks["mid"])["subsampling"] > 0.5).any()
    assert len(case("gray1/4096")[2][0]) == len(case("gray1/2501")[2][0]) == 1672
    aligned, ragged = CASES["gray1/4096"][1]["max_pts"], CASES["gray1/2501"][1]["max_pts"]
    assert aligned % 4096 == 0 and ragged % 4096 != 0 and (ragged * 64) % 256 != 0
    # the full list: the only searched octave is the last of the plan, the oracle with ample max_pts finds exactly max_pts
    # keypoints there -- nothing is lost, the same records -- and the two lists end on a 256-byte boundary
    imgs, prm, want, _ = case("full list")
    ample = oracle_upsampled(Oracle(), imgs[0], **dict(prm, max_pts=4096))
    assert len(ample) == prm["max_pts"] == len(want[0]) and ample.tobytes() == want[0].tobytes()
    assert np.all(ample["subsampling"] == 1.0) and prm["num_octaves"] == 2 and (2 * prm["max_pts"] * 64) % 256 == 0
    assert keeps("full list")["the total"] == prm["max_pts"]  # a K that keeps the head in the last slot, whichever it is
    totals = [len(w) for w in case("batch")[2]]
    assert all(keeps("batch")["image %d's total" % i] == t for i, t in enumerate(totals))
    assert len({len(w) for w in case("batch")[2]}) == 3  # three different totals: three different cuts
    # the calls with every option off in test_options_interleaved_on_one_context: nothing saturates, K = mid cuts there too
    for p in plain_case("batch"):
        assert keeps("batch")["mid"] < len(p) < case("batch")[1]["max_pts"]
    # the tie: a group of bit-equal |sharpness| straddles the cut and spans the half-pixel octave and a coarser one
    w = case("gray1/4096")[2][0]
    k = keeps("gray1/4096")["through a tie"]
    assert k is not None and 40 <= k < len(w) and k not in [keeps("gray1/4096")[l] for l in K_LABELS]
    order, key = strongest_order(w), strength_key(w["sharpness"])
    assert key[order[k - 1]] == key[order[k]]
    group = tie_group(w, k)
    assert len(group) >= 2 and len(np.unique(group["coords2D"], axis=0)) == len(group)
    assert 0.5 in group["subsampling"] and group["subsampling"].max() > 0.5
    # ... and the cut falls between the octaves: the coarser member is kept, the half-pixel one is dropped
    assert w[order[k - 1]]["subsampling"] > 0.5 and w[order[k]]["subsampling"] == 0.5
    np.testing.assert_array_equal(order, device_order(w))


# ------------------------------------------------------------------------------------------------------------------
# on the GPU
# ------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def kctx():
    """A context of this module's own (the setting is sticky: the session's shared context is never given one)."""
    c = capi.Context(0)
    yield c
    c.close()


def check_kept(cnt, pts, k, want, unselected=None):
    """One call's output against the oracle's strongest K and, where given, against its own unselected run."""
    for i in range(len(want)):
        assert_layout(cnt[i], pts[i], k, len(want[i]))
        assert_matches_oracle(pts[i, : cnt[i]], strongest(want[i], k))
        if unselected is not None:
            cnt_all, pts_all = unselected
            assert int(cnt_all[i]) == len(want[i])
            assert_same_bits(pts[i, : cnt[i]], strongest(pts_all[i, : cnt_all[i]], k))


# ---- the stage entry point: the half-pixel octave among the lists ----
@gpu
def test_select_with_a_half_pixel_list(kctx):
    """cusift_select_strongest on lists with subsampling 2, 1 and 0.5: secondary_words against strongest_order directly.
    levels = 1: every key equal, the octave word decides the whole cut."""
    rng = np.random.default_rng(22)
    for n, levels in ((700, 1), (1025, 3), (300, 37)):
        lists = lists_with_half_pixel_octave(rng, n, levels=levels)
        for keep in (1, n - 1, n, n + 1, 2 * n, 2 * n + 1, 3 * n - 1, 3 * n):
            check_select(kctx, lists, keep)
    # unequal lists, the half-pixel one the longest and a coarser one empty
    lists = [[synthetic_heads(rng, n, levels=2, sub=s)] for n, s in ((0, 4.0), (65, 2.0), (1, 1.0), (1500, 0.5))]
    for keep in (1, 40, 66, 67, 800, 1565):
        check_select(kctx, lists, keep)


# ---- extract_batch on a context with default policies, against both yardsticks ----
@gpu
@pytest.mark.parametrize("root_sift", [0, 1])
@pytest.mark.parametrize("name", sorted(CASES))
def test_upsample_and_k_keep_the_oracles_strongest(kctx, name, root_sift):
    imgs = case(name)[0]
    prm = params(name, upsample=1, root_sift=root_sift)
    want = expected(name, root_sift)
    unselected = run_batch(kctx, imgs, prm)
    for i in range(len(imgs)):
        assert_matches_oracle(unselected[1][i, : unselected[0][i]], want[i])
    for label, k in keeps(name).items():
        kctx.set_keep_strongest(k)
        cnt, pts = run_batch(kctx, imgs, prm)
        check_kept(cnt, pts, k, want, unselected)
    if root_sift:
        kept = pts[0, : cnt[0]]["data"].astype(np.float64)
        np.testing.assert_allclose((kept[np.isfinite(kept).all(axis=1)] ** 2).sum(axis=1), 1.0, atol=1e-5)


# ---- every staged launch policy ----
@gpu
@pytest.mark.parametrize("name,label,root_sift", [("batch", "mid", 1), ("gray1/2501", "through a tie", 0),
                                                  ("lowest_scale", "mid", 0), ("full list", "the total", 0),
                                                  ("full list", "one below the total", 1)])
@pytest.mark.parametrize("mode", sorted(MODES))
def test_every_launch_policy(mode, name, label, root_sift):
    imgs = case(name)[0]
    prm = params(name, upsample=1, root_sift=root_sift)
    k = keeps(name)[label]
    with context_with(0, 0) as plain:
        unselected = run_batch(plain, imgs, prm)
    with context_with(*MODES[mode], keep=k) as c:
        cnt, pts = run_batch(c, imgs, prm)
        forks = c.forks()
        again = run_batch(c, imgs, prm)  # the second call finds the arena as the first left it
    # (an octave 0 that is not searched has nothing to run on the side stream)
    assert forks == (1 if "fork" in mode and name not in UNSEARCHED else 0)
    check_kept(cnt, pts, k, expected(name, root_sift), unselected)
    check_kept(*again, k, expected(name, root_sift), unselected)


# ---- cusift_extract_host ----
@gpu
@pytest.mark.parametrize("name", ["101x77", "gray1/2501"])
def test_host_entry_point(kctx, name):
    """The upload goes into the context's own memory while the enlarged image claims the head of the arena."""
    img = case(name)[0][0]
    prm = params(name, upsample=1, root_sift=1)
    want = expected(name, 1)[0]
    for label in ("mid", "above the total", "one below the total"):
        k = keeps(name)[label]
        kctx.set_keep_strongest(k)
        d_pts = DeviceBuffer(kctx, prm.max_pts * 588)
        kctx.memset(d_pts.ptr, 0x5A, prm.max_pts * 588)
        h_pts = np.zeros(prm.max_pts, dtype=SIFT_POINT_DTYPE)
        n = kctx.extract_host(img, prm, d_pts.ptr, h_pts)
        kctx.synchronize()
        dev = d_pts.to_numpy(SIFT_POINT_DTYPE, (prm.max_pts,)).copy()
        d_pts.free()
        assert_layout(n, dev, k, len(want))
        assert_matches_oracle(h_pts[:n], strongest(want, k))
        assert_same_bits(h_pts[:n], dev[:n])


# ---- a recorded graph ----
@gpu
def test_graph_replay_keeps_the_recorded_k(kctx):
    """The graph is recorded on the arena of the enlarged plan with K = mid; K is changed (to another cut, then to 0)
    before the replays and eager calls with other options run in between: the recorded K holds, every replay."""
    name = "batch"
    imgs, _, want, _ = case(name)
    prm = params(name, upsample=1)
    k, other = keeps(name)["mid"], keeps(name)["one below the total"]
    stack = np.stack([pitched(i) for i in imgs])
    n, (h, w), p = len(imgs), imgs[0].shape, stack.shape[2]
    d_imgs = DeviceBuffer.from_numpy(kctx, stack)
    d_pts = DeviceBuffer(kctx, n * prm.max_pts * 588)
    d_cnt = DeviceBuffer(kctx, 4 * n)
    kctx.set_keep_strongest(k)
    g = kctx.record_graph(d_imgs.ptr, n, w, h, p, h * p, prm, d_pts.ptr, d_cnt.ptr)
    try:
        for setting in (other, 0):
            kctx.set_keep_strongest(setting)
            kctx.memset(d_pts.ptr, 0x5A, n * prm.max_pts * 588)
            g.launch()
            kctx.synchronize()
            cnt = d_cnt.to_numpy(np.uint32, (n,)).copy()
            pts = d_pts.to_numpy(SIFT_POINT_DTYPE, (n, prm.max_pts)).copy()
            check_kept(cnt, pts, k, want)
            # an eager call between the replays uses the setting of its own time, on the same arena
            cnt_e, pts_e = run_batch(kctx, imgs, prm)
            if setting:
                check_kept(cnt_e, pts_e, setting, want)
            else:
                for i in range(n):
                    assert_matches_oracle(pts_e[i, : cnt_e[i]], want[i])
    finally:
        g.close()
        for b in (d_imgs, d_pts, d_cnt):
            b.free()


# ---- the torch front end ----
@gpu
def test_batch_extractor_with_both_options():
    import torch
    from cusift_amd.batch import BatchExtractor

    name = "batch"
    imgs, prm_kw, _, rooted = case(name)
    k = keeps(name)["mid"]
    ex = BatchExtractor(len(imgs), 160, 120, keep_strongest=k, upsample=1, root_sift=1, **prm_kw)
    try:
        assert ex.params.upsample == 1 and ex.keep_strongest == k
        before = ex.ctx.arena_bytes()
        for _ in range(2):
            _, counts = ex.extract(ex.images_from_numpy(np.stack(imgs)))
            torch.cuda.synchronize()
            assert counts.cpu().tolist() == [k] * len(imgs)
            for got, want in zip(ex.to_host(), rooted):
                assert np.all(np.diff(got["subsampling"]) <= 0)
                assert_matches_oracle(got, strongest(want, k))
        assert ex.ctx.arena_bytes() == before  # reserved for the enlarged plan with its lists and the selection's scratch
    finally:
        ex.close()


# ---- back-to-back calls with different options on one context ----
@gpu
@pytest.mark.parametrize("mode", ["default"] + sorted(MODES))
def test_options_interleaved_on_one_context(mode):
    """Each call lays the arena out its own way -- with or without the enlarged images at its head, with or without a
    list per octave and the selection's scratch, for one image or three -- and must be right whatever ran before it."""
    c = capi.Context(0) if mode == "default" else context_with(*MODES[mode])

    def check(name, upsample, label, root_sift=0):
        k = keeps(name)[label] if label else 0
        c.set_keep_strongest(k)
        want = expected(name, root_sift) if upsample else plain_case(name)
        assert not (root_sift and not upsample)
        cnt, pts = run_batch(c, case(name)[0], params(name, upsample=upsample, root_sift=root_sift))
        if k:
            check_kept(cnt, pts, k, want)
            return
        for i in range(len(want)):
            assert int(cnt[i]) == len(want[i])
            assert np.all(np.diff(pts[i, : cnt[i]]["subsampling"]) <= 0)
            assert_matches_oracle(pts[i, : cnt[i]], want[i])
            assert np.all(pts[i, cnt[i]:].view(np.uint8) == 0x5A)

    try:
        check("batch", 1, "mid")
        check("batch", 0, None)            # both off: no enlarged image, the coarser octaves move to the head
        check("batch", 1, "mid", 1)
        check("batch", 1, "mid", 1)        # the second call finds what the first left
        check("101x77", 1, "one")          # one image: every region elsewhere
        check("batch", 0, "mid")           # K alone
        check("batch", 1, None)            # upsample alone
        check("batch", 1, "one below the total")
        check("gray1/2501", 1, "through a tie")  # the arena grows: everything moves
        check("lowest_scale", 1, "mid")
        check("full list", 1, "the total")  # the last list full to its last slot, the scratch right behind it
        check("batch", 0, None)
        check("batch", 1, "mid")
    finally:
        c.close()


# ---- num_octaves up to kMaxOctaves ----
@gpu
def test_num_octaves_up_to_the_limit_of_the_structure(kctx):
    """num_octaves = 16 (kMaxOctaves) with upsample = 1 on a 64x48 image: the plan holds the enlarged 128x96 octave and is
    clipped where halving ends, 7 octaves down to 2x1.  Halving passes through a width below 4 before it reaches 0 on every
    image, and an octave narrower than 4 (or lower than 3) is not one the fused detection takes, so it has no list: with K
    such a call is REFUSED, with that message -- it cannot be run.  The most octaves K takes here is 6 (down to 4x3), the
    case "64x48" of this file.  With K = 0 the 16-octave call runs, and equals the oracle on the enlarged image."""
    name = "64x48"
    imgs, prm_kw, want, _ = case(name)
    many = params(name, upsample=1, num_octaves=16)
    cnt, pts = run_batch(kctx, imgs, many)
    assert_matches_oracle(pts[0, : cnt[0]], want[0])  # octaves beyond the sixth hold nothing: the same records
    sixteen = oracle_upsampled(Oracle(), imgs[0], **dict(prm_kw, num_octaves=16))
    assert len(sixteen) == len(want[0])
    for f in ("coords2D", "scale", "sharpness", "edgeness", "orientation", "subsampling", "data"):
        assert sixteen[f].tobytes() == want[0][f].tobytes(), f  # the oracle's octaves beyond the sixth hold nothing either
    k = keeps(name)["mid"]
    kctx.set_keep_strongest(k)
    for n_oct in (7, 16):
        with pytest.raises(capi.CusiftError) as e:
            run_batch(kctx, imgs, params(name, upsample=1, num_octaves=n_oct))
        assert "cusift error -1:" in str(e.value) and "not one the fused detection takes" in str(e.value), str(e.value)
        assert "128x96" in str(e.value)  # the message names the enlarged geometry, which is what was refused
    cnt, pts = run_batch(kctx, imgs, params(name, upsample=1))  # ... and 6 octaves still run afterwards
    check_kept(cnt, pts, k, want)


# ---- refusals ----
REFUSAL_CASE = "101x77"


def refused(ctx, images, prm, *words):
    with pytest.raises(capi.CusiftError) as e:
        run_batch(ctx, images, prm)
    assert "cusift error -1:" in str(e.value) and all(w in str(e.value) for w in words), str(e.value)


def still_works(ctx, name=REFUSAL_CASE):
    """After a refusal the context is as it was: the combined call runs and is right."""
    k = keeps(name)["mid"]
    ctx.set_keep_strongest(k)
    cnt, pts = run_batch(ctx, case(name)[0], params(name, upsample=1))
    check_kept(cnt, pts, k, case(name)[2])


@gpu
def test_what_k_cannot_take_is_refused_with_upsample_too(kctx):
    """fused_detect = 0, CUSIFT_POLICY_GENERIC_KERNELS and K > max_pts refuse K with upsample = 1 as they do without."""
    name = REFUSAL_CASE
    imgs = case(name)[0]
    kctx.set_keep_strongest(keeps(name)["mid"])
    refused(kctx, imgs, params(name, upsample=1, fused_detect=0), "keep_strongest", "fused_detect")
    kctx.set_policy(capi.POLICY_GENERIC_KERNELS, 1)
    refused(kctx, imgs, params(name, upsample=1), "keep_strongest", "GENERIC_KERNELS")
    kctx.set_policy(capi.POLICY_GENERIC_KERNELS, 0)
    kctx.set_keep_strongest(case(name)[1]["max_pts"] + 1)
    refused(kctx, imgs, params(name, upsample=1), "keep_strongest", "max_pts")
    still_works(kctx)


@gpu
def test_the_tiled_extractor_refuses_each_option_and_both(kctx):
    name = REFUSAL_CASE
    kctx.set_keep_strongest(keeps(name)["mid"])
    with pytest.raises(capi.CusiftError) as e:  # both set: either refusal will do
        capi.Tiled(kctx, None, 0, 1, 256, 768, params(name, upsample=1))
    assert "cusift error -1:" in str(e.value) and ("upsample" in str(e.value) or "keep_strongest" in str(e.value))
    with pytest.raises(capi.CusiftError, match="keep_strongest"):
        capi.Tiled(kctx, None, 0, 1, 256, 768, params(name))
    kctx.set_keep_strongest(0)
    with pytest.raises(capi.CusiftError, match="upsample"):
        capi.Tiled(kctx, None, 0, 1, 256, 768, params(name, upsample=1))
    still_works(kctx)


@gpu
def test_a_width_whose_clipped_octave_is_too_narrow_is_refused(kctx):
    """With upsample = 1 the enlarged image lies in the arena at a pitch of whole 128 floats, so no caller's width can give
    the enlarged octave a pitch or an alignment that the fused detection does not take.  What a width can still do is leave
    a coarser octave narrower than 4: 6 wide, enlarged 12, halved to 6 and then 3.  Refused with K, by name, not run
    without a list; the same image with two octaves (12 and 6 wide) is taken."""
    narrow = [crop(100, 200, 40, 6)]
    two = dict(num_octaves=2, init_blur=0.0, peak_thresh=0.5, max_pts=256)
    kctx.set_keep_strongest(5)
    refused(kctx, narrow, capi.default_params(upsample=1, **dict(two, num_octaves=3)), "keep_strongest",
            "not one the fused detection takes", "12x80")
    want = oracle_upsampled(Oracle(), narrow[0], **two)
    assert len(want) > 5
    cnt, pts = run_batch(kctx, narrow, capi.default_params(upsample=1, **two))
    check_kept(cnt, pts, 5, [want])
    still_works(kctx)


@gpu
def test_a_callers_odd_pitch_is_gone_after_the_enlargement(kctx):
    """A pitch of 103 floats (rows not 16-byte aligned) is refused with K alone, by the same message, and taken with
    upsample = 1: octave 0 of that plan is the enlarged image in the arena."""
    name = REFUSAL_CASE
    imgs, _, want, _ = case(name)
    k = keeps(name)["mid"]
    kctx.set_keep_strongest(k)
    h, w = imgs[0].shape
    src = np.zeros((h, 103), np.float32)
    src[:, :w] = imgs[0]
    d_img = DeviceBuffer.from_numpy(kctx, src)
    prm = params(name, upsample=1)
    d_pts = DeviceBuffer(kctx, prm.max_pts * 588)
    d_cnt = DeviceBuffer(kctx, 4)
    try:
        with pytest.raises(capi.CusiftError, match="not one the fused detection takes"):
            kctx.extract_batch(d_img.ptr, 1, w, h, 103, h * 103, params(name), d_pts.ptr, d_cnt.ptr)
        kctx.memset(d_pts.ptr, 0x5A, prm.max_pts * 588)
        kctx.extract_batch(d_img.ptr, 1, w, h, 103, h * 103, prm, d_pts.ptr, d_cnt.ptr)
        kctx.synchronize()
        cnt = d_cnt.to_numpy(np.uint32, (1,)).copy()
        pts = d_pts.to_numpy(SIFT_POINT_DTYPE, (1, prm.max_pts)).copy()
    finally:
        for b in (d_img, d_pts, d_cnt):
            b.free()
    check_kept(cnt, pts, k, want)
