"""The guided registration chains with their second pass on bytes (capi.Context.register_planar_guided /
register_epipolar_guided / register_pnp_guided and the same three on BatchExtractor, match8=True): with
set_match_bits(8) both passes match bytes; the second runs cusift_match8_guided_records / cusift_match8_projected_records,
which quantise into the context's own tables and run the 8-bit guided matcher.

YARDSTICKS.  Both results of a chain equal, bit for bit, the staged route of existing calls under set_match_bits(8): the
register_* call, quantize_descriptors of both record sets into tables of the caller's, match8_guided / match8_projected
under the first result's model at the chain's radius, the estimate_* call.  The scenes are the decoy scenes of
tests/test_guided_registration.py and tests/test_pnp_guided.py: their descriptors 0.75 e_a + 0.5 e_b quantise to two bytes
of 255, so a copy stays a copy and the first pass still names the decoy, which stands in front of the partner.  No
tolerance appears in this file.
"""
import numpy as np
import pytest

import test_guided_registration as planar_scene
import test_pnp_guided as pnp_scene
from match8_model import match8_model, quantize_model
from oracle_binding import SIFT_POINT_DTYPE
from test_match_guided import EPIPOLAR, HOMOGRAPHY

KINDS = ("planar", "epipolar", "pnp")
N = planar_scene.N
N_DUP = planar_scene.N_DUP
OPTS = planar_scene.OPTS
assert (pnp_scene.N, pnp_scene.N_DUP, pnp_scene.OPTS) == (N, N_DUP, OPTS)
RADIUS = {"planar": 5.0, "epipolar": 1.0, "pnp": 2.0}  # the calls' default thresh, which is the guided pass's radius
# On bytes a duplicated row's best and second keys are both 0, and the reference's ambiguity 0 / (0 + 1e-6) is 0: the row is
# a CONFIDENT candidate that names its decoy, where the float descriptors' 0.375 / 0.375 made it no candidate at all.  The
# first pass therefore draws from 280 candidates of which 130 are true: an all-inlier sample of eight has probability
# (130 / 280)^8 = 0.0022, about four in the scenes' 2,000 hypotheses -- too few to rely on -- and about 43 in 20,000.  Four
# points (0.046) and six (0.010) are fine at 2,000.
OPTS_OF = {"planar": OPTS, "pnp": OPTS, "epipolar": dict(OPTS, loops=20000)}


def scene_of(kind):
    """(frame 1, frame 2, rows of the duplicated matches, their partners, their decoys)"""
    if kind == "pnp":
        f1, f2, rows, partners, decoys = pnp_scene.scene()
        return f1, f2, rows[:N_DUP], partners[:N_DUP], decoys
    return planar_scene.scene(HOMOGRAPHY if kind == "planar" else EPIPOLAR)[:5]


def blob(x):
    """Every byte of a result: named tuples, lists, arrays, scalars, None."""
    if x is None:
        return b"none"
    if isinstance(x, (tuple, list)):
        return b"|".join(blob(v) for v in x)
    return np.ascontiguousarray(x).tobytes()


# ----------------------------------------------------------------------------------------------------------------------
# without a GPU
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_first_pass_on_bytes_still_names_the_decoys(kind):
    """The scenes' structure survives quantisation: on bytes a duplicated row ties between its partner and the decoy at a
    key of 0, and the lowest column -- the decoy -- is its match; every other true match is unambiguous."""
    f1, f2, dup_rows, partners, decoys = scene_of(kind)
    q1, q2 = quantize_model(f1["data"]), quantize_model(f2["data"])
    assert q2[decoys].tobytes() == q2[partners].tobytes() == q1[dup_rows].tobytes()
    assert (decoys < partners).all()
    got = match8_model(q1, q2, 1, f2["coords2D"])
    assert np.array_equal(got["match"][dup_rows], decoys) and (got["score"][dup_rows] == 0).all()


def test_the_chains_take_the_option_and_the_refusal_text_is_gone():
    import inspect
    import os

    from cusift_amd import capi

    text = inspect.getsource(capi.Context._guided_chain)
    assert "match8" in text and "cross_check" in text
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for name in ("INTEGRATION.md", "README.md", os.path.join("cusift_amd", "capi.py")):
        assert "no 8-bit guided matcher" not in open(os.path.join(root, name)).read(), name


# ----------------------------------------------------------------------------------------------------------------------
# on the GPU
# ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def own():
    """A context of this test's own: the session's shared context is never switched."""
    from cusift_amd import capi

    if capi.device_count() < 1:
        pytest.fail("gpu test selected but no HIP device is visible")
    c = capi.Context(0)
    yield c
    c.close()


def chain_of(ctx, kind):
    """(the register call, the estimate call, the guided 8-bit matcher on tables, the same on records, the chain), in one
    argument order"""
    cam = pnp_scene.camera()
    if kind == "pnp":
        return (lambda d1, n1, d2, n2, **o: ctx.register_pnp(d1, n1, d2, n2, cam, **o),
                lambda d1, n1, n2, **o: ctx.estimate_pnp(d1, n1, cam, n2, **o),
                lambda t1, t2, m, r, d: ctx.match8_projected(*t1, *t2, m, cam, r, d),
                lambda d1, n1, d2, n2, m, r, d: ctx.match8_projected_records(d1, n1, d2, n2, m, cam, r, d),
                lambda d1, n1, d2, n2, radius=None, **o: ctx.register_pnp_guided(d1, n1, d2, n2, cam, radius, **o))
    model = "homography" if kind == "planar" else "epipolar"
    reg, est, chain = ((ctx.register_planar, ctx.estimate_homography, ctx.register_planar_guided) if kind == "planar" else
                       (ctx.register_epipolar, ctx.estimate_fundamental, ctx.register_epipolar_guided))
    return (reg, est, lambda t1, t2, m, r, d: ctx.match8_guided(*t1, *t2, model, m, r, d),
            lambda d1, n1, d2, n2, m, r, d: ctx.match8_guided_records(d1, n1, d2, n2, model, m, r, d), chain)


def staged(ctx, kind, f1, n1, f2, n2, radius, opts, records):
    """The sequence at bits 8 -- records: through the records front; else on tables of the caller's --: (first result,
    second result, frame 1's records afterwards)."""
    from cusift_amd import capi
    from cusift_amd.capi import DeviceBuffer

    reg, est, on_tables, on_records, _ = chain_of(ctx, kind)
    b1, b2 = DeviceBuffer.from_numpy(ctx, f1), DeviceBuffer.from_numpy(ctx, f2)
    tables = [DeviceBuffer(ctx, len(f) * k) for f in (f1, f2) for k in (128, 8)]
    try:
        first = reg(b1.ptr, n1, b2.ptr, n2, **opts)
        distance = opts.get("distance", 1)
        if records:
            on_records(b1.ptr, n1, b2.ptr, n2, first[0], radius, distance)
        else:
            ctx.quantize_descriptors(b1.ptr, n1, tables[0].ptr, tables[1].ptr)
            ctx.quantize_descriptors(b2.ptr, n2, tables[2].ptr, tables[3].ptr)
            on_tables((b1.ptr, n1, tables[0].ptr, tables[1].ptr), (b2.ptr, n2, tables[2].ptr, tables[3].ptr), first[0],
                      radius, distance)
        rule, lo, hi = capi._rule_defaults(distance, opts.get("rule"), opts.get("lo"), opts.get("hi"))
        again = {k: v for k, v in opts.items() if k != "distance"}
        again.update(rule=rule, lo=lo, hi=hi)
        second = est(b1.ptr, n1, n2, **again)
        assert b2.to_numpy(SIFT_POINT_DTYPE, (len(f2),)).tobytes() == f2.tobytes()
        return first, second, b1.to_numpy(SIFT_POINT_DTYPE, (len(f1),))
    finally:
        for b in [b1, b2] + tables:
            b.free()


def run_chain(ctx, kind, f1, n1, f2, n2, radius, opts):
    """The chain on fresh uploads: (first result, second result, frame 1's records afterwards)."""
    from cusift_amd.capi import DeviceBuffer

    d1, d2 = DeviceBuffer.from_numpy(ctx, f1), DeviceBuffer.from_numpy(ctx, f2)
    try:
        first, guided = chain_of(ctx, kind)[4](d1.ptr, n1, d2.ptr, n2, radius, match8=True, **opts)
        assert d2.to_numpy(SIFT_POINT_DTYPE, (len(f2),)).tobytes() == f2.tobytes()
        return first, guided, d1.to_numpy(SIFT_POINT_DTYPE, (len(f1),))
    finally:
        d1.free()
        d2.free()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_chain_at_8_bits_equals_the_staged_route_and_recovers_the_duplicated_matches(own, kind):
    f1, f2, dup_rows, partners, decoys = scene_of(kind)
    own.set_match_bits(8)
    # the chain's own radius with every record, a radius of the caller's with frame 1 short of its buffer
    for n1, radius in ((N, None), (N - 37, 1.5 * RADIUS[kind])):
        first, guided, after = run_chain(own, kind, f1, n1, f2, N, radius, OPTS_OF[kind])
        for records in (False, True):  # tables of the caller's; the records front by hand
            want_first, want_guided, want_after = staged(own, kind, f1, n1, f2, N, radius or RADIUS[kind], OPTS_OF[kind],
                                                         records=records)
            assert blob(list(first)) == blob(list(want_first))
            assert blob(list(guided)) == blob(list(want_guided))
            assert after.tobytes() == want_after.tobytes()
        assert after[n1:].tobytes() == f1[n1:].tobytes()
        if n1 < N:
            continue
        print("%s at 8 bits: first %d candidates, %d inliers, %d fit; guided %d candidates, %d inliers, %d fit" % (
            kind, first.num_candidates, first.num_matches, first.num_fit, guided.num_candidates, guided.num_matches,
            guided.num_fit))
        # the first pass keeps none of the duplicated matches, the guided pass counts all of them
        assert first.num_matches >= 100 and not first.inliers[dup_rows].any()
        assert guided.inliers[dup_rows].all() and guided.num_fit >= first.num_fit + N_DUP
        assert np.array_equal(after["match"][dup_rows], partners) and (after["score"][dup_rows] == 0).all()


def extractor_stub(ctx, f1, f2, n1):
    """A BatchExtractor around two frames in N-record slots, as tests/test_pnp_guided.py makes one: frame 0 holds n1
    records, frame 1's counter is past the capacity and is clamped."""
    import torch

    from cusift_amd import batch

    stub = batch.BatchExtractor.__new__(batch.BatchExtractor)
    points = torch.from_numpy(np.stack([f1, f2]).view(np.uint8).reshape(2, N, 588).copy()).to("cuda")
    counts = torch.tensor([n1, N + 1000], dtype=torch.int32, device="cuda")
    stub.ctx, stub.max_pts, stub.n, stub.slots, stub.device = ctx, N, 2, [(points, counts)], points.device
    torch.cuda.synchronize()
    return stub, points


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_batch_extractor_chain_at_8_bits_equals_the_staged_route(own, kind):
    """BatchExtractor.register_*_guided(match8=True) over its slots' records with its context at 8 bits: the staged
    route's two results and the same bytes in frame i's records, with frame i holding fewer records than its slot."""
    import torch

    f1, f2 = scene_of(kind)[:2]
    n1 = N - 37
    own.set_match_bits(8)
    stub, points = extractor_stub(own, f1, f2, n1)
    if kind == "pnp":
        got = stub.register_pnp_guided(0, 1, pnp_scene.camera(), match8=True, **OPTS_OF[kind])
    else:
        chain = stub.register_planar_guided if kind == "planar" else stub.register_epipolar_guided
        got = chain(0, 1, match8=True, **OPTS_OF[kind])
    torch.cuda.synchronize()
    after = points[0].cpu().numpy().reshape(-1).view(SIFT_POINT_DTYPE)
    want_first, want_guided, want_after = staged(own, kind, f1, n1, f2, N, RADIUS[kind], OPTS_OF[kind], records=False)
    assert blob(list(got[0])) == blob(list(want_first)) and blob(list(got[1])) == blob(list(want_guided))
    assert after.tobytes() == want_after.tobytes()
    assert got[1].num_matches > got[0].num_matches >= 6


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_batch_extractor_match8_guided_equals_the_records_front(own, kind):
    """BatchExtractor.match8_guided / match8_projected on quantize(slot)'s tables: frame i's records afterwards are the
    records front's, with frame i holding fewer records than its slot."""
    import torch

    from cusift_amd.capi import DeviceBuffer

    f1, f2 = scene_of(kind)[:2]
    n1 = N - 37
    model = pnp_scene.RT_TRUE if kind == "pnp" else planar_scene.scene(HOMOGRAPHY if kind == "planar" else EPIPOLAR)[5]
    stub, points = extractor_stub(own, f1, f2, n1)
    with pytest.raises(Exception, match="quantize"):
        stub.match8_guided(0, 1, "homography", np.eye(3), 5.0)
    # the tables are torch's, the context has a stream of its own: they are made, and zeroed, before it writes them
    stub._desc8 = {0: (torch.zeros((2, N, 128), dtype=torch.uint8, device="cuda"),
                       torch.zeros((2, N, 2), dtype=torch.int32, device="cuda"))}
    torch.cuda.synchronize()
    stub.quantize(0)
    if kind == "pnp":
        stub.match8_projected(0, 1, model, pnp_scene.camera(), RADIUS[kind])
    else:
        stub.match8_guided(0, 1, "homography" if kind == "planar" else "epipolar", model, RADIUS[kind])
    torch.cuda.synchronize()
    after = points[0].cpu().numpy().reshape(-1).view(SIFT_POINT_DTYPE)
    on_records = chain_of(own, kind)[3]
    b1, b2 = DeviceBuffer.from_numpy(own, f1), DeviceBuffer.from_numpy(own, f2)
    try:
        on_records(b1.ptr, n1, b2.ptr, N, model, RADIUS[kind], 1)
        own.synchronize()
        want = b1.to_numpy(SIFT_POINT_DTYPE, (N,))
    finally:
        b1.free()
        b2.free()
    assert after.tobytes() == want.tobytes()
    assert (after["match"][:n1] >= 0).sum() >= 100 and after[n1:].tobytes() == f1[n1:].tobytes()


@pytest.mark.gpu
def test_chains_still_refuse_under_the_cross_check_and_32_bits_is_what_it_was(own):
    from cusift_amd import capi
    from cusift_amd.capi import DeviceBuffer

    f1, f2 = scene_of("planar")[:2]
    d1, d2 = DeviceBuffer.from_numpy(own, f1), DeviceBuffer.from_numpy(own, f2)
    p1, p2 = (DeviceBuffer.from_numpy(own, f) for f in scene_of("pnp")[:2])
    try:
        own.set_cross_check(True)
        for bits, more in ((8, dict(match8=True)), (32, dict(match8=True)), (32, {})):
            own.set_match_bits(bits)
            for chain in (own.register_planar_guided, own.register_epipolar_guided):
                with pytest.raises(capi.CusiftError, match="cross-check"):
                    chain(d1.ptr, N, d2.ptr, N, **OPTS, **more)
            with pytest.raises(capi.CusiftError, match="cross-check"):
                own.register_pnp_guided(p1.ptr, N, p2.ptr, N, pnp_scene.camera(), **OPTS, **more)
        own.synchronize()
        assert d1.to_numpy(SIFT_POINT_DTYPE, (N,)).tobytes() == f1.tobytes()  # refused before anything ran
        own.set_cross_check(False)
        # at 32 the chain enqueues what it always did: register, match_guided, estimate
        own.set_match_bits(32)
        first, guided = own.register_planar_guided(d1.ptr, N, d2.ptr, N, **OPTS)
        after = d1.to_numpy(SIFT_POINT_DTYPE, (N,))
        own.h2d(d1.ptr, f1)
        want_first = own.register_planar(d1.ptr, N, d2.ptr, N, **OPTS)
        own.match_guided(d1.ptr, N, d2.ptr, N, "homography", want_first[0], 5.0, 1)
        rule, lo, hi = capi._rule_defaults(1, None, OPTS["lo"], None)
        want_guided = own.estimate_homography(d1.ptr, N, N, rule=rule, lo=lo, hi=hi, loops=OPTS["loops"], seed=OPTS["seed"])
        assert blob(list(first)) == blob(list(want_first)) and blob(list(guided)) == blob(list(want_guided))
        assert after.tobytes() == d1.to_numpy(SIFT_POINT_DTYPE, (N,)).tobytes()
        assert (after["score"][scene_of("planar")[2]] == np.float32(0.375)).all()  # the float descriptors' score
    finally:
        for d in (d1, d2, p1, p2):
            d.free()
