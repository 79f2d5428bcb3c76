"""Batched SIFT extraction on torch device tensors.

torch is plumbing here (HBM allocations, the stream, torch.distributed); every kernel is launched by
libcusift_amd.so through the C ABI on the stream this object was created on.
"""
import numpy as np
import torch

from . import capi


class Tracks:
    """What BatchExtractor.build_tracks leaves on the device (cusift_build_tracks): track int32 [n, max_pts] (the track of
    every record, -1: none), offsets int32 [N // 2 + 1] and obs int32 [N] (the nodes frame * max_pts + record of track t
    at obs[offsets[t] : offsets[t + 1]], ascending), stats int32 [8] (tracks, observations, accepted rows, components
    dropped for a shared frame, dropped for min_views only), and what they were built from: the pair list, the matcher's
    rows / rows_back int32 [P, max_pts, 4] (MatchRow) and keep uint8 [P, max_pts] or None."""

    def __init__(self, n_images, max_pts, pairs, track, offsets, obs, stats, rows, rows_back, keep):
        self.n_images, self.max_pts, self.pairs = n_images, max_pts, pairs
        self.track, self.offsets, self.obs, self.stats = track, offsets, obs, stats
        self.rows, self.rows_back, self.keep = rows, rows_back, keep

    def to_host(self):
        """Blocking: (T, [[(frame, record), ...] per track])."""
        n_tracks = int(self.stats[0].item())
        offsets = self.offsets[: n_tracks + 1].cpu().numpy()
        obs = self.obs[: int(offsets[-1])].cpu().numpy()
        return n_tracks, [[(int(v) // self.max_pts, int(v) % self.max_pts) for v in obs[offsets[t]:offsets[t + 1]]]
                          for t in range(n_tracks)]


class BundleResult:
    """What BatchExtractor.bundle_adjust leaves on the device (cusift_bundle_adjust), all float64: poses [n, 12] (row-
    major [R | t], camera to world), points3d [cap, 4] = (X, Y, Z, largest reprojection error in pixels; an unused
    track keeps its input row), history [iterations, 4] = (cost, trial cost, lambda, 1 accepted / 0 rejected / 2 not
    run), summary [8] = (entry cost, final cost, accepted steps, iterations run, used tracks, used observations, free
    frames, final lambda)."""

    def __init__(self, poses, points3d, history, summary):
        self.poses, self.points3d, self.history, self.summary = poses, points3d, history, summary

    def to_host(self):
        """Blocking: (poses [n, 4, 4] as chain_poses returns them, points3d, history, summary) as numpy arrays."""
        rt = self.poses.cpu().numpy().reshape(-1, 3, 4)
        poses = np.tile(np.eye(4), (len(rt), 1, 1))
        poses[:, :3, :] = rt
        return poses, self.points3d.cpu().numpy(), self.history.cpu().numpy(), self.summary.cpu().numpy()


class BatchExtractor:
    """Extracts SiftData for a batch of equally sized, HBM-resident float32 images.

    The batch form of SiftData::Extract (cuSIFT.cu:61-120): `extract()` only enqueues work -- no
    allocation, no host read-back -- and returns device tensors:
        points  uint8  [n, max_pts, 588]   (SiftPoint records, cuSIFT.h:10-30)
        counts  int32  [n]                 raw counters; valid points = min(count, max_pts)
    keep_strongest = K > 0: every image keeps its K strongest keypoints (cusift_ctx_set_keep_strongest; K <= max_pts),
    selected on the device before anything is described; counts are then the kept counts.
    second_orientation = ratio > 0 (0.8 is the reference's constant): every image's records are followed by a duplicate of
    each keypoint whose orientation histogram has a second peak above ratio x the first, at that orientation
    (cusift_ctx_set_second_orientation); counts include them, up to max_pts.
    cross_check = True: register_planar, register_epipolar, register_pose, register_planar_sequence and register_sequence feed their
    RANSAC mutual matches only (cusift_ctx_set_cross_check on this extractor's context).
    match_bits = 8: the same calls quantise their records and match the bytes on the int8 matrix pipe
    (cusift_ctx_set_match_bits on this extractor's context); 32, the default, matches the float descriptors.
    """

    def __init__(self, n_images, w, h, params=None, device=None, pitch=None, n_slots=1, keep_strongest=0,
                 cross_check=False, match_bits=32, second_orientation=0.0, **param_overrides):
        if not torch.cuda.is_available():
            raise capi.CusiftError("BatchExtractor needs a GPU (no CPU fallback)")
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.n, self.w, self.h = int(n_images), int(w), int(h)
        self.pitch = capi.ialign_up(self.w, 128) if pitch is None else int(pitch)
        self.params = params if params is not None else capi.default_params(**param_overrides)
        self.max_pts = self.params.max_pts
        self.keep_strongest = capi.check_keep_strongest(keep_strongest, self.max_pts)
        self.second_orientation = capi.check_second_orientation(second_orientation)
        self.cross_check = bool(capi.check_cross_check(cross_check))
        self.match_bits = capi.check_match_bits(match_bits)
        with torch.cuda.device(self.device):
            self.stream = torch.cuda.current_stream()
            self.ctx = capi.Context(self.device.index, stream=self.stream.cuda_stream)
            if self.keep_strongest:
                self.ctx.set_keep_strongest(self.keep_strongest)
            if self.second_orientation:
                self.ctx.set_second_orientation(self.second_orientation)
            if self.cross_check:
                self.ctx.set_cross_check(True)
            if self.match_bits != 32:
                self.ctx.set_match_bits(self.match_bits)
            self.ctx.reserve(self.n, self.w, self.h, self.params)
            # n_slots > 1: output ring, so that a consumer (D2H copy, all-gatherv on another stream) can still
            # read step i's SiftData while step i+1 is being extracted
            self.slots = [(torch.zeros((self.n, self.max_pts, capi.SIFT_POINT_BYTES), dtype=torch.uint8,
                                       device=self.device),
                           torch.zeros((self.n,), dtype=torch.int32, device=self.device)) for _ in range(n_slots)]
            self.points, self.counts = self.slots[0]

    def images_from_numpy(self, imgs):
        """(n, h, w) float32 host array -> pitched device tensor (n, h, pitch)."""
        imgs = np.asarray(imgs, dtype=np.float32)
        assert imgs.shape == (self.n, self.h, self.w), imgs.shape
        dev = torch.zeros((self.n, self.h, self.pitch), dtype=torch.float32, device=self.device)
        dev[:, :, : self.w] = torch.from_numpy(imgs).to(self.device)
        return dev

    def extract(self, d_imgs, slot=0):
        assert d_imgs.is_cuda and d_imgs.dtype == torch.float32 and d_imgs.is_contiguous()
        assert tuple(d_imgs.shape) == (self.n, self.h, self.pitch), tuple(d_imgs.shape)
        self.points, self.counts = self.slots[slot]
        self.ctx.extract_batch(d_imgs.data_ptr(), self.n, self.w, self.h, self.pitch, self.h * self.pitch,
                               self.params, self.points.data_ptr(), self.counts.data_ptr())
        return self.points, self.counts

    def describe(self, d_imgs, points=None, counts=None, slot=0, keep_orientation=False, octave_from_scale=False):
        """cusift_describe_batch: orientation + descriptor of the records as they stand, in place -- by default the
        slot's own tensors (what extract() left there, or what the caller wrote into them: coords2D and scale in image
        pixels).  points: uint8 [n, max_pts, 588] device tensor; counts: int32 [n] device tensor of its own, or None with
        `points` given: every image has max_pts records.  Only enqueues work; returns (points, counts)."""
        assert d_imgs.is_cuda and d_imgs.dtype == torch.float32 and d_imgs.is_contiguous()
        assert tuple(d_imgs.shape) == (self.n, self.h, self.pitch), tuple(d_imgs.shape)
        if points is None:
            points, own_counts = self.slots[slot]
            counts = own_counts if counts is None else counts
        assert points.is_cuda and points.dtype == torch.uint8 and points.is_contiguous()
        assert tuple(points.shape) == (self.n, self.max_pts, capi.SIFT_POINT_BYTES), tuple(points.shape)
        if counts is not None:
            assert counts.is_cuda and counts.dtype == torch.int32 and counts.is_contiguous() and counts.numel() == self.n
        flags = (capi.DESCRIBE_KEEP_ORIENTATION if keep_orientation else 0) | \
                (capi.DESCRIBE_OCTAVE_FROM_SCALE if octave_from_scale else 0)
        self.ctx.describe_batch(d_imgs.data_ptr(), self.n, self.w, self.h, self.pitch, self.h * self.pitch, self.params,
                                points.data_ptr(), counts.data_ptr() if counts is not None else None, flags)
        return points, counts

    def second_orientations(self, d_imgs, points=None, counts=None, slot=0, ratio=0.8, octave_from_scale=False):
        """cusift_second_orientations_batch: appends the second-peak duplicates behind the records as they stand -- by
        default the slot's own tensors (what extract() or describe() left there).  points: uint8 [n, max_pts, 588] device
        tensor; counts: int32 [n] device tensor, read and updated (required with `points` given).  Only enqueues work;
        returns (points, counts)."""
        assert d_imgs.is_cuda and d_imgs.dtype == torch.float32 and d_imgs.is_contiguous()
        assert tuple(d_imgs.shape) == (self.n, self.h, self.pitch), tuple(d_imgs.shape)
        if points is None:
            points, own_counts = self.slots[slot]
            counts = own_counts if counts is None else counts
        if counts is None:
            raise ValueError("second_orientations: counts is read and written, None given")
        assert points.is_cuda and points.dtype == torch.uint8 and points.is_contiguous()
        assert tuple(points.shape) == (self.n, self.max_pts, capi.SIFT_POINT_BYTES), tuple(points.shape)
        assert counts.is_cuda and counts.dtype == torch.int32 and counts.is_contiguous() and counts.numel() == self.n
        self.ctx.second_orientations(d_imgs.data_ptr(), self.n, self.w, self.h, self.pitch, self.h * self.pitch,
                                     self.params, points.data_ptr(), counts.data_ptr(), ratio,
                                     capi.DESCRIBE_OCTAVE_FROM_SCALE if octave_from_scale else 0)
        return points, counts

    def make_packer(self, stream=None):
        """A `packer(points, counts, max_pts)` for cusift_amd.dist.allgather_siftdata that runs cusift_pack_points on
        `stream` (a torch.cuda.Stream; default: this extractor's stream) through a context of its own that borrows
        that stream -- so the exchange of step i can be packed and sent on a side stream while step i+1 is extracted."""
        stream = self.stream if stream is None else stream
        ctx = self.ctx if stream == self.stream else capi.Context(self.device.index, stream=stream.cuda_stream)
        self._packer_ctxs = getattr(self, "_packer_ctxs", []) + [ctx]

        def packer(points, counts, max_pts, out=None):
            """Valid records of all images back to back.  out=None: returns (packed, valid counts) like
            cusift_amd.dist.pack_points (one host read-back for the size); out=<uint8 [total, 588] tensor of exactly
            the valid total>: packs into it, no read-back, returns None."""
            n = points.shape[0]
            if n > 256 or not points.is_cuda:  # kMaxFlatImages
                from .dist import pack_points
                packed, valid = pack_points(points, counts, max_pts)
                if out is None:
                    return packed, valid
                out.copy_(packed)
                return None
            with torch.cuda.stream(stream):
                if out is None:
                    valid = torch.clamp(counts, max=max_pts)
                    total = int(valid.sum().item())  # the one host read-back of the packing
                    out_t = torch.empty((total, capi.SIFT_POINT_BYTES), dtype=torch.uint8, device=points.device)
                else:
                    assert out.is_contiguous() and out.dtype == torch.uint8 and out.shape[1] == capi.SIFT_POINT_BYTES
                    out_t, total = out, out.shape[0]
                if total > 0:
                    ctx.pack_points(points.data_ptr(), counts.data_ptr(), n, max_pts, out_t.data_ptr(), total, None)
            return (out_t, valid) if out is None else None

        return packer

    def _pairs(self, pairs):
        return [(i, i + 1) for i in range(self.n - 1)] if pairs is None else pairs

    def _pair_counts(self, counts, i, j):
        n_i, n_j = torch.clamp(counts[[i, j]], max=self.max_pts).tolist()  # the one read-back of the counts
        return int(n_i), int(n_j)

    def _depth_layout(self, d_depth):
        """Checks a depth tensor [n, h, w'] of 16-bit samples; returns (pitch, image_stride) in samples."""
        assert d_depth.is_cuda and d_depth.element_size() == 2 and d_depth.is_contiguous()
        assert d_depth.dim() == 3 and d_depth.shape[0] == self.n and d_depth.shape[1] == self.h, tuple(d_depth.shape)
        assert d_depth.shape[2] >= self.w, tuple(d_depth.shape)
        return d_depth.shape[2], self.h * d_depth.shape[2]

    def register_sequence(self, d_depth, camera, pairs=None, slot=0, **ransac):
        """Registers the frames of the last extract() into `slot` against each other: cusift_register_rgbd_batch over
        this extractor's own device records and raw counters -- no count is read back, the frame counts never reach
        the host.  d_depth: int16 / uint16 device tensor [n, h, w'] (contiguous; w' >= w is the row pitch), one depth
        image per frame at base-image scale.  pairs: (frame 1, frame 2) rows; None: (i, i + 1) for every consecutive
        frame.  **ransac goes to capi.Context.register_rgbd_batch (loops, thresh2, kind, seed, distance, score_threshold,
        ambiguity_threshold).  Returns its tuple: (rt [P, 3, 4], num_matches [P], num_inliers [P], pairs list, flags
        list); capi.chain_poses(rt) turns the default pair list's result into per-frame poses.  Blocking."""
        pitch, image_stride = self._depth_layout(d_depth)
        points, counts = self.slots[slot]
        return self.ctx.register_rgbd_batch(points.data_ptr(), counts.data_ptr(), self.n, self.max_pts,
                                            d_depth.data_ptr(), self.w, self.h, camera, self._pairs(pairs),
                                            pitch=pitch, image_stride=image_stride, **ransac)

    def register_planar(self, i, j, slot=0, **opts):
        """Planar registration of frames i and j of the last extract() into `slot`: cusift_register_planar over this
        extractor's device records (frame i's match fields and match_error are written).  The two counts are read with
        one call.  **opts goes to capi.Context.register_planar (distance, rule, lo, hi, loops, thresh, refine_loops,
        refine_thresh, seed, want_all).  Returns its PlanarResult: homography maps frame i onto frame j.  Blocking."""
        points, counts = self.slots[slot]
        n_i, n_j = self._pair_counts(counts, i, j)
        return self.ctx.register_planar(points[i].data_ptr(), n_i, points[j].data_ptr(), n_j, **opts)

    def register_epipolar(self, i, j, slot=0, **opts):
        """Epipolar registration of frames i and j of the last extract() into `slot`: cusift_register_epipolar over this
        extractor's device records (frame i's match fields and match_error are written).  The two counts are read with
        one call.  **opts goes to capi.Context.register_epipolar (distance, rule, lo, hi, loops, thresh, refine_loops,
        refine_thresh, seed, want_all).  Returns its EpipolarResult: x_j^T F x_i = 0.  Blocking."""
        points, counts = self.slots[slot]
        n_i, n_j = self._pair_counts(counts, i, j)
        return self.ctx.register_epipolar(points[i].data_ptr(), n_i, points[j].data_ptr(), n_j, **opts)

    def match_guided(self, i, j, model, m, radius, slot=0, distance=1):
        """Guided match of frames i and j of the last extract() into `slot`: cusift_match_guided over this extractor's
        device records (frame i's match fields are written) -- frame j's records that fail `model` ("homography": x_j ~ m
        x_i; "epipolar": x_j^T m x_i = 0) by more than `radius` pixels cannot be a record's match.  The two counts are
        read with one call.  Asynchronous on the extractor's stream."""
        points, counts = self.slots[slot]
        n_i, n_j = self._pair_counts(counts, i, j)
        self.ctx.match_guided(points[i].data_ptr(), n_i, points[j].data_ptr(), n_j, model, m, radius, distance)

    def quantize(self, slot=0):
        """8-bit descriptors of the last extract() into `slot`: cusift_quantize_descriptors over this extractor's device
        records and raw counters.  Returns (uint8 [n, max_pts, 128], int32 [n, max_pts, 2]) device tensors, allocated once
        per slot: the bytes are the OpenCV / VLFeat / COLMAP convention (512 v clipped to 255) -- what a caller hands to
        them -- and the ints are (sum q, sum q^2), which match8() needs.  Rows past a frame's count keep what they held.
        Asynchronous on the extractor's stream."""
        if not hasattr(self, "_desc8"):
            self._desc8 = {}
        if slot not in self._desc8:
            with torch.cuda.device(self.device):
                self._desc8[slot] = (torch.zeros((self.n, self.max_pts, 128), dtype=torch.uint8, device=self.device),
                                     torch.zeros((self.n, self.max_pts, 2), dtype=torch.int32, device=self.device))
        q, sums = self._desc8[slot]
        points, counts = self.slots[slot]
        self.ctx.quantize_descriptors(points.data_ptr(), self.max_pts, q.data_ptr(), sums.data_ptr(), n_images=self.n,
                                      d_counters=counts.data_ptr())
        return q, sums

    def match8(self, i, j, slot=0, distance=1):
        """8-bit match of frames i and j of `slot` on the tensors of the last quantize(slot): cusift_match8 writes frame
        i's five match fields (exact integer scores scaled by 2^-18; int8 matrix pipe).  The two counts are read with one
        call.  Asynchronous on the extractor's stream."""
        if slot not in getattr(self, "_desc8", {}):
            raise capi.CusiftError("match8: call quantize(slot=%d) first" % slot)
        q, sums = self._desc8[slot]
        points, counts = self.slots[slot]
        n_i, n_j = self._pair_counts(counts, i, j)
        self.ctx.match8(points[i].data_ptr(), n_i, q[i].data_ptr(), sums[i].data_ptr(), points[j].data_ptr(), n_j,
                        q[j].data_ptr(), sums[j].data_ptr(), distance)

    def match8_mutual(self, i, j, slot=0, distance=1):
        """match8(i, j) and match8(j, i) from one pass, on the tensors of the last quantize(slot): cusift_match8_mutual
        writes the five match fields of both frames' records.  i == j is refused (both sets are written).  Asynchronous
        on the extractor's stream."""
        if slot not in getattr(self, "_desc8", {}):
            raise capi.CusiftError("match8_mutual: call quantize(slot=%d) first" % slot)
        q, sums = self._desc8[slot]
        points, counts = self.slots[slot]
        n_i, n_j = self._pair_counts(counts, i, j)
        self.ctx.match8_mutual(points[i].data_ptr(), n_i, q[i].data_ptr(), sums[i].data_ptr(), points[j].data_ptr(), n_j,
                               q[j].data_ptr(), sums[j].data_ptr(), distance)

    def _tables8(self, who, i, j, slot):
        """(records i, count, table, sums, records j, count, table, sums) of the last quantize(slot), as the 8-bit pair
        calls take them"""
        if slot not in getattr(self, "_desc8", {}):
            raise capi.CusiftError("%s: call quantize(slot=%d) first" % (who, slot))
        q, sums = self._desc8[slot]
        points, counts = self.slots[slot]
        n_i, n_j = self._pair_counts(counts, i, j)
        return (points[i].data_ptr(), n_i, q[i].data_ptr(), sums[i].data_ptr(), points[j].data_ptr(), n_j, q[j].data_ptr(),
                sums[j].data_ptr())

    def match8_guided(self, i, j, model, m, radius, slot=0, distance=1):
        """match_guided(i, j, model, m, radius) on the tensors of the last quantize(slot): cusift_match8_guided writes frame
        i's five match fields from the bytes, the test reads the records' coords2D.  Asynchronous on the extractor's
        stream."""
        self.ctx.match8_guided(*self._tables8("match8_guided", i, j, slot), model, m, radius, distance)

    def match8_projected(self, i, j, rt, camera2, radius, slot=0, distance=1):
        """match_projected(i, j, rt, camera2, radius) on the tensors of the last quantize(slot): cusift_match8_projected
        writes frame i's five match fields from the bytes, the test reads frame i's coords3D and frame j's coords2D.
        Asynchronous on the extractor's stream."""
        self.ctx.match8_projected(*self._tables8("match8_projected", i, j, slot), rt, camera2, radius, distance)

    def register_planar_guided(self, i, j, radius=None, slot=0, **opts):
        """register_planar(i, j) with a second, guided matching pass: capi.Context.register_planar_guided over this
        extractor's device records.  Returns its (first pass, guided pass).  Refused while cross_check is on; with
        match_bits = 8 it runs with match8=True among the options (the second pass on bytes too).  Blocking."""
        points, counts = self.slots[slot]
        n_i, n_j = self._pair_counts(counts, i, j)
        return self.ctx.register_planar_guided(points[i].data_ptr(), n_i, points[j].data_ptr(), n_j, radius, **opts)

    def register_epipolar_guided(self, i, j, radius=None, slot=0, **opts):
        """register_epipolar(i, j) with a second, guided matching pass: capi.Context.register_epipolar_guided over this
        extractor's device records.  Returns its (first pass, guided pass).  Refused while cross_check is on; with
        match_bits = 8 it runs with match8=True among the options (the second pass on bytes too).  Blocking."""
        points, counts = self.slots[slot]
        n_i, n_j = self._pair_counts(counts, i, j)
        return self.ctx.register_epipolar_guided(points[i].data_ptr(), n_i, points[j].data_ptr(), n_j, radius, **opts)

    def register_pose(self, i, j, camera, camera2=None, slot=0, **opts):
        """Calibrated two-view pose of frames i and j of the last extract() into `slot`: cusift_register_pose over this
        extractor's device records (frame i's match fields, match_error and coords3D are written).  camera: the
        capi.Camera of frame i, camera2 of frame j (None: the same).  The two counts are read with one call.  **opts goes
        to capi.Context.register_pose.  Returns its RegisterPoseResult: X_i = R X_j + t with |t| = 1.  Blocking."""
        points, counts = self.slots[slot]
        n_i, n_j = self._pair_counts(counts, i, j)
        return self.ctx.register_pose(points[i].data_ptr(), n_i, points[j].data_ptr(), n_j, camera, camera2, **opts)

    def register_pnp(self, i, j, camera2, slot=0, **opts):
        """Absolute pose of frame j of the last extract() into `slot` from frame i's coords3D (as lift_depth or an earlier
        register_pose(i, ...) wrote them): cusift_register_pnp over this extractor's device records (frame i's match
        fields and match_error are written, coords3D is not).  camera2: the capi.Camera of frame j.  The two counts are
        read with one call.  **opts goes to capi.Context.register_pnp.  Returns its PnPResult: X_i = R X_j + t, t in the
        unit of frame i's coords3D.  Blocking."""
        points, counts = self.slots[slot]
        n_i, n_j = self._pair_counts(counts, i, j)
        return self.ctx.register_pnp(points[i].data_ptr(), n_i, points[j].data_ptr(), n_j, camera2, **opts)

    def match_projected(self, i, j, rt, camera2, radius, slot=0, distance=1):
        """Match by projection of frames i and j of the last extract() into `slot`: cusift_match_projected over this
        extractor's device records (frame i's match fields are written, its coords3D read) -- a record of frame j counts
        for a record of frame i only within `radius` pixels of where rt (X_i = R X_j + t) and camera2, the capi.Camera of
        frame j, put that record's coords3D.  The two counts are read with one call.  Asynchronous on the extractor's
        stream."""
        points, counts = self.slots[slot]
        n_i, n_j = self._pair_counts(counts, i, j)
        self.ctx.match_projected(points[i].data_ptr(), n_i, points[j].data_ptr(), n_j, rt, camera2, radius, distance)

    def register_pnp_guided(self, i, j, camera2, radius=None, slot=0, **opts):
        """register_pnp(i, j, camera2) with a second matching pass by projection: capi.Context.register_pnp_guided over
        this extractor's device records.  Returns its (first pass, guided pass).  Refused while cross_check is on;
        with match_bits = 8 it runs with match8=True among the options (the second pass on bytes too).  Blocking."""
        points, counts = self.slots[slot]
        n_i, n_j = self._pair_counts(counts, i, j)
        return self.ctx.register_pnp_guided(points[i].data_ptr(), n_i, points[j].data_ptr(), n_j, camera2, radius, **opts)

    def register_planar_sequence(self, pairs=None, slot=0, **opts):
        """Planar registration of the frames of the last extract() into `slot` against each other:
        cusift_register_planar_batch over this extractor's own device records and raw counters -- no count is read
        back and the records are not written, so a frame may be the first member of any number of pairs.  pairs:
        (frame a, frame b) rows; None: (i, i + 1) for every consecutive frame.  **opts goes to
        capi.Context.register_planar_batch (distance, rule, lo, hi, loops, thresh, refine_loops, refine_thresh, seed,
        want_inliers, want_errors).  Returns its PlanarBatchResult: homography[p] maps frame a onto frame b;
        capi.chain_homographies(homography) turns the default pair list's result into per-frame maps into frame 0.
        Blocking."""
        points, counts = self.slots[slot]
        return self.ctx.register_planar_batch(points.data_ptr(), counts.data_ptr(), self.n, self.max_pts,
                                              self._pairs(pairs), **opts)

    def register_epipolar_sequence(self, pairs=None, slot=0, **opts):
        """Epipolar registration of the frames of the last extract() into `slot` against each other:
        cusift_register_epipolar_batch over this extractor's own device records and raw counters -- no count is read back
        and the records are not written.  pairs: (frame a, frame b) rows; None: (i, i + 1) for every consecutive frame.
        **opts goes to capi.Context.register_epipolar_batch.  Returns its EpipolarBatchResult: x_b^T F x_a = 0.
        Blocking."""
        points, counts = self.slots[slot]
        return self.ctx.register_epipolar_batch(points.data_ptr(), counts.data_ptr(), self.n, self.max_pts,
                                                self._pairs(pairs), **opts)

    def register_pose_sequence(self, camera, camera2=None, pairs=None, slot=0, **opts):
        """Calibrated two-view poses of the frames of the last extract() into `slot`: cusift_register_pose_batch over this
        extractor's own device records and raw counters, one pair of cameras for every pair of the list (camera2 None:
        the same camera).  The records are not written: want_points=True returns each pair's triangulated points.
        **opts goes to capi.Context.register_pose_batch.  Returns its PoseBatchResult: X_a = R X_b + t with |t| = 1 per
        pair -- capi.chain_poses does NOT apply to these poses, every pair has a scale of its own.  Blocking."""
        points, counts = self.slots[slot]
        return self.ctx.register_pose_batch(points.data_ptr(), counts.data_ptr(), self.n, self.max_pts,
                                            self._pairs(pairs), camera, camera2, **opts)

    def register_pnp_sequence(self, camera2, pairs=None, slot=0, d_depth=None, depth_camera=None, **opts):
        """Absolute poses of the frames of the last extract() into `slot`: cusift_register_pnp_batch over this extractor's
        own device records and raw counters.  camera2: the capi.Camera of every pair's frame b.  coords3D of the records
        is read and not written.  d_depth (int16 / uint16 device tensor [n, h, w'], as register_sequence takes it) with
        depth_camera (None: camera2): one cusift_lift_depth over the whole batch is enqueued on the same stream first --
        an RGB-D sequence registered by reprojection error, where only frame a of each pair needs depth (register_sequence
        needs both).  **opts goes to capi.Context.register_pnp_batch.  Returns its PnPBatchResult: X_a = R X_b + t in the
        unit of coords3D, metric after a lift, so capi.chain_poses(rt) turns the default pair list's result into
        per-frame poses.  Blocking."""
        points, counts = self.slots[slot]
        if d_depth is not None:
            pitch, image_stride = self._depth_layout(d_depth)
            self.ctx.lift_depth(points.data_ptr(), self.max_pts, d_depth.data_ptr(), self.w, self.h,
                                camera2 if depth_camera is None else depth_camera, pitch=pitch, n_images=self.n,
                                d_counters=counts.data_ptr(), image_stride=image_stride)
        return self.ctx.register_pnp_batch(points.data_ptr(), counts.data_ptr(), self.n, self.max_pts,
                                           self._pairs(pairs), camera2, **opts)

    def build_tracks(self, pairs=None, slot=0, mutual=True, inliers=None, rule=1, lo=None, hi=None, min_views=2,
                     distance=1, match_bits=None):
        """Feature tracks of the frames of the last extract() into `slot`: the pair-list matcher (match_batch_mutual, or
        match_batch with mutual=False; the 8-bit matchers on quantize(slot)'s tables when match_bits, by default this
        extractor's, is 8) and cusift_build_tracks behind it on the same stream.  pairs: (frame a, frame b) rows; None:
        (i, i + 1) for every consecutive frame.  inliers: [P, max_pts] flags, or one array per pair as a
        PlanarBatchResult's `inliers` -- only rows flagged there can be edges.  rule / lo / hi: the match filter of the
        registrations (capi.Context.build_tracks).  Returns a Tracks of device tensors; nothing is read back."""
        pairs = capi.pair_list(self._pairs(pairs))
        bits = self.match_bits if match_bits is None else capi.check_match_bits(match_bits)
        points, counts = self.slots[slot]
        n_pairs, n_nodes = len(pairs), self.n * self.max_pts
        with torch.cuda.device(self.device), torch.cuda.stream(self.stream):
            rows = torch.zeros((n_pairs, self.max_pts, 4), dtype=torch.int32, device=self.device)
            rows_back = torch.zeros_like(rows) if mutual else None
            keep = None
            if inliers is not None:
                flags = np.zeros((n_pairs, self.max_pts), dtype=np.uint8)
                for p, row in enumerate(inliers):
                    row = np.asarray(row).reshape(-1)
                    flags[p, : len(row)] = row != 0
                keep = torch.from_numpy(flags).to(self.device)
            track = torch.empty((self.n, self.max_pts), dtype=torch.int32, device=self.device)
            offsets = torch.zeros((n_nodes // 2 + 1,), dtype=torch.int32, device=self.device)
            obs = torch.zeros((max(n_nodes, 1),), dtype=torch.int32, device=self.device)
            stats = torch.zeros((8,), dtype=torch.int32, device=self.device)
            back = rows_back.data_ptr() if mutual else None
            if bits == 8:
                q, sums = self.quantize(slot)
                if mutual:
                    self.ctx.match8_batch_mutual(q.data_ptr(), sums.data_ptr(), counts.data_ptr(), self.n, self.max_pts,
                                                 pairs, rows.data_ptr(), back, distance)
                else:
                    self.ctx.match8_batch(q.data_ptr(), sums.data_ptr(), counts.data_ptr(), self.n, self.max_pts, pairs,
                                          rows.data_ptr(), distance)
            elif mutual:
                self.ctx.match_batch_mutual(points.data_ptr(), counts.data_ptr(), self.n, self.max_pts, pairs,
                                            rows.data_ptr(), back, distance)
            else:
                self.ctx.match_batch(points.data_ptr(), counts.data_ptr(), self.n, self.max_pts, pairs, rows.data_ptr(),
                                     distance)
            self.ctx.build_tracks(counts.data_ptr(), self.n, self.max_pts, pairs, rows.data_ptr(), track.data_ptr(),
                                  offsets.data_ptr(), obs.data_ptr(), stats.data_ptr(), d_rows_back=back,
                                  d_keep=keep.data_ptr() if keep is not None else None, rule=rule, lo=lo, hi=hi,
                                  min_views=min_views)
        return Tracks(self.n, self.max_pts, pairs, track, offsets, obs, stats, rows, rows_back, keep)

    def triangulate_tracks(self, tracks, poses, camera, min_pivot=1e-12, slot=0):
        """The 3-D point of every track of build_tracks() from all its views: cusift_triangulate_tracks over the records
        of `slot`.  poses: capi.chain_poses' [n, 4, 4] or [n, 3, 4], camera to world; camera: one capi.Camera for all
        frames.  Returns device tensors points3d float64 [cap, 4] = (X, Y, Z, largest reprojection error in pixels) and
        front int32 [cap] with cap = n * max_pts // 2; rows at and past the track count stay zero, and so does a
        degenerate track (min_pivot: capi.Context.triangulate_tracks).  Nothing is read back."""
        points, _ = self.slots[slot]
        cap = tracks.offsets.numel() - 1
        with torch.cuda.device(self.device), torch.cuda.stream(self.stream):
            points3d = torch.zeros((cap, 4), dtype=torch.float64, device=self.device)
            front = torch.zeros((cap,), dtype=torch.int32, device=self.device)
            self.ctx.triangulate_tracks(points.data_ptr(), self.n, self.max_pts, tracks.offsets.data_ptr(),
                                        tracks.obs.data_ptr(), tracks.stats.data_ptr(), cap, poses, camera,
                                        points3d.data_ptr(), front.data_ptr(), min_pivot=min_pivot)
        return points3d, front

    def bundle_adjust(self, tracks, poses, camera, points3d, fixed=None, slot=0, **params):
        """Refines the poses and the points of triangulate_tracks() together: cusift_bundle_adjust over the records of
        `slot`, Schur-complement Levenberg-Marquardt with every decision on the device.  poses: capi.chain_poses'
        [n, 4, 4] or [n, 3, 4], camera to world; points3d: triangulate_tracks' tensor (read, not written: the result
        has its own copy); fixed: flags of the frames that must not move (None: frame 0); params: the fields of
        capi.BundleParams (iterations, lam, lambda_min, lambda_max, huber, max_error, min_decrease).  Returns a
        BundleResult of device tensors; nothing is read back."""
        points, _ = self.slots[slot]
        cap = tracks.offsets.numel() - 1
        par = capi.BundleParams(**params)
        with torch.cuda.device(self.device), torch.cuda.stream(self.stream):
            out = points3d.to(dtype=torch.float64, copy=True).contiguous()
            if out.numel() != 4 * cap:
                raise ValueError("bundle_adjust: points3d has %d entries, the tracks take [%d, 4]" % (out.numel(), cap))
            d_poses = torch.zeros((self.n, 12), dtype=torch.float64, device=self.device)
            history = torch.zeros((par.iterations, 4), dtype=torch.float64, device=self.device)
            summary = torch.zeros((8,), dtype=torch.float64, device=self.device)
            self.ctx.bundle_adjust(points.data_ptr(), self.n, self.max_pts, tracks.offsets.data_ptr(),
                                   tracks.obs.data_ptr(), tracks.stats.data_ptr(), cap, poses, camera, out.data_ptr(),
                                   d_poses.data_ptr(), history.data_ptr(), summary.data_ptr(), fixed=fixed, params=par)
        return BundleResult(d_poses, out, history, summary)

    def valid_counts(self):
        return torch.clamp(self.counts, max=self.max_pts)

    def to_host(self):
        """Blocking: list of numpy SiftPoint arrays, one per image."""
        cnt = self.valid_counts().cpu().numpy()
        out = []
        for i in range(self.n):
            raw = self.points[i, : int(cnt[i])].cpu().numpy()
            out.append(raw.view(capi.SIFT_POINT_DTYPE).reshape(-1))
        return out

    def close(self):
        self.ctx.close()


class PipelinedExtractor:
    """Consecutive batches on `n_streams` HIP streams, one BatchExtractor (context, arena, output slots) each.

    A single launch sequence leaves the chip part-idle at times: the ScaleDown chain is HBM-bound while everything
    else is VALU-bound, and the last waves of every detection / description launch run on a nearly empty device.
    With several batches in flight those gaps are filled by the other batches' kernels, and the detection can use tall
    row chunks (cusift_params.concurrent_batches, set here to the stream count).  64 x 1080p on MI355X: 1.64 ms per
    batch on one stream, 1.44 on two, 1.41 on four (1.38 with the chunk hint).  Results are those of BatchExtractor.

        pipe = PipelinedExtractor(64, 1920, 1080, n_streams=4, num_octaves=5, init_blur=1.0, peak_thresh=3.0)
        for frames in source:                       # frames: float32 device tensor [n, h, pitch]
            points, counts, done = pipe.submit(frames)
            ...                                     # consume after `done` (an event) -- e.g. other_stream.wait_event(done)
    The output tensors of a submit are reused by the submit `n_streams * n_slots` calls later.
    """

    def __init__(self, n_images, w, h, n_streams=4, n_slots=1, device=None, **kw):
        if not torch.cuda.is_available():
            raise capi.CusiftError("PipelinedExtractor needs a GPU (no CPU fallback)")
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        with torch.cuda.device(self.device):
            self.streams = [torch.cuda.current_stream()] + [torch.cuda.Stream() for _ in range(max(1, n_streams) - 1)]
            kw.setdefault("concurrent_batches", len(self.streams))  # scheduling hint: other batches fill launch tails
            self.extractors = []
            for st in self.streams:
                with torch.cuda.stream(st):
                    self.extractors.append(BatchExtractor(n_images, w, h, n_slots=n_slots, device=self.device, **kw))
        self.n_slots = n_slots
        self.submitted = 0
        first = self.extractors[0]
        self.n, self.w, self.h, self.pitch, self.max_pts, self.params = (first.n, first.w, first.h, first.pitch,
                                                                         first.max_pts, first.params)

    def images_from_numpy(self, imgs):
        return self.extractors[0].images_from_numpy(imgs)

    def submit(self, d_imgs, ready=None):
        """Enqueue one batch on the next stream.  `ready`: an event after which d_imgs may be read (None: the caller
        has made sure already, e.g. by a device synchronisation after the upload).
        Returns (points, counts, done_event)."""
        k = self.submitted
        self.submitted += 1
        e = k % len(self.streams)
        st = self.streams[e]
        with torch.cuda.stream(st):
            if ready is not None:
                st.wait_event(ready)
            pts, cnt = self.extractors[e].extract(d_imgs, slot=(k // len(self.streams)) % self.n_slots)
            done = torch.cuda.Event()
            done.record(st)
        return pts, cnt, done

    def synchronize(self):
        for st in self.streams:
            st.synchronize()

    def close(self):
        for x in self.extractors:
            x.close()
