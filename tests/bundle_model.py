"""cusift_bundle_adjust restated in numpy: the definition of include/cusift_amd_extras.h, every expression in float64 and
in the header's order.  Sums whose order the header pins are taken in that order: a track's members in d_obs order from
0, a frame's records and the tracks' costs as 256 strided partials and a halving tree, the factorisation column by column.
Everything per observation is evaluated for all nodes at once (element-wise numpy keeps the order of an expression)."""
import functools

import numpy as np

f64 = np.float64
DEFAULTS = dict(iterations=10, lam=1e-3, lambda_min=1e-9, lambda_max=1e6, huber=0.0, max_error=0.0, min_decrease=1e-12)


def strided_tree_sum(terms):
    """terms [m, ...] (zeros where nothing is summed) -> [...]: partial k = terms[k] + terms[k + 256] + ... from 0 in
    ascending order, then partial[k] += partial[k + h] for h = 128, 64 .. 1."""
    terms = np.asarray(terms, dtype=f64)
    m = terms.shape[0]
    pad = (-m) % 256
    if pad or m == 0:
        terms = np.concatenate([terms, np.zeros((pad if m else 256,) + terms.shape[1:])])
    chunks = terms.reshape((-1, 256) + terms.shape[1:])
    part = np.zeros(chunks.shape[1:])
    for ch in chunks:
        part = part + ch
    h = 128
    while h >= 1:
        part = part[:h] + part[h:2 * h]
        h //= 2
    return part[0]


def rodrigues(w):
    """Exp(w) as sift_pnp.hip's refit writes it."""
    w0, w1, w2 = (f64(v) for v in w)
    th2 = (w0 * w0 + w1 * w1) + w2 * w2
    th = np.sqrt(th2)
    tiny = th2 < 1e-20
    A = f64(1.0) if tiny else np.sin(th) / th
    B = f64(0.5) if tiny else (1.0 - np.cos(th)) / th2
    return np.array([[1.0 - B * (w1 * w1 + w2 * w2), B * (w0 * w1) - A * w2, B * (w0 * w2) + A * w1],
                     [B * (w0 * w1) + A * w2, 1.0 - B * (w0 * w0 + w2 * w2), B * (w1 * w2) - A * w0],
                     [B * (w0 * w2) - A * w1, B * (w1 * w2) + A * w0, 1.0 - B * (w0 * w0 + w1 * w1)]], dtype=f64)


class _Problem:
    def __init__(self, xy, max_pts, offsets, obs, fx, fy, cx, cy, origin, huber):
        self.fx, self.fy = f64(np.float32(fx)), f64(np.float32(fy))
        self.px = f64(np.float32(cx)) - f64(np.float32(origin))
        self.py = f64(np.float32(cy)) - f64(np.float32(origin))
        self.huber = f64(huber)
        self.max_pts = max_pts
        xy = np.asarray(xy, dtype=np.float32).reshape(-1, 2)
        self.x, self.y = xy[:, 0].astype(f64), xy[:, 1].astype(f64)
        self.offsets, self.obs = np.asarray(offsets, dtype=np.int64), np.asarray(obs, dtype=np.int64)

    def residuals(self, poses, X, nodes, tracks):
        """(c [m, 3], r0, r1, err2) of the observations (nodes[k], tracks[k])."""
        P = poses[nodes // self.max_pts]
        R, tr = P[:, :, :3], P[:, :, 3]
        e = X[tracks] - tr
        c = np.stack([(R[:, 0, j] * e[:, 0] + R[:, 1, j] * e[:, 1]) + R[:, 2, j] * e[:, 2] for j in range(3)], axis=1)
        q0, q1 = c[:, 0] / c[:, 2], c[:, 1] / c[:, 2]
        r0, r1 = (self.fx * q0 + self.px) - self.x[nodes], (self.fy * q1 + self.py) - self.y[nodes]
        return c, R, q0, q1, r0, r1, r0 * r0 + r1 * r1

    def rho(self, err2):
        if self.huber == 0.0:
            return err2
        h = self.huber
        return np.where(err2 <= h * h, err2, (2.0 * h) * np.sqrt(err2) - h * h)

    def jacobians(self, poses, X, nodes, tracks):
        """r [m, 2], w [m], JX [m, 2, 3], Jc [m, 2, 6] at (poses, X)."""
        c, R, q0, q1, r0, r1, err2 = self.residuals(poses, X, nodes, tracks)
        h = self.huber
        w = np.ones(len(nodes)) if h == 0.0 else np.where(err2 <= h * h, 1.0, h / np.sqrt(err2))
        a0, a1 = self.fx / c[:, 2], self.fy / c[:, 2]
        b0, b1 = 0.0 - a0 * q0, 0.0 - a1 * q1
        JX = np.zeros((len(nodes), 2, 3))
        for k in range(3):
            JX[:, 0, k] = a0 * R[:, k, 0] + b0 * R[:, k, 2]
            JX[:, 1, k] = a1 * R[:, k, 1] + b1 * R[:, k, 2]
        Jc = np.zeros((len(nodes), 2, 6))
        Jc[:, 0, 0], Jc[:, 0, 1], Jc[:, 0, 2] = 0.0 - b0 * c[:, 1], b0 * c[:, 0] - a0 * c[:, 2], a0 * c[:, 1]
        Jc[:, 1, 0], Jc[:, 1, 1], Jc[:, 1, 2] = a1 * c[:, 2] - b1 * c[:, 1], b1 * c[:, 0], 0.0 - a1 * c[:, 0]
        Jc[:, :, 3:] = 0.0 - JX
        return np.stack([r0, r1], axis=1), w, JX, Jc


def _member_sum(terms, first, length):
    """terms [E, ...] per observation slot (zeros where unused), tracks at first[t] .. first[t] + length[t]: the sum over
    a track's members in d_obs order, from 0."""
    out = np.zeros((len(first),) + terms.shape[1:])
    for m in range(int(length.max()) if len(length) else 0):
        has = length > m
        out[has] = out[has] + terms[first[has] + m]
    return out


def bundle_model(xy, max_pts, offsets, obs, poses, fx, fy, cx, cy, points3d, origin=0.0, fixed=None, n_tracks=None,
                 **params):
    """xy float32 [n, max_pts, 2]; poses [n, 3, 4] camera to world; points3d [>= T, 4] (the input rows).  Returns a dict:
    poses [n, 3, 4], points3d [T, 4], history [iterations, 4], summary [8], used (bool per track), used_obs, held, and
    two diagnostics: causes, one record per iteration that ran -- sfail (a Cholesky pivot failed), vfail (used tracks
    whose 3 x 3 pivot test failed), behind (used observations with c2 <= 0 at the trial), pivot (column, value, S[j][j]
    of the first failed Cholesky pivot or None) -- and, with keep_system=True, systems: (S, rhs, step) per iteration."""
    p = dict(DEFAULTS, **params)
    iterations, lam = int(p["iterations"]), f64(p["lam"])
    poses = np.array(poses, dtype=f64).reshape(-1, 3, 4)
    n = len(poses)
    T = len(offsets) - 1 if n_tracks is None else n_tracks
    offsets, obs = np.asarray(offsets, dtype=np.int64)[: T + 1], np.asarray(obs, dtype=np.int64)
    rows = np.array(points3d, dtype=f64)[:T].reshape(T, 4)
    pr = _Problem(xy, max_pts, offsets, obs, fx, fy, cx, cy, origin, p["huber"])
    E = int(offsets[T]) if T else 0
    nodes, first, length = obs[:E], offsets[:T], np.diff(offsets)
    slot_track = np.repeat(np.arange(T), length)
    N = n * max_pts
    history, summary = np.zeros((iterations, 4)), np.zeros(8)
    with np.errstate(all="ignore"):
        # ---- entry: which observations are used
        X = rows[:, :3].copy()
        c, _, _, _, _, _, err2 = pr.residuals(poses, X, nodes, slot_track)
        ok = (c[:, 2] > 0.0) & (err2 < np.inf)
        if p["max_error"] > 0.0:
            ok &= np.sqrt(err2) <= f64(p["max_error"])
        finite = np.isfinite(pr.x[nodes]) & np.isfinite(pr.y[nodes])
        alive = ~(rows == 0.0).all(axis=1)
        for t in range(T):
            s = slice(first[t], first[t] + length[t])
            if not (alive[t] and finite[s].all() and ok[s].sum() >= 2):
                ok[s] = False
        used_track = np.zeros(T, dtype=bool)
        used_track[slot_track[ok]] = True
        node_track = np.full(N, -1, dtype=np.int64)
        node_track[nodes[ok]] = slot_track[ok]
        frame_used = np.zeros(n, dtype=np.int64)
        np.add.at(frame_used, nodes[ok] // max_pts, 1)
        held = frame_used == 0
        if fixed is None:
            held[0] = True
        else:
            held |= np.asarray(fixed).astype(bool)
        un, ut = nodes[ok], slot_track[ok]  # the used observations, in d_obs order
        # member[t, f]: the used node of track t in frame f, -1: none
        member = np.full((T, n), -1, dtype=np.int64)
        member[ut, un // max_pts] = un

        def per_slot(values):  # values of the used observations -> every slot of d_obs, zeros elsewhere
            out = np.zeros((E,) + values.shape[1:])
            out[ok] = values
            return out

        def total_cost(poses_, X_, extra_inf=None):
            c_, _, _, _, _, _, e2 = pr.residuals(poses_, X_, un, ut)
            tc = _member_sum(per_slot(pr.rho(e2)), first, length)
            bad = _member_sum(per_slot((~(c_[:, 2] > 0.0)).astype(f64)), first, length) > 0
            if extra_inf is not None:
                bad |= extra_inf
            tc[bad | ~(tc < np.inf)] = np.inf
            tc[~used_track] = 0.0
            return strided_tree_sum(tc)

        cost = total_cost(poses, X) if T else f64(0.0)
        entry_cost, accepted, ran, stopped = cost, 0, 0, not used_track.any()  # no used track: stopped at entry
        causes, systems = [], []  # diagnostics for the tests: why a trial was infinite; the reduced systems on request
        for k in range(iterations):
            if stopped:
                history[k] = (cost, cost, lam, 2.0)
                continue
            ran += 1
            r, w, JX, Jc = pr.jacobians(poses, X, un, ut)
            # ---- per track: V, g, the damped inverse
            Vt = np.zeros((len(un), 3, 3))
            for i in range(3):
                for j in range(3):
                    Vt[:, i, j] = w * (JX[:, 0, i] * JX[:, 0, j] + JX[:, 1, i] * JX[:, 1, j])
            gt_t = np.stack([w * (JX[:, 0, i] * r[:, 0] + JX[:, 1, i] * r[:, 1]) for i in range(3)], axis=1)
            V, gt = _member_sum(per_slot(Vt), first, length), _member_sum(per_slot(gt_t), first, length)
            v00, v11, v22 = (V[:, i, i] + lam * V[:, i, i] for i in range(3))
            v10, v20, v21 = V[:, 1, 0], V[:, 2, 0], V[:, 2, 1]
            c00, c10, c20 = v11 * v22 - v21 * v21, v21 * v20 - v10 * v22, v10 * v21 - v11 * v20
            det = (v00 * c00 + v10 * c10) + v20 * c20
            c11, c21, c22 = v00 * v22 - v20 * v20, v10 * v20 - v00 * v21, v00 * v11 - v10 * v10
            vfail = used_track & ~((v00 > 0.0) & (c22 > 0.0) & (det > 0.0) & (det < np.inf))
            Vi = np.zeros((T, 3, 3))
            Vi[:, 0, 0], Vi[:, 1, 1], Vi[:, 2, 2] = c00 / det, c11 / det, c22 / det
            Vi[:, 1, 0] = Vi[:, 0, 1] = c10 / det
            Vi[:, 2, 0] = Vi[:, 0, 2] = c20 / det
            Vi[:, 2, 1] = Vi[:, 1, 2] = c21 / det
            # ---- per observation: W, Y = W V^-1, and the frame terms, laid out by node
            W = np.zeros((len(un), 6, 3))
            for a in range(6):
                for kk in range(3):
                    W[:, a, kk] = w * (Jc[:, 0, a] * JX[:, 0, kk] + Jc[:, 1, a] * JX[:, 1, kk])
            vi = Vi[ut]
            Y = np.zeros((len(un), 6, 3))
            for a in range(6):
                for kk in range(3):
                    Y[:, a, kk] = (W[:, a, 0] * vi[:, 0, kk] + W[:, a, 1] * vi[:, 1, kk]) + W[:, a, 2] * vi[:, 2, kk]
            g = gt[ut]
            Ut = np.zeros((len(un), 6, 6))
            for a in range(6):
                for b in range(6):
                    Ut[:, a, b] = w * (Jc[:, 0, a] * Jc[:, 0, b] + Jc[:, 1, a] * Jc[:, 1, b])
            gf_t = np.stack([w * (Jc[:, 0, a] * r[:, 0] + Jc[:, 1, a] * r[:, 1]) for a in range(6)], axis=1)
            ef_t = np.stack([(Y[:, a, 0] * g[:, 0] + Y[:, a, 1] * g[:, 1]) + Y[:, a, 2] * g[:, 2] for a in range(6)], axis=1)
            slot_of_node = np.full(N, -1, dtype=np.int64)
            slot_of_node[un] = np.arange(len(un))
            M = 6 * n
            S, rhs = np.zeros((M, M)), np.zeros(M)
            for f in range(n):
                if held[f]:
                    S[6 * f:6 * f + 6, 6 * f:6 * f + 6] = np.eye(6)
                    continue
                fs = slot_of_node[f * max_pts:(f + 1) * max_pts]  # by record: the used-observation index or -1
                on = fs >= 0

                def by_record(values):
                    out = np.zeros((max_pts,) + values.shape[1:])
                    out[on] = values[fs[on]]
                    return out

                U, gf, ef = (strided_tree_sum(by_record(v)) for v in (Ut, gf_t, ef_t))
                for gg in range(f, n):
                    if held[gg]:
                        continue
                    other = np.full(max_pts, -1, dtype=np.int64)
                    other[on] = member[ut[fs[on]], gg]
                    both = other >= 0
                    Et = np.zeros((max_pts, 6, 6))
                    if both.any():
                        Yf, Wg = Y[fs[both]], W[slot_of_node[other[both]]]
                        for a in range(6):
                            for b in range(6):
                                Et[both, a, b] = (Yf[:, a, 0] * Wg[:, b, 0] + Yf[:, a, 1] * Wg[:, b, 1]) + Yf[:, a, 2] * Wg[:, b, 2]
                    Efg = strided_tree_sum(Et)
                    if gg == f:
                        D = U.copy()
                        for a in range(6):
                            D[a, a] = U[a, a] + lam * U[a, a]
                        S[6 * f:6 * f + 6, 6 * f:6 * f + 6] = D - Efg
                    else:
                        S[6 * f:6 * f + 6, 6 * gg:6 * gg + 6] = 0.0 - Efg
                        S[6 * gg:6 * gg + 6, 6 * f:6 * f + 6] = (0.0 - Efg).T
                rhs[6 * f:6 * f + 6] = ef - gf
            # ---- Cholesky, column by column, every sum from k = 0 ascending; then L y = rhs and L^T x = y
            L, sfail, pivot = np.zeros((M, M)), False, None
            for j in range(M):
                acc = S[j:, j].copy()
                for kk in range(j):
                    acc = acc - L[j:, kk] * L[j, kk]
                if not (acc[0] > 0.0 and acc[0] < np.inf):
                    if not sfail:
                        pivot = (j, float(acc[0]), float(S[j, j]))
                    sfail = True
                d = np.sqrt(acc[0])
                L[j, j] = d
                L[j + 1:, j] = acc[1:] / d
            yv = rhs.copy()
            for j in range(M):
                yv[j] = yv[j] / L[j, j]
                yv[j + 1:] = yv[j + 1:] - L[j + 1:, j] * yv[j]
            for j in range(M - 1, -1, -1):
                yv[j] = yv[j] / L[j, j]
                yv[:j] = yv[:j] - L[j, :j] * yv[j]
            delta = yv.reshape(n, 6)
            trial_poses = poses.copy()
            for f in range(n):
                if held[f]:
                    continue
                Ex, R = rodrigues(delta[f, :3]), poses[f, :, :3]
                for i in range(3):
                    for j in range(3):
                        trial_poses[f, i, j] = (R[i, 0] * Ex[0, j] + R[i, 1] * Ex[1, j]) + R[i, 2] * Ex[2, j]
                    trial_poses[f, i, 3] = poses[f, i, 3] + delta[f, 3 + i]
            # ---- back-substitution and the trial cost
            dl = delta[un // max_pts]
            z = np.zeros((len(un), 3))
            for kk in range(3):
                acc = W[:, 0, kk] * dl[:, 0] + W[:, 1, kk] * dl[:, 1]
                for a in range(2, 6):
                    acc = acc + W[:, a, kk] * dl[:, a]
                z[:, kk] = acc
            s = gt + _member_sum(per_slot(z), first, length)
            dX = np.stack([0.0 - ((Vi[:, i, 0] * s[:, 0] + Vi[:, i, 1] * s[:, 1]) + Vi[:, i, 2] * s[:, 2]) for i in range(3)],
                          axis=1)
            trial_X = X.copy()
            trial_X[used_track] = X[used_track] + dX[used_track]
            trial = total_cost(trial_poses, trial_X, vfail)
            if sfail or not (trial < np.inf):
                trial = f64(np.inf)
            c_trial = pr.residuals(trial_poses, trial_X, un, ut)[0]
            causes.append(dict(sfail=bool(sfail), vfail=int(vfail.sum()), behind=int((c_trial[:, 2] <= 0.0).sum()),
                               pivot=pivot))
            if p.get("keep_system"):
                systems.append((S, rhs, yv.copy()))
            # ---- the decision
            if trial < cost:
                gain = (cost - trial) / cost
                history[k] = (cost, trial, lam, 1.0)
                poses, X, cost, accepted = trial_poses, trial_X, trial, accepted + 1
                lam = max(lam / 10.0, f64(p["lambda_min"]))
                if gain <= p["min_decrease"]:
                    stopped = True
            else:
                history[k] = (cost, trial, lam, 0.0)
                lam = 10.0 * lam
                if lam > p["lambda_max"]:
                    stopped = True
        # ---- outputs
        out = rows.copy()
        if T:
            _, _, _, _, _, _, e2 = pr.residuals(poses, X, un, ut)
            worst = np.zeros(T)
            for m in range(int(length.max())):
                has = length > m
                cand = per_slot(e2)[first[has] + m]
                cur = worst[has]
                worst[has] = np.where(cand > cur, cand, cur)
            out[used_track, :3] = X[used_track]
            out[used_track, 3] = np.sqrt(worst[used_track])
        summary[:] = (entry_cost, cost, accepted, ran, used_track.sum(), ok.sum(), (~held).sum(), lam)
    return dict(poses=poses, points3d=out, history=history, summary=summary, used=used_track, used_obs=ok, held=held,
                causes=causes, systems=systems)


def perturbed(poses, rot_sigma, trans_sigma, frames, seed=5):
    """poses with R <- R Exp(N(0, rot_sigma)) and t <- t + N(0, trans_sigma) on `frames`."""
    rng = np.random.default_rng(seed)
    out = np.array(poses, dtype=f64)
    for f in frames:
        out[f, :, :3] = out[f, :, :3] @ rodrigues(rng.normal(0.0, rot_sigma, 3))
        out[f, :, 3] += rng.normal(0.0, trans_sigma, 3)
    return out


def draw_tracks(n_tracks, n_cams, max_pts, max_views, seed=4):
    """Track t is record t of 2 .. max_views of the first n_cams frames, drawn as tests/test_triangulate_tracks.py does."""
    rng = np.random.default_rng(seed)
    offsets, obs = [0], []
    for t in range(n_tracks):
        frames = sorted(rng.choice(n_cams, size=int(rng.integers(2, max_views + 1)), replace=False).tolist())
        obs += [f * max_pts + t for f in frames]
        offsets.append(len(obs))
    return np.asarray(offsets, np.int32), np.asarray(obs, np.int32)


def planted_scene(n_tracks, n_cams, max_views, extra_frames, scene_seed, rot_sigma, trans_sigma):
    """The planted scene of the bundle tests: six_camera_scene plus `extra_frames` frames no track touches (frame 0's
    pose again), frames 1 .. n_cams - 1 perturbed, the entry points triangulated under the perturbed poses.  Returns a
    dict: xy float32 [n, max_pts, 2], max_pts, offsets, obs, true_poses, planted, poses (the start), points (the start,
    [T, 4]), cam."""
    from tracks_model import six_camera_scene, triangulate_model

    true6, planted, pixels, cam = six_camera_scene(n_tracks, seed=scene_seed, n_cams=n_cams)
    n, max_pts = n_cams + extra_frames, n_tracks + 8
    true_poses = np.concatenate([true6] + [true6[:1]] * extra_frames)
    xy = np.zeros((n, max_pts, 2), np.float32)
    xy[:n_cams, :n_tracks] = pixels
    offsets, obs = draw_tracks(n_tracks, n_cams, max_pts, max_views)
    poses = perturbed(true_poses, rot_sigma, trans_sigma, range(1, n_cams))
    points, _ = triangulate_model(xy, max_pts, offsets, obs, poses, *cam)
    return dict(xy=xy, max_pts=max_pts, offsets=offsets, obs=obs, true_poses=true_poses, planted=planted, poses=poses,
                points=points, cam=cam, n=n)


@functools.lru_cache(maxsize=None)
def scene_a():
    """Scene A: 800 tracks of 2 .. 6 views over six cameras and a seventh frame without observations, max_pts 808;
    frames 1 .. 5 start 0.01 rad and 0.02 units off.  Shared: treat it as read-only."""
    return planted_scene(800, 6, 6, 1, 21, 0.01, 0.02)


FAR_SEED = 28  # of the perturbation seeds 0 .. 39 tried, one whose first Gauss-Newton steps throw points behind cameras


@functools.lru_cache(maxsize=None)
def scene_a_far():
    """Scene A from 0.05 rad and 0.2 units off, the entry points triangulated under those poses."""
    from tracks_model import triangulate_model

    sc = dict(scene_a())
    sc["poses"] = perturbed(sc["true_poses"], 0.05, 0.2, range(1, 6), seed=FAR_SEED)
    sc["points"], _ = triangulate_model(sc["xy"], sc["max_pts"], sc["offsets"], sc["obs"], sc["poses"], *sc["cam"])
    return sc


@functools.lru_cache(maxsize=None)
def scene_a_gated():
    """Scene A with every kind of unused track, for max_error = 20: track 5's input row four zeros; a NaN pixel in track
    7; `gate3`, a track of three or more views with one pixel moved 50 px (it keeps two or more); `gate2`, a two-view
    track with one pixel moved 50 px (it keeps one: unused).  The moved pixels are gross outliers for huber = 1 without
    the gate.  Returns (scene, dict of the named tracks and the two cut observation slots)."""
    base = scene_a()
    views = np.diff(base["offsets"])
    who = dict(zero=5, nan=7, gate3=int(np.where(views >= 3)[0][10]), gate2=int(np.where(views == 2)[0][3]))
    assert len(set(who.values())) == 4
    sc = dict(base, xy=base["xy"].copy(), points=base["points"].copy())
    flat = sc["xy"].reshape(-1, 2)
    sc["points"][who["zero"]] = 0.0
    flat[sc["obs"][sc["offsets"][who["nan"]] + 1], 1] = np.nan
    who["cut3"], who["cut2"] = int(sc["offsets"][who["gate3"]] + 1), int(sc["offsets"][who["gate2"]])
    flat[sc["obs"][who["cut3"]]] += (50.0, 0.0)
    flat[sc["obs"][who["cut2"]]] += (0.0, -50.0)
    return sc, who


@functools.lru_cache(maxsize=None)
def scene_small():
    """The scene of the stop tests: 60 tracks of 2 .. 5 views over five cameras, max_pts 68.  The model's history from
    the default start: 5526.1 -> 5.3675 -> 9.871e-3 -> 1.1405e-5 -> 1.3366e-8 at lambda = 1e-3 .. 1e-6.  Shared:
    treat it as read-only."""
    return planted_scene(60, 5, 5, 0, 3, 0.01, 0.02)


FAR_TRACK, FAR_SCALE = 4, 1e170  # a two-view track (frames 3 and 4) that stays in front of both cameras when moved out


@functools.lru_cache(maxsize=None)
def scene_small_far_point():
    """scene_small() with track FAR_TRACK's entry point FAR_SCALE times as far from the origin: still in front of its
    two cameras and with finite pixel errors, so the track is used, but its JX is of the order fx / 1e170 and every
    product of two of them is below the smallest subnormal: V_t is exactly zero, v00 > 0 fails, V_t^-1 = 0 / 0.
    Returns (scene, the track's frames)."""
    base = scene_small()
    sc = dict(base, points=base["points"].copy())
    sc["points"][FAR_TRACK, :3] *= FAR_SCALE
    s = slice(base["offsets"][FAR_TRACK], base["offsets"][FAR_TRACK + 1])
    return sc, tuple((base["obs"][s] // base["max_pts"]).tolist())


def planted_cost(sc, **params):
    """C*: the cost of the planted poses and points on the scene's float32 pixels (no iteration: the entry cost)."""
    rows = np.concatenate([sc["planted"], np.ones((len(sc["planted"]), 1))], axis=1)
    return bundle_model(sc["xy"], sc["max_pts"], sc["offsets"], sc["obs"], sc["true_poses"], *sc["cam"], rows,
                        iterations=1, **params)["summary"][0]


def run_model(sc, **kw):
    """The model on a scene dictionary; the scene's "origin" (absent: 0) is the camera's, unless the call names one."""
    kw.setdefault("origin", sc.get("origin", 0.0))
    return bundle_model(sc["xy"], sc["max_pts"], sc["offsets"], sc["obs"], sc["poses"], *sc["cam"], sc["points"], **kw)


def with_origin(sc, origin):
    """The scene seen through a camera whose cx / cy count from `origin`: the pixels moved by -origin (rounded to float32
    again: they are this scene's pixels, not exact copies), the entry points triangulated with that camera.  The
    geometry is the scene's; only a reader that drops or flips the origin sees another one."""
    from tracks_model import triangulate_model

    xy = (sc["xy"].astype(f64) - origin).astype(np.float32)
    points, _ = triangulate_model(xy, sc["max_pts"], sc["offsets"], sc["obs"], sc["poses"], *sc["cam"], origin=origin)
    return dict(sc, xy=xy, points=points, origin=origin)


FILL = -7.0  # what device_bundle puts into every output entry before the call


def scene_records(sc):
    """The scene's pixels as SiftPoint records [n, max_pts]."""
    from oracle_binding import SIFT_POINT_DTYPE

    recs = np.zeros((sc["n"], sc["max_pts"]), SIFT_POINT_DTYPE)
    recs["coords2D"] = sc["xy"]
    return recs


class DeviceBundle:
    """A scene on the device for capi.Context.bundle_adjust: the records, offsets, obs and stats uploaded once, `cap`
    rows of points.  run() fills every output with FILL (the points: the scene's rows, FILL behind them), calls and
    reads everything back."""

    def __init__(self, ctx, sc, cap=None, n_tracks=None):
        self.ctx, self.sc = ctx, sc
        self.T = len(sc["offsets"]) - 1
        self.cap = self.T + 5 if cap is None else cap
        self.recs = scene_records(sc)
        stats = np.zeros(8, np.uint32)
        stats[0], stats[1] = (self.T if n_tracks is None else n_tracks), sc["offsets"][-1]
        self.inputs = [self.recs, np.ascontiguousarray(sc["offsets"], np.int32), np.ascontiguousarray(sc["obs"], np.int32),
                       stats]
        self.ptrs = [ctx.malloc(max(a.nbytes, 16)) for a in self.inputs]
        for p, a in zip(self.ptrs, self.inputs):
            ctx.h2d(p, a)
        self.outs = [ctx.malloc(max(8 * k, 16)) for k in (4 * max(self.cap, 1), 12 * sc["n"], 4 * 100, 8)]
        ctx.synchronize()

    def points_in(self):
        rows = np.full((max(self.cap, 1), 4), FILL)
        k = min(self.cap, self.T)
        rows[:k] = self.sc["points"][:k]
        return rows

    def run(self, n_images=None, max_tracks=None, **kw):
        """-> dict(points3d [cap, 4], poses [n, 3, 4], history [100, 4], summary [8]); entries not written are FILL."""
        ctx, n = self.ctx, self.sc["n"] if n_images is None else n_images
        host = [self.points_in(), np.full((self.sc["n"], 12), FILL), np.full((100, 4), FILL), np.full(8, FILL)]
        for p, a in zip(self.outs, host):
            ctx.h2d(p, a)
        ctx.synchronize()
        d_recs, d_offsets, d_obs, d_stats = self.ptrs
        ctx.bundle_adjust(d_recs, n, self.sc["max_pts"], d_offsets, d_obs, d_stats,
                          self.cap if max_tracks is None else max_tracks, self.sc["poses"][:n], self.camera(), *self.outs,
                          **kw)
        ctx.synchronize()
        for p, a in zip(self.outs, host):
            ctx.d2h(a, p)
        return dict(points3d=host[0], poses=host[1].reshape(-1, 3, 4), history=host[2], summary=host[3])

    def camera(self):
        from cusift_amd import capi

        return capi.Camera(*self.sc["cam"], origin=self.sc.get("origin", 0.0))

    def records_back(self):
        back = np.empty_like(self.recs)
        self.ctx.d2h(back, self.ptrs[0])
        return back

    def close(self):
        for p in self.ptrs + self.outs:
            self.ctx.free(p)
