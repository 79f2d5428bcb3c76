"""cusift_describe_batch's front, restated in numpy float32 (include/cusift_amd_extras.h pins it expression by
expression): the validity test, the octave rule, the octave units -- and, from the CPU oracle's stages, the records the
call must return.  Shared by test_describe_model.py (no GPU) and test_describe.py."""
import numpy as np

K_LOW = np.float32(0.93303299)  # 2^-0.1: scales[0] * 2^(-0.5 / NUM_SCALES), the detector's lowest scale / subsampling
KEEP_ORIENTATION, OCTAVE_FROM_SCALE = 1, 2


def octave_subsamplings(num_octaves, subsampling=1.0, upsample=0, w=None, h=None):
    """sub[o] of the octave images: sub[0] = subsampling (half of it with upsample), doubled per octave; with (w, h) the
    list ends where the extraction's pyramid does (an image side below 1)."""
    sub = [np.float32(subsampling) * np.float32(0.5) if upsample else np.float32(subsampling)]
    if w is not None:
        w, h = (2 * w, 2 * h) if upsample else (w, h)
    for _ in range(1, max(1, min(int(num_octaves), 16))):
        if w is not None:
            w, h = w // 2, h // 2
            if w < 1 or h < 1:
                break
        sub.append(np.float32(sub[-1] * np.float32(2.0)))
    return np.array(sub, dtype=np.float32)


def valid(x, y, scale):
    """A record is described iff both coordinates and the scale are finite and the scale is positive."""
    x, y, scale = (np.asarray(v, dtype=np.float32) for v in (x, y, scale))
    with np.errstate(invalid="ignore"):
        return np.isfinite(x) & np.isfinite(y) & np.isfinite(scale) & (scale > 0)


def octave_of(scale, rec_sub, sub, flags=0):
    """The octave index of every record: the recorded one (flag clear, the record's subsampling has exactly the bits of
    some sub[o]: the first such o), else the largest o with scale >= K_LOW * sub[o] in float32, 0 if there is none."""
    scale = np.asarray(scale, dtype=np.float32)
    rec_bits = np.asarray(rec_sub, dtype=np.float32).view(np.uint32)
    sub = np.asarray(sub, dtype=np.float32)
    bound = (K_LOW * sub).astype(np.float32)  # one float32 product per octave
    out = np.zeros(len(scale), dtype=np.int64)
    with np.errstate(invalid="ignore"):
        for o in range(1, len(sub)):
            out[scale >= bound[o]] = o
    if not flags & OCTAVE_FROM_SCALE:
        for o in range(len(sub) - 1, -1, -1):
            out[rec_bits == sub[o:o + 1].view(np.uint32)[0]] = o
    return out


def octave_units(recs, sub_of_rec):
    """(px, py, kscale): three float32 divisions by the octave's subsampling."""
    s = np.asarray(sub_of_rec, dtype=np.float32)
    with np.errstate(all="ignore"):
        return ((recs["coords2D"][:, 0] / s).astype(np.float32), (recs["coords2D"][:, 1] / s).astype(np.float32),
                (recs["scale"] / s).astype(np.float32))


def up2(img):
    """cusift_scale_up in numpy float32, associated as the header writes its four formulas."""
    s = np.ascontiguousarray(img, dtype=np.float32)
    h, w = s.shape
    x1, y1 = np.minimum(np.arange(w) + 1, w - 1), np.minimum(np.arange(h) + 1, h - 1)
    sx, sy, sxy = s[:, x1], s[y1, :], s[y1][:, x1]
    d = np.empty((2 * h, 2 * w), dtype=np.float32)
    d[0::2, 0::2] = s
    d[0::2, 1::2] = np.float32(0.5) * (s + sx)
    d[1::2, 0::2] = np.float32(0.5) * (s + sy)
    d[1::2, 1::2] = np.float32(0.25) * ((s + sx) + (sy + sxy))
    return d


def oracle_pyramid(oracle, img, num_octaves, upsample=0):
    """[(pitched image, w, h)] per octave: the oracle's ScaleDown chain (on the enlarged image with upsample)."""
    from oracle_binding import pitched

    img = up2(img) if upsample else np.asarray(img, dtype=np.float32)
    h, w = img.shape
    levels = [(pitched(img), w, h)]
    for _ in range(1, max(1, min(int(num_octaves), 16))):
        if w // 2 < 1 or h // 2 < 1:
            break
        levels.append((oracle.scale_down(levels[-1][0], w, h), w // 2, h // 2))
        w, h = w // 2, h // 2
    return levels


def oracle_describe(oracle, img, recs, flags=0, num_octaves=5, subsampling=1.0, upsample=0, tex_frac_bits=8,
                    root_sift=0):
    """What cusift_describe_batch must leave in `recs` (a copy is returned), from the CPU oracle's stages run per
    octave on the oracle's pyramid; the octave per record comes from octave_of."""
    h, w = img.shape
    levels = oracle_pyramid(oracle, img, num_octaves, upsample)
    sub = octave_subsamplings(num_octaves, subsampling, upsample, w, h)
    assert len(sub) == len(levels)
    out = recs.copy()
    ok = valid(recs["coords2D"][:, 0], recs["coords2D"][:, 1], recs["scale"])
    octv = octave_of(recs["scale"], recs["subsampling"], sub, flags)
    out["data"][~ok] = 0
    out["subsampling"][~ok] = 0
    for o, (lvl, lw, lh) in enumerate(levels):
        idx = np.flatnonzero(ok & (octv == o))
        if not len(idx):
            continue
        work = recs[idx].copy()
        px, py, ks = octave_units(work, np.full(len(idx), sub[o], dtype=np.float32))
        work["coords2D"][:, 0], work["coords2D"][:, 1], work["scale"] = px, py, ks
        if not flags & KEEP_ORIENTATION:
            oracle.compute_orientations(lvl, lw, lh, work, 0, len(work), tex_frac_bits)
        oracle.extract_descriptors(lvl, lw, lh, work, 0, len(work), float(sub[o]), tex_frac_bits)
        if root_sift:
            oracle.rootsift(work, len(work))
        out["orientation"][idx] = work["orientation"]
        out["data"][idx] = work["data"]
        out["subsampling"][idx] = sub[o]
    return out, octv, ok
