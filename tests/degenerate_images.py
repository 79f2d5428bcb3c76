"""Images on which the detection and keypoint stages meet exact ties, symmetry and non-finite arithmetic
(tests/test_degenerate_content.py; tools/fuzz_parity.py draws them too).  Plain numpy, fixed seeds, float32, any size.

  rows, cols     pixel = f(y) / f(x), uniform random levels in [0, 255): every DoG value equals both of its neighbours
                 along the stripe, so no centre is a STRICT extremum and thousands are tied ones
  checker        ((x + y) & 1) * 255: strict extrema among tied centres, orientation peaks within 1e-3 of each other
  dots8, dots16  255 where x % p == p/2 and y % p == p/2: four-fold symmetric gradients, orientation peaks exactly equal
  mirror         noise whose right half is its left half mirrored (even widths): tied centres across the axis
  nan_pixel,     noise with one NaN / one +Inf pixel: 9 x 9 x 7 NaN DoG values and, for Inf, NaN orientations and
  inf_pixel      descriptors further out
  scaled         noise * 2^e (thresholds * 2^e with it): the DoG scales exactly, the refinement's products leave the
                 normal float range
"""
import numpy as np

SIZES = [(256, 40), (481, 33), (241, 9)]  # cross a 240-column strip border; 481 and 241 are ragged
STRIP = 240
SCALED_EXPONENTS = (-46, -48, -50, -52, 36, 44, 60)


def noise(seed, w, h):
    return (np.random.RandomState(seed).rand(h, w) * 255.0).astype(np.float32)


def rows(seed, w, h):
    lv = (np.random.RandomState(seed).rand(h) * 255.0).astype(np.float32)
    return np.ascontiguousarray(np.broadcast_to(lv[:, None], (h, w)))


def cols(seed, w, h):
    lv = (np.random.RandomState(seed).rand(w) * 255.0).astype(np.float32)
    return np.ascontiguousarray(np.broadcast_to(lv[None, :], (h, w)))


def checker(w, h):
    y, x = np.mgrid[0:h, 0:w]
    return (((x + y) & 1) * 255).astype(np.float32)


def dots(w, h, period):
    y, x = np.mgrid[0:h, 0:w]
    return (((x % period == period // 2) & (y % period == period // 2)) * 255).astype(np.float32)


def mirror(seed, w, h):
    assert w % 2 == 0, "mirror: even widths only"
    img = noise(seed, w, h)
    img[:, w // 2:] = img[:, :w // 2][:, ::-1]
    return img


def pixel_positions(w, h):
    """(name, y, x) of the poisoned pixel: the image centre, both sides of the 240-column strip border in a middle row
    (where the image is wider than a strip), and the corner."""
    pos = [("centre", h // 2, w // 2)]
    if w > STRIP:
        pos += [("col239", h // 2, STRIP - 1), ("col240", h // 2, STRIP)]
    return pos + [("corner", 0, 0)]


def poisoned(seed, w, h, value, y, x):
    img = noise(seed, w, h)
    img[y, x] = value
    return img


def scaled(seed, w, h, e):
    """noise * 2^e, exact (a power of two, and no product leaves the normal range: 255 * 2^-52 and 255 * 2^60 are
    normal floats)."""
    return noise(seed, w, h) * np.float32(2.0 ** e)


def fuzz_image(rng, w, h):
    """One image of a random family for the randomised sweep (finite thresholds of the sweep apply, so `scaled` stays
    out: its thresholds scale with it)."""
    seed = int(rng.integers(0, 10 ** 6))
    kinds = ["rows", "cols", "checker", "dots8", "dots16", "nan_pixel", "inf_pixel"] + (["mirror"] if w % 2 == 0 else [])
    kind = kinds[int(rng.integers(0, len(kinds)))]
    if kind in ("nan_pixel", "inf_pixel"):
        _, y, x = pixel_positions(w, h)[int(rng.integers(0, len(pixel_positions(w, h))))]
        return poisoned(seed, w, h, np.nan if kind == "nan_pixel" else np.inf, y, x)
    return {"rows": lambda: rows(seed, w, h), "cols": lambda: cols(seed, w, h), "checker": lambda: checker(w, h),
            "dots8": lambda: dots(w, h, 8), "dots16": lambda: dots(w, h, 16), "mirror": lambda: mirror(seed, w, h)}[kind]()
