"""Deterministic grey test images for SIFT extraction, from integer arithmetic alone: an integer hash of the pixel index
(multiply / xor / shift modulo 2^32) thresholded into sparse seeds, integer box blurs of several radii (running sums, floor
division, clamped borders) and an integer contrast stretch.  No libm and no floating point sits between the recipe and the
pixels, so every host produces the same bytes.

The texture is dense blobs of radii from about 1.5 to 8 pixels: seeds blurred twice with box radii 1, 2, 4 and 7, summed.

CASES is the list tools/make_sift_golden.py runs through VLFeat (both of its builds) into tests/golden/sift_vlfeat_v1.npz and
the tests read back: (name, image, options) with options as the keywords of dsm_sift_options that the VLFeat stage sees
(num_octaves, octave_resolution, first_octave, peak_threshold, edge_threshold, upright).  What COLMAP does after VLFeat
(max_num_orientations, normalization, max_num_features) needs no run of its own: tests/sift_ref.py applies it to the stored data.

VLFeat's counts for the stored cases, as the tool prints them (refined keypoints, descriptors = orientations over all
keypoints, octaves and DoG levels that hold keypoints):
  tex96x80        241 keypoints,  287 descriptors, octaves [-1, 0, 1], 9 DoG levels
  tex64x48        100 keypoints,  117 descriptors, octaves [-1, 0, 1], 9 DoG levels
  tex64x48_b       94 keypoints,  110 descriptors, octaves [-1, 0, 1, 2], 9 DoG levels
  odd37x29         27 keypoints,   36 descriptors, octaves [-1, 0], 5 DoG levels
  odd65x63        132 keypoints,  155 descriptors, octaves [-1, 0, 1], 7 DoG levels
  thin130x20       66 keypoints,   73 descriptors, octaves [-1, 0], 5 DoG levels
  tiny16x16         4 keypoints,    4 descriptors, octaves [-1], 2 DoG levels
  constant40x30     0 keypoints,    0 descriptors, octaves [], 0 DoG levels
  border48x40       5 keypoints,    5 descriptors, octaves [-1, 0], 3 DoG levels
  first0           14 keypoints,   17 descriptors, octaves [0, 1], 6 DoG levels
  first1            4 keypoints,    5 descriptors, octaves [1], 2 DoG levels
  res2             76 keypoints,   92 descriptors, octaves [-1, 0, 1], 5 DoG levels
  res5            109 keypoints,  128 descriptors, octaves [-1, 0, 1], 13 DoG levels
  upright         100 keypoints,  100 descriptors, octaves [-1, 0, 1], 9 DoG levels
  single            1 keypoints,    2 descriptors, octaves [-1], 1 DoG levels
"""
import numpy as np

_M = np.uint64(0xFFFFFFFF)


def hash_field(width, height, seed):
    """uint32 per pixel: a multiply-xorshift hash of (index, seed)."""
    i = np.arange(width * height, dtype=np.uint64)
    v = (i * np.uint64(2654435761) + np.uint64(seed) * np.uint64(40503) + np.uint64(12345)) & _M
    v ^= v >> np.uint64(15)
    v = (v * np.uint64(2246822519)) & _M
    v ^= v >> np.uint64(13)
    v = (v * np.uint64(3266489917)) & _M
    v ^= v >> np.uint64(16)
    return v.reshape(height, width)


def box_blur(a, r):
    """Integer box blur of radius r along both axes: the sum over the clamped window, floor-divided by its nominal size."""
    a = np.asarray(a, np.int64)
    for axis in (0, 1):
        n = a.shape[axis]
        idx = np.clip(np.arange(-r, n + r), 0, n - 1)
        p = np.take(a, idx, axis=axis)
        c = np.concatenate([np.zeros_like(np.take(p, [0], axis=axis)), np.cumsum(p, axis=axis)], axis=axis)
        hi = np.take(c, np.arange(2 * r + 1, n + 2 * r + 1), axis=axis)
        lo = np.take(c, np.arange(0, n), axis=axis)
        a = (hi - lo) // (2 * r + 1)
    return a


def stretch(a):
    """Integer contrast stretch to 0 .. 255."""
    a = np.asarray(a, np.int64)
    lo, hi = int(a.min()), int(a.max())
    if hi == lo:
        return np.full(a.shape, 128, np.uint8)
    return ((a - lo) * 255 // (hi - lo)).astype(np.uint8)


def texture(width, height, seed=1):
    """Dense blob texture, uint8 [height, width]."""
    total = np.zeros((height, width), np.int64)
    for k, (r, sparsity) in enumerate(((1, 5), (2, 11), (4, 37), (7, 101))):
        seeds = (hash_field(width, height, seed * 16 + k) % np.uint64(sparsity) == 0).astype(np.int64) * 4096
        total += stretch(box_blur(box_blur(seeds, r), r)).astype(np.int64)
    return stretch(total)


def constant(width, height, value=93):
    return np.full((height, width), value, np.uint8)


def border_only(width, height, seed=3, margin=3):
    """Structure within `margin` pixels of each border only; the interior is flat."""
    im = texture(width, height, seed)
    out = np.full((height, width), 128, np.uint8)
    for sl in ((slice(0, margin), slice(None)), (slice(height - margin, height), slice(None)),
               (slice(None), slice(0, margin)), (slice(None), slice(width - margin, width))):
        out[sl] = im[sl]
    return out


DEFAULTS = dict(num_octaves=4, octave_resolution=3, first_octave=-1, peak_threshold=0.02 / 3, edge_threshold=10.0, upright=0)


def _opts(**kw):
    o = dict(DEFAULTS)
    o.update(kw)
    return o


def cases():
    """[(name, image uint8 [h, w], options)]: the runs stored in the golden file."""
    mid = texture(64, 48, 2)
    return [
        ("tex96x80", texture(96, 80, 1), _opts()),
        ("tex64x48", mid, _opts()),
        ("tex64x48_b", np.roll(mid, (-2, -3), axis=(0, 1)), _opts()),  # the same texture moved by (3, 2), wrapping: matches tex64x48
        ("odd37x29", texture(37, 29, 4), _opts()),
        ("odd65x63", texture(65, 63, 5), _opts()),
        ("thin130x20", texture(130, 20, 6), _opts()),
        ("tiny16x16", texture(16, 16, 8), _opts(num_octaves=4)),
        ("constant40x30", constant(40, 30), _opts()),
        ("border48x40", border_only(48, 40), _opts()),
        ("first0", mid, _opts(first_octave=0)),
        ("first1", mid, _opts(first_octave=1)),
        ("res2", mid, _opts(octave_resolution=2, peak_threshold=0.02 / 2)),
        ("res5", mid, _opts(octave_resolution=5, peak_threshold=0.02 / 5)),
        ("upright", mid, _opts(upright=1)),
        ("single", mid, _opts(peak_threshold=SINGLE_PEAK_THRESHOLD)),
    ]


# a peak_threshold that leaves exactly one keypoint on texture(64, 48, 2) (found with tools/make_sift_golden.py --peaks)
SINGLE_PEAK_THRESHOLD = 0.034
