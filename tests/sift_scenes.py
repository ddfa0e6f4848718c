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


# ---------------------------------------------------------------------------------------------------------------------------
# The second golden file (tests/golden/sift_vlfeat_v2.npz): the octaves, sizes and options cases() leaves out.


def coarse(width, height, seed, k):
    """texture() of 1 / k the size, every pixel repeated k x k, box-blurred with radius k / 2 and stretched: structure large
    enough to survive first_octave = 2 and 3, with neighbouring pixels that still differ (a sampling offset would show)."""
    t = texture((width + k - 1) // k, (height + k - 1) // k, seed)
    big = np.repeat(np.repeat(t, k, axis=0), k, axis=1)[:height, :width]
    return stretch(box_blur(big, k // 2))


def checkerboard(width, height, cell=4):
    """0 / 255 squares of `cell` pixels: exact symmetries, so equal DoG samples and equal histogram bins."""
    y, x = np.mgrid[0:height, 0:width]
    return ((((x // cell) + (y // cell)) & 1) * 255).astype(np.uint8)


def dots(width, height, period=8, size=2):
    """size x size squares of 255 every `period` pixels on 0.  A square of even size has its centre between four pixels, so
    the DoG extremum over it is shared by equal neighbouring samples."""
    y, x = np.mgrid[0:height, 0:width]
    return (((x % period < size) & (y % period < size)) * 255).astype(np.uint8)


def binary_noise(width, height, seed):
    """The lowest bit of hash_field as 0 / 255: every pixel an extremum of something."""
    return ((hash_field(width, height, seed) & np.uint64(1)) * np.uint64(255)).astype(np.uint8)


ZERO_RESULT_V2 = ("line40x1", "line1x40", "rows40x2", "small20x5")


def cases_v2():
    """[(name, image uint8 [h, w], options)]: the runs stored in tests/golden/sift_vlfeat_v2.npz.

    VLFeat's counts, as the tool prints them (it now adds the most orientations any keypoint has):
      first-2_sq20     14 keypoints,   16 descriptors, octaves [-2, -1, 0], 6 DoG levels, at most 2 orientations
      first-2_32x24    30 keypoints,   36 descriptors, octaves [-2, -1], 4 DoG levels, at most 2 orientations
      first-3_sq16     10 keypoints,   11 descriptors, octaves [-3, -2, -1], 5 DoG levels, at most 2 orientations
      first2_253x191   20 keypoints,   21 descriptors, octaves [2, 3], 5 DoG levels, at most 2 orientations
      first3_253x191    4 keypoints,    4 descriptors, octaves [3], 2 DoG levels, at most 1 orientations
      octaves-1       100 keypoints,  117 descriptors, octaves [-1, 0, 1], 9 DoG levels, at most 2 orientations
      octaves0          0 keypoints,    0 descriptors, octaves [], 0 DoG levels, at most 0 orientations
      octaves1         87 keypoints,  103 descriptors, octaves [-1], 3 DoG levels, at most 2 orientations
      octaves10_16x16    4 keypoints,    4 descriptors, octaves [-1], 2 DoG levels, at most 1 orientations
      line40x1          0 keypoints,    0 descriptors, octaves [], 0 DoG levels, at most 0 orientations
      line1x40          0 keypoints,    0 descriptors, octaves [], 0 DoG levels, at most 0 orientations
      rows40x2          0 keypoints,    0 descriptors, octaves [], 0 DoG levels, at most 0 orientations
      small20x5         0 keypoints,    0 descriptors, octaves [], 0 DoG levels, at most 0 orientations
      thin44x10         9 keypoints,   10 descriptors, octaves [-1, 0], 4 DoG levels, at most 2 orientations
      checker40x40    120 keypoints,  368 descriptors, octaves [-1], 2 DoG levels, at most 4 orientations
      dots40x40        39 keypoints,   81 descriptors, octaves [-1, 0], 3 DoG levels, at most 4 orientations
      noise64x48       16 keypoints,   25 descriptors, octaves [-1], 2 DoG levels, at most 3 orientations
      lowthreshold    104 keypoints,  122 descriptors, octaves [-1, 0, 1], 9 DoG levels, at most 2 orientations
      dense18x48      110 keypoints,  332 descriptors, octaves [-1], 2 DoG levels, at most 4 orientations
    thin44x10 asks for 6 octaves: 88 x 20, 44 x 10 and 22 x 5 are searched, 11 x 2 is smoothed and skipped (under 3 rows), 5 x 1
    ends the loop (under 2).  octaves10_16x16 goes 32, 16, 8, 4 (searched), 2 (skipped), 1 (the end)."""
    mid = texture(64, 48, 2)
    big = coarse(253, 191, 6, 4)  # 253 >> 2 = 63 and 191 >> 2 = 47 drop a remainder; 31 x 23 at first_octave = 3
    return [
        ("first-2_sq20", texture(20, 20, 22), _opts(first_octave=-2)),
        ("first-2_32x24", texture(32, 24, 23), _opts(first_octave=-2)),  # non-square: the second doubling is scrambled
        ("first-3_sq16", texture(16, 16, 20), _opts(first_octave=-3)),
        ("first2_253x191", big, _opts(first_octave=2)),
        ("first3_253x191", big, _opts(first_octave=3)),
        ("octaves-1", mid, _opts(num_octaves=-1)),  # automatic: floor(log2(48)) + 1 - 3 = 3 octaves, as many as hold keypoints
        ("octaves0", mid, _opts(num_octaves=0)),
        ("octaves1", mid, _opts(num_octaves=1)),
        ("octaves10_16x16", texture(16, 16, 8), _opts(num_octaves=10)),
        ("line40x1", texture(40, 1, 3), _opts()),
        ("line1x40", texture(1, 40, 3), _opts()),
        ("rows40x2", texture(40, 2, 3), _opts()),
        ("small20x5", texture(20, 5, 3), _opts()),
        ("thin44x10", texture(44, 10, 7), _opts(num_octaves=6)),
        ("checker40x40", checkerboard(40, 40), _opts()),
        ("dots40x40", dots(40, 40), _opts()),  # ties that decide: samples >= all 26 neighbours and equal to one of them
        ("noise64x48", binary_noise(64, 48, 5), _opts()),
        ("lowthreshold", mid, _opts(peak_threshold=1e-4, edge_threshold=100.0)),
        ("dense18x48", checkerboard(18, 48, 3), _opts()),  # 36 samples a row: a chunk of 256 flags spans 7 rows of close extrema
    ]
