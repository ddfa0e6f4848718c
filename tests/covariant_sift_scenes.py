"""The cases of covariant SIFT extraction (dsm_extract_covariant_sift): (name, image, options) as
tools/make_covdet_golden.py runs them through the reference's VLFeat into tests/golden/covdet_vlfeat_v1.npz.  The images come
from tests/sift_scenes.py: integer arithmetic alone, the same bytes on every host.

Options are the keywords of dsm_covariant_sift_options that VLFeat's half sees (octave_resolution, first_octave,
max_num_features, upright, domain_size_pooling, dsp_num_scales, peak_threshold, edge_threshold, dsp_min_scale, dsp_max_scale).
The normalisation is COLMAP's half and needs no run of its own: tests/covariant_sift_ref.py applies it to the stored data.

VLFeat's counts, as the tool prints them (detected, VLFeat's suppression counter, after the orientations, kept by the cut,
octaves that hold features, the most copies one detection has, patches that took the padded path of all kept x scales):
  blobs96x80     detected   12, suppressed   0, oriented   36, kept   36, octaves [0, 1], at most 4 orientations, 274 of 360 patches padded
  checker64      detected   54, suppressed   0, oriented  166, kept  166, octaves [0], at most 4 orientations, 1120 of 1660 patches padded
  checker17      detected    1, suppressed   0, oriented    4, kept    4, octaves [0], at most 4 orientations, 32 of 40 patches padded
  checker17_dsp_off detected    1, suppressed   0, oriented    4, kept    4, octaves [0], at most 4 orientations, 4 of 4 patches padded
  tex200x150     detected 1035, suppressed  11, oriented 1381, kept 1381, octaves [-1, 0, 1, 2], at most 4 orientations, 5291 of 13810 patches padded
  mid            detected  101, suppressed   1, oriented  119, kept  119, octaves [-1, 0, 1], at most 3 orientations, 843 of 1190 patches padded
  flat40x30      detected    0, suppressed   0, oriented    0, kept    0, octaves [], at most 0 orientations, 0 of 0 patches padded
  upright        detected  101, suppressed   1, oriented  100, kept  100, octaves [-1, 0, 1], at most 1 orientations, 667 of 1000 patches padded
  dsp_off        detected  101, suppressed   1, oriented  119, kept  119, octaves [-1, 0, 1], at most 3 orientations, 78 of 119 patches padded
  scales1        detected  101, suppressed   1, oriented  119, kept  119, octaves [-1, 0, 1], at most 3 orientations, 5 of 119 patches padded
  scales3        detected  101, suppressed   1, oriented  119, kept  119, octaves [-1, 0, 1], at most 3 orientations, 205 of 357 patches padded
  scales_other   detected  101, suppressed   1, oriented  119, kept  119, octaves [-1, 0, 1], at most 3 orientations, 311 of 476 patches padded
  first0         detected   13, suppressed   2, oriented   12, kept   12, octaves [0, 1], at most 2 orientations, 104 of 120 patches padded
  res2           detected   95, suppressed   1, oriented  114, kept  114, octaves [-1, 0, 1], at most 2 orientations, 824 of 1140 patches padded
  maxf_octaves   detected   13, suppressed   1, oriented   13, kept   13, octaves [0, 1], at most 2 orientations, 111 of 130 patches padded
  maxf_groups    detected  101, suppressed   1, oriented  119, kept   36, octaves [-1, 0, 1], at most 3 orientations, 293 of 360 patches padded
  maxf_inside    detected  101, suppressed   1, oriented  119, kept   36, octaves [-1, 0, 1], at most 3 orientations, 293 of 360 patches padded
  odd37x29       detected   28, suppressed   1, oriented   32, kept   32, octaves [-1, 0], at most 2 orientations, 267 of 320 patches padded
The octave of a feature is the one it was detected in; its patches come from the level the frame's size selects, down to
octave -1 for the small pooling scales.
"""
import numpy as np

from tests import sift_scenes

DEFAULTS = dict(octave_resolution=3, first_octave=-1, max_num_features=8192, upright=0, domain_size_pooling=1, dsp_num_scales=10,
                peak_threshold=0.02 / 3, edge_threshold=10.0, dsp_min_scale=1.0 / 6.0, dsp_max_scale=3.0)
OPTION_KEYS = ("octave_resolution", "first_octave", "max_num_features", "upright", "domain_size_pooling", "dsp_num_scales",
               "peak_threshold", "edge_threshold", "dsp_min_scale", "dsp_max_scale")

# cases whose raw descriptors are stored as floats; the others store one SHA-256 per feature over its [scales x 128] floats
FLOAT_CASES = ("checker17", "checker17_dsp_off", "first0")

# max_num_features of the three cut cases on `mid`, from the (o, s) group counts of the case "mid" as the tool prints them, in
# sorted order: 1,3:1 1,2:2 1,1:1 0,3:2 0,2:2 0,1:5 -1,4:1 -1,3:21 -1,2:34 -1,1:50 (running totals 1 3 4 6 8 13 14 35 69 119);
# the detection itself holds 5 features after octave 1 and 13 after octave 0 (the tool's "detected" of a run that stops there).
#   MAXF_BETWEEN_OCTAVES  above 5, at most 13: the detection loop stops after octave 0, octave -1 is never searched
#   MAXF_BETWEEN_GROUPS   a running total: the limit is reached by the last feature of group (-1, 3); the feature that opens
#                         (-1, 2) ends the loop and is kept (sift.cc:501 pushes before :507 tests)
#   MAXF_INSIDE_GROUP     inside group (-1, 3), which is kept whole: the same 36 features
# tools/make_covdet_golden.py asserts all three against the counts when it writes the file.
MAXF_BETWEEN_OCTAVES = 10
MAXF_BETWEEN_GROUPS = 35
MAXF_INSIDE_GROUP = 30


def blobs(width, height):
    """Twelve bright squares of sides 3 .. 9 on a dark ground, box-blurred three times: near-Gaussian blobs of several sizes, two of them
    overlapping."""
    a = np.zeros((height, width), np.int64)
    spots = [(12, 12, 3), (34, 14, 5), (60, 12, 7), (82, 16, 4), (14, 40, 6), (38, 42, 9), (41, 45, 8), (66, 40, 5), (84, 44, 7),
             (16, 66, 8), (44, 68, 4), (72, 66, 6)]
    for x, y, s in spots:
        a[y - s // 2:y - s // 2 + s, x - s // 2:x - s // 2 + s] += 4096
    for r in (1, 1, 2):
        a = sift_scenes.box_blur(a, r)
    return sift_scenes.stretch(a)


def _opts(**kw):
    o = dict(DEFAULTS)
    o.update(kw)
    return o


def cases():
    """[(name, image uint8 [h, w], options)]: the runs stored in the golden file."""
    mid = sift_scenes.texture(64, 48, 2)
    return [
        ("blobs96x80", blobs(96, 80), _opts()),
        ("checker64", sift_scenes.checkerboard(64, 64, 6), _opts()),
        ("checker17", sift_scenes.checkerboard(17, 17, 6), _opts()),
        ("checker17_dsp_off", sift_scenes.checkerboard(17, 17, 6), _opts(domain_size_pooling=0)),
        ("tex200x150", sift_scenes.texture(200, 150, 1), _opts()),
        ("mid", mid, _opts()),
        ("flat40x30", sift_scenes.constant(40, 30), _opts()),
        ("upright", mid, _opts(upright=1)),
        ("dsp_off", mid, _opts(domain_size_pooling=0)),
        ("scales1", mid, _opts(dsp_num_scales=1)),
        ("scales3", mid, _opts(dsp_num_scales=3)),
        ("scales_other", mid, _opts(dsp_num_scales=4, dsp_min_scale=0.5, dsp_max_scale=2.0)),
        ("first0", mid, _opts(first_octave=0)),
        ("res2", mid, _opts(octave_resolution=2, peak_threshold=0.02 / 2)),
        ("maxf_octaves", mid, _opts(max_num_features=MAXF_BETWEEN_OCTAVES)),
        ("maxf_groups", mid, _opts(max_num_features=MAXF_BETWEEN_GROUPS)),
        ("maxf_inside", mid, _opts(max_num_features=MAXF_INSIDE_GROUP)),
        ("odd37x29", sift_scenes.texture(37, 29, 4), _opts()),
    ]
