"""The cases of covariant SIFT extraction with estimate_affine_shape = 1 (dsm_extract_covariant_sift_affine):
(name, image, options) as tools/make_covdet_affine_golden.py runs them through the reference's VLFeat into
tests/golden/covdet_vlfeat_affine_v1.npz.  The images are those of tests/sift_scenes.py and covariant_sift_scenes.blobs.

Every case has estimate_affine_shape = 1; OPTION_KEYS is covariant_sift_scenes.OPTION_KEYS with that key appended.  With it
vl_covdet_extract_affine_shape replaces vl_covdet_extract_orientations (sift.cc:467-473): no feature is dropped and none is
copied, so the adapted list has the length and the order of the list after the suppression, which
tests/golden/covdet_vlfeat_v1.npz holds for the same scene.

VLFeat's counts, as the tool prints them (detected, after the suppression = adapted, kept by the cut, octaves that hold
features, frames the adaptation made anisotropic, patches that took the padded path of all kept x scales):
  blobs96x80     detected   12, adapted   12, kept   12, octaves [0, 1], 12 anisotropic, 89 of 120 patches padded
  checker64      detected   54, adapted   54, kept   54, octaves [0], 39 anisotropic, 394 of 540 patches padded
  checker17      detected    1, adapted    1, kept    1, octaves [0], 1 anisotropic, 8 of 10 patches padded
  tex200x150     detected 1035, adapted 1024, kept 1024, octaves [-1, 0, 1, 2], 1024 anisotropic, 3912 of 10240 patches padded
  mid            detected  101, adapted  100, kept  100, octaves [-1, 0, 1], 100 anisotropic, 731 of 1000 patches padded
  dsp_off        detected  101, adapted  100, kept  100, octaves [-1, 0, 1], 100 anisotropic, 64 of 100 patches padded
  first0         detected   13, adapted   11, kept   11, octaves [0, 1], 11 anisotropic, 95 of 110 patches padded
  res2           detected   95, adapted   94, kept   94, octaves [-1, 0, 1], 94 anisotropic, 680 of 940 patches padded
  odd37x29       detected   28, adapted   27, kept   27, octaves [-1, 0], 27 anisotropic, 229 of 270 patches padded
  flat40x30      detected    0, adapted    0, kept    0, octaves [], 0 anisotropic, 0 of 0 patches padded
  upright        detected  101, adapted  100, kept  100, octaves [-1, 0, 1], 0 anisotropic, 667 of 1000 patches padded
  maxf_octaves   detected   13, adapted   12, kept   12, octaves [0, 1], 12 anisotropic, 101 of 120 patches padded
  maxf_groups    detected  101, adapted  100, kept   32, octaves [-1, 0, 1], 32 anisotropic, 262 of 320 patches padded
  maxf_inside    detected  101, adapted  100, kept   32, octaves [-1, 0, 1], 32 anisotropic, 262 of 320 patches padded
"""
from tests import sift_scenes
from tests.covariant_sift_scenes import DEFAULTS, blobs
from tests.covariant_sift_scenes import OPTION_KEYS as BASE_OPTION_KEYS

OPTION_KEYS = BASE_OPTION_KEYS + ("estimate_affine_shape",)

# cases whose raw descriptors are stored as floats; the others store one SHA-256 per feature over its [scales x 128] floats
FLOAT_CASES = ("checker17", "first0", "blobs96x80")

# max_num_features of the three cut cases on `mid`, from the (o, s) group counts of the affine case "mid" (100 features, no
# copies) as the tool prints them, in sorted order: 1,3:1 1,2:2 1,1:1 0,3:2 0,2:2 0,1:4 -1,4:1 -1,3:18 -1,2:31 -1,1:38 (running
# totals 1 3 4 6 8 12 13 31 62 100); the detection itself holds 5 features after octave 1 and 13 after octave 0.
#   MAXF_BETWEEN_OCTAVES  above 5, at most 13: the detection loop stops after octave 0, octave -1 is never searched
#   MAXF_BETWEEN_GROUPS   a running total: the limit is reached by the last feature of group (-1, 3); the feature that opens
#                         (-1, 2) ends the loop and is kept
#   MAXF_INSIDE_GROUP     inside group (-1, 3), which is kept whole: the same 32 features
# tools/make_covdet_affine_golden.py asserts all three against the counts when it writes the file.
MAXF_BETWEEN_OCTAVES = 10
MAXF_BETWEEN_GROUPS = 31
MAXF_INSIDE_GROUP = 20

# the case of tests/golden/covdet_vlfeat_v1.npz that holds the same scene's detection lists (`detected`, `suppressed`); the two
# cuts that search every octave have those of `mid` (max_num_features ends the detection between octaves and nowhere else)
V1_CASE = {"blobs96x80": "blobs96x80", "checker64": "checker64", "checker17": "checker17", "tex200x150": "tex200x150", "mid": "mid",
           "dsp_off": "dsp_off", "first0": "first0", "res2": "res2", "odd37x29": "odd37x29", "flat40x30": "flat40x30", "upright": "upright",
           "maxf_octaves": "maxf_octaves", "maxf_groups": "mid", "maxf_inside": "mid"}

# why each feature left vl_covdet_extract_affine_shape_for_frame: (diverged, max iterations, zero moment, converged), counted
# with an instrumented build of the reference's covdet.c (unmodified VLFeat does not report it)
EXITS = {"blobs96x80": (0, 1, 0, 11), "checker64": (0, 0, 0, 54), "checker17": (0, 0, 0, 1), "tex200x150": (1, 7, 0, 1016),
         "mid": (0, 1, 0, 99), "first0": (0, 0, 0, 11), "res2": (0, 1, 0, 93), "odd37x29": (0, 0, 0, 27)}
CHECKER64_CONVERGED_AT_FIRST_TEST = 15


def _opts(**kw):
    o = dict(DEFAULTS)
    o["estimate_affine_shape"] = 1
    o.update(kw)
    return o


def cases():
    """[(name, image uint8 [h, w], options)]: the runs stored in the golden file."""
    mid = sift_scenes.texture(64, 48, 2)
    return [
        ("blobs96x80", blobs(96, 80), _opts()),
        ("checker64", sift_scenes.checkerboard(64, 64, 6), _opts()),
        ("checker17", sift_scenes.checkerboard(17, 17, 6), _opts()),
        ("tex200x150", sift_scenes.texture(200, 150, 1), _opts()),
        ("mid", mid, _opts()),
        ("dsp_off", mid, _opts(domain_size_pooling=0)),
        ("first0", mid, _opts(first_octave=0)),
        ("res2", mid, _opts(octave_resolution=2, peak_threshold=0.02 / 2)),
        ("odd37x29", sift_scenes.texture(37, 29, 4), _opts()),
        ("flat40x30", sift_scenes.constant(40, 30), _opts()),
        ("upright", mid, _opts(upright=1)),
        ("maxf_octaves", mid, _opts(max_num_features=MAXF_BETWEEN_OCTAVES)),
        ("maxf_groups", mid, _opts(max_num_features=MAXF_BETWEEN_GROUPS)),
        ("maxf_inside", mid, _opts(max_num_features=MAXF_INSIDE_GROUP)),
    ]
