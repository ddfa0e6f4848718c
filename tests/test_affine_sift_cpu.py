"""CPU-only: the public surface of dsm_extract_covariant_sift_affine, the golden file
tests/golden/covdet_vlfeat_affine_v1.npz (its structure, its relation to covdet_vlfeat_v1.npz, the coverage conditions its
cases are stored for, and -- where the reference tree is present -- that tools/make_covdet_affine_golden.py reproduces its
bytes).  Every comparison is exact."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import affine_sift_ref as ref
from tests import affine_sift_scenes as scenes
from tests import covariant_sift_ref as v1ref
from tests import covariant_sift_scenes as v1scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE = "/root/reference"


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else a.dtype)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and (bits(a) == bits(b)).all()


def groups_of(os_sorted):
    out = []
    for o, s in os_sorted.tolist():
        if out and out[-1][0] == (o, s):
            out[-1][1] += 1
        else:
            out.append([(o, s), 1])
    return out


def test_public_surface():
    """Both builds export the two new symbols, the binding has the two methods, and the default of the option is still 0."""
    from dagsfm_amd import capi
    for path in (capi.LIB_PATH, capi.CHECK_LIB_PATH):
        assert os.path.exists(path), path
        lib = ctypes.CDLL(path)
        for s in ("dsm_extract_covariant_sift_affine", "dsm_get_affine_shape_stats"):
            assert hasattr(lib, s), "missing export in %s: %s" % (os.path.basename(path), s)
    assert callable(capi.Context.extract_covariant_sift_affine) and callable(capi.Context.affine_shape_stats)
    assert capi.default_covariant_sift_options().estimate_affine_shape == 0
    assert capi.default_covariant_sift_options(check=True).estimate_affine_shape == 0
    assert capi.Context.AFFINE_SHAPE_EXITS == ("diverged", "max_iterations", "zero_moment", "converged")
    header = open(os.path.join(ROOT, "include", "dagsfm_mi355x.h")).read()
    assert "#define DSM_AFFINE_SHAPE_MAX_ROUNDS 14" in header


def test_cases_are_the_issues():
    names = [n for n, _, _ in scenes.cases()]
    assert len(set(names)) == len(names) == 14
    by = {n: (im, o) for n, im, o in scenes.cases()}
    assert all(o["estimate_affine_shape"] == 1 for _, o in by.values())
    mid = by["mid"][0]
    for n, kw in (("dsp_off", dict(domain_size_pooling=0)), ("first0", dict(first_octave=0)), ("upright", dict(upright=1)),
                  ("res2", dict(octave_resolution=2, peak_threshold=0.01)), ("maxf_octaves", dict(max_num_features=scenes.MAXF_BETWEEN_OCTAVES)),
                  ("maxf_groups", dict(max_num_features=scenes.MAXF_BETWEEN_GROUPS)), ("maxf_inside", dict(max_num_features=scenes.MAXF_INSIDE_GROUP))):
        assert (by[n][0] == mid).all() and by[n][1] == dict(by["mid"][1], **kw), n
    assert mid.shape == (48, 64) and by["tex200x150"][0].shape == (150, 200) and by["odd37x29"][0].shape == (29, 37)
    assert max(im.shape[0] for im, _ in by.values()) <= 150 and max(im.shape[1] for im, _ in by.values()) <= 200
    assert set(scenes.EXITS) <= set(names) and all(len(e) == 4 for e in scenes.EXITS.values())


def test_golden_file_structure():
    g, v1 = ref.golden(), v1ref.golden()
    assert sorted(g) == sorted(name for name, _, _ in scenes.cases())
    assert os.path.getsize(ref.GOLDEN) <= 578734
    for name, image, options in scenes.cases():
        c, old = g[name], v1[scenes.V1_CASE[name]]
        assert (c["image"] == image).all() and c["image"].dtype == np.uint8
        assert c["options"] == {k: options[k] for k in scenes.OPTION_KEYS} and c["options"]["estimate_affine_shape"] == 1
        # the same scene: max_num_features may differ where both runs search every octave (the counts below say that they do)
        assert (old["image"] == image).all() and all(old["options"][k] == options[k] for k in v1scenes.OPTION_KEYS if k != "max_num_features")
        assert old["options"]["max_num_features"] == options["max_num_features"] or name in ("maxf_groups", "maxf_inside")
        counts = c["counts"].tolist()
        assert len(counts) == 6 and counts[:3] == old["counts"].tolist()[:3]
        n = len(old["suppressed_frames"])
        assert counts[2] == counts[3] == n  # no feature is dropped and no copy is added
        for stage in ref.STAGES:
            assert c[stage + "_frames"].shape == (n, 6) and c[stage + "_frames"].dtype == np.float32
            assert c[stage + "_os"].shape == (n, 2) and c[stage + "_os"].dtype == np.int32
            assert c[stage + "_scores"].shape == (n, 3) and c[stage + "_scores"].dtype == np.float32
        # only the four shape entries move
        assert same(c["adapted_frames"][:, :2], old["suppressed_frames"][:, :2])
        assert same(c["adapted_os"], old["suppressed_os"]) and same(c["adapted_scores"], old["suppressed_scores"])
        assert not c["adapted_scores"][:, 2].any()  # the orientation score keeps its detection value
        idx = c["sorted_index"]
        assert idx.dtype == np.int32 and sorted(idx.tolist()) == list(range(n))
        for k in ("frames", "os", "scores"):
            assert same(c["adapted_" + k][idx], c["sorted_" + k])
        key = c["sorted_os"][:, 0].astype(np.int64) * 1000 + c["sorted_os"][:, 1]
        assert (np.diff(key) <= 0).all()
        scales = options["dsp_num_scales"] if options["domain_size_pooling"] else 1
        assert counts[5] == scales and counts[4] == (ref.cut(c["sorted_os"], options["max_num_features"]) if n else 0)
        if name in scenes.FLOAT_CASES:
            assert c["raw"].shape == (counts[4], scales, 128) and c["raw"].dtype == np.float32 and "digests" not in c
        else:
            assert c["digests"].shape == (counts[4], 32) and c["digests"].dtype == np.uint8 and "raw" not in c
        assert set(c) == {"image", "options", "counts", "sorted_index", "raw" if name in scenes.FLOAT_CASES else "digests"} | {
            s + "_" + k for s in ref.STAGES for k in ("frames", "os", "scores")}
        if name in scenes.EXITS:
            assert sum(scenes.EXITS[name]) == n


def test_golden_cases_cover_what_they_are_stored_for():
    g, v1 = ref.golden(), v1ref.golden()

    def anisotropic(c):
        f = c["sorted_frames"]
        return int(((f[:, 3] != 0) | (f[:, 2] != f[:, 5])).sum())
    assert anisotropic(g["mid"]) > 0 and anisotropic(g["checker17"]) == 1
    assert any(anisotropic(g[n]) for n in g) and anisotropic(g["upright"]) == 0
    # upright = 1 runs neither the orientations nor the adaptation: v1's `upright` case in every array the two files share
    # (this file's `adapted` list stands where v1 has its `oriented` one; its options carry the one key more)
    up, old = g["upright"], v1["upright"]
    assert (up["image"] == old["image"]).all() and up["counts"].tolist() == old["counts"].tolist()
    assert {k: v for k, v in up["options"].items() if k != "estimate_affine_shape"} == old["options"]
    for k in ("frames", "os", "scores"):
        assert same(up["adapted_" + k], old["oriented_" + k]) and same(up["sorted_" + k], old["sorted_" + k])
    assert same(up["sorted_index"], old["sorted_index"]) and same(up["digests"], old["digests"])
    # the three cuts against the (o, s) groups of the full run
    full = g["mid"]
    assert full["counts"][4] == 100 == len(full["sorted_os"])
    groups = groups_of(full["sorted_os"])
    totals = np.cumsum([n for _, n in groups]).tolist()
    assert scenes.MAXF_BETWEEN_GROUPS in totals[:-1] and g["maxf_groups"]["counts"][4] == scenes.MAXF_BETWEEN_GROUPS + 1
    later = [t for t in totals if t > scenes.MAXF_INSIDE_GROUP]
    assert scenes.MAXF_INSIDE_GROUP not in totals and len(later) >= 2 and g["maxf_inside"]["counts"][4] == later[0] + 1
    assert g["maxf_groups"]["counts"][0] == g["maxf_inside"]["counts"][0] == full["counts"][0]
    stopped = g["maxf_octaves"]
    assert stopped["counts"][0] < full["counts"][0] and stopped["counts"][0] >= scenes.MAXF_BETWEEN_OCTAVES
    assert stopped["sorted_os"][:, 0].min() > full["sorted_os"][:, 0].min()  # octave -1 was never searched
    # the cut keeps a prefix of the full run's sorted list
    for n in ("maxf_groups", "maxf_inside"):
        k = int(g[n]["counts"][4])
        assert same(g[n]["sorted_frames"], full["sorted_frames"]) and same(g[n]["digests"], full["digests"][:k])
    # patches that take the padded path and patches that do not
    c = g["first0"]
    o = c["options"]
    h, w = c["image"].shape
    sc = ref.scale_list(o["domain_size_pooling"], o["dsp_min_scale"], o["dsp_max_scale"], o["dsp_num_scales"])
    flags = [ref.patch_is_padded(f, s, w, h, o["first_octave"], o["octave_resolution"]) for f in c["sorted_frames"][:c["counts"][4]] for s in sc]
    assert 0 < sum(flags) < len(flags)
    assert g["flat40x30"]["counts"].tolist()[:5] == [0, 0, 0, 0, 0] and g["checker17"]["counts"].tolist()[2:] == [1, 1, 1, 10]
    assert max(len(set(c["sorted_os"][:, 0].tolist())) for c in g.values()) >= 3


@pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, "lib", "VLFeat")), reason="the reference tree is absent")
def test_golden_file_regenerates():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_covdet_affine_golden.py"), "--reference", REFERENCE, "--check"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "identical to the committed file" in r.stdout
