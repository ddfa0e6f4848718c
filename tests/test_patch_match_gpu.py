"""dsm_patch_match on the device against the normative restatement (tests/patch_match_ref.py): every output
array equal bit for bit.  The shapes are the smallest at which the kernels can go wrong: widths that are no multiple of 64,
frames whose sides swap under the rotation, a frame wider than one wave, an image lower than the window, every window
step, one and several source images of different sizes, more samples than a wave has items for, one and two iterations,
both filters, the photometric and the geometric pass.  Every case runs in the product's schedule (a wave per column) and in
the check build's (a lane per column, DSM_PATCH_MATCH_LANES): both equal the restatement, hence each other; one larger case at
the default options compares the two schedules only."""
import numpy as np
import pytest

from tests import patch_match_cases as cases

pytestmark = pytest.mark.gpu

A, B, C, D = (37, 23), (23, 37), (65, 9), (11, 5)

# name: (view sizes, reference, sources, options)
PHOTOMETRIC = {
    "37x23-r5-S3-n15": ((A, A, A, A), 0, (1, 2, 3), dict(window_radius=5, num_samples=15)),
    "23x37-r1-S1-n1-it2-filter": ((B, B), 0, (1,), dict(window_radius=1, num_samples=1, num_iterations=2, filter=True, filter_min_num_consistent=1)),
    "65x9-r7-step2-S5-n17-filter": ((C, A, B, C, (40, 30), (19, 21)), 0, (1, 2, 3, 4, 5), dict(window_radius=7, window_step=2, num_samples=17, filter=True)),
    "11x5-r5-lower-than-window": ((D, D, A, B), 0, (1, 2, 3), dict(window_radius=5, num_samples=3)),
    "37x23-S5-n1": ((A, B, A, C, A, B), 2, (0, 1, 3, 4, 5), dict(window_radius=2, num_samples=1, filter=True)),
    "23x37-r3-sigmas": ((B, A, B), 1, (0, 2), dict(window_radius=3, sigma_spatial=1.5, sigma_color=0.1, ncc_sigma=0.4, num_samples=4, filter=True,
                                                 filter_min_ncc=0.3, filter_min_triangulation_angle=1.0, incident_angle_sigma=0.5,
                                                 min_triangulation_angle=4.0)),
}


SCHEDULES = ["product", "lanes"]


def _select(monkeypatch, schedule):
    if schedule == "lanes":
        monkeypatch.setenv("DSM_PATCH_MATCH_LANES", "1")  # the check build's lane-per-column sweep


@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("name", sorted(PHOTOMETRIC))
def test_photometric_pass_equals_the_restatement(dsm, monkeypatch, name, schedule):
    _select(monkeypatch, schedule)
    sizes, ref_idx, srcs, kw = PHOTOMETRIC[name]
    kind = "step" if "S5" in name else "slanted"
    images, _ = cases.scene(kind, sizes)
    o = cases.options(**kw)
    problem = (ref_idx, list(srcs), 2.0, 8.0)
    want = cases.reference((kind, sizes), images, problem, o)
    got = dsm.patch_match(images, [problem], cases.capi_options(o))[0]
    cases.assert_same_bits(got, want, name)
    assert np.isfinite(want["depth"]).all()


def _with_truth_maps(images, truth):
    """The images with ground-truth depth and normal maps, float32: the input of a geometric pass."""
    out = []
    for im, t in zip(images, truth):
        im = dict(im)
        im["depth_map"], im["normal_map"] = t["depth"].astype(np.float32), t["normal"].astype(np.float32)
        out.append(im)
    return out


@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("filt", [False, True])
def test_geometric_pass_equals_the_restatement(dsm, monkeypatch, filt, schedule):
    _select(monkeypatch, schedule)
    sizes = (A, B, (30, 26), A)
    images, truth = cases.scene("step", sizes)
    fed = _with_truth_maps(images, truth)
    o = cases.options(window_radius=2, num_samples=4, geom_consistency=True, filter=filt, num_iterations=1)
    problem = (0, [1, 2, 3], 2.0, 8.0)
    want = cases.reference(("step-truth", sizes), fed, problem, o)
    got = dsm.patch_match(fed, [problem], cases.capi_options(o))[0]
    cases.assert_same_bits(got, want, "geometric filter=%s" % filt)
    if filt:
        assert want["mask"].any() and (want["depth"] > 0).any()


@pytest.mark.parametrize("schedule", SCHEDULES)
def test_two_pass_stereo_equals_the_restatements_two_passes(dsm, monkeypatch, schedule):
    from tests import patch_match_ref as ref
    _select(monkeypatch, schedule)
    sizes = (B, A, B)
    images, _ = cases.scene("slanted", sizes)
    o = cases.options(window_radius=2, num_samples=3, geom_consistency=True, filter=True)
    problems = [(0, [1, 2], 2.0, 8.0), (1, [0, 2], 2.5, 7.0), (2, [1, 0], 2.0, 8.0)]
    key = ("stereo", sizes)
    if key not in cases._cache:
        cases._cache[key] = ref.patch_match_stereo(images, problems, o)
    want = cases._cache[key]
    got = dsm.patch_match_stereo(images, problems, cases.capi_options(o))
    assert len(got) == len(want) == 3
    for k in range(3):
        cases.assert_same_bits(got[k], want[k], "problem %d" % k)


def test_larger_case_at_the_defaults_is_the_same_in_both_schedules(dsm, monkeypatch):
    """160 x 120, 5 source images, the default options (radius 5, 15 samples, 5 iterations, the geometric term, the filter),
    fed with the true depth and normal maps: the product's wave-per-column sweep against the check build's lane-per-column
    sweep, every byte."""
    from dagsfm_amd import capi
    images, truth = cases.scene("step", ((160, 120),) * 6)
    fed = _with_truth_maps(images, truth)
    problems = [(0, [1, 2, 3, 4, 5], 2.0, 8.0)]
    o = capi.default_patch_match_options(seed=5)
    product = dsm.patch_match(fed, problems, o)[0]
    monkeypatch.setenv("DSM_PATCH_MATCH_LANES", "1")
    lanes = dsm.patch_match(fed, problems, o)[0]
    cases.assert_same_bits(product, lanes, "product against the lane-per-column schedule")
    assert (product["depth"] > 0).mean() > 0.3 and product["mask"].any()


def test_stage_times_are_reported(dsm):
    images, _ = cases.scene("slanted", (A, A))
    dsm.patch_match(images, [(0, [1], 2.0, 8.0)], cases.capi_options(cases.options()))
    t = dsm.patch_match_time()
    assert list(t) == ["upload", "reference_filter", "initial_cost", "sweeps", "rotation", "download"]
    assert all(v >= 0 for v in t.values()) and t["sweeps"] > 0
