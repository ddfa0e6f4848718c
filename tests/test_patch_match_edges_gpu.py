"""dsm_patch_match at its edges: a batch of problems of different sizes in one call, the same batch cut into chunks by the
memory budget and in another order (identical bytes per problem), geometry that sends every patch off the source images,
no source images, no problems, and every invalid option."""
import numpy as np
import pytest

from tests import patch_match_cases as cases

pytestmark = pytest.mark.gpu

SIZES = ((37, 23), (23, 37), (30, 26), (37, 23))
PROBLEMS = [(0, [1, 2, 3], 2.0, 8.0), (1, [0, 3], 2.5, 7.0), (2, [3, 0, 1], 2.0, 9.0)]


def _opts():
    return cases.options(window_radius=2, num_samples=3, filter=True, filter_min_num_consistent=1)


def _references(images):
    return [cases.reference(("slanted", SIZES), images, p, _opts()) for p in PROBLEMS]


@pytest.mark.parametrize("schedule", ["product", "lanes"])
def test_batch_of_three_problems_in_one_call(dsm, monkeypatch, schedule):
    if schedule == "lanes":
        monkeypatch.setenv("DSM_PATCH_MATCH_LANES", "1")  # the check build's lane-per-column sweep
    images, _ = cases.scene("slanted", SIZES)
    got = dsm.patch_match(images, PROBLEMS, cases.capi_options(_opts()))
    for k, want in enumerate(_references(images)):
        cases.assert_same_bits(got[k], want, "problem %d" % k)


def test_memory_budget_cuts_the_batch_without_changing_a_byte(dsm):
    images, _ = cases.scene("slanted", SIZES)
    dsm.set_memory_budget(1)  # one problem always runs: three chunks
    try:
        got = dsm.patch_match(images, PROBLEMS, cases.capi_options(_opts()))
    finally:
        dsm.set_memory_budget(0)
    for k, want in enumerate(_references(images)):
        cases.assert_same_bits(got[k], want, "problem %d under a budget" % k)


def test_problem_order_does_not_change_a_byte(dsm):
    images, _ = cases.scene("slanted", SIZES)
    order = [2, 0, 1]
    got = dsm.patch_match(images, [PROBLEMS[k] for k in order], cases.capi_options(_opts()))
    want = _references(images)
    for slot, k in enumerate(order):
        cases.assert_same_bits(got[slot], want[k], "problem %d in slot %d" % (k, slot))


def test_source_camera_behind_the_plane(dsm):
    """A source camera on the far side of the surface, looking back at it: every homography has a negative or vanishing
    plane distance somewhere; the results are the restatement's, and nothing faults."""
    images, _ = cases.scene("slanted", ((37, 23), (37, 23), (23, 37)))
    images = [dict(im) for im in images]
    R = np.diag([1.0, -1.0, -1.0])  # looks along -z from (0, 0, 9)
    images[1]["R"] = R.reshape(9).astype(np.float32)
    images[1]["T"] = (-R @ np.array([0.0, 0.0, 9.0])).astype(np.float32)
    o = cases.options(window_radius=2, num_samples=3, filter=True, filter_min_num_consistent=0)
    problem = (0, [1, 2], 2.0, 8.0)
    want = cases.reference(("behind", 0), images, problem, o)
    got = dsm.patch_match(images, [problem], cases.capi_options(o))[0]
    cases.assert_same_bits(got, want, "behind the plane")


def test_depth_range_that_leaves_every_source_image(dsm):
    images, _ = cases.scene("slanted", ((37, 23), (37, 23), (23, 37)))
    o = cases.options(window_radius=2, num_samples=3, filter=True)
    problem = (0, [1, 2], 0.01, 0.02)
    want = cases.reference(("slanted", "near"), images, problem, o)
    got = dsm.patch_match(images, [problem], cases.capi_options(o))[0]
    cases.assert_same_bits(got, want, "off every source image")
    assert not want["mask"].any() and not want["depth"].any()  # every cost is the maximum: nothing survives the filter


@pytest.mark.parametrize("filt", [False, True])
def test_zero_source_images(dsm, filt):
    images, _ = cases.scene("slanted", ((37, 23), (37, 23), (23, 37)))
    o = cases.options(window_radius=2, num_samples=3, filter=filt)
    problem = (0, [], 2.0, 8.0)
    want = cases.reference(("slanted", "alone"), images, problem, o)
    got = dsm.patch_match(images, [problem], cases.capi_options(o))[0]
    cases.assert_same_bits(got, want, "no source images")
    assert got["sel_prob"].shape == (0, 23, 37)
    if filt:
        assert not got["depth"].any() and not got["normal"].any()
    else:
        assert (got["depth"] > 0).all()


def test_empty_batch(dsm):
    images, _ = cases.scene("slanted", ((37, 23), (37, 23), (23, 37)))
    assert dsm.patch_match(images, [], cases.capi_options(cases.options())) == []
    assert dsm.patch_match([], [], cases.capi_options(cases.options())) == []


INVALID = [dict(window_radius=0), dict(window_radius=33), dict(window_step=0), dict(window_step=3), dict(sigma_color=0.0),
           dict(num_samples=0), dict(ncc_sigma=0.0), dict(min_triangulation_angle=-1.0), dict(min_triangulation_angle=180.0),
           dict(incident_angle_sigma=0.0), dict(num_iterations=0), dict(geom_consistency_regularizer=-0.1),
           dict(geom_consistency_max_cost=-1.0), dict(filter_min_ncc=-1.5), dict(filter_min_ncc=1.5),
           dict(filter_min_triangulation_angle=-1.0), dict(filter_min_triangulation_angle=181.0), dict(filter_min_num_consistent=-1),
           dict(filter_geom_consistency_max_cost=-1.0), dict(sigma_color=float("nan")), dict(ncc_sigma=float("nan"))]


@pytest.mark.parametrize("bad", INVALID, ids=lambda d: "%s=%s" % next(iter(d.items())))
def test_every_invalid_option_is_refused(dsm, bad):
    from dagsfm_amd import capi
    from tests import patch_match_ref as ref
    images, _ = cases.scene("slanted", ((37, 23), (37, 23), (23, 37)))
    o = capi.default_patch_match_options(geom_consistency=0, **bad)
    with pytest.raises(capi.DsmError, match="dsm_patch_match: "):
        dsm.patch_match(images, [(0, [1, 2], 2.0, 8.0)], o)
    assert ref.Options(**bad).check() is not None  # the restatement refuses the same options


@pytest.mark.parametrize("problem", [(0, [1, 2], 0.0, 8.0), (0, [1, 2], -1.0, 8.0), (0, [1, 2], 5.0, 4.0), (0, [1, 7], 2.0, 8.0),
                                     (0, [1, 2], float("nan"), 8.0)])
def test_invalid_problems_are_refused(dsm, problem):
    from dagsfm_amd import capi
    images, _ = cases.scene("slanted", ((37, 23), (37, 23), (23, 37)))
    with pytest.raises(capi.DsmError, match="dsm_patch_match: "):
        dsm.patch_match(images, [problem], cases.capi_options(cases.options()))


def test_geometric_pass_without_maps_is_refused(dsm):
    from dagsfm_amd import capi
    images, _ = cases.scene("slanted", ((37, 23), (37, 23), (23, 37)))
    with pytest.raises(capi.DsmError, match="geom_consistency without"):
        dsm.patch_match(images, [(0, [1, 2], 2.0, 8.0)], cases.capi_options(cases.options(geom_consistency=True)))
