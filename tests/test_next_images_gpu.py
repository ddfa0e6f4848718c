"""dsm_find_next_images and dsm_find_local_bundles on the device against the restatement (tests/next_images_ref.py), on the product and on
the check build.  Everything is compared for equality: the image lists, the counts and the scores are integers, and the one
rank that rounds (the ratio, a float quotient) is a correctly rounded IEEE operation on both sides; the shared counts exactly
and tri_angle bit for bit -- the acos is correctly rounded and the percentile is an exact select.  Every local-bundle scene keeps
its tri_angle margins above 1e-9 under the restatement (tests/test_next_images_cpu.py holds that without a GPU)."""
import copy

import numpy as np
import pytest

from dagsfm_amd import capi
from tests import next_images_ref as ref
from tests import next_images_scenes as scenes
from tests.test_next_images_cpu import (CASES, broken, invalid_cases, lb_broken, lb_expected, lb_invalid_cases, same, same_bundles)

pytestmark = pytest.mark.gpu

_expected = {}


def expected(name, method=None):
    """The restatement's results of a named scene, computed once and left unchanged."""
    if (name, method) not in _expected:
        s, problems, kw = scenes.get(name)
        kw = dict(kw) if method is None else dict(kw, image_selection_method=method)
        _expected[(name, method)] = ref.find_next_images(s, problems, **kw)
    return _expected[(name, method)]


def options_of(name, method=None):
    kw = scenes.get(name)[2]
    return dict(kw) if method is None else dict(kw, image_selection_method=method)


@pytest.fixture(scope="module", params=["product", "check"])
def ctx(request):
    return capi.Context(0, check=request.param == "check")


@pytest.fixture(scope="module")
def check_ctx():
    """A context of the check build for the serial cross-check (the binding forwards DSM_NEXT_IMAGES_SERIAL from the
    environment before every call, so a test sets it with monkeypatch after its last call on `ctx`)."""
    return capi.Context(0, check=True)


@pytest.mark.parametrize("name,method", CASES)
def test_device_equals_the_restatement(ctx, name, method):
    s, problems, _ = scenes.get(name)
    out = ctx.find_next_images(s, problems, **options_of(name, method))
    exp = expected(name, method)
    same(out["results"], exp)
    rep = out["report"]
    assert rep.num_eligible == sum(len(e["next_image_ids"]) for e in exp) == rep.num_first_bucket + rep.num_second_bucket
    assert rep.num_batches == (1 if problems else 0) and rep.device_ms > 0


def test_report_counts_the_buckets(ctx):
    s, problems, _ = scenes.get("ranks")
    rep = ctx.find_next_images(s, problems, **options_of("ranks"))["report"]
    assert (rep.num_eligible, rep.num_first_bucket, rep.num_second_bucket) == (7, 5, 2)


@pytest.mark.parametrize("name,method", CASES)
def test_serial_check_schedule_equals_the_kernels(check_ctx, monkeypatch, name, method):
    s, problems, _ = scenes.get(name)
    par = check_ctx.find_next_images(s, problems, **options_of(name, method))["results"]
    monkeypatch.setenv("DSM_NEXT_IMAGES_SERIAL", "1")
    ser = check_ctx.find_next_images(s, problems, **options_of(name, method))["results"]
    same(ser, par)
    same(ser, expected(name, method))


@pytest.mark.parametrize("name", ["shared_images", "nothing_eligible", "random_1", "random_2"])
def test_a_batched_call_equals_single_problem_calls(ctx, name):
    s, problems, _ = scenes.get(name)
    batched = ctx.find_next_images(s, problems, **options_of(name))["results"]
    single = [ctx.find_next_images(s, [pr], **options_of(name))["results"][0] for pr in problems]
    same(batched, single)


@pytest.mark.parametrize("budget", [128 << 20, 1])
@pytest.mark.parametrize("name", ["shared_images", "random_3", "many_slots"])
def test_a_memory_budget_changes_no_byte(ctx, name, budget):
    """128 MiB holds these calls whole; a budget of one byte cuts them into one batch per problem."""
    s, problems, _ = scenes.get(name)
    try:
        ctx.set_memory_budget(budget)
        out = ctx.find_next_images(s, problems, **options_of(name))
    finally:
        ctx.set_memory_budget(0)
    same(out["results"], expected(name))
    assert out["report"].num_batches == (1 if budget > 1 else len(problems))


@pytest.mark.parametrize("name", ["shared_images", "duplicates", "random_1", "random_2", "random_3", "many_slots"])
def test_the_order_of_problems_pairs_and_matches_changes_nothing(ctx, name):
    s, problems, _ = scenes.get(name)
    s2, problems2, perm = scenes.permuted(s, problems, seed=5)
    out = ctx.find_next_images(s2, problems2, **options_of(name))["results"]
    exp = expected(name)
    same(out, [exp[k] for k in perm])


@pytest.mark.parametrize("label,fn", invalid_cases(), ids=[c[0] for c in invalid_cases()])
def test_invalid_arguments_leave_the_outputs_untouched(ctx, label, fn):
    s, problems, kw = broken(fn)
    with pytest.raises(capi.DsmError, match="dsm error 1:") as e:
        ctx.find_next_images(s, problems, **kw)
    assert all(not np.asarray(a).any() for a in e.value.outputs)


def test_an_unknown_camera_model_is_refused(ctx):
    s, problems, kw = copy.deepcopy(scenes.get("duplicates"))
    s["cameras"][0].model_id = 99
    with pytest.raises(capi.DsmError, match="dsm error 1:") as e:
        ctx.find_next_images(s, problems, **kw)
    assert all(not np.asarray(a).any() for a in e.value.outputs)


def test_too_small_a_capacity_is_out_of_range(ctx):
    s, problems, _ = scenes.get("ranks")
    with pytest.raises(capi.DsmError, match="dsm error 4:") as e:
        ctx.find_next_images(s, problems, capacity=6, **options_of("ranks"))
    assert all(not np.asarray(a).any() for a in e.value.outputs)
    same(ctx.find_next_images(s, problems, capacity=7, **options_of("ranks"))["results"], expected("ranks"))


def test_defaults_are_the_reference_s(ctx):
    o = capi.default_next_images_options()
    assert (o.image_selection_method, o.abs_pose_min_num_inliers, o.max_reg_trials) == (2, 30, 3)
    s, problems, _ = scenes.get("boundaries")
    same(ctx.find_next_images(s, problems)["results"], ref.find_next_images(s, problems))


# ================================================================== dsm_find_local_bundles
@pytest.mark.parametrize("name", scenes.LB_NAMES)
def test_local_bundles_equal_the_restatement(ctx, name):
    s, problems, queries, kw = scenes.lb_get(name)
    exp, margin = lb_expected(name)
    out = ctx.find_local_bundles(s, problems, queries, **kw)
    same_bundles(out["results"], exp)
    rep = out["report"]
    assert rep.min_tri_angle_margin == margin and rep.num_copied + rep.num_chained == len(queries)
    assert rep.num_chained == sum(1 for e in exp if len(e["overlap_image_ids"]) > kw.get("local_ba_num_images", 6) - 1)
    assert rep.num_angles == sum(1 for e in exp for a in e["overlap_tri_angle"] if a != -1.0)
    assert rep.num_filled == sum(e["accepted_at"].count(8) for e in exp) and rep.num_batches == (1 if queries else 0)


@pytest.mark.parametrize("name", scenes.LB_NAMES)
def test_local_bundles_serial_check_schedule_equals_the_kernels(check_ctx, monkeypatch, name):
    s, problems, queries, kw = scenes.lb_get(name)
    par = check_ctx.find_local_bundles(s, problems, queries, **kw)
    monkeypatch.setenv("DSM_NEXT_IMAGES_SERIAL", "1")
    ser = check_ctx.find_local_bundles(s, problems, queries, **kw)
    same_bundles(ser["results"], par["results"])
    same_bundles(ser["results"], lb_expected(name)[0])
    assert ser["report"].min_tri_angle_margin == par["report"].min_tri_angle_margin


@pytest.mark.parametrize("name", ["copy_and_chain", "queries", "random_2", "random_3"])
def test_batched_local_bundles_equal_single_query_calls(ctx, name):
    s, problems, queries, kw = scenes.lb_get(name)
    single = [ctx.find_local_bundles(s, [problems[p]], [(0, i)], **kw)["results"][0] for p, i in queries]
    same_bundles(single, lb_expected(name)[0])


@pytest.mark.parametrize("budget", [128 << 20, 1])
@pytest.mark.parametrize("name", ["sizes", "queries", "random_3"])
def test_a_memory_budget_changes_no_local_bundle(ctx, name, budget):
    """128 MiB holds these calls whole; a budget of one byte cuts them into one batch per query."""
    s, problems, queries, kw = scenes.lb_get(name)
    try:
        ctx.set_memory_budget(budget)
        out = ctx.find_local_bundles(s, problems, queries, **kw)
    finally:
        ctx.set_memory_budget(0)
    same_bundles(out["results"], lb_expected(name)[0])
    assert out["report"].num_batches == (1 if budget > 1 else len(queries))
    assert out["report"].min_tri_angle_margin == lb_expected(name)[1]


@pytest.mark.parametrize("name", ["copy_and_chain", "degenerate", "queries", "random_1", "random_2", "random_3"])
def test_the_order_of_problems_points_and_queries_changes_no_local_bundle(ctx, name):
    s, problems, queries, kw = scenes.lb_get(name)
    problems2, queries2, qperm = scenes.lb_permuted(problems, queries, seed=9)
    out = ctx.find_local_bundles(s, problems2, queries2, **kw)["results"]
    exp = lb_expected(name)[0]
    same_bundles(out, [exp[k] for k in qperm])


@pytest.mark.parametrize("label,fn", lb_invalid_cases(), ids=[c[0] for c in lb_invalid_cases()])
def test_invalid_local_bundle_arguments_leave_the_outputs_untouched(ctx, label, fn):
    s, problems, queries, kw = lb_broken(fn)
    with pytest.raises(capi.DsmError, match="dsm error 1:") as e:
        ctx.find_local_bundles(s, problems, queries, **kw)
    assert all(not np.asarray(a).any() for a in e.value.outputs)


def test_local_bundle_capacities(ctx):
    s, problems, queries, kw = scenes.lb_get("degenerate")
    exp = lb_expected("degenerate")[0]
    nb, no = sum(len(e["bundle_image_ids"]) for e in exp), sum(len(e["overlap_image_ids"]) for e in exp)
    for caps in ((nb - 1, no), (nb, no - 1)):
        with pytest.raises(capi.DsmError, match="dsm error 4:") as e:
            ctx.find_local_bundles(s, problems, queries, bundle_capacity=caps[0], overlap_capacity=caps[1], **kw)
        assert all(not np.asarray(a).any() for a in e.value.outputs)
    same_bundles(ctx.find_local_bundles(s, problems, queries, bundle_capacity=nb, overlap_capacity=no, **kw)["results"], exp)


def test_local_bundle_defaults_are_the_reference_s(ctx):
    o = capi.default_local_bundle_selection_options()
    assert (o.local_ba_num_images, o.local_ba_min_tri_angle) == (6, 6.0)
