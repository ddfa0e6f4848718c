"""dsm_update_tracks on the device against the restatement (tests/track_update_ref.py) and the hand-computed
answers of tests/track_update_scenes.py: ids, track order, modified ids, step counts and trial counts exactly, xyz bit for bit.
Every scene keeps its decision margins above 1e-9 under the restatement (tests/test_track_update_cpu.py holds that without a
GPU)."""
import numpy as np
import pytest

from dagsfm_amd import capi
from tests import track_update_ref as ref
from tests import track_update_scenes as scenes

pytestmark = pytest.mark.gpu
MERGE, COMPLETE = ref.MERGE, ref.COMPLETE
CASES, invalid_cases, random_scene = scenes.CASES, scenes.invalid_cases, scenes.named_random_scene

_expected = {}


def expected(key, scene, steps, selected=None, **options):
    """The restatement's result of a named scene and step order, computed once and left unchanged."""
    k = (key, tuple(steps))
    if k not in _expected:
        _expected[k] = ref.update_tracks(scene, steps, selected, **options)
        assert ref.min_margin(_expected[k]) >= scenes.MIN_MARGIN
    return _expected[k]


def result_bytes(r):
    return b"".join(np.ascontiguousarray(r[k]).tobytes() for k in ("point_ids", "xyz", "track_offsets", "track_obs", "modified", "step_counts"))


@pytest.fixture(scope="module", params=["product", "check"])
def ctx(request):
    return capi.Context(0, check=request.param == "check")


@pytest.mark.parametrize("name", sorted(CASES))
def test_known_answer(ctx, name):
    c = CASES[name]
    got = ctx.update_tracks(c["scene"], c["steps"], c["selected"], **c["options"])
    scenes.check_case(c, got)
    ct, mt = scenes.trial_counts(got)
    assert c["complete_trials"] in (None, ct) and c["merge_trials"] in (None, mt), (ct, mt)
    scenes.same_result(got, expected(name, c["scene"], c["steps"], c["selected"], **c["options"]))


@pytest.mark.parametrize("L", [16, 17, 30, 31, 62, 63, 64, 65, 257])
def test_long_tracks(ctx, L):
    """16 / 17: the last track on a lane and the first on a wave in COMPLETE; 30 / 31: with B's two elements the component holds
    32 and 33 track elements, the last on a lane and the first on a wave in MERGE; 62 / 63: the all-inlier test fills one run of
    64 lanes and starts a second; 64, 65, 257: runs that end inside the first track."""
    s = scenes.long_track(L)
    for steps in scenes.STEP_ORDERS:
        scenes.same_result(ctx.update_tracks(s, steps), expected(("long", L), s, steps))


@pytest.mark.parametrize("track", [2, 17], ids=["lane", "wave"])
@pytest.mark.parametrize("K", [1, 63, 64, 65, 130])
def test_candidates_of_one_level(ctx, K, track):
    """On the wave path 64 candidates are one full ballot, 65 one and a tail of one lane, 130 two and a tail of two."""
    s = scenes.wide_level(K, track)
    got = ctx.update_tracks(s, [COMPLETE])
    scenes.same_result(got, expected(("wide", K, track), s, [COMPLETE]))
    assert int(got["step_counts"][0]) == 2 * K and got["report"].complete_serial_steps == 0


def test_wave_accepted_list_overflow(ctx):
    """A wave walk that accepts more features than its list in LDS holds (2 048) ends the rounds; the serial form finishes."""
    s = scenes.wide_level(1100, 17)
    got = ctx.update_tracks(s, [COMPLETE])
    scenes.same_result(got, expected(("wide", 1100, 17), s, [COMPLETE]))
    assert int(got["step_counts"][0]) == 2200 and got["report"].complete_serial_steps == 1


@pytest.mark.parametrize("k", [1, 2, 9])
def test_claim_chain_rounds(ctx, k):
    """k points, each contesting one feature with the next: the claim rounds equal the chain."""
    s = scenes.claim_chain(k)
    got = ctx.update_tracks(s, [COMPLETE])
    scenes.same_result(got, expected(("chain", k), s, [COMPLETE]))
    assert got["report"].complete_rounds == k and got["report"].complete_serial_steps == 0


@pytest.mark.parametrize("n", [1, 2, 64, 65])
def test_component_sizes(ctx, n):
    s = scenes.merge_chain(n)
    got = ctx.update_tracks(s, [MERGE])
    scenes.same_result(got, expected(("component", n), s, [MERGE]))
    assert (got["report"].num_components, got["report"].largest_component) == (1, n)
    assert int(got["report"].num_merge_events) == n - 1


@pytest.mark.parametrize("name", ["small", "unregistered", "forty"])
@pytest.mark.parametrize("steps", scenes.STEP_ORDERS, ids=["complete_merge", "merge_complete"])
def test_random_scenes(ctx, name, steps):
    """forty: 40 images with a third of the observations stripped and some points split in two."""
    s = random_scene(name)
    got = ctx.update_tracks(s, steps)
    scenes.same_result(got, expected(name, s, steps))
    assert got["report"].num_components > 1 and got["report"].complete_rounds >= 1


def test_wrappers_and_selection(ctx):
    s = random_scene("medium")
    scenes.same_result(ctx.complete_and_merge_tracks(s), expected("medium", s, [COMPLETE, MERGE]))
    ids = np.sort(np.asarray(s["point3D_ids"]))[::3]
    scenes.same_result(ctx.merge_and_complete_tracks(s, ids), ref.update_tracks(s, [MERGE, COMPLETE], ids))
    steps = [COMPLETE, MERGE, MERGE, COMPLETE]
    scenes.same_result(ctx.update_tracks(s, steps), ref.update_tracks(s, steps))


def test_same_bytes_across_repeats_and_input_orders(ctx):
    s = random_scene("forty")
    for steps in scenes.STEP_ORDERS:
        base = result_bytes(ctx.update_tracks(s, steps))
        assert result_bytes(ctx.update_tracks(s, steps)) == base
        assert result_bytes(ctx.update_tracks(scenes.shuffled_points(s, 3), steps)) == base
        assert result_bytes(ctx.update_tracks(scenes.shuffled_matches(s, 4), steps)) == base


def test_serial_form_and_exhausted_pool_give_the_same_bytes(monkeypatch):
    """The check build's DSM_TRACK_UPDATE_SERIAL=1 (the reference's loops on one lane) and a claim pool of three entries (the
    rounds give way to the serial form) against the product."""
    s = random_scene("forty")
    product = capi.Context(0, check=False)
    base = {tuple(steps): ctx_result for steps, ctx_result in ((tuple(st), product.update_tracks(s, st)) for st in scenes.STEP_ORDERS)}
    for value in ("1", "pool:3"):
        monkeypatch.setenv("DSM_TRACK_UPDATE_SERIAL", value)
        check = capi.Context(0)
        assert check.check
        for steps in scenes.STEP_ORDERS:
            got = check.update_tracks(s, steps)
            scenes.same_result(got, base[tuple(steps)])
            assert result_bytes(got) == result_bytes(base[tuple(steps)])
            assert got["report"].complete_serial_steps == 1
    monkeypatch.delenv("DSM_TRACK_UPDATE_SERIAL")


@pytest.mark.parametrize("case", invalid_cases(), ids=lambda c: c[0])
def test_invalid_arguments(ctx, case):
    _, s, steps, selected, next_id, kw = case
    with pytest.raises(capi.DsmError):
        ctx.update_tracks(s, steps, selected, next_id, **kw)
