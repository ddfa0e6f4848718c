"""Global rotation averaging at the sizes, options, inputs and graph shapes the first test file leaves out: grids of more than
256 blocks (the strided loop of sum_partials), block-boundary sizes, every option against the restatement with the same
option, DSM_ERR_NOT_CONVERGED and the state it leaves, the cold restart of the warm-started solver, ceres' conversions at
q / -q, w = 0 and near pi, hubs, extreme ids, and the n_pairs refusal.

Every device comparison asserts what tests/test_rotation_averaging.py::_compare asserts, that no stopping decision of the
restatement sits within 1e-6 of its threshold, and the property that makes the fixture worth having, read from the report."""
import ctypes

import numpy as np
import pytest

from tests import rotation_averaging_ref as ref
from tests.test_rotation_averaging import _compare, _edges_random, _graph, _qmul, _qvecs, _rand_q, _same_bytes

RA_BLOCK = 256
# restatement keyword -> dsm_rotation_averaging_options field
_OPT = {"max_num_l1_iterations": "max_num_l1_iterations", "max_num_irls_iterations": "max_num_irls_iterations",
        "l1_thr": "l1_step_convergence_threshold", "irls_thr": "irls_step_convergence_threshold", "sigma": "irls_loss_parameter_sigma",
        "admm_initial": "admm_initial_max_iterations", "rho": "admm_rho", "alpha": "admm_alpha", "abs_tol": "admm_absolute_tolerance",
        "rel_tol": "admm_relative_tolerance", "filter_degrees": "max_relative_rotation_difference_degrees"}


def _blocks(n):
    return -(-n // RA_BLOCK)


def _expect(p, q, partition=None, **kw):
    exp = ref.rotation_averaging(p, q, partition=partition, **kw)
    assert ref.min_margin(exp["decisions"]) > 1e-6, "fixture on a knife edge"
    return exp


def _check(dsm, p, q, partition=None, **kw):
    """device == restatement under the same options; returns (device, restatement)"""
    from dagsfm_amd import capi
    exp = _expect(p, q, partition, **kw)
    dev = dsm.rotation_averaging(p, q, options=capi.default_rotation_averaging_options(**{_OPT[k]: v for k, v in kw.items()}))
    _compare(dev, exp)
    return dev, exp


def _whole(p):
    """the partition with one block holding every image: the restatement's dense Cholesky, formed once per system"""
    return [np.unique(p)], []


def _near_identity_q(rng, n, spread):
    q = np.hstack([np.ones((n, 1)), rng.normal(scale=spread, size=(n, 3))])
    return q / np.linalg.norm(q, axis=1, keepdims=True)


def _hub_cliques(n_hub=64, n_cl=8256, k=8, seed=41):
    """n_hub sub-hubs joined as a clique; n_cl cliques of k images, each image also joined to one sub-hub.  Ids shuffled,
    noise 0.002, 1 % of the edges corrupted.  Returns (pairs, qvecs, partition of ids: (cliques, sub-hubs))."""
    rng = np.random.default_rng(seed)
    hub = np.arange(n_hub)
    iu, ju = np.triu_indices(n_hub, 1)
    base = n_hub + np.arange(n_cl)[:, None] * k + np.arange(k)[None, :]
    bi, bj = np.triu_indices(k, 1)
    pairs = np.vstack([np.stack([iu, ju], 1), np.stack([base[:, bi].ravel(), base[:, bj].ravel()], 1),
                       np.stack([base.ravel(), rng.integers(0, n_hub, base.size)], 1)])
    n = n_hub + n_cl * k
    absq = _near_identity_q(rng, n, 0.3)  # orientations within ~0.5 rad of each other: the L1 loop converges in 4 iterations
    q = _qvecs(rng, absq, pairs, 0.002, rng.choice(len(pairs), len(pairs) // 100, replace=False))
    ids = rng.permutation(n).astype(np.int64) * 3 + 5
    o = rng.permutation(len(pairs))
    return ids[pairs][o].astype(np.uint32), q[o], (ids[base], ids[hub])


def _tree_plus(seed, n_img, n_extra, noise=0.01):
    """a random spanning tree of n_img images plus n_extra further edges"""
    rng = np.random.default_rng(seed)
    e = [(int(rng.integers(0, v)), v) for v in range(1, n_img)]
    s = set(e)
    while len(s) < n_img - 1 + n_extra:
        a, b = sorted(int(x) for x in rng.choice(n_img, 2, replace=False))
        s.add((a, b))
    pairs = np.array(e + sorted(s - set(e)), np.int64)
    return _graph(seed, n_img, pairs, noise=noise)


# ---------------------------------------------------------------- CPU: the restatement itself
def _random_partitioned_graph(rng, n_blocks, n_sep):
    sizes = rng.integers(1, 7, n_blocks)
    start = n_sep + np.concatenate([[0], np.cumsum(sizes)[:-1]])
    N = n_sep + int(sizes.sum())
    e = set()
    for a in range(n_sep):
        for b in range(a + 1, n_sep):
            if rng.random() < 0.5 or b == a + 1:
                e.add((a, b))
    blocks = []
    for s0, sz in zip(start, sizes):
        m = list(range(s0, s0 + sz))
        blocks.append(m)
        for a, b in zip(m[:-1], m[1:]):  # a chain keeps the block connected
            e.add((a, b))
        for _ in range(int(sz)):
            a, b = sorted(int(x) for x in rng.choice(m, 2)) if sz > 1 else (m[0], m[0])
            if a != b:
                e.add((a, b))
        for t in rng.choice(n_sep, int(rng.integers(1, 3)), replace=False):
            e.add((int(t), int(rng.choice(m))))
    ed = np.array(sorted(e), np.int64)
    return N, ed[:, 0], ed[:, 1], blocks, list(range(n_sep))


@pytest.mark.parametrize("grounded", ["separator", "block"])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_block_solve_equals_dense_cholesky(seed, grounded):
    rng = np.random.default_rng(seed)
    N, ei, ej, blocks, sep = _random_partitioned_graph(rng, 40, 6)
    # component index 0 is grounded: relabel so that it is a separator image or a block image
    g = 0 if grounded == "separator" else blocks[int(rng.integers(0, len(blocks)))][0]
    perm = np.arange(N)
    perm[[0, g]] = perm[[g, 0]]
    ei, ej = perm[ei], perm[ej]
    blocks = [[int(perm[v]) for v in b] for b in blocks]
    sep = [int(perm[v]) for v in sep]
    assert (0 in sep) == (grounded == "separator")
    groups, sep_c = ref._partition_groups((blocks, sep), np.arange(N))
    w = rng.uniform(0.1, 10.0, len(ei))
    rhs = rng.normal(size=(N - 1, 3))
    x = ref.BlockFactor(N, ei, ej, w, groups, sep_c).solve(rhs)
    xd = ref._chol_solve(ref._laplacian(N, ei, ej, w), rhs)
    assert np.abs(x - xd).max() <= 1e-13 * np.abs(xd).max()


def test_block_factor_refuses_an_edge_between_blocks():
    with pytest.raises(ValueError):
        ref.BlockFactor(5, np.array([0, 1, 2]), np.array([1, 2, 3]), np.ones(3), [np.array([[1, 2], [3, 4]])], np.zeros(0, np.int64))


def test_partitioned_restatement_equals_dense():
    n = 200
    pairs = np.vstack([_edges_random(np.random.default_rng(7), n, 5)])
    # a partition that is valid for any graph: one block holding every image
    p, q, _, _ = _graph(8, n, pairs, noise=0.004, n_corrupt=6)
    a = ref.rotation_averaging(p, q)
    b = ref.rotation_averaging(p, q, partition=([np.unique(p)], []))
    assert ref.angle_between(a["orientations"], b["orientations"]).max() < 1e-12
    assert np.array_equal(a["edge_state"], b["edge_state"]) and a["report"]["admm_iterations"] == b["report"]["admm_iterations"]
    assert [d[0] for d in a["decisions"]] == [d[0] for d in b["decisions"]]


def test_zero_iteration_options():
    p, q, _, _ = _graph(9, 40, _edges_random(np.random.default_rng(9), 40, 6), noise=0.004)
    none = ref.rotation_averaging(p, q, max_num_l1_iterations=0, max_num_irls_iterations=0)
    assert (none["orientations"] == 0.0).all() and none["report"]["num_l1_iterations"] == 0
    assert none["report"]["num_irls_iterations"] == 0 and none["report"]["admm_iterations"] == []
    assert {d[0] for d in none["decisions"]} == {"filter"}
    irls = ref.rotation_averaging(p, q, max_num_l1_iterations=0)
    assert irls["report"]["num_l1_iterations"] == 0 and irls["report"]["num_irls_iterations"] > 0
    assert {d[0] for d in irls["decisions"]} == {"irls_step", "filter", "cold"}
    l1 = ref.rotation_averaging(p, q, max_num_irls_iterations=0)
    assert l1["report"]["num_l1_iterations"] > 0 and l1["report"]["num_irls_iterations"] == 0
    assert "irls_step" not in {d[0] for d in l1["decisions"]}


def test_cold_restart_is_recorded_and_zero_threshold_margin():
    p, q, _, _ = _graph(13, 40, _edges_random(np.random.default_rng(13), 40, 8), noise=0.002, n_corrupt=10)
    dec = ref.rotation_averaging(p, q)["decisions"]
    cold = [d for d in dec if d[0] == "cold"]
    assert cold and ref.cold_restarts(dec) > 0 and ref.cold_restarts(dec) < len(cold)
    assert ref.min_margin([("filter", 0.25, 0.0)]) == 0.25 and ref.min_margin([("x", 3.0, 2.0)]) == 0.5


# ---------------------------------------------------------------- GPU: grid sizes
@pytest.mark.gpu
def test_more_than_256_blocks_of_images_and_of_edges(dsm):
    p, q, part = _hub_cliques()
    dev, exp = _check(dsm, p, q, partition=part)
    r = dev["report"]
    assert _blocks(r.num_images) > 256 and _blocks(r.num_edges) > 256, (r.num_images, r.num_edges)
    assert ref.cold_restarts(exp["decisions"]) > 0
    assert r.num_filtered_edges > 0 and r.num_final_images > 0.99 * r.num_images


@pytest.mark.gpu
def test_more_than_256_blocks_of_edges_dense_restatement(dsm):
    from dagsfm_amd import capi
    n = 2000
    p, q, _, _ = _graph(51, n, _edges_random(np.random.default_rng(51), n, 40), noise=0.003, n_corrupt=800)
    dev, exp = _check(dsm, p, q, partition=_whole(p))
    assert _blocks(dev["report"].num_edges) > 256 and _blocks(dev["report"].num_images) < 256
    assert ref.cold_restarts(exp["decisions"]) > 0
    for batch in (7, 4096):
        _same_bytes(dev, dsm.rotation_averaging(p, q, options=capi.default_rotation_averaging_options(cg_batch_iterations=batch)))
    o = np.random.default_rng(2).permutation(len(p))
    devp = dsm.rotation_averaging(p[o], q[o])
    inv = np.argsort(o)
    assert devp["edge_state"][inv].tobytes() == dev["edge_state"].tobytes()
    assert devp["relative_rotations"][inv].tobytes() == dev["relative_rotations"].tobytes()
    assert devp["orientations"].tobytes() == dev["orientations"].tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("n_img,n_edges", [(2, 1), (256, 255), (256, 256), (256, 257), (257, 256), (257, 257), (257, 258)])
def test_block_boundary_sizes(dsm, n_img, n_edges):
    p, q, _, _ = _tree_plus(60 + n_img + n_edges, n_img, n_edges - (n_img - 1))
    dev, _ = _check(dsm, p, q)
    r = dev["report"]
    assert (r.num_images, r.num_edges) == (n_img, n_edges)
    if n_edges == n_img - 1:  # a spanning tree: every edge is fitted exactly
        assert r.num_filtered_edges == 0 and (dev["edge_state"] == 3).all()


# ---------------------------------------------------------------- GPU: options
def _sweep_graph(noise=0.005):
    """150 images with orientations within ~0.5 rad of each other, so that ADMM stops on its tolerances before its cap"""
    rng = np.random.default_rng(71)
    pairs = _edges_random(rng, 150, 10)
    q = _qvecs(rng, _near_identity_q(rng, 150, 0.3), pairs, noise, rng.choice(len(pairs), 20, replace=False))
    return pairs.astype(np.uint32), q


OPTION_CASES = {
    "alpha_1.5": dict(alpha=1.5),
    "rho_0.5": dict(rho=0.5),
    "rho_2": dict(rho=2.0),
    "admm_initial_1": dict(admm_initial=1),
    "tolerances": dict(abs_tol=3e-3, rel_tol=0.2),
    "l1_0": dict(max_num_l1_iterations=0),
    "l1_1": dict(max_num_l1_iterations=1),
    "l1_8": dict(max_num_l1_iterations=8, l1_thr=1e-7),
    "irls_0": dict(max_num_irls_iterations=0),
    "irls_1": dict(max_num_irls_iterations=1, max_num_l1_iterations=2),  # the defaults' IRLS would go on
    "sigma_1deg": dict(sigma=1.0 * ref.DEG2RAD),
    "sigma_20deg": dict(sigma=20.0 * ref.DEG2RAD),
    "step_thresholds_0": dict(l1_thr=0.0, irls_thr=0.0, max_num_irls_iterations=3),
    "filter_0deg": dict(filter_degrees=0.0),
    "filter_180deg": dict(filter_degrees=180.0),
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(OPTION_CASES))
def test_options_against_restatement(dsm, case):
    kw = OPTION_CASES[case]
    p, q = _sweep_graph(0.03 if case == "filter_0deg" else 0.005)  # filter 0: every loop error well away from 0
    dev, exp = _check(dsm, p, q, **kw)
    base = ref.rotation_averaging(p, q)
    r, rb = dev["report"], base["report"]
    # the option changes what is computed: the run differs from the defaults'
    changed = (list(r.admm_iterations)[:r.num_l1_iterations] != rb["admm_iterations"] or r.num_irls_iterations != rb["num_irls_iterations"]
               or ref.angle_between(dev["orientations"], base["orientations"]).max() > 1e-6
               or not np.array_equal(dev["edge_state"], base["edge_state"]))
    assert changed
    if "max_num_l1_iterations" in kw:
        assert r.num_l1_iterations == kw["max_num_l1_iterations"]
    if "max_num_irls_iterations" in kw:
        assert r.num_irls_iterations == kw["max_num_irls_iterations"]
    if kw.get("l1_thr") == 0.0:
        assert r.num_l1_iterations == 5 and r.last_l1_step > 0.0
    if case == "l1_0" or case == "irls_0":
        assert np.isfinite(dev["orientations"]).all()
    if case == "filter_0deg":  # every edge goes, every image is alone, the smallest id wins the tie
        assert (dev["edge_state"] == 2).all() and r.num_final_images == 1 and dev["in_final_cc"][0] and not dev["in_final_cc"][1:].any()
    if case == "filter_180deg":
        assert (dev["edge_state"] == 3).all() and r.num_final_images == r.num_images and rb["num_filtered_edges"] > 0


@pytest.mark.gpu
def test_no_l1_and_no_irls_iterations_leave_zero_orientations(dsm):
    p, q = _sweep_graph()
    dev, _ = _check(dsm, p, q, max_num_l1_iterations=0, max_num_irls_iterations=0)
    assert (dev["orientations"] == 0.0).all() and dev["report"].total_cg_iterations == 0


# ---------------------------------------------------------------- GPU: DSM_ERR_NOT_CONVERGED
def _raw_call(ctx, p, q, options):
    """the C-ABI directly, with output buffers pre-filled with garbage"""
    from dagsfm_amd import capi
    n = len(p)
    p = np.ascontiguousarray(p, np.uint32)
    q = np.ascontiguousarray(q, np.float64)
    out = {"image_ids": np.full(2 * n, 0xABCD, np.uint32), "orientations": np.full((2 * n, 3), 7.0), "in_final_cc": np.full(2 * n, 9, np.uint8),
           "edge_state": np.full(n, 0xAA, np.uint8), "relative_rotations": np.full((n, 3), 5.0)}
    nimg = ctypes.c_uint32(12345)
    rep = capi.RotationAveragingReport()
    rc = ctx._L.dsm_view_graph_rotation_averaging(ctx._h, n, p.ctypes.data, q.ctypes.data, None, ctypes.byref(options),
                                                  out["image_ids"].ctypes.data, out["orientations"].ctypes.data, out["in_final_cc"].ctypes.data,
                                                  ctypes.addressof(nimg), out["edge_state"].ctypes.data, out["relative_rotations"].ctypes.data,
                                                  ctypes.addressof(rep))
    return rc, ctx._L.dsm_last_error(ctx._h).decode(), nimg.value, rep, out


@pytest.mark.gpu
def test_not_converged_status_and_what_it_leaves():
    from dagsfm_amd import capi
    p, q, _, _ = _graph(81, 300, _edges_random(np.random.default_rng(81), 300, 10), noise=0.005, n_corrupt=10)
    ctx = capi.Context(0)
    rc, msg, nimg, rep, out = _raw_call(ctx, p, q, capi.default_rotation_averaging_options(max_num_cg_iterations=2))
    assert rc == capi.DSM_ERR_NOT_CONVERGED == 6, (rc, msg)
    assert "conjugate-gradient" in msg and "relative residual" in msg
    assert (out["edge_state"] == 0).all() and nimg == 0
    assert rep.max_cg_relative_residual > 1e-9 and rep.total_cg_iterations > 0 and rep.num_images == 300
    # the next call on the same context is unaffected
    after = ctx.rotation_averaging(p, q)
    fresh = capi.Context(0).rotation_averaging(p, q)
    _same_bytes(after, fresh)
    assert after["report"].total_cg_iterations == fresh["report"].total_cg_iterations
    # the same iteration cap with a residual bound it meets is a normal return
    rc, msg, nimg, rep, out = _raw_call(ctx, p, q, capi.default_rotation_averaging_options(max_num_cg_iterations=2, cg_max_residual=1.0))
    assert rc == 0, msg
    assert nimg == 300 and rep.max_cg_relative_residual > 1e-9 and set(np.unique(out["edge_state"])) <= {2, 3}


# ---------------------------------------------------------------- GPU: rotations
@pytest.mark.gpu
def test_negated_qvecs_give_the_same_bytes(dsm):
    p, q, _, _ = _graph(91, 60, _edges_random(np.random.default_rng(91), 60, 6), noise=0.004, n_corrupt=5)
    flip = np.random.default_rng(92).random(len(q)) < 0.5
    assert flip.any() and (q[:, 0] != 0.0).all()
    qn = np.where(flip[:, None], -q, q)
    dev = dsm.rotation_averaging(p, q)
    devn = dsm.rotation_averaging(p, qn)
    _same_bytes(dev, devn)
    _compare(devn, _expect(p, qn))


def _pi_graph(seed, n=40):
    """a graph whose tree edges (v - 1, v) for v = 1, 5, 9 carry a relative rotation of exactly pi (w = 0), for v = 2, 6 one
    within 1e-9 of pi; the other edges are noisy"""
    rng = np.random.default_rng(seed)
    pairs = np.vstack([np.stack([np.arange(n - 1), np.arange(1, n)], 1), _edges_random(rng, n, 3)])
    pairs = np.unique(np.sort(pairs, axis=1), axis=0)
    absq = _rand_q(rng, n)
    special = {}
    for v, theta in ((1, np.pi), (5, np.pi), (9, np.pi), (2, np.pi - 1e-9), (6, np.pi - 1e-9)):
        ax = rng.normal(size=3)
        ax /= np.linalg.norm(ax)
        rq = np.concatenate([[np.cos(theta / 2) if theta != np.pi else 0.0], np.sin(theta / 2) * ax])
        absq[v] = _qmul(rq[None], absq[v - 1:v])[0]
        special[v] = rq
    q = _qvecs(rng, absq, pairs, noise=0.003)
    exact = np.zeros(len(pairs), bool)
    for v, rq in special.items():
        e = int(np.nonzero((pairs[:, 0] == v - 1) & (pairs[:, 1] == v))[0][0])
        q[e] = rq
        exact[e] = True
    return pairs.astype(np.uint32), q, exact


@pytest.mark.gpu
def test_relative_rotations_of_pi(dsm):
    p, q, exact = _pi_graph(95)
    ang = np.linalg.norm(ref.quaternion_to_angle_axis(q[exact]), axis=1)
    assert (q[exact, 0] == 0.0).sum() == 3 and np.abs(ang - np.pi).max() < 1.5e-9
    dev = dsm.rotation_averaging(p, q)
    _compare(dev, _expect(p, q))
    # q -> -q: where w != 0 the same bytes, where w = +-0 the angle-axis flips sign but is the same rotation
    qn = -q
    devn = dsm.rotation_averaging(p, qn)
    _compare(devn, _expect(p, qn))
    w0 = q[:, 0] == 0.0
    aa, aan = ref.quaternion_to_angle_axis(q[w0]), ref.quaternion_to_angle_axis(qn[w0])
    assert np.array_equal(aa, -aan) and ref.angle_between(aa, aan).max() < 1e-12
    assert np.array_equal(dev["edge_state"], devn["edge_state"])


@pytest.mark.gpu
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_orientations_near_pi(dsm, axis):
    """R_v R_0^T within 1e-7 of pi about one axis: the output reaches the largest-diagonal branch of RotationMatrixToQuaternion"""
    n = 30
    pairs = _edges_random(np.random.default_rng(100 + axis), n, 5)
    rng = np.random.default_rng(110 + axis)
    absq = _rand_q(rng, n)
    theta = np.pi - 5e-8
    targets = (7, 13, 21)
    for k, v in enumerate(targets):
        ax = np.zeros(3)
        ax[axis] = 1.0
        ax += 1e-3 * k * rng.normal(size=3)  # three images near the same axis
        ax /= np.linalg.norm(ax)
        rq = np.concatenate([[np.cos(theta / 2)], np.sin(theta / 2) * ax])
        absq[v] = _qmul(rq[None], absq[:1])[0]
    p = pairs.astype(np.uint32)
    q = _qvecs(rng, absq, pairs)
    dev = dsm.rotation_averaging(p, q)
    _compare(dev, _expect(p, q))
    o = dev["orientations"][list(targets)]
    assert (np.linalg.norm(o, axis=1) > np.pi - 1e-7).all()
    R = ref.angle_axis_to_rotation(o)
    tr = R[:, 0, 0] + R[:, 1, 1] + R[:, 2, 2]
    assert (tr < 0).all() and (np.argmax(R[:, [0, 1, 2], [0, 1, 2]], axis=1) == axis).all()


@pytest.mark.gpu
@pytest.mark.parametrize("scale", [1e-3, 1e3])
def test_unnormalised_qvecs(dsm, scale):
    p, q, _, _ = _graph(121, 60, _edges_random(np.random.default_rng(121), 60, 6), noise=0.004, n_corrupt=4)
    qs = q * scale
    assert np.allclose(np.linalg.norm(qs, axis=1), scale)
    dev = dsm.rotation_averaging(p, qs)
    _compare(dev, _expect(p, qs))
    unit = dsm.rotation_averaging(p, q)
    assert np.array_equal(dev["edge_state"], unit["edge_state"])
    assert ref.angle_between(dev["orientations"], unit["orientations"]).max() < 1e-8


@pytest.mark.gpu
def test_identity_relative_rotations_give_exact_zeros(dsm):
    pairs = _edges_random(np.random.default_rng(131), 50, 6)
    p = pairs.astype(np.uint32)
    q = np.tile([1.0, 0.0, 0.0, 0.0], (len(p), 1))
    dev = dsm.rotation_averaging(p, q)
    _compare(dev, _expect(p, q))
    r = dev["report"]
    assert (dev["orientations"] == 0.0).all() and (dev["relative_rotations"] == 0.0).all()
    assert np.isfinite(dev["orientations"]).all() and (dev["edge_state"] == 3).all()
    assert r.num_l1_iterations == 1 and r.admm_iterations[0] == 1 and r.num_irls_iterations == 1
    assert r.last_l1_step == 0.0 and r.last_irls_step == 0.0 and r.total_cg_iterations == 0


# ---------------------------------------------------------------- GPU: shapes and ids
def _hub_graph(seed, n_leaf=1100):
    """image 0 joined to every other image, the others joined as a chain plus a few random edges"""
    rng = np.random.default_rng(seed)
    n = n_leaf + 1
    pairs = np.vstack([np.stack([np.zeros(n_leaf, np.int64), np.arange(1, n)], 1), np.stack([np.arange(1, n - 1), np.arange(2, n)], 1),
                       _edges_random(rng, n, 1)])
    pairs = np.unique(np.sort(pairs, axis=1), axis=0)
    return pairs, n


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["constant", "largest_id"])
def test_hub_of_degree_over_1000(dsm, where):
    pairs, n = _hub_graph(141)
    ids = np.arange(n, dtype=np.int64) + 10 if where == "constant" else np.arange(n, dtype=np.int64)[::-1] + 10
    p, q, _, _ = _graph(142, n, pairs, noise=0.004, n_corrupt=20, ids=ids)
    dev, _ = _check(dsm, p, q, partition=_whole(p))
    hub = p.min() if where == "constant" else p.max()
    deg = int((p == hub).sum())
    assert deg >= 1000 and dev["report"].num_images == n
    assert dev["image_ids"][0 if where == "constant" else -1] == hub


@pytest.mark.gpu
def test_constant_image_of_degree_one(dsm):
    pairs = _edges_random(np.random.default_rng(151), 60, 6) + 1
    pairs = np.vstack([pairs, [[0, 17]]])
    p, q, _, _ = _graph(152, 61, pairs, noise=0.004, n_corrupt=3)
    dev, _ = _check(dsm, p, q)
    assert dev["image_ids"][0] == 0 and int((p == 0).sum()) == 1 and dev["report"].num_images == 61


@pytest.mark.gpu
def test_ids_zero_and_uint32_max(dsm):
    n = 50
    ids = np.concatenate([[0, 0xFFFFFFFF], np.random.default_rng(161).choice(0xFFFFFFF0, n - 2, replace=False) + 1]).astype(np.int64)
    p, q, _, _ = _graph(162, n, _edges_random(np.random.default_rng(163), n, 6), noise=0.004, n_corrupt=3, ids=ids)
    dev, _ = _check(dsm, p, q)
    assert dev["image_ids"][0] == 0 and dev["image_ids"][-1] == 0xFFFFFFFF and dev["report"].num_images == n


@pytest.mark.gpu
def test_too_many_pairs_refused_before_reading(dsm):
    from dagsfm_amd import capi
    p = np.array([(1, 2)], np.uint32)
    q = np.array([[1.0, 0, 0, 0]])
    ids, fin, state = np.zeros(2, np.uint32), np.zeros(2, np.uint8), np.zeros(1, np.uint8)
    orient, rel = np.zeros((2, 3)), np.zeros((1, 3))
    nimg = ctypes.c_uint32(7)
    L = dsm._L
    rc = L.dsm_view_graph_rotation_averaging(dsm._h, 2 ** 30, p.ctypes.data, q.ctypes.data, None, None, ids.ctypes.data, orient.ctypes.data,
                                             fin.ctypes.data, ctypes.addressof(nimg), state.ctypes.data, rel.ctypes.data, None)
    assert rc == 1 and "too many pairs" in L.dsm_last_error(dsm._h).decode()
    # the context still works
    out = dsm.rotation_averaging(p, q)
    assert out["report"].num_images == 2 and capi.DSM_ERR_NOT_CONVERGED == 6


@pytest.mark.gpu
def test_large_small_large_on_one_context():
    from dagsfm_amd import capi
    n = 2000
    big = _graph(51, n, _edges_random(np.random.default_rng(51), n, 40), noise=0.003, n_corrupt=800)[:2]
    small = _graph(12, 5, _edges_random(np.random.default_rng(12), 5, 4), noise=0.005)[:2]
    ctx = capi.Context(0)
    seq = [ctx.rotation_averaging(*g) for g in (big, small, big)]
    fresh_big = capi.Context(0).rotation_averaging(*big)
    fresh_small = capi.Context(0).rotation_averaging(*small)
    _same_bytes(seq[0], fresh_big)
    _same_bytes(seq[1], fresh_small)
    _same_bytes(seq[2], fresh_big)
