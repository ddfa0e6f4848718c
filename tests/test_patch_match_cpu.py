"""CPU-only: the normative restatement of PatchMatch (tests/patch_match_ref.py) held to the geometry and to
published values, not to itself; the host build of exact_exp.h against the host libm; the binding's file format and
consistency graph; the options' defaults and ranges."""
import ctypes
import math
import os

import numpy as np
import pytest

from tests import patch_match_ref as ref
from tests import patch_match_scenes as scenes

f32 = np.float32
U = 2.0 ** -24  # the unit roundoff of float32


def gamma(n):
    return n * U / (1.0 - n * U)


@pytest.fixture(scope="module")
def slanted():
    return scenes.make_scene("slanted", 48, 40, 4, seed=1)


def _pose_parts(pose):
    p = pose.astype(np.float64)
    K = np.array([[p[0], 0, p[1]], [0, p[2], p[3]], [0, 0, 1]])
    return K, p[4:13].reshape(3, 3), p[13:16]


def test_compose_homography_is_the_plane_induced_homography(slanted):
    """H of ComposeHomography against K (R + T n^T / dist) K_ref^-1 in float64, dist = depth * n . ray: the plane through the
    pixel's point X satisfies n . X = dist, so R X + T = (R + T n^T / dist) X on it (the reference's comment writes the other
    sign of n).  Both sides start from the same float32 tables, so the difference is the rounding of the float32 evaluation.

    Bound (Higham, Accuracy and Stability, 3.1 / 3.4): a float32 expression of + - * / whose longest operand-to-result
    path has n roundings differs from its exact value by at most gamma_n * (sum of the absolute values of its monomials),
    gamma_n = n u / (1 - n u), u = 2^-24.  The monomials of H are those of |K| |R| |K_ref^-1| and of |K| |T| |n|^T |K_ref^-1| /
    |dist|.  dist itself is a sum with cancellation: its relative error is at most gamma * distabs / |dist| (distabs the
    sum of the absolute values of its terms), which the terms holding 1 / dist inherit, hence the factor
    (1 + distabs / |dist|) on them.  The longest path -- ray (2), dist (5), 1 / dist (1), N (1), N T (1), + R (1), K (1),
    + (1), inv_K (1), the sums of H[2] (3) -- has 17 roundings; n = 24 leaves room for the second-order terms."""
    images, truth = slanted
    K4, iK4, poses = ref.init_transforms(images, 0, [1, 2, 3])
    rng = np.random.RandomState(3)
    n_paths = 24
    worst = 0.0
    for _ in range(200):
        s = rng.randint(3)
        row, col = rng.randint(40), rng.randint(48)
        depth = f32(rng.uniform(2.0, 8.0))
        nrm = rng.normal(size=3)
        nrm[2] = -abs(nrm[2]) - 0.5
        nrm = (nrm / np.linalg.norm(nrm)).astype(f32)
        iK = iK4[0]
        H32 = np.array(ref.compose_homography(poses[0][s], iK, f32(row), f32(col), depth, [nrm[0], nrm[1], nrm[2]]), dtype=np.float64)
        K, R, T = _pose_parts(poses[0][s])
        iKm = np.array([[iK[0], 0, iK[1]], [0, iK[2], iK[3]], [0, 0, 1]], dtype=np.float64)
        n64 = nrm.astype(np.float64)
        ray = np.array([float(iK[0]) * col + float(iK[1]), float(iK[2]) * row + float(iK[3]), 1.0])
        dist = float(depth) * (n64 @ ray)
        distabs = float(depth) * (np.abs(n64) @ np.array([abs(float(iK[0])) * col + abs(float(iK[1])), abs(float(iK[2])) * row + abs(float(iK[3])), 1.0]))
        H64 = K @ (R + np.outer(T, n64) / dist) @ iKm
        A0 = np.abs(K) @ np.abs(R) @ np.abs(iKm)
        A1 = np.abs(K) @ (np.outer(np.abs(T), np.abs(n64)) / abs(dist)) @ np.abs(iKm)
        bound = gamma(n_paths) * (A0 + (1.0 + distabs / abs(dist)) * A1)
        err = np.abs(H32.reshape(3, 3) - H64)
        assert (err <= bound).all(), (err / bound).max()
        worst = max(worst, float((err / bound).max()))
    assert worst > 0.0  # the float32 evaluation is not the float64 one: the comparison is not vacuous


def test_propagate_depth_returns_the_planes_depth_at_the_next_row():
    """PropagateDepth works in the (y, z) section of the pixel's column and ignores n[0], so it is exact for planes whose
    normal lies in that section: the ray of `row2` meets the plane n1 y + n2 z = c at depth c / (n1 y2 + n2), y2 the ray's y.
    nom = y1 x2 - x1 y2 and denom = (x2 - x1) + x4 (y1 - y2) both cancel (depth1 * x1 appears twice in nom, x1 twice in
    denom); with nomabs / denabs the sums of the absolute values of their terms, the relative error of nom / denom is at most
    gamma_n (nomabs / |nom| + denabs / |denom|): the same forward bound as above with n = 10 (x1: 3, x2 / y2: 1, the
    products and differences of nom: 2, denom: 4, the quotient: 1, rounded up)."""
    iK = np.array([1 / 52.0, -23.8 / 52.0, 1 / 52.0, -19.3 / 52.0], dtype=f32)
    rng = np.random.RandomState(5)
    for _ in range(300):
        row1 = rng.randint(0, 40)
        row2 = row1 + 1
        depth1 = f32(rng.uniform(2.0, 8.0))
        ang = rng.uniform(-1.2, 1.2)
        n = np.array([0.0, math.sin(ang), -math.cos(ang)], dtype=f32)
        got = float(ref.propagate_depth(iK, np.array([depth1]), [n[:1], n[1:2], n[2:3]], row1, row2)[0])
        i2, i3, d1, n1, n2 = float(iK[2]), float(iK[3]), float(depth1), float(n[1]), float(n[2])
        y1r, y2r = i2 * row1 + i3, i2 * row2 + i3
        c = n1 * (d1 * y1r) + n2 * d1
        want = c / (n1 * y2r + n2)
        x1 = d1 * y1r
        nom, nomabs = d1 * (x1 + n2) - x1 * (d1 - n1), 2 * abs(d1 * x1) + abs(d1 * n2) + abs(x1 * n1)
        den, denabs = n2 + y2r * n1, 2 * abs(x1) + abs(n2) + abs(y2r) * (2 * d1 + abs(n1))
        if abs(den) < 1e-3:
            continue
        bound = gamma(10) * (nomabs / abs(nom) + denabs / abs(den)) * abs(want)
        assert abs(got - want) <= bound, (got, want, bound)


def test_geom_consistency_cost_vanishes_for_true_depth_maps_and_is_maximal_off_the_image(slanted):
    """With the ground-truth depth maps the forward-backward reprojection error is the error of sampling the source depth at
    the NEAREST pixel: at most half a pixel times the depth slope of the plane, 0.03 pixels back in the reference image
    for this scene (focal 53, baseline 0.6, depth 4, slope 0.026 per pixel); asserted below 0.1.  Where the projection leaves
    the source image the cost is max_cost exactly."""
    images, truth = slanted
    fed = [dict(im, depth_map=t["depth"].astype(f32)) for im, t in zip(images, truth)]
    c = ref.constants(ref.Options())
    K, iK, poses = ref.init_transforms(fed, 0, [1, 2, 3])
    sources = ref.Sources(fed, [1, 2, 3], True)
    rows, cols = np.meshgrid(np.arange(40, dtype=f32), np.arange(48, dtype=f32), indexing="ij")
    depth = truth[0]["depth"].astype(f32)
    inside_seen = 0
    with np.errstate(all="ignore"):
        for s in range(3):
            cost = ref.geom_consistency_cost(c, sources, poses[0][s], K[0], iK[0], s, rows, cols, depth)
            P = poses[0][s][19:31].astype(np.float64).reshape(3, 4)
            X = np.stack([depth * (iK[0][0] * cols + iK[0][1]), depth * (iK[0][2] * rows + iK[0][3]), depth, np.ones_like(depth)]).astype(np.float64)
            x = np.einsum("ij,jhw->ihw", P, X)
            u, v = x[0] / x[2], x[1] / x[2]
            inside = (u > 1) & (u < 46) & (v > 1) & (v < 38)
            outside = (u < -1.5) | (u > 48.5) | (v < -1.5) | (v > 40.5)
            assert (cost[inside] < 0.1).all(), cost[inside].max()
            assert (cost[outside] == c["geom_max_cost"]).all()
            inside_seen += int(inside.sum())
        far = ref.geom_consistency_cost(c, sources, poses[0][0], K[0], iK[0], 0, rows, cols, depth * f32(40.0))
    assert inside_seen > 3000
    assert (far <= c["geom_max_cost"]).all()


def test_rotated_tables_map_a_pixel_and_its_rotated_twin_to_the_same_ray(slanted):
    """InitTransforms: in rotation r the pixel (x, y) of the original frame is the pixel of the r times counter-clockwise
    rotated image, its ray is R_z90^r times the original ray, and the rotated pose takes it to the same point of every
    source camera."""
    images, _ = slanted
    K, iK, poses = ref.init_transforms(images, 0, [1, 2, 3])
    h, w = 40, 48
    Rz = np.array([[0.0, 1.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    for x, y in [(0, 0), (47, 0), (13, 29), (47, 39), (20, 5)]:
        ray0 = np.array([iK[0][0] * x + iK[0][1], iK[0][2] * y + iK[0][3], 1.0], dtype=np.float64)
        xr, yr, wr = x, y, w
        hr = h
        rot = np.eye(3)
        for r in range(1, 4):
            xr, yr = yr, wr - 1 - xr  # CudaRotate: out[(w - 1 - x) * h + y] = in[y * w + x]
            wr, hr = hr, wr
            rot = Rz @ rot
            ray = np.array([iK[r][0] * xr + iK[r][1], iK[r][2] * yr + iK[r][3], 1.0], dtype=np.float64)
            assert np.allclose(ray, rot @ ray0, rtol=0, atol=1e-5), (r, ray, rot @ ray0)
            for s in range(3):
                _, R0, T0 = _pose_parts(poses[0][s])
                _, Rr, Tr = _pose_parts(poses[r][s])
                X = 4.2 * ray0
                assert np.allclose(Rr @ (rot @ X) + Tr, R0 @ X + T0, rtol=0, atol=2e-5)
                assert np.allclose(-Rr.T @ Tr, rot @ (-R0.T @ T0), rtol=0, atol=2e-5)  # the projection centre turns with the frame
                assert np.array_equal(poses[r][s][:4], poses[0][s][:4])


def test_four_rotations_of_every_map_are_the_identity():
    rng = np.random.RandomState(2)
    for shape in [(23, 37), (3, 37, 23), (5, 9, 65), (1, 1), (0, 5, 7)]:
        a = rng.normal(size=shape).astype(f32)
        b = a
        for _ in range(4):
            b = ref.rotate_map(b)
        assert b.shape == a.shape and np.array_equal(b.view(np.uint32), a.view(np.uint32))
    one = ref.rotate_map(np.arange(6, dtype=f32).reshape(2, 3))
    assert one.tolist() == [[2.0, 5.0], [1.0, 4.0], [0.0, 3.0]]  # counter-clockwise
    n = rng.normal(size=(3, 9, 14)).astype(f32)
    m = n
    for _ in range(4):
        m = ref.rotate_normal_map(m)
    assert np.array_equal(m.view(np.uint32), n.view(np.uint32))
    q = ref.rotate_normal_map(n)
    assert np.array_equal(q[0], np.rot90(n[1])) and np.array_equal(q[1], np.rot90(-n[0])) and np.array_equal(q[2], np.rot90(n[2]))


def test_philox_known_answers():
    """The Philox4x32-10 vectors of Random123's kat_vectors (Salmon, Moraes, Dror, Shaw, SC'11)."""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for counter, key, want in kat:
        assert tuple(int(x) for x in ref.philox4x32_10(counter, key)) == want
    got = ref.philox4x32_10((np.array([0, 0x243f6a88], dtype=np.uint32), np.array([0, 0x85a308d3], dtype=np.uint32),
                             np.array([0, 0x13198a2e], dtype=np.uint32), np.array([0, 0x03707344], dtype=np.uint32)), (0, 0))
    assert int(got[0][0]) == 0x6627e8d5  # vectorised over the counter
    u = ref.uniform(7, 3, np.arange(1000, dtype=np.uint32), 5, 1, 0)
    assert u.dtype == f32 and (u > 0).all() and (u <= 1).all() and 0.4 < u.mean() < 0.6


def _exp_lib():
    from dagsfm_amd import capi
    path = os.path.join(os.path.dirname(capi.LIB_PATH), "libdsm_exact_exp.so")
    assert os.path.exists(path), "build first: " + path
    L = ctypes.CDLL(path)
    L.dsm_host_exp_f32.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64]
    L.dsm_host_exp_f32.restype = None
    return L


def test_exact_exp_is_the_host_libm_rounded_to_float():
    """exact_exp.h, compiled for the host, against math.exp rounded to float on 1 050 000 float arguments of [-60, 0] (and the
    ends of its range): equality, not a tolerance."""
    L = _exp_lib()
    rng = np.random.RandomState(17)
    x = np.concatenate([rng.uniform(-60.0, 0.0, size=700000), -np.exp(rng.uniform(-20.0, math.log(60.0), size=250000)),
                        np.linspace(-60.0, 0.0, 100000)]).astype(f32)
    assert len(x) >= 10 ** 6 and x.min() >= -60.0 and x.max() <= 0.0
    y = np.empty_like(x)
    L.dsm_host_exp_f32(x.ctypes.data, y.ctypes.data, len(x))
    want = np.array([math.exp(v) for v in x.astype(np.float64).tolist()], dtype=np.float64).astype(f32)
    bad = np.flatnonzero(y.view(np.uint32) != want.view(np.uint32))
    assert len(bad) == 0, (len(bad), x[bad[:5]], y[bad[:5]], want[bad[:5]])
    edge = np.array([-0.0, 0.0, -103.0, -104.0, -200.0, -745.0, -1e30, -np.inf, np.nan, 1.0, 88.0, 89.0, 1e30], dtype=f32)
    out = np.empty_like(edge)
    L.dsm_host_exp_f32(edge.ctypes.data, out.ctypes.data, len(edge))
    with np.errstate(all="ignore"):
        assert np.array_equal(out, ref.exp32(edge), equal_nan=True)


def test_option_defaults_and_ranges_are_the_references():
    """patch_match.h:59-139 (defaults; the float literals assigned to doubles keep their float value) and :141-168 (Check)."""
    from dagsfm_amd import capi
    want = dict(window_radius=5, window_step=1, num_samples=15, num_iterations=5, geom_consistency=1, filter=1, filter_min_num_consistent=2,
                seed=0, sigma_spatial=-1.0, sigma_color=float(f32(0.2)), ncc_sigma=float(f32(0.6)), min_triangulation_angle=1.0,
                incident_angle_sigma=float(f32(0.9)), geom_consistency_regularizer=float(f32(0.3)), geom_consistency_max_cost=3.0,
                filter_min_ncc=float(f32(0.1)), filter_min_triangulation_angle=3.0, filter_geom_consistency_max_cost=1.0)
    o = capi.default_patch_match_options()
    assert {name: getattr(o, name) for name, _ in o._fields_} == want
    r = ref.Options()
    assert {k: (int(v) if isinstance(v, bool) else v) for k, v in r.as_dict().items()} == want
    assert r.check() is None
    good = [dict(window_radius=1), dict(window_radius=32), dict(window_step=2), dict(min_triangulation_angle=0.0), dict(filter_min_ncc=-1.0),
            dict(filter_min_ncc=1.0), dict(filter_min_triangulation_angle=180.0), dict(filter_min_num_consistent=0),
            dict(geom_consistency_regularizer=0.0), dict(sigma_spatial=0.0)]
    for kw in good:
        assert ref.Options(**kw).check() is None, kw
    bad = [dict(window_radius=0), dict(window_radius=33), dict(window_step=0), dict(window_step=3), dict(sigma_color=0.0), dict(num_samples=0),
           dict(ncc_sigma=0.0), dict(min_triangulation_angle=-0.1), dict(min_triangulation_angle=180.0), dict(incident_angle_sigma=0.0),
           dict(num_iterations=0), dict(geom_consistency_regularizer=-1.0), dict(geom_consistency_max_cost=-1.0), dict(filter_min_ncc=-1.1),
           dict(filter_min_ncc=1.1), dict(filter_min_triangulation_angle=-1.0), dict(filter_min_triangulation_angle=180.5),
           dict(filter_min_num_consistent=-1), dict(filter_geom_consistency_max_cost=-0.5)]
    for kw in bad:
        assert ref.Options(**kw).check() is not None, kw
    c = ref.constants(ref.Options(window_radius=7))
    assert c["w_spatial"][7 * 15 + 7] == 1.0 and c["w_spatial"][0] == f32(math.exp(-98.0 / 98.0))  # sigma_spatial <= 0: window_radius


def test_requantisation_of_the_reference_image_changes_no_byte():
    """gpu_mat_ref_image.cu:80 stores uint8(255.0f * (b / 255.0f)): under IEEE float that is b for all 256 bytes."""
    b = np.arange(256, dtype=np.uint8)
    assert np.array_equal(ref.requantise(b), b)


def test_mvs_array_file_round_trip(tmp_path):
    """mvs/mat.h:157-191: `W&H&C&` in text, then the floats little-endian, slice after slice."""
    from dagsfm_amd import capi
    depth = np.arange(6, dtype=f32).reshape(2, 3) + f32(0.5)
    path = str(tmp_path / "depth.bin")
    capi.write_mvs_array(path, depth)
    blob = open(path, "rb").read()
    assert blob[:6] == b"3&2&1&" and len(blob) == 6 + 24
    assert blob[6:10] == np.array([0.5], dtype="<f4").tobytes()
    back = capi.read_mvs_array(path)
    assert back.shape == (1, 2, 3) and np.array_equal(back[0].view(np.uint32), depth.view(np.uint32))
    normal = np.random.RandomState(1).normal(size=(3, 5, 12)).astype(f32)
    normal[0, 0, 0] = np.nan
    path = str(tmp_path / "normal.bin")
    capi.write_mvs_array(path, normal)
    assert open(path, "rb").read()[:7] == b"12&5&3&"
    assert np.array_equal(capi.read_mvs_array(path).view(np.uint32), normal.view(np.uint32))
    open(path, "ab").write(b"\0")
    with pytest.raises(capi.DsmError):
        capi.read_mvs_array(path)


def test_consistency_graph_of_a_hand_made_mask():
    """GetConsistentImageIdxs :1217-1241: col, row, count, ids... per pixel with a consistent image, row-major."""
    from dagsfm_amd import capi
    mask = np.zeros((3, 2, 4), np.uint8)
    mask[0, 0, 1] = 1
    mask[2, 0, 1] = 1
    mask[1, 1, 3] = 7  # any non-zero byte counts
    mask[0, 1, 0] = mask[1, 1, 0] = mask[2, 1, 0] = 1
    srcs = [11, 5, 9]
    want = [1, 0, 2, 11, 9, 0, 1, 3, 11, 5, 9, 3, 1, 1, 5]
    got = capi.consistency_graph(mask, srcs)
    assert got.dtype == np.int32 and got.tolist() == want
    assert ref.consistency_graph(mask, srcs).tolist() == want
    assert capi.consistency_graph(np.zeros((3, 2, 4), np.uint8), srcs).tolist() == []
    assert capi.consistency_graph(np.zeros((0, 2, 4), np.uint8), []).tolist() == []


def test_restatement_recovers_the_slanted_plane(slanted):
    """Accuracy of the restatement on the slanted plane, 48 x 40, 3 source images, radius 3, 3 iterations, filter on,
    depth range [2, 8] around the true 3.5 .. 5.6: the median relative depth error of the pixels that survive the filter.
    Measured: 0.00185 (99.9 % of the pixels further than the radius from the border survive); asserted at twice that, a
    margin for later changes of the seed or of the contract.  Condition: at least half of those pixels survive."""
    images, truth = slanted
    o = ref.Options(window_radius=3, num_iterations=3, geom_consistency=False, filter=True)
    r = ref.patch_match(images, 0, [1, 2, 3], 2.0, 8.0, o)
    depth, gt = r["depth"], truth[0]["depth"]
    keep = depth > 0
    inner = np.zeros_like(keep)
    inner[3:-3, 3:-3] = True
    survive = (keep & inner).sum() / inner.sum()
    median = float(np.median((np.abs(depth - gt) / gt)[keep]))
    print("survivors %.4f, median relative depth error %.6f" % (survive, median))
    assert survive >= 0.5
    assert median <= 2 * 0.00185
    nrm = r["normal"][:, keep]
    cosang = (nrm * truth[0]["normal"][:, keep]).sum(axis=0)
    assert np.median(cosang) > 0.99  # the normals agree with the plane's
    assert r["mask"].shape == (3, 40, 48) and (r["mask"].sum(axis=0)[keep] >= 2).all() and not r["mask"][:, ~keep].any()
