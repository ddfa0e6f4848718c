"""CPU-only: the restatement of stereo fusion (tests/stereo_fusion_ref.py) held to the reference's text and to
geometry -- not to itself -- and the host build of the kernels' header (libdsm_stereo_fusion_host.so) held to the restatement
bit for bit."""
import math

import numpy as np
import pytest

from dagsfm_amd import capi
from tests import stereo_fusion_cases as cases
from tests import stereo_fusion_ref as ref


def test_defaults_and_ranges_are_the_reference_s():
    o = capi.default_stereo_fusion_options()
    f32 = np.float32
    assert (o.min_num_pixels, o.max_num_pixels, o.max_traversal_depth, o.lane_capacity) == (5, 10000, 100, 0)
    assert (o.max_reproj_error, o.max_depth_error, o.max_normal_error) == (float(f32(2.0)), float(f32(0.01)), float(f32(10.0)))
    assert ref.DEFAULTS == {k: getattr(o, k) for k in ref.DEFAULTS}
    ok = dict(ref.DEFAULTS)
    assert ref.check_options(ok)
    for bad in ({"min_num_pixels": 0}, {"min_num_pixels": 6, "max_num_pixels": 5}, {"max_traversal_depth": 0}, {"max_reproj_error": -1.0},
                {"max_depth_error": -1e-9}, {"max_normal_error": -1.0}, {"max_depth_error": float("nan")}):
        assert not ref.check_options(dict(ok, **bad)), bad
    for fine in ({"min_num_pixels": 1}, {"min_num_pixels": 7, "max_num_pixels": 7}, {"max_traversal_depth": 1}, {"max_reproj_error": 0.0}):
        assert ref.check_options(dict(ok, **fine)), fine


@pytest.mark.parametrize("n", [1, 2, 3, 4, 7, 10, 31, 64])
def test_median_is_numpy_s(n):
    rng = np.random.RandomState(n)
    floats = rng.standard_normal(n).astype(np.float32)
    got = ref.median(list(floats))
    assert isinstance(got, np.float32)
    # the mean of the two middle floats in float: numpy's median of float32 does the same sum in float
    assert got == np.float32(np.median(floats))
    ints = rng.randint(0, 256, size=n).astype(np.uint8)
    assert ref.median(list(ints)) == np.float32(np.median(ints.astype(np.float32)))
    assert ref.median(list(np.full(n, 255, dtype=np.uint8))) == np.float32(255.0)  # the uint8 are cast before they are added


def test_find_next_image_order():
    #           0       1     2      3       4   5
    overlap = [[3, 1], [0], [4, 0], [1, 2], [], [0]]
    used = [True, True, True, True, True, False]
    # 0 -> its list: 3 -> its list: 1 -> (0 fused) the first unfused: 2 -> its list: 4 -> none left
    assert ref.image_order(overlap, used) == [0, 3, 1, 2, 4]
    used0 = [False, True, True, True, True, False]
    # the loop starts at image 0 although it is unused; its list still steers the order
    assert ref.image_order(overlap, used0) == [0, 3, 1, 2, 4]
    assert ref.image_order([[], [], []], [False, False, True]) == [0, 2]
    assert ref.image_order([[], []], [False, False]) == [0]
    assert ref.image_order([], []) == []


class _Recording(ref.Fusion):
    """The restatement, keeping every cluster next to its point."""

    def __init__(self, *a):
        super().__init__(*a)
        self.clusters = []

    def finish(self, acc, vals):
        out = super().finish(acc, vals)
        self.clusters.append((acc, vals, out))
        return out


GAMMA_13 = 13 * 2.0 ** -24 / (1 - 13 * 2.0 ** -24)


def _plane_terms(images, image, row, col):
    """sum |terms| of n . X + d for the pixel's X = inv_P (col depth, row depth, depth, 1), X's own row sums expanded."""
    n, d = cases.SLANTED_PLANE
    inv_P = images[image]["inv_P"].astype(np.float64).reshape(3, 4)
    depth = float(images[image]["depth"][row, col])
    v = np.abs([col * depth, row * depth, depth, 1.0])
    return (np.abs(n)[:, None] * np.abs(inv_P) * v[None, :]).sum() + d


def test_accepted_pixels_lie_on_the_plane_and_the_point_is_their_median():
    """Every pixel a cluster accepts back-projects onto the slanted plane within gamma_13 * sum |terms|: per term the rounding
    of K, R, T to float (3), of the inverse and of the depth (2), of col * depth (1), of the product (1) and the three sums of
    the row, the dot product with the plane's normal on top (3).  The fused coordinates are medians of these, so each lies
    within its cluster's range, and the normal is the plane's."""
    images, overlap, options = cases.case("slanted")
    n, d = cases.SLANTED_PLANE
    f = _Recording(images, overlap, options)
    res = f.run()
    assert res["points"].tobytes() == cases.expected("slanted")["points"].tobytes() and len(res["points"]) >= 100
    worst = 0.0
    for acc, vals, out in f.clusters:
        xyz = np.array([[float(c) for c in v[0]] for v in vals])
        for (image, row, col), x in zip(acc, xyz):
            ratio = abs(n @ x + d) / (GAMMA_13 * _plane_terms(images, image, row, col))
            worst = max(worst, ratio)
            assert ratio <= 1.0, (image, row, col, ratio)
        if out is not None:
            p = out[0].astype(np.float64)
            assert (xyz.min(axis=0) <= p[:3]).all() and (p[:3] <= xyz.max(axis=0)).all()
            assert abs(np.linalg.norm(p[3:]) - 1.0) < 1e-6
            assert math.degrees(math.acos(min(1.0, abs(p[3:] @ n)))) < 10.0
    print("worst plane residual of an accepted pixel / bound: %.3f" % worst)
    assert max(len(v) for v in res["visibility"]) >= 3
    assert all(v == sorted(set(v)) and len(v) >= 1 for v in res["visibility"])


GAMMA_14 = 14 * 2.0 ** -24 / (1 - 14 * 2.0 ** -24)


def test_fused_points_lie_on_the_plane():
    """Every fused point of the slanted plane's truth maps satisfies the plane equation within gamma_n * sum |terms|, and every
    normal is within 10 degrees of the plane's.
    The bound is a rounding bound, so it can hold only where a fused point is an affine combination of back-projected pixels:
    Fuse() takes the medians of x, of y and of z separately (fusion.cc:454-456), and with three or more pixels the three may
    come from different pixels of the cluster, which lie up to two pixels apart on the plane (at the defaults: residual max
    1.7e-2, median 2.0e-3 over the 270 points, against a bound of 1.1e-5 -- the reference's arithmetic, not an error).  With
    max_num_pixels = 2 every cluster has one pixel -- the point is its back-projection, within gamma_13 * sum |terms| as the
    test above derives -- or two, of different images or of the same: Median then gives (a + b) / 2 in each coordinate, the
    midpoint of two points of the plane, one more rounding: gamma_14 * the larger sum |terms| of the two.  min_num_pixels = 1
    keeps every cluster, so every pixel with a depth is in exactly one point.  At the defaults the normals are checked too."""
    images, overlap, options = cases.case("slanted_pairs")
    n, d = cases.SLANTED_PLANE
    f = _Recording(images, overlap, options)
    res = f.run()
    assert res["points"].tobytes() == cases.expected("slanted_pairs")["points"].tobytes()
    assert len(res["points"]) >= 100 and len(res["points"]) == sum(out is not None for _, _, out in f.clusters) == len(f.clusters)
    pairs = two_images = 0
    worst = 0.0
    for acc, vals, out in f.clusters:
        assert 1 <= len(acc) <= 2
        pairs += len(acc) == 2
        two_images += len(out[2]) == 2
        terms = max(_plane_terms(images, image, row, col) for image, row, col in acc)
        p = out[0].astype(np.float64)
        ratio = abs(n @ p[:3] + d) / (GAMMA_14 * terms)
        worst = max(worst, ratio)
        assert ratio <= 1.0, (acc, ratio)
        assert math.degrees(math.acos(min(1.0, abs(p[3:] / np.linalg.norm(p[3:]) @ n)))) < 10.0
    print("worst plane residual of a fused point / bound: %.3f; %d of %d points from two pixels, %d from two images" % (worst, pairs, len(f.clusters), two_images))
    assert pairs >= 100 and two_images >= 100  # the midpoint case, across images, is what most points show
    assert sum(len(acc) for acc, _, _ in f.clusters) == sum(int((im["depth"] > 0).sum()) for im in images)
    for q in cases.expected("slanted")["points"].astype(np.float64):
        assert math.degrees(math.acos(min(1.0, abs(q[3:] / np.linalg.norm(q[3:]) @ n)))) < 10.0


def test_mask_persists_below_min_num_pixels():
    images, overlap, _ = cases.case("slanted")
    low = ref.fuse(images, overlap, {"min_num_pixels": 2})
    high = ref.fuse(images, overlap, {"min_num_pixels": 9999, "max_num_pixels": 10000})
    assert len(low["points"]) > 0 and len(high["points"]) == 0
    # the traversals do not depend on min_num_pixels, so the clusters without a point consumed the same pixels
    for a, b, im in zip(low["masks"], high["masks"], images):
        assert (a == b).all() and (b == (im["depth"] > 0)).all()
    assert low["stats"]["traversals"] == high["stats"]["traversals"]
    got = capi.fusion_host(images, overlap, min_num_pixels=9999)
    assert len(got[0]) == 0 and (got[4].astype(bool) == np.concatenate([m.reshape(-1) for m in high["masks"]])).all()


def test_bitmap_of_another_size_and_colour_outside_it():
    images, overlap, options = cases.case("slanted_bitmap_2x")
    same, _, _ = cases.case("slanted")
    assert images[1]["rgb"].shape[:2] == (46, 74) and images[1]["depth"].shape == (23, 37)
    a, b = cases.expected("slanted_bitmap_2x"), cases.expected("slanted")
    # the doubled bitmap repeats every pixel, and round(col / 0.5) = 2 col reads the same colour: the same cloud
    assert a["points"].tobytes() == b["points"].tobytes() and a["colours"].tobytes() == b["colours"].tobytes()
    f = ref.Fusion(images, overlap)
    assert f.colour(1, 22, 36) == tuple(int(c) for c in images[1]["rgb"][44, 72])
    # a bitmap smaller than its scale promises: the pixels beyond it are black (BitmapColor() after a failed GetPixel)
    cut = [dict(im) for im in same]
    cut[0]["rgb"] = np.ascontiguousarray(same[0]["rgb"][:12, :20])
    f = ref.Fusion(cut, overlap)
    assert f.colour(0, 11, 19) == tuple(int(c) for c in same[0]["rgb"][11, 19]) and f.colour(0, 12, 19) == (0, 0, 0) and f.colour(0, 0, 20) == (0, 0, 0)
    want = f.run()
    got = capi.fusion_host(cut, overlap)
    assert cases.same_result(got, want)
    assert want["colours"].tobytes() != b["colours"].tobytes()


@pytest.mark.parametrize("name", cases.TABLE)
def test_round_rule_equals_the_sequential_loop(name):
    images, overlap, options = cases.case(name)
    want = cases.expected(name)
    got = ref.fuse(images, overlap, options, rounds=True)
    assert got["points"].tobytes() == want["points"].tobytes() and got["colours"].tobytes() == want["colours"].tobytes()
    assert got["visibility"] == want["visibility"]
    assert all((a == b).all() for a, b in zip(got["masks"], want["masks"]))
    assert len(got["stats"]["rounds"]) == len(images) and got["stats"]["rounds"][0] > 1  # the schedule had something to order


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_host_build_equals_the_restatement(name):
    images, overlap, options = cases.case(name)
    want = cases.expected(name)
    got = capi.fusion_host(images, overlap, **options)
    assert cases.same_result(got, want)
    assert got[5] == want["stats"]["traversals"]
    assert (got[4].astype(bool) == np.concatenate([m.reshape(-1) for m in want["masks"]])).all()
    # the conditions under which a case shows anything
    assert len(want["points"]) >= 100
    if name in cases.DEFAULT_CASES:
        assert max(len(v) for v in want["visibility"]) >= 3
    if name == "step_max_pixels":
        assert want["stats"]["breaks"] >= 1
    if name == "slanted_depth_limit":
        assert want["stats"]["depth_hits"] >= 1


def test_host_build_unused_images_and_refusals():
    images, overlap, _ = cases.case("step_noise_holes")
    part = [dict(im) for im in images]
    part[0] = {"used": False}  # image 0 unused: the loop still starts there
    part[3]["used"] = False
    lists = [[1, 2], [0, 2, 3], [3, 1], [0], []]  # image 4 is named in no list and lists nobody
    want = ref.fuse([dict(im, used=False, depth=np.zeros((0, 0), np.float32)) if not im["used"] else im for im in part], lists,
                    {"min_num_pixels": 2})
    got = capi.fusion_host(part, lists, min_num_pixels=2)
    assert cases.same_result(got, want) and len(want["points"]) > 0
    assert {i for v in want["visibility"] for i in v} == {1, 2}  # a pixel of image 4 stays alone, below min_num_pixels
    assert want["masks"][4].sum() == (images[4]["depth"] > 0).sum()  # ... and is consumed all the same
    for bad in ({"min_num_pixels": 0}, {"max_traversal_depth": 0}, {"max_depth_error": float("nan")}, {"max_reproj_error": -1.0},
                {"min_num_pixels": 4, "max_num_pixels": 3}, {"lane_capacity": -1}):
        with pytest.raises(capi.DsmError) as e:
            capi.fusion_host(images, overlap, **bad)
        assert e.value.rc == 1, bad
    for lists_bad in ([[0]] + overlap[1:], [[5]] + overlap[1:]):
        with pytest.raises(capi.DsmError):
            capi.fusion_host(images, lists_bad)
    assert len(capi.fusion_host([], [])[0]) == 0
    assert len(capi.fusion_host([{"used": False}], [[]])[0]) == 0


def test_fusion_matrices_invert_each_other():
    rng = np.random.RandomState(3)
    K = np.array([700.0, 0, 320.5, 0, 710.0, 239.5, 0, 0, 1], dtype=np.float32)
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    R = (q * np.sign(np.linalg.det(q))).astype(np.float32)
    T = rng.standard_normal(3).astype(np.float32)
    P, inv_P, inv_R = capi.fusion_matrices(K, R, T, 0.5, 0.25)
    assert P.dtype == inv_P.dtype == inv_R.dtype == np.float32
    P4 = np.vstack([P.reshape(3, 4).astype(np.float64), [0, 0, 0, 1]])
    I4 = np.vstack([inv_P.reshape(3, 4).astype(np.float64), [0, 0, 0, 1]])
    assert np.abs(P4 @ I4 - np.eye(4)).max() < 1e-3
    Ks = K.reshape(3, 3).astype(np.float64) * np.array([[0.5], [0.25], [1.0]])
    assert np.allclose(P.reshape(3, 4), Ks @ np.hstack([R.astype(np.float64), T[:, None].astype(np.float64)]), rtol=1e-6, atol=1e-4)
    assert (inv_R.reshape(3, 3) == R.reshape(3, 3).T).all()


def test_overlapping_images_counts_shared_points():
    tracks = [[0, 1, 2], [0, 1], [1, 2], [0, 1, 3], [3, 2], [2, 2, 0]]
    # shared: 0-1: 3, 0-2: 1 + 2 (the repeated 2 counts twice, as ComputeSharedPoints counts it), 0-3: 1, 1-2: 2, 1-3: 1, 2-3: 1
    got = capi.overlapping_images(tracks, 5, 2)
    assert got == [[1, 2], [0, 2], [0, 1], [0, 1], []]
    assert capi.overlapping_images(tracks, 5, 10)[3] == [0, 1, 2]  # ties: the lower index first


def test_writers_round_trip(tmp_path):
    res = cases.expected("step_sizes")
    ply = str(tmp_path / "fused.ply")
    capi.write_fused_ply(ply, res["points"][:, :3], res["points"][:, 3:], res["colours"])
    blob = open(ply, "rb").read()
    n = len(res["points"])
    header = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
              "property float nx\nproperty float ny\nproperty float nz\nproperty uchar red\nproperty uchar green\nproperty uchar blue\n"
              "end_header\n" % n).encode()
    assert blob.startswith(header) and len(blob) == len(header) + 27 * n
    assert blob[len(header):len(header) + 24] == res["points"][0].astype("<f4").tobytes() and blob[len(header) + 24:len(header) + 27] == res["colours"][0].tobytes()
    p, nrm, c = capi.read_fused_ply(ply)
    assert p.tobytes() == res["points"][:, :3].tobytes() and nrm.tobytes() == np.ascontiguousarray(res["points"][:, 3:]).tobytes() and (c == res["colours"]).all()
    vis = str(tmp_path / "fused.ply.vis")
    capi.write_points_visibility(vis, res["visibility"])
    blob = open(vis, "rb").read()
    assert int(np.frombuffer(blob[:8], "<u8")[0]) == n and len(blob) == 8 + 4 * (n + sum(len(v) for v in res["visibility"]))
    assert int(np.frombuffer(blob[8:12], "<u4")[0]) == len(res["visibility"][0])
    assert capi.read_points_visibility(vis) == res["visibility"]
