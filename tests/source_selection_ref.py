"""The contract of dsm_select_source_images, in plain Python / numpy in the reference's evaluation order: the
queries of mvs::Model that turn a sparse model into PatchMatch's problems.

  GetMaxOverlappingImages      src/mvs/model.cc:119-169 (+ ReadProblems' candidate condition, src/mvs/patch_match.cc:349)
  ComputeDepthRanges           src/mvs/model.cc:176-216
  ComputeSharedPoints          src/mvs/model.cc:218-233
  ComputeTriangulationAngles   src/mvs/model.cc:235-274
  ComputeProjectionCenter      src/mvs/image.cc:125-130
  CalculateTriangulationAngle  src/base/triangulation.cc:122-145
  DegToRad, Percentile         src/util/math.h:194-200, 231-246

float arithmetic is numpy.float32 scalars (every operation rounds once, no contraction), double arithmetic is Python floats.
Where Eigen fixes no order a sum runs left to right.  acos is math.acos -- the host libm, which returns the correctly rounded
value for all but a vanishing fraction of arguments; the device's is csrc/exact_acos.h, the correctly rounded value itself, and
tests/test_source_selection_cpu.py shows that the two give the same float angle on every item of the fixtures.  (numpy.arccos is
not used: its SIMD loops are not libm and differ between hosts.)
Rulings: an item whose quotient left [-1, 1] has the angle NaN, which orders above every number and fails `>=`; equal counts go
to the lower image index.
"""
import math

import numpy as np

f32 = np.float32
DEG_TO_RAD = 0.0174532925199432954743716805978692718781530857086181640625
NAN = float("nan")


def projection_center(R, T):
    """C = -R^T T in float, widened to double: a list of 3 Python floats."""
    R = np.asarray(R, dtype=f32).reshape(9)
    T = np.asarray(T, dtype=f32).reshape(3)
    return [float(-((R[i] * T[0] + R[3 + i] * T[1]) + R[6 + i] * T[2])) for i in range(3)]


def depth(R, T, X):
    R = np.asarray(R, dtype=f32).reshape(9)
    T = np.asarray(T, dtype=f32).reshape(3)
    X = np.asarray(X, dtype=f32).reshape(3)
    return ((R[6] * X[0] + R[7] * X[1]) + R[8] * X[2]) + T[2]


def depth_index(size, factor):
    """image_depths[image_depths.size() * kPercentile]: the product is a FLOAT product (size_t -> float, times a float)."""
    return int(f32(size) * f32(factor))


def percentile_index(p, n):
    """Percentile's index: std::round(p / 100 * (n - 1)) -- half away from zero -- clamped to [0, n - 1]."""
    x = float(f32(p)) / 100 * (n - 1)
    fl = math.floor(x)
    idx = int(fl) + (1 if x - fl >= 0.5 else 0)
    return max(0, min(n - 1, idx))


def percentile(elems, p):
    """Percentile<T> (math.h:231-246): NaN orders last."""
    ordered = sorted(elems, key=lambda v: (v != v, v))
    return ordered[percentile_index(p, len(ordered))]


def min_angle_rad(deg):
    return f32(float(deg) * DEG_TO_RAD)


def item_quotient(c1, c2, X):
    """The argument of acos in CalculateTriangulationAngle, or None where the denominator is 0 (the angle is 0 then)."""
    d = [c1[k] - c2[k] for k in range(3)]
    b = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
    d = [X[k] - c1[k] for k in range(3)]
    r1 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
    d = [X[k] - c2[k] for k in range(3)]
    r2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
    den = 2.0 * math.sqrt(r1 * r2)
    if den == 0.0:
        return None
    return ((r1 + r2) - b) / den


def angle_of_quotient(q, acos=math.acos):
    """min(|acos q|, pi - |acos q|) narrowed to float (a numpy.float32); NaN where q left [-1, 1]."""
    if q is None:
        return f32(0.0)
    if not (-1.0 <= q <= 1.0):
        return f32(NAN)
    a = abs(acos(q))
    o = math.pi - a
    return f32(o if o < a else a)


def triangulation_angle(c1, c2, X, acos=math.acos):
    return angle_of_quotient(item_quotient(c1, c2, X), acos)


def items(R, T, xyz, tracks):
    """Every item in the reference's order: (point, i, j, image[i], image[j], quotient or None)."""
    R = np.asarray(R, dtype=f32).reshape(-1, 9)
    T = np.asarray(T, dtype=f32).reshape(-1, 3)
    xyz = np.asarray(xyz, dtype=f32).reshape(-1, 3)
    centers = [projection_center(R[a], T[a]) for a in range(len(R))]
    for p, track in enumerate(tracks):
        X = [float(v) for v in xyz[p]]
        for i in range(len(track)):
            for j in range(i):
                i1, i2 = int(track[i]), int(track[j])
                if i1 != i2:
                    yield p, i, j, i1, i2, item_quotient(centers[i1], centers[i2], X)


def select(R, T, xyz, tracks, max_num_src_images=20, min_triangulation_angle=1.0, triangulation_angle_percentile=75.0,
           candidate_mask=None, acos=math.acos):
    """-> {"sources": list of lists, "depth_ranges": [n][2] float32, "pairs": (a, b, count, angle) arrays in ascending (a, b),
    "items", "n_pairs", "nan_items"}."""
    R = np.asarray(R, dtype=f32).reshape(-1, 9)
    T = np.asarray(T, dtype=f32).reshape(-1, 3)
    xyz = np.asarray(xyz, dtype=f32).reshape(-1, 3)
    n = len(R)
    assert len(T) == n and len(xyz) == len(tracks)
    # ComputeDepthRanges
    depths = [[] for _ in range(n)]
    for p, track in enumerate(tracks):
        for a in track:
            d = depth(R[a], T[a], xyz[p])
            if d > 0:
                depths[a].append(d)
    ranges = np.full((n, 2), -1.0, dtype=f32)
    for a in range(n):
        if not depths[a]:
            continue
        d = sorted(depths[a])
        ranges[a, 0] = d[depth_index(len(d), 0.01)] * (f32(1.0) - f32(0.25))
        ranges[a, 1] = d[depth_index(len(d), 0.99)] * (f32(1.0) + f32(0.25))
    # ComputeSharedPoints and ComputeTriangulationAngles: the value of an item is symmetric in its two images, so a pair's count
    # and angles are kept once
    angles = {}
    n_items = nan_items = 0
    for p, i, j, i1, i2, q in items(R, T, xyz, tracks):
        ang = angle_of_quotient(q, acos)
        n_items += 1
        nan_items += int(ang != ang)
        angles.setdefault((min(i1, i2), max(i1, i2)), []).append(ang)
    keys = sorted(angles)
    count = {k: len(angles[k]) for k in keys}
    pangle = {k: percentile(angles[k], triangulation_angle_percentile) for k in keys}
    # GetMaxOverlappingImages
    thr = min_angle_rad(min_triangulation_angle)
    neighbours = [[] for _ in range(n)]
    for (a, b) in keys:
        if pangle[(a, b)] >= thr:
            if candidate_mask is None or candidate_mask[b]:
                neighbours[a].append((b, count[(a, b)]))
            if candidate_mask is None or candidate_mask[a]:
                neighbours[b].append((a, count[(a, b)]))
    sources = []
    for a in range(n):
        ordered = sorted(neighbours[a], key=lambda bc: (-bc[1], bc[0]))
        sources.append([b for b, _ in ordered[:min(len(ordered), int(max_num_src_images))]])
    pairs = (np.array([k[0] for k in keys], dtype=np.uint32), np.array([k[1] for k in keys], dtype=np.uint32),
             np.array([count[k] for k in keys], dtype=np.uint32), np.array([pangle[k] for k in keys], dtype=f32))
    return {"sources": sources, "depth_ranges": ranges, "pairs": pairs, "items": n_items, "n_pairs": len(keys), "nan_items": nan_items}
