"""The normative restatement of StereoFusion (src/mvs/fusion.cc:58-79, 169-293, 295-473) in numpy float32 scalars -- DESIGN.md 26.

Written from the reference's text, independently of csrc/stereo_fusion.h: every operation is one IEEE float operation in the
reference's evaluation order (numpy scalars never contract).  The rulings the reference leaves open:
  * P * v, inv_P * v, inv_R * n: each row summed left to right, ((m0 v0 + m1 v1) + m2 v2) + m3 v3; so are the dot product and
    the squared norm;
  * std::round is half away from zero; a projected coordinate that is NaN or not below 2^31 in magnitude is outside the map;
  * a NaN that arithmetic produces fails the test it enters (inputs must be finite);
  * the visibility list of a point is in ascending image index.

An image is a dict: used, depth [h][w] float32, normal [3][h][w] float32, rgb [bh][bw][3] uint8, P [12], inv_P [12], inv_R [9]
float32 and scale [2] float32 (depth-map size / bitmap size).  overlap is a list of lists of image indices.

run() is the reference's loop, seed after seed.  run_rounds() is the device's schedule -- speculate every pending seed against
the committed masks, claim, commit in rank order below the barrier -- written a second time here so that the CPU suite shows
the two equal without a GPU."""
import math

import numpy as np

f32 = np.float32
FLT_EPSILON = f32(1.1920928955078125e-07)

# StereoFusionOptions, src/mvs/fusion.h:55-85: the doubles hold float literals
DEFAULTS = {"min_num_pixels": 5, "max_num_pixels": 10000, "max_traversal_depth": 100, "max_reproj_error": float(f32(2.0)),
            "max_depth_error": float(f32(0.01)), "max_normal_error": float(f32(10.0))}


def check_options(o):
    """Check() (fusion.cc:98-108) plus min_num_pixels >= 1 (Median CHECKs a non-empty vector); a NaN fails."""
    return (o["min_num_pixels"] >= 1 and o["min_num_pixels"] <= o["max_num_pixels"] and o["max_traversal_depth"] > 0
            and o["max_reproj_error"] >= 0 and o["max_depth_error"] >= 0 and o["max_normal_error"] >= 0)


def median(elems):
    """internal::Median (fusion.cc:40-53): a float."""
    a = sorted(elems)
    n = len(a)
    assert n > 0
    mid = n // 2
    if n % 2 == 0:
        return (f32(a[mid]) + f32(max(a[:mid]))) / f32(2.0)
    return f32(a[mid])


def find_next_image(overlap, used, fused, prev):
    """internal::FindNextImage (fusion.cc:58-79)."""
    for i in overlap[prev]:
        if used[i] and not fused[i]:
            return i
    for i in range(len(fused)):
        if used[i] and not fused[i]:
            return i
    return -1


def image_order(overlap, used):
    """The images in the order Run()'s loop visits them (:239-241): it starts at 0 whether or not image 0 is used."""
    if not len(used):
        return []
    fused = [False] * len(used)
    order, cur = [], 0
    while cur >= 0:
        order.append(cur)
        fused[cur] = True
        cur = find_next_image(overlap, used, fused, cur)
    return order


def _row4(m, r, v0, v1, v2, v3):
    return ((m[4 * r] * v0 + m[4 * r + 1] * v1) + m[4 * r + 2] * v2) + m[4 * r + 3] * v3


def _row3(m, r, v0, v1, v2):
    return (m[3 * r] * v0 + m[3 * r + 1] * v1) + m[3 * r + 2] * v2


def round_index(x, size):
    """static_cast<int>(std::round(x)) as an index below size, or -1 (outside; NaN and |x| >= 2^31 included)."""
    x = float(x)
    if x != x or abs(x) >= 2147483648.0:
        return -1
    r = math.floor(abs(x) + 0.5)
    if x < 0 and r > 0:
        return -1
    return int(r) if r < size else -1


class Fusion:
    def __init__(self, images, overlap, options=None):
        self.o = dict(DEFAULTS)
        self.o.update(options or {})
        assert check_options(self.o)
        self.images = images
        self.overlap = overlap
        self.n = len(images)
        self.used = [bool(im["used"]) for im in images]
        self.fused = [False] * self.n
        self.masks = [np.zeros(im["depth"].shape, dtype=bool) if u else np.zeros((0, 0), dtype=bool) for im, u in zip(images, self.used)]
        self.max_sq_reproj = f32(self.o["max_reproj_error"] * self.o["max_reproj_error"])   # fusion.cc:120-121
        self.min_cos = f32(math.cos(self.o["max_normal_error"] * 0.0174532925199432954743716805978692718781530857086181640625))  # :122
        self.points, self.colours, self.vis = [], [], []
        self.stats = {"traversals": 0, "breaks": 0, "depth_hits": 0, "rounds": []}

    def pixel_values(self, image, row, col, depth):
        im = self.images[image]
        nm = im["normal"]
        n = [_row3(im["inv_R"], r, nm[0, row, col], nm[1, row, col], nm[2, row, col]) for r in range(3)]
        a, b = f32(col) * depth, f32(row) * depth
        xyz = [_row4(im["inv_P"], r, a, b, depth, f32(1.0)) for r in range(3)]
        return xyz, n

    def colour(self, image, row, col):
        im = self.images[image]
        bh, bw = im["rgb"].shape[:2]
        xx = round_index(f32(col) / im["scale"][0], bw)
        yy = round_index(f32(row) / im["scale"][1], bh)
        if xx < 0 or yy < 0:
            return (0, 0, 0)
        return tuple(int(c) for c in im["rgb"][yy, xx])

    def traverse(self, image, row, col, own=None):
        """The while loop of Fuse() (:312-437).  own None: marks are made in the masks at once (the reference).  own a set:
        the masks are only read and `own` collects the marks this seed would make.
        -> (accepted [(image, row, col)], values [(xyz, normal, rgb)], limit)."""
        o = self.o
        queue = [(image, row, col, 0)]
        acc, vals = [], []
        limit = False
        ref, ref_n = None, None
        one = f32(1.0)
        self.stats["traversals"] += 1
        while queue:
            image, row, col, td = queue.pop()
            if self.masks[image][row, col] or (own is not None and (image, row, col) in own):
                continue
            im = self.images[image]
            depth = im["depth"][row, col]
            if depth <= 0:
                continue
            if td > 0:
                P = im["P"]
                p0, p1, p2 = (_row4(P, r, ref[0], ref[1], ref[2], one) for r in range(3))
                depth_error = abs((p2 - depth) / depth)
                if not float(depth_error) <= o["max_depth_error"]:
                    continue
                col_diff = p0 / p2 - f32(col)
                row_diff = p1 / p2 - f32(row)
                if not col_diff * col_diff + row_diff * row_diff <= self.max_sq_reproj:
                    continue
            xyz, normal = self.pixel_values(image, row, col, depth)
            if td > 0:
                cos_err = (ref_n[0] * normal[0] + ref_n[1] * normal[1]) + ref_n[2] * normal[2]
                if not cos_err >= self.min_cos:
                    continue
            if own is None:
                self.masks[image][row, col] = True
            else:
                own.add((image, row, col))
            acc.append((image, row, col))
            vals.append((xyz, normal, self.colour(image, row, col)))
            if td == 0:
                ref, ref_n = xyz, normal
            if len(acc) >= o["max_num_pixels"]:
                self.stats["breaks"] += 1
                limit = True
                break
            if td + 1 >= o["max_traversal_depth"]:
                self.stats["depth_hits"] += 1
                limit = True
                continue
            for nxt in self.overlap[image]:
                if not self.used[nxt] or self.fused[nxt]:
                    continue
                nim = self.images[nxt]
                q0, q1, q2 = (_row4(nim["P"], r, xyz[0], xyz[1], xyz[2], one) for r in range(3))
                h, w = nim["depth"].shape
                ncol = round_index(q0 / q2, w)
                nrow = round_index(q1 / q2, h)
                if ncol < 0 or nrow < 0:
                    continue
                queue.append((nxt, nrow, ncol, td + 1))
        return acc, vals, limit

    def finish(self, acc, vals):
        """The tail of Fuse() (:441-472) -> (point [6] float32, colour [3] uint8, visibility) or None."""
        if len(acc) < self.o["min_num_pixels"]:
            return None
        nx, ny, nz = (median([v[1][k] for v in vals]) for k in range(3))
        norm = np.sqrt((nx * nx + ny * ny) + nz * nz)
        if norm < FLT_EPSILON:
            return None
        x, y, z = (median([v[0][k] for v in vals]) for k in range(3))
        rgb = []
        for k in range(3):
            m = float(median([np.uint8(v[2][k]) for v in vals]))
            r = math.floor(abs(m) + 0.5) * (1 if m >= 0 else -1)
            rgb.append(min(max(int(r), 0), 255))
        return (np.array([x, y, z, nx / norm, ny / norm, nz / norm], dtype=f32), np.array(rgb, dtype=np.uint8),
                sorted(set(a[0] for a in acc)))

    def _emit(self, point):
        if point is not None:
            self.points.append(point[0])
            self.colours.append(point[1])
            self.vis.append(point[2])

    def run(self):
        """Run()'s loop (:239-279), seed after seed."""
        with np.errstate(all="ignore"):
            for image in image_order(self.overlap, self.used):
                if self.used[image]:
                    h, w = self.images[image]["depth"].shape
                    for row in range(h):
                        for col in range(w):
                            if self.masks[image][row, col]:
                                continue
                            acc, vals, _ = self.traverse(image, row, col)
                            self._emit(self.finish(acc, vals))
                self.fused[image] = True
        return self.result()

    def run_rounds(self):
        """The device's schedule: every pending seed of the image traverses against the committed masks; a pixel
        is claimed by the lowest rank that accepted it; a seed commits when it holds every claim of its list and its rank is at
        most the barrier, the lowest rank among the seeds that are not free and hit a limit."""
        with np.errstate(all="ignore"):
            for image in image_order(self.overlap, self.used):
                rounds = 0
                if self.used[image]:
                    h, w = self.images[image]["depth"].shape
                    depth = self.images[image]["depth"]
                    pending = [s for s in range(h * w) if not self.masks[image][s // w, s % w] and depth[s // w, s % w] > 0]
                    done, runs = {}, {}
                    while pending:
                        rounds += 1
                        pending = [s for s in pending if not self.masks[image][s // w, s % w]]  # a seed whose pixel got masked dies
                        claim = {}
                        for s in pending:
                            # masked and rejected pixels act alike on a traversal, so it stands until one of ITS pixels is masked
                            if s not in runs or any(self.masks[a[0]][a[1], a[2]] for a in runs[s][0]):
                                runs[s] = self.traverse(image, s // w, s % w, own=set())
                            acc = runs[s][0]
                            for a in acc:
                                claim[a] = min(claim.get(a, s), s)
                        free = {s: all(claim[a] == s for a in runs[s][0]) for s in pending}
                        barrier = min([s for s in pending if not free[s] and runs[s][2]], default=h * w)
                        left = []
                        for s in pending:
                            if free[s] and s <= barrier:
                                acc, vals, _ = runs[s]
                                for a in acc:
                                    self.masks[a[0]][a[1], a[2]] = True
                                done[s] = self.finish(acc, vals)
                            else:
                                left.append(s)
                        assert len(left) < len(pending) or not pending, "a round without progress"
                        pending = left
                    for s in sorted(done):
                        self._emit(done[s])
                self.stats["rounds"].append(rounds)
                self.fused[image] = True
        return self.result()

    def result(self):
        n = len(self.points)
        return {"points": np.array(self.points, dtype=f32).reshape(n, 6), "colours": np.array(self.colours, dtype=np.uint8).reshape(n, 3),
                "visibility": [list(v) for v in self.vis], "masks": self.masks, "stats": self.stats}


def fuse(images, overlap, options=None, rounds=False):
    f = Fusion(images, overlap, options)
    return f.run_rounds() if rounds else f.run()
