"""What the PatchMatch GPU tests share: cached scenes, the reference result of a problem computed once
(tests/patch_match_ref.py), the translation of the options, and the bit comparison of every output array."""
import functools

import numpy as np

from tests import patch_match_ref as ref
from tests import patch_match_scenes as scenes


@functools.lru_cache(maxsize=None)
def scene(kind, sizes, seed=0):
    """sizes: a tuple of (width, height) per view."""
    images, truth = scenes.make_scene(kind, n_views=len(sizes), sizes=list(sizes), seed=seed)
    return images, truth


def options(**kw):
    """Small defaults for the tests; every field can be overridden."""
    base = dict(window_radius=2, num_samples=3, num_iterations=1, geom_consistency=False, filter=False, seed=11)
    base.update(kw)
    return ref.Options(**base)


def capi_options(o):
    from dagsfm_amd import capi
    d = o.as_dict()
    d["geom_consistency"], d["filter"] = int(d["geom_consistency"]), int(d["filter"])
    return capi.default_patch_match_options(**d)


_cache = {}


def reference(scene_key, images, problem, o):
    """ref.patch_match of one problem, computed once per (scene, problem, options); the result is shared: do not write to it."""
    key = (scene_key, problem[0], tuple(problem[1]), float(problem[2]), float(problem[3]), tuple(sorted(o.as_dict().items())))
    if key not in _cache:
        r = ref.patch_match(images, problem[0], problem[1], problem[2], problem[3], o)
        for v in r.values():
            if v is not None:
                v.setflags(write=False)
        _cache[key] = r
    return _cache[key]


def assert_same_bits(got, want, what=""):
    """Every output array with == on the bits: the float maps as uint32, the mask as bytes."""
    for name in ("depth", "normal", "sel_prob", "mask"):
        g, w = got[name], want[name]
        if w is None or g is None:
            assert name in ("sel_prob", "mask") and (g is None or name == "sel_prob"), (what, name)
            continue
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape, g.dtype, w.dtype)
        gb = np.ascontiguousarray(g).view(np.uint32 if g.dtype == np.float32 else np.uint8)
        wb = np.ascontiguousarray(w).view(np.uint32 if w.dtype == np.float32 else np.uint8)
        bad = np.argwhere(gb != wb)
        assert len(bad) == 0, "%s %s: %d of %d elements differ, first at %s: %r vs %r" % (
            what, name, len(bad), gb.size, bad[0].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])
