"""Sequential numpy restatement of the undistortion stage: UndistortCamera, the point loop of
UndistortReconstruction, Camera::Rescale, the three warps of warp.cc up to their final Bitmap::Rescale, and
Bitmap::InterpolateBilinear + BitmapColor<float>::Cast<uint8_t>.

ImageToWorld is the oracle's (oracle.image_to_world).  The forward model is written in the order of
point_filter_ref.world_to_image, with atan / tan through the oracle's correctly rounded ones (oracle_exact_trig), which is what
the device's exact_trig.h computes.  std::min(a, b) is (b < a) ? b : a, std::max(a, b) is (a < b) ? b : a and Clip is
max(low, min(value, high)): with these a NaN scale clips to min_scale, as the reference's does.
"""
import ctypes
import math

import numpy as np

from dagsfm_amd import capi

EPS = float(np.finfo(np.float64).eps)
DBL_MAX = float(np.finfo(np.float64).max)
TWO_FOCAL = (1, 4, 5, 6, 7, 10)
SIZE_ONLY = -1
_DP = ctypes.POINTER(ctypes.c_double)


def default_options(**kw):
    o = dict(blank_pixels=0.0, min_scale=0.2, max_scale=2.0, max_image_size=-1, roi_min_x=0.0, roi_min_y=0.0, roi_max_x=1.0,
             roi_max_y=1.0)
    o.update(kw)
    return o


def std_min(a, b):
    return b if b < a else a


def std_max(a, b):
    return b if a < b else a


def clip(value, low, high):
    return std_max(low, std_min(value, high))


def c_round(x):
    """std::round of a non-negative double: half away from zero."""
    f = math.floor(x)
    return f + 1.0 if x - f >= 0.5 else f


def _xt(oracle, kind, x):
    """The oracle's exact atan (kind 0) / tan (kind 3) of an array."""
    a = np.ascontiguousarray(np.broadcast_to(np.asarray(x, np.float64), np.shape(x)), np.float64).reshape(-1)
    out = np.zeros_like(a)
    if len(a):
        oracle.lib.oracle_exact_trig(kind, a.ctypes.data_as(_DP), len(a), out.ctypes.data_as(_DP))
    return out.reshape(np.shape(x))


def params_of(cam):
    return [float(cam.params[i]) for i in range(capi.CAMERA_MODEL_NUM_PARAMS[cam.model_id])]


def world_to_image(oracle, model, p, u, v):
    """CameraModel::WorldToImage in ba_project.h's order for arrays u, v."""
    p = [float(x) for x in p]
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    with np.errstate(all="ignore"):
        if model not in TWO_FOCAL:
            du, dv = _distortion(oracle, model, p[3:], u, v)
            return p[0] * (u + du) + p[1], p[0] * (v + dv) + p[2]
        if model == 7:
            omega = p[4]
            radius2 = u * u + v * v
            omega2 = omega * omega
            if omega2 < 1e-4:
                factor = (omega2 * radius2) / 3.0 - omega2 / 12.0 + 1.0
            else:
                t = float(_xt(oracle, 3, np.array([omega / 2.0]))[0])
                small = (-2.0 * t * (4.0 * radius2 * t * t - 3.0)) / (3.0 * omega)
                radius = np.sqrt(radius2)
                big = _xt(oracle, 0, radius * 2.0 * t) / (radius * omega)
                factor = np.where(radius2 < 1e-4, small, big)
            return p[0] * (u * factor) + p[2], p[1] * (v * factor) + p[3]
        if model == 10:
            r = np.sqrt(u * u + v * v)
            theta = _xt(oracle, 0, r)
            ok = r > EPS
            rs = np.where(ok, r, 1.0)
            u, v = np.where(ok, theta * u / rs, u), np.where(ok, theta * v / rs, v)
        du, dv = _distortion(oracle, model, p[4:], u, v)
        return p[0] * (u + du) + p[2], p[1] * (v + dv) + p[3]


def _distortion(oracle, model, e, u, v):
    if model == 2:
        r2 = u * u + v * v
        radial = e[0] * r2
        return u * radial, v * radial
    if model == 3:
        r2 = u * u + v * v
        radial = e[0] * r2 + e[1] * r2 * r2
        return u * radial, v * radial
    if model == 4:
        u2, uv, v2 = u * u, u * v, v * v
        r2 = u2 + v2
        radial = e[0] * r2 + e[1] * r2 * r2
        return (u * radial + 2.0 * e[2] * uv + e[3] * (r2 + 2.0 * u2), v * radial + 2.0 * e[3] * uv + e[2] * (r2 + 2.0 * v2))
    if model in (5, 8, 9):
        r = np.sqrt(u * u + v * v)
        ok = r > EPS
        rs = np.where(ok, r, 1.0)
        theta = _xt(oracle, 0, r)
        theta2 = theta * theta
        if model == 8:
            thetad = theta * (1.0 + e[0] * theta2)
        elif model == 9:
            theta4 = theta2 * theta2
            thetad = theta * (1.0 + e[0] * theta2 + e[1] * theta4)
        else:
            theta4 = theta2 * theta2
            theta6 = theta4 * theta2
            theta8 = theta4 * theta4
            thetad = theta * (1.0 + e[0] * theta2 + e[1] * theta4 + e[2] * theta6 + e[3] * theta8)
        return np.where(ok, u * thetad / rs - u, u * 0.0), np.where(ok, v * thetad / rs - v, v * 0.0)
    if model == 6:
        u2, uv, v2 = u * u, u * v, v * v
        r2 = u2 + v2
        r4 = r2 * r2
        r6 = r4 * r2
        radial = (1.0 + e[0] * r2 + e[1] * r4 + e[4] * r6) / (1.0 + e[5] * r2 + e[6] * r4 + e[7] * r6)
        return (u * radial + 2.0 * e[2] * uv + e[3] * (r2 + 2.0 * u2) - u, v * radial + 2.0 * e[3] * uv + e[2] * (r2 + 2.0 * v2) - v)
    if model == 10:
        u2, uv, v2 = u * u, u * v, v * v
        r2 = u2 + v2
        r4 = r2 * r2
        r6 = r4 * r2
        r8 = r6 * r2
        radial = e[0] * r2 + e[1] * r4 + e[4] * r6 + e[5] * r8
        return (u * radial + 2.0 * e[2] * uv + e[3] * (r2 + 2.0 * u2) + e[6] * r2,
                v * radial + 2.0 * e[3] * uv + e[2] * (r2 + 2.0 * v2) + e[7] * r2)
    return u * 0.0, v * 0.0


def image_to_world(oracle, cam, x, y):
    """Camera::ImageToWorld of arrays x, y: the oracle's, point by point."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    xs, ys = np.broadcast_arrays(x, y)
    out = np.zeros(xs.shape + (2,))
    flat = out.reshape(-1, 2)
    for i, (a, b) in enumerate(zip(xs.reshape(-1), ys.reshape(-1))):
        flat[i] = oracle.image_to_world(cam, np.array([a, b]))
    return out[..., 0], out[..., 1]


def _pp_idx(model):
    return (2, 3) if model in TWO_FOCAL else (1, 2)


def rescale_to_size(cam, width, height):
    """Camera::Rescale(width, height), camera.cc:249-267."""
    c = capi.copy_camera(cam)
    scale_x = float(width) / float(cam.width)
    scale_y = float(height) / float(cam.height)
    c.width, c.height = width, height
    ix, iy = _pp_idx(cam.model_id)
    c.params[ix] = scale_x * cam.params[ix]
    c.params[iy] = scale_y * cam.params[iy]
    if cam.model_id in TWO_FOCAL:
        c.params[0] = scale_x * cam.params[0]
        c.params[1] = scale_y * cam.params[1]
    else:
        c.params[0] = (scale_x + scale_y) / 2.0 * cam.params[0]
    return c


def rescale_by(cam, scale):
    """Camera::Rescale(scale), camera.cc:228-247."""
    c = capi.copy_camera(cam)
    scale_x = c_round(scale * cam.width) / float(cam.width)
    scale_y = c_round(scale * cam.height) / float(cam.height)
    c.width = int(c_round(scale * cam.width))
    c.height = int(c_round(scale * cam.height))
    ix, iy = _pp_idx(cam.model_id)
    c.params[ix] = scale_x * cam.params[ix]
    c.params[iy] = scale_y * cam.params[iy]
    if cam.model_id in TWO_FOCAL:
        c.params[0] = scale_x * cam.params[0]
        c.params[1] = scale_y * cam.params[1]
    else:
        c.params[0] = (scale_x + scale_y) / 2.0 * cam.params[0]
    return c


def _div(a, b):
    """IEEE division of two Python floats (x / 0 is an infinity or a NaN, not an exception)."""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def undistort_camera(oracle, cam, **options):
    """UndistortCamera, undistortion.cc:659-842 (the options are assumed to pass its CHECKs)."""
    o = default_options(**options)
    W, Hh = int(cam.width), int(cam.height)
    two = cam.model_id in TWO_FOCAL
    fx = float(cam.params[0])
    fy = float(cam.params[1]) if two else fx
    cx, cy = float(cam.params[2 if two else 1]), float(cam.params[3 if two else 2])
    uw, uh = W, Hh
    x0, y0, x1, y1 = 0, 0, W, Hh
    roi = o["roi_min_x"] > 0.0 or o["roi_min_y"] > 0.0 or o["roi_max_x"] < 1.0 or o["roi_max_y"] < 1.0
    if roi:
        x0, y0 = int(c_round(o["roi_min_x"] * float(W))), int(c_round(o["roi_min_y"] * float(Hh)))
        x1, y1 = int(c_round(o["roi_max_x"] * float(W))), int(c_round(o["roi_max_y"] * float(Hh)))
        x0, y0 = min(x0, W - 1), min(y0, Hh - 1)
        x1, y1 = max(x1, x0 + 1), max(y1, y0 + 1)
        uw, uh = x1 - x0, y1 - y0
        cx, cy = cx - float(x0), cy - float(y0)
    if roi or cam.model_id not in (0, 1):
        with np.errstate(all="ignore"):
            left_min = right_min = top_min = bottom_min = DBL_MAX
            left_max = right_max = top_max = bottom_max = -DBL_MAX
            for y in range(y0, y1):
                u, _ = oracle.image_to_world(cam, np.array([0.5, y + 0.5]))
                px = float(np.float64(fx) * u + np.float64(cx))
                left_min, left_max = std_min(left_min, px), std_max(left_max, px)
                u, _ = oracle.image_to_world(cam, np.array([W - 0.5, y + 0.5]))
                px = float(np.float64(fx) * u + np.float64(cx))
                right_min, right_max = std_min(right_min, px), std_max(right_max, px)
            for x in range(x0, x1):
                _, v = oracle.image_to_world(cam, np.array([x + 0.5, 0.5]))
                py = float(np.float64(fy) * v + np.float64(cy))
                top_min, top_max = std_min(top_min, py), std_max(top_max, py)
                _, v = oracle.image_to_world(cam, np.array([x + 0.5, Hh - 0.5]))
                py = float(np.float64(fy) * v + np.float64(cy))
                bottom_min, bottom_max = std_min(bottom_min, py), std_max(bottom_max, py)
            f = np.float64
            min_scale_x = std_min(_div(cx, f(cx) - f(left_min)), _div(f(uw) - 0.5 - f(cx), f(right_max) - f(cx)))
            min_scale_y = std_min(_div(cy, f(cy) - f(top_min)), _div(f(uh) - 0.5 - f(cy), f(bottom_max) - f(cy)))
            max_scale_x = std_max(_div(cx, f(cx) - f(left_max)), _div(f(uw) - 0.5 - f(cx), f(right_min) - f(cx)))
            max_scale_y = std_max(_div(cy, f(cy) - f(top_max)), _div(f(uh) - 0.5 - f(cy), f(bottom_min) - f(cy)))
            bp = f(o["blank_pixels"])
            scale_x = _div(1.0, f(min_scale_x) * bp + f(max_scale_x) * (f(1.0) - bp))
            scale_y = _div(1.0, f(min_scale_y) * bp + f(max_scale_y) * (f(1.0) - bp))
            scale_x = clip(scale_x, o["min_scale"], o["max_scale"])
            scale_y = clip(scale_y, o["min_scale"], o["max_scale"])
            ow, oh = uw, uh
            uw = int(std_max(1.0, scale_x * uw))
            uh = int(std_max(1.0, scale_y * uh))
            cx = cx * float(uw) / float(ow)
            cy = cy * float(uh) / float(oh)
    out = capi.camera(1, [fx, fy, cx, cy], uw, uh, prior=False)
    if o["max_image_size"] > 0:
        s = std_min(o["max_image_size"] / float(uw), o["max_image_size"] / float(uh))
        if s < 1.0:
            out = rescale_by(out, s)
    return out


def undistort_points2D(oracle, cameras, undistorted, camera_index, xy):
    """The loop of UndistortReconstruction, undistortion.cc:869-879."""
    xy = np.array(xy, np.float64).reshape(-1, 2)
    out = np.zeros_like(xy)
    for i, c in enumerate(np.asarray(camera_index).reshape(-1)):
        u, v = oracle.image_to_world(cameras[c], xy[i])
        x, y = world_to_image(oracle, undistorted[c].model_id, params_of(undistorted[c]), np.array([u]), np.array([v]))
        out[i] = (x[0], y[0])
    return out


def interpolate_bilinear_u8(image, sx, sy):
    """Bitmap::InterpolateBilinear(sx - 0.5, sy - 0.5) followed by Cast<uint8_t> at the arrays sx, sy of one shape.  image:
    uint8 [height, width] or [height, width, channels], rows top-down (FreeImage's scanline k is row height - 1 - k).  0 where
    the reference refuses the sample, and where the coordinate is NaN or its floor outside int."""
    im = np.asarray(image)
    h, w = im.shape[:2]
    px = im.reshape(h, w, -1).astype(np.float64)
    with np.errstate(all="ignore"):
        x = np.asarray(sx, np.float64) - 0.5
        y = np.asarray(sy, np.float64) - 0.5
        inv_y = float(h - 1) - y
        fx, fy = np.floor(x), np.floor(inv_y)
        in_int = (fx >= -2147483648.0) & (fx <= 2147483647.0) & (fy >= -2147483648.0) & (fy <= 2147483647.0)
        ok = in_int & (fx >= 0) & (fx + 1 < w) & (fy >= 0) & (fy + 1 < h)
        x0 = np.where(ok, fx, 0).astype(np.int64)
        y0 = np.where(ok, fy, 0).astype(np.int64)
        x1 = np.minimum(x0 + 1, w - 1)
        y1 = np.minimum(y0 + 1, h - 1)
        dx = np.where(ok, x - x0, 0.0)[..., None]
        dy = np.where(ok, inv_y - y0, 0.0)[..., None]
        dx_1, dy_1 = 1 - dx, 1 - dy
        r0, r1 = h - 1 - y0, h - 1 - y1
        v0 = dx_1 * px[r0, x0] + dx * px[r0, x1]
        v1 = dx_1 * px[r1, x0] + dx * px[r1, x1]
        value = (dy_1 * v0 + dy * v1).astype(np.float32)  # BitmapColor<float>
        t = np.trunc(value)
        r = t + (value - t >= np.float32(0.5))  # std::round of a non-negative float
        r = np.minimum(np.float32(255), np.maximum(np.float32(0), r))
    out = np.where(ok[..., None], r, 0).astype(np.uint8)
    return out.reshape(ok.shape + im.shape[2:])


def source_points(oracle, source, target, H=None, target_size=None):
    """The source point (before the - 0.5) of every target pixel, [height, width, 2], the scaled target camera and whether the
    reference's final Rescale is owed.  source / target: Camera, or a size-only Camera / None for WarpImageWithHomography."""
    size_only = source.model_id == SIZE_ONLY
    sw, sh = int(source.width), int(source.height)
    tw, th = (int(target.width), int(target.height)) if (size_only and target is not None) else (sw, sh)
    ys, xs = np.mgrid[0:th, 0:tw]
    ix, iy = xs + 0.5, ys + 0.5
    owed = False
    scaled = capi.copy_camera(source if target is None else target)
    if not size_only and (int(target.width) != sw or int(target.height) != sh):
        scaled = rescale_to_size(target, sw, sh)
        owed = True
    with np.errstate(all="ignore"):
        if H is None:
            u, v = image_to_world(oracle, scaled, ix, iy)
        else:
            Hm = np.asarray(H, np.float64).reshape(3, 3)
            w0 = (Hm[0, 0] * ix + Hm[0, 1] * iy) + Hm[0, 2]
            w1 = (Hm[1, 0] * ix + Hm[1, 1] * iy) + Hm[1, 2]
            w2 = (Hm[2, 0] * ix + Hm[2, 1] * iy) + Hm[2, 2]
            hx, hy = w0 / w2, w1 / w2
            if size_only:
                return np.stack([hx, hy], -1), scaled, owed
            u, v = image_to_world(oracle, target, hx, hy)  # warp.cc:154: the unscaled target
        sx, sy = world_to_image(oracle, source.model_id, params_of(source), u, v)
    return np.stack([sx, sy], -1), scaled, owed


def warp_images(oracle, source, target, images, H=None):
    """{"images", "source_xy", "scaled_target", "needs_rescale"} of Context.warp_images for images [n, h, w] or [n, h, w, c]."""
    images = np.asarray(images)
    sxy, scaled, owed = source_points(oracle, source, target, H)
    out = np.stack([interpolate_bilinear_u8(im, sxy[..., 0], sxy[..., 1]) for im in images]) if len(images) else \
        np.zeros((0,) + sxy.shape[:2] + images.shape[3:], np.uint8)
    return {"images": out, "source_xy": sxy, "scaled_target": scaled, "needs_rescale": owed}


def cameras_equal(a, b):
    return bytes(a) == bytes(b)
