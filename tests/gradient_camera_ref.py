"""numpy restatement, in f64, of the temporal gradient under a moving camera (include/pathtrace_amd.h): the
lookup of pt_temporal_gradient_camera_device on top of tests/gradient_ref.py (strata, records, the per-pixel rule) and
tests/temporal_ref.reproject (rule 2 of PtTemporal).  Written from the rule's statement, not from the C++.

The lookup is an integer, so two computations of x' can disagree only where x' + 0.5 or y' + 0.5 is next to an integer:
lookup() also returns that band (BAND wide), which the tests leave out and cap at BAND_CAP of the image."""
import numpy as np

import gradient_ref as gr
import temporal_ref as tr

BAND = 1e-6
BAND_CAP = 0.01
W, H = 47, 31                      # clipped strata at the right and bottom edges: 16 x 11 strata


def cameras(pt, w=W, h=H):
    """(previous, current): the default camera, and one moved by a non-round fraction of a pixel's footprint (about 1.7 mm
    at the Cornell box's back wall for 47 pixels) and turned a little by look_at."""
    prev = pt.camera_new(width=w, height=h)
    cur = pt.camera_look_at((0.0437, 0.0213, 1.9871), (0.0113, -0.0071, 0.0), (0.0, 1.0, 0.0), w, h, 35.0)
    return prev, cur


def orbit(pt, k, w, h, step=0.006):
    """Camera k of an orbit of radius 2 around the box's centre (k = 0: on the axis): the point of the circle whose half-angle
    tangent is step * k, in + - * / alone -- the statements of examples/gradient_frames.cpp --camera, the same bits."""
    t = step * k
    q = 1.0 + t * t
    return pt.camera_look_at((2.0 * (2.0 * t) / q, 0.0, 2.0 * (1.0 - t * t) / q), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), w, h, 35.0)


def same_camera(cam, prev_cam):
    return tr.cam_fields(cam) == tr.cam_fields(prev_cam)


def lookup_pixel(xr, yr, w, h):
    """The helper of pt_gradient.h: (x', y') -> (xi, yi, inside); xi = floor(x' + 0.5), yi = floor(y' + 0.5)."""
    xr, yr = np.asarray(xr, np.float64), np.asarray(yr, np.float64)
    with np.errstate(invalid="ignore"):
        fx, fy = np.floor(xr + 0.5), np.floor(yr + 0.5)
        inside = (fx >= 0) & (fx < w) & (fy >= 0) & (fy < h)
    xi = np.where(inside, fx, 0).astype(np.int64)
    yi = np.where(inside, fy, 0).astype(np.int64)
    return xi, yi, inside


def lookup(cam, prev_cam, depth):
    """Rule 2 of 5j for every pixel of cam; depth f32[H,W] (the features' lane 7).
    -> xi, yi int[H,W], ok bool[H,W] (False: the entry is NaN), band bool[H,W] (the lookup is within BAND of flipping)"""
    w, h = cam.width, cam.height
    assert (prev_cam.width, prev_cam.height) == (w, h)
    ys, xs = np.mgrid[0:h, 0:w]
    if same_camera(cam, prev_cam):
        return xs, ys, np.ones((h, w), bool), np.zeros((h, w), bool)
    d = np.asarray(depth, np.float32).astype(np.float64)
    xr, yr, _, _, ok = tr.reproject(cam, prev_cam, np.where(d > 0, d, 1.0))
    ok = ok & (d > 0)
    xi, yi, inside = lookup_pixel(np.where(ok, xr, -9.0), np.where(ok, yr, -9.0), w, h)
    with np.errstate(invalid="ignore"):
        band = ok & ((np.abs(xr + 0.5 - np.round(xr + 0.5)) < BAND) | (np.abs(yr + 0.5 - np.round(yr + 0.5)) < BAND))
    return xi, yi, ok & inside, band


def alpha_plane(rec, cam, prev_cam, depth, radius=1, scale=1.0, alpha_min=0.2):
    """d_alpha of pt_temporal_gradient_camera_device from the strata's records -> (f32[H,W], band)"""
    w, h = cam.width, cam.height
    xi, yi, ok, band = lookup(cam, prev_cam, depth)
    prev_plane = gr.alpha_plane(rec, w, h, radius, scale, alpha_min)       # the weight of every PREVIOUS-image pixel
    return np.where(ok, prev_plane[yi, xi], np.float32(np.nan)).astype(np.float32), band
