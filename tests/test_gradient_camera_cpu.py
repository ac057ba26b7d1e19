"""Temporal gradients under a moving camera without a device: the ABI (symbols, the argument checks that need no context),
the lookup helper of pathtrace_amd/csrc/pt_gradient.h compiled with the host compiler as the kernels include it against the
numpy restatement (tests/gradient_camera_ref.py) bit for bit, the restatement itself on a wall under a camera moved
sideways, and the near-boundary band of the camera moves the GPU tests use."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import denoise_ref as dr
import gradient_camera_ref as gc
import gradient_ref as gr
import temporal_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pt_temporal_gradient_camera_device", "pt_render_denoised_gradient_camera")
SRC = r"""
#include "pt_gradient.h"
extern "C" void gc_lookup(const double* xr, const double* yr, unsigned n, unsigned W, unsigned H, int* out) {
    for (unsigned k = 0; k < n; ++k) {
        unsigned xi = 77777u, yi = 88888u;
        out[3 * k] = ptgr::lookup_pixel(xr[k], yr[k], W, H, &xi, &yi) ? 1 : 0;
        out[3 * k + 1] = (int)xi;
        out[3 * k + 2] = (int)yi;
    }
}
extern "C" void gc_plane(const double* rec, const double* xr, const double* yr, unsigned W, unsigned H, unsigned radius, float scale,
                         float alpha_min, float* out) {
    for (unsigned p = 0; p < W * H; ++p) {
        unsigned xi, yi;
        out[p] = ptgr::lookup_pixel(xr[p], yr[p], W, H, &xi, &yi)
                     ? ptgr::pixel_alpha(rec, ptgr::strata(W), ptgr::strata(H), xi, yi, radius, scale, alpha_min) : __builtin_nanf("");
    }
}
"""
SIZES = ((2, 2), (4, 3), (7, 5), (16, 11), (47, 31))


def test_the_new_symbols_are_exported(pt):
    lib = pt._lib.lib()
    for name in NEW:
        assert name in pt._lib.SYMBOLS and hasattr(lib, name), name
    assert lib.pt_abi_version() == 6
    header = open(os.path.join(ROOT, "include", "pathtrace_amd.h")).read()
    for name in NEW:
        assert f"int {name}(" in header, name
    for name in ("temporal_gradient_camera", "render_denoised_gradient_camera"):
        assert hasattr(pt.Context, name)
    hpp = open(os.path.join(ROOT, "pathtrace_amd", "host", "pathtrace.hpp")).read()
    assert "void render_denoised_gradient_camera(" in hpp and "pt_render_denoised_gradient_camera" in hpp
    rs = open(os.path.join(ROOT, "rust", "pathtrace-amd-sys", "src", "lib.rs")).read()
    for name in NEW:
        assert f"pub fn {name}(" in rs, name
    gh = open(os.path.join(ROOT, "pathtrace_amd", "csrc", "pt_gradient.h")).read()
    assert "lookup_pixel(" in gh


def test_null_misaligned_and_mismatched_arguments_are_refused_without_a_device(pt):
    lib = pt._lib.lib()
    cam = pt.camera_new(width=8, height=8)
    prm = pt.default_params(spp=2)
    dn, tp, g = pt.default_denoise(), pt.default_temporal(), pt.default_gradient()
    buf = (C.c_float * 2048)()
    base = C.addressof(buf)
    base += (-base) % 16
    ok, odd4, odd16 = C.c_void_p(base), C.c_void_p(base + 2), C.c_void_p(base + 4)
    out = C.c_void_p(base + 2048)
    fake = C.c_void_p(base + 4096)                              # a context-shaped pointer that is never followed
    R = lambda p: C.byref(p)  # noqa: E731
    grad = lib.pt_temporal_gradient_camera_device
    who = b"pt_temporal_gradient_camera_device"
    good = (R(cam), R(cam), R(prm), 0, ok, ok, R(g), 0.2, out)
    assert grad(None, *good) == 1 and who in lib.pt_last_error() and b"null context" in lib.pt_last_error()
    for k in (0, 1, 2, 4, 5, 6, 8):                            # every pointer, prev_cam and d_features among them
        args = list(good)
        args[k] = None
        assert grad(fake, *args) == 1, k
        assert who in lib.pt_last_error() and b"null argument" in lib.pt_last_error(), k
    for k, word in ((4, b"4-byte"), (8, b"4-byte"), (5, b"d_features")):
        args = list(good)
        args[k] = odd4
        assert grad(fake, *args) == 1 and word in lib.pt_last_error() and b"aligned" in lib.pt_last_error(), k
    args = list(good)
    args[5] = odd16                                             # 4-byte aligned is not enough for the feature records
    assert grad(fake, *args) == 1 and b"d_features must be 16-byte aligned" in lib.pt_last_error()
    for w, h in ((9, 8), (8, 7), (4, 4)):
        other = pt.camera_new(width=w, height=h)
        assert grad(fake, R(cam), R(other), R(prm), 0, ok, ok, R(g), 0.2, out) == 1 and b"previous camera is" in lib.pt_last_error()
        assert grad(fake, R(other), R(cam), R(prm), 0, ok, ok, R(g), 0.2, out) == 1 and b"previous camera is" in lib.pt_last_error()
    # the checks of pt_temporal_gradient_device
    banded = pt.default_params(spp=2, band_rows=2, band_count=2)
    assert grad(fake, R(cam), R(cam), R(banded), 0, ok, ok, R(g), 0.2, out) == 1 and b"band_count" in lib.pt_last_error()
    assert grad(fake, R(cam), R(cam), R(prm), 0, ok, ok, R(pt.default_gradient(radius=9)), 0.2, out) == 1 and b"radius" in lib.pt_last_error()
    assert grad(fake, R(cam), R(cam), R(prm), 0, ok, ok, R(pt.default_gradient(scale=-1.0)), 0.2, out) == 1 and b"scale" in lib.pt_last_error()
    assert grad(fake, R(cam), R(cam), R(prm), 0, ok, ok, R(g), 1.5, out) == 1 and b"alpha_min" in lib.pt_last_error()
    small = pt._lib.PtCamera.from_buffer_copy(cam)
    small.width = 1
    assert grad(fake, R(small), R(small), R(prm), 0, ok, ok, R(g), 0.2, out) == 1 and b">= 2" in lib.pt_last_error()
    # the one call
    one = lib.pt_render_denoised_gradient_camera
    who = b"pt_render_denoised_gradient_camera"
    assert one(None, R(cam), R(prm), 2, R(dn), R(tp), R(g), buf, None, None, None, None, None) == 1 and b"null" in lib.pt_last_error()
    for args in ((None, R(prm), 2, R(dn), R(tp), R(g), buf), (R(cam), None, 2, R(dn), R(tp), R(g), buf), (R(cam), R(prm), 2, None, R(tp), R(g), buf),
                 (R(cam), R(prm), 2, R(dn), None, R(g), buf), (R(cam), R(prm), 2, R(dn), R(tp), None, buf), (R(cam), R(prm), 2, R(dn), R(tp), R(g), None)):
        assert one(fake, *args, None, None, None, None, None) == 1 and who in lib.pt_last_error() and b"null" in lib.pt_last_error()
    assert one(fake, R(cam), R(prm), 0, R(dn), R(tp), R(g), buf, None, None, None, None, None) == 1 and b"feature_samples" in lib.pt_last_error()
    assert one(fake, R(cam), R(banded), 2, R(dn), R(tp), R(g), buf, None, None, None, None, None) == 1 and b"band_count" in lib.pt_last_error()
    assert one(fake, R(cam), R(prm), 2, R(dn), R(tp), R(pt.default_gradient(radius=9)), buf, None, None, None, None, None) == 1
    assert who in lib.pt_last_error() and b"radius" in lib.pt_last_error()


# ---------------------------------------------------------------- the helper of pt_gradient.h
@pytest.fixture(scope="module")
def rule(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("gcrule")
    (d / "rule.cpp").write_text(SRC)
    so = d / "rule.so"
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-I",
                           os.path.join(ROOT, "pathtrace_amd", "csrc"), str(d / "rule.cpp"), "-o", str(so)])
    lib = C.CDLL(str(so))
    lib.gc_lookup.argtypes = [C.c_void_p, C.c_void_p, C.c_uint, C.c_uint, C.c_uint, C.c_void_p]
    lib.gc_plane.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint, C.c_uint, C.c_uint, C.c_float, C.c_float, C.c_void_p]
    return lib


def _grid(w, h):
    """(x', y') around and across the image: exact halves and integers, their neighbours in f64, negatives, values >= W,
    huge values, infinities and NaN."""
    def axis(n):
        v = [-1e300, -3.0, -1.5, -1.0, -0.75, -0.5, -0.25, -0.0, 0.0, 0.25, 0.5, 1.0, 1.49999, 1.5, 2.5, n - 1.5, n - 1.0, n - 0.75, n - 0.5,
             n - 0.25, float(n), n + 0.5, n + 3.0, 2.0 ** 31, 2.0 ** 32 + 0.5, 1e300, np.inf, -np.inf, np.nan]
        v += [np.nextafter(-0.5, -1.0), np.nextafter(-0.5, 1.0), np.nextafter(n - 0.5, -1.0), np.nextafter(n - 0.5, n), np.nextafter(0.5, 0.0)]
        v += [k + 0.5 for k in range(n)] + [float(k) for k in range(n)]
        return np.array(v, np.float64)
    xr, yr = np.meshgrid(axis(w), axis(h))
    return np.ascontiguousarray(xr.ravel()), np.ascontiguousarray(yr.ravel())


def test_lookup_pixel_against_the_restatement(rule):
    for w, h in SIZES:
        xr, yr = _grid(w, h)
        out = np.zeros((xr.size, 3), np.int32)
        rule.gc_lookup(xr.ctypes.data, yr.ctypes.data, xr.size, w, h, out.ctypes.data)
        xi, yi, inside = gc.lookup_pixel(xr, yr, w, h)
        assert np.array_equal(out[:, 0] == 1, inside), (w, h)
        assert inside.any() and (~inside).any()
        assert np.array_equal(out[inside, 1], xi[inside]) and np.array_equal(out[inside, 2], yi[inside]), (w, h)
        assert (out[~inside, 1] == 77777).all() and (out[~inside, 2] == 88888).all()      # a refused lookup writes nothing
        assert (out[inside, 1] < w).all() and (out[inside, 2] < h).all() and (out[inside, 1:] >= 0).all()
    # the rounding: halves go up, the image is [-0.5, W - 0.5) x [-0.5, H - 0.5)
    for x, want in ((-0.5, 0), (0.49999, 0), (0.5, 1), (1.5, 2), (45.5, 46), (46.49, 46), (46.5, None), (-0.50001, None), (47.0, None)):
        xi, _, inside = gc.lookup_pixel(x, 3.0, 47, 31)
        assert (int(xi) if inside else None) == want, x


def test_the_plane_through_the_helper_against_the_restatement(rule):
    """pixel_alpha behind lookup_pixel, as k_gradient_alpha_camera composes them, against gathering the previous image's plane."""
    rng = np.random.default_rng(51)
    for w, h in SIZES:
        sw, sh = gr.strata_shape(w, h)
        old = rng.exponential(0.5, (sh, sw, 3)).astype(np.float32)
        new = np.where(rng.random((sh, sw, 1)) < 0.5, old, rng.exponential(0.5, (sh, sw, 3)).astype(np.float32))
        rec = np.ascontiguousarray(gr.records(new, old))
        xr = np.ascontiguousarray(rng.uniform(-2.0, w + 1.0, (h, w)))
        yr = np.ascontiguousarray(rng.uniform(-2.0, h + 1.0, (h, w)))
        xr[0, 0], yr[0, 0] = -0.5, -0.5                          # the corner pixel, on the rounding's edge
        xr[-1, -1], yr[-1, -1] = np.nextafter(w - 0.5, 0.0), np.nextafter(h - 0.5, 0.0)
        for radius, scale, amin in ((1, 1.0, 0.2), (0, 2.5, 0.0), (8, 1.0, 0.2)):
            got = np.zeros((h, w), np.float32)
            rule.gc_plane(rec.ctypes.data, xr.ctypes.data, yr.ctypes.data, w, h, radius, scale, amin, got.ctypes.data)
            xi, yi, inside = gc.lookup_pixel(xr, yr, w, h)
            want = np.where(inside, gr.alpha_plane(rec, w, h, radius, scale, amin)[yi, xi], np.float32(np.nan)).astype(np.float32)
            assert np.array_equal(np.isnan(got), ~inside) and inside[0, 0] and inside[-1, -1]
            assert np.array_equal(got[inside].view(np.uint32), want[inside].view(np.uint32)), (w, h, radius)


# ---------------------------------------------------------------- the restatement
def test_a_wall_under_a_camera_moved_sideways_lands_in_the_predicted_stratum(pt):
    """A wall z = -1 facing the camera, the previous camera 4.3 pixel footprints (at the wall) to the right: the wall point of
    pixel (x, y) lay at x' = x - 4.3 in the previous image, so xi = x - 4, yi = y, and columns 0-3 have no measurement."""
    w, h = gc.W, gc.H
    cam = pt.camera_new(width=w, height=h)
    o, l, hz = np.array(cam.origin), np.array(cam.lower_left), np.array(cam.horizontal)
    assert hz[1] == 0 and hz[2] == 0 and hz[0] > 0               # the image plane is z = const, x to the right
    k = (-1.0 - o[2]) / (l[2] - o[2])                            # wall distance over screen distance
    e = 4.3 * k * hz[0] / (w - 1)
    prev = pt.camera_new(origin=(o[0] + e, o[1], o[2]), width=w, height=h)
    feat = tr.wall_features(cam, -1.0).astype(np.float32)
    xi, yi, ok, band = gc.lookup(cam, prev, feat[..., 7])
    ys, xs = np.mgrid[0:h, 0:w]
    assert not band.any()
    assert np.array_equal(ok, xs >= 4)
    assert np.array_equal(xi[ok], (xs - 4)[ok]) and np.array_equal(yi[ok], ys[ok])
    # radius 0: the weight of a pixel is its one stratum's, ((x - 4) / 3, y / 3)
    rng = np.random.default_rng(52)
    sw, sh = gr.strata_shape(w, h)
    rec = np.stack([rng.uniform(0.0, 1.0, (sh, sw)), rng.uniform(1.0, 2.0, (sh, sw))], -1)
    plane, _ = gc.alpha_plane(rec, cam, prev, feat[..., 7], radius=0, scale=1.0, alpha_min=0.2)
    a = np.float64(np.float32(0.2))
    q = rec[ys // 3, np.maximum(xs - 4, 0) // 3]
    want = (a + q[..., 0] / q[..., 1] * (1.0 - a)).astype(np.float32)
    assert np.isnan(plane[:, :4]).all() and np.array_equal(plane[:, 4:], want[:, 4:])
    assert len(np.unique(plane[:, 4:])) == sh * len(np.unique((np.arange(4, w) - 4) // 3))
    # a pixel without depth has no measurement; equal cameras look every pixel up in place, misses included
    feat[3, 10, 7] = 0.0
    assert not gc.lookup(cam, prev, feat[..., 7])[2][3, 10]
    xi, yi, ok, band = gc.lookup(cam, pt.camera_new(width=w, height=h), feat[..., 7])
    assert ok.all() and not band.any() and np.array_equal(xi, xs) and np.array_equal(yi, ys)
    same, _ = gc.alpha_plane(rec, cam, cam, feat[..., 7], radius=1)
    assert np.array_equal(same, gr.alpha_plane(rec, w, h, 1))


@pytest.mark.parametrize("scene", [1, 2, 4])
def test_the_camera_moves_of_the_gpu_tests_stay_clear_of_the_band(pt, orc, scene):
    """On the oracle's features: at most 1 % of the pixels within 1e-6 of a flip, at least half with a measurement -- in the
    two closed boxes; the 300 small spheres of scene 4 cover a few percent of the view, the rest has no depth."""
    objs = pt.builtin_scene(4, 300) if scene == 4 else pt.builtin_scene(scene)
    pairs = [gc.cameras(pt)] + [(gc.orbit(pt, k, gc.W, gc.H), gc.orbit(pt, k + 1, gc.W, gc.H)) for k in (0, 3)]
    for prev, cur in pairs:
        assert not gc.same_camera(cur, prev)
        feat = dr.features_f32(orc, objs, cur, 0, 1)
        xi, yi, ok, band = gc.lookup(cur, prev, feat[..., 7])
        assert band.mean() <= gc.BAND_CAP
        assert ok.mean() >= 0.5 if scene != 4 else ok.any(), (scene, ok.mean())
