"""The thin-lens camera (pt_render_lens_device) without a GPU: the refusals through the C ABI with a null context,
the pinned defaults, the host side of the rule (pt_debug_lens_setup) against the numpy restatement (tests/lens_ref.py), the
restatement's Philox words against the project's generator, and the rule header under the sanitizers."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import lens_ref as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = [C.c_void_p(0x1000 * k) for k in range(1, 6)]      # aligned, distinct addresses no check may read
AXIS = dict(origin=(0.1, -0.2, 2.5), width=37, height=23, screen_distance=1.3, fov_degrees=41.0)
LOOK = ((1.0, 0.7, 2.0), (0.0, -0.1, -2.0), (0.1, 1.0, 0.0), 37, 23, 33.0)


def _refused(pt, rc, part):
    assert rc == 1, rc                                            # PT_ERR_INVALID_ARG
    msg = pt._lib.lib().pt_last_error().decode()
    assert part in msg, msg


def test_default_lens_is_a_pinhole(pt):
    l = pt.default_lens()
    assert (l.aperture, l.focus_distance) == (0.0, 1.0)
    assert C.sizeof(pt._lib.PtLens) == 16
    assert pt.default_lens(aperture=0.25).aperture == 0.25
    pt._lib.lib().pt_default_lens(None)                           # a null pointer is ignored


def test_every_entry_refuses_a_null_context_and_null_arguments(pt):
    L = pt._lib.lib()
    cam, lens, prm, dn = pt.camera_new(width=8, height=8), pt.default_lens(aperture=0.1), pt.default_params(spp=2), pt.default_denoise()
    cb, lb, pb, db = C.byref(cam), C.byref(lens), C.byref(prm), C.byref(dn)
    xys = (C.c_uint32 * 3)(1, 2, 3)
    out8 = (C.c_float * 8)()
    _refused(pt, L.pt_render_lens_device(None, cb, lb, pb, FAKE[0], FAKE[1]), "pt_render_lens_device: null argument")
    _refused(pt, L.pt_render_lens_host(None, cb, lb, pb, FAKE[0], FAKE[1]), "pt_render_lens_host: null argument")
    _refused(pt, L.pt_render_features_lens_device(None, cb, lb, pb, 2, FAKE[0]), "pt_render_features_lens_device: null argument")
    _refused(pt, L.pt_render_features_lens_device(None, cb, None, pb, 2, FAKE[0]), "pt_render_features_lens_device: null argument")
    _refused(pt, L.pt_render_lens_denoised(None, cb, lb, pb, 2, db, FAKE[0], None, None, None), "pt_render_lens_denoised: null argument")
    _refused(pt, L.pt_render_lens_denoised(None, cb, None, pb, 2, db, FAKE[0], None, None, None), "pt_render_lens_denoised: null argument")
    _refused(pt, L.pt_debug_lens_rays(None, cb, lb, xys, 1, 0, out8), "pt_debug_lens_rays: null argument")
    out7 = (C.c_float * 7)()
    for args in ((None, lb, out7), (cb, None, out7), (cb, lb, None)):
        _refused(pt, L.pt_debug_lens_setup(*args), "pt_debug_lens_setup: null argument")


def test_setup_refuses_bad_lenses_and_degenerate_cameras(pt):
    L = pt._lib.lib()
    cam = pt.camera_new(**AXIS)
    out7 = (C.c_float * 7)(*([7.0] * 7))

    def call(cam=cam, **kw):
        return L.pt_debug_lens_setup(C.byref(cam), C.byref(pt.default_lens(**kw)), out7)

    for a in (-1.0, -1e-300, math.inf, -math.inf, math.nan):
        _refused(pt, call(aperture=a), "aperture")
    for f in (0.0, -2.0, math.inf, -math.inf, math.nan):
        _refused(pt, call(aperture=0.3, focus_distance=f), "focus_distance")
    for field, value in (("horizontal", (0.0, 0.0, 0.0)), ("vertical", (0.0, 0.0, 0.0)), ("horizontal", (math.nan, 0.0, 0.0)),
                         ("vertical", (math.inf, 0.0, 0.0)), ("origin", (math.nan, 0.0, 0.0))):
        bad = pt._lib.PtCamera.from_buffer_copy(cam)
        for k in range(3):
            getattr(bad, field)[k] = value[k]
        _refused(pt, call(cam=bad, aperture=0.3), "degenerate camera")
    centre = pt._lib.PtCamera.from_buffer_copy(cam)               # D = 0: the screen's centre is the origin
    for k, (o, h, v) in enumerate(((1.0, 2.0, 0.0), (2.0, 0.0, 1.0), (3.0, 0.0, 0.0))):      # values whose halves and sums are exact
        centre.origin[k], centre.horizontal[k], centre.vertical[k], centre.lower_left[k] = o, h, v, o - h / 2 - v / 2
    _refused(pt, call(cam=centre, aperture=0.3), "degenerate camera")
    assert list(out7) == [7.0] * 7                                # a refusal writes nothing
    assert call(aperture=0.3, focus_distance=2.0) == 0


@pytest.mark.parametrize("kind", ["axis", "look_at"])
def test_setup_against_the_restatement(pt, kind):
    cam = pt.camera_new(**AXIS) if kind == "axis" else pt.camera_look_at(*LOOK)
    assert cam.width != cam.height
    for aperture, focus in ((0.3, 2.0), (0.05, 0.7), (2.5, 40.0)):
        got = pt.lens_setup(cam, pt.default_lens(aperture=aperture, focus_distance=focus))
        ref = lr.setup(cam, aperture, focus)
        # f64 on both sides, rounded to f32 once: at most the last bit of a differently ordered f64 expression away
        assert np.all(np.abs(got.astype(np.float64) - ref.astype(np.float64)) <= lr.ulp32(np.maximum(np.abs(ref.astype(np.float64)), 1e-30))), (got, ref)
        lu, lv = got[0:3].astype(np.float64), got[3:6].astype(np.float64)
        assert abs(np.linalg.norm(lu) - aperture / 2) <= 1e-6 * aperture and abs(np.linalg.norm(lv) - aperture / 2) <= 1e-6 * aperture
        assert abs(lu @ lv) <= 1e-6 * aperture * aperture         # the screen's axes are orthogonal
        if kind == "axis":                                        # the screen of camera_new: x and y axes, D = screen_distance
            assert lu[1] == 0 and lu[2] == 0 and lv[0] == 0 and lv[2] == 0 and lu[0] > 0 and lv[1] > 0
            assert abs(got[6] - 1.3 / focus) <= 2e-7 * 1.3 / focus


@pytest.mark.parametrize("kind", ["axis", "look_at"])
def test_aperture_zero_gives_exact_zeros(pt, kind):
    cam = pt.camera_new(**AXIS) if kind == "axis" else pt.camera_look_at(*LOOK)
    got = pt.lens_setup(cam, pt.default_lens(focus_distance=3.0))
    assert np.array_equal(got[:6].view(np.uint32) & 0x7FFFFFFF, np.zeros(6, dtype=np.uint32))
    assert got[6] > 0


def test_restatement_draws_the_generators_words(orc):
    rng = np.random.default_rng(7)
    ctr = rng.integers(0, 2 ** 32, size=(200, 3), dtype=np.uint64)
    ctr[0] = (0, 0, 0)
    ctr[1] = (36, 22, 2 ** 32 - 1)
    w = lr.words(ctr[:, 0], ctr[:, 1], ctr[:, 2])
    for c, got in zip(ctr, w):
        assert [int(v) for v in got] == orc.philox([int(c[0]), int(c[1]), int(c[2]), lr.DEPTH_CAMERA], [lr.BLK_SURFACE, 0])
    assert lr.u01(0) == orc.u01(0) and lr.u01(0xFFFFFFFF) == orc.u01(0xFFFFFFFF) and lr.u01(0x12345678) == orc.u01(0x12345678)


def test_restatement_maps_the_square_onto_the_disc():
    """Shirley's map: the square's edge midpoints and corners land on the unit circle's axes and diagonals, the disc is covered
    evenly (area-preserving), and every lens ray of a sample passes its focus point."""
    top = 0xFFFFFFFF
    mid = 0x80000000
    dx, dy = lr.disc(np.array([top, mid, 0, mid, top]), np.array([mid, top, mid, 0, top]))
    e = 2.0 ** -22
    assert np.allclose(dx, [1, 0, -1, 0, math.sqrt(0.5)], atol=e) and np.allclose(dy, [0, 1, 0, -1, math.sqrt(0.5)], atol=e)
    rng = np.random.default_rng(3)
    w = rng.integers(0, 2 ** 32, size=(200000, 2), dtype=np.uint64)
    dx, dy = lr.disc(w[:, 0], w[:, 1])
    r2 = dx * dx + dy * dy
    assert r2.max() <= 1.0
    assert abs((r2 <= 0.25).mean() - 0.25) < 0.005 and abs((dx > 0).mean() - 0.5) < 0.005 and abs((dy > 0).mean() - 0.5) < 0.005


def test_rule_header_is_clean_under_asan_and_ubsan(tmp_path):
    """tests/tools/lens_san.cpp: a stand-alone program around the host functions of pt_lens.h"""
    exe = str(tmp_path / "lens_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "tools", "lens_san.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "lens_san: 0 failed checks" in out, out[-3000:]
    assert "runtime error" not in out and "AddressSanitizer" not in out, out[-3000:]
