"""The projections (pt_render_projection_device and friends) without a GPU: the rule on the CPU
(pt_projection_rays_host, pathtrace_amd/csrc/pt_projection.h in exact arithmetic) against the numpy restatement
(tests/projection_ref.py), the geometric identities of every kind, the refusals through the C ABI, the cap on borderline samples
of the GPU coverage test's inputs, and the rule header under the sanitizers."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import lens_ref as lr
import projection_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = [C.c_void_p(0x1000 * k) for k in range(1, 6)]      # aligned, distinct addresses no check may read
FOVS = {pr.PERSPECTIVE: 180.0, pr.ORTHOGRAPHIC: 180.0, pr.FISHEYE: 200.0, pr.EQUIRECT: 180.0}


def _xys(seed):
    rng = np.random.default_rng(seed)
    n = 4096 + 4
    xys = np.stack([rng.integers(0, 37, n), rng.integers(0, 23, n), rng.integers(0, 2 ** 32, n)], axis=1).astype(np.uint32)
    xys[:4] = [(0, 0, 0), (36, 22, 2 ** 32 - 1), (36, 0, 1), (0, 22, 7)]      # the four corners
    return xys


def _refused(pt, rc, part):
    assert rc == 1, rc                                            # PT_ERR_INVALID_ARG
    msg = pt._lib.lib().pt_last_error().decode()
    assert msg and part in msg, msg


def test_default_projection_is_the_pinhole(pt):
    p = pt.default_projection()
    assert (p.kind, p.reserved, p.fov_degrees) == (0, 0, 180.0)
    assert C.sizeof(pt._lib.PtProjection) == 16
    assert pt.default_projection(kind="fisheye", fov_degrees=220.0).kind == 2
    assert pt.default_projection(kind=3).kind == 3
    pt._lib.lib().pt_default_projection(None)                     # a null pointer is ignored
    assert pt._lib.lib().pt_abi_version() == 6


# ---------------------------------------------------------------- 1. the host rule against the restatement
@pytest.mark.parametrize("kind", pr.KINDS)
def test_host_rays_against_the_restatement(pt, kind):
    cam = pt.camera_look_at(*pr.LOOK)
    proj = pt.default_projection(kind=kind, fov_degrees=FOVS[kind])
    xys = _xys(11 + kind)
    got = pt.projection_rays_host(cam, proj, xys).astype(np.float64)
    ref = pr.rays(cam, kind, FOVS[kind], xys)
    o, d = got[:, 0:3], got[:, 3:6]
    bound = pr.bound(cam, kind, o)
    err_o, err_d = np.abs(o - ref["o"]).max(), np.abs(d - ref["d"]).max()
    err_ab = max(np.abs(got[:, 6] - ref["a"]).max(), np.abs(got[:, 7] - ref["b"]).max())
    print(f"kind {kind}: |o - ref| {err_o:.2e}, |d - ref| {err_d:.2e}, |(a, b) - ref| {err_ab:.2e}, bound {bound:.2e}")
    assert err_o <= bound and err_d <= bound and err_ab <= bound
    # the setup: f64 on both sides, rounded to f32 once
    s, sref = pt.projection_setup(cam, proj).astype(np.float64), pr.setup(cam, kind, FOVS[kind]).astype(np.float64)
    assert np.all(np.abs(s - sref) <= lr.ulp32(np.maximum(np.abs(sref), 1e-30))), (s, sref)


# ---------------------------------------------------------------- 2. geometric identities
@pytest.mark.parametrize("kind", pr.KINDS)
def test_directions_are_unit_vectors(pt, kind):
    cam = pt.camera_look_at(*pr.LOOK)
    got = pt.projection_rays_host(cam, pt.default_projection(kind=kind, fov_degrees=FOVS[kind]), _xys(21)).astype(np.float64)
    assert np.abs(np.linalg.norm(got[:, 3:6], axis=1) - 1.0).max() <= 4 * 2.0 ** -23


def test_orthographic_rays_are_parallel_and_start_on_the_camera_plane(pt):
    cam = pt.camera_look_at(*pr.LOOK)
    proj = pt.default_projection(kind="orthographic")
    xys = _xys(22)
    got = pt.projection_rays_host(cam, proj, xys)
    wv = pt.projection_setup(cam, proj)[6:9]
    assert np.array_equal(got[:, 3:6].view(np.uint32), np.broadcast_to(wv, (len(xys), 3)).view(np.uint32))      # bitwise Wv
    f = pr.frame(cam)
    o = got[:, 0:3].astype(np.float64)
    off = (o - f["origin"]) @ f["W"]
    assert np.abs(off).max() <= pr.bound(cam, pr.ORTHOGRAPHIC, o)
    # the window: |horizontal| x |vertical|, the sample's position in it
    assert np.abs((o - f["origin"]) @ f["U"] - got[:, 6] / 2 * f["nh"]).max() <= pr.bound(cam, pr.ORTHOGRAPHIC, o)
    assert np.abs((o - f["origin"]) @ f["V"] - got[:, 7] / 2 * f["nv"]).max() <= pr.bound(cam, pr.ORTHOGRAPHIC, o)


@pytest.mark.parametrize("fov", [200.0, 360.0, 90.0])
def test_fisheye_angle_is_the_radius_times_half_the_field(pt, fov):
    cam = pt.camera_look_at(*pr.LOOK)
    got = pt.projection_rays_host(cam, pt.default_projection(kind="fisheye", fov_degrees=fov), _xys(23)).astype(np.float64)
    f = pr.frame(cam)
    rho = np.hypot(got[:, 6], got[:, 7] * f["aspect"])
    want = np.minimum(rho * math.radians(fov) / 2, math.pi)
    d = got[:, 3:6]
    # the angle from both of its well-conditioned forms: atan2(|d x W|, d . W)
    angle = np.arctan2(np.linalg.norm(np.cross(d, f["W"]), axis=1), d @ f["W"])
    assert np.abs(angle - want).max() <= pr.bound(cam, pr.FISHEYE)
    if fov == 360.0:
        assert (want == math.pi).any() and (want < 0.2).any()      # the cap is reached, and so is the centre


def test_equirect_centre_looks_along_the_axis_and_column_zero_backwards(pt):
    cam = pt.camera_look_at(*pr.LOOK)                              # 37 x 23: pixel (18, 11) with jitter 0 is the centre
    f = pr.frame(cam)
    b = pr.bound(cam, pr.EQUIRECT)
    one = np.array([[18, 11, 0]])
    centre = pr.rays(cam, pr.EQUIRECT, 180.0, one, jitter=(np.array([0.0]), np.array([0.0])))
    assert np.abs(centre["d"][0] - f["W"]).max() <= 1e-15
    xys = _xys(24)
    got = pt.projection_rays_host(cam, pt.default_projection(kind="equirect"), xys).astype(np.float64)
    d, a, bb = got[:, 3:6], got[:, 6], got[:, 7]
    # longitude and latitude of every ray, from the ray itself
    assert np.abs(d @ f["V"] - np.sin(np.pi * bb / 2)).max() <= b
    assert np.abs(d @ f["W"] - np.cos(np.pi * bb / 2) * np.cos(np.pi * a)).max() <= b
    assert np.abs(d @ f["U"] - np.cos(np.pi * bb / 2) * np.sin(np.pi * a)).max() <= b
    # the samples of the centre pixel look along Wv to within the pixel, those of column 0 along -Wv on the left
    pix = 2 * np.pi / 36
    more = np.array([[18, 11, s] for s in range(16)] + [[0, 11, s] for s in range(16)], dtype=np.uint32)
    g2 = pt.projection_rays_host(cam, pt.default_projection(kind="equirect"), more).astype(np.float64)
    assert np.all(g2[:16, 3:6] @ f["W"] >= math.cos(pix * 1.5))
    assert np.all(g2[16:, 3:6] @ f["W"] <= -math.cos(pix * 1.5)) and np.all(g2[16:, 3:6] @ f["U"] <= 0)


# ---------------------------------------------------------------- 3. PERSPECTIVE is the pinhole
def test_perspective_host_rays_are_the_pinhole(pt):
    cam = pt.camera_look_at(*pr.LOOK)
    xys = _xys(31)
    got = pt.projection_rays_host(cam, pt.default_projection(), xys).astype(np.float64)
    assert np.abs(got[:, 3:6] - pr.pinhole(cam, xys)).max() <= pr.bound(cam, pr.PERSPECTIVE)
    assert np.array_equal(got[:, 0:3], np.broadcast_to(np.array(lr.cam_fields(cam, f32=True)[0]), (len(xys), 3)))


# ---------------------------------------------------------------- 4. refusals
def test_setup_refuses_bad_projections_and_degenerate_cameras(pt):
    L = pt._lib.lib()
    cam = pt.camera_look_at(*pr.LOOK)
    out11 = (C.c_float * 11)(*([7.0] * 11))
    xys = (C.c_uint32 * 3)(1, 2, 3)
    out8 = (C.c_float * 8)(*([7.0] * 8))

    def both(part, cam=cam, **kw):
        p = pt.default_projection(**kw)
        _refused(pt, L.pt_projection_setup_host(C.byref(cam), C.byref(p), out11), part)
        _refused(pt, L.pt_projection_rays_host(C.byref(cam), C.byref(p), xys, 1, out8), part)

    for kind in (4, 17, 2 ** 32 - 1):
        both("unknown projection kind", kind=kind)
    for kind in pr.KINDS:
        both("reserved", kind=kind, reserved=1)
    for fov in (0.0, -1.0, 360.0001, math.inf, -math.inf, math.nan):
        both("fov_degrees", kind=pr.FISHEYE, fov_degrees=fov)
    for field, value in (("horizontal", (0.0, 0.0, 0.0)), ("vertical", (0.0, 0.0, 0.0)), ("horizontal", (math.nan, 0.0, 0.0)),
                         ("vertical", (math.inf, 0.0, 0.0)), ("origin", (math.nan, 0.0, 0.0))):
        bad = pt._lib.PtCamera.from_buffer_copy(cam)
        for k in range(3):
            getattr(bad, field)[k] = value[k]
        for kind in pr.KINDS:
            both("degenerate camera", cam=bad, kind=kind)
    centre = pt._lib.PtCamera.from_buffer_copy(cam)               # |C| = 0: the screen's centre is the origin
    for k, (o, h, v) in enumerate(((1.0, 2.0, 0.0), (2.0, 0.0, 1.0), (3.0, 0.0, 0.0))):      # values whose halves and sums are exact
        centre.origin[k], centre.horizontal[k], centre.vertical[k], centre.lower_left[k] = o, h, v, o - h / 2 - v / 2
    both("degenerate camera", cam=centre, kind=pr.EQUIRECT)
    assert list(out11) == [7.0] * 11 and list(out8) == [7.0] * 8  # a refusal writes nothing
    # a fov outside the range is nobody's business but the fisheye's; 360 itself is allowed
    for kind in (pr.PERSPECTIVE, pr.ORTHOGRAPHIC, pr.EQUIRECT):
        assert L.pt_projection_setup_host(C.byref(cam), C.byref(pt.default_projection(kind=kind, fov_degrees=-5.0)), out11) == 0
    assert L.pt_projection_setup_host(C.byref(cam), C.byref(pt.default_projection(kind=pr.FISHEYE, fov_degrees=360.0)), out11) == 0


def test_every_entry_refuses_null_arguments_and_bad_projections_before_the_context(pt):
    L = pt._lib.lib()
    cam, proj, prm, dn = pt.camera_new(width=8, height=8), pt.default_projection(kind=3), pt.default_params(spp=2), pt.default_denoise()
    cb, pb, mb, db = C.byref(cam), C.byref(proj), C.byref(prm), C.byref(dn)
    xys = (C.c_uint32 * 3)(1, 2, 3)
    out8 = (C.c_float * 8)()
    _refused(pt, L.pt_render_projection_device(None, cb, pb, mb, FAKE[0], FAKE[1]), "pt_render_projection_device: null argument")
    _refused(pt, L.pt_render_projection_device(FAKE[2], cb, None, mb, FAKE[0], FAKE[1]), "pt_render_projection_device: null argument")
    _refused(pt, L.pt_render_projection_host(None, cb, pb, mb, FAKE[0], FAKE[1]), "pt_render_projection_host: null argument")
    _refused(pt, L.pt_render_features_projection_device(None, cb, pb, mb, 2, FAKE[0]), "pt_render_features_projection_device: null argument")
    _refused(pt, L.pt_render_features_projection_device(None, cb, None, mb, 2, FAKE[0]), "pt_render_features_projection_device: null argument")
    _refused(pt, L.pt_render_projection_denoised(None, cb, pb, mb, 2, db, FAKE[0], None, None, None), "pt_render_projection_denoised: null argument")
    _refused(pt, L.pt_render_projection_denoised(None, cb, None, mb, 2, db, FAKE[0], None, None, None), "pt_render_projection_denoised: null argument")
    _refused(pt, L.pt_debug_projection_rays(None, cb, pb, xys, 1, 0, out8), "pt_debug_projection_rays: null argument")
    _refused(pt, L.pt_render_rays_device(None, 8, 8, mb, FAKE[0], None, FAKE[1], FAKE[2]), "pt_render_rays_device: null argument")
    _refused(pt, L.pt_render_rays_device(FAKE[3], 8, 8, mb, None, None, FAKE[1], FAKE[2]), "pt_render_rays_device: null argument")
    _refused(pt, L.pt_render_rays_device(FAKE[3], 8, 8, None, FAKE[0], None, FAKE[1], FAKE[2]), "pt_render_rays_device: null argument")
    _refused(pt, L.pt_render_rays_device(FAKE[3], 8, 8, mb, C.c_void_p(0x1004), None, FAKE[1], FAKE[2]), "8-byte aligned")
    _refused(pt, L.pt_render_rays_device(FAKE[3], 8, 8, mb, FAKE[0], C.c_void_p(0x2002), FAKE[1], FAKE[2]), "4-byte aligned")
    out11 = (C.c_float * 11)()
    for args in ((None, pb, out11), (cb, None, out11), (cb, pb, None)):
        _refused(pt, L.pt_projection_setup_host(*args), "pt_projection_setup_host: null argument")
    for args in ((None, pb, xys, 1, out8), (cb, None, xys, 1, out8), (cb, pb, None, 1, out8), (cb, pb, xys, 1, None)):
        _refused(pt, L.pt_projection_rays_host(*args), "pt_projection_rays_host: null argument")
    # a bad projection is refused before the context is looked at (the address is nobody's)
    bad = C.byref(pt.default_projection(kind=9))
    _refused(pt, L.pt_render_projection_device(FAKE[2], cb, bad, mb, FAKE[0], FAKE[1]), "unknown projection kind")
    _refused(pt, L.pt_render_projection_host(FAKE[2], cb, bad, mb, FAKE[0], FAKE[1]), "unknown projection kind")
    _refused(pt, L.pt_render_features_projection_device(FAKE[2], cb, bad, mb, 2, FAKE[0]), "unknown projection kind")
    _refused(pt, L.pt_render_projection_denoised(FAKE[2], cb, bad, mb, 2, db, FAKE[0], None, None, None), "unknown projection kind")
    _refused(pt, L.pt_debug_projection_rays(FAKE[2], cb, bad, xys, 1, 0, out8), "unknown projection kind")


# ---------------------------------------------------------------- 5. the coverage inputs: the cap hides nothing
@pytest.mark.parametrize("kind,fov,sphere", [(pr.EQUIRECT, 180.0, pr.COV_BEHIND), (pr.FISHEYE, 360.0, pr.COV_BEHIND),
                                             (pr.ORTHOGRAPHIC, 180.0, pr.COV_FRONT)])
def test_coverage_inputs_have_few_borderline_samples(pt, kind, fov, sphere):
    cam = pt.camera_look_at(*pr.COV_LOOK)
    ref = pr.rays(cam, kind, fov, pr.coverage_xys())
    sure, amb = pr.coverage(ref["o"], ref["d"], sphere)
    seen = (sure + amb) > 0
    print(f"kind {kind}: {int(seen.sum())} pixels see the sphere, {int((amb > 0).sum())} hold a borderline sample, {int(sure.sum())} sure hits")
    assert seen.sum() >= 12                                       # the sphere is in the picture
    assert (amb > 0).sum() <= pr.COV_CAP * seen.sum()
    assert (~seen).sum() >= 12                                    # and does not fill it
    if kind != pr.ORTHOGRAPHIC:                                   # behind the camera: the pinhole sees none of it
        pin = pr.rays(cam, pr.PERSPECTIVE, 180.0, pr.coverage_xys())
        oc = np.asarray(sphere[0]) - pin["o"]                     # the centre lies behind every pinhole ray, the origin outside
        assert np.all((oc * pin["d"]).sum(axis=1) < 0) and np.all(np.linalg.norm(oc, axis=1) > sphere[1])
        assert pr.coverage(pin["o"], pin["d"], sphere)[0].sum() == 0


# ---------------------------------------------------------------- 6. the rule header under the sanitizers
def test_rule_header_is_clean_under_asan_and_ubsan(tmp_path):
    """tests/tools/projection_san.cpp: a stand-alone program around pt_projection.h"""
    exe = str(tmp_path / "projection_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "tools", "projection_san.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "projection_san: 0 failed checks" in out, out[-3000:]
    assert "runtime error" not in out and "AddressSanitizer" not in out, out[-3000:]
