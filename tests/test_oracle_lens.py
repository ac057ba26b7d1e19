"""The oracle's thin lens (oracle/pt_oracle.hpp "thin lens") without a GPU: its frame against the library's host side
bit for bit, its rays against the numpy restatement (tests/lens_ref.py), aperture 0 against the pinhole oracle bit for bit, the
per-sample replay against the film, and -- for every job of tests/test_gpu_lens_parity.py -- that the f32 oracle stays within the
project's FP32 bar of the f64 oracle, which is what the fast-arithmetic GPU cases are then asked."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import lens_parity_jobs as lj
import lens_ref as lr

THREADS = min(16, os.cpu_count() or 1)
AXIS = dict(origin=(0.1, -0.2, 2.5), width=37, height=23, screen_distance=1.3, fov_degrees=41.0)      # the cameras of test_lens_cpu.py
LOOK = ((1.0, 0.7, 2.0), (0.0, -0.1, -2.0), (0.1, 1.0, 0.0), 37, 23, 33.0)
LENSES = ((0.3, 2.0), (0.05, 0.7), (2.5, 40.0), (0.0, 3.0), (0.2, 2.0), (3.0, 0.7), (1e-300, 1e300), (1e30, 1e-30))


def _cam(pt, kind):
    return pt.camera_new(**AXIS) if kind == "axis" else pt.camera_look_at(*LOOK)


def _xys(seed, n=4096):
    rng = np.random.default_rng(seed)
    xys = np.stack([rng.integers(0, 37, n), rng.integers(0, 23, n), rng.integers(0, 2 ** 32, n)], axis=1).astype(np.uint32)
    xys[:4] = [(0, 0, 0), (36, 22, 2 ** 32 - 1), (36, 0, 1), (0, 22, 7)]
    return xys


# ---------------------------------------------------------------- 1. the frame
@pytest.mark.parametrize("kind", ["axis", "look_at"])
def test_setup_is_the_librarys_bit_for_bit(pt, orc, kind):
    cam = _cam(pt, kind)
    for aperture, focus in LENSES:
        lens = pt.default_lens(aperture=aperture, focus_distance=focus)
        got, ref = orc.lens_setup(cam, lens), pt.lens_setup(cam, lens)
        assert got.dtype == ref.dtype == np.float32
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (aperture, focus, got, ref)


def test_setup_refuses_what_the_library_refuses(pt, orc):
    """The bad lenses and degenerate cameras of test_lens_cpu.py: the same refusal, in the same order of checks."""
    L = pt._lib.lib()
    cam = pt.camera_new(**AXIS)
    cases = [(cam, dict(aperture=a), "aperture") for a in (-1.0, -1e-300, math.inf, -math.inf, math.nan)]
    cases += [(cam, dict(aperture=0.3, focus_distance=f), "focus_distance") for f in (0.0, -2.0, math.inf, -math.inf, math.nan)]
    cases += [(cam, dict(aperture=-1.0, focus_distance=0.0), "aperture")]              # the aperture is checked first
    for field, value in (("horizontal", (0.0, 0.0, 0.0)), ("vertical", (0.0, 0.0, 0.0)), ("horizontal", (math.nan, 0.0, 0.0)),
                         ("vertical", (math.inf, 0.0, 0.0)), ("origin", (math.nan, 0.0, 0.0)), ("origin", (0.0, math.inf, 0.0))):
        bad = pt._lib.PtCamera.from_buffer_copy(cam)
        for k in range(3):
            getattr(bad, field)[k] = value[k]
        cases.append((bad, dict(aperture=0.3), "degenerate camera"))
        cases.append((bad, dict(aperture=0.3, focus_distance=-1.0), "focus_distance"))      # the lens before the camera
    centre = pt._lib.PtCamera.from_buffer_copy(cam)                # D = 0: the screen's centre is the origin
    for k, (o, h, v) in enumerate(((1.0, 2.0, 0.0), (2.0, 0.0, 1.0), (3.0, 0.0, 0.0))):
        centre.origin[k], centre.horizontal[k], centre.vertical[k], centre.lower_left[k] = o, h, v, o - h / 2 - v / 2
    cases.append((centre, dict(aperture=0.3), "degenerate camera"))
    xys = np.array([[1, 2, 3]], dtype=np.uint32)
    for c, kw, part in cases:
        lens = pt.default_lens(**kw)
        out7 = (C.c_float * 7)(*([7.0] * 7))
        assert L.pt_debug_lens_setup(C.byref(c), C.byref(lens), out7) == 1 and part in L.pt_last_error().decode(), (kw, part)
        for call in (lambda: orc.lens_setup(c, lens), lambda: orc.lens_rays(c, lens, xys),
                     lambda: orc.render_lens(c, lens, pt.builtin_scene(2), pt.default_params(spp=1)),
                     lambda: orc.render_pixels_lens(c, lens, pt.builtin_scene(2), pt.default_params(spp=1), xys[:, :2])):
            with pytest.raises(orc.LensRefused) as e:
                call()
            assert e.value.part == part, (kw, part, e.value.part)
    raw = np.full(7, 7.0, dtype=np.float32)                        # a refusal writes nothing
    assert orc.lib().orc_lens_setup(C.byref(cam), C.byref(pt.default_lens(aperture=-1.0)), raw.ctypes.data_as(C.c_void_p)) == 1
    assert np.array_equal(raw, np.full(7, 7.0, dtype=np.float32))


# ---------------------------------------------------------------- 2. the rays
@pytest.mark.parametrize("kind", ["axis", "look_at"])
@pytest.mark.parametrize("aperture,focus", [(0.3, 2.5), (3.0, 0.7)])
def test_rays_against_the_numpy_restatement(pt, orc, kind, aperture, focus):
    """f64: both sides state the rule in f64 with no f32 anywhere (the uniforms are exact in either), so they differ by
    rounding alone.  The rule makes 8 roundings on the way to o' (test_gpu_lens.py counts them: the quotient, the angle, the
    sine / cosine, r cos, dx Lu, dy Lv, their sum, origin + l); each side may be off by that, and numpy states the angle in
    radians where the oracle has revolutions: 16 f64 ulps of the largest coordinate magnitude involved.
    f32: against the restatement under the device's f32 words, within the 8 f32 ulps test_gpu_lens.py derives."""
    cam = _cam(pt, kind)
    lens = pt.default_lens(aperture=aperture, focus_distance=focus)
    xys = _xys(11)
    mag = max(np.abs(np.concatenate(lr.cam_fields(cam))).max(), aperture / 2 + np.abs(lr.cam_fields(cam)[0]).max())
    for precision, ref, bound in (
            (orc.F64, lr.rays(cam, lr.setup(cam, aperture, focus, f32=False), xys, f32=False), 16 * lr.ulp32(mag) * 2.0 ** -29),
            (orc.F32, lr.rays(cam, orc.lens_setup(cam, lens), xys), 8 * lr.ulp32(mag))):
        got = orc.lens_rays(cam, lens, xys, precision)
        o, d, dx, dy = got[:, 0:3], got[:, 3:6], got[:, 6], got[:, 7]
        errs = [np.abs(o - ref["o"]).max(), np.abs(d - ref["d"]).max(), np.abs(dx - ref["dx"]).max(), np.abs(dy - ref["dy"]).max()]
        print(f"{kind} aperture {aperture} f{precision}: |o'|, |d'|, |dx|, |dy| off by {errs[0]:.2e} {errs[1]:.2e} {errs[2]:.2e} {errs[3]:.2e}, bound {bound:.2e}")
        assert max(errs) <= bound
        assert np.all(dx * dx + dy * dy <= 1.0)
        assert np.abs(np.linalg.norm(d, axis=1) - 1.0).max() <= (4 * 2.0 ** -23 if precision == orc.F32 else 4 * 2.0 ** -52)
        assert np.linalg.norm(o - ref["origin"], axis=1).max() > 0.9 * aperture / 2            # the lens is used to its rim
        # every ray passes its sample's focus point
        to_f = ref["focus"] - o
        dist = np.linalg.norm(to_f, axis=1)
        off = np.linalg.norm(to_f - (to_f * d).sum(axis=1)[:, None] * d, axis=1)
        assert np.all(off <= bound * np.maximum(dist, 1.0))
        if precision == orc.F32:
            assert np.array_equal(got, got.astype(np.float32).astype(np.float64))              # f32 values, carried in f64


def test_rays_at_aperture_zero_are_the_pinhole_rays(pt, orc):
    cam = pt.camera_look_at(*LOOK)
    xys = _xys(12, 512)
    words = np.array([orc.philox((int(x), int(y), int(s), 0xFFFFFFFF), (0, 0)) for x, y, s in xys], dtype=np.uint64)
    off = np.stack([lr.u01(words[:, 0]), lr.u01(words[:, 1])], axis=1)
    flipped = np.stack([xys[:, 0], cam.height - 1 - xys[:, 1]], axis=1)
    for precision in (orc.F32, orc.F64):
        pin = orc.camera_rays(cam, flipped, off, precision)
        got = orc.lens_rays(cam, pt.default_lens(focus_distance=3.5), xys, precision)
        assert np.array_equal(got[:, :6], pin)


# ---------------------------------------------------------------- 3. aperture 0 is the pinhole render
@pytest.mark.parametrize("scene", ["diffuse", "mirror", "tiled"])
def test_aperture_zero_is_the_pinhole_oracle(pt, orc, scene):
    objs = pt.builtin_scene(*lj.SCENES[scene])
    cam = pt.camera_new(width=37, height=23)
    lens = pt.default_lens(focus_distance=1.7)
    for integ in (0, 1):
        for precision in (orc.F32, orc.F64):
            for form in (orc.RECURSIVE, orc.ITERATIVE):
                for band in (None, 0, 1, 2):
                    kw = dict(band_rows=4, band_count=3, band_index=band) if band is not None else {}
                    prm = pt.default_params(spp=3, spp_offset=2, integrator=integ, **kw)
                    a = orc.render_lens(cam, lens, objs, prm, precision, form, THREADS)
                    b = orc.render(cam, objs, prm, precision, form, THREADS)
                    assert a[0].shape == b[0].shape and a[0].shape[0] == (23 if band is None else len(pt.tile_row_indices(23, 4, band, 3)))
                    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2], (integ, precision, form, band)
    assert b[2]["vertices"] > 0


# ---------------------------------------------------------------- 4. the replay is the film
@pytest.mark.parametrize("job", lj.JOBS[:4], ids=lj.job_id)
def test_per_sample_radiance_sums_to_the_film(pt, orc, job):
    objs, cam, lens, prm = lj.make(pt, job)
    ys, xs = np.mgrid[0:cam.height, 0:cam.width]
    xy = np.stack([xs.ravel(), ys.ravel()], axis=1)
    for precision, form in ((orc.F32, orc.ITERATIVE), (orc.F64, orc.RECURSIVE)):
        film, _, _ = orc.render_lens(cam, lens, objs, prm, precision, form, THREADS)
        lin, smp = orc.render_pixels_lens(cam, lens, objs, prm, xy, precision, form)
        assert smp.shape == (len(xy), prm.spp, 3)
        acc = np.zeros((len(xy), 3))
        for s in range(prm.spp):                                   # the film's own order of summation
            acc = acc + smp[:, s]
        assert np.array_equal(acc / prm.spp, film.reshape(-1, 3)) and np.array_equal(lin, film.reshape(-1, 3))
        pin, _, _ = orc.render(cam, objs, prm, precision, form, THREADS)
        assert not np.array_equal(pin, film)                       # (the lens does something)


# ---------------------------------------------------------------- 5. the bar condition of the GPU jobs, on the reference alone
@pytest.mark.parametrize("job", lj.JOBS, ids=lj.job_id)
def test_f32_oracle_is_within_the_fp32_bar_of_the_f64_oracle(pt, orc, job):
    """What test_gpu_lens_parity.py asks of the fast-arithmetic GPU film against the f64 recursive oracle, asked of the f32
    iterative oracle first: a job the reference does not pass is changed in lens_parity_jobs.py, the bar is not."""
    objs, cam, lens, prm = lj.make(pt, job)
    r32, _, c32 = orc.render_lens(cam, lens, objs, prm, orc.F32, orc.ITERATIVE, THREADS)
    r64, _, c64 = orc.render_lens(cam, lens, objs, prm, orc.F64, orc.RECURSIVE, THREADS)
    p32, _, _ = orc.render(cam, objs, prm, orc.F32, orc.ITERATIVE, THREADS)
    p64, _, _ = orc.render(cam, objs, prm, orc.F64, orc.RECURSIVE, THREADS)
    (ls, lm), (ps, pm) = lj.outside_bar(r32, r64), lj.outside_bar(p32, p64)
    n = cam.width * cam.height * prm.spp
    print(f"{lj.job_id(job)}: outside the bar lens {ls:.4%} (mean off {lm:.1e}), pinhole {ps:.4%} ({pm:.1e}); "
          f"{c64['vertices'] / n - 1:.3f} vertices per sample past the first, film mean {r64.mean():.3g}")
    assert c64["vertices"] > n and r64.max() > 0                    # paths go on past their first vertex, and light arrives
    lj.within_bar(r32, r64)


def test_the_jobs_cover_what_they_claim():
    seen = {}
    for job in lj.JOBS:
        seen.setdefault(lj.route(job), []).append(job)
    assert set(seen) == {"lds", "tiled", "bvh"}
    for route, jobs in seen.items():
        assert {j[2] for j in jobs} == {0, 1} and {j[3] for j in jobs} == {"narrow", "wide"}, route
        assert {j[4] for j in jobs} == {lj.BIG, lj.ODD} and {j[5] for j in jobs} == {0, 5}, route
        assert all(6 <= j[6] <= 8 for j in jobs)
    assert {j[0] for j in seen["lds"]} == {"diffuse", "mirror"} and {j[0] for j in seen["bvh"]} == set(lj.SCENES)
    assert all((w * h * j[6]) % 64 for j in lj.JOBS for w, h in [j[4]] if (w, h) == lj.ODD)
