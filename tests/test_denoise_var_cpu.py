"""The variance-guided filter without a device: the ABI (symbols, the argument checks that need no context), the rule of
pathtrace_amd/csrc/pt_denoise_var.h compiled with the host compiler exactly as the kernel includes it against the numpy
restatement (tests/denoise_var_ref.py) bit for bit, and that restatement against tests/denoise_ref.py."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import denoise_ref as dr
import denoise_var_ref as dvr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pt_denoise_var_device", "pt_adaptive_variance_device", "pt_render_adaptive_denoised")
SRC = r"""
#include "pt_denoise_var.h"
extern "C" float dv_pixel_variance(const double* sums, unsigned n, float r, float g, float b) {
    return ptdv::pixel_variance(sums, n, r, g, b);
}
"""


def test_the_new_symbols_are_exported(pt):
    lib = pt._lib.lib()
    for name in NEW:
        assert name in pt._lib.SYMBOLS and hasattr(lib, name), name
    assert lib.pt_abi_version() == 6
    header = open(os.path.join(ROOT, "include", "pathtrace_amd.h")).read()
    for name in NEW:
        assert f"int {name}(" in header, name


def test_null_and_misaligned_arguments_are_refused_without_a_device(pt):
    lib = pt._lib.lib()
    cam = pt.camera_new(width=8, height=8)
    prm = pt.default_params(spp=8)
    dn = pt.default_denoise()
    ad = pt._lib.PtAdaptive(4, 4, 0.1, 1e-3)
    buf = (C.c_float * 1024)()
    base = C.addressof(buf)
    base += (-base) % 16
    ok, odd4, odd16 = C.c_void_p(base), C.c_void_p(base + 2), C.c_void_p(base + 4)
    out = C.c_void_p(base + 2048)
    # no context: every entry fails loudly
    assert lib.pt_denoise_var_device(None, 8, 8, ok, ok, ok, C.byref(dn), out, None) == 1
    assert b"pt_denoise_var_device" in lib.pt_last_error() and b"null" in lib.pt_last_error()
    assert lib.pt_adaptive_variance_device(None, 8, 8, ok, out) == 1
    assert b"pt_adaptive_variance_device" in lib.pt_last_error() and b"null" in lib.pt_last_error()
    assert lib.pt_render_adaptive_denoised(None, C.byref(cam), C.byref(prm), C.byref(ad), 4, C.byref(dn), buf, None, None, None, None, None) == 1
    assert b"pt_render_adaptive_denoised" in lib.pt_last_error() and b"null" in lib.pt_last_error()
    # a context-shaped pointer is never followed: the checks below fail on the argument before the context is used
    fake = C.c_void_p(base + 3072)
    for args in ((None, ok, ok, C.byref(dn), out), (ok, None, ok, C.byref(dn), out), (ok, ok, None, C.byref(dn), out),
                 (ok, ok, ok, None, out), (ok, ok, ok, C.byref(dn), None)):
        assert lib.pt_denoise_var_device(fake, 8, 8, *args, None) == 1
        assert b"null" in lib.pt_last_error()
    assert lib.pt_denoise_var_device(fake, 0, 8, ok, ok, ok, C.byref(dn), out, None) == 1
    assert lib.pt_denoise_var_device(fake, 8, 8, ok, odd16, ok, C.byref(dn), out, None) == 1
    assert b"16-byte" in lib.pt_last_error()
    assert lib.pt_denoise_var_device(fake, 8, 8, ok, ok, odd4, C.byref(dn), out, None) == 1
    assert b"d_var" in lib.pt_last_error()
    assert lib.pt_denoise_var_device(fake, 8, 8, odd4, ok, ok, C.byref(dn), out, None) == 1
    assert lib.pt_denoise_var_device(fake, 8, 8, ok, ok, ok, C.byref(dn), ok, None) == 1          # output = input
    for f, v in ((None, out), (ok, None)):
        assert lib.pt_adaptive_variance_device(fake, 8, 8, f, v) == 1
        assert b"null" in lib.pt_last_error()
    assert lib.pt_adaptive_variance_device(fake, 8, 8, odd16, out) == 1
    assert b"16-byte" in lib.pt_last_error()
    assert lib.pt_adaptive_variance_device(fake, 8, 8, ok, odd4) == 1
    assert b"d_var" in lib.pt_last_error()
    for args in ((None, C.byref(prm), C.byref(ad), 4, C.byref(dn), buf), (C.byref(cam), None, C.byref(ad), 4, C.byref(dn), buf),
                 (C.byref(cam), C.byref(prm), None, 4, C.byref(dn), buf), (C.byref(cam), C.byref(prm), C.byref(ad), 4, None, buf),
                 (C.byref(cam), C.byref(prm), C.byref(ad), 4, C.byref(dn), None)):
        assert lib.pt_render_adaptive_denoised(fake, *args, None, None, None, None, None) == 1
        assert b"null" in lib.pt_last_error()
    assert lib.pt_render_adaptive_denoised(fake, C.byref(cam), C.byref(prm), C.byref(ad), 0, C.byref(dn), buf, None, None, None, None, None) == 1
    assert b"feature_samples" in lib.pt_last_error()


# ---------------------------------------------------------------- the rule of pt_denoise_var.h
@pytest.fixture(scope="module")
def rule(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("dvrule")
    (d / "rule.cpp").write_text(SRC)
    so = d / "rule.so"
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-I",
                           os.path.join(ROOT, "pathtrace_amd", "csrc"), str(d / "rule.cpp"), "-o", str(so)])
    lib = C.CDLL(str(so))
    lib.dv_pixel_variance.restype = C.c_float
    lib.dv_pixel_variance.argtypes = [C.POINTER(C.c_double), C.c_uint, C.c_float, C.c_float, C.c_float]

    def fn(sums, n, albedo):
        s = (C.c_double * 5)(*[float(v) for v in sums])
        return np.float32(lib.dv_pixel_variance(s, int(n), float(albedo[0]), float(albedo[1]), float(albedo[2])))
    return fn


def _bits(v):
    return np.asarray(v, np.float32).view(np.uint32)


def _same(rule, sums, n, albedo):
    """header == numpy, bit for bit (one NaN is as good as another) -> the value"""
    got = rule(sums, n, albedo)
    want = dvr.pixel_variance(np.asarray(sums, np.float64), n, np.asarray(albedo, np.float32))
    assert (math.isnan(got) and math.isnan(want)) or _bits(got) == _bits(want), (sums, n, albedo, got, want)
    return got


def test_rule_on_random_sums(rule):
    rng = np.random.default_rng(11)
    seen_pos = 0
    for _ in range(600):
        n = int(rng.integers(2, 80))
        smp = rng.exponential(rng.uniform(1e-4, 3.0), size=(n, 3)).astype(np.float32)
        smp[rng.random(n) < 0.2] = 0.0
        albedo = rng.uniform(0.0, 1.0, 3).astype(np.float32)
        if rng.random() < 0.3:
            albedo[:] = albedo[0]                               # grey
        v = _same(rule, dvr.sums_of(smp), n, albedo)
        assert v >= 0 and np.isfinite(v)
        seen_pos += v > 0
    assert seen_pos > 500


def test_rule_is_exact_for_a_grey_albedo(rule):
    """L_u = mean / a, so var_u = var_c / a^2 up to the rounding of the ratio."""
    rng = np.random.default_rng(12)
    smp = rng.uniform(0.0, 2.0, (16, 3)).astype(np.float32)
    s = dvr.sums_of(smp)
    mean = s[3] / 16
    var_c = max(0.0, (s[4] - s[3] * mean) / 15) / 16
    for a in (1.0, 0.5, 0.18):
        v = _same(rule, s, 16, (a, a, a))
        assert v == pytest.approx(var_c / np.float64(np.float32(a)) ** 2, rel=1e-6)


def test_rule_edge_cases(rule):
    grey = (0.5, 0.5, 0.5)
    # n = 2: samples of luminance 0 and 2 -> mean 1, var 2, var_c 1; albedo 1 -> L_u = mean
    s = dvr.sums_of([[0, 0, 0], [2, 2, 2]])
    assert _same(rule, s, 2, (1, 1, 1)) == pytest.approx(1.0, rel=1e-6)
    # all samples equal: variance 0 (a pixel that sees the light directly)
    assert _bits(_same(rule, dvr.sums_of([[15, 15, 15]] * 8), 8, (1, 1, 1))) == 0
    assert _same(rule, dvr.sums_of([[0.3, 0.2, 0.1]] * 5), 5, grey) <= 1e-15      # (the sums of k L round: not exactly 0)
    # mean 0 (black, a miss): 0, not the NaN of 0 / 0
    assert _bits(_same(rule, np.zeros(5), 4, (1, 1, 1))) == 0
    assert _bits(_same(rule, np.zeros(5), 4, (0, 0, 0))) == 0
    # albedo below 1e-3 is clamped: no division by 0, and the value of an albedo at the clamp (f32(1e-3) is 5e-8 above it)
    s = dvr.sums_of(np.random.default_rng(13).uniform(0, 1, (12, 3)))
    tiny = _same(rule, s, 12, (0.0, 1e-5, -1.0))
    assert np.isfinite(tiny) and tiny > 0
    assert tiny == pytest.approx(float(_same(rule, s, 12, (1e-3, 1e-3, 1e-3))), rel=1e-6)
    # non-finite S1 or S2: NaN, whatever the rest
    for s1, s2 in ((math.nan, 1.0), (1.0, math.nan), (math.inf, math.inf), (1.0, math.inf), (-math.inf, 1.0), (math.inf, 1.0)):
        assert math.isnan(_same(rule, [1.0, 1.0, 1.0, s1, s2], 16, grey))
    # finite luminance sums with a non-finite colour sum: no measurement of L_u, 0
    assert _bits(_same(rule, [math.inf, 1.0, 1.0, 4.0, 5.0], 4, grey)) == 0
    assert _bits(_same(rule, [math.nan, 1.0, 1.0, 4.0, 5.0], 4, grey)) == 0
    # negative raw variance (S2 < S1^2 / n) is clamped to 0
    assert _bits(_same(rule, [4.0, 4.0, 4.0, 4.0, 3.9], 4, grey)) == 0


# ---------------------------------------------------------------- the restatement of the filter
def test_restatement_with_no_measurement_is_denoise_ref_exactly():
    rng = np.random.default_rng(21)
    c, f = dr.random_inputs(rng, 19, 23)
    for iters in (0, 1, 3):
        want = dr.denoise(c, f, iterations=iters)
        for fill in (np.nan, -1.0, np.inf, -np.inf):
            got = dvr.denoise_var(c, f, np.full((19, 23), fill, np.float32), iterations=iters)
            assert np.array_equal(got, want), (iters, fill)


def test_restatement_takes_the_plane_where_it_is_a_measurement():
    rng = np.random.default_rng(22)
    H, W = 17, 21
    c, f = dr.random_inputs(rng, H, W)
    u, a = dr.demodulate(c, f)
    spatial = dr.initial_variance(u)
    # the filter's own variance handed in as the plane: the same film (f64 -> f32 -> f64 rounds the plane, so not bit for bit)
    got = dvr.denoise_var(c, f, spatial.astype(np.float32), iterations=3)
    assert np.allclose(got, dr.denoise(c, f, iterations=3), rtol=1e-5, atol=1e-9)
    # variance 0 everywhere: the luminance stop closes, every pixel keeps its value
    got = dvr.denoise_var(c, f, np.zeros((H, W), np.float32), iterations=3)
    assert np.allclose(got, c, rtol=1e-12, atol=0)
    # a huge variance opens the luminance stop, a tiny one all but closes it (one depth, no emitters: nothing else stops a tap)
    f[..., 3] = 0
    f[..., 7] = 2.0
    wide = dvr.denoise_var(c, f, np.full((H, W), 1e30, np.float32), iterations=3)
    narrow = dvr.denoise_var(c, f, np.full((H, W), 1e-8, np.float32), iterations=3)
    assert (wide / a @ dr.LW).std() < 0.5 * (narrow / a @ dr.LW).std()      # the filter smooths u = c / a
    # iterations = 0 never reads the plane
    assert np.array_equal(dvr.denoise_var(c, f, dvr.random_variance(rng, H, W), iterations=0), dr.denoise(c, f, iterations=0))


def test_random_variance_planes_hold_every_kind_of_entry():
    """The planes of tests/test_gpu_denoise_var.py: zeros, 1e-8 .. 1e2, a third NaN or negative."""
    for H, W in ((9, 33), (61, 97)):
        v = dvr.random_variance(np.random.default_rng(H), H, W)
        t = dvr.taken(v)
        pos = v[t & (v > 0)]
        assert 0.25 <= 1 - t.mean() - np.mean(v == np.inf) <= 0.42
        assert np.isnan(v).any() and (v[~np.isnan(v)] < 0).any() and (v == 0).any() and (v == np.inf).any() and (v == -np.inf).any()
        assert pos.min() >= 1e-8 * 0.999 and pos.max() <= 1e2 * 1.001 and pos.min() < 1e-6 and pos.max() > 1.0
