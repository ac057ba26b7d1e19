"""The stopping rule of pt_render_adaptive (pathtrace_amd/csrc/pt_adaptive.h), compiled with the host compiler exactly as the
kernels include it, against a numpy restatement of the rule.  Both sides are IEEE f64 operations in the same order, so
they must agree bit for bit -- also right at the threshold, where only the rounding of rel_tol * scale decides."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LUM = (0.2126, 0.7152, 0.0722)
SRC = r"""
#include "pt_adaptive.h"
extern "C" int ad_check(double s1, double s2, unsigned n, double rel_tol, double abs_floor, double* rel_err) {
    return ptad::check(s1, s2, n, rel_tol, abs_floor, rel_err) ? 1 : 0;
}
extern "C" double ad_luminance(float r, float g, float b) { return ptad::luminance(r, g, b); }
"""


@pytest.fixture(scope="module")
def rule(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("adrule")
    (d / "rule.cpp").write_text(SRC)
    so = d / "rule.so"
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-I",
                           os.path.join(ROOT, "pathtrace_amd", "csrc"), str(d / "rule.cpp"), "-o", str(so)])
    lib = C.CDLL(str(so))
    lib.ad_check.restype = C.c_int
    lib.ad_check.argtypes = [C.c_double, C.c_double, C.c_uint, C.c_double, C.c_double, C.POINTER(C.c_double)]
    lib.ad_luminance.restype = C.c_double
    lib.ad_luminance.argtypes = [C.c_float, C.c_float, C.c_float]

    def check(s1, s2, n, tol, floor):
        rel = C.c_double(0.0)
        ok = lib.ad_check(s1, s2, n, tol, floor, C.byref(rel))
        return bool(ok), rel.value
    check.luminance = lib.ad_luminance
    return check


def numpy_rule(s1, s2, n, tol, floor):
    s1, s2 = np.float64(s1), np.float64(s2)
    mean = s1 / np.float64(n)
    var = (s2 - s1 * mean) / (np.float64(n) - 1.0)
    var = var if var > 0.0 else np.float64(0.0)
    se = np.sqrt(var / np.float64(n))
    scale = mean if mean > floor else np.float64(floor)
    finite = np.isfinite(s1) and np.isfinite(s2)
    rel = se / scale if finite else math.nan
    return bool(finite and tol > 0.0 and se <= tol * scale), float(rel)


def sums(L):
    L = np.asarray(L, dtype=np.float64)
    s1 = s2 = 0.0
    for v in L:                       # in sample order, like the resolve
        s1 += v
        s2 += v * v
    return s1, s2


def same(a, b):
    return a[0] == b[0] and (a[1] == b[1] or (math.isnan(a[1]) and math.isnan(b[1])))


def test_zero_variance(rule):
    s1, s2 = sums([0.75] * 8)
    assert rule(s1, s2, 8, 1e-6, 1e-3) == (True, 0.0)
    assert rule(s1, s2, 8, 0.0, 1e-3) == (False, 0.0)          # rel_tol = 0: no tolerance, nothing converges
    assert same(rule(s1, s2, 8, 1e-6, 1e-3), numpy_rule(s1, s2, 8, 1e-6, 1e-3))


def test_dark_pixel_uses_the_floor(rule):
    s1, s2 = sums([0.0, 2e-5, 0.0, 1e-5])                      # mean 7.5e-6 < abs_floor
    ok, rel = rule(s1, s2, 4, 0.5, 1e-3)
    mean = s1 / 4
    se = math.sqrt(max(0.0, (s2 - s1 * mean) / 3) / 4)
    assert rel == se / 1e-3 and ok == (se <= 0.5 * 1e-3)
    assert ok                                                  # against the mean itself it would not pass
    assert not rule(s1, s2, 4, 0.5, 1e-9)[0]
    assert same(rule(s1, s2, 4, 0.5, 1e-3), numpy_rule(s1, s2, 4, 0.5, 1e-3))


@pytest.mark.parametrize("s1,s2", [(math.nan, 1.0), (1.0, math.nan), (math.inf, math.inf), (1.0, math.inf), (-math.inf, 1.0)])
def test_non_finite_sums_never_converge(rule, s1, s2):
    ok, rel = rule(s1, s2, 16, 1e300, 1e-3)
    assert not ok and math.isnan(rel)


def test_two_samples(rule):
    s1, s2 = sums([0.0, 2.0])                                  # mean 1, var 2, se 1
    assert rule(s1, s2, 2, 1.0, 1e-3) == (True, 1.0)
    assert rule(s1, s2, 2, math.nextafter(1.0, 0.0), 1e-3) == (False, 1.0)


def test_at_the_threshold(rule):
    """se <= rel_tol * scale with rel_tol at and next to se / scale: the C++ and numpy answers are the same bits."""
    rng = np.random.default_rng(7)
    hits = 0
    for _ in range(400):
        n = int(rng.integers(2, 64))
        L = rng.exponential(rng.uniform(1e-4, 3.0), size=n)
        L[rng.random(n) < 0.2] = 0.0
        s1, s2 = sums(L)
        _, rel = numpy_rule(s1, s2, n, 1.0, 1e-3)
        for tol in (rel, math.nextafter(rel, 0.0), math.nextafter(rel, math.inf)):
            got, want = rule(s1, s2, n, tol, 1e-3), numpy_rule(s1, s2, n, tol, 1e-3)
            assert same(got, want), (n, s1, s2, tol, got, want)
            hits += got[0]
    assert 0 < hits < 1200


def test_luminance_weights(rule):
    rng = np.random.default_rng(3)
    for r, g, b in rng.uniform(0, 20, size=(200, 3)).astype(np.float32):
        want = LUM[0] * np.float64(r) + LUM[1] * np.float64(g) + LUM[2] * np.float64(b)
        assert rule.luminance(r, g, b) == want
