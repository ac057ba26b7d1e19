"""The brightness cascade without a GPU (include/pathtrace_amd.h): exports, defaults and refusals, the split of
one luminance at every level and special value, pt_cascade_host against the numpy restatement (tests/cascade_ref.py) bit for
bit, the properties the rule promises, and the rule header under the address and undefined-behaviour sanitizers in a
stand-alone program."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import cascade_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(2, 2), (3, 5), (17, 9), (33, 16)]          # (W, H)
COUNTS = [1, 3, 4, 5, 16]
LAYERS = [2, 6, 8]
SPECIALS = [0.0, -1.0, -0.0, 1e-42, float("nan"), float("inf")]      # zero, negative, denormal, NaN, +inf


def make_samples(seed, n, W, H):
    """log-uniform over 2^-4 .. 2^24 with the special values sprinkled in (whole samples and single channels)"""
    rng = np.random.default_rng(seed)
    s = np.exp2(rng.uniform(-4.0, 24.0, (n, H, W, 3))).astype(np.float32)
    m = n * H * W
    flat = s.reshape(m, 3)
    for k, v in enumerate(SPECIALS):
        for i in rng.choice(m, max(1, m // 40), replace=False):
            if (i + k) % 2:
                flat[i] = v
            else:
                flat[i, rng.integers(3)] = v
    return s


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b))


def test_symbols_are_exported_and_the_defaults(pt):
    lib = pt._lib.lib()
    for name in ("pt_default_cascade", "pt_render_cascade_device", "pt_render_cascade_host", "pt_cascade_samples_device", "pt_cascade_host",
                 "pt_debug_cascade_split"):
        assert hasattr(lib, name) and name in pt._lib.SYMBOLS
    cs = pt.default_cascade()
    assert (cs.layers, cs.start, cs.base) == (6, 1.0, 8.0)
    assert cs.kappa == 1.0                         # docs/EXPERIMENTS.md "Brightness cascade": chosen by measurement
    lib.pt_default_cascade(None)                   # tolerated, as the other defaults
    assert C.sizeof(pt._lib.PtCascade) == 16


def _host(pt, cs, W, H, n, smp, lin, rgba=None, plain=None, layers=None, weights=None):
    ptr = lambda a: None if a is None else (a if isinstance(a, (int, C.c_void_p)) else a.ctypes.data_as(C.c_void_p))  # noqa: E731
    return pt._lib.lib().pt_cascade_host(C.byref(cs) if cs is not None else None, W, H, n, ptr(smp), ptr(lin), ptr(rgba), ptr(plain),
                                         ptr(layers), ptr(weights))


def test_refusals(pt):
    lib = pt._lib.lib()
    W, H, n = 4, 3, 2
    smp = np.ones((n, H, W, 3), np.float32)
    lin, plain = np.empty((H, W, 3), np.float32), np.empty((H, W, 3), np.float32)
    rgba = np.empty((H, W, 4), np.uint8)
    ok = pt.default_cascade()
    assert _host(pt, ok, W, H, n, smp, lin, rgba, plain) == 0
    assert _host(pt, None, W, H, n, smp, lin) == 1 and _host(pt, ok, W, H, n, None, lin) == 1 and _host(pt, ok, W, H, n, smp, None) == 1
    for bad in (dict(layers=1), dict(layers=9), dict(layers=0), dict(start=0.0), dict(start=-1.0), dict(start=float("nan")),
                dict(start=float("inf")), dict(base=1.5), dict(base=float("inf")), dict(base=float("nan")), dict(kappa=-1.0),
                dict(kappa=float("nan")), dict(kappa=float("inf"))):
        cs = pt.default_cascade(**bad)
        assert _host(pt, cs, W, H, n, smp, lin) == 1, bad
        j, lo, hi = C.c_uint32(), C.c_double(), C.c_double()
        assert lib.pt_debug_cascade_split(C.byref(cs), 1.0, C.byref(j), C.byref(lo), C.byref(hi)) == 1, bad
        # the device entries refuse the parameters before they look at the context (none is needed to be refused)
        assert lib.pt_cascade_samples_device(None, C.byref(cs), W, H, n, 0, smp.ctypes.data_as(C.c_void_p), lin.ctypes.data_as(C.c_void_p),
                                             None, None) == 1, bad
    # No f32 start and base reach the overflow refusal within 8 layers: FLT_MAX^8 = 2^1024 (1 - 2^-24)^8 is below DBL_MAX, so
    # the largest table there is is accepted (the check guards the kernels against a table that a later, wider K could make)
    fmax = float(np.finfo(np.float32).max)
    assert _host(pt, pt.default_cascade(layers=8, start=fmax, base=fmax), W, H, n, smp, lin) == 0
    assert np.isfinite(cr.levels(8, fmax, fmax)).all()
    assert _host(pt, ok, 1, 8, n, smp, lin) == 1 and _host(pt, ok, 8, 1, n, smp, lin) == 1 and _host(pt, ok, 0, 0, n, smp, lin) == 1
    assert _host(pt, ok, W, H, 0, smp, lin) == 1
    # misaligned planes (4 bytes)
    raw = np.zeros(4 * H * W * 3 + 8, np.uint8)
    odd = C.c_void_p(raw.ctypes.data + 1 + (-raw.ctypes.data) % 4)
    assert _host(pt, ok, W, H, n, smp, odd) == 1 and _host(pt, ok, W, H, n, smp, lin, odd) == 1 and _host(pt, ok, W, H, n, smp, lin, None, odd) == 1
    assert _host(pt, ok, W, H, n, odd, lin) == 1
    # an output that aliases the input (anywhere inside it) or another output
    inside = C.c_void_p(smp.ctypes.data + 12 * H * W)
    assert _host(pt, ok, W, H, n, smp, smp) == 1 and _host(pt, ok, W, H, n, smp, inside) == 1
    assert _host(pt, ok, W, H, n, smp, lin, inside) == 1 and _host(pt, ok, W, H, n, smp, lin, None, inside) == 1
    assert _host(pt, ok, W, H, n, smp, lin, None, lin) == 1
    # the device entries: the same checks, before the context is looked at
    dev = lambda *a: lib.pt_cascade_samples_device(None, *a)  # noqa: E731
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert dev(C.byref(ok), W, H, n, 0, p(smp), p(lin), None, None) == 1 and "null context" in lib.pt_last_error().decode()
    assert dev(None, W, H, n, 0, p(smp), p(lin), None, None) == 1 and dev(C.byref(ok), W, H, n, 0, None, p(lin), None, None) == 1
    assert dev(C.byref(ok), W, H, n, 0, p(smp), None, None, None) == 1
    assert dev(C.byref(ok), 1, 1, n, 0, p(smp), p(lin), None, None) == 1 and "null context" not in lib.pt_last_error().decode()
    assert dev(C.byref(ok), W, H, 0, 0, p(smp), p(lin), None, None) == 1 and "null context" not in lib.pt_last_error().decode()
    assert dev(C.byref(ok), W, H, n, 0, p(smp), odd, None, None) == 1 and "aligned" in lib.pt_last_error().decode()
    assert dev(C.byref(ok), W, H, n, 0, p(smp), inside, None, None) == 1 and "alias" in lib.pt_last_error().decode()
    cam, prm = pt.camera_new(width=8, height=8), pt.default_params(spp=2)
    assert lib.pt_render_cascade_device(None, C.byref(cam), C.byref(prm), C.byref(ok), p(lin), None, None) == 1
    assert lib.pt_render_cascade_host(None, C.byref(cam), C.byref(prm), C.byref(ok), p(lin), None, None, None, None) == 1


def _ulp_neighbours(v):
    return [np.nextafter(v, -np.inf), v, np.nextafter(v, np.inf)]


@pytest.mark.parametrize("K", LAYERS)
def test_split_at_every_level_and_special_value(pt, K):
    cs = pt.default_cascade(layers=K)
    B = cr.levels(K, cs.start, cs.base)
    assert B[0] == 1.0 and all(B[k + 1] == B[k] * 8.0 for k in range(K - 1))
    cases = [float(x) for b in B for x in _ulp_neighbours(b)] + [0.0, -2.5, 5e-324, 1e-310, float("nan"), float("inf"), 3.0, 100.0, 2.0 ** 40]
    for L in cases:
        j, lo, hi = pt.cascade_split(cs, L)
        rj, rlo, rhi = (a.item() for a in cr.split(B, np.float64(L)))
        assert (j, lo, hi) == (rj, rlo, rhi) or (math.isnan(lo) and math.isnan(rlo)), L
        below = [k for k in range(K - 1) if B[k] <= L]
        assert j == (below[-1] if below else 0), L
        first, last = not (L > B[j]), L >= B[j + 1]
        if first:                                  # NaN, negatives, L <= B_0, L exactly a level
            assert (lo, hi) == (1.0, 0.0), L
        elif last:                                 # L >= B_{K-1}, +inf
            assert j == K - 2 and (lo, hi) == (0.0, 1.0), L
        else:
            assert B[j] < L < B[j + 1] and 0.0 <= lo <= 1.0 and 0.0 <= hi <= 1.0, L
            assert abs((lo + hi) - 1.0) <= 2.0 ** -52, L
            assert abs((lo * L + hi * L) - L) <= 4.0 * np.spacing(L), L
        assert first + last + (not first and not last) == 1
    # a level itself belongs to the layer it names; one ulp below it the layer under it holds almost nothing
    for k in range(1, K - 1):
        assert pt.cascade_split(cs, float(B[k])) == (k, 1.0, 0.0)
        j, lo, hi = pt.cascade_split(cs, float(np.nextafter(B[k], 0.0)))
        assert j == k - 1 and lo < 1e-15 and hi > 1.0 - 1e-15
    assert pt.cascade_split(cs, float(B[K - 1])) == (K - 2, 0.0, 1.0)


@pytest.mark.parametrize("K", LAYERS)
@pytest.mark.parametrize("W,H", SIZES)
def test_host_is_the_reference_bit_for_bit(pt, W, H, K):
    for n in COUNTS:
        smp = make_samples(1000 * K + 10 * W + n, n, W, H)
        cs = pt.default_cascade(layers=K, kappa=2.0 if n % 2 else 16.0)
        got = pt.cascade_host(smp, cs)
        ref = cr.cascade(smp, K, cs.start, cs.base, cs.kappa)
        for name, a, b in zip(("film", "rgba", "plain", "layers", "weights"), got, ref):
            assert same(a, b), (name, n)
        if n == 16 and K == 6 and (W, H) == (33, 16):
            assert (got[4] < 1.0).any() and (got[4] == 1.0).any()      # both branches of the weight were taken


def test_dark_samples_give_the_plain_film(pt):
    rng = np.random.default_rng(3)
    smp = rng.uniform(0.0, 1.0, (5, 9, 17, 3)).astype(np.float32)      # every luminance <= start = 1
    smp[2, 4, 4] = 1.0
    film, rgba, plain, layers, w = pt.cascade_host(smp, pt.default_cascade(kappa=8.0))
    assert same(film, plain) and not layers[1:].any()
    assert same(plain, (smp.astype(np.float64).cumsum(0)[-1] / 5.0).astype(np.float32))      # the sums of k_resolve, in sample order


def test_kappa_zero_keeps_every_sample(pt):
    rng = np.random.default_rng(4)
    n = 16
    smp = np.exp2(rng.uniform(-4.0, 24.0, (n, 9, 17, 3))).astype(np.float32)
    film, _, plain, _, w = pt.cascade_host(smp, pt.default_cascade(kappa=0.0))
    assert (w == 1.0).all()
    # the split's relative error is below n * 2^-51, far under half an f32 ulp: only rounding ties differ
    assert (np.abs(film.view(np.int32) - plain.view(np.int32)) <= 1).all()


def test_one_firefly_is_damped_and_nothing_else_moves(pt):
    n, S = 16, 9
    smp = np.full((n, S, S, 3), 0.5, np.float32)
    smp[7, 4, 4] = 1000.0                           # luminance 1000 (the weights add up to 1)
    cs = pt.default_cascade()
    film, _, plain, _, w = pt.cascade_host(smp, cs)
    ref = cr.cascade(smp, cs.layers, cs.start, cs.base, cs.kappa)
    assert same(film, ref[0])
    assert (film[4, 4] < plain[4, 4]).all() and same(film[4, 4], ref[0][4, 4])
    others = np.ones((S, S), bool)
    others[4, 4] = False
    assert same(film[others], plain[others])
    # 512 <= 1000 < 4096: the sample lies in layers 3 and 4; cnt_3 = 1000 / 512 reaches kappa = 1, cnt_4 = 1000 / 4096 does not
    assert w[3, 4, 4] == 1.0 and 0.0 < w[4, 4, 4] < 0.25


def test_a_block_of_bright_samples_is_kept(pt):
    n, S = 16, 9
    smp = np.full((n, S, S, 3), 0.5, np.float32)
    smp[:, 3:6, 3:6] = 1000.0
    film = pt.cascade_host(smp, pt.default_cascade())[0]
    keep = pt.cascade_host(smp, pt.default_cascade(kappa=0.0))[0]
    assert same(film, keep)


def test_nan_and_inf_stay_where_the_plain_film_has_them(pt):
    for seed, (W, H) in enumerate(SIZES):
        smp = make_samples(50 + seed, 5, W, H)
        film, _, plain, _, _ = pt.cascade_host(smp, pt.default_cascade())
        assert np.isnan(plain).any() and np.isinf(plain).any()
        assert np.array_equal(np.isnan(film), np.isnan(plain))
        assert np.array_equal(np.isinf(film), np.isinf(plain)) and not np.isneginf(film).any()
    # an infinite sample leaves no NaN in the layer under it
    smp = np.full((2, 2, 2, 3), 3.0, np.float32)
    smp[1, 0, 0] = np.inf
    film, _, plain, layers, _ = pt.cascade_host(smp, pt.default_cascade())
    assert np.isposinf(film[0, 0]).all() and np.isfinite(layers[:5]).all() and np.isposinf(layers[5, 0, 0]).all()


def test_rule_header_is_clean_under_asan_and_ubsan(tmp_path):
    """tests/tools/cascade_san.cpp: a stand-alone program around the host functions of pt_cascade.h"""
    exe = str(tmp_path / "cascade_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "tools", "cascade_san.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "cascade_san: 0 failed checks" in out, out[-3000:]
    assert "runtime error" not in out and "AddressSanitizer" not in out, out[-3000:]
