"""The film's reconstruction filters without a GPU (include/pathtrace_amd.h): exports, defaults and refusals, the
jitter against the Philox words of tests/lens_ref.py, the one-dimensional weight at every piece boundary, exp_neg against numpy,
pt_filter_host against the numpy restatement (tests/filter_ref.py) bit for bit, the properties the rule promises, and the rule
header under the address and undefined-behaviour sanitizers in a stand-alone program."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import filter_ref as fr
import lens_ref as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(2, 2), (3, 5), (17, 9), (33, 16)]          # (W, H)
COUNTS = [1, 3, 4, 5, 16]
RADII = [0.5, 0.75, 1.5, 1.51, 2.0, 2.5]             # both sides of each change of m
# (kind, a, b): every kind; two Gaussians and two Mitchells (the second with the deepest negative lobes)
KINDS = [(fr.BOX, 0.0, 0.0), (fr.TENT, 0.0, 0.0), (fr.GAUSSIAN, 2.0, 0.0), (fr.GAUSSIAN, 16.0, 0.0), (fr.MITCHELL, 1.0 / 3.0, 1.0 / 3.0),
         (fr.MITCHELL, 0.0, 1.0)]
POSITIVE = [k for k in KINDS if k[0] != fr.MITCHELL]


def make_samples(seed, n, W, H, wild=True):
    """log-uniform over 2^-8 .. 2^8, with zeros, negatives, denormals, NaN and +inf sprinkled in when wild"""
    rng = np.random.default_rng(seed)
    s = np.exp2(rng.uniform(-8.0, 8.0, (n, H, W, 3))).astype(np.float32)
    if wild:
        flat = s.reshape(-1, 3)
        m = flat.shape[0]
        for k, v in enumerate([0.0, -1.0, 1e-42, float("nan"), float("inf")]):
            for i in rng.choice(m, max(1, m // 60), replace=False):
                if (i + k) % 2:
                    flat[i] = v
                else:
                    flat[i, rng.integers(3)] = v
    return s


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def same(a, b):
    """bit for bit, except that any NaN equals any NaN: IEEE 754 leaves the sign and payload of a NaN result open (inf - inf under
    Mitchell's negative weights gives x86's negative default NaN, and which of two NaN operands an addition hands on depends on
    the order the compiler gave them), so they are not part of what the rule fixes"""
    if not (a.dtype == b.dtype and a.shape == b.shape):
        return False
    if a.dtype.kind != "f":
        return np.array_equal(bits(a), bits(b))
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(bits(np.where(na, 0, a).astype(a.dtype)), bits(np.where(nb, 0, b).astype(b.dtype)))


def flt_of(pt, kind, radius, a=0.0, b=0.0):
    return pt.default_filter(kind=kind, radius=radius, a=a, b=b)


def test_symbols_are_exported_and_the_defaults(pt):
    lib = pt._lib.lib()
    for name in ("pt_default_filter", "pt_render_filtered_device", "pt_render_filtered_host", "pt_filter_samples_device", "pt_filter_host",
                 "pt_debug_filter_weight", "pt_debug_filter_offsets", "pt_debug_filter_exp_neg"):
        assert hasattr(lib, name) and name in pt._lib.SYMBOLS
    f = pt.default_filter()
    assert (f.kind, f.radius, f.a) == (pt._lib.FILTER_GAUSSIAN, 1.5, 2.0)
    assert (pt._lib.FILTER_BOX, pt._lib.FILTER_TENT, pt._lib.FILTER_GAUSSIAN, pt._lib.FILTER_MITCHELL) == (fr.BOX, fr.TENT, fr.GAUSSIAN, fr.MITCHELL)
    lib.pt_default_filter(None)                    # tolerated, as the other defaults
    assert C.sizeof(pt._lib.PtFilter) == 16
    assert pt.default_filter(kind="mitchell").kind == fr.MITCHELL


def _host(pt, flt, W, H, n, smp, lin, rgba=None, plain=None, wsum=None, first=0):
    ptr = lambda a: None if a is None else (a if isinstance(a, (int, C.c_void_p)) else a.ctypes.data_as(C.c_void_p))  # noqa: E731
    return pt._lib.lib().pt_filter_host(C.byref(flt) if flt is not None else None, W, H, n, first, ptr(smp), ptr(lin), ptr(rgba), ptr(plain), ptr(wsum))


BAD_FILTERS = [dict(kind=4), dict(kind=0xFFFFFFFF), dict(radius=0.49), dict(radius=2.51), dict(radius=0.0), dict(radius=-1.0),
               dict(radius=float("nan")), dict(radius=float("inf")), dict(a=0.0), dict(a=-1.0), dict(a=16.5), dict(a=float("nan")),
               dict(a=float("inf")), dict(kind=3, a=-0.1, b=0.5), dict(kind=3, a=1.1, b=0.5), dict(kind=3, a=float("nan"), b=0.5),
               dict(kind=3, a=0.5, b=-0.1), dict(kind=3, a=0.5, b=1.1), dict(kind=3, a=0.5, b=float("nan")), dict(kind=3, a=0.5, b=float("inf"))]


def test_refusals(pt):
    lib = pt._lib.lib()
    W, H, n = 4, 3, 2
    smp = np.ones((n, H, W, 3), np.float32)
    lin, plain = np.empty((H, W, 3), np.float32), np.empty((H, W, 3), np.float32)
    rgba, wsum = np.empty((H, W, 4), np.uint8), np.empty((H, W), np.float64)
    ok = pt.default_filter()
    assert _host(pt, ok, W, H, n, smp, lin, rgba, plain, wsum) == 0
    assert _host(pt, None, W, H, n, smp, lin) == 1 and _host(pt, ok, W, H, n, None, lin) == 1 and _host(pt, ok, W, H, n, smp, None) == 1
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    for bad in BAD_FILTERS:
        f = pt.default_filter(**bad)
        assert _host(pt, f, W, H, n, smp, lin) == 1, bad
        out = C.c_double()
        assert lib.pt_debug_filter_weight(C.byref(f), 0.25, C.byref(out)) == 1, bad
        # the device entries refuse the parameters before they look at the context (none is needed to be refused)
        assert lib.pt_filter_samples_device(None, C.byref(f), W, H, n, 0, 0, p(smp), p(lin), None, None, None) == 1, bad
        assert "null context" not in lib.pt_last_error().decode(), bad
    # a and b are ignored where the kind has no use for them
    for kind in (fr.BOX, fr.TENT):
        assert _host(pt, pt.default_filter(kind=kind, a=float("nan"), b=-5.0), W, H, n, smp, lin) == 0
    assert _host(pt, pt.default_filter(b=float("nan")), W, H, n, smp, lin) == 0
    assert _host(pt, ok, 1, 8, n, smp, lin) == 1 and _host(pt, ok, 8, 1, n, smp, lin) == 1 and _host(pt, ok, 0, 0, n, smp, lin) == 1
    assert _host(pt, ok, W, H, 0, smp, lin) == 1
    # misaligned planes
    raw = np.zeros(8 * H * W * 3 + 16, np.uint8)
    odd = C.c_void_p(raw.ctypes.data + 1 + (-raw.ctypes.data) % 8)
    four = C.c_void_p(raw.ctypes.data + 4 + (-raw.ctypes.data) % 8)
    assert _host(pt, ok, W, H, n, smp, odd) == 1 and _host(pt, ok, W, H, n, smp, lin, odd) == 1 and _host(pt, ok, W, H, n, smp, lin, None, odd) == 1
    assert _host(pt, ok, W, H, n, odd, lin) == 1 and _host(pt, ok, W, H, n, smp, lin, None, None, four) == 1
    # an output that aliases the input (anywhere inside it) or another output
    inside = C.c_void_p(smp.ctypes.data + 12 * H * W)
    assert _host(pt, ok, W, H, n, smp, smp) == 1 and _host(pt, ok, W, H, n, smp, inside) == 1
    assert _host(pt, ok, W, H, n, smp, lin, inside) == 1 and _host(pt, ok, W, H, n, smp, lin, None, inside) == 1
    assert _host(pt, ok, W, H, n, smp, lin, None, lin) == 1 and _host(pt, ok, W, H, n, smp, lin, None, None, p(lin)) == 1
    # the device entries: the same checks, before the context is looked at
    dev = lambda *a: lib.pt_filter_samples_device(None, *a)  # noqa: E731
    assert dev(C.byref(ok), W, H, n, 0, 0, p(smp), p(lin), None, None, None) == 1 and "null context" in lib.pt_last_error().decode()
    assert dev(None, W, H, n, 0, 0, p(smp), p(lin), None, None, None) == 1 and dev(C.byref(ok), W, H, n, 0, 0, None, p(lin), None, None, None) == 1
    assert dev(C.byref(ok), W, H, n, 0, 0, p(smp), None, None, None, None) == 1
    assert dev(C.byref(ok), 1, 1, n, 0, 0, p(smp), p(lin), None, None, None) == 1 and "null context" not in lib.pt_last_error().decode()
    assert dev(C.byref(ok), W, H, 0, 0, 0, p(smp), p(lin), None, None, None) == 1 and "null context" not in lib.pt_last_error().decode()
    assert dev(C.byref(ok), W, H, n, 0, 0, p(smp), odd, None, None, None) == 1 and "aligned" in lib.pt_last_error().decode()
    assert dev(C.byref(ok), W, H, n, 0, 0, p(smp), inside, None, None, None) == 1 and "alias" in lib.pt_last_error().decode()
    cam, prm = pt.camera_new(width=8, height=8), pt.default_params(spp=2)
    assert lib.pt_render_filtered_device(None, C.byref(cam), C.byref(prm), C.byref(ok), p(lin), None, None) == 1
    assert lib.pt_render_filtered_host(None, C.byref(cam), C.byref(prm), C.byref(ok), p(lin), None, None, None) == 1
    ox = C.c_double()
    assert lib.pt_debug_filter_offsets(0, 0, 0, None, C.byref(ox)) == 1 and lib.pt_debug_filter_weight(C.byref(ok), 0.0, None) == 1
    assert lib.pt_debug_filter_exp_neg(-1.0, C.byref(ox)) == 1 and lib.pt_debug_filter_exp_neg(100.5, C.byref(ox)) == 1


def test_offsets_are_the_camera_words(pt):
    rng = np.random.default_rng(11)
    n = 300
    x = rng.integers(0, 2 ** 12, n)
    y = rng.integers(0, 2 ** 12, n)
    s = rng.integers(0, 2 ** 10, n) + 5                              # from a non-zero first_sample
    big = np.arange(n) % 3 == 0                                      # every third: x, y, s above 2^16
    x[big] += 2 ** 16 + rng.integers(0, 2 ** 15, big.sum())
    y[big] += 2 ** 17
    s[big] += 2 ** 16 + 2 ** 31
    x[:4], y[:4], s[:4] = [0, 0xFFFFFFFF, 0, 1], [0, 0xFFFFFFFF, 1, 0], [0, 0xFFFFFFFF, 0, 0]
    w = lr.words(x, y, s)
    ox, oy = lr.u01(w[:, 0]), lr.u01(w[:, 1])
    for i in range(n):
        got = pt.filter_offsets(int(x[i]), int(y[i]), int(s[i]))
        assert got == (ox[i], oy[i]), (x[i], y[i], s[i])
        k = int(w[i, 0]) >> 9
        assert got[0] * 2.0 ** 24 == 2 * k + 1 and 0.0 < got[0] < 1.0    # exact in f64


def _around(v):
    return [np.nextafter(v, -np.inf), v, np.nextafter(v, np.inf)]


@pytest.mark.parametrize("kind,a,b", KINDS)
def test_weight_at_every_piece_boundary(pt, kind, a, b):
    for radius in RADII:
        f = flt_of(pt, kind, radius, a, b)
        R = np.float64(np.float32(radius))
        ts = [0.0, 5e-324, 1e-300, 0.1, 0.5, 1.0, 3.0, 1e30] + _around(R) + _around(R / 2.0) + [float(v) for v in np.linspace(0.0, float(R), 37)]
        ts += _around(np.float64(0.5) * R)         # z = 1: where Mitchell's pieces meet
        ref = fr.weight1(kind, radius, a, b, np.array(ts, np.float64))
        for t, want in zip(ts, ref):
            got = pt.filter_weight(f, float(t))
            assert np.float64(got).tobytes() == np.float64(want).tobytes(), (radius, t, got, want)
            assert pt.filter_weight(f, -float(t)) == got
            if t >= R:
                assert got == 0.0
        if kind == fr.BOX:
            assert pt.filter_weight(f, float(np.nextafter(R, 0.0))) == 1.0
        if kind in (fr.TENT, fr.GAUSSIAN):
            assert pt.filter_weight(f, 0.0) > 0.0 and pt.filter_weight(f, 0.25) > pt.filter_weight(f, 0.45)
    if kind == fr.MITCHELL:                        # the textbook values of the cubic: f(0) = (6 - 2B) / 6, f(R/2) = B / 6 ... continuous at z = 1
        f = flt_of(pt, kind, 2.0, a, b)
        B = np.float64(np.float32(a))
        assert abs(pt.filter_weight(f, 0.0) - (6.0 - 2.0 * B) / 6.0) < 1e-15
        lo, hi = pt.filter_weight(f, float(np.nextafter(1.0, 0.0))), pt.filter_weight(f, 1.0)
        assert abs(lo - hi) < 1e-14 and abs(hi - B / 6.0) < 1e-15
        assert abs(pt.filter_weight(f, float(np.nextafter(2.0, 0.0)))) < 1e-14


def test_exp_neg_against_numpy(pt):
    """1e-12 relative: eight squarings amplify the polynomial's rounding (~1e-16) by 2^8, with a wide margin"""
    e = np.concatenate([np.linspace(0.0, 100.0, 4094), [np.nextafter(0.0, 1.0), np.nextafter(100.0, 0.0)]])
    got = np.array([pt.filter_exp_neg(float(v)) for v in e])
    want = np.exp(-e)
    rel = np.abs(got - want) / want
    print("exp_neg: worst relative error %.3g" % rel.max())
    assert rel.max() <= 1e-12
    assert same(got, fr.exp_neg(e))                # ... and the restatement is the header bit for bit
    assert pt.filter_exp_neg(0.0) == 1.0


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("kind,a,b", KINDS)
def test_host_is_the_reference_bit_for_bit(pt, W, H, kind, a, b):
    seen_m = set()
    for ri, radius in enumerate(RADII):
        for n in COUNTS:
            first = 0 if n % 2 else 7
            smp = make_samples(100 * W + 10 * n + ri, n, W, H)
            got = pt.filter_host(smp, flt_of(pt, kind, radius, a, b), first_sample=first)
            ref = fr.film(smp, kind, radius, a, b, first_sample=first)
            for name, x, y in zip(("film", "rgba", "plain", "wsum"), got, ref):
                assert same(x, y), (name, radius, n)
            seen_m.add(fr.taps(radius))
    assert seen_m == {0, 1, 2}


def test_box_half_is_the_plain_mean(pt):
    for seed, (W, H) in enumerate(SIZES):
        for n in COUNTS:
            smp = make_samples(300 + seed, n, W, H)
            film, rgba, plain, wsum = pt.filter_host(smp, flt_of(pt, fr.BOX, 0.5), first_sample=3)
            assert same(film, plain) and (wsum == float(n)).all()
            assert same(plain, (smp.astype(np.float64).cumsum(0)[-1] / np.float64(n)).astype(np.float32))      # the sums of k_resolve, in sample order
            assert same(rgba[..., :3], fr.byte8(smp.astype(np.float64).cumsum(0)[-1] / np.float64(n))) and (rgba[..., 3] == 255).all()


@pytest.mark.parametrize("kind,a,b", POSITIVE)
def test_a_constant_image_stays_constant(pt, kind, a, b):
    for radius in RADII:
        smp = np.full((5, 9, 17, 3), 0.37, np.float32)
        film, _, plain, wsum = pt.filter_host(smp, flt_of(pt, kind, radius, a, b))
        assert (wsum > 0.0).all()
        c = np.float64(np.float32(0.37))
        assert (np.abs(film.astype(np.float64) - c) <= 1e-12 * c + np.spacing(np.float32(0.37)) / 2).all(), radius      # 1e-12 relative in f64, then the one f32 rounding
        assert same(plain, np.full((9, 17, 3), 0.37, np.float32))


def _support(pt, kind, radius, a, b, W, H, x, y, s):
    """the output pixels q whose weight for sample index s of pixel (x, y) is not 0, from the text of the rule"""
    ox, oy = pt.filter_offsets(x, y, s)
    qs = set()
    R = np.float64(np.float32(radius))
    for qy in range(H):
        for qx in range(W):
            tx, ty = (x - qx) + (ox - 0.5), (y - qy) - (oy - 0.5)
            if abs(tx) < R and abs(ty) < R:
                w = fr.weight1(kind, radius, a, b, np.array([abs(tx)]))[0] * fr.weight1(kind, radius, a, b, np.array([abs(ty)]))[0]
                if w != 0.0:
                    qs.add((qx, qy))
    return qs


@pytest.mark.parametrize("kind,a,b", KINDS)
def test_inf_and_nan_reach_exactly_their_support(pt, kind, a, b):
    W, H, n = 17, 9, 3
    for radius in RADII:
        for (x, y, s) in ((8, 4, 1), (0, 0, 0), (16, 8, 2)):
            for bad in (np.inf, np.nan):
                smp = np.full((n, H, W, 3), 0.5, np.float32)
                smp[s, y, x] = bad
                film, _, plain, wsum = pt.filter_host(smp, flt_of(pt, kind, radius, a, b), first_sample=4)
                hit = _support(pt, kind, radius, a, b, W, H, x, y, 4 + s)
                assert (x, y) in hit or kind == fr.MITCHELL
                touched = {(qx, qy) for qy in range(H) for qx in range(W) if not np.isfinite(film[qy, qx]).all()}
                fallback = {(qx, qy) for (qx, qy) in hit if not wsum[qy, qx] > 0.0}      # Wt <= 0: the pixel shows its own plain mean
                assert touched - {(x, y)} == hit - fallback - {(x, y)}, (radius, x, y, bad)
                assert np.isfinite(wsum).all()
                assert not np.isfinite(plain[y, x]).any() and np.isfinite(np.delete(plain.reshape(-1, 3), y * W + x, axis=0)).all()
                if bad is np.inf and kind != fr.MITCHELL:
                    assert all(np.isposinf(film[qy, qx]).all() for (qx, qy) in hit)


def test_a_pixel_without_positive_weight_falls_back_to_the_plain_mean(pt):
    """Mitchell B = 0, C = 1 at n = 1: a sample index is searched for which some pixel's weights sum to <= 0"""
    W, H = 6, 5
    f = flt_of(pt, fr.MITCHELL, 2.0, 0.0, 1.0)
    smp = make_samples(5, 1, W, H, wild=False)
    found = None
    for s in range(4000):
        film, rgba, plain, wsum = pt.filter_host(smp, f, first_sample=s)
        if (wsum <= 0.0).any():
            found = s
            break
    assert found is not None
    bad = wsum <= 0.0
    assert same(film[bad], plain[bad]) and not same(film[~bad], plain[~bad])
    ref = fr.film(smp, fr.MITCHELL, 2.0, 0.0, 1.0, first_sample=found)
    assert all(same(x, y) for x, y in zip((film, rgba, plain, wsum), ref))
    # under Mitchell the film may be negative and is kept; its RGBA8 byte is 0
    neg = film < 0.0
    if neg.any():
        assert (rgba[..., :3][neg] == 0).all()


def test_rule_header_is_clean_under_asan_and_ubsan(tmp_path):
    """tests/tools/filter_san.cpp: a stand-alone program around the host functions of pt_filter.h"""
    exe = str(tmp_path / "filter_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "tools", "filter_san.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "filter_san: 0 failed checks" in out, out[-3000:]
    assert "runtime error" not in out and "AddressSanitizer" not in out, out[-3000:]
