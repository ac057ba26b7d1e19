"""Auto-exposure and tone mapping (pt_tonemap_device) without a GPU: the argument checks through the C ABI, the
pinned defaults, the shared header (pathtrace_amd/csrc/pt_tonemap.h) through its host debug entries and under the
sanitizers, and the numpy restatement (tests/tonemap_ref.py) against cases worked out by hand."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import tonemap_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = C.c_void_p(0x1000)         # an aligned address no check may read
ODD = C.c_void_p(0x1002)
SHAPES = [(2, 2), (67, 35), (257, 3), (130, 129)]
CURVE_SEEDS = [0, 1, 2, 3]


def _refused(pt, rc, part):
    assert rc == 1, rc                                            # PT_ERR_INVALID_ARG
    msg = pt._lib.lib().pt_last_error().decode()
    assert part in msg, msg


def test_defaults_are_pinned(pt):
    t = pt.default_tonemap()
    assert (t.mode, t.curve, t.transfer) == (pt._lib.PT_EXPOSURE_AUTO, pt._lib.PT_CURVE_ACES, pt._lib.PT_TRANSFER_SQRT)
    f32 = lambda v: float(np.float32(v))
    assert (t.ev, t.key, t.pct_lo, t.pct_hi) == (0.0, f32(0.18), 0.5, f32(0.95))
    assert (t.log2_min, t.log2_max, t.adapt, t.white) == (-8.0, 8.0, f32(0.1), 4.0)
    assert C.sizeof(pt._lib.PtTonemap) == 44
    assert pt.default_tonemap(curve="reinhard", mode="manual", ev=1.5).curve == pt._lib.PT_CURVE_REINHARD
    assert {k: tr.params()[k] for k in ("key", "adapt", "pct_hi")} == {"key": t.key, "adapt": t.adapt, "pct_hi": t.pct_hi}


def test_tonemap_refuses_bad_arguments_without_a_device(pt):
    """every check comes before the context is looked at: a null context and addresses nothing may read"""
    L = pt._lib.lib()
    who = "pt_tonemap_device"
    ok = pt.default_tonemap()
    call = lambda tm=ok, w=8, h=8, lin=FAKE, out=FAKE, rgba=FAKE: L.pt_tonemap_device(None, w, h, lin, C.byref(tm) if tm else None, out, rgba)
    _refused(pt, call(lin=None), who + ": null argument")
    _refused(pt, call(rgba=None), who + ": null argument")
    _refused(pt, call(tm=None), who + ": null argument")
    _refused(pt, call(lin=ODD), "4-byte aligned")
    _refused(pt, call(out=ODD), "4-byte aligned")
    _refused(pt, call(rgba=ODD), "4-byte aligned")
    _refused(pt, call(w=1), "image 1x8")
    _refused(pt, call(h=0), "image 8x0")
    for field, bad, part in [("mode", 2, "unknown mode 2"), ("curve", 3, "unknown curve 3"), ("transfer", 2, "unknown transfer 2"),
                             ("ev", float("nan"), "ev must be finite"), ("ev", float("inf"), "ev must be finite"),
                             ("pct_lo", -0.1, "pct_lo"), ("pct_hi", 1.5, "pct_hi"), ("pct_lo", float("nan"), "pct_lo"),
                             ("pct_lo", 0.97, "pct_lo"),                       # above pct_hi = 0.95
                             ("key", 0.0, "key and white"), ("key", float("inf"), "key and white"), ("key", float("nan"), "key and white"),
                             ("white", -1.0, "key and white"), ("white", float("nan"), "key and white"),
                             ("adapt", 1.01, "adapt"), ("adapt", -0.5, "adapt"), ("adapt", float("nan"), "adapt"),
                             ("log2_min", 9.0, "log2_min")]:
        _refused(pt, call(tm=pt.default_tonemap(**{field: bad})), part)
    # an optional float plane, a window without width and equal bounds are arguments like any other: only the context is missing
    _refused(pt, call(out=None), who + ": null context")
    _refused(pt, call(tm=pt.default_tonemap(pct_lo=0.5, pct_hi=0.5, log2_min=1.0, log2_max=1.0)), who + ": null context")
    _refused(pt, call(w=2, h=2), who + ": null context")


def test_histogram_and_state_entries_refuse_bad_arguments_without_a_device(pt):
    L = pt._lib.lib()
    who = "pt_film_histogram_device"
    _refused(pt, L.pt_film_histogram_device(None, 8, 8, None, FAKE), who + ": null argument")
    _refused(pt, L.pt_film_histogram_device(None, 8, 8, FAKE, None), who + ": null argument")
    _refused(pt, L.pt_film_histogram_device(None, 8, 8, ODD, FAKE), "4-byte aligned")
    _refused(pt, L.pt_film_histogram_device(None, 8, 8, FAKE, ODD), "4-byte aligned")
    _refused(pt, L.pt_film_histogram_device(None, 8, 1, FAKE, FAKE), "image 8x1")
    _refused(pt, L.pt_film_histogram_device(None, 8, 8, FAKE, FAKE), who + ": null context")
    _refused(pt, L.pt_exposure_reset(None), "pt_exposure_reset: null context")
    v = C.c_double(0)
    _refused(pt, L.pt_exposure_get(None, C.byref(v), None), "pt_exposure_get: null argument")
    _refused(pt, L.pt_tonemap_host(None, 8, 8, None, C.byref(pt.default_tonemap()), None, FAKE), "pt_tonemap_host: null argument")


def test_bins_of_exact_powers_of_two(pt):
    """the shared header through pt_debug_tonemap_bin, and the restatement, on the boundaries of the rule"""
    f = np.float32
    below = lambda v: np.nextafter(f(v), f(0))
    cases = [(f(2.0 ** -16), 0), (below(2.0 ** -16), tr.DARK), (f(1.0), 128), (below(1.0), 127), (f(2.0 ** 16), 255), (below(2.0 ** 16), 255),
             (f(2.0 ** 15), 248), (f(2.0 ** -15), 8), (f(1.125), 129), (f(3.0e38), 255), (f(0.0), tr.DARK), (f(-0.0), tr.DARK), (f(-1.0), tr.DARK),
             (f(1e-40), tr.DARK), (f(np.nan), tr.INVALID), (f(np.inf), tr.INVALID), (f(-np.inf), tr.INVALID)]
    L = pt._lib.lib()
    for v, want in cases:
        assert L.pt_debug_tonemap_bin(float(v)) == want, (v, want)
        assert tr.words(np.array([v]))[0] == want, (v, want)
    # the two agree on every eighth of every octave, on its neighbours, and on random bit patterns
    rng = np.random.default_rng(5)
    grid = (2.0 ** (np.arange(-20 * 8, 20 * 8 + 1) / 8.0)).astype(np.float32)
    vals = np.concatenate([grid, np.nextafter(grid, f(0)), np.nextafter(grid, f(np.inf)), rng.integers(0, 2 ** 32, 4000, dtype=np.uint64).astype(np.uint32).view(np.float32)])
    got = np.array([L.pt_debug_tonemap_bin(C.c_float(float(v)) if np.isfinite(v) else float(v)) for v in vals])
    keep = ~np.isnan(vals)                                         # (a NaN's payload does not survive the way through a Python float)
    assert np.array_equal(got[keep], tr.words(vals)[keep])
    assert (got[~keep] == tr.INVALID).all()


def test_a_film_of_powers_of_two_lands_on_the_boundaries():
    """a small film by hand: the invalid, dark and bin words and their sum.  (The three weights do not add up to 1 in f32, so a
    grey pixel of value 1 has L = 1 or the f32 below it: the bin boundaries themselves are pinned on L in the test above.)"""
    film = np.zeros((4, 4, 3), dtype=np.float32)
    film[0, 0] = np.nan; film[0, 1] = np.inf; film[0, 2] = -1.0; film[0, 3] = (1.0, 1.0, 1.0)
    film[1] = 2.0 ** -20
    h = tr.histogram(film)
    assert h.sum() == 16 and h[tr.INVALID] == 2 and h[tr.DARK] == 1 + 4 + 8
    L1 = tr.luminance_f32(np.array([[1.0, 1.0, 1.0]]))[0]
    assert h[tr.words(np.array([L1]))[0]] == 1 and tr.words(np.array([L1]))[0] in (127, 128)


def test_metering_of_a_two_value_film_by_hand(pt):
    """100 pixels in bin 128 (centre z = 0.0625) and 300 in bin 160 (z = 4.0625), N = 400.
    Window 0.5 .. 0.95: ranks 200 .. 380, all inside bin 160 (ranks 100 .. 400): m = 4.0625.
    Window 0 .. 0.5: ranks 0 .. 200: 100 of bin 128, 100 of bin 160: m = (100 * 0.0625 + 100 * 4.0625) / 200 = 2.0625.
    Window 0.2 .. 0.3: ranks 80 .. 120: 20 of bin 128 and 20 of bin 160: m = 2.0625.
    Window 0.25 .. 0.25 (no width): rank 100: the first bin whose ranks end at or behind it is bin 128: m = 0.0625."""
    hist = np.zeros(tr.WORDS, dtype=np.uint32)
    hist[128], hist[160], hist[tr.DARK], hist[tr.INVALID] = 100, 300, 50, 3
    lg = np.log2(float(np.float32(0.18)))
    for lo, hi, m in [(0.5, 0.95, 4.0625), (0.0, 0.5, 2.0625), (0.25, 0.25, 0.0625)]:
        p = tr.params(pct_lo=lo, pct_hi=hi)
        assert tr.target(hist, p) == pytest.approx(lg - m, abs=1e-13)
        got = pt._lib.lib().pt_debug_tonemap_meter(hist.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(pt.default_tonemap(pct_lo=lo, pct_hi=hi)), 1, 0.0)
        assert got == pytest.approx(lg - m, abs=1e-12)
    p = tr.params(pct_lo=0.2, pct_hi=0.3)            # (0.2f, 0.3f are not the decimals: within their rounding)
    assert tr.target(hist, p) == pytest.approx(lg - 2.0625, abs=1e-5)
    # the clamp, the black frame, the adaptation
    assert tr.target(hist, tr.params(log2_min=-1.0, log2_max=1.0)) == -1.0
    black = np.zeros(tr.WORDS, dtype=np.uint32); black[tr.DARK] = 400
    assert tr.target(black, tr.params()) == 0.0 and tr.target(black, tr.params(), prev=2.5) == 2.5
    p = tr.params(adapt=0.5)
    assert tr.adapt(hist, p, prev=0.0) == pytest.approx(0.5 * (lg - 4.0625), abs=1e-13)
    tm = pt.default_tonemap(adapt=0.5)
    hp = hist.ctypes.data_as(C.POINTER(C.c_uint32))
    assert pt._lib.lib().pt_debug_tonemap_meter(hp, C.byref(tm), 0, 0.0) == pytest.approx(0.5 * (lg - 4.0625), abs=1e-12)
    assert pt._lib.lib().pt_debug_tonemap_meter(black.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(tm), 0, 2.5) == 2.5


@pytest.mark.parametrize("W,H", SHAPES[1:])
def test_header_metering_is_the_restatement_on_the_test_films(pt, W, H):
    for film in (tr.crafted_film(W, H, 11), tr.curve_film(W, H, 2)):
        hist = tr.histogram(film)
        assert hist.sum() == W * H
        for seed in (None, 0, 1):
            over = tr.random_params(seed) if seed is not None else {}
            tm = pt.default_tonemap(**over)
            got = pt._lib.lib().pt_debug_tonemap_meter(hist.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(tm), 1, 0.0)
            assert abs(got - tr.target(hist, tr.params(**over))) <= 1e-12


def _pixel(pt, tm, E, rgb):
    y = (C.c_float * 3)()
    q = (C.c_uint8 * 4)()
    assert pt._lib.lib().pt_debug_tonemap_pixel(C.byref(tm), float(E), (C.c_float * 3)(*[float(v) for v in rgb]), y, q) == 0
    return np.array(y[:], dtype=np.float32), np.array(q[:], dtype=np.uint8)


def test_curves_and_transfers_by_hand(pt):
    # clamp + sqrt at E = 1 is the render's transform: 0.25 -> sqrt = 0.5 -> 127
    y, q = _pixel(pt, pt.default_tonemap(curve="clamp"), 1.0, (0.25, 4.0, 0.0))
    assert list(y) == [0.25, 4.0, 0.0] and list(q) == [127, 255, 0, 255]
    # Reinhard: grey x = white maps to 1: (1 + 4/16) * 4 / 5 = 1 with white = 4
    y, q = _pixel(pt, pt.default_tonemap(curve="reinhard", transfer="srgb"), 2.0, (2.0, 2.0, 2.0))
    assert np.allclose(y, 1.0, rtol=1e-6) and list(q[:3]) in ([255] * 3, [254] * 3)
    # ACES at x = 1: 2.54 / 3.16
    y, _ = _pixel(pt, pt.default_tonemap(), 1.0, (1.0, 1.0, 1.0))
    assert np.allclose(y, 2.54 / 3.16, rtol=1e-6)
    # sRGB: 0.5 -> 1.055 * 0.5^(1/2.4) - 0.055 = 0.735357 -> 187; the linear toe: 0.002 -> 0.02584 -> 6
    _, q = _pixel(pt, pt.default_tonemap(curve="clamp", transfer="srgb"), 1.0, (0.5, 0.002, 1.0))
    assert list(q) == [187, 6, 255, 255]
    # a NaN channel is 0 on both planes; an overflowing one saturates
    for curve in ("clamp", "aces"):
        y, q = _pixel(pt, pt.default_tonemap(curve=curve), 1.0, (np.nan, 0.5, 3e38))
        assert y[0] == 0.0 and q[0] == 0 and q[2] == 255 and y[1] > 0
    y, q = _pixel(pt, pt.default_tonemap(curve="reinhard"), 1.0, (np.nan, 0.5, 0.5))
    assert list(y) == [0.0, 0.0, 0.0] and list(q) == [0, 0, 0, 255]


@pytest.mark.parametrize("W,H", SHAPES)
@pytest.mark.parametrize("seed", CURVE_SEEDS)
def test_margin_unsafe_pixels_stay_under_the_cap_and_the_header_meets_the_bars(pt, W, H, seed):
    """What tests/test_gpu_tonemap.py compares on the device, here with the header's functions as the host compiler builds
    them: for the committed seeds at most 2 % of the pixels of any compared image are margin-unsafe in the restatement
    alone, the float plane is within 1e-4 (floor 1e-3) of it, RGBA8 equal on the safe pixels and within 1 LSB elsewhere."""
    film = tr.curve_film(W, H, seed)
    over = tr.random_params(seed) if seed else {}
    E = np.float32(2.0 ** tr.target(tr.histogram(film), tr.params(**over)))
    for curve in (tr.CLAMP, tr.REINHARD, tr.ACES):
        for transfer in (tr.SQRT, tr.SRGB):
            p = tr.params(curve=curve, transfer=transfer, **over)
            y = tr.curve(film, E, p)
            ref8, safe = tr.rgba8(y, p)
            assert (~safe).mean() <= 0.02, (curve, transfer, (~safe).mean())
            if W * H > 600:
                continue                                           # (one ctypes call per pixel: the small shapes suffice here)
            tm = pt.default_tonemap(curve=curve, transfer=transfer, **over)
            for iy in range(H):
                for ix in range(W):
                    gy, g8 = _pixel(pt, tm, E, film[iy, ix])
                    assert np.all(np.abs(gy - y[iy, ix]) <= 1e-4 * np.maximum(np.abs(y[iy, ix]), 1e-3))
                    d = np.abs(g8.astype(int) - ref8[iy, ix].astype(int)).max()
                    assert d == 0 if safe[iy, ix] else d <= 1


def test_header_is_clean_under_asan_and_ubsan(tmp_path):
    """tests/tools/tonemap_san.cpp: a stand-alone program around the host functions of pt_tonemap.h"""
    exe = str(tmp_path / "tonemap_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "tools", "tonemap_san.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "tonemap_san: 0 failed checks" in out, out[-3000:]
    assert "runtime error" not in out and "AddressSanitizer" not in out, out[-3000:]
