"""The bloom rule on the CPU (pt_bloom_host, pt_debug_bloom_plan, pt_debug_bloom_bright) against the numpy restatement
tests/bloom_ref.py: exports, defaults and refusals, the plan, the bright pass bit for bit, the whole rule against the f64 restatement
under the restatement's own f32-versus-f64 bound, and the rule's properties.  No GPU."""
import ctypes as C
import math

import numpy as np
import pytest

import bloom_ref as br

INVALID = 1                                                     # PT_ERR_INVALID_ARG
PLAN_SIZES = [(2, 2), (3, 2), (2, 7), (5, 3), (17, 33), (33, 17), (63, 65), (64, 64), (96, 80), (130, 70)]


def _pb(pt, p):
    return pt.default_bloom(**p)


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def test_exports_and_defaults(pt):
    lib = pt._lib.lib()
    for name in ("pt_default_bloom", "pt_bloom_device", "pt_bloom_host", "pt_display_device", "pt_display_host", "pt_debug_bloom_plan",
                 "pt_debug_bloom_bright", "pt_debug_bloom_tail"):
        assert hasattr(lib, name), name
    b = pt.default_bloom()
    assert (b.levels, b.threshold, b.knee, b.scatter, b.intensity) == (6, 1.0, 0.5, np.float32(0.7), np.float32(0.05))
    assert math.isinf(b.clamp) and b.clamp > 0
    assert C.sizeof(pt._lib.PtBloom) == 24
    for k, v in br.DEFAULT.items():
        assert np.float32(getattr(b, k)) == np.float32(v), k


BAD_FIELDS = [("levels", 0), ("levels", 9), ("threshold", -0.5), ("threshold", float("nan")), ("threshold", float("inf")),
              ("knee", -1.0), ("knee", float("nan")), ("knee", float("inf")), ("clamp", 0.0), ("clamp", -1.0), ("clamp", float("nan")),
              ("scatter", -0.1), ("scatter", 1.5), ("scatter", float("nan")), ("intensity", -1.0), ("intensity", float("nan")),
              ("intensity", float("inf"))]


def test_every_refusal(pt):
    """PT_ERR_INVALID_ARG from every entry, before a context is looked at (the device entries are called without one, on addresses
    that are never read)"""
    lib = pt._lib.lib()
    film = br.random_hdr(4, 4, 0)
    out = np.empty_like(film)
    rgba = np.empty((4, 4, 4), np.uint8)
    good, tm = pt.default_bloom(), pt.default_tonemap()
    fin, fout, f8 = _ptr(film), _ptr(out), _ptr(rgba)
    odd = C.c_void_p(film.ctypes.data + 1)

    def entries(W, H, src, bl, dst):
        yield lib.pt_bloom_host(W, H, src, bl, dst)
        yield lib.pt_bloom_device(None, W, H, src, bl, dst)
        if bl is not None:                                     # (a null bloom is pt_display_device's "no bloom stage")
            yield lib.pt_display_device(None, W, H, src, bl, C.byref(tm), dst, f8)
            yield lib.pt_display_host(None, W, H, src, bl, C.byref(tm), dst, f8)

    cases = [(4, 4, None, C.byref(good), fout), (4, 4, fin, None, fout), (4, 4, odd, C.byref(good), fout),
             (1, 4, fin, C.byref(good), fout), (4, 1, fin, C.byref(good), fout), (1 << 16, (1 << 14) + 1, fin, C.byref(good), fout)]
    for name, v in BAD_FIELDS:
        cases.append((4, 4, fin, C.byref(pt.default_bloom(**{name: v})), fout))
    for case in cases:
        for rc in entries(*case):
            assert rc == INVALID, (case[:2], rc)
    # the output plane of the bloom entries proper: null, misaligned
    for dst in (None, C.c_void_p(out.ctypes.data + 2)):
        assert lib.pt_bloom_host(4, 4, fin, C.byref(good), dst) == INVALID
        assert lib.pt_bloom_device(None, 4, 4, fin, C.byref(good), dst) == INVALID
    # the display entry also refuses what the tone mapper refuses, and a null RGBA8 plane
    assert lib.pt_display_device(None, 4, 4, fin, C.byref(good), None, fout, f8) == INVALID
    assert lib.pt_display_device(None, 4, 4, fin, C.byref(good), C.byref(tm), fout, None) == INVALID
    assert lib.pt_display_device(None, 4, 4, fin, C.byref(good), C.byref(pt.default_tonemap(curve=7)), fout, f8) == INVALID
    # valid arguments, no context: still a refusal, not a crash
    assert lib.pt_bloom_device(None, 4, 4, fin, C.byref(good), fout) == INVALID
    assert lib.pt_display_device(None, 4, 4, fin, C.byref(good), C.byref(tm), fout, f8) == INVALID
    assert lib.pt_debug_bloom_tail(None, 0) == INVALID
    # the debug entries
    wh, n, ft = np.zeros(16, np.uint32), C.c_uint32(0), C.c_uint32(0)
    for W, H, lv in [(1, 8, 3), (8, 1, 3), (8, 8, 0), (8, 8, 9)]:
        assert lib.pt_debug_bloom_plan(W, H, lv, wh.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(n), C.byref(ft)) == INVALID
    assert lib.pt_debug_bloom_plan(8, 8, 3, None, C.byref(n), C.byref(ft)) == INVALID
    assert lib.pt_debug_bloom_bright(None, fin, fout) == INVALID
    assert lib.pt_debug_bloom_bright(C.byref(pt.default_bloom(knee=-1.0)), fin, fout) == INVALID
    # and a good call goes through
    assert lib.pt_bloom_host(4, 4, fin, C.byref(good), fout) == 0


@pytest.mark.parametrize("W,H", PLAN_SIZES)
def test_plan_against_the_restatement(pt, W, H):
    for levels in range(1, 9):
        assert pt.bloom_plan(W, H, levels) == br.plan(W, H, levels), (W, H, levels)


def test_plan_shapes_the_tests_rely_on(pt):
    assert pt.bloom_plan(64, 64, 8) == ([(32, 32), (16, 16), (8, 8), (4, 4), (2, 2), (1, 1)], 0)
    assert pt.bloom_plan(96, 80, 8)[1] == 1 and pt.bloom_plan(2, 2, 8) == ([(1, 1)], 0)
    assert pt.bloom_plan(1024, 1024, 8)[1] == 4 and pt.bloom_plan(1024, 1024, 2)[1] == 2       # no level small enough: no tail
    lv, ft = pt.bloom_plan(257, 31, 8)
    assert lv[0] == (129, 16) and ft == 3 and lv[-1] == (2, 1) and len(lv) == 8


def test_bright_pass_on_the_knee_points_bit_for_bit(pt):
    for p in br.PARAM_SETS + [br.params(threshold=1.0, knee=0.5, clamp=1.25), br.params(knee=0.0)]:
        T, k = p["threshold"], p["knee"]
        film = np.concatenate([br.knee_film(9, 1, T, k if k > 0 else 0.5), br.specials(8, 1), br.random_hdr(16, 1, 5)], axis=1)
        ref = br.bright(film[0].astype(np.float32), p, np.float32)
        b = _pb(pt, p)
        for px, want in zip(film[0], ref):
            got = pt.bloom_bright(b, px)
            assert br.same_bits(got, want), (p, px, got, want)
    # the points themselves: nothing at T - k, the knee's quarter at T, the full excess at T + k
    b = pt.default_bloom()
    v = [br.grey_with_lum(t) for t in (0.5, 1.0, 1.5)]
    assert np.all(pt.bloom_bright(b, [v[0]] * 3) == 0)
    assert br.lum(pt.bloom_bright(b, [v[1]] * 3), np.float32) == pytest.approx(0.125, rel=1e-6)
    assert br.lum(pt.bloom_bright(b, [v[2]] * 3), np.float32) == pytest.approx(0.5, rel=1e-6)


def _bound(film, p):
    """the restatement in f64, and its largest absolute difference from itself in f32 over the finite pixels"""
    r64, r32 = br.bloom(film, p, np.float64), br.bloom(film, p, np.float32)
    fin = np.isfinite(r64) & np.isfinite(r32)
    assert br.same(np.where(fin, 0, r64), np.where(fin, 0, r32.astype(np.float64)))     # the same pixels are non-finite, the same way
    return r64, (float(np.abs(r32[fin].astype(np.float64) - r64[fin]).max()) if fin.any() else 0.0)


@pytest.mark.parametrize("W,H", br.SIZES)
def test_host_against_the_f64_restatement(pt, W, H):
    """Every pixel, NaN = NaN.  The bar is 4 x the restatement's own f32-versus-f64 difference on the same input (the factor for a
    summation order inside a pass that may differ from numpy's).  Measured, relative to the film's largest finite value: the bound
    itself is at most 8.65e-8 (17 x 33; 6.4e-8 to 8.4e-8 at the other sizes) and the host's difference from f64 equals it -- the host
    equals the f32 restatement bit for bit on every case here (docs/EXPERIMENTS.md, "Bloom")."""
    worst = (0.0, 0.0)
    for name, film in br.crafted(W, H).items():
        top = float(np.abs(film[np.isfinite(film)]).max())
        for levels in br.LEVELS:
            for p in br.PARAM_SETS:
                p = dict(p, levels=levels)
                ref, bound = _bound(film, p)
                got = pt.bloom_host(film, _pb(pt, p))
                fin = np.isfinite(ref)
                assert br.same(np.where(fin, 0, got.astype(np.float64)), np.where(fin, 0, ref)), (name, levels)
                err = float(np.abs(got[fin].astype(np.float64) - ref[fin]).max()) if fin.any() else 0.0
                worst = max(worst, (bound / top, err / top))
                assert err <= 4 * bound, (name, levels, p, err, bound)
    print(f"{W}x{H}: largest f32-vs-f64 bound {worst[0]:.3e}, host-vs-f64 there {worst[1]:.3e} (relative to the film's largest value)")


def test_no_bloom_term_copies_the_film_bit_for_bit(pt):
    film = br.specials(17, 33)
    for p in (br.params(threshold=1e9, knee=0.0), br.params(intensity=0.0), br.params(threshold=1e9, knee=0.5, levels=1)):
        assert br.same_bits(pt.bloom_host(film, _pb(pt, p)), film)
    assert np.signbit(film).any() and np.isnan(film).any()


def test_impulse_energy(pt):
    """sum(out - in) = intensity sum(b): power-of-two sides, a support away from the borders, T = 0, k = 0.  The bar is the
    restatement's f32-versus-f64 difference of the same sum, times 4 as above (0 where every product is dyadic: s = 0 and 1)."""
    film = br.impulse(64, 64)
    for levels in (1, 2, 3, 4):
        for s in (0.0, 0.3, 1.0):
            p = br.params(levels=levels, threshold=0.0, knee=0.0, scatter=s, intensity=0.25)
            out64, b64 = br.bloom(film, p, np.float64, parts=True)
            want = 0.25 * b64.sum()
            assert abs((out64 - film).sum() - want) <= 1e-12 * want                  # the rule's own consequence, in f64
            out32 = br.bloom(film, p, np.float32)
            bar = 4 * abs((out32.astype(np.float64) - film).sum() - (out64 - film).sum())
            got = pt.bloom_host(film, _pb(pt, p))
            err = abs((got.astype(np.float64) - film).sum() - want)
            print(f"levels {levels} s {s}: sum error {err:.3e}, bar {bar:.3e}")
            assert err <= bar + 1e-12 * want, (levels, s, err, bar)


def test_constant_film_is_exact(pt):
    p = br.params(threshold=0.0, knee=0.0, scatter=0.5, intensity=0.25)
    for W, H in ((64, 64), (17, 33)):
        for levels in (1, 3, 8):
            got = pt.bloom_host(br.constant(W, H), _pb(pt, dict(p, levels=levels)))
            assert np.all(got == np.float32(0.5 * 1.25)), (W, H, levels)


def test_a_nan_pixel_stays_alone(pt):
    film = br.random_hdr(17, 33, 8)
    zero = film.copy()
    zero[16, 8] = 0.0
    film[16, 8] = np.nan
    p = br.params(threshold=0.25, intensity=0.5)
    got, ref = pt.bloom_host(film, _pb(pt, p)), pt.bloom_host(zero, _pb(pt, p))
    assert np.isnan(got[16, 8]).all()
    got[16, 8] = ref[16, 8]
    assert np.isfinite(got).all() and br.same_bits(got, ref)
