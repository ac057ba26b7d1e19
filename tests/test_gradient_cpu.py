"""Temporal gradients without a device: the ABI (symbols, defaults, the argument checks that need no context), the rule of
pathtrace_amd/csrc/pt_gradient.h compiled with the host compiler exactly as the kernels include it against the numpy
restatement (tests/gradient_ref.py) bit for bit, and the alpha restatement against tests/motion_ref.py."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import gradient_ref as gr
import motion_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pt_temporal_gradient_device", "pt_denoise_temporal_alpha_device", "pt_render_denoised_gradient", "pt_debug_gradient_strata")
SRC = r"""
#include "pt_gradient.h"
extern "C" void gr_pixels(unsigned W, unsigned H, unsigned seed, unsigned* xy) {
    const unsigned SW = ptgr::strata(W), SH = ptgr::strata(H);
    for (unsigned by = 0; by < SH; ++by)
        for (unsigned bx = 0; bx < SW; ++bx) ptgr::stratum_pixel(bx, by, W, H, seed, xy + 2 * (by * SW + bx), xy + 2 * (by * SW + bx) + 1);
}
extern "C" void gr_records(const float* c_new, const float* c_old, unsigned n, double* rec) {
    for (unsigned s = 0; s < n; ++s) ptgr::stratum_record(c_new + 3 * s, c_old + 3 * s, rec + 2 * s);
}
extern "C" void gr_plane(const double* rec, unsigned W, unsigned H, unsigned radius, float scale, float alpha_min, float* out) {
    for (unsigned y = 0; y < H; ++y)
        for (unsigned x = 0; x < W; ++x) out[y * W + x] = ptgr::pixel_alpha(rec, ptgr::strata(W), ptgr::strata(H), x, y, radius, scale, alpha_min);
}
"""
SIZES = ((2, 2), (3, 3), (4, 4), (7, 5), (16, 11))
RADII = (0, 1, 2, 8)


def test_the_new_symbols_are_exported_and_the_defaults(pt):
    lib = pt._lib.lib()
    for name in NEW + ("pt_default_gradient",):
        assert name in pt._lib.SYMBOLS and hasattr(lib, name), name
    assert lib.pt_abi_version() == 6
    header = open(os.path.join(ROOT, "include", "pathtrace_amd.h")).read()
    for name in NEW:
        assert f"int {name}(" in header, name
    g = pt.default_gradient()
    assert (g.radius, g.scale) == (1, 1.0)
    assert C.sizeof(pt._lib.PtGradient) == 8
    lib.pt_default_gradient(None)                               # a null output is ignored
    for name in ("temporal_gradient", "denoise_temporal_alpha", "render_denoised_gradient"):
        assert hasattr(pt.Context, name)
    hpp = open(os.path.join(ROOT, "pathtrace_amd", "host", "pathtrace.hpp")).read()
    assert "void render_denoised_gradient(" in hpp and "pt_render_denoised_gradient(" in hpp


def test_null_and_misaligned_arguments_are_refused_without_a_device(pt):
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
    grad = lib.pt_temporal_gradient_device
    # no context
    assert grad(None, R(cam), R(prm), 0, ok, R(g), 0.2, out) == 1
    assert b"pt_temporal_gradient_device" in lib.pt_last_error() and b"null" in lib.pt_last_error()
    for args in ((None, R(prm), 0, ok, R(g), 0.2, out), (R(cam), None, 0, ok, R(g), 0.2, out), (R(cam), R(prm), 0, None, R(g), 0.2, out),
                 (R(cam), R(prm), 0, ok, None, 0.2, out), (R(cam), R(prm), 0, ok, R(g), 0.2, None)):
        assert grad(fake, *args) == 1
        assert b"null" in lib.pt_last_error()
    assert grad(fake, R(cam), R(prm), 0, odd4, R(g), 0.2, out) == 1 and b"aligned" in lib.pt_last_error()
    assert grad(fake, R(cam), R(prm), 0, ok, R(g), 0.2, odd4) == 1 and b"aligned" in lib.pt_last_error()
    banded = pt.default_params(spp=2, band_rows=2, band_count=2)
    assert grad(fake, R(cam), R(banded), 0, ok, R(g), 0.2, out) == 1 and b"band_count" in lib.pt_last_error()
    assert grad(fake, R(cam), R(pt.default_params(spp=2)), 0, ok, R(pt.default_gradient(radius=9)), 0.2, out) == 1
    assert b"radius" in lib.pt_last_error()
    assert grad(fake, R(cam), R(prm), 0, ok, R(pt.default_gradient(radius=8)), 2.0, out) == 1 and b"alpha_min" in lib.pt_last_error()
    for s in (-1.0, math.nan, math.inf, -math.inf):
        assert grad(fake, R(cam), R(prm), 0, ok, R(pt.default_gradient(scale=s)), 0.2, out) == 1 and b"scale" in lib.pt_last_error()
    for a in (-0.1, 1.5, math.nan, math.inf):
        assert grad(fake, R(cam), R(prm), 0, ok, R(g), a, out) == 1 and b"alpha_min" in lib.pt_last_error()
    for w, h in ((1, 8), (8, 1), (1, 1), (0, 0)):
        small = pt._lib.PtCamera.from_buffer_copy(cam)
        small.width, small.height = w, h
        assert grad(fake, R(small), R(prm), 0, ok, R(g), 0.2, out) == 1 and b">= 2" in lib.pt_last_error()
    # the alpha entry: the motion entry's checks and the plane's
    alpha = lib.pt_denoise_temporal_alpha_device
    assert alpha(None, R(cam), ok, ok, ok, ok, R(dn), R(tp), out, None) == 1 and b"null context" in lib.pt_last_error()
    assert alpha(fake, R(cam), ok, ok, ok, None, R(dn), R(tp), out, None) == 1 and b"null argument" in lib.pt_last_error()
    assert alpha(fake, R(cam), ok, ok, None, ok, R(dn), R(tp), out, None) == 1 and b"null argument" in lib.pt_last_error()
    assert alpha(fake, R(cam), ok, ok, ok, odd4, R(dn), R(tp), out, None) == 1 and b"d_alpha" in lib.pt_last_error()
    assert alpha(fake, R(cam), ok, odd16, ok, ok, R(dn), R(tp), out, None) == 1 and b"16-byte" in lib.pt_last_error()
    # the one call
    one = lib.pt_render_denoised_gradient
    assert one(None, R(cam), R(prm), 2, R(dn), R(tp), R(g), buf, None, None, None, None, None) == 1 and b"null" in lib.pt_last_error()
    for args in ((None, R(prm), 2, R(dn), R(tp), R(g), buf), (R(cam), None, 2, R(dn), R(tp), R(g), buf), (R(cam), R(prm), 2, None, R(tp), R(g), buf),
                 (R(cam), R(prm), 2, R(dn), None, R(g), buf), (R(cam), R(prm), 2, R(dn), R(tp), None, buf), (R(cam), R(prm), 2, R(dn), R(tp), R(g), None)):
        assert one(fake, *args, None, None, None, None, None) == 1 and b"null" in lib.pt_last_error()
    assert one(fake, R(cam), R(prm), 0, R(dn), R(tp), R(g), buf, None, None, None, None, None) == 1 and b"feature_samples" in lib.pt_last_error()
    assert one(fake, R(cam), R(banded), 2, R(dn), R(tp), R(g), buf, None, None, None, None, None) == 1 and b"band_count" in lib.pt_last_error()
    assert one(fake, R(cam), R(prm), 2, R(dn), R(tp), R(pt.default_gradient(radius=9)), buf, None, None, None, None, None) == 1
    assert b"radius" in lib.pt_last_error()
    assert lib.pt_debug_gradient_strata(None, 8, 8, None, None, None) == 1


# ---------------------------------------------------------------- the rule of pt_gradient.h
@pytest.fixture(scope="module")
def rule(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("grrule")
    (d / "rule.cpp").write_text(SRC)
    so = d / "rule.so"
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-I",
                           os.path.join(ROOT, "pathtrace_amd", "csrc"), str(d / "rule.cpp"), "-o", str(so)])
    lib = C.CDLL(str(so))
    lib.gr_pixels.argtypes = [C.c_uint, C.c_uint, C.c_uint, C.c_void_p]
    lib.gr_records.argtypes = [C.c_void_p, C.c_void_p, C.c_uint, C.c_void_p]
    lib.gr_plane.argtypes = [C.c_void_p, C.c_uint, C.c_uint, C.c_uint, C.c_float, C.c_float, C.c_void_p]

    class Rule:
        @staticmethod
        def pixels(W, H, seed):
            SW, SH = gr.strata_shape(W, H)
            xy = np.zeros((SH, SW, 2), np.uint32)
            lib.gr_pixels(W, H, seed, xy.ctypes.data)
            return xy

        @staticmethod
        def records(c_new, c_old):
            c_new, c_old = np.ascontiguousarray(c_new, np.float32), np.ascontiguousarray(c_old, np.float32)
            rec = np.zeros(c_new.shape[:-1] + (2,), np.float64)
            lib.gr_records(c_new.ctypes.data, c_old.ctypes.data, rec.size // 2, rec.ctypes.data)
            return rec

        @staticmethod
        def plane(rec, W, H, radius, scale, alpha_min):
            rec = np.ascontiguousarray(rec, np.float64)
            out = np.zeros((H, W), np.float32)
            lib.gr_plane(rec.ctypes.data, W, H, radius, scale, alpha_min, out.ctypes.data)
            return out
    return Rule


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    u = np.uint32 if a.dtype == np.float32 else np.uint64
    return a.shape == b.shape and a.dtype == b.dtype and bool(np.all((a.view(u) == b.view(u)) | (np.isnan(a) & np.isnan(b))))


def _films(rng, W, H):
    SW, SH = gr.strata_shape(W, H)
    old = rng.exponential(0.5, (SH, SW, 3)).astype(np.float32)
    new = old.copy()
    m = rng.random((SH, SW)) < 0.5
    new[m] = rng.exponential(0.5, (int(m.sum()), 3)).astype(np.float32)
    return new, old


def test_strata_geometry(rule):
    for W, H in SIZES:
        SW, SH = gr.strata_shape(W, H)
        assert (SW, SH) == (math.ceil(W / 3), math.ceil(H / 3))
        clipped = False
        for seed in list(range(9)) + [9, 17, 2 ** 32 - 1]:
            xy = rule.pixels(W, H, seed)
            assert np.array_equal(xy, gr.stratum_pixels(W, H, seed)), (W, H, seed)
            assert (xy[..., 0] < W).all() and (xy[..., 1] < H).all()
            assert (xy[..., 0] // 3 == np.arange(SW)[None, :]).all() and (xy[..., 1] // 3 == np.arange(SH)[:, None]).all()   # inside its own block
            clipped |= bool((xy[-1, -1] != (3 * (SW - 1) + seed % 3, 3 * (SH - 1) + (seed // 3) % 3)).any())
        assert clipped == (W % 3 != 0 or H % 3 != 0)            # a clipped gradient pixel at the right / bottom edge
        # the nine seeds walk through every pixel of an unclipped block
        assert {tuple(rule.pixels(W, H, s)[0, 0]) for s in range(9)} == {(x, y) for x in range(min(3, W)) for y in range(min(3, H))}
    assert gr.strata_shape(2, 2) == (1, 1) and gr.strata_shape(3, 3) == (1, 1)      # a single stratum


def test_records_and_plane_against_the_restatement(rule):
    rng = np.random.default_rng(41)
    raised = 0
    for W, H in SIZES:
        new, old = _films(rng, W, H)
        rec = rule.records(new, old)
        assert _same_bits(rec, gr.records(new, old))
        assert (rec[..., 0] >= 0).all() and (rec[..., 1] >= rec[..., 0]).all()
        for radius in RADII:                                    # 8 is wider than every strata grid here
            for scale, amin in ((1.0, 0.2), (0.5, 0.0), (3.0, 0.05), (0.0, 0.2), (1e30, 0.2), (1.0, 1.0)):
                got = rule.plane(rec, W, H, radius, scale, amin)
                assert _same_bits(got, gr.alpha_plane(rec, W, H, radius, scale, amin)), (W, H, radius, scale, amin)
                assert (got >= np.float32(amin)).all() and (got <= 1).all()
                if scale == 0.0:
                    assert _same_bits(got, np.full((H, W), amin, np.float32))                 # scale 0: lambda 0
                if scale == 1e30:
                    D = gr.window_sums(rec, W, H, radius)[0]
                    assert _same_bits(got[D > 0], np.ones(int((D > 0).sum()), np.float32))   # saturated
                raised += int((got > np.float32(amin)).sum())
    assert raised > 1000


def test_no_change_gives_alpha_min_exactly(rule):
    rng = np.random.default_rng(42)
    for W, H in SIZES:
        _, old = _films(rng, W, H)
        rec = rule.records(old, old)
        assert (rec[..., 0] == 0).all() and _same_bits(rec[..., 1], gr.luminance(old))
        for radius in RADII:
            for amin in (0.0, 0.2, 0.3333333, 1.0):
                assert _same_bits(rule.plane(rec, W, H, radius, 1.0, amin), np.full((H, W), amin, np.float32))


def test_a_black_window_and_non_finite_records(rule):
    W, H = 16, 11
    SW, SH = gr.strata_shape(W, H)
    z = np.zeros((SH, SW, 3), np.float32)
    rec = rule.records(z, z)
    assert (rec == 0).all()
    assert _same_bits(rule.plane(rec, W, H, 1, 1.0, 0.2), np.full((H, W), 0.2, np.float32))       # Nn = 0: lambda = 0
    # one lit stratum among black ones: Nn > 0 only where the window reaches it
    lit = z.copy()
    lit[2, 3] = (1.0, 1.0, 1.0)
    got = rule.plane(rule.records(lit, z), W, H, 1, 1.0, 0.2)
    assert _same_bits(got, gr.alpha_plane(gr.records(lit, z), W, H, 1, 1.0, 0.2))
    reach = np.zeros((H, W), bool)
    reach[3:12, 6:15] = True                                     # strata rows 1-3, columns 2-4
    assert (got[reach] == 1.0).all() and _same_bits(got[~reach], np.full(int((~reach).sum()), 0.2, np.float32))
    # a non-finite record: lambda = 1 inside its window, untouched outside
    rng = np.random.default_rng(43)
    for bad in (np.nan, np.inf, -np.inf):
        new, old = _films(rng, W, H)
        for which in (0, 1):
            a, b = new.copy(), old.copy()
            (a if which == 0 else b)[1, 4, 1] = bad
            rec = rule.records(a, b)
            assert _same_bits(rec, gr.records(a, b)) and np.isnan(rec[1, 4]).all() and np.isfinite(np.delete(rec.reshape(-1, 2), SW + 4, 0)).all()
            for radius in (0, 1, 2):
                got = rule.plane(rec, W, H, radius, 1.0, 0.2)
                assert _same_bits(got, gr.alpha_plane(rec, W, H, radius, 1.0, 0.2))
                inwin = np.zeros((H, W), bool)
                inwin[max(0, 3 * (1 - radius)):3 * (2 + radius), max(0, 3 * (4 - radius)):3 * (5 + radius)] = True
                assert (got[inwin] == 1.0).all()
                clean = rule.plane(rule.records(new, old), W, H, radius, 1.0, 0.2)
                assert _same_bits(got[~inwin], clean[~inwin])


def test_a_dimmed_film_gives_the_same_weight_everywhere(rule):
    """Every radiance x 0.25 (a power of two: exact): delta = 0.75 L_old up to one rounding, and the plane is
    (float)(alpha_min + 0.75 (1 - alpha_min)) wherever the window is not black."""
    rng = np.random.default_rng(44)
    W, H = 16, 11
    _, old = _films(rng, W, H)
    old[0, 0] = 0
    got = rule.plane(rule.records(old * np.float32(0.25), old), W, H, 1, 1.0, 0.2)
    a = np.float64(np.float32(0.2))
    assert _same_bits(got, np.full((H, W), np.float32(a + 0.75 * (1 - a))))


# ---------------------------------------------------------------- the restatement of the alpha entry
def test_alpha_restatement_with_no_measurement_is_motion_ref_exactly(pt):
    frames, kw = mc.case(pt, "sphere")
    want = mc.run_ref(frames, iterations=1, **kw)
    H, W = frames[0][1].shape[:2]
    for fill in (np.nan, -0.5, 1.5, np.inf, -np.inf):
        got = gr.run_ref_alpha(frames, [np.full((H, W), fill, np.float32)] * len(frames), iterations=1, **kw)
        for (a, ia), (b, ib) in zip(got, want):
            assert np.array_equal(a, b) and np.array_equal(ia["fresh"], ib["fresh"]), fill
    # a constant plane is the scalar alpha
    want = mc.run_ref(frames, iterations=1, alpha=0.5, **kw)
    got = gr.run_ref_alpha(frames, [np.full((H, W), 0.5, np.float32)] * len(frames), iterations=1, **kw)
    assert all(np.array_equal(a, b) for (a, _), (b, _) in zip(got, want))
    # the random planes of the GPU test hold every kind of entry
    p = gr.random_plane(np.random.default_rng(5), H, W)
    t = gr.taken(p)
    assert 0.25 <= 1 - t.mean() <= 0.42 and np.isnan(p).any() and (p[~np.isnan(p)] < 0).any() and (p > 1).any() and np.isinf(p).any()
    assert p[t].min() == 0.0 and p[t].max() == 1.0
