"""Feature-guided upsampling (pt_upsample_device) without a GPU: the argument checks through the C ABI, the
pinned defaults, the shared rule header (pathtrace_amd/csrc/pt_upsample.h) through pt_upsample_host and under the
sanitizers, and the numpy restatement (tests/upsample_ref.py) against cases worked out by hand."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import upsample_ref as ur

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = [C.c_void_p(0x1000 * k) for k in range(1, 6)]      # aligned, distinct addresses no check may read
ODD, ODD4 = C.c_void_p(0x7002), C.c_void_p(0x7004)        # not 4-byte aligned; 4- but not 16-byte aligned
BAR = 1e-4                                                # the bar of the filter parity tests, floor 1e-3 under the reference


def _refused(pt, rc, part):
    assert rc == 1, rc                                            # PT_ERR_INVALID_ARG
    msg = pt._lib.lib().pt_last_error().decode()
    assert part in msg, msg


def test_defaults_are_pinned(pt):
    u, d = pt.default_upsample(), pt.default_denoise()
    assert (u.sigma_n, u.sigma_d) == (128.0, float(np.float32(0.025)))
    assert (u.sigma_n, u.sigma_d) == (d.sigma_n, d.sigma_d)          # the denoiser's
    assert C.sizeof(pt._lib.PtUpsample) == 8
    assert pt.default_upsample(sigma_n=2.0).sigma_n == 2.0


@pytest.mark.parametrize("entry", ["pt_upsample_device", "pt_upsample_host"])
def test_upsample_refuses_bad_arguments_without_a_device(pt, entry):
    """every check comes before the context or a plane is looked at: a null context and addresses nothing may read"""
    L = pt._lib.lib()
    ok = pt.default_upsample()

    def call(up=ok, lo=(4, 4), full=(8, 8), c=FAKE[0], f=FAKE[1], F=FAKE[2], out=FAKE[3], rgba=FAKE[4]):
        args = (lo[0], lo[1], c, f, full[0], full[1], F, C.byref(up) if up else None, out, rgba)
        return L.pt_upsample_device(None, *args) if entry == "pt_upsample_device" else L.pt_upsample_host(*args)

    for name in ("c", "f", "F", "out", "up"):
        _refused(pt, call(**{name: None}), entry + ": null argument")
    for name in ("f", "F"):
        _refused(pt, call(**{name: ODD4}), "16-byte aligned")
    for name in ("c", "out", "rgba"):
        _refused(pt, call(**{name: ODD}), "4-byte aligned")
    for lo, full in [((1, 4), (8, 8)), ((4, 0), (8, 8)), ((1, 1), (1, 8)), ((2, 2), (8, 1))]:
        _refused(pt, call(lo=lo, full=full), "every dimension must be >= 2")
    _refused(pt, call(lo=(9, 4)), "above the full size")
    _refused(pt, call(lo=(4, 9)), "above the full size")
    for src in (0, 1, 2):
        _refused(pt, call(out=FAKE[src]), "must not be an input")
        _refused(pt, call(rgba=FAKE[src]), "must not be an input")
    # byte ranges, not addresses: 4 x 4 low (film 192 B, records 512 B), 8 x 8 full (records 2048 B, film 768 B, RGBA8 256 B)
    at = lambda p, off: C.c_void_p(p.value + off)
    for src, size in ((0, 192), (1, 512), (2, 2048)):
        _refused(pt, call(out=at(FAKE[src], 4)), "must not be an input")                  # starts 4 bytes into the input
        _refused(pt, call(rgba=at(FAKE[src], 4)), "must not be an input")
        _refused(pt, call(out=at(FAKE[src], 4 - 768)), "must not be an input")            # ends 4 bytes into it
        _refused(pt, call(rgba=at(FAKE[src], 4 - 256)), "must not be an input")
        _refused(pt, call(out=at(FAKE[src], size - 4)), "must not be an input")           # starts in its last word
    for off in (0, 4, 768 - 256, 768 - 4, 4 - 256):
        _refused(pt, call(rgba=at(FAKE[3], off)), "the two outputs must not share a byte")
    _refused(pt, call(out=FAKE[0], rgba=FAKE[3]), "must not be an input")                 # (an input comes before the other output)
    for field in ("sigma_n", "sigma_d"):
        for bad in (-1.0, float("nan"), float("inf")):
            _refused(pt, call(up=pt.default_upsample(**{field: bad})), "finite and >= 0")
    # ranges that only touch share no byte: accepted up to the null context (the host entry would go on to read them: device only)
    touching = [dict(out=at(FAKE[0], 192)), dict(out=at(FAKE[1], 512)), dict(out=at(FAKE[2], 2048)), dict(out=at(FAKE[2], -768)),
                dict(rgba=at(FAKE[0], -256)), dict(rgba=at(FAKE[3], 768)), dict(rgba=at(FAKE[3], -256)), dict(out=at(FAKE[4], 256))]
    if entry == "pt_upsample_device":
        for kw in touching:
            _refused(pt, call(**kw), entry + ": null context")
    if entry == "pt_upsample_device":      # zero sigmas, equal sizes, the least image and no RGBA8 plane are arguments like any other
        for kw in (dict(up=pt.default_upsample(sigma_n=0.0, sigma_d=0.0)), dict(lo=(8, 8)), dict(lo=(2, 2), full=(2, 2)), dict(rgba=None)):
            _refused(pt, call(**kw), entry + ": null context")


def test_one_call_entry_refuses_bad_arguments_without_a_device(pt):
    L = pt._lib.lib()
    cam, prm, dn, up = pt.camera_new(width=8, height=8), pt.default_params(spp=4), pt.default_denoise(), pt.default_upsample()
    buf = (C.c_float * 8)()
    _refused(pt, L.pt_render_denoised_upsampled(None, C.byref(cam), C.byref(prm), 4, 4, 4, C.byref(dn), C.byref(up), buf, None, None, None),
             "pt_render_denoised_upsampled: null argument")


@pytest.mark.parametrize("full,low", ur.SHAPES)
def test_host_entry_is_the_restatement(pt, full, low):
    """pt_upsample_host -- the rule header as the host compiler builds it -- against the f64 restatement, every pixel."""
    for seed in (0, 1):
        c, f, F = ur.crafted_inputs(1000 * full[0] + seed, full, low)
        got, rgba = pt.upsample_host(c, f, F)
        ref = ur.upsample(c, f, F)
        err = ur.max_rel(got, ref)
        print(f"{full} from {low}, seed {seed}: max rel err {err:.2e}")
        assert err <= BAR
        assert np.array_equal(rgba, _rgba8(got))
    got, _ = pt.upsample_host(c, f, F, sigma_n=3.0, sigma_d=0.5)
    err = ur.max_rel(got, ur.upsample(c, f, F, sigma_n=3.0, sigma_d=0.5))
    print(f"{full} from {low}, sigma_n 3, sigma_d 0.5: max rel err {err:.2e}")
    assert err <= BAR


def _rgba8(lin):
    """sqrt, clamp, `as u8`, alpha 255: the RGBA8 rule of every film"""
    q = (np.clip(np.sqrt(np.asarray(lin, np.float32).astype(np.float64)), 0.0, 1.0) * 255.0).astype(np.uint8)
    return np.concatenate([q, np.full(q.shape[:-1] + (1,), 255, np.uint8)], -1)


def test_equal_sizes_give_back_the_film(pt):
    """w = W, h = H, F = f: every pixel has one tap, itself: c' = (c / a) a in f32, the denoiser's iterations = 0"""
    for full, low in ur.SHAPES[:2]:
        c, f, F = ur.crafted_inputs(7, full, low)
        got, _ = pt.upsample_host(c, f, F)
        a = np.maximum(f[..., 0:3], np.float32(1e-3))
        want = (c / a) * a
        assert want.dtype == np.float32
        assert np.all(np.abs(got - want) <= 2 * np.spacing(np.abs(want)))
        _, info = ur.upsample(c, f, F, info=True)
        assert (info["anchor"] == 0).all() and info["own"].all()


def _flat(w, h, depth=1.0):
    f = np.zeros((h, w, 8), np.float32)
    f[..., 0:3] = 1.0
    f[..., 6] = 1.0
    f[..., 7] = depth
    return f


def test_a_ramp_across_a_depth_edge_by_hand(pt):
    """5 x 2 from 3 x 2, albedo 1, one normal: the rows are alike (h = H: Y = y), X = x / 2 - 0.25.  Low film u = 1, 2, 4 at depths
    1, 1, 2; full depths 1, 1, 1, 2, 2; r = 2, so the depth weight of a tap across the edge is exp(-1 / (0.05 d)).
      x = 0   X0 = -1 (skipped), tap 0 with b = 0.75: u = 1
      x = 1   taps 0 (b 0.75, anchor) and 1 (b 0.25), both at the pixel's depth: u = 1 + 0.25 (2 - 1) / (1 + 1e-6)
      x = 2   taps 0 (b 0.25) and 1 (b 0.75, anchor): u = 2 + 0.25 (1 - 2) / (1 + 1e-6)
      x = 3   d = 2: taps 1 (b 0.75, depth 1: w = 0.75 e^-10, the anchor all the same) and 2 (b 0.25, depth 2: w = 0.25):
              u = 2 + 0.25 (4 - 2) / (0.75 e^-10 + 0.25 + 1e-6) = 3.99972...: the far side of the edge, where bilinear gives 2.5
      x = 4   taps 1 (b 0.25, w = 0.25 e^-10) and 2 (b 0.75, anchor): u = 4 + 0.25 e^-10 (2 - 4) / (0.75 + 0.25 e^-10 + 1e-6)"""
    f, F = _flat(3, 2), _flat(5, 2)
    f[:, 2, 7] = 2.0
    F[:, 3:, 7] = 2.0
    c = np.zeros((2, 3, 3), np.float32)
    c[:, 0], c[:, 1], c[:, 2] = 1.0, 2.0, 4.0
    e10 = math.exp(-1.0 / (0.025 * 2.0 * 2.0 + 1e-10))
    want = [1.0 + 0.75 * 0.0 / (0.75 + 1e-6),
            1.0 + 0.25 * (2.0 - 1.0) / (1.0 + 1e-6),
            2.0 + 0.25 * (1.0 - 2.0) / (1.0 + 1e-6),
            2.0 + 0.25 * (4.0 - 2.0) / (0.75 * e10 + 0.25 + 1e-6),
            4.0 + 0.25 * e10 * (2.0 - 4.0) / (0.75 + 0.25 * e10 + 1e-6)]
    ref, info = ur.upsample(c, f, F, info=True)
    for y in (0, 1):
        assert np.allclose(ref[y, :, 0], want, rtol=1e-12, atol=0)
        assert list(info["anchor"][y]) == [1, 0, 1, 0, 1]          # (the row's taps are numbers 0 and 1: fy = 0)
    assert abs(want[3] - 3.99972) < 1e-5 and abs(ur.bilinear(c, 5, 2)[0, 3, 0] - 2.5) < 1e-12
    got, _ = pt.upsample_host(c, f, F)
    assert ur.max_rel(got, ref) <= BAR


def test_a_pixel_whose_taps_are_all_of_another_class_by_hand(pt):
    """4 x 4 from 2 x 2: X = x / 3 - 1 / 3 = -1/3, 0, 1/3, 2/3 and Y = 1.5 - (3.5 - y) / 3 = 1/3, 2/3, 1, 4/3 (rows count from the
    top, t from the bottom).  Pixel (x 1, y 2): X = 0, Y = 1 exactly -- one tap, low pixel (row 1, column 0).  Pixel (2, 2):
    X = 1/3: taps (1, 0) with b = 2/3 and (1, 1) with b = 1/3.  The low records are all emitters, the full records surfaces:
    no tap agrees, every weight is 0, and the pixel takes the anchor -- the tap with the largest b -- times its own albedo."""
    f, F = _flat(2, 2), _flat(4, 4)
    f[..., 3] = 1.0
    F[..., 0:3] = 0.5
    c = np.array([[[1.0, 2.0, 3.0], [10.0, 20.0, 30.0]], [[5.0, 6.0, 7.0], [50.0, 60.0, 70.0]]], np.float32)
    ref, info = ur.upsample(c, f, F, info=True)
    assert not info["own"].any()
    assert np.array_equal(ref[2, 1], [2.5, 3.0, 3.5]) and info["anchor"][2, 1] == 0
    assert np.array_equal(ref[2, 2], [2.5, 3.0, 3.5]) and info["anchor"][2, 2] == 0
    assert np.array_equal(ref[2, 3], [25.0, 30.0, 35.0]) and info["anchor"][2, 3] == 1      # X = 2/3: the anchor is (1, 1)
    assert np.array_equal(ref[0, 1], [0.5, 1.0, 1.5]) and info["anchor"][0, 1] == 0         # Y = 1/3: rows 0 (b 2/3) and 1
    assert np.array_equal(ref[1, 0], [2.5, 3.0, 3.5]) and info["anchor"][1, 0] == 3         # X0 = -1, Y = 2/3: (1, 0) is tap 3
    assert np.array_equal(ref[3, 3], [25.0, 30.0, 35.0])                                    # Y = 4/3: low row 2 is outside
    got, _ = pt.upsample_host(c, f, F)
    assert np.array_equal(got, ref.astype(np.float32))
    # the same taps under the pixel's own class: now they are weighted, b = 2/3 and 1/3
    f[..., 3] = 0.0
    ref = ur.upsample(c, f, F)
    c64 = c.astype(np.float64)
    assert np.allclose(ref[2, 2], 0.5 * (c64[1, 0] + (1.0 / 3.0) * (c64[1, 1] - c64[1, 0]) / (1.0 + 1e-6)), rtol=1e-6, atol=0)


@pytest.mark.parametrize("full,low", ur.SHAPES[2:])
def test_a_tap_of_another_class_never_reaches_a_pixel_with_a_tap_of_its_own(pt, full, low):
    """the low film times 1000 under every emitter and every miss record: a surface pixel with a surface tap keeps its bits"""
    c, f, F = ur.crafted_inputs(5, full, low)
    base, _ = pt.upsample_host(c, f, F)
    _, info = ur.upsample(c, f, F, info=True)
    loud = c.copy()
    loud[ur.classes(f) != ur.SURFACE] *= 1000.0
    got, _ = pt.upsample_host(loud, f, F)
    keep = (ur.classes(F) == ur.SURFACE) & info["own"]
    assert keep.mean() > 0.5 and (~keep).sum() > 0
    assert np.array_equal(got[keep].view(np.uint32), base[keep].view(np.uint32))
    assert not np.array_equal(got[~keep], base[~keep])             # (and the film did change where it may)


def test_rule_header_is_clean_under_asan_and_ubsan(tmp_path):
    """tests/tools/upsample_san.cpp: a stand-alone program around the host functions of pt_upsample.h"""
    exe = str(tmp_path / "upsample_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "tools", "upsample_san.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "upsample_san: 0 failed checks" in out, out[-3000:]
    assert "runtime error" not in out and "AddressSanitizer" not in out, out[-3000:]
