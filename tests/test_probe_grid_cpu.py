"""The irradiance volume on the CPU (pt_probe_grid_count, pt_probe_grid_positions_host, pt_probe_shade_host) against the
numpy restatement of the rule (tests/probe_grid_ref.py), bit for bit; a constant field, an affine field, unlit pixels, a NaN
coefficient, and the refusals that need no device."""
import ctypes as C
import math

import numpy as np
import pytest

import probe_grid_ref as pr

INVALID = 1
U = 2.0 ** -53


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _shade(pt, cam, g, sh, feat, fallback, bias, weight):
    return pt.probe_shade_host(pr.pt_camera(pt, cam), g.as_pt(pt), sh, feat, fallback, pt.default_probe_shade(normal_bias=bias, weight=weight))


def test_symbols_and_defaults(pt):
    lib = pt._lib.lib()
    for name in ("pt_default_probe_shade", "pt_probe_grid_count", "pt_probe_grid_positions_host", "pt_probe_grid_bake_device", "pt_probe_shade_device",
                 "pt_probe_shade_host", "pt_render_probe_lit_device", "pt_render_probe_lit_host"):
        assert name in pt._lib.SYMBOLS and hasattr(lib, name), name
    s = pt.default_probe_shade()
    assert (s.normal_bias, s.weight) == (0.0, pt._lib.PT_PROBE_WEIGHT_TRILINEAR) and pt._lib.PT_PROBE_WEIGHT_FACING == 1
    assert C.sizeof(pt._lib.PtProbeGrid) == 64 and C.sizeof(pt._lib.PtProbeShade) == 8
    assert lib.pt_abi_version() == 6


def test_positions_index_order_and_bits(pt):
    g = pr.Grid((0.1, -0.7, 2.3), (0.3, 0.7, 1.1), (2, 3, 4))
    pos = pt.probe_grid_positions(g.as_pt(pt))
    assert pt.probe_grid_count(g.as_pt(pt)) == 24 and pos.shape == (24, 3)
    assert np.array_equal(_bits(pos), _bits(pr.positions(g)))
    for iz in range(4):
        for iy in range(3):
            for ix in range(2):
                want = [np.float32(0.1 + ix * 0.3), np.float32(-0.7 + iy * 0.7), np.float32(2.3 + iz * 1.1)]
                assert list(pos[(iz * 3 + iy) * 2 + ix]) == want
    one = pr.Grid((1e-3, 2.0, -3.0), (0.0, -1.0, 5.0), (1, 1, 1))      # an axis with one probe: any finite spacing
    assert pt.probe_grid_count(one.as_pt(pt)) == 1
    assert np.array_equal(_bits(pt.probe_grid_positions(one.as_pt(pt))), _bits(np.array([[1e-3, 2.0, -3.0]], dtype=np.float32)))


@pytest.mark.parametrize("origin, spacing, counts", [
    ((0, 0, 0), (1, 1, 1), (0, 2, 2)), ((0, 0, 0), (1, 1, 1), (2, 2, 0)), ((0, 0, 0), (1, np.inf, 1), (2, 1, 2)), ((0, 0, 0), (np.nan, 1, 1), (1, 2, 2)),
    ((0, 0, 0), (1, 0, 1), (2, 2, 2)), ((0, 0, 0), (1, 1, -1), (2, 2, 2)), ((0, np.inf, 0), (1, 1, 1), (2, 2, 2)), ((np.nan, 0, 0), (1, 1, 1), (2, 2, 2)),
    ((0, 0, 0), (1, 1, 1), (41, 40, 40)), ((0, 0, 0), (1, 1, 1), (65536, 1, 1)), ((0, 0, 0), (1, 1, 1), (65536, 65536, 65536))])
def test_invalid_grids_count_zero(pt, origin, spacing, counts):
    g = pr.Grid(origin, spacing, counts)
    assert pr.count(g) == 0 and pt.probe_grid_count(g.as_pt(pt)) == 0
    out = np.zeros(3, dtype=np.float32)
    assert pt._lib.lib().pt_probe_grid_positions_host(C.byref(g.as_pt(pt)), out.ctypes.data_as(C.c_void_p)) == INVALID
    assert "invalid probe grid" in pt._lib.lib().pt_last_error().decode()
    assert pt.probe_grid_count(pr.Grid((0, 0, 0), (1, 1, 1), (65535, 1, 1)).as_pt(pt)) == 65535
    assert pt._lib.lib().pt_probe_grid_count(None) == 0


@pytest.mark.parametrize("name", sorted(pr.GRIDS))
@pytest.mark.parametrize("size", pr.SIZES)
def test_shade_against_the_restatement(pt, name, size):
    W, H = size
    cam, g, sh, feat, fallback = pr.make_case(name, W, H, seed=11)
    xc, yc = pr.centre_pixel(W, H)
    for weight in (pr.TRILINEAR, pr.FACING):
        for bias in (0.0, 0.05):
            for fb in (fallback, None):
                det = {}
                want, want8, lit = pr.shade(cam, g, sh, feat, fb, bias, weight, det)
                got, got8 = _shade(pt, cam, g, sh, feat, fb, bias, weight)
                assert np.array_equal(_bits(got), _bits(want)), (name, size, weight, bias)
                assert np.array_equal(got8, want8)
                assert lit[yc, xc] and np.isfinite(want).all()
    # the centre pixel's point is a probe, bit for bit
    det = {}
    pr.shade(cam, g, sh, feat, None, 0.0, pr.TRILINEAR, det)
    k = int(np.nonzero((det["ys"] == yc) & (det["xs"] == xc))[0][0])
    assert np.array_equal(det["P"][k], g.origin + np.array(pr.on_probe(g)) * g.spacing)
    if W * H > 4:      # inside, and outside on each side of every axis that has sides
        rel = (det["P"] - g.origin) / np.where(g.spacing > 0, g.spacing, 1.0)
        for a in range(3):
            if g.counts[a] > 1:
                assert (rel[:, a] < 0).any() and (rel[:, a] > g.counts[a] - 1).any()
        assert ((rel > 0) & (rel < np.array(g.counts) - 1))[:, [a for a in range(3) if g.counts[a] > 1]].all(axis=1).any()
        assert (~lit).sum() == 4


def test_random_cameras(pt):
    rng = np.random.default_rng(5)
    g = pr.GRIDS["5x4x3"]
    for trial in range(4):
        c = pt.camera_look_at(rng.uniform(-1, 1, 3) + [0, 0, 1.0], rng.uniform(-0.3, 0.3, 3) + [0, 0, -2.5], (0.1, 1.0, 0.05), 19, 13, rng.uniform(30, 80))
        cam = pr.cam_tuple(c)
        feat = pr.make_case("5x4x3", 19, 13, seed=trial)[3]
        sh = rng.normal(size=(60, 9, 3)).astype(np.float32)
        for weight in (pr.TRILINEAR, pr.FACING):
            want, want8, lit = pr.shade(cam, g, sh, feat, None, 0.05, weight)
            got, got8 = pt.probe_shade_host(c, g.as_pt(pt), sh, feat, None, pt.default_probe_shade(normal_bias=0.05, weight=weight))
            assert np.array_equal(_bits(got), _bits(want)) and np.array_equal(got8, want8) and lit.sum() > 200


@pytest.mark.parametrize("name", sorted(pr.GRIDS))
def test_a_constant_field_comes_out_exactly(pt, name):
    cam, g, sh, feat, _ = pr.make_case(name, 33, 17, seed=3)
    sh[:] = sh[0]
    det = {}
    pr.shade(cam, g, sh, feat, None, 0.05, pr.TRILINEAR, det)
    E = pr.irradiance(np.broadcast_to(sh[0].astype(np.float64), (len(det["ys"]), 9, 3)), det["nn"])
    a = feat[det["ys"], det["xs"], 0:3].astype(np.float64)
    want = ((np.where(a < 0.0, 0.0, a) * E) / math.pi).astype(np.float32)
    assert (E > 0).any() and (want > 0).any()
    for weight in (pr.TRILINEAR, pr.FACING):
        got, _ = _shade(pt, cam, g, sh, feat, None, 0.05, weight)
        assert np.array_equal(_bits(got[det["ys"], det["xs"]]), _bits(want))


def test_an_affine_field_is_reproduced(pt):
    """An L0-only field C(p) = alpha + beta . p, exact in f32 at every probe, seen by the axis-aligned camera with albedo 1: a pixel
    whose point P lies inside the grid must give Y0 C(P).  With u = 2^-53, G = the largest count - 1, D = max_j |C_j - C_0| over the
    grid and M = max |C|, the rule's own roundings allow:
      g (a subtraction, a division): |dg| <= 2 u G; f = g - i is exact, 1 - f adds u / 2: per axis the point moves by at most
      (2 G + 1) u cells, and the field changes by at most D per cell: 3 (2 G + 1) u D;
      a weight is two products (2 u), a term a difference and a product more (4 u), seven additions (7 u) of terms whose sizes sum
      to at most D: 11 u D; the denominator two products and eight additions: 10 u D; the quotient u D; C_0 + ...: u M;
      A_0 C, Y_0 ..., ... / pi: 3 u of the result r; the expectation Y0 (alpha + beta . P) formed here in f64: 5 u (|alpha| +
      sum |beta_a P_a|) Y0; and the one rounding to f32: 2^-24 |r|."""
    g = pr.GRIDS["5x4x3"]
    alpha, beta = 4.0, np.array([0.5, -0.25, 0.75])
    pos = pr.positions(g).astype(np.float64)
    field = alpha + pos @ beta
    assert np.array_equal(field.astype(np.float32).astype(np.float64), field) and field.min() > 0
    sh = np.zeros((pr.count(g), 9, 3), dtype=np.float32)
    sh[:, 0, :] = field[:, None]
    W, H = 33, 17
    cam, _, _, feat, _ = pr.make_case("5x4x3", W, H, seed=9)
    feat[..., 0:3] = 1.0
    det = {}
    pr.shade(cam, g, sh, feat, None, 0.0, pr.TRILINEAR, det)
    rel = (det["P"] - g.origin) / g.spacing
    inside = ((rel >= 0) & (rel <= np.array(g.counts) - 1)).all(axis=1)
    assert inside.sum() >= 10
    got, _ = _shade(pt, cam, g, sh, feat, None, 0.0, pr.TRILINEAR)
    r = got[det["ys"], det["xs"]][inside].astype(np.float64)
    P = det["P"][inside]
    want = 0.282095 * (alpha + P @ beta)
    G, D, M = max(g.counts) - 1, field.max() - field.min(), field.max()
    bound = 0.282095 * ((3 * (2 * G + 1) + 11 + 10 + 1) * U * D + U * M) + 3 * U * np.abs(want) \
        + 5 * U * 0.282095 * (abs(alpha) + (np.abs(beta) * np.abs(P)).sum(axis=1)) + 2.0 ** -24 * np.abs(want)
    err = np.abs(r - want[:, None])
    print(f"affine field: {inside.sum()} points inside, worst error {err.max():.3e}, bound {bound.min():.3e}")
    assert (err <= bound[:, None]).all()
    assert np.array_equal(r[:, 0], r[:, 1]) and np.array_equal(r[:, 0], r[:, 2])


def test_unlit_pixels_take_the_fallback(pt):
    g = pr.GRIDS["2x2x2"]
    rng = np.random.default_rng(2)
    W, H = 4, 2
    cam = pr.axis_camera(W, H, (0.0, 0.0, 0.5))
    feat = np.empty((H, W, 8), dtype=np.float32)
    feat[..., 0:3], feat[..., 3], feat[..., 4:7], feat[..., 7] = 0.5, 0.0, (0.0, 0.6, 0.8), 3.0
    feat[0, 0, 7] = 0.0                       # depth 0
    feat[0, 1, 7] = np.nan                    # NaN depth
    feat[0, 2, 3] = 0.25                      # emitter
    feat[0, 3, 4:7] = 0.0                     # zero normal
    feat[1, 0, 5] = np.nan                    # NaN normal
    feat[1, 1, 1] = np.inf                    # infinite albedo
    feat[1, 2, 7] = -1.0                      # behind the camera
    unlit = np.ones((H, W), dtype=bool)
    unlit[1, 3] = False
    fallback = rng.uniform(0, 2, (H, W, 3)).astype(np.float32)
    fallback[0, 0] = (np.nan, -0.0, np.inf)
    fallback.view(np.uint32)[0, 1, 0] = 0x7FC12345      # a NaN with a payload: the bits, not the value
    for sh in (rng.normal(size=(8, 9, 3)).astype(np.float32), np.full((8, 9, 3), np.nan, dtype=np.float32), np.full((8, 9, 3), np.inf, dtype=np.float32)):
        for weight in (pr.TRILINEAR, pr.FACING):
            got, got8 = _shade(pt, cam, g, sh, feat, fallback, 0.0, weight)
            assert np.array_equal(_bits(got)[unlit], _bits(fallback)[unlit])
            assert np.array_equal(got8[unlit], pr.rgba8(fallback)[unlit])
            got, got8 = _shade(pt, cam, g, sh, feat, None, 0.0, weight)
            assert not _bits(got)[unlit].any()                                                  # +0.0
            assert np.array_equal(got8[unlit], np.broadcast_to(np.array([0, 0, 0, 255], dtype=np.uint8), (7, 4)))
            assert np.array_equal(_bits(got), _bits(pr.shade(cam, g, sh, feat, None, 0.0, weight)[0]))
    # W = 1 and H = 1: s or t divides by zero, no pixel has a point
    for (w, h) in ((1, 3), (3, 1), (1, 1)):
        cam1 = (cam[0], cam[1], cam[2], cam[3], w, h)
        f1 = np.broadcast_to(feat[1, 3], (h, w, 8)).copy()
        fb1 = fallback.reshape(-1, 3)[:w * h].reshape(h, w, 3)
        got, got8 = _shade(pt, cam1, g, np.full((8, 9, 3), np.nan, dtype=np.float32), f1, fb1, 0.0, pr.TRILINEAR)
        assert np.array_equal(_bits(got), _bits(fb1)) and np.array_equal(got8, pr.rgba8(fb1))
        got, got8 = _shade(pt, cam1, g, np.full((8, 9, 3), np.nan, dtype=np.float32), f1, None, 0.0, pr.FACING)
        assert not _bits(got).any() and (got8.reshape(-1, 4) == (0, 0, 0, 255)).all()


def test_a_nan_coefficient_stays_in_its_cells(pt):
    cam, g, sh, feat, _ = pr.make_case("5x4x3", 33, 17, seed=4)
    det = {}
    clean, clean8, lit = pr.shade(cam, g, sh, feat, None, 0.0, pr.TRILINEAR, det)
    probe, k, ch = (1 * 4 + 2) * 5 + 3, 5, 1
    bad = sh.copy()
    bad[probe, k, ch] = np.nan
    for weight in (pr.TRILINEAR, pr.FACING):
        base, base8 = _shade(pt, cam, g, sh, feat, None, 0.0, weight)
        got, got8 = _shade(pt, cam, g, bad, feat, None, 0.0, weight)
        touched = np.zeros(lit.shape, dtype=bool)
        sel = (det["idx"] == probe).any(axis=1)
        touched[det["ys"][sel], det["xs"][sel]] = True
        assert 0 < touched.sum() < lit.sum()
        assert np.isnan(got[touched][:, ch]).all()
        assert np.array_equal(_bits(got)[~touched], _bits(base)[~touched]) and np.array_equal(got8[~touched], base8[~touched])
        others = [c for c in range(3) if c != ch]
        assert np.array_equal(_bits(got[touched][:, others]), _bits(base[touched][:, others]))


def test_refusals_without_a_device(pt):
    L = pt._lib.lib()
    g = pr.GRIDS["2x2x2"].as_pt(pt)
    cam = pr.pt_camera(pt, pr.axis_camera(4, 4, (0.0, 0.0, 0.5)))
    sp = pt.default_probe_shade()
    buf = np.zeros(4 * 4 * 8 + 8 * 27 + 64, dtype=np.float32)
    base = buf.ctypes.data + (-buf.ctypes.data % 16)
    FAKE, ODD = C.c_void_p(base), C.c_void_p(base + 2)
    OFF4 = C.c_void_p(base + 4)

    def refused(rc, text):
        assert rc == INVALID and text in L.pt_last_error().decode(), (rc, L.pt_last_error())

    for entry, who in ((lambda *a: L.pt_probe_shade_host(*a), "pt_probe_shade_host"), (lambda *a: L.pt_probe_shade_device(None, *a), "pt_probe_shade_device")):
        refused(entry(None, C.byref(g), FAKE, FAKE, None, C.byref(sp), FAKE, None), who + ": null argument")
        refused(entry(C.byref(cam), None, FAKE, FAKE, None, C.byref(sp), FAKE, None), who + ": null argument")
        refused(entry(C.byref(cam), C.byref(g), FAKE, FAKE, None, None, FAKE, None), who + ": null argument")
        refused(entry(C.byref(cam), C.byref(g), None, FAKE, None, C.byref(sp), FAKE, None), "sh27 is null")
        refused(entry(C.byref(cam), C.byref(g), FAKE, None, None, C.byref(sp), FAKE, None), "the feature plane is null")
        refused(entry(C.byref(cam), C.byref(g), FAKE, FAKE, None, C.byref(sp), None, None), "the linear output is null")
        refused(entry(C.byref(cam), C.byref(g), ODD, FAKE, None, C.byref(sp), FAKE, None), "sh27 must be 4-byte aligned")
        refused(entry(C.byref(cam), C.byref(g), FAKE, ODD, None, C.byref(sp), FAKE, None), "the feature plane must be")
        refused(entry(C.byref(cam), C.byref(g), FAKE, FAKE, ODD, C.byref(sp), FAKE, None), "the fallback plane must be 4-byte aligned")
        refused(entry(C.byref(cam), C.byref(g), FAKE, FAKE, None, C.byref(sp), ODD, None), "the linear output must be 4-byte aligned")
        refused(entry(C.byref(cam), C.byref(g), FAKE, FAKE, None, C.byref(sp), FAKE, ODD), "the RGBA8 output must be 4-byte aligned")
        refused(entry(C.byref(cam), C.byref(pr.Grid((0, 0, 0), (1, 0, 1), (2, 2, 2)).as_pt(pt)), FAKE, FAKE, None, C.byref(sp), FAKE, None), "invalid probe grid")
        refused(entry(C.byref(cam), C.byref(g), FAKE, FAKE, None, C.byref(pt.default_probe_shade(weight=2)), FAKE, None), "unknown weight 2")
        for b in (np.inf, -np.inf, np.nan):
            refused(entry(C.byref(cam), C.byref(g), FAKE, FAKE, None, C.byref(pt.default_probe_shade(normal_bias=b)), FAKE, None), "normal_bias must be finite")
        for (w, h) in ((0, 4), (4, 0)):
            zero = pr.pt_camera(pt, pr.axis_camera(4, 4, (0.0, 0.0, 0.5)))
            zero.width, zero.height = w, h
            refused(entry(C.byref(zero), C.byref(g), FAKE, FAKE, None, C.byref(sp), FAKE, None), "a zero size")
    # the device entry wants its features 16-byte aligned, and a context once everything else is right
    refused(L.pt_probe_shade_device(None, C.byref(cam), C.byref(g), FAKE, OFF4, None, C.byref(sp), FAKE, None), "the feature plane must be 16-byte aligned")
    refused(L.pt_probe_shade_device(None, C.byref(cam), C.byref(g), FAKE, FAKE, None, C.byref(sp), FAKE, None), "pt_probe_shade_device: null context")
    prm = pt.default_params(spp=1)
    refused(L.pt_probe_grid_bake_device(None, C.byref(g), 64, C.byref(prm), FAKE), "pt_probe_grid_bake_device: null argument")
    refused(L.pt_render_probe_lit_device(None, C.byref(cam), C.byref(prm), 1, C.byref(g), FAKE, None, C.byref(sp), FAKE, None), "pt_render_probe_lit_device: null argument")
    refused(L.pt_render_probe_lit_host(None, C.byref(cam), C.byref(prm), 1, C.byref(g), FAKE, None, C.byref(sp), FAKE, None), "pt_render_probe_lit_host: null argument")
    refused(L.pt_probe_grid_positions_host(C.byref(g), None), "out_positions3 is null")
    refused(L.pt_probe_grid_positions_host(None, FAKE), "null argument")
    # the host entry works on 4-byte aligned features
    cam4, g4, sh, feat, _ = pr.make_case("2x2x2", 2, 2, seed=1)
    raw = np.zeros(2 * 2 * 8 + 1, dtype=np.float32)
    view = raw[1:]
    view[:] = feat.ravel()
    out, out8 = np.empty((2, 2, 3), dtype=np.float32), np.empty((2, 2, 4), dtype=np.uint8)
    assert L.pt_probe_shade_host(C.byref(pr.pt_camera(pt, cam4)), C.byref(g4.as_pt(pt)), sh.ctypes.data_as(C.c_void_p), C.c_void_p(view.ctypes.data), None,
                                 C.byref(sp), out.ctypes.data_as(C.c_void_p), out8.ctypes.data_as(C.c_void_p)) == 0
    assert np.array_equal(_bits(out), _bits(pr.shade(cam4, g4, sh, feat)[0]))
