"""The case table of tests/atrous_cases.py without a device: its admission condition (the f32 evaluation of the restatement
against the f64 one), the NaN footprint the rule implies, and closed forms of the rule written without the restatement."""
import numpy as np
import pytest

import atrous_cases as ac
import denoise_ref as dr


@pytest.mark.parametrize("family", ac.FAMILIES)
def test_every_case_meets_the_admission_condition(family):
    """A condition of entry, not a measurement: within ADMIT of f64 when every array is f32, and the same non-finite mask."""
    worst = 0.0
    for c in (c for c in ac.CASES if c.family == family):
        ref = ac.reference(c.name)
        f32 = ac.evaluate(c, np.float32)
        assert f32.dtype == np.float32 and ref.dtype == np.float64
        assert np.array_equal(np.isfinite(f32), np.isfinite(ref)), c.name
        err = ac.max_rel(f32, ref)
        worst = max(worst, err)
        assert err <= ac.ADMIT, (c.name, err)
    print(f"{family}: f32 restatement against f64, worst {worst:.2e}")


def test_the_table_holds_what_it_says():
    names = set(ac.NAMES)
    for H, W in ac.SIZES:
        assert f"size_{H}x{W}" in names
    for c in ac.CASES:
        H, W = c.film.shape[:2]
        assert c.film.shape == (H, W, 3) and c.feat.shape == (H, W, 8) and c.film.dtype == c.feat.dtype == np.float32
        assert c.var is None or (c.var.shape == (H, W) and c.var.dtype == np.float32)
        assert c.dn["iterations"] <= 16 and min(c.dn["sigma_l"], c.dn["sigma_n"], c.dn["sigma_d"]) >= 0
        assert np.isfinite(np.float32(max(c.dn["sigma_l"], c.dn["sigma_n"], c.dn["sigma_d"])))
        assert not (np.signbit(c.film) & (c.film == 0)).any()          # (-0 + 0 = +0: the exact statements ask for no -0)
    # the quantised palette: every finite film value a multiple of 1/64, every depth of 1/8 (but the 1e-4 of its case)
    for c in ac.CASES:
        fin = c.film[np.isfinite(c.film)]
        assert np.array_equal(fin * 64, np.round(fin * 64)), c.name
        if c.name != "feat_depth_tiny":
            assert np.array_equal(c.feat[..., 7] * 8, np.round(c.feat[..., 7] * 8)), c.name
    assert np.float32(1e-42) > 0 and np.float32(1e-42) < np.finfo(np.float32).tiny


NAN_CASES = [n for n in ac.NAMES if n.startswith("film_nan")]


@pytest.mark.parametrize("name", NAN_CASES)
def test_a_nan_reaches_the_pixels_the_rule_connects_it_to(name):
    """The restatement's NaN mask is the footprint that follows from the rule's structure (ac.nan_footprint)."""
    c = ac.BY_NAME[name]
    ref = ac.reference(name)
    assert not np.isinf(ref).any()
    assert np.array_equal(np.isnan(ref), ac.nan_footprint(c))


def test_nan_footprints_by_class():
    """Through the TAPS a NaN on an emitter or on a miss pixel reaches nobody: an emitter inside an emitter, a miss pixel
    among miss pixels, poisons its own entry only.  Beside a surface it still reaches it through the 3 x 3 variance, which
    looks at no class (k_denoise_init and the rule agree on that), and from there on as a surface NaN does."""
    for name, (y, x, ch) in (("film_nan_emitter_block", (4, 8, 1)), ("film_nan_miss_deep", (4, 12, 2))):
        m = ac.nonfinite_mask(name)
        assert m.sum() == 1 and m[y, x, ch]
    m = ac.nonfinite_mask("film_nan_emitter")
    assert m[4, 8].tolist() == [False, True, False] and m.all(-1).sum() > 9           # the emitter keeps its finite channels
    m = ac.nonfinite_mask("film_nan_miss_edge")
    assert m[4, 15].tolist() == [False, False, True] and not m[:, :15].any() and m[:, 16:].all(-1).sum() > 9
    # a surface NaN: two iterations reach +-(2 + 4) pixels and the 3 x 3 of the variance twice more, inside one class; the
    # wall of normal (1,0,0) is never crossed by a tap, and crossed by the variance only
    m = ac.nonfinite_mask("film_nan_surface").any(-1)
    assert m[4, 8] and not m[:, 25:].any() and m[:, :20].sum() > 50
    m5 = ac.nonfinite_mask("film_nan_surface_it5").any(-1)
    assert (m5 | ~m).all() and m5.sum() > m.sum()


def _b3_blur(u, iterations):
    """The normalised B3 blur at steps 1, 2, 4, .. with loops over pixels and taps, taps outside the image skipped."""
    H, W = u.shape[:2]
    for it in range(iterations):
        h, out = 1 << it, np.zeros_like(u)
        for y in range(H):
            for x in range(W):
                num, den = np.zeros(3), 0.0
                for j in range(5):
                    for i in range(5):
                        qy, qx = y + (j - 2) * h, x + (i - 2) * h
                        if 0 <= qy < H and 0 <= qx < W:
                            num += dr.B3[j] * dr.B3[i] * u[qy, qx]
                            den += dr.B3[j] * dr.B3[i]
                out[y, x] = num / den
        u = out
    return u


@pytest.mark.parametrize("name", ["sigma_off_9x33_it5", "sigma_off_5x7_it12"])
def test_all_stops_off_is_the_normalised_b3_blur(name):
    c = ac.BY_NAME[name]
    a = np.maximum(c.feat[..., 0:3].astype(np.float64), 1e-3)
    want = _b3_blur(c.film.astype(np.float64) / a, c.dn["iterations"]) * a
    assert np.allclose(ac.reference(name), want, rtol=1e-12, atol=0)


@pytest.mark.parametrize("name", ["sigma_off_1x9_it5", "sigma_off_1x512_it12", "sigma_off_512x1_it12"])
def test_a_one_pixel_wide_image_is_the_blur_in_one_dimension(name):
    c = ac.BY_NAME[name]
    a = np.maximum(c.feat[..., 0:3].astype(np.float64), 1e-3).reshape(-1, 3)
    u = c.film.astype(np.float64).reshape(-1, 3) / a
    n = len(u)
    for it in range(c.dn["iterations"]):
        h, out = 1 << it, np.zeros_like(u)
        for x in range(n):
            taps = [(dr.B3[i], x + (i - 2) * h) for i in range(5) if 0 <= x + (i - 2) * h < n]
            out[x] = sum(w * u[q] for w, q in taps) / sum(w for w, _ in taps)
        u = out
    assert np.allclose(ac.reference(name).reshape(-1, 3), u * a, rtol=1e-12, atol=0)


def test_a_miss_pixel_is_its_input_for_every_sigma():
    for name in ("feat_miss_checker", "feat_miss_halves"):
        c = ac.BY_NAME[name]
        miss = ~(c.feat[..., 4:7] != 0).any(-1)
        assert miss.any() and not miss.all()
        for sig in (dict(), dict(sigma_n=0.0), dict(sigma_l=0.0), dict(sigma_d=0.0), ac.OFF, dict(sigma_l=0.0, sigma_n=0.0, sigma_d=0.0)):
            out = ac.evaluate(c, **sig)
            assert np.allclose(out[miss], c.film[miss].astype(np.float64), rtol=1e-15, atol=0), (name, sig)
            assert not np.allclose(out[~miss], c.film[~miss], rtol=1e-3) or sig.get("sigma_l") == 0.0


def test_sigma_n_zero_does_not_mix_orthogonal_halves_or_opposite_normals():
    """n_p.n_q <= 0 is weight 0 for every sigma_n, 0 included (0^0 is not consulted): the dark half stays exactly 0, and with
    every stop off each class of a checkerboard of opposite normals is blurred on its own."""
    c = ac.BY_NAME["feat_ortho_halves_sn0"]
    for sig in (c.dn, dict(c.dn, **ac.OFF)):
        out = dr.denoise(c.film, c.feat, **sig)
        assert not out[:, :16].any() and out[:, 16:].all()
        assert not np.allclose(out[:, 16:], c.film[:, 16:], rtol=1e-3)          # (the lit half does mix)
    c = ac.BY_NAME["feat_opposite_checker_sn0"]
    out = dr.denoise(c.film, c.feat, **dict(c.dn, iterations=1, **ac.OFF))
    front = c.feat[..., 6] > 0
    a = np.maximum(c.feat[..., 0:3].astype(np.float64), 1e-3)
    u = c.film / a
    H, W = front.shape
    for y, x in ((0, 0), (4, 16), (8, 32), (3, 7)):
        num, den = np.zeros(3), 0.0
        for j in range(5):
            for i in range(5):
                qy, qx = y + j - 2, x + i - 2
                if 0 <= qy < H and 0 <= qx < W and front[qy, qx] == front[y, x]:
                    num += dr.B3[j] * dr.B3[i] * u[qy, qx]
                    den += dr.B3[j] * dr.B3[i]
        assert np.allclose(out[y, x], num / den * a[y, x], rtol=1e-12)


def test_an_excluded_tap_is_not_read():
    """A NaN or an infinity at a tap of weight 0 by one of the rule's cases stays out of the sum (a selection, not 0 * x):
    with a finite variance at every pixel, the surfaces see exactly the film without its emitters and miss pixels."""
    c = ac.BY_NAME["feat_emitter_quarter"]
    feat = c.feat.copy()
    feat[0:3, 25:30] = ac.MISS
    out_of_it = (feat[..., 3] > 0) | ~(feat[..., 4:7] != 0).any(-1)
    film = c.film.copy()
    film[out_of_it] = np.nan
    film[7, 20] = np.inf
    u, a = dr.demodulate(film, feat)
    var = np.full(out_of_it.shape, 0.25)
    for sig in ((4.0, 128.0, 0.025), (0.0, 0.0, 0.0), (3e38, 0.0, 3e38)):
        for h in (1, 4, 64):
            got, gv = dr.atrous_step(u, var, feat, h, *sig)
            want, wv = dr.atrous_step(np.where(out_of_it[..., None], 0.0, u), var, feat, h, *sig)
            assert np.isfinite(got[~out_of_it]).all() and np.isfinite(gv).all()
            assert np.array_equal(got[~out_of_it], want[~out_of_it]) and np.array_equal(gv, wv)
            assert np.array_equal(np.isnan(got), np.isnan(u)) and np.array_equal(np.isinf(got), np.isinf(u))
