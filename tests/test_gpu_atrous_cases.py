"""pt_denoise_device and pt_denoise_var_device on the case table of tests/atrous_cases.py: every case against the f64
restatement under the bar of tests/test_gpu_denoise.py (1e-4, of which the table's admission condition leaves the
restatement's own f32 evaluation a quarter), and the statements that hold exactly, compared as bits (a NaN equals a NaN:
its payload is no part of the rule)."""
import numpy as np
import pytest

import atrous_cases as ac
import denoise_ref as dr

pytestmark = pytest.mark.gpu
BAR = 1e-4


def _run(ctx, case, **override):
    dn = dict(case.dn, **override)
    if case.var is None:
        return ctx.denoise(case.film, case.feat, **dn)
    return ctx.denoise_var(case.film, case.feat, case.var, **dn)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != np.float32:
        return np.array_equal(a, b)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


@pytest.mark.parametrize("name", ac.NAMES)
def test_case_matches_the_f64_restatement(pt, gpu_ctx, name):
    c = ac.BY_NAME[name]
    lin, rgba = _run(gpu_ctx, c)
    ref = ac.reference(name)
    err = ac.max_rel(lin, ref)
    print(f"atrous case {name} family {c.family}: max rel err {err:.2e}, {int((~np.isfinite(ref)).sum())} non-finite")
    assert lin.dtype == np.float32 and lin.shape == ref.shape
    assert np.array_equal(~np.isfinite(lin), ac.nonfinite_mask(name))
    assert err <= BAR
    with np.errstate(invalid="ignore"):
        assert np.array_equal(rgba, dr.rgba8(lin))
    # emitters and pixels without a tap of n_p.n_q > 0 (every miss pixel) come out as iterations = 0 gives them
    keep = ac.untouched(c)
    if keep.any():
        lin0, rgba0 = _run(gpu_ctx, c, iterations=0)
        assert _same_bits(lin[keep], lin0[keep]) and np.array_equal(rgba[keep], rgba0[keep])


@pytest.mark.parametrize("iterations", [1, 5, 16])
def test_a_one_pixel_image_is_its_input(gpu_ctx, iterations):
    c = ac.BY_NAME["size_1x1"]
    for sig in (dict(), ac.OFF, dict(sigma_l=0.0, sigma_n=0.0, sigma_d=0.0)):
        assert _same_bits(_run(gpu_ctx, c, iterations=iterations, **sig)[0], _run(gpu_ctx, c, iterations=0)[0])


@pytest.mark.parametrize("name,enough,more", [("steps_5x7_it16", 4, (6, 12, 16)), ("steps_9x33_it16", 7, (12, 16)),
                                               ("sigma_off_1x9_it5", 5, (6, 16))])
def test_steps_past_the_image_change_nothing(gpu_ctx, name, enough, more):
    """From iteration ceil(log2 max(H, W)) on every tap but the centre lies outside: u_p + 0."""
    c = ac.BY_NAME[name]
    assert (1 << (enough - 1)) >= max(c.film.shape[:2]) > (1 << (enough - 2))
    want = _run(gpu_ctx, c, iterations=enough)
    assert not _same_bits(want[0], _run(gpu_ctx, c, iterations=enough - 2)[0])
    for it in more:
        got = _run(gpu_ctx, c, iterations=it)
        assert _same_bits(got[0], want[0]) and np.array_equal(got[1], want[1]), it


@pytest.mark.parametrize("name", [n for n in ac.NAMES if "_distinct_" in n])
def test_a_stop_of_1e10_between_distinct_values_lets_nothing_through(gpu_ctx, name):
    """sigma_l = 0 with all luminances distinct, sigma_d = 0 with all depths distinct: every weight exp(-1e8 ..) = 0."""
    c = ac.BY_NAME[name]
    for it in (1, 5, 12):
        got, want = _run(gpu_ctx, c, iterations=it), _run(gpu_ctx, c, iterations=0)
        assert _same_bits(got[0], want[0]) and np.array_equal(got[1], want[1])


@pytest.mark.parametrize("size", ac.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_an_all_nan_plane_is_pt_denoise_device(gpu_ctx, size):
    c = ac.BY_NAME[f"size_{size[0]}x{size[1]}"]
    for it in (1, 5):
        a = gpu_ctx.denoise(c.film, c.feat, iterations=it)
        b = gpu_ctx.denoise_var(c.film, c.feat, np.full(size, np.nan, np.float32), iterations=it)
        assert _same_bits(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("name", [n for n in ac.NAMES if n.startswith("var_const_")])
def test_a_constant_image_stays_within_2_ulp(gpu_ctx, name):
    c = ac.BY_NAME[name]
    ulp = np.spacing(np.float32(0.375))
    for it in (5, 12):
        out, _ = _run(gpu_ctx, c, iterations=it)
        assert np.abs(out - c.film).max() <= 2 * ulp, np.abs(out - c.film).max() / ulp


def test_one_context_across_every_shape(pt):
    """The context-owned (u, var) planes grow, serve smaller images and change roles an odd or even number of times: the
    whole table twice in shuffled orders on one context gives the bits of a fresh context per case."""
    fresh = {}
    for c in ac.CASES:
        ctx = pt.Context(0)
        try:
            fresh[c.name] = _run(ctx, c)
        finally:
            ctx.close()
    ctx = pt.Context(0)
    try:
        for seed in (1, 2):
            for k in np.random.default_rng(seed).permutation(len(ac.CASES)):
                c = ac.CASES[k]
                lin, rgba = _run(ctx, c)
                assert _same_bits(lin, fresh[c.name][0]) and np.array_equal(rgba, fresh[c.name][1]), (seed, c.name)
    finally:
        ctx.close()


@pytest.mark.parametrize("name", ["steps_2x512_it12", "steps_5x7_it16", "feat_miss_checker"])
def test_the_first_temporal_frame_is_the_spatial_filter(pt, gpu_ctx, name):
    """after pt_temporal_reset every pixel is fresh, u = u_c with the 3 x 3 variance, and the step loop is shared
    (a camera is at least 2 x 2, so the strip is two pixels high)."""
    c = ac.BY_NAME[name]
    H, W = c.film.shape[:2]
    gpu_ctx.temporal_reset()
    got = gpu_ctx.denoise_temporal(pt.camera_new(width=W, height=H), c.film, c.feat, **c.dn)
    gpu_ctx.temporal_reset()
    want = _run(gpu_ctx, c)
    assert _same_bits(got[0], want[0]) and np.array_equal(got[1], want[1])
