"""pt_upsample_device on the case table of tests/upsample_cases.py: k_upsample against the f64 restatement on every case and
sigma pair (the same non-finite set, everything else within 1e-4), against pt_upsample_host -- the same rule header as the host
compiler builds it -- bit for bit wherever no exp2f / log2f reaches the value, the RGBA8 plane, class isolation under a
poisoned film, the non-finite pixels exactly where the rule's decisions put them, the call without an RGBA8 plane, and the
one-call entry against its five parts at the least, the identical and an odd-ratio low size."""
import ctypes as C

import numpy as np
import pytest

import denoise_ref as dr
import upsample_cases as uc
import upsample_ref as ur

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def device(gpu_ctx):
    """pt_upsample_device on (case name, sigma index), one launch each, kept for the module (read-only)"""
    done = {}

    def run(name, k):
        if (name, k) not in done:
            c = uc.BY_NAME[name]
            lin, rgba = gpu_ctx.upsample(c.c, c.f, c.F, *c.sigmas[k])
            lin.setflags(write=False)
            done[name, k] = (lin, rgba)
        return done[name, k]

    return run


@pytest.fixture(scope="module")
def host(pt):
    done = {}

    def run(name, k):
        if (name, k) not in done:
            c = uc.BY_NAME[name]
            done[name, k] = pt.upsample_host(c.c, c.f, c.F, *c.sigmas[k])
        return done[name, k]

    return run


@pytest.mark.parametrize("name", uc.NAMES)
def test_kernel_matches_the_f64_restatement_on_every_case(device, name):
    c = uc.BY_NAME[name]
    for k, (sn, sd) in enumerate(c.sigmas):
        lin, _ = device(name, k)
        ref, _ = uc.reference(name, k)
        same, err = uc.compare(lin, ref)
        print(f"upsample case {name} sigma_n {sn:g} sigma_d {sd:g}: max rel err {err:.2e}, {int((~np.isfinite(lin)).sum())} non-finite")
        assert lin.dtype == np.float32 and lin.shape == ref.shape
        assert same, (name, sn, sd)
        assert err <= uc.BAR, (name, sn, sd)


@pytest.mark.parametrize("name", uc.NAMES)
def test_kernel_against_the_host_entry(device, host, name):
    """The linear plane bit for bit on the exact family, on every miss and emitter pixel and on every pixel without a tap of
    its class (weights b_q or 0, f64 sums, IEEE divisions: nothing the two compilers may do differently); on the other pixels
    glibc's and the device's exp2f / log2f meet, and the distance is printed, not bounded: the bar there is the restatement's.
    The RGBA8 plane: equal bytes wherever the linear bits agree, and everywhere the transform of the device's own linear plane."""
    c = uc.BY_NAME[name]
    cls = ur.classes(c.F)
    for k, (sn, sd) in enumerate(c.sigmas):
        (lin, rgba), (h_lin, h_rgba) = device(name, k), host(name, k)
        _, info = uc.reference(name, k)
        plain = np.ones(cls.shape, bool) if c.family == "exact" else (cls != ur.SURFACE) | ~info["own"]
        rest = ~plain
        print(f"upsample case {name} family {c.family} sigma_n {sn:g} sigma_d {sd:g}: {int(plain.sum())} pixels bit for bit, "
              f"device-host distance on the other {int(rest.sum())}: {uc.ulp_distance(lin[rest], h_lin[rest])} ulp")
        assert uc.same_bits(lin[plain], h_lin[plain]), (name, sn, sd, int(plain.sum()))
        nan, h_nan = np.isnan(lin), np.isnan(h_lin)
        agree = ((lin.view(np.uint32) == h_lin.view(np.uint32)) | (nan & h_nan)).all(-1)
        assert np.array_equal(rgba[agree], h_rgba[agree])
        with np.errstate(invalid="ignore"):
            assert np.array_equal(rgba, dr.rgba8(lin))


def test_rgba8_of_the_values_no_film_should_hold(device):
    """NaN and negative -> 0, +inf -> 255 (ptone::unorm8), on pixels the table is known to have"""
    c = uc.BY_NAME["poison_ii_nan_" + uc._tag(*uc.HARD)]
    lin, rgba = device(c.name, 0)
    assert np.isnan(lin).any() and (rgba[..., 0:3][np.isnan(lin)] == 0).all() and (rgba[..., 3] == 255).all()
    lin, rgba = device("poison_ii_pinf_" + uc._tag(*uc.HARD), 0)
    assert np.isposinf(lin).any() and (rgba[..., 0:3][np.isposinf(lin)] == 255).all()
    for name in ("poison_ii_ninf_", "poison_ii_negative_"):
        lin, rgba = device(name + uc._tag(*uc.HARD), 0)
        assert (lin < 0).any() and (rgba[..., 0:3][lin < 0] == 0).all()


@pytest.mark.parametrize("pair", [uc.HARD, uc.SMALL], ids=["67x35", "16x10"])
@pytest.mark.parametrize("poison", list(uc.POISONS))
def test_a_poisoned_tap_of_another_class_never_reaches_a_protected_pixel(gpu_ctx, device, pair, poison):
    c = uc.BY_NAME[f"poison_i_{poison}_" + uc._tag(*pair)]
    clean = ur.crafted_inputs(5, *pair)[0]
    for k, (sn, sd) in enumerate(c.sigmas):
        base, base_rgba = gpu_ctx.upsample(clean, c.f, c.F, sn, sd)
        got, rgba = device(c.name, k)
        keep = uc.protected(c, uc.reference(c.name, k)[1])
        assert np.isfinite(base[keep]).all()
        assert np.array_equal(got[keep].view(np.uint32), base[keep].view(np.uint32)), (sn, sd, int((got[keep] != base[keep]).any(-1).sum()))
        assert np.array_equal(rgba[keep], base_rgba[keep])
        if poison != "denormal":
            assert not uc.same_bits(got[~keep], base[~keep])


@pytest.mark.parametrize("pair", [uc.HARD, uc.SMALL], ids=["67x35", "16x10"])
@pytest.mark.parametrize("poison", ["nan", "pinf", "ninf"])
def test_lone_poisoned_pixels_reach_exactly_the_pixels_that_read_them(device, pair, poison):
    c = uc.BY_NAME[f"poison_iii_{poison}_" + uc._tag(*pair)]
    mask = ~np.isfinite(c.c).all(-1)
    for k in range(len(c.sigmas)):
        want = uc.predicted_nonfinite(uc.reference(c.name, k)[1], mask)
        got = ~np.isfinite(device(c.name, k)[0])
        assert np.array_equal(got.any(-1), want) and np.array_equal(got.all(-1), want), c.sigmas[k]


@pytest.mark.parametrize("name", ["crafted_" + uc._tag(*uc.ODD_RATIO[3]), "poison_iii_nan_" + uc._tag(*uc.SMALL)])
def test_a_call_without_the_rgba8_plane_gives_the_same_linear_bits(pt, gpu_ctx, device, name):
    c = uc.BY_NAME[name]
    (W, H), (w, h) = c.full, c.low
    up = pt.default_upsample(sigma_n=c.sigmas[0][0], sigma_d=c.sigmas[0][1])
    d_lo, d_lo_feat, d_feat = gpu_ctx._upload(c.c, np.float32, (h, w, 3)), gpu_ctx._upload(c.f, np.float32, (h, w, 8)), gpu_ctx._upload(c.F, np.float32, (H, W, 8))
    out = gpu_ctx._empty((H, W, 3))
    gpu_ctx._on_stream(pt._lib.lib().pt_upsample_device, w, h, d_lo, d_lo_feat, W, H, d_feat, C.byref(up), out, None)
    assert uc.same_bits(out.cpu().numpy(), device(name, 0)[0])


@pytest.mark.parametrize("lo_size", [(2, 2), (64, 48), (22, 48)], ids=["least", "identity", "odd_ratio_x"])
def test_the_one_call_is_its_five_parts_at_the_edges_of_the_low_size(pt, gpu_ctx, lo_size):
    """C2 at 4 spp, full 64 x 48: from 2 x 2, from 64 x 48 itself, and from 22 x 48 (63 / 21 = 3 in x, y unscaled)"""
    gpu_ctx.upload(pt.builtin_scene(2))
    cam = pt.camera_new(width=64, height=48)
    lo_cam = pt._lib.PtCamera.from_buffer_copy(cam)
    lo_cam.width, lo_cam.height = lo_size
    prm = pt.default_params(spp=4, spp_offset=3)
    lin, rgba, lo, feat = gpu_ctx.render_denoised_upsampled(cam, prm, lo_size, 4)
    noisy = gpu_ctx.render(lo_cam, prm)[0].cpu().numpy()
    lo_feat = gpu_ctx.render_features(lo_cam, prm, 4)
    ref_lo, _ = gpu_ctx.denoise(noisy, lo_feat)
    ref_feat = gpu_ctx.render_features(cam, prm, 4)
    ref_lin, ref_rgba = gpu_ctx.upsample(ref_lo, lo_feat, ref_feat)
    assert np.array_equal(lo, ref_lo) and np.array_equal(feat, ref_feat)
    assert np.array_equal(lin.view(np.uint32), ref_lin.view(np.uint32)) and np.array_equal(rgba, ref_rgba)
    assert ur.max_rel(lin, ur.upsample(ref_lo, lo_feat, ref_feat)) <= uc.BAR
