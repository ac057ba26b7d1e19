"""The case table of tests/upsample_cases.py without a GPU: the conditions that make the table meaningful (lattice pixels where
it says there are, protected and unprotected pixels, planted NaNs), and pt_upsample_host -- the rule header as the host
compiler builds it -- against the f64 restatement on every case and sigma pair: the same non-finite set, everything else
within 1e-4; class isolation under a poisoned film, bit for bit; the non-finite pixels exactly where the rule's decisions put
them."""
import numpy as np
import pytest

import upsample_cases as uc
import upsample_ref as ur


@pytest.fixture(scope="module")
def host(pt):
    """pt_upsample_host on (case name, sigma index), computed once per module (read-only)"""
    done = {}

    def run(name, k):
        if (name, k) not in done:
            c = uc.BY_NAME[name]
            lin, rgba = pt.upsample_host(c.c, c.f, c.F, *c.sigmas[k])
            lin.setflags(write=False)
            done[name, k] = (lin, rgba)
        return done[name, k]

    return run


# ---------------------------------------------------------------- the table
def test_the_table_covers_the_shape_pairs_and_stays_small():
    assert set(uc.SHAPES) == {(c.full, c.low) for c in uc.CASES if c.family == "crafted"} and len(set(uc.SHAPES)) == 18
    assert max(c.F.shape[0] * c.F.shape[1] for c in uc.CASES) <= 17000
    assert sum(W * H for (W, H), _ in uc.SHAPES) < 45000
    assert {c.family for c in uc.CASES} == set(uc.FAMILIES)
    for c in uc.CASES:
        (W, H), (w, h) = c.full, c.low
        assert c.c.shape == (h, w, 3) and c.f.shape == (h, w, 8) and c.F.shape == (H, W, 8)
        assert all(np.isfinite(s) and s >= 0 for pair in c.sigmas for s in pair)
        if c.family == "exact":
            assert all(sd == 0.0 for _, sd in c.sigmas)


@pytest.mark.parametrize("full,low", uc.ODD_RATIO)
def test_odd_ratios_put_pixels_on_the_low_lattice(full, low):
    """(W - 1) / (w - 1) an odd integer: X is an integer at some columns, so fx = 0 and the right-hand taps are skipped"""
    for n_full, n_low, flipped, want in ((full[0], low[0], False, uc.LATTICE[full, low][0]), (full[1], low[1], True, uc.LATTICE[full, low][1])):
        X0, fr = ur.position(n_full, n_low, flipped)
        assert int((fr == 0).sum()) == want
        assert ((X0[fr == 0] >= 0) & (X0[fr == 0] < n_low)).all()


def test_the_five_earlier_pairs_have_lattice_pixels_in_the_identities_only():
    """(what the table adds; beside the odd ratios, an even size from an even size has the one pixel in the middle: 32 x 8 from 16 x 4)"""
    for full, low in ur.SHAPES:
        for n_full, n_low, flipped in ((full[0], low[0], False), (full[1], low[1], True)):
            zero = int((ur.position(n_full, n_low, flipped)[1] == 0).sum())
            assert zero == (n_full if n_full == n_low else 0), (full, low)
    assert [int((ur.position(a, b, fl)[1] == 0).sum()) for a, b, fl in ((32, 16, False), (8, 4, True))] == [1, 1]


@pytest.mark.parametrize("pair", [uc.HARD, uc.SMALL], ids=["67x35", "16x10"])
def test_poison_cases_have_protected_and_unprotected_pixels(pair):
    tag = uc._tag(*pair)
    c = uc.BY_NAME["poison_i_nan_" + tag]
    _, info = uc.reference(c.name, 0)
    keep = uc.protected(c, info)
    assert keep.mean() >= 0.25 and (~keep).sum() >= 1
    assert np.isnan(c.c).any(-1).sum() == (ur.classes(c.f) != ur.SURFACE).sum() > 0
    ref, _ = uc.reference("poison_iii_nan_" + tag, 0)
    bad = ~np.isfinite(ref).all(-1)
    assert bad.any() and bad.mean() < 0.5
    for name in uc.POISONS:
        assert ("poison_ii_%s_%s" % (name, tag)) in uc.BY_NAME


def test_one_class_low_images_leave_no_pixel_a_tap_of_its_own():
    for kind, cls in (("miss", ur.MISS), ("emitter", ur.EMITTER)):
        c = uc.BY_NAME[f"degenerate_low_all_{kind}_" + uc._tag(*uc.HARD)]
        assert (ur.classes(c.f) == cls).all()
        _, info = uc.reference(c.name, 0)
        other = ur.classes(c.F) != cls
        assert other.any() and (~other).any()
        assert not info["own"][other].any() and info["own"][~other].all()
    c = uc.BY_NAME["degenerate_low_checker_" + uc._tag(*uc.HARD)]
    assert min(int((ur.classes(c.f) == k).sum()) for k in (0, 1, 2)) >= 200


def test_wild_cases_plant_a_nan_and_keep_the_normals_short():
    wild = [c for c in uc.CASES if "_wild_" in c.name]
    assert len(wild) == 16
    base = ur.crafted_inputs(6, *uc.HARD)
    for c in wild:
        side, ref = (c.f, base[1]) if "_low_" in c.name else (c.F, base[2])
        changed = (side.view(np.uint32) != ref.view(np.uint32)).any(-1)
        assert np.isnan(side).any() and 0.01 < changed.mean() < 0.06, c.name
        n = side[..., 4:7].astype(np.float64)
        with np.errstate(invalid="ignore"):
            assert not ((n * n).sum(-1) > 1.0 + 1e-6).any(), c.name
        if "normal" not in c.name:
            assert np.isinf(side).any(), c.name


def test_degenerate_depths_and_normals_are_what_their_names_say():
    tag = uc._tag(*uc.HARD)
    tiny = np.finfo(np.float32).tiny
    d = uc.BY_NAME["degenerate_depth_denormal_" + tag].F[..., 7]
    assert ((d == 0) | ((d > 0) & (d < tiny))).all() and (d > 0).mean() > 0.5
    assert (uc.BY_NAME["degenerate_depth_negative_" + tag].F[..., 7] <= 0).all()
    assert uc.BY_NAME["degenerate_depth_1e30_" + tag].F[..., 7].max() > 1e30 and 0 < uc.BY_NAME["degenerate_depth_1e-30_" + tag].F[..., 7].max() < 1e-28
    c = uc.BY_NAME["degenerate_normals_1e-20_" + tag]
    nd = (c.F[:18, :34, 4:7] * c.f[..., 4:7]).sum(-1)                # f32 products: denormal
    assert ((nd == 0) | (np.abs(nd) < tiny)).all() and (nd != 0).mean() > 0.5
    assert not uc.BY_NAME["degenerate_albedo_zero_" + tag].F[..., 0:3].any()


# ---------------------------------------------------------------- pt_upsample_host against the restatement
@pytest.mark.parametrize("name", uc.NAMES)
def test_host_entry_is_the_restatement_on_every_case(host, name):
    c = uc.BY_NAME[name]
    for k, (sn, sd) in enumerate(c.sigmas):
        lin, rgba = host(name, k)
        ref, _ = uc.reference(name, k)
        same, err = uc.compare(lin, ref)
        print(f"upsample case {name} sigma_n {sn:g} sigma_d {sd:g}: max rel err {err:.2e}, {int((~np.isfinite(lin)).sum())} non-finite")
        assert same, (name, sn, sd)
        assert err <= uc.BAR, (name, sn, sd)


@pytest.mark.parametrize("name", [n for n in uc.NAMES if n.startswith("exact_")])
def test_exact_family_has_no_weight_between_0_and_b(name):
    """sigma_d = 0 on the palette: the restatement's surface weights are b_q or 0 whatever sigma_n is, so every sigma pair of
    the family gives the same picture, and the host entry gives it bit for bit across the pairs"""
    c = uc.BY_NAME[name]
    for k in range(1, len(c.sigmas)):
        assert np.array_equal(uc.reference(name, k)[0], uc.reference(name, 0)[0])


@pytest.mark.parametrize("pair", [uc.HARD, uc.SMALL], ids=["67x35", "16x10"])
@pytest.mark.parametrize("poison", list(uc.POISONS))
def test_a_poisoned_tap_of_another_class_never_reaches_a_protected_pixel(pt, host, pair, poison):
    """family poison (i): whatever the low film holds under the emitter and miss records, a surface pixel with a surface tap
    keeps the bits it has with the clean film (0 x NaN would be NaN: rule 5 does not read a tap with w_q = 0)"""
    c = uc.BY_NAME[f"poison_i_{poison}_" + uc._tag(*pair)]
    clean = ur.crafted_inputs(5, *pair)[0]
    for k, (sn, sd) in enumerate(c.sigmas):
        base, base_rgba = pt.upsample_host(clean, c.f, c.F, sn, sd)
        got, rgba = host(c.name, k)
        keep = uc.protected(c, uc.reference(c.name, k)[1])
        assert np.isfinite(base[keep]).all()
        assert np.array_equal(got[keep].view(np.uint32), base[keep].view(np.uint32)), (sn, sd, int((got[keep] != base[keep]).any(-1).sum()))
        assert np.array_equal(rgba[keep], base_rgba[keep])
        if poison != "denormal":                      # (a denormal film value under a record is a small film value: it may vanish in the sums)
            assert not uc.same_bits(got[~keep], base[~keep])


@pytest.mark.parametrize("pair", [uc.HARD, uc.SMALL], ids=["67x35", "16x10"])
@pytest.mark.parametrize("poison", ["nan", "pinf", "ninf"])
def test_lone_poisoned_pixels_reach_exactly_the_pixels_that_read_them(host, pair, poison):
    """family poison (iii): a pixel is non-finite if and only if a poisoned tap is its anchor or has w_q > 0"""
    c = uc.BY_NAME[f"poison_iii_{poison}_" + uc._tag(*pair)]
    mask = ~np.isfinite(c.c).all(-1)
    assert 0 < mask.sum() < 0.1 * mask.size
    for k in range(len(c.sigmas)):
        want = uc.predicted_nonfinite(uc.reference(c.name, k)[1], mask)
        got = ~np.isfinite(host(c.name, k)[0])
        assert np.array_equal(got.any(-1), want) and np.array_equal(got.all(-1), want), c.sigmas[k]
        assert 0 < want.mean() < 0.5
