"""Temporal accumulation in front of the a-trous filter without a device: the ABI (symbols, defaults, the argument checks
that come before the context is looked at), the numpy restatement (tests/temporal_ref.py) against properties the rule
implies, and the inputs of tests/temporal_cases.py against what they claim: the share of pixels that a GPU comparison
may skip is a property of the inputs, so it is checked here."""
import ctypes as C

import numpy as np

import pytest

import denoise_ref as dr
import temporal_cases as tc
import temporal_ref as tr

NEW = ("pt_default_temporal", "pt_temporal_reset", "pt_denoise_temporal_device", "pt_render_denoised_temporal")


def test_the_new_symbols_are_exported(pt):
    lib = pt._lib.lib()
    for name in NEW:
        assert name in pt._lib.SYMBOLS and hasattr(lib, name), name
    assert lib.pt_abi_version() == 6
    assert [f[0] for f in pt._lib.PtTemporal._fields_] == ["alpha", "depth_tol", "normal_tol"]
    assert C.sizeof(pt._lib.PtTemporal) == 12


def test_default_temporal_is_the_documented_rule(pt):
    t = pt._lib.PtTemporal()
    pt._lib.lib().pt_default_temporal(C.byref(t))
    assert (t.alpha, t.depth_tol, t.normal_tol) == (np.float32(0.2), np.float32(0.1), np.float32(0.9))
    t = pt.default_temporal(alpha=0.5)
    assert (t.alpha, t.depth_tol, t.normal_tol) == (0.5, np.float32(0.1), np.float32(0.9))
    pt._lib.lib().pt_default_temporal(None)          # ignored, no crash


def test_null_and_out_of_range_arguments_are_rejected_without_a_device(pt):
    lib = pt._lib.lib()
    cam = pt.camera_new(width=8, height=8)
    prm = pt.default_params(spp=4)
    dn = pt.default_denoise()
    buf = (C.c_float * 512)()
    out = (C.c_float * 512)()

    def call(cam=C.byref(cam), lin=buf, feat=buf, dn=C.byref(dn), tp=None, out=out):
        t = pt.default_temporal() if tp is None else tp
        return lib.pt_denoise_temporal_device(None, cam, lin, feat, dn, C.byref(t), out, None), lib.pt_last_error()

    assert lib.pt_temporal_reset(None) == 1
    assert call()[0] == 1 and b"null context" in call()[1]          # every other argument is fine
    for kw in ({"cam": None}, {"lin": None}, {"feat": None}, {"dn": None}, {"out": None}):
        rc, msg = call(**kw)
        assert rc == 1 and b"null argument" in msg, kw
    assert lib.pt_denoise_temporal_device(None, C.byref(cam), buf, buf, C.byref(dn), None, out, None) == 1
    for bad in ({"alpha": -0.1}, {"alpha": 1.5}, {"alpha": float("nan")}, {"depth_tol": -1.0}, {"depth_tol": float("inf")},
                {"normal_tol": -0.5}, {"normal_tol": float("nan")}):
        rc, msg = call(tp=pt.default_temporal(**bad))
        assert rc == 1 and b"null context" not in msg, (bad, msg)
    for ok in ({"alpha": 0.0}, {"alpha": 1.0}, {"depth_tol": 0.0, "normal_tol": 0.0}):
        assert b"null context" in call(tp=pt.default_temporal(**ok))[1], ok
    rc, msg = call(cam=C.byref(pt.camera_new(width=1, height=8)))
    assert rc == 1 and b"2" in msg
    rc, msg = call(dn=C.byref(pt.default_denoise(iterations=17)))
    assert rc == 1 and b"iterations" in msg
    rc, msg = call(out=buf)
    assert rc == 1 and b"output" in msg
    t = pt.default_temporal()
    assert lib.pt_render_denoised_temporal(None, C.byref(cam), C.byref(prm), 4, C.byref(dn), C.byref(t), buf, None, None, None) == 1
    assert lib.pt_render_denoised_temporal(None, C.byref(cam), None, 4, C.byref(dn), None, buf, None, None, None) == 1


def _feat(H, W, albedo=0.5, normal=(0.0, 0.0, 1.0), depth=2.0):
    f = np.zeros((H, W, 8))
    f[..., 0:3] = albedo
    f[..., 4:7] = normal
    f[..., 7] = depth
    return f


def test_restatement_first_frame_is_the_spatial_filter(pt):
    rng = np.random.default_rng(1)
    c, f = dr.random_inputs(rng, 13, 11)
    cam = pt.camera_new(width=11, height=13)
    for it in (0, 2):
        out, _, info = tr.step(c, f, None, cam, iterations=it)
        assert info["fresh"].all()
        assert np.allclose(out, dr.denoise(c, f, iterations=it), rtol=1e-13, atol=0)


def test_restatement_static_camera_is_the_running_mean(pt):
    rng = np.random.default_rng(2)
    H, W = 9, 12
    cam = pt.camera_new(width=W, height=H)
    f = _feat(H, W, albedo=0.4)
    hist, films = None, []
    for k in range(6):
        c = rng.uniform(0, 1, (H, W, 3))
        films.append(c)
        out, hist, info = tr.step(c, f, hist, cam, alpha=0.0, iterations=0)
        assert info["fresh"].all() if k == 0 else not info["fresh"].any()
        assert np.allclose(out, np.mean(films, 0), rtol=1e-12)
        assert np.all(hist["n"] == k + 1)
    # alpha = 1 keeps only the current frame
    out, hist, _ = tr.step(films[0], f, hist, cam, alpha=1.0, iterations=0)
    assert np.allclose(out, films[0], rtol=1e-12)


def test_restatement_integer_pixel_translation(pt):
    """A wall facing the camera; the camera moves by exactly 3 pixel footprints at the wall's depth."""
    H, W = 20, 24
    cam0 = pt.camera_new(width=W, height=H)
    zw = -1.0
    Z = cam0.origin[2] - zw
    step_x = cam0.horizontal[0] / (W - 1) * Z / (cam0.origin[2] - cam0.lower_left[2])
    step_y = cam0.vertical[1] / (H - 1) * Z / (cam0.origin[2] - cam0.lower_left[2])
    rng = np.random.default_rng(3)
    for axis, cam1 in (("x", pt.camera_new(origin=(3 * step_x, 0.0, 2.0), width=W, height=H)),
                       ("y", pt.camera_new(origin=(0.0, 3 * step_y, 2.0), width=W, height=H))):
        f0, f1 = tr.wall_features(cam0, zw), tr.wall_features(cam1, zw)
        c0, c1 = rng.uniform(0.1, 1, (H, W, 3)), rng.uniform(0.1, 1, (H, W, 3))
        _, hist, _ = tr.step(c0, f0, None, cam0, alpha=0.0, iterations=0)
        out, _, info = tr.step(c1, f1, hist, cam1, alpha=0.0, iterations=0)
        if axis == "x":                     # a point at column x now was at column x + 3
            assert info["fresh"][:, W - 3:].all() and not info["fresh"][:, :W - 3].any()
            assert np.allclose(out[:, :W - 3], 0.5 * (c0[:, 3:] + c1[:, :W - 3]), rtol=1e-9)
            assert np.allclose(out[:, W - 3:], c1[:, W - 3:], rtol=1e-12)
        else:                               # camera up: a point at row y now was at row y - 3 (rows run top-down)
            assert info["fresh"][:3].all() and not info["fresh"][3:].any()
            assert np.allclose(out[3:], 0.5 * (c0[:H - 3] + c1[3:]), rtol=1e-9)
            assert np.allclose(out[:3], c1[:3], rtol=1e-12)


def test_restatement_fresh_after_reset_size_change_and_misses(pt):
    rng = np.random.default_rng(4)
    H, W = 10, 14
    cam = pt.camera_new(width=W, height=H)
    f = _feat(H, W)
    f[2:4, 3:6, 7] = 0.0                     # misses
    c = rng.uniform(0, 1, (H, W, 3))
    _, hist, _ = tr.step(c, f, None, cam, iterations=0)
    _, hist2, info = tr.step(c, f, hist, cam, iterations=0)
    assert info["fresh"][2:4, 3:6].all() and info["fresh"].sum() == 6
    assert np.all(hist2["n"][2:4, 3:6] == 1) and np.all(hist2["n"][f[..., 7] > 0] == 2)
    other = pt.camera_new(width=W + 1, height=H)
    f2 = _feat(H, W + 1)
    _, _, info = tr.step(rng.uniform(0, 1, (H, W + 1, 3)), f2, hist2, other, iterations=0)
    assert info["fresh"].all()
    # a history tap behind a depth, normal or emitter edge is not taken
    for key, val in (("depth", 3.0), ("normal", (1.0, 0.0, 0.0)), ("emitter", 1.0)):
        f3 = f.copy()
        if key == "depth":
            f3[..., 7] = np.where(f[..., 7] > 0, val, 0.0)
        elif key == "normal":
            f3[..., 4:7] = val
        else:
            f3[..., 3] = val
        _, _, info = tr.step(c, f3, hist, cam, iterations=0)
        assert info["fresh"].all(), key


# ------------------------------------------------------------------------------------------- the margin of the n >= 4 hand-over
def _six_frames(pt, move_before=None):
    W, H = 24, 20
    cam0 = pt.camera_new(width=W, height=H)
    sx, sy = tc.footprint(cam0)
    cam1 = pt.camera_new(origin=(0.4 * sx, 0.3 * sy, 2.0), width=W, height=H)
    res, hist = [], None
    for k, c in enumerate(tc.films(5, 6, H, W)):
        cam = cam1 if move_before is not None and k >= move_before else cam0
        _, hist, info = tr.step(c, tr.wall_features(cam, tc.ZW), hist, cam, iterations=0)
        res.append((hist, info))
    return res


def test_restatement_static_camera_crosses_n_4_without_an_unsafe_pixel(pt):
    """An unmoved camera takes one tap of weight 1: n = hn + 1 is the same integer in f32 and f64, at n = 4 too."""
    for k, (hist, info) in enumerate(_six_frames(pt)):
        assert np.all(hist["n"] == k + 1)
        assert np.all(np.isinf(info["margins"]["n"]))
        safe, frac = tr.safe_mask(info)
        assert frac == 1.0 and safe.all(), k


def test_restatement_n_margin_stays_zero_where_the_count_is_a_mixture(pt):
    """The camera moves by (0.4, 0.3) pixels before frame 3: n = 4 there is a bilinear mixture of 3s divided by S, which
    f32 and f64 round to either side of 4.  Later frames of the then unmoved camera inherit the inexact count."""
    res = _six_frames(pt, move_before=3)
    for k in (0, 1, 2):
        assert np.all(np.isinf(res[k][1]["margins"]["n"]))
    hist, info = res[3]
    took = ~info["fresh"]
    assert took.mean() > 0.9
    assert np.all(np.abs(hist["n"][took] - 4) < 1e-12)
    assert np.all(info["margins"]["n"][took] < 1e-12)
    assert np.all(np.isinf(info["margins"]["n"][info["fresh"]]))          # n = 1 exactly
    assert tr.safe_mask(info)[1] < 0.1
    for k in (4, 5):                              # the camera stands again, the count it inherits is still a mixture
        hist, info = res[k]
        m = info["margins"]["n"][took]
        assert np.all(np.isfinite(m)) and np.allclose(m, k + 1 - 4, atol=1e-12)


# ------------------------------------------------------------------------------------------------- the cases of temporal_cases
def _compared(info, iters):
    """The pixels test_moving_sequences_match_the_f64_restatement would compare in a frame whose history is all safe."""
    safe, frac = tr.safe_mask(info, iterations=iters)
    return frac, float(safe.mean())


@pytest.mark.parametrize("iters", [0, 2])
@pytest.mark.parametrize("params", ["default", "random"])
def test_wall_sequence_is_safe_everywhere_and_crosses_n_4(pt, params, iters):
    kw = dict(tc.RANDOM) if params == "random" else {}
    frames = tc.wall_sequence(pt)
    hist = None
    for k, (cam, c, f) in enumerate(frames):
        _, hist, info = tr.step(c, f, hist, cam, iterations=iters, **kw)
        assert tr.safe_mask(info)[1] == 1.0, k
        n = hist["n"]
        if k < 5:
            assert np.all(n == k + 1) and info["fresh"].all() == (k == 0)
        else:
            assert info["fresh"].sum() == 254, (k, info["fresh"].sum())
            assert n.min() == 1 and abs(n.max() - (k + 1)) < 1e-9
            mixed = np.abs(n - np.round(n)) > 1e-3                      # mixtures of old and new counts at the incoming edges,
            assert mixed.sum() >= (100 if k > 5 else 0)                 # once a frame with fresh pixels is the history
    assert len(frames) == 12


@pytest.mark.parametrize("which", [0, 1, 2])
def test_gate_frames_sit_a_known_distance_from_every_gate(pt, which):
    frames = tc.gate_frames(pt)
    for i in range(len(tc.GATE_BLOCKS)):                               # blocks >= 4 pixels from each other and the border
        ys, xs = tc.gate_block(i)
        assert ys.start >= 4 and xs.start >= 4 and ys.stop <= tc.GATE_H - 4 and xs.stop <= tc.GATE_W - 4
        for j in range(i):
            yj, xj = tc.gate_block(j)
            assert max(ys.start - yj.stop, yj.start - ys.stop, xs.start - xj.stop, xj.start - xs.stop) >= 4
    (_, _), (out, info) = tc.run_ref(frames, iterations=0, **tc.GATE_PARAMS[which])
    exp, taken = tc.gate_expected(which)
    assert np.array_equal(~info["fresh"], taken)
    assert np.allclose(out, exp[..., None], rtol=1e-12, atol=0)
    assert taken.any() and (~taken).any()
    for i, (name, e) in enumerate(tc.GATE_BLOCKS):
        assert np.all(taken[tc.gate_block(i)] == e[which]), name
    m = info["margins"]
    if which < 2:
        assert tr.safe_mask(info)[1] == 1.0
        # the stated factors scale the current depth, and the gate is relative to it: x 1.12 is 0.1071, 0.007 outside 0.1
        assert m["depth"].min() > (0.007 if which == 0 else 0.02) and m["normal"].min() > 0.0199
        for i, (name, _) in enumerate(tc.GATE_BLOCKS):
            if name.startswith("depth /"):
                assert m["depth"][tc.gate_block(i)].min() > 0.0199, name
    else:
        # depth_tol = 0 and normal_tol = 0 put equal depths and the perpendicular normal ON the threshold, on purpose.  The
        # operands are the same f32 numbers there (a difference of exactly 0, a dot product of exactly 0), so the decision
        # is exact although its margin is 0; every other decision is at least 0.02 away
        for k in ("depth", "normal"):
            assert np.all((m[k] == 0.0) | (m[k] > 0.0199)), k
        assert np.all(m["S"] > 1e-3) and np.all(np.isinf(m["n"]) & np.isinf(m["inside"]) & np.isinf(m["reproj"]))


@pytest.mark.parametrize("shift", tc.THIN_SHIFTS)
def test_thin_tap_frames_leave_one_tap_of_the_stated_weight(pt, shift):
    frames = tc.thin_tap_frames(pt, shift)
    for iters in (0, 2):
        (_, _), (out, info) = tc.run_ref(frames, iterations=iters)
        frac, cmp = _compared(info, iters)
        assert frac >= 0.99 and cmp >= 0.9, (iters, frac, cmp)
    assert info["margins"]["S"].min() >= 0.005 - 1e-7
    S = tc.thin_tap_S(shift)
    for k in range(4):
        col = info["fresh"][:, k::4]
        assert np.all(col == (S[k] < 1e-2)), (k, S[k])
    # a taken pixel of weight S < 1 is the blend with that ONE column's history, renormalised: alpha' = 1/2
    k = 3 if shift < 0.5 else 0                    # the thin column class: tap x + 1 (weight shift) or tap x (weight 1 - shift)
    if S[k] >= 1e-2:
        (_, c0, _), (_, c1, _) = frames
        (_, _), (out, _) = tc.run_ref(frames, iterations=0)
        xs = np.arange(k, tc.THIN_W - 1, 4)
        src = xs + 1 if shift < 0.5 else xs
        want = 0.5 * (c0[1:-1, src].astype(np.float64) + c1[1:-1, xs])
        assert np.allclose(out[1:-1, xs], want, rtol=1e-9)
        assert not np.allclose(out[1:-1, xs], 0.5 * (S[k] * c0[1:-1, src] + c1[1:-1, xs]), rtol=1e-2)


def test_camera_pairs_are_safe_and_cover_what_they_claim(pt):
    pairs = tc.camera_pairs(pt)
    assert {(f[1][0].width, f[1][0].height) for f in pairs.values()} >= {(2, 2), (33, 9), (97, 61)}
    fresh = {}
    for name, frames in pairs.items():
        for iters in (0, 2):
            (_, _), (_, info) = tc.run_ref(frames, iterations=iters)
            frac, cmp = _compared(info, iters)
            assert frac >= 0.99 and cmp >= 0.9, (name, iters, frac, cmp)
        fresh[name] = float(info["fresh"].mean())
    for name in ("yaw 2 deg", "fov 30 -> 35", "33 x 9", "97 x 61"):      # history for most pixels, none for some
        assert 0.0 < fresh[name] < 0.3, (name, fresh[name])
    for name in ("fov 35 -> 30", "dolly 0.3"):
        assert fresh[name] == 0.0, name
    for name in ("120 footprints", "2 x 2", "turned round"):
        assert fresh[name] == 1.0, name
    # the turned camera is rejected by lambda <= 0 alone: its reprojections lie inside the previous image, on valid
    # history of the expected depth and normal
    (prev, _, fp), (cur, _, fc) = pairs["turned round"]
    xr, yr, dexp, lam, ok = tr.reproject(cur, prev, fc[..., 7].astype(np.float64))
    assert not ok.any() and np.all(lam < 0)
    inside = (xr > 0) & (xr < cur.width - 1) & (yr > 0) & (yr < cur.height - 1)
    assert inside.mean() > 0.9 and np.all(fp[..., 7] > 0)
    assert np.abs(fp[..., 7].astype(np.float64)[::-1, ::-1] - dexp).max() < 0.1 * dexp.min()
    # one tap column inside the image: reprojections in (-1, 0) or (W - 1, W)
    for name in ("yaw 2 deg", "97 x 61", "33 x 9"):
        (prev, _, _), (cur, _, fc) = pairs[name]
        xr, yr, _, _, ok = tr.reproject(cur, prev, fc[..., 7].astype(np.float64))
        half = ok & (((xr > -1) & (xr < 0)) | ((xr > cur.width - 1) & (xr < cur.width))) & (yr > 0) & (yr < cur.height - 1)
        assert half.sum() >= 3, (name, half.sum())
