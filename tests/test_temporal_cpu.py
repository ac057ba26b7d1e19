"""Temporal accumulation in front of the a-trous filter without a device: the ABI (symbols, defaults, the argument checks
that come before the context is looked at) and the numpy restatement (tests/temporal_ref.py) against properties the rule
implies."""
import ctypes as C

import numpy as np

import denoise_ref as dr
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
