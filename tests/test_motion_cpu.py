"""The host side of the temporal denoiser's motion entry (pt_scene_update, pt_debug_motion_maps, the new symbols) without a
GPU, and the committed GPU cases (tests/motion_cases.py) on the f64 restatement (tests/motion_ref.py) alone."""
import ctypes as C

import numpy as np
import pytest

import motion_cases as mc
import motion_ref as mr

NEW = ("pt_scene_update", "pt_debug_motion_maps", "pt_render_feature_ids_device", "pt_denoise_temporal_motion_device",
       "pt_render_denoised_motion")


def test_new_symbols_are_bound_and_fail_loudly_without_a_context(pt):
    lib = pt._lib.lib()
    assert lib.pt_abi_version() == 6                      # additive: the version stays
    for name in NEW:
        assert name in pt._lib.SYMBOLS and getattr(lib, name)
    objs = pt.builtin_scene(1)
    cam = pt.camera_new(width=8, height=8)
    prm, dn, tp = pt.default_params(spp=1), pt.default_denoise(), pt.default_temporal()
    buf = np.zeros(8 * 8 * 8, np.float32)
    p = buf.ctypes.data_as(C.c_void_p)
    assert lib.pt_scene_update(None, objs, len(objs)) != 0
    assert b"pt_scene_update" in lib.pt_last_error()
    assert lib.pt_render_feature_ids_device(None, C.byref(cam), C.byref(prm), p) != 0
    assert lib.pt_denoise_temporal_motion_device(None, C.byref(cam), p, p, p, C.byref(dn), C.byref(tp), p, None) != 0
    assert b"pt_denoise_temporal_motion_device" in lib.pt_last_error()
    assert lib.pt_render_denoised_motion(None, C.byref(cam), C.byref(prm), 1, C.byref(dn), C.byref(tp), p, None, None, None, None) != 0
    assert lib.pt_debug_motion_maps(None, objs, len(objs), None, None) != 0
    for m in ("scene_update", "feature_ids", "denoise_temporal_motion", "render_denoised_motion"):
        assert callable(getattr(pt.Context, m))


def _well_conditioned_triangle(rng):
    """cond(E) <= 100 by construction: E = Q diag(s) R-ish with singular values in [1/6, 6] ... checked, redrawn otherwise."""
    while True:
        v0 = rng.uniform(-5, 5, 3)
        e1, e2 = rng.normal(size=3) * rng.uniform(0.3, 3), rng.normal(size=3) * rng.uniform(0.3, 3)
        n = np.cross(e1, e2)
        if np.linalg.norm(n) == 0:
            continue
        E = np.stack([e1, e2, n / np.linalg.norm(n)], 1)
        if np.linalg.cond(E) <= 100:
            return tuple(v0) + tuple(v0 + e1) + tuple(v0 + e2)


def _random_scene(rng, n):
    specs = []
    for k in range(n):
        if k % 2:
            specs.append((0, tuple(rng.uniform(-5, 5, 3)) + (rng.uniform(0.1, 3),)) + mc.GREY)
        else:
            specs.append((1, _well_conditioned_triangle(rng)) + mc.GREY)
    return specs


def _walls(pt):
    return [(o.shape_tag, tuple(o.shape[k] for k in range(9 if o.shape_tag else 4)), 0, (0.5, 0.5, 0.5)) for o in pt.builtin_scene(1)]


def _moved(rng, specs):
    """Every object rotated, scaled and translated (a sphere: moved and resized)."""
    out = []
    for tag, v, mt, mv in specs:
        v = np.array(v, float)
        if tag == 0:
            out.append((0, tuple(v[0:3] + rng.uniform(-1, 1, 3)) + (v[3] * rng.uniform(0.5, 2),), mt, mv))
        else:
            q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
            t = rng.uniform(-1, 1, 3)
            out.append((1, tuple(np.concatenate([q @ v[3 * i:3 * i + 3] * 1.3 + t for i in range(3)])), mt, mv))
    return out


def test_maps_match_the_restatement(pt):
    rng = np.random.default_rng(5)
    cur = _random_scene(rng, 40) + _walls(pt)
    prev = _moved(rng, cur)
    A, b, flags = pt.motion_maps(pt.make_objects(prev), pt.make_objects(cur))
    pp, tags = mc.pose(prev)
    pc, _ = mc.pose(cur)
    rA, rb, rf = mr.maps(pp, pc, tags)
    assert np.array_equal(flags, rf) and not flags.any()
    worst = 0.0
    for k in range(len(cur)):
        scale = max(1.0, np.abs(rA[k]).max(), np.abs(rb[k]).max())
        worst = max(worst, max(np.abs(A[k] - rA[k]).max(), np.abs(b[k] - rb[k]).max()) / scale)
    print(f"max |delta| / max(1, |A|, |b|) = {worst:.2e}")
    assert worst <= 1e-12
    # the maps reach: triangle corners and v0 + n -> their primed counterparts, a sphere's surface -> the primed sphere's
    for k, (sp, sc) in enumerate(zip(prev, cur)):
        vp, vc = np.array(sp[1], float), np.array(sc[1], float)
        if sc[0] == 1:
            def unit(v):
                n = np.cross(v[3:6] - v[0:3], v[6:9] - v[0:3])
                return n / np.linalg.norm(n)
            src = [vc[0:3], vc[3:6], vc[6:9], vc[0:3] + unit(vc)]
            dst = [vp[0:3], vp[3:6], vp[6:9], vp[0:3] + unit(vp)]
        else:
            u = rng.normal(size=3)
            u /= np.linalg.norm(u)
            src, dst = [vc[0:3] + vc[3] * u], [vp[0:3] + vp[3] * u]
        for s, d in zip(src, dst):
            assert np.abs(A[k] @ s + b[k] - d).max() <= 1e-10 * max(1.0, np.abs(d).max()), (k, s, d)


def test_identity_and_invalid_flags(pt):
    tri = (1, (0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0)) + mc.GREY
    sph = (0, (0.1, 0.2, 0.3, 0.5)) + mc.GREY
    there = (0, (0.1 + 0.7, 0.2, 0.3, 0.5)) + mc.GREY
    back = (0, (0.1 + 0.7 - 0.7, 0.2, 0.3, 0.5)) + mc.GREY              # moved and moved back: 0.1 again only if the bits are
    nearly = (0, (np.nextafter(0.1, 1.0), 0.2, 0.3, 0.5)) + mc.GREY
    flat = (1, (0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 2.0, 0.0, 0.0)) + mc.GREY
    nan = (1, (0.0, 0.0, 0.0, 1.0, float("nan"), 0.0, 0.0, 1.0, 0.0)) + mc.GREY
    r0 = (0, (0.1, 0.2, 0.3, 0.0)) + mc.GREY
    prev = [tri, sph, sph, sph, sph, tri, flat, tri, nan, sph, r0]
    cur = [tri, sph, there, back, nearly, flat, tri, nan, tri, r0, sph]
    A, b, flags = pt.motion_maps(pt.make_objects(prev), pt.make_objects(cur))
    same_bits = [np.array(p[1], float).tobytes() == np.array(c[1], float).tobytes() for p, c in zip(prev, cur)]
    assert same_bits[:5] == [True, True, False, back[1] == sph[1], False]
    assert [bool(f & 1) for f in flags] == same_bits
    assert [bool(f & 2) for f in flags] == [False] * 5 + [True] * 6
    assert np.array_equal(A[0], np.eye(3)) and not b[0].any() and np.array_equal(A[1], np.eye(3)) and not b[1].any()
    pp, tags = mc.pose(prev)
    assert np.array_equal(mr.maps(pp, mc.pose(cur)[0], tags)[2], flags)
    # an unchanged degenerate object is both
    _, _, f2 = pt.motion_maps(pt.make_objects([flat, r0]), pt.make_objects([flat, r0]))
    assert list(f2) == [3, 3]


@pytest.mark.parametrize("name", mc.CASES)
def test_committed_cases_are_margin_safe(pt, name):
    """At least 95 % of every frame's pixels have no decision within 1e-4 of flipping: what the GPU tests may skip."""
    frames, kw = mc.case(pt, name)
    res = mc.run_ref(frames, iterations=0, **kw)
    for k, (_, info) in enumerate(res):
        frac = mr.safe_mask(info)[1]
        print(f"{name} frame {k}: safe {frac:.4f}, fresh {info['fresh'].mean():.3f}")
        assert frac >= 0.95, (name, k, frac)
    # and what they compare: those, less the pixels that read an unsafe pixel's history, less the a-trous footprint
    for it, least in mc.COMPARED.items():
        for k, (m, _) in enumerate(mr.compared([info for _, info in res], it)):
            assert m.mean() >= least or m.all(), (name, it, k, float(m.mean()))
    if name == "sphere":
        # pixels uncovered behind the sphere are fresh, pixels the sphere moves onto are not
        for k in range(1, len(frames)):
            ids0, ids1 = frames[k - 1][3], frames[k][3]
            fresh = res[k][1]["fresh"]
            assert fresh[(ids0 == 1) & (ids1 == 0)].all()
            onto = (ids0 == 0) & (ids1 == 1)
            assert onto.sum() >= 10 and not fresh[onto].any()
    if name == "seam":
        ids0, ids1 = frames[0][3], frames[1][3]
        unc = (ids0 < 2) & (ids1 >= 2)
        assert unc.sum() >= 100 and res[1][1]["fresh"][unc].all()
        assert not res[1][1]["fresh"][(ids0 < 2) & (ids1 < 2) & (ids0 == ids1)].all()
    if name == "rotation":
        hit = frames[1][3] >= 0
        assert (~res[1][1]["fresh"][hit]).mean() > 0.8          # kept through n_h; n_p would fail normal_tol = 0.99
    if name == "hostile":
        assert res[1][1]["fresh"][10:].all() and not res[1][1]["fresh"][:10].any()
