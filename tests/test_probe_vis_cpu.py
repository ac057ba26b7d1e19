"""The irradiance volume's probe visibility on the CPU (pt_probe_moments_host, pt_probe_shade_visibility_host) against
the numpy restatement of the rule (tests/probe_vis_ref.py), bit for bit; the octahedral map's round trip and wrap; the cases where
the term must vanish; a two-probe case with a closed form; the leak scene's geometry; and the refusals that need no device."""
import ctypes as C

import numpy as np
import pytest

import probe_grid_ref as pr
import probe_vis_ref as pv

INVALID = 1
U = 2.0 ** -53


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _vis(pt, T=8, k=5, max_distance=1.0):
    return pt.default_probe_visibility(None, resolution=T, sharpness_log2=k, max_distance=max_distance)


def _shade(pt, cam, g, sh, maps, feat, fallback, bias, weight=pr.TRILINEAR):
    return pt.probe_shade_visibility_host(pr.pt_camera(pt, cam), g.as_pt(pt), sh, maps, _vis(pt, maps.shape[1]), feat, fallback,
                                          pt.default_probe_shade(normal_bias=bias, weight=weight))


def _facing(pt, cam, g, sh, feat, fallback, bias):
    return pt.probe_shade_host(pr.pt_camera(pt, cam), g.as_pt(pt), sh, feat, fallback, pt.default_probe_shade(normal_bias=bias, weight=pr.FACING))


def test_symbols_and_defaults(pt):
    lib = pt._lib.lib()
    for name in ("pt_default_probe_visibility", "pt_probe_distances_device", "pt_probe_distances_host", "pt_probe_moments_device",
                 "pt_probe_moments_host", "pt_probe_grid_visibility_device", "pt_probe_shade_visibility_device", "pt_probe_shade_visibility_host",
                 "pt_render_probe_lit_visibility_device", "pt_render_probe_lit_visibility_host"):
        assert name in pt._lib.SYMBOLS and hasattr(lib, name), name
    assert C.sizeof(pt._lib.PtProbeVisibility) == 16 and lib.pt_abi_version() == 6
    v = pt.default_probe_visibility()
    assert (v.resolution, v.sharpness_log2, v.max_distance) == (8, 5, 1.0)
    g = pr.Grid((0, 0, 0), (3.0, 4.0, 12.0), (2, 2, 2))
    assert pt.default_probe_visibility(g.as_pt(pt)).max_distance == np.float32(1.5 * 13.0)
    assert pt.default_probe_visibility(pr.Grid((0, 0, 0), (3.0, 0.0, 4.0), (2, 1, 2)).as_pt(pt)).max_distance == np.float32(7.5)
    assert pt.default_probe_visibility(pr.Grid((0, 0, 0), (1, -1, 1), (2, 2, 2)).as_pt(pt)).max_distance == 1.0      # an invalid grid


@pytest.mark.parametrize("T", [2, 8, 16])
@pytest.mark.parametrize("R", [1, 63, 256, 300])
def test_moments_against_the_restatement(pt, R, T):
    dirs = pt.probe_directions(R)
    for k, md in ((0, 0.75), (5, 2.0), (8, 1.0)):
        t = pv.hostile_distances(3, R, md, seed=R + T + k)
        t[0, 0] = np.inf
        want = pv.moments(t, dirs, T, k, md)
        got = pt.probe_moments_host(t, _vis(pt, T, k, md))
        assert got.shape == (3, T, T, 2) and np.array_equal(_bits(got), _bits(want)), (R, T, k)
        assert np.isfinite(got).all() and (got[..., 0] >= 0).all() and (got[..., 0] <= np.float32(md)).all()      # (0: w 1e-30 underflows)
    # no ray in a texel's hemisphere (one ray, k = 0: the lower texels see it with weight 0): (max_distance, max_distance^2)
    if R == 1:
        got = pt.probe_moments_host(np.array([[0.25]], dtype=np.float32), _vis(pt, T, 0, 0.75))
        empty = pv.texel_dirs(T) @ dirs[0].astype(np.float64) <= 0.0
        assert empty.any() and (got[0][empty] == (np.float32(0.75), np.float32(0.5625))).all() and (got[0][~empty, 0] == 0.25).all()


@pytest.mark.parametrize("name", sorted(pr.GRIDS))
@pytest.mark.parametrize("size", pr.SIZES)
def test_shade_against_the_restatement(pt, name, size):
    W, H = size
    cam, g, sh, feat, fallback = pr.make_case(name, W, H, seed=11)
    seen = []
    for T in (2, 8, 16):
        maps = pv.random_maps(pr.count(g), T, seed=T)
        for bias, fb in ((0.0, fallback), (0.05, None)):
            det = {}
            want, want8, lit = pv.shade(cam, g, sh, maps, feat, fb, bias, det)
            got, got8 = _shade(pt, cam, g, sh, maps, feat, fb, bias)
            assert np.array_equal(_bits(got), _bits(want)), (name, size, T, bias)
            assert np.array_equal(got8, want8) and np.isfinite(want).all() and (det["den"] > 0).all()
            seen.append(det["vis"])
            # the weight field is not read
            again = _shade(pt, cam, g, sh, maps, feat, fb, bias, weight=pr.FACING)[0]
            assert np.array_equal(_bits(again), _bits(got))
    vis = np.concatenate([v.ravel() for v in seen])
    assert (vis == 1.0).any() and (vis < 0.5).any() and ((vis >= 0) & (vis <= 1)).all()      # both sides of the Chebyshev test


@pytest.mark.parametrize("T", [2, 8, 16])
def test_encode_inverts_decode_at_every_texel_centre(T):
    """Roundings between a centre and its round trip, all on quantities of magnitude <= sqrt 3 whose effect on the result has a gain
    <= 1: decode 2 (z) + 1 (the fold) + 5 (the dot) + 1 (sqrt) + 1 (reciprocal) + 3 (the products; all three enter the encoder's sum)
    = 13, encode 2 (the sum) + 1 (the division) + 1 (the fold) = 4: |error| <= 17 * 2^-53 * sqrt 3 to first order."""
    j, i = np.meshgrid(np.arange(T), np.arange(T), indexing="ij")
    u, v = pv.centre(T, i), pv.centre(T, j)
    eu, ev = pv.oct_encode(pv.oct_decode(u, v))
    bound = 17 * U * np.sqrt(3.0)
    err = max(np.abs(eu - u).max(), np.abs(ev - v).max())
    print("T", T, "round-trip error", err / U, "u; bound", bound / U, "u")
    assert err <= bound
    d = pv.oct_decode(u, v)
    assert np.abs(np.sqrt((d * d).sum(-1)) - 1.0).max() <= 4 * U


@pytest.mark.parametrize("T", [2, 8, 16])
def test_out_of_map_taps_resolve_to_neighbouring_directions(T):
    """Every tap across an edge, and from T = 4 on every corner's diagonal tap, lands no further from the texel it was taken from than
    4-neighbours inside the map are apart.  At T = 2 the four texels ARE the four corners, the diagonally opposite one is the
    antipode (pi away, against pi / 2 between 4-neighbours): there the diagonal tap is only checked to resolve by the rule."""
    d = pv.texel_dirs(T)

    def angle(a, b):
        return np.arccos(np.clip((a * b).sum(-1), -1.0, 1.0))

    inside = max(angle(d[:, 1:], d[:, :-1]).max(), angle(d[1:], d[:-1]).max())      # the largest angle between 4-neighbours of the map
    n = 0
    for j in range(T):
        for i in range(T):
            for di, dj in ((-1, 0), (1, 0), (0, -1), (0, 1), (-1, -1), (1, -1), (-1, 1), (1, 1)):
                ti, tj = i + di, j + dj
                out_i, out_j = not 0 <= ti < T, not 0 <= tj < T
                if not (out_i or out_j) or (di and dj and not (out_i and out_j)):
                    continue                                  # inside; or a diagonal that is not a corner's
                wi, wj = pv.wrap(T, ti, tj)
                assert 0 <= wi < T and 0 <= wj < T
                if T > 2 or not (di and dj):
                    assert angle(d[wj, wi], d[j, i]) <= inside * (1 + 1e-12), (T, i, j, ti, tj)
                n += 1
    assert n == 4 * T + 4                      # one tap across the edge per edge position, and each corner's diagonal
    assert tuple(int(x) for x in pv.wrap(T, -1, -1)) == (T - 1, T - 1) and tuple(int(x) for x in pv.wrap(T, T, 1)) == (T - 1, T - 2)
    assert tuple(int(x) for x in pv.wrap(T, 1, -1)) == (T - 2, 0) and tuple(int(x) for x in pv.wrap(T, 0, T)) == (T - 1, T - 1)


@pytest.mark.parametrize("name", sorted(pr.GRIDS))
def test_far_or_broken_maps_are_the_facing_weight(pt, name):
    cam, g, sh, feat, fallback = pr.make_case(name, 33, 17, seed=3)
    feat[5, 5, 1] = np.inf
    feat[6, 6, 5] = np.nan
    feat[7, 7, 3] = 0.25
    P = pr.count(g)
    far = pv.random_maps(P, 8, seed=1, far=1e3)
    broken = far.copy()
    broken[..., 0].flat[::3] = np.nan
    broken[..., 0].flat[1::3] = np.inf
    broken[..., 1].flat[2::3] = -np.inf
    for bias, fb in ((0.0, fallback), (0.05, None)):
        want, want8 = _facing(pt, cam, g, sh, feat, fb, bias)
        for maps in (far, broken):
            got, got8 = _shade(pt, cam, g, sh, maps, feat, fb, bias)
            assert np.array_equal(_bits(got), _bits(want)) and np.array_equal(got8, want8)
    lit = pr.shade(cam, g, sh, feat)[2]
    assert (~lit).sum() == 7
    # a NaN coefficient: NaN in every lit pixel, the fallback bit for bit elsewhere; no moment of an unlit pixel is read
    nan_sh = np.full_like(sh, np.nan)
    got = _shade(pt, cam, g, nan_sh, pv.random_maps(P, 8, seed=2), feat, fallback, 0.0)[0]
    assert np.isnan(got[lit]).all() and np.array_equal(_bits(got)[~lit], _bits(fallback)[~lit])


def _two_probe_case():
    """Probe A at x = 0, probe B at x = 1 (one probe on the other axes).  Every pixel's point lies in the plane z = 0 with
    0.17 < x < 0.38 and |y| < 0.13: further than 0.6 from B, and with B's trilinear weight f <= 0.45."""
    g = pr.Grid((0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (2, 1, 1))
    W = H = 5
    o = np.array([0.25, 0.0, 1.0])
    cam = (o, o + np.array([-0.1, -0.1, -1.0]), np.array([0.2, 0.0, 0.0]), np.array([0.0, 0.2, 0.0]), W, H)
    feat = np.zeros((H, W, 8), dtype=np.float32)
    feat[..., 0:3] = 0.5
    feat[..., 6] = 1.0
    D = pr.points(cam, np.ones((H, W), dtype=np.float32)) - o
    feat[..., 7] = (1.0 / -D[..., 2]).astype(np.float32)
    return g, cam, feat


def test_an_occluded_probe_drops_out(pt):
    g, cam, feat = _two_probe_case()
    P = pr.points(cam, feat[..., 7])
    assert (np.abs(P[..., 2]) < 1e-6).all() and (P[..., 0] > 0.17).all() and (P[..., 0] < 0.38).all()
    assert (np.linalg.norm(P - np.array([1.0, 0.0, 0.0]), axis=-1) > 0.6).all()
    a, b = np.float32(1.0), np.float32(3.0)
    sh = np.zeros((2, 9, 3), dtype=np.float32)
    sh[0, 0], sh[1, 0] = a, b
    only_a = np.zeros_like(sh)
    only_a[:, 0] = a
    T = 8
    maps = pv.random_maps(2, T, seed=0, far=1e3)
    maps[1, ..., 0], maps[1, ..., 1] = 0.5, 0.25                      # B: a surface at 0.5, no variance
    got = _shade(pt, cam, g, sh, maps, feat, None, 0.0)[0]
    want_a = _facing(pt, cam, g, only_a, feat, None, 0.0)[0]        # a constant field comes out exactly
    # vis_B = 0, so g_B = (1e-6)^3 / 0.04 = 2.5e-17 against g_A = F_A >= 0.2, and tri_B / tri_A <= 0.45 / 0.55: the blend is off A's
    # value by at most (0.45 / 0.55) (2.5e-17 / 0.2) |b - a| / a = 2.1e-16 of it, and by three f64 roundings of the blend: below
    # 1e-15 in all, far inside half an f32 ulp -- the rounding to f32 moves the value by one ulp at the most.
    leak = (0.45 / 0.55) * (2.5e-17 / 0.2) * abs(float(b) - float(a)) / float(a) + 3 * U
    assert leak < 1e-15
    ulp = np.spacing(want_a)
    print("occluded probe: largest deviation", float((np.abs(got - want_a) / ulp).max()), "f32 ulp")
    assert (want_a > 0).all() and (np.abs(got.astype(np.float64) - want_a) <= ulp).all()
    # the same through the restatement, bit for bit
    assert np.array_equal(_bits(got), _bits(pv.shade(cam, g, sh, maps, feat)[0]))
    # B's map far: the FACING blend
    maps[1] = maps[0]
    got = _shade(pt, cam, g, sh, maps, feat, None, 0.0)[0]
    want = _facing(pt, cam, g, sh, feat, None, 0.0)[0]
    assert np.array_equal(_bits(got), _bits(want)) and (got > want_a).all()


def test_the_leak_scene_puts_the_dark_pixels_behind_the_wall():
    """tests/test_gpu_probe_vis.py's leak scene, before any GPU time: with hand-made maps that say "the wall's plane x = 0" towards
    +x for the lit-side probes, every dark-side floor point is beyond the wall as those probes see it (r > m1, so vis < 1, everywhere; how far below 1 is
    the maps' business: these are bilinear in a distance that varies across a texel, and the Chebyshev bound is soft where that
    variance is not small against the distance behind the wall), and every lit-side floor point is in front of it (vis = 1)."""
    L = pv.LEAK
    g = L["grid"]
    pos = pr.positions(g).astype(np.float64)
    T = 16
    d = pv.texel_dirs(T)
    with np.errstate(all="ignore"):
        wall = np.where(d[..., 0] > 1e-9, -pos[:, None, None, 0] / d[None, ..., 0], 1e3)      # distance along the texel direction to x = 0
    wall = np.where((pos[:, None, None, 0] < 0) & (wall > 0) & (wall < L["max_distance"]), wall, L["max_distance"])
    maps = np.stack([wall, wall * wall], axis=-1).astype(np.float32)
    lit_side = np.nonzero(pos[:, 0] < 0)[0]
    near = pos[lit_side, 0].max()
    for region, hidden in (("dark", True), ("lit", False)):
        x0, x1, z0, z1 = L[region]
        xs, zs = np.meshgrid(np.linspace(x0, x1, 9), np.linspace(z0, z1, 9))
        Q = np.stack([xs.ravel(), np.zeros(81), zs.ravel()], axis=1)
        for p in lit_side:
            if abs(pos[p, 0] - near) > 1e-6:
                continue                                                    # the probes of the cell that holds the strip
            vis = pv.visibility(maps, np.full(81, p), Q, np.broadcast_to(pos[p], (81, 3)))
            if hidden:
                assert (vis < 1.0).all(), (region, p, vis.max())
            elif np.linalg.norm(Q - pos[p], axis=1).max() < L["max_distance"]:
                assert (vis == 1.0).all(), (region, p, vis.min())


def test_refusals_that_need_no_device(pt):
    L = pt._lib.lib()
    g = pr.GRIDS["2x2x2"]
    cam, _, sh, feat, fallback = pr.make_case("2x2x2", 33, 17, seed=1)
    c, pg, sp = pr.pt_camera(pt, cam), g.as_pt(pt), pt.default_probe_shade()
    maps = pv.random_maps(8, 8, seed=0)
    out, out8 = np.zeros((17, 33, 3), dtype=np.float32), np.zeros((17, 33, 4), dtype=np.uint8)
    dist, mom = np.ones((2, 16), dtype=np.float32), np.zeros((2, 8, 8, 2), dtype=np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)

    def refused(rc, text):
        assert rc == INVALID and text in L.pt_last_error().decode(), L.pt_last_error().decode()

    def shade(vis, moments=maps, **kw):
        a = dict(cam=C.byref(c), grid=C.byref(pg), sh=p(sh), feat=p(feat), out=p(out))
        a.update(kw)
        return L.pt_probe_shade_visibility_host(a["cam"], a["grid"], a["sh"], None if moments is None else p(moments),
                                                None if vis is None else C.byref(vis), a["feat"], None, C.byref(sp), a["out"], p(out8))

    bad = [(dict(resolution=1), "resolution"), (dict(resolution=17), "resolution"), (dict(sharpness_log2=9), "sharpness_log2"),
           (dict(max_distance=0.0), "max_distance"), (dict(max_distance=-1.0), "max_distance"), (dict(max_distance=float("nan")), "max_distance"),
           (dict(max_distance=float("inf")), "max_distance")]
    for over, text in bad:
        v = pt.default_probe_visibility(None, **over)
        refused(shade(v), "pt_probe_shade_visibility_host: " + text)
        refused(L.pt_probe_moments_host(p(dist), 2, 16, C.byref(v), p(mom)), "pt_probe_moments_host: " + text)
        refused(L.pt_probe_moments_device(None, p(dist), 2, 16, C.byref(v), p(mom)), "pt_probe_moments_device: " + text)
    v = pt.default_probe_visibility()
    assert shade(v) == 0
    refused(shade(None), "null argument")
    refused(shade(v, moments=None), "the moments plane")
    refused(shade(v, sh=None), "sh27")
    refused(shade(v, out=None), "the linear output")
    refused(shade(v, grid=C.byref(pr.Grid((0, 0, 0), (1, -1, 1), (2, 2, 2)).as_pt(pt))), "invalid probe grid")
    sp.weight = 2
    refused(shade(v), "unknown weight")
    sp.weight = 0
    refused(L.pt_probe_moments_host(None, 2, 16, C.byref(v), p(mom)), "the distances plane")
    refused(L.pt_probe_moments_host(p(dist), 2, 16, C.byref(v), None), "the moments plane")
    refused(L.pt_probe_moments_host(p(dist), 2, 16, None, p(mom)), "null argument")
    refused(L.pt_probe_moments_host(p(dist), 0, 16, C.byref(v), p(mom)), "n_probes")
    refused(L.pt_probe_moments_host(p(dist), 2, 0, C.byref(v), p(mom)), "rays_per_probe")
    refused(L.pt_probe_moments_host(p(dist), 2, 65536, C.byref(v), p(mom)), "rays_per_probe")
    # device entries refuse what they can before they look at the context: a moments plane that is not 8-byte aligned, a null context
    refused(L.pt_probe_moments_device(None, p(dist), 2, 16, C.byref(v), C.c_void_p(mom.ctypes.data + 4)), "the moments plane")
    refused(L.pt_probe_moments_device(None, p(dist), 2, 16, C.byref(v), p(mom)), "null context")
    prm = pt.default_params(spp=1)
    refused(L.pt_probe_distances_device(None, p(dist), 2, 16, C.byref(prm), p(dist)), "null argument")
    refused(L.pt_probe_grid_visibility_device(None, C.byref(pg), 16, C.byref(prm), C.byref(v), p(mom)), "null argument")
    refused(L.pt_render_probe_lit_visibility_device(None, C.byref(c), C.byref(prm), 1, C.byref(pg), p(sh), p(maps), C.byref(v), None, C.byref(sp),
                                                    p(out), None), "null argument")
