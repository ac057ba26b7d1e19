"""Light baking (pt_bake_lightmap_device, pt_bake_probes_device, pt_sh_project_device) on the GPU: the device's
rays against the rule on the CPU and the numpy restatement (tests/bake_ref.py); a bake against pt_render_rays_device fed the
bake's own rays; a furnace; the closed form of a sphere light over a plane; probes under a cap of light; interreflection against
the camera's integrator; empty texels; and what the entries leave of the context."""
import numpy as np
import pytest

import bake_ref as br

pytestmark = pytest.mark.gpu
SPH, TRI, LAMBERT, EMISSIVE = 0, 1, 0, 1
LIGHT_C, LIGHT_R, LIGHT_L = np.array([0.0, 0.0, 2.0]), 0.5, np.array([4.0, 2.0, 1.0], dtype=np.float32)
CAP_PROBES = np.array([(0.0, 0.0, 0.0), (0.3, -0.2, 0.5), (-0.7, 0.4, -0.5), (0.1, 0.9, 1.0)], dtype=np.float32)


def _bits(a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _np(a):
    return a.cpu().numpy()


def _sphere_light(pt):
    return pt.make_objects([(SPH, list(LIGHT_C) + [LIGHT_R], EMISSIVE, list(LIGHT_L))])


# ---------------------------------------------------------------- 1. device rays against the CPU rule
@pytest.mark.parametrize("exact_math", [1, 0])
def test_device_rays_against_the_host_rule(pt, gpu_ctx, exact_math):
    t = br.slanted_texels()
    t[6, 1, 3:6] = 0.0                                            # one empty texel
    xys = br.all_xys(8, 8, 4)
    got = gpu_ctx.bake_rays("texels", t, xys, exact_math=exact_math)
    host = pt.bake_rays_host("texels", t, xys)
    ref = br.texel_rays(t, xys)
    err = br.ulps(np.abs(got[:, 3:6].astype(np.float64) - ref["d"]).max())
    print(f"texels, exact_math {exact_math}: |d - restatement| {err:.3f} ulps (bound {br.TEXEL_D_ULPS})")
    assert np.array_equal(got[:, 0:3].view(np.uint32), host[:, 0:3].view(np.uint32))
    pos = np.array([(0.5, -1.0, 2.0), (3.0, 4.0, 5.0)], dtype=np.float32)
    pxys = br.all_xys(64, 2, 4)
    pgot = gpu_ctx.bake_rays("probes", (pos, 64), pxys, exact_math=exact_math)
    phost = pt.bake_rays_host("probes", (pos, 64), pxys)
    perr = br.ulps(np.abs(pgot[:, 3:6].astype(np.float64) - br.probe_dirs(64)[pxys[:, 0]]).max())
    print(f"probes, exact_math {exact_math}: |d - restatement| {perr:.3f} ulps (bound {br.PROBE_D_ULPS})")
    assert np.array_equal(pgot[:, 0:3], pos[pxys[:, 1]])
    if exact_math:
        assert np.array_equal(got.view(np.uint32), host.view(np.uint32))
        assert np.array_equal(pgot.view(np.uint32), phost.view(np.uint32))
    assert err <= br.TEXEL_D_ULPS
    assert perr <= br.PROBE_D_ULPS


# ---------------------------------------------------------------- 2. closing the loop
@pytest.mark.parametrize("exact_math", [0, 1])
def test_a_bake_is_render_rays_fed_the_bakes_own_rays(pt, gpu_ctx, exact_math):
    import torch
    gpu_ctx.upload(pt.builtin_scene(2))
    W, H, SPP, OFF = 8, 8, 4, 3
    t = br.slanted_texels()
    t[..., 0:3] *= 0.4                                            # inside the box of builtin scene 2: [-1, 1]^2 x [-3, -1]
    t[..., 2] -= 2.0
    prm = pt.default_params(spp=SPP, spp_offset=OFF, exact_math=exact_math)
    rays = gpu_ctx.bake_rays("texels", t, br.all_xys(W, H, SPP, OFF), exact_math=exact_math)
    planes = torch.from_numpy(rays.reshape(SPP, H, W, 6)).cuda()
    gpu_ctx.launch_log()
    ref = gpu_ctx.render_rays(planes, params=prm)
    log = gpu_ctx.launch_log()
    got = gpu_ctx.bake_lightmap(t, prm)
    assert log and log == gpu_ctx.launch_log()
    assert _same(got[0], ref[0]) and _same(got[1], ref[1])
    assert float(ref[0].max()) > 0
    small = pt.default_params(spp=SPP, spp_offset=OFF, exact_math=exact_math, max_paths_in_flight=W * H * 2)
    got = gpu_ctx.bake_lightmap(t, small)
    assert gpu_ctx.stats().batches == 2
    assert _same(got[0], ref[0]) and _same(got[1], ref[1])
    # probes: a probe per row, a direction per column
    P, R = 4, 64
    pos = (0.5 * np.random.default_rng(2).uniform(-1.0, 1.0, (P, 3)) + np.array([0.0, 0.0, -2.0])).astype(np.float32)
    rays = gpu_ctx.bake_rays("probes", (pos, R), br.all_xys(R, P, SPP, OFF), exact_math=exact_math)
    planes = torch.from_numpy(rays.reshape(SPP, P, R, 6)).cuda()
    gpu_ctx.launch_log()
    ref = gpu_ctx.render_rays(planes, params=prm, want_rgba=False)[0]
    log = gpu_ctx.launch_log()
    rad, sh = gpu_ctx.bake_probes(pos, R, prm)
    assert log and log == gpu_ctx.launch_log()
    assert _same(rad, ref) and float(ref.max()) > 0
    assert _same(sh, pt.sh_project_host(_np(rad)))
    rad2, _ = gpu_ctx.bake_probes(pos, R, pt.default_params(spp=SPP, spp_offset=OFF, exact_math=exact_math, max_paths_in_flight=P * R * 2), want_sh=False)
    assert gpu_ctx.stats().batches == 2
    assert _same(rad2, ref)


# ---------------------------------------------------------------- 3. furnace
@pytest.mark.parametrize("exact_math", [1, 0])
def test_furnace_is_exact(pt, gpu_ctx, exact_math):
    E = np.array([0.75, 0.5, 0.25], dtype=np.float32)
    gpu_ctx.upload(pt.make_objects([(SPH, [0.0, 0.0, 0.0, 10.0], EMISSIVE, list(E))]))
    rng = np.random.default_rng(7)
    t = np.empty((16, 16, 6), dtype=np.float32)
    p = rng.normal(size=(16, 16, 3))
    t[..., 0:3] = p / np.linalg.norm(p, axis=-1, keepdims=True) * 5.0 * rng.uniform(0.0, 1.0, (16, 16, 1)) ** (1.0 / 3.0) * 0.999
    t[..., 3:6] = rng.normal(size=(16, 16, 3))
    prm = pt.default_params(spp=16, exact_math=exact_math)
    lin, rgba = gpu_ctx.bake_lightmap(t, prm)
    assert np.array_equal(_np(lin), np.broadcast_to(E, (16, 16, 3)))
    assert len(np.unique(_np(rgba).reshape(-1, 4), axis=0)) == 1 and _np(rgba)[0, 0, 3] == 255
    pos = t[0, :4, 0:3].copy()
    rad, sh = gpu_ctx.bake_probes(pos, 256, pt.default_params(spp=1, exact_math=exact_math))
    assert np.array_equal(_np(rad), np.broadcast_to(E, (4, 256, 3)))
    assert _same(sh, pt.sh_project_host(_np(rad)))
    # the smallest films: one texel, one probe of one direction
    lin, _ = gpu_ctx.bake_lightmap(t[:1, :1], prm)
    assert np.array_equal(_np(lin), E.reshape(1, 1, 3))
    rad, sh = gpu_ctx.bake_probes(pos[:1], 1, prm)
    assert np.array_equal(_np(rad), E.reshape(1, 1, 3)) and _same(sh, pt.sh_project_host(_np(rad)))


# ---------------------------------------------------------------- 4. a sphere light over a plane: the closed form
@pytest.mark.parametrize("integrator", [0, 1])
def test_sphere_light_closed_form(pt, gpu_ctx, integrator):
    """The only object is the light, so a sample is L where its ray hits the sphere, else 0: with probability
    p = (r / d)^2 cos(theta), the cosine-weighted share of the hemisphere a sphere wholly above the horizon takes."""
    gpu_ctx.upload(_sphere_light(pt))
    SPP = 4096
    g = (np.arange(16) + 0.5) / 8.0 - 1.0
    t = np.zeros((16, 16, 6), dtype=np.float32)
    t[..., 0], t[..., 1] = g[None, :], g[:, None]
    t[..., 5] = 1.0
    lin = _np(gpu_ctx.bake_lightmap(t, pt.default_params(spp=SPP, integrator=integrator), want_rgba=False)[0]).astype(np.float64)
    to = LIGHT_C - t[..., 0:3].astype(np.float64)
    d = np.linalg.norm(to, axis=-1)
    p = (LIGHT_R / d) ** 2 * (to[..., 2] / d)
    sd = np.sqrt(p * (1.0 - p) / SPP)
    L = LIGHT_L.astype(np.float64)
    dev = np.abs(lin - L * p[..., None]) / (L * sd[..., None])
    mean, want = lin[..., 0].mean() / L[0], p.mean()
    se = np.sqrt((sd ** 2).sum()) / p.size
    print(f"integrator {integrator}: worst texel {dev.max():.2f} sd; mean hit share {mean:.6f}, closed form {want:.6f}, {abs(mean - want) / se:.2f} se")
    assert np.all(np.abs(lin - L * p[..., None]) <= 5.0 * L * sd[..., None])
    assert abs(mean - want) <= 4.0 * se
    assert np.array_equal(lin[..., 0] * (L[1] / L[0]), lin[..., 1])      # the channels are one hit count


# ---------------------------------------------------------------- 5. probes under a cap of light
def test_probes_see_the_cap(pt, gpu_ctx):
    """The radiance plane is L x (the direction hits the sphere), decided in f64 from the restatement's directions; no direction
    passes within 1e-4 of the silhouette, which an f32 direction (an error of 1e-7) cannot cross."""
    gpu_ctx.upload(_sphere_light(pt))
    R = 256
    d = br.probe_dirs(R)
    oc = LIGHT_C[None, :] - CAP_PROBES.astype(np.float64)
    b = oc @ d.T                                                  # [P, R]: the centre's distance along the ray
    perp = np.linalg.norm(oc[:, None, :] - b[:, :, None] * d[None, :, :], axis=2)
    hit = (perp < LIGHT_R) & (b > 0)
    margin = np.abs(perp - LIGHT_R)[b > 0].min()
    print(f"hits per probe {hit.sum(axis=1).tolist()}, smallest distance from the silhouette {margin:.3e}")
    assert margin > 1e-4
    assert hit.sum(axis=1).tolist() == [4, 7, 2, 10]
    for exact_math in (0, 1):
        rad, sh = gpu_ctx.bake_probes(CAP_PROBES, R, pt.default_params(spp=1, exact_math=exact_math))
        assert np.array_equal(_np(rad), hit[:, :, None] * LIGHT_L[None, None, :])
        assert _same(sh, pt.sh_project_host(_np(rad)))
        assert _same(gpu_ctx.sh_project(rad), sh)


# ---------------------------------------------------------------- 6. interreflection against the camera's integrator
def test_interreflection_against_the_camera(pt, gpu_ctx):
    """Under PT_INTEGRATOR_BRDF_ONLY a camera ray that hits the Lambert floor (albedo 0.5) at X continues by the cosine sampling
    a baked texel at X starts with: 0.5 x the bake = the camera's radiance, in expectation.  65536 independent streams each:
    the texels of a 256 x 256 lightmap that all hold X (a film's width stays below 65536, so 65536 x 1 is no lightmap), and
    pt_ray_color on copies of one ray under distinct keys."""
    floor = [(TRI, [-5.0, -1.0, -5.0, -5.0, -1.0, 5.0, 5.0, -1.0, 5.0], LAMBERT, [0.5, 0.5, 0.5]),
             (TRI, [-5.0, -1.0, -5.0, 5.0, -1.0, 5.0, 5.0, -1.0, -5.0], LAMBERT, [0.5, 0.5, 0.5])]
    gpu_ctx.upload(pt.make_objects(floor + [(SPH, [0.7, -0.6, 0.0, 0.4], LAMBERT, [0.8, 0.8, 0.8]),
                                            (SPH, [0.0, 1.5, 0.0, 0.5], EMISSIVE, [8.0, 8.0, 8.0])]))
    N = 256
    X = np.array([0.0, -1.0, 0.3])
    t = np.zeros((N, N, 6), dtype=np.float32)
    t[..., 0:3] = X
    t[..., 4] = 1.0
    prm = pt.default_params(spp=1, integrator=1)
    bake = 0.5 * _np(gpu_ctx.bake_lightmap(t, prm, want_rgba=False)[0]).astype(np.float64)[..., 0].ravel()
    o = np.array([0.4, 0.5, 1.0])
    dirn = (X - o) / np.linalg.norm(X - o)
    ys, xs = np.meshgrid(np.arange(N), np.arange(N), indexing="ij")
    cam = gpu_ctx.ray_color(prm, np.broadcast_to(np.concatenate([o, dirn]), (N * N, 6)), np.stack([xs.ravel(), ys.ravel()], axis=1))
    cam = cam.astype(np.float64)[:, 0]
    se = np.sqrt(bake.var(ddof=1) / bake.size + cam.var(ddof=1) / cam.size)
    print(f"0.5 x bake {bake.mean():.5f}, camera {cam.mean():.5f}, combined standard error {se:.5f} ({se / cam.mean():.2%} of the mean)")
    assert se < 0.03 * cam.mean()
    assert abs(bake.mean() - cam.mean()) <= 4.0 * se


# ---------------------------------------------------------------- 7. empty texels
def test_empty_texels_are_black_and_cost_nothing_else(pt, gpu_ctx):
    gpu_ctx.upload(pt.builtin_scene(2))
    t = br.slanted_texels(16, 12, seed=8)
    t[..., 0:3] *= 0.4                                            # inside the box of builtin scene 2: [-1, 1]^2 x [-3, -1]
    t[..., 2] -= 2.0
    holes = t.copy()
    ys, xs = np.meshgrid(np.arange(12), np.arange(16), indexing="ij")
    board = (xs + ys) % 2 == 0
    holes[board, 3:6] = 0.0
    holes[1, 2, 0] = np.nan
    holes[3, 2, 4] = np.inf
    holes[5, 2, 2] = -np.inf
    holes[7, 2, 3:6] = np.nan
    empty = br.empty(holes)
    assert empty.sum() == board.sum() + 4
    for exact_math in (0, 1):
        prm = pt.default_params(spp=8, exact_math=exact_math)
        full = gpu_ctx.bake_lightmap(t, prm)
        gpu_ctx.stats()
        lin, rgba = gpu_ctx.bake_lightmap(holes, prm)             # (_on_stream: pt_sync has succeeded)
        st = gpu_ctx.stats()
        assert st.samples == st.samples_expected == 16 * 12 * 8
        lin, rgba = _np(lin), _np(rgba)
        assert np.array_equal(lin[empty].view(np.uint32), np.zeros((empty.sum(), 3), dtype=np.uint32))      # +0.0
        assert np.array_equal(rgba[empty], np.broadcast_to(np.array([0, 0, 0, 255], dtype=np.uint8), (empty.sum(), 4)))
        assert np.array_equal(lin[~empty].view(np.uint32), _np(full[0])[~empty].view(np.uint32))
        assert np.array_equal(rgba[~empty], _np(full[1])[~empty])
        assert np.isfinite(lin).all() and float(lin.max()) > 0
    # whatever was traced: in the furnace an unmasked empty texel would not be black under a throughput that is not 0 either
    gpu_ctx.upload(pt.make_objects([(SPH, [0.0, 0.0, 0.0, 10.0], EMISSIVE, [1.0, 1.0, 1.0])]))
    lin = _np(gpu_ctx.bake_lightmap(holes, pt.default_params(spp=2), want_rgba=False)[0])
    assert np.array_equal(lin[..., 0], np.where(empty, 0.0, 1.0).astype(np.float32))


# ---------------------------------------------------------------- 8. hygiene
def test_bakes_leave_the_context_alone(pt):
    import torch
    cam = pt.camera_new(width=48, height=40)
    prm = pt.default_params(spp=4)
    lens = pt.default_lens(aperture=0.15, focus_distance=2.2)
    t = br.slanted_texels(16, 12, seed=8)
    t[..., 0:3] *= 0.4                                            # inside the box of builtin scene 2: [-1, 1]^2 x [-3, -1]
    t[..., 2] -= 2.0
    t[2, 3, 3:6] = 0.0
    pos = t[0, :5, 0:3].copy()

    def run(with_bake):
        ctx = pt.Context(0)
        try:
            out = []
            if with_bake:                                         # no scene yet: the projection needs none, a bake is refused
                rad = torch.rand((3, 100, 3), dtype=torch.float32, device="cuda")
                assert _same(ctx.sh_project(rad), pt.sh_project_host(_np(rad)))
                with pytest.raises(pt._lib.PtError) as e:
                    ctx.bake_lightmap(t, prm)
                assert e.value.code == 1 and "no scene" in str(e.value)
            ctx.upload(pt.builtin_scene(2))
            if with_bake:
                a = ctx.bake_lightmap(t, pt.default_params(spp=3, max_paths_in_flight=16 * 12))
                b = ctx.bake_probes(pos, 100, pt.default_params(spp=2))
                for bad in (pt.default_params(spp=0), pt.default_params(integrator=9), pt.default_params(band_rows=4, band_count=3)):
                    with pytest.raises(pt._lib.PtError):
                        ctx.bake_lightmap(t, bad)
                    with pytest.raises(pt._lib.PtError):
                        ctx.bake_probes(pos, 100, bad)
                out += [_np(a[0]), _np(a[1]), _np(b[0]), _np(b[1])]
            lens0 = _np(ctx.render_lens(cam, lens, prm)[0])      # shares the inject planes with the bakes
            plain = _np(ctx.render(cam, prm)[0])
            if with_bake:
                a2 = ctx.bake_lightmap(t, pt.default_params(spp=3))
                assert _same(a2[0], out[0]) and _same(a2[1], out[1])      # (and the batching does not show)
                hl, hr = np.empty((12, 16, 3), dtype=np.float32), np.empty((12, 16, 4), dtype=np.uint8)
                pt.api.check(pt._lib.lib().pt_bake_lightmap_host(ctx._h, 16, 12, t.ctypes.data, pt.default_params(spp=3), hl.ctypes.data, hr.ctypes.data))
                assert _same(hl, out[0]) and np.array_equal(hr, out[1])
                hrad, hsh = np.empty((5, 100, 3), dtype=np.float32), np.empty((5, 9, 3), dtype=np.float32)
                pt.api.check(pt._lib.lib().pt_bake_probes_host(ctx._h, pos.ctypes.data, 5, 100, pt.default_params(spp=2), hrad.ctypes.data, hsh.ctypes.data))
                assert _same(hrad, out[2]) and _same(hsh, out[3])
            return [lens0, plain, _np(ctx.render_lens(cam, lens, prm)[0])]
        finally:
            ctx.close()

    for a, b in zip(run(True), run(False)):
        assert np.array_equal(a, b, equal_nan=True)
