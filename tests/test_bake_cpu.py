"""Light baking (pt_bake_lightmap_device and friends) without a GPU: the rule on the CPU (pt_bake_rays_host,
pathtrace_amd/csrc/pt_bake.h in exact arithmetic) against the numpy restatement (tests/bake_ref.py), the probe directions and
their Gram matrix, the SH projection and the irradiance against numpy, and the refusals through the C ABI."""
import ctypes as C

import numpy as np
import pytest

import bake_ref as br

FAKE = [C.c_void_p(0x1000 * k) for k in range(1, 7)]      # aligned, distinct addresses no check may read
# max |(4 pi / R) sum Y_i Y_j - identity| of the rule's directions, computed in f64
GRAM = {64: 0.010895, 256: 0.0012648, 1024: 0.00017623}


def _refused(pt, rc, part):
    assert rc == 1, rc                                            # PT_ERR_INVALID_ARG
    msg = pt._lib.lib().pt_last_error().decode()
    assert msg and part in msg, msg


# ---------------------------------------------------------------- 1. the host rule against the restatement
def test_texel_rays_against_the_restatement(pt):
    t = br.slanted_texels()
    xys = br.all_xys(8, 8, 4)
    got32 = pt.bake_rays_host("texels", t, xys)
    got = got32.astype(np.float64)
    ref = br.texel_rays(t, xys)
    assert not ref["empty"].any()
    assert np.array_equal(got32[:, 0:3].view(np.uint32), t[xys[:, 1], xys[:, 0], 0:3].view(np.uint32))      # o = point exactly
    err = br.ulps(np.abs(got[:, 3:6] - ref["d"]).max())
    unit = br.ulps(np.abs(np.linalg.norm(got[:, 3:6], axis=1) - 1.0).max())
    cos = (got[:, 3:6] * ref["n"]).sum(axis=1)
    print(f"texel rays: |d - ref| {err:.3f} ulps (bound {br.TEXEL_D_ULPS}), | |d| - 1 | {unit:.3f} ulps, min d.n {cos.min():.4f}")
    assert err <= br.TEXEL_D_ULPS
    assert unit <= br.TEXEL_D_ULPS
    assert np.all(cos > 0.0)
    assert np.abs(ref["n"][:8 * 4:1, 1]).max() > 0.999 and np.abs(ref["n"][:, 1]).min() < 0.999      # both branches of the frame
    # the samples of a texel differ, and a sample does not depend on the others asked for
    assert len({tuple(r) for r in got32[(xys[:, 0] == 3) & (xys[:, 1] == 5), 3:6].tolist()}) == 4
    one = pt.bake_rays_host("texels", t, [(3, 5, 2)])
    assert np.array_equal(one.view(np.uint32), got32[(xys[:, 0] == 3) & (xys[:, 1] == 5) & (xys[:, 2] == 2)].view(np.uint32))


def test_empty_texels_get_the_valid_ray(pt):
    t = br.slanted_texels()
    t[1, 2, 3:6] = 0.0
    t[2, 3, 0] = np.nan
    t[3, 4, 4] = np.inf
    t[4, 5, 3:6] = (1e-20, 0.0, 0.0)                              # shorter than the fast normalize can tell from nothing
    t[5, 6, 3:6] = (3e19, 0.0, 0.0)                               # the square of its length overflows f32
    xys = br.all_xys(8, 8, 2)
    got = pt.bake_rays_host("texels", t, xys)
    ref = br.texel_rays(t, xys)
    e = ref["empty"]
    assert e.sum() == 2 * 5
    assert np.array_equal(got[e], np.broadcast_to(np.array([0, 0, 0, 0, 0, 1], dtype=np.float32), (10, 6)))
    assert np.isfinite(got).all()
    assert br.ulps(np.abs(got[~e, 3:6].astype(np.float64) - ref["d"][~e]).max()) <= br.TEXEL_D_ULPS


# ---------------------------------------------------------------- 2. probe directions
@pytest.mark.parametrize("R", [64, 256, 1024])
def test_probe_directions(pt, R):
    d32 = pt.probe_directions(R)
    d = d32.astype(np.float64)
    ref = br.probe_dirs(R)
    assert np.array_equal(d[:, 2], ref[:, 2])                     # z is exact
    err = br.ulps(np.abs(d - ref).max())
    assert len(set(br.probe_phase_words(R).tolist())) == R        # the phases are pairwise distinct
    g = np.abs(br.gram(d) - np.eye(9)).max()
    print(f"R {R}: |d - ref| {err:.3f} ulps (bound {br.PROBE_D_ULPS}), Gram deviation {g:.6g} (computed: {GRAM[R]})")
    assert err <= br.PROBE_D_ULPS
    assert g <= GRAM[R] * 1.05
    assert g >= GRAM[R] * 0.95                                    # (the figure is this rule's)
    # every probe and every sample has the same directions; the origin is the probe's position
    pos = np.array([[0.5, -1.0, 2.0], [3.0, 4.0, 5.0]], dtype=np.float32)
    xys = np.array([(r, p, s) for p in (0, 1) for s in (0, 9) for r in (0, 1, R - 1)], dtype=np.uint32)
    got = pt.bake_rays_host("probes", (pos, R), xys)
    assert np.array_equal(got[:, 3:6].view(np.uint32), d32[xys[:, 0]].view(np.uint32))
    assert np.array_equal(got[:, 0:3], pos[xys[:, 1]])


def test_probe_direction_zero_has_phase_zero(pt):
    d = pt.probe_directions(100)                                  # no power of two: z is the f64 quotient rounded once
    assert d[0, 1] == 0.0 and d[0, 0] > 0.0
    z = 1.0 - (2.0 * np.arange(100) + 1.0) / 100.0
    assert np.array_equal(d[:, 2], z.astype(np.float32))
    assert br.ulps(np.abs(np.linalg.norm(d.astype(np.float64), axis=1) - 1.0).max()) <= br.PROBE_D_ULPS


# ---------------------------------------------------------------- 3. the SH projection
def _planes(R, seed):
    rng = np.random.default_rng(seed)
    z = br.probe_dirs(R)[:, 2]
    planes = [np.ones((R, 3)), np.repeat(z[:, None], 3, axis=1), np.repeat(np.maximum(0.0, z)[:, None], 3, axis=1), rng.uniform(0.0, 4.0, (R, 3)),
              rng.normal(size=(R, 3)) * np.array([1.0, 10.0, 0.1])]
    return np.stack(planes).astype(np.float32)


@pytest.mark.parametrize("R", [64, 256, 1024, 100, 1, 63, 65])
def test_sh_projection_against_numpy(pt, R):
    rad = _planes(R, 3 + R)
    sh = pt.sh_project_host(rad)
    d = pt.probe_directions(R).astype(np.float64)
    ref, mag = br.sh_project(rad, d)
    err = np.abs(sh.astype(np.float64) - ref)
    print(f"R {R}: |sh - numpy| / sum |terms| = {(err[mag > 0] / mag[mag > 0]).max():.3e}")
    assert np.all(err <= 1e-6 * mag)                              # (a coefficient all of whose terms are 0 is 0)
    assert np.array_equal(sh.view(np.uint32), pt.sh_project_host(rad).view(np.uint32))      # the order is fixed
    assert np.array_equal(sh[1:2].view(np.uint32), pt.sh_project_host(rad[1:2]).view(np.uint32))      # a probe does not see its neighbours
    if R >= 64:
        # radiance 1 is Y0 alone, radiance z is Y(1, 0) alone, to within the directions' Gram error
        tol = GRAM.get(R, 0.02) * 1.05 * np.sqrt(4.0 * np.pi)
        want1 = np.zeros(9); want1[0] = np.sqrt(4.0 * np.pi)
        wantz = np.zeros(9); wantz[2] = np.sqrt(4.0 * np.pi / 3.0)
        assert np.abs(sh[0, :, 0] - want1).max() <= tol and np.abs(sh[1, :, 1] - wantz).max() <= tol


# ---------------------------------------------------------------- 4. irradiance
@pytest.mark.parametrize("R", [64, 256])
def test_irradiance_of_constant_radiance(pt, R):
    L = np.array([0.75, 2.0, 0.125])
    sh = pt.sh_project_host(np.broadcast_to(L.astype(np.float32), (1, R, 3)))[0]
    rng = np.random.default_rng(9)
    n = rng.normal(size=(64, 3))
    n /= np.linalg.norm(n, axis=1)[:, None]
    E = pt.sh_irradiance(sh, n * rng.uniform(0.5, 3.0, (64, 1))).astype(np.float64)      # (the entry normalises)
    dev = np.abs(E / (np.pi * L) - 1.0).max()
    print(f"R {R}: |E / (pi L) - 1| = {dev:.3e} (Gram deviation {GRAM[R]})")
    assert dev <= GRAM[R] * 1.05
    assert np.abs(E - br.sh_irradiance(sh, n)).max() <= 4 * 2.0 ** -23 * np.pi * L.max()
    assert np.array_equal(pt.sh_irradiance(sh, [(0.0, 0.0, 0.0)]), np.zeros((1, 3), dtype=np.float32))


# ---------------------------------------------------------------- 5. refusals
def test_refusals(pt):
    L = pt._lib.lib()
    prm = pt.default_params(spp=2)
    mb = C.byref(prm)
    ctx, tex, lin, rgba, sh, pos = FAKE
    odd = C.c_void_p(0x1004)                                      # 4-byte aligned, not 8
    off = C.c_void_p(0x2002)
    # lightmaps
    for entry in (L.pt_bake_lightmap_device, L.pt_bake_lightmap_host):
        name = "pt_bake_lightmap_device" if entry is L.pt_bake_lightmap_device else "pt_bake_lightmap_host"
        _refused(pt, entry(None, 8, 8, tex, mb, lin, rgba), name + ": null argument")
        _refused(pt, entry(ctx, 8, 8, tex, None, lin, rgba), name + ": null argument")
        _refused(pt, entry(ctx, 8, 8, None, mb, lin, rgba), "texels6 is null")
        _refused(pt, entry(ctx, 8, 8, tex, mb, None, rgba), "the linear output is null")
        _refused(pt, entry(ctx, 8, 8, off, mb, lin, rgba), "texels6 must be")
        _refused(pt, entry(ctx, 8, 8, tex, mb, off, rgba), "the linear output must be 4-byte aligned")
        _refused(pt, entry(ctx, 8, 8, tex, mb, lin, off), "the RGBA8 output must be 4-byte aligned")
        _refused(pt, entry(ctx, 0, 8, tex, mb, lin, rgba), "a zero size")
        _refused(pt, entry(ctx, 8, 0, tex, mb, lin, rgba), "a zero size")
        _refused(pt, entry(ctx, 65536, 1, tex, mb, lin, rgba), "< 65536")
        _refused(pt, entry(ctx, 8, 8, tex, C.byref(pt.default_params(spp=2, band_rows=4, band_count=2)), lin, rgba), "band_count = 1")
    _refused(pt, L.pt_bake_lightmap_device(ctx, 8, 8, odd, mb, lin, rgba), "texels6 must be 8-byte aligned")
    # probes
    for entry in (L.pt_bake_probes_device, L.pt_bake_probes_host):
        name = "pt_bake_probes_device" if entry is L.pt_bake_probes_device else "pt_bake_probes_host"
        _refused(pt, entry(None, pos, 4, 64, mb, lin, sh), name + ": null argument")
        _refused(pt, entry(ctx, pos, 4, 64, None, lin, sh), name + ": null argument")
        _refused(pt, entry(ctx, None, 4, 64, mb, lin, sh), "positions3 is null")
        _refused(pt, entry(ctx, pos, 4, 64, mb, None, sh), "the radiance output is null")
        _refused(pt, entry(ctx, off, 4, 64, mb, lin, sh), "positions3 must be 4-byte aligned")
        _refused(pt, entry(ctx, pos, 4, 64, mb, off, sh), "the radiance output must be 4-byte aligned")
        _refused(pt, entry(ctx, pos, 4, 64, mb, lin, off), "sh27 must be 4-byte aligned")
        _refused(pt, entry(ctx, pos, 0, 64, mb, lin, sh), "a zero size")
        _refused(pt, entry(ctx, pos, 4, 0, mb, lin, sh), "rays_per_probe must be > 0")
        _refused(pt, entry(ctx, pos, 4, 65536, mb, lin, sh), "< 65536")
        _refused(pt, entry(ctx, pos, 4, 64, C.byref(pt.default_params(spp=2, band_rows=1, band_count=4)), lin, sh), "band_count = 1")
    # the SH entries
    rad = np.ones((2, 64, 3), dtype=np.float32)
    out = np.full((2, 9, 3), 7.0, dtype=np.float32)
    pv = lambda a: a.ctypes.data_as(C.c_void_p)
    _refused(pt, L.pt_sh_project_device(None, 2, 64, lin, sh), "pt_sh_project_device: null argument")
    _refused(pt, L.pt_sh_project_device(ctx, 2, 0, lin, sh), "rays_per_probe must be > 0")
    _refused(pt, L.pt_sh_project_device(ctx, 0, 64, lin, sh), "a zero size")
    _refused(pt, L.pt_sh_project_device(ctx, 2, 64, None, sh), "the radiance plane is null")
    _refused(pt, L.pt_sh_project_device(ctx, 2, 64, lin, off), "sh27 must be 4-byte aligned")
    _refused(pt, L.pt_sh_project_host(2, 0, pv(rad), pv(out)), "rays_per_probe must be > 0")
    _refused(pt, L.pt_sh_project_host(0, 64, pv(rad), pv(out)), "a zero size")
    _refused(pt, L.pt_sh_project_host(2, 64, None, pv(out)), "the radiance plane is null")
    _refused(pt, L.pt_sh_project_host(2, 64, pv(rad), None), "sh27 is null")
    _refused(pt, L.pt_sh_project_host(2, 64, pv(rad), C.c_void_p(out.ctypes.data + 2)), "sh27 must be 4-byte aligned")
    _refused(pt, L.pt_sh_irradiance_host(None, pv(rad), 1, pv(out)), "pt_sh_irradiance_host: null argument")
    _refused(pt, L.pt_sh_irradiance_host(pv(out), None, 1, pv(out)), "pt_sh_irradiance_host: null argument")
    # the ray entries
    t = br.slanted_texels()
    xys = (C.c_uint32 * 3)(1, 2, 3)
    out6 = np.full(6, 7.0, dtype=np.float32)
    _refused(pt, L.pt_bake_rays_host(2, 8, 8, pv(t), xys, 1, pv(out6)), "unknown bake kind")
    _refused(pt, L.pt_bake_rays_host(0, 0, 8, pv(t), xys, 1, pv(out6)), "a zero size")
    _refused(pt, L.pt_bake_rays_host(1, 0, 8, pv(t), xys, 1, pv(out6)), "rays_per_probe must be > 0")
    _refused(pt, L.pt_bake_rays_host(0, 8, 8, None, xys, 1, pv(out6)), "pt_bake_rays_host: null argument")
    _refused(pt, L.pt_bake_rays_host(0, 8, 8, pv(t), None, 1, pv(out6)), "pt_bake_rays_host: null argument")
    _refused(pt, L.pt_bake_rays_host(0, 8, 8, pv(t), (C.c_uint32 * 3)(8, 2, 0), 1, pv(out6)), "outside the 8x8 film")
    _refused(pt, L.pt_bake_rays_host(0, 8, 8, pv(t), (C.c_uint32 * 3)(1, 8, 0), 1, pv(out6)), "outside the 8x8 film")
    _refused(pt, L.pt_debug_bake_rays(None, 0, 8, 8, pv(t), xys, 1, 0, pv(out6)), "pt_debug_bake_rays: null argument")
    _refused(pt, L.pt_debug_bake_rays(ctx, 3, 8, 8, pv(t), xys, 1, 0, pv(out6)), "unknown bake kind")
    _refused(pt, L.pt_debug_bake_rays(ctx, 0, 8, 8, pv(t), (C.c_uint32 * 3)(9, 9, 0), 1, 0, pv(out6)), "outside the 8x8 film")
    assert np.all(out == 7.0) and np.all(out6 == 7.0)             # a refusal writes nothing
    assert L.pt_abi_version() == 6
