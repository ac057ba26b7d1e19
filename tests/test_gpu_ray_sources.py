"""What the three kernel forms of one ray source (pt_kernels_rays.hip: paths, feature rays, debug rays) owe each other, row by row
over the sources: the lens, the four projections, the bake's texels and probes, in both arithmetic modes.

1. paths = debug: the film of the source's own entry is, bit for bit, the film of pt_render_rays_device fed the debug entry's rays
   of every (x, y, sample) in state order (the bake: and the throughputs), with the sample batches cut so that the caller's rays of
   a later batch start at the right state.
2. feature = debug (lens, projections): the depth plane of one feature sample is t of pt_debug_hit_scene on that sample's debug
   rays, 0 at a miss, and the emitter flag is 1 exactly on emissive hits.
3. the film does not depend on the batching.

Image 7 x 5 (odd, not square), 5 samples, builtin scene 1 (the Cornell box of triangles) seen from inside the box: the camera looks up
at the ceiling light, and the wide projections send rays out through the box's open front (misses)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
W, H, SPP, OFF = 7, 5, 5, 2
NP = W * H
EMISSIVE = 1
SCENE = 1
LOOK = ((0.05, 0.59, -1.9), (0.0, 0.99, -2.0), (0.0, 0.0, 1.0), W, H, 60.0)     # 0.4 under the centre of the light, looking at it; up: the open front


def _bits(a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _all_xys(spp, spp_offset):
    """(x, y, sample) of every state of a [spp, H, W] ray plane, in its order"""
    ss, ys, xs = np.meshgrid(np.arange(spp) + spp_offset, np.arange(H), np.arange(W), indexing="ij")
    return np.stack([xs.ravel(), ys.ravel(), ss.ravel()], axis=1).astype(np.uint32)


def _texels():
    """7 x 5 texels inside the box ([-1, 1]^2 x [-3, -1]), three of them empty (a zero normal)"""
    rng = np.random.default_rng(75)
    t = np.empty((H, W, 6), dtype=np.float32)
    t[..., 0:3] = rng.uniform(-0.7, 0.7, (H, W, 3)) + np.array([0.0, 0.0, -2.0])
    t[..., 3:6] = rng.normal(size=(H, W, 3))
    empty = np.zeros((H, W), dtype=bool)
    for y, x in ((0, 0), (2, 5), (4, 6)):
        t[y, x, 3:6] = 0.0
        empty[y, x] = True
    return t, empty


def _probes():
    """5 probes (the film's rows) of 7 directions (its columns)"""
    return (np.random.default_rng(76).uniform(-0.6, 0.6, (H, 3)) + np.array([0.0, 0.0, -2.0])).astype(np.float32)


# name -> (entry(ctx, pt, params) -> linear film, debug(ctx, xys, exact_math) -> rays[n, >= 6], weights[H, W] or None,
#          features(ctx, params, n) or None)
def _lens_row(pt):
    cam, lens = pt.camera_look_at(*LOOK), pt.default_lens(aperture=0.05, focus_distance=0.4)
    return (lambda ctx, prm: ctx.render_lens(cam, lens, prm, want_rgba=False)[0],
            lambda ctx, xys, em: ctx.lens_rays(cam, lens, xys, exact_math=em), None,
            lambda ctx, prm, n: ctx.render_features_lens(cam, lens, prm, n))


def _projection_row(kind, fov):
    def make(pt):
        cam, proj = pt.camera_look_at(*LOOK), pt.default_projection(kind=kind, fov_degrees=fov)
        return (lambda ctx, prm: ctx.render_projection(cam, proj, prm, want_rgba=False)[0],
                lambda ctx, xys, em: ctx.projection_rays(cam, proj, xys, exact_math=em), None,
                lambda ctx, prm, n: ctx.render_features_projection(cam, proj, prm, n))
    return make


def _texel_row(pt):
    t, empty = _texels()
    return (lambda ctx, prm: ctx.bake_lightmap(t, prm, want_rgba=False)[0],
            lambda ctx, xys, em: ctx.bake_rays("texels", t, xys, exact_math=em), np.where(empty, 0.0, 1.0).astype(np.float32), None)


def _probe_row(pt):
    pos = _probes()
    return (lambda ctx, prm: ctx.bake_probes(pos, W, prm, want_sh=False)[0],
            lambda ctx, xys, em: ctx.bake_rays("probes", (pos, W), xys, exact_math=em), None, None)


ROWS = {"lens": _lens_row, "perspective": _projection_row("perspective", 180.0), "orthographic": _projection_row("orthographic", 180.0),
        "fisheye": _projection_row("fisheye", 240.0), "equirect": _projection_row("equirect", 180.0),
        "texels": _texel_row, "probes": _probe_row}
CAMERA_ROWS = [r for r in ROWS if r not in ("texels", "probes")]


def _batch_sizes(cap):
    nb = cap // NP
    return [min(nb, SPP - done) for done in range(0, SPP, nb)]


@pytest.mark.parametrize("exact_math", [1, 0])
@pytest.mark.parametrize("row", list(ROWS))
def test_paths_form_is_the_debug_form_across_batches(pt, gpu_ctx, row, exact_math):
    import torch
    gpu_ctx.upload(pt.builtin_scene(SCENE))
    entry, debug, weights, _ = ROWS[row](pt)
    # the smallest max_paths_in_flight the checks admit (>= np) that cuts the samples into >= 3 batches of unequal size: below
    # 2 np every batch is one sample
    cap = next(c for c in range(NP, SPP * NP + 1) if len(_batch_sizes(c)) >= 3 and len(set(_batch_sizes(c))) > 1)
    assert cap == 2 * NP and _batch_sizes(cap) == [2, 2, 1]
    batched = pt.default_params(spp=SPP, spp_offset=OFF, exact_math=exact_math, max_paths_in_flight=cap)
    whole = pt.default_params(spp=SPP, spp_offset=OFF, exact_math=exact_math, max_paths_in_flight=SPP * NP)
    rays = debug(gpu_ctx, _all_xys(SPP, OFF), exact_math)
    planes = torch.from_numpy(np.ascontiguousarray(rays[:, :6]).reshape(SPP, H, W, 6)).cuda()
    wplanes = None
    if weights is not None:
        wplanes = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(weights[None, :, :, None], (SPP, H, W, 3)))).cuda()
    film = entry(gpu_ctx, batched)
    assert gpu_ctx.stats().batches == 3
    ref = gpu_ctx.render_rays(planes, weights=wplanes, params=batched, want_rgba=False)[0]
    assert gpu_ctx.stats().batches == 3
    assert float(ref.max()) > 0
    assert _same(film.reshape(H, W, 3), ref)                                  # 1. paths form = debug form
    one = entry(gpu_ctx, whole)
    assert gpu_ctx.stats().batches == 1
    assert _same(one, film)                                                   # 3. the film does not depend on the batching


@pytest.mark.parametrize("exact_math", [1, 0])
@pytest.mark.parametrize("row", CAMERA_ROWS)
def test_feature_form_is_the_debug_form(pt, gpu_ctx, row, exact_math):
    objs = pt.builtin_scene(SCENE)
    gpu_ctx.upload(objs)
    emissive = np.array([o.mat_tag == EMISSIVE for o in objs])
    _, debug, _, features = ROWS[row](pt)
    seen = set()
    for s in (0, 3):
        prm = pt.default_params(spp=1, spp_offset=s, exact_math=exact_math, accel=0)
        feat = features(gpu_ctx, prm, 1)
        rays = debug(gpu_ctx, _all_xys(1, s), exact_math)
        ids, ts = gpu_ctx.debug_hit_scene(rays[:, :6], t_min=prm.t_min, exact_math=exact_math, accel=0)
        hit = ids >= 0
        depth = np.where(hit, ts, np.float32(0.0)).astype(np.float32)
        assert _same(feat[..., 7].ravel(), depth)
        lit = np.zeros(NP, dtype=bool)
        lit[hit] = emissive[ids[hit]]
        assert np.array_equal(feat[..., 3].ravel(), lit.astype(np.float32))
        seen |= {"emitter"} if lit.any() else set()
        seen |= {"surface"} if (hit & ~lit).any() else set()
        seen |= {"miss"} if (~hit).any() else set()
    print(f"{row}, exact_math {exact_math}: saw {sorted(seen)}")
    assert {"emitter", "surface"} <= seen                                     # (the camera looks at the light, the box around it)
    if row in ("fisheye", "equirect"):
        assert "miss" in seen                                                 # rays off the view axis leave through the open front
