"""The irradiance volume's updates over frames on the GPU (pt_debug_probe_update_rays, pt_probe_blend_device,
pt_probe_grid_update_device): the update's ray source and k_probe_update against the rule on the CPU bit for bit, the
identity update against the bake and the visibility pass, the one call against its parts, the chunk boundary of the distance pass,
a light that is dimmed under running updates, reuse of a context and a captured update, and the refusals behind the context."""
import ctypes as C

import numpy as np
import pytest

import bake_ref as br
import probe_grid_ref as pr
import probe_update_ref as pu
from test_probe_update_cpu import GRID, ray_case

pytestmark = pytest.mark.gpu


def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.ascontiguousarray(a)


def _bits(a):
    a = _np(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def _state(P, T=None, age=0, fill=np.nan):
    """(sh27, moments or None, age) device tensors of a grid that was never written"""
    sh = _dev(np.full((P, 9, 3), fill, dtype=np.float32))
    mom = None if T is None else _dev(np.full((P, T, T, 2), fill, dtype=np.float32))
    return sh, mom, _dev(np.full(P, age, dtype=np.uint32))


@pytest.mark.parametrize("frame", [0, 5])
@pytest.mark.parametrize("R", [12, 16])
def test_device_rays_against_the_host_rule(pt, gpu_ctx, R, frame):
    g = GRID.as_pt(pt)
    upd, _, xys = ray_case(pt, R, frame)
    want = pt.probe_update_rays_host(g, upd, xys)
    assert _same(gpu_ctx.probe_update_rays(g, upd, xys, exact_math=1), want)
    fast = gpu_ctx.probe_update_rays(g, upd, xys, exact_math=0)
    worst = br.ulps(np.abs(fast[:, 3:6].astype(np.float64) - want[:, 3:6].astype(np.float64)).max())
    print("fast-arithmetic directions, R %d frame %d: worst component error %.3f ulp of 1" % (R, frame, worst))
    assert _same(fast[:, 0:3], want[:, 0:3]) and worst <= 2.0


@pytest.mark.parametrize("R, T, index", pu.blend_cases())
def test_device_blend_against_the_host_rule(pt, gpu_ctx, R, T, index):
    c = pu.blend_case(R, T, index)
    upd, vis = pu.pt_update(pt, c["upd"]), pu.pt_vis(pt, c["vis"])
    want = pt.probe_blend_host(upd, vis, c["rad"], c["dist"], c["sh"], c["mom"], c["age"])
    sh, mom, age = _dev(c["sh"]), None if T is None else _dev(c["mom"]), _dev(c["age"])
    gpu_ctx.probe_blend(upd, vis, c["rad"], c["dist"], sh, mom, age)
    assert _same(sh, want[0]) and np.array_equal(_np(age).view(np.uint32), want[2])
    assert T is None or _same(mom, want[1])
    rest = np.setdiff1d(np.arange(c["P"]), pu.slots(c["P"], 1, 2))
    assert _same(_np(sh)[rest], c["sh"][rest]) and np.array_equal(_np(age).view(np.uint32)[rest], c["age"][rest])
    assert T is None or _same(_np(mom)[rest], c["mom"][rest])


def identity_is_the_bake(pt, ctx):
    """identity rotation, first 0, stride 1, ages 0 over planes that were never written, a 2 x 2 x 2 grid, R = 64, spp 1"""
    ctx.upload(pt.builtin_scene(2))
    g = pr.Grid((-0.6, -0.6, -2.6), (1.2, 1.2, 1.2), (2, 2, 2)).as_pt(pt)
    for exact_math in (0, 1):
        prm = pt.default_params(spp=1, exact_math=exact_math)
        v = pt.default_probe_visibility(g)
        upd = pt.default_probe_update(0, 1)
        assert upd.rays_per_probe == 64 and pu.is_identity(upd.rotation[:])
        sh, mom, age = _state(8, 8)
        ctx.probe_grid_update(g, prm, v, upd, sh, mom, age)
        assert _same(sh, ctx.probe_grid_bake(g, 64, prm)), exact_math
        assert _same(mom, ctx.probe_grid_visibility(g, 64, prm, v)), exact_math
        assert (_np(age) == 1).all() and np.isfinite(_np(sh)).all()
        # without a visibility struct the maps are not touched
        sh2, mom2, age2 = _state(8, 8)
        ctx.probe_grid_update(g, prm, None, upd, sh2, mom2, age2)
        assert _same(sh2, sh) and np.isnan(_np(mom2)).all()


def test_identity_update_is_the_bake_and_the_visibility_pass(pt, gpu_ctx):
    identity_is_the_bake(pt, gpu_ctx)


def test_one_call_equals_its_parts(pt, gpu_ctx):
    """grid 3 x 2 x 2, stride 3, first 1, frame 5: the call against the debug rays traced through pt_render_rays_device, then
    pt_probe_blend_device; its launch log against that render's"""
    import torch
    gpu_ctx.upload(pt.builtin_scene(2))
    g = GRID.as_pt(pt)
    R, spp = 16, 2
    upd, n_upd, _ = ray_case(pt, R, 5)
    rng = np.random.default_rng(9)
    sh0 = rng.uniform(0.0, 2.0, (12, 9, 3)).astype(np.float32)
    age0 = np.arange(12, dtype=np.uint32)
    for exact_math in (0, 1):
        prm = pt.default_params(spp=spp, exact_math=exact_math, spp_offset=7)
        xys = np.array([(r, k, s) for s in range(spp) for k in range(n_upd) for r in range(R)], dtype=np.uint32)
        rays = torch.from_numpy(gpu_ctx.probe_update_rays(g, upd, xys, exact_math=exact_math).reshape(spp, n_upd, R, 6)).cuda()
        gpu_ctx.launch_log()
        rad = gpu_ctx.render_rays(rays, None, prm, want_rgba=False)[0]
        log_parts = gpu_ctx.launch_log()
        want_sh, _, want_age = _dev(sh0), None, _dev(age0)
        gpu_ctx.probe_blend(upd, None, rad, None, want_sh, None, want_age)
        sh, _, age = _dev(sh0), None, _dev(age0)
        gpu_ctx.launch_log()
        gpu_ctx.probe_grid_update(g, prm, None, upd, sh, None, age)
        log = gpu_ctx.launch_log()
        assert _same(sh, want_sh) and _same(age, want_age), exact_math
        assert not _same(sh, sh0) and float(rad.max()) > 0
        assert log == log_parts and len(log) > 0, (log, log_parts)
        # with the maps: the distances of the same rays, then the blend
        v = pt.default_probe_visibility(g, resolution=4)
        ids, t = gpu_ctx.debug_hit_scene(_np(rays[0]).reshape(-1, 6).astype(np.float64), float(prm.t_min), float("inf"), exact_math=exact_math, accel=0)
        dist = np.where(ids >= 0, t, np.float32(np.inf)).astype(np.float32).reshape(n_upd, R)
        a, b = (_dev(sh0), _dev(np.ones((12, 4, 4, 2), dtype=np.float32)), _dev(age0)), (_dev(sh0), _dev(np.ones((12, 4, 4, 2), dtype=np.float32)), _dev(age0))
        gpu_ctx.probe_blend(upd, v, rad, dist, *a)
        gpu_ctx.probe_grid_update(g, prm, v, upd, *b)
        assert all(_same(x, y) for x, y in zip(a, b)) and _same(a[0], want_sh)


def test_the_distance_pass_crosses_a_chunk_boundary(pt, gpu_ctx):
    """33 slots x 65535 rays: the first-hit pass takes 2^21 rays a chunk, 32 whole slots, so slot 32 is a chunk of its own.  Every
    sample is traced, and the maps are those of two calls over slots 0..31 (a 32-probe grid with the same origin and spacing) and
    slot 32 (first = 32).  The coefficients of slots 0..31 are the first call's too: their film rows are the same.  Slot 32 is film
    row 0 of a call of its own, so its paths draw other continuations there; its coefficients, and everyone's, are held to the
    call's parts instead: the whole film's debug rays through pt_render_rays_device, then pt_probe_blend_device."""
    import torch
    gpu_ctx.upload(pt.builtin_scene(2))
    R = 65535
    assert (1 << 21) // R == 32
    g33 = pr.Grid((-0.8, 0.1, -2.2), (0.05, 0.0, 0.0), (33, 1, 1)).as_pt(pt)
    g32 = pr.Grid((-0.8, 0.1, -2.2), (0.05, 0.0, 0.0), (32, 1, 1)).as_pt(pt)
    prm = pt.default_params(spp=1)
    v = pt.default_probe_visibility(g33, resolution=4, max_distance=1.5)
    upd = pt.default_probe_update(3, 1, rays_per_probe=R)
    sh, mom, age = _state(33, 4)
    gpu_ctx.probe_grid_update(g33, prm, v, upd, sh, mom, age)
    st = gpu_ctx.stats()
    assert st.samples == st.samples_expected == 33 * R
    sh_a, mom_a, age_a = _state(32, 4)
    gpu_ctx.probe_grid_update(g32, prm, v, upd, sh_a, mom_a, age_a)
    sh_b, mom_b, age_b = _state(33, 4)
    gpu_ctx.probe_grid_update(g33, prm, v, pt.default_probe_update(3, 1, rays_per_probe=R, first=32), sh_b, mom_b, age_b)
    assert _same(_np(mom)[:32], mom_a) and _same(_np(mom)[32], _np(mom_b)[32]) and _same(_np(sh)[:32], sh_a)
    assert np.isfinite(_np(sh)).all() and np.isfinite(_np(mom)).all() and (_np(age) == 1).all()
    assert np.isnan(_np(sh_b)[:32]).all() and list(_np(age_b)) == [0] * 32 + [1]
    assert (_np(mom)[..., 0] < 1.5).any()
    xys = np.empty((33 * R, 3), dtype=np.uint32)
    xys[:, 0], xys[:, 1], xys[:, 2] = np.tile(np.arange(R, dtype=np.uint32), 33), np.repeat(np.arange(33, dtype=np.uint32), R), 0
    rays = torch.from_numpy(gpu_ctx.probe_update_rays(g33, upd, xys, exact_math=0).reshape(1, 33, R, 6)).cuda()
    rad = gpu_ctx.render_rays(rays, None, prm, want_rgba=False)[0]
    sh_c, _, age_c = _state(33)
    gpu_ctx.probe_blend(upd, None, rad, None, sh_c, None, age_c)
    assert _same(sh_c, sh) and not _same(_np(sh)[32], _np(sh_b)[32])


def _dc_luminance(sh):
    c = _np(sh).astype(np.float64)[:, 0]
    return float((0.2126 * c[:, 0] + 0.7152 * c[:, 1] + 0.0722 * c[:, 2]).mean())


def test_updates_follow_a_dimmed_light(pt, gpu_ctx):
    """The 10-sphere box, its light dimmed to a quarter with pt_scene_update under a 3 x 3 x 3 grid that was baked in the bright scene
    and has run for 16 frames (age 16).  Updates with stride 1, R = 64, spp 1, a fresh spp_offset and rotation per frame.  The
    distance is |mean DC luminance over the probes - that of a fresh bake of the dimmed scene at R = 4096, spp 16| over the latter.
      gate off: non-increasing over windows of 4 frames (it starts at 3 and falls by 15/16 a frame: 3 (15/16)^24 = 0.64 at the end,
        so a state that keeps its hysteresis cannot reach a fresh bake's level in 24 frames);
      gate on (threshold 0.5, alpha 0.5): smaller after 4 frames than with the gate off.  Without noise every probe's state goes 4 ->
        2.5 -> 1.75 in units of the dimmed level (the gate trips twice: |1 - 4| > 0.5 x 4, |1 - 2.5| > 0.5 x 2.5, then |1 - 1.75| <
        0.5 x 1.75) and falls by 15/16 a frame from there: a distance of 0.75 (15/16)^(n - 2) after n frames, 0.659 after 4 and 0.181
        after 24.  Asserted: no further off than that plus the worst of the five bakes below (the noise of one frame's rays);
      ages reset to 0 at the change -- what an application that knows of the change does: after 24 frames no further off than the
        worst of five fresh R = 64 bakes (spp_offset 0, 1000, ..., 4000): the margin over one bake is that observed spread.
    Measured on one MI355X (docs/EXPERIMENTS.md, "Irradiance volume: updates"): gate off 3.00 -> 0.64, gate on 0.59 after 4 and 0.12
    after 24 frames, ages reset 0.0035 after 24 frames; the five bakes 0.0007 .. 0.0205."""
    bright = pt.builtin_scene(2)
    dim = pt.builtin_scene(2)
    for k in range(3):
        dim[5].mat[k] = bright[5].mat[k] / 4.0
    g = pr.Grid((-0.8, -0.8, -2.8), (0.8, 0.8, 0.8), (3, 3, 3))
    pg = g.as_pt(pt)
    gpu_ctx.upload(bright)
    sh_bright = gpu_ctx.probe_grid_bake(pg, 4096, pt.default_params(spp=4))
    gpu_ctx.scene_update(dim)
    truth = _dc_luminance(gpu_ctx.probe_grid_bake(pg, 4096, pt.default_params(spp=16)))
    dist = lambda sh: abs(_dc_luminance(sh) - truth) / truth
    bakes = [dist(gpu_ctx.probe_grid_bake(pg, 64, pt.default_params(spp=1, spp_offset=off))) for off in (0, 1000, 2000, 3000, 4000)]

    def run(age0, **gate):
        sh, age = sh_bright.clone(), _dev(np.full(27, age0, dtype=np.uint32))
        d = [dist(sh)]
        for frame in range(24):
            upd = pt.default_probe_update(frame + 1, 1, **gate)
            gpu_ctx.probe_grid_update(pg, pt.default_params(spp=1, spp_offset=16 + frame), None, upd, sh, None, age)
            d.append(dist(sh))
        return d

    off, on, reset = run(16), run(16, change_threshold=0.5, change_alpha=0.5), run(0)
    print("distance to the fresh bake: start %.4f; gate off %s; gate on %s; ages reset %s; five R = 64 bakes %s" %
          (off[0], ["%.4f" % v for v in off[4::4]], ["%.4f" % v for v in on[4::4]], ["%.4f" % v for v in reset[4::4]], ["%.4f" % v for v in bakes]))
    assert 2.5 < off[0] < 3.5
    for k in range(0, 24, 4):
        assert off[k + 4] <= off[k] and on[k + 4] <= on[k], (k, off, on)
    assert on[4] < off[4]
    for n in (4, 24):
        assert on[n] <= 0.75 * (15.0 / 16.0) ** (n - 2) + max(bakes), (n, on[n], bakes)
    assert reset[24] <= max(bakes), (reset[24], bakes)


def test_a_context_is_reusable_and_an_update_can_be_captured(pt):
    import torch
    ctx = pt.Context(0)
    try:
        ctx.upload(pt.builtin_scene(2))
        for grid, R, T in ((GRID, 12, 2), (pr.Grid((-0.6, -0.6, -2.6), (1.2, 1.2, 1.2), (2, 2, 2)), 300, 16)):
            pg = grid.as_pt(pt)
            v = pt.default_probe_visibility(pg, resolution=T)
            sh, mom, age = _state(pr.count(grid), T)
            ctx.probe_grid_update(pg, pt.default_params(spp=2), v, pt.default_probe_update(7, 2, rays_per_probe=R), sh, mom, age)
            assert sorted(set(_np(age))) == [0, 1]
        identity_is_the_bake(pt, ctx)
        # a captured update after the first use: nothing is allocated (a hipMalloc would end the capture), replays are the direct call
        pg = GRID.as_pt(pt)
        v = pt.default_probe_visibility(pg, resolution=8)
        prm = pt.default_params(spp=2)
        upd = pt.default_probe_update(9, 2)
        rng = np.random.default_rng(3)
        sh0 = rng.uniform(0.0, 1.0, (12, 9, 3)).astype(np.float32)
        mom0 = rng.uniform(0.1, 1.0, (12, 8, 8, 2)).astype(np.float32)
        age0 = np.arange(12, dtype=np.uint32)
        want = (_dev(sh0), _dev(mom0), _dev(age0))
        ctx.probe_grid_update(pg, prm, v, upd, *want)
        got = (_dev(sh0), _dev(mom0), _dev(age0))
        L = pt._lib.lib()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            ctx.set_stream(side.cuda_stream)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                pt.api.check(L.pt_probe_grid_update_device(ctx._h, C.byref(pg), C.byref(prm), C.byref(v), C.byref(upd), C.c_void_p(got[0].data_ptr()),
                                                           C.c_void_p(got[1].data_ptr()), C.c_void_p(got[2].data_ptr())))
            for _ in range(2):
                for t, a in zip(got, (sh0, mom0, age0)):
                    t.copy_(_dev(a))
                graph.replay()
                side.synchronize()
                assert all(_same(x, y) for x, y in zip(got, want))
        ctx.set_stream(None)
        del graph
    finally:
        ctx.close()


def test_the_host_entry_and_the_mirror(pt, gpu_ctx, tmp_path):
    """pt_probe_grid_update_host = the device entry on the same planes, with the maps and without; examples/probe_preview --update
    (World::update_probe_grid) writes every frame, and the frames get darker as the state follows the dimmed light"""
    import os
    import subprocess
    gpu_ctx.upload(pt.builtin_scene(2))
    pg = GRID.as_pt(pt)
    rng = np.random.default_rng(21)
    sh0 = rng.uniform(0.0, 1.0, (12, 9, 3)).astype(np.float32)
    mom0 = rng.uniform(0.1, 1.0, (12, 8, 8, 2)).astype(np.float32)
    age0 = np.arange(12, dtype=np.uint32)
    prm = pt.default_params(spp=2, spp_offset=5)
    upd = pt.default_probe_update(4, 3)
    for v in (pt.default_probe_visibility(pg, resolution=8), None):
        dev = (_dev(sh0), _dev(mom0), _dev(age0))
        gpu_ctx.probe_grid_update(pg, prm, v, upd, *dev)
        host = gpu_ctx.probe_grid_update_host(pg, prm, v, upd, sh0, mom0, age0)
        assert _same(host[0], dev[0]) and np.array_equal(host[2], _np(dev[2]).view(np.uint32)) and not _same(host[0], sh0)
        assert (v is None and host[1] is None and _same(dev[1], mom0)) or _same(host[1], dev[1])
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "probe_preview")
    prefix = str(tmp_path / "pp")
    r = subprocess.run([exe, "--visibility=4", "--update", "4,2", "3", "3", "3", "2", prefix], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr

    def mean(name):
        with open(prefix + name, "rb") as f:
            data = f.read()
        return float(np.frombuffer(data[-256 * 256 * 3:], dtype=np.uint8).mean())

    levels = [mean("_probe_lit.ppm")] + [mean("_update_%03d.ppm" % k) for k in range(4)]
    print("mean display level: baked %.2f, after the update frames %s" % (levels[0], ["%.2f" % v for v in levels[1:]]))
    assert levels[2] < levels[0] and levels[4] < levels[2], levels          # (two frames of stride 2 pass over every probe once)
    assert not os.path.exists(prefix + "_update_004.ppm")


def test_device_side_refusals_leave_the_context_usable(pt):
    import torch
    cam = pt.camera_new(width=16, height=16)
    pg = GRID.as_pt(pt)
    prm = pt.default_params(spp=1)

    def run(with_refusals):
        ctx = pt.Context(0)
        try:
            v = pt.default_probe_visibility(pg)
            upd = pt.default_probe_update(1, 2)
            sh, mom, age = _state(12, 8, fill=1.0)

            def refused(call, text):
                with pytest.raises(pt._lib.PtError) as e:
                    call()
                assert e.value.code == 1 and text in str(e.value), str(e.value)

            if with_refusals:
                refused(lambda: ctx.probe_grid_update(pg, prm, v, upd, sh, mom, age), "no scene")
            ctx.upload(pt.builtin_scene(2))
            if with_refusals:
                ctx.render(cam, pt.default_params(spp=2))
                refused(lambda: ctx.probe_grid_update(pg, pt.default_params(spp=1, band_rows=4, band_count=2), v, upd, sh, mom, age), "band_count = 1")
                refused(lambda: ctx.probe_grid_update(pg, pt.default_params(spp=1, accel=7), v, upd, sh, mom, age), "accel")
                refused(lambda: ctx.probe_grid_update(pg, pt.default_params(spp=0), v, upd, sh, mom, age), "spp")
                for over, text in ((dict(rays_per_probe=0), "rays_per_probe"), (dict(stride=0), "stride"), (dict(first=12), "first"),
                                   (dict(hysteresis=1.0), "hysteresis"), (dict(change_threshold=float("nan")), "change_threshold"),
                                   (dict(change_alpha=-0.5), "change_alpha"), (dict(rotation=np.eye(3) * 1.01), "orthonormal")):
                    bad = pt.default_probe_update(1, 2, **{k: val for k, val in over.items() if k != "stride"})
                    if "stride" in over:
                        bad.stride = 0
                    refused(lambda: ctx.probe_grid_update(pg, prm, v, bad, sh, mom, age), text)
                    refused(lambda: ctx.probe_blend(bad, None, np.ones((6, 64, 3), dtype=np.float32), None, sh, None, age), text)
                refused(lambda: ctx.probe_grid_update(pg, prm, pt.default_probe_visibility(pg, resolution=1), upd, sh, mom, age), "resolution")
                bad_grid = pr.Grid((0.0, 0.0, 0.0), (1.0, 0.0, 1.0), (3, 2, 2)).as_pt(pt)
                L = pt._lib.lib()
                p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
                for rc in (L.pt_probe_grid_update_device(ctx._h, C.byref(bad_grid), C.byref(prm), C.byref(v), C.byref(upd), p(sh), p(mom), p(age)),
                           L.pt_probe_grid_update_device(ctx._h, C.byref(pg), C.byref(prm), C.byref(v), C.byref(upd), p(sh), p(mom), None),
                           L.pt_probe_grid_update_device(ctx._h, C.byref(pg), C.byref(prm), C.byref(v), C.byref(upd), p(sh), p(mom), p(age, 2)),
                           L.pt_probe_grid_update_device(ctx._h, C.byref(pg), C.byref(prm), C.byref(v), C.byref(upd), p(sh), p(mom, 4), p(age)),
                           L.pt_probe_grid_update_device(ctx._h, C.byref(pg), C.byref(prm), C.byref(v), C.byref(upd), None, p(mom), p(age)),
                           L.pt_probe_blend_device(ctx._h, 12, C.byref(upd), C.byref(v), p(sh), None, p(sh), p(mom), p(age))):
                    assert rc == 1 and L.pt_last_error()
                assert (_np(age) == 0).all() and (_np(sh) == 1).all() and (_np(mom) == 1).all()
            ctx.probe_grid_update(pg, prm, v, upd, sh, mom, age)
            return _np(sh), _np(mom), _np(age), _np(ctx.render(cam, pt.default_params(spp=2))[0])
        finally:
            ctx.close()

    a, b = run(True), run(False)
    assert all(_same(x, y) for x, y in zip(a, b))
