"""Auto-exposure and tone mapping on the GPU (pt_film_histogram_device, pt_tonemap_device, pt_exposure_*) against
the numpy restatement tests/tonemap_ref.py: the histogram word for word, the display transform of a render reproduced bit for
bit, the exposure's metering and adaptation in f64, every curve and transfer, in-place and caller-stream use, and that the
exposure state disturbs no other entry of the context."""
import ctypes as C

import numpy as np
import pytest

import launch_cover as lc
import tonemap_ref as tr

pytestmark = pytest.mark.gpu
SHAPES = [(2, 2), (67, 35), (257, 3), (130, 129)]
CAM64 = ((0.6, 0.3, 1.8), (0.0, -0.3, -2.0), (0, 1, 0), 64, 48, 40.0)
_cache = {}


def _real_films(pt, ctx):
    """the films of pt_render_device, C2 and World::new(), 64 x 48 at 4 spp, with their own RGBA8 planes: rendered once"""
    if "real" not in _cache:
        out = []
        for scene in (2, 1):
            ctx.upload(pt.builtin_scene(scene))
            lin, rgba = ctx.render(pt.camera_look_at(*CAM64), pt.default_params(spp=4))
            out.append((lin.cpu().numpy(), rgba.cpu().numpy()))
        _cache["real"] = out
    return _cache["real"]


@pytest.fixture()
def ctx(pt):
    c = pt.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("W,H", SHAPES)
def test_histogram_is_exact_and_cleared(pt, gpu_ctx, W, H):
    film = tr.crafted_film(W, H, 11)
    ref = tr.histogram(film)
    assert ref.sum() == W * H
    got = gpu_ctx.film_histogram(film)
    assert np.array_equal(got, ref), np.argwhere(got != ref)[:8]
    assert int(got.sum()) == W * H
    assert np.array_equal(gpu_ctx.film_histogram(film), ref)          # the words were zeroed in front of the second pass


def _large_shapes():
    """the two film sizes past the launch boundaries of k_film_histogram on this device (tests/launch_cover.py)"""
    import torch
    return lc.hist_sizes(torch.cuda.get_device_properties(0).multi_processor_count)


@pytest.mark.parametrize("which", [0, 1])
def test_histogram_past_the_grid_cap(pt, gpu_ctx, which):
    """More pixels than the capped grid holds in one slot (which = 0: batch slots 1 .. 3 in use) and than it holds in one trip
    (which = 1: a second grid-stride trip, a few workgroups long, the last of them partly filled)"""
    import torch
    n_cus = torch.cuda.get_device_properties(0).multi_processor_count
    W, H = _large_shapes()[which]
    reach = lc.hist_reach(W * H, n_cus)
    assert reach["grid"] == n_cus and (reach["max_slot"] >= 1 and reach["trips"] == 1 if which == 0 else
                                       reach["max_slot"] == 3 and reach["trips"] == 2 and reach["last_trip_fill"] < 1.0)
    film = tr.crafted_film(W, H, 11 + which)
    ref = tr.histogram(film)
    assert ref.sum() == W * H
    for _ in range(2):
        got = gpu_ctx.film_histogram(film)
        assert np.array_equal(got, ref), np.argwhere(got != ref)[:8]


def test_auto_exposure_past_the_grid_cap(pt, ctx):
    """One auto-mode frame of the larger film: the stored histogram and the metered exposure, then the two planes on the curve
    film of that size at the bars of test_curves_and_transfers"""
    W, H = _large_shapes()[1]
    film = tr.crafted_film(W, H, 12)
    over = dict(log2_min=-40.0, log2_max=40.0)                 # (the crafted film's median lies far outside the default range)
    ctx.exposure_reset()
    ctx.tonemap(film, **over)
    log2E, hist = ctx.exposure()
    ref = tr.histogram(film)
    assert np.array_equal(hist, ref), np.argwhere(hist != ref)[:8]
    want = tr.target(ref, tr.params(**over))
    print(f"{W}x{H} crafted: log2E {log2E:.15f} restatement {want:.15f} diff {abs(log2E - want):.2e}")
    assert abs(log2E - want) <= 1e-12
    for seed, curve, transfer in ((0, tr.ACES, tr.SQRT), (1, tr.REINHARD, tr.SRGB)):
        film = tr.curve_film(W, H, seed)
        over = tr.random_params(seed) if seed else {}
        p = tr.params(curve=curve, transfer=transfer, **over)
        ctx.exposure_reset()
        got8, gotf = ctx.tonemap(film, curve=curve, transfer=transfer, **over)
        log2E, hist = ctx.exposure()
        ref = tr.histogram(film)
        assert np.array_equal(hist, ref) and abs(log2E - tr.target(ref, p)) <= 1e-12
        _, E, valid = ctx.debug_exposure_state()
        assert valid == 1
        y = tr.curve(film, E, p)
        ref8, safe = tr.rgba8(y, p)
        assert (~safe).mean() <= 0.02
        err = _max_rel(gotf.astype(np.float64), y)
        print(f"{W}x{H} seed {seed}: max rel err of the float plane {err:.2e}")
        assert err <= 1e-4, (curve, transfer, err)
        d = np.abs(got8.astype(int) - ref8.astype(int)).max(-1)
        assert (d[safe] == 0).all() and (d <= 1).all(), (curve, transfer, int(d.max()), int((d[safe] != 0).sum()))
        assert (got8[..., 3] == 255).all()
        assert gotf.reshape(-1, 3)[5, 1] == 0.0 and got8.reshape(-1, 4)[5, 1] == 0


def test_histogram_of_the_real_films(pt, gpu_ctx):
    for lin, _ in _real_films(pt, gpu_ctx):
        assert np.array_equal(gpu_ctx.film_histogram(lin), tr.histogram(lin))


def test_identity_anchor(pt, gpu_ctx):
    """manual, ev = 0, clamp, sqrt = the display transform of pt_render_device"""
    for lin, rgba in _real_films(pt, gpu_ctx):
        got8, gotf = gpu_ctx.tonemap(lin, mode="manual", ev=0.0, curve="clamp", transfer="sqrt")
        assert np.array_equal(gotf.view(np.uint32), lin.view(np.uint32))
        assert np.array_equal(got8, rgba), np.argwhere(got8 != rgba)[:8]


def test_first_frame_meets_the_restatements_target(pt, ctx):
    films = [tr.crafted_film(130, 129, 11), tr.crafted_film(67, 35, 12)] + [lin for lin, _ in _real_films(pt, ctx)]
    for k, film in enumerate(films):
        over = tr.random_params(k) if k % 2 else {}
        if k < 2:
            over.update(log2_min=-40.0, log2_max=40.0)             # the crafted films' medians lie far outside the default range
        ctx.exposure_reset()
        ctx.tonemap(film, **over)
        log2E, hist = ctx.exposure()
        ref = tr.histogram(film)
        assert np.array_equal(hist, ref)
        want = tr.target(ref, tr.params(**over))
        print(f"film {k}: log2E {log2E:.15f} restatement {want:.15f} diff {abs(log2E - want):.2e}")
        assert abs(log2E - want) <= 1e-12
        _, E, valid = ctx.debug_exposure_state()
        assert valid == 1 and abs(float(E) - 2.0 ** log2E) <= 2.0 ** log2E * 2.0 ** -23


def test_adaptation_follows_the_recursion(pt, ctx):
    """6 frames, the film scaled by 1/4 from frame 3 on, adapt 0.5; then a reset, a size change, a black frame, manual mode"""
    film = tr.curve_film(67, 35, 5, planted=False)
    p = tr.params(adapt=0.5)
    assert ctx.exposure()[0] == 0.0 and ctx.debug_exposure_state()[2] == 0          # nothing metered yet
    prev, seq = None, []
    for frame in range(6):
        f = film * np.float32(0.25) if frame >= 3 else film
        ctx.tonemap(f, adapt=0.5)
        prev = tr.adapt(tr.histogram(f), p, prev)
        got = ctx.exposure()[0]
        seq.append(got)
        assert abs(got - prev) <= 1e-12, (frame, got, prev)
    assert seq[0] == seq[1] == seq[2]                                               # at its target: t - log2E = 0
    assert seq[3] - seq[2] == pytest.approx(1.0, abs=0.02) and seq[5] - seq[2] == pytest.approx(1.75, abs=0.03)
    dim = film * np.float32(0.25)
    ctx.exposure_reset()
    ctx.tonemap(dim, adapt=0.5)
    t_dim = tr.target(tr.histogram(dim), p)
    assert abs(ctx.exposure()[0] - t_dim) <= 1e-12                                  # after a reset: the jump
    # a change of W x H resets: the same pixels as 35 x 67 jump to the bright film's target
    ctx.tonemap(film.reshape(67, 35, 3), adapt=0.5)
    t_bright = tr.target(tr.histogram(film), p)
    assert abs(ctx.exposure()[0] - t_bright) <= 1e-12 and abs(t_bright - t_dim) > 1.9
    # an all-black frame keeps the exposure (dark pixels alone: N = 0), whatever adapt is
    ctx.tonemap(np.zeros((67, 35, 3), dtype=np.float32), adapt=0.5)
    log2E, hist = ctx.exposure()
    assert log2E == pytest.approx(t_bright, abs=1e-12) and hist[tr.DARK] == 67 * 35 and hist[:256].sum() == 0
    # manual mode leaves the state and the last histogram untouched
    before = ctx.debug_exposure_state()
    ctx.tonemap(dim.reshape(67, 35, 3), mode="manual", ev=3.0)
    assert ctx.debug_exposure_state() == before and np.array_equal(ctx.exposure()[1], hist)
    # a black first frame after a reset: 0
    ctx.exposure_reset()
    ctx.tonemap(np.zeros((67, 35, 3), dtype=np.float32))
    assert ctx.exposure()[0] == 0.0 and ctx.debug_exposure_state()[2] == 1


def _max_rel(got, ref):
    return float(np.max(np.abs(got - ref) / np.maximum(np.abs(ref), 1e-3)))


@pytest.mark.parametrize("W,H", SHAPES)
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_curves_and_transfers(pt, gpu_ctx, W, H, seed):
    """each curve x each transfer, default (seed 0) and random parameters, against the f64 restatement under the device's own
    f32 E.  The bar of the filter parity tests: 1e-4 relative with the floor 1e-3 under the reference.  RGBA8: equal on the
    margin-safe pixels, at most 1 LSB elsewhere; the restatement alone keeps the unsafe ones under 2 % (asserted on the CPU
    too, tests/test_tonemap_cpu.py).  Measured maxima: docs/EXPERIMENTS.md, "Tone mapping"."""
    film = tr.curve_film(W, H, seed)
    over = tr.random_params(seed) if seed else {}
    worst = 0.0
    for curve in (tr.CLAMP, tr.REINHARD, tr.ACES):
        for transfer in (tr.SQRT, tr.SRGB):
            p = tr.params(curve=curve, transfer=transfer, **over)
            gpu_ctx.exposure_reset()
            got8, gotf = gpu_ctx.tonemap(film, curve=curve, transfer=transfer, **over)
            _, E, valid = gpu_ctx.debug_exposure_state()
            assert valid == 1
            y = tr.curve(film, E, p)
            ref8, safe = tr.rgba8(y, p)
            assert (~safe).mean() <= 0.02
            err = _max_rel(gotf.astype(np.float64), y)
            worst = max(worst, err)
            assert err <= 1e-4, (curve, transfer, err)
            d = np.abs(got8.astype(int) - ref8.astype(int)).max(-1)
            assert (d[safe] == 0).all() and (d <= 1).all(), (curve, transfer, int(d.max()), int((d[safe] != 0).sum()))
            assert (got8[..., 3] == 255).all()
            if W * H > 8:                                          # the planted NaN channel: 0 on both planes
                assert gotf.reshape(-1, 3)[5, 1] == 0.0 and got8.reshape(-1, 4)[5, 1] == 0
    print(f"{W}x{H} seed {seed}: max rel err of the float plane {worst:.2e}")


def test_manual_exposure_and_curves_on_a_real_film(pt, gpu_ctx):
    lin, _ = _real_films(pt, gpu_ctx)[1]
    for ev in (-2.0, 1.5):
        E = np.float32(2.0 ** ev)
        for curve in (tr.REINHARD, tr.ACES):
            p = tr.params(curve=curve, transfer=tr.SRGB)
            got8, gotf = gpu_ctx.tonemap(lin, mode="manual", ev=ev, curve=curve, transfer=tr.SRGB)
            y = tr.curve(lin, E, p)
            assert _max_rel(gotf.astype(np.float64), y) <= 1e-4
            ref8, safe = tr.rgba8(y, p)
            d = np.abs(got8.astype(int) - ref8.astype(int)).max(-1)
            assert (d[safe] == 0).all() and (d <= 1).all()


def test_in_place_and_on_a_callers_stream(pt, gpu_ctx):
    import torch
    film = tr.curve_film(130, 129, 7)
    gpu_ctx.exposure_reset()
    ref8, reff = gpu_ctx.tonemap(film)
    gpu_ctx.exposure_reset()
    got8, gotf = gpu_ctx.tonemap(film, in_place=True)
    assert np.array_equal(got8, ref8) and np.array_equal(gotf.view(np.uint32), reff.view(np.uint32))
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):                                  # Context.tonemap runs on torch's current stream
        gpu_ctx.exposure_reset()
        got8, gotf = gpu_ctx.tonemap(film)
    assert np.array_equal(got8, ref8) and np.array_equal(gotf.view(np.uint32), reff.view(np.uint32))
    gpu_ctx.set_stream(None)


def test_graph_capture_after_the_first_use(pt, ctx):
    """nothing is allocated after the first auto-mode call: a frame can be captured, and replays adapt on the device"""
    import torch
    film = tr.curve_film(67, 35, 9, planted=False)
    p = tr.params(adapt=0.5)
    dev = torch.device("cuda", 0)
    d_lin = torch.from_numpy(film * np.float32(4.0)).to(dev)
    rgba = torch.empty((35, 67, 4), dtype=torch.uint8, device=dev)
    tm = pt.default_tonemap(adapt=0.5)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        ctx.set_stream(side.cuda_stream)
        pt._lib.check(pt._lib.lib().pt_tonemap_device(ctx._h, 67, 35, C.c_void_p(d_lin.data_ptr()), C.byref(tm), None, C.c_void_p(rgba.data_ptr())))
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            pt._lib.check(pt._lib.lib().pt_tonemap_device(ctx._h, 67, 35, C.c_void_p(d_lin.data_ptr()), C.byref(tm), None, C.c_void_p(rgba.data_ptr())))
        prev = tr.adapt(tr.histogram(film * np.float32(4.0)), p, None)
        d_lin.copy_(torch.from_numpy(film).to(dev))
        for _ in range(3):
            g.replay()
            prev = tr.adapt(tr.histogram(film), p, prev)
        side.synchronize()
    assert abs(ctx.exposure()[0] - prev) <= 1e-12
    ctx.set_stream(None)


def test_the_exposure_state_disturbs_no_denoiser_frame(pt, ctx):
    """a pt_denoise_device and two pt_denoise_temporal_device frames with pt_tonemap_device on their outputs in between = the
    same frames without it"""
    objs = pt.builtin_scene(2)
    cam = pt.camera_look_at(*CAM64)
    runs = []
    for with_tonemap in (False, True):
        ctx.upload(objs)
        ctx.temporal_reset()
        frames = []
        for k in range(2):
            prm = pt.default_params(spp=4, spp_offset=4 * k)
            lin, _ = ctx.render(cam, prm)
            lin = lin.cpu().numpy()
            feat = ctx.render_features(cam, prm, 4)
            a = ctx.denoise(lin, feat)
            if with_tonemap:
                ctx.tonemap(a[0])
            b = ctx.denoise_temporal(cam, lin, feat)
            if with_tonemap:
                ctx.tonemap(b[0], curve="reinhard", transfer="srgb")
                ctx.film_histogram(b[0])
            frames.append((a, b))
        runs.append(frames)
    for (a0, b0), (a1, b1) in zip(*runs):
        for x, y in zip(a0 + b0, a1 + b1):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    # and the scene entries left the exposure alone
    before = ctx.debug_exposure_state()
    ctx.upload(pt.builtin_scene(1))
    ctx.scene_update(pt.builtin_scene(1))
    assert ctx.debug_exposure_state() == before and before[2] == 1
