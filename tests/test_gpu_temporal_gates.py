"""k_denoise_temporal and the a-trous steps behind it against the f64 restatement (tests/temporal_ref.py) on the inputs of
tests/temporal_cases.py: past n = 4, where the moment variance m2 - m1^2 steers the filter weights; with alpha' = alpha;
a known distance on each side of every history gate; one thin valid tap that is renormalised by S; rotation, zoom, a
point behind the previous camera, reprojections with one tap column in the image, and image sizes that are no multiple
of the 32 x 8 block.  tests/test_temporal_cpu.py checks how many pixels of each input a comparison may skip; here the cap
is asserted again on what was skipped.

The bar is the one test_gpu_temporal.py and test_gpu_denoise.py hold against the same restatements: a maximum relative
error of 1e-4 with a floor of 1e-3 under the reference.  Measured maxima: docs/EXPERIMENTS.md, "Temporal denoiser"."""
import numpy as np
import pytest

import denoise_ref as dr
import temporal_cases as tc
import temporal_ref as tr

pytestmark = pytest.mark.gpu
BAR = 1e-4
SKIP_CAP = 0.10


@pytest.fixture(scope="module", autouse=True)
def scene(pt, gpu_ctx):
    gpu_ctx.upload(pt.builtin_scene(1))             # the entry takes films and features; the scene only makes the context valid


def _max_rel(got, ref):
    return float(np.max(np.abs(got - ref) / np.maximum(np.abs(ref), 1e-3))) if got.size else 0.0


def _grow(bad, r):
    g = bad.copy()
    if not bad.any():
        return g
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            sh, m = dr._shift(bad, dy, dx)
            g |= sh & m
    return g


def _parity(ctx, frames, iters, label, **kw):
    """Feeds the frames to the kernel and the restatement after a reset; compares every frame as
    test_moving_sequences_match_the_f64_restatement does -> the outputs of the last frame (gpu linear, gpu rgba, info)."""
    ctx.temporal_reset()
    hist, bad = None, None
    for i, (cam, c, f) in enumerate(frames):
        lin, rgba = ctx.denoise_temporal(cam, c, f, iterations=iters, **kw)
        ref, hist, info = tr.step(c, f, hist, cam, iterations=iters, **kw)
        unsafe = ~tr.safe_mask(info)[0]
        bad = unsafe if bad is None else _grow(bad, 3) | unsafe     # a pixel decided differently spoils the history near it
        cmp = ~_grow(bad, 2 * ((1 << iters) - 1) + iters) if iters else ~bad
        err = _max_rel(lin[cmp], ref[cmp])
        print(f"{label} it {iters} frame {i}: compared {cmp.mean():.4f}, fresh {info['fresh'].mean():.4f}, "
              f"n <= {hist['n'].max():.3f}, max rel err {err:.2e}")
        assert 1.0 - cmp.mean() <= SKIP_CAP, (label, i)
        assert err <= BAR, (label, i, err)
        assert np.array_equal(rgba, dr.rgba8(lin)), (label, i)
    return lin, rgba, info


@pytest.mark.parametrize("iters", [0, 1, 3])
@pytest.mark.parametrize("params", ["default", "random"])
def test_wall_sequence_matches_the_f64_restatement_over_twelve_frames(pt, gpu_ctx, params, iters):
    """Five frames of a standing camera (n = 1 .. 5: the variance changes hands at n = 4), then seven moving ones with
    alpha' = alpha, fractional n at the incoming edges, and the two history buffers swapped every frame."""
    kw = dict(tc.RANDOM) if params == "random" else {}
    _parity(gpu_ctx, tc.wall_sequence(pt), iters, f"wall {params}", **kw)


def test_static_camera_with_the_full_filter_matches_on_every_pixel(pt, gpu_ctx):
    frames = tc.static_sequence(pt)
    assert len(frames) == 8
    gpu_ctx.temporal_reset()
    hist = None
    for i, (cam, c, f) in enumerate(frames):
        lin, rgba = gpu_ctx.denoise_temporal(cam, c, f, iterations=5, alpha=0.2)
        ref, hist, info = tr.step(c, f, hist, cam, iterations=5, alpha=0.2)
        assert tr.safe_mask(info)[0].all() and np.all(hist["n"] == i + 1)
        err = _max_rel(lin, ref)
        print(f"static it 5 frame {i}: max rel err {err:.2e}")
        assert err <= BAR, (i, err)
        assert np.array_equal(rgba, dr.rgba8(lin))


def test_a_flat_sequence_stays_flat(pt, gpu_ctx):
    """The temporal twin of test_filter_properties: m2 - m1^2 is exactly 0 from n = 4 on, and that must not upset the
    weights (sigma_l * 0 + 1e-10 under |L_p - L_q| = 0)."""
    gpu_ctx.temporal_reset()
    v = np.float32(0.37)
    for i, (cam, c, f) in enumerate(tc.flat_sequence(pt)):
        lin, _ = gpu_ctx.denoise_temporal(cam, c, f, iterations=5)
        assert np.all(np.isfinite(lin)), i
        assert np.abs(lin.astype(np.float64) - float(v)).max() <= 2 * float(np.spacing(v)), (i, np.abs(lin - v).max())


@pytest.mark.parametrize("which", [0, 1, 2])
def test_history_gates_take_and_reject_at_a_known_distance(pt, gpu_ctx, which):
    """A film of zeros, then a film of ones: 0.5 where the history was taken, 1.0 where the pixel is fresh.  which = 1
    narrows the depth and normal gates so that three kinds of block flip; which = 2 sets both tolerances to 0, where equal
    depths and a dot product of exactly 0 are still taken (the comparisons are <= and >=)."""
    kw = tc.GATE_PARAMS[which]
    frames = tc.gate_frames(pt)
    exp, taken = tc.gate_expected(which)
    gpu_ctx.temporal_reset()
    for cam, c, f in frames:
        lin, _ = gpu_ctx.denoise_temporal(cam, c, f, iterations=0, **kw)
    wrong = [name for i, (name, _) in enumerate(tc.GATE_BLOCKS)
             if not np.array_equal(lin[tc.gate_block(i)][..., 0] < 0.75, taken[tc.gate_block(i)])]
    assert not wrong, wrong
    assert np.array_equal(lin[..., 0] < 0.75, taken)
    assert np.all(np.abs(lin - exp[..., None]) <= 3e-7 * exp[..., None]), np.abs(lin - exp[..., None]).max()
    for iters in (0, 2):                     # every pixel: the margins are 0.007 or more, or the operands are equal
        gpu_ctx.temporal_reset()
        hist = None
        for i, (cam, c, f) in enumerate(frames):
            lin, rgba = gpu_ctx.denoise_temporal(cam, c, f, iterations=iters, **kw)
            ref, hist, info = tr.step(c, f, hist, cam, iterations=iters, **kw)
            err = _max_rel(lin, ref)
            print(f"gates {which} it {iters} frame {i}: max rel err {err:.2e}")
            assert err <= BAR, (iters, i, err)
            assert np.array_equal(rgba, dr.rgba8(lin))


@pytest.mark.parametrize("iters", [0, 2])
@pytest.mark.parametrize("shift", tc.THIN_SHIFTS)
def test_one_thin_tap_is_dropped_below_and_renormalised_above_the_weight_floor(pt, gpu_ctx, shift, iters):
    frames = tc.thin_tap_frames(pt, shift)
    lin, _, info = _parity(gpu_ctx, frames, iters, f"thin {shift}")
    if iters == 0:                           # the fresh pixels are the current frame's, to the bit
        cur, _ = gpu_ctx.denoise(frames[1][1], frames[1][2], iterations=0)
        assert np.array_equal(lin[info["fresh"]], cur[info["fresh"]])
        assert not np.array_equal(lin[~info["fresh"]], cur[~info["fresh"]])


@pytest.mark.parametrize("iters", [0, 2])
@pytest.mark.parametrize("name", tc.PAIR_NAMES)
def test_camera_pairs_match_the_f64_restatement(pt, gpu_ctx, name, iters):
    frames = tc.camera_pairs(pt)[name]
    lin, rgba, info = _parity(gpu_ctx, frames, iters, name)
    if name == "turned round":               # lambda <= 0 for every pixel: the spatial filter of the frame
        assert info["fresh"].all()
        cur = gpu_ctx.denoise(frames[1][1], frames[1][2], iterations=iters)
        assert np.array_equal(lin, cur[0]) and np.array_equal(rgba, cur[1])


def test_a_spatial_call_between_temporal_frames_leaves_the_history_alone(pt, gpu_ctx):
    """pt_denoise_device shares the two (u, var) planes with the temporal entry, not the history."""
    frames = tc.wall_sequence(pt, W=80, H=60, frames=7, still=4)
    other = tc.wall_sequence(pt, W=96, H=80, frames=1)[0]
    runs = []
    for between in (False, True):
        gpu_ctx.temporal_reset()
        outs = []
        for cam, c, f in frames:
            outs.append(gpu_ctx.denoise_temporal(cam, c, f, iterations=3))
            if between:
                gpu_ctx.denoise(other[1], other[2], iterations=4)
                gpu_ctx.denoise(c, f, iterations=1)
        runs.append(outs)
    for i, (a, b) in enumerate(zip(*runs)):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), i
    assert not np.array_equal(runs[0][-1][0], gpu_ctx.denoise(frames[-1][1], frames[-1][2], iterations=3)[0])
