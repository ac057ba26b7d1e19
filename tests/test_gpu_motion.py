"""The temporal denoiser that follows moving objects, on the GPU: pt_scene_update, pt_render_feature_ids_device,
pt_denoise_temporal_motion_device (k_denoise_temporal_motion) and pt_render_denoised_motion against the existing entries, the
f64 restatement (tests/motion_ref.py) on the committed cases (tests/motion_cases.py), and a reference render."""
import os
import subprocess

import numpy as np
import pytest

import denoise_ref as dr
import motion_cases as mc
import motion_ref as mr
import temporal_cases as tc
import temporal_ref as tr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PT_ERR_INVALID_ARG = 1


@pytest.fixture(scope="module")
def ctx2(pt):
    """A second context: the existing entry beside the motion entry, fed the same buffers."""
    c = pt.Context(0)
    yield c
    c.close()


def _prm(pt, spp, off, **kw):
    return pt.default_params(spp=spp, spp_offset=off, **kw)


def _copy(pt, objs):
    return (pt._lib.PtObject * len(objs))(*objs)


def _moved(pt, objs, k, dx, dy=0.0, dz=0.0):
    out = _copy(pt, objs)
    out[k].shape[0] += dx
    out[k].shape[1] += dy
    out[k].shape[2] += dz
    return out


def _small_sphere(objs):
    """The smallest non-emissive sphere of a builtin scene."""
    ks = [k for k, o in enumerate(objs) if o.shape_tag == 0 and o.mat_tag != 1]
    return min(ks, key=lambda k: objs[k].shape[3])


def _max_rel(got, ref):
    return float(np.max(np.abs(got - ref) / np.maximum(np.abs(ref), 1e-3))) if got.size else 0.0


# ------------------------------------------------------------------------------------------------ 1 pt_scene_update
@pytest.mark.parametrize("scene", ["c2", "spheres"])
def test_scene_update_renders_what_scene_upload_renders(pt, gpu_ctx, ctx2, scene):
    base = pt.builtin_scene(2) if scene == "c2" else pt.builtin_scene(4, 200)
    k = _small_sphere(base)
    moved = _moved(pt, base, k, 0.21, 0.05)
    if scene == "spheres":                                   # (one of 200 small spheres may hide from a 64 x 48 film: move them all)
        for o in moved:
            o.shape[0] += 0.05
    cam = pt.camera_new(width=64, height=48)
    for accel in ((0, 1) if scene == "c2" else (1,)):
        prm = _prm(pt, 4, 0, accel=accel)
        gpu_ctx.upload(base)
        old = gpu_ctx.render(cam, prm)[0].cpu().numpy()        # (with accel = 1 this builds the old scene's BVH)
        gpu_ctx.scene_update(moved)
        got = gpu_ctx.render(cam, prm)
        ctx2.upload(moved)
        want = ctx2.render(cam, prm)
        assert np.array_equal(got[0].cpu().numpy(), want[0].cpu().numpy()) and np.array_equal(got[1].cpu().numpy(), want[1].cpu().numpy())
        assert not np.array_equal(got[0].cpu().numpy(), old)
    # a wrong count or a changed shape tag: refused, and the scene stays
    fewer = (pt._lib.PtObject * (len(moved) - 1))(*list(moved)[:-1])
    other = _copy(pt, moved)
    other[k].shape_tag = 1
    for bad in (fewer, other):
        with pytest.raises(pt._lib.PtError) as e:
            gpu_ctx.scene_update(bad)
        assert e.value.code == PT_ERR_INVALID_ARG
        assert np.array_equal(gpu_ctx.render(cam, prm)[0].cpu().numpy(), want[0].cpu().numpy())
    empty = pt.Context(0)
    try:
        with pytest.raises(pt._lib.PtError):
            empty.scene_update(base)                            # no scene uploaded
    finally:
        empty.close()


# ------------------------------------------------------------------------------------------------------------- 2 ids
@pytest.mark.parametrize("scene", [1, 2, "spheres"])
def test_feature_ids_are_the_first_hits_of_the_camera_rays(pt, gpu_ctx, scene):
    gpu_ctx.upload(pt.builtin_scene(4, 200) if scene == "spheres" else pt.builtin_scene(scene))
    for W, H in ((33, 9), (97, 61)):
        cam = pt.camera_new(width=W, height=H)
        ys, xs = np.mgrid[0:H, 0:W]
        xys = np.stack([xs.ravel(), ys.ravel(), np.full(W * H, 7)], 1)
        for accel in (0, 1):
            for exact in (0, 1):
                prm = _prm(pt, 1, 7, accel=accel, exact_math=exact)
                ids = gpu_ctx.feature_ids(cam, prm)
                rays = gpu_ctx.debug_camera_rays(cam, xys, exact_math=exact)[:, :6]
                want, _ = gpu_ctx.debug_hit_scene(rays, t_min=prm.t_min, exact_math=exact, accel=accel)
                assert np.array_equal(ids.ravel(), want), (W, H, accel, exact, int((ids.ravel() != want).sum()))
                assert W < 97 or (ids >= 0).sum() >= 50          # (the 200 small spheres may miss all of 33 x 9)
    prm = _prm(pt, 4, 7)
    before = gpu_ctx.render_features(cam, prm, 3)
    gpu_ctx.feature_ids(cam, prm)
    assert np.array_equal(gpu_ctx.render_features(cam, prm, 3), before)


# --------------------------------------------------------------------------------- 3 nothing moves: the existing entry
def _arc(pt, i, W, H, step=0.01):
    phi = step * i
    return pt.camera_look_at((4 * np.sin(phi), 0.02 * i, -2 + 4 * np.cos(phi)), (0.0, 0.0, -2.0), (0.0, 1.0, 0.0), W, H, 35.0)


@pytest.mark.parametrize("camera", ["static", "moving"])
def test_nothing_moves_is_the_existing_entry(pt, gpu_ctx, ctx2, camera):
    W, H = 64, 48
    objs = pt.builtin_scene(2)
    gpu_ctx.upload(objs)
    frames = []
    for i in range(6):
        cam = _arc(pt, i if camera == "moving" else 0, W, H)
        prm = _prm(pt, 2, 2 * i)
        frames.append((cam, gpu_ctx.render(cam, prm)[0].cpu().numpy(), gpu_ctx.render_features(cam, prm, 1), gpu_ctx.feature_ids(cam, prm)))
    for it in (0, 3):
        ctx2.temporal_reset()
        want = [ctx2.denoise_temporal(cam, c, f, iterations=it) for cam, c, f, _ in frames]
        assert not np.array_equal(want[-1][0], ctx2.denoise(frames[-1][1], frames[-1][2], iterations=it)[0])   # history is in use
        for mixed in (False, True):
            gpu_ctx.temporal_reset()
            for i, (cam, c, f, ids) in enumerate(frames):
                gpu_ctx.scene_update(_copy(pt, objs))
                if mixed and i % 2:
                    got = gpu_ctx.denoise_temporal(cam, c, f, iterations=it)
                else:
                    got = gpu_ctx.denoise_temporal_motion(cam, c, f, ids, iterations=it)
                assert np.array_equal(got[0], want[i][0]) and np.array_equal(got[1], want[i][1]), (it, mixed, i)


# ------------------------------------------------------------------------------------ the committed cases on both sides
def _run_motion(pt, ctx, frames, iterations, **kw):
    ctx.upload(pt.make_objects(frames[0][4]))
    ctx.temporal_reset()
    out = []
    for k, (cam, c, f, ids, specs) in enumerate(frames):
        if k:
            ctx.scene_update(pt.make_objects(specs))
        out.append(ctx.denoise_temporal_motion(cam, c, f, ids, iterations=iterations, **kw))
    return out


def _fresh_on_gpu(ctx, frames, outs):
    """iterations = 0: a fresh pixel shows the frame's own film through the same demodulation, bit for bit."""
    return [np.all(o[0] == ctx.denoise(c, f, iterations=0)[0], axis=-1) for (_, c, f, _, _), o in zip(frames, outs)]


def _check_case(pt, ctx, name, iterations=(0, 2)):
    """Fresh masks and values of a committed case against the restatement, on the margin-safe pixels -> (frames, reference
    results, GPU fresh masks, compared masks at iterations 0)."""
    frames, kw = mc.case(pt, name)
    ref0 = mc.run_ref(frames, iterations=0, **kw)
    fresh = cmp0 = None
    for it in iterations:
        ref = ref0 if it == 0 else mc.run_ref(frames, iterations=it, **kw)
        outs = _run_motion(pt, ctx, frames, it, **kw)
        masks = mr.compared([info for _, info in ref], it)
        cmps = [m for m, _ in masks]
        for k, ((want, info), (lin, rgba)) in enumerate(zip(ref, outs)):
            cmp, frac = masks[k]
            err = _max_rel(lin[cmp], want[cmp])
            print(f"{name} it {it} frame {k}: safe {frac:.4f}, compared {cmp.mean():.3f}, fresh {info['fresh'].mean():.3f}, max rel err {err:.2e}")
            assert frac >= 0.95 and cmp.mean() >= mc.COMPARED[it], (name, it, k)
            assert err <= 1e-4
            assert np.array_equal(rgba, dr.rgba8(lin))
        if it == 0:
            fresh, cmp0 = _fresh_on_gpu(ctx, frames, outs), cmps
            for k, (_, info) in enumerate(ref):
                assert np.array_equal(fresh[k][cmp0[k]], info["fresh"][cmp0[k]]), (name, k)
    return frames, ref0, fresh, cmp0


# ------------------------------------------------------------------------ 4 moving everything = moving the camera
worst_translation = {}


@pytest.mark.parametrize("name", mc.TRANSLATIONS)
def test_moving_every_object_is_moving_the_camera(pt, gpu_ctx, ctx2, name):
    moving, static = mc.translation_case(pt, name)
    unsafe = [~tr.safe_mask(i)[0] for _, i in tc.run_ref(moving, iterations=0)]
    taps = [i for _, i in mc.run_ref(static, iterations=0)]   # the same taps, from the restatement that returns them
    for it in (0, 2):
        ctx2.temporal_reset()
        want = [ctx2.denoise_temporal(cam, c, f, iterations=it) for cam, c, f in moving]
        got = _run_motion(pt, gpu_ctx, static, it)
        masks = mr.compared(taps, it, unsafe)
        for k in range(len(moving)):
            cmp = masks[k][0]
            err = _max_rel(got[k][0][cmp], want[k][0][cmp])
            worst_translation[name] = max(worst_translation.get(name, 0.0), err)
            print(f"{name} it {it} frame {k}: compared {cmp.mean():.3f}, max rel difference {err:.2e}")
            assert cmp.mean() >= 0.5 or cmp.sum() >= 4      # (2 x 2: all four pixels)
            assert err <= 1e-4
    print(f"worst {name}: {worst_translation[name]:.2e}")


# -------------------------------------------------------------------------------------------------- 5 the mixed case
def test_a_sphere_moves_in_front_of_a_static_wall(pt, gpu_ctx, ctx2):
    frames, ref, fresh, cmp = _check_case(pt, gpu_ctx, "sphere")
    # wall pixels the sphere never covers: the existing entry under a static camera, bit for bit
    outs = _run_motion(pt, gpu_ctx, frames, 0)
    ctx2.temporal_reset()
    never = np.all([ids == 0 for _, _, _, ids, _ in frames], axis=0)
    assert never.mean() > 0.8
    for k, (cam, c, f, _, _) in enumerate(frames):
        want = ctx2.denoise_temporal(cam, c, f, iterations=0)
        assert np.array_equal(outs[k][0][never], want[0][never]) and np.array_equal(outs[k][1][never], want[1][never]), k
    for k in range(1, len(frames)):
        ids0, ids1 = frames[k - 1][3], frames[k][3]
        uncovered, onto = (ids0 == 1) & (ids1 == 0), (ids0 == 0) & (ids1 == 1)
        assert uncovered.sum() >= 10 and onto.sum() >= 10
        assert fresh[k][uncovered & cmp[k]].all() and not fresh[k][onto & cmp[k]].any(), k


# ---------------------------------------------------------------------------------------------- 6 the id gate alone
def test_the_id_gate_alone_separates_two_coplanar_quads(pt, gpu_ctx):
    frames, ref, fresh, cmp = _check_case(pt, gpu_ctx, "seam")
    for k in (1, 2):
        ids0, ids1 = frames[k - 1][3], frames[k][3]
        unc = (ids0 < 2) & (ids1 >= 2)                       # the static quad shows where the slider was
        assert (unc & cmp[k]).sum() >= 100 and fresh[k][unc & cmp[k]].all()
        S = ref[k][1]["S"]
        part = (S > 0.02) & (S < 0.98) & cmp[k]              # taps on both sides of a seam, one side refused: compared above
        print(f"seam frame {k}: uncovered {unc.sum()}, partial-weight pixels compared {part.sum()}")
        assert part.sum() >= 50


# -------------------------------------------------------------------------------------------- 7 a rotating triangle
def test_a_rotating_quad_keeps_its_history_through_the_carried_normal(pt, gpu_ctx):
    frames, ref, fresh, cmp = _check_case(pt, gpu_ctx, "rotation")
    for k in (1, 2):
        hit = (frames[k][3] >= 0) & cmp[k]
        print(f"rotation frame {k}: kept {(~fresh[k][hit]).mean():.3f} of {hit.sum()}")
        assert hit.sum() >= 500 and (~fresh[k][hit]).mean() > 0.8
    # with the pixel's own normal the gate refuses everything: the existing entry on the same buffers
    gpu_ctx.temporal_reset()
    for cam, c, f, _, _ in frames[:2]:
        out = gpu_ctx.denoise_temporal(cam, c, f, iterations=0, **mc.ROTATION_PARAMS)
    own = np.all(out[0] == gpu_ctx.denoise(frames[1][1], frames[1][2], iterations=0)[0], axis=-1)
    both = (frames[0][3] >= 0) & (frames[1][3] >= 0)
    assert own[both].all()


# ---------------------------------------------------------------------------------- 8 degenerate and hostile input
def test_hostile_ids_and_a_degenerate_history_pose_give_fresh_pixels(pt, gpu_ctx):
    """The kernel checks 0 <= id < n_objs before it reads maps[id] (k_denoise_temporal_motion: `known`)."""
    frames, ref, fresh, cmp = _check_case(pt, gpu_ctx, "hostile", iterations=(0,))
    assert fresh[1][10:].all() and not fresh[1][:10].any()
    gpu_ctx.sync()


# ------------------------------------------------------------------------------------------------------ 9 one call
def test_render_denoised_motion_is_the_composition_of_its_parts(pt, gpu_ctx):
    W, H = 80, 72
    base = pt.builtin_scene(1)
    k = _small_sphere(base)
    cam = pt.camera_new(width=W, height=H)
    seq = [_moved(pt, base, k, 0.05 * i) for i in range(3)]
    one = []
    gpu_ctx.upload(seq[0])
    for i in range(3):
        gpu_ctx.scene_update(seq[i])
        one.append(gpu_ctx.render_denoised_motion(cam, _prm(pt, 4, 4 * i), 2))
    gpu_ctx.upload(seq[0])
    for i in range(3):
        gpu_ctx.scene_update(seq[i])
        prm = _prm(pt, 4, 4 * i)
        noisy = gpu_ctx.render(cam, prm)[0].cpu().numpy()
        feat, ids = gpu_ctx.render_features(cam, prm, 2), gpu_ctx.feature_ids(cam, prm)
        lin, rgba = gpu_ctx.denoise_temporal_motion(cam, noisy, feat, ids)
        assert np.array_equal(one[i][2], noisy) and np.array_equal(one[i][3], feat) and np.array_equal(one[i][4], ids)
        assert np.array_equal(one[i][0], lin) and np.array_equal(one[i][1], rgba), i
    assert (one[2][4] == k).any()


def test_host_mirror_render_denoised_motion_gives_the_python_film(pt, gpu_ctx, tmp_path):
    """World::set_object + scene_update + render_denoised_motion of pathtrace.hpp (examples/motion_frames) = the Python calls."""
    exe = os.path.join(ROOT, "examples", "motion_frames")
    prefix = str(tmp_path / "mo")
    W, H = 96, 80
    r = subprocess.run([exe, str(W), str(H), "2", "3", prefix], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    base = pt.builtin_scene(1)
    k = next(i for i, o in enumerate(base) if o.shape_tag == 0)
    cam = pt.camera_new(width=W, height=H)
    gpu_ctx.upload(base)
    counts = []
    for i in range(3):
        gpu_ctx.scene_update(_moved(pt, base, k, 0.05 * i))
        lin, rgba, _, _, ids = gpu_ctx.render_denoised_motion(cam, _prm(pt, 2, 2 * i), 2)
        counts.append((k, int((ids == k).sum())))
    with open(prefix + ".ppm", "rb") as fh:
        assert fh.readline().strip() == b"P6"
        w, h = map(int, fh.readline().split())
        fh.readline()
        rgb = np.frombuffer(fh.read(), dtype=np.uint8).reshape(h, w, 3)
    assert np.array_equal(rgb, rgba[..., :3])
    assert [tuple(map(int, line.split())) for line in open(prefix + "_ids.txt")] == counts


# ------------------------------------------------------------------------------------------------------ 10 quality
def test_following_a_moving_sphere_beats_dropping_or_wrongly_keeping_the_history(pt, gpu_ctx, ctx2):
    """C2 at 128^2, 12 frames of 2 spp and 2 feature samples, 5 iterations; a small sphere crosses the floor.  Against 4096 spp
    from sample 10^6 of the last frame's scene: (a) the motion entry with pt_scene_update, (b) pt_scene_upload every frame
    with the existing entry (spatial only), (c) the history kept with all-identity poses (ghosting)."""
    S, N = 128, 12
    base = pt.builtin_scene(2)
    k = _small_sphere(base)
    cam = pt.camera_new(width=S, height=S)
    seq = [_moved(pt, base, k, 0.05 * (i - N // 2)) for i in range(N)]
    gpu_ctx.upload(seq[0])
    ctx2.upload(seq[0])
    swept = np.zeros((S, S), bool)
    for i in range(N):
        prm = _prm(pt, 2, 2 * i)
        gpu_ctx.scene_update(seq[i])
        a, _, noisy, feat, ids = gpu_ctx.render_denoised_motion(cam, prm, 2)
        swept |= ids == k
        ctx2.scene_update(seq[0])                            # (c): unchanged objects, the moved scene's films
        c = ctx2.denoise_temporal_motion(cam, noisy, feat, ids)[0]
    gpu_ctx.upload(seq[-1])                                  # (b): the history is gone, the frame is the spatial filter's
    b = gpu_ctx.denoise_temporal(cam, noisy, feat)[0]
    ref = gpu_ctx.render(cam, _prm(pt, 4096, 1000000))[0].cpu().numpy().astype(np.float64)
    keep = feat[..., 3] == 0                                 # non-emitter pixels

    def rel(x, m):
        return float(np.mean(((x.astype(np.float64) - ref) ** 2 / (ref ** 2 + 0.01))[m]))
    ra, rb, rc = rel(a, keep), rel(b, keep), rel(c, keep)
    sa, sc = rel(a, keep & swept), rel(c, keep & swept)
    print(f"relMSE whole image: motion {ra:.5f}, upload every frame {rb:.5f}, history wrongly kept {rc:.5f}; motion / upload "
          f"{ra / rb:.3f}; swept footprint ({int((keep & swept).sum())} px): motion {sa:.5f}, wrongly kept {sc:.5f}, ratio {sa / sc:.3f}")
    assert ra <= rb
    assert sa < sc
