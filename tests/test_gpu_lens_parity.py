"""The thin-lens entries against the oracle's own statement of the lens rule (oracle/pt_oracle.hpp "thin lens"), on
the GPU.  tests/test_gpu_lens.py holds the lens to the pinhole at aperture 0 and to itself; here every entry is held, with an
OPEN lens, to an independent film:

  * exact arithmetic: the rays, the linear film, RGBA8, every band, every batch split, every depth limit and the feature
    buffers are the f32 iterative oracle's bit for bit;
  * fast arithmetic: the same jobs within the project's FP32 bar (test_gpu_kernel_instances._within_bar) of the f64 recursive
    oracle, the share of pixels outside the bar printed beside that of the same job through the pinhole;
  * the launch log of each job shows the scan it was meant for -- k_paths over the scene in LDS, k_paths over tiles (more than
    128 objects), k_paths_bvh -- taking up the lens paths.

Counters: a lens render is several render_impl calls on one stream with no collection between them (begin_period runs only for
the first render after pt_sync / pt_get_stats, and the binding collects after every entry), so all its batches fall into one
statistics period: `samples`, `vertices` and `shadow_rays` of a whole film are compared with the oracle's.

The jobs (tests/lens_parity_jobs.py) pass the fast bar on the reference alone, f32 oracle against f64 oracle
(tests/test_oracle_lens.py)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import denoise_ref as dr
import lens_parity_jobs as lj

pytestmark = pytest.mark.gpu
THREADS = min(16, os.cpu_count() or 1)
LOOK = ((1.0, 0.7, 2.0), (0.0, -0.1, -2.0), (0.1, 1.0, 0.0), 37, 23, 33.0)


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a,
                                                                        b.view(np.uint32) if b.dtype == np.float32 else b)


def _render(pt, ctx, job, **over):
    """One GPU lens render of the job -> dict(lin, rgba, stats, log)"""
    objs, cam, lens, prm = lj.make(pt, job, **over)
    ctx.upload(objs)
    ctx.launch_log()
    lin, rgba = ctx.render_lens(cam, lens, prm)
    st = ctx.stats()
    return dict(lin=lin.cpu().numpy(), rgba=rgba.cpu().numpy(), log=ctx.launch_log(), batches=st.batches, samples=st.samples,
                samples_expected=st.samples_expected, vertices=st.vertices, shadow_rays=st.shadow_rays)


def _oracle(pt, orc, job, precision, **over):
    objs, cam, lens, prm = lj.make(pt, job, **over)
    return orc.render_lens(cam, lens, objs, prm, precision, orc.ITERATIVE if precision == orc.F32 else orc.RECURSIVE, THREADS)


@functools.lru_cache(maxsize=None)
def _oracle_whole(pt, orc, job, precision):
    return _oracle(pt, orc, job, precision)


def _check_route(pt, job, log, exact):
    """The job's launches are queue-form launches of the scan it was built for (a lens render never regenerates)."""
    ds = [pt.path_instance(c) for c in log]
    assert ds and all(d["exact"] == bool(exact) for d in ds), [d["kernel"] for d in ds]
    assert all(d["mis"] == (job[2] == lj.MIS) for d in ds)
    want = lj.route(job)
    if want == "bvh":
        assert all(d["family"] == "k_paths_bvh" for d in ds), [d["kernel"] for d in ds]
    else:
        assert all(d["family"] == "k_paths" and d["mode"] == (1 if want == "tiled" else 0) for d in ds), [d["kernel"] for d in ds]


def _assert_film_is_the_oracles(r, ref, what=""):
    lin, rgba = ref[0].astype(np.float32), ref[1]
    assert r["lin"].shape == lin.shape
    assert _same(r["lin"], lin), f"{what}: {int((r['lin'] != lin).any(-1).sum())} of {lin.shape[0] * lin.shape[1]} pixels differ from the f32 oracle"
    assert _same(r["rgba"], rgba), what


# ---------------------------------------------------------------- 1. rays
@pytest.mark.parametrize("aperture,focus", [(0.3, 2.5), (3.0, 0.7)])
def test_exact_rays_are_the_f32_oracles(pt, orc, gpu_ctx, aperture, focus):
    gpu_ctx.upload(pt.builtin_scene(2))
    cam = pt.camera_look_at(*LOOK)
    lens = pt.default_lens(aperture=aperture, focus_distance=focus)
    rng = np.random.default_rng(17)
    n = 4096
    xys = np.stack([rng.integers(0, 37, n), rng.integers(0, 23, n), rng.integers(0, 2 ** 32, n)], axis=1).astype(np.uint32)
    corners = [(x, y, s) for x in (0, 36) for y in (0, 22) for s in (0, 2 ** 32 - 1)]
    xys = np.concatenate([np.array(corners, dtype=np.uint32), xys])
    got = gpu_ctx.lens_rays(cam, lens, xys, exact_math=1)
    ref = orc.lens_rays(cam, lens, xys, orc.F32)
    assert np.array_equal(ref, ref.astype(np.float32).astype(np.float64))
    bad = (got.view(np.uint32) != ref.astype(np.float32).view(np.uint32)).any(axis=1)
    assert not bad.any(), (int(bad.sum()), xys[bad][:4], got[bad][:4], ref[bad][:4])
    assert np.linalg.norm(got[:, 0:3] - np.array(list(cam.origin), dtype=np.float32), axis=1).max() > 0.45 * aperture      # to the rim


# ---------------------------------------------------------------- 2. films
@pytest.mark.parametrize("job", lj.JOBS, ids=lj.job_id)
def test_exact_film_is_the_f32_oracles(pt, orc, gpu_ctx, job):
    r = _render(pt, gpu_ctx, job, exact_math=1)
    _check_route(pt, job, r["log"], 1)
    ref = _oracle_whole(pt, orc, job, orc.F32)
    _assert_film_is_the_oracles(r, ref, lj.job_id(job))
    (w, h), spp = job[4], job[6]
    assert r["samples"] == r["samples_expected"] == w * h * spp
    assert (r["vertices"], r["shadow_rays"]) == (ref[2]["vertices"], ref[2]["shadow_rays"])
    assert float(r["lin"].max()) > 0 and ref[2]["vertices"] > w * h * spp


@pytest.mark.parametrize("job", lj.JOBS, ids=lj.job_id)
def test_fast_film_is_within_the_fp32_bar_of_the_f64_oracle(pt, orc, gpu_ctx, job):
    r = _render(pt, gpu_ctx, job)
    _check_route(pt, job, r["log"], 0)
    ref = _oracle_whole(pt, orc, job, orc.F64)
    objs, cam, lens, prm = lj.make(pt, job)
    pin = gpu_ctx.render(cam, prm)[0].cpu().numpy()
    pin_ref = orc.render(cam, objs, prm, orc.F64, orc.RECURSIVE, THREADS)[0]
    (ls, lm), (ps, pm) = lj.outside_bar(r["lin"], ref[0]), lj.outside_bar(pin, pin_ref)
    print(f"{lj.job_id(job)}: outside the FP32 bar lens {ls:.4%} (mean off {lm:.1e}), pinhole {ps:.4%} ({pm:.1e})")
    assert r["samples"] == r["samples_expected"] == cam.width * cam.height * prm.spp
    lj.within_bar(r["lin"], ref[0])


# ---------------------------------------------------------------- 3. batches, bands, depth limits
@pytest.mark.parametrize("job", [lj.JOBS[0], lj.JOBS[9]], ids=lj.job_id)
def test_batches_add_up_to_the_oracles_film(pt, orc, gpu_ctx, job):
    """spp 6 with room for two samples of every pixel: three batches, the f64 film sums carried between them"""
    assert job[6] == 6
    w, h = job[4]
    r = _render(pt, gpu_ctx, job, exact_math=1, max_paths_in_flight=2 * w * h)
    assert r["batches"] >= 3 and len(r["log"]) >= 3
    _check_route(pt, job, r["log"], 1)
    ref = _oracle_whole(pt, orc, job, orc.F32)
    _assert_film_is_the_oracles(r, ref)
    assert r["samples"] == r["samples_expected"] == w * h * 6
    assert (r["vertices"], r["shadow_rays"]) == (ref[2]["vertices"], ref[2]["shadow_rays"])


@pytest.mark.parametrize("job", [lj.JOBS[2], lj.JOBS[8]], ids=lj.job_id)
def test_every_band_is_the_oracles_band(pt, orc, gpu_ctx, job):
    rows = 0
    for band in range(3):
        kw = dict(exact_math=1, band_rows=8, band_count=3, band_index=band)
        r = _render(pt, gpu_ctx, job, **kw)
        ref = _oracle(pt, orc, job, orc.F32, **kw)
        _assert_film_is_the_oracles(r, ref, f"band {band}")
        assert (r["vertices"], r["shadow_rays"]) == (ref[2]["vertices"], ref[2]["shadow_rays"])
        rows += r["lin"].shape[0]
    assert rows == job[4][1]


@pytest.mark.parametrize("depths", [(1, 1), (0, 2), None], ids=["1-1", "0-2", "defaults"])
@pytest.mark.parametrize("job", [lj.JOBS[0], lj.JOBS[2], lj.JOBS[6]], ids=lj.job_id)
def test_depth_limits_against_the_oracle(pt, orc, gpu_ctx, job, depths):
    kw = dict(exact_math=1)
    if depths:
        kw.update(min_depth=depths[0], max_depth=depths[1])
    r = _render(pt, gpu_ctx, job, **kw)
    ref = _oracle(pt, orc, job, orc.F32, **kw)
    _assert_film_is_the_oracles(r, ref)
    assert (r["vertices"], r["shadow_rays"]) == (ref[2]["vertices"], ref[2]["shadow_rays"])
    if depths:      # (the limit does something: fewer vertices than the defaults allow)
        assert ref[2]["vertices"] < _oracle_whole(pt, orc, job, orc.F32)[2]["vertices"]


# ---------------------------------------------------------------- 4. features
@pytest.mark.parametrize("accel", [0, 1])
@pytest.mark.parametrize("scene,lens", [("mirror", "wide"), ("tiled", "narrow"), ("diffuse", "narrow")])
def test_exact_lens_features_are_the_f32_restatement(pt, orc, gpu_ctx, scene, lens, accel):
    objs = pt.builtin_scene(*lj.SCENES[scene])
    gpu_ctx.upload(objs)
    cam = pt.camera_look_at((0.3, 0.2, -1.2), (0.0, -0.1, -2.0), (0.1, 1.0, 0.0), 37, 23, 60.0) if scene == "tiled" else pt.camera_look_at(*LOOK)
    ln = pt.default_lens(**lj.LENSES[lens])
    prm = pt.default_params(spp=16, spp_offset=7, exact_math=1, accel=accel)
    pin = gpu_ctx.render_features(cam, prm, 4)
    for n in (1, 4):
        got = gpu_ctx.render_features_lens(cam, ln, prm, n)
        ref = dr.features_f32(orc, objs, cam, 7, n, lens=ln)
        assert got.shape == (23, 37, 8)
        assert _same(got, ref), np.argwhere(got != ref)[:5]
    assert (got[..., 7] > 0).any() and not _same(got, pin)


# ---------------------------------------------------------------- 5. the host entry
def test_render_lens_host_gives_the_device_entrys_bits(pt, gpu_ctx):
    job = lj.JOBS[2]
    objs, cam, lens, prm = lj.make(pt, job, exact_math=0, band_rows=8, band_count=3, band_index=1)
    gpu_ctx.upload(objs)
    lin, rgba = gpu_ctx.render_lens(cam, lens, prm)
    rows = lin.shape[0]
    out_lin = np.full((rows, cam.width, 3), np.nan, dtype=np.float32)
    out_rgba = np.zeros((rows, cam.width, 4), dtype=np.uint8)
    rc = pt._lib.lib().pt_render_lens_host(gpu_ctx._h, C.byref(cam), C.byref(lens), C.byref(prm), out_lin.ctypes.data_as(C.c_void_p),
                                           out_rgba.ctypes.data_as(C.c_void_p))
    assert rc == 0, pt._lib.lib().pt_last_error().decode()
    assert _same(out_lin, lin.cpu().numpy()) and _same(out_rgba, rgba.cpu().numpy())
    assert float(out_lin.max()) > 0
