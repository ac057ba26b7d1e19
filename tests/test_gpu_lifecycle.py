"""A context's lifetime on the GPU: created, used over every group of buffers it owns, and destroyed again and again in one
process; an upload that is rejected; a change of stream between two renders.  The members of PtContext free what they own
(csrc/pt_context.h); what these tests pin is that a context built and torn down that way computes what a long-lived one does."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
PT_ERR_INVALID_ARG = 1
PT_ACCEL_BVH = 1
SMALL_OBJS = 128          # ptk::kSmallObjs: one object more and the scene no longer lives in LDS


def _copy(pt, objs):
    return (pt._lib.PtObject * len(objs))(*objs)


def _render_host(pt, ctx, cam, prm):
    """pt_render_host on the context (host buffers, blocking)"""
    lin = np.empty((cam.height, cam.width, 3), dtype=np.float32)
    rgba = np.empty((cam.height, cam.width, 4), dtype=np.uint8)
    pt._lib.check(pt._lib.lib().pt_render_host(ctx._h, C.byref(cam), C.byref(prm), lin.ctypes.data_as(C.c_void_p),
                                               rgba.ctypes.data_as(C.c_void_p)))
    return lin, rgba


def _workload(pt, ctx):
    """Four jobs that between them touch the scene, BVH, wavefront, scheduling, statistics, adaptive, feature, denoiser,
    temporal and motion buffers of a context.  -> their outputs, as a flat list of arrays"""
    cam = pt.camera_new(width=32, height=32)
    out = []
    ctx.upload(pt.builtin_scene(1))
    out += _render_host(pt, ctx, cam, pt.default_params(spp=4))
    out += ctx.render_adaptive(cam, pt.default_params(spp=4), spp_min=2, spp_step=2, rel_tol=0.05)
    base = pt.builtin_scene(2)
    k = min((i for i, o in enumerate(base) if o.shape_tag == 0 and o.mat_tag != 1), key=lambda i: base[i].shape[3])
    moved = _copy(pt, base)
    moved[k].shape[0] += 0.2
    ctx.upload(base)
    ctx.render_denoised_motion(cam, pt.default_params(spp=4), feature_samples=2)
    ctx.scene_update(moved)
    out += ctx.render_denoised_motion(cam, pt.default_params(spp=4, spp_offset=4), feature_samples=2)
    ctx.upload(pt.builtin_scene(4, SMALL_OBJS + 1))
    out += _render_host(pt, ctx, cam, pt.default_params(spp=4, accel=PT_ACCEL_BVH))
    return out


def _same(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_create_use_destroy_three_times_gives_what_a_long_lived_context_gives(pt):
    keep = pt.Context(0)
    try:
        ref = _workload(pt, keep)
        assert all(np.isfinite(a).all() for a in ref if a.dtype.kind == "f")
        assert float(ref[0].max()) > 0.0 and float(ref[-2].max()) > 0.0
        for cycle in range(3):
            ctx = pt.Context(0)
            try:
                got = _workload(pt, ctx)
            finally:
                ctx.close()
            assert _same(got, ref), "cycle %d differs from the long-lived context" % (cycle + 1)
        assert _same(_workload(pt, keep), ref)      # ... which stayed alive throughout
    finally:
        keep.close()


def test_rejected_upload_leaves_the_uploaded_scene_in_place(pt):
    cam = pt.camera_new(width=32, height=32)
    prm = pt.default_params(spp=4)
    ctx = pt.Context(0)
    try:
        ctx.upload(pt.builtin_scene(1))
        layout = ctx.scan_layout()
        ref = _render_host(pt, ctx, cam, prm)
        bad = _copy(pt, pt.builtin_scene(4, 40))     # another layout altogether; its last object carries the bad tag
        bad[len(bad) - 1].mat_tag = 9
        with pytest.raises(pt._lib.PtError) as e:
            ctx.upload(bad)
        assert e.value.code == PT_ERR_INVALID_ARG
        assert ctx.scan_layout() == layout
        assert _same(_render_host(pt, ctx, cam, prm), ref)
    finally:
        ctx.close()


def test_stream_switched_and_back_between_two_renders_gives_the_same_films(pt):
    import torch
    dev = torch.device("cuda", 0)
    cam = pt.camera_new(width=64, height=64)
    prms = [pt.default_params(spp=4), pt.default_params(spp=4, spp_offset=4)]
    s1, s2 = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    ctx = pt.Context(0)
    try:
        ctx.upload(pt.builtin_scene(1))
        films = []
        for switch in (False, True):
            lin = [torch.zeros((64, 64, 3), dtype=torch.float32, device=dev) for _ in prms]
            rgba = [torch.zeros((64, 64, 4), dtype=torch.uint8, device=dev) for _ in prms]
            torch.cuda.synchronize(dev)
            ctx.set_stream(s1.cuda_stream)
            ctx.render_into(cam, prms[0], lin[0].data_ptr(), rgba[0].data_ptr())
            if switch:
                ctx.set_stream(s2.cuda_stream)
                ctx.set_stream(s1.cuda_stream)
            ctx.render_into(cam, prms[1], lin[1].data_ptr(), rgba[1].data_ptr())
            ctx.sync()
            films.append([t.cpu().numpy() for t in lin + rgba])
        assert float(films[0][0].max()) > 0.0 and not np.array_equal(films[0][0], films[0][1])
        assert _same(films[1], films[0])
    finally:
        ctx.set_stream(None)
        ctx.close()
