"""The refusals of the film and bake entries that lie behind their first read of the context (test_entry_refusals_cpu.py pins the
ones in front of it): a fresh context with no scene uploaded, arguments that pass every check of the entry's own, an 8 x 8 film
(2 probes of 4 rays for the bakes).  Every call is refused before anything is launched, with render_impl's words; the expected
texts are those of commit 05349f1's source (check_scene_and_camera in pt_api.cpp, check_target in pt_denoise.cpp, and the copies
pt_filter.cpp, pt_cascade.cpp and pt_probe_grid.cpp held then).
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PT_ERR_INVALID_ARG = 1
NO_SCENE = "render: no scene uploaded"


@pytest.fixture(scope="module")
def bare(pt):
    """a context that never saw a scene, and the planes of the calls: device memory for the device entries, host arrays for the others"""
    import torch
    ctx = pt.Context(0)
    dev = {k: torch.zeros(n, dtype=torch.float32, device="cuda:0") for k, n in (("lin", 192), ("rgba", 64), ("plain", 192), ("in", 384), ("sh", 54))}
    host = {k: np.zeros(n, dtype=np.float32) for k, n in (("lin", 192), ("rgba", 64), ("plain", 192))}
    yield ctx, {k: C.c_void_p(v.data_ptr()) for k, v in dev.items()}, {k: v.ctypes.data_as(C.c_void_p) for k, v in host.items()}, (dev, host)
    ctx.close()


def _calls(pt, c, d, h):
    cam, prm = C.byref(pt.camera_new(width=8, height=8)), C.byref(pt.default_params(spp=2))
    flt, cs = C.byref(pt.default_filter()), C.byref(pt.default_cascade())
    grid, sp = C.byref(pt.probe_grid((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (2, 1, 1))), C.byref(pt.default_probe_shade())
    lens, proj = C.byref(pt.default_lens()), C.byref(pt.default_projection())
    return {
        "pt_render_filtered_device": (c, cam, prm, flt, d["lin"], d["rgba"], d["plain"]),
        "pt_render_filtered_host": (c, cam, prm, flt, h["lin"], h["rgba"], h["plain"], None),
        "pt_render_cascade_device": (c, cam, prm, cs, d["lin"], d["rgba"], d["plain"]),
        "pt_render_cascade_host": (c, cam, prm, cs, h["lin"], h["rgba"], h["plain"], None, None),
        "pt_bake_lightmap_device": (c, 8, 8, d["in"], prm, d["lin"], d["rgba"]),
        "pt_bake_probes_device": (c, d["in"], 2, 4, prm, d["lin"], d["sh"]),
        "pt_probe_grid_bake_device": (c, grid, 4, prm, d["sh"]),
        "pt_render_probe_lit_device": (c, cam, prm, 2, grid, d["sh"], None, sp, d["lin"], d["rgba"]),
        "pt_render_lens_host": (c, cam, lens, prm, h["lin"], h["rgba"]),
        "pt_render_projection_host": (c, cam, proj, prm, h["lin"], h["rgba"]),
    }


ENTRIES = ("pt_render_filtered_device", "pt_render_filtered_host", "pt_render_cascade_device", "pt_render_cascade_host", "pt_bake_lightmap_device",
           "pt_bake_probes_device", "pt_probe_grid_bake_device", "pt_render_probe_lit_device", "pt_render_lens_host", "pt_render_projection_host")


@pytest.mark.parametrize("entry", ENTRIES)
def test_without_a_scene_the_entry_refuses_in_the_render_words(pt, bare, entry):
    ctx, d, h, _keep = bare
    lib = pt._lib.lib()
    rc = getattr(lib, entry)(*_calls(pt, ctx._h, d, h)[entry])
    assert [rc, lib.pt_last_error().decode()] == [PT_ERR_INVALID_ARG, NO_SCENE]
