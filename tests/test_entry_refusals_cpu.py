"""The refusals of the film, bake and camera entries that need no device, pinned: for every extern "C" entry that returns a code in
pt_filter.cpp, pt_cascade.cpp, pt_bake.cpp, pt_probe_grid.cpp, pt_tonemap.cpp, pt_bloom.cpp, pt_upsample.cpp, pt_projection.cpp and
pt_lens.cpp, and for the two lens renders of pt_api.cpp, every check it makes before it first reads the context -- each alone, each
pair of checks that follow one another (the pair pins their order: the earlier one answers), and the null context -- against the
(return code, pt_last_error() text) that commit 05349f1 gave, in tests/golden/entry_refusals.json: per entry one line per answer,
[code, message, the cases that get it], with {who} for the entry's own name.  (What lies behind the first read of the context --
"render: no scene uploaded" and everything after it -- is pinned on a device: test_gpu_entry_refusals.py.)

The table is a record of that commit, not of the code under test.  It was written by

    git worktree add ../parent 05349f1 && cp tests/test_entry_refusals_cpu.py tests/refusal_cases.py ../parent/tests/ &&
    (cd ../parent && python -c "import __graft_entry__ as g; g.build()" && python tests/test_entry_refusals_cpu.py --record) &&
    cp ../parent/tests/golden/entry_refusals.json tests/golden/

and is only ever recorded again from a commit whose refusals are meant to be the new truth.  ENTRIES below restates that
commit's order of checks, entry by entry (the machinery: refusal_cases.py); the context is a pointer that is never followed.  A
case that a check lets through is given a null context, or a null plane that a later check refuses, so that it is refused
all the same, by the answer the table shows.

The alias checks of the filter and the cascade come behind the alignment check, and every plane is a whole number of 4-byte
words: the least overlap of two ranges that reaches them is one word, not one byte.  The cases take that word (the last one of
the range in front), and the ranges that only touch.
"""
import ctypes as C
import math
import os
import re
import sys

import pytest

from refusal_cases import BAD_F, HUGE, at, call as _call, cases as _cases, floats, merge, nulls, record, table_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "golden", "entry_refusals.json")

# the planes of an 8 x 8 image (64 pixels) with n = 2 samples, apart from one another in the scratch: the samples 1536 bytes,
# a film plane 768, an RGBA8 plane 256, the weight sums 512
SAMPLES, LIN, RGBA, PLAIN, WSUM, FEAT, FAKE = (at(k) for k in (0, 2048, 3072, 3584, 4608, 5120, 8192))
SAMPLES_END, LIN_END = 1536, 2048 + 768
ODD = at(16384 + 2)             # no multiple of 4
ODD8 = at(16384 + 4)            # of 4, not of 8
ODD16 = at(16384 + 8)           # of 8, not of 16
U32 = (C.c_uint32 * 16)()
F64 = (C.c_double * 4)()
F32 = (C.c_float * 16)()
U8 = (C.c_uint8 * 4)()


def xys(x, y):
    return (C.c_uint32 * 3)(x, y, 0)


# ---------------------------------------------------------------- the structs, by argument name
def _grid(pt):
    return pt.probe_grid((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (2, 1, 1))


STRUCTS = {
    "cam": lambda pt: pt.camera_new(width=8, height=8),
    "prm": lambda pt: pt.default_params(spp=2),
    "flt": lambda pt: pt.default_filter(),
    "cs": lambda pt: pt.default_cascade(),
    "tm": lambda pt: pt.default_tonemap(),
    "bl": lambda pt: pt.default_bloom(),
    "up": lambda pt: pt.default_upsample(),
    "dn": lambda pt: pt.default_denoise(),
    "lens": lambda pt: pt.default_lens(),
    "proj": lambda pt: pt.default_projection(),
    "g": _grid,
    "sp": lambda pt: pt.default_probe_shade(),
}


def _struct(pt, name, fields):
    s = STRUCTS[name](pt)
    for k, v in fields.items():
        setattr(s, k, v)
    return s


# ---------------------------------------------------------------- the arguments of a call that passes every check
_image = dict(width=8, height=8)
_planes = dict(lin=LIN, rgba=RGBA, plain=PLAIN)
_shade = dict(g={}, sh27=SAMPLES, feat=FEAT, fallback=None, sp={}, lin=LIN, rgba=RGBA)
_lit = dict(c=FAKE, cam={}, prm={}, fs=2, g={}, sh27=SAMPLES, fallback=None, sp={}, lin=LIN, rgba=RGBA)
_upsample = dict(lo_width=8, lo_height=8, lo_lin=SAMPLES, lo_feat=FEAT, **_image, feat=at(6144), up={}, lin=LIN, rgba=RGBA)
_display = dict(c=FAKE, **_image, lin=LIN, bl={}, tm={}, out=PLAIN, rgba=RGBA)
_outs4 = dict(lin=LIN, rgba=None, o1=None, o2=None)
GOOD = {
    # pt_filter.cpp
    "pt_debug_filter_weight": dict(flt={}, t=0.5, f=F64),
    "pt_debug_filter_offsets": dict(x=0, y=0, sample=0, ox=F64, oy=F64),
    "pt_debug_filter_exp_neg": dict(e=1.0, out=F64),
    "pt_filter_host": dict(flt={}, **_image, n=2, first=0, samples=SAMPLES, **_planes, wsum=WSUM),
    "pt_filter_samples_device": dict(c=FAKE, flt={}, **_image, n=2, first=0, batch=0, samples=SAMPLES, **_planes, wsum=WSUM),
    "pt_render_filtered_device": dict(c=FAKE, cam={}, prm={}, flt={}, **_planes),
    "pt_render_filtered_host": dict(c=FAKE, cam={}, prm={}, flt={}, **_planes, wsum=WSUM),
    # pt_cascade.cpp
    "pt_debug_cascade_split": dict(cs={}, L=1.0, j=U32, w_lo=F64, w_hi=F64),
    "pt_cascade_host": dict(cs={}, **_image, n=2, samples=SAMPLES, **_planes, layers=None, weights=None),
    "pt_cascade_samples_device": dict(c=FAKE, cs={}, **_image, n=2, batch=0, samples=SAMPLES, **_planes),
    "pt_render_cascade_device": dict(c=FAKE, cam={}, prm={}, cs={}, **_planes),
    "pt_render_cascade_host": dict(c=FAKE, cam={}, prm={}, cs={}, **_planes, layers=None, weights=None),
    # pt_bake.cpp
    "pt_bake_lightmap_device": dict(c=FAKE, **_image, tex=SAMPLES, prm={}, lin=LIN, rgba=RGBA),
    "pt_bake_lightmap_host": dict(c=FAKE, **_image, tex=SAMPLES, prm={}, lin=LIN, rgba=RGBA),
    "pt_bake_probes_device": dict(c=FAKE, pos=SAMPLES, n_probes=2, rays=4, prm={}, rad=LIN, sh27=PLAIN),
    "pt_bake_probes_host": dict(c=FAKE, pos=SAMPLES, n_probes=2, rays=4, prm={}, rad=LIN, sh27=PLAIN),
    "pt_sh_project_device": dict(c=FAKE, n_probes=2, rays=4, rad=LIN, sh27=PLAIN),
    "pt_sh_project_host": dict(n_probes=2, rays=4, rad=LIN, sh27=PLAIN),
    "pt_sh_irradiance_host": dict(sh27=PLAIN, normals=SAMPLES, n=1, out=LIN),
    "pt_bake_rays_host": dict(kind=0, **_image, data=SAMPLES, xys=xys(0, 0), n=1, out=LIN),
    "pt_debug_bake_rays": dict(c=FAKE, kind=0, **_image, data=SAMPLES, xys=xys(0, 0), n=1, exact=0, out=LIN),
    # pt_probe_grid.cpp
    "pt_probe_grid_positions_host": dict(g={}, out=LIN),
    "pt_probe_grid_bake_device": dict(c=FAKE, g={}, rays=4, prm={}, sh27=PLAIN),
    "pt_probe_shade_device": dict(c=FAKE, cam={}, **_shade),
    "pt_probe_shade_host": dict(cam={}, **_shade),
    "pt_render_probe_lit_device": dict(_lit),
    "pt_render_probe_lit_host": dict(_lit),
    "pt_debug_probe_positions": dict(c=FAKE, g={}, out=LIN),
    # pt_tonemap.cpp
    "pt_film_histogram_device": dict(c=FAKE, **_image, lin=LIN, hist=PLAIN),
    "pt_tonemap_device": dict(c=FAKE, **_image, lin=LIN, tm={}, out=PLAIN, rgba=RGBA),
    "pt_tonemap_host": dict(c=FAKE, **_image, lin=LIN, tm={}, out=PLAIN, rgba=RGBA),
    "pt_exposure_reset": dict(c=FAKE),
    "pt_debug_exposure_state": dict(c=FAKE, log2E=None, E=None, valid=None, hist=None),
    "pt_exposure_get": dict(c=FAKE, log2E=F64, hist=None),
    "pt_debug_tonemap_pixel": dict(tm={}, E=1.0, rgb=F32, y=F32, rgba=U8),
    # pt_bloom.cpp
    "pt_bloom_device": dict(c=FAKE, **_image, lin=LIN, bl={}, out=PLAIN),
    "pt_display_device": dict(_display),
    "pt_display_host": dict(_display),
    "pt_bloom_host": dict(**_image, lin=LIN, bl={}, out=PLAIN),
    "pt_debug_bloom_plan": dict(**_image, levels=2, wh=U32, n_levels=U32, first_tail=U32),
    "pt_debug_bloom_bright": dict(bl={}, lin=LIN, out=PLAIN),
    "pt_debug_bloom_tail": dict(c=FAKE, enable=1),
    # pt_upsample.cpp
    "pt_upsample_device": dict(c=FAKE, **_upsample),
    "pt_upsample_host": dict(_upsample),
    "pt_render_denoised_upsampled": dict(c=FAKE, cam={}, prm={}, lo_width=4, lo_height=4, fs=2, dn={}, up={}, **_outs4),
    # pt_projection.cpp
    "pt_render_projection_device": dict(c=FAKE, cam={}, proj={}, prm={}, lin=LIN, rgba=RGBA),
    "pt_render_projection_host": dict(c=FAKE, cam={}, proj={}, prm={}, lin=LIN, rgba=RGBA),
    "pt_render_features_projection_device": dict(c=FAKE, cam={}, proj={}, prm={}, n=2, feat=FEAT),
    "pt_render_projection_denoised": dict(c=FAKE, cam={}, proj={}, prm={}, fs=2, dn={}, **_outs4),
    "pt_render_rays_device": dict(c=FAKE, **_image, prm={}, rays6=SAMPLES, weights3=None, lin=LIN, rgba=RGBA),
    "pt_projection_setup_host": dict(cam={}, proj={}, out=F32),
    "pt_projection_rays_host": dict(cam={}, proj={}, xys=xys(0, 0), n=1, out=F32),
    "pt_debug_projection_rays": dict(c=FAKE, cam={}, proj={}, xys=xys(0, 0), n=1, exact=0, out=F32),
    # pt_lens.cpp
    "pt_render_features_lens_device": dict(c=FAKE, cam={}, lens={}, prm={}, n=2, feat=FEAT),
    "pt_render_lens_denoised": dict(c=FAKE, cam={}, lens={}, prm={}, fs=2, dn={}, **_outs4),
    "pt_debug_lens_setup": dict(cam={}, lens={}, out=F32),
    "pt_debug_lens_rays": dict(c=FAKE, cam={}, lens={}, xys=xys(0, 0), n=1, exact=0, out=F32),
    # pt_api.cpp: the lens renders
    "pt_render_lens_device": dict(c=FAKE, cam={}, lens={}, prm={}, lin=LIN, rgba=RGBA),
    "pt_render_lens_host": dict(c=FAKE, cam={}, lens={}, prm={}, lin=LIN, rgba=RGBA),
}

# ---------------------------------------------------------------- the checks, in the order 05349f1 makes them
NO_CONTEXT = [("null context", {"c": None})]
BAND = [("band_count=2", {"prm": {"band_rows": 2, "band_count": 2}}), ("band_index=1", {"prm": {"band_index": 1}})]
SPP = [("spp=0", {"prm": {"spp": 0}})]
FS = [("feature_samples=0", {"fs": 0})]
N0 = [("n=0", {"n": 0})]
DENOISE = [[("iterations=17", {"dn": {"iterations": 17}})],
           floats("dn", "sigma_l") + floats("dn", "sigma_n", BAD_F[:1]) + floats("dn", "sigma_d", BAD_F[1:2])]
# a size as two integers (image=True) or in the camera
def _small(cam):
    return [(f"image {w}x{h}", {"cam": {"width": w, "height": h}} if cam else {"width": w, "height": h}) for w, h in ((1, 8), (8, 1), (0, 0))]


def _huge(cam):
    return [("2^31 pixels", {"cam": HUGE} if cam else dict(HUGE))]


def _size(cam):
    return [_small(cam), _huge(cam)]


def _plane(name, odd=ODD, null=True):
    return ([(f"null {name}", {name: None})] if null else []) + [(f"{name} misaligned", {name: odd})]


FILTER = [[("kind=4", {"flt": {"kind": 4}})],
          [("radius=nan", {"flt": {"radius": math.nan}}), ("radius=0.4", {"flt": {"radius": 0.4}}), ("radius=2.6", {"flt": {"radius": 2.6}})],
          [("gaussian a=0", {"flt": {"a": 0.0}}), ("gaussian a=17", {"flt": {"a": 17.0}}), ("gaussian a=nan", {"flt": {"a": math.nan}})],
          [("mitchell b=2", {"flt": {"kind": 3, "a": 0.5, "b": 2.0}}), ("mitchell a=-0.1", {"flt": {"kind": 3, "a": -0.1, "b": 0.5}}),
           ("mitchell b=nan", {"flt": {"kind": 3, "a": 0.5, "b": math.nan}})]]
CASCADE = [[("layers=1", {"cs": {"layers": 1}}), ("layers=9", {"cs": {"layers": 9}})],
           [("start=0", {"cs": {"start": 0.0}}), ("start=nan", {"cs": {"start": math.nan}}), ("start=inf", {"cs": {"start": math.inf}})],
           [("base=1.5", {"cs": {"base": 1.5}}), ("base=nan", {"cs": {"base": math.nan}})],
           [("kappa=-1", {"cs": {"kappa": -1.0}}), ("kappa=inf", {"cs": {"kappa": math.inf}})]]
# (the level table cannot overflow within 8 layers of f32 parameters -- FLT_MAX^8 is a finite double --: that answer is out of reach)
TONEMAP = [[("mode=7", {"tm": {"mode": 7}})], [("curve=7", {"tm": {"curve": 7}})], [("transfer=7", {"tm": {"transfer": 7}})],
           [("ev=nan", {"tm": {"ev": math.nan}}), ("ev=inf", {"tm": {"ev": math.inf}})],
           [("pct_lo=-0.1", {"tm": {"pct_lo": -0.1}}), ("pct_hi=1.5", {"tm": {"pct_hi": 1.5}}), ("pct_lo>pct_hi", {"tm": {"pct_lo": 0.9, "pct_hi": 0.5}}),
            ("pct_lo=nan", {"tm": {"pct_lo": math.nan}})],
           [("key=0", {"tm": {"key": 0.0}}), ("white=inf", {"tm": {"white": math.inf}}), ("key=nan", {"tm": {"key": math.nan}})],
           [("adapt=1.5", {"tm": {"adapt": 1.5}}), ("adapt=nan", {"tm": {"adapt": math.nan}})],
           [("log2_min=9", {"tm": {"log2_min": 9.0}}), ("log2_max=nan", {"tm": {"log2_max": math.nan}})]]
BLOOM_RULE = [[("levels=0", {"bl": {"levels": 0}}), ("levels=9", {"bl": {"levels": 9}})],
              floats("bl", "threshold"), floats("bl", "knee"),
              [("clamp=0", {"bl": {"clamp": 0.0}}), ("clamp=nan", {"bl": {"clamp": math.nan}})],
              [("scatter=1.5", {"bl": {"scatter": 1.5}}), ("scatter=nan", {"bl": {"scatter": math.nan}})],
              floats("bl", "intensity")]
UPSAMPLE = [[(f"upsample {t}", o) for t, o in floats("up", "sigma_n") + floats("up", "sigma_d", BAD_F[2:])]]
_degenerate = [("horizontal=0", {"cam": {"horizontal": (0.0, 0.0, 0.0)}}), ("vertical=nan", {"cam": {"vertical": (math.nan, 0.0, 0.0)}}),
               ("origin=inf", {"cam": {"origin": (math.inf, 0.0, 2.0)}})]
LENS = [[("aperture=-1", {"lens": {"aperture": -1.0}}), ("aperture=nan", {"lens": {"aperture": math.nan}})],
        [("focus_distance=0", {"lens": {"focus_distance": 0.0}}), ("focus_distance=inf", {"lens": {"focus_distance": math.inf}})],
        _degenerate]
PROJ = [[("kind=4", {"proj": {"kind": 4}})], [("reserved=1", {"proj": {"reserved": 1}})],
        [("fisheye fov=0", {"proj": {"kind": 2, "fov_degrees": 0.0}}), ("fisheye fov=400", {"proj": {"kind": 2, "fov_degrees": 400.0}}),
         ("fisheye fov=nan", {"proj": {"kind": 2, "fov_degrees": math.nan}})],
        _degenerate]
CAMERA_SIZE = [(f"camera {w}x{h}", {"cam": {"width": w, "height": h}}) for w, h in ((1, 8), (8, 1))]
GRID = [[("null g", {"g": None}), ("counts=0", {"g": {"counts": (0, 1, 1)}}), ("65536 probes", {"g": {"counts": (256, 256, 1)}}), ("spacing=0", {"g": {"spacing": (0.0, 1.0, 1.0)}}),
         ("origin=nan", {"g": {"origin": (math.nan, 0.0, 0.0)}})]]     # (one check: a null grid counts as invalid)


# the planes of the filter (wsum: its weight sums too) and the cascade: aligned, then no output on the samples, then no output
# on another output.  device: a null context refuses what the checks let through (ranges that only touch)
def _film_planes(wsum, device):
    align = [("samples % 4", {"samples": ODD}), ("lin % 4", {"lin": ODD}), ("rgba % 4", {"rgba": ODD}), ("plain % 4", {"plain": ODD})]
    on_samples = [("lin on the samples' last word", {"lin": at(SAMPLES_END - 4)}), ("rgba inside the samples", {"rgba": at(512)}),
                  ("the samples' first word on plain's last", {"samples": at(3584 + 768 - 4), "lin": at(8192), "rgba": at(9216)})]
    on_outputs = [("rgba on lin's last word", {"rgba": at(LIN_END - 4)}), ("plain = lin", {"plain": LIN}),
                  ("lin on plain, rgba on the samples", {"lin": at(3584 + 4), "rgba": at(4)})]
    if wsum:
        align.append(("wsum % 8", {"wsum": ODD8}))
        on_outputs.append(("wsum on plain's last word", {"wsum": at(3584 + 768 - 8)}))
    if device:
        on_samples.append(("lin touches the samples' end, null context", {"lin": at(SAMPLES_END), "c": None}))
        on_outputs.append(("rgba touches lin's end, null context", {"rgba": at(LIN_END), "c": None}))
    return [align, on_samples, on_outputs]


def _samples(rule, arg, wsum, device):
    return ([nulls("samples", arg, "lin")] + rule + _size(False) + [N0] + _film_planes(wsum, device) + ([NO_CONTEXT] if device else []))


def _render_film(rule, arg, *more):
    return [nulls("c", "cam", "prm", arg, "lin")] + rule + list(more) + _size(True) + [BAND, SPP]


_texels = [[("lightmap 0x8", {"width": 0}), ("lightmap 8x0", {"height": 0})],
           [("lightmap 65536x8", {"width": 65536}), ("lightmap 8x65536", {"height": 65536})]]
_probes = [[("n_probes=0", {"n_probes": 0})], [("rays_per_probe=0", {"rays": 0})],
           [("65536 probes", {"n_probes": 65536}), ("65536 rays", {"rays": 65536})]]
# (a band_index above 0 is not refused by the bakes' whole-image check: the null plane behind it answers)
_bake_band = [("band_count=2", {"prm": {"band_rows": 2, "band_count": 2}})]


def _lightmap(odd_in):
    return ([nulls("c", "prm")] + _texels + [_bake_band, _plane("tex", odd_in) + [("band_index=1, null tex", {"prm": {"band_index": 1}, "tex": None})],
                                              _plane("lin") + [("tex % 8, null lin", {"tex": ODD8, "lin": None})], _plane("rgba", null=False)])


def _bake_probes():
    return ([nulls("c", "prm")] + _probes + [_bake_band, _plane("pos") + [("band_index=1, null pos", {"prm": {"band_index": 1}, "pos": None})],
                                             _plane("rad"), _plane("sh27", null=False)])


_bake_film = [[("kind=2", {"kind": 2})],
              _texels[0] + [("probes: n_probes=0", {"kind": 1, "height": 0}), ("probes: rays_per_probe=0", {"kind": 1, "width": 0})],
              _texels[1] + [("probes: 65536 probes", {"kind": 1, "height": 65536})]]
_outside = [("x=8", {"xys": xys(8, 0)}), ("y=8", {"xys": xys(0, 8)})]


def _shade(feat_odd, context, own_features=False):
    feat = [] if own_features else [_plane("feat", feat_odd) + [("feat % 16, null lin", {"feat": ODD16, "lin": None})]]
    return ([nulls("c", "prm")] if own_features else []) + [nulls("cam", "sp")] + GRID + [
        [("weight=2", {"sp": {"weight": 2}})], floats("sp", "normal_bias", BAD_F[1:]),
        [("image 0x8", {"cam": {"width": 0}}), ("image 8x0", {"cam": {"height": 0}})], _huge(True), _plane("sh27")] + feat + [
        _plane("fallback", null=False), _plane("lin"), _plane("rgba", null=False)] + ([NO_CONTEXT] if context else [])


_tone_film = [[("null lin", {"lin": None})], [("lin % 4", {"lin": ODD})]] + _size(False)
_tone_outs = [("out % 4", {"out": ODD}), ("rgba % 4", {"rgba": ODD})]
_bloom_film = [[("lin % 4", {"lin": ODD})], _small(False), _huge(False)]


def _upsample_planes(context):
    return [nulls("lo_lin", "lo_feat", "feat", "up", "lin"),
            [("lo_feat % 16", {"lo_feat": ODD16}), ("feat % 16", {"feat": ODD16})],
            [("lo_lin % 4", {"lo_lin": ODD}), ("lin % 4", {"lin": ODD}), ("rgba % 4", {"rgba": ODD})],
            [("lo_width=1", {"lo_width": 1}), ("lo_height=1", {"lo_height": 1}), ("width=1", {"width": 1, "lo_width": 1}), ("height=0", {"height": 0})],
            [("lo_width=9", {"lo_width": 9}), ("lo_height=9", {"lo_height": 9})], _huge(False),
            [("lin = lo_lin", {"lin": SAMPLES}), ("lin = feat", {"lin": at(6144)}), ("rgba = lo_feat", {"rgba": FEAT})]] + UPSAMPLE + (
                [NO_CONTEXT] if context else [])


_features = [N0]        # pt_render_features_*: behind the nulls, in front of the lens or the projection
_features_tail = [BAND, [("feat % 16", {"feat": ODD16})], [("accel=3", {"prm": {"accel": 3}})]]
_rays_nulls = nulls("xys", "out", "cam")
ENTRIES = {
    "pt_debug_filter_weight": [nulls("f", "flt")] + FILTER,
    "pt_debug_filter_offsets": [nulls("ox", "oy")],
    "pt_debug_filter_exp_neg": [[("null out", {"out": None}), ("e=-1", {"e": -1.0}), ("e=101", {"e": 101.0}), ("e=nan", {"e": math.nan})]],
    "pt_filter_host": _samples(FILTER, "flt", True, False),
    "pt_filter_samples_device": _samples(FILTER, "flt", True, True),
    "pt_render_filtered_device": _render_film(FILTER, "flt"),
    "pt_render_filtered_host": _render_film(FILTER, "flt"),
    "pt_debug_cascade_split": [nulls("j", "cs", "w_lo", "w_hi")] + CASCADE,
    "pt_cascade_host": _samples(CASCADE, "cs", False, False),
    "pt_cascade_samples_device": _samples(CASCADE, "cs", False, True),
    "pt_render_cascade_device": _render_film(CASCADE, "cs"),
    "pt_render_cascade_host": _render_film(CASCADE, "cs"),
    "pt_bake_lightmap_device": _lightmap(ODD8),
    "pt_bake_lightmap_host": _lightmap(ODD),
    "pt_bake_probes_device": _bake_probes(),
    "pt_bake_probes_host": _bake_probes(),
    "pt_sh_project_device": [NO_CONTEXT] + _probes + [_plane("rad"), _plane("sh27")],
    "pt_sh_project_host": _probes + [_plane("rad"), _plane("sh27")],
    "pt_sh_irradiance_host": [nulls("sh27", "normals", "out")],
    "pt_bake_rays_host": _bake_film + [nulls("data", "xys", "out"), _outside],
    "pt_debug_bake_rays": _bake_film + [nulls("c", "data", "xys", "out"), _outside],
    "pt_probe_grid_positions_host": GRID + [_plane("out")],
    "pt_probe_grid_bake_device": [nulls("c", "prm")] + GRID + [[("rays_per_probe=0", {"rays": 0}), ("rays_per_probe=65536", {"rays": 65536})],
                                                                _plane("sh27"), _bake_band],
    "pt_probe_shade_device": _shade(ODD16, True),
    "pt_probe_shade_host": _shade(ODD, False),
    "pt_render_probe_lit_device": _shade(None, False, own_features=True),
    "pt_render_probe_lit_host": _shade(None, False, own_features=True),
    "pt_debug_probe_positions": GRID + [_plane("out"), NO_CONTEXT],
    "pt_film_histogram_device": [nulls("hist")] + _tone_film + [[("hist % 4", {"hist": ODD})], NO_CONTEXT],
    "pt_tonemap_device": [nulls("tm", "rgba")] + _tone_film + [_tone_outs] + TONEMAP + [NO_CONTEXT],
    "pt_tonemap_host": [nulls("tm", "rgba")] + _tone_film + TONEMAP + [NO_CONTEXT],
    "pt_exposure_reset": [NO_CONTEXT],
    "pt_debug_exposure_state": [NO_CONTEXT],
    "pt_exposure_get": [nulls("c", "log2E")],
    "pt_debug_tonemap_pixel": [nulls("rgb", "tm", "y", "rgba")] + TONEMAP,
    "pt_bloom_device": [nulls("bl", "lin", "out"), [("lin % 4", {"lin": ODD}), ("out % 4", {"out": ODD})]] + _bloom_film[1:] + BLOOM_RULE + [NO_CONTEXT],
    # without a bloom the display entries are the tone mapping's, and pt_display_device answers in its name
    "pt_display_device": [nulls("lin")] + _bloom_film + BLOOM_RULE + [nulls("tm", "rgba"), _tone_outs] + TONEMAP + [
        NO_CONTEXT, [("no bloom: null tm", {"bl": None, "tm": None}), ("no bloom: null context", {"bl": None, "c": None})]],
    "pt_display_host": [nulls("lin")] + _bloom_film + BLOOM_RULE + [nulls("tm", "rgba"), _tone_outs] + TONEMAP + [
        NO_CONTEXT, [("no bloom: 2^31 pixels", dict(HUGE, bl=None)), ("no bloom: null lin", {"bl": None, "lin": None})]],
    "pt_bloom_host": [nulls("bl", "lin", "out"), [("lin % 4", {"lin": ODD}), ("out % 4", {"out": ODD})]] + _bloom_film[1:] + BLOOM_RULE,
    "pt_debug_bloom_plan": [nulls("wh", "n_levels", "first_tail"),
                            [("width=1", {"width": 1}), ("height=1", {"height": 1}), ("2^31 pixels", dict(HUGE)), ("levels=0", {"levels": 0}),
                             ("levels=9", {"levels": 9})]],
    "pt_debug_bloom_bright": [nulls("bl", "lin", "out"), [("lin % 4", {"lin": ODD}), ("out % 4", {"out": ODD})]] + BLOOM_RULE,
    "pt_debug_bloom_tail": [NO_CONTEXT],
    "pt_upsample_device": _upsample_planes(True),
    "pt_upsample_host": _upsample_planes(False),
    "pt_render_denoised_upsampled": [nulls("c", "cam", "prm", "dn", "up", "lin"),
                                     [("lo_width=1", {"lo_width": 1}), ("camera 1x8", {"cam": {"width": 1}, "lo_width": 1})],
                                     [("lo_width=9", {"lo_width": 9})], _huge(True)] + UPSAMPLE + [BAND, FS] + DENOISE,
    "pt_render_projection_device": [nulls("c", "cam", "proj", "prm")] + PROJ,
    "pt_render_projection_host": [nulls("c", "cam", "proj", "prm", "lin")] + PROJ,
    "pt_render_features_projection_device": [nulls("proj", "c", "cam", "prm", "feat")] + _features + PROJ + _features_tail,
    "pt_render_projection_denoised": [nulls("c", "proj", "cam", "prm", "dn", "lin")] + PROJ + [BAND, FS],
    "pt_render_rays_device": [nulls("c", "prm", "rays6"), [("rays6 % 8", {"rays6": ODD8})], [("weights3 % 4", {"weights3": ODD})]],
    "pt_projection_setup_host": [nulls("cam", "proj", "out")] + PROJ,
    "pt_projection_rays_host": [_rays_nulls + nulls("proj")] + PROJ + [CAMERA_SIZE],
    "pt_debug_projection_rays": [nulls("c", "proj") + _rays_nulls] + PROJ + [CAMERA_SIZE],
    "pt_render_features_lens_device": [nulls("lens", "c", "cam", "prm", "feat")] + _features + LENS + _features_tail,
    "pt_render_lens_denoised": [nulls("c", "lens", "cam", "prm", "dn", "lin")] + LENS + [BAND, FS],
    "pt_debug_lens_setup": [nulls("cam", "lens", "out")] + LENS,
    "pt_debug_lens_rays": [nulls("c", "lens") + _rays_nulls] + LENS + [CAMERA_SIZE],
    "pt_render_lens_device": [nulls("c", "cam", "lens", "prm")] + LENS,
    "pt_render_lens_host": [nulls("c", "cam", "lens", "prm", "lin")] + LENS,
}
# the entries of a file that the table covers: all that return a code, but for pt_api.cpp (its two lens renders; the other
# entries there make no check of their own in front of render_impl's, which read the context)
FILES = {"pt_filter.cpp": None, "pt_cascade.cpp": None, "pt_bake.cpp": None, "pt_probe_grid.cpp": None, "pt_tonemap.cpp": None, "pt_bloom.cpp": None,
         "pt_upsample.cpp": None, "pt_projection.cpp": None, "pt_lens.cpp": None, "pt_api.cpp": r"pt_render_lens_\w+"}


def cases(entry):
    """-> [(label, overrides)]: every case of every step, then the pair of each step with the next"""
    return _cases(ENTRIES[entry])


def call(pt, entry, overrides):
    """-> [return code, message]"""
    return _call(pt, entry, merge(GOOD[entry], overrides), STRUCTS, _struct)


def _entries_of(name):
    src = open(os.path.join(ROOT, "pathtrace_amd", "csrc", name)).read()
    found = []
    for block in src.split('extern "C" {')[1:]:
        found += re.findall(r"^int (pt_\w+)\(", block[:block.index('}  // extern "C"')], re.M)
    return {e for e in found if FILES[name] is None or re.fullmatch(FILES[name], e)}


@pytest.mark.parametrize("name", sorted(FILES))
def test_every_entry_of_the_file_is_covered(name):
    """The extern "C" functions of the file that return a code (the pt_default_* return nothing and ignore a null)."""
    mine = _entries_of(name)
    assert mine and mine <= set(ENTRIES), sorted(mine - set(ENTRIES))


def test_the_table_covers_nothing_else():
    assert set().union(*(_entries_of(n) for n in FILES)) == set(ENTRIES) == set(GOOD)


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_refusals_are_those_of_the_recorded_commit(pt, entry):
    table = table_of(TABLE, entry)
    mine = cases(entry)
    assert sorted(t for t, _ in mine) == sorted(table) and len(mine) == len(table), "the cases are not the recorded ones"
    for label, overrides in mine:
        assert call(pt, entry, overrides) == table[label], (entry, label)


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit(__doc__)
    sys.path.insert(0, ROOT)
    import pathtrace_amd
    record(TABLE, ENTRIES, cases, lambda e, o: call(pathtrace_amd, e, o))
