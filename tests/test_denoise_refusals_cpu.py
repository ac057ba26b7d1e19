"""The refusals of pathtrace_amd/csrc/pt_denoise.cpp that need no device, pinned: for every extern "C" entry of that file, every
check it makes before it first reads the context -- each alone, each pair of checks that follow one another (the pair pins
their order: the earlier one answers), and the null context -- against the (return code, pt_last_error() text) that commit
6aa9e05 gave, in tests/golden/denoise_refusals.json: per entry one line per answer, [code, message, the cases that get it], with
{who} for the entry's own name.

The table is a record of that commit, not of the code under test.  It was written by

    git checkout 6aa9e05 && python -c "import __graft_entry__ as g; g.build()" && python tests/test_denoise_refusals_cpu.py --record

with this file copied into that checkout, and is only ever recorded again from a commit whose refusals are meant to be the
new truth.  ENTRIES below restates that commit's order of checks, entry by entry; the context is a pointer that is never
followed (a case that reached the context would read the zeroed scratch behind it, not a PtContext).
"""
import math
import os
import sys

import pytest

from refusal_cases import BAD_F, HUGE, at, merge, call as _call, cases as _cases, floats as _floats, nulls as _nulls, record, table_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "golden", "denoise_refusals.json")
STRUCTS = ("cam", "prev_cam", "prm", "dn", "tp", "g", "ad")

OK, ODD4, ODD16, OUT, FAKE = (at(k) for k in (0, 2, 4, 2048, 4096))

# ---------------------------------------------------------------- the arguments of a call that passes every check
_frame = dict(c=FAKE, cam={}, prm={}, fs=2, dn={})
_film = dict(lin=OK, feat=OK)
_outs = dict(out=OUT, rgba=None)
GOOD = {
    "pt_render_features_device": dict(c=FAKE, cam={}, prm={}, n=2, feat=OK),
    "pt_render_feature_ids_device": dict(c=FAKE, cam={}, prm={}, ids=OK),
    "pt_denoise_device": dict(c=FAKE, width=8, height=8, **_film, dn={}, **_outs),
    "pt_denoise_var_device": dict(c=FAKE, width=8, height=8, **_film, var=OK, dn={}, **_outs),
    "pt_adaptive_variance_device": dict(c=FAKE, width=8, height=8, feat=OK, var=OUT),
    "pt_render_adaptive_denoised": dict(c=FAKE, cam={}, prm={}, ad={}, fs=2, dn={}, out=OUT, o1=None, o2=None, o3=None, o4=None, o5=None),
    "pt_render_denoised": dict(**_frame, out=OUT, o1=None, o2=None, o3=None),
    "pt_temporal_reset": dict(c=FAKE),
    "pt_denoise_temporal_device": dict(c=FAKE, cam={}, **_film, dn={}, tp={}, **_outs),
    "pt_denoise_temporal_motion_device": dict(c=FAKE, cam={}, **_film, ids=OK, dn={}, tp={}, **_outs),
    "pt_denoise_temporal_alpha_device": dict(c=FAKE, cam={}, **_film, ids=OK, alpha=OK, dn={}, tp={}, **_outs),
    "pt_render_denoised_temporal": dict(**_frame, tp={}, out=OUT, o1=None, o2=None, o3=None),
    "pt_render_denoised_motion": dict(**_frame, tp={}, out=OUT, o1=None, o2=None, o3=None, o4=None),
    "pt_temporal_gradient_device": dict(c=FAKE, cam={}, prm={}, seed=0, prev=OK, g={}, alpha_min=0.2, alpha=OUT),
    "pt_temporal_gradient_camera_device": dict(c=FAKE, cam={}, prev_cam={}, prm={}, seed=0, prev=OK, feat=OK, g={}, alpha_min=0.2, alpha=OUT),
    "pt_debug_gradient_strata": dict(c=FAKE, width=8, height=8, o1=None, o2=None, o3=None),
    "pt_render_denoised_gradient": dict(**_frame, tp={}, g={}, out=OUT, o1=None, o2=None, o3=None, o4=None, o5=None),
    "pt_render_denoised_gradient_camera": dict(**_frame, tp={}, g={}, out=OUT, o1=None, o2=None, o3=None, o4=None, o5=None),
}


# ---------------------------------------------------------------- the checks, in the order 6aa9e05 makes them
# A step is one check: a list of (label, the arguments that trip it).  Every entry of the list is a case of its own; the
# first stands for the step in the pair with the step after it.  A dict as the value of a struct argument names the fields
# that differ from the defaults.  (The machinery: refusal_cases.py.)
BAND = [("band_count=2", {"prm": {"band_rows": 2, "band_count": 2}}), ("band_index=1", {"prm": {"band_index": 1}})]
SMALL = [(f"camera {w}x{h}", {"cam": {"width": w, "height": h}}) for w, h in ((1, 8), (8, 1), (0, 0))]
DENOISE = [[("iterations=17", {"dn": {"iterations": 17}})],
           _floats("dn", "sigma_l") + _floats("dn", "sigma_n", BAD_F[:1]) + _floats("dn", "sigma_d", BAD_F[1:2])]
ALPHA = [("alpha=1.5", {"tp": {"alpha": 1.5}}), ("alpha=-0.1", {"tp": {"alpha": -0.1}}), ("alpha=nan", {"tp": {"alpha": math.nan}})]
TEMPORAL = [ALPHA, _floats("tp", "depth_tol") + _floats("tp", "normal_tol", BAD_F[2:])]
GRADIENT = [[("radius=9", {"g": {"radius": 9}})], _floats("g", "scale")]
FEAT16 = [("d_features % 16", {"feat": ODD16})]
FILM4 = [("d_out_rgba % 4", {"rgba": ODD4}), ("d_linear % 4", {"lin": ODD4}), ("d_out_linear % 4", {"out": ODD4})]
SAME = [("output = input", {"lin": OK, "out": OK})]
FS = [("feature_samples=0", {"fs": 0})]
NO_CONTEXT = [("null context", {"c": None})]


def _filter(var):
    return ([_nulls("c", "dn", "lin", "feat", "out") + (_nulls("var") if var else []),
             [("image 0x8", {"width": 0}), ("image 8x0", {"height": 0})]] + DENOISE + [FEAT16, FILM4] +
            ([[("d_var % 4", {"var": ODD4})]] if var else []) + [SAME, [("2^31 pixels", dict(HUGE))]])


def _temporal(*planes):
    return ([_nulls("dn", "cam", "tp", "lin", "feat", "out", *planes), SMALL] + DENOISE + TEMPORAL +
            [FEAT16, FILM4, SAME, [("2^31 pixels", {"cam": HUGE})]] + [[(f"d_{p} % 4", {p: ODD4})] for p in planes] + [NO_CONTEXT])


def _gradient(camera):
    both = {"cam": HUGE, "prev_cam": HUGE} if camera else {"cam": HUGE}
    small = [(t, dict(a, prev_cam=a["cam"]) if camera else a) for t, a in SMALL]
    return ([_nulls("cam", "prm", "prev", "g", "alpha", *(("prev_cam", "feat") if camera else ())),
             [("d_prev_linear % 4", {"prev": ODD4}), ("d_alpha % 4", {"alpha": ODD4})]] +
            ([FEAT16, [("previous camera 8x9", {"prev_cam": {"height": 9}}), ("previous camera 9x8", {"prev_cam": {"width": 9}})]] if camera else []) +
            [BAND] + GRADIENT +
            [[(f"alpha_min={t}", {"alpha_min": v}) for t, v in (("2", 2.0), ("-0.1", -0.1), ("nan", math.nan))], small,
             [("spp=0", {"prm": {"spp": 0}})], [("integrator=2", {"prm": {"integrator": 2}})], [("accel=3", {"prm": {"accel": 3}})],
             [("2^31 pixels", both)], NO_CONTEXT])


_frame_nulls = ("c", "cam", "prm", "dn", "out")
ENTRIES = {
    "pt_render_features_device": [_nulls("feat", "c", "cam", "prm"), [("n_samples=0", {"n": 0})], BAND, FEAT16, [("accel=3", {"prm": {"accel": 3}})]],
    "pt_render_feature_ids_device": [_nulls("ids", "c", "cam", "prm"), BAND, [("d_ids % 4", {"ids": ODD4})], [("accel=3", {"prm": {"accel": 3}})]],
    "pt_denoise_device": _filter(False),
    "pt_denoise_var_device": _filter(True),
    "pt_adaptive_variance_device": [_nulls("c", "feat", "var"), FEAT16, [("d_var % 4", {"var": ODD4})]],
    "pt_render_adaptive_denoised": [_nulls("c", "cam", "prm", "ad", "dn", "out"), FS],
    "pt_render_denoised": [_nulls(*_frame_nulls), BAND, FS],
    "pt_temporal_reset": [NO_CONTEXT],
    "pt_denoise_temporal_device": _temporal(),
    "pt_denoise_temporal_motion_device": _temporal("ids"),
    "pt_denoise_temporal_alpha_device": _temporal("ids", "alpha"),
    "pt_render_denoised_temporal": [_nulls(*_frame_nulls, "tp"), BAND, FS],
    "pt_render_denoised_motion": [_nulls(*_frame_nulls, "tp"), BAND, FS],
    "pt_temporal_gradient_device": _gradient(False),
    "pt_temporal_gradient_camera_device": _gradient(True),
    "pt_debug_gradient_strata": [NO_CONTEXT],
    "pt_render_denoised_gradient": [_nulls(*_frame_nulls, "tp", "g"), BAND, FS] + GRADIENT + [ALPHA],
    "pt_render_denoised_gradient_camera": [_nulls(*_frame_nulls, "tp", "g"), BAND, FS] + GRADIENT + [ALPHA],
}


def cases(entry):
    """-> [(label, overrides)]: every case of every step, then the pair of each step with the next"""
    return _cases(ENTRIES[entry])


def _struct(pt, name, fields):
    if name in ("cam", "prev_cam"):
        s = pt.camera_new(width=8, height=8)
    elif name == "ad":
        s = pt._lib.PtAdaptive(4, 4, 0.1, 1e-3)
    else:
        s = {"prm": lambda: pt.default_params(spp=2), "dn": pt.default_denoise, "tp": pt.default_temporal, "g": pt.default_gradient}[name]()
    for k, v in fields.items():
        setattr(s, k, v)
    return s


def call(pt, entry, overrides):
    """-> [return code, message]"""
    return _call(pt, entry, merge(GOOD[entry], overrides), STRUCTS, _struct)


def test_every_entry_of_the_file_is_covered():
    """The extern "C" functions of pt_denoise.cpp that return a code (pt_default_gradient returns nothing and ignores a null)."""
    import re
    src = open(os.path.join(ROOT, "pathtrace_amd", "csrc", "pt_denoise.cpp")).read()
    block = src[src.index('extern "C" {'):]
    assert set(re.findall(r"^int (pt_\w+)\(", block, re.M)) == set(ENTRIES) == set(GOOD)


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
