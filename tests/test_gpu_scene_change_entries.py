"""Every ray entry of a context after the scene under it changed (tests/scene_change_cases.py) against a fresh context's linear
scan of the new scene: a film is a function of the scene, the camera and the parameters -- not of the tree the context held, of the
class of the scene it ran before, or of what an entry sized and cached for the old one.

Context A: upload(S0), the entry once (discarded), the transition, the entry (got), a plain render.  Context B, fresh: upload(S1),
the entry with accel = 0 (want), a plain render.  got is want and the renders are one another, bit for bit, NaN equal to NaN.
B's results are computed once per (entry, scene) and never changed."""
import time

import numpy as np
import pytest

import scene_change_cases as cc

pytestmark = pytest.mark.gpu
_T0 = time.perf_counter()


def _fresh(pt, key, fn):
    ctx = pt.Context(0)
    try:
        ctx.upload(cc.scene(pt, key))
        return fn(ctx)
    finally:
        ctx.close()


def _plain(pt, ctx, fam, accel):
    return cc.run_entry(pt, ctx, cc.ENTRY["frame"], fam, accel)


@pytest.fixture(scope="module")
def want(pt):
    """(entry name, scene key) -> the entry's outputs on a fresh context of that scene under the linear scan"""
    held = {}

    def get(name, key):
        if (name, key) not in held:
            held[(name, key)] = _fresh(pt, key, lambda ctx: cc.run_entry(pt, ctx, cc.ENTRY[name], cc.family(key), 0))
        return held[(name, key)]

    yield get
    print(f"\nscene change: {len(held)} fresh references, {len(cc.cases())} cases, {time.perf_counter() - _T0:.1f} s since import")


def _describe(diffs):
    return ", ".join(f"plane {i}: {n}" + (" words" if isinstance(n, int) else "") for i, n in diffs)


# ---- conditions on the inputs
@pytest.mark.parametrize("key", cc.SCENE_KEYS)
def test_traversal_order_cannot_show_on_these_scenes(pt, key):
    """fresh, scan against tree: a plain render and debug_hit_scene"""
    for name in ("frame", "hit_scene", "hit_scene_exact"):
        a, b = (_fresh(pt, key, lambda ctx: cc.run_entry(pt, ctx, cc.ENTRY[name], cc.family(key), accel)) for accel in (0, 1))
        assert not cc.differences(a, b), f"{name} on {key}: {_describe(cc.differences(a, b))}"


@pytest.mark.parametrize("name", cc.CLASS_EDITS)
def test_a_class_change_moves_the_dispatch(pt, name):
    def log(key):
        def run(ctx):
            ctx.launch_log()
            _plain(pt, ctx, "box", 0)
            return ctx.launch_log()
        return _fresh(pt, key, run)

    a, b = log("box0"), log("box_" + name)
    assert a and b and (set(a) != set(b)) == (name in cc.DISPATCH_MOVES), (a, b)


def test_the_adaptive_pixels_do_not_all_stop_together(pt, want):
    for key in ("cloud1", "box1"):
        spp = want("adaptive", key)[2]
        assert spp.min() == 2 and spp.max() == 6 and len(np.unique(spp)) == 3, (key, np.unique(spp, return_counts=True))


@pytest.mark.parametrize("entry", [e.name for e in cc.ENTRIES])
def test_every_transition_changes_the_entrys_output(pt, want, entry):
    """want on the transition's final scene differs from want on its start (the refusals: they are the same scene); an entry that
    reads nothing of the scene gives the same on all, one that reads only shapes the same across a class change"""
    for t in cc.TRANSITIONS:
        if t.kind == "refused" or not any(c[0] == entry and c[1] == t.name for c in cc.cases()):
            continue
        a, b = want(entry, t.start), want(entry, t.final)
        diffs, reads = cc.differences(a, b), cc.ENTRY[entry].reads
        if reads == "nothing" or (reads == "shapes" and t.kind == "class"):
            assert not diffs, (t.name, diffs)
        else:
            assert diffs, (f"{t.name} ({t.start} -> {t.final}) does not change {entry}; planes (shape, non-zero words): "
                           f"{[(x.shape, int(np.count_nonzero(cc.as_bits(x)))) for x in a]}")


# ---- the property
def _run_case(pt, want, name, tname, accel):
    entry, t = cc.ENTRY[name], cc.TRANSITION[tname]
    fam = cc.family(t.start)
    ctx = pt.Context(0)
    try:
        ctx.upload(cc.scene(pt, t.start))
        cc.run_entry(pt, ctx, entry, fam, accel)
        for op, key in t.steps:
            cc.apply_step(pt, ctx, op, cc.scene(pt, key))
        got = cc.run_entry(pt, ctx, entry, fam, accel)
        uses_tree = name not in ("camera_rays",)
        if accel and uses_tree:
            refits = ctx.bvh_cost()[2]                            # (raises without a tree)
            ops = [op for op, _ in t.steps]
            assert refits == (ops.count("refit") if ops[-1] == "refit" else 0), (ops, refits)
        elif any(op in ("morton", "median") for op, _ in t.steps):
            assert ctx.bvh_cost()[2] == 0
        plain = _plain(pt, ctx, fam, accel)
    finally:
        ctx.close()
    diffs = cc.differences(got, want(name, t.final))
    assert not diffs, f"{name} after {tname} (accel {accel}) differs from a fresh context's scan of {t.final}: {_describe(diffs)}"
    diffs = cc.differences(plain, want("frame", t.final))
    assert not diffs, f"the plain render after {name} after {tname} (accel {accel}) differs from a fresh context's: {_describe(diffs)}"


def _ids(group):
    return [pytest.param(*c, id=f"{c[0]}-{c[1]}-accel{c[2]}") for c in cc.cases() if cc.ENTRY[c[0]].group == group]


@pytest.mark.parametrize("name, tname, accel", _ids("paths"))
def test_path_entries_through_injected_rays(pt, want, name, tname, accel):
    _run_case(pt, want, name, tname, accel)


@pytest.mark.parametrize("name, tname, accel", _ids("features"))
def test_feature_ray_entries(pt, want, name, tname, accel):
    _run_case(pt, want, name, tname, accel)


@pytest.mark.parametrize("name, tname, accel", _ids("film"))
def test_pixel_list_and_film_entries(pt, want, name, tname, accel):
    _run_case(pt, want, name, tname, accel)


@pytest.mark.parametrize("name, tname, accel", _ids("debug"))
def test_debug_ray_entries(pt, want, name, tname, accel):
    _run_case(pt, want, name, tname, accel)
