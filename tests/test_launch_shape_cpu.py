"""The launch sizing of a render without a GPU.

render_impl (csrc/pt_api.cpp) sizes a render -- level-0 form, batches, grids, queue segments, hand-over queue, the job the
scheduler plans, the per-launch words -- with the pure functions of csrc/pt_shape.h; pt_debug_render_shape runs the same
functions on the caller's numbers.  Here they are held, field by field, to the plain-Python restatement of
tests/launch_shape_ref.py (written from the driver's text before the arithmetic moved) over a grid of cases that crosses every
branch and boundary; a sample of the jobs goes on through the planner (pt_debug_sched_render), and every planned launch must
fit what was sized: n_first <= waves * seg_cap inside the queue allocated, ovf_slots <= nw_cont * seg_cap_cont.  The grids of
the jobs recorded on an MI355X (tests/golden/launch_counts.json) come out of the same two calls."""
import ctypes as C
import json
import os

import pytest

import bench
import pathtrace_amd as pt
from pathtrace_amd._lib import PtSchedJob, PtSchedOp, PtShapeIn, PtShapeLaunch, PtShapeOut
from tests import launch_shape_jobs as J
from tests import launch_shape_ref as R
from tests.test_sched_cpu import Sched

OP_LAUNCH = 6
PRIME = 65521
OUT_FIELDS = ("lds_job", "split", "regen_scene", "over_cap", "cap", "n_paths_max", "ovf_slots", "q_slots_cont", "q_slots", "np", "spp", "nb_max",
              "n_batches", "export_small", "paths_per_wave", "small_scene", "hand_off", "regen", "overlap", "grid", "nw", "seg_cap",
              "regen_per_cu", "regen_capacity", "regen_grid", "regen_launch_grid", "cont_grid", "nw_cont", "seg_cap_cont", "regen_export")
LAUNCH_FIELDS = ("s0", "nb", "n_first", "seg_cap", "src_mode", "export_below", "regen_static")


def _job_fields():
    return [n for n, _ in PtSchedJob._fields_]


def device_shape(i, occupancy, ops=None):
    """pt_debug_render_shape -> (rc, PtShapeOut, [PtShapeLaunch per op])"""
    cin = PtShapeIn(**i)
    out = PtShapeOut()
    n = len(ops) if ops else 0
    arr = (PtSchedOp * max(n, 1))(*(ops or []))
    ls = (PtShapeLaunch * max(n, 1))()
    rc = pt._lib.lib().pt_debug_render_shape(C.byref(cin), occupancy, C.byref(out), arr if n else None, n, ls if n else None)
    return rc, out, list(ls)[:n]


def cases():
    """(inputs, occupancy) over every branch and boundary of the sizing."""
    mk, out = R.make_in, []
    for n in (1, 2, 63, 64, 65, PRIME):                                   # tile sizes; one sample and several
        for spp in (1, 7):
            out.append((mk(np=n, spp=spp), 0))
    for n, spp in ((1 << 16, 2), (1 << 16, 3), (1 << 17, 1), ((1 << 17) + 1, 1),        # kRegenMinPaths
                   (1 << 20, 4), (1 << 20, 5), (1 << 22, 1), ((1 << 22) + 1, 1)):       # kExportMinPaths
        for form in (0, 1):
            out.append((mk(np=n, spp=spp, level0_form=form), 0))
        out.append((mk(np=n, spp=spp, n_objs=129, blob_f4=0), 0))
    for form in (0, 1):                                                   # np == cap, cap + 1 (refused): default caps and a given one
        cap = 1 << (28 if form == 0 else 26)
        out += [(mk(np=cap, spp=2, level0_form=form), 0), (mk(np=cap + 1, spp=2, level0_form=form), 0)]
    out += [(mk(np=1000, max_paths_in_flight=1000), 0), (mk(np=1001, max_paths_in_flight=1000), 0)]
    out += [(mk(np=4096, spp=64, max_paths_in_flight=8192), 0),           # small cap: many batches
            (mk(np=1 << 20, spp=64, max_paths_in_flight=(1 << 30) + 5), 0),       # clamped to 2^30 ...
            (mk(np=1 << 30, spp=3, max_paths_in_flight=1 << 40), 0), (mk(np=(1 << 30) + 1, spp=3, max_paths_in_flight=1 << 40), 0)]
    for spp in (15, 16, 17, 33):                                          # spp below, at and above nb_max = 16
        out.append((mk(np=1 << 16, spp=spp, max_paths_in_flight=1 << 20), 0))
    out += [(mk(np=2, spp=65534), 0), (mk(np=2, spp=65535), 0), (mk(np=2, spp=65536), 0), (mk(np=1, spp=1 << 20), 0)]   # nb_max hits 65535
    for key in ("workgroups", "export_below", "cont_workgroups", "regen_workgroups", "in_order", "profile", "capturing"):
        for v in (0, 1, 7, 300, 100000):                                  # every override zero and non-zero, beyond its clamps
            for n, spp in ((4096, 8), (1 << 20, 5)):
                out.append((mk(np=n, spp=spp, **{key: v}), 0))
                out.append((mk(np=n, spp=spp, level0_form=1, **{key: v}), 0))
    for n_objs in (128, 129):
        for blob in (0, 1152):
            for accel in (0, 1):
                for n, spp in ((4096, 8), (1 << 20, 5)):
                    out.append((mk(np=n, spp=spp, n_objs=n_objs, blob_f4=blob, accel=accel, diffuse_only=0), 0))
    for form in (0, 1, 2, 3):
        for split_ok in (0, 1):
            for diffuse in (0, 1):
                for occ in (0, 1, 3, 5, 6, 9):                            # occupancy unknown, below, at and above the compile-time figures
                    out.append((mk(np=1 << 20, spp=5, n_objs=13, blob_f4=117, level0_form=form, split_ok=split_ok, diffuse_only=diffuse), occ))
    for lst, regen, inject in ((1, 0, 0), (1, 1, 0), (1, 0, 1), (1, 1, 1)):    # pixel list, list with regen, given paths
        for n, spp in ((2048, 8), (1 << 18, 16)):
            for split_ok in (0, 1):
                out.append((mk(np=n, spp=spp, list=lst, list_regen=regen, inject=inject, split_ok=split_ok), 0))
    for n_cus in (1, 256, 304):
        out.append((mk(np=1 << 20, spp=5, n_cus=n_cus), 0))
    for scene, arg, W, H, spp, _ in bench.WORKLOADS.values():             # bench.py's own workloads (c1-c5, the 400 x 400 x 3000 job)
        n_objs = {1: 13, 2: 10, 4: arg}[scene]
        out.append((mk(np=W * H, spp=spp, n_objs=n_objs, blob_f4=9 * n_objs if n_objs <= 128 else 0, diffuse_only=int(scene != 1),
                       split_ok=int(scene == 1)), 0))
    return out


CASES = cases()


def test_case_grid_crosses_every_branch():
    """The grid reaches both sides of every decision of the restatement (a case list that stopped doing so would pass idly)."""
    seen = {}
    for i, occ in CASES:
        s = R.shape(i, occ)
        for k in ("lds_job", "split", "regen_scene", "over_cap", "hand_off", "regen", "overlap", "small_scene", "inject"):
            if k in s:
                seen.setdefault(k, set()).add(bool(s[k]))
        if not s["over_cap"]:
            seen.setdefault("clamped", set()).add(i["max_paths_in_flight"] > s["cap"])
            seen.setdefault("nb_65535", set()).add(s["nb_max"] == 65535)
            seen.setdefault("occ_binds", set()).add(bool(s["regen_scene"] and occ and occ < 5))
            seen.setdefault("chunk_bound_grid", set()).add(s["regen_launch_grid"] < s["regen_grid"])
            seen.setdefault("job_split", set()).add(bool(s["job"]["split"]))
            seen.setdefault("regen_export", set()).add(s["regen_export"] > 1)
    assert all(v == {False, True} for v in seen.values()), {k: v for k, v in seen.items() if v != {False, True}}


def test_sizing_equals_the_restatement():
    jf = _job_fields()
    for i, occ in CASES:
        want = R.shape(i, occ)
        rc, got, _ = device_shape(i, occ)
        assert rc == (5 if want["over_cap"] else 0), (i, rc)              # PT_ERR_UNSUPPORTED, as the render answers
        for k in OUT_FIELDS:
            if k in want:
                assert getattr(got, k) == int(want[k]), (k, getattr(got, k), want[k], i, occ)
        if not want["over_cap"]:
            for k in jf:
                assert getattr(got.job, k) == want["job"][k], ("job." + k, getattr(got.job, k), want["job"][k], i, occ)


def test_planned_launches_fit_what_was_sized():
    """shape() -> pt_debug_sched_render -> launch() for every launch of the plan, against the restatement and the two
    conditions of the sizing; every third case, each on a fresh scheduling state and once more behind itself."""
    n_checked = 0
    for i, occ in CASES[::3]:
        want = R.shape(i, occ)
        if want["over_cap"] or want["n_batches"] > 64:
            continue
        _, got, _ = device_shape(i, occ)
        sch = Sched()
        try:
            for _ in range(2):
                rc, ops, _ = sch.render(got.job)
                assert rc == 0
                _, _, ls = device_shape(i, occ, ops)
                for o, l in zip(ops, ls):
                    if o.kind != OP_LAUNCH:
                        assert all(getattr(l, k) == 0 for k in LAUNCH_FIELDS)
                        continue
                    ref = R.launch(want, o.batch, o.grid, o.level, o.flags)
                    assert {k: getattr(l, k) for k in LAUNCH_FIELDS} == ref, (i, occ, o.batch, o.level)
                    n_checked += 1
                    if o.level == 0:
                        assert l.n_first <= got.nw * l.seg_cap and l.seg_cap <= got.seg_cap, (i, occ)
                        if not got.regen:                                  # the queue the launch's segments live in
                            assert got.nw * l.seg_cap <= got.q_slots, (i, occ)
                        else:                                              # dealt chunks: whole rounds over the launch's waves, inside the batch
                            assert l.regen_static % (o.grid * 4) == 0 and l.regen_static * 64 <= l.n_first + 63, (i, occ)
                    else:
                        assert l.seg_cap == got.seg_cap_cont and got.nw_cont * l.seg_cap <= (got.q_slots_cont if o.own_queue else got.q_slots)
                if got.hand_off:
                    assert got.ovf_slots <= got.nw_cont * got.seg_cap_cont, (i, occ)
        finally:
            sch.close()
    assert n_checked > 200


def test_null_and_zero_arguments_are_refused():
    lib = pt._lib.lib()
    out = PtShapeOut()
    assert lib.pt_debug_render_shape(None, 0, C.byref(out), None, 0, None) == 1
    for key in ("np", "spp", "n_cus"):
        cin = PtShapeIn(**R.make_in(**{key: 0}))
        assert lib.pt_debug_render_shape(C.byref(cin), 0, C.byref(out), None, 0, None) == 1, key


# ---- the jobs recorded on an MI355X
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_counts.json")
SCENES = {1: dict(n_objs=13, diffuse_only=0, split_ok=1), 2: dict(n_objs=10, diffuse_only=1, split_ok=0)}


@pytest.mark.parametrize("name", [n for n in J.JOBS])
def test_recorded_grids_come_out_of_the_sizing(name):
    """shape() with the recorded CU count and occupancy, then the planner: the grids of the job's path-kernel dispatches in
    the kernel trace, in order.  (Of the adaptive job the first pass: the sizes of the later lists are the device's results.)"""
    rec = json.load(open(GOLDEN))
    job = rec["jobs"][name]
    scene, arg, entry, W, H, spp, cap, accel, form = J.JOBS[name]
    facts = SCENES.get(scene) or dict(n_objs=arg, diffuse_only=1, split_ok=0)
    if entry == "adaptive":
        spp = J.ADAPTIVE["spp_min"]
    i = R.make_in(np=W * H, spp=spp, max_paths_in_flight=cap, accel=accel, level0_form=form, n_cus=rec["n_cus"],
                  blob_f4=9 * facts["n_objs"] if facts["n_objs"] <= 128 else 0, **facts)
    rc, got, _ = device_shape(i, job["regen_per_cu"] or 0)
    assert rc == 0
    sch = Sched()
    try:
        _, ops, _ = sch.render(got.job)
    finally:
        sch.close()
    planned = [o.grid for o in ops if o.kind == OP_LAUNCH]
    traced = [d[1] for d in job["dispatches"] if "k_paths" in d[0]]
    assert all(d[2] == 256 for d in job["dispatches"] if "k_paths" in d[0])
    if entry == "adaptive":
        assert traced[:len(planned)] == planned
        assert all(g <= max(got.regen_capacity, got.cont_grid, got.grid) for g in traced)
    else:
        assert traced == planned
        assert (job["bounce_launches"], job["batches"]) == (len(planned), got.n_batches)
