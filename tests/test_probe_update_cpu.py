"""The irradiance volume's updates over frames (pt_probe_blend_host, pt_probe_rotation, pt_probe_update_rays_host)
without a GPU: the rule on the CPU against its numpy restatement (tests/probe_update_ref.py) bit for bit, the rotation of a frame,
the rays, what a fresh rotation per frame buys, and the refusals that need no device."""
import ctypes as C

import numpy as np
import pytest

import bake_ref as br
import probe_grid_ref as pr
import probe_update_ref as pu


GRID = pr.Grid((-0.8, -0.5, -2.6), (0.8, 1.0, 1.2), (3, 2, 2))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def test_exports_and_defaults(pt):
    lib = pt._lib.lib()
    for name in ("pt_probe_rotation", "pt_default_probe_update", "pt_probe_update_rays_host", "pt_debug_probe_update_rays", "pt_probe_blend_device",
                 "pt_probe_blend_host", "pt_probe_grid_update_device"):
        assert hasattr(lib, name) and name in pt._lib.SYMBOLS
    assert C.sizeof(pt._lib.PtProbeUpdate) == 64
    u = pt.default_probe_update(13, 8)
    assert (u.rays_per_probe, u.first, u.stride, u.hysteresis, u.change_threshold, u.reserved) == (64, 5, 8, 0.9375, 0.0, 0)
    assert _same(np.array(u.rotation[:], dtype=np.float32), pt.probe_rotation(13).reshape(9))
    assert pt.default_probe_update(3, 0).stride == 1 and pt.default_probe_update(3, 0).first == 0
    assert pt.probe_update_slots(12, pt.default_probe_update(1, 3)) == 4 and pt.probe_update_slots(11, pt.default_probe_update(2, 3)) == 3


@pytest.mark.parametrize("R, T, index", pu.blend_cases())
def test_blend_against_the_restatement(pt, R, T, index):
    c = pu.blend_case(R, T, index)
    want = pu.update(c["upd"], c["vis"], pt.probe_directions(R), c["rad"], c["dist"], c["sh"], c["mom"], c["age"])
    keep = [None if a is None else a.copy() for a in (c["sh"], c["mom"], c["age"])]
    got = pt.probe_blend_host(pu.pt_update(pt, c["upd"]), pu.pt_vis(pt, c["vis"]), c["rad"], c["dist"], c["sh"], c["mom"], c["age"])
    assert _same(got[0], want[0]) and np.array_equal(got[2], want[2])
    assert (T is None and got[1] is None) or _same(got[1], want[1])
    # the probes that are no slot, as words; the ages; what a NaN plane becomes; the inputs
    rest = np.setdiff1d(np.arange(c["P"]), pu.slots(c["P"], 1, 2))
    assert _same(got[0][rest], c["sh"][rest]) and np.array_equal(got[2][rest], c["age"][rest])
    assert list(got[2][1::2]) == [1, 2, 16, 17, 65535]
    assert _same(c["sh"], keep[0]) and np.array_equal(c["age"], keep[2])
    assert np.isfinite(got[0][1]).all() or not np.isfinite(c["rad"][0]).all()           # slot 0: age 0 over a NaN plane
    if T is not None:
        assert _same(got[1][rest], c["mom"][rest]) and np.isfinite(got[1][1]).all() and _same(c["mom"], keep[1])


def test_the_gate_and_the_hysteresis_act(pt):
    """what the cases above rely on: with the gate tripped a changed probe moves further than the floor takes it, a gate that is not
    tripped is the gate off bit for bit, and h = 0 replaces the state"""
    c = pu.blend_case(64, 8, 1)
    outs = {}
    for name, (threshold, ca) in zip(("off", "quiet", "tripped"), pu.GATES):
        upd = dict(c["upd"], h=0.9375, threshold=threshold, change_alpha=ca)
        outs[name] = pt.probe_blend_host(pu.pt_update(pt, upd), pu.pt_vis(pt, c["vis"]), c["rad"], c["dist"], c["sh"], c["mom"], c["age"])
    assert _same(outs["off"][0], outs["quiet"][0]) and _same(outs["off"][1], outs["quiet"][1])
    p = 9                                                                              # slot 4: age 65535, radiance x 40
    assert not _same(outs["off"][0][p], outs["tripped"][0][p]) and not _same(outs["off"][1][p], outs["tripped"][1][p])
    move = lambda o: abs(float(o[0][p, 0, 0]) - float(c["sh"][p, 0, 0]))
    assert move(outs["tripped"]) > 4.0 * move(outs["off"])
    fresh = pt.probe_blend_host(pu.pt_update(pt, dict(c["upd"], h=0.0, threshold=0.0)), None, c["rad"], None, c["sh"], None, c["age"])
    zero = pt.probe_blend_host(pu.pt_update(pt, dict(c["upd"], h=0.0, threshold=0.0)), None, c["rad"], None, c["sh"], None, np.zeros(11, dtype=np.uint32))
    assert _same(fresh[0][[7, 9]], zero[0][[7, 9]])                                       # (slot 2, probe 5, has radiance that is not finite)


@pytest.mark.parametrize("stride", [10, 11, 12, 0x7FFFFFFF, 0xFFFFFFFF])
def test_a_stride_past_the_grid_leaves_one_slot(pt, stride):
    """first = 1 of 11 probes: every stride from 10 on leaves the slot `first` alone, up to 2^32 - 1 (no sum in the slot count may wrap)"""
    c = pu.blend_case(65, 2, 3)
    upd = dict(c["upd"], stride=stride)
    assert pt.probe_update_slots(c["P"], pu.pt_update(pt, upd)) == len(pu.slots(c["P"], 1, stride)) == 1
    want = pu.update(upd, c["vis"], pt.probe_directions(65), c["rad"][:1], c["dist"][:1], c["sh"], c["mom"], c["age"])
    got = pt.probe_blend_host(pu.pt_update(pt, upd), pu.pt_vis(pt, c["vis"]), c["rad"][:1], c["dist"][:1], c["sh"], c["mom"], c["age"])
    assert _same(got[0], want[0]) and _same(got[1], want[1]) and np.array_equal(got[2], want[2])
    assert got[2][1] == 1 and not _same(got[0][1], c["sh"][1])
    g = GRID.as_pt(pt)
    far = pt.default_probe_update(0, stride, rays_per_probe=4, first=11)
    rays = pt.probe_update_rays_host(g, far, np.array([(3, 0, 0)], dtype=np.uint32))
    assert _same(rays[0, :3], pr.positions(GRID).astype(np.float32)[11])
    with pytest.raises(pt._lib.PtError):
        pt.probe_update_rays_host(g, far, np.array([(0, 1, 0)], dtype=np.uint32))


def test_rotation_of_a_frame(pt):
    assert _same(pt.probe_rotation(0), np.eye(3, dtype=np.float32))
    seen = set()
    for frame in range(1, 65):
        M = pt.probe_rotation(frame).astype(np.float64)
        assert np.abs(M @ M.T - np.eye(3)).max() <= 1e-6 and np.linalg.det(M) > 0.99
        assert np.abs(M - pu.rotation(frame).astype(np.float64)).max() <= 1e-6
        seen.add(M.tobytes())
    assert len(seen) == 64 and np.eye(3).tobytes() not in seen




def ray_case(pt, R, frame):
    upd = pt.default_probe_update(frame, 3, rays_per_probe=R, first=1)
    n_upd = pt.probe_update_slots(12, upd)
    xys = np.array([(r, k, s) for k in range(n_upd) for r in range(R) for s in (0, 3)], dtype=np.uint32)
    return upd, n_upd, xys


@pytest.mark.parametrize("frame", [0, 5])
@pytest.mark.parametrize("R", [12, 16])
def test_rays_against_the_restatement(pt, R, frame):
    g = GRID.as_pt(pt)
    upd, n_upd, xys = ray_case(pt, R, frame)
    assert n_upd == 4
    got = pt.probe_update_rays_host(g, upd, xys)
    pos = pr.positions(GRID).astype(np.float32)
    dirs = pu.rotate(pu.rotation(frame), pt.probe_directions(R))
    assert _same(np.array(upd.rotation[:], dtype=np.float32), pu.rotation(frame).reshape(9))
    want = np.concatenate([pos[1 + 3 * xys[:, 1]], dirs[xys[:, 0]]], axis=1)
    assert _same(got, want)
    assert np.abs(np.linalg.norm(got[:, 3:6].astype(np.float64), axis=1) - 1.0).max() < 1e-6
    probes = 1 + 3 * xys[:, 1]
    bake = pt.bake_rays_host("probes", (pos, R), np.stack([xys[:, 0], probes, xys[:, 2]], axis=1))
    assert _same(got, bake) == (frame == 0)


def _sq_err(sh, truth):
    return float(((sh.astype(np.float64) - truth.astype(np.float64)) ** 2).sum())


def test_a_fresh_rotation_per_frame_pays(pt):
    """An analytic field of three cos^8 lobes (not band-limited), one probe, R = 16.  The plain mean of the frames 1..16 (h = 15/16
    from age 0: alpha = 1 / (age + 1) throughout) has at most a quarter of the mean squared SH error of the sixteen single updates,
    against the projection of the same field at R = 65536: independent errors would give 1/16, the factor 4 is room for correlation
    between rotated spirals.  Sixteen identity frames leave a single update's error as it is."""
    R, big = 16, 65536
    truth = br.sh_project(pu.field(br.probe_dirs(big))[None], br.probe_dirs(big))[0][0]          # (f64: the library's rows end at 65535)
    g = pr.Grid((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (1, 1, 1)).as_pt(pt)
    xys = np.array([(r, 0, 0) for r in range(R)], dtype=np.uint32)

    def run(frames):
        sh, age, singles = np.full((1, 9, 3), np.nan, dtype=np.float32), np.zeros(1, dtype=np.uint32), []
        for f in frames:
            upd = pt.default_probe_update(f, 1, rays_per_probe=R, hysteresis=15.0 / 16.0)
            rad = pu.field(pt.probe_update_rays_host(g, upd, xys)[:, 3:6])[None]
            sh, _, age = pt.probe_blend_host(upd, None, rad, None, sh, None, age)
            singles.append(pt.probe_blend_host(upd, None, rad, None, np.zeros((1, 9, 3), dtype=np.float32), None, np.zeros(1, dtype=np.uint32))[0][0])
        return sh[0], singles, int(age[0])

    mean, singles, age = run(range(1, 17))
    single_err = [_sq_err(s, truth) for s in singles]
    print("squared SH error: mean of 16 rotated frames %.6g, single updates mean %.6g (min %.6g max %.6g), ratio %.4f" %
          (_sq_err(mean, truth), np.mean(single_err), min(single_err), max(single_err), _sq_err(mean, truth) / np.mean(single_err)))
    assert age == 16
    assert _sq_err(mean, truth) <= 0.25 * np.mean(single_err)
    same, ident, _ = run([0] * 16)
    assert _same(same, ident[0]) and _sq_err(same, truth) == _sq_err(ident[0], truth)
    assert _sq_err(same, truth) > 4.0 * _sq_err(mean, truth)


def test_refusals_that_need_no_device(pt):
    L = pt._lib.lib()
    c = pu.blend_case(16, 8, 0)
    vis = pu.pt_vis(pt, c["vis"])
    pv_ = lambda a: a.ctypes.data_as(C.c_void_p)

    def blend(upd, vis=vis, age=c["age"].copy(), dist=c["dist"], P=c["P"]):
        sh, mom = c["sh"].copy(), c["mom"].copy()
        age_p = age if age is None or isinstance(age, C.c_void_p) else pv_(age)
        return L.pt_probe_blend_host(P, C.byref(upd), None if vis is None else C.byref(vis), pv_(c["rad"]), None if dist is None else pv_(dist),
                                     pv_(sh), pv_(mom), age_p)

    def refused(rc, text):
        assert rc == 1 and text in L.pt_last_error().decode() and L.pt_last_error(), (rc, L.pt_last_error())

    good = pu.pt_update(pt, c["upd"])
    assert blend(good) == 0
    skew = np.eye(3, dtype=np.float32); skew[0, 1] = 1e-4
    for over, text in ((dict(rays_per_probe=0), "rays_per_probe"), (dict(rays_per_probe=65536), "rays_per_probe"), (dict(stride=0), "stride"),
                       (dict(first=11), "first"), (dict(hysteresis=1.0), "hysteresis"), (dict(hysteresis=-0.1), "hysteresis"),
                       (dict(hysteresis=float("nan")), "hysteresis"), (dict(change_threshold=-1.0), "change_threshold"),
                       (dict(change_threshold=float("inf")), "change_threshold"), (dict(change_alpha=1.5), "change_alpha"),
                       (dict(change_alpha=float("nan")), "change_alpha"), (dict(rotation=np.full(9, np.nan)), "rotation"),
                       (dict(rotation=skew), "orthonormal"), (dict(rotation=np.diag([1.0, 1.0, -1.0])), "determinant"),
                       (dict(rotation=np.zeros(9)), "orthonormal")):
        bad = pu.pt_update(pt, c["upd"])
        for k, v in over.items():
            if k == "rotation":
                for i, m in enumerate(np.asarray(v, dtype=np.float32).reshape(9)):
                    bad.rotation[i] = float(m)
            else:
                setattr(bad, k, v)
        refused(blend(bad), text)
        g = GRID.as_pt(pt)
        xys, out = np.zeros((1, 3), dtype=np.uint32), np.zeros((1, 6), dtype=np.float32)
        if over != dict(first=11):
            refused(L.pt_probe_update_rays_host(C.byref(g), C.byref(bad), pv_(xys), 1, pv_(out)), text)
        refused(L.pt_probe_blend_device(None, c["P"], C.byref(bad), C.byref(vis), pv_(c["rad"]), pv_(c["dist"]), pv_(c["sh"]), pv_(c["mom"]),
                                        pv_(c["age"])), text)
    refused(blend(good, age=None), "age")
    refused(blend(good, age=C.c_void_p(c["age"].ctypes.data + 2)), "age")
    refused(blend(good, dist=None), "distances")
    refused(blend(good, P=0), "n_probes")
    refused(blend(good, vis=pt.default_probe_visibility(None, resolution=17)), "resolution")
    refused(L.pt_probe_blend_host(c["P"], None, None, pv_(c["rad"]), None, pv_(c["sh"]), None, pv_(c["age"])), "null")
    refused(L.pt_probe_grid_update_device(None, None, None, None, None, None, None, None), "null")
    # the rays: a position outside the film, an invalid grid
    g = GRID.as_pt(pt)
    upd = pt.default_probe_update(0, 3, rays_per_probe=16, first=1)
    out = np.zeros((1, 6), dtype=np.float32)
    for xy in ((16, 0, 0), (0, 4, 0)):
        refused(L.pt_probe_update_rays_host(C.byref(g), C.byref(upd), pv_(np.array([xy], dtype=np.uint32)), 1, pv_(out)), "outside")
    bad_grid = pr.Grid((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (0, 1, 1)).as_pt(pt)
    refused(L.pt_probe_update_rays_host(C.byref(bad_grid), C.byref(upd), pv_(np.zeros((1, 3), dtype=np.uint32)), 1, pv_(out)), "grid")
