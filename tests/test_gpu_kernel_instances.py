"""Every path-kernel instance the library ships, run on purpose and pinned against the oracle.

The dispatch picks one instance of k_paths / k_paths_bvh / k_paths_regen / k_paths_regen_split per launch from the scene's
material set, the integrator, the object count, accel, the entry (image, pixel list, adaptive pass), the batch size and
PtTuning.level0_form; the launch log (pt_debug_launch_log) records which.  The table of every instance
(pt_debug_path_instances) is the set of kernels in the shipped code objects (tests/test_kernel_instances_cpu.py).  Here
one case per table entry builds the job that lands on that instance and checks

  * that the instance ran (it is in the job's launch log; a continuation instance after its level-0 launch);
  * exact arithmetic: the film is the f32 oracle's bit for bit (the whole film and the counters of small jobs; a seeded
    subset of pixels of jobs above the 2^22-path hand-off), and bit-identical to the film of the same job in another form;
  * fast arithmetic: bit-identical to the film of the same job on a different instance, and within the FP32 bar of
    test_gpu_parity against the f64 oracle;
  * adaptive passes (pixel lists of the regenerating kernel): a pixel with n samples is pt_render_pixels at spp = n.

Jobs are cached: the level-0 and continuation instances of one job share its GPU run and its oracle."""
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
F64, F32, REC, ITER = 64, 32, 0, 1
THREADS = min(16, os.cpu_count() or 1)
OBSERVED = set()          # every code seen in any launch log of this module

# Job sizes.  small: below both hand-off thresholds (one queue-form launch); regen: above 2^17 paths (regenerating level-0
# launch + continuation) and below 2^22; big: above 2^22 paths (queue-form hand-off to a continuation launch).
SIZES = {"small": (64, 64, 8), "regen": (128, 128, 9), "big": (1024, 1024, 5)}
# Adaptive jobs: the first pass (the whole image, spp_min samples) is not a pixel list; the second (spp_step more samples for
# the pixels whose noise estimate is above rel_tol: most of them) is, and above 2^17 paths: the regenerating LIST kernel.
ADAPTIVE = dict(W=384, H=384, spp_min=8, spp_step=16, spp_max=40, rel_tol=0.05)
N_SUBSET = 1024           # pixels of the big jobs compared with the oracle (>= 99.5 % within the bar: at most 5 outside)


def _with(prm, **kw):
    q = type(prm)()
    for name, _ in prm._fields_:
        setattr(q, name, getattr(prm, name))
    for k, v in kw.items():
        setattr(q, k, v)
    return q


@functools.lru_cache(maxsize=None)
def _scene(pt, name):
    """diffuse: the ten-sphere Cornell box (Lambertian + emissive); oren: the same with OrenNayar walls and spheres, no
    Mirror; mirror_min: the reference Cornell box (one Mirror sphere of 13 objects); mirror_min_oren: the same with
    OrenNayar walls; mirror_maj: the reference box with eight Mirror walls; tiled: 200 random spheres (more than 128
    objects: the tiled scan), some OrenNayar and Mirror."""
    if name in ("diffuse", "oren"):
        objs = list(pt.builtin_scene(2))
    elif name == "tiled":
        objs = list(pt.builtin_scene(4, 200))
    else:
        objs = list(pt.builtin_scene(1))
    glass = list(pt.builtin_scene(1)[12].mat)
    for k, o in enumerate(objs):
        if o.mat_tag != 0:
            continue
        if name in ("oren", "mirror_min_oren") or (name == "tiled" and k % 5 == 1):
            o.mat_tag = 3
            o.mat[3] = [0.0, 0.3, 0.6, 1.0][k % 4]
        elif (name == "mirror_maj" and k < 8) or (name == "tiled" and k % 7 == 3):
            o.mat_tag = 2
            for j in range(6):
                o.mat[j] = glass[j]
    return (pt._lib.PtObject * len(objs))(*objs)


def _job_for(pt, code):
    """The job that lands on instance `code`: (scene, entry, size, accel, level0_form, integrator, exact, export_below).
    A regenerating launch hands its last live paths to a continuation launch only with PtTuning.export_below set."""
    d = pt.path_instance(code)
    integ, exact = 0 if d["mis"] else 1, int(d["exact"])
    fam = d["family"]
    if fam == "k_paths" and d["mode"] == 1:                  # tiled scan: > 128 objects
        return ("tiled", "pixels" if d["list"] else "render", "big" if d["ovf"] else "small", 0, 1, integ, exact, 0)
    if fam == "k_paths" and d["list"]:                       # continuation of an adaptive pass / plain pixel list
        if d["ovf"]:
            return ("mirror_min", "adaptive", "adaptive", 0, 2, integ, exact, 64)
        return ("mirror_min", "pixels", "small", 0, 1, integ, exact, 0)
    if fam == "k_paths":                                     # continuation of a regenerating launch / queue-form level 0
        scene = "diffuse" if d["mats"] else "mirror_min"
        if d["ovf"]:
            return (scene, "render", "regen", 0, 2, integ, exact, 64)
        return (scene, "render", "small", 0, 1, integ, exact, 0)
    if fam == "k_paths_bvh":
        scene = "diffuse" if d["mats"] else "mirror_min"
        return (scene, "pixels" if d["list"] else "render", "big" if d["ovf"] else "small", 1, 1, integ, exact, 0)
    if fam == "k_paths_regen":
        scene = {0: "mirror_maj", 1: "diffuse", 2: "oren"}[d["mats"]]
        if d["list"]:     # (with BRDF-only sampling most pixels of the Mirror-walled box see no light and stop at spp_min)
            return ("mirror_min" if scene == "mirror_maj" else scene, "adaptive", "adaptive", 0, 2, integ, exact, 0)
        return (scene, "render", "regen", 0, 2, integ, exact, 0)
    scene = "mirror_min" if d["mats"] == 1 else "mirror_min_oren"   # k_paths_regen_split: PLAIN
    return (scene, "render", "regen", 0, 3, integ, exact, 0)


def _alt(job):
    """The same job in another form -- a different instance, the same film (the film depends on neither level0_form nor
    accel): regenerating forms -> the queue form; otherwise the linear scan <-> the BVH."""
    scene, entry, size, accel, form, integ, exact, eb = job
    if form in (2, 3):
        return (scene, entry, size, accel, 1, integ, exact, eb)
    return (scene, entry, size, 1 - accel, 1, integ, exact, eb)


def _list_xy(W, H, size):
    """Pixel list of a pixels job: every pixel of a big image, 2048 of a small one, in a seeded random order."""
    rng = np.random.default_rng(7)
    n = W * H if size == "big" else 2048
    flat = rng.permutation(W * H)[:n]
    return np.stack([flat % W, flat // W], axis=1).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def _run(pt, ctx, job):
    """-> dict(log, lin, rgba, stats[, xy, spp]) of one GPU run of the job."""
    scene, entry, size, accel, form, integ, exact, eb = job
    W, H, spp = (ADAPTIVE["W"], ADAPTIVE["H"], ADAPTIVE["spp_max"]) if entry == "adaptive" else SIZES[size]
    cam = pt.camera_new(width=W, height=H)
    ctx.upload(_scene(pt, scene))
    ctx.set_tuning(level0_form=form, export_below=eb)
    try:
        ctx.launch_log()
        out = {}
        if entry == "render":
            prm = pt.default_params(spp=spp, integrator=integ, exact_math=exact, accel=accel)
            lin, rgba = ctx.render(cam, prm)
            st = ctx.stats()
            out.update(lin=lin.cpu().numpy(), rgba=rgba.cpu().numpy(), vertices=st.vertices, shadow_rays=st.shadow_rays)
        elif entry == "pixels":
            prm = pt.default_params(spp=spp, integrator=integ, exact_math=exact, accel=accel)
            xy = _list_xy(W, H, size)
            lin, rgba, _ = ctx.render_pixels(cam, prm, xy)
            out.update(lin=lin, rgba=rgba, xy=xy)
        else:
            prm = pt.default_params(spp=spp, integrator=integ, exact_math=exact, accel=accel)
            lin, rgba, n, _ = ctx.render_adaptive(cam, prm, spp_min=ADAPTIVE["spp_min"], spp_step=ADAPTIVE["spp_step"],
                                                  rel_tol=ADAPTIVE["rel_tol"])
            out.update(lin=lin, rgba=rgba, spp=n)
        out.update(log=ctx.launch_log(), cam=cam, prm=prm)
    finally:
        ctx.set_tuning()
    OBSERVED.update(out["log"])
    return out


@functools.lru_cache(maxsize=None)
def _oracle_full(pt, orc, job, precision):
    scene, entry, size, accel, form, integ, exact, eb = job
    W, H, spp = SIZES[size]
    prm = pt.default_params(spp=spp, integrator=integ)
    return orc.render(pt.camera_new(width=W, height=H), _scene(pt, scene), prm, precision, ITER if precision == F32 else REC,
                      THREADS)


def _subset(n, k, seed):
    rng = np.random.default_rng(seed)
    return np.sort(rng.choice(n, size=min(n, k), replace=False))


def _within_bar(got, ref):
    """test_gpu_parity._check's FP32 bar: per channel |d| <= 1e-3 + 1e-2 |ref| on >= 99.5 % of pixels, mean within 1e-3."""
    g = got.astype(np.float64).reshape(-1, 3)
    ref = ref.reshape(-1, 3)
    ok = (np.abs(g - ref) <= 1e-3 + 1e-2 * np.abs(ref)).all(-1)
    assert ok.mean() >= 0.995, f"{int((~ok).sum())} of {len(ok)} pixels outside the FP32 bar"
    if ref.mean() > 0:
        assert abs(g.mean() - ref.mean()) <= 1e-3 * ref.mean(), (g.mean(), ref.mean())


def _check_oracle(pt, orc, job, r):
    """Exact: bit for bit with the f32 oracle.  Fast: the FP32 bar against the f64 oracle."""
    scene, entry, size, accel, form, integ, exact, eb = job
    objs, cam, prm = _scene(pt, scene), r["cam"], r["prm"]
    prec = F32 if exact else F64
    form_o = ITER if exact else REC
    if entry == "render" and size != "big":
        ref, ref8, cnt = _oracle_full(pt, orc, job, prec)
        if exact:
            assert np.array_equal(r["lin"], ref.astype(np.float32)), \
                f"{int((r['lin'] != ref.astype(np.float32)).any(-1).sum())} pixels differ from the f32 oracle"
            assert np.array_equal(r["rgba"], ref8)
            assert (r["vertices"], r["shadow_rays"]) == (cnt["vertices"], cnt["shadow_rays"])
        else:
            _within_bar(r["lin"], ref)
        return
    if entry == "adaptive":       # per spp group, a seeded subset
        W = cam.width
        sel = _subset(W * cam.height, 256 if exact else N_SUBSET, 11)
        ys, xs = sel // W, sel % W
        got, ref = [], []
        for n in np.unique(r["spp"][ys, xs]):
            m = r["spp"][ys, xs] == n
            xy = np.stack([xs[m], ys[m]], axis=1)
            lin, _ = orc.render_pixels(cam, objs, _with(prm, spp=int(n)), xy, prec, form_o)
            got.append(r["lin"][ys[m], xs[m]])
            ref.append(lin)
        got, ref = np.concatenate(got), np.concatenate(ref)
    else:
        if entry == "render":     # big image: a seeded subset of pixels
            sel = _subset(cam.width * cam.height, N_SUBSET, 5)
            xy = np.stack([sel % cam.width, sel // cam.width], axis=1)
            got = r["lin"].reshape(-1, 3)[sel]
        else:                     # pixel list: all of a small one, a subset of a big one
            sel = _subset(len(r["xy"]), N_SUBSET if size == "big" else len(r["xy"]), 5)
            xy = r["xy"][sel]
            got = r["lin"][sel]
        ref, _ = orc.render_pixels(cam, objs, prm, xy, prec, form_o)
    if exact:
        assert np.array_equal(got, ref.astype(np.float32)), \
            f"{int((got != ref.astype(np.float32)).any(-1).sum())} of {len(got)} pixels differ from the f32 oracle"
    else:
        _within_bar(got, ref)


def _check_adaptive_rule(pt, ctx, r):
    """A pixel with n samples is pt_render_pixels at spp = n, bit for bit (linear film and RGBA8)."""
    cam, prm, spp = r["cam"], r["prm"], r["spp"]
    assert len(np.unique(spp)) >= 2, np.unique(spp)
    sel = _subset(cam.width * cam.height, 512, 3)
    ys, xs = sel // cam.width, sel % cam.width
    for n in np.unique(spp[ys, xs]):
        m = spp[ys, xs] == n
        xy = np.stack([xs[m], ys[m]], axis=1)
        plin, prgba, _ = ctx.render_pixels(cam, _with(prm, spp=int(n)), xy)
        assert np.array_equal(plin, r["lin"][ys[m], xs[m]]), f"spp {n}: linear film differs from pt_render_pixels"
        assert np.array_equal(prgba, r["rgba"][ys[m], xs[m]]), f"spp {n}: RGBA8 differs from pt_render_pixels"


def _table():
    import pathtrace_amd as pt
    return pt.path_instances()


def _name(code):
    import pathtrace_amd as pt
    d = pt.path_instance(code)
    return d["kernel"].replace(" ", "") + ("-exact" if d["exact"] else "-fast")


@pytest.mark.parametrize("code", _table(), ids=_name)
def test_instance(pt, orc, gpu_ctx, code):
    d = pt.path_instance(code)
    job = _job_for(pt, code)
    r = _run(pt, gpu_ctx, job)
    log = r["log"]
    # 1. the instance ran; a continuation launch follows the level-0 launch of its batch
    assert code in log, (d["kernel"], [pt.path_instance(c)["kernel"] for c in log])
    if d["ovf"]:
        first = log.index(code)
        assert any(not pt.path_instance(c)["ovf"] for c in log[:first]), "continuation launch without a level-0 launch before it"
    assert all(pt.path_instance(c)["exact"] == d["exact"] for c in log)
    # 2. / 3. the oracle
    _check_oracle(pt, orc, job, r)
    # the same job in another form: another instance, the same film
    if job[1] == "adaptive":
        _check_adaptive_rule(pt, gpu_ctx, r)
    else:
        a = _run(pt, gpu_ctx, _alt(job))
        assert code not in a["log"], "the other form took the same instance"
        assert np.array_equal(r["lin"], a["lin"]), f"{int((r['lin'] != a['lin']).any(-1).sum())} pixels differ between the forms"
        assert np.array_equal(r["rgba"], a["rgba"])
        if job[1] == "render":
            assert (r["vertices"], r["shadow_rays"]) == (a["vertices"], a["shadow_rays"])


def test_every_instance_was_launched(pt, gpu_ctx):
    """The union of the launch logs of the jobs above is the table: each instance ran (the jobs are cached: this runs only
    what the cases above did not)."""
    table = pt.path_instances()
    for code in table:
        _run(pt, gpu_ctx, _job_for(pt, code))
    assert OBSERVED <= set(table), sorted(OBSERVED - set(table))
    missing = sorted(set(table) - OBSERVED)
    assert not missing, [_name(c) for c in missing]
