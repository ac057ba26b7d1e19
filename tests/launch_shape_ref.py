"""The launch sizing of a render, restated in plain Python (test infrastructure for tests/test_launch_shape_cpu.py).

Written from render_impl as it stood at commit daf88e4 (pt_api.cpp:182-265 and the per-launch values at 389-431), where the
arithmetic was inline; it shares NO code with csrc/pt_shape.h and knows the constants by value.  C++'s unsigned 32-bit
arithmetic is spelled out (u32) where the driver computes in it."""

K_DEFAULT_MAX_PATHS, K_DEFAULT_MAX_PATHS_REGEN = 1 << 26, 1 << 28
K_PATHS_PER_WAVE_LDS, K_PATHS_PER_WAVE = 672, 1024
K_MIN_GRID, K_CONT_GRID = 256 * 8, 1024
K_REGEN_COUNTERS, K_REGEN_COUNTER_STRIDE = 8, 64
K_COUNT_STRIDE = (1 + K_REGEN_COUNTERS) * K_REGEN_COUNTER_STRIDE
K_SPLIT_BY_DEFAULT = True
K_REGEN_STATIC16, K_REGEN_EXPORT_BELOW, K_EXPORT_SMALL = 4, 1, 64
K_EXPORT_MIN_PATHS, K_REGEN_MIN_PATHS = 1 << 22, 1 << 17
K_BLOCK, K_SMALL_OBJS = 256, 128
K_WAVES_PER_BLOCK = K_BLOCK // 64
K_REGEN_WAVES_DIFFUSE, K_REGEN_WAVES_GENERIC, K_REGEN_WAVES_SPLIT = 6, 5, 5
K_REGEN_SPLIT_F4_PER_WAVE = 128 * 5
LAUNCH_REGEN, LAUNCH_STATIC_DEAL = 1, 8          # ptsched: Op.flags

IN_FIELDS = ("np", "max_paths_in_flight", "spp", "workgroups", "accel", "profile", "list", "list_regen", "inject", "n_objs", "blob_f4",
             "diffuse_only", "split_ok", "n_cus", "export_below", "cont_workgroups", "level0_form", "regen_workgroups", "in_order", "capturing")


def u32(x):
    return x & 0xFFFFFFFF


def make_in(**kw):
    """The inputs of a 64 x 64, 8 spp render of a ten-sphere diffuse scene on a 256-CU device, with overrides."""
    d = dict.fromkeys(IN_FIELDS, 0)
    d.update(np=4096, spp=8, n_objs=10, blob_f4=90, diffuse_only=1, n_cus=256)
    for k, v in kw.items():
        assert k in d, k
        d[k] = v
    return d


def shape(i, occupancy):
    """-> dict of every value render_impl derived before PREPARE ('over_cap': True and 'cap' alone for a refused tile)."""
    lst, inject = bool(i["list"]), bool(i["inject"])
    lds_job = (not lst or bool(i["list_regen"])) and not i["accel"] and i["n_objs"] <= K_SMALL_OBJS and i["blob_f4"] != 0
    split = lds_job and not lst and (i["level0_form"] == 3 or (i["level0_form"] == 0 and bool(i["split_ok"]) and K_SPLIT_BY_DEFAULT))
    regen_scene = split or (i["level0_form"] in (2, 0) and lds_job)
    out = dict(lds_job=lds_job, split=split, regen_scene=regen_scene)
    cap = i["max_paths_in_flight"] or (K_DEFAULT_MAX_PATHS_REGEN if regen_scene else K_DEFAULT_MAX_PATHS)
    cap = min(cap, 1 << 30)
    out.update(cap=cap, over_cap=i["np"] > cap)
    if out["over_cap"]:
        return out
    np_ = i["np"]
    spp = 1 if inject else i["spp"]
    nb_max = min(cap // np_, 65535, spp) or 1
    n_paths_max = np_ * nb_max
    n_batches = u32(spp + nb_max - 1) // nb_max
    export_small = min(256, max(1, i["export_below"])) if i["export_below"] else K_EXPORT_SMALL
    chunks_max = (n_paths_max + 63) // 64
    grid = i["workgroups"]
    small_scene = i["n_objs"] <= K_SMALL_OBJS or bool(i["accel"])
    paths_per_wave = K_PATHS_PER_WAVE_LDS if (i["n_objs"] <= K_SMALL_OBJS and not i["accel"]) else K_PATHS_PER_WAVE
    if not grid:
        per_block = paths_per_wave * K_WAVES_PER_BLOCK
        grid = u32(max((n_paths_max + per_block - 1) // per_block, K_MIN_GRID))
    grid = min(grid, (chunks_max + K_WAVES_PER_BLOCK - 1) // K_WAVES_PER_BLOCK) or 1
    nw = u32(grid * K_WAVES_PER_BLOCK)
    seg_cap = u32(((chunks_max + nw - 1) // nw) * 64)
    hand_off = not inject and n_paths_max > (K_REGEN_MIN_PATHS if regen_scene else K_EXPORT_MIN_PATHS)
    regen = regen_scene and hand_off
    regen_per_cu = K_REGEN_WAVES_SPLIT if split else K_REGEN_WAVES_DIFFUSE if i["diffuse_only"] else K_REGEN_WAVES_GENERIC
    if regen_scene and occupancy:
        regen_per_cu = min(regen_per_cu, occupancy)
    regen_capacity = u32(i["n_cus"] * regen_per_cu)
    regen_grid = min(65536, i["workgroups"] or i["regen_workgroups"] or regen_capacity)
    cont_grid = min(65536, i["cont_workgroups"]) if i["cont_workgroups"] else K_CONT_GRID
    nw_cont = cont_grid * K_WAVES_PER_BLOCK
    ovf_slots = (u32(regen_grid * K_WAVES_PER_BLOCK) if regen else nw) * max(export_small, 64) + 64
    seg_cap_cont = u32((((ovf_slots + 63) // 64 + nw_cont - 1) // nw_cont) * 64)
    q_slots_cont = nw_cont * seg_cap_cont if hand_off else 0
    q_slots = max(q_slots_cont, 64) if regen else max(nw * seg_cap, q_slots_cont)
    regen_export = 1 if split else min(export_small, 64) if i["export_below"] else K_REGEN_EXPORT_BELOW
    regen_launch_grid = min(regen_grid, (chunks_max + K_WAVES_PER_BLOCK - 1) // K_WAVES_PER_BLOCK)
    job_split = regen and split
    job = dict(n_batches=n_batches, regen=int(regen), split=int(job_split), hand_off=int(hand_off), regen_export=regen_export,
               profile=int(i["profile"] != 0), in_order=int(i["in_order"] != 0), capturing=int(i["capturing"] != 0), grid=grid,
               regen_grid=regen_launch_grid, cont_grid=cont_grid, regen_capacity=regen_capacity,
               fixed_grid=int(i["workgroups"] != 0 or i["regen_workgroups"] != 0), counter_words=K_COUNT_STRIDE,
               xchg_need=regen_launch_grid * K_WAVES_PER_BLOCK * K_REGEN_SPLIT_F4_PER_WAVE + 1024 if job_split else 0)
    out.update(np=np_, spp=spp, nb_max=nb_max, n_paths_max=n_paths_max, n_batches=n_batches, export_small=export_small,
               paths_per_wave=paths_per_wave, small_scene=small_scene, grid=grid, nw=nw, seg_cap=seg_cap, hand_off=hand_off, regen=regen,
               regen_per_cu=regen_per_cu, regen_capacity=regen_capacity, regen_grid=regen_grid, regen_launch_grid=regen_launch_grid,
               cont_grid=cont_grid, nw_cont=nw_cont, ovf_slots=ovf_slots, seg_cap_cont=seg_cap_cont, q_slots_cont=q_slots_cont,
               q_slots=q_slots, regen_export=regen_export, overlap=n_batches > 1 and not regen, inject=inject, job=job)
    return out


def launch(s, batch, grid, level, flags):
    """The per-launch values of the `exec` lambda's kOpLaunch case for a planned launch (batch, grid, level, flags)."""
    s0 = u32(batch * s["nb_max"])
    nb = min(s["nb_max"], u32(s["spp"] - s0))
    n_first = u32(s["np"] * nb)
    seg_cap = u32(((u32(n_first + 63) // 64 + s["nw"] - 1) // s["nw"]) * 64)
    src_mode = 1 if s["inject"] else 0
    export_below = (s["export_small"] if s["small_scene"] else K_BLOCK) if s["hand_off"] else 1
    if level > 0:
        n_first, seg_cap, src_mode, export_below = 0, s["seg_cap_cont"], 1, 1
    regen_static = 0
    if flags & LAUNCH_REGEN:
        export_below = s["regen_export"]
        nwr, nch = u32(grid * K_WAVES_PER_BLOCK), u32(n_first + 63) // 64
        if flags & LAUNCH_STATIC_DEAL:
            regen_static = u32(((nch * K_REGEN_STATIC16 // 16) // nwr) * nwr)
    return dict(s0=s0, nb=nb, n_first=n_first, seg_cap=seg_cap, src_mode=src_mode, export_below=export_below, regen_static=regen_static)
