"""The recorded jobs of tests/golden/launch_counts.json: small renders either side of every threshold of the launch sizing
(csrc/pt_shape.h).  Test infrastructure shared by tools/record_launch_counts.py (which records them, once, on an MI355X),
tests/test_gpu_launch_shape.py (the device repeats them) and tests/test_launch_shape_cpu.py (the sizing reproduces their grids).

A job: name -> (scene, scene arg, entry, width, height, spp, max_paths_in_flight, accel, level0_form).  accel is explicit
(never PT_ACCEL_AUTO), so that the sizing's input is in the job and not in the scene's weight."""
JOBS = {
    "queue_4_batches": (2, 0, "render", 64, 64, 8, 8192, 0, 0),       # four batches of 8192 paths: the queue form, overlapped
    "below_2_17": (2, 0, "render", 256, 256, 2, 0, 0, 0),             # 2^17 paths: not above kRegenMinPaths
    "above_2_17": (2, 0, "render", 256, 256, 3, 0, 0, 0),             # the regenerating kernel
    "below_2_22": (2, 0, "render", 1024, 1024, 4, 0, 0, 0),
    "above_2_22": (2, 0, "render", 1024, 1024, 5, 0, 0, 0),
    "queue_below_2_22": (2, 0, "render", 1024, 1024, 4, 0, 0, 1),     # level0_form = 1: kExportMinPaths decides the hand-off
    "queue_above_2_22": (2, 0, "render", 1024, 1024, 5, 0, 0, 1),
    "split": (1, 0, "render", 256, 256, 3, 0, 0, 0),                  # a minority of Mirror objects: k_paths_regen_split
    "objs_129": (4, 129, "render", 256, 256, 3, 0, 0, 0),             # one object too many for LDS: the tiled scan
    "accel_1": (2, 0, "render", 256, 256, 3, 0, 1, 0),
    "adaptive_list": (2, 0, "adaptive", 384, 384, 40, 0, 0, 0),       # passes after the first: pixel lists with regen
}
ADAPTIVE = dict(spp_min=8, spp_step=16, rel_tol=0.05)


def run(pt, ctx, name):
    """One job on the device -> dict(bounce_launches, batches, primary_launches, launch_log)"""
    scene, arg, entry, W, H, spp, cap, accel, form = JOBS[name]
    ctx.upload(pt.builtin_scene(scene, arg))
    ctx.set_tuning(level0_form=form)
    try:
        ctx.launch_log()
        cam = pt.camera_new(width=W, height=H)
        prm = pt.default_params(spp=spp, max_paths_in_flight=cap, accel=accel)
        if entry == "render":
            ctx.render(cam, prm)
        else:
            ctx.render_adaptive(cam, prm, **ADAPTIVE)
        st = ctx.stats()          # (the sums over an adaptive render's passes)
        out = dict(bounce_launches=st.bounce_launches, batches=st.batches, primary_launches=st.primary_launches,
                   launch_log=ctx.launch_log())
    finally:
        ctx.set_tuning()
    return out
