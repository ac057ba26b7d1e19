#!/usr/bin/env python3
"""Records tests/golden/launch_counts.json: what the jobs of tests/launch_shape_jobs.py launch on an MI355X.

  python tools/record_launch_counts.py run RUN.json
      runs every job once on device 0 and writes the statistics (bounce_launches, batches, primary_launches), the launch log
      and the device's CU count.  Under a kernel trace,
          rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/record_launch_counts.py run RUN.json
      (tracing alone, no counters), DIR/*/*_kernel_trace.csv then holds every dispatch of the run.
  python tools/record_launch_counts.py merge RUN.json TRACE.csv OUT.json
      adds to every job its dispatches in the order they were enqueued -- [kernel name, grid in workgroups, workgroup size] --
      and the workgroups per CU its regenerating launch took (regen_per_cu: grid / CU count where the grid is not bounded by
      the batch's chunks; the occupancy the context cached for the job's kernel, capped by the figure it is compiled for).

A job starts with a scene upload, whose two k_scene_setup dispatches mark its begin in the trace."""
import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def record(out_path):
    import torch
    import pathtrace_amd as pt
    from tests import launch_shape_jobs as J
    ctx = pt.Context(0)
    rec = {"n_cus": torch.cuda.get_device_properties(0).multi_processor_count, "jobs": {}}
    for name in J.JOBS:
        rec["jobs"][name] = J.run(pt, ctx, name)
    ctx.close()
    with open(out_path, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps({k: {x: y for x, y in v.items() if x != "launch_log"} for k, v in rec["jobs"].items()}))


def merge(run_path, trace_path, out_path):
    from tests import launch_shape_jobs as J
    rec = json.load(open(run_path))
    rows = [r for r in csv.DictReader(open(trace_path)) if r["Kind"] == "KERNEL_DISPATCH"]
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    jobs, cur, prev_setup = [], None, False
    for r in rows:
        name = r["Kernel_Name"]
        name = name[:-3] if name.endswith(".kd") else name
        if "k_scene_setup" in name:
            if not prev_setup:
                cur = []
                jobs.append(cur)
            prev_setup = True
            continue
        prev_setup = False
        if cur is not None and not name.startswith("__amd_rocclr_"):      # (the runtime's own copy and fill kernels)
            wg = int(r["Workgroup_Size_X"])
            cur.append([name, int(r["Grid_Size_X"]) // wg, wg])
    assert len(jobs) == len(J.JOBS), (len(jobs), len(J.JOBS))
    for (name, job), disp in zip(J.JOBS.items(), jobs):
        rec["jobs"][name]["dispatches"] = disp
        paths = [d for d in disp if "k_paths" in d[0]]
        assert len(paths) == len(rec["jobs"][name]["launch_log"]), name
        regen = [d[1] for d in paths if "k_paths_regen" in d[0]]
        per_cu = None
        if regen and job[2] == "render":
            W, H, spp = job[3], job[4], job[5]
            bound = ((W * H * spp + 63) // 64 + 3) // 4
            if regen[0] < bound and regen[0] % rec["n_cus"] == 0:
                per_cu = regen[0] // rec["n_cus"]
        rec["jobs"][name]["regen_per_cu"] = per_cu
    with open(out_path, "w") as f:
        json.dump(rec, f, indent=1)
    print(f"{out_path}: {sum(len(j['dispatches']) for j in rec['jobs'].values())} dispatches of {len(jobs)} jobs")


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "run":
        record(sys.argv[2])
    elif len(sys.argv) == 5 and sys.argv[1] == "merge":
        merge(*sys.argv[2:])
    else:
        sys.exit(__doc__)
