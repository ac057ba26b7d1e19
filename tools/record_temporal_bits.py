#!/usr/bin/env python3
"""Records tests/golden/temporal_bits.json: SHA-256 digests of what the temporal entries return, per case and frame, for the
cases of tests/temporal_bits_cases.py, on device 0 of an MI355X.
    python tools/record_temporal_bits.py OUT.json COMMIT

Run it on a build of the commit whose bits are to be kept (COMMIT is recorded in the file); tests/test_gpu_temporal_bits.py
replays the cases on the current build.  So that a digest cannot pin a path that was never taken, the file is written only if
  the motion entry's last frame differs from the plain entry's on the same inputs (an object moved, ids gate),
  the alpha entry's differs from the motion entry's (the plane was used),
  the moving-camera chain's differs from the same films under the first camera (the reprojection ran),
  the gradient plane under the moved camera holds both NaN and finite entries."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main(out_path, commit):
    import numpy as np
    import pathtrace_amd as pt
    import temporal_bits_cases as B
    ctx = pt.Context(0)
    rec = {"recorded_at": commit, "cases": {}}
    for W, H in B.SIZES:
        got = {name: B.run(pt, ctx, name, W, H) for name in B.CASES}
        for name, frames in got.items():
            rec["cases"][B.key(name, W, H)] = B.digests(frames)

        def differ(a, b):
            return not np.array_equal(a[-1][0], b[-1][0])
        for cam in ("fixed", "moving"):
            assert differ(got["motion " + cam], B.run_motion(pt, ctx, W, H, cam == "moving", False, entry="plain")), (W, H, cam, "motion = plain")
            assert differ(got["alpha " + cam], got["motion " + cam]), (W, H, cam, "alpha = motion")
        assert differ(got["plain moving"], B.run_plain(pt, ctx, W, H, 3, False, 1, 51)), (W, H, "moving = fixed")
        plane = got["gradient camera"][0][0]
        assert np.isnan(plane).any() and np.isfinite(plane).any(), (W, H, "gradient plane")
    ctx.close()
    with open(out_path, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(f"{out_path}: {len(rec['cases'])} cases, {sum(len(v) for v in rec['cases'].values())} frames")


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    main(sys.argv[1], sys.argv[2])
