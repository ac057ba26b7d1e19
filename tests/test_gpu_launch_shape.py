"""What the recorded jobs launch on the device (tests/golden/launch_counts.json, recorded at commit daf88e4 by
tools/record_launch_counts.py): small renders either side of every threshold of the launch sizing -- four batches in the
queue form, 2^17 and 2^22 paths from both sides, the split form, 129 objects, the BVH, an adaptive render's pixel lists.
The statistics of pt_get_stats and the launch log of each must be the recorded ones: the sizing (csrc/pt_shape.h) decides
how many launches a render makes and which kernel instance each one takes."""
import json
import os

import pytest

from tests import launch_shape_jobs as J

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_counts.json")


@pytest.fixture(scope="module")
def recorded():
    return json.load(open(GOLDEN))


@pytest.mark.parametrize("name", list(J.JOBS))
def test_job_launches_what_was_recorded(pt, gpu_ctx, recorded, name):
    want = recorded["jobs"][name]
    got = J.run(pt, gpu_ctx, name)
    for k in ("bounce_launches", "batches", "primary_launches", "launch_log"):
        assert got[k] == want[k], (k, got[k], want[k])
    assert len(want["launch_log"]) == want["bounce_launches"] == sum("k_paths" in d[0] for d in want["dispatches"])
