"""Write tests/golden/reference_patch_targets.json from a checkout of the reference: for every file that
rust/reference-shim/reference-gpu.patch touches, its line count and the sha256 of the lines each hunk replaces, and the
number of `impl Shape for` in src/objects/shape.rs.  test_rust_binding.py::test_reference_patch_applies checks the patch
against it, so the test needs no copy of the reference.

    python tests/tools/make_patch_targets.py <reference checkout>
"""
import hashlib
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PATCH = os.path.join(ROOT, "rust", "reference-shim", "reference-gpu.patch")
OUT = os.path.join(ROOT, "tests", "golden", "reference_patch_targets.json")


def main(ref):
    files, src = {}, None
    for line in open(PATCH).read().splitlines():
        m = re.match(r"^\+\+\+ b/(\S+)", line)
        if m:
            src = open(os.path.join(ref, m.group(1))).read().splitlines(keepends=True)
            cur = files[m.group(1)] = {"lines": len(src), "hunks": []}
            continue
        m = re.match(r"^@@ -(\d+)(?:,(\d+))? \+", line)
        if m:
            start, n = int(m.group(1)), int(m.group(2) or 1)
            region = "".join(src[start - 1:start - 1 + n])
            cur["hunks"].append({"old_start": start, "old_lines": n, "sha256": hashlib.sha256(region.encode()).hexdigest()})
    shape = open(os.path.join(ref, "src", "objects", "shape.rs")).read()
    out = {"files": files, "shape_impls": len(re.findall(r"^impl Shape for", shape, flags=re.M))}
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1])
