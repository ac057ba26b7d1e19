"""The instance table of the launch log (pt_debug_path_instances) is the set of path kernels the library ships.

The path kernels are templates; the dispatch in pt_kernels_*.hip picks one instance per launch and the launch log records
which (include/pathtrace_amd.h).  tests/test_gpu_kernel_instances.py runs one job per table entry, so a kernel instance
that is compiled into the library but missing from the table would ship untested: this test lists the kernels of the
gfx950 code objects inside libpathtrace_amd.so and requires them to be the table, one to one."""
import os
import re
import shutil
import subprocess
from collections import Counter

import pytest

LLVM = "/opt/rocm/llvm/bin"
SYM = re.compile(r"\bFUNC\s+GLOBAL\s+\w+\s+\d+\s+void (ptk_(exact|fast)_impl)::(k_paths\w*<[^>]*>)\(ptk::BounceArgs\)$")


def _tool(name):
    p = os.path.join(LLVM, name)
    return p if os.path.exists(p) else shutil.which(name)


def _shipped_path_kernels(pt, tmp_path):
    objdump, readelf = _tool("llvm-objdump"), _tool("llvm-readelf")
    if not objdump or not readelf:
        pytest.fail("llvm-objdump / llvm-readelf not found (ROCm's LLVM is needed to read the code objects)")
    so = tmp_path / "lib.so"
    shutil.copy(pt._lib.LIB_PATH, so)
    # --offloading writes one file per bundle entry next to its (relative) input: run it in tmp_path
    subprocess.run([objdump, "--offloading", so.name], cwd=tmp_path, check=True, capture_output=True)
    objs = sorted(p for p in os.listdir(tmp_path) if p.endswith("gfx950"))
    assert len(objs) == 9, objs             # the kernel units: main, rays, split, BVH, each exact and fast, and film (fast only)
    found = []
    for o in objs:
        out = subprocess.run([readelf, "--syms", "--demangle", "-W", o], cwd=tmp_path, check=True, capture_output=True,
                             text=True).stdout
        here = set()                        # (a kernel is in both .dynsym and .symtab)
        for line in out.splitlines():
            m = SYM.search(line.strip())
            if m:
                here.add((m.group(2) == "exact", m.group(3)))
        found += sorted(here)
    return found


def test_instance_codes_decode_to_distinct_kernels(pt):
    table = pt.path_instances()
    assert len(table) == len(set(table)) == 96
    kernels = [(pt.path_instance(c)["exact"], pt.path_instance(c)["kernel"]) for c in table]
    assert len(set(kernels)) == len(kernels)
    fams = Counter(pt.path_instance(c)["family"] for c in table)
    assert fams == {"k_paths": 40, "k_paths_regen": 24, "k_paths_bvh": 24, "k_paths_regen_split": 8}, fams
    # the encoding: continuation (OVF) launches are queue forms only; pixel lists never take the split form
    for c in table:
        d = pt.path_instance(c)
        assert not (d["ovf"] and d["family"] in ("k_paths_regen", "k_paths_regen_split")), d
        assert not (d["list"] and d["family"] == "k_paths_regen_split"), d
        assert not (d["list"] and d["mats"] and d["family"] in ("k_paths", "k_paths_bvh")), d


def test_table_is_the_set_of_shipped_path_kernels(pt, tmp_path):
    shipped = _shipped_path_kernels(pt, tmp_path)
    assert shipped, "no k_paths* kernel symbols found in the code objects"
    dup = [k for k, n in Counter(shipped).items() if n > 1]
    assert not dup, f"kernels in more than one code object: {dup}"
    table = {(pt.path_instance(c)["exact"], pt.path_instance(c)["kernel"]) for c in pt.path_instances()}
    assert set(shipped) == table, (f"shipped but not in the table: {sorted(set(shipped) - table)}; "
                                   f"in the table but not shipped: {sorted(table - set(shipped))}")


def test_launch_log_needs_a_context(pt):
    import ctypes as C
    n = C.c_uint32(7)
    assert pt._lib.lib().pt_debug_launch_log(None, None, 0, C.byref(n)) != 0
    assert pt._lib.lib().pt_debug_path_instances(None, 4, C.byref(n)) != 0     # cap without a buffer
