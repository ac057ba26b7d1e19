"""The Rust -sys crate (rust/pathtrace-amd-sys) is source only here -- no cargo/rustc in the image.
What can be checked without a compiler is that it declares exactly the header's ABI: every function with the
same argument count, every struct with the same fields in the same order and the same scalar types."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "pathtrace_amd.h")).read()
RUST = open(os.path.join(ROOT, "rust", "pathtrace-amd-sys", "src", "lib.rs")).read()

C2RUST = {"double": "f64", "float": "f32", "uint32_t": "u32", "uint64_t": "u64", "int32_t": "i32", "uint8_t": "u8", "int": "c_int"}


def _strip_comments(src):
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def _c_functions():
    out = {}
    for m in re.finditer(r"^(?:const\s+)?[a-z_0-9A-Z]+\*?\s+\**(pt_[a-z_]+)\(([^;]*?)\);", _strip_comments(HEADER), flags=re.M | re.S):
        args = m.group(2).strip()
        out[m.group(1)] = 0 if args in ("", "void") else len(args.split(","))
    return out


def _rust_functions():
    out = {}
    for m in re.finditer(r"pub fn (pt_[a-z_]+)\((.*?)\)\s*(?:->[^;]+)?;", RUST, flags=re.S):
        args = m.group(2).strip()
        out[m.group(1)] = 0 if not args else len([a for a in args.split(",") if a.strip()])
    return out


def test_every_header_function_is_declared_with_the_same_arity():
    c, r = _c_functions(), _rust_functions()
    assert len(c) >= 39 and "pt_render_pixels" in c and "pt_multi_render_device" in c and "pt_render_device" in c and "pt_debug_bvh_check" in c
    assert c == r


def _c_struct(name):
    body = re.search(r"typedef struct \{([^}]*)\} %s;" % name, _strip_comments(HEADER)).group(1)
    fields = []
    for decl in body.split(";"):
        decl = " ".join(decl.split())
        if not decl:
            continue
        m = re.match(r"(\w+)\s+(.*)", decl)
        for var in m.group(2).split(","):
            var = var.strip()
            am = re.match(r"(\w+)\[(\d+)\]", var)
            fields.append((am.group(1), "[%s; %s]" % (C2RUST[m.group(1)], am.group(2))) if am else (var, C2RUST[m.group(1)]))
    return fields


def _rust_struct(name):
    body = re.search(r"pub struct %s \{(.*?)\}" % name, RUST, flags=re.S).group(1)
    return [(m.group(1), m.group(2).strip()) for m in re.finditer(r"pub (\w+): ([^,]+),", body)]


def test_struct_fields_match_the_header():
    for name in ("PtCamera", "PtObject", "PtRenderParams", "PtTuning", "PtStats"):
        assert _c_struct(name) == _rust_struct(name), name


def test_constants_match_the_header():
    hdr = _strip_comments(HEADER)
    for m in re.finditer(r"(PT_(?:OK|ERR|SHAPE|MAT|INTEGRATOR|ACCEL)_?\w*)\s*=\s*(\d+)", hdr):
        assert re.search(r"pub const %s: \w+ = %s;" % (m.group(1), m.group(2)), RUST), m.group(1)
    assert re.search(r"#define PT_ABI_VERSION (\d+)", HEADER).group(1) == re.search(r"PT_ABI_VERSION: u32 = (\d+);", RUST).group(1)


def _patch_hunks(text):
    """unified diff -> {file: [(old_start, old_lines, pre-image text), ...]}; asserts every hunk's line counts."""
    out, cur, hunk = {}, None, None
    lines = text.splitlines()
    i = 0
    while i < len(lines):
        m = re.match(r"^\+\+\+ b/(\S+)", lines[i])
        h = re.match(r"^@@ -(\d+)(?:,(\d+))? \+(\d+)(?:,(\d+))? @@", lines[i])
        if m:
            cur = out.setdefault(m.group(1), [])
        elif h:
            old_n, new_n = int(h.group(2) or 1), int(h.group(4) or 1)
            pre, n_old, n_new = [], 0, 0
            i += 1
            while i < len(lines) and (n_old < old_n or n_new < new_n):
                tag, body = lines[i][:1], lines[i][1:]
                assert tag in (" ", "-", "+"), lines[i]
                if tag != "+":
                    pre.append(body + "\n")
                    n_old += 1
                if tag != "-":
                    n_new += 1
                i += 1
            assert (n_old, n_new) == (old_n, new_n), h.group(0)
            cur.append((int(h.group(1)), old_n, "".join(pre)))
            continue
        i += 1
    return out


def test_reference_patch_applies():
    """rust/reference-shim/reference-gpu.patch (describe() on the traits, Camera::to_pod, gpu::render in main) must
    apply to the reference's sources.  The reference is not part of this repository: tests/golden/reference_patch_targets.json
    records, per file the patch touches, its line count and the sha256 of the lines each hunk replaces (tests/tools/
    make_patch_targets.py), so every hunk must find exactly its pre-image at its own position -- no offset, no fuzz."""
    import hashlib
    import json
    targets = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_patch_targets.json")))
    patch = open(os.path.join(ROOT, "rust", "reference-shim", "reference-gpu.patch")).read()
    hunks = _patch_hunks(patch)
    touched = sorted(hunks)
    assert "src/main.rs" in touched and "src/objects/shape.rs" in touched and "src/objects/material.rs" in touched
    assert touched == sorted(targets["files"])
    for f in touched:
        want = targets["files"][f]
        assert [(s, n) for s, n, _ in hunks[f]] == [(h["old_start"], h["old_lines"]) for h in want["hunks"]], f
        end = 0
        for (start, n, pre), h in zip(hunks[f], want["hunks"]):
            assert start > end and start - 1 + n <= want["lines"], (f, start)       # in order, inside the file
            assert hashlib.sha256(pre.encode()).hexdigest() == h["sha256"], (f, start)
            end = start - 1 + n
    # every impl of the two traits in the reference gets a description (or the trait's default)
    assert patch.count("fn describe(&self) -> (u32, [f64; 9])") == targets["shape_impls"] + 1        # + the trait itself
    gpu_rs = open(os.path.join(ROOT, "rust", "reference-shim", "gpu.rs")).read()
    assert "unsafe" not in gpu_rs.replace("forbid(unsafe_code)", "").replace("`unsafe`", "")
