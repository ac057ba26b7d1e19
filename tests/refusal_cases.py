"""What the refusal tables share (test_denoise_refusals_cpu.py, test_entry_refusals_cpu.py): the scratch the pointer arguments
point into, the cases of an entry's chain of checks, the call, and the reading and the recording of a table.

A table (tests/golden/*_refusals.json) holds, per entry, one line per answer: [return code, message, the cases that get it],
with {who} for the entry's own name.  A chain of checks is a list of steps; a step is one check: a list of (label, the
arguments that trip it).  Every entry of the list is a case of its own; the first stands for the step in the pair with the
step after it (the pair pins their order: the earlier one answers).  A dict as the value of a struct argument names the fields
that differ from the defaults.
"""
import ctypes as C
import json
import math

HUGE = {"width": 1 << 16, "height": 1 << 15}                   # 2^31 pixels
BAD_F = (("-1", -1.0), ("nan", math.nan), ("inf", math.inf))

_scratch = (C.c_char * (1 << 16))()
_base = C.addressof(_scratch) + (-C.addressof(_scratch)) % 16


def at(offset):
    """the address `offset` bytes into the 16-byte aligned, zeroed scratch: never read or written by a refused call"""
    return C.c_void_p(_base + offset)


def nulls(*names):
    return [(f"null {n}", {n: None}) for n in names]


def floats(arg, field, bad=BAD_F):
    return [(f"{field}={t}", {arg: {field: v}}) for t, v in bad]


def merge(a, b):
    out = dict(a)
    for k, v in b.items():
        assert not (isinstance(v, dict) and k in out and out[k] is None), "a field of a null struct"
        out[k] = {**out[k], **v} if isinstance(v, dict) and isinstance(out.get(k), dict) else v
    return out


def cases(steps):
    """-> [(label, overrides)]: every case of every step, then the pair of each step with the next"""
    out = [case for step in steps for case in step]
    out += [(f"{a[0][0]} + {b[0][0]}", merge(a[0][1], b[0][1])) for a, b in zip(steps, steps[1:])]
    return out


def call(pt, entry, args, structs, make):
    """-> [return code, message]; args in the entry's order, those named in structs built by make(pt, name, fields)"""
    lib = pt._lib.lib()
    held = [make(pt, n, v) if n in structs and v is not None else v for n, v in args.items()]
    rc = getattr(lib, entry)(*[C.byref(v) if isinstance(v, C.Structure) else v for v in held])
    return [rc, lib.pt_last_error().decode()]


def table_of(path, entry):
    """-> {label: [return code, message]} of one entry"""
    return {t: [rc, msg.replace("{who}", entry)] for rc, msg, labels in json.load(open(path))[entry] for t in labels}


def record(path, entries, cases_of, call_of):
    """Writes the table of what the loaded library answers: cases_of(entry) -> [(label, overrides)], call_of(entry, overrides)"""
    n, lines = 0, []
    for e in sorted(entries):
        answers = {}                                            # (code, message) -> labels, in the order of first appearance
        for t, o in cases_of(e):
            rc, msg = call_of(e, o)
            assert rc != 0, f"{e}: {t} was not refused"
            answers.setdefault((rc, msg.replace(e, "{who}")), []).append(t)
            n += 1
        lines.append(json.dumps(e) + ": [\n" + ",\n".join("  " + json.dumps([rc, msg, ts]) for (rc, msg), ts in answers.items()) + "\n ]")
    with open(path, "w") as f:
        f.write("{\n " + ",\n ".join(lines) + "\n}\n")
    print(n, "cases ->", path)
