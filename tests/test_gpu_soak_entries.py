"""Every entry of a context, interleaved on ONE long-lived context at changing sizes (tests/soak_cases.py), against fresh
contexts: whatever ran before a job -- a larger image in the same scratch buffers, another entry in the shared ones, another
object count in the BVH's caches --, the job returns the bits a context that never ran anything else returns for it."""
import time

import numpy as np
import pytest

import soak_cases as sc

pytestmark = pytest.mark.gpu
SEEDS = (2026, 7)


def _fresh_run(pt, job):
    ctx = pt.Context(0)
    try:
        return sc.run(pt, ctx, job)
    finally:
        ctx.close()


@pytest.fixture(scope="module")
def fresh(pt):
    """every distinct job as the first call of a context of its own -> {job: outputs}; computed once, never changed"""
    t0 = time.perf_counter()
    out = {job: _fresh_run(pt, job) for job in sc.jobs()}
    print(f"fresh references: {len(out)} jobs of {len(sc.KINDS)} kinds in {time.perf_counter() - t0:.2f} s")
    return out


def _describe(diffs):
    return ", ".join(f"plane {i}: {n}" + (" positions" if isinstance(n, int) else "") for i, n in diffs)


def test_two_fresh_contexts_agree_on_every_job(pt, fresh):
    """an entry two fresh contexts disagree on is not deterministic, and nothing below could hold for it"""
    bad = []
    for job, ref in fresh.items():
        diffs = sc.differences(_fresh_run(pt, job), ref)
        if diffs:
            bad.append(f"{job}: {_describe(diffs)}")
    assert not bad, "two fresh contexts differ:\n" + "\n".join(bad)


@pytest.fixture(scope="module")
def long_lived(pt):
    """the long-lived contexts, one per shuffle seed, with the first outputs of their jobs: {seed: (context, {job: (outputs,
    position, the job before)})}; a seed's halves run on the same one"""
    held = {}

    def get(seed):
        if seed not in held:
            held[seed] = (pt.Context(0), {})
        return held[seed]

    yield get
    for ctx, _ in held.values():
        ctx.close()


@pytest.mark.parametrize("half", (0, 1))
@pytest.mark.parametrize("seed", SEEDS)
def test_a_long_lived_context_gives_what_fresh_contexts_give(pt, fresh, long_lived, seed, half):
    """One context runs the whole order of its seed, in two halves (two cases, each near the older soak's time): every float
    plane is finite unless the entry's contract plants NaN there, a job's second run equals its first bit for bit, and every run
    equals the job's run on a fresh context bit for bit -- the assertion that matters: twice the same also holds for a job that
    is deterministically wrong behind a larger one.  A failure names the job, the job before it and the planes that differ."""
    order = sc.order(seed)
    n = len(order) // 2
    ctx, first = long_lived(seed)
    bad = []
    t0 = time.perf_counter()
    for pos in range(half * n, (half + 1) * n):
        job, before = order[pos], order[pos - 1] if pos else None
        out = sc.run(pt, ctx, job)
        for i, a in enumerate(out):
            if a.dtype.kind == "f" and i not in sc.NAN_PLANES.get(job.kind, ()):
                assert np.isfinite(a).all(), f"{job} (behind {before}): plane {i} is not finite at {int((~np.isfinite(a)).sum())} positions"
        if job in first:
            diffs = sc.differences(out, first[job][0])
            if diffs:
                bad.append(f"run {pos} of {job} (behind {before}) differs from its run {first[job][1]} (behind {first[job][2]}): {_describe(diffs)}")
        else:
            first[job] = (out, pos, before)
        diffs = sc.differences(out, fresh[job])
        if diffs:
            bad.append(f"run {pos} of {job} (behind {before}) differs from a fresh context: {_describe(diffs)}")
    print(f"seed {seed}, half {half}: {n} runs in {time.perf_counter() - t0:.2f} s; {len(first)} jobs seen")
    assert not bad, "\n".join(bad)
