"""Conditions on the table and the order of the all-entries soak (tests/soak_cases.py), so that a later edit cannot hollow
tests/test_gpu_soak_entries.py out: every kind is there at three sizes, and the order puts small jobs behind large ones of every
kind they share a buffer with."""
import pytest

import soak_cases as sc

SEEDS = (2026, 7)                      # the shuffle seeds of tests/test_gpu_soak_entries.py


def test_every_required_kind_is_in_the_table_with_a_function():
    assert set(sc.REQUIRED) <= set(sc.KINDS) and len(sc.REQUIRED) == len(set(sc.REQUIRED)) == 38
    assert all(callable(f) for f in sc.KINDS.values())
    for group, kinds in sc.SHARING.items():
        assert set(kinds) <= set(sc.KINDS), group
    assert all(any(k in g for g in sc.SHARING.values()) for k in sc.KINDS)
    assert set(sc.NAN_PLANES) <= set(sc.KINDS)


def test_every_kind_has_a_small_a_middle_and_a_large_job():
    jobs = sc.jobs()
    assert len(jobs) == len(set(jobs)) == 3 * len(sc.KINDS) and len({j.seed for j in jobs}) == len(jobs)
    for kind in sc.KINDS:
        mine = [j for j in jobs if j.kind == kind]
        assert sorted(sc.size_class(j.W, j.H) for j in mine) == ["large", "middle", "small"], kind
    for j in jobs:
        assert j.W % 16 and j.H % 16 and 2 <= j.W <= 200 and 2 <= j.H <= 160, j
        cls = sc.size_class(j.W, j.H)
        assert max(j.W, j.H) <= 40 if cls == "small" else min(j.W, j.H) >= 120 if cls == "large" else max(j.W, j.H) > 64, j
    assert sc.MAX_SPP == 8 and len(set(sc.BVH_OBJECTS.values())) == 3


@pytest.mark.parametrize("seed", SEEDS)
def test_the_order_runs_small_jobs_behind_the_large_ones_they_share_buffers_with(seed):
    order = sc.order(seed)
    jobs = sc.jobs()
    assert sorted(order) == sorted(jobs * 2) and order == sc.order(seed)
    assert all(a != b for a, b in zip(order, order[1:]))                      # a job's two runs are never adjacent
    first_large = {}
    for pos, j in enumerate(order):
        if sc.size_class(j.W, j.H) == "large":
            first_large.setdefault(j.kind, pos)
    last_small = {j.kind: pos for pos, j in enumerate(order) if sc.size_class(j.W, j.H) == "small"}
    for kind in sc.KINDS:
        assert first_large[kind] < last_small[kind], kind
        for other in sc.sharers(kind):
            assert first_large[other] < last_small[kind], (kind, other)
        assert any(b.kind == kind and a.kind != kind for a, b in zip(order, order[1:])), kind


def test_the_two_orders_differ():
    assert sc.order(SEEDS[0]) != sc.order(SEEDS[1])


def test_bloom_kinds_take_and_leave_the_tail_kernel(pt):
    """6 levels end in k_bloom_tail at every size; 1 level is above the tail's 32 x 32 at the middle and large sizes"""
    for j in sc.jobs():
        if j.kind == "bloom_tail":
            levels, first_tail = pt.bloom_plan(j.W, j.H, 6)
            assert first_tail < len(levels), j
        if j.kind == "bloom_flat" and sc.size_class(j.W, j.H) != "small":
            levels, first_tail = pt.bloom_plan(j.W, j.H, 1)
            assert first_tail == len(levels) == 1, j


def test_differences_names_the_plane():
    import numpy as np
    a = (np.zeros((4, 3), np.float32), np.arange(5, dtype=np.uint32), np.array([np.nan], np.float64))
    b = (a[0].copy(), a[1].copy(), a[2].copy())
    assert sc.differences(a, b) == []
    b[0][1, 2] = -0.0                                                 # equal as numbers, not as bits
    b[1][3] = 9
    assert sc.differences(a, b) == [(0, 1), (1, 1)]
    assert sc.differences(a, b[:2]) == [(-1, "count")] and sc.differences(a, (a[0], a[1], a[2].astype(np.float32))) == [(2, "shape")]
