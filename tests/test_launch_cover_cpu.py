"""The index plans of k_film_histogram and k_adaptive_select (tests/launch_cover.py) cover every pixel once, the sizes of the
new GPU tests run their loops past the first trip, and the sizes of the older tests never did."""
import numpy as np
import pytest

import launch_cover as lc
import tonemap_ref as tr

N_CUS = 256                                                   # MI355X
OLD_HIST_SHAPES = [(2, 2), (67, 35), (257, 3), (130, 129), (64, 48)]          # tests/test_gpu_tonemap.py before these tests
OLD_ADAPTIVE_SIZES = [(256, 256), (400, 400), (200, 200), (128, 128), (96, 80)]     # the largest adaptive images, the README's job


@pytest.mark.parametrize("n_pixels,n_cus", [(1, 256), (1023, 256), (1024, 256), (1025, 256), (16770, 256), (5000, 4), (4096 * 4, 4),
                                            (4096 * 4 + 1, 4), (4096 * 9 - 7, 4), (37 * 1024 + 5, 3), (393516, 256), (1031 * 1021, 256),
                                            (1031 * 1021, 304), (2 * 1048576 + 3, 256)])
def test_histogram_plan_reads_every_pixel_once(n_pixels, n_cus):
    wg, trip, slot, tid, p = lc.hist_plan(n_pixels, n_cus)
    assert len(p) == n_pixels and np.array_equal(np.sort(p), np.arange(n_pixels))
    assert wg.max() < lc.hist_grid(n_pixels, n_cus) <= n_cus and slot.max() < lc.HIST_BATCH and tid.max() < lc.HIST_BLOCK
    # the closed form of the plan: the trip, slot and workgroup of pixel p
    stride = lc.hist_grid(n_pixels, n_cus) * lc.HIST_BLOCK
    r = p % (lc.HIST_BATCH * stride)
    assert np.array_equal(trip, p // (lc.HIST_BATCH * stride)) and np.array_equal(slot, r // stride)
    assert np.array_equal(wg, r % stride // lc.HIST_BLOCK) and np.array_equal(tid, r % lc.HIST_BLOCK)


@pytest.mark.parametrize("n_cus", [256, 304, 128, 64])
def test_the_new_histogram_sizes_reach_every_slot_and_a_second_trip(n_cus):
    (w1, h1), (w2, h2) = lc.hist_sizes(n_cus)
    stride = n_cus * lc.HIST_BLOCK
    assert stride < w1 * h1 < 2 * stride
    assert w2 * h2 > 4 * stride and (w2 * h2) % 1024 != 0 and w2 % 64 != 0
    mid, big = lc.hist_reach(w1 * h1, n_cus), lc.hist_reach(w2 * h2, n_cus)
    assert mid["grid"] == n_cus and mid["max_slot"] >= 1 and mid["trips"] == 1
    assert big["grid"] == n_cus and big["max_slot"] == 3 and big["trips"] == 2 and 0.0 < big["last_trip_fill"] < 1.0
    # the last trip's last workgroup is itself partly filled
    wg, trip, slot, tid, p = lc.hist_plan(w2 * h2, n_cus)
    last = (trip == 1) & (wg == wg[trip == 1].max())
    assert 0 < last.sum() < lc.HIST_BLOCK and slot[trip == 1].max() == 0
    if n_cus == N_CUS:
        assert (w2, h2) == (1031, 1021) and (w1, h1) == (643, 612)


def test_the_older_histogram_sizes_stay_in_slot_zero_of_the_first_trip():
    for W, H in OLD_HIST_SHAPES:
        r = lc.hist_reach(W * H, N_CUS)
        assert r["max_slot"] == 0 and r["trips"] == 1 and r["grid"] <= 17, (W, H, r)


def test_select_offsets_are_the_exclusive_prefix_sum():
    rng = np.random.default_rng(5)
    for n_wg in (1, 2, 255, 256, 257, 258, 265, 513, 700):
        counts = rng.integers(0, lc.SELECT_TILE + 1, n_wg)
        want = np.concatenate([[0], np.cumsum(counts)[:-1]])
        assert np.array_equal(lc.select_offsets(counts), want), n_wg


def test_the_new_adaptive_size_makes_a_second_offset_trip_and_the_older_ones_do_not():
    W, H = lc.ADAPTIVE_SIZE
    trips = lc.select_trips(W * H)
    assert len(trips) == 265 and trips.max() == 2 and (trips == 2).sum() == 8 and trips[257] == 2 and trips[256] == 1
    # every row from 505 on has slots in workgroups 256 and above; from 507 on all of a row's slots make the second trip
    assert 505 * W >= 256 * lc.SELECT_TILE > 504 * W
    assert lc.select_first_row_of_workgroup(257, W) == 507 < H
    for w, h in OLD_ADAPTIVE_SIZES:
        assert lc.select_trips(w * h).max() <= 1, (w, h)
    assert lc.select_trips(512 * 512).max() == 1 and lc.select_trips(513 * 513).max() == 2


@pytest.mark.parametrize("seed", [0, 1])
def test_margin_unsafe_share_of_the_large_curve_film(seed):
    """tests/test_gpu_tonemap.py compares RGBA8 exactly on the margin-safe pixels: the restatement alone keeps the others under
    2 % at the large size too"""
    _, (W, H) = lc.hist_sizes(N_CUS)
    film = tr.curve_film(W, H, seed)
    over = tr.random_params(seed) if seed else {}
    E = np.float32(2.0 ** tr.target(tr.histogram(film), tr.params(**over)))
    for curve, transfer in ((tr.ACES, tr.SQRT), (tr.REINHARD, tr.SRGB)):
        p = tr.params(curve=curve, transfer=transfer, **over)
        _, safe = tr.rgba8(tr.curve(film, E, p), p)
        assert (~safe).mean() <= 0.02, (curve, transfer, (~safe).mean())
