"""The object counts at which tests/test_gpu_bvh_build.py and tests/test_gpu_bvh_median.py pin the device-side builds past one
iteration of k_bvh_sort_scan and past a 32-bit sort key: no GPU.  The counts are chosen against the tile sizes of the kernels,
so the sizes are held to the source here, and every count to the code it is there to reach (bvh_median_cases.device_levels
restates the level loop of ptbvh::median_plan).  A retune of a tile size fails here and points at the counts, instead of the
GPU tests quietly falling back to one scan iteration or four passes."""
import os
import re

import pytest

import bvh_median_cases as mc

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pathtrace_amd", "csrc")

# count -> (sort tiles, scan iterations, index_bits, passes per level, longest gap, its chunks)
TABLE = {
    10000: (5, 1, 14, [4, 4, 4], 0, 0),                          # the largest count of the median file before these
    32768: (16, 1, 15, [4, 4, 5, 5], 0, 0),
    32769: (17, 2, 16, [4, 5, 5, 5, 5], 30720, 1),
    65537: (33, 3, 17, [5] * 6, 63488, 1),
    131073: (65, 5, 18, [5] * 7, 129024, 2),
    262145: (129, 9, 19, [5] * 6 + [6, 5], 260096, 4),
}


@pytest.mark.parametrize("name, header, value", [
    ("kSortTile", "pt_kernels.h", mc.K_SORT_TILE), ("kSortDigits", "pt_kernels.h", mc.K_SORT_DIGITS), ("kScanBlock", "pt_film_bvh.h", mc.K_SCAN_BLOCK),
    ("kMedianTile", "pt_bvh.h", mc.K_MEDIAN_TILE), ("kMedianChunk", "pt_bvh.h", mc.K_MEDIAN_CHUNK)])
def test_the_sizes_are_the_sources(name, header, value):
    with open(os.path.join(CSRC, header)) as f:
        found = re.findall(r"^\s*constexpr\s+uint32_t\s+%s\s*=\s*(\d+)u?\s*;" % name, f.read(), re.M)
    assert found == [str(value)], (name, header, found)


def test_the_scan_walks_four_words_per_thread():
    """scan_iterations() counts 4 * kScanBlock words per loop iteration: the loop's own stride"""
    with open(os.path.join(CSRC, "pt_film_bvh.h")) as f:
        assert re.search(r"for \(uint32_t base = 0; base < total; base \+= 4u \* kScanBlock\)", f.read())


def test_the_plan_tile_is_the_median_tile(pt):
    assert pt.bvh_median_plan(5)[1] == mc.K_MEDIAN_TILE


def test_the_count_lists_are_the_tables(pt):
    assert mc.MEDIAN_LARGE == [n for n in sorted(TABLE) if n > 10000] and mc.MEDIAN_ONCE == mc.MEDIAN_LARGE[-1]
    assert mc.MORTON_LARGE == mc.MEDIAN_LARGE[:3] and (mc.SCAN_FULL, mc.SCAN_CARRY) == (32768, 32769)


@pytest.mark.parametrize("n", sorted(TABLE))
def test_every_count_reaches_what_it_is_there_for(pt, n):
    tiles, iterations, bits, passes, gap, chunks = TABLE[n]
    levels = mc.device_levels(pt.bvh_median_plan(n)[0], n)
    assert (mc.sort_tiles(n), mc.scan_iterations(n), mc.index_bits(n)) == (tiles, iterations, bits)
    assert [lv["passes"] for lv in levels] == passes
    assert max(lv["longest_gap"] for lv in levels) == gap and max(lv["gap_chunks"] for lv in levels) == chunks
    for lv in levels:                                            # the groups: ascending from 0, numbered within `bits` bits
        starts = [g[0] for g in lv["groups"]]
        assert starts[0] == 0 and starts == sorted(set(starts)) and starts[-1] < n
        assert (1 << lv["bits"]) >= len(starts) and (lv["bits"] == 0 or (1 << (lv["bits"] - 1)) < len(starts))
        assert any(g[1] for g in lv["groups"])
    # what the count is there for
    if n == mc.SCAN_FULL:
        assert mc.sort_tiles(n) == 16 and mc.K_SORT_DIGITS * 16 == 4 * mc.K_SCAN_BLOCK          # one iteration, exactly full
    if n > mc.SCAN_FULL:
        assert -(-n // 2048) > 16 and iterations > 1                                            # the carry of k_bvh_sort_scan
        assert max(passes) > 4                                   # a key past 32 bits: sort_digit's high word
        assert len(set(p % 2 for p in passes)) == 2 or n > mc.SCAN_CARRY                        # 32769: odd and even pass counts
    if n == mc.SCAN_CARRY:
        assert (mc.K_SORT_DIGITS * tiles) % (4 * mc.K_SCAN_BLOCK) != 0                          # the last iteration is partial
    if n >= 131073:
        assert gap > mc.K_MEDIAN_CHUNK and chunks >= 2           # a gap cut into chunks; step and gap groups mixed
        assert any(len(set(g[1] for g in lv["groups"])) == 2 for lv in levels)
    if n == 262145:
        assert passes.count(6) == 1 and set(passes) == {5, 6}
    if n == 10000:
        assert max(passes) == 4 and iterations == 1              # (what the suite reached before)
