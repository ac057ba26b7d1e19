"""The index plans of the two film kernels whose loops depend on the image size, restated in numpy from the kernels' text
(csrc/pt_film_tonemap.h, csrc/pt_film_adaptive.h), and the image sizes the GPU tests take to run those loops past their first
trip.  No GPU, no library."""
import numpy as np

HIST_BLOCK, HIST_BATCH = 1024, 4         # kHistBlock, kHistBatch
BLOCK, SELECT_TILE = 256, 1024           # kBlock, kSelectTile


# ---- k_film_histogram: the grid is min(ceil(np / 1024), n_cus) workgroups of 1024; a workgroup's trip t starts at
# base = wg * 1024 + t * 4 * stride, stride = grid * 1024, and runs while base < np; slot k of thread tid reads pixel
# base + k * stride + tid when that is < np
def hist_grid(n_pixels, n_cus):
    return min((n_pixels + HIST_BLOCK - 1) // HIST_BLOCK, n_cus)


def hist_plan(n_pixels, n_cus):
    """every read of the launch -> int64 arrays (workgroup, trip, slot, thread, pixel), one entry per read"""
    grid = hist_grid(n_pixels, n_cus)
    stride = grid * HIST_BLOCK
    out = []
    for wg in range(grid):
        trip = 0
        base = wg * HIST_BLOCK
        while base < n_pixels:
            k, tid = np.meshgrid(np.arange(HIST_BATCH, dtype=np.int64), np.arange(HIST_BLOCK, dtype=np.int64), indexing="ij")
            p = base + k * stride + tid
            have = p < n_pixels
            n = int(have.sum())
            out.append(np.stack([np.full(n, wg, dtype=np.int64), np.full(n, trip, dtype=np.int64), k[have], tid[have], p[have]]))
            base += HIST_BATCH * stride
            trip += 1
    return tuple(np.concatenate(out, axis=1)) if out else tuple(np.zeros((5, 0), dtype=np.int64))


def hist_reach(n_pixels, n_cus):
    """-> dict: grid, the highest slot any read uses, the trips of the launch, and the reads of its last trip as a share of a
    full trip (4 * grid * 1024 reads)"""
    wg, trip, slot, _, _ = hist_plan(n_pixels, n_cus)
    grid = hist_grid(n_pixels, n_cus)
    trips = int(trip.max()) + 1
    return dict(grid=grid, max_slot=int(slot.max()), trips=trips,
                last_trip_fill=float((trip == trips - 1).sum()) / (HIST_BATCH * grid * HIST_BLOCK))


def hist_sizes(n_cus):
    """The two films of the histogram tests on a device of n_cus compute units -> ((W, H), (W, H)): the first between one and
    two strides of pixels (slots 1 .. 3 come into use), the second past four strides (a second trip, a few workgroups long), its
    pixel count no multiple of 1024 and its width no multiple of 64.  256 compute units: 643 x 612 and 1031 x 1021."""
    stride = n_cus * HIST_BLOCK
    mid = (643, (3 * stride // 2 + 642) // 643)
    W = 1031
    H = 4 * stride // W + 4
    while (W * H) % HIST_BLOCK == 0:
        H += 1
    return mid, (W, H)


# ---- k_adaptive_select: workgroup b owns list slots b * 1024 ..; thread t adds block_counts[t], [t + 256], .. below b
def select_grid(n):
    return (n + SELECT_TILE - 1) // SELECT_TILE


def select_trips(n):
    """-> int64[workgroups]: the trips of the offset loop's longest-running thread (thread 0) in every workgroup"""
    b = np.arange(select_grid(n), dtype=np.int64)
    return (b + BLOCK - 1) // BLOCK


def select_offsets(block_counts):
    """The output offsets the loop forms, thread by thread, then summed as the wave and workgroup reductions do (integers: any
    order) -> int64[workgroups]; equal to the exclusive prefix sum of block_counts"""
    c = np.asarray(block_counts, dtype=np.int64)
    out = np.zeros(len(c), dtype=np.int64)
    for b in range(len(c)):
        part = np.zeros(BLOCK, dtype=np.int64)
        for t in range(min(BLOCK, b)):
            part[t] = c[t:b:BLOCK].sum()
        out[b] = part.sum()
    return out


def select_first_row_of_workgroup(wg, width):
    """the first image row that lies wholly in workgroups >= wg of the image-form select"""
    return -(-wg * SELECT_TILE // width)


ADAPTIVE_SIZE = (520, 520)               # 270 400 slots, 265 select workgroups: 257 .. 264 make a second offset trip
