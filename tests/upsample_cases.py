"""Named inputs of feature-guided upsampling (pathtrace_amd/csrc/pt_upsample.h) where the rule can go wrong without
the five shape pairs of tests/upsample_ref.py noticing: size ratios that put full-size pixels exactly on the low lattice (a
bilinear weight of exactly 0: the tap is skipped), ratios far above 8 and barely above 1, one axis scaled, sizes around the 32 x 8
block; sigmas of 0 and up to FLT_MAX; films with NaN, infinities, 3e38, a denormal or negative values under chosen records;
low images of one class, albedo 0, depths across the f32 range, normals whose product underflows, any bit pattern in a field.

A case is (c f32[h,w,3], f f32[h,w,8], F f32[H,W,8]) with the sigma pairs it is run with; every array comes from the case's
name and seed alone.  tests/test_upsample_cases_cpu.py holds the table to the conditions that make it meaningful and
pt_upsample_host to the f64 restatement (tests/upsample_ref.py) on all of it; tests/test_gpu_upsample_cases.py holds the kernel to
the restatement and to pt_upsample_host.  About 43 000 pixels over the shape pairs, the largest image 130 x 129.

Families:
  crafted     ur.crafted_inputs on every shape pair, every sigma pair
  exact       normals +-(0,0,1) (a quarter flipped), depths in {1, 2, 4}, albedo in {0, 1/4, 1/2, 1}, the planted miss and emitter
              blocks, sigma_d = 0: every weight is exactly b_q or 0 (log2f(1) = 0, exp2f(0) = 1, exp2f(-1.4e10) = 0), so no
              transcendental decides a bit and host and device agree bit for bit
  poison      the crafted inputs with one of POISONS in the low film (i) under every non-surface record, (ii) under every
              non-miss record, (iii) at about 3 % of lone low pixels of any class
  degenerate  the low image all miss / all emitter / a checkerboard of the three classes; albedo 0 everywhere; depths times
              1e-30 and 1e30, denormal, negative; normals of length 1e-20; any bit pattern in one of the eight fields of about
              3 % of the low or of the full records (NaN and +-inf among them; in a normal field NaN and patterns below 1 in
              magnitude, the normal then shortened to length 1 where it is longer: the rule's precondition n . n_q <= 1)

The negative poison is -2^-20: demodulated it lies in [-1e-3, -1e-6] (the albedo floor), beside film values of 0.1 and above.
A pixel's value is then P - |N| with P the positive taps' part and |N| <= 1e-3; a relative error d of the f32 weights moves it
by d P, and max(|P - |N||, 1e-3) >= P / 2 wherever P > 2e-3: the measure (floor 1e-3) sees at most 2 d.  A negative value of the
film's own size among positive taps lets the sum cross 0 far above the floor, where the relative measure says nothing about
an f32 weight (tried: the film negated at the lone pixels, 1.8e-4 on the host).
"""
import functools
import zlib
from collections import namedtuple

import numpy as np

import upsample_ref as ur

BAR = 1e-4                                       # the bar of the filter parity tests, floor 1e-3 under the reference (ur.max_rel)
FLT_MAX = float(np.finfo(np.float32).max)
Case = namedtuple("Case", "name family full low c f F sigmas")

ODD_RATIO = [((7, 7), (3, 3)), ((16, 10), (6, 4)), ((97, 65), (33, 17)), ((101, 21), (21, 5))]
LATTICE = {((7, 7), (3, 3)): (2, 2), ((16, 10), (6, 4)): (5, 3), ((97, 65), (33, 17)): (32, 0), ((101, 21), (21, 5)): (20, 4)}    # columns, rows with X (Y) an integer
EXTREME = [((1025, 2), (2, 2)), ((2, 513), (2, 3)), ((300, 3), (3, 3))]
NEAR_ONE = [((66, 34), (65, 33))]
ONE_AXIS = [((67, 35), (34, 35)), ((67, 35), (67, 18))]
BLOCK = [((31, 7), (16, 4)), ((32, 8), (16, 4)), ((33, 9), (17, 5))]
SHAPES = ur.SHAPES + ODD_RATIO + EXTREME + NEAR_ONE + ONE_AXIS + BLOCK          # (W, H) / (w, h)

SIGMAS = [(128.0, 0.025), (0.0, 0.0), (0.0, 0.025), (128.0, 0.0), (3.0, 0.5), (1e4, 1e-6), (1e-3, 1e3), (FLT_MAX, 0.025), (128.0, FLT_MAX),
          (FLT_MAX, FLT_MAX)]                    # (sigma_n, sigma_d)
SIGMAS_EXACT = [(0.0, 0.0), (128.0, 0.0), (1e-3, 0.0), (FLT_MAX, 0.0)]
SIGMAS_FEW = [SIGMAS[k] for k in (0, 1, 4, 6, 9)]

POISONS = {"nan": np.nan, "pinf": np.inf, "ninf": -np.inf, "3e38": 3e38, "denormal": 1e-40, "negative": -2.0 ** -20}
HARD = ((67, 35), (34, 18))                     # the pair of the existing isolation test
SMALL = ((16, 10), (6, 4))                      # odd ratios 3 x 3: lattice columns and rows beside the poisoned taps


def _seed(name):
    return zlib.crc32(name.encode())


def _tag(full, low):
    return f"{full[0]}x{full[1]}_from_{low[0]}x{low[1]}"


def exact_inputs(seed, full, low):
    """The exact family: the crafted classes and film, the surface records from a palette that makes every weight b_q or 0."""
    c, f, F = ur.crafted_inputs(seed, full, low)
    rng = np.random.default_rng(seed + 1)

    def palette(feat):
        H, W = feat.shape[:2]
        surf = ur.classes(feat) == ur.SURFACE
        rec = np.zeros((H, W, 8), np.float32)
        rec[..., 0:3] = rng.choice(np.array([0.0, 0.25, 0.5, 1.0], np.float32), (H, W, 3))
        rec[..., 6] = np.where(rng.uniform(size=(H, W)) < 0.25, -1.0, 1.0)
        rec[..., 7] = rng.choice(np.array([1.0, 2.0, 4.0], np.float32), (H, W))
        out = feat.copy()
        out[surf] = rec[surf]
        return out

    f = palette(f)
    F = f.copy() if full == low else palette(F)
    return c, f, F


def poison_mask(f, mode, seed):
    """bool[h,w]: the low pixels whose film is poisoned -- (i) every non-surface record, (ii) every non-miss record, (iii) lone pixels"""
    cls = ur.classes(f)
    if mode == "i":
        return cls != ur.SURFACE
    if mode == "ii":
        return cls != ur.MISS
    return np.random.default_rng(seed).uniform(size=cls.shape) < 0.03


def poisoned(c, mask, value):
    out = c.copy()
    out[mask] = np.float32(value)
    return out


def _wild(rng, n, normal):
    """n f32 values of any bit pattern, the first ones NaN, +inf, -inf (a normal field: NaN, and patterns below 1 in magnitude)"""
    bits = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    if normal:                                                      # the exponent field at most 126: |v| < 1
        e = np.minimum((bits >> np.uint32(23)) & np.uint32(0x7F), np.uint32(126))
        bits = (bits & np.uint32(0x807FFFFF)) | (e << np.uint32(23))
    v = bits.view(np.float32).copy()
    special = [np.nan] if normal else [np.nan, np.inf, -np.inf]
    for k in range(min(n, 2 * len(special))):
        v[k] = special[k % len(special)]
    return v


def wild_field(feat, field, seed):
    """feat with any-bit-pattern values in `field` of about 3 % of its records, at least one of them NaN"""
    rng = np.random.default_rng(seed)
    out = feat.copy()
    H, W = out.shape[:2]
    hit = rng.uniform(size=(H, W)) < 0.03
    hit.flat[rng.integers(0, H * W)] = True
    plane = out[..., field]
    plane[hit] = rng.permutation(_wild(rng, int(hit.sum()), 4 <= field <= 6))
    if 4 <= field <= 6:                                             # keep |n| <= 1 (a NaN length compares false: left alone)
        n = out[..., 4:7].astype(np.float64)
        with np.errstate(invalid="ignore"):
            length = np.sqrt((n * n).sum(-1))
            long = hit & (length > 1.0)
        n[long] *= (0.999999 / length[long])[:, None]
        out[..., 4:7] = n
    return out


def _build():
    cases = []

    def add(name, family, pair, c, f, F, sigmas):
        arrs = [np.ascontiguousarray(a, np.float32) for a in (c, f, F)]
        cases.append(Case(name, family, pair[0], pair[1], *arrs, tuple(sigmas)))

    for pair in SHAPES:
        add("crafted_" + _tag(*pair), "crafted", pair, *ur.crafted_inputs(_seed("crafted" + _tag(*pair)), *pair), SIGMAS)
        add("exact_" + _tag(*pair), "exact", pair, *exact_inputs(_seed("exact" + _tag(*pair)), *pair), SIGMAS_EXACT)
    for pair in (HARD, SMALL):
        c, f, F = ur.crafted_inputs(5, *pair)
        for mode in ("i", "ii", "iii"):
            mask = poison_mask(f, mode, _seed("poison" + _tag(*pair)))
            for pname, value in POISONS.items():
                add(f"poison_{mode}_{pname}_" + _tag(*pair), "poison", pair, poisoned(c, mask, value), f, F, SIGMAS if pair == HARD else SIGMAS_FEW)
    pair = HARD
    c, f, F = ur.crafted_inputs(6, *pair)
    tag = _tag(*pair)
    miss = np.array([1, 1, 1, 0, 0, 0, 0, 0], np.float32)
    g = f.copy()
    g[...] = miss
    add("degenerate_low_all_miss_" + tag, "degenerate", pair, c, g, F, SIGMAS_FEW)
    g = f.copy()
    g[..., 0:4] = 1.0
    g[..., 7] = np.where(g[..., 7] == 0, 1.0, g[..., 7])
    add("degenerate_low_all_emitter_" + tag, "degenerate", pair, c, g, F, SIGMAS_FEW)
    g = f.copy()
    ys, xs = np.mgrid[0:g.shape[0], 0:g.shape[1]]
    k = (ys + xs) % 3
    g[..., 7] = np.where(g[..., 7] == 0, 1.0, g[..., 7])
    g[..., 3] = 0.0
    g[k == 0] = miss
    g[k == 1, 0:4] = 1.0
    add("degenerate_low_checker_" + tag, "degenerate", pair, c, g, F, SIGMAS)

    def both(name, change, sigmas=SIGMAS):
        g, G = f.copy(), F.copy()
        change(g), change(G)
        add(f"degenerate_{name}_" + tag, "degenerate", pair, c, g, G, sigmas)

    def scale_depth(s):
        def change(a):
            a[..., 7] *= np.float32(s)
        return change

    def albedo_zero(a):
        a[..., 0:3] = 0.0

    def depth_denormal(a):                                          # k x 2^-149, k in 1 .. 127, where there is a depth
        a[..., 7] = np.where(a[..., 7] != 0, (1 + (a[..., 7] * 1000).astype(np.uint32) % 127).astype(np.uint32).view(np.float32), 0.0)

    def short_normals(a):
        a[..., 4:7] *= np.float32(1e-20)

    both("albedo_zero", albedo_zero)
    both("depth_1e-30", scale_depth(1e-30))
    both("depth_1e30", scale_depth(1e30))
    both("depth_denormal", depth_denormal)
    both("depth_negative", scale_depth(-1.0))
    both("normals_1e-20", short_normals)
    names = ("albedo_r", "albedo_g", "albedo_b", "emitter", "normal_x", "normal_y", "normal_z", "depth")
    for field, fname in enumerate(names):
        s = _seed("wild" + fname)
        add(f"degenerate_wild_low_{fname}_" + tag, "degenerate", pair, c, wild_field(f, field, s), F, SIGMAS_FEW)
        add(f"degenerate_wild_full_{fname}_" + tag, "degenerate", pair, c, f, wild_field(F, field, s + 1), SIGMAS_FEW)
    return cases


CASES = _build()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
NAMES = [c.name for c in CASES]
FAMILIES = ("crafted", "exact", "poison", "degenerate")
RUNS = [(c.name, k) for c in CASES for k in range(len(c.sigmas))]


@functools.lru_cache(maxsize=None)
def reference(name, k):
    """(the f64 restatement of case `name` under its k-th sigma pair, its info), computed once (read-only)."""
    c = BY_NAME[name]
    ref, info = ur.upsample(c.c, c.f, c.F, *c.sigmas[k], info=True)
    ref.setflags(write=False)
    return ref, info


def nonfinite(ref):
    """What the rule makes NaN, +inf, -inf in the f32 output -> three bool arrays"""
    with np.errstate(over="ignore", invalid="ignore"):
        r = np.asarray(ref).astype(np.float32)
    return np.isnan(r), np.isposinf(r), np.isneginf(r)


def compare(got, ref):
    """got f32 against the restatement -> (the non-finite sets agree: NaN for NaN, inf for inf of the same sign; ur.max_rel over
    the other entries)"""
    nan, pinf, ninf = nonfinite(ref)
    same = np.array_equal(np.isnan(got), nan) and np.array_equal(np.isposinf(got), pinf) and np.array_equal(np.isneginf(got), ninf)
    ok = ~(nan | pinf | ninf) & np.isfinite(got)
    if not ok.any():
        return same, 0.0
    return same, ur.max_rel(np.asarray(got, np.float64)[ok], np.asarray(ref)[ok])


def same_bits(a, b):
    """f32 arrays agree bit for bit, a NaN equal to a NaN (its payload is no part of the rule)"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


def ulp_distance(a, b):
    """Largest distance in f32 ulp between the entries finite in both (0 when there are none)"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    ok = np.isfinite(a) & np.isfinite(b)
    if not ok.any():
        return 0

    def key(v):                                                     # the f32 values in order, as integers
        i = v.view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)

    return int(np.max(np.abs(key(a[ok]) - key(b[ok]))))


def predicted_nonfinite(info, mask):
    """bool[H,W]: the pixels that read a poisoned low pixel -- as the anchor or as a tap with w_q > 0 (rule 5); from the
    restatement's decisions alone, no arithmetic on the film"""
    hit = np.zeros(info["own"].shape, bool)
    flat = mask.ravel()
    for k in range(4):
        hit |= info["live"][k] & flat[info["index"][k]] & ((info["anchor"] == k) | info["summed"][k])
    return hit


def protected(case, info):
    """Family poison (i): the surface pixels with a surface tap -- no poisoned record is of their class"""
    return (ur.classes(case.F) == ur.SURFACE) & info["own"]
