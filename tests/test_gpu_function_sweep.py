"""The per-vertex device functions of pt_device.h -- bsdf_pdf, bsdf_pdf_sample, shape_sample and what they call -- swept
over material and light parameters (function_sweep_cases.py), through pt_debug_*, one object uploaded per cell.

  (a) exact arithmetic == the f32 oracle, bit for bit, on every row of every cell;
  (b) decisions (lobe side, failure tuple) against f64 in the decision-stable cells, both arithmetic modes;
  (c) f, pdf, wo against f64: per cell, the device's median and 99th-percentile error is at most
      max(today's bar, 4 x the f32 ORACLE's same quantile over the same rows) -- today's bar = 1e-4 (1e-3 Mirror) relative
      with the floor 1e-5 under the reference, 5e-5 absolute for directions;
  (d) shapes against f64 under the same rule; observer inside, at the centre, in a triangle's plane;
  (e) consequences of the rules that need no reference number.

What the oracle alone does on these cases, and why normal incidence on a general normal is left out of (b)-(d), is
tests/test_function_sweep_cpu.py.  Run with -s for the device / f32-oracle ratios per cell (docs/EXPERIMENTS.md,
"Device-function sweep")."""
import numpy as np
import pytest

import function_sweep_cases as fc

pytestmark = pytest.mark.gpu
FACTOR = 4.0
MODES = (1, 0)                      # exact_math


@pytest.fixture(scope="module")
def bsdf(pt, orc):
    return fc.bsdf_tables(pt, orc)


@pytest.fixture(scope="module")
def shapes(pt, orc):
    return fc.shape_tables(pt, orc)


@pytest.fixture(scope="module")
def dev_bsdf(pt, gpu_ctx, bsdf):
    """{cell: {("eval" | "sample", exact): float32 rows}}: every cell through the device once."""
    R = fc.rows()
    out = {}
    for name, t in bsdf.items():
        gpu_ctx.upload(pt.make_objects([t.cell.spec]))
        out[name] = {}
        for exact in MODES:
            out[name]["eval", exact] = gpu_ctx.debug_bsdf_eval(0, t.eval_in, exact_math=exact)
            out[name]["sample", exact] = gpu_ctx.debug_bsdf_sample(0, t.sample_in, R.words, exact_math=exact)
    return out


@pytest.fixture(scope="module")
def dev_shape(pt, gpu_ctx, shapes):
    out = {}
    for name, t in shapes.items():
        gpu_ctx.upload(pt.make_objects([t.cell.spec]))
        out[name] = {}
        for exact in MODES:
            out[name]["sampled", exact] = gpu_ctx.debug_shape_sample(0, t.cell.frm, r12=t.cell.r12, exact_math=exact)
            out[name]["target", exact] = gpu_ctx.debug_shape_sample(0, t.cell.frm, target=t.cell.target, exact_math=exact)
    return out


def _holds(dev_q, orc_q, bar):
    return dev_q <= max(bar, FACTOR * orc_q)


def _ratio(dev_q, orc_q):
    return dev_q / orc_q if orc_q > 0 else (0.0 if dev_q == 0 else float("inf"))


# ---------------------------------------------------------------- (a)
def test_exact_arithmetic_is_the_f32_oracle_bit_for_bit_on_every_material_cell(bsdf, dev_bsdf):
    bad = []
    for name, t in bsdf.items():
        for fn, ref in (("eval", t.ev32), ("sample", t.sm32)):
            got = dev_bsdf[name][fn, 1]
            same = (got == ref.astype(np.float32)) | (np.isnan(got) & np.isnan(ref))
            if not same.all():
                rows = np.flatnonzero(~same.all(1))
                bad.append((name, fn, len(rows), [fc.KIND_NAMES[k] for k in sorted(set(fc.rows().kind[rows]))], int(rows[0])))
    assert not bad, bad


def test_exact_arithmetic_is_the_f32_oracle_bit_for_bit_on_every_light_cell(shapes, dev_shape):
    bad = []
    for name, t in shapes.items():
        for form, ref in (("sampled", t.s32), ("target", t.t32)):
            # the with-target form produces the point and the pdf; direction and distance are the caller's
            cols = fc.DEVICE_COLUMNS if form == "sampled" else fc.DEVICE_COLUMNS[:4]
            got = dev_shape[name][form, 1][:, :len(cols)]
            if not np.array_equal(got, ref[:, cols].astype(np.float32), equal_nan=True):
                bad.append((name, form, int((got != ref[:, cols].astype(np.float32)).any(1).sum())))
    assert not bad, bad


# ---------------------------------------------------------------- (b)
def test_decisions_agree_with_f64_in_the_stable_cells(bsdf, dev_bsdf):
    R = fc.rows()
    bad = []
    for name, t in bsdf.items():
        if not t.stable:
            continue
        for exact in MODES:
            share = fc.same_decision(dev_bsdf[name]["sample", exact], t.sm64, R.nrm).mean()
            if share < t.share32 - 0.005:           # a coin flip within one f32 ulp of u may fall the other way
                bad.append((name, exact, share, t.share32))
    assert not bad, bad


# ---------------------------------------------------------------- (c)
def test_values_against_f64_within_four_times_the_f32_oracles_own_error(bsdf, dev_bsdf):
    R = fc.rows()
    inc = fc.included(R.kind)
    bad, worst = [], {}
    print(f"\n{'cell':48s} mode  device/f32-oracle: sample f,pdf med   p99 | wo med   p99 | eval med   p99     (device p99: sample, wo, eval)")
    for name, t in bsdf.items():
        if not t.stable:
            continue
        bar = 1e-3 if t.cell.tag == fc.MIRROR else 1e-4
        for exact in MODES:
            sm, ev = dev_bsdf[name]["sample", exact], dev_bsdf[name]["eval", exact]
            rows = t.finite64 & inc & t.agree32 & fc.same_decision(sm, t.sm64, R.nrm)
            checks = [("sample f,pdf", fc.rel_err(sm[rows][:, 3:7], t.sm64[rows][:, 3:7]), fc.rel_err(t.sm32[rows][:, 3:7], t.sm64[rows][:, 3:7]), bar),
                      ("wo", fc.abs_err(sm[rows][:, 0:3], t.sm64[rows][:, 0:3]), fc.abs_err(t.sm32[rows][:, 0:3], t.sm64[rows][:, 0:3]), 5e-5),
                      ("eval f,pdf", fc.rel_err(ev[t.ev_finite64], t.ev64[t.ev_finite64]), fc.rel_err(t.ev32[t.ev_finite64], t.ev64[t.ev_finite64]), bar)]
            line, p99s = [], []
            for what, e_dev, e_orc, b in checks:
                qd, qo = fc.quantiles(e_dev), fc.quantiles(e_orc)
                for k, q in enumerate(("median", "p99")):
                    r = _ratio(qd[k], qo[k])
                    line.append(r)
                    if qd[k] > b:                   # below today's bar the ratio is of two rounding residues
                        worst[what, q, exact] = max(worst.get((what, q, exact), 0.0), r)
                    if not _holds(qd[k], qo[k], b):
                        bad.append((name, exact, what, q, qd[k], qo[k]))
                p99s.append(qd[1])
            print(f"{name:48s} {'exact' if exact else 'fast '} {line[0]:24.2f} {line[1]:5.2f} | {line[2]:5.2f} {line[3]:5.2f} | {line[4]:7.2f} {line[5]:5.2f}"
                  f"     {p99s[0]:.1e} {p99s[1]:.1e} {p99s[2]:.1e}")
    print("largest ratio among the quantiles above today's bar:", {k: round(v, 3) for k, v in sorted(worst.items())})
    assert not bad, bad


# ---------------------------------------------------------------- (d)
def test_light_samples_against_f64(shapes, dev_shape):
    bad = []
    print(f"\n{'cell':32s} mode   point/scale: device p99, max | f32 oracle p99, max | pdf ratio med p99 | with-target pdf ratio med p99 | dir ratio p99")
    for name, t in shapes.items():
        cell = t.cell
        fin = np.isfinite(t.s64).all(1)
        for exact in MODES:
            got = dev_shape[name]["sampled", exact].astype(np.float64)
            got_t = dev_shape[name]["target", exact].astype(np.float64)
            # with-target form: no draw, every row
            qd, qo = fc.quantiles(fc.rel_err(got_t[:, 3:4], t.t64[:, 6:7])), fc.quantiles(fc.rel_err(t.t32[:, 6:7], t.t64[:, 6:7]))
            rt = [_ratio(qd[k], qo[k]) for k in (0, 1)]
            for k in (0, 1):
                if not _holds(qd[k], qo[k], 1e-4):
                    bad.append((name, exact, "with-target pdf", k, qd[k], qo[k]))
            assert np.array_equal(got_t[:, 0:3], cell.target), (name, exact)            # the point is handed back
            if not fin.any():
                print(f"{name:32s} {'exact' if exact else 'fast '}  (sampled form: not finite in f64)   with-target pdf ratio {rt[0]:.2f} {rt[1]:.2f}")
                continue
            qd, qo = fc.quantiles(fc.rel_err(got[fin][:, 3:4], t.s64[fin][:, 6:7])), fc.quantiles(fc.rel_err(t.s32[fin][:, 6:7], t.s64[fin][:, 6:7]))
            rp = [_ratio(qd[k], qo[k]) for k in (0, 1)]
            for k in (0, 1):
                if not _holds(qd[k], qo[k], 1e-4):
                    bad.append((name, exact, "pdf", k, qd[k], qo[k]))
            # the point, in units of the radius / the longest edge: bulk and worst case
            dp = fc.abs_err(got[fin][:, 0:3], t.s64[fin][:, 0:3]) / cell.scale
            dp32 = fc.abs_err(t.s32[fin][:, 0:3], t.s64[fin][:, 0:3]) / cell.scale
            bar = max(5e-5, FACTOR * fc.quantiles(dp32)[1])
            if not (np.mean(dp <= bar) >= 0.95 and dp.max() <= max(bar, FACTOR * dp32.max())):
                bad.append((name, exact, "point", float(np.mean(dp <= bar)), float(dp.max()), bar, float(dp32.max())))
            dd, dd32 = fc.abs_err(got[fin][:, 4:7], t.s64[fin][:, 7:10]), fc.abs_err(t.s32[fin][:, 7:10], t.s64[fin][:, 7:10])
            qd, qo = fc.quantiles(dd), fc.quantiles(dd32)
            for k in (0, 1):
                if not _holds(qd[k], qo[k], 5e-5):
                    bad.append((name, exact, "direction", k, qd[k], qo[k]))
            print(f"{name:32s} {'exact' if exact else 'fast '} {fc.quantiles(dp)[1]:9.1e} {dp.max():9.1e} | {fc.quantiles(dp32)[1]:9.1e} {dp32.max():9.1e} | "
                  f"{rp[0]:5.2f} {rp[1]:5.2f} | {rt[0]:5.2f} {rt[1]:5.2f} | {_ratio(qd[1], qo[1]):5.2f}")
    assert not bad, bad


def test_observer_inside_a_sphere_light(shapes, dev_shape):
    """shape.rs:139-144: the reference returns (point - from).normalize() and its length.  The near root is negative for an
    observer inside; the device flips direction and sign, so distance > 0 and point = from + dir * dist still holds."""
    for name, t in shapes.items():
        if t.cell.key["where"] != fc.INSIDE:
            continue
        r = t.cell.key["radius"]
        for exact in MODES:
            got = dev_shape[name]["sampled", exact].astype(np.float64)
            assert (got[:, 7] > 0).all(), (name, exact)
            assert np.abs(got[:, 0:3] - (t.cell.frm + got[:, 4:7] * got[:, 7:8])).max() <= 1e-5 * r, (name, exact)
            assert ((got[:, 4:7] * t.s64[:, 7:10]).sum(1) > 0.999).all(), (name, exact)          # the flipped direction is f64's
            assert np.allclose(got[:, 7], t.s64[:, 10], rtol=1e-4), (name, exact)
            assert np.abs(np.linalg.norm(got[:, 0:3] - fc.SPHERE_CENTRE, axis=1) / r - 1).max() <= 1e-4, (name, exact)   # a point OF the light


def test_observer_in_a_triangles_plane_gets_the_safety_pdf(shapes, dev_shape):
    """shape.rs:235-239: pdf_omega = 1e-8 when cos_light <= 1e-8 -- also for d = 0, where cos_light is NaN (exact arithmetic)
    or 0 (fast arithmetic: the zero vector stays zero)."""
    tiny = np.float32(1e-8)
    seen = 0
    for name, t in shapes.items():
        if t.cell.spec[0] != fc.TRIANGLE:
            continue
        for form, ref in (("sampled", t.s32), ("target", t.t32)):
            says = ref[:, 6].astype(np.float32) == tiny
            seen += int(says.sum())
            if t.cell.key["where"] == fc.IN_PLANE:
                assert says.all(), name
            for exact in MODES:
                assert (dev_shape[name][form, exact][says, 3] == tiny).all(), (name, form, exact)
    assert seen >= 4 * 2 * (64 + 12)


# ---------------------------------------------------------------- (e)
@pytest.mark.parametrize("albedo", fc.ALBEDO)
def test_oren_nayar_with_sigma_zero_is_lambert_bit_for_bit(pt, gpu_ctx, albedo):
    """sigma = 0: A = 1, B = 0 (material.rs:183-186), term = 1 + 0 * x."""
    R = fc.rows()
    gpu_ctx.upload(pt.make_objects([fc.lambert_cell(list(albedo)).spec, (fc.SPHERE, [3, 0, 0, 1], fc.OREN_NAYAR, list(albedo) + [0.0])]))
    for exact in MODES:
        lam, on = gpu_ctx.debug_bsdf_eval(0, R.eval_in(), exact_math=exact), gpu_ctx.debug_bsdf_eval(1, R.eval_in(), exact_math=exact)
        assert np.isfinite(lam).all() and np.array_equal(lam, on), exact
        lam, on = (gpu_ctx.debug_bsdf_sample(k, R.sample_in(), R.words, exact_math=exact) for k in (0, 1))
        assert np.isfinite(lam).all() and np.array_equal(lam, on), exact


def test_cosine_sampled_direction_does_not_depend_on_the_material(bsdf, dev_bsdf):
    R = fc.rows()
    for exact in MODES:
        wo = dev_bsdf[fc.lambert_cell().name]["sample", exact][:, 0:3]
        assert np.isfinite(wo).all() and (np.abs(np.linalg.norm(wo.astype(np.float64), axis=1) - 1) <= 1e-6).all()
        for name, t in bsdf.items():
            if t.cell.tag == fc.OREN_NAYAR:
                assert np.array_equal(dev_bsdf[name]["sample", exact][:, 0:3], wo), (name, exact)
        assert np.array_equal(dev_bsdf["emissive"]["sample", exact][:, 0:3], R.nrm.astype(np.float32))     # material.rs:150-158


def test_metallic_above_the_threshold_never_refracts_and_at_it_flips_the_coin(bsdf, dev_bsdf):
    """`metallic > 0.99` (mirror.rs:184, :226): 1.0 and the f32 next above 0.99 take the same branches; 0.99 itself does not."""
    R = fc.rows()
    refracting_cells = 0
    for r in fc.ROUGHNESS:
        for ior in fc.IOR:
            cell = {m: f"ggx r={r:g} m={m} ior={ior:g}" for m in ("1", "0.99+", "0.99")}
            for exact in MODES:
                one, above = (dev_bsdf[cell[m]]["sample", exact] for m in ("1", "0.99+"))
                assert np.array_equal(fc.failed(one, R.nrm), fc.failed(above, R.nrm)), (r, ior, exact)
                assert np.array_equal(fc.side(one, R.nrm), fc.side(above, R.nrm)) and (fc.side(above, R.nrm) >= 0).all(), (r, ior, exact)
                ev1, eva = (dev_bsdf[cell[m]]["eval", exact] for m in ("1", "0.99+"))
                below = ((-R.din * R.nrm).sum(1) > 1e-3) & ((R.wo * R.nrm).sum(1) < -1e-3)      # clear of the f32 rounding of either cosine
                assert (eva[below, 0:3] == 0).all() and (eva[below, 3] == 1).all() and (ev1[below, 3] == 1).all(), (r, ior, exact)
            t = bsdf[cell["0.99"]]
            if not t.stable or r == 0.0:
                continue
            refr64 = ~fc.failed(t.sm64, R.nrm) & (fc.side(t.sm64, R.nrm) < 0)
            refr32 = ~fc.failed(t.sm32, R.nrm) & (fc.side(t.sm32, R.nrm) < 0)
            assert refr64.sum() > 0, cell["0.99"]                      # the Fresnel coin is flipped, and falls on "transmit"
            refracting_cells += 1
            both = refr64 & refr32
            for exact in MODES:
                got = dev_bsdf[cell["0.99"]]["sample", exact]
                refr = ~fc.failed(got, R.nrm) & (fc.side(got, R.nrm) < 0)
                assert refr[both].mean() >= 0.995, (cell["0.99"], exact, refr[both].mean())
    assert refracting_cells >= 9
