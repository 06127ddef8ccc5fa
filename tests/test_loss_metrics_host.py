"""CPU-side pins of the training loss and the depth metrics (no GPU needed):

  1. what the REFERENCE returned (tests/golden/g16_loss_metrics.npz, recorded by tests/golden/make_golden_metrics.py from the
     reference's own utils.py / models/module.py) lies within the reference's own fp32 rounding of the float64 restatement
     (tests/loss_metrics_ref.py) -- so the restatement the GPU tests compare against IS the reference's function;
  2. the threshold metrics equal the recording bitwise;
  3. a numpy emulation of the block structure of csrc/metrics.hip lies within the kernels' derived bounds, and every mutant of it
     (a plausible bug each) is caught by those same checks -- so the checks the GPU tests apply can fail;
  4. the host-side pieces: the scalar sets, the average meter, the header / binding agreement.
"""
import os

import numpy as np
import pytest
import torch

import loss_metrics_ref as R

LOSS_CASES, METRIC_CASES = R.GOLDEN_LOSS_CASES, R.GOLDEN_METRIC_CASES

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g16_loss_metrics.npz")
U24 = R.U24


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("name", sorted(LOSS_CASES))
def test_reference_loss_is_the_restatement(golden, name):
    """l_i: the bound in use is 8 x 2^-24 = 3 x 2^-24 for the three roundings outside the sum (the fp32 term is shared with the
    restatement; the difference est - gt, the division, the result) plus an ALLOWANCE of 5 x 2^-24 for the reference's fp32
    summation.  The allowance is not a tight derivation: the summation's worst case for an unknown order, (n - 1) x 2^-24, is
    vacuous at these sizes and is not asserted; torch sums in a cascade whose error grows with the depth of its tree (a few
    levels at up to 3 x 10^5 terms), and 5 is room for that above the measured 2.2.  Total:
    three fp32 roundings per term (fl32(w_i), the product, the addition) over positive partial sums; gradients: 4 x 2^-24 per
    element (fl32(w), / count, x c, and the indexing's scatter is exact); masked gradients exactly 0.  Measured with the recorded
    reference values: l_i <= 2.2, total <= 1.6, gradients <= 3.0 units of 2^-24."""
    sizes, B, seed, empty, with_grad = LOSS_CASES[name]
    est, gt, mask = R.loss_case(sizes, B, seed, empty_output=empty)
    w = R.loss_weights(len(est))
    ref = R.loss_ref(est, gt, mask, w)
    got_l = golden[name + "_l"].astype(np.float64)
    assert np.array_equal(np.isnan(got_l), np.isnan(ref["q"]))
    ok = ~np.isnan(got_l)
    rel = np.abs(got_l - ref["q"])[ok] / np.abs(ref["q"][ok])
    print(f"{name}: l_i distance <= {rel.max() / U24:.2f} x 2^-24")
    assert rel.max() <= 8 * U24
    total = float(golden[name + "_total"])
    if np.isnan(ref["total"]):
        assert np.isnan(total)
    else:
        from_l = float(np.sum(np.asarray(w) * got_l))
        print(f"{name}: total distance {abs(total - from_l) / from_l / U24:.2f} x 2^-24")
        assert abs(total - from_l) <= 3 * len(est) * U24 * from_l
    if with_grad:
        want = R.loss_grad_ref(est, gt, mask, w, 1.0)
        got = np.split(golden[name + "_grad"].astype(np.float64), np.cumsum([e.size for e in est])[:-1])
        worst = 0.0
        for g, wt, m in zip(got, want, mask):
            v = m.reshape(-1) > 0.5
            wt = wt.reshape(-1)
            assert (g[~v] == 0).all()
            err = np.abs(g[v] - wt[v])
            assert (err <= 4 * U24 * np.abs(wt[v])).all()
            if err.size:
                worst = max(worst, float((err / np.abs(wt[v])).max() / U24))
        print(f"{name}: gradient distance <= {worst:.2f} x 2^-24")


@pytest.mark.parametrize("name", sorted(METRIC_CASES))
def test_reference_metrics_are_the_restatement(golden, name):
    """Thresholds: bitwise fl32(count / n) per image for B <= 2 (the fp32 mean of two values is exact up to the one rounding the
    restatement also makes).  Means: within one fp32 ulp (2^-23) of the float64 value for B <= 2 -- the reference sums in fp32 --
    and two for B = 3."""
    shape, seed, kw = METRIC_CASES[name]
    est, gt, valid = R.metrics_case(shape, seed, **kw)
    ref = R.metrics_ref(est, gt, valid, R.ALL_THRES, R.TEST_BANDS)
    T = len(R.ALL_THRES)
    got = np.concatenate([[golden[name + "_abs"]], golden[name + "_thres"], golden[name + "_bands"]]).astype(np.float32)
    want = ref["want"]
    assert np.array_equal(np.isnan(got), np.isnan(want)), (got, want)
    if shape[0] <= 2:
        assert np.array_equal(got[1:1 + T], want[1:1 + T].astype(np.float32), equal_nan=True)
    ok = ~np.isnan(want)
    tol = (2.0 ** -23 if shape[0] <= 2 else 2.0 ** -22) * np.abs(want[ok])
    assert (np.abs(got.astype(np.float64)[ok] - want[ok]) <= tol).all(), (got, want)


def _tensor_args(est, gt, valid, mask_u8):
    return est, gt, (valid.astype(np.uint8) if mask_u8 else valid.astype(np.float32))


EMU_METRIC_CASES = {
    "wave": ((1, 5, 7), 31, {}),
    "tail": ((1, 37, 50), 32, {}),
    "blocks": ((2, 50, 90), 33, {}),                     # 4500 per image: 3 workgroups, the last partial, a tail past 64
    "empty": ((3, 16, 24), 34, {"empty_image": 1}),
    "nan": ((2, 37, 50), 35, {"nan_valid": True}),
}


def _check_metrics(got, est, gt, valid, thr, bands):
    scalars, counts, sums = got
    ref = R.metrics_ref(est, gt, valid, thr, bands)
    assert np.array_equal(counts, ref["counts"]), "counts"
    T = len(thr)
    R.check_sums(sums, ref["sums"], np.concatenate([ref["counts"][:, :1], ref["counts"][:, 1 + T:]], axis=1), np.abs(ref["sums"]), "sums")
    R.check_scalars(scalars, ref["want"], "scalars")


@pytest.mark.parametrize("mask_u8", [True, False])
@pytest.mark.parametrize("name", sorted(EMU_METRIC_CASES))
def test_emulated_metrics_kernels_meet_the_bounds(name, mask_u8):
    shape, seed, kw = EMU_METRIC_CASES[name]
    est, gt, valid = R.metrics_case(shape, seed, **kw)
    for thr, bands in ((R.TRAIN_THRES, ()), (R.TEST_THRES, R.TEST_BANDS)):
        e, g, m = _tensor_args(est, gt, valid, mask_u8)
        _check_metrics(R.emulate_metrics(e, g, m, thr, bands, mask_u8=mask_u8), est, gt, valid, thr, bands)


# the check each mutant must fail, by the message of the assertion it trips
METRIC_MUTANT_FAILS = {"threshold_ge": "^counts", "band_exclusive": "^counts", "drop_last_block": "^counts", "drop_tail64": "^counts",
                       "mean_all_pixels": "^counts", "one_mean_over_batch": "^scalars: .* outside the bound", "mask_multiply": "^sums: NaN pattern"}
LOSS_MUTANT_FAILS = {"drop_last_block": "^loss: counts", "drop_tail64": "^loss: counts", "mean_all_pixels": "^loss: counts",
                     "mask_multiply": "^loss l_i: NaN pattern", "count_per_image": "^loss l_i: .* outside the bound",
                     "weights_reversed": "^loss: total", "bwd:quadratic_gradient": "^grad: output .* outside 2.5 x",
                     "bwd:mask_multiply": "^grad: output .* masked elements are not 0"}


@pytest.mark.parametrize("mutant", R.MUTANTS_METRICS)
def test_metrics_mutants_are_caught(mutant):
    shape, seed, kw = EMU_METRIC_CASES["blocks"]
    est, gt, valid = R.metrics_case(shape, seed, **kw)
    got = R.emulate_metrics(est, gt, valid.astype(np.uint8), R.TEST_THRES, R.TEST_BANDS, mask_u8=True, mutant=mutant)
    with pytest.raises(AssertionError, match=METRIC_MUTANT_FAILS[mutant]):
        _check_metrics(got, est, gt, valid, R.TEST_THRES, R.TEST_BANDS)


SMALL = [(5, 7), (11, 13), (21, 27), (43, 53)]


def _check_loss_all(est, gt, mask, w, fwd, grads, g):
    valid = [m > 0.5 for m in mask]
    ref = R.loss_ref(est, gt, valid, w)
    R.check_loss(fwd[0], fwd[1], fwd[2], ref, "loss")
    R.check_grads(grads, R.loss_grad_ref(est, gt, valid, w, g), valid, "grad")


@pytest.mark.parametrize("B,empty", [(1, None), (2, None), (2, 5)])
def test_emulated_loss_kernels_meet_the_bounds(B, empty):
    est, gt, mask = R.loss_case(SMALL, B, 41 + B, empty_output=empty)
    w = R.loss_weights(len(est))
    for g in (1.0, 0.37):
        fwd = R.emulate_loss(est, gt, mask, w)
        grads = R.emulate_loss_bwd(est, gt, mask, w, fwd[1], g)
        _check_loss_all(est, gt, mask, w, fwd, grads, g)
    if empty is not None:
        assert np.isnan(fwd[0][empty]) and (grads[empty] == 0).all()


@pytest.mark.parametrize("mutant", R.MUTANTS_LOSS + tuple("bwd:" + m for m in R.MUTANTS_LOSS_BWD))
def test_loss_mutants_are_caught(mutant):
    est, gt, mask = R.loss_case(SMALL, 2, 43)
    w = R.loss_weights(len(est))
    bwd = mutant.startswith("bwd:")
    fwd = R.emulate_loss(est, gt, mask, w, mutant=None if bwd else mutant)
    good = R.emulate_loss(est, gt, mask, w)
    grads = R.emulate_loss_bwd(est, gt, mask, w, good[1], 0.37, mutant=mutant[4:] if bwd else None)
    with pytest.raises(AssertionError, match=LOSS_MUTANT_FAILS[mutant]):
        _check_loss_all(est, gt, mask, w, fwd, grads, 0.37)


# ------------------------------------------------------------------------------------------------- host-side pieces
def test_scalar_sets_name_the_reference_dictionaries():
    from effi_mvs_plus_amd import metrics
    tr, te = metrics.TRAIN_SCALARS, metrics.TEST_SCALARS
    assert tr.thresholds == R.TRAIN_THRES and tr.bands == () and tr.keys == ("abs_depth_error", "thres2mm_error", "thres4mm_error",
                                                                             "thres8mm_error")
    assert te.thresholds == R.TEST_THRES and te.bands == R.TEST_BANDS
    assert te.keys == ("abs_depth_error", "thres2mm_error", "thres4mm_error", "thres8mm_error", "thres14mm_error", "thres20mm_error",
                       "thres2mm_abserror", "thres4mm_abserror", "thres8mm_abserror", "thres14mm_abserror", "thres20mm_abserror",
                       "thres>20mm_abserror")
    for s in (tr, te):
        assert len(s.keys) == 1 + len(s.thresholds) + len(s.bands)
    for name in ("Thres_metrics", "AbsDepthError_metrics", "depth_scalars", "DeviceAverageMeter"):
        assert name in metrics.__all__


def test_average_meter_mirrors_the_reference_meter():
    """utils.py:103-122 on a vector: sums of the updates divided by their number; values stay tensors until mean()."""
    from effi_mvs_plus_amd.metrics import DeviceAverageMeter
    m = DeviceAverageMeter(device="cpu")
    assert m.mean() == {}
    m.update({"loss": torch.tensor(1.5), "abs": torch.tensor(0.25, dtype=torch.float64), "time": 2.0})
    m.update({"loss": torch.tensor(2.5), "abs": torch.tensor(0.75), "time": 4.0})
    assert m.count == 2 and m.data.dtype == torch.float64
    assert m.mean() == {"loss": 2.0, "abs": 0.5, "time": 3.0}
    with pytest.raises(ValueError):
        m.update({"loss": torch.tensor(1.0)})
    with pytest.raises(NotImplementedError):
        m.update({"loss": "x", "abs": 1.0, "time": 1.0})
    k = DeviceAverageMeter(("a", "b", "c"), device="cpu")
    k.slots("b", 2).add_(torch.tensor([1.0, 3.0], dtype=torch.float64))
    k.tick()
    k.slots("b", 2).add_(torch.tensor([2.0, 3.0], dtype=torch.float64))
    k.tick()
    assert k.mean() == {"a": 0.0, "b": 1.5, "c": 3.0}


def test_entries_are_declared_and_bound():
    from effi_mvs_plus_amd import _lib
    names = {"effi_metrics_blocks", "effi_mvs_loss_f32", "effi_mvs_loss_bwd_f32", "effi_depth_metrics_f32"}
    assert names <= set(_lib.SIGNATURES) and names | {"effi_metrics_scratch_bytes"} <= set(_lib.declared_symbols())
    assert "effi_metrics_scratch_bytes" in _lib.NON_STATUS_SYMBOLS
    from effi_mvs_plus_amd import models, train_graph
    assert callable(models.mvs_loss_fused) and hasattr(train_graph, "GraphedTestStep")


def test_cpu_tensors_are_refused():
    """No eager fall-back: the metrics raise on CPU tensors instead of computing with torch."""
    from effi_mvs_plus_amd import metrics
    from effi_mvs_plus_amd._lib import EffiLibraryError
    est, gt, valid = (torch.from_numpy(a) for a in R.metrics_case((1, 5, 7), 1))
    with pytest.raises(EffiLibraryError):
        metrics.Thres_metrics(est, gt, valid, 2)
