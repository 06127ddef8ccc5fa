"""GPU: the DTU evaluation on the device (effi_mvs_plus_amd/dtu_eval.py on csrc/dtu_eval.hip) against the CPU restatement of the
reference's MATLAB files (tests/dtu_eval_ref.py: numpy fp64 + cKDTree candidates, the squared distance in the stated order).

The bar is BITWISE (torch.equal) for every mask, every kept set and every squared distance: both sides make the same fp64 decisions
on the same fp32 coordinates, a minimum does not depend on the visiting order, and the generators keep every pair distance at least
1e-12 (relative) away from dst, so no rounding can flip a neighbour test.  Only the statistics carry a tolerance (test E1).
"""
import numpy as np
import pytest
import torch

import dtu_eval_ref as R
from common import t
from effi_mvs_plus_amd import synth

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DST = 0.2


def _randperm(n, seed):
    return torch.randperm(n, generator=torch.Generator().manual_seed(seed))


@pytest.fixture(scope="module")
def patch():
    """R1's cloud, its neighbour lists and the reference sets for seeds 0-2 and the index order: computed once, never modified."""
    xyz = R.noisy_patch(20000, 0)
    adj = R.adjacency(xyz, DST)
    print(f"[dtu eval] R1: {len(adj[1]) / len(xyz):.1f} neighbours per point")
    orders = {s: _randperm(len(xyz), s).numpy() for s in range(3)}
    orders[None] = np.arange(len(xyz))
    want = {k: R.reduce_sequential(xyz, DST, o, adj=adj) for k, o in orders.items()}
    return {"xyz": xyz, "dev": t(torch.from_numpy(xyz), DEV), "orders": orders, "want": want}


# ---- R1 -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2, None])
def test_r1_dense_patch_equals_the_sequential_loop(patch, seed):
    from effi_mvs_plus_amd import dtu_eval
    keep, rounds = dtu_eval.reduce_points(patch["dev"], DST, seed=seed)
    want = patch["want"][seed]
    print(f"[dtu eval] R1 seed {seed}: {rounds} rounds, keeps {int(keep.sum())} of {len(want)} (reference {int(want.sum())})")
    assert keep.dtype == torch.bool and torch.equal(keep.cpu(), torch.from_numpy(want))
    assert rounds >= 3
    assert rounds == R.reduce_rounds(patch["xyz"], DST, patch["orders"][seed])[1]
    if seed is not None:                                          # the same order given as a permutation tensor
        keep2, _ = dtu_eval.reduce_points(patch["dev"], DST, order=torch.from_numpy(patch["orders"][seed]))
        assert torch.equal(keep2, keep)


# ---- R2 -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reverse", [False, True])
def test_r2_collinear_chain_takes_one_round_per_point(reverse):
    from effi_mvs_plus_amd import dtu_eval
    xyz = R.collinear(300, 0.15)
    order = np.arange(300)[::-1].copy() if reverse else np.arange(300)
    keep, rounds = dtu_eval.reduce_points(t(torch.from_numpy(xyz), DEV), DST, order=torch.from_numpy(order))
    want, want_rounds = R.reduce_rounds(xyz, DST, order)
    assert np.array_equal(want, R.reduce_sequential(xyz, DST, order))
    assert torch.equal(keep.cpu(), torch.from_numpy(want))
    assert rounds == want_rounds and rounds >= 290                # a round that read its own writes would finish in far fewer
    assert int(keep.sum()) == 150 and bool(keep[-1 if reverse else 0])


# ---- R3 -----------------------------------------------------------------------------------------------------------------------
def test_r3_threshold_is_a_closed_interval():
    from effi_mvs_plus_amd import dtu_eval
    dst = 0.25
    cases = {"at dst": ([(0, 0, 0), (0.25, 0, 0)], True),
             "one fp32 step of 2^-20 past dst": ([(0, 0, 0), (0.25 + 2.0 ** -20, 0, 0)], False),
             "exact duplicates": ([(0.1, -0.3, 7.0), (0.1, -0.3, 7.0)], True),
             "diagonal cells": ([(0.2, 0.2, 0.2), (0.3, 0.3, 0.3)], True),
             "diagonal cells across zero": ([(-0.05, -0.05, -0.05), (0.05, 0.05, 0.05)], True),
             "diagonal cells, too far": ([(0.2, 0.2, 0.2), (0.4, 0.4, 0.4)], False),
             "at dst along z, negative side": ([(0, 0, -0.25), (0, 0, -0.5)], True)}
    for name, (pts, neighbours) in cases.items():
        xyz = np.array(pts, np.float32)
        if name.startswith(("at dst", "one fp32")):
            assert (xyz.astype(np.float64) == np.array(pts)).all(), name           # these coordinates are exact in fp32
        cell = np.floor(xyz.astype(np.float64) / (dst * (1 + 2.0 ** -20)))
        if "diagonal" in name:
            assert (cell[0] != cell[1]).all(), name
        for order in ([0, 1], [1, 0]):
            keep, _ = dtu_eval.reduce_points(t(torch.from_numpy(xyz), DEV), dst, order=torch.tensor(order))
            want = R.reduce_sequential(xyz, dst, np.array(order))
            assert list(want) == ([i == order[0] for i in range(2)] if neighbours else [True, True]), name
            assert torch.equal(keep.cpu(), torch.from_numpy(want)), (name, order)


# ---- R4 -----------------------------------------------------------------------------------------------------------------------
def test_r4_zero_one_and_two_points():
    from effi_mvs_plus_amd import dtu_eval
    keep, rounds = dtu_eval.reduce_points(torch.zeros(0, 3, device=DEV), DST)
    assert keep.shape == (0,) and keep.dtype == torch.bool and keep.device.type == "cuda" and rounds == 0
    keep, rounds = dtu_eval.reduce_points(torch.tensor([[1.0, -2.0, 3.0]], device=DEV), DST, seed=4)
    assert keep.tolist() == [True] and rounds == 1
    keep, rounds = dtu_eval.reduce_points(torch.tensor([[0.0, 0, 0], [0.1, 0, 0]], device=DEV), DST, order=torch.tensor([1, 0]))
    assert keep.tolist() == [False, True] and rounds == 2
    keep, rounds = dtu_eval.reduce_points(torch.tensor([[0.0, 0, 0], [500.0, -300.0, 20.0]], device=DEV), DST)
    assert keep.tolist() == [True, True] and rounds == 1
    with pytest.raises(ValueError):
        dtu_eval.reduce_points(torch.zeros(3, 3, device=DEV), DST, order=torch.tensor([0, 1, 1]))
    with pytest.raises(ValueError):
        dtu_eval.reduce_points(torch.zeros(3, 3, device=DEV), DST, order=torch.tensor([0, 1, 3]))
    with pytest.raises(ValueError):
        dtu_eval.reduce_points(torch.zeros(3, 3, device=DEV), DST, cell=0.2)       # below dst * (1 + 2^-20)


# ---- R5 -----------------------------------------------------------------------------------------------------------------------
def test_r5_result_does_not_depend_on_the_cell_or_on_the_storage_order(patch):
    from effi_mvs_plus_amd import dtu_eval
    want = torch.from_numpy(patch["want"][1])
    order = torch.from_numpy(patch["orders"][1])
    for f in (1.0, 1.5, 3.0):
        keep, _ = dtu_eval.reduce_points(patch["dev"], DST, order=order, cell=f * DST * dtu_eval.CELL_MARGIN)
        assert torch.equal(keep.cpu(), want), f
    n = len(want)
    p = _randperm(n, 11)                                           # xyz2[j] = xyz[p[j]]; the point visited k-th is now at inv[order[k]]
    inv = torch.empty(n, dtype=torch.long)
    inv[p] = torch.arange(n)
    keep, _ = dtu_eval.reduce_points(patch["dev"][p.to(DEV)].contiguous(), DST, order=inv[order])
    assert torch.equal(keep.cpu(), want[p])


# ---- N1, N2 -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def surfaces():
    q, tg = R.two_surfaces(5000, 8000, 3)
    return {"q": q, "t": tg, "want": {cap: R.nn_dist2_capped(q, tg, cap) for cap in (60.0, 2.0)}}


@pytest.mark.parametrize("cap", [60.0, 2.0])
def test_n1_capped_nearest_neighbour_is_exact_for_every_cell_size(surfaces, cap):
    from effi_mvs_plus_amd import dtu_eval
    q, tg = t(torch.from_numpy(surfaces["q"]), DEV), t(torch.from_numpy(surfaces["t"]), DEV)
    want = torch.from_numpy(surfaces["want"][cap])
    capped = int((want == cap * cap).sum())
    print(f"[dtu eval] N1 cap {cap}: {capped} of {len(want)} queries at the cap, median d = {float(want.sqrt().median()):.3f}")
    assert (200 if cap == 60.0 else 300) <= capped < len(want) // 2      # the far queries; at cap 2 most of those beside the box too
    for cell in (None, 0.7, 5.0):
        got = dtu_eval.nn_dist2_capped(q, tg, cap, cell=cell)
        assert got.dtype == torch.float64 and torch.equal(got.cpu(), want), cell


def test_n2_empty_target_set_gives_the_cap():
    from effi_mvs_plus_amd import dtu_eval
    q = torch.randn(777, 3, device=DEV)
    got = dtu_eval.nn_dist2_capped(q, torch.zeros(0, 3, device=DEV), 60.0)
    assert torch.equal(got, torch.full((777,), 3600.0, device=DEV, dtype=torch.float64))
    assert dtu_eval.nn_dist2_capped(torch.zeros(0, 3, device=DEV), q, 60.0).shape == (0,)
    one = dtu_eval.nn_dist2_capped(q, torch.tensor([[0.5, 0.25, -1.0]], device=DEV), 60.0)      # a single target: a 1-cell grid
    assert torch.equal(one.cpu(), torch.from_numpy(R.nn_dist2_capped(q.cpu().numpy(), np.array([[0.5, 0.25, -1.0]]), 60.0)))


def test_n3_queries_deep_inside_the_targets_box_walk_many_shells(surfaces):
    """The targets get a second sheet 40 above the first and 100 queries sit 10-30 above the first sheet: INSIDE the grid's box and
    >= 10 from every target, so their searches walk >= 14 full shells at cell 0.7, interior columns included (a query outside the
    box starts at the first shell that touches it and is done after a few)."""
    from effi_mvs_plus_amd import dtu_eval
    g = np.random.default_rng(8)
    tg_h = np.concatenate([surfaces["t"], surfaces["t"][:500] + np.float32([0, 0, 40])])
    deep = np.stack([g.uniform(-15, 15, 100), g.uniform(-15, 15, 100), g.uniform(10, 30, 100)], -1).astype(np.float32)
    q_h = np.concatenate([surfaces["q"][:1000], deep])
    want = torch.from_numpy(R.nn_dist2_capped(q_h, tg_h, 60.0))
    assert 81.0 <= float(want[-100:].min()) and float(want[-100:].max()) < 3600.0
    q, tg = t(torch.from_numpy(q_h), DEV), t(torch.from_numpy(tg_h), DEV)
    for cell in (None, 0.7, 5.0):
        assert torch.equal(dtu_eval.nn_dist2_capped(q, tg, 60.0, cell=cell).cpu(), want), cell


# ---- masks on voxel edges -----------------------------------------------------------------------------------------------------
def test_masks_round_halves_away_from_zero_and_sum_the_plane_left_to_right():
    from effi_mvs_plus_amd import ops
    obs = np.zeros((3, 3, 3), bool)
    obs[1, 0, 0] = obs[0, 0, 0] = obs[2, 2, 2] = True
    bb0 = [10.0, 10.0, 10.0]
    q = np.array([[11.0, 10, 10], [9.0, 10, 10], [8.999, 10, 10], [13.0, 10, 10], [10, 10, 15.0], [14.9, 14.9, 14.9], [15.0, 15, 15],
                  [-1e30, 10, 10], [1e30, 1e30, 1e30]], np.float32)
    want = R.data_in_mask(q, obs, np.array([bb0, bb0]), 2.0)
    assert list(want) == [True, True, False, False, False, True, False, False, False]
    got = ops.dtu_obs_mask(t(torch.from_numpy(q), DEV), torch.from_numpy(obs).to(DEV), bb0, 2.0)
    assert got.dtype == torch.bool and torch.equal(got.cpu(), torch.from_numpy(want))
    g = np.random.default_rng(0)
    s = g.normal(0, 30, (4099, 3)).astype(np.float32)
    plane = np.array([0.3, -0.2, 0.93, 1.7])
    above = ops.dtu_above_plane(t(torch.from_numpy(s), DEV), plane)
    want = R.stl_above_plane(s, plane)
    assert 0.3 < want.mean() < 0.7 and torch.equal(above.cpu(), torch.from_numpy(want))


# ---- E1 -----------------------------------------------------------------------------------------------------------------------
def test_e1_point_compare_on_a_synthetic_scan():
    from effi_mvs_plus_amd import dtu_eval
    s = R.synthetic_scan(0)
    order = _randperm(len(s["xyz"]), 0).numpy()
    want = R.point_compare(s["xyz"], s["stl"], s["obs_mask"], s["bb"], s["res"], s["plane"], order)
    got = dtu_eval.point_compare(t(torch.from_numpy(s["xyz"]), DEV), t(torch.from_numpy(s["stl"]), DEV), torch.from_numpy(s["obs_mask"]),
                                 s["bb"], s["res"], s["plane"], seed=0)
    lo, hi = R.block_range(s["bb"], 60.0)
    q = want["Qdata"].astype(np.float64)
    outside = ~((q >= lo) & (q < hi)).all(1)
    print(f"[dtu eval] E1: {want['n_input']} -> {want['n_reduced']} points, {int(outside.sum())} beyond the block range, "
          f"{int((~want['DataInMask']).sum())} outside the mask, {int((~want['StlAbovePlane']).sum())} ground-truth points below the plane, "
          f"{int((want['Ddata'] >= 20).sum())} outliers; n_acc {want['n_acc']}, n_comp {want['n_comp']}")
    assert list(np.floor((s["bb"][1] - s["bb"][0]) / 60.0)) == [1, 0, 0]                          # two blocks along x
    assert outside.sum() > 50 and (~want["DataInMask"]).sum() > 1000 and (want["Ddata"] >= 20).sum() > 100
    assert 0.3 < want["StlAbovePlane"].mean() < 0.7 and want["n_reduced"] < want["n_input"]
    for k in ("keep", "DataInMask", "StlAbovePlane"):
        assert got[k].dtype == torch.bool and torch.equal(got[k].cpu(), torch.from_numpy(want[k])), k
    assert torch.equal(got["Qdata"].cpu(), torch.from_numpy(want["Qdata"]))
    for k in ("Ddata2", "Dstl2"):                                  # every element: values at or above the cap are the cap on both sides
        assert got[k].dtype == torch.float64 and torch.equal(got[k].cpu(), torch.from_numpy(want[k])), k
    for k in ("Ddata", "Dstl"):
        assert torch.equal(got[k].cpu() >= 60.0, torch.from_numpy(want[k] >= 60.0)), k
    for k in ("n_input", "n_reduced", "n_acc", "n_comp"):
        assert got[k].dtype == torch.int64 and got[k].is_cuda and int(got[k]) == want[k], k
    # The means' only freedom is the fp64 summation order (the device reduces as a tree, numpy pairwise): 1e-12 relative covers
    # n * 2^-53 for the 3e4 terms here a thousand times over, and nothing else.
    for k in ("acc_mean", "comp_mean", "overall"):
        g_, w_ = float(got[k]), want[k]
        print(f"[dtu eval] E1 {k}: {g_:.17g} (reference {w_:.17g})")
        assert got[k].dtype == torch.float64 and got[k].is_cuda and abs(g_ - w_) <= 1e-12 * abs(w_), k
    # A median is one sorted element (or the mean of two) of sqrt(d^2) with d^2 bitwise equal above and IEEE sqrt correctly rounded
    # on both sides; the downsample factor is one division of two equal counts: exact.
    for k in ("acc_median", "comp_median", "downsample_factor"):
        g_, w_ = float(got[k]), want[k]
        print(f"[dtu eval] E1 {k}: {g_:.17g} (reference {w_:.17g})")
        assert got[k].dtype == torch.float64 and got[k].is_cuda and g_ == w_, k


# ---- E2 -----------------------------------------------------------------------------------------------------------------------
def test_e2_fuse_scan_output_goes_straight_into_point_compare():
    from effi_mvs_plus_amd import dtu_eval, dtu_fusion
    h, w, n = 64, 80, 3
    d, cams = synth.synth_depth_maps(h, w, n, seed=3, noise_mm=0.03, outlier_frac=0.08, pixel_center=0.0)
    g = torch.Generator().manual_seed(10)
    conf, img = torch.rand(n, h // 2, w // 2, generator=g), torch.rand(n, h, w, 3, generator=g)
    fused = dtu_fusion.fuse_scan(t(d, DEV), t(conf, DEV), t(cams, DEV), t(img, DEV), [(0, [1, 2]), (1, [0, 2]), (2, [0, 1])], conf=0.3)
    xyz = fused["xyz"]
    assert xyz.is_cuda and xyz.dtype == torch.float32 and xyz.shape[0] > 500
    lo, hi = xyz.amin(0).double(), xyz.amax(0).double()
    res = float((hi - lo).max()) / 38.0
    stl = (xyz[::3] + 0.5).contiguous()                            # a "scanned surface" half a millimetre beside every third vertex
    out = dtu_eval.point_compare(xyz, stl, torch.ones(40, 40, 40, dtype=torch.bool), torch.stack([lo, hi]).cpu(), res,
                                 [0.0, 0.0, 1.0, -float(xyz[:, 2].median())], dst=4.0)
    assert out["Qdata"].device == xyz.device and int(out["n_input"]) == xyz.shape[0] and 0 < int(out["n_reduced"]) <= xyz.shape[0]
    assert int(out["n_acc"]) > 0 and int(out["n_comp"]) > 0
    for k in ("acc_mean", "acc_median", "comp_mean", "comp_median", "overall", "downsample_factor"):
        assert bool(torch.isfinite(out[k])), k
    assert 0.0 < float(out["acc_median"]) < 20.0 and 0.0 < float(out["comp_median"]) < 20.0
