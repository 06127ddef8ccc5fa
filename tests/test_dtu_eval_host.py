"""Host: the CPU restatement of the DTU evaluation (tests/dtu_eval_ref.py) against the .m files' literal loops, and the host-only
parts of effi_mvs_plus_amd/dtu_eval.py (PLY / .mat readers, the block range, the statistics).  No GPU.

  1. reducePts_haa.m's sequential loop, chunk ranges included, == the rounds form (the form the device runs);
  2. MaxDistCP.m's block loop == capped nearest neighbour + the range rule wherever either is below MaxDist, both >= MaxDist elsewhere;
  3. MATLAB's round at .5 and at negative halves;
  4. PLY round trips; 5. load_gt on .mat files; 6. the generators stay clear of the dst threshold.
"""
import numpy as np
import pytest
import torch

import dtu_eval_ref as R
from effi_mvs_plus_amd import dtu_eval, dtu_fusion


def _clouds():
    g = np.random.default_rng(5)
    blob = g.normal(0, 0.25, (1500, 3)).astype(np.float32)
    blob[100:140] = blob[:40]                                     # exact duplicates
    R.assert_clear(blob, 0.2)
    return {"patch": R.noisy_patch(3000, 0, half=1.0), "line": R.collinear(300), "blob": blob}


@pytest.mark.parametrize("name", ["patch", "line", "blob"])
def test_sequential_loop_with_chunks_equals_the_rounds_form(name):
    xyz = _clouds()[name]
    n = len(xyz)
    orders = [np.arange(n), np.arange(n)[::-1].copy(), np.random.default_rng(1).permutation(n)]
    for order in orders:
        want = R.reduce_sequential(xyz, 0.2, order)
        for chunk in (7, 1000):                                   # several overlapping chunk ranges / two
            assert np.array_equal(R.reduce_sequential(xyz, 0.2, order, chunk=chunk), want)
        got, rounds = R.reduce_rounds(xyz, 0.2, order)
        assert np.array_equal(got, want), name
        assert 0 < want.sum() < n and rounds >= 2
        # maximal independent set: no two kept points are neighbours, every removed point has a kept neighbour
        start, idx = R.adjacency(xyz, 0.2)
        for i in range(n):
            nb = idx[start[i]:start[i + 1]]
            assert not want[nb].any() if want[i] else want[nb].any()
    if name == "line":                                            # a dependency chain: one point decided per round, about
        assert R.reduce_rounds(xyz, 0.2, np.arange(n))[1] >= 290


def test_reduce_edge_sizes():
    for n in (0, 1, 2):
        xyz = np.zeros((n, 3), np.float32)
        keep = R.reduce_sequential(xyz, 0.2, np.arange(n))
        assert np.array_equal(keep, R.reduce_rounds(xyz, 0.2, np.arange(n))[0])
        assert keep.sum() == min(n, 1)                            # duplicates: the first visited survives


def _block_cloud():
    g = np.random.default_rng(2)
    bb = np.array([[0.0, 0.0, 0.0], [100.0, 70.0, 30.0]])         # floor([100 70 30] / 60) = [1 1 0]: 2 x 2 x 1 blocks
    to = np.concatenate([g.uniform([5, 5, 5], [40, 40, 25], (400, 3)), g.uniform([100, 100, 0], [118, 118, 50], (200, 3))])
    frm = np.concatenate([g.uniform([0, 0, 0], [120, 120, 60], (1500, 3)),                 # inside the range, near and far
                          g.uniform([-30, -30, -30], [0, 150, 90], (200, 3)),              # x below the range
                          g.uniform([120, 0, 0], [150, 120, 60], (200, 3)),                # x above
                          g.uniform([0, 0, 60], [120, 120, 90], (200, 3))])                # z above
    return to.astype(np.float32), frm.astype(np.float32), bb


def test_block_loop_equals_capped_nn_plus_range_rule():
    to, frm, bb = _block_cloud()
    assert list(np.floor((bb[1] - bb[0]) / 60.0)) == [1, 1, 0]
    lit = R.max_dist_cp_literal(to, frm, bb, 60.0)
    got, got2 = R.max_dist_cp(to, frm, bb, 60.0)
    lo, hi = R.block_range(bb, 60.0)
    inside = ((frm >= lo) & (frm < hi)).all(1)
    assert 0 < inside.sum() < len(frm) and (lit[~inside] == 60.0).all() and (got[~inside] == 60.0).all()
    below = (lit < 60.0) | (got < 60.0)
    assert 100 < below.sum() < inside.sum()                       # some in-range points are farther than MaxDist from every target
    assert np.array_equal(lit[below], got[below])
    assert (lit[~below] >= 60.0).all() and (got[~below] == 60.0).all()
    assert np.array_equal(got2[below], R.nn_dist2_capped(frm, to, 60.0)[below])
    # the package's range rule is the same box
    plo, phi = dtu_eval.block_range(torch.from_numpy(bb), 60.0)
    assert np.array_equal(plo.numpy(), lo) and np.array_equal(phi.numpy(), hi)


def test_matlab_round_at_halves():
    v = np.array([0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 0.49999999999999994, -0.49999999999999994, 2.4999, -2.5001, 0.0, 7.0])
    assert list(R.matlab_round(v)) == [1, 2, 3, -1, -2, -3, 0, -0.0, 2, -3, 0, 7]
    assert list(np.round(v[:3])) == [0, 2, 2]                     # what half-to-even would give instead
    # voxel edges: (q - bb0) / res + 1 = 1.5 -> index 2; 0.5 -> index 1 (inside); just below 0.5 -> 0 (outside)
    obs = np.zeros((3, 3, 3), bool)
    obs[1, 0, 0] = obs[0, 0, 0] = True
    bb = np.array([[10.0, 10.0, 10.0], [20.0, 20.0, 20.0]])
    q = np.array([[11.0, 10, 10], [9.0, 10, 10], [8.999, 10, 10], [13.0, 10, 10], [10, 10, 15.0]], np.float32)
    assert list(R.data_in_mask(q, obs, bb, 2.0)) == [True, True, False, False, False]


def test_ply_round_trips(tmp_path):
    g = np.random.default_rng(0)
    xyz = g.normal(0, 50, (257, 3)).astype(np.float32)
    rgb = g.integers(0, 256, (257, 3)).astype(np.uint8)
    dtu_fusion.write_ply(str(tmp_path / "a.ply"), xyz, rgb)
    assert dtu_eval.read_ply_xyz(tmp_path / "a.ply").tobytes() == xyz.tobytes()
    # extra float normals between and after the coordinates, big-endian, with a comment and a trailing face element
    rec = np.empty(257, dtype=[("nx", ">f4"), ("x", ">f4"), ("y", ">f4"), ("ny", ">f4"), ("z", ">f4"), ("nz", ">f4"), ("red", "u1")])
    for k, a in zip(("x", "y", "z"), xyz.T):
        rec[k] = a
    rec["nx"], rec["ny"], rec["nz"], rec["red"] = 1.0, 2.0, 3.0, 7
    head = ("ply\nformat binary_big_endian 1.0\ncomment made by a test\nelement vertex 257\nproperty float nx\nproperty float x\n"
            "property float y\nproperty float ny\nproperty float z\nproperty float nz\nproperty uchar red\n"
            "element face 0\nproperty list uchar int vertex_indices\nend_header\n")
    (tmp_path / "b.ply").write_bytes(head.encode() + rec.tobytes())
    assert dtu_eval.read_ply_xyz(tmp_path / "b.ply").tobytes() == xyz.tobytes()
    # ASCII with normals; %.9g prints float32 exactly
    with open(tmp_path / "c.ply", "w") as f:
        f.write("ply\nformat ascii 1.0\nelement vertex 257\nproperty float x\nproperty float y\nproperty float z\nproperty float nx\n"
                "property float ny\nproperty float nz\nend_header\n")
        for p in xyz:
            f.write("%.9g %.9g %.9g 0 0 1\n" % tuple(p))
    assert dtu_eval.read_ply_xyz(tmp_path / "c.ply").tobytes() == xyz.tobytes()
    (tmp_path / "d.ply").write_bytes(b"ply\nformat ascii 1.0\nelement vertex 0\nproperty float x\nproperty float y\nproperty float z\nend_header\n")
    assert dtu_eval.read_ply_xyz(tmp_path / "d.ply").shape == (0, 3)
    (tmp_path / "e.ply").write_bytes(head.encode() + rec.tobytes()[:100])
    with pytest.raises(ValueError):
        dtu_eval.read_ply_xyz(tmp_path / "e.ply")


def test_load_gt_reads_the_sample_set_layout(tmp_path):
    from scipy.io import savemat
    g = np.random.default_rng(1)
    obs = g.random((5, 6, 7)) < 0.5
    bb = np.array([[-1.0, -2.0, -3.0], [4.0, 5.0, 6.0]])
    plane = np.array([[0.1], [0.2], [0.9], [-3.0]])
    stl = g.normal(0, 10, (33, 3)).astype(np.float32)
    (tmp_path / "ObsMask").mkdir()
    (tmp_path / "Points" / "stl").mkdir(parents=True)
    savemat(tmp_path / "ObsMask" / "ObsMask9_10.mat", {"ObsMask": obs, "BB": bb, "Res": 0.25})
    savemat(tmp_path / "ObsMask" / "Plane9.mat", {"P": plane})
    dtu_fusion.write_ply(str(tmp_path / "Points" / "stl" / "stl009_total.ply"), stl, np.zeros((33, 3), np.uint8))
    gt = dtu_eval.load_gt(str(tmp_path), 9)
    assert gt["obs_mask"].dtype == bool and gt["obs_mask"].flags["C_CONTIGUOUS"] and np.array_equal(gt["obs_mask"], obs)
    assert np.array_equal(gt["bb"], bb) and gt["res"] == 0.25 and np.array_equal(gt["plane"], plane.reshape(4))
    assert gt["stl"].tobytes() == stl.tobytes()


def test_generators_stay_clear_of_the_threshold():
    for seed in range(3):
        c = R.min_clearance(R.noisy_patch(20000, seed), 0.2)
        print(f"[dtu eval] noisy_patch seed {seed}: closest pair distance to dst, relative: {c:.2e}")
        assert c > R.CLEARANCE
    assert R.min_clearance(R.collinear(), 0.2) > 0.2
    assert R.min_clearance(R.synthetic_scan()["xyz"], 0.2) > R.CLEARANCE


def test_statistics_and_argument_checks_on_the_host():
    g = np.random.default_rng(3)
    for n in (0, 1, 6, 7):
        v = g.random(n)
        m, d = dtu_eval._mean_median(torch.from_numpy(v))
        wm, wd = R.mean_median(v)
        if n == 0:
            assert np.isnan(float(m)) and np.isnan(float(d)) and np.isnan(wm) and np.isnan(wd)
        else:
            assert float(d) == wd and abs(float(m) - wm) <= 1e-15
    assert dtu_eval._grid(torch.tensor([[-0.3, 0.0, 0.1], [0.5, 0.0, 0.1]], dtype=torch.float64), 0.2) == ([-2, 0, 0], [5, 1, 1])
    with pytest.raises(ValueError):
        dtu_eval._grid(torch.tensor([[0.0, 0.0, 0.0], [1e9, 0.0, 0.0]], dtype=torch.float64), 0.2)
    keep, rounds = dtu_eval.reduce_points(torch.zeros(0, 3), 0.2)
    assert keep.shape == (0,) and rounds == 0
    from effi_mvs_plus_amd._lib import EffiLibraryError
    with pytest.raises(EffiLibraryError):                         # no CPU fallback
        dtu_eval.reduce_points(torch.zeros(4, 3), 0.2)
    with pytest.raises(ValueError):
        dtu_eval.reduce_points(torch.zeros(4, 3), 0.2, order=torch.arange(4), seed=1)
