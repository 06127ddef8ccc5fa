"""GPU: training on batches whose samples each have their own depth range (BlendedMVS, datasets/blend.py).

K  the two ranged conversion kernels (effi_inv_to_depth_ranged_f32 / _bwd) equal the by-value cases of pointwise_kernel bit for bit,
   per sample, on the vector and the scalar path, and lie inside the float64 intervals of tests/pixel_bound.py;
E  the train-mode forward composed from them: unchanged for a common range, the same composition for mixed ranges, and the mixed
   batch against torch autograd through the training-mode oracle (which is batched like the reference);
G  ``GraphedTrainStep(depth_range="sample")`` replays batches of any ranges; the default mode still refuses a foreign range;
R  BlendedMVS samples end to end: ``load_raw_sample``, ``train_epoch`` with a scheduler;
C  tools/finetune_blend.py in a child process writes a checkpoint that loads.
"""
import copy
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import pixel_bound as PB
from common import ROOT, build_model, model_args
from conv_bound import check_bounded
from train_input_trees import cam_text, write_blend_tree
from effi_mvs_plus_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, W, N = 128, 160, 3
DLOSS = [1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4]           # train.py:246


def rel(got, want):
    want = want.detach().double().cpu()
    return float((got.detach().double().cpu() - want).abs().max() / (want.abs().max() + 1e-30))


def bounded(name, got, iv):
    return check_bounded(name, got, iv.mid, iv.half, quiet=True)


# ---- K: the kernels ----------------------------------------------------------------------------------------------------------------
N_RANGE = 5
K_SIZES = [1, 257, 4 * 257, 20 * 24 + 3]     # one element; no multiple of 4 or 256; vector path past one workgroup; scalar path
K_RANGES = ("pw_range", "clamp_edge", "other")


def _k_ranges():
    return [PB.PW_RANGE, (PB.clamp_edge_lo(), PB.PW_RANGE[1]), (1.0 / 748.0, 1.0 / 340.0)]


def _k_case(n, aligned):
    """-> host (inv, g, dv) [3,n], [3,n], [3,N_RANGE] and their device forms; ``aligned``: every device tensor starts on a 16-byte
    boundary, else inv / g / depth_values start one element into their storage.  Only the two ends of a depth_values row are read:
    the entries between them are NaN."""
    ranges = _k_ranges()
    inv, g = [], []
    for b in range(3):
        t_ = PB.pw_inputs(n, seed=400 + n + b)
        iv = t_["inv"].clone()
        if K_RANGES[b] == "clamp_edge":
            iv[::5] = 0.0                        # s sits ON the clamp's threshold there
        inv.append(iv), g.append(t_["g"])
    inv, g = torch.stack(inv), torch.stack(g)
    dv = torch.full((3, N_RANGE), float("nan"))
    for b, (lo, hi) in enumerate(ranges):
        dv[b, 0], dv[b, -1] = lo, hi
    off = 0 if aligned else 1

    def dev(x):
        store = torch.zeros(x.numel() + off, device=DEV)
        view = store[off:].view(x.shape)
        view.copy_(x)
        assert view.is_contiguous() and (view.data_ptr() % 16 == 0) == aligned
        return view

    return inv, g, dv, dev(inv), dev(g), dev(dv)


def _k_out(n, aligned):
    """[3,n] output inside a NaN-filled store with guard elements on either side: four (the output stays 16-byte aligned, so that
    n % 4 == 0 takes the vector path) or one (the output itself is misaligned)."""
    pad = 4 if aligned else 1
    store = torch.full((3 * n + 2 * pad,), float("nan"), device=DEV)
    out = store[pad:pad + 3 * n].view(3, n)
    assert (out.data_ptr() % 16 == 0) == aligned
    return store, out, pad


def _k_canary(store, pad):
    assert bool(torch.isnan(store[:pad]).all()) and bool(torch.isnan(store[-pad:]).all()), "wrote outside the output"


@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("n", K_SIZES)
def test_ranged_kernels_equal_the_by_value_kernels_bit_for_bit(n, aligned):
    """K1."""
    from effi_mvs_plus_amd import ops
    inv, g, dv, inv_d, g_d, dv_d = _k_case(n, aligned)
    store_f, out_f, pad = _k_out(n, aligned)
    store_b, out_b, _ = _k_out(n, aligned)
    assert ops.inv_to_depth_ranged(inv_d, dv_d, out=out_f) is out_f
    assert ops.inv_to_depth_ranged_bwd(g_d, inv_d, dv_d, out=out_b) is out_b
    torch.cuda.synchronize()
    _k_canary(store_f, pad), _k_canary(store_b, pad)
    # without out=: the same bits in a fresh tensor
    assert torch.equal(ops.inv_to_depth_ranged(inv_d, dv_d), out_f) and torch.equal(ops.inv_to_depth_ranged_bwd(g_d, inv_d, dv_d), out_b)
    for b, kind in enumerate(K_RANGES):
        lo, hi = float(dv[b, 0]), float(dv[b, -1])
        ib, gb = inv_d[b].contiguous(), g_d[b].contiguous()
        want_f = ops.pointwise(ops.PW_INV_TO_DEPTH, ib, s0=lo, s1=hi)
        want_b = ops.pointwise(ops.PW_INV_TO_DEPTH_BWD, gb, ib, s0=lo, s1=hi)
        assert torch.equal(out_f[b], want_f), (n, aligned, kind, "forward")
        assert torch.equal(out_b[b], want_b), (n, aligned, kind, "backward")
        assert bool(torch.isfinite(out_f[b]).all()) and bool(torch.isfinite(out_b[b]).all())
        if kind != "other":
            bounded(f"inv_to_depth_ranged n={n} {kind}", out_f[b], PB.pw_interval("inv_to_depth", a=inv[b], s0=lo, s1=hi)[0])
            iv = PB.pw_interval("inv_to_depth_bwd", a=g[b], b=inv[b], s0=lo, s1=hi)[0]
            if kind == "clamp_edge":
                assert bool((iv.half[::5] == 0).all())           # on the threshold: pinned to 0
            bounded(f"inv_to_depth_ranged_bwd n={n} {kind}", out_b[b], iv)


@pytest.mark.parametrize("n", [257, 4 * 257])
def test_ranged_conversion_through_autograd(n):
    """K2: forward / backward of the autograd Function are the kernels' bits; depth_values receives no gradient."""
    from effi_mvs_plus_amd import autograd as A, ops
    _, _, _, inv_d, g_d, dv_d = _k_case(n, True)
    dv_d = torch.nan_to_num(dv_d, nan=1.0).requires_grad_(True)      # a leaf that COULD receive a gradient
    leaf = inv_d.clone().requires_grad_(True)
    out = A.inv_to_depth_ranged(leaf, dv_d)
    out.backward(g_d)
    assert torch.equal(out.detach(), ops.inv_to_depth_ranged(inv_d, dv_d.detach()))
    assert torch.equal(leaf.grad, ops.inv_to_depth_ranged_bwd(g_d, inv_d, dv_d.detach()))
    assert dv_d.grad is None
    for b in range(3):
        lo, hi = float(dv_d.detach()[b, 0]), float(dv_d.detach()[b, -1])
        assert torch.equal(leaf.grad[b], ops.pointwise(ops.PW_INV_TO_DEPTH_BWD, g_d[b].contiguous(), inv_d[b].contiguous(), s0=lo, s1=hi))


def test_ranged_operators_refuse_mismatched_arguments():
    from effi_mvs_plus_amd import ops
    inv, dv = torch.zeros(2, 8, device=DEV), torch.ones(2, 4, device=DEV)
    for bad_inv, bad_dv in ((inv, dv[:1]), (inv, dv[:, :1]), (inv, dv[0]), (inv, dv.cpu())):
        with pytest.raises(ValueError):
            ops.inv_to_depth_ranged(bad_inv, bad_dv)
        with pytest.raises(ValueError):
            ops.inv_to_depth_ranged_bwd(bad_inv, bad_inv, bad_dv)
    with pytest.raises(ValueError):
        ops.inv_to_depth_ranged_bwd(inv[:, :4].contiguous(), inv, dv)


# ---- E: the train-mode forward -----------------------------------------------------------------------------------------------------
def _loss_inputs(B, seed):
    g = torch.Generator().manual_seed(seed)
    gt, mask = {}, {}
    for k, f in (("stage1", 8), ("stage2", 4), ("stage3", 2), ("stage4", 1)):
        gt[k] = synth.DEPTH_MIN_MM + (synth.DEPTH_MAX_MM - synth.DEPTH_MIN_MM) * torch.rand(B, H // f, W // f, generator=g)
        mask[k] = (torch.rand(B, H // f, W // f, generator=g) > 0.3).float()
    return gt, mask


def _batch(seeds, scales, loss_seed=2):
    """Host batch: synthetic samples ``seeds``, sample b's inverse-depth range scaled by ``scales[b]`` -> (imgs, pm, dv, gt, mask)."""
    samples = [synth.synth_sample(H, W, N, seed=s) for s in seeds]
    imgs = torch.cat([s[0] for s in samples])
    pm = {k: torch.cat([s[1][k] for s in samples]) for k in samples[0][1]}
    dv = torch.cat([s[2] * float(c) for s, c in zip(samples, scales)])
    gt, mask = _loss_inputs(len(seeds), loss_seed)
    return imgs, pm, dv, gt, mask


def _to_dev(batch):
    imgs, pm, dv, gt, mask = batch
    d = lambda m: {k: v.to(DEV) for k, v in m.items()}      # noqa: E731
    return imgs.to(DEV), d(pm), dv.to(DEV), d(gt), d(mask)


def _train_net(seed):
    net, sd = build_model("8,8,8", seed=seed, device=DEV)
    net.train()
    for m in net.modules():
        if isinstance(m, torch.nn.Dropout2d):
            m.p = 0.0
    return net, sd


@pytest.fixture(scope="module")
def net13():
    return _train_net(13)


def _restore_buffers(net, state):
    with torch.no_grad():
        for k, b_ in net.named_buffers():
            b_.copy_(state[k])


@pytest.mark.parametrize("scales", [(1.0, 1.0), (1.0, 1.25)], ids=["E1-uniform", "E2-mixed"])
def test_train_forward_equals_the_per_sample_by_value_composition(net13, monkeypatch, scales):
    """E1 / E2: the 13 outputs and the loss with the ranged kernels equal, bit for bit, those with every sample converted by the
    existing by-value operator at its own (lo, hi).  For the uniform batch that IS the path as it was before the ranged kernels."""
    from effi_mvs_plus_amd import autograd as A
    from effi_mvs_plus_amd.models import mvs_loss
    net, _ = net13
    imgs, pm, dv, gt, mask = _to_dev(_batch((30, 31), scales))
    if scales[0] != scales[1]:
        assert not torch.equal(dv[0], dv[1])
    st0 = {k: v.clone() for k, v in net.state_dict().items()}
    calls = []

    def run():
        with torch.no_grad():
            out = net(imgs, pm, dv)["depth"]
            loss, _ = mvs_loss(out, gt, mask, DLOSS)
        _restore_buffers(net, st0)
        return [o.clone() for o in out], loss.clone()

    got, got_loss = run()

    def per_sample(inv, depth_values):
        calls.append(tuple(inv.shape))
        return torch.cat([A.inv_to_depth(inv[b:b + 1], float(depth_values[b, 0]), float(depth_values[b, -1])) for b in range(inv.shape[0])])

    monkeypatch.setattr(A, "inv_to_depth_ranged", per_sample)
    want, want_loss = run()
    # 13 outputs: the soft-argmin depth of stage 1, then per stage one conversion per GRU iteration and one of the upsampled map
    assert len(calls) == 12 and len(got) == 13 == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert torch.equal(a, b), i
    assert bool(torch.isfinite(got_loss)) and torch.equal(got_loss, want_loss)


def _oracle_training_pass(net, sd, imgs, pm, dv, gt, mask, nd, dtype=torch.float32):
    """torch autograd through the training-mode oracle on the CPU, with the model's aliased parameters tied to one leaf each."""
    from oracle import effi_oracle as O
    cast = lambda v: v.clone().to(dtype) if v.is_floating_point() else v.clone()       # noqa: E731
    sd2 = {k: cast(v) for k, v in sd.items()}
    groups = {}
    for k, p_ in net.named_parameters(remove_duplicate=False):
        groups.setdefault(id(p_), []).append(k)
    leaves = {}
    for ks in groups.values():
        lf = sd2[ks[0]].requires_grad_(True)
        for k in ks:
            sd2[k] = lf
            leaves[k] = lf
    bgroups = {}
    for k, b_ in net.named_buffers(remove_duplicate=False):
        bgroups.setdefault(id(b_), []).append(k)
    for ks in bgroups.values():
        for k in ks[1:]:
            sd2[k] = sd2[ks[0]]
    with O.training(0.0):
        out = O.full_forward(sd2, cast(imgs), {k: cast(v) for k, v in pm.items()}, cast(dv), ndepths=nd)
        loss, _ = O.mvs_loss(out["depth"], {k: cast(v) for k, v in gt.items()}, mask, DLOSS)
    loss.backward()
    return out, loss, leaves, sd2


def test_mixed_range_training_step_matches_autograd_through_the_oracle():
    """E3: the batch (seeds 30, 31; range scales 1.0, 1.25) -- outputs, loss, every parameter gradient and the BatchNorm statistics
    against torch autograd through the training-mode oracle, with the bounds of
    test_gpu_train.py::test_training_step_matches_autograd_through_the_oracle: outputs mean abs <= 1e-3 of EACH SAMPLE'S OWN depth
    range, loss 2e-3 relative, every gradient within max(5e-2, 2 e_ref) of its peak (e_ref: the oracle's own fp32 pass against its
    fp64 pass), relative L2 over all gradients <= 1e-3, running statistics <= 1e-4."""
    from effi_mvs_plus_amd.models import mvs_loss
    nd = (8, 8, 8)
    net, sd = _train_net(13)
    batch = _batch((30, 31), (1.0, 1.25))
    imgs, pm, dv, gt, mask = batch
    want_out, want_loss, leaves32, sd2 = _oracle_training_pass(net, sd, imgs, pm, dv, gt, mask, nd)
    _, _, leaves64, _ = _oracle_training_pass(net, sd, imgs, pm, dv, gt, mask, nd, dtype=torch.float64)
    d_imgs, d_pm, d_dv, d_gt, d_mask = _to_dev(batch)
    out = net(d_imgs, d_pm, d_dv)
    loss, _ = mvs_loss(out["depth"], d_gt, d_mask, DLOSS)
    loss.backward()
    assert len(out["depth"]) == 13
    span = (1.0 / dv[:, 0] - 1.0 / dv[:, -1]).double()              # each sample's own depth range
    assert abs(float(span[0]) - 510.0) < 1e-2 and abs(float(span[1]) - 408.0) < 1e-2
    for i, (a, b) in enumerate(zip(out["depth"], want_out["depth"])):
        assert tuple(a.shape) == tuple(b.shape)
        err = (a.detach().double().cpu() - b.detach().double()).abs().flatten(1).mean(1) / span
        print(f"[mixed ranges] output {i}: mean abs error / own range = {[f'{float(e):.2e}' for e in err]}")
        assert bool((err <= 1e-3).all()), (i, err)
    got_l, want_l = float(loss.detach()), float(want_loss.detach())
    print(f"[mixed ranges] loss {got_l:.4f} vs {want_l:.4f}")
    assert abs(got_l - want_l) <= 2e-3 * abs(want_l)
    num = den = 0.0
    failures, n = [], 0
    for k, p_ in net.named_parameters():
        assert p_.grad is not None, f"{k}: no gradient"
        e_hip = rel(p_.grad, leaves64[k].grad)
        e_ref = rel(leaves32[k].grad, leaves64[k].grad)
        bound = max(5e-2, 2 * e_ref)
        if e_hip > bound:
            failures.append(f"{k}: gradient off by {e_hip:.3e} of its peak (bound {bound:.3e}; reference fp32 vs fp64: {e_ref:.3e})")
        num += float((p_.grad.detach().double().cpu() - leaves64[k].grad).pow(2).sum())
        den += float(leaves64[k].grad.pow(2).sum())
        n += 1
    print(f"[mixed ranges] {n} parameters, relative L2 distance of all gradients {math.sqrt(num / den):.3e}")
    assert not failures, "; ".join(failures)
    assert n > 200 and math.sqrt(num / den) <= 1e-3
    for k, v in net.state_dict().items():
        if "running_" in k:
            assert rel(v, sd2[k]) <= 1e-4, k
        if "num_batches_tracked" in k:
            assert int(v) == int(sd2[k]), k


# ---- G: the graphed step -----------------------------------------------------------------------------------------------------------
def test_graphed_step_in_sample_mode_replays_any_ranges():
    from effi_mvs_plus_amd import train_graph
    from effi_mvs_plus_amd.models.module import mvs_loss_static
    net, _ = _train_net(4)
    ref = copy.deepcopy(net)
    DL = list(train_graph.DLOSS)
    first = _to_dev(_batch((30, 31), (1.0, 1.25)))
    replays = [_to_dev(_batch((32, 33), sc)) for sc in ((1.25, 1.0), (1.0, 1.25), (1.0, 1.0))]
    eager = []
    ref_state = {k: v.clone() for k, v in ref.state_dict().items()}
    for imgs, pm, dv, gt, mask in replays:
        with torch.no_grad():
            loss, _ = mvs_loss_static(ref(imgs, pm, dv)["depth"], gt, mask, DL)
        _restore_buffers(ref, ref_state)
        eager.append(float(loss))
    print(f"[sample mode] eager losses {eager}")
    # what keeps the comparison meaningful: the ranges move the loss by far more than the tolerance
    for i in range(3):
        for j in range(i + 1, 3):
            assert abs(eager[i] - eager[j]) >= 5e-3 * max(abs(eager[i]), abs(eager[j])), eager
    with pytest.raises(ValueError):
        train_graph.GraphedTrainStep(net, torch.optim.AdamW(net.parameters(), lr=0.0, capturable=True), *first, depth_range="nonsense")
    opt = torch.optim.AdamW(net.parameters(), lr=0.0, weight_decay=0.0, capturable=True)      # the weights stay: replays are comparable
    step = train_graph.GraphedTrainStep(net, opt, *first, depth_range="sample")
    assert step.depth_range is None and getattr(net, "static_depth_range", None) is None
    got = []
    for smp in replays:
        got.append(float(step(*smp).detach()))
        assert getattr(net, "static_depth_range", None) is None
    print(f"[sample mode] replayed losses {got}")
    for a, b in zip(got, eager):
        assert abs(a - b) <= 2e-4 * abs(b), (got, eager)
    step.check_ranges()
    # an unusable range: host tensor -> refused before anything is written; device tensor -> counted, reported by check_ranges()
    imgs, pm, dv, gt, mask = replays[0]
    kept = step.depth_values.clone()
    bad_dv = dv.clone()
    bad_dv[:, -1] = bad_dv[:, 0] * 0.5                               # last <= first
    one_bad = dv.clone()
    one_bad[1, -1] = one_bad[1, 0]                                   # in one sample of the batch only
    for host in (bad_dv.cpu(), one_bad.cpu()):
        with pytest.raises(ValueError, match="depth range"):
            step.load_sample(imgs, pm, host, gt, mask)
    assert torch.equal(step.depth_values, kept)
    for other in (torch.where(torch.arange(dv.shape[1], device=DEV) == 0, torch.zeros_like(dv), dv),          # first = 0
                  torch.where(torch.arange(dv.shape[1], device=DEV) == dv.shape[1] - 1, torch.full_like(dv, float("inf")), dv),
                  torch.where(torch.arange(dv.shape[1], device=DEV) == 0, torch.full_like(dv, float("nan")), dv)):
        with pytest.raises(ValueError, match="depth range"):
            step.load_sample(imgs, pm, other.cpu(), gt, mask)
    step.check_ranges()
    step.load_sample(imgs, pm, bad_dv, gt, mask)
    with pytest.raises(ValueError, match="depth range"):
        step.check_ranges()
    step.load_sample(imgs, pm, dv, gt, mask)
    # the default mode still holds its range by value and refuses another one
    opt_s = torch.optim.AdamW(net.parameters(), lr=0.0, weight_decay=0.0, capturable=True)
    static = train_graph.GraphedTrainStep(net, opt_s, *replays[2])
    assert static.depth_range == (float(replays[2][2][0, 0]), float(replays[2][2][0, -1]))
    with pytest.raises(ValueError, match="depth range"):
        static.load_sample(imgs, pm, dv.cpu(), gt, mask)
    assert getattr(net, "static_depth_range", None) is None


# ---- R / C: BlendedMVS end to end ----------------------------------------------------------------------------------------------------
BLEND_VIEWS = 9


@pytest.fixture(scope="module")
def blend_rig(tmp_path_factory):
    """A BlendedMVS tree of 9 views at 128x160 whose cameras are the synthetic ring (not random rotations); odd views carry the range
    (425, 935), even views (340, 748)."""
    root = str(tmp_path_factory.mktemp("blend_rig"))
    ranges = {v: ((425.0, 935.0) if v % 2 else (340.0, 748.0)) for v in range(BLEND_VIEWS)}
    listfile, stored = write_blend_tree(root, ["scene"], BLEND_VIEWS, (H, W), ranges=ranges)
    pm = synth.synth_cameras(H, W, BLEND_VIEWS, torch.float64)["stage4"][0]      # the dataset's stage4 is the cam file as stored
    for v in range(BLEND_VIEWS):
        lo, hi = ranges[v]
        with open(os.path.join(root, "scene", "cams", f"{v:08d}_cam.txt"), "w") as f:
            f.write(cam_text(pm[v, 0].numpy(), pm[v, 1, :3, :3].numpy(), f"{lo!r} 0.05 128 {hi!r}"))
    return root, listfile


def _args(s):
    return s["imgs"], s["proj_matrices"], s["depth_values"], s["depth"], s["mask"]


def test_blendedmvs_batches_with_their_own_ranges_end_to_end(blend_rig):
    """R."""
    from torch.utils.data import DataLoader, default_collate
    from effi_mvs_plus_amd import train_graph
    from effi_mvs_plus_amd.datasets import blend, prepare_train_sample
    from effi_mvs_plus_amd.models import mvs_loss_fused
    root, listfile = blend_rig
    ds = blend.MVSDataset(root, listfile, "val", N, 64, device="host")
    assert len(ds) == BLEND_VIEWS - 1
    raws = [default_collate([ds[0], ds[1]]), default_collate([ds[2], ds[3]])]
    for r in raws:
        assert not torch.equal(r["depth_values"][0], r["depth_values"][1])         # two ranges in every batch
    prepared = [prepare_train_sample(r, device=DEV) for r in raws]
    net, _ = _train_net(4)
    opt = torch.optim.AdamW(net.parameters(), lr=0.0, weight_decay=0.0, capturable=True)
    step = train_graph.GraphedTrainStep(net, opt, *_args(prepared[0]), depth_range="sample", loss_fn=mvs_loss_fused)
    step.load_sample(*_args(prepared[1]))
    kept = (step.imgs.clone(), {k: v.clone() for k, v in step.gt.items()}, {k: v.clone() for k, v in step.mask.items()},
            {k: v.clone() for k, v in step.proj.items()}, step.depth_values.clone())
    loss_a = float(step().detach())
    for t_ in [step.imgs, step.depth_values] + list(step.gt.values()) + list(step.mask.values()) + list(step.proj.values()):
        t_.fill_(float("nan"))
    step.load_raw_sample(raws[1])
    assert torch.equal(step.imgs, kept[0]) and torch.equal(step.depth_values, kept[4])
    for k in step.gt:
        assert torch.equal(step.gt[k].nan_to_num(-1.0), kept[1][k].nan_to_num(-1.0)) and torch.equal(step.mask[k], kept[2][k]), k
        assert bool((torch.isnan(step.gt[k]) == torch.isnan(kept[1][k])).all())
    for k in step.proj:
        assert torch.equal(step.proj[k], kept[3][k]), k
    loss_b = float(step().detach())
    assert np.isfinite(loss_b) and loss_b == loss_a
    step.check_ranges()
    # the loop around it, with the reference's scheduler on a real rate
    opt2 = torch.optim.AdamW(net.parameters(), lr=1e-4, capturable=True)
    loader = DataLoader(ds, batch_size=2, shuffle=False, num_workers=2, drop_last=True)
    sched = lambda o: torch.optim.lr_scheduler.OneCycleLR(o, 1e-3, len(loader) + 4, pct_start=0.25, cycle_momentum=False,   # noqa: E731
                                                          anneal_strategy="linear")
    sch = sched(opt2)
    step2 = train_graph.GraphedTrainStep(net, opt2, *_args(prepared[0]), depth_range="sample", loss_fn=mvs_loss_fused)
    before = [p.detach().clone() for p in net.parameters()]
    mean_loss, steps = train_graph.train_epoch(step2, loader, sch)
    assert steps == len(loader) == (BLEND_VIEWS - 1) // 2 and np.isfinite(mean_loss) and mean_loss > 0
    assert step2.replays == steps
    twin_opt = torch.optim.AdamW([torch.nn.Parameter(torch.zeros(1))], lr=1e-4)
    twin = sched(twin_opt)
    for _ in range(steps):
        twin_opt.step()
        twin.step()
    assert abs(float(opt2.param_groups[0]["lr"]) - float(twin_opt.param_groups[0]["lr"])) <= 1e-6 * float(twin_opt.param_groups[0]["lr"])
    assert any(not torch.equal(p, q) for p, q in zip(net.parameters(), before))          # it trained
    assert all(bool(torch.isfinite(p).all()) for p in net.parameters())


def test_finetune_blend_driver_writes_a_checkpoint_that_loads(blend_rig, tmp_path):
    """C."""
    from effi_mvs_plus_amd.models import Effi_MVS_plus
    root, listfile = blend_rig
    logdir = str(tmp_path / "log")
    cmd = [sys.executable, os.path.join(ROOT, "tools", "finetune_blend.py"), "--trainpath", root, "--trainlist", listfile, "--logdir", logdir,
           "--ndepths", "8,8,8", "--numdepth", "64", "--trainviews", "3", "--batch_size", "2", "--num_workers", "2", "--epochs", "1",
           "--lr", "1e-4"]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    print(res.stdout[-2000:], res.stderr[-2000:])
    assert res.returncode == 0, res.stderr[-2000:]
    path = os.path.join(logdir, "model_000000.ckpt")
    assert os.path.isfile(path)
    ckpt = torch.load(path, map_location="cpu")
    assert set(ckpt) == {"epoch", "model", "optimizer"} and ckpt["epoch"] == 0
    net = Effi_MVS_plus(model_args("8,8,8"))
    net.load_state_dict(ckpt["model"], strict=True)
    assert all(bool(torch.isfinite(v).all()) for v in ckpt["model"].values() if v.is_floating_point())
    opt = torch.optim.AdamW(net.parameters(), lr=1e-4)
    opt.load_state_dict(ckpt["optimizer"])
    assert len(opt.state_dict()["state"]) > 0
