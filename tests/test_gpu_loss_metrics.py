"""The training loss and the depth metrics on the GPU (csrc/metrics.hip) against the float64 restatement of tests/loss_metrics_ref.py,
which tests/test_loss_metrics_host.py pins to the recorded reference.  Bounds (derived there and in DESIGN.md section 2.4, nothing
left out): integer tables exact; fp64 sums within (N - 1) 2^-53 sum|x|; every fp32 scalar and l_i one rounding of its fp64 quotient;
the total within 2.5 x 2^-24 sum w_i |l_i|; gradients within 2.5 x 2^-24 per element and exactly 0 at masked pixels.
"""
import copy
import functools

import numpy as np
import pytest
import torch

import loss_metrics_ref as R
from common import build_model
from effi_mvs_plus_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

SMALL = [(5, 7), (11, 13), (21, 27), (43, 53)]
MID = [(16, 20), (32, 40), (64, 80), (128, 160)]
METRIC_SHAPES = {"wave": ((1, 5, 7), {}), "tail": ((1, 37, 50), {}), "blocks": ((2, 128, 160), {}), "empty": ((3, 64, 96), {"empty_image": 1}),
                 "nan": ((2, 37, 50), {"nan_valid": True})}
SETS = {"train": (R.TRAIN_THRES, ()), "test": (R.TEST_THRES, R.TEST_BANDS)}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def mask_form(valid, u8):
    return dev(valid) if u8 else dev(valid.astype(np.float32))


@functools.lru_cache(maxsize=None)
def metric_inputs(name):
    shape, kw = METRIC_SHAPES[name]
    est, gt, valid = R.metrics_case(shape, 50 + len(name), **kw)
    refs = {k: R.metrics_ref(est, gt, valid, *v) for k, v in SETS.items()}
    return est, gt, valid, refs


def check_metrics(got, ref, T):
    scalars, counts, sums = (x.cpu().numpy() for x in got)
    assert np.array_equal(counts, ref["counts"]), (counts, ref["counts"])
    terms = np.concatenate([ref["counts"][:, :1], ref["counts"][:, 1 + T:]], axis=1)
    R.check_sums(sums, ref["sums"], terms, np.abs(ref["sums"]), "sums")
    worst = R.check_scalars(scalars, ref["want"], "scalars")
    print(f"scalars: worst error / bound = {worst:.3f}")


@pytest.mark.parametrize("u8", [True, False], ids=["bool", "float"])
@pytest.mark.parametrize("which", sorted(SETS))
@pytest.mark.parametrize("name", sorted(METRIC_SHAPES))
def test_depth_metrics_table_and_scalars(name, which, u8):
    """Less than one wave, an odd size with a tail, >= 3 workgroups per image, a fully masked image (NaN abs_mean and thresholds, 0
    bands for it), a NaN estimate at a valid pixel (in no threshold and no band; abs_mean NaN); planted e = 0, 0.125, 2, 4, 20 exactly
    and a NaN / Inf estimate at masked pixels in every case."""
    from effi_mvs_plus_amd import ops
    est, gt, valid, refs = metric_inputs(name)
    thr, bands = SETS[which]
    if name == "blocks":
        assert ops.metrics_blocks(est[0].size) >= 3
    got = ops.depth_metrics(dev(est), dev(gt), mask_form(valid, u8), thr, bands)
    check_metrics(got, refs[which], len(thr))
    again = ops.depth_metrics(dev(est), dev(gt), mask_form(valid, u8), thr, bands)
    for a, b in zip(got, again):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))               # bitwise repeatable, NaNs included


def test_metric_functions_keep_the_reference_signatures_and_accumulate():
    """Thres_metrics / AbsDepthError_metrics return the entries of the one-call vector as 0-dim device tensors; depth_scalars(acc=)
    over three calls leaves the fp64 sum of the three fp32 vectors (exactly: three fp64 additions of fp32 values of one magnitude
    carry no rounding beyond 3 x 2^-53)."""
    from effi_mvs_plus_amd import metrics
    est, gt, valid, refs = metric_inputs("tail")
    e, g, m = dev(est), dev(gt), dev(valid)
    thr, bands = SETS["test"]
    full = metrics.depth_scalars(e, g, m, thr, bands)
    assert full.dtype == torch.float32 and full.shape == (1 + len(thr) + len(bands),) and full.is_cuda
    for t_, th in enumerate(thr):
        v = metrics.Thres_metrics(e, g, m, th)
        assert v.dim() == 0 and v.is_cuda and torch.equal(v, full[1 + t_])
    assert torch.equal(metrics.AbsDepthError_metrics(e, g, m), full[0])
    for r_, b in enumerate(bands):
        assert torch.equal(metrics.AbsDepthError_metrics(e, g, m, list(b)), full[1 + len(thr) + r_])
    meter = metrics.DeviceAverageMeter(metrics.TEST_SCALARS.keys, device=DEV)
    vecs = []
    for k in range(3):
        e_k = dev(est + np.float32(0.25 * k))
        vecs.append(metrics.depth_scalars(e_k, g, m, thr, bands, acc=meter.slots("abs_depth_error", len(meter.keys))).double().cpu().numpy())
        meter.tick()
    want = (vecs[0] + vecs[1]) + vecs[2]
    got = meter.data.cpu().numpy()
    assert (np.abs(got - want) <= 3 * 2.0 ** -53 * np.abs(want)).all()
    mean = meter.mean()
    assert list(mean) == list(metrics.TEST_SCALARS.keys) and abs(mean["abs_depth_error"] - want[0] / 3) <= 1e-15 * want[0]


# ------------------------------------------------------------------------------------------------- loss
@functools.lru_cache(maxsize=None)
def loss_inputs(sizes, B, K, empty):
    sizes = SMALL if sizes == "small" else MID
    dloss = R.DLOSS if K == 13 else tuple(min(4, 1 + i * 4 // K) for i in range(K))
    est, gt, mask = R.loss_case(sizes, B, 60 + B + K, K=K, dloss=dloss, empty_output=empty)
    w = R.loss_weights(K)
    valid = [m > 0.5 for m in mask]
    return est, gt, mask, w, valid, R.loss_ref(est, gt, valid, w)


@pytest.mark.parametrize("u8", [False, True], ids=["float", "bool"])
@pytest.mark.parametrize("sizes,B,K,empty", [("small", 1, 13, None), ("mid", 2, 13, None), ("small", 1, 13, 5), ("mid", 2, 13, 12),
                                             ("small", 1, 1, None), ("small", 2, 16, None)])
def test_mvs_loss_forward_and_backward(sizes, B, K, empty, u8):
    """K = 13 outputs with DLOSS over odd sizes (less than a workgroup .. two workgroups and a tail) and over 16x20 .. 128x160 at
    B = 2 (20 workgroups); K = 1 and K = 16; d = +-1 exactly, NaN / Inf estimates at masked pixels in every output; one output
    without a valid pixel: its l_i is NaN (and so the total), its gradient all 0, the other outputs' gradients as without it.
    Backward with grad_total = 1 and 0.37; two runs bitwise equal."""
    from effi_mvs_plus_amd import autograd as A, ops
    est, gt, mask, w, valid, ref = loss_inputs(sizes, B, K, empty)
    by_id = {}
    share = lambda a, f: by_id.setdefault(id(a), f(a))                            # noqa: E731  (outputs of one stage share gt / mask)
    gts = [share(a, dev) for a in gt]
    masks = [share(a, (lambda a: dev(a > 0.5)) if u8 else dev) for a in mask]
    runs = []
    out, count = ops.mvs_loss([dev(a) for a in est], gts, masks, w)                 # the entry itself: [l_0 .. l_{K-1}, total], counts
    assert out.shape == (K + 1,) and count.dtype == torch.int64
    for g in (1.0, 0.37):
        ests = [dev(a).requires_grad_(True) for a in est]
        total, per = A.mvs_loss(ests, gts, masks, w)
        assert total.dim() == 0 and per.shape == (K,)
        (total * g).backward()
        R.check_loss(per.detach().cpu().numpy(), count.cpu().numpy(), float(total.detach()), ref, "loss")
        grads = [e.grad.cpu().numpy() for e in ests]
        worst = R.check_grads(grads, R.loss_grad_ref(est, gt, valid, w, g), valid, f"grad g={g}")
        print(f"g={g}: worst gradient distance {worst:.2f} x 2^-24")
        if empty is not None:
            assert np.isnan(per[empty].item()) and np.isnan(float(total.detach())) and (grads[empty] == 0).all()
        runs.append((total.detach().clone(), per.detach().clone(), grads))
    ests = [dev(a).requires_grad_(True) for a in est]
    total, per = A.mvs_loss(ests, gts, masks, w)
    (total * 0.37).backward()
    assert torch.equal(total.view(torch.int32), runs[1][0].view(torch.int32)) and torch.equal(per.view(torch.int32), runs[1][1].view(torch.int32))
    for a, b in zip(ests, runs[1][2]):
        assert np.array_equal(a.grad.cpu().numpy().view(np.int32), b.view(np.int32))


def stage_dicts(gt, mask, u8=False):
    first = {s: R.DLOSS.index(s) for s in (1, 2, 3, 4)}
    return ({"stage{}".format(s): dev(gt[i]) for s, i in first.items()},
            {"stage{}".format(s): (dev(mask[i] > 0.5) if u8 else dev(mask[i])) for s, i in first.items()})


def test_mvs_loss_fused_has_the_signature_of_mvs_loss():
    from effi_mvs_plus_amd.models import mvs_loss, mvs_loss_fused
    est, gt, mask, w, valid, ref = loss_inputs("mid", 2, 13, None)
    gt_ms, mask_ms = stage_dicts(gt, mask)
    ests = [dev(a).requires_grad_(True) for a in est]
    total, per = mvs_loss_fused(ests, gt_ms, mask_ms, list(R.DLOSS), loss_rate=0.9)
    assert sorted(per) == sorted("l{}".format(i) for i in range(13))
    base = {p._base.data_ptr() if p._base is not None else p.data_ptr() for p in per.values()}
    assert len(base) == 1                                                         # views of one device vector
    R.check_loss(np.array([per["l{}".format(i)].item() for i in range(13)]), ref["count"], float(total.detach()), ref, "fused")
    total.backward()
    clean = [torch.where(dev(v), dev(a), dev(g)).requires_grad_(True) for a, g, v in zip(est, gt, valid)]   # the torch loss needs finite inputs
    want, _ = mvs_loss(clean, gt_ms, mask_ms, list(R.DLOSS), loss_rate=0.9)
    want.backward()
    assert abs(float(total.detach()) - float(want.detach())) <= 1e-5 * float(want.detach())
    for a, b in zip(ests, clean):
        assert float((a.grad - b.grad).abs().max()) <= 1e-5 * float(b.grad.abs().max())


def test_loss_and_metrics_replay_in_a_captured_graph():
    """mvs_loss_fused forward + backward and depth_scalars inside torch.cuda.graph: three replays on changed inputs, each bitwise
    the eager call on the same inputs (no host sync, no data-dependent shape, nothing read from the host)."""
    from effi_mvs_plus_amd import metrics
    from effi_mvs_plus_amd.models import mvs_loss_fused
    est, gt, mask, w, valid, _ = loss_inputs("mid", 2, 13, None)
    gt_ms, mask_ms = stage_dicts(gt, mask)
    DL = list(R.DLOSS)
    thr, bands = SETS["test"]

    def run(ests):
        total, per = mvs_loss_fused(ests, gt_ms, mask_ms, DL)
        grads = torch.autograd.grad(total, ests)
        vec = torch.stack([per["l{}".format(i)] for i in range(13)]).detach()
        sc = metrics.depth_scalars(ests[-1], gt_ms["stage4"], mask_ms["stage4"], thr, bands)
        return total.detach(), vec, grads, sc

    static = [dev(a).requires_grad_(True) for a in est]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(static)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = run(static)
    bits = lambda x: x.contiguous().view(torch.int32)                             # noqa: E731
    for k in range(3):
        new = [dev(np.where(np.isfinite(a), a + np.float32(0.125 * (k + 1)), a).astype(np.float32)) for a in est]
        with torch.no_grad():
            for s, n in zip(static, new):
                s.copy_(n)
        graph.replay()
        torch.cuda.synchronize()
        total, vec, grads, sc = run([n.requires_grad_(True) for n in new])
        assert torch.equal(bits(captured[0]), bits(total)) and torch.equal(bits(captured[1]), bits(vec)) and torch.equal(bits(captured[3]), bits(sc))
        for a, b in zip(captured[2], grads):
            assert torch.equal(bits(a), bits(b))


# ------------------------------------------------------------------------------------------------- the graphed steps
H, W, N = 128, 160, 3


def sample(seed):
    imgs, pm, dv = synth.synth_sample(H, W, N, seed=seed)
    g = torch.Generator().manual_seed(seed)
    gt, mask = {}, {}
    for k, f in (("stage1", 8), ("stage2", 4), ("stage3", 2), ("stage4", 1)):
        gt[k] = (synth.DEPTH_MIN_MM + (synth.DEPTH_MAX_MM - synth.DEPTH_MIN_MM) * torch.rand(1, H // f, W // f, generator=g)).to(DEV)
        mask[k] = (torch.rand(1, H // f, W // f, generator=g) > 0.3).float().to(DEV)
    return imgs.to(DEV), {k: v.to(DEV) for k, v in pm.items()}, dv.to(DEV), gt, mask


def test_graphed_training_step_with_the_fused_loss_and_scalars():
    """GraphedTrainStep(loss_fn=mvs_loss_fused, scalars=TRAIN_SCALARS) on the rig of test_graphed_training_step_replays_the_eager_step:
    three replays against three eager steps with the reference-style ``mvs_loss`` (that test's 2e-4), and step.scalars within the
    scalar bound of the restatement on the step's own last depth map."""
    from effi_mvs_plus_amd import metrics, train_graph
    from effi_mvs_plus_amd.models import mvs_loss, mvs_loss_fused
    net, _ = build_model("8,8,8", seed=4, device=DEV)
    net.train()
    for m in net.modules():
        if isinstance(m, torch.nn.Dropout2d):
            m.p = 0.0
    ref = copy.deepcopy(net)
    DL = list(train_graph.DLOSS)
    samples = [sample(s) for s in (31, 32, 33)]
    lr = 1e-4
    opt_e = torch.optim.AdamW(ref.parameters(), lr=lr, capturable=True)
    eager = []
    for imgs, pm, dv, gt, mask in samples:
        opt_e.zero_grad(set_to_none=True)
        loss, _ = mvs_loss(ref(imgs, pm, dv)["depth"], gt, mask, DL)
        loss.backward()
        opt_e.step()
        eager.append(float(loss))
    opt_g = torch.optim.AdamW(net.parameters(), lr=lr, capturable=True)
    step = train_graph.GraphedTrainStep(net, opt_g, *samples[0], loss_fn=mvs_loss_fused, scalars=metrics.TRAIN_SCALARS)
    for smp, want in zip(samples, eager):
        got = float(step(*smp))
        assert abs(got - want) <= 2e-4 * abs(want), (got, want)
        depth = step.depth_est.cpu().numpy()
        r = R.metrics_ref(depth, smp[3]["stage4"].cpu().numpy(), smp[4]["stage4"].cpu().numpy() > 0.5, *SETS["train"])
        R.check_scalars(step.scalars.cpu().numpy(), r["want"], "step.scalars")


def test_graphed_test_step_averages_on_the_device():
    """GraphedTestStep over three samples: its depth map is bitwise the eager eval forward's; mean() is the average of the
    per-sample restatement values on the step's own outputs within the per-sample bounds (one rounding per scalar and l_i, 2.5 for
    the total) plus 3 x 2^-53 for the fp64 accumulator."""
    from effi_mvs_plus_amd import metrics, train_graph
    net, _ = build_model("8,8,8", seed=4, device=DEV)
    net.eval()
    DL = list(train_graph.DLOSS)
    samples = [sample(s) for s in (41, 42, 43)]
    step = train_graph.GraphedTestStep(net, *samples[0])
    keys = ("depth_loss",) + metrics.TEST_SCALARS.keys + tuple("l{}".format(i) for i in range(13)) + ("loss",)
    want, bound = {k: 0.0 for k in keys}, {k: 0.0 for k in keys}
    w = R.loss_weights(13)
    for imgs, pm, dv, gt, mask in samples:
        loss = step(imgs, pm, dv, gt, mask)
        with torch.no_grad():
            eager = net(imgs, pm, dv)["depth"]
        for a, b in zip(step.outputs["depth"], eager):
            assert torch.equal(a, b)
        est = [d.cpu().numpy() for d in step.outputs["depth"]]
        gts = [gt["stage{}".format(s)].cpu().numpy() for s in DL]
        valid = [mask["stage{}".format(s)].cpu().numpy() > 0.5 for s in DL]
        lr_ = R.loss_ref(est, gts, valid, w)
        R.check_loss(step.per_output.cpu().numpy(), lr_["count"], float(loss), lr_, "sample loss")
        mr = R.metrics_ref(est[-1], gts[-1], valid[-1], *SETS["test"])
        R.check_scalars(step.scalars.cpu().numpy(), mr["want"], "sample scalars")
        vals = dict(zip(metrics.TEST_SCALARS.keys, mr["want"]))
        vals.update({"l{}".format(i): lr_["q"][i] for i in range(13)})
        vals["depth_loss"], vals["loss"] = lr_["q"][12], lr_["total"]
        for k in keys:
            want[k] += vals[k] / 3
            bound[k] += (R.TOTAL_REL * lr_["total_scale"] if k == "loss" else R.SCALAR_REL * abs(vals[k])) / 3
    got = step.mean()
    assert set(got) == set(keys) and step.meter.count == 3
    for k in keys:
        assert abs(got[k] - want[k]) <= bound[k] + 3 * 2.0 ** -53 * abs(want[k]), (k, got[k], want[k], bound[k])
