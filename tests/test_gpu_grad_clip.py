"""Gradient clipping by global norm and the non-finite guard of FusedAdamW on the GPU (csrc/optim.hip: gradnorm_partial_kernel,
gradnorm_finish_kernel, the CLIP instantiations of the AdamW kernels).  The reference is tests/clip_ref.py (validated against torch
on the CPU in tests/test_grad_clip_host.py): the returned norm must be an admissible fp32 value of the exact norm, the returned
coefficient the formula of that value bitwise, and every element of p, exp_avg and exp_avg_sq inside the interval of
tests/optim_ref.py for the gradient g' = fl32(g * coef).  Buffers are carved out of one allocation between sentinels
(test_gpu_optim.Carved), so a write outside a tensor shows.  No test compares the kernels with themselves.
"""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import clip_ref as CR
import optim_ref as R
import test_gpu_optim as T
from common import build_model

pytestmark = pytest.mark.gpu
DEV = T.DEV
CHUNK = T.CHUNK
SIZES = T.SIZES
assert tuple(SIZES) == CR.SIZES
DSENT = 0x7FF8DEADBEEF0001                      # a NaN pattern for the fp64 workspace: written and compared bitwise


class ClipCarved(T.Carved):
    def grads(self):
        return [h[1] for h in self.host]

    def check_clipped(self, coef, lr, wd, label):
        """Carved.check with every tensor's gradient replaced by g' = fl32(g * coef) in the reference (the buffer's gradient spans
        are still compared bitwise with what was uploaded: the kernel must not scale g in memory)."""
        host = self.host
        self.host = [(p, CR.scaled(g, coef), m, v) for p, g, m, v in host]
        try:
            return self.check(lr, wd, label)
        finally:
            self.host = host

    def grad_span(self, i):
        return self.where[i][1]


def _chain(opt, exact, max_norm, label):
    """The norm and coefficient a step left on the device: admissible, and the formula's value bitwise.  -> the coefficient."""
    norm, coef = opt.grad_norm.cpu().numpy(), opt.clip_coef.cpu().numpy()
    assert opt.grad_norm.dim() == 0 and opt.clip_coef.dim() == 0 and opt.grad_norm.dtype == torch.float32
    assert CR.is_admissible(norm, exact), f"{label}: norm {float(norm)!r} is not within one fp32 ulp of {exact!r}"
    want = CR.coef_ref(norm, max_norm)
    assert CR.same_bits(coef, want), f"{label}: coefficient {float(coef)!r}, the formula gives {float(want)!r}"
    return np.float32(coef)


def _second_launch_sizes(K):
    sizes = [SIZES[i % len(SIZES)] if i % 3 == 0 else (1, 3, 0, 5)[i % 4] for i in range(K)] + [CHUNK + 1]
    assert len(sizes) == K + 1 and set(SIZES) <= set(sizes)
    return sizes


# ---- 1. the norm alone ----------------------------------------------------------------------------------------------------------
def _raw_norm(c, max_norm):
    """The three entries called as ops.grad_norm_multi calls them, with the partial workspace carved between sentinels.
    -> (clip [4] CPU, workspace as int64 CPU, first slot, number of slots)."""
    from effi_mvs_plus_amd import _lib, ops
    L = _lib.lib()
    K = ops.gradnorm_max_tensors()
    n = len(c.sizes)
    ptrs = [c.buf[s:e].data_ptr() if e > s else c.buf.data_ptr() for (s, e) in (c.grad_span(i) for i in range(n))]
    total = int(L.effi_gradnorm_chunks((C.c_long * n)(*c.sizes), n))
    pad = 16
    work = torch.full((total + 2 * pad,), DSENT, dtype=torch.int64, device=DEV)
    clip = torch.full((4 + 2 * pad,), T.SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32)
    st = ops._stream()
    base = 0
    for s in range(0, n, K):
        e = min(n, s + K)
        sizes = (C.c_long * (e - s))(*c.sizes[s:e])
        _lib.check(L.effi_gradnorm_partial_f32((C.c_void_p * (e - s))(*ptrs[s:e]), sizes, e - s, C.c_void_p(work.data_ptr() + 8 * (pad + base)), st),
                   "effi_gradnorm_partial_f32")
        base += int(L.effi_gradnorm_chunks(sizes, e - s))
    assert base == total
    _lib.check(L.effi_gradnorm_finish_f32(C.c_void_p(work.data_ptr() + 8 * pad), total, float(max_norm), C.c_void_p(clip.data_ptr() + 4 * pad),
                                          None, st), "effi_gradnorm_finish_f32")
    torch.cuda.synchronize()
    return clip.cpu(), work.cpu(), pad, total


@pytest.mark.parametrize("layout", ["aligned", "offset1", "second_launch"])
def test_norm_is_admissible_deterministic_and_only_the_workspace_is_written(layout):
    from effi_mvs_plus_amd import ops
    K = ops.gradnorm_max_tensors()
    sizes, offsets = (_second_launch_sizes(K), (0, 0, 0, 0)) if layout == "second_launch" else T.LAYOUTS[layout]
    c = ClipCarved(sizes, offsets, 1, seed=4242)
    exact = CR.exact_norm(c.grads())
    clip, work, pad, total = _raw_norm(c, 1.0)
    assert total == sum((s + CHUNK - 1) // CHUNK for s in sizes)
    ci = clip.view(torch.int32)
    assert bool((ci[:pad] == T.SENTINEL).all()) and bool((ci[pad + 4:] == T.SENTINEL).all())
    assert bool((work[:pad] == DSENT).all()) and bool((work[pad + total:] == DSENT).all())            # nothing beside the slots
    slots = work[pad:pad + total].view(torch.float64)
    assert bool((work[pad:pad + total] != DSENT).all()) and bool(torch.isfinite(slots).all())        # every slot written
    # each slot is the sum of its chunk's exact squares: the double sum of <= 2048 of them is within 2048 x 2^-53 of fsum
    k = 0
    for g in c.grads():
        for i0 in range(0, g.numel(), CHUNK):
            want = CR.exact_norm([g[i0:i0 + CHUNK]]) ** 2
            assert abs(float(slots[k]) - want) <= want * 2.0 ** -40, (k, float(slots[k]), want)
            k += 1
    assert k == total
    norm = clip[pad:pad + 4].numpy()
    assert CR.is_admissible(norm[0], exact), (float(norm[0]), exact)
    assert CR.same_bits(norm[1], CR.coef_ref(norm[0], 1.0)) and norm[2] == 1.0 and norm[3] == 0.0
    print(f"[{layout}] norm {float(norm[0])!r}, exact {exact!r}")
    # gradients, gaps and everything else in the buffer: bitwise as uploaded
    assert torch.equal(c.buf.cpu().view(torch.int32), c.before.view(torch.int32))
    # a second run, and the Python entry on its own workspace: the same bits
    clip2, work2, _, _ = _raw_norm(c, 1.0)
    assert torch.equal(clip2.view(torch.int32), ci) and torch.equal(work2, work)
    views = [c.buf[s:e] for (s, e) in (c.grad_span(i) for i in range(len(sizes)))]
    got = ops.grad_norm_multi(views, 1.0)
    assert got.shape == (4,) and torch.equal(got.cpu().view(torch.int32), ci[pad:pad + 4])
    assert torch.equal(c.buf.cpu().view(torch.int32), c.before.view(torch.int32))


def test_norm_of_nothing_is_zero_and_grad_norm_of_parameters():
    from effi_mvs_plus_amd import ops, optim
    clip = torch.full((4,), 7.0, device=DEV)
    out = ops.grad_norm_multi([], 1.0, clip=clip)
    assert out is clip and clip.tolist() == [0.0, 1.0, 1.0, 0.0]
    empty = [torch.zeros(0, device=DEV), torch.zeros(0, device=DEV)]
    assert ops.grad_norm_multi(empty).tolist() == [0.0, 1.0, 1.0, 0.0]
    # max_norm = inf never clips; 0 clips to nothing
    g = torch.full((5,), 2.0, device=DEV)
    assert ops.grad_norm_multi([g]).tolist()[1:3] == [1.0, 1.0]
    assert ops.grad_norm_multi([g], 0.0).tolist()[1:3] == [0.0, 1.0]
    c = ClipCarved(SIZES, (0, 0, 0, 0), 1, seed=99)
    none = torch.nn.Parameter(torch.ones(3, device=DEV))              # no gradient: left out
    norm = optim.grad_norm(c.p + [none])
    assert norm.dim() == 0 and norm.dtype == torch.float32 and norm.is_cuda
    assert CR.is_admissible(norm.cpu().numpy(), CR.exact_norm(c.grads()))
    assert torch.equal(c.buf.cpu().view(torch.int32), c.before.view(torch.int32))


# ---- 2. the clipped step, every element ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout,max_norm", [("aligned", m) for m in CR.MAX_NORMS] + [("offset1", 0.37), ("grad_offset1", 0.37),
                                                                                      ("second_launch", 0.37)])
def test_clipped_step_every_element_is_bounded(layout, max_norm):
    from effi_mvs_plus_amd import ops
    sizes, offsets = (_second_launch_sizes(ops.adamw_max_tensors()), (0, 0, 0, 0)) if layout == "second_launch" else T.LAYOUTS[layout]
    worst = 0.0
    for step_old, wd, lr_kind in R.CASES:
        label = f"{layout} max_norm={max_norm} step {step_old}->{step_old + 1} wd={wd} lr={lr_kind}"
        c = ClipCarved(sizes, offsets, step_old, seed=1000 * step_old + 7)
        exact = CR.exact_norm(c.grads())
        assert exact > 1e4 * (1 + 1e-3), exact                       # every max_norm of the cases clips
        opt = c.optimizer(lr=R.lr_arg(lr_kind, DEV), betas=R.BETAS, eps=R.ADAM_EPS, weight_decay=wd, max_grad_norm=max_norm)
        opt.step()
        torch.cuda.synchronize()
        coef = _chain(opt, exact, max_norm, label)
        assert coef < 1
        worst = max(worst, c.check_clipped(coef, R.lr_value(lr_kind), wd, label))
        assert int(opt.skipped_steps) == 0 and opt.skipped_steps.dtype == torch.int64 and opt.skipped_steps.dim() == 0
    print(f"[{layout}, max_norm {max_norm}] worst |got - ref| / bound over all cases and elements: {worst:.3f}")


# ---- 3. a step that does not clip is today's step -----------------------------------------------------------------------------
def test_a_step_that_does_not_clip_is_the_unclipped_step_bitwise():
    for offsets in ((0, 0, 0, 0), (1, 1, 1, 1)):
        c = ClipCarved(SIZES, offsets, 1, seed=31)
        hyper = dict(lr=R.LR, betas=R.BETAS, eps=R.ADAM_EPS, weight_decay=1e-3)
        c.optimizer(**hyper).step()
        plain = c.buf.clone()
        assert not torch.equal(plain.cpu().view(torch.int32), c.before.view(torch.int32))
        for kw in (dict(max_grad_norm=1e5), dict(max_grad_norm=None, skip_nonfinite=True), dict(max_grad_norm=1e5, skip_nonfinite=True)):
            c.restore()
            opt = c.optimizer(**hyper, **kw)
            opt.step()
            assert torch.equal(c.buf.view(torch.int32), plain.view(torch.int32)), kw
            assert float(opt.clip_coef) == 1.0 and int(opt.skipped_steps) == 0
            assert CR.is_admissible(opt.grad_norm.cpu().numpy(), CR.exact_norm(c.grads()))


# ---- 4. non-finite gradients ------------------------------------------------------------------------------------------------------
def _poisons(c):
    """(label, [(buffer index, value)]): the first element of the first tensor, the last of the 6149-element one (scalar tail), and
    two elements of 3e38 (the sum of squares is finite in double, the norm is inf in fp32)."""
    big = c.sizes.index(3 * CHUNK + 5)
    first, last = c.grad_span(0)[0], c.grad_span(big)[1] - 1
    out = []
    for name, val in (("inf", float("inf")), ("nan", float("nan"))):
        out.append((f"{name} at the first element", [(first, val)]))
        out.append((f"{name} at the last element of the tail", [(last, val)]))
    out.append(("two elements of 3e38", [(c.grad_span(big)[0], 3e38), (c.grad_span(big)[0] + CHUNK + 1, 3e38)]))
    return out


def test_nonfinite_gradient_skips_the_step_and_the_next_one_steps():
    max_norm, lr, wd = 1.0, R.LR, 1e-3
    c = ClipCarved(SIZES, (0, 0, 0, 0), 1, seed=555)
    exact = CR.exact_norm(c.grads())
    opt = c.optimizer(lr=lr, betas=R.BETAS, eps=R.ADAM_EPS, weight_decay=wd, max_grad_norm=max_norm, skip_nonfinite=True)
    loose = c.optimizer(lr=lr, betas=R.BETAS, eps=R.ADAM_EPS, weight_decay=wd, max_grad_norm=max_norm)            # skip_nonfinite=False
    skipped = 0
    for label, writes in _poisons(c):
        c.restore()
        for idx, val in writes:
            c.buf[idx] = val
        poisoned = c.buf.clone()
        opt.step()
        torch.cuda.synchronize()
        assert torch.equal(c.buf.view(torch.int32), poisoned.view(torch.int32)), f"{label}: a skipped step wrote something"
        skipped += 1
        assert int(opt.skipped_steps) == skipped, label
        norm = opt.grad_norm.cpu().numpy()
        assert not np.isfinite(norm), (label, norm)
        assert CR.same_bits(opt.clip_coef.cpu().numpy(), CR.coef_ref(norm, max_norm)), label
        # without the guard: the coefficient is the formula's (0 for an infinite norm, NaN for NaN), as torch's is; only that is asserted
        loose.step()
        torch.cuda.synchronize()
        ln = loose.grad_norm.cpu().numpy()
        assert not np.isfinite(ln) and CR.same_bits(ln, norm), label
        want = CR.coef_ref(ln, max_norm)
        assert CR.same_bits(loose.clip_coef.cpu().numpy(), want) and (np.isnan(want) or want == 0.0), (label, want)
        assert int(loose.skipped_steps) == skipped, label             # counted there too; nothing was skipped
        # the following clean step is the clipped step from the old counter
        c.restore()
        opt.step()
        torch.cuda.synchronize()
        coef = _chain(opt, exact, max_norm, label)
        c.check_clipped(coef, lr, wd, f"clean step after {label}")
        assert int(opt.skipped_steps) == skipped


# ---- 5. capture -----------------------------------------------------------------------------------------------------------------
def test_captured_guarded_step_replays_skips_and_follows_the_rate():
    max_norm = 0.37
    c = ClipCarved(SIZES, (0, 0, 0, 0), 1, seed=77)
    exact = CR.exact_norm(c.grads())
    lr = torch.tensor(R.LR, dtype=torch.float32, device=DEV)
    opt = c.optimizer(lr=lr, betas=R.BETAS, eps=R.ADAM_EPS, weight_decay=1e-3, max_grad_norm=max_norm, skip_nonfinite=True)
    opt.step()
    first = c.buf.clone()
    c.check_clipped(_chain(opt, exact, max_norm, "eager"), R.lr_value("tensor"), 1e-3, "eager")
    addresses = (opt.grad_norm.data_ptr(), opt.clip_coef.data_ptr(), opt.skipped_steps.data_ptr())
    c.restore()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()
    assert addresses == (opt.grad_norm.data_ptr(), opt.clip_coef.data_ptr(), opt.skipped_steps.data_ptr())
    c.restore()
    graph.replay()
    assert torch.equal(c.buf.view(torch.int32), first.view(torch.int32))          # the replay IS the eager step
    assert int(opt.skipped_steps) == 0
    # a poisoned gradient written between replays: that replay is a no-op ...
    c.restore()
    c.buf[c.grad_span(4)[0] + 7] = float("nan")
    poisoned = c.buf.clone()
    graph.replay()
    assert torch.equal(c.buf.view(torch.int32), poisoned.view(torch.int32))
    assert int(opt.skipped_steps) == 1 and np.isnan(float(opt.grad_norm))
    # ... and the next one, on the clean gradient, a step
    c.buf.copy_(c.before)
    graph.replay()
    assert torch.equal(c.buf.view(torch.int32), first.view(torch.int32))
    assert int(opt.skipped_steps) == 1
    graph.replay()                                                                 # steps on: 2 -> 3
    assert all(float(st["step"]) == 3.0 for st in c.state)
    # a scheduler's fill_ after capture: rate 0 -> p * 1 - 0 exactly, while the moments still move
    c.restore()
    lr.fill_(0.0)
    graph.replay()
    torch.cuda.synchronize()
    after = c.buf.cpu()
    for i, spans in enumerate(c.where):
        if not c.sizes[i]:
            continue
        (ps, pe), (ms, me) = spans[0], spans[2]
        assert torch.equal(after[ps:pe].view(torch.int32), c.before[ps:pe].view(torch.int32)), f"tensor {i}: p moved at rate 0"
        assert not torch.equal(after[ms:me], c.before[ms:me]), f"tensor {i}: exp_avg did not move"
        assert torch.equal(after[ms:me].view(torch.int32), first.cpu()[ms:me].view(torch.int32))


# ---- 6. the real model -----------------------------------------------------------------------------------------------------------
def test_clipped_step_on_the_real_model_beside_torch_clip_grad_norm():
    net, _ = T._model_with_gradients(seed=21)
    twin = T._twin_with_gradients(net)
    before = [(p.detach().clone(), None if p.grad is None else p.grad.detach().clone()) for p in net.parameters()]
    grads = [g for _, g in before if g is not None]
    assert len(grads) > 200
    exact = CR.exact_norm(grads)
    max_norm = 0.5 * exact
    opt_f = T._fused(net.parameters(), max_grad_norm=max_norm, **T.HYPER)
    opt_f.step()
    norm_t = torch.nn.utils.clip_grad_norm_(twin.parameters(), max_norm)
    opt_t = torch.optim.AdamW(twin.parameters(), capturable=True, **T.HYPER)
    opt_t.step()
    torch.cuda.synchronize()
    coef = _chain(opt_f, exact, max_norm, "real model")
    assert coef < 1
    rel_t = abs(float(norm_t) - exact) / exact
    print(f"[real model] exact norm {exact!r}, kernel {float(opt_f.grad_norm)!r}, torch {float(norm_t)!r} (relative error {rel_t:.3e} "
          f"= {rel_t / R.EPS32:.2f} x 2^-24), coefficient {float(coef)!r}")
    worst = {"fused": 0.0, "torch": 0.0}
    for (name, p), q, (p0, g0) in zip(net.named_parameters(), twin.parameters(), before):
        if g0 is None:
            assert torch.equal(p.detach(), p0) and torch.equal(q.detach(), p0), name
            continue
        assert torch.equal(p.grad, g0), f"{name}: the gradient was modified"
        zero = torch.zeros_like(p0)
        ref = CR.clipped_step_ref(p0, g0, zero, zero, coef, 1, T.HYPER["lr"], wd=T.HYPER["weight_decay"], normal_only=False)
        for key, got in (("p", p), ("exp_avg", opt_f.state[p]["exp_avg"]), ("exp_avg_sq", opt_f.state[p]["exp_avg_sq"])):
            n_bad, w = R.outside(got, ref[key])
            worst["fused"] = max(worst["fused"], w)
            assert n_bad == 0, f"{name} {key} (FusedAdamW): {n_bad} of {p.numel()} outside the interval (worst {w:.3f} bounds)"
        assert float(opt_f.state[p]["step"]) == 1.0
        gv, ge, _ = CR.torch_clip_gradient_interval(g0, exact, max_norm, norm_t)
        ref_t = CR.adamw_step_ref_g(p0, gv, ge, zero, zero, 1, T.HYPER["lr"], wd=T.HYPER["weight_decay"], scalars="fp32")
        n_bad, w = R.outside(q, ref_t["p"])
        worst["torch"] = max(worst["torch"], w)
        assert n_bad == 0, f"{name} (clip_grad_norm_ + torch AdamW): {n_bad} of {p.numel()} outside its interval (worst {w:.3f} bounds)"
    print(f"[real model] worst |got - ref| / bound: FusedAdamW {worst['fused']:.3f}, clip_grad_norm_ + torch AdamW {worst['torch']:.3f}")


# ---- 7. the graphed training step ---------------------------------------------------------------------------------------------
def test_graphed_training_step_skips_the_poisoned_sample():
    """GraphedTrainStep(net, FusedAdamW(max_grad_norm, skip_nonfinite=True)) at 128 x 160, N = 3, dropout 0: three replays, the second
    on a sample with one NaN in its ground truth, against an eager copy with clip_grad_norm_ + torch.optim.AdamW that omits step()
    on that sample; tolerances of test_gpu_optim.test_graphed_training_step_with_the_fused_optimizer, for 2 steps."""
    from effi_mvs_plus_amd import synth, train_graph
    from effi_mvs_plus_amd.models.module import mvs_loss_static
    H, W, N = 128, 160, 3
    net, _ = build_model("8,8,8", seed=4, device=DEV)
    net.train()
    for m in net.modules():
        if isinstance(m, torch.nn.Dropout2d):
            m.p = 0.0
    ref = copy.deepcopy(net)
    DL = list(train_graph.DLOSS)

    def sample(seed):
        imgs, pm, dv = T._small_sample(H, W, N, seed)
        g = torch.Generator().manual_seed(seed)
        gt, mask = {}, {}
        for k, f in (("stage1", 8), ("stage2", 4), ("stage3", 2), ("stage4", 1)):
            gt[k] = (synth.DEPTH_MIN_MM + (synth.DEPTH_MAX_MM - synth.DEPTH_MIN_MM) * torch.rand(1, H // f, W // f, generator=g)).to(DEV)
            mask[k] = (torch.rand(1, H // f, W // f, generator=g) > 0.3).float().to(DEV)
        return imgs, pm, dv, gt, mask

    samples = [sample(s) for s in (31, 32, 33)]
    valid = torch.nonzero(samples[1][4]["stage4"][0] > 0)[17]
    samples[1][3]["stage4"][0, valid[0], valid[1]] = float("nan")    # the loss only: images and cameras stay finite
    lr, max_norm = 1e-4, 1.0
    opt_e = torch.optim.AdamW(ref.parameters(), lr=lr, capturable=True)
    eager = []
    for i, (imgs, pm, dv, gt, mask) in enumerate(samples):
        opt_e.zero_grad(set_to_none=True)
        loss, _ = mvs_loss_static(ref(imgs, pm, dv)["depth"], gt, mask, DL)
        loss.backward()
        if i != 1:
            torch.nn.utils.clip_grad_norm_(ref.parameters(), max_norm)
            opt_e.step()
        eager.append(float(loss.detach()))
    assert not np.isfinite(eager[1])
    opt_g = T._fused(net.parameters(), lr=lr, max_grad_norm=max_norm, skip_nonfinite=True)
    step = train_graph.GraphedTrainStep(net, opt_g, *samples[0])
    assert int(opt_g.skipped_steps) == 0                               # warm-up and capture do not count
    got = [float(step(*samples[0]).detach())]
    params_1 = [p.detach().clone() for p in net.parameters()]
    got.append(float(step(*samples[1]).detach()))
    for p, q in zip(net.parameters(), params_1):
        assert torch.equal(p.detach().view(torch.int32), q.view(torch.int32))                      # replay 2 changed no parameter
    assert int(opt_g.skipped_steps) == 1 and not np.isfinite(float(opt_g.grad_norm))
    got.append(float(step(*samples[2]).detach()))
    assert int(opt_g.skipped_steps) == 1 and np.isfinite(float(opt_g.grad_norm))
    assert {float(st["step"]) for st in opt_g.state.values()} == {2.0}
    assert not np.isfinite(got[1])
    for a, b in ((got[0], eager[0]), (got[2], eager[2])):
        assert abs(a - b) <= 2e-4 * abs(b), (got, eager)
    worst = max(float((p.detach() - q.detach()).abs().max()) for p, q in zip(net.parameters(), ref.parameters()))
    assert worst <= 3 * 2 * lr
    close = sum(int(((p.detach() - q.detach()).abs() <= 0.05 * lr).sum()) for p, q in zip(net.parameters(), ref.parameters()))
    total = sum(p.numel() for p in net.parameters())
    assert close >= 0.97 * total, (close, total)
