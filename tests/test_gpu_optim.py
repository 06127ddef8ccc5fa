"""The AdamW step on HIP (csrc/optim.hip, effi_mvs_plus_amd/optim.FusedAdamW) on the GPU: every element of p, exp_avg and
exp_avg_sq inside the interval of tests/optim_ref.py (validated against torch's CPU AdamW in tests/test_optim_host.py), nothing
written outside the tensors, determinism, graph capture with the rate read at replay, torch.optim.AdamW on the same gradients of the
real model, the captured training step, and resuming from torch's state.  No test compares the kernel with itself.
"""
import copy

import pytest
import torch
import torch.nn.functional as F

import optim_ref as R
from common import build_model
from effi_mvs_plus_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CHUNK = 2048                                    # elements per workgroup of csrc/optim.hip (include/effi_mvs_hip.h: effi_adamw_multi_f32)
SIZES = (1, 3, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 5, 0)
GAP = 64                                        # sentinel elements on both sides of every tensor, at least
SENTINEL = 0x7FC0BEEF                           # a NaN pattern: written bitwise, compared bitwise


def _fused(params, **kw):
    from effi_mvs_plus_amd.optim import FusedAdamW
    return FusedAdamW(params, **kw)


class Carved:
    """p, g, exp_avg, exp_avg_sq and step of a list of tensors as views of ONE device buffer, each between sentinel-filled gaps of
    >= GAP elements.  ``offsets``: the element offset (mod 64) of the four arrays' starts: (0, 0, 0, 0) = every view 256-byte
    aligned (what separate allocations are: the allocator hands out 512-byte multiples -- but here with sentinels around them),
    (1, 1, 1, 1) = every view at an odd element, (0, 1, 0, 0) = only the gradient misaligned.  The state is set on the optimizer as
    views of the buffer (``load_state_dict()`` would copy it out of the sentinels' reach; test_resume_from_torch_state loads one)."""

    def __init__(self, sizes, offsets, step_old, seed):
        self.sizes, self.step_old = list(sizes), step_old
        self.host, self.where = [], []                  # per tensor: (p, g, m, v) CPU tensors; element ranges in the buffer
        pos = GAP
        for i, n in enumerate(self.sizes):
            self.host.append(R.make_inputs(n, seed=seed + i, fresh=step_old == 0))
            spans = []
            for off in tuple(offsets) + (0,):           # the fifth: the step counter, one element
                start = (pos + 63) // 64 * 64 + off
                length = n if len(spans) < 4 else 1
                spans.append((start, start + length))
                pos = start + length + GAP
            self.where.append(spans)
        total = pos + GAP
        buf = torch.full((total,), SENTINEL, dtype=torch.int32).view(torch.float32)
        for arrs, spans in zip(self.host, self.where):
            for a, (s, e) in zip(arrs, spans[:4]):
                buf[s:e] = a
            buf[spans[4][0]] = float(step_old)
        self.before = buf.clone()
        self.buf = buf.to(DEV)
        view = lambda k, i: self.buf[self.where[i][k][0]:self.where[i][k][1]]                  # noqa: E731
        self.p = [torch.nn.Parameter(view(0, i)) for i in range(len(self.sizes))]
        for i, p in enumerate(self.p):
            p.grad = view(1, i)
        self.state = [{"step": view(4, i).reshape(()), "exp_avg": view(2, i), "exp_avg_sq": view(3, i)} for i in range(len(self.sizes))]
        for i, p in enumerate(self.p):
            for k, off in enumerate(tuple(offsets)):
                if self.sizes[i]:
                    assert (view(k, i).data_ptr() % 256) == 4 * off

    def optimizer(self, **kw):
        opt = _fused(self.p, **kw)
        for p, st in zip(self.p, self.state):
            opt.state[p] = st                           # views of the buffer: the kernel's writes to the state land between sentinels
        return opt

    def restore(self):
        self.buf.copy_(self.before)

    def check(self, lr, wd, label):
        """Every element against the interval; every sentinel and every gradient element bitwise unchanged."""
        after = self.buf.cpu()
        writable = torch.zeros(after.numel(), dtype=torch.bool)
        worst = 0.0
        for i, (arrs, spans) in enumerate(zip(self.host, self.where)):
            ref = R.adamw_step_ref(*arrs, self.step_old + 1, lr, wd=wd)
            for key, k in (("p", 0), ("exp_avg", 2), ("exp_avg_sq", 3)):
                s, e = spans[k]
                writable[s:e] = True
                n_bad, w = R.outside(after[s:e], ref[key])
                worst = max(worst, w)
                assert n_bad == 0, f"{label}: tensor {i} ({self.sizes[i]} elements) {key}: {n_bad} outside the interval (worst {w:.3f} bounds)"
            s = spans[4][0]
            writable[s] = True
            assert float(after[s]) == self.step_old + 1, f"{label}: tensor {i}: step {float(after[s])}"
        same = after.view(torch.int32) == self.before.view(torch.int32)
        assert bool(same[~writable].all()), f"{label}: {int((~same[~writable]).sum())} elements outside p / exp_avg / exp_avg_sq / step changed"
        return worst


LAYOUTS = {"aligned": (SIZES, (0, 0, 0, 0)), "offset1": (SIZES, (1, 1, 1, 1)), "grad_offset1": (SIZES, (0, 1, 0, 0))}


@pytest.mark.parametrize("layout", sorted(LAYOUTS) + ["second_launch"])
def test_every_element_is_bounded_and_nothing_else_is_written(layout):
    from effi_mvs_plus_amd import ops
    K = ops.adamw_max_tensors()
    if layout == "second_launch":
        # K + 1 tensors: the last one goes into a launch of its own; small sizes dominate, every edge size occurs
        sizes, offsets = [SIZES[i % len(SIZES)] if i % 3 == 0 else (1, 3, 0, 5)[i % 4] for i in range(K)] + [CHUNK + 1], (0, 0, 0, 0)
        assert len(sizes) == K + 1 and set(SIZES) <= set(sizes)
    else:
        sizes, offsets = LAYOUTS[layout]
    worst = 0.0
    for step_old, wd, lr_kind in R.CASES:
        c = Carved(sizes, offsets, step_old, seed=1000 * step_old + 7)
        opt = c.optimizer(lr=R.lr_arg(lr_kind, DEV), betas=R.BETAS, eps=R.ADAM_EPS, weight_decay=wd)
        opt.step()
        torch.cuda.synchronize()
        worst = max(worst, c.check(R.lr_value(lr_kind), wd, f"{layout} step {step_old}->{step_old + 1} wd={wd} lr={lr_kind}"))
    print(f"[{layout}] worst |got - ref| / bound over all cases and elements: {worst:.3f}")


def test_parameter_without_gradient_is_skipped():
    """grad is None between two parameters that have one: bitwise untouched, no state; the neighbours are updated (state created
    lazily by step(), as torch does)."""
    host = [R.make_inputs(n, seed=50 + n, fresh=True) for n in (5, CHUNK + 1, 7)]
    ps = [torch.nn.Parameter(h[0].to(DEV)) for h in host]
    ps[0].grad, ps[2].grad = host[0][1].to(DEV), host[2][1].to(DEV)
    opt = _fused(ps, lr=R.LR, weight_decay=1e-3)
    opt.step()
    assert ps[1] not in opt.state and len(opt.state) == 2
    assert torch.equal(ps[1].detach().cpu().view(torch.int32), host[1][0].view(torch.int32))
    for i in (0, 2):
        ref = R.adamw_step_ref(*host[i], 1, R.LR, wd=1e-3)
        st = opt.state[ps[i]]
        assert st["step"].dim() == 0 and st["step"].dtype == torch.float32 and st["step"].is_cuda and float(st["step"]) == 1.0
        for key, got in (("p", ps[i]), ("exp_avg", st["exp_avg"]), ("exp_avg_sq", st["exp_avg_sq"])):
            assert R.outside(got, ref[key])[0] == 0, (i, key)
        assert torch.equal(ps[i].grad.cpu(), host[i][1])
    # the second step counts on: 2 for the two, still nothing for the one in between
    opt.step()
    assert float(opt.state[ps[0]]["step"]) == 2.0 and ps[1] not in opt.state


def test_deterministic_and_capturable_with_the_rate_read_at_replay():
    c = Carved(SIZES, (0, 0, 0, 0), 1, seed=77)
    lr = torch.tensor(R.LR, dtype=torch.float32, device=DEV)
    opt = c.optimizer(lr=lr, betas=R.BETAS, eps=R.ADAM_EPS, weight_decay=1e-3)
    opt.step()
    first = c.buf.clone()
    c.check(R.lr_value("tensor"), 1e-3, "eager")
    c.restore()
    opt.step()
    assert torch.equal(c.buf.view(torch.int32), first.view(torch.int32))          # bitwise repeatable
    c.restore()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()
    c.restore()
    graph.replay()
    assert torch.equal(c.buf.view(torch.int32), first.view(torch.int32))          # the replay IS the eager step
    graph.replay()                                                                 # a second replay steps on: 2 -> 3
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
        assert torch.equal(after[ms:me].view(torch.int32), first.cpu()[ms:me].view(torch.int32))     # the moments do not depend on the rate


# ---- the real model ---------------------------------------------------------------------------------------------------------------
HYPER = dict(lr=2e-4, betas=R.BETAS, eps=R.ADAM_EPS, weight_decay=1e-3)        # the reference's AdamW (train.py:441, --wd 0.001)


def _small_sample(H, W, N, seed):
    imgs, pm, dv = synth.synth_sample(H, W, N, seed=seed)
    return imgs.to(DEV), {k: v.to(DEV) for k, v in pm.items()}, dv.to(DEV)


def _backward_once(net, imgs, pm, dv, gt, mask):
    from effi_mvs_plus_amd import train_graph
    from effi_mvs_plus_amd.models import mvs_loss
    net.train()
    for p in net.parameters():
        p.grad = None
    loss, _ = mvs_loss(net(imgs, pm, dv)["depth"], gt, mask, list(train_graph.DLOSS))
    loss.backward()


def _model_with_gradients(seed):
    """build_model("8,8,8") at 64 x 96, N = 3 (the shape of test_optimizer_step_reduces_the_loss) after an eval forward (packed
    weights are cached) and one backward."""
    H, W, N = 64, 96, 3
    net, _ = build_model("8,8,8", seed=seed, device=DEV)
    imgs, pm, dv = _small_sample(H, W, N, seed=3)
    net.eval()
    with torch.no_grad():
        target = net(imgs, pm, dv)["depth"][-1]
    gt = {k: F.interpolate((target + 15.0).unsqueeze(1), scale_factor=1 / f, mode="nearest").squeeze(1) if f > 1 else target + 15.0
          for k, f in (("stage1", 8), ("stage2", 4), ("stage3", 2), ("stage4", 1))}
    mask = {k: torch.ones_like(v) for k, v in gt.items()}
    _backward_once(net, imgs, pm, dv, gt, mask)
    return net, (imgs, pm, dv, gt, mask)


def _twin_with_gradients(net):
    twin = copy.deepcopy(net)
    for p, q in zip(net.parameters(), twin.parameters()):
        q.grad = None if p.grad is None else p.grad.detach().clone()
    return twin


def _check_model_step(net, twin, before, step_new, label):
    """net stepped by FusedAdamW, twin by torch's capturable AdamW, from the same ``before`` = [(p, g, m, v)]: the kernel against
    the interval of its own (double) scalars, torch against the interval of the fp32 scalars its capturable step forms (measured:
    at step 1, 58 404 of torch's 759 100 elements lie outside the kernel's interval, 15 269 at step 3 -- its bias corrections are
    1 - pow(fl32(0.999), t) in fp32, 1.3e-5 off at t = 1; the kernel's own worst element is at 0.54 of its bound)."""
    worst = {"fused": 0.0, "torch": 0.0}
    torch_outside_tight, total = 0, 0
    for (name, p), q, (p0, g0, m0, v0) in zip(net.named_parameters(), twin.parameters(), before):
        if g0 is None:
            assert torch.equal(p.detach(), p0) and torch.equal(q.detach(), p0), name
            continue
        for who, got, scalars in (("fused", p, "double"), ("torch", q, "fp32")):
            ref = R.adamw_step_ref(p0, g0, m0, v0, step_new, HYPER["lr"], wd=HYPER["weight_decay"], scalars=scalars, normal_only=False)
            n_bad, w = R.outside(got, ref["p"])
            worst[who] = max(worst[who], w)
            assert n_bad == 0, f"{label}: {name} ({who}): {n_bad} of {p.numel()} elements outside the interval (worst {w:.3f} bounds)"
            if who == "fused":                        # for the record only: torch's capturable step against the kernel's interval
                torch_outside_tight += R.outside(q, ref["p"])[0]
                total += p.numel()
    print(f"[{label}] worst |got - ref| / bound: FusedAdamW {worst['fused']:.3f}, torch capturable AdamW {worst['torch']:.3f} "
          f"(of its own interval; {torch_outside_tight} of its {total} elements lie outside the kernel's)")


def test_same_gradients_two_optimizers_on_the_real_model_and_the_pack_cache():
    net, (imgs, pm, dv, gt, mask) = _model_with_gradients(seed=21)
    twin = _twin_with_gradients(net)
    before = [(p.detach().clone(), None if p.grad is None else p.grad.detach().clone(), torch.zeros_like(p), torch.zeros_like(p))
              for p in net.parameters()]
    assert sum(b[1] is not None for b in before) > 200
    opt_f = _fused(net.parameters(), **HYPER)
    opt_t = torch.optim.AdamW(twin.parameters(), capturable=True, **HYPER)
    opt_f.step()
    opt_t.step()
    _check_model_step(net, twin, before, 1, "real model, step 1")
    for p in net.parameters():
        if p.grad is not None:
            assert float(opt_f.state[p]["step"]) == 1.0
    # the pack cache: the stepped model's eval forward is that of a fresh model with its weights, bit for bit
    net.eval()
    with torch.no_grad():
        got = net(imgs, pm, dv)["depth"]
    fresh, _ = build_model("8,8,8", seed=99, device=DEV)
    fresh.load_state_dict(net.state_dict())
    fresh.eval()
    with torch.no_grad():
        want = fresh(imgs, pm, dv)["depth"]
    for a, b in zip(got, want):
        assert torch.equal(a, b)


def test_resume_from_torch_state():
    """Two eager steps of torch.optim.AdamW, its state_dict() into a FusedAdamW, a third step of both on the same gradients."""
    net, (imgs, pm, dv, gt, mask) = _model_with_gradients(seed=22)
    twin = copy.deepcopy(net)                                         # (a stepped model holds cached views: copy it before)
    opt_t0 = torch.optim.AdamW(net.parameters(), capturable=True, **HYPER)
    opt_t0.step()
    _backward_once(net, imgs, pm, dv, gt, mask)
    opt_t0.step()
    _backward_once(net, imgs, pm, dv, gt, mask)
    twin.load_state_dict(net.state_dict())
    for p, q in zip(net.parameters(), twin.parameters()):
        assert torch.equal(p, q)
        q.grad = None if p.grad is None else p.grad.detach().clone()
    opt_f = _fused(net.parameters())                                  # other hyper-parameters: the checkpoint's must win
    opt_f.load_state_dict(copy.deepcopy(opt_t0.state_dict()))
    opt_t = torch.optim.AdamW(twin.parameters(), capturable=True)
    opt_t.load_state_dict(copy.deepcopy(opt_t0.state_dict()))
    assert opt_f.param_groups[0]["lr"] == HYPER["lr"] and opt_f.param_groups[0]["weight_decay"] == HYPER["weight_decay"]
    before = []
    for p in net.parameters():
        st = opt_f.state.get(p)
        if p.grad is None:
            before.append((p.detach().clone(), None, None, None))
            continue
        assert float(st["step"]) == 2.0
        before.append((p.detach().clone(), p.grad.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone()))
    opt_f.step()
    opt_t.step()
    _check_model_step(net, twin, before, 3, "resume, step 3")
    for p, q in zip(net.parameters(), twin.parameters()):
        if p.grad is not None:
            assert float(opt_f.state[p]["step"]) == 3.0 and float(opt_t.state[q]["step"]) == 3.0


def test_graphed_training_step_with_the_fused_optimizer():
    """GraphedTrainStep(net, FusedAdamW) at 128 x 160, N = 3, dropout 0: three replays on three samples against three eager steps of
    torch.optim.AdamW(capturable=True) on a copy, with the tolerances of
    test_gpu_train.py::test_graphed_training_step_replays_the_eager_step (graph against eager)."""
    from effi_mvs_plus_amd import train_graph
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
        imgs, pm, dv = _small_sample(H, W, N, seed)
        g = torch.Generator().manual_seed(seed)
        gt, mask = {}, {}
        for k, f in (("stage1", 8), ("stage2", 4), ("stage3", 2), ("stage4", 1)):
            gt[k] = (synth.DEPTH_MIN_MM + (synth.DEPTH_MAX_MM - synth.DEPTH_MIN_MM) * torch.rand(1, H // f, W // f, generator=g)).to(DEV)
            mask[k] = (torch.rand(1, H // f, W // f, generator=g) > 0.3).float().to(DEV)
        return imgs, pm, dv, gt, mask

    samples = [sample(s) for s in (31, 32, 33)]
    lr = 1e-4
    opt_e = torch.optim.AdamW(ref.parameters(), lr=lr, capturable=True)
    eager = []
    for imgs, pm, dv, gt, mask in samples:
        opt_e.zero_grad(set_to_none=True)
        loss, _ = mvs_loss_static(ref(imgs, pm, dv)["depth"], gt, mask, DL)
        loss.backward()
        opt_e.step()
        eager.append(float(loss.detach()))
    opt_g = _fused(net.parameters(), lr=lr)
    step = train_graph.GraphedTrainStep(net, opt_g, *samples[0])
    assert torch.is_tensor(opt_g.param_groups[0]["lr"])                # converted in place, as for torch's optimizer
    nbt0 = int(net.feature.conv0[0].bn.num_batches_tracked)
    got = [float(step(*smp).detach()) for smp in samples]
    for a, b in zip(got, eager):
        assert abs(a - b) <= 2e-4 * abs(b), (got, eager)
    assert int(net.feature.conv0[0].bn.num_batches_tracked) == nbt0 + 3 * N
    worst = max(float((p - q).abs().max()) for p, q in zip(net.parameters(), ref.parameters()))
    assert worst <= 3 * 3 * lr
    close = sum(int(((p - q).abs() <= 0.05 * lr).sum()) for p, q in zip(net.parameters(), ref.parameters()))
    total = sum(p.numel() for p in net.parameters())
    assert close >= 0.97 * total, (close, total)
    for (k, a), (_, b) in zip(net.named_buffers(), ref.named_buffers()):
        if a.dtype.is_floating_point:
            assert float((a - b).abs().max()) <= 1e-4 * max(1.0, float(b.abs().max())), k
    steps = {float(st["step"]) for st in opt_g.state.values()}
    assert steps == {3.0}, steps                                       # warm-up and capture were undone: three replays, step 3
