"""CPU-side checks of the AdamW step on HIP (csrc/optim.hip, effi_mvs_plus_amd/optim.py); no GPU needed:

  1. the entry is declared in the header and bound with the expected arity;
  2. the bound of tests/optim_ref.py is validated: torch.optim.AdamW(foreach=False) on CPU fp32 tensors lies inside the interval for
     every element of p, exp_avg and exp_avg_sq in every case -- so the interval the GPU tests hold the kernel to is one that a
     correct fp32 AdamW fits;
  3. state dicts travel between torch.optim.AdamW and FusedAdamW in both directions;
  4. the refusals (amsgrad, CPU step) and the slicing of a long tensor list into launches.
"""
import copy

import pytest
import torch

import optim_ref as R

from effi_mvs_plus_amd import _lib, ops
from effi_mvs_plus_amd.optim import FusedAdamW

NUMEL = 4099


def test_entry_is_declared_and_bound():
    names = {"effi_adamw_max_tensors", "effi_adamw_multi_f32"}
    assert names <= set(_lib.SIGNATURES) and names <= set(_lib.declared_symbols())
    assert len(_lib.SIGNATURES["effi_adamw_multi_f32"]) == 14 and _lib.SIGNATURES["effi_adamw_max_tensors"] == []
    from effi_mvs_plus_amd import train_graph
    assert train_graph.FusedAdamW is FusedAdamW
    K = ops.adamw_max_tensors()                         # host-only query
    assert 1 <= K and K * 56 < 4096                     # five pointers, a size and a chunk count per tensor, by value


def _torch_cpu_step(step_old, wd, lr_kind, p0, g, m0, v0):
    p = torch.nn.Parameter(p0.clone())
    opt = torch.optim.AdamW([p], lr=R.lr_arg(lr_kind), betas=R.BETAS, eps=R.ADAM_EPS, weight_decay=wd, foreach=False)
    if step_old > 0:
        sd = opt.state_dict()
        sd["state"] = {0: {"step": torch.tensor(float(step_old)), "exp_avg": m0.clone(), "exp_avg_sq": v0.clone()}}
        opt.load_state_dict(sd)
    p.grad = g.clone()
    opt.step()
    st = opt.state[p]
    assert float(st["step"]) == step_old + 1
    return p.detach(), st["exp_avg"], st["exp_avg_sq"]


@pytest.mark.parametrize("step_old,wd,lr_kind", R.CASES)
def test_torch_cpu_adamw_lies_inside_the_interval(step_old, wd, lr_kind):
    p0, g, m0, v0 = R.make_inputs(NUMEL, seed=100 + step_old, fresh=step_old == 0)
    ref = R.adamw_step_ref(p0, g, m0, v0, step_old + 1, R.lr_value(lr_kind), wd=wd)
    p1, m1, v1 = _torch_cpu_step(step_old, wd, lr_kind, p0, g, m0, v0)
    for key, got in (("p", p1), ("exp_avg", m1), ("exp_avg_sq", v1)):
        n_bad, worst = R.outside(got, ref[key])
        print(f"step {step_old}->{step_old + 1} wd={wd} lr={lr_kind} {key}: worst |got - ref| / bound = {worst:.3f}")
        assert n_bad == 0, f"{key}: {n_bad} of {NUMEL} elements outside the interval (worst {worst:.3f} bounds)"
    # the interval is not vacuous: an update with the OLD step's bias corrections, or without the decay, leaves it
    if lr_kind != "zero":
        wrong = R.adamw_step_ref(p0, g, m0, v0, step_old + 2, R.lr_value(lr_kind), wd=wd)["p"][0]
        assert R.outside(torch.from_numpy(wrong).float(), ref["p"])[0] > NUMEL // 4
        if wd:
            undecayed = R.adamw_step_ref(p0, g, m0, v0, step_old + 1, R.lr_value(lr_kind), wd=0.0)["p"][0]
            assert R.outside(torch.from_numpy(undecayed).float(), ref["p"])[0] > NUMEL // 4


def test_bias_correction_one_underflows_at_step_1001():
    """What the 1000 -> 1001 case is for: beta1^1001 is below half an ulp of 1, beta2^1001 is not."""
    import numpy as np
    assert np.float32(1.0 - R.BETAS[0] ** 1001) == np.float32(1.0) and np.float32(1.0 - R.BETAS[1] ** 1001) < np.float32(0.7)


def _two_torch_steps():
    torch.manual_seed(3)
    ps = [torch.nn.Parameter(torch.randn(5, 3)), torch.nn.Parameter(torch.randn(7)), torch.nn.Parameter(torch.randn(2, 2))]
    opt = torch.optim.AdamW(ps, lr=2e-4, weight_decay=1e-3, eps=1e-8)
    for _ in range(2):
        for p in ps[:2]:                                # the third parameter never gets a gradient: no state
            p.grad = torch.randn_like(p)
        opt.step()
    return ps, opt


def _assert_same_state(a, b):
    sa, sb = a.state_dict()["state"], b.state_dict()["state"]
    assert sorted(sa) == sorted(sb) == [0, 1]
    for i in sa:
        assert sorted(sa[i]) == sorted(sb[i]) == ["exp_avg", "exp_avg_sq", "step"]
        for k in sa[i]:
            assert torch.is_tensor(sb[i][k]) and sb[i][k].dtype == torch.float32
            assert torch.equal(sa[i][k].cpu(), sb[i][k].cpu()), (i, k)


def test_state_dict_round_trip_with_torch_adamw():
    ps, topt = _two_torch_steps()
    keys = set(topt.param_groups[0])
    fused = FusedAdamW(ps)
    assert set(fused.param_groups[0]) == keys            # before loading
    g0 = fused.param_groups[0]
    assert (g0["lr"], g0["betas"], g0["eps"], g0["weight_decay"]) == (1e-3, (0.9, 0.999), 1e-8, 1e-2)      # torch.optim.AdamW's defaults
    assert g0["capturable"] is True and g0["amsgrad"] is False and g0["maximize"] is False and g0["foreach"] is None
    assert g0["fused"] is None and g0["differentiable"] is False
    fused.load_state_dict(copy.deepcopy(topt.state_dict()))
    assert set(fused.param_groups[0]) == keys
    g1 = fused.param_groups[0]
    assert (g1["lr"], g1["weight_decay"], g1["eps"], g1["capturable"]) == (2e-4, 1e-3, 1e-8, True)
    _assert_same_state(topt, fused)
    for p in ps[:2]:
        st = fused.state[p]
        assert st["step"].dim() == 0 and st["step"].device == p.device and float(st["step"]) == 2.0
    assert ps[2] not in fused.state
    # and back into a fresh torch.optim.AdamW
    back = torch.optim.AdamW(ps)
    back.load_state_dict(copy.deepcopy(fused.state_dict()))
    assert set(back.param_groups[0]) == keys
    _assert_same_state(fused, back)
    assert back.param_groups[0]["lr"] == 2e-4 and back.param_groups[0]["weight_decay"] == 1e-3


def test_amsgrad_and_maximize_are_refused():
    p = torch.nn.Parameter(torch.zeros(3))
    with pytest.raises(NotImplementedError, match="not on the HIP path"):
        FusedAdamW([p], amsgrad=True)
    with pytest.raises(NotImplementedError, match="not on the HIP path"):
        FusedAdamW([p], maximize=True)
    opt = FusedAdamW([p])
    opt.param_groups[0]["amsgrad"] = True
    p.grad = torch.ones(3)
    with pytest.raises(NotImplementedError, match="not on the HIP path"):
        opt.step()


def test_cpu_step_is_refused():
    """No eager fall-back: parameters on the CPU can be constructed (state dicts), but a step raises."""
    from effi_mvs_plus_amd._lib import EffiLibraryError
    p = torch.nn.Parameter(torch.ones(3))
    opt = FusedAdamW([p], lr=0.1)
    p.grad = torch.ones(3)
    with pytest.raises(EffiLibraryError):
        opt.step()
    assert torch.equal(p.detach(), torch.ones(3))
    p64 = torch.nn.Parameter(torch.ones(3, dtype=torch.float64))
    p64.grad = torch.ones(3, dtype=torch.float64)
    with pytest.raises(TypeError):
        FusedAdamW([p64]).step()
    p.grad = torch.ones(3).to_sparse()
    with pytest.raises(RuntimeError, match="sparse"):
        opt.step()


def test_a_step_without_gradients_does_nothing():
    p = torch.nn.Parameter(torch.ones(3))
    opt = FusedAdamW([p])
    assert opt.step() is None and len(opt.state) == 0
    assert opt.step(lambda: torch.tensor(2.5)) == 2.5


def test_slices_cover_a_long_list_in_order():
    K = ops.adamw_max_tensors()
    for n in (1, K - 1, K, K + 1, 2 * K + 3):
        sl = ops._adamw_slices(n, K)
        assert all(0 < e - s <= K for s, e in sl)
        assert [i for s, e in sl for i in range(s, e)] == list(range(n))
        assert len(sl) == (n + K - 1) // K
    assert ops._adamw_slices(0, K) == []
