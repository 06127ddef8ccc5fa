"""CPU-side checks of gradient clipping and the non-finite guard of FusedAdamW (csrc/optim.hip, effi_mvs_plus_amd/optim.py); no GPU
needed:

  1. the entries are declared in the header and bound with the expected arities; the table fits the kernel argument;
  2. the helper tests/clip_ref.py is validated against torch.nn.utils.clip_grad_norm_(foreach=False) on CPU tensors: torch's norm is
     an admissible value, its scaled gradients are fl32(g * coef) to within one rounding of the coefficient (parity with torch is
     by interval, never bitwise: 8 of the 9 cases below were bitwise equal when this was written, max_norm 0.37 at step 0 was not);
  3. a FusedAdamW with the options set exchanges state dicts with torch.optim.AdamW and carries no new key;
  4. the refusals.
"""
import copy
import math

import numpy as np
import pytest
import torch

import clip_ref as CR
import optim_ref as R

from effi_mvs_plus_amd import _lib, ops
from effi_mvs_plus_amd.optim import FusedAdamW


def test_entries_are_declared_and_bound():
    arity = {"effi_gradnorm_max_tensors": 0, "effi_gradnorm_chunks": 2, "effi_gradnorm_partial_f32": 5, "effi_gradnorm_finish_f32": 6,
             "effi_adamw_multi_clip_f32": 16}
    assert set(arity) <= set(_lib.SIGNATURES) and set(arity) <= set(_lib.declared_symbols())
    for name, n in arity.items():
        assert len(_lib.SIGNATURES[name]) == n, name
    assert len(_lib.SIGNATURES["effi_adamw_multi_clip_f32"]) == len(_lib.SIGNATURES["effi_adamw_multi_f32"]) + 2
    K = ops.gradnorm_max_tensors()                      # host-only query
    assert 1 <= K and K * 20 < 4096                     # a pointer, a size and a chunk count per tensor, by value
    from effi_mvs_plus_amd import optim
    assert callable(optim.grad_norm)


def test_chunk_count_is_host_only():
    import ctypes as C
    L = _lib.lib()
    sizes = list(CR.SIZES)
    assert L.effi_gradnorm_chunks((C.c_long * len(sizes))(*sizes), len(sizes)) == sum((s + 2047) // 2048 for s in sizes) == 10
    assert L.effi_gradnorm_chunks(None, 0) == 0
    assert L.effi_gradnorm_chunks((C.c_long * 1)(-1), 1) == -1
    many = [2049] * (2 * ops.gradnorm_max_tensors() + 1)
    assert L.effi_gradnorm_chunks((C.c_long * len(many))(*many), len(many)) == 2 * len(many)


def test_admissible_norms_and_the_coefficient():
    exact = 12345.678901234
    adm = CR.admissible_norms(exact)
    assert 2 <= len(adm) <= 3 and np.float32(exact) in adm
    assert all(abs(float(a) - exact) <= float(np.spacing(np.float32(exact))) for a in adm)
    assert CR.is_admissible(np.float32(exact), exact) and not CR.is_admissible(np.float32(exact * (1 + 4e-7)), exact)
    assert CR.admissible_norms(0.0) == [np.float32(0.0)] or np.float32(0.0) in CR.admissible_norms(0.0)
    assert np.isinf(CR.admissible_norms(4.2e38)[0]) and len(CR.admissible_norms(4.2e38)) == 1
    assert CR.coef_ref(np.float32(0.5), 1.0) == np.float32(1.0)                    # clamped
    assert CR.coef_ref(np.float32(0.0), math.inf) == np.float32(1.0)
    assert CR.coef_ref(np.float32(np.inf), 1.0) == np.float32(0.0)
    assert np.isnan(CR.coef_ref(np.float32(np.nan), 1.0)) and np.isnan(CR.coef_ref(np.float32(np.inf), math.inf))
    assert CR.coef_ref(np.float32(4.0), 1.0) == np.float32(1.0) / (np.float32(4.0) + np.float32(1e-6))
    g = torch.tensor([1.0, -3.0, 1e-12])
    assert torch.equal(CR.scaled(g, np.float32(1.0)), g)                           # a coefficient of one leaves g bitwise


@pytest.mark.parametrize("max_norm", CR.MAX_NORMS)
@pytest.mark.parametrize("step_old", R.STEPS)
def test_torch_cpu_clip_grad_norm_agrees_with_the_helper(step_old, max_norm):
    grads = [R.make_inputs(n, seed=1000 * step_old + 7 + i, fresh=step_old == 0)[1] for i, n in enumerate(CR.SIZES)]
    exact = CR.exact_norm(grads)
    assert 1.2e4 < exact < 1.4e4                        # all three max_norm values clip
    ps = [torch.nn.Parameter(torch.zeros(n)) for n in CR.SIZES]
    for p, g in zip(ps, grads):
        p.grad = g.clone()
    norm_t = torch.nn.utils.clip_grad_norm_(ps, max_norm, foreach=False)
    assert norm_t.dtype == torch.float32
    assert CR.is_admissible(norm_t.numpy(), exact), (float(norm_t), exact)
    coef = CR.coef_ref(norm_t.numpy(), max_norm)
    assert coef < 1
    bitwise = True
    for p, g in zip(ps, grads):
        want = g.double().numpy() * float(coef)
        got = p.grad.double().numpy()
        # torch forms max_norm / x as reciprocal(x) * max_norm: one rounding more than the division, which moves its coefficient to
        # a neighbouring fp32 value at most (1 ulp <= 2 x 2^-24 relative); then the rounding of the product itself
        assert np.all(np.abs(got - want) <= 3 * R.EPS32 * np.abs(want) + 2.0 ** -149)
        bitwise &= torch.equal(p.grad, CR.scaled(g, coef))
    print(f"step_old {step_old} max_norm {max_norm}: torch norm {float(norm_t)!r}, exact {exact!r}, scaled gradients bitwise fl32(g coef): {bitwise}")


def test_clipped_reference_is_not_vacuous():
    """The interval of the clipped step excludes the unclipped step and a step with a coefficient 1e-3 off."""
    p, g, m, v = R.make_inputs(4099, seed=1007, fresh=False)
    coef = CR.coef_ref(np.float32(CR.exact_norm([g])), 1.0)
    ref = CR.clipped_step_ref(p, g, m, v, coef, 2, R.LR, wd=1e-3)
    unclipped = R.adamw_step_ref(p, g, m, v, 2, R.LR, wd=1e-3)
    off = CR.clipped_step_ref(p, g, m, v, np.float32(float(coef) * 1.001), 2, R.LR, wd=1e-3)
    for key in ("exp_avg", "exp_avg_sq"):               # (where the old moment dwarfs the gradient, no coefficient shows)
        assert R.outside(torch.from_numpy(unclipped[key][0]).float(), ref[key])[0] > 4099 // 4
        assert R.outside(torch.from_numpy(off[key][0]).float(), ref[key])[0] > 4099 // 4
    # and the walk with a bounded gradient reduces to the plain one when the bound is zero
    gs = CR.scaled(g, coef)
    same = CR.adamw_step_ref_g(p, gs.double().numpy(), np.zeros(4099), m, v, 2, R.LR, wd=1e-3)
    plain = R.adamw_step_ref(p, gs, m, v, 2, R.LR, wd=1e-3, normal_only=False)
    for key in plain:
        assert np.array_equal(same[key][0], plain[key][0]) and np.allclose(same[key][1], plain[key][1], rtol=1e-12, atol=0)


def _two_torch_steps():
    torch.manual_seed(3)
    ps = [torch.nn.Parameter(torch.randn(5, 3)), torch.nn.Parameter(torch.randn(7)), torch.nn.Parameter(torch.randn(2, 2))]
    opt = torch.optim.AdamW(ps, lr=2e-4, weight_decay=1e-3, eps=1e-8)
    for _ in range(2):
        for p in ps[:2]:
            p.grad = torch.randn_like(p)
        opt.step()
    return ps, opt


def test_state_dict_carries_no_new_key_and_round_trips():
    ps, topt = _two_torch_steps()
    keys = set(topt.param_groups[0])
    fused = FusedAdamW(ps, max_grad_norm=1.0, skip_nonfinite=True)
    assert fused.max_grad_norm == 1.0 and fused.skip_nonfinite is True
    assert set(fused.param_groups[0]) == keys and set(fused.defaults) == set(FusedAdamW(ps).defaults)
    assert fused.grad_norm is None and fused.clip_coef is None and fused.skipped_steps is None      # before the first step
    fused.load_state_dict(copy.deepcopy(topt.state_dict()))
    assert fused.max_grad_norm == 1.0 and fused.skip_nonfinite is True                              # loading leaves the options alone
    sd = fused.state_dict()
    assert set(sd) == {"state", "param_groups"} and set(sd["param_groups"][0]) == keys
    for st in sd["state"].values():
        assert sorted(st) == ["exp_avg", "exp_avg_sq", "step"]
    back = torch.optim.AdamW(ps)
    back.load_state_dict(copy.deepcopy(sd))
    assert set(back.param_groups[0]) == keys and back.param_groups[0]["lr"] == 2e-4
    for i, st in topt.state_dict()["state"].items():
        for k, x in st.items():
            assert torch.equal(torch.as_tensor(x).float(), back.state_dict()["state"][i][k].float()), (i, k)
    plain = FusedAdamW(ps)
    assert plain.max_grad_norm is None and plain.skip_nonfinite is False
    assert FusedAdamW(ps, max_grad_norm=math.inf).max_grad_norm == math.inf and FusedAdamW(ps, max_grad_norm=0).max_grad_norm == 0.0


def test_refusals():
    from effi_mvs_plus_amd._lib import EffiLibraryError
    from effi_mvs_plus_amd import optim
    p = torch.nn.Parameter(torch.ones(3))
    for bad in (-1.0, float("nan"), -math.inf):
        with pytest.raises(ValueError, match="max_grad_norm"):
            FusedAdamW([p], max_grad_norm=bad)
        with pytest.raises(ValueError, match="max_norm"):
            ops.grad_norm_multi([torch.ones(3)], max_norm=bad)
    # no eager fall-back: the options with parameters on the CPU raise at the step, and nothing moves
    for kw in (dict(max_grad_norm=1.0), dict(skip_nonfinite=True), dict(max_grad_norm=0.5, skip_nonfinite=True)):
        opt = FusedAdamW([p], lr=0.1, **kw)
        p.grad = torch.ones(3)
        with pytest.raises(EffiLibraryError):
            opt.step()
        assert torch.equal(p.detach(), torch.ones(3)) and torch.equal(p.grad, torch.ones(3))
    with pytest.raises(EffiLibraryError):
        optim.grad_norm([p])
    with pytest.raises(ValueError, match="no parameter has a gradient"):
        optim.grad_norm([torch.nn.Parameter(torch.ones(2))])
    with pytest.raises(ValueError, match="skip_nonfinite"):
        ops.adamw_multi([], [], [], [], [], 1e-3, 0.9, 0.999, 1e-8, 0.0, clip=None, skip_nonfinite=True)
    with pytest.raises(ValueError, match="empty list"):
        ops.grad_norm_multi([])
    # a step without gradients launches nothing and creates nothing, with or without the options
    q = torch.nn.Parameter(torch.ones(3))
    opt = FusedAdamW([q], max_grad_norm=1.0, skip_nonfinite=True)
    assert opt.step() is None and len(opt.state) == 0 and opt.skipped_steps is None
