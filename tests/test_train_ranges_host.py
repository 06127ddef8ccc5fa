"""No GPU: the host side of training on per-sample depth ranges -- the two new C-ABI entries are declared and bound, the graphed
step's ``depth_range`` keyword is validated before anything touches a device, and ``train_epoch`` drives a step in the reference
loop's order (train.py:115-127)."""
import pytest
import torch

from effi_mvs_plus_amd import _lib


def test_ranged_entries_are_declared_and_bound():
    declared = _lib.declared_symbols()
    # inv | g, inv; depth_values; n_range; B; n; out; stream
    for name, n_args in (("effi_inv_to_depth_ranged_f32", 7), ("effi_inv_to_depth_ranged_bwd_f32", 8)):
        assert name in _lib.SIGNATURES and name in declared
        assert len(_lib.SIGNATURES[name]) == n_args
    fwd, bwd = _lib.SIGNATURES["effi_inv_to_depth_ranged_f32"], _lib.SIGNATURES["effi_inv_to_depth_ranged_bwd_f32"]
    assert bwd[1:] == fwd                                      # the backward takes the gradient in front of the forward's arguments
    assert fwd[2:5] == [_lib._i, _lib._i, _lib._l]             # n_range, B are int; n is long


def test_graphed_train_step_rejects_an_unknown_depth_range_mode_before_touching_the_device():
    from effi_mvs_plus_amd import train_graph
    model = torch.nn.Linear(2, 2)
    opt = torch.optim.AdamW(model.parameters(), lr=0.0)        # not even capturable: the keyword is checked first
    x = torch.zeros(1, 2)
    with pytest.raises(ValueError, match="depth_range"):
        train_graph.GraphedTrainStep(model, opt, x, {}, x, {}, {}, depth_range="nonsense")
    assert not torch.is_tensor(opt.param_groups[0]["lr"])      # nothing was converted or moved


class _StubStep:
    def __init__(self, log, losses):
        self.log, self.losses, self.i = log, losses, 0

    def load_raw_sample(self, batch):
        self.log.append(("load_raw_sample", batch))

    def __call__(self):
        self.log.append(("step",))
        self.i += 1
        return torch.tensor(self.losses[self.i - 1])

    def check_ranges(self):
        self.log.append(("check_ranges",))


class _StubScheduler:
    def __init__(self, log):
        self.log = log

    def step(self):
        self.log.append(("scheduler.step",))


def test_train_epoch_runs_the_reference_loops_order():
    from effi_mvs_plus_amd import train_graph
    log, losses = [], [1.0, 2.0, 6.0]
    mean, steps = train_graph.train_epoch(_StubStep(log, losses), ["a", "b", "c"], _StubScheduler(log))
    want = []
    for b in ("a", "b", "c"):
        want += [("load_raw_sample", b), ("step",), ("scheduler.step",)]
    assert log == want + [("check_ranges",)]
    assert steps == 3 and mean == pytest.approx(3.0)
    log.clear()
    mean, steps = train_graph.train_epoch(_StubStep(log, losses), ["a"])          # no scheduler
    assert log == [("load_raw_sample", "a"), ("step",), ("check_ranges",)] and steps == 1 and mean == pytest.approx(1.0)
