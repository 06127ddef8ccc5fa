"""CPU: the oracle against the REFERENCE ITSELF, through fixtures recorded by running it (tests/golden/make_golden_reference.py:
its forward, training-mode loss and gradients, and its interface).  This is what pins the oracle: the reference ships no tests or
golden vectors of its own.

The oracle is the reference's op sequence, so on CPU it reproduces the recorded outputs bitwise -- given the same rounding of
ATen's CPU kernels, which depends on the thread split, the instruction set and the torch build: the numeric tests run with the
thread count the vectors were recorded with, and fail up front, saying so, under another ATen CPU capability or torch version
than ``ref_interface.json`` records (re-record the vectors there with tests/golden/make_golden_reference.py)."""
import functools
import hashlib
import json
import os

import pytest
import torch

from common import GOLDEN, load_golden
from effi_mvs_plus_amd import synth
from oracle import effi_oracle as O


@functools.lru_cache(maxsize=None)
def interface():
    with open(os.path.join(GOLDEN, "ref_interface.json")) as f:
        return json.load(f)


def recorded_with():
    rec = interface()["recorded_with"]
    return f"fixtures recorded with torch {rec['torch']}, ATen CPU capability {rec['cpu_capability']}, {rec['torch_threads']} threads"


@pytest.fixture
def recording_environment():
    """The recording host's thread count for a numeric test; another ATen CPU capability or torch build rounds differently, and a
    bitwise comparison with the recorded vectors then says nothing about the oracle: fail with that message instead."""
    rec = interface()["recorded_with"]
    here = (torch.__version__, torch.backends.cpu.get_cpu_capability())
    if here != (rec["torch"], rec["cpu_capability"]):
        pytest.fail(f"{recorded_with()}; this process runs torch {here[0]} with ATen CPU capability {here[1]}: re-record the "
                    "fixtures with tests/golden/make_golden_reference.py on this host", pytrace=False)
    before = torch.get_num_threads()
    torch.set_num_threads(rec["torch_threads"])
    yield
    torch.set_num_threads(before)


def state_dict_table(ndepths):
    """The reference model's state-dict key / shape table: tests/golden/state_dict_keys.json, whose digest the fixture records
    for each cascade."""
    with open(os.path.join(GOLDEN, "state_dict_keys.json")) as f:
        table = json.load(f)
    digest = hashlib.sha256(json.dumps(table, sort_keys=True).encode()).hexdigest()
    assert digest == interface()["state_dict_sha256"][ndepths], f"state_dict_keys.json is not the reference's {ndepths} table"
    return table


def reference_state_dict(ndepths, seed):
    """The reference model's state dict (its key names and shapes) with the seeded-random values both sides use."""
    shapes = {k: torch.empty(v[0], dtype=getattr(torch, v[1])) for k, v in state_dict_table(ndepths).items()}
    return synth.randomize_state_dict(shapes, seed=seed)


def _compare(tag, sd, H, W, N, nd):
    want = load_golden("g14_ref_forward.npz")
    imgs, pm, dv = synth.synth_sample(H, W, N, seed=5)
    with torch.no_grad():
        got = O.full_forward(sd, imgs, pm, dv, ndepths=nd)
    assert len(got["depth"]) == 13 and f"{tag}_depth12" in want and f"{tag}_depth13" not in want
    for i, a in enumerate(got["depth"]):                   # same op sequence, same ATen kernels: bitwise
        assert torch.equal(a, want[f"{tag}_depth{i}"]), f"depth map {i} differs from the reference's ({recorded_with()})"
    assert torch.equal(got["photometric_confidence"], want[f"{tag}_confidence"]), f"confidence differs ({recorded_with()})"


@pytest.mark.usefixtures("recording_environment")
def test_random_weights_bitwise():
    _compare("a", reference_state_dict("48,8,8", 3), 128, 160, 4, (48, 8, 8))


@pytest.mark.usefixtures("recording_environment")
def test_other_hypothesis_counts_bitwise():
    # BASELINE.json's wording of the cascade
    _compare("b", reference_state_dict("48,32,8", 4), 96, 128, 3, (48, 32, 8))


@pytest.mark.usefixtures("recording_environment")
def test_depthnet_without_view_weight_net_bitwise():
    """The reference's ``pixel_wise_net=None`` branch of DepthNet (models/Effi_MVS_plus.py:55-58,70), which the shipped model never
    takes: the oracle's restatement of it against the reference's DepthNet called that way."""
    sd = reference_state_dict("8,8,8", 6)
    feats = [f for f in synth.smooth_features(4, 32, 16, 20, seed=2)]
    _, pm, dv = synth.synth_sample(128, 160, 4, seed=7)
    proj = pm["stage1"]
    samples = (1.0 / torch.linspace(1 / 935.0, 1 / 425.0, 8)).view(1, 8, 1, 1).expand(1, 8, 16, 20).contiguous()
    want = load_golden("g14_ref_forward.npz")
    with torch.no_grad():
        got = O.depthnet(sd, feats, proj, samples, 8, pixelwise_prefix=None)
    assert got["view_weights"] == []
    for k in ("volume", "reg_volume", "depth", "photometric_confidence"):
        assert torch.equal(got[k], want["nopw_" + k]), f"{k} differs from the reference's ({recorded_with()})"


def test_our_modules_load_the_shipped_checkpoint_strictly():
    """The keys and shapes of the reference's shipped T&T checkpoint (checkpoints/Effi_MVS_plus/model_tank.ckpt; the fixture
    records the digest of its key / shape table, which is that of tests/golden/state_dict_keys.json) load into our modules
    strictly."""
    from common import build_model
    net, _ = build_model("96,8,8")
    with open(os.path.join(GOLDEN, "state_dict_keys.json")) as f:
        table = json.load(f)
    assert hashlib.sha256(json.dumps(table, sort_keys=True).encode()).hexdigest() == interface()["tank_checkpoint_sha256"]
    sd = {k: torch.zeros(v[0], dtype=getattr(torch, v[1])) for k, v in table.items()}
    assert len(sd) > 400
    res = net.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys


def _loss_inputs(H, W, seed):
    """Synthetic ground truth for mvs_loss: per-stage depth maps + masks (stage k at 1/8, 1/4, 1/2, 1 of the image)."""
    g = torch.Generator().manual_seed(seed)
    gt, mask = {}, {}
    for k, f in (("stage1", 8), ("stage2", 4), ("stage3", 2), ("stage4", 1)):
        gt[k] = synth.DEPTH_MIN_MM + (synth.DEPTH_MAX_MM - synth.DEPTH_MIN_MM) * torch.rand(1, H // f, W // f, generator=g)
        mask[k] = (torch.rand(1, H // f, W // f, generator=g) > 0.3).float()
    return gt, mask


DLOSS = [1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4]       # train.py:246: which ground-truth scale each of the 13 outputs is compared with


@pytest.mark.parametrize("dropout_p", [0.0, 0.1])
@pytest.mark.usefixtures("recording_environment")
def test_training_mode_loss_and_gradients_match_the_reference(dropout_p):
    """Scope row n2's checker: torch autograd through the oracle in training mode (batch-statistics BatchNorm, Dropout2d, the
    detach points of update.py:121 and Effi_MVS_plus.py:495) reproduces the reference's model.train() forward, loss and
    parameter gradients on CPU.  The FPN is included (its BatchNorms also run on batch statistics).  Every gradient is stored
    whole (in the fixture's ``_grads<k>`` parts) and compared element by element."""
    H, W, N = 64, 96, 3
    imgs, pm, dv = synth.synth_sample(H, W, N, seed=6)
    gt, mask = _loss_inputs(H, W, 1)
    name = "g15_ref_train_p0" if dropout_p == 0.0 else "g15_ref_train_p01"
    ref = load_golden(name + ".npz")
    want = {}
    for i in range(int(ref["grad_parts"])):
        part = load_golden(f"{name}_grads{i}.npz")
        assert part and all(k.startswith("grad:") and k[len("grad:"):] not in want for k in part), (name, i)
        want.update({k[len("grad:"):]: v for k, v in part.items()})
    want_stats = {k[len("stat:"):]: v for k, v in ref.items() if k.startswith("stat:")}
    sd = reference_state_dict("8,8,8", 11)

    # the reference registers some modules under two names (update_block.N / update_block_depthN+1, CSP_R.N / CSP_RN+1): tie the
    # aliases to one leaf tensor, as the shared nn.Parameter is
    sd2 = {k: v.clone() for k, v in sd.items()}
    groups = {k: [k] for k in interface()["parameters"]}
    for ks in interface()["param_aliases"]:
        for k in ks:
            groups[k] = ks
    leaves = {}
    for ks in {tuple(ks) for ks in groups.values()}:
        leaf = sd2[ks[0]].requires_grad_(True)
        for k in ks:
            sd2[k] = leaf
            leaves[k] = leaf
    for ks in interface()["buffer_aliases"]:
        for k in ks[1:]:
            sd2[k] = sd2[ks[0]]
    torch.manual_seed(123)
    with O.training(dropout_p):
        got = O.full_forward(sd2, imgs, pm, dv, ndepths=(8, 8, 8))
        loss2, _ = O.mvs_loss(got["depth"], gt, mask, DLOSS)
    loss2.backward()
    assert torch.equal(loss2.detach(), ref["loss"]), f"loss {float(loss2)} vs the reference's {float(ref['loss'])} ({recorded_with()})"
    assert len(got["depth"]) == 13 and "depth12" in ref and "depth13" not in ref
    for i, a in enumerate(got["depth"]):
        assert torch.equal(a.detach(), ref[f"depth{i}"]), f"depth map {i} differs from the reference's ({recorded_with()})"
    n_checked = 0
    for k, g in want.items():
        assert leaves[k].grad is not None, k
        assert torch.allclose(leaves[k].grad, g, rtol=1e-5, atol=1e-7 * float(g.abs().max()) + 1e-12), k
        n_checked += 1
    assert n_checked > 150
    for k, v in want_stats.items():                     # running statistics were updated the same way
        assert torch.allclose(sd2[k].detach().float(), v.float(), rtol=1e-6, atol=1e-7), k


def _json_value(v):
    return json.loads(json.dumps(v))                    # tuples -> lists, as the fixture stores them


def _signature(obj):
    """[[name, has_default, default], ...] per function (a class: __init__ and forward), in the fixture's form."""
    import inspect
    fs = [obj.__init__, obj.forward] if inspect.isclass(obj) else [obj]
    out = []
    for f in fs:
        ps = []
        for p_ in inspect.signature(f).parameters.values():
            if p_.default is inspect.Parameter.empty:
                ps.append([p_.name, False, None])
            elif isinstance(p_.default, (int, float, bool, str, type(None), list)):
                ps.append([p_.name, True, _json_value(p_.default)])
            elif callable(p_.default):
                ps.append([p_.name, True, f"{p_.default.__module__}.{p_.default.__name__}"])
            else:
                ps.append([p_.name, True, repr(p_.default)])
        out.append(ps)
    return out


def test_public_callables_of_the_three_mirrored_files_have_the_references_signatures():
    """Every live public class / function the reference's models/{module,update,Effi_MVS_plus}.py define (dead code of SURVEY
    section 2 excluded) exists in the mirror with the same parameter names, order and defaults; a mirror may only APPEND
    keyword arguments with defaults."""
    import sys

    import effi_mvs_plus_amd.models  # noqa: F401
    ours = {"main": sys.modules["effi_mvs_plus_amd.models.Effi_MVS_plus"], "module": sys.modules["effi_mvs_plus_amd.models.module"],
            "update": sys.modules["effi_mvs_plus_amd.models.update"]}
    sigs = interface()["signatures"]
    assert sorted(sigs) == sorted(ours) and sum(len(v) for v in sigs.values()) == 25
    for mod, names in sigs.items():
        for name, want in names.items():
            got = _signature(getattr(ours[mod], name))
            assert len(got) == len(want), f"{mod}.{name}"
            for w_, g_ in zip(want, got):
                assert g_[:len(w_)] == w_, f"{mod}.{name}: {g_} vs reference {w_}"
                for extra in g_[len(w_):]:
                    assert extra[1], f"{mod}.{name}: appended parameter {extra[0]} needs a default"


def test_fusion_and_dtu_filter_functions_have_the_references_signatures():
    """Row n3's surface: the functions of misc/fusion.py that test_tank.py:486-509 calls and the two of test_dtu_dypcd.py:164-233,
    by name, parameter names, order and defaults (the fixture holds the reference's signatures as parsed from its source with
    ``ast``: test_dtu_dypcd.py imports cv2 / plyfile, which are not importable here)."""
    import inspect

    from effi_mvs_plus_amd import dtu_fusion, fusion

    def our_sig(fn):
        return [[p_.name, p_.default is not inspect.Parameter.empty,
                 None if p_.default is inspect.Parameter.empty else _json_value(p_.default)]
                for p_ in inspect.signature(fn).parameters.values()]

    tank = ["get_pixel_grids", "bin_op_reduce", "idx_img2cam", "idx_cam2world", "idx_world2cam", "idx_cam2img", "get_reproj_dynamic",
            "vis_filter_dynamic"]
    want = interface()["fusion_signatures"]
    assert sorted(want) == sorted(tank)
    for name in tank:
        got = our_sig(getattr(fusion, name))
        assert got[:len(want[name])] == want[name], f"fusion.{name}: {got} vs reference {want[name]}"
        assert all(has_default for _, has_default, _ in got[len(want[name]):]), f"fusion.{name}: appended parameters need defaults"
    dtu = ["reproject_with_depth", "check_geometric_consistency", "read_camera_parameters", "read_pair_file", "read_img", "save_mask"]
    want = interface()["dtu_filter_signatures"]
    assert sorted(want) == sorted(dtu)
    for name in dtu:
        got = our_sig(getattr(dtu_fusion, name))
        w_ = want[name]
        if name == "check_geometric_consistency":          # the reference's last parameter (confidence, unused) has no default; ours accepts its absence
            assert [g_[0] for g_ in got[:len(w_)]] == [x[0] for x in w_], (got, w_)
        else:
            assert got[:len(w_)] == w_, f"dtu_fusion.{name}: {got} vs reference {w_}"
        assert all(has_default for _, has_default, _ in got[len(w_):]), f"dtu_fusion.{name}: appended parameters need defaults"
    # the driver's call sites name no other attribute of the module (test_tank.py:455-571)
    used = interface()["tank_driver_fusion_names"]
    assert used and all(hasattr(fusion, u) for u in used), sorted(u for u in used if not hasattr(fusion, u))
