#!/usr/bin/env python3
"""Golden vectors for tests/test_oracle_vs_reference.py, produced by running the REFERENCE itself on CPU.

Run in the build container only (needs the reference tree; see tests/refimport.py for the import recipe):
    python -B tests/golden/make_golden_reference.py
Writes
  g14_ref_forward.npz     the reference's forward (13 depth maps + confidence) on seeded-random weights, two cascades, and its
                          DepthNet called with ``pixel_wise_net=None``
  g15_ref_train_p*.npz    the reference's model.train() forward, mvs_loss and updated BatchNorm statistics (Dropout2d p = 0
                          and 0.1); every parameter gradient, whole, in g15_ref_train_p*_grads<k>.npz (split in parts of at
                          most GRAD_PART_BYTES so that each fixture file stays small)
  ref_interface.json      what the tests check of the reference's interface: digests of its state-dict key / shape table for
                          each cascade and of its shipped T&T checkpoint's (all equal to tests/golden/state_dict_keys.json; the
                          checkpoint's weights are not copied: no licence), its parameters and the aliases it registers under
                          two names, the signatures of its public callables, the ``fusion.*`` names its T&T driver calls, and
                          the thread count / ATen CPU capability / torch version the vectors were recorded with
Weights are never stored: both sides rebuild them with ``effi_mvs_plus_amd.synth.randomize_state_dict(shapes, seed)``.
"""
import ast
import hashlib
import inspect
import json
import os
import re
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from refimport import REF_ROOT, load_reference, reference_model  # noqa: E402
from effi_mvs_plus_amd import synth  # noqa: E402

# the cascades of the forward fixtures: name -> (ndepths, weight seed, H, W, N)
FORWARD_CASES = {"a": ("48,8,8", 3, 128, 160, 4), "b": ("48,32,8", 4, 96, 128, 3)}
DEPTHNET_SEED = 6
DLOSS = [1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4]
TRAIN_SEED, TRAIN_H, TRAIN_W, TRAIN_N = 11, 64, 96, 3
THREADS = 8
GRAD_PART_BYTES = 760_000

# live public callables of the reference's models/{Effi_MVS_plus,module,update}.py (dead code of SURVEY section 2 excluded)
LIVE = {
    "main": ["DepthNet", "bilinear_sampler", "pro_bilinear_sampler", "disp_to_depth", "depth_to_disp", "upsample_depth",
             "GetCost_initvolume", "GetCost", "Effi_MVS_plus"],
    "module": ["homo_warping_new", "Conv3d", "Deconv3d", "Conv2d", "ConvBnReLU", "CostRegNet_2_sample_FPN3D_Fast", "cost_up_small",
               "depth_regression", "get_cur_depth_range_samples", "get_depth_range_samples", "P_1to8_FeatureNet_Fast", "mvs_loss"],
    "update": ["DepthHead", "ConvGRU", "ProjectionInput", "BasicUpdateBlock"],
}
TANK_FUSION = ["get_pixel_grids", "bin_op_reduce", "idx_img2cam", "idx_cam2world", "idx_world2cam", "idx_cam2img", "get_reproj_dynamic",
               "vis_filter_dynamic"]
DTU_FILTER = ["reproject_with_depth", "check_geometric_consistency", "read_camera_parameters", "read_pair_file", "read_img", "save_mask"]


def signature(obj):
    """[[name, has_default, default], ...] per function (a class: __init__ and forward); defaults that are not plain JSON
    values are kept as their repr, callables as module.name."""
    fs = [obj.__init__, obj.forward] if inspect.isclass(obj) else [obj]
    out = []
    for f in fs:
        ps = []
        for p in inspect.signature(f).parameters.values():
            if p.default is inspect.Parameter.empty:
                ps.append([p.name, False, None])
            elif isinstance(p.default, (int, float, bool, str, type(None), list)):
                ps.append([p.name, True, p.default])
            elif callable(p.default):                     # e.g. torch.tanh: its name, not its address
                ps.append([p.name, True, f"{p.default.__module__}.{p.default.__name__}"])
            else:
                ps.append([p.name, True, repr(p.default)])
        out.append(ps)
    return out


def ast_signatures(path, names):
    """Signatures read from a source file without importing it: {name: [[arg, has_default, default], ...]}."""
    tree = ast.parse(open(path).read())
    out = {}
    for node in tree.body:
        if isinstance(node, ast.FunctionDef) and node.name in names:
            a = node.args
            pos = [x.arg for x in a.args]
            n_plain = len(pos) - len(a.defaults)
            defaults = [None] * n_plain + [ast.literal_eval(d) for d in a.defaults]
            out[node.name] = [[p, i >= n_plain, d] for i, (p, d) in enumerate(zip(pos, defaults))]
    return out


def shapes_of(sd):
    return {k: [list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in sd.items()}


def table_digest(table):
    """sha256 of a {key: [shape, dtype]} table (tests/test_oracle_vs_reference.py computes the same)."""
    return hashlib.sha256(json.dumps(table, sort_keys=True).encode()).hexdigest()


def save(name, **arrs):
    out = {k: np.asarray(v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in arrs.items()}
    path = os.path.join(HERE, name)
    np.savez_compressed(path, **out)
    print(f"{name}: {os.path.getsize(path) / 1024:.1f} KiB, {len(out)} arrays")


def loss_inputs(H, W, seed):
    g = torch.Generator().manual_seed(seed)
    gt, mask = {}, {}
    for k, f in (("stage1", 8), ("stage2", 4), ("stage3", 2), ("stage4", 1)):
        gt[k] = synth.DEPTH_MIN_MM + (synth.DEPTH_MAX_MM - synth.DEPTH_MIN_MM) * torch.rand(1, H // f, W // f, generator=g)
        mask[k] = (torch.rand(1, H // f, W // f, generator=g) > 0.3).float()
    return gt, mask


def main():
    torch.set_num_threads(THREADS)
    # ATen's CPU kernels round differently with another thread split or instruction set: the tests run with the same thread
    # count, and the instruction set is recorded beside the vectors
    iface = {"state_dict_sha256": {}, "recorded_with": {"torch_threads": THREADS, "cpu_capability": torch.backends.cpu.get_cpu_capability(),
                                                 "torch": torch.__version__}}

    # ---- forward of two cascades on seeded-random weights ------------------------------------------------
    arrs = {}
    for tag, (nd, seed, H, W, N) in FORWARD_CASES.items():
        _, net = reference_model(nd)
        iface["state_dict_sha256"][nd] = table_digest(shapes_of(net.state_dict()))
        sd = synth.randomize_state_dict(net.state_dict(), seed=seed)
        net.load_state_dict(sd, strict=True)
        imgs, pm, dv = synth.synth_sample(H, W, N, seed=5)
        with torch.no_grad():
            out = net(imgs, pm, dv)
        assert len(out["depth"]) == 13
        for i, d in enumerate(out["depth"]):
            arrs[f"{tag}_depth{i}"] = d
        arrs[f"{tag}_confidence"] = out["photometric_confidence"]

    # ---- DepthNet with pixel_wise_net=None (a branch the shipped model never takes) ------------------------
    _, net = reference_model("8,8,8")
    iface["state_dict_sha256"]["8,8,8"] = table_digest(shapes_of(net.state_dict()))
    sd = synth.randomize_state_dict(net.state_dict(), seed=DEPTHNET_SEED)
    net.load_state_dict(sd, strict=True)
    net.eval()
    feats = [f for f in synth.smooth_features(4, 32, 16, 20, seed=2)]
    _, pm, dv = synth.synth_sample(128, 160, 4, seed=7)
    samples = (1.0 / torch.linspace(1 / 935.0, 1 / 425.0, 8)).view(1, 8, 1, 1).expand(1, 8, 16, 20).contiguous()
    with torch.no_grad():
        want = net.depthnet(feats, pm["stage1"], depth_values=samples, num_depth=8, cost_regularization=net.cost_regularization,
                            pixel_wise_net=None, G=1)
    assert want["view_weights"] == []
    for k in ("volume", "reg_volume", "depth", "photometric_confidence"):
        arrs["nopw_" + k] = want[k]
    save("g14_ref_forward.npz", **arrs)

    # ---- training mode: forward, loss, gradients, BatchNorm statistics -------------------------------------
    for p_drop, name in ((0.0, "g15_ref_train_p0.npz"), (0.1, "g15_ref_train_p01.npz")):
        ref, net = reference_model("8,8,8")
        sd = synth.randomize_state_dict(net.state_dict(), seed=TRAIN_SEED)
        net.load_state_dict(sd, strict=True)
        net.train()
        for m in net.modules():
            if isinstance(m, torch.nn.Dropout2d):
                m.p = p_drop
        imgs, pm, dv = synth.synth_sample(TRAIN_H, TRAIN_W, TRAIN_N, seed=6)
        gt, mask = loss_inputs(TRAIN_H, TRAIN_W, 1)
        torch.manual_seed(123)
        out = net(imgs, pm, dv)
        loss, _ = ref.module.mvs_loss(out["depth"], gt, mask, DLOSS)
        loss.backward()
        arrs = {"loss": loss.detach()}
        for i, d in enumerate(out["depth"]):
            arrs[f"depth{i}"] = d.detach()
        parts, size = [{}], 0
        for k, p in net.named_parameters():
            if p.grad is None:
                continue
            if size and size + 4 * p.grad.numel() > GRAD_PART_BYTES:
                parts.append({})
                size = 0
            parts[-1]["grad:" + k] = p.grad
            size += 4 * p.grad.numel()
        arrs["grad_parts"] = np.int64(len(parts))
        for i, part in enumerate(parts):
            save(name.replace(".npz", f"_grads{i}.npz"), **part)
        for k, v in net.state_dict().items():
            if "running_" in k or "num_batches" in k:
                arrs["stat:" + k] = v
        save(name, **arrs)
    # the reference registers some modules under two names (update_block.N / update_block_depthN+1, CSP_R.N / CSP_RN+1)
    groups, bgroups = {}, {}
    for k, p in net.named_parameters(remove_duplicate=False):
        groups.setdefault(id(p), []).append(k)
    for k, b in net.named_buffers(remove_duplicate=False):
        bgroups.setdefault(id(b), []).append(k)
    iface["parameters"] = [k for k, _ in net.named_parameters(remove_duplicate=False)]
    iface["param_aliases"] = [ks for ks in groups.values() if len(ks) > 1]
    iface["buffer_aliases"] = [ks for ks in bgroups.values() if len(ks) > 1]

    # ---- interface: signatures, the T&T driver's fusion.* names, the shipped checkpoint's keys ------------
    ref = load_reference()
    iface["signatures"] = {mod: {name: signature(getattr(getattr(ref, mod), name)) for name in names} for mod, names in LIVE.items()}
    iface["fusion_signatures"] = ast_signatures(os.path.join(REF_ROOT, "misc", "fusion.py"), TANK_FUSION)
    iface["dtu_filter_signatures"] = ast_signatures(os.path.join(REF_ROOT, "test_dtu_dypcd.py"), DTU_FILTER)
    src = open(os.path.join(REF_ROOT, "test_tank.py")).read()
    iface["tank_driver_fusion_names"] = sorted(set(re.findall(r"\bfusion\.([A-Za-z_][A-Za-z0-9_]*)", src)))
    ckpt = os.path.join(REF_ROOT, "checkpoints", "Effi_MVS_plus", "model_tank.ckpt")
    iface["tank_checkpoint_sha256"] = table_digest(shapes_of(torch.load(ckpt, map_location="cpu", weights_only=True)["model"]))
    with open(os.path.join(HERE, "state_dict_keys.json")) as f:
        keys = table_digest(json.load(f))
    assert keys == iface["tank_checkpoint_sha256"] and all(d == keys for d in iface["state_dict_sha256"].values()), \
        "the reference's state-dict tables differ from tests/golden/state_dict_keys.json"
    path = os.path.join(HERE, "ref_interface.json")
    with open(path, "w") as f:
        json.dump(iface, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"ref_interface.json: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
