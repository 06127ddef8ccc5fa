"""Shared helpers for the parity tests: seeded models / inputs and an error reporter."""
import argparse
import contextlib
import io
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from effi_mvs_plus_amd import synth  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


def model_args(ndepths="48,8,8", gru="3,3,3", cost_num=3):
    return argparse.Namespace(ndepths=ndepths, GRUiters=gru, CostNum=cost_num)


def build_model(ndepths="48,8,8", seed=1, device="cpu"):
    """Our model with seeded-random weights (BN statistics randomised) + the same state dict on CPU."""
    from effi_mvs_plus_amd.models import Effi_MVS_plus
    with contextlib.redirect_stdout(io.StringIO()):
        net = Effi_MVS_plus(model_args(ndepths))
    sd = synth.randomize_state_dict(net.state_dict(), seed=seed)
    net.load_state_dict(sd, strict=True)
    net.eval()
    if device != "cpu":
        net = net.to(device)
    return net, sd


def stats(got, want):
    got = got.detach().double().cpu()
    want = want.detach().double().cpu()
    diff = (got - want).abs()
    scale = want.abs().max().item() + 1e-30
    return {"max_abs": diff.max().item(), "mean_abs": diff.mean().item(), "ref_max": scale,
            "max_rel_to_peak": diff.max().item() / scale,
            "p99": torch.quantile(diff.flatten()[:: max(1, diff.numel() // 1_000_000)], 0.99).item()}


def check_close(name, got, want, rtol=1e-4, atol=1e-5, frac_ok=1.0, outlier_atol=None):
    """allclose with a readable report; ``frac_ok`` < 1 tolerates a small fraction of outliers
    (discontinuities: floor / clamp / out-of-bounds flips).  The excluded set is not ignored: its size and its largest error
    are printed and the largest error is bounded by ``outlier_atol`` (default: the peak of ``want`` -- a flip can move a value
    across the data's own range, garbage cannot hide behind the fraction)."""
    assert tuple(got.shape) == tuple(want.shape), f"{name}: shape {tuple(got.shape)} vs {tuple(want.shape)}"
    s = stats(got, want)
    g, w = got.detach().double().cpu(), want.detach().double().cpu()
    err = (g - w).abs()
    ok = (err <= atol + rtol * w.abs())
    frac = ok.double().mean().item()
    n_out = int((~ok).sum())
    out_max = float(err[~ok].max()) if n_out else 0.0
    print(f"[parity] {name:42s} max_abs={s['max_abs']:.3e} mean_abs={s['mean_abs']:.3e} p99={s['p99']:.3e} "
          f"peak={s['ref_max']:.3e} within_tol={frac:.6f} excluded={n_out} excluded_max_abs={out_max:.3e}")
    assert torch.isfinite(g).all(), f"{name}: non-finite values"
    assert frac >= frac_ok, f"{name}: only {frac:.6f} of elements within rtol={rtol} atol={atol} (need {frac_ok})"
    bound = s["ref_max"] + atol if outlier_atol is None else outlier_atol
    assert out_max <= bound, f"{name}: an excluded element is off by {out_max:.3e} (bound {bound:.3e})"
    s["excluded"], s["excluded_max_abs"] = n_out, out_max
    return s


def load_golden(name):
    path = os.path.join(GOLDEN, name)
    with np.load(path, allow_pickle=False) as z:
        return {k: torch.from_numpy(z[k]) for k in z.files}


def t(x, device):
    return x.to(device=device, dtype=torch.float32).contiguous()


def conv_tol(precision, want, rtol, atol, layers=1):
    """Per-operator tolerance of a convolution chain: the fp32 MFMA path keeps (rtol, atol); the split-bf16 path adds
    4e-5 of the output's peak per chained layer (each product carries ~2^-16 relative error; measured ~5e-6 of peak per layer)."""
    if precision == "split":
        peak = float(torch.as_tensor(want).abs().max())
        return dict(rtol=rtol, atol=atol + 4e-5 * layers * peak)
    return dict(rtol=rtol, atol=atol)


def _edge_cameras(h, w, N, kind):
    """Camera rigs that stress the window logic of the stage-1 kernel: `rolled` = source views rotated about the optical
    axis (slanted epipolar lines, windows taller than wide), `wide` = large baselines (windows that exceed the LDS budget:
    chunks shrink, then fall back to global loads), `inside` = a source camera inside the depth range (Z <= 0 for part of
    the volume: those chunks must take the global path), `far` = a view that looks away (every tap out of bounds)."""
    import math
    pm = synth.synth_cameras(h * 8, w * 8, N)["stage1"].clone()
    for v in range(1, N):
        E = pm[0, v, 0]
        if kind == "rolled":
            a = math.radians(25.0 * v)
            Rz = torch.tensor([[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1.0]])
            E[:3, :3] = Rz @ E[:3, :3]
            E[:3, 3] = Rz @ E[:3, 3]
        elif kind == "wide":
            E[:3, 3] = E[:3, 3] * (4.0 + v)
        elif kind == "inside":
            E[2, 3] = E[2, 3] - 600.0 - 40.0 * v          # camera centre moved into the scene
        elif kind == "far":
            a = math.radians(100.0)
            Ry = torch.tensor([[math.cos(a), 0, math.sin(a)], [0, 1.0, 0], [-math.sin(a), 0, math.cos(a)]])
            E[:3, :3] = Ry @ E[:3, :3]
    return pm


# ---- gradients too large to store in full (tests/golden/make_golden_reference.py, tests/test_oracle_vs_reference.py) ----------
GRAD_FULL_MAX = 1024          # a gradient with at most this many elements is stored whole
GRAD_SAMPLE = 512             # elements of a larger one stored at fixed positions
GRAD_PROJECTIONS = 8          # +-1 projections of the whole tensor stored beside them


def grad_sample_index(n, name):
    """GRAD_SAMPLE fixed positions spread over a flattened tensor of n elements, by integer arithmetic only (the same on every
    host and library version): a stride coprime with n from an offset derived from the parameter's name."""
    import math
    import zlib
    stride = 7919
    while math.gcd(stride, n) != 1:
        stride += 2
    return (torch.arange(GRAD_SAMPLE, dtype=torch.int64) * stride + zlib.crc32(name.encode()) % n) % n


def grad_signs(n):
    """[GRAD_PROJECTIONS, n] fixed +-1 patterns (an integer hash of position and row), float64."""
    i = torch.arange(n, dtype=torch.int64)
    rows = []
    for j in range(GRAD_PROJECTIONS):
        h = (i * 2654435761 + (j + 1) * 0x9E3779B1) & 0xFFFFFFFF
        h = h ^ (h >> 15)
        h = (h * 0x2C1B3C6D) & 0xFFFFFFFF
        h = h ^ (h >> 12)
        rows.append(1.0 - 2.0 * ((h >> 7) & 1).double())
    return torch.stack(rows)


def grad_summary(g):
    """What is stored of a large gradient beside its sampled elements: [sum |g|, ||g||_2, max |g|] and the +-1 projections,
    all in float64 over the whole tensor."""
    f = g.detach().double().reshape(-1)
    return (torch.stack([f.abs().sum(), f.norm(), f.abs().max()]), grad_signs(f.numel()) @ f)
