"""An exact read-out of the costs that ``effi_getcost_pixel`` hands to the 1x1 matrix of the fused entries.

``getcost_conv1x1_block`` (effi_mvs_plus_amd/csrc/volume_ops.hip) computes, per output channel c,  acc = bias[c];
acc = fmaf(cost[k], weight[k][c], acc)  for k = 0 .. 2 nq - 1, then the optional ReLU.  With bias 0 and a weight matrix of zeros
and +-1 entries every product is exact and every sum has one non-zero term, so for finite costs
  * ``getcost_conv1x1(relu=False)``, cout 8, weight[k][k] = 1: channel k IS cost[k], channels >= 2 nq are exactly 0;
  * ``encoder_inputs`` (ReLU fixed, nq = 3), weight[k][k] = +1 and weight[k][8 + k] = -1: channel k is max(cost[k], 0), channel
    8 + k is max(-cost[k], 0), one of the two is 0 and their difference IS cost[k]; every other channel is exactly 0.
A cost that is NaN or Inf would reach every channel (0 * NaN): the "exactly 0" assertions below fail then.  The helpers are plain
torch: they serve the GPU tests (tests/test_gpu_getcost_readout.py) and the fp32 restatement on the CPU
(tests/test_getcost_pixel_host.py) alike."""
import torch

RELU_COUTS = (16, 32, 48)


def selection_plain(nq, device="cpu"):
    """-> weight [2 nq, 8], bias [8] for ``getcost_conv1x1(relu=False)``."""
    assert 2 * nq <= 8
    w = torch.zeros(2 * nq, 8, device=device)
    for k in range(2 * nq):
        w[k, k] = 1.0
    return w, torch.zeros(8, device=device)


def selection_relu(nq, cout, device="cpu"):
    """-> weight [2 nq, cout], bias [cout] for the entries whose ReLU is fixed."""
    assert 2 * nq <= 8 and cout >= 16
    w = torch.zeros(2 * nq, cout, device=device)
    for k in range(2 * nq):
        w[k, k] = 1.0
        w[k, 8 + k] = -1.0
    return w, torch.zeros(cout, device=device)


def _exactly_zero(name, out, channels):
    for c in channels:
        nz = int((out[c] != 0).sum())
        assert nz == 0, f"{name}: channel {c} must be exactly 0, {nz} elements are not (first {out[c][out[c] != 0][:4].tolist()})"


def recover_plain(name, out, nq):
    """out [8, ...] of the ``selection_plain`` matrix -> cost [2 nq, ...]."""
    assert out.shape[0] == 8
    _exactly_zero(name, out, range(2 * nq, 8))
    return out[:2 * nq]


def recover_relu(name, out, nq):
    """out [cout, ...] of the ``selection_relu`` matrix -> cost [2 nq, ...]."""
    pos, neg = out[:2 * nq], out[8:8 + 2 * nq]
    _exactly_zero(name, out, [c for c in range(out.shape[0]) if not (c < 2 * nq or 8 <= c < 8 + 2 * nq)])
    assert bool(((pos >= 0) & (neg >= 0)).all()), f"{name}: a negative value behind the ReLU"
    both = int(((pos != 0) & (neg != 0)).sum())
    assert both == 0, f"{name}: {both} costs are non-zero in both of their channels"
    return pos - neg


def conv1x1_fp32(cost, weight, bias, relu):
    """The matrix of ``getcost_conv1x1_block`` in fp32 torch for weights of zeros and +-1: each product is exact, so the unfused
    multiply-add below rounds like the kernel's fmaf.  cost [2 nq, n], weight [2 nq, cout] -> [cout, n]."""
    assert bool(((weight == 0) | (weight.abs() == 1)).all())
    acc = bias.view(-1, 1).expand(weight.shape[1], cost.shape[1]).clone()
    for k in range(cost.shape[0]):
        acc = acc + cost[k].view(1, -1) * weight[k].view(-1, 1)
    return acc.clamp(min=0) if relu else acc


# ---- the fused entries on the GPU -----------------------------------------------------------------------------------------------
def readout_conv1x1(name, x, disp_range, itv, cur, reg, lo, hi, nq, h, w, input_is_depth):
    """cost [2 nq, h, w] as ``ops.getcost_conv1x1`` sees it (device tensors; cur / reg in any layout the entry takes)."""
    from effi_mvs_plus_amd import ops
    wgt, bias = selection_plain(nq, x.device)
    out = ops.getcost_conv1x1(x, disp_range, itv, cur, reg, lo, hi, nq, h, w, wgt, bias, 8, relu=False, input_is_depth=input_is_depth)
    return recover_plain(name, out, nq)


def readout_encoder_inputs(name, x, disp_range, itv, cur, reg, lo, hi, h, w, cout, w7, b7):
    """cost [6, h, w] as ``ops.encoder_inputs`` sees it (nq = 3, normalised inverse depth), in the precision that is set; the 7x7 half
    of the launch must be ``ops.conv2d_c1k7_relu`` bit for bit."""
    from effi_mvs_plus_amd import ops
    wgt, bias = selection_relu(3, cout, x.device)
    c1, d1 = ops.encoder_inputs(x, disp_range, itv, cur, reg, lo, hi, 3, h, w, wgt, bias, w7, b7, cout)
    assert torch.equal(d1, ops.conv2d_c1k7_relu(x, w7, b7, cout)), f"{name}: the 7x7 half differs from conv2d_c1k7_relu"
    return recover_relu(name, c1, 3)
