"""GPU: the sliding-plane body of the row-pair rolling 3-D convolution (csrc/conv2d.hip, conv3d_roll_rp_bf16x3_body) against the
three-slot body it replaced (option roll_slide = 0), bitwise, on random normal inputs.

Every output receives the same MFMAs in the same order in both bodies, so the comparison is exact.  What can go wrong in the new one
is its bookkeeping: which accumulator an output lives in while the planes slide past (runs shorter than the three-step rotation, runs
that end in the middle of it), the first and last steps that multiply fewer than three dz blocks, the halo planes at both ends of a
run, the two LDS slots (a slot read before it is refilled, or after).  The shapes are the smallest that reach each of those: D from 1
to 8, runs of 1, 2, 3 and D planes (a ragged last run wherever D is no multiple), both rows-per-wave forms, 8 and 16 input channels
(one source or two), 8 and 4 output channels, a ragged last tile row (6x20), a width that is a multiple of 4 but not of 16 (17x36)
and exact tiles (32x32), the single, pair and sample-batched entries."""
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

DEPTHS = (1, 2, 3, 4, 7, 8)
MAPS = ((6, 20), (17, 36), (32, 32))
CINS = ("8", "16", "8+8")
N_SMP = 2

_VOLS, _LAYERS = {}, {}


def _volume(cin, hw, k):
    """Random normal [cin, 8, h, w] volume number k of a map size, made once; a case takes its first D planes."""
    key = (cin, hw, k)
    if key not in _VOLS:
        g = torch.Generator().manual_seed(1000 * cin + 10 * hw[0] + k)
        _VOLS[key] = torch.randn(cin, max(DEPTHS), *hw, generator=g).to(DEV)
    return _VOLS[key]


def _layer(cin, cout, k):
    """Packed row-pair operand and bias of random layer number k (packing.pack_conv3d_roll_bf16x3), made once."""
    from effi_mvs_plus_amd import packing
    key = (cin, cout, k)
    if key not in _LAYERS:
        torch.manual_seed(77 * cin + 7 * cout + k)
        conv = torch.nn.Conv3d(cin, cout, 3, padding=1).to(DEV)
        with torch.no_grad():
            _LAYERS[key] = packing.pack_conv3d_roll_bf16x3(conv, None)
    return _LAYERS[key]


def _sources(cins, x):
    """x [..., 16 or 8, D, h, w] as the source list of the channel split ``cins``."""
    return [x[..., :8, :, :, :].contiguous(), x[..., 8:, :, :, :].contiguous()] if cins == "8+8" else [x]


def _run(entry, cins, cout, D, hw, relu, vols=None):
    """One launch of ``entry`` under the current options -> list of output volumes."""
    from effi_mvs_plus_amd import ops
    cin = 8 if cins == "8" else 16
    vols = vols or [_volume(cin, hw, k)[:, :D].contiguous() for k in range(N_SMP)]
    wa, ba = _layer(cin, cout, 0)
    if entry == "single":
        return [ops.conv3d_k3s1_roll(_sources(cins, vols[0]), wa, ba, cout, relu=relu)]
    if entry == "batch":
        return [ops.conv3d_k3s1_roll(_sources(cins, torch.stack(vols)), wa, ba, cout, relu=relu)]
    wb, bb = _layer(cin, cout, 1)
    return list(ops.conv3d_k3s1_roll_pair(_sources(cins, vols[0]), wa, ba, _sources(cins, vols[1]), wb, bb, cout, relu=relu))


def _both(entry, cins, cout, D, hw, relu, mr, zt, vols=None):
    """(sliding, three-slot) outputs of one case at the tile form (mr, zt), which the launch rule must confirm."""
    from effi_mvs_plus_amd import ops
    count = {"single": 1, "pair": 2, "batch": N_SMP}[entry]
    with ops.options(roll_mr=mr, roll_zt=zt):
        form = ops.launch_form("roll", hw[0], hw[1], nt=1, planes=D, count=count, cout=cout, oct2=cins != "8")
        assert tuple(form) == (mr, 16, 4, zt, 1), f"the rule picks {tuple(form)}: not the row-pair kernel at ({mr}, {zt})"
        got = _run(entry, cins, cout, D, hw, relu, vols)
        with ops.options(roll_slide=0):
            want = _run(entry, cins, cout, D, hw, relu, vols)
    return got, want


@pytest.mark.parametrize("entry,mr,cins", list(itertools.product(("single", "pair", "batch"), (2, 4), CINS)),
                         ids=lambda v: str(v))
def test_sliding_body_is_bitwise_the_three_slot_body(entry, mr, cins):
    checked = 0
    with torch.no_grad():
        for D, hw, cout, relu in itertools.product(DEPTHS, MAPS, (8, 4), (True, False)):
            for zt in sorted({1, 2, 3, D} & set(range(1, D + 1))):
                got, want = _both(entry, cins, cout, D, hw, relu, mr, zt)
                for k, (g, w_) in enumerate(zip(got, want)):
                    assert g.shape == w_.shape and g.shape[-4:] == (cout, D, *hw)
                    if not torch.equal(g, w_):
                        bad = (g != w_).nonzero()
                        raise AssertionError(f"{entry} mr{mr} cin {cins} cout{cout} D{D} zt{zt} {hw} relu={relu}, output {k}: {len(bad)} elements "
                                             f"differ, first at {bad[0].tolist()}: {g[tuple(bad[0])].item()!r} vs {w_[tuple(bad[0])].item()!r}")
                    checked += 1
    assert checked >= len(DEPTHS) * len(MAPS) * 4


@pytest.mark.parametrize("cins,mr", list(itertools.product(("8", "16"), (2, 4))), ids=lambda v: str(v))
def test_nan_and_inf_in_one_plane_stay_in_the_outputs_that_read_it(cins, mr):
    """A NaN and an Inf planted in input plane 2 of 8: the outputs that multiply them may change, every other output is bitwise the
    clean run's -- a fragment read from a stale or not yet refilled slot would carry them elsewhere.  "Multiply" is the row-pair
    operand's: output rows y (even) and y + 1 share the K index over input rows y - 1 .. y + 2, with zero weights where a row does not
    reach, and 0 x NaN is NaN -- so an input row r reaches both rows of every pair whose four-row window holds it, one row further
    than the convolution's own 3 x 3 x 3 support; planes and columns are the support's.  Runs of 8 (one
    workgroup sees the plane come and go), 3 (the plane ends the first run and is the lower halo of the second) and 2 (it starts the
    second run and is the upper halo of the first)."""
    D, hw, cout, zp = 8, (17, 36), 8, 2
    cin = 8 if cins == "8" else 16
    spots = ((0, 5, 9), (cin - 1, 12, 30))                         # (channel, y, x) of the NaN and of the Inf
    clean = [_volume(cin, hw, k)[:, :D].contiguous() for k in range(N_SMP)]
    dirty = [v.clone() for v in clean]
    dirty[0][spots[0][0], zp, spots[0][1], spots[0][2]] = float("nan")
    dirty[0][spots[1][0], zp, spots[1][1], spots[1][2]] = float("inf")
    touched = torch.zeros(D, *hw, dtype=torch.bool, device=DEV)
    for _, y, x in spots:
        for ye in range(0, hw[0], 2):                              # the row pairs (ye, ye + 1) whose window ye - 1 .. ye + 2 holds row y
            if ye - 1 <= y <= ye + 2:
                touched[zp - 1:zp + 2, ye:ye + 2, max(x - 1, 0):x + 2] = True
    with torch.no_grad():
        for zt in (8, 3, 2):
            (got,), (want,) = _both("single", cins, cout, D, hw, False, mr, zt, dirty)
            (ref,), _ = _both("single", cins, cout, D, hw, False, mr, zt, clean)
            keep = ~touched.expand_as(got)
            assert torch.equal(got[keep], ref[keep]), f"zt{zt}: an output that reads neither value changed"
            assert bool(torch.isfinite(got[keep]).all())
            assert not bool(torch.isfinite(got[:, zp, spots[0][1], spots[0][2]]).any()), "the NaN did not reach its own output pixel"
            # the touched outputs: non-finite in the same places as in the three-slot body, the same bits elsewhere
            assert torch.equal(torch.isfinite(got), torch.isfinite(want))
            fin = torch.isfinite(got)
            assert torch.equal(got[fin], want[fin])
