"""GPU: the small per-pixel launches of the hot path folded into their neighbours, each against the launches it replaces.

  * ops.depth_head_sr           = ops.conv2d_k3_k1_sr (conv1 + ReLU + nine tap projections) + ops.head_update
  * ops.split_tanh_relu_stages_sr(clear=...) = ops.sr_clear_border + ops.split_tanh_relu_stages_sr
  * ops.cascade_setup           = ops.stage1_hypotheses + ops.compose_rel_proj_stages
  * ops.softmax_regress_conf(conf_up=4) = ops.softmax_regress_conf + ops.upsample_nearest

The bar is BITWISE (torch.equal on every output): the fused forms do the same arithmetic in the same order on the same values; what
they remove is launches and round trips through memory.  The cascade with every new option on must equal the cascade with every new
option off, map for map.
"""
import pytest
import torch

from common import build_model
from effi_mvs_plus_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# the three stage shapes of cfg3 with their hidden sizes, one shape whose height and width are not tile multiples, one smaller than a
# tile (16 x 16 and 8 x 16 computed pixels) in one dimension
HEAD_CASES = [(0, 148, 200), (1, 296, 400), (2, 592, 800), (0, 74, 100), (1, 74, 100), (2, 74, 100), (0, 6, 40), (2, 40, 8)]
NEW_OPTIONS = ("head_fused", "clear_fused", "setup_fused", "conf_fused")


@pytest.fixture(scope="module")
def model():
    return build_model("8,8,8", seed=11, device=DEV)


@pytest.fixture(params=["split", "bf16"])
def precision(request):
    from effi_mvs_plus_amd import ops
    before = ops.get_precision()
    ops.set_precision(request.param)
    yield request.param
    ops.set_precision(before)


def _head_inputs(blk, hd, h, w, seed, big_border):
    from effi_mvs_plus_amd import ops
    g = torch.Generator().manual_seed(seed)
    hid = torch.tanh(torch.randn(hd, h, w, generator=g))
    if big_border:
        # a hidden state that is large on the two outermost rows / columns of the map: conv1 of a ring pixel OUTSIDE the map still
        # sees those values through its own 3x3 window, so its (meaningless) taps are several times the interior's -- adding one
        # instead of skipping it would move the result by far more than a rounding (4: large, yet short of saturating every tanh)
        edge = torch.zeros(h, w, dtype=torch.bool)
        edge[:2, :] = edge[-2:, :] = True
        edge[:, :2] = edge[:, -2:] = True
        hid = torch.where(edge, 4.0 * hid.sign() + hid, hid)
    hid = hid.to(DEV)
    Hm = ops.sr_alloc(1, hd, h, w, DEV)[0]
    ops.sr_from_planar(hid, out=Hm)
    inv = torch.rand(1, h, w, generator=g).to(DEV)
    dr = torch.linspace(1 / 935.0, 1 / 425.0, 384).to(DEV)
    return Hm, inv, dr


@pytest.mark.parametrize("big_border", [False, True])
@pytest.mark.parametrize("tile", [2, 4, 8])
@pytest.mark.parametrize("stage,h,w", HEAD_CASES)
def test_depth_head_in_one_launch_is_bitwise_the_two_launches(model, precision, stage, h, w, tile, big_border):
    from effi_mvs_plus_amd import ops, packing
    from effi_mvs_plus_amd.models.update import _pack
    net, _ = model
    blk = net.update_block[stage]
    hd = net.hdim_stage[stage]
    dh = blk.depth_head
    Hm, inv, dr = _head_inputs(blk, hd, h, w, 1000 * stage + h + w, big_border)
    wh1, bh1 = _pack(dh._c1, dh.conv1)
    wh2, bh2 = packing.pack_head_taps(dh.conv2.weight, hd)
    part = ops.conv2d_k3_k1_sr([Hm], wh1.wx, bh1, hd, None, wh2, bh2, 9, relu=False, relu1=True)
    want_inv, want_depth = ops.head_update(part, dh.conv2.bias, inv, dr)
    got_inv, got_depth = ops.depth_head_sr([Hm], wh1.wx, bh1, hd, wh2, bh2, dh.conv2.bias, inv, dr, tile)
    torch.cuda.synchronize()
    assert tuple(got_inv.shape) == tuple(want_inv.shape) and tuple(got_depth.shape) == tuple(want_depth.shape)
    assert torch.isfinite(want_inv).all()
    assert torch.equal(got_inv, want_inv), f"inverse depth differs in {int((got_inv != want_inv).sum())} of {h * w} pixels"
    assert torch.equal(got_depth, want_depth), "depth differs"


@pytest.mark.parametrize("h,w", [(148, 200), (74, 100), (20, 28), (6, 40)])
def test_border_clear_inside_the_context_split(model, h, w):
    """Stage maps of (h, w), (2h, 2w), (4h, 4w) -- (148, 200): the three stage shapes of cfg3 -- poisoned before each form runs."""
    from effi_mvs_plus_amd import ops
    from effi_mvs_plus_amd.models.update import BasicUpdateBlock
    net, _ = model
    before = ops.get_precision()
    ops.set_precision("split")
    try:
        g = torch.Generator().manual_seed(h)
        hds, cds = net.hdim_stage, net.cdim_stage
        ctxs = [torch.randn(hd + cd, h * 2 ** s, w * 2 ** s, generator=g).to(DEV) for s, (hd, cd) in enumerate(zip(hds, cds))]
        nm = BasicUpdateBlock.N_SR_MAPS
        for q4 in ([False] * 3, [True] * 3):
            res = []
            for fused in (False, True):
                blocks = [ops.sr_alloc(nm, hd, c.shape[1], c.shape[2], DEV, clear=False) for hd, c in zip(hds, ctxs)]
                for b in blocks:
                    for m in b:
                        m.t.fill_(3.0)                   # recycled memory: neither form may rely on what the maps held
                if not fused:
                    ops.sr_clear_border(blocks)
                outs = ops.split_tanh_relu_stages_sr(ctxs, hds, cds, [b[-1] for b in blocks], q4=q4, clear=blocks if fused else None)
                torch.cuda.synchronize()
                res.append((blocks, outs))
            (b0, o0), (b1, o1) = res
            for s in range(3):
                assert torch.equal(o0[s][0], o1[s][0]) and torch.equal(o0[s][1], o1[s][1]), f"stage {s}: fp32 halves differ"
                for m0, m1 in zip(b0[s], b1[s]):
                    # interiors of the maps the launch does not write stay poisoned in both forms; borders are zero in both
                    assert torch.equal(m0.t.view(torch.int16), m1.t.view(torch.int16)), f"stage {s}: SR block differs"
                full = b1[s][0].t.float().clone()
                full[:, :, 1:b1[s][0].h + 1, 1:b1[s][0].w + 1, :] = 0
                assert float(full.abs().max()) == 0.0
    finally:
        ops.set_precision(before)


@pytest.mark.parametrize("D,n_views", [(48, 5), (8, 4), (96, 7), (130, 13)])
def test_cascade_setup_is_bitwise_the_two_launches(D, n_views):
    from effi_mvs_plus_amd import ops
    _, pm, dv = synth.synth_sample(128, 160, n_views, seed=D)
    dr = dv[0].to(DEV).contiguous()
    keys = ["stage1", "stage2", "stage3"]
    pairs = [pm[k][0].to(DEV).contiguous() for k in keys]
    want_hyp, want_misc = ops.stage1_hypotheses(dr, D)
    want_rts = ops.compose_rel_proj_stages(pairs)
    (hyp, misc), rts = ops.cascade_setup(dr, D, pairs)
    torch.cuda.synchronize()
    assert torch.equal(hyp, want_hyp) and torch.equal(misc, want_misc)
    assert len(rts) == len(want_rts)
    for a, b in zip(rts, want_rts):
        assert torch.isfinite(b).all() and torch.equal(a, b)
    (hyp1, misc1), rts1 = ops.cascade_setup(dr, D, pairs[:1])          # one stage
    assert torch.equal(hyp1, want_hyp) and torch.equal(misc1, want_misc) and torch.equal(rts1[0], want_rts[0])


@pytest.mark.parametrize("D", [48, 8, 12])                  # 12: the generic kernel (no register form)
@pytest.mark.parametrize("h,w", [(148, 200), (296, 400), (74, 100), (6, 40), (37, 3)])
def test_full_size_confidence_from_the_soft_argmin(D, h, w):
    from effi_mvs_plus_amd import ops
    g = torch.Generator().manual_seed(D + h)
    logits = (3.0 * torch.randn(D, h, w, generator=g)).to(DEV)
    hyp = torch.linspace(425.0, 935.0, D).to(DEV)
    dr = torch.linspace(1 / 935.0, 1 / 425.0, 384).to(DEV)
    want_d, want_c, want_i = ops.softmax_regress_conf(logits, hyp, dr)
    want_up = ops.upsample_nearest(want_c.unsqueeze(0), 4)[0]
    got_d, got_c, got_i, got_up = ops.softmax_regress_conf(logits, hyp, dr, conf_up=4)
    torch.cuda.synchronize()
    assert torch.equal(got_d, want_d) and torch.equal(got_c, want_c) and torch.equal(got_i, want_i)
    assert tuple(got_up.shape) == (4 * h, 4 * w) and torch.equal(got_up, want_up)
    want_up3 = ops.upsample_nearest(want_c.unsqueeze(0), 3)[0]           # a factor without the 16-byte store
    d2, c2, up3 = ops.softmax_regress_conf(logits, hyp, conf_up=3)
    assert torch.equal(d2, want_d) and torch.equal(c2, want_c) and torch.equal(up3, want_up3)


@pytest.mark.parametrize("name,H,W,N,nd", [("cfg1", 128, 160, 4, "8,8,8"), ("cfg2", 576, 800, 5, "48,8,8")])
def test_cascade_with_every_new_option_on_equals_every_new_option_off(name, H, W, N, nd):
    """forward_hot at the sizes of bench.py's cfg1 / cfg2: all 13 depth maps and the confidence, new forms against old forms
    (head_fused = 2: the one-launch depth head at every stage, whatever the per-stage rule keeps by default)."""
    from effi_mvs_plus_amd import ops
    net, _ = build_model(nd, seed=1, device=DEV)
    imgs, pm, dv = synth.synth_sample(H, W, N, seed=3)
    imgs = imgs.to(DEV)
    with torch.no_grad():
        feats = [net.feature(imgs[:, v]) for v in range(N)]
        ctx = net.cnet_depth(imgs[:, 0])
        args = (feats, ctx, {k: v.to(DEV) for k, v in pm.items()}, dv.to(DEV))

        def run(**kw):
            with ops.options(**kw):
                out = net.forward_hot(*args)
            torch.cuda.synchronize()
            return [d.clone() for d in out["depth"]], out["photometric_confidence"].clone()

        off = run(**{k: 0 for k in NEW_OPTIONS})
        forms = {"defaults": run(), "all on": run(**{k: (2 if k == "head_fused" else 1) for k in NEW_OPTIONS})}
        for tile in (2, 8):
            forms[f"head tile {tile}"] = run(head_fused=2, head_fused_tile=tile)
    assert len(off[0]) == 13
    for what, (depths, conf) in forms.items():
        for i, (a, b) in enumerate(zip(depths, off[0])):
            assert torch.equal(a, b), f"{name}, {what}: depth[{i}] differs from the separate launches"
        assert torch.equal(conf, off[1]), f"{name}, {what}: confidence differs"
