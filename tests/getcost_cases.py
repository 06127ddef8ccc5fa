"""Case lists of the GetCost read-out tests, shared by the CPU proof (test_getcost_pixel_host.py: the fp32 restatement of
``effi_getcost_pixel`` stands in for the kernel) and the GPU tests (test_gpu_getcost_readout.py).  Everything here is CPU torch."""
import torch

import interval_cases as cases
import interval_ref as IR
import test_gpu_lookup_taps as taps            # the tap-class rig: 6 x 8 map, one class per pixel

H, W, DMIN, DMAX = taps.H, taps.W, taps.DMIN, taps.DMAX
ALL = taps.ALL

# (Dcur, Dreg, nq, h, w, per_pixel): test_getcost_inside's four, a Dreg != Dcur case with nq = 4, nq = 2 -- and nq = 3 at 20 x 29, the
# map that spans three workgroups (the last one partial), so that ``encoder_inputs`` (nq = 3 only) runs its GetCost blocks behind
# more than one 7x7 tile of the same grid
INSIDE_CASES = [(8, 8, 3, 9, 13, False), (48, 8, 4, 20, 29, True), (2, 48, 3, 9, 13, True), (48, 48, 4, 20, 29, False),
                (8, 48, 4, 9, 13, True), (8, 8, 2, 9, 13, False), (48, 8, 3, 20, 29, True)]

# planar [D,h,w]; the zero-copy pixel-major VIEW [h*w,1,1,D] of it (same memory: ds = h*w, ps = 1, through the entry's 4-D branch);
# and the mixed ones, where one volume is pixel-major IN MEMORY (ds = 1, ps = D) and the other planar: cds != rds and cps != rps
LAYOUTS = ("planar", "view", "cur_pixel_major", "reg_pixel_major")
MIXED = ("cur_pixel_major", "reg_pixel_major")


def _lay(vol, kind):
    D, h, w = vol.shape
    vol = vol.contiguous()
    if kind == "planar":
        return vol
    if kind == "view":
        v = vol.unsqueeze(0).permute(0, 2, 3, 1).reshape(h * w, 1, 1, D)
        assert v.data_ptr() == vol.data_ptr()
        return v
    assert kind == "pixel_major"
    return vol.permute(1, 2, 0).contiguous().view(h * w, 1, 1, D)


def layout(cur, reg, name):
    """cur / reg [D,h,w] (any device) -> the two tensors handed to the entry."""
    kc, kr = {"planar": ("planar", "planar"), "view": ("view", "view"), "cur_pixel_major": ("pixel_major", "planar"),
              "reg_pixel_major": ("planar", "pixel_major")}[name]
    return _lay(cur, kc), _lay(reg, kr)


def flat_and_strides(vol, h, w):
    """What ``ops._vol_strides`` makes of a volume, for the restatement: (flat storage from the volume's first element, (ds, ps), D)."""
    if vol.dim() == 3:
        D = vol.shape[0]
        return vol.contiguous().reshape(-1), (h * w, 1), D
    assert vol.dim() == 4 and vol.shape[0] == h * w
    D, ds, ps = vol.shape[3], vol.stride(3), vol.stride(0)
    return vol.as_strided(((h * w - 1) * ps + (D - 1) * ds + 1,), (1,)), (ds, ps), D


def inside_case(Dcur, Dreg, nq, h, w, per_pixel, input_is_depth):
    """``interval_cases.getcost_case`` with the float64 queries and both intervals -> dict."""
    from oracle import effi_oracle as O
    cur, reg, x, disp_range, itv, dmin, dmax = cases.getcost_case(Dcur, Dreg, nq, h, w, per_pixel, input_is_depth)
    qd = IR.getcost_queries(O, x, disp_range, itv, nq, input_is_depth)
    iv = [IR.lookup_interval(v, qd, dmin, dmax, n_round=IR.GETCOST_ROUNDINGS) for v in (cur, reg)]
    return dict(cur=cur, reg=reg, x=x, disp_range=disp_range, itv=itv, dmin=dmin, dmax=dmax, nq=nq, h=h, w=w,
                input_is_depth=input_is_depth, qd=qd, iv=iv)


def shares(vol, q, dmin, dmax):
    """test_gpu_intervals._shares: at least half of the queries inside the volume's range, at least a twentieth outside."""
    pos, _ = IR.lookup_position(q, dmin, dmax, vol.shape[0])
    inside = float(((pos >= 0) & (pos <= vol.shape[0] - 1)).double().mean())
    assert inside >= 0.5 and 1.0 - inside >= 0.05, f"queries in range: {inside:.3f}"


# ---- the tap-class rig for any nq, as depth or as normalised inverse depth ---------------------------------------------------------
def rig_disp_range():
    return taps._disp_range()


def rig_inputs(kinds, D, nq, input_is_depth):
    """-> (x [H,W] fp32, interval [1] fp32).  The nq hypotheses of a pixel lie within +-0.1 positions of its target (fractional part
    0.5): GetCost spreads them over +-(nq // 2) intervals, so one interval is 0.1 / (nq // 2) positions.  The normalised inverse depth
    is the float64 inverse of ``effi_inv_to_depth`` rounded to fp32; the queries are rebuilt from that fp32 value."""
    depth = taps._depth_at(taps._targets(kinds, D), D)
    itv = torch.tensor([taps.SPREAD / (nq // 2) * taps._den() / (D - 1)], dtype=torch.float32)
    if input_is_depth:
        return depth.float(), itv
    dr = rig_disp_range().double()
    return ((1.0 / depth - dr[0]) / (dr[-1] - dr[0])).float(), itv


def rig_queries(x, itv, nq, input_is_depth):
    from oracle import effi_oracle as O
    return IR.getcost_queries(O, x, rig_disp_range(), itv, nq, input_is_depth)


def first_tap(q, D):
    """First tap of every query, certain under GetCost's own position bound."""
    tpos, dt = IR.lookup_box(q, DMIN, DMAX, D, n_round=IR.GETCOST_ROUNDINGS)
    x0 = torch.floor(tpos - dt)
    assert torch.equal(x0, torch.floor(tpos + dt)), "a query whose first tap is uncertain"
    return x0


def classes(q, D):
    """Per query index k: how many pixels fall into each tap class -> {class: [count of k = 0, 1, ..]}."""
    x0 = first_tap(q, D)
    sel = {"both": (x0 >= 0) & (x0 <= D - 2), "upper": x0 == -1, "lower": x0 == D - 1, "out_low": x0 <= -2, "out_high": x0 >= D}
    return {k: [int(v[i].sum()) for i in range(q.shape[0])] for k, v in sel.items()}


def rig_case(D, nq, input_is_depth, kinds=ALL, nan=None, seed=31):
    """Random volumes [D,H,W] with the rig's queries and intervals -> dict (as ``inside_case``).  nan = "all": both volumes NaN
    everywhere (kinds must keep every tap outside); nan = "edges": NaN in planes 0 and D - 1, the intervals being those of the volume
    with these planes 0 (kinds must keep every selected tap off them: asserted by the caller with ``first_tap``)."""
    g = torch.Generator().manual_seed(seed * D)
    cur, reg = torch.randn(D, H, W, generator=g), torch.randn(D, H, W, generator=g)
    if nan == "all":
        cur, reg = torch.full_like(cur, float("nan")), torch.full_like(reg, float("nan"))
    elif nan == "edges":
        for v in (cur, reg):
            v[0] = float("nan")
            v[D - 1] = float("nan")
    x, itv = rig_inputs(kinds, D, nq, input_is_depth)
    qd = rig_queries(x, itv, nq, input_is_depth)
    dmin, dmax = torch.tensor([DMIN]), torch.tensor([DMAX])
    iv = [IR.lookup_interval(torch.nan_to_num(v), qd, dmin, dmax, n_round=IR.GETCOST_ROUNDINGS) for v in (cur, reg)]
    return dict(cur=cur, reg=reg, x=x, disp_range=rig_disp_range(), itv=itv, dmin=dmin, dmax=dmax, nq=nq, h=H, w=W,
                input_is_depth=input_is_depth, qd=qd, iv=iv)


def assert_every_class(c, D):
    """Every tap class present at EVERY query index (nq = 4: in both QB halves)."""
    cls = classes(c["qd"], D)
    assert all(n > 0 for v in cls.values() for n in v), cls
    return cls


def assert_all_outside(c, D):
    cls = classes(c["qd"], D)
    assert sum(cls["both"] + cls["upper"] + cls["lower"]) == 0 and min(cls["out_low"] + cls["out_high"]) > 0, cls


def assert_off_the_edge_planes(c, D):
    x0 = first_tap(c["qd"], D)
    inner = (x0 >= 1) & (x0 <= D - 3)
    assert bool((inner | (x0 <= -2) | (x0 >= D)).all()), "a query touches a NaN plane"
    assert D < 4 or int(inner.sum()) > 0


NAN_EDGE_KINDS = ("inner", "out_low", "out_high")


# ---- volumes that span 2^31 bytes -------------------------------------------------------------------------------------------------
BIG_ELEMS = (1 << 29) + 4096            # floats of the one large buffer: a little over 2^31 bytes
BIG_REG_OFFSET = 16                     # reg's first element in it (cur's: 0): the two pixel-major views interleave


def span_bytes(npix, ps, D, ds):
    """The extent ``effi_vol_fits32`` compares with 2^31 (common.hpp)."""
    return ((npix - 1) * ps + (D - 1) * ds + 1) * 4


def interleaved_views(buf, ps, cur, reg):
    """cur / reg [D,h,w] laid pixel-major (ds = 1) with pixel stride ``ps`` over the flat buffer ``buf`` of their device: cur from
    element 0, reg from BIG_REG_OFFSET.  Only the elements of the two views are written -> the [h*w,1,1,D] views."""
    views = []
    for vol, off in ((cur, 0), (reg, BIG_REG_OFFSET)):
        D, h, w = vol.shape
        assert D <= BIG_REG_OFFSET and BIG_REG_OFFSET + D <= ps and off + (h * w - 1) * ps + D <= buf.numel()
        v = buf.as_strided((h * w, 1, 1, D), (ps, D, D, 1), off)
        v.copy_(vol.permute(1, 2, 0).reshape(h * w, 1, 1, D))
        views.append(v)
    return views


def compact_views(cur, reg):
    """The same values as contiguous pixel-major tensors [h*w,1,1,D] (ds = 1, ps = D)."""
    return [_lay(v, "pixel_major") for v in (cur, reg)]


def big_pixel_strides(npix, D, ds=1):
    """-> (ps_below, ps_at_or_above): the pixel stride with the largest extent below 2^31 bytes (32-bit offsets at their largest)
    and the next one, the smallest extent at or above it (64-bit addressing)."""
    below = ((1 << 29) - 2 - (D - 1) * ds) // (npix - 1)
    assert span_bytes(npix, below, D, ds) < (1 << 31) <= span_bytes(npix, below + 1, D, ds)
    return below, below + 1
