"""The impulse families of tests/test_gpu_conv_bounds.py, shared with tests/test_conv_bound_host.py (which proves on the CPU that the
emulated arithmetic lies inside every interval on exactly these inputs and that every coverage table is full).  CPU only.

Seam geometry (tile sizes per axis whose multiples are seams; DESIGN.md section 2.2 lists where each comes from):

  split 3x3 (conv2d_x3.hpp, launch_bf16x3)   x: 16-pixel segments; y: a wave's row group of MR rows and the workgroup's 4 MR rows
  generic fp32 MFMA conv2d (conv2d.hip)      16 x 16 pixel tiles
  split-resident 3x3 (conv2d_sr.hip)         the split tile's, plus the 8-wave workgroup's 8 MR rows
  3x3 -> 1x1, 3x3 twice, encoder tail        16-pixel segments in x; 4 / 8 / 16 rows in y (every tile height the forms use)
  5x5 stride 2                               16 output columns = 32 input columns; groups of two output tiles: 8 and 16 input rows
  7x7 single channel                         32 x 8 pixel tiles; in split precision made of 16-pixel segments, 2 rows per wave
  one-launch ConvGRU (gru_fused.hpp)         14 x 14 output tiles inside 16 x 16 staged ones
  one-launch depth head                      2 / 4 / 8 rows per wave: 8 x 16, 16 x 16, 32 x 16 pixel workgroups
  split FPN head                             the split 3x3 tile's at both resolutions
  3-D forms                                  the union over all forms, so that one family serves every branch: z: 2, 4 and 8 planes
                                             per thread and the rolling window's plane runs; y: 4, 8, 16; x: 16, 32
  tile forms of the launch rules              the tiles the rules pick on LARGE maps (form_cases() below): x 64 for the 4 x 64 wide tile of
                                             the split 3x3; y 4 / 8 / 16; z the multiples of each plane run (ZT) of the rolling window
"""
import collections
import functools

import torch

import conv_bound as CB


def split_tiles(mr):
    return [(4,) if mr == 1 else (mr, 4 * mr), (16,)]


SR_TILES = [(4, 8, 16), (16,)]
FUSED_TILES = [(4, 8, 16), (16,)]
K5S2_TILES = [(8, 16), (32,)]
C1K7_TILES = [(2, 4, 8), (16, 32)]      # fp32: 32 x 8 tiles; split: the same tile as 16-pixel segments, two rows per wave of four
VOL_TILES = [(2,), (4, 8, 16), (16, 32)]
GRU_TILES = [(14, 16), (14, 16)]          # the one-launch ConvGRU: 14 x 14 output tiles (16 x 16 staged), on split-resident maps
HEAD_TILES = [(2, 4, 8, 16), (16,)]       # the one-launch depth head: workgroups of 8 x 16, 16 x 16 and 32 x 16 pixels (tile 2, 4, 8)
GENERIC_TILES = [(16,), (16,)]
FORM_TILES = [(4, 8, 16), (16, 64)]       # every tile form of the split 3x3: 4 / 8 / 16 rows of 16-pixel segments, and the 4 x 64 wide tile
FORM_VOL_TILES = [(2, 4, 5, 8, 10), (4, 8, 16), (16, 32)]     # VOL_TILES + the rolling window's runs of 4 (full) and 5 (ragged last) planes

# (cins, cout) of the split 3x3 entry: every cins and every cout of the issue's lists once or more (ragged last 16-tiles: 7, 12, 20)
SPLIT_CHANNELS = [((5,), 7), ((16,), 16), ((16, 16), 12), ((24, 8, 12), 20), ((48,), 48), ((48, 48), 96), ((64,), 64)]
SPLIT_SHAPES = [(21, 28), (37, 52)]
# the generic kernel: (ks, cins, cout, act) of test_conv2d_generic, at w = 30 (scalar stores) and w = 28 (vector stores)
GENERIC = [(3, (5,), 7, 1), (3, (16, 16), 36, 0), (1, (6,), 48, 1), (1, (36, 12), 48, 1), (3, (48,), 96, 1), (1, (96,), 36, 0),
           (3, (17, 3, 9), 20, 3), (3, (64,), 64, 2)]
GENERIC_SHAPES = [(21, 30), (21, 28)]


def split_cases():
    """(cins, cout, (h, w), mr): the small channel counts at both shapes and every rows-per-wave; the large ones (hundreds of members
    each) at 21 x 28 with the rows-per-wave dealt round, and once at 37 x 52."""
    out = []
    for cins, cout in SPLIT_CHANNELS:
        if sum(cins) <= 16:
            out += [(cins, cout, s, mr) for s in SPLIT_SHAPES for mr in (1, 2, 4)]
    out += [((16, 16), 12, (21, 28), 1), ((16, 16), 12, (37, 52), 2), ((24, 8, 12), 20, (21, 28), 4), ((24, 8, 12), 20, (37, 52), 1),
            ((48,), 48, (21, 28), 2), ((48,), 48, (37, 52), 4), ((48, 48), 96, (21, 28), 4), ((64,), 64, (21, 28), 1)]
    return out


@functools.lru_cache(maxsize=None)
def family(cins, spatial, reach=1, tiles=None, seed=0, parities=False):
    """Cached: the GPU file and the host test build each family once; members are never modified."""
    tiles = None if tiles is None else [tuple(t) for t in tiles]
    return CB.impulse_inputs(cins, spatial, reach, tiles, seed, parities)


def fam_key(tiles):
    return tuple(tuple(t) for t in tiles)


def weights(cout, cin, ks, seed, bias, dims=2, transposed=False):
    """He-scaled Gaussian weights [cout, cin, *ks] ([cin, cout, *ks] transposed) and a bias: zero (None) for half of the cases, random
    for the other half -- the caller passes ``bias`` = case index parity."""
    g = torch.Generator().manual_seed(seed)
    shape = ((cin, cout) if transposed else (cout, cin)) + (ks,) * dims
    w = CB.he_weights(shape, cin * ks ** dims, g)
    b = 0.1 * torch.randn(cout, generator=g) if bias else None
    return w, b


def all_2d_families():
    """(name, family) of every 2-D family the GPU file uses."""
    out = {}
    for cins, cout, s, mr in split_cases():
        out[("split", cins, s, mr)] = split_family(cins, s, mr)
    for cins, cout, s, mr, q, bias in SPLIT_GRU:
        out[("split", cins, s, mr)] = split_family(cins, s, mr)
    for ks, cins, cout, act in GENERIC:
        for s in GENERIC_SHAPES:
            out[("generic", ks, cins, s)] = family(cins, s, ks // 2, fam_key(GENERIC_TILES), seed=ks + sum(cins))
    for name, cins, s, reach, tiles, par in FUSED_FAMILIES:
        out[(name, cins, s)] = fused_family(name, cins, s)
    for cins, s in FORM_FAMILIES:
        out[("form", cins, s)] = form_family(cins, s)
    for ks, cins, s in GENERIC_FORM_FAMILIES:
        out[("generic", ks, cins, s)] = family(cins, s, ks // 2, fam_key(GENERIC_TILES), seed=ks + sum(cins))
    for hw, n, form in K5S2_FORM_CASES:
        out[("k5s2", K5S2_FORM_CHANNELS[0], hw)] = k5s2_form_family(hw)
    return out


# (name, cins, spatial, reach, tiles, parities) of the split-resident and the fused / special 2-D forms ("extra": the sparse extra /
# context channels fed beside the main sources)
FUSED_FAMILIES = [
    ("sr", (16,), (37, 52), 1, SR_TILES, False), ("sr", (16, 16), (37, 52), 1, SR_TILES, False), ("sr", (16, 16), (21, 40), 1, SR_TILES, False),
    ("sr", (32,), (21, 40), 1, SR_TILES, False),
    ("k3k1", (16, 16), (21, 28), 1, FUSED_TILES, False), ("k3k1", (16,), (21, 28), 1, FUSED_TILES, False),
    ("k3k1", (8, 8), (37, 52), 1, FUSED_TILES, False), ("extra", (4,), (21, 28), 1, FUSED_TILES, False), ("extra", (3,), (37, 52), 1, FUSED_TILES, False),
    ("twice", (3,), (21, 28), 2, FUSED_TILES, False), ("twice", (8,), (37, 52), 2, FUSED_TILES, False), ("twice", (5,), (12, 16), 2, FUSED_TILES, False),
    ("tail", (16, 16), (21, 28), 2, FUSED_TILES, False), ("tail", (16, 16), (37, 52), 2, FUSED_TILES, False),
    ("ctx", (4,), (21, 28), 2, FUSED_TILES, False), ("ctx", (8,), (37, 52), 2, FUSED_TILES, False),
    ("k5s2", (3,), (21, 28), 2, K5S2_TILES, True), ("k5s2", (8,), (37, 52), 2, K5S2_TILES, True), ("k5s2", (32,), (20, 36), 2, K5S2_TILES, True),
    ("k5s2", (8,), (12, 20), 2, K5S2_TILES, True),
    ("c1k7", (1,), (21, 28), 3, C1K7_TILES, False), ("c1k7", (1,), (37, 52), 3, C1K7_TILES, False),
    ("gru", (16, 16), (37, 52), 2, GRU_TILES, False), ("gru", (32, 32), (29, 16), 2, GRU_TILES, False),
    ("head", (16,), (37, 52), 2, HEAD_TILES, False), ("head", (32,), (21, 28), 2, HEAD_TILES, False),
    ("mask", (16,), (21, 28), 1, FUSED_TILES, False), ("mask", (32,), (37, 52), 1, FUSED_TILES, False),
    ("fpn_top", (32,), (11, 16), 1, FUSED_TILES, False), ("fpn_l1", (8,), (22, 32), 1, FUSED_TILES, False),
    ("fpn_top", (64,), (19, 28), 1, FUSED_TILES, False), ("fpn_l1", (16,), (38, 56), 1, FUSED_TILES, False),
]
# the GRU epilogues of the split 3x3 entry: (cins, cout, (h, w), mr, GRU_Q?, bias)
SPLIT_GRU = [((16, 16), 32, (21, 28), 1, False, 0), ((48, 48), 96, (21, 28), 4, False, 1), ((16, 16), 32, (37, 52), 2, True, 1),
             ((32, 32), 32, (21, 28), 2, True, 0)]


def split_family(cins, hw, mr):
    return family(cins, hw, 1, fam_key(split_tiles(mr)), seed=sum(cins))


def fused_family(name, cins, hw):
    for n, c, s, reach, tiles, par in FUSED_FAMILIES:
        if (n, c, s) == (name, tuple(cins), tuple(hw)):
            return family(c, s, reach, fam_key(tiles), seed=len(name), parities=par)
    raise KeyError((name, cins, hw))


# 3-D: (kind, cin (sources), cout, stride, (D, h, w), relu, skip) -- the branch of Conv3d.run / Deconv3d.run each one takes, per
# precision, is asserted by the GPU file from VOL_KEYS
VOL_CASES = [
    ("conv", (8,), 8, 1, (12, 20, 28), True, False),       # split: roll oct1          fp32: c8_s11
    ("conv", (8, 8), 8, 1, (1, 9, 12), True, False),       # split: roll oct2 (two sources)   fp32: c8_s11
    ("conv", (16,), 16, 1, (3, 10, 16), True, False),      # split: roll oct2          fp32: mfma nt1
    ("conv", (8,), 16, 1, (2, 9, 13), False, False),       # split: x3 (unaligned w)   fp32: mfma nt1, relu=False
    ("conv", (32,), 32, 1, (3, 10, 12), True, False),      # split: x3 nt2             fp32: mfma nt2
    ("conv", (8,), 1, 1, (5, 12, 20), True, False),        # c1_s11 in both (one output channel)
    ("conv", (8,), 16, 2, (12, 20, 28), True, False),      # split: s2x3               fp32: mfma_s2
    ("conv", (16,), 32, 2, (5, 9, 12), True, False),       # split: s2x3 nt2           fp32: mfma_s2 nt2
    ("conv", (8,), 8, 2, (5, 9, 13), True, False),         # c8_s22 in both (unaligned w, cout 8)
    ("conv", (1,), 8, (1, 2, 2), (5, 12, 20), True, False),  # c8_s12 in both
    ("deconv", (16,), 8, 2, (3, 5, 7), True, True),        # split: deconv3d_x3 + skip  fp32: c8_s2 + skip
    ("deconv", (32,), 16, 2, (2, 5, 6), True, False),      # split: deconv3d_x3         fp32: c8_s2
    ("deconv", (8,), 8, 2, (2, 5, 6), False, False),       # c8_s2 in both, relu=False
    ("deconv", (8,), 1, (1, 2, 2), (5, 6, 10), True, False),  # c1_s1 in both
    ("conv", (1,), 8, 1, (5, 9, 12), True, False),         # c8_s11 in both: the one-input-channel kernel
    ("conv", (8,), 8, 1, (3, 9, 12), True, True),          # c8_s11 in both: the additive skip keeps the layer on the vector kernel
    # from here on: cases of the tile-form tests only (FORM_CASES below), not of test_conv3d_every_branch_bounded
    ("conv", (16,), 16, 1, (12, 20, 28), True, False),     # split: roll oct2, the kernel without the row-pair operand, D = 12
]
N_VOL_BRANCH_CASES = 16
VOL_KEYS = {
    0: ("conv3d_roll_oct1_nt1", "conv3d_c8_s11"), 1: ("conv3d_roll_oct2_nt1", "conv3d_c8_s11"), 2: ("conv3d_roll_oct2_nt1", "conv3d_mfma_nt1"),
    3: ("conv3d_x3_nt1", "conv3d_mfma_nt1"), 4: ("conv3d_x3_nt2", "conv3d_mfma_nt2"), 5: ("conv3d_c1_s11", "conv3d_c1_s11"),
    6: ("conv3d_s2x3_nt1", "conv3d_mfma_s2_nt1"), 7: ("conv3d_s2x3_nt2", "conv3d_mfma_s2_nt2"), 8: ("conv3d_c8_s22", "conv3d_c8_s22"),
    9: ("conv3d_c8_s12", "conv3d_c8_s12"), 10: ("deconv3d_x3", "deconv3d_c8_s2"), 11: ("deconv3d_x3", "deconv3d_c8_s2"),
    12: ("deconv3d_c8_s2", "deconv3d_c8_s2"), 13: ("deconv3d_c1_s1", "deconv3d_c1_s1"), 14: ("conv3d_c8_s11", "conv3d_c8_s11"),
    15: ("conv3d_c8_s11", "conv3d_c8_s11"), 16: ("conv3d_roll_oct2_nt1", "conv3d_mfma_nt1")}


def vol_family(i):
    kind, cins, cout, stride, dims, relu, skip = VOL_CASES[i]
    strided = stride != 1
    return family(cins, dims, 1, fam_key(VOL_TILES), seed=100 + i, parities=strided)


def all_families():
    out = dict(all_2d_families())
    for i in range(len(VOL_CASES)):
        if i < N_VOL_BRANCH_CASES:
            out[("vol", i)] = vol_family(i)
        if i in FORM_VOL:
            out[("vol", i, "forms")] = form_vol_family(i)
    return out


# ---------------------------------------------------------------------------------------------
# Tile forms of the launch rules (csrc/launch_form.hpp, ops.launch_form).  Every bound case above runs the form its rule picks for a
# tiny map -- the smallest one.  FORM_CASES lists, per launcher, every form the rule can pick on the maps of the workloads and how a
# small case reaches it: an option where one exists (force_mr, roll_mr / roll_zt / roll_rp, deconv_mr), a 528-wide map for the wide
# tile (the rule's own w >= 512), the rule unaided where a narrow map or a batch crosses its threshold.  FORMS, the table, is DERIVED
# from the cases: a form whose case is removed leaves the table, and tests/test_conv_bound_host.py's sweep over the stage maps of the
# benchmark's workloads fails for it on the CPU.
# ---------------------------------------------------------------------------------------------
FormCase = collections.namedtuple("FormCase", "row query options form how")

MR1, MR2, MR4, WIDE, W8 = (1, 16, 4, 1, 0), (2, 16, 4, 1, 0), (4, 16, 4, 1, 0), (4, 64, 4, 1, 1), (1, 16, 8, 1, 0)
NARROW, WIDE_MAP, WIDE_MAP9 = (21, 28), (21, 528), (9, 528)       # 528 = 8 tiles of 64 + a ragged 16: the rule's own w >= 512
_X3_FORM = {"mr1": (MR1, NARROW, {}), "mr2": (MR2, NARROW, {"force_mr": 2}), "mr4": (MR4, NARROW, {"force_mr": 4}),
            "wide": (WIDE, WIDE_MAP, {"force_mr": 4}), "wide9": (WIDE, WIDE_MAP9, {"force_mr": 4}), "w8": (W8, NARROW, {})}

# the split 3x3 entry and its fused epilogues: (epilogue, split-resident input?, form).  Every epilogue under MR 4 narrow and MR 4
# wide, planar and SR; MR 2 dealt round; the SR eight-wave workgroup where the rule picks it: (48, 48) -> 96 z | r at 21 x 28.
# Channels (the smallest that instantiate the epilogue): see x3_channels.
X3_EPIS = {False: ("plain", "nhwc", "gru_zr", "gru_q", "shuf2", "nhwc_shuf2", "k1", "k1up"), True: ("plain", "gru_zr", "gru_q", "k1", "k1up")}
# The wide tile at 21 x 528 (six tile rows, the last ragged) for the plain epilogues and the 1x1 tail, at 9 x 528 (three tile rows)
# for the others: a third of the pixels.
X3_WIDE21 = ("plain", "k1")
X3_CASES = ([(e, sr, f if f == "mr4" or e in X3_WIDE21 else "wide9") for sr in (False, True) for e in X3_EPIS[sr] for f in ("mr4", "wide")]
            + [("k1", False, "mr2"), ("shuf2", False, "mr2"), ("gru_zr", False, "mr2"), ("nhwc", False, "mr2"),
               ("plain", True, "mr2"), ("k1up", True, "mr2"), ("gru_q", True, "mr2"), ("gru_zr96", True, "w8")])
X3_BF16 = ("plain", False, "wide")          # this case once more in "bf16" precision: it must leave the split interval


K1_EXTRA = 4                          # extra channels fed to the 1x1 of the "k1" cases beside the 3x3's output


def x3_channels(epi):
    """(cins, cout of the 3x3) of an X3 case."""
    return {"plain": ((16,), 16), "nhwc": ((16,), 16), "gru_zr": ((16, 16), 32), "gru_q": ((16, 16), 16), "gru_zr96": ((48, 48), 96),
            "shuf2": ((8,), 8), "nhwc_shuf2": ((8,), 8), "k1": ((16,), 16), "k1up": ((16,), 32)}[epi]


def x3_form(epi, sr, f):
    """(expected form, (h, w) of the map whose tiles the rule counts, options) of an X3 case."""
    form, hw, opts = _X3_FORM[f]
    if "shuf2" in epi:                     # the fine map of the FPN head is twice the coarse one: even sizes
        hw = {NARROW: (22, 32), WIDE_MAP: (10, 528), WIDE_MAP9: (10, 528)}[hw]
    return form, hw, opts


# pair launches, planar and SR: (sr, form)
PAIR_CASES = [(sr, f) for sr in (False, True) for f in ("mr1", "mr2", "mr4", "wide9")]
# image batch of the split 3x3 (PLAIN / NHWC) and the z-batched 3-D form with its sample batch: (launcher, form)
BATCH_CASES = [("x3_batch", f) for f in ("mr1", "mr2", "mr4", "wide9")]
# the generic fp32 kernel has no option: the narrowest map that crosses the threshold of 512 (1x1: 256) tiles, (ks, cins, cout, act,
# (h, w), images, form): 3x3 MR 2 at 9 x 4096 (256 * 2 tiles of 8 rows = 512; 256 of 16 rows), MR 4 at 17 x 4096 (256 * 2 of 16 rows
# = 512); 1x1 MR 4 at 17 x 2048 (128 * 2 = 256).  Batched: the tiles of all images -- 4 images of 9 x 1024 (64 * 2 * 4 = 512 of 8
# rows, 256 of 16) and 4 of 17 x 1024 (64 * 2 * 4 = 512 of 16 rows).
GENERIC_FORM_CASES = [(3, (5,), 7, 1, (9, 4096), 1, MR2), (3, (5,), 7, 1, (17, 4096), 1, MR4), (1, (6,), 48, 1, (17, 2048), 1, MR4),
                      (3, (5,), 7, 0, (9, 1024), 4, MR2), (3, (5,), 7, 0, (17, 1024), 4, MR4), (1, (6,), 48, 0, (17, 1024), 2, MR4)]
GENERIC_FORM_FAMILIES = sorted({(ks, cins, hw) for ks, cins, cout, act, hw, n, form in GENERIC_FORM_CASES})
# rolling window: VOL case 0, (8,) -> 8 at D = 12 (row-pair kernels), case 2, (16,) -> 16 at D = 3 ... see ROLL_CASES: D = 12 with
# (MR, ZT) in {2, 4} x {12, 4, 5}: one run, three full runs, a ragged last run; single, pair and batched entries, row-pair on and off
FORM_VOL = (0, 16)                    # VOL cases with a family on FORM_VOL_TILES
ROLL_ZT = {12: "one run", 4: "full runs", 5: "ragged last run"}
# (entry, VOL case, roll_rp, MR, ZT)
ROLL_CASES = ([("single", 0, None, mr, zt) for mr in (2, 4) for zt in (12, 4, 5)]
              + [("single", 0, 0, 2, 5), ("single", 0, 0, 4, 4), ("single", 16, None, 4, 5), ("single", 16, None, 2, 4),
                 ("pair", 0, None, 4, 5), ("pair", 0, None, 2, 4), ("pair", 0, 0, 4, 4), ("pair", 16, None, 2, 12),
                 ("batch", 0, None, 4, 4), ("batch", 0, None, 2, 5), ("batch", 0, 0, 2, 4), ("batch", 16, None, 4, 12)])
ROLL_BATCH = 4                        # samples per batched launch
ROLL_BF16 = ("single", 0, None, 4, 5)
# the split transposed convolution: VOL cases 10 (cout 8, unaligned rows, skip) and 11 (cout 16): (VOL case, samples, deconv_mr)
ZB_BATCH = 4                          # samples per launch of the z-batched form's sample batch
DECONV_CASES = [(10, 1, 2), (11, 1, 2), (10, 3, 2), (11, 3, 2)]
# Rules without an option, 3-D: the members of a VOL case's family, repeated in turn until the sample batch crosses the rule's
# threshold (the rule counts the workgroups of all samples).  (row, launcher, VOL case, precision, samples, form); the count beside the
# threshold it crosses:
VOL_BATCH_CASES = [
    ("planes3d", "planes3d", 2, "fp32", 88, MR2),          # 3 x 10 x 16: 1 * 2 tiles of 8 rows * 3 planes * 88 = 528 >= 512 (of 16 rows: 264)
    ("planes3d", "planes3d", 2, "fp32", 172, MR4),         # 1 tile of 16 rows * 3 planes * 172 = 516 >= 512
    ("planes3d s2", "planes3d", 6, "fp32", 44, MR2),       # output 6 x 10 x 14: 2 tiles of 8 rows * 6 planes * 44 = 528 >= 512
    ("s2_x3 3-D", "s2_x3", 6, "split", 36, MR2),           # 2 * 6 * 36 = 432 >= 400
    ("c3_planes", "c3_planes", 14, "fp32", 256, (1, 32, 4, 8, 0)),     # 1 -> 8: 5 x 9 x 12: 2 tiles of 32 x 8 * 1 group of 8 planes * 256 = 512
    ("c3_planes", "c3_planes", 5, "fp32", 256, (1, 32, 4, 8, 0)),      # 8 -> 1: 5 x 12 x 20: 2 * 1 * 256 = 512
    ("c3_planes", "c3_planes", 13, "fp32", 512, (1, 32, 4, 8, 0)),     # 8 -> 1 transposed: input 5 x 6 x 10: 1 * 1 * 512 = 512
    ("deconv_k3", "deconv_k3", 12, "fp32", 256, (1, 32, 4, 8, 0)),     # 8 -> 8 stride 2: input 2 x 5 x 6: 1 tile * 2 planes * 256 = 512
]
# Planes per thread of the general vector-ALU 3-D kernel (effi_pick_c3_zpt): 4 (2 at stride (2,2,2)) from 384 workgroups of that form,
# 1 below.  Host rows only, at both sides of the threshold on ONE tile of the 32 x 8 output map (7 x 29): (row, s2, N-tiles of 8 output
# channels, output planes, calls / samples, planes per thread, the record of csrc/vol_host_check.cpp that launches it).
C3_ZPT_FORM_CASES = [
    ("c3_zpt", False, 1, 1532, 1, 1, "s111 1 tile D1532: 383"), ("c3_zpt", False, 1, 1533, 1, 4, "s111 1 tile D1533: 384"),
    ("c3_zpt s2", True, 1, 766, 1, 1, "s222 1 tile D1532: 766 output planes, 383"), ("c3_zpt s2", True, 1, 767, 1, 2, "s222 1 tile D1533: 384"),
    ("c3_zpt", False, 1, 508, 3, 1, "s111 1 tile D508 n_smp3: 127 x 3 = 381"), ("c3_zpt", False, 1, 512, 3, 4, "s111 1 tile D512 n_smp3: 384"),
    ("c3_zpt", False, 1, 764, 2, 1, "pair cin4 s1 1 tile D764: 191 x 2 = 382"), ("c3_zpt", False, 1, 765, 2, 4, "pair cin4 s1 1 tile D765: 384"),
    ("c3_zpt", False, 2, 764, 1, 1, "two tiles of 8 output channels: 382"), ("c3_zpt", False, 2, 765, 1, 4, "two tiles of 8 output channels: 384"),
]
# 5x5 stride 2, both arithmetics (fp32: 512 tiles of 8 output rows; split: 400): (input h, w), images, form.  17 x 8192 -> output 9 x 4096:
# 256 * 2 = 512 tiles; two images of 17 x 4096 -> 128 * 2 * 2 = 512 (one alone: 256, one row per wave -- the form it is compared with)
K5S2_FORM_CASES = [((17, 8192), 1, MR2), ((17, 4096), 2, MR2)]
K5S2_FORM_CHANNELS = ((3,), 24)


def roll_run(zt, D):
    return "one run" if zt >= D else "full runs" if D % zt == 0 else "ragged last run"


def form_family(cins, hw):
    return family(tuple(cins), tuple(hw), 1, fam_key(FORM_TILES), seed=7 + sum(cins))


def form_vol_family(i):
    kind, cins, cout, stride, dims, relu, skip = VOL_CASES[i]
    return family(cins, dims, 1, fam_key(FORM_VOL_TILES), seed=200 + i, parities=stride != 1)


def k5s2_form_family(hw):
    return family(K5S2_FORM_CHANNELS[0], tuple(hw), 2, fam_key(K5S2_TILES), seed=4, parities=True)


def vol_query(launcher, i, n):
    """The ops.launch_form query of VOL case i as a batch of n samples: the map whose tiles the rule of ``launcher`` counts."""
    kind, cins, cout, stride, (D, h, w), relu, skip = VOL_CASES[i]
    st = CB._tuple(stride, 3)
    if kind == "conv":              # the output map
        D, h, w = ((d - 1) // s_ + 1 for d, s_ in zip((D, h, w), st))
    q = dict(launcher=launcher, h=h, w=w, nt=(cout + 15) // 16, planes=D, count=n, cout=cout)
    if launcher == "planes3d":
        q["s2"] = st[0] == 2
    return q


def _form_families():
    out = set()
    for epi, sr, f in X3_CASES:
        cins, _ = x3_channels(epi)
        _, hw, _ = x3_form(epi, sr, f)
        if "shuf2" in epi:
            out.add(((32,), (hw[0] // 2, hw[1] // 2)))
        if epi == "k1":
            out.add(((K1_EXTRA,), hw))
        out.add((cins, hw))
    for sr, f in PAIR_CASES:
        out.add(((16,), _X3_FORM[f][1]))
    for launcher, f in BATCH_CASES:
        out.add(((16,), _X3_FORM[f][1]))
    return sorted(out)


FORM_FAMILIES = _form_families()


def form_cases():
    """Every (launcher row, form) of the table with the query of ops.launch_form that a case asserts, the options it sets, and how it
    reaches the form."""
    out = []
    for epi, sr, f in X3_CASES:
        form, (h, w), opts = x3_form(epi, sr, f)
        nt = (x3_channels(epi)[1] + 15) // 16
        out.append(FormCase("x3 sr" if sr else "x3 planar", dict(launcher="x3", h=h, w=w, nt=nt, sr=sr), opts, form,
                            f"{epi} at {h} x {w}" + (f", {opts}" if opts else ", the rule")))
    out.append(FormCase("x3 planar", dict(launcher="x3", h=21, w=28, nt=1), {}, MR1, "test_split_3x3_every_element_bounded, the rule"))
    out.append(FormCase("x3 sr", dict(launcher="x3", h=37, w=52, nt=2, sr=True), {}, MR1, "test_split_resident_3x3_bounded, the rule"))
    for sr, f in PAIR_CASES:
        form, (h, w), opts = _X3_FORM[f]
        out.append(FormCase("x3_pair sr" if sr else "x3_pair planar", dict(launcher="x3_pair", h=h, w=w, nt=1, sr=sr), opts, form,
                            f"{h} x {w}" + (f", {opts}" if opts else ", the rule")))
    for launcher, f in BATCH_CASES:
        form, (h, w), opts = _X3_FORM[f]
        n = len(form_family((16,), (h, w)).members)
        opts = {} if f == "wide9" else opts           # (48 images of 9 x 528 are 1584 tiles of 16 rows: the rule picks the wide tile)
        out.append(FormCase(launcher, dict(launcher=launcher, h=h, w=w, nt=1, count=n), opts, form,
                            f"the family of {n} images of {h} x {w} as one batch, {opts or 'the rule'}"))
    for f in ("mr1", "mr2", "mr4"):           # the z-batched 3-D form (VOL case 3, 2 x 9 x 13 -> w 13 is unaligned: case 4, 3 x 10 x 12)
        form, _, opts = _X3_FORM[f]
        out.append(FormCase("x3 z-batched", dict(launcher="x3", h=10, w=12, nt=2, planes=3, zb=True), opts, form, f"VOL case 4, {opts or 'the rule'}"))
        out.append(FormCase("x3_zb_batch", dict(launcher="x3_zb_batch", h=10, w=12, nt=2, planes=3, count=ZB_BATCH), opts, form,
                            f"{ZB_BATCH} samples of VOL case 4, {opts or 'the rule'}"))
    for ks, cins, cout, act, (h, w), n, form in GENERIC_FORM_CASES:
        out.append(FormCase(f"conv2d k{ks}", dict(launcher="conv2d", h=h, w=w, nt=(cout + 15) // 16, count=n, k1=ks == 1), {}, form,
                            f"{n} image(s) of {h} x {w}: the rule"))
    out.append(FormCase("conv2d k3", dict(launcher="conv2d", h=21, w=28, nt=1), {}, MR1, "test_generic_fp32_conv2d_bounded at 21 x 28"))
    out.append(FormCase("conv2d k3", dict(launcher="conv2d", h=21, w=30, nt=1), {}, (0, 16, 4, 1, 0), "test_generic_fp32_conv2d_bounded at 21 x 30"))
    out.append(FormCase("conv2d k1", dict(launcher="conv2d", h=21, w=28, nt=3, k1=True), {}, MR2, "test_generic_fp32_conv2d_bounded at 21 x 28"))
    out.append(FormCase("conv2d k1", dict(launcher="conv2d", h=21, w=30, nt=3, k1=True), {}, (0, 16, 4, 1, 0), "test_generic_fp32_conv2d_bounded at 21 x 30"))
    for entry, i, rp, mr, zt in ROLL_CASES:
        kind, cins, cout, stride, (D, h, w), relu, skip = VOL_CASES[i]
        opts = {"roll_mr": mr, "roll_zt": zt}          # (the rule's own pick on these maps: 2 rows per wave, runs of ONE plane)
        if rp is not None:
            opts["roll_rp"] = rp
        variant = 1 if cout <= 8 and rp != 0 else 0
        out.append(FormCase("roll", dict(launcher="roll", h=h, w=w, nt=(cout + 15) // 16, planes=D, cout=cout,
                                         count={"single": 1, "pair": 2, "batch": ROLL_BATCH}[entry], oct2=sum(cins) == 16), opts,
                            (mr, 16, 4, zt, variant), f"{entry} entry, VOL case {i}, {opts}: {ROLL_ZT[zt]}"))
    for row, launcher, i, mode, n, form in VOL_BATCH_CASES:
        out.append(FormCase(row, vol_query(launcher, i, n), {}, form, f"{n} samples of VOL case {i}: the rule"))
        small = {MR2: MR1, MR4: MR1}.get(form, (1, 32, 4, 4, 0))
        out.append(FormCase(row, vol_query(launcher, i, 1), {}, small, f"VOL case {i} in test_conv3d_every_branch_bounded: the rule"))
    for row, s2, nt, planes, count, zpt, how in C3_ZPT_FORM_CASES:
        out.append(FormCase(row, dict(launcher="c3_zpt", h=7, w=29, nt=nt, planes=planes, count=count, s2=s2), {}, (1, 32, 4, zpt, 0),
                            f"vol_host_check, {how}: the rule"))
    (kc, kco), (h, w) = K5S2_FORM_CHANNELS, (21, 28)
    for hw, n, form in K5S2_FORM_CASES + [((21, 28), 1, MR1)]:
        q = dict(h=(hw[0] - 1) // 2 + 1, w=(hw[1] - 1) // 2 + 1, nt=(kco + 15) // 16, count=n)
        how = f"{n} image(s) of {hw[0]} x {hw[1]}: the rule" if form != MR1 else "test_5x5_stride2_bounded: the rule"
        out.append(FormCase("k5s2", dict(q, launcher="k5s2"), {}, form, how))
        out.append(FormCase("s2_x3 2-D", dict(q, launcher="s2_x3"), {}, form, how))
    for i, n, mr in DECONV_CASES:
        kind, cins, cout, stride, (D, h, w), relu, skip = VOL_CASES[i]
        out.append(FormCase("deconv_x3", dict(launcher="deconv_x3", h=h, w=w, planes=D, cout=cout, count=n), {"deconv_mr": mr}, (mr, 16, 4, 1, 0),
                            f"{n} sample(s) of VOL case {i}, deconv_mr={mr}"))
        out.append(FormCase("deconv_x3", dict(launcher="deconv_x3", h=h, w=w, planes=D, cout=cout, count=1), {}, MR1, f"VOL case {i}, the rule"))
    return out


def table_form(row, form, D=1):
    """A form as the table keys it: the rolling window by (rows per wave, kind of plane run, row-pair operand?) -- ZT itself takes
    every value up to D on the workloads' maps; what a case can get wrong is a refill at a run boundary and a ragged last run."""
    form = tuple(form)
    return (form[0], roll_run(form[3], D), form[4]) if row == "roll" else form


def forms():
    """The table: row (launcher) -> {form: how the first case that launches it reaches it}."""
    out = {}
    for c in form_cases():
        out.setdefault(c.row, {}).setdefault(table_form(c.row, c.form, c.query.get("planes", 1)), c.how)
    return out


# The workloads bench.py names: image sizes of cfg1-cfg5, their stage maps at 1/8, 1/4, 1/2 and full resolution, D of the cascades,
# 1-5 images / samples per launch.
WORKLOAD_IMAGES = [(128, 160), (576, 800), (1184, 1600), (1056, 1920)]
WORKLOAD_MAPS = sorted({(h // s, w // s) for h, w in WORKLOAD_IMAGES for s in (8, 4, 2, 1)})
WORKLOAD_D = (48, 32, 8)
WORKLOAD_COUNTS = (1, 2, 3, 4, 5)


def workload_queries():
    """(row, query, D) of every launch-form query of the sweep: each launcher of the table over every stage map, every N-tile count
    its entry instantiates and every count."""
    for h, w in WORKLOAD_MAPS:
        for nt in (1, 2, 3, 4, 6):
            for sr in (False, True):
                yield "x3 sr" if sr else "x3 planar", dict(launcher="x3", h=h, w=w, nt=nt, sr=sr), 1
                if nt <= 4:
                    yield "x3_pair sr" if sr else "x3_pair planar", dict(launcher="x3_pair", h=h, w=w, nt=nt, sr=sr), 1
            for n in WORKLOAD_COUNTS:
                yield "x3_batch", dict(launcher="x3_batch", h=h, w=w, nt=nt, count=n), 1
                for ks in (3, 1):
                    yield f"conv2d k{ks}", dict(launcher="conv2d", h=h, w=w, nt=nt, count=n, k1=ks == 1), 1
        for D in WORKLOAD_D:
            for nt in (1, 2):
                yield "x3 z-batched", dict(launcher="x3", h=h, w=w, nt=nt, planes=D, zb=True), D
                for n in WORKLOAD_COUNTS:
                    yield "x3_zb_batch", dict(launcher="x3_zb_batch", h=h, w=w, nt=nt, planes=D, count=n), D
                    for cout in ((8, 16) if nt == 1 else (32,)):
                        for oct2 in (False, True):
                            q = dict(launcher="roll", h=h, w=w, nt=nt, planes=D, cout=cout, oct2=oct2)
                            yield "roll", dict(q, count=n), D
            for n in WORKLOAD_COUNTS:
                for cout in (8, 16):
                    yield "deconv_x3", dict(launcher="deconv_x3", h=h, w=w, planes=D, cout=cout, count=n), D
                    yield "deconv_k3", dict(launcher="deconv_k3", h=h, w=w, planes=D, cout=cout, count=n), D
                yield "c3_planes", dict(launcher="c3_planes", h=h, w=w, planes=D, count=n), D
                for nt in (1, 2):
                    yield "c3_zpt", dict(launcher="c3_zpt", h=h, w=w, nt=nt, planes=D, count=n), D
                    yield "c3_zpt s2", dict(launcher="c3_zpt", h=h, w=w, nt=nt, planes=D, count=n, s2=True), D
                    yield "planes3d", dict(launcher="planes3d", h=h, w=w, nt=nt, planes=D, count=n), D
                    yield "planes3d s2", dict(launcher="planes3d", h=h, w=w, nt=nt, planes=D, count=n, s2=True), D
                    yield "s2_x3 3-D", dict(launcher="s2_x3", h=h, w=w, nt=nt, planes=D, count=n), D
        for n in WORKLOAD_COUNTS:
            for nt in (1, 2, 4):
                yield "k5s2", dict(launcher="k5s2", h=h, w=w, nt=nt, count=n), 1
                yield "s2_x3 2-D", dict(launcher="s2_x3", h=h, w=w, nt=nt, count=n), 1
