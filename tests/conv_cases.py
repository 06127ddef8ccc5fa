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
"""
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
]
VOL_KEYS = {
    0: ("conv3d_roll_oct1_nt1", "conv3d_c8_s11"), 1: ("conv3d_roll_oct2_nt1", "conv3d_c8_s11"), 2: ("conv3d_roll_oct2_nt1", "conv3d_mfma_nt1"),
    3: ("conv3d_x3_nt1", "conv3d_mfma_nt1"), 4: ("conv3d_x3_nt2", "conv3d_mfma_nt2"), 5: ("conv3d_c1_s11", "conv3d_c1_s11"),
    6: ("conv3d_s2x3_nt1", "conv3d_mfma_s2_nt1"), 7: ("conv3d_s2x3_nt2", "conv3d_mfma_s2_nt2"), 8: ("conv3d_c8_s22", "conv3d_c8_s22"),
    9: ("conv3d_c8_s12", "conv3d_c8_s12"), 10: ("deconv3d_x3", "deconv3d_c8_s2"), 11: ("deconv3d_x3", "deconv3d_c8_s2"),
    12: ("deconv3d_c8_s2", "deconv3d_c8_s2"), 13: ("deconv3d_c1_s1", "deconv3d_c1_s1"), 14: ("conv3d_c8_s11", "conv3d_c8_s11"),
    15: ("conv3d_c8_s11", "conv3d_c8_s11")}


def vol_family(i):
    kind, cins, cout, stride, dims, relu, skip = VOL_CASES[i]
    strided = stride != 1
    return family(cins, dims, 1, fam_key(VOL_TILES), seed=100 + i, parities=strided)


def all_families():
    out = dict(all_2d_families())
    for i in range(len(VOL_CASES)):
        out[("vol", i)] = vol_family(i)
    return out
