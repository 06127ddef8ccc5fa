// The launch rules of the convolution kernels as pure host functions: sizes, N-tile count, image / sample / pair counts and a snapshot
// of the tuning options go in, the tile form comes out.  Every launcher calls the pick function of its rule and launches what it
// returns; effi_launch_form (api.hip) calls the same functions without launching anything, so that a test can assert the form a case
// is written for (tests/conv_cases.py: FORMS) and sweep the forms the workloads take.  There is no second copy of a rule.
// The rules of the vector-ALU 3-D kernels (conv3d.hip) are among them: planes per thread of the 1 -> 8 / 8 -> 1 kernels and of the
// general kernel (effi_pick_c3_planes, effi_pick_c3_zpt), output channels per thread of the transposed one, the element limits of
// the two dedicated kernels; csrc/vol_host_check.cpp pins them through the entries.
// The rules of the warp and correlation kernels (warpcorr.hip) are at the end: which kernel a stage-1 ("views") call and a call of
// the dynamic stage take, with the size of their LDS window; csrc/warp_host_check.cpp pins them through the entries.
// In front of the rules, the helpers every launcher dispatches with: effi_switch (a run-time value as a template argument) and
// effi_launch (effi_launch_lds: with dynamic LDS).
#pragma once
#include "common.hpp"
#include <type_traits>

// f(std::integral_constant<int, V>) for the V of Vs... that equals v; ``miss`` when there is none
template <int... Vs, class F>
static int effi_switch_or(int miss, long v, F&& f) {
    int rc = miss;
    (void)(... || (v == Vs ? (rc = f(std::integral_constant<int, Vs>{}), true) : false));
    return rc;
}
// rows per wave, tile forms and flags: a value outside the set is a bad argument (of an option, as a rule)
template <int... Vs, class F>
static int effi_switch(long v, F&& f) { return effi_switch_or<Vs...>(EFFI_ERR_BADARG, v, f); }
// N-tile and channel counts (and other sizes a kernel is instantiated for): a layer outside the set is unsupported
template <int... Vs, class F>
static int effi_switch_nt(long v, F&& f) { return effi_switch_or<Vs...>(EFFI_ERR_UNSUPPORTED, v, f); }

template <auto KERNEL, class... Args>
static int effi_launch_lds(dim3 grid, int threads, size_t dynamic_lds, hipStream_t st, const Args&... args) {
    hipLaunchKernelGGL(KERNEL, grid, dim3(threads), dynamic_lds, st, args...);
    return hipPeekAtLastError() == hipSuccess ? EFFI_OK : EFFI_ERR_LAUNCH;
}
template <auto KERNEL, class... Args>
static int effi_launch(dim3 grid, int threads, hipStream_t st, const Args&... args) {
    return effi_launch_lds<KERNEL>(grid, threads, 0, st, args...);
}

#ifndef EFFI_C3_TX
#define EFFI_C3_TX 32          // tile of the vector-ALU 3-D kernels (A/B builds: -DEFFI_C3_TX=64 -DEFFI_C3_TY=4)
#define EFFI_C3_TY 8
#endif

struct EffiFormOpts {           // the options a rule reads, defaults of the thresholds resolved
    long force_mr;              // 0 = the rule
    long mr4_min, mr4_nt2_max, mr2_min;
    long wide_tiles;            // -1 = the rule
    long sr_waves, roll_mr, roll_zt, roll_rp, deconv_mr;        // EFFI_OPT_UNSET = the rule
    long roll_slide;            // 0 = the three-slot body of the row-pair rolling kernel (same tile form, kernels of their own)
};

static inline long effi_opt_or(int id, long dflt) {
    const long v = effi_option(id);
    return v == EFFI_OPT_UNSET ? dflt : v;
}

static inline EffiFormOpts effi_form_opts() {
    EffiFormOpts o;
    o.force_mr = effi_opt_or(EFFI_OPT_FORCE_MR, 0);
    o.mr4_min = effi_opt_or(EFFI_OPT_MR4_MIN, 400);
    o.mr4_nt2_max = effi_opt_or(EFFI_OPT_MR4_NT2_MAX, 1024);
    o.mr2_min = effi_opt_or(EFFI_OPT_MR2_MIN, 400);
    o.wide_tiles = effi_opt_or(EFFI_OPT_WIDE_TILES, -1);
    o.sr_waves = effi_option(EFFI_OPT_SR_WAVES);
    o.roll_mr = effi_option(EFFI_OPT_ROLL_MR);
    o.roll_zt = effi_option(EFFI_OPT_ROLL_ZT);
    o.roll_rp = effi_option(EFFI_OPT_ROLL_RP);
    o.deconv_mr = effi_option(EFFI_OPT_DECONV_MR);
    o.roll_slide = effi_opt_or(EFFI_OPT_ROLL_SLIDE, 1);
    return o;
}

struct EffiForm {
    int rows;       // rows per wave (the kernels' MR); 0 = the 16 x 16 kernel of the generic convolution on unaligned rows
    int cols;       // columns of a workgroup's tile
    int waves;      // waves per workgroup
    int planes;     // planes per workgroup (rolling window), planes per thread (1 -> 8 / 8 -> 1 kernels), output channels per thread
                    // (vector transposed convolution); 1 elsewhere
    int variant;    // 1 = the 4 x 64 "wide" instantiation (split 3x3) / the row-pair operand kernel (rolling window)
};

// ---- split-precision 3x3 (conv2d_x3.hpp) ------------------------------------------------------------------------------------------
// Rows per wave (MR): 4 rows amortise the B fragments best, but the grid must still cover the 256 CUs (>= ~400 workgroups), and with
// two N-tiles the 4-row variant drops to 2 workgroups per CU where the 2-row one keeps 4: on large maps the latter wins.  ``count``:
// the planes (z-batched form), images, samples x planes or the 2 of a pair whose tiles the rule counts.
static inline int effi_pick_x3_rows(int nt, int h, int w, long count, const EffiFormOpts& o) {
    const long cols = effi_cdiv(w, 16);
    const long t4 = cols * effi_cdiv(h, 16) * count, t2 = cols * effi_cdiv(h, 8) * count;
    int mr;
    if (t4 >= o.mr4_min && !(nt == 2 && t4 >= o.mr4_nt2_max)) mr = 4;
    else if (t2 >= o.mr2_min) mr = 2;
    else mr = 1;
    if (o.force_mr) mr = (int)o.force_mr;
    return mr;
}

// launch_bf16x3: wide tiles (4 rows x 64 columns) pay off on the large maps only (measured with an HBM-cold working set, 592x800:
// 16->16 23.8 -> 22.6 us, 32->12 33.3 -> 30.7, 32->16 GRU update 41.9 -> 38.6; 296x400: 38 -> 49 us for 64->64).
// Eight waves per workgroup (split-resident maps): the tile of 4-row waves' workgroup at half the rows per wave, twice the pixels
// behind one copy of the weight fragments.  Rule (option sr_waves unset): one row per wave AND six N-tiles -- the stage-1 z | r
// layer, whose 61 KB of weight fragments per chunk and 64-pixel workgroup are what its launch moves (84.7-87.0 -> 78.4-79.0 us per
// view, profiles/r04_ai_sr_waves_ab2.txt); every other layer is equal or slower with eight waves (stage-3 z | r: +12 us).
// sr_waves = 8: wherever the rule picks 1 or 2 rows per wave (A/B); sr_waves = 4: never.
static inline EffiForm effi_pick_x3(int nt, int h, int w, long planes, bool zb, bool sr, const EffiFormOpts& o) {
    const int mr = effi_pick_x3_rows(nt, h, w, planes, o);
    const bool wide = o.wide_tiles >= 0 ? o.wide_tiles != 0 : (mr == 4 && w >= 512 && !zb);
    if (wide) return EffiForm{mr, 16 * mr, 4, 1, 1};
    if (sr && ((o.sr_waves == 8 && mr <= 2) || (o.sr_waves == EFFI_OPT_UNSET && mr == 1 && nt >= 6))) return EffiForm{mr, 16, 8, 1, 0};
    return EffiForm{mr, 16, 4, 1, 0};
}

// launch_bf16x3 with an image batch: the single-image rule on the tile count of ALL images
static inline EffiForm effi_pick_x3_batch(int nt, int h, int w, long n_img, const EffiFormOpts& o) {
    const int mr = effi_pick_x3_rows(nt, h, w, n_img, o);
    const bool wide = o.wide_tiles >= 0 ? o.wide_tiles != 0 : (mr == 4 && w >= 512);
    return wide ? EffiForm{mr, 16 * mr, 4, 1, 1} : EffiForm{mr, 16, 4, 1, 0};
}

// launch_bf16x3, z-batched form with a sample batch: the tiles of all planes of all samples; never the wide tiles
static inline EffiForm effi_pick_x3_zb_batch(int nt, int h, int w, long planes, const EffiFormOpts& o) {
    return EffiForm{effi_pick_x3_rows(nt, h, w, planes, o), 16, 4, 1, 0};
}

// launch_bf16x3_pair: tile shape chosen as launch_bf16x3 does for two planes (eight waves only with sr_waves = 8)
static inline EffiForm effi_pick_x3_pair(int nt, int h, int w, bool sr, const EffiFormOpts& o) {
    const int mr = effi_pick_x3_rows(nt, h, w, 2, o);
    if (mr == 4 && w >= 512) return EffiForm{4, 64, 4, 1, 1};
    if (sr && o.sr_waves == 8 && mr <= 2) return EffiForm{mr, 16, 8, 1, 0};
    return EffiForm{mr, 16, 4, 1, 0};
}

// ---- generic fp32 MFMA convolution (conv2d.hip: launch2d, single image or batch) ---------------------------------------------------
// rows per wave: the largest of {4, 2, 1} that still yields >= 2 workgroups per CU (256 CUs) over the tiles of all images; a 1x1
// convolution takes at least two rows (and four from 256 tiles); rows of w % 4 != 0 take the 16 x 16 kernel
static inline EffiForm effi_pick_generic(int ks, int h, int w, long n_img) {
    if (w & 3) return EffiForm{0, 16, 4, 1, 0};
    const long cols = effi_cdiv(w, 16);
    const long t4 = cols * effi_cdiv(h, 16) * n_img, t2 = cols * effi_cdiv(h, 8) * n_img;
    int mr;
    if (t4 >= 512 || (ks == 1 && t4 >= 256)) mr = 4;
    else if (t2 >= 512 || ks == 1) mr = 2;
    else mr = 1;
    return EffiForm{mr, 16, 4, 1, 0};
}

// ---- fp32 z-batched 3-D forms (launch3d_planes, stride 1 and 2), 5x5 stride 2 (launch_k5s2) ----------------------------------------
// rows per wave: keep >= 2 workgroups per CU over all planes (of all samples) / all images; the stride-2 forms stop at two rows
static inline EffiForm effi_pick_planes(int h, int w, long planes, int max_rows) {
    const long cols = effi_cdiv(w, 16);
    if (max_rows >= 4 && cols * effi_cdiv(h, 16) * planes >= 512) return EffiForm{4, 16, 4, 1, 0};
    if (cols * effi_cdiv(h, 8) * planes >= 512) return EffiForm{2, 16, 4, 1, 0};
    return EffiForm{1, 16, 4, 1, 0};
}

// ---- split-precision stride-2 forms (launch_s2_x3: 2-D, z-batched, either one batched) --------------------------------------------
// two rows per wave from 400 workgroups: tiles x N-tile groups x planes (of all samples) or images
static inline EffiForm effi_pick_s2_x3(int h, int w, int ngroups, long planes) {
    const int cols = effi_cdiv(w, 16);
    return EffiForm{(long)cols * effi_cdiv(h, 8) * ngroups * planes >= 400 ? 2 : 1, 16, 4, 1, 0};
}

// ---- rolling-window 3-D convolution (launch_roll) ---------------------------------------------------------------------------------
// Rows per wave (MR) and planes per workgroup (ZT) from a small cost model fitted to sweeps at the cfg3 shapes
// (tools/sweep_roll.sh): the chip holds 256 * occ workgroups at a time (occ from the LDS image / register count of the
// instantiation), a launch takes ceil(workgroups / that) rounds, and a workgroup costs (ZT + 3) plane steps (3 ~ filling
// the window), 1.3x as much with 4 rows per wave as with 2.  E.g. 8->8 at 48x148x200: MR 4 / ZT 6 (1040 workgroups, 3
// rounds) 74 us, MR 2 / ZT 16 (741 workgroups, 1 round) 55 us.  ``mult``: 2 for a pair, the samples of a batch, else 1.
static inline EffiForm effi_pick_roll(int noct, int nt, int cout, int h, int w, int D, long mult, const EffiFormOpts& o) {
    const int cols = effi_cdiv(w, 16);
    const bool rp = nt == 1 && cout <= 8 && o.roll_rp != 0;      // row-pair operand (see conv3d_roll_rp_bf16x3_body)
    int mr = 2, zt = D;
    double best = 1e30;
    for (int m = 2; m <= 4; m += 2) {
        // (row-pair kernels, weights in registers: 3 workgroups per CU with 8 input channels, 2 with 16, whatever MR)
        const int occ = rp ? (noct == 1 ? 3 : 2) : (noct == 1 && nt == 1) ? (m == 2 ? 3 : 2) : (noct == 1 ? 2 : (nt == 1 && m == 2 ? 2 : 1));
        const long tiles_m = (long)cols * effi_cdiv(h, 4 * m), slots = 256L * occ;
        for (int nz = 1; nz <= D; ++nz) {
            const int z = effi_cdiv(D, nz);
            const long wgs = tiles_m * effi_cdiv(D, z) * mult;     // (batched: the workgroups of all samples)
            const double cost = (double)effi_cdiv(wgs, slots) * (z + 3) * (m == 4 ? 1.3 : 1.0);
            if (cost < best - 1e-9) { best = cost; mr = m; zt = z; }
        }
    }
    if (o.roll_mr != EFFI_OPT_UNSET) mr = (int)o.roll_mr;       // A/B overrides of the rounds model
    if (o.roll_zt != EFFI_OPT_UNSET) zt = (int)o.roll_zt;
    return EffiForm{mr, 16, 4, zt, rp ? 1 : 0};
}

// ---- split-precision transposed 3-D convolution (deconv3d_k3s2_x3_impl) -----------------------------------------------------------
// rows per wave from the same rounds model as launch_roll: 256 * occ workgroups at a time (occ 5 / 3 with cout <= 8, 3 / 2
// otherwise, for 1 / 2 rows per wave), a workgroup costs (rows per wave + 2); measured 16->8 into 48x148x200: 57 -> 43 us
// (the batched unaligned-row instantiation with cout <= 8 holds 4 workgroups per CU, not 5: 88 registers against 80)
static inline EffiForm effi_pick_deconv_x3(int cout, int h, int w, int D, long n_smp, const EffiFormOpts& o) {
    const int tiles_x = effi_cdiv(w, 16);
    const bool al = (w & 3) == 0, half = cout <= 8;
    const int occ1 = half ? ((n_smp > 1 && !al) ? 4 : 5) : 3, occ2 = half ? 3 : 2;
    const long wg1 = (long)tiles_x * effi_cdiv(h, 4) * D * n_smp, wg2 = (long)tiles_x * effi_cdiv(h, 8) * D * n_smp;   // (all samples)
    bool mr2 = effi_cdiv(wg2, 256L * occ2) * 4 < effi_cdiv(wg1, 256L * occ1) * 3;
    if (o.deconv_mr != EFFI_OPT_UNSET) mr2 = o.deconv_mr == 2;
    return EffiForm{mr2 ? 2 : 1, 16, 4, 1, 0};
}

// ---- vector-ALU 3-D kernels (conv3d.hip) ------------------------------------------------------------------------------------------
// 1 -> 8 and 8 -> 1 channels: 8 planes per thread when the grid still covers the chip twice (h, w: the OUTPUT map; ncall: the two
// calls of a pair or the samples of a batch)
static inline EffiForm effi_pick_c3_planes(int h, int w, int D, long ncall) {
    const long tiles = (long)effi_cdiv(w, EFFI_C3_TX) * effi_cdiv(h, EFFI_C3_TY);
    return EffiForm{1, EFFI_C3_TX, 4, tiles * effi_cdiv(D, 8) * ncall >= 512 ? 8 : 4, 0};
}

// Both kernels address their input with 32-bit byte offsets: fewer than 2^29 elements in the input tensor (D x h x w: the INPUT volume)
static inline bool effi_c1to8_fits32(int D, int h, int w) { return (long)D * h * w < (1L << 29); }
static inline bool effi_c8to1_fits32(int D, int h, int w) { return 8L * D * h * w < (1L << 29); }

// General kernel, stride (sz, sxy, sxy): output planes per thread.  4 (2 with stride 2 in z and xy) amortise the z halo of the LDS
// tile; low-resolution layers fall back to 1 so that the grid still has >= 2 workgroups per CU (384 workgroups of the larger form).
// ho, wo, Do: the OUTPUT volume; cout_tiles: groups of output channels a workgroup owns; ncall: the two calls of a pair or the
// samples of a batch (an output's FMA order does not depend on the planes per thread, so the rule counts all their workgroups).
constexpr int effi_c3_zbig(int sz, int sxy) { return (sxy == 1 || sz == 1) ? 4 : 2; }
static inline int effi_pick_c3_zpt(int sz, int sxy, int ho, int wo, int Do, int cout_tiles, long ncall) {
    const int zbig = effi_c3_zbig(sz, sxy);
    const long blocks = (long)effi_cdiv(wo, EFFI_C3_TX) * effi_cdiv(ho, EFFI_C3_TY) * effi_cdiv(Do, zbig) * cout_tiles * ncall;
    return blocks >= 384 ? zbig : 1;
}
// its id in effi_launch_form (beside EFFI_LF_* of include/effi_mvs_hip.h, which stays as it is): nt = cout_tiles, h, w, planes = the
// output volume, count = ncall, EFFI_LF_FLAG_S2 = stride (2, 2, 2); form.planes = the planes per thread
constexpr int EFFI_LF_C3_ZPT = 12;

// transposed convolution, stride 2, cout % 8 == 0: 8 output channels per thread, 4 on the low-resolution level (the output channels
// split finer so that the grid covers the chip)
static inline EffiForm effi_pick_deconv_k3(int cout, int h, int w, int D, long n_smp) {
    const int tiles = effi_cdiv(w, EFFI_C3_TX) * effi_cdiv(h, EFFI_C3_TY);
    return EffiForm{1, EFFI_C3_TX, 4, (long)tiles * D * (cout / 8) * n_smp >= 512 ? 8 : 4, 0};
}

// ---- warp and correlation kernels (warpcorr.hip) ------------------------------------------------------------------------------------
struct EffiWarpOpts {           // the options the two rules below read, as set (EFFI_OPT_UNSET = the rule)
    long warp_lds_kb, dyn_form, dyn_setup_exact, dyn_win;
};
static inline EffiWarpOpts effi_warp_opts() {
    return EffiWarpOpts{effi_option(EFFI_OPT_WARP_LDS_KB), effi_option(EFFI_OPT_DYN_FORM), effi_option(EFFI_OPT_DYN_SETUP_EXACT),
                        effi_option(EFFI_OPT_DYN_WIN)};
}

// Window capacity of the stage-1 LDS kernels in pixels (128 B each): 72 KB leaves room for two 512-thread workgroups per CU.
constexpr int EFFI_WIN_MAXPX = 576;

// Option warp_lds_kb (effi_set_option; tests and A/B runs only): unset = the windowed kernel with its full 72 KB window;
// 0 = the windowed kernel with every chunk sampled from global memory (same arithmetic, the bitwise cross-check);
// -1 = the direct-gather kernel (also what C != 32 and per-pixel hypotheses use).
static inline int effi_warp_lds_px(const EffiWarpOpts& o) {
    if (o.warp_lds_kb == EFFI_OPT_UNSET) return EFFI_WIN_MAXPX;
    if (o.warp_lds_kb < 0) return -1;
    const long px = o.warp_lds_kb * 1024 / 128;
    return px < EFFI_WIN_MAXPX ? (int)px : EFFI_WIN_MAXPX;
}

enum EffiViewsKernel { EFFI_VIEWS_GATHER, EFFI_VIEWS_WINDOW, EFFI_VIEWS_MM };
struct EffiViewsForm {
    EffiViewsKernel kernel;
    int lds_px;                 // window kernels: pixels of the LDS window (0 = every chunk from global memory)
};
// Stage 1 (the views family, forward and backward; x3: the split-precision forward entries).  Hypotheses shared by all pixels
// (C = 32, no per-pixel depth stride, D <= 256 -- the cascade's stage 1) serve their taps from an LDS window, and the
// split-precision entries run them on the matrix cores (coordinates below 32000; option warp_lds_kb does not reach that kernel);
// everything else takes the direct-gather kernels, which exist for C = 32 / 16 / 8.
static inline EffiViewsForm effi_pick_views(bool x3, int C, long dps, int D, int h, int w, const EffiWarpOpts& o) {
    const bool shared = C == 32 && dps == 0 && D <= 256;
    if (x3 && shared && h < 32000 && w < 32000) return EffiViewsForm{EFFI_VIEWS_MM, 0};
    const int lds_px = effi_warp_lds_px(o);
    if (shared && lds_px >= 0) return EffiViewsForm{EFFI_VIEWS_WINDOW, lds_px};
    return EffiViewsForm{EFFI_VIEWS_GATHER, 0};
}

enum EffiDynKernel { EFFI_DYN_EXACT, EFFI_DYN_SPLIT, EFFI_DYN_HYP, EFFI_DYN_WINDOW };
struct EffiDynForm {
    EffiDynKernel kernel;
    int lds_px;                 // window kernel: at most this many pixels per window (0 = every view from global memory)
};
// The dynamic stage (stages 2 / 3), forward.
// EXACT: the channel-split kernel with the reference's IEEE divisions op for op -- option dyn_setup_exact = 1 (A/B runs, tests), or a
//   map too large for the 32-bit byte offsets of every other form.
// SPLIT: the channel-split (exchange-free) kernel with the "fast" set-up arithmetic (see the kernel) -- C = 32, or option dyn_form = 1.
// HYP: the hypothesis-per-lane kernel, the default for C = 8 / 16 (91 vs 107 us at 592x800, 60 vs 75 us at 296x400 against SPLIT).
// WINDOW: its LDS-window form (warpcorr_dyn_win_kernel), D <= 8 (a lane holds the set-ups of its 4 / 2 hypotheses for two views)
//   and coordinates below 32000; option dyn_win: -1 = HYP instead, 0 = the window kernel with every view sampled from global memory,
//   n > 0 = windows of at most n pixels (tests: most boxes then overflow and mix with LDS-served views).
// (An 8-channels-per-lane form -- one lane per pixel at C = 8, no exchange, no reduction, cheaper projection -- was built and
// measured at 592x800: 121 us against 109 us; at 296x400, C = 16: 63 against 58.  These kernels are bound by the number of distinct
// cache lines a wave-instruction touches in the L1 / texture path, not by instruction issue.)
static inline EffiDynForm effi_pick_dyn(int C, int S, int D, int h, int w, const EffiWarpOpts& o) {
    if (o.dyn_setup_exact == 1 || (long)h * w * C * 4 >= (1L << 31)) return EffiDynForm{EFFI_DYN_EXACT, 0};
    if (o.dyn_form == 1 || (C != 8 && C != 16)) return EffiDynForm{EFFI_DYN_SPLIT, 0};
    if (o.dyn_win == -1 || D > 8 || S > EFFI_MAX_VIEWS || h >= 32000 || w >= 32000) return EffiDynForm{EFFI_DYN_HYP, 0};
    return EffiDynForm{EFFI_DYN_WINDOW, o.dyn_win == EFFI_OPT_UNSET ? (1 << 20) : (int)(o.dyn_win > 0 ? o.dyn_win : 0)};
}
