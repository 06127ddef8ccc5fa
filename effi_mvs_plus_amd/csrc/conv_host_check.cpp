// Stand-alone host check of the convolution entries of csrc/conv2d.hip and csrc/conv2d_sr.hip (with conv2d_x3.hpp and
// gru_fused.hpp): make -C effi_mvs_plus_amd/csrc host-check.  Every extern "C" entry is called over a table of cases that reaches
// each branch of its host code (N-tile counts, rows per wave, wide tiles, eight waves, unaligned rows, batches, pairs, refusals),
// and every launch is RECORDED instead of made: kernel instantiation, grid, block and each by-value argument, field by field.  The
// records are compared with tests/golden/conv_launch_records.txt (tests/test_conv_host_check.py), which pins what the GPU tests
// cannot see: every tile form of a layer is bitwise equal by design, so a wrong instantiation or grid passes them.
// NOTHING here reaches a GPU, with or without one in the machine: the two .hip files are included with hipLaunchKernelGGL redefined
// to the recorder and the error queries answering hipSuccess, and the program is compiled for the host only (-DEFFI_BF16_ONLY for the
// second precision), under -fsanitize=address,undefined and -ftrivial-auto-var-init=pattern: an argument field that an entry leaves
// unset prints as 0xAA.. and not, by luck, as zero.  The made-up device addresses are copied into the arguments and never read
// through.  Referring to the kernels makes the host object want the device image's symbol; the Makefile links with
// --unresolved-symbols=ignore-all, and nothing registers or launches a kernel.
#include "host_check_record.hpp"           // the recorder: the launch macro is redefined from here on
#include "conv2d.hip"
#include "conv2d_sr.hip"

namespace {                                 // (beside the structs: the recorder's show finds these by argument-dependent lookup)
void show_one(const Conv2dArgs& a) {
    for (int i = 0; i < EFFI_MAX_SRC; ++i) ptr(L("src%d", i).c_str(), a.src[i]);
    for (int i = 0; i < EFFI_MAX_SRC; ++i) if (a.ch[i]) put(" ch%d=%d", i, a.ch[i]);
    FI(a, cin), FI(a, kgroups), FP(a, wpack), FP(a, bias), FI(a, cout), FI(a, h), FI(a, w), FI(a, act), FI(a, hd), FP(a, aux0), FP(a, aux1);
    FP(a, disp_range), FI(a, n_range), FP(a, out0), FP(a, out1), FI(a, cstride), FI(a, ostride), FI(a, zcount), FI(a, zin), FI(a, hin);
    FI(a, win), FP(a, zeros), FP(a, xptr0), FI(a, sr_hp), FI(a, sr_wp), FP(a, out_sr), FI(a, aux_q4);
}
void show_one(const ConvBatch& b) {
    FI(b, n_img);
    for (int i = 0; i < EFFI_MAX_SRC; ++i) if (b.src[i]) put(" src%d=%ld", i, b.src[i]);
    FI(b, aux0), FI(b, out0);
}
void show_one(const EncGenArgs& g) {
    FP(g, inv_depth), FP(g, disp_range), FI(g, n_range), FP(g, interval), FP(g, cur_vol), FI(g, cds), FI(g, cps), FI(g, Dcur), FP(g, reg_vol);
    FI(g, rds), FI(g, rps), FI(g, Dreg), FP(g, dmin), FP(g, dmax), FI(g, range_ps), FP(g, w_c1), FP(g, b_c1), FP(g, w_d1), FP(g, b_d1), FI(g, hd);
    FI(g, off32);
}
void show_one(const DeconvArgs& a) {
    FP(a, in), FP(a, wpack), FP(a, bias), FP(a, skip), FP(a, zeros), FP(a, out), FI(a, cin), FI(a, cout), FI(a, D), FI(a, h), FI(a, w), FI(a, relu);
}
void show_one(const ConvTwiceArgs& a) {
    FP(a, src), FI(a, cin), FP(a, w_a), FP(a, bias_a), FP(a, w_b), FP(a, bias_b), FI(a, cout), FI(a, h), FI(a, w), FP(a, out), FP(a, zeros);
}
void show_one(const EncTailArgs& a) {
    FP(a, src_a), FP(a, src_b), FP(a, w_a), FP(a, bias_a), FP(a, w_b), FP(a, bias_b), FP(a, w_d), FP(a, bias_d), FP(a, extra), FI(a, c_extra);
    FP(a, w2), FP(a, bias2), FI(a, cout2), FI(a, h), FI(a, w), FP(a, out), FP(a, zeros);
}
void show_one(const CspGenCall& c) { FP(c, prior), FP(c, w0), FP(c, b0), FP(c, wc), FP(c, bc), FP(c, w1), FP(c, b1), FP(c, out); }
void show_one(const GruFusedArgs& g) {
    FP(g, H_in), FP(g, X), FP(g, h_in), FP(g, wzr), FP(g, bzr), FP(g, wq), FP(g, bq), FP(g, h_out), FP(g, H_out), FI(g, h), FI(g, w), FI(g, hp);
    FI(g, wp);
}
}  // namespace

#define XSTR2(x) #x
#define XSTR(x) XSTR2(x)
// RUN: an entry compiled in both precisions (EFFI_FN appends _bf16 in the second); the recorder's RUNF: an fp32-only entry
#define RUN(fn, label, ...) do { g_rec.clear(); const int rc_ = EFFI_FN(fn)(__VA_ARGS__); emit(XSTR(EFFI_FN(fn)), (label), rc_); } while (0)
// the one behaviour this layer changed: rows per wave outside a launcher's set are refused by every launcher (not in the golden)
#define EXPECT_BADARG(fn, ...)                                                                                          \
    do {                                                                                                                \
        g_rec.clear();                                                                                                  \
        const int rc_ = EFFI_FN(fn)(__VA_ARGS__);                                                                       \
        if (rc_ != EFFI_ERR_BADARG || !g_rec.empty()) { std::printf("FAILED line %d: %s -> %s\n", __LINE__, #fn, rc_name(rc_)); ++g_failures; } \
    } while (0)

static const float* const S[3] = {P(1), P(2), P(3)};           // sources
static const float* const S2[3] = {P(4), P(5), P(6)};
static const void* const V[3] = {P(1), P(2), P(3)};            // split-resident sources
static const void* const V2[3] = {P(4), P(5), P(6)};
static float* const W = P(10);                                  // weights / bias / outputs / auxiliaries
static float* const B = P(11);
static float* const O0 = P(12);
static float* const O1 = P(13);
static float* const A0 = P(14);
static float* const A1 = P(15);
static float* const DR = P(16);
static float* const W2 = P(17);
static float* const B2 = P(18);
static float* const X = P(19);
static const long ST[3] = {1000, 0, 3000};                      // image strides: one shared tensor (stride 0)
static const int C16[3] = {16, 16, 16}, C8[3] = {8, 8, 8};
static int hp_of(int h) { return ((h + 15) & ~15) + 2; }
static int wp_of(int w) { return (w >= 512 ? ((w + 63) & ~63) : ((w + 15) & ~15)) + 2; }

struct HW { int h, w; };

#ifndef EFFI_BF16_ONLY
static void cases_fp32() {
    // ---- z-batched fp32 3-D forms: rows 1 / 2 / 4 by (D, h, w), unaligned rows, both N-tile counts, sample batches
    const struct { int D, h, w; } vols[] = {{2, 16, 16}, {16, 64, 64}, {32, 64, 64}, {3, 30, 34}, {32, 128, 128}};
    for (auto v : vols)
        for (int cout : {16, 32}) {
            if (cout == 32 && v.D != 2) continue;
            RUNF(effi_conv3d_k3s1_mfma_f32, L("D%d %dx%d cout%d", v.D, v.h, v.w, cout), S[0], 8, W, B, cout, v.D, v.h, v.w, 1, O0, nullptr);
            RUNF(effi_conv3d_k3s2_mfma_f32, L("D%d %dx%d cout%d", v.D, v.h, v.w, cout), S[0], 8, W, B, cout, v.D, v.h, v.w, 0, O0, nullptr);
        }
    for (int n : {1, 2, 3}) {
        RUNF(effi_conv3d_k3s1_mfma_f32_batch, L("n_smp%d", n), S[0], 8, W, B, 16, 16, 64, 64, 1, O0, n, 0L, 5000L, nullptr);
        RUNF(effi_conv3d_k3s2_mfma_f32_batch, L("n_smp%d", n), S[0], 8, W, B, 32, 16, 64, 64, 1, O0, n, 4000L, 5000L, nullptr);
    }
    RUNF(effi_conv3d_k3s1_mfma_f32, "cout48", S[0], 8, W, B, 48, 2, 16, 16, 1, O0, nullptr);
    RUNF(effi_conv3d_k3s1_mfma_f32, "null in", nullptr, 8, W, B, 16, 2, 16, 16, 1, O0, nullptr);
    RUNF(effi_conv3d_k3s1_mfma_f32_batch, "n_smp0", S[0], 8, W, B, 16, 2, 16, 16, 1, O0, 0, 0L, 0L, nullptr);
    RUNF(effi_conv3d_k3s1_mfma_f32_batch, "stride<0", S[0], 8, W, B, 16, 2, 16, 16, 1, O0, 2, -1L, 0L, nullptr);
    RUNF(effi_conv3d_k3s2_mfma_f32, "cout48", S[0], 8, W, B, 48, 2, 16, 16, 1, O0, nullptr);
    RUNF(effi_conv3d_k3s2_mfma_f32_batch, "n_smp65536", S[0], 8, W, B, 16, 2, 16, 16, 1, O0, 65536, 0L, 0L, nullptr);

    // ---- generic fp32 convolution
    auto c2d = [&](const std::string& label, int n_src, int cout, int ks, int h, int w, int epi, int act, int n_img = 0, const float* aux0 = A0,
                   const float* aux1 = A1, float* out1 = O1, int n_range = 4) {
        if (n_img == 0)
            RUNF(effi_conv2d_f32, label, S, C8, n_src, W, B, cout, ks, h, w, epi, act, aux0, aux1, DR, n_range, O0, out1, nullptr);
        else
            RUNF(effi_conv2d_f32_batch, label + L(" n_img%d", n_img), S, C8, n_src, W, B, cout, ks, h, w, epi, act, aux0, aux1, DR, n_range, O0,
                 out1, n_img, ST, 7000L, 8000L, nullptr);
    };
    const HW maps[] = {{16, 16}, {128, 512}, {256, 512}, {16, 18}};      // rows 1 (k1: 2) / 2 (k1: 4) / 4 / the 16 x 16 kernel
    for (int n_img : {1, 3}) c2d("plain k3 cout16 16x16", 2, 16, 3, 16, 16, EFFI_EPI_PLAIN, EFFI_ACT_RELU, n_img);
    for (int n_img : {0, 2})
        for (int ks : {1, 3})
            for (int cout : {16, 32, 48, 64, 96, 80}) {
                c2d(L("plain k%d cout%d 16x16", ks, cout), 2, cout, ks, 16, 16, EFFI_EPI_PLAIN, EFFI_ACT_RELU, n_img);
                if (n_img || cout == 16) c2d(L("nhwc k%d cout%d 16x16", ks, cout), 1, cout, ks, 16, 16, EFFI_EPI_NHWC, EFFI_ACT_NONE, n_img);
            }
    for (int n_img : {0, 2})
        for (int ks : {1, 3})
            for (HW m : maps) {
                c2d(L("plain k%d cout24 %dx%d", ks, m.h, m.w), 3, 24, ks, m.h, m.w, EFFI_EPI_PLAIN, EFFI_ACT_TANH, n_img);
                if (m.h != 128 && (!n_img || m.w == 18)) c2d(L("nhwc k%d cout24 %dx%d", ks, m.h, m.w), 3, 24, ks, m.h, m.w, EFFI_EPI_NHWC, EFFI_ACT_NONE, n_img);
                if (ks == 1 && m.h != 128 && (!n_img || m.h == 256)) c2d(L("add_up2 k1 cout32 %dx%d", m.h, m.w), 1, 32, 1, m.h, m.w, EFFI_EPI_ADD_UP2, EFFI_ACT_NONE, n_img);
            }
    for (int n_img : {0, 2}) {
        for (int cout : {32, 64, 128, 192, 256, 16})
            if (!n_img || cout == 32) c2d(L("gru_zr cout%d", cout), 2, cout, 3, 16, 16, EFFI_EPI_GRU_ZR, EFFI_ACT_NONE, n_img);
        for (int cout : {16, 32, 48, 64, 8})
            if (!n_img || cout == 32) c2d(L("gru_q cout%d", cout), 2, cout, 3, 16, 16, EFFI_EPI_GRU_Q, EFFI_ACT_NONE, n_img);
        for (HW m : {HW{16, 16}, HW{512, 512}, HW{512, 516}, HW{16, 18}}) {
            c2d(L("head %dx%d", m.h, m.w), 2, 1, 3, m.h, m.w, EFFI_EPI_HEAD, EFFI_ACT_NONE, n_img);
            c2d(L("plain cout1 %dx%d", m.h, m.w), 2, 1, 3, m.h, m.w, EFFI_EPI_PLAIN, EFFI_ACT_SIGMOID, n_img);
        }
        c2d("gru_zr no aux0", 1, 32, 3, 16, 16, EFFI_EPI_GRU_ZR, 0, n_img, nullptr);
        c2d("add_up2 k3", 1, 16, 3, 16, 16, EFFI_EPI_ADD_UP2, 0, n_img);
        c2d("plain act9", 1, 16, 3, 16, 16, EFFI_EPI_PLAIN, 9, n_img);
        c2d("epilogue 99", 1, 16, 3, 16, 16, 99, 0, n_img);
        if (n_img) continue;                   // the refusals below sit in front of anything a batch changes
        c2d("head cout2", 1, 2, 3, 16, 16, EFFI_EPI_HEAD, 0, n_img);
        c2d("head n_range1", 1, 1, 3, 16, 16, EFFI_EPI_HEAD, 0, n_img, A0, A1, O1, 1);
        c2d("head large n_range1", 1, 1, 3, 512, 512, EFFI_EPI_HEAD, 0, n_img, A0, A1, O1, 1);
        c2d("head large no out1", 1, 1, 3, 512, 512, EFFI_EPI_HEAD, 0, n_img, A0, A1, nullptr);
        c2d("gru_zr no out1", 1, 32, 3, 16, 16, EFFI_EPI_GRU_ZR, 0, n_img, A0, A1, nullptr);
        c2d("gru_zr k1", 1, 32, 1, 16, 16, EFFI_EPI_GRU_ZR, 0, n_img);
        c2d("gru_q no aux1", 1, 16, 3, 16, 16, EFFI_EPI_GRU_Q, 0, n_img, A0, nullptr);
        c2d("add_up2 no aux0", 1, 16, 1, 16, 16, EFFI_EPI_ADD_UP2, 0, n_img, nullptr);
        c2d("add_up2 odd h", 1, 16, 1, 15, 16, EFFI_EPI_ADD_UP2, 0, n_img);
        c2d("nhwc act-1", 1, 16, 3, 16, 16, EFFI_EPI_NHWC, -1, n_img);
        c2d("k5", 1, 16, 5, 16, 16, EFFI_EPI_PLAIN, 0, n_img);
        c2d("cout0", 1, 0, 3, 16, 16, EFFI_EPI_PLAIN, 0, n_img);
        c2d("n_src0", 0, 16, 3, 16, 16, EFFI_EPI_PLAIN, 0, n_img);
        c2d("n_src4", EFFI_MAX_SRC + 1, 16, 3, 16, 16, EFFI_EPI_PLAIN, 0, n_img);
    }
    {
        const float* bad[3] = {P(1), nullptr, P(3)};
        const int ch0[3] = {8, 0, 8};
        RUNF(effi_conv2d_f32, "null src1", bad, C8, 2, W, B, 16, 3, 16, 16, EFFI_EPI_PLAIN, 0, A0, A1, DR, 4, O0, O1, nullptr);
        RUNF(effi_conv2d_f32, "ch1 = 0", S, ch0, 2, W, B, 16, 3, 16, 16, EFFI_EPI_PLAIN, 0, A0, A1, DR, 4, O0, O1, nullptr);
        RUNF(effi_conv2d_f32, "null srcs", nullptr, C8, 2, W, B, 16, 3, 16, 16, EFFI_EPI_PLAIN, 0, A0, A1, DR, 4, O0, O1, nullptr);
        const long neg[3] = {0, -8, 0};
        RUNF(effi_conv2d_f32_batch, "stride1<0", S, C8, 2, W, B, 16, 3, 16, 16, EFFI_EPI_PLAIN, 0, A0, A1, DR, 4, O0, O1, 2, neg, 0L, 0L, nullptr);
        RUNF(effi_conv2d_f32_batch, "stride1<0 past n_src", S, C8, 1, W, B, 16, 3, 16, 16, EFFI_EPI_PLAIN, 0, A0, A1, DR, 4, O0, O1, 2, neg, 0L, 0L, nullptr);
        RUNF(effi_conv2d_f32_batch, "null strides", S, C8, 1, W, B, 16, 3, 16, 16, EFFI_EPI_PLAIN, 0, A0, A1, DR, 4, O0, O1, 2, nullptr, 0L, 0L, nullptr);
        RUNF(effi_conv2d_f32_batch, "n_img0", S, C8, 1, W, B, 16, 3, 16, 16, EFFI_EPI_PLAIN, 0, A0, A1, DR, 4, O0, O1, 0, ST, 0L, 0L, nullptr);
        RUNF(effi_conv2d_f32_batch, "aux0 stride<0", S, C8, 1, W, B, 16, 3, 16, 16, EFFI_EPI_PLAIN, 0, A0, A1, DR, 4, O0, O1, 2, ST, -1L, 0L, nullptr);
    }

    // ---- 5x5 stride 2, fp32
    for (int n_img : {0, 1, 2, 3})
        for (HW m : {HW{32, 32}, HW{512, 512}, HW{30, 30}, HW{32, 36}})
            for (int cout : {16, 32, 64, 48}) {
                if (((n_img & 1) || m.w != 32) && cout != 16) continue;
                if (n_img == 0) RUNF(effi_conv2d_k5s2_f32, L("%dx%d cout%d", m.h, m.w, cout), S[0], 3, W, B, cout, m.h, m.w, EFFI_ACT_RELU, O0, nullptr);
                else RUNF(effi_conv2d_k5s2_f32_batch, L("%dx%d cout%d n_img%d", m.h, m.w, cout, n_img), S[0], 3, W, B, cout, m.h, m.w, EFFI_ACT_RELU,
                          O0, n_img, n_img == 3 ? 0L : 6000L, 7000L, nullptr);
            }
    RUNF(effi_conv2d_k5s2_f32, "act9", S[0], 3, W, B, 16, 32, 32, 9, O0, nullptr);
    RUNF(effi_conv2d_k5s2_f32, "cin0", S[0], 0, W, B, 16, 32, 32, 0, O0, nullptr);
    RUNF(effi_conv2d_k5s2_f32_batch, "n_img0", S[0], 3, W, B, 16, 32, 32, 0, O0, 0, 0L, 0L, nullptr);
    RUNF(effi_conv2d_k5s2_f32_batch, "out stride<0", S[0], 3, W, B, 16, 32, 32, 0, O0, 2, 0L, -4L, nullptr);

    for (int cout : {16, 32, 48, 8}) RUNF(effi_conv2d_c1k7_relu_f32, L("cout%d", cout), S[0], W, B, cout, 20, 40, O0, nullptr);
    RUNF(effi_conv2d_c1k7_relu_f32, "null in", nullptr, W, B, 16, 20, 40, O0, nullptr);
}
#endif

static void cases_x3() {
    // ---- stride-2 split-precision forms: 5x5 of the pyramid, 3x3x3 of the U-Net
    for (int n_img : {0, 1, 2, 3})
        for (HW m : {HW{32, 32}, HW{256, 512}, HW{30, 32}})
            for (int cout : {16, 32, 64, 128}) {
                if (((n_img & 1) || m.h == 30) && cout != 16) continue;
                if (n_img == 0) RUN(effi_conv2d_k5s2_bf16x3_f32, L("%dx%d cout%d", m.h, m.w, cout), S[0], 3, W, B, cout, m.h, m.w, EFFI_ACT_RELU, O0, nullptr);
                else RUN(effi_conv2d_k5s2_bf16x3_f32_batch, L("%dx%d cout%d n_img%d", m.h, m.w, cout, n_img), S[0], 3, W, B, cout, m.h, m.w,
                         EFFI_ACT_RELU, O0, n_img, n_img == 3 ? 0L : 6000L, 7000L, nullptr);
            }
    RUN(effi_conv2d_k5s2_bf16x3_f32, "cout129", S[0], 3, W, B, 129, 32, 32, 0, O0, nullptr);
    RUN(effi_conv2d_k5s2_bf16x3_f32, "win 34", S[0], 3, W, B, 16, 32, 34, 0, O0, nullptr);
    RUN(effi_conv2d_k5s2_bf16x3_f32, "act9", S[0], 3, W, B, 16, 32, 32, 9, O0, nullptr);
    RUN(effi_conv2d_k5s2_bf16x3_f32, "null w", S[0], 3, nullptr, B, 16, 32, 32, 0, O0, nullptr);
    RUN(effi_conv2d_k5s2_bf16x3_f32_batch, "n_img0", S[0], 3, W, B, 16, 32, 32, 0, O0, 0, 0L, 0L, nullptr);
    g_have_zero_page = false;
    RUN(effi_conv2d_k5s2_bf16x3_f32, "no zero page", S[0], 3, W, B, 16, 32, 32, 0, O0, nullptr);
    RUN(effi_conv3d_k3s2_bf16x3_f32, "no zero page", S[0], 8, W, B, 16, 4, 16, 16, 1, O0, nullptr);
    g_have_zero_page = true;
    const struct { int D, h, w; } vols[] = {{4, 16, 16}, {32, 128, 128}, {3, 30, 32}};
    for (auto v : vols)
        for (int cout : {16, 32, 64}) {
            if (cout != 16 && v.D == 3) continue;
            RUN(effi_conv3d_k3s2_bf16x3_f32, L("D%d %dx%d cout%d", v.D, v.h, v.w, cout), S[0], 8, W, B, cout, v.D, v.h, v.w, 1, O0, nullptr);
            for (int n : {1, 2, 3})
                if (n == 2 || (cout == 16 && v.D == 4)) RUN(effi_conv3d_k3s2_bf16x3_f32_batch, L("D%d %dx%d cout%d n_smp%d", v.D, v.h, v.w, cout, n), S[0], 8, W, B, cout, v.D, v.h, v.w, 0, O0,
                    n, n == 3 ? 0L : 4000L, 5000L, nullptr);
        }
    RUN(effi_conv3d_k3s2_bf16x3_f32, "cout65", S[0], 8, W, B, 65, 4, 16, 16, 1, O0, nullptr);
    RUN(effi_conv3d_k3s2_bf16x3_f32, "w 18", S[0], 8, W, B, 16, 4, 16, 18, 1, O0, nullptr);
    RUN(effi_conv3d_k3s2_bf16x3_f32, "D0", S[0], 8, W, B, 16, 0, 16, 16, 1, O0, nullptr);
    RUN(effi_conv3d_k3s2_bf16x3_f32_batch, "planes > 65535", S[0], 8, W, B, 16, 3, 16, 16, 1, O0, 40000, 1L, 1L, nullptr);
    RUN(effi_conv3d_k3s2_bf16x3_f32_batch, "n_smp0", S[0], 8, W, B, 16, 3, 16, 16, 1, O0, 0, 1L, 1L, nullptr);

    // ---- split-precision 3x3: rows 1 / 2 / 4 by map size (nt 2: 2 rows from 1024 tiles), wide tiles from 512 columns
    auto c3 = [&](const std::string& label, int n_src, int cout, int h, int w, int epi, int act, int n_img = 0, const float* aux0 = A0,
                  const float* aux1 = A1, float* out1 = O1) {
        if (n_img == 0) RUN(effi_conv2d_k3_bf16x3_f32, label, S, C8, n_src, W, B, cout, h, w, epi, act, aux0, aux1, DR, 4, O0, out1, nullptr);
        else RUN(effi_conv2d_k3_bf16x3_f32_batch, label + L(" n_img%d", n_img), S, C8, n_src, W, B, cout, h, w, epi, act, aux0, aux1, DR, 4, O0, out1,
                 n_img, ST, 7000L, 8000L, nullptr);
    };
    const HW maps[] = {{16, 16}, {74, 100}, {160, 320}, {320, 320}, {512, 512}, {200, 528}};
    for (int n_img : {1, 3}) c3("plain cout16 16x16", 2, 16, 16, 16, EFFI_EPI_PLAIN, EFFI_ACT_RELU, n_img);
    for (int n_img : {0, 2}) {
        for (int cout : {16, 32, 48, 64, 96, 80}) {
            c3(L("plain cout%d 16x16", cout), 2, cout, 16, 16, EFFI_EPI_PLAIN, EFFI_ACT_RELU, n_img);
            if (n_img || cout == 16) c3(L("nhwc cout%d 16x16", cout), 1, cout, 16, 16, EFFI_EPI_NHWC, EFFI_ACT_NONE, n_img);
        }
        for (int cout : {8, 32, 48}) {
            if (cout != 48) c3(L("add_shuf2 cout%d", cout), 1, cout, 16, 16, EFFI_EPI_ADD_SHUF2, EFFI_ACT_NONE, n_img);
            c3(L("nhwc_add_shuf2 cout%d", cout), 1, cout, 16, 16, EFFI_EPI_NHWC_ADD_SHUF2, EFFI_ACT_NONE, n_img);
        }
    }
    for (int n_img : {0, 2})
        for (HW m : maps)
            for (int cout : {16, 32}) {
                if (cout == 32 && (m.h < 320 || m.h == 200)) continue;
                c3(L("plain cout%d %dx%d", cout, m.h, m.w), 3, cout, m.h, m.w, EFFI_EPI_PLAIN, EFFI_ACT_TANH, n_img);
                if (cout == 16 && m.h >= 320) c3(L("nhwc_add_shuf2 cout%d %dx%d", cout, m.h, m.w), 3, cout, m.h, m.w, EFFI_EPI_NHWC_ADD_SHUF2, EFFI_ACT_NONE, n_img);
            }
    for (int mr : {1, 2, 4})
        for (int wide : {-1, 0, 1})
            for (int n_img : {0, 2}) {
                if (wide != 1 && n_img) continue;
                Opt o(EFFI_OPT_FORCE_MR, mr), o2(EFFI_OPT_WIDE_TILES, wide == -1 ? EFFI_OPT_UNSET : wide);
                c3(L("force_mr%d wide_tiles%d plain cout48 74x100", mr, wide), 2, 48, 74, 100, EFFI_EPI_PLAIN, EFFI_ACT_RELU, n_img);
            }
    for (int n_img : {0, 2}) {
        for (int cout : {32, 64, 128, 192, 256, 16})
            if (!n_img || cout == 32) c3(L("gru_zr cout%d", cout), 2, cout, 16, 16, EFFI_EPI_GRU_ZR, EFFI_ACT_NONE, n_img);
        for (int cout : {16, 32, 48, 64, 8})
            if (!n_img || cout == 32) c3(L("gru_q cout%d", cout), 2, cout, 16, 16, EFFI_EPI_GRU_Q, EFFI_ACT_NONE, n_img);
        c3("gru_zr 74x100", 2, 64, 74, 100, EFFI_EPI_GRU_ZR, 0, n_img);
        c3("head", 1, 1, 16, 16, EFFI_EPI_HEAD, 0, n_img);
        c3("plain act9", 1, 16, 16, 16, EFFI_EPI_PLAIN, 9, n_img);
        c3("add_shuf2 relu", 1, 16, 16, 16, EFFI_EPI_ADD_SHUF2, EFFI_ACT_RELU, n_img);
        c3("w 18", 1, 16, 16, 18, EFFI_EPI_PLAIN, 0, n_img);
        if (n_img) continue;                   // the refusals below sit in front of anything a batch changes
        c3("gru_zr no aux0", 1, 32, 16, 16, EFFI_EPI_GRU_ZR, 0, n_img, nullptr);
        c3("gru_zr no out1", 1, 32, 16, 16, EFFI_EPI_GRU_ZR, 0, n_img, A0, A1, nullptr);
        c3("gru_q no aux1", 1, 16, 16, 16, EFFI_EPI_GRU_Q, 0, n_img, A0, nullptr);
        c3("add_up2", 1, 16, 16, 16, EFFI_EPI_ADD_UP2, 0, n_img);
        c3("epilogue 99", 1, 16, 16, 16, 99, 0, n_img);
        c3("nhwc act-1", 1, 16, 16, 16, EFFI_EPI_NHWC, -1, n_img);
        c3("add_shuf2 no aux0", 1, 16, 16, 16, EFFI_EPI_ADD_SHUF2, 0, n_img, nullptr);
        c3("nhwc_add_shuf2 odd h", 1, 16, 15, 16, EFFI_EPI_NHWC_ADD_SHUF2, 0, n_img);
        c3("cout0", 1, 0, 16, 16, EFFI_EPI_PLAIN, 0, n_img);
        c3("n_src0", 0, 16, 16, 16, EFFI_EPI_PLAIN, 0, n_img);
        c3("n_src4", EFFI_MAX_SRC + 1, 16, 16, 16, EFFI_EPI_PLAIN, 0, n_img);
    }
    const float* bad[3] = {P(1), nullptr, P(3)};
    const int ch0[3] = {8, 0, 8}, ch4[3] = {8, 4, 8};
    {
        RUN(effi_conv2d_k3_bf16x3_f32, "null src1", bad, C8, 2, W, B, 16, 16, 16, EFFI_EPI_PLAIN, 0, A0, A1, DR, 4, O0, O1, nullptr);
        RUN(effi_conv2d_k3_bf16x3_f32, "ch1 = 0", S, ch0, 2, W, B, 16, 16, 16, EFFI_EPI_PLAIN, 0, A0, A1, DR, 4, O0, O1, nullptr);
        RUN(effi_conv2d_k3_bf16x3_f32, "ch1 = 4 of 3", S, ch4, 3, W, B, 16, 16, 16, EFFI_EPI_PLAIN, 0, A0, A1, DR, 4, O0, O1, nullptr);
        RUN(effi_conv2d_k3_bf16x3_f32, "ch1 = 4 last", S, ch4, 2, W, B, 16, 16, 16, EFFI_EPI_PLAIN, 0, A0, A1, DR, 4, O0, O1, nullptr);
        RUN(effi_conv2d_k3_bf16x3_f32, "null bias", S, C8, 2, W, nullptr, 16, 16, 16, EFFI_EPI_PLAIN, 0, A0, A1, DR, 4, O0, O1, nullptr);
        g_have_zero_page = false;
        RUN(effi_conv2d_k3_bf16x3_f32, "no zero page", S, C8, 2, W, B, 16, 16, 16, EFFI_EPI_PLAIN, 0, A0, A1, DR, 4, O0, O1, nullptr);
        g_have_zero_page = true;
        const long neg[3] = {0, -8, 0};
        RUN(effi_conv2d_k3_bf16x3_f32_batch, "stride1<0", S, C8, 2, W, B, 16, 16, 16, EFFI_EPI_PLAIN, 0, A0, A1, DR, 4, O0, O1, 2, neg, 0L, 0L, nullptr);
        RUN(effi_conv2d_k3_bf16x3_f32_batch, "n_img0", S, C8, 2, W, B, 16, 16, 16, EFFI_EPI_PLAIN, 0, A0, A1, DR, 4, O0, O1, 0, ST, 0L, 0L, nullptr);
        RUN(effi_conv2d_k3_bf16x3_f32_batch, "n_src0", S, C8, 0, W, B, 16, 16, 16, EFFI_EPI_PLAIN, 0, A0, A1, DR, 4, O0, O1, 2, ST, 0L, 0L, nullptr);
    }

    // ---- the planar pair
    for (HW m : {HW{16, 16}, HW{148, 200}, HW{296, 400}, HW{112, 528}})
        for (int cout : {16, 32, 48, 64, 80})
            if (m.h == 16 || cout == 16 || cout == 32) RUN(effi_conv2d_k3_bf16x3_pair_f32, L("%dx%d cout%d", m.h, m.w, cout), S, C8, 2, W, B, O0, S2, C16, 1, W2, B2, O1, cout, m.h, m.w,
                EFFI_ACT_RELU, nullptr);
    for (int mr : {1, 2, 4}) {
        Opt o(EFFI_OPT_FORCE_MR, mr);
        RUN(effi_conv2d_k3_bf16x3_pair_f32, L("force_mr%d", mr), S, C8, 2, W, B, O0, S2, C16, 1, W2, B2, O1, 16, 74, 100, EFFI_ACT_RELU, nullptr);
    }
    RUN(effi_conv2d_k3_bf16x3_pair_f32, "act9", S, C8, 2, W, B, O0, S2, C16, 1, W2, B2, O1, 16, 16, 16, 9, nullptr);
    RUN(effi_conv2d_k3_bf16x3_pair_f32, "w 18", S, C8, 2, W, B, O0, S2, C16, 1, W2, B2, O1, 16, 16, 18, 0, nullptr);
    RUN(effi_conv2d_k3_bf16x3_pair_f32, "null out_b", S, C8, 2, W, B, O0, S2, C16, 1, W2, B2, nullptr, 16, 16, 16, 0, nullptr);
    RUN(effi_conv2d_k3_bf16x3_pair_f32, "a: ch1 = 4 of 3", S, ch4, 3, W, B, O0, S2, C16, 1, W2, B2, O1, 16, 16, 16, 0, nullptr);
    RUN(effi_conv2d_k3_bf16x3_pair_f32, "b: null src1", S, C8, 2, W, B, O0, bad, C16, 2, W2, B2, O1, 16, 16, 16, 0, nullptr);

    // ---- 3x3 + fused 1x1
    for (int cout1 : {16, 32, 48, 64, 96, 80, 97})
        for (int c_extra : {0, 8})
            if (c_extra || cout1 == 32) RUN(effi_conv2d_k3_k1_bf16x3_f32, L("cout1 %d c_extra%d", cout1, c_extra), S, C8, 2, W, B, cout1, c_extra ? 1 : 0, X, c_extra, W2, B2, 24, 1,
                74, 100, O0, nullptr);
    RUN(effi_conv2d_k3_k1_bf16x3_f32, "200x528", S, C8, 2, W, B, 32, 1, X, 8, W2, B2, 24, 0, 200, 528, O0, nullptr);
    RUN(effi_conv2d_k3_k1_bf16x3_f32, "no extra", S, C8, 2, W, B, 32, 1, nullptr, 8, W2, B2, 24, 0, 16, 16, O0, nullptr);
    RUN(effi_conv2d_k3_k1_bf16x3_f32, "c_extra 17", S, C8, 2, W, B, 32, 1, X, 17, W2, B2, 24, 0, 16, 16, O0, nullptr);
    RUN(effi_conv2d_k3_k1_bf16x3_f32, "cout2 97", S, C8, 2, W, B, 32, 1, X, 8, W2, B2, 97, 0, 16, 16, O0, nullptr);
    RUN(effi_conv2d_k3_k1_bf16x3_f32, "w 18", S, C8, 2, W, B, 32, 1, X, 8, W2, B2, 24, 0, 16, 18, O0, nullptr);
    RUN(effi_conv2d_k3_k1_bf16x3_f32, "null w2", S, C8, 2, W, B, 32, 1, X, 8, nullptr, B2, 24, 0, 16, 16, O0, nullptr);
    RUN(effi_conv2d_k3_k1_bf16x3_f32, "ch0 = 4 of 2", S, ch4 + 1, 2, W, B, 32, 1, X, 8, W2, B2, 24, 0, 16, 16, O0, nullptr);
    for (int cout1 : {16, 32, 64, 96, 48, 97})
        RUN(effi_conv2d_k3_k1_up2x_bf16x3_f32, L("cout1 %d", cout1), S, C8, 2, W, B, cout1, W2, B2, A0, DR, 5, 74, 100, O0, O1, nullptr);
    RUN(effi_conv2d_k3_k1_up2x_bf16x3_f32, "n_range1", S, C8, 2, W, B, 32, W2, B2, A0, DR, 1, 16, 16, O0, O1, nullptr);
    RUN(effi_conv2d_k3_k1_up2x_bf16x3_f32, "no out_depth_inv", S, C8, 2, W, B, 32, W2, B2, A0, DR, 5, 16, 16, O0, nullptr, nullptr);
    RUN(effi_conv2d_k3_k1_up2x_bf16x3_f32, "w 18", S, C8, 2, W, B, 32, W2, B2, A0, DR, 5, 16, 18, O0, O1, nullptr);
    RUN(effi_conv2d_k3_k1_up2x_bf16x3_f32, "ch0 = 4 of 2", S, ch4 + 1, 2, W, B, 32, W2, B2, A0, DR, 5, 16, 16, O0, O1, nullptr);

    // ---- the pyramid's first block, the encoder tail
    for (HW m : {HW{16, 16}, HW{600, 800}}) {
        RUN(effi_conv2d_k3_twice_bf16x3_f32, L("%dx%d", m.h, m.w), S[0], 3, W, B, W2, B2, 8, m.h, m.w, O0, nullptr);
        for (int n : {1, 2, 3}) RUN(effi_conv2d_k3_twice_bf16x3_f32_batch, L("%dx%d n_img%d", m.h, m.w, n), S[0], 3, W, B, W2, B2, 8, m.h, m.w, O0, n,
                                    n == 3 ? 0L : 9000L, 9500L, nullptr);
    }
    RUN(effi_conv2d_k3_twice_bf16x3_f32, "cin9", S[0], 9, W, B, W2, B2, 8, 16, 16, O0, nullptr);
    RUN(effi_conv2d_k3_twice_bf16x3_f32, "w 18", S[0], 3, W, B, W2, B2, 8, 16, 18, O0, nullptr);
    RUN(effi_conv2d_k3_twice_bf16x3_f32, "null bias2", S[0], 3, W, B, W2, nullptr, 8, 16, 16, O0, nullptr);
    RUN(effi_conv2d_k3_twice_bf16x3_f32_batch, "n_img0", S[0], 3, W, B, W2, B2, 8, 16, 16, O0, 0, 0L, 0L, nullptr);
    RUN(effi_conv2d_k3_twice_bf16x3_f32_batch, "stride<0", S[0], 3, W, B, W2, B2, 8, 16, 16, O0, 2, -1L, 0L, nullptr);
    RUN(effi_conv2d_k3_twice_bf16x3_f32_batch, "stride<0 n_img1", S[0], 3, W, B, W2, B2, 8, 16, 16, O0, 1, -1L, 0L, nullptr);
    for (int c_extra : {0, 8})
        RUN(effi_encoder_tail_bf16x3_f32, L("c_extra%d", c_extra), S[0], S[1], 16, W, B, W2, B2, P(20), P(21), 15, X, c_extra, P(22), P(23), 24, 74, 100,
            O0, nullptr);
    RUN(effi_encoder_tail_bf16x3_f32, "hd32", S[0], S[1], 32, W, B, W2, B2, P(20), P(21), 15, X, 8, P(22), P(23), 24, 74, 100, O0, nullptr);
    RUN(effi_encoder_tail_bf16x3_f32, "null dfm1", S[0], nullptr, 16, W, B, W2, B2, P(20), P(21), 15, X, 8, P(22), P(23), 24, 74, 100, O0, nullptr);
    RUN(effi_encoder_tail_bf16x3_f32, "cmix0", S[0], S[1], 16, W, B, W2, B2, P(20), P(21), 0, X, 8, P(22), P(23), 24, 74, 100, O0, nullptr);

    // ---- z-batched split-precision 3-D form: any w; rows by the planes of all samples
    const long SS[3] = {4000, 0, 0};
    const struct { int D, h, w; } v1[] = {{2, 16, 16}, {16, 64, 64}, {32, 64, 64}, {2, 16, 18}};
    for (auto v : v1)
        for (int cout : {16, 32, 48})
            if (cout == 16 || v.h == 16)
            for (int n_src : {1, 2}) {
                if (n_src == 2 && v.D != 2) continue;
                RUN(effi_conv3d_k3s1_bf16x3_f32, L("D%d %dx%d cout%d n_src%d", v.D, v.h, v.w, cout, n_src), S, C8, n_src, W, B, cout, v.D, v.h, v.w, 1, O0,
                    nullptr);
                for (int n : {1, 2, 3})
                    if (n == 2 || (cout == 16 && v.D == 2)) RUN(effi_conv3d_k3s1_bf16x3_f32_batch, L("D%d %dx%d cout%d n_src%d n_smp%d", v.D, v.h, v.w, cout, n_src, n), S, C8, n_src, W, B, cout,
                        v.D, v.h, v.w, 0, O0, n, SS, 5000L, nullptr);
            }
    for (int mr : {1, 2, 4}) {
        Opt o(EFFI_OPT_FORCE_MR, mr);
        RUN(effi_conv3d_k3s1_bf16x3_f32, L("force_mr%d", mr), S, C8, 1, W, B, 16, 4, 30, 34, 1, O0, nullptr);
        RUN(effi_conv3d_k3s1_bf16x3_f32_batch, L("force_mr%d n_smp2", mr), S, C8, 1, W, B, 16, 4, 30, 34, 1, O0, 2, SS, 5000L, nullptr);
    }
    RUN(effi_conv3d_k3s1_bf16x3_f32, "cin 12", S, ch4, 2, W, B, 16, 2, 16, 16, 1, O0, nullptr);
    RUN(effi_conv3d_k3s1_bf16x3_f32, "ch0 = 4 of 2", S, ch4 + 1, 2, W, B, 16, 2, 16, 16, 1, O0, nullptr);
    RUN(effi_conv3d_k3s1_bf16x3_f32, "cin 4", S, ch4 + 1, 1, W, B, 16, 2, 16, 16, 1, O0, nullptr);
    RUN(effi_conv3d_k3s1_bf16x3_f32, "D0", S, C8, 1, W, B, 16, 0, 16, 16, 1, O0, nullptr);
    RUN(effi_conv3d_k3s1_bf16x3_f32, "null out", S, C8, 1, W, B, 16, 2, 16, 16, 1, nullptr, nullptr);
    RUN(effi_conv3d_k3s1_bf16x3_f32_batch, "n_src0", S, C8, 0, W, B, 16, 2, 16, 16, 1, O0, 2, SS, 0L, nullptr);
    RUN(effi_conv3d_k3s1_bf16x3_f32_batch, "n_smp0", S, C8, 1, W, B, 16, 2, 16, 16, 1, O0, 0, SS, 0L, nullptr);

    // ---- rolling-window 3-D convolution
    auto roll = [&](const std::string& label, const int* ch, int n_src, int cout, int D, int h, int w, bool all = true) {
        RUN(effi_conv3d_k3s1_roll_bf16x3_f32, label, S, ch, n_src, W, B, cout, D, h, w, 1, O0, nullptr);
        if (!all) return;                      // (a refusal of the shared filler: the single entry shows it)
        for (int n : {1, 2, 3})
            if (n == 2 || (cout == 16 && n_src == 2)) RUN(effi_conv3d_k3s1_roll_bf16x3_f32_batch, label + L(" n_smp%d", n), S, ch, n_src, W, B, cout, D, h, w, 1, O0, n, SS, 5000L, nullptr);
        RUN(effi_conv3d_k3s1_roll_bf16x3_pair_f32, label, S, W, B, O0, S2, W2, B2, O1, ch, n_src, cout, D, h, w, 1, nullptr);
    };
    for (int cout : {8, 16, 32, 33}) {
        roll(L("cin8 cout%d", cout), C8, 1, cout, 8, 32, 32);
        if (cout != 33) roll(L("cin16 cout%d", cout), C16, 1, cout, 8, 32, 32);
        if (cout == 16) roll(L("cin8+8 cout%d", cout), C8, 2, cout, 8, 32, 32);
    }
    roll("128x160 D48", C8, 1, 8, 48, 128, 160);
    roll("296x400 D8", C8, 2, 16, 8, 296, 400);
    for (int mr : {2, 4})
        for (int zt : {1, 3}) {
            if (mr == 4 && zt == 1) continue;
            Opt o(EFFI_OPT_ROLL_MR, mr), o2(EFFI_OPT_ROLL_ZT, zt);
            roll(L("roll_mr%d roll_zt%d cout8", mr, zt), C8, 1, 8, 8, 32, 32);
            Opt o3(EFFI_OPT_ROLL_RP, 0);
            roll(L("roll_mr%d roll_zt%d roll_rp0 cout8", mr, zt), C8, 1, 8, 8, 32, 32);
        }
    // option roll_slide = 0 (not in the golden): the three-slot kernels under their own names, and nothing else of a record changes
    for (int cin : {8, 16})
        for (int entry = 0; entry < 3; ++entry) {
            std::string rec[2];
            for (int slide = 1; slide >= 0; --slide) {
                Opt o(EFFI_OPT_ROLL_SLIDE, slide ? EFFI_OPT_UNSET : 0);
                const int* ch = cin == 8 ? C8 : C16;
                g_rec.clear();
                const int rc = entry == 0   ? EFFI_FN(effi_conv3d_k3s1_roll_bf16x3_f32)(S, ch, 1, W, B, 8, 8, 32, 32, 1, O0, nullptr)
                               : entry == 1 ? EFFI_FN(effi_conv3d_k3s1_roll_bf16x3_f32_batch)(S, ch, 1, W, B, 8, 8, 32, 32, 1, O0, 2, SS, 5000L, nullptr)
                                            : EFFI_FN(effi_conv3d_k3s1_roll_bf16x3_pair_f32)(S, W, B, O0, S2, W2, B2, O1, ch, 1, 8, 8, 32, 32, 1, nullptr);
                rec[slide] = rc == EFFI_OK ? g_rec : std::string("?");
            }
            const size_t at = rec[0].find("conv3d_roll_rp3_bf16x3_");
            if (at == std::string::npos || rec[1].find("conv3d_roll_rp_bf16x3_") != at || std::string(rec[0]).erase(at + 14, 1) != rec[1]) {
                std::printf("FAILED: roll_slide=0, cin %d, entry %d:%s\n   against%s\n", cin, entry, rec[0].c_str(), rec[1].c_str());
                ++g_failures;
            }
        }
    roll("n_src3", C8, 3, 8, 8, 32, 32);
    roll("cin 4", ch4 + 1, 1, 8, 8, 32, 32, false);
    roll("w 18", C8, 1, 8, 8, 32, 18, false);
    RUN(effi_conv3d_k3s1_roll_bf16x3_f32, "null src1", bad, C8, 2, W, B, 8, 8, 32, 32, 1, O0, nullptr);
    RUN(effi_conv3d_k3s1_roll_bf16x3_pair_f32, "b: null src", S, W, B, O0, bad + 1, W2, B2, O1, C8, 1, 8, 8, 32, 32, 1, nullptr);
    RUN(effi_conv3d_k3s1_roll_bf16x3_f32_batch, "n_smp0", S, C8, 1, W, B, 8, 8, 32, 32, 1, O0, 0, SS, 0L, nullptr);
    g_have_zero_page = false;
    RUN(effi_conv3d_k3s1_roll_bf16x3_f32, "no zero page", S, C8, 1, W, B, 8, 8, 32, 32, 1, O0, nullptr);
    RUN(effi_conv3d_k3s1_bf16x3_f32, "no zero page", S, C8, 1, W, B, 16, 2, 16, 16, 1, O0, nullptr);
    g_have_zero_page = true;

    RUN(effi_csp_gen_roll_bf16x3_pair_f32, "D8 64x80", X, 8, 64, 80, P(30), P(31), P(32), P(33), P(34), P(35), P(36), O0, P(40), P(41), P(42), P(43),
        P(44), P(45), P(46), O1, nullptr);
    RUN(effi_csp_gen_roll_bf16x3_pair_f32, "D15", X, 15, 64, 80, P(30), P(31), P(32), P(33), P(34), P(35), P(36), O0, P(40), P(41), P(42), P(43), P(44),
        P(45), P(46), O1, nullptr);
    RUN(effi_csp_gen_roll_bf16x3_pair_f32, "null prior_b", X, 8, 64, 80, P(30), P(31), P(32), P(33), P(34), P(35), P(36), O0, nullptr, P(41), P(42), P(43),
        P(44), P(45), P(46), O1, nullptr);

    // ---- transposed 3-D convolution
    for (int n : {0, 1, 2, 3})
        for (int cin : {16, 32})
            for (int cout : {8, 16})
                for (HW m : {HW{16, 18}, HW{74, 100}})
                    for (int dmr : {0, 1, 2}) {
                        if (((dmr || cin == 32) && (cout != 8 || m.h != 74)) || ((n & 1) && (cin != 16 || cout != 8 || m.h != 74))) continue;
                        Opt o(EFFI_OPT_DECONV_MR, dmr ? dmr : EFFI_OPT_UNSET);
                        const std::string label = L("cin%d cout%d %dx%d deconv_mr%d", cin, cout, m.h, m.w, dmr);
                        if (n == 0) RUN(effi_deconv3d_k3s2_bf16x3_f32, label, S[0], cin, W, B, cout, 8, m.h, m.w, 1, X, O0, nullptr);
                        else RUN(effi_deconv3d_k3s2_bf16x3_f32_batch, label + L(" n_smp%d", n), S[0], cin, W, B, cout, 8, m.h, m.w, 1, n == 2 ? nullptr : X, O0,
                                 n, 4000L, n == 3 ? 0L : 4500L, 5000L, nullptr);
                    }
    RUN(effi_deconv3d_k3s2_bf16x3_f32, "cin8", S[0], 8, W, B, 8, 8, 16, 16, 1, X, O0, nullptr);
    RUN(effi_deconv3d_k3s2_bf16x3_f32, "cin24", S[0], 24, W, B, 8, 8, 16, 16, 1, X, O0, nullptr);
    RUN(effi_deconv3d_k3s2_bf16x3_f32, "cout17", S[0], 16, W, B, 17, 8, 16, 16, 1, X, O0, nullptr);
    RUN(effi_deconv3d_k3s2_bf16x3_f32, "null in", nullptr, 16, W, B, 8, 8, 16, 16, 1, X, O0, nullptr);
    RUN(effi_deconv3d_k3s2_bf16x3_f32_batch, "n_smp0", S[0], 16, W, B, 8, 8, 16, 16, 1, X, O0, 0, 0L, 0L, 0L, nullptr);
    RUN(effi_deconv3d_k3s2_bf16x3_f32_batch, "skip stride<0", S[0], 16, W, B, 8, 8, 16, 16, 1, X, O0, 2, 0L, -1L, 0L, nullptr);
    g_have_zero_page = false;
    RUN(effi_deconv3d_k3s2_bf16x3_f32, "no zero page", S[0], 16, W, B, 8, 8, 16, 16, 1, X, O0, nullptr);
    g_have_zero_page = true;
}

static void cases_sr() {
    void* const OS = P<void>(50);
    void* const OS2 = P<void>(51);
    const int C32[3] = {32, 32, 32}, c24[3] = {16, 24, 16};
    auto sr = [&](const std::string& label, int n_src, int cout, int h, int w, int epi, int act, const float* aux0 = A0, const float* aux1 = A1,
                  float* out0 = O0, void* out_sr = P<void>(50), int dhp = 0) {
        RUN(effi_conv2d_k3_bf16x3_sr, label, V, C16, n_src, W, B, cout, h, w, hp_of(h) + dhp, wp_of(w), epi, act, aux0, aux1, out0, out_sr, nullptr);
    };
    const HW maps[] = {{16, 16}, {74, 100}, {160, 320}, {320, 320}, {512, 512}, {200, 528}};
    for (HW m : maps) {
        for (int cout : {16, 32, 48, 64, 96, 80})
            if (m.h == 16 || cout == 32 || cout == 96) sr(L("plain cout%d %dx%d", cout, m.h, m.w), 2, cout, m.h, m.w, EFFI_EPI_PLAIN, EFFI_ACT_RELU);
        if (m.h != 74) continue;
        for (int q4 : {0, EFFI_EPI_Q4}) {
            for (int cout : {32, 64, 96, 128, 48})
                if (!q4 || cout == 96) sr(L("gru_zr%s cout%d %dx%d", q4 ? " q4" : "", cout, m.h, m.w), 2, cout, m.h, m.w, EFFI_EPI_GRU_ZR | q4, 0);
            for (int cout : {16, 32, 48, 64})
                if (!q4 || cout == 32) sr(L("gru_q%s cout%d %dx%d", q4 ? " q4" : "", cout, m.h, m.w), 3, cout, m.h, m.w, EFFI_EPI_GRU_Q | q4, 0);
        }
    }
    for (long waves : {4, 8})
        for (int mr : {0, 1, 2, 4}) {
            Opt o(EFFI_OPT_SR_WAVES, waves), o2(EFFI_OPT_FORCE_MR, mr ? mr : EFFI_OPT_UNSET);
            sr(L("sr_waves%ld force_mr%d plain cout96", waves, mr), 2, 96, 74, 100, EFFI_EPI_PLAIN, EFFI_ACT_RELU);
        }
    for (int wide : {0, 1})
        for (int mr : {1, 2, 4}) {
            Opt o(EFFI_OPT_WIDE_TILES, wide), o2(EFFI_OPT_FORCE_MR, mr);
            RUN(effi_conv2d_k3_bf16x3_sr, L("wide_tiles%d force_mr%d", wide, mr), V, C16, 2, W, B, 32, 74, 100, hp_of(74), wp_of(512), EFFI_EPI_PLAIN, 0, A0, A1,
                O0, OS, nullptr);
        }
    {
        Opt o(EFFI_OPT_WIDE_TILES, 1);
        sr("wide_tiles1 narrow wp", 2, 32, 74, 100, EFFI_EPI_PLAIN, 0);
    }
    sr("plain no out0", 2, 32, 16, 16, EFFI_EPI_PLAIN, 0, A0, A1, nullptr);
    sr("plain act9", 2, 32, 16, 16, EFFI_EPI_PLAIN, 9);
    sr("plain q4", 2, 32, 16, 16, EFFI_EPI_PLAIN | EFFI_EPI_Q4, 0);
    sr("gru_zr q4 aux0 + 4", 2, 32, 16, 16, EFFI_EPI_GRU_ZR | EFFI_EPI_Q4, 0, A0 + 1);
    sr("gru_zr no aux0", 2, 32, 16, 16, EFFI_EPI_GRU_ZR, 0, nullptr);
    sr("gru_zr no out0", 2, 32, 16, 16, EFFI_EPI_GRU_ZR, 0, A0, A1, nullptr);
    sr("gru_q no aux1", 2, 32, 16, 16, EFFI_EPI_GRU_Q, 0, A0, nullptr);
    sr("nhwc", 2, 32, 16, 16, EFFI_EPI_NHWC, 0);
    sr("cout 24", 2, 24, 16, 16, EFFI_EPI_PLAIN, 0);
    sr("no out_sr", 2, 32, 16, 16, EFFI_EPI_PLAIN, 0, A0, A1, O0, nullptr);
    sr("out_sr + 8", 2, 32, 16, 16, EFFI_EPI_PLAIN, 0, A0, A1, O0, P<char>(50) + 8);
    sr("hp too small", 2, 32, 16, 16, EFFI_EPI_PLAIN, 0, A0, A1, O0, OS, -1);
    sr("n_src0", 0, 32, 16, 16, EFFI_EPI_PLAIN, 0);
    sr("cout0", 2, 0, 16, 16, EFFI_EPI_PLAIN, 0);
    RUN(effi_conv2d_k3_bf16x3_sr, "wp too small", V, C16, 2, W, B, 32, 16, 16, hp_of(16), wp_of(16) - 1, EFFI_EPI_PLAIN, 0, A0, A1, O0, OS, nullptr);
    RUN(effi_conv2d_k3_bf16x3_sr, "ch1 = 24", V, c24, 2, W, B, 32, 16, 16, hp_of(16), wp_of(16), EFFI_EPI_PLAIN, 0, A0, A1, O0, OS, nullptr);
    RUN(effi_conv2d_k3_bf16x3_sr, "plane of 2^29 units", V, C16, 2, W, B, 32, 16, 16, 23171, 23171, EFFI_EPI_PLAIN, 0, A0, A1, O0, OS, nullptr);
    RUN(effi_conv2d_k3_bf16x3_sr, "cout x plane of 2^31", V, C16, 2, W, B, 96, 16, 16, 4800, 4800, EFFI_EPI_PLAIN, 0, A0, A1, O0, OS, nullptr);
    {
        const void* odd[3] = {P<char>(1) + 8, P(2), P(3)};
        const void* nul[3] = {P(1), nullptr, P(3)};
        RUN(effi_conv2d_k3_bf16x3_sr, "src0 + 8", odd, C16, 2, W, B, 32, 16, 16, hp_of(16), wp_of(16), EFFI_EPI_PLAIN, 0, A0, A1, O0, OS, nullptr);
        RUN(effi_conv2d_k3_bf16x3_sr, "null src1", nul, C16, 2, W, B, 32, 16, 16, hp_of(16), wp_of(16), EFFI_EPI_PLAIN, 0, A0, A1, O0, OS, nullptr);
    }

    for (HW m : {HW{16, 16}, HW{148, 200}, HW{296, 400}, HW{112, 528}})
        for (int cout : {16, 32, 48, 64, 80, 24})
            if (m.h == 16 || cout == 32) RUN(effi_conv2d_k3_bf16x3_pair_sr, L("%dx%d cout%d", m.h, m.w, cout), V, C16, 2, W, B, OS, V2, C32, 1, W2, B2, OS2, cout, m.h, m.w, hp_of(m.h),
                wp_of(m.w), EFFI_ACT_RELU, nullptr);
    for (long waves : {4, 8})
        for (int mr : {1, 2, 4}) {
            Opt o(EFFI_OPT_SR_WAVES, waves), o2(EFFI_OPT_FORCE_MR, mr);
            RUN(effi_conv2d_k3_bf16x3_pair_sr, L("sr_waves%ld force_mr%d", waves, mr), V, C16, 2, W, B, OS, V2, C32, 1, W2, B2, OS2, 32, 74, 100, hp_of(74),
                wp_of(100), EFFI_ACT_RELU, nullptr);
        }
    RUN(effi_conv2d_k3_bf16x3_pair_sr, "act9", V, C16, 2, W, B, OS, V2, C32, 1, W2, B2, OS2, 32, 16, 16, hp_of(16), wp_of(16), 9, nullptr);
    RUN(effi_conv2d_k3_bf16x3_pair_sr, "no out_sr_b", V, C16, 2, W, B, OS, V2, C32, 1, W2, B2, nullptr, 32, 16, 16, hp_of(16), wp_of(16), 0, nullptr);
    RUN(effi_conv2d_k3_bf16x3_pair_sr, "out_sr_a + 8", V, C16, 2, W, B, P<char>(50) + 8, V2, C32, 1, W2, B2, OS2, 32, 16, 16, hp_of(16), wp_of(16), 0, nullptr);
    RUN(effi_conv2d_k3_bf16x3_pair_sr, "b: ch0 = 24", V, C16, 2, W, B, OS, V2, c24 + 1, 1, W2, B2, OS2, 32, 16, 16, hp_of(16), wp_of(16), 0, nullptr);

    auto gen = [&](const std::string& label, int hd, int cout, int h, int w, int nq = 3, int act = EFFI_ACT_RELU, int Dcur = 8) {
        RUN(effi_encoder_pair_gen_bf16x3_sr, label, A0, DR, 5, P(60), P(61), 100000L, 1L, Dcur, P(62), 200000L, 2L, 12, P(63), P(64), 0L, nq, h, w, P(65),
            P(66), P(67), P(68), hd, W, B, OS, W2, B2, OS2, cout, hp_of(h), wp_of(w), act, nullptr);
    };
    for (HW m : {HW{16, 16}, HW{148, 200}, HW{296, 400}})
        for (int hd : {16, 32, 48})
            for (int cout : {16, 32, 48, 64})
                if (m.h == 16 ? (hd == 16 || cout == 16) : (hd == 16 && cout == 16)) gen(L("%dx%d hd%d cout%d", m.h, m.w, hd, cout), hd, cout, m.h, m.w);
    {
        Opt o(EFFI_OPT_ENC_GEN_MR3, 0);
        gen("enc_gen_mr3 = 0 296x400", 16, 16, 296, 400);
    }
    for (int mr : {1, 2, 4}) {
        Opt o(EFFI_OPT_FORCE_MR, mr);
        gen(L("force_mr%d", mr), 16, 16, 74, 100);
    }
    gen("hd24", 24, 16, 16, 16);
    gen("nq4", 16, 16, 16, 16, 4);
    gen("act9", 16, 16, 16, 16, 3, 9);
    gen("Dcur1", 16, 16, 16, 16, 3, 0, 1);
    gen("cout24", 16, 24, 16, 16);

    for (int cout1 : {16, 32, 48, 64, 96, 80, 97})
        for (int to_sr : {0, 1})
            if (!to_sr || cout1 == 32) RUN(effi_conv2d_k3_k1_bf16x3_sr, L("cout1 %d %s", cout1, to_sr ? "out_sr" : "out"), V, C16, 2, W, B, cout1, 1, X, to_sr ? 0 : 8, W2, B2, 32, to_sr, 74,
                100, hp_of(74), wp_of(100), to_sr ? nullptr : O0, to_sr ? OS : nullptr, nullptr);
    RUN(effi_conv2d_k3_k1_bf16x3_sr, "200x528", V, C16, 2, W, B, 32, 0, X, 8, W2, B2, 32, 0, 200, 528, hp_of(200), wp_of(528), O0, nullptr, nullptr);
    RUN(effi_conv2d_k3_k1_bf16x3_sr, "both outputs", V, C16, 2, W, B, 32, 0, X, 8, W2, B2, 32, 0, 16, 16, hp_of(16), wp_of(16), O0, OS, nullptr);
    RUN(effi_conv2d_k3_k1_bf16x3_sr, "no output", V, C16, 2, W, B, 32, 0, X, 8, W2, B2, 32, 0, 16, 16, hp_of(16), wp_of(16), nullptr, nullptr, nullptr);
    RUN(effi_conv2d_k3_k1_bf16x3_sr, "out_sr cout2 24", V, C16, 2, W, B, 32, 0, X, 8, W2, B2, 24, 0, 16, 16, hp_of(16), wp_of(16), nullptr, OS, nullptr);
    RUN(effi_conv2d_k3_k1_bf16x3_sr, "c_extra 17", V, C16, 2, W, B, 32, 0, X, 17, W2, B2, 32, 0, 16, 16, hp_of(16), wp_of(16), O0, nullptr, nullptr);
    RUN(effi_conv2d_k3_k1_bf16x3_sr, "no extra", V, C16, 2, W, B, 32, 0, nullptr, 8, W2, B2, 32, 0, 16, 16, hp_of(16), wp_of(16), O0, nullptr, nullptr);
    RUN(effi_conv2d_k3_k1_bf16x3_sr, "hp too small", V, C16, 2, W, B, 32, 0, X, 8, W2, B2, 32, 0, 16, 16, hp_of(16) - 1, wp_of(16), O0, nullptr, nullptr);

    for (int tile : {2, 4, 8, 3})
        for (int cout1 : {16, 32, 48, 49})
            if (tile == 4 || cout1 == 16) RUN(effi_depth_head_bf16x3_sr, L("tile%d cout1 %d", tile, cout1), V, C16, 1, W, B, cout1, W2, P(70), B2, A0, DR, 5, 74, 100, hp_of(74), wp_of(100),
                tile, O0, O1, nullptr);
    RUN(effi_depth_head_bf16x3_sr, "n_range1", V, C16, 1, W, B, 16, W2, P(70), B2, A0, DR, 1, 74, 100, hp_of(74), wp_of(100), 4, O0, O1, nullptr);
    RUN(effi_depth_head_bf16x3_sr, "no out_depth", V, C16, 1, W, B, 16, W2, P(70), B2, A0, DR, 5, 74, 100, hp_of(74), wp_of(100), 4, O0, nullptr, nullptr);
    RUN(effi_depth_head_bf16x3_sr, "n_src0", V, C16, 0, W, B, 16, W2, P(70), B2, A0, DR, 5, 74, 100, hp_of(74), wp_of(100), 4, O0, O1, nullptr);

    for (HW m : {HW{74, 100}, HW{320, 320}})
        for (int cout1 : {32, 64, 96, 16, 97})
            if (m.h == 74 || cout1 == 32)
            RUN(effi_conv2d_k3_k1_up2x_bf16x3_sr, L("%dx%d cout1 %d", m.h, m.w, cout1), V, C16, 2, W, B, cout1, W2, B2, A0, DR, 5, m.h, m.w, hp_of(m.h),
                wp_of(m.w), O0, O1, nullptr);
    RUN(effi_conv2d_k3_k1_up2x_bf16x3_sr, "n_range1", V, C16, 2, W, B, 32, W2, B2, A0, DR, 1, 16, 16, hp_of(16), wp_of(16), O0, O1, nullptr);
    RUN(effi_conv2d_k3_k1_up2x_bf16x3_sr, "no out_depth_inv", V, C16, 2, W, B, 32, W2, B2, A0, DR, 5, 16, 16, hp_of(16), wp_of(16), O0, nullptr, nullptr);
    RUN(effi_conv2d_k3_k1_up2x_bf16x3_sr, "ch1 = 24", V, c24, 2, W, B, 32, W2, B2, A0, DR, 5, 16, 16, hp_of(16), wp_of(16), O0, O1, nullptr);

    for (int hd : {16, 32, 48})
        RUN(effi_gru_zr_q_fused_bf16x3_sr, L("hd%d", hd), V[0], V[1], A0, W, B, W2, B2, hd, 74, 100, 76, 102, O0, OS, nullptr);
    RUN(effi_gru_zr_q_fused_bf16x3_sr, "H_out = X", V[0], V[1], A0, W, B, W2, B2, 16, 74, 100, 76, 102, O0, const_cast<void*>(V[1]), nullptr);
    RUN(effi_gru_zr_q_fused_bf16x3_sr, "hp too small", V[0], V[1], A0, W, B, W2, B2, 16, 74, 100, 75, 102, O0, OS, nullptr);
    RUN(effi_gru_zr_q_fused_bf16x3_sr, "null h_in", V[0], V[1], nullptr, W, B, W2, B2, 16, 74, 100, 76, 102, O0, OS, nullptr);
}

// rows per wave outside {1, 2, 4}: every launcher of the split 3x3 family refuses them (single, batched, z-batched, pairs)
static void cases_rows_refused() {
    Opt o(EFFI_OPT_FORCE_MR, 3);
    void* const OS = P<void>(50);
    void* const OS2 = P<void>(51);
    const long SS[3] = {4000, 0, 0};
    const int C32[3] = {32, 32, 32};
    for (int wide : {0, 1}) {
        Opt o2(EFFI_OPT_WIDE_TILES, wide);
        EXPECT_BADARG(effi_conv2d_k3_bf16x3_f32, S, C8, 2, W, B, 16, 16, 16, EFFI_EPI_PLAIN, 0, A0, A1, DR, 4, O0, O1, nullptr);
        EXPECT_BADARG(effi_conv2d_k3_bf16x3_f32_batch, S, C8, 2, W, B, 16, 16, 16, EFFI_EPI_PLAIN, 0, A0, A1, DR, 4, O0, O1, 2, ST, 0L, 0L, nullptr);
        EXPECT_BADARG(effi_conv2d_k3_bf16x3_sr, V, C16, 2, W, B, 32, 16, 16, hp_of(16), wp_of(512), EFFI_EPI_PLAIN, 0, A0, A1, O0, OS, nullptr);
    }
    EXPECT_BADARG(effi_conv2d_k3_bf16x3_pair_f32, S, C8, 2, W, B, O0, S2, C16, 1, W2, B2, O1, 16, 16, 16, 0, nullptr);
    EXPECT_BADARG(effi_conv2d_k3_bf16x3_pair_sr, V, C16, 2, W, B, OS, V2, C32, 1, W2, B2, OS2, 32, 16, 16, hp_of(16), wp_of(16), 0, nullptr);
    EXPECT_BADARG(effi_conv2d_k3_k1_bf16x3_f32, S, C8, 2, W, B, 32, 1, X, 8, W2, B2, 24, 0, 16, 16, O0, nullptr);
    EXPECT_BADARG(effi_conv3d_k3s1_bf16x3_f32, S, C8, 1, W, B, 16, 2, 16, 16, 1, O0, nullptr);
    EXPECT_BADARG(effi_conv3d_k3s1_bf16x3_f32_batch, S, C8, 1, W, B, 16, 2, 16, 16, 1, O0, 2, SS, 0L, nullptr);
    {
        Opt r(EFFI_OPT_ROLL_MR, 3);             // the rolling window: 2 or 4
        EXPECT_BADARG(effi_conv3d_k3s1_roll_bf16x3_f32, S, C8, 1, W, B, 8, 8, 32, 32, 1, O0, nullptr);
        EXPECT_BADARG(effi_conv3d_k3s1_roll_bf16x3_f32_batch, S, C8, 1, W, B, 16, 8, 32, 32, 1, O0, 2, SS, 0L, nullptr);
    }
    Opt o3(EFFI_OPT_SR_WAVES, 8);
    EXPECT_BADARG(effi_conv2d_k3_bf16x3_pair_sr, V, C16, 2, W, B, OS, V2, C32, 1, W2, B2, OS2, 32, 16, 16, hp_of(16), wp_of(16), 0, nullptr);
}

int main() {
    for (long& v : g_opt) v = EFFI_OPT_UNSET;
#ifndef EFFI_BF16_ONLY
    cases_fp32();
#endif
    std::printf("# split-precision entries: the records of both builds (the second appends _bf16 to the entry names)\n");
    cases_x3();
    cases_sr();
    cases_rows_refused();
    if (g_failures) std::printf("conv host check: %d FAILED\n", g_failures);
    return g_failures ? 1 : 0;
}
