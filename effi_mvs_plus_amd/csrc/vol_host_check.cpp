// Stand-alone host check of the 3-D and volume entries of csrc/conv3d.hip and csrc/volume_ops.hip: make -C effi_mvs_plus_amd/csrc
// host-check.  Every extern "C" entry of the two files is called over a table of cases that reaches each branch of its host code at
// both sides of each threshold (planes per thread of the vector-ALU 3-D kernels, dense / strided weight rows, single / pair / batch
// wrappers, option c3_lean, the register and the generic soft-argmin kernel, 32-bit tap offsets of the look-up family, vector and
// scalar forms of the splitters, refusals), and every launch is RECORDED instead of made (host_check_record.hpp): kernel
// instantiation, grid, block and each by-value argument, field by field.  The records are compared with
// tests/golden/vol_launch_records.txt (tests/test_vol_host_check.py), which pins what the GPU tests cannot see: the 4- and 8-planes
// forms, the dense and strided forms and the two soft-argmin kernels are bitwise equal by design, and a sample stride in the wrong
// slot of a batch of one changes nothing.
// NOTHING here reaches a GPU: the program is compiled for the host only, under -fsanitize=address,undefined and
// -ftrivial-auto-var-init=pattern (an argument field an entry leaves unset prints as 0xAA..), and the made-up device addresses are
// copied into the arguments and never read through.
#include "host_check_record.hpp"           // the recorder: the launch macro is redefined from here on
#include "conv3d.hip"
#include "volume_ops.hip"

static void show_one(const EffiPtrList& l) {
    for (int i = 0; i <= EFFI_MAX_VIEWS; ++i) ptr(L("p%d", i).c_str(), l.p[i]);
    FP(l, tbl);
}
static void show_one(const EffiOutList& l) {
    for (int i = 0; i <= EFFI_MAX_VIEWS; ++i) ptr(L("p%d", i).c_str(), l.p[i]);
}
#define FA(s, f, n) do { for (int i_ = 0; i_ < (n); ++i_) if ((s).f[i_] != 0) put(" " #f "%d=%ld", i_, (long)(s).f[i_]); } while (0)
#define FPA(s, f, n) do { for (int i_ = 0; i_ < (n); ++i_) ptr(L(#f "%d", i_).c_str(), (s).f[i_]); } while (0)
namespace {                                 // (beside the structs: the recorder's show finds these by argument-dependent lookup)
void show_one(const SrcSet& s) { FPA(s, p, EFFI_MAX_SRC); FA(s, ch, EFFI_MAX_SRC); }
void show_one(const C3Batch& b) { FA(b, src, EFFI_MAX_SRC); FI(b, skip), FI(b, out); }
void show_one(const Conv3dCall& c) { show_one(c.src); FP(c, wgt), FP(c, bias), FP(c, skip), FP(c, out); }
void show_one(const C1Call& c) { FP(c, in), FP(c, wgt), FP(c, bias), FP(c, out); }
void show_one(const C8Call& c) { FP(c, in), FP(c, wgt), FP(c, bias), FP(c, out); }
void show_one(const Deconv3dCall& c) { FP(c, in), FP(c, wgt), FP(c, bias), FP(c, skip), FP(c, out); }
void show_one(const SoftmaxBatch& b) {
    FI(b, logits), FI(b, depth), FI(b, out_depth), FI(b, out_conf), FI(b, range), FI(b, out_dinv), FI(b, out_conf_up);
}
void show_one(const GetcostConvArgs& g) {
    FP(g, inv_depth), FP(g, disp_range), FI(g, n_range), FI(g, input_is_depth), FP(g, interval);
    FP(g, cur_vol), FI(g, cds), FI(g, cps), FI(g, Dcur), FP(g, reg_vol), FI(g, rds), FI(g, rps), FI(g, Dreg);
    FP(g, dmin), FP(g, dmax), FI(g, range_ps), FI(g, hw), FP(g, weight), FP(g, bias), FI(g, cout), FI(g, relu), FP(g, out);
    FP(g, out_sr), FP(g, out7_sr), FI(g, w), FI(g, sr_hp), FI(g, sr_wp), FI(g, off32);
}
void show_one(const SplitStages& a) {
    FPA(a, ctx, 4); FPA(a, hidden, 4); FPA(a, inp, 4); FA(a, nh, 4); FA(a, n, 4); FA(a, first, 5); FI(a, vec4);
}
void show_one(const SrMaps& a) { FPA(a, base, 4); FA(a, planes, 4); FA(a, h, 4); FA(a, w, 4); FA(a, hp, 4); FA(a, wp, 4); FA(a, first, 5); }
void show_one(const SplitStagesSr& a) {
    FPA(a, ctx, 4); FPA(a, hidden, 4); FPA(a, inp, 4); FPA(a, hidden_sr, 4);
    FA(a, hd, 4); FA(a, cd, 4); FA(a, h, 4); FA(a, w, 4); FA(a, hp, 4); FA(a, wp, 4); FA(a, q4, 4); FA(a, first, 5);
    FPA(a, clear_base, 4); FA(a, clear_planes, 4); FA(a, nsplit, 4);
}
}  // namespace

static void direct_failure(const std::string& what) {
    std::printf("FAILED: %s\n", what.c_str());
    ++g_failures;
}
template <class T> static T* off(T* p, long floats) { return reinterpret_cast<T*>(reinterpret_cast<uintptr_t>(p) + 4 * floats); }

// ---- the general 3-D convolution and its 1 -> 8 / 8 -> 1 routes --------------------------------------------------------------------
static const float* const SRCS[4] = {P(2), P(3), P(4), P(5)};
static const float* const SRCS_NULL1[3] = {P(2), nullptr, P(4)};
struct ConvArgs {
    const float* const* srcs = SRCS;
    int ch[4] = {8, 4, 3, 2};
    bool null_ch = false, null_ss = false;
    int n_src = 1;
    const float* wgt = P(10);
    const float* bias = P(11);
    int cout = 8, D = 6, h = 37, w = 50, sz = 1, sxy = 1, relu = 1;             // (h, w: no multiple of the tile)
    const float* skip = nullptr;
    float* out = P(13);
    int n_smp = 3;
    long ss[3] = {1000, 2000, 3000}, skip_ss = 4000, out_ss = 5000;
};
static std::string conv(bool batch, const std::string& label, const ConvArgs& a) {
    g_rec.clear();
    const int rc = batch ? effi_conv3d_k3_f32_batch(a.srcs, (a.null_ch ? nullptr : a.ch), a.n_src, a.wgt, a.bias, a.cout, a.D, a.h, a.w, a.sz, a.sxy, a.relu, a.skip,
                                                    a.out, a.n_smp, (a.null_ss ? nullptr : a.ss), a.skip_ss, a.out_ss, nullptr)
                         : effi_conv3d_k3_f32(a.srcs, (a.null_ch ? nullptr : a.ch), a.n_src, a.wgt, a.bias, a.cout, a.D, a.h, a.w, a.sz, a.sxy, a.relu, a.skip, a.out,
                                              nullptr);
    emit(batch ? "effi_conv3d_k3_f32_batch" : "effi_conv3d_k3_f32", batch ? label + L(" n_smp%d", a.n_smp) : label, rc);
    return g_rec;
}
static ConvArgs conv_at(int cin, int cout, int sz, int sxy, int D = 6, int h = 37, int w = 50) {
    ConvArgs a;
    a.ch[0] = cin, a.cout = cout, a.sz = sz, a.sxy = sxy, a.D = D, a.h = h, a.w = w;
    return a;
}

static void cases_conv() {
    for (int batch : {0, 1}) {
        // strides, output channels (8: dense rows; 16: strided rows of two tiles; 1: its own tile, stride 1 only; 12: refused)
        for (int s : {0, 1, 2}) {
            const int sz = s == 1 ? 2 : 1, sxy = s == 0 ? 1 : 2;
            for (int cout : {8, 16, 1, 12}) {
                Opt o(EFFI_OPT_C3_LEAN, cout == 1 ? 0 : EFFI_OPT_UNSET);          // (8 -> 1 channels on the general kernel)
                conv(batch, L("s%d%d%d cin8 cout%d", sz, sxy, sxy, cout) + (cout == 1 ? " c3_lean0" : ""), conv_at(8, cout, sz, sxy));
            }
            // planes per thread: one tile (output 7 x 29), 383 / 384 workgroups over the planes; over the samples of a batch too
            const int h = sxy == 1 ? 7 : 13, w = sxy == 1 ? 29 : 57;
            for (int D : {1532, 1533}) {
                ConvArgs a = conv_at(8, 8, sz, sxy, D, h, w);
                a.n_smp = 1;
                conv(batch, L("s%d%d%d 1 tile D%d", sz, sxy, sxy, D), a);
            }
            if (batch)
                for (int D : {508, 512}) conv(1, L("s%d%d%d 1 tile D%d", sz, sxy, sxy, D), conv_at(8, 8, sz, sxy, D, h, w));   // 127 / 128 x 3
        }
        conv(batch, "s122 cin8 cout8 sz2 sxy1: refused", conv_at(8, 8, 2, 1));
        conv(batch, "sxy3: refused", conv_at(8, 8, 1, 3));
        conv(batch, "sz0 sxy11: refused", conv_at(8, 8, 0, 11));
        conv(batch, "sz1 sxy12: refused", conv_at(8, 8, 1, 12));
        conv(batch, "sz0 sxy2: refused", conv_at(8, 8, 0, 2));
        // sources and the skip tensor
        for (int n : {1, 2, 3, 4})
            for (int skip : {0, 1}) {
                ConvArgs a;
                a.n_src = n, a.skip = skip ? P(12) : nullptr;
                conv(batch, L("n_src%d skip%d", n, skip), a);
            }
        // the 1 -> 8 and 8 -> 1 routes under option c3_lean (unset: both dedicated kernels; bit 0 / bit 1)
        for (long lean : {EFFI_OPT_UNSET, 0L, 1L, 2L, 3L}) {
            Opt o(EFFI_OPT_C3_LEAN, lean);
            const std::string l = lean == EFFI_OPT_UNSET ? std::string("c3_lean unset") : L("c3_lean%ld", lean);
            for (int sxy : {1, 2, 3}) conv(batch, l + L(" 1->8 sxy%d", sxy), conv_at(1, 8, 1, sxy));
            conv(batch, l + " 8->1", conv_at(8, 1, 1, 1));
        }
        {
            ConvArgs a = conv_at(1, 8, 1, 1);
            a.skip = P(12);
            conv(batch, "1->8 skip: general kernel", a);
            a = conv_at(8, 1, 1, 1), a.skip = P(12);
            conv(batch, "8->1 skip: general kernel", a);
            a = conv_at(5, 1, 1, 1), a.n_src = 2, a.ch[1] = 3;
            conv(batch, "8->1 of two sources: general kernel", a);
            conv(batch, "1->8 sz2: general kernel", conv_at(1, 8, 2, 2));
            conv(batch, "8->1 sxy2: refused", conv_at(8, 1, 1, 2));
        }
        // 4 / 8 planes per thread at 511 / 512 workgroups (one tile), the 2^29-element limit and one row less
        for (int sxy : {1, 2}) {
            const int h = sxy == 1 ? 7 : 13, w = sxy == 1 ? 29 : 57;
            for (int D : {4088, 4089}) {
                ConvArgs a = conv_at(1, 8, 1, sxy, D, h, w);
                a.n_smp = 1;
                conv(batch, L("1->8 sxy%d 1 tile D%d", sxy, D), a);
            }
            if (batch)
                for (int D : {584, 585}) {
                    ConvArgs a = conv_at(1, 8, 1, sxy, D, h, w);
                    a.n_smp = 7;
                    conv(1, L("1->8 sxy%d 1 tile D%d", sxy, D), a);                  // 73 x 7 = 511, 74 x 7 = 518
                }
            conv(batch, L("1->8 sxy%d 512x1024x1024: 2^29 elements", sxy), conv_at(1, 8, 1, sxy, 512, 1024, 1024));
            conv(batch, L("1->8 sxy%d 512x1023x1024", sxy), conv_at(1, 8, 1, sxy, 512, 1023, 1024));
            conv(batch, L("1->8 sxy%d 233x1103x2089: 2^29 - 1 elements", sxy), conv_at(1, 8, 1, sxy, 233, 1103, 2089));
        }
        for (int D : {4088, 4089}) {
            ConvArgs a = conv_at(8, 1, 1, 1, D, 7, 29);
            a.n_smp = 1;
            conv(batch, L("8->1 1 tile D%d", D), a);
        }
        if (batch)
            for (int D : {584, 585}) {
                ConvArgs a = conv_at(8, 1, 1, 1, D, 7, 29);
                a.n_smp = 7;
                conv(1, L("8->1 1 tile D%d", D), a);
            }
        conv(batch, "8->1 64x1024x1024: 2^29 elements", conv_at(8, 1, 1, 1, 64, 1024, 1024));
        conv(batch, "8->1 64x1023x1024", conv_at(8, 1, 1, 1, 64, 1023, 1024));
        conv(batch, "8->1 3x2731x8191: 2^29 - 8 elements, one pixel less", conv_at(8, 1, 1, 1, 3, 2731, 8191));

        // refusals
        ConvArgs a;
        a.srcs = nullptr;
        conv(batch, "null srcs", a);
        a = ConvArgs(), a.null_ch = true;
        conv(batch, "null src_channels", a);
        a = ConvArgs(), a.n_src = 3, a.srcs = SRCS_NULL1;
        conv(batch, "null srcs[1]", a);
        a.n_src = 1;
        conv(batch, "null srcs[1] past n_src", a);
        a = ConvArgs(), a.n_src = 2, a.ch[1] = 0;
        conv(batch, "src_channels[1] = 0", a);
        a = ConvArgs(), a.n_src = 0;
        conv(batch, "n_src0", a);
        a = ConvArgs(), a.wgt = nullptr;
        conv(batch, "null weight", a);
        a = ConvArgs(), a.bias = nullptr;
        conv(batch, "null bias: allowed", a);
        a = ConvArgs(), a.out = nullptr;
        conv(batch, "null out", a);
        a = ConvArgs(), a.cout = 0;
        conv(batch, "cout0", a);
        a = ConvArgs(), a.D = 0;
        conv(batch, "D0", a);
        a = ConvArgs(), a.h = 0;
        conv(batch, "h0", a);
        a = ConvArgs(), a.w = 0;
        conv(batch, "w0", a);
        if (!batch) continue;
        for (int n : {0, 65536, 65535}) {
            a = ConvArgs(), a.n_smp = n;
            conv(1, "samples", a);
        }
        a = ConvArgs(), a.null_ss = true;
        conv(1, "null src_sstride", a);
        for (int k = 0; k < 3; ++k) {
            a = ConvArgs(), a.n_src = 3, a.ss[k] = -1;
            conv(1, L("src_sstride[%d] < 0", k), a);
            a.ss[k] = 0;
            conv(1, L("src_sstride[%d] = 0", k), a);
        }
        a = ConvArgs(), a.ss[1] = -1;
        conv(1, "src_sstride[1] < 0 past n_src", a);
        a = ConvArgs(), a.skip_ss = -1;
        conv(1, "skip_sstride < 0", a);
        a = ConvArgs(), a.skip = P(12), a.skip_ss = 0;
        conv(1, "skip_sstride = 0", a);
        a = ConvArgs(), a.out_ss = -1;
        conv(1, "out_sstride < 0", a);
    }
    // one sample in the batch entry: the unbatched launch, the strides unused
    for (int route : {0, 1, 2}) {
        ConvArgs a = route == 0 ? conv_at(8, 8, 1, 1) : route == 1 ? conv_at(1, 8, 1, 2) : conv_at(8, 1, 1, 1);
        a.n_smp = 1;
        const std::string one = conv(1, L("route %d", route), a), plain = conv(0, L("route %d (again)", route), a);
        if (one != plain || one.empty()) direct_failure(L("conv3d route %d: n_smp = 1 is not the unbatched launch", route));
    }
}

struct ConvPairArgs {
    const float* in_a = P(2);
    const float* wgt_a = P(10);
    const float* bias_a = P(11);
    float* out_a = P(13);
    const float* in_b = P(3);
    const float* wgt_b = P(14);
    const float* bias_b = P(15);
    float* out_b = P(16);
    int cin = 8, cout = 8, D = 6, h = 37, w = 50, s = 1, relu = 1;              // s: sxy (convolution) / sz (transposed)
};
static void pair(bool deconv, const std::string& label, const ConvPairArgs& a) {
    if (deconv)
        RUNF(effi_deconv3d_k3_pair_f32, label, a.in_a, a.wgt_a, a.bias_a, a.out_a, a.in_b, a.wgt_b, a.bias_b, a.out_b, a.cin, a.cout, a.D, a.h,
             a.w, a.s, a.relu, nullptr);
    else
        RUNF(effi_conv3d_k3_pair_f32, label, a.in_a, a.wgt_a, a.bias_a, a.out_a, a.in_b, a.wgt_b, a.bias_b, a.out_b, a.cin, a.cout, a.D, a.h,
             a.w, a.s, a.relu, nullptr);
}
static void cases_pair() {
    for (int deconv : {0, 1}) {
        auto at = [&](int cin, int s, int D = 6, int h = 37, int w = 50) {
            ConvPairArgs a;
            a.cin = cin, a.cout = deconv ? 1 : 8, a.s = s, a.D = D, a.h = h, a.w = w;
            return a;
        };
        const int lean_cin = deconv ? 8 : 1;
        for (long lean : {EFFI_OPT_UNSET, 0L, 1L, 2L, 3L}) {
            Opt o(EFFI_OPT_C3_LEAN, lean);
            const std::string l = lean == EFFI_OPT_UNSET ? std::string("c3_lean unset") : L("c3_lean%ld", lean);
            for (int s : {1, 2, 3}) pair(deconv, l + L(" cin%d s%d", lean_cin, s), at(lean_cin, s));
        }
        for (int s : {1, 2}) pair(deconv, L("cin4 s%d", s), at(4, s));
        // the dedicated kernels: 4 / 8 planes at 510 / 512 workgroups of the two calls; their element limit
        for (int s : (deconv ? std::initializer_list<int>{1} : std::initializer_list<int>{1, 2})) {
            const int h = (!deconv && s == 2) ? 13 : 7, w = (!deconv && s == 2) ? 57 : 29;
            for (int D : {2040, 2041}) pair(deconv, L("cin%d s%d 1 tile D%d", lean_cin, s, D), at(lean_cin, s, D, h, w));
            // the general kernel: 1 / 4 planes at 382 / 384 workgroups of the two calls
            if (!deconv)
                for (int D : {764, 765}) pair(0, L("cin4 s%d 1 tile D%d", s, D), at(4, s, D, h, w));
        }
        const int Dlim = deconv ? 64 : 512;
        pair(deconv, "2^29 elements", at(lean_cin, 1, Dlim, 1024, 1024));
        pair(deconv, "2^29 elements less a row", at(lean_cin, 1, Dlim, 1023, 1024));
        if (deconv) pair(1, "3x2731x8191: 2^29 - 8 elements, one pixel less", at(8, 1, 3, 2731, 8191));
        else pair(0, "233x1103x2089: 2^29 - 1 elements", at(1, 1, 233, 1103, 2089));

        ConvPairArgs a;
        a.cout = deconv ? 1 : 8;
        const ConvPairArgs d = a;
        a.in_a = nullptr;
        pair(deconv, "null in_a", a);
        a = d, a.wgt_a = nullptr;
        pair(deconv, "null weight_a", a);
        a = d, a.bias_a = nullptr, a.bias_b = nullptr;
        pair(deconv, "null biases: allowed", a);
        a = d, a.out_a = nullptr;
        pair(deconv, "null out_a", a);
        a = d, a.in_b = nullptr;
        pair(deconv, "null in_b", a);
        a = d, a.wgt_b = nullptr;
        pair(deconv, "null weight_b", a);
        a = d, a.out_b = nullptr;
        pair(deconv, "null out_b", a);
        a = d, a.cin = 0;
        pair(deconv, "cin0", a);
        a = d, a.D = 0;
        pair(deconv, "D0", a);
        a = d, a.h = 0;
        pair(deconv, "h0", a);
        a = d, a.w = 0;
        pair(deconv, "w0", a);
        a = d, a.cout = deconv ? 8 : 16;
        pair(deconv, L("cout%d", a.cout), a);
    }
}

// ---- the transposed convolution ----------------------------------------------------------------------------------------------------
struct DeconvArgs {
    const float* in = P(2);
    int cin = 8;
    const float* wgt = P(10);
    const float* bias = P(11);
    int cout = 8, D = 6, h = 37, w = 50, sz = 2, relu = 1;
    const float* skip = nullptr;
    float* out = P(13);
    int n_smp = 3;
    long in_ss = 1000, skip_ss = 4000, out_ss = 5000;
};
static std::string deconv(bool batch, const std::string& label, const DeconvArgs& a) {
    g_rec.clear();
    const int rc = batch ? effi_deconv3d_k3_f32_batch(a.in, a.cin, a.wgt, a.bias, a.cout, a.D, a.h, a.w, a.sz, a.relu, a.skip, a.out, a.n_smp,
                                                      a.in_ss, a.skip_ss, a.out_ss, nullptr)
                         : effi_deconv3d_k3_f32(a.in, a.cin, a.wgt, a.bias, a.cout, a.D, a.h, a.w, a.sz, a.relu, a.skip, a.out, nullptr);
    emit(batch ? "effi_deconv3d_k3_f32_batch" : "effi_deconv3d_k3_f32", batch ? label + L(" n_smp%d", a.n_smp) : label, rc);
    return g_rec;
}
static void cases_deconv() {
    const DeconvArgs d;
    auto at = [&](int cin, int cout, int sz, int D = 6, int h = 37, int w = 50) {
        DeconvArgs a = d;
        a.cin = cin, a.cout = cout, a.sz = sz, a.D = D, a.h = h, a.w = w;
        return a;
    };
    for (int batch : {0, 1}) {
        // stride 2: 8 output channels per thread from 512 workgroups (one tile of the input map), 4 below
        for (int cout : {8, 16})
            for (int skip : {0, 1}) {
                DeconvArgs a = at(16, cout, 2);
                a.skip = skip ? P(12) : nullptr;
                deconv(batch, L("sz2 cout%d skip%d", cout, skip), a);
            }
        for (int D : {511, 512}) {
            DeconvArgs a = at(16, 8, 2, D, 7, 29);
            a.n_smp = 1;
            deconv(batch, L("sz2 cout8 1 tile D%d", D), a);
        }
        for (int D : {255, 256}) {
            DeconvArgs a = at(16, 16, 2, D, 7, 29);
            a.n_smp = 1;
            deconv(batch, L("sz2 cout16 1 tile D%d", D), a);
        }
        if (batch)
            for (int D : {73, 74}) {
                DeconvArgs a = at(16, 8, 2, D, 7, 29);
                a.n_smp = 7;
                deconv(1, L("sz2 cout8 1 tile D%d", D), a);                          // 73 x 7 = 511, 74 x 7 = 518
            }
        // stride 1 to one channel: the 8 -> 1 kernel (cin 8, no skip, option c3_lean bit 1) or the general body
        for (long lean : {EFFI_OPT_UNSET, 0L, 1L, 2L, 3L}) {
            Opt o(EFFI_OPT_C3_LEAN, lean);
            const std::string l = lean == EFFI_OPT_UNSET ? std::string("c3_lean unset") : L("c3_lean%ld", lean);
            deconv(batch, l + " sz1 cin8 cout1", at(8, 1, 1));
        }
        deconv(batch, "sz1 cin4 cout1", at(4, 1, 1));
        {
            DeconvArgs a = at(8, 1, 1);
            a.skip = P(12);
            deconv(batch, "sz1 cin8 cout1 skip: general body", a);
            a.cin = 4;
            deconv(batch, "sz1 cin4 cout1 skip", a);
        }
        for (int D : {4088, 4089}) {
            DeconvArgs a = at(8, 1, 1, D, 7, 29);
            a.n_smp = 1;
            deconv(batch, L("sz1 cin8 cout1 1 tile D%d", D), a);
        }
        if (batch)
            for (int D : {584, 585}) {
                DeconvArgs a = at(8, 1, 1, D, 7, 29);
                a.n_smp = 7;
                deconv(1, L("sz1 cin8 cout1 1 tile D%d", D), a);                  // 73 x 7 = 511, 74 x 7 = 518
            }
        deconv(batch, "sz1 cin8 cout1 64x1024x1024: 2^29 elements", at(8, 1, 1, 64, 1024, 1024));
        deconv(batch, "sz1 cin8 cout1 64x1023x1024", at(8, 1, 1, 64, 1023, 1024));
        deconv(batch, "sz1 cin8 cout1 3x2731x8191: 2^29 - 8 elements, one pixel less", at(8, 1, 1, 3, 2731, 8191));
        // refusals
        deconv(batch, "sz2 cout12", at(16, 12, 2));
        deconv(batch, "sz2 cout1", at(16, 1, 2));
        deconv(batch, "sz1 cout8", at(16, 8, 1));
        deconv(batch, "sz3 cout8", at(16, 8, 3));
        DeconvArgs a = d;
        a.in = nullptr;
        deconv(batch, "null in", a);
        a = d, a.wgt = nullptr;
        deconv(batch, "null weight", a);
        a = d, a.bias = nullptr;
        deconv(batch, "null bias: allowed", a);
        a = d, a.out = nullptr;
        deconv(batch, "null out", a);
        a = d, a.cin = 0;
        deconv(batch, "cin0", a);
        a = d, a.cout = 0;
        deconv(batch, "cout0", a);
        a = d, a.D = 0;
        deconv(batch, "D0", a);
        a = d, a.h = 0;
        deconv(batch, "h0", a);
        a = d, a.w = 0;
        deconv(batch, "w0", a);
        if (!batch) continue;
        for (int n : {0, 65536, 65535}) {
            a = d, a.n_smp = n;
            deconv(1, "samples", a);
        }
        a = d, a.in_ss = -1;
        deconv(1, "in_sstride < 0", a);
        a = d, a.in_ss = 0;
        deconv(1, "in_sstride = 0", a);
        a = d, a.skip_ss = -1;
        deconv(1, "skip_sstride < 0", a);
        a = d, a.out_ss = -1;
        deconv(1, "out_sstride < 0", a);
    }
    for (int route : {0, 1, 2}) {
        DeconvArgs a = route == 0 ? at(16, 8, 2) : route == 1 ? at(8, 1, 1) : at(4, 1, 1);
        a.n_smp = 1;
        const std::string one = deconv(1, L("route %d", route), a), plain = deconv(0, L("route %d (again)", route), a);
        if (one != plain || one.empty()) direct_failure(L("deconv3d route %d: n_smp = 1 is not the unbatched launch", route));
    }
}

// ---- soft-argmin: four entries behind one argument set -----------------------------------------------------------------------------
enum SoftEntry { S_PLAIN, S_UP, S_BATCH, S_UP_BATCH, S_ENTRIES };
static bool soft_up(int e) { return e == S_UP || e == S_UP_BATCH; }
static bool soft_batch(int e) { return e >= S_BATCH; }
struct SoftArgs {
    const float* logits = P(1);
    const float* depth = P(2);
    long dds = 1850, dps = 1;
    int D = 48, h = 37, w = 50;
    float* out_depth = P(3);
    float* out_conf = P(4);
    const float* range = P(5);
    int n_range = 2;
    float* out_dinv = P(6);
    float* out_up = P(7);
    int f = 4, n_smp = 3;
    long ss[7] = {1000, 2000, 3000, 4000, 5000, 6000, 7000};    // logits, depth, out_depth, out_conf, range, out_depth_inv, out_conf_up
};
static std::string soft(int e, const std::string& label, const SoftArgs& a) {
    g_rec.clear();
    int rc = -1;
    const char* name = "?";
    switch (e) {
        case S_PLAIN:
            name = "effi_softmax_regress_conf_f32";
            rc = effi_softmax_regress_conf_f32(a.logits, a.depth, a.dds, a.dps, a.D, a.h * a.w, a.out_depth, a.out_conf, a.range, a.n_range,
                                               a.out_dinv, nullptr);
            break;
        case S_UP:
            name = "effi_softmax_regress_conf_up_f32";
            rc = effi_softmax_regress_conf_up_f32(a.logits, a.depth, a.dds, a.dps, a.D, a.h, a.w, a.out_depth, a.out_conf, a.range, a.n_range,
                                                  a.out_dinv, a.out_up, a.f, nullptr);
            break;
        case S_BATCH:
            name = "effi_softmax_regress_conf_f32_batch";
            rc = effi_softmax_regress_conf_f32_batch(a.logits, a.depth, a.dds, a.dps, a.D, a.h * a.w, a.out_depth, a.out_conf, a.range,
                                                     a.n_range, a.out_dinv, a.n_smp, a.ss[0], a.ss[1], a.ss[2], a.ss[3], a.ss[4], a.ss[5], nullptr);
            break;
        case S_UP_BATCH:
            name = "effi_softmax_regress_conf_up_f32_batch";
            rc = effi_softmax_regress_conf_up_f32_batch(a.logits, a.depth, a.dds, a.dps, a.D, a.h, a.w, a.out_depth, a.out_conf, a.range,
                                                        a.n_range, a.out_dinv, a.out_up, a.f, a.n_smp, a.ss[0], a.ss[1], a.ss[2], a.ss[3],
                                                        a.ss[4], a.ss[5], a.ss[6], nullptr);
            break;
    }
    emit(name, soft_batch(e) ? label + L(" n_smp%d", a.n_smp) : label, rc);
    return g_rec;
}
static void cases_soft() {
    const SoftArgs d;
    for (int e = 0; e < S_ENTRIES; ++e) {
        for (int D : {8, 16, 32, 48, 64, 96, 24, 1})
            for (int dinv : {1, 0}) {
                SoftArgs a = d;
                a.D = D, a.out_dinv = dinv ? d.out_dinv : nullptr;
                if (!dinv) a.range = nullptr, a.n_range = 0;
                soft(e, L("D%d dinv%d", D, dinv), a);
            }
        SoftArgs a = d;
        if (soft_up(e)) {
            for (int f : {1, 2, 4}) {
                a = d, a.f = f, a.out_up = off(d.out_up, 1);
                soft(e, L("f%d out_conf_up misaligned", f), a);
                a = d, a.f = f, a.ss[6] = 7001;
                soft(e, L("f%d out_conf_up stride 7001", f), a);
            }
            a = d, a.out_up = nullptr;
            soft(e, "null out_conf_up", a);
            a = d, a.f = 0;
            soft(e, "f0", a);
            a = d, a.h = 0;
            soft(e, "h0", a);
            a = d, a.w = 0;
            soft(e, "w0", a);
        } else {
            a = d, a.h = 0;
            soft(e, "hw0", a);
        }
        a = d, a.logits = nullptr;
        soft(e, "null logits", a);
        a = d, a.depth = nullptr;
        soft(e, "null depth", a);
        a = d, a.out_depth = nullptr;
        soft(e, "null out_depth", a);
        a = d, a.out_conf = nullptr;
        soft(e, "null out_conf", a);
        a = d, a.range = nullptr;
        soft(e, "null disp_range with out_depth_inv", a);
        a = d, a.n_range = 1;
        soft(e, "n_range1 with out_depth_inv", a);
        a = d, a.D = 0;
        soft(e, "D0", a);
        if (!soft_batch(e)) continue;
        for (int n : {0, 65536, 65535}) {
            a = d, a.n_smp = n;
            soft(e, "samples", a);
        }
        for (int k = 0; k < (soft_up(e) ? 7 : 6); ++k) {
            a = d, a.ss[k] = -1;
            soft(e, L("stride %d < 0", k), a);
            a.ss[k] = 0;
            soft(e, L("stride %d = 0", k), a);
        }
    }
    for (int up : {0, 1})
        for (int D : {48, 24}) {
            SoftArgs a = d;
            a.D = D, a.n_smp = 1, a.ss[6] = 7001;                                 // (a misaligned stride no sample uses)
            const std::string one = soft(up ? S_UP_BATCH : S_BATCH, L("D%d", D), a), plain = soft(up ? S_UP : S_PLAIN, L("D%d (again)", D), a);
            if (one != plain || one.empty()) direct_failure(L("soft-argmin up %d D %d: n_smp = 1 is not the unbatched launch", up, D));
        }
}

// ---- the look-up family: GetCost, GetCost + 1x1 convolution, the three encoder-input entries ---------------------------------------
enum LookEntry { G_COST, G_CONV, G_ENC, G_ENC_X3, G_ENC_SR, G_ENTRIES };
static bool is_enc(int e) { return e >= G_ENC; }
struct LookArgs {
    const float* inv = P(1);
    const float* range = P(2);
    int n_range = 2, input_is_depth = 0;
    const float* itv = P(3);
    const float* cur = P(4);
    long cds = 1850, cps = 1;
    int Dcur = 8;
    const float* reg = P(5);
    long rds = 1, rps = 48;
    int Dreg = 48;
    const float* dmin = P(6);
    const float* dmax = P(7);
    long range_ps = 0;
    int nq = 3, h = 37, w = 50;
    const float* wgt = P(10);
    const float* bias = P(11);
    const float* wgt_d1 = P(12);
    const float* bias_d1 = P(13);
    int cout = 16, relu = 1;
    float* out = P(14);                     // cost / out / out_c1
    float* out_d1 = P(15);
    void* sr_c1 = P<void>(16);
    void* sr_d1 = P<void>(17);
    int hp = 50, wp = 66;
};
static void look(int e, const std::string& label, const LookArgs& a) {
    switch (e) {
        case G_COST:
            RUNF(effi_getcost_f32, label, a.inv, a.range, a.n_range, a.input_is_depth, a.itv, a.cur, a.cds, a.cps, a.Dcur, a.reg, a.rds, a.rps,
                 a.Dreg, a.dmin, a.dmax, a.range_ps, a.nq, a.h, a.w, a.out, nullptr);
            break;
        case G_CONV:
            RUNF(effi_getcost_conv1x1_f32, label, a.inv, a.range, a.n_range, a.input_is_depth, a.itv, a.cur, a.cds, a.cps, a.Dcur, a.reg, a.rds,
                 a.rps, a.Dreg, a.dmin, a.dmax, a.range_ps, a.nq, a.h, a.w, a.wgt, a.bias, a.cout, a.relu, a.out, nullptr);
            break;
        case G_ENC:
            RUNF(effi_encoder_inputs_f32, label, a.inv, a.range, a.n_range, a.itv, a.cur, a.cds, a.cps, a.Dcur, a.reg, a.rds, a.rps, a.Dreg,
                 a.dmin, a.dmax, a.range_ps, a.nq, a.h, a.w, a.wgt, a.bias, a.wgt_d1, a.bias_d1, a.cout, a.out, a.out_d1, nullptr);
            break;
        case G_ENC_X3:
            RUNF(effi_encoder_inputs_bf16x3_f32, label, a.inv, a.range, a.n_range, a.itv, a.cur, a.cds, a.cps, a.Dcur, a.reg, a.rds, a.rps,
                 a.Dreg, a.dmin, a.dmax, a.range_ps, a.nq, a.h, a.w, a.wgt, a.bias, a.wgt_d1, a.bias_d1, a.cout, a.out, a.out_d1, nullptr);
            break;
        case G_ENC_SR:
            RUNF(effi_encoder_inputs_bf16x3_sr, label, a.inv, a.range, a.n_range, a.itv, a.cur, a.cds, a.cps, a.Dcur, a.reg, a.rds, a.rps,
                 a.Dreg, a.dmin, a.dmax, a.range_ps, a.nq, a.h, a.w, a.wgt, a.bias, a.wgt_d1, a.bias_d1, a.cout, a.sr_c1, a.sr_d1, a.hp, a.wp,
                 nullptr);
            break;
    }
}
static void cases_look() {
    const LookArgs d;
    for (int e = 0; e < G_ENTRIES; ++e) {
        for (int nq : {2, 3, 4, 5}) {
            LookArgs a = d;
            a.nq = nq;
            look(e, L("nq%d", nq), a);
        }
        if (e != G_COST)
            for (int cout : {16, 32, 48, 24, 12, 8}) {
                LookArgs a = d;
                a.cout = cout;
                look(e, L("cout%d", cout), a);
            }
        for (int pp : {0, 1}) {
            LookArgs a = d;
            a.range_ps = pp;
            look(e, pp ? "per-pixel range" : "global range", a);
        }
        // 32-bit tap offsets: a planar volume [D][4096][4096] of 2^31 bytes (D = 32) and one row less, either volume
        for (int which : {0, 1})
            for (int h : {4096, 4095}) {
                LookArgs a = d;
                a.h = h, a.w = 4096, a.hp = 4112, a.wp = 4162;
                a.cds = a.rds = (long)h * 4096, a.cps = a.rps = 1, a.Dcur = which ? 8 : 32, a.Dreg = which ? 32 : 8;
                look(e, L("%s 32x%dx4096", which ? "reg_vol" : "cur_vol", h), a);
            }
        {
            LookArgs a = d;
            a.cds = -1;
            look(e, "cds < 0: 64-bit offsets", a);
            a = d, a.rps = -1;
            look(e, "rps < 0: 64-bit offsets", a);
        }
        if (!is_enc(e)) {
            LookArgs a = d;
            a.input_is_depth = 1;
            look(e, "input_is_depth", a);
            a.range = nullptr, a.n_range = 0;
            look(e, "input_is_depth, no disp_range", a);
            a = d, a.relu = 0;
            if (e == G_CONV) look(e, "relu0", a);
        }
        // refusals
        LookArgs a = d;
        a.inv = nullptr;
        look(e, "null inv_depth", a);
        a = d, a.range = nullptr;
        look(e, "null disp_range", a);
        a = d, a.n_range = 1;
        look(e, "n_range1", a);
        a = d, a.itv = nullptr;
        look(e, "null interval", a);
        a = d, a.cur = nullptr;
        look(e, "null cur_vol", a);
        a = d, a.reg = nullptr;
        look(e, "null reg_vol", a);
        a = d, a.dmin = nullptr;
        look(e, "null dmin", a);
        a = d, a.dmax = nullptr;
        look(e, "null dmax", a);
        a = d, a.Dcur = 1;
        look(e, "Dcur1", a);
        a = d, a.Dreg = 1;
        look(e, "Dreg1", a);
        a = d, a.nq = 1;
        look(e, "nq1", a);
        a = d, a.h = 0;
        look(e, "h0", a);
        a = d, a.w = 0;
        look(e, "w0", a);
        if (e == G_ENC_SR) {
            a = d, a.sr_c1 = nullptr;
            look(e, "null sr_c1", a);
            a = d, a.sr_d1 = nullptr;
            look(e, "null sr_d1", a);
            a = d, a.sr_c1 = off(d.sr_c1, 1);
            look(e, "sr_c1 misaligned", a);
            a = d, a.sr_d1 = off(d.sr_d1, 2);
            look(e, "sr_d1 misaligned", a);
            a = d, a.hp = 38;
            look(e, "hp = h + 1", a);
            a.hp = 39;
            look(e, "hp = h + 2", a);
            a = d, a.wp = 51;
            look(e, "wp = w + 1", a);
            a.wp = 52;
            look(e, "wp = w + 2", a);
        } else {
            a = d, a.out = nullptr;
            look(e, e == G_COST ? "null cost" : is_enc(e) ? "null out_c1" : "null out", a);
        }
        if (e == G_COST) continue;
        a = d, a.wgt = nullptr;
        look(e, "null weight", a);
        a = d, a.bias = nullptr;
        look(e, "null bias", a);
        a = d, a.cout = 0;
        look(e, "cout0", a);
        if (!is_enc(e)) continue;
        a = d, a.wgt_d1 = nullptr;
        look(e, "null weight_d1", a);
        a = d, a.bias_d1 = nullptr;
        look(e, "null bias_d1", a);
        a = d, a.out_d1 = nullptr;
        if (e != G_ENC_SR) look(e, "null out_d1", a);
    }
}

// ---- 1-D look-ups, view aggregation, the small per-pixel entries -------------------------------------------------------------------
static void cases_lookup1d() {
    const float* vol = P(1);
    const float* vol_b = P(2);
    const float* q = P(3);
    const float* dmin = P(4);
    const float* dmax = P(5);
    float* out = P(6);
    float* out_b = P(7);
    for (int pair : {0, 1}) {
        auto run = [&](const std::string& label, const float* v, const float* vb, int Dp, const float* qq, int nq, const float* lo, const float* hi,
                       long rps, int h, int w, float* o, float* ob) {
            if (pair) RUNF(effi_vol_lookup1d_pair_f32, label, v, vb, 1850L, 1L, Dp, qq, 1850L, 50L, 1L, nq, lo, hi, rps, h, w, o, ob, nullptr);
            else RUNF(effi_vol_lookup1d_f32, label, v, 1850L, 1L, Dp, qq, 1850L, 50L, 1L, nq, lo, hi, rps, h, w, o, nullptr);
        };
        run("Dp48 nq3 global range", vol, vol_b, 48, q, 3, dmin, dmax, 0, 37, 50, out, out_b);
        run("Dp8 nq1 per-pixel range", vol, vol_b, 8, q, 1, dmin, dmax, 1, 37, 50, out, out_b);
        run("1x1", vol, vol_b, 2, q, 1, dmin, dmax, 0, 1, 1, out, out_b);
        run("null vol", nullptr, vol_b, 48, q, 3, dmin, dmax, 0, 37, 50, out, out_b);
        if (pair) run("null vol_b", vol, nullptr, 48, q, 3, dmin, dmax, 0, 37, 50, out, out_b);
        run("null query", vol, vol_b, 48, nullptr, 3, dmin, dmax, 0, 37, 50, out, out_b);
        run("null dmin", vol, vol_b, 48, q, 3, nullptr, dmax, 0, 37, 50, out, out_b);
        run("null dmax", vol, vol_b, 48, q, 3, dmin, nullptr, 0, 37, 50, out, out_b);
        run("null out", vol, vol_b, 48, q, 3, dmin, dmax, 0, 37, 50, nullptr, out_b);
        if (pair) run("null out_b", vol, vol_b, 48, q, 3, dmin, dmax, 0, 37, 50, out, nullptr);
        run("Dp1", vol, vol_b, 1, q, 3, dmin, dmax, 0, 37, 50, out, out_b);
        run("nq0", vol, vol_b, 48, q, 0, dmin, dmax, 0, 37, 50, out, out_b);
        run("h0", vol, vol_b, 48, q, 3, dmin, dmax, 0, 0, 50, out, out_b);
        run("w0", vol, vol_b, 48, q, 3, dmin, dmax, 0, 37, 0, out, out_b);
    }
    const float* img = P(1);
    const float* coords = P(2);
    float* mask = P(4);
    RUNF(effi_bilinear_sampler1d_f32, "N1850 C1 W48 nq3 mask", img, 1850, 1, 48, coords, 3L, out, mask, nullptr);
    RUNF(effi_bilinear_sampler1d_f32, "N7 C5 W9 nq1 no mask", img, 7, 5, 9, coords, 1L, out, nullptr, nullptr);
    RUNF(effi_bilinear_sampler1d_f32, "null img", nullptr, 7, 5, 9, coords, 1L, out, mask, nullptr);
    RUNF(effi_bilinear_sampler1d_f32, "null coords", img, 7, 5, 9, nullptr, 1L, out, mask, nullptr);
    RUNF(effi_bilinear_sampler1d_f32, "null out", img, 7, 5, 9, coords, 1L, nullptr, mask, nullptr);
    RUNF(effi_bilinear_sampler1d_f32, "N0", img, 0, 5, 9, coords, 1L, out, mask, nullptr);
    RUNF(effi_bilinear_sampler1d_f32, "C0", img, 7, 0, 9, coords, 1L, out, mask, nullptr);
    RUNF(effi_bilinear_sampler1d_f32, "W0", img, 7, 5, 0, coords, 1L, out, mask, nullptr);
    RUNF(effi_bilinear_sampler1d_f32, "nq0", img, 7, 5, 9, coords, 0L, out, mask, nullptr);
}

struct AggArgs {
    const float* sim = P(1);
    const float* wts = P(2);
    int S = 3, D = 48, hw = 1850;
    float* out = P(3);
    int n_smp = 3;
    long ss[3] = {1000, 2000, 3000};
};
static std::string agg(bool batch, const std::string& label, const AggArgs& a) {
    g_rec.clear();
    const int rc = batch ? effi_view_aggregate_f32_batch(a.sim, a.wts, a.S, a.D, a.hw, a.out, a.n_smp, a.ss[0], a.ss[1], a.ss[2], nullptr)
                         : effi_view_aggregate_f32(a.sim, a.wts, a.S, a.D, a.hw, a.out, nullptr);
    emit(batch ? "effi_view_aggregate_f32_batch" : "effi_view_aggregate_f32", batch ? label + L(" n_smp%d", a.n_smp) : label, rc);
    return g_rec;
}
static void cases_agg() {
    const AggArgs d;
    for (int batch : {0, 1}) {
        agg(batch, "S3 D48", d);
        AggArgs a = d;
        a.S = EFFI_MAX_VIEWS, a.D = 9, a.hw = 257;
        agg(batch, "S12 D9 hw257", a);
        a = d, a.wts = nullptr;
        agg(batch, "null weights: the plain mean", a);
        a = d, a.sim = nullptr;
        agg(batch, "null sim_views", a);
        a = d, a.out = nullptr;
        agg(batch, "null out", a);
        for (int S : {0, EFFI_MAX_VIEWS + 1}) {
            a = d, a.S = S;
            agg(batch, L("S%d", S), a);
        }
        a = d, a.D = 0;
        agg(batch, "D0", a);
        a = d, a.hw = 0;
        agg(batch, "hw0", a);
        if (!batch) continue;
        for (int n : {0, 65536, 65535}) {
            a = d, a.n_smp = n;
            agg(1, "samples", a);
        }
        for (int k = 0; k < 3; ++k) {
            a = d, a.ss[k] = -1;
            agg(1, L("stride %d < 0", k), a);
            a.ss[k] = 0;
            agg(1, L("stride %d = 0", k), a);
        }
        a = d, a.n_smp = 1, a.sim = nullptr;
        agg(1, "null sim_views", a);
    }
    AggArgs a = d;
    a.n_smp = 1;
    if (agg(1, "S3 D48", a) != agg(0, "S3 D48 (again)", a)) direct_failure("view_aggregate: n_smp = 1 is not the unbatched launch");
}

static void cases_small() {
    // planar -> NHWC: the lists past n stay null
    const float* srcs[EFFI_MAX_VIEWS + 2];
    float* dsts[EFFI_MAX_VIEWS + 2];
    for (int i = 0; i < EFFI_MAX_VIEWS + 2; ++i) srcs[i] = P(20 + i), dsts[i] = P(40 + i);
    for (int n : {1, 3, EFFI_MAX_VIEWS + 1, 0, EFFI_MAX_VIEWS + 2}) RUNF(effi_planar_to_nhwc_f32, L("n%d C32 HW1850", n), srcs, dsts, n, 32, 1850, nullptr);
    RUNF(effi_planar_to_nhwc_f32, "C128 HW64", srcs, dsts, 2, 128, 64, nullptr);
    RUNF(effi_planar_to_nhwc_f32, "C129", srcs, dsts, 2, 129, 1850, nullptr);
    RUNF(effi_planar_to_nhwc_f32, "C0", srcs, dsts, 2, 0, 1850, nullptr);
    RUNF(effi_planar_to_nhwc_f32, "HW0", srcs, dsts, 2, 32, 0, nullptr);
    RUNF(effi_planar_to_nhwc_f32, "null srcs", nullptr, dsts, 2, 32, 1850, nullptr);
    RUNF(effi_planar_to_nhwc_f32, "null dsts", srcs, nullptr, 2, 32, 1850, nullptr);
    srcs[1] = nullptr;
    RUNF(effi_planar_to_nhwc_f32, "null srcs[1]", srcs, dsts, 2, 32, 1850, nullptr);
    RUNF(effi_planar_to_nhwc_f32, "null srcs[1] past n", srcs, dsts, 1, 32, 1850, nullptr);
    srcs[1] = P(21), dsts[1] = nullptr;
    RUNF(effi_planar_to_nhwc_f32, "null dsts[1]", srcs, dsts, 2, 32, 1850, nullptr);

    // the context split: float4 form for hw % 4 == 0 and 16-byte aligned pointers
    const float* ctx = P(1);
    float* hid = P(2);
    float* inp = P(3);
    RUNF(effi_split_tanh_relu_f32, "hd32 cd32 hw1852", ctx, 32, 32, 1852, hid, inp, nullptr);
    RUNF(effi_split_tanh_relu_f32, "hd32 cd32 hw1850: hw % 4", ctx, 32, 32, 1850, hid, inp, nullptr);
    RUNF(effi_split_tanh_relu_f32, "hw1852 ctx misaligned", off(ctx, 1), 32, 32, 1852, hid, inp, nullptr);
    RUNF(effi_split_tanh_relu_f32, "hw1852 hidden misaligned", ctx, 32, 32, 1852, off(hid, 2), inp, nullptr);
    RUNF(effi_split_tanh_relu_f32, "hw1852 inp misaligned", ctx, 32, 32, 1852, hid, off(inp, 3), nullptr);
    RUNF(effi_split_tanh_relu_f32, "hw2^20: the scalar grid stops at 4096", off(ctx, 1), 32, 32, 1 << 20, hid, inp, nullptr);
    RUNF(effi_split_tanh_relu_f32, "null ctx", nullptr, 32, 32, 1852, hid, inp, nullptr);
    RUNF(effi_split_tanh_relu_f32, "null hidden", ctx, 32, 32, 1852, nullptr, inp, nullptr);
    RUNF(effi_split_tanh_relu_f32, "null inp", ctx, 32, 32, 1852, hid, nullptr, nullptr);
    RUNF(effi_split_tanh_relu_f32, "hd0", ctx, 0, 32, 1852, hid, inp, nullptr);
    RUNF(effi_split_tanh_relu_f32, "cd0", ctx, 32, 0, 1852, hid, inp, nullptr);
    RUNF(effi_split_tanh_relu_f32, "hw0", ctx, 32, 32, 0, hid, inp, nullptr);

    RUNF(effi_depth_to_inv_f32, "n1850", P(1), P(2), 2, 1850, P(3), nullptr);
    RUNF(effi_depth_to_inv_f32, "n2^21: the grid stops at 4096", P(1), P(2), 2, 1 << 21, P(3), nullptr);
    RUNF(effi_depth_to_inv_f32, "null depth", nullptr, P(2), 2, 1850, P(3), nullptr);
    RUNF(effi_depth_to_inv_f32, "null disp_range", P(1), nullptr, 2, 1850, P(3), nullptr);
    RUNF(effi_depth_to_inv_f32, "null inv", P(1), P(2), 2, 1850, nullptr, nullptr);
    RUNF(effi_depth_to_inv_f32, "n_range1", P(1), P(2), 1, 1850, P(3), nullptr);
    RUNF(effi_depth_to_inv_f32, "n0", P(1), P(2), 2, 0, P(3), nullptr);

    RUNF(effi_stage1_hypotheses_f32, "D48", P(1), 2, 48, P(2), P(3), nullptr);
    RUNF(effi_stage1_hypotheses_f32, "null disp_range", nullptr, 2, 48, P(2), P(3), nullptr);
    RUNF(effi_stage1_hypotheses_f32, "null depths", P(1), 2, 48, nullptr, P(3), nullptr);
    RUNF(effi_stage1_hypotheses_f32, "null intervals", P(1), 2, 48, P(2), nullptr, nullptr);
    RUNF(effi_stage1_hypotheses_f32, "n_range1", P(1), 1, 48, P(2), P(3), nullptr);
    RUNF(effi_stage1_hypotheses_f32, "D1", P(1), 2, 1, P(2), P(3), nullptr);

    RUNF(effi_upsample_nearest_f32, "C1 37x50 f4", P(1), 1, 37, 50, 4, P(2), nullptr);
    RUNF(effi_upsample_nearest_f32, "C8 370x500 f4: the grid stops at 8192", P(1), 8, 370, 500, 4, P(2), nullptr);
    RUNF(effi_upsample_nearest_f32, "null in", nullptr, 1, 37, 50, 4, P(2), nullptr);
    RUNF(effi_upsample_nearest_f32, "null out", P(1), 1, 37, 50, 4, nullptr, nullptr);
    RUNF(effi_upsample_nearest_f32, "C0", P(1), 0, 37, 50, 4, P(2), nullptr);
    RUNF(effi_upsample_nearest_f32, "h0", P(1), 1, 0, 50, 4, P(2), nullptr);
    RUNF(effi_upsample_nearest_f32, "w0", P(1), 1, 37, 0, 4, P(2), nullptr);
    RUNF(effi_upsample_nearest_f32, "f0", P(1), 1, 37, 50, 0, P(2), nullptr);

    RUNF(effi_head_update_f32, "37x52", P(1), P(2), P(3), P(4), 2, 37, 52, P(5), P(6), nullptr);
    RUNF(effi_head_update_f32, "37x50: w % 4", P(1), P(2), P(3), P(4), 2, 37, 50, P(5), P(6), nullptr);
    RUNF(effi_head_update_f32, "null partial9", nullptr, P(2), P(3), P(4), 2, 37, 52, P(5), P(6), nullptr);
    RUNF(effi_head_update_f32, "null bias2", P(1), nullptr, P(3), P(4), 2, 37, 52, P(5), P(6), nullptr);
    RUNF(effi_head_update_f32, "null inv_depth", P(1), P(2), nullptr, P(4), 2, 37, 52, P(5), P(6), nullptr);
    RUNF(effi_head_update_f32, "null disp_range", P(1), P(2), P(3), nullptr, 2, 37, 52, P(5), P(6), nullptr);
    RUNF(effi_head_update_f32, "n_range1", P(1), P(2), P(3), P(4), 1, 37, 52, P(5), P(6), nullptr);
    RUNF(effi_head_update_f32, "null out_inv", P(1), P(2), P(3), P(4), 2, 37, 52, nullptr, P(6), nullptr);
    RUNF(effi_head_update_f32, "null out_depth", P(1), P(2), P(3), P(4), 2, 37, 52, P(5), nullptr, nullptr);
    RUNF(effi_head_update_f32, "h0", P(1), P(2), P(3), P(4), 2, 0, 52, P(5), P(6), nullptr);
    RUNF(effi_head_update_f32, "w0", P(1), P(2), P(3), P(4), 2, 37, 0, P(5), P(6), nullptr);

    for (int cout : {16, 32, 48, 24}) RUNF(effi_conv2d_c1k7_relu_bf16x3_f32, L("cout%d 37x50", cout), P(1), P(2), P(3), cout, 37, 50, P(4), nullptr);
    RUNF(effi_conv2d_c1k7_relu_bf16x3_f32, "null in", nullptr, P(2), P(3), 16, 37, 50, P(4), nullptr);
    RUNF(effi_conv2d_c1k7_relu_bf16x3_f32, "null weight", P(1), nullptr, P(3), 16, 37, 50, P(4), nullptr);
    RUNF(effi_conv2d_c1k7_relu_bf16x3_f32, "null bias", P(1), P(2), nullptr, 16, 37, 50, P(4), nullptr);
    RUNF(effi_conv2d_c1k7_relu_bf16x3_f32, "null out", P(1), P(2), P(3), 16, 37, 50, nullptr, nullptr);
    RUNF(effi_conv2d_c1k7_relu_bf16x3_f32, "h0", P(1), P(2), P(3), 16, 0, 50, P(4), nullptr);
    RUNF(effi_conv2d_c1k7_relu_bf16x3_f32, "w0", P(1), P(2), P(3), 16, 37, 0, P(4), nullptr);

    RUNF(effi_convex_upsample2x_f32, "37x50 all outputs", P(1), P(2), P(3), 2, 37, 50, P(4), P(5), P(6), nullptr);
    RUNF(effi_convex_upsample2x_f32, "out_inv only, no range", P(1), P(2), nullptr, 0, 37, 50, P(4), nullptr, nullptr, nullptr);
    RUNF(effi_convex_upsample2x_f32, "out_depth only", P(1), P(2), P(3), 2, 37, 50, nullptr, P(5), nullptr, nullptr);
    RUNF(effi_convex_upsample2x_f32, "null inv_depth", nullptr, P(2), P(3), 2, 37, 50, P(4), P(5), P(6), nullptr);
    RUNF(effi_convex_upsample2x_f32, "null mask", P(1), nullptr, P(3), 2, 37, 50, P(4), P(5), P(6), nullptr);
    RUNF(effi_convex_upsample2x_f32, "no output", P(1), P(2), P(3), 2, 37, 50, nullptr, nullptr, nullptr, nullptr);
    RUNF(effi_convex_upsample2x_f32, "out_depth without disp_range", P(1), P(2), nullptr, 2, 37, 50, P(4), P(5), P(6), nullptr);
    RUNF(effi_convex_upsample2x_f32, "out_depth n_range1", P(1), P(2), P(3), 1, 37, 50, P(4), P(5), P(6), nullptr);
    RUNF(effi_convex_upsample2x_f32, "out_depth_inv without out_depth", P(1), P(2), P(3), 2, 37, 50, P(4), nullptr, P(6), nullptr);
    RUNF(effi_convex_upsample2x_f32, "h0", P(1), P(2), P(3), 2, 0, 50, P(4), P(5), P(6), nullptr);
    RUNF(effi_convex_upsample2x_f32, "w0", P(1), P(2), P(3), 2, 37, 0, P(4), P(5), P(6), nullptr);
}

// ---- the splitters over the stages, split-resident maps ----------------------------------------------------------------------------
struct StageArgs {
    const float* ctx[4] = {P(1), P(2), P(3), P(4)};
    int hd[4] = {32, 32, 16, 8}, cd[4] = {32, 16, 16, 4}, h[4] = {37, 74, 148, 9}, w[4] = {50, 100, 200, 12}, hw[4] = {1852, 7400, 29600, 108};
    float* hidden[4] = {P(5), P(6), P(7), P(8)};
    float* inp[4] = {P(9), P(10), P(11), P(12)};
    void* hidden_sr[4] = {P<void>(13), P<void>(14), P<void>(15), P<void>(16)};
    int hp[4] = {50, 82, 162, 18}, wp[4] = {66, 114, 210, 18}, q4[4] = {0, 1, 0, 1};
    void* clear_base[4] = {P<void>(17), P<void>(18), P<void>(19), P<void>(20)};
    int clear_planes[4] = {4, 2, 6, 1};
    int n = 3;
};
enum StageEntry { T_PLAIN, T_SR, T_SR_CLEAR, T_ENTRIES };
static void stages(int e, const std::string& label, const StageArgs& a, int null_arg = -1) {
    // null_arg: which pointer argument of the entry is passed as null
    auto arg = [&](int k, auto p) { return null_arg == k ? decltype(p)(nullptr) : p; };
    const std::string l = label + L(" n%d", a.n);
    if (e == T_PLAIN)
        RUNF(effi_split_tanh_relu_stages_f32, l, arg(0, (const float* const*)a.ctx), arg(1, (const int*)a.hd), arg(2, (const int*)a.cd),
             arg(3, (const int*)a.hw), arg(4, (float* const*)a.hidden), arg(5, (float* const*)a.inp), a.n, nullptr);
    else if (e == T_SR)
        RUNF(effi_split_tanh_relu_stages_sr_f32, l, arg(0, (const float* const*)a.ctx), arg(1, (const int*)a.hd), arg(2, (const int*)a.cd),
             arg(3, (const int*)a.h), arg(4, (const int*)a.w), arg(5, (float* const*)a.hidden), arg(6, (void* const*)a.hidden_sr),
             arg(7, (const int*)a.hp), arg(8, (const int*)a.wp), arg(9, (float* const*)a.inp), arg(10, (const int*)a.q4), a.n, nullptr);
    else
        RUNF(effi_split_tanh_relu_stages_sr_clear_f32, l, arg(0, (const float* const*)a.ctx), arg(1, (const int*)a.hd), arg(2, (const int*)a.cd),
             arg(3, (const int*)a.h), arg(4, (const int*)a.w), arg(5, (float* const*)a.hidden), arg(6, (void* const*)a.hidden_sr),
             arg(7, (const int*)a.hp), arg(8, (const int*)a.wp), arg(9, (float* const*)a.inp), arg(10, (const int*)a.q4), arg(11, (void* const*)a.clear_base),
             arg(12, (const int*)a.clear_planes), a.n, nullptr);
}
static void cases_stages() {
    const StageArgs d;
    for (int e = 0; e < T_ENTRIES; ++e) {
        for (int n : {1, 2, 3, 4, 0, 5}) {
            StageArgs a = d;
            a.n = n;
            stages(e, "stages", a);
        }
        for (int k = 0; k < (e == T_PLAIN ? 6 : e == T_SR ? 11 : 13); ++k) stages(e, L("null argument %d", k), d, k);
        for (int which : {0, 1, 2}) {
            StageArgs a = d;
            if (which == 0) a.ctx[1] = nullptr;
            else if (which == 1) a.hidden[1] = nullptr;
            else a.inp[1] = nullptr;
            stages(e, L("null %s[1]", which == 0 ? "ctx" : which == 1 ? "hidden" : "inp"), a);
            a.n = 1;
            stages(e, L("null %s[1] past n", which == 0 ? "ctx" : which == 1 ? "hidden" : "inp"), a);
        }
        StageArgs a = d;
        a.hd[2] = 0;
        stages(e, "hd[2] = 0", a);
        a = d, a.cd[2] = 0;
        stages(e, "cd[2] = 0", a);
        if (e == T_PLAIN) {
            a = d, a.hw[2] = 0;
            stages(e, "hw[2] = 0", a);
            // the float4 form: every map's halves a multiple of 4 elements and every pointer 16-byte aligned
            a = d, a.hw[1] = 7401;
            stages(e, "hw[1] odd, both halves still multiples of 4: float4", a);    // 32 x 7401, 48 x 7401
            a = d, a.hw[1] = 7401, a.hd[1] = 2;
            stages(e, "hd[1] x hw[1] % 4: scalar", a);                             // 2 x 7401 = 14802
            a = d, a.hw[1] = 7401, a.hd[1] = 4, a.cd[1] = 1;
            stages(e, "(hd[1] + cd[1]) x hw[1] % 4: scalar", a);                   // 4 x 7401 is a multiple, 5 x 7401 is not
            a = d, a.hw[3] = 109, a.hd[3] = 1;
            stages(e, "hd[3] x hw[3] % 4 past n: float4", a);
            a = d, a.ctx[0] = off(d.ctx[0], 1);
            stages(e, "ctx[0] misaligned: scalar", a);
            a = d, a.hidden[2] = off(d.hidden[2], 2);
            stages(e, "hidden[2] misaligned: scalar", a);
            a = d, a.inp[1] = off(d.inp[1], 3);
            stages(e, "inp[1] misaligned: scalar", a);
            a = d, a.inp[3] = off(d.inp[3], 3);
            stages(e, "inp[3] misaligned past n", a);
            continue;
        }
        a = d, a.h[2] = 0;
        stages(e, "h[2] = 0", a);
        a = d, a.w[2] = 0;
        stages(e, "w[2] = 0", a);
        a = d, a.hidden_sr[1] = nullptr;
        stages(e, "null hidden_sr[1]", a);
        a = d, a.hidden_sr[1] = off(d.hidden_sr[1], 1);
        stages(e, "hidden_sr[1] misaligned", a);
        a = d, a.hd[0] = 4;
        stages(e, "hd[0] = 4", a);
        a = d, a.hd[0] = 12;
        stages(e, "hd[0] = 12", a);
        a = d, a.cd[0] = 2;
        stages(e, "cd[0] = 2", a);
        a = d, a.cd[0] = 6;
        stages(e, "cd[0] = 6", a);
        a = d, a.hp[1] = 75;
        stages(e, "hp[1] = h + 1", a);
        a.hp[1] = 76;
        stages(e, "hp[1] = h + 2", a);
        a = d, a.wp[1] = 101;
        stages(e, "wp[1] = w + 1", a);
        a = d, a.hidden[1] = off(d.hidden[1], 1);
        stages(e, "hidden[1] misaligned with hidden_q4", a);
        a = d, a.hidden[0] = off(d.hidden[0], 1);
        stages(e, "hidden[0] misaligned without hidden_q4", a);
        if (e != T_SR_CLEAR) continue;
        a = d, a.clear_base[1] = nullptr;
        stages(e, "null clear_base[1]", a);
        a = d, a.clear_base[1] = off(d.clear_base[1], 1);
        stages(e, "clear_base[1] misaligned", a);
        a = d, a.clear_planes[1] = 0;
        stages(e, "clear_planes[1] = 0", a);
    }
}

static void cases_sr() {
    for (int h : {37, 16, 1})
        for (int w : {50, 511, 512, 513}) {
            int hp = -1, wp = -1;
            const int rc = effi_sr_geometry(h, w, &hp, &wp);
            std::printf("effi_sr_geometry | %dx%d | %s hp=%d wp=%d\n", h, w, rc_name(rc), hp, wp);
        }
    int hp = -1, wp = -1;
    std::printf("effi_sr_geometry | h0 | %s\n", rc_name(effi_sr_geometry(0, 50, &hp, &wp)));
    std::printf("effi_sr_geometry | w0 | %s\n", rc_name(effi_sr_geometry(37, 0, &hp, &wp)));
    std::printf("effi_sr_geometry | null hp | %s\n", rc_name(effi_sr_geometry(37, 50, nullptr, &wp)));
    std::printf("effi_sr_geometry | null wp | %s\n", rc_name(effi_sr_geometry(37, 50, &hp, nullptr)));

    struct Groups {
        void* maps[4] = {P<void>(1), P<void>(2), P<void>(3), P<void>(4)};
        int planes[4] = {4, 2, 6, 1}, h[4] = {37, 74, 148, 9}, w[4] = {50, 100, 200, 12}, hp[4] = {50, 82, 162, 18}, wp[4] = {66, 114, 210, 18};
    };
    const Groups d;
    auto clear = [&](const std::string& label, const Groups& g, int n, int null_arg = -1) {
        RUNF(effi_sr_clear_border, label + L(" n%d", n), null_arg == 0 ? nullptr : (void* const*)g.maps, null_arg == 1 ? nullptr : g.planes,
             null_arg == 2 ? nullptr : g.h, null_arg == 3 ? nullptr : g.w, null_arg == 4 ? nullptr : g.hp, null_arg == 5 ? nullptr : g.wp, n, nullptr);
    };
    for (int n : {1, 2, 3, 4, 0, 5}) clear("groups", d, n);
    for (int k = 0; k < 6; ++k) clear(L("null argument %d", k), d, 3, k);
    Groups g = d;
    g.maps[1] = nullptr;
    clear("null maps[1]", g, 3);
    clear("null maps[1] past n", g, 1);
    g = d, g.maps[1] = off(d.maps[1], 1);
    clear("maps[1] misaligned", g, 3);
    g = d, g.planes[2] = 0;
    clear("planes[2] = 0", g, 3);
    g = d, g.h[2] = 0;
    clear("h[2] = 0", g, 3);
    g = d, g.w[2] = 0;
    clear("w[2] = 0", g, 3);
    g = d, g.hp[0] = 38;
    clear("hp[0] = h + 1", g, 3);
    g.hp[0] = 39;
    clear("hp[0] = h + 2", g, 3);
    g = d, g.wp[0] = 51;
    clear("wp[0] = w + 1", g, 3);
    g.wp[0] = 52;
    clear("wp[0] = w + 2", g, 3);

    const float* in = P(1);
    void* sr = P<void>(2);
    RUNF(effi_sr_from_planar_f32, "C32 37x50", in, 32, 37, 50, sr, 50, 66, nullptr);
    RUNF(effi_sr_from_planar_f32, "C8 1x1", in, 8, 1, 1, sr, 3, 3, nullptr);
    RUNF(effi_sr_from_planar_f32, "null in", nullptr, 32, 37, 50, sr, 50, 66, nullptr);
    RUNF(effi_sr_from_planar_f32, "null sr", in, 32, 37, 50, nullptr, 50, 66, nullptr);
    RUNF(effi_sr_from_planar_f32, "sr misaligned", in, 32, 37, 50, off(sr, 1), 50, 66, nullptr);
    RUNF(effi_sr_from_planar_f32, "C0", in, 0, 37, 50, sr, 50, 66, nullptr);
    RUNF(effi_sr_from_planar_f32, "C12", in, 12, 37, 50, sr, 50, 66, nullptr);
    RUNF(effi_sr_from_planar_f32, "h0", in, 32, 0, 50, sr, 50, 66, nullptr);
    RUNF(effi_sr_from_planar_f32, "w0", in, 32, 37, 0, sr, 50, 66, nullptr);
    RUNF(effi_sr_from_planar_f32, "hp = h + 1", in, 32, 37, 50, sr, 38, 66, nullptr);
    RUNF(effi_sr_from_planar_f32, "wp = w + 1", in, 32, 37, 50, sr, 50, 51, nullptr);
}

int main() {
    for (long& v : g_opt) v = EFFI_OPT_UNSET;
    cases_conv();
    cases_pair();
    cases_deconv();
    cases_soft();
    cases_look();
    cases_lookup1d();
    cases_agg();
    cases_small();
    cases_stages();
    cases_sr();
    if (g_failures) std::printf("vol host check: %d FAILED\n", g_failures);
    return g_failures ? 1 : 0;
}
