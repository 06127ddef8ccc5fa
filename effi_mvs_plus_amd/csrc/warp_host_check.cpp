// Stand-alone host check of the warp and correlation entries of csrc/warpcorr.hip: make -C effi_mvs_plus_amd/csrc host-check.  Every
// extern "C" entry is called over a table of cases that reaches each branch of its host code (window / gather / matrix-core forms of
// the views family, the four forms of the dynamic stage, channel counts, options, tables, sample batches, refusals), and every launch
// is RECORDED instead of made (host_check_record.hpp): kernel instantiation, grid, block and each by-value argument, field by field.
// The records are compared with tests/golden/warp_launch_records.txt (tests/test_warp_host_check.py), which pins what the GPU tests
// cannot see: the forms of a stage are equal by design, so a wrong instantiation, grid, window size or sample stride passes them.
// NOTHING here reaches a GPU: the program is compiled for the host only, under -fsanitize=address,undefined and
// -ftrivial-auto-var-init=pattern (an argument field an entry leaves unset prints as 0xAA..), and the made-up device addresses are
// copied into the arguments and never read through.  One program serves every precision: hi_only is a run-time argument.
#include "host_check_record.hpp"           // the recorder: the launch macro is redefined from here on
#include "warpcorr.hip"

static void show_one(const EffiPtrList& l) {
    for (int i = 0; i <= EFFI_MAX_VIEWS; ++i) ptr(L("p%d", i).c_str(), l.p[i]);
    FP(l, tbl);
}
static void show_one(const EffiOutList& l) {
    for (int i = 0; i <= EFFI_MAX_VIEWS; ++i) ptr(L("p%d", i).c_str(), l.p[i]);
}
static void show_one(const EffiTableArgs& a) {
    for (int i = 0; i < EFFI_VIEW_TABLE_MAX; ++i) ptr(L("p%d", i).c_str(), a.p[i]);
}
namespace {                                 // (beside the struct: the recorder's show finds it by argument-dependent lookup)
void show_one(const WarpBatch& b) { FI(b, ref), FI(b, src), FI(b, rt), FI(b, depth), FI(b, sim), FI(b, ent); }
}  // namespace

static void direct_failure(const std::string& what) {
    std::printf("FAILED: %s\n", what.c_str());
    ++g_failures;
}

// ---- made-up arguments -------------------------------------------------------------------------------------------------------------
static const float* const SRC[EFFI_MAX_VIEWS + 1] = {P(2), P(3), P(4), P(5), P(6), P(7), P(8), P(9), P(10), P(11), P(12), P(13), P(14)};
static float* const GSRC[EFFI_MAX_VIEWS + 1] = {P(42), P(43), P(44), P(45), P(46), P(47), P(48), P(49), P(50), P(51), P(52), P(53), P(54)};
static const float* const SRC_NULL1[3] = {P(2), nullptr, P(4)};
static float* const GSRC_NULL1[3] = {P(42), nullptr, P(44)};
static const float* const* const TBL = P<const float*>(30);

// the stage-1 ("views") family: six forward entries behind one argument set
enum ViewsEntry { V_PLAIN, V_TBL, V_BATCH, V_X3, V_X3_TBL, V_X3_BATCH, V_ENTRIES };
static bool is_tbl(int e) { return e == V_TBL || e == V_X3_TBL; }
static bool is_batch(int e) { return e == V_BATCH || e == V_X3_BATCH; }
static bool is_x3(int e) { return e >= V_X3; }
struct ViewsArgs {
    const float* ref = P(1);
    const float* const* src = SRC;
    const float* const* tbl = TBL;
    int S = 3;
    const float* rt = P(20);
    const float* depth = P(21);
    long dds = 11, dps = 0;
    int C = 32, h = 37, w = 50, D = 48;     // (h, w: no multiple of any tile)
    float* sim = P(22);
    float* ent = P(23);
    int hi_only = 0, n_smp = 3;
    long ss[6] = {1000, 2000, 3000, 4000, 5000, 6000};          // sample strides: ref, src, rt, depth, sim, entropy
};
static std::string views(int entry, const std::string& label, const ViewsArgs& a) {
    g_rec.clear();
    int rc = -1;
    const char* name = "?";
    switch (entry) {
        case V_PLAIN:
            name = "effi_warpcorr_views_f32";
            rc = effi_warpcorr_views_f32(a.ref, a.src, a.S, a.rt, a.depth, a.dds, a.dps, a.C, a.h, a.w, a.D, a.sim, a.ent, nullptr);
            break;
        case V_TBL:
            name = "effi_warpcorr_views_tbl_f32";
            rc = effi_warpcorr_views_tbl_f32(a.tbl, a.S, a.rt, a.depth, a.dds, a.dps, a.C, a.h, a.w, a.D, a.sim, a.ent, nullptr);
            break;
        case V_BATCH:
            name = "effi_warpcorr_views_f32_batch";
            rc = effi_warpcorr_views_f32_batch(a.ref, a.src, a.S, a.rt, a.depth, a.dds, a.dps, a.C, a.h, a.w, a.D, a.sim, a.ent, a.n_smp, a.ss[0],
                                               a.ss[1], a.ss[2], a.ss[3], a.ss[4], a.ss[5], nullptr);
            break;
        case V_X3:
            name = "effi_warpcorr_views_x3_f32";
            rc = effi_warpcorr_views_x3_f32(a.ref, a.src, a.S, a.rt, a.depth, a.dds, a.dps, a.C, a.h, a.w, a.D, a.sim, a.ent, a.hi_only, nullptr);
            break;
        case V_X3_TBL:
            name = "effi_warpcorr_views_x3_tbl_f32";
            rc = effi_warpcorr_views_x3_tbl_f32(a.tbl, a.S, a.rt, a.depth, a.dds, a.dps, a.C, a.h, a.w, a.D, a.sim, a.ent, a.hi_only, nullptr);
            break;
        case V_X3_BATCH:
            name = "effi_warpcorr_views_x3_f32_batch";
            rc = effi_warpcorr_views_x3_f32_batch(a.ref, a.src, a.S, a.rt, a.depth, a.dds, a.dps, a.C, a.h, a.w, a.D, a.sim, a.ent, a.hi_only,
                                                  a.n_smp, a.ss[0], a.ss[1], a.ss[2], a.ss[3], a.ss[4], a.ss[5], nullptr);
            break;
    }
    emit(name, is_batch(entry) ? label + L(" n_smp%d", a.n_smp) : label, rc);
    return g_rec;
}

struct ViewsBwdArgs : ViewsArgs {
    const float* gsim = P(24);
    float* gref = P(25);
    float* const* gsrc = GSRC;
};
static void views_bwd(const std::string& label, const ViewsBwdArgs& a) {
    RUNF(effi_warpcorr_views_bwd_f32, label, a.ref, a.src, a.S, a.rt, a.depth, a.dds, a.dps, a.C, a.h, a.w, a.D, a.gsim, a.gref, a.gsrc, nullptr);
}

struct HomoArgs {
    const float* src = P(2);
    const float* rt = P(20);
    const float* depth = P(21);
    long dds = 11, dps = 13;
    int C = 32, h = 37, w = 50, D = 5;
    float* out = P(26);                     // forward: the warped volume; backward: grad_src_nhwc
    const float* gout = P(27);
};
static void homo(bool bwd, const std::string& label, const HomoArgs& a) {
    if (bwd) RUNF(effi_homo_warp_bwd_f32, label, a.rt, a.depth, a.dds, a.dps, a.C, a.h, a.w, a.D, a.gout, a.out, nullptr);
    else RUNF(effi_homo_warp_f32, label, a.src, a.rt, a.depth, a.dds, a.dps, a.C, a.h, a.w, a.D, a.out, nullptr);
}

// the dynamic stage (stages 2 / 3): two forward entries and the backward behind one argument set
struct DynArgs {
    const float* ref = P(1);
    const float* const* src = SRC;
    const float* const* tbl = TBL;
    int S = 3;
    const float* rt = P(20);
    const float* cur = P(31);
    const float* itv = P(32);
    const float* vw = P(33);
    int vw_shift = 0, C = 8, h = 38, w = 50, D = 8;
    float* sim = P(34);
    float* smp = P(35);
    const float* gsim = P(24);              // backward only, from here on (sim is its input)
    float* gref = P(25);
    float* const* gsrc = GSRC;
    double* gvw = P<double>(36);
};
enum DynEntry { D_PLAIN, D_TBL, D_BWD };
static void dyn(int entry, const std::string& label, const DynArgs& a) {
    if (entry == D_PLAIN)
        RUNF(effi_warpcorr_dyn_f32, label, a.ref, a.src, a.S, a.rt, a.cur, a.itv, a.vw, a.vw_shift, a.C, a.h, a.w, a.D, a.sim, a.smp, nullptr);
    else if (entry == D_TBL)
        RUNF(effi_warpcorr_dyn_tbl_f32, label, a.tbl, a.S, a.rt, a.cur, a.itv, a.vw, a.vw_shift, a.C, a.h, a.w, a.D, a.sim, a.smp, nullptr);
    else
        RUNF(effi_warpcorr_dyn_bwd_f32, label, a.ref, a.src, a.S, a.rt, a.cur, a.itv, a.vw, a.vw_shift, a.C, a.h, a.w, a.D, a.sim, a.gsim, a.gref,
             a.gsrc, a.gvw, nullptr);
}

// ---- the cases ---------------------------------------------------------------------------------------------------------------------
template <class A> static A with(A a, int C, long dps, int D) { a.C = C, a.dps = dps, a.D = D; return a; }

static void cases_views() {
    const ViewsArgs d;
    // the exact entries: window kernel (C = 32, shared hypotheses, D <= 256) or the gather kernel; a table; a sample batch
    for (int e : {V_PLAIN, V_TBL, V_BATCH}) {
        views(e, "C32 dps0 D48", d);
        for (long kb : {0L, 16L, 1000L, -1L}) {
            Opt o(EFFI_OPT_WARP_LDS_KB, kb);
            views(e, L("C32 dps0 D48 warp_lds_kb%ld", kb), d);
        }
        for (int D : {256, 257}) views(e, L("C32 dps0 D%d", D), with(d, 32, 0, D));
        views(e, "C32 dps13 D48", with(d, 32, 13, 48));
        for (int C : {16, 8, 24}) views(e, L("C%d dps0 D48", C), with(d, C, 0, 48));
        ViewsArgs a = d;
        a.h = 64, a.w = 96, a.S = EFFI_MAX_VIEWS;
        views(e, "C32 64x96 S12", a);
        a.C = 16;
        views(e, "C16 64x96 S12", a);
    }
    // the split-precision entries: matrix-core kernel (bf16 x 3 or plain bf16 operands), else the exact launcher
    for (int e : {V_X3, V_X3_TBL, V_X3_BATCH})
        for (int hi : {0, 1}) {
            ViewsArgs a = d;
            a.hi_only = hi;
            views(e, L("hi_only%d C32 dps0 D48", hi), a);
            if (hi) continue;
            {
                Opt o(EFFI_OPT_WARP_LDS_KB, -1);
                views(e, "C32 dps0 D48 warp_lds_kb-1", a);
            }
            views(e, "C32 dps0 D256", with(a, 32, 0, 256));
            views(e, "C16: exact", with(a, 16, 0, 48));
            views(e, "C8: exact", with(a, 8, 0, 48));
            views(e, "C24: exact", with(a, 24, 0, 48));
            views(e, "dps13: exact", with(a, 32, 13, 48));
            views(e, "D257: exact", with(a, 32, 0, 257));
            a.h = 32000, a.w = 18;
            views(e, "h32000: exact", a);
            a.h = 31999;
            views(e, "h31999", a);
            a.h = 18, a.w = 32000;
            views(e, "w32000: exact", a);
            a.w = 31999;
            views(e, "w31999", a);
        }
    // one sample in a batch entry: the unbatched launch, the strides unused
    for (int x3 : {0, 1}) {
        ViewsArgs a = d;
        a.n_smp = 1;
        for (int gather : {0, 1}) {
            if (gather) a.dps = 13;
            const std::string one = views(x3 ? V_X3_BATCH : V_BATCH, gather ? "C32 dps13 D48" : "C32 dps0 D48", a);
            const std::string plain = views(x3 ? V_X3 : V_PLAIN, gather ? "C32 dps13 D48 (again)" : "C32 dps0 D48 (again)", a);
            if (one != plain || one.empty()) direct_failure(L("x3 %d gather %d: n_smp = 1 is not the unbatched launch", x3, gather));
        }
    }

    // refusals
    for (int e = 0; e < V_ENTRIES; ++e) {
        ViewsArgs a = d;
        if (is_tbl(e)) {
            a.tbl = nullptr;
            views(e, "null view_table_dev", a);
        } else {
            a.ref = nullptr;
            views(e, "null ref_nhwc", a);
            a = d, a.src = nullptr;
            views(e, "null src_nhwc", a);
            a = d, a.src = SRC_NULL1;
            views(e, "null src_nhwc[1]", a);
            a.S = 1;
            views(e, "null src_nhwc[1] past S", a);
        }
        a = d, a.rt = nullptr;
        views(e, "null rt", a);
        a = d, a.depth = nullptr;
        views(e, "null depth", a);
        a = d, a.sim = nullptr;
        views(e, "null sim_views", a);
        a = d, a.ent = nullptr;
        views(e, "null entropy", a);
        for (int S : {0, EFFI_MAX_VIEWS + 1}) {
            a = d, a.S = S;
            views(e, L("S%d", S), a);
        }
        a = d, a.h = 1;
        views(e, "h1", a);
        a = d, a.w = 1;
        views(e, "w1", a);
        a = d, a.D = 0;
        views(e, "D0", a);
        a = d, a.h = 2, a.w = 2, a.D = 1, a.S = 1;
        views(e, "2x2 D1 S1", a);
        if (!is_batch(e)) continue;
        for (int n : {0, 65536, 65535}) {
            a = d, a.n_smp = n;
            views(e, "samples", a);
        }
        for (int k = 0; k < 6; ++k) {
            a = d, a.ss[k] = -1;
            views(e, L("stride %d < 0", k), a);
            a.ss[k] = 0;
            views(e, L("stride %d = 0", k), a);
        }
    }
}

static void cases_views_bwd() {
    const ViewsBwdArgs d;
    views_bwd("C32 dps0 D48", d);
    for (long kb : {-1L, 0L, 16L}) {
        Opt o(EFFI_OPT_WARP_LDS_KB, kb);
        views_bwd(L("C32 dps0 D48 warp_lds_kb%ld", kb), d);
    }
    for (int D : {256, 257}) views_bwd(L("C32 dps0 D%d", D), with(d, 32, 0, D));
    views_bwd("C32 dps13 D48", with(d, 32, 13, 48));
    for (int C : {16, 8, 24}) views_bwd(L("C%d dps0 D48", C), with(d, C, 0, 48));
    ViewsBwdArgs a = d;
    a.h = 64, a.w = 96, a.S = EFFI_MAX_VIEWS;
    views_bwd("C32 64x96 S12", a);
    a.C = 8;
    views_bwd("C8 64x96 S12", a);

    a = d, a.ref = nullptr;
    views_bwd("null ref_nhwc", a);
    a = d, a.src = nullptr;
    views_bwd("null src_nhwc", a);
    a = d, a.src = SRC_NULL1;
    views_bwd("null src_nhwc[1]", a);
    a = d, a.rt = nullptr;
    views_bwd("null rt", a);
    a = d, a.depth = nullptr;
    views_bwd("null depth", a);
    a = d, a.gsim = nullptr;
    views_bwd("null grad_sim", a);
    a = d, a.gref = nullptr;
    views_bwd("null grad_ref_nhwc", a);
    a = d, a.gsrc = nullptr;
    views_bwd("null grad_src_nhwc", a);
    a = d, a.gsrc = GSRC_NULL1;
    views_bwd("null grad_src_nhwc[1]", a);
    a.S = 1;
    views_bwd("null grad_src_nhwc[1] past S", a);
    for (int S : {0, EFFI_MAX_VIEWS + 1}) {
        a = d, a.S = S;
        views_bwd(L("S%d", S), a);
    }
    a = d, a.h = 1;
    views_bwd("h1", a);
    a = d, a.w = 1;
    views_bwd("w1", a);
    a = d, a.D = 0;
    views_bwd("D0", a);
}

static void cases_homo() {
    const HomoArgs d;
    for (int bwd : {0, 1}) {
        for (int C : {32, 16, 8, 24}) {
            HomoArgs a = d;
            a.C = C;
            homo(bwd, L("C%d", C), a);
        }
        HomoArgs a = d;
        a.h = 2, a.w = 2, a.D = 1, a.dps = 0;
        homo(bwd, "2x2 D1", a);
        a = d, (bwd ? a.gout : a.src) = nullptr;
        homo(bwd, bwd ? "null grad_out" : "null src_nhwc", a);
        a = d, a.rt = nullptr;
        homo(bwd, "null rt", a);
        a = d, a.depth = nullptr;
        homo(bwd, "null depth", a);
        a = d, a.out = nullptr;
        homo(bwd, bwd ? "null grad_src_nhwc" : "null out", a);
        a = d, a.h = 1;
        homo(bwd, "h1", a);
        a = d, a.w = 1;
        homo(bwd, "w1", a);
        a = d, a.D = 0;
        homo(bwd, "D0", a);
    }
}

static void cases_dyn() {
    const DynArgs d;
    auto at = [&](int C, int D, int h = 38, int w = 50) {
        DynArgs a = d;
        a.C = C, a.D = D, a.h = h, a.w = w;
        return a;
    };
    for (int e : {D_PLAIN, D_TBL}) {
        // C = 8 / 16: the window kernel up to 8 hypotheses, the hypothesis-per-lane kernel beyond; C = 32: the channel-split form
        for (int C : {8, 16, 32, 24})
            for (int D : {2, 8, 9}) dyn(e, L("C%d D%d", C, D), at(C, D));
        for (long dw : {-1L, 0L, 64L})
            for (int C : {8, 16}) {
                Opt o(EFFI_OPT_DYN_WIN, dw);
                dyn(e, L("C%d D8 dyn_win%ld", C, dw), at(C, 8));
            }
        for (int C : {8, 16, 32}) {
            Opt o(EFFI_OPT_DYN_FORM, 1);
            dyn(e, L("C%d D8 dyn_form1", C), at(C, 8));
        }
        for (int C : {8, 16, 32, 24}) {
            Opt o(EFFI_OPT_DYN_SETUP_EXACT, 1);
            dyn(e, L("C%d D8 dyn_setup_exact1", C), at(C, 8));
            Opt o2(EFFI_OPT_DYN_FORM, 1);
            dyn(e, L("C%d D8 dyn_setup_exact1 dyn_form1", C), at(C, 8));
        }
        // the coordinate limit of the window kernel, the byte-offset limit of every fast form (nothing is allocated)
        dyn(e, "C8 D8 h32000", at(8, 8, 32000, 18));
        dyn(e, "C8 D8 h31999", at(8, 8, 31999, 18));
        dyn(e, "C16 D8 w32000", at(16, 8, 18, 32000));
        dyn(e, "C16 D8 w31999", at(16, 8, 18, 31999));
        dyn(e, "C8 D8 8192x8192: 2^31 bytes", at(8, 8, 8192, 8192));
        dyn(e, "C8 D8 8192x8191", at(8, 8, 8192, 8191));
        dyn(e, "C16 D9 8192x4096: 2^31 bytes", at(16, 9, 8192, 4096));
        dyn(e, "C16 D9 8191x4096", at(16, 9, 8191, 4096));
        dyn(e, "C32 D8 4096x4096: 2^31 bytes", at(32, 8, 4096, 4096));
        dyn(e, "C32 D8 4096x4095", at(32, 8, 4096, 4095));
        {
            Opt o(EFFI_OPT_DYN_FORM, 1);
            dyn(e, "C8 D8 8192x8192: 2^31 bytes dyn_form1", at(8, 8, 8192, 8192));
        }
        for (int shift : {0, 1, 4}) {
            DynArgs a = at(8, 8, 48, 64);
            a.vw_shift = shift, a.S = EFFI_MAX_VIEWS;
            dyn(e, L("C8 D8 48x64 S12 vw_shift%d", shift), a);
            a.C = 32;
            dyn(e, L("C32 D8 48x64 S12 vw_shift%d", shift), a);
        }
    }
    for (int C : {32, 16, 8, 24})
        for (int shift : {0, 2}) {
            DynArgs a = at(C, 8, 40, 52);
            a.vw_shift = shift;
            dyn(D_BWD, L("C%d D8 40x52 vw_shift%d", C, shift), a);
        }
    {
        DynArgs a = at(8, 2, 48, 64);
        a.vw_shift = 4, a.S = EFFI_MAX_VIEWS;
        dyn(D_BWD, "C8 D2 48x64 S12 vw_shift4", a);
    }

    // refusals
    for (int e : {D_PLAIN, D_TBL, D_BWD}) {
        DynArgs a = d;
        if (e == D_TBL) {
            a.tbl = nullptr;
            dyn(e, "null view_table_dev", a);
        } else {
            a.ref = nullptr;
            dyn(e, "null ref_nhwc", a);
            a = d, a.src = nullptr;
            dyn(e, "null src_nhwc", a);
            a = d, a.src = SRC_NULL1;
            dyn(e, "null src_nhwc[1]", a);
        }
        a = d, a.rt = nullptr;
        dyn(e, "null rt", a);
        a = d, a.cur = nullptr;
        dyn(e, "null cur_depth", a);
        a = d, a.itv = nullptr;
        dyn(e, "null interval", a);
        a = d, a.vw = nullptr;
        dyn(e, "null view_w", a);
        a = d, a.sim = nullptr;
        dyn(e, "null sim", a);
        if (e == D_BWD) {
            a = d, a.gsim = nullptr;
            dyn(e, "null grad_sim", a);
            a = d, a.gref = nullptr;
            dyn(e, "null grad_ref_nhwc", a);
            a = d, a.gsrc = nullptr;
            dyn(e, "null grad_src_nhwc", a);
            a = d, a.gsrc = GSRC_NULL1;
            dyn(e, "null grad_src_nhwc[1]", a);
            a = d, a.gvw = nullptr;
            dyn(e, "null grad_view_w", a);
        } else {
            a = d, a.smp = nullptr;
            dyn(e, "null samples", a);
        }
        for (int S : {0, EFFI_MAX_VIEWS + 1}) {
            a = d, a.S = S;
            dyn(e, L("S%d", S), a);
        }
        a = d, a.h = 1;
        dyn(e, "h1", a);
        a = d, a.w = 1;
        dyn(e, "w1", a);
        a = d, a.D = 1;
        dyn(e, "D1", a);
        for (int shift : {-1, 5}) {
            a = d, a.h = 64, a.w = 64, a.vw_shift = shift;
            dyn(e, L("64x64 vw_shift%d", shift), a);
        }
        a = d, a.h = 40, a.w = 48, a.vw_shift = 4;
        dyn(e, "40x48 vw_shift4", a);
        a.h = 48, a.w = 40;
        dyn(e, "48x40 vw_shift4", a);
        a.vw_shift = 3;
        dyn(e, "48x40 vw_shift3", a);
    }
}

static void cases_table() {
    const void* ptrs[EFFI_VIEW_TABLE_MAX + 1];
    for (int i = 0; i <= EFFI_VIEW_TABLE_MAX; ++i) ptrs[i] = P(100 + i);
    const void** const table = P<const void*>(90);
    for (int n : {1, 14, EFFI_VIEW_TABLE_MAX, 0, EFFI_VIEW_TABLE_MAX + 1}) RUNF(effi_view_table_set, L("n%d", n), table, ptrs, n, nullptr);
    RUNF(effi_view_table_set, "null table_dev", nullptr, ptrs, 1, nullptr);
    RUNF(effi_view_table_set, "null ptrs", table, nullptr, 1, nullptr);
}

int main() {
    for (long& v : g_opt) v = EFFI_OPT_UNSET;
    cases_views();
    cases_views_bwd();
    cases_homo();
    cases_dyn();
    cases_table();
    if (g_failures) std::printf("warp host check: %d FAILED\n", g_failures);
    return g_failures ? 1 : 0;
}
