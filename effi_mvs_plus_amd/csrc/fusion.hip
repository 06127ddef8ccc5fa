// Scope row n3: the dynamic geometric-consistency filter and depth averaging that consume the
// path's depth maps (reference: misc/fusion.py:8-46,117-181 and the tensor part of test_tank.py:466-512).
// One thread per reference pixel walks all source views: project into the source view, bilinear-sample its depth
// (F.grid_sample, align_corners=True, zero padding), project the sampled point back, compare position and depth against
// the V+1-thres_view threshold pairs, count, and finish with the averaged depth, the dynamic view-count rule, the
// photometric mask and the world-space point -- nothing of the reference's [n,v,3,h,w] intermediates is materialised
// unless the caller asks for reproj_xyd.  Arithmetic is fp32 in the reference's operation order; the 3x3 / 4x4 inverses
// are formed once per view on the device in fp64 and rounded (torch.inverse in fp32 differs from that by ~1e-7 relative).
//
// The file holds three fused filters -- this dynamic one, the fixed-threshold one of the same module and the DTU driver's -- and each
// is ONE kernel (fusion_filter_kernel over FusDynamic / FusStatic / FusDtu) for both launch forms: a scan launch addresses its views
// through a pair table, a single view is one row without a table (FusRows); the filter kernel is compiled once per form, the two
// view-prepare kernels choose per launch.  The six entry points are thin wrappers over one fus_*_impl per filter (end of the file).
#include "common.hpp"

namespace {

constexpr int FUS_MAX_VIEWS = 16;
constexpr int MAT_STRIDE = 52;        // per view: K[9] Kinv[9] E[16] Einv[16] (+2 pad)

__device__ void fus_invert(const double* A, int n, double* inv) {           // Gauss-Jordan, partial pivoting, n <= 4
    double M[4][8];
    for (int r = 0; r < n; ++r)
        for (int c = 0; c < n; ++c) {
            M[r][c] = A[r * n + c];
            M[r][c + n] = (r == c) ? 1.0 : 0.0;
        }
    for (int col = 0; col < n; ++col) {
        int piv = col;
        double best = fabs(M[col][col]);
        for (int r = col + 1; r < n; ++r)
            if (fabs(M[r][col]) > best) { best = fabs(M[r][col]); piv = r; }
        if (piv != col)
            for (int c = 0; c < 2 * n; ++c) { const double t = M[col][c]; M[col][c] = M[piv][c]; M[piv][c] = t; }
        const double d = 1.0 / M[col][col];
        for (int c = 0; c < 2 * n; ++c) M[col][c] *= d;
        for (int r = 0; r < n; ++r) {
            if (r == col) continue;
            const double f = M[r][col];
            for (int c = 0; c < 2 * n; ++c) M[r][c] -= f * M[col][c];
        }
    }
    for (int r = 0; r < n; ++r)
        for (int c = 0; c < n; ++c) inv[r * n + c] = M[r][c + n];
}

// one view's K[9] Kinv[9] E[16] Einv[16] from its camera [2][4][4] (extrinsic, intrinsic in the top-left 3x3)
__device__ void fus_prepare_view(const float* __restrict__ cam, float* __restrict__ m) {
    double K[9], Ki[9], E[16], Ei[16];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) K[r * 3 + c] = (double)cam[16 + r * 4 + c];
    for (int i = 0; i < 16; ++i) E[i] = (double)cam[i];
    fus_invert(K, 3, Ki);
    fus_invert(E, 4, Ei);
    for (int i = 0; i < 9; ++i) { m[i] = (float)K[i]; m[9 + i] = (float)Ki[i]; }
    for (int i = 0; i < 16; ++i) { m[18 + i] = (float)E[i]; m[34 + i] = (float)Ei[i]; }
}

// Pair table of a scan launch: row r = [reference id, source ids ..., -1 padding], 1 + v_max ints.  The entry points validate the
// HOST copy of the table (ids inside the scan, source counts, padding only at the end) before any kernel reads the device copy.
__device__ __forceinline__ int fus_row_sources(const int* __restrict__ row, int v_max) {
    int n = 0;
    while (n < v_max && row[1 + n] >= 0) ++n;
    return n;
}

// Where row r of a launch finds its views (depth maps, or cameras; ``stride`` = floats per view).  With a table (scan launch) the
// row's ids index one array of views, ref_base == src_base; without one (single view, one row) the reference is ref_base itself and
// the v_max sources are stacked at src_base.  Per-row data -- matrices [v_max+1][52], confidence, outputs -- follows row r - 1's in
// both forms.
struct FusRows {
    const float* ref_base;
    const float* src_base;
    const int* table;
    int v_max;
    __device__ __forceinline__ const int* row(int r) const { return table ? table + (long)r * (v_max + 1) : nullptr; }   // null: single view
    __device__ __forceinline__ const float* ref(const int* row, long stride) const { return row ? ref_base + (long)row[0] * stride : ref_base; }
    __device__ __forceinline__ const float* src(const int* row, int s, long stride) const {
        return src_base + (long)(row ? row[1 + s] : s) * stride;
    }
};

// mats [n_rows][v_max+1][52], one thread per (row, slot): cameras [2][4][4] (extrinsic, intrinsic in the top-left 3x3); slots past a
// row's source count stay unwritten
__global__ void fusion_prepare_kernel(FusRows cams, int n_rows, float* __restrict__ mats) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rows * (cams.v_max + 1)) return;
    const int r = i / (cams.v_max + 1), v = i - r * (cams.v_max + 1);
    const int* row = cams.row(r);
    if (row && row[v] < 0) return;
    fus_prepare_view(v == 0 ? cams.ref(row, 32) : cams.src(row, v - 1, 32), mats + (long)i * MAT_STRIDE);
}

struct V3 { float x, y, z; };
struct V4 { float x, y, z, w; };

__device__ __forceinline__ V3 mul3(const float* M, V3 p) {
    return {M[0] * p.x + M[1] * p.y + M[2] * p.z, M[3] * p.x + M[4] * p.y + M[5] * p.z, M[6] * p.x + M[7] * p.y + M[8] * p.z};
}
__device__ __forceinline__ V4 mul4(const float* M, V4 p) {
    return {M[0] * p.x + M[1] * p.y + M[2] * p.z + M[3] * p.w, M[4] * p.x + M[5] * p.y + M[6] * p.z + M[7] * p.w,
            M[8] * p.x + M[9] * p.y + M[10] * p.z + M[11] * p.w, M[12] * p.x + M[13] * p.y + M[14] * p.z + M[15] * p.w};
}
// The reference divides every component by the same denominator.  On the way INTO the source view (up to the bilinear sample,
// whose floor() is discontinuous) the quotients are formed exactly as the reference does; on the way BACK the denominator is
// inverted once (IEEE division) and the components are multiplied (<= 1 ulp per component, continuous outputs only), which
// removes 12 of the 27 division sequences per pixel and source view -- the kernel is bound by them.
// idx_img2cam (misc/fusion.py:23-28): K^-1 [u v 1], normalised by its z (+1e-9), times depth; homogeneous w = 1
template <bool EXACT>
__device__ __forceinline__ V4 img2cam(const float* Kinv, float u, float v, float depth) {
    V3 c = mul3(Kinv, {u, v, 1.0f});
    const float d = c.z + 1e-9f;
    if (EXACT) return {c.x / d * depth, c.y / d * depth, c.z / d * depth, 1.0f};
    const float r = 1.0f / d;
    return {c.x * r * depth, c.y * r * depth, c.z * r * depth, 1.0f};
}
// idx_cam2world / idx_world2cam (:31-40): 4x4 times the point, normalised by w (+1e-9)
template <bool EXACT>
__device__ __forceinline__ V4 xform(const float* M, V4 p) {
    V4 q = mul4(M, p);
    const float d = q.w + 1e-9f;
    if (EXACT) return {q.x / d, q.y / d, q.z / d, q.w / d};
    const float r = 1.0f / d;
    return {q.x * r, q.y * r, q.z * r, q.w * r};
}
// idx_cam2img (:43-47)
template <bool EXACT>
__device__ __forceinline__ V3 cam2img(const float* K, V4 c) {
    const float d = c.w + 1e-9f;
    if (EXACT) {
        V3 i = mul3(K, {c.x / d, c.y / d, c.z / d});
        const float e = i.z + 1e-9f;
        return {i.x / e, i.y / e, i.z / e};
    }
    const float r = 1.0f / d;
    V3 i = mul3(K, {c.x * r, c.y * r, c.z * r});
    const float e = 1.0f / (i.z + 1e-9f);
    return {i.x * e, i.y * e, i.z * e};
}

__device__ __forceinline__ float sample_bilinear_zero(const float* __restrict__ img, int h, int w, float u, float v) {
    // F.grid_sample(mode=bilinear, padding_mode=zeros, align_corners=True) on coordinates normalised as the reference does
    const float gx = u / ((float)(w - 1) / 2.0f) - 1.0f, gy = v / ((float)(h - 1) / 2.0f) - 1.0f;
    const float ix = ((gx + 1.0f) / 2.0f) * (float)(w - 1), iy = ((gy + 1.0f) / 2.0f) * (float)(h - 1);
    const float fx = floorf(ix), fy = floorf(iy);
    const int x0 = (int)fx, y0 = (int)fy;
    const float tx = ix - fx, ty = iy - fy;
    auto at = [&](int yy, int xx) { return (yy >= 0 && yy < h && xx >= 0 && xx < w) ? img[(long)yy * w + xx] : 0.0f; };
    const float nw = (1.0f - tx) * (1.0f - ty), ne = tx * (1.0f - ty), sw = (1.0f - tx) * ty, se = tx * ty;
    return at(y0, x0) * nw + at(y0, x0 + 1) * ne + at(y0 + 1, x0) * sw + at(y0 + 1, x0 + 1) * se;
}

// What a filter launch reads and writes per row besides the depth maps.  The kernel moves the pointers to its row (to_row), so a
// pixel function sees the reference view's own, as it does the depth maps (``src_of(s)`` = depth map of its s-th source).
struct FusIO {
    const float* __restrict__ conf;             // [ch][cw] (DTU: [h][w]) or null
    int ch, cw;
    float prob_thr;
    float* __restrict__ out_depth;              // [h][w]
    unsigned char *__restrict__ out_geo, *__restrict__ out_prob, *__restrict__ out_mask;    // [h][w] or null; DTU: prob = photometric, mask = final
    float* __restrict__ out_points;             // [3][h][w] or null
    float *__restrict__ out_xyd, *__restrict__ out_in_range;       // [V][3][h][w], [V][h][w] or null: single view only, the scan entries pass null

    __device__ __forceinline__ void to_row(int r, long hw) {
        if (conf) conf += (long)r * ch * cw;
        out_depth += r * hw;
        if (out_geo) out_geo += r * hw;
        if (out_prob) out_prob += r * hw;
        if (out_mask) out_mask += r * hw;
        if (out_points) out_points += 3 * r * hw;
    }

    // The end of the dynamic and the fixed-threshold pixel: photometric mask, the stores, the averaged depth as a world point.
    __device__ __forceinline__ void finish(int p, int h, int w, const float* Mr, float davg, bool geo) const {
        const long hw = (long)h * w;
        const int y = p / w, x = p - y * w;
        const float u = (float)x + 0.5f, vv = (float)y + 0.5f;
        bool pm = true;
        if (conf) {                                                     // F.interpolate(nearest) of the confidence, test_tank.py:471-473
            const int sy = min((int)floorf((float)y * ((float)ch / (float)h)), ch - 1);
            const int sx = min((int)floorf((float)x * ((float)cw / (float)w)), cw - 1);
            pm = conf[(long)sy * cw + sx] > prob_thr;
        }
        out_depth[p] = davg;
        if (out_geo) out_geo[p] = geo ? 1 : 0;
        if (out_prob) out_prob[p] = pm ? 1 : 0;
        if (out_mask) out_mask[p] = (geo & pm) ? 1 : 0;
        if (out_points) {                                               // :507-509 / :513-515
            const V4 pc = img2cam<true>(Mr + 9, u, vv, davg);
            const V4 pw = xform<true>(Mr + 34, pc);
            out_points[p] = pw.x;
            out_points[hw + p] = pw.y;
            out_points[2 * hw + p] = pw.z;
        }
    }
};

// One kernel for every filter and both launch forms: blockIdx.y = row r (one row for a single view), so no workgroup straddles two
// reference views, and ``Filter::pixel`` is the filter of ONE reference pixel p.  A scan launch reads maps [n_views][h][w] in place
// through the table's ids; conf [n_rows][ch][cw]; outputs [n_rows][h][w] / points [n_rows][3][h][w].  ``Filter::kMinWaves`` is the
// occupancy the register allocator has to keep where it would not by itself: the single view of the fixed-threshold filter takes
// 101 scalar registers without it (7 waves per SIMD, not 8); the DTU filter keeps its 4 waves without it as the code stands, but one
// more live offset in this kernel has put it at 149 vector registers (3 waves), so it names them; the dynamic one asks nothing.  ``TABLE`` is the
// launch form the kernel is compiled for (fus_run picks the instance): with the choice made per launch instead, the source
// loop of a single view loses its running pointer and holds the scalars of both forms, which cost the dynamic and the DTU filter
// more than their run-to-run spread (profiles/fusion_unify_ab.txt).
template <class Filter, bool TABLE>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(Filter::kMinWaves))) void fusion_filter_kernel(
    FusRows maps, int h, int w, const float* __restrict__ mats, Filter f) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    const long hw = (long)h * w;
    if (p >= hw) return;
    const int r = TABLE ? blockIdx.y : 0;                          // a single view is one row
    const int* row = TABLE ? maps.row(r) : nullptr;
    f.to_row(r, hw);
    if (TABLE) f.out_xyd = f.out_in_range = nullptr;                // single-view outputs: the scan entries pass null
    mats += (long)r * (maps.v_max + 1) * MAT_STRIDE;
    f.pixel(p, maps.ref(row, hw), [=](int s) { return maps.src(row, s, hw); }, TABLE ? fus_row_sources(row, maps.v_max) : maps.v_max, h, w,
            mats);
}

// The dynamic filter: thresholds i / dist_base and i / rel_base for i = dh .. V
struct FusDynamic : FusIO {
    static constexpr int kMinWaves = 1;
    int dh;
    float dist_base, rel_base;
    int relative;
    template <class SrcOf>
    __device__ void pixel(int p, const float* __restrict__ ref_depth, SrcOf src_of, int V, int h, int w,
                          const float* __restrict__ mats) const;
};

template <class SrcOf>
__device__ __forceinline__ void FusDynamic::pixel(int p, const float* __restrict__ ref_depth, SrcOf src_of, int V, int h, int w,
                                                  const float* __restrict__ mats) const {
    const long hw = (long)h * w;
    const int y = p / w, x = p - y * w;
    const float u = (float)x + 0.5f, vv = (float)y + 0.5f;
    const float* Mr = mats;
    const float dref = ref_depth[p];
    const V4 ref_cam_pt = img2cam<true>(Mr + 9, u, vv, dref);
    const V4 world = xform<true>(Mr + 34, ref_cam_pt);
    int counts[FUS_MAX_VIEWS + 1];
#pragma unroll
    for (int i = 0; i <= FUS_MAX_VIEWS; ++i) counts[i] = 0;
    const int nthr = V + 1 - dh;                                   // thresholds i = dh .. V
    float dsum = 0.0f;
    int nvis = 0;
    for (int s = 0; s < V; ++s) {
        const float* Ms = mats + (long)(s + 1) * MAT_STRIDE;
        const V4 c = xform<true>(Ms + 18, world);
        const V3 im = cam2img<true>(Ms, c);
        const float ds = sample_bilinear_zero(src_of(s), h, w, im.x, im.y);
        const V4 sc = img2cam<false>(Ms + 9, im.x, im.y, ds);
        const V4 sw = xform<false>(Ms + 34, sc);
        const V4 rc = xform<false>(Mr + 18, sw);
        const float reproj_depth = rc.z;
        const V3 ri = cam2img<false>(Mr, rc);
        if (out_xyd) {
            out_xyd[((long)s * 3 + 0) * hw + p] = ri.x;
            out_xyd[((long)s * 3 + 1) * hw + p] = ri.y;
            out_xyd[((long)s * 3 + 2) * hw + p] = reproj_depth;
        }
        const float dx = ri.x - u, dy = ri.y - vv;
        const float cdiff = sqrtf(dx * dx + dy * dy);
        float ddiff = fabsf(dref - reproj_depth);
        if (relative) ddiff = ddiff / dref;
#pragma unroll
        for (int k = 0; k <= FUS_MAX_VIEWS; ++k) {
            if (k < nthr) {
                const float step = (float)(dh + k);
                const bool m = (cdiff < step / dist_base) & (ddiff < step / rel_base);
                counts[k] += m ? 1 : 0;
                if (k == nthr - 1 && m) {                           // vis_mask = loosest threshold (misc/fusion.py:179)
                    dsum += reproj_depth;
                    nvis += 1;
                }
            }
        }
    }
    const float davg = (dsum + dref) / (float)(nvis + 1);           // test_tank.py:498-499
    bool geo = nvis >= V + 1;                                        // :502 (never true; kept for fidelity)
#pragma unroll
    for (int k = 0; k <= FUS_MAX_VIEWS; ++k)
        if (k < nthr && k < V + 1 - dh) geo = geo | (counts[k] >= dh + k);   // :503-504
    finish(p, h, w, Mr, davg, geo);
}

// ------------------------------------------------------------------------------------------------------------------------
// The FIXED-threshold visibility filter of the same module (Vis-MVSNet's): project_img, get_reproj, vis_filter, ave_fusion
// (misc/fusion.py:50-65,79-115).  The reference first maps every SOURCE pixel q into the reference view, S(q) = (x, y of the image
// point, z of the reference-camera point), then samples that [3,h,w] map at the reference pixel's projection into the source view
// (project_img).  Here one thread per reference pixel evaluates S only at the four taps its sample touches, from the four source
// depths, so the [v,3,h,w] map never exists.  The reference's oddities are kept: the projection is normalised by the size
// (u / w * 2 - 1, not w - 1) and clamped to +-1.1 while grid_sample runs with align_corners=True, the centres are (x+0.5, y+0.5),
// in_range does not enter vis_filter's result.

// project_img's warp coordinate of one destination pixel (:53-63) and grid_sample's tap set-up (bilinear, zeros, align_corners=True)
struct StaticTaps {
    int x0, y0;
    float nw, ne, sw, se;       // weights of (y0,x0) (y0,x0+1) (y0+1,x0) (y0+1,x0+1)
    float in_range;             // 0/1 on the clamped coordinates (:62)
};
__device__ __forceinline__ StaticTaps fus_static_taps(const float* Md, const float* Ms, float u, float vv, float depth, int height,
                                                      int width, int hs, int ws) {
    const V4 cp = img2cam<true>(Md + 9, u, vv, depth);
    const V4 world = xform<true>(Md + 34, cp);
    const V4 c = xform<true>(Ms + 18, world);
    const V3 im = cam2img<true>(Ms, c);
    float gx = im.x / (float)width * 2.0f - 1.0f, gy = im.y / (float)height * 2.0f - 1.0f;     // :59-61
    gx = gx < -1.1f ? -1.1f : (gx > 1.1f ? 1.1f : gx);
    gy = gy < -1.1f ? -1.1f : (gy > 1.1f ? 1.1f : gy);
    StaticTaps t;
    t.in_range = (-1.0f <= gx && gx <= 1.0f && -1.0f <= gy && gy <= 1.0f) ? 1.0f : 0.0f;
    const float ix = ((gx + 1.0f) / 2.0f) * (float)(ws - 1), iy = ((gy + 1.0f) / 2.0f) * (float)(hs - 1);
    const float fx = floorf(ix), fy = floorf(iy);
    t.x0 = (fx == fx) ? (int)fx : -2;                                // a NaN coordinate touches no tap
    t.y0 = (fy == fy) ? (int)fy : -2;
    const float tx = ix - fx, ty = iy - fy;
    t.nw = (1.0f - tx) * (1.0f - ty);
    t.ne = tx * (1.0f - ty);
    t.sw = (1.0f - tx) * ty;
    t.se = tx * ty;
    return t;
}

// S(q) of one source pixel (get_reproj, :87-91), zero outside the map as grid_sample's padding makes it.  Continuous outputs: the
// reciprocal forms.
__device__ __forceinline__ V3 fus_static_tap(const float* Mr, const float* Ms, const float* __restrict__ src, int h, int w, int yy, int xx) {
    if (yy < 0 || yy >= h || xx < 0 || xx >= w) return {0.0f, 0.0f, 0.0f};
    const V4 sc = img2cam<false>(Ms + 9, (float)xx + 0.5f, (float)yy + 0.5f, src[(long)yy * w + xx]);
    const V4 sw = xform<false>(Ms + 34, sc);
    const V4 rc = xform<false>(Mr + 18, sw);
    const V3 ri = cam2img<false>(Mr, rc);
    return {ri.x, ri.y, rc.z};
}

// vis_filter's two tests of one (view, pixel) (:102,105): thresholds are the fp32 roundings of 1/img_dist_thresh, 1/depth_thresh
__device__ __forceinline__ float fus_static_test(float u, float vv, float dref, float x, float y, float d, float dist_thr, float depth_thr) {
    const float dx = x - u, dy = y - vv;
    const float dist = sqrtf(dx * dx + dy * dy), ddiff = fabsf(dref - d);
    const bool m = (dist < dist_thr) & (ddiff < depth_thr);
    return m ? 1.0f : 0.0f;
}

// The fixed-threshold filter: thresholds as fus_static_thresholds (below) rounds them
struct FusStatic : FusIO {
    static constexpr int kMinWaves = 8;
    float dist_thr, depth_thr, count_thr;
    template <class SrcOf>
    __device__ void pixel(int p, const float* __restrict__ ref_depth, SrcOf src_of, int V, int h, int w,
                          const float* __restrict__ mats) const;
};

template <class SrcOf>
__device__ __forceinline__ void FusStatic::pixel(int p, const float* __restrict__ ref_depth, SrcOf src_of, int V, int h, int w,
                                                 const float* __restrict__ mats) const {
    const long hw = (long)h * w;
    const int y = p / w, x = p - y * w;
    const float u = (float)x + 0.5f, vv = (float)y + 0.5f;
    const float* Mr = mats;
    const float dref = ref_depth[p];
    float dsum = 0.0f, msum = 0.0f;
    for (int s = 0; s < V; ++s) {
        const float* Ms = mats + (long)(s + 1) * MAT_STRIDE;
        const float* src = src_of(s);
        const StaticTaps t = fus_static_taps(Mr, Ms, u, vv, dref, h, w, h, w);
        const V3 a = fus_static_tap(Mr, Ms, src, h, w, t.y0, t.x0), b = fus_static_tap(Mr, Ms, src, h, w, t.y0, t.x0 + 1);
        const V3 c = fus_static_tap(Mr, Ms, src, h, w, t.y0 + 1, t.x0), e = fus_static_tap(Mr, Ms, src, h, w, t.y0 + 1, t.x0 + 1);
        const float rx = a.x * t.nw + b.x * t.ne + c.x * t.sw + e.x * t.se;
        const float ry = a.y * t.nw + b.y * t.ne + c.y * t.sw + e.y * t.se;
        const float rd = a.z * t.nw + b.z * t.ne + c.z * t.sw + e.z * t.se;
        if (out_xyd) {
            out_xyd[((long)s * 3 + 0) * hw + p] = rx;
            out_xyd[((long)s * 3 + 1) * hw + p] = ry;
            out_xyd[((long)s * 3 + 2) * hw + p] = rd;
        }
        if (out_in_range) out_in_range[(long)s * hw + p] = t.in_range;
        const float m = fus_static_test(u, vv, dref, rx, ry, rd, dist_thr, depth_thr);
        dsum = dsum + rd * m;                                       // ave_fusion (:114): the product, in view order
        msum = msum + m;
    }
    const float davg = (dsum + dref) / (msum + 1.0f);
    const bool geo = msum >= count_thr;                             // :109, count_thr = (float)(vthresh - 1.1)
    finish(p, h, w, Mr, davg, geo);
}

// mats [n][2][52]: slot 2b = destination camera b, slot 2b + 1 = source camera b
__global__ void fusion_prepare_pairs_kernel(const float* __restrict__ dst_cams, const float* __restrict__ src_cams, int n,
                                            float* __restrict__ mats) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 2 * n) return;
    fus_prepare_view(((i & 1) ? src_cams : dst_cams) + (long)(i >> 1) * 32, mats + (long)i * MAT_STRIDE);
}

// project_img (:50-65) for any channel count: blockIdx.y = batch element, mats [n][2][52] = destination camera, source camera.
// src_img [n][C][hs][ws], dst_depth [n][height][width] -> out [n][C][height][width], in_range [n][height][width]; the weights are
// computed once, the channels loop over them.
__global__ __launch_bounds__(256) void fusion_project_img_kernel(const float* __restrict__ src_img, const float* __restrict__ dst_depth,
                                                                 const float* __restrict__ mats, int C, int hs, int ws, int height,
                                                                 int width, float* __restrict__ out, float* __restrict__ in_range) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    const long hw = (long)height * width, shw = (long)hs * ws;
    if (p >= hw) return;
    const int b = blockIdx.y;
    const int y = p / width, x = p - y * width;
    const float* Md = mats + (long)b * 2 * MAT_STRIDE;
    const StaticTaps t = fus_static_taps(Md, Md + MAT_STRIDE, (float)x + 0.5f, (float)y + 0.5f, dst_depth[b * hw + p], height, width, hs, ws);
    if (in_range) in_range[b * hw + p] = t.in_range;
    const bool x0in = t.x0 >= 0 && t.x0 < ws, x1in = t.x0 + 1 >= 0 && t.x0 + 1 < ws;
    const bool y0in = t.y0 >= 0 && t.y0 < hs, y1in = t.y0 + 1 >= 0 && t.y0 + 1 < hs;
    const long o00 = (long)t.y0 * ws + t.x0;
    for (int c = 0; c < C; ++c) {
        const float* img = src_img + ((long)b * C + c) * shw;
        const float a = (y0in && x0in) ? img[o00] : 0.0f, bb = (y0in && x1in) ? img[o00 + 1] : 0.0f;
        const float cc = (y1in && x0in) ? img[o00 + ws] : 0.0f, e = (y1in && x1in) ? img[o00 + ws + 1] : 0.0f;
        out[((long)b * C + c) * hw + p] = a * t.nw + bb * t.ne + cc * t.sw + e * t.se;
    }
}

// vis_filter (:99-110) and ave_fusion (:113-115) on a GIVEN reproj_xyd [n][V][3][h][w], blockIdx.y = batch element: per pixel the
// loop over the views.  masks_in != NULL: ave_fusion with the caller's masks [n][V][h][w] (any values: the product is formed);
// otherwise the masks are vis_filter's and go to masks_out (0/1 floats) / mask_out (bytes) when asked for.
__global__ __launch_bounds__(256) void fusion_static_vis_kernel(const float* __restrict__ ref_depth, const float* __restrict__ xyd,
                                                                const float* __restrict__ masks_in, int V, int h, int w, float dist_thr,
                                                                float depth_thr, float count_thr, float* __restrict__ masks_out,
                                                                unsigned char* __restrict__ mask_out, float* __restrict__ ave_out) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    const long hw = (long)h * w;
    if (p >= hw) return;
    const int b = blockIdx.y;
    const int y = p / w, x = p - y * w;
    const float u = (float)x + 0.5f, vv = (float)y + 0.5f;
    const float dref = ref_depth[b * hw + p];
    float dsum = 0.0f, msum = 0.0f;
    for (int s = 0; s < V; ++s) {
        const float* q = xyd + ((long)b * V + s) * 3 * hw + p;
        const float rd = q[2 * hw];
        const float m = masks_in ? masks_in[((long)b * V + s) * hw + p] : fus_static_test(u, vv, dref, q[0], q[hw], rd, dist_thr, depth_thr);
        if (masks_out) masks_out[((long)b * V + s) * hw + p] = m;
        dsum = dsum + rd * m;
        msum = msum + m;
    }
    if (mask_out) mask_out[b * hw + p] = (msum >= count_thr) ? 1 : 0;
    if (ave_out) ave_out[b * hw + p] = (dsum + dref) / (msum + 1.0f);
}

// prob_filter (:68-76), one channel per launch: mask = (first ? 1 : mask) & (prob > thr); prob of batch element b at b * bstride
__global__ __launch_bounds__(256) void fusion_prob_filter_kernel(const float* __restrict__ prob, long bstride, long hw, float thr, int first,
                                                                 unsigned char* __restrict__ mask) {
    const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= hw) return;
    const int b = blockIdx.y;
    const unsigned char m = prob[b * bstride + p] > thr ? 1 : 0;
    mask[b * hw + p] = first ? m : (mask[b * hw + p] & m);
}

// ------------------------------------------------------------------------------------------------------------------------
// DTU branch of row n3: reproject_with_depth + check_geometric_consistency + the array part of filter_depth of the reference's
// test_dtu_dypcd.py:164-333 (the numpy / cv2 filter its DTU driver runs per scan on the host, in a multiprocessing pool), one thread
// per reference pixel walking the source views.  Differences from the Tanks-and-Temples kernel above that matter for parity: pixel
// coordinates are INTEGERS (no half-pixel offset), the projection chain is evaluated in DOUBLE (numpy promotes int64 grid x
// float32 depth to float64) and rounded to float32 exactly where the reference calls .astype(np.float32), the source depth is
// sampled with cv2.remap(INTER_LINEAR)'s arithmetic (coordinates rounded to 1/32 pixel, table weights, zero outside), and ten
// (distance, depth-difference) threshold pairs i = s .. e-1 are counted.  PARITY UNPINNED: cv2 is not installed in the build image
// and the reference holds no fixtures for this code; the checker is oracle/effi_dtu_filter_oracle.py (the numpy lines restated with
// their dtypes, OpenCV's published remap algorithm restated).  Matrix inverses / products are formed once per view in double and
// rounded to float32 (the reference: single-precision LAPACK / float32 matmul; ~1e-7 relative apart).
// per view: ref: K[9] Kinv[9] E[16] Einv[16]; source s: K[9] Kinv[9] T_ref->src[16] = E_s . E_ref^-1, T_src->ref[16] = E_ref . E_s^-1
__device__ __noinline__ void fus_dtu_prepare_view(const float* __restrict__ ref_cam, const float* __restrict__ src_cam, float* __restrict__ m) {
    auto load = [](const float* cam, double* K, double* E) {
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) K[r * 3 + c] = (double)cam[16 + r * 4 + c];
        for (int i = 0; i < 16; ++i) E[i] = (double)cam[i];
    };
    double K[9], Ki[9], E[16], Ei[16], Kr[9], Er[16], Eri[16];
    load(ref_cam, Kr, Er);
    fus_invert(Er, 4, Eri);
    if (!src_cam) {                                                         // the reference view's own slot
        fus_invert(Kr, 3, Ki);
        for (int i = 0; i < 9; ++i) { m[i] = (float)Kr[i]; m[9 + i] = (float)Ki[i]; }
        for (int i = 0; i < 16; ++i) { m[18 + i] = (float)Er[i]; m[34 + i] = (float)Eri[i]; }
        return;
    }
    load(src_cam, K, E);
    fus_invert(K, 3, Ki);
    fus_invert(E, 4, Ei);
    for (int i = 0; i < 9; ++i) { m[i] = (float)K[i]; m[9 + i] = (float)Ki[i]; }
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) {
            double a = 0.0, b = 0.0;
            for (int k = 0; k < 4; ++k) {
                a += (double)(float)E[r * 4 + k] * (double)(float)Eri[k * 4 + c];       // operands as float32, as the reference holds them
                b += (double)(float)Er[r * 4 + k] * (double)(float)Ei[k * 4 + c];
            }
            m[18 + r * 4 + c] = (float)a;
            m[34 + r * 4 + c] = (float)b;
        }
}

// layout and addressing as fusion_prepare_kernel: the per-pair products of every (reference, source) pair in one launch
__global__ void fusion_dtu_prepare_kernel(FusRows cams, int n_rows, float* __restrict__ mats) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rows * (cams.v_max + 1)) return;
    const int r = i / (cams.v_max + 1), v = i - r * (cams.v_max + 1);
    const int* row = cams.row(r);
    if (row && row[v] < 0) return;
    fus_dtu_prepare_view(cams.ref(row, 32), v == 0 ? nullptr : cams.src(row, v - 1, 32), mats + (long)i * MAT_STRIDE);
}

struct D3 { double x, y, z; };
__device__ __forceinline__ D3 dmul3(const float* M, double x, double y, double z) {
    return {(double)M[0] * x + (double)M[1] * y + (double)M[2] * z, (double)M[3] * x + (double)M[4] * y + (double)M[5] * z,
            (double)M[6] * x + (double)M[7] * y + (double)M[8] * z};
}
__device__ __forceinline__ D3 dmul4_xyz(const float* M, D3 p) {          // rows 0..2 of M . [p; 1]
    return {(double)M[0] * p.x + (double)M[1] * p.y + (double)M[2] * p.z + (double)M[3],
            (double)M[4] * p.x + (double)M[5] * p.y + (double)M[6] * p.z + (double)M[7],
            (double)M[8] * p.x + (double)M[9] * p.y + (double)M[10] * p.z + (double)M[11]};
}

// cv2.remap(src, map_x, map_y, INTER_LINEAR), BORDER_CONSTANT 0, one sample (OpenCV imgwarp.cpp: INTER_BITS = 5)
__device__ __forceinline__ float cv_remap_linear(const float* __restrict__ img, int h, int w, float mx, float my) {
    auto fix = [](float v) -> long {
        double f = (double)v * 32.0;
        if (!(f == f)) return -2147483648L;                    // NaN: cvRound gives INT_MIN
        f = fmin(fmax(f, -2147483648.0), 2147483647.0);
        return (long)rint(f);                                   // cvRound: round half to even
    };
    const long sx = fix(mx), sy = fix(my);
    const int ax = (int)(sx & 31), ay = (int)(sy & 31);
    const long x0 = min(max(sx >> 5, -32768L), 32767L), y0 = min(max(sy >> 5, -32768L), 32767L);      // saturate_cast<short>
    const float tx = (float)ax * (1.0f / 32.0f), ty = (float)ay * (1.0f / 32.0f);
    const float wx0 = 1.0f - tx, wy0 = 1.0f - ty;
    auto at = [&](long yy, long xx) { return (yy >= 0 && yy < h && xx >= 0 && xx < w) ? img[yy * w + xx] : 0.0f; };
    return at(y0, x0) * (wy0 * wx0) + at(y0, x0 + 1) * (wy0 * tx) + at(y0 + 1, x0) * (ty * wx0) + at(y0 + 1, x0 + 1) * (ty * tx);
}

constexpr int DTU_MAX_THR = 16;

// reproject_with_depth for ONE reference pixel and one source view (test_dtu_dypcd.py:164-205), shared by the fused filter kernel and
// the per-function kernel below: one arithmetic.
struct DtuReproj {
    float x_src, y_src, depth_rep, x_rep, y_rep;
};
__device__ __forceinline__ DtuReproj dtu_reproject_pixel(const float* __restrict__ Mr, const float* __restrict__ Ms,
                                                         const float* __restrict__ src_depth, int h, int w, double xd, double yd,
                                                         float dref) {
    // reference 3-D point: K_ref^-1 . ([x y 1] * depth)                                                     (:172-173)
    const D3 xyz_ref = dmul3(Mr + 9, xd * (double)dref, yd * (double)dref, (double)dref);
    const D3 xs = dmul4_xyz(Ms + 18, xyz_ref);                                                             // (:175-176)
    const D3 kx = dmul3(Ms, xs.x, xs.y, xs.z);                                                             // (:178-179)
    const double u = kx.x / kx.z, v = kx.y / kx.z;
    DtuReproj r;
    r.x_src = (float)u;                                                                                    // (:182-183)
    r.y_src = (float)v;
    const float samp = cv_remap_linear(src_depth, h, w, r.x_src, r.y_src);                                 // (:184)
    const D3 s3 = dmul3(Ms + 9, u * (double)samp, v * (double)samp, (double)samp);                         // (:190-191)
    const D3 rp = dmul4_xyz(Ms + 34, s3);                                                                  // (:193-194)
    r.depth_rep = (float)rp.z;                                                                             // (:196)
    D3 kr = dmul3(Mr, rp.x, rp.y, rp.z);                                                                   // (:197)
    if (kr.z == 0.0) kr.z += 0.00001;                                                                      // (:198)
    r.x_rep = (float)(kr.x / kr.z);                                                                        // (:199-201)
    r.y_rep = (float)(kr.y / kr.z);
    return r;
}

// Threshold pair i of check_geometric_consistency (:227), shared by the two DTU kernels: dist < i * dist_base in float64,
// depth_diff < math.log(max(i, 1.05), 10) * diff_base as a float32 comparison
struct DtuThr {
    double dist;
    float diff;
};
__device__ __forceinline__ DtuThr dtu_thresholds(int i, float dist_base, float diff_base) {
    return {(double)i * (double)dist_base, (float)(log(fmax((double)i, 1.05)) / log(10.0) * (double)diff_base)};
}

// The DTU filter: pairs i = s_lo .. e_hi - 1; conf [h][w], already at the depth size, prob_thr = the photometric threshold
struct FusDtu : FusIO {
    static constexpr int kMinWaves = 4;
    float conf_keep;
    int s_lo, e_hi;
    float dist_base, diff_base;
    template <class SrcOf>
    __device__ void pixel(int p, const float* __restrict__ ref_depth, SrcOf src_of, int V, int h, int w,
                          const float* __restrict__ mats) const;
};

template <class SrcOf>
__device__ __forceinline__ void FusDtu::pixel(int p, const float* __restrict__ ref_depth, SrcOf src_of, int V, int h, int w,
                                              const float* __restrict__ mats) const {
    const long hw = (long)h * w;
    const int y = p / w, x = p - y * w;
    const double xd = (double)x, yd = (double)y;
    const float* Mr = mats;
    const float dref = ref_depth[p];
    const int nthr = e_hi - s_lo;
    float thr_diff[DTU_MAX_THR];
    double thr_dist[DTU_MAX_THR];
    int counts[DTU_MAX_THR];
#pragma unroll
    for (int k = 0; k < DTU_MAX_THR; ++k) {
        const DtuThr t = dtu_thresholds(s_lo + k, dist_base, diff_base);
        counts[k] = 0;
        thr_dist[k] = t.dist;
        thr_diff[k] = t.diff;
    }
    float num = 0.0f;                          // sum(all_srcview_depth_ests): float32, in view order (:299)
    int nlast = 0;
    for (int sv = 0; sv < V; ++sv) {
        const float* Ms = mats + (long)(sv + 1) * MAT_STRIDE;
        const DtuReproj rr = dtu_reproject_pixel(Mr, Ms, src_of(sv), h, w, xd, yd, dref);     // (:164-205)
        const float depth_rep = rr.depth_rep, xr = rr.x_rep, yr = rr.y_rep;
        const double dxr = (double)xr - xd, dyr = (double)yr - yd;
        const double dist = sqrt(dxr * dxr + dyr * dyr);                                                       // (:218) float32 - int64 -> float64
        const float ddiff = fabsf(depth_rep - dref);                                                           // (:225)
        bool last = false;
#pragma unroll
        for (int k = 0; k < DTU_MAX_THR; ++k) {
            if (k < nthr) {
                const bool m = (dist < thr_dist[k]) & (ddiff < thr_diff[k]);
                counts[k] += m ? 1 : 0;
                if (k == nthr - 1) last = m;
            }
        }
        if (last) {                            // depth_reprojected[~mask] = 0 with mask = the LAST (loosest) pair (:229)
            num = num + depth_rep;
            nlast += 1;
        }
    }
    double davg = (double)(num + dref) / (double)(nlast + 1);                                                  // (:299) float32 / int -> float64
    const float c = conf ? conf[p] : 1.0f;
    if (c > conf_keep) davg = (double)dref;                                                                    // (:300)
    bool geo = nlast >= e_hi;                                                                                  // (:303) dy_range = e
#pragma unroll
    for (int k = 0; k < DTU_MAX_THR; ++k)
        if (k < nthr) geo = geo | (counts[k] >= s_lo + k);                                                     // (:304-305)
    const bool photo = c > prob_thr;                                                                           // (:261)
    out_depth[p] = (float)davg;
    if (out_prob) out_prob[p] = photo ? 1 : 0;
    if (out_geo) out_geo[p] = geo ? 1 : 0;
    if (out_mask) out_mask[p] = (photo & geo) ? 1 : 0;
    if (out_points) {                                                                                          // (:327-330)
        const D3 pc = dmul3(Mr + 9, xd * davg, yd * davg, davg);
        const D3 pw = dmul4_xyz(Mr + 34, pc);
        out_points[p] = (float)pw.x;
        out_points[hw + p] = (float)pw.y;
        out_points[2 * hw + p] = (float)pw.z;
    }
}

// reproject_with_depth (test_dtu_dypcd.py:164-205) and, with ``masks``, check_geometric_consistency (:208-233) for one
// (reference, source) pair as functions of their own: out5 = depth_reprojected, x_reprojected, y_reprojected, x_src, y_src.
// With masks: masks[k] = dist < (s+k) * dist_base & depth_diff < log10(max(s+k, 1.05)) * diff_base, and the first three outputs are
// zeroed where the LAST mask is false (:229-231).  PARITY UNPINNED like the fused DTU kernel (cv2.remap restated).
__global__ __launch_bounds__(256) void fusion_dtu_reproject_kernel(const float* __restrict__ ref_depth, const float* __restrict__ src_depth,
                                                                   int h, int w, const float* __restrict__ mats, int s_lo, int e_hi,
                                                                   float dist_base, float diff_base, float* __restrict__ out5,
                                                                   unsigned char* __restrict__ masks) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    const long hw = (long)h * w;
    if (p >= hw) return;
    const int y = p / w, x = p - y * w;
    const double xd = (double)x, yd = (double)y;
    const float dref = ref_depth[p];
    DtuReproj r = dtu_reproject_pixel(mats, mats + MAT_STRIDE, src_depth, h, w, xd, yd, dref);
    if (masks) {
        const double dxr = (double)r.x_rep - xd, dyr = (double)r.y_rep - yd;
        const double dist = sqrt(dxr * dxr + dyr * dyr);
        const float ddiff = fabsf(r.depth_rep - dref);
        bool last = false;
        for (int k = 0; k < e_hi - s_lo; ++k) {
            const DtuThr t = dtu_thresholds(s_lo + k, dist_base, diff_base);
            last = (dist < t.dist) & (ddiff < t.diff);
            masks[(long)k * hw + p] = last ? 1 : 0;
        }
        if (!last) r.depth_rep = r.x_rep = r.y_rep = 0.0f;
    }
    out5[p] = r.depth_rep;
    out5[hw + p] = r.x_rep;
    out5[2 * hw + p] = r.y_rep;
    out5[3 * hw + p] = r.x_src;
    out5[4 * hw + p] = r.y_src;
}

// ------------------------------------------------------------------------------------------------------------------------
// The reference's misc/fusion.py functions the T&T driver calls ONE BY ONE (test_tank.py:486-509) -- vis_filter_dynamic and the
// idx_* point transforms -- as kernels of their own, so that the driver's lines run unchanged on this package.
// The fused kernel above remains the fast path (dynamic_filter); these reproduce the individual functions' outputs.

// vis_filter_dynamic (misc/fusion.py:157-181): masks[n][v][k][p] = |reproj_xy - pixel centre| < (thres+k)/dist_base  AND
// |ref_depth - reproj_depth| (/ ref_depth) < (thres+k)/rel_diff_base, k = 0 .. v - thres
__global__ __launch_bounds__(256) void fusion_vis_filter_kernel(const float* __restrict__ ref_depth, const float* __restrict__ xyd,
                                                                int V, int h, int w, float dist_base, float rel_base, int thres,
                                                                int relative, unsigned char* __restrict__ masks) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    const long hw = (long)h * w;
    if (p >= hw) return;
    const int b = blockIdx.y / V, s = blockIdx.y - b * V;
    const int y = p / w, x = p - y * w;
    const float u = (float)x + 0.5f, vv = (float)y + 0.5f;
    const float dref = ref_depth[(long)b * hw + p];
    const float* q = xyd + ((long)(b * V + s) * 3) * hw + p;
    const float dx = q[0] - u, dy = q[hw] - vv;
    const float cdiff = sqrtf(dx * dx + dy * dy);
    float ddiff = fabsf(dref - q[2 * hw]);
    if (relative) ddiff = ddiff / dref;
    const int nthr = V + 1 - thres;
    unsigned char* m = masks + ((long)(b * V + s) * nthr) * hw + p;
    for (int k = 0; k < nthr; ++k) {
        const float step = (float)(thres + k);
        m[(long)k * hw] = ((cdiff < step / dist_base) & (ddiff < step / rel_base)) ? 1 : 0;
    }
}

// one camera per batch element: K[9] Kinv[9] E[16] Einv[16]
__global__ void fusion_prepare_batch_kernel(const float* __restrict__ cams, int n, float* __restrict__ mats) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n) return;
    const float* cam = cams + (long)v * 32;
    double K[9], Ki[9], E[16], Ei[16];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) K[r * 3 + c] = (double)cam[16 + r * 4 + c];
    for (int i = 0; i < 16; ++i) E[i] = (double)cam[i];
    fus_invert(K, 3, Ki);
    fus_invert(E, 4, Ei);
    float* m = mats + (long)v * MAT_STRIDE;
    for (int i = 0; i < 9; ++i) { m[i] = (float)K[i]; m[9 + i] = (float)Ki[i]; }
    for (int i = 0; i < 16; ++i) { m[18 + i] = (float)E[i]; m[34 + i] = (float)Ei[i]; }
}

// MODE 0: idx_img2cam (:23-28)  in [..,3] (+ depth) -> out [..,4];  1: idx_cam2world (:31-34)  4 -> 4;
//      2: idx_world2cam (:37-40) 4 -> 4;                             3: idx_cam2img (:43-47)    4 -> 3
template <int MODE>
__global__ __launch_bounds__(256) void fusion_points_kernel(const float* __restrict__ in, long in_bstride, const float* __restrict__ depth,
                                                            const float* __restrict__ mats, int hw, float* __restrict__ out) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= hw) return;
    const int b = blockIdx.y;
    const float* M = mats + (long)b * MAT_STRIDE;
    constexpr int NI = (MODE == 0) ? 3 : 4, NO = (MODE == 3) ? 3 : 4;
    const float* q = in + (long)b * in_bstride + (long)p * NI;
    float* o = out + ((long)b * hw + p) * NO;
    if (MODE == 0) {
        const V3 c = mul3(M + 9, {q[0], q[1], q[2]});
        const float d = c.z + 1e-9f, dep = depth[(long)b * hw + p];
        o[0] = c.x / d * dep; o[1] = c.y / d * dep; o[2] = c.z / d * dep; o[3] = 1.0f;
    } else if (MODE == 1 || MODE == 2) {
        const V4 r = xform<true>(M + (MODE == 1 ? 34 : 18), {q[0], q[1], q[2], q[3]});
        o[0] = r.x; o[1] = r.y; o[2] = r.z; o[3] = r.w;
    } else {
        const V3 r = cam2img<true>(M, {q[0], q[1], q[2], q[3]});
        o[0] = r.x; o[1] = r.y; o[2] = r.z;
    }
}

// ------------------------------------------------------------------------------------------------------------------------
// Ordered compaction of a scan's survivors (the host side of test_dtu_dypcd.py:327-333 and test_tank.py:517-533: boolean indexing of
// the points and the reference image, view after view, then np.concatenate).  Vertex order = reference views in table order, row-major
// survivors within a view.  Three kernels and no atomics, so the arrays are bitwise reproducible: (1) survivors per workgroup
// (64-bit ballot popcount per wave, the waves combined through LDS), (2) one exclusive scan over the n_ref * blocks_per_view counts,
// which also leaves the per-view vertex ranges, (3) scatter: rank inside the wave from the ballot bits below the lane, plus the bases
// of the wave and of the workgroup.  A workgroup covers 256 consecutive pixels of ONE view (blockIdx.y = view).
constexpr int CMP_THREADS = 256, CMP_WAVES = CMP_THREADS / 64;
constexpr int SCAN_THREADS = 1024, SCAN_ITEMS = 4, SCAN_WAVES = SCAN_THREADS / 64;
constexpr int SCAN_TILE = SCAN_THREADS * SCAN_ITEMS;          // counts per pass of the scan kernel's loop

__global__ __launch_bounds__(CMP_THREADS) void fusion_compact_count_kernel(const unsigned char* __restrict__ mask, int hw,
                                                                           int* __restrict__ counts) {
    __shared__ int wave_n[CMP_WAVES];
    const int p = blockIdx.x * CMP_THREADS + threadIdx.x;
    const bool m = p < hw && mask[(long)blockIdx.y * hw + p] != 0;
    const unsigned long long b = __ballot(m);
    if ((threadIdx.x & 63) == 0) wave_n[threadIdx.x >> 6] = __popcll(b);
    __syncthreads();
    if (threadIdx.x == 0) {
        int n = 0;
        for (int i = 0; i < CMP_WAVES; ++i) n += wave_n[i];
        counts[(long)blockIdx.y * gridDim.x + blockIdx.x] = n;
    }
}

// In place: counts[i] -> number of survivors before workgroup i.  One workgroup walks the array in tiles of SCAN_TILE and carries the
// running total; offsets[v] = survivors before view v (v = 0 .. n_views, the last entry the total M).
__global__ __launch_bounds__(SCAN_THREADS) void fusion_compact_scan_kernel(int* __restrict__ counts, int n, int blocks_per_view,
                                                                           int* __restrict__ offsets) {
    __shared__ int wave_sum[SCAN_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int carry = 0;
    for (int base = 0; base < n; base += SCAN_TILE) {
        const int i0 = base + tid * SCAN_ITEMS;
        int v[SCAN_ITEMS], sum = 0;
#pragma unroll
        for (int k = 0; k < SCAN_ITEMS; ++k) {
            v[k] = (i0 + k < n) ? counts[i0 + k] : 0;
            sum += v[k];
        }
        int inc = sum;                                          // inclusive scan of the threads' sums inside the wave
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int up = __shfl_up(inc, d, 64);
            if (lane >= d) inc += up;
        }
        if (lane == 63) wave_sum[wv] = inc;
        __syncthreads();
        int before = 0, tile = 0;
#pragma unroll
        for (int j = 0; j < SCAN_WAVES; ++j) {
            const int ws = wave_sum[j];
            if (j < wv) before += ws;
            tile += ws;
        }
        int run = carry + before + inc - sum;
#pragma unroll
        for (int k = 0; k < SCAN_ITEMS; ++k) {
            const int i = i0 + k;
            if (i < n) {
                counts[i] = run;
                if (i % blocks_per_view == 0) offsets[i / blocks_per_view] = run;
                run += v[k];
            }
        }
        carry += tile;
        __syncthreads();                                        // wave_sum is rewritten by the next tile
    }
    if (tid == 0) offsets[n / blocks_per_view] = carry;
}

// points [n_ref][3][h][w]; image of row r = images + view * img_view_stride with view = table ? table[r * table_stride] : r, channel c of
// pixel p at p * pix_stride + c * ch_stride ([h][w][3]: 3, 1; [3][h][w]: 1, h*w).  Colour = (uint8)(c * 255.0f): one multiply, truncation.
__global__ __launch_bounds__(CMP_THREADS) void fusion_compact_scatter_kernel(
    const unsigned char* __restrict__ mask, const float* __restrict__ points, const float* __restrict__ images, const int* __restrict__ table,
    int table_stride, long img_view_stride, long pix_stride, long ch_stride, int hw, const int* __restrict__ block_base,
    float* __restrict__ xyz, unsigned char* __restrict__ rgb) {
    __shared__ int wave_n[CMP_WAVES];
    const int p = blockIdx.x * CMP_THREADS + threadIdx.x, r = blockIdx.y;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const bool m = p < hw && mask[(long)r * hw + p] != 0;
    const unsigned long long b = __ballot(m);
    if (lane == 0) wave_n[wv] = __popcll(b);
    __syncthreads();
    if (!m) return;
    long dst = block_base[(long)r * gridDim.x + blockIdx.x] + __popcll(b & ((1ull << lane) - 1ull));
    for (int j = 0; j < wv; ++j) dst += wave_n[j];
    const float* pt = points + (long)r * 3 * hw + p;
    const int view = table ? table[(long)r * table_stride] : r;
    const float* px = images + (long)view * img_view_stride + (long)p * pix_stride;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        xyz[dst * 3 + c] = pt[(long)c * hw];
        rgb[dst * 3 + c] = (unsigned char)(int)(px[c * ch_stride] * 255.0f);
    }
}

}  // namespace

// Host-side check of a pair table [n_ref][1 + v_max] (row = reference id, source ids, -1 padding at the end only): every id inside
// [0, n_views), at least min_src and at most FUS_MAX_VIEWS sources per row.
static int fus_check_table(const int* table, int n_ref, int v_max, int n_views, int min_src) {
    if (!table || n_ref < 1 || n_ref > 65535 || v_max < 1 || v_max > FUS_MAX_VIEWS || n_views < 1) return EFFI_ERR_BADARG;
    for (int r = 0; r < n_ref; ++r) {
        const int* row = table + (long)r * (v_max + 1);
        if (row[0] < 0 || row[0] >= n_views) return EFFI_ERR_BADARG;
        int n = 0;
        while (n < v_max && row[1 + n] >= 0) ++n;
        for (int k = 0; k < v_max; ++k)
            if (k < n ? row[1 + k] >= n_views : row[1 + k] != -1) return EFFI_ERR_BADARG;
        if (n < min_src) return EFFI_ERR_BADARG;
    }
    return EFFI_OK;
}

extern "C" int effi_fusion_compact_blocks(int n_ref, int h, int w) {
    if (n_ref < 1 || n_ref > 65535 || h < 1 || w < 1 || (long)n_ref * h * w >= (1L << 31)) return 0;
    return n_ref * effi_cdiv((long)h * w, CMP_THREADS);
}

extern "C" int effi_fusion_compact_scan_tile(void) { return SCAN_TILE; }

extern "C" int effi_fusion_compact_count_u8(const unsigned char* mask, int n_ref, int h, int w, int* block_base, int* offsets,
                                            effi_stream_t stream) {
    if (!mask || !block_base || !offsets || n_ref < 1 || n_ref > 65535 || h < 1 || w < 1) return EFFI_ERR_BADARG;
    if ((long)n_ref * h * w >= (1L << 31)) return EFFI_ERR_BADARG;
    hipStream_t st = effi_s(stream);
    const int hw = h * w, bpv = effi_cdiv(hw, CMP_THREADS);
    hipLaunchKernelGGL(fusion_compact_count_kernel, dim3(bpv, n_ref), dim3(CMP_THREADS), 0, st, mask, hw, block_base);
    EFFI_LAUNCH_CHECK();
    hipLaunchKernelGGL(fusion_compact_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, st, block_base, n_ref * bpv, bpv, offsets);
    EFFI_LAUNCH_CHECK();
    return EFFI_OK;
}

extern "C" int effi_fusion_compact_scatter_f32(const unsigned char* mask, const float* points, const float* images, int n_images,
                                               const int* pair_table_host, const int* pair_table, int table_stride, long img_view_stride,
                                               long pix_stride, long ch_stride, int n_ref, int h, int w, const int* block_base,
                                               float* xyz, unsigned char* rgb, effi_stream_t stream) {
    if (!mask || !points || !images || !block_base || !xyz || !rgb || n_ref < 1 || n_ref > 65535 || h < 1 || w < 1) return EFFI_ERR_BADARG;
    if ((long)n_ref * h * w >= (1L << 31) || n_images < 1 || img_view_stride < 0 || pix_stride < 1 || ch_stride < 1) return EFFI_ERR_BADARG;
    if ((pair_table == nullptr) != (pair_table_host == nullptr)) return EFFI_ERR_BADARG;
    if (pair_table_host) {
        if (table_stride < 1) return EFFI_ERR_BADARG;
        for (int r = 0; r < n_ref; ++r)
            if (pair_table_host[(long)r * table_stride] < 0 || pair_table_host[(long)r * table_stride] >= n_images) return EFFI_ERR_BADARG;
    } else if (n_images < n_ref) {
        return EFFI_ERR_BADARG;
    }
    hipStream_t st = effi_s(stream);
    const int hw = h * w;
    hipLaunchKernelGGL(fusion_compact_scatter_kernel, dim3(effi_cdiv(hw, CMP_THREADS), n_ref), dim3(CMP_THREADS), 0, st, mask, points, images,
                       pair_table, table_stride, img_view_stride, pix_stride, ch_stride, hw, block_base, xyz, rgb);
    EFFI_LAUNCH_CHECK();
    return EFFI_OK;
}

extern "C" int effi_fusion_vis_filter_f32(const float* ref_depth, const float* reproj_xyd, int n, int n_src, int h, int w,
                                          float dist_base, float rel_diff_base, int thres_view, int relative, unsigned char* masks,
                                          effi_stream_t stream) {
    if (!ref_depth || !reproj_xyd || !masks || n < 1 || n_src < 1 || h < 1 || w < 1) return EFFI_ERR_BADARG;
    if (thres_view < 0 || thres_view > n_src || dist_base <= 0.0f || rel_diff_base <= 0.0f || (long)n * n_src > 65535) return EFFI_ERR_BADARG;
    hipStream_t st = effi_s(stream);
    hipLaunchKernelGGL(fusion_vis_filter_kernel, dim3(effi_cdiv((long)h * w, 256), n * n_src), dim3(256), 0, st, ref_depth, reproj_xyd,
                       n_src, h, w, dist_base, rel_diff_base, thres_view, relative, masks);
    EFFI_LAUNCH_CHECK();
    return EFFI_OK;
}

extern "C" int effi_fusion_points_f32(int mode, const float* in, long in_batch_stride, const float* depth, const float* cams, int n,
                                      int h, int w, float* mats_scratch, float* out, effi_stream_t stream) {
    if (!in || !cams || !mats_scratch || !out || n < 1 || n > 65535 || h < 1 || w < 1 || mode < 0 || mode > 3) return EFFI_ERR_BADARG;
    if (mode == 0 && !depth) return EFFI_ERR_BADARG;
    hipStream_t st = effi_s(stream);
    const int hw = h * w;
    hipLaunchKernelGGL(fusion_prepare_batch_kernel, dim3(effi_cdiv(n, 64)), dim3(64), 0, st, cams, n, mats_scratch);
    EFFI_LAUNCH_CHECK();
    const dim3 grid(effi_cdiv(hw, 256), n), blk(256);
    switch (mode) {
        case 0: hipLaunchKernelGGL(fusion_points_kernel<0>, grid, blk, 0, st, in, in_batch_stride, depth, mats_scratch, hw, out); break;
        case 1: hipLaunchKernelGGL(fusion_points_kernel<1>, grid, blk, 0, st, in, in_batch_stride, depth, mats_scratch, hw, out); break;
        case 2: hipLaunchKernelGGL(fusion_points_kernel<2>, grid, blk, 0, st, in, in_batch_stride, depth, mats_scratch, hw, out); break;
        default: hipLaunchKernelGGL(fusion_points_kernel<3>, grid, blk, 0, st, in, in_batch_stride, depth, mats_scratch, hw, out); break;
    }
    EFFI_LAUNCH_CHECK();
    return EFFI_OK;
}

extern "C" int effi_fusion_dtu_reproject_f32(const float* ref_depth, const float* src_depth, const float* ref_cam, const float* src_cam,
                                             int h, int w, int s, int e, float dist_base, float diff_base, float* mats_scratch,
                                             float* out5, unsigned char* masks, effi_stream_t stream) {
    if (!ref_depth || !src_depth || !ref_cam || !src_cam || !mats_scratch || !out5 || h < 2 || w < 2) return EFFI_ERR_BADARG;
    if (masks && (s < 1 || e <= s || dist_base <= 0.0f || diff_base <= 0.0f)) return EFFI_ERR_BADARG;
    hipStream_t st = effi_s(stream);
    const FusRows cams{ref_cam, src_cam, nullptr, 1};
    hipLaunchKernelGGL(fusion_dtu_prepare_kernel, dim3(1), dim3(64), 0, st, cams, 1, mats_scratch);
    EFFI_LAUNCH_CHECK();
    hipLaunchKernelGGL(fusion_dtu_reproject_kernel, dim3(effi_cdiv((long)h * w, 256)), dim3(256), 0, st, ref_depth, src_depth, h, w,
                       mats_scratch, s, e, dist_base, diff_base, out5, masks);
    EFFI_LAUNCH_CHECK();
    return EFFI_OK;
}

// ---- the fixed-threshold visibility filter (misc/fusion.py:50-115) ----
static int fus_static_thresholds(double img_dist_thresh, double depth_thresh, double vthresh, float* dist_thr, float* depth_thr,
                                 float* count_thr) {
    if (!(img_dist_thresh > 0.0) || !(depth_thresh > 0.0) || !(vthresh == vthresh)) return EFFI_ERR_BADARG;
    *dist_thr = (float)(1.0 / img_dist_thresh);                      // formed in double, compared as its fp32 rounding
    *depth_thr = (float)(1.0 / depth_thresh);
    *count_thr = (float)(vthresh - 1.1);
    return EFFI_OK;
}

// ---- the three fused filters, each as a single-view and a scan entry over one body ----
// One filter launch as its entry describes it: depth maps and cameras under one addressing, mats [n_rows][v_max+1][52].
struct FusLaunch {
    bool scan;                  // false: one row, no table, maps / cams = (reference, stacked sources)
    FusRows maps, cams;
    const int* table_host;
    int n_views, n_rows, h, w;
    float* mats;
};
static FusLaunch fus_single(const float* ref_depth, const float* src_depths, const float* ref_cam, const float* src_cams, int n_src, int h,
                            int w, float* mats) {
    return {false, {ref_depth, src_depths, nullptr, n_src}, {ref_cam, src_cams, nullptr, n_src}, nullptr, 0, 1, h, w, mats};
}
static FusLaunch fus_scan(const float* depths, const float* cams, int n_views, const int* table_host, const int* table, int n_ref,
                          int v_max, int h, int w, float* mats) {
    return {true, {depths, depths, table, v_max}, {cams, cams, table, v_max}, table_host, n_views, n_ref, h, w, mats};
}

// What every filter entry refuses beyond its own parameters.  A single view may have too many sources for the kernels
// (UNSUPPORTED, as is ``over_limit``, a filter's own capacity); a table with such a row is a bad argument.  Every entry refuses
// 2^31 pixels or more per launch (BADARG): the kernels index pixels with an int.  The single-view dynamic and DTU entries did not
// before they shared this check, and could not have run such a size.
static int fus_check(const FusLaunch& L, const FusIO& io, int min_src, bool over_limit) {
    const int V = L.maps.v_max;
    if (!L.maps.ref_base || !L.maps.src_base || !L.cams.ref_base || !L.cams.src_base || !L.mats || !io.out_depth) return EFFI_ERR_BADARG;
    if ((L.scan && !L.maps.table) || L.h < 2 || L.w < 2) return EFFI_ERR_BADARG;
    if (!L.scan && (V < 1 || V < min_src || (long)L.h * L.w >= (1L << 31))) return EFFI_ERR_BADARG;
    if (over_limit || (!L.scan && V > FUS_MAX_VIEWS)) return EFFI_ERR_UNSUPPORTED;
    if (io.conf && (io.ch < 1 || io.cw < 1)) return EFFI_ERR_BADARG;
    if (L.scan && (fus_check_table(L.table_host, L.n_rows, V, L.n_views, min_src) != EFFI_OK || (long)L.n_rows * L.h * L.w >= (1L << 31)))
        return EFFI_ERR_BADARG;
    return EFFI_OK;
}

// the view matrices of every row, then the filter: one workgroup row per table row
template <class Filter>
static int fus_run(const FusLaunch& L, void (*prepare)(FusRows, int, float*), const Filter& f, effi_stream_t stream) {
    hipStream_t st = effi_s(stream);
    hipLaunchKernelGGL(prepare, dim3(effi_cdiv((long)L.n_rows * (L.maps.v_max + 1), 64)), dim3(64), 0, st, L.cams, L.n_rows, L.mats);
    EFFI_LAUNCH_CHECK();
    hipLaunchKernelGGL((L.scan ? fusion_filter_kernel<Filter, true> : fusion_filter_kernel<Filter, false>),
                       dim3(effi_cdiv((long)L.h * L.w, 256), L.n_rows), dim3(256), 0, st, L.maps, L.h, L.w, L.mats, f);
    EFFI_LAUNCH_CHECK();
    return EFFI_OK;
}

static int fus_dynamic_impl(const FusLaunch& L, const FusIO& io, int dh, float dist_base, float rel_base, int relative,
                            effi_stream_t stream) {
    if (dh < 1 || dist_base <= 0.0f || rel_base <= 0.0f) return EFFI_ERR_BADARG;
    const int rc = fus_check(L, io, dh, false);                     // every row needs dh sources
    if (rc != EFFI_OK) return rc;
    return fus_run(L, fusion_prepare_kernel, FusDynamic{io, dh, dist_base, rel_base, relative}, stream);
}

static int fus_static_impl(const FusLaunch& L, const FusIO& io, double img_dist_thresh, double depth_thresh, double vthresh,
                           effi_stream_t stream) {
    const int rc = fus_check(L, io, 1, false);
    if (rc != EFFI_OK) return rc;
    FusStatic f{io};
    if (fus_static_thresholds(img_dist_thresh, depth_thresh, vthresh, &f.dist_thr, &f.depth_thr, &f.count_thr) != EFFI_OK) return EFFI_ERR_BADARG;
    return fus_run(L, fusion_prepare_kernel, f, stream);
}

static int fus_dtu_impl(const FusLaunch& L, const FusIO& io, float conf_keep, int s, int e, float dist_base, float diff_base,
                        effi_stream_t stream) {
    if (s < 1 || e <= s || dist_base <= 0.0f || diff_base <= 0.0f) return EFFI_ERR_BADARG;
    const int rc = fus_check(L, io, 1, e - s > DTU_MAX_THR);
    if (rc != EFFI_OK) return rc;
    return fus_run(L, fusion_dtu_prepare_kernel, FusDtu{io, conf_keep, s, e, dist_base, diff_base}, stream);
}

extern "C" int effi_fusion_dynamic_filter_f32(const float* ref_depth, const float* src_depths, const float* ref_cam,
                                              const float* src_cams, int n_src, int h, int w, const float* ref_conf, int conf_h,
                                              int conf_w, float prob_threshold, int dh_view_num, float dist_base,
                                              float rel_diff_base, int relative, float* mats_scratch, float* out_depth,
                                              unsigned char* out_geo_mask, unsigned char* out_prob_mask,
                                              unsigned char* out_mask, float* out_points, float* out_reproj_xyd,
                                              effi_stream_t stream) {
    return fus_dynamic_impl(fus_single(ref_depth, src_depths, ref_cam, src_cams, n_src, h, w, mats_scratch),
                            {ref_conf, conf_h, conf_w, prob_threshold, out_depth, out_geo_mask, out_prob_mask, out_mask, out_points,
                             out_reproj_xyd, nullptr},
                            dh_view_num, dist_base, rel_diff_base, relative, stream);
}

extern "C" int effi_fusion_dynamic_filter_scan_f32(const float* depths, const float* cams, int n_views, const int* pair_table_host,
                                                   const int* pair_table, int n_ref, int v_max, int h, int w, const float* ref_conf,
                                                   int conf_h, int conf_w, float prob_threshold, int dh_view_num, float dist_base,
                                                   float rel_diff_base, int relative, float* mats_scratch, float* out_depth,
                                                   unsigned char* out_geo_mask, unsigned char* out_prob_mask, unsigned char* out_mask,
                                                   float* out_points, effi_stream_t stream) {
    return fus_dynamic_impl(fus_scan(depths, cams, n_views, pair_table_host, pair_table, n_ref, v_max, h, w, mats_scratch),
                            {ref_conf, conf_h, conf_w, prob_threshold, out_depth, out_geo_mask, out_prob_mask, out_mask, out_points,
                             nullptr, nullptr},
                            dh_view_num, dist_base, rel_diff_base, relative, stream);
}

extern "C" int effi_fusion_static_filter_f32(const float* ref_depth, const float* src_depths, const float* ref_cam, const float* src_cams,
                                             int n_src, int h, int w, const float* ref_conf, int conf_h, int conf_w, float prob_threshold,
                                             double img_dist_thresh, double depth_thresh, double vthresh, float* mats_scratch,
                                             float* out_depth, unsigned char* out_geo_mask, unsigned char* out_prob_mask,
                                             unsigned char* out_mask, float* out_points, float* out_reproj_xyd, float* out_in_range,
                                             effi_stream_t stream) {
    return fus_static_impl(fus_single(ref_depth, src_depths, ref_cam, src_cams, n_src, h, w, mats_scratch),
                           {ref_conf, conf_h, conf_w, prob_threshold, out_depth, out_geo_mask, out_prob_mask, out_mask, out_points,
                            out_reproj_xyd, out_in_range},
                           img_dist_thresh, depth_thresh, vthresh, stream);
}

extern "C" int effi_fusion_static_filter_scan_f32(const float* depths, const float* cams, int n_views, const int* pair_table_host,
                                                  const int* pair_table, int n_ref, int v_max, int h, int w, const float* ref_conf,
                                                  int conf_h, int conf_w, float prob_threshold, double img_dist_thresh, double depth_thresh,
                                                  double vthresh, float* mats_scratch, float* out_depth, unsigned char* out_geo_mask,
                                                  unsigned char* out_prob_mask, unsigned char* out_mask, float* out_points,
                                                  effi_stream_t stream) {
    return fus_static_impl(fus_scan(depths, cams, n_views, pair_table_host, pair_table, n_ref, v_max, h, w, mats_scratch),
                           {ref_conf, conf_h, conf_w, prob_threshold, out_depth, out_geo_mask, out_prob_mask, out_mask, out_points, nullptr,
                            nullptr},
                           img_dist_thresh, depth_thresh, vthresh, stream);
}

// confidence [n_rows][h][w], already at the depth size
extern "C" int effi_fusion_dtu_filter_f32(const float* ref_depth, const float* src_depths, const float* ref_cam, const float* src_cams,
                                          int n_src, int h, int w, const float* confidence, float conf_threshold, float conf_keep,
                                          int s, int e, float dist_base, float diff_base, float* mats_scratch, float* out_depth,
                                          unsigned char* out_photo_mask, unsigned char* out_geo_mask, unsigned char* out_final_mask,
                                          float* out_points, effi_stream_t stream) {
    return fus_dtu_impl(fus_single(ref_depth, src_depths, ref_cam, src_cams, n_src, h, w, mats_scratch),
                        {confidence, h, w, conf_threshold, out_depth, out_geo_mask, out_photo_mask, out_final_mask, out_points, nullptr,
                         nullptr},
                        conf_keep, s, e, dist_base, diff_base, stream);
}

extern "C" int effi_fusion_dtu_filter_scan_f32(const float* depths, const float* cams, int n_views, const int* pair_table_host,
                                               const int* pair_table, int n_ref, int v_max, int h, int w, const float* confidence,
                                               float conf_threshold, float conf_keep, int s, int e, float dist_base, float diff_base,
                                               float* mats_scratch, float* out_depth, unsigned char* out_photo_mask,
                                               unsigned char* out_geo_mask, unsigned char* out_final_mask, float* out_points,
                                               effi_stream_t stream) {
    return fus_dtu_impl(fus_scan(depths, cams, n_views, pair_table_host, pair_table, n_ref, v_max, h, w, mats_scratch),
                        {confidence, h, w, conf_threshold, out_depth, out_geo_mask, out_photo_mask, out_final_mask, out_points, nullptr,
                         nullptr},
                        conf_keep, s, e, dist_base, diff_base, stream);
}

extern "C" int effi_fusion_project_img_f32(const float* src_img, const float* dst_depth, const float* src_cams, const float* dst_cams,
                                           int n, int channels, int src_h, int src_w, int height, int width, float* mats_scratch,
                                           float* out_img, float* out_in_range, effi_stream_t stream) {
    if (!src_img || !dst_depth || !src_cams || !dst_cams || !mats_scratch || !out_img) return EFFI_ERR_BADARG;
    if (n < 1 || n > 65535 || channels < 1 || src_h < 1 || src_w < 1 || height < 1 || width < 1) return EFFI_ERR_BADARG;
    if ((long)n * channels * height * width >= (1L << 31) || (long)n * channels * src_h * src_w >= (1L << 31)) return EFFI_ERR_BADARG;
    hipStream_t st = effi_s(stream);
    hipLaunchKernelGGL(fusion_prepare_pairs_kernel, dim3(effi_cdiv(2L * n, 64)), dim3(64), 0, st, dst_cams, src_cams, n, mats_scratch);
    EFFI_LAUNCH_CHECK();
    hipLaunchKernelGGL(fusion_project_img_kernel, dim3(effi_cdiv((long)height * width, 256), n), dim3(256), 0, st, src_img, dst_depth,
                       mats_scratch, channels, src_h, src_w, height, width, out_img, out_in_range);
    EFFI_LAUNCH_CHECK();
    return EFFI_OK;
}

extern "C" int effi_fusion_static_vis_filter_f32(const float* ref_depth, const float* reproj_xyd, const float* masks_in, int n, int n_src,
                                                 int h, int w, double img_dist_thresh, double depth_thresh, double vthresh,
                                                 float* masks_out, unsigned char* mask_out, float* ave_out, effi_stream_t stream) {
    if (!ref_depth || !reproj_xyd || n < 1 || n > 65535 || n_src < 1 || h < 1 || w < 1) return EFFI_ERR_BADARG;
    if (!masks_out && !mask_out && !ave_out) return EFFI_ERR_BADARG;
    if ((long)n * n_src * 3 * h * w >= (1L << 31)) return EFFI_ERR_BADARG;
    float dist_thr = 0.0f, depth_thr = 0.0f, count_thr = 0.0f;
    if (!masks_in && fus_static_thresholds(img_dist_thresh, depth_thresh, vthresh, &dist_thr, &depth_thr, &count_thr) != EFFI_OK)
        return EFFI_ERR_BADARG;
    hipStream_t st = effi_s(stream);
    hipLaunchKernelGGL(fusion_static_vis_kernel, dim3(effi_cdiv((long)h * w, 256), n), dim3(256), 0, st, ref_depth, reproj_xyd, masks_in,
                       n_src, h, w, dist_thr, depth_thr, count_thr, masks_out, mask_out, ave_out);
    EFFI_LAUNCH_CHECK();
    return EFFI_OK;
}

extern "C" int effi_fusion_prob_filter_f32(const float* prob, long batch_stride, int n, long hw, float threshold, int first,
                                           unsigned char* mask, effi_stream_t stream) {
    if (!prob || !mask || n < 1 || n > 65535 || hw < 1 || hw >= (1L << 31) || batch_stride < hw) return EFFI_ERR_BADARG;
    hipStream_t st = effi_s(stream);
    hipLaunchKernelGGL(fusion_prob_filter_kernel, dim3(effi_cdiv(hw, 256), n), dim3(256), 0, st, prob, batch_stride, hw, threshold, first,
                       mask);
    EFFI_LAUNCH_CHECK();
    return EFFI_OK;
}
