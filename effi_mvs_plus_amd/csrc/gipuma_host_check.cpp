// Stand-alone host check of the Gipuma fusion kernel (make -C effi_mvs_plus_amd/csrc host-check), under
// -fsanitize=address,undefined.  It includes only gipuma_pixel.hpp, is compiled for the host alone and never touches a GPU: every
// thread of the launch grid runs gip_thread -- the kernel's whole body -- as a loop over exactly sized host arrays, so the one store
// whose address depends on data, used[s][q], is a heap overflow under the sanitizer if q ever leaves the image.  Cases: projections
// that land outside the image on each of its four sides, behind the camera, not-a-number and negative coordinates, depths that are
// NaN / infinite / negative / zero, h * w not a multiple of the workgroup, and a reference view with the full 64 sources.  Checked
// besides: masks and flags hold 0 or 1, counts stay within the source count, a fused pixel carries its own flag, an unfused pixel
// leaves its point untouched, and flags are only ever raised.
#include "gipuma_pixel.hpp"

#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

static int failures = 0;
#define EXPECT(cond)                                                   \
    do {                                                               \
        if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
    } while (0)

struct Cam { float m[32]; };

// R = I (or the half turn about y when `behind`), centre C, focal f, principal point (cx, cy)
static Cam make_cam(float cx_world, float cy_world, float cz_world, float f, float cx, float cy, bool behind = false) {
    Cam c{};
    const float sx = behind ? -1.0f : 1.0f;
    c.m[0] = sx; c.m[5] = 1.0f; c.m[10] = sx; c.m[15] = 1.0f;
    c.m[3] = -sx * cx_world; c.m[7] = -cy_world; c.m[11] = -sx * cz_world;
    c.m[16] = f; c.m[18] = cx; c.m[21] = f; c.m[22] = cy; c.m[26] = 1.0f; c.m[31] = 1.0f;
    return c;
}

struct Result { long fused, marked; };

static Result run_view(const std::vector<Cam>& cams, const std::vector<float>& depths, const std::vector<float>* images, int h, int w,
                       int ref, const std::vector<int>& sources, float thr, int num_consistent, std::vector<unsigned char>& used) {
    const int n_views = (int)cams.size(), n_src = (int)sources.size();
    const long hw = (long)h * w;
    EXPECT((long)depths.size() == n_views * hw && (long)used.size() == n_views * hw && n_src >= 1 && n_src <= GIP_MAX_SRC);
    std::vector<float> mats((size_t)(n_src + 1) * GIP_STRIDE);
    for (int i = 0; i <= n_src; ++i)
        gip_prepare_slot(cams[i == 0 ? ref : sources[i - 1]].m, cams[ref].m, mats.data() + (size_t)i * GIP_STRIDE);
    const float untouched = -12345.0f;
    std::vector<float> points(3 * hw, untouched), colour(images ? 3 * hw : 0, untouched);
    std::vector<unsigned char> mask(hw, 7), count(hw, 255), before(used);
    const GipView a{depths.data(), images ? images->data() : nullptr, sources.data(), mats.data(), ref, n_src, h, w, thr, num_consistent,
                    0.001f, 100000.0f, used.data(), points.data(), images ? colour.data() : nullptr, mask.data(), count.data()};
    const long blocks = (hw + GIP_THREADS - 1) / GIP_THREADS;
    for (long b = 0; b < blocks; ++b)
        for (int t = 0; t < GIP_THREADS; ++t) gip_thread(a, b, t);
    Result r{0, 0};
    for (long p = 0; p < hw; ++p) {
        EXPECT(mask[p] <= 1 && count[p] <= n_src);
        if (mask[p]) {
            ++r.fused;
            EXPECT(used[ref * hw + p] == 1 && before[ref * hw + p] == 0 && count[p] >= num_consistent);
            EXPECT(std::isfinite(points[p]) && std::isfinite(points[hw + p]) && std::isfinite(points[2 * hw + p]));
            if (images) EXPECT(colour[3 * p] >= 0.0f && colour[3 * p] <= 1.0f);
        } else {
            EXPECT(points[p] == untouched && points[hw + p] == untouched && points[2 * hw + p] == untouched);
            EXPECT(used[ref * hw + p] == before[ref * hw + p]);
            if (images) EXPECT(colour[3 * p] == untouched);
        }
    }
    for (size_t i = 0; i < used.size(); ++i) {
        EXPECT(used[i] <= 1 && used[i] >= before[i]);
        r.marked += used[i] - before[i];
    }
    return r;
}

// a fronto-parallel plane at depth 64 seen by a row of cameras 4 apart (disparity 4 px per camera step), with poisoned pixels
static void scene(int n_views, int h, int w, std::vector<Cam>& cams, std::vector<float>& depths, std::vector<float>& images) {
    const long hw = (long)h * w;
    cams.clear();
    for (int v = 0; v < n_views; ++v) cams.push_back(make_cam(4.0f * (float)(v % 7), 0.0f, 0.0f, 64.0f, (float)(w / 2), (float)(h / 2)));
    depths.assign(n_views * hw, 64.0f);
    images.assign(n_views * hw * 3, 0.5f);
    const float bad[6] = {std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity(), -64.0f, 0.0f, 1e-4f, 1e6f};
    for (long i = 0; i < n_views * hw; i += 5) depths[i] = bad[(i / 5) % 6];
}

int main() {
    std::vector<Cam> cams;
    std::vector<float> depths, images;
    // h * w not a multiple of 256, more than one workgroup; all-others sources, every view in turn; the flags persist
    {
        const int n = 6, h = 37, w = 53;
        scene(n, h, w, cams, depths, images);
        std::vector<unsigned char> used((size_t)n * h * w, 0);
        long fused = 0;
        for (int r = 0; r < n; ++r) {
            std::vector<int> src;
            for (int s = 0; s < n; ++s)
                if (s != r) src.push_back(s);
            const Result res = run_view(cams, depths, &images, h, w, r, src, 0.25f, 2, used);
            fused += res.fused;
            EXPECT(res.marked >= res.fused);
        }
        EXPECT(fused > 0);
    }
    // less than one wave, no colours
    {
        const int n = 3, h = 7, w = 9;
        scene(n, h, w, cams, depths, images);
        std::vector<unsigned char> used((size_t)n * h * w, 0);
        EXPECT(run_view(cams, depths, nullptr, h, w, 0, {1, 2}, 0.25f, 1, used).fused > 0);
    }
    // sources whose projections leave the image on each side, lie behind the camera, or are not numbers
    {
        const int h = 19, w = 23;
        const long hw = (long)h * w;
        const float nan = std::numeric_limits<float>::quiet_NaN();
        cams.clear();
        cams.push_back(make_cam(0, 0, 0, 64.0f, 11.0f, 9.0f));                     // 0: reference
        cams.push_back(make_cam(30.0f, 0, 0, 64.0f, 11.0f, 9.0f));                 // 1: shifted right -> q.x negative
        cams.push_back(make_cam(-30.0f, 0, 0, 64.0f, 11.0f, 9.0f));                // 2: q.x >= w
        cams.push_back(make_cam(0, 30.0f, 0, 64.0f, 11.0f, 9.0f));                 // 3: q.y negative
        cams.push_back(make_cam(0, -30.0f, 0, 64.0f, 11.0f, 9.0f));                // 4: q.y >= h
        cams.push_back(make_cam(0, 0, 200.0f, 64.0f, 11.0f, 9.0f));                // 5: the point lies behind it (z < 0)
        cams.push_back(make_cam(0, 0, 0, 64.0f, 11.0f, 9.0f, true));               // 6: looks the other way
        cams.push_back(make_cam(0, 0, 64.0f, 64.0f, 11.0f, 9.0f));                 // 7: the point lies in its centre plane (z = 0: 0 / 0, x / 0)
        cams.push_back(make_cam(nan, 0, 0, 64.0f, 11.0f, 9.0f));                   // 8: not a number
        cams.push_back(make_cam(0, 0, 0, nan, 11.0f, 9.0f));                       // 9: not a number in K
        cams.push_back(make_cam(1e30f, -1e30f, 0, 64.0f, 11.0f, 9.0f));            // 10: coordinates beyond the int range
        cams.push_back(make_cam(0.25f, 0.25f, 0, 64.0f, 11.0f, 9.0f));             // 11: a neighbour that does agree
        cams.push_back(make_cam(5.0f, 3.0f, 0, 64.0f, 11.0f, 9.0f));               // 12: straddles the left / top border
        cams.push_back(make_cam(-5.0f, -3.0f, 0, 64.0f, 11.0f, 9.0f));             // 13: straddles the right / bottom border
        const int n = (int)cams.size();
        depths.assign(n * hw, 64.0f);
        std::vector<unsigned char> used((size_t)n * hw, 0);
        std::vector<int> src;
        for (int s = 1; s < n; ++s) src.push_back(s);
        const Result res = run_view(cams, depths, nullptr, h, w, 0, src, 0.25f, 1, used);
        EXPECT(res.fused > 0);
        for (int s = 1; s <= 10; ++s)
            for (long p = 0; p < hw; ++p) EXPECT(used[s * hw + p] == 0);
        long edge = 0;
        for (long p = 0; p < hw; ++p) edge += used[12 * hw + p] + used[13 * hw + p];
        EXPECT(edge > 0 && edge < 2 * hw);
        // the same with every view as the reference in turn (the flags persist)
        for (int r = 1; r < n; ++r) {
            src.clear();
            for (int s = 0; s < n; ++s)
                if (s != r) src.push_back(s);
            run_view(cams, depths, nullptr, h, w, r, src, 0.25f, 1, used);
        }
    }
    // a reference view with the full 64 sources (bit 63 of the mask)
    {
        const int n = 65, h = 5, w = 8;
        scene(n, h, w, cams, depths, images);
        for (int v = 0; v < n; ++v) cams[v] = make_cam(0.001f * (float)v, 0, 0, 64.0f, 4.0f, 2.0f);
        std::vector<unsigned char> used((size_t)n * h * w, 0);
        std::vector<int> src;
        for (int s = 1; s < n; ++s) src.push_back(s);
        const Result res = run_view(cams, depths, &images, h, w, 0, src, 0.25f, 64, used);
        EXPECT(res.fused > 0);
        long last = 0;
        for (long p = 0; p < (long)h * w; ++p) last += used[64L * h * w + p];
        EXPECT(last == res.fused);                          // source 63 (view 64) was consistent wherever a pixel fused
    }
    std::printf(failures ? "gipuma host check: %d FAILED\n" : "gipuma host check: ok\n", failures);
    return failures ? 1 : 0;
}
