// Stand-alone host check of the address arithmetic of csrc/train_input.hip (make -C effi_mvs_plus_amd/csrc host-check), under
// -fsanitize=address,undefined.  It includes only train_input_index.hpp, is compiled for the host alone and never touches a GPU: every
// thread of both launch grids is run as a loop over exactly sized host arrays, with the kernels' own guards and store widths, so an
// index past an end is a heap overflow under the sanitizer.  Checked besides: every output element has exactly one writer, and the
// pyramid reads source (f y, f x).
#include "train_input_index.hpp"

#include <cstdio>
#include <vector>

static int failures = 0;
#define EXPECT(cond)                                                   \
    do {                                                               \
        if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
    } while (0)

static void pyramid(int B, int h, int w) {
    const long hw = (long)h * w;
    std::vector<float> depth(B * hw);
    for (long i = 0; i < B * hw; ++i) depth[i] = (float)i;
    std::vector<float> out[4] = {std::vector<float>(B * (hw >> 6), -1.0f), std::vector<float>(B * (hw >> 4), -1.0f),
                                 std::vector<float>(B * (hw >> 2), -1.0f), std::vector<float>(B * hw, -1.0f)};
    std::vector<int> writers[4] = {std::vector<int>(out[0].size()), std::vector<int>(out[1].size()), std::vector<int>(out[2].size()),
                                   std::vector<int>(out[3].size())};
    const long n_oct = (long)h * (w >> 3), blocks = (n_oct + 63) / 64;
    auto store = [&](int k, long at, const float* v, int n) {
        for (int i = 0; i < n; ++i) out[k].at(at + i) = v[i], ++writers[k].at(at + i);
    };
    for (long b = 0; b < B; ++b)
        for (long bx = 0; bx < blocks; ++bx)
            for (int t = 0; t < 64; ++t) {
                const long o = bx * 64 + t;
                if (o >= n_oct) continue;
                const EffiPyramidIndex ix = effi_pyramid_index(o, b, h, w);
                EXPECT(ix.src % 8 == 0 && ix.o3 % 4 == 0 && ix.o2 % 2 == 0);       // the vector stores' alignment
                float d[8];
                for (int i = 0; i < 8; ++i) d[i] = depth.at(ix.src + i);
                store(3, ix.src, d, 8);
                if (ix.y & 1) continue;
                const float d3[4] = {d[0], d[2], d[4], d[6]};
                store(2, ix.o3, d3, 4);
                if (ix.y & 3) continue;
                const float d2[2] = {d[0], d[4]};
                store(1, ix.o2, d2, 2);
                if (ix.y & 7) continue;
                store(0, ix.o1, d, 1);
            }
    for (int k = 0; k < 4; ++k) {
        const int f = 8 >> k, hk = h / f, wk = w / f;
        for (long b = 0; b < B; ++b)
            for (int y = 0; y < hk; ++y)
                for (int x = 0; x < wk; ++x) {
                    const long at = (b * hk + y) * wk + x;
                    EXPECT(writers[k][at] == 1);
                    EXPECT(out[k][at] == depth[b * hw + (long)(f * y) * w + f * x]);
                }
    }
}

static void images(int V, int h, int w) {
    const long hw = (long)h * w;
    std::vector<unsigned char> src(V * hw * 3);
    for (size_t i = 0; i < src.size(); ++i) src[i] = (unsigned char)(i * 7);
    std::vector<float> dst(V * 3 * hw, -1.0f);
    std::vector<int> writers(dst.size());
    const long blocks = ((hw + 3) / 4 + 127) / 128;
    for (long v = 0; v < V; ++v)
        for (long bx = 0; bx < blocks; ++bx)
            for (int t = 0; t < 128; ++t) {
                const long p0 = effi_images_first_pixel(bx, t);
                if (p0 >= hw) continue;
                const long s = effi_images_src_byte(v, hw, p0), d = effi_images_dst_elem(v, hw, p0);
                if (hw % 4 == 0) EXPECT(s % 4 == 0 && d % 4 == 0);                  // the vector path's alignment
                const int n = hw % 4 == 0 ? 4 : (int)(hw - p0 < 4 ? hw - p0 : 4);
                for (int i = 0; i < n; ++i)
                    for (int c = 0; c < 3; ++c) dst.at(d + c * hw + i) = (float)src.at(s + 3 * i + c), ++writers.at(d + c * hw + i);
            }
    for (long v = 0; v < V; ++v)
        for (int c = 0; c < 3; ++c)
            for (long p = 0; p < hw; ++p) {
                EXPECT(writers[(v * 3 + c) * hw + p] == 1);
                EXPECT(dst[(v * 3 + c) * hw + p] == (float)src[(v * hw + p) * 3 + c]);
            }
}

int main() {
    pyramid(1, 8, 8);
    pyramid(2, 24, 72);
    pyramid(3, 64, 8);
    pyramid(1, 512, 640);
    images(5, 8, 72);
    images(3, 5, 7);
    images(1, 1, 1);
    images(2, 512, 640);
    std::printf(failures ? "train input host check: %d FAILED\n" : "train input host check: ok\n", failures);
    return failures ? 1 : 0;
}
