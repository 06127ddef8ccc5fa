// Stand-alone host check of the argument packing of csrc/optim.hip (make -C effi_mvs_plus_amd/csrc host-check): the entry is called
// with every refused argument and with n = 1 and n = AW_MAX_T tensors in exactly sized host arrays under
// -fsanitize=address,undefined, and the chunk table it builds is walked as the update kernel walks it: every element of every
// tensor must fall into exactly one chunk.  The same for the gradient-norm entries (GN_MAX_T tensors; effi_gradnorm_chunks must give
// the walk's count) and for the refusals of the clipped step.  NOTHING here reaches a GPU, with or without one in the machine: optim.hip is included
// below with its launch path stubbed (hipLaunchKernelGGL expands to nothing, the error queries answer hipSuccess) and the program
// is compiled for the host only, so the made-up device addresses are copied into the by-value argument and never read through.
#include <hip/hip_runtime.h>

#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(...) ((void)0)
#define hipPeekAtLastError() hipSuccess
#define hipGetLastError() hipSuccess
#include "optim.hip"

#include <cmath>
#include <cstdio>
#include <vector>

static int failures = 0;
#define EXPECT(cond)                                                   \
    do {                                                               \
        if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
    } while (0)

struct Lists {                  // exactly n entries per array: a read past the end is a heap overflow under the sanitizer
    std::vector<float*> p, m, v, step;
    std::vector<const float*> g;
    std::vector<long> numel;
    explicit Lists(const std::vector<long>& sizes) : numel(sizes) {
        const long n = (long)sizes.size();
        auto fake = [](long i) { return reinterpret_cast<float*>(0x100000 + 0x1000 * i); };
        for (long i = 0; i < n; ++i) {
            p.push_back(fake(5 * i)), g.push_back(fake(5 * i + 1)), m.push_back(fake(5 * i + 2)), v.push_back(fake(5 * i + 3));
            step.push_back(fake(5 * i + 4));
        }
    }
    int call(int n, double b1 = 0.9, double b2 = 0.999, double eps = 1e-8) {
        return effi_adamw_multi_f32(p.data(), g.data(), m.data(), v.data(), step.data(), numel.data(), n, 1e-3, nullptr, b1, b2, eps, 1e-2,
                                    nullptr);
    }
};

// the walk of adamw_update_kernel over the packed table: cover[t][i] counts the chunks that hold element i of tensor t
static void check_cover(const std::vector<long>& sizes) {
    Lists l(sizes);
    const int n = (int)sizes.size();
    AdamWArgs a;
    int chunks = -1;
    EXPECT(aw_pack(l.p.data(), l.g.data(), l.m.data(), l.v.data(), l.step.data(), l.numel.data(), n, 1e-3, nullptr, 0.9, 0.999, 1e-8,
                   1e-2, &a, &chunks) == EFFI_OK);
    std::vector<std::vector<int>> cover(n);
    for (int t = 0; t < n; ++t) cover[t].assign(sizes[t], 0);
    for (int c = 0; c < chunks; ++c) {
        int lo = 0, hi = a.n - 1;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (a.chunk_end[mid] > c) hi = mid;
            else lo = mid + 1;
        }
        const int t = lo;
        const long i0 = (long)(c - (t ? a.chunk_end[t - 1] : 0)) * AW_CHUNK;
        EXPECT(i0 >= 0 && i0 < a.numel[t]);
        if (i0 < 0 || i0 >= a.numel[t]) continue;
        const long len = a.numel[t] - i0 < AW_CHUNK ? a.numel[t] - i0 : AW_CHUNK;
        EXPECT(a.p[t] == l.p[t] && a.g[t] == l.g[t] && a.m[t] == l.m[t] && a.v[t] == l.v[t] && a.step[t] == l.step[t]);
        for (long i = i0; i < i0 + len; ++i) cover[t][i] += 1;
    }
    long total = 0;
    for (int t = 0; t < n; ++t) {
        total += (sizes[t] + AW_CHUNK - 1) / AW_CHUNK;
        for (long i = 0; i < sizes[t]; ++i) {
            if (cover[t][i] != 1) {
                std::printf("FAILED: element %ld of tensor %d (%ld elements) is in %d chunks\n", i, t, sizes[t], cover[t][i]);
                ++failures;
                break;
            }
        }
    }
    EXPECT(chunks == total);
}

// the clipped entry: the refusals of the unclipped one (it packs through aw_pack as well) and a null clip
static void check_clipped_entry(const std::vector<long>& full) {
    const int K = (int)full.size();
    const float* clip = reinterpret_cast<const float*>(0xA00000);
    auto call = [&](Lists& l, int n, const float* c, int skip, double b1 = 0.9) {
        return effi_adamw_multi_clip_f32(l.p.data(), l.g.data(), l.m.data(), l.v.data(), l.step.data(), l.numel.data(), n, 1e-3, nullptr, b1,
                                         0.999, 1e-8, 1e-2, c, skip, nullptr);
    };
    Lists all(full);
    Lists one({5});
    EXPECT(call(one, 1, clip, 0) == EFFI_OK);
    EXPECT(call(all, K, clip, 0) == EFFI_OK);
    EXPECT(call(all, K, clip, 1) == EFFI_OK);
    EXPECT(call(all, K, nullptr, 0) == EFFI_ERR_BADARG);
    EXPECT(call(all, K, nullptr, 1) == EFFI_ERR_BADARG);
    EXPECT(call(all, 0, clip, 1) == EFFI_ERR_BADARG);
    EXPECT(call(all, K + 1, clip, 1) == EFFI_ERR_BADARG);
    EXPECT(call(all, K, clip, 1, 1.0) == EFFI_ERR_BADARG);
    Lists bad(full);
    bad.g[K - 1] = nullptr;
    EXPECT(call(bad, K, clip, 1) == EFFI_ERR_BADARG);
    // aw_pack leaves the new fields cleared: the unclipped entry's argument names no clip tensor
    AdamWArgs a;
    int chunks = -1;
    EXPECT(aw_pack(all.p.data(), all.g.data(), all.m.data(), all.v.data(), all.step.data(), all.numel.data(), K, 1e-3, nullptr, 0.9, 0.999,
                   1e-8, 1e-2, &a, &chunks) == EFFI_OK && a.clip == nullptr && a.skip == 0);
}

struct Grads {                  // exactly n entries per array
    std::vector<const float*> g;
    std::vector<long> numel;
    explicit Grads(const std::vector<long>& sizes) : numel(sizes) {
        for (long i = 0; i < (long)sizes.size(); ++i) g.push_back(reinterpret_cast<const float*>(0x100000 + 0x1000 * i));
    }
    int call(int n, double* partial) { return effi_gradnorm_partial_f32(g.data(), numel.data(), n, partial, nullptr); }
};

// the walk of gradnorm_partial_kernel over the packed table, and effi_gradnorm_chunks against its count
static void check_gn_cover(const std::vector<long>& sizes) {
    Grads l(sizes);
    const int n = (int)sizes.size();
    double* partial = reinterpret_cast<double*>(0xB00000);
    GradNormArgs a;
    int chunks = -1;
    EXPECT(gn_pack(l.g.data(), l.numel.data(), n, partial, &a, &chunks) == EFFI_OK);
    EXPECT(a.partial == partial && a.n == n);
    std::vector<std::vector<int>> cover(n);
    for (int t = 0; t < n; ++t) cover[t].assign(sizes[t], 0);
    for (int c = 0; c < chunks; ++c) {
        int lo = 0, hi = a.n - 1;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (a.chunk_end[mid] > c) hi = mid;
            else lo = mid + 1;
        }
        const int t = lo;
        const long i0 = (long)(c - (t ? a.chunk_end[t - 1] : 0)) * AW_CHUNK;
        EXPECT(i0 >= 0 && i0 < a.numel[t]);
        if (i0 < 0 || i0 >= a.numel[t]) continue;
        const long len = a.numel[t] - i0 < AW_CHUNK ? a.numel[t] - i0 : AW_CHUNK;
        EXPECT(a.g[t] == l.g[t]);
        for (long i = i0; i < i0 + len; ++i) cover[t][i] += 1;
    }
    for (int t = 0; t < n; ++t)
        for (long i = 0; i < sizes[t]; ++i)
            if (cover[t][i] != 1) {
                std::printf("FAILED: gradient element %ld of tensor %d (%ld elements) is in %d chunks\n", i, t, sizes[t], cover[t][i]);
                ++failures;
                break;
            }
    EXPECT(effi_gradnorm_chunks(l.numel.data(), n) == chunks);
}

static void check_gradnorm(const std::vector<long>& edge) {
    const int K = effi_gradnorm_max_tensors();
    EXPECT(K == GN_MAX_T && K >= 1);
    double* partial = reinterpret_cast<double*>(0xB00000);
    float* clip = reinterpret_cast<float*>(0xC00000);
    long long* skipped = reinterpret_cast<long long*>(0xD00000);

    // valid calls: one tensor, and a full table
    for (long s : edge) {
        Grads one({s});
        EXPECT(one.call(1, partial) == EFFI_OK);
        EXPECT(effi_gradnorm_chunks(one.numel.data(), 1) == (s + AW_CHUNK - 1) / AW_CHUNK);
    }
    std::vector<long> full(K);
    for (int i = 0; i < K; ++i) full[i] = edge[i % edge.size()] + (i / (long)edge.size());
    Grads all(full);
    EXPECT(all.call(K, partial) == EFFI_OK);
    {
        Grads empty({0, 0});                            // no chunk: no launch, and no workspace needed
        EXPECT(empty.call(2, nullptr) == EFFI_OK);
        EXPECT(effi_gradnorm_chunks(empty.numel.data(), 2) == 0);
    }

    // refusals of the partial entry
    EXPECT(all.call(0, partial) == EFFI_ERR_BADARG);
    EXPECT(all.call(-1, partial) == EFFI_ERR_BADARG);
    EXPECT(all.call(K + 1, partial) == EFFI_ERR_BADARG);            // refused before entry K is read
    EXPECT(all.call(K, nullptr) == EFFI_ERR_BADARG);
    EXPECT(effi_gradnorm_partial_f32(nullptr, all.numel.data(), K, partial, nullptr) == EFFI_ERR_BADARG);
    EXPECT(effi_gradnorm_partial_f32(all.g.data(), nullptr, K, partial, nullptr) == EFFI_ERR_BADARG);
    for (int i : {0, K - 1}) {
        Grads bad(full);
        bad.g[i] = nullptr;
        EXPECT(bad.call(K, partial) == EFFI_ERR_BADARG);
        Grads neg(full);
        neg.numel[i] = -1;
        EXPECT(neg.call(K, partial) == EFFI_ERR_BADARG);
        EXPECT(effi_gradnorm_chunks(neg.numel.data(), K) < 0);
    }
    {
        Grads tail(full);                               // a null pointer or a negative size PAST n is not looked at
        tail.g[K - 1] = nullptr, tail.numel[K - 1] = -5;
        if (K > 1) EXPECT(tail.call(K - 1, partial) == EFFI_OK);
        if (K > 1) EXPECT(effi_gradnorm_chunks(tail.numel.data(), K - 1) >= 0);
        Grads big({1L << 41, 1L << 41});                // 2^31 chunks together
        EXPECT(big.call(1, partial) == EFFI_OK);
        EXPECT(big.call(2, partial) == EFFI_ERR_BADARG);
        EXPECT(effi_gradnorm_chunks(big.numel.data(), 1) == 1L << 30);
        EXPECT(effi_gradnorm_chunks(big.numel.data(), 2) < 0);
        Grads huge({LONG_MAX});
        EXPECT(huge.call(1, partial) == EFFI_ERR_BADARG);
    }
    // the host-only count takes any number of tensors, none included
    EXPECT(effi_gradnorm_chunks(nullptr, 0) == 0);
    EXPECT(effi_gradnorm_chunks(nullptr, 1) < 0);
    EXPECT(effi_gradnorm_chunks(all.numel.data(), -1) < 0);
    {
        std::vector<long> many(2 * K + 3, AW_CHUNK + 1);
        EXPECT(effi_gradnorm_chunks(many.data(), (int)many.size()) == 2 * (long)many.size());
    }

    // the finish entry
    EXPECT(effi_gradnorm_finish_f32(partial, 7, 1.0, clip, skipped, nullptr) == EFFI_OK);
    EXPECT(effi_gradnorm_finish_f32(partial, 7, 0.0, clip, nullptr, nullptr) == EFFI_OK);
    EXPECT(effi_gradnorm_finish_f32(partial, 7, INFINITY, clip, nullptr, nullptr) == EFFI_OK);
    EXPECT(effi_gradnorm_finish_f32(nullptr, 0, 1.0, clip, nullptr, nullptr) == EFFI_OK);         // no partial: norm 0
    EXPECT(effi_gradnorm_finish_f32(nullptr, 7, 1.0, clip, nullptr, nullptr) == EFFI_ERR_BADARG);
    EXPECT(effi_gradnorm_finish_f32(partial, -1, 1.0, clip, nullptr, nullptr) == EFFI_ERR_BADARG);
    EXPECT(effi_gradnorm_finish_f32(partial, 7, 1.0, nullptr, skipped, nullptr) == EFFI_ERR_BADARG);
    EXPECT(effi_gradnorm_finish_f32(partial, 7, -1e-9, clip, nullptr, nullptr) == EFFI_ERR_BADARG);
    EXPECT(effi_gradnorm_finish_f32(partial, 7, -INFINITY, clip, nullptr, nullptr) == EFFI_ERR_BADARG);
    EXPECT(effi_gradnorm_finish_f32(partial, 7, std::nan(""), clip, nullptr, nullptr) == EFFI_ERR_BADARG);

    // the chunks of the packed table cover every gradient element exactly once
    check_gn_cover(edge);
    for (long s : edge) check_gn_cover({s});
    std::vector<long> rev(edge.rbegin(), edge.rend());
    check_gn_cover(rev);
    check_gn_cover({0, 0, 5, 0, AW_CHUNK, 0});
    std::vector<long> fullc(K);
    for (int i = 0; i < K; ++i) fullc[i] = edge[(i * 3) % edge.size()];
    check_gn_cover(fullc);
}

int main() {
    const int K = effi_adamw_max_tensors();
    EXPECT(K == AW_MAX_T && K >= 1);
    const std::vector<long> edge = {1, 3, AW_CHUNK - 1, AW_CHUNK, AW_CHUNK + 1, 3 * AW_CHUNK + 5, 0};

    // valid calls: one tensor, and a full table
    for (long s : edge) {
        Lists one({s});
        EXPECT(one.call(1) == EFFI_OK);
    }
    std::vector<long> full(K);
    for (int i = 0; i < K; ++i) full[i] = edge[i % edge.size()] + (i / (long)edge.size());
    Lists all(full);
    EXPECT(all.call(K) == EFFI_OK);
    EXPECT(all.call(K, 0.0, 0.0, 0.0) == EFFI_OK);
    float* lr_dev = reinterpret_cast<float*>(0x900000);
    EXPECT(effi_adamw_multi_f32(all.p.data(), all.g.data(), all.m.data(), all.v.data(), all.step.data(), all.numel.data(), K, 0.0, lr_dev,
                                0.9, 0.999, 1e-8, 0.0, nullptr) == EFFI_OK);

    // refusals
    EXPECT(all.call(0) == EFFI_ERR_BADARG);
    EXPECT(all.call(-1) == EFFI_ERR_BADARG);
    EXPECT(all.call(K + 1) == EFFI_ERR_BADARG);          // refused before entry K is read
    EXPECT(all.call(K, 1.0) == EFFI_ERR_BADARG);
    EXPECT(all.call(K, -0.1) == EFFI_ERR_BADARG);
    EXPECT(all.call(K, std::nan("")) == EFFI_ERR_BADARG);
    EXPECT(all.call(K, 0.9, 1.0) == EFFI_ERR_BADARG);
    EXPECT(all.call(K, 0.9, -1e-3) == EFFI_ERR_BADARG);
    EXPECT(all.call(K, 0.9, std::nan("")) == EFFI_ERR_BADARG);
    EXPECT(all.call(K, 0.9, 0.999, -1e-8) == EFFI_ERR_BADARG);
    EXPECT(all.call(K, 0.9, 0.999, std::nan("")) == EFFI_ERR_BADARG);
    const long* nm = all.numel.data();
    EXPECT(effi_adamw_multi_f32(nullptr, all.g.data(), all.m.data(), all.v.data(), all.step.data(), nm, K, 1e-3, nullptr, 0.9, 0.999, 1e-8, 0, nullptr) == EFFI_ERR_BADARG);
    EXPECT(effi_adamw_multi_f32(all.p.data(), nullptr, all.m.data(), all.v.data(), all.step.data(), nm, K, 1e-3, nullptr, 0.9, 0.999, 1e-8, 0, nullptr) == EFFI_ERR_BADARG);
    EXPECT(effi_adamw_multi_f32(all.p.data(), all.g.data(), nullptr, all.v.data(), all.step.data(), nm, K, 1e-3, nullptr, 0.9, 0.999, 1e-8, 0, nullptr) == EFFI_ERR_BADARG);
    EXPECT(effi_adamw_multi_f32(all.p.data(), all.g.data(), all.m.data(), nullptr, all.step.data(), nm, K, 1e-3, nullptr, 0.9, 0.999, 1e-8, 0, nullptr) == EFFI_ERR_BADARG);
    EXPECT(effi_adamw_multi_f32(all.p.data(), all.g.data(), all.m.data(), all.v.data(), nullptr, nm, K, 1e-3, nullptr, 0.9, 0.999, 1e-8, 0, nullptr) == EFFI_ERR_BADARG);
    EXPECT(effi_adamw_multi_f32(all.p.data(), all.g.data(), all.m.data(), all.v.data(), all.step.data(), nullptr, K, 1e-3, nullptr, 0.9, 0.999, 1e-8, 0, nullptr) == EFFI_ERR_BADARG);
    for (int which = 0; which < 5; ++which)
        for (int i : {0, K - 1}) {
            Lists bad(full);
            if (which == 0) bad.p[i] = nullptr;
            if (which == 1) bad.g[i] = nullptr;
            if (which == 2) bad.m[i] = nullptr;
            if (which == 3) bad.v[i] = nullptr;
            if (which == 4) bad.step[i] = nullptr;
            EXPECT(bad.call(K) == EFFI_ERR_BADARG);
        }
    {
        Lists bad(full);
        bad.numel[K - 1] = -1;
        EXPECT(bad.call(K) == EFFI_ERR_BADARG);
        // a null pointer or a negative size PAST n is not looked at
        Lists tail(full);
        tail.p[K - 1] = nullptr, tail.numel[K - 1] = -5;
        if (K > 1) EXPECT(tail.call(K - 1) == EFFI_OK);
    }
    {
        // chunk counts that overflow the grid: two tensors of 2^41 elements are 2^31 chunks together
        Lists big({1L << 41, 1L << 41});
        EXPECT(big.call(1) == EFFI_OK);
        EXPECT(big.call(2) == EFFI_ERR_BADARG);
        Lists huge({LONG_MAX});
        EXPECT(huge.call(1) == EFFI_ERR_BADARG);
    }

    // the chunks of the packed table cover every element exactly once
    check_cover(edge);
    for (long s : edge) check_cover({s});
    {
        std::vector<long> rev(edge.rbegin(), edge.rend());      // the empty tensor first
        check_cover(rev);
        check_cover({0, 0, 5, 0, AW_CHUNK, 0});
        std::vector<long> fullc(K);
        for (int i = 0; i < K; ++i) fullc[i] = edge[(i * 3) % edge.size()];
        check_cover(fullc);
    }
    {
        // all tensors empty: no update launch, chunks = 0
        Lists l({0, 0});
        AdamWArgs a;
        int chunks = -1;
        EXPECT(aw_pack(l.p.data(), l.g.data(), l.m.data(), l.v.data(), l.step.data(), l.numel.data(), 2, 1e-3, nullptr, 0.9, 0.999, 1e-8, 0,
                       &a, &chunks) == EFFI_OK && chunks == 0);
        EXPECT(l.call(2) == EFFI_OK);
    }
    check_clipped_entry(full);
    check_gradnorm(edge);
    std::printf(failures ? "optim host check: %d FAILED\n" : "optim host check: ok\n", failures);
    return failures ? 1 : 0;
}
