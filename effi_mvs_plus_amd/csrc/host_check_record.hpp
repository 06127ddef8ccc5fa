// The launch recorder of the stand-alone host checks (conv_host_check.cpp, warp_host_check.cpp, vol_host_check.cpp).  Include it BEFORE the .hip files
// under test: from here on hipLaunchKernelGGL appends a record to g_rec instead of launching -- kernel instantiation, grid, block and
// each by-value argument, field by field -- and the error queries answer hipSuccess.  The stand-ins for what api.hip gives the library
// (zero page, option table) are here too.  A program adds a show_one overload per argument struct of its kernels, in the namespace of
// the struct (the generic show finds it by argument-dependent lookup), and its case table.
#pragma once
#include "common.hpp"

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cxxabi.h>
#include <string>
#include <type_traits>
#include <typeinfo>

static std::string g_rec;                      // the launches of the case that runs
static void put(const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_rec += buf;
}
static std::string L(const char* fmt, ...) {
    char buf[256];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    return buf;
}

template <auto K> struct kernel_tag {};
template <class T> static void show(const T& v);
template <auto K, class... A>
static void rec_launch(dim3 grid, dim3 block, size_t shmem, const A&... args) {
    int status = 0;
    char* name = abi::__cxa_demangle(typeid(kernel_tag<K>).name(), nullptr, nullptr, &status);
    std::string k = name ? name : "?";                          // "kernel_tag<&(anonymous namespace)::f<...>>" -> "f<...>"
    std::free(name);
    if (const size_t amp = k.find('&'); amp != std::string::npos) k = k.substr(amp + 1, k.size() - amp - 2);
    for (size_t at; (at = k.find("(anonymous namespace)::")) != std::string::npos;) k.erase(at, 23);
    if (k.rfind("(void ", 0) == 0) k.erase(0, 6);               // "(void f<...>(Args...))" -> "f<...>"
    else if (k.rfind("(", 0) == 0) k.erase(0, 1);               // "(f(Args...))", a global kernel that is no template -> "f"
    const size_t gt = k.rfind('>');
    if (const size_t par = k.find('(', gt == std::string::npos ? 0 : gt); par != std::string::npos) k.erase(par);
    put(" || %s grid %u,%u,%u block %u shmem %zu", k.c_str(), grid.x, grid.y, grid.z, block.x, shmem);
    ((put(" |"), show(args)), ...);
}

#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(kernel, grid, block, shmem, stream, ...) rec_launch<(kernel)>(dim3(grid), dim3(block), (shmem), __VA_ARGS__)
#define hipPeekAtLastError() hipSuccess
#define hipGetLastError() hipSuccess

// ---- what api.hip gives the library: the zero page and the option table ----------------------------------------------------------
static const uintptr_t kBase = 0x100000000UL;                   // fake device addresses: kBase + k * 0x100
template <class T = float> static T* P(int k) { return reinterpret_cast<T*>(kBase + 0x100UL * (unsigned)k); }
static bool g_have_zero_page = true;
const float* effi_zero_page() { return g_have_zero_page ? P(99) : nullptr; }
static long g_opt[EFFI_OPT_COUNT];
long effi_option(int id) { return g_opt[id]; }
struct Opt {                                                    // an option for the length of a scope
    int id;
    Opt(int i, long v) : id(i) { g_opt[i] = v; }
    ~Opt() { g_opt[id] = EFFI_OPT_UNSET; }
};

// ---- printing ---------------------------------------------------------------------------------------------------------------------
// A struct's fields that are 0 / null are left out of its line (an unset one is 0xAA.. under the pattern initialisation and shows).
static void ptr(const char* n, const void* p) {
    const uintptr_t v = reinterpret_cast<uintptr_t>(p);
    if (!p) return;
    if (v >= kBase && v < kBase + (1UL << 32)) put(" %s=@%lx", n, (unsigned long)(v - kBase));
    else put(" %s=0x%lx", n, (unsigned long)v);
}
#define FI(s, f) ((s).f != 0 ? put(" " #f "=%ld", (long)(s).f) : (void)0)
#define FP(s, f) ptr(#f, (s).f)
template <class T> static void show(const T& v) {
    if constexpr (std::is_null_pointer_v<T>) put(" null");      // (a literal nullptr among the arguments)
    else if constexpr (std::is_pointer_v<T>) v ? ptr("ptr", v) : put(" null");
    else if constexpr (std::is_integral_v<T>) put(" %ld", (long)v);
    else show_one(v);
}

// ---- a case's line: entry | label | return code || launch || launch ... -----------------------------------------------------------
static int g_failures = 0;
static const char* rc_name(int rc) {
    switch (rc) {
        case EFFI_OK: return "OK";
        case EFFI_ERR_BADARG: return "BADARG";
        case EFFI_ERR_UNSUPPORTED: return "UNSUPPORTED";
        case EFFI_ERR_WORKSPACE: return "WORKSPACE";
        case EFFI_ERR_LAUNCH: return "LAUNCH";
        default: return "?";
    }
}
static void emit(const char* entry, const std::string& label, int rc) {
    if (rc != EFFI_OK && !g_rec.empty()) { std::printf("FAILED: %s | %s launched and returned %s\n", entry, label.c_str(), rc_name(rc)); ++g_failures; }
    if (rc == EFFI_OK && g_rec.empty()) { std::printf("FAILED: %s | %s returned OK without a launch\n", entry, label.c_str()); ++g_failures; }
    std::printf("%s | %s | %s%s\n", entry, label.c_str(), rc_name(rc), g_rec.c_str());
}
// RUNF: call an entry, print its line
#define RUNF(fn, label, ...) do { g_rec.clear(); const int rc_ = fn(__VA_ARGS__); emit(#fn, (label), rc_); } while (0)
