// What the stand-alone host programs of the definitions share (cloud_host.cpp, cloud_flow_host.cpp, cloud_objects_host.cpp,
// depth_host.cpp): reading the case file, buffers of exactly the size a case passes, and the frame around the cases.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstdlib>

template <typename T>
static bool get(FILE* f, T* v, size_t n = 1) { return fread(v, sizeof(T), n, f) == n; }

// count elements and not a byte more (one element for an empty array, so that the pointer is not null): a read or write past it is
// the sanitizer's to report
template <typename T>
static T* exactly(size_t count) { return static_cast<T*>(malloc((count ? count : 1) * sizeof(T))); }

// main of `NAME IN OUT`: IN starts with int32 n_cases; one_case(in, out) reads one case and writes its answer, false: IN is malformed
template <class F>
static int run_cases(int argc, char** argv, const char* name, F&& one_case) {
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    int32_t n_cases = 0;
    if (!get(in, &n_cases)) return 2;
    for (int32_t c = 0; c < n_cases; ++c)
        if (!one_case(in, out)) return 2;
    fclose(in);
    fclose(out);
    printf("%s: done\n", name);
    return 0;
}
