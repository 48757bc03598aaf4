// The HIP calls that the host-only headers under csrc/ use, defined for the stand-alone host
// checks (device_mem_check.cpp, pair_outputs_check.cpp; no GPU): a fake allocator that records
// sizes, can fail the n-th hipMalloc, and aborts when asked to free a pointer it does not hold.
// Include it in one translation unit per program.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <vector>

namespace {
std::map<void*, size_t> g_dev, g_pin;  // live allocations
std::vector<size_t> g_mallocs;         // byte counts of the hipMalloc calls, in order (failed ones too)
int g_fail_at = -1;                    // fail the hipMalloc call with this index in g_mallocs
int g_syncs = 0, g_frees = 0;
std::vector<int> g_devices;            // the hipSetDevice calls

[[noreturn]] void die(const char* what, int line) {
    std::fprintf(stderr, "host check: %s (line %d)\n", what, line);
    std::abort();
}
#define CHECK(c) \
    if (!(c)) die(#c, __LINE__)

void reset_log() {
    g_mallocs.clear();
    g_devices.clear();
    g_fail_at = -1;
    g_syncs = g_frees = 0;
}
}  // namespace

extern "C" {
hipError_t hipMalloc(void** p, size_t n) {
    const bool fail = (int)g_mallocs.size() == g_fail_at;
    g_mallocs.push_back(n);
    if (fail) return hipErrorOutOfMemory;
    *p = std::malloc(n ? n : 1);
    g_dev[*p] = n;
    return hipSuccess;
}
hipError_t hipFree(void* p) {
    if (!g_dev.erase(p)) die("hipFree of a pointer that is not live", __LINE__);
    std::free(p);
    ++g_frees;
    return hipSuccess;
}
hipError_t hipHostMalloc(void** p, size_t n, unsigned int) {
    *p = std::malloc(n ? n : 1);
    g_pin[*p] = n;
    return hipSuccess;
}
hipError_t hipHostFree(void* p) {
    if (!g_pin.erase(p)) die("hipHostFree of a pointer that is not live", __LINE__);
    std::free(p);
    return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t) {
    ++g_syncs;
    return hipSuccess;
}
hipError_t hipMemcpyAsync(void* dst, const void* src, size_t n, hipMemcpyKind, hipStream_t) {
    std::memcpy(dst, src, n);
    return hipSuccess;
}
hipError_t hipSetDevice(int device) {
    g_devices.push_back(device);
    return hipSuccess;
}
}
