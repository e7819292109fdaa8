// Translation unit of the wide chunk layer (kernels_wchunk.hip.h): evals of 2 .. 8 tokens of a block-quantized file that is not BioGPT-base -- 5 block formats
// x {q/k/v, out_proj / fc2, fc1} = 15 kernels.  Same arrangement as wdecode_tu.hip: own namespace name for the headers' non-inline kernels, the parameter
// block crosses as bytes, and the unit is built without packed f32 instructions (Makefile).
#define bgk bgk_wc
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <mutex>
#include <set>
#include <utility>

#include "kernels_wchunk.hip.h"

namespace {

enum : int { WS_QKV = 0, WS_OPROJ = 2, WS_FC1 = 3, WS_FC2 = 4 };      // the wide decode layer's stage numbers (1 is its attention launch)
struct Geo { int threads, grid, lds, max_rows; };

std::mutex g_attr_mu;
std::set<std::pair<int, const void *>> g_attr_done;      // (device, kernel): > 64 KB of dynamic LDS needs the opt-in attribute once per device

// The launch shape of a linear stage at (M, K) for N columns: wdecode_tu.hip's rule for the grid and the rows, a finisher thread per (row, column), and the
// N columns' blocks and terms in LDS.  lds_limit: the most dynamic LDS a workgroup gets on the device (0: not asked).  false: a shape the kernels do not hold.
bool geometry(int stage, int M, int K, int N, size_t lds_limit, Geo &g) {
    if (stage != WS_QKV && stage != WS_OPROJ && stage != WS_FC1 && stage != WS_FC2) return false;
    if (N < bgk::WCHUNK_MIN_COLS || N > bgk::WCHUNK_MAX_COLS || M < 1 || K < bgk::QK || K % bgk::QK != 0) return false;
    const int bpr = K / bgk::QK;
    if (stage == WS_FC1) {
        if (M % bgk::WDEC_FC1_ROWS != 0) return false;
        g.grid = M / bgk::WDEC_FC1_ROWS; g.max_rows = bgk::WDEC_FC1_ROWS;
    } else {
        const int min_rows = (64 + bpr - 1) / bpr;      // a wave of units at least
        g.grid = std::min(256, std::max(1, M / min_rows));
        g.max_rows = (M + g.grid - 1) / g.grid;
    }
    const int units = g.max_rows * bpr, passes = (units + 1023) / 1024;
    g.threads = (((units + passes - 1) / passes) + 63) & ~63;
    g.threads = std::max(g.threads, (g.max_rows * N + 63) & ~63);      // a finisher thread per (row, column)
    if (g.threads > 1024) return false;
    const size_t lds = bgk::wchunk_smem_bytes(stage == WS_FC1, N, K, g.max_rows);
    if (lds > (size_t)INT32_MAX || (lds_limit && lds > lds_limit)) return false;
    g.lds = (int)lds;
    return true;
}

// the most dynamic LDS of a workgroup on the current device, as the device reports it
hipError_t device_lds_limit(size_t &limit) {
    static thread_local int known_dev = -1;      // (asked once per thread and device: every stage launch comes through here)
    static thread_local size_t known = 0;
    int dev = 0, v = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e == hipSuccess && dev == known_dev) { limit = known; return hipSuccess; }
    if (e == hipSuccess) e = hipDeviceGetAttribute(&v, hipDeviceAttributeSharedMemPerBlockOptin, dev);
    if (e == hipSuccess && v < 64 * 1024) e = hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, dev);
    limit = e == hipSuccess ? (size_t)v : 0;
    if (e == hipSuccess) { known_dev = dev; known = limit; }
    return e;
}

template <class Kernel>
hipError_t launch_k(Kernel kernel, const bgk::WchunkParams &p, const Geo &g, size_t lds_limit, hipStream_t st) {
    if (g.lds > 64 * 1024) {
        const void *fn = reinterpret_cast<const void *>(kernel);
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess) return hipErrorInvalidDevice;
        std::lock_guard<std::mutex> lk(g_attr_mu);
        if (!g_attr_done.count({dev, fn})) {      // once, for everything the geometry can ask of this device
            const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_limit);
            if (e != hipSuccess) return e;
            g_attr_done.insert({dev, fn});
        }
    }
    hipLaunchKernelGGL(kernel, dim3(g.grid), dim3(g.threads), g.lds, st, p);
    return hipGetLastError();
}

template <int WT>
hipError_t launch_t(int stage, const bgk::WchunkParams &p, const Geo &g, size_t lds_limit, hipStream_t st) {
    if (stage == WS_QKV) return launch_k(bgk::wchunk_qkv_kernel<WT>, p, g, lds_limit, st);
    if (stage == WS_FC1) return launch_k(bgk::wchunk_fc1_kernel<WT>, p, g, lds_limit, st);
    return launch_k(bgk::wchunk_resid_kernel<WT>, p, g, lds_limit, st);
}

}  // namespace

// four words of a linear stage's launch at (M, K) for N columns: threads, grid, LDS bytes, most rows of a workgroup; non-zero: the kernels do not hold the
// shape.  lds_limit: bytes of dynamic LDS a workgroup may have; 0: the LDS request is not held against a device (no HIP call); < 0: the current device's
extern "C" int bg_wchunk_geometry(int stage, int M, int K, int N, int64_t lds_limit, int32_t *four) {
    Geo g{};
    size_t limit = lds_limit > 0 ? (size_t)lds_limit : 0;
    if (lds_limit < 0) { const hipError_t e = device_lds_limit(limit); if (e != hipSuccess) return (int)e; }
    if (!geometry(stage, M, K, N, limit, g)) return (int)hipErrorInvalidValue;
    if (four) { four[0] = g.threads; four[1] = g.grid; four[2] = g.lds; four[3] = g.max_rows; }
    return 0;
}

// wt: the kernels' WType value (2, 3, 6, 7, 8); stage: 0 q/k/v, 2 out_proj, 3 fc1, 4 fc2; params: a bgk::WchunkParams with W, N and the stage's pointers (bpr,
// pstride and max_rows are set here); q/k/v needs W.M == 3 D, W.K == D, 64 | D.  report: null, or the four words of bg_wchunk_geometry
extern "C" int bg_wchunk_launch(int wt, int stage, const void *params, size_t params_bytes, hipStream_t st, int32_t *report) {
    if (!params || params_bytes != sizeof(bgk::WchunkParams)) return (int)hipErrorInvalidValue;
    bgk::WchunkParams p = *static_cast<const bgk::WchunkParams *>(params);
    Geo g{};
    size_t limit = 0;
    const hipError_t e = device_lds_limit(limit);
    if (e != hipSuccess) return (int)e;
    if (!geometry(stage, p.W.M, p.W.K, p.N, limit, g)) return (int)hipErrorInvalidValue;
    if (stage == WS_QKV && (p.W.K != p.D || p.W.M != 3 * p.D || p.D % 64 != 0)) return (int)hipErrorInvalidValue;
    p.bpr = p.W.K / bgk::QK; p.pstride = bgk::wdec_pstride(p.bpr); p.max_rows = g.max_rows;
    if (report) { report[0] = g.threads; report[1] = g.grid; report[2] = g.lds; report[3] = g.max_rows; }
    switch (wt) {
        case bgk::W_Q4_0: return (int)launch_t<bgk::W_Q4_0>(stage, p, g, limit, st);
        case bgk::W_Q4_1: return (int)launch_t<bgk::W_Q4_1>(stage, p, g, limit, st);
        case bgk::W_Q5_0: return (int)launch_t<bgk::W_Q5_0>(stage, p, g, limit, st);
        case bgk::W_Q5_1: return (int)launch_t<bgk::W_Q5_1>(stage, p, g, limit, st);
        case bgk::W_Q8_0: return (int)launch_t<bgk::W_Q8_0>(stage, p, g, limit, st);
        default: return (int)hipErrorInvalidValue;
    }
}
