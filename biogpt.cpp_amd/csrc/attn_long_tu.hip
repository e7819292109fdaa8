// Translation unit of the long-context attention (kernels_attn_long.hip.h): attn_long_col_kernel and attn_long_tile_kernel, head size 64 at 1025 .. 2048 keys.
// Same arrangement as wchunk_tu.hip: own namespace name for the headers' non-inline kernels, the parameter block crosses as bytes; built with
// -ffp-contract=off (Makefile: the unit's own flag, whatever CXXFLAGS says).
#define bgk bgk_al
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <mutex>
#include <set>
#include <utility>

#include "kernels_attn_long.hip.h"

namespace {

std::mutex g_attr_mu;
std::set<int> g_attr_done;      // devices on which the tile kernel's > 64 KB dynamic-LDS opt-in attribute is set

// the most dynamic LDS of a workgroup on the current device, as the device reports it
hipError_t device_lds_limit(size_t &limit) {
    static thread_local int known_dev = -1;
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

}  // namespace

// six words of a launch: form (0 column, 1 tile), threads, grid x, grid y, LDS bytes, t_cap; non-zero: a shape the kernels do not hold (no HIP call)
extern "C" int bg_attn_long_geometry(int form, int H, int N, int t_cap, int32_t *six) {
    if ((form != 0 && form != 1) || H < 1 || N < 1 || t_cap < 1 || t_cap > bgk::LONG_ATTN_MAX_KEYS) return (int)hipErrorInvalidValue;
    if (six) {
        six[0] = form; six[1] = bgk::LONG_ATTN_THREADS; six[2] = H; six[3] = form ? (N + bgk::LONG_TILE_COLS - 1) / bgk::LONG_TILE_COLS : N;
        six[4] = form ? (int32_t)bgk::attn_long_tile_smem_bytes(t_cap) : bgk::LONG_COL_LDS_BYTES; six[5] = t_cap;
    }
    return 0;
}

// 1: the current device's opt-in LDS limit holds the tile kernel's workgroup at t_cap keys; 0: it does not; < 0: minus the HIP error of asking
extern "C" int bg_attn_long_tile_fits(int t_cap) {
    size_t limit = 0;
    const hipError_t e = device_lds_limit(limit);
    if (e != hipSuccess) return -(int)e;
    return t_cap >= 1 && t_cap <= bgk::LONG_ATTN_MAX_KEYS && bgk::attn_long_tile_smem_bytes(t_cap) <= limit ? 1 : 0;
}

// params: a bgk::AttnParams over a device state (no column states), head size 64, t_cap <= min(P, 2048); report: null, or the six words of bg_attn_long_geometry
extern "C" int bg_attn_long_launch(int form, const void *params, size_t params_bytes, int H, int N, hipStream_t st, int32_t *report) {
    if (!params || params_bytes != sizeof(bgk::AttnParams)) return (int)hipErrorInvalidValue;
    const bgk::AttnParams &p = *static_cast<const bgk::AttnParams *>(params);
    if (p.seq || !p.st || !p.q || !p.kcache || !p.vcache || !p.out || !p.exp_tab || p.dk != 64 || p.D != H * 64 || p.N != N || p.t_cap > p.P) return (int)hipErrorInvalidValue;
    int32_t six[6];
    if (bg_attn_long_geometry(form, H, N, p.t_cap, six)) return (int)hipErrorInvalidValue;
    if (report) for (int i = 0; i < 6; i++) report[i] = six[i];
    const dim3 grid(six[2], six[3]), block(six[1]);
    if (form == 0) {
        hipLaunchKernelGGL(bgk::attn_long_col_kernel, grid, block, 0, st, p);
        return (int)hipGetLastError();
    }
    size_t limit = 0;
    hipError_t e = device_lds_limit(limit);
    if (e != hipSuccess) return (int)e;
    if ((size_t)six[4] > limit) return (int)hipErrorInvalidValue;
    {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess) return (int)hipErrorInvalidDevice;
        std::lock_guard<std::mutex> lk(g_attr_mu);
        if (!g_attr_done.count(dev)) {      // once, for every key count of this device
            const size_t most = std::min(limit, bgk::attn_long_tile_smem_bytes(bgk::LONG_ATTN_MAX_KEYS));
            e = hipFuncSetAttribute(reinterpret_cast<const void *>(bgk::attn_long_tile_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)most);
            if (e != hipSuccess) return (int)e;
            g_attr_done.insert(dev);
        }
    }
    hipLaunchKernelGGL(bgk::attn_long_tile_kernel, grid, block, (size_t)six[4], st, p);
    return (int)hipGetLastError();
}
