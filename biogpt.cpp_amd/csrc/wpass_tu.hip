// Translation unit of the wide pass layer (kernels_wpass.hip.h): passes of 9 or more of the context's own columns of a block-quantized file that is not
// BioGPT-base -- 5 block formats x {q/k/v, residual, fc1 with its Q8 hand-off, logits} x {1, 2 column tiles per wave} x {1, 4 waves per workgroup} = 80
// kernels.  Same arrangement as wchunk_tu.hip: own namespace name for the headers' non-inline kernels, the parameter block crosses as bytes, and the unit is
// built without packed f32 instructions (Makefile).
#define bgk bgk_wp
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <mutex>
#include <set>
#include <utility>

#include "kernels_wpass.hip.h"

namespace {

struct Geo { int ct, wpb, grid_x, grid_y, lds; };
struct DevLimits { size_t lds; int cus; };      // the most dynamic LDS of a workgroup and the compute units, as the device reports them

std::mutex g_attr_mu;
std::set<std::pair<int, const void *>> g_attr_done;      // (device, kernel): > 64 KB of dynamic LDS needs the opt-in attribute once per device

// The launch shape of a stage at (M, K) for N columns.
//   CT: two column tiles per wave wherever the pass has more than 16 columns (one A operand and one quad of row scales for two MFMAs); one where 16 columns
//       are all there is, or where the device's LDS does not hold two buffers of 32 columns.
//   WPB: four waves per workgroup share one staged copy of the columns where that still leaves a workgroup per compute unit (units x column groups >= 4 x
//       compute units); below that every wave is a workgroup of its own, so that a pass of 9 .. 32 columns puts its 100 row tiles of out_proj / fc2 on 100
//       compute units and not on 25.
// cfg -1: the rule; 11, 14, 21, 24: CT and WPB as given (the probe and the tests: every instantiation at any shape -- a second column tile without live columns re-reads
// column N - 1 and stores nothing).  lim.lds 0: the LDS request is not held against a device; lim.cus 0: taken as 256.  false: a shape the kernels do not hold.
bool geometry(int epi, int M, int K, int N, bool q81, DevLimits lim, int cfg, Geo &g) {
    if (cfg != -1 && cfg != 11 && cfg != 14 && cfg != 21 && cfg != 24) return false;
    if (epi != bgk::EPI_QKV && epi != bgk::EPI_RESID && epi != bgk::EPI_GELU_Q8 && epi != bgk::EPI_LOGITS) return false;
    if (N < bgk::WPASS_MIN_COLS || M < 1 || K < bgk::QK || K % bgk::QK != 0) return false;
    if (epi != bgk::EPI_LOGITS && M % (epi == bgk::EPI_GELU_Q8 ? 32 : 16) != 0) return false;
    if (epi == bgk::EPI_QKV && (M != 3 * K || K % 64 != 0)) return false;
    const int cus = lim.cus > 0 ? lim.cus : 256;
    g.ct = cfg > 0 ? cfg / 10 : N > 16 ? 2 : 1;
    if (cfg < 0 && lim.lds && bgk::wpass_smem_bytes(q81, g.ct, K) > lim.lds) g.ct = 1;
    const size_t lds = bgk::wpass_smem_bytes(q81, g.ct, K);
    if (lim.lds && lds > lim.lds) return false;
    const int tiles = (M + 15) / 16, units = epi == bgk::EPI_GELU_Q8 ? tiles / 2 : tiles;
    g.grid_y = (N + 16 * g.ct - 1) / (16 * g.ct);
    g.wpb = cfg > 0 ? cfg % 10 : (long)units * g.grid_y >= 4L * cus ? 4 : 1;
    g.grid_x = (units + g.wpb - 1) / g.wpb;
    if (g.grid_y > 65535) return false;
    g.lds = (int)lds;
    return true;
}

hipError_t device_limits(DevLimits &lim) {
    static thread_local int known_dev = -1;      // (asked once per thread and device: every stage launch comes through here)
    static thread_local DevLimits known{0, 0};
    int dev = 0, v = 0, cus = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e == hipSuccess && dev == known_dev) { lim = known; return hipSuccess; }
    if (e == hipSuccess) e = hipDeviceGetAttribute(&v, hipDeviceAttributeSharedMemPerBlockOptin, dev);
    if (e == hipSuccess && v < 64 * 1024) e = hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, dev);
    if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    lim = e == hipSuccess ? DevLimits{(size_t)v, cus} : DevLimits{0, 0};
    if (e == hipSuccess) { known_dev = dev; known = lim; }
    return e;
}

template <class Kernel>
hipError_t launch_k(Kernel kernel, const bgk::WpassParams &p, const Geo &g, size_t lds_limit, hipStream_t st) {
    if (g.lds > 64 * 1024) {
        const void *fn = reinterpret_cast<const void *>(kernel);
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess) return hipErrorInvalidDevice;
        std::lock_guard<std::mutex> lk(g_attr_mu);
        if (!g_attr_done.count({dev, fn})) {
            const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_limit);
            if (e != hipSuccess) return e;
            g_attr_done.insert({dev, fn});
        }
    }
    hipLaunchKernelGGL(kernel, dim3(g.grid_x, g.grid_y), dim3(64 * g.wpb), g.lds, st, p);
    return hipGetLastError();
}

template <int WT, int EPI>
hipError_t launch_e(const bgk::WpassParams &p, const Geo &g, size_t lds_limit, hipStream_t st) {
    if (g.ct == 2) return g.wpb == 4 ? launch_k(bgk::wpass_kernel<WT, EPI, 2, 4>, p, g, lds_limit, st) : launch_k(bgk::wpass_kernel<WT, EPI, 2, 1>, p, g, lds_limit, st);
    return g.wpb == 4 ? launch_k(bgk::wpass_kernel<WT, EPI, 1, 4>, p, g, lds_limit, st) : launch_k(bgk::wpass_kernel<WT, EPI, 1, 1>, p, g, lds_limit, st);
}

template <int WT>
hipError_t launch_t(int epi, const bgk::WpassParams &p, const Geo &g, size_t lds_limit, hipStream_t st) {
    switch (epi) {
        case bgk::EPI_QKV: return launch_e<WT, bgk::EPI_QKV>(p, g, lds_limit, st);
        case bgk::EPI_RESID: return launch_e<WT, bgk::EPI_RESID>(p, g, lds_limit, st);
        case bgk::EPI_GELU_Q8: return launch_e<WT, bgk::EPI_GELU_Q8>(p, g, lds_limit, st);
        case bgk::EPI_LOGITS: return launch_e<WT, bgk::EPI_LOGITS>(p, g, lds_limit, st);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace

// six words of a stage's launch at (M, K) for N columns: column tiles per wave, waves per workgroup, grid x, grid y, LDS bytes, the compute units the rule
// counted (256 where no device was asked); cfg: -1 the rule, or 10 CT + WPB; non-zero: the kernels do
// not hold the shape.  epi: EPI_QKV 0, EPI_RESID 1, EPI_GELU_Q8 4 (fc1), EPI_LOGITS 3.  lds_limit: bytes of dynamic LDS a workgroup may have; 0: the request is
// not held against a device and 256 compute units are assumed (no HIP call); < 0: the current device's LDS and compute units
extern "C" int bg_wpass_geometry(int epi, int M, int K, int N, int q81, int64_t lds_limit, int cfg, int32_t *six) {
    Geo g{};
    DevLimits lim{lds_limit > 0 ? (size_t)lds_limit : 0, 0};
    if (lds_limit < 0) { const hipError_t e = device_limits(lim); if (e != hipSuccess) return (int)e; }
    if (!geometry(epi, M, K, N, q81 != 0, lim, cfg, g)) return (int)hipErrorInvalidValue;
    if (six) { six[0] = g.ct; six[1] = g.wpb; six[2] = g.grid_x; six[3] = g.grid_y; six[4] = g.lds; six[5] = lim.cus > 0 ? lim.cus : 256; }
    return 0;
}

// wt: the kernels' WType value (2, 3, 6, 7, 8); params: a bgk::WpassParams (M, K, N, the image and the site's pointers).  cfg: -1 the rule (the engine), or 10 CT + WPB.  report: null, or the six words of
// bg_wpass_geometry
extern "C" int bg_wpass_launch(int wt, int epi, const void *params, size_t params_bytes, int cfg, hipStream_t st, int32_t *report) {
    if (!params || params_bytes != sizeof(bgk::WpassParams)) return (int)hipErrorInvalidValue;
    const bgk::WpassParams &p = *static_cast<const bgk::WpassParams *>(params);
    const bool q81 = wt == bgk::W_Q4_1 || wt == bgk::W_Q5_1;
    Geo g{};
    DevLimits lim{0, 0};
    const hipError_t e = device_limits(lim);
    if (e != hipSuccess) return (int)e;
    if (!p.img_q || !p.img_s || !geometry(epi, p.M, p.K, p.N, q81, lim, cfg, g)) return (int)hipErrorInvalidValue;
    if (epi == bgk::EPI_QKV && p.K != p.D) return (int)hipErrorInvalidValue;
    if (report) { report[0] = g.ct; report[1] = g.wpb; report[2] = g.grid_x; report[3] = g.grid_y; report[4] = g.lds; report[5] = lim.cus; }
    switch (wt) {
        case bgk::W_Q4_0: return (int)launch_t<bgk::W_Q4_0>(epi, p, g, lim.lds, st);
        case bgk::W_Q4_1: return (int)launch_t<bgk::W_Q4_1>(epi, p, g, lim.lds, st);
        case bgk::W_Q5_0: return (int)launch_t<bgk::W_Q5_0>(epi, p, g, lim.lds, st);
        case bgk::W_Q5_1: return (int)launch_t<bgk::W_Q5_1>(epi, p, g, lim.lds, st);
        case bgk::W_Q8_0: return (int)launch_t<bgk::W_Q8_0>(epi, p, g, lim.lds, st);
        default: return (int)hipErrorInvalidValue;
    }
}
