// Translation unit of the wide column layer (kernels_wcols.hip.h): the wide chain's linear stage for passes of 1 .. 16 column states -- 5 block formats x
// {q/k/v, residual, GELU, logits} x {4, 8 waves} = 40 kernels.  Same arrangement as mfma_wide_tu.hip: own namespace name for the headers' non-inline kernels,
// the parameter blocks cross as bytes; built with -ffp-contract=off (Makefile: the unit's own flag, whatever CXXFLAGS says).
#define bgk bgk_wcl
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "kernels_wcols.hip.h"

namespace {

struct Geo { int nw, threads, grid, lds, rounds; };

// The launch shape at (M, K) for N columns.  nw: 0 the rule (8 waves where a row has more than 32 blocks, so that a round of 8 x 4 blocks is full; otherwise 4),
// or 4 / 8 forced.  lds_limit: the most dynamic LDS a workgroup gets on the device (0: not asked).  false: a shape the kernels do not hold.
bool geometry(int epi, int M, int K, int N, int nw, size_t lds_limit, Geo &g) {
    if (epi != bgk::EPI_QKV && epi != bgk::EPI_RESID && epi != bgk::EPI_GELU && epi != bgk::EPI_LOGITS) return false;
    if (N < 1 || N > bgk::WCOLS_MAX_COLS || M < 1 || M > (1 << 24) || K < bgk::QK || K % bgk::QK != 0 || (nw != 0 && nw != 4 && nw != 8)) return false;
    if (epi != bgk::EPI_LOGITS && M % 16 != 0) return false;
    if (epi == bgk::EPI_QKV && (M != 3 * K || K % 64 != 0)) return false;
    const int bpr = K / bgk::QK;
    g.nw = nw ? nw : (bpr > 32 ? 8 : 4);
    g.threads = 64 * g.nw;
    g.grid = (M + 15) / 16;
    g.lds = (int)bgk::wcols_smem_bytes(g.nw);
    g.rounds = (bpr + g.nw * bgk::WCOLS_R - 1) / (g.nw * bgk::WCOLS_R);
    return !(lds_limit && (size_t)g.lds > lds_limit);
}

// the dynamic LDS a launch gets without an attribute of its own, or less where the device reports less
hipError_t device_lds_limit(size_t &limit) {
    static thread_local int known_dev = -1;      // (asked once per thread and device: every stage launch comes through here)
    static thread_local size_t known = 0;
    int dev = 0, v = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e == hipSuccess && dev == known_dev) { limit = known; return hipSuccess; }
    if (e == hipSuccess) e = hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, dev);
    limit = e == hipSuccess ? std::min((size_t)v, (size_t)65536) : 0;
    if (e == hipSuccess) { known_dev = dev; known = limit; }
    return e;
}

template <int WT, int EPI>
hipError_t launch_one(const bgk::MatvecParams &p, const bgk::DevMatrix &img, const Geo &g, hipStream_t st) {
    if (g.nw == 8) hipLaunchKernelGGL((bgk::wcols_kernel<WT, EPI, 8>), dim3(g.grid), dim3(g.threads), g.lds, st, p, img);
    else hipLaunchKernelGGL((bgk::wcols_kernel<WT, EPI, 4>), dim3(g.grid), dim3(g.threads), g.lds, st, p, img);
    return hipGetLastError();
}

template <int WT>
hipError_t launch_t(int epi, const bgk::MatvecParams &p, const bgk::DevMatrix &img, const Geo &g, hipStream_t st) {
    switch (epi) {
        case bgk::EPI_QKV: return launch_one<WT, bgk::EPI_QKV>(p, img, g, st);
        case bgk::EPI_RESID: return launch_one<WT, bgk::EPI_RESID>(p, img, g, st);
        case bgk::EPI_GELU: return launch_one<WT, bgk::EPI_GELU>(p, img, g, st);
        case bgk::EPI_LOGITS: return launch_one<WT, bgk::EPI_LOGITS>(p, img, g, st);
        default: return hipErrorInvalidValue;
    }
}

void report_geo(const Geo &g, int32_t *five) {
    if (five) { five[0] = g.nw; five[1] = g.threads; five[2] = g.grid; five[3] = g.lds; five[4] = g.rounds; }
}

}  // namespace

// five words of a stage's launch at (M, K) for N columns: waves, threads, grid, LDS bytes, rounds; non-zero: the kernels do not hold the shape (1 <= N <= 16,
// 32 | K, 16 | M but at the logits site, q/k/v 3 K x K with 64 | K).  epi: EPI_QKV 0, EPI_RESID 1, EPI_GELU 2, EPI_LOGITS 3.  nw: 0 the rule, 4 or 8 forced.
// lds_limit: bytes of dynamic LDS a workgroup may have; 0: the LDS request is not held against a device (no HIP call); < 0: the current device's
extern "C" int bg_wcols_geometry(int epi, int M, int K, int N, int nw, int64_t lds_limit, int32_t *five) {
    Geo g{};
    size_t limit = lds_limit > 0 ? (size_t)lds_limit : 0;
    if (lds_limit < 0) { const hipError_t e = device_lds_limit(limit); if (e != hipSuccess) return (int)e; }
    if (!geometry(epi, M, K, N, nw, limit, g)) return (int)hipErrorInvalidValue;
    report_geo(g, five);
    return 0;
}

// wt: the kernels' WType value (2, 3, 6, 7, 8); params: a bgk::MatvecParams as bg_wide_launch takes it (N <= 16; aq_* the columns' Q8 blocks); img: the
// row-tiled image with ceil(M / 16) tiles (the last one zero-padded).  report: null, or the five words of bg_wcols_geometry
extern "C" int bg_wcols_launch(int wt, int epi, const void *params, size_t params_bytes, const void *img, size_t img_bytes, int nw, hipStream_t st, int32_t *report) {
    if (!params || !img || params_bytes != sizeof(bgk::MatvecParams) || img_bytes != sizeof(bgk::DevMatrix)) return (int)hipErrorInvalidValue;
    const bgk::MatvecParams &p = *static_cast<const bgk::MatvecParams *>(params);
    const bgk::DevMatrix &im = *static_cast<const bgk::DevMatrix *>(img);
    Geo g{};
    size_t limit = 0;
    const hipError_t e = device_lds_limit(limit);
    if (e != hipSuccess) return (int)e;
    if (!geometry(epi, p.W.M, p.W.K, p.N, nw, limit, g)) return (int)hipErrorInvalidValue;
    if (epi == bgk::EPI_QKV && (p.W.K != p.D || p.dk < 4 || p.D % p.dk != 0)) return (int)hipErrorInvalidValue;
    if (!p.aq_q || !p.aq_d || !p.aq_s || !im.qs || !im.sc) return (int)hipErrorInvalidValue;
    report_geo(g, report);
    switch (wt) {
        case bgk::W_Q4_0: return (int)launch_t<bgk::W_Q4_0>(epi, p, im, g, st);
        case bgk::W_Q4_1: return (int)launch_t<bgk::W_Q4_1>(epi, p, im, g, st);
        case bgk::W_Q5_0: return (int)launch_t<bgk::W_Q5_0>(epi, p, im, g, st);
        case bgk::W_Q5_1: return (int)launch_t<bgk::W_Q5_1>(epi, p, im, g, st);
        case bgk::W_Q8_0: return (int)launch_t<bgk::W_Q8_0>(epi, p, im, g, st);
        default: return (int)hipErrorInvalidValue;
    }
}
