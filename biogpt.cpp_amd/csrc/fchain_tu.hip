// Translation unit of the float chain (kernels_fchain.hip.h): the many-column linear stage for F32 / F16 files -- 2 weight types x {q/k/v, residual, GELU,
// logits} x 3 tile shapes = 24 kernels -- and the LayerNorm producer in front of it.  Same arrangement as mfma_wide_tu.hip: own namespace name for the
// headers' non-inline kernels, the parameter block crosses as bytes.
#define bgk bgk_fc
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "kernels_fchain.hip.h"

namespace {

template <int WT, int EPI, typename C>
hipError_t launch_one(const bgk::MatvecParams &p, hipStream_t st, int32_t *report) {
    const dim3 grid((p.W.M + C::TM - 1) / C::TM, (p.N + C::TN - 1) / C::TN);
    hipLaunchKernelGGL((bgk::fchain_kernel<WT, EPI, C>), grid, dim3(256), 0, st, p);
    if (report) { report[0] = 256; report[1] = (int32_t)grid.x; report[2] = (int32_t)grid.y; report[3] = C::LDS_BYTES; }
    return hipGetLastError();
}

template <int WT, int EPI>
hipError_t launch_c(int cfg, const bgk::MatvecParams &p, hipStream_t st, int32_t *report) {
    switch (cfg) {
        case 0: return launch_one<WT, EPI, bgk::FchainCfg0>(p, st, report);
        case 1: return launch_one<WT, EPI, bgk::FchainCfg1>(p, st, report);
        case 2: return launch_one<WT, EPI, bgk::FchainCfg2>(p, st, report);
        default: return hipErrorInvalidValue;
    }
}

template <int WT>
hipError_t launch_t(int epi, int cfg, const bgk::MatvecParams &p, hipStream_t st, int32_t *report) {
    switch (epi) {
        case bgk::EPI_QKV: return launch_c<WT, bgk::EPI_QKV>(cfg, p, st, report);
        case bgk::EPI_RESID: return launch_c<WT, bgk::EPI_RESID>(cfg, p, st, report);
        case bgk::EPI_GELU: return launch_c<WT, bgk::EPI_GELU>(cfg, p, st, report);
        case bgk::EPI_LOGITS: return launch_c<WT, bgk::EPI_LOGITS>(cfg, p, st, report);
        default: return hipErrorInvalidValue;
    }
}

// workgroups a tile shape gives a stage of M rows and N columns
template <typename C>
long grid_of(int M, int N) { return (long)((M + C::TM - 1) / C::TM) * (long)((N + C::TN - 1) / C::TN); }

}  // namespace

// The tile shape a stage of M rows and N columns gets: the largest tile that still gives the 256 compute units two workgroups each, else the next smaller
// one (DESIGN.md 4.7 has the measurement behind the figure).
extern "C" int bg_fchain_cfg(int M, int N) {
    constexpr long ENOUGH = 512;
    if (grid_of<bgk::FchainCfg2>(M, N) >= ENOUGH) return 2;
    if (grid_of<bgk::FchainCfg1>(M, N) >= ENOUGH) return 1;
    return 0;
}

// wt: the kernels' WType value (0 F32, 1 F16); epi: EPI_QKV 0, EPI_RESID 1, EPI_GELU 2, EPI_LOGITS 3; params: a bgk::MatvecParams (W.qs the row-major weights,
// W.K % 32 == 0, N >= 1, x / ldx the f32 columns); cfg: 0 .. 2 a tile shape (FchainCfg0 .. 2), -1 bg_fchain_cfg's choice; report: null, or five words
// (threads, grid x, grid y, LDS bytes, cfg).  q/k/v needs K == D, M == 3 D, heads of a power of two.
extern "C" int bg_fchain_launch(int wt, int epi, const void *params, size_t params_bytes, int cfg, hipStream_t st, int32_t *report) {
    if (!params || params_bytes != sizeof(bgk::MatvecParams)) return (int)hipErrorInvalidValue;
    const bgk::MatvecParams &p = *static_cast<const bgk::MatvecParams *>(params);
    if (p.N < 1 || p.W.M < 1 || p.W.K < bgk::QK || p.W.K % bgk::QK != 0 || !p.W.qs || !p.x || p.ldx < p.W.K || p.ldx % 4 != 0) return (int)hipErrorInvalidValue;
    if (epi == bgk::EPI_QKV && (p.W.K != p.D || p.W.M != 3 * p.D || p.dk < 1 || (1 << p.dk_log2) != p.dk || p.D % p.dk != 0)) return (int)hipErrorInvalidValue;
    if (cfg < 0) cfg = bg_fchain_cfg(p.W.M, p.N);
    if (report) report[4] = cfg;
    switch (wt) {
        case bgk::W_F32: return (int)launch_t<bgk::W_F32>(epi, cfg, p, st, report);
        case bgk::W_F16: return (int)launch_t<bgk::W_F16>(epi, cfg, p, st, report);
        default: return (int)hipErrorInvalidValue;
    }
}

// LayerNorm of N columns of K values into f32 rows out[N][K] (fchain_ln_kernel); wt 1: the rows rounded through fp16
extern "C" int bg_fchain_ln(int wt, const float *x, int ldx, int K, int N, const float *ln_w, const float *ln_b, float eps, float *out, hipStream_t st) {
    if (!x || !ln_w || !ln_b || !out || N < 1 || K < 4 || K % 4 != 0 || ldx < K || ldx % 4 != 0 || (wt != bgk::W_F32 && wt != bgk::W_F16)) return (int)hipErrorInvalidValue;
    const dim3 grid((N + 3) / 4);
    if (wt == bgk::W_F16) hipLaunchKernelGGL((bgk::fchain_ln_kernel<true>), grid, dim3(256), 0, st, x, ldx, K, N, ln_w, ln_b, eps, out);
    else hipLaunchKernelGGL((bgk::fchain_ln_kernel<false>), grid, dim3(256), 0, st, x, ldx, K, N, ln_w, ln_b, eps, out);
    return (int)hipGetLastError();
}
