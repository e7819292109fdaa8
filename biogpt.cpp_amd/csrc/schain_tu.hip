// Translation unit of the SIMD chain (kernels_schain.hip.h): the many-column linear stage of a context in the SIMD association -- 5 block formats x {q/k/v,
// residual, GELU, logits} x 3 tile shapes = 60 kernels -- the Q8 producer in front of it and the attention over column states.  Same arrangement as
// fchain_tu.hip: own namespace name for the headers' non-inline kernels, the parameter blocks cross as bytes.
#define bgk bgk_sc
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "kernels_schain.hip.h"

namespace {

template <int WT, int EPI, typename C>
hipError_t launch_one(const bgk::MatvecParams &p, hipStream_t st, int32_t *report) {
    const dim3 grid((p.W.M + C::TM - 1) / C::TM, (p.N + C::TN - 1) / C::TN);
    hipLaunchKernelGGL((bgk::schain_kernel<WT, EPI, C>), grid, dim3(256), 0, st, p);
    if (report) { report[0] = 256; report[1] = (int32_t)grid.x; report[2] = (int32_t)grid.y; report[3] = C::LDS_BYTES; }
    return hipGetLastError();
}

template <int WT, int EPI>
hipError_t launch_c(int cfg, const bgk::MatvecParams &p, hipStream_t st, int32_t *report) {
    switch (cfg) {
        case 0: return launch_one<WT, EPI, bgk::SchainCfg0>(p, st, report);
        case 1: return launch_one<WT, EPI, bgk::SchainCfg1>(p, st, report);
        case 2: return launch_one<WT, EPI, bgk::SchainCfg2>(p, st, report);
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

// The tile shape a stage of M rows and N columns gets.  Reasoning, not a sweep: a workgroup is four waves, one per SIMD of a compute unit, and
// a thread's 8 CN fma chains hide the fma latency from CN = 1 on, so what a wider tile buys is only fewer unpacks and weight loads per column -- worth having
// once the grid still gives each of the 256 compute units two workgroups (a second wave per SIMD covers the weight loads); below that the next narrower tile
// has four (two) times the workgroups.  A tile never wider than the columns there are.
extern "C" int bg_schain_cfg(int M, int N) {
    constexpr long ENOUGH = 512;
    if (N > bgk::SchainCfg1::TN && grid_of<bgk::SchainCfg2>(M, N) >= ENOUGH) return 2;
    if (N > bgk::SchainCfg0::TN && grid_of<bgk::SchainCfg1>(M, N) >= ENOUGH) return 1;
    return 0;
}

// wt: the kernels' WType value of a block format; epi: EPI_QKV 0, EPI_RESID 1, EPI_GELU 2, EPI_LOGITS 3; params: a bgk::MatvecParams (W the matrix in the
// arena's layout, W.K % 32 == 0, N >= 1, aq_q / aq_d / aq_s the producer's rows); cfg: 0 .. 2 a tile shape (SchainCfg0 .. 2), -1 bg_schain_cfg's choice;
// report: null, or five words (threads, grid x, grid y, LDS bytes, cfg).  q/k/v needs K == D, M == 3 D, heads of a power of two.
extern "C" int bg_schain_launch(int wt, int epi, const void *params, size_t params_bytes, int cfg, hipStream_t st, int32_t *report) {
    if (!params || params_bytes != sizeof(bgk::MatvecParams)) return (int)hipErrorInvalidValue;
    const bgk::MatvecParams &p = *static_cast<const bgk::MatvecParams *>(params);
    if (p.N < 1 || p.W.M < 1 || p.W.K < bgk::QK || p.W.K % bgk::QK != 0 || !p.W.qs || !p.W.sc || !p.aq_q || !p.aq_d || !p.aq_s) return (int)hipErrorInvalidValue;
    if (epi == bgk::EPI_QKV && (p.W.K != p.D || p.W.M != 3 * p.D || p.dk < 1 || (1 << p.dk_log2) != p.dk || p.D % p.dk != 0)) return (int)hipErrorInvalidValue;
    if (cfg < 0) cfg = bg_schain_cfg(p.W.M, p.N);
    if (report) report[4] = cfg;
    switch (wt) {
        case bgk::W_Q4_0: return (int)launch_t<bgk::W_Q4_0>(epi, cfg, p, st, report);
        case bgk::W_Q4_1: return (int)launch_t<bgk::W_Q4_1>(epi, cfg, p, st, report);
        case bgk::W_Q5_0: return p.W.qh ? (int)launch_t<bgk::W_Q5_0>(epi, cfg, p, st, report) : (int)hipErrorInvalidValue;
        case bgk::W_Q5_1: return p.W.qh ? (int)launch_t<bgk::W_Q5_1>(epi, cfg, p, st, report) : (int)hipErrorInvalidValue;
        case bgk::W_Q8_0: return (int)launch_t<bgk::W_Q8_0>(epi, cfg, p, st, report);
        default: return (int)hipErrorInvalidValue;
    }
}

// The Q8 producer: N columns x [N][ldx] of K values (behind the LayerNorm when ln_w / ln_b are given) -> oq [N][K], od / os [N][K / 32]; q81 1: the Q8_1 form
// (Q4_1 / Q5_1 weights).  report: null, or four words (threads, grid x, grid y, LDS bytes)
extern "C" int bg_schain_q8(int q81, const float *x, int ldx, int K, int N, const float *ln_w, const float *ln_b, float eps, int8_t *oq, float *od, uint32_t *os,
                            hipStream_t st, int32_t *report) {
    if (!x || !oq || !od || !os || N < 1 || K < bgk::QK || K % bgk::QK != 0 || ldx < K || ldx % 4 != 0 || (ln_w != nullptr) != (ln_b != nullptr)) return (int)hipErrorInvalidValue;
    const bgk::SchainQ8Params p{x, ldx, K, N, ln_w, ln_b, eps, oq, od, os};
    const dim3 grid(N), block(256);
    if (ln_w) {
        if (q81) hipLaunchKernelGGL((bgk::schain_q8_kernel<true, true>), grid, block, 0, st, p);
        else hipLaunchKernelGGL((bgk::schain_q8_kernel<false, true>), grid, block, 0, st, p);
    } else {
        if (q81) hipLaunchKernelGGL((bgk::schain_q8_kernel<true, false>), grid, block, 0, st, p);
        else hipLaunchKernelGGL((bgk::schain_q8_kernel<false, false>), grid, block, 0, st, p);
    }
    if (report) { report[0] = 256; report[1] = N; report[2] = 1; report[3] = 0; }
    return (int)hipGetLastError();
}

// The attention over column states: params a bgk::AttnParams with seq set (head size 64, every column's keys <= SIMD_ATTN_MAXT); shared 1: the columns' first
// pad[0] rows lie in slot pad[1].  report: null, or four words (threads, grid x, grid y, static LDS bytes)
extern "C" int bg_schain_attn(const void *params, size_t params_bytes, int shared, int H, int N, hipStream_t st, int32_t *report) {
    if (!params || params_bytes != sizeof(bgk::AttnParams)) return (int)hipErrorInvalidValue;
    const bgk::AttnParams &a = *static_cast<const bgk::AttnParams *>(params);
    if (!a.seq || !a.q || !a.kcache || !a.vcache || !a.out || !a.exp_tab || a.dk != 64 || H < 1 || N < 1 || a.D != H * 64) return (int)hipErrorInvalidValue;
    const dim3 grid(H, N), block(256);
    if (shared) hipLaunchKernelGGL((bgk::attn_simd_cols_kernel<true>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((bgk::attn_simd_cols_kernel<false>), grid, block, 0, st, a);
    if (report) { report[0] = 256; report[1] = H; report[2] = N; report[3] = 64 * 4 + bgk::SIMD_ATTN_MAXT * 4 + 32 * 64 * 4 + 16 * 8; }
    return (int)hipGetLastError();
}
