// Translation unit of the wide decode layer (kernels_wdecode.hip.h): one token of a block-quantized file that is not BioGPT-base -- 5 block formats x {q/k/v,
// out_proj, fc1, fc2} = 20 kernels, and the three instantiations of dec_attn_kernel (kernels_decode.hip.h) its attention launch takes up to 256 keys.  Same
// arrangement as mfma_wide_tu.hip: own namespace name for the headers' non-inline kernels, the parameter blocks cross as bytes.
#define bgk bgk_wd
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "kernels_wdecode.hip.h"

namespace {

enum : int { WS_QKV = 0, WS_ATTN = 1, WS_OPROJ = 2, WS_FC1 = 3, WS_FC2 = 4 };
struct Geo { int threads, grid, lds, max_rows; };

// The launch shape of a linear stage at (M, K): see the header for the split.  false: a shape the kernels do not hold.
bool geometry(int stage, int M, int K, Geo &g) {
    if (M < 1 || K < bgk::QK || K % bgk::QK != 0) return false;
    const int bpr = K / bgk::QK;
    const bool ln = stage == WS_QKV || stage == WS_FC1;
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
    if (ln) {
        const int need = ((((K >> 2) + bgk::WDEC_MAXCH - 1) / bgk::WDEC_MAXCH) + 63) & ~63;      // the column in WDEC_MAXCH chunks per thread
        if (need > 1024) return false;
        g.threads = std::max(g.threads, need);
    }
    if (g.max_rows > 64 * (g.threads >> 6)) return false;      // a finisher thread per row
    const size_t lds = bgk::wdec_smem_bytes(ln, K, g.max_rows);
    if (lds > 64 * 1024) return false;
    g.lds = (int)lds;
    return true;
}

template <int WT>
hipError_t launch_t(int stage, const bgk::WdecParams &p, const Geo &g, hipStream_t st) {
    const dim3 grid(g.grid), block(g.threads);
    switch (stage) {
        case WS_QKV: hipLaunchKernelGGL((bgk::wdec_qkv_kernel<WT>), grid, block, g.lds, st, p); break;
        case WS_OPROJ: hipLaunchKernelGGL((bgk::wdec_oproj_kernel<WT>), grid, block, g.lds, st, p); break;
        case WS_FC1: hipLaunchKernelGGL((bgk::wdec_fc1_kernel<WT>), grid, block, g.lds, st, p); break;
        case WS_FC2: hipLaunchKernelGGL((bgk::wdec_fc2_kernel<WT>), grid, block, g.lds, st, p); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace

// four words of a linear stage's launch at (M, K): threads, grid, LDS bytes, most rows of a workgroup; non-zero: the kernels do not hold the shape
extern "C" int bg_wdec_geometry(int stage, int M, int K, int32_t *four) {
    Geo g{};
    if (stage == WS_ATTN || stage < WS_QKV || stage > WS_FC2 || !geometry(stage, M, K, g)) return (int)hipErrorInvalidValue;
    if (four) { four[0] = g.threads; four[1] = g.grid; four[2] = g.lds; four[3] = g.max_rows; }
    return 0;
}

// wt: the kernels' WType value (2, 3, 6, 7, 8); stage: 0 q/k/v, 2 out_proj, 3 fc1, 4 fc2; params: a bgk::WdecParams with W and the stage's pointers (bpr
// and pstride are set here); q/k/v needs W.M == 3 D, W.K == D, 64 | D.  report: null, or the four words of bg_wdec_geometry
extern "C" int bg_wdec_launch(int wt, int stage, const void *params, size_t params_bytes, hipStream_t st, int32_t *report) {
    if (!params || params_bytes != sizeof(bgk::WdecParams)) return (int)hipErrorInvalidValue;
    bgk::WdecParams p = *static_cast<const bgk::WdecParams *>(params);
    Geo g{};
    if (stage == WS_ATTN || !geometry(stage, p.W.M, p.W.K, g)) return (int)hipErrorInvalidValue;
    if (stage == WS_QKV && (p.W.K != p.D || p.W.M != 3 * p.D || p.D % 64 != 0)) return (int)hipErrorInvalidValue;
    p.bpr = p.W.K / bgk::QK; p.pstride = bgk::wdec_pstride(p.bpr);
    if (report) { report[0] = g.threads; report[1] = g.grid; report[2] = g.lds; report[3] = g.max_rows; }
    switch (wt) {
        case bgk::W_Q4_0: return (int)launch_t<bgk::W_Q4_0>(stage, p, g, st);
        case bgk::W_Q4_1: return (int)launch_t<bgk::W_Q4_1>(stage, p, g, st);
        case bgk::W_Q5_0: return (int)launch_t<bgk::W_Q5_0>(stage, p, g, st);
        case bgk::W_Q5_1: return (int)launch_t<bgk::W_Q5_1>(stage, p, g, st);
        case bgk::W_Q8_0: return (int)launch_t<bgk::W_Q8_0>(stage, p, g, st);
        default: return (int)hipErrorInvalidValue;
    }
}

// The load bounds up to which the attention launch below runs at 16 / 8 / 4 lanes per key; the last is the most keys it holds.  The one place they are written.
static const int ATTN_BORDERS[3] = {64, 128, 256};
extern "C" int bg_wdec_attn_max_keys(void) { return ATTN_BORDERS[2]; }
// returns how many borders there are; out (or null) takes the first cap
extern "C" int bg_wdec_attn_borders(int32_t *out, int cap) {
    for (int i = 0; i < 3 && i < cap && out; i++) out[i] = ATTN_BORDERS[i];
    return 3;
}
// The attention of H heads of 64 over up to 256 keys: dec_attn_kernel at 16 / 8 / 4 lanes per key for a load bound t_cap of up to 64 / 128 / 256.
// params: a bgk::DecAttnParams (att_out: the f32 row; oq_*: its Q8 blocks).  report: null, or threads, grid, lanes per key, 0
extern "C" int bg_wdec_attn(const void *params, size_t params_bytes, int H, hipStream_t st, int32_t *report) {
    if (!params || params_bytes != sizeof(bgk::DecAttnParams) || H < 1) return (int)hipErrorInvalidValue;
    const bgk::DecAttnParams &a = *static_cast<const bgk::DecAttnParams *>(params);
    if (a.t_cap < 1 || a.t_cap > ATTN_BORDERS[2] || a.t_cap > a.P) return (int)hipErrorInvalidValue;
    const int lpk = a.t_cap <= ATTN_BORDERS[0] ? 16 : (a.t_cap <= ATTN_BORDERS[1] ? 8 : 4);
    if (report) { report[0] = 1024; report[1] = H; report[2] = lpk; report[3] = 0; }
    if (lpk == 16) hipLaunchKernelGGL((bgk::dec_attn_kernel<16, 16>), dim3(H), dim3(1024), 0, st, a);
    else if (lpk == 8) hipLaunchKernelGGL((bgk::dec_attn_kernel<8, 16>), dim3(H), dim3(1024), 0, st, a);
    else hipLaunchKernelGGL((bgk::dec_attn_kernel<4, 16>), dim3(H), dim3(1024), 0, st, a);
    return hipGetLastError();
}
