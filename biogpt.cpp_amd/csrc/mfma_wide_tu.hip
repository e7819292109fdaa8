// Translation unit of the wide chain (kernels_mfma_wide.hip.h): the many-column linear stage on the int8 matrix cores for block-quantized files that are
// not BioGPT-base -- 5 block formats x {q/k/v, residual, GELU, logits} = 20 kernels -- and the two Q8 producers in front of it.  Same arrangement as
// mfma_tu.hip: own namespace name for the headers' non-inline kernels, the parameter blocks cross as bytes.
#define bgk bgk_mw
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "kernels_mfma_wide.hip.h"

namespace {

template <int WT, int EPI>
hipError_t launch_one(const bgk::MatvecParams &p, const bgk::DevMatrix &img, hipStream_t st) {
    const dim3 grid(((p.W.M + 15) / 16 + 3) / 4, (p.N + 15) / 16);
    hipLaunchKernelGGL((bgk::matmul_wide_kernel<WT, EPI>), grid, dim3(256), 0, st, p, img);
    return hipGetLastError();
}

template <int WT>
hipError_t launch_t(int epi, const bgk::MatvecParams &p, const bgk::DevMatrix &img, hipStream_t st) {
    switch (epi) {
        case bgk::EPI_QKV: return launch_one<WT, bgk::EPI_QKV>(p, img, st);
        case bgk::EPI_RESID: return launch_one<WT, bgk::EPI_RESID>(p, img, st);
        case bgk::EPI_GELU: return launch_one<WT, bgk::EPI_GELU>(p, img, st);
        case bgk::EPI_LOGITS: return launch_one<WT, bgk::EPI_LOGITS>(p, img, st);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace

// wt: the kernels' WType value (2, 3, 6, 7, 8); epi: EPI_QKV 0, EPI_RESID 1, EPI_GELU 2, EPI_LOGITS 3; params: a bgk::MatvecParams (W.K % 32 == 0, N >= 1, aq_* the
// columns' Q8 blocks); img: a bgk::DevMatrix, the row-tiled image with ceil(M / 16) tiles (the last one zero-padded).  The layer sites need 16 | M; q/k/v also K == D, 64 | D.
extern "C" int bg_wide_launch(int wt, int epi, const void *params, size_t params_bytes, const void *img, size_t img_bytes, hipStream_t st) {
    if (!params || !img || params_bytes != sizeof(bgk::MatvecParams) || img_bytes != sizeof(bgk::DevMatrix)) return (int)hipErrorInvalidValue;
    const bgk::MatvecParams &p = *static_cast<const bgk::MatvecParams *>(params);
    const bgk::DevMatrix &im = *static_cast<const bgk::DevMatrix *>(img);
    if (p.N < 1 || p.W.M < 1 || p.W.K < bgk::QK || p.W.K % bgk::QK != 0) return (int)hipErrorInvalidValue;
    if (epi != bgk::EPI_LOGITS && p.W.M % 16 != 0) return (int)hipErrorInvalidValue;
    if (epi == bgk::EPI_QKV && (p.W.K != p.D || p.W.M != 3 * p.D || p.dk < 4 || p.D % p.dk != 0)) return (int)hipErrorInvalidValue;
    switch (wt) {
        case bgk::W_Q4_0: return (int)launch_t<bgk::W_Q4_0>(epi, p, im, st);
        case bgk::W_Q4_1: return (int)launch_t<bgk::W_Q4_1>(epi, p, im, st);
        case bgk::W_Q5_0: return (int)launch_t<bgk::W_Q5_0>(epi, p, im, st);
        case bgk::W_Q5_1: return (int)launch_t<bgk::W_Q5_1>(epi, p, im, st);
        case bgk::W_Q8_0: return (int)launch_t<bgk::W_Q8_0>(epi, p, im, st);
        default: return (int)hipErrorInvalidValue;
    }
}

// LayerNorm + Q8_0 / Q8_1 blocks of N columns of K values (lnq_wide_kernel); ln_w == null: plain Q8 of the rows (q8_rows_kernel)
extern "C" int bg_wide_quantize(const float *x, int ldx, int K, int N, const float *ln_w, const float *ln_b, float eps, int q81, int8_t *oq_q, float *oq_d,
                                uint32_t *oq_s, hipStream_t st) {
    if (!x || !oq_q || !oq_d || !oq_s || N < 1 || K < bgk::QK || K % bgk::QK != 0 || (ln_w != nullptr && ln_b == nullptr)) return (int)hipErrorInvalidValue;
    if (ln_w) {
        const dim3 grid((N + 3) / 4);
        if (q81) hipLaunchKernelGGL((bgk::lnq_wide_kernel<true>), grid, dim3(256), 0, st, x, ldx, K, N, ln_w, ln_b, eps, oq_q, oq_d, oq_s);
        else hipLaunchKernelGGL((bgk::lnq_wide_kernel<false>), grid, dim3(256), 0, st, x, ldx, K, N, ln_w, ln_b, eps, oq_q, oq_d, oq_s);
    } else {
        const dim3 grid((K / 4 + 255) / 256, N);
        if (q81) hipLaunchKernelGGL((bgk::q8_rows_kernel<true>), grid, dim3(256), 0, st, x, ldx, K, oq_q, oq_d, oq_s);
        else hipLaunchKernelGGL((bgk::q8_rows_kernel<false>), grid, dim3(256), 0, st, x, ldx, K, oq_q, oq_d, oq_s);
    }
    return hipGetLastError();
}
