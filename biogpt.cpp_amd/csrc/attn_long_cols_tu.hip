// Translation unit of the long attention over column states (kernels_attn_long_cols.hip.h): attn_long_seq_kernel<SHARED> and attn_long_runs_kernel, head size 64
// at 1025 .. 2048 keys.  Same arrangement as attn_long_tu.hip: own namespace name for the headers' non-inline kernels, the parameter block crosses as bytes;
// built with -ffp-contract=off (Makefile: the unit's own flag, whatever CXXFLAGS says).
#define bgk bgk_alc
#include <hip/hip_runtime.h>

#include <cstdint>
#include <mutex>
#include <set>

#include "kernels_attn_long_cols.hip.h"

// (attn_long_tu.hip) the device's opt-in LDS limit against the tile kernel's workgroup; the run form's workgroup is as large (attn_long_runs_smem_bytes)
extern "C" int bg_attn_long_tile_fits(int t_cap);

namespace {
std::mutex g_attr_mu;
std::set<int> g_attr_done;      // devices on which the run kernel's > 64 KB dynamic-LDS opt-in attribute is set
}  // namespace

// six words of a launch: form (0 column, 1 run), threads, grid x, grid y (columns / runs), LDS bytes, t_cap; non-zero: a shape the kernels do not hold (no HIP call)
extern "C" int bg_attn_long_cols_geometry(int form, int H, int N, int n_runs, int t_cap, int32_t *six) {
    if ((form != 0 && form != 1) || H < 1 || N < 1 || t_cap < 1 || t_cap > bgk::LONG_ATTN_MAX_KEYS || (form == 1 && (n_runs < 1 || n_runs > N))) return (int)hipErrorInvalidValue;
    if (six) {
        six[0] = form; six[1] = bgk::LONG_ATTN_THREADS; six[2] = H; six[3] = form ? n_runs : N;
        six[4] = form ? (int32_t)bgk::attn_long_runs_smem_bytes(t_cap) : bgk::LONG_COL_LDS_BYTES; six[5] = t_cap;
    }
    return 0;
}

// 1: the current device's opt-in LDS holds the run form's workgroup at t_cap keys; 0: it does not; < 0: minus the HIP error of asking
extern "C" int bg_attn_long_runs_fits(int t_cap) { return bg_attn_long_tile_fits(t_cap); }

// params: a bgk::AttnParams over column states (seq), head size 64, t_cap <= min(P, 2048).  form 0: attn_long_seq_kernel<shared != 0>, one workgroup per column;
// form 1: attn_long_runs_kernel over the n_runs {c0, n} pairs at `runs` (device memory; packed columns only).  report: null, or the six words of the geometry
extern "C" int bg_attn_long_cols_launch(int form, const void *params, size_t params_bytes, int shared, const int32_t *runs, int n_runs, int H, int N, hipStream_t st,
                                        int32_t *report) {
    if (!params || params_bytes != sizeof(bgk::AttnParams)) return (int)hipErrorInvalidValue;
    const bgk::AttnParams &p = *static_cast<const bgk::AttnParams *>(params);
    if (!p.seq || !p.q || !p.kcache || !p.vcache || !p.out || !p.exp_tab || p.dk != 64 || p.D != H * 64 || p.N != N || p.t_cap > p.P) return (int)hipErrorInvalidValue;
    if (form == 1 && (!runs || p.col_mode != 1)) return (int)hipErrorInvalidValue;
    int32_t six[6];
    if (bg_attn_long_cols_geometry(form, H, N, n_runs, p.t_cap, six)) return (int)hipErrorInvalidValue;
    if (report) for (int i = 0; i < 6; i++) report[i] = six[i];
    const dim3 grid(six[2], six[3]), block(six[1]);
    if (form == 0) {
        if (shared) hipLaunchKernelGGL((bgk::attn_long_seq_kernel<true>), grid, block, 0, st, p);
        else hipLaunchKernelGGL((bgk::attn_long_seq_kernel<false>), grid, block, 0, st, p);
        return (int)hipGetLastError();
    }
    if (bg_attn_long_runs_fits(p.t_cap) != 1) return (int)hipErrorInvalidValue;
    {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess) return (int)hipErrorInvalidDevice;
        std::lock_guard<std::mutex> lk(g_attr_mu);
        if (!g_attr_done.count(dev)) {      // once, for every key count, on a device that holds the largest workgroup; otherwise per launch, for this one
            const bool all = bg_attn_long_runs_fits(bgk::LONG_ATTN_MAX_KEYS) == 1;
            const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(bgk::attn_long_runs_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                     (int)bgk::attn_long_runs_smem_bytes(all ? bgk::LONG_ATTN_MAX_KEYS : p.t_cap));
            if (e != hipSuccess) return (int)e;
            if (all) g_attr_done.insert(dev);
        }
    }
    const bgk::AttnLongRunsParams rp{p, runs};
    hipLaunchKernelGGL(bgk::attn_long_runs_kernel, grid, block, (size_t)six[4], st, rp);
    return (int)hipGetLastError();
}
