// Whole-vocabulary sampling (biogpt_hip_generate_sample_wide): the sampler of kernels_sample.hip.h for any top_k up to n_vocab, with a min-p stage between
// the top-p cut and the draw.  sample_wide_rows_kernel runs where sample_rows_kernel runs, one workgroup of WIDE_THREADS threads per logits row, and never
// sorts the row or holds it on chip.  
//
// Everything is decided on the unnormalised weights w_i = exp(l_i * scale - maxl) of the candidates in row order (row_before: value descending, equal
// values lower id first), as integers q_i = round(w_i * 2^62):
//   top k    the k-th non-NaN element of the row, by count
//   cut      the first candidate whose running weight reaches top_p * Z, Z the weight of the k candidates
//   min-p    the candidates with w_i >= min_p (w_0 = 1), as a bound on the value found by bisection
//   draw     the first candidate whose running weight reaches u * W, W the weight of the n candidates left
// Each is a rank query, answered by a radix descent over the order-preserving bits of the f32 value (11 + 11 + 10 bits, one walk of the row and one
// histogram of WIDE_BINS bins in LDS per level), then among the elements of that one value by id (one more walk).  The sums are integers, so the order in which
// the atomics arrive changes nothing: a row, a sampler and a generator state give one id whatever else runs.  A weight errs by 2^-63 of the best
// candidate's, a running sum of k of them by k * 2^-63 <= 4.6e-15 of it (k <= 42 384), and so relative to Z or W, which are at least the best candidate's
// weight; the sums are up to 2^78 and kept as two 64-bit words per bin (the low 32 bits and the rest).
// The generator's block and the step's epilogue are sample_rows_kernel's (sample_mt_refill, sample_append); the order, the walk and the arg-max are the
// row kernels' (kernels_rows.hip.h).
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "kernels_rows.hip.h"
#include "kernels_sample.hip.h"

namespace bgk {

constexpr int WIDE_THREADS = 512;      // 8 waves per row, the four exp() of a quad in flight in each: ~160 registers, which 16 waves would not have
constexpr int WIDE_BINS = 2048;        // bins of a histogram: a digit of 11 bits
constexpr int WIDE_PER = WIDE_BINS / WIDE_THREADS;      // wide_find gives every thread that many, in a row
static_assert(WIDE_BINS == WIDE_PER * WIDE_THREADS, "whole bins per thread");

// a sampler (biogpt_hip_sampler), in device memory: one set of captured steps serves any values
struct SampleWide {
    int32_t top_k, pad;      // 0: the whole vocabulary
    double top_p, min_p, temp;
};

typedef unsigned __int128 wide_u128;

struct WideLds {
    unsigned long long lo[WIDE_BINS], hi[WIDE_BINS];      // a bin's sum is (hi << 32) + lo
    unsigned long long wave_lo[WIDE_THREADS / 64], wave_hi[WIDE_THREADS / 64];
    unsigned long long rem_lo, rem_hi;
    double u;
    uint32_t count;
    int32_t found, bin, id;
};

// ---- the key: ascending in row order (best value first); -0 is 0.  A NaN has no key. ----
__device__ __forceinline__ uint32_t wide_key(float v) {
    const uint32_t u = __float_as_uint(v == 0.0f ? 0.0f : v);
    return ~((u >> 31) ? ~u : (u | 0x80000000u));
}
__device__ __forceinline__ float wide_key_value(uint32_t key) {
    const uint32_t o = ~key;
    return __uint_as_float((o >> 31) ? (o ^ 0x80000000u) : ~o);
}
__device__ __forceinline__ double wide_weight(float v, double scale, double maxl) { return exp((double)v * scale - maxl); }
// round(w * 2^62), w in [0, 1]
__device__ __forceinline__ unsigned long long wide_q(float v, double scale, double maxl) {
    return (unsigned long long)(wide_weight(v, scale, maxl) * 4611686018427387904.0 + 0.5);
}

__device__ __forceinline__ wide_u128 wide_shfl_up(wide_u128 x, int d) {
    const unsigned long long l = __shfl_up((unsigned long long)x, d, 64);
    const unsigned long long h = __shfl_up((unsigned long long)(x >> 64), d, 64);
    return ((wide_u128)h << 64) | l;
}

// ceil(f * total) within [1, total]
__device__ __forceinline__ wide_u128 wide_fraction(double f, wide_u128 total) {
    wide_u128 t = 1;
    if (f > 0.0) {
        const double td = ((double)(unsigned long long)(total >> 64) * 18446744073709551616.0 + (double)(unsigned long long)total) * f;      // < 2^79
        const double th = floor(td * (1.0 / 4294967296.0));
        const double tl = td - th * 4294967296.0;      // exact, in [0, 2^32)
        t = ((wide_u128)(unsigned long long)th << 32) + (unsigned long long)ceil(tl);
    }
    if (t < 1) t = 1;
    return t > total ? total : t;
}

// The histogram is complete and visible (a barrier lies behind the last add).  target(total, count) -- called by every thread with the same values, it may hold
// barriers -- names the rank wanted, 0 for none.  Returns whether a bin reaches it: then bin is the first whose running sum does, and rem what is left of the
// rank inside it (>= 1).  Every thread returns the same.  Ends on a barrier: the histogram may be written again.
template <class Target>
__device__ __forceinline__ bool wide_find(WideLds &L, Target target, int &bin, wide_u128 &rem) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    wide_u128 s = 0;
    for (int j = 0; j < WIDE_PER; j++) s += ((wide_u128)L.hi[WIDE_PER * tid + j] << 32) + L.lo[WIDE_PER * tid + j];
    wide_u128 incl = s;
    for (int d = 1; d < 64; d <<= 1) {
        const wide_u128 o = wide_shfl_up(incl, d);
        if (lane >= d) incl += o;
    }
    if (lane == 63) { L.wave_lo[wv] = (unsigned long long)incl; L.wave_hi[wv] = (unsigned long long)(incl >> 64); }
    if (tid == 0) L.found = 0;
    __syncthreads();
    wide_u128 total = 0;
    for (int w = 0; w < WIDE_THREADS / 64; w++) {
        const wide_u128 x = ((wide_u128)L.wave_hi[w] << 64) | L.wave_lo[w];
        if (w < wv) incl += x;
        total += x;
    }
    const wide_u128 T = target(total, L.count);
    const wide_u128 excl = incl - s;
    if (T >= 1 && excl < T && T <= incl) {      // one thread at most
        wide_u128 left = T - excl;      // in [1, s]
        int j = 0;
        for (; j < WIDE_PER - 1; j++) {
            const wide_u128 b = ((wide_u128)L.hi[WIDE_PER * tid + j] << 32) + L.lo[WIDE_PER * tid + j];
            if (b >= left) break;
            left -= b;
        }
        L.found = 1;
        L.bin = WIDE_PER * tid + j;
        L.rem_lo = (unsigned long long)left; L.rem_hi = (unsigned long long)(left >> 64);
    }
    __syncthreads();
    const bool found = L.found != 0;
    bin = L.bin;
    rem = ((wide_u128)L.rem_hi << 64) | L.rem_lo;
    __syncthreads();
    return found;
}

__device__ __forceinline__ void wide_clear(WideLds &L) {
    const int tid = threadIdx.x;
    for (int b = tid; b < WIDE_BINS; b += WIDE_THREADS) { L.lo[b] = 0; L.hi[b] = 0; }
}

// The rank query: among the row's elements with elig(value, id), in row order, the first at which the running sum -- of the weights q (WEIGHTED) or of ones --
// reaches target(total, count): total the sum over all of them, count their number.  Returns whether there is one, then (out_v, out_i) is the element.
// Called by every thread; every thread returns the same.
template <bool WEIGHTED, class Elig, class Target>
__device__ __forceinline__ bool wide_select(const float *row, int n, double scale, double maxl, WideLds &L, Elig elig, Target target, float &out_v, int &out_i) {
    const int tid = threadIdx.x;
    uint32_t prefix = 0;
    wide_u128 rem = 0;
    // ---- the value: three levels of its key's bits ----
    for (int level = 0, have = 0; level < 3; level++) {
        const int bits = level < 2 ? 11 : 10, shift = 32 - have - bits;
        wide_clear(L);
        if (level == 0 && tid == 0) L.count = 0;
        __syncthreads();
        uint32_t cnt = 0;
        row_scan<WIDE_THREADS>(row, n, [&](float v, int i) {
            if (!elig(v, i)) return;
            const uint32_t key = wide_key(v);
            if (have && (key >> (32 - have)) != prefix) return;
            const uint32_t d = (key >> shift) & ((1u << bits) - 1u);
            if (WEIGHTED) {
                const unsigned long long q = wide_q(v, scale, maxl);
                if (q & 0xffffffffull) atomicAdd(&L.lo[d], q & 0xffffffffull);
                if (q >> 32) atomicAdd(&L.hi[d], q >> 32);
            } else {
                atomicAdd(&L.lo[d], 1ull);
            }
            cnt++;
        });
        if (level == 0) {
            for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
            if ((tid & 63) == 0 && cnt) atomicAdd(&L.count, cnt);
        }
        __syncthreads();
        int bin;
        const bool found = level == 0 ? wide_find(L, target, bin, rem)
                                      : wide_find(L, [&](wide_u128, uint32_t) { return rem; }, bin, rem);
        if (!found) return false;
        prefix = (prefix << bits) | (uint32_t)bin;
        have += bits;
    }
    const uint32_t key = prefix;
    const float val = wide_key_value(key);
    // ---- the id: the m-th of the eligible elements of that value, m = ceil(rem / q) ----
    unsigned long long m = (unsigned long long)rem;
    if (WEIGHTED) {
        const unsigned long long q = wide_q(val, scale, maxl);      // > 0: the bin's sum reached a rank >= 1
        const double rd = (double)(unsigned long long)(rem >> 64) * 18446744073709551616.0 + (double)(unsigned long long)rem;
        m = (unsigned long long)(rd / (double)q);
        if (m < 1) m = 1;
        while ((wide_u128)m * q < rem) m++;
        while (m > 1 && (wide_u128)(m - 1) * q >= rem) m--;
    }
    int s = 0;
    while (((n - 1) >> s) >= WIDE_BINS) s++;
    wide_clear(L);
    __syncthreads();
    row_scan<WIDE_THREADS>(row, n, [&](float v, int i) {
        if (elig(v, i) && wide_key(v) == key) atomicAdd(&L.lo[i >> s], 1ull);
    });
    __syncthreads();
    int bin;
    if (!wide_find(L, [&](wide_u128, uint32_t) { return (wide_u128)m; }, bin, rem)) return false;
    if (tid == 0) {
        unsigned long long left = (unsigned long long)rem;
        int id = ROW_NONE_I;
        const int end = (int)min((long long)n, ((long long)bin + 1) << s);
        for (int i = bin << s; i < end; i++) {
            const float v = row[i];
            if (elig(v, i) && wide_key(v) == key && --left == 0) { id = i; break; }
        }
        L.id = id;
    }
    __syncthreads();
    out_v = val;
    out_i = L.id;
    __syncthreads();
    return out_i != ROW_NONE_I;
}

// The step of sample_rows_kernel with the wide sampler *sp as the selection.  ctl: the call's EOS id and its count of unfinished sequences (its sampler
// is not read).  n_cand_out (or null): per row, the candidates left after all cuts (0: a row without a finite value).
__global__ __launch_bounds__(WIDE_THREADS) void sample_wide_rows_kernel(const float *logits, int ldl, int n_vocab, const SampleWide *sp, SampleCtl *ctl,
                                                                        SampleSeq *sq, SeqState *seq, int32_t *seq_gen, int gen_stride, int32_t *n_cand_out) {
    __shared__ WideLds L;
    __shared__ uint32_t mt_old[MT_N], mt_new[MT_N];
    const int r = blockIdx.x, tid = threadIdx.x;
    SampleSeq *const me = sq + r;
    if (me->finished) return;
    const float *row = logits + (size_t)r * ldl;
    const int K = sp->top_k <= 0 ? n_vocab : min(sp->top_k, n_vocab);
    const double top_p = sp->top_p, min_p = sp->min_p, scale = 1.0 / sp->temp;

    sample_mt_refill<WIDE_THREADS>(me, mt_old, mt_new);

    float mv;
    int mi;
    row_argmax<WIDE_THREADS>(row, n_vocab, mv, mi);
    __syncthreads();
    int id = 0;
    uint32_t n_cand = 0;
    if (mi != ROW_NONE_I && mv > -INFINITY) {      // (else: nothing to draw from -- id 0, the generator untouched)
        const double maxl = (double)mv * scale;
        // the bound: the last candidate; the empty pair: every element but a NaN is one
        float bv = ROW_NONE_V, sv;
        int bi = ROW_NONE_I, si;
        if (K < n_vocab &&
            wide_select<false>(row, n_vocab, scale, maxl, L, [&](float v, int) { return v == v; }, [&](wide_u128, uint32_t) { return (wide_u128)K; }, sv, si)) {
            bv = sv; bi = si;
        }
        if (top_p < 1.0 && wide_select<true>(row, n_vocab, scale, maxl, L, [&](float v, int i) { return v == v && !row_before(bv, bi, v, i); },
                                             [&](wide_u128 total, uint32_t) { return wide_fraction(top_p, total); }, sv, si)) {
            bv = sv; bi = si;
        }
        // min-p: the last key whose weight is >= min_p (weights fall as keys rise; the best element's is 1)
        uint32_t key_mp = 0xffffffffu;
        if (min_p > 0.0) {
            uint32_t lo = wide_key(mv), hi = wide_key(-INFINITY);
            while (hi - lo > 1u) {
                const uint32_t mid = lo + (hi - lo) / 2u;
                if (wide_weight(wide_key_value(mid), scale, maxl) >= min_p) lo = mid; else hi = mid;
            }
            key_mp = lo;
        }
        // the draw: std::discrete_distribution's, fewer than two candidates: the first, and no output is taken
        id = mi;
        if (wide_select<true>(row, n_vocab, scale, maxl, L, [&](float v, int i) { return v == v && !row_before(bv, bi, v, i) && wide_key(v) <= key_mp; },
                              [&](wide_u128 total, uint32_t count) -> wide_u128 {
                                  n_cand = count;
                                  if (count < 2) return 0;
                                  if (tid == 0) {
                                      const double a = (double)mt_next(me->mt);      // generate_canonical<double, 53>: (a + b * 2^32) / 2^64
                                      const double b = (double)mt_next(me->mt);
                                      double u = (a + b * 4294967296.0) / 18446744073709551616.0;
                                      if (u >= 1.0) u = 0x1.fffffffffffffp-1;
                                      L.u = u;
                                  }
                                  __syncthreads();
                                  return wide_fraction(L.u, total);
                              },
                              sv, si))
            id = si;
    }
    if (tid == 0) {
        if (n_cand_out) n_cand_out[r] = (int32_t)n_cand;
        sample_append(r, id, ctl->eos_id, &ctl->n_live, me, seq, seq_gen, gen_stride, [](int) {});
    }
}

}  // namespace bgk
