// xq_score.hip -- scoring finished samples against a network, and the epoch counts of policy-surprise weighted training
// (include/xq_hip.h: xq_samples_to_requests, xq_score_samples, xq_surprise_counts).  Nothing here touches an engine: the inputs are
// compact xq_sample records in device memory.
// The gather and the score kernel run one 64-lane wavefront per output row, four rows per 256-thread workgroup, no workgroup
// barrier and no LDS traffic between waves (the idiom of xq_batch.hip).  The gather is HBM-bound (about 640 bytes in, 5.7 KB out
// per row); the score kernel reads 640 + 4 m bytes per row and does a few float64 transcendentals per move.
#include <stddef.h>

#include "xq_engine_state.cuh"     // philox_u64: the engine's own Philox, host- and device-callable

#pragma clang fp contract(off)

static_assert(sizeof(xq_score_opts) == 16 && sizeof(xq_sample_score) == 16 && sizeof(xq_sample_policy_stats) == 8 &&
              sizeof(xq_surprise_opts) == 24, "include/xq_hip.h pins these sizes");
static_assert(XQ_SAMPLE_POLICY_STATS_OFFSET >= XQ_SAMPLE_ROOT_STATS_OFFSET + offsetof(xq_sample_root_stats, zero) &&
              XQ_SAMPLE_POLICY_STATS_OFFSET + sizeof(xq_sample_policy_stats) <= XQ_SAMPLE_ROOT_STATS_OFFSET + sizeof(xq_sample_root_stats) &&
              XQ_SAMPLE_POLICY_STATS_OFFSET % 4 == 0,
              "the policy statistics lie inside the zero bytes of xq_sample_root_stats, 4-byte aligned");
static_assert(XQ_SAMPLE_ROOT_STATS_OFFSET == offsetof(xq_sample, pad) && sizeof(xq_sample) == XQ_SAMPLE_BYTES, "record layout");

namespace {

constexpr int SWPW = 4;            // rows per 256-thread workgroup, one per wave
constexpr int SUM_BLOCK = 256;     // threads per workgroup of the two surprise kernels

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off));
    return v;
}
__device__ __forceinline__ int wave_max_i(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off));
    return v;
}
__device__ __forceinline__ int wave_min_i(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = min(v, __shfl_xor(v, off));
    return v;
}

__device__ __forceinline__ int moves_of(const xq_sample *s) { return s->n_moves < XQ_MAXM ? s->n_moves : XQ_MAXM; }

// k_samples_to_batch's planes with flip = 0, two floats per lane and store (a row is 5400 bytes: 8-byte aligned with its base)
__global__ __launch_bounds__(64 * SWPW) void k_samples_to_requests(const xq_sample *__restrict__ rec, const int32_t *__restrict__ idx,
                                                                    int n, float *__restrict__ planes, uint16_t *__restrict__ moves,
                                                                    int32_t *__restrict__ counts) {
    const int o = blockIdx.x * SWPW + (int)(threadIdx.x >> 6);
    if (o >= n) return;
    const int lane = lane_id();
    const xq_sample *s = rec + (idx ? idx[o] : o);
    const int side = s->side;
    float2 *st = (float2 *)(planes + (size_t)o * XQ_STATE_FLOATS);
    for (int e2 = lane; e2 < XQ_STATE_FLOATS / 2; e2 += 64) {
        float v[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int e = 2 * e2 + h;
            const int plane = e / 90, sq = e - plane * 90;
            if (plane == 14) {
                v[h] = side == 1 ? 1.0f : 0.0f;
            } else {
                const int p = s->board[sq];
                const int want = (plane < 7 ? plane + 1 : plane - 6) * (plane < 7 ? side : -side);
                v[h] = p == want ? 1.0f : 0.0f;
            }
        }
        st[e2] = make_float2(v[0], v[1]);
    }
    const int m = moves_of(s);
    const int i0 = 2 * lane, i1 = 2 * lane + 1;                      // one 4-byte store per lane: the whole 256-byte row
    const uint32_t a0 = i0 < m ? s->actions[i0] : 0u, a1 = i1 < m ? s->actions[i1] : 0u;
    ((uint32_t *)(moves + (size_t)o * XQ_MAXM))[lane] = a0 | (a1 << 16);
    if (lane == 0) counts[o] = m;
}

// lane L owns moves L and L + 64
__global__ __launch_bounds__(64 * SWPW) void k_score_samples(xq_sample *rec, const int32_t *__restrict__ idx, int n,
                                                              const float *__restrict__ logits, const float *__restrict__ value,
                                                              double late_temperature, int write_back, xq_sample_score *scores) {
    __shared__ double s_w[SWPW][XQ_MAXM];
    const int o = blockIdx.x * SWPW + (int)(threadIdx.x >> 6);
    if (o >= n) return;
    const int lane = lane_id();
    xq_sample *s = rec + (idx ? idx[o] : o);
    const int m = moves_of(s);
    const bool lt = s->late_temp != 0;
    const double inv_t = lt ? 1.0 / late_temperature : 1.0;
    const float *lg = logits + (size_t)o * XQ_MAXM;
    double w[2], l[2];
    int cv[2];
    bool bad = false;
    double lmax = -DBL_MAX;
    int vmax = -1;
    double *sw = s_w[threadIdx.x >> 6];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int i = lane + 64 * h;
        w[h] = 0.0; l[h] = 0.0; cv[h] = -1;
        if (i < m) {
            const double c = (double)s->visits[i];
            w[h] = lt ? (c > 0.0 ? pow(c, inv_t) : 0.0) : c;
            cv[h] = s->visits[i];
            const float lf = lg[i];
            bad = bad || !isfinite(lf);
            l[h] = (double)lf;
            lmax = fmax(lmax, l[h]);
            vmax = max(vmax, cv[h]);
            sw[i] = w[h];
        }
    }
    wave_sync();
    // total: one sequential sum in move order, as k_samples_to_batch forms it (every lane the same value); the terms come from
    // the wave's own LDS row, so a lane computes two powers, not m
    double total = 0.0;
    for (int i = 0; i < m; ++i) total += sw[i];
    const bool any_bad = __ballot(bad) != 0ull;
    const bool invalid = m == 0 || !(total > 0.0) || !isfinite(total) || any_bad;  // wave-uniform; a small T can overflow the powers
    xq_sample_score sc;
    sc.policy_kl = 0.0f; sc.policy_ce = 0.0f; sc.value = 0.0f; sc.top1 = 0; sc.valid = 0; sc.zero[0] = 0; sc.zero[1] = 0;
    if (!invalid) {
        lmax = wave_max(lmax);
        vmax = wave_max_i(vmax);
        double se = 0.0;
        int first_l = XQ_MAXM, first_v = XQ_MAXM;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int i = lane + 64 * h;
            if (i < m) {
                se += exp(l[h] - lmax);
                if (l[h] == lmax) first_l = min(first_l, i);
                if (cv[h] == vmax) first_v = min(first_v, i);
            }
        }
        const double logz = log(wave_sum(se));
        double ce = 0.0, kl = 0.0;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int i = lane + 64 * h;
            if (i < m && w[h] > 0.0) {
                const double t = w[h] / total;
                if (t > 0.0) {
                    const double logp = l[h] - lmax - logz;
                    ce -= t * logp;
                    kl += t * (log(t) - logp);
                }
            }
        }
        ce = wave_sum(ce);
        kl = fmax(0.0, wave_sum(kl));
        first_l = wave_min_i(first_l);
        first_v = wave_min_i(first_v);
        sc.policy_kl = (float)kl; sc.policy_ce = (float)ce; sc.value = value[o];
        sc.top1 = first_l == first_v ? 1 : 0; sc.valid = 1;
    }
    if (lane == 0) {
        if (scores) scores[o] = sc;
        if (write_back && !invalid) {
            uint32_t *dst = (uint32_t *)((uint8_t *)s + XQ_SAMPLE_POLICY_STATS_OFFSET);
            dst[0] = __float_as_uint(sc.policy_kl);
            dst[1] = 1u | ((uint32_t)sc.top1 << 8);
        }
    }
}

__host__ __device__ __forceinline__ const xq_sample_policy_stats *policy_stats_of(const xq_sample *s) {
    return (const xq_sample_policy_stats *)((const uint8_t *)s + XQ_SAMPLE_POLICY_STATS_OFFSET);
}

// q_i of the header: the KL capped at 64 nats, in units of 2^-20 nat (the product is exact in float32: a power of two)
__host__ __device__ __forceinline__ uint64_t surprise_q(float kl) {
    const float x = kl >= 0.0f ? (kl < 64.0f ? kl : 64.0f) : 0.0f;               // NaN and negatives: 0
    return (uint64_t)llrint((double)(x * 1048576.0f));
}

// c_i of the header: ONE copy for the kernel and xq_surprise_count_host
__host__ __device__ inline int32_t surprise_count(float kl, bool marked, uint64_t M, uint64_t S, double alpha, uint64_t seed,
                                                  uint32_t epoch, uint32_t slot, uint32_t game_seq, uint32_t ply) {
    if (!marked || S == 0) return 1;
    const double ratio = ((double)surprise_q(kl) * (double)M) / (double)S;
    const double a = 1.0 - alpha, b = alpha * ratio;
    const double w = a + b;
    const double fl = floor(w);
    const double u = (double)(philox_u64(seed, epoch, slot, (uint32_t)XQ_RNG_KIND_SURPRISE, game_seq, ply) >> 11) * 0x1p-53;
    return (int32_t)fl + (u < w - fl ? 1 : 0);
}

// S and M: integer sums, so any order gives the same.  Grid-stride, wave reduction, one pair of atomics per workgroup.
__global__ __launch_bounds__(SUM_BLOCK) void k_surprise_sum(const xq_sample *__restrict__ rec, int n, unsigned long long *__restrict__ sm) {
    __shared__ unsigned long long part[2][SUM_BLOCK / 64];
    unsigned long long q = 0, cnt = 0;
    for (long long i = (long long)blockIdx.x * SUM_BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * SUM_BLOCK) {
        const xq_sample_policy_stats *ps = policy_stats_of(rec + i);
        if (ps->has_policy_stats == 1) { q += surprise_q(ps->policy_kl); ++cnt; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { q += __shfl_xor(q, off); cnt += __shfl_xor(cnt, off); }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { part[0][wave] = q; part[1][wave] = cnt; }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long tq = 0, tc = 0;
#pragma unroll
        for (int k = 0; k < SUM_BLOCK / 64; ++k) { tq += part[0][k]; tc += part[1][k]; }
        if (tc) { atomicAdd(sm, tq); atomicAdd(sm + 1, tc); }
    }
}

__global__ __launch_bounds__(SUM_BLOCK) void k_surprise_counts(const xq_sample *__restrict__ rec, int n, double alpha, uint64_t seed,
                                                               uint32_t epoch, const unsigned long long *__restrict__ sm,
                                                               int32_t *__restrict__ counts) {
    const unsigned long long S = sm[0], M = sm[1];
    for (long long i = (long long)blockIdx.x * SUM_BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * SUM_BLOCK) {
        const xq_sample *s = rec + i;
        const xq_sample_policy_stats *ps = policy_stats_of(s);
        counts[i] = surprise_count(ps->policy_kl, ps->has_policy_stats == 1, M, S, alpha, seed, epoch, s->slot, s->game_seq, s->ply);
    }
}

}  // namespace

extern "C" {

int xq_samples_to_requests(const void *dev_samples, const int32_t *dev_index, int n, float *dev_planes, uint16_t *dev_moves,
                           int32_t *dev_counts, void *stream) {
    if (n < 0 || (n > 0 && (!dev_samples || !dev_planes || !dev_moves || !dev_counts))) return XQ_ERR_ARG;
    if (((uintptr_t)dev_planes & 7) || ((uintptr_t)dev_moves & 3)) return XQ_ERR_ARG;
    if (n == 0) return XQ_OK;
    hipLaunchKernelGGL(k_samples_to_requests, dim3((n + SWPW - 1) / SWPW), dim3(64 * SWPW), 0, (hipStream_t)stream,
                       (const xq_sample *)dev_samples, dev_index, n, dev_planes, dev_moves, dev_counts);
    return launch_status();
}

int xq_score_samples(void *dev_samples, const int32_t *dev_index, int n, const float *dev_legal_logits, const float *dev_value,
                     const xq_score_opts *opts, xq_sample_score *dev_scores, void *stream) {
    if (!opts || opts->reserved != 0 || (opts->write_back != 0 && opts->write_back != 1)) return XQ_ERR_ARG;
    if (!(opts->late_temperature > 0.0) || !isfinite(opts->late_temperature)) return XQ_ERR_ARG;
    if (n < 0 || (n > 0 && (!dev_samples || !dev_legal_logits || !dev_value || (!dev_scores && !opts->write_back)))) return XQ_ERR_ARG;
    if (((uintptr_t)dev_samples | (uintptr_t)dev_scores) & 3) return XQ_ERR_ARG;
    if (n == 0) return XQ_OK;
    hipLaunchKernelGGL(k_score_samples, dim3((n + SWPW - 1) / SWPW), dim3(64 * SWPW), 0, (hipStream_t)stream, (xq_sample *)dev_samples,
                       dev_index, n, dev_legal_logits, dev_value, opts->late_temperature, (int)opts->write_back, dev_scores);
    return launch_status();
}

int xq_surprise_counts(const void *dev_samples, int n_records, const xq_surprise_opts *opts, int32_t *dev_counts, void *dev_scratch,
                       void *stream) {
    if (!opts || !(opts->alpha >= 0.0 && opts->alpha <= 1.0) || opts->reserved != 0) return XQ_ERR_ARG;
    if (n_records < 0 || (n_records > 0 && (!dev_samples || !dev_counts || !dev_scratch))) return XQ_ERR_ARG;
    if (((uintptr_t)dev_scratch & 7) || ((uintptr_t)dev_samples & 3)) return XQ_ERR_ARG;
    if (n_records == 0) return XQ_OK;
    const hipStream_t s = (hipStream_t)stream;
    XQ_TRY(hipMemsetAsync(dev_scratch, 0, XQ_SURPRISE_SCRATCH_BYTES, s));
    int blocks = (n_records + SUM_BLOCK - 1) / SUM_BLOCK;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(k_surprise_sum, dim3(blocks), dim3(SUM_BLOCK), 0, s, (const xq_sample *)dev_samples, n_records,
                       (unsigned long long *)dev_scratch);
    hipLaunchKernelGGL(k_surprise_counts, dim3(blocks), dim3(SUM_BLOCK), 0, s, (const xq_sample *)dev_samples, n_records, opts->alpha,
                       opts->seed, opts->epoch, (const unsigned long long *)dev_scratch, dev_counts);
    return launch_status();
}

int xq_surprise_count_host(float policy_kl, int marked, uint64_t M, uint64_t S, double alpha, uint64_t seed, uint32_t epoch,
                           uint32_t slot, uint32_t game_seq, uint32_t ply) {
    if (!(alpha >= 0.0 && alpha <= 1.0)) return XQ_ERR_ARG;
    return surprise_count(policy_kl, marked != 0, M, S, alpha, seed, epoch, slot, game_seq, ply);
}

}  // extern "C"
