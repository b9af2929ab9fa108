// xq_merge.hip -- merging the records of one position into one training sample (include/xq_hip.h: xq_position_keys,
// xq_position_key_host, xq_position_group_heads, xq_groups_to_batch).  Nothing here touches an engine or rewrites a record: the
// inputs are compact xq_sample records in device memory, and the merged form lives in index arrays that the caller builds
// (a stable sort by key between the first two kernels is the caller's).
// The key and the head kernel run one 64-lane wavefront per row, four rows per 256-thread workgroup, no barrier (the idiom of
// xq_score.hip): a row is 90 board bytes in, 9 bytes out.  The batch kernel runs one 256-thread workgroup per output row: a row
// of a group of one takes k_samples_to_batch's path (zero fill, scatter); a larger group adds its members' targets one after the
// other into a float64 accumulator of 8100 entries in LDS (64 800 bytes: two workgroups per CU) and writes the row from there.
#include <stddef.h>

#include "xq_common.h"

#pragma clang fp contract(off)

using namespace xq;

static_assert(sizeof(xq_sample) == XQ_SAMPLE_BYTES && sizeof(xq_batch_opts) == 16, "include/xq_hip.h pins these sizes");
static_assert(XQ_ACTION_SPACE % 4 == 0 && XQ_MAXM == 128 && XQ_SQUARES == 90, "the lane maps below assume these");

namespace {

constexpr int KWPW = 4;            // rows per 256-thread workgroup of the key and the head kernel, one per wave
constexpr int GB_THREADS = 256;    // threads per workgroup (= per output row) of the batch kernel

__host__ __device__ __forceinline__ int mir_sq(int sq) { return (sq / 9) * 9 + 8 - sq % 9; }

__host__ __device__ __forceinline__ uint64_t key_mix(uint64_t x) {
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27; x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}
// term(i, b) of the header: i = the square (90: the side to move), b = the byte there
__host__ __device__ __forceinline__ uint64_t key_term(int i, int8_t b) {
    return key_mix(0x9E3779B97F4A7C15ull * (uint64_t)(i * 256 + (int)(uint8_t)b + 1));
}
// the canonical orientation, given the smallest square at which the board differs from its mirror image (-1: none)
__host__ __device__ __forceinline__ int mirrored_of(const int8_t *board, int first_diff) {
    return first_diff >= 0 && board[mir_sq(first_diff)] < board[first_diff] ? 1 : 0;
}

__device__ __forceinline__ int lane_id() { return (int)(threadIdx.x & 63u); }
// LDS operations of one wave execute in issue order; this keeps the compiler from moving them (csrc/xq_rules.cuh)
__device__ __forceinline__ void wave_sync() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

__global__ __launch_bounds__(64 * KWPW) void k_position_keys(const xq_sample *__restrict__ rec, const int32_t *__restrict__ idx,
                                                              int n, int flags, uint64_t *__restrict__ keys,
                                                              uint8_t *__restrict__ mirrored) {
    const int o = blockIdx.x * KWPW + (int)(threadIdx.x >> 6);
    if (o >= n) return;
    const int lane = lane_id();
    const xq_sample *s = rec + (idx ? idx[o] : o);
    // lane L owns squares L and L + 64 (the latter for L < 26)
    const int sq0 = lane, sq1 = lane + 64 < XQ_SQUARES ? lane + 64 : XQ_SQUARES - 1;
    const bool has1 = lane + 64 < XQ_SQUARES;
    const int8_t b0 = s->board[sq0], m0 = s->board[mir_sq(sq0)];
    const int8_t b1 = s->board[sq1], m1 = s->board[mir_sq(sq1)];
    int mir = 0;
    if (flags & XQ_POSITION_KEY_MIRROR) {
        const unsigned long long d0 = __ballot(b0 != m0), d1 = __ballot(has1 && b1 != m1);
        const int first = d0 ? __ffsll((long long)d0) - 1 : (d1 ? 64 + __ffsll((long long)d1) - 1 : -1);   // wave-uniform
        mir = mirrored_of(s->board, first);
    }
    uint64_t k = key_term(sq0, mir ? m0 : b0);
    if (has1) k ^= key_term(sq1, mir ? m1 : b1);
    if (lane == 0) k ^= key_term(XQ_SQUARES, s->side);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) k ^= (uint64_t)__shfl_xor((unsigned long long)k, off);
    if (lane == 0) { keys[o] = k; mirrored[o] = (uint8_t)mir; }
}

// one byte of a row's canonical board
__device__ __forceinline__ int8_t canon_at(const xq_sample *s, bool mir, int sq) { return s->board[mir ? mir_sq(sq) : sq]; }

// head[j] of the header: row order[j] against its predecessor in the sorted order
__global__ __launch_bounds__(64 * KWPW) void k_position_group_heads(const xq_sample *__restrict__ rec, const int32_t *__restrict__ idx,
                                                                     const int32_t *__restrict__ order,
                                                                     const uint64_t *__restrict__ keys,
                                                                     const uint8_t *__restrict__ mirrored, int n,
                                                                     uint8_t *__restrict__ head) {
    const int j = blockIdx.x * KWPW + (int)(threadIdx.x >> 6);
    if (j >= n) return;
    const int lane = lane_id();
    const int r = order[j], p = j > 0 ? order[j - 1] : -1;
    bool h = true;                                                           // wave-uniform
    if (j > 0 && r >= 0 && r < n && p >= 0 && p < n) {                       // a row outside [0, n) is read nowhere: a head
        const xq_sample *a = rec + (idx ? idx[r] : r), *b = rec + (idx ? idx[p] : p);
        h = keys[r] != keys[p] || a->side != b->side;
        if (!h) {
            const bool ma = mirrored[r] != 0, mb = mirrored[p] != 0;
            const int sq1 = lane + 64 < XQ_SQUARES ? lane + 64 : lane;
            const bool d = canon_at(a, ma, lane) != canon_at(b, mb, lane) || canon_at(a, ma, sq1) != canon_at(b, mb, sq1);
            h = __ballot(d) != 0ull;
        }
    }
    if (lane == 0) head[j] = h ? 1 : 0;
}

// k_samples_to_batch's plane entry e of record s under flip fl
__device__ __forceinline__ float plane_entry(const xq_sample *s, int side, bool fl, int e) {
    const int plane = e / 90, sq = e - plane * 90;
    if (plane == 14) return side == 1 ? 1.0f : 0.0f;
    const int p = s->board[fl ? mir_sq(sq) : sq];
    const int want = (plane < 7 ? plane + 1 : plane - 6) * (plane < 7 ? side : -side);
    return p == want ? 1.0f : 0.0f;
}

__device__ __forceinline__ int mirror_action(int a) {
    const int from = a / 90, to = a - from * 90;
    return mir_sq(from) * 90 + mir_sq(to);
}

// One wave: lane L gets the weights of moves L and L + 64 of record s (k_samples_to_batch's w_i, 0 behind m) and every lane the
// record's total, the sequential float64 sum in move order.  Each power is computed once; the sum walks the lanes by shuffle.
__device__ __forceinline__ double member_weights(const xq_sample *s, int m, double late_temperature, int lane, double w[2]) {
    const bool lt = s->late_temp != 0;
    const double inv_t = lt ? 1.0 / late_temperature : 1.0;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int i = lane + 64 * h;
        w[h] = 0.0;
        if (i < m) {
            const double c = (double)s->visits[i];
            w[h] = lt ? (c > 0.0 ? pow(c, inv_t) : 0.0) : c;
        }
    }
    double total = 0.0;
    const int m0 = m < 64 ? m : 64;
    for (int i = 0; i < m0; ++i) total += __shfl(w[0], i);
    for (int i = 64; i < m; ++i) total += __shfl(w[1], i - 64);
    return total;
}

// zt of the header: the float64 value xq_samples_to_batch_ex forms before its cast
__device__ __forceinline__ double member_z(const xq_sample *s, double q_mix) {
    const xq_sample_root_stats *rs = (const xq_sample_root_stats *)((const uint8_t *)s + XQ_SAMPLE_ROOT_STATS_OFFSET);
    if (q_mix != 0.0 && rs->has_root_stats == 1) {
        const double a = (1.0 - q_mix) * (double)s->z, b = q_mix * (double)rs->root_q;
        return a + b;
    }
    return (double)s->z;
}

__global__ __launch_bounds__(GB_THREADS) void k_groups_to_batch(const xq_sample *__restrict__ rec, const int32_t *__restrict__ offsets,
                                                                const int32_t *__restrict__ members,
                                                                const uint8_t *__restrict__ member_mirrored, int n_groups,
                                                                const int32_t *__restrict__ group, const uint8_t *__restrict__ flip,
                                                                int n, double late_temperature, double q_mix,
                                                                float *__restrict__ states, float *__restrict__ pi,
                                                                float *__restrict__ z) {
    __shared__ double acc[XQ_ACTION_SPACE];          // the dense float64 sums of a group of two or more members
    __shared__ int s_n_pi;                           // the number of valid members, from wave 0 to the row's writers
    const int o = blockIdx.x;
    if (o >= n) return;
    const int tid = threadIdx.x, lane = lane_id();
    const int g = group[o];
    int off = 0, nm = 0;                             // workgroup-uniform from here on
    if (g >= 0 && g < n_groups) { off = offsets[g]; nm = offsets[g + 1] - off; }
    float *st = states + (size_t)o * XQ_STATE_FLOATS;
    float4 *p4 = (float4 *)(pi + (size_t)o * XQ_ACTION_SPACE);
    if (nm <= 0) {                                   // no such group, or an empty one: zeros, and no record is read
        for (int e = tid; e < XQ_STATE_FLOATS; e += GB_THREADS) st[e] = 0.0f;
        for (int i = tid; i < XQ_ACTION_SPACE / 4; i += GB_THREADS) p4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (tid == 0) z[o] = 0.0f;
        return;
    }
    const bool f = flip[o] != 0;
    const xq_sample *s0 = rec + members[off];
    const bool o0 = (member_mirrored[off] != 0) != f;
    const int side = s0->side;
    for (int e = tid; e < XQ_STATE_FLOATS; e += GB_THREADS) st[e] = plane_entry(s0, side, o0, e);

    if (nm == 1) {                                   // k_samples_to_batch's path: zero fill, then the scatter of the one record
        for (int i = tid; i < XQ_ACTION_SPACE / 4; i += GB_THREADS) p4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        __syncthreads();                             // orders the workgroup's zero fill before wave 0's scatter
        if (tid >= 64) return;
        const int m = s0->n_moves < XQ_MAXM ? s0->n_moves : XQ_MAXM;
        double w[2];
        const double total = member_weights(s0, m, late_temperature, lane, w);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int i = lane + 64 * h;
            if (i < m) {
                const int a = s0->actions[i];
                if (a < XQ_ACTION_SPACE)
                    pi[(size_t)o * XQ_ACTION_SPACE + (o0 ? mirror_action(a) : a)] = total > 0.0 ? (float)(w[h] / total) : 0.0f;
            }
        }
        if (lane == 0) z[o] = (float)member_z(s0, q_mix);
        return;
    }

    for (int i = tid; i < XQ_ACTION_SPACE; i += GB_THREADS) acc[i] = 0.0;
    __syncthreads();
    if (tid < 64) {                                  // wave 0 takes the members one after the other: the sums are in member order
        double zsum = 0.0;
        int n_pi = 0;
        for (int k = 0; k < nm; ++k) {
            const xq_sample *s = rec + members[off + k];
            const bool ok = (member_mirrored[off + k] != 0) != f;
            const int m = s->n_moves < XQ_MAXM ? s->n_moves : XQ_MAXM;
            double w[2];
            const double total = member_weights(s, m, late_temperature, lane, w);
            zsum += member_z(s, q_mix);
            if (total > 0.0) {                       // wave-uniform: a valid member
                ++n_pi;
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int i = lane + 64 * h;
                    if (i < m) {
                        const int a = s->actions[i];
                        if (a < XQ_ACTION_SPACE) {
                            const int d = ok ? mirror_action(a) : a;
                            acc[d] = acc[d] + w[h] / total;
                        }
                    }
                }
                wave_sync();                         // member k's sums are in LDS before member k + 1 reads them
            }
        }
        if (lane == 0) {
            s_n_pi = n_pi;
            z[o] = (float)(zsum / (double)nm);
        }
    }
    __syncthreads();
    const double n_pi = (double)s_n_pi;
    for (int i = tid; i < XQ_ACTION_SPACE / 4; i += GB_THREADS) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (n_pi > 0.0) {
            v.x = (float)(acc[4 * i] / n_pi); v.y = (float)(acc[4 * i + 1] / n_pi);
            v.z = (float)(acc[4 * i + 2] / n_pi); v.w = (float)(acc[4 * i + 3] / n_pi);
        }
        p4[i] = v;
    }
}

}  // namespace

extern "C" {

uint64_t xq_position_key_host(const int8_t *board, int8_t side, int flags, uint8_t *mirrored) {
    if (mirrored) *mirrored = 0;
    if (!board || (flags & ~XQ_POSITION_KEY_MIRROR)) return 0;
    int mir = 0;
    if (flags & XQ_POSITION_KEY_MIRROR) {
        int first = -1;
        for (int sq = 0; sq < XQ_SQUARES && first < 0; ++sq)
            if (board[sq] != board[mir_sq(sq)]) first = sq;
        mir = mirrored_of(board, first);
    }
    uint64_t k = 0;
    for (int sq = 0; sq < XQ_SQUARES; ++sq) k ^= key_term(sq, board[mir ? mir_sq(sq) : sq]);
    k ^= key_term(XQ_SQUARES, side);
    if (mirrored) *mirrored = (uint8_t)mir;
    return k;
}

int xq_position_keys(const void *dev_samples, const int32_t *dev_index, int n, int flags, uint64_t *dev_keys, uint8_t *dev_mirrored,
                     void *stream) {
    if (n < 0 || (flags & ~XQ_POSITION_KEY_MIRROR)) return XQ_ERR_ARG;
    if (n > 0 && (!dev_samples || !dev_keys || !dev_mirrored)) return XQ_ERR_ARG;
    if ((uintptr_t)dev_keys & 7) return XQ_ERR_ARG;
    if (n == 0) return XQ_OK;
    hipLaunchKernelGGL(k_position_keys, dim3((n + KWPW - 1) / KWPW), dim3(64 * KWPW), 0, (hipStream_t)stream,
                       (const xq_sample *)dev_samples, dev_index, n, flags, dev_keys, dev_mirrored);
    return launch_status();
}

int xq_position_group_heads(const void *dev_samples, const int32_t *dev_index, const int32_t *dev_order, const uint64_t *dev_keys,
                            const uint8_t *dev_mirrored, int n, uint8_t *dev_head, void *stream) {
    if (n < 0) return XQ_ERR_ARG;
    if (n > 0 && (!dev_samples || !dev_order || !dev_keys || !dev_mirrored || !dev_head)) return XQ_ERR_ARG;
    if ((uintptr_t)dev_keys & 7) return XQ_ERR_ARG;
    if (n == 0) return XQ_OK;
    hipLaunchKernelGGL(k_position_group_heads, dim3((n + KWPW - 1) / KWPW), dim3(64 * KWPW), 0, (hipStream_t)stream,
                       (const xq_sample *)dev_samples, dev_index, dev_order, dev_keys, dev_mirrored, n, dev_head);
    return launch_status();
}

int xq_groups_to_batch(const void *dev_samples, const int32_t *dev_group_offsets, const int32_t *dev_members,
                       const uint8_t *dev_member_mirrored, int n_groups, const int32_t *dev_group, const uint8_t *dev_flip, int n,
                       double late_temperature, const xq_batch_opts *opts, float *dev_states, float *dev_pi, float *dev_z,
                       void *stream) {
    if (opts && (!(opts->q_mix >= 0.0 && opts->q_mix <= 1.0) || opts->reserved[0] != 0 || opts->reserved[1] != 0)) return XQ_ERR_ARG;
    if (n < 0 || n_groups < 0) return XQ_ERR_ARG;
    if (n > 0 && (!dev_group || !dev_flip || !dev_states || !dev_pi || !dev_z)) return XQ_ERR_ARG;
    if (n > 0 && n_groups > 0 && (!dev_samples || !dev_group_offsets || !dev_members || !dev_member_mirrored)) return XQ_ERR_ARG;
    if (!(late_temperature > 0.0) || ((uintptr_t)dev_pi & 15)) return XQ_ERR_ARG;
    if (n == 0) return XQ_OK;
    hipLaunchKernelGGL(k_groups_to_batch, dim3(n), dim3(GB_THREADS), 0, (hipStream_t)stream, (const xq_sample *)dev_samples,
                       dev_group_offsets, dev_members, dev_member_mirrored, n_groups, dev_group, dev_flip, n, late_temperature,
                       opts ? opts->q_mix : 0.0, dev_states, dev_pi, dev_z);
    return launch_status();
}

}  // extern "C"
