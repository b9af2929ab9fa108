// xq_evkey.cuh -- the exact key of one evaluation request, shared by the evaluation cache (xq_evcache.hip) and the request
// dedup (xq_evdedup.hip).  A request's output depends only on its 15 input planes, and the key is an injective packing of them:
//
//   key   : 90 squares x 4 bits (1 + the plane 0..13 that holds the square's piece, 0 = empty) and the side to move (plane
//           14) as nibble 90; nibble i sits at bits 4 (i mod 8) of word i / 8 -- 12 words, injective over k_select's planes.
//
// Device and host helpers only, as in xq_engine_state.cuh: every kernel lives in one unit.
#pragma once

#include "xq_engine_state.cuh"

#pragma clang fp contract(off)

namespace {

constexpr int EC_KEYW = 12;

// nibble of square sq (sq < 90): 1 + the piece plane that is set there, 0 when none is
__host__ __device__ inline uint32_t evkey_nibble(const float *planes, int sq) {
    uint32_t n = 0;
    for (int p = 0; p < 14; ++p) n = planes[p * 90 + sq] != 0.0f ? (uint32_t)(p + 1) : n;
    return n;
}

__host__ __device__ inline uint32_t evkey_side(const float *planes) { return planes[14 * 90] != 0.0f ? 1u : 0u; }

__host__ __device__ inline uint32_t evkey_hash(const uint32_t *k) {
    uint32_t h = 0x811C9DC5u;
    for (int i = 0; i < EC_KEYW; ++i) h = (h ^ k[i]) * 0x01000193u;
    h ^= h >> 16; h *= 0x7FEB352Du; h ^= h >> 15;
    return h;
}

// the 12 key words of one slot's planes, built by one wave: lane l decodes squares l and 64 + l (or the side at 90), groups
// of eight lanes OR their shifted nibbles into one word, and every lane receives all 12 words
__device__ inline void wave_evkey(const float *__restrict__ x, uint32_t key[EC_KEYW]) {
    const int lane = lane_id(), sq1 = 64 + lane;
    uint32_t lo = evkey_nibble(x, lane) << (4 * (lane & 7));
    const uint32_t n1 = sq1 < 90 ? evkey_nibble(x, sq1) : (sq1 == 90 ? evkey_side(x) : 0u);
    uint32_t hi = n1 << (4 * (lane & 7));
#pragma unroll
    for (int o = 1; o < 8; o <<= 1) {
        lo |= (uint32_t)__shfl_xor((int)lo, o);
        hi |= (uint32_t)__shfl_xor((int)hi, o);
    }
#pragma unroll
    for (int w = 0; w < 8; ++w) key[w] = (uint32_t)__shfl((int)lo, 8 * w);
#pragma unroll
    for (int w = 0; w < 4; ++w) key[8 + w] = (uint32_t)__shfl((int)hi, 8 * w);
}

__device__ __forceinline__ bool key_eq(const uint32_t *__restrict__ e, const uint32_t key[EC_KEYW]) {
    const uint4 a = ((const uint4 *)e)[0], b = ((const uint4 *)e)[1], c = ((const uint4 *)e)[2];
    return a.x == key[0] && a.y == key[1] && a.z == key[2] && a.w == key[3] && b.x == key[4] && b.y == key[5] &&
           b.z == key[6] && b.w == key[7] && c.x == key[8] && c.y == key[9] && c.z == key[10] && c.w == key[11];
}

}  // namespace
