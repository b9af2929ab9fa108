// xq_tools.cuh -- what the stateless device tools share (xq_batch.hip, xq_replay.hip, xq_supervise.hip, xq_alphabeta.hip,
// xq_mate.hip): the one-wave-per-item prologue and the scaffold of a search per root move.
// Nothing of the engine includes this header.
#pragma once

#include "xq_common.h"
#include "xq_rules.cuh"

namespace xq {

// four items per 256-thread workgroup, one per wave; LDS carved per wave, no workgroup barrier (see xq_rules.cuh)
constexpr int WPW = 4;
#define XQ_WAVE_ITEM(n)                                             \
    const int wv = (int)(threadIdx.x >> 6);                         \
    const int i = blockIdx.x * WPW + wv;                            \
    if (i >= (n)) return;

__device__ __forceinline__ int ld_uniform(const int *p) { return __builtin_amdgcn_readfirstlane(*p); }

// ---- a search per root move (xq_alphabeta.hip, xq_mate.hip): a root kernel with one wave per position, then a search kernel
// with one wave per (position, root move), XQ_MAXM waves per position, four per 256-thread workgroup, LDS carved per wave and no
// workgroup barrier; launched over chunks of positions
struct RootLds {
    __attribute__((aligned(16))) int8_t board[XQ_BS];
    MoveGenLds mg;
    uint16_t moves[XQ_MAXM];
};

// Position i of a root kernel: the king test, the ordered root moves (zeros past the count, <= XQ_MAXM), counts[i] and status[i]
// (0 fine, 1 capacity, 2 a king is missing).  defaults(o, live) gives the kernel's own per-move words at index o their values:
// every one of them is written here, and the search overwrites those of the live moves, the ones below the count.
template <class F>
__device__ __forceinline__ void wave_root_moves(const int8_t *__restrict__ boards, const int8_t *__restrict__ side, int i, RootLds &L,
                                                uint16_t *__restrict__ moves, uint16_t *__restrict__ counts,
                                                uint8_t *__restrict__ status, F defaults) {
    const int lane = lane_id();
    wave_load_board(boards + (size_t)i * 90, L.board);
    wave_sync();
    const VMove none{-1, -1, 0};
    int cnt = 0, st = 0;
    if (find_king(L.board, none, 1) < 0 || find_king(L.board, none, -1) < 0) {
        st = 2;
    } else {
        int ovf = 0;
        cnt = wave_movegen(L.board, (int)side[i], L.mg, L.moves, &ovf);
        st = ovf;
    }
    for (int j = lane; j < XQ_MAXM; j += 64) {
        const size_t o = (size_t)i * XQ_MAXM + j;
        moves[o] = j < cnt ? L.moves[j] : (uint16_t)0;
        defaults(o, j < cnt);
    }
    if (lane == 0) {
        counts[i] = (uint16_t)cnt;
        status[i] = (uint8_t)st;
    }
}

// The wave of a search kernel: wv, lane, position i, root move j = from -> to (a legal move: both squares are below 90), root_side
// to move at the root.  A wave past the positions or past the position's count exits at once: it has nothing to search.
#define XQ_WAVE_ROOT_MOVE(n, side, moves, counts)                                                          \
    const int wv = (int)(threadIdx.x >> 6);                                                                \
    const int w = (int)blockIdx.x * WPW + wv; /* < n * XQ_MAXM <= 2^25 (for_position_chunks) */            \
    const int i = w / XQ_MAXM, j = w % XQ_MAXM;                                                            \
    if (i >= (n)) return;                                                                                  \
    if (j >= __builtin_amdgcn_readfirstlane((int)(counts)[i])) return;                                     \
    const int lane = lane_id();                                                                            \
    const int root_side = __builtin_amdgcn_readfirstlane((int)(side)[i]);                                  \
    const int action = __builtin_amdgcn_readfirstlane((int)(moves)[(size_t)i * XQ_MAXM + j]);              \
    const int from = action / 90, to = action - from * 90;

// from -> to played on `dst`, which holds `src`'s position: src itself (the root move, in place on level 0) or the copy of it
// that wave_child_board makes a level down.  Boards are copied per ply, never unmade.  The caller's wave_sync() publishes the
// move, after lane 0's further stores for the new level where it has any.
__device__ __forceinline__ void wave_play(int8_t *dst, const int8_t *src, int from, int to) {
    const int mover = src[from];
    wave_sync();
    if (lane_id() == 0) { dst[to] = (int8_t)mover; dst[from] = 0; }
}

__device__ __forceinline__ void wave_child_board(int8_t *dst, const int8_t *src, int action) {
    const int from = action / 90, to = action - from * 90;
    lds_copy_dwords(dst, src, XQ_BS / 4);
    wave_play(dst, src, from, to);
}

// fn(first position, positions) over chunks of the n positions, so that no grid passes 2^31 threads (a search's has
// XQ_MAXM * 64 per position)
template <class F>
inline void for_position_chunks(int n, F fn) {
    constexpr int CHUNK = 1 << 18;
    for (int base = 0; base < n; base += CHUNK) fn((size_t)base, n - base < CHUNK ? n - base : CHUNK);
}

}  // namespace xq
