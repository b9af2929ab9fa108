// xq_tb_index.cuh -- the dense index of the endgame tables (include/xq_hip.h, xq_tb_*) as more than one unit needs it: the
// admissible squares, a signature by value, one decoded entry, and the matching of a board against a signature.  xq_tablebase.hip
// generates, probes and plays with it; xq_adjudicate.hip matches the real boards of the engine's games.  Device and host helpers
// only: every kernel lives in one unit.  Include after xq_rules.cuh (find_king, lane_id).
#pragma once

#include "xq_common.h"
#include "xq_rules.cuh"

using namespace xq;

namespace {

// ---- the admissible squares of every piece kind and colour, built at compile time: one copy for the host, one for the device
struct TbTables {
    uint8_t nsq[8];              // admissible squares by kind (the same for both colours)
    uint8_t sq[2][8][90];        // [black][kind][digit] -> square, in row-major order of the square
    uint8_t dig[2][8][90];       // [black][kind][square] -> digit, 0xFF outside the list
};

constexpr bool tb_red_admissible(int kind, int s) {
    const int r = s / 9, c = s % 9;
    if (kind == 2) return (r == 1 && c == 4) || ((r == 0 || r == 2) && (c == 3 || c == 5));
    if (kind == 3) return ((r == 0 || r == 4) && (c == 2 || c == 6)) || (r == 2 && (c == 0 || c == 4 || c == 8));
    if (kind == 7) return r >= 5 || ((r == 3 || r == 4) && c % 2 == 0);
    return kind >= 4 && kind <= 6;
}

constexpr TbTables tb_make_tables() {
    TbTables t{};
    for (int kind = 0; kind < 8; ++kind)
        for (int black = 0; black < 2; ++black) {
            int n = 0;
            for (int s = 0; s < 90; ++s) {
                t.dig[black][kind][s] = 0xFF;
                if (tb_red_admissible(kind, black ? 89 - s : s)) {
                    t.sq[black][kind][n] = (uint8_t)s;
                    t.dig[black][kind][s] = (uint8_t)n;
                    ++n;
                }
            }
            t.nsq[kind] = (uint8_t)n;
        }
    return t;
}

constexpr TbTables H_TB = tb_make_tables();
__constant__ TbTables D_TB = tb_make_tables();

// ---- a signature as the kernels take it, by value: per piece its code, its radix (squares + 1, the last digit is "captured"),
// the index units of one step of its digit, and how many earlier pieces of the signature carry the same code
struct TbSig {
    int32_t P;
    int32_t entries;                       // <= XQ_TB_MAX_ENTRIES
    int32_t s_side, s_rk, s_bk;            // index units of the side, the red king's and the black king's digit
    int32_t code[XQ_TB_MAX_PIECES];
    int32_t radix[XQ_TB_MAX_PIECES];
    int32_t stride[XQ_TB_MAX_PIECES];
    int32_t rank[XQ_TB_MAX_PIECES];
};

// 0 entries: a bad signature, or one beyond XQ_TB_MAX_ENTRIES
inline long long make_sig(const int8_t *pieces, int P, TbSig &S) {
    S = TbSig{};
    if (P < 0 || P > XQ_TB_MAX_PIECES || (P > 0 && !pieces)) return 0;
    long long entries = 162;
    for (int p = 0; p < P; ++p) {
        const int c = pieces[p], kind = c < 0 ? -c : c;
        if (kind < 2 || kind > 7) return 0;
        S.code[p] = c;
        S.radix[p] = H_TB.nsq[kind] + 1;
        for (int q = 0; q < p; ++q) S.rank[p] += pieces[q] == c;
        entries *= S.radix[p];
        if (entries > XQ_TB_MAX_ENTRIES) return 0;
    }
    S.P = P;
    S.entries = (int32_t)entries;
    int32_t unit = 1;
    for (int p = P - 1; p >= 0; --p) { S.stride[p] = unit; unit *= S.radix[p]; }
    S.s_bk = unit;
    S.s_rk = unit * 9;
    S.s_side = unit * 81;
    return entries;
}

// one entry, decoded; everything here is wave-uniform
struct TbPos {
    int side;                              // +1 red to move, -1 black
    int rk, bk, rk_sq, bk_sq;              // the kings' digits and squares
    int dig[XQ_TB_MAX_PIECES], sq[XQ_TB_MAX_PIECES];      // sq -1: captured
};

// the square of the (rank + 1)-th piece `code` of the board in row-major order, -1 when there are not that many
__device__ __forceinline__ int tb_nth_piece(int p0, int p1, int code, int rank) {
    unsigned long long m0 = __ballot(p0 == code), m1 = __ballot(p1 == code);
    for (int r = 0; r < rank; ++r) {
        if (m0) m0 &= m0 - 1ull;
        else if (m1) m1 &= m1 - 1ull;
    }
    return m0 ? __ffsll((long long)m0) - 1 : (m1 ? 64 + __ffsll((long long)m1) - 1 : -1);
}

// k_tb_probe's matching as a function (the probe keeps its own text: its object code is held fixed).  The board of an LDS slot
// against the signature, `side` wave-uniform (1 is red, anything else black): pos, and the status bits +1 (not in this table) and
// +2 (a king is missing); with status 0, e is the entry's index.
__device__ __forceinline__ int tb_match(const TbSig &S, const int8_t *board, int side, TbPos &pos, int &e) {
    const int lane = lane_id();
    const int p0 = board[lane], p1 = lane < 32 ? (int)board[lane + 64] : 0;         // padding reads 0
    const VMove none{-1, -1, 0};
    pos.side = side == 1 ? 1 : -1;
    pos.rk_sq = find_king(board, none, 1);
    pos.bk_sq = find_king(board, none, -1);
    int st = (pos.rk_sq < 0 || pos.bk_sq < 0) ? 2 : 0;
    // greedy, in signature order: the r-th piece of a code in the signature takes the r-th such piece of the board
    int matched = 0;
    e = pos.side == 1 ? 0 : S.s_side;
#pragma unroll
    for (int p = 0; p < XQ_TB_MAX_PIECES; ++p) {
        pos.dig[p] = 0;
        pos.sq[p] = -1;
        if (p < S.P) {
            const int code = S.code[p];
            const int sq = tb_nth_piece(p0, p1, code, S.rank[p]);
            int d = S.radix[p] - 1;                            // absent from the board: captured
            if (sq >= 0) {
                ++matched;
                d = (int)D_TB.dig[code < 0][code < 0 ? -code : code][sq];
                if (d == 0xFF) { st |= 1; d = 0; }             // a square outside the piece's list
            }
            pos.sq[p] = sq;
            pos.dig[p] = d;
            e += d * S.stride[p];
        }
    }
    const int men = __popcll(__ballot(p0 != 0)) + __popcll(__ballot(p1 != 0));
    // a piece the signature lacks (a second king, or one outside its palace, is one)
    if (men != matched + (pos.rk_sq >= 0) + (pos.bk_sq >= 0)) st |= 1;
    if (st == 0) {
        pos.rk = (pos.rk_sq / 9) * 3 + pos.rk_sq % 9 - 3;
        pos.bk = (pos.bk_sq / 9 - 7) * 3 + pos.bk_sq % 9 - 3;
        e += pos.rk * S.s_rk + pos.bk * S.s_bk;                // < S.entries: every digit is below its radix
    }
    return st;
}

}  // namespace
