// xq_tablebase.hip -- endgame tablebases by retrograde analysis over a dense index (include/xq_hip.h, xq_tb_*): the exact value of
// every position of a signature of up to XQ_TB_MAX_PIECES non-king pieces, as plies to the end under the move generator's rules
// alone.  A stateless device tool beside xq_alphabeta.hip and xq_mate.hip; nothing of the engine knows of it.
//   k_tb_init    pass 0, one wave per entry: decode the index into an LDS board; XQ_TB_INVALID, -1 (no legal move) or 0;
//   k_tb_pass    pass k >= 1, one wave per entry, in place: a wave whose entry is not 0 exits after one load; otherwise every lane
//                computes the child index of its move from the parent's digits and loads the child's value;
//   k_tb_probe   one wave per position: the board matched against the signature, the value, and every root move's value;
//   k_tb_play    one wave per position: the probe's work, then one move (the table's best, or the caller's) played on the board;
//   k_tb_samples one wave per entry: pass k's decoding and the probe's move values, written as one xq_sample row.
// Index, digits, strides and squares of one entry are wave-uniform.  No atomics, no scratch, no workgroup barrier.
#include "xq_tools.cuh"
#include "xq_tb_index.cuh"

using namespace xq;

namespace {

__device__ __forceinline__ int tb_palace_square(int digit, int black) { return ((black ? 7 : 0) + digit / 3) * 9 + 3 + digit % 3; }

__device__ __forceinline__ void tb_decode(const TbSig &S, int e, TbPos &pos) {
    int x = e;
#pragma unroll
    for (int p = XQ_TB_MAX_PIECES - 1; p >= 0; --p) {
        pos.dig[p] = 0;
        pos.sq[p] = -1;
        if (p < S.P) {
            const int q = x / S.radix[p], d = x - q * S.radix[p];
            x = q;
            pos.dig[p] = d;
            const int c = S.code[p];
            if (d < S.radix[p] - 1) pos.sq[p] = D_TB.sq[c < 0][c < 0 ? -c : c][d];
        }
    }
    pos.bk = x % 9; x /= 9;
    pos.rk = x % 9; x /= 9;
    pos.side = x ? -1 : 1;
    pos.rk_sq = tb_palace_square(pos.rk, 0);
    pos.bk_sq = tb_palace_square(pos.bk, 1);
}

// two men on one square (the kings' palaces are disjoint)
__device__ __forceinline__ bool tb_collision(const TbSig &S, const TbPos &pos) {
    bool hit = false;
#pragma unroll
    for (int p = 0; p < XQ_TB_MAX_PIECES; ++p) {
        if (p < S.P && pos.sq[p] >= 0) {
            hit = hit || pos.sq[p] == pos.rk_sq || pos.sq[p] == pos.bk_sq;
#pragma unroll
            for (int q = 0; q < p; ++q) hit = hit || pos.sq[q] == pos.sq[p];
        }
    }
    return hit;
}

// the entry's board into a 96-byte LDS slot, padding zeroed; the caller's wave_sync() publishes it
__device__ __forceinline__ void tb_store_board(const TbSig &S, const TbPos &pos, int8_t *b) {
    const int lane = lane_id();
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int j = lane + 64 * h;
        int v = j == pos.rk_sq ? 1 : (j == pos.bk_sq ? -1 : 0);
#pragma unroll
        for (int p = 0; p < XQ_TB_MAX_PIECES; ++p)
            if (p < S.P) v = pos.sq[p] == j ? S.code[p] : v;
        if (j < XQ_BS) b[j] = (int8_t)v;
    }
}

// The index of the entry that legal move from -> to of entry e leads to: the mover's digit changes, a captured piece's digit
// becomes "captured", the side flips.  A legal move keeps every man within its list of squares and never takes a king.
__device__ __forceinline__ int tb_child_index(const TbSig &S, const TbPos &pos, int e, int from, int to) {
    int c = e + (pos.side == 1 ? S.s_side : -S.s_side);
    const int tr = to / 9, tc = to - tr * 9;
    if (from == pos.rk_sq) c += (tr * 3 + tc - 3 - pos.rk) * S.s_rk;
    if (from == pos.bk_sq) c += ((tr - 7) * 3 + tc - 3 - pos.bk) * S.s_bk;
#pragma unroll
    for (int p = 0; p < XQ_TB_MAX_PIECES; ++p) {
        if (p < S.P) {
            const int code = S.code[p];
            if (pos.sq[p] == from) c += ((int)D_TB.dig[code < 0][code < 0 ? -code : code][to] - pos.dig[p]) * S.stride[p];
            if (pos.sq[p] == to) c += (S.radix[p] - 1 - pos.dig[p]) * S.stride[p];
        }
    }
    return c;
}

// the value of lane-owned move `a` of entry e: the child's table word; 0 for a lane without a move.  The range test never fires
// for a legal move (above); it keeps a load inside the table whatever the index arithmetic was given.
__device__ __forceinline__ int tb_child_value(const TbSig &S, const TbPos &pos, const int16_t *table, int e, bool live, int a) {
    if (!live) return 0;
    const int from = a / 90, to = a - from * 90;
    const int c = tb_child_index(S, pos, e, from, to);
    return (unsigned)c < (unsigned)S.entries ? (int)table[c] : 0;
}

// what the mover gets by a move into a child of table word c: a child lost in p plies (-(p + 1)) gives +(p + 1); a child won in
// p plies (+p) gives -(p + 2); a drawn child 0
__device__ __forceinline__ int tb_move_value(int c) { return c < 0 ? -c : (c > 0 ? -(c + 2) : 0); }

// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64 * WPW) void k_tb_init(TbSig S, int16_t *__restrict__ table, int base, int m) {
    __shared__ RootLds Ls[WPW];
    XQ_WAVE_ITEM(m)
    RootLds &L = Ls[wv];
    const int e = base + i;
    TbPos pos;
    tb_decode(S, e, pos);
    int v = XQ_TB_INVALID;
    if (!tb_collision(S, pos)) {
        tb_store_board(S, pos, L.board);
        wave_sync();
        if (!wave_in_check(L.board, -pos.side)) {
            int ovf = 0;
            v = wave_movegen(L.board, pos.side, L.mg, L.moves, &ovf) == 0 ? -1 : 0;
        }
    }
    if (lane_id() == 0) table[e] = (int16_t)v;
}

__global__ __launch_bounds__(64 * WPW) void k_tb_pass(TbSig S, int16_t *table, int base, int m, int k, int32_t *changed) {
    __shared__ RootLds Ls[WPW];
    XQ_WAVE_ITEM(m)
    const int e = base + i;
    if (__builtin_amdgcn_readfirstlane((int)table[e]) != 0) return;
    RootLds &L = Ls[wv];
    const int lane = lane_id();
    TbPos pos;
    tb_decode(S, e, pos);
    tb_store_board(S, pos, L.board);
    wave_sync();
    int ovf = 0;
    const int cnt = wave_movegen(L.board, pos.side, L.mg, L.moves, &ovf);       // >= 1: pass 0 gave an entry without a move its -1
    const int v0 = tb_child_value(S, pos, table, e, lane < cnt, (int)L.moves[lane]);
    const int v1 = tb_child_value(S, pos, table, e, lane + 64 < cnt, (int)L.moves[lane + 64]);
    int decided = 0;
    if (k & 1) {
        if (__ballot((lane < cnt && v0 == -k) || (lane + 64 < cnt && v1 == -k)) != 0ull) decided = k;
    } else {
        const bool open = (lane < cnt && v0 <= 0) || (lane + 64 < cnt && v1 <= 0);
        const int best = wave_max(v0 > v1 ? v0 : v1);         // a lane without a move holds 0
        if (__ballot(open) == 0ull && best == k - 1) decided = -(k + 1);
    }
    if (decided != 0 && lane == 0) {
        table[e] = (int16_t)decided;
        *changed = 1;
    }
}

__global__ __launch_bounds__(64 * WPW) void k_tb_probe(TbSig S, const int16_t *__restrict__ table, const int8_t *__restrict__ boards,
                                                        const int8_t *__restrict__ side, int n, int16_t *__restrict__ value,
                                                        uint16_t *__restrict__ moves, uint16_t *__restrict__ counts,
                                                        int16_t *__restrict__ move_value, uint16_t *__restrict__ best_action,
                                                        uint8_t *__restrict__ status) {
    __shared__ RootLds Ls[WPW];
    XQ_WAVE_ITEM(n)
    RootLds &L = Ls[wv];
    const int lane = lane_id();
    wave_load_board(boards + (size_t)i * 90, L.board);
    wave_sync();
    const int p0 = L.board[lane], p1 = lane < 32 ? (int)L.board[lane + 64] : 0;         // padding reads 0
    const VMove none{-1, -1, 0};
    TbPos pos;
    pos.side = __builtin_amdgcn_readfirstlane((int)side[i]) == 1 ? 1 : -1;
    pos.rk_sq = find_king(L.board, none, 1);
    pos.bk_sq = find_king(L.board, none, -1);
    int st = (pos.rk_sq < 0 || pos.bk_sq < 0) ? 2 : 0;
    // greedy, in signature order: the r-th piece of a code in the signature takes the r-th such piece of the board
    int matched = 0;
    int e = pos.side == 1 ? 0 : S.s_side;
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
    int v = 0, cnt = 0, act = XQ_TB_NO_MOVE;
    if (st == 0) {
        pos.rk = (pos.rk_sq / 9) * 3 + pos.rk_sq % 9 - 3;
        pos.bk = (pos.bk_sq / 9 - 7) * 3 + pos.bk_sq % 9 - 3;
        e += pos.rk * S.s_rk + pos.bk * S.s_bk;                // < S.entries: every digit is below its radix
        v = __builtin_amdgcn_readfirstlane((int)table[e]);
        if (v == XQ_TB_INVALID) { st = 4; v = 0; }
    }
    int mv0 = 0, mv1 = 0;
    if (st == 0) {
        int ovf = 0;
        cnt = wave_movegen(L.board, pos.side, L.mg, L.moves, &ovf);
        // a child lost in p plies (-(p + 1)) gives +(p + 1); a child won in p plies (+p) gives -(p + 2); a drawn child 0
        const int c0 = tb_child_value(S, pos, table, e, lane < cnt, (int)L.moves[lane]);
        const int c1 = tb_child_value(S, pos, table, e, lane + 64 < cnt, (int)L.moves[lane + 64]);
        mv0 = c0 < 0 ? -c0 : (c0 > 0 ? -(c0 + 2) : 0);
        mv1 = c1 < 0 ? -c1 : (c1 > 0 ? -(c1 + 2) : 0);
        const unsigned long long b0 = __ballot(lane < cnt && mv0 == v), b1 = __ballot(lane + 64 < cnt && mv1 == v);
        if (b0) act = (int)L.moves[__ffsll((long long)b0) - 1];
        else if (b1) act = (int)L.moves[64 + __ffsll((long long)b1) - 1];
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int j = lane + 64 * h;
        const size_t o = (size_t)i * XQ_MAXM + j;
        moves[o] = j < cnt ? L.moves[j] : (uint16_t)0;
        if (move_value) move_value[o] = (int16_t)(j < cnt ? (h ? mv1 : mv0) : 0);
    }
    if (lane == 0) {
        value[i] = (int16_t)v;
        counts[i] = (uint16_t)cnt;
        best_action[i] = (uint16_t)act;
        status[i] = (uint8_t)st;
    }
}

// The first set bit of the 128 (b0: moves 0..63, b1: moves 64..127), -1 when there is none.
__device__ __forceinline__ int tb_first_move(unsigned long long b0, unsigned long long b1) {
    return b0 ? __ffsll((long long)b0) - 1 : (b1 ? 64 + __ffsll((long long)b1) - 1 : -1);
}

// One move per position: the probe's matching and move values, then the chosen move (the table's, or the caller's looked up among
// the ordered legal moves) played on the LDS board.  boards_out / side_out may be boards / side: the item is in LDS and registers
// before the first store, so neither pair is __restrict__.
__global__ __launch_bounds__(64 * WPW) void k_tb_play(TbSig S, const int16_t *__restrict__ table, const int8_t *boards, const int8_t *side,
                                                       const uint16_t *__restrict__ action, int n, int8_t *boards_out, int8_t *side_out,
                                                       uint16_t *__restrict__ played, int16_t *__restrict__ value,
                                                       int16_t *__restrict__ move_value, int16_t *__restrict__ value_out,
                                                       uint8_t *__restrict__ status) {
    __shared__ RootLds Ls[WPW];
    XQ_WAVE_ITEM(n)
    RootLds &L = Ls[wv];
    const int lane = lane_id();
    wave_load_board(boards + (size_t)i * 90, L.board);
    const int side_in = __builtin_amdgcn_readfirstlane((int)side[i]);
    const int want = action ? __builtin_amdgcn_readfirstlane((int)action[i]) : XQ_TB_NO_MOVE;
    wave_sync();
    TbPos pos;
    int e;
    int st = tb_match(S, L.board, side_in, pos, e);
    int v = 0, act = XQ_TB_NO_MOVE, mv = 0, child = 0;
    if (st == 0) {
        v = __builtin_amdgcn_readfirstlane((int)table[e]);
        if (v == XQ_TB_INVALID) { st = 4; v = 0; }
        else if (v == -1) st = 8;                              // -1 is "no legal move now" and nothing else (pass 0)
    }
    if (st == 0) {
        int ovf = 0;
        const int cnt = wave_movegen(L.board, pos.side, L.mg, L.moves, &ovf);
        const int c0 = tb_child_value(S, pos, table, e, lane < cnt, (int)L.moves[lane]);
        const int c1 = tb_child_value(S, pos, table, e, lane + 64 < cnt, (int)L.moves[lane + 64]);
        const int mv0 = tb_move_value(c0), mv1 = tb_move_value(c1);
        const bool pick0 = lane < cnt && (want == XQ_TB_NO_MOVE ? mv0 == v : (int)L.moves[lane] == want);
        const bool pick1 = lane + 64 < cnt && (want == XQ_TB_NO_MOVE ? mv1 == v : (int)L.moves[lane + 64] == want);
        const int j = tb_first_move(__ballot(pick0), __ballot(pick1));
        if (j < 0) {
            st = cnt == 0 ? 8 : 16;        // a valid entry's value is some move's value, so the table always finds its move
        } else {
            act = (int)L.moves[j];
            mv = __shfl(j < 64 ? mv0 : mv1, j & 63);
            child = __shfl(j < 64 ? c0 : c1, j & 63);
            wave_play(L.board, L.board, act / 90, act - (act / 90) * 90);
            wave_sync();
        }
    }
    int8_t *out = boards_out + (size_t)i * 90;
    out[lane] = L.board[lane];
    if (lane + 64 < 90) out[lane + 64] = L.board[lane + 64];
    if (lane == 0) {
        side_out[i] = (int8_t)(st == 0 ? -pos.side : side_in);
        played[i] = (uint16_t)act;
        value[i] = (int16_t)v;
        move_value[i] = (int16_t)mv;
        value_out[i] = (int16_t)child;
        status[i] = (uint8_t)st;
    }
}

constexpr int ROW_CHUNKS = XQ_SAMPLE_BYTES / 16;    // a row is 40 16-byte stores, one per lane

static_assert(sizeof(xq_sample) == XQ_SAMPLE_BYTES && XQ_SAMPLE_BYTES % 16 == 0, "xq_sample layout");
static_assert(offsetof(xq_sample, side) == 90 && offsetof(xq_sample, n_moves) == 92 && offsetof(xq_sample, ply) == 94 &&
              offsetof(xq_sample, slot) == 100 && offsetof(xq_sample, game_seq) == 104 && offsetof(xq_sample, actions) == 128 &&
              offsetof(xq_sample, visits) == 384, "xq_sample layout");

// Entries as xq_sample rows, the row layout of k_records_to_samples (xq_supervise.hip): the decoded board's 96 LDS bytes are the
// row's first 96 (tb_store_board zeroes bytes 90..95), and a visit is one bit of the optimal moves' ballots.
__global__ __launch_bounds__(64 * WPW) void k_tb_samples(TbSig S, const int16_t *__restrict__ table, const int32_t *__restrict__ index,
                                                          int n, int policy, uint4 *__restrict__ samples, uint8_t *__restrict__ status) {
    __shared__ RootLds Ls[WPW];
    XQ_WAVE_ITEM(n)
    RootLds &L = Ls[wv];
    const int lane = lane_id();
    const int e = __builtin_amdgcn_readfirstlane(index[i]);
    int st = 0, v = 0;
    if ((unsigned)e >= (unsigned)S.entries) {
        st = 1;
    } else {
        v = __builtin_amdgcn_readfirstlane((int)table[e]);
        st = v == XQ_TB_INVALID ? 4 : (v == -1 ? 8 : 0);       // -1 is "no legal move now" and nothing else (pass 0)
    }
    uint4 row = make_uint4(0u, 0u, 0u, 0u);
    if (st == 0) {
        TbPos pos;
        tb_decode(S, e, pos);
        tb_store_board(S, pos, L.board);
        wave_sync();
        int ovf = 0;
        const int cnt = wave_movegen(L.board, pos.side, L.mg, L.moves, &ovf);       // >= 1: the entry is not -1
        const int mv0 = tb_move_value(tb_child_value(S, pos, table, e, lane < cnt, (int)L.moves[lane]));
        const int mv1 = tb_move_value(tb_child_value(S, pos, table, e, lane + 64 < cnt, (int)L.moves[lane + 64]));
        unsigned long long b0 = __ballot(lane < cnt && mv0 == v), b1 = __ballot(lane + 64 < cnt && mv1 == v);
        if (policy == 1) {                                     // the first optimal move alone
            b1 = b0 ? 0ull : b1 & (0ull - b1);
            b0 &= 0ull - b0;
        }
        if (lane < XQ_BS / 16) row = ((const uint4 *)L.board)[lane];
        if (lane == 5) {                // bytes 80..95: board[80..89], side, z, n_moves, late_temp = 0, ply = 0
            const int z = v > 0 ? 1 : (v < 0 ? -1 : 0);
            row.z = (row.z & 0xFFFFu) | ((uint32_t)(pos.side & 0xFF) << 16) | ((uint32_t)(z & 0xFF) << 24);
            row.w = (uint32_t)cnt;
        } else if (lane == 6) {         // bytes 96..111: reserved0, reserved1, slot = 0, game_seq, pad
            row.z = (uint32_t)e;
        } else if (lane >= 8 && lane < 24) {    // eight entries of actions[]
            const int e0 = (lane - 8) * 8;
            uint32_t w[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int a = e0 + 2 * k;
                w[k] = (a < cnt ? (uint32_t)L.moves[a] : 0u) | ((a + 1 < cnt ? (uint32_t)L.moves[a + 1] : 0u) << 16);
            }
            row = make_uint4(w[0], w[1], w[2], w[3]);
        } else if (lane >= 24) {        // eight entries of visits[]: bits e0 .. e0 + 7 of the optimal moves
            const int e0 = (lane - 24) * 8;
            const uint32_t bits = (uint32_t)((e0 < 64 ? b0 >> e0 : b1 >> (e0 - 64)) & 0xFFull);
            uint32_t w[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) w[k] = ((bits >> (2 * k)) & 1u) | (((bits >> (2 * k + 1)) & 1u) << 16);
            row = make_uint4(w[0], w[1], w[2], w[3]);
        }
    }
    if (lane < ROW_CHUNKS) samples[(size_t)i * ROW_CHUNKS + lane] = row;
    if (lane == 0) status[i] = (uint8_t)st;
}

// fn(first entry, entries) over chunks of the table, so that no grid passes 2^31 threads (64 per entry)
template <class F>
inline void for_entry_chunks(int entries, F fn) {
    constexpr int CHUNK = 1 << 24;
    for (int base = 0; base < entries; base += CHUNK) fn(base, entries - base < CHUNK ? entries - base : CHUNK);
}

}  // namespace

extern "C" {

int64_t xq_tb_entries(const int8_t *pieces, int n_pieces) {
    TbSig S;
    return (int64_t)make_sig(pieces, n_pieces, S);
}

int xq_tb_init(const int8_t *pieces, int n_pieces, int16_t *dev_table, void *stream) {
    TbSig S;
    if (make_sig(pieces, n_pieces, S) == 0 || !dev_table) return XQ_ERR_ARG;
    for_entry_chunks(S.entries, [&](int base, int m) {
        hipLaunchKernelGGL(k_tb_init, dim3((m + WPW - 1) / WPW), dim3(64 * WPW), 0, (hipStream_t)stream, S, dev_table, base, m);
    });
    return launch_status();
}

int xq_tb_pass(const int8_t *pieces, int n_pieces, int16_t *dev_table, int k, int32_t *dev_changed, void *stream) {
    TbSig S;
    if (make_sig(pieces, n_pieces, S) == 0 || !dev_table || !dev_changed || k < 1 || k > XQ_TB_MAX_PASSES) return XQ_ERR_ARG;
    for_entry_chunks(S.entries, [&](int base, int m) {
        hipLaunchKernelGGL(k_tb_pass, dim3((m + WPW - 1) / WPW), dim3(64 * WPW), 0, (hipStream_t)stream, S, dev_table, base, m, k,
                           dev_changed);
    });
    return launch_status();
}

int xq_tb_probe_batch(const int8_t *pieces, int n_pieces, const int16_t *dev_table, const int8_t *dev_boards, const int8_t *dev_side,
                      int n, int16_t *dev_value, uint16_t *dev_moves, uint16_t *dev_counts, int16_t *dev_move_value,
                      uint16_t *dev_best_action, uint8_t *dev_status, void *stream) {
    TbSig S;
    if (n < 0 || make_sig(pieces, n_pieces, S) == 0) return XQ_ERR_ARG;
    if (n > 0 && (!dev_table || !dev_boards || !dev_side || !dev_value || !dev_moves || !dev_counts || !dev_best_action || !dev_status))
        return XQ_ERR_ARG;
    if (n == 0) return XQ_OK;
    for_position_chunks(n, [&](size_t o, int m) {
        hipLaunchKernelGGL(k_tb_probe, dim3((m + WPW - 1) / WPW), dim3(64 * WPW), 0, (hipStream_t)stream, S, dev_table, dev_boards + o * 90,
                           dev_side + o, m, dev_value + o, dev_moves + o * XQ_MAXM, dev_counts + o,
                           dev_move_value ? dev_move_value + o * XQ_MAXM : nullptr, dev_best_action + o, dev_status + o);
    });
    return launch_status();
}

int xq_tb_play_batch(const int8_t *pieces, int n_pieces, const int16_t *dev_table, const int8_t *dev_boards, const int8_t *dev_side,
                     const uint16_t *dev_action, int n, int8_t *dev_boards_out, int8_t *dev_side_out, uint16_t *dev_played,
                     int16_t *dev_value, int16_t *dev_move_value, int16_t *dev_value_out, uint8_t *dev_status, void *stream) {
    TbSig S;
    if (n < 0 || make_sig(pieces, n_pieces, S) == 0) return XQ_ERR_ARG;
    if (n > 0 && (!dev_table || !dev_boards || !dev_side || !dev_boards_out || !dev_side_out || !dev_played || !dev_value ||
                  !dev_move_value || !dev_value_out || !dev_status))
        return XQ_ERR_ARG;
    if (n == 0) return XQ_OK;
    for_position_chunks(n, [&](size_t o, int m) {
        hipLaunchKernelGGL(k_tb_play, dim3((m + WPW - 1) / WPW), dim3(64 * WPW), 0, (hipStream_t)stream, S, dev_table, dev_boards + o * 90,
                           dev_side + o, dev_action ? dev_action + o : nullptr, m, dev_boards_out + o * 90, dev_side_out + o,
                           dev_played + o, dev_value + o, dev_move_value + o, dev_value_out + o, dev_status + o);
    });
    return launch_status();
}

int xq_tb_samples(const int8_t *pieces, int n_pieces, const int16_t *dev_table, const int32_t *dev_index, int n,
                  const xq_tb_sample_opts *opts, void *dev_samples, uint8_t *dev_status, void *stream) {
    TbSig S;
    if (n < 0 || make_sig(pieces, n_pieces, S) == 0 || !opts || (opts->policy != 0 && opts->policy != 1) || opts->reserved[0] != 0 ||
        opts->reserved[1] != 0 || opts->reserved[2] != 0)
        return XQ_ERR_ARG;
    if (n > 0 && (!dev_table || !dev_index || !dev_samples || !dev_status || ((uintptr_t)dev_samples & 15u) != 0)) return XQ_ERR_ARG;
    if (n == 0) return XQ_OK;
    for_position_chunks(n, [&](size_t o, int m) {
        hipLaunchKernelGGL(k_tb_samples, dim3((m + WPW - 1) / WPW), dim3(64 * WPW), 0, (hipStream_t)stream, S, dev_table, dev_index + o, m,
                           opts->policy, (uint4 *)dev_samples + o * ROW_CHUNKS, dev_status + o);
    });
    return launch_status();
}

}  // extern "C"
