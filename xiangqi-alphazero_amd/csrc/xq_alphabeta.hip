// xq_alphabeta.hip -- the fixed, non-learning opponent (include/xq_hip.h, xq_alphabeta_batch): a batched fixed-depth minimax search
// with alpha-beta pruning over the material evaluation.  Three launches on one stream, the search per root move of xq_tools.cuh:
//   k_ab_root    the root moves, and every per-move output's default value;
//   k_ab_search  root move j is searched on its own under a full window, fail-soft alpha-beta in move order below it: its score
//                is the plain minimax value;
//   k_ab_pick    one wavefront per position: the largest score and the draw-th of the moves that reach it.
// The search keeps an explicit stack of at most XQ_AB_MAX_DEPTH - 1 levels in LDS: a board and a move list per level (boards are
// copied per ply, never unmade), five state words per level.  Level l holds the position l + 1 plies below the root.  The last
// level that generates moves scores all its children at once, a lane per move: a leaf's value is the material balance, which a
// move changes by the captured piece's value only, so no leaf board is ever built.  No recursion, no atomics, no scratch.
#include "xq_tools.cuh"

#pragma clang fp contract(off)

using namespace xq;

namespace {

constexpr int AB_LEVELS = XQ_AB_MAX_DEPTH - 1;      // levels that generate moves below a root move
constexpr int AB_INF = 1 << 30;
// every level's node is entered once and revisited once per child and once to leave: a bound no search reaches
constexpr int AB_MAX_ITERS = 2 * (1 + XQ_MAXM + XQ_MAXM * XQ_MAXM) + 2 * (1 + XQ_MAXM) * (XQ_MAXM + 1);

struct AbLevel {
    int cnt, idx, best, alpha, beta;
};

struct AbLds {
    __attribute__((aligned(16))) int8_t board[AB_LEVELS][XQ_BS];
    MoveGenLds mg;
    uint16_t moves[AB_LEVELS][XQ_MAXM];
    AbLevel st[AB_LEVELS];
};

// wave_material's piece values (game.py:552-563); the king counts 0
__device__ __forceinline__ int piece_value(int p) {
    const int a = p < 0 ? -p : p;
    return (a == 2 || a == 3) ? 20 : (a == 4) ? 40 : (a == 5) ? 90 : (a == 6) ? 45 : (a == 7) ? 10 : 0;
}

// The material balance from `side`'s view after its best capture: max over the `cnt` moves of the captured piece's value, added to
// the balance before the move.  This is max over the moves of -V(child, 0, .) of the header's rule.
__device__ __forceinline__ int wave_frontier(const int8_t *b, int side, const uint16_t *moves, int cnt) {
    const int lane = lane_id();
    int red, black;
    wave_material(b, red, black);
    int gain = 0;
    for (int base = 0; base < cnt; base += 64) {
        const int m = base + lane;
        if (m < cnt) {
            const int v = piece_value(b[(int)moves[m] % 90]);
            gain = v > gain ? v : gain;
        }
    }
    return side * (red - black) + wave_max(gain);
}

// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64 * WPW) void k_ab_root(const int8_t *__restrict__ boards, const int8_t *__restrict__ side, int n,
                                                      uint16_t *__restrict__ moves, uint16_t *__restrict__ counts,
                                                      int32_t *__restrict__ scores, uint32_t *__restrict__ nodes,
                                                      uint8_t *__restrict__ status) {
    __shared__ RootLds Ls[WPW];
    XQ_WAVE_ITEM(n)
    wave_root_moves(boards, side, i, Ls[wv], moves, counts, status, [&](size_t o, bool live) {
        scores[o] = live ? 0 : XQ_AB_UNSCORED;      // depth 0 searches nothing
        if (nodes) nodes[o] = 0u;
    });
}

__global__ __launch_bounds__(64 * WPW) void k_ab_search(const int8_t *__restrict__ boards, const int8_t *__restrict__ side, int n,
                                                        int depth, const uint16_t *__restrict__ moves,
                                                        const uint16_t *__restrict__ counts, int32_t *__restrict__ scores,
                                                        uint32_t *__restrict__ nodes, uint8_t *__restrict__ status) {
    __shared__ AbLds Ls[WPW];
    XQ_WAVE_ROOT_MOVE(n, side, moves, counts)
    AbLds &L = Ls[wv];

    wave_load_board(boards + (size_t)i * 90, L.board[0]);
    wave_sync();
    int score, visited = 1, ovf = 0;
    if (depth == 1) {
        // the child is a leaf: the root's balance plus what the move captures
        int red, black;
        wave_material(L.board[0], red, black);
        score = root_side * (red - black) + piece_value(L.board[0][to]);
    } else {
        wave_play(L.board[0], L.board[0], from, to);
        if (lane == 0) { L.st[0].alpha = -AB_INF; L.st[0].beta = AB_INF; }
        wave_sync();
        const int last = depth - 2;                              // the level whose children are leaves; last < AB_LEVELS
        int l = 0, ret = 0;
        bool enter = true;
        visited = 0;
        int it = 0;
        for (; it < AB_MAX_ITERS; ++it) {
            bool leave = false;
            const int sd = (l & 1) ? root_side : -root_side;     // the side to move at level l
            if (enter) {
                ++visited;
                const int cnt = wave_movegen(L.board[l], sd, L.mg, L.moves[l], &ovf);      // cnt <= XQ_MAXM
                if (cnt == 0) {
                    ret = -(XQ_AB_MATE - (l + 1));
                    leave = true;
                } else if (l == last) {
                    ret = wave_frontier(L.board[l], sd, L.moves[l], cnt);
                    visited += cnt;
                    leave = true;
                } else {
                    if (lane == 0) { L.st[l].cnt = cnt; L.st[l].idx = 0; L.st[l].best = -AB_INF; }
                    wave_sync();
                    enter = false;
                }
            } else {
                const int cnt = ld_uniform(&L.st[l].cnt), idx = ld_uniform(&L.st[l].idx), best = ld_uniform(&L.st[l].best);
                const int alpha = ld_uniform(&L.st[l].alpha), beta = ld_uniform(&L.st[l].beta);
                if (idx >= cnt || best >= beta) {
                    ret = best;
                    leave = true;
                } else {
                    // l < last <= AB_LEVELS - 1: level l + 1 exists
                    const int a = __builtin_amdgcn_readfirstlane((int)L.moves[l][idx]);
                    wave_child_board(L.board[l + 1], L.board[l], a);
                    if (lane == 0) {
                        L.st[l + 1].alpha = -beta;
                        L.st[l + 1].beta = -(alpha > best ? alpha : best);
                    }
                    wave_sync();
                    ++l;
                    enter = true;
                }
            }
            if (leave) {
                if (l == 0) break;
                --l;
                const int v = -ret;
                if (lane == 0) {
                    const int best = L.st[l].best;
                    L.st[l].best = v > best ? v : best;
                    L.st[l].idx = L.st[l].idx + 1;
                }
                wave_sync();
                enter = false;
            }
        }
        if (it >= AB_MAX_ITERS) ovf |= 1;
        score = -ret;
    }
    if (lane == 0) {
        const size_t o = (size_t)i * XQ_MAXM + j;
        scores[o] = score;
        if (nodes) nodes[o] = (uint32_t)visited;
        if (ovf) status[i] = (uint8_t)1;      // k_ab_root wrote 0 or 1; every wave that writes here writes the same 1
    }
}

__global__ __launch_bounds__(64 * WPW) void k_ab_pick(int n, const uint32_t *__restrict__ draws, const uint16_t *__restrict__ moves,
                                                      const uint16_t *__restrict__ counts, const int32_t *__restrict__ scores,
                                                      const uint8_t *__restrict__ status, uint16_t *__restrict__ best_action,
                                                      int32_t *__restrict__ best_score) {
    XQ_WAVE_ITEM(n)
    const int lane = lane_id();
    const int cnt = __builtin_amdgcn_readfirstlane((int)counts[i]);       // <= XQ_MAXM
    if (cnt == 0) {
        if (lane == 0) {
            best_action[i] = (uint16_t)XQ_AB_NO_MOVE;
            best_score[i] = status[i] == 2 ? 0 : -XQ_AB_MATE;
        }
        return;
    }
    const int32_t *s = scores + (size_t)i * XQ_MAXM;
    const int s0 = lane < cnt ? s[lane] : INT32_MIN;
    const int s1 = lane + 64 < cnt ? s[lane + 64] : INT32_MIN;
    const int best = wave_max(s0 > s1 ? s0 : s1);
    const bool t0 = lane < cnt && s0 == best, t1 = lane + 64 < cnt && s1 == best;
    const unsigned long long m0 = __ballot(t0), m1 = __ballot(t1);
    const int n0 = __popcll(m0), ties = n0 + __popcll(m1);                // ties >= 1
    const int k = draws ? (int)(draws[i] % (uint32_t)ties) : 0;
    const uint16_t *mv = moves + (size_t)i * XQ_MAXM;
    if (t0 && lane_prefix(m0) == k) { best_action[i] = mv[lane]; best_score[i] = best; }
    if (t1 && n0 + lane_prefix(m1) == k) { best_action[i] = mv[lane + 64]; best_score[i] = best; }
}

}  // namespace

extern "C" {

int xq_alphabeta_batch(const int8_t *dev_boards, const int8_t *dev_side, int n, int depth, const uint32_t *dev_draws,
                       uint16_t *dev_moves, uint16_t *dev_counts, int32_t *dev_scores, uint32_t *dev_nodes,
                       uint16_t *dev_best_action, int32_t *dev_best_score, uint8_t *dev_status, void *stream) {
    if (n < 0 || depth < 0 || depth > XQ_AB_MAX_DEPTH) return XQ_ERR_ARG;
    if (n > 0 && (!dev_boards || !dev_side || !dev_moves || !dev_counts || !dev_scores || !dev_best_action || !dev_best_score ||
                  !dev_status))
        return XQ_ERR_ARG;
    if (n == 0) return XQ_OK;
    for_position_chunks(n, [&](size_t o, int m) {
        const size_t om = o * XQ_MAXM;
        const dim3 per_pos((m + WPW - 1) / WPW), block(64 * WPW);
        hipLaunchKernelGGL(k_ab_root, per_pos, block, 0, (hipStream_t)stream, dev_boards + o * 90, dev_side + o, m, dev_moves + om,
                           dev_counts + o, dev_scores + om, dev_nodes ? dev_nodes + om : nullptr, dev_status + o);
        if (depth >= 1)
            hipLaunchKernelGGL(k_ab_search, dim3((unsigned)m * (XQ_MAXM / WPW)), block, 0, (hipStream_t)stream, dev_boards + o * 90,
                               dev_side + o, m, depth, dev_moves + om, dev_counts + o, dev_scores + om,
                               dev_nodes ? dev_nodes + om : nullptr, dev_status + o);
        hipLaunchKernelGGL(k_ab_pick, per_pos, block, 0, (hipStream_t)stream, m, dev_draws ? dev_draws + o : nullptr, dev_moves + om,
                           dev_counts + o, dev_scores + om, dev_status + o, dev_best_action + o, dev_best_score + o);
    });
    return launch_status();
}

}  // extern "C"
