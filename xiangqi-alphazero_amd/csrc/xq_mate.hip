// xq_mate.hip -- the forced-mate search (include/xq_hip.h, xq_mate_search_batch): does the side to move force mate within N of its
// own moves, by checks only or by any move?  A boolean AND/OR search in move order, iteratively deepened per root move, with an
// exact visit count and a node limit.  Three launches on one stream, the search per root move of xq_tools.cuh:
//   k_mate_root    the root moves, and every per-move output's default value;
//   k_mate_search  the search below one root move;
//   k_mate_pick    one wavefront per position: the quickest mate, the first move that reaches it, and the +4 of the status.
// The search keeps an explicit stack of 2N - 1 levels in LDS: a board and a move list per level (boards are copied per ply, never
// unmade) and two state words.  Level l holds the position l + 1 plies below the root: even levels are the defender's (AND nodes),
// odd levels the attacker's (OR nodes).  Level, mode, result and the visit counter are wave-uniform.  No recursion, no atomics, no
// scratch.
#include "xq_tools.cuh"

using namespace xq;

namespace {

constexpr int MATE_LEVELS = 2 * XQ_MATE_MAX_MOVES - 1;
// a visit costs one iteration to enter, one per move of its list, one to find the list exhausted and one to return; every
// deepening adds one more: a bound no search under its node limit reaches
constexpr unsigned long long MATE_ITERS_PER_VISIT = XQ_MAXM + 3;

enum Mode { ENTER = 0, NEXT = 1, RETURN = 2 };

struct MateLevel {
    int cnt, idx;
};

struct MateLds {
    __attribute__((aligned(16))) int8_t board[MATE_LEVELS][XQ_BS];
    MoveGenLds mg;
    uint16_t moves[MATE_LEVELS][XQ_MAXM];
    MateLevel st[MATE_LEVELS];
};

// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64 * WPW) void k_mate_root(const int8_t *__restrict__ boards, const int8_t *__restrict__ side, int n,
                                                        uint16_t *__restrict__ moves, uint16_t *__restrict__ counts,
                                                        uint8_t *__restrict__ mate_in, uint32_t *__restrict__ nodes,
                                                        uint8_t *__restrict__ status) {
    __shared__ RootLds Ls[WPW];
    XQ_WAVE_ITEM(n)
    wave_root_moves(boards, side, i, Ls[wv], moves, counts, status, [&](size_t o, bool) {
        mate_in[o] = (uint8_t)0;
        if (nodes) nodes[o] = 0u;
    });
}

__global__ __launch_bounds__(64 * WPW) void k_mate_search(const int8_t *__restrict__ boards, const int8_t *__restrict__ side, int n,
                                                          int max_moves, int checks_only, uint32_t node_limit,
                                                          const uint16_t *__restrict__ moves, const uint16_t *__restrict__ counts,
                                                          uint8_t *__restrict__ mate_in, uint32_t *__restrict__ nodes,
                                                          uint8_t *__restrict__ status) {
    __shared__ MateLds Ls[WPW];
    XQ_WAVE_ROOT_MOVE(n, side, moves, counts)
    MateLds &L = Ls[wv];
    const int attacker = root_side;
    wave_load_board(boards + (size_t)i * 90, L.board[0]);
    wave_sync();
    wave_play(L.board[0], L.board[0], from, to);
    wave_sync();

    int result = 0, ovf = 0;
    uint32_t visited = 0;
    if (!checks_only || wave_in_check(L.board[0], -attacker)) {
        // D(child, m - 1) for m = 1 .. max_moves; level 0's board is the child and is never written again
        const unsigned long long cap = (unsigned long long)node_limit * MATE_ITERS_PER_VISIT + XQ_MATE_MAX_MOVES;
        int m = 1, l = 0, ret = 0, mode = ENTER;
        bool done = false;
        for (unsigned long long it = 0; it < cap; ++it) {
            const int or_node = l & 1;                            // the attacker is to move at odd levels
            if (mode == ENTER) {
                if (visited >= node_limit) { result = XQ_MATE_UNKNOWN; done = true; break; }
                ++visited;
                const int cnt = wave_movegen(L.board[l], or_node ? attacker : -attacker, L.mg, L.moves[l], &ovf);   // <= XQ_MAXM
                if (!or_node && cnt == 0) {
                    ret = 1;
                    mode = RETURN;
                } else if (!or_node && m - 1 - (l >> 1) == 0) {   // the attacker has no move left
                    ret = 0;
                    mode = RETURN;
                } else {
                    if (lane == 0) { L.st[l].cnt = cnt; L.st[l].idx = 0; }
                    wave_sync();
                    mode = NEXT;
                }
            } else if (mode == NEXT) {
                const int cnt = ld_uniform(&L.st[l].cnt), idx = ld_uniform(&L.st[l].idx);
                if (idx >= cnt) {
                    ret = or_node ^ 1;                            // no reply escaped: mated; no attacking move worked: not forced
                    mode = RETURN;
                } else if (l + 1 >= MATE_LEVELS) {                // unreachable: a defender's level with no move left returns above
                    ovf |= 1;
                    break;
                } else {
                    const int a = __builtin_amdgcn_readfirstlane((int)L.moves[l][idx]);
                    wave_child_board(L.board[l + 1], L.board[l], a);
                    wave_sync();
                    if (or_node && checks_only && !wave_in_check(L.board[l + 1], -attacker)) {
                        if (lane == 0) L.st[l].idx = idx + 1;     // a move that gives no check: skipped, no visit
                        wave_sync();
                    } else {
                        ++l;
                        mode = ENTER;
                    }
                }
            } else {
                // level l has returned `ret`
                if (l == 0) {
                    if (ret) { result = m; done = true; break; }
                    if (m >= max_moves) { result = 0; done = true; break; }
                    ++m;
                    mode = ENTER;
                } else {
                    --l;
                    // an AND node ends on the first false, an OR node on the first true: level l returns the same value
                    if (ret != (l & 1)) {
                        if (lane == 0) L.st[l].idx = L.st[l].idx + 1;
                        wave_sync();
                        mode = NEXT;
                    }
                }
            }
        }
        if (!done) { ovf |= 1; result = XQ_MATE_UNKNOWN; }
    }
    if (lane == 0) {
        const size_t o = (size_t)i * XQ_MAXM + j;
        mate_in[o] = (uint8_t)result;
        if (nodes) nodes[o] = visited;
        if (ovf) status[i] = (uint8_t)1;      // k_mate_root wrote 0 or 1; every wave that writes here writes the same 1
    }
}

__global__ __launch_bounds__(64 * WPW) void k_mate_pick(int n, int max_moves, const uint16_t *__restrict__ moves,
                                                        const uint16_t *__restrict__ counts, const uint8_t *__restrict__ mate_in,
                                                        uint16_t *__restrict__ best_action, uint8_t *__restrict__ best_mate_in,
                                                        uint8_t *__restrict__ status) {
    XQ_WAVE_ITEM(n)
    const int lane = lane_id();
    const int cnt = __builtin_amdgcn_readfirstlane((int)counts[i]);       // <= XQ_MAXM
    const uint8_t *mi = mate_in + (size_t)i * XQ_MAXM;
    const int none = XQ_MATE_UNKNOWN + 1;
    const int r0 = lane < cnt ? (int)mi[lane] : 0, r1 = lane + 64 < cnt ? (int)mi[lane + 64] : 0;
    const int v0 = (r0 >= 1 && r0 <= max_moves) ? r0 : none, v1 = (r1 >= 1 && r1 <= max_moves) ? r1 : none;
    const int best = wave_min(v0 < v1 ? v0 : v1);
    const bool cut = __ballot(r0 == XQ_MATE_UNKNOWN || r1 == XQ_MATE_UNKNOWN) != 0ull;
    const unsigned long long m0 = __ballot(v0 == best), m1 = __ballot(v1 == best);
    if (lane == 0) {
        int act = XQ_MATE_NO_MOVE;
        if (best != none) {
            const int j = m0 ? __ffsll((long long)m0) - 1 : 64 + __ffsll((long long)m1) - 1;      // < cnt
            act = (int)moves[(size_t)i * XQ_MAXM + j];
        }
        best_action[i] = (uint16_t)act;
        best_mate_in[i] = (uint8_t)(best != none ? best : 0);
        if (cut) status[i] = (uint8_t)(status[i] | 4);
    }
}

}  // namespace

extern "C" {

int xq_mate_search_batch(const int8_t *dev_boards, const int8_t *dev_side, int n, const xq_mate_opts *opts, uint16_t *dev_moves,
                         uint16_t *dev_counts, uint8_t *dev_mate_in, uint32_t *dev_nodes, uint16_t *dev_best_action,
                         uint8_t *dev_best_mate_in, uint8_t *dev_status, void *stream) {
    if (n < 0 || !opts) return XQ_ERR_ARG;
    if (opts->max_moves < 1 || opts->max_moves > XQ_MATE_MAX_MOVES || (opts->checks_only != 0 && opts->checks_only != 1) ||
        opts->node_limit == 0 || opts->reserved != 0)
        return XQ_ERR_ARG;
    if (n > 0 && (!dev_boards || !dev_side || !dev_moves || !dev_counts || !dev_mate_in || !dev_best_action || !dev_best_mate_in ||
                  !dev_status))
        return XQ_ERR_ARG;
    if (n == 0) return XQ_OK;
    for_position_chunks(n, [&](size_t o, int m) {
        const size_t om = o * XQ_MAXM;
        const dim3 per_pos((m + WPW - 1) / WPW), block(64 * WPW);
        hipLaunchKernelGGL(k_mate_root, per_pos, block, 0, (hipStream_t)stream, dev_boards + o * 90, dev_side + o, m, dev_moves + om,
                           dev_counts + o, dev_mate_in + om, dev_nodes ? dev_nodes + om : nullptr, dev_status + o);
        hipLaunchKernelGGL(k_mate_search, dim3((unsigned)m * (XQ_MAXM / WPW)), block, 0, (hipStream_t)stream, dev_boards + o * 90,
                           dev_side + o, m, (int)opts->max_moves, (int)opts->checks_only, opts->node_limit, dev_moves + om,
                           dev_counts + o, dev_mate_in + om, dev_nodes ? dev_nodes + om : nullptr, dev_status + o);
        hipLaunchKernelGGL(k_mate_pick, per_pos, block, 0, (hipStream_t)stream, m, (int)opts->max_moves, dev_moves + om,
                           dev_counts + o, dev_mate_in + om, dev_best_action + o, dev_best_mate_in + o, dev_status + o);
    });
    return launch_status();
}

}  // extern "C"
