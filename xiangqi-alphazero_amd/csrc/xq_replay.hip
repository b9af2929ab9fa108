// xq_replay.hip -- batched replay of game records (include/xq_hip.h, xq_replay_games_batch): one 64-lane wavefront per record,
// four records per 256-thread workgroup, LDS carved per wave and no workgroup barrier (xq_rules.cuh).  A record is played from
// the initial position on an LDS board with the 12-board ring the engine's real game keeps: every ply generates the ordered legal
// moves and looks the record's action up among them, so a record replays only if every move of it was legal where it was played.
#include "xq_tools.cuh"

#pragma clang fp contract(off)

using namespace xq;

namespace {

static_assert(sizeof(xq_game_record) == XQ_RECORD_BYTES && offsetof(xq_game_record, moves) == 16, "xq_game_record layout");

struct ReplayLds {
    __attribute__((aligned(16))) int8_t board[XQ_BS];
    __attribute__((aligned(16))) int8_t ring[XQ_HIST][XQ_BS];   // pre-move board of ply p in row p % 12
    MoveGenLds mg;
    uint16_t moves[XQ_MAXM];
};

__global__ __launch_bounds__(64 * WPW) void k_replay_games(const xq_game_record *__restrict__ records, const int32_t *__restrict__ stop_ply,
                                                           int n, int perpetual, int8_t *__restrict__ boards, int8_t *__restrict__ out_side,
                                                           int32_t *__restrict__ out_mc, int32_t *__restrict__ out_nocap,
                                                           int8_t *__restrict__ hist12, int32_t *__restrict__ status,
                                                           int8_t *__restrict__ over_kind, int8_t *__restrict__ out_winner) {
    __shared__ ReplayLds Ls[WPW];
    XQ_WAVE_ITEM(n)
    ReplayLds &L = Ls[wv];
    const int lane = lane_id();
    const xq_game_record *rec = records + i;
    const int n_moves = __builtin_amdgcn_readfirstlane((int)rec->n_moves);
    int stop = stop_ply ? __builtin_amdgcn_readfirstlane(stop_ply[i]) : n_moves;
    stop = stop < 0 ? 0 : (stop > n_moves ? n_moves : stop);
    int st = 0;
    if (n_moves > XQ_RECORD_MAX_PLIES) { st = -1; stop = 0; }    // malformed: moves[] holds no such ply

    init_board_lds(L.board);
    for (int j = lane; j < XQ_HIST * XQ_BS / 4; j += 64) ((uint32_t *)L.ring)[j] = 0u;
    wave_sync();
    int side = 1, mc = 0, nocap = 0, ovf = 0;
    for (int ply = 0; ply < stop; ++ply) {
        const int action = __builtin_amdgcn_readfirstlane((int)rec->moves[ply]);    // ply < stop <= XQ_RECORD_MAX_PLIES
        const int cnt = wave_movegen(L.board, side, L.mg, L.moves, &ovf);           // cnt <= XQ_MAXM
        bool found = false;
        for (int base = 0; base < cnt; base += 64)
            found = found || __ballot(base + lane < cnt && (int)L.moves[base + lane] == action) != 0ull;
        if (!found) { st = ply + 1; break; }
        wave_make_move(L.board, L.ring, action, side, mc, nocap);
    }

    int cnt = 0, winner = 2;
    const int over = wave_game_over(L.board, L.ring, side, mc, nocap, perpetual != 0, L.mg, L.moves, &cnt, &winner, &ovf);
    if (boards)
        for (int sq = lane; sq < 90; sq += 64) boards[(size_t)i * 90 + sq] = L.board[sq];
    if (hist12) {
        // entry e (oldest first) is the pre-move board of ply mc - k + e, k = min(12, mc); the entries behind them are zero
        const int k = mc < XQ_HIST ? mc : XQ_HIST;
        int8_t *h = hist12 + (size_t)i * XQ_HIST * 90;
        for (int j = lane; j < XQ_HIST * 90; j += 64) {
            const int e = j / 90, sq = j - e * 90;
            h[j] = e < k ? L.ring[(mc - k + e) % XQ_HIST][sq] : (int8_t)0;
        }
    }
    if (lane == 0) {
        status[i] = st;
        if (out_side) out_side[i] = (int8_t)side;
        if (out_mc) out_mc[i] = mc;
        if (out_nocap) out_nocap[i] = nocap;
        if (over_kind) over_kind[i] = (int8_t)over;
        if (out_winner) out_winner[i] = (int8_t)winner;
    }
}

}  // namespace

extern "C" {

int xq_replay_games_batch(const void *dev_records, const int32_t *dev_stop_ply, int n, int perpetual_check, int8_t *dev_boards,
                          int8_t *dev_side, int32_t *dev_move_count, int32_t *dev_no_capture, int8_t *dev_hist12, int32_t *dev_status,
                          int8_t *dev_over_kind, int8_t *dev_winner, void *stream) {
    if (n < 0 || (n > 0 && (!dev_records || !dev_status)) || (perpetual_check != 0 && perpetual_check != 1)) return XQ_ERR_ARG;
    if (n == 0) return XQ_OK;
    hipLaunchKernelGGL(k_replay_games, dim3((n + WPW - 1) / WPW), dim3(64 * WPW), 0, (hipStream_t)stream,
                       (const xq_game_record *)dev_records, dev_stop_ply, n, perpetual_check, dev_boards, dev_side, dev_move_count,
                       dev_no_capture, dev_hist12, dev_status, dev_over_kind, dev_winner);
    return launch_status();
}

}  // extern "C"
