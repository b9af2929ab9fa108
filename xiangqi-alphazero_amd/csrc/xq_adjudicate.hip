// xq_adjudicate.hip -- table adjudication: a game whose real position an endgame table decides ends there (map: xq_engine.hip;
// the tables: xq_tablebase.hip, the index: xq_tb_index.cuh).
//
// Every real position of a game goes PH_NEWPOS -> slot_root_request -> PH_WAIT_ROOT -> expand_root_finish, and that function ends
// the game when gi[GI_RSTATUS] != 0, with winner gi[GI_RWINNER] and the status as the result's reason.  k_adjudicate, launched
// between the select and the expand kernels, writes those two words for a slot whose real board a table holds: the expand kernel
// that follows finishes the game, its samples get the exact z, and the result carries reason XQ_REASON_TABLE.  No existing kernel's
// arguments or code change -- a kernel of its own for the reason k_start_pool and k_settle are.
//
// THE RULE, wave_adjudicate, one device function for both kernels.  The board (96 LDS bytes, padding zero) is matched against the
// signature (tb_match).  "Not in this table" with opts.both_colours: the colour-swapped image board'[i] = -board[89 - i] with the
// other side to move is written to the same LDS bytes from registers and matched again -- one table for "Ra" also serves K+A
// against K+R; an entry's value is from the view of the side to move, which the swap keeps.  With a match the int16 word is
// loaded: XQ_TB_INVALID is "not covered", 0 a draw that is adjudicated only under opts.draws, v > 0 a win of the real side to
// move, v < 0 its loss.  Status: 0 decided, +1 not in the table under either colouring, +2 a king is missing, +4 an invalid entry,
// +8 a drawn entry with draws off, +16 (informational, beside 0 or 8) matched through the swapped image.
//
//   k_tb_adjudicate  the stateless batch call, one wave per position, four per workgroup; every output word is written;
//   k_adjudicate     the engine stage, one wave per slot, four per workgroup.  A wave exits after its first loads unless the slot
//                    waits for its root's evaluation, the rules have not ended the game (status 0: wave_game_over's verdict, the
//                    max_game_length adjudication and an earlier table's come first) and the game has min_ply plies.  Lane 0 alone
//                    stores: the two words, and the slot's own counter row.  E.req is not touched: the root's row is still
//                    evaluated, because expand_root_finish reads value[slot] for the resign rule before it looks at the status.
// No scratch, no atomics, no workgroup barrier.
//
// Counters: caller-owned uint64[n_games][4], row s written by slot s's wave only -- [0] games ended decisive, [1] games ended drawn,
// [2] covered but left alone (a drawn entry with draws off), [3] matched through the swapped colours.
#include "xq_engine_state.cuh"
#include "xq_tools.cuh"
#include "xq_tb_index.cuh"

namespace {

struct AdjVerdict {
    int status, value, winner;             // wave-uniform
};

__device__ __forceinline__ AdjVerdict wave_adjudicate(const TbSig &S, const int16_t *__restrict__ table, int8_t *board, int side_in,
                                                      const xq_adjudicate_opts &o) {
    const int lane = lane_id();
    const int side = side_in == 1 ? 1 : -1;
    TbPos pos;
    int e;
    int st = tb_match(S, board, side, pos, e);
    int swapped = 0;
    if ((st & 1) && o.both_colours) {
        // the image from registers: square i takes -board[89 - i]; lanes 0..63 own squares 0..63, lanes 0..25 also 64..89
        const int a = -(int)board[89 - lane];
        const int b = lane < 26 ? -(int)board[lane < 26 ? 25 - lane : 0] : 0;      // the index stays inside for every lane
        wave_sync();
        board[lane] = (int8_t)a;
        if (lane < 32) board[lane + 64] = (int8_t)b;           // bytes 90..95 stay zero
        wave_sync();
        TbPos pos2;
        int e2;
        const int st2 = tb_match(S, board, -side, pos2, e2);
        if (!(st2 & 1)) { st = st2; e = e2; swapped = st2 == 0; }
    }
    AdjVerdict r{st, 0, 0};
    if (st == 0 && (unsigned)e >= (unsigned)S.entries) r.status = st = 1;      // never expected (tb_match): keeps the load inside
    if (st == 0) {
        const int v = __builtin_amdgcn_readfirstlane((int)table[e]);
        if (v == XQ_TB_INVALID) {
            r.status = 4;
        } else {
            r.value = v;
            r.status = (v == 0 && !o.draws) ? 8 : 0;
            if (r.status == 0) r.winner = v > 0 ? side : (v < 0 ? -side : 0);
            if (swapped) r.status |= 16;
        }
    }
    return r;
}

__global__ __launch_bounds__(64 * WPW) void k_tb_adjudicate(TbSig S, const int16_t *__restrict__ table, const int8_t *__restrict__ boards,
                                                             const int8_t *__restrict__ side, int n, xq_adjudicate_opts o,
                                                             uint8_t *__restrict__ status, int8_t *__restrict__ winner,
                                                             int16_t *__restrict__ value) {
    __shared__ __attribute__((aligned(16))) int8_t Ls[WPW][XQ_BS];
    XQ_WAVE_ITEM(n)
    wave_load_board(boards + (size_t)i * 90, Ls[wv]);
    const int sd = __builtin_amdgcn_readfirstlane((int)side[i]);
    wave_sync();
    const AdjVerdict r = wave_adjudicate(S, table, Ls[wv], sd, o);
    if (lane_id() == 0) {
        status[i] = (uint8_t)r.status;
        winner[i] = (int8_t)r.winner;
        value[i] = (int16_t)r.value;
    }
}

__global__ __launch_bounds__(64 * WPW) void k_adjudicate(Dev E, TbSig S, const int16_t *__restrict__ table, xq_adjudicate_opts o,
                                                          unsigned long long *__restrict__ counters) {
    __shared__ __attribute__((aligned(16))) int8_t Ls[WPW][XQ_BS];
    const int wv = (int)(threadIdx.x >> 6);
    const int slot = blockIdx.x * WPW + wv;
    if (slot >= E.cfg.n_games) return;
    int32_t *gi = E.gi + (size_t)slot * GI_N;
    if (__builtin_amdgcn_readfirstlane(gi[GI_PHASE]) != PH_WAIT_ROOT) return;
    if (__builtin_amdgcn_readfirstlane(gi[GI_RSTATUS]) != 0) return;           // the rules' verdict, or an earlier table's
    if (__builtin_amdgcn_readfirstlane(gi[GI_MC]) < o.min_ply) return;
    const int side = __builtin_amdgcn_readfirstlane(gi[GI_SIDE]);
    const int lane = lane_id();
    if (lane < XQ_BS / 4) {                                    // the real board, its padding zeroed whatever the workspace holds
        const uint32_t w = ((const uint32_t *)(E.board + (size_t)slot * XQ_BS))[lane];
        ((uint32_t *)Ls[wv])[lane] = lane < 22 ? w : (lane == 22 ? w & 0xFFFFu : 0u);
    }
    wave_sync();
    const AdjVerdict r = wave_adjudicate(S, table, Ls[wv], side, o);
    if (lane == 0) {
        unsigned long long *c = counters + (size_t)slot * 4;
        const int base = r.status & ~16;
        if (base == 0) {
            gi[GI_RSTATUS] = XQ_REASON_TABLE;
            gi[GI_RWINNER] = r.winner;
            c[r.winner != 0 ? 0 : 1] += 1ull;
        } else if (base == 8) {
            c[2] += 1ull;
        }
        if (r.status & 16) c[3] += 1ull;
    }
}

bool opts_ok(const xq_adjudicate_opts *o) {
    return o && o->reserved == 0 && o->min_ply >= 0 && (o->draws == 0 || o->draws == 1) && (o->both_colours == 0 || o->both_colours == 1);
}

}  // namespace

extern "C" {

int xq_tb_adjudicate_batch(const int8_t *pieces, int n_pieces, const int16_t *dev_table, int64_t entries, const int8_t *dev_boards,
                           const int8_t *dev_side, int n, const xq_adjudicate_opts *opts, uint8_t *dev_status, int8_t *dev_winner,
                           int16_t *dev_value, void *stream) {
    TbSig S;
    if (n < 0 || !opts_ok(opts) || make_sig(pieces, n_pieces, S) == 0 || entries != (int64_t)S.entries) return XQ_ERR_ARG;
    if (n > 0 && (!dev_table || !dev_boards || !dev_side || !dev_status || !dev_winner || !dev_value)) return XQ_ERR_ARG;
    if (n == 0) return XQ_OK;
    const xq_adjudicate_opts o = *opts;
    for_position_chunks(n, [&](size_t off, int m) {
        hipLaunchKernelGGL(k_tb_adjudicate, dim3((m + WPW - 1) / WPW), dim3(64 * WPW), 0, (hipStream_t)stream, S, dev_table,
                           dev_boards + off * 90, dev_side + off, m, o, dev_status + off, dev_winner + off, dev_value + off);
    });
    return launch_status();
}

int xq_engine_adjudicate(const xq_engine *eng, const int8_t *pieces, int n_pieces, const int16_t *dev_table, int64_t entries,
                         const xq_adjudicate_opts *opts, unsigned long long *dev_counters, void *stream) {
    TbSig S;
    if (!eng || !dev_table || !dev_counters || !opts_ok(opts)) return XQ_ERR_ARG;
    if (make_sig(pieces, n_pieces, S) == 0 || entries != (int64_t)S.entries) return XQ_ERR_ARG;
    if (eng->cfg.manual_moves != 0 && eng->cfg.manual_moves != 2) return XQ_ERR_ARG;   // 1: the caller asked for a search
    if (eng->cfg.n_games <= 0 || !eng->p[P_GI] || !eng->p[P_BOARD]) return XQ_ERR_ARG;
    hipLaunchKernelGGL(k_adjudicate, dim3((eng->cfg.n_games + WPW - 1) / WPW), dim3(64 * WPW), 0, (hipStream_t)stream, make_dev(eng), S,
                       dev_table, *opts, dev_counters);
    return launch_status();
}

}  // extern "C"
