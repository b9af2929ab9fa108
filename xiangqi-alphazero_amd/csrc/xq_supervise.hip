// xq_supervise.hip -- game records as training samples (include/xq_hip.h, xq_records_sample_counts / xq_records_to_samples).
// The conversion has xq_replay.hip's shape: one 64-lane wavefront per record, four records per 256-thread workgroup, LDS carved
// per wave and no workgroup barrier (xq_rules.cuh).  A record is played from the initial position; every ply generates the
// ordered legal moves and looks the record's action up among them, and a selected ply leaves one xq_sample: the position, the
// legal moves and one visit at the move played.  Rows are placed by the caller's prefix sum of the counts: no atomics, and the
// same bytes on every run.
#include "xq_tools.cuh"

#pragma clang fp contract(off)

using namespace xq;

namespace {

constexpr int ROW_CHUNKS = XQ_SAMPLE_BYTES / 16;    // a row is 40 16-byte stores, one per lane

static_assert(sizeof(xq_sample) == XQ_SAMPLE_BYTES && XQ_SAMPLE_BYTES % 16 == 0, "xq_sample layout");
static_assert(offsetof(xq_sample, side) == 90 && offsetof(xq_sample, n_moves) == 92 && offsetof(xq_sample, ply) == 94 &&
              offsetof(xq_sample, slot) == 100 && offsetof(xq_sample, game_seq) == 104 && offsetof(xq_sample, actions) == 128 &&
              offsetof(xq_sample, visits) == 384, "xq_sample layout");
static_assert(sizeof(xq_game_record) == XQ_RECORD_BYTES, "xq_game_record layout");

// What a record selects, from its header alone: plies p with lo <= p < n_moves whose parity bit is set in `parity` (bit 0: red's
// plies, the even ones; bit 1: black's).  One copy for the counts kernel and the conversion.
struct Selection {
    int lo, n_moves, parity, count;
    bool malformed;
};

__device__ __forceinline__ Selection select_plies(int n_moves, int opening, int winner, int movers, int skip_opening, int skip_draws) {
    Selection s;
    s.malformed = n_moves > XQ_RECORD_MAX_PLIES || opening > n_moves || winner < -1 || winner > 1 || movers < 0 || movers > 3;
    s.n_moves = s.malformed ? 0 : n_moves;
    s.lo = s.malformed ? 0 : (skip_opening ? opening : 0);
    int parity = movers == 0 ? 3 : movers == 2 ? 1 : movers == 3 ? 2 : (winner == 1 ? 1 : winner == -1 ? 2 : 0);
    if (s.malformed || (skip_draws && winner == 0)) parity = 0;
    s.parity = parity;
    const int even = (s.n_moves + 1) / 2 - (s.lo + 1) / 2, odd = s.n_moves / 2 - s.lo / 2;
    s.count = ((parity & 1) ? even : 0) + ((parity & 2) ? odd : 0);
    return s;
}

__device__ __forceinline__ bool ply_selected(const Selection &s, int ply) { return ply >= s.lo && ((s.parity >> (ply & 1)) & 1) != 0; }

__global__ __launch_bounds__(256) void k_sample_counts(const xq_game_record *__restrict__ records, const uint8_t *__restrict__ movers_of,
                                                       int n, int movers, int skip_opening, int skip_draws,
                                                       int32_t *__restrict__ counts) {
    const int i = blockIdx.x * 256 + (int)threadIdx.x;
    if (i >= n) return;
    const xq_game_record *rec = records + i;
    const Selection s = select_plies((int)rec->n_moves, (int)rec->opening_plies, (int)rec->winner,
                                     movers_of ? (int)movers_of[i] : movers, skip_opening, skip_draws);
    counts[i] = s.count;
}

struct SuperviseLds {
    __attribute__((aligned(16))) int8_t board[XQ_BS];          // bytes 90..95 stay zero: the row's first 96 bytes start from here
    __attribute__((aligned(16))) int8_t ring[XQ_HIST][XQ_BS];  // wave_make_move keeps it; the conversion judges no repetition
    MoveGenLds mg;
    __attribute__((aligned(16))) uint16_t moves[XQ_MAXM];
};

__global__ __launch_bounds__(64 * WPW) void k_records_to_samples(const xq_game_record *__restrict__ records,
                                                                 const uint8_t *__restrict__ movers_of,
                                                                 const int32_t *__restrict__ offsets, int n, int movers,
                                                                 int skip_opening, int skip_draws, uint4 *__restrict__ samples,
                                                                 int32_t *__restrict__ status) {
    __shared__ SuperviseLds Ls[WPW];
    XQ_WAVE_ITEM(n)
    SuperviseLds &L = Ls[wv];
    const int lane = lane_id();
    const xq_game_record *rec = records + i;
    const int winner = __builtin_amdgcn_readfirstlane((int)rec->winner);
    const Selection s = select_plies(__builtin_amdgcn_readfirstlane((int)rec->n_moves),
                                     __builtin_amdgcn_readfirstlane((int)rec->opening_plies), winner,
                                     movers_of ? __builtin_amdgcn_readfirstlane((int)movers_of[i]) : movers, skip_opening, skip_draws);
    const int off = __builtin_amdgcn_readfirstlane(offsets[i]), end = __builtin_amdgcn_readfirstlane(offsets[i + 1]);
    const int total = __builtin_amdgcn_readfirstlane(offsets[n]);
    int st = 0;
    if (s.malformed) st = -1;
    else if (end - off != s.count || off < 0 || end > total) st = -2;    // rows that are not this record's are never written
    if (st != 0) {      // a well-formed record that selects nothing is still replayed for its status
        if (lane == 0) status[i] = st;
        return;
    }
    const uint32_t slot = (uint32_t)__builtin_amdgcn_readfirstlane((int)rec->slot);
    const uint32_t game_seq = (uint32_t)__builtin_amdgcn_readfirstlane((int)rec->game_seq);

    init_board_lds(L.board);
    for (int j = lane; j < XQ_HIST * XQ_BS / 4; j += 64) ((uint32_t *)L.ring)[j] = 0u;
    wave_sync();
    int side = 1, mc = 0, nocap = 0, ovf = 0;
    int row = off, ply = 0;
    for (; ply < s.n_moves; ++ply) {
        const int action = __builtin_amdgcn_readfirstlane((int)rec->moves[ply]);    // ply < n_moves <= XQ_RECORD_MAX_PLIES
        const int cnt = wave_movegen(L.board, side, L.mg, L.moves, &ovf);           // cnt <= XQ_MAXM
        int played = -1;
        for (int base = 0; base < cnt; base += 64) {
            const unsigned long long m = __ballot(base + lane < cnt && (int)L.moves[base + lane] == action);
            if (m != 0ull && played < 0) played = base + (int)__builtin_ctzll(m);
        }
        if (played < 0) { st = ply + 1; break; }
        if (ply_selected(s, ply)) {
            if (lane < ROW_CHUNKS) {
                uint4 v = make_uint4(0u, 0u, 0u, 0u);
                if (lane < XQ_BS / 16) v = ((const uint4 *)L.board)[lane];
                if (lane == 5) {        // bytes 80..95: board[80..89], side, z, n_moves, late_temp = 0, ply
                    const int z = winner == 0 ? 0 : (winner == side ? 1 : -1);
                    v.z = (v.z & 0xFFFFu) | ((uint32_t)(side & 0xFF) << 16) | ((uint32_t)(z & 0xFF) << 24);
                    v.w = (uint32_t)cnt | ((uint32_t)mc << 16);
                } else if (lane == 6) { // bytes 96..111: reserved0, reserved1, slot, game_seq, pad
                    v.y = slot;
                    v.z = game_seq;
                } else if (lane >= 8) { // eight entries of actions[] (lanes 8..23) or visits[] (lanes 24..39)
                    const bool vis = lane >= 24;
                    const int e0 = (lane - (vis ? 24 : 8)) * 8;
                    uint32_t w[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int a = e0 + 2 * k, b = a + 1;
                        const uint32_t lo = vis ? (a == played ? 1u : 0u) : (a < cnt ? (uint32_t)L.moves[a] : 0u);
                        const uint32_t hi = vis ? (b == played ? 1u : 0u) : (b < cnt ? (uint32_t)L.moves[b] : 0u);
                        w[k] = lo | (hi << 16);
                    }
                    v = make_uint4(w[0], w[1], w[2], w[3]);
                }
                samples[(size_t)row * ROW_CHUNKS + lane] = v;
            }
            ++row;
        }
        wave_make_move(L.board, L.ring, action, side, mc, nocap);
    }
    // an illegal ply: the selected plies from it on keep their rows, as zeros
    for (; ply < s.n_moves; ++ply)
        if (ply_selected(s, ply)) {
            if (lane < ROW_CHUNKS) samples[(size_t)row * ROW_CHUNKS + lane] = make_uint4(0u, 0u, 0u, 0u);
            ++row;
        }
    if (lane == 0) status[i] = st;
}

bool bad_opts(const xq_supervise_opts *o) {
    return !o || o->movers < 0 || o->movers > 3 || (o->skip_opening != 0 && o->skip_opening != 1) ||
           (o->skip_draws != 0 && o->skip_draws != 1) || o->reserved != 0;
}

}  // namespace

extern "C" {

int xq_records_sample_counts(const void *dev_records, const uint8_t *dev_movers, int n, const xq_supervise_opts *opts,
                             int32_t *dev_counts, void *stream) {
    if (n < 0 || bad_opts(opts) || (n > 0 && (!dev_records || !dev_counts))) return XQ_ERR_ARG;
    if (n == 0) return XQ_OK;
    hipLaunchKernelGGL(k_sample_counts, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream,
                       (const xq_game_record *)dev_records, dev_movers, n, opts->movers, opts->skip_opening, opts->skip_draws,
                       dev_counts);
    return launch_status();
}

int xq_records_to_samples(const void *dev_records, const uint8_t *dev_movers, const int32_t *dev_offsets, int n,
                          const xq_supervise_opts *opts, void *dev_samples, int32_t *dev_status, void *stream) {
    if (n < 0 || bad_opts(opts) || (n > 0 && (!dev_records || !dev_offsets || !dev_samples || !dev_status)) ||
        ((uintptr_t)dev_samples & 15u) != 0)
        return XQ_ERR_ARG;
    if (n == 0) return XQ_OK;
    hipLaunchKernelGGL(k_records_to_samples, dim3((n + WPW - 1) / WPW), dim3(64 * WPW), 0, (hipStream_t)stream,
                       (const xq_game_record *)dev_records, dev_movers, dev_offsets, n, opts->movers, opts->skip_opening,
                       opts->skip_draws, (uint4 *)dev_samples, dev_status);
    return launch_status();
}

}  // extern "C"
