// xq_engine_state.cuh -- what more than one of the engine's translation units needs (map: xq_engine.hip): the numbering of the
// phases, state words, counters and workspace regions, the device view of the handle, the words behind the square-root table,
// the pad0 encoding, Philox, and the one-workgroup compaction.  Device and host helpers only: every kernel lives in one unit.
//
// include/xq_hip.h pins the handle; tests pin the Gi / St / Ptr numbering and the workspace layout, and
// xiangqi-alphazero_amd/hip.py mirrors the entries Python reads (P_*, GI_*, PH_HOLD).  A change here changes both.
#pragma once

#include <float.h>
#include <math.h>
#include <string.h>

#include "xq_common.h"
#include "xq_rules.cuh"

#pragma clang fp contract(off)

using namespace xq;

namespace xq {

// k_gather_rows over the engine's own packed buffers, for the first `rows` request rows (xq_engine_packed.hip).  The one call
// that crosses units: the evaluation cache's miss compaction gathers as the packed step does.  Not exported.
__attribute__((visibility("hidden"))) int gather_packed_rows(const xq_engine *eng, const float *dev_nn_input, int rows, hipStream_t s);

}  // namespace xq

namespace {

enum Phase : int { PH_NEWGAME = 0, PH_NEWPOS = 1, PH_WAIT_ROOT = 2, PH_SEARCH = 3, PH_WAIT_LEAF = 4, PH_FINISHED = 5,
                   PH_IDLE = 6, PH_HOLD = 7 };

enum Gi : int { GI_SIDE = 0, GI_MC, GI_NOCAP, GI_PHASE, GI_SIMS, GI_NSAMP, GI_GSEQ, GI_ALLOC, GI_PLEAF, GI_PDEPTH,
                GI_PCOUNT, GI_RSTATUS, GI_RWINNER, GI_RESIGN_N, GI_RNG0, GI_RNG1, GI_RNG2, GI_RNG3, GI_FWINNER,
                GI_FREASON, GI_MANNOISE, GI_DELAY, GI_NPEND, GI_RR_NODE, GI_RR_MARK, GI_RR_DROP,
                // playout cap (xq_engine_init_cap): this move's kind (1 full, 0 fast) and budget, written by k_select<.., true> at
                // PH_NEWPOS; S_fast and the two halves of the float64 threshold p, written once by k_init_cap
                GI_CAP_FULL, GI_CAP_BUDGET, GI_CAP_SFAST, GI_CAP_PLO, GI_CAP_PHI,
                // forced playouts (xq_engine_init_fp): k as float32 bits, written once by k_init_fp
                GI_FP_K, GI_N = 32 };
static_assert(GI_FP_K == 31, "the forced-playout parameter takes the last free state word");

enum St : int { ST_SIMS = 0, ST_TERM, ST_LEAF, ST_ROOT, ST_MOVES, ST_GAMES, ST_RED, ST_BLACK, ST_DRAW, ST_PLIES, ST_NODES,
                ST_DEPTH, ST_SCAN, ST_RESIGN, ST_SAMP, ST_DROP, ST_OVF, ST_STARTED, ST_ROWS, ST_COLL, ST_LPS, ST_LSTEPS, ST_REUSED,
                ST_REROOTS, ST_FASTM, ST_FASTS, ST_FORCED, ST_PRUNEDV, ST_PRUNEDC, ST_GZ_MOVES, ST_GZ_CONS, ST_GZ_OFF, ST_N = 32 };
static_assert(ST_GZ_OFF == 31, "the Gumbel counters take the last free statistics words");

enum Ptr : int { P_BOARD = 0, P_HIST, P_GI, P_RESIGN, P_PMOVES, P_PATH, P_TN, P_TW, P_TP, P_TA, P_TC, P_TM, P_ROOTP,
                 P_STAGE, P_OUTS, P_OUTR, P_CNT, P_STATS, P_INJECT, P_SQRT, P_MNOISE, P_STATSUM, P_REQ,
                 P_PK_N, P_PK_ROWS, P_PK_X, P_PK_MOVES, P_PK_COUNTS, P_PK_LOGITS, P_PK_VALUE, P_VL, P_LEAF };

enum Rng : int { RNG_RANDINT = 0, RNG_CHOICE = 1, RNG_DIRICHLET = 2, RNG_UNIFORM = 3 };

// pad0 of an engine handle: leaves per step in the low 16 bits (0 = 1), the XQ_ENGINE_* flags in the public flag byte above them
// (bits 16-23), and one private bit per option that is on.  Bits 24-31 are all taken; of the flag byte bit 16 is public and bits
// 23 and 22 are private: flags_ok lets no caller's flag reach either.
constexpr int PAD0_EVAL_MIRROR = (int)(1u << 31);   // "evaluation mirror on" (xq_engine_init_em): the last private bit, the sign
constexpr int PAD0_CAP = 1 << 30;           // "playout cap on" (xq_engine_init_cap)
constexpr int PAD0_FORCED = 1 << 29;        // "forced playouts on" (xq_engine_init_fp)
constexpr int PAD0_GUMBEL = 1 << 28;        // "Gumbel root search on" (xq_engine_init_gz)
constexpr int PAD0_ARENA = 1 << 27;         // "arena options on" (xq_engine_init_ar)
constexpr int PAD0_PERPETUAL = 1 << 26;     // "perpetual-check rule on" (xq_engine_init_ru)
constexpr int PAD0_SOLVER = 1 << 25;        // "proven-result search on" (xq_engine_init_sv)
constexpr int PAD0_ROOT_STATS = 1 << 24;    // "root statistics per sample on" (xq_engine_init_rs)
constexpr int PAD0_GAME_RECORDS = 1 << 23;  // "game records on" (xq_engine_init_gr): the top bit of the public flag byte
constexpr int PAD0_START_POOL = 1 << 22;    // "start-position pool on" (xq_engine_init_sp): the next bit of that byte

// The node meta word tM: the child count in bits 0-11 (at most XQ_MAXM = 128), the node's proven state in bits 12-13 (always 0
// without xq_engine_init_sv: every reader masks the count, and an engine without the solver stays byte-identical), the prior
// kind in bits 14-15.  States are seen from the side that moved into the node, the view of its W.
constexpr int XQ_CNT_MASK = 0x0FFF;
constexpr int XQ_STATE_SHIFT = 12;
enum NodeState : int { NS_UNKNOWN = 0, NS_WIN = 1, NS_DRAW = 2, NS_LOSS = 3 };
__host__ __device__ inline int node_state(int m) { return (m >> XQ_STATE_SHIFT) & 3; }

// Device view of the engine (passed by value to kernels)
struct Dev {
    xq_engine_config cfg;
    int node_cap, path_cap, stage_cap;
    int8_t *board, *hist;
    int32_t *gi;
    double *resign;
    uint16_t *pmoves;
    int32_t *path;
    int32_t *tN; double *tW; float *tP; uint16_t *tA; int32_t *tC; uint16_t *tM;
    double *rootP;
    uint8_t *stage, *outs, *outr;
    unsigned int *cnt;              // [0] out samples, [1] out results
    unsigned long long *started;    // games started (quota)
    unsigned long long *stats;      // [G][ST_N]
    const uint64_t *inject;
    const double *sqrt_tab;
    double *mnoise;
    int32_t *req;                   // [G] legal moves of the evaluation each slot asked for this step (0: none)
    int perpetual;                  // xq_rules_opts.perpetual_check of xq_engine_init_ru (wave-uniform: a kernel argument)
    int root_stats;                 // xq_root_stats_opts.enabled of xq_engine_init_rs (wave-uniform, like perpetual)
    uint16_t *gr_log;               // xq_engine_init_gr: the move log [G][XQ_RECORD_MAX_PLIES]; NULL without game records (wave-uniform)
};

// ---------------------------------------------------------------------------------------------------------
// THE OPTION WORDS.  The handle, the config struct and the per-slot state words are full, so every option that needs device
// words keeps them in ONE workspace region, the square-root table's (P_SQRT).  This is the one description of that region:
// include/xq_hip.h repeats it for callers (xq_engine_option_words_sp fills it in for an engine's shape), and every reader and
// writer, host or device, takes its addresses from the functions below.  Offsets are bytes from the region's first byte, up()
// rounds up to 256 (align_up); G slots, S simulations, K leaves per step.
//   the front, located from the region's first byte
//     0                  table    double[S + 2 + (K > 1 ? K : 0)]: sqrt(i)                                    every engine
//     (S + 2) * 8        GzHead | v_hat double[G] | visits uint16[m][S], row k - 1 for k considered moves     Gumbel
//     up((S + 2) * 8)    ArHead | op_counts int32[G] | op_actions uint16[G][XQ_ARENA_MAX_OPENING] | n_live int32[2] |
//                        2 x (rows int32[G] | x float[G][XQ_STATE_FLOATS] | moves uint16[G][XQ_MAXM] | counts int32[G]),
//                        every part up(): set 0 the new model's slots, set 1 the old model's                  arena
//     up((S + 2) * 8), or the arena words' end:  counters uint64[G][SV_WORDS]                                 solver
//   the tail, located from the region's end (where P_MNOISE begins); it starts at up(the front's end), every part up()
//     ring xq_game_record[max_out_games] | log uint16[G][XQ_RECORD_MAX_PLIES] | opening uint16[G] | GrHead   records
//     rows int8[n][XQ_BS] (a board, its side in byte 90) | start_index int32[G] | SpHead                      pool, never with records
// Gumbel, arena and solver words start behind a table of S + 2 entries: opts_ok accepts none of them with K > 1, Gumbel with
// neither of the other two, and tests/test_workspace_map.py holds the blocks of every accepted combination disjoint.  m,
// max_out_games and n exist only on the device (in the heads), so they are arguments only where an end is asked for: every start
// follows from cfg, pad0, p[P_SQRT] and p[P_MNOISE].
// Gumbel root search (xq_engine_init_gz): considered moves at most; c_visit, c_scale rounded to float32 once, widened at every use
struct GzHead { int32_t m; float c_visit, c_scale; int32_t pad; };
struct ArHead { int32_t opening_plies, first_game, pad[2]; };       // arena options (xq_engine_init_ar)
// proven-result search (xq_engine_init_sv): per slot proven_nodes, proven_stops, proven_moves, unspent_sims, removed_visits, 3 spare
constexpr int SV_WORDS = 8;
enum Sv : int { SV_NODES = 0, SV_STOPS, SV_MOVES, SV_UNSPENT, SV_REMOVED };
struct GrHead {                     // game records (xq_engine_init_gr)
    int32_t max_out_games;
    unsigned int count;             // games flushed since the last xq_engine_drain_games: the ring's cursor
    unsigned long long recorded, dropped, pad[29];
};
struct SpHead {                     // start-position pool (xq_engine_init_sp)
    int32_t n, pad0;
    double prob;
    unsigned long long pool_games, pad[29];     // games started from the pool
};
// the pool reaches k_start_pool as an argument of its own: every other kernel keeps its arguments.  start_index [G]: the entry the
// slot's current game started from, or -1
struct SpDev { int32_t *start_index; SpHead *head; };
static_assert(sizeof(GzHead) == 16 && sizeof(ArHead) == 16 && sizeof(GrHead) == 256 && sizeof(SpHead) == 256, "the heads' layout");
static_assert(sizeof(xq_game_record) == XQ_RECORD_BYTES && offsetof(xq_game_record, moves) == 16, "xq_game_record layout");

__host__ __device__ constexpr size_t align_up(size_t x) { return (x + 255) & ~(size_t)255; }
__host__ __device__ constexpr size_t ow_max(size_t a, size_t b) { return a > b ? a : b; }
__host__ __device__ constexpr size_t ow_table_bytes(size_t S, size_t K) { return (S + 2 + (K > 1 ? K : 0)) * 8; }
__host__ __device__ constexpr size_t ow_gz_head(size_t S) { return ow_table_bytes(S, 1); }
__host__ __device__ constexpr size_t ow_gz_vhat(size_t S) { return ow_gz_head(S) + sizeof(GzHead); }
__host__ __device__ constexpr size_t ow_gz_visits(size_t G, size_t S) { return ow_gz_vhat(S) + G * 8; }
struct ArOff { size_t head, op_counts, op_actions, n_live, rows[2], x[2], moves[2], counts[2], end; };
__host__ __device__ constexpr ArOff ar_off(size_t G, size_t S) {
    ArOff a{};
    size_t o = align_up(ow_table_bytes(S, 1));
    a.head = o; o = align_up(o + sizeof(ArHead));
    a.op_counts = o; o = align_up(o + G * 4);
    a.op_actions = o; o = align_up(o + G * XQ_ARENA_MAX_OPENING * 2);
    a.n_live = o; o = align_up(o + 2 * 4);
    for (int m = 0; m < 2; ++m) {
        a.rows[m] = o; o = align_up(o + G * 4);
        a.x[m] = o; o = align_up(o + G * XQ_STATE_FLOATS * 4);
        a.moves[m] = o; o = align_up(o + G * XQ_MAXM * 2);
        a.counts[m] = o; o = align_up(o + G * 4);
    }
    a.end = o;
    return a;
}
__host__ __device__ constexpr size_t sv_off(size_t G, size_t S, bool arena_opts) { return arena_opts ? ar_off(G, S).end : align_up(ow_table_bytes(S, 1)); }
__host__ __device__ constexpr size_t sv_bytes(size_t G) { return G * SV_WORDS * 8; }
// the end of the front's last block (m = 0: no Gumbel words), and the region's size (max_out_games = 0: no records, n = 0: no pool)
__host__ __device__ constexpr size_t ow_front_end(size_t G, size_t S, size_t K, size_t m, bool arena_opts, bool solver) {
    return ow_max(ow_max(ow_table_bytes(S, K), m ? ow_gz_visits(G, S) + m * S * 2 : 0),
                  ow_max(arena_opts ? ar_off(G, S).end : 0, solver ? sv_off(G, S, arena_opts) + sv_bytes(G) : 0));
}
__host__ __device__ constexpr size_t gr_log_bytes(size_t G) { return align_up(G * XQ_RECORD_MAX_PLIES * 2); }
__host__ __device__ constexpr size_t gr_open_bytes(size_t G) { return align_up(G * 2); }
__host__ __device__ constexpr size_t sp_rows_bytes(size_t n) { return align_up(n * XQ_BS); }
__host__ __device__ constexpr size_t sp_index_bytes(size_t G) { return align_up(G * 4); }
__host__ __device__ constexpr size_t ow_region_bytes(size_t front_end, size_t G, size_t max_out_games, size_t n) {
    return max_out_games ? align_up(front_end) + max_out_games * XQ_RECORD_BYTES + gr_log_bytes(G) + gr_open_bytes(G) + sizeof(GrHead)
           : n           ? align_up(front_end) + sp_rows_bytes(n) + sp_index_bytes(G) + sizeof(SpHead)
                         : front_end;
}
// the tail, from the region's end
__host__ __device__ constexpr size_t ow_tail_head(size_t end) { return end - 256; }      // GrHead or SpHead
__host__ __device__ constexpr size_t ow_gr_opening(size_t end, size_t G) { return ow_tail_head(end) - gr_open_bytes(G); }
__host__ __device__ constexpr size_t ow_gr_log(size_t end, size_t G) { return ow_gr_opening(end, G) - gr_log_bytes(G); }
__host__ __device__ constexpr size_t ow_gr_ring(size_t end, size_t G, size_t max_out_games) { return ow_gr_log(end, G) - max_out_games * XQ_RECORD_BYTES; }
__host__ __device__ constexpr size_t ow_sp_index(size_t end, size_t G) { return ow_tail_head(end) - sp_index_bytes(G); }
__host__ __device__ constexpr size_t ow_sp_rows(size_t end, size_t G, size_t n) { return ow_sp_index(end, G) - sp_rows_bytes(n); }

// The kernels hold one start of the tail (Dev.gr_log, SpDev.start_index) and step from it, and reach the Gumbel words by pointer
// steps from the table (written through the map's functions, k_select<GUMBEL> schedules differently); every step is the map's.
__host__ __device__ inline uint16_t *gr_opening(uint16_t *log, size_t G) { return (uint16_t *)((char *)log + gr_log_bytes(G)); }
__host__ __device__ inline GrHead *gr_head(uint16_t *log, size_t G) { return (GrHead *)((char *)log + gr_log_bytes(G) + gr_open_bytes(G)); }
__host__ __device__ inline xq_game_record *gr_ring(uint16_t *log, size_t max_out_games) { return (xq_game_record *)log - max_out_games; }
__host__ __device__ inline int8_t *sp_rows(int32_t *start_index, size_t n) { return (int8_t *)start_index - sp_rows_bytes(n); }
__device__ __forceinline__ const GzHead *gz_head(const Dev &E) { return (const GzHead *)(E.sqrt_tab + E.cfg.num_simulations + 2); }
__device__ __forceinline__ double *gz_vhat(const Dev &E) { return (double *)(gz_head(E) + 1); }
__device__ __forceinline__ const uint16_t *gz_table(const Dev &E) { return (const uint16_t *)(gz_vhat(E) + E.cfg.n_games); }
static_assert(ow_gr_log(1 << 20, 5) + gr_log_bytes(5) == ow_gr_opening(1 << 20, 5) &&
              ow_gr_log(1 << 20, 200) + gr_log_bytes(200) + gr_open_bytes(200) == ow_tail_head(1 << 20) &&
              ow_gr_log(1 << 20, 5) - 3 * sizeof(xq_game_record) == ow_gr_ring(1 << 20, 5, 3) &&
              ow_sp_index(1 << 20, 5) - sp_rows_bytes(3) == ow_sp_rows(1 << 20, 5, 3), "gr_opening, gr_head, gr_ring, sp_rows step as the map does");
static_assert(ow_gz_head(800) == (800 + 2) * sizeof(double) && ow_gz_vhat(7) == ow_gz_head(7) + 1 * sizeof(GzHead) &&
              ow_gz_visits(5, 7) == ow_gz_vhat(7) + 5 * sizeof(double), "gz_head, gz_vhat, gz_table step as the map does");
char *ow_base(const xq_engine *e) { return (char *)e->p[P_SQRT]; }
size_t ow_end(const xq_engine *e) { return (size_t)((char *)e->p[P_MNOISE] - (char *)e->p[P_SQRT]); }    // the region, from the handle

Dev make_dev(const xq_engine *e) {
    Dev d;
    d.cfg = e->cfg;
    d.node_cap = e->node_cap; d.path_cap = e->path_cap; d.stage_cap = e->stage_cap;
    d.board = (int8_t *)e->p[P_BOARD]; d.hist = (int8_t *)e->p[P_HIST]; d.gi = (int32_t *)e->p[P_GI];
    d.resign = (double *)e->p[P_RESIGN]; d.pmoves = (uint16_t *)e->p[P_PMOVES]; d.path = (int32_t *)e->p[P_PATH];
    d.tN = (int32_t *)e->p[P_TN]; d.tW = (double *)e->p[P_TW]; d.tP = (float *)e->p[P_TP];
    d.tA = (uint16_t *)e->p[P_TA]; d.tC = (int32_t *)e->p[P_TC]; d.tM = (uint16_t *)e->p[P_TM];
    d.rootP = (double *)e->p[P_ROOTP]; d.stage = (uint8_t *)e->p[P_STAGE]; d.outs = (uint8_t *)e->p[P_OUTS];
    d.outr = (uint8_t *)e->p[P_OUTR]; d.cnt = (unsigned int *)e->p[P_CNT];
    d.started = (unsigned long long *)((char *)e->p[P_CNT] + 16);
    d.stats = (unsigned long long *)e->p[P_STATS]; d.inject = (const uint64_t *)e->p[P_INJECT];
    d.sqrt_tab = (const double *)e->p[P_SQRT]; d.mnoise = (double *)e->p[P_MNOISE]; d.req = (int32_t *)e->p[P_REQ];
    d.perpetual = (e->pad0 & PAD0_PERPETUAL) != 0;
    d.root_stats = (e->pad0 & PAD0_ROOT_STATS) != 0;
    d.gr_log = (e->pad0 & PAD0_GAME_RECORDS) ? (uint16_t *)(ow_base(e) + ow_gr_log(ow_end(e), (size_t)e->cfg.n_games)) : nullptr;
    return d;
}

int leaves_of(const xq_engine *e) { return (e->pad0 & 0xFFFF) > 1 ? (e->pad0 & 0xFFFF) : 1; }
bool reuse_of(const xq_engine *e) { return ((unsigned)e->pad0 >> 16) & XQ_ENGINE_TREE_REUSE; }
bool cap_of(const xq_engine *e) { return (e->pad0 & PAD0_CAP) != 0; }
bool forced_of(const xq_engine *e) { return (e->pad0 & PAD0_FORCED) != 0; }
bool gumbel_of(const xq_engine *e) { return (e->pad0 & PAD0_GUMBEL) != 0; }
bool solver_of(const xq_engine *e) { return (e->pad0 & PAD0_SOLVER) != 0; }
bool mirror_of(const xq_engine *e) { return (e->pad0 & PAD0_EVAL_MIRROR) != 0; }
bool records_of(const xq_engine *e) { return e && (e->pad0 & PAD0_GAME_RECORDS) != 0 && e->cfg.n_games > 0 && e->p[P_MNOISE]; }
bool pool_of(const xq_engine *e) { return e && (e->pad0 & PAD0_START_POOL) != 0 && e->cfg.n_games > 0 && e->p[P_MNOISE]; }
SpDev make_sp(const xq_engine *e) {
    SpDev p;
    p.head = (SpHead *)(ow_base(e) + ow_tail_head(ow_end(e)));
    p.start_index = (int32_t *)(ow_base(e) + ow_sp_index(ow_end(e), (size_t)e->cfg.n_games));
    return p;
}
bool arena_of(const xq_engine *e) { return e && (e->pad0 & PAD0_ARENA) != 0 && e->cfg.n_games > 0 && e->p[P_SQRT]; }

// ---------------------------------------------------------------------------------------------------------
// RNG: Philox4x32-10 keyed by (seed, rank), counter (slot, kind, ctr, sub); or injected raw draws (tests).  Host-callable as
// well: xq_eval_mirror_bit_host runs the device's own code.
__host__ __device__ __forceinline__ void philox_round(uint32_t &c0, uint32_t &c1, uint32_t &c2, uint32_t &c3, uint32_t k0, uint32_t k1) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
}

__host__ __device__ inline uint64_t philox_u64(uint64_t seed, uint32_t rank, uint32_t slot, uint32_t kind, uint32_t ctr, uint32_t sub) {
    uint32_t c0 = slot, c1 = kind | (sub << 8), c2 = ctr, c3 = rank;
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        philox_round(c0, c1, c2, c3, k0, k1);
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return ((uint64_t)c0 << 32) | c1;
}

// The start-position pool's draw for the game that will carry `game_seq` (xq_engine_init_sp): stateless, never injected.  The entry
// the game starts from, or -1 for the initial position.  xq_start_pool_draw_host runs this code.
constexpr uint32_t RNG_START_POOL = (uint32_t)XQ_RNG_KIND_START_POOL;
__host__ __device__ inline int start_pool_draw(uint64_t seed, uint32_t rank, uint32_t slot, uint32_t game_seq, int n, double prob) {
    const uint64_t x0 = philox_u64(seed, rank, slot, RNG_START_POOL, game_seq, 0u);
    if (!((double)(x0 >> 11) * (1.0 / 9007199254740992.0) < prob)) return -1;      // u64_to_unit(x0) < prob
    return (int)(philox_u64(seed, rank, slot, RNG_START_POOL, game_seq, 1u) % (uint64_t)n);
}

// waiting for an evaluation: k_expand's own predicate
__device__ __forceinline__ bool slot_waits(const Dev &E, int slot) {
    const int ph = E.gi[(size_t)slot * GI_N + GI_PHASE];
    return ph == PH_WAIT_ROOT || ph == PH_WAIT_LEAF;
}

// Stable compaction by ONE workgroup of the rows r < R with live(r), for any R: thread t owns the contiguous rows
// [t K, t K + K), K = ceil(R / 1024); it counts its live rows, a block-wide exclusive scan of the counts gives its first packed
// row, and it writes rows[] in row order.  R = 8192: eight strided 4-byte reads per thread, a few microseconds.
constexpr int CPT = 1024;
template <class Live>
__device__ __forceinline__ void block_compact(const Dev &E, int R, Live live, int32_t *__restrict__ n_live, int32_t *__restrict__ rows) {
    __shared__ int wsum[CPT / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int K = (R + CPT - 1) / CPT;
    const int r0 = t * K, r1 = min(r0 + K, R);
    int cnt = 0;
    for (int r = r0; r < r1; ++r) cnt += live(r);
    int inc = cnt;                                    // inclusive scan within the wave
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int v = __shfl_up(inc, off);
        if (lane >= off) inc += v;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    int base = 0, total = 0;
#pragma unroll
    for (int w = 0; w < CPT / 64; ++w) {
        const int v = wsum[w];
        base += w < wave ? v : 0;
        total += v;
    }
    int o = base + inc - cnt;
    for (int r = r0; r < r1; ++r)
        if (live(r)) rows[o++] = r;
    if (t == 0) {
        *n_live = total;
        E.stats[ST_ROWS] += (unsigned long long)total;   // slot 0's counter row: k_reduce_stats sums the column
    }
}

}  // namespace
