// xq_engine.hip -- device-resident self-play engine (B3): SoA MCTS trees in HBM, one wavefront per game.
//
//   k_select : per game, advance the game/search state machine until ONE network evaluation is needed:
//                finish games (flush samples with z), start games (random opening), finish moves (visit
//                counts -> sample -> sampled action -> make_move), run simulations: PUCT descent with lanes over
//                the children of each node (coalesced N/W/P reads), moves replayed on an LDS board with the
//                12-board repetition ring, leaf terminal test (full ordered move generation).  Terminal leaves
//                are backed up in place and the next simulation starts at once, so every live slot hands exactly
//                one position to the evaluator per step.
//   k_expand : per game, consume the evaluator's output: softmax over all 8100 logits (as model.py:122), the
//                reference's sequential-float32 mask-and-normalise (mcts.py:176-188), children appended to the
//                slot's bump arena, Dirichlet noise at the root (mcts.py:117-121), resign probe
//                (parallel_selfplay.py:110-121), backup along the recorded path (mcts.py:66-73).
//   k_reroot : tree reuse (opt-in, XQ_ENGINE_TREE_REUSE; k_select<true> / k_expand<true>): the chosen child's subtree moved to the
//                front of the slot's arena, in place, between select and expand of the step that ends a move.
//
// Numeric contract (pinned by tests against the reference's MCTS under a stub evaluator): priors float32,
// PUCT evaluated in float32 as f32(q) + ((f32(c)*P)*f32(sqrt(N_parent)))/f32(1+N); at a noisy root (and for the
// uniform fallback) priors and PUCT are float64; W accumulates in float64; first maximum wins.
// Floating-point contraction is OFF for this file.
#include <float.h>
#include <math.h>
#include <string.h>

#include "xq_common.h"
#include "xq_rules.cuh"

#pragma clang fp contract(off)

using namespace xq;

static_assert(sizeof(xq_sample) == XQ_SAMPLE_BYTES, "xq_sample layout");
static_assert(sizeof(xq_game_result) == XQ_RESULT_BYTES, "xq_game_result layout");

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
constexpr uint32_t RNG_ARENA_OPENING = 8u;  // xq_engine_init_ar: keyed by the PAIR and rank 0, never by the slot (7 is k_init's stagger)

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
};

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
    return d;
}

// Gumbel root search (xq_engine_init_gz): its words live behind the square-root table, in that table's workspace region (the handle,
// the config struct and the per-slot state words are full): the parameters, the root's network value of every slot, and the
// considered-visit tables, row k - 1 for k considered moves.  K = 1 always, so the square-root table has S + 2 entries.
struct GzHead {
    int32_t m;                      // considered moves at most
    float c_visit, c_scale;         // rounded to float32 once, widened at every use
    int32_t pad;
};
static_assert(sizeof(GzHead) == 16, "GzHead layout");

size_t gz_bytes(size_t G, size_t S, size_t m) { return sizeof(GzHead) + G * 8 + m * S * 2; }

__device__ __forceinline__ const GzHead *gz_head(const Dev &E) { return (const GzHead *)(E.sqrt_tab + E.cfg.num_simulations + 2); }
__device__ __forceinline__ double *gz_vhat(const Dev &E) { return (double *)(gz_head(E) + 1); }
__device__ __forceinline__ const uint16_t *gz_table(const Dev &E) { return (const uint16_t *)(gz_vhat(E) + E.cfg.n_games); }

// Arena options (xq_engine_init_ar; manual_moves = 2, so never a Gumbel engine): their words lie behind the square-root table as
// well, from the next 256-byte boundary on: the parameters, what every slot played as its opening, and the two buffer sets of the
// per-model packed step (set 0: the new model's slots, set 1: the old model's).  Offsets from the table's first byte.
struct ArHead {
    int32_t opening_plies, first_game, pad[2];
};
static_assert(sizeof(ArHead) == 16, "ArHead layout");

struct ArOff {
    size_t head, op_counts, op_actions, n_live, rows[2], x[2], moves[2], counts[2], end;
};

__host__ __device__ inline size_t ar_align(size_t x) { return (x + 255) & ~(size_t)255; }

__host__ __device__ inline ArOff ar_off(size_t G, size_t S) {
    ArOff a;
    size_t o = ar_align((S + 2) * 8);
    a.head = o; o = ar_align(o + sizeof(ArHead));
    a.op_counts = o; o = ar_align(o + G * 4);
    a.op_actions = o; o = ar_align(o + G * XQ_ARENA_MAX_OPENING * 2);
    a.n_live = o; o = ar_align(o + 2 * 4);
    for (int m = 0; m < 2; ++m) {
        a.rows[m] = o; o = ar_align(o + G * 4);
        a.x[m] = o; o = ar_align(o + G * XQ_STATE_FLOATS * 4);
        a.moves[m] = o; o = ar_align(o + G * XQ_MAXM * 2);
        a.counts[m] = o; o = ar_align(o + G * 4);
    }
    a.end = o;
    return a;
}

// get_sequence_of_considered_visits(k, S) of include/xq_hip.h: out[t] = the visit count a root child must have to be a
// candidate of simulation t
__host__ void gz_considered_visits(int k, int S, uint16_t *out) {
    if (k <= 1) { for (int t = 0; t < S; ++t) out[t] = (uint16_t)t; return; }
    int log2max = 0;
    while ((1 << log2max) < k) ++log2max;
    int n = 0, considered = k, base = 0;           // every considered move has `base` visits when a phase starts
    while (n < S) {
        int extra = S / (log2max * considered);
        if (extra < 1) extra = 1;
        for (int e = 0; e < extra; ++e)
            for (int i = 0; i < considered && n < S; ++i) out[n++] = (uint16_t)(base + e);
        base += extra;
        considered = considered / 2 > 2 ? considered / 2 : 2;
    }
}

// ---------------------------------------------------------------------------------------------------------
// RNG: Philox4x32-10 keyed by (seed, rank), counter (slot, kind, ctr, sub); or injected raw draws (tests).
__device__ __forceinline__ void philox_round(uint32_t &c0, uint32_t &c1, uint32_t &c2, uint32_t &c3, uint32_t k0, uint32_t k1) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
}

__device__ inline uint64_t philox_u64(uint64_t seed, uint32_t rank, uint32_t slot, uint32_t kind, uint32_t ctr, uint32_t sub) {
    uint32_t c0 = slot, c1 = kind | (sub << 8), c2 = ctr, c3 = rank;
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        philox_round(c0, c1, c2, c3, k0, k1);
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return ((uint64_t)c0 << 32) | c1;
}

// raw 64-bit draw number `ctr` (0-based) of stream `kind` of this slot
__device__ inline uint64_t draw_u64(const Dev &E, int slot, int kind, int ctr, unsigned long long *st) {
    if (E.cfg.inject_len > 0) {
        if (ctr >= E.cfg.inject_len) { st[ST_OVF] |= 2ull; return 0; }
        return E.inject[((size_t)slot * 4 + kind) * E.cfg.inject_len + ctr];
    }
    return philox_u64(E.cfg.seed, (uint32_t)E.cfg.rank, (uint32_t)slot, (uint32_t)kind, (uint32_t)ctr, 0);
}

__device__ inline double u64_to_unit(uint64_t x) { return (double)(x >> 11) * (1.0 / 9007199254740992.0); }

// Gamma(alpha) variate for lane-private use (Marsaglia-Tsang on alpha+1, boosted by U^(1/alpha))
__device__ __forceinline__ double gamma_variate(const Dev &E, int slot, int ctr, double alpha) {
    const double d = alpha + 1.0 - 1.0 / 3.0, c = 1.0 / sqrt(9.0 * d);
    double g = d;
    for (uint32_t it = 0; it < 64; ++it) {
        const uint64_t r0 = philox_u64(E.cfg.seed, (uint32_t)E.cfg.rank, (uint32_t)slot, RNG_DIRICHLET, (uint32_t)ctr, 1 + 2 * it);
        const uint64_t r1 = philox_u64(E.cfg.seed, (uint32_t)E.cfg.rank, (uint32_t)slot, RNG_DIRICHLET, (uint32_t)ctr, 2 + 2 * it);
        const double u1 = ((double)(r0 >> 11) + 0.5) * (1.0 / 9007199254740992.0);
        const double u2 = u64_to_unit(r1);
        const double u3 = ((double)(uint32_t)(r0 * 0x9E3779B97F4A7C15ull >> 32) + 0.5) * (1.0 / 4294967296.0);
        const double x = sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2);
        double v = 1.0 + c * x;
        if (v <= 0.0) continue;
        v = v * v * v;
        if (log(u3) < 0.5 * x * x + d * (1.0 - v + log(v))) { g = d * v; break; }
    }
    const uint64_t rb = philox_u64(E.cfg.seed, (uint32_t)E.cfg.rank, (uint32_t)slot, RNG_DIRICHLET, (uint32_t)ctr, 0);
    const double ub = ((double)(rb >> 11) + 0.5) * (1.0 / 9007199254740992.0);
    return g * pow(ub, 1.0 / alpha);
}

// ---------------------------------------------------------------------------------------------------------
struct SelectLds {
    __attribute__((aligned(16))) int8_t root[XQ_BS];          // the game's real board
    __attribute__((aligned(16))) int8_t rhist[XQ_HIST][XQ_BS]; // its last 12 pre-move boards (slot = ply % 12)
    __attribute__((aligned(16))) int8_t board[XQ_BS];         // simulation board
    __attribute__((aligned(16))) int8_t hist[XQ_HIST][XQ_BS];  // simulation ring
    MoveGenLds mg;
    uint16_t moves[XQ_MAXM];
    uint16_t sa[XQ_MAXM];
    double sw[XQ_MAXM];
    double cdf[XQ_MAXM];
    uint16_t a_tmp[XQ_MAXM];
    double w_tmp[XQ_MAXM];
};

__device__ __forceinline__ void lds_copy_dwords(void *dst, const void *src, int ndw) {
    const int lane = lane_id();
    uint32_t *d = (uint32_t *)dst;
    const uint32_t *s = (const uint32_t *)src;
    for (int i = lane; i < ndw; i += 64) d[i] = s[i];
}

__device__ __forceinline__ void init_board_lds(int8_t *b) {
    const int lane = lane_id();
    for (int sq = lane; sq < XQ_BS; sq += 64) {
        int v = 0;
        if (sq < 90) {
            const int r = sq / 9, c = sq % 9;
            const int back = (c == 0 || c == 8) ? 5 : (c == 1 || c == 7) ? 4 : (c == 2 || c == 6) ? 3 : (c == 3 || c == 5) ? 2 : 1;
            if (r == 0) v = back;
            else if (r == 9) v = -back;
            else if (r == 2 && (c == 1 || c == 7)) v = 6;
            else if (r == 7 && (c == 1 || c == 7)) v = -6;
            else if (r == 3 && (c % 2 == 0)) v = 7;
            else if (r == 6 && (c % 2 == 0)) v = -7;
        }
        b[sq] = (int8_t)v;
    }
}

// game.py:565-616 on an LDS position.  Leaves the ordered legal moves in `moves` (count in *cnt) whenever both
// kings stand.  Wave-uniform result.
__device__ inline bool wave_game_over(const int8_t *b, const int8_t (*ring)[XQ_BS], int side, int mc, int nocap,
                                      MoveGenLds &mg, uint16_t *moves, int *cnt, int *winner, int *ovf) {
    const VMove none{-1, -1, 0};
    const int lane = lane_id();
    *cnt = 0;
    if (find_king(b, none, 1) < 0) { *winner = -1; return true; }
    if (find_king(b, none, -1) < 0) { *winner = 1; return true; }
    const int n = wave_movegen(b, side, mg, moves, ovf);
    *cnt = n;
    if (n == 0) { *winner = -side; return true; }
    if (nocap >= 120) { *winner = 0; return true; }
    if (mc >= 200) {
        int red, black;
        wave_material(b, red, black);
        const int diff = red - black;
        *winner = diff > 30 ? 1 : (diff < -30 ? -1 : 0);
        return true;
    }
    if (mc >= 6) {
        const int k = mc < XQ_HIST ? mc : XQ_HIST;
        int rep = 0;
        for (int e = 0; e < k; ++e) {
            const int8_t *h = ring[(mc - 1 - e) % XQ_HIST];
            const uint32_t x = lane < 23 ? (((const uint32_t *)h)[lane] ^ ((const uint32_t *)b)[lane]) : 0u;
            if (__ballot(x != 0u) == 0ull) ++rep;
        }
        if (rep >= 3) { *winner = 0; return true; }
    }
    *winner = 2;
    return false;
}

// game.py:528-550 on an LDS position + ring.  Wave-uniform scalars updated by reference.
__device__ __forceinline__ void wave_make_move(int8_t *b, int8_t (*ring)[XQ_BS], int action, int &side, int &mc, int &nocap) {
    const int from = action / 90, to = action - from * 90;
    lds_copy_dwords(ring[mc % XQ_HIST], b, XQ_BS / 4);
    const int captured = b[to], mover = b[from];
    wave_sync();
    if (lane_id() == 0) { b[to] = (int8_t)mover; b[from] = 0; }
    wave_sync();
    nocap = captured != 0 ? 0 : nocap + 1;
    side = -side;
    mc += 1;
}

// One slot's tree: six arrays of node_cap entries (node 0 is the root)
struct Tree {
    int32_t *N; double *W; float *P; uint16_t *A; int32_t *C; uint16_t *M;
};

__device__ __forceinline__ Tree slot_tree(const Dev &E, int slot) {
    const size_t nb = (size_t)slot * E.node_cap;
    return Tree{E.tN + nb, E.tW + nb, E.tP + nb, E.tA + nb, E.tC + nb, E.tM + nb};
}

// mcts.py:66-73 along path[0..depth].  VL (leaf batching): the pending descent's virtual loss is removed on the way.
template <bool VL>
__device__ __forceinline__ void wave_backup(const Tree &T, int32_t *vl, const int32_t *path, int depth, double v) {
    for (int j = lane_id(); j <= depth; j += 64) {
        const int nd = path[j];
        const double s = ((depth - j) & 1) ? -v : v;
        T.N[nd] += 1;
        T.W[nd] += s;
        if (VL) vl[nd] -= 1;
    }
}

// ---------------------------------------------------------------------------------------------------------
// The per-slot phases of the select kernels (k_select<REUSE, CAP, FORCED> and k_select_multi), one copy each.
//
// Wave-uniform state of the slot a select kernel works on: slot_load reads it from gi[], slot_store writes it back.  The
// counter deltas are kept wave-uniform and written by lane 0 at the end.
struct Slot {
    int slot, lane;
    int32_t *gi;
    unsigned long long *st;
    Tree T;
    int side, mc, nocap;                    // the real game (its board and ring are SelectLds.root / .rhist)
    int sims_done, n_samples, game_seq;
    int rng_ctr[4];
    int ovf;
    bool dirty;                             // real game state changed -> write back
    unsigned long long d_sims, d_term, d_moves, d_depth, d_scan;
    unsigned d_forced, d_prunedv, d_prunedc;    // FORCED only (one launch runs fewer than 2^31 simulations)
};

__device__ __forceinline__ void slot_load(Slot &s) {
    const int32_t *gi = s.gi;
    s.side = __builtin_amdgcn_readfirstlane(gi[GI_SIDE]);
    s.mc = __builtin_amdgcn_readfirstlane(gi[GI_MC]);
    s.nocap = __builtin_amdgcn_readfirstlane(gi[GI_NOCAP]);
    s.sims_done = __builtin_amdgcn_readfirstlane(gi[GI_SIMS]);
    s.n_samples = __builtin_amdgcn_readfirstlane(gi[GI_NSAMP]);
    s.game_seq = __builtin_amdgcn_readfirstlane(gi[GI_GSEQ]);
    s.rng_ctr[0] = __builtin_amdgcn_readfirstlane(gi[GI_RNG0]); s.rng_ctr[1] = __builtin_amdgcn_readfirstlane(gi[GI_RNG1]);
    s.rng_ctr[2] = __builtin_amdgcn_readfirstlane(gi[GI_RNG2]); s.rng_ctr[3] = __builtin_amdgcn_readfirstlane(gi[GI_RNG3]);
    s.ovf = 0;
    s.dirty = false;
    s.d_sims = s.d_term = s.d_moves = s.d_depth = s.d_scan = 0;
    s.d_forced = s.d_prunedv = s.d_prunedc = 0;
}

// the real game's board and ring (when a move or a new game changed them), the state words and the common counters
__device__ __forceinline__ void slot_store(const Dev &E, const Slot &s, const SelectLds &L, int phase) {
    if (s.dirty) {
        lds_copy_dwords(E.board + (size_t)s.slot * XQ_BS, L.root, XQ_BS / 4);
        lds_copy_dwords(E.hist + (size_t)s.slot * XQ_HIST * XQ_BS, L.rhist, XQ_HIST * XQ_BS / 4);
    }
    if (s.lane == 0) {
        int32_t *gi = s.gi;
        unsigned long long *st = s.st;
        gi[GI_SIDE] = s.side; gi[GI_MC] = s.mc; gi[GI_NOCAP] = s.nocap; gi[GI_PHASE] = phase; gi[GI_SIMS] = s.sims_done;
        gi[GI_NSAMP] = s.n_samples; gi[GI_GSEQ] = s.game_seq;
        gi[GI_RNG0] = s.rng_ctr[0]; gi[GI_RNG1] = s.rng_ctr[1]; gi[GI_RNG2] = s.rng_ctr[2]; gi[GI_RNG3] = s.rng_ctr[3];
        st[ST_SIMS] += s.d_sims; st[ST_TERM] += s.d_term; st[ST_MOVES] += s.d_moves; st[ST_DEPTH] += s.d_depth;
        st[ST_SCAN] += s.d_scan;
        if (s.ovf) st[ST_OVF] |= (unsigned long long)s.ovf << 8;
    }
}

// PH_FINISHED: flush the finished game's samples with z (parallel_selfplay.py:123-132) and its result
__device__ __forceinline__ void slot_flush_finished(const Dev &E, const Slot &s) {
    const int lane = s.lane, n_samples = s.n_samples;
    unsigned long long *st = s.st;
    const int winner = __builtin_amdgcn_readfirstlane(s.gi[GI_FWINNER]);
    const int reason = __builtin_amdgcn_readfirstlane(s.gi[GI_FREASON]);
    unsigned base = 0;
    bool fits = true;
    if (n_samples > 0) {
        if (lane == 0) base = atomicAdd(&E.cnt[0], (unsigned)n_samples);
        base = __builtin_amdgcn_readfirstlane(base);
        fits = (unsigned long long)base + (unsigned)n_samples <= (unsigned)E.cfg.max_out_samples;
        if (fits) {
            const uint8_t *src = E.stage + (size_t)s.slot * E.stage_cap * XQ_SAMPLE_BYTES;
            uint8_t *dst = E.outs + (size_t)base * XQ_SAMPLE_BYTES;
            const int ndw = n_samples * (XQ_SAMPLE_BYTES / 4);
            for (int i = lane; i < ndw; i += 64) ((uint32_t *)dst)[i] = ((const uint32_t *)src)[i];
            for (int i = lane; i < n_samples; i += 64) {
                const int sside = ((const int8_t *)src)[(size_t)i * XQ_SAMPLE_BYTES + 90];
                ((int8_t *)dst)[(size_t)i * XQ_SAMPLE_BYTES + 91] = (int8_t)(winner == 0 ? 0 : (winner == sside ? 1 : -1));
            }
        }
    }
    if (lane == 0) {
        if (fits) st[ST_SAMP] += (unsigned)n_samples; else st[ST_DROP] += (unsigned)n_samples;
        const unsigned r = atomicAdd(&E.cnt[1], 1u);
        if (r < (unsigned)E.cfg.max_out_results) {
            xq_game_result res;
            res.slot = (uint32_t)s.slot; res.game_seq = (uint32_t)s.game_seq; res.winner = (int8_t)winner;
            res.reason = (uint8_t)reason; res.steps = (uint16_t)s.mc; res.n_samples = (uint16_t)n_samples;
            res.reserved = 0;
            *(xq_game_result *)(E.outr + (size_t)r * XQ_RESULT_BYTES) = res;
        }
        st[ST_GAMES] += 1;
        st[winner == 1 ? ST_RED : (winner == -1 ? ST_BLACK : ST_DRAW)] += 1;
        st[ST_PLIES] += (unsigned)s.mc;
        if (reason == 3) st[ST_RESIGN] += 1;
    }
}

// PH_NEWGAME: new game + random opening (parallel_selfplay.py:58-72).  False when the games quota is used up: the slot idles.
__device__ __forceinline__ bool slot_new_game(const Dev &E, Slot &s, SelectLds &L, bool arena) {
    const int lane = s.lane, slot = s.slot;
    unsigned long long idx = 0;
    if (lane == 0) idx = atomicAdd(E.started, 1ull);
    idx = ((unsigned long long)__builtin_amdgcn_readfirstlane((unsigned)(idx >> 32)) << 32) |
          (unsigned)__builtin_amdgcn_readfirstlane((unsigned)idx);
    if (E.cfg.games_target > 0 && idx >= (unsigned long long)E.cfg.games_target) return false;
    s.game_seq += 1;
    s.n_samples = 0;
    init_board_lds(L.root);
    s.side = 1; s.mc = 0; s.nocap = 0;
    if (lane == 0) { s.gi[GI_RESIGN_N] = 0; s.st[ST_STARTED] += 1; }
    wave_sync();
    const int R = arena ? 0 : E.cfg.random_opening_moves;
    const int k = R > 0 ? (int)(draw_u64(E, slot, RNG_RANDINT, s.rng_ctr[RNG_RANDINT], s.st) % (uint64_t)(R + 1)) : 0;
    if (!arena) s.rng_ctr[RNG_RANDINT] += 1;   // random.randint is called even when R == 0
    for (int i = 0; i < k; ++i) {
        const int cnt = wave_movegen(L.root, s.side, L.mg, L.moves, &s.ovf);
        if (cnt == 0) break;
        const int pick = (int)(draw_u64(E, slot, RNG_CHOICE, s.rng_ctr[RNG_CHOICE], s.st) % (uint64_t)cnt);
        s.rng_ctr[RNG_CHOICE] += 1;
        const int action = L.moves[pick];
        wave_make_move(L.root, L.rhist, action, s.side, s.mc, s.nocap);
        int c2, w2;
        if (wave_game_over(L.root, L.rhist, s.side, s.mc, s.nocap, L.mg, L.moves, &c2, &w2, &s.ovf)) {
            init_board_lds(L.root);
            s.side = 1; s.mc = 0; s.nocap = 0;
            wave_sync();
            break;
        }
    }
    s.dirty = true;
    return true;
}

// AROPEN (arena options, xq_engine_init_ar), after slot_new_game: the paired random opening of arena game g = first_game + slot.
// Exactly R uniformly random legal plies, ply i the move x_i % cnt of the ordered legal moves; x_i belongs to the PAIR g / 2
// (philox_u64(seed, 0, g / 2, 8, i, 0)) or, with injected draws, is entry i of the slot's own choice stream.  A ply that ends the
// game restarts it from the initial position without an opening (recorded count 0), as self-play does.  The plies count in
// move_count.  What was played goes to the engine's record (xq_engine_arena_openings).
__device__ __forceinline__ void slot_arena_opening(const Dev &E, Slot &s, SelectLds &L) {
    const ArOff o = ar_off((size_t)E.cfg.n_games, (size_t)E.cfg.num_simulations);
    char *base = (char *)E.sqrt_tab;
    const ArHead *h = (const ArHead *)(base + o.head);
    const int R = __builtin_amdgcn_readfirstlane(h->opening_plies);
    const int pair = (__builtin_amdgcn_readfirstlane(h->first_game) + s.slot) >> 1;
    uint16_t *rec = (uint16_t *)(base + o.op_actions) + (size_t)s.slot * XQ_ARENA_MAX_OPENING;
    int played = 0;
    for (int i = 0; i < R; ++i) {
        const int cnt = wave_movegen(L.root, s.side, L.mg, L.moves, &s.ovf);
        if (cnt == 0) break;
        uint64_t x = 0;
        if (E.cfg.inject_len > 0) {
            if (i < E.cfg.inject_len) x = E.inject[((size_t)s.slot * 4 + RNG_CHOICE) * E.cfg.inject_len + i];
            else s.st[ST_OVF] |= 2ull;
        } else {
            x = philox_u64(E.cfg.seed, 0u, (uint32_t)pair, RNG_ARENA_OPENING, (uint32_t)i, 0u);
        }
        const int action = L.moves[(int)(x % (uint64_t)cnt)];
        wave_make_move(L.root, L.rhist, action, s.side, s.mc, s.nocap);
        if (s.lane == 0) rec[i] = (uint16_t)action;
        played = i + 1;
        int c2, w2;
        if (wave_game_over(L.root, L.rhist, s.side, s.mc, s.nocap, L.mg, L.moves, &c2, &w2, &s.ovf)) {
            init_board_lds(L.root);
            s.side = 1; s.mc = 0; s.nocap = 0;
            wave_sync();
            played = 0;
            break;
        }
    }
    if (s.lane == 0) {
        for (int i = played; i < XQ_ARENA_MAX_OPENING; ++i) rec[i] = 0;
        ((int32_t *)(base + o.op_counts))[s.slot] = played;
    }
    s.dirty = true;
}

// PH_NEWPOS, the root request: terminal status of the real position (0: to be searched), its planes to x and its ordered
// legal moves to pmoves (the slot's first request row), and a fresh tree root.  Returns the number of legal moves.
__device__ __forceinline__ int slot_root_request(const Dev &E, Slot &s, SelectLds &L, bool manual, bool arena, float *x,
                                                 uint16_t *pmoves, int &status) {
    const Tree &T = s.T;
    int cnt, winner;
    status = 0;
    const bool done = wave_game_over(L.root, L.rhist, s.side, s.mc, s.nocap, L.mg, L.moves, &cnt, &winner, &s.ovf);
    if (done) status = 1;
    else if (arena && s.mc >= E.cfg.max_game_length) {     // train.py:477,494-496: not over after max plies => draw
        winner = 0;
        status = 2;
    } else if (!manual && !arena && s.mc >= E.cfg.max_game_length) {   // parallel_selfplay.py:79-89
        int red, black;
        wave_material(L.root, red, black);
        const int diff = red - black;
        winner = diff > 30 ? 1 : (diff < -30 ? -1 : 0);
        status = 2;
    }
    wave_encode(L.root, s.side, x);
    for (int j = s.lane; j < cnt; j += 64) pmoves[j] = L.moves[j];
    if (s.lane == 0) {
        s.gi[GI_PCOUNT] = cnt; s.gi[GI_RSTATUS] = status; s.gi[GI_RWINNER] = winner;
        s.gi[GI_ALLOC] = 1;
        T.N[0] = 0; T.W[0] = 0.0; T.C[0] = -1; T.M[0] = 0; T.A[0] = 0; T.P[0] = 0.0f;
    }
    s.sims_done = 0;
    return cnt;
}

// first maximum of n[0 .. nch): its index (lowest on ties) and value, wave-uniform
__device__ __forceinline__ int wave_first_max(const int32_t *n, int nch, int &max) {
    int bn = -1, bi = 0x7FFFFFFF;
    for (int i = lane_id(); i < nch; i += 64) {
        const int v = n[i];
        if (v > bn) { bn = v; bi = i; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const int on = __shfl_xor(bn, off), oi = __shfl_xor(bi, off);
        if (on > bn || (on == bn && oi < bi)) { bn = on; bi = oi; }
    }
    max = __builtin_amdgcn_readfirstlane(bn);
    return __builtin_amdgcn_readfirstlane(bi);
}

// the real game advances by one move
__device__ __forceinline__ void slot_play(Slot &s, SelectLds &L, int action) {
    wave_make_move(L.root, L.rhist, action, s.side, s.mc, s.nocap);
    s.d_moves += 1;
    s.dirty = true;
}

// arena move, MCTS.get_action(temperature=0) (mcts.py:166-174, 197-200): first maximum of the visit counts, move order
__device__ __forceinline__ void slot_arena_move(Slot &s, SelectLds &L, int nch, int first) {
    int bn;
    const int bi = wave_first_max(s.T.N + first, nch, bn);
    slot_play(s, L, __builtin_amdgcn_readfirstlane((int)s.T.A[first + bi]));
}

// FORCED: policy target pruning at a kind-1 root.  c* = first maximum of N; P* its PUCT score at the root's final
// count, in the kind-1 float64 arithmetic of the descent; every other visited child gives back, one at a time and
// at most while (d + 1)^2 < f_i, the visits after which its score (q held constant) would still be below P*.
// The pruned counts go to L.w_tmp (slot_end_move's lanes read back only what they wrote here).
__device__ __forceinline__ void wave_prune_visits(const Dev &E, Slot &s, SelectLds &L, const double *rootP, float fp_k, int nch,
                                                  int first) {
    const Tree &T = s.T;
    const int lane = s.lane;
    int bn;
    const int p_star_i = wave_first_max(T.N + first, nch, bn);
    const int nr = __builtin_amdgcn_readfirstlane(T.N[0]);
    const double p_nr = (double)nr, p_sqrt = E.sqrt_tab[nr];
    double p_star;
    {
        const double w = T.W[first + p_star_i];
        double t = E.cfg.c_puct * rootP[p_star_i];
        t = t * p_sqrt;
        t = t / (double)(1 + bn);
        p_star = (bn ? w / (double)bn : 0.0) + t;
    }
    int l_prunedv = 0, l_prunedc = 0;
    for (int i = lane; i < nch; i += 64) {
        int n = T.N[first + i];
        if (i != p_star_i && n > 0) {
            const int n0 = n;
            const double p = rootP[i];
            const double f = ((double)fp_k * p) * p_nr;
            const double q = T.W[first + i] / (double)n0;
            double e = E.cfg.c_puct * p;
            e = e * p_sqrt;
            int d = 0;
            while (n > 1 && (double)(d + 1) * (double)(d + 1) < f && q + e / (double)n < p_star) { n -= 1; d += 1; }
            if (d > 0 && n == 1) n = 0;               // reduced to a single playout: removed
            l_prunedv += n0 - n;
            l_prunedc += n == 0 ? 1 : 0;
        }
        L.w_tmp[i] = (double)n;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { l_prunedv += __shfl_xor(l_prunedv, off); l_prunedc += __shfl_xor(l_prunedc, off); }
    s.d_prunedv += (unsigned)l_prunedv; s.d_prunedc += (unsigned)l_prunedc;
}

// End of a move: the sample (parallel_selfplay.py:97-107) and the sampled action, pi from visit counts (mcts.py:190-206).
// full_move false (a fast move of the playout cap) stages no sample; pruned: the visits are wave_prune_visits' counts in
// L.w_tmp.  Leaves child i's action in L.a_tmp[i]; the caller plays the returned action.
__device__ __forceinline__ int slot_end_move(const Dev &E, Slot &s, SelectLds &L, bool full_move, bool pruned, int nch, int first) {
    const Tree &T = s.T;
    const int lane = s.lane;
    const bool late = s.mc >= E.cfg.temperature_threshold;
    const double inv_t = 1.0 / E.cfg.late_temperature;
    uint8_t *rec = E.stage + ((size_t)s.slot * E.stage_cap + (s.n_samples < E.stage_cap ? s.n_samples : E.stage_cap - 1)) * XQ_SAMPLE_BYTES;
    if (full_move) {
        if (s.n_samples >= E.stage_cap) s.ovf |= 4;
        for (int i = lane; i < XQ_SAMPLE_BYTES / 4; i += 64) ((uint32_t *)rec)[i] = 0u;
        wave_sync_mem();
        for (int i = lane; i < 90; i += 64) rec[i] = (uint8_t)L.root[i];
        if (lane == 0) {
            xq_sample *r = (xq_sample *)rec;
            r->side = (int8_t)s.side; r->z = 0; r->n_moves = (uint8_t)nch; r->late_temp = late ? 1 : 0;
            r->ply = (uint16_t)s.mc; r->slot = (uint32_t)s.slot; r->game_seq = (uint32_t)s.game_seq;
        }
    }
    for (int i = lane; i < nch; i += 64) {
        const int a = T.A[first + i];
        const int n = pruned ? (int)L.w_tmp[i] : T.N[first + i];
        if (full_move) {
            ((xq_sample *)rec)->actions[i] = (uint16_t)a;
            ((xq_sample *)rec)->visits[i] = (uint16_t)(n > 65535 ? 65535 : n);
        }
        L.a_tmp[i] = (uint16_t)a;
        L.w_tmp[i] = late ? (n > 0 ? pow((double)n, inv_t) : 0.0) : (double)n;
    }
    wave_sync();
    // np.random.choice walks the dense pi in ACTION-ID order: sort the (action, weight) pairs by id
    for (int i = lane; i < nch; i += 64) {
        const int a = L.a_tmp[i];
        int rank = 0;
        for (int j = 0; j < nch; ++j) rank += (L.a_tmp[j] < a) ? 1 : 0;
        L.sa[rank] = (uint16_t)a;
        L.sw[rank] = L.w_tmp[i];
    }
    wave_sync();
    const double u = u64_to_unit(draw_u64(E, s.slot, RNG_UNIFORM, s.rng_ctr[RNG_UNIFORM], s.st));
    s.rng_ctr[RNG_UNIFORM] += 1;
    // every lane runs the same short sequential scan (LDS broadcast reads); result is wave-uniform
    double total = 0.0;
    for (int i = 0; i < nch; ++i) total += L.sw[i];
    double run = 0.0;
    for (int i = 0; i < nch; ++i) run += L.sw[i] / total;
    const double last = run;
    run = 0.0;
    int pick = nch - 1;
    for (int i = 0; i < nch; ++i) {
        run += L.sw[i] / total;
        if (run / last > u) { pick = i; break; }
    }
    if (full_move) s.n_samples += 1;
    return __builtin_amdgcn_readfirstlane((int)L.sa[pick]);
}

// GUMBEL: the end of a self-play move at a root of prior kind 3 (include/xq_hip.h).  The played child is the first maximum, over
// the children with N_i == maxN, of rootP[i] + sigma(q_i): no temperature and no draw.  The sample's visits[] are the completed-Q
// improved policy softmax(l_i + sigma(completed q_i)) quantised to 16 bits (reserved0 = 1 says so).  maxN, sumN and the two
// prior-weighted sums run sequentially in move order over LDS (every lane the same scan), so the host model can repeat them bit
// for bit; the maxima are wave reductions.  `considered` / `offprior` take the move's k and whether the played child is not the
// first maximum of the float32 priors.
__device__ __forceinline__ int slot_end_move_gumbel(const Dev &E, Slot &s, SelectLds &L, const double *rootP, int nch, int first,
                                                    unsigned &considered, unsigned &offprior) {
    const Tree &T = s.T;
    const int lane = s.lane;
    uint8_t *rec = E.stage + ((size_t)s.slot * E.stage_cap + (s.n_samples < E.stage_cap ? s.n_samples : E.stage_cap - 1)) * XQ_SAMPLE_BYTES;
    if (s.n_samples >= E.stage_cap) s.ovf |= 4;
    for (int i = lane; i < XQ_SAMPLE_BYTES / 4; i += 64) ((uint32_t *)rec)[i] = 0u;
    wave_sync_mem();
    for (int i = lane; i < 90; i += 64) rec[i] = (uint8_t)L.root[i];
    if (lane == 0) {
        xq_sample *r = (xq_sample *)rec;
        r->side = (int8_t)s.side; r->z = 0; r->n_moves = (uint8_t)nch; r->late_temp = 0;
        r->ply = (uint16_t)s.mc; r->reserved0 = 1; r->slot = (uint32_t)s.slot; r->game_seq = (uint32_t)s.game_seq;
    }
    for (int i = lane; i < nch; i += 64) {
        const int n = T.N[first + i];
        L.a_tmp[i] = (uint16_t)n;                                 // n <= S < 16000
        L.sw[i] = n ? T.W[first + i] / (double)n : 0.0;           // q_i
        L.cdf[i] = (double)T.P[first + i];
    }
    wave_sync();
    int max_n = 0, sum_n = 0;
    double num = 0.0, den = 0.0;
    for (int i = 0; i < nch; ++i) {
        const int n = L.a_tmp[i];
        max_n = n > max_n ? n : max_n;
        sum_n += n;
        if (n > 0) { const double p = L.cdf[i]; num += p * L.sw[i]; den += p; }
    }
    const GzHead *h = gz_head(E);
    const double v_hat = gz_vhat(E)[s.slot];
    const double scale = ((double)h->c_visit + (double)max_n) * (double)h->c_scale;
    const double v_mix = (v_hat + (double)sum_n * (den > 0.0 ? num / den : v_hat)) / (1.0 + (double)sum_n);
    // per child: the logit of the improved policy, and the move-choice score of the most-visited children
    double bx = -INFINITY, bs = -INFINITY;
    float bp = -INFINITY;
    int bs_i = 0x7FFFFFFF, bp_i = 0x7FFFFFFF;
    for (int i = lane; i < nch; i += 64) {
        const int n = L.a_tmp[i];
        const double q = L.sw[i];
        const float p = T.P[first + i];
        const double x = log((double)fmaxf(p, FLT_MIN)) + scale * (((n ? q : v_mix) + 1.0) * 0.5);
        L.w_tmp[i] = x;
        bx = x > bx ? x : bx;
        if (n == max_n) {
            const double sc = rootP[i] + scale * ((q + 1.0) * 0.5);
            if (sc > bs) { bs = sc; bs_i = i; }
        }
        if (p > bp) { bp = p; bp_i = i; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double ox = __shfl_xor(bx, off), os = __shfl_xor(bs, off);
        const float op = __shfl_xor(bp, off);
        const int osi = __shfl_xor(bs_i, off), opi = __shfl_xor(bp_i, off);
        bx = ox > bx ? ox : bx;
        if (os > bs || (os == bs && osi < bs_i)) { bs = os; bs_i = osi; }
        if (op > bp || (op == bp && opi < bp_i)) { bp = op; bp_i = opi; }
    }
    bs_i = __builtin_amdgcn_readfirstlane(bs_i);
    bp_i = __builtin_amdgcn_readfirstlane(bp_i);
    if (bs_i == 0x7FFFFFFF) { s.ovf |= 8; bs_i = 0; }             // all-NaN scores
    for (int i = lane; i < nch; i += 64) L.w_tmp[i] = exp(L.w_tmp[i] - bx);
    wave_sync();
    double total = 0.0;
    for (int i = 0; i < nch; ++i) total += L.w_tmp[i];
    for (int i = lane; i < nch; i += 64) {
        ((xq_sample *)rec)->actions[i] = T.A[first + i];
        ((xq_sample *)rec)->visits[i] = (uint16_t)floor((L.w_tmp[i] / total) * 65535.0 + 0.5);
    }
    considered = (unsigned)min((int)h->m, nch);
    offprior = bs_i != bp_i ? 1u : 0u;
    s.n_samples += 1;
    return __builtin_amdgcn_readfirstlane((int)T.A[first + bs_i]);
}

// The leaf a descent ends on, and the simulated position there (its board and ring are SelectLds.board / .hist)
struct Leaf {
    int node, depth, side, mc, nocap;
};

// One PUCT descent (mcts.py:126-153) from the root, replaying moves on the LDS board; the nodes passed go to path[0 .. depth].
// VL (leaf batching): each in-flight descent through a node counts as a visit and as a loss for the side choosing there (W is
// from the chooser's view): n = N + vl in q and in 1 + n, w = W - vl, parent count N + vl; vl = 0 gives the plain values exactly.
// FORCED: at a root of prior kind 1 a visited child below its minimum share of the root's visits scores +infinity.
// GUMBEL: at a root of prior kind 3 the candidates are the children whose N equals this simulation's considered-visit count
// (the sequential halving); they score rootP[i] = g_i + l_i plus, once visited, sigma(q_i), everyone else -infinity.  sigma needs
// the maximum of the children's N first: one more pass over the (at most 128) counts and one more wave reduction, at that level only.
//
// One dependent round trip to memory per level: every lane reads, with its candidate child's N / W / P, that child's own
// node words (children count + kind, first child, action) as well, so the winner's are already in a register when the arg-max
// is known -- the next level starts from a lane read instead of three more dependent loads (tM -> tC/tN -> ... -> tA).  The
// winner's N, read here, IS the next level's parent count.
template <bool VL, bool FORCED, bool GUMBEL = false>
__device__ __forceinline__ Leaf wave_descend(const Dev &E, Slot &s, SelectLds &L, const int32_t *vl, const double *rootP, float fp_k,
                                             int32_t *path) {
    const Tree &T = s.T;
    const int lane = s.lane;
    lds_copy_dwords(L.board, L.root, XQ_BS / 4);
    lds_copy_dwords(L.hist, L.rhist, XQ_HIST * XQ_BS / 4);
    wave_sync();
    int side = s.side, mc = s.mc, nocap = s.nocap, node = 0, depth = 0;
    if (lane == 0) path[0] = 0;
    int m = __builtin_amdgcn_readfirstlane((int)T.M[0]);
    int first = __builtin_amdgcn_readfirstlane(T.C[0]);
    int pn = __builtin_amdgcn_readfirstlane(VL ? T.N[0] + vl[0] : T.N[0]);
    for (;;) {
        const int nch = m & 0x3FFF, kind = m >> 14;
        if (nch == 0) break;
        const double sqrtp = E.sqrt_tab[pn];
        const float sqrtp_f = (float)sqrtp, c_f = (float)E.cfg.c_puct;
        const double uni = 1.0 / (double)nch;
        double best = -INFINITY;
        int best_i = 0x7FFFFFFF;
        int c_m = 0, c_first = 0, c_n = 0, c_a = 0;              // node words of this lane's best candidate
        double gz_scale = 0.0;                                   // GUMBEL, kind 3: (c_visit + maxN) * c_scale
        int gz_cv = 0;                                           //                 the considered-visit count of this simulation
        if (GUMBEL && kind == 3) {
            int mx = 0;
            for (int i = lane; i < nch; i += 64) mx = max(mx, T.N[first + i]);
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) mx = max(mx, __shfl_xor(mx, off));
            const GzHead *h = gz_head(E);
            const int S = E.cfg.num_simulations, k = min(h->m, nch);
            gz_scale = ((double)h->c_visit + (double)mx) * (double)h->c_scale;
            gz_cv = (int)gz_table(E)[(size_t)(k - 1) * S + min(pn, S - 1)];
        }
        for (int base = 0; base < nch; base += 64) {
            const int i = base + lane;
            if (i < nch) {
                int n = T.N[first + i];
                double w = T.W[first + i];
                if (VL) { const int v = vl[first + i]; n += v; w -= (double)v; }
                const int cm = (int)T.M[first + i], cf = T.C[first + i], ca = (int)T.A[first + i];
                const double q = n ? w / (double)n : 0.0;
                double ucb;
                if (GUMBEL && kind == 3) {
                    ucb = n != gz_cv ? -INFINITY : (gz_cv > 0 ? rootP[i] + gz_scale * ((q + 1.0) * 0.5) : rootP[i]);
                } else if (kind == 0) {
                    float t = c_f * T.P[first + i];
                    t = t * sqrtp_f;
                    t = t / (float)(1 + n);
                    t = (float)q + t;
                    ucb = (double)t;
                } else {
                    const double p = kind == 1 ? rootP[i] : uni;
                    double t = E.cfg.c_puct * p;
                    t = t * sqrtp;
                    t = t / (double)(1 + n);
                    ucb = q + t;
                    if (FORCED && kind == 1 && n > 0 && (double)n * (double)n < ((double)fp_k * p) * (double)pn) ucb = INFINITY;
                }
                if (ucb > best) { best = ucb; best_i = i; c_m = cm; c_first = cf; c_n = n; c_a = ca; }
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const double ov = __shfl_xor(best, off);
            const int oi = __shfl_xor(best_i, off);
            if (ov > best || (ov == best && oi < best_i)) { best = ov; best_i = oi; }
        }
        best_i = __builtin_amdgcn_readfirstlane(best_i);
        if (FORCED && kind == 1 && best == INFINITY) s.d_forced += 1;   // wave-uniform after the reduction
        s.d_scan += (unsigned)nch;
        int action, child;
        if (best_i == 0x7FFFFFFF) {                              // all-NaN scores: the reference would raise
            s.ovf |= 8;
            child = first;
            m = __builtin_amdgcn_readfirstlane((int)T.M[child]);
            pn = __builtin_amdgcn_readfirstlane(VL ? T.N[child] + vl[child] : T.N[child]);
            action = __builtin_amdgcn_readfirstlane((int)T.A[child]);
            first = __builtin_amdgcn_readfirstlane(T.C[child]);
        } else {
            child = first + best_i;
            const int src = best_i & 63;                         // child i was lane i % 64's candidate, and its best (it won)
            action = __builtin_amdgcn_readlane(c_a, src);
            m = __builtin_amdgcn_readlane(c_m, src);
            pn = __builtin_amdgcn_readlane(c_n, src);
            first = __builtin_amdgcn_readlane(c_first, src);
        }
        wave_make_move(L.board, L.hist, action, side, mc, nocap);
        depth += 1;
        if (depth >= E.path_cap) { s.ovf |= 16; depth = E.path_cap - 1; }
        if (lane == 0) path[depth] = child;
        node = child;
    }
    return Leaf{node, depth, side, mc, nocap};
}

// ---------------------------------------------------------------------------------------------------------
// Four independent games per 256-thread workgroup (one per wave, LDS carved per wave, no workgroup barrier anywhere).
// Measured: k_select's time at G = 8192 does not depend on the workgroup shape (0.15 ms either way, 0.04 ms at G = 2048):
// it saturates a CU at ~8 resident games because the leaf's move generation / legality scan is LDS-instruction bound
// (thousands of byte reads of the LDS board per game), not HBM bound.
constexpr int WAVES_PER_WG = 4;

#ifndef XQ_SELECT_WAVES_PER_EU
// 0 = the compiler's choice (240 VGPRs, two waves per SIMD, no spills) -- the shipped setting.  Capping the registers for three / four
// waves per SIMD (168 / 128 VGPRs) was measured: select 0.135 / 0.159 ms instead of 0.177 (near-uniform) and 0.350 / 0.328 instead of 0.364
// (peaked), but the 47 / 94 spilled registers are stored by EVERY wave (12 KB of scratch per game): k_select's HBM-side writes went from
// 47 MB to 146 MB per launch (TCC_EA0_WRREQ).  0.04 ms of a 50 ms step is not worth tripling the kernel's traffic.
#define XQ_SELECT_WAVES_PER_EU 0
#endif
#if XQ_SELECT_WAVES_PER_EU > 0
#define XQ_SELECT_OCC __attribute__((amdgpu_waves_per_eu(XQ_SELECT_WAVES_PER_EU, XQ_SELECT_WAVES_PER_EU)))
#else
// Nothing for the instances without forced playouts (0, 0 emits no attribute).  The FORCED instances are held to the same two
// waves per SIMD: left alone, the two with CAP take 256 VGPRs plus a few AGPRs and halve their occupancy.  Headroom of the
// unpinned instances: <0,1,0> and <1,1,0> stand at 255 of the 256 VGPRs that two waves allow, the others at 244 / 245, so a
// change to a shared helper wants the resource table regenerated (profiles/r12_gumbel_kernel_resource_usage.txt).  The GUMBEL
// instance is held to two waves like the FORCED ones.
#define XQ_SELECT_OCC __attribute__((amdgpu_waves_per_eu((FORCED || GUMBEL) ? 2 : 0, (FORCED || GUMBEL) ? 2 : 0)))
#endif
// REUSE (tree reuse): at the end of a move the chosen child and the old allocation mark are handed to k_reroot and
// k_expand<true> of the same step (GI_RR_NODE / GI_RR_MARK).
// CAP (playout cap randomization, xq_engine_init_cap): every searched position takes one draw of the slot's uniform stream when
// its root request is issued; u < p makes the move FULL (the move without the cap), otherwise FAST: budget S_fast, no root noise
// (k_expand), no sample.  The kind and the budget live in GI_CAP_FULL / GI_CAP_BUDGET from the root request to the move's end.
// FORCED (forced playouts and policy target pruning, xq_engine_init_fp): at a root of prior kind 1 -- the noisy root of a full
// move, always node 0 -- a visited child i with N_i^2 < (k rootP[i]) N_root scores +infinity in the descent (the first maximum
// then takes the lowest-index forced child), and at the move's end the sample's visits and the move-choice weights are the
// PRUNED counts v_i (include/xq_hip.h); the tree keeps its N and W.
// GUMBEL (Gumbel root search with sequential halving, xq_engine_init_gz; one instance, <false, false, false, true>): the root of
// every searched position has prior kind 3 (k_expand<.., .., true>); the descent picks among its equal-visit candidates
// (wave_descend), and a self-play move ends in slot_end_move_gumbel: no temperature, no uniform draw, the improved policy as the
// sample's target.  Every other level is the PUCT of the other instances.
// AROPEN (arena options, xq_engine_init_ar; one instance, <false, false, false, false, true>): a new game starts with its pair's
// random opening (slot_arena_opening).  Everything after it is the arena game of the plain instance.
template <bool REUSE, bool CAP = false, bool FORCED = false, bool GUMBEL = false, bool AROPEN = false>
__global__ __launch_bounds__(64 * WAVES_PER_WG) XQ_SELECT_OCC void k_select(Dev E, float *__restrict__ nn_in) {
    __shared__ SelectLds Ls[WAVES_PER_WG];
    SelectLds &L = Ls[threadIdx.x >> 6];
    const int slot = blockIdx.x * WAVES_PER_WG + (int)(threadIdx.x >> 6);
    if (slot >= E.cfg.n_games) return;
    const int lane = lane_id();
    Slot s;
    s.slot = slot; s.lane = lane; s.gi = E.gi + (size_t)slot * GI_N; s.st = E.stats + (size_t)slot * ST_N; s.T = slot_tree(E, slot);
    int32_t *gi = s.gi;
    const Tree &T = s.T;
    int32_t *path = E.path + (size_t)slot * E.path_cap;
    uint16_t *pmoves = E.pmoves + (size_t)slot * XQ_MAXM;
    float *x = nn_in + (size_t)slot * XQ_STATE_FLOATS;
    const double *rootP = E.rootP + (size_t)slot * XQ_MAXM;
    const int S = E.cfg.num_simulations;
    const bool manual = E.cfg.manual_moves == 1;     // search only (MCTS.search parity / serving)
    const bool arena = E.cfg.manual_moves == 2;      // evaluation games (train.py:453-535): T = 0, no opening, no samples

    int phase = __builtin_amdgcn_readfirstlane(gi[GI_PHASE]);
    if (phase == PH_WAIT_ROOT || phase == PH_WAIT_LEAF) return;        // still waiting: the request stands
    if (phase == PH_IDLE || phase == PH_HOLD) { if (lane == 0) E.req[slot] = 0; return; }
    const int delay = __builtin_amdgcn_readfirstlane(gi[GI_DELAY]);
    if (delay > 0) {                                  // start_stagger: not started yet
        if (lane == 0) { gi[GI_DELAY] = delay - 1; E.req[slot] = 0; }
        return;
    }
    int req_cnt = 0;
    slot_load(s);
    int term_run = 0;
    // CAP: the kind and budget of the move being searched.  A launch never searches a move whose root request it issued
    // itself (PH_NEWPOS ends the launch), so the words read here hold for the whole launch.
    const bool full_move = CAP ? __builtin_amdgcn_readfirstlane(gi[GI_CAP_FULL]) != 0 : true;
    const int budget = CAP ? __builtin_amdgcn_readfirstlane(gi[GI_CAP_BUDGET]) : S;
    unsigned long long d_fast_moves = 0, d_fast_sims = 0;
    // FORCED: k, a float32 widened at every use
    const float fp_k = FORCED ? __int_as_float(__builtin_amdgcn_readfirstlane(gi[GI_FP_K])) : 0.0f;
    unsigned d_gz_moves = 0, d_gz_cons = 0, d_gz_off = 0;      // GUMBEL only

    lds_copy_dwords(L.root, E.board + (size_t)slot * XQ_BS, XQ_BS / 4);
    lds_copy_dwords(L.rhist, E.hist + (size_t)slot * XQ_HIST * XQ_BS, XQ_HIST * XQ_BS / 4);
    wave_sync();

    for (int guard = 0; guard < 4 * S + 64; ++guard) {
        if (phase == PH_FINISHED) {
            slot_flush_finished(E, s);
            phase = PH_NEWGAME;
        }
        if (phase == PH_NEWGAME) {
            if (!slot_new_game(E, s, L, arena)) { phase = PH_IDLE; break; }
            if (AROPEN) slot_arena_opening(E, s, L);
            if (REUSE && lane == 0) gi[GI_RR_NODE] = 0;     // a new game never sees a hand-off
            phase = PH_NEWPOS;
        }
        if (phase == PH_NEWPOS) {
            int status;
            req_cnt = slot_root_request(E, s, L, manual, arena, x, pmoves, status);
            if (REUSE && lane == 0) gi[GI_RR_DROP] = 0;      // this move's tree is grown under the current weights
            if (CAP) {
                // the cap draw: one uniform per position that will be searched, ahead of that move's move-choice draw
                bool full = true;
                if (status == 0) {
                    const double u = u64_to_unit(draw_u64(E, slot, RNG_UNIFORM, s.rng_ctr[RNG_UNIFORM], s.st));
                    s.rng_ctr[RNG_UNIFORM] += 1;
                    const unsigned long long pb = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane(gi[GI_CAP_PHI]) << 32) |
                                                  (unsigned)__builtin_amdgcn_readfirstlane(gi[GI_CAP_PLO]);
                    full = u < __longlong_as_double((long long)pb);
                }
                const int sfast = __builtin_amdgcn_readfirstlane(gi[GI_CAP_SFAST]);
                if (lane == 0) { gi[GI_CAP_FULL] = full ? 1 : 0; gi[GI_CAP_BUDGET] = full ? S : sfast; }
            }
            phase = PH_WAIT_ROOT;
            break;
        }
        // ---- phase == PH_SEARCH
        if (s.sims_done >= budget) {
            if (manual) { phase = PH_HOLD; break; }
            const int nch = __builtin_amdgcn_readfirstlane((int)(T.M[0] & 0x3FFF));
            const int first = __builtin_amdgcn_readfirstlane(T.C[0]);
            phase = PH_NEWPOS;
            if (arena) { slot_arena_move(s, L, nch, first); continue; }
            if (GUMBEL && (__builtin_amdgcn_readfirstlane((int)T.M[0]) >> 14) == 3) {
                unsigned cons, off;
                const int action = slot_end_move_gumbel(E, s, L, rootP, nch, first, cons, off);
                d_gz_moves += 1; d_gz_cons += cons; d_gz_off += off;
                slot_play(s, L, action);
                continue;
            }
            const bool pruned = FORCED && (__builtin_amdgcn_readfirstlane((int)T.M[0]) >> 14) == 1;
            if (pruned) wave_prune_visits(E, s, L, rootP, fp_k, nch, first);
            const int action = slot_end_move(E, s, L, full_move, pruned, nch, first);
            if (REUSE) {
                // hand the chosen child c to k_reroot / k_expand<true> of this step when it was expanded and no drop
                // (xq_engine_drop_reroots) ran since this move began; L.a_tmp[i] is child i's action
                int c = 0;
                for (int base = 0; base < nch; base += 64) {
                    const unsigned long long b = __ballot(base + lane < nch && (int)L.a_tmp[base + lane] == action);
                    if (b) { c = first + base + (int)__builtin_ctzll(b); break; }
                }
                c = __builtin_amdgcn_readfirstlane(c);
                const bool keep = c > 0 && __builtin_amdgcn_readfirstlane(T.C[c]) >= 0 &&
                                  __builtin_amdgcn_readfirstlane(gi[GI_RR_DROP]) == 0;
                if (lane == 0) { gi[GI_RR_NODE] = keep ? c : 0; gi[GI_RR_MARK] = keep ? gi[GI_ALLOC] : 0; }
            }
            slot_play(s, L, action);
            if (CAP && !full_move) d_fast_moves += 1;
            continue;
        }
        const Leaf lf = wave_descend<false, FORCED, GUMBEL>(E, s, L, nullptr, rootP, fp_k, path);
        s.d_depth += (unsigned)lf.depth;
        int cnt, winner;
        const bool term = wave_game_over(L.board, L.hist, lf.side, lf.mc, lf.nocap, L.mg, L.moves, &cnt, &winner, &s.ovf);
        if (term) {
            wave_sync_mem();   // path[] stores of lane 0 must be visible to the other lanes
            wave_backup<false>(T, nullptr, path, lf.depth, winner == 0 ? 0.0 : 1.0);   // mcts.py:137-140
            wave_sync_mem();   // the next descent reads N/W written here by other lanes
            s.sims_done += 1; s.d_sims += 1; s.d_term += 1;
            if (CAP && !full_move) d_fast_sims += 1;
            // A root with a mating reply re-tests that terminal child on every visit (as mcts.py does); bound how
            // many such simulations one launch runs so a single slot cannot stretch the step (it resumes next step
            // and hands the evaluator no position this time).
            if (++term_run >= 48) break;
            continue;
        }
        wave_encode(L.board, lf.side, x);
        for (int j = lane; j < cnt; j += 64) pmoves[j] = L.moves[j];
        if (lane == 0) { gi[GI_PLEAF] = lf.node; gi[GI_PDEPTH] = lf.depth; gi[GI_PCOUNT] = cnt; }
        req_cnt = cnt;
        phase = PH_WAIT_LEAF;
        break;
    }

    slot_store(E, s, L, phase);
    if (lane == 0) {
        E.req[slot] = (phase == PH_WAIT_ROOT || phase == PH_WAIT_LEAF) ? req_cnt : 0;
        if (CAP) { s.st[ST_FASTM] += d_fast_moves; s.st[ST_FASTS] += d_fast_sims; }
        if (FORCED) { s.st[ST_FORCED] += s.d_forced; s.st[ST_PRUNEDV] += s.d_prunedv; s.st[ST_PRUNEDC] += s.d_prunedc; }
        if (GUMBEL) { s.st[ST_GZ_MOVES] += d_gz_moves; s.st[ST_GZ_CONS] += d_gz_cons; s.st[ST_GZ_OFF] += d_gz_off; }
    }
}

// ---------------------------------------------------------------------------------------------------------
// The pieces of the expand kernels (k_expand<REUSE, CAP> and k_expand_multi), one copy each.
struct ExpandLds {
    float p[XQ_MAXM];
    double eta[XQ_MAXM];
    uint16_t act[XQ_MAXM];
};

// A root's evaluation has arrived: the resign probe on the position after the move (parallel_selfplay.py:110-121), then the
// position's own terminal status.  True: the game (a manual search: the slot) ends here and the root is not expanded.
__device__ __forceinline__ bool expand_root_finish(const Dev &E, int32_t *gi, unsigned long long *st, int slot, double v_net) {
    const int lane = lane_id();
    const bool manual = E.cfg.manual_moves == 1, arena = E.cfg.manual_moves == 2;
    if (lane == 0) st[ST_ROOT] += 1;
    const int side = gi[GI_SIDE];
    int fin = 0, fwinner = 0, freason = 0;
    if (!manual && !arena && E.cfg.enable_resign && gi[GI_NSAMP] > 10) {
        const int K = E.cfg.resign_check_steps;
        double *rh = E.resign + (size_t)slot * 16;
        int rn = gi[GI_RESIGN_N];
        wave_sync_mem();
        if (lane == 0) { rh[rn % 16] = v_net; gi[GI_RESIGN_N] = rn + 1; }
        wave_sync_mem();
        rn += 1;
        if (rn >= K) {
            bool all_low = true;
            for (int i = rn - K; i < rn; ++i) all_low = all_low && (rh[i % 16] < E.cfg.resign_threshold);
            if (all_low) { fin = 1; fwinner = -side; freason = 3; }
        }
    }
    const int rstatus = gi[GI_RSTATUS];
    if (!fin && rstatus != 0) { fin = 1; fwinner = gi[GI_RWINNER]; freason = rstatus; }
    fin = __builtin_amdgcn_readfirstlane(fin);
    if (fin && lane == 0) {
        gi[GI_FWINNER] = fwinner; gi[GI_FREASON] = freason;
        gi[GI_PHASE] = manual ? PH_HOLD : PH_FINISHED;
    }
    return fin != 0;
}

// Unnormalised priors of the cnt legal moves into L.p (their actions into L.act): softmax over ALL 8100 logits (model.py:122),
// to be normalised as mcts.py:176-188 by the returned builtin sum() (sequential float32, move order).
// is_probs: 0 logits over all 8100 actions, 1 probabilities over all 8100, 2 logits of the legal moves only
// ([XQ_MAXM], move order): softmax over the legal logits -- the common factor of the full softmax cancels in
// mcts.py:176-188's renormalisation
__device__ __forceinline__ float wave_priors(ExpandLds &L, const float *pol, const uint16_t *pmoves, int cnt, int is_probs) {
    const int lane = lane_id();
    float mx = 0.0f, den = 1.0f;
    if (is_probs == 2) {
        float m = -INFINITY;
        for (int i = lane; i < cnt; i += 64) m = fmaxf(m, pol[i]);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
        mx = m;
    } else if (!is_probs) {
        const float4 *p4 = (const float4 *)pol;
        float m = -INFINITY;
        for (int i = lane; i < XQ_ACTION_SPACE / 4; i += 64) {
            const float4 x = p4[i];
            m = fmaxf(fmaxf(m, fmaxf(x.x, x.y)), fmaxf(x.z, x.w));
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
        float s = 0.0f;
        for (int i = lane; i < XQ_ACTION_SPACE / 4; i += 64) {
            const float4 x = p4[i];
            s += expf(x.x - m) + expf(x.y - m) + expf(x.z - m) + expf(x.w - m);
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
        mx = m; den = s;
    }
    for (int i = lane; i < cnt; i += 64) {
        const int a = pmoves[i];
        const float x = pol[is_probs == 2 ? i : a];
        L.p[i] = is_probs == 1 ? x : expf(x - mx) / den;
        L.act[i] = (uint16_t)a;
    }
    wave_sync();
    float sum = 0.0f;
    for (int i = 0; i < cnt; ++i) sum = sum + L.p[i];
    return sum;
}

// eta ~ Dirichlet(alpha) over the legal moves, in move order, into L.eta (mcts.py:117-121); or the noise set by hand
__device__ __forceinline__ void wave_root_noise(const Dev &E, ExpandLds &L, int32_t *gi, unsigned long long *st, int slot, int cnt) {
    const int lane = lane_id();
    if (gi[GI_MANNOISE] != 0) {
        const double *mn = E.mnoise + (size_t)slot * XQ_MAXM;
        for (int i = lane; i < cnt; i += 64) L.eta[i] = mn[i];
    } else {
        const int ctr0 = gi[GI_RNG0 + RNG_DIRICHLET];
        for (int i = lane; i < cnt; i += 64) {
            double g;
            if (E.cfg.inject_len > 0) {           // tests/draws.py Draws.dirichlet: w = (1 + (u>>40)%4096)^3
                const double w = (double)(1 + (int)((draw_u64(E, slot, RNG_DIRICHLET, ctr0 + i, st) >> 40) % 4096ull));
                g = w * w * w;
            } else {
                g = gamma_variate(E, slot, ctr0 + i, E.cfg.dirichlet_alpha);
            }
            L.eta[i] = g;
        }
        wave_sync();
        double tot = 0.0;
        for (int i = 0; i < cnt; ++i) tot += L.eta[i];
        wave_sync();
        for (int i = lane; i < cnt; i += 64) L.eta[i] = L.eta[i] / tot;
        if (lane == 0) gi[GI_RNG0 + RNG_DIRICHLET] = ctr0 + cnt;
    }
    wave_sync();
}

// The float32 priors of the children at tP[0 .. cnt) and, at a noisy root, the float64 mixed priors in rootP.  Returns the
// node's prior kind: 0 float32 priors, 1 rootP, 2 uniform (the network gave the legal moves no mass).
__device__ __forceinline__ int wave_write_priors(const Dev &E, const ExpandLds &L, float *tP, double *rootP, int cnt, float sum,
                                                 bool noisy) {
    const int lane = lane_id();
    const double eps = E.cfg.noise_eps;
    const float keep_f = (float)(1.0 - eps);
    if (sum > 0.0f) {
        for (int i = lane; i < cnt; i += 64) {
            const float pr = L.p[i] / sum;
            if (noisy) { const float sc = keep_f * pr; rootP[i] = (double)sc + eps * L.eta[i]; }
            tP[i] = pr;
        }
        return noisy ? 1 : 0;
    }
    const double uni = 1.0 / (double)cnt;
    for (int i = lane; i < cnt; i += 64) {
        if (noisy) rootP[i] = (1.0 - eps) * uni + eps * L.eta[i];
        tP[i] = (float)uni;
    }
    return noisy ? 1 : 2;
}

// GUMBEL root: rootP[i] = g_i + l_i over the float32 priors this lane wrote to tP just before (wave_write_priors, the same
// lane-to-child map), l_i = log((double)max(tP[i], FLT_MIN)), g_i one Gumbel(0, 1) draw per legal move from the slot's Dirichlet
// stream (or the values set by hand).  The root's network value is kept for the end of the move.
__device__ __forceinline__ void wave_gumbel_root(const Dev &E, int32_t *gi, unsigned long long *st, int slot, const float *tP,
                                                 double *rootP, int cnt, double v_net) {
    const int lane = lane_id();
    const bool by_hand = gi[GI_MANNOISE] != 0;
    const double *mn = E.mnoise + (size_t)slot * XQ_MAXM;
    const int ctr0 = gi[GI_RNG0 + RNG_DIRICHLET];
    for (int i = lane; i < cnt; i += 64) {
        double g;
        if (by_hand) {
            g = mn[i];
        } else {
            const uint64_t x = draw_u64(E, slot, RNG_DIRICHLET, ctr0 + i, st);
            if (E.cfg.inject_len > 0) g = ((double)(int)((x >> 40) % 4096ull) - 1024.0) / 512.0;   // exact: no transcendental
            else g = -log(-log(((double)(x >> 11) + 0.5) * (1.0 / 9007199254740992.0)));
        }
        rootP[i] = g + log((double)fmaxf(tP[i], FLT_MIN));
    }
    if (lane == 0) {
        if (!by_hand) gi[GI_RNG0 + RNG_DIRICHLET] = ctr0 + cnt;
        gz_vhat(E)[slot] = v_net;
    }
}

// fresh children of `node` at [first, first + cnt), in move order
__device__ __forceinline__ void wave_new_children(const Tree &T, const ExpandLds &L, unsigned long long *st, int node, int first,
                                                  int cnt, int kind) {
    const int lane = lane_id();
    for (int i = lane; i < cnt; i += 64) {
        T.N[first + i] = 0; T.W[first + i] = 0.0; T.A[first + i] = L.act[i]; T.C[first + i] = -1; T.M[first + i] = 0;
    }
    if (lane == 0) {
        T.C[node] = first; T.M[node] = (uint16_t)(cnt | (kind << 14));
        st[ST_NODES] += (unsigned)cnt;
    }
}

// one game per 64-thread workgroup: this kernel streams 32 KB of logits per game and measured faster with more,
// smaller workgroups in flight (0.111 vs 0.132 ms at G = 8192) than with four games per workgroup
// REUSE (k_expand<true>): a root request of a slot that k_select<true> handed a chosen child to (GI_RR_NODE; k_reroot has moved
// that child's subtree to the front of the arena) keeps the children, their N, W, first-child and meta words, rewrites their
// float32 priors, draws fresh noise into rootP and starts the search at sims_done = root N = the sum of their visits.
// CAP (k_expand<.., true>): the root of a fast move (GI_CAP_FULL == 0) takes the no-noise path: no Dirichlet draw, rootP unused,
// prior kind 0 (or 2), also when it is a reused root; a leaf backed up under a fast move counts in ST_FASTS.
// GUMBEL (k_expand<false, false, true>): a root never takes Dirichlet noise; it gets prior kind 3 and rootP = g + l.
template <bool REUSE, bool CAP = false, bool GUMBEL = false>
__global__ __launch_bounds__(64) void k_expand(Dev E, const float *__restrict__ policy, const float *__restrict__ value,
                                               int is_probs) {
    __shared__ ExpandLds L;
    const int slot = blockIdx.x;
    if (slot >= E.cfg.n_games) return;
    const int lane = lane_id();
    int32_t *gi = E.gi + (size_t)slot * GI_N;
    unsigned long long *st = E.stats + (size_t)slot * ST_N;
    int phase = __builtin_amdgcn_readfirstlane(gi[GI_PHASE]);
    if (phase != PH_WAIT_ROOT && phase != PH_WAIT_LEAF) return;
    const Tree T = slot_tree(E, slot);
    const int32_t *path = E.path + (size_t)slot * E.path_cap;
    const uint16_t *pmoves = E.pmoves + (size_t)slot * XQ_MAXM;
    double *rootP = E.rootP + (size_t)slot * XQ_MAXM;
    const bool manual = E.cfg.manual_moves == 1;
    const bool is_root = phase == PH_WAIT_ROOT;
    const double v_net = (double)value[slot];        // tensor.item(): float32 widened
    const int cnt = __builtin_amdgcn_readfirstlane(gi[GI_PCOUNT]);
    int sims_done = __builtin_amdgcn_readfirstlane(gi[GI_SIMS]);
    int ovf = 0;
    int rr = 0;                                       // REUSE: the re-rooted child of this step's hand-off (0: none)

    if (is_root) {
        if (REUSE) {
            rr = __builtin_amdgcn_readfirstlane(gi[GI_RR_NODE]);
            // consumed: a hand-off lives for one step.  The store depends on rr: the word is read by a scalar load, and a
            // vector store issued before that load returns could overtake it (the load would then see the cleared word)
            if (rr != 0 && lane == 0) gi[GI_RR_NODE] = 0;
        }
        if (expand_root_finish(E, gi, st, slot, v_net)) return;
    } else {
        if (lane == 0) st[ST_LEAF] += 1;
    }

    const float sum = wave_priors(L, policy + (size_t)slot * (is_probs == 2 ? XQ_MAXM : XQ_ACTION_SPACE), pmoves, cnt, is_probs);
    const bool full_move = CAP ? __builtin_amdgcn_readfirstlane(gi[GI_CAP_FULL]) != 0 : true;
    const bool noisy = !GUMBEL && is_root && full_move && (E.cfg.add_noise != 0 || gi[GI_MANNOISE] != 0);
    if (noisy) wave_root_noise(E, L, gi, st, slot, cnt);

    const int node = is_root ? 0 : __builtin_amdgcn_readfirstlane(gi[GI_PLEAF]);
    int first = __builtin_amdgcn_readfirstlane(gi[GI_ALLOC]);
    bool reused = false;
    int root_sims = 0;                                // the search's first sims_done: 0, or the reused root's visits
    if (REUSE && rr > 0) {
        // node 0 holds the chosen child's words (k_reroot); its children must be this position's legal moves
        const int m0 = __builtin_amdgcn_readfirstlane((int)T.M[0]), f0 = __builtin_amdgcn_readfirstlane(T.C[0]);
        reused = cnt > 0 && (m0 & 0x3FFF) == cnt && f0 >= 1 && f0 + cnt <= E.node_cap;
        if (reused) {
            first = f0;
        } else {                                      // a defect: reported, and the root is expanded afresh
            ovf |= 64;
            if (lane == 0) { T.N[0] = 0; T.W[0] = 0.0; }
        }
    }
    if (cnt > 0) {
        if (first + cnt > E.node_cap) {
            ovf |= 32;
        } else {
            int kind = wave_write_priors(E, L, T.P + first, rootP, cnt, sum, noisy);
            if (GUMBEL && is_root) {
                wave_gumbel_root(E, gi, st, slot, T.P + first, rootP, cnt, v_net);
                kind = 3;
            }
            if (REUSE && reused) {
                // the kept children keep N, W, action, first child and meta; the budget is visits: sims_done = root N = sum N
                int vis = 0, bad = 0;
                for (int i = lane; i < cnt; i += 64) {
                    vis += T.N[first + i];
                    bad |= T.A[first + i] != L.act[i];
                }
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) { vis += __shfl_xor(vis, off); bad |= __shfl_xor(bad, off); }
                root_sims = __builtin_amdgcn_readfirstlane(vis);
                if (__builtin_amdgcn_readfirstlane(bad)) ovf |= 64;
                if (lane == 0) {
                    T.M[0] = (uint16_t)(cnt | (kind << 14)); T.N[0] = root_sims;
                    st[ST_REUSED] += (unsigned)root_sims; st[ST_REROOTS] += 1;
                }
            } else {
                wave_new_children(T, L, st, node, first, cnt, kind);
                if (lane == 0) gi[GI_ALLOC] = first + cnt;
            }
        }
    }
    if (is_root) {
        if (lane == 0) { gi[GI_PHASE] = PH_SEARCH; gi[GI_SIMS] = root_sims; if (ovf) st[ST_OVF] |= (unsigned long long)ovf << 8; }
        return;
    }
    // ---- leaf: value = -v (mcts.py:150), backup
    const int depth = __builtin_amdgcn_readfirstlane(gi[GI_PDEPTH]);
    wave_sync_mem();
    wave_backup<false>(T, nullptr, path, depth, -v_net);
    sims_done += 1;
    if (lane == 0) {
        gi[GI_SIMS] = sims_done;
        gi[GI_PHASE] = (manual && sims_done >= E.cfg.num_simulations) ? PH_HOLD : PH_SEARCH;
        st[ST_SIMS] += 1;
        if (CAP && !full_move) st[ST_FASTS] += 1;
        if (ovf) st[ST_OVF] |= (unsigned long long)ovf << 8;
    }
}

// ---------------------------------------------------------------------------------------------------------
// Tree reuse (xq_engine_init_ex, XQ_ENGINE_TREE_REUSE): k_reroot moves the subtree of the chosen child c that k_select<true>
// handed over (GI_RR_NODE, with the old allocation mark GI_RR_MARK) to the front of the slot's arena, in place.
//   * [1, mark) is the child blocks laid end to end in allocation order, and a block is allocated when its parent is expanded:
//     allocation order is topological, every kept node lies after its parent and c's children block is the first kept one.
//   * The kept nodes are c's descendants (whole blocks), marked level by level from c in an LDS bitmap over [0, mark).  A kept
//     node's new index is 1 + the number of kept nodes before it (per-word prefix counts); c's words go to node 0.  This stable
//     compaction moves every kept node to an index below its old one, so an ascending copy whose chunks read everything into
//     registers and pass a barrier before writing never overwrites a word that is still to be read.
// The tree is validated before the first write: a malformed one drops the hand-off (k_expand<true> then expands a fresh root)
// and sets overflow bit 64 << 8.  LDS atomics only build the bitmap and the level queue, whose order does not change the
// result.  One 256-thread workgroup per slot (grid G: the step stays one graph); slots without a hand-off exit at once.
constexpr int RR_THREADS = 256, RR_PER_THREAD = 4;

// dynamic LDS of k_reroot: bitmap and prefix words over node_cap, and the level queue of kept expanded nodes (at most S + 1)
size_t reroot_lds_bytes(int node_cap, int num_simulations) {
    return ((size_t)2 * ((node_cap + 31) / 32) + (size_t)num_simulations + 2) * 4;
}

__global__ __launch_bounds__(RR_THREADS) void k_reroot(Dev E) {
    extern __shared__ uint32_t rr_lds[];
    __shared__ int s_tail, s_bad, s_wsum[RR_THREADS / 64];
    const int slot = blockIdx.x;
    if (slot >= E.cfg.n_games) return;
    int32_t *gi = E.gi + (size_t)slot * GI_N;
    const int c = __builtin_amdgcn_readfirstlane(gi[GI_RR_NODE]);
    if (c <= 0) return;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    unsigned long long *st = E.stats + (size_t)slot * ST_N;
    const size_t nb = (size_t)slot * E.node_cap;
    int32_t *tN = E.tN + nb; double *tW = E.tW + nb; float *tP = E.tP + nb;
    uint16_t *tA = E.tA + nb; int32_t *tC = E.tC + nb; uint16_t *tM = E.tM + nb;
    const int mark = __builtin_amdgcn_readfirstlane(gi[GI_RR_MARK]);
    const int nw = (E.node_cap + 31) >> 5, qcap = E.cfg.num_simulations + 2;
    uint32_t *bits = rr_lds;                          // [nw]   kept-node bitmap
    int32_t *pre = (int32_t *)(rr_lds + nw);          // [nw]   kept nodes before each bitmap word
    int32_t *q = pre + nw;                            // [qcap] kept expanded nodes, level after level

    // c's words first: its index may be a destination of the compaction
    const bool c_in = c < mark && mark <= E.node_cap;
    const int cN = c_in ? tN[c] : 0, cF = c_in ? tC[c] : -1, cM = c_in ? (int)tM[c] : 0;
    const double cW = c_in ? tW[c] : 0.0;
    const float cP = c_in ? tP[c] : 0.0f;
    const uint16_t cA = c_in ? tA[c] : 0;
    if (!(c_in && cF > c && (cM & 0x3FFF) > 0 && cF + (cM & 0x3FFF) <= mark)) {
        if (t == 0) { gi[GI_RR_NODE] = 0; st[ST_OVF] |= 64ull << 8; }
        return;
    }
    const int mw = (mark + 31) >> 5;
    for (int w = t; w < mw; w += RR_THREADS) bits[w] = 0u;
    if (t == 0) { q[0] = c; s_tail = 1; s_bad = 0; }
    __syncthreads();
    // ---- mark c's descendants: level by level, the children blocks of the queue entries [lo, hi), one wave per entry
    int lo = 0, hi = 1;
    while (lo < hi) {
        for (int e = lo + wave; e < hi; e += RR_THREADS / 64) {
            const int x = q[e];
            const int f = tC[x], n = tM[x] & 0x3FFF;
            if (!(f > x && n > 0 && f + n <= mark)) { s_bad = 1; continue; }
            for (int i = lane; i < n; i += 64) {
                const int y = f + i;
                atomicOr(&bits[y >> 5], 1u << (y & 31));
                if (tC[y] >= 0) {
                    const int k = atomicAdd(&s_tail, 1);
                    if (k < qcap) q[k] = y; else s_bad = 1;
                }
            }
        }
        __syncthreads();
        lo = hi;
        hi = min(s_tail, qcap);
        __syncthreads();                              // every thread has read s_tail before the next level appends
    }
    if (s_bad) {
        if (t == 0) { gi[GI_RR_NODE] = 0; st[ST_OVF] |= 64ull << 8; }
        return;
    }
    // ---- exclusive prefix of the per-word counts: thread t owns the contiguous words [w0, w1)
    const int per = (mw + RR_THREADS - 1) / RR_THREADS;
    const int w0 = min(t * per, mw), w1 = min(w0 + per, mw);
    int cnt = 0;
    for (int w = w0; w < w1; ++w) cnt += __popc(bits[w]);
    int inc = cnt;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int v = __shfl_up(inc, off);
        if (lane >= off) inc += v;
    }
    if (lane == 63) s_wsum[wave] = inc;
    __syncthreads();
    int base = 0, kept = 0;
#pragma unroll
    for (int w = 0; w < RR_THREADS / 64; ++w) {
        const int v = s_wsum[w];
        base += w < wave ? v : 0;
        kept += v;
    }
    int run = base + inc - cnt;
    for (int w = w0; w < w1; ++w) { pre[w] = run; run += __popc(bits[w]); }
    __syncthreads();
    auto new_index = [&](int x) { return 1 + pre[x >> 5] + __popc(bits[x >> 5] & ((1u << (x & 31)) - 1u)); };
    // ---- ascending copy of [cF, mark): read a chunk into registers, barrier, write it below
    for (int a = cF; a < mark; a += RR_THREADS * RR_PER_THREAD) {
        int dst[RR_PER_THREAD], vN[RR_PER_THREAD], vC[RR_PER_THREAD];
        double vW[RR_PER_THREAD];
        float vP[RR_PER_THREAD];
        uint16_t vA[RR_PER_THREAD], vM[RR_PER_THREAD];
#pragma unroll
        for (int r = 0; r < RR_PER_THREAD; ++r) {
            const int x = a + r * RR_THREADS + t;
            dst[r] = -1; vN[r] = 0; vC[r] = -1; vW[r] = 0.0; vP[r] = 0.0f; vA[r] = 0; vM[r] = 0;
            if (x < mark && ((bits[x >> 5] >> (x & 31)) & 1u)) {
                dst[r] = new_index(x);
                vN[r] = tN[x]; vW[r] = tW[x]; vP[r] = tP[x]; vA[r] = tA[x]; vM[r] = tM[x];
                const int f = tC[x];
                vC[r] = f < 0 ? -1 : new_index(f);
            }
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < RR_PER_THREAD; ++r) {
            const int d = dst[r];
            if (d >= 0) { tN[d] = vN[r]; tW[d] = vW[r]; tP[d] = vP[r]; tA[d] = vA[r]; tC[d] = vC[r]; tM[d] = vM[r]; }
        }
    }
    if (t == 0) {
        tN[0] = cN; tW[0] = cW; tP[0] = cP; tA[0] = cA; tM[0] = (uint16_t)cM; tC[0] = new_index(cF);
        gi[GI_ALLOC] = 1 + kept;
    }
}

// xq_engine_drop_reroots: no slot hands its chosen child over at the end of the move it is searching now
__global__ void k_drop_reroots(Dev E) {
    const int slot = blockIdx.x * blockDim.x + threadIdx.x;
    if (slot < E.cfg.n_games) E.gi[(size_t)slot * GI_N + GI_RR_DROP] = 1;
}

// ---------------------------------------------------------------------------------------------------------
// Leaf batching (xq_engine_init_leaves, K > 1): k_select_multi / k_expand_multi replace k_select / k_expand.  Per step a
// searching slot runs up to K descents under virtual loss (a separate int32 counter per node, never folded into N / W):
// wave_descend<true, ..>.  A descent that chooses a non-terminal leaf adds 1 to vl along its path (the root included) and
// hands the leaf to the evaluator in row slot K + j; a terminal leaf is backed up at once; a descent that ends on a leaf
// already pending in this step (a collision) is dropped and ends the slot's collection.  k_expand_multi expands and backs
// up the pending leaves in descent order and removes each one's virtual loss: every vl is 0 again after every step.
struct Mx {
    int K;                          // leaves per step (2..64)
    int32_t *vl;                    // [G][node_cap] in-flight descents through each node
    int32_t *leaf;                  // [G][K][4] pending leaf j of a slot: node, depth, legal-move count, -
};

// One game per 64-thread workgroup: at the small G where leaf batching pays, each slot's K descents are its step's
// critical path, and a workgroup of its own gives the slot a CU's LDS instead of a quarter of it (k_select: four per CU).
__global__ __launch_bounds__(64) void k_select_multi(Dev E, Mx X, float *__restrict__ nn_in) {
    __shared__ SelectLds L;
    const int slot = blockIdx.x;
    if (slot >= E.cfg.n_games) return;
    const int lane = lane_id();
    Slot s;
    s.slot = slot; s.lane = lane; s.gi = E.gi + (size_t)slot * GI_N; s.st = E.stats + (size_t)slot * ST_N; s.T = slot_tree(E, slot);
    int32_t *gi = s.gi;
    unsigned long long *st = s.st;
    const Tree &T = s.T;
    const int K = X.K;
    const size_t row0 = (size_t)slot * K;                // the slot's first request row; descent j uses row row0 + j
    int32_t *vl = X.vl + (size_t)slot * E.node_cap;
    int32_t *path = E.path + row0 * E.path_cap;
    uint16_t *pmoves = E.pmoves + row0 * XQ_MAXM;
    const double *rootP = E.rootP + (size_t)slot * XQ_MAXM;
    const int S = E.cfg.num_simulations;
    const bool manual = E.cfg.manual_moves == 1;     // search only (MCTS.search parity / serving)
    const bool arena = E.cfg.manual_moves == 2;      // evaluation games: not with K > 1 (leaves_ok)

    int phase = __builtin_amdgcn_readfirstlane(gi[GI_PHASE]);
    if (phase == PH_WAIT_ROOT || phase == PH_WAIT_LEAF) return;        // still waiting: the request stands
    if (phase == PH_IDLE || phase == PH_HOLD) { for (int j = lane; j < K; j += 64) E.req[row0 + j] = 0; return; }
    const int delay = __builtin_amdgcn_readfirstlane(gi[GI_DELAY]);
    if (delay > 0) {                                  // start_stagger: not started yet
        if (lane == 0) gi[GI_DELAY] = delay - 1;
        for (int j = lane; j < K; j += 64) E.req[row0 + j] = 0;
        return;
    }
    slot_load(s);
    int term_run = 0;
    // pending leaves of this step: lane j holds leaf j's node and legal-move count (K <= 64)
    int npend = 0, my_node = -1, my_cnt = 0;
    unsigned long long d_coll = 0;

    lds_copy_dwords(L.root, E.board + (size_t)slot * XQ_BS, XQ_BS / 4);
    lds_copy_dwords(L.rhist, E.hist + (size_t)slot * XQ_HIST * XQ_BS, XQ_HIST * XQ_BS / 4);
    wave_sync();

    for (int guard = 0; guard < 4 * S + 64; ++guard) {
        if (phase == PH_FINISHED) {
            slot_flush_finished(E, s);
            phase = PH_NEWGAME;
        }
        if (phase == PH_NEWGAME) {
            if (!slot_new_game(E, s, L, arena)) { phase = PH_IDLE; break; }
            phase = PH_NEWPOS;
        }
        if (phase == PH_NEWPOS) {
            int status;
            const int cnt = slot_root_request(E, s, L, manual, arena, nn_in + row0 * XQ_STATE_FLOATS, pmoves, status);
            my_cnt = lane == 0 ? cnt : 0;
            phase = PH_WAIT_ROOT;
            break;
        }
        // ---- phase == PH_SEARCH
        // stop collecting: K leaves pending, or the pending leaves complete the move's S simulations
        if (npend > 0 && (npend >= K || s.sims_done + npend >= S)) { phase = PH_WAIT_LEAF; break; }
        if (s.sims_done >= S) {
            if (manual) { phase = PH_HOLD; break; }
            const int nch = __builtin_amdgcn_readfirstlane((int)(T.M[0] & 0x3FFF));
            const int first = __builtin_amdgcn_readfirstlane(T.C[0]);
            if (arena) slot_arena_move(s, L, nch, first);
            else slot_play(s, L, slot_end_move(E, s, L, true, false, nch, first));
            phase = PH_NEWPOS;
            continue;
        }
        int32_t *pathj = path + (size_t)npend * E.path_cap;   // this descent's row (reused after a terminal leaf / collision)
        const Leaf lf = wave_descend<true, false>(E, s, L, vl, rootP, 0.0f, pathj);
        // collision: the descent ended on a leaf an earlier descent of this step already waits on -- it is not a simulation
        // (it added no virtual loss yet) and ends this step's collection
        if (__ballot(lane < npend && my_node == lf.node) != 0ull) { d_coll += 1; phase = PH_WAIT_LEAF; break; }
        s.d_depth += (unsigned)lf.depth;
        int cnt, winner;
        const bool term = wave_game_over(L.board, L.hist, lf.side, lf.mc, lf.nocap, L.mg, L.moves, &cnt, &winner, &s.ovf);
        if (term) {
            wave_sync_mem();   // path[] stores of lane 0 must be visible to the other lanes
            wave_backup<false>(T, nullptr, pathj, lf.depth, winner == 0 ? 0.0 : 1.0);   // mcts.py:137-140
            wave_sync_mem();   // the next descent reads N/W written here by other lanes
            s.sims_done += 1; s.d_sims += 1; s.d_term += 1;
            // the bound on terminal simulations per launch, for k_select's reason
            if (++term_run >= 48) { if (npend > 0) phase = PH_WAIT_LEAF; break; }
            continue;
        }
        // ---- pending leaf j = npend: its request goes to row row0 + j; virtual loss along its path, the root included
        wave_encode(L.board, lf.side, nn_in + (row0 + npend) * XQ_STATE_FLOATS);
        uint16_t *pm = pmoves + (size_t)npend * XQ_MAXM;
        for (int j = lane; j < cnt; j += 64) pm[j] = L.moves[j];
        if (lane == npend) { my_node = lf.node; my_cnt = cnt; }
        if (lane == 0) { int32_t *rec = X.leaf + (row0 + npend) * 4; rec[0] = lf.node; rec[1] = lf.depth; rec[2] = cnt; }
        wave_sync_mem();   // pathj[] stores of lane 0 must be visible to the other lanes
        for (int j = lane; j <= lf.depth; j += 64) vl[pathj[j]] += 1;
        wave_sync_mem();   // the next descent reads vl written here by other lanes
        npend += 1;
    }

    slot_store(E, s, L, phase);
    const int nrows = phase == PH_WAIT_ROOT ? 1 : (phase == PH_WAIT_LEAF ? npend : 0);
    for (int j = lane; j < K; j += 64) E.req[row0 + j] = j < nrows ? my_cnt : 0;
    if (lane == 0) {
        gi[GI_NPEND] = nrows;
        if (phase == PH_WAIT_LEAF) { st[ST_LPS] += (unsigned)npend; st[ST_LSTEPS] += 1; }
        st[ST_COLL] += d_coll;
    }
}

// k_expand for request rows slot K + j: the root (one row, j = 0); the pending leaves j = 0 .. npend-1 expanded (children
// bump-allocated in j order) and backed up in j order
__global__ __launch_bounds__(64) void k_expand_multi(Dev E, Mx X, const float *__restrict__ policy, const float *__restrict__ value,
                                                     int is_probs) {
    __shared__ ExpandLds L;
    const int slot = blockIdx.x;
    if (slot >= E.cfg.n_games) return;
    const int lane = lane_id();
    int32_t *gi = E.gi + (size_t)slot * GI_N;
    unsigned long long *st = E.stats + (size_t)slot * ST_N;
    int phase = __builtin_amdgcn_readfirstlane(gi[GI_PHASE]);
    if (phase != PH_WAIT_ROOT && phase != PH_WAIT_LEAF) return;
    const int K = X.K;
    const size_t row0 = (size_t)slot * K;
    const Tree T = slot_tree(E, slot);
    int32_t *vl = X.vl + (size_t)slot * E.node_cap;
    double *rootP = E.rootP + (size_t)slot * XQ_MAXM;
    const bool manual = E.cfg.manual_moves == 1;
    const bool is_root = phase == PH_WAIT_ROOT;
    const int nrows = is_root ? 1 : __builtin_amdgcn_readfirstlane(gi[GI_NPEND]);
    int sims_done = __builtin_amdgcn_readfirstlane(gi[GI_SIMS]);
    int alloc = __builtin_amdgcn_readfirstlane(gi[GI_ALLOC]);
    int ovf = 0;

    if (is_root && expand_root_finish(E, gi, st, slot, (double)value[row0])) return;

    for (int j = 0; j < nrows; ++j) {
        const size_t row = row0 + j;
        const int32_t *lf = X.leaf + row * 4;
        const int cnt = is_root ? __builtin_amdgcn_readfirstlane(gi[GI_PCOUNT]) : __builtin_amdgcn_readfirstlane(lf[2]);
        wave_sync();       // the previous row's readers of L are done
        const float sum = wave_priors(L, policy + row * (is_probs == 2 ? XQ_MAXM : XQ_ACTION_SPACE), E.pmoves + row * XQ_MAXM, cnt,
                                      is_probs);
        const bool noisy = is_root && (E.cfg.add_noise != 0 || gi[GI_MANNOISE] != 0);
        if (noisy) wave_root_noise(E, L, gi, st, slot, cnt);

        const int node = is_root ? 0 : __builtin_amdgcn_readfirstlane(lf[0]);
        const int first = alloc;
        if (cnt > 0) {
            if (first + cnt > E.node_cap) {
                ovf |= 32;
            } else {
                const int kind = wave_write_priors(E, L, T.P + first, rootP, cnt, sum, noisy);
                wave_new_children(T, L, st, node, first, cnt, kind);
                alloc = first + cnt;
            }
        }
        if (is_root) break;
        // ---- leaf j: value = -v (mcts.py:150), backup along its path, its virtual loss removed
        const double v_net = (double)value[row];
        const int depth = __builtin_amdgcn_readfirstlane(lf[1]);
        wave_sync_mem();
        wave_backup<true>(T, vl, E.path + row * E.path_cap, depth, -v_net);
        wave_sync_mem();   // the next leaf's backup updates nodes of this path from other lanes
    }
    if (lane == 0) gi[GI_ALLOC] = alloc;
    if (is_root) {
        if (lane == 0) { gi[GI_PHASE] = PH_SEARCH; gi[GI_SIMS] = 0; gi[GI_NPEND] = 0; if (ovf) st[ST_OVF] |= (unsigned long long)ovf << 8; }
        return;
    }
    sims_done += nrows;
    if (lane == 0) {
        gi[GI_SIMS] = sims_done;
        gi[GI_NPEND] = 0;
        gi[GI_PHASE] = (manual && sims_done >= E.cfg.num_simulations) ? PH_HOLD : PH_SEARCH;
        st[ST_SIMS] += (unsigned)nrows;
        st[ST_LEAF] += (unsigned)nrows;
        if (ovf) st[ST_OVF] |= (unsigned long long)ovf << 8;
    }
}

__global__ void k_init(Dev E) {
    const int slot = blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= E.cfg.n_games) return;
    int32_t *gi = E.gi + (size_t)slot * GI_N;
    for (int i = 0; i < GI_N; ++i) gi[i] = 0;
    gi[GI_PHASE] = E.cfg.manual_moves == 1 ? PH_HOLD : PH_NEWGAME;
    gi[GI_SIDE] = 1;
    if (E.cfg.start_stagger && E.cfg.manual_moves == 0)
        gi[GI_DELAY] = (int)(philox_u64(E.cfg.seed, (uint32_t)E.cfg.rank, (uint32_t)slot, 7u, 0u, 0u) % (uint64_t)(E.cfg.num_simulations + 1));
    unsigned long long *st = E.stats + (size_t)slot * ST_N;
    for (int i = 0; i < ST_N; ++i) st[i] = 0;
    if (slot == 0) { E.cnt[0] = 0; E.cnt[1] = 0; *E.started = 0; }
}

// xq_engine_init_cap: the playout cap's parameters, after k_init, in free state words of every slot (the handle and the config
// struct are full): S_fast and the float64 threshold p as two words.  The kernels read them with their other scalar loads.
__global__ void k_init_cap(Dev E, int fast_simulations, double full_search_prob) {
    const int slot = blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= E.cfg.n_games) return;
    int32_t *gi = E.gi + (size_t)slot * GI_N;
    const unsigned long long pb = (unsigned long long)__double_as_longlong(full_search_prob);
    gi[GI_CAP_FULL] = 1; gi[GI_CAP_BUDGET] = E.cfg.num_simulations;
    gi[GI_CAP_SFAST] = fast_simulations; gi[GI_CAP_PLO] = (int32_t)(uint32_t)pb; gi[GI_CAP_PHI] = (int32_t)(uint32_t)(pb >> 32);
}

// xq_engine_init_fp: the forced-playout parameter k, rounded to float32 by the host, in the last free state word of every slot.
__global__ void k_init_fp(Dev E, float k) {
    const int slot = blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= E.cfg.n_games) return;
    E.gi[(size_t)slot * GI_N + GI_FP_K] = __float_as_int(k);
}

// Column sums of the per-slot counters [G][ST_N] (OR for the overflow word): each 256-thread block sweeps slot rows
// (8 rows x 32 columns per pass, 256 contiguous bytes per row), folds its eight partial rows through LDS and adds the
// result to the zeroed output with one atomic per column.
__global__ __launch_bounds__(256) void k_reduce_stats(Dev E, unsigned long long *out) {
    __shared__ unsigned long long part[8][ST_N];
    const int col = threadIdx.x & (ST_N - 1), row = threadIdx.x >> 5;
    unsigned long long acc = 0;
    for (int s = blockIdx.x * 8 + row; s < E.cfg.n_games; s += gridDim.x * 8) {
        const unsigned long long v = E.stats[(size_t)s * ST_N + col];
        acc = (col == ST_OVF) ? (acc | v) : (acc + v);
    }
    part[row][col] = acc;
    __syncthreads();
    if (row == 0) {
#pragma unroll
        for (int r = 1; r < 8; ++r) acc = (col == ST_OVF) ? (acc | part[r][col]) : (acc + part[r][col]);
        if (col == ST_OVF) atomicOr(&out[col], acc); else atomicAdd(&out[col], acc);
    }
}

// ---------------------------------------------------------------------------------------------------------
// Packed step (xq_engine_compact / xq_engine_expand_packed): the evaluator sees only the slots that asked for an
// evaluation, packed to the front of engine-owned buffers in slot order.  The predicate is k_expand's own (phase
// WAIT_ROOT / WAIT_LEAF after select), so the two kernels cannot disagree about which slots need output.

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

__global__ __launch_bounds__(CPT) void k_compact(Dev E, int32_t *__restrict__ n_live, int32_t *__restrict__ rows) {
    block_compact(E, E.cfg.n_games, [&](int s) { return slot_waits(E, s); }, n_live, rows);
}

// Gather of the packed rows: one workgroup per row of the capacity, rows past *n_live exit.  Per row the 5 400-byte
// planes (8-byte aligned: float2), the 256-byte ordered move list and its count.
__global__ __launch_bounds__(256) void k_gather_rows(Dev E, const int32_t *__restrict__ n_live, const int32_t *__restrict__ rows,
                                                     const float *__restrict__ nn_in, float *__restrict__ x, uint16_t *__restrict__ moves,
                                                     int32_t *__restrict__ counts) {
    const int r = blockIdx.x;
    if (r >= *n_live) return;
    const int slot = rows[r], t = threadIdx.x;
    const float2 *src = (const float2 *)(nn_in + (size_t)slot * XQ_STATE_FLOATS);
    float2 *dst = (float2 *)(x + (size_t)r * XQ_STATE_FLOATS);
    for (int i = t; i < XQ_STATE_FLOATS / 2; i += 256) dst[i] = src[i];
    if (t < XQ_MAXM / 2)
        ((uint32_t *)(moves + (size_t)r * XQ_MAXM))[t] = ((const uint32_t *)(E.pmoves + (size_t)slot * XQ_MAXM))[t];
    if (t == 0) counts[r] = E.req[slot];
}

// Hand-back: packed row r's legal-move logits and value go to slot rows[r] of the slot-ordered buffers k_expand reads.
// One wave per row (two floats per lane), four rows per workgroup.
__global__ __launch_bounds__(256) void k_scatter_rows(const int32_t *__restrict__ n_live, const int32_t *__restrict__ rows,
                                                      const float *__restrict__ logits, const float *__restrict__ value,
                                                      float *__restrict__ slot_logits, float *__restrict__ slot_value, int G) {
    const int r = blockIdx.x * 4 + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= G || r >= *n_live) return;
    const int slot = rows[r];
    ((float2 *)(slot_logits + (size_t)slot * XQ_MAXM))[lane] = ((const float2 *)(logits + (size_t)r * XQ_MAXM))[lane];
    if (lane == 0) slot_value[slot] = value[r];
}

// Leaf batching (K > 1): k_compact over the G K request rows, slot-major.  Row slot K + j is live when the slot waits and
// j < its request-row count (1 for a root, the pending leaves for a leaf step); rows[r] is then that ROW's index, so
// k_gather_rows / k_scatter_rows serve it unchanged over the row-indexed request buffers.
__global__ __launch_bounds__(CPT) void k_compact_multi(Dev E, int K, int32_t *__restrict__ n_live, int32_t *__restrict__ rows) {
    block_compact(E, E.cfg.n_games * K, [&](int r) { return slot_waits(E, r / K) && (r % K) < E.gi[(size_t)(r / K) * GI_N + GI_NPEND]; },
                  n_live, rows);
}

// Per-model packed step of an arena-options engine (xq_engine_compact_arena): ONE pass of one workgroup compacts the waiting slots
// twice, into set 0 (the slots the NEW model searches for) and set 1 (the OLD model's).  Slot s is the new model's iff
// ((first_game + s) even) == (red is to move in the slot's real game).  Every waiting slot is in exactly one set.
struct ArSets {
    const ArHead *head;             // first_game is read on the device: the handle has no word left for it
    int32_t *n_live;                // [2]
    int32_t *rows[2];
    float *x[2];
    uint16_t *moves[2];
    int32_t *counts[2];
};

__device__ __forceinline__ bool slot_is_new_models(const Dev &E, int first_game, int slot) {
    return (((first_game + slot) & 1) == 0) == (E.gi[(size_t)slot * GI_N + GI_SIDE] == 1);
}

__global__ __launch_bounds__(CPT) void k_compact_arena(Dev E, ArSets A) {
    const int first_game = A.head->first_game;
    block_compact(E, E.cfg.n_games, [&](int s) { return slot_waits(E, s) && slot_is_new_models(E, first_game, s); }, A.n_live,
                  A.rows[0]);
    __syncthreads();                                  // block_compact's scan scratch is read by every thread before it is reused
    block_compact(E, E.cfg.n_games, [&](int s) { return slot_waits(E, s) && !slot_is_new_models(E, first_game, s); }, A.n_live + 1,
                  A.rows[1]);
}

size_t align_up(size_t x) { return (x + 255) & ~(size_t)255; }

// ---------------------------------------------------------------------------------------------------------
// Evaluation cache (xq_evcache_*, opt-in): per slot K entries in W-way sets (W = min(4, K)) holding the legal-move logits and
// value the network returned for a position.  A request's output depends only on its 15 input planes (board + side to move;
// the ordered legal moves are a function of them) and each evaluator kernel's arithmetic for a row is independent of its
// batch position, so a cached row is bit-identical to a recomputed one.  Private to a slot: no sharing, no atomics.
//
//   key   : 90 squares x 4 bits (1 + the plane 0..13 that holds the square's piece, 0 = empty) and the side to move (plane
//           14) as nibble 90; nibble i sits at bits 4 (i mod 8) of word i / 8 -- 12 words, injective over k_select's planes.
//   set   : a hash of the key picks the set; a hit needs all 12 key words, the current generation and the count to match.
//   stamp : the slot's probe clock at insert / last hit; the victim is an entry of an older generation, else the oldest stamp
//           (lowest way on ties).

enum Ec : int { EC_GEN = 0, EC_CLOCK, EC_HIT, EC_SKEY, EC_STATS, EC_EGEN, EC_STAMP, EC_COUNT, EC_VALUE, EC_KEY, EC_LOGITS, EC_N };
enum EcSt : int { ECS_PROBES = 0, ECS_HITS, ECS_INSERTS, ECS_EVICTIONS, ECS_MISMATCHES, ECS_N = 8 };
constexpr int EC_KEYW = 12;

struct EvDev {
    int K, W, sets;
    uint32_t *gen;                    // the current generation (device word: no host value is recorded into a graph)
    uint32_t *clock;                  // [G] probes of the slot so far
    int32_t *hit;                     // [G] 1: this step's request was answered by the cache
    uint32_t *skey;                   // [G][12] the key probed this step (commit's input)
    unsigned long long *stats;        // [G][ECS_N]
    uint32_t *egen, *stamp;           // [G K]
    int32_t *count;                   // [G K]
    float *value;                     // [G K]
    uint32_t *key;                    // [G K][12]
    float *logits;                    // [G K][XQ_MAXM]
};

EvDev make_evdev(const xq_evcache *c) {
    EvDev d;
    d.K = c->entries; d.W = c->ways; d.sets = c->sets;
    d.gen = (uint32_t *)c->p[EC_GEN]; d.clock = (uint32_t *)c->p[EC_CLOCK]; d.hit = (int32_t *)c->p[EC_HIT];
    d.skey = (uint32_t *)c->p[EC_SKEY]; d.stats = (unsigned long long *)c->p[EC_STATS];
    d.egen = (uint32_t *)c->p[EC_EGEN]; d.stamp = (uint32_t *)c->p[EC_STAMP]; d.count = (int32_t *)c->p[EC_COUNT];
    d.value = (float *)c->p[EC_VALUE]; d.key = (uint32_t *)c->p[EC_KEY]; d.logits = (float *)c->p[EC_LOGITS];
    return d;
}

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

// Probe: one wave per slot, four per workgroup; slots that are not waiting exit.  Lane w < W tests way w of the key's set.
// A hit writes the entry's logits / value into the slot-ordered hand-back rows k_expand reads (as k_scatter_rows does for
// evaluated rows) and refreshes its stamp; every probe records its key for k_evcache_commit.
__global__ __launch_bounds__(256) void k_evcache_probe(Dev E, EvDev C, const float *__restrict__ nn_in,
                                                       float *__restrict__ slot_logits, float *__restrict__ slot_value) {
    const int slot = blockIdx.x * 4 + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (slot >= E.cfg.n_games) return;
    const int ph = E.gi[(size_t)slot * GI_N + GI_PHASE];
    if (ph != PH_WAIT_ROOT && ph != PH_WAIT_LEAF) return;
    uint32_t key[EC_KEYW];
    wave_evkey(nn_in + (size_t)slot * XQ_STATE_FLOATS, key);
    const int count = E.req[slot];
    const uint32_t gen = *C.gen, clock = C.clock[slot] + 1u;
    const size_t e0 = (size_t)slot * C.K + (size_t)(evkey_hash(key) & (uint32_t)(C.sets - 1)) * C.W;
    bool kmatch = false, same = false;
    if (lane < C.W) {
        const size_t e = e0 + lane;
        kmatch = C.egen[e] == gen && key_eq(C.key + e * EC_KEYW, key);
        same = kmatch && C.count[e] == count;
    }
    const unsigned long long km = __ballot(kmatch), sm = __ballot(same);
    const int way = sm ? __ffsll((long long)sm) - 1 : -1;
    if (way >= 0) {
        const size_t e = e0 + way;
        ((float2 *)(slot_logits + (size_t)slot * XQ_MAXM))[lane] = ((const float2 *)(C.logits + e * XQ_MAXM))[lane];
        if (lane == 0) { slot_value[slot] = C.value[e]; C.stamp[e] = clock; }
    }
    if (lane == 0) {
        uint4 *sk = (uint4 *)(C.skey + (size_t)slot * EC_KEYW);
        sk[0] = make_uint4(key[0], key[1], key[2], key[3]);
        sk[1] = make_uint4(key[4], key[5], key[6], key[7]);
        sk[2] = make_uint4(key[8], key[9], key[10], key[11]);
        C.hit[slot] = way >= 0 ? 1 : 0;
        C.clock[slot] = clock;
        unsigned long long *st = C.stats + (size_t)slot * ECS_N;
        st[ECS_PROBES] += 1;
        st[ECS_HITS] += way >= 0 ? 1 : 0;
        st[ECS_MISMATCHES] += (way < 0 && km) ? 1 : 0;     // key and generation match, count differs: never expected
    }
}

// Stable compaction of the misses (xq_engine_compact_misses): k_compact with the predicate "waiting and not a hit".
__global__ __launch_bounds__(CPT) void k_compact_misses(Dev E, const int32_t *__restrict__ hit, int32_t *__restrict__ n_live,
                                                        int32_t *__restrict__ rows) {
    block_compact(E, E.cfg.n_games, [&](int s) { return slot_waits(E, s) && hit[s] == 0; }, n_live, rows);
}

// Commit: one wave per evaluated (packed) row r < n_live; the row's slot inserts the key it probed with this step.  One
// insert per slot and step, so the victim choice is deterministic without atomics.
__global__ __launch_bounds__(256) void k_evcache_commit(EvDev C, int G, const int32_t *__restrict__ n_live,
                                                        const int32_t *__restrict__ rows, const int32_t *__restrict__ counts,
                                                        const float *__restrict__ logits, const float *__restrict__ value) {
    const int r = blockIdx.x * 4 + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= G || r >= *n_live) return;
    const int slot = rows[r];
    const uint4 *sk = (const uint4 *)(C.skey + (size_t)slot * EC_KEYW);
    const uint4 k0 = sk[0], k1 = sk[1], k2 = sk[2];
    const uint32_t key[EC_KEYW] = {k0.x, k0.y, k0.z, k0.w, k1.x, k1.y, k1.z, k1.w, k2.x, k2.y, k2.z, k2.w};
    const uint32_t gen = *C.gen, clock = C.clock[slot];
    const size_t e0 = (size_t)slot * C.K + (size_t)(evkey_hash(key) & (uint32_t)(C.sets - 1)) * C.W;
    int victim = 0;
    bool evict = true;
    uint32_t oldest = 0xFFFFFFFFu;
    for (int w = 0; w < C.W; ++w) {
        const size_t e = e0 + w;
        if (C.egen[e] != gen) { victim = w; evict = false; break; }
        const uint32_t st = C.stamp[e];
        if (st < oldest) { oldest = st; victim = w; }
    }
    const size_t e = e0 + victim;
    ((float2 *)(C.logits + e * XQ_MAXM))[lane] = ((const float2 *)(logits + (size_t)r * XQ_MAXM))[lane];
    if (lane == 0) {
        uint4 *ek = (uint4 *)(C.key + e * EC_KEYW);
        ek[0] = k0; ek[1] = k1; ek[2] = k2;
        C.value[e] = value[r];
        C.count[e] = counts[r];
        C.egen[e] = gen;
        C.stamp[e] = clock;
        unsigned long long *st = C.stats + (size_t)slot * ECS_N;
        st[ECS_INSERTS] += 1;
        st[ECS_EVICTIONS] += evict ? 1 : 0;
    }
}

// Invalidation: a new generation; entries of older ones never hit and are the first victims.
__global__ void k_evcache_invalidate(uint32_t *gen) {
    if (threadIdx.x == 0) *gen += 1u;
}

struct EcLayout {
    size_t off[EC_N];
    size_t total;
};

bool evcache_args_ok(long long n_slots, long long k) { return n_slots > 0 && k > 0 && (k & (k - 1)) == 0 && k <= (1 << 20); }

EcLayout make_ec_layout(size_t G, size_t K) {
    EcLayout l;
    memset(&l, 0, sizeof(l));
    const size_t GK = G * K;
    size_t o = 0;
    auto put = [&](int id, size_t bytes) { l.off[id] = o; o = align_up(o + bytes); };
    put(EC_GEN, 4);
    put(EC_CLOCK, G * 4);
    put(EC_HIT, G * 4);
    put(EC_SKEY, G * EC_KEYW * 4);
    put(EC_STATS, G * ECS_N * 8);
    put(EC_EGEN, GK * 4);            // everything up to here is zeroed by xq_evcache_init
    put(EC_STAMP, GK * 4);
    put(EC_COUNT, GK * 4);
    put(EC_VALUE, GK * 4);
    put(EC_KEY, GK * EC_KEYW * 4);
    put(EC_LOGITS, GK * XQ_MAXM * 4);
    l.total = o;
    return l;
}

bool evcache_ok(const xq_evcache *c) {
    return c && evcache_args_ok(c->n_slots, c->entries) && c->ways > 0 && c->sets > 0 && c->ways * c->sets == c->entries &&
           c->p[EC_GEN] && c->p[EC_LOGITS];
}


struct Layout {
    size_t off[32];
    size_t total;
    int node_cap, path_cap, stage_cap;
};

// K > 1 (leaf batching): the request rows (moves, counts, paths, packed buffers) are G K, slot-major; the virtual-loss
// counters and the pending-leaf records follow the K = 1 layout, which is unchanged.  gz_m > 0 (Gumbel root search, K = 1): the
// square-root table's region also holds the Gumbel words (gz_bytes); every other engine has the layout it had.
// arena (arena options, K = 1, never Gumbel): that region holds the arena words instead (ar_off).
Layout make_layout(const xq_engine_config *c, int K = 1, int gz_m = 0, bool arena = false) {
    Layout l;
    memset(&l, 0, sizeof(l));
    const size_t G = (size_t)c->n_games, S = (size_t)c->num_simulations, GK = G * (size_t)K;
    l.node_cap = (int)(1 + (S + 1) * XQ_MAXM);
    l.path_cap = (int)(S + 2);
    int sc = c->max_game_length < 200 ? c->max_game_length : 200;
    if (sc < 1) sc = 1;
    l.stage_cap = c->manual_moves ? 1 : sc + 1;
    size_t o = 0;
    auto put = [&](int id, size_t bytes) { l.off[id] = o; o = align_up(o + bytes); };
    put(P_BOARD, G * XQ_BS);
    put(P_HIST, G * XQ_HIST * XQ_BS);
    put(P_GI, G * GI_N * 4);
    put(P_RESIGN, G * 16 * 8);
    put(P_PMOVES, GK * XQ_MAXM * 2);
    put(P_PATH, GK * (size_t)l.path_cap * 4);
    put(P_TN, G * (size_t)l.node_cap * 4);
    put(P_TW, G * (size_t)l.node_cap * 8);
    put(P_TP, G * (size_t)l.node_cap * 4);
    put(P_TA, G * (size_t)l.node_cap * 2);
    put(P_TC, G * (size_t)l.node_cap * 4);
    put(P_TM, G * (size_t)l.node_cap * 2);
    put(P_ROOTP, G * XQ_MAXM * 8);
    put(P_STAGE, G * (size_t)l.stage_cap * XQ_SAMPLE_BYTES);
    put(P_OUTS, (size_t)(c->max_out_samples > 0 ? c->max_out_samples : 1) * XQ_SAMPLE_BYTES);
    put(P_OUTR, (size_t)(c->max_out_results > 0 ? c->max_out_results : 1) * XQ_RESULT_BYTES);
    put(P_CNT, 64);
    put(P_STATS, G * ST_N * 8);
    put(P_SQRT, arena ? ar_off(G, S).end : (S + 2 + (K > 1 ? (size_t)K : 0)) * 8 + (gz_m > 0 ? gz_bytes(G, S, (size_t)gz_m) : 0));
    put(P_MNOISE, G * XQ_MAXM * 8);
    put(P_STATSUM, ST_N * 8);
    put(P_REQ, GK * 4);
    put(P_PK_N, 4);
    put(P_PK_ROWS, GK * 4);
    put(P_PK_X, GK * XQ_STATE_FLOATS * 4);
    put(P_PK_MOVES, GK * XQ_MAXM * 2);
    put(P_PK_COUNTS, GK * 4);
    put(P_PK_LOGITS, GK * XQ_MAXM * 4);
    put(P_PK_VALUE, GK * 4);
    if (K > 1) {
        put(P_VL, G * (size_t)l.node_cap * 4);
        put(P_LEAF, GK * 4 * 4);
    }
    l.total = o;
    return l;
}

bool config_ok(const xq_engine_config *c) {
    return c && c->n_games > 0 && c->num_simulations > 0 && c->num_simulations < 16000 && c->resign_check_steps >= 1 &&
           c->resign_check_steps <= 16 && c->random_opening_moves >= 0 && c->late_temperature > 0.0 && c->inject_len >= 0;
}

bool leaves_ok(const xq_engine_config *c, int K) { return K >= 1 && K <= 64 && !(K > 1 && c->manual_moves == 2); }

// tree reuse: self-play only, one leaf per step, S within k_reroot's LDS (64 KiB at S = XQ_REUSE_MAX_SIMS)
bool flags_ok(const xq_engine_config *c, int K, unsigned flags) {
    if (flags & ~(unsigned)XQ_ENGINE_TREE_REUSE) return false;
    if (!(flags & XQ_ENGINE_TREE_REUSE)) return true;
    return c->manual_moves == 0 && K == 1 && c->num_simulations <= XQ_REUSE_MAX_SIMS;
}

// playout cap: self-play only, one leaf per step, 1 <= S_fast < S, 0 < p <= 1 (a NaN fails both comparisons)
bool cap_ok(const xq_engine_config *c, int K, const xq_playout_cap *cap) {
    return c->manual_moves == 0 && K == 1 && cap->reserved == 0 && cap->fast_simulations >= 1 &&
           cap->fast_simulations < c->num_simulations && cap->full_search_prob > 0.0 && cap->full_search_prob <= 1.0;
}

// forced playouts: self-play with root noise only, one leaf per step, 0 < k <= 16 (a NaN fails both comparisons)
bool forced_ok(const xq_engine_config *c, int K, const xq_forced_playouts *fp) {
    if (c->manual_moves != 0 || c->add_noise == 0 || K != 1) return false;
    for (uint32_t r : fp->reserved) if (r != 0) return false;
    return fp->k > 0.0 && fp->k <= 16.0;
}

// Gumbel root search: self-play or search only, one leaf per step, none of tree reuse, playout cap and forced playouts;
// 1 <= m <= XQ_MAXM, c_visit >= 0 and c_scale > 0, finite as the float32 values the kernels use (a NaN fails the comparisons)
bool gumbel_ok(const xq_engine_config *c, int K, unsigned flags, const xq_playout_cap *cap, const xq_forced_playouts *forced,
               const xq_gumbel *gz) {
    if (c->manual_moves == 2 || K != 1 || (flags & XQ_ENGINE_TREE_REUSE) || cap || forced || gz->reserved != 0) return false;
    if (!(gz->c_visit >= 0.0 && gz->c_visit <= (double)FLT_MAX && gz->c_scale > 0.0 && gz->c_scale <= (double)FLT_MAX)) return false;
    return gz->considered >= 1 && gz->considered <= XQ_MAXM && (float)gz->c_scale > 0.0f;
}

// arena options: arena games only (so K = 1 and none of tree reuse, playout cap, forced playouts, Gumbel: each refuses
// manual_moves = 2 itself), 0 <= opening_plies <= XQ_ARENA_MAX_OPENING, first_game >= 0 with first_game + n_games an int32
bool arena_ok(const xq_engine_config *c, const xq_arena_opts *ar) {
    if (c->manual_moves != 2 || ar->reserved[0] != 0 || ar->reserved[1] != 0) return false;
    if (ar->opening_plies < 0 || ar->opening_plies > XQ_ARENA_MAX_OPENING) return false;
    return ar->first_game >= 0 && ar->first_game <= 0x7FFFFFFF - c->n_games;
}

// pad0 of an engine handle: leaves per step in the low 16 bits (0 = 1), the XQ_ENGINE_* flags above them, and above the public
// flag bits "playout cap on" (xq_engine_init_cap), "forced playouts on" (xq_engine_init_fp) and "Gumbel root search on"
// (xq_engine_init_gz) and "arena options on" (xq_engine_init_ar)
constexpr int PAD0_CAP = 1 << 30;
constexpr int PAD0_FORCED = 1 << 29;
constexpr int PAD0_GUMBEL = 1 << 28;
constexpr int PAD0_ARENA = 1 << 27;
int leaves_of(const xq_engine *e) { return (e->pad0 & 0xFFFF) > 1 ? (e->pad0 & 0xFFFF) : 1; }
bool reuse_of(const xq_engine *e) { return ((unsigned)e->pad0 >> 16) & XQ_ENGINE_TREE_REUSE; }
bool cap_of(const xq_engine *e) { return (e->pad0 & PAD0_CAP) != 0; }
bool forced_of(const xq_engine *e) { return (e->pad0 & PAD0_FORCED) != 0; }
bool gumbel_of(const xq_engine *e) { return (e->pad0 & PAD0_GUMBEL) != 0; }
bool arena_of(const xq_engine *e) { return e && (e->pad0 & PAD0_ARENA) != 0 && e->cfg.n_games > 0 && e->p[P_SQRT]; }

ArSets make_ar_sets(const xq_engine *e) {
    const ArOff o = ar_off((size_t)e->cfg.n_games, (size_t)e->cfg.num_simulations);
    char *base = (char *)e->p[P_SQRT];
    ArSets a;
    a.head = (const ArHead *)(base + o.head);
    a.n_live = (int32_t *)(base + o.n_live);
    for (int m = 0; m < 2; ++m) {
        a.rows[m] = (int32_t *)(base + o.rows[m]); a.x[m] = (float *)(base + o.x[m]);
        a.moves[m] = (uint16_t *)(base + o.moves[m]); a.counts[m] = (int32_t *)(base + o.counts[m]);
    }
    return a;
}

// the K = 1 step's two kernels, by the engine's options: instance [FORCED][CAP][REUSE]; a Gumbel engine has none of the three
// and its own instance of each kernel
void launch_select(const xq_engine *eng, const Dev &d, float *nn_in, hipStream_t s) {
    static void (*const k[2][2][2])(Dev, float *) = {
        {{k_select<false, false, false>, k_select<true, false, false>}, {k_select<false, true, false>, k_select<true, true, false>}},
        {{k_select<false, false, true>, k_select<true, false, true>}, {k_select<false, true, true>, k_select<true, true, true>}}};
    const dim3 grid((eng->cfg.n_games + WAVES_PER_WG - 1) / WAVES_PER_WG), block(64 * WAVES_PER_WG);
    if (gumbel_of(eng)) {
        hipLaunchKernelGGL((k_select<false, false, false, true>), grid, block, 0, s, d, nn_in);
        return;
    }
    if (arena_of(eng)) {
        hipLaunchKernelGGL((k_select<false, false, false, false, true>), grid, block, 0, s, d, nn_in);
        return;
    }
    hipLaunchKernelGGL(k[forced_of(eng)][cap_of(eng)][reuse_of(eng)], grid, block, 0, s, d, nn_in);
}

void launch_expand(const xq_engine *eng, const Dev &d, const float *policy, const float *value, int is_probs, hipStream_t s) {
    static void (*const k[2][2])(Dev, const float *, const float *, int) = {{k_expand<false, false>, k_expand<true, false>},
                                                                            {k_expand<false, true>, k_expand<true, true>}};
    if (gumbel_of(eng)) {
        hipLaunchKernelGGL((k_expand<false, false, true>), dim3(eng->cfg.n_games), dim3(64), 0, s, d, policy, value, is_probs);
        return;
    }
    hipLaunchKernelGGL(k[cap_of(eng)][reuse_of(eng)], dim3(eng->cfg.n_games), dim3(64), 0, s, d, policy, value, is_probs);
}

Mx make_mx(const xq_engine *e) {
    Mx x;
    x.K = leaves_of(e);
    x.vl = (int32_t *)e->p[P_VL];
    x.leaf = (int32_t *)e->p[P_LEAF];
    return x;
}

}  // namespace

extern "C" {

size_t xq_engine_workspace_bytes(const xq_engine_config *cfg) {
    if (!config_ok(cfg)) return 0;
    return make_layout(cfg).total;
}

size_t xq_engine_workspace_bytes_leaves(const xq_engine_config *cfg, int leaves_per_step) {
    return xq_engine_workspace_bytes_ex(cfg, leaves_per_step, 0u);
}

size_t xq_engine_workspace_bytes_ex(const xq_engine_config *cfg, int leaves_per_step, unsigned flags) {
    return xq_engine_workspace_bytes_cap(cfg, leaves_per_step, flags, nullptr);
}

size_t xq_engine_workspace_bytes_cap(const xq_engine_config *cfg, int leaves_per_step, unsigned flags, const xq_playout_cap *cap) {
    return xq_engine_workspace_bytes_fp(cfg, leaves_per_step, flags, cap, nullptr);
}

size_t xq_engine_workspace_bytes_fp(const xq_engine_config *cfg, int leaves_per_step, unsigned flags, const xq_playout_cap *cap,
                                    const xq_forced_playouts *forced) {
    if (!config_ok(cfg) || !leaves_ok(cfg, leaves_per_step) || !flags_ok(cfg, leaves_per_step, flags)) return 0;
    if (cap && !cap_ok(cfg, leaves_per_step, cap)) return 0;
    if (forced && !forced_ok(cfg, leaves_per_step, forced)) return 0;
    return make_layout(cfg, leaves_per_step).total;   // tree reuse, the playout cap and forced playouts need no workspace of their own
}

size_t xq_engine_workspace_bytes_gz(const xq_engine_config *cfg, int leaves_per_step, unsigned flags, const xq_playout_cap *cap,
                                    const xq_forced_playouts *forced, const xq_gumbel *gumbel) {
    if (!gumbel) return xq_engine_workspace_bytes_fp(cfg, leaves_per_step, flags, cap, forced);
    if (!config_ok(cfg) || !leaves_ok(cfg, leaves_per_step) || !flags_ok(cfg, leaves_per_step, flags)) return 0;
    if (!gumbel_ok(cfg, leaves_per_step, flags, cap, forced, gumbel)) return 0;
    return make_layout(cfg, 1, gumbel->considered).total;
}

size_t xq_engine_workspace_bytes_ar(const xq_engine_config *cfg, int leaves_per_step, unsigned flags, const xq_playout_cap *cap,
                                    const xq_forced_playouts *forced, const xq_gumbel *gumbel, const xq_arena_opts *arena) {
    const size_t plain = xq_engine_workspace_bytes_gz(cfg, leaves_per_step, flags, cap, forced, gumbel);
    if (!arena || plain == 0) return plain;
    if (!arena_ok(cfg, arena)) return 0;
    return make_layout(cfg, 1, 0, true).total;
}

int xq_gumbel_considered_visits_host(int k, int num_simulations, uint16_t *host_out) {
    if (k < 1 || k > XQ_MAXM || num_simulations < 1 || num_simulations > 65535 || !host_out) return XQ_ERR_ARG;
    gz_considered_visits(k, num_simulations, host_out);
    return XQ_OK;
}

int xq_engine_init(xq_engine *eng, const xq_engine_config *cfg, void *ws, size_t ws_bytes, const uint64_t *dev_inject,
                   void *stream) {
    return xq_engine_init_ex(eng, cfg, 1, 0u, ws, ws_bytes, dev_inject, stream);
}

int xq_engine_init_leaves(xq_engine *eng, const xq_engine_config *cfg, int leaves_per_step, void *ws, size_t ws_bytes,
                          const uint64_t *dev_inject, void *stream) {
    return xq_engine_init_ex(eng, cfg, leaves_per_step, 0u, ws, ws_bytes, dev_inject, stream);
}

int xq_engine_init_ex(xq_engine *eng, const xq_engine_config *cfg, int leaves_per_step, unsigned flags, void *ws,
                      size_t ws_bytes, const uint64_t *dev_inject, void *stream) {
    return xq_engine_init_cap(eng, cfg, leaves_per_step, flags, nullptr, ws, ws_bytes, dev_inject, stream);
}

int xq_engine_init_cap(xq_engine *eng, const xq_engine_config *cfg, int leaves_per_step, unsigned flags, const xq_playout_cap *cap,
                       void *ws, size_t ws_bytes, const uint64_t *dev_inject, void *stream) {
    return xq_engine_init_fp(eng, cfg, leaves_per_step, flags, cap, nullptr, ws, ws_bytes, dev_inject, stream);
}

int xq_engine_init_fp(xq_engine *eng, const xq_engine_config *cfg, int leaves_per_step, unsigned flags, const xq_playout_cap *cap,
                      const xq_forced_playouts *forced, void *ws, size_t ws_bytes, const uint64_t *dev_inject, void *stream) {
    return xq_engine_init_gz(eng, cfg, leaves_per_step, flags, cap, forced, nullptr, ws, ws_bytes, dev_inject, stream);
}

int xq_engine_init_gz(xq_engine *eng, const xq_engine_config *cfg, int leaves_per_step, unsigned flags, const xq_playout_cap *cap,
                      const xq_forced_playouts *forced, const xq_gumbel *gumbel, void *ws, size_t ws_bytes,
                      const uint64_t *dev_inject, void *stream) {
    return xq_engine_init_ar(eng, cfg, leaves_per_step, flags, cap, forced, gumbel, nullptr, ws, ws_bytes, dev_inject, stream);
}

int xq_engine_init_ar(xq_engine *eng, const xq_engine_config *cfg, int leaves_per_step, unsigned flags, const xq_playout_cap *cap,
                      const xq_forced_playouts *forced, const xq_gumbel *gumbel, const xq_arena_opts *arena, void *ws,
                      size_t ws_bytes, const uint64_t *dev_inject, void *stream) {
    if (!eng || !config_ok(cfg) || !leaves_ok(cfg, leaves_per_step) || !flags_ok(cfg, leaves_per_step, flags) || !ws ||
        ((uintptr_t)ws & 255))
        return XQ_ERR_ARG;
    if (cap && !cap_ok(cfg, leaves_per_step, cap)) return XQ_ERR_ARG;
    if (forced && !forced_ok(cfg, leaves_per_step, forced)) return XQ_ERR_ARG;
    if (gumbel && !gumbel_ok(cfg, leaves_per_step, flags, cap, forced, gumbel)) return XQ_ERR_ARG;
    if (arena && !arena_ok(cfg, arena)) return XQ_ERR_ARG;
    if (cfg->inject_len > 0 && !dev_inject) return XQ_ERR_ARG;
    const int K = leaves_per_step;
    const Layout l = make_layout(cfg, K, gumbel ? gumbel->considered : 0, arena != nullptr);
    if (ws_bytes < l.total) return XQ_ERR_WORKSPACE;
    memset(eng, 0, sizeof(*eng));
    eng->cfg = *cfg;
    eng->node_cap = l.node_cap; eng->path_cap = l.path_cap; eng->stage_cap = l.stage_cap;
    eng->pad0 = (K > 1 ? K : 0) | (int)(flags << 16) | (cap ? PAD0_CAP : 0) | (forced ? PAD0_FORCED : 0) | (gumbel ? PAD0_GUMBEL : 0) |
                (arena ? PAD0_ARENA : 0);
    for (int i = 0; i < 32; ++i) eng->p[i] = (char *)ws + l.off[i];
    eng->p[P_INJECT] = (void *)dev_inject;
    hipStream_t s = (hipStream_t)stream;
    // small state is zeroed; tree arenas need no clearing (nodes are initialised when created)
    XQ_TRY(hipMemsetAsync(eng->p[P_BOARD], 0, l.off[P_PATH] - l.off[P_BOARD], s));
    XQ_TRY(hipMemsetAsync(eng->p[P_ROOTP], 0, (size_t)cfg->n_games * XQ_MAXM * 8, s));
    XQ_TRY(hipMemsetAsync(eng->p[P_MNOISE], 0, (size_t)cfg->n_games * XQ_MAXM * 8, s));
    XQ_TRY(hipMemsetAsync(eng->p[P_REQ], 0, (size_t)cfg->n_games * K * 4, s));
    // packed-step buffers: zero count, rows, requests, hand-back (the packed planes are written before they are read);
    // with K > 1 the virtual-loss counters and pending-leaf records behind them as well
    XQ_TRY(hipMemsetAsync(eng->p[P_PK_N], 0, l.off[P_PK_X] - l.off[P_PK_N], s));
    XQ_TRY(hipMemsetAsync(eng->p[P_PK_MOVES], 0, l.total - l.off[P_PK_MOVES], s));
    {
        const int n = cfg->num_simulations + 2 + (K > 1 ? K : 0);   // K > 1: N_parent + vl_parent < S + K
        // Gumbel root search: the parameters, a zeroed v_hat per slot and the considered-visit tables for k = 1 .. m follow the table
        const size_t S = (size_t)cfg->num_simulations, G = (size_t)cfg->n_games;
        // arena options: the whole region zeroed (openings record, both sets' counts and rows), then the table and the parameters
        const ArOff ao = ar_off(G, S);
        if (arena) XQ_TRY(hipMemsetAsync(eng->p[P_SQRT], 0, ao.end, s));
        const size_t bytes = arena ? ao.head + sizeof(ArHead) : sizeof(double) * n + (gumbel ? gz_bytes(G, S, (size_t)gumbel->considered) : 0);
        double *tab = (double *)calloc(bytes, 1);
        if (!tab) return XQ_ERR_ARG;
        for (int i = 0; i < n; ++i) tab[i] = sqrt((double)i);   // math.sqrt(visit_count), mcts.py:49
        if (gumbel) {
            GzHead *h = (GzHead *)(tab + n);
            h->m = gumbel->considered; h->c_visit = (float)gumbel->c_visit; h->c_scale = (float)gumbel->c_scale;
            uint16_t *vis = (uint16_t *)((char *)(h + 1) + G * 8);
            for (int k = 1; k <= gumbel->considered; ++k) gz_considered_visits(k, (int)S, vis + (size_t)(k - 1) * S);
        }
        if (arena) {
            ArHead *h = (ArHead *)((char *)tab + ao.head);
            h->opening_plies = arena->opening_plies; h->first_game = arena->first_game;
        }
        const int rc = xq::check(hipMemcpyAsync(eng->p[P_SQRT], tab, bytes, hipMemcpyHostToDevice, s));
        if (rc == XQ_OK) (void)hipStreamSynchronize(s);
        free(tab);
        if (rc != XQ_OK) return rc;
    }
    const Dev d = make_dev(eng);
    hipLaunchKernelGGL(k_init, dim3((cfg->n_games + 255) / 256), dim3(256), 0, s, d);
    if (cap) {
        const int rc = launch_status();
        if (rc != XQ_OK) return rc;
        hipLaunchKernelGGL(k_init_cap, dim3((cfg->n_games + 255) / 256), dim3(256), 0, s, d, (int)cap->fast_simulations,
                           cap->full_search_prob);
    }
    if (forced) {
        const int rc = launch_status();
        if (rc != XQ_OK) return rc;
        hipLaunchKernelGGL(k_init_fp, dim3((cfg->n_games + 255) / 256), dim3(256), 0, s, d, (float)forced->k);
    }
    return launch_status();
}

int xq_engine_select(const xq_engine *eng, float *dev_nn_input, void *stream) {
    if (!eng || !dev_nn_input) return XQ_ERR_ARG;
    const Dev d = make_dev(eng);
    if (leaves_of(eng) > 1) {
        hipLaunchKernelGGL(k_select_multi, dim3(eng->cfg.n_games), dim3(64), 0, (hipStream_t)stream, d, make_mx(eng), dev_nn_input);
        return launch_status();
    }
    launch_select(eng, d, dev_nn_input, (hipStream_t)stream);
    if (reuse_of(eng)) {
        // the re-root runs here, between k_select<true> and the expansion, so every step variant (full, packed, cached) has it
        const int rc = launch_status();
        if (rc != XQ_OK) return rc;
        hipLaunchKernelGGL(k_reroot, dim3(eng->cfg.n_games), dim3(RR_THREADS),
                           (unsigned)reroot_lds_bytes(eng->node_cap, eng->cfg.num_simulations), (hipStream_t)stream, d);
    }
    return launch_status();
}

int xq_engine_drop_reroots(const xq_engine *eng, void *stream) {
    if (!eng || !reuse_of(eng) || eng->cfg.n_games <= 0) return XQ_ERR_ARG;
    hipLaunchKernelGGL(k_drop_reroots, dim3((eng->cfg.n_games + 255) / 256), dim3(256), 0, (hipStream_t)stream, make_dev(eng));
    return launch_status();
}

int xq_engine_expand(const xq_engine *eng, const float *dev_policy, const float *dev_value, int policy_is_probs,
                     void *stream) {
    if (!eng || !dev_policy || !dev_value) return XQ_ERR_ARG;
    const Dev d = make_dev(eng);
    if (leaves_of(eng) > 1) {
        hipLaunchKernelGGL(k_expand_multi, dim3(eng->cfg.n_games), dim3(64), 0, (hipStream_t)stream, d, make_mx(eng), dev_policy,
                           dev_value, policy_is_probs ? 1 : 0);
        return launch_status();
    }
    launch_expand(eng, d, dev_policy, dev_value, policy_is_probs ? 1 : 0, (hipStream_t)stream);
    return launch_status();
}

int xq_engine_requests(const xq_engine *eng, const uint16_t **dev_moves, const int32_t **dev_counts) {
    if (!eng || !dev_moves || !dev_counts) return XQ_ERR_ARG;
    *dev_moves = (const uint16_t *)eng->p[P_PMOVES];
    *dev_counts = (const int32_t *)eng->p[P_REQ];
    return XQ_OK;
}

int xq_engine_expand_legal(const xq_engine *eng, const float *dev_legal_logits, const float *dev_value, void *stream) {
    if (!eng || !dev_legal_logits || !dev_value) return XQ_ERR_ARG;
    const Dev d = make_dev(eng);
    if (leaves_of(eng) > 1) {
        hipLaunchKernelGGL(k_expand_multi, dim3(eng->cfg.n_games), dim3(64), 0, (hipStream_t)stream, d, make_mx(eng), dev_legal_logits,
                           dev_value, 2);
        return launch_status();
    }
    launch_expand(eng, d, dev_legal_logits, dev_value, 2, (hipStream_t)stream);
    return launch_status();
}

int xq_engine_compact(const xq_engine *eng, const float *dev_nn_input, void *stream) {
    if (!eng || !dev_nn_input || eng->cfg.n_games <= 0) return XQ_ERR_ARG;
    const Dev d = make_dev(eng);
    hipStream_t s = (hipStream_t)stream;
    int32_t *n_live = (int32_t *)eng->p[P_PK_N], *rows = (int32_t *)eng->p[P_PK_ROWS];
    const int K = leaves_of(eng);
    if (K > 1) hipLaunchKernelGGL(k_compact_multi, dim3(1), dim3(CPT), 0, s, d, K, n_live, rows);
    else hipLaunchKernelGGL(k_compact, dim3(1), dim3(CPT), 0, s, d, n_live, rows);
    int rc = launch_status();
    if (rc != XQ_OK) return rc;
    hipLaunchKernelGGL(k_gather_rows, dim3(eng->cfg.n_games * K), dim3(256), 0, s, d, (const int32_t *)n_live, (const int32_t *)rows,
                       dev_nn_input, (float *)eng->p[P_PK_X], (uint16_t *)eng->p[P_PK_MOVES], (int32_t *)eng->p[P_PK_COUNTS]);
    return launch_status();
}

int xq_engine_packed(const xq_engine *eng, xq_engine_packed_buffers *out) {
    if (!eng || !out) return XQ_ERR_ARG;
    out->n_live = (const int32_t *)eng->p[P_PK_N];
    out->rows = (const int32_t *)eng->p[P_PK_ROWS];
    out->x = (const float *)eng->p[P_PK_X];
    out->moves = (const uint16_t *)eng->p[P_PK_MOVES];
    out->counts = (const int32_t *)eng->p[P_PK_COUNTS];
    out->slot_logits = (const float *)eng->p[P_PK_LOGITS];
    out->slot_value = (const float *)eng->p[P_PK_VALUE];
    return XQ_OK;
}

int xq_engine_expand_packed(const xq_engine *eng, const float *dev_packed_logits, const float *dev_packed_value, void *stream) {
    if (!eng || !dev_packed_logits || !dev_packed_value || eng->cfg.n_games <= 0) return XQ_ERR_ARG;
    if (((uintptr_t)dev_packed_logits) & 7) return XQ_ERR_ARG;
    const int G = eng->cfg.n_games * leaves_of(eng);   // request rows
    float *slot_logits = (float *)eng->p[P_PK_LOGITS], *slot_value = (float *)eng->p[P_PK_VALUE];
    hipLaunchKernelGGL(k_scatter_rows, dim3((G + 3) / 4), dim3(256), 0, (hipStream_t)stream, (const int32_t *)eng->p[P_PK_N],
                       (const int32_t *)eng->p[P_PK_ROWS], dev_packed_logits, dev_packed_value, slot_logits, slot_value, G);
    const int rc = launch_status();
    if (rc != XQ_OK) return rc;
    return xq_engine_expand_legal(eng, slot_logits, slot_value, stream);
}

int xq_engine_arena_openings(const xq_engine *eng, const uint16_t **dev_actions, const int32_t **dev_counts) {
    if (!arena_of(eng) || !dev_actions || !dev_counts) return XQ_ERR_ARG;
    const ArOff o = ar_off((size_t)eng->cfg.n_games, (size_t)eng->cfg.num_simulations);
    *dev_actions = (const uint16_t *)((char *)eng->p[P_SQRT] + o.op_actions);
    *dev_counts = (const int32_t *)((char *)eng->p[P_SQRT] + o.op_counts);
    return XQ_OK;
}

int xq_engine_compact_arena(const xq_engine *eng, const float *dev_nn_input, void *stream) {
    if (!arena_of(eng) || !dev_nn_input) return XQ_ERR_ARG;
    const Dev d = make_dev(eng);
    const ArSets a = make_ar_sets(eng);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_compact_arena, dim3(1), dim3(CPT), 0, s, d, a);
    for (int m = 0; m < 2; ++m) {
        const int rc = launch_status();
        if (rc != XQ_OK) return rc;
        hipLaunchKernelGGL(k_gather_rows, dim3(eng->cfg.n_games), dim3(256), 0, s, d, (const int32_t *)(a.n_live + m),
                           (const int32_t *)a.rows[m], dev_nn_input, a.x[m], a.moves[m], a.counts[m]);
    }
    return launch_status();
}

int xq_engine_packed_arena(const xq_engine *eng, xq_engine_packed_buffers out[2]) {
    if (!arena_of(eng) || !out) return XQ_ERR_ARG;
    const ArSets a = make_ar_sets(eng);
    for (int m = 0; m < 2; ++m) {
        out[m].n_live = a.n_live + m; out[m].rows = a.rows[m]; out[m].x = a.x[m]; out[m].moves = a.moves[m];
        out[m].counts = a.counts[m];
        out[m].slot_logits = (const float *)eng->p[P_PK_LOGITS]; out[m].slot_value = (const float *)eng->p[P_PK_VALUE];
    }
    return XQ_OK;
}

int xq_engine_expand_packed_arena(const xq_engine *eng, const float *dev_logits_new, const float *dev_value_new,
                                  const float *dev_logits_old, const float *dev_value_old, void *stream) {
    if (!arena_of(eng) || !dev_logits_new || !dev_value_new || !dev_logits_old || !dev_value_old) return XQ_ERR_ARG;
    if ((((uintptr_t)dev_logits_new) | ((uintptr_t)dev_logits_old)) & 7) return XQ_ERR_ARG;
    const int G = eng->cfg.n_games;
    const ArSets a = make_ar_sets(eng);
    float *slot_logits = (float *)eng->p[P_PK_LOGITS], *slot_value = (float *)eng->p[P_PK_VALUE];
    const float *logits[2] = {dev_logits_new, dev_logits_old}, *value[2] = {dev_value_new, dev_value_old};
    for (int m = 0; m < 2; ++m) {
        hipLaunchKernelGGL(k_scatter_rows, dim3((G + 3) / 4), dim3(256), 0, (hipStream_t)stream, (const int32_t *)(a.n_live + m),
                           (const int32_t *)a.rows[m], logits[m], value[m], slot_logits, slot_value, G);
        const int rc = launch_status();
        if (rc != XQ_OK) return rc;
    }
    return xq_engine_expand_legal(eng, slot_logits, slot_value, stream);
}

int xq_engine_stats_read(const xq_engine *eng, xq_engine_stats *host_out, void *stream) {
    if (!eng || !host_out) return XQ_ERR_ARG;
    const Dev d = make_dev(eng);
    hipStream_t s = (hipStream_t)stream;
    unsigned long long *sum = (unsigned long long *)eng->p[P_STATSUM];
    XQ_TRY(hipMemsetAsync(sum, 0, ST_N * sizeof(unsigned long long), s));
    int blocks = (eng->cfg.n_games + 63) / 64;
    if (blocks > 256) blocks = 256;
    hipLaunchKernelGGL(k_reduce_stats, dim3(blocks), dim3(256), 0, s, d, sum);
    int rc = launch_status();
    if (rc != XQ_OK) return rc;
    unsigned long long h[ST_N];
    XQ_TRY(hipMemcpyAsync(h, sum, sizeof(h), hipMemcpyDeviceToHost, s));
    XQ_TRY(hipStreamSynchronize(s));
    memset(host_out, 0, sizeof(*host_out));
    host_out->sims = h[ST_SIMS]; host_out->terminal_sims = h[ST_TERM]; host_out->leaf_evals = h[ST_LEAF];
    host_out->root_evals = h[ST_ROOT]; host_out->moves_played = h[ST_MOVES]; host_out->games_finished = h[ST_GAMES];
    host_out->red_wins = h[ST_RED]; host_out->black_wins = h[ST_BLACK]; host_out->draws = h[ST_DRAW];
    host_out->plies_finished = h[ST_PLIES]; host_out->nodes_created = h[ST_NODES]; host_out->depth_sum = h[ST_DEPTH];
    host_out->children_scanned = h[ST_SCAN]; host_out->resigns = h[ST_RESIGN]; host_out->samples_written = h[ST_SAMP];
    host_out->samples_dropped = h[ST_DROP]; host_out->overflow = h[ST_OVF]; host_out->games_started = h[ST_STARTED];
    host_out->rows_evaluated = h[ST_ROWS];
    host_out->reserved[XQ_STAT_COLLISIONS] = h[ST_COLL]; host_out->reserved[XQ_STAT_LEAVES_SUM] = h[ST_LPS];
    host_out->reserved[XQ_STAT_LEAF_STEPS] = h[ST_LSTEPS];
    host_out->reserved[XQ_STAT_REUSED_VISITS] = h[ST_REUSED]; host_out->reserved[XQ_STAT_REROOTS] = h[ST_REROOTS];
    host_out->reserved[XQ_STAT_FAST_MOVES] = h[ST_FASTM]; host_out->reserved[XQ_STAT_FAST_SIMS] = h[ST_FASTS];
    host_out->reserved[XQ_STAT_FORCED_SIMS] = h[ST_FORCED]; host_out->reserved[XQ_STAT_PRUNED_VISITS] = h[ST_PRUNEDV];
    host_out->reserved[XQ_STAT_PRUNED_CHILDREN] = h[ST_PRUNEDC];
    host_out->reserved[XQ_STAT_GUMBEL_MOVES] = h[ST_GZ_MOVES]; host_out->reserved[XQ_STAT_GUMBEL_CONSIDERED] = h[ST_GZ_CONS];
    host_out->reserved[XQ_STAT_GUMBEL_OFFPRIOR] = h[ST_GZ_OFF];
    return h[ST_OVF] ? XQ_ERR_OVERFLOW : XQ_OK;
}

int xq_engine_drain(const xq_engine *eng, void *host_samples, int max_samples, int *n_samples, void *host_results,
                    int max_results, int *n_results, void *stream) {
    if (!eng || !n_samples || !n_results) return XQ_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    unsigned cnt[2];
    XQ_TRY(hipStreamSynchronize(s));
    XQ_TRY(hipMemcpy(cnt, eng->p[P_CNT], sizeof(cnt), hipMemcpyDeviceToHost));
    unsigned ns = cnt[0] < (unsigned)eng->cfg.max_out_samples ? cnt[0] : (unsigned)eng->cfg.max_out_samples;
    unsigned nr = cnt[1] < (unsigned)eng->cfg.max_out_results ? cnt[1] : (unsigned)eng->cfg.max_out_results;
    if ((int)ns > max_samples || (int)nr > max_results) {   // caller's buffers too small: report sizes, keep the data
        *n_samples = (int)ns; *n_results = (int)nr;
        return XQ_ERR_ARG;
    }
    if (ns && host_samples) XQ_TRY(hipMemcpy(host_samples, eng->p[P_OUTS], (size_t)ns * XQ_SAMPLE_BYTES, hipMemcpyDeviceToHost));
    if (nr && host_results) XQ_TRY(hipMemcpy(host_results, eng->p[P_OUTR], (size_t)nr * XQ_RESULT_BYTES, hipMemcpyDeviceToHost));
    XQ_TRY(hipMemset(eng->p[P_CNT], 0, 8));
    *n_samples = (int)ns; *n_results = (int)nr;
    return XQ_OK;
}

int xq_engine_drain_device(const xq_engine *eng, void *dev_samples, int max_samples, int *n_samples, void *dev_results,
                           int max_results, int *n_results, void *stream) {
    if (!eng || !n_samples || !n_results) return XQ_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    unsigned cnt[2];
    XQ_TRY(hipStreamSynchronize(s));
    XQ_TRY(hipMemcpy(cnt, eng->p[P_CNT], sizeof(cnt), hipMemcpyDeviceToHost));
    const unsigned ns = cnt[0] < (unsigned)eng->cfg.max_out_samples ? cnt[0] : (unsigned)eng->cfg.max_out_samples;
    const unsigned nr = cnt[1] < (unsigned)eng->cfg.max_out_results ? cnt[1] : (unsigned)eng->cfg.max_out_results;
    *n_samples = (int)ns; *n_results = (int)nr;
    if (!dev_samples && !dev_results) return XQ_OK;          // size query: nothing is consumed
    if ((int)ns > max_samples || (int)nr > max_results || (ns && !dev_samples) || (nr && !dev_results)) return XQ_ERR_ARG;
    if (ns) XQ_TRY(hipMemcpyAsync(dev_samples, eng->p[P_OUTS], (size_t)ns * XQ_SAMPLE_BYTES, hipMemcpyDeviceToDevice, s));
    if (nr) XQ_TRY(hipMemcpyAsync(dev_results, eng->p[P_OUTR], (size_t)nr * XQ_RESULT_BYTES, hipMemcpyDeviceToDevice, s));
    XQ_TRY(hipMemsetAsync(eng->p[P_CNT], 0, 8, s));
    XQ_TRY(hipStreamSynchronize(s));
    return XQ_OK;
}

int xq_engine_set_position(const xq_engine *eng, int slot, const int8_t *host_board, int side, int move_count,
                           int no_capture, const int8_t *host_hist12, const double *host_noise, void *stream) {
    if (!eng || !host_board || slot < 0 || slot >= eng->cfg.n_games || (side != 1 && side != -1) || move_count < 0)
        return XQ_ERR_ARG;
    XQ_TRY(hipStreamSynchronize((hipStream_t)stream));
    int8_t b[XQ_BS];
    memset(b, 0, sizeof(b));
    memcpy(b, host_board, 90);
    XQ_TRY(hipMemcpy((char *)eng->p[P_BOARD] + (size_t)slot * XQ_BS, b, XQ_BS, hipMemcpyHostToDevice));
    int8_t ring[XQ_HIST][XQ_BS];
    memset(ring, 0, sizeof(ring));
    const int k = move_count < XQ_HIST ? move_count : XQ_HIST;
    if (k > 0 && !host_hist12) return XQ_ERR_ARG;
    for (int e = 0; e < k; ++e) {               // entry e (oldest first) is the pre-move board of ply mc-k+e
        const int ply = move_count - k + e;
        memcpy(ring[ply % XQ_HIST], host_hist12 + (size_t)e * 90, 90);
    }
    XQ_TRY(hipMemcpy((char *)eng->p[P_HIST] + (size_t)slot * XQ_HIST * XQ_BS, ring, sizeof(ring), hipMemcpyHostToDevice));
    int32_t gi[GI_N];
    memset(gi, 0, sizeof(gi));
    gi[GI_SIDE] = side; gi[GI_MC] = move_count; gi[GI_NOCAP] = no_capture; gi[GI_PHASE] = PH_NEWPOS;
    gi[GI_MANNOISE] = host_noise ? 1 : 0;
    XQ_TRY(hipMemcpy((char *)eng->p[P_GI] + (size_t)slot * GI_N * 4, gi, sizeof(gi), hipMemcpyHostToDevice));
    if (host_noise)
        XQ_TRY(hipMemcpy((char *)eng->p[P_MNOISE] + (size_t)slot * XQ_MAXM * 8, host_noise, XQ_MAXM * 8, hipMemcpyHostToDevice));
    return XQ_OK;
}

int xq_engine_read_root(const xq_engine *eng, int slot, uint16_t *actions, int32_t *visits, double *total_value,
                        double *prior, int *prior_kind, int32_t *root_visits, int32_t *sims_done, void *stream) {
    if (!eng || slot < 0 || slot >= eng->cfg.n_games || !actions || !visits || !total_value || !prior) return XQ_ERR_ARG;
    XQ_TRY(hipStreamSynchronize((hipStream_t)stream));
    const size_t nb = (size_t)slot * eng->node_cap;
    uint16_t m; int32_t first, rn; int32_t gi[GI_N];
    XQ_TRY(hipMemcpy(&m, (uint16_t *)eng->p[P_TM] + nb, 2, hipMemcpyDeviceToHost));
    XQ_TRY(hipMemcpy(&first, (int32_t *)eng->p[P_TC] + nb, 4, hipMemcpyDeviceToHost));
    XQ_TRY(hipMemcpy(&rn, (int32_t *)eng->p[P_TN] + nb, 4, hipMemcpyDeviceToHost));
    XQ_TRY(hipMemcpy(gi, (char *)eng->p[P_GI] + (size_t)slot * GI_N * 4, sizeof(gi), hipMemcpyDeviceToHost));
    const int n = m & 0x3FFF, kind = m >> 14;
    if (root_visits) *root_visits = rn;
    if (sims_done) *sims_done = gi[GI_SIMS];
    if (prior_kind) *prior_kind = kind == 0 ? 0 : (kind == 3 ? 3 : 1);
    if (n == 0) return 0;
    float pf[XQ_MAXM];
    XQ_TRY(hipMemcpy(actions, (uint16_t *)eng->p[P_TA] + nb + first, (size_t)n * 2, hipMemcpyDeviceToHost));
    XQ_TRY(hipMemcpy(visits, (int32_t *)eng->p[P_TN] + nb + first, (size_t)n * 4, hipMemcpyDeviceToHost));
    XQ_TRY(hipMemcpy(total_value, (double *)eng->p[P_TW] + nb + first, (size_t)n * 8, hipMemcpyDeviceToHost));
    if (kind == 1 || kind == 3) {
        XQ_TRY(hipMemcpy(prior, (double *)eng->p[P_ROOTP] + (size_t)slot * XQ_MAXM, (size_t)n * 8, hipMemcpyDeviceToHost));
    } else if (kind == 2) {
        for (int i = 0; i < n; ++i) prior[i] = 1.0 / (double)n;
    } else {
        XQ_TRY(hipMemcpy(pf, (float *)eng->p[P_TP] + nb + first, (size_t)n * 4, hipMemcpyDeviceToHost));
        for (int i = 0; i < n; ++i) prior[i] = (double)pf[i];
    }
    return n;
}


// ---- evaluation cache --------------------------------------------------------------------------------------------------
size_t xq_evcache_bytes(int n_slots, int entries_per_slot) {
    if (!evcache_args_ok(n_slots, entries_per_slot)) return 0;
    return make_ec_layout((size_t)n_slots, (size_t)entries_per_slot).total;
}

int xq_evcache_init(xq_evcache *cache, int n_slots, int entries_per_slot, void *dev_mem, size_t bytes, void *stream) {
    if (!cache || !evcache_args_ok(n_slots, entries_per_slot) || !dev_mem || ((uintptr_t)dev_mem & 255)) return XQ_ERR_ARG;
    const EcLayout l = make_ec_layout((size_t)n_slots, (size_t)entries_per_slot);
    if (bytes < l.total) return XQ_ERR_WORKSPACE;
    memset(cache, 0, sizeof(*cache));
    cache->n_slots = n_slots;
    cache->entries = entries_per_slot;
    cache->ways = entries_per_slot < 4 ? entries_per_slot : 4;
    cache->sets = entries_per_slot / cache->ways;
    for (int i = 0; i < EC_N; ++i) cache->p[i] = (char *)dev_mem + l.off[i];
    hipStream_t s = (hipStream_t)stream;
    XQ_TRY(hipMemsetAsync(dev_mem, 0, l.off[EC_COUNT], s));   // generation 0, clocks, flags, counters, entry generations, stamps
    hipLaunchKernelGGL(k_evcache_invalidate, dim3(1), dim3(64), 0, s, (uint32_t *)cache->p[EC_GEN]);   // generation 1
    return launch_status();
}

int xq_evcache_hit_flags(const xq_evcache *cache, const int32_t **dev_hit) {
    if (!evcache_ok(cache) || !dev_hit) return XQ_ERR_ARG;
    *dev_hit = (const int32_t *)cache->p[EC_HIT];
    return XQ_OK;
}

int xq_evcache_probe(const xq_evcache *cache, const xq_engine *eng, const float *dev_nn_input, void *stream) {
    if (!eng || leaves_of(eng) > 1) return XQ_ERR_ARG;            // the cache serves one request row per slot
    if (!evcache_ok(cache) || !dev_nn_input || eng->cfg.n_games <= 0 || cache->n_slots != eng->cfg.n_games)
        return XQ_ERR_ARG;
    const int G = eng->cfg.n_games;
    hipLaunchKernelGGL(k_evcache_probe, dim3((G + 3) / 4), dim3(256), 0, (hipStream_t)stream, make_dev(eng), make_evdev(cache),
                       dev_nn_input, (float *)eng->p[P_PK_LOGITS], (float *)eng->p[P_PK_VALUE]);
    return launch_status();
}

int xq_engine_compact_misses(const xq_engine *eng, const float *dev_nn_input, const int32_t *dev_hit_flags, void *stream) {
    if (!eng || !dev_nn_input || !dev_hit_flags || eng->cfg.n_games <= 0 || leaves_of(eng) > 1) return XQ_ERR_ARG;
    const Dev d = make_dev(eng);
    hipStream_t s = (hipStream_t)stream;
    int32_t *n_live = (int32_t *)eng->p[P_PK_N], *rows = (int32_t *)eng->p[P_PK_ROWS];
    hipLaunchKernelGGL(k_compact_misses, dim3(1), dim3(CPT), 0, s, d, dev_hit_flags, n_live, rows);
    int rc = launch_status();
    if (rc != XQ_OK) return rc;
    hipLaunchKernelGGL(k_gather_rows, dim3(eng->cfg.n_games), dim3(256), 0, s, d, (const int32_t *)n_live, (const int32_t *)rows,
                       dev_nn_input, (float *)eng->p[P_PK_X], (uint16_t *)eng->p[P_PK_MOVES], (int32_t *)eng->p[P_PK_COUNTS]);
    return launch_status();
}

int xq_evcache_commit(const xq_evcache *cache, const xq_engine *eng, const float *dev_packed_logits,
                      const float *dev_packed_value, void *stream) {
    if (!evcache_ok(cache) || !eng || leaves_of(eng) > 1 || !dev_packed_logits || !dev_packed_value || eng->cfg.n_games <= 0 ||
        cache->n_slots != eng->cfg.n_games || (((uintptr_t)dev_packed_logits) & 7))
        return XQ_ERR_ARG;
    const int G = eng->cfg.n_games;
    hipLaunchKernelGGL(k_evcache_commit, dim3((G + 3) / 4), dim3(256), 0, (hipStream_t)stream, make_evdev(cache), G,
                       (const int32_t *)eng->p[P_PK_N], (const int32_t *)eng->p[P_PK_ROWS], (const int32_t *)eng->p[P_PK_COUNTS],
                       dev_packed_logits, dev_packed_value);
    return launch_status();
}

int xq_evcache_invalidate(const xq_evcache *cache, void *stream) {
    if (!evcache_ok(cache)) return XQ_ERR_ARG;
    hipLaunchKernelGGL(k_evcache_invalidate, dim3(1), dim3(64), 0, (hipStream_t)stream, (uint32_t *)cache->p[EC_GEN]);
    return launch_status();
}

int xq_evcache_stats_read(const xq_evcache *cache, xq_evcache_stats *host_out, void *stream) {
    if (!evcache_ok(cache) || !host_out) return XQ_ERR_ARG;
    const size_t n = (size_t)cache->n_slots * ECS_N;
    unsigned long long *h = (unsigned long long *)malloc(n * sizeof(unsigned long long));
    if (!h) return XQ_ERR_ARG;
    int rc = xq::check(hipMemcpyAsync(h, cache->p[EC_STATS], n * sizeof(unsigned long long), hipMemcpyDeviceToHost,
                                      (hipStream_t)stream));
    if (rc == XQ_OK) rc = xq::check(hipStreamSynchronize((hipStream_t)stream));
    if (rc == XQ_OK) {
        unsigned long long sum[ECS_N] = {0};
        for (size_t i = 0; i < n; ++i) sum[i % ECS_N] += h[i];
        memset(host_out, 0, sizeof(*host_out));
        host_out->probes = sum[ECS_PROBES]; host_out->hits = sum[ECS_HITS]; host_out->inserts = sum[ECS_INSERTS];
        host_out->evictions = sum[ECS_EVICTIONS]; host_out->mismatches = sum[ECS_MISMATCHES];
    }
    free(h);
    return rc;
}

int xq_evcache_key_host(const float *host_planes, uint32_t *host_out12) {
    if (!host_planes || !host_out12) return XQ_ERR_ARG;
    for (int w = 0; w < EC_KEYW; ++w) host_out12[w] = 0;
    for (int sq = 0; sq < 90; ++sq) host_out12[sq >> 3] |= evkey_nibble(host_planes, sq) << (4 * (sq & 7));
    host_out12[90 >> 3] |= evkey_side(host_planes) << (4 * (90 & 7));
    return XQ_OK;
}

}  // extern "C"
