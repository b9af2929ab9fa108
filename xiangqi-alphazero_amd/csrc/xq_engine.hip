// xq_engine.hip -- device-resident self-play engine (B3): SoA MCTS trees in HBM, one wavefront per game.
//
// The engine's source, file by file:
//   xq_engine_state.cuh  : shared by the four units below -- enums (Phase, Gi, St, Ptr, Rng), the device view Dev, the Gumbel and
//                          arena words behind the square-root table, the pad0 encoding, Philox, block_compact.  No kernel.
//   xq_engine.hip        : the search (this file) -- k_select, k_expand, k_reroot, k_drop_reroots, k_select_multi, k_expand_multi and
//                          xq_engine_select / _expand / _expand_legal / _requests / _drop_reroots.
//   xq_engine_setup.hip  : the workspace layout, the option checks (Opts, opts_ok), every xq_engine_workspace_bytes* and
//                          xq_engine_init*, and the host-side readers (stats, drain, set_position, read_root).
//   xq_engine_packed.hip : the packed steps -- compaction, gather, scatter, and the arena's two-set variant.
//   xq_evcache.hip       : the evaluation cache (xq_evcache_*, xq_engine_compact_misses).
//   xq_evdedup.hip       : the request dedup (xq_evdedup_*, xq_engine_compact_unique / _expand_dedup, xq_dedup_rows_batch); the
//                          key both share is in xq_evkey.cuh.
//   xq_rules.cuh         : the wave-level rules, shared with the stateless tools (xq_batch, xq_replay, xq_supervise, xq_alphabeta,
//                          xq_mate .hip); what only those five share is in xq_tools.cuh, which nothing of the engine includes.
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
//   k_flush_records : game records (opt-in, xq_engine_init_gr): the record of every finished game, ahead of the select kernel
//                that starts the slot's next game; the moves themselves are logged by the select kernels (slot_log_move).
//   k_start_pool : start-position pool (opt-in, xq_engine_init_sp): the games that start from a pool entry, ahead of the select
//                kernel, which starts the others and issues every root request.
//   k_reroot : tree reuse (opt-in, XQ_ENGINE_TREE_REUSE; k_select<true> / k_expand<true>): the chosen child's subtree moved to the
//                front of the slot's arena, in place, between select and expand of the step that ends a move.
//
// Numeric contract (pinned by tests against the reference's MCTS under a stub evaluator): priors float32,
// PUCT evaluated in float32 as f32(q) + ((f32(c)*P)*f32(sqrt(N_parent)))/f32(1+N); at a noisy root (and for the
// uniform fallback) priors and PUCT are float64; W accumulates in float64; first maximum wins.
// Floating-point contraction is OFF for this file.
#include "xq_engine_state.cuh"

#pragma clang fp contract(off)

static_assert(sizeof(xq_sample) == XQ_SAMPLE_BYTES, "xq_sample layout");
static_assert(sizeof(xq_game_result) == XQ_RESULT_BYTES, "xq_game_result layout");
static_assert(sizeof(xq_sample_root_stats) == 20 && offsetof(xq_sample, pad) == XQ_SAMPLE_ROOT_STATS_OFFSET &&
                  sizeof(((xq_sample *)0)->pad) == sizeof(xq_sample_root_stats), "xq_sample_root_stats overlays xq_sample.pad");

namespace {

constexpr uint32_t RNG_ARENA_OPENING = 8u;  // xq_engine_init_ar: keyed by the PAIR and rank 0, never by the slot (7 is k_init's stagger)

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

// mcts.py:137-140: the value a terminal leaf backs up, from the view of the side that moved into it -- 0 for a draw, else 1: the
// reference takes every decided leaf for a win of the mover.  Only the perpetual-check verdict (`over` == 4) can name the side
// to move the winner (the mover's check completed its own perpetual): that leaf is the mover's loss.
__device__ __forceinline__ double terminal_leaf_value(int over, int winner, int side) {
    return winner == 0 ? 0.0 : (over == 4 && winner == side ? -1.0 : 1.0);
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

// Game records (xq_engine_init_gr; E.gr_log is NULL without them, a wave-uniform test): a real move's action goes to the slot's
// move log at the ply it is played at, before wave_make_move advances the count.  Indexing by the ply makes an opening that
// ended its game right by construction: the game restarts at ply 0 and the next moves overwrite the log.
__device__ __forceinline__ void slot_log_move(const Dev &E, Slot &s, int action) {
    if (!E.gr_log) return;
    if (s.mc >= XQ_RECORD_MAX_PLIES) { s.ovf |= 256; return; }
    if (s.lane == 0) E.gr_log[(size_t)s.slot * XQ_RECORD_MAX_PLIES + s.mc] = (uint16_t)action;
}

// the plies of the game that no search chose, once its opening is played
__device__ __forceinline__ void slot_log_opening(const Dev &E, const Slot &s) {
    if (E.gr_log && s.lane == 0) gr_opening(E.gr_log, (size_t)E.cfg.n_games)[s.slot] = (uint16_t)s.mc;
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
        // The cursor advances only for a game that fits: it never passes max_out_samples, and every row below it has been
        // written since the last drain.  A game that does not fit is dropped whole; a shorter one may still fit after it.
        if (lane == 0) {
            const unsigned cap = (unsigned)E.cfg.max_out_samples;
            unsigned seen = atomicAdd(&E.cnt[0], 0u);
            for (;;) {
                if ((unsigned long long)seen + (unsigned)n_samples > cap) { base = 0xFFFFFFFFu; break; }
                const unsigned prev = atomicCAS(&E.cnt[0], seen, seen + (unsigned)n_samples);
                if (prev == seen) { base = seen; break; }
                seen = prev;
            }
        }
        base = __builtin_amdgcn_readfirstlane(base);
        fits = base != 0xFFFFFFFFu;
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
        slot_log_move(E, s, action);
        wave_make_move(L.root, L.rhist, action, s.side, s.mc, s.nocap);
        int c2, w2;
        if (wave_game_over(L.root, L.rhist, s.side, s.mc, s.nocap, E.perpetual != 0, L.mg, L.moves, &c2, &w2, &s.ovf)) {
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
        slot_log_move(E, s, action);
        wave_make_move(L.root, L.rhist, action, s.side, s.mc, s.nocap);
        if (s.lane == 0) rec[i] = (uint16_t)action;
        played = i + 1;
        int c2, w2;
        if (wave_game_over(L.root, L.rhist, s.side, s.mc, s.nocap, E.perpetual != 0, L.mg, L.moves, &c2, &w2, &s.ovf)) {
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
    const int done = wave_game_over(L.root, L.rhist, s.side, s.mc, s.nocap, E.perpetual != 0, L.mg, L.moves, &cnt, &winner, &s.ovf);
    if (done) status = done;                               // 1, or 4: decided by the perpetual-check rule
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
__device__ __forceinline__ void slot_play(const Dev &E, Slot &s, SelectLds &L, int action) {
    slot_log_move(E, s, action);
    wave_make_move(L.root, L.rhist, action, s.side, s.mc, s.nocap);
    s.d_moves += 1;
    s.dirty = true;
}

// arena move, MCTS.get_action(temperature=0) (mcts.py:166-174, 197-200): first maximum of the visit counts, move order
__device__ __forceinline__ void slot_arena_move(const Dev &E, Slot &s, SelectLds &L, int nch, int first) {
    int bn;
    const int bi = wave_first_max(s.T.N + first, nch, bn);
    slot_play(E, s, L, __builtin_amdgcn_readfirstlane((int)s.T.A[first + bi]));
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
// L.w_tmp (wave_prune_visits', or wave_solver_counts').  Leaves child i's action in L.a_tmp[i]; the caller plays the returned
// action.  proven >= 0 (SOLVER, rule 4): child `proven` is played, no temperature, no uniform draw, the sample says reserved1 = 1.
// E.root_stats (xq_engine_init_rs): a staged sample also takes the root's search value, visits and mark into its pad bytes.
__device__ __forceinline__ int slot_end_move(const Dev &E, Slot &s, SelectLds &L, bool full_move, bool pruned, int nch, int first,
                                             int proven = -1) {
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
            if (proven >= 0) r->reserved1 = 1;
        }
        if (E.root_stats) {
            // xq_engine_init_rs: the root's search value over the RAW tree arrays (before pruning and rule 5's counts).  sumN is
            // an exact integer reduction; sumW is one sequential float64 scan in move order over LDS, the same in every lane, so a
            // host model repeats it bit for bit.  L.sw is free here: the action-id sort below rewrites it after the next wave_sync.
            int sum_n = 0;
            for (int i = lane; i < nch; i += 64) { L.sw[i] = T.W[first + i]; sum_n += T.N[first + i]; }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) sum_n += __shfl_xor(sum_n, off);
            wave_sync();
            double sum_w = 0.0;
            for (int i = 0; i < nch; ++i) sum_w += L.sw[i];
            if (lane == 0) {
                xq_sample_root_stats *rs = (xq_sample_root_stats *)(rec + XQ_SAMPLE_ROOT_STATS_OFFSET);
                rs->root_q = proven >= 0 ? 1.0f : (sum_n > 0 ? (float)(sum_w / (double)sum_n) : 0.0f);
                rs->root_visits = (uint32_t)sum_n;
                rs->has_root_stats = 1;
            }
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
    if (proven >= 0) {
        if (full_move) s.n_samples += 1;
        return __builtin_amdgcn_readfirstlane((int)T.A[first + proven]);
    }
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

// SOLVER (proven-result search, xq_engine_init_sv; the rules are include/xq_hip.h's).  The exact value of a decided node, from
// the view of the side that moved into it.
__device__ __forceinline__ double state_value(int st) { return st == NS_WIN ? 1.0 : (st == NS_DRAW ? 0.0 : -1.0); }

// Rule 2: the state of path[depth] has just become `cstate`; go up the recorded path while a state changes.  An UNKNOWN parent of
// a WIN child is LOSS; otherwise, once no child is UNKNOWN, it is DRAW when some child is DRAW and WIN when every child is LOSS.
// One wave pass over the parent's children (at most 128) per changed ancestor.  Returns the number of states set.
__device__ __forceinline__ unsigned wave_propagate(const Tree &T, const int32_t *path, int depth, int cstate) {
    const int lane = lane_id();
    unsigned changed = 0;
    for (int j = depth - 1; j >= 0; --j) {
        const int p = __builtin_amdgcn_readfirstlane(path[j]);
        const int pm = __builtin_amdgcn_readfirstlane((int)T.M[p]);
        if (node_state(pm) != NS_UNKNOWN) break;
        int ns = NS_LOSS;
        if (cstate != NS_WIN) {
            const int f = __builtin_amdgcn_readfirstlane(T.C[p]), nch = pm & XQ_CNT_MASK;
            bool unk = false, drw = false;
            for (int i = lane; i < nch; i += 64) {
                const int st = node_state((int)T.M[f + i]);
                unk = unk || st == NS_UNKNOWN;
                drw = drw || st == NS_DRAW;
            }
            if (__ballot(unk) != 0ull) break;
            ns = __ballot(drw) != 0ull ? NS_DRAW : NS_WIN;
        }
        if (lane == 0) T.M[p] = (uint16_t)(pm | (ns << XQ_STATE_SHIFT));
        wave_sync_mem();   // the next level's pass reads this word from other lanes
        changed += 1;
        cstate = ns;
    }
    return changed;
}

// Rule 5: the counts a move ends with, into L.w_tmp (slot_end_move's lanes read back only what they wrote here): v_i = 0 for a
// LOSS child when some child is not LOSS, else N_i; the proven child of an early end (or -1) gets the unspent simulations; if
// every v_i would be 0, v = N.  Returns the visits taken away.
__device__ __forceinline__ unsigned wave_solver_counts(const Tree &T, SelectLds &L, int nch, int first, int proven, int unspent) {
    const int lane = lane_id();
    int nonloss = 0, sum = 0, rem = 0;
    for (int i = lane; i < nch; i += 64) {
        const int n = T.N[first + i];
        if (node_state((int)T.M[first + i]) == NS_LOSS) rem += n; else { nonloss = 1; sum += n; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { nonloss |= __shfl_xor(nonloss, off); sum += __shfl_xor(sum, off); rem += __shfl_xor(rem, off); }
    const bool zero = nonloss != 0 && sum + unspent > 0;
    for (int i = lane; i < nch; i += 64) {
        int v = (zero && node_state((int)T.M[first + i]) == NS_LOSS) ? 0 : T.N[first + i];
        if (i == proven) v += unspent;
        L.w_tmp[i] = (double)v;
    }
    return zero ? (unsigned)__builtin_amdgcn_readfirstlane(rem) : 0u;
}

// REUSE: hand the chosen child c to k_reroot / k_expand<true> of this step when it was expanded and no drop
// (xq_engine_drop_reroots) ran since this move began; L.a_tmp[i] is child i's action
__device__ __forceinline__ void slot_hand_off(const Slot &s, const SelectLds &L, int nch, int first, int action) {
    const Tree &T = s.T;
    int32_t *gi = s.gi;
    const int lane = s.lane;
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

// The leaf a descent ends on, and the simulated position there (its board and ring are SelectLds.board / .hist)
struct Leaf {
    int node, depth, side, mc, nocap;
    int state;                              // SOLVER: the proven state of the node the descent stopped on (0: an ordinary leaf)
};

// One PUCT descent (mcts.py:126-153) from the root, replaying moves on the LDS board; the nodes passed go to path[0 .. depth].
// VL (leaf batching): each in-flight descent through a node counts as a visit and as a loss for the side choosing there (W is
// from the chooser's view): n = N + vl in q and in 1 + n, w = W - vl, parent count N + vl; vl = 0 gives the plain values exactly.
// FORCED: at a root of prior kind 1 a visited child below its minimum share of the root's visits scores +infinity.
// GUMBEL: at a root of prior kind 3 the candidates are the children whose N equals this simulation's considered-visit count
// (the sequential halving); they score rootP[i] = g_i + l_i plus, once visited, sigma(q_i), everyone else -infinity.  sigma needs
// the maximum of the children's N first: one more pass over the (at most 128) counts and one more wave reduction, at that level only.
//
// SOLVER (proven-result search, xq_engine_init_sv): the descent stops at the first non-root node whose state is not UNKNOWN, and
// a child of state LOSS scores -infinity unless the parent itself is WIN (every child LOSS: the root only, plain PUCT).  The
// states ride in the meta words the descent reads anyway.
//
// One dependent round trip to memory per level: every lane reads, with its candidate child's N / W / P, that child's own
// node words (children count + kind, first child, action) as well, so the winner's are already in a register when the arg-max
// is known -- the next level starts from a lane read instead of three more dependent loads (tM -> tC/tN -> ... -> tA).  The
// winner's N, read here, IS the next level's parent count.
template <bool VL, bool FORCED, bool GUMBEL = false, bool SOLVER = false>
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
    int stop = 0;
    for (;;) {
        const int nch = m & XQ_CNT_MASK, kind = m >> 14;
        if (SOLVER && depth > 0 && node_state(m) != NS_UNKNOWN) { stop = node_state(m); break; }
        if (nch == 0) break;
        const bool skip_loss = SOLVER && node_state(m) != NS_WIN;
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
                if (SOLVER && skip_loss && node_state(cm) == NS_LOSS) ucb = -INFINITY;
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
    return Leaf{node, depth, side, mc, nocap, stop};
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
// Every instance is held to two waves per SIMD.  The FORCED instances came first: left alone, the two with CAP took 256 VGPRs plus
// a few AGPRs and halved their occupancy; then the GUMBEL one, the AROPEN one when the perpetual-check rule joined wave_game_over
// (profiles/r14_perpetual_check_kernel_resource_usage.txt), and the SOLVER ones (profiles/r15_solver_kernel_resource_usage.txt).
// The four plain instances <*, *, 0, 0, 0, 0> stood at 255 / 256 of the 256 VGPRs that two waves allow; the game records' one
// store per real move (slot_log_move) tipped the two with CAP over into AGPRs and one wave, so they are held as well: 250 to 256
// VGPRs, no spill, no scratch (profiles/r18_game_records_kernel_resource_usage.txt).  A change to a shared helper wants that table
// regenerated.
#define XQ_SELECT_OCC __attribute__((amdgpu_waves_per_eu(2, 2)))
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
// SOLVER (proven-result search, xq_engine_init_sv; instances {REUSE} x {CAP}, the plain one for search only and arena games, and
// one with AROPEN): tree nodes carry a proven state in their meta word (rules: include/xq_hip.h).  A terminal leaf sets its state
// from the true result and backs up the exact value, wave_propagate carries it up the path, a descent stops at a decided node,
// LOSS children are skipped, a root with a WIN child ends the move at once, and a move ends on the counts of wave_solver_counts.
template <bool REUSE, bool CAP = false, bool FORCED = false, bool GUMBEL = false, bool AROPEN = false, bool SOLVER = false>
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
    // SOLVER: its counters are bumped in memory where the (rare) events happen -- five more wave-uniform words kept live across
    // the loop cost the AROPEN instance a spilled VGPR
    auto sv_add = [&](int word, unsigned v) {
        if (lane == 0)
            ((unsigned long long *)((char *)E.sqrt_tab + sv_off((size_t)E.cfg.n_games, (size_t)S, AROPEN)))[(size_t)slot * SV_WORDS + word] += v;
    };

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
            slot_log_opening(E, s);
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
        if (SOLVER && node_state(__builtin_amdgcn_readfirstlane((int)T.M[0])) == NS_LOSS) {
            // rule 4, whenever a search looks at its root -- before every simulation, and before the test of the budget, so a
            // reused root that inherits its whole budget plays its proven win too: some root child is WIN (what makes a root LOSS),
            // the move ends at once on the first such child in move order; the unspent simulations are not run and not counted
            const int nch = __builtin_amdgcn_readfirstlane((int)(T.M[0] & XQ_CNT_MASK));
            const int first = __builtin_amdgcn_readfirstlane(T.C[0]);
            int c = -1;
            for (int base = 0; base < nch; base += 64) {
                const unsigned long long b = __ballot(base + lane < nch && node_state((int)T.M[first + base + lane]) == NS_WIN);
                if (b) { c = base + (int)__builtin_ctzll(b); break; }
            }
            c = __builtin_amdgcn_readfirstlane(c);
            if (c < 0) { s.ovf |= 128; c = 0; }              // a LOSS root without a WIN child: a defect
            const int unspent = budget > s.sims_done ? budget - s.sims_done : 0;
            sv_add(SV_MOVES, 1u); sv_add(SV_UNSPENT, (unsigned)unspent);
            if (manual) { phase = PH_HOLD; break; }
            phase = PH_NEWPOS;
            sv_add(SV_REMOVED, wave_solver_counts(T, L, nch, first, c, unspent));     // rule 5, arena moves included
            if (arena) { slot_play(E, s, L, __builtin_amdgcn_readfirstlane((int)T.A[first + c])); continue; }
            const int action = slot_end_move(E, s, L, full_move, true, nch, first, c);
            if (REUSE) slot_hand_off(s, L, nch, first, action);
            slot_play(E, s, L, action);
            if (CAP && !full_move) d_fast_moves += 1;
            continue;
        }
        if (s.sims_done >= budget) {
            if (manual) { phase = PH_HOLD; break; }
            const int nch = __builtin_amdgcn_readfirstlane((int)(T.M[0] & XQ_CNT_MASK));
            const int first = __builtin_amdgcn_readfirstlane(T.C[0]);
            phase = PH_NEWPOS;
            if (SOLVER && arena) {                   // rule 5: the first maximum of v
                sv_add(SV_REMOVED, wave_solver_counts(T, L, nch, first, -1, 0));
                int32_t *v = (int32_t *)L.cdf;
                for (int i = lane; i < nch; i += 64) v[i] = (int)L.w_tmp[i];
                wave_sync();
                int bn;
                const int bi = wave_first_max(v, nch, bn);
                slot_play(E, s, L, __builtin_amdgcn_readfirstlane((int)T.A[first + bi]));
                continue;
            }
            if (arena) { slot_arena_move(E, s, L, nch, first); continue; }
            if (GUMBEL && (__builtin_amdgcn_readfirstlane((int)T.M[0]) >> 14) == 3) {
                unsigned cons, off;
                const int action = slot_end_move_gumbel(E, s, L, rootP, nch, first, cons, off);
                d_gz_moves += 1; d_gz_cons += cons; d_gz_off += off;
                slot_play(E, s, L, action);
                continue;
            }
            const bool pruned = SOLVER || (FORCED && (__builtin_amdgcn_readfirstlane((int)T.M[0]) >> 14) == 1);
            if (SOLVER) sv_add(SV_REMOVED, wave_solver_counts(T, L, nch, first, -1, 0));
            else if (pruned) wave_prune_visits(E, s, L, rootP, fp_k, nch, first);
            const int action = slot_end_move(E, s, L, full_move, pruned, nch, first);
            if (REUSE) slot_hand_off(s, L, nch, first, action);
            slot_play(E, s, L, action);
            if (CAP && !full_move) d_fast_moves += 1;
            continue;
        }
        const Leaf lf = wave_descend<false, FORCED, GUMBEL, SOLVER>(E, s, L, nullptr, rootP, fp_k, path);
        s.d_depth += (unsigned)lf.depth;
        if (SOLVER && lf.state != NS_UNKNOWN) {
            // rule 3: the descent stopped on a decided node -- no terminal test, no request, its exact value backed up
            wave_sync_mem();
            wave_backup<false>(T, nullptr, path, lf.depth, state_value(lf.state));
            wave_sync_mem();
            s.sims_done += 1; s.d_sims += 1; s.d_term += 1; sv_add(SV_STOPS, 1u);
            if (CAP && !full_move) d_fast_sims += 1;
            if (++term_run >= 48) break;
            continue;
        }
        int cnt, winner;
        const int term = wave_game_over(L.board, L.hist, lf.side, lf.mc, lf.nocap, E.perpetual != 0, L.mg, L.moves, &cnt, &winner, &s.ovf);
        if (term) {
            wave_sync_mem();   // path[] stores of lane 0 must be visible to the other lanes
            if (SOLVER) {
                // rule 1: the leaf's state from the TRUE result, seen from the side that moved into it (-lf.side), its exact value
                // backed up (not the reference's "every decided leaf is the mover's win"), then rule 2 up the path
                const int st = winner == 0 ? NS_DRAW : (winner == -lf.side ? NS_WIN : NS_LOSS);
                if (lane == 0 && lf.depth > 0) T.M[lf.node] = (uint16_t)(st << XQ_STATE_SHIFT);
                wave_backup<false>(T, nullptr, path, lf.depth, state_value(st));
                wave_sync_mem();
                sv_add(SV_NODES, 1u + wave_propagate(T, path, lf.depth, st));
            } else {
                wave_backup<false>(T, nullptr, path, lf.depth, terminal_leaf_value(term, winner, lf.side));   // mcts.py:137-140
            }
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
    int root_state = 0;                               // REUSE: the kept root's proven-state bits (0 without xq_engine_init_sv)
    if (REUSE && rr > 0) {
        // node 0 holds the chosen child's words (k_reroot); its children must be this position's legal moves
        const int m0 = __builtin_amdgcn_readfirstlane((int)T.M[0]), f0 = __builtin_amdgcn_readfirstlane(T.C[0]);
        reused = cnt > 0 && (m0 & XQ_CNT_MASK) == cnt && f0 >= 1 && f0 + cnt <= E.node_cap;
        root_state = m0 & (3 << XQ_STATE_SHIFT);
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
                    // the kept root keeps its proven state (bits 12-13: always 0 without xq_engine_init_sv)
                    T.M[0] = (uint16_t)(cnt | root_state | (kind << 14)); T.N[0] = root_sims;
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
    if (!(c_in && cF > c && (cM & XQ_CNT_MASK) > 0 && cF + (cM & XQ_CNT_MASK) <= mark)) {
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
            const int f = tC[x], n = tM[x] & XQ_CNT_MASK;
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
            slot_log_opening(E, s);
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
            const int nch = __builtin_amdgcn_readfirstlane((int)(T.M[0] & XQ_CNT_MASK));
            const int first = __builtin_amdgcn_readfirstlane(T.C[0]);
            if (arena) slot_arena_move(E, s, L, nch, first);
            else slot_play(E, s, L, slot_end_move(E, s, L, true, false, nch, first));
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
        const int term = wave_game_over(L.board, L.hist, lf.side, lf.mc, lf.nocap, E.perpetual != 0, L.mg, L.moves, &cnt, &winner, &s.ovf);
        if (term) {
            wave_sync_mem();   // path[] stores of lane 0 must be visible to the other lanes
            wave_backup<false>(T, nullptr, pathj, lf.depth, terminal_leaf_value(term, winner, lf.side));   // mcts.py:137-140
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
    if (solver_of(eng)) {                              // never Gumbel or forced playouts: instance [CAP][REUSE], or the AROPEN one
        static void (*const ksv[2][2])(Dev, float *) = {
            {k_select<false, false, false, false, false, true>, k_select<true, false, false, false, false, true>},
            {k_select<false, true, false, false, false, true>, k_select<true, true, false, false, false, true>}};
        if (arena_of(eng)) hipLaunchKernelGGL((k_select<false, false, false, false, true, true>), grid, block, 0, s, d, nn_in);
        else hipLaunchKernelGGL(ksv[cap_of(eng)][reuse_of(eng)], grid, block, 0, s, d, nn_in);
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

// Game records (xq_engine_init_gr): the record of every game that stands at PH_FINISHED, one wavefront per slot, launched ahead of
// the select kernel that flushes the game's samples and result and starts the slot's next game over the same log row.  A game is
// finished by an expand kernel, so move count, game number, sample count, winner and reason are the slot's state words.  The
// game takes the next row of the ring while there is one: header and moves copied, the rest of the row zeroed (a drained row
// never shows an earlier game's tail); on a full ring it only counts as dropped.  Its own kernel: inside slot_flush_finished the
// copy cost the select instances registers they do not have (profiles/r18_game_records_kernel_resource_usage.txt).
__global__ __launch_bounds__(64 * WAVES_PER_WG) void k_flush_records(Dev E) {
    const int slot = blockIdx.x * WAVES_PER_WG + (int)(threadIdx.x >> 6);
    if (slot >= E.cfg.n_games) return;
    const int lane = lane_id();
    const int32_t *gi = E.gi + (size_t)slot * GI_N;
    if (__builtin_amdgcn_readfirstlane(gi[GI_PHASE]) != PH_FINISHED) return;
    const size_t G = (size_t)E.cfg.n_games;
    GrHead *h = gr_head(E.gr_log, G);
    const int cap = __builtin_amdgcn_readfirstlane(h->max_out_games);
    unsigned r = 0;
    if (lane == 0) {
        r = atomicAdd(&h->count, 1u);
        atomicAdd(r < (unsigned)cap ? &h->recorded : &h->dropped, 1ull);
    }
    r = __builtin_amdgcn_readfirstlane(r);
    if (r >= (unsigned)cap) return;
    const int mc = __builtin_amdgcn_readfirstlane(gi[GI_MC]);
    const int n = mc < XQ_RECORD_MAX_PLIES ? mc : XQ_RECORD_MAX_PLIES;
    xq_game_record *rec = gr_ring(E.gr_log, (size_t)cap) + r;            // r < cap: inside the ring
    const uint16_t *log = E.gr_log + (size_t)slot * XQ_RECORD_MAX_PLIES;
    for (int i = lane; i < XQ_RECORD_MAX_PLIES; i += 64) rec->moves[i] = i < n ? log[i] : (uint16_t)0;
    if (lane == 0) {
        rec->slot = (uint32_t)slot; rec->game_seq = (uint32_t)gi[GI_GSEQ]; rec->winner = (int8_t)gi[GI_FWINNER];
        rec->reason = (uint8_t)gi[GI_FREASON]; rec->n_moves = (uint16_t)mc;
        rec->opening_plies = gr_opening(E.gr_log, G)[slot]; rec->n_samples = (uint16_t)gi[GI_NSAMP];
    }
}

// Start-position pool (xq_engine_init_sp): one wavefront per slot, launched ahead of the select kernel.  A slot that stands at
// PH_FINISHED, or at PH_NEWGAME with its stagger run down, is where a game begins: the finished game is flushed as the select
// kernel flushes it, then the stateless draw for the game that will carry game_seq + 1 says where from.  Not from the pool: the
// slot is left at PH_NEWGAME and the select kernel starts the game as ever.  From the pool: what slot_new_game does, with the
// entry in place of the initial board and no opening -- the quota ticket, the new game's state words, the entry's board to the
// slot's row (its side, byte 90, and the padding masked to zero, as init_board_lds leaves them), an empty history -- and the slot
// goes to PH_NEWPOS: the select kernel issues the root request.  The rows are copied global to global, so the kernel needs no LDS
// at all.  Its own kernel ahead of k_select, not a branch of slot_new_game: the select instances have no register to spare
// (XQ_SELECT_OCC), and so no existing kernel's arguments or code change.
__global__ __launch_bounds__(64 * WAVES_PER_WG) void k_start_pool(Dev E, SpDev P) {
    const int slot = blockIdx.x * WAVES_PER_WG + (int)(threadIdx.x >> 6);
    if (slot >= E.cfg.n_games) return;
    const int lane = lane_id();
    Slot s;
    s.slot = slot; s.lane = lane; s.gi = E.gi + (size_t)slot * GI_N; s.st = E.stats + (size_t)slot * ST_N; s.T = slot_tree(E, slot);
    int32_t *gi = s.gi;
    const int phase = __builtin_amdgcn_readfirstlane(gi[GI_PHASE]);
    if (phase != PH_FINISHED && phase != PH_NEWGAME) return;
    if (__builtin_amdgcn_readfirstlane(gi[GI_DELAY]) > 0) return;      // start_stagger: the select kernel keeps the countdown
    slot_load(s);
    if (phase == PH_FINISHED) slot_flush_finished(E, s);
    const int n = __builtin_amdgcn_readfirstlane(P.head->n);
    const int idx = start_pool_draw(E.cfg.seed, (uint32_t)E.cfg.rank, (uint32_t)slot, (uint32_t)(s.game_seq + 1), n, P.head->prob);
    if (idx < 0 || idx >= n) {                         // the initial position (idx >= n: n < 1, which init never lets in)
        if (lane == 0) { gi[GI_PHASE] = PH_NEWGAME; P.start_index[slot] = -1; }
        return;
    }
    unsigned long long ticket = 0;
    if (lane == 0) ticket = atomicAdd(E.started, 1ull);
    ticket = ((unsigned long long)__builtin_amdgcn_readfirstlane((unsigned)(ticket >> 32)) << 32) |
             (unsigned)__builtin_amdgcn_readfirstlane((unsigned)ticket);
    if (E.cfg.games_target > 0 && ticket >= (unsigned long long)E.cfg.games_target) {
        if (lane == 0) gi[GI_PHASE] = PH_IDLE;         // the games quota is used up: the slot idles
        return;
    }
    const uint32_t *row = (const uint32_t *)(sp_rows(P.start_index, (size_t)n) + (size_t)idx * XQ_BS);
    const int side = (int)(int8_t)(__builtin_amdgcn_readfirstlane((int)row[22]) >> 16);
    uint32_t *board = (uint32_t *)(E.board + (size_t)slot * XQ_BS);
    if (lane < XQ_BS / 4) board[lane] = lane < 22 ? row[lane] : (lane == 22 ? row[22] & 0xFFFFu : 0u);
    uint32_t *hist = (uint32_t *)(E.hist + (size_t)slot * XQ_HIST * XQ_BS);
    for (int i = lane; i < XQ_HIST * XQ_BS / 4; i += 64) hist[i] = 0u;
    if (lane == 0) {
        gi[GI_SIDE] = side; gi[GI_MC] = 0; gi[GI_NOCAP] = 0; gi[GI_NSAMP] = 0; gi[GI_GSEQ] = s.game_seq + 1;
        gi[GI_RESIGN_N] = 0; gi[GI_RR_NODE] = 0; gi[GI_PHASE] = PH_NEWPOS;
        s.st[ST_STARTED] += 1;
        P.start_index[slot] = idx;
        atomicAdd(&P.head->pool_games, 1ull);
    }
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

int xq_engine_select(const xq_engine *eng, float *dev_nn_input, void *stream) {
    if (!eng || !dev_nn_input) return XQ_ERR_ARG;
    const Dev d = make_dev(eng);
    if (d.gr_log) {
        // game records: the finished games' records first, before the select kernel starts the slots' next games
        hipLaunchKernelGGL(k_flush_records, dim3((eng->cfg.n_games + WAVES_PER_WG - 1) / WAVES_PER_WG), dim3(64 * WAVES_PER_WG), 0,
                           (hipStream_t)stream, d);
        const int rc = launch_status();
        if (rc != XQ_OK) return rc;
    }
    if (pool_of(eng)) {
        // start-position pool: the games that start from a pool entry first; the select kernel starts the others
        hipLaunchKernelGGL(k_start_pool, dim3((eng->cfg.n_games + WAVES_PER_WG - 1) / WAVES_PER_WG), dim3(64 * WAVES_PER_WG), 0,
                           (hipStream_t)stream, d, make_sp(eng));
        const int rc = launch_status();
        if (rc != XQ_OK) return rc;
    }
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

}  // extern "C"
