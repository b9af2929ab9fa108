// xq_engine_setup.hip -- the engine's set-up and host-side readers (map: xq_engine.hip): the workspace layout, the option checks,
// every xq_engine_workspace_bytes* and xq_engine_init* entry point, the init kernels, and stats / drain / set_position / read_root.
#include "xq_engine_state.cuh"

#pragma clang fp contract(off)

namespace {

// An engine's options as one record.  Every xq_engine_workspace_bytes* / xq_engine_init* entry point is the widest one with the
// options it does not take absent (K = 1, no flags, NULL), so each builds this record and shares opts_ok, make_layout and engine_init.
struct Opts {
    int K;                          // leaves per step
    unsigned flags;                 // XQ_ENGINE_*
    const xq_playout_cap *cap;
    const xq_forced_playouts *forced;
    const xq_gumbel *gumbel;
    const xq_arena_opts *arena;
    const xq_rules_opts *rules;     // absent from an initialiser: NULL, the reference's rules
    const xq_solver_opts *solver;   // absent, NULL or enabled = 0: no proven-result search
    const xq_root_stats_opts *root_stats;   // absent, NULL or enabled = 0: the samples' pad bytes stay zero
    const xq_eval_mirror_opts *mirror;      // absent, NULL or mode = 0: every request is evaluated as it stands
    const xq_game_records_opts *records;    // absent, NULL or enabled = 0: no game is recorded
    const xq_start_pool *pool;              // absent, NULL or n = 0: every game starts from the initial position
    bool pool_on() const { return pool && pool->n != 0; }
    bool solver_on() const { return solver && solver->enabled != 0; }
    bool mirror_on() const { return mirror && mirror->mode != 0; }
    bool root_stats_on() const { return root_stats && root_stats->enabled != 0; }
    bool records_on() const { return records && records->enabled != 0; }
};

struct Layout {
    size_t off[32];
    size_t total;
    int node_cap, path_cap, stage_cap;
};

// the option words of an engine with these options: THE OPTION WORDS of xq_engine_state.cuh filled in, a block the engine has
// not left {0, 0}.  make_layout, engine_init and xq_engine_option_words_sp all read this one record.
xq_option_words option_words(const xq_engine_config *c, const Opts &o) {
    const size_t G = (size_t)c->n_games, S = (size_t)c->num_simulations, K = (size_t)o.K;
    const size_t m = o.gumbel ? (size_t)o.gumbel->considered : 0, M = o.records_on() ? (size_t)o.records->max_out_games : 0,
                 n = o.pool_on() ? (size_t)o.pool->n : 0;
    const bool arena = o.arena != nullptr, solver = o.solver_on();
    xq_option_words w;
    memset(&w, 0, sizeof(w));
    w.table = {0, ow_table_bytes(S, K)};
    if (m) {
        w.gz_head = {ow_gz_head(S), sizeof(GzHead)}; w.gz_vhat = {ow_gz_vhat(S), G * 8}; w.gz_visits = {ow_gz_visits(G, S), m * S * 2};
    }
    if (arena) {
        const ArOff a = ar_off(G, S);
        w.ar_head = {a.head, sizeof(ArHead)}; w.ar_op_counts = {a.op_counts, G * 4};
        w.ar_op_actions = {a.op_actions, G * XQ_ARENA_MAX_OPENING * 2}; w.ar_n_live = {a.n_live, 2 * 4};
        for (int i = 0; i < 2; ++i) {
            w.ar_rows[i] = {a.rows[i], G * 4}; w.ar_x[i] = {a.x[i], G * XQ_STATE_FLOATS * 4};
            w.ar_moves[i] = {a.moves[i], G * XQ_MAXM * 2}; w.ar_counts[i] = {a.counts[i], G * 4};
        }
    }
    if (solver) w.solver = {sv_off(G, S, arena), sv_bytes(G)};
    const size_t end = ow_region_bytes(ow_front_end(G, S, K, m, arena, solver), G, M, n);
    w.bytes = end;
    if (M) {
        w.gr_ring = {ow_gr_ring(end, G, M), M * XQ_RECORD_BYTES}; w.gr_log = {ow_gr_log(end, G), G * XQ_RECORD_MAX_PLIES * 2};
        w.gr_opening = {ow_gr_opening(end, G), G * 2}; w.gr_head = {ow_tail_head(end), sizeof(GrHead)};
    } else if (n) {
        w.sp_rows = {ow_sp_rows(end, G, n), n * XQ_BS}; w.sp_index = {ow_sp_index(end, G), G * 4};
        w.sp_head = {ow_tail_head(end), sizeof(SpHead)};
    }
    return w;
}

// K > 1 (leaf batching): the request rows (moves, counts, paths, packed buffers) are G K, slot-major; the virtual-loss
// counters and the pending-leaf records follow the K = 1 layout, which is unchanged.  The square-root table's region holds every
// option's words (option_words): only an engine with such an option grows there.
Layout make_layout(const xq_engine_config *c, const Opts &opts) {
    const int K = opts.K;
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
    put(P_SQRT, option_words(c, opts).bytes);
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

// tree reuse: self-play only, one leaf per step, S within k_reroot's LDS (64 KiB at S = XQ_REUSE_MAX_SIMS).  Any other bit is
// refused, so no caller's flag reaches the private bits of the handle's flag byte (PAD0_GAME_RECORDS, PAD0_START_POOL)
static_assert((((unsigned)XQ_ENGINE_TREE_REUSE << 16) & (unsigned)(PAD0_GAME_RECORDS | PAD0_START_POOL)) == 0, "private pad0 bits");
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

// rules options: perpetual_check 0 or 1, reserved words zero; they go with every mode and every other option
bool rules_ok(const xq_rules_opts *r) {
    return (r->perpetual_check == 0 || r->perpetual_check == 1) && r->reserved[0] == 0 && r->reserved[1] == 0 && r->reserved[2] == 0;
}

// proven-result search: enabled 0 or 1, reserved words zero; on, it needs one leaf per step and goes with neither Gumbel root
// search (its equal-visit candidates cannot skip a child) nor forced playouts
bool solver_ok(const Opts &o) {
    const xq_solver_opts *sv = o.solver;
    if ((sv->enabled != 0 && sv->enabled != 1) || sv->reserved[0] != 0 || sv->reserved[1] != 0 || sv->reserved[2] != 0) return false;
    return sv->enabled == 0 || (o.K == 1 && !o.gumbel && !o.forced);
}

// root statistics per sample: enabled 0 or 1, reserved words zero; on, it needs an engine that records samples (self-play) and
// goes with everything but Gumbel root search, whose root value is its own v_mix
bool root_stats_ok(const xq_engine_config *c, const Opts &o) {
    const xq_root_stats_opts *rs = o.root_stats;
    if ((rs->enabled != 0 && rs->enabled != 1) || rs->reserved[0] != 0 || rs->reserved[1] != 0 || rs->reserved[2] != 0) return false;
    return rs->enabled == 0 || (c && c->manual_moves == 0 && !o.gumbel);
}

// evaluation mirror: mode 0 or 1, reserved words zero; on, it goes with everything but arena games, whose gate stays deterministic
// and whose per-model packed step shares k_gather_rows
bool mirror_ok(const xq_engine_config *c, const Opts &o) {
    const xq_eval_mirror_opts *em = o.mirror;
    if ((em->mode != 0 && em->mode != 1) || em->reserved[0] != 0 || em->reserved[1] != 0 || em->reserved[2] != 0) return false;
    return em->mode == 0 || (c && c->manual_moves != 2);
}

// game records: enabled 0 or 1, reserved words zero; on, a ring of at least one record, an engine that plays games, and games
// that fit a record
bool records_ok(const xq_engine_config *c, const Opts &o) {
    const xq_game_records_opts *gr = o.records;
    if ((gr->enabled != 0 && gr->enabled != 1) || gr->reserved[0] != 0 || gr->reserved[1] != 0) return false;
    if (gr->enabled == 0) return true;
    return gr->max_out_games >= 1 && c && c->manual_moves != 1 && c->max_game_length <= XQ_RECORD_MAX_PLIES &&
           c->random_opening_moves <= XQ_RECORD_MAX_PLIES;
}

// start-position pool: 0 <= n <= XQ_START_POOL_MAX, reserved zero; n = 0 is off; on, prob in (0, 1] (a NaN fails both
// comparisons), both arrays, a self-play engine, no game records
bool pool_ok(const xq_engine_config *c, const Opts &o) {
    const xq_start_pool *sp = o.pool;
    if (sp->n < 0 || sp->n > XQ_START_POOL_MAX || sp->reserved != 0) return false;
    if (sp->n == 0) return true;
    return sp->prob > 0.0 && sp->prob <= 1.0 && sp->dev_boards && sp->dev_side && c && c->manual_moves == 0 && !o.records_on();
}

// every option check, in the order the entry points have always refused in; an absent option passes
bool opts_ok(const xq_engine_config *c, const Opts &o) {
    if (o.pool && !pool_ok(c, o)) return false;
    if (o.rules && !rules_ok(o.rules)) return false;
    if (o.solver && !solver_ok(o)) return false;
    if (o.root_stats && !root_stats_ok(c, o)) return false;
    if (o.mirror && !mirror_ok(c, o)) return false;
    if (o.records && !records_ok(c, o)) return false;
    if (!config_ok(c) || !leaves_ok(c, o.K) || !flags_ok(c, o.K, o.flags)) return false;
    if (o.cap && !cap_ok(c, o.K, o.cap)) return false;
    if (o.forced && !forced_ok(c, o.K, o.forced)) return false;
    if (o.gumbel && !gumbel_ok(c, o.K, o.flags, o.cap, o.forced, o.gumbel)) return false;
    return !o.arena || arena_ok(c, o.arena);
}

// tree reuse, the playout cap, forced playouts and the evaluation mirror need no workspace of their own
size_t workspace_bytes(const xq_engine_config *cfg, const Opts &o) { return opts_ok(cfg, o) ? make_layout(cfg, o).total : 0; }

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

// xq_engine_init_sp: the caller's pool as the workspace's 96-byte rows, one thread per byte: the board, its side in byte 90, zeros
__global__ void k_init_pool(const int8_t *__restrict__ boards, const int8_t *__restrict__ side, int n, int8_t *__restrict__ rows) {
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long j = gid / XQ_BS;
    const int b = (int)(gid - j * XQ_BS);
    if (j >= n) return;
    rows[gid] = b < 90 ? boards[(size_t)j * 90 + b] : (b == 90 ? side[j] : (int8_t)0);
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

// the one implementation behind every xq_engine_init*
int engine_init(xq_engine *eng, const xq_engine_config *cfg, const Opts &o, void *ws, size_t ws_bytes, const uint64_t *dev_inject,
                void *stream) {
    if (!eng || !opts_ok(cfg, o) || !ws || ((uintptr_t)ws & 255)) return XQ_ERR_ARG;
    if (cfg->inject_len > 0 && !dev_inject) return XQ_ERR_ARG;
    const int K = o.K;
    const Layout l = make_layout(cfg, o);
    if (ws_bytes < l.total) return XQ_ERR_WORKSPACE;
    if (o.pool_on()) {
        // the pool is checked before anything else is written: its status bytes borrow the head of the workspace (n <= the
        // pool's own rows), and an entry with a fatal bit refuses the engine
        const size_t n = (size_t)o.pool->n;
        int rc = xq_positions_check_batch(o.pool->dev_boards, o.pool->dev_side, o.pool->n, (uint8_t *)ws, stream);
        if (rc != XQ_OK) return rc;
        uint8_t *st = (uint8_t *)malloc(n);
        if (!st) return XQ_ERR_ARG;
        rc = xq::check(hipMemcpyAsync(st, ws, n, hipMemcpyDeviceToHost, (hipStream_t)stream));
        if (rc == XQ_OK) rc = xq::check(hipStreamSynchronize((hipStream_t)stream));
        for (size_t i = 0; rc == XQ_OK && i < n; ++i)
            if (st[i] & XQ_POSITION_FATAL) rc = XQ_ERR_ARG;
        free(st);
        if (rc != XQ_OK) return rc;
    }
    memset(eng, 0, sizeof(*eng));
    eng->cfg = *cfg;
    eng->node_cap = l.node_cap; eng->path_cap = l.path_cap; eng->stage_cap = l.stage_cap;
    eng->pad0 = (K > 1 ? K : 0) | (int)(o.flags << 16) | (o.cap ? PAD0_CAP : 0) | (o.forced ? PAD0_FORCED : 0) |
                (o.gumbel ? PAD0_GUMBEL : 0) | (o.arena ? PAD0_ARENA : 0) |
                (o.rules && o.rules->perpetual_check ? PAD0_PERPETUAL : 0) | (o.solver_on() ? PAD0_SOLVER : 0) |
                (o.root_stats_on() ? PAD0_ROOT_STATS : 0) | (o.mirror_on() ? PAD0_EVAL_MIRROR : 0) |
                (o.records_on() ? PAD0_GAME_RECORDS : 0) | (o.pool_on() ? PAD0_START_POOL : 0);
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
    const xq_option_words w = option_words(cfg, o);
    char *words = (char *)eng->p[P_SQRT];
    {
        // arena options: their words zeroed whole (openings record, both sets' counts and rows); the solver's counters zeroed
        if (o.arena) XQ_TRY(hipMemsetAsync(words, 0, ar_off((size_t)cfg->n_games, (size_t)cfg->num_simulations).end, s));
        if (o.solver_on()) XQ_TRY(hipMemsetAsync(words + w.solver.offset, 0, w.solver.bytes, s));
        // one host image: the table (K > 1: N_parent + vl_parent < S + K) and, behind it, the Gumbel words (the parameters, a zeroed
        // v_hat per slot, the considered-visit tables for k = 1 .. m) or the arena's parameters
        const size_t bytes = o.arena ? w.ar_head.offset + w.ar_head.bytes : o.gumbel ? w.gz_visits.offset + w.gz_visits.bytes : w.table.bytes;
        char *img = (char *)calloc(bytes, 1);
        if (!img) return XQ_ERR_ARG;
        for (size_t i = 0; i < w.table.bytes / 8; ++i) ((double *)img)[i] = sqrt((double)i);   // math.sqrt(visit_count), mcts.py:49
        if (o.gumbel) {
            GzHead *h = (GzHead *)(img + w.gz_head.offset);
            h->m = o.gumbel->considered; h->c_visit = (float)o.gumbel->c_visit; h->c_scale = (float)o.gumbel->c_scale;
            const int S = cfg->num_simulations;
            for (int k = 1; k <= o.gumbel->considered; ++k) gz_considered_visits(k, S, (uint16_t *)(img + w.gz_visits.offset) + (size_t)(k - 1) * S);
        }
        if (o.arena) {
            ArHead *h = (ArHead *)(img + w.ar_head.offset);
            h->opening_plies = o.arena->opening_plies; h->first_game = o.arena->first_game;
        }
        const int rc = xq::check(hipMemcpyAsync(words, img, bytes, hipMemcpyHostToDevice, s));
        if (rc == XQ_OK) (void)hipStreamSynchronize(s);
        free(img);
        if (rc != XQ_OK) return rc;
    }
    const Dev d = make_dev(eng);
    if (o.records_on()) {
        // game records: the ring, the log, the opening counts and the head zeroed, then the ring's size
        XQ_TRY(hipMemsetAsync(words + w.gr_ring.offset, 0, w.bytes - w.gr_ring.offset, s));
        XQ_TRY(hipMemcpyAsync(words + w.gr_head.offset + offsetof(GrHead, max_out_games), &o.records->max_out_games, 4, hipMemcpyHostToDevice, s));
        XQ_TRY(hipStreamSynchronize(s));
    }
    if (o.pool_on()) {
        // start-position pool: the checked entries as rows, every slot's index -1, then the head
        SpHead h;
        memset(&h, 0, sizeof(h));
        h.n = o.pool->n; h.prob = o.pool->prob;
        const long long threads = (long long)o.pool->n * XQ_BS;
        hipLaunchKernelGGL(k_init_pool, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, o.pool->dev_boards, o.pool->dev_side,
                           o.pool->n, (int8_t *)(words + w.sp_rows.offset));
        const int rc = launch_status();
        if (rc != XQ_OK) return rc;
        XQ_TRY(hipMemsetAsync(words + w.sp_index.offset, 0xFF, w.sp_head.offset - w.sp_index.offset, s));
        XQ_TRY(hipMemcpyAsync(words + w.sp_head.offset, &h, sizeof(h), hipMemcpyHostToDevice, s));
        XQ_TRY(hipStreamSynchronize(s));
    }
    hipLaunchKernelGGL(k_init, dim3((cfg->n_games + 255) / 256), dim3(256), 0, s, d);
    if (o.cap) {
        const int rc = launch_status();
        if (rc != XQ_OK) return rc;
        hipLaunchKernelGGL(k_init_cap, dim3((cfg->n_games + 255) / 256), dim3(256), 0, s, d, (int)o.cap->fast_simulations,
                           o.cap->full_search_prob);
    }
    if (o.forced) {
        const int rc = launch_status();
        if (rc != XQ_OK) return rc;
        hipLaunchKernelGGL(k_init_fp, dim3((cfg->n_games + 255) / 256), dim3(256), 0, s, d, (float)o.forced->k);
    }
    return launch_status();
}

}  // namespace

extern "C" {

size_t xq_engine_workspace_bytes(const xq_engine_config *cfg) { return workspace_bytes(cfg, Opts{1, 0u, nullptr, nullptr, nullptr, nullptr}); }

size_t xq_engine_workspace_bytes_leaves(const xq_engine_config *cfg, int leaves_per_step) {
    return workspace_bytes(cfg, Opts{leaves_per_step, 0u, nullptr, nullptr, nullptr, nullptr});
}

size_t xq_engine_workspace_bytes_ex(const xq_engine_config *cfg, int leaves_per_step, unsigned flags) {
    return workspace_bytes(cfg, Opts{leaves_per_step, flags, nullptr, nullptr, nullptr, nullptr});
}

size_t xq_engine_workspace_bytes_cap(const xq_engine_config *cfg, int leaves_per_step, unsigned flags, const xq_playout_cap *cap) {
    return workspace_bytes(cfg, Opts{leaves_per_step, flags, cap, nullptr, nullptr, nullptr});
}

size_t xq_engine_workspace_bytes_fp(const xq_engine_config *cfg, int leaves_per_step, unsigned flags, const xq_playout_cap *cap,
                                    const xq_forced_playouts *forced) {
    return workspace_bytes(cfg, Opts{leaves_per_step, flags, cap, forced, nullptr, nullptr});
}

size_t xq_engine_workspace_bytes_gz(const xq_engine_config *cfg, int leaves_per_step, unsigned flags, const xq_playout_cap *cap,
                                    const xq_forced_playouts *forced, const xq_gumbel *gumbel) {
    return workspace_bytes(cfg, Opts{leaves_per_step, flags, cap, forced, gumbel, nullptr});
}

size_t xq_engine_workspace_bytes_ar(const xq_engine_config *cfg, int leaves_per_step, unsigned flags, const xq_playout_cap *cap,
                                    const xq_forced_playouts *forced, const xq_gumbel *gumbel, const xq_arena_opts *arena) {
    return workspace_bytes(cfg, Opts{leaves_per_step, flags, cap, forced, gumbel, arena});
}

size_t xq_engine_workspace_bytes_ru(const xq_engine_config *cfg, int leaves_per_step, unsigned flags, const xq_playout_cap *cap,
                                    const xq_forced_playouts *forced, const xq_gumbel *gumbel, const xq_arena_opts *arena,
                                    const xq_rules_opts *rules) {
    return workspace_bytes(cfg, Opts{leaves_per_step, flags, cap, forced, gumbel, arena, rules});
}

size_t xq_engine_workspace_bytes_sv(const xq_engine_config *cfg, int leaves_per_step, unsigned flags, const xq_playout_cap *cap,
                                    const xq_forced_playouts *forced, const xq_gumbel *gumbel, const xq_arena_opts *arena,
                                    const xq_rules_opts *rules, const xq_solver_opts *solver) {
    return workspace_bytes(cfg, Opts{leaves_per_step, flags, cap, forced, gumbel, arena, rules, solver});
}

size_t xq_engine_workspace_bytes_rs(const xq_engine_config *cfg, int leaves_per_step, unsigned flags, const xq_playout_cap *cap,
                                    const xq_forced_playouts *forced, const xq_gumbel *gumbel, const xq_arena_opts *arena,
                                    const xq_rules_opts *rules, const xq_solver_opts *solver, const xq_root_stats_opts *root_stats) {
    return workspace_bytes(cfg, Opts{leaves_per_step, flags, cap, forced, gumbel, arena, rules, solver, root_stats});
}

size_t xq_engine_workspace_bytes_em(const xq_engine_config *cfg, int leaves_per_step, unsigned flags, const xq_playout_cap *cap,
                                    const xq_forced_playouts *forced, const xq_gumbel *gumbel, const xq_arena_opts *arena,
                                    const xq_rules_opts *rules, const xq_solver_opts *solver, const xq_root_stats_opts *root_stats,
                                    const xq_eval_mirror_opts *mirror) {
    return workspace_bytes(cfg, Opts{leaves_per_step, flags, cap, forced, gumbel, arena, rules, solver, root_stats, mirror});
}

size_t xq_engine_workspace_bytes_gr(const xq_engine_config *cfg, int leaves_per_step, unsigned flags, const xq_playout_cap *cap,
                                    const xq_forced_playouts *forced, const xq_gumbel *gumbel, const xq_arena_opts *arena,
                                    const xq_rules_opts *rules, const xq_solver_opts *solver, const xq_root_stats_opts *root_stats,
                                    const xq_eval_mirror_opts *mirror, const xq_game_records_opts *records) {
    return workspace_bytes(cfg, Opts{leaves_per_step, flags, cap, forced, gumbel, arena, rules, solver, root_stats, mirror, records});
}

int xq_gumbel_considered_visits_host(int k, int num_simulations, uint16_t *host_out) {
    if (k < 1 || k > XQ_MAXM || num_simulations < 1 || num_simulations > 65535 || !host_out) return XQ_ERR_ARG;
    gz_considered_visits(k, num_simulations, host_out);
    return XQ_OK;
}

int xq_engine_init(xq_engine *eng, const xq_engine_config *cfg, void *ws, size_t ws_bytes, const uint64_t *dev_inject,
                   void *stream) {
    return engine_init(eng, cfg, Opts{1, 0u, nullptr, nullptr, nullptr, nullptr}, ws, ws_bytes, dev_inject, stream);
}

int xq_engine_init_leaves(xq_engine *eng, const xq_engine_config *cfg, int leaves_per_step, void *ws, size_t ws_bytes,
                          const uint64_t *dev_inject, void *stream) {
    return engine_init(eng, cfg, Opts{leaves_per_step, 0u, nullptr, nullptr, nullptr, nullptr}, ws, ws_bytes, dev_inject, stream);
}

int xq_engine_init_ex(xq_engine *eng, const xq_engine_config *cfg, int leaves_per_step, unsigned flags, void *ws,
                      size_t ws_bytes, const uint64_t *dev_inject, void *stream) {
    return engine_init(eng, cfg, Opts{leaves_per_step, flags, nullptr, nullptr, nullptr, nullptr}, ws, ws_bytes, dev_inject, stream);
}

int xq_engine_init_cap(xq_engine *eng, const xq_engine_config *cfg, int leaves_per_step, unsigned flags, const xq_playout_cap *cap,
                       void *ws, size_t ws_bytes, const uint64_t *dev_inject, void *stream) {
    return engine_init(eng, cfg, Opts{leaves_per_step, flags, cap, nullptr, nullptr, nullptr}, ws, ws_bytes, dev_inject, stream);
}

int xq_engine_init_fp(xq_engine *eng, const xq_engine_config *cfg, int leaves_per_step, unsigned flags, const xq_playout_cap *cap,
                      const xq_forced_playouts *forced, void *ws, size_t ws_bytes, const uint64_t *dev_inject, void *stream) {
    return engine_init(eng, cfg, Opts{leaves_per_step, flags, cap, forced, nullptr, nullptr}, ws, ws_bytes, dev_inject, stream);
}

int xq_engine_init_gz(xq_engine *eng, const xq_engine_config *cfg, int leaves_per_step, unsigned flags, const xq_playout_cap *cap,
                      const xq_forced_playouts *forced, const xq_gumbel *gumbel, void *ws, size_t ws_bytes,
                      const uint64_t *dev_inject, void *stream) {
    return engine_init(eng, cfg, Opts{leaves_per_step, flags, cap, forced, gumbel, nullptr}, ws, ws_bytes, dev_inject, stream);
}

int xq_engine_init_ar(xq_engine *eng, const xq_engine_config *cfg, int leaves_per_step, unsigned flags, const xq_playout_cap *cap,
                      const xq_forced_playouts *forced, const xq_gumbel *gumbel, const xq_arena_opts *arena, void *ws,
                      size_t ws_bytes, const uint64_t *dev_inject, void *stream) {
    return engine_init(eng, cfg, Opts{leaves_per_step, flags, cap, forced, gumbel, arena}, ws, ws_bytes, dev_inject, stream);
}

int xq_engine_init_ru(xq_engine *eng, const xq_engine_config *cfg, int leaves_per_step, unsigned flags, const xq_playout_cap *cap,
                      const xq_forced_playouts *forced, const xq_gumbel *gumbel, const xq_arena_opts *arena,
                      const xq_rules_opts *rules, void *ws, size_t ws_bytes, const uint64_t *dev_inject, void *stream) {
    return engine_init(eng, cfg, Opts{leaves_per_step, flags, cap, forced, gumbel, arena, rules}, ws, ws_bytes, dev_inject, stream);
}

int xq_engine_init_sv(xq_engine *eng, const xq_engine_config *cfg, int leaves_per_step, unsigned flags, const xq_playout_cap *cap,
                      const xq_forced_playouts *forced, const xq_gumbel *gumbel, const xq_arena_opts *arena,
                      const xq_rules_opts *rules, const xq_solver_opts *solver, void *ws, size_t ws_bytes, const uint64_t *dev_inject,
                      void *stream) {
    return engine_init(eng, cfg, Opts{leaves_per_step, flags, cap, forced, gumbel, arena, rules, solver}, ws, ws_bytes, dev_inject,
                       stream);
}

int xq_engine_init_rs(xq_engine *eng, const xq_engine_config *cfg, int leaves_per_step, unsigned flags, const xq_playout_cap *cap,
                      const xq_forced_playouts *forced, const xq_gumbel *gumbel, const xq_arena_opts *arena,
                      const xq_rules_opts *rules, const xq_solver_opts *solver, const xq_root_stats_opts *root_stats, void *ws,
                      size_t ws_bytes, const uint64_t *dev_inject, void *stream) {
    return engine_init(eng, cfg, Opts{leaves_per_step, flags, cap, forced, gumbel, arena, rules, solver, root_stats}, ws, ws_bytes,
                       dev_inject, stream);
}

int xq_engine_init_em(xq_engine *eng, const xq_engine_config *cfg, int leaves_per_step, unsigned flags, const xq_playout_cap *cap,
                      const xq_forced_playouts *forced, const xq_gumbel *gumbel, const xq_arena_opts *arena,
                      const xq_rules_opts *rules, const xq_solver_opts *solver, const xq_root_stats_opts *root_stats,
                      const xq_eval_mirror_opts *mirror, void *ws, size_t ws_bytes, const uint64_t *dev_inject, void *stream) {
    return engine_init(eng, cfg, Opts{leaves_per_step, flags, cap, forced, gumbel, arena, rules, solver, root_stats, mirror}, ws,
                       ws_bytes, dev_inject, stream);
}

int xq_engine_init_gr(xq_engine *eng, const xq_engine_config *cfg, int leaves_per_step, unsigned flags, const xq_playout_cap *cap,
                      const xq_forced_playouts *forced, const xq_gumbel *gumbel, const xq_arena_opts *arena,
                      const xq_rules_opts *rules, const xq_solver_opts *solver, const xq_root_stats_opts *root_stats,
                      const xq_eval_mirror_opts *mirror, const xq_game_records_opts *records, void *ws, size_t ws_bytes,
                      const uint64_t *dev_inject, void *stream) {
    return engine_init(eng, cfg, Opts{leaves_per_step, flags, cap, forced, gumbel, arena, rules, solver, root_stats, mirror, records},
                       ws, ws_bytes, dev_inject, stream);
}

size_t xq_engine_workspace_bytes_sp(const xq_engine_config *cfg, int leaves_per_step, unsigned flags, const xq_playout_cap *cap,
                                    const xq_forced_playouts *forced, const xq_gumbel *gumbel, const xq_arena_opts *arena,
                                    const xq_rules_opts *rules, const xq_solver_opts *solver, const xq_root_stats_opts *root_stats,
                                    const xq_eval_mirror_opts *mirror, const xq_game_records_opts *records,
                                    const xq_start_pool *pool) {
    return workspace_bytes(cfg, Opts{leaves_per_step, flags, cap, forced, gumbel, arena, rules, solver, root_stats, mirror, records, pool});
}

int xq_engine_option_words_sp(const xq_engine_config *cfg, int leaves_per_step, unsigned flags, const xq_playout_cap *cap,
                              const xq_forced_playouts *forced, const xq_gumbel *gumbel, const xq_arena_opts *arena,
                              const xq_rules_opts *rules, const xq_solver_opts *solver, const xq_root_stats_opts *root_stats,
                              const xq_eval_mirror_opts *mirror, const xq_game_records_opts *records, const xq_start_pool *pool,
                              xq_option_words *out) {
    const Opts o{leaves_per_step, flags, cap, forced, gumbel, arena, rules, solver, root_stats, mirror, records, pool};
    if (!out || !opts_ok(cfg, o)) return XQ_ERR_ARG;
    *out = option_words(cfg, o);
    return XQ_OK;
}

int xq_engine_init_sp(xq_engine *eng, const xq_engine_config *cfg, int leaves_per_step, unsigned flags, const xq_playout_cap *cap,
                      const xq_forced_playouts *forced, const xq_gumbel *gumbel, const xq_arena_opts *arena,
                      const xq_rules_opts *rules, const xq_solver_opts *solver, const xq_root_stats_opts *root_stats,
                      const xq_eval_mirror_opts *mirror, const xq_game_records_opts *records, const xq_start_pool *pool, void *ws,
                      size_t ws_bytes, const uint64_t *dev_inject, void *stream) {
    return engine_init(eng, cfg, Opts{leaves_per_step, flags, cap, forced, gumbel, arena, rules, solver, root_stats, mirror, records, pool},
                       ws, ws_bytes, dev_inject, stream);
}

int xq_start_pool_draw_host(uint64_t seed, int rank, int slot, uint32_t game_seq, int n, double prob) {
    if (n < 1 || !(prob > 0.0 && prob <= 1.0)) return -1;
    return start_pool_draw(seed, (uint32_t)rank, (uint32_t)slot, game_seq, n, prob);
}

int xq_engine_start_indices(const xq_engine *eng, const int32_t **dev_index) {
    if (!pool_of(eng) || !dev_index) return XQ_ERR_ARG;
    *dev_index = make_sp(eng).start_index;
    return XQ_OK;
}

int xq_engine_start_pool_stats_read(const xq_engine *eng, xq_start_pool_stats *host_out, void *stream) {
    if (!pool_of(eng) || !host_out) return XQ_ERR_ARG;
    SpHead h;
    XQ_TRY(hipStreamSynchronize((hipStream_t)stream));
    XQ_TRY(hipMemcpy(&h, make_sp(eng).head, 32, hipMemcpyDeviceToHost));
    memset(host_out, 0, sizeof(*host_out));
    host_out->pool_games = h.pool_games;
    return XQ_OK;
}

// the pending records of a game-records engine: the head read back after a synchronise
static int gr_pending(const xq_engine *eng, hipStream_t s, GrHead *h, uint16_t **log) {
    if (!records_of(eng)) return XQ_ERR_ARG;
    *log = make_dev(eng).gr_log;
    XQ_TRY(hipStreamSynchronize(s));
    XQ_TRY(hipMemcpy(h, gr_head(*log, (size_t)eng->cfg.n_games), 32, hipMemcpyDeviceToHost));
    return h->max_out_games >= 1 ? XQ_OK : XQ_ERR_ARG;
}

static int gr_drain(const xq_engine *eng, void *out, int max_records, int *n_records, hipStream_t s, hipMemcpyKind kind) {
    if (!n_records) return XQ_ERR_ARG;
    GrHead h;
    uint16_t *log;
    const int rc = gr_pending(eng, s, &h, &log);
    if (rc != XQ_OK) return rc;
    const unsigned n = h.count < (unsigned)h.max_out_games ? h.count : (unsigned)h.max_out_games;
    *n_records = (int)n;
    if (!out) return XQ_OK;                                  // size query: nothing is consumed
    if ((int)n > max_records) return XQ_ERR_ARG;             // caller's buffer too small: report the size, keep the data
    if (n) XQ_TRY(hipMemcpyAsync(out, gr_ring(log, (size_t)h.max_out_games), (size_t)n * XQ_RECORD_BYTES, kind, s));
    XQ_TRY(hipMemsetAsync(&gr_head(log, (size_t)eng->cfg.n_games)->count, 0, 4, s));
    XQ_TRY(hipStreamSynchronize(s));
    return XQ_OK;
}

int xq_engine_drain_games(const xq_engine *eng, void *host_records, int max_records, int *n_records, void *stream) {
    return gr_drain(eng, host_records, max_records, n_records, (hipStream_t)stream, hipMemcpyDeviceToHost);
}

int xq_engine_drain_games_device(const xq_engine *eng, void *dev_records, int max_records, int *n_records, void *stream) {
    return gr_drain(eng, dev_records, max_records, n_records, (hipStream_t)stream, hipMemcpyDeviceToDevice);
}

int xq_engine_game_records_stats_read(const xq_engine *eng, xq_game_records_stats *host_out, void *stream) {
    if (!host_out) return XQ_ERR_ARG;
    GrHead h;
    uint16_t *log;
    const int rc = gr_pending(eng, (hipStream_t)stream, &h, &log);
    if (rc != XQ_OK) return rc;
    memset(host_out, 0, sizeof(*host_out));
    host_out->recorded = h.recorded; host_out->dropped = h.dropped;
    return XQ_OK;
}

int xq_engine_solver_stats_read(const xq_engine *eng, xq_solver_stats *host_out, void *stream) {
    if (!eng || !host_out || !solver_of(eng) || eng->cfg.n_games <= 0 || !eng->p[P_SQRT]) return XQ_ERR_ARG;
    const size_t G = (size_t)eng->cfg.n_games, S = (size_t)eng->cfg.num_simulations;
    XQ_TRY(hipStreamSynchronize((hipStream_t)stream));
    unsigned long long *h = (unsigned long long *)malloc(sv_bytes(G));
    if (!h) return XQ_ERR_ARG;
    const int rc = xq::check(hipMemcpy(h, ow_base(eng) + sv_off(G, S, arena_of(eng)), sv_bytes(G), hipMemcpyDeviceToHost));
    memset(host_out, 0, sizeof(*host_out));
    if (rc == XQ_OK)
        for (size_t g = 0; g < G; ++g) {
            const unsigned long long *r = h + g * SV_WORDS;
            host_out->proven_nodes += r[SV_NODES]; host_out->proven_stops += r[SV_STOPS]; host_out->proven_moves += r[SV_MOVES];
            host_out->unspent_sims += r[SV_UNSPENT]; host_out->removed_visits += r[SV_REMOVED];
        }
    free(h);
    return rc;
}

int xq_engine_read_root_states(const xq_engine *eng, int slot, int8_t *child_state, int8_t *root_state, void *stream) {
    if (!eng || !solver_of(eng) || slot < 0 || slot >= eng->cfg.n_games || !child_state || !root_state) return XQ_ERR_ARG;
    XQ_TRY(hipStreamSynchronize((hipStream_t)stream));
    const size_t nb = (size_t)slot * eng->node_cap;
    uint16_t m; int32_t first;
    XQ_TRY(hipMemcpy(&m, (uint16_t *)eng->p[P_TM] + nb, 2, hipMemcpyDeviceToHost));
    XQ_TRY(hipMemcpy(&first, (int32_t *)eng->p[P_TC] + nb, 4, hipMemcpyDeviceToHost));
    // node states are seen from the side that moved into the node: a child's is the root mover's own view, the root's the opponent's
    static const int8_t of_child[4] = {0, 1, 2, -1}, of_root[4] = {0, -1, 2, 1};
    *root_state = of_root[node_state(m)];
    const int n = m & XQ_CNT_MASK;
    memset(child_state, 0, XQ_MAXM);
    if (n == 0 || n > XQ_MAXM || first < 0) return 0;
    uint16_t cm[XQ_MAXM];
    XQ_TRY(hipMemcpy(cm, (uint16_t *)eng->p[P_TM] + nb + first, (size_t)n * 2, hipMemcpyDeviceToHost));
    for (int i = 0; i < n; ++i) child_state[i] = of_child[node_state(cm[i])];
    return n;
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
    const int n = m & XQ_CNT_MASK, kind = m >> 14;
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

}  // extern "C"
