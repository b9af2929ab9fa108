/*
 * xq_hip.h -- C ABI of libxq_hip.so: the MI355X (gfx950) self-play hot path of
 * wenjunyang/xiangqi-alphazero as hand-written HIP kernels.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no torch / C++ types.
 *   - every pointer named dev_* / ws is DEVICE memory owned by the caller; nothing is allocated or
 *     freed behind the caller's back.  `stream` is a hipStream_t passed as void*.
 *   - return value: XQ_OK (0) or a negative XQ_ERR_* code; no exceptions cross the ABI; all entry
 *     points are re-entrant (no global mutable state).  Launches are asynchronous on `stream`
 *     unless the function says it synchronises.
 *   - boards are the reference's layout: int8[10][9] row-major (90 bytes), red positive, black
 *     negative, pieces 1..7 = king advisor bishop knight rook cannon pawn (training/game.py:49-65);
 *     player/side is +1 (red) or -1 (black); an action id is (from_sq*90 + to_sq),
 *     sq = row*9+col (training/game.py:112-121).
 *
 * Each entry point cites the reference interface it replaces (paths relative to the reference root).
 */
#ifndef XQ_HIP_H
#define XQ_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define XQ_OK 0
#define XQ_ERR_ARG (-1)      /* bad argument (null pointer, non-positive size, ...) */
#define XQ_ERR_HIP (-2)      /* a HIP runtime call / kernel launch failed; see xq_last_hip_error() */
#define XQ_ERR_WORKSPACE (-3) /* workspace too small */
#define XQ_ERR_OVERFLOW (-4) /* a device-side capacity was exceeded (reported by xq_engine_stats) */

#define XQ_SQUARES 90
#define XQ_ACTION_SPACE 8100
#define XQ_STATE_FLOATS 1350  /* 15 planes x 90, training/game.py:627 */
#define XQ_MAXM 128           /* legal moves kept per position (reference buffer: 200, observed max 69) */
#define XQ_SAMPLE_BYTES 640
#define XQ_RESULT_BYTES 16

const char *xq_version(void);
/* hipGetErrorString of the last failing HIP call on this thread ("" if none). */
const char *xq_last_hip_error(void);

/* =====================================================================================
 * B1 -- rules engine plug point.  Replaces training/cython_engine/game_core.pyx:493-569
 * (cy_generate_legal_moves, cy_is_in_check, cy_find_king, cy_is_attacked, cy_has_legal_moves)
 * and their Python twins training/game.py:176-265, 297-521, 552-563, 618-640, batched over n boards.
 * ===================================================================================== */

/* cy_generate_legal_moves + cy_is_in_check(board, side) + cy_has_legal_moves for n boards.
 * dev_moves[i][0..counts[i]) = action ids in the reference's emission order.
 * dev_in_check may be NULL.  dev_status (may be NULL): per board 0, or 1 if more than XQ_MAXM
 * legal moves / more than 256 pseudo-legal candidates were met (list truncated). */
int xq_movegen_batch(const int8_t *dev_boards, const int8_t *dev_side, int n, uint16_t *dev_moves,
                     uint16_t *dev_counts, uint8_t *dev_in_check, uint8_t *dev_status, void *stream);

/* cy_is_attacked(board, r, c, by) for every square and both attackers:
 * dev_out[i][0][sq] = attacked by red, dev_out[i][1][sq] = attacked by black (uint8 0/1). */
int xq_attack_map_batch(const int8_t *dev_boards, int n, uint8_t *dev_out, void *stream);

/* cy_find_king for both sides: dev_out[i][0] = red king square or -1, dev_out[i][1] = black. */
int xq_find_king_batch(const int8_t *dev_boards, int n, int16_t *dev_out, void *stream);

/* XiangqiGame.get_state_for_nn (training/game.py:618-640): dev_out[i] = float32[15][10][9]. */
int xq_encode_batch(const int8_t *dev_boards, const int8_t *dev_side, int n, float *dev_out, void *stream);

/* XiangqiGame.get_material_score (training/game.py:552-563): dev_out[i][0] red, [i][1] black. */
int xq_material_batch(const int8_t *dev_boards, int n, int32_t *dev_out, void *stream);

/* XiangqiGame.make_move on copies (training/game.py:528-550, board part): child j is
 * dev_boards[parent[j]] with action[j] applied; side flipped.  Used for perft-style expansion. */
int xq_apply_moves_batch(const int8_t *dev_boards, const int8_t *dev_side, const uint32_t *dev_parent,
                         const uint16_t *dev_action, int m, int8_t *dev_out_boards, int8_t *dev_out_side,
                         void *stream);

/* XiangqiGame.is_game_over (training/game.py:565-616) for n independent game states.
 * dev_hist[i] = the last min(12, move_count) pre-move boards (int8[12][90], oldest first, rest ignored).
 * dev_out[i][0] = done (0/1), dev_out[i][1] = winner (+1/-1/0, or 2 when not done). */
int xq_game_over_batch(const int8_t *dev_boards, const int8_t *dev_side, const int32_t *dev_move_count,
                       const int32_t *dev_no_capture, const int8_t *dev_hist, int n, int8_t *dev_out,
                       void *stream);

/* Rules options (opt-in; NULL everywhere is the reference's rules).  perpetual_check = 1: the side that checks through a repetition
 * loses.  The reference calls every repetition a draw (game.py:606-614); under every real Xiangqi rule set the side that repeats
 * the position by checking on every move loses, and a network trained on the draw learns to escape lost positions into a
 * perpetual check no opponent will grant it.  Outside the reference-parity contract, like the other opt-in options.
 * THE RULE.  The trigger is the reference's and does not move: the repetition test is reached exactly as before (after king
 * capture, no legal move, 120 no-capture plies and the ply-200 material rule) and counts the boards of the 12-board window that
 * equal the current one; nothing changes below three matches.  With three or more, and the option on:
 *     s = the side to move now; entry e = 0, 1, ... = the board e + 1 plies ago (entry 0 is the newest pre-move board);
 *     E = the oldest entry of the window that equals the current board: the start of the repetition span;
 *     by ply parity -s is to move in the even entries and s in the odd ones (boards carry no side, none is stored);
 *     chk(-s) = the side to move is in check now and in every odd entry e <= E: every move -s made in the span gave check;
 *     chk(s)  = the side to move is in check in every even entry e <= E;
 *     exactly one of the two holds: that side loses, the winner is the other; both or neither: a draw, as before.
 * "In check" is xq_movegen_batch's in_check (a missing king counts as in check).  In practice only a 4-ply cycle played three times
 * reaches three matches in twelve boards (distances 4, 8, 12, E = 11).  Chase rules (perpetual attack on an unprotected piece) are
 * out of scope.
 * xq_game_over_batch_ex: xq_game_over_batch with the options; dev_kind (or NULL) = uint8[n], what ended the game: 0 not over,
 * 1 king missing, 2 no legal move, 3 no-capture, 4 ply-200, 5 repetition draw, 6 perpetual-check loss.  rules == NULL gives
 * xq_game_over_batch's dev_out byte for byte, and xq_game_over_batch is that call.  XQ_ERR_ARG before any launch: perpetual_check
 * outside {0, 1} or a non-zero reserved word. */
typedef struct xq_rules_opts { int32_t perpetual_check; int32_t reserved[3]; } xq_rules_opts;
int xq_game_over_batch_ex(const int8_t *dev_boards, const int8_t *dev_side, const int32_t *dev_move_count,
                          const int32_t *dev_no_capture, const int8_t *dev_hist, int n, const xq_rules_opts *rules,
                          int8_t *dev_out, uint8_t *dev_kind, void *stream);

/* =====================================================================================
 * B3 -- self-play operator.  Replaces the search + game loop that the reference fans out over
 * processes: training/mcts.py:21-206 (MCTSNode, MCTS.search), training/parallel_selfplay.py:42-134
 * (_play_one_game) and the per-evaluation IPC of training/inference_server.py:37-497.
 *
 * One engine = n_games concurrent game slots resident on one GPU.  A *step* is
 *     xq_engine_select   every slot advances (finishing moves/games, running simulations whose leaves are
 *                        terminal) until it needs ONE network evaluation, and writes that position's
 *                        15x10x9 planes into dev_nn_input[slot]
 *     <evaluator>        B2: any batched policy/value function over dev_nn_input (the ResNet)
 *     xq_engine_expand   consumes dev_policy[slot] / dev_value[slot]: root or leaf expansion with the
 *                        reference's mask-and-normalise, backup along the recorded path
 * By default the simulations of one game stay strictly sequential (as in mcts.py:126-153) and parallelism is across
 * games.  Opt-in leaf batching (xq_engine_init_leaves, K = leaves_per_step > 1) lets a slot hand the evaluator up to K
 * leaves per step, collected under virtual loss -- for few slots, where there is nothing to be parallel across.  K > 1 is
 * knowingly NOT the reference's sequential search (outside the reference-parity contract); K = 1 is today's engine.
 * ===================================================================================== */

typedef struct xq_engine_config {
    int32_t n_games;               /* concurrent slots G */
    int32_t num_simulations;       /* MCTS simulations per move (TrainingConfig.num_simulations) */
    double  c_puct;                /* 1.5 */
    int32_t temperature_threshold; /* plies with T=1.0, then late_temperature (parallel_selfplay.py:92) */
    int32_t max_game_length;
    int32_t random_opening_moves;
    int32_t enable_resign;
    double  resign_threshold;
    int32_t resign_check_steps;    /* <= 16 */
    int32_t add_noise;             /* Dirichlet noise at the root (mcts.py:117-121); self-play: 1 */
    double  dirichlet_alpha;       /* 0.3 */
    double  noise_eps;             /* 0.25 */
    double  late_temperature;      /* 0.3 */
    uint64_t seed;                 /* Philox key (run seed); rank goes into the key as well */
    int32_t rank;
    int32_t inject_len;            /* 0: device RNG; >0: draws come from dev_inject (tests), per slot
                                      4 streams x inject_len raw uint64 (tests/draws.py order) */
    int64_t games_target;          /* stop starting games after this many (<=0: unlimited) */
    int32_t max_out_samples;       /* capacity of the finished-sample ring */
    int32_t max_out_results;       /* capacity of the game-result ring */
    int32_t manual_moves;          /* 0: self-play.  1: search only -- never plays the move (xq_engine_set_position +
                                      num_simulations steps, then xq_engine_read_root); MCTS.search parity / serving.
                                      2: arena games (training/train.py:453-535): no opening, no noise unless add_noise,
                                      move = first maximum of the visit counts (temperature 0), no samples, no resign,
                                      a game still running after max_game_length plies is a draw */
    int32_t start_stagger;         /* 1: slot s idles hash(s) mod (num_simulations+1) steps before its first game, so a
                                      freshly initialised engine reaches the steady-state mix of search depths */
} xq_engine_config;

/* Host-side handle: plain pointers into the caller's workspace.  Treat as opaque. */
typedef struct xq_engine {
    xq_engine_config cfg;
    int32_t node_cap, path_cap, stage_cap, pad0;
    void *p[32];
} xq_engine;

typedef struct xq_engine_stats {
    uint64_t sims;            /* completed simulations (leaf evaluated or terminal) */
    uint64_t terminal_sims;
    uint64_t leaf_evals;      /* network evaluations consumed by simulations */
    uint64_t root_evals;      /* network evaluations consumed by roots (incl. the resign probe) */
    uint64_t moves_played;
    uint64_t games_finished, red_wins, black_wins, draws;
    uint64_t plies_finished;  /* sum of move_count over finished games */
    uint64_t nodes_created;
    uint64_t depth_sum;       /* sum over simulations of descent depth */
    uint64_t children_scanned;/* sum over descents of children read by PUCT select */
    uint64_t resigns;
    uint64_t samples_written, samples_dropped;
    uint64_t overflow;        /* non-zero: a device capacity was exceeded (results invalid) */
    uint64_t games_started;
    uint64_t rows_evaluated;  /* sum over xq_engine_compact calls of n_live: rows the evaluator ran on in packed steps */
    uint64_t reserved[13];    /* [XQ_STAT_COLLISIONS], [XQ_STAT_LEAVES_SUM], [XQ_STAT_LEAF_STEPS]: the leaf-batching counters below;
                                 [XQ_STAT_REUSED_VISITS], [XQ_STAT_REROOTS]: the tree-reuse counters (xq_engine_init_ex);
                                 [XQ_STAT_FAST_MOVES], [XQ_STAT_FAST_SIMS]: the playout-cap counters (xq_engine_init_cap);
                                 [XQ_STAT_FORCED_SIMS], [XQ_STAT_PRUNED_VISITS], [XQ_STAT_PRUNED_CHILDREN]: forced playouts
                                 (xq_engine_init_fp);
                                 [XQ_STAT_GUMBEL_MOVES], [XQ_STAT_GUMBEL_CONSIDERED], [XQ_STAT_GUMBEL_OFFPRIOR]: Gumbel root search
                                 (xq_engine_init_gz) */

} xq_engine_stats;
/* Leaf-batching counters (xq_engine_init_leaves), kept in the reserved words so the struct's layout is unchanged:
 *   reserved[XQ_STAT_COLLISIONS]  descents dropped because they ended on a leaf already pending in their step
 *   reserved[XQ_STAT_LEAVES_SUM]  pending leaves handed to the evaluator, summed over slot-steps
 *   reserved[XQ_STAT_LEAF_STEPS]  slot-steps that handed leaves: mean batch per slot = LEAVES_SUM / LEAF_STEPS
 * All three are 0 with K = 1; the other reserved words stay 0. */
#define XQ_STAT_COLLISIONS 0
#define XQ_STAT_LEAVES_SUM 1
#define XQ_STAT_LEAF_STEPS 2
/* Tree-reuse counters (XQ_ENGINE_TREE_REUSE), 0 without it:
 *   reserved[XQ_STAT_REUSED_VISITS]  visits a search started with from the previous move's tree (sum over re-rooted roots)
 *   reserved[XQ_STAT_REROOTS]        searches that started from the previous move's subtree
 * `sims` keeps counting new simulations only: the samples' visits sum to sims + REUSED_VISITS over finished moves. */
#define XQ_STAT_REUSED_VISITS 3
#define XQ_STAT_REROOTS 4

/* Bytes of device workspace the engine needs for cfg (tree arenas dominate:
 * n_games * (1 + (num_simulations+1)*XQ_MAXM) nodes * 24 B -- sized for 288 GB HBM, no per-node malloc). */
size_t xq_engine_workspace_bytes(const xq_engine_config *cfg);

/* Carves `ws` (>= workspace_bytes, 256-byte aligned) and initialises the engine: boards, history rings, per-slot state
 * words (allocation marks and RNG counters among them), request counts, root prior / injected-noise tables, ring
 * counters and the statistics are zeroed, and every slot starts a new game at its first step.  The tree arenas (N, W, P, action, first-child, meta) are NOT cleared: a slot's nodes are valid only below its
 * allocation mark (bump allocator, reset at every move), nothing in the engine reads past it, and whatever the caller's
 * buffer held before stays there -- tools that walk the arenas (`SelfPlayEngine.arena_views`) must stop at the mark.
 * dev_inject: uint64[n_games][4][inject_len] or NULL. */
int xq_engine_init(xq_engine *eng, const xq_engine_config *cfg, void *ws, size_t ws_bytes,
                   const uint64_t *dev_inject, void *stream);

/* Leaf batching (opt-in): K = leaves_per_step leaves per slot and step, 1 <= K <= 64 (K = 1: exactly xq_engine_init).
 * In one step a searching slot runs descents j = 0, 1, ... from the root until K leaves are pending, or sims_done + pending
 * == num_simulations, or a collision occurs.  Virtual loss is a separate per-node counter vl (never folded into N or W):
 * child i of parent p is scored with n = N_i + vl_i (in q = w / n and in 1 + n), w = W_i - vl_i (float64) and
 * sqrt(N_p + vl_p); otherwise the arithmetic above, for all three prior kinds, first maximum wins; with every vl = 0 the
 * score is bit-identical to K = 1's.  A descent that chooses a non-terminal leaf adds 1 to vl along its path (the root
 * included); a terminal leaf is backed up at once and counts as a simulation (at most 48 per launch, as with K = 1); a
 * descent that ends on a leaf an earlier descent of the same step waits on is a COLLISION: not a simulation, and it ends
 * the slot's collection for this step.  xq_engine_expand* expands and backs up the pending leaves in descent order (child
 * blocks bump-allocated in that order), each backup removing its descent's virtual loss: every vl is 0 after every step.
 * Roots, noise, the resign probe, move choice and samples are unchanged; every move still ends with exactly num_simulations
 * simulations.
 * Request ROWS are slot-major: row slot*K + j carries pending leaf j (the root request is row slot*K): dev_nn_input is
 * [G*K][15][90], dev_policy / dev_legal_logits / dev_value have G*K rows, xq_engine_requests' moves / counts are
 * [G*K][XQ_MAXM] / [G*K] (count 0: the row asks for nothing), and the packed buffers hold G*K rows whose rows[r] is the
 * packed row's REQUEST ROW (slot = rows[r] / K); the *_live evaluator entry points then take capacity G*K.  Every count
 * stays on the device and every grid is sized by G*K: the step records into one graph as with K = 1.  K is kept in the
 * handle (pad0); select, expand, expand_legal, requests, compact, packed and expand_packed read it.
 * XQ_ERR_ARG (before any launch): K < 1 or K > 64, K > 1 with manual_moves == 2 (arena), and the evaluation cache
 * (xq_evcache_probe / _commit, xq_engine_compact_misses) on an engine with K > 1.  The workspace adds G * node_cap int32
 * virtual-loss counters and the G*K request rows; xq_engine_workspace_bytes_leaves returns 0 for invalid arguments. */
size_t xq_engine_workspace_bytes_leaves(const xq_engine_config *cfg, int leaves_per_step);
int xq_engine_init_leaves(xq_engine *eng, const xq_engine_config *cfg, int leaves_per_step, void *ws, size_t ws_bytes,
                          const uint64_t *dev_inject, void *stream);

/* Tree reuse across moves (opt-in flag XQ_ENGINE_TREE_REUSE of xq_engine_init_ex; flags = 0 is xq_engine_init_leaves).
 * When a self-play move ends, the chosen child c becomes the next search's root with its whole subtree: every kept node keeps
 * its N, W, P, action, child count and kind, its children stay in order; the old root and the sibling subtrees are discarded.
 * Within the step of the move's end, xq_engine_select also launches k_reroot, which compacts c's subtree in place to the front
 * of the slot's arena (c at node 0, the allocation mark at 1 + the kept nodes).  The new position still issues its root
 * request: resign probe, terminal / adjudication status and the evaluation cache are unchanged.  The reused root's children
 * get their float32 priors from this evaluation (bit-identical to the stored ones under unchanged weights) and fresh Dirichlet
 * noise (the same draws a fresh root takes), and the search starts at sims_done = root N = the sum of its children's visits:
 * it stops at num_simulations as always, so a sample still holds exactly num_simulations visits, some of them gathered before
 * that root's noise was drawn, and a move costs num_simulations minus the reused visits in new simulations.
 * A slot starts a fresh tree on a new game, when the chosen child was never expanded, and when xq_engine_drop_reroots ran
 * since the move began (call it after every weight update: graph-safe, one device-side word per slot, no host sync).  A
 * reused root whose child count differs from the position's legal-move count (a defect) sets overflow bit 64 << 8.
 * XQ_ERR_ARG before any launch: unknown flags, and tree reuse with manual_moves 1 or 2, leaves_per_step > 1 or
 * num_simulations > XQ_REUSE_MAX_SIMS (k_reroot keeps a bitmap of the arena in at most 64 KiB of LDS).  The flag lives in the
 * handle (pad0's upper 16 bits); it adds no workspace: xq_engine_workspace_bytes_ex is xq_engine_workspace_bytes_leaves for
 * valid flags and 0 otherwise.  Combining it with the evaluation cache is supported. */
#define XQ_ENGINE_TREE_REUSE 1u
#define XQ_REUSE_MAX_SIMS 1600
size_t xq_engine_workspace_bytes_ex(const xq_engine_config *cfg, int leaves_per_step, unsigned flags);
int xq_engine_init_ex(xq_engine *eng, const xq_engine_config *cfg, int leaves_per_step, unsigned flags, void *ws,
                      size_t ws_bytes, const uint64_t *dev_inject, void *stream);
/* No slot of a tree-reuse engine re-roots at the end of the move it is searching now (XQ_ERR_ARG without the flag). */
int xq_engine_drop_reroots(const xq_engine *eng, void *stream);

/* Playout cap randomization (opt-in; cap == NULL is xq_engine_init_ex exactly, and xq_engine_init_ex is that call).  Outside the
 * reference-parity contract, like leaf batching and tree reuse: the reference searches every move at one size.
 *   fast_simulations = S_fast, 1 <= S_fast < num_simulations;  full_search_prob = p, 0 < p <= 1 (NaN refused);  reserved = 0.
 * The draw: for every position of a self-play game that will be searched (its root request is issued with status 0: neither
 * game over nor adjudicated at max_game_length) xq_engine_select takes ONE uniform draw u from the slot's existing uniform
 * stream (the stream of the move-choice draw; injected runs: stream 3 of dev_inject, whose layout is unchanged) when it issues
 * that root request; the move is FULL iff u < p.  Per searched position that stream so yields the cap draw first and the
 * move-choice draw at the move's end (size inject_len for two draws per position); a position whose root evaluation ends the
 * game by resignation has taken its cap draw and no move-choice draw.
 *   FULL move: exactly the move of an engine without the cap: Dirichlet noise at the root, budget num_simulations, a sample is
 *              staged, n_samples grows.
 *   FAST move: no root noise and no Dirichlet draws taken (the root is a root with add_noise = 0), budget S_fast, NO sample
 *              staged, n_samples unchanged.  The move choice is unchanged (temperature 1 before temperature_threshold,
 *              late_temperature after, one uniform draw).
 * Everything keyed on the sample count keeps that key: the resign rule starts after 10 RECORDED samples (with p = 0.25 about four
 * times later in plies: intended, not tuned), xq_game_result.n_samples is the recorded count, z is written to recorded samples
 * only; a game may record no sample at all.  Random opening moves, terminal handling, the resign probe, adjudication: unchanged.
 * With XQ_ENGINE_TREE_REUSE the hand-off happens at the end of full and fast moves alike and the budget stays visits: a search
 * starts at sims_done = reused visits and ends when sims_done >= THIS move's budget, so a fast search that inherits >= S_fast
 * visits runs no new simulation and its root may hold more than S_fast visits (it is not sampled); a full search still ends with
 * exactly num_simulations visits.  A reused root of a fast move gets its float32 priors from the new evaluation, keeps the prior
 * kind it had as an inner node and uses no float64 root priors.  The evaluation cache combines with the cap unchanged.
 * XQ_ERR_ARG before any launch (xq_engine_workspace_bytes_cap: 0): manual_moves 1 or 2, leaves_per_step > 1, parameters out of
 * range, reserved != 0, and whatever xq_engine_init_ex refuses.  No workspace is added; the parameters live in free per-slot
 * state words, "cap on" in the handle (pad0, above the public flag bits).  Counters, 0 without the cap:
 *   reserved[XQ_STAT_FAST_MOVES]  moves played after a fast search
 *   reserved[XQ_STAT_FAST_SIMS]   new simulations run by fast searches (`sims` keeps counting all new simulations) */
typedef struct xq_playout_cap { int32_t fast_simulations; int32_t reserved; double full_search_prob; } xq_playout_cap;
#define XQ_STAT_FAST_MOVES 5
#define XQ_STAT_FAST_SIMS 6
size_t xq_engine_workspace_bytes_cap(const xq_engine_config *cfg, int leaves_per_step, unsigned flags, const xq_playout_cap *cap);
int xq_engine_init_cap(xq_engine *eng, const xq_engine_config *cfg, int leaves_per_step, unsigned flags,
                       const xq_playout_cap *cap, void *ws, size_t ws_bytes, const uint64_t *dev_inject, void *stream);

/* Forced playouts and policy target pruning (opt-in; forced == NULL is xq_engine_init_cap exactly, and xq_engine_init_cap is
 * that call).  The two rules the KataGo scheme pairs with the playout cap; outside the reference-parity contract like the cap.
 * Parameter k, 0 < k <= 16 (KataGo: 2; NaN refused), reserved = 0.  k is rounded to float32 ONCE at init and kept as that float32
 * in a per-slot state word; every use widens the float32 to double.
 * WHERE: only at a root of prior kind 1, i.e. the noisy root of a full self-play move, which is always node 0 (a reused root of a
 * full move becomes kind 1).  Not on fast moves of the cap (their roots carry no noise), not at inner nodes.
 * FORCING, in the descent at node 0.  Nr = the root's visit count as used for sqrt_tab[Nr].  Child i is FORCED iff
 *     N_i > 0  and  (double)N_i * (double)N_i < f_i,   f_i = (k * rootP[i]) * (double)Nr   (two float64 products, that order),
 * with rootP the float64 noisy root priors.  A forced child scores +infinity; the first-maximum rule then picks the forced child
 * of lowest index.  Everything else in the descent is unchanged.  A simulation whose root choice was a forced child counts in
 * reserved[XQ_STAT_FORCED_SIMS].
 * PRUNING, at the end of a full move, before the sample is staged and before the move-choice weights are formed.  Nr = the root's
 * visits (the move's budget S), c* = the first maximum of the children's N,
 *     PUCT(i, n) = q_i + ((c_puct * rootP[i]) * sqrt_tab[Nr]) / (double)(1 + n),   q_i = W_i / N_i held constant
 * (the kind-1 float64 arithmetic of the descent), P* = PUCT(c*, N_c*).  For every other child with N_i > 0: n = N_i, d = 0;
 * while n > 1 and (d+1)*(d+1) < f_i and PUCT(i, n-1) < P*: n -= 1, d += 1.  If d > 0 and n == 1 then n = 0 (a child reduced to a
 * single playout is removed).  v_i = n; v_c* = N_c*.  The loop runs at most ceil(sqrt(k * S)) times per child.
 * The sample's visits[] AND the move-choice weights (temperature 1 and late_temperature alike, the same single uniform draw) use
 * v; n_moves and the action list are unchanged.  The tree keeps its real N and W: tree reuse, `sims`, REUSED_VISITS, the budget
 * and xq_engine_read_root are unaffected.  Counters, 0 without the option:
 *   reserved[XQ_STAT_FORCED_SIMS]      simulations that took a forced child at the root
 *   reserved[XQ_STAT_PRUNED_VISITS]    sum over full moves and children of N_i - v_i
 *   reserved[XQ_STAT_PRUNED_CHILDREN]  children with N_i > 0 and v_i == 0
 * Consequences: a sample's visits sum to AT MOST num_simulations, no longer exactly; with k * num_simulations < 1 no child is
 * ever forced (N_i^2 >= 1 > f_i) and no visit is subtracted ((d+1)^2 >= 1 > f_i), so every record equals an engine's without the
 * option byte for byte.
 * It combines with XQ_ENGINE_TREE_REUSE, with the playout cap (full moves only) and with the evaluation cache (unchanged).
 * XQ_ERR_ARG before any launch (xq_engine_workspace_bytes_fp: 0): manual_moves 1 or 2, add_noise == 0, leaves_per_step > 1, k not
 * finite, k <= 0 or k > 16, a non-zero reserved word, and whatever xq_engine_init_cap refuses.  No workspace is added: k lives in
 * the last free per-slot state word, "forced on" in the handle (pad0, above the public flag bits). */
typedef struct xq_forced_playouts { double k; uint32_t reserved[2]; } xq_forced_playouts;
#define XQ_STAT_FORCED_SIMS 7
#define XQ_STAT_PRUNED_VISITS 8
#define XQ_STAT_PRUNED_CHILDREN 9
size_t xq_engine_workspace_bytes_fp(const xq_engine_config *cfg, int leaves_per_step, unsigned flags, const xq_playout_cap *cap,
                                    const xq_forced_playouts *forced);
int xq_engine_init_fp(xq_engine *eng, const xq_engine_config *cfg, int leaves_per_step, unsigned flags, const xq_playout_cap *cap,
                      const xq_forced_playouts *forced, void *ws, size_t ws_bytes, const uint64_t *dev_inject, void *stream);

/* Gumbel root search with sequential halving (opt-in; gumbel == NULL is xq_engine_init_fp exactly, and xq_engine_init_fp is that
 * call).  The root rule of Gumbel AlphaZero (Danihelka et al., "Policy improvement by planning with Gumbel", ICLR 2022; the usual
 * formulation is DeepMind's mctx): at the root, m moves are sampled without replacement by the Gumbel-top-k trick and the budget is
 * spent on them by sequential halving; the training target is the completed-Q improved policy, not the visit counts.  Interior
 * nodes keep PUCT.  Outside the reference-parity contract, like the other opt-in options.
 * Parameters: considered = m, 1 <= m <= 128; c_visit >= 0 (mctx: 50); c_scale > 0 (mctx: 1.0 for two-player games here, values
 * bounded by +-1); reserved = 0.  c_visit and c_scale are rounded to float32 ONCE at init and widened to double at every use.
 * ROOT EXPANSION (every root of a Gumbel engine, self-play and manual_moves = 1).  The root has its float32 priors tP[i] over the cnt
 * ordered legal moves exactly as without the option (uniform 1 / cnt when the network gave the legal moves no mass).
 *     l_i = log((double)max(tP[i], FLT_MIN))
 *     g_i = one Gumbel(0, 1) draw per legal move from the slot's Dirichlet stream (stream 2), whose counter advances by cnt:
 *           device RNG  g = -log(-log(u)), u = ((x >> 11) + 0.5) * 2^-53 for the raw 64-bit draw x;
 *           inject_len > 0  g = ((double)((x >> 40) % 4096) - 1024.0) / 512.0 (exact, no transcendental);
 *           manual_moves = 1 with a non-null host_noise in xq_engine_set_position: the handed values ARE the g_i, no draw is taken.
 *     rootP[i] = g_i + l_i  (float64), the root's prior kind is 3 (xq_engine_read_root: prior = rootP, *prior_kind = 3).
 * The root never takes Dirichlet noise, whatever add_noise says.  The root's network value v_hat (the float32 widened) is kept for
 * the end of the move.  The resign probe, terminal status and adjudication are unchanged.
 * CONSIDERED VISITS.  considered_visits(k, S) is mctx's get_sequence_of_considered_visits, a sequence of length S:
 *     k <= 1: t -> t.   Otherwise: L = ceil(log2(k)); c = k; base = 0; until S entries exist:
 *       e = max(1, S / (L * c)) (integer division); append base, c times; base + 1, c times; ... base + e - 1, c times;
 *       base += e; c = max(2, c / 2).
 * xq_gumbel_considered_visits_host writes it for 1 <= k <= 128, 1 <= S <= 65535 (tests pin the table with it).
 * ROOT SELECTION, in the descent at a node of kind 3 (always node 0); every other level is unchanged.  k = min(m, cnt); t = the
 * root's visit count before this simulation; cv = considered_visits(k, S)[t].  The CANDIDATES are the children with N_i == cv.
 *     cv == 0: the winner is the first maximum over the candidates of rootP[i];
 *     cv  > 0: the first maximum over the candidates of rootP[i] + sigma(q_i),
 *     sigma(q) = ((c_visit + maxN) * c_scale) * ((q + 1) * 0.5),  q_i = W_i / N_i,  maxN = the maximum of the children's N,
 * all in float64, products and sums in the order written, no fused multiply-add.  No considered set is stored: the equal-visit
 * rule is the sequential halving (the first k simulations take the k largest g + l in order, every later phase revisits the best
 * of the children that reached the phase's count).  The fixed map (q + 1) / 2 replaces mctx's min-max rescaling of q: values here
 * are bounded by +-1.  No candidate (never observed) sets overflow bit 8 << 8 like an all-NaN level.
 * END OF A MOVE (self-play, root of kind 3).  maxN = max N_i, sumN = sum N_i, both over the children in move order.
 *     played child = the first maximum, over the children with N_i == maxN, of rootP[i] + sigma(q_i).
 * No temperature is applied and NO draw of the uniform stream (stream 3) is consumed.  The sample's visits[] hold the improved
 * policy quantised to 16 bits:
 *     v_mix = (v_hat + sumN * (sum_{N_b>0} tP[b] q_b / sum_{N_b>0} tP[b])) / (1 + sumN), the two sums float64, sequential in move
 *             order over the float32 priors widened (a zero denominator takes v_hat for the quotient);
 *     completed q_i = q_i if N_i > 0, else v_mix;
 *     pi'_i = softmax_i(l_i + sigma(completed q_i)) in float64: x_i - max x, exp, the denominator summed sequentially in move order;
 *     visits[i] = (uint16_t)floor(pi'_i * 65535 + 0.5).
 * late_temp = 0 and reserved0 = 1 ("visits are a quantised improved policy"; 0 in every other sample).  The record size and every
 * consumer stay as they are: they normalise visits by their sum, which lies within cnt / 2 of 65535.  The tree keeps its real N
 * and W.  A search-only engine (manual_moves = 1) holds after S simulations as always.
 * Counters, 0 without the option:
 *   reserved[XQ_STAT_GUMBEL_MOVES]       moves chosen by a Gumbel search
 *   reserved[XQ_STAT_GUMBEL_CONSIDERED]  the sum of k = min(m, cnt) over those moves
 *   reserved[XQ_STAT_GUMBEL_OFFPRIOR]    those moves whose played child is not the first maximum of tP
 * XQ_ERR_ARG before any launch (xq_engine_workspace_bytes_gz: 0): gumbel with manual_moves = 2 (arena), XQ_ENGINE_TREE_REUSE, a
 * playout cap, forced playouts or leaves_per_step > 1; m outside [1, 128]; c_visit or c_scale not finite (as float32), c_visit < 0,
 * c_scale <= 0; reserved != 0; and whatever xq_engine_init_fp refuses.  The evaluation cache and manual_moves = 1 are allowed.
 * Workspace: the parameters, one double per slot and the tables for k = 1 .. m (2 m S bytes) lie behind the engine's square-root
 * table (THE OPTION WORDS below); only Gumbel engines grow, "gumbel on" lives in the handle (pad0, above the public flag bits). */
typedef struct xq_gumbel { int32_t considered; int32_t reserved; double c_visit; double c_scale; } xq_gumbel;
#define XQ_STAT_GUMBEL_MOVES 10
#define XQ_STAT_GUMBEL_CONSIDERED 11
#define XQ_STAT_GUMBEL_OFFPRIOR 12
size_t xq_engine_workspace_bytes_gz(const xq_engine_config *cfg, int leaves_per_step, unsigned flags, const xq_playout_cap *cap,
                                    const xq_forced_playouts *forced, const xq_gumbel *gumbel);
int xq_engine_init_gz(xq_engine *eng, const xq_engine_config *cfg, int leaves_per_step, unsigned flags, const xq_playout_cap *cap,
                      const xq_forced_playouts *forced, const xq_gumbel *gumbel, void *ws, size_t ws_bytes,
                      const uint64_t *dev_inject, void *stream);
int xq_gumbel_considered_visits_host(int k, int num_simulations, uint16_t *host_out);

/* Arena options (opt-in; arena == NULL is xq_engine_init_gz exactly, and xq_engine_init_gz is that call): paired random openings
 * and a per-model packed step for the arena games (manual_moves = 2), so a gate can play hundreds of DISTINCT games whose
 * evaluator cost follows each model's own live requests.  Without the options an arena plays two distinct games however many it
 * is asked for (no opening, no noise, first maximum of the visits); that stays the default.  Outside the reference-parity
 * contract, like the other opt-in options; with opening_plies = 0 the games are the reference's.
 * Parameters: opening_plies = R, 0 <= R <= XQ_ARENA_MAX_OPENING; first_game >= 0, the arena game index of slot 0 (a shard of a
 * larger arena starts on any index); reserved = 0.
 * PAIRED OPENINGS, when a slot starts its game and R > 0.  Slot s plays arena game g = first_game + s (slot == game); its pair is
 * p = g / 2 (integer division).  The new model is red in even games, as in every arena.
 *     The game starts with exactly R uniformly random legal plies: ply i (0-based) plays move x_i % cnt of the cnt ORDERED legal
 *     moves of the position, the mechanics of the self-play opening.
 *     The raw 64-bit draw x_i is a function of the PAIR, never of the slot, the rank or the shard:
 *           device RNG      x_i = philox_u64(cfg.seed, 0, p, 8, i, 0): rank word 0, the slot word holds p, kind 8 (no other draw
 *                           uses it; 7 is the start stagger's), counter i, sub 0;
 *           inject_len > 0  x_i = entry i of the slot's own stream 1 (choice); a test gives both slots of a pair the same stream.
 *                           i >= inject_len sets overflow bit 2 and takes x_i = 0.  The stream's counter is not advanced.
 *     If an opening ply ends the game (xq_game_over_batch's rule on the position after it), the game restarts from the initial
 *     position with NO opening, as self-play does; its recorded count is 0.
 *     So games 2p and 2p + 1 start from the same position with colours swapped, and a shard that starts on any game index plays
 *     the same games as the unsharded arena.
 * The opening plies count in move_count (the result's steps); they are not counted in moves_played.  Everything after the
 * opening is the arena move rule: S simulations without noise, the first maximum of the visit counts, a draw when the game is
 * not over at max_game_length plies.
 * xq_engine_arena_openings: *dev_actions = uint16[G][XQ_ARENA_MAX_OPENING], row s = the actions slot s played as its opening,
 * zero past *dev_counts[s]; *dev_counts = int32[G], R for a played opening, 0 before the slot's game started, after the restart
 * rule and with R = 0.  Workspace pointers valid for the engine's lifetime.
 * PER-MODEL PACKED STEP.  Slot s belongs to the NEW model iff ((first_game + s) even) == (red is to move in the slot's REAL game):
 * the model that is searching evaluates every node of its search, root and leaves at any depth.  On one stream:
 *     xq_engine_select(eng, nn_input)                       as before
 *     xq_engine_compact_arena(eng, nn_input)                stable, slot-ordered compaction of the waiting slots (phase WAIT_ROOT /
 *                                                           WAIT_LEAF: exactly k_expand's test) into TWO buffer sets, set 0 the new
 *                                                           model's slots and set 1 the old model's; each set has its own n_live,
 *                                                           rows, x, moves, counts as xq_engine_compact fills them.  Every waiting
 *                                                           slot is in exactly one set; rows_evaluated grows by n_live0 + n_live1
 *     <new model over set 0, old model over set 1>          the *_live entry points, capacity = n_games, dev_n = the set's n_live;
 *                                                           the two evaluations are independent and may run concurrently
 *     xq_engine_expand_packed_arena(eng, logits_new, value_new, logits_old, value_old)
 *                                                           scatters packed row r of set 0 from the new model's outputs and of
 *                                                           set 1 from the old model's back to slot rows[r] of slot_logits /
 *                                                           slot_value (shared by both sets) and runs xq_engine_expand_legal
 * xq_engine_packed_arena writes the two sets' addresses to out[0] (new) and out[1] (old); slot_logits / slot_value are the
 * engine's one pair.  No count leaves the device and every grid is sized by n_games, so the step records into one replayable
 * graph; n_live = 0 in either set, or both, is a valid step.  The games are those of the full-width step with the other model's
 * requests masked: a row's arithmetic in every evaluator kernel does not depend on its position in the batch.
 * XQ_ERR_ARG before any launch (xq_engine_workspace_bytes_ar: 0): arena options with manual_moves != 2; opening_plies outside
 * [0, 16]; first_game < 0 (or first_game + n_games beyond int32); reserved != 0; and whatever xq_engine_init_gz refuses -- so
 * with arena options leaves_per_step = 1 and none of tree reuse, playout cap, forced playouts and Gumbel root search.  The three
 * xq_engine_*_arena calls and xq_engine_arena_openings return XQ_ERR_ARG on an engine without arena options.
 * Workspace: the parameters, the openings record and the two buffer sets (about 5.7 KB per slot and set) lie behind the engine's
 * square-root table (THE OPTION WORDS below); only arena-option engines grow, "arena options on" lives in the handle (pad0, above the public flag bits). */
#define XQ_ARENA_MAX_OPENING 16
typedef struct xq_arena_opts { int32_t opening_plies; int32_t first_game; uint32_t reserved[2]; } xq_arena_opts;
size_t xq_engine_workspace_bytes_ar(const xq_engine_config *cfg, int leaves_per_step, unsigned flags, const xq_playout_cap *cap,
                                    const xq_forced_playouts *forced, const xq_gumbel *gumbel, const xq_arena_opts *arena);
int xq_engine_init_ar(xq_engine *eng, const xq_engine_config *cfg, int leaves_per_step, unsigned flags, const xq_playout_cap *cap,
                      const xq_forced_playouts *forced, const xq_gumbel *gumbel, const xq_arena_opts *arena, void *ws,
                      size_t ws_bytes, const uint64_t *dev_inject, void *stream);
int xq_engine_arena_openings(const xq_engine *eng, const uint16_t **dev_actions /* [G][16] */, const int32_t **dev_counts /* [G] */);

/* Rules options of an engine (opt-in; rules == NULL or perpetual_check = 0 is xq_engine_init_ar exactly, and xq_engine_init_ar is
 * that call): the perpetual-check rule of xq_rules_opts above at every terminal test of the engine -- the root's status, the real
 * game (openings included) and the leaves of the descent in k_select and k_select_multi.  It changes a terminal verdict and nothing
 * else, so it goes with every mode (self-play, search only, arena) and every other option, and refuses only perpetual_check
 * outside {0, 1} and a non-zero reserved word (XQ_ERR_ARG before any launch; xq_engine_workspace_bytes_ru: 0).
 * A game the rule decides carries reason 4 in its xq_game_result and its root's status word is 4; reason 1 stays for every other
 * rules ending, a repetition that stays a draw under the option included.  A leaf the rule decides backs up 1 for the side that
 * moved into it when that side wins (the usual case: the checked side completes the repetition), like a mate, and -1 when that
 * side loses (its own check completed its perpetual); every other decided leaf keeps the reference's 1 (mcts.py:137-140).
 * No workspace, no state word, no counter: "rule on" lives in the handle (pad0, above the public flag bits) and reaches the
 * kernels as a kernel argument. */
size_t xq_engine_workspace_bytes_ru(const xq_engine_config *cfg, int leaves_per_step, unsigned flags, const xq_playout_cap *cap,
                                    const xq_forced_playouts *forced, const xq_gumbel *gumbel, const xq_arena_opts *arena,
                                    const xq_rules_opts *rules);
int xq_engine_init_ru(xq_engine *eng, const xq_engine_config *cfg, int leaves_per_step, unsigned flags, const xq_playout_cap *cap,
                      const xq_forced_playouts *forced, const xq_gumbel *gumbel, const xq_arena_opts *arena,
                      const xq_rules_opts *rules, void *ws, size_t ws_bytes, const uint64_t *dev_inject, void *stream);

/* Proven-result search (MCTS-solver; opt-in; solver == NULL or enabled = 0 is xq_engine_init_ru exactly, and xq_engine_init_ru is
 * that call).  Exact result propagation as chess-like engines ship it (Winands et al., "Monte-Carlo Tree Search Solver", 2008;
 * lc0's "sticky endgames"): the search learns that a position is decided, stops re-testing it, never prefers a move it has shown
 * to lose and plays a move it has shown to win at once.  Outside the reference-parity contract, like the other opt-in options;
 * off, every byte is as before.
 * THE RULE.  Every tree node carries a state in {UNKNOWN, WIN, DRAW, LOSS}, seen from the side that MOVED INTO the node -- the view
 * of its W.  New nodes are UNKNOWN.  A tree node has one path from the root, so the history-dependent verdicts (repetition,
 * no-capture count, ply 200) are properties of the node.
 * 1. TERMINAL LEAF.  When a descent ends on a node that the terminal test (xq_game_over_batch's rule, with the engine's rules
 *    options) decides, the node's state is set from the TRUE result: DRAW if winner == 0, WIN if the winner is the side that moved
 *    into the leaf, LOSS otherwise (ply 200's material rule and the perpetual-check rule can name the side to move the winner).
 *    The value backed up is the state's exact value, +1 / 0 / -1.  This is NOT the reference's "every decided leaf is the mover's
 *    win" (mcts.py:137-140), which an engine without the option keeps.
 * 2. PROPAGATION, in xq_engine_select right after that backup, up the recorded path while a state changes.  For the parent p, if
 *    UNKNOWN, of the node c whose state just changed: c WIN makes p LOSS; otherwise, if no child of p is UNKNOWN, p becomes DRAW
 *    when some child is DRAW and WIN when every child is LOSS; otherwise propagation stops.  It also stops at a parent that is
 *    already decided.  All of p's children exist from its expansion on.  The root takes part.
 * 3. DESCENT.  A descent stops at the first NON-ROOT node whose state is not UNKNOWN: no terminal test, no evaluator request, the
 *    node's exact value is backed up; it counts as a simulation and as a terminal simulation (also towards the bound of 48 per
 *    launch).  At every level a child of state LOSS scores -infinity, unless the parent's own state is WIN (then every child is
 *    LOSS; reachable only at the root; plain PUCT).  Everything else in the score, the first-maximum rule included, is unchanged.
 * 4. EARLY END OF A MOVE.  Whenever a search looks at its root -- before every simulation, the first one after the root's expansion
 *    or a re-root included, and AHEAD of the test of the budget, so a reused root that inherits its whole budget in visits, or a
 *    win proven by the budget's last simulation, is covered too -- if some root child is WIN (equivalently: the root is LOSS), the
 *    move ends at once.  c = the first such child in move order is played: no temperature and no draw of the uniform stream (a
 *    playout cap's cap draw has already happened).  unspent = max(0, budget - sims_done); the unspent simulations are not run and
 *    not counted in `sims`.  Search only (manual_moves = 1): the slot holds, with sims_done < num_simulations when unspent > 0.
 * 5. THE COUNTS A MOVE ENDS WITH (self-play full and fast moves, arena moves).  v_i = 0 for a LOSS child when some child is not
 *    LOSS, otherwise v_i = N_i; on an early end v_c += unspent; if every v_i is 0, v = N (nothing is taken away).  The sample's
 *    visits[] and the move-choice weights use v: self-play takes its one uniform draw as always unless rule 4 applied; the arena
 *    takes the first maximum of v.  A sample whose move rule 4 chose carries reserved1 = 1 (0 in every other sample).  A sample's
 *    visits sum to AT MOST the budget.  The tree keeps its real N and W.
 * 6. TREE REUSE.  Kept nodes keep their state through the re-root, the new root included (its other meta bits are rewritten).  A
 *    reused root may already be decided; rules 3-5 cover it: a WIN root (the side to move has lost) is searched by plain PUCT over
 *    its LOSS children, every simulation a stop.
 * 7. UNCHANGED: the root request and its status, resignation, max_game_length adjudication, the z of samples, the evaluation cache
 *    (decided nodes never ask), the perpetual-check rule (it only changes what rule 1 sees).
 * The state lives in bits 12-13 of the node meta word (child count: bits 0-11, prior kind: bits 14-15); they are 0 on every engine
 * without the option.  Counters (xq_engine_solver_stats_read; the engine's own statistics words are all taken), all 0 on a game
 * where nothing is ever decided:
 *   proven_nodes    states set, by rules 1 and 2          proven_stops    simulations that ended by rule 3
 *   proven_moves    moves (search only: searches) ended by rule 4          unspent_sims    the sum of their unspent
 *   removed_visits  the sum of N_i - v_i over rule 5's zeroed children
 * Allowed: self-play with tree reuse, the playout cap and the evaluation cache in every combination; search only; arena games with
 * and without arena options; the perpetual-check rule.  XQ_ERR_ARG before any launch (xq_engine_workspace_bytes_sv: 0): enabled
 * outside {0, 1}, a non-zero reserved word; with enabled = 1: leaves_per_step > 1, Gumbel root search (its equal-visit candidates
 * cannot skip a child), forced playouts; and whatever xq_engine_init_ru refuses.  A LOSS root without a WIN child (a defect) sets
 * overflow bit 128 << 8.  Workspace: 64 bytes of counters per slot behind the engine's square-root table (THE OPTION WORDS
 * below); only solver engines grow, "solver on" lives in the handle (pad0, above the public flag bits).
 * xq_engine_read_root_states: the states at the root of `slot` from the view of the SIDE TO MOVE there: child_state[i] (move order,
 * XQ_MAXM entries, zero past the count) +1 this move wins, -1 it loses, 2 draw, 0 unknown; *root_state in the same code.  Returns
 * the child count; XQ_ERR_ARG on an engine without the option.  Synchronises, as xq_engine_solver_stats_read does. */
typedef struct xq_solver_opts { int32_t enabled; int32_t reserved[3]; } xq_solver_opts;
typedef struct xq_solver_stats {
    uint64_t proven_nodes, proven_stops, proven_moves, unspent_sims, removed_visits;
    uint64_t reserved[3];
} xq_solver_stats;
size_t xq_engine_workspace_bytes_sv(const xq_engine_config *cfg, int leaves_per_step, unsigned flags, const xq_playout_cap *cap,
                                    const xq_forced_playouts *forced, const xq_gumbel *gumbel, const xq_arena_opts *arena,
                                    const xq_rules_opts *rules, const xq_solver_opts *solver);
int xq_engine_init_sv(xq_engine *eng, const xq_engine_config *cfg, int leaves_per_step, unsigned flags, const xq_playout_cap *cap,
                      const xq_forced_playouts *forced, const xq_gumbel *gumbel, const xq_arena_opts *arena,
                      const xq_rules_opts *rules, const xq_solver_opts *solver, void *ws, size_t ws_bytes, const uint64_t *dev_inject,
                      void *stream);
int xq_engine_read_root_states(const xq_engine *eng, int slot, int8_t *child_state /* [XQ_MAXM] */, int8_t *root_state, void *stream);
int xq_engine_solver_stats_read(const xq_engine *eng, xq_solver_stats *host_out, void *stream);

/* Root statistics per sample (opt-in; root_stats == NULL or enabled = 0 is xq_engine_init_sv exactly -- same workspace bytes, same
 * handle, same bytes out -- and xq_engine_init_sv is that call).  The search's own value of the root is kept with every sample a
 * self-play move stages, so a trainer can regress the value head on a mix of the game's result z and the search value q
 * (xq_samples_to_batch_ex below; lc0's q-ratio, KataGo).  Outside the reference-parity contract, like the other opt-in options.
 * WHAT IS WRITTEN.  At the end of every move that stages a sample (k_select and k_select_multi; a fast move of the playout cap
 * stages none and writes nothing), into the sample's `pad` bytes, the layout of xq_sample_root_stats at byte
 * XQ_SAMPLE_ROOT_STATS_OFFSET = 108 of the record:
 *     root_q          float32  the search value of the position from the view of the side to move
 *     root_visits     uint32   the sum of N_i over the root's children
 *     has_root_stats  uint8    1
 *     the other 11 bytes zero.
 * ARITHMETIC, over the RAW tree arrays at the end of the move -- before forced-playout pruning and before the solver's rule-5
 * counts -- so that a host model repeats it bit for bit:
 *     sumW = 0.0 (double), sumN = 0
 *     for i = 0 .. nch-1 in move order:  sumW += W[first+i];  sumN += N[first+i]     (one sequential scan)
 *     root_q = proven >= 0 ? 1.0f : (sumN > 0 ? (float)(sumW / (double)sumN) : 0.0f)  (round to nearest even)
 * proven >= 0 is the solver's rule 4 (the side to move has a proven win); root_visits is the raw sumN in that case too.
 * Without the option the pad bytes stay the zeros the move end fills in.  No draw, visit, move or record changes with the option
 * on or off, outside those 20 bytes.  It goes with leaf batching, tree reuse, the playout cap, forced playouts, the solver, the
 * perpetual-check rule and the evaluation cache.
 * XQ_ERR_ARG before any launch (xq_engine_workspace_bytes_rs: 0): enabled outside {0, 1}; a non-zero reserved word; enabled = 1
 * with manual_moves != 0 (search-only and arena engines record no samples) or with Gumbel root search (its root value is its own
 * v_mix; left for later); and whatever xq_engine_init_sv refuses.  No workspace, no state word, no counter: "root statistics on"
 * lives in the handle (pad0, above the public flag bits) and reaches the kernels as a kernel argument. */
typedef struct xq_root_stats_opts { int32_t enabled; int32_t reserved[3]; } xq_root_stats_opts;
#define XQ_SAMPLE_ROOT_STATS_OFFSET 108
typedef struct xq_sample_root_stats {
    float root_q;
    uint32_t root_visits;
    uint8_t has_root_stats;
    uint8_t zero[11];
} xq_sample_root_stats;
size_t xq_engine_workspace_bytes_rs(const xq_engine_config *cfg, int leaves_per_step, unsigned flags, const xq_playout_cap *cap,
                                    const xq_forced_playouts *forced, const xq_gumbel *gumbel, const xq_arena_opts *arena,
                                    const xq_rules_opts *rules, const xq_solver_opts *solver, const xq_root_stats_opts *root_stats);
int xq_engine_init_rs(xq_engine *eng, const xq_engine_config *cfg, int leaves_per_step, unsigned flags, const xq_playout_cap *cap,
                      const xq_forced_playouts *forced, const xq_gumbel *gumbel, const xq_arena_opts *arena,
                      const xq_rules_opts *rules, const xq_solver_opts *solver, const xq_root_stats_opts *root_stats, void *ws,
                      size_t ws_bytes, const uint64_t *dev_inject, void *stream);

/* Evaluation mirror (opt-in; mirror == NULL or mode = 0 is xq_engine_init_rs exactly -- same workspace bytes, same handle, same
 * kernels launched, same bytes out -- and xq_engine_init_rs is that call).  Xiangqi is left-right symmetric and the trainer doubles
 * every sample by its mirror image, but a search evaluates every request in the orientation its game happens to be in, so whatever
 * left/right asymmetry the network has is backed up into every W with one sign.  With the option each request of the PACKED step is
 * evaluated under a randomly chosen symmetry (AlphaGo Zero; KataGo's self-play does the same): one random bit per request, and the
 * values a search backs up average over the two orientations at no extra evaluator cost.  Outside the reference-parity contract,
 * like the other opt-in options.  mode: 0 off, 1 random; reserved = 0.
 * THE MIRRORED ROW (one device function; xq_mirror_requests_batch runs it over caller-owned rows):
 *     planes  float[15][10][9]: out[p][r][c] = in[p][r][8 - c] in all 15 planes; the centre column maps to itself.
 *     moves   uint16[XQ_MAXM], a = from * 90 + to: both squares' columns go to 8 - c, the arithmetic of xq_samples_to_batch's flip:
 *                 mirror(a) = ((from / 9) * 9 + 8 - from % 9) * 90 + (to / 9) * 9 + 8 - to % 9
 *             word i of the output is mirror(word i of the input): the list keeps its ORDER.  xq_policy_head_legal returns
 *             out[i] for moves[i], so the evaluator's logits come back already un-mirrored and xq_engine_expand_packed does
 *             not know of the option.  (The mirrored position's own move generation lists the same moves as a set, in another
 *             order for most positions: the list must be mirrored in place, not regenerated.)
 *     count   copied.
 *     All XQ_MAXM words are written.  A word at or past the count, or a word that is no action id (>= 8100), is copied as it is:
 *     no evaluator kernel reads past the count.
 * THE BIT of a request is a pure function of (seed, rank, slot, game_seq, ply, is_root, sims_done, row):
 *           h   = philox_u64(seed, rank, slot, 9, game_seq, ply & 0xFFFFFF)
 *           r   = philox_u64(h,    rank, slot, 9, (is_root << 31) | (row << 16) | sims_done, 0)
 *           bit = r >> 63
 *     philox_u64(key, rank, slot, kind, ctr, sub) is the engine's Philox4x32-10: key words (key low, key high), counter words
 *     (slot, kind | sub << 8, ctr, rank), the result is output word 0 in the high half and word 1 in the low half.  Kind 9: no other
 *     draw uses it (0-3 are the four per-slot streams, 7 the start stagger, 8 the arena openings).  The first draw is the key of
 *     the second, so the eight coordinates fit the 32-bit ctr and the 24-bit sub.
 *     The mirrored gather reads the coordinates after xq_engine_select from the slot's state words: game_seq and ply (move_count)
 *     of the real game, is_root = the slot waits for its root's evaluation, sims_done = the simulations done of the current
 *     search (taken as 0 for a root request), row = the request's index among the slot's leaves_per_step rows (0 with K = 1).
 *     No step counter and no state word: eager, graph-replayed and repeated runs agree, and the four per-slot draw streams do
 *     not move -- games with the option on differ from games with it off only through the network's answers.
 *     xq_eval_mirror_bit_host runs the same code on the host and returns 0 or 1; XQ_ERR_ARG for rank, slot or ply < 0, is_root
 *     outside {0, 1}, sims_done outside [0, 16000), row outside [0, 64).
 * WHERE IT ACTS: only in xq_engine_compact, whose gather is then a separate kernel that copies a row whose bit is 0 as before
 * and writes the mirrored row when it is 1; it takes everything from device memory, so the step records into a graph as before.
 * A full-width host (xq_engine_requests + xq_engine_expand_legal) gets NO mirroring: the requests it reads are the slots' own.
 * xq_engine_compact_misses on a mirror engine returns XQ_ERR_ARG: an evaluation-cache hit would return whichever orientation was
 * evaluated first, and the cache's promise of identical games would be false.
 * Allowed: manual_moves 0 and 1, leaf batching, tree reuse, the playout cap, forced playouts, Gumbel root search, the solver, the
 * perpetual-check rule and root statistics.  XQ_ERR_ARG before any launch (xq_engine_workspace_bytes_em: 0): mode outside {0, 1};
 * a non-zero reserved word; mode = 1 with manual_moves = 2 (arena engines, with or without arena options: the gate stays
 * deterministic, and xq_engine_compact_arena shares the plain gather and stays as it is); and whatever xq_engine_init_rs refuses.
 * No workspace, no state word, no counter: "evaluation mirror on" lives in the handle (pad0, bit 31).
 * xq_mirror_requests_batch: rows r < n of dev_x (float32[n][15][10][9], 8-byte aligned), dev_moves (uint16[n][XQ_MAXM]) and
 * dev_counts go to dev_x_out / dev_moves_out, mirrored where dev_flags[r] != 0 (uint8[n]) and copied otherwise; nothing past row
 * n is written.  n = 0 is a no-op; n < 0, a null pointer, a misaligned pointer or an output that is its input return XQ_ERR_ARG.
 * xq_mirror_action_host: mirror(a) on the host, XQ_ERR_ARG outside [0, 8100). */
typedef struct xq_eval_mirror_opts { int32_t mode; int32_t reserved[3]; } xq_eval_mirror_opts;
size_t xq_engine_workspace_bytes_em(const xq_engine_config *cfg, int leaves_per_step, unsigned flags, const xq_playout_cap *cap,
                                    const xq_forced_playouts *forced, const xq_gumbel *gumbel, const xq_arena_opts *arena,
                                    const xq_rules_opts *rules, const xq_solver_opts *solver, const xq_root_stats_opts *root_stats,
                                    const xq_eval_mirror_opts *mirror);
int xq_engine_init_em(xq_engine *eng, const xq_engine_config *cfg, int leaves_per_step, unsigned flags, const xq_playout_cap *cap,
                      const xq_forced_playouts *forced, const xq_gumbel *gumbel, const xq_arena_opts *arena,
                      const xq_rules_opts *rules, const xq_solver_opts *solver, const xq_root_stats_opts *root_stats,
                      const xq_eval_mirror_opts *mirror, void *ws, size_t ws_bytes, const uint64_t *dev_inject, void *stream);
int xq_eval_mirror_bit_host(uint64_t seed, int rank, int slot, uint32_t game_seq, int ply, int is_root, int sims_done, int row);
int xq_mirror_action_host(int action);
int xq_mirror_requests_batch(const float *dev_x, const uint16_t *dev_moves, const int32_t *dev_counts, const uint8_t *dev_flags, int n,
                             float *dev_x_out, uint16_t *dev_moves_out, void *stream);

int xq_engine_select(const xq_engine *eng, float *dev_nn_input /* [G][15][90] */, void *stream);

/* dev_policy[slot] = float32[8100]: network LOGITS (policy_is_probs = 0; softmax over all 8100 as
 * model.py:122 does) or already-softmaxed probabilities (policy_is_probs = 1, evaluator-plugin
 * protocol of mcts.py:157-164).  dev_value[slot] = tanh output. */
int xq_engine_expand(const xq_engine *eng, const float *dev_policy, const float *dev_value,
                     int policy_is_probs, void *stream);

/* Sparse hand-off between the engine and the evaluator (replaces the dense 8100-wide policy row of mcts.py:157-188).
 * xq_engine_requests: after xq_engine_select, *dev_moves = uint16[G][XQ_MAXM] holds the ORDERED legal moves of the
 * position each slot handed to the evaluator and *dev_counts = int32[G] their number (0: the slot asked for nothing this
 * step).  Both point into the engine's workspace and stay valid for its lifetime.
 * xq_engine_expand_legal: like xq_engine_expand, but dev_legal_logits[slot][m] is the network's logit of legal move m
 * only.  Priors = softmax over the legal logits, summed sequentially in float32 in move order and divided -- the
 * reference's softmax over all 8100 followed by mask-and-normalise (model.py:122, mcts.py:176-188), whose common factor
 * exp(max_legal - max_all)/denominator cancels; identical up to float32 rounding unless the reference's float32 softmax
 * underflows (a logit gap above ~87), where the reference degrades to denormal or uniform priors and this stays exact. */
int xq_engine_requests(const xq_engine *eng, const uint16_t **dev_moves, const int32_t **dev_counts);
int xq_engine_expand_legal(const xq_engine *eng, const float *dev_legal_logits, const float *dev_value, void *stream);

/* Packed step: the evaluator runs only over the slots that asked for an evaluation.  A C host calls, on one stream,
 *     xq_engine_select(eng, nn_input)                 as before
 *     xq_engine_compact(eng, nn_input)                stable, slot-ordered compaction of the waiting slots (phase
 *                                                     WAIT_ROOT / WAIT_LEAF: exactly k_expand's test) into engine-owned
 *                                                     buffers: *n_live, rows[r] = slot of packed row r, x[r] = nn_input[rows[r]],
 *                                                     moves[r] / counts[r] = that slot's request (xq_engine_requests)
 *     <evaluator over x, moves, counts>               the *_live entry points below, capacity = n_games, dev_n = n_live:
 *                                                     rows [0, *n_live) are computed, nothing past them is read or written
 *     xq_engine_expand_packed(eng, logits, value)     scatters packed row r's float32[XQ_MAXM] legal logits and value back to
 *                                                     slot rows[r] of slot_logits / slot_value and runs xq_engine_expand_legal
 *                                                     on them (slots that asked for nothing are ignored there, as always)
 * The row count stays in device memory: no host synchronisation, and the sequence records into one replayable graph whose
 * launch grids are sized for n_games.  n_live = 0 is a valid step.  Results are identical to the full-width step (select,
 * evaluator over all n_games rows, xq_engine_expand_legal): a row's arithmetic in every evaluator kernel does not depend on
 * its position in the batch.  xq_engine_packed returns the buffers' addresses (workspace, valid for the engine's lifetime). */
typedef struct xq_engine_packed_buffers {
    const int32_t *n_live;        /* int32, device */
    const int32_t *rows;          /* int32[G] */
    const float *x;               /* float32[G][15][10][9], rows [0, n_live) valid */
    const uint16_t *moves;        /* uint16[G][XQ_MAXM] */
    const int32_t *counts;        /* int32[G] */
    const float *slot_logits;     /* float32[G][XQ_MAXM], slot-ordered hand-back of xq_engine_expand_packed */
    const float *slot_value;      /* float32[G] */
} xq_engine_packed_buffers;
int xq_engine_compact(const xq_engine *eng, const float *dev_nn_input, void *stream);
int xq_engine_packed(const xq_engine *eng, xq_engine_packed_buffers *out);
int xq_engine_expand_packed(const xq_engine *eng, const float *dev_packed_logits, const float *dev_packed_value, void *stream);
/* the per-model packed step of an engine with arena options (rules: xq_engine_init_ar above) */
int xq_engine_compact_arena(const xq_engine *eng, const float *dev_nn_input, void *stream);
int xq_engine_packed_arena(const xq_engine *eng, xq_engine_packed_buffers out[2]);
int xq_engine_expand_packed_arena(const xq_engine *eng, const float *dev_logits_new, const float *dev_value_new,
                                  const float *dev_logits_old, const float *dev_value_old, void *stream);

/* Evaluation cache (opt-in): a table private to each slot that remembers the legal-move logits and value the network
 * returned for a position, so the next search, which revisits most of the previous move's subtree, does not ask again.
 * A request's output depends only on its 15 input planes, so a cached row is bit-identical to a recomputed one and the
 * games do not change.  The cached step, on one stream:
 *     xq_engine_select(eng, nn_input)
 *     xq_evcache_probe(cache, eng, nn_input)          per waiting slot: key from nn_input, probe the slot's set; a hit writes
 *                                                     the slot's row of slot_logits / slot_value and sets its hit flag
 *     xq_engine_compact_misses(eng, nn_input, hit)    xq_engine_compact restricted to waiting slots whose flag is 0
 *                                                     (rows_evaluated counts only these rows)
 *     <evaluator over the packed rows>                as in the packed step
 *     xq_engine_expand_packed(eng, logits, value)     as in the packed step
 *     xq_evcache_commit(cache, eng, logits, value)    each evaluated row inserts its slot's key, logits, value and count
 *                                                     (it reads only the packed rows: before or after the expansion alike)
 * Every count stays in device memory and every grid is sized by n_games: the sequence records into one graph.
 * Table: per slot `entries_per_slot` (K, a power of two) entries in sets of min(4, K) ways, one caller-owned allocation of
 * xq_evcache_bytes(n_slots, K) bytes: per entry a 12-word key (90 squares x 4 bits + the side to move), generation, stamp,
 * legal-move count, float32 value and float32[XQ_MAXM] logits -- 576 B -- plus ~100 B per slot.  A hit needs the whole key,
 * the current generation and the count to match (a key match with another count is a "mismatch": counted, never expected,
 * treated as a miss).  The victim is an entry of an older generation, else the least recently stamped (lowest way on ties).
 * xq_evcache_invalidate bumps the device-side generation (after a weight update): older entries never hit again.
 * Errors: K zero or not a power of two, null pointers, logits not 8-byte aligned, or a cache whose n_slots differs from the
 * engine's n_games return XQ_ERR_ARG before any launch.  xq_evcache_bytes returns 0 for invalid arguments. */
typedef struct xq_evcache {
    int32_t n_slots, entries, ways, sets;
    void *p[16];                  /* device addresses in the caller's allocation; treat as opaque */
} xq_evcache;
typedef struct xq_evcache_stats {
    uint64_t probes;              /* waiting slots probed */
    uint64_t hits;                /* probes answered from the table (their rows were not evaluated) */
    uint64_t inserts, evictions;  /* evictions: inserts that replaced a current-generation entry */
    uint64_t mismatches;          /* key and generation matched, legal-move count did not: must stay 0 */
    uint64_t reserved[3];
} xq_evcache_stats;
size_t xq_evcache_bytes(int n_slots, int entries_per_slot);
/* Carves dev_mem (256-byte aligned, >= xq_evcache_bytes) and clears the table (asynchronous on stream). */
int xq_evcache_init(xq_evcache *cache, int n_slots, int entries_per_slot, void *dev_mem, size_t bytes, void *stream);
/* *dev_hit = int32[n_slots] hit flags written by xq_evcache_probe (valid for waiting slots of the current step). */
int xq_evcache_hit_flags(const xq_evcache *cache, const int32_t **dev_hit);
int xq_evcache_probe(const xq_evcache *cache, const xq_engine *eng, const float *dev_nn_input, void *stream);
int xq_engine_compact_misses(const xq_engine *eng, const float *dev_nn_input, const int32_t *dev_hit_flags, void *stream);
int xq_evcache_commit(const xq_evcache *cache, const xq_engine *eng, const float *dev_packed_logits,
                      const float *dev_packed_value, void *stream);
int xq_evcache_invalidate(const xq_evcache *cache, void *stream);
/* Synchronises `stream`, sums the per-slot counters. */
int xq_evcache_stats_read(const xq_evcache *cache, xq_evcache_stats *host_out, void *stream);
/* The key the probe builds, computed on the host from one position's float32[15][90] planes (tests). */
int xq_evcache_key_host(const float *host_planes, uint32_t *host_out12);

/* Request dedup (opt-in): within one step, slots that ask for the same position share one evaluated row.  The packed step
 * drops idle slots and the evaluation cache drops what the SAME slot asked before; this drops what DIFFERENT slots ask in the
 * SAME step (a lockstep start, the first plies of every search).  It rests on the cache's two premises -- a request's output
 * depends only on its 15 planes, and an evaluator kernel's arithmetic for a row does not depend on the row's place in the
 * batch -- so the games do not change; rows_evaluated counts the rows the network really ran.  The dedup step, on one stream:
 *     xq_engine_select(eng, nn_input)
 *     xq_engine_compact_unique(dedup, eng, nn_input)  three kernels and the packed step's gather:
 *                                                     keys     per waiting slot s: the cache's 12-word key of its planes, and
 *                                                              atomicMin(&table[hash(key) & (T - 1)], s)
 *                                                     resolve  with m = the bucket's minimum: rep[s] = m when m != s, all 12
 *                                                              key words agree and the legal-move counts agree, else s
 *                                                     compact  xq_engine_compact restricted to waiting slots with rep[s] == s,
 *                                                              into the engine's own live count and row map; the buckets
 *                                                              this step used are stored back to "empty"
 *     <evaluator over the packed rows>                as in the packed step
 *     xq_engine_expand_dedup(dedup, eng, logits, value)   per waiting slot s: the packed row of rep[s] goes to slot s of
 *                                                     slot_logits / slot_value; then xq_engine_expand_legal
 * Every count stays in device memory and every grid is sized by n_games: the sequence records into one graph.
 * Table: T = the smallest power of two >= max(16, 4 n_slots) int32 buckets, empty (INT32_MAX) before and after every
 * xq_engine_compact_unique / xq_dedup_rows_batch, eager or replayed; one caller-owned allocation of xq_evdedup_bytes(n_slots)
 * bytes holds it with 92 B per slot (key, bucket, representative, packed row, four counters).  The minimum does not depend on
 * the order of the atomics, so the representative of a group is its lowest slot, always.  Two different keys in one bucket are a
 * "collision": the higher slot evaluates itself.  Equal keys under different legal-move counts are a "mismatch": never
 * expected, counted, the slot evaluates itself.  Neither can change an answer.  Nothing is kept from one step to the next, so a
 * weight update needs no invalidation.
 * Refused with XQ_ERR_ARG before any launch: null pointers, logits not 8-byte aligned, a dedup whose n_slots differs from the
 * engine's n_games, and an engine the dedup cannot serve: leaf batching (xq_engine_init_leaves, K > 1: a slot asks for several
 * rows), the evaluation mirror (xq_engine_init_em: equal planes are evaluated under different orientations) and arena games
 * (manual_moves = 2: two models answer).  The evaluation cache is an object of its own that neither handle knows of: its step
 * (xq_evcache_probe / xq_engine_compact_misses) and this one are alternatives, and the Python engine refuses to own both.
 * xq_evdedup_bytes returns 0 for n_slots <= 0 or above 2^24. */
typedef struct xq_evdedup {
    int32_t n_slots, table_size, reserved[2];
    void *p[8];                   /* device addresses in the caller's allocation; treat as opaque */
} xq_evdedup;
typedef struct xq_evdedup_stats {
    uint64_t requests;            /* waiting slots (or live rows) seen */
    uint64_t merged;              /* requests answered by another slot's row: requests - merged rows were evaluated */
    uint64_t collisions;          /* another key held the bucket: not merged, evaluated */
    uint64_t mismatches;          /* the key matched, the legal-move count did not: must stay 0 */
    uint64_t reserved[4];
} xq_evdedup_stats;
size_t xq_evdedup_bytes(int n_slots);
/* Carves dev_mem (256-byte aligned, >= xq_evdedup_bytes), empties the table and zeroes the counters (asynchronous on stream). */
int xq_evdedup_init(xq_evdedup *dedup, int n_slots, void *dev_mem, size_t bytes, void *stream);
int xq_engine_compact_unique(const xq_evdedup *dedup, const xq_engine *eng, const float *dev_nn_input, void *stream);
int xq_engine_expand_dedup(const xq_evdedup *dedup, const xq_engine *eng, const float *dev_packed_logits,
                           const float *dev_packed_value, void *stream);
/* Synchronises `stream`, sums the per-slot counters. */
int xq_evdedup_stats_read(const xq_evdedup *dedup, xq_evdedup_stats *host_out, void *stream);
/* The bucket of a 12-word key (xq_evcache_key_host) in a table of table_size buckets, a power of two; needs no GPU.
 * XQ_ERR_ARG for a null key or another size. */
int xq_evdedup_bucket_host(const uint32_t *key12, int table_size);
/* The same keys / resolve / compact kernels over n <= n_slots caller-owned request rows (tests, tools): dev_x float32[n][15][90],
 * dev_counts int32[n] legal-move counts, dev_live_flags int32[n] (0: the row asks for nothing and nothing of it is read past
 * its flag or written).  dev_rep_out int32[n] receives rep[] of the live rows, dev_rows_out int32[n] the representatives in
 * row order, dev_n_out int32[1] their number; the dedup's counters count the live rows.  n = 0 writes *dev_n_out = 0. */
int xq_dedup_rows_batch(const float *dev_x, const int32_t *dev_counts, const int32_t *dev_live_flags, int n,
                        const xq_evdedup *dedup, int32_t *dev_rep_out, int32_t *dev_rows_out, int32_t *dev_n_out, void *stream);

/* Synchronises `stream`, copies the counters to host. */
int xq_engine_stats_read(const xq_engine *eng, xq_engine_stats *host_out, void *stream);

/* Synchronises; copies the finished samples (XQ_SAMPLE_BYTES each, layout xq_sample) and the game results (xq_game_result)
 * that are pending in the rings to host buffers and resets the rings.
 * What a drain returns, full rings included:
 *   - samples: every row was written since the last drain, by a finished game that is there whole (all n_samples rows of its
 *     result, contiguous) or not at all.  A game finds room only while its rows fit under cfg.max_out_samples: one that does not
 *     fit is dropped whole, counted in samples_dropped and leaves the ring as it was, so a later, shorter game may still fit.
 *     The rows of all drains add up to samples_written; samples_written + samples_dropped is the n_samples of all finished games.
 *   - results: the first min(games finished since the last drain, cfg.max_out_results) of them, in the order they finished;
 *     a result is returned whether or not its game's samples were dropped.
 *   - a full ring is no capacity error: overflow stays 0, the games go on unchanged.
 * max_samples / max_results smaller than what is pending: XQ_ERR_ARG, *n_samples / *n_results report the pending sizes and
 * nothing is consumed. */
int xq_engine_drain(const xq_engine *eng, void *host_samples, int max_samples, int *n_samples,
                    void *host_results, int max_results, int *n_results, void *stream);

/* The same into DEVICE buffers (the samples stay on the GPU for the replay buffer / the RCCL all-gather; nothing crosses
 * PCIe); the same rows under the same contract.  With both buffers NULL it only reports the pending counts and consumes
 * nothing; so does a call whose buffers are too small (XQ_ERR_ARG).  Synchronises. */
int xq_engine_drain_device(const xq_engine *eng, void *dev_samples, int max_samples, int *n_samples,
                           void *dev_results, int max_results, int *n_results, void *stream);

/* Test / serving hooks (MCTS.search for a given position, mcts.py:94-155). Synchronise. */
int xq_engine_set_position(const xq_engine *eng, int slot, const int8_t *host_board, int side, int move_count,
                           int no_capture, const int8_t *host_hist12 /* int8[12][90], oldest first, last
                           min(12,move_count) valid */, const double *host_noise /* eta per legal move or NULL */,
                           void *stream);
/* Root children of `slot` after a search: returns n; arrays sized XQ_MAXM. prior_kind: 0 float32, 1 float64, 3 float64 g + l of a
 * Gumbel root (xq_engine_init_gz). */
int xq_engine_read_root(const xq_engine *eng, int slot, uint16_t *actions, int32_t *visits, double *total_value,
                        double *prior, int *prior_kind, int32_t *root_visits, int32_t *sims_done, void *stream);

/* =====================================================================================
 * B2 -- evaluator plug point helpers (training/model.py:20-36, 87-107 run over the leaf batch).
 * ===================================================================================== */

/* y = act(y + bias[c] (+ residual)) in place over a channels-last float32 tensor [rows][channels]
 * (folded BatchNorm bias + ReLU + skip connection of ResBlock.forward, model.py:30-36).
 * channels % 4 == 0, pointers 16-byte aligned; dev_residual may be NULL. */
int xq_bias_act(float *dev_y, const float *dev_bias, const float *dev_residual, long long rows, int channels,
                int relu, void *stream);

/* Input convolution (model.py:87-93: Conv2d(15, C, 3, padding=1), BatchNorm folded, ReLU) straight from the encoder's
 * planes:  y = relu(conv(planes) + bias).  Exact for any input; fast because the planes are sparse (zero inputs are skipped).
 *   dev_planes : float32[games][15][10][9] (xq_engine_select's nn_input);  dev_y : float32[games][90][channels] (NHWC);
 *   dev_wt : float32[135][channels], dev_wt[plane*9 + ky*3 + kx][co] = folded filter w[co][plane][ky][kx];
 *   dev_bias : float32[channels].  channels % 4 == 0. */
int xq_stem_conv(const float *dev_planes, const float *dev_wt, const float *dev_bias, float *dev_y, int games,
                 int channels, void *stream);

/* Both heads' 1x1 convolutions (model.py:43-62: policy Conv2d(C,32,1), value Conv2d(C,4,1), BatchNorm folded, ReLU) in one
 * pass over the tower output:  out[r][o] = relu(bias[o] + sum_c h[r][c] w[o][c]),  o < 36.
 *   dev_h : float32[rows][channels] (NHWC rows);  dev_w : float32[36][channels], rows 0-31 policy, 32-35 value;
 *   dev_bias : float32[36];  dev_p : float32[rows][32];  dev_v : float32[rows][4].  channels % 16 == 0, <= 1024. */
int xq_heads_1x1(const float *dev_h, const float *dev_w, const float *dev_bias, float *dev_p, float *dev_v,
                 long long rows, int channels, void *stream);

/* Live-row variants of the evaluator kernels (the packed step above).  Each takes the CAPACITY where its plain twin takes
 * the batch -- launch grids are sized by it, so a recorded graph stays valid -- and dev_n, an int32 in device memory that
 * holds the live count n (clamped to [0, capacity]): positions [0, n) are computed bit-identically to the plain entry point,
 * positions past n are neither read nor written, n = 0 does nothing.  Capacity 0 is a no-op; a negative capacity or a null
 * dev_n is XQ_ERR_ARG.  xq_heads_1x1_live: `rows` = capacity x 90 and n counts positions (90 rows each). */
int xq_stem_conv_live(const float *dev_planes, const float *dev_wt, const float *dev_bias, float *dev_y, int capacity,
                      const int32_t *dev_n, int channels, void *stream);
int xq_heads_1x1_live(const float *dev_h, const float *dev_w, const float *dev_bias, float *dev_p, float *dev_v,
                      long long rows, const int32_t *dev_n, int channels, void *stream);

/* Policy head's Linear(2880, 8100) (model.py:64-71) evaluated ONLY at the ordered legal moves of each pending evaluation
 * -- what mcts.py:176-188 keeps of the 8 100 logits:  dev_out[g][m] = dev_bias[a] + <dev_feat[g], dev_w[a]>,
 * a = dev_moves[g][m], m < dev_counts[g] (counts <= 0: the game is skipped, its row is left untouched).
 *   dev_feat : float32[games][2880], the policy features in NHWC order (position-major, 32 channels) as xq_heads_1x1 writes
 *              them;  dev_w : float32[8100][2880] with the columns permuted to that order
 *              (w[a][hw*32 + c] = policy_head.4.weight[a][c*90 + hw]);  dev_bias : float32[8100];
 *   dev_moves : uint16[games][XQ_MAXM], dev_counts : int32[games] (xq_engine_requests);  dev_out : float32[games][XQ_MAXM]. */
int xq_policy_head_legal(const float *dev_feat, const float *dev_w, const float *dev_bias, const uint16_t *dev_moves,
                         const int32_t *dev_counts, int games, float *dev_out, void *stream);

/* Value head's Linear(360,128) + ReLU + Linear(128,1) + tanh (model.py:73-85) over the value features float32[games][360]
 * (NHWC order, xq_heads_1x1's dev_v):  dev_w1t : float32[360][128], w1t[hw*4 + c][j] = value_head.4.weight[j][c*90 + hw];
 * dev_b1 float32[128]; dev_w2 float32[128] = value_head.6.weight[0]; dev_b2 float32[1];  dev_value : float32[games]. */
int xq_value_head(const float *dev_vfeat, const float *dev_w1t, const float *dev_b1, const float *dev_w2,
                  const float *dev_b2, int games, float *dev_value, void *stream);
/* live-row variants (see xq_stem_conv_live) */
int xq_policy_head_legal_live(const float *dev_feat, const float *dev_w, const float *dev_bias, const uint16_t *dev_moves,
                              const int32_t *dev_counts, int capacity, const int32_t *dev_n, float *dev_out, void *stream);
int xq_value_head_live(const float *dev_vfeat, const float *dev_w1t, const float *dev_b1, const float *dev_w2,
                       const float *dev_b2, int capacity, const int32_t *dev_n, float *dev_value, void *stream);

/* 3x3 convolution, stride 1, pad 1, C -> C channels (ResBlock.conv1/conv2 with BatchNorm folded, model.py:25-36)
 * as fused Winograd F(2x3,3x3) -- F(2,3) along the 10 rows, F(3,3) at the points 0, +-1, 2, inf along the 9 columns -- on
 * the fp32 MFMA:  y = act(conv(x) + bias (+ residual)).
 *   dev_x, dev_y, dev_residual : float32[batch][90][channels] (NHWC; y must not alias x or residual)
 *   dev_u : pre-transformed weights, float32[C/64][C/8][20][2][64][4] with
 *           u[cog][chunk][5p+j][quad][co][k] = s_p (G_r g G_c'^T)[p][j] for output channel 64*cog+co and input channel
 *           8*chunk+4*quad+k, g = the folded 3x3 filter (cross-correlation, as torch.nn.Conv2d), G_r the F(2,3) matrix,
 *           G_c' = diag(1/2, 1/2, 1/6, 1/6, 1) [[1,0,0],[1,1,1],[1,-1,1],[1,2,4],[0,0,1]], s_p = -1 for p = 2 and +1
 *           otherwise (the kernel forms row 2 of B_r^T d with the opposite sign);
 *           xq_wino_weight_bytes(C) = 80 C^2 bytes.  channels in {64, 128, 256, 512}; batch*90*channels*4 < 2^32. */
size_t xq_wino_weight_bytes(int channels);
int xq_wino_conv3x3(const float *dev_x, const float *dev_u, const float *dev_bias, const float *dev_residual,
                    float *dev_y, int batch, int channels, int flags, void *stream);
/* flags: bit 0 = ReLU; bit 1 = walk the batch back to front (same results; alternate it between consecutive layers so
 * that each launch first reads what the previous one wrote last, while it is still in the Infinity Cache). */
#define XQ_CONV_RELU 1
#define XQ_CONV_REVERSE 2
/* bit 2: "wide" variant -- 128 output channels per workgroup (one workgroup per CU, 320 accumulators per wave): dev_u is then
 * float32[C/128][C/8][20][2][128][4] (the same element formula with 128-channel blocks), channels in {128, 256, 512}. */
#define XQ_CONV_WIDE 4
/* live-row variant (see xq_stem_conv_live): tile groups, the XQ_CONV_REVERSE walk and the buffer extents follow *dev_n */
int xq_wino_conv3x3_live(const float *dev_x, const float *dev_u, const float *dev_bias, const float *dev_residual,
                         float *dev_y, int capacity, const int32_t *dev_n, int channels, int flags, void *stream);

/* The filter transform of xq_wino_conv3x3 on the device (the train step re-transforms after every optimizer step; self-play
 * transforms once per weight update and may use this or the host's float64 einsum, which give the same float32 values):
 *   dev_w : float32[C][C][3][3] (torch.nn.Conv2d.weight, train.py:376-447 trains it);  dev_u : xq_wino_weight_bytes(C) bytes in the
 *   layout above (64-channel blocks, or 128 with XQ_CONV_WIDE in flags).  With XQ_FILTER_DGRAD the filters of the DATA-GRADIENT
 *   convolution are produced, w'[co][ci][r][s] = w[ci][co][2-r][2-s]: xq_wino_conv3x3(dL/dy, u', 0-bias) is dL/dx of
 *   y = conv3x3(x, w) (stride 1, pad 1) -- what torch autograd's convolution_backward computes for ResBlock.conv1/conv2. */
#define XQ_FILTER_DGRAD 8
/* XQ_FILTER_BOTH: forward filters into dev_u[0 .. 20 C^2) and data-gradient filters into dev_u[20 C^2 .. 40 C^2) (floats) in one launch;
 * dev_u then holds 2 * xq_wino_weight_bytes(C) bytes. */
#define XQ_FILTER_BOTH 16
int xq_wino_transform_filters(const float *dev_w, float *dev_u, int channels, int flags, void *stream);

/* BatchNorm2d in TRAINING mode fused with the ReLU / skip-add around it in a ResBlock (training/model.py:20-36: bn1 + relu, bn2 + add +
 * relu; trained by training/train.py:376-447), on NHWC activations float32[rows][channels], rows = batch * 90:
 *   forward :  y = act((x - mean) * invstd * gamma + beta (+ residual)) with the batch statistics of the rows (biased variance);
 *              running_mean / running_var (nullable pair) updated as torch.nn.BatchNorm2d does (momentum, unbiased variance);
 *              save_mean / save_invstd float32[channels] are kept for the backward call; dev_batches_tracked (nullable): the module's
 *              int64 num_batches_tracked, incremented by one.  relu: 0 / 1.
 *   backward:  g = dy * (y > 0) if relu;  dbeta = sum g;  dgamma = sum g * xhat;  dx = gamma * invstd * (g - dbeta / rows - xhat * dgamma / rows);
 *              dev_dresidual (nullable) receives g, the gradient of the skip input.
 * Sums are float64 per row segment, reduced in a fixed order (deterministic).  dev_scratch: xq_bn_scratch_bytes(channels) bytes.
 * channels in {64, 128, 256, 512, 1024}; all pointers 16-byte aligned. */
size_t xq_bn_scratch_bytes(int channels);
int xq_bn_train_forward(const float *dev_x, const float *dev_residual, const float *dev_gamma, const float *dev_beta,
                        float *dev_running_mean, float *dev_running_var, float momentum, float eps, long long rows, int channels,
                        int relu, float *dev_y, float *dev_save_mean, float *dev_save_invstd, long long *dev_batches_tracked,
                        void *dev_scratch, void *stream);
int xq_bn_train_backward(const float *dev_dy, const float *dev_x, const float *dev_y, const float *dev_gamma, const float *dev_save_mean,
                         const float *dev_save_invstd, long long rows, int channels, int relu, float *dev_dx, float *dev_dresidual,
                         float *dev_dgamma, float *dev_dbeta, void *dev_scratch, void *stream);

/* The same BatchNorm with the statistics of a whole GROUP of ranks (torch.nn.SyncBatchNorm semantics: the data-parallel train step),
 * split where the host runs its collective.  dev_sums: xq_bn_sync_sums_count(channels) = 2 * channels + 1 doubles on the device,
 * 8-byte aligned.  A stats call writes this rank's per-channel sums, the host all-reduces them (SUM, float64) over the group, the
 * apply call reads the group's:
 *   forward :  xq_bn_sync_forward_stats   -> sums = [sum x (C) | sum x^2 (C) | rows]
 *              all-reduce(sums)
 *              xq_bn_sync_forward_apply   -> y, save_mean / save_invstd of the group's batch, running statistics updated with the
 *                                            group's count n (unbiased variance var * n / (n - 1)), num_batches_tracked += 1;
 *   backward:  xq_bn_sync_backward_stats  -> sums = [sum g (C) | sum g * xhat (C) | rows]; dev_dgamma / dev_dbeta receive this rank's
 *                                            LOCAL sums (what SyncBatchNorm's backward returns; the data-parallel gradient all-reduce
 *                                            combines them with the other gradients)
 *              all-reduce(sums)
 *              xq_bn_sync_backward_apply  -> dx with the group's sum g, sum g * xhat and n; dev_dresidual (nullable) receives g.
 * rows is this rank's row count in every call (ranks may hold different counts); dev_scratch: xq_bn_scratch_bytes(channels) bytes, free
 * again when the stats call's kernels have run.  Argument rules as the fused entry points.  With one rank (the all-reduce leaves the sums
 * as they are) every output is bit-identical to xq_bn_train_forward / xq_bn_train_backward: the same partials, summed in the same order,
 * the same finalize arithmetic. */
size_t xq_bn_sync_sums_count(int channels);
int xq_bn_sync_forward_stats(const float *dev_x, long long rows, int channels, double *dev_sums, void *dev_scratch, void *stream);
int xq_bn_sync_forward_apply(const float *dev_x, const float *dev_residual, const float *dev_gamma, const float *dev_beta,
                             float *dev_running_mean, float *dev_running_var, float momentum, float eps, long long rows, int channels,
                             int relu, const double *dev_sums, float *dev_y, float *dev_save_mean, float *dev_save_invstd,
                             long long *dev_batches_tracked, void *stream);
int xq_bn_sync_backward_stats(const float *dev_dy, const float *dev_x, const float *dev_y, const float *dev_save_mean,
                              const float *dev_save_invstd, long long rows, int channels, int relu, double *dev_sums, float *dev_dgamma,
                              float *dev_dbeta, void *dev_scratch, void *stream);
int xq_bn_sync_backward_apply(const float *dev_dy, const float *dev_x, const float *dev_y, const float *dev_gamma, const float *dev_save_mean,
                              const float *dev_save_invstd, long long rows, int channels, int relu, const double *dev_sums, float *dev_dx,
                              float *dev_dresidual, void *stream);

/* Weight gradient of y = conv3x3(x, w) (stride 1, pad 1, C -> C; what torch autograd's convolution_backward returns for
 * ResBlock.conv1/conv2.weight under training/train.py:376-447), in the Winograd domain of xq_wino_conv3x3 on the fp32 MFMA:
 *   dev_x, dev_dy : float32[batch][90][channels] (NHWC);  dev_dw : float32[channels][channels][3][3] (torch's layout), overwritten;
 *   dev_scratch   : xq_wino_wgrad_scratch_bytes(batch, channels) bytes (per-split partial sums, added in a fixed order: deterministic).
 * channels in {64, 128, 256, 512}. */
size_t xq_wino_wgrad_scratch_bytes(int batch, int channels);
int xq_wino_wgrad(const float *dev_x, const float *dev_dy, float *dev_dw, void *dev_scratch, int batch, int channels, void *stream);

/* REDUCED-PRECISION throughput mode of the same convolution (never the parity path; outside the 1e-5 contract): the identical
 * fused Winograd decomposition with the 20 per-frequency products on the bf16 MFMA (operands rounded to bf16 after the float32
 * transforms, float32 accumulation, float32 activations in HBM).  Replaces nothing in the reference -- its own inference is
 * float32 (model.py:109-124); it is the "throughput mode" of SURVEY.md section 7.
 *   dev_u_bf16 : bf16[C/128][C/16][20][2][128][8], u[cog][chunk][5p+j][h][co][k] = the float32 tensor's element for output
 *                channel 128*cog+co and input channel 16*chunk+8*h+k, rounded to nearest-even;  xq_wino_weight_bytes_bf16(C) = 40 C^2.
 *   channels in {128, 256, 512}; flags: XQ_CONV_RELU, XQ_CONV_REVERSE. */
size_t xq_wino_weight_bytes_bf16(int channels);
int xq_wino_conv3x3_bf16(const float *dev_x, const void *dev_u_bf16, const float *dev_bias, const float *dev_residual,
                         float *dev_y, int batch, int channels, int flags, void *stream);
/* live-row variant (see xq_stem_conv_live) */
int xq_wino_conv3x3_bf16_live(const float *dev_x, const void *dev_u_bf16, const float *dev_bias, const float *dev_residual,
                              float *dev_y, int capacity, const int32_t *dev_n, int channels, int flags, void *stream);

/* =====================================================================================
 * Next row (section 8f.1) -- training-batch materialisation.  Replaces SelfPlayDataset.__getitem__ + augment_data
 * (training/train.py:114-151) and _augment_data (training/parallel_selfplay.py:137-151) for a batch drawn from a
 * device-resident buffer of compact samples: output j is sample dev_index[j] (mirrored left-right when dev_flip[j]):
 * dev_states[j] float32[15][10][9], dev_pi[j] float32[8100] (visits^(1/T) normalised in float64, cast to float32),
 * dev_z[j] float32.  dev_samples: xq_sample[...] in device memory.
 * ===================================================================================== */
int xq_samples_to_batch(const void *dev_samples, const int32_t *dev_index, const uint8_t *dev_flip, int n,
                        double late_temperature, float *dev_states, float *dev_pi, float *dev_z, void *stream);

/* The same with a q-mixed value target (opt-in; opts == NULL or q_mix = 0.0 gives xq_samples_to_batch's three outputs byte for
 * byte, and xq_samples_to_batch is that call).  For a record whose has_root_stats is 1 (xq_engine_init_rs), in float64, products
 * and the sum in the order written, no fused multiply-add:
 *     dev_z[j] = (float)((1.0 - q_mix) * (double)z + q_mix * (double)root_q)
 * A record without the mark gets (float)z.  The mirror flag does not touch the value; planes and pi do not depend on the option.
 * XQ_ERR_ARG before any launch: q_mix outside [0, 1] or NaN, a non-zero reserved word, and xq_samples_to_batch's argument rules.
 * n = 0 is a no-op. */
typedef struct xq_batch_opts { double q_mix; int32_t reserved[2]; } xq_batch_opts;
int xq_samples_to_batch_ex(const void *dev_samples, const int32_t *dev_index, const uint8_t *dev_flip, int n,
                           double late_temperature, const xq_batch_opts *opts, float *dev_states, float *dev_pi, float *dev_z,
                           void *stream);

/* Finished training sample (compact form of the reference's (state, pi, z) tuple,
 * parallel_selfplay.py:97-99,123-132; dense pi / planes / flip augmentation materialise on the consumer). */
typedef struct xq_sample {
    int8_t board[XQ_SQUARES];
    int8_t side;        /* player to move when the sample was taken */
    int8_t z;           /* +1 win / 0 draw / -1 loss from `side`'s view */
    uint8_t n_moves;
    uint8_t late_temp;  /* 0: T = 1.0, 1: T = late_temperature */
    uint16_t ply;       /* move_count */
    uint16_t reserved0, reserved1; /* explicit: no implicit padding anywhere in this struct */
    uint32_t slot, game_seq;
    uint8_t pad[20];
    uint16_t actions[XQ_MAXM];
    uint16_t visits[XQ_MAXM];
} xq_sample;

typedef struct xq_game_result {
    uint32_t slot, game_seq;
    int8_t winner;      /* +1 / -1 / 0 */
    uint8_t reason;     /* 1 rules (is_game_over), 2 max_game_length adjudication, 3 resign, 4 rules: repetition, perpetual check
                         * (xq_engine_init_ru only), 5 an endgame table (xq_engine_adjudicate only) */
    uint16_t steps;     /* game.move_count */
    uint16_t n_samples;
    uint16_t reserved;
} xq_game_result;

/* Game records (opt-in, xq_engine_init_gr): every finished game's moves, and a batched device replay of records.
 * THE RECORD: 1024 bytes, no implicit padding.  slot and game_seq join it with the game's xq_game_result and xq_sample rows;
 * winner, reason and n_samples are the result's; n_moves is the result's steps.  moves[i] is the action (from * 90 + to) of ply i
 * of the real game, in ply order, whoever chose it: a random opening ply, an arena opening ply or a searched move (fast moves of
 * the playout cap and arena moves included); the entries at and after n_moves are 0.  opening_plies counts the leading plies no
 * search chose: the random opening of a self-play game, the paired opening of an arena game; an opening whose plies ended the
 * game restarted it from the initial position at ply 0, and opening_plies is then 0, as the arena's own opening record has it.
 * THE ENGINE: xq_engine_workspace_bytes_gr / xq_engine_init_gr are the widest pair: everything the _em pair takes, then the
 * options.  NULL or enabled = 0 is exactly the _em pair: the same workspace size, the same bytes, the same launches.  XQ_ERR_ARG
 * before any launch (xq_engine_workspace_bytes_gr: 0): a non-zero reserved word; enabled outside {0, 1}; and, with enabled = 1,
 * max_out_games < 1, manual_moves = 1 (a search-only engine plays no games), max_game_length > XQ_RECORD_MAX_PLIES or
 * random_opening_moves > XQ_RECORD_MAX_PLIES; and whatever xq_engine_init_em refuses.  Every other option goes with it, leaf
 * batching included.  Workspace: behind the engine's square-root table (THE OPTION WORDS below: the region's tail), a ring of
 * max_out_games records, a move log uint16[G][XQ_RECORD_MAX_PLIES], the opening count of every slot, and 256 bytes holding the
 * ring's counter and the two statistics; "game records on" lives in the handle (pad0, bit 23).  The handle's layout and size do
 * not change.
 * Every real move writes log[slot][move_count before the move] = action with one 2-byte store of lane 0; an index at or above
 * XQ_RECORD_MAX_PLIES is never written and sets overflow bit 256 << 8 (it cannot happen within the refusals above: rules end a
 * game at ply 200).  A finished game's record is written by xq_engine_select, in a kernel of its own ahead of the select kernel
 * that flushes the game's samples and result and starts the slot's next game (one more launch per step, on a records engine
 * only): the game takes the next ring index r; r < max_out_games copies the header and the n_moves entries to row r, zeroes the
 * rest of the row and counts in `recorded`; otherwise the game counts in `dropped`.  Games that finish in one step take their
 * rows in an order of their own, which need not be that of their results: join on (slot, game_seq).  A full ring is no capacity
 * error: overflow stays 0, and games, samples and results go on unchanged.
 * xq_engine_drain_games / _device: independent of xq_engine_drain, under its contract: they synchronise, return the first
 * min(games finished since the last drain of this ring, max_out_games) records in the order the games finished and reset this
 * ring only.  max_records smaller than what is pending: XQ_ERR_ARG, *n_records reports the pending count and nothing is
 * consumed.  A NULL buffer reports the count and consumes nothing.  XQ_ERR_ARG on an engine without the option.
 * xq_engine_game_records_stats_read: synchronises; recorded + dropped = the games finished.  XQ_ERR_ARG without the option.
 * THE REPLAY: xq_replay_games_batch, one wavefront per record, plays record i from the initial position for
 * min(max(stop_ply[i], 0), n_moves) plies (all n_moves without dev_stop_ply): at each ply the ordered legal moves of the
 * position are generated and the record's action must be one of them.
 *   dev_status[i]   0: every requested ply was legal; k > 0: ply k - 1 is no legal move of its position, the replay stopped
 *                   before it and every output describes the position before that ply; -1: n_moves > XQ_RECORD_MAX_PLIES, nothing
 *                   is replayed and the outputs describe the initial position.
 *   dev_boards[i], dev_side[i], dev_move_count[i], dev_no_capture[i]: the position reached.
 *   dev_hist12[i]   int8[12][90]: the last min(12, move_count) pre-move boards, oldest first, zeros elsewhere --
 *                   xq_engine_set_position's host_hist12.
 *   dev_over_kind[i], dev_winner[i]: the rules' verdict at the position reached, as an engine's root status has it: 0 not over
 *                   (winner 2), 1 over, 4 over by the perpetual-check rule (only with perpetual_check = 1); max_game_length is
 *                   no rule and is not judged.
 * Every output pointer but dev_status may be NULL.  n = 0 is a no-op; XQ_ERR_ARG before any launch: n < 0, with n > 0 a NULL
 * dev_records or dev_status, perpetual_check outside {0, 1}. */
#define XQ_RECORD_MAX_PLIES 504
#define XQ_RECORD_BYTES 1024
typedef struct xq_game_record {
    uint32_t slot, game_seq;     /* join key with xq_game_result and xq_sample */
    int8_t   winner;             /* as xq_game_result */
    uint8_t  reason;             /* as xq_game_result */
    uint16_t n_moves;            /* == the result's steps (game.move_count) */
    uint16_t opening_plies;      /* leading plies no search chose: the random opening (self-play) or the paired arena opening */
    uint16_t n_samples;          /* as xq_game_result */
    uint16_t moves[XQ_RECORD_MAX_PLIES];   /* action codes in ply order; entries at and after n_moves are 0 */
} xq_game_record;
typedef struct xq_game_records_opts { int32_t enabled; int32_t max_out_games; int32_t reserved[2]; } xq_game_records_opts;
typedef struct xq_game_records_stats { uint64_t recorded, dropped, reserved[2]; } xq_game_records_stats;
size_t xq_engine_workspace_bytes_gr(const xq_engine_config *cfg, int leaves_per_step, unsigned flags, const xq_playout_cap *cap,
                                    const xq_forced_playouts *forced, const xq_gumbel *gumbel, const xq_arena_opts *arena,
                                    const xq_rules_opts *rules, const xq_solver_opts *solver, const xq_root_stats_opts *root_stats,
                                    const xq_eval_mirror_opts *mirror, const xq_game_records_opts *records);
int xq_engine_init_gr(xq_engine *eng, const xq_engine_config *cfg, int leaves_per_step, unsigned flags, const xq_playout_cap *cap,
                      const xq_forced_playouts *forced, const xq_gumbel *gumbel, const xq_arena_opts *arena,
                      const xq_rules_opts *rules, const xq_solver_opts *solver, const xq_root_stats_opts *root_stats,
                      const xq_eval_mirror_opts *mirror, const xq_game_records_opts *records, void *ws, size_t ws_bytes,
                      const uint64_t *dev_inject, void *stream);
int xq_engine_drain_games(const xq_engine *eng, void *host_records, int max_records, int *n_records, void *stream);
int xq_engine_drain_games_device(const xq_engine *eng, void *dev_records, int max_records, int *n_records, void *stream);
int xq_engine_game_records_stats_read(const xq_engine *eng, xq_game_records_stats *host_out, void *stream);
int xq_replay_games_batch(const void *dev_records /* xq_game_record[n] */, const int32_t *dev_stop_ply /* [n] or NULL = all moves */,
                          int n, int perpetual_check,
                          int8_t *dev_boards /* [n][90] */, int8_t *dev_side, int32_t *dev_move_count, int32_t *dev_no_capture,
                          int8_t *dev_hist12 /* [n][12][90], oldest first, xq_engine_set_position's layout */,
                          int32_t *dev_status, int8_t *dev_over_kind, int8_t *dev_winner, void *stream);

/* A fixed alpha-beta opponent (nothing in the engine knows of it, and no existing entry point, struct or byte changes): a batched
 * fixed-depth minimax search over the material evaluation, one wavefront per (position, root move).  A non-learning yardstick for
 * a training run (baseline.py plays a network against it), and a per-move tactical score for any batch of positions.
 * ROOT MOVES.  dev_moves[i][0..dev_counts[i]) are the ordered legal moves of the side to move: xq_movegen_batch's output exactly.
 * SCORE OF ROOT MOVE j.  dev_scores[i][j] = -V(child_j, depth - 1, 1).  V(pos, d, ply) is taken from the view of the side to move
 * in pos:
 *     d == 0:    V = material(side to move) - material(other), xq_material_batch's piece values; no moves are generated and there
 *                is no quiescence;
 *     otherwise  generate the ordered legal moves; none: V = -(XQ_AB_MATE - ply) (a side without a legal move has lost, and a
 *                quicker mate scores higher); else V = the maximum over the moves of -V(child, d - 1, ply + 1).
 * Repetition, the no-capture count and the ply-200 rule do not enter the search.
 * DEPTH 0.  Every root move scores 0 and nothing is searched: with draws the uniformly random player, without them the player of
 * the first legal move.  0 <= depth <= XQ_AB_MAX_DEPTH.
 * PRUNING.  Each root move is searched on its own under a full window; below it the search is fail-soft alpha-beta in move order,
 * and the level whose children are leaves scores all of them at once.  dev_scores[i][j] is exactly the plain minimax value of
 * every root move: the tie-break needs it and an analysis caller wants it.
 * PICK.  dev_best_score[i] is the largest score; B = the root moves that reach it, in move order; dev_best_action[i] =
 * B[dev_draws[i] % |B|], or B[0] when dev_draws is NULL.
 * EVERY OUTPUT IS WRITTEN.  At and past the count dev_scores[i][j] = XQ_AB_UNSCORED, dev_nodes[i][j] = 0, dev_moves[i][j] = 0.
 * dev_nodes[i][j] (or NULL) is the number of positions visited below root move j, the child itself included: between 1 and the
 * plain minimax count for depth >= 1, 0 at depth 0.
 * dev_status[i]: 0 fine; 1 a move-generation capacity was exceeded somewhere in the tree, by xq_movegen_batch's rule; 2 a king is
 * missing on the input board: no search is done, the count is 0, dev_best_action[i] = XQ_AB_NO_MOVE and dev_best_score[i] = 0.
 * A root without legal moves has count 0, dev_best_action[i] = XQ_AB_NO_MOVE and dev_best_score[i] = -XQ_AB_MATE.
 * XQ_ERR_ARG before any launch: n < 0, a depth outside the range, with n > 0 a NULL pointer other than dev_draws and dev_nodes.
 * n == 0 is a no-op that returns XQ_OK.  Three launches on `stream` (two at depth 0) per 2^18 positions, no atomics, no
 * workspace. */
#define XQ_AB_MAX_DEPTH 4
#define XQ_AB_MATE      30000
#define XQ_AB_UNSCORED  INT32_MIN
#define XQ_AB_NO_MOVE   0xFFFF
int xq_alphabeta_batch(const int8_t *dev_boards /* [n][90] */, const int8_t *dev_side /* [n] */, int n, int depth,
                       const uint32_t *dev_draws /* [n] or NULL */,
                       uint16_t *dev_moves /* [n][XQ_MAXM] */, uint16_t *dev_counts /* [n] */,
                       int32_t *dev_scores /* [n][XQ_MAXM] */, uint32_t *dev_nodes /* [n][XQ_MAXM] or NULL */,
                       uint16_t *dev_best_action /* [n] */, int32_t *dev_best_score /* [n] */,
                       uint8_t *dev_status /* [n] */, void *stream);

/* A forced-mate search (nothing in the engine knows of it, and no existing entry point, struct or byte changes): does the side to
 * move, the attacker, force mate within N of its own moves, by checks only (the classic puzzle, a mate forced by an unbroken
 * series of checks) or by any move?  A boolean AND/OR search in move order, one wavefront per (position, root move): the labels of
 * a tactics puzzle set (tactics.py), and a per-move mate distance for any batch of positions.
 * ROOT MOVES.  dev_moves[i][0..dev_counts[i]) are the ordered legal moves of the side to move: xq_movegen_batch's output exactly.
 * RESULT OF ROOT MOVE j with child c, N = opts->max_moves:
 *     if checks_only and the defender is not in check in c:  mate_in = 0, nodes = 0
 *     else for m = 1 .. N:  if D(c, m - 1): mate_in = m, stop                                    (none: mate_in = 0)
 *     D(pos, k)  the defender to move, k attacker moves left:  visit; no legal move -> true; k == 0 -> false;
 *                for each reply in move order: if not A(child, k) -> false;   -> true
 *     A(pos, k)  the attacker to move:  visit; for each move in move order: (checks_only: skip a move that gives no check)
 *                if D(child, k - 1) -> true;   -> false
 * A side without a legal move has lost, whether it is in check or not.  Repetition, the no-capture count and the ply-200 rule do
 * not enter the search.  dev_mate_in[i][j] in 1..N: root move j forces mate in that many attacker moves, itself included.
 * VISITS.  A visit is one move generation; dev_nodes[i][j] (or NULL) counts them over all m.  A move that fails the check test
 * costs no visit.
 * NODE LIMIT.  A search that would make visit number opts->node_limit + 1 stops with dev_mate_in[i][j] = XQ_MATE_UNKNOWN and
 * dev_nodes[i][j] = node_limit.
 * EXACT ORDER.  The traversal order above is part of the contract: visit counts and the limit's outcome are exact.  There is no
 * move reordering and no transposition table.
 * BEST.  dev_best_mate_in[i] is the smallest value in 1..N over the root moves, or 0 when there is none; dev_best_action[i] is the
 * first move in move order that reaches it, or XQ_MATE_NO_MOVE.
 * EVERY OUTPUT IS WRITTEN.  At and past the count dev_mate_in[i][j] = 0, dev_nodes[i][j] = 0, dev_moves[i][j] = 0.
 * dev_status[i]: 0 fine; 1 a move-generation capacity was exceeded somewhere in the tree, by xq_movegen_batch's rule; 2 a king is
 * missing on the input board: nothing is searched, the count is 0, the best mate-in is 0 and the action XQ_MATE_NO_MOVE; +4 some
 * root move ended XQ_MATE_UNKNOWN.  A root without legal moves has count 0, best 0 and XQ_MATE_NO_MOVE.
 * XQ_ERR_ARG before any launch: n < 0, NULL opts, max_moves outside 1..XQ_MATE_MAX_MOVES, checks_only outside {0, 1}, node_limit
 * == 0, reserved != 0, with n > 0 a NULL pointer other than dev_nodes.  n == 0 is a no-op that returns XQ_OK.  Three launches on
 * `stream` per 2^18 positions, no atomics, no workspace. */
#define XQ_MATE_MAX_MOVES 5
#define XQ_MATE_UNKNOWN   255
#define XQ_MATE_NO_MOVE   0xFFFF
typedef struct xq_mate_opts { int32_t max_moves;   /* N, 1..XQ_MATE_MAX_MOVES */
                              int32_t checks_only; /* 0 | 1 */
                              uint32_t node_limit; /* per root move, >= 1 */
                              uint32_t reserved;   /* 0 */ } xq_mate_opts;
int xq_mate_search_batch(const int8_t *dev_boards /* [n][90] */, const int8_t *dev_side /* [n] */, int n, const xq_mate_opts *opts,
                         uint16_t *dev_moves /* [n][XQ_MAXM] */, uint16_t *dev_counts /* [n] */,
                         uint8_t *dev_mate_in /* [n][XQ_MAXM] */, uint32_t *dev_nodes /* [n][XQ_MAXM] or NULL */,
                         uint16_t *dev_best_action /* [n] */, uint8_t *dev_best_mate_in /* [n] */, uint8_t *dev_status /* [n] */,
                         void *stream);

/* Scoring samples against a network, and policy-surprise weighted training (opt-in; nothing in the engine knows of it, and no
 * existing entry point, struct or byte changes).  A finished sample is turned back into an evaluation request, a network answers
 * it, and the answer is compared with the sample's search target: how well does network X predict the samples in buffer Y, and
 * which samples did the search change the most (KataGo's policy surprise)?  Self-play is played by one deterministic evaluator, so
 * running an iteration's samples through the same evaluator once reproduces the search's raw, noise-free root prior.
 * Both kernels run one wavefront per output row j, four rows per workgroup; row j is record dev_index[j] of dev_samples, or record
 * j itself when dev_index is NULL.  The engine writes n_moves <= XQ_MAXM; a larger byte is read as XQ_MAXM.
 *
 * xq_samples_to_requests: compact records -> the three inputs of the evaluator's legal-move protocol (xq_policy_head_legal):
 *     dev_planes[j]  float32[15][10][9], un-mirrored: the arithmetic of xq_samples_to_batch with flip = 0 (xq_encode_batch's planes)
 *     dev_moves[j]   uint16[XQ_MAXM]: moves[j][i] = actions[i] for i < n_moves, 0 behind that (all XQ_MAXM words are written)
 *     dev_counts[j]  int32: n_moves
 *   About 640 bytes read and 5.7 KB written per row: HBM-bound.  dev_planes must be 8-byte and dev_moves 4-byte aligned.
 *
 * xq_score_samples: per row, with m = n_moves, the record's visits c_i, the evaluator's legal-move logits l_i =
 * dev_legal_logits[j][i] (float32, i < m; entries at and behind m are never read) and T = late_temperature, in float64:
 *     TARGET  w_i = late_temp ? (c_i > 0 ? pow(c_i, 1 / T) : 0) : c_i;  total = w_0 + w_1 + ... in move order;  t_i = w_i / total
 *             -- w_i and total exactly as xq_samples_to_batch forms them; a Gumbel record's 16-bit improved policy (late_temp = 0)
 *             is normalised the same way.
 *     PRIOR   M = max_j l_j;  logp_i = l_i - M - log(sum_j exp(l_j - M))
 *     SCORES  policy_ce = -sum_{t_i > 0} t_i * logp_i
 *             policy_kl = max(0, sum_{t_i > 0} t_i * (log t_i - logp_i))
 *             value     = dev_value[j]
 *             top1      = (first index of the largest logit == first index of the largest visit count)
 *   policy_kl and policy_ce are cast to float32 once.  The sums over the moves are wave reductions: their order is not the move
 *   order, and they agree with a sequential float64 sum to about 1e-13.
 *   INVALID rows -- m = 0, total = 0, a total that is not finite (a late record's powers overflow for a small T), or a logit
 *   among the m that is not finite -- get valid = 0 and zeros in every other field, and nothing is written back.
 *   write_back = 1 also writes 8 bytes into the RECORD (dev_samples is then written to): xq_sample_policy_stats at byte
 *   XQ_SAMPLE_POLICY_STATS_OFFSET = 120, inside the 11 zero bytes of xq_sample_root_stats, whose own fields (root_q, root_visits,
 *   has_root_stats at byte 116) are not touched:
 *       policy_kl         float32 at 120   the score's policy_kl
 *       has_policy_stats  uint8   at 124   1
 *       prior_top1        uint8   at 125   the score's top1
 *       two zero bytes
 *   dev_scores may be NULL when write_back = 1.  Rows that name one record write the same bytes.
 *   XQ_ERR_ARG before any launch: opts NULL, a non-zero reserved word, write_back outside {0, 1}, late_temperature not positive
 *   and finite, n < 0, and with n > 0 a NULL dev_samples, dev_legal_logits or dev_value, or a NULL dev_scores with write_back = 0.
 *   n = 0 is a no-op (the options are still checked).
 *
 * xq_surprise_counts: how often each of the n_records records of dev_samples is drawn in one epoch, dev_counts int32[n_records].
 * A record without the mark (has_policy_stats != 1) counts 1.  Over the marked records the normaliser is integer, so that it does
 * not depend on the order of summation (atomics and any tree give the same):
 *     q_i = llrint(min(policy_kl_i, 64.0f) * 2^20) as uint64  (a policy_kl that is negative or NaN is taken as 0; the score kernel
 *           writes neither);  S = sum q_i;  M = the number of marked records
 *     S = 0: every count is 1.  Otherwise, in float64, uncontracted, in this order:
 *     w_i = (1 - alpha) + alpha * (((double)q_i * (double)M) / (double)S)
 *     u_i = (double)(philox_u64(seed, epoch, slot, 10, game_seq, ply) >> 11) * 2^-53
 *     c_i = floor(w_i) + (u_i < w_i - floor(w_i))
 *   so the counts of the marked records sum to M in expectation, alpha = 0 is the uniform epoch, and alpha = 1 draws in proportion
 *   to the KL.  philox_u64(key, rank, slot, kind, ctr, sub) is the engine's Philox4x32-10 (see the evaluation mirror above): the
 *   epoch takes the rank word, and kind 10 is used by no other draw (0-3, 7, 8 and 9 are taken).  The rounding decision is keyed by
 *   the record's identity (slot, game_seq, ply), not by its place in the buffer.  There is no cap on w_i beyond the 64 nats.
 *   dev_scratch: XQ_SURPRISE_SCRATCH_BYTES bytes of device memory, 8-byte aligned, zeroed and used by the call (S and M).
 *   XQ_ERR_ARG before any launch: opts NULL, alpha outside [0, 1] or NaN, a non-zero reserved word, n_records < 0, and with
 *   n_records > 0 a NULL pointer or a misaligned dev_scratch.  n_records = 0 is a no-op.
 * xq_surprise_count_host: c_i of one record on the host, by the device's own code, bit for bit; -1 for alpha outside [0, 1]. */
typedef struct xq_score_opts { double late_temperature; int32_t write_back; int32_t reserved; } xq_score_opts;
typedef struct xq_sample_score {
    float policy_kl, policy_ce, value;
    uint8_t top1, valid;
    uint8_t zero[2];
} xq_sample_score;
#define XQ_SAMPLE_POLICY_STATS_OFFSET 120
typedef struct xq_sample_policy_stats {
    float policy_kl;
    uint8_t has_policy_stats;
    uint8_t prior_top1;
    uint8_t zero[2];
} xq_sample_policy_stats;
typedef struct xq_surprise_opts { double alpha; uint64_t seed; uint32_t epoch; uint32_t reserved; } xq_surprise_opts;
#define XQ_SURPRISE_SCRATCH_BYTES 16
#define XQ_RNG_KIND_SURPRISE 10
int xq_samples_to_requests(const void *dev_samples, const int32_t *dev_index /* int32[n] or NULL = 0..n-1 */, int n,
                           float *dev_planes /* [n][15][90] */, uint16_t *dev_moves /* [n][XQ_MAXM] */,
                           int32_t *dev_counts /* [n] */, void *stream);
int xq_score_samples(void *dev_samples, const int32_t *dev_index /* int32[n] or NULL = 0..n-1 */, int n,
                     const float *dev_legal_logits /* [n][XQ_MAXM] */, const float *dev_value /* [n] */,
                     const xq_score_opts *opts, xq_sample_score *dev_scores /* [n], or NULL with write_back = 1 */, void *stream);
int xq_surprise_counts(const void *dev_samples, int n_records, const xq_surprise_opts *opts, int32_t *dev_counts /* [n_records] */,
                       void *dev_scratch, void *stream);
int xq_surprise_count_host(float policy_kl, int marked, uint64_t M, uint64_t S, double alpha, uint64_t seed, uint32_t epoch,
                           uint32_t slot, uint32_t game_seq, uint32_t ply);

/* Merging the records of one position into one training sample (opt-in; nothing in the engine knows of it, no record is
 * rewritten, and no existing entry point, struct or byte changes).  The network's input is the board and the side to move, so two
 * records with the same board and side are one training input; a buffer of self-play games holds the opening positions many
 * times over, with contradictory z.  The merged form lives in index arrays only: keys per record (xq_position_keys), a stable
 * sort by key (the caller's), group heads in the sorted order (xq_position_group_heads), and a batch kernel that reads groups of
 * records instead of records (xq_groups_to_batch).
 *
 * MIRROR      mir(sq) = (sq / 9) * 9 + 8 - sq % 9; on an action both squares are mirrored (xq_samples_to_batch's arithmetic).
 * CANONICAL ORIENTATION, with flag XQ_POSITION_KEY_MIRROR (= 1): let sq* be the smallest square with board[sq*] != board[mir(sq*)].
 *             No such square (the board is its own mirror image): mirrored = 0 and the canonical board c = board.  Otherwise
 *             mirrored = (board[mir(sq*)] < board[sq*]), compared as int8, and c[sq] = board[mir(sq)] when mirrored is set,
 *             c = board otherwise.  Without the flag mirrored = 0 and c = board.  A position and its mirror image share one c.
 * KEY         all arithmetic uint64 with wrap-around:
 *             mix(x):      x ^= x >> 30; x *= 0xBF58476D1CE4E5B9; x ^= x >> 27; x *= 0x94D049BB133111EB; x ^= x >> 31
 *             term(i, b) = mix(0x9E3779B97F4A7C15 * (uint64)(i * 256 + (uint8)b + 1))
 *             key        = XOR over sq < 90 of term(sq, c[sq]), then ^ term(90, side)
 *             XOR is order-free: the wave reduction, the host twin and a numpy loop agree bit for bit.
 * GROUPS      rows are taken in the caller's order (oldest first), sorted STABLY by key; order[j] is the row at sorted place j.
 *             Row order[j] starts a group iff j == 0, or its key, its side or its canonical board (90 bytes) differs from that
 *             of row order[j-1].  The full compare makes a wrong merge impossible; two positions with one key can at worst split
 *             a group (A, B, A gives three groups).  Members of a group are in the caller's order.
 * MERGED SAMPLE of group g with members k = 0 .. n-1 (record indices members[offsets[g] + k]), output flip f and member
 *             orientation o_k = member_mirrored_k XOR f:
 *             planes  those of member 0 under o_0 (xq_samples_to_batch's planes with flip = o_0)
 *             t_k[a]  exactly what xq_samples_to_batch writes into pi for member k with flip = o_k, in float64 before its cast
 *                     (w_i / total_k at the member's actions, 0 elsewhere); total_k its sequential sum in move order; member k
 *                     is VALID iff total_k > 0; n_pi = the number of valid members
 *             pi[a] = (float)((0.0 + t_0[a] + t_1[a] + ...) / (double)n_pi) over the valid members in member order, float64,
 *                     no fused multiply-add; all zeros when n_pi = 0
 *             z     = (float)((0.0 + zt_0 + zt_1 + ...) / (double)n) with zt_k the float64 value xq_samples_to_batch_ex forms
 *                     before its cast: (double)z, or (1 - q_mix) z + q_mix root_q for a member carrying root statistics
 *             The definition is dense: members may name different actions.  No floating-point atomics are used.  A group of one
 *             gives xq_samples_to_batch_ex's three outputs for that record with flip = o_0, byte for byte.  A record names an
 *             action at most once; n_moves above XQ_MAXM is read as XQ_MAXM and an action id >= 8100 is skipped.
 *
 * xq_position_keys: dev_keys[j] and dev_mirrored[j] of row j = record dev_index[j] of dev_samples, or record j when dev_index is
 *   NULL.  One wavefront per row, four rows per workgroup; sq* comes from a ballot over the 90 squares.
 * xq_position_key_host: the same code on the host, bit for bit; needs no GPU.  *mirrored may be NULL.  A NULL board or flags
 *   other than 0 or 1 give key 0 and mirrored 0.
 * xq_position_group_heads: dev_head[j] = 1 iff row dev_order[j] starts a group (the rule above), else 0, for j < n.  dev_keys and
 *   dev_mirrored are indexed by row and taken as given.  An entry of dev_order outside [0, n) makes places j and j + 1 heads and
 *   is read nowhere.
 * xq_groups_to_batch: output row j is group dev_group[j] under flip dev_flip[j]: dev_states[j] float32[15][10][9], dev_pi[j]
 *   float32[8100], dev_z[j] float32, as defined above.  dev_group_offsets int32[n_groups + 1], dev_members int32[] record indices
 *   into dev_samples, dev_member_mirrored uint8[] parallel to dev_members.  A row whose group id is outside [0, n_groups), or
 *   whose group is empty, gets zero planes, zero pi and z = 0, and no record is read for it.  One 256-thread workgroup per row; a
 *   group of one takes xq_samples_to_batch's path (zero fill and scatter), a larger one adds its members one after the other
 *   into a float64 accumulator of 8100 entries in LDS (64 800 bytes) and writes the row from there as float4.
 * XQ_ERR_ARG before any launch (no GPU needed): n < 0 or n_groups < 0; flags other than 0 or 1; with n > 0 a NULL pointer where
 *   one is required (dev_index may always be NULL; with n_groups = 0 the record and group arrays may be); late_temperature not
 *   positive, q_mix outside [0, 1] or NaN, a non-zero reserved word (opts may be NULL: q_mix = 0); dev_keys not 8-byte aligned;
 *   dev_pi not 16-byte aligned.  n = 0 is a no-op. */
#define XQ_POSITION_KEY_MIRROR 1
int xq_position_keys(const void *dev_samples, const int32_t *dev_index /* int32[n] or NULL = 0..n-1 */, int n, int flags,
                     uint64_t *dev_keys /* [n] */, uint8_t *dev_mirrored /* [n] */, void *stream);
uint64_t xq_position_key_host(const int8_t *board /* [90] */, int8_t side, int flags, uint8_t *mirrored);
int xq_position_group_heads(const void *dev_samples, const int32_t *dev_index /* int32[n] or NULL */,
                            const int32_t *dev_order /* int32[n]: rows in sorted order */, const uint64_t *dev_keys /* [n] */,
                            const uint8_t *dev_mirrored /* [n] */, int n, uint8_t *dev_head /* [n] */, void *stream);
int xq_groups_to_batch(const void *dev_samples, const int32_t *dev_group_offsets /* int32[n_groups + 1] */,
                       const int32_t *dev_members /* int32[]: record indices */,
                       const uint8_t *dev_member_mirrored /* uint8[], parallel to members */, int n_groups,
                       const int32_t *dev_group /* int32[n] */, const uint8_t *dev_flip /* uint8[n] */, int n,
                       double late_temperature, const xq_batch_opts *opts, float *dev_states, float *dev_pi, float *dev_z,
                       void *stream);

/* Game records as training samples (opt-in; nothing in the engine knows of it, and no existing entry point, struct or byte
 * changes): a supervised warm start from recorded games.  A record (xq_game_record) holds every move of a game, whoever chose it;
 * these two calls turn the plies a caller selects into ordinary xq_sample rows, which the batch kernels read as one-hot policy
 * targets.
 * SELECTION   ply p of record i is selected when lo_i <= p < n_moves_i, with lo_i = skip_opening ? opening_plies_i : 0; the mover
 *             of p is in the record's mover set (red moves the even plies): the set is dev_movers[i] when that pointer is given,
 *             else opts->movers: 0 every ply, 1 the winner's plies only (a drawn game selects none), 2 red's plies, 3 black's;
 *             and the record is not dropped by skip_draws (winner 0 selects no ply).
 * MALFORMED   n_moves > XQ_RECORD_MAX_PLIES, opening_plies > n_moves, winner outside {-1, 0, 1}, or a dev_movers entry outside
 *             [0, 3]: the record selects nothing (count 0) and its status is -1.  Both calls apply the same rule.
 * xq_records_sample_counts: dev_counts[i] = the number of selected plies of record i.  Arithmetic over the headers, one thread per
 *             record, no replay: an illegal ply does not change a count.
 * PLACEMENT   the caller forms the exclusive prefix sum of the counts (dev_offsets int32[n + 1], the dev_group_offsets style of
 *             xq_groups_to_batch): the rows of record i are exactly [dev_offsets[i], dev_offsets[i + 1]), in ply order.  No atomics;
 *             the same bytes on every run.  xq_records_to_samples recomputes the count: when dev_offsets[i + 1] - dev_offsets[i]
 *             differs from it, or the range leaves [0, dev_offsets[n]], nothing is written for the record and its status is -2
 *             (-1 goes first on a malformed record).
 * xq_records_to_samples: one wavefront per record, four per workgroup.  The record is played from the initial position as
 *             xq_replay_games_batch plays it (no repetition, no-capture or length rule is judged: the record's winner is trusted);
 *             at every ply the ordered legal moves are generated and the record's action is looked up among them.  A selected ply
 *             writes one xq_sample, all 640 bytes: board, side and ply (the move count) before the move; z = 0 for winner 0, else
 *             +1 when the winner is the side to move, else -1; n_moves and actions[0 .. n_moves) = the ordered legal moves
 *             (xq_movegen_batch's output for the position); visits = 1 at the move played, 0 elsewhere; late_temp, reserved0 and
 *             reserved1 = 0; slot and game_seq the record's; pad and the tails of actions and visits zero.  Rows are written with
 *             16-byte vector stores.
 *   dev_status[i]   0: the record was written whole; k > 0: ply k - 1 is no legal move of its position: the rows of selected
 *                   plies before it are complete, those of selected plies from it on are 640 zero bytes; -1 malformed; -2 the
 *                   offsets do not fit the record.  A well-formed record that selects nothing is still replayed for its status.
 * XQ_ERR_ARG before any launch (no GPU needed): n < 0; opts NULL, movers outside [0, 3], a flag outside {0, 1}, a non-zero reserved
 * word; with n > 0 a NULL pointer other than dev_movers; dev_samples not 16-byte aligned.  n = 0 is a no-op. */
typedef struct xq_supervise_opts {
    int32_t movers;        /* 0 every ply, 1 the winner's plies only (a drawn game selects none), 2 red's plies, 3 black's plies */
    int32_t skip_opening;  /* 1: plies < record.opening_plies are replayed but select no sample */
    int32_t skip_draws;    /* 1: a record with winner 0 selects no ply */
    int32_t reserved;
} xq_supervise_opts;
int xq_records_sample_counts(const void *dev_records /* xq_game_record[n] */, const uint8_t *dev_movers /* [n] or NULL */, int n,
                             const xq_supervise_opts *opts, int32_t *dev_counts /* [n] */, void *stream);
int xq_records_to_samples(const void *dev_records /* xq_game_record[n] */, const uint8_t *dev_movers /* [n] or NULL */,
                          const int32_t *dev_offsets /* [n + 1] */, int n, const xq_supervise_opts *opts,
                          void *dev_samples /* xq_sample[dev_offsets[n]] */, int32_t *dev_status /* [n] */, void *stream);

/* Endgame tablebases (nothing in the engine knows of them, and no existing entry point, struct or byte changes): the exact value
 * of every position with both kings and up to XQ_TB_MAX_PIECES further pieces, by retrograde analysis over a dense index.
 * SIGNATURE   P <= XQ_TB_MAX_PIECES non-king pieces as signed codes (2 advisor, 3 elephant, 4 knight, 5 rook, 6 cannon, 7 pawn;
 *             red positive), in the caller's order.  Both kings are implicit.
 * INDEX       dense, mixed radix, most significant digit first: the side to move (0 red, 1 black); the red king (9 palace squares,
 *             rows 0-2, columns 3-5, row-major); the black king (9 squares, rows 7-9); then one digit per piece in signature order.
 *             A piece's digits are its admissible squares in row-major order of the actual square, followed by one extra digit
 *             meaning "captured".  Admissible for red: advisor (0,3) (0,5) (1,4) (2,3) (2,5); elephant (0,2) (0,6) (2,0) (2,4) (2,8)
 *             (4,2) (4,6); pawn rows 3-4 on columns 0, 2, 4, 6, 8 and every square of rows 5-9 (55); knight, rook and cannon all 90.
 *             For black the sets are the 180-degree rotation of red's (square s becomes 89 - s).  The captured digit makes every
 *             sub-ending part of the same table: a capture is an index transition, there is no chain of tables.  Two equal pieces
 *             are two digits; no symmetry is reduced.
 *             xq_tb_entries: the entry count, on the host (no GPU needed); 0 for a bad signature (a code outside 2..7, P outside
 *             0..XQ_TB_MAX_PIECES, NULL pieces with P > 0) or one beyond XQ_TB_MAX_ENTRIES.
 * RULES       the move generator alone (xq_movegen_batch's moves).  The side to move without a legal move has lost, mated or
 *             stalemated, as in the engine.  No repetition rule, no 120-ply no-capture rule, no ply-200 rule.
 * VALUE       one int16 per entry, from the view of the side to move: 0 a draw; +p (p odd, >= 1) a win: with best play the loser
 *             is without a move p plies from now; -(p + 1) (p even, >= 0) a loss in p plies, -1 no legal move now; XQ_TB_INVALID
 *             an entry that is no position: two men on one square, or the side not to move in check, which includes facing kings.
 *             Every legal move from a valid entry leads to a valid entry, so a king is never captured.
 * xq_tb_init  pass 0, one wavefront per entry: the index is decoded into a board; XQ_TB_INVALID, -1 or 0 is written.
 * xq_tb_pass  pass k in 1..XQ_TB_MAX_PASSES, in place on the one table, one wavefront per entry.  A wavefront whose entry is not 0
 *             exits after one load.  Otherwise it generates the moves; every lane computes the child index of its move from the
 *             parent's digits (the mover's digit changes, a captured piece's digit becomes "captured", the side flips) and loads
 *             the child's value.  Odd k: the entry becomes +k when some child equals -k.  Even k: the entry becomes -(k + 1) when
 *             every child is positive and the largest is k - 1.  A wavefront that decides an entry stores 1 into *dev_changed (a
 *             plain store; the caller zeroes the word before the pass and reads it after).  The caller runs k = 1, 2, ... and stops
 *             at the first pass that decided nothing.
 *             IN PLACE IS EXACT.  Pass k writes only values of distance k (+k for odd k, -(k + 1) for even k) and only over a 0,
 *             and it tests children only for distance k - 1 (-k written by pass k - 1 for odd k; a largest child of k - 1 for even
 *             k).  A value written earlier in the same pass is +k or -(k + 1): it is never -k, and in an even pass it is negative,
 *             which fails "every child is positive" exactly as the 0 it replaced did.  So a test gives the same answer whether it
 *             sees a child's word from before this pass or from within it.  An aligned 2-byte load or store is atomic, so a word
 *             is never seen half written.  Values of distance k - 1 and below never change again.
 *             Neither call synchronises or allocates.  Launches go over chunks so that no grid passes 2^31 threads.
 * xq_tb_probe_batch   one wavefront per position.  The board is matched against the signature greedily in signature order (the r-th
 *             piece of a code in the signature takes the r-th such piece of the board, row-major); a signature piece absent from
 *             the board is "captured".  dev_value[i] is the entry's value; dev_moves / dev_counts the ordered legal moves;
 *             dev_move_value[i][j] (or NULL) what the side to move gets by playing root move j: a child lost in p plies gives
 *             +(p + 1), a child won in p plies gives -(p + 2), a drawn child 0.  dev_best_action[i] is the first move in move order
 *             whose move value equals dev_value[i], XQ_TB_NO_MOVE when there is no move.
 *   dev_status[i]   a bit set: +1 the position is not in this table (a piece the signature lacks, or a piece on a square outside its
 *                   list); +2 a king is missing; +4 the entry is XQ_TB_INVALID.  With any bit set the value is 0, the count 0 and
 *                   the action XQ_TB_NO_MOVE.  Every output word is written; past the count moves and move values are zeros.
 * XQ_ERR_ARG before any launch: n < 0; NULL pointers where n > 0 (dev_move_value may be NULL), a NULL table or flag; a bad
 * signature; k outside 1..XQ_TB_MAX_PASSES.  An empty batch is a no-op returning 0. */
#define XQ_TB_MAX_PIECES  5
#define XQ_TB_MAX_ENTRIES (1 << 28)
#define XQ_TB_MAX_PASSES  32000
#define XQ_TB_INVALID     (-32768)
#define XQ_TB_NO_MOVE     0xFFFF
int64_t xq_tb_entries(const int8_t *pieces /* [n_pieces] */, int n_pieces);
int xq_tb_init(const int8_t *pieces, int n_pieces, int16_t *dev_table /* [entries] */, void *stream);
int xq_tb_pass(const int8_t *pieces, int n_pieces, int16_t *dev_table /* [entries] */, int k, int32_t *dev_changed /* [1] */,
               void *stream);
int xq_tb_probe_batch(const int8_t *pieces, int n_pieces, const int16_t *dev_table /* [entries] */,
                      const int8_t *dev_boards /* [n][90] */, const int8_t *dev_side /* [n] */, int n, int16_t *dev_value /* [n] */,
                      uint16_t *dev_moves /* [n][XQ_MAXM] */, uint16_t *dev_counts /* [n] */,
                      int16_t *dev_move_value /* [n][XQ_MAXM] or NULL */, uint16_t *dev_best_action /* [n] */,
                      uint8_t *dev_status /* [n] */, void *stream);

/* The table as opponent and as teacher (opt-in; xq_tb_init, xq_tb_pass and xq_tb_probe_batch are what they were, byte for byte).
 * Both calls run one wavefront per item, four per workgroup, LDS carved per wave, no atomics, no scratch, no workgroup barrier;
 * neither synchronises or allocates, and launches go over chunks as the probe's do.
 * xq_tb_play_batch   one move per position.  The board is matched against the signature exactly as xq_tb_probe_batch matches it,
 *             and status bits 1, 2 and 4 have the probe's meaning.  dev_action[i] is the move to play, or XQ_TB_NO_MOVE: the table
 *             chooses the probe's best_action, the first move in move order whose move value equals the position's value (the
 *             quickest win, a draw-holding move, or the longest defence).  dev_action == NULL: the table chooses everywhere.
 *   dev_status[i]   the probe's bits, and +8 the position has no legal move; +16 the given action is not among the position's
 *                   ordered legal moves.
 *             With status 0: dev_boards_out[i] = the board after the move (`to` takes the man of `from`, `from` becomes empty),
 *             dev_side_out[i] = -side, dev_played[i] = the action, dev_value[i] = the entry's value before the move,
 *             dev_move_value[i] = what the mover gets by it (the probe's convention), dev_value_out[i] = the child entry's table
 *             word, from the new side's view.  With any bit set: dev_boards_out[i] and dev_side_out[i] copy the input, dev_played[i]
 *             = XQ_TB_NO_MOVE, dev_move_value[i] = dev_value_out[i] = 0, and dev_value[i] is the entry's value when only bits 8 or
 *             16 are set, else 0.  Every output word is written for every item.
 *   ALIASING  dev_boards_out may be dev_boards and dev_side_out may be dev_side (the same pointers, for a walk in place): a
 *             wavefront reads its item's board and side into LDS and registers before it writes them, and touches no other item's.
 * xq_tb_samples   table entries as xq_sample rows.  Row i is entry dev_index[i], decoded as xq_tb_pass decodes it; all 640 bytes
 *             are written, with 16-byte vector stores as xq_records_to_samples writes its rows: board and side the entry's; z the
 *             sign of the entry's value; n_moves and actions[0 .. n_moves) the ordered legal moves; visits[j] = 1 where move j's
 *             value equals the entry's value (policy 1: only at the first such j), else 0; ply, late_temp, reserved0, reserved1
 *             and slot = 0; game_seq = the entry index (a unique identity for the Philox-keyed draws over samples); pad and the
 *             tails of actions and visits zero.
 *   dev_status[i]   0 written; 1 the index is outside [0, entries); 4 the entry is XQ_TB_INVALID; 8 the entry has no legal move,
 *                   so there is no policy target.  With a non-zero status the row is 640 zero bytes, the zero-row convention of
 *                   xq_records_to_samples.
 * XQ_ERR_ARG before any launch (no GPU needed): n < 0; a bad signature; with n > 0 a NULL pointer (dev_action may be NULL);
 * xq_tb_samples: opts NULL, policy outside {0, 1}, a non-zero reserved word, dev_samples not 16-byte aligned.  n = 0 is a no-op
 * returning 0. */
typedef struct xq_tb_sample_opts {
    int32_t policy;        /* 0: every optimal move is a policy target; 1: the first one in move order */
    int32_t reserved[3];
} xq_tb_sample_opts;
int xq_tb_play_batch(const int8_t *pieces, int n_pieces, const int16_t *dev_table /* [entries] */,
                     const int8_t *dev_boards /* [n][90] */, const int8_t *dev_side /* [n] */,
                     const uint16_t *dev_action /* [n] or NULL; XQ_TB_NO_MOVE: the table chooses */, int n,
                     int8_t *dev_boards_out /* [n][90], may alias dev_boards */, int8_t *dev_side_out /* [n], may alias dev_side */,
                     uint16_t *dev_played /* [n] */, int16_t *dev_value /* [n] */, int16_t *dev_move_value /* [n] */,
                     int16_t *dev_value_out /* [n] */, uint8_t *dev_status /* [n] */, void *stream);
int xq_tb_samples(const int8_t *pieces, int n_pieces, const int16_t *dev_table /* [entries] */, const int32_t *dev_index /* [n] */,
                  int n, const xq_tb_sample_opts *opts, void *dev_samples /* xq_sample[n], 16-byte aligned */,
                  uint8_t *dev_status /* [n] */, void *stream);

/* Start-position pool (opt-in, xq_engine_init_sp): self-play games from given positions, and the check that says whether a board
 * is a position the rules code can safely run on.
 * THE CHECK: xq_positions_check_batch, one wavefront per position, the board in LDS, no atomics, no scratch.  dev_status[i] is a
 * set of bits:
 *    1  a square outside -7..7, or a side outside {1, -1}
 *    2  a colour without exactly one king, or a king outside its palace (red rows 0-2, black rows 7-9, columns 3-5)
 *    4  a piece on a square it can never stand on, or more of a kind than a set has: advisor and elephant on their own points
 *       only; a red pawn never on rows 0-2 and on rows 3-4 only on columns 0, 2, 4, 6, 8, black mirrored; at most 2 of advisor,
 *       elephant, knight, rook, cannon and 5 pawns per colour
 *    8  the side not to move is in check (facing kings included)
 *   16  the side to move has no legal move
 * With bit 1 or 2 set the later bits are not evaluated and stay 0: the rules code is not run on such a board.  Bits 1, 2, 4 and 8
 * are fatal (XQ_POSITION_FATAL); bit 16 (XQ_POSITION_NO_MOVE) is information: such a game is over at ply 0.  n == 0 is a no-op;
 * XQ_ERR_ARG before any launch for n < 0, or for a NULL pointer with n > 0.
 * THE ENGINE: xq_engine_workspace_bytes_sp / xq_engine_init_sp are the widest pair: everything the _gr pair takes, then the pool.
 * NULL or n == 0 is exactly the _gr pair: the same workspace size, the same bytes, the same launches.  XQ_ERR_ARG before any
 * launch (xq_engine_workspace_bytes_sp: 0): n < 0 or n > XQ_START_POOL_MAX; reserved != 0; and, with n > 0, prob not in (0, 1]
 * (a NaN included), a NULL array, manual_moves != 0 (search-only and arena engines), game records enabled (a record has no room
 * for a start position and its replay starts from the initial one); and whatever xq_engine_init_gr refuses.  It goes with every
 * other option: leaf batching, tree reuse, the playout cap, forced playouts, Gumbel root search, the solver, root statistics, the
 * perpetual-check rule, the evaluation cache, the evaluation mirror and graph capture.
 * Init runs the check over the pool and returns XQ_ERR_ARG when an entry has a fatal bit: no unchecked board reaches a slot.  It
 * then copies the pool into the workspace; the caller's arrays need not outlive the call.  Workspace: behind the engine's
 * square-root table (THE OPTION WORDS below: the region's tail), the pool as 96-byte rows (the board, its side in byte 90),
 * int32 start_index[G] (the entry the slot's current game started from, -1 for the initial position) and 256 bytes holding n,
 * prob and the counter; "start-position pool on" lives in the handle (pad0, bit 22).  The handle's layout and size do not change.
 * THE DRAW for the game of a slot that will carry game_seq (the slot's previous game_seq + 1) is stateless:
 *           x0 = philox_u64(seed, rank, slot, 11, game_seq, 0),   x1 = philox_u64(seed, rank, slot, 11, game_seq, 1)
 * (the engine's Philox4x32-10, see the evaluation mirror above); the game starts from the pool iff (x0 >> 11) * 2^-53 < prob, at
 * entry x1 % n.  An engine with injected draws draws the same way: the pool draw is never injected.  xq_start_pool_draw_host runs
 * the same code on the host and returns the entry, or -1 for the initial position (also for n < 1 or a prob outside (0, 1]).
 * A game is started by xq_engine_select, in a kernel of its own ahead of the select kernel (one more launch per step, on a pool
 * engine only), one wavefront per slot: a slot whose game is finished has it flushed (samples with z, result, counters, exactly as
 * the select kernel does), then the draw is made.  Not from the pool: the select kernel that follows starts the game as ever
 * (quota, random opening, its draws).  From the pool: the game takes its ticket of games_target (none left: the slot idles),
 * game_seq + 1, no samples, the entry's board and side, move_count 0, no_capture 0, an empty history -- no random opening and no
 * draw of the opening's streams -- and the select kernel issues its root request.  An entry without a legal move therefore
 * finishes at ply 0 with no sample.  max_game_length, temperature_threshold and the rules' own limits count from the pool position.
 * xq_engine_start_indices: the device address of start_index.  xq_engine_start_pool_stats_read: synchronises; pool_games counts
 * the games started from the pool.  Both return XQ_ERR_ARG on an engine without the option. */
#define XQ_POSITION_FATAL 15
#define XQ_POSITION_NO_MOVE 16
#define XQ_START_POOL_MAX (1 << 20)
#define XQ_RNG_KIND_START_POOL 11
typedef struct xq_start_pool {
    const int8_t *dev_boards;    /* [n][90] */
    const int8_t *dev_side;      /* [n] */
    int32_t n;
    int32_t reserved;
    double prob;                 /* a new game starts from the pool with this probability, (0, 1] */
} xq_start_pool;
typedef struct xq_start_pool_stats { uint64_t pool_games, reserved[3]; } xq_start_pool_stats;
int xq_positions_check_batch(const int8_t *dev_boards /* [n][90] */, const int8_t *dev_side /* [n] */, int n,
                             uint8_t *dev_status /* [n] */, void *stream);
size_t xq_engine_workspace_bytes_sp(const xq_engine_config *cfg, int leaves_per_step, unsigned flags, const xq_playout_cap *cap,
                                    const xq_forced_playouts *forced, const xq_gumbel *gumbel, const xq_arena_opts *arena,
                                    const xq_rules_opts *rules, const xq_solver_opts *solver, const xq_root_stats_opts *root_stats,
                                    const xq_eval_mirror_opts *mirror, const xq_game_records_opts *records,
                                    const xq_start_pool *pool);
int xq_engine_init_sp(xq_engine *eng, const xq_engine_config *cfg, int leaves_per_step, unsigned flags, const xq_playout_cap *cap,
                      const xq_forced_playouts *forced, const xq_gumbel *gumbel, const xq_arena_opts *arena,
                      const xq_rules_opts *rules, const xq_solver_opts *solver, const xq_root_stats_opts *root_stats,
                      const xq_eval_mirror_opts *mirror, const xq_game_records_opts *records, const xq_start_pool *pool, void *ws,
                      size_t ws_bytes, const uint64_t *dev_inject, void *stream);
int xq_start_pool_draw_host(uint64_t seed, int rank, int slot, uint32_t game_seq, int n, double prob);
int xq_engine_start_indices(const xq_engine *eng, const int32_t **dev_index /* [n_games] */);
int xq_engine_start_pool_stats_read(const xq_engine *eng, xq_start_pool_stats *host_out, void *stream);

/* THE OPTION WORDS: where every option keeps its device words.  The handle is full, so Gumbel root search, arena options, the
 * solver, game records and the start-position pool all keep theirs in one workspace region, the square-root table's; this is its
 * map (csrc/xq_engine_state.cuh holds the functions every reader uses).  Offsets are bytes from the region's first byte, up()
 * rounds up to 256; G = n_games, S = num_simulations, K = leaves_per_step.
 *   the front, located from the region's first byte
 *     0                  table      double[S + 2 + (K > 1 ? K : 0)]
 *     (S + 2) * 8        gz_head 16 bytes (m, c_visit and c_scale as float32) | gz_vhat double[G] | gz_visits uint16[m][S]
 *     up((S + 2) * 8)    ar_head 16 bytes (opening_plies, first_game) | ar_op_counts int32[G] |
 *                        ar_op_actions uint16[G][XQ_ARENA_MAX_OPENING] | ar_n_live int32[2] | two sets (0 the new model's slots, 1
 *                        the old model's) of ar_rows int32[G] | ar_x float[G][1350] | ar_moves uint16[G][128] | ar_counts int32[G],
 *                        every part up()
 *     up((S + 2) * 8), or the end of the arena words
 *                        solver     uint64[G][8]
 *   the tail, located from the region's end; it starts at up(the front's end), every part up()
 *     game records       gr_ring xq_game_record[max_out_games] | gr_log uint16[G][XQ_RECORD_MAX_PLIES] | gr_opening uint16[G] |
 *                        gr_head 256 bytes
 *     start pool         sp_rows int8[n][96] | sp_index int32[G] | sp_head 256 bytes
 * xq_engine_option_words_sp takes what xq_engine_workspace_bytes_sp takes and fills the map for that engine: offset and size of
 * every block it has (a block it has not: 0, 0) and the region's size.  It needs no GPU and launches nothing.  XQ_ERR_ARG where
 * xq_engine_workspace_bytes_sp returns 0, and for out == NULL. */
typedef struct xq_words_block { uint64_t offset, bytes; } xq_words_block;
typedef struct xq_option_words {
    uint64_t bytes;              /* the region's */
    xq_words_block table;
    xq_words_block gz_head, gz_vhat, gz_visits;
    xq_words_block ar_head, ar_op_counts, ar_op_actions, ar_n_live, ar_rows[2], ar_x[2], ar_moves[2], ar_counts[2];
    xq_words_block solver;
    xq_words_block gr_ring, gr_log, gr_opening, gr_head;
    xq_words_block sp_rows, sp_index, sp_head;
} xq_option_words;
int xq_engine_option_words_sp(const xq_engine_config *cfg, int leaves_per_step, unsigned flags, const xq_playout_cap *cap,
                              const xq_forced_playouts *forced, const xq_gumbel *gumbel, const xq_arena_opts *arena,
                              const xq_rules_opts *rules, const xq_solver_opts *solver, const xq_root_stats_opts *root_stats,
                              const xq_eval_mirror_opts *mirror, const xq_game_records_opts *records, const xq_start_pool *pool,
                              xq_option_words *out);

/* Settled-move cutoff (opt-in): end a search whose first choice is fixed.  A move played at temperature 0 -- every arena move
 * (manual_moves = 2), and a search-only engine's (manual_moves = 1) under get_action(temperature = 0) -- is the FIRST MAXIMUM of the
 * root's visit counts in move order.  xq_engine_settle, called ahead of xq_engine_select in a step and on the same stream, ends
 * the search of every slot whose remaining simulations cannot move that maximum: one kernel, one wavefront per slot, no LDS, no
 * scratch, no atomics.  A slot that searches (sims_done < budget = num_simulations) with nch root children is SETTLED when
 *     nch == 1                          the move is forced, or
 *     n1 - n2 > budget - sims_done      n1 the largest child visit count, n2 the second largest counted with multiplicity (a tie
 *                                       for first: lead 0).  Strict: at lead == remaining the runner-up can still tie, and the
 *                                       first maximum in move order might then be the runner-up.
 * A simulation adds one visit to one root child, so the rule is exact: no move, game or verdict changes.
 * A settled slot of an arena engine gets sims_done = budget: the select kernel that follows plays the first maximum as at the end
 * of a full search, and the next root request resets the word; the simulations not run are not counted in `sims`.  A settled
 * slot of a search-only engine goes to phase HOLD and keeps its sims_done: xq_engine_read_root reports what was really run.
 * Slots that wait for an evaluation, idle or hold are not touched.
 * dev_counters: caller-owned, zeroed by the caller, uint64[n_games][2]; row s is written by slot s's wavefront only -- [0] searches
 * settled, [1] simulations not run.  The caller sums the columns.
 * XQ_ERR_ARG before any launch: a null engine or counter buffer; a self-play engine (manual_moves = 0: there the visit counts are
 * the training target); leaf batching (K > 1: pending descents), proven-result search (its rule 5 plays the first maximum of
 * adjusted counts, not of N), Gumbel root search, playout cap, forced playouts and tree reuse.  An engine that is never handed
 * to this call launches exactly what it launched before. */
int xq_engine_settle(const xq_engine *eng, unsigned long long *dev_counters /* [n_games][2] */, void *stream);

/* Table adjudication (opt-in): a game whose real position an endgame table decides ends there, with the exact result.
 * THE RULE (one device function for both calls).  The board is matched against the signature as xq_tb_probe_batch matches it.
 * Where that says "not in this table" and opts->both_colours is 1, the colour-swapped image -- board'[i] = -board[89 - i], the
 * other side to move -- is matched as well: the table of "Ra" also serves K+A against K+R.  A value is from the view of the side
 * to move, so the swap does not change it.  With a match the entry is read: XQ_TB_INVALID is "not covered"; 0 is a draw,
 * adjudicated only when opts->draws is 1; otherwise the winner is the side to move for v > 0 and the other side for v < 0.
 *   status   0 decided; +1 not in the table under either colouring; +2 a king is missing; +4 the entry is XQ_TB_INVALID; +8 a
 *            drawn entry with draws = 0; +16 matched through the swapped image (informational: beside 0 or 8 only).
 *   winner   +1 / -1 / 0 with status 0 or 16, else 0.     value   the entry's word with status 0, 8, 16 or 24, else 0.
 * xq_tb_adjudicate_batch: stateless, one wavefront per position; boards int8[n][90], side int8[n] (1 red, anything else black);
 * every output word is written.  n = 0 is a no-op.
 * xq_engine_adjudicate: the engine stage, called after xq_engine_select and ahead of the expand call of the same step, on the
 * same stream, once per table.  One wavefront per slot, no scratch, no atomics.  A slot is looked at when it waits for its root's
 * evaluation, its root status word is 0 (the rules' own verdicts -- game over, max_game_length -- and an earlier table's come
 * first) and its game has at least opts->min_ply plies.  A decided slot gets root status XQ_REASON_TABLE and the winner, the two
 * words the root request itself writes; nothing else of the engine's state is written.  The expand call that follows ends the game:
 * its samples carry the exact z and its xq_game_result reason XQ_REASON_TABLE.  The slot's root row is still evaluated once: the
 * resign rule reads its value before the status.  With enable_resign a resignation at that very position takes precedence, as it
 * does over a position the rules end.
 * dev_counters: caller-owned, zeroed by the caller, uint64[n_games][4]; row s is written by slot s's wavefront only -- [0] games
 * ended decisive, [1] games ended drawn, [2] covered but left alone (a drawn entry with draws = 0), [3] matched through the
 * swapped colours.  The caller sums the columns.
 * XQ_ERR_ARG before any launch (no GPU needed): a null engine, table, opts or counter pointer (the batch call: with n > 0 a null
 * pointer, and n < 0); a bad signature, or entries != xq_tb_entries(pieces, n_pieces); reserved != 0; min_ply < 0; draws or
 * both_colours outside {0, 1}; manual_moves = 1 (a search-only engine's caller asked for a search) or outside 0..2.  Self-play
 * (0) and arena (2) engines are accepted.  An engine that is never handed to this call launches exactly what it launched before. */
#define XQ_REASON_TABLE 5      /* xq_game_result.reason of a game a table adjudicated */
typedef struct xq_adjudicate_opts {
    int32_t draws;          /* 1: a drawn entry ends the game as a draw */
    int32_t both_colours;   /* 1: the colour-swapped image is matched as well */
    int32_t min_ply;        /* games shorter than this are left alone */
    int32_t reserved;       /* 0 */
} xq_adjudicate_opts;
int xq_tb_adjudicate_batch(const int8_t *pieces, int n_pieces, const int16_t *dev_table, int64_t entries,
                           const int8_t *dev_boards /* [n][90] */, const int8_t *dev_side /* [n] */, int n,
                           const xq_adjudicate_opts *opts, uint8_t *dev_status, int8_t *dev_winner, int16_t *dev_value,
                           void *stream);
int xq_engine_adjudicate(const xq_engine *eng, const int8_t *pieces, int n_pieces, const int16_t *dev_table, int64_t entries,
                         const xq_adjudicate_opts *opts, unsigned long long *dev_counters /* [n_games][4] */, void *stream);

/* Per-side resign rule with a no-resign holdout (opt-in).  The engine's own rule (enable_resign; the reference's) asks that the
 * last resign_check_steps root values, each seen from its own side to move, all lie below the threshold: for K >= 2 both sides
 * must judge themselves lost on neighbouring plies.  That rule stays as it is.  This option reads the same values per side.
 * THE RULE (one device function for both calls).  v_0, v_1, .. are a game's root values in the order the engine records them: one
 * per real position once the game has more than 10 samples, written into the slot's ring of 16 doubles (a float32 widened) and
 * counted per game.  The sides to move alternate.  With K = check_steps, 1 <= K <= XQ_RESIGN_MAX_STEPS,
 *     w_n = max(v_n, v_{n-2}, .., v_{n-2(K-1)})      the K latest values of the side to move at n; defined for n >= 2(K-1); a
 *                                                    window that holds a NaN is NaN.  2K - 1 <= 15: the ring holds every window.
 *   level       level[s] is the minimum of w_n over the positions where s was to move ([0] red, [1] black), +inf while there is
 *               none; level_ply[s] is the game ply where that minimum was FIRST reached (strict <; a NaN window lowers nothing).
 *   resign      a game that is not exempt is resigned by the side to move at the first n with w_n < threshold: strict, the
 *               recorded double against the double threshold, a NaN never.  The result: winner -side, reason 3.  The position
 *               gets no sample -- the engine's own rule likewise ends a game before a move is searched there.
 *   holdout     a game is exempt iff (philox_u64(seed, rank, slot, XQ_RNG_KIND_RESIGN_HOLDOUT, game_seq, 0) >> 11) * 2^-53 <
 *               holdout_prob: the engine's Philox4x32-10, the start pool's kind of draw; stateless, never injected, repeated on
 *               the host by xq_resign_exempt_host (1 exempt, 0 not; XQ_ERR_ARG for rank or slot < 0 or a probability outside
 *               [0, 1]).  An exempt game is never resigned.
 *   row         when an exempt game finishes, by whatever ending, one xq_resign_row is appended to dev_rows: the row index is
 *               atomicAdd(dev_row_count, 1); a row at or past max_rows is not written and counts as dropped.  The caller reads
 *               min(*dev_row_count, max_rows) rows and zeroes the counter between steps.
 * xq_engine_resign: the engine stage, called once per step ahead of xq_engine_select and on the same stream: behind the previous
 * step's expand call, which recorded the value and expanded the root, and ahead of the select call's own kernels, which flush a
 * finished game.  One wavefront per slot, no LDS, no scratch, no workgroup barrier; the row index is the only atomic.  A slot is
 * looked at when its game number changed (the state is reset), when a new value was recorded, or when it stands finished and is
 * not yet closed.  A slot that searches, whose new window is below the threshold and whose game is not exempt, gets the three
 * words a finished game has (winner -side, reason 3, phase finished); the select call that follows flushes the game and counts it
 * in xq_engine_stats.resigns.  A slot the rules (or a table) ended at this very position stays theirs.
 * The engine's own rule must be the recorder: cfg.enable_resign = 1 with cfg.resign_threshold = -INFINITY fills the ring and never
 * fires.  dev_state: caller-owned, zeroed by the caller, xq_resign_state_bytes(n_games) bytes (0 for n_games < 1): per slot the
 * values seen, the game number, the two levels and plies and a closed mark.  dev_counters: caller-owned, zeroed by the caller,
 * uint64[n_games][4]; row s is written by slot s's wavefront only -- [0] games resigned, [1] holdout games closed, [2] rows
 * dropped, [3] values seen.  The caller sums the columns.
 * xq_resign_scan_batch: the stateless twin over n sequences, one wavefront each: values float[n][max_len], len int32[n] (clamped
 * to [0, max_len]), first_side int8[n] (1 red, anything else black: the side to move at index 0).  Every output word is written:
 * resign_index int32[n] (the first n with w_n < threshold, -1 for none), resigner int8[n] (that side, 0 for none), level
 * float[n][2] and level_index int32[n][2] (the index the level was first reached at, -1 while +inf) over the WHOLE sequence, as for
 * an exempt game.  n = 0 is a no-op.
 * XQ_ERR_ARG before any launch (no GPU needed): a null pointer (dev_rows may be NULL with max_rows = 0; the batch call: with n > 0,
 * dev_values may be NULL with max_len = 0); reserved != 0; check_steps outside 1..XQ_RESIGN_MAX_STEPS; holdout_prob outside [0, 1]
 * or NaN; a NaN threshold; max_rows < 0 (the batch call: n < 0, max_len < 0); manual_moves != 0 (arena and search-only engines
 * record no values); an engine whose enable_resign is 0 or whose own resign_threshold is not -INFINITY.  Every other engine option
 * is accepted: the words an expanded root leaves behind are rewritten by the next root request.  An
 * engine that is never handed to this call launches exactly what it launched before. */
#define XQ_RNG_KIND_RESIGN_HOLDOUT 12
#define XQ_RESIGN_MAX_STEPS 8
typedef struct xq_resign_opts {
    double threshold;       /* resign when the window is below this; -INFINITY: nobody resigns */
    double holdout_prob;    /* the share of games played out, in [0, 1] */
    int32_t check_steps;    /* K */
    int32_t reserved;       /* 0 */
} xq_resign_opts;
typedef struct xq_resign_row {      /* 32 bytes: one finished exempt game */
    uint32_t slot, game_seq;
    float level[2];         /* red, black; +inf: that side never had a full window */
    uint16_t level_ply[2];  /* the game ply the level was first reached at (0 with +inf) */
    int8_t winner;          /* as in xq_game_result */
    uint8_t reason;
    uint16_t plies;
    uint32_t zero[2];
} xq_resign_row;
size_t xq_resign_state_bytes(int n_games);
int xq_resign_exempt_host(uint64_t seed, int rank, int slot, uint32_t game_seq, double holdout_prob);
int xq_resign_scan_batch(const float *dev_values /* [n][max_len] */, const int32_t *dev_len, const int8_t *dev_first_side, int n,
                         int max_len, int check_steps, double threshold, int32_t *dev_resign_index, int8_t *dev_resigner,
                         float *dev_level /* [n][2] */, int32_t *dev_level_index /* [n][2] */, void *stream);
int xq_engine_resign(const xq_engine *eng, const xq_resign_opts *opts, void *dev_state, xq_resign_row *dev_rows, int max_rows,
                     unsigned int *dev_row_count, unsigned long long *dev_counters /* [n_games][4] */, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* XQ_HIP_H */
