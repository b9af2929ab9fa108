"""Device-resident self-play engine: host-side driver of the B3 entry points (include/xq_hip.h).

One `SelfPlayEngine` owns G concurrent game slots on one GPU.  A step is

    select (HIP)  ->  evaluator over the [G,15,10,9] leaf batch  ->  expand/backup (HIP)

all enqueued on torch's current stream; no host round-trip per simulation and no IPC (the reference's
per-evaluation socket hop, training/inference_server.py:333-349, does not exist here).  torch provides
device memory, the stream and (optionally) the network; search, rules, sampling and bookkeeping are the
hand-written kernels.  There is no CPU fallback.

`step()` / `capture_step()` take the PACKED step when the evaluator offers `live_rows` (the HIP evaluators):

    select  ->  compact (the waiting slots, packed to the front, slot order)  ->  evaluator over the first n_live rows
            ->  scatter back to slot order + expand

The live count never leaves the device, so the packed step records into one HIP graph like the full-width one; once games
finish (games_target reached: idle slots) the evaluator's work follows the slots that are still playing.  Results are
identical to the full-width step.  The explicit stage calls (`select`, `evaluate_and_expand`, `expand_legal`) stay full width.

With `eval_cache_entries = K > 0` (opt-in, a power of two) the engine owns a per-slot evaluation cache (xq_evcache_*) and
`step()` / `capture_step()` take the CACHED step:

    select  ->  probe (hits answered from the slot's table)  ->  compact the misses + gather  ->  evaluator over n_live rows
            ->  scatter back to slot order + expand  ->  commit (insert the evaluated rows)

A cached row is bit-identical to a recomputed one, so the games are those of the packed step; `rows_evaluated` counts only
the rows the network ran on.  The table costs `eval_cache_bytes(G, K)` (576 B per entry); `recommended_cache_entries(S)`
is the next power of two >= 2 S, about two moves of evaluations.  A weight update of the evaluator (`weights_version`) or
another evaluator invalidates the table before the next step.

With `leaves_per_step = K > 1` (opt-in, K <= 64; xq_engine_init_leaves) a searching slot hands the evaluator up to K leaves
per step, collected under virtual loss (include/xq_hip.h), so a move needs about S / K steps instead
of S.  Every request buffer then has G K rows, slot-major (row slot K + j is pending leaf j): `nn_input`, `req_moves`,
`req_counts`, the packed buffers and the evaluator's outputs.  Dense, sparse and packed protocols, eager and replayed, work
as with K = 1.  K > 1 is knowingly not the reference's sequential search; it cannot be combined with the evaluation cache
or with arena games (manual_moves = 2).  K = 1 is the engine as before.

With `tree_reuse=True` (opt-in; xq_engine_init_ex, XQ_ENGINE_TREE_REUSE) a slot keeps the chosen child's subtree when a move
ends: the next search starts from it with its visits, stops at S visits as always and so costs S minus
the reused visits in new simulations.  `stats()` adds `reused_visits` and `reroots`.  A weight update of the evaluator
(`weights_version`) or another evaluator drops the pending re-roots before the next step (`drop_reroots`).  Self-play only
(manual_moves = 0), K = 1 and S <= 1600; it combines with the evaluation cache.

With `playout_cap=(full_search_prob, fast_simulations)` (opt-in; xq_engine_init_cap) every searched
position takes one draw of the slot's uniform stream: with probability p the move is a full move (noise, S simulations, a
sample), otherwise a fast one (no noise, `fast_simulations`, no sample).  `stats()` adds `fast_moves` and `fast_sims`.
Self-play only, K = 1; it combines with tree reuse and the evaluation cache.

With `forced_playouts=k` (opt-in, 0 < k <= 16, KataGo uses 2; xq_engine_init_fp) a visited child of a
noisy root is forced until its visits reach sqrt(k * noisy prior * root visits), and the forced visits the search would not have
spent by itself are subtracted again before the visit counts become the sample's target and the move distribution, so a
sample's visits sum to at most S.  The tree keeps its real counts.  `stats()` adds `forced_sims`, `pruned_visits` and
`pruned_children`.  Self-play with root noise only, K = 1; it combines with tree reuse, the playout cap (full moves only) and
the evaluation cache.

With `gumbel=(m, c_visit, c_scale)` (opt-in, 1 <= m <= 128, mctx uses c_visit = 50 and c_scale = 1; xq_engine_init_gz, DESIGN.md
section 4.9) the root rule is Gumbel AlphaZero's: m moves sampled without replacement by the Gumbel-top-k trick, the budget spent
on them by sequential halving, the move with the best g + log prior + sigma(q) among the most visited played without temperature,
and the sample's `visits` hold the completed-Q improved policy quantised to 16 bits (`reserved0` = 1) instead of visit counts.
Interior nodes keep PUCT.  `stats()` adds `gumbel_moves`, `gumbel_considered` and `gumbel_offprior`.  Self-play and search only
(manual_moves 0 or 1), K = 1; it combines with the evaluation cache and with nothing else.

With `arena_opts=(opening_plies, first_game)` (opt-in; xq_engine_init_ar) an arena engine (manual_moves = 2)
starts game `first_game + slot` with `opening_plies` random legal plies drawn for the game's PAIR, so games 2p and 2p + 1 share an
opening with colours swapped, and offers the per-model packed step: `compact_arena()` packs the waiting slots into two buffer sets
(`arena_packed[0]`: the new model's slots, `arena_packed[1]`: the old model's), `expand_packed_arena()` scatters both models'
outputs back.  `arena_openings()` reads what was played.  K = 1, none of the other options.

With `perpetual_check=True` (opt-in; xq_engine_init_ru) the side that checks through a repetition loses:
where the reference calls three repetitions in the 12-board window a draw, the side whose every move of the repetition span gave
check loses when the other side's did not.  The verdict holds at the root, in the real game and at the leaves of the search; a
game it decides has `reason` 4 in its result (1 rules, 2 max_game_length adjudication, 3 resign, 4 rules: repetition, perpetual
check, 5 an endgame table: `adjudicate` below).  Every mode, every other option.

With `solver=True` (opt-in; xq_engine_init_sv) the search keeps exact results (MCTS-solver): a terminal leaf
sets its node's proven state and backs up the true +1 / 0 / -1, states propagate up the path, a descent stops at a decided node, a
child shown to lose is never chosen while a sibling is not, a root with a winning child ends the move at once on that child (the
sample then carries `reserved1` = 1), and a losing child's visits leave the sample and the move distribution.  `read_root_states`
reads the states at a root, `solver_stats` (merged into `stats()`) the five counters.  Self-play with tree reuse, the playout cap
and the evaluation cache, search only, arena games, the perpetual-check rule; not with leaves_per_step > 1, gumbel or
forced_playouts.

With `root_stats=True` (opt-in; xq_engine_init_rs) every sample carries the search's own value of its
position in its 20 spare bytes (`sample_format.root_stats`): `root_q` from the view of the side to move, `root_visits`, and the
mark `has_root_stats`.  `ReplayBuffer.batch(..., q_mix=...)` mixes it into the value target.  Nothing else about the games
changes.  Self-play only; every other option but gumbel.

With `eval_mirror=True` (opt-in; xq_engine_init_em) every request of the packed step is evaluated under a
randomly chosen left-right orientation: `compact()` hands the evaluator the mirrored planes and the mirrored move list, in the
original order, when the request's bit (`hip.eval_mirror_bit`, a function of seed, rank, slot, game, ply, root / leaf, simulations
done and row) is 1, so the logits come back un-mirrored and the search averages the network's left/right asymmetry away.  It needs
the packed step (an evaluator with `live_rows`); not with the evaluation cache and not for arena games; every other option.

With `record_games=True` (opt-in; xq_engine_init_gr) every finished game leaves a 1024-byte record
(`hip.GAME_RECORD_DTYPE`): slot and game_seq (the join key with its result and samples), winner, reason, n_moves, opening_plies,
n_samples and the action of every ply, opening plies, fast moves and arena moves included.  `drain_games()` returns the records of
the games finished since its last call (at most `max_out_games`, default the config's max_out_results; later games count in
`game_records_stats()['dropped']`), `drain_games_device()` the same as a device tensor.  `replay_games` plays records on the
device: legality of every move, the position at any ply in `set_position`'s form, and the rules' verdict there.  Games, samples,
results and statistics are byte-identical with and without it.  Self-play and arena engines, every other option.

With `start_pool=(boards, sides, prob)` (opt-in; xq_engine_init_sp) a new game starts, with probability
`prob`, from an entry of the pool instead of the initial position: `boards` int8[n, 90] and `sides` int8[n], numpy arrays or
device tensors (`start_pool.py` makes them from FEN lines, tablebase entries or game records).  The draw is a function of seed,
rank, slot and the game's number (`hip.start_pool_index`).  A pool game plays no random opening, starts at ply 0 with an empty
history, and every ply counter counts from there.  The engine checks the pool first (`hip.positions_check`) and refuses an entry
the rules code cannot run on; an entry without a legal move is a game that finishes at ply 0 with no sample.  `start_indices()`
reads the entry every slot's current game started from (-1: the initial position), `start_pool_stats()` the number of pool games.
Self-play only; not with record_games, whose record has no room for a start position; every other option.

With `eval_dedup=True` (opt-in; xq_evdedup_*) slots that ask for the same position in the same step share
one evaluated row, and `step()` / `capture_step()` take the DEDUP step:

    select  ->  keys + resolve (per waiting slot: the cache's exact 12-word key, the lowest slot with that key and count represents
                it)  ->  compact the representatives + gather  ->  evaluator over n_live rows
            ->  every waiting slot takes its representative's row + expand

The row a slot is handed is bit-identical to the one it would have computed, so the games are those of the packed step;
`rows_evaluated` counts only the rows the network ran on and `stats()` adds `eval_dedup_requests`, `eval_dedup_merged`,
`eval_dedup_collisions` (two positions in one bucket: the higher slot evaluates itself) and `eval_dedup_mismatches` (must stay 0).
Nothing is kept across steps, so a weight update needs no invalidation.  It needs the packed step (an evaluator with `live_rows`);
not with the evaluation cache, leaves_per_step > 1, eval_mirror or arena games; every other option.

With `early_stop=True` (opt-in; xq_engine_settle) `select()` first ends every search whose first choice is
fixed: one root child (a forced move), or a leader whose lead over the runner-up is larger than the simulations that are left.  An
arena engine then plays that move at once, a search-only engine holds the search with its true `sims_done`; the move is the one the
full search plays, always.  `early_stop_stats()` reads `settled_moves` and `simulations_saved`.  One more kernel per step, eager and
recorded.  Arena (manual_moves = 2) and search-only (1) engines; not with leaves_per_step > 1, solver, gumbel, playout_cap,
forced_playouts or tree_reuse.  A caller that reads a search-only engine's visit counts as a distribution wants the full search.

With `adjudicate=(tables, dict(draws=..., both_colours=..., min_ply=...))` (opt-in; xq_engine_adjudicate)
a game stops as soon as its real position is in one of the `tables` (one to four `endgame.Tablebase` objects on the engine's
device): `select()` then runs the public stage `adjudicate()` behind the select kernel, once per table in order, and the expand
kernels end every game it decided with `reason` 5 and the table's winner, so every sample of the game carries the exact z.
`both_colours` (default on) also matches the colour-swapped image, so the table of "Ra" serves K+A against K+R; `draws` (default
on) ends drawn entries as draws; `min_ply` (default 1) leaves shorter games alone, so a start-pool game that begins inside a table
still yields the one move that leads to its first adjudicated root (0: it ends at ply 0 with no sample).  The rules' own verdicts
and, with enable_resign, a resignation at that position come first.  `adjudication_stats()` sums the counters.  One more kernel
per table per step, in all four step paths, eager and recorded.  Self-play and arena engines, every other option.

With `resign=dict(threshold=, check_steps=, holdout_prob=, max_rows=)` (opt-in; xq_engine_resign) a side
resigns when its own last `check_steps` root values -- every second recorded value -- all lie below `threshold`; the engine's own
rule, which asks that of both sides at once, is turned into the recorder of those values (enable_resign with threshold -inf) and
never fires.  `select()` first runs the public stage `resign_stage()`; a resigned game has `reason` 3 and counts in `resigns`.  A
share `holdout_prob` of the games, drawn statelessly per (slot, game_seq) (`hip.resign_exempt` repeats the draw), is exempt and
played out; `drain_resign_rows()` returns, per finished holdout game, the lowest window each side ever had and the result, which
`resign.false_positive_curve` and `resign.calibrate` turn into a threshold.  `resign_stats()` sums the counters,
`set_resign_threshold()` plays on under another threshold.  One more kernel per step, in all four step paths, eager and recorded.
Self-play engines only, every other option.
"""
from __future__ import annotations

import collections
import ctypes as C
import math
from typing import Callable, Optional

import numpy as np
import torch

from . import hip

from .sample_format import RESULT_DTYPE, SAMPLE_DTYPE, dense_pi  # noqa: E402

assert SAMPLE_DTYPE.itemsize == hip.SAMPLE_BYTES and RESULT_DTYPE.itemsize == hip.RESULT_BYTES


def make_config(n_games: int, num_simulations: int, *, c_puct: float = 1.5, temperature_threshold: int = 20,
                max_game_length: int = 300, random_opening_moves: int = 4, enable_resign: bool = True,
                resign_threshold: float = -0.9, resign_check_steps: int = 5, add_noise: bool = True,
                dirichlet_alpha: float = 0.3, noise_eps: float = 0.25, late_temperature: float = 0.3,
                seed: int = 0, rank: int = 0, inject_len: int = 0, games_target: int = 0,
                max_out_samples: int = 0, max_out_results: int = 0, manual_moves: int = 0,
                start_stagger: bool = False) -> hip.EngineConfig:
    """Defaults are the reference's TrainingConfig (training/train.py:55-111) and hard-coded constants
    (mcts.py:118-121, parallel_selfplay.py:92)."""
    if max_out_samples <= 0:
        max_out_samples = max(4096, 4 * n_games * 64)
    if max_out_results <= 0:
        max_out_results = max(1024, 8 * n_games)
    return hip.EngineConfig(n_games, num_simulations, c_puct, temperature_threshold, max_game_length,
                            random_opening_moves, int(enable_resign), resign_threshold, resign_check_steps,
                            int(add_noise), dirichlet_alpha, noise_eps, late_temperature, seed, rank, inject_len,
                            games_target, max_out_samples, max_out_results, int(manual_moves), int(start_stagger))


def recommended_cache_entries(num_simulations: int) -> int:
    """Evaluation-cache entries per slot that hold about two moves of a slot's evaluations: the next power of two >= 2 S."""
    n = 1
    while n < 2 * max(1, int(num_simulations)):
        n *= 2
    return n


def eval_cache_bytes(n_slots: int, entries_per_slot: int) -> int:
    """Device bytes of an evaluation cache (xq_evcache_bytes): 576 B per entry plus ~100 B per slot; 0 for invalid sizes.
    BASELINE configs[2] (8192 slots, 800 simulations, K = 2048): 9.7 GB, next to the engine's 20 GB tree arenas."""
    return int(hip.lib().xq_evcache_bytes(int(n_slots), int(entries_per_slot)))


# What `parse_engine_options` returns: the arguments every xq_engine_workspace_bytes_* / xq_engine_init_* call takes after the
# config, the four structs as ctypes structures or None (the C side's NULL)
class EngineOptions(collections.namedtuple("EngineOptions", "K flags cap forced gumbel arena")):
    # the tuple is the argument list of xq_engine_*_ar; `rules` (hip.RulesOpts or None) is what xq_engine_*_ru take after it
    rules = None
    solver = None              # hip.SolverOpts or None: what xq_engine_*_sv take after `rules`
    root_stats = None          # hip.RootStatsOpts or None: what xq_engine_*_rs take after `solver`
    eval_mirror = None         # hip.EvalMirrorOpts or None: what xq_engine_*_em take after `root_stats`
    game_records = None        # hip.GameRecordsOpts or None: what xq_engine_*_gr take after `eval_mirror`
    eval_dedup = False         # no C struct: the dedup is an object of its own (hip.DedupTable), like the evaluation cache


RULES_REASONS = (1, 4)     # a result's `reason` for a game the rules ended: is_game_over, and its perpetual-check verdict


def parse_start_pool(cfg: hip.EngineConfig, start_pool, record_games: bool = False):
    """The `start_pool=(boards, sides, prob)` argument checked, without a GPU -> (boards, sides, prob) with numpy arrays made
    int8[n, 90] / int8[n] and device tensors left as they are, or None.  Every rule of xq_engine_init_sp's refusal list but the
    check of the positions themselves, which needs the device (`SelfPlayEngine` runs it)."""
    if start_pool is None:
        return None
    try:
        boards, sides, prob = start_pool
        prob = float(prob)
    except (TypeError, ValueError):
        raise hip.XqError("start_pool must be (boards, sides, prob)")
    if not isinstance(boards, torch.Tensor):
        boards = np.ascontiguousarray(boards, dtype=np.int8)
    if not isinstance(sides, torch.Tensor):
        sides = np.ascontiguousarray(sides, dtype=np.int8)
    n = int(boards.shape[0]) if boards.ndim >= 1 else -1
    bad_dtype = any(isinstance(a, torch.Tensor) and a.dtype != torch.int8 for a in (boards, sides))    # numpy: cast above
    if n < 0 or bad_dtype or int(np.prod(tuple(boards.shape))) != n * 90 or tuple(sides.shape) != (n,):
        raise hip.XqError(f"start_pool: boards must be int8[n, 90] and sides int8[n], got {tuple(boards.shape)} and "
                          f"{tuple(sides.shape)}")
    if not 1 <= n <= hip.START_POOL_MAX:
        raise hip.XqError(f"start_pool: the pool must hold 1 to {hip.START_POOL_MAX} positions, got {n}")
    if not 0.0 < prob <= 1.0:                          # a NaN fails both comparisons
        raise hip.XqError(f"start_pool: prob must be in (0, 1], got {prob}")
    if int(cfg.manual_moves) != 0:
        raise hip.XqError("start_pool is a self-play option: not available with manual_moves = 1 (search only) or 2 (arena)")
    if record_games:
        raise hip.XqError("start_pool cannot be combined with record_games: a record has no room for a start position and its "
                          "replay starts from the initial one")
    return boards.reshape(n, 90), sides, prob


def parse_early_stop(cfg: hip.EngineConfig, early_stop, *, leaves_per_step: int = 1, tree_reuse: bool = False, playout_cap=None,
                     forced_playouts=None, gumbel=None, solver: bool = False) -> bool:
    """The `early_stop=` argument checked, without a GPU -> bool.  Every rule of xq_engine_settle's refusal list
    (include/xq_hip.h), each with a message that names the option."""
    if early_stop not in (False, True, 0, 1):
        raise hip.XqError(f"early_stop must be a bool, got {early_stop!r}")
    if not early_stop:
        return False
    if int(cfg.manual_moves) == 0:
        raise hip.XqError("early_stop is an option of decided moves (arena games, manual_moves = 2, and searches read at "
                          "temperature 0, manual_moves = 1): in self-play the visit counts are the training target")
    if int(leaves_per_step) > 1:
        raise hip.XqError("early_stop cannot be combined with leaves_per_step > 1: pending descents are not in the visit counts yet")
    if solver:
        raise hip.XqError("early_stop cannot be combined with solver: its move is the first maximum of adjusted counts, not of "
                          "the visit counts")
    if gumbel is not None:
        raise hip.XqError("early_stop cannot be combined with gumbel: a Gumbel root does not play the first maximum of its visits")
    if playout_cap is not None:
        raise hip.XqError("early_stop cannot be combined with playout_cap: a fast move has another budget")
    if forced_playouts is not None:
        raise hip.XqError("early_stop cannot be combined with forced_playouts: its move is chosen from pruned counts")
    if tree_reuse:
        raise hip.XqError("early_stop cannot be combined with tree_reuse: a reused root starts with visits that are not this search's")
    return True


ADJUDICATE_MAX_TABLES = 4
ADJUDICATE_DEFAULTS = dict(draws=True, both_colours=True, min_ply=1)


def parse_adjudicate(cfg: hip.EngineConfig, adjudicate):
    """The `adjudicate=(tables, options)` argument checked, without a GPU -> (tuple of endgame.Tablebase, hip.AdjudicateOpts), or
    None.  `tables`: one `endgame.Tablebase` or a sequence of 1 to 4; `options`: a dict (or None) with draws, both_colours (bools,
    default True) and min_ply (an integer >= 0, default 1).  Every rule of xq_engine_adjudicate's refusal list (include/xq_hip.h),
    each with a message that names the option."""
    if adjudicate is None:
        return None
    from .endgame import Tablebase
    try:
        tables, options = adjudicate
    except (TypeError, ValueError):
        raise hip.XqError("adjudicate must be (tables, options): endgame.Tablebase objects and a dict of draws, both_colours, min_ply")
    if isinstance(tables, Tablebase):
        tables = (tables,)
    try:
        tables = tuple(tables)
    except TypeError:
        raise hip.XqError(f"adjudicate: tables must be endgame.Tablebase objects, got {type(tables).__name__}")
    if not 1 <= len(tables) <= ADJUDICATE_MAX_TABLES:
        raise hip.XqError(f"adjudicate: 1 to {ADJUDICATE_MAX_TABLES} tables, got {len(tables)}")
    for tb in tables:
        if not isinstance(tb, Tablebase):
            raise hip.XqError(f"adjudicate: tables must be endgame.Tablebase objects, got {type(tb).__name__}")
    if options is None:
        options = {}
    if not isinstance(options, dict) or any(k not in ADJUDICATE_DEFAULTS for k in options):
        raise hip.XqError(f"adjudicate: options must be a dict with keys from {sorted(ADJUDICATE_DEFAULTS)}, got {options!r}")
    opts = hip.adjudicate_opts(**{**ADJUDICATE_DEFAULTS, **options}, what="adjudicate")
    if int(cfg.manual_moves) == 1:
        raise hip.XqError("adjudicate is an option of engines that play games (self-play, manual_moves = 0, and arena, 2): the "
                          "caller of a search-only engine (manual_moves = 1) asked for a search")
    if int(cfg.manual_moves) not in (0, 2):
        raise hip.XqError(f"adjudicate: manual_moves must be 0 or 2, got {cfg.manual_moves}")
    return tables, opts


RESIGN_KEYS = ("threshold", "check_steps", "holdout_prob", "max_rows")


def parse_resign(cfg: hip.EngineConfig, resign):
    """The `resign=dict(threshold=, check_steps=, holdout_prob=, max_rows=)` argument checked, without a GPU -> (hip.ResignOpts,
    max_rows), or None.  threshold is required (-inf: nobody resigns); check_steps defaults to 5, holdout_prob to 0.1, max_rows
    (the holdout rows kept between two drains) to max(1024, 8 n_games).  Every rule of xq_engine_resign's refusal list
    (include/xq_hip.h) but the engine's own rule as recorder, which `SelfPlayEngine` sets itself."""
    if resign is None:
        return None
    if not isinstance(resign, dict) or not set(resign) <= set(RESIGN_KEYS) or "threshold" not in resign:
        raise hip.XqError(f"resign must be a dict with threshold and keys from {list(RESIGN_KEYS)}, got {resign!r}")
    opts = hip.resign_opts(resign["threshold"], resign.get("check_steps", 5), resign.get("holdout_prob", 0.1), what="resign")
    max_rows = resign.get("max_rows")
    if max_rows is None:
        max_rows = max(1024, 8 * int(cfg.n_games))
    try:
        ok = not isinstance(max_rows, bool) and int(max_rows) == max_rows and 0 <= int(max_rows) <= 2 ** 31 - 1
    except (TypeError, ValueError, OverflowError):
        ok = False
    if not ok:
        raise hip.XqError(f"resign: max_rows must be an integer >= 0, got {max_rows!r}")
    if int(cfg.manual_moves) != 0:
        raise hip.XqError("resign is a self-play option: not available with manual_moves = 1 (search only) or 2 (arena), whose "
                          "engines record no root values")
    return opts, int(max_rows)


def parse_engine_options(cfg: hip.EngineConfig, *, leaves_per_step: int = 1, tree_reuse: bool = False, playout_cap=None,
                         forced_playouts=None, gumbel=None, arena_opts=None, eval_cache_entries: int = 0,
                         perpetual_check: bool = False, solver: bool = False, root_stats: bool = False,
                         eval_mirror: bool = False, record_games: bool = False, max_out_games=None,
                         eval_dedup: bool = False) -> EngineOptions:
    """The engine options of `SelfPlayEngine` checked and turned into the C structs; needs no GPU.  Every rule of the header's
    refusal lists (include/xq_hip.h; opts_ok in csrc/xq_engine_setup.hip) is refused here first, with a message that names the
    option; tests/test_engine_options.py holds the two side by side."""
    K = int(leaves_per_step)
    if not 1 <= K <= 64:
        raise hip.XqError(f"leaves_per_step must be in [1, 64], got {leaves_per_step}")
    tree_reuse = bool(tree_reuse)
    if tree_reuse and int(cfg.manual_moves) != 0:
        raise hip.XqError("tree_reuse is a self-play option: not available with manual_moves = 1 (search only) or 2 (arena)")
    if tree_reuse and K > 1:
        raise hip.XqError("tree_reuse cannot be combined with leaves_per_step > 1")
    if tree_reuse and int(cfg.num_simulations) > hip.REUSE_MAX_SIMS:
        raise hip.XqError(f"tree_reuse supports num_simulations <= {hip.REUSE_MAX_SIMS}, got {cfg.num_simulations}")
    cap = None
    if playout_cap is not None:
        try:
            p_full, s_fast = float(playout_cap[0]), int(playout_cap[1])
        except (TypeError, ValueError, IndexError):
            raise hip.XqError("playout_cap must be (full_search_prob, fast_simulations)")
        if int(cfg.manual_moves) != 0:
            raise hip.XqError("playout_cap is a self-play option: not available with manual_moves = 1 (search only) or 2 (arena)")
        if K > 1:
            raise hip.XqError("playout_cap cannot be combined with leaves_per_step > 1")
        if not 1 <= s_fast < int(cfg.num_simulations):
            raise hip.XqError(f"playout_cap: fast_simulations must be in [1, num_simulations), got {s_fast}")
        if not 0.0 < p_full <= 1.0:                    # a NaN fails both comparisons
            raise hip.XqError(f"playout_cap: full_search_prob must be in (0, 1], got {p_full}")
        cap = hip.PlayoutCap(s_fast, 0, p_full)
    forced = None
    if forced_playouts is not None:
        try:
            fk = float(forced_playouts)
        except (TypeError, ValueError):
            raise hip.XqError("forced_playouts must be a number k with 0 < k <= 16")
        if int(cfg.manual_moves) != 0:
            raise hip.XqError("forced_playouts is a self-play option: not available with manual_moves = 1 (search only) or 2 (arena)")
        if not int(cfg.add_noise):
            raise hip.XqError("forced_playouts acts at noisy roots only: not available with add_noise = 0")
        if K > 1:
            raise hip.XqError("forced_playouts cannot be combined with leaves_per_step > 1")
        if not 0.0 < fk <= 16.0:                       # a NaN fails both comparisons
            raise hip.XqError(f"forced_playouts: k must be in (0, 16], got {fk}")
        forced = hip.ForcedPlayouts(fk)
    gz = None
    if gumbel is not None:
        try:
            gm, gcv, gcs = int(gumbel[0]), float(gumbel[1]), float(gumbel[2])
            if len(gumbel) != 3 or gm != gumbel[0]:
                raise ValueError
        except (TypeError, ValueError, IndexError, OverflowError):
            raise hip.XqError("gumbel must be (considered_moves, c_visit, c_scale)")
        if int(cfg.manual_moves) == 2:
            raise hip.XqError("gumbel is a self-play and search option: not available for arena games (manual_moves = 2)")
        if tree_reuse or cap is not None or forced is not None:
            raise hip.XqError("gumbel cannot be combined with tree_reuse, playout_cap or forced_playouts")
        if K > 1:
            raise hip.XqError("gumbel cannot be combined with leaves_per_step > 1")
        if not 1 <= gm <= hip.MAXM:
            raise hip.XqError(f"gumbel: considered moves must be in [1, {hip.MAXM}], got {gm}")
        f32_max = float(np.finfo(np.float32).max)
        if not (0.0 <= gcv <= f32_max) or not (0.0 < gcs <= f32_max) or not float(np.float32(gcs)) > 0.0:   # a NaN fails them
            raise hip.XqError(f"gumbel: c_visit >= 0 and c_scale > 0, finite as float32, required; got {gcv}, {gcs}")
        gz = hip.Gumbel(gm, 0, gcv, gcs)
    ar = None
    if arena_opts is not None:
        try:
            ar_plies, ar_first = int(arena_opts[0]), int(arena_opts[1])
            if len(arena_opts) != 2 or ar_plies != arena_opts[0] or ar_first != arena_opts[1]:
                raise ValueError
        except (TypeError, ValueError, IndexError, OverflowError):
            raise hip.XqError("arena_opts must be (opening_plies, first_game)")
        if int(cfg.manual_moves) != 2:
            raise hip.XqError("arena_opts needs an arena engine (manual_moves = 2)")
        if K > 1 or tree_reuse or cap is not None or forced is not None or gz is not None or eval_cache_entries:
            raise hip.XqError("arena_opts cannot be combined with another engine option")
        if not 0 <= ar_plies <= hip.ARENA_MAX_OPENING:
            raise hip.XqError(f"arena_opts: opening_plies must be in [0, {hip.ARENA_MAX_OPENING}], got {ar_plies}")
        if not 0 <= ar_first <= 2 ** 31 - 1 - int(cfg.n_games):
            raise hip.XqError(f"arena_opts: first_game must be a non-negative int32 game index, got {ar_first}")
        ar = hip.ArenaOpts(ar_plies, ar_first)
    if K > 1 and eval_cache_entries:
        raise hip.XqError("leaves_per_step > 1 cannot be combined with an evaluation cache (eval_cache_entries > 0)")
    if K > 1 and int(cfg.manual_moves) == 2:
        raise hip.XqError("leaves_per_step > 1 is not available for arena games (manual_moves = 2)")
    if perpetual_check not in (False, True, 0, 1):
        raise hip.XqError(f"perpetual_check must be a bool, got {perpetual_check!r}")
    if solver not in (False, True, 0, 1):
        raise hip.XqError(f"solver must be a bool, got {solver!r}")
    if solver and K > 1:
        raise hip.XqError("solver cannot be combined with leaves_per_step > 1")
    if solver and gz is not None:
        raise hip.XqError("solver cannot be combined with gumbel: its equal-visit candidates cannot skip a child")
    if solver and forced is not None:
        raise hip.XqError("solver cannot be combined with forced_playouts")
    if root_stats not in (False, True, 0, 1):
        raise hip.XqError(f"root_stats must be a bool, got {root_stats!r}")
    if root_stats and int(cfg.manual_moves) != 0:
        raise hip.XqError("root_stats is a self-play option: search-only (manual_moves = 1) and arena (2) engines record no samples")
    if root_stats and gz is not None:
        raise hip.XqError("root_stats cannot be combined with gumbel: a Gumbel root's value is its own v_mix")
    if eval_mirror not in (False, True, 0, 1):
        raise hip.XqError(f"eval_mirror must be a bool, got {eval_mirror!r}")
    if eval_mirror and int(cfg.manual_moves) == 2:
        raise hip.XqError("eval_mirror is a self-play and search option: not available for arena games (manual_moves = 2), whose "
                          "gate stays deterministic")
    if eval_mirror and eval_cache_entries:
        raise hip.XqError("eval_mirror cannot be combined with an evaluation cache (eval_cache_entries > 0): a hit would return "
                          "whichever orientation was evaluated first")
    if eval_dedup not in (False, True, 0, 1):
        raise hip.XqError(f"eval_dedup must be a bool, got {eval_dedup!r}")
    if eval_dedup and eval_cache_entries:
        raise hip.XqError("eval_dedup cannot be combined with an evaluation cache (eval_cache_entries > 0): the cached step "
                          "compacts by its own hit flags")
    if eval_dedup and K > 1:
        raise hip.XqError("eval_dedup cannot be combined with leaves_per_step > 1: a slot then asks for several rows")
    if eval_dedup and eval_mirror:
        raise hip.XqError("eval_dedup cannot be combined with eval_mirror: equal planes are evaluated under different orientations")
    if eval_dedup and int(cfg.manual_moves) == 2:
        raise hip.XqError("eval_dedup is a self-play and search option: not available for arena games (manual_moves = 2), where "
                          "two models answer")
    if record_games not in (False, True, 0, 1):
        raise hip.XqError(f"record_games must be a bool, got {record_games!r}")
    if max_out_games is not None and not record_games:
        raise hip.XqError("max_out_games is record_games' ring size: it needs record_games=True")
    gr = None
    if record_games:
        if int(cfg.manual_moves) == 1:
            raise hip.XqError("record_games needs an engine that plays games: not available with manual_moves = 1 (search only)")
        if int(cfg.max_game_length) > hip.RECORD_MAX_PLIES or int(cfg.random_opening_moves) > hip.RECORD_MAX_PLIES:
            raise hip.XqError(f"record_games: max_game_length and random_opening_moves must be <= {hip.RECORD_MAX_PLIES}, got "
                              f"{cfg.max_game_length}, {cfg.random_opening_moves}")
        try:
            n_out = int(cfg.max_out_results) if max_out_games is None else int(max_out_games)
            if max_out_games is not None and n_out != max_out_games:
                raise ValueError
        except (TypeError, ValueError, OverflowError):
            raise hip.XqError(f"record_games: max_out_games must be an integer, got {max_out_games!r}")
        if not 1 <= n_out <= 2 ** 31 - 1:
            raise hip.XqError(f"record_games: max_out_games must be in [1, 2^31), got {n_out}")
        gr = hip.GameRecordsOpts(1, n_out)
    opts = EngineOptions(K, hip.ENGINE_TREE_REUSE if tree_reuse else 0, cap, forced, gz, ar)
    opts.game_records = gr
    opts.eval_dedup = bool(eval_dedup)
    if eval_mirror:
        opts.eval_mirror = hip.EvalMirrorOpts(1)
    if solver:
        opts.solver = hip.SolverOpts(1)
    if root_stats:
        opts.root_stats = hip.RootStatsOpts(1)
    if perpetual_check:                                # a verdict, not a search option: it goes with every mode and option
        opts.rules = hip.RulesOpts(1)
    return opts


class SelfPlayEngine:
    def __init__(self, cfg: hip.EngineConfig, device="cuda", evaluator: Optional[Callable] = None,
                 inject: Optional[np.ndarray] = None, eval_cache_entries: int = 0, leaves_per_step: int = 1,
                 tree_reuse: bool = False, playout_cap=None, forced_playouts=None, gumbel=None, arena_opts=None,
                 perpetual_check: bool = False, solver: bool = False, root_stats: bool = False, eval_mirror: bool = False,
                 record_games: bool = False, max_out_games=None, start_pool=None, eval_dedup: bool = False,
                 early_stop: bool = False, adjudicate=None, resign=None):
        rsn = parse_resign(cfg, resign)
        if rsn is not None:
            # the engine's own rule becomes the recorder of the root values: it fills the ring and never fires
            cfg = hip.EngineConfig.from_buffer_copy(cfg)
            cfg.enable_resign, cfg.resign_threshold = 1, float("-inf")
        opts = parse_engine_options(
            cfg, leaves_per_step=leaves_per_step, tree_reuse=tree_reuse, playout_cap=playout_cap, forced_playouts=forced_playouts,
            gumbel=gumbel, arena_opts=arena_opts, eval_cache_entries=eval_cache_entries, perpetual_check=perpetual_check,
            solver=solver, root_stats=root_stats, eval_mirror=eval_mirror, record_games=record_games, max_out_games=max_out_games,
            eval_dedup=eval_dedup)
        K, flags, cap, forced, gz, ar = opts
        rules, sv, rs, em, gr = opts.rules, opts.solver, opts.root_stats, opts.eval_mirror, opts.game_records
        if em is not None and not getattr(evaluator, "live_rows", False):
            raise hip.XqError("eval_mirror acts in the packed step only: it needs an evaluator with live_rows (the HIP evaluators)")
        if opts.eval_dedup and not getattr(evaluator, "live_rows", False):
            raise hip.XqError("eval_dedup acts in the packed step only: it needs an evaluator with live_rows (the HIP evaluators)")
        pool = parse_start_pool(cfg, start_pool, record_games=gr is not None)
        self.early_stop = parse_early_stop(cfg, early_stop, leaves_per_step=K, tree_reuse=tree_reuse, playout_cap=cap,
                                           forced_playouts=forced, gumbel=gz, solver=sv is not None)
        adj = parse_adjudicate(cfg, adjudicate)
        if not torch.cuda.is_available():
            raise hip.XqError("SelfPlayEngine needs a GPU: the HIP engine has no CPU fallback")
        self.lib = hip.lib()
        self.device = torch.device(device)
        sp = None
        if pool is not None:
            # the pool on the device, checked there: the first entry the rules code cannot run on is named
            pb, ps = (a.to(self.device).contiguous() if isinstance(a, torch.Tensor) else torch.from_numpy(a).to(self.device)
                      for a in pool[:2])
            with torch.cuda.device(self.device):
                status = hip.positions_check(pb, ps).cpu().numpy()
            bad = np.flatnonzero(status & hip.POSITION_FATAL)
            if len(bad):
                raise hip.XqError(f"start_pool: row {int(bad[0])} is no position the rules can run on (positions_check bits "
                                  f"{int(status[bad[0]])}; {len(bad)} of {len(status)} rows are refused)")
            sp = hip.StartPool(pb.data_ptr(), ps.data_ptr(), len(status), 0, pool[2])
        self.start_pool = None if sp is None else (int(sp.n), float(sp.prob))
        self.cfg = cfg
        self.G = cfg.n_games
        self.K = K
        self.tree_reuse = bool(flags & hip.ENGINE_TREE_REUSE)
        self.playout_cap = None if cap is None else (cap.full_search_prob, cap.fast_simulations)
        self.forced_playouts = None if forced is None else float(np.float32(forced.k))   # k as the kernels use it
        self.gumbel = None if gz is None else (gz.considered, float(np.float32(gz.c_visit)), float(np.float32(gz.c_scale)))
        self.arena_opts = None if ar is None else (ar.opening_plies, ar.first_game)
        self.perpetual_check = rules is not None
        self.solver = sv is not None
        self.root_stats = rs is not None
        self.eval_mirror = em is not None
        self.record_games = gr is not None
        self.max_out_games = 0 if gr is None else int(gr.max_out_games)
        self.rows = self.G * K                         # request rows: slot-major, row slot * K + j
        self.evaluator = evaluator
        # every entry point is the widest one with NULL for the options it does not take (include/xq_hip.h)
        refs = [None if o is None else C.byref(o) for o in (cap, forced, gz, ar, rules, sv, rs, em, gr, sp)]
        nbytes = self.lib.xq_engine_workspace_bytes_sp(C.byref(cfg), K, flags, *refs)
        if nbytes == 0:
            raise hip.XqError("invalid engine configuration")
        self.workspace_bytes = int(nbytes)
        self._words = hip.OptionWords()                # where the options' device words lie behind the square-root table
        hip.check(self.lib.xq_engine_option_words_sp(C.byref(cfg), K, flags, *refs, C.byref(self._words)), "xq_engine_option_words_sp")
        self.ws = torch.empty(self.workspace_bytes + 256, dtype=torch.uint8, device=self.device)
        base = (self.ws.data_ptr() + 255) & ~255
        self._inject = None
        inj_ptr = None
        if cfg.inject_len > 0:
            inj = np.ascontiguousarray(inject, dtype=np.uint64)
            assert inj.shape == (self.G, 4, cfg.inject_len)
            self._inject = torch.from_numpy(inj.view(np.int64)).to(self.device)
            inj_ptr = self._inject.data_ptr()
        self.h = hip.Engine()
        self.nn_input = torch.zeros((self.rows, 15, 10, 9), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            hip.check(self.lib.xq_engine_init_sp(C.byref(self.h), C.byref(cfg), K, flags, *refs, base, self.workspace_bytes, inj_ptr,
                                                 hip.stream_ptr(self.device)), "xq_engine_init_sp")
        self._start_index = None
        if sp is not None:                             # init copied the pool into the workspace: pb and ps may go
            pi = C.c_void_p()
            hip.check(self.lib.xq_engine_start_indices(C.byref(self.h), C.byref(pi)), "xq_engine_start_indices")
            self._start_index = self._ws_view(pi.value, self.G, torch.int32)
        # zero-copy int32 view of the per-slot state words (columns hip.GI_*: side to move of the REAL game, move_count, phase,
        # simulations done): host-side policies such as the arena's model choice read it between stages
        self.slot_ints = self._ws_view(self.h.p[hip.P_GI], (self.G, 32), torch.int32)
        # sparse hand-off to the evaluator (xq_engine_requests): ordered legal moves + their number per pending evaluation
        pm, pc = C.c_void_p(), C.c_void_p()
        hip.check(self.lib.xq_engine_requests(C.byref(self.h), C.byref(pm), C.byref(pc)), "xq_engine_requests")
        self.req_moves = self._ws_view(pm.value, (self.rows, hip.MAXM), torch.int16)
        self.req_counts = self._ws_view(pc.value, self.rows, torch.int32)
        # packed-step buffers (xq_engine_packed): live count, row -> slot map, packed planes / requests, slot-ordered hand-back
        pb = hip.PackedBuffers()
        hip.check(self.lib.xq_engine_packed(C.byref(self.h), C.byref(pb)), "xq_engine_packed")
        G, view = self.rows, self._ws_view              # packed buffers hold request rows (= slots when K = 1)
        self.n_live = view(pb.n_live, 1, torch.int32)
        self.packed_rows = view(pb.rows, G, torch.int32)
        self.packed_x = view(pb.x, (G, 15, 10, 9), torch.float32)
        self.packed_moves = view(pb.moves, (G, hip.MAXM), torch.int16)
        self.packed_counts = view(pb.counts, G, torch.int32)
        self.slot_logits = view(pb.slot_logits, (G, hip.MAXM), torch.float32)
        self.slot_value = view(pb.slot_value, G, torch.float32)
        self.arena_packed = None
        if ar is not None:
            # the per-model packed step's two buffer sets (xq_engine_packed_arena) and the openings record
            pbs = (hip.PackedBuffers * 2)()
            hip.check(self.lib.xq_engine_packed_arena(C.byref(self.h), pbs), "xq_engine_packed_arena")
            self.arena_packed = tuple(dict(
                n_live=view(b.n_live, 1, torch.int32), rows=view(b.rows, G, torch.int32), x=view(b.x, (G, 15, 10, 9), torch.float32),
                moves=view(b.moves, (G, hip.MAXM), torch.int16), counts=view(b.counts, G, torch.int32)) for b in pbs)
            pa, pc = C.c_void_p(), C.c_void_p()
            hip.check(self.lib.xq_engine_arena_openings(C.byref(self.h), C.byref(pa), C.byref(pc)), "xq_engine_arena_openings")
            self._opening_actions = view(pa.value, (G, hip.ARENA_MAX_OPENING), torch.int16)
            self._opening_counts = view(pc.value, G, torch.int32)
        self.cache = None
        if eval_cache_entries:
            self._init_cache(int(eval_cache_entries))
        self.eval_dedup = bool(opts.eval_dedup)
        self.dedup = hip.DedupTable(self.G, self.device) if self.eval_dedup else None
        # settled-move cutoff: xq_engine_settle's counters, one row per slot (searches settled, simulations not run)
        self._settle_counters = torch.zeros((self.G, 2), dtype=torch.int64, device=self.device) if self.early_stop else None
        # table adjudication: the tables' device words, xq_engine_adjudicate's options and counters, one row per slot (games ended
        # decisive, drawn, covered but left alone, matched through the swapped colours)
        self.adjudicate_tables = None
        if adj is not None:
            tabs = []
            for tb in adj[0]:
                t = tb.device_table()
                if t.device != self.ws.device:
                    raise hip.XqError(f"adjudicate: the table of {tb.signature!r} is on {t.device}, the engine on {self.ws.device}")
                tabs.append((tb.codes, t))
            self.adjudicate_tables, self._adjudicate_opts = tuple(tabs), adj[1]
            self._adjudicate_counters = torch.zeros((self.G, 4), dtype=torch.int64, device=self.device)
        # per-side resign rule: xq_engine_resign's options, per-slot state, holdout rows with their counter, and counters, one row
        # per slot (games resigned, holdout games closed, rows dropped, values seen)
        self.resign = None
        if rsn is not None:
            self._resign_opts, self._resign_max_rows = rsn
            self.resign = dict(threshold=float(rsn[0].threshold), check_steps=int(rsn[0].check_steps),
                               holdout_prob=float(rsn[0].holdout_prob), max_rows=int(rsn[1]))
            self._resign_state = torch.zeros(int(self.lib.xq_resign_state_bytes(self.G)), dtype=torch.uint8, device=self.device)
            self._resign_rows = torch.zeros((max(1, rsn[1]), hip.RESIGN_ROW_BYTES), dtype=torch.uint8, device=self.device)
            self._resign_row_count = torch.zeros(1, dtype=torch.int32, device=self.device)
            self._resign_counters = torch.zeros((self.G, 4), dtype=torch.int64, device=self.device)
        self._reuse_seen = (self.evaluator, getattr(self.evaluator, "weights_version", 0))
        self.steps = 0
        self._graph = None
        self._graph_generation = 0
        self.launch_mode = "eager"                     # "graph" once capture_step has recorded a step
        self.capture_error = None

    def _init_cache(self, entries: int):
        if not getattr(self.evaluator, "live_rows", False):
            raise hip.XqError("eval_cache_entries needs an evaluator with live_rows (the HIP evaluators): the cached step "
                              "evaluates the packed misses")
        nbytes = eval_cache_bytes(self.G, entries)
        if nbytes == 0:
            raise hip.XqError(f"eval_cache_entries must be a positive power of two, got {entries}")
        self.cache_entries = entries
        self.cache_bytes = nbytes
        self.cache_ws = torch.empty(nbytes + 256, dtype=torch.uint8, device=self.device)
        self.cache = hip.EvCache()
        with torch.cuda.device(self.device):
            hip.check(self.lib.xq_evcache_init(C.byref(self.cache), self.G, entries, (self.cache_ws.data_ptr() + 255) & ~255,
                                               nbytes, hip.stream_ptr(self.device)), "xq_evcache_init")
        hf = C.c_void_p()
        hip.check(self.lib.xq_evcache_hit_flags(C.byref(self.cache), C.byref(hf)), "xq_evcache_hit_flags")
        self._cache_hit_ptr = int(hf.value)
        self._cache_seen = (self.evaluator, getattr(self.evaluator, "weights_version", 0))

    def _sync_cache(self):
        """Invalidate the evaluation cache (a device-side generation bump, outside any recorded graph) when the evaluator or
        its weights changed since the cache last saw them: stale hits are the one way the cache could alter the games."""
        seen = (self.evaluator, getattr(self.evaluator, "weights_version", 0))
        if seen[0] is not self._cache_seen[0] or seen[1] != self._cache_seen[1]:
            hip.check(self.lib.xq_evcache_invalidate(C.byref(self.cache), hip.stream_ptr(self.device)), "xq_evcache_invalidate")
            self._cache_seen = seen

    def drop_reroots(self):
        """Tree reuse: no slot keeps its tree at the end of the move it is searching now (xq_engine_drop_reroots, one
        device-side word per slot; asynchronous).  For trees grown partly under weights that have since changed."""
        hip.check(self.lib.xq_engine_drop_reroots(C.byref(self.h), hip.stream_ptr(self.device)), "xq_engine_drop_reroots")

    def _sync_reuse(self):
        """Drop the pending re-roots (outside any recorded graph) when the evaluator or its weights changed since the engine
        last saw them: a kept subtree would carry the old network's priors and values into the next search."""
        seen = (self.evaluator, getattr(self.evaluator, "weights_version", 0))
        if seen[0] is not self._reuse_seen[0] or seen[1] != self._reuse_seen[1]:
            self.drop_reroots()
            self._reuse_seen = seen

    # ---- the three stages of a step --------------------------------------------------------------------
    def select(self):
        if self.early_stop:                            # ahead of the select kernel, which ends the settled arena searches
            hip.check(self.lib.xq_engine_settle(C.byref(self.h), self._settle_counters.data_ptr(), hip.stream_ptr(self.device)),
                      "xq_engine_settle")
        if self.resign is not None:                    # behind the last expand kernel, ahead of the kernels that flush a finished game
            self.resign_stage()
        hip.check(self.lib.xq_engine_select(C.byref(self.h), self.nn_input.data_ptr(), hip.stream_ptr(self.device)),
                  "xq_engine_select")
        if self.adjudicate_tables is not None:         # behind the select kernel's root requests, ahead of every expand kernel
            self.adjudicate()
        return self.nn_input

    def adjudicate(self):
        """After `select`, ahead of the expand call: end every game whose real position one of the tables decides
        (xq_engine_adjudicate, once per table, in order; a slot an earlier table decided is skipped by the later ones).  `select()`
        calls it; public for callers that drive the stages themselves.  Asynchronous."""
        if self.adjudicate_tables is None:
            raise hip.XqError("adjudicate needs an engine with adjudicate=")
        for codes, table in self.adjudicate_tables:
            hip.engine_adjudicate(self.h, codes, table, self._adjudicate_opts, self._adjudicate_counters)

    def resign_stage(self):
        """Ahead of `select`: update every slot's levels from the root value the last expand call recorded, end the games the
        per-side rule resigns and write the row of every finished holdout game (xq_engine_resign).  `select()` calls it; public
        for callers that drive the stages themselves.  Asynchronous."""
        if self.resign is None:
            raise hip.XqError("resign_stage needs an engine with resign=")
        hip.check(self.lib.xq_engine_resign(C.byref(self.h), C.byref(self._resign_opts), self._resign_state.data_ptr(),
                                            self._resign_rows.data_ptr(), self._resign_max_rows, self._resign_row_count.data_ptr(),
                                            self._resign_counters.data_ptr(), hip.stream_ptr(self.device)), "xq_engine_resign")

    def set_resign_threshold(self, threshold: float):
        """Play on under another threshold (a calibrated one): a kernel argument, so a recorded step is released."""
        if self.resign is None:
            raise hip.XqError("set_resign_threshold needs an engine with resign=")
        self._resign_opts = hip.resign_opts(threshold, self.resign["check_steps"], self.resign["holdout_prob"], what="resign")
        self.resign["threshold"] = float(self._resign_opts.threshold)
        if self._graph is not None:
            self.release_graph()

    def expand(self, policy: torch.Tensor, value: torch.Tensor, is_probs: bool = False):
        if policy.dtype != torch.float32 or value.dtype != torch.float32:
            raise hip.XqError("policy/value must be float32")
        policy = policy.contiguous()
        value = value.contiguous().view(-1)
        if policy.shape != (self.rows, hip.ACTION_SPACE) or value.shape != (self.rows,):
            raise hip.XqError(f"bad evaluator output shapes {tuple(policy.shape)} {tuple(value.shape)}")
        hip.check(self.lib.xq_engine_expand(C.byref(self.h), policy.data_ptr(), value.data_ptr(), int(is_probs),
                                            hip.stream_ptr(self.device)), "xq_engine_expand")
        self._keep = (policy, value)   # keep alive until the stream has consumed them

    def expand_legal(self, legal_logits: torch.Tensor, value: torch.Tensor):
        """Expansion from the logits of the ORDERED LEGAL MOVES only (float32[G, 128], xq_engine_expand_legal)."""
        if legal_logits.dtype != torch.float32 or value.dtype != torch.float32:
            raise hip.XqError("legal_logits/value must be float32")
        legal_logits = legal_logits.contiguous()
        value = value.contiguous().view(-1)
        if legal_logits.shape != (self.rows, hip.MAXM) or value.shape != (self.rows,):
            raise hip.XqError(f"bad evaluator output shapes {tuple(legal_logits.shape)} {tuple(value.shape)}")
        hip.check(self.lib.xq_engine_expand_legal(C.byref(self.h), legal_logits.data_ptr(), value.data_ptr(),
                                                  hip.stream_ptr(self.device)), "xq_engine_expand_legal")
        self._keep = (legal_logits, value)

    def evaluate_and_expand(self, x: torch.Tensor, evaluator=None):
        """Evaluator -> expansion in the evaluator's own protocol: one that offers `evaluate_legal(x, moves, counts)`
        (the hand-written evaluator) is asked for the legal moves' logits only; any other callable returns the dense
        [G, 8100] logits row of the reference protocol."""
        ev = evaluator if evaluator is not None else self.evaluator
        if hasattr(ev, "evaluate_legal"):
            ll, value = ev.evaluate_legal(x, self.req_moves, self.req_counts)
            self.expand_legal(ll, value)
        else:
            logits, value = ev(x)
            self.expand(logits, value, False)

    def compact(self):
        """After `select`: pack the slots waiting for an evaluation (xq_engine_compact) into `packed_x`, `packed_moves`,
        `packed_counts` (rows [0, n_live) valid, slot order; `packed_rows[r]` is row r's slot).  Asynchronous."""
        hip.check(self.lib.xq_engine_compact(C.byref(self.h), self.nn_input.data_ptr(), hip.stream_ptr(self.device)),
                  "xq_engine_compact")

    def expand_packed(self, legal_logits: torch.Tensor, value: torch.Tensor):
        """Expansion from PACKED evaluator outputs (rows [0, n_live) of float32[G, 128] / [G]): scattered back to
        `slot_logits` / `slot_value` in slot order, then xq_engine_expand_legal (xq_engine_expand_packed)."""
        if legal_logits.dtype != torch.float32 or value.dtype != torch.float32:
            raise hip.XqError("legal_logits/value must be float32")
        legal_logits = legal_logits.contiguous()
        value = value.contiguous().view(-1)
        if legal_logits.shape != (self.rows, hip.MAXM) or value.shape != (self.rows,):
            raise hip.XqError(f"bad evaluator output shapes {tuple(legal_logits.shape)} {tuple(value.shape)}")
        hip.check(self.lib.xq_engine_expand_packed(C.byref(self.h), legal_logits.data_ptr(), value.data_ptr(),
                                                   hip.stream_ptr(self.device)), "xq_engine_expand_packed")
        self._keep = (self.slot_logits, self.slot_value)    # slot-ordered, as the full-width step's (bench.py --dump-outputs)
        self._keep_packed = (legal_logits, value)          # keep alive until the stream has consumed them

    def expand_dedup(self, legal_logits: torch.Tensor, value: torch.Tensor):
        """Expansion from the PACKED outputs of the dedup step (rows [0, n_live): the representatives'): every waiting slot
        takes its representative's row into `slot_logits` / `slot_value`, then xq_engine_expand_legal (xq_engine_expand_dedup)."""
        if self.dedup is None:
            raise hip.XqError("expand_dedup needs an engine with eval_dedup=True")
        if legal_logits.dtype != torch.float32 or value.dtype != torch.float32:
            raise hip.XqError("legal_logits/value must be float32")
        legal_logits = legal_logits.contiguous()
        value = value.contiguous().view(-1)
        if legal_logits.shape != (self.rows, hip.MAXM) or value.shape != (self.rows,):
            raise hip.XqError(f"bad evaluator output shapes {tuple(legal_logits.shape)} {tuple(value.shape)}")
        hip.check(self.lib.xq_engine_expand_dedup(C.byref(self.dedup.h), C.byref(self.h), legal_logits.data_ptr(), value.data_ptr(),
                                                  hip.stream_ptr(self.device)), "xq_engine_expand_dedup")
        self._keep = (self.slot_logits, self.slot_value)
        self._keep_packed = (legal_logits, value)          # keep alive until the stream has consumed them

    # ---- arena options (xq_engine_init_ar) -----------------------------------------------------------------
    def _need_arena_opts(self, what: str):
        if self.arena_packed is None:
            raise hip.XqError(f"{what} needs an engine with arena_opts=")

    def compact_arena(self):
        """After `select`: pack the waiting slots into the two sets of `arena_packed` (xq_engine_compact_arena): [0] the slots the
        new model searches for, [1] the old model's; per set `n_live`, `rows`, `x`, `moves`, `counts`.  Asynchronous."""
        self._need_arena_opts("compact_arena")
        hip.check(self.lib.xq_engine_compact_arena(C.byref(self.h), self.nn_input.data_ptr(), hip.stream_ptr(self.device)),
                  "xq_engine_compact_arena")

    def expand_packed_arena(self, logits_new: torch.Tensor, value_new: torch.Tensor, logits_old: torch.Tensor,
                            value_old: torch.Tensor):
        """Expansion from the two models' PACKED outputs (rows [0, n_live) of float32[G, 128] / [G] each, over set 0 and set 1):
        scattered back to `slot_logits` / `slot_value`, then xq_engine_expand_legal (xq_engine_expand_packed_arena)."""
        self._need_arena_opts("expand_packed_arena")
        keep = []
        for ll, v in ((logits_new, value_new), (logits_old, value_old)):
            if ll.dtype != torch.float32 or v.dtype != torch.float32:
                raise hip.XqError("legal_logits/value must be float32")
            ll, v = ll.contiguous(), v.contiguous().view(-1)
            if ll.shape != (self.rows, hip.MAXM) or v.shape != (self.rows,):
                raise hip.XqError(f"bad evaluator output shapes {tuple(ll.shape)} {tuple(v.shape)}")
            keep += [ll, v]
        hip.check(self.lib.xq_engine_expand_packed_arena(C.byref(self.h), keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr(),
                                                         keep[3].data_ptr(), hip.stream_ptr(self.device)),
                  "xq_engine_expand_packed_arena")
        self._keep = (self.slot_logits, self.slot_value)
        self._keep_packed = tuple(keep)                    # keep alive until the stream has consumed them

    def arena_openings(self):
        """-> (actions uint16 [G, 16], counts int32 [G]) on the host: what every slot played as its opening (zero past its count;
        count 0 before the game started, after the restart rule and with opening_plies = 0).  Synchronises."""
        self._need_arena_opts("arena_openings")
        return self._opening_actions.cpu().numpy().view(np.uint16).copy(), self._opening_counts.cpu().numpy().copy()

    @property
    def path(self) -> str:
        """The step `step()` runs: "cached" with an evaluation cache, "dedup" with eval_dedup, "packed" when the evaluator
        evaluates a device-side live row count, else "full"."""
        if self.cache is not None:
            return "cached"
        if self.dedup is not None:
            return "dedup"
        return "packed" if getattr(self.evaluator, "live_rows", False) else "full"

    def _one_step(self):
        if self.cache is not None:
            sp = hip.stream_ptr(self.device)
            x = self.select()
            hip.check(self.lib.xq_evcache_probe(C.byref(self.cache), C.byref(self.h), x.data_ptr(), sp), "xq_evcache_probe")
            hip.check(self.lib.xq_engine_compact_misses(C.byref(self.h), x.data_ptr(), self._cache_hit_ptr, sp),
                      "xq_engine_compact_misses")
            ll, value = self.evaluator.evaluate_legal(self.packed_x, self.packed_moves, self.packed_counts, n_live=self.n_live)
            self.expand_packed(ll, value)
            ll, value = self._keep_packed                # checked float32 [G, 128] / [G], contiguous
            hip.check(self.lib.xq_evcache_commit(C.byref(self.cache), C.byref(self.h), ll.data_ptr(), value.data_ptr(), sp),
                      "xq_evcache_commit")
        elif self.dedup is not None:
            if not getattr(self.evaluator, "live_rows", False):    # the evaluator was swapped: an error, not a silent full-width step
                raise hip.XqError("eval_dedup needs the packed step: the evaluator has no live_rows")
            sp = hip.stream_ptr(self.device)
            x = self.select()
            hip.check(self.lib.xq_engine_compact_unique(C.byref(self.dedup.h), C.byref(self.h), x.data_ptr(), sp),
                      "xq_engine_compact_unique")
            ll, value = self.evaluator.evaluate_legal(self.packed_x, self.packed_moves, self.packed_counts, n_live=self.n_live)
            self.expand_dedup(ll, value)
        elif self.path == "packed":
            self.select()
            self.compact()
            ll, value = self.evaluator.evaluate_legal(self.packed_x, self.packed_moves, self.packed_counts, n_live=self.n_live)
            self.expand_packed(ll, value)
        else:
            if self.eval_mirror:                       # the full-width step never mirrors: an error, not a silent no-op
                raise hip.XqError("eval_mirror needs the packed step: the evaluator has no live_rows")
            self.evaluate_and_expand(self.select())

    def step(self):
        """select -> evaluator -> expand, all asynchronous on the current stream (one graph launch once `capture_step`
        has recorded it); the packed step (module docstring) when the evaluator has `live_rows`."""
        if self._graph is not None and getattr(self.evaluator, "generation", 0) != self._graph_generation:
            self.release_graph()                       # the evaluator reallocated a buffer: the recording holds stale pointers
        if self.cache is not None:
            self._sync_cache()
        if self.tree_reuse:
            self._sync_reuse()
        if self._graph is not None:
            self._graph.replay()
        else:
            self._one_step()
        self.steps += 1

    def capture_step(self, warmup: int = 2) -> bool:
        """Record one step (xq_engine_select, every evaluator kernel, xq_engine_expand[_legal]) into a HIP graph and make
        `step()` replay it: one launch per step instead of ~2B+8 launches issued from Python.  All kernel arguments of a
        step are constants of the engine (the workspace, the evaluator's persistent buffers), so the recording stays valid
        until the evaluator's weights are replaced (`release_graph()` then).  Matters where steps are short: at BASELINE
        configs[1] (1024 games, 128x6) the launches of an eager step leave the GPU idle for ~17 % of it; at configs[2] a
        step is 52 ms and the gain is nil.  `warmup` eager steps run first (allocations, function attributes).  Returns
        False, and stays eager, for evaluators that are not capturable (they synchronise or allocate outside torch)."""
        if self.evaluator is None:
            raise hip.XqError("capture_step needs an evaluator")
        if self.cache is not None:
            self._sync_cache()
        if self.tree_reuse:
            self._sync_reuse()
        for _ in range(warmup):
            self._one_step()
            self.steps += 1
        torch.cuda.synchronize(self.device)
        g = torch.cuda.CUDAGraph()
        try:
            # thread_local: other threads of the process (the RCCL watchdog of a multi-rank run polls events) must not
            # invalidate the capture
            with torch.cuda.graph(g, capture_error_mode="thread_local"):
                self._one_step()
        except hip.XqError:
            raise                                      # argument / shape / launch errors of our own entry points: never hidden
        except RuntimeError as e:
            # ONLY "this evaluator cannot be recorded" (it synchronises, allocates outside torch's pool or launches on
            # another stream while the stream is capturing) keeps the engine eager; anything else is a real error
            msg = str(e).lower()
            if not any(k in msg for k in ("captur", "hiperrorstreamcapture", "cudaerrorstreamcapture", "operation not permitted")):
                raise
            torch.cuda.synchronize(self.device)
            self.launch_mode, self.capture_error = "eager", str(e).splitlines()[0][:200]
            return False
        self._graph = g
        self._graph_generation = getattr(self.evaluator, "generation", 0)
        self.launch_mode = "graph"
        return True

    def release_graph(self):
        self._graph = None
        self.launch_mode = "eager"

    # ---- bookkeeping --------------------------------------------------------------------------------------
    def stats(self, check: bool = True) -> dict:
        s = hip.EngineStats()
        rc = self.lib.xq_engine_stats_read(C.byref(self.h), C.byref(s), hip.stream_ptr(self.device))
        if rc != 0 and (check or rc != -4):
            hip.check(rc, "xq_engine_stats_read")
        out = s.as_dict()
        if self.solver:
            out.update(self.solver_stats())
        if self.cache is not None:
            cs = hip.EvCacheStats()
            hip.check(self.lib.xq_evcache_stats_read(C.byref(self.cache), C.byref(cs), hip.stream_ptr(self.device)),
                      "xq_evcache_stats_read")
            out.update({"eval_cache_" + k: v for k, v in cs.as_dict().items()})
            out["eval_cache_entries"] = self.cache_entries
            out["eval_cache_bytes"] = self.cache_bytes
        if self.dedup is not None:
            out.update({"eval_dedup_" + k: v for k, v in self.dedup.stats().items()})
        return out

    def early_stop_stats(self) -> dict:
        """The settled-move cutoff's counters: settled_moves (searches ended before their budget) and simulations_saved (the
        simulations they did not run).  Synchronises."""
        if not self.early_stop:
            raise hip.XqError("early_stop_stats needs an engine with early_stop=True")
        s = self._settle_counters.sum(dim=0).cpu()
        return dict(settled_moves=int(s[0]), simulations_saved=int(s[1]))

    def adjudication_stats(self) -> dict:
        """Table adjudication's counters: adjudicated_decisive and adjudicated_drawn (games a table ended), adjudicated_left_alone
        (root positions a table covers as drawn while draws is off) and adjudicated_swapped (matched through the colour-swapped
        image, among all three).  Synchronises."""
        if self.adjudicate_tables is None:
            raise hip.XqError("adjudication_stats needs an engine with adjudicate=")
        s = self._adjudicate_counters.sum(dim=0).cpu()
        return dict(adjudicated_decisive=int(s[0]), adjudicated_drawn=int(s[1]), adjudicated_left_alone=int(s[2]),
                    adjudicated_swapped=int(s[3]))

    def resign_stats(self) -> dict:
        """The per-side resign rule's counters: resigned (games it ended), holdout_games (exempt games that finished),
        rows_dropped (their rows that found the row array full) and values_seen, with the threshold in use.  Synchronises."""
        if self.resign is None:
            raise hip.XqError("resign_stats needs an engine with resign=")
        s = self._resign_counters.sum(dim=0).cpu()
        return dict(resigned=int(s[0]), holdout_games=int(s[1]), rows_dropped=int(s[2]), values_seen=int(s[3]),
                    threshold=self.resign["threshold"])

    def drain_resign_rows(self) -> np.ndarray:
        """-> the rows of the holdout games finished since the last call (sample_format.RESIGN_ROW_DTYPE, sorted by slot and
        game_seq, at most max_rows); empties the row array.  Synchronises; call it between steps."""
        if self.resign is None:
            raise hip.XqError("drain_resign_rows needs an engine with resign=")
        n = min(int(self._resign_row_count.item()), self._resign_max_rows)
        rows = self._resign_rows[:n].cpu().numpy().reshape(-1).view(hip.RESIGN_ROW_DTYPE).copy()
        self._resign_row_count.zero_()
        return rows[np.lexsort((rows["game_seq"], rows["slot"]))]

    def solver_stats(self) -> dict:
        """The proven-result search's counters (xq_engine_solver_stats_read): proven_nodes, proven_stops, proven_moves,
        unspent_sims, removed_visits.  Synchronises."""
        if not self.solver:
            raise hip.XqError("solver_stats needs an engine with solver=True")
        s = hip.SolverStats()
        hip.check(self.lib.xq_engine_solver_stats_read(C.byref(self.h), C.byref(s), hip.stream_ptr(self.device)),
                  "xq_engine_solver_stats_read")
        return s.as_dict()

    def read_root_states(self, slot: int) -> dict:
        """The proven states at the root of `slot`, from the view of the side to move there (xq_engine_read_root_states):
        `children` int8 per legal move in move order (+1 the move wins, -1 it loses, 2 draw, 0 unknown) and `root` in the same
        code.  Synchronises."""
        if not self.solver:
            raise hip.XqError("read_root_states needs an engine with solver=True")
        cs = np.zeros(hip.MAXM, dtype=np.int8)
        rs = np.zeros(1, dtype=np.int8)
        n = self.lib.xq_engine_read_root_states(C.byref(self.h), int(slot), cs.ctypes.data, rs.ctypes.data,
                                                hip.stream_ptr(self.device))
        if n < 0:
            hip.check(n, "xq_engine_read_root_states")
        return dict(children=cs[:n].copy(), root=int(rs[0]))

    def drain(self):
        """-> (samples structured array, results structured array); empties the device rings."""
        smp = np.zeros(self.cfg.max_out_samples, dtype=SAMPLE_DTYPE)
        res = np.zeros(self.cfg.max_out_results, dtype=RESULT_DTYPE)
        ns, nr = C.c_int(), C.c_int()
        hip.check(self.lib.xq_engine_drain(C.byref(self.h), smp.ctypes.data, len(smp), C.byref(ns), res.ctypes.data,
                                           len(res), C.byref(nr), hip.stream_ptr(self.device)), "xq_engine_drain")
        return smp[:ns.value].copy(), res[:nr.value].copy()

    def drain_device(self):
        """-> (samples uint8[n, 640], results uint8[m, 16]) as DEVICE tensors (xq_engine_drain_device); empties the rings.
        View them with `.cpu().numpy().view(SAMPLE_DTYPE / RESULT_DTYPE)` where host records are wanted."""
        ns, nr = C.c_int(), C.c_int()
        sp = hip.stream_ptr(self.device)
        hip.check(self.lib.xq_engine_drain_device(C.byref(self.h), None, 0, C.byref(ns), None, 0, C.byref(nr), sp),
                  "xq_engine_drain_device")
        smp = torch.empty((ns.value, hip.SAMPLE_BYTES), dtype=torch.uint8, device=self.device)
        res = torch.empty((nr.value, hip.RESULT_BYTES), dtype=torch.uint8, device=self.device)
        if ns.value or nr.value:
            hip.check(self.lib.xq_engine_drain_device(C.byref(self.h), smp.data_ptr() if ns.value else None, ns.value, C.byref(ns),
                                                      res.data_ptr() if nr.value else None, nr.value, C.byref(nr), sp),
                      "xq_engine_drain_device")
        return smp, res

    def drain_games(self) -> np.ndarray:
        """-> the records of the games finished since the last call (hip.GAME_RECORD_DTYPE, in the order they finished, at most
        max_out_games); empties the record ring only (xq_engine_drain_games).  Needs record_games=True."""
        if not self.record_games:
            raise hip.XqError("drain_games needs an engine with record_games=True")
        n = C.c_int()
        sp = hip.stream_ptr(self.device)
        hip.check(self.lib.xq_engine_drain_games(C.byref(self.h), None, 0, C.byref(n), sp), "xq_engine_drain_games")
        rec = np.zeros(n.value, dtype=hip.GAME_RECORD_DTYPE)
        if n.value:
            hip.check(self.lib.xq_engine_drain_games(C.byref(self.h), rec.ctypes.data, len(rec), C.byref(n), sp),
                      "xq_engine_drain_games")
        return rec[:n.value]

    def drain_games_device(self) -> torch.Tensor:
        """-> the same records as a DEVICE tensor uint8[n, 1024] (xq_engine_drain_games_device), what `replay_games` takes."""
        if not self.record_games:
            raise hip.XqError("drain_games_device needs an engine with record_games=True")
        n = C.c_int()
        sp = hip.stream_ptr(self.device)
        hip.check(self.lib.xq_engine_drain_games_device(C.byref(self.h), None, 0, C.byref(n), sp), "xq_engine_drain_games_device")
        rec = torch.empty((n.value, hip.RECORD_BYTES), dtype=torch.uint8, device=self.device)
        if n.value:
            hip.check(self.lib.xq_engine_drain_games_device(C.byref(self.h), rec.data_ptr(), n.value, C.byref(n), sp),
                      "xq_engine_drain_games_device")
        return rec[:n.value]

    def _ws_view(self, addr, shape, dtype) -> torch.Tensor:
        """Zero-copy view of the workspace from device address `addr` on: `shape` (an int or a tuple) elements of `dtype`."""
        shape = (shape,) if isinstance(shape, int) else tuple(shape)
        off = int(addr) - int(self.ws.data_ptr())
        nbytes = math.prod(shape) * torch.empty(0, dtype=dtype).element_size()
        return self.ws[off:off + nbytes].view(dtype).view(shape)

    def _words_view(self, block, shape, dtype) -> torch.Tensor:
        """_ws_view of one block of the option words (hip.OptionWords), which lie in the square-root table's region."""
        return self._ws_view(int(self.h.p[hip.P_SQRT]) + int(block.offset), shape, dtype)

    def game_records_stats(self) -> dict:
        """recorded: games whose record found a row of the ring; dropped: games that finished on a full ring."""
        if not self.record_games:
            raise hip.XqError("game_records_stats needs an engine with record_games=True")
        s = hip.GameRecordsStats()
        hip.check(self.lib.xq_engine_game_records_stats_read(C.byref(self.h), C.byref(s), hip.stream_ptr(self.device)),
                  "xq_engine_game_records_stats_read")
        return dict(recorded=int(s.recorded), dropped=int(s.dropped))

    def start_indices(self) -> np.ndarray:
        """-> int32[G] on the host: the pool entry every slot's current game started from, -1 for the initial position (and
        before the slot's first game).  Synchronises.  Needs start_pool=."""
        if self._start_index is None:
            raise hip.XqError("start_indices needs an engine with start_pool=")
        return self._start_index.cpu().numpy().copy()

    def start_pool_stats(self) -> dict:
        """pool_games: the games started from a pool entry (xq_engine_start_pool_stats_read).  Synchronises."""
        if self._start_index is None:
            raise hip.XqError("start_pool_stats needs an engine with start_pool=")
        s = hip.StartPoolStats()
        hip.check(self.lib.xq_engine_start_pool_stats_read(C.byref(self.h), C.byref(s), hip.stream_ptr(self.device)),
                  "xq_engine_start_pool_stats_read")
        return dict(pool_games=int(s.pool_games))

    def game_record_views(self) -> dict:
        """Zero-copy views of the game records' words in the workspace (the tail of the option words, include/xq_hip.h): `ring`
        int16 [max_out_games, 512] (uint16 bits: 8 header words, then the moves), `log` int16 [G, 504] (the running games' moves
        so far) and `opening` int16 [G].  For tests and tools."""
        if not self.record_games:
            raise hip.XqError("game_record_views needs an engine with record_games=True")
        w = self._words
        return dict(ring=self._words_view(w.gr_ring, (self.max_out_games, hip.RECORD_BYTES // 2), torch.int16),
                    log=self._words_view(w.gr_log, (self.G, hip.RECORD_MAX_PLIES), torch.int16),
                    opening=self._words_view(w.gr_opening, self.G, torch.int16))

    def arena_views(self) -> dict:
        """Zero-copy torch views of the SoA tree arenas in the workspace, [G, node_cap] each:
        N int32, W float64, P float32, action int16 (uint16 bits), first int32 (first child, -1 = none), meta int16
        (uint16 bits: child count, mask hip.META_COUNT_MASK | proven state << 12 (solver=True only) | kind << 14), plus the root boards int8 [G, 96] (90 squares + pad).  For inspection and tests."""
        cap = int(self.h.node_cap)

        def view(idx, dtype, cols):
            return self._ws_view(self.h.p[idx], (self.G, cols), dtype)

        out = dict(N=view(hip.P_TN, torch.int32, cap), W=view(hip.P_TW, torch.float64, cap), P=view(hip.P_TP, torch.float32, cap),
                   action=view(hip.P_TA, torch.int16, cap), first=view(hip.P_TC, torch.int32, cap),
                   meta=view(hip.P_TM, torch.int16, cap), board=view(hip.P_BOARD, torch.int8, 96), node_cap=cap)
        if self.K > 1:
            out["vl"] = view(hip.P_VL, torch.int32, cap)     # virtual-loss counters: all 0 between steps
        return out

    def slot_counters(self) -> torch.Tensor:
        """Zero-copy int64 [G, 32] view of the per-slot counters that xq_engine_stats_read sums (column 19: collisions, 20:
        pending leaves handed out, 21: slot-steps that handed leaves, 22: reused visits, 23: re-rooted searches, 24: fast moves,
        25: simulations of fast searches, 26: forced simulations, 27: pruned visits, 28: pruned children, 29: Gumbel moves, 30: the sum
        of their considered moves, 31: Gumbel moves off the prior's first maximum).  For tests."""
        return self._ws_view(self.h.p[hip.P_STATS], (self.G, 32), torch.int64)

    def gumbel_root_values(self) -> torch.Tensor:
        """Gumbel engines: zero-copy float64 [G] view of v_hat, the root's network value every slot keeps for the end of its
        move (gz_vhat of the option words, include/xq_hip.h).  For tools and tests."""
        if self.gumbel is None:
            raise hip.XqError("gumbel_root_values needs an engine with gumbel=")
        return self._words_view(self._words.gz_vhat, self.G, torch.float64)

    def held(self) -> bool:
        """Search-only engines: every slot holds its finished search (phase HOLD).  Synchronises."""
        return bool((self.slot_ints[:, hip.GI_PHASE] == hip.PH_HOLD).all().item())

    # ---- MCTS.search for a given position (manual_moves engines; mcts.py:94-155) ---------------------------
    def set_position(self, slot: int, board, side: int, move_count: int = 0, no_capture: int = 0, hist12=None,
                     noise=None):
        b = np.ascontiguousarray(board, dtype=np.int8).reshape(90)
        h = None
        if hist12 is not None and len(hist12):
            h = np.zeros((12, 90), dtype=np.int8)
            hh = np.ascontiguousarray(hist12, dtype=np.int8).reshape(-1, 90)[-12:]
            h[:len(hh)] = hh
        nz = None
        if noise is not None:
            nz = np.zeros(hip.MAXM, dtype=np.float64)
            nz[:len(noise)] = noise
        hip.check(self.lib.xq_engine_set_position(
            C.byref(self.h), slot, b.ctypes.data, int(side), int(move_count), int(no_capture),
            None if h is None else h.ctypes.data, None if nz is None else nz.ctypes.data,
            hip.stream_ptr(self.device)), "xq_engine_set_position")

    def read_root(self, slot: int) -> dict:
        a = np.zeros(hip.MAXM, dtype=np.uint16)
        v = np.zeros(hip.MAXM, dtype=np.int32)
        w = np.zeros(hip.MAXM, dtype=np.float64)
        p = np.zeros(hip.MAXM, dtype=np.float64)
        kind, rv, sd = C.c_int(), C.c_int32(), C.c_int32()
        n = self.lib.xq_engine_read_root(C.byref(self.h), slot, a.ctypes.data, v.ctypes.data, w.ctypes.data,
                                         p.ctypes.data, C.byref(kind), C.byref(rv), C.byref(sd),
                                         hip.stream_ptr(self.device))
        if n < 0:
            hip.check(n, "xq_engine_read_root")
        return dict(actions=a[:n], visits=v[:n], total_value=w[:n], prior=p[:n], prior_is_f64=bool(kind.value),
                    prior_kind=int(kind.value), root_visits=rv.value, sims_done=sd.value)


def arena_engine(cfg: hip.EngineConfig, device, opening_plies: int, first_game: int, inject=None,
                 perpetual_check: bool = False, solver: bool = False, record_games: bool = False,
                 early_stop: bool = False, adjudicate=None) -> SelfPlayEngine:
    """The arena's engine with arena options (paired openings from game index `first_game`, the per-model packed step)."""
    return SelfPlayEngine(cfg, device, inject=inject, arena_opts=(int(opening_plies), int(first_game)),
                          perpetual_check=perpetual_check, solver=solver, record_games=record_games, early_stop=early_stop,
                          **({} if adjudicate is None else {"adjudicate": adjudicate}))


def replay_games(records, stop_ply=None, perpetual_check: bool = False, device="cuda") -> dict:
    """Replay game records on the device (xq_replay_games_batch, one wavefront per record).  `records`: a structured array of
    hip.GAME_RECORD_DTYPE (as `drain_games` returns) or a uint8 tensor [n, 1024] (as `drain_games_device` does); `stop_ply`: None
    (every move), one int for all records or one per record, clamped to [0, n_moves].  Returns a dict of device tensors:
    `status` (0: every requested ply was legal; k > 0: ply k - 1 is illegal and the outputs describe the position before it; -1:
    a malformed record), `board` int8[n, 90], `side`, `move_count`, `no_capture`, `hist12` int8[n, 12, 90] -- these five rows go
    straight into `set_position` or `MCTS` -- and `over_kind` (0 not over, 1 over, 4 over by the perpetual-check rule) with
    `winner` (2 while not over): the rules' verdict at the position reached."""
    if isinstance(records, torch.Tensor):
        rec = records.to(device)
    else:
        arr = np.ascontiguousarray(records)
        if arr.dtype != hip.GAME_RECORD_DTYPE:
            raise hip.XqError(f"replay_games: records must have hip.GAME_RECORD_DTYPE, got {arr.dtype}")
        rec = torch.from_numpy(arr.reshape(-1).view(np.uint8).reshape(-1, hip.RECORD_BYTES).copy()).to(device)
    rec = rec.contiguous()
    n = rec.shape[0]
    stop = None
    if stop_ply is not None:
        if isinstance(stop_ply, torch.Tensor):
            stop = stop_ply.to(device=rec.device, dtype=torch.int32).contiguous()
        else:
            stop = torch.from_numpy(np.broadcast_to(np.asarray(stop_ply, dtype=np.int32), (n,)).copy()).to(rec.device)
    with torch.cuda.device(rec.device):
        return hip.replay_games(rec, stop, perpetual_check)


action_probs_dense = dense_pi   # the reference's dense pi (mcts.py:190-206) from compact (action, visit) pairs
