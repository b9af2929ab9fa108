"""B3 -- the self-play operator behind the reference's own call shape.

    all_data, stats = parallel_self_play(model, config, num_workers=None, use_gpu_server=False, gpu_device='cuda')

Same arguments, return schema and stats keys as training/parallel_selfplay.py:264-334, so
`AlphaZeroTrainer._parallel_self_play` (training/train.py:313-327) can call it unchanged.  What runs underneath is
the device-resident engine (`engine.SelfPlayEngine`): all `num_games_per_iter` games advance concurrently on one
GPU, the network is evaluated on whole leaf batches, and nothing is pickled or sent over a socket.
`num_workers` / `use_gpu_server` are accepted for signature compatibility and only recorded in the stats.
"""
from __future__ import annotations

import time
from typing import Any, Dict, List, Optional, Tuple

import numpy as np

from . import engine, evaluator, hip
from .sample_format import to_reference_tuples

_CFG_KEYS = ("num_simulations", "c_puct", "temperature_threshold", "max_game_length", "random_opening_moves",
             "enable_resign", "resign_threshold", "resign_check_steps")     # parallel_selfplay.py:184-187


def root_stats_q_mix(config) -> float:
    """`config.value_target_q_mix` (a reference TrainingConfig has no such key: 0), checked: the share of the search's root value
    in the value target.  Above 0 it turns the recording of root statistics on and excludes Gumbel root search."""
    q_mix = float(getattr(config, "value_target_q_mix", 0.0) or 0.0)
    if not 0.0 <= q_mix <= 1.0:
        raise hip.XqError(f"config.value_target_q_mix must be in [0, 1], got {q_mix}")
    if q_mix > 0.0 and int(getattr(config, "gumbel_considered", 0) or 0):
        raise hip.XqError("config.value_target_q_mix > 0 needs root_stats, which cannot be combined with gumbel "
                          "(config.gumbel_considered): a Gumbel root's value is its own v_mix")
    return q_mix


def policy_surprise_weight(config) -> float:
    """`config.policy_surprise_weight` (a reference TrainingConfig has no such key: 0; None is the absent key), checked: alpha of
    the policy-surprise weighted epochs (training.train_network).  Above 0 it turns the scoring of the self-play samples on."""
    alpha = float(getattr(config, "policy_surprise_weight", 0.0) or 0.0)
    if not 0.0 <= alpha <= 1.0:
        raise hip.XqError(f"config.policy_surprise_weight must be in [0, 1], got {alpha}")
    return alpha


def score_samples(evaluator, samples_dev, late_temperature: float = 0.3, write_back: bool = True, chunk: int = 2048):
    """Score finished samples against a network: samples_dev uint8[n, 640] on the GPU (`SelfPlayEngine.drain_device`, a replay
    buffer's store) go through the evaluator once, `chunk` records at a time -- `hip.samples_to_requests`, the evaluator's
    `evaluate_legal`, `hip.score_samples` -- and come back as scores uint8[n, 16] on the device (sample_format.SCORE_DTYPE: KL and
    cross-entropy of the search target against the network's raw prior over the legal moves, the network's value, top-1
    agreement, valid).  `write_back` also marks the records in place (sample_format.policy_stats), which is what the
    policy-surprise weighted epochs of `training.train_network` read.  The evaluator that played the games reproduces the
    search's noise-free root prior; any other network answers "how well does it predict these samples".  `evaluate_legal`
    returns views of buffers it reuses: every chunk is consumed, on the evaluator's stream, before the next is issued.  An
    evaluator without `evaluate_legal` (the library comparison kinds) is refused."""
    import torch
    if not hasattr(evaluator, "evaluate_legal"):
        raise hip.XqError("score_samples needs an evaluator with evaluate_legal (kinds 'hip' and 'bf16'), got %s" % type(evaluator).__name__)
    chunk = int(chunk)
    if chunk < 1:
        raise hip.XqError(f"score_samples: chunk must be at least 1, got {chunk}")
    n, dev = samples_dev.shape[0], samples_dev.device
    scores = torch.zeros((n, hip.SCORE_BYTES), dtype=torch.uint8, device=dev)
    if n == 0:
        return scores
    width = min(chunk, n)
    x = torch.empty((width, 15, 10, 9), dtype=torch.float32, device=dev)
    moves = torch.empty((width, hip.MAXM), dtype=torch.int16, device=dev)
    counts = torch.empty(width, dtype=torch.int32, device=dev)
    for lo in range(0, n, width):
        b = min(width, n - lo)
        rows = samples_dev[lo:lo + b]
        hip.samples_to_requests(rows, None, out=(x[:b], moves[:b], counts[:b]))
        ll, v = evaluator.evaluate_legal(x[:b], moves[:b], counts[:b])
        hip.score_samples(rows, None, ll[:b], v[:b], late_temperature, write_back, out=scores[lo:lo + b])
    return scores


def score_summary(scores_dev, samples_dev) -> Dict[str, float]:
    """Means over the valid rows of `score_samples`' output: mean_policy_kl, mean_policy_ce, prior_top1_rate, and value_mse_vs_z,
    the network's value against the game's result of the same records (byte 91: z).  One host read."""
    import torch
    if scores_dev.shape[0] == 0:
        return {"mean_policy_kl": 0.0, "mean_policy_ce": 0.0, "prior_top1_rate": 0.0, "value_mse_vs_z": 0.0, "scored_samples": 0}
    f = scores_dev[:, :12].contiguous().view(torch.float32).double()          # policy_kl, policy_ce, value
    valid = (scores_dev[:, 13] == 1).double()
    z = samples_dev[:, 91].view(torch.int8).double()
    k = valid.sum().clamp(min=1.0)
    out = torch.stack([(f[:, 0] * valid).sum() / k, (f[:, 1] * valid).sum() / k, (scores_dev[:, 12].double() * valid).sum() / k,
                       (((f[:, 2] - z) ** 2) * valid).sum() / k, valid.sum()]).tolist()
    return {"mean_policy_kl": out[0], "mean_policy_ce": out[1], "prior_top1_rate": out[2], "value_mse_vs_z": out[3],
            "scored_samples": int(out[4])}


def run_games(model, config, num_games: int, device="cuda", n_slots: Optional[int] = None, seed: int = 0, rank: int = 0,
              evaluator_kind: str = "hip", poll_every: int = 64, device_records: bool = False, use_graph: bool = True,
              eval_cache_entries: Optional[int] = None, leaves_per_step: Optional[int] = None,
              tree_reuse: Optional[bool] = None, playout_cap=None, forced_playouts: Optional[float] = None, gumbel=None,
              perpetual_check: Optional[bool] = None, solver: Optional[bool] = None, root_stats: Optional[bool] = None,
              eval_mirror: Optional[bool] = None, record_games: Optional[bool] = None, start_pool=None,
              eval_dedup: Optional[bool] = None, adjudicate=None, resign=None):
    """Play `num_games` complete games; returns (samples, results, stats dict, elapsed seconds) in compact form:
    structured numpy arrays, or -- `device_records` -- uint8 device tensors [n, 640] / [m, 16] that never left the GPU.
    `eval_cache_entries` (None: `config.eval_cache_entries`, absent = 0 = off) gives every slot an evaluation cache of that
    many entries (engine.recommended_cache_entries); the games are the same, the network runs on fewer rows.
    `leaves_per_step` (None: `config.leaves_per_step`, absent = 1) batches up to that many leaves per slot and step under
    virtual loss (engine.SelfPlayEngine); K > 1 is not the reference's sequential search and excludes the cache.
    `tree_reuse` (None: `config.tree_reuse`, absent = off) keeps the chosen child's subtree across moves: a move then costs
    S minus the reused visits in new simulations (stats `reused_visits`, `reroots`); it needs K = 1.
    `playout_cap` = (full_search_prob, fast_simulations) (None: `config.playout_cap_full_prob` and
    `config.playout_cap_fast_simulations`, absent = off) searches only that share of the moves at full size and records only
    those as samples; the others get `fast_simulations`, no noise and no sample (stats `fast_moves`, `fast_sims`,
    `playout_cap`).  Games finish sooner and carry fewer samples each; it needs K = 1.
    `forced_playouts` = k (None: `config.forced_playouts_k`, absent or 0 = off) forces visited children of a noisy root up to
    sqrt(k * prior * root visits) visits and prunes those visits from the samples' targets and the move distribution again
    (stats `forced_sims`, `pruned_visits`, `pruned_children`, `forced_playouts`); it needs K = 1.
    `gumbel` = (m, c_visit, c_scale) (None: `config.gumbel_considered`, absent or 0 = off, with `config.gumbel_c_visit`, default
    50, and `config.gumbel_c_scale`, default 1.0) replaces the root rule by Gumbel top-m sampling with sequential halving and
    the samples' visit counts by the quantised improved policy (stats `gumbel_moves`, `gumbel_considered`, `gumbel_offprior`,
    `gumbel`); it needs K = 1 and none of tree reuse, playout cap and forced playouts.
    `perpetual_check` (None: `config.perpetual_check_loses`, absent = off) plays under the perpetual-check rule: the side that
    checks through a repetition loses instead of drawing (stats `perpetual_check`, `perpetual_check_games`: the finished games
    with reason 4).  It goes with every other option; gate under the same rule (arena.evaluate_models).
    `solver` (None: `config.mcts_solver`, absent = off) searches with proven results (stats `solver`, `proven_nodes`,
    `proven_stops`, `proven_moves`, `unspent_sims`, `removed_visits`, all 0 when off); it needs K = 1 and
    neither Gumbel root search nor forced playouts.
    `root_stats` (None: `config.record_root_stats`, absent = off, or a `config.value_target_q_mix` above 0, which needs them)
    records the search's value of every sampled position in the sample's spare bytes (`sample_format.root_stats`; stats
    `root_stats`); the games do not change.  It goes with every option but Gumbel root search.
    `eval_mirror` (None: `config.eval_random_mirror`, absent = off) evaluates every request under a randomly chosen left-right
    orientation (stats `eval_mirror`); it needs the packed step and excludes the evaluation cache.
    `record_games` (None: `config.record_games`, absent = off) keeps every finished game's moves: stats
    `record_games`, `game_records` (a hip.GAME_RECORD_DTYPE array, or under `device_records` a uint8 device tensor [n, 1024]; None
    when off), `game_records_recorded` and `game_records_dropped` (0 when off).  The games do not change; every other option.
    `start_pool` = (boards, sides, prob) (an argument only: `start_pool.py` makes the arrays, `AlphaZeroLoop` reads the config
    keys) starts a new game from an entry of the pool with probability prob: stats `start_pool`
    ((positions, prob), None when off) and `start_pool_games` (0 when off).  Not with record_games; every other option.
    `eval_dedup` (None: `config.eval_dedup`, absent = off) evaluates every distinct position once per step (DESIGN.md section
    4.24): stats `eval_dedup`, `eval_dedup_requests`, `eval_dedup_merged`, `eval_dedup_collisions`, `eval_dedup_mismatches` (0
    when off).  The games do not change, the network runs on fewer rows; it needs the packed step and excludes the evaluation
    cache, leaves_per_step > 1 and eval_mirror.
    `adjudicate` = (tables, options) (an argument only: `AlphaZeroLoop` reads the config keys and generates the tables) ends a game
    as soon as an endgame table decides its position (engine.SelfPlayEngine): stats `adjudicated_games`
    (the finished games with reason 5), `adjudicated_decisive`, `adjudicated_drawn`, `adjudicated_left_alone` and
    `adjudicated_swapped` (the engine's counters; all 0 when off).  Every other option.
    `resign` = dict(threshold=, check_steps=, holdout_prob=, max_rows=) (an argument only: `AlphaZeroLoop` reads the config keys)
    lets a side resign on its own last `check_steps` root values and plays a share `holdout_prob` of the games out
    (engine.SelfPlayEngine); max_rows defaults to num_games + 8, one row per game.  Stats `resign` (the
    options in use, None when off), `resign_rows` (sample_format.RESIGN_ROW_DTYPE, one row per finished holdout game; None when
    off), `resign_resigned`, `resign_holdout_games`, `resign_rows_dropped` and `resign_values_seen` (0 when off).  Self-play
    with every other option; `config.enable_resign`'s own rule is then only the recorder of the values."""
    if eval_dedup is None:
        eval_dedup = bool(getattr(config, "eval_dedup", False))
    if record_games is None:
        record_games = bool(getattr(config, "record_games", False))
    if eval_mirror is None:
        eval_mirror = bool(getattr(config, "eval_random_mirror", False))
    if root_stats is None:
        root_stats = bool(getattr(config, "record_root_stats", False)) or root_stats_q_mix(config) > 0.0
    if eval_cache_entries is None:
        eval_cache_entries = int(getattr(config, "eval_cache_entries", 0) or 0)
    if leaves_per_step is None:
        leaves_per_step = int(getattr(config, "leaves_per_step", 1) or 1)
    if tree_reuse is None:
        tree_reuse = bool(getattr(config, "tree_reuse", False))
    if playout_cap is None:
        p_full = getattr(config, "playout_cap_full_prob", None)
        s_fast = getattr(config, "playout_cap_fast_simulations", None)
        if (p_full is None) != (s_fast is None):
            raise ValueError("config.playout_cap_full_prob and config.playout_cap_fast_simulations go together")
        if p_full is not None:
            playout_cap = (float(p_full), int(s_fast))
    if forced_playouts is None:
        forced_playouts = float(getattr(config, "forced_playouts_k", 0) or 0) or None
    if gumbel is None:
        gm = int(getattr(config, "gumbel_considered", 0) or 0)
        if gm:
            gcv, gcs = getattr(config, "gumbel_c_visit", None), getattr(config, "gumbel_c_scale", None)
            gumbel = (gm, 50.0 if gcv is None else float(gcv), 1.0 if gcs is None else float(gcs))
    if perpetual_check is None:
        perpetual_check = bool(getattr(config, "perpetual_check_loses", False))
    if solver is None:
        solver = bool(getattr(config, "mcts_solver", False))
    slots = int(n_slots or min(num_games, 8192))
    slots = max(1, min(slots, num_games))
    ev, ev_name = evaluator.make_evaluator(model, device, evaluator_kind)
    cfg = engine.make_config(
        slots, int(config.num_simulations), c_puct=float(config.c_puct),
        temperature_threshold=int(config.temperature_threshold), max_game_length=int(config.max_game_length),
        random_opening_moves=int(config.random_opening_moves), enable_resign=bool(config.enable_resign),
        resign_threshold=float(config.resign_threshold), resign_check_steps=int(config.resign_check_steps),
        add_noise=True, seed=seed, rank=rank, games_target=num_games,
        max_out_samples=num_games * 201, max_out_results=num_games + 8)
    eng = engine.SelfPlayEngine(cfg, device, evaluator=ev, eval_cache_entries=eval_cache_entries,
                                leaves_per_step=leaves_per_step, tree_reuse=tree_reuse, playout_cap=playout_cap,
                                forced_playouts=forced_playouts, gumbel=gumbel, perpetual_check=perpetual_check, solver=solver,
                                root_stats=root_stats, eval_mirror=eval_mirror, record_games=record_games, start_pool=start_pool,
                                eval_dedup=eval_dedup, **({} if adjudicate is None else {"adjudicate": adjudicate}),
                                **({} if resign is None else {"resign": {"max_rows": num_games + 8, **resign}}))
    t0 = time.time()
    if use_graph and hasattr(ev, "evaluate_legal"):
        eng.capture_step()                             # one graph launch per step (short steps are launch-bound otherwise)
    while True:
        for _ in range(poll_every):
            eng.step()
        st = eng.stats()
        if st["games_finished"] >= num_games:
            break
    samples, results = eng.drain_device() if device_records else eng.drain()
    st = eng.stats()
    st["evaluator"] = ev_name
    st["launch"] = eng.launch_mode                     # "graph" (one HIP-graph replay per step) or "eager"
    st["path"] = eng.path                              # "packed": the evaluator ran over the waiting slots only; "full": all
    st["steps"] = eng.steps                            # rows_evaluated / (steps * slots): the share of the full width evaluated
    st["leaves_per_step"] = eng.K
    st["tree_reuse"] = eng.tree_reuse
    st["playout_cap"] = eng.playout_cap                # None, or (full_search_prob, fast_simulations)
    st["forced_playouts"] = eng.forced_playouts        # None, or k
    st["gumbel"] = eng.gumbel                          # None, or (m, c_visit, c_scale)
    st["perpetual_check"] = eng.perpetual_check
    st["solver"] = eng.solver
    st["root_stats"] = eng.root_stats
    st["eval_mirror"] = eng.eval_mirror
    st["record_games"] = eng.record_games
    st["eval_dedup"] = eng.eval_dedup
    for k in ("requests", "merged", "collisions", "mismatches"):   # the dedup's keys are present (0) when it is off
        st.setdefault("eval_dedup_" + k, 0)
    st["game_records"], st["game_records_recorded"], st["game_records_dropped"] = None, 0, 0
    if eng.record_games:
        st["game_records"] = eng.drain_games_device() if device_records else eng.drain_games()
        gs = eng.game_records_stats()
        st["game_records_recorded"], st["game_records_dropped"] = gs["recorded"], gs["dropped"]
    st["start_pool"] = eng.start_pool                  # None, or (positions, prob)
    st["start_pool_games"] = eng.start_pool_stats()["pool_games"] if eng.start_pool else 0
    for k in hip.SOLVER_KEYS:                          # the solver's keys are present (0) when it is off
        st.setdefault(k, 0)
    if device_records:
        st["perpetual_check_games"] = int((results[:, 9] == 4).sum().item()) if len(results) else 0   # byte 9: reason
    else:
        st["perpetual_check_games"] = int((results["reason"] == 4).sum())
    if device_records:                                 # the games a table ended, counted the same way
        st["adjudicated_games"] = int((results[:, 9] == hip.REASON_TABLE).sum().item()) if len(results) else 0
    else:
        st["adjudicated_games"] = int((results["reason"] == hip.REASON_TABLE).sum())
    adj = eng.adjudication_stats() if adjudicate is not None else {}
    for k in ("decisive", "drawn", "left_alone", "swapped"):       # the counters' keys are present (0) when it is off
        st["adjudicated_" + k] = adj.get("adjudicated_" + k, 0)
    rsn = eng.resign_stats() if eng.resign is not None else {}
    st["resign"] = None if eng.resign is None else dict(eng.resign)
    st["resign_rows"] = eng.drain_resign_rows() if eng.resign is not None else None
    for k in ("resigned", "holdout_games", "rows_dropped", "values_seen"):     # the counters' keys are present (0) when it is off
        st["resign_" + k] = rsn.get(k, 0)
    st.setdefault("eval_cache_probes", 0)              # the cache's keys are present (0) when it is off
    st.setdefault("eval_cache_hits", 0)
    if eng.capture_error:
        st["capture_error"] = eng.capture_error
    return samples, results, st, time.time() - t0


def parallel_self_play(model, config, num_workers: Optional[int] = None, use_gpu_server: bool = False,
                       gpu_device: str = "cuda", *, n_slots: Optional[int] = None, seed: int = 0,
                       return_compact: bool = False, eval_cache_entries: Optional[int] = None,
                       leaves_per_step: Optional[int] = None,
                       tree_reuse: Optional[bool] = None, playout_cap=None,
                       forced_playouts: Optional[float] = None, gumbel=None,
                       perpetual_check: Optional[bool] = None, solver: Optional[bool] = None,
                       record_games: Optional[bool] = None,
                       start_pool=None, eval_dedup: Optional[bool] = None) -> Tuple[List[Tuple[np.ndarray, np.ndarray, float]], Dict[str, Any]]:
    for k in _CFG_KEYS + ("num_games_per_iter",):
        if not hasattr(config, k):
            raise AttributeError(f"config lacks '{k}' (see training/train.py:55-111)")
    num_games = int(config.num_games_per_iter)
    if leaves_per_step is None:
        leaves_per_step = int(getattr(config, "leaves_per_step", 1) or 1)   # a reference TrainingConfig has no such key
    if perpetual_check is None:                        # read once, here: a reference TrainingConfig has no such key
        perpetual_check = bool(getattr(config, "perpetual_check_loses", False))
    samples, results, st, elapsed = run_games(model, config, num_games, gpu_device, n_slots, seed,
                                              eval_cache_entries=eval_cache_entries, leaves_per_step=leaves_per_step,
                                              tree_reuse=tree_reuse, playout_cap=playout_cap,
                                              forced_playouts=forced_playouts, gumbel=gumbel, perpetual_check=perpetual_check,
                                              solver=solver, record_games=record_games, start_pool=start_pool,
                                              eval_dedup=eval_dedup)
    all_data, per_game = to_reference_tuples(samples, results, augment=True, q_mix=root_stats_q_mix(config))
    wins = {1: 0, -1: 0, 0: 0}
    total_steps = 0
    for winner, steps, _n in per_game:
        wins[winner] += 1
        total_steps += steps
    stats = {
        "games": len(per_game), "red_wins": wins[1], "black_wins": wins[-1], "draws": wins[0],
        "avg_steps": total_steps / max(len(per_game), 1), "new_samples": len(all_data), "total_time": elapsed,
        "num_workers": int(st.get("games_started", num_games) and (n_slots or min(num_games, 8192))), "mode": "hip",
        "simulations": st["sims"], "leaf_evals": st["leaf_evals"], "root_evals": st["root_evals"],
        "evaluator": st["evaluator"], "launch": st["launch"], "path": st["path"], "rows_evaluated": st["rows_evaluated"],
        "eval_cache_probes": st["eval_cache_probes"], "eval_cache_hits": st["eval_cache_hits"],
        "reused_visits": st["reused_visits"], "reroots": st["reroots"],
        "fast_moves": st["fast_moves"], "fast_sims": st["fast_sims"], "playout_cap": st["playout_cap"],
        "forced_sims": st["forced_sims"], "pruned_visits": st["pruned_visits"], "pruned_children": st["pruned_children"],
        "forced_playouts": st["forced_playouts"],
        "gumbel_moves": st["gumbel_moves"], "gumbel_considered": st["gumbel_considered"],
        "gumbel_offprior": st["gumbel_offprior"], "gumbel": st["gumbel"],
        "perpetual_check": st["perpetual_check"], "perpetual_check_games": st["perpetual_check_games"],
        "solver": st["solver"], **{k: st[k] for k in hip.SOLVER_KEYS}, "root_stats": st["root_stats"],
        "record_games": st["record_games"], "game_records": st["game_records"],
        "game_records_recorded": st["game_records_recorded"], "game_records_dropped": st["game_records_dropped"],
        "start_pool": st["start_pool"], "start_pool_games": st["start_pool_games"],
        "eval_dedup": st["eval_dedup"],
        **{"eval_dedup_" + k: st["eval_dedup_" + k] for k in ("requests", "merged", "collisions", "mismatches")},
    }
    if return_compact:
        stats["compact_samples"], stats["compact_results"] = samples, results
    return all_data, stats
