"""Arena gate -- the reference's model-vs-model evaluation (`AlphaZeroTrainer._serial_evaluate`,
training/train.py:453-535) on the device-resident engine: all `eval_games` games run concurrently (one slot
each), colours alternate by game index, every move is `MCTS.get_action(temperature=0, add_noise=False)` with
`eval_simulations`, a game still running after `max_game_length` plies is a draw, and
`win_rate = (new_wins + 0.5 draws) / games >= eval_win_rate` promotes the candidate.  Deterministic (no random
draws at all), so results are checked game by game against the reference's own arena under stub evaluators.

Per step every slot is expanded from ONE network's output -- the one whose side is searching (train.py:479-483).  With the
hand-written evaluators both models run over the whole slot batch (a few dozen games: the launches, not the FLOPs, are
the cost) with the other model's requests masked out, and the merge happens on the device: a step has no host round trip.
Dense-protocol evaluators (the stubs of the fixtures) are run on their own slots only.  With a process group the games are sharded over the
ranks like self-play games (`distributed.shard_games`); the per-game results are all-gathered and every rank derives the
same verdict from the same gathered table.

Opt-in, for a gate with statistical power (rules in include/xq_hip.h, xq_engine_init_ar).  The default gate
above plays two distinct games however many it is asked for: every even game is one game, every odd game the other.
`opening_plies = R > 0` starts game g with R random legal plies drawn for the PAIR g // 2, so games 2p and 2p + 1 share an opening
with colours swapped and the games of different pairs differ; a shard plays the same games as the unsharded arena.  `packed`
(the default with openings, when both evaluators take a device-side live row count) replaces the masked step by the per-model
packed one: the waiting slots are compacted into the new model's and the old model's buffer sets on the device and each network
runs over its own live rows only.  Same games as the masked step.  `evaluate_models` reads `config.arena_opening_plies` and
`config.arena_seed` and reports the standard error of the win rate over the pairs (`pair_statistics`).

Opt-in as well: `perpetual_check` (`config.perpetual_check_loses` for `evaluate_models`) plays the gate under the perpetual-check
rule: a game one side forces into a repetition by checking on every move is that side's loss, not half a
point.  A loop that trains under the rule gates under it (`AlphaZeroLoop` passes one value to both); off, the gate is the
reference's.

Opt-in as well: `record_games` (`config.record_games` for `evaluate_models`) keeps every game's moves: an
arena game writes no samples, so its record is all that is left of it besides winner and ply count.  `play_arena` then returns
`(results, records)`, both ordered by game; `evaluate_models` adds `game_records` (this rank's games, `slot` = the game's index).

Opt-in as well: `early_stop` (`config.early_stop_decided` for `evaluate_models`) ends a search as soon as the move it will play is
fixed: one legal move, or a leader the simulations that are left cannot catch.  Every move is the first
maximum of the visit counts, so the games are the same games; `info["stats"]` adds `settled_moves` and `simulations_saved`.

Opt-in as well: `play_arena(adjudicate=(tables, options))` ends a game as soon as an endgame table decides its position (DESIGN.md
section 4.26); the result then carries reason 5.  `evaluate_models` and the loop's gate do not use it.
"""
from __future__ import annotations

from typing import Callable, Dict, Optional

import os

import numpy as np
import torch

from . import engine, evaluator as ev_mod, hip
from .sample_format import RESULT_DTYPE


def _evaluate_subset(eng, ev, x, idx, policy_is_probs, dense, legal, value):
    """Run `ev` on the slots `idx` (int64 device tensor) and scatter its outputs into the full-width buffers."""
    if idx.numel() == 0:
        return
    xs = x.index_select(0, idx)
    if hasattr(ev, "evaluate_legal") and not policy_is_probs:
        ll, v = ev.evaluate_legal(xs, eng.req_moves.index_select(0, idx), eng.req_counts.index_select(0, idx))
        legal.index_copy_(0, idx, ll)
    else:
        p, v = ev(xs)
        dense.index_copy_(0, idx, p)
    value.index_copy_(0, idx, v.view(-1))


def play_arena(eval_new: Callable, eval_old: Callable, eval_games: int, eval_simulations: int, max_game_length: int,
               c_puct: float = 1.5, device="cuda", policy_is_probs: bool = False, first_game: int = 0,
               opening_plies: int = 0, seed: int = 0, packed: Optional[bool] = None, inject=None, info: Optional[dict] = None,
               perpetual_check: bool = False, solver: bool = False, record_games: bool = False, early_stop: bool = False,
               adjudicate=None):
    """eval_*: evaluators in either protocol (`evaluate_legal`, or a callable float32[n,15,10,9] -> (policy
    float32[n,8100], value float32[n])); both must use the same one.  Plays games first_game .. first_game+eval_games-1
    of the arena (the new model is red in even games) and returns the results array ordered by game (slot == game -
    first_game).
    Opt-in: `opening_plies` > 0 and `seed` give every pair of games its random opening; `packed` (None: yes with openings when
    both evaluators offer `live_rows`) takes the per-model packed step; `inject` (uint64 [games, 4, n], tests only) replaces the
    device draws; `info` (a dict) receives `openings`, `opening_counts`, `steps` (engine steps run) and the engine's `stats`;
    `perpetual_check` builds the engine with the perpetual-check rule (results then may carry reason 4); `solver` with the
    proven-result search (a move shown to lose is not played while another is not, a move shown to win is
    played at once; `info["stats"]` then carries the five solver counters); `record_games` with game records: the return value is
    then `(results, records)`, the records (hip.GAME_RECORD_DTYPE) ordered by game like the results; `early_stop` with the
    settled-move cutoff (a search ends as soon as its first choice is fixed; the same games, and
    `info["stats"]` then carries `settled_moves` and `simulations_saved`); `adjudicate` = (tables, options) with table adjudication
    (engine.SelfPlayEngine, DESIGN.md section 4.26: a game ends, with reason 5, as soon as an endgame table decides its position;
    `info["stats"]` then carries the `adjudicated_*` counters)."""
    cfg = engine.make_config(eval_games, eval_simulations, c_puct=c_puct, max_game_length=max_game_length,
                             random_opening_moves=0, enable_resign=False, add_noise=False, games_target=eval_games,
                             manual_moves=2)
    opts = int(opening_plies) > 0 or bool(packed) or inject is not None or info is not None
    adj = {} if adjudicate is None else {"adjudicate": adjudicate}      # off: the engine is built by the call without the key
    if not opts:
        eng = engine.SelfPlayEngine(cfg, device, perpetual_check=perpetual_check, solver=solver, record_games=record_games,
                                    early_stop=early_stop, **adj)
    else:
        if inject is not None:
            cfg.inject_len = int(np.asarray(inject).shape[-1])
        cfg.seed = int(seed)
        eng = engine.arena_engine(cfg, device, opening_plies, first_game, inject, perpetual_check=perpetual_check, solver=solver,
                                  record_games=record_games, early_stop=early_stop, **adj)
    dev = eng.device
    new_is_red = ((torch.arange(eval_games, device=dev) + first_game) % 2 == 0)
    sparse = hasattr(eval_new, "evaluate_legal") and hasattr(eval_old, "evaluate_legal") and not policy_is_probs
    dense = None if sparse else torch.zeros((eval_games, 8100), dtype=torch.float32, device=dev)
    legal = torch.zeros((eval_games, 128), dtype=torch.float32, device=dev) if sparse else None
    value = torch.zeros(eval_games, dtype=torch.float32, device=dev)
    zero = torch.zeros_like(eng.req_counts)
    # XQ_ARENA_STREAMS=0: both networks on the one stream (A/B runs and the equality test)
    side = torch.cuda.Stream(device=dev) if sparse and os.environ.get("XQ_ARENA_STREAMS", "1") != "0" else None
    can_pack = sparse and bool(getattr(eval_new, "live_rows", False)) and bool(getattr(eval_old, "live_rows", False))
    if packed and not can_pack:
        raise hip.XqError("packed arena step: both evaluators must offer evaluate_legal with live_rows (the HIP evaluators)")
    packed = (can_pack and int(opening_plies) > 0) if packed is None else bool(packed)
    if opts and eval_old is eval_new:
        side = None                                        # one evaluator's buffers serve one branch at a time

    def packed_step():
        # select -> two slot-ordered compactions by searching model -> each network over its own live rows -> scatter + expand.
        # The counts stay on the device and every grid is sized by the slot count: the step records into one graph, the old
        # network on the side stream as a parallel branch like the masked step's.
        eng.select()
        eng.compact_arena()
        s_new, s_old = eng.arena_packed
        if side is not None:
            main = torch.cuda.current_stream(dev)
            side.wait_stream(main)
            with torch.cuda.stream(side):
                ll_old, v_old = eval_old.evaluate_legal(s_old["x"], s_old["moves"], s_old["counts"], n_live=s_old["n_live"])
            ll_new, v_new = eval_new.evaluate_legal(s_new["x"], s_new["moves"], s_new["counts"], n_live=s_new["n_live"])
            main.wait_stream(side)
        else:
            ll_new, v_new = eval_new.evaluate_legal(s_new["x"], s_new["moves"], s_new["counts"], n_live=s_new["n_live"])
            if eval_old is eval_new:
                ll_new, v_new = ll_new.clone(), v_new.clone()   # the second call reuses the evaluator's output buffers
            ll_old, v_old = eval_old.evaluate_legal(s_old["x"], s_old["moves"], s_old["counts"], n_live=s_old["n_live"])
        eng.expand_packed_arena(ll_new, v_new, ll_old, v_old)

    def step():
        if packed:
            return packed_step()
        x = eng.select()
        # the model that is SEARCHING evaluates every node of its search (root and leaves at any depth), so the
        # choice follows the side to move of the real game, not of the evaluated position (train.py:479-483)
        red_to_move = eng.slot_ints[:, hip.GI_SIDE] == 1
        use_new = new_is_red == red_to_move
        if sparse:
            # No host round trip in a step: each model runs over the whole (small) slot batch with the OTHER model's
            # request counts masked to zero -- xq_policy_head_legal skips those rows -- and the two results are merged
            # on the device.  Batch size and conv variant are the same every step (no nonzero(), no data-dependent shapes).
            # The two networks are independent: the old one runs on a side stream (forked from / joined to the main one), so at arena
            # batch sizes -- ten games, every kernel a fraction of the chip -- the two towers overlap; recorded into the graph as two
            # parallel branches.
            c_new, c_old = torch.where(use_new, eng.req_counts, zero), torch.where(use_new, zero, eng.req_counts)
            if side is not None:
                main = torch.cuda.current_stream(dev)
                side.wait_stream(main)
                with torch.cuda.stream(side):
                    ll_old, v_old = eval_old.evaluate_legal(x, eng.req_moves, c_old)
                ll_new, v_new = eval_new.evaluate_legal(x, eng.req_moves, c_new)
                main.wait_stream(side)
            else:
                ll_new, v_new = eval_new.evaluate_legal(x, eng.req_moves, c_new)
                ll_old, v_old = eval_old.evaluate_legal(x, eng.req_moves, c_old)
            torch.where(use_new.unsqueeze(1), ll_new, ll_old, out=legal)
            torch.where(use_new, v_new.view(-1), v_old.view(-1), out=value)
            eng.expand_legal(legal, value)
        else:
            _evaluate_subset(eng, eval_new, x, use_new.nonzero().view(-1), policy_is_probs, dense, legal, value)
            _evaluate_subset(eng, eval_old, x, (~use_new).nonzero().view(-1), policy_is_probs, dense, legal, value)
            eng.expand(dense, value, policy_is_probs)

    # A sparse step is ~70 launches for a handful of games (eval_games = 10 in the reference's config): launch-bound.  It has no host
    # synchronisation and no data-dependent shape, so it is recorded once into a HIP graph and replayed (same kernels, same results);
    # XQ_ARENA_GRAPH=0 keeps it eager.  Only a capture-unsupported error keeps the eager path (as engine.capture_step).
    graph = None
    if sparse and os.environ.get("XQ_ARENA_GRAPH", "1") != "0":
        step()
        step()                                               # real steps: buffers of both evaluators exist before the recording
        torch.cuda.synchronize(dev)
        g = torch.cuda.CUDAGraph()
        try:
            with torch.cuda.graph(g, capture_error_mode="thread_local"):
                step()
            graph = g
        except hip.XqError:
            raise
        except RuntimeError as e:
            msg = str(e).lower()
            if not any(k in msg for k in ("captur", "hiperrorstreamcapture", "cudaerrorstreamcapture", "operation not permitted")):
                raise
            torch.cuda.synchronize(dev)
    n_steps = 2 if graph is not None else 0               # the two warm-up steps are steps of the games (the recording runs nothing)
    while True:
        for _ in range(64):
            if graph is not None:
                graph.replay()
            else:
                step()
        n_steps += 64
        st = eng.stats()
        if st["games_finished"] >= eval_games:
            break
    _, results = eng.drain()
    if eng.early_stop:
        st.update(eng.early_stop_stats())
    if adjudicate is not None:
        st.update(eng.adjudication_stats())
    if info is not None:
        info["openings"], info["opening_counts"] = eng.arena_openings()
        info["steps"], info["stats"], info["packed"] = n_steps, st, bool(packed)
    results = results[results["slot"].argsort()]
    if not record_games:
        return results
    records = eng.drain_games()
    return results, records[records["slot"].argsort()]


def pair_statistics(winners) -> Dict[str, object]:
    """Win rate of the new model with its standard error over PAIRS.  `winners[g]` is game g's winner (1 red, -1 black, 0 draw),
    the new model red in even games; games 2p and 2p + 1 share an opening, so they are not independent and the pair is the
    sample: s_p = the mean of the new model's scores (1 / 0.5 / 0) in the pair's two games, win_rate = mean(s_p),
    se = std(s_p, ddof=1) / sqrt(P) (0 for a single pair), ci95 = win_rate -+ 1.96 se."""
    w = np.asarray(winners, dtype=np.int64).reshape(-1)
    if w.size == 0 or w.size % 2:
        raise ValueError("pair_statistics needs an even, positive number of games")
    red_score = np.where(w == 1, 1.0, np.where(w == 0, 0.5, 0.0))
    score = np.where(np.arange(w.size) % 2 == 0, red_score, 1.0 - red_score)
    s = score.reshape(-1, 2).mean(axis=1)
    pairs = int(s.size)
    rate = float(s.mean())
    se = float(s.std(ddof=1) / np.sqrt(pairs)) if pairs > 1 else 0.0
    return {"pairs": pairs, "win_rate": rate, "win_rate_se": se, "win_rate_ci95": (rate - 1.96 * se, rate + 1.96 * se)}


def evaluate_models(new_model, old_model, config, device="cuda", evaluator_kind: str = "hip", group=None,
                    seed: Optional[int] = None, perpetual_check: Optional[bool] = None,
                    solver: Optional[bool] = None, record_games: Optional[bool] = None,
                    early_stop: Optional[bool] = None) -> Dict[str, object]:
    """Same stats dict as the reference (`new_wins, old_wins, draws, win_rate, model_updated`); reads
    `eval_games, eval_simulations, c_puct, max_game_length, eval_win_rate` from `config` (train.py:97-100).
    Under torch.distributed the games are split over the ranks and the winners all-gathered.
    `config.arena_opening_plies` = R > 0 (absent or 0: off) plays paired random openings (module docstring) under the seed
    `seed` (None: `config.arena_seed`, absent: 0); `eval_games` must then be even, and the result adds `opening_plies`, `pairs`,
    `openings` (uint16 [games, R]), `win_rate_se` and `win_rate_ci95`.  The promotion rule is unchanged.
    `perpetual_check` (None: `config.perpetual_check_loses`, absent: off) plays the games under the perpetual-check rule; the
    result then adds `perpetual_check` = True.  Off, `play_arena` is called as before.
    `solver` (None: `config.mcts_solver`, absent: off) searches with proven results; the result then adds `solver` = True.
    `record_games` (None: `config.record_games`, absent: off) adds `game_records`: the records of the games THIS rank played
    (hip.GAME_RECORD_DTYPE, `slot` = the game's index in the arena); records are not gathered across ranks.
    `early_stop` (None: `config.early_stop_decided`, absent: off) plays with the settled-move cutoff; the result then adds
    `early_stop` = True.  The games and the verdict are those without it."""
    import torch.distributed as dist
    from . import distributed as xdist
    total = int(config.eval_games)
    plies = int(getattr(config, "arena_opening_plies", 0) or 0)
    if plies > 0 and total % 2:
        raise ValueError(f"arena_opening_plies needs an even eval_games (games come in colour-swapped pairs), got {total}")
    if seed is None:
        seed = int(getattr(config, "arena_seed", 0) or 0)
    if perpetual_check is None:
        perpetual_check = bool(getattr(config, "perpetual_check_loses", False))
    rule = {"perpetual_check": True} if perpetual_check else {}
    if solver is None:
        solver = bool(getattr(config, "mcts_solver", False))
    if solver:
        rule["solver"] = True
    if record_games is None:
        record_games = bool(getattr(config, "record_games", False))
    records = np.zeros(0, dtype=hip.GAME_RECORD_DTYPE)
    if record_games:
        rule["record_games"] = True
    if early_stop is None:
        early_stop = bool(getattr(config, "early_stop_decided", False))
    if early_stop:
        rule["early_stop"] = True
    openings = np.zeros((total, max(plies, 0)), dtype=np.int64)
    world = dist.get_world_size(group) if dist.is_initialized() else 1
    rank = dist.get_rank(group) if dist.is_initialized() else 0
    mine = xdist.shard_games(total, world, rank)
    first = sum(xdist.shard_games(total, world, r) for r in range(rank))
    winners = np.zeros(total, dtype=np.int64)
    steps = np.zeros(total, dtype=np.int64)
    if mine > 0:
        en, _ = ev_mod.make_evaluator(new_model, device, evaluator_kind)
        eo, _ = ev_mod.make_evaluator(old_model, device, evaluator_kind)
        if plies > 0:
            info = {}
            res = play_arena(en, eo, mine, int(config.eval_simulations), int(config.max_game_length), float(config.c_puct),
                             device, first_game=first, opening_plies=plies, seed=int(seed), info=info, **rule)
            if record_games:
                res, records = res
            openings[first:first + mine] = info["openings"][:, :plies]
        else:
            res = play_arena(en, eo, mine, int(config.eval_simulations), int(config.max_game_length), float(config.c_puct),
                             device, first_game=first, **rule)
            if record_games:
                res, records = res
        winners[first:first + mine] = res["winner"].astype(np.int64)
        steps[first:first + mine] = res["steps"].astype(np.int64)
        records["slot"] += first
    if dist.is_initialized():         # disjoint shards: a sum gathers them; every rank ends with the same table (a group of
                                      # one rank runs the same collective)
        t = torch.from_numpy(np.stack([winners, steps])).to(device if dist.get_backend(group) == "nccl" else "cpu")
        dist.all_reduce(t, group=group)
        winners, steps = t[0].cpu().numpy(), t[1].cpu().numpy()
        if plies > 0:
            t = torch.from_numpy(openings).to(device if dist.get_backend(group) == "nccl" else "cpu")
            dist.all_reduce(t, group=group)
            openings = t.cpu().numpy()
    new_wins = old_wins = draws = 0
    for game in range(total):
        w, new_is_red = int(winners[game]), game % 2 == 0
        if w == 0:
            draws += 1
        elif (w == 1) == new_is_red:
            new_wins += 1
        else:
            old_wins += 1
    win_rate = (new_wins + 0.5 * draws) / total
    games = np.zeros(total, dtype=RESULT_DTYPE)
    games["slot"], games["winner"], games["steps"] = np.arange(total), winners, steps
    out = {"new_wins": new_wins, "old_wins": old_wins, "draws": draws, "win_rate": win_rate,
           "model_updated": win_rate >= float(config.eval_win_rate), "games": games, **rule}
    if record_games:
        out["game_records"] = records
    if plies > 0:
        ps = pair_statistics(winners)
        out.update({"opening_plies": plies, "pairs": ps["pairs"], "openings": openings.astype(np.uint16),
                    "win_rate_se": ps["win_rate_se"], "win_rate_ci95": ps["win_rate_ci95"]})
    return out
