"""The outer training loop on top of the self-play path -- `AlphaZeroTrainer.train()` (training/train.py:581-638) with
the engine underneath, one process per GPU (BASELINE configs[4]).

Per iteration, exactly the reference's order:
  1. self-play     every rank plays `shard_games(num_games_per_iter, world, rank)` games on its own engine with the
                   current best weights (no collective during search); the finished compact samples stay on the device
                   (`xq_engine_drain_device`) and one padded all-gather of those device buffers brings every rank's
                   records to every rank's device-resident replay buffer.  Opt-in (`config.adjudicate_signatures`, with
                   `adjudicate_draws` and `adjudicate_min_ply`): a game ends as soon as one of those endgame tables decides
                   its position, and its samples get the exact result (engine.SelfPlayEngine's `adjudicate`).  Opt-in
                   (`config.resign_per_side`): a side resigns on its own last root values, a share `resign_holdout_prob` of
                   the games is played out, and the iteration logs under "resign" the threshold used, the games resigned, the
                   holdout games, the pairs below the threshold with their false-positive rate and the calibrated threshold
                   (`resign.calibrate`); with `resign_calibrate` the next iteration plays under it;
  2. train        `train_network` data-parallel over the ranks (every batch split, SyncBatchNorm, bucketed gradient
                   all-reduce: the reference's full-batch update) -- or on rank 0 alone with `config.ddp = False` -- then
                   ONE flat `broadcast_weights`;
  3. arena gate    every second iteration (train.py:609) the candidate plays the best model, the games sharded over the
                   ranks (`arena.evaluate_models`); promote at win_rate >= eval_win_rate, else the candidate reverts to
                   the best weights (train.py:525-533).  Every rank derives the verdict from the same all-reduced table
                   and rank 0's decision is broadcast on top, so the replicas cannot drift apart;
  3b. baseline     opt-in (`config.baseline_games` > 0): every `baseline_interval`-th iteration rank 0 plays the best model
                   against the fixed alpha-beta opponent (`baseline.play_vs_baseline`) and logs the result under "baseline" in
                   that iteration's entry: an absolute yardstick next to the gate's relative one; it decides nothing;
  3c. tactics      opt-in (`config.tactics_file`): every `tactics_interval`-th iteration rank 0 scores the best model on the
                   file's forced mates (`tactics.solve_rate`) and logs the result under "tactics"; it decides nothing;
  3d. endgame      opt-in (`config.endgame_signature`): every `endgame_interval`-th iteration rank 0 scores the best model on
                   won (or drawn) positions of the signature's tablebase (`endgame.hold_rate`) and logs the result under
                   "endgame"; it decides nothing.  With `endgame_rescore` the samples the table covers get their exact outcome
                   before they enter the buffer (`endgame.rescore_samples`).  With `endgame_playout_positions` rank 0 also plays
                   won entries out against the table's best defence (`endgame.play_out`, logged under "endgame_playout"), and with
                   `endgame_teacher_samples` every rank appends that many table samples to its buffer after self-play's;
  4. checkpoint    every `save_interval` iterations and once more after the last one (train.py:613-615, 636-637), the
                   reference's file format; `training_stats.json` like train.py:620-634.
`resume(path)` is the reference's `--resume` (train.py:569-579, 759-761): iteration, total_games, both models, optimizer
and scheduler come back from a `checkpoint_iter*.pt` (written here or by the reference); the loop then continues at the
next iteration.  Like the reference the checkpoint itself does not hold the replay buffer; this loop additionally writes
`replay_buffer.pt` (its compact device records) next to it and restores it when present, so that a resumed run continues
exactly where an uninterrupted one would be.
Works unchanged with world_size 1, with or without a process group: every collective below runs whenever a group is
initialised (a one-rank RCCL group exercises the same calls as eight ranks).
"""
from __future__ import annotations

import copy
import json
import os
import time
from typing import Optional

import numpy as np
import torch
import torch.distributed as dist

from . import arena, distributed as xdist, hip, selfplay, training
from .model import XiangqiNet
from .sample_format import GAME_RECORD_DTYPE, RESULT_DTYPE, SAMPLE_DTYPE, records_from_text, records_to_text


def _baseline_options(config):
    """The baseline gate's keys (all optional; absent means off): None when config.baseline_games is absent or 0, else a dict of
    games, depth, simulations, opening_plies, interval.  A key outside its range raises XqError with the key's name."""
    def key(name, default):
        v = getattr(config, name, None)
        v = default if v is None else v
        if isinstance(v, bool) or int(v) != v:
            raise hip.XqError(f"config.{name} must be an integer, got {v!r}")
        return int(v)

    games = key("baseline_games", 0)
    if games < 0 or games % 2:
        raise hip.XqError(f"config.baseline_games must be even and >= 0 (games come in colour-swapped pairs), got {games}")
    depth = key("baseline_depth", 2)
    if not 0 <= depth <= hip.AB_MAX_DEPTH:
        raise hip.XqError(f"config.baseline_depth must be in [0, {hip.AB_MAX_DEPTH}], got {depth}")
    plies = key("baseline_opening_plies", 4)
    if not 0 <= plies <= hip.ARENA_MAX_OPENING:
        raise hip.XqError(f"config.baseline_opening_plies must be in [0, {hip.ARENA_MAX_OPENING}], got {plies}")
    interval = key("baseline_interval", 2)
    if interval < 1:
        raise hip.XqError(f"config.baseline_interval must be >= 1, got {interval}")
    if games == 0:
        return None
    sims = key("baseline_simulations", int(config.eval_simulations))
    if sims < 1:
        raise hip.XqError(f"config.baseline_simulations must be >= 1, got {sims}")
    return {"games": games, "depth": depth, "simulations": sims, "opening_plies": plies, "interval": interval}


def _tactics_options(config):
    """The tactics yardstick's keys (all optional; absent means off): None when config.tactics_file is absent or None, else a dict
    of file, max_moves, checks_only, simulations, interval and positions (the file's positions, read here: a missing file raises
    at construction).  A key outside its range raises XqError with the key's name, whether the yardstick is on or not."""
    def key(name, default):
        v = getattr(config, name, None)
        v = default if v is None else v
        if isinstance(v, bool) or int(v) != v:
            raise hip.XqError(f"config.{name} must be an integer, got {v!r}")
        return int(v)

    path = getattr(config, "tactics_file", None)
    if path is not None and not isinstance(path, (str, os.PathLike)):
        raise hip.XqError(f"config.tactics_file must be a path, got {path!r}")
    max_moves = key("tactics_max_moves", 3)
    if not 1 <= max_moves <= hip.MATE_MAX_MOVES:
        raise hip.XqError(f"config.tactics_max_moves must be in [1, {hip.MATE_MAX_MOVES}], got {max_moves}")
    checks_only = getattr(config, "tactics_checks_only", None)
    if checks_only is not None and not isinstance(checks_only, bool):
        raise hip.XqError(f"config.tactics_checks_only must be a bool, got {checks_only!r}")
    interval = key("tactics_interval", 1)
    if interval < 1:
        raise hip.XqError(f"config.tactics_interval must be >= 1, got {interval}")
    sims = key("tactics_simulations", int(config.eval_simulations))
    if sims < 1:
        raise hip.XqError(f"config.tactics_simulations must be >= 1, got {sims}")
    if path is None:
        return None
    from . import tactics
    with open(path) as f:
        try:
            positions = tactics.puzzles_from_text(f.read())
        except ValueError as e:
            raise hip.XqError(f"config.tactics_file {os.fspath(path)!r}: {e}") from None
    return {"file": os.fspath(path), "max_moves": max_moves, "checks_only": True if checks_only is None else checks_only,
            "simulations": sims, "interval": interval, "positions": positions}


def _endgame_options(config):
    """The endgame yardstick's keys (all optional; absent means off): None when config.endgame_signature is absent or None, else a
    dict of signature, positions, kind, simulations, interval and rescore.  A key outside its range raises XqError with the key's
    name, whether the yardstick is on or not.  The table is generated at first use."""
    def key(name, default):
        v = getattr(config, name, None)
        v = default if v is None else v
        if isinstance(v, bool) or int(v) != v:
            raise hip.XqError(f"config.{name} must be an integer, got {v!r}")
        return int(v)

    from . import endgame
    sig = getattr(config, "endgame_signature", None)
    if sig is not None:
        try:
            hip.tb_entries(sig)
        except hip.XqError as e:
            raise hip.XqError(f"config.endgame_signature: {e}") from None
    positions = key("endgame_positions", 256)
    if positions < 1:
        raise hip.XqError(f"config.endgame_positions must be >= 1, got {positions}")
    kind = getattr(config, "endgame_kind", None)
    kind = "win" if kind is None else kind
    if kind not in ("win", "draw"):
        raise hip.XqError(f"config.endgame_kind must be 'win' or 'draw' (a lost position cannot be held), got {kind!r}")
    sims = key("endgame_simulations", int(config.eval_simulations))
    if sims < 1:
        raise hip.XqError(f"config.endgame_simulations must be >= 1, got {sims}")
    interval = key("endgame_interval", 1)
    if interval < 1:
        raise hip.XqError(f"config.endgame_interval must be >= 1, got {interval}")
    rescore = getattr(config, "endgame_rescore", None)
    if rescore is not None and not isinstance(rescore, bool):
        raise hip.XqError(f"config.endgame_rescore must be a bool, got {rescore!r}")
    if sig is None:
        return None
    return {"signature": endgame.signature_text(sig), "positions": positions, "kind": kind, "simulations": sims,
            "interval": interval, "rescore": bool(rescore)}


def _endgame_play_options(config):
    """The keys that use the table as opponent and as teacher (all optional; absent means off) -> (playout, teacher): playout None
    or a dict of positions and max_plies (config.endgame_playout_positions, endgame_playout_max_plies); teacher None or a dict of
    samples and policy (config.endgame_teacher_samples, endgame_teacher_policy).  Both need config.endgame_signature.  A key
    outside its range raises XqError with the key's name."""
    def key(name):
        v = getattr(config, name, None)
        if v is not None and (isinstance(v, bool) or not isinstance(v, (int, np.integer))):
            raise hip.XqError(f"config.{name} must be an integer, got {v!r}")
        return None if v is None else int(v)

    positions, max_plies = key("endgame_playout_positions"), key("endgame_playout_max_plies")
    samples, policy = key("endgame_teacher_samples"), key("endgame_teacher_policy")
    if positions is not None and positions < 1:
        raise hip.XqError(f"config.endgame_playout_positions must be >= 1, got {positions}")
    if max_plies is not None and max_plies < 1:
        raise hip.XqError(f"config.endgame_playout_max_plies must be >= 1, got {max_plies}")
    if samples is not None and samples < 1:
        raise hip.XqError(f"config.endgame_teacher_samples must be >= 1, got {samples}")
    if policy is not None and policy not in (0, 1):
        raise hip.XqError(f"config.endgame_teacher_policy must be 0 (every optimal move) or 1 (the first one), got {policy}")
    if getattr(config, "endgame_signature", None) is None:
        for name, v in (("endgame_playout_positions", positions), ("endgame_teacher_samples", samples)):
            if v is not None:
                raise hip.XqError(f"config.{name} needs config.endgame_signature")
        return None, None
    playout = None if positions is None else {"positions": positions, "max_plies": 100 if max_plies is None else max_plies}
    teacher = None if samples is None else {"samples": samples, "policy": 0 if policy is None else policy}
    return playout, teacher


def _resign_options(config):
    """The per-side resign rule's keys (all optional; absent means off): None unless config.resign_per_side is true, else a dict
    of threshold (config.resign_threshold), check_steps (config.resign_check_steps), holdout_prob (config.resign_holdout_prob,
    default 0.1), calibrate (config.resign_calibrate, default false), fp_target (config.resign_fp_target, default 0.05),
    min_pairs (config.resign_min_pairs, default 20) and threshold_max (config.resign_threshold_max, default the larger of -0.5 and
    the threshold).  A bad value raises XqError with the key's name, whether the option is on or not."""
    on = getattr(config, "resign_per_side", None)
    calibrate = getattr(config, "resign_calibrate", None)
    for key, v in (("resign_per_side", on), ("resign_calibrate", calibrate)):
        if v is not None and not isinstance(v, bool):
            raise hip.XqError(f"config.{key} must be a bool, got {v!r}")

    def number(key, default, lo, hi):
        v = getattr(config, key, None)
        v = default if v is None else v
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not lo <= float(v) <= hi:      # a NaN fails the comparison
            raise hip.XqError(f"config.{key} must be a number in [{lo}, {hi}], got {v!r}")
        return float(v)

    prob = number("resign_holdout_prob", 0.1, 0.0, 1.0)
    target = number("resign_fp_target", 0.05, 0.0, 1.0)
    min_pairs = getattr(config, "resign_min_pairs", None)
    min_pairs = 20 if min_pairs is None else min_pairs
    if isinstance(min_pairs, bool) or not isinstance(min_pairs, int) or min_pairs < 1:
        raise hip.XqError(f"config.resign_min_pairs must be an integer >= 1, got {min_pairs!r}")
    t_max = getattr(config, "resign_threshold_max", None)
    if t_max is not None and (isinstance(t_max, bool) or not isinstance(t_max, (int, float)) or t_max != t_max):
        raise hip.XqError(f"config.resign_threshold_max must be a number, got {t_max!r}")
    if not on:
        return None
    if not bool(getattr(config, "enable_resign", False)):
        raise hip.XqError("config.resign_per_side needs config.enable_resign: the engine's own rule records the root values")
    opts = hip.resign_opts(config.resign_threshold, config.resign_check_steps, prob, what="config.resign_per_side")
    return {"threshold": float(opts.threshold), "check_steps": int(opts.check_steps), "holdout_prob": prob,
            "calibrate": bool(calibrate), "fp_target": target, "min_pairs": int(min_pairs),
            "threshold_max": max(-0.5, float(opts.threshold)) if t_max is None else float(t_max)}


def _adjudicate_options(config):
    """Table adjudication's keys (all optional; absent means off): None when config.adjudicate_signatures is absent, None or empty,
    else a dict of signatures (FEN letters, one to four), draws (config.adjudicate_draws, default true) and min_ply
    (config.adjudicate_min_ply, default 1).  A bad value raises XqError with the key's name, whether the option is on or not.  The
    tables are generated at first use."""
    from . import endgame, engine
    draws = getattr(config, "adjudicate_draws", None)
    if draws is not None and not isinstance(draws, bool):
        raise hip.XqError(f"config.adjudicate_draws must be a bool, got {draws!r}")
    min_ply = getattr(config, "adjudicate_min_ply", None)
    min_ply = 1 if min_ply is None else min_ply
    if isinstance(min_ply, bool) or not isinstance(min_ply, int) or min_ply < 0:
        raise hip.XqError(f"config.adjudicate_min_ply must be an integer >= 0, got {min_ply!r}")
    sigs = getattr(config, "adjudicate_signatures", None)
    if sigs is None:
        return None
    if isinstance(sigs, str) or not isinstance(sigs, (list, tuple)):
        raise hip.XqError(f"config.adjudicate_signatures must be a list of signatures such as ['Ra', 'CA'], got {sigs!r}")
    if len(sigs) > engine.ADJUDICATE_MAX_TABLES:
        raise hip.XqError(f"config.adjudicate_signatures: at most {engine.ADJUDICATE_MAX_TABLES} tables, got {len(sigs)}")
    for sig in sigs:
        try:
            hip.tb_entries(sig)
        except hip.XqError as e:
            raise hip.XqError(f"config.adjudicate_signatures: {e}") from None
    if not sigs:
        return None
    return {"signatures": [endgame.signature_text(sig) for sig in sigs], "draws": True if draws is None else draws,
            "min_ply": int(min_ply)}


def _start_pool_options(config):
    """The start-position pool's keys (all optional; absent means off): None when neither config.start_positions_file nor
    config.start_positions_endgame is set, else a dict of file, boards and sides (the file's positions, read here: a missing file
    raises at construction), endgame (entries of config.endgame_signature's table per iteration, or None) and prob
    (config.start_positions_prob: required with a source, no default).  A key outside its range raises XqError with the key's
    name, whether the pool is on or not; either source with config.record_games or config.game_records_dir does as well."""
    from . import start_pool
    path = getattr(config, "start_positions_file", None)
    if path is not None and not isinstance(path, (str, os.PathLike)):
        raise hip.XqError(f"config.start_positions_file must be a path, got {path!r}")
    n_end = getattr(config, "start_positions_endgame", None)
    if n_end is not None and (isinstance(n_end, bool) or not isinstance(n_end, (int, np.integer))):
        raise hip.XqError(f"config.start_positions_endgame must be an integer, got {n_end!r}")
    if n_end is not None and not 1 <= int(n_end) <= hip.START_POOL_MAX:
        raise hip.XqError(f"config.start_positions_endgame must be in [1, {hip.START_POOL_MAX}], got {n_end}")
    prob = getattr(config, "start_positions_prob", None)
    if prob is not None and (isinstance(prob, bool) or not isinstance(prob, (int, float, np.integer, np.floating))):
        raise hip.XqError(f"config.start_positions_prob must be a number, got {prob!r}")
    if prob is not None and not 0.0 < float(prob) <= 1.0:            # a NaN fails both comparisons
        raise hip.XqError(f"config.start_positions_prob must be in (0, 1], got {prob}")
    if path is None and n_end is None:
        if prob is not None:
            raise hip.XqError("config.start_positions_prob needs config.start_positions_file or config.start_positions_endgame")
        return None
    if prob is None:
        raise hip.XqError("config.start_positions_prob is required with config.start_positions_file or "
                          "config.start_positions_endgame: it has no default")
    if n_end is not None and getattr(config, "endgame_signature", None) is None:
        raise hip.XqError("config.start_positions_endgame needs config.endgame_signature")
    if bool(getattr(config, "record_games", False)) or getattr(config, "game_records_dir", None):
        raise hip.XqError("config.start_positions_file / config.start_positions_endgame cannot be combined with config.record_games "
                          "or config.game_records_dir: a game record has no room for a start position")
    boards, sides = np.zeros((0, 90), dtype=np.int8), np.zeros(0, dtype=np.int8)
    if path is not None:
        try:
            boards, sides = start_pool.from_fens(os.fspath(path) if os.path.exists(path) else open(path).read())
        except ValueError as e:
            raise hip.XqError(f"config.start_positions_file: {e}") from None
        if not 1 <= len(boards) <= hip.START_POOL_MAX:
            raise hip.XqError(f"config.start_positions_file must hold 1 to {hip.START_POOL_MAX} positions, {path!r} holds {len(boards)}")
    return {"file": None if path is None else os.fspath(path), "boards": boards, "sides": sides,
            "endgame": None if n_end is None else int(n_end), "prob": float(prob)}


def _pretrain_options(config):
    """The supervised warm start's keys (all optional; absent means off): None when config.pretrain_records is absent or empty,
    else a dict of paths, epochs, movers, skip_draws and records (the games of every file, read here: a missing file raises at
    construction).  A key outside its range raises XqError with the key's name."""
    paths = getattr(config, "pretrain_records", None)
    if isinstance(paths, (str, os.PathLike)):
        paths = [paths]
    if paths is not None and (not isinstance(paths, (list, tuple)) or not all(isinstance(p, (str, os.PathLike)) for p in paths)):
        raise hip.XqError(f"config.pretrain_records must be a path or a list of paths, got {paths!r}")

    def key(name, default):
        v = getattr(config, name, None)
        v = default if v is None else v
        if isinstance(v, bool) or int(v) != v:
            raise hip.XqError(f"config.{name} must be an integer, got {v!r}")
        return int(v)

    epochs = key("pretrain_epochs", 1)
    if epochs < 1:
        raise hip.XqError(f"config.pretrain_epochs must be >= 1, got {epochs}")
    movers = key("pretrain_movers", 0)
    if not 0 <= movers <= 3:
        raise hip.XqError(f"config.pretrain_movers must be 0 (every ply), 1 (the winner's), 2 (red's) or 3 (black's), got {movers}")
    skip_draws = getattr(config, "pretrain_skip_draws", None)
    if skip_draws is not None and not isinstance(skip_draws, bool):
        raise hip.XqError(f"config.pretrain_skip_draws must be a bool, got {skip_draws!r}")
    if not paths:
        return None
    games = []
    for p in paths:
        with open(p) as f:
            games.append(records_from_text(f.read()))
    return {"paths": [os.fspath(p) for p in paths], "epochs": epochs, "movers": movers, "skip_draws": bool(skip_draws),
            "records": np.concatenate(games)}


class AlphaZeroLoop:
    def __init__(self, config, device="cuda", seed: int = 0, evaluator_kind: str = "hip"):
        self.config = config
        self.device = torch.device(device)
        self.grouped = dist.is_initialized()           # collectives run under ANY initialised group, one rank included
        self.world = dist.get_world_size() if self.grouped else 1
        self.rank = dist.get_rank() if self.grouped else 0
        self.seed = seed
        self.evaluator_kind = evaluator_kind
        # the perpetual-check rule (config.perpetual_check_loses; absent: off), read once: self-play and the arena gate get this
        # one value, so a loop never trains under one rule and gates under the other
        self.perpetual_check = bool(getattr(config, "perpetual_check_loses", False))
        # the proven-result search (config.mcts_solver; absent: off), read once as well, for self-play and the gate alike
        self.solver = bool(getattr(config, "mcts_solver", False))
        # the settled-move cutoff (config.early_stop_decided; absent: off), read once and checked here, for the searches whose move
        # is played at temperature 0: the arena gate and the baseline, tactics and endgame yardsticks.  Never self-play
        self.early_stop = bool(getattr(config, "early_stop_decided", False))
        if self.early_stop and self.solver:
            raise hip.XqError("config.early_stop_decided and config.mcts_solver cannot be combined: the solver's move is the first "
                              "maximum of adjusted counts, not of the visit counts")
        self._decided = {"early_stop": True} if self.early_stop else {}     # off: every call is the call without the key
        # the q-mixed value target (config.value_target_q_mix = lambda, absent: 0; config.record_root_stats): checked here, so a
        # lambda outside [0, 1] or one with Gumbel root search fails at construction; lambda > 0 turns the recording on.  Read
        # once: self-play and the train step below are handed these two values and do not read the keys again
        self.q_mix = selfplay.root_stats_q_mix(config)
        self.record_root_stats = bool(getattr(config, "record_root_stats", False)) or self.q_mix > 0.0
        # the evaluation mirror (config.eval_random_mirror; absent: off), read once, for self-play ONLY: the arena gate never gets
        # it, so a gate's games stay a function of the two models and the seed
        self.eval_mirror = bool(getattr(config, "eval_random_mirror", False))
        # game records (config.record_games; absent: off), read once, for self-play and the gate alike; with
        # config.game_records_dir every iteration's games are written there as text (sample_format.records_to_text), per rank
        self.record_games = bool(getattr(config, "record_games", False))
        self.game_records_dir = getattr(config, "game_records_dir", None) if self.record_games else None
        # policy-surprise weighting (config.policy_surprise_weight = alpha, absent: 0) and the scoring pass on its own
        # (config.score_samples; absent: off), read once and checked here: either one has every shard of self-play scored against
        # the network that played it, before the all-gather, so the marks travel inside the records
        self.surprise_weight = selfplay.policy_surprise_weight(config)
        self.score_samples = bool(getattr(config, "score_samples", False)) or self.surprise_weight > 0.0
        self._shard_scores = None
        self._score_ev = None
        # merging the records of one position into one training sample (config.merge_duplicate_positions, absent: off;
        # config.merge_mirror_positions, absent: on), read once; the train step's stats carry the counts of every iteration
        # (distinct_positions, merged_records, largest_group) into training_stats.json
        self.merge_duplicates = training.merge_duplicate_positions(config)
        self.merge_mirror = training.merge_mirror_positions(config)
        if self.merge_duplicates and self.surprise_weight > 0.0:
            raise hip.XqError("config.merge_duplicate_positions and config.policy_surprise_weight > 0 cannot be combined")
        # the baseline gate (config.baseline_games; absent or 0: off), read once and checked here: every baseline_interval-th
        # iteration rank 0 plays best_model against the fixed alpha-beta opponent (baseline.py): no promotion, no collective
        self.baseline = _baseline_options(config)
        # the supervised warm start (config.pretrain_records; absent: off), read once and checked here, the game files included: a
        # fresh run trains current_model on their samples before iteration 1 (training.pretrain_from_records)
        self.pretrain = _pretrain_options(config)
        # the tactics yardstick (config.tactics_file; absent: off), read once and checked here, the file included: every
        # tactics_interval-th iteration rank 0 scores best_model on the file's forced mates (tactics.py): it decides nothing and
        # uses no collective.  The positions are labelled on the device at first use
        self.tactics = _tactics_options(config)
        self._tactics_puzzles = None
        # the endgame yardstick (config.endgame_signature; absent: off), read once and checked here: every endgame_interval-th
        # iteration rank 0 scores best_model on positions of the signature's tablebase (endgame.hold_rate): it decides nothing and
        # uses no collective.  With endgame_rescore every iteration's samples the table covers get their exact outcome before
        # they enter the buffer.  The table is generated on the device at first use
        self.endgame = _endgame_options(config)
        self._endgame_tb = None
        self._endgame_positions = None
        # the table as opponent and as teacher (config.endgame_playout_positions, config.endgame_teacher_samples; absent: off):
        # on the yardstick's iterations rank 0 also plays won entries out against the table's best defence (endgame.play_out), and
        # every iteration every rank appends the same table samples to its buffer after self-play's
        self.endgame_playout, self.endgame_teacher = _endgame_play_options(config)
        self._endgame_playout_positions = None
        # the start-position pool (config.start_positions_file, config.start_positions_endgame, config.start_positions_prob;
        # absent: off), read once and checked here, the file included: self-play starts that share of its games from the file's
        # positions and from entries of the endgame table, redrawn every iteration from seed + iteration with no rank term, so
        # every rank holds the same pool; the ranks' draws differ through Philox's rank word
        self.start_pool = _start_pool_options(config)
        self._shard_pool = (0, 0)
        # table adjudication (config.adjudicate_signatures, adjudicate_draws, adjudicate_min_ply; absent: off), read once and
        # checked here: a self-play game ends as soon as one of the signatures' tables decides its position.  The tables are
        # generated on the device at first use; a signature equal to endgame_signature shares that table.  Self-play only
        self.adjudicate = _adjudicate_options(config)
        self._adjudicate_tbs = None
        self._shard_adjudicated = (0, 0, 0)
        # the per-side resign rule (config.resign_per_side with resign_holdout_prob, resign_calibrate, resign_fp_target,
        # resign_min_pairs, resign_threshold_max; absent: off), read once and checked here: a side resigns on its own last
        # resign_check_steps root values, a share of the games is played out, and every iteration logs what the holdout says of
        # the threshold; with resign_calibrate the next iteration plays under the threshold it gives.  Self-play only
        self.resign = _resign_options(config)
        self.resign_threshold = None if self.resign is None else self.resign["threshold"]
        self._shard_resign = None
        self._iteration_resign = None
        torch.manual_seed(seed)                     # identical initial weights on every rank
        self.current_model = XiangqiNet(config.num_channels, config.num_res_blocks).to(self.device)
        self.best_model = copy.deepcopy(self.current_model)
        on_gpu = self.device.type == "cuda"
        from . import native_conv
        if on_gpu and native_conv.supported(config.num_channels):
            # train step on the hand-written kernels: tower convolutions (forward, data and weight gradient) and the fused
            # training-mode BatchNorm (native_conv.py); the deep copy above -- the self-play / arena model -- is not touched
            self.current_model.use_native_conv(True)
        # fused=True: the whole Adam update in one launch instead of torch's five foreach launches (same formula)
        self.optimizer = torch.optim.Adam(self.current_model.parameters(), lr=config.learning_rate,
                                          weight_decay=config.weight_decay, **({"fused": True} if on_gpu else {}))
        self.scheduler = torch.optim.lr_scheduler.MultiStepLR(self.optimizer, milestones=config.lr_milestones,
                                                              gamma=config.lr_gamma)
        self.buffer = training.ReplayBuffer(config.max_buffer_size, self.device)
        self.iteration = 0
        self.total_games = 0
        self.training_stats = []

    # ---- the three stages --------------------------------------------------------------------------------
    def _play_shard(self, n_games: int):
        """-> (samples uint8[n,640], results uint8[m,16]) on self.device."""
        if n_games <= 0:
            return (torch.empty((0, 640), dtype=torch.uint8, device=self.device),
                    torch.empty((0, 16), dtype=torch.uint8, device=self.device))
        samples, results, st, _ = selfplay.run_games(self.best_model, self.config, n_games, self.device,
                                                    seed=self.seed + 1000 * self.iteration, rank=self.rank,
                                                    evaluator_kind=self.evaluator_kind, device_records=True,
                                                    # leaf batching is a self-play option only: the arena stays sequential
                                                    leaves_per_step=int(getattr(self.config, "leaves_per_step", 1) or 1),
                                                    # forced playouts too (config.forced_playouts_k; absent or 0: off): the
                                                    # arena (arena.py) never takes it
                                                    forced_playouts=float(getattr(self.config, "forced_playouts_k", 0) or 0) or None,
                                                    perpetual_check=self.perpetual_check, solver=self.solver,
                                                    root_stats=self.record_root_stats, eval_mirror=self.eval_mirror,
                                                    record_games=self.record_games, start_pool=self._iteration_pool(),
                                                    **self._adjudicate_arg(), **self._resign_arg())
        if self.resign is not None:
            self._shard_resign = (st["resign_rows"], st["resign_resigned"], st["resign_holdout_games"], st["resign_rows_dropped"])
        if self.start_pool is not None:
            self._shard_pool = (st["start_pool"][0], st["start_pool_games"])
        if self.adjudicate is not None:
            self._shard_adjudicated = (st["adjudicated_games"], st["adjudicated_decisive"], st["adjudicated_drawn"])
        if self.record_games:
            self._write_records("selfplay", st["game_records"].cpu().numpy().reshape(-1).view(GAME_RECORD_DTYPE))
        # the Gumbel root search (config.gumbel_considered, gumbel_c_visit, gumbel_c_scale; absent or 0: off) reaches the engine
        # through run_games, which reads those keys from the config it is handed; the arena never takes it either
        if self.score_samples:
            self._shard_scores = selfplay.score_samples(self._scoring_evaluator(), samples, self.buffer.late_temperature,
                                                        write_back=True)     # the target the batch kernel trains on
        return samples, results

    def _iteration_pool(self):
        """This iteration's start-position pool as run_games takes it, or None: the file's positions, then the endgame table's
        entries of this iteration (every kind one can move from; as many as the table has when it has fewer)."""
        p = self.start_pool
        if p is None:
            return None
        boards, sides = p["boards"], p["sides"]
        if p["endgame"] is not None:
            from . import start_pool
            tb = self._endgame_table()
            have = int(((tb.table != -1) & (tb.table != hip.TB_INVALID)).sum())
            from .endgame import KINDS
            eb, es = start_pool.from_table(tb, min(p["endgame"], have), KINDS, seed=self.seed + self.iteration)
            boards, sides = np.concatenate([boards, eb]), np.concatenate([sides, es])
        return boards, sides, p["prob"]

    def _adjudicate_arg(self) -> dict:
        """run_games' `adjudicate` keyword, or nothing: with the keys absent the call is the call without it.  The tables are
        generated on self.device at first use and kept; the endgame yardstick's table serves its own signature."""
        a = self.adjudicate
        if a is None:
            return {}
        if self._adjudicate_tbs is None:
            from . import endgame
            tbs = []
            for sig in a["signatures"]:
                if self.endgame is not None and self.endgame["signature"] == sig:
                    tbs.append(self._endgame_table())
                else:
                    tbs.append(endgame.Tablebase.generate(sig, self.device))
            self._adjudicate_tbs = tuple(tbs)
        return {"adjudicate": (self._adjudicate_tbs, dict(draws=a["draws"], min_ply=a["min_ply"]))}

    def _resign_arg(self) -> dict:
        """run_games' `resign` keyword, or nothing: with the keys absent the call is the call without it."""
        r = self.resign
        if r is None:
            return {}
        return {"resign": dict(threshold=self.resign_threshold, check_steps=r["check_steps"], holdout_prob=r["holdout_prob"])}

    def _resign_entry(self) -> dict:
        """This iteration's "resign" entry, and the next threshold.  Every rank's holdout rows are gathered with the records'
        all-gather and the counters summed, so every rank computes the same entry from the same rows."""
        from . import resign as rsn
        from .sample_format import RESIGN_ROW_DTYPE
        r = self.resign
        rows, *counts = self._shard_resign if self._shard_resign is not None else (np.zeros(0, RESIGN_ROW_DTYPE), 0, 0, 0)
        if self.grouped:
            dev = self.device
            packed = torch.from_numpy(np.ascontiguousarray(rows).view(np.uint8).reshape(-1, RESIGN_ROW_DTYPE.itemsize).copy()).to(dev)
            rows = xdist.all_gather_records_device(packed).cpu().numpy().reshape(-1).view(RESIGN_ROW_DTYPE)
            total = torch.tensor(counts, dtype=torch.int64, device=dev)
            dist.all_reduce(total)
            counts = [int(v) for v in total.tolist()]
        below, bad = rsn.rate_below(rows, self.resign_threshold)
        nxt = rsn.calibrate(rows, r["fp_target"], r["min_pairs"], r["threshold_max"])
        entry = {"threshold": self.resign_threshold, "resigned": int(counts[0]), "holdout_games": int(counts[1]),
                 "rows_dropped": int(counts[2]), "pairs_below": below, "fp_rate": bad / below if below else None,
                 "calibrated_threshold": nxt, "calibrate": r["calibrate"]}
        if r["calibrate"]:
            self.resign_threshold = nxt
        return entry

    def _scoring_evaluator(self):
        """The evaluator of `best_model` that scores the shards: built once and kept (its activation and logits buffers with it);
        every iteration refreshes its weights in place, which is one more filter transform per iteration beside run_games' own."""
        if self._score_ev is None:
            from . import evaluator
            self._score_ev = evaluator.make_evaluator(self.best_model, self.device, self.evaluator_kind)[0]
        else:
            self._score_ev.update(self.best_model)
        return self._score_ev

    def _write_records(self, stage: str, records, folder=None) -> None:
        """This rank's game records of one stage of the current iteration, as text, when config.game_records_dir is set (`folder`:
        the directory of a stage that has records without config.record_games)."""
        folder = folder or self.game_records_dir
        if not folder:
            return
        os.makedirs(folder, exist_ok=True)
        name = "iter%04d_%s_rank%d.txt" % (self.iteration, stage, self.rank)
        with open(os.path.join(folder, name), "w") as f:
            f.write(records_to_text(records))

    def self_play(self) -> dict:
        cfg = self.config
        t0 = time.time()
        self._shard_scores = None
        self._shard_pool = (0, 0)
        self._shard_adjudicated = (0, 0, 0)
        self._shard_resign = None
        samples, results = self._play_shard(xdist.shard_games(cfg.num_games_per_iter, self.world, self.rank))
        self._iteration_resign = None if self.resign is None else self._resign_entry()
        pooled = {}
        if self.start_pool is not None:
            # every rank's pool is the same; the games started from it are summed over the ranks
            games = torch.tensor([self._shard_pool[1]], dtype=torch.int64, device=self.device)
            if self.grouped:
                dist.all_reduce(games)
            positions = len(self.start_pool["boards"]) + (self.start_pool["endgame"] or 0)
            pooled = {"start_pool_positions": self._shard_pool[0] or positions, "start_pool_games": int(games.item())}
        if self.adjudicate is not None:
            # the games the tables ended, summed over the ranks
            ended = torch.tensor(list(self._shard_adjudicated), dtype=torch.int64, device=self.device)
            if self.grouped:
                dist.all_reduce(ended)
            pooled.update(zip(("adjudicated_games", "adjudicated_decisive", "adjudicated_drawn"), (int(v) for v in ended.tolist())))
        scores = None
        if self.score_samples:
            # one score row per sample of this shard; a shard without games (or a _play_shard that does not score) has none, and
            # still takes part in the gather below: every rank runs the same collectives
            scores = self._shard_scores
            if scores is None or scores.shape[0] != samples.shape[0]:
                scores = torch.zeros((int(samples.shape[0]), 16), dtype=torch.uint8, device=samples.device)
        if self.grouped:
            samples = xdist.all_gather_records_device(samples)
            results = xdist.all_gather_records_device(results)
            if scores is not None:
                scores = xdist.all_gather_records_device(scores)
        rescored = {}
        if self.endgame is not None and self.endgame["rescore"]:
            # after the gather: every rank holds the same samples and the same table, so every buffer gets the same bytes
            from . import endgame
            host = np.ascontiguousarray(samples.cpu().numpy()).reshape(-1).view(SAMPLE_DTYPE)
            new, covered, changed = endgame.rescore_samples(host, self._endgame_table())
            if changed:
                samples = torch.from_numpy(new.view(np.uint8).reshape(-1, 640)).to(samples.device)
            rescored = {"endgame_covered": covered, "endgame_changed": changed}
        self.buffer.extend(samples)
        taught = {}
        if self.endgame_teacher is not None:
            # seeded by the loop's seed and the iteration, no rank term: every rank appends the same rows, so the buffers stay
            # identical without a collective
            tb = self._endgame_table()
            have = int(((tb.table != -1) & (tb.table != hip.TB_INVALID)).sum())
            index = tb.entries_of(n=min(self.endgame_teacher["samples"], have), seed=self.seed + self.iteration)[2]
            rows = tb.samples(index, self.endgame_teacher["policy"], as_tensor=True)
            self.buffer.extend(rows)
            taught = {"endgame_teacher_samples": int(rows.shape[0])}
        res = results.cpu().numpy().reshape(-1).view(RESULT_DTYPE) if len(results) else np.zeros(0, RESULT_DTYPE)
        self.total_games += len(res)
        wins = {1: 0, -1: 0, 0: 0}
        for r in res:
            wins[int(r["winner"])] += 1
        scored = selfplay.score_summary(scores, samples) if scores is not None else {}
        return {"games": len(res), "red_wins": wins[1], "black_wins": wins[-1], "draws": wins[0],
                "avg_steps": float(res["steps"].mean()) if len(res) else 0.0, "new_samples": 2 * int(samples.shape[0]),
                "total_time": time.time() - t0, "num_workers": self.world, "mode": "hip", "buffer_size": len(self.buffer), **scored,
                **rescored, **taught, **pooled}

    def train_network(self) -> dict:
        """World 1: the reference's step.  World > 1: the same full-batch update computed data-parallel -- every rank
        holds the same buffer and weights, takes its slice of every batch, SyncBatchNorm + bucketed gradient all-reduce
        (`training.train_network(ddp=True)`); `config.ddp = False` falls back to training on rank 0 alone.  Either way one
        flat weight broadcast from rank 0 closes the step, so the replicas cannot drift.  `config.native_sync_bn = True` (opt-in)
        runs the data-parallel step's synchronised BatchNorm on the hand-written kernels (`training.prepare_ddp(native_bn=True)`)."""
        stats = {}
        ddp = self.grouped and bool(getattr(self.config, "ddp", True)) and self.device.type == "cuda"
        # the batch order is a function of (seed, iteration): the same on every rank, and the same in a resumed run
        gen = torch.Generator().manual_seed(self.seed * 1000003 + 7919 * self.iteration + 17)
        if ddp or self.rank == 0:
            stats = training.train_network(self.current_model, self.optimizer, self.scheduler, self.buffer, self.config,
                                           generator=gen, ddp=ddp, native_bn=bool(getattr(self.config, "native_sync_bn", False)),
                                           q_mix=self.q_mix, surprise_weight=self.surprise_weight,
                                           merge_duplicates=self.merge_duplicates, merge_mirror=self.merge_mirror)
        if self.grouped:
            xdist.broadcast_weights(self.current_model, src=0, device=self.device)
        return stats

    def _arena(self) -> dict:
        if int(getattr(self.config, "arena_opening_plies", 0) or 0) > 0:
            # paired random openings (opt-in): another seed every iteration, so successive gates see different openings
            seed = int(getattr(self.config, "arena_seed", 0) or 0) + self.iteration
            return arena.evaluate_models(self.current_model, self.best_model, self.config, self.device, self.evaluator_kind,
                                         seed=seed, perpetual_check=self.perpetual_check, solver=self.solver,
                                         record_games=self.record_games, **self._decided)
        return arena.evaluate_models(self.current_model, self.best_model, self.config, self.device, self.evaluator_kind,
                                     perpetual_check=self.perpetual_check, solver=self.solver, record_games=self.record_games,
                                     **self._decided)

    def evaluate(self) -> dict:
        stats = self._arena()
        stats.pop("games", None)
        records = stats.pop("game_records", None)
        if records is not None:
            self._write_records("arena", records)
        if self.grouped:                               # one verdict for all replicas: rank 0's
            flag = torch.tensor([1 if stats["model_updated"] else 0], dtype=torch.int64,
                                device=self.device if dist.get_backend() == "nccl" else "cpu")
            dist.broadcast(flag, src=0)
            stats["model_updated"] = bool(flag.item())
        if stats["model_updated"]:
            self.best_model.load_state_dict(self.current_model.state_dict())
        else:
            self.current_model.load_state_dict(self.best_model.state_dict())
        return stats

    def _decided_search(self, simulations: int):
        """What the baseline match and the tactics pass search with: best_model, or under config.early_stop_decided an `MCTS` of
        it with early_stop=True and the options those calls would have given it (their signatures are closed; the endgame calls
        take the keyword)."""
        if not self.early_stop:
            return self.best_model
        from . import mcts
        return mcts.MCTS(self.best_model, int(simulations), float(self.config.c_puct), self.device, self.evaluator_kind,
                         seed=self.seed + self.iteration, perpetual_check=self.perpetual_check, solver=self.solver, early_stop=True)

    def play_baseline(self) -> dict:
        """best_model against the fixed alpha-beta opponent (baseline.play_vs_baseline), seed + iteration as the match's seed.
        The records go to config.game_records_dir, when set, like the other stages'; the rest is this iteration's "baseline"
        entry."""
        from . import baseline
        b = self.baseline
        out = baseline.play_vs_baseline(self._decided_search(b["simulations"]), b["games"], b["depth"], b["simulations"], opening_plies=b["opening_plies"],
                                        seed=self.seed + self.iteration, max_game_length=int(self.config.max_game_length),
                                        c_puct=float(self.config.c_puct), perpetual_check=self.perpetual_check, solver=self.solver,
                                        device=self.device, evaluator_kind=self.evaluator_kind)
        # the match keeps its records whatever config.record_games says: they are its state
        self._write_records("baseline", out["game_records"], getattr(self.config, "game_records_dir", None))
        return {k: out[k] for k in ("depth", "games", "wins", "losses", "draws", "win_rate", "win_rate_se", "seconds")}

    def score_tactics(self) -> dict:
        """best_model on the puzzles of config.tactics_file (tactics.solve_rate) under the loop's solver and perpetual-check
        values, seed + iteration as the search's seed -> this iteration's "tactics" entry.  The first call labels the file's
        positions with one mate search; a position without a mate in [1, tactics_max_moves] is dropped and counted."""
        from . import tactics
        t = self.tactics
        if self._tactics_puzzles is None:
            labelled = tactics.label(t["positions"]["board"], t["positions"]["side"], t["max_moves"], t["checks_only"],
                                     device=self.device)
            self._tactics_puzzles = tactics.select(labelled, t["max_moves"], 1, unique=False)
            t["dropped"] = len(labelled) - len(self._tactics_puzzles)
        out = tactics.solve_rate(self._decided_search(t["simulations"]), self._tactics_puzzles, t["simulations"], c_puct=float(self.config.c_puct),
                                 solver=self.solver, perpetual_check=self.perpetual_check, seed=self.seed + self.iteration,
                                 device=self.device, evaluator_kind=self.evaluator_kind)
        # by_mate_in keyed by text, as the JSON file holds it: the entry in memory equals the entry on disk
        return {**{k: out[k] for k in ("puzzles", "solved", "optimal", "solve_rate")},
                "by_mate_in": {str(m): v for m, v in out["by_mate_in"].items()}, "max_moves": t["max_moves"],
                "simulations": out["simulations"], "seconds": out["seconds"]}

    def _endgame_table(self):
        """The tablebase of config.endgame_signature, generated on self.device at first use and kept."""
        if self._endgame_tb is None:
            from . import endgame
            self._endgame_tb = endgame.Tablebase.generate(self.endgame["signature"], self.device)
        return self._endgame_tb

    def score_endgame(self) -> dict:
        """best_model on endgame_positions entries of kind endgame_kind of the signature's table (endgame.hold_rate) under the
        loop's solver and perpetual-check values, seed + iteration as the search's seed -> this iteration's "endgame" entry.  The
        first call generates the table and draws the positions (the loop's seed); a table with fewer such entries gives all of
        them."""
        from . import endgame
        e = self.endgame
        tb = self._endgame_table()
        if self._endgame_positions is None:
            t = tb.table
            have = int((t > 0).sum()) if e["kind"] == "win" else int((t == 0).sum())
            boards, sides, _ = tb.positions(e["kind"], min(e["positions"], have), seed=self.seed)
            self._endgame_positions = (boards, sides)
        out = endgame.hold_rate(self.best_model, tb, *self._endgame_positions, e["simulations"], c_puct=float(self.config.c_puct),
                                solver=self.solver, perpetual_check=self.perpetual_check, seed=self.seed + self.iteration,
                                evaluator_kind=self.evaluator_kind, **self._decided)
        return {"signature": e["signature"], "kind": e["kind"], **{k: v for k, v in out.items() if k != "chosen"}}

    def play_out_endgame(self) -> dict:
        """best_model playing endgame_playout_positions won entries of the signature's table out against the table's best
        defence (endgame.play_out) with the yardstick's simulations, under the loop's solver and perpetual-check values, seed +
        iteration as the search's seed -> this iteration's "endgame_playout" entry.  The first call draws the entries (the
        loop's seed); a table with fewer won entries gives all of them."""
        from . import endgame
        e, p = self.endgame, self.endgame_playout
        tb = self._endgame_table()
        if self._endgame_playout_positions is None:
            boards, sides, _ = tb.entries_of(("win",), min(p["positions"], int((tb.table > 0).sum())), seed=self.seed)
            self._endgame_playout_positions = (boards, sides)
        out = endgame.play_out(self.best_model, tb, *self._endgame_playout_positions, e["simulations"], max_plies=p["max_plies"],
                               c_puct=float(self.config.c_puct), solver=self.solver, perpetual_check=self.perpetual_check,
                               seed=self.seed + self.iteration, evaluator_kind=self.evaluator_kind, **self._decided)
        return {"signature": e["signature"], **{k: v for k, v in out.items() if k != "games"}}

    def pretrain_from_records(self) -> dict:
        """The supervised warm start of a fresh run: config.pretrain_epochs epochs of current_model on the samples of the games of
        config.pretrain_records (every ply after the opening of the movers chosen), then best_model takes the weights.  Every rank
        holds the same games and draws the batch order from the same seed, so every rank ends with the same weights and no
        collective is needed; the loop's scheduler is not stepped.  A record that does not convert is dropped and counted.
        -> the "pretrain" entry of the first iteration's stats."""
        p = self.pretrain
        t0 = time.time()
        gen = torch.Generator().manual_seed(self.seed * 1000003 + 17)
        info = {}
        epochs = training.pretrain_from_records(self.current_model, self.optimizer, p["records"], self.config, p["epochs"],
                                                invalid="drop", generator=gen, merge_duplicates=self.merge_duplicates,
                                                device=self.device, info=info, movers=p["movers"], skip_opening=True,
                                                skip_draws=p["skip_draws"])
        self.best_model.load_state_dict(self.current_model.state_dict())
        return {"games": info["games"], "samples": info["samples"], "invalid": info["invalid"], "epochs": p["epochs"],
                "policy_loss": [e["policy_loss"] for e in epochs], "value_loss": [e["value_loss"] for e in epochs],
                "seconds": time.time() - t0}

    def _save(self, iteration: int) -> None:
        if self.rank == 0:
            training.save_checkpoint(self.config.checkpoint_dir, iteration, self.current_model, self.best_model,
                                     self.optimizer, self.scheduler, self.total_games, is_best=True)
            b = self.buffer                            # beside the reference's files: the compact replay records, oldest first
            oldest = (b.head - b.count) % b.cap
            rec = torch.roll(b.store, -oldest, 0)[:b.count].cpu()
            torch.save({"iteration": iteration, "records": rec}, os.path.join(self.config.checkpoint_dir, "replay_buffer.pt"))

    def resume(self, path: str) -> dict:
        """`AlphaZeroTrainer.load_checkpoint` + `--resume` (train.py:569-579, 759-761): restore iteration, total_games, both
        models, optimizer and scheduler from `path` (a `checkpoint_iter*.pt` of this loop or of the reference; loaded with
        `weights_only=True`); `train()` then continues with iteration + 1.  If `replay_buffer.pt` of the same iteration lies
        beside the checkpoint the replay buffer is restored too (the reference restarts with an empty one), and so is the
        `training_stats.json` history up to that iteration.  Every rank of a multi-rank run calls this with the same file."""
        info = training.load_checkpoint(path, self.current_model, self.best_model, self.optimizer, self.scheduler,
                                        map_location=self.device)
        self.iteration = int(info["iteration"])
        self.total_games = int(info["total_games"])
        folder = os.path.dirname(os.path.abspath(path))
        info["replay_buffer_restored"] = False
        rb = os.path.join(folder, "replay_buffer.pt")
        if os.path.exists(rb):
            saved = torch.load(rb, map_location="cpu", weights_only=True)
            if int(saved.get("iteration", -1)) == self.iteration:
                self.buffer = training.ReplayBuffer(self.config.max_buffer_size, self.device)
                self.buffer.extend(saved["records"])
                info["replay_buffer_restored"] = True
        st = os.path.join(folder, "training_stats.json")
        if os.path.exists(st):
            try:
                with open(st) as f:
                    self.training_stats = [e for e in json.load(f) if int(e.get("iteration", 0)) <= self.iteration]
            except (ValueError, OSError):
                self.training_stats = []
        if self.resign is not None and self.resign["calibrate"]:
            # a resumed run plays on under the threshold its last logged iteration calibrated
            logged = [e["resign"] for e in self.training_stats if isinstance(e.get("resign"), dict)]
            if logged:
                self.resign_threshold = float(logged[-1]["calibrated_threshold"])
        return info

    # ---- train.py:581-638 ------------------------------------------------------------------------------------
    def train(self, num_iterations: Optional[int] = None) -> list:
        cfg = self.config
        last = num_iterations if num_iterations is not None else cfg.num_iterations
        pre = None
        if self.pretrain is not None and self.iteration == 0 and last >= 1:       # a fresh run: a resumed one has its weights
            pre = self.pretrain_from_records()
        for iteration in range(self.iteration + 1, last + 1):
            self.iteration = iteration
            t0 = time.time()
            sp = self.self_play()
            tr = self.train_network()
            ev = {}
            if iteration % 2 == 0 and len(self.buffer) >= cfg.min_buffer_size:
                ev = self.evaluate()
            bl = None
            if self.baseline is not None and self.rank == 0 and iteration % self.baseline["interval"] == 0:
                bl = self.play_baseline()
            tc = None
            if self.tactics is not None and self.rank == 0 and iteration % self.tactics["interval"] == 0:
                tc = self.score_tactics()
            eg = po = None
            if self.endgame is not None and self.rank == 0 and iteration % self.endgame["interval"] == 0:
                eg = self.score_endgame()
                if self.endgame_playout is not None:
                    po = self.play_out_endgame()
            if iteration % cfg.save_interval == 0:
                self._save(iteration)
            self.training_stats.append({"iteration": iteration, "time": time.time() - t0, "self_play": sp,
                                        "training": tr, "evaluation": ev, **({} if bl is None else {"baseline": bl}),
                                        **({} if tc is None else {"tactics": tc}),
                                        **({} if eg is None else {"endgame": eg}),
                                        **({} if po is None else {"endgame_playout": po}),
                                        **({} if pre is None else {"pretrain": pre}),
                                        **({} if self._iteration_resign is None else {"resign": self._iteration_resign})})
            pre = None
            if self.rank == 0:
                os.makedirs(cfg.checkpoint_dir, exist_ok=True)
                with open(os.path.join(cfg.checkpoint_dir, "training_stats.json"), "w") as f:
                    json.dump(self.training_stats, f, indent=2, default=str)
        if self.iteration > 0:
            self._save(self.iteration)                 # train.py:636-637: the final state is always on disk
        return self.training_stats
