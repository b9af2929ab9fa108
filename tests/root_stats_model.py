"""Host model of the root statistics per sample (include/xq_hip.h, xq_engine_init_rs).  TEST INFRASTRUCTURE ONLY.

The game is tests/selfplay_model.py's, untouched: `play_game` here hands it an `on_move` callback that reads the finished search's
raw tree arrays -- before forced-playout pruning and before the solver's rule-5 counts -- and repeats the header's arithmetic:

    sumW = 0.0 (double), sumN = 0;  for the root's children in move order: sumW += W[i]; sumN += N[i]
    root_q = proven ? 1.0f : (sumN > 0 ? (float)(sumW / (double)sumN) : 0.0f)

`proven` is the solver's rule 4 (the sample's own `proven` mark); a fast move of the playout cap stages no sample, so its root
statistics are dropped (`stats["moves"][k]["full"]`).  Every sample of the returned game carries `root_q` (np.float32) and
`root_visits` (int) next to the fields selfplay_model gives it.
"""
from __future__ import annotations

import hashlib

import numpy as np

import selfplay_model as SP


def root_sums(search):
    """(sumW, sumN) over the root's children of a finished search, one sequential scan in move order."""
    first, nch = int(search.first[0]), int(search.nch[0])
    sum_w, sum_n = 0.0, 0
    for i in range(first, first + nch):
        sum_w += float(search.W[i])
        sum_n += int(search.N[i])
    return sum_w, sum_n


def root_q_of(sum_w: float, sum_n: int, proven: bool) -> np.float32:
    if proven:
        return np.float32(1.0)
    return np.float32(sum_w / float(sum_n)) if sum_n > 0 else np.float32(0.0)


def play_game(cfg: dict, peaked: bool, draws, **options):
    """selfplay_model.play_game(cfg, peaked, draws, **options) -> (samples, winner, plies, stats), every sample with `root_q` and
    `root_visits`."""
    sums = []
    samples, winner, plies, stats = SP.play_game(cfg, peaked, draws, on_move=lambda s, c, kept, g: sums.append(root_sums(s)),
                                                 **options)
    assert len(sums) == len(stats["moves"])
    full = [sm for sm, mv in zip(sums, stats["moves"]) if mv["full"]]
    assert len(full) == len(samples)
    for smp, (sum_w, sum_n) in zip(samples, full):
        smp["root_q"] = root_q_of(sum_w, sum_n, bool(smp["proven"]))
        smp["root_visits"] = sum_n
    return samples, winner, plies, stats


def pad_bytes(sample: dict) -> bytes:
    """The 20 bytes the engine writes at offset 108 of the sample's record."""
    return np.float32(sample["root_q"]).tobytes() + np.uint32(sample["root_visits"]).tobytes() + b"\x01" + bytes(11)


def digest(samples) -> str:
    """sha256 over (root_q bits, root_visits) of a game's samples, in order."""
    h = hashlib.sha256()
    for s in samples:
        h.update(np.float32(s["root_q"]).tobytes() + np.uint32(s["root_visits"]).tobytes())
    return h.hexdigest()
