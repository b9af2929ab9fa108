"""Compact training-sample format of the engine and its adapter to the reference's dense schema.

The engine emits 640-byte `xq_sample` records (include/xq_hip.h): board, side to move, z, and the root's
(action, visit-count) pairs.  The reference's schema -- `(state float32[15,10,9], pi float64[8100], z float)`
doubled by the left-right mirror (training/parallel_selfplay.py:97-99, 123-151) -- is 70 KB per sample; it is
materialised here, on the consumer, with the same numpy operations the reference uses, so dense values are
bit-identical for T = 1 and agree to rounding of numpy's pow for T = 0.3.  This is data-format code (host side of
the boundary), not part of the search path.
"""
from __future__ import annotations

from typing import List, Tuple

import numpy as np

ACTION_SPACE = 8100

SAMPLE_DTYPE = np.dtype([("board", np.int8, 90), ("side", np.int8), ("z", np.int8), ("n_moves", np.uint8),
                         ("late_temp", np.uint8), ("ply", np.uint16), ("reserved0", np.uint16),
                         ("reserved1", np.uint16), ("slot", np.uint32), ("game_seq", np.uint32), ("pad", np.uint8, 20),
                         ("actions", np.uint16, 128), ("visits", np.uint16, 128)])
RESULT_DTYPE = np.dtype([("slot", np.uint32), ("game_seq", np.uint32), ("winner", np.int8), ("reason", np.uint8),
                         ("steps", np.uint16), ("n_samples", np.uint16), ("reserved", np.uint16)])
assert SAMPLE_DTYPE.itemsize == 640 and RESULT_DTYPE.itemsize == 16
# xq_game_record: what an engine with record_games=True (xq_engine_init_gr) keeps of every finished game
RECORD_MAX_PLIES = 504
GAME_RECORD_DTYPE = np.dtype([("slot", np.uint32), ("game_seq", np.uint32), ("winner", np.int8), ("reason", np.uint8),
                              ("n_moves", np.uint16), ("opening_plies", np.uint16), ("n_samples", np.uint16),
                              ("moves", np.uint16, RECORD_MAX_PLIES)])
assert GAME_RECORD_DTYPE.itemsize == 1024 and GAME_RECORD_DTYPE.fields["moves"][1] == 16
# xq_sample_root_stats: what an engine with root_stats=True (xq_engine_init_rs) writes into a sample's `pad` bytes
ROOT_STATS_DTYPE = np.dtype([("root_q", np.float32), ("root_visits", np.uint32), ("has_root_stats", np.uint8),
                             ("zero", np.uint8, 11)])
assert ROOT_STATS_DTYPE.itemsize == SAMPLE_DTYPE["pad"].itemsize == 20 and SAMPLE_DTYPE.fields["pad"][1] == 108


def root_stats(samples: np.ndarray) -> np.ndarray:
    """The samples' `pad` bytes as ROOT_STATS_DTYPE records, one per sample (a copy when `pad` is not contiguous)."""
    pad = np.ascontiguousarray(np.asarray(samples)["pad"])
    return pad.view(ROOT_STATS_DTYPE).reshape(pad.shape[:-1])


def mixed_z(samples: np.ndarray, q_mix: float) -> np.ndarray:
    """The value target of xq_samples_to_batch_ex, float32 per sample: (1 - q_mix) z + q_mix root_q in float64 for a sample
    that carries root statistics, z for every other sample (and for all of them at q_mix = 0)."""
    q_mix = float(q_mix)
    if not 0.0 <= q_mix <= 1.0:
        raise ValueError(f"q_mix must be in [0, 1], got {q_mix}")
    samples = np.asarray(samples)
    z = samples["z"].astype(np.float64)
    if q_mix == 0.0:
        return z.astype(np.float32)
    rs = root_stats(samples)
    a = (1.0 - q_mix) * z
    b = q_mix * rs["root_q"].astype(np.float64)
    return np.where(rs["has_root_stats"] == 1, a + b, z).astype(np.float32)


def encode_planes(board: np.ndarray, side: int) -> np.ndarray:
    """XiangqiGame.get_state_for_nn (training/game.py:618-640) from a compact sample."""
    b = np.asarray(board, dtype=np.int8).reshape(10, 9)
    out = np.zeros((15, 10, 9), dtype=np.float32)
    for i in range(1, 8):
        out[i - 1] = (b == i * side)
        out[6 + i] = (b == -i * side)
    if side == 1:
        out[14] = 1.0
    return out


def dense_pi(actions: np.ndarray, visits: np.ndarray, temperature: float) -> np.ndarray:
    """MCTS._get_action_probs (training/mcts.py:190-206) from (action, visit) pairs, same numpy operations."""
    pi = np.zeros(ACTION_SPACE)
    pi[np.asarray(actions, dtype=np.int64)] = visits
    if temperature == 0:
        best = int(actions[int(np.argmax(visits))])
        pi = np.zeros(ACTION_SPACE)
        pi[best] = 1.0
    elif pi.sum() > 0:
        pi = pi ** (1.0 / temperature)
        pi /= pi.sum()
    return pi


def _flip_perm() -> np.ndarray:
    a = np.arange(ACTION_SPACE)
    frm, to = a // 90, a % 90
    fr, fc, tr, tc = frm // 9, frm % 9, to // 9, to % 9
    return ((fr * 9 + (8 - fc)) * 90 + (tr * 9 + (8 - tc))).astype(np.int64)


FLIP_PERM = _flip_perm()


def flip_sample(state: np.ndarray, pi: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """_augment_data (training/parallel_selfplay.py:137-151): mirror columns; pi'[flip(a)] = pi[a]."""
    flipped = np.zeros_like(pi)
    nz = np.nonzero(pi > 0)[0]
    flipped[FLIP_PERM[nz]] = pi[nz]
    return np.flip(state, axis=2).copy(), flipped


def to_reference_tuples(samples: np.ndarray, results: np.ndarray, late_temperature: float = 0.3,
                        augment: bool = True, q_mix: float = 0.0):
    """-> (all_data, per_game) where all_data is the reference's list of (state, pi, z) with each sample followed by
    its mirror image, games in result order, plies in order; per_game = [(winner, steps, n_samples)].  q_mix > 0: z is the
    mixed value target `mixed_z`, as the batch kernel materialises it."""
    all_data: List[tuple] = []
    per_game = []
    key = samples["slot"].astype(np.int64) << 32 | samples["game_seq"].astype(np.int64)
    for r in results:
        k = int(r["slot"]) << 32 | int(r["game_seq"])
        mine = samples[key == k]
        mine = mine[np.argsort(mine["ply"], kind="stable")]
        zs = mixed_z(mine, q_mix)
        for s, zq in zip(mine, zs):
            n = int(s["n_moves"])
            t = late_temperature if s["late_temp"] else 1.0
            state = encode_planes(s["board"], int(s["side"]))
            pi = dense_pi(s["actions"][:n], s["visits"][:n].astype(np.float64), t)
            z = float(zq)
            all_data.append((state, pi, z))
            if augment:
                fs, fp = flip_sample(state, pi)
                all_data.append((fs, fp, z))
        per_game.append((int(r["winner"]), int(r["steps"]), len(mine)))
    return all_data, per_game


def reachable_actions() -> np.ndarray:
    """Sorted action ids (from*90 + to) along which SOME piece on SOME square can ever move, whatever the position:
    rook/cannon/pawn/king lines (same row or column), knight jumps, one- and two-step diagonals (advisor, elephant;
    taken on the whole board, a superset of game.py:262-452 / game_core.pyx:185-330 for any placement, legal or not).
    2 550 of the 8 100 ids: the policy head only has to produce these columns for the engine, every other logit can
    never belong to a legal move."""
    acts = []
    for fr in range(10):
        for fc in range(9):
            for tr in range(10):
                for tc in range(9):
                    dr, dc = abs(tr - fr), abs(tc - fc)
                    if (dr, dc) == (0, 0):
                        continue
                    if dr == 0 or dc == 0 or (dr, dc) in ((1, 2), (2, 1), (1, 1), (2, 2)):
                        acts.append((fr * 9 + fc) * 90 + tr * 9 + tc)
    return np.array(sorted(acts), dtype=np.int64)


# ---- game records as text: one game per line, ICCS coordinate moves ---------------------------------------------------------
_RESULT_TEXT = {1: "1-0", -1: "0-1", 0: "1/2-1/2"}
_RESULT_WINNER = {v: k for k, v in _RESULT_TEXT.items()}
_RECORD_KEYS = ("reason", "opening_plies", "n_samples", "slot", "game_seq")


def action_to_iccs(action: int) -> str:
    """The project's action code (from * 90 + to, square = row * 9 + column, row 0 red's back rank) as an ICCS coordinate move:
    files a-i for columns 0-8, ranks 0-9 for rows 0-9, e.g. 1732 -> 'b2e2'."""
    a = int(action)
    if not 0 <= a < ACTION_SPACE:
        raise ValueError(f"no action code: {action}")
    f, t = divmod(a, 90)
    return "%s%d%s%d" % ("abcdefghi"[f % 9], f // 9, "abcdefghi"[t % 9], t // 9)


def iccs_to_action(move: str) -> int:
    if len(move) != 4 or move[0] not in "abcdefghi" or move[2] not in "abcdefghi" or not (move[1] + move[3]).isdigit():
        raise ValueError(f"no ICCS coordinate move: {move!r}")
    return (int(move[1]) * 9 + ord(move[0]) - 97) * 90 + int(move[3]) * 9 + ord(move[2]) - 97


def records_to_text(records: np.ndarray) -> str:
    """Game records (GAME_RECORD_DTYPE) as text, one game per line: the moves as ICCS coordinates in ply order, the result
    ('1-0' red won, '0-1' black won, '1/2-1/2'), then reason, opening_plies, n_samples, slot and game_seq as key=value.
    `records_from_text` reads it back exactly."""
    lines = []
    for r in np.asarray(records).reshape(-1):
        n = int(r["n_moves"])
        if n > RECORD_MAX_PLIES or int(r["winner"]) not in _RESULT_TEXT:
            raise ValueError(f"malformed game record: n_moves {n}, winner {int(r['winner'])}")
        words = [action_to_iccs(a) for a in r["moves"][:n]] + [_RESULT_TEXT[int(r["winner"])]]
        words += ["%s=%d" % (k, int(r[k])) for k in _RECORD_KEYS]
        lines.append(" ".join(words))
    return "".join(line + "\n" for line in lines)


def records_from_text(text: str) -> np.ndarray:
    """The inverse of `records_to_text`; blank lines and lines starting with '#' are skipped."""
    out = []
    for line in text.splitlines():
        words = line.split()
        if not words or words[0].startswith("#"):
            continue
        at = [i for i, w in enumerate(words) if w in _RESULT_WINNER]
        if len(at) != 1:
            raise ValueError(f"a game line holds exactly one result: {line!r}")
        rec = np.zeros((), dtype=GAME_RECORD_DTYPE)
        moves = [iccs_to_action(w) for w in words[:at[0]]]
        if len(moves) > RECORD_MAX_PLIES:
            raise ValueError(f"a game record holds at most {RECORD_MAX_PLIES} moves, got {len(moves)}")
        rec["n_moves"], rec["winner"] = len(moves), _RESULT_WINNER[words[at[0]]]
        rec["moves"][:len(moves)] = moves
        keys = dict(w.split("=", 1) for w in words[at[0] + 1:])
        if sorted(keys) != sorted(_RECORD_KEYS):
            raise ValueError(f"a game line carries the keys {_RECORD_KEYS}: {line!r}")
        for k in _RECORD_KEYS:
            rec[k] = int(keys[k])
        out.append(rec)
    return np.array(out, dtype=GAME_RECORD_DTYPE).reshape(-1)
