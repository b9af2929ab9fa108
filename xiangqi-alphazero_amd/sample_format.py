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
# xq_resign_row: what the per-side resign rule (xq_engine_resign) keeps of every finished holdout game: the lowest window of red
# and of black (+inf: none) and the ply each was first reached at
RESIGN_ROW_DTYPE = np.dtype([("slot", np.uint32), ("game_seq", np.uint32), ("level", np.float32, 2), ("level_ply", np.uint16, 2),
                             ("winner", np.int8), ("reason", np.uint8), ("plies", np.uint16), ("zero", np.uint32, 2)])
assert RESIGN_ROW_DTYPE.itemsize == 32
# xq_sample_root_stats: what an engine with root_stats=True (xq_engine_init_rs) writes into a sample's `pad` bytes
ROOT_STATS_DTYPE = np.dtype([("root_q", np.float32), ("root_visits", np.uint32), ("has_root_stats", np.uint8),
                             ("zero", np.uint8, 11)])
assert ROOT_STATS_DTYPE.itemsize == SAMPLE_DTYPE["pad"].itemsize == 20 and SAMPLE_DTYPE.fields["pad"][1] == 108
# xq_sample_policy_stats: what xq_score_samples(write_back = 1) writes into bytes 120..127 of a record, inside the zero bytes of
# ROOT_STATS_DTYPE; xq_sample_score: one row of its output
POLICY_STATS_OFFSET = 120
POLICY_STATS_DTYPE = np.dtype([("policy_kl", np.float32), ("has_policy_stats", np.uint8), ("prior_top1", np.uint8),
                               ("zero", np.uint8, 2)])
SCORE_DTYPE = np.dtype([("policy_kl", np.float32), ("policy_ce", np.float32), ("value", np.float32), ("top1", np.uint8),
                        ("valid", np.uint8), ("zero", np.uint8, 2)])
# the float64 reference of a score row (sample_scores): the entropy of the target rides along, ce - kl
SCORE_REF_DTYPE = np.dtype([("policy_kl", np.float64), ("policy_ce", np.float64), ("entropy", np.float64), ("value", np.float32),
                            ("top1", np.uint8), ("valid", np.uint8)])
assert POLICY_STATS_DTYPE.itemsize == 8 and SCORE_DTYPE.itemsize == 16
assert SAMPLE_DTYPE.fields["pad"][1] + ROOT_STATS_DTYPE.fields["zero"][1] <= POLICY_STATS_OFFSET \
    and POLICY_STATS_OFFSET + POLICY_STATS_DTYPE.itemsize <= SAMPLE_DTYPE.fields["pad"][1] + ROOT_STATS_DTYPE.itemsize
SURPRISE_KL_CAP = 64.0            # nats: the only cap on a sample's weight
SURPRISE_Q_SCALE = float(2 ** 20)
RNG_KIND_SURPRISE = 10            # XQ_RNG_KIND_SURPRISE: the Philox stream kind of the epoch counts' rounding draws


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


def policy_stats(samples: np.ndarray) -> np.ndarray:
    """Bytes 120..127 of the samples as POLICY_STATS_DTYPE records, one per sample (a copy): policy_kl, the mark
    has_policy_stats (1 where xq_score_samples wrote the record back) and prior_top1."""
    samples = np.asarray(samples)
    raw = np.ascontiguousarray(samples).view(np.uint8).reshape(samples.shape + (SAMPLE_DTYPE.itemsize,))
    ps = np.ascontiguousarray(raw[..., POLICY_STATS_OFFSET:POLICY_STATS_OFFSET + POLICY_STATS_DTYPE.itemsize])
    return ps.view(POLICY_STATS_DTYPE).reshape(samples.shape)


def sample_scores(samples: np.ndarray, legal_logits: np.ndarray, value: np.ndarray, late_temperature: float = 0.3) -> np.ndarray:
    """The float64 reference of xq_score_samples, SCORE_REF_DTYPE per sample: legal_logits[j][:n_moves] are a network's logits of
    the sample's moves, value[j] its value.  Target t = w / sum w with w = visits^(1/T) for late_temp records and the plain visits
    otherwise; logp = log_softmax of the n_moves logits; ce = -sum t logp, kl = max(0, sum t (log t - logp)) over t > 0,
    entropy = -sum t log t; top1 = the first largest logit is the first largest visit count.  A sample without moves, without
    visits, with a total that is not finite or with a logit among its moves that is not finite is invalid: valid = 0 and zeros."""
    samples = np.asarray(samples).reshape(-1)
    legal_logits, value = np.asarray(legal_logits), np.asarray(value)
    out = np.zeros(len(samples), dtype=SCORE_REF_DTYPE)
    for j, s in enumerate(samples):
        m = min(int(s["n_moves"]), 128)
        c = s["visits"][:m].astype(np.float64)
        lg = legal_logits[j][:m].astype(np.float64)
        if s["late_temp"]:
            with np.errstate(over="ignore"):            # a small T overflows the powers: the total is then not finite
                w = np.where(c > 0.0, c ** (1.0 / float(late_temperature)), 0.0)
        else:
            w = c
        total = 0.0
        for x in w:                                     # the kernels' sequential sum in move order
            total += float(x)
        if m == 0 or not total > 0.0 or not np.isfinite(total) or not np.isfinite(lg).all():
            continue
        t = w / total
        mx = lg.max()
        logp = lg - mx - np.log(np.exp(lg - mx).sum())
        nz = t > 0.0
        ent = float(-(t[nz] * np.log(t[nz])).sum())
        out[j] = (max(0.0, float((t[nz] * (np.log(t[nz]) - logp[nz])).sum())), float(-(t[nz] * logp[nz]).sum()), ent,
                  np.float32(value[j]), int(np.argmax(lg)) == int(np.argmax(s["visits"][:m])), 1)
    return out


def _philox_u64(seed: int, rank, slot, kind: int, ctr, sub) -> np.ndarray:
    """The engine's Philox4x32-10 (philox_u64 of csrc/xq_engine_state.cuh) over arrays: key = the two halves of `seed`, counter
    words (slot, kind | sub << 8, ctr, rank); output word 0 in the high half, word 1 in the low half."""
    m32 = np.uint64(0xFFFFFFFF)
    slot, ctr, sub = (np.asarray(a).astype(np.uint64) for a in (slot, ctr, sub))
    c0, c2 = slot & m32, ctr & m32
    c1 = (np.uint64(kind) | (sub << np.uint64(8))) & m32
    c3 = np.full_like(c0, np.uint64(int(rank) & 0xFFFFFFFF))
    k0, k1 = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = ((p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0)) & m32, p1 & m32, \
            ((p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1)) & m32, p0 & m32
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return (c0 << np.uint64(32)) | c1


def surprise_q(policy_kl: np.ndarray) -> np.ndarray:
    """q of xq_surprise_counts, uint64: the KL capped at 64 nats in units of 2^-20 nat, rounded to nearest even; a KL that is
    negative or NaN counts 0."""
    kl = np.asarray(policy_kl, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        x = np.where(kl >= 0, np.minimum(kl, np.float32(SURPRISE_KL_CAP)), np.float32(0.0)).astype(np.float32)
    return np.rint(x.astype(np.float64) * SURPRISE_Q_SCALE).astype(np.uint64)


def surprise_weights(samples: np.ndarray, alpha: float):
    """-> (w float64 per record, marked bool per record, M, S) of xq_surprise_counts: w = (1 - alpha) + alpha q M / S over the
    marked records, 1.0 for an unmarked one and for all of them when S = 0."""
    alpha = float(alpha)
    if not 0.0 <= alpha <= 1.0:
        raise ValueError(f"alpha must be in [0, 1], got {alpha}")
    ps = policy_stats(np.asarray(samples).reshape(-1))
    marked = ps["has_policy_stats"] == 1
    q = np.where(marked, surprise_q(ps["policy_kl"]), np.uint64(0)).astype(np.uint64)
    M, S = int(marked.sum()), int(sum(int(x) for x in q))
    w = np.ones(len(ps), dtype=np.float64)
    if S > 0:
        ratio = (q.astype(np.float64) * float(M)) / float(S)
        w = np.where(marked, (1.0 - alpha) + alpha * ratio, 1.0)
    return w, marked, M, S


def surprise_counts(samples: np.ndarray, alpha: float, seed: int, epoch: int) -> np.ndarray:
    """The numpy reference of xq_surprise_counts, int32 per record: c = floor(w) + (u < w - floor(w)) with `surprise_weights`' w
    and u = (philox_u64(seed, epoch, slot, 10, game_seq, ply) >> 11) * 2^-53 -- a draw keyed by the record's identity, so a record
    keeps its rounding decision wherever it lies in a buffer.  It repeats the host twin xq_surprise_count_host."""
    samples = np.asarray(samples).reshape(-1)
    w, _, _, _ = surprise_weights(samples, alpha)
    r = _philox_u64(seed, int(epoch), samples["slot"], RNG_KIND_SURPRISE, samples["game_seq"], samples["ply"])
    u = (r >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    fl = np.floor(w)
    return (fl + (u < w - fl)).astype(np.int32)


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


# ---- positions as text: the standard Xiangqi FEN ---------------------------------------------------------------------------
_FEN_LETTERS = "KABNRCP"          # piece codes 1..7; red is upper case
_FEN_READ = {**{c: i + 1 for i, c in enumerate(_FEN_LETTERS)}, "E": 3, "H": 4}
_FEN_SIDES = {"w": 1, "r": 1, "b": -1}


def board_to_fen(board, side: int) -> str:
    """A position as a Xiangqi FEN: ranks 9 down to 0 (row 0 is red's back rank) separated by '/', files a-i for columns 0-8
    (`action_to_iccs`'s squares), red in upper case (K A B N R C P for codes 1..7), runs of empty squares as digits, then 'w'
    when red is to move and 'b' when black is."""
    b = np.asarray(board, dtype=np.int64).reshape(10, 9)
    if int(side) not in (1, -1) or (np.abs(b) > 7).any():
        raise ValueError(f"no position: side {side!r}, pieces {int(b.min())}..{int(b.max())}")
    ranks = []
    for r in range(9, -1, -1):
        text, run = "", 0
        for p in b[r].tolist():
            if p == 0:
                run += 1
                continue
            text += (str(run) if run else "") + (_FEN_LETTERS[p - 1] if p > 0 else _FEN_LETTERS[-p - 1].lower())
            run = 0
        ranks.append(text + (str(run) if run else ""))
    return "/".join(ranks) + (" w" if int(side) == 1 else " b")


def board_from_fen(text: str):
    """-> (board int8[90], side): the inverse of `board_to_fen`.  Reading also takes E for B and H for N, 'w', 'r' or 'b' for
    the side, and ignores the fields behind it.  A malformed line raises ValueError naming it."""
    words = str(text).split()
    if len(words) < 2 or words[1] not in _FEN_SIDES:
        raise ValueError(f"a FEN line holds a board and a side (w, r or b): {text!r}")
    ranks = words[0].split("/")
    if len(ranks) != 10:
        raise ValueError(f"a FEN board holds 10 ranks: {text!r}")
    board = np.zeros((10, 9), dtype=np.int8)
    for k, rank in enumerate(ranks):
        c = 0
        for ch in rank:
            if ch in "123456789":
                c += int(ch)
                continue
            if ch.upper() not in _FEN_READ or c >= 9:
                raise ValueError(f"rank {9 - k} of a FEN board is malformed: {text!r}")
            board[9 - k, c] = _FEN_READ[ch.upper()] * (1 if ch.isupper() else -1)
            c += 1
        if c != 9:
            raise ValueError(f"rank {9 - k} of a FEN board does not hold 9 files: {text!r}")
    return board.reshape(90), _FEN_SIDES[words[1]]


# ---- merging the records of one position (xq_position_keys, xq_position_group_heads, xq_groups_to_batch) --------------------
POSITION_KEY_MIRROR = 1           # XQ_POSITION_KEY_MIRROR
MIR_SQ = np.array([(sq // 9) * 9 + 8 - sq % 9 for sq in range(90)], dtype=np.int64)      # mir(sq) of the header


def _key_mix(x: np.ndarray) -> np.ndarray:
    """mix(x) of the header over a uint64 array (numpy's uint64 arithmetic wraps around)."""
    x = x ^ (x >> np.uint64(30))
    x = x * np.uint64(0xBF58476D1CE4E5B9)
    x = x ^ (x >> np.uint64(27))
    x = x * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def _key_term(i: np.ndarray, b: np.ndarray) -> np.ndarray:
    """term(i, b) = mix(0x9E3779B97F4A7C15 * (uint64)(i * 256 + (uint8)b + 1))."""
    arg = np.asarray(i, dtype=np.uint64) * np.uint64(256) + np.asarray(b, dtype=np.int8).view(np.uint8).astype(np.uint64) + np.uint64(1)
    return _key_mix(np.uint64(0x9E3779B97F4A7C15) * arg)


def canonical_board(board: np.ndarray, mirror: bool = True):
    """-> (canonical board int8[90], mirrored 0 / 1): with `mirror`, the board or its left-right mirror image, whichever has the
    smaller int8 at the first square where the two differ (a board that is its own image: itself, mirrored = 0)."""
    b = np.asarray(board, dtype=np.int8).reshape(90)
    if not mirror:
        return b, 0
    m = b[MIR_SQ]
    diff = np.nonzero(b != m)[0]
    if len(diff) == 0:
        return b, 0
    sq = int(diff[0])
    mirrored = 1 if int(m[sq]) < int(b[sq]) else 0
    return (m if mirrored else b), mirrored


def position_key(board: np.ndarray, side: int, mirror: bool = True):
    """The numpy reference of xq_position_keys / xq_position_key_host -> (key as a Python int in [0, 2^64), mirrored 0 / 1):
    key = XOR over sq < 90 of term(sq, c[sq]), then ^ term(90, side), over the canonical board c."""
    c, mirrored = canonical_board(board, mirror)
    with np.errstate(over="ignore"):
        terms = _key_term(np.arange(90), c)
        key = np.bitwise_xor.reduce(terms) ^ _key_term(np.array([90]), np.array([side], dtype=np.int8))[0]
    return int(key), mirrored


def position_group_heads(samples: np.ndarray, order: np.ndarray, keys: np.ndarray, mirrored: np.ndarray) -> np.ndarray:
    """The numpy reference of xq_position_group_heads, uint8 per sorted place: row order[j] starts a group iff j == 0 or its key,
    its side or its canonical board differs from that of row order[j - 1].  Keys and mirrored flags are taken as given."""
    samples = np.asarray(samples).reshape(-1)
    head = np.ones(len(order), dtype=np.uint8)
    for j in range(1, len(order)):
        r, p = int(order[j]), int(order[j - 1])
        if int(keys[r]) != int(keys[p]) or samples["side"][r] != samples["side"][p]:
            continue
        ca = samples["board"][r][MIR_SQ] if mirrored[r] else samples["board"][r]
        cb = samples["board"][p][MIR_SQ] if mirrored[p] else samples["board"][p]
        head[j] = 0 if np.array_equal(ca, cb) else 1
    return head


def position_groups(samples: np.ndarray, mirror: bool = True, keys=None):
    """The numpy reference of the grouping -> (offsets int32[n_groups + 1], members int32[n], member_mirrored uint8[n]): the rows
    (oldest first) are sorted stably by key, the heads found by the predecessor rule, the groups numbered by the age of their
    oldest member; members of a group are in age order.  `keys` replaces the computed keys (a test's made-up equal keys); the
    mirrored flags are always the computed ones."""
    samples = np.asarray(samples).reshape(-1)
    n = len(samples)
    km = [position_key(s["board"], int(s["side"]), mirror) for s in samples]
    mirrored = np.array([m for _, m in km], dtype=np.uint8).reshape(n)
    if keys is None:
        keys = np.array([k for k, _ in km], dtype=np.uint64).reshape(n)
    keys = np.asarray(keys, dtype=np.uint64)
    order = np.argsort(keys, kind="stable")
    head = position_group_heads(samples, order, keys, mirrored)
    gid_sorted = np.cumsum(head, dtype=np.int64) - 1                     # group of sorted place j, in sorted numbering
    n_groups = int(gid_sorted[-1]) + 1 if n else 0
    first_row = order[head == 1]                                         # the oldest member of each group: the sort is stable
    label = np.empty(n_groups, dtype=np.int64)
    label[np.argsort(first_row, kind="stable")] = np.arange(n_groups)
    row_label = np.empty(n, dtype=np.int64)
    row_label[order] = label[gid_sorted] if n else []
    members = np.argsort(row_label, kind="stable").astype(np.int32)     # by group, age order inside a group
    sizes = np.bincount(row_label, minlength=n_groups)
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    return offsets, members, mirrored[members]


def member_target(s, flip: bool, late_temperature: float):
    """One record's policy target as xq_samples_to_batch forms it before its cast -> (actions int64[m] under `flip`,
    t float64[m], total): w = visits, or visits^(1/T) for a late-temperature record; total = their sequential sum in move order;
    t = w / total (zeros when total is not above 0).  n_moves above 128 reads as 128; an action id >= 8100 is dropped."""
    m = min(int(s["n_moves"]), 128)
    c = s["visits"][:m].astype(np.float64)
    if s["late_temp"]:
        with np.errstate(over="ignore"):
            w = np.where(c > 0.0, c ** (1.0 / float(late_temperature)), 0.0)
    else:
        w = c
    total = 0.0
    for x in w:
        total += float(x)
    with np.errstate(invalid="ignore", divide="ignore"):
        t = w / total if total > 0.0 else np.zeros(m)
    a = s["actions"][:m].astype(np.int64)
    keep = a < ACTION_SPACE
    a, t = a[keep], t[keep]
    return (FLIP_PERM[a] if flip else a), t, total


def merged_targets(samples: np.ndarray, groups, group: np.ndarray, flip: np.ndarray, late_temperature: float = 0.3,
                   q_mix: float = 0.0):
    """The numpy reference of xq_groups_to_batch -> (states float32[n,15,10,9], pi float32[n,8100], z float32[n]).  `groups` =
    (offsets, members, member_mirrored) as `position_groups` returns them, members indexing `samples`; output row j is group
    group[j] under flip[j].  Member k enters under orientation o_k = member_mirrored_k XOR flip: planes of member 0 under o_0;
    pi = (float32)((0.0 + t_0 + t_1 + ...) / n_pi) over the valid members (total > 0) in member order, float64; z =
    (float32)((0.0 + zt_0 + ...) / n) with zt the float64 value of `mixed_z` before its cast.  A group id outside
    [0, n_groups) and an empty group give zeros."""
    samples = np.asarray(samples).reshape(-1)
    offsets, members, member_mirrored = (np.asarray(a) for a in groups)
    q_mix = float(q_mix)
    if not 0.0 <= q_mix <= 1.0:
        raise ValueError(f"q_mix must be in [0, 1], got {q_mix}")
    n, n_groups = len(group), len(offsets) - 1
    states = np.zeros((n, 15, 10, 9), dtype=np.float32)
    pi = np.zeros((n, ACTION_SPACE), dtype=np.float32)
    z = np.zeros(n, dtype=np.float32)
    for j in range(n):
        g = int(group[j])
        if not 0 <= g < n_groups or offsets[g + 1] <= offsets[g]:
            continue
        f = bool(flip[j])
        mem = [(samples[int(members[i])], bool(member_mirrored[i]) != f) for i in range(int(offsets[g]), int(offsets[g + 1]))]
        s0, o0 = mem[0]
        st = encode_planes(s0["board"], int(s0["side"]))
        states[j] = np.flip(st, axis=2) if o0 else st
        acc = np.zeros(ACTION_SPACE)
        zsum, n_pi = 0.0, 0
        for s, o in mem:
            a, t, total = member_target(s, o, late_temperature)
            if total > 0.0:
                n_pi += 1
                acc[a] = acc[a] + t                   # a dense sum: a member adds 0.0 at every action it does not name
            zt = float(s["z"])
            if q_mix != 0.0:
                rs = root_stats(np.asarray(s).reshape(1))[0]
                if rs["has_root_stats"] == 1:
                    zt = (1.0 - q_mix) * float(s["z"]) + q_mix * float(np.float64(rs["root_q"]))
            zsum += zt
        if n_pi:
            pi[j] = (acc / float(n_pi)).astype(np.float32)
        z[j] = np.float32(zsum / float(len(mem)))
    return states, pi, z
