"""Endgame tablebases: exact values of the endings with up to five pieces beside the kings, and a yardstick built on them
(DESIGN.md section 4.21).

The arena gate is relative, the alpha-beta baseline positional and the tactics file asks about short forced mates; none says
whether a network plus S simulations wins a won ending or holds a drawn one.  A table (`hip.tb_generate`, include/xq_hip.h:
xq_tb_*) holds one int16 per entry of a dense index over a signature's positions: 0 a draw, +p a win in p plies, -(p + 1) a loss
in p plies, from the view of the side to move, under the move generator's rules alone.

`parse_signature`, `index_to_board` and `board_to_index` are the numpy reference of the index layout, vectorised over an index
array.  `Tablebase` generates, saves, loads, probes and draws positions.  `hold_rate` runs one search-only `MCTS` over positions
of a table (`search_many`: move count 0, no history, no noise) and asks the probe about the move the search chose.
`rescore_samples` replaces the game outcome of every sample the table covers by the exact one.

The table is also an opponent and a teacher.  `Tablebase.play` applies one move per position on the
device, the table's best or the caller's; `play_out_with` plays won endings out against the table's best defence, and `play_out`
does so with one search-only `MCTS` choosing the winner's moves.  `Tablebase.entries_of` draws entries, and `Tablebase.samples`
turns them into training samples whose policy target is the optimal moves and whose value target is the exact outcome."""
from __future__ import annotations

import time
from typing import Dict

import numpy as np
import torch

from . import hip
from .sample_format import SAMPLE_DTYPE

LAYOUT_VERSION = 1
INVALID = hip.TB_INVALID
NO_MOVE = hip.TB_NO_MOVE
KINDS = ("win", "draw", "loss")
_LETTERS = {2: "A", 3: "B", 4: "N", 5: "R", 6: "C", 7: "P"}


def _red_admissible(kind: int, s: int) -> bool:
    r, c = divmod(s, 9)
    if kind == 2:
        return (r, c) in ((0, 3), (0, 5), (1, 4), (2, 3), (2, 5))
    if kind == 3:
        return (r, c) in ((0, 2), (0, 6), (2, 0), (2, 4), (2, 8), (4, 2), (4, 6))
    if kind == 7:
        return r >= 5 or (r in (3, 4) and c % 2 == 0)
    return True


def piece_squares(code: int) -> np.ndarray:
    """The admissible squares of a piece code in row-major order: digit d of the piece stands for square piece_squares(code)[d];
    black's squares are the 180-degree rotation of red's."""
    kind = abs(int(code))
    return np.array([s for s in range(90) if _red_admissible(kind, s if code > 0 else 89 - s)], dtype=np.int64)


RED_KING_SQUARES = np.array([r * 9 + c for r in range(0, 3) for c in range(3, 6)], dtype=np.int64)
BLACK_KING_SQUARES = np.array([r * 9 + c for r in range(7, 10) for c in range(3, 6)], dtype=np.int64)


def parse_signature(signature):
    """-> the signed piece codes of a signature (`hip.tb_signature`: a string of FEN letters or a sequence of codes)."""
    return hip.tb_signature(signature, "parse_signature")


def signature_text(signature) -> str:
    """The signature as FEN letters, in its own order."""
    return "".join(_LETTERS[abs(c)] if c > 0 else _LETTERS[abs(c)].lower() for c in parse_signature(signature))


def radices(signature):
    """-> the radix of every digit, most significant first: side, red king, black king, then squares + 1 per piece."""
    return [2, 9, 9] + [len(piece_squares(c)) + 1 for c in parse_signature(signature)]


def entries(signature) -> int:
    """The entry count from the layout alone (`hip.tb_entries` asks the library)."""
    n = 1
    for r in radices(signature):
        n *= r
    return n


def index_to_digits(signature, index) -> np.ndarray:
    """int64[n, 3 + P]: the digits of every index, most significant first."""
    idx = np.asarray(index, dtype=np.int64).reshape(-1).copy()
    rad = radices(signature)
    if len(idx) and (idx.min() < 0 or idx.max() >= entries(signature)):
        raise hip.XqError(f"index_to_digits: an index outside [0, {entries(signature)})")
    out = np.zeros((len(idx), len(rad)), dtype=np.int64)
    for j in range(len(rad) - 1, -1, -1):
        out[:, j] = idx % rad[j]
        idx //= rad[j]
    return out


def index_to_board(signature, index, return_collisions: bool = False):
    """-> (boards int8[n, 90], sides int8[n]) of the entries `index`; with return_collisions also bool[n]: two men of the entry
    stand on one square (the board then shows the later one, and the entry is no position)."""
    codes = parse_signature(signature)
    dig = index_to_digits(signature, index)
    n = len(dig)
    rows = np.arange(n)
    boards = np.zeros((n, 90), dtype=np.int8)
    collide = np.zeros(n, dtype=bool)
    boards[rows, RED_KING_SQUARES[dig[:, 1]]] = 1
    boards[rows, BLACK_KING_SQUARES[dig[:, 2]]] = -1
    for p, code in enumerate(codes):
        sqs = piece_squares(code)
        d = dig[:, 3 + p]
        on = d < len(sqs)
        sq = sqs[np.minimum(d, len(sqs) - 1)]
        collide |= on & (boards[rows, sq] != 0)
        boards[rows[on], sq[on]] = code
    sides = np.where(dig[:, 0] == 0, 1, -1).astype(np.int8)
    return (boards, sides, collide) if return_collisions else (boards, sides)


def board_to_index(signature, boards, sides) -> np.ndarray:
    """int64[n]: the index of every position, -1 where the table does not cover it (a king missing, a piece the signature lacks,
    a piece on a square outside its list).  The board is matched greedily in signature order: the r-th piece of a code in the
    signature takes the r-th such piece of the board in row-major order; a signature piece absent from the board is captured."""
    codes = parse_signature(signature)
    b = np.asarray(boards, dtype=np.int8).reshape(-1, 90)
    s = np.asarray(sides, dtype=np.int64).reshape(-1)
    if len(b) != len(s):
        raise hip.XqError(f"board_to_index: {len(b)} boards and {len(s)} sides")
    n = len(b)
    ok = np.ones(n, dtype=bool)
    idx = np.where(s == 1, 0, 1).astype(np.int64)
    for squares, code in ((RED_KING_SQUARES, 1), (BLACK_KING_SQUARES, -1)):
        at = b[:, squares] == code
        ok &= at.any(axis=1)
        idx = idx * 9 + at.argmax(axis=1)
    matched = np.zeros(n, dtype=np.int64)
    for p, code in enumerate(codes):
        sqs = piece_squares(code)
        digit_of = np.full(90, -1, dtype=np.int64)
        digit_of[sqs] = np.arange(len(sqs))
        rank = sum(1 for q in codes[:p] if q == code)
        is_p = b == code
        hit = is_p & (np.cumsum(is_p, axis=1) == rank + 1)
        present = hit.any(axis=1)
        d = np.where(present, digit_of[hit.argmax(axis=1)], len(sqs))
        ok &= d >= 0
        matched += present
        idx = idx * (len(sqs) + 1) + np.maximum(d, 0)
    ok &= (b != 0).sum(axis=1) == matched + 2
    return np.where(ok, idx, -1)


def _positions(boards, sides):
    b = np.ascontiguousarray(np.asarray(boards, dtype=np.int8)).reshape(-1, 90)
    s = np.ascontiguousarray(np.asarray(sides, dtype=np.int8)).reshape(-1)
    if len(b) != len(s):
        raise hip.XqError(f"endgame: {len(b)} boards and {len(s)} sides")
    return b, s


class Tablebase:
    """One signature's table on the host (`table`, int16[entries]) and, once a probe needs it, on the device."""

    def __init__(self, signature, table, passes: int = 0, device="cuda"):
        self.codes = parse_signature(signature)
        self.signature = signature_text(self.codes)
        t = np.ascontiguousarray(np.asarray(table))
        if t.dtype != np.int16 or t.ndim != 1 or len(t) != entries(self.codes):
            raise hip.XqError(f"Tablebase: the table of {self.signature!r} holds {entries(self.codes)} int16 entries, got "
                              f"{t.dtype}{list(t.shape)}")
        self.table = t
        self.passes = int(passes)
        self.device = torch.device(device)
        self._dev_table = None

    @classmethod
    def generate(cls, signature, device="cuda", max_passes=None) -> "Tablebase":
        """`hip.tb_generate` on `device` (it synchronises), the table kept there and copied to the host."""
        table, passes = hip.tb_generate(signature, device, max_passes)
        tb = cls(signature, table.cpu().numpy(), passes, device)
        tb._dev_table = table
        return tb

    def save(self, path) -> None:
        """An .npz holding the signature (its codes), the layout version, the passes and the table."""
        with open(path, "wb") as f:
            np.savez_compressed(f, signature=np.array(self.codes, dtype=np.int8), layout_version=np.int64(LAYOUT_VERSION),
                                passes=np.int64(self.passes), table=self.table)

    @classmethod
    def load(cls, path, device="cuda") -> "Tablebase":
        """The inverse of `save`.  Refused: another layout version, and a table whose length is not the signature's entry count."""
        with np.load(path, allow_pickle=False) as z:
            missing = [k for k in ("signature", "layout_version", "passes", "table") if k not in z.files]
            if missing:
                raise hip.XqError(f"Tablebase.load: {path!r} lacks {missing}")
            version = int(z["layout_version"])
            if version != LAYOUT_VERSION:
                raise hip.XqError(f"Tablebase.load: {path!r} has layout version {version}, this code reads {LAYOUT_VERSION}")
            codes = tuple(int(c) for c in z["signature"])
            table = z["table"]
            want = hip.tb_entries(codes)
            if table.ndim != 1 or len(table) != want:
                raise hip.XqError(f"Tablebase.load: {path!r} holds {table.size} entries, signature "
                                  f"{signature_text(codes)!r} has {want}")
            return cls(codes, table.astype(np.int16, copy=False), int(z["passes"]), device)

    def device_table(self) -> torch.Tensor:
        if self._dev_table is None:
            self._dev_table = torch.from_numpy(self.table).to(self.device)
        return self._dev_table

    def probe(self, boards, sides, move_values: bool = True) -> Dict[str, np.ndarray]:
        """`hip.tb_probe_batch` over host positions -> host arrays: value, moves (uint16), counts, move_value, best_action (uint16)
        and status."""
        b, s = _positions(boards, sides)
        table = self.device_table()
        with torch.cuda.device(table.device):
            r = hip.tb_probe_batch(self.codes, table, torch.from_numpy(b).to(table.device), torch.from_numpy(s).to(table.device),
                                   move_values)
            r = {k: v.cpu().numpy() for k, v in r.items()}
        r["moves"], r["best_action"], r["counts"] = r["moves"].view(np.uint16), r["best_action"].view(np.uint16), r["counts"].view(np.uint16)
        return r

    def _by_side(self):
        half = len(self.table) // 2
        return {"red": self.table[:half], "black": self.table[half:]}

    def stats(self) -> dict:
        """Invalid / win / loss / draw entries per side to move, the longest win in plies, the entry count and the passes."""
        out = {"signature": self.signature, "entries": int(len(self.table)), "passes": self.passes}
        for name, t in self._by_side().items():
            valid = t != INVALID
            out[name] = {"invalid": int((~valid).sum()), "win": int((t > 0).sum()), "loss": int((valid & (t < 0)).sum()),
                         "draw": int((t == 0).sum())}
        out["longest_win"] = int(max(int(self.table.max()), 0)) if len(self.table) else 0
        return out

    def positions(self, kind: str, n: int, seed: int = 0, side=None, min_plies: int = 1):
        """A seeded draw without replacement of `n` valid entries of one kind ("win", "draw" or "loss" for the side to move),
        decoded -> (boards int8[n, 90], sides int8[n], index int64[n]), in ascending index order.  `side` (1 red, -1 black)
        keeps one side to move; `min_plies` keeps wins and losses of at least that many plies.  Fewer than n such entries:
        XqError."""
        if kind not in KINDS:
            raise hip.XqError(f"positions: kind must be one of {KINDS}, got {kind!r}")
        if side not in (None, 1, -1):
            raise hip.XqError(f"positions: side must be None, 1 or -1, got {side!r}")
        if isinstance(n, bool) or int(n) != n or int(n) < 0:
            raise hip.XqError(f"positions: n must be an integer >= 0, got {n!r}")
        t = self.table.astype(np.int64)
        if kind == "win":
            keep = t >= max(int(min_plies), 1)
        elif kind == "loss":
            keep = (t != INVALID) & (t < 0) & (-t - 1 >= int(min_plies))
        else:
            keep = t == 0
        half = len(t) // 2
        if side == 1:
            keep[half:] = False
        elif side == -1:
            keep[:half] = False
        pool = np.nonzero(keep)[0]
        if len(pool) < int(n):
            raise hip.XqError(f"positions: {self.signature!r} holds {len(pool)} such {kind} entries, {n} were asked for")
        pick = np.sort(np.random.default_rng(int(seed)).choice(pool, size=int(n), replace=False))
        boards, sides = index_to_board(self.codes, pick)
        return boards, sides, pick


    def play(self, boards, sides, actions=None) -> Dict[str, np.ndarray]:
        """`hip.tb_play_batch` over host positions -> host arrays: boards and side after the move, played (uint16), value,
        move_value, value_out and status.  `actions` None: the table plays its best move everywhere; else one action per position,
        NO_MOVE (or -1) where the table chooses."""
        b, s = _positions(boards, sides)
        table = self.device_table()
        act = None
        if actions is not None:
            a = np.asarray(actions, dtype=np.int64).reshape(-1)
            if len(a) != len(b) or bool(((a < -1) | (a > NO_MOVE)).any()):
                raise hip.XqError(f"play: actions must hold one action in [0, {NO_MOVE}] (or -1) per position ({len(b)}), got "
                                  f"{len(a)} values in [{a.min() if len(a) else 0}, {a.max() if len(a) else 0}]")
            act = torch.from_numpy((a & 0xFFFF).astype(np.uint16).view(np.int16)).to(table.device)
        with torch.cuda.device(table.device):
            r = hip.tb_play_batch(self.codes, table, torch.from_numpy(b).to(table.device), torch.from_numpy(s).to(table.device), act)
            r = {k: v.cpu().numpy() for k, v in r.items()}
        r["played"] = r["played"].view(np.uint16)
        return r

    def entries_of(self, kinds=KINDS, n: int = 256, seed: int = 0, side=None, min_plies: int = 0):
        """`positions` over several kinds at once, for entries one can move from: a seeded draw without replacement of `n` valid
        entries that have a legal move and whose kind ("win", "draw" or "loss" for the side to move) is in `kinds`, decoded ->
        (boards int8[n, 90], sides int8[n], index int64[n]), in ascending index order.  `side` (1 red, -1 black) keeps one side to
        move; `min_plies` keeps wins and losses of at least that many plies.  Fewer than n such entries: XqError."""
        kinds = (kinds,) if isinstance(kinds, str) else tuple(kinds)
        if not kinds or any(k not in KINDS for k in kinds):
            raise hip.XqError(f"entries_of: kinds must be taken from {KINDS}, got {kinds!r}")
        if side not in (None, 1, -1):
            raise hip.XqError(f"entries_of: side must be None, 1 or -1, got {side!r}")
        if isinstance(n, bool) or int(n) != n or int(n) < 0:
            raise hip.XqError(f"entries_of: n must be an integer >= 0, got {n!r}")
        if isinstance(min_plies, bool) or int(min_plies) != min_plies or int(min_plies) < 0:
            raise hip.XqError(f"entries_of: min_plies must be an integer >= 0, got {min_plies!r}")
        t = self.table.astype(np.int64)
        keep = np.zeros(len(t), dtype=bool)
        if "win" in kinds:
            keep |= t >= max(int(min_plies), 1)
        if "loss" in kinds:           # -1 is a loss in 0 plies: no legal move
            keep |= (t != INVALID) & (t < -1) & (-t - 1 >= int(min_plies))
        if "draw" in kinds:
            keep |= t == 0
        half = len(t) // 2
        if side == 1:
            keep[half:] = False
        elif side == -1:
            keep[:half] = False
        pool = np.nonzero(keep)[0]
        if len(pool) < int(n):
            raise hip.XqError(f"entries_of: {self.signature!r} holds {len(pool)} such entries of {kinds}, {n} were asked for")
        pick = np.sort(np.random.default_rng(int(seed)).choice(pool, size=int(n), replace=False))
        boards, sides = index_to_board(self.codes, pick)
        return boards, sides, pick

    def samples(self, index, policy: int = 0, invalid: str = "raise", as_tensor: bool = False):
        """`hip.tb_samples` over the entries `index` -> SAMPLE_DTYPE rows on the host, or with as_tensor the uint8[m, 640] device
        tensor that `ReplayBuffer.extend` takes.  An entry that gives no sample (an index outside the table, an invalid entry, one
        without a legal move) is refused by name (invalid="raise") or left out (invalid="drop"), as `rows_from_records` treats a
        record that does not convert."""
        if invalid not in ("raise", "drop"):
            raise hip.XqError(f"samples: invalid must be 'raise' or 'drop', got {invalid!r}")
        idx = np.asarray(index).reshape(-1)
        if idx.dtype.kind not in "iu":
            raise hip.XqError(f"samples: index must hold integers, got {idx.dtype}")
        idx = idx.astype(np.int64)
        inside = (idx >= 0) & (idx < len(self.table))
        table = self.device_table()
        with torch.cuda.device(table.device):
            rows, status = hip.tb_samples(self.codes, table, torch.from_numpy(np.where(inside, idx, -1).astype(np.int32)).to(table.device),
                                          policy)
            bad = torch.nonzero(status != 0).reshape(-1)
            if int(bad.numel()):
                if invalid == "raise":
                    i = int(bad[0].item())
                    why = {1: "is outside the table", 4: "is no position", 8: "has no legal move"}[int(status[i].item())]
                    raise hip.XqError(f"samples: entry {int(idx[i])} of {self.signature!r} {why} ({int(bad.numel())} of {len(idx)} "
                                      "entries give no sample; invalid='drop' leaves them out)")
                rows = rows[status == 0]
            if as_tensor:
                return rows
            return rows.cpu().numpy().reshape(-1).view(SAMPLE_DTYPE)

class _Position:
    """One position as `MCTS.search_many` takes it: the start of a game, nothing behind it, until `push` plays a move."""

    def __init__(self, board, side):
        self.board = board
        self.current_player = int(side)
        self.move_count = 0
        self.no_capture_count = 0
        self.history = []

    def push(self, action: int, board_after) -> None:
        """One ply of a play-out: the board before it joins the history, the counters move on as a game's do."""
        self.history.append(np.ascontiguousarray(self.board, dtype=np.int8).tobytes())
        self.no_capture_count = 0 if self.board[int(action) % 90] != 0 else self.no_capture_count + 1
        self.board = board_after
        self.current_player = -self.current_player
        self.move_count += 1


def _searched_moves(mcts, games, width: int, solver: bool, what: str):
    """The move one search-only `MCTS` gives every game of `games`, `width` at a time (the last chunk padded with its first game):
    the first maximum of the visits in move order, or `solver_choice` under `solver`."""
    from .mcts import solver_choice
    chosen = np.zeros(len(games), dtype=np.int64)
    for base in range(0, len(games), width):
        part = list(games[base:base + width])
        count = len(part)
        eng = mcts.search_decided(part + [part[0]] * (width - count))
        for slot in range(count):
            r = eng.read_root(slot)
            if len(r["actions"]) == 0:
                raise hip.XqError(f"{what}: a position has no legal move")
            if solver:
                chosen[base + slot] = solver_choice(r["actions"], r["visits"], eng.read_root_states(slot)["children"])
            else:
                chosen[base + slot] = int(r["actions"][int(np.argmax(r["visits"]))])
    return chosen


def score(probe: Dict[str, np.ndarray], chosen) -> Dict[str, object]:
    """What a probe says of one chosen action per position: positions, held (a won position stays won, a drawn one is not lost),
    optimal (the move's value equals the position's), hold_rate and by_kind {kind: [count, held]}.  An action that is no root
    move holds nothing."""
    value = probe["value"].astype(np.int64)
    n = len(value)
    chosen = np.asarray(chosen, dtype=np.int64).reshape(-1)
    if len(chosen) != n:
        raise hip.XqError(f"score: {n} positions and {len(chosen)} chosen actions")
    live = np.arange(hip.MAXM)[None, :] < probe["counts"].astype(np.int64)[:, None]
    at = live & (probe["moves"].astype(np.int64) == chosen[:, None])
    found = at.any(axis=1)
    got = probe["move_value"].astype(np.int64)[np.arange(n), at.argmax(axis=1)]
    held = found & np.where(value > 0, got > 0, got >= 0)
    optimal = found & (got == value)
    by = {}
    for name, mask in (("win", value > 0), ("draw", value == 0)):
        if mask.any():
            by[name] = [int(mask.sum()), int((held & mask).sum())]
    return {"positions": n, "held": int(held.sum()), "optimal": int(optimal.sum()), "hold_rate": float(held.sum()) / n if n else 0.0,
            "by_kind": by}


def hold_rate(model_or_evaluator, tb: Tablebase, boards, sides, num_simulations: int, c_puct: float = 1.5, solver: bool = False,
              perpetual_check: bool = False, seed: int = 0, chunk: int = 256, evaluator_kind: str = "hip",
              early_stop: bool = False) -> Dict[str, object]:
    """How many won or drawn positions of a table a search of `num_simulations` simulations holds (module docstring).  The move is
    the first maximum of the visits in move order, or `solver_choice` under `solver`; the probe's move value scores it (`score`).
    Refused: a position the table does not cover, an invalid one, a lost one.  -> positions, held, optimal, hold_rate, by_kind,
    simulations, seconds, chosen (the action per position).  `early_stop` ends a search as soon as its first choice is fixed
    (MCTS): the same moves, sooner."""
    from .mcts import MCTS
    t0 = time.time()
    if not isinstance(tb, Tablebase):
        raise hip.XqError(f"hold_rate: tb must be a Tablebase, got {type(tb).__name__}")
    if int(num_simulations) < 1:
        raise hip.XqError(f"hold_rate: num_simulations must be >= 1, got {num_simulations}")
    if int(chunk) < 1:
        raise hip.XqError(f"hold_rate: chunk must be >= 1, got {chunk}")
    b, s = _positions(boards, sides)
    n = len(b)
    probe = tb.probe(b, s)
    if n and bool((probe["status"] != 0).any()):
        raise hip.XqError(f"hold_rate: {int((probe['status'] != 0).sum())} positions are not valid entries of {tb.signature!r}")
    if n and bool((probe["value"] < 0).any()):
        raise hip.XqError(f"hold_rate: {int((probe['value'] < 0).sum())} positions are lost for the side to move; only won and "
                          "drawn positions can be held")
    chosen = np.zeros(n, dtype=np.int64)
    if n:
        device = tb.device_table().device
        mcts = MCTS(model_or_evaluator, int(num_simulations), c_puct, device, evaluator_kind, seed=int(seed),
                    perpetual_check=perpetual_check, solver=solver, early_stop=early_stop)
        with torch.cuda.device(device):
            chosen = _searched_moves(mcts, [_Position(b[j], s[j]) for j in range(n)], min(int(chunk), n), solver, "hold_rate")
    return {**score(probe, chosen), "simulations": int(num_simulations), "seconds": time.time() - t0, "chosen": chosen}


OUTCOMES = ("converted", "dropped", "repeated", "unfinished")


def play_out_with(choose, tb: Tablebase, boards, sides, max_plies: int) -> Dict[str, object]:
    """Won endings played out against the table's best defence, one game per position.  `choose(games)` returns one action per
    game for the side that is winning (`games` carry board, current_player, move_count, no_capture_count and history as
    `MCTS.search_many` reads them, counted from the start of the play-out); the table answers through `Tablebase.play`.  A game
    ends converted (the defender has no move), dropped (the mover's move has a value <= 0: the table defends perfectly, so the
    win is gone for good), repeated (a mover-to-move position of this game recurs) or unfinished (`max_plies` plies played and
    still won).  Refused: a position that is not a won entry of the table, max_plies < 1, a chosen action that is no legal move.
    -> positions, the four counts, conversion_rate, conversion_se (binomial), mean_plies_ratio (plies used over the table's
    distance, over the converted games; 0.0 without one) and games: per game its outcome, plies, distance (the table's at the
    start) and moves (every ply, both sides')."""
    if not isinstance(tb, Tablebase):
        raise hip.XqError(f"play_out_with: tb must be a Tablebase, got {type(tb).__name__}")
    if isinstance(max_plies, bool) or int(max_plies) != max_plies or int(max_plies) < 1:
        raise hip.XqError(f"play_out_with: max_plies must be an integer >= 1, got {max_plies!r}")
    b, s = _positions(boards, sides)
    n = len(b)
    start = tb.probe(b, s, move_values=False) if n else {"status": np.zeros(0, np.uint8), "value": np.zeros(0, np.int16)}
    if bool((start["status"] != 0).any()):
        raise hip.XqError(f"play_out_with: {int((start['status'] != 0).sum())} positions are not valid entries of {tb.signature!r}")
    if bool((start["value"] <= 0).any()):
        raise hip.XqError(f"play_out_with: {int((start['value'] <= 0).sum())} positions are drawn or lost for the side to move; "
                          "only won positions can be played out")
    games = [_Position(b[j].copy(), s[j]) for j in range(n)]
    seen = [{g.board.tobytes()} for g in games]
    report = [{"outcome": None, "plies": 0, "distance": int(start["value"][j]), "moves": []} for j in range(n)]
    live = list(range(n))

    def end(j, outcome):
        report[j]["outcome"], report[j]["plies"] = outcome, games[j].move_count

    while live:
        acts = np.asarray(choose([games[j] for j in live]), dtype=np.int64).reshape(-1)
        if len(acts) != len(live):
            raise hip.XqError(f"play_out_with: choose returned {len(acts)} actions for {len(live)} games")
        r = tb.play(np.stack([games[j].board for j in live]), [games[j].current_player for j in live], acts)
        if bool((r["status"] != 0).any()):
            k = int(np.nonzero(r["status"] != 0)[0][0])
            raise hip.XqError(f"play_out_with: action {int(acts[k])} is no legal move of game {live[k]} at ply "
                              f"{games[live[k]].move_count} (status {int(r['status'][k])})")
        defend = []
        for k, j in enumerate(live):
            games[j].push(int(acts[k]), r["boards"][k].copy())
            report[j]["moves"].append(int(acts[k]))
            if r["move_value"][k] <= 0:
                end(j, "dropped")
            elif r["value_out"][k] == -1:
                end(j, "converted")
            elif games[j].move_count >= int(max_plies):
                end(j, "unfinished")
            else:
                defend.append(j)
        live = []
        if defend:
            r = tb.play(np.stack([games[j].board for j in defend]), [games[j].current_player for j in defend])
            for k, j in enumerate(defend):
                games[j].push(int(r["played"][k]), r["boards"][k].copy())
                report[j]["moves"].append(int(r["played"][k]))
                key = games[j].board.tobytes()
                if key in seen[j]:
                    end(j, "repeated")
                elif games[j].move_count >= int(max_plies):
                    end(j, "unfinished")
                else:
                    seen[j].add(key)
                    live.append(j)
    counts = {o: sum(1 for g in report if g["outcome"] == o) for o in OUTCOMES}
    rate = counts["converted"] / n if n else 0.0
    ratios = [g["plies"] / g["distance"] for g in report if g["outcome"] == "converted"]
    return {"positions": n, **counts, "conversion_rate": rate, "conversion_se": float(np.sqrt(rate * (1.0 - rate) / n)) if n else 0.0,
            "mean_plies_ratio": float(np.mean(ratios)) if ratios else 0.0, "games": report}


def play_out(model_or_evaluator, tb: Tablebase, boards, sides, num_simulations: int, max_plies: int = 100, c_puct: float = 1.5,
             solver: bool = False, perpetual_check: bool = False, seed: int = 0, chunk: int = 256,
             evaluator_kind: str = "hip", early_stop: bool = False) -> Dict[str, object]:
    """`play_out_with` with one search-only `MCTS` of `num_simulations` simulations choosing the winner's moves as `hold_rate`
    chooses them (the first maximum of the visits in move order, or `solver_choice` under `solver`), except that every search
    sees its game's move count, no-capture count and history.  -> play_out_with's result and simulations, max_plies, seconds.
    `early_stop` as in `hold_rate`."""
    from .mcts import MCTS
    t0 = time.time()
    if not isinstance(tb, Tablebase):
        raise hip.XqError(f"play_out: tb must be a Tablebase, got {type(tb).__name__}")
    if int(num_simulations) < 1:
        raise hip.XqError(f"play_out: num_simulations must be >= 1, got {num_simulations}")
    if int(chunk) < 1:
        raise hip.XqError(f"play_out: chunk must be >= 1, got {chunk}")
    if isinstance(max_plies, bool) or int(max_plies) != max_plies or int(max_plies) < 1:
        raise hip.XqError(f"play_out: max_plies must be an integer >= 1, got {max_plies!r}")
    b, s = _positions(boards, sides)
    device = tb.device_table().device
    width = max(1, min(int(chunk), len(b)))
    mcts = []

    def choose(games):
        if not mcts:            # built at the first move: a refused set of positions builds no engine
            mcts.append(MCTS(model_or_evaluator, int(num_simulations), c_puct, device, evaluator_kind, seed=int(seed),
                             perpetual_check=perpetual_check, solver=solver, early_stop=early_stop))
        with torch.cuda.device(device):
            return _searched_moves(mcts[0], games, width, solver, "play_out")

    out = play_out_with(choose, tb, b, s, int(max_plies))
    return {**out, "simulations": int(num_simulations), "max_plies": int(max_plies), "seconds": time.time() - t0}

def rescore_samples(samples, tb: Tablebase):
    """-> (new array, covered, changed): a copy of `samples` (SAMPLE_DTYPE) in which every record whose position the table covers
    (probe status 0) has z = the sign of the exact value.  A record's z is the game's outcome from the view of the side to move in
    the record's position (+1 that side won, -1 it lost, 0 a draw: xq_records_to_samples and the engine's drain write it so), which
    is the view the table's value takes.  No other byte of any record changes and the input is not modified."""
    if not isinstance(tb, Tablebase):
        raise hip.XqError(f"rescore_samples: tb must be a Tablebase, got {type(tb).__name__}")
    if not isinstance(samples, np.ndarray) or samples.dtype != SAMPLE_DTYPE:
        raise hip.XqError(f"rescore_samples: samples must be a numpy array of SAMPLE_DTYPE, got "
                          f"{samples.dtype if isinstance(samples, np.ndarray) else type(samples).__name__}")
    out = samples.copy()
    flat = out.reshape(-1)
    if len(flat) == 0:
        return out, 0, 0
    # the host's index first: only the records the layout covers go to the device
    cand = np.nonzero(board_to_index(tb.codes, flat["board"], flat["side"]) >= 0)[0]
    if len(cand) == 0:
        return out, 0, 0
    probe = tb.probe(flat["board"][cand], flat["side"][cand], move_values=False)
    hit = probe["status"] == 0
    rows = cand[hit]
    z = np.sign(probe["value"][hit].astype(np.int64)).astype(np.int8)
    changed = int((flat["z"][rows] != z).sum())
    flat["z"][rows] = z
    return out, int(len(rows)), changed
