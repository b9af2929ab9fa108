"""Hand-made boards, records and groups for the merge-duplicates tests (CPU model, ABI and GPU files share them)."""
from functools import lru_cache

import numpy as np

from golden_io import corpus
from xiangqi_alphazero_amd import sample_format as F

BOUNDARY_SQUARES = (0, 63, 64, 89)          # the ballot's lane and word boundaries
GROUP_SIZES = (2, 3, 64, 65, 200)


def mirror_board(board: np.ndarray) -> np.ndarray:
    return np.asarray(board, dtype=np.int8).reshape(-1, 90)[:, F.MIR_SQ].reshape(np.shape(board))


def initial_board() -> np.ndarray:
    d = corpus()
    return d["board"][int(np.nonzero(d["ply"] == 0)[0][0])].astype(np.int8)


@lru_cache(maxsize=None)
def boundary_pairs():
    """-> list of (board_a, side_a, board_b, side_b, what): pairs that must get different keys.  The base board is asymmetric at
    row 5 so that a change at one square never makes the two boards mirror images of each other."""
    base = np.zeros(90, dtype=np.int8)
    base[4], base[85], base[45], base[47] = 1, -1, 3, -4
    out = []
    for sq in BOUNDARY_SQUARES:
        other = base.copy()
        other[sq] = 6
        out.append((base.copy(), 1, other, 1, "square %d" % sq))
    out.append((base.copy(), 1, base.copy(), -1, "side"))
    return out


def records_of(boards: np.ndarray, sides: np.ndarray) -> np.ndarray:
    smp = np.zeros(len(boards), dtype=F.SAMPLE_DTYPE)
    smp["board"], smp["side"] = boards, sides
    return smp


@lru_cache(maxsize=None)
def key_records() -> np.ndarray:
    """257 records for the key kernel: the boundary boards, the initial position, then corpus boards and mirror images of some."""
    d = corpus()
    boards, sides = [], []
    for a, sa, b, sb, _ in boundary_pairs():
        boards += [a, b]
        sides += [sa, sb]
    boards.append(initial_board())
    sides.append(1)
    pick = np.linspace(0, len(d["board"]) - 1, 257 - len(boards)).astype(np.int64)
    for j, i in enumerate(pick):
        b = d["board"][i].astype(np.int8)
        boards.append(mirror_board(b) if j % 3 == 1 else b)
        sides.append(int(d["side"][i]))
    smp = records_of(np.array(boards, dtype=np.int8), np.array(sides, dtype=np.int8))
    smp.setflags(write=False)
    return smp


def fresh_targets(s, rng, kind: str, m: int, actions=None) -> None:
    """Fresh visits, z and root statistics for one record, in place; kind: plain | late_temp | gumbel | no_visits."""
    s["n_moves"], s["z"] = m, rng.integers(-1, 2)
    s["late_temp"], s["reserved0"] = 0, 0
    s["actions"][:] = 0
    s["visits"][:] = 0
    s["actions"][:m] = rng.choice(8100, m, replace=False) if actions is None else actions[:m]
    vis = rng.integers(0, 200, m)
    if kind == "late_temp":
        s["late_temp"] = 1
    elif kind == "gumbel":
        s["reserved0"] = 1
        vis = np.floor(rng.dirichlet(np.full(m, 0.3)) * 65535).astype(np.int64) if m else vis
    elif kind == "no_visits":
        vis[:] = 0
    if kind != "no_visits" and m:
        vis[rng.integers(0, m)] = max(1, int(vis.max()))
    s["visits"][:m] = vis
    rs = np.zeros(1, dtype=F.ROOT_STATS_DTYPE)
    rs["root_q"], rs["root_visits"], rs["has_root_stats"] = rng.uniform(-1, 1), rng.integers(1, 800), rng.integers(0, 2)
    s["pad"] = rs.view(np.uint8).reshape(20)


def make_group(board: np.ndarray, side: int, size: int, rng, kinds=("plain", "gumbel"), shared_actions: bool = True,
               m: int = 40) -> np.ndarray:
    """`size` records of one position: the board (or, at random, its mirror image) and side copied under fresh visits, z and root
    statistics.  shared_actions: every member names the same action list (in its own orientation), as engine records of one
    position do; otherwise each draws its own (disjoint lists with near certainty are the caller's to build)."""
    smp = np.zeros(size, dtype=F.SAMPLE_DTYPE)
    base_actions = rng.choice(8100, 128, replace=False)
    for k in range(size):
        s = smp[k]
        flipped = bool(rng.integers(0, 2))
        s["board"] = mirror_board(board) if flipped else board
        s["side"] = side
        acts = None
        if shared_actions:
            acts = F.FLIP_PERM[base_actions] if flipped else base_actions
        fresh_targets(s, rng, kinds[k % len(kinds)], m if shared_actions else int(rng.integers(1, 129)), acts)
        s["slot"], s["game_seq"], s["ply"] = rng.integers(0, 8192), rng.integers(0, 2 ** 31), rng.integers(0, 400)
    return smp


@lru_cache(maxsize=None)
def group_buffer(late: bool):
    """-> (records, groups (offsets, members, member_mirrored), notes): one buffer holding, interleaved in age, groups of the
    sizes GROUP_SIZES over distinct corpus positions, a group with disjoint action lists, a group with some invalid members, a
    group whose members are all invalid, and a few singletons.  late: every third member is a late-temperature record."""
    rng = np.random.default_rng(20 + int(late))
    d = corpus()
    kinds = ("plain", "gumbel", "late_temp") if late else ("plain", "gumbel")
    parts, notes = [], []
    pos = np.linspace(100, len(d["board"]) - 100, len(GROUP_SIZES) + 6).astype(np.int64)
    for size, i in zip(GROUP_SIZES, pos):
        parts.append(make_group(d["board"][i].astype(np.int8), int(d["side"][i]), size, rng, kinds))
        notes.append("size %d" % size)
    i = pos[len(GROUP_SIZES)]
    disjoint = make_group(d["board"][i].astype(np.int8), int(d["side"][i]), 3, rng, kinds, shared_actions=False)
    ids = rng.permutation(8100)
    for k in range(3):                                   # three disjoint action lists, in the record's stored frame
        m = (20, 128, 1)[k]
        disjoint[k]["n_moves"] = m
        disjoint[k]["actions"][:m] = ids[200 * k:200 * k + m]
        disjoint[k]["visits"][:m] = rng.integers(1, 100, m)
    parts.append(disjoint)
    notes.append("disjoint")
    i = pos[len(GROUP_SIZES) + 1]
    parts.append(make_group(d["board"][i].astype(np.int8), int(d["side"][i]), 5, rng, ("plain", "no_visits", "gumbel", "no_visits", "plain")))
    notes.append("some invalid")
    i = pos[len(GROUP_SIZES) + 2]
    parts.append(make_group(d["board"][i].astype(np.int8), int(d["side"][i]), 3, rng, ("no_visits",)))
    notes.append("all invalid")
    for j in range(3):
        i = pos[len(GROUP_SIZES) + 3 + j]
        parts.append(make_group(d["board"][i].astype(np.int8), int(d["side"][i]), 1, rng, (kinds[j % len(kinds)],)))
        notes.append("single")
    smp = np.concatenate(parts)
    smp = smp[rng.permutation(len(smp))]                 # interleave the groups in age
    groups = F.position_groups(smp, True)
    smp.setflags(write=False)
    return smp, groups, notes
