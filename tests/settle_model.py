"""Host model of the settled-move cutoff (xq_engine_settle, csrc/xq_settle.hip).

A move played at temperature 0 is the FIRST MAXIMUM of the root's visit counts in move order.  A search with `sims_done` of its
`budget` simulations run is settled when the simulations that are left cannot move that maximum:

    nch == 1                          the move is forced, or
    n1 - n2 > budget - sims_done      n1 the largest count, n2 the second largest counted with multiplicity

`settled` is the rule; `first_max` and `after` are what the tests need to show that it is exact and strict.
"""
from __future__ import annotations

import numpy as np


def first_max(visits) -> int:
    """The index a temperature-0 move takes: the lowest index of the largest count (np.argmax; slot_arena_move)."""
    return int(np.argmax(np.asarray(visits, dtype=np.int64)))


def lead(visits) -> int:
    """n1 - n2 with multiplicity: 0 for a tie for first.  One child has no runner-up: its lead is its own count."""
    v = np.sort(np.asarray(visits, dtype=np.int64))
    return int(v[-1] - v[-2]) if len(v) > 1 else int(v[-1])


def settled(visits, sims_done: int, budget: int) -> bool:
    """The kernel's verdict on a slot in PH_SEARCH.  A search that has run its budget is not settled: it is over, and the select
    kernel ends it as it always did."""
    v = np.asarray(visits, dtype=np.int64)
    remaining = int(budget) - int(sims_done)
    if len(v) < 1 or remaining <= 0:
        return False
    if len(v) == 1:
        return True
    return lead(v) > remaining


def after(visits, child: int, n: int) -> np.ndarray:
    """The counts after `n` more simulations that all go through root child `child`."""
    v = np.asarray(visits, dtype=np.int64).copy()
    v[child] += int(n)
    return v


def totals(roots, budget: int):
    """(settled slots, settled_moves, simulations_saved) over `roots` = [(slot, visits, sims_done)] of the searching slots."""
    named = [(slot, int(budget) - int(done)) for slot, v, done in roots if settled(v, done, budget)]
    return [s for s, _ in named], len(named), sum(r for _, r in named)
