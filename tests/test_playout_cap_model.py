"""The playout-cap host model (tests/playout_cap_model.py) on the CPU, before tests/test_playout_cap_gpu.py uses it to judge the
engine: with the cap off it is tree_reuse_model.play_game on every recorded game; with p = 1 and a dummy draw spliced in before
every move-choice draw it replays the cap-off game (this pins the draw order); with the cap on every sample holds S visits, only
full moves are sampled and the simulations add up."""
import numpy as np
import pytest

import golden_io as G
import playout_cap_model as PC
import tree_reuse_model as M


def cap_of(cfg, p):
    """The cap the tests use on a recorded configuration: S_fast = S / 4 (4 of 16, 25 of 100)."""
    return (p, max(1, int(cfg["num_simulations"]) // 4))


def _same_samples(got, want):
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert list(a["actions"]) == list(b["actions"]) and list(a["visits"]) == list(b["visits"])
        assert a["z"] == b["z"] and a["player"] == b["player"] and a["late"] == b["late"]
        assert bytes(a["board"]) == bytes(b["board"])


@pytest.mark.parametrize("reuse", [False, True])
@pytest.mark.parametrize("idx", range(4))
def test_cap_off_is_the_tree_reuse_model(idx, reuse):
    t = G.game_traces()[idx]
    peaked = t["stub"] == "peaked"
    want, w_winner, w_plies, w_stats = M.play_game(t["cfg"], peaked, t["seed"], tree_reuse=reuse)
    got, winner, plies, stats = PC.play_game(t["cfg"], peaked, t["seed"], tree_reuse=reuse, cap=None)
    assert (winner, plies) == (w_winner, w_plies)
    _same_samples(got, want)
    assert all(stats[k] == w_stats[k] for k in ("sims", "reused_visits", "reroots"))
    assert stats["fast_moves"] == stats["fast_sims"] == 0 and stats["full_moves"] == len(got)


@pytest.mark.parametrize("reuse", [False, True])
@pytest.mark.parametrize("idx", range(4))
def test_p_one_on_the_spliced_stream_is_the_cap_off_game(idx, reuse):
    t = G.game_traces()[idx]
    peaked = t["stub"] == "peaked"
    want, w_winner, w_plies, w_stats = M.play_game(t["cfg"], peaked, t["seed"], tree_reuse=reuse)
    got, winner, plies, stats = PC.play_game(t["cfg"], peaked, PC.SplicedDraws(t["seed"]), tree_reuse=reuse,
                                             cap=(1.0, 1))
    assert (winner, plies) == (w_winner, w_plies)
    _same_samples(got, want)
    assert all(stats[k] == w_stats[k] for k in ("sims", "reused_visits", "reroots")) and stats["fast_moves"] == 0


@pytest.mark.parametrize("p", [0.25, 0.5])
@pytest.mark.parametrize("reuse", [False, True])
@pytest.mark.parametrize("idx", range(4))
def test_cap_on_invariants(idx, reuse, p):
    t = G.game_traces()[idx]
    S = int(t["cfg"]["num_simulations"])
    cap = cap_of(t["cfg"], p)
    got, winner, plies, st = PC.play_game(t["cfg"], t["stub"] == "peaked", t["seed"], tree_reuse=reuse, cap=cap)
    assert all(int(s["visits"].sum()) == S for s in got)
    assert len(got) == st["full_moves"] and st["fast_moves"] + st["full_moves"] == len(st["moves"])
    assert st["fast_moves"] > 0
    if not reuse:
        assert st["sims"] == S * st["full_moves"] + cap[1] * st["fast_moves"] and st["fast_sims"] == cap[1] * st["fast_moves"]
        assert st["reused_visits"] == 0
    for m in st["moves"]:
        assert m["visits"] == (S if m["full"] else max(cap[1], m["reused"])) and m["reused"] < S
        assert m["new"] == m["visits"] - m["reused"]
    assert st["sims"] == sum(m["new"] for m in st["moves"])
