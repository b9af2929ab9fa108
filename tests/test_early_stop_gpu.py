"""The settled-move cutoff on the GPU (k_settle, xq_engine_settle) against tests/settle_model.py.

1. the kernel against the model: a search-only and an arena engine, 16 slots, S = 32, the peaked stub, corpus positions and three
   crafted ones (121 and 128 legal moves: the second load and the XQ_MAXM edge; one legal move: settled at once).  After 1, 5, 17
   and 30 eager steps one xq_engine_settle call changes exactly the words the model names, on exactly the slots it names, and the
   counters are the model's sums; a call between select and expand, when every slot waits, changes nothing;
2. the kernel on crafted counts written into the tree: leaders and ties in either half of 128 children, lead == remaining;
3. arena games are byte-identical with and without the option -- packed and masked, recorded and eager, under the perpetual-check
   rule -- searches do settle, and the simulations run plus the simulations saved are the simulations of the full searches;
4. serving: get_action(temperature=0) returns the full search's action from fewer simulations; search() keeps the full search.
"""
import ctypes as C
import types

import numpy as np
import pytest

import capacity_boards as CB
import golden_io as G
import settle_model as SM
from oracle import xq_oracle as O
from test_hip_engine import _run_steps, _stub_batch

pytestmark = pytest.mark.gpu

SLOTS, S = 16, 32
CHECKPOINTS = (1, 5, 17, 30)


def _positions():
    """[(board int8[90], side)]: 13 corpus positions that are not over, then the three crafted ones."""
    d = G.corpus()
    picks = [i for i in range(7, len(d["board"]), 61) if not d["done"][i]][:SLOTS - 3]
    out = [(d["board"][i].reshape(90).copy(), int(d["side"][i])) for i in picks]
    out += [(CB.edge_board(121).reshape(90), 1), (CB.edge_board(128).reshape(90), 1), (CB.rook_board(8).reshape(90), -1)]
    assert len(out) == SLOTS
    assert [len(O.legal_actions(b, s)) for b, s in out[-3:]] == [121, 128, 1]
    return out


def _engine(manual_moves):
    from xiangqi_alphazero_amd import engine
    cfg = engine.make_config(SLOTS, S, add_noise=False, manual_moves=manual_moves, random_opening_moves=0, enable_resign=False,
                             games_target=SLOTS if manual_moves == 2 else 0)
    eng = engine.SelfPlayEngine(cfg)
    assert not eng.early_stop
    for slot, (b, s) in enumerate(_positions()):
        eng.set_position(slot, b, s)
    return eng


def _settle(eng, counters):
    import torch
    from xiangqi_alphazero_amd import hip
    rc = eng.lib.xq_engine_settle(C.byref(eng.h), counters.data_ptr(), hip.stream_ptr(eng.device))
    assert rc == 0
    torch.cuda.synchronize()


def _check_one_call(eng, arena):
    """One xq_engine_settle call on the engine as it stands, against the model; the state words are put back afterwards, so the
    searches go on as if the call had not been made.  -> (searching slots, settled slots)."""
    import torch
    from xiangqi_alphazero_amd import hip
    torch.cuda.synchronize()
    before = eng.slot_ints.clone()
    host = before.cpu().numpy()
    searching = [s for s in range(SLOTS) if host[s, hip.GI_PHASE] == 3]
    roots = []
    for s in searching:
        r = eng.read_root(s)
        assert r["sims_done"] == host[s, hip.GI_SIMS]
        roots.append((s, r["visits"].copy(), r["sims_done"]))
    named, moves, saved = SM.totals(roots, S)
    counters = torch.zeros((SLOTS, 2), dtype=torch.int64, device="cuda")
    _settle(eng, counters)
    want = host.copy()
    for s in named:
        if arena:
            want[s, hip.GI_SIMS] = S
        else:
            want[s, hip.GI_PHASE] = hip.PH_HOLD
    got = eng.slot_ints.cpu().numpy()
    assert got.tobytes() == want.tobytes(), (named, np.argwhere(got != want).tolist())
    c = counters.cpu().numpy()
    assert int(c[:, 0].sum()) == moves and int(c[:, 1].sum()) == saved
    for s, v, done in roots:
        assert (int(c[s, 0]), int(c[s, 1])) == ((1, S - done) if s in named else (0, 0)), s
    assert not c[[s for s in range(SLOTS) if s not in searching]].any()
    eng.slot_ints.copy_(before)
    torch.cuda.synchronize()
    return searching, named


@pytest.mark.parametrize("manual_moves", [1, 2], ids=["search_only", "arena"])
def test_kernel_equals_model_along_a_search(manual_moves):
    import torch
    from xiangqi_alphazero_amd import hip
    eng = _engine(manual_moves)
    arena = manual_moves == 2
    done, settled_at = 0, {}
    for steps in CHECKPOINTS:
        _run_steps(eng, steps - done, [True] * SLOTS)
        done = steps
        searching, named = _check_one_call(eng, arena)
        print(f"manual_moves={manual_moves} after {steps} steps: {len(searching)} searching, settled {named}")
        # after a whole step a slot searches, unless runs of terminal leaves (simulations that need no evaluation) have already
        # brought it to its budget
        assert len(searching) >= SLOTS // 2
        settled_at[steps] = named
        # between select and expand every slot that asked waits for its evaluation: the call touches none of them
        x = eng.select().cpu().numpy()
        torch.cuda.synchronize()
        waiting = int(((eng.slot_ints[:, hip.GI_PHASE] == 2) | (eng.slot_ints[:, hip.GI_PHASE] == 4)).sum())
        assert waiting >= SLOTS // 2
        _check_one_call(eng, arena)
        p, v = _stub_batch(x, [True] * SLOTS)
        eng.expand(torch.from_numpy(p).cuda(), torch.from_numpy(v).cuda(), is_probs=True)
        done += 1
    assert eng.stats()["overflow"] == 0
    assert settled_at[1] == [SLOTS - 1]                          # the forced move, before its first simulation
    assert len(set().union(*settled_at.values())) >= 3           # and leads the remaining simulations cannot catch


def _craft(nch, kind, rng, remaining):
    """Child counts for a root of `nch` children with `remaining` simulations to go."""
    v = rng.integers(0, 4, size=nch).astype(np.int64)
    if nch == 1:
        return v
    a, b = (int(x) for x in rng.choice(nch, size=2, replace=False))
    if kind == "high_half" and nch > 64:
        a, b = nch - 1, 3                                        # the leader in the second load, the runner-up in the first
    if kind == "low_half" and nch > 64:
        a, b = 2, nch - 2
    top = 3 + remaining
    if kind == "tie":
        v[a] = v[b] = top + 5
    elif kind == "equal":                                        # lead == remaining: not settled
        v[b], v[a] = 3, top
    elif kind == "behind":
        v[b], v[a] = 3, top - 1
    else:                                                        # "ahead", "high_half", "low_half": lead == remaining + 1
        v[b], v[a] = 3, top + 1
    return v


@pytest.mark.parametrize("manual_moves", [1, 2], ids=["search_only", "arena"])
def test_kernel_equals_model_on_crafted_counts(manual_moves):
    """Counts written over the root's children of searching slots, sims_done over GI_SIMS: every lead around the threshold, for
    40-odd, 121, 128 children and one."""
    import torch
    from xiangqi_alphazero_amd import hip
    eng = _engine(manual_moves)
    _run_steps(eng, 3, [True] * SLOTS)
    torch.cuda.synchronize()
    views = eng.arena_views()
    phase = eng.slot_ints[:, hip.GI_PHASE].cpu().numpy()
    assert (phase == 3).all()
    rng = np.random.default_rng(29)
    kinds = ("ahead", "equal", "behind", "tie", "high_half", "low_half")
    verdicts = set()
    for round_ in range(len(kinds)):
        for s in range(SLOTS):
            kind = kinds[(s + round_) % len(kinds)]
            remaining = int(rng.integers(1, S + 1))
            first = int(views["first"][s, 0])
            nch = int(views["meta"][s, 0]) & hip.META_COUNT_MASK
            v = _craft(nch, kind, rng, remaining)
            views["N"][s, first:first + nch] = torch.from_numpy(v.astype(np.int32)).cuda()
            eng.slot_ints[s, hip.GI_SIMS] = S - remaining
            verdicts.add((nch > 64, kind, SM.settled(v, S - remaining, S)))
        _check_one_call(eng, manual_moves == 2)
    for wide in (False, True):
        assert (wide, "ahead", True) in verdicts and (wide, "equal", False) in verdicts and (wide, "tie", False) in verdicts
    assert (True, "high_half", True) in verdicts and (True, "low_half", True) in verdicts


# ---- 3. arena games ------------------------------------------------------------------------------------------------------------
GAMES, PLIES, OPENING = 8, 40, 2


def _evaluators():
    from xiangqi_alphazero_amd import evaluator, model, weights
    out = []
    for seed in (1, 2):
        n = model.XiangqiNet(64, 2)
        n.load_state_dict(weights.make_state_dict(64, 2, seed=seed, policy_gain=8.0))
        out.append(evaluator.make_evaluator(n, "cuda", "hip")[0])
    return out


def _arena(early_stop, **kw):
    from xiangqi_alphazero_amd import arena
    en, eo = _evaluators()
    info = {}
    res, rec = arena.play_arena(en, eo, GAMES, S, PLIES, opening_plies=OPENING, seed=3, record_games=True, info=info,
                                early_stop=early_stop, **kw)
    assert info["stats"]["overflow"] == 0 and len(res) == len(rec) == GAMES
    return res.tobytes(), rec.tobytes(), info


@pytest.fixture(scope="module")
def full_arena():
    """The games of the full searches: the shipped path (packed, recorded).  Computed once, read-only."""
    res, rec, info = _arena(False)
    assert "settled_moves" not in info["stats"] and info["packed"]
    assert info["stats"]["sims"] == S * info["stats"]["moves_played"]           # every arena move costs exactly S
    return res, rec, info["stats"]


@pytest.mark.parametrize("packed", [True, False], ids=["packed", "masked"])
@pytest.mark.parametrize("graph", [True, False], ids=["recorded", "eager"])
def test_arena_games_are_byte_identical(full_arena, monkeypatch, packed, graph):
    if not graph:
        monkeypatch.setenv("XQ_ARENA_GRAPH", "0")
    res, rec, info = _arena(True, packed=packed)
    st = info["stats"]
    print(f"packed={packed} graph={graph}: settled {st['settled_moves']} of {st['moves_played']} moves, saved "
          f"{st['simulations_saved']} of {full_arena[2]['sims']} simulations, {info['steps']} steps")
    assert info["packed"] is packed
    assert res == full_arena[0] and rec == full_arena[1]
    assert st["settled_moves"] > 0
    assert st["moves_played"] == full_arena[2]["moves_played"]
    assert st["sims"] + st["simulations_saved"] == full_arena[2]["sims"]
    assert 0 < st["simulations_saved"] <= S * st["settled_moves"]


def test_arena_games_are_byte_identical_under_the_perpetual_check_rule():
    res0, rec0, info0 = _arena(False, perpetual_check=True)
    res1, rec1, info1 = _arena(True, perpetual_check=True)
    assert res1 == res0 and rec1 == rec0 and info1["stats"]["settled_moves"] > 0
    assert info1["stats"]["sims"] + info1["stats"]["simulations_saved"] == info0["stats"]["sims"]


def test_plain_arena_engine_without_arena_options():
    """play_arena's other engine (no openings, no info): the same results with and without the option."""
    from xiangqi_alphazero_amd import arena
    en, eo = _evaluators()
    a = arena.play_arena(en, eo, 2, S, 24)
    b = arena.play_arena(en, eo, 2, S, 24, early_stop=True)
    assert a.tobytes() == b.tobytes()


# ---- 4. serving ----------------------------------------------------------------------------------------------------------------
class _PeakedStub:
    """Deterministic dense-protocol evaluator on the device: logits and value are elementwise functions of an exact integer key
    of the planes (0/1 planes times small integer weights: the float32 sums are exact in any order).  Logits span 0 .. 15."""

    def __init__(self):
        import torch
        g = torch.Generator().manual_seed(9)
        self.w = torch.randint(1, 512, (1350,), generator=g).float().cuda()
        self.a = torch.randint(1, 1 << 12, (8100,), generator=g).float().cuda()

    def __call__(self, x):
        import torch
        key = (x.reshape(x.shape[0], -1) * self.w).sum(1)
        logits = torch.remainder(key[:, None] + self.a[None, :], 61.0) / 4.0
        value = (torch.remainder(key * 3.0, 201.0) - 100.0) / 128.0
        return logits, value


def test_get_action_is_the_full_searchs_from_fewer_simulations():
    from xiangqi_alphazero_amd import mcts as M
    sims = 64
    d = G.corpus()
    picks = [i for i in range(11, len(d["board"]), 37) if not d["done"][i]][:32]
    assert len(picks) == 32
    games = []
    for i in picks:
        hist = G.history_tail(d, i)
        games.append(types.SimpleNamespace(board=d["board"][i].reshape(10, 9).copy(), current_player=int(d["side"][i]),
                                           move_count=int(d["ply"][i]), no_capture_count=0, history=[bytes(h) for h in hist]))
    ev = _PeakedStub()
    on, off = M.MCTS(ev, sims, seed=3, early_stop=True), M.MCTS(ev, sims, seed=3)
    ran = []
    for g in games:
        a = on.get_action(g, temperature=0)
        r = on._engine(1, False, True).read_root(0)
        assert 0 <= r["sims_done"] <= sims and r["sims_done"] == int(r["visits"].sum())
        ran.append(r["sims_done"])
        assert a == off.get_action(g, temperature=0)
        assert off._engine(1, False).read_root(0)["sims_done"] == sims
    print("simulations run per position:", ran)
    assert min(ran) < sims
    st = on._engine(1, False, True).early_stop_stats()
    assert st["settled_moves"] == sum(n < sims for n in ran) and st["simulations_saved"] == sum(sims - n for n in ran)
    # search() on the same object keeps the full search: its pi is a function of all S simulations
    pi = on.search(games[0], temperature=1.0, add_noise=False)
    assert on._engine(1, False).read_root(0)["sims_done"] == sims
    assert pi.tobytes() == off.search(games[0], temperature=1.0, add_noise=False).tobytes()
    assert set(on._engines) == {(1, False, True), (1, False)}
