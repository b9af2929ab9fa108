"""The per-side resign rule on the GPU (k_resign_scan, k_resign; xq_resign_scan_batch, xq_engine_resign)
against tests/resign_model.py.

1. the rule alone: hip.resign_scan over 512 random sequences (lengths 0..40, with NaNs and values equal to the threshold) for every
   K, under two value distributions, one with about half the values below the threshold;
2. the engine against the model: whole games with a scripted evaluator whose value is a fixed function of the planes.  Every game
   record is replayed on the device, every position whose value the engine recorded is encoded and evaluated again, and the model
   must reproduce reason, winner and plies of every game, the statistics' resigns, the exempt set and every holdout row;
3. identity: with holdout_prob = 1, and with threshold = -inf, samples, results and records are the bytes of an engine with
   enable_resign=False;
4. "red despairs": an evaluator that says -0.95 with red to move and +0.95 with black to move.  The engine's own rule at the
   shipped -0.9 and K = 5 resigns no game; the option resigns every game that is not exempt, red the resigner;
5. the packed step with the hand-written 64-channel evaluator, eager and replayed from a HIP graph with equal bytes; tree reuse and
   the playout cap;
6. a row array of one row: one row kept, the others counted, nothing else changed.
"""
import bisect
import math

import numpy as np
import pytest

import resign_model as RM

pytestmark = pytest.mark.gpu

SLOTS, SIMS, LENGTH, GAMES, SEED = 16, 8, 60, 32, 21
# a value is below -0.7 with probability 0.15, a window of two with 0.02, and a game has some 45 windows: about half the games
# that may resign do
THRESHOLD, STEPS, HOLDOUT = -0.7, 2, 0.25


# ---- 1. the rule alone --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dist", ["half_below", "mostly_above"])
def test_resign_scan_equals_the_model(dist):
    import torch
    from xiangqi_alphazero_amd import hip
    rng = np.random.default_rng(3 if dist == "half_below" else 4)
    n, max_len, t = 512, 40, -0.5
    values = (rng.uniform(-1.0, 0.0, (n, max_len)) if dist == "half_below" else rng.uniform(-0.7, 1.0, (n, max_len))).astype(np.float32)
    values[rng.random((n, max_len)) < 0.02] = np.float32(t)                  # equality at the threshold
    values[rng.random((n, max_len)) < 0.01] = np.nan
    values[:8] = np.float32(-0.99)                                            # all low: the earliest index for every K
    lengths = rng.integers(0, max_len + 1, n).astype(np.int32)
    lengths[:8] = [0, 1, 2, 3, 14, 15, 39, 40]
    first = np.where(rng.random(n) < 0.5, 1, -1).astype(np.int8)
    first[8:16] = [0, 2, -2, 3, 127, -128, 5, -5]                             # anything but 1 is black
    dv, dl, df = (torch.from_numpy(a).cuda() for a in (values, lengths, first))
    fired = 0
    for K in range(1, hip.RESIGN_MAX_STEPS + 1):
        index, resigner, level, where = (a.cpu().numpy() for a in hip.resign_scan(dv, dl, df, t, K))
        for i in range(n):
            want = RM.scan(values[i, :lengths[i]], int(first[i]), K, t)
            got = (int(index[i]), int(resigner[i]), level[i].tolist(), where[i].tolist())
            assert got == (want["resign_index"], want["resigner"], [float(x) for x in want["level"]], want["level_index"]), (K, i)
        fired += int((index >= 0).sum())
        assert int(index[0]) == -1 and int(index[7]) == 2 * (K - 1)           # no value at all; forty low values
    print(f"{dist}: {fired} of {n * 8} scans resign")
    assert 0 < fired < n * 8
    empty = hip.resign_scan(dv[:0], dl[:0], df[:0], t, 3)
    assert [tuple(a.shape) for a in empty] == [(0,), (0,), (0, 2), (0, 2)]
    index = hip.resign_scan(dv[:, :0].contiguous(), torch.zeros_like(dl), df, t, 1)[0]      # max_len = 0: no values at all
    assert (index == -1).all().item()


# ---- the scripted evaluators --------------------------------------------------------------------------------------------------------
class _Scripted:
    """Deterministic, capturable dense-protocol evaluator: logits and value are elementwise functions of an exact integer key of
    the planes (0/1 planes times small integer weights: float32 sums are exact in any order, so a row's value does not depend on
    the batch it is in).  The value is a hash of the row mapped into [-1, 1]."""

    def __init__(self):
        import torch
        g = torch.Generator().manual_seed(9)
        self.w = torch.randint(1, 512, (1350,), generator=g).float().cuda()
        self.a = torch.randint(1, 1 << 12, (8100,), generator=g).float().cuda()

    def key(self, x):
        return (x.reshape(x.shape[0], -1) * self.w).sum(1)

    def value(self, x):
        import torch
        return (torch.remainder(self.key(x) * 7.0, 257.0) - 128.0) / 128.0

    def __call__(self, x):
        import torch
        logits = torch.remainder(self.key(x)[:, None] + self.a[None, :], 61.0) / 4.0
        return logits, self.value(x)


class _RedDespairs(_Scripted):
    """-0.95 with red to move (plane 14 is all ones), +0.95 with black to move."""

    def value(self, x):
        import torch
        red = x[:, 14, 0, 0] > 0.5
        return torch.where(red, torch.full_like(x[:, 0, 0, 0], -0.95), torch.full_like(x[:, 0, 0, 0], 0.95))


def _hip_value(ev):
    return lambda x: ev(x.contiguous())[1].clone()


# ---- playing, and the model of what was played ------------------------------------------------------------------------------------------
def _play(ev, resign=None, graph=False, n_games=GAMES, **kw):
    """-> dict of the drained samples, results and records (sorted), the statistics, and with the option its rows and counters."""
    from xiangqi_alphazero_amd import engine
    cfg_kw = dict(add_noise=False, max_game_length=LENGTH, games_target=n_games, seed=SEED)
    cfg_kw.update(kw.pop("cfg", {}))
    eng = engine.SelfPlayEngine(engine.make_config(SLOTS, SIMS, **cfg_kw), evaluator=ev, record_games=True,
                                **({} if resign is None else {"resign": resign}), **kw)
    if graph:
        assert eng.capture_step() and eng.launch_mode == "graph"
    while True:
        eng.step()
        if eng.steps % 16 == 0 and eng.stats()["games_finished"] >= n_games:
            break
        assert eng.steps < 40000, "games did not finish"
    st = eng.stats()
    assert st["overflow"] == 0 and st["games_finished"] == n_games
    samples, results = eng.drain()
    out = dict(samples=np.sort(samples, order=["slot", "game_seq", "ply"]), results=np.sort(results, order=["slot", "game_seq"]),
               records=np.sort(eng.drain_games(), order=["slot", "game_seq"]), stats=st, path=eng.path)
    if resign is not None:
        out["rows"], out["resign_stats"] = eng.drain_resign_rows(), eng.resign_stats()
        assert len(eng.drain_resign_rows()) == 0                             # the drain empties the array
    return out


def _model(run, value_of, K, threshold):
    """Per game (slot, game_seq): the rule over the values the engine recorded -- one per real position from the first with more
    than 10 samples behind it, the last position included -- recomputed from the record's replay."""
    import torch
    from xiangqi_alphazero_amd import engine, hip
    records, samples = run["records"], run["samples"]
    sample_plies = {}
    for s in samples:
        sample_plies.setdefault((int(s["slot"]), int(s["game_seq"])), []).append(int(s["ply"]))
    idx, plies, spans = [], [], []
    for i, r in enumerate(records):
        sp = sorted(sample_plies.get((int(r["slot"]), int(r["game_seq"])), []))
        mine = [p for p in range(int(r["opening_plies"]), int(r["n_moves"]) + 1) if bisect.bisect_left(sp, p) > 10]
        assert mine == list(range(mine[0], int(r["n_moves"]) + 1)) if mine else True
        spans.append((len(idx), len(mine)))
        idx += [i] * len(mine)
        plies += mine
    at = engine.replay_games(records[idx], stop_ply=np.array(plies, dtype=np.int32))
    assert not at["status"].any().item()
    values = value_of(hip.encode(at["board"], at["side"])).cpu().numpy()
    sides = at["side"].cpu().numpy()
    over = engine.replay_games(records)["over_kind"].cpu().numpy()
    torch.cuda.synchronize()
    out = {}
    for i, r in enumerate(records):
        lo, m = spans[i]
        scan = RM.scan(values[lo:lo + m], int(sides[lo]) if m else 1, K, threshold, plies=plies[lo:lo + m])
        out[(int(r["slot"]), int(r["game_seq"]))] = dict(scan=scan, values=m, over=int(over[i]) != 0 or int(r["n_moves"]) >= LENGTH)
    return out


def _check(run, model, threshold_holdout, what):
    """Every game's ending, the counters and the holdout rows against the model.  -> (games resigned, games exempt)."""
    results, rows = run["results"], run["rows"]
    assert [(int(r["slot"]), int(r["game_seq"])) for r in results] == sorted(model)
    resigned, exempt = [], []
    for r in results:
        key = (int(r["slot"]), int(r["game_seq"]))
        m = model[key]
        scan = m["scan"]
        ex = RM.exempt(SEED, 0, key[0], key[1], threshold_holdout)
        at = scan["resign_ply"]
        # a position the rules end stays the rules': it is the game's last, so no earlier index is affected
        fires = not ex and at >= 0 and not (at == int(r["steps"]) and m["over"])
        if fires:
            assert (int(r["reason"]), int(r["winner"]), int(r["steps"])) == (3, -scan["resigner"], at), (what, key)
            resigned.append(key)
        else:
            assert int(r["reason"]) != 3, (what, key)
        if ex:
            exempt.append(key)
    assert run["stats"]["resigns"] == len(resigned) == run["resign_stats"]["resigned"], what
    assert run["resign_stats"]["holdout_games"] == len(exempt) and run["resign_stats"]["rows_dropped"] == 0
    assert run["resign_stats"]["values_seen"] == sum(m["values"] for m in model.values())
    assert [(int(w["slot"]), int(w["game_seq"])) for w in rows] == exempt       # sorted by slot and game_seq, like the results
    for w in rows:
        key = (int(w["slot"]), int(w["game_seq"]))
        scan = model[key]["scan"]
        res = results[(results["slot"] == key[0]) & (results["game_seq"] == key[1])][0]
        assert w["level"].tobytes() == np.array(scan["level"], dtype=np.float32).tobytes(), (what, key, w["level"], scan["level"])
        assert w["level_ply"].tolist() == scan["level_ply"], (what, key)
        assert (int(w["winner"]), int(w["reason"]), int(w["plies"])) == (int(res["winner"]), int(res["reason"]), int(res["steps"]))
        assert not w["zero"].any()
    print(f"{what}: {len(resigned)} resigned, {len(exempt)} exempt, {len(results) - len(resigned)} not resigned, "
          f"{len(run['samples'])} samples, mean plies {results['steps'].mean():.1f}")
    return resigned, exempt


_shared = {}


def _scripted_run():
    """The engine case, played once and shared, never modified."""
    if "run" not in _shared:
        ev = _Scripted()
        run = _play(ev, dict(threshold=THRESHOLD, check_steps=STEPS, holdout_prob=HOLDOUT))
        for a in (run["samples"], run["results"], run["records"], run["rows"]):
            a.setflags(write=False)
        _shared["run"], _shared["ev"] = run, ev
    return _shared["run"], _shared["ev"]


# ---- 2. the engine against the model ---------------------------------------------------------------------------------------------------
def test_engine_equals_the_model():
    run, ev = _scripted_run()
    assert run["path"] == "full"
    resigned, exempt = _check(run, _model(run, ev.value, STEPS, THRESHOLD), HOLDOUT, "scripted")
    n = len(run["results"])
    assert n == GAMES and 4 * len(resigned) >= n and 4 * (n - len(resigned)) >= n
    assert 0 < len(exempt) < n
    # a resigned game's last position has no sample; every resigner really was low
    for r in run["results"][run["results"]["reason"] == 3]:
        s = run["samples"][(run["samples"]["slot"] == r["slot"]) & (run["samples"]["game_seq"] == r["game_seq"])]
        assert len(s) == int(r["n_samples"]) and (s["ply"] < r["steps"]).all()
        assert set(s["z"].tolist()) <= {1, -1}


# ---- 3. identity -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("resign", [dict(threshold=THRESHOLD, check_steps=STEPS, holdout_prob=1.0),
                                    dict(threshold=-math.inf, check_steps=STEPS, holdout_prob=0.0)], ids=["all_exempt", "minus_inf"])
def test_nobody_resigns_is_the_engine_without_resignation(resign):
    ev = _Scripted()
    if "plain" not in _shared:
        _shared["plain"] = _play(ev, None, cfg=dict(enable_resign=False))
    plain, on = _shared["plain"], _play(ev, resign)
    for k in ("samples", "results", "records"):
        assert on[k].tobytes() == plain[k].tobytes(), k
    assert on["stats"] == plain["stats"] and on["stats"]["resigns"] == 0 and len(on["samples"]) > 0
    rs = on["resign_stats"]
    assert rs["resigned"] == 0 and rs["values_seen"] > 0
    if resign["holdout_prob"] == 1.0:
        assert rs["holdout_games"] == GAMES == len(on["rows"]) and np.isfinite(on["rows"]["level"]).any()
    else:
        assert rs["holdout_games"] == 0 == len(on["rows"])
    # the shared engine case, under the same seed, is another run: some game did resign there
    assert _scripted_run()[0]["results"].tobytes() != plain["results"].tobytes()


# ---- 4. red despairs ---------------------------------------------------------------------------------------------------------------------
def test_red_despairs_only_the_per_side_rule_resigns():
    ev = _RedDespairs()
    plain = _play(ev, None, cfg=dict(enable_resign=True, resign_threshold=-0.9, resign_check_steps=5))
    assert plain["stats"]["resigns"] == 0 and not (plain["results"]["reason"] == 3).any()
    run = _play(ev, dict(threshold=-0.9, check_steps=5, holdout_prob=HOLDOUT))
    resigned, exempt = _check(run, _model(run, ev.value, 5, -0.9), HOLDOUT, "red despairs")
    res = run["results"]
    assert 0 < len(exempt) < GAMES
    for r in res:
        key = (int(r["slot"]), int(r["game_seq"]))
        if key in exempt:
            assert int(r["reason"]) != 3
        elif int(r["reason"]) == 3:
            # red's fifth recorded value: index 8 when the first recorded position is red's, else 9
            assert int(r["winner"]) == -1, key
            assert int(r["n_samples"]) in (19, 20) and int(r["steps"]) % 2 == 0      # red is to move at even plies
        else:
            # the rules were faster: the game ended before red had five recorded values, or (19 or 20 samples) at the very
            # position that would have been red's fifth, which stays the rules'
            assert int(r["reason"]) in (1, 4) and int(r["n_samples"]) <= 20, key
    assert len(resigned) > 0
    for w in run["rows"]:                                                    # a holdout game that got that far: red's level is -0.95
        if int(w["plies"]) >= 4 + 11 + 9:
            assert w["level"].tolist() == [float(np.float32(-0.95)), float(np.float32(0.95))]


# ---- 5. the other paths ------------------------------------------------------------------------------------------------------------------
def test_packed_step_eager_and_graph():
    from test_tree_reuse_gpu import _hip_evaluator
    _, ev = _hip_evaluator()
    resign = dict(threshold=0.0, check_steps=STEPS, holdout_prob=HOLDOUT)
    eager = _play(ev, resign)
    assert eager["path"] == "packed"
    _check(eager, _model(eager, _hip_value(ev), STEPS, 0.0), HOLDOUT, "packed")
    graph = _play(ev, resign, graph=True)
    for k in ("samples", "results", "records", "rows"):
        assert graph[k].tobytes() == eager[k].tobytes(), k
    assert graph["resign_stats"] == eager["resign_stats"] and graph["stats"] == eager["stats"]


@pytest.mark.parametrize("kw", [dict(tree_reuse=True), dict(playout_cap=(0.5, 4))], ids=["tree_reuse", "playout_cap"])
def test_with_tree_reuse_and_with_the_playout_cap(kw):
    ev = _Scripted()
    run = _play(ev, dict(threshold=THRESHOLD, check_steps=STEPS, holdout_prob=HOLDOUT), **kw)
    resigned, _ = _check(run, _model(run, ev.value, STEPS, THRESHOLD), HOLDOUT, sorted(kw)[0])
    assert len(resigned) > 0
    if "tree_reuse" in kw:
        assert run["stats"]["reused_visits"] > 0
    else:
        assert run["stats"]["fast_moves"] > 0


# ---- 6. overflow -------------------------------------------------------------------------------------------------------------------------
def test_a_full_row_array_drops_and_counts():
    run, ev = _scripted_run()
    small = _play(ev, dict(threshold=THRESHOLD, check_steps=STEPS, holdout_prob=HOLDOUT, max_rows=1))
    for k in ("samples", "results", "records"):
        assert small[k].tobytes() == run[k].tobytes(), k
    n = run["resign_stats"]["holdout_games"]
    assert n > 1 and len(small["rows"]) == 1 and small["rows"][0].tobytes() in {w.tobytes() for w in run["rows"]}
    assert small["resign_stats"] == dict(run["resign_stats"], rows_dropped=n - 1) and small["stats"] == run["stats"]
    none = _play(ev, dict(threshold=THRESHOLD, check_steps=STEPS, holdout_prob=HOLDOUT, max_rows=0))
    assert len(none["rows"]) == 0 and none["resign_stats"]["rows_dropped"] == n and none["results"].tobytes() == run["results"].tobytes()
