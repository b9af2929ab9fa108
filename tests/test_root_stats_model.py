"""Pins of tests/root_stats_model.py, the host model of the root statistics per sample (xq_engine_init_rs): what the recorded
games and the S = 100 peaked game give under plain search, tree reuse, the playout cap, forced playouts, the solver, and solver +
tree reuse + cap.  The GPU test (tests/test_root_stats_gpu.py) holds the engine to this model bit for bit; the pins here keep the
model itself from drifting, and state the facts that make the GPU comparison mean something (a value of exactly 1.0, a rule-4
sample whose raw visits are below the budget, targets that differ from z)."""
import numpy as np
import pytest

import golden_io as G
import root_stats_model as RS

LONG = dict(num_simulations=100, c_puct=1.5, temperature_threshold=10, max_game_length=70, random_opening_moves=4,
            enable_resign=False, resign_threshold=-0.9, resign_check_steps=5)
GAMES = [(t["cfg"], t["stub"] == "peaked", t["seed"], t["name"]) for t in G.game_traces()] + [(LONG, True, 31, "long_peaked")]
IDS = [g[3] for g in GAMES]
OPTIONS = ("plain", "reuse", "cap", "forced", "solver", "solver_reuse_cap")


def options(name: str, S: int) -> dict:
    """selfplay_model.play_game's keywords of an option set; the cap is (0.5, S / 4)."""
    cap = (0.5, max(1, S // 4))
    return dict(plain={}, reuse=dict(tree_reuse=True), cap=dict(cap=cap), forced=dict(forced=2.0), solver=dict(solver=True),
                solver_reuse_cap=dict(solver=True, tree_reuse=True, cap=cap))[name]


DIGESTS = {
    "resign/plain": "9a16bc5cc514e10c785dfb1d34a37ab017e5453c5884db85be8946bc28ee07f1",
    "resign/reuse": "004e1ffd425fe3e2719b290e001dc7f7fe9eb7c30398ca7e7fd2cc14939a8aa4",
    "resign/cap": "4be9294938979d6c9049c2ab46841c55418c154df9187748fa4e08916fe66558",
    "resign/forced": "f7d3307b2bdc7305a421fd8194821a1095fd014209f473748070c383f1127c3f",
    "resign/solver": "9a16bc5cc514e10c785dfb1d34a37ab017e5453c5884db85be8946bc28ee07f1",
    "resign/solver_reuse_cap": "a4dcad1c335e17e5491b1a210020c275fa6a018db7bcda189b1a0e3f44b90cbd",
    "maxlen/plain": "1fa17bfc7047ec74cd5981c170b78f759c87334cda1e7b128728bfc63f38d9dd",
    "maxlen/reuse": "cc9f82dd5ba458c668ade02a613d3cbdaa67321efe255ec08b23667a0fe04645",
    "maxlen/cap": "b621d64797f2a13bb0c36816736f7a695275c0fd5a84a778c6234d8ebda6f932",
    "maxlen/forced": "696d0a3b8b7339db2596f7a2e61244b1eceb48a9da60c533a88d12fd7f9b4b35",
    "maxlen/solver": "1fa17bfc7047ec74cd5981c170b78f759c87334cda1e7b128728bfc63f38d9dd",
    "maxlen/solver_reuse_cap": "5cab330fb9218827d76c066c9e5978042e45e72df72e079aef164d3e710f2117",
    "natural/plain": "0a169693c641a809727fc5c39ecf05bb60138d1d733294940907f6151ce0f1d9",
    "natural/reuse": "e5a3454fba3842439cf05a851f506fe69d71351733f25406ff1387c5054dbd9f",
    "natural/cap": "06164d19348e5808199adcab96c2b04ac5d7451a76c75a1842146293a5fbac2e",
    "natural/forced": "ca7ab79268202be5004af72798e6aa4f99630aaf408f3b3fc77ac3f087a8f6cf",
    "natural/solver": "1db4422ca66c3d9007d25668edb864d60c367b3620db31cfe894d1e883045aaa",
    "natural/solver_reuse_cap": "60313024fd601616779eae489f8b5459983511a4ce156383ce8de17e7d80ff47",
    "resign_late/plain": "9e52bd90f572b4479cc64a742c27816484bb91ecd589e9614e8e3cf448cbee12",
    "resign_late/reuse": "b311cf7d56a3d1b13a8192b764943c06406469ff1296ed2fa8efd390299702a5",
    "resign_late/cap": "899ced4a8d382be4d99f3fdab9924530958b7a5a63e950db6271b1ebc85d8324",
    "resign_late/forced": "d02238eb3042c3918ec6ace58ddf09837578c1580fa048f3401b501e831be9b1",
    "resign_late/solver": "9e52bd90f572b4479cc64a742c27816484bb91ecd589e9614e8e3cf448cbee12",
    "resign_late/solver_reuse_cap": "28a5fa730af395e94e7491ba6dcd6104e9215060ca187530f38aa008cc6606eb",
    "long_peaked/plain": "82909c4841e5b9fe4531804ac231595d26efed7e4ff003ca41c0d708e7f89a5e",
    "long_peaked/reuse": "57aede6a19da69df2f6bd35012a30fbd4c54a9b17d533d7f3549258ccfab071d",
    "long_peaked/cap": "eb89bf40d9447b92a0e3c8cc789d2b1a703ce8a2fc72daa0446ed5655e82f2b6",
    "long_peaked/forced": "6272fa59ea17b7f9075b6362146e8cdf13c9f2f2028a2816cb148ee5cba7d50e",
    "long_peaked/solver": "6df9ce79a52b9ba46ed6e615d338eb1c62aff5f7cb909e0407326ede1d554676",
    "long_peaked/solver_reuse_cap": "4c807eff57ecebc8074f60b7f9363d585244dbba8184adc67197f500e826e035",
}

_cache = {}


def model_game(game, opt):
    """(samples, winner, plies, stats) of the model, computed once per (game, option set) and shared; never modified."""
    c, peaked, seed, name = game
    key = (name, opt)
    if key not in _cache:
        _cache[key] = RS.play_game(c, peaked, seed, **options(opt, int(c["num_simulations"])))
    return _cache[key]


@pytest.mark.parametrize("opt", OPTIONS)
@pytest.mark.parametrize("game", GAMES, ids=IDS)
def test_model_pins(game, opt):
    c, _, _, name = game
    S = int(c["num_simulations"])
    samples = model_game(game, opt)[0]
    q = np.array([s["root_q"] for s in samples], dtype=np.float32)
    assert q.dtype == np.float32 and len(samples) > 0
    assert (np.abs(q) <= 1.0).all() and (q != 0.0).all()
    proven = [k for k, s in enumerate(samples) if s["proven"]]
    for k, s in enumerate(samples):
        if k in proven:
            assert s["root_q"] == np.float32(1.0)
        else:
            assert s["root_visits"] == S, k
    if (name, opt) == ("long_peaked", "solver"):       # the one rule-4 sample: the raw visits of an early end, below the budget
        assert proven == [31] and samples[31]["root_visits"] == 79
    else:
        assert proven == []
    assert RS.digest(samples) == DIGESTS["%s/%s" % (name, opt)]
    assert all(len(RS.pad_bytes(s)) == 20 for s in samples)


def test_value_of_exactly_one_without_the_solver():
    """`natural` (S = 16) holds a position whose every simulation came back won: root_q == 1.0 from the division itself."""
    samples = model_game(GAMES[IDS.index("natural")], "plain")[0]
    assert sum(1 for s in samples if s["root_q"] == np.float32(1.0)) == 1 and not any(s["proven"] for s in samples)


@pytest.mark.parametrize("name, differ, total", [("resign", 10, 18), ("natural", 104, 199), ("long_peaked", 36, 68)])
def test_a_mixed_target_differs_from_z(name, differ, total):
    samples = model_game(GAMES[IDS.index(name)], "plain")[0]
    assert len(samples) == total
    assert sum(1 for s in samples if np.sign(s["root_q"]) != s["z"]) == differ


def test_root_q_arithmetic():
    assert RS.root_q_of(0.0, 0, False) == np.float32(0.0) and RS.root_q_of(-3.0, 0, True) == np.float32(1.0)
    assert RS.root_q_of(1.0, 3, False) == np.float32(1.0 / 3.0)                # one rounding: float64 quotient -> float32
    assert RS.root_q_of(-0.1 - 0.2, 3, False) == np.float32((-0.1 - 0.2) / 3.0)
    assert RS.pad_bytes(dict(root_q=np.float32(1.0), root_visits=79)) == b"\x00\x00\x80\x3f" + b"\x4f\x00\x00\x00" + b"\x01" + bytes(11)
