"""k_game_over judges through the engine's wave_game_over: its oldest-first history rows are staged into the 12-row ring that
function reads, entry e of the k = min(12, move_count) valid ones into row (move_count - k + e) % 12.  This pins that mapping.

One 18-ply record from the initial position: two pawn moves, then four rounds of both left rooks stepping forward and back.
Every ply is legal; on the CPU oracle the game is not over at plies 0..13 and is a repetition draw at ply 14, with the
perpetual-check rule off and on (nobody checks).  The replay kernel walks the record with the engine's own ring and reports
wave_game_over's verdict at each stop ply; its board, side, counters and oldest-first hist12 then go through
xq_game_over_batch_ex.  Stop plies 0..14 cover k < 12, k = 12 and a ring that has wrapped by two rows.

That record's verdicts only count equal rows, which any placement of the rows leaves alone.  The perpetual-check rule reads them
in order, so the second test judges order-sensitive positions with a wrapped ring against the host model: the model's short_span
fixtures (a quiet board just outside the span, or inside it) at move counts 13..23, every rotation of the ring but none, and its
three checking cycles played on to plies 13, 14 and 15.  The model test before it shows that the rows do tell placements apart.
"""
import numpy as np
import pytest

import perpetual_check_model as PC
from oracle import xq_oracle as O

STOPS = list(range(15))


def _act(fr, fc, tr, tc):
    return (fr * 9 + fc) * 90 + tr * 9 + tc


MOVES = [_act(3, 0, 4, 0), _act(6, 0, 5, 0)] + [_act(0, 0, 1, 0), _act(9, 0, 8, 0), _act(1, 0, 0, 0), _act(8, 0, 9, 0)] * 4


def test_record_is_legal_and_draws_at_ply_14_on_the_oracle():
    g = O.Game()
    for ply, a in enumerate(MOVES):
        if ply <= 13:
            assert g.is_game_over()[0] is False
        elif ply == 14:
            assert g.is_game_over() == (True, 0)
        assert a in g.legal_actions(), ply
        g.make_action(a)


@pytest.mark.gpu
@pytest.mark.parametrize("perpetual", [False, True], ids=["rule_off", "rule_on"])
def test_game_over_batch_equals_the_replay_verdict_and_the_model(perpetual):
    import torch

    from xiangqi_alphazero_amd import engine, hip
    assert len(MOVES) == 18
    rec = np.zeros(1, dtype=hip.GAME_RECORD_DTYPE)
    rec["n_moves"][0] = len(MOVES)
    rec["moves"][0, :len(MOVES)] = MOVES
    at = engine.replay_games(np.repeat(rec, len(STOPS)), stop_ply=STOPS, perpetual_check=perpetual)
    assert not at["status"].any().item() and at["move_count"].cpu().tolist() == STOPS
    out, kind = hip.game_over_batch(at["board"], at["side"], at["move_count"], at["no_capture"], at["hist12"],
                                    perpetual_check=perpetual, return_kind=True)
    torch.cuda.synchronize()
    host = {k: v.cpu().numpy() for k, v in at.items()}
    out, kind = out.cpu().numpy(), kind.cpu().numpy()
    for i, ply in enumerate(STOPS):
        over_kind, winner = int(host["over_kind"][i]), int(host["winner"][i])
        got = (int(out[i, 0]), int(out[i, 1]), int(kind[i]))
        print(f"ply {ply}: replay over_kind {over_kind} winner {winner}; game_over_batch done {got[0]} winner {got[1]} kind {got[2]}")
        assert got[0] == int(over_kind != 0), ply
        assert got[1] == winner, ply
        assert (got[2] == PC.PERPETUAL) == (over_kind == 4), ply
        assert (got[2], got[1]) == ((PC.NOT_OVER, 2) if ply <= 13 else (PC.REPETITION, 0)), ply
        k = min(12, ply)
        want = PC.verdict(host["board"][i], host["side"][i], host["move_count"][i], host["no_capture"][i], host["hist12"][i][:k],
                          perpetual)
        assert (got[2], got[1]) == want, ply


def _ordered_rows():
    """[(name, (board, side, move_count, no_capture, hist oldest first))] whose verdict under the rule depends on the rows' order."""
    rows = []
    for name, (board, side, _, nc, hist), _, _ in PC.synthetic_cases():
        if name.startswith("short_span"):
            rows += [(f"{name}@{mc}", (board, side, mc, nc, hist)) for mc in range(13, 24)]
    for make in (PC.pc_red, PC.pc_black, PC.pc_red_rotated):
        rows += [(f"{make.__name__}@{plies}", PC.state_of(make(plies))) for plies in (13, 14, 15)]
    return rows


def _verdict_through_ring(row_of, board, side, mc, nc, hist):
    """The model's verdict, rule on, when entry e of the 12 oldest-first rows is staged into ring row row_of(mc, e) and read back
    as wave_game_over reads the ring: the board e + 1 plies ago in row (mc - 1 - e) % 12."""
    ring = np.zeros((12, 90), dtype=np.int8)
    for e in range(12):
        ring[row_of(mc, e)] = hist[e]
    newest_first = [ring[(mc - 1 - e) % 12] for e in range(12)]
    return PC.verdict(board, side, mc, nc, np.stack(newest_first[::-1]), True)


def test_ordered_rows_tell_ring_placements_apart_in_the_model():
    rows = dict(_ordered_rows())
    for name, state in rows.items():
        assert _verdict_through_ring(lambda mc, e: (mc - 12 + e) % 12, *state) == PC.verdict(*state, True), name
    for mc in range(13, 24):                           # every rotation but none: unrotated rows, then the order reversed
        state, want = rows[f"short_span@{mc}"], (PC.PERPETUAL, -1)
        assert PC.verdict(*state, True) == want
        assert _verdict_through_ring(lambda mc, e: e, *state) != want, mc
        assert _verdict_through_ring(lambda mc, e: (mc - 1 - e) % 12, *state) != want, mc


@pytest.mark.gpu
def test_game_over_batch_reads_a_wrapped_history_in_order():
    import torch

    from xiangqi_alphazero_amd import hip
    names, states = zip(*_ordered_rows())
    dev = lambda col, dtype: torch.from_numpy(np.stack([np.asarray(st[col], dtype=dtype) for st in states])).cuda()
    args = (dev(0, np.int8), dev(1, np.int8), dev(2, np.int32), dev(3, np.int32), dev(4, np.int8))
    for perpetual in (False, True):
        out, kind = hip.game_over_batch(*args, perpetual_check=perpetual, return_kind=True)
        out, kind = out.cpu().numpy(), kind.cpu().numpy()
        for i, name in enumerate(names):
            got, want = (int(kind[i]), int(out[i, 1])), PC.verdict(*states[i], perpetual)
            print(f"{name} rule {int(perpetual)}: kind {got[0]} winner {got[1]}; model {want}")
            assert got == want and int(out[i, 0]) == 1, (name, perpetual)
        assert perpetual == bool((kind == PC.PERPETUAL).any())
