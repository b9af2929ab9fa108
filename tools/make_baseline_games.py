#!/usr/bin/env python3
"""A teacher corpus out of the shipped baseline: ladder matches between fixed-depth alpha-beta players, written as game text.

    python tools/make_baseline_games.py --depths 3:3 --games 1024 --opening-plies 4 --seed 0 --out games/ladder_d3.txt
    python tools/make_baseline_games.py --depths 3:3,3:2,2:3 --games 512 --out games/ladder_mix.txt

--depths is a comma-separated mix of A:B pairs; every pair is one match of --games games (`baseline.play_vs_baseline(A, games, B,
...)`: depth A in the first seat, which is red in even games, depth B in the other; colour-swapped pairs share an opening of
--opening-plies uniformly random plies).  Match k of the mix plays on seed --seed + k, and its games get game_seq = k, so
(slot, game_seq) stays a key over the whole file.  The file is `sample_format.records_to_text`'s format, one game per line: what
`config.pretrain_records` and `sample_format.records_from_text` read.  A summary of every match goes to stdout as JSON."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parse_depths(text):
    pairs = []
    for word in text.split(","):
        a, _, b = word.strip().partition(":")
        pairs.append((int(a), int(b if b else a)))
    return pairs


def play(depths, games, opening_plies, seed, max_game_length=200):
    """-> (records of every match, in order; one summary row per match)."""
    import numpy as np
    from xiangqi_alphazero_amd import baseline
    records, rows = [], []
    for k, (a, b) in enumerate(depths):
        res = baseline.play_vs_baseline(int(a), games, int(b), 0, opening_plies=opening_plies, seed=seed + k,
                                        max_game_length=max_game_length)
        rec = res["game_records"].copy()
        rec["game_seq"] = k
        records.append(rec)
        rows.append({"first_seat_depth": a, "other_depth": b, "games": games, "seed": seed + k, "opening_plies": opening_plies,
                     "first_seat_win_rate": res["win_rate"], "draws": res["draws"], "mean_plies": round(float(rec["n_moves"].mean()), 2),
                     "plies": int(rec["n_moves"].sum()), "seconds": round(res["seconds"], 2)})
    return np.concatenate(records), rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--depths", default="3:3")
    ap.add_argument("--games", type=int, default=1024, help="games per match of the mix (even)")
    ap.add_argument("--opening-plies", type=int, default=4)
    ap.add_argument("--max-game-length", type=int, default=200)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    from xiangqi_alphazero_amd.sample_format import records_to_text
    records, rows = play(parse_depths(args.depths), args.games, args.opening_plies, args.seed, args.max_game_length)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(records_to_text(records))
    print(json.dumps({"tool": "tools/make_baseline_games.py", "out": args.out, "games": int(len(records)), "matches": rows}, indent=1))


if __name__ == "__main__":
    main()
