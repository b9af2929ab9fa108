#!/usr/bin/env python3
"""A puzzle file out of games: every position of a game collection in which the side to move forces mate.

    python tools/make_puzzles.py --games games/ladder_d3.txt --max-moves 3 --out puzzles/ladder_d3_n3.txt
    python tools/make_puzzles.py --play 3:3 --num-games 1024 --seed 0 --max-moves 3 --out puzzles/ladder_d3_n3.txt

--games reads game text (`sample_format.records_from_text`, several files separated by commas); --play plays ladder matches
between fixed-depth alpha-beta players first (`make_baseline_games.play`, the same --play / --num-games / --opening-plies / --seed).
The games become one row per ply after the opening (`hip.records_to_samples`), the rows are labelled on the device in parts of
--part positions (`tactics.label`), and the positions whose best mate-in lies in [--min-moves, --max-moves] are kept, one per
position with mirror images merged (`tactics.select`).  The file is `tactics.puzzles_to_text`'s format: one FEN per line behind a
'#' header with the counts per mate-in.  It holds no labels: `tactics.label` makes them again wherever the file is read.  A summary
goes to stdout as JSON."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def mine(records, max_moves, min_moves=2, checks_only=True, node_limit=None, unique=True, part=16384):
    """-> (puzzles, summary) from game records (GAME_RECORD_DTYPE)."""
    import numpy as np
    from xiangqi_alphazero_amd import hip, tactics
    from xiangqi_alphazero_amd.sample_format import SAMPLE_DTYPE
    t0 = time.time()
    conv = hip.records_to_samples(records, movers=0, skip_opening=True)
    bad = int((conv["status"] != 0).sum().item())
    rows = conv["samples"].cpu().numpy().reshape(-1).view(SAMPLE_DTYPE)
    labelled = [tactics.label(rows[at:at + part], None, max_moves, checks_only, node_limit) for at in range(0, len(rows), part)]
    labelled = np.concatenate(labelled) if labelled else np.zeros(0, dtype=tactics.PUZZLE_DTYPE)
    puzzles = tactics.select(labelled, max_moves, min_moves, unique)
    count = lambda p: {str(m): int((p["mate_in"] == m).sum()) for m in range(1, max_moves + 1)}      # noqa: E731
    return puzzles, {"games": int(len(records)), "games_not_converted": bad, "positions": int(len(rows)),
                     "max_moves": max_moves, "min_moves": min_moves, "checks_only": bool(checks_only), "unique": bool(unique),
                     "positions_by_mate_in": count(labelled), "puzzles": int(len(puzzles)), "puzzles_by_mate_in": count(puzzles),
                     "root_moves_cut": int((labelled["move_mate_in"] == tactics.UNKNOWN).sum()),
                     "seconds": round(time.time() - t0, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", default=None, help="game text files, comma-separated")
    ap.add_argument("--play", default=None, help="ladder matches to play instead, as make_baseline_games.py --depths")
    ap.add_argument("--num-games", type=int, default=1024)
    ap.add_argument("--opening-plies", type=int, default=4)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--max-moves", type=int, default=3)
    ap.add_argument("--min-moves", type=int, default=2)
    ap.add_argument("--all-moves", action="store_true", help="the attacker may play any move (checks only without it)")
    ap.add_argument("--node-limit", type=int, default=None)
    ap.add_argument("--keep-duplicates", action="store_true")
    ap.add_argument("--part", type=int, default=16384)
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    if (args.games is None) == (args.play is None):
        ap.error("give --games or --play")
    import numpy as np
    from xiangqi_alphazero_amd import tactics
    from xiangqi_alphazero_amd.sample_format import records_from_text
    matches = None
    if args.games:
        records = np.concatenate([records_from_text(open(p).read()) for p in args.games.split(",")])
    else:
        import make_baseline_games
        records, matches = make_baseline_games.play(make_baseline_games.parse_depths(args.play), args.num_games, args.opening_plies,
                                                    args.seed)
    puzzles, summary = mine(records, args.max_moves, args.min_moves, not args.all_moves, args.node_limit, not args.keep_duplicates,
                            args.part)
    header = ["%d forced mates in %d..%d moves (%s) out of %d positions of %d games" % (
        len(puzzles), args.min_moves, args.max_moves, "any move" if args.all_moves else "checks only", summary["positions"],
        summary["games"]), "per mate-in: " + json.dumps(summary["puzzles_by_mate_in"])]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(tactics.puzzles_to_text(puzzles, header=header))
    print(json.dumps({"tool": "tools/make_puzzles.py", "out": args.out, **summary, **({} if matches is None else {"matches": matches})},
                     indent=1))


if __name__ == "__main__":
    main()
