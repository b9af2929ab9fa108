#!/usr/bin/env python3
"""Game records as text.  Reads a .npy of records -- a structured array of GAME_RECORD_DTYPE as `SelfPlayEngine.drain_games` and
`run_games(record_games=True)` return it, or the uint8 [n, 1024] bytes of a device drain -- and prints one game per line: the
moves as ICCS coordinates, the result, then reason, opening_plies, n_samples, slot and game_seq (sample_format.records_to_text).
Needs no GPU.

    python tools/games_to_text.py games.npy [-o games.txt]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from xiangqi_alphazero_amd.sample_format import GAME_RECORD_DTYPE, records_to_text  # noqa: E402


def load_records(path: str) -> np.ndarray:
    a = np.load(path)
    if a.dtype == np.uint8:
        a = np.ascontiguousarray(a).reshape(-1).view(GAME_RECORD_DTYPE)
    if a.dtype != GAME_RECORD_DTYPE:
        raise SystemExit(f"{path}: neither game records nor their bytes (dtype {a.dtype})")
    return a.reshape(-1)


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("records", help=".npy of game records")
    ap.add_argument("-o", "--output", help="write here instead of standard output")
    args = ap.parse_args()
    text = records_to_text(load_records(args.records))
    if args.output:
        with open(args.output, "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()
