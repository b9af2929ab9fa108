"""The grid of engine shapes behind tests/golden/workspace_bytes.json, and the generator of that fixture.

    python tests/workspace_grid.py <libxq_hip.so built from the commit to record> [out.json]

calls xq_engine_workspace_bytes_sp over the whole grid (CPU only: nothing is launched) and stores the accepted cases with their
sizes; every case that is not stored returned 0.  tests/test_workspace_map.py holds the current build to the stored sizes, so the
fixture is recorded from the PARENT of a commit that touches the layout, never from that commit itself."""
import ctypes as C
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "workspace_bytes.json")
PTR = 4096              # a pointer that is not NULL and is never followed: no call here launches anything

# G, S, manual_moves, K, Gumbel m (0: off), arena options (2, 0) or off, solver, records' max_out_games (0: off), pool n (0: off)
AXES = ((1, 5, 64), (1, 7, 100), (0, 1, 2), (1, 4), (0, 1, 16), (0, 1), (0, 1), (0, 1, 5), (0, 1, 3))
FIELDS = ("G", "S", "manual_moves", "K", "gumbel_m", "arena", "solver", "max_out_games", "pool_n")


def cases():
    return list(itertools.product(*AXES))


def arguments(case):
    """The arguments of xq_engine_workspace_bytes_sp (and, with one more, xq_engine_option_words_sp) for a case; the structs are
    returned too so that they outlive the call."""
    from xiangqi_alphazero_amd import engine, hip
    G, S, mm, K, m, arena, solver, M, n = case
    cfg = engine.make_config(G, S, manual_moves=mm)
    opts = (None, None, hip.Gumbel(m, 0, 50.0, 1.0) if m else None, hip.ArenaOpts(2, 0) if arena else None, None,
            hip.SolverOpts(1) if solver else None, None, None, hip.GameRecordsOpts(1, M) if M else None,
            hip.StartPool(PTR, PTR, n, 0, 0.5) if n else None)
    return (C.byref(cfg), K, 0) + tuple(None if o is None else C.byref(o) for o in opts), (cfg, opts)


def workspace_bytes(lib, case):
    args, keep = arguments(case)
    return int(lib.xq_engine_workspace_bytes_sp(*args))


def main():
    sys.path.insert(0, ROOT)
    lib = C.CDLL(os.path.abspath(sys.argv[1]))
    lib.xq_engine_workspace_bytes_sp.restype = C.c_size_t
    sized = [(c, workspace_bytes(lib, c)) for c in cases()]
    accepted = [list(c) + [b] for c, b in sized if b]
    out = sys.argv[2] if len(sys.argv) > 2 else FIXTURE
    with open(out, "w") as f:
        f.write('{"fields": %s,\n "calls": %d,\n "accepted": [\n' % (json.dumps(list(FIELDS) + ["bytes"]), len(sized)))
        f.write(",\n".join("  " + json.dumps(a) for a in accepted) + "\n ]}\n")
    print(f"{len(sized)} calls, {len(accepted)} accepted, {len({a[-1] for a in accepted})} distinct sizes -> {out}")


if __name__ == "__main__":
    main()
