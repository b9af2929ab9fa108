"""ctypes loader of libxq_hip.so (C ABI: include/xq_hip.h) plus thin torch-tensor adapters.

The product path has NO CPU fallback: if the library is missing or a call fails, this module raises.
torch is used only for device memory and streams; every computation below runs in the HIP kernels.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import torch  # imported BEFORE the library is loaded: both must share one HIP runtime (libamdhip64.so.7)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("XQ_HIP_LIB", os.path.join(_HERE, "libxq_hip.so"))   # override: perf experiments only
CSRC = os.path.join(_HERE, "csrc")

# numpy only: the records' layouts live with the other formats
from .sample_format import GAME_RECORD_DTYPE, POLICY_STATS_DTYPE, RESIGN_ROW_DTYPE, SCORE_DTYPE  # noqa: E402,F401

MAXM = 128
SAMPLE_BYTES = 640
RESULT_BYTES = 16
ACTION_SPACE = 8100
STATE_FLOATS = 1350
ENGINE_TREE_REUSE = 1          # XQ_ENGINE_TREE_REUSE
ARENA_MAX_OPENING = 16         # XQ_ARENA_MAX_OPENING
REUSE_MAX_SIMS = 1600          # XQ_REUSE_MAX_SIMS
RECORD_MAX_PLIES = 504         # XQ_RECORD_MAX_PLIES
RECORD_BYTES = 1024            # XQ_RECORD_BYTES
POSITION_KEY_MIRROR = 1        # XQ_POSITION_KEY_MIRROR
AB_MAX_DEPTH = 4               # XQ_AB_MAX_DEPTH
AB_MATE = 30000                # XQ_AB_MATE
AB_UNSCORED = -2 ** 31         # XQ_AB_UNSCORED
AB_NO_MOVE = 0xFFFF            # XQ_AB_NO_MOVE
MATE_MAX_MOVES = 5             # XQ_MATE_MAX_MOVES
MATE_UNKNOWN = 255             # XQ_MATE_UNKNOWN
MATE_NO_MOVE = 0xFFFF          # XQ_MATE_NO_MOVE
MATE_DEFAULT_NODE_LIMIT = 10000    # visits per root move
TB_MAX_PIECES = 5              # XQ_TB_MAX_PIECES
TB_MAX_ENTRIES = 1 << 28       # XQ_TB_MAX_ENTRIES
TB_MAX_PASSES = 32000          # XQ_TB_MAX_PASSES
TB_INVALID = -32768            # XQ_TB_INVALID
TB_NO_MOVE = 0xFFFF            # XQ_TB_NO_MOVE
POSITION_FATAL = 15            # XQ_POSITION_FATAL: the bits of positions_check that refuse a position
POSITION_NO_MOVE = 16          # XQ_POSITION_NO_MOVE: the side to move has no legal move (the game is over at ply 0)
START_POOL_MAX = 1 << 20       # XQ_START_POOL_MAX
RNG_KIND_START_POOL = 11       # XQ_RNG_KIND_START_POOL
REASON_TABLE = 5               # XQ_REASON_TABLE: a result's reason for a game an endgame table adjudicated
RNG_KIND_RESIGN_HOLDOUT = 12   # XQ_RNG_KIND_RESIGN_HOLDOUT
RESIGN_MAX_STEPS = 8           # XQ_RESIGN_MAX_STEPS


class XqError(RuntimeError):
    pass


def build(force: bool = False) -> str:
    """Compile the HIP sources for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    srcs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hip", ".cuh", ".h"))]
    srcs.append(os.path.join(_HERE, "..", "include", "xq_hip.h"))
    stale = (not os.path.exists(LIB_PATH)) or os.path.getmtime(LIB_PATH) < max(os.path.getmtime(s) for s in srcs)
    if force or stale:
        subprocess.check_call(["make", "-s", "-j4", "-C", CSRC, "all"])
    return LIB_PATH


class EngineConfig(C.Structure):
    _fields_ = [("n_games", C.c_int32), ("num_simulations", C.c_int32), ("c_puct", C.c_double),
                ("temperature_threshold", C.c_int32), ("max_game_length", C.c_int32),
                ("random_opening_moves", C.c_int32), ("enable_resign", C.c_int32),
                ("resign_threshold", C.c_double), ("resign_check_steps", C.c_int32), ("add_noise", C.c_int32),
                ("dirichlet_alpha", C.c_double), ("noise_eps", C.c_double), ("late_temperature", C.c_double),
                ("seed", C.c_uint64), ("rank", C.c_int32), ("inject_len", C.c_int32),
                ("games_target", C.c_int64), ("max_out_samples", C.c_int32), ("max_out_results", C.c_int32),
                ("manual_moves", C.c_int32), ("start_stagger", C.c_int32)]


class Engine(C.Structure):
    _fields_ = [("cfg", EngineConfig), ("node_cap", C.c_int32), ("path_cap", C.c_int32),
                ("stage_cap", C.c_int32), ("pad0", C.c_int32), ("p", C.c_void_p * 32)]


# Where Python looks into the workspace: indices into Engine.p, columns of a slot's 32 state words, one phase value.
P_BOARD = 0        # mirrors P_BOARD of enum Ptr in csrc/xq_engine_state.cuh: the real games' boards
P_GI = 2           # mirrors P_GI of enum Ptr: the per-slot state words
P_TN, P_TW, P_TP, P_TA, P_TC, P_TM = 6, 7, 8, 9, 10, 11   # mirror P_TN .. P_TM of enum Ptr: the six tree arrays
P_ROOTP = 12       # mirrors P_ROOTP of enum Ptr: the float64 root priors
P_OUTS, P_OUTR = 14, 15   # mirror P_OUTS, P_OUTR of enum Ptr: the sample ring and the result ring that the drains read
P_STATS = 17       # mirrors P_STATS of enum Ptr: the per-slot counters
P_SQRT = 19        # mirrors P_SQRT of enum Ptr: the square-root table's region, which holds every option's words (OptionWords)
P_VL = 30          # mirrors P_VL of enum Ptr: the virtual-loss counters (leaves_per_step > 1)
GI_SIDE = 0        # mirrors GI_SIDE of enum Gi in csrc/xq_engine_state.cuh: side to move of the real game
GI_MC = 1          # mirrors GI_MC of enum Gi: its move count
GI_PHASE = 3       # mirrors GI_PHASE of enum Gi
GI_SIMS = 4        # mirrors GI_SIMS of enum Gi: simulations done
GI_GSEQ = 6        # mirrors GI_GSEQ of enum Gi: the slot's game sequence number
GI_ALLOC = 7       # mirrors GI_ALLOC of enum Gi: the tree's allocation mark
GI_RSTATUS = 11    # mirrors GI_RSTATUS of enum Gi: the root's terminal status (0 searched, 1 rules, 2 max length, 4 perpetual check)
GI_RWINNER = 12    # mirrors GI_RWINNER of enum Gi: the winner that goes with a non-zero status
GI_RNG0 = 14       # mirrors GI_RNG0 of enum Gi: the first of the four stream counters
PH_HOLD = 7        # mirrors PH_HOLD of enum Phase in csrc/xq_engine_state.cuh


class EngineStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in
                ("sims", "terminal_sims", "leaf_evals", "root_evals", "moves_played", "games_finished", "red_wins",
                 "black_wins", "draws", "plies_finished", "nodes_created", "depth_sum", "children_scanned", "resigns",
                 "samples_written", "samples_dropped", "overflow", "games_started", "rows_evaluated", "collisions",
                 "leaves_per_step_sum", "leaf_steps", "reused_visits", "reroots", "fast_moves", "fast_sims", "forced_sims",
                 "pruned_visits", "pruned_children")] + [("reserved", C.c_uint64 * 3)]

    # the Gumbel root search's counters (xq_engine_init_gz) are the struct's last three words, kept under `reserved`
    GUMBEL_KEYS = ("gumbel_moves", "gumbel_considered", "gumbel_offprior")

    def as_dict(self):
        out = {n: int(getattr(self, n)) for n, _ in self._fields_ if n != "reserved"}
        out.update({n: int(self.reserved[i]) for i, n in enumerate(self.GUMBEL_KEYS)})
        return out


class PlayoutCap(C.Structure):
    """xq_playout_cap: playout cap randomization (xq_engine_init_cap): S_fast and the probability p of a full search."""
    _fields_ = [("fast_simulations", C.c_int32), ("reserved", C.c_int32), ("full_search_prob", C.c_double)]


class ForcedPlayouts(C.Structure):
    """xq_forced_playouts: forced playouts and policy target pruning (xq_engine_init_fp): the parameter k."""
    _fields_ = [("k", C.c_double), ("reserved", C.c_uint32 * 2)]


class Gumbel(C.Structure):
    """xq_gumbel: Gumbel root search with sequential halving (xq_engine_init_gz): considered moves m, c_visit, c_scale."""
    _fields_ = [("considered", C.c_int32), ("reserved", C.c_int32), ("c_visit", C.c_double), ("c_scale", C.c_double)]


class ArenaOpts(C.Structure):
    """xq_arena_opts: arena options (xq_engine_init_ar): opening plies R of the paired random openings, game index of slot 0."""
    _fields_ = [("opening_plies", C.c_int32), ("first_game", C.c_int32), ("reserved", C.c_uint32 * 2)]


class RulesOpts(C.Structure):
    """xq_rules_opts: rules options (xq_engine_init_ru, xq_game_over_batch_ex): the side that checks through a repetition loses."""
    _fields_ = [("perpetual_check", C.c_int32), ("reserved", C.c_int32 * 3)]


class SolverOpts(C.Structure):
    """xq_solver_opts: proven-result search (xq_engine_init_sv): enabled 0 / 1."""
    _fields_ = [("enabled", C.c_int32), ("reserved", C.c_int32 * 3)]


class RootStatsOpts(C.Structure):
    """xq_root_stats_opts: the root's search value per sample (xq_engine_init_rs): enabled 0 / 1."""
    _fields_ = [("enabled", C.c_int32), ("reserved", C.c_int32 * 3)]


class EvalMirrorOpts(C.Structure):
    """xq_eval_mirror_opts: random mirror of the packed step's evaluation requests (xq_engine_init_em): mode 0 off / 1 random."""
    _fields_ = [("mode", C.c_int32), ("reserved", C.c_int32 * 3)]


class GameRecordsOpts(C.Structure):
    """xq_game_records_opts: game records (xq_engine_init_gr): enabled 0 / 1, rows of the ring of finished games."""
    _fields_ = [("enabled", C.c_int32), ("max_out_games", C.c_int32), ("reserved", C.c_int32 * 2)]


class GameRecordsStats(C.Structure):
    """xq_game_records_stats: games whose record found a row of the ring, and games that did not (xq_engine_game_records_stats_read)."""
    _fields_ = [("recorded", C.c_uint64), ("dropped", C.c_uint64), ("reserved", C.c_uint64 * 2)]


class StartPool(C.Structure):
    """xq_start_pool: the start-position pool (xq_engine_init_sp): n boards int8[n][90] and sides int8[n] on the device, and the
    probability that a new game starts from one of them."""
    _fields_ = [("dev_boards", C.c_void_p), ("dev_side", C.c_void_p), ("n", C.c_int32), ("reserved", C.c_int32),
                ("prob", C.c_double)]


class StartPoolStats(C.Structure):
    """xq_start_pool_stats: games started from the pool (xq_engine_start_pool_stats_read)."""
    _fields_ = [("pool_games", C.c_uint64), ("reserved", C.c_uint64 * 3)]


class WordsBlock(C.Structure):
    """xq_words_block: a block of the option words, offset from the region's first byte; bytes = 0: the engine has no such block."""
    _fields_ = [("offset", C.c_uint64), ("bytes", C.c_uint64)]


class OptionWords(C.Structure):
    """xq_option_words: where every option's device words lie in the square-root table's region (xq_engine_option_words_sp;
    include/xq_hip.h: THE OPTION WORDS)."""
    _fields_ = [("bytes", C.c_uint64)] + \
               [(n, WordsBlock) for n in ("table", "gz_head", "gz_vhat", "gz_visits", "ar_head", "ar_op_counts", "ar_op_actions",
                                          "ar_n_live")] + \
               [(n, WordsBlock * 2) for n in ("ar_rows", "ar_x", "ar_moves", "ar_counts")] + \
               [(n, WordsBlock) for n in ("solver", "gr_ring", "gr_log", "gr_opening", "gr_head", "sp_rows", "sp_index", "sp_head")]


class GameRecord(C.Structure):
    """xq_game_record: one finished game, 1024 bytes."""
    _fields_ = [("slot", C.c_uint32), ("game_seq", C.c_uint32), ("winner", C.c_int8), ("reason", C.c_uint8),
                ("n_moves", C.c_uint16), ("opening_plies", C.c_uint16), ("n_samples", C.c_uint16),
                ("moves", C.c_uint16 * RECORD_MAX_PLIES)]


# xq_game_record as a numpy record: what drain_games returns, what replay_games and sample_format.records_to_text take
assert GAME_RECORD_DTYPE.itemsize == RECORD_BYTES == C.sizeof(GameRecord)


class SuperviseOpts(C.Structure):
    """xq_supervise_opts: which plies of a game record become samples (xq_records_sample_counts / xq_records_to_samples): movers
    0 every ply, 1 the winner's, 2 red's, 3 black's; skip_opening and skip_draws 0 / 1."""
    _fields_ = [("movers", C.c_int32), ("skip_opening", C.c_int32), ("skip_draws", C.c_int32), ("reserved", C.c_int32)]


class TbSampleOpts(C.Structure):
    """xq_tb_sample_opts: table entries as samples (xq_tb_samples): policy 0 every optimal move is a target, 1 the first one."""
    _fields_ = [("policy", C.c_int32), ("reserved", C.c_int32 * 3)]


class AdjudicateOpts(C.Structure):
    """xq_adjudicate_opts: table adjudication (xq_tb_adjudicate_batch / xq_engine_adjudicate): draws 1 a drawn entry ends the game,
    both_colours 1 the colour-swapped image is matched too, min_ply the shortest game the engine stage looks at."""
    _fields_ = [("draws", C.c_int32), ("both_colours", C.c_int32), ("min_ply", C.c_int32), ("reserved", C.c_int32)]


class ResignOpts(C.Structure):
    """xq_resign_opts: the per-side resign rule (xq_engine_resign): resign when the K latest values of the side to move are all
    below threshold; holdout_prob the share of games that are exempt and played out."""
    _fields_ = [("threshold", C.c_double), ("holdout_prob", C.c_double), ("check_steps", C.c_int32), ("reserved", C.c_int32)]


class ResignRow(C.Structure):
    """xq_resign_row: one finished holdout game: the lowest window of each side and the ply it was first reached at."""
    _fields_ = [("slot", C.c_uint32), ("game_seq", C.c_uint32), ("level", C.c_float * 2), ("level_ply", C.c_uint16 * 2),
                ("winner", C.c_int8), ("reason", C.c_uint8), ("plies", C.c_uint16), ("zero", C.c_uint32 * 2)]


RESIGN_ROW_BYTES = 32            # sizeof(xq_resign_row)
RESIGN_STATE_BYTES = 32          # xq_resign_state_bytes(1)
assert C.sizeof(ResignRow) == RESIGN_ROW_BYTES == RESIGN_ROW_DTYPE.itemsize and C.sizeof(ResignOpts) == 24


class MateOpts(C.Structure):
    """xq_mate_opts: the forced-mate search (xq_mate_search_batch): N attacker moves, checks only 0 / 1, visits per root move."""
    _fields_ = [("max_moves", C.c_int32), ("checks_only", C.c_int32), ("node_limit", C.c_uint32), ("reserved", C.c_uint32)]


class BatchOpts(C.Structure):
    """xq_batch_opts: the q-mixed value target of xq_samples_to_batch_ex: q_mix in [0, 1]."""
    _fields_ = [("q_mix", C.c_double), ("reserved", C.c_int32 * 2)]


class ScoreOpts(C.Structure):
    """xq_score_opts: scoring samples against a network (xq_score_samples): the samples' late temperature, write_back 0 / 1."""
    _fields_ = [("late_temperature", C.c_double), ("write_back", C.c_int32), ("reserved", C.c_int32)]


class SampleScore(C.Structure):
    """xq_sample_score: one sample against one network: KL and cross-entropy of the search target against the raw prior, the
    network's value, whether the prior's first choice is the search's, and whether the row could be scored at all."""
    _fields_ = [("policy_kl", C.c_float), ("policy_ce", C.c_float), ("value", C.c_float), ("top1", C.c_uint8),
                ("valid", C.c_uint8), ("zero", C.c_uint8 * 2)]


class SamplePolicyStats(C.Structure):
    """xq_sample_policy_stats: what xq_score_samples writes back into a record, at byte POLICY_STATS_OFFSET."""
    _fields_ = [("policy_kl", C.c_float), ("has_policy_stats", C.c_uint8), ("prior_top1", C.c_uint8), ("zero", C.c_uint8 * 2)]


class SurpriseOpts(C.Structure):
    """xq_surprise_opts: the epoch counts of policy-surprise weighted training (xq_surprise_counts): alpha in [0, 1]."""
    _fields_ = [("alpha", C.c_double), ("seed", C.c_uint64), ("epoch", C.c_uint32), ("reserved", C.c_uint32)]


SCORE_BYTES = 16                 # sizeof(xq_sample_score)
POLICY_STATS_OFFSET = 120        # XQ_SAMPLE_POLICY_STATS_OFFSET
SURPRISE_SCRATCH_BYTES = 16      # XQ_SURPRISE_SCRATCH_BYTES
RNG_KIND_SURPRISE = 10           # XQ_RNG_KIND_SURPRISE
assert C.sizeof(SampleScore) == SCORE_BYTES == SCORE_DTYPE.itemsize and C.sizeof(SamplePolicyStats) == POLICY_STATS_DTYPE.itemsize


class SolverStats(C.Structure):
    """xq_solver_stats: the proven-result search's counters (xq_engine_solver_stats_read)."""
    _fields_ = [(n, C.c_uint64) for n in ("proven_nodes", "proven_stops", "proven_moves", "unspent_sims", "removed_visits")] + \
               [("reserved", C.c_uint64 * 3)]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_ if n != "reserved"}


SOLVER_KEYS = ("proven_nodes", "proven_stops", "proven_moves", "unspent_sims", "removed_visits")
META_COUNT_MASK = 0x0FFF       # XQ_CNT_MASK of csrc/xq_engine_state.cuh: the child count in a node's meta word (bits 12-13: its
                               # proven state, 14-15: the prior kind)

# what ended a game, xq_game_over_batch_ex's dev_kind
OVER_KINDS = ("not_over", "king_missing", "no_legal_move", "no_capture", "ply_200", "repetition_draw", "perpetual_check")


class PackedBuffers(C.Structure):
    """xq_engine_packed_buffers: device addresses of the packed step's buffers in the engine workspace."""
    _fields_ = [(n, C.c_void_p) for n in ("n_live", "rows", "x", "moves", "counts", "slot_logits", "slot_value")]


class EvCache(C.Structure):
    """xq_evcache: the evaluation cache's geometry and device addresses (opaque)."""
    _fields_ = [("n_slots", C.c_int32), ("entries", C.c_int32), ("ways", C.c_int32), ("sets", C.c_int32),
                ("p", C.c_void_p * 16)]


class EvCacheStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("probes", "hits", "inserts", "evictions", "mismatches")] + [("reserved", C.c_uint64 * 3)]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_ if n != "reserved"}


class EvDedup(C.Structure):
    """xq_evdedup: the request dedup's geometry and device addresses (opaque)."""
    _fields_ = [("n_slots", C.c_int32), ("table_size", C.c_int32), ("reserved", C.c_int32 * 2), ("p", C.c_void_p * 8)]


class EvDedupStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("requests", "merged", "collisions", "mismatches")] + [("reserved", C.c_uint64 * 4)]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_ if n != "reserved"}


_lib = None


def lib():
    """Load libxq_hip.so; raises XqError when it is absent (no silent fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise XqError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                      "(hipcc --offload-arch=gfx950); there is no CPU fallback for the product path")
    L = C.CDLL(LIB_PATH)
    vp, i32, u64p = C.c_void_p, C.c_int, C.POINTER(C.c_uint64)
    L.xq_version.restype = C.c_char_p
    L.xq_last_hip_error.restype = C.c_char_p
    L.xq_movegen_batch.argtypes = [vp, vp, i32, vp, vp, vp, vp, vp]
    L.xq_attack_map_batch.argtypes = [vp, i32, vp, vp]
    L.xq_find_king_batch.argtypes = [vp, i32, vp, vp]
    L.xq_encode_batch.argtypes = [vp, vp, i32, vp, vp]
    L.xq_material_batch.argtypes = [vp, i32, vp, vp]
    L.xq_apply_moves_batch.argtypes = [vp, vp, vp, vp, i32, vp, vp, vp]
    L.xq_game_over_batch.argtypes = [vp, vp, vp, vp, vp, i32, vp, vp]
    L.xq_game_over_batch_ex.argtypes = [vp, vp, vp, vp, vp, i32, C.POINTER(RulesOpts), vp, vp, vp]
    L.xq_engine_workspace_bytes.argtypes = [C.POINTER(EngineConfig)]
    L.xq_engine_workspace_bytes.restype = C.c_size_t
    L.xq_engine_init.argtypes = [C.POINTER(Engine), C.POINTER(EngineConfig), vp, C.c_size_t, vp, vp]
    L.xq_engine_workspace_bytes_leaves.argtypes = [C.POINTER(EngineConfig), i32]
    L.xq_engine_workspace_bytes_leaves.restype = C.c_size_t
    L.xq_engine_init_leaves.argtypes = [C.POINTER(Engine), C.POINTER(EngineConfig), i32, vp, C.c_size_t, vp, vp]
    L.xq_engine_workspace_bytes_ex.argtypes = [C.POINTER(EngineConfig), i32, C.c_uint]
    L.xq_engine_workspace_bytes_ex.restype = C.c_size_t
    L.xq_engine_init_ex.argtypes = [C.POINTER(Engine), C.POINTER(EngineConfig), i32, C.c_uint, vp, C.c_size_t, vp, vp]
    L.xq_engine_drop_reroots.argtypes = [C.POINTER(Engine), vp]
    L.xq_engine_workspace_bytes_cap.argtypes = [C.POINTER(EngineConfig), i32, C.c_uint, C.POINTER(PlayoutCap)]
    L.xq_engine_workspace_bytes_cap.restype = C.c_size_t
    L.xq_engine_init_cap.argtypes = [C.POINTER(Engine), C.POINTER(EngineConfig), i32, C.c_uint, C.POINTER(PlayoutCap), vp,
                                     C.c_size_t, vp, vp]
    L.xq_engine_workspace_bytes_fp.argtypes = [C.POINTER(EngineConfig), i32, C.c_uint, C.POINTER(PlayoutCap),
                                               C.POINTER(ForcedPlayouts)]
    L.xq_engine_workspace_bytes_fp.restype = C.c_size_t
    L.xq_engine_init_fp.argtypes = [C.POINTER(Engine), C.POINTER(EngineConfig), i32, C.c_uint, C.POINTER(PlayoutCap),
                                    C.POINTER(ForcedPlayouts), vp, C.c_size_t, vp, vp]
    L.xq_engine_workspace_bytes_gz.argtypes = [C.POINTER(EngineConfig), i32, C.c_uint, C.POINTER(PlayoutCap),
                                               C.POINTER(ForcedPlayouts), C.POINTER(Gumbel)]
    L.xq_engine_workspace_bytes_gz.restype = C.c_size_t
    L.xq_engine_init_gz.argtypes = [C.POINTER(Engine), C.POINTER(EngineConfig), i32, C.c_uint, C.POINTER(PlayoutCap),
                                    C.POINTER(ForcedPlayouts), C.POINTER(Gumbel), vp, C.c_size_t, vp, vp]
    L.xq_gumbel_considered_visits_host.argtypes = [i32, i32, vp]
    L.xq_engine_workspace_bytes_ar.argtypes = [C.POINTER(EngineConfig), i32, C.c_uint, C.POINTER(PlayoutCap),
                                               C.POINTER(ForcedPlayouts), C.POINTER(Gumbel), C.POINTER(ArenaOpts)]
    L.xq_engine_workspace_bytes_ar.restype = C.c_size_t
    L.xq_engine_init_ar.argtypes = [C.POINTER(Engine), C.POINTER(EngineConfig), i32, C.c_uint, C.POINTER(PlayoutCap),
                                    C.POINTER(ForcedPlayouts), C.POINTER(Gumbel), C.POINTER(ArenaOpts), vp, C.c_size_t, vp, vp]
    L.xq_engine_workspace_bytes_ru.argtypes = L.xq_engine_workspace_bytes_ar.argtypes + [C.POINTER(RulesOpts)]
    L.xq_engine_workspace_bytes_ru.restype = C.c_size_t
    L.xq_engine_init_ru.argtypes = L.xq_engine_init_ar.argtypes[:8] + [C.POINTER(RulesOpts)] + L.xq_engine_init_ar.argtypes[8:]
    L.xq_engine_workspace_bytes_sv.argtypes = L.xq_engine_workspace_bytes_ru.argtypes + [C.POINTER(SolverOpts)]
    L.xq_engine_workspace_bytes_sv.restype = C.c_size_t
    L.xq_engine_init_sv.argtypes = L.xq_engine_init_ru.argtypes[:9] + [C.POINTER(SolverOpts)] + L.xq_engine_init_ru.argtypes[9:]
    L.xq_engine_workspace_bytes_rs.argtypes = L.xq_engine_workspace_bytes_sv.argtypes + [C.POINTER(RootStatsOpts)]
    L.xq_engine_workspace_bytes_rs.restype = C.c_size_t
    L.xq_engine_init_rs.argtypes = L.xq_engine_init_sv.argtypes[:10] + [C.POINTER(RootStatsOpts)] + L.xq_engine_init_sv.argtypes[10:]
    L.xq_engine_workspace_bytes_em.argtypes = L.xq_engine_workspace_bytes_rs.argtypes + [C.POINTER(EvalMirrorOpts)]
    L.xq_engine_workspace_bytes_em.restype = C.c_size_t
    L.xq_engine_init_em.argtypes = L.xq_engine_init_rs.argtypes[:11] + [C.POINTER(EvalMirrorOpts)] + L.xq_engine_init_rs.argtypes[11:]
    L.xq_engine_workspace_bytes_gr.argtypes = L.xq_engine_workspace_bytes_em.argtypes + [C.POINTER(GameRecordsOpts)]
    L.xq_engine_workspace_bytes_gr.restype = C.c_size_t
    L.xq_engine_init_gr.argtypes = L.xq_engine_init_em.argtypes[:12] + [C.POINTER(GameRecordsOpts)] + L.xq_engine_init_em.argtypes[12:]
    L.xq_engine_workspace_bytes_sp.argtypes = L.xq_engine_workspace_bytes_gr.argtypes + [C.POINTER(StartPool)]
    L.xq_engine_workspace_bytes_sp.restype = C.c_size_t
    L.xq_engine_init_sp.argtypes = L.xq_engine_init_gr.argtypes[:13] + [C.POINTER(StartPool)] + L.xq_engine_init_gr.argtypes[13:]
    L.xq_engine_option_words_sp.argtypes = L.xq_engine_workspace_bytes_sp.argtypes + [C.POINTER(OptionWords)]
    L.xq_positions_check_batch.argtypes = [vp, vp, i32, vp, vp]
    L.xq_start_pool_draw_host.argtypes = [C.c_uint64, i32, i32, C.c_uint32, i32, C.c_double]
    L.xq_engine_start_indices.argtypes = [C.POINTER(Engine), C.POINTER(vp)]
    L.xq_engine_start_pool_stats_read.argtypes = [C.POINTER(Engine), C.POINTER(StartPoolStats), vp]
    L.xq_engine_settle.argtypes = [C.POINTER(Engine), vp, vp]
    L.xq_tb_adjudicate_batch.argtypes = [vp, i32, vp, C.c_int64, vp, vp, i32, C.POINTER(AdjudicateOpts), vp, vp, vp, vp]
    L.xq_engine_adjudicate.argtypes = [C.POINTER(Engine), vp, i32, vp, C.c_int64, C.POINTER(AdjudicateOpts), vp, vp]
    L.xq_resign_state_bytes.argtypes = [i32]
    L.xq_resign_state_bytes.restype = C.c_size_t
    L.xq_resign_exempt_host.argtypes = [C.c_uint64, i32, i32, C.c_uint32, C.c_double]
    L.xq_resign_scan_batch.argtypes = [vp, vp, vp, i32, i32, i32, C.c_double, vp, vp, vp, vp, vp]
    L.xq_engine_resign.argtypes = [C.POINTER(Engine), C.POINTER(ResignOpts), vp, vp, i32, vp, vp, vp]
    L.xq_engine_drain_games.argtypes = [C.POINTER(Engine), vp, i32, C.POINTER(C.c_int), vp]
    L.xq_engine_drain_games_device.argtypes = [C.POINTER(Engine), vp, i32, C.POINTER(C.c_int), vp]
    L.xq_engine_game_records_stats_read.argtypes = [C.POINTER(Engine), C.POINTER(GameRecordsStats), vp]
    L.xq_replay_games_batch.argtypes = [vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.xq_alphabeta_batch.argtypes = [vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.xq_mate_search_batch.argtypes = [vp, vp, i32, C.POINTER(MateOpts), vp, vp, vp, vp, vp, vp, vp, vp]
    L.xq_eval_mirror_bit_host.argtypes = [C.c_uint64, i32, i32, C.c_uint32, i32, i32, i32, i32]
    L.xq_mirror_action_host.argtypes = [i32]
    L.xq_mirror_requests_batch.argtypes = [vp, vp, vp, vp, i32, vp, vp, vp]
    L.xq_engine_read_root_states.argtypes = [C.POINTER(Engine), i32, vp, vp, vp]
    L.xq_engine_solver_stats_read.argtypes = [C.POINTER(Engine), C.POINTER(SolverStats), vp]
    L.xq_engine_arena_openings.argtypes = [C.POINTER(Engine), C.POINTER(vp), C.POINTER(vp)]
    L.xq_engine_compact_arena.argtypes = [C.POINTER(Engine), vp, vp]
    L.xq_engine_packed_arena.argtypes = [C.POINTER(Engine), C.POINTER(PackedBuffers)]
    L.xq_engine_expand_packed_arena.argtypes = [C.POINTER(Engine), vp, vp, vp, vp, vp]
    L.xq_engine_select.argtypes = [C.POINTER(Engine), vp, vp]
    L.xq_engine_expand.argtypes = [C.POINTER(Engine), vp, vp, i32, vp]
    L.xq_engine_stats_read.argtypes = [C.POINTER(Engine), C.POINTER(EngineStats), vp]
    L.xq_engine_drain.argtypes = [C.POINTER(Engine), vp, i32, C.POINTER(C.c_int), vp, i32, C.POINTER(C.c_int), vp]
    L.xq_engine_drain_device.argtypes = [C.POINTER(Engine), vp, i32, C.POINTER(C.c_int), vp, i32, C.POINTER(C.c_int), vp]
    L.xq_engine_set_position.argtypes = [C.POINTER(Engine), i32, vp, i32, i32, i32, vp, vp, vp]
    L.xq_engine_read_root.argtypes = [C.POINTER(Engine), i32, vp, vp, vp, vp, C.POINTER(C.c_int),
                                      C.POINTER(C.c_int32), C.POINTER(C.c_int32), vp]
    L.xq_bias_act.argtypes = [vp, vp, vp, C.c_longlong, i32, i32, vp]
    L.xq_heads_1x1.argtypes = [vp, vp, vp, vp, vp, C.c_longlong, i32, vp]
    L.xq_stem_conv.argtypes = [vp, vp, vp, vp, i32, i32, vp]
    L.xq_samples_to_batch.argtypes = [vp, vp, vp, i32, C.c_double, vp, vp, vp, vp]
    L.xq_samples_to_batch_ex.argtypes = [vp, vp, vp, i32, C.c_double, C.POINTER(BatchOpts), vp, vp, vp, vp]
    L.xq_wino_weight_bytes.argtypes = [i32]
    L.xq_wino_weight_bytes.restype = C.c_size_t
    L.xq_wino_conv3x3.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, vp]
    L.xq_wino_transform_filters.argtypes = [vp, vp, i32, i32, vp]
    L.xq_wino_wgrad_scratch_bytes.argtypes = [i32, i32]
    L.xq_wino_wgrad_scratch_bytes.restype = C.c_size_t
    L.xq_wino_wgrad.argtypes = [vp, vp, vp, vp, i32, i32, vp]
    L.xq_bn_scratch_bytes.argtypes = [i32]
    L.xq_bn_scratch_bytes.restype = C.c_size_t
    L.xq_bn_train_forward.argtypes = [vp, vp, vp, vp, vp, vp, C.c_float, C.c_float, C.c_longlong, i32, i32, vp, vp, vp, vp, vp, vp]
    L.xq_bn_train_backward.argtypes = [vp, vp, vp, vp, vp, vp, C.c_longlong, i32, i32, vp, vp, vp, vp, vp, vp]
    L.xq_bn_sync_sums_count.argtypes = [i32]
    L.xq_bn_sync_sums_count.restype = C.c_size_t
    L.xq_bn_sync_forward_stats.argtypes = [vp, C.c_longlong, i32, vp, vp, vp]
    L.xq_bn_sync_forward_apply.argtypes = [vp, vp, vp, vp, vp, vp, C.c_float, C.c_float, C.c_longlong, i32, i32, vp, vp, vp, vp, vp, vp]
    L.xq_bn_sync_backward_stats.argtypes = [vp, vp, vp, vp, vp, C.c_longlong, i32, i32, vp, vp, vp, vp, vp]
    L.xq_bn_sync_backward_apply.argtypes = [vp, vp, vp, vp, vp, vp, C.c_longlong, i32, i32, vp, vp, vp, vp]
    L.xq_wino_weight_bytes_bf16.argtypes = [i32]
    L.xq_wino_weight_bytes_bf16.restype = C.c_size_t
    L.xq_wino_conv3x3_bf16.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, vp]
    L.xq_policy_head_legal.argtypes = [vp, vp, vp, vp, vp, i32, vp, vp]
    L.xq_value_head.argtypes = [vp, vp, vp, vp, vp, i32, vp, vp]
    L.xq_engine_requests.argtypes = [C.POINTER(Engine), C.POINTER(vp), C.POINTER(vp)]
    L.xq_engine_expand_legal.argtypes = [C.POINTER(Engine), vp, vp, vp]
    L.xq_engine_compact.argtypes = [C.POINTER(Engine), vp, vp]
    L.xq_engine_packed.argtypes = [C.POINTER(Engine), C.POINTER(PackedBuffers)]
    L.xq_engine_expand_packed.argtypes = [C.POINTER(Engine), vp, vp, vp]
    L.xq_stem_conv_live.argtypes = [vp, vp, vp, vp, i32, vp, i32, vp]
    L.xq_heads_1x1_live.argtypes = [vp, vp, vp, vp, vp, C.c_longlong, vp, i32, vp]
    L.xq_wino_conv3x3_live.argtypes = [vp, vp, vp, vp, vp, i32, vp, i32, i32, vp]
    L.xq_wino_conv3x3_bf16_live.argtypes = [vp, vp, vp, vp, vp, i32, vp, i32, i32, vp]
    L.xq_policy_head_legal_live.argtypes = [vp, vp, vp, vp, vp, i32, vp, vp, vp]
    L.xq_value_head_live.argtypes = [vp, vp, vp, vp, vp, i32, vp, vp, vp]
    L.xq_evcache_bytes.argtypes = [i32, i32]
    L.xq_evcache_bytes.restype = C.c_size_t
    L.xq_evcache_init.argtypes = [C.POINTER(EvCache), i32, i32, vp, C.c_size_t, vp]
    L.xq_evcache_hit_flags.argtypes = [C.POINTER(EvCache), C.POINTER(vp)]
    L.xq_evcache_probe.argtypes = [C.POINTER(EvCache), C.POINTER(Engine), vp, vp]
    L.xq_engine_compact_misses.argtypes = [C.POINTER(Engine), vp, vp, vp]
    L.xq_evcache_commit.argtypes = [C.POINTER(EvCache), C.POINTER(Engine), vp, vp, vp]
    L.xq_evcache_invalidate.argtypes = [C.POINTER(EvCache), vp]
    L.xq_evcache_stats_read.argtypes = [C.POINTER(EvCache), C.POINTER(EvCacheStats), vp]
    L.xq_evcache_key_host.argtypes = [vp, vp]
    L.xq_evdedup_bytes.argtypes = [i32]
    L.xq_evdedup_bytes.restype = C.c_size_t
    L.xq_evdedup_init.argtypes = [C.POINTER(EvDedup), i32, vp, C.c_size_t, vp]
    L.xq_engine_compact_unique.argtypes = [C.POINTER(EvDedup), C.POINTER(Engine), vp, vp]
    L.xq_engine_expand_dedup.argtypes = [C.POINTER(EvDedup), C.POINTER(Engine), vp, vp, vp]
    L.xq_evdedup_stats_read.argtypes = [C.POINTER(EvDedup), C.POINTER(EvDedupStats), vp]
    L.xq_evdedup_bucket_host.argtypes = [vp, i32]
    L.xq_dedup_rows_batch.argtypes = [vp, vp, vp, i32, C.POINTER(EvDedup), vp, vp, vp, vp]
    L.xq_samples_to_requests.argtypes = [vp, vp, i32, vp, vp, vp, vp]
    L.xq_score_samples.argtypes = [vp, vp, i32, vp, vp, C.POINTER(ScoreOpts), vp, vp]
    L.xq_surprise_counts.argtypes = [vp, i32, C.POINTER(SurpriseOpts), vp, vp, vp]
    L.xq_surprise_count_host.argtypes = [C.c_float, i32, C.c_uint64, C.c_uint64, C.c_double, C.c_uint64, C.c_uint32, C.c_uint32,
                                         C.c_uint32, C.c_uint32]
    L.xq_position_keys.argtypes = [vp, vp, i32, i32, vp, vp, vp]
    L.xq_position_key_host.argtypes = [vp, C.c_int8, i32, vp]
    L.xq_position_key_host.restype = C.c_uint64
    L.xq_position_group_heads.argtypes = [vp, vp, vp, vp, vp, i32, vp, vp]
    L.xq_groups_to_batch.argtypes = [vp, vp, vp, vp, i32, vp, vp, i32, C.c_double, C.POINTER(BatchOpts), vp, vp, vp, vp]
    L.xq_records_sample_counts.argtypes = [vp, vp, i32, C.POINTER(SuperviseOpts), vp, vp]
    L.xq_records_to_samples.argtypes = [vp, vp, vp, i32, C.POINTER(SuperviseOpts), vp, vp, vp]
    L.xq_tb_entries.argtypes = [vp, i32]
    L.xq_tb_entries.restype = C.c_int64
    L.xq_tb_init.argtypes = [vp, i32, vp, vp]
    L.xq_tb_pass.argtypes = [vp, i32, vp, i32, vp, vp]
    L.xq_tb_probe_batch.argtypes = [vp, i32, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp]
    L.xq_tb_play_batch.argtypes = [vp, i32, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp]
    L.xq_tb_samples.argtypes = [vp, i32, vp, vp, i32, C.POINTER(TbSampleOpts), vp, vp, vp]
    _lib = L
    return L


EXPORTS = ["xq_version", "xq_last_hip_error", "xq_movegen_batch", "xq_attack_map_batch", "xq_find_king_batch",
           "xq_encode_batch", "xq_material_batch", "xq_apply_moves_batch", "xq_game_over_batch",
           "xq_engine_workspace_bytes", "xq_engine_init", "xq_engine_select", "xq_engine_expand",
           "xq_engine_stats_read", "xq_engine_drain", "xq_engine_set_position", "xq_engine_read_root",
           "xq_bias_act", "xq_stem_conv", "xq_heads_1x1", "xq_wino_weight_bytes", "xq_wino_conv3x3", "xq_samples_to_batch",
           "xq_policy_head_legal", "xq_value_head", "xq_engine_requests", "xq_engine_expand_legal", "xq_engine_drain_device",
           "xq_wino_weight_bytes_bf16", "xq_wino_conv3x3_bf16", "xq_wino_transform_filters",
           "xq_bn_scratch_bytes", "xq_bn_train_forward", "xq_bn_train_backward", "xq_wino_wgrad_scratch_bytes", "xq_wino_wgrad",
           "xq_engine_compact", "xq_engine_packed", "xq_engine_expand_packed", "xq_stem_conv_live", "xq_heads_1x1_live",
           "xq_wino_conv3x3_live", "xq_wino_conv3x3_bf16_live", "xq_policy_head_legal_live", "xq_value_head_live",
           "xq_bn_sync_sums_count", "xq_bn_sync_forward_stats", "xq_bn_sync_forward_apply", "xq_bn_sync_backward_stats",
           "xq_bn_sync_backward_apply", "xq_evcache_bytes", "xq_evcache_init", "xq_evcache_hit_flags", "xq_evcache_probe",
           "xq_engine_compact_misses", "xq_evcache_commit", "xq_evcache_invalidate", "xq_evcache_stats_read",
           "xq_evcache_key_host", "xq_engine_workspace_bytes_leaves", "xq_engine_init_leaves", "xq_engine_workspace_bytes_ex",
           "xq_engine_init_ex", "xq_engine_drop_reroots", "xq_engine_workspace_bytes_cap", "xq_engine_init_cap",
           "xq_engine_workspace_bytes_fp", "xq_engine_init_fp", "xq_engine_workspace_bytes_gz", "xq_engine_init_gz",
           "xq_gumbel_considered_visits_host", "xq_engine_workspace_bytes_ar", "xq_engine_init_ar", "xq_engine_arena_openings",
           "xq_engine_compact_arena", "xq_engine_packed_arena", "xq_engine_expand_packed_arena",
           "xq_engine_workspace_bytes_ru", "xq_engine_init_ru", "xq_game_over_batch_ex",
           "xq_engine_workspace_bytes_sv", "xq_engine_init_sv", "xq_engine_read_root_states", "xq_engine_solver_stats_read",
           "xq_engine_workspace_bytes_rs", "xq_engine_init_rs", "xq_samples_to_batch_ex",
           "xq_engine_workspace_bytes_em", "xq_engine_init_em", "xq_eval_mirror_bit_host", "xq_mirror_action_host",
           "xq_mirror_requests_batch", "xq_engine_workspace_bytes_gr", "xq_engine_init_gr", "xq_engine_drain_games",
           "xq_engine_drain_games_device", "xq_engine_game_records_stats_read", "xq_replay_games_batch",
           "xq_samples_to_requests", "xq_score_samples", "xq_surprise_counts", "xq_surprise_count_host",
           "xq_position_keys", "xq_position_key_host", "xq_position_group_heads", "xq_groups_to_batch",
           "xq_alphabeta_batch", "xq_records_sample_counts", "xq_records_to_samples", "xq_mate_search_batch",
           "xq_tb_entries", "xq_tb_init", "xq_tb_pass", "xq_tb_probe_batch", "xq_tb_play_batch", "xq_tb_samples",
           "xq_positions_check_batch", "xq_engine_workspace_bytes_sp", "xq_engine_init_sp", "xq_start_pool_draw_host",
           "xq_engine_start_indices", "xq_engine_start_pool_stats_read", "xq_engine_option_words_sp", "xq_evdedup_bytes", "xq_evdedup_init",
           "xq_engine_compact_unique", "xq_engine_expand_dedup", "xq_evdedup_stats_read", "xq_evdedup_bucket_host",
           "xq_dedup_rows_batch", "xq_engine_settle", "xq_tb_adjudicate_batch", "xq_engine_adjudicate",
           "xq_resign_state_bytes", "xq_resign_exempt_host", "xq_resign_scan_batch", "xq_engine_resign"]


def check(rc: int, what: str):
    if rc != 0:
        raise XqError(f"{what} failed: code {rc} ({lib().xq_last_hip_error().decode()})")


def stream_ptr(device=None) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def _dev(t: torch.Tensor) -> int:
    if not t.is_cuda or not t.is_contiguous():
        raise XqError("device-resident contiguous tensor required")
    return t.data_ptr()


# ---- B1 adapters (tensors in, tensors out; all on the current stream) -------------------------------------

def movegen(boards: torch.Tensor, side: torch.Tensor):
    """boards int8[n,90] (or [n,10,9]), side int8[n] -> (moves u16-as-int16 [n,128], counts int16[n],
    in_check uint8[n], status uint8[n])."""
    n = boards.shape[0]
    dev = boards.device
    moves = torch.zeros((n, MAXM), dtype=torch.int16, device=dev)
    counts = torch.zeros(n, dtype=torch.int16, device=dev)
    chk = torch.zeros(n, dtype=torch.uint8, device=dev)
    status = torch.zeros(n, dtype=torch.uint8, device=dev)
    if n:
        check(lib().xq_movegen_batch(_dev(boards), _dev(side), n, _dev(moves), _dev(counts), _dev(chk), _dev(status),
                                     stream_ptr(dev)), "xq_movegen_batch")
    return moves, counts, chk, status


def attack_map(boards: torch.Tensor) -> torch.Tensor:
    n = boards.shape[0]
    out = torch.zeros((n, 2, 90), dtype=torch.uint8, device=boards.device)
    if n:
        check(lib().xq_attack_map_batch(_dev(boards), n, _dev(out), stream_ptr(boards.device)), "xq_attack_map_batch")
    return out


def find_king(boards: torch.Tensor) -> torch.Tensor:
    n = boards.shape[0]
    out = torch.zeros((n, 2), dtype=torch.int16, device=boards.device)
    if n:
        check(lib().xq_find_king_batch(_dev(boards), n, _dev(out), stream_ptr(boards.device)), "xq_find_king_batch")
    return out


def encode(boards: torch.Tensor, side: torch.Tensor) -> torch.Tensor:
    n = boards.shape[0]
    out = torch.empty((n, 15, 10, 9), dtype=torch.float32, device=boards.device)
    if n:
        check(lib().xq_encode_batch(_dev(boards), _dev(side), n, _dev(out), stream_ptr(boards.device)), "xq_encode_batch")
    return out


def material(boards: torch.Tensor) -> torch.Tensor:
    n = boards.shape[0]
    out = torch.zeros((n, 2), dtype=torch.int32, device=boards.device)
    if n:
        check(lib().xq_material_batch(_dev(boards), n, _dev(out), stream_ptr(boards.device)), "xq_material_batch")
    return out


def apply_moves(boards, side, parent, action):
    """parent int32[m] (indices into boards), action int16[m] (u16 ids) -> (child boards int8[m,90], side int8[m])."""
    m = parent.shape[0]
    ob = torch.empty((m, 90), dtype=torch.int8, device=boards.device)
    os_ = torch.empty(m, dtype=torch.int8, device=boards.device)
    if m:
        check(lib().xq_apply_moves_batch(_dev(boards), _dev(side), _dev(parent), _dev(action), m, _dev(ob), _dev(os_),
                                         stream_ptr(boards.device)), "xq_apply_moves_batch")
    return ob, os_


def game_over(boards, side, move_count, no_capture, hist):
    n = boards.shape[0]
    out = torch.zeros((n, 2), dtype=torch.int8, device=boards.device)
    if n:
        check(lib().xq_game_over_batch(_dev(boards), _dev(side), _dev(move_count), _dev(no_capture), _dev(hist), n,
                                       _dev(out), stream_ptr(boards.device)), "xq_game_over_batch")
    return out


def game_over_batch(boards, side, move_count, no_capture, hist, perpetual_check: bool = False, return_kind: bool = False):
    """`game_over` through xq_game_over_batch_ex: `perpetual_check` turns the perpetual-check rule on (xq_rules_opts; off: NULL
    rules, `game_over`'s bytes); `return_kind` adds uint8[n], what ended each game (index into OVER_KINDS)."""
    n = boards.shape[0]
    out = torch.zeros((n, 2), dtype=torch.int8, device=boards.device)
    kind = torch.zeros(n, dtype=torch.uint8, device=boards.device) if return_kind else None
    rules = RulesOpts(1) if perpetual_check else None
    if n:
        check(lib().xq_game_over_batch_ex(_dev(boards), _dev(side), _dev(move_count), _dev(no_capture), _dev(hist), n,
                                          None if rules is None else C.byref(rules), _dev(out),
                                          None if kind is None else _dev(kind), stream_ptr(boards.device)),
              "xq_game_over_batch_ex")
    return (out, kind) if return_kind else out


def replay_games(records: torch.Tensor, stop_ply=None, perpetual_check: bool = False):
    """Replay of game records on the device (xq_replay_games_batch): records uint8[n, 1024] on the GPU, stop_ply int32[n] there or
    None (all moves) -> dict of tensors: status int32[n], board int8[n,90], side int8[n], move_count / no_capture int32[n],
    hist12 int8[n,12,90] (oldest first, set_position's layout), over_kind / winner int8[n]."""
    if records.dtype != torch.uint8 or records.dim() != 2 or records.shape[1] != RECORD_BYTES:
        raise XqError(f"replay_games: records must be uint8[n, {RECORD_BYTES}], got {records.dtype} {tuple(records.shape)}")
    n, dev = records.shape[0], records.device
    if stop_ply is not None and (stop_ply.dtype != torch.int32 or tuple(stop_ply.shape) != (n,)):
        raise XqError(f"replay_games: stop_ply must be int32[{n}]")
    out = {"status": torch.zeros(n, dtype=torch.int32, device=dev), "board": torch.zeros((n, 90), dtype=torch.int8, device=dev),
           "side": torch.zeros(n, dtype=torch.int8, device=dev), "move_count": torch.zeros(n, dtype=torch.int32, device=dev),
           "no_capture": torch.zeros(n, dtype=torch.int32, device=dev),
           "hist12": torch.zeros((n, 12, 90), dtype=torch.int8, device=dev),
           "over_kind": torch.zeros(n, dtype=torch.int8, device=dev), "winner": torch.zeros(n, dtype=torch.int8, device=dev)}
    if n:
        check(lib().xq_replay_games_batch(_dev(records), None if stop_ply is None else _dev(stop_ply), n, 1 if perpetual_check else 0,
                                          _dev(out["board"]), _dev(out["side"]), _dev(out["move_count"]), _dev(out["no_capture"]),
                                          _dev(out["hist12"]), _dev(out["status"]), _dev(out["over_kind"]), _dev(out["winner"]),
                                          stream_ptr(dev)), "xq_replay_games_batch")
    return out


def records_to_samples(records, movers: int = 0, per_record_movers=None, skip_opening: bool = True, skip_draws: bool = False,
                       device="cuda"):
    """Game records as training samples (xq_records_sample_counts, one torch.cumsum, xq_records_to_samples): records = host
    records (GAME_RECORD_DTYPE; copied to `device`) or a uint8[n, 1024] tensor on the GPU; movers 0 every ply, 1 the winner's
    plies, 2 red's, 3 black's, or per_record_movers = one such value per record (anything numpy turns into uint8[n], or a uint8
    device tensor); skip_opening leaves out the plies before record.opening_plies, skip_draws the drawn games -> dict of device
    tensors: samples uint8[total, 640] (the rows of record i are offsets[i] .. offsets[i + 1], in ply order), offsets
    int32[n + 1], status int32[n] (0 whole; k > 0: ply k - 1 is illegal, the rows from it on are zero; -1 malformed).  One host
    synchronisation, to read the total."""
    if isinstance(records, torch.Tensor):
        rec = records
    else:
        import numpy as np
        host = np.ascontiguousarray(records)
        if host.dtype != GAME_RECORD_DTYPE:
            raise XqError(f"records_to_samples: host records must be GAME_RECORD_DTYPE, got {host.dtype}")
        rec = torch.from_numpy(host.reshape(-1).view(np.uint8).reshape(-1, RECORD_BYTES).copy()).to(device)
    if rec.dtype != torch.uint8 or rec.dim() != 2 or rec.shape[1] != RECORD_BYTES:
        raise XqError(f"records_to_samples: records must be uint8[n, {RECORD_BYTES}], got {rec.dtype} {tuple(rec.shape)}")
    n, dev = rec.shape[0], rec.device
    if isinstance(movers, bool) or int(movers) != movers or not 0 <= int(movers) <= 3:
        raise XqError(f"records_to_samples: movers must be 0, 1, 2 or 3, got {movers!r}")
    opts = SuperviseOpts(int(movers), 1 if skip_opening else 0, 1 if skip_draws else 0, 0)
    per = None
    if per_record_movers is not None:
        if isinstance(per_record_movers, torch.Tensor):
            per = per_record_movers.to(dev).contiguous()
        else:
            import numpy as np
            per = torch.from_numpy(np.ascontiguousarray(per_record_movers, dtype=np.uint8)).to(dev)
        if per.dtype != torch.uint8 or tuple(per.shape) != (n,):
            raise XqError(f"records_to_samples: per_record_movers must be uint8[{n}], got {per.dtype} {tuple(per.shape)}")
    offsets = torch.zeros(n + 1, dtype=torch.int32, device=dev)
    status = torch.zeros(n, dtype=torch.int32, device=dev)
    if n == 0:
        return {"samples": torch.zeros((0, SAMPLE_BYTES), dtype=torch.uint8, device=dev), "offsets": offsets, "status": status}
    counts = torch.zeros(n, dtype=torch.int32, device=dev)
    p_per = None if per is None else _dev(per)
    check(lib().xq_records_sample_counts(_dev(rec), p_per, n, C.byref(opts), _dev(counts), stream_ptr(dev)),
          "xq_records_sample_counts")
    running = torch.cumsum(counts, 0, dtype=torch.int64)
    total = int(running[n - 1].item())
    if total >= 2 ** 31:
        raise XqError(f"records_to_samples: {total} rows do not fit the int32 offsets of xq_records_to_samples; convert in parts")
    offsets[1:] = running.to(torch.int32)
    rows = torch.empty((max(total, 1), SAMPLE_BYTES), dtype=torch.uint8, device=dev)
    check(lib().xq_records_to_samples(_dev(rec), p_per, _dev(offsets), n, C.byref(opts), _dev(rows), _dev(status), stream_ptr(dev)),
          "xq_records_to_samples")
    return {"samples": rows[:total], "offsets": offsets, "status": status}


def _positions_arg(boards, side, what: str):
    if boards.dtype != torch.int8 or boards.numel() != len(boards) * 90 or side.dtype != torch.int8 or side.shape != boards.shape[:1]:
        raise XqError(f"{what}: boards must be int8[n, 90] and side int8[n], got {tuple(boards.shape)} and {tuple(side.shape)}")
    return len(boards), boards.device


def positions_check(boards: torch.Tensor, side: torch.Tensor) -> torch.Tensor:
    """Is each board a position the rules code can safely run on (xq_positions_check_batch)?  boards int8[n,90] (or [n,10,9]) and
    side int8[n] on the GPU -> uint8[n] of bits: 1 a square outside -7..7 or a side outside {1, -1}; 2 not exactly one king per
    colour, or a king outside its palace; 4 a piece where it can never stand, or more of a kind than a set has; 8 the side not to
    move is in check; 16 the side to move has no legal move.  With bit 1 or 2 the later bits stay 0.  POSITION_FATAL (15) refuses a
    position; POSITION_NO_MOVE (16) alone is a game that is over at ply 0."""
    n, dev = _positions_arg(boards, side, "positions_check")
    status = torch.zeros(n, dtype=torch.uint8, device=dev)
    if n:
        check(lib().xq_positions_check_batch(_dev(boards), _dev(side), n, _dev(status), stream_ptr(dev)), "xq_positions_check_batch")
    return status


def start_pool_index(seed: int, rank: int, slot: int, game_seq: int, n: int, prob: float) -> int:
    """The start-position pool's draw on the host (xq_start_pool_draw_host, the device's own code; no GPU needed): the pool entry
    the game `game_seq` of `slot` starts from, or -1 for the initial position."""
    if n < 1 or not 0.0 < float(prob) <= 1.0:
        raise XqError(f"start_pool_index: n >= 1 and prob in (0, 1] required, got {n}, {prob}")
    if min(int(rank), int(slot), int(game_seq)) < 0:
        raise XqError(f"start_pool_index: rank, slot and game_seq must not be negative, got {rank}, {slot}, {game_seq}")
    return int(lib().xq_start_pool_draw_host(int(seed) & (2 ** 64 - 1), int(rank), int(slot), int(game_seq), int(n), float(prob)))


def alphabeta_batch(boards: torch.Tensor, side: torch.Tensor, depth: int, draws=None):
    """The fixed alpha-beta opponent (xq_alphabeta_batch): boards int8[n,90] (or [n,10,9]) and side int8[n] on the GPU, 0 <= depth
    <= AB_MAX_DEPTH, draws None (the first best move) or one uint32 per position (an int32 / int64 device tensor, or anything
    numpy turns into uint32) -> dict of device tensors: moves (u16-as-int16 [n,128], as `movegen`), counts int16[n], scores
    int32[n,128] (the exact minimax score of every root move, AB_UNSCORED past the count), nodes int32[n,128], best_action
    (u16-as-int16 [n]; AB_NO_MOVE reads -1), best_score int32[n], status uint8[n] (0 fine, 1 capacity, 2 a king is missing)."""
    if not 0 <= int(depth) <= AB_MAX_DEPTH:
        raise XqError(f"alphabeta_batch: depth must be in [0, {AB_MAX_DEPTH}], got {depth}")
    n, dev = _positions_arg(boards, side, "alphabeta_batch")
    d = None
    if draws is not None:
        if isinstance(draws, torch.Tensor):
            d = (draws.to(dev).to(torch.int64) & 0xFFFFFFFF)
        else:
            import numpy as np
            d = torch.from_numpy(np.asarray(draws, dtype=np.uint64).astype(np.int64) & 0xFFFFFFFF).to(dev)
        d = torch.where(d >= 2 ** 31, d - 2 ** 32, d).to(torch.int32).contiguous()      # the uint32's bits
        if tuple(d.shape) != (n,):
            raise XqError(f"alphabeta_batch: draws must hold one value per position ({n}), got {tuple(d.shape)}")
    out = {"moves": torch.zeros((n, MAXM), dtype=torch.int16, device=dev), "counts": torch.zeros(n, dtype=torch.int16, device=dev),
           "scores": torch.zeros((n, MAXM), dtype=torch.int32, device=dev), "nodes": torch.zeros((n, MAXM), dtype=torch.int32, device=dev),
           "best_action": torch.zeros(n, dtype=torch.int16, device=dev), "best_score": torch.zeros(n, dtype=torch.int32, device=dev),
           "status": torch.zeros(n, dtype=torch.uint8, device=dev)}
    if n:
        check(lib().xq_alphabeta_batch(_dev(boards), _dev(side), n, int(depth), None if d is None else _dev(d), _dev(out["moves"]),
                                       _dev(out["counts"]), _dev(out["scores"]), _dev(out["nodes"]), _dev(out["best_action"]),
                                       _dev(out["best_score"]), _dev(out["status"]), stream_ptr(dev)), "xq_alphabeta_batch")
    return out


def mate_search_batch(boards: torch.Tensor, side: torch.Tensor, max_moves: int, checks_only: bool = True, node_limit=None):
    """The forced-mate search (xq_mate_search_batch): boards int8[n,90] (or [n,10,9]) and side int8[n] on the GPU, the side to move
    attacks; 1 <= max_moves <= MATE_MAX_MOVES, checks_only restricts the attacker to checking moves, node_limit (None:
    MATE_DEFAULT_NODE_LIMIT) bounds the visits per root move -> dict of device tensors: moves (u16-as-int16 [n,128], as
    `movegen`), counts int16[n], mate_in uint8[n,128] (1..max_moves: the root move forces mate in that many moves; 0 none;
    MATE_UNKNOWN cut by the limit), nodes int32[n,128] (the uint32's bits), best_action (u16-as-int16 [n]; MATE_NO_MOVE reads
    -1), best_mate_in uint8[n], status uint8[n] (0 fine, 1 capacity, 2 a king is missing, +4 some root move was cut)."""
    if isinstance(max_moves, bool) or int(max_moves) != max_moves or not 1 <= int(max_moves) <= MATE_MAX_MOVES:
        raise XqError(f"mate_search_batch: max_moves must be an integer in [1, {MATE_MAX_MOVES}], got {max_moves!r}")
    if checks_only not in (True, False, 0, 1):
        raise XqError(f"mate_search_batch: checks_only must be a bool, got {checks_only!r}")
    if node_limit is None:
        node_limit = MATE_DEFAULT_NODE_LIMIT
    if isinstance(node_limit, bool) or int(node_limit) != node_limit or not 1 <= int(node_limit) < 2 ** 32:
        raise XqError(f"mate_search_batch: node_limit must be an integer in [1, 2^32), got {node_limit!r}")
    n, dev = _positions_arg(boards, side, "mate_search_batch")
    opts = MateOpts(int(max_moves), 1 if checks_only else 0, int(node_limit), 0)
    out = {"moves": torch.zeros((n, MAXM), dtype=torch.int16, device=dev), "counts": torch.zeros(n, dtype=torch.int16, device=dev),
           "mate_in": torch.zeros((n, MAXM), dtype=torch.uint8, device=dev),
           "nodes": torch.zeros((n, MAXM), dtype=torch.int32, device=dev),
           "best_action": torch.zeros(n, dtype=torch.int16, device=dev), "best_mate_in": torch.zeros(n, dtype=torch.uint8, device=dev),
           "status": torch.zeros(n, dtype=torch.uint8, device=dev)}
    if n:
        check(lib().xq_mate_search_batch(_dev(boards), _dev(side), n, C.byref(opts), _dev(out["moves"]), _dev(out["counts"]),
                                         _dev(out["mate_in"]), _dev(out["nodes"]), _dev(out["best_action"]),
                                         _dev(out["best_mate_in"]), _dev(out["status"]), stream_ptr(dev)), "xq_mate_search_batch")
    return out


# ---- endgame tablebases (xq_tb_*; endgame.py holds the numpy reference of the layout and the Tablebase class) ----------------

_TB_LETTERS = {"A": 2, "B": 3, "E": 3, "N": 4, "H": 4, "R": 5, "C": 6, "P": 7}


def tb_signature(signature, what: str = "tb_signature"):
    """A signature -> its signed piece codes (a tuple).  A string of FEN letters as `sample_format.board_to_fen` writes them (A B
    N R C P, upper case for red, lower case for black; E and H are read too), or a sequence of signed codes (2 advisor, 3
    elephant, 4 knight, 5 rook, 6 cannon, 7 pawn).  Both kings are implicit.  Refused: an unknown letter or code, more than
    TB_MAX_PIECES pieces."""
    if isinstance(signature, str):
        bad = [ch for ch in signature if ch.upper() not in _TB_LETTERS]
        if bad:
            raise XqError(f"{what}: signature {signature!r} holds {bad[0]!r}; the letters are A B N R C P (E, H), lower case for black")
        codes = tuple(_TB_LETTERS[ch.upper()] * (1 if ch.isupper() else -1) for ch in signature)
    else:
        try:
            codes = tuple(int(c) for c in signature)
        except (TypeError, ValueError):
            raise XqError(f"{what}: signature must be a string of piece letters or a sequence of piece codes, got {signature!r}")
        if any(isinstance(c, bool) or int(c) != c for c in signature) or any(not 2 <= abs(c) <= 7 for c in codes):
            raise XqError(f"{what}: signature codes must be integers with 2 <= |code| <= 7, got {signature!r}")
    if len(codes) > TB_MAX_PIECES:
        raise XqError(f"{what}: signature {signature!r} holds {len(codes)} pieces, at most {TB_MAX_PIECES} fit")
    return codes


def _tb_pieces(codes):
    return (C.c_int8 * max(len(codes), 1))(*codes), len(codes)


def tb_entries(signature) -> int:
    """xq_tb_entries: the entry count of a signature's table, on the host (no GPU needed).  A signature beyond TB_MAX_ENTRIES
    is refused."""
    codes = tb_signature(signature, "tb_entries")
    arr, P = _tb_pieces(codes)
    n = int(lib().xq_tb_entries(arr, P))
    if n <= 0:
        raise XqError(f"tb_entries: signature {signature!r} is beyond {TB_MAX_ENTRIES} entries")
    return n


def _tb_table_arg(signature, table, what: str):
    codes = tb_signature(signature, what)
    entries = tb_entries(signature)
    if not isinstance(table, torch.Tensor) or table.dtype != torch.int16 or tuple(table.shape) != (entries,):
        got = (table.dtype, tuple(table.shape)) if isinstance(table, torch.Tensor) else type(table).__name__
        raise XqError(f"{what}: table must be an int16 tensor of {entries} entries for signature {signature!r}, got {got}")
    return codes, entries


def tb_init(signature, table: torch.Tensor) -> torch.Tensor:
    """Pass 0 (xq_tb_init) over `table`, an int16 device tensor of tb_entries(signature) words: TB_INVALID, -1 (no legal move) or
    0 per entry.  On the current stream; does not synchronise.  -> table."""
    codes, _ = _tb_table_arg(signature, table, "tb_init")
    arr, P = _tb_pieces(codes)
    check(lib().xq_tb_init(arr, P, _dev(table), stream_ptr(table.device)), "xq_tb_init")
    return table


def tb_pass(signature, table: torch.Tensor, k: int, changed: torch.Tensor) -> torch.Tensor:
    """Pass k >= 1 (xq_tb_pass), in place on `table`; `changed` is an int32[1] device tensor that a deciding wavefront sets to 1
    (the caller zeroes it before and reads it after).  On the current stream; does not synchronise.  -> changed."""
    codes, _ = _tb_table_arg(signature, table, "tb_pass")
    if isinstance(k, bool) or int(k) != k or not 1 <= int(k) <= TB_MAX_PASSES:
        raise XqError(f"tb_pass: k must be an integer in [1, {TB_MAX_PASSES}], got {k!r}")
    if not isinstance(changed, torch.Tensor) or changed.dtype != torch.int32 or changed.numel() != 1 or changed.device != table.device:
        raise XqError("tb_pass: changed must be an int32 tensor of one word on the table's device")
    arr, P = _tb_pieces(codes)
    check(lib().xq_tb_pass(arr, P, _dev(table), int(k), _dev(changed), stream_ptr(table.device)), "xq_tb_pass")
    return changed


def tb_generate(signature, device="cuda", max_passes=None):
    """The whole table of a signature -> (table int16 device tensor, passes).  tb_init, then tb_pass for k = 1, 2, ...; the flag is
    read after each pass and the loop stops at the first pass that decided nothing (or at max_passes); `passes` is that pass's
    number.  THIS CALL SYNCHRONISES: it reads the flag on the host once per pass."""
    codes = tb_signature(signature, "tb_generate")
    entries = tb_entries(signature)
    if max_passes is None:
        max_passes = TB_MAX_PASSES
    if isinstance(max_passes, bool) or int(max_passes) != max_passes or not 1 <= int(max_passes) <= TB_MAX_PASSES:
        raise XqError(f"tb_generate: max_passes must be an integer in [1, {TB_MAX_PASSES}], got {max_passes!r}")
    dev = torch.device(device)
    with torch.cuda.device(dev):
        table = torch.empty(entries, dtype=torch.int16, device=dev)
        changed = torch.zeros(1, dtype=torch.int32, device=dev)
        tb_init(codes, table)
        k = 0
        while k < int(max_passes):
            k += 1
            changed.zero_()
            tb_pass(codes, table, k, changed)
            if int(changed.item()) == 0:
                break
    return table, k


def tb_probe_batch(signature, table: torch.Tensor, boards: torch.Tensor, side: torch.Tensor, move_values: bool = True):
    """The probe (xq_tb_probe_batch): boards int8[n,90] (or [n,10,9]) and side int8[n] on the table's device -> dict of device
    tensors: value int16[n] (0 draw, +p a win in p plies, -(p + 1) a loss in p plies), moves (u16-as-int16 [n,128], as `movegen`),
    counts int16[n], move_value int16[n,128] (what the side to move gets by each root move; absent with move_values=False),
    best_action (u16-as-int16 [n]; TB_NO_MOVE reads -1), status uint8[n] (+1 not in this table, +2 a king is missing, +4 the
    entry is TB_INVALID; with any bit the value is 0, the count 0 and the action TB_NO_MOVE)."""
    codes, _ = _tb_table_arg(signature, table, "tb_probe_batch")
    if move_values not in (True, False, 0, 1):
        raise XqError(f"tb_probe_batch: move_values must be a bool, got {move_values!r}")
    n, _ = _positions_arg(boards, side, "tb_probe_batch")
    dev = table.device
    if n and (boards.device != dev or side.device != dev):
        raise XqError(f"tb_probe_batch: boards and side must be on the table's device {dev}, got {boards.device} and {side.device}")
    out = {"value": torch.zeros(n, dtype=torch.int16, device=dev), "moves": torch.zeros((n, MAXM), dtype=torch.int16, device=dev),
           "counts": torch.zeros(n, dtype=torch.int16, device=dev),
           "best_action": torch.zeros(n, dtype=torch.int16, device=dev), "status": torch.zeros(n, dtype=torch.uint8, device=dev)}
    if move_values:
        out["move_value"] = torch.zeros((n, MAXM), dtype=torch.int16, device=dev)
    if n:
        arr, P = _tb_pieces(codes)
        check(lib().xq_tb_probe_batch(arr, P, _dev(table), _dev(boards), _dev(side), n, _dev(out["value"]), _dev(out["moves"]),
                                      _dev(out["counts"]), _dev(out["move_value"]) if move_values else None,
                                      _dev(out["best_action"]), _dev(out["status"]), stream_ptr(dev)), "xq_tb_probe_batch")
    return out


def tb_play_batch(signature, table: torch.Tensor, boards: torch.Tensor, side: torch.Tensor, action=None, out=None):
    """One move per position (xq_tb_play_batch): boards int8[n,90] (or [n,10,9]) and side int8[n] on the table's device; action
    None (the table plays its best move everywhere) or int16[n] there holding uint16 action ids, TB_NO_MOVE (-1) where the table
    chooses -> dict of device tensors: boards int8[n,90] and side int8[n] after the move, played (u16-as-int16 [n]; TB_NO_MOVE
    reads -1), value int16[n] (the entry's before the move), move_value int16[n] (what the mover gets by it), value_out int16[n]
    (the new entry's, from the new side's view), status uint8[n] (the probe's bits, +8 no legal move, +16 the action is no legal
    move; with any bit the position is copied and nothing is played).  `out` = such a dict to write into; its boards and side may
    be the inputs themselves (a walk in place)."""
    codes, _ = _tb_table_arg(signature, table, "tb_play_batch")
    n, _ = _positions_arg(boards, side, "tb_play_batch")
    dev = table.device
    if n and (boards.device != dev or side.device != dev):
        raise XqError(f"tb_play_batch: boards and side must be on the table's device {dev}, got {boards.device} and {side.device}")
    if action is not None and (not isinstance(action, torch.Tensor) or action.dtype != torch.int16 or tuple(action.shape) != (n,) or
                               (n and action.device != dev)):
        got = (action.dtype, tuple(action.shape), action.device) if isinstance(action, torch.Tensor) else type(action).__name__
        raise XqError(f"tb_play_batch: action must be None or int16[{n}] on the table's device, got {got}")
    shapes = {"boards": ((n, 90), torch.int8), "side": ((n,), torch.int8), "played": ((n,), torch.int16), "value": ((n,), torch.int16),
              "move_value": ((n,), torch.int16), "value_out": ((n,), torch.int16), "status": ((n,), torch.uint8)}
    if out is None:
        out = {k: torch.zeros(shape, dtype=dt, device=dev) for k, (shape, dt) in shapes.items()}
    else:
        for k, (shape, dt) in shapes.items():
            t = out.get(k) if isinstance(out, dict) else None
            if not isinstance(t, torch.Tensor) or t.dtype != dt or t.numel() != n * (90 if k == "boards" else 1) or (n and t.device != dev):
                raise XqError(f"tb_play_batch: out[{k!r}] must be a {dt} tensor of shape {shape} on the table's device")
    if n:
        arr, P = _tb_pieces(codes)
        check(lib().xq_tb_play_batch(arr, P, _dev(table), _dev(boards), _dev(side), None if action is None else _dev(action), n,
                                     _dev(out["boards"]), _dev(out["side"]), _dev(out["played"]), _dev(out["value"]),
                                     _dev(out["move_value"]), _dev(out["value_out"]), _dev(out["status"]), stream_ptr(dev)),
              "xq_tb_play_batch")
    return out


def tb_samples(signature, table: torch.Tensor, index: torch.Tensor, policy: int = 0):
    """Table entries as training samples (xq_tb_samples): index int32[n] on the table's device -> (samples uint8[n, 640], status
    uint8[n]) there.  Row i is entry index[i]: its board and side, z the sign of its value, the ordered legal moves, one visit at
    every optimal move (policy 0) or at the first one (policy 1), game_seq the entry index.  status 0 written; 1 the index is
    outside the table; 4 an invalid entry; 8 no legal move: such a row is 640 zero bytes."""
    codes, _ = _tb_table_arg(signature, table, "tb_samples")
    if isinstance(policy, bool) or not isinstance(policy, int) or policy not in (0, 1):
        raise XqError(f"tb_samples: policy must be 0 (every optimal move) or 1 (the first one), got {policy!r}")
    dev = table.device
    if not isinstance(index, torch.Tensor) or index.dtype != torch.int32 or index.dim() != 1 or (len(index) and index.device != dev):
        got = (index.dtype, tuple(index.shape), index.device) if isinstance(index, torch.Tensor) else type(index).__name__
        raise XqError(f"tb_samples: index must be int32[n] on the table's device, got {got}")
    n = len(index)
    rows = torch.empty((n, SAMPLE_BYTES), dtype=torch.uint8, device=dev)
    status = torch.zeros(n, dtype=torch.uint8, device=dev)
    if n:
        arr, P = _tb_pieces(codes)
        opts = TbSampleOpts(int(policy), (C.c_int32 * 3)(0, 0, 0))
        check(lib().xq_tb_samples(arr, P, _dev(table), _dev(index), n, C.byref(opts), _dev(rows), _dev(status), stream_ptr(dev)),
              "xq_tb_samples")
    return rows, status


def adjudicate_opts(draws=True, both_colours=True, min_ply=0, what: str = "adjudicate") -> AdjudicateOpts:
    """The options of table adjudication checked -> AdjudicateOpts (no GPU needed): draws and both_colours bools, min_ply an
    integer >= 0."""
    for name, v in (("draws", draws), ("both_colours", both_colours)):
        if v not in (False, True, 0, 1):
            raise XqError(f"{what}: {name} must be a bool, got {v!r}")
    try:
        ok = not isinstance(min_ply, bool) and int(min_ply) == min_ply and 0 <= int(min_ply) <= 2 ** 31 - 1
    except (TypeError, ValueError, OverflowError):
        ok = False
    if not ok:
        raise XqError(f"{what}: min_ply must be an integer >= 0, got {min_ply!r}")
    return AdjudicateOpts(int(bool(draws)), int(bool(both_colours)), int(min_ply), 0)


def tb_adjudicate_batch(signature, table: torch.Tensor, boards: torch.Tensor, side: torch.Tensor, draws: bool = True,
                        both_colours: bool = True):
    """The adjudication rule over positions (xq_tb_adjudicate_batch): boards int8[n,90] (or [n,10,9]) and side int8[n] on the
    table's device -> (status uint8[n], winner int8[n], value int16[n]) there.  status 0 decided; +1 not in the table under either
    colouring; +2 a king is missing; +4 an invalid entry; +8 a drawn entry with draws off; +16 matched through the colour-swapped
    image (beside 0 or 8).  winner is +1 / -1 / 0 where the position is decided, value the entry's word where one was read."""
    codes, entries = _tb_table_arg(signature, table, "tb_adjudicate_batch")
    opts = adjudicate_opts(draws, both_colours, 0, "tb_adjudicate_batch")
    n, _ = _positions_arg(boards, side, "tb_adjudicate_batch")
    dev = table.device
    if n and (boards.device != dev or side.device != dev):
        raise XqError(f"tb_adjudicate_batch: boards and side must be on the table's device {dev}, got {boards.device} and {side.device}")
    status = torch.zeros(n, dtype=torch.uint8, device=dev)
    winner = torch.zeros(n, dtype=torch.int8, device=dev)
    value = torch.zeros(n, dtype=torch.int16, device=dev)
    if n:
        arr, P = _tb_pieces(codes)
        check(lib().xq_tb_adjudicate_batch(arr, P, _dev(table), entries, _dev(boards), _dev(side), n, C.byref(opts), _dev(status),
                                           _dev(winner), _dev(value), stream_ptr(dev)), "xq_tb_adjudicate_batch")
    return status, winner, value


def engine_adjudicate(engine_handle, signature, table: torch.Tensor, opts: AdjudicateOpts, counters: torch.Tensor) -> None:
    """The engine stage (xq_engine_adjudicate) between select and expand: every slot that waits for its root's evaluation, whose
    game the rules have not ended and whose real board `table` decides gets root status REASON_TABLE and the winner.
    `engine_handle` is a `hip.Engine` (SelfPlayEngine.h), `counters` an int64 device tensor [n_games, 4] the caller zeroed
    (decisive, drawn, left alone, swapped).  On the current stream; does not synchronise."""
    codes, entries = _tb_table_arg(signature, table, "engine_adjudicate")
    if not isinstance(opts, AdjudicateOpts):
        raise XqError(f"engine_adjudicate: opts must be a hip.AdjudicateOpts, got {type(opts).__name__}")
    G = int(engine_handle.cfg.n_games)
    if not isinstance(counters, torch.Tensor) or counters.dtype != torch.int64 or tuple(counters.shape) != (G, 4) or \
            counters.device != table.device:
        raise XqError(f"engine_adjudicate: counters must be an int64 tensor [{G}, 4] on the table's device")
    arr, P = _tb_pieces(codes)
    check(lib().xq_engine_adjudicate(C.byref(engine_handle), arr, P, _dev(table), entries, C.byref(opts), _dev(counters),
                                     stream_ptr(table.device)), "xq_engine_adjudicate")


def resign_opts(threshold, check_steps, holdout_prob=0.0, what: str = "resign") -> ResignOpts:
    """The options of the per-side resign rule checked -> ResignOpts (no GPU needed): threshold a float that is no NaN (-inf:
    nobody resigns), check_steps an integer in 1..RESIGN_MAX_STEPS, holdout_prob in [0, 1]."""
    try:
        t, p = float(threshold), float(holdout_prob)
    except (TypeError, ValueError):
        raise XqError(f"{what}: threshold and holdout_prob must be numbers, got {threshold!r} and {holdout_prob!r}")
    if t != t:
        raise XqError(f"{what}: threshold must not be NaN")
    if not 0.0 <= p <= 1.0:                            # a NaN fails both comparisons
        raise XqError(f"{what}: holdout_prob must be in [0, 1], got {holdout_prob!r}")
    try:
        ok = not isinstance(check_steps, bool) and int(check_steps) == check_steps and 1 <= int(check_steps) <= RESIGN_MAX_STEPS
    except (TypeError, ValueError, OverflowError):
        ok = False
    if not ok:
        raise XqError(f"{what}: check_steps must be an integer in 1..{RESIGN_MAX_STEPS}, got {check_steps!r}")
    return ResignOpts(t, p, int(check_steps), 0)


def resign_exempt(seed: int, rank: int, slot: int, game_seq: int, holdout_prob: float) -> bool:
    """The holdout draw on the host (xq_resign_exempt_host, the device's own code; no GPU needed): is game `game_seq` of `slot`
    exempt from resignation?"""
    if not 0.0 <= float(holdout_prob) <= 1.0:
        raise XqError(f"resign_exempt: holdout_prob must be in [0, 1], got {holdout_prob!r}")
    if min(int(rank), int(slot), int(game_seq)) < 0:
        raise XqError(f"resign_exempt: rank, slot and game_seq must not be negative, got {rank}, {slot}, {game_seq}")
    rc = int(lib().xq_resign_exempt_host(int(seed) & (2 ** 64 - 1), int(rank), int(slot), int(game_seq), float(holdout_prob)))
    if rc < 0:
        check(rc, "xq_resign_exempt_host")
    return rc == 1


def resign_scan(values: torch.Tensor, lengths: torch.Tensor, first_side: torch.Tensor, threshold: float, check_steps: int):
    """The per-side resign rule over sequences of values (xq_resign_scan_batch): values float32[n, max_len], lengths int32[n] and
    first_side int8[n] (1 red, else black: the side to move at index 0) on the GPU -> (resign_index int32[n], the first index whose
    window is below the threshold or -1; resigner int8[n], that side or 0; level float32[n, 2], the lowest window of red and of
    black over the whole sequence, +inf for none; level_index int32[n, 2], where it was first reached, or -1)."""
    opts = resign_opts(threshold, check_steps, 0.0, "resign_scan")
    if not isinstance(values, torch.Tensor) or values.dtype != torch.float32 or values.dim() != 2:
        raise XqError("resign_scan: values must be a float32 tensor [n, max_len]")
    n, max_len = int(values.shape[0]), int(values.shape[1])
    dev = values.device
    if not (isinstance(lengths, torch.Tensor) and lengths.dtype == torch.int32 and tuple(lengths.shape) == (n,) and
            isinstance(first_side, torch.Tensor) and first_side.dtype == torch.int8 and tuple(first_side.shape) == (n,) and
            lengths.device == dev and first_side.device == dev):
        raise XqError(f"resign_scan: lengths must be int32[{n}] and first_side int8[{n}] on the values' device")
    index = torch.full((n,), -1, dtype=torch.int32, device=dev)
    resigner = torch.zeros(n, dtype=torch.int8, device=dev)
    level = torch.full((n, 2), float("inf"), dtype=torch.float32, device=dev)
    level_index = torch.full((n, 2), -1, dtype=torch.int32, device=dev)
    if n:
        with torch.cuda.device(dev):
            check(lib().xq_resign_scan_batch(_dev(values) if max_len else None, _dev(lengths), _dev(first_side), n, max_len,
                                             opts.check_steps, opts.threshold, _dev(index), _dev(resigner), _dev(level),
                                             _dev(level_index), stream_ptr(dev)), "xq_resign_scan_batch")
    return index, resigner, level, level_index


def _records_arg(samples: torch.Tensor, what: str):
    if samples.dtype != torch.uint8 or samples.dim() != 2 or samples.shape[1] != SAMPLE_BYTES:
        raise XqError(f"{what}: samples must be uint8[n, {SAMPLE_BYTES}], got {samples.dtype} {tuple(samples.shape)}")
    return _dev(samples)


def _index_arg(index, device, what: str):
    if index is None:
        return None
    if index.dtype != torch.int32 or index.dim() != 1 or index.device != device:
        raise XqError(f"{what}: index must be int32[n] on the samples' device")
    return _dev(index)


def samples_to_requests(samples: torch.Tensor, index=None, out=None):
    """Compact records as evaluation requests (xq_samples_to_requests): samples uint8[r, 640] on the GPU, index int32[n] there or
    None (the records in order) -> (planes float32[n,15,10,9], moves int16[n,128] holding uint16 action ids, counts int32[n]),
    the three arguments of an evaluator's `evaluate_legal`.  `out` = such a triple, preallocated."""
    p_s = _records_arg(samples, "samples_to_requests")
    dev = samples.device
    p_i = _index_arg(index, dev, "samples_to_requests")
    n = samples.shape[0] if index is None else index.shape[0]
    if out is None:
        out = (torch.empty((n, 15, 10, 9), dtype=torch.float32, device=dev), torch.empty((n, MAXM), dtype=torch.int16, device=dev),
               torch.empty(n, dtype=torch.int32, device=dev))
    x, moves, counts = out
    if x.shape != (n, 15, 10, 9) or x.dtype != torch.float32 or moves.shape != (n, MAXM) or moves.element_size() != 2 \
            or counts.shape != (n,) or counts.dtype != torch.int32:
        raise XqError("samples_to_requests: out = (float32[n,15,10,9], 16-bit [n,128], int32[n]) required")
    if n:
        check(lib().xq_samples_to_requests(p_s, p_i, n, _dev(x), _dev(moves), _dev(counts), stream_ptr(dev)), "xq_samples_to_requests")
    return x, moves, counts


def score_samples(samples: torch.Tensor, index, legal_logits: torch.Tensor, value: torch.Tensor, late_temperature: float = 0.3,
                  write_back: bool = False, out=None) -> torch.Tensor:
    """Samples against a network's answers (xq_score_samples): legal_logits float32[n,128] and value float32[n] as an evaluator's
    `evaluate_legal` returns them for the requests of `samples_to_requests(samples, index)` -> scores uint8[n, 16]
    (sample_format.SCORE_DTYPE).  `write_back` also marks the records themselves (sample_format.policy_stats)."""
    p_s = _records_arg(samples, "score_samples")
    dev = samples.device
    p_i = _index_arg(index, dev, "score_samples")
    n = samples.shape[0] if index is None else index.shape[0]
    if legal_logits.shape != (n, MAXM) or legal_logits.dtype != torch.float32 or value.shape != (n,) or value.dtype != torch.float32:
        raise XqError(f"score_samples: legal_logits float32[{n},{MAXM}] and value float32[{n}] required")
    if out is None:
        out = torch.zeros((n, SCORE_BYTES), dtype=torch.uint8, device=dev)
    elif out.shape != (n, SCORE_BYTES) or out.dtype != torch.uint8:
        raise XqError(f"score_samples: out uint8[{n},{SCORE_BYTES}] required")
    opts = ScoreOpts(float(late_temperature), 1 if write_back else 0, 0)
    check(lib().xq_score_samples(p_s, p_i, n, _dev(legal_logits) if n else None, _dev(value) if n else None, C.byref(opts),
                                 _dev(out) if n else None, stream_ptr(dev)), "xq_score_samples")
    return out


def surprise_counts(samples: torch.Tensor, alpha: float, seed: int, epoch: int) -> torch.Tensor:
    """How often each record is drawn in one epoch of policy-surprise weighted training (xq_surprise_counts): samples
    uint8[n, 640] on the GPU -> int32[n]; sample_format.surprise_counts is the numpy reference."""
    p_s = _records_arg(samples, "surprise_counts")
    n, dev = samples.shape[0], samples.device
    counts = torch.empty(n, dtype=torch.int32, device=dev)
    scratch = torch.empty(SURPRISE_SCRATCH_BYTES // 8, dtype=torch.int64, device=dev)
    opts = SurpriseOpts(float(alpha), int(seed) & (2 ** 64 - 1), int(epoch) & 0xFFFFFFFF, 0)
    check(lib().xq_surprise_counts(p_s if n else None, n, C.byref(opts), _dev(counts) if n else None, _dev(scratch),
                                   stream_ptr(dev)), "xq_surprise_counts")
    return counts


def surprise_count_host(policy_kl: float, marked, M: int, S: int, alpha: float, seed: int, epoch: int, slot: int, game_seq: int,
                        ply: int) -> int:
    """One record's epoch count by the device's own code on the host (xq_surprise_count_host; needs no GPU)."""
    c = lib().xq_surprise_count_host(float(policy_kl), 1 if marked else 0, int(M), int(S), float(alpha), int(seed) & (2 ** 64 - 1),
                                     int(epoch) & 0xFFFFFFFF, int(slot), int(game_seq), int(ply))
    if c < 0:
        raise XqError(f"xq_surprise_count_host failed: code {c} (alpha must be in [0, 1], got {alpha})")
    return c


def position_key_host(board, side: int, mirror: bool = True):
    """One position's key by the device's own code on the host (xq_position_key_host; needs no GPU): board = 90 int8 values ->
    (key as a Python int, mirrored 0 / 1); sample_format.position_key is the numpy reference."""
    import numpy as np
    b = np.ascontiguousarray(np.asarray(board, dtype=np.int8).reshape(90))
    mirrored = C.c_uint8(0)
    key = lib().xq_position_key_host(b.ctypes.data, int(side), POSITION_KEY_MIRROR if mirror else 0, C.addressof(mirrored))
    return int(key), int(mirrored.value)


def position_keys(samples: torch.Tensor, index=None, mirror: bool = True):
    """Position keys of compact records (xq_position_keys): samples uint8[r, 640] on the GPU, index int32[n] there or None (the
    records in order) -> (keys int64[n] holding the uint64 bit patterns, mirrored uint8[n])."""
    p_s = _records_arg(samples, "position_keys")
    dev = samples.device
    p_i = _index_arg(index, dev, "position_keys")
    n = samples.shape[0] if index is None else index.shape[0]
    keys = torch.empty(n, dtype=torch.int64, device=dev)
    mirrored = torch.empty(n, dtype=torch.uint8, device=dev)
    if n:
        check(lib().xq_position_keys(p_s, p_i, n, POSITION_KEY_MIRROR if mirror else 0, _dev(keys), _dev(mirrored), stream_ptr(dev)),
              "xq_position_keys")
    return keys, mirrored


def position_group_heads(samples: torch.Tensor, index, order: torch.Tensor, keys: torch.Tensor, mirrored: torch.Tensor) -> torch.Tensor:
    """Group heads in sorted order (xq_position_group_heads): order int32[n] = the rows in (stably) sorted order, keys int64[n]
    and mirrored uint8[n] per row as `position_keys` returns them (taken as given) -> head uint8[n], 1 where row order[j] starts
    a group: its key, side or canonical board differs from that of row order[j - 1]."""
    p_s = _records_arg(samples, "position_group_heads")
    dev = samples.device
    p_i = _index_arg(index, dev, "position_group_heads")
    n = samples.shape[0] if index is None else index.shape[0]
    if order.shape != (n,) or order.dtype != torch.int32 or keys.shape != (n,) or keys.dtype != torch.int64 \
            or mirrored.shape != (n,) or mirrored.dtype != torch.uint8:
        raise XqError(f"position_group_heads: order int32[{n}], keys int64[{n}] and mirrored uint8[{n}] required")
    head = torch.empty(n, dtype=torch.uint8, device=dev)
    if n:
        check(lib().xq_position_group_heads(p_s, p_i, _dev(order), _dev(keys), _dev(mirrored), n, _dev(head), stream_ptr(dev)),
              "xq_position_group_heads")
    return head


def groups_to_batch(samples: torch.Tensor, offsets: torch.Tensor, members: torch.Tensor, member_mirrored: torch.Tensor,
                    group: torch.Tensor, flip: torch.Tensor, late_temperature: float = 0.3, q_mix: float = 0.0, out=None):
    """Merged training samples (xq_groups_to_batch): offsets int32[n_groups + 1], members int32[] (record indices into samples) and
    member_mirrored uint8[] describe the groups; output row j is group group[j] (int32[n]) under flip[j] (uint8[n]) ->
    (states float32[n,15,10,9], pi float32[n,8100], z float32[n,1]); sample_format.merged_targets is the numpy reference."""
    p_s = _records_arg(samples, "groups_to_batch")
    dev = samples.device
    n, n_groups = group.shape[0], offsets.shape[0] - 1
    if offsets.dtype != torch.int32 or members.dtype != torch.int32 or member_mirrored.dtype != torch.uint8 \
            or member_mirrored.shape != members.shape or n_groups < 0:
        raise XqError("groups_to_batch: offsets int32[n_groups + 1], members int32[m] and member_mirrored uint8[m] required")
    if group.dtype != torch.int32 or flip.dtype != torch.uint8 or flip.shape != (n,):
        raise XqError(f"groups_to_batch: group int32[{n}] and flip uint8[{n}] required")
    if out is None:
        out = (torch.empty((n, 15, 10, 9), dtype=torch.float32, device=dev),
               torch.empty((n, ACTION_SPACE), dtype=torch.float32, device=dev), torch.empty((n, 1), dtype=torch.float32, device=dev))
    states, pi, z = out
    opts = BatchOpts(float(q_mix))
    if members.numel() == 0:                       # only empty groups: the arrays are never read, but the ABI wants pointers
        members, member_mirrored = torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.uint8, device=dev)
    if n:
        check(lib().xq_groups_to_batch(p_s, _dev(offsets), _dev(members), _dev(member_mirrored), n_groups, _dev(group), _dev(flip), n,
                                       float(late_temperature), C.byref(opts), _dev(states), _dev(pi), _dev(z), stream_ptr(dev)),
              "xq_groups_to_batch")
    return states, pi, z


def eval_mirror_bit(seed: int, rank: int, slot: int, game_seq: int, ply: int, is_root, sims_done: int, row: int = 0) -> int:
    """The evaluation mirror's bit of one request (xq_eval_mirror_bit_host: the device's own code on the host; needs no GPU).
    A root request is asked with sims_done = 0, as the mirrored gather does."""
    if not (0 <= int(seed) < 2 ** 64 and 0 <= int(game_seq) < 2 ** 32):
        raise XqError(f"eval_mirror_bit: seed must be a uint64 and game_seq a uint32, got {seed}, {game_seq}")
    b = lib().xq_eval_mirror_bit_host(int(seed), int(rank), int(slot), int(game_seq), int(ply), int(is_root), int(sims_done), int(row))
    if b not in (0, 1):
        raise XqError(f"xq_eval_mirror_bit_host failed: code {b}")
    return b


def mirror_requests(x: torch.Tensor, moves: torch.Tensor, counts: torch.Tensor, flags: torch.Tensor, out=None):
    """Rows of evaluation requests under the left-right mirror (xq_mirror_requests_batch): x float32[n,15,10,9], moves 16-bit
    [n,128], counts int32[n], flags uint8[n] -> (x_out, moves_out); row r is mirrored where flags[r] != 0 and copied otherwise.
    The move list keeps its order, so the evaluator's legal-move logits of a mirrored row are those of the original moves.
    `out` = (x_out, moves_out) preallocated, holding at least n rows (rows past n are not written)."""
    n = x.shape[0]
    if x.shape[1:] != (15, 10, 9) or x.dtype != torch.float32 or moves.shape != (n, MAXM) or moves.element_size() != 2 \
            or counts.shape != (n,) or counts.dtype != torch.int32 or flags.shape != (n,) or flags.dtype != torch.uint8:
        raise XqError("mirror_requests: x float32[n,15,10,9], moves 16-bit [n,128], counts int32[n], flags uint8[n] required")
    if out is None:
        out = (torch.empty_like(x), torch.empty_like(moves))
    xo, mo = out
    if xo.shape[0] < n or xo.shape[1:] != x.shape[1:] or xo.dtype != x.dtype or mo.shape[0] < n or mo.shape[1:] != moves.shape[1:] \
            or mo.dtype != moves.dtype:
        raise XqError("mirror_requests: out = (float32[>=n,15,10,9], 16-bit [>=n,128]) required")
    if n:
        check(lib().xq_mirror_requests_batch(_dev(x), _dev(moves), _dev(counts), _dev(flags), n, _dev(xo), _dev(mo), stream_ptr(x.device)),
              "xq_mirror_requests_batch")
    return xo, mo


def dedup_table_size(n_slots: int) -> int:
    """The request dedup's bucket count for `n_slots` slots: the smallest power of two >= max(16, 4 n_slots)."""
    t = 16
    while t < 4 * int(n_slots):
        t *= 2
    return t


def dedup_bucket(key12, table_size: int) -> int:
    """The bucket of a 12-word evaluation key in a table of `table_size` buckets (xq_evdedup_bucket_host; needs no GPU)."""
    import numpy as np
    k = np.ascontiguousarray(key12, dtype=np.uint32)
    if k.shape != (12,):
        raise XqError(f"dedup_bucket: a key has 12 uint32 words, got shape {k.shape}")
    b = lib().xq_evdedup_bucket_host(k.ctypes.data, int(table_size))
    if b < 0:
        raise XqError(f"xq_evdedup_bucket_host failed: code {b} (table_size must be a power of two, got {table_size})")
    return b


class DedupTable:
    """A request dedup object (xq_evdedup) for up to `n_slots` requests per step, with the device memory it lives in."""

    def __init__(self, n_slots: int, device="cuda"):
        nbytes = int(lib().xq_evdedup_bytes(int(n_slots)))
        if nbytes == 0:
            raise XqError(f"eval_dedup: n_slots must be in [1, 2^24], got {n_slots}")
        self.n_slots, self.bytes, self.device = int(n_slots), nbytes, torch.device(device)
        self.ws = torch.empty(nbytes + 256, dtype=torch.uint8, device=self.device)
        self.h = EvDedup()
        with torch.cuda.device(self.device):
            check(lib().xq_evdedup_init(C.byref(self.h), self.n_slots, (self.ws.data_ptr() + 255) & ~255, nbytes,
                                        stream_ptr(self.device)), "xq_evdedup_init")
        self.table_size = int(self.h.table_size)

    def table(self) -> torch.Tensor:
        """Zero-copy int32 [table_size] view of the buckets (2^31 - 1: empty).  For tests."""
        off = int(self.h.p[0]) - int(self.ws.data_ptr())
        return self.ws[off:off + 4 * self.table_size].view(torch.int32)

    def keys(self) -> torch.Tensor:
        """Zero-copy int32 [n_slots, 12] view of the keys of the last requests (uint32 bits; all 0 where no row ever asked).  For
        tests."""
        off = int(self.h.p[1]) - int(self.ws.data_ptr())
        return self.ws[off:off + 48 * self.n_slots].view(torch.int32).view(self.n_slots, 12)

    def stats(self) -> dict:
        """requests, merged, collisions, mismatches (xq_evdedup_stats_read).  Synchronises."""
        s = EvDedupStats()
        check(lib().xq_evdedup_stats_read(C.byref(self.h), C.byref(s), stream_ptr(self.device)), "xq_evdedup_stats_read")
        return s.as_dict()


def dedup_requests(x: torch.Tensor, counts: torch.Tensor, live: torch.Tensor, table: DedupTable, out=None):
    """The request dedup's kernels over caller-owned rows (xq_dedup_rows_batch): x float32[n,15,10,9], counts int32[n] legal-move
    counts, live int32[n] flags -> (rep int32[n], rows int32[n], n_live int32[1]) on the device.  rep[r] of a live row is the
    row that answers it (itself, or the lowest live row with the same planes and count); rows[:n_live] are the rows that
    represent themselves, in row order.  Entries of idle rows, and rows[] past n_live, are not written: `out` = (rep, rows,
    n_live) preallocated keeps whatever it held there."""
    n = x.shape[0]
    if x.shape[1:] != (15, 10, 9) or x.dtype != torch.float32 or counts.shape != (n,) or counts.dtype != torch.int32 \
            or live.shape != (n,) or live.dtype != torch.int32:
        raise XqError("dedup_requests: x float32[n,15,10,9], counts int32[n], live int32[n] required")
    if n > table.n_slots:
        raise XqError(f"dedup_requests: {n} rows do not fit a table made for {table.n_slots}")
    if out is None:
        out = (torch.zeros(n, dtype=torch.int32, device=x.device), torch.zeros(n, dtype=torch.int32, device=x.device),
               torch.zeros(1, dtype=torch.int32, device=x.device))
    rep, rows, n_live = out
    if any(t.dtype != torch.int32 for t in out) or rep.shape != (n,) or rows.shape != (n,) or n_live.shape != (1,):
        raise XqError("dedup_requests: out = (int32[n], int32[n], int32[1]) required")
    check(lib().xq_dedup_rows_batch(_dev(x) if n else None, _dev(counts) if n else None, _dev(live) if n else None, n,
                                    C.byref(table.h), _dev(rep) if n else None, _dev(rows) if n else None, _dev(n_live),
                                    stream_ptr(x.device)), "xq_dedup_rows_batch")
    return rep, rows, n_live


def bias_act_(y: torch.Tensor, bias: torch.Tensor, residual=None, relu: bool = True) -> torch.Tensor:
    """In place on a channels-last activation: y = act(y + bias[c] (+ residual)).  `y` is a 4-d tensor whose
    memory is NHWC-contiguous (torch.channels_last) or a 2-d [rows, C] tensor."""
    if y.dim() == 4:
        if not y.is_contiguous(memory_format=torch.channels_last):
            raise XqError("bias_act_: channels_last tensor required")
        c = y.shape[1]
        rows = y.numel() // c
        if residual is not None and not residual.is_contiguous(memory_format=torch.channels_last):
            raise XqError("bias_act_: channels_last residual required")
    else:
        rows, c = y.shape
        if not y.is_contiguous():
            raise XqError("bias_act_: contiguous tensor required")
    check(lib().xq_bias_act(y.data_ptr(), bias.data_ptr(), None if residual is None else residual.data_ptr(),
                            rows, c, int(relu), stream_ptr(y.device)), "xq_bias_act")
    return y


def stem_weights(w_in: torch.Tensor) -> torch.Tensor:
    """Folded input filters float32[C,15,3,3] -> float32[135, C] (entry = plane*9 + ky*3 + kx), see xq_stem_conv."""
    c = w_in.shape[0]
    if w_in.shape != (c, 15, 3, 3):
        raise XqError("stem_weights: [C,15,3,3] required")
    return w_in.detach().permute(1, 2, 3, 0).reshape(135, c).contiguous()


def _live_ptr(n_live, device) -> int:
    """The live-row count of the *_live entry points: an int32 scalar tensor on the computing device (read there, never
    on the host)."""
    if n_live.dtype != torch.int32 or n_live.numel() != 1 or n_live.device != device:
        raise XqError("n_live: one int32 element on the computing device required")
    return n_live.data_ptr()


def stem_conv(planes: torch.Tensor, wt: torch.Tensor, bias: torch.Tensor, out: torch.Tensor, n_live=None) -> torch.Tensor:
    """planes float32[G,15,10,9] contiguous -> out float32[G,90,C] = relu(conv3x3(planes) + bias), NHWC.  With `n_live`
    (int32 device scalar) only boards [0, n_live) are read and written (xq_stem_conv_live); G is the capacity."""
    g = planes.shape[0]
    c = wt.shape[1]
    if planes.shape[1:] != (15, 10, 9) or not planes.is_contiguous() or wt.shape != (135, c) or not wt.is_contiguous() \
            or out.shape != (g, 90, c) or not out.is_contiguous() or planes.dtype != torch.float32:
        raise XqError("stem_conv: planes [G,15,10,9], wt [135,C], out [G,90,C] contiguous float32 required")
    if n_live is not None:
        check(lib().xq_stem_conv_live(planes.data_ptr(), wt.data_ptr(), bias.data_ptr(), out.data_ptr(), g,
                                      _live_ptr(n_live, planes.device), c, stream_ptr(planes.device)), "xq_stem_conv_live")
        return out
    check(lib().xq_stem_conv(planes.data_ptr(), wt.data_ptr(), bias.data_ptr(), out.data_ptr(), g, c,
                             stream_ptr(planes.device)), "xq_stem_conv")
    return out


def heads_1x1(rows: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, n_live=None, out=None):
    """rows float32[R, C] (NHWC rows of the tower output), w float32[36, C], bias float32[36] ->
    (policy features float32[R, 32], value features float32[R, 4]), ReLU applied (model.py:43-62).  With `n_live` (int32
    device scalar, in POSITIONS of 90 rows) only rows [0, 90 n_live) are read and written (xq_heads_1x1_live); `out` = (p, v)
    preallocated."""
    r, c = rows.shape
    if not rows.is_contiguous() or w.shape != (36, c) or not w.is_contiguous() or bias.shape != (36,):
        raise XqError("heads_1x1: rows [R,C] contiguous, w [36,C], bias [36] required")
    if out is not None:
        p, v = out
        if p.shape != (r, 32) or v.shape != (r, 4) or not p.is_contiguous() or not v.is_contiguous():
            raise XqError("heads_1x1: out = (float32[R,32], float32[R,4]) contiguous")
    else:
        p = torch.empty((r, 32), dtype=torch.float32, device=rows.device)
        v = torch.empty((r, 4), dtype=torch.float32, device=rows.device)
    if n_live is not None:
        check(lib().xq_heads_1x1_live(rows.data_ptr(), w.data_ptr(), bias.data_ptr(), p.data_ptr(), v.data_ptr(), r,
                                      _live_ptr(n_live, rows.device), c, stream_ptr(rows.device)), "xq_heads_1x1_live")
        return p, v
    check(lib().xq_heads_1x1(rows.data_ptr(), w.data_ptr(), bias.data_ptr(), p.data_ptr(), v.data_ptr(), r, c,
                             stream_ptr(rows.device)), "xq_heads_1x1")
    return p, v


def wino_transform_weights(w: torch.Tensor, co_block: int = 64) -> torch.Tensor:
    """Folded 3x3 filters float32[C,C,3,3] -> the kernel's pre-transformed layout (see include/xq_hip.h,
    xq_wino_conv3x3): U = s_p (G_r g G_c'^T)[p][j] per (co, ci) for the F(2,3) x F(3,3) transform, computed in float64,
    stored float32 [C/co_block][C/8][20][2][co_block][4]; co_block = 64 (narrow kernel) or 128 (XQ_CONV_WIDE)."""
    c = w.shape[0]
    if w.shape != (c, c, 3, 3) or co_block not in (64, 128) or c % co_block or 8 % (c // co_block):
        raise XqError("wino_transform_weights: [C,C,3,3] with C a multiple of co_block (64 or 128), C / co_block in {1,2,4,8}")
    gr = torch.tensor([[1.0, 0.0, 0.0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0.0, 0.0, 1.0]], dtype=torch.float64)
    # F(3,3) at the points 0, 1, -1, 2, inf; the kernel's B^T rows are the textbook ones times (2, 2, 6, 6, 1)
    gc = torch.tensor([[1.0, 0.0, 0.0], [1.0, 1.0, 1.0], [1.0, -1.0, 1.0], [1.0, 2.0, 4.0], [0.0, 0.0, 1.0]], dtype=torch.float64)
    gc = gc * torch.tensor([0.5, 0.5, 1.0 / 6.0, 1.0 / 6.0, 1.0], dtype=torch.float64)[:, None]
    u = torch.einsum("pr,oirs,qs->pqoi", gr, w.detach().to("cpu", torch.float64), gc)      # [4,5,co,ci]
    u[2] = -u[2]                    # the kernel forms row 2 of B_r^T d as d1 - d2 (the negative of the textbook row)
    u = u.reshape(20, c // co_block, co_block, c // 8, 2, 4)                               # xi, cog, co, chunk, quad, k
    u = u.permute(1, 3, 0, 4, 2, 5).contiguous().to(torch.float32)                         # cog, chunk, xi, quad, co, k
    return u.to(w.device)


def wino_transform_filters_device(w: torch.Tensor, co_block: int = 64, dgrad: bool = False, out: torch.Tensor = None,
                                  both: bool = False) -> torch.Tensor:
    """`wino_transform_weights` by one kernel launch on the device (xq_wino_transform_filters; the train step re-transforms every
    optimizer step).  `dgrad=True`: the filters of the data-gradient convolution, w'[co][ci][r][s] = w[ci][co][2-r][2-s].
    `both=True`: one launch, returns a [2, ...] tensor -- [0] the forward filters, [1] the data-gradient filters."""
    c = w.shape[0]
    if w.shape != (c, c, 3, 3) or w.dtype != torch.float32 or not w.is_cuda or co_block not in (64, 128) or c % co_block \
            or 8 % (c // co_block):
        raise XqError("wino_transform_filters_device: float32[C,C,3,3] on the GPU, C a multiple of co_block (64 or 128), C / co_block in {1,2,4,8}")
    w = w.detach().contiguous()
    shape = (c // co_block, c // 8, 20, 2, co_block, 4)
    if out is None:
        out = torch.empty(((2,) + shape) if both else shape, dtype=torch.float32, device=w.device)
    check(lib().xq_wino_transform_filters(w.data_ptr(), out.data_ptr(), c, (4 if co_block == 128 else 0) | (16 if both else 8 if dgrad else 0),
                                          stream_ptr(w.device)), "xq_wino_transform_filters")
    return out


def wino_wgrad(x: torch.Tensor, dy: torch.Tensor) -> torch.Tensor:
    """Weight gradient of the 3x3 convolution (xq_wino_wgrad): x, dy float32[B, 90, C] contiguous -> float32[C, C, 3, 3]."""
    b, n, c = x.shape
    if n != 90 or dy.shape != x.shape or x.dtype != torch.float32 or dy.dtype != torch.float32 or not x.is_contiguous() \
            or not dy.is_contiguous() or not x.is_cuda:
        raise XqError("wino_wgrad: float32[B,90,C] contiguous tensors on the GPU required")
    nbytes = lib().xq_wino_wgrad_scratch_bytes(b, c)
    if nbytes == 0:
        raise XqError("wino_wgrad: channels must be 64, 128, 256 or 512")
    scratch = torch.empty(nbytes // 4, dtype=torch.float32, device=x.device)
    dw = torch.empty((c, c, 3, 3), dtype=torch.float32, device=x.device)
    check(lib().xq_wino_wgrad(x.data_ptr(), dy.data_ptr(), dw.data_ptr(), scratch.data_ptr(), b, c, stream_ptr(x.device)), "xq_wino_wgrad")
    return dw


def wino_transform_weights_bf16(w: torch.Tensor) -> torch.Tensor:
    """Folded 3x3 filters float32[C,C,3,3] -> the bf16 layout of xq_wino_conv3x3_bf16 (REDUCED PRECISION, throughput mode):
    the float32 wide-layout tensor of `wino_transform_weights(w, 128)` regrouped to 16-channel chunks and rounded to bf16,
    bf16[C/128][C/16][20][2][128][8] with input channel 16*chunk + 8*h + k."""
    c = w.shape[0]
    if c % 128 or (c // 16) % 4:
        raise XqError("wino_transform_weights_bf16: C must be 128, 256 or 512")
    u = wino_transform_weights(w, 128)                                 # [cog, chunk8, xi, quad, co, k4]
    ng = c // 128
    u = u.view(ng, c // 16, 2, 20, 2, 128, 4)                          # cog, chunk16, h, xi, quad, co, k4
    u = u.permute(0, 1, 3, 2, 5, 4, 6).contiguous().view(ng, c // 16, 20, 2, 128, 8)   # cog, chunk16, xi, h, co, (quad, k4)
    return u.to(torch.bfloat16).contiguous()


def wino_conv3x3_bf16(x: torch.Tensor, u: torch.Tensor, bias: torch.Tensor, out: torch.Tensor, residual=None,
                      relu: bool = True, reverse: bool = False, n_live=None) -> torch.Tensor:
    """REDUCED-PRECISION convolution (xq_wino_conv3x3_bf16): x, out, residual float32[B, 90, C]; u from
    `wino_transform_weights_bf16`.  `n_live`: as `wino_conv3x3`."""
    b, n, c = x.shape
    if n != 90 or not x.is_contiguous() or not out.is_contiguous() or out.shape != x.shape or u.dtype != torch.bfloat16:
        raise XqError("wino_conv3x3_bf16: float32[B,90,C] contiguous tensors and bf16 weights required")
    if n_live is not None:
        check(lib().xq_wino_conv3x3_bf16_live(x.data_ptr(), u.data_ptr(), bias.data_ptr(),
                                              None if residual is None else residual.data_ptr(), out.data_ptr(), b,
                                              _live_ptr(n_live, x.device), c, int(relu) | (2 if reverse else 0),
                                              stream_ptr(x.device)), "xq_wino_conv3x3_bf16_live")
        return out
    check(lib().xq_wino_conv3x3_bf16(x.data_ptr(), u.data_ptr(), bias.data_ptr(),
                                     None if residual is None else residual.data_ptr(), out.data_ptr(), b, c,
                                     int(relu) | (2 if reverse else 0), stream_ptr(x.device)), "xq_wino_conv3x3_bf16")
    return out


def wino_conv3x3(x: torch.Tensor, u: torch.Tensor, bias: torch.Tensor, out: torch.Tensor, residual=None,
                 relu: bool = True, reverse: bool = False, n_live=None) -> torch.Tensor:
    """x, out, residual: float32[B, 90, C] contiguous (NHWC); out must not alias x / residual.  `reverse` walks the batch
    back to front (identical results; see XQ_CONV_REVERSE).  The kernel variant follows the weight layout: `u` from
    `wino_transform_weights(w, 128)` (shape [C/128, ...]) selects XQ_CONV_WIDE.  With `n_live` (int32 device scalar) B is the
    capacity and only boards [0, n_live) are read and written (xq_wino_conv3x3_live)."""
    b, n, c = x.shape
    if n != 90 or not x.is_contiguous() or not out.is_contiguous() or out.shape != x.shape:
        raise XqError("wino_conv3x3: float32[B,90,C] contiguous tensors required")
    flags = int(relu) | (2 if reverse else 0) | (4 if u.shape[4] == 128 else 0)
    if n_live is not None:
        check(lib().xq_wino_conv3x3_live(x.data_ptr(), u.data_ptr(), bias.data_ptr(),
                                         None if residual is None else residual.data_ptr(), out.data_ptr(), b,
                                         _live_ptr(n_live, x.device), c, flags, stream_ptr(x.device)), "xq_wino_conv3x3_live")
        return out
    check(lib().xq_wino_conv3x3(x.data_ptr(), u.data_ptr(), bias.data_ptr(),
                                None if residual is None else residual.data_ptr(), out.data_ptr(), b, c,
                                int(relu) | (2 if reverse else 0) | (4 if u.shape[4] == 128 else 0), stream_ptr(x.device)),
          "xq_wino_conv3x3")
    return out



def policy_head_legal(feat: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, moves: torch.Tensor, counts: torch.Tensor,
                      out: torch.Tensor, n_live=None) -> torch.Tensor:
    """feat float32[G, 2880] (NHWC policy features), w float32[8100, 2880] (columns in that order), bias float32[8100],
    moves int16[G, 128] (uint16 action ids), counts int32[G] -> out float32[G, 128]: logits of the listed moves only."""
    g = feat.shape[0]
    if feat.shape != (g, 2880) or w.shape != (ACTION_SPACE, 2880) or moves.shape != (g, MAXM) or counts.shape != (g,) \
            or out.shape != (g, MAXM) or counts.dtype != torch.int32 or moves.element_size() != 2 \
            or not (feat.is_contiguous() and w.is_contiguous() and moves.is_contiguous() and counts.is_contiguous() and out.is_contiguous()):
        raise XqError("policy_head_legal: feat [G,2880], w [8100,2880], moves 16-bit [G,128], counts int32 [G], out [G,128]")
    if n_live is not None:
        check(lib().xq_policy_head_legal_live(feat.data_ptr(), w.data_ptr(), bias.data_ptr(), moves.data_ptr(), counts.data_ptr(), g,
                                              _live_ptr(n_live, feat.device), out.data_ptr(), stream_ptr(feat.device)),
              "xq_policy_head_legal_live")
        return out
    check(lib().xq_policy_head_legal(feat.data_ptr(), w.data_ptr(), bias.data_ptr(), moves.data_ptr(), counts.data_ptr(), g,
                                     out.data_ptr(), stream_ptr(feat.device)), "xq_policy_head_legal")
    return out


def value_head(vfeat: torch.Tensor, w1t: torch.Tensor, b1: torch.Tensor, w2: torch.Tensor, b2: torch.Tensor, n_live=None,
               out=None) -> torch.Tensor:
    """vfeat float32[G, 360] (NHWC value features), w1t float32[360, 128], b1 [128], w2 [128], b2 [1] -> value float32[G].
    With `n_live` (int32 device scalar) only games [0, n_live) are read and written (xq_value_head_live); `out` preallocated."""
    g = vfeat.shape[0]
    if vfeat.shape != (g, 360) or w1t.shape != (360, 128) or not vfeat.is_contiguous() or not w1t.is_contiguous():
        raise XqError("value_head: vfeat [G,360], w1t [360,128] contiguous required")
    if out is None:
        out = torch.empty(g, dtype=torch.float32, device=vfeat.device)
    elif out.shape != (g,) or out.dtype != torch.float32 or not out.is_contiguous():
        raise XqError("value_head: out float32[G] contiguous")
    if n_live is not None:
        check(lib().xq_value_head_live(vfeat.data_ptr(), w1t.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), g,
                                       _live_ptr(n_live, vfeat.device), out.data_ptr(), stream_ptr(vfeat.device)), "xq_value_head_live")
        return out
    check(lib().xq_value_head(vfeat.data_ptr(), w1t.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), g, out.data_ptr(),
                              stream_ptr(vfeat.device)), "xq_value_head")
    return out
