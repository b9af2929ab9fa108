// xq_resign.hip -- the per-side resign rule with a no-resign holdout (map: xq_engine.hip; the normative text: include/xq_hip.h).
//
// The engine's own rule (expand_root_finish, the reference's) asks that the last K root values, each from its own side to move,
// all lie below the threshold: for K >= 2 red and black must both judge themselves lost on neighbouring plies.  It stays as it is.
// Under this option it is configured as a pure recorder (enable_resign = 1, resign_threshold = -inf): it fills the slot's ring
// E.resign[slot][16] and counts in GI_RESIGN_N, and never fires.  k_resign, launched ahead of the select call, reads the ring.
//
// THE RULE, one device function for both kernels (wave_window, level_update).  v_n is the n-th recorded value of a game, the
// sides to move alternate.  w_n = max(v_n, v_{n-2}, .., v_{n-2(K-1)}), defined for n >= 2(K-1): the K latest values of the side to
// move at n.  A window that holds a NaN is NaN.  level[s] is the minimum of the w_n of side s (strict <: the first position that
// reaches it gives level_ply; a NaN window lowers nothing), +inf while there is none.  The side to move resigns at the first n with
// w_n < threshold (a double comparison of the widened float32 values; NaN never).  Lane j < K of the wave loads v_{n-2j}, three
// shuffle steps give the maximum, one ballot the NaN.
//
//   k_resign_scan  the stateless batch call, one wave per sequence, WPW per workgroup; every output word is written; it walks the
//                  whole sequence, so the levels are those of an exempt game and resign_index is where any other game ends;
//   k_resign       the engine stage, one wave per slot, WPW per workgroup.  A wave exits after its first loads unless the slot's
//                  GI_GSEQ changed (a new game: the state is reset), GI_RESIGN_N advanced past seen_n (a new value: the level of
//                  the side to move is updated) or the slot stands at PH_FINISHED unclosed.  A slot at PH_SEARCH whose new window
//                  is below the threshold, in a game the holdout draw does not exempt, is ended: lane 0 writes the three words
//                  expand_root_finish writes (GI_FWINNER = -side, GI_FREASON = 3, GI_PHASE = PH_FINISHED).  The root was expanded
//                  by the expand kernel and has sims_done = 0 (tree reuse: its kept visits); no move was chosen, so the position
//                  has no sample.  What the expanded root leaves behind -- GI_ALLOC, the tree's node 0, GI_SIMS, the cap words, the
//                  Gumbel words -- the next root request rewrites; GI_RR_NODE was consumed by that expand kernel, GI_NPEND is 0 and
//                  no virtual loss is out.  The select call that follows flushes the game and counts it in ST_RESIGN.  A slot the
//                  rules ended at this very position is at PH_FINISHED already and stays the rules'.
//                  A finished exempt game appends one xq_resign_row; the row index is the one atomic of the kernel.
// No LDS, no scratch, no workgroup barrier.
//
// Counters: caller-owned uint64[n_games][4], row s written by slot s's wave only -- [0] games resigned, [1] holdout games closed,
// [2] rows dropped (the row array was full), [3] values seen.
#include "xq_engine_state.cuh"
#include "xq_tools.cuh"

namespace {

constexpr uint32_t RNG_RESIGN_HOLDOUT = (uint32_t)XQ_RNG_KIND_RESIGN_HOLDOUT;

// per-slot state of the stage, caller-owned and zeroed by the caller (game_seq 0 is no game: the first game resets the state)
struct RsState {
    int32_t seen_n;             // GI_RESIGN_N when the slot was last looked at
    int32_t game_seq;
    float level[2];             // red, black
    uint16_t level_ply[2];
    int32_t closed;             // the game is over and accounted for
    int32_t pad[2];
};
static_assert(sizeof(RsState) == 32 && sizeof(xq_resign_row) == 32 && sizeof(xq_resign_opts) == 24, "the resign stage's layouts");

// the holdout draw of the game that carries game_seq: stateless, never injected.  xq_resign_exempt_host runs this code.
__host__ __device__ inline bool resign_exempt(uint64_t seed, uint32_t rank, uint32_t slot, uint32_t game_seq, double prob) {
    const uint64_t x = philox_u64(seed, rank, slot, RNG_RESIGN_HOLDOUT, game_seq, 0u);
    return (double)(x >> 11) * (1.0 / 9007199254740992.0) < prob;
}

// w_n from the lanes' values: lane j < K holds v_{n-2j}, every other lane -inf.  Wave-uniform; NaN when a lane holds one.
__device__ __forceinline__ double wave_window(double x) {
    const bool nan = __ballot(x != x) != 0ull;
    double m = x;
#pragma unroll
    for (int off = 4; off > 0; off >>= 1) {          // K <= 8: lanes 0..7 hold the window
        const double o = __shfl_xor(m, off);
        m = o > m ? o : m;
    }
    const unsigned long long b = (unsigned long long)__double_as_longlong(m);
    const double w = __longlong_as_double((long long)(((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((unsigned)(b >> 32)) << 32) |
                                                      (unsigned)__builtin_amdgcn_readfirstlane((unsigned)b)));
    return nan ? __longlong_as_double(0x7FF8000000000000ll) : w;
}

// the level of the side to move takes window w, first reached at `ply`: strict, so a NaN and an equal window change nothing
__device__ __forceinline__ bool level_update(float &level, double w) { return w < (double)level; }

__global__ __launch_bounds__(64 * WPW) void k_resign_scan(const float *__restrict__ values, const int32_t *__restrict__ len,
                                                           const int8_t *__restrict__ first_side, int n, int max_len, int K,
                                                           double threshold, int32_t *__restrict__ resign_index,
                                                           int8_t *__restrict__ resigner, float *__restrict__ level,
                                                           int32_t *__restrict__ level_index) {
    XQ_WAVE_ITEM(n)
    const int lane = lane_id();
    int L = __builtin_amdgcn_readfirstlane(len[i]);
    L = L < 0 ? 0 : (L > max_len ? max_len : L);      // the loads stay inside the row
    const int first = __builtin_amdgcn_readfirstlane((int)first_side[i]) == 1 ? 1 : -1;
    const float *v = values + (size_t)i * max_len;
    float lv[2] = {INFINITY, INFINITY};
    int li[2] = {-1, -1};
    int ri = -1, rs = 0;
    for (int m = 2 * (K - 1); m < L; ++m) {
        const int k = m - 2 * lane;                   // lane < K: k >= m - 2(K-1) >= 0
        const double x = lane < K ? (double)v[k] : -INFINITY;
        const double w = wave_window(x);
        const int side = (m & 1) ? -first : first;
        const int s = side == 1 ? 0 : 1;
        if (level_update(lv[s], w)) { lv[s] = (float)w; li[s] = m; }
        if (ri < 0 && w < threshold) { ri = m; rs = side; }
    }
    if (lane == 0) {
        resign_index[i] = ri;
        resigner[i] = (int8_t)rs;
        level[(size_t)i * 2] = lv[0]; level[(size_t)i * 2 + 1] = lv[1];
        level_index[(size_t)i * 2] = li[0]; level_index[(size_t)i * 2 + 1] = li[1];
    }
}

__global__ __launch_bounds__(64 * WPW) void k_resign(Dev E, xq_resign_opts o, RsState *__restrict__ state, xq_resign_row *__restrict__ rows,
                                                      int max_rows, unsigned int *__restrict__ row_count,
                                                      unsigned long long *__restrict__ counters) {
    const int slot = blockIdx.x * WPW + (int)(threadIdx.x >> 6);
    if (slot >= E.cfg.n_games) return;
    const int lane = lane_id();
    int32_t *gi = E.gi + (size_t)slot * GI_N;
    RsState *st = state + slot;
    const int phase = __builtin_amdgcn_readfirstlane(gi[GI_PHASE]);
    const int gseq = __builtin_amdgcn_readfirstlane(gi[GI_GSEQ]);
    const int rn = __builtin_amdgcn_readfirstlane(gi[GI_RESIGN_N]);
    int seen = __builtin_amdgcn_readfirstlane(st->seen_n);
    int closed = __builtin_amdgcn_readfirstlane(st->closed);
    const bool new_game = gseq != __builtin_amdgcn_readfirstlane(st->game_seq);
    if (new_game) { seen = 0; closed = 0; }
    const bool new_value = rn > seen;
    const bool closing = phase == PH_FINISHED && !closed && gseq != 0;
    if (!new_game && !new_value && !closing) return;

    float lv[2] = {INFINITY, INFINITY};
    int lp[2] = {0, 0};
    if (!new_game) {
        lv[0] = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(st->level[0])));
        lv[1] = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(st->level[1])));
        lp[0] = __builtin_amdgcn_readfirstlane((int)st->level_ply[0]);
        lp[1] = __builtin_amdgcn_readfirstlane((int)st->level_ply[1]);
    }
    const int side = __builtin_amdgcn_readfirstlane(gi[GI_SIDE]);
    const int mc = __builtin_amdgcn_readfirstlane(gi[GI_MC]);
    const int K = o.check_steps;
    bool low = false;
    const int m = rn - 1;                             // the newest value's index
    if (new_value && m >= 2 * (K - 1)) {
        const double *ring = E.resign + (size_t)slot * 16;
        const double x = lane < K ? ring[(m - 2 * lane) & 15] : -INFINITY;      // m - 2 lane >= 0 for lane < K
        const double w = wave_window(x);
        const int s = side == 1 ? 0 : 1;
        if (level_update(lv[s], w)) { lv[s] = (float)w; lp[s] = mc; }
        low = w < o.threshold;
    }
    bool exempt = false;
    if ((low && phase == PH_SEARCH) || closing)
        exempt = resign_exempt(E.cfg.seed, (uint32_t)E.cfg.rank, (uint32_t)slot, (uint32_t)gseq, o.holdout_prob);
    const bool fire = low && phase == PH_SEARCH && !exempt;
    if (lane != 0) return;
    unsigned long long *c = counters + (size_t)slot * 4;
    if (fire) {
        gi[GI_FWINNER] = -side; gi[GI_FREASON] = 3; gi[GI_PHASE] = PH_FINISHED;
        c[0] += 1ull;
        closed = 1;
    }
    if (closing) {
        closed = 1;
        if (exempt) {
            c[1] += 1ull;
            const unsigned r = atomicAdd(row_count, 1u);
            if (r < (unsigned)max_rows) {
                xq_resign_row row;
                row.slot = (uint32_t)slot; row.game_seq = (uint32_t)gseq;
                row.level[0] = lv[0]; row.level[1] = lv[1];
                row.level_ply[0] = (uint16_t)lp[0]; row.level_ply[1] = (uint16_t)lp[1];
                row.winner = (int8_t)gi[GI_FWINNER]; row.reason = (uint8_t)gi[GI_FREASON]; row.plies = (uint16_t)mc;
                row.zero[0] = 0u; row.zero[1] = 0u;
                rows[r] = row;
            } else {
                c[2] += 1ull;
            }
        }
    }
    if (new_value) c[3] += 1ull;
    st->seen_n = rn; st->game_seq = gseq; st->closed = closed;
    st->level[0] = lv[0]; st->level[1] = lv[1];
    st->level_ply[0] = (uint16_t)lp[0]; st->level_ply[1] = (uint16_t)lp[1];
}

bool opts_ok(const xq_resign_opts *o) {
    return o && o->reserved == 0 && o->check_steps >= 1 && o->check_steps <= XQ_RESIGN_MAX_STEPS && o->threshold == o->threshold &&
           o->holdout_prob >= 0.0 && o->holdout_prob <= 1.0;      // a NaN probability fails both comparisons
}

}  // namespace

extern "C" {

size_t xq_resign_state_bytes(int n_games) { return n_games > 0 ? (size_t)n_games * sizeof(RsState) : 0; }

int xq_resign_exempt_host(uint64_t seed, int rank, int slot, uint32_t game_seq, double holdout_prob) {
    if (rank < 0 || slot < 0 || !(holdout_prob >= 0.0 && holdout_prob <= 1.0)) return XQ_ERR_ARG;
    return resign_exempt(seed, (uint32_t)rank, (uint32_t)slot, game_seq, holdout_prob) ? 1 : 0;
}

int xq_resign_scan_batch(const float *dev_values, const int32_t *dev_len, const int8_t *dev_first_side, int n, int max_len,
                         int check_steps, double threshold, int32_t *dev_resign_index, int8_t *dev_resigner, float *dev_level,
                         int32_t *dev_level_index, void *stream) {
    if (n < 0 || max_len < 0 || check_steps < 1 || check_steps > XQ_RESIGN_MAX_STEPS || threshold != threshold) return XQ_ERR_ARG;
    if (n > 0 && (!dev_len || !dev_first_side || !dev_resign_index || !dev_resigner || !dev_level || !dev_level_index)) return XQ_ERR_ARG;
    if (n > 0 && max_len > 0 && !dev_values) return XQ_ERR_ARG;
    if (n == 0) return XQ_OK;
    for_position_chunks(n, [&](size_t off, int m) {
        hipLaunchKernelGGL(k_resign_scan, dim3((m + WPW - 1) / WPW), dim3(64 * WPW), 0, (hipStream_t)stream,
                           dev_values + off * (size_t)max_len, dev_len + off, dev_first_side + off, m, max_len, check_steps, threshold,
                           dev_resign_index + off, dev_resigner + off, dev_level + off * 2, dev_level_index + off * 2);
    });
    return launch_status();
}

int xq_engine_resign(const xq_engine *eng, const xq_resign_opts *opts, void *dev_state, xq_resign_row *dev_rows, int max_rows,
                     unsigned int *dev_row_count, unsigned long long *dev_counters, void *stream) {
    if (!eng || !dev_state || !dev_row_count || !dev_counters || !opts_ok(opts) || max_rows < 0) return XQ_ERR_ARG;
    if (max_rows > 0 && !dev_rows) return XQ_ERR_ARG;
    if (eng->cfg.manual_moves != 0) return XQ_ERR_ARG;             // arena and search-only engines record no root values
    // the engine's own rule must be the recorder: it fills the ring and never fires (no value is below -inf)
    if (!eng->cfg.enable_resign || !(eng->cfg.resign_threshold == -INFINITY)) return XQ_ERR_ARG;
    if (eng->cfg.n_games <= 0 || !eng->p[P_GI] || !eng->p[P_RESIGN]) return XQ_ERR_ARG;
    hipLaunchKernelGGL(k_resign, dim3((eng->cfg.n_games + WPW - 1) / WPW), dim3(64 * WPW), 0, (hipStream_t)stream, make_dev(eng), *opts,
                       (RsState *)dev_state, dev_rows, max_rows, dev_row_count, dev_counters);
    return launch_status();
}

}  // extern "C"
