// xq_engine_packed.hip -- the engine's packed steps (map: xq_engine.hip).
//
// Packed step (xq_engine_compact / xq_engine_expand_packed): the evaluator sees only the slots that asked for an
// evaluation, packed to the front of engine-owned buffers in slot order.  The predicate is k_expand's own (phase
// WAIT_ROOT / WAIT_LEAF after select), so the two kernels cannot disagree about which slots need output.
#include "xq_engine_state.cuh"

#pragma clang fp contract(off)

namespace {

__global__ __launch_bounds__(CPT) void k_compact(Dev E, int32_t *__restrict__ n_live, int32_t *__restrict__ rows) {
    block_compact(E, E.cfg.n_games, [&](int s) { return slot_waits(E, s); }, n_live, rows);
}

// Gather of the packed rows: one workgroup per row of the capacity, rows past *n_live exit.  Per row the 5 400-byte
// planes (8-byte aligned: float2), the 256-byte ordered move list and its count.
__global__ __launch_bounds__(256) void k_gather_rows(Dev E, const int32_t *__restrict__ n_live, const int32_t *__restrict__ rows,
                                                     const float *__restrict__ nn_in, float *__restrict__ x, uint16_t *__restrict__ moves,
                                                     int32_t *__restrict__ counts) {
    const int r = blockIdx.x;
    if (r >= *n_live) return;
    const int slot = rows[r], t = threadIdx.x;
    const float2 *src = (const float2 *)(nn_in + (size_t)slot * XQ_STATE_FLOATS);
    float2 *dst = (float2 *)(x + (size_t)r * XQ_STATE_FLOATS);
    for (int i = t; i < XQ_STATE_FLOATS / 2; i += 256) dst[i] = src[i];
    if (t < XQ_MAXM / 2)
        ((uint32_t *)(moves + (size_t)r * XQ_MAXM))[t] = ((const uint32_t *)(E.pmoves + (size_t)slot * XQ_MAXM))[t];
    if (t == 0) counts[r] = E.req[slot];
}

// Evaluation mirror (xq_engine_init_em, opt-in; rules in include/xq_hip.h).  The board is left-right symmetric, so a request may be
// evaluated in either orientation; the gather below hands the evaluator the mirrored row when the request's bit is 1.  The move
// list is mirrored IN PLACE -- word i stays word i -- so k_policy_legal's out[i] is the logit of the original move i and
// k_scatter_rows / k_expand see nothing of it.

// one action id under the mirror: both squares' columns c -> 8 - c (k_samples_to_batch's arithmetic); an involution over [0, 8100)
__host__ __device__ inline int mirror_action(int a) {
    const int from = a / 90, to = a - from * 90;
    const int fr = from / 9, fc = from - fr * 9, tr = to / 9, tc = to - tr * 9;
    return (fr * 9 + (8 - fc)) * 90 + tr * 9 + (8 - tc);
}

// The bit of one request: include/xq_hip.h writes the packing out.  Philox stream kind 9, two draws: the first keys the second.
__host__ __device__ inline int eval_mirror_bit(uint64_t seed, uint32_t rank, uint32_t slot, uint32_t game_seq, uint32_t ply,
                                               uint32_t is_root, uint32_t sims_done, uint32_t row) {
    const uint64_t h = philox_u64(seed, rank, slot, 9u, game_seq, ply & 0xFFFFFFu);
    const uint64_t r = philox_u64(h, rank, slot, 9u, (is_root << 31) | (row << 16) | sims_done, 0u);
    return (int)(r >> 63);
}

// One request row, by the 256 threads of a workgroup (t = threadIdx.x): the 15 planes with column c -> 8 - c (the centre column
// maps to itself) and the XQ_MAXM words of the move list.  Word i < count is mirrored when it is an action id (< 8100); a word at
// or past the count, or one that is no action id, is copied as it is.  All 128 words are written either way.
__device__ __forceinline__ void mirror_row(const float *__restrict__ src_x, const uint16_t *__restrict__ src_m, int count,
                                           float *__restrict__ dst_x, uint16_t *__restrict__ dst_m, int t) {
    for (int e = t; e < XQ_STATE_FLOATS; e += 256) {
        const int c = e % 9;
        dst_x[e] = src_x[e + 8 - 2 * c];
    }
    if (t < XQ_MAXM) {
        const int a = src_m[t];
        dst_m[t] = (uint16_t)((t < count && a < XQ_ACTION_SPACE) ? mirror_action(a) : a);
    }
}

// k_gather_rows's copy of one row: the aligned float2 path over the planes, the move list as 64 words
__device__ __forceinline__ void copy_row(const float *__restrict__ src_x, const uint16_t *__restrict__ src_m, float *__restrict__ dst_x,
                                         uint16_t *__restrict__ dst_m, int t) {
    const float2 *src = (const float2 *)src_x;
    float2 *dst = (float2 *)dst_x;
    for (int i = t; i < XQ_STATE_FLOATS / 2; i += 256) dst[i] = src[i];
    if (t < XQ_MAXM / 2) ((uint32_t *)dst_m)[t] = ((const uint32_t *)src_m)[t];
}

// The mirrored gather: k_gather_rows with a decision per row.  rows[r] is a request ROW (slot K + j; the slot itself with K = 1);
// the bit's coordinates are read from the slot's state words as k_select left them, so the kernel takes nothing from the host and
// records into a graph.  A root request takes sims_done = 0 (GI_SIMS may hold the last move's count, or a reused root's visits).
__global__ __launch_bounds__(256) void k_gather_rows_mirror(Dev E, int K, int mode, const int32_t *__restrict__ n_live,
                                                            const int32_t *__restrict__ rows, const float *__restrict__ nn_in,
                                                            float *__restrict__ x, uint16_t *__restrict__ moves,
                                                            int32_t *__restrict__ counts) {
    const int r = blockIdx.x;
    if (r >= *n_live) return;
    const int row = rows[r], t = threadIdx.x;
    const int slot = row / K, j = row - slot * K;
    const int32_t *gi = E.gi + (size_t)slot * GI_N;
    const uint32_t is_root = gi[GI_PHASE] == PH_WAIT_ROOT ? 1u : 0u;
    const int bit = mode == 1 ? eval_mirror_bit(E.cfg.seed, (uint32_t)E.cfg.rank, (uint32_t)slot, (uint32_t)gi[GI_GSEQ], (uint32_t)gi[GI_MC],
                                                is_root, is_root ? 0u : (uint32_t)gi[GI_SIMS], (uint32_t)j)
                              : 0;
    const int count = E.req[row];
    const float *src_x = nn_in + (size_t)row * XQ_STATE_FLOATS;
    const uint16_t *src_m = E.pmoves + (size_t)row * XQ_MAXM;
    float *dst_x = x + (size_t)r * XQ_STATE_FLOATS;
    uint16_t *dst_m = moves + (size_t)r * XQ_MAXM;
    if (bit) mirror_row(src_x, src_m, count, dst_x, dst_m, t);
    else copy_row(src_x, src_m, dst_x, dst_m, t);
    if (t == 0) counts[r] = count;
}

// xq_mirror_requests_batch: the same two row functions over n caller-owned rows, flags[r] != 0 mirrors
__global__ __launch_bounds__(256) void k_mirror_rows(const float *__restrict__ x, const uint16_t *__restrict__ moves,
                                                     const int32_t *__restrict__ counts, const uint8_t *__restrict__ flags, int n,
                                                     float *__restrict__ x_out, uint16_t *__restrict__ moves_out) {
    const int r = blockIdx.x, t = threadIdx.x;
    if (r >= n) return;
    const float *src_x = x + (size_t)r * XQ_STATE_FLOATS;
    const uint16_t *src_m = moves + (size_t)r * XQ_MAXM;
    float *dst_x = x_out + (size_t)r * XQ_STATE_FLOATS;
    uint16_t *dst_m = moves_out + (size_t)r * XQ_MAXM;
    if (flags[r] != 0) mirror_row(src_x, src_m, counts[r], dst_x, dst_m, t);
    else copy_row(src_x, src_m, dst_x, dst_m, t);
}

// Hand-back: packed row r's legal-move logits and value go to slot rows[r] of the slot-ordered buffers k_expand reads.
// One wave per row (two floats per lane), four rows per workgroup.
__global__ __launch_bounds__(256) void k_scatter_rows(const int32_t *__restrict__ n_live, const int32_t *__restrict__ rows,
                                                      const float *__restrict__ logits, const float *__restrict__ value,
                                                      float *__restrict__ slot_logits, float *__restrict__ slot_value, int G) {
    const int r = blockIdx.x * 4 + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= G || r >= *n_live) return;
    const int slot = rows[r];
    ((float2 *)(slot_logits + (size_t)slot * XQ_MAXM))[lane] = ((const float2 *)(logits + (size_t)r * XQ_MAXM))[lane];
    if (lane == 0) slot_value[slot] = value[r];
}

// Leaf batching (K > 1): k_compact over the G K request rows, slot-major.  Row slot K + j is live when the slot waits and
// j < its request-row count (1 for a root, the pending leaves for a leaf step); rows[r] is then that ROW's index, so
// k_gather_rows / k_scatter_rows serve it unchanged over the row-indexed request buffers.
__global__ __launch_bounds__(CPT) void k_compact_multi(Dev E, int K, int32_t *__restrict__ n_live, int32_t *__restrict__ rows) {
    block_compact(E, E.cfg.n_games * K, [&](int r) { return slot_waits(E, r / K) && (r % K) < E.gi[(size_t)(r / K) * GI_N + GI_NPEND]; },
                  n_live, rows);
}

// Per-model packed step of an arena-options engine (xq_engine_compact_arena): ONE pass of one workgroup compacts the waiting slots
// twice, into set 0 (the slots the NEW model searches for) and set 1 (the OLD model's).  Slot s is the new model's iff
// ((first_game + s) even) == (red is to move in the slot's real game).  Every waiting slot is in exactly one set.
struct ArSets {
    const ArHead *head;             // first_game is read on the device: the handle has no word left for it
    int32_t *n_live;                // [2]
    int32_t *rows[2];
    float *x[2];
    uint16_t *moves[2];
    int32_t *counts[2];
};

__device__ __forceinline__ bool slot_is_new_models(const Dev &E, int first_game, int slot) {
    return (((first_game + slot) & 1) == 0) == (E.gi[(size_t)slot * GI_N + GI_SIDE] == 1);
}

__global__ __launch_bounds__(CPT) void k_compact_arena(Dev E, ArSets A) {
    const int first_game = A.head->first_game;
    block_compact(E, E.cfg.n_games, [&](int s) { return slot_waits(E, s) && slot_is_new_models(E, first_game, s); }, A.n_live,
                  A.rows[0]);
    __syncthreads();                                  // block_compact's scan scratch is read by every thread before it is reused
    block_compact(E, E.cfg.n_games, [&](int s) { return slot_waits(E, s) && !slot_is_new_models(E, first_game, s); }, A.n_live + 1,
                  A.rows[1]);
}

ArSets make_ar_sets(const xq_engine *e) {
    const ArOff o = ar_off((size_t)e->cfg.n_games, (size_t)e->cfg.num_simulations);
    char *base = (char *)e->p[P_SQRT];
    ArSets a;
    a.head = (const ArHead *)(base + o.head);
    a.n_live = (int32_t *)(base + o.n_live);
    for (int m = 0; m < 2; ++m) {
        a.rows[m] = (int32_t *)(base + o.rows[m]); a.x[m] = (float *)(base + o.x[m]);
        a.moves[m] = (uint16_t *)(base + o.moves[m]); a.counts[m] = (int32_t *)(base + o.counts[m]);
    }
    return a;
}

}  // namespace

int xq::gather_packed_rows(const xq_engine *eng, const float *dev_nn_input, int rows, hipStream_t s) {
    if (mirror_of(eng)) {                              // the kernel follows the handle; every other engine launches k_gather_rows
        hipLaunchKernelGGL(k_gather_rows_mirror, dim3(rows), dim3(256), 0, s, make_dev(eng), leaves_of(eng), 1,
                           (const int32_t *)eng->p[P_PK_N], (const int32_t *)eng->p[P_PK_ROWS], dev_nn_input, (float *)eng->p[P_PK_X],
                           (uint16_t *)eng->p[P_PK_MOVES], (int32_t *)eng->p[P_PK_COUNTS]);
        return launch_status();
    }
    hipLaunchKernelGGL(k_gather_rows, dim3(rows), dim3(256), 0, s, make_dev(eng), (const int32_t *)eng->p[P_PK_N],
                       (const int32_t *)eng->p[P_PK_ROWS], dev_nn_input, (float *)eng->p[P_PK_X], (uint16_t *)eng->p[P_PK_MOVES],
                       (int32_t *)eng->p[P_PK_COUNTS]);
    return launch_status();
}

extern "C" {

int xq_engine_compact(const xq_engine *eng, const float *dev_nn_input, void *stream) {
    if (!eng || !dev_nn_input || eng->cfg.n_games <= 0) return XQ_ERR_ARG;
    const Dev d = make_dev(eng);
    hipStream_t s = (hipStream_t)stream;
    int32_t *n_live = (int32_t *)eng->p[P_PK_N], *rows = (int32_t *)eng->p[P_PK_ROWS];
    const int K = leaves_of(eng);
    if (K > 1) hipLaunchKernelGGL(k_compact_multi, dim3(1), dim3(CPT), 0, s, d, K, n_live, rows);
    else hipLaunchKernelGGL(k_compact, dim3(1), dim3(CPT), 0, s, d, n_live, rows);
    int rc = launch_status();
    if (rc != XQ_OK) return rc;
    return gather_packed_rows(eng, dev_nn_input, eng->cfg.n_games * K, s);
}

int xq_eval_mirror_bit_host(uint64_t seed, int rank, int slot, uint32_t game_seq, int ply, int is_root, int sims_done, int row) {
    if (rank < 0 || slot < 0 || ply < 0 || (is_root != 0 && is_root != 1) || sims_done < 0 || sims_done >= 16000 || row < 0 || row >= 64)
        return XQ_ERR_ARG;
    return eval_mirror_bit(seed, (uint32_t)rank, (uint32_t)slot, game_seq, (uint32_t)ply, (uint32_t)is_root, (uint32_t)sims_done,
                           (uint32_t)row);
}

int xq_mirror_action_host(int action) { return action < 0 || action >= XQ_ACTION_SPACE ? XQ_ERR_ARG : mirror_action(action); }

int xq_mirror_requests_batch(const float *dev_x, const uint16_t *dev_moves, const int32_t *dev_counts, const uint8_t *dev_flags, int n,
                             float *dev_x_out, uint16_t *dev_moves_out, void *stream) {
    if (n < 0) return XQ_ERR_ARG;
    if (n == 0) return XQ_OK;
    if (!dev_x || !dev_moves || !dev_counts || !dev_flags || !dev_x_out || !dev_moves_out) return XQ_ERR_ARG;
    if (dev_x_out == dev_x || dev_moves_out == dev_moves) return XQ_ERR_ARG;      // a mirrored row reads what it would overwrite
    if ((((uintptr_t)dev_x) | ((uintptr_t)dev_x_out)) & 7 || (((uintptr_t)dev_moves) | ((uintptr_t)dev_moves_out)) & 3)
        return XQ_ERR_ARG;                                                          // the copied rows take the aligned path
    hipLaunchKernelGGL(k_mirror_rows, dim3(n), dim3(256), 0, (hipStream_t)stream, dev_x, dev_moves, dev_counts, dev_flags, n, dev_x_out,
                       dev_moves_out);
    return launch_status();
}

int xq_engine_packed(const xq_engine *eng, xq_engine_packed_buffers *out) {
    if (!eng || !out) return XQ_ERR_ARG;
    out->n_live = (const int32_t *)eng->p[P_PK_N];
    out->rows = (const int32_t *)eng->p[P_PK_ROWS];
    out->x = (const float *)eng->p[P_PK_X];
    out->moves = (const uint16_t *)eng->p[P_PK_MOVES];
    out->counts = (const int32_t *)eng->p[P_PK_COUNTS];
    out->slot_logits = (const float *)eng->p[P_PK_LOGITS];
    out->slot_value = (const float *)eng->p[P_PK_VALUE];
    return XQ_OK;
}

int xq_engine_expand_packed(const xq_engine *eng, const float *dev_packed_logits, const float *dev_packed_value, void *stream) {
    if (!eng || !dev_packed_logits || !dev_packed_value || eng->cfg.n_games <= 0) return XQ_ERR_ARG;
    if (((uintptr_t)dev_packed_logits) & 7) return XQ_ERR_ARG;
    const int G = eng->cfg.n_games * leaves_of(eng);   // request rows
    float *slot_logits = (float *)eng->p[P_PK_LOGITS], *slot_value = (float *)eng->p[P_PK_VALUE];
    hipLaunchKernelGGL(k_scatter_rows, dim3((G + 3) / 4), dim3(256), 0, (hipStream_t)stream, (const int32_t *)eng->p[P_PK_N],
                       (const int32_t *)eng->p[P_PK_ROWS], dev_packed_logits, dev_packed_value, slot_logits, slot_value, G);
    const int rc = launch_status();
    if (rc != XQ_OK) return rc;
    return xq_engine_expand_legal(eng, slot_logits, slot_value, stream);
}

int xq_engine_arena_openings(const xq_engine *eng, const uint16_t **dev_actions, const int32_t **dev_counts) {
    if (!arena_of(eng) || !dev_actions || !dev_counts) return XQ_ERR_ARG;
    const ArOff o = ar_off((size_t)eng->cfg.n_games, (size_t)eng->cfg.num_simulations);
    *dev_actions = (const uint16_t *)((char *)eng->p[P_SQRT] + o.op_actions);
    *dev_counts = (const int32_t *)((char *)eng->p[P_SQRT] + o.op_counts);
    return XQ_OK;
}

int xq_engine_compact_arena(const xq_engine *eng, const float *dev_nn_input, void *stream) {
    if (!arena_of(eng) || !dev_nn_input) return XQ_ERR_ARG;
    const Dev d = make_dev(eng);
    const ArSets a = make_ar_sets(eng);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_compact_arena, dim3(1), dim3(CPT), 0, s, d, a);
    for (int m = 0; m < 2; ++m) {
        const int rc = launch_status();
        if (rc != XQ_OK) return rc;
        hipLaunchKernelGGL(k_gather_rows, dim3(eng->cfg.n_games), dim3(256), 0, s, d, (const int32_t *)(a.n_live + m),
                           (const int32_t *)a.rows[m], dev_nn_input, a.x[m], a.moves[m], a.counts[m]);
    }
    return launch_status();
}

int xq_engine_packed_arena(const xq_engine *eng, xq_engine_packed_buffers out[2]) {
    if (!arena_of(eng) || !out) return XQ_ERR_ARG;
    const ArSets a = make_ar_sets(eng);
    for (int m = 0; m < 2; ++m) {
        out[m].n_live = a.n_live + m; out[m].rows = a.rows[m]; out[m].x = a.x[m]; out[m].moves = a.moves[m];
        out[m].counts = a.counts[m];
        out[m].slot_logits = (const float *)eng->p[P_PK_LOGITS]; out[m].slot_value = (const float *)eng->p[P_PK_VALUE];
    }
    return XQ_OK;
}

int xq_engine_expand_packed_arena(const xq_engine *eng, const float *dev_logits_new, const float *dev_value_new,
                                  const float *dev_logits_old, const float *dev_value_old, void *stream) {
    if (!arena_of(eng) || !dev_logits_new || !dev_value_new || !dev_logits_old || !dev_value_old) return XQ_ERR_ARG;
    if ((((uintptr_t)dev_logits_new) | ((uintptr_t)dev_logits_old)) & 7) return XQ_ERR_ARG;
    const int G = eng->cfg.n_games;
    const ArSets a = make_ar_sets(eng);
    float *slot_logits = (float *)eng->p[P_PK_LOGITS], *slot_value = (float *)eng->p[P_PK_VALUE];
    const float *logits[2] = {dev_logits_new, dev_logits_old}, *value[2] = {dev_value_new, dev_value_old};
    for (int m = 0; m < 2; ++m) {
        hipLaunchKernelGGL(k_scatter_rows, dim3((G + 3) / 4), dim3(256), 0, (hipStream_t)stream, (const int32_t *)(a.n_live + m),
                           (const int32_t *)a.rows[m], logits[m], value[m], slot_logits, slot_value, G);
        const int rc = launch_status();
        if (rc != XQ_OK) return rc;
    }
    return xq_engine_expand_legal(eng, slot_logits, slot_value, stream);
}

}  // extern "C"
