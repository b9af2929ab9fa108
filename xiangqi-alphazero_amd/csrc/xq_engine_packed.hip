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
