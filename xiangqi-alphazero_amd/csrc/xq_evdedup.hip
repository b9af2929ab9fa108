// xq_evdedup.hip -- the request dedup of the packed self-play step (map: xq_engine.hip).
//
// Request dedup (xq_evdedup_*, opt-in): within ONE step, slots that ask for the same position are answered by one evaluated
// row.  A request's output depends only on its 15 input planes and each evaluator kernel's arithmetic for a row is independent
// of its batch position (the evaluation cache's two premises, xq_evcache.hip), so the row a slot is handed is bit-identical to
// the one it would have computed.  Nothing is kept across steps.
//
//   key    : the 12 words of xq_evkey.cuh, stored per waiting slot.
//   table  : T = the smallest power of two >= max(16, 4 n_slots) int32 buckets, "empty" = INT32_MAX.  Every waiting slot does
//            atomicMin(&table[hash(key) & (T - 1)], slot): the one atomic of this file.  The minimum does not depend on the
//            order of the atomics, so eager, replayed and repeated runs agree.
//   rep    : with m = the bucket's minimum, slot s is represented by m when m != s, all 12 key words agree and the legal-move
//            counts agree; otherwise by itself.  Different keys in one bucket are a "collision", equal keys under different
//            counts a "mismatch" (never expected): both only cost the merge, never the answer.
//   empty  : k_compact_unique, the last kernel behind the table's only reader (k_dedup_resolve), stores INT32_MAX back into
//            the bucket of every waiting slot.  Chosen over a recorded memset of the table: no node is added to the step's
//            graph, at most n_slots words are written instead of 4 n_slots, and xq_dedup_rows_batch, which has no
//            scatter kernel, leaves the table empty by the same code.  The three kernels are launched by ONE entry point
//            (xq_engine_compact_unique / xq_dedup_rows_batch), so a table is never left between them.
//
// Counters per slot (requests, merged, collisions, mismatches), summed on the host as the cache's are.
#include "xq_engine_state.cuh"
#include "xq_evkey.cuh"

#pragma clang fp contract(off)

namespace {

enum Dd : int { DD_TABLE = 0, DD_KEYS, DD_BUCKET, DD_REP, DD_ROWOF, DD_STATS, DD_SINK, DD_N };
enum DdSt : int { DDS_REQUESTS = 0, DDS_MERGED, DDS_COLLISIONS, DDS_MISMATCHES, DDS_N = 4 };
constexpr int32_t DD_EMPTY = 0x7FFFFFFF;
constexpr int DD_MAX_SLOTS = 1 << 24;

struct DdDev {
    int T;
    int32_t *table;                   // [T] the lowest waiting slot of the bucket, DD_EMPTY between steps
    uint32_t *keys;                   // [n_slots][12] the key of every waiting slot's request
    int32_t *bucket;                  // [n_slots] its bucket
    int32_t *rep;                     // [n_slots] its representative (the object's own DD_REP, or the caller's array)
    int32_t *rowof;                   // [n_slots] the packed row of every representative
    unsigned long long *stats;        // [n_slots][DDS_N]
};

// Who asks: an engine's slots by k_expand's own predicate, caller-owned rows (flags != NULL) by their live flags.  Uniform
// over the launch.
__device__ __forceinline__ bool dd_waits(const Dev &E, const int32_t *__restrict__ flags, int s) {
    return flags ? flags[s] != 0 : slot_waits(E, s);
}

// Keys: one wave per slot, four per workgroup; a slot that does not wait exits after one load.
__global__ __launch_bounds__(256) void k_dedup_keys(Dev E, DdDev D, const int32_t *__restrict__ flags, const float *__restrict__ x, int n) {
    const int slot = blockIdx.x * 4 + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (slot >= n) return;
    if (!dd_waits(E, flags, slot)) return;
    uint32_t key[EC_KEYW];
    wave_evkey(x + (size_t)slot * XQ_STATE_FLOATS, key);
    if (lane == 0) {
        uint4 *k = (uint4 *)(D.keys + (size_t)slot * EC_KEYW);
        k[0] = make_uint4(key[0], key[1], key[2], key[3]);
        k[1] = make_uint4(key[4], key[5], key[6], key[7]);
        k[2] = make_uint4(key[8], key[9], key[10], key[11]);
        const int b = (int)(evkey_hash(key) & (uint32_t)(D.T - 1));
        D.bucket[slot] = b;
        atomicMin(&D.table[b], (int32_t)slot);
    }
}

// Resolve: one wave per waiting slot s; lane w < 12 compares word w of the two keys.
__global__ __launch_bounds__(256) void k_dedup_resolve(Dev E, DdDev D, const int32_t *__restrict__ flags, const int32_t *__restrict__ req,
                                                       int n) {
    const int slot = blockIdx.x * 4 + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (slot >= n) return;
    if (!dd_waits(E, flags, slot)) return;
    int m = D.table[D.bucket[slot]];
    if (m < 0 || m >= n) m = slot;                                  // never expected: the slot's own atomic bounds the minimum
    bool differ = false;
    if (lane < EC_KEYW) differ = D.keys[(size_t)m * EC_KEYW + lane] != D.keys[(size_t)slot * EC_KEYW + lane];
    const bool same_key = __ballot(differ) == 0ull;
    if (lane == 0) {
        const bool same_count = req[m] == req[slot];
        const bool merged = m != slot && same_key && same_count;
        D.rep[slot] = merged ? m : slot;
        unsigned long long *st = D.stats + (size_t)slot * DDS_N;
        st[DDS_REQUESTS] += 1;
        st[DDS_MERGED] += merged ? 1 : 0;
        st[DDS_COLLISIONS] += (m != slot && !same_key) ? 1 : 0;
        st[DDS_MISMATCHES] += (m != slot && same_key && !same_count) ? 1 : 0;
    }
}

// Stable compaction of the representatives: k_compact with the predicate "waits and represents itself", into the packed
// step's own live count and row map.  Then, by the same workgroup: the packed row of every representative, and the buckets
// of this step's requests back to "empty".
__global__ __launch_bounds__(CPT) void k_compact_unique(Dev E, DdDev D, const int32_t *__restrict__ flags, int n, int32_t *n_live,
                                                        int32_t *rows) {
    block_compact(E, n, [&](int s) { return dd_waits(E, flags, s) && D.rep[s] == s; }, n_live, rows);
    __syncthreads();                                                // rows[] and *n_live are this workgroup's own stores
    const int total = *n_live;
    for (int r = threadIdx.x; r < total; r += CPT) D.rowof[rows[r]] = r;
    for (int s = threadIdx.x; s < n; s += CPT)
        if (dd_waits(E, flags, s)) D.table[D.bucket[s]] = DD_EMPTY;
}

// Hand-back: one wave per waiting slot, four per workgroup; the slot's row is its representative's packed row.
__global__ __launch_bounds__(256) void k_scatter_dedup(Dev E, DdDev D, const float *__restrict__ logits, const float *__restrict__ value,
                                                       float *__restrict__ slot_logits, float *__restrict__ slot_value) {
    const int G = E.cfg.n_games;
    const int slot = blockIdx.x * 4 + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (slot >= G) return;
    if (!slot_waits(E, slot)) return;
    const int m = D.rep[slot];
    if (m < 0 || m >= G) return;                                    // never expected
    const int r = D.rowof[m];
    if (r < 0 || r >= G) return;                                    // never expected
    ((float2 *)(slot_logits + (size_t)slot * XQ_MAXM))[lane] = ((const float2 *)(logits + (size_t)r * XQ_MAXM))[lane];
    if (lane == 0) slot_value[slot] = value[r];
}

struct DdLayout {
    size_t off[DD_N];
    size_t total;
};

bool dedup_args_ok(long long n_slots) { return n_slots > 0 && n_slots <= DD_MAX_SLOTS; }

int dedup_table_size(long long n_slots) {
    long long t = 16;
    while (t < 4 * n_slots) t <<= 1;
    return (int)t;
}

DdLayout make_dd_layout(size_t G) {
    DdLayout l;
    memset(&l, 0, sizeof(l));
    size_t o = 0;
    auto put = [&](int id, size_t bytes) { l.off[id] = o; o = align_up(o + bytes); };
    put(DD_TABLE, (size_t)dedup_table_size((long long)G) * 4);
    put(DD_KEYS, G * EC_KEYW * 4);            // everything from here on is zeroed by xq_evdedup_init
    put(DD_BUCKET, G * 4);
    put(DD_REP, G * 4);
    put(DD_ROWOF, G * 4);
    put(DD_STATS, G * DDS_N * 8);
    put(DD_SINK, ST_N * 8);                   // xq_dedup_rows_batch: where block_compact's rows counter goes without an engine
    l.total = o;
    return l;
}

bool dedup_ok(const xq_evdedup *d) {
    return d && dedup_args_ok(d->n_slots) && d->table_size == dedup_table_size(d->n_slots) && d->p[DD_TABLE] && d->p[DD_SINK];
}

DdDev make_dddev(const xq_evdedup *d) {
    DdDev v;
    v.T = d->table_size;
    v.table = (int32_t *)d->p[DD_TABLE]; v.keys = (uint32_t *)d->p[DD_KEYS]; v.bucket = (int32_t *)d->p[DD_BUCKET];
    v.rep = (int32_t *)d->p[DD_REP]; v.rowof = (int32_t *)d->p[DD_ROWOF]; v.stats = (unsigned long long *)d->p[DD_STATS];
    return v;
}

// an engine the dedup can serve: one request row per slot, gathered as it is, one model
bool dedup_engine_ok(const xq_evdedup *d, const xq_engine *eng) {
    if (!dedup_ok(d) || !eng || eng->cfg.n_games <= 0 || d->n_slots != eng->cfg.n_games) return false;
    if (leaves_of(eng) > 1) return false;             // leaf batching: a slot asks for several rows
    if (mirror_of(eng)) return false;                 // evaluation mirror: equal planes are evaluated under different orientations
    if (eng->cfg.manual_moves == 2) return false;     // arena games: two models answer
    return true;
}

// keys -> resolve -> compact over n rows; E carries the predicate's state words (an engine) or only the counter sink
int launch_dedup(const Dev &E, const DdDev &D, const int32_t *flags, const int32_t *req, const float *x, int n, int32_t *n_live,
                 int32_t *rows, hipStream_t s) {
    hipLaunchKernelGGL(k_dedup_keys, dim3((n + 3) / 4), dim3(256), 0, s, E, D, flags, x, n);
    int rc = launch_status();
    if (rc != XQ_OK) return rc;
    hipLaunchKernelGGL(k_dedup_resolve, dim3((n + 3) / 4), dim3(256), 0, s, E, D, flags, req, n);
    rc = launch_status();
    if (rc != XQ_OK) return rc;
    hipLaunchKernelGGL(k_compact_unique, dim3(1), dim3(CPT), 0, s, E, D, flags, n, n_live, rows);
    return launch_status();
}

}  // namespace

extern "C" {

size_t xq_evdedup_bytes(int n_slots) {
    if (!dedup_args_ok(n_slots)) return 0;
    return make_dd_layout((size_t)n_slots).total;
}

int xq_evdedup_init(xq_evdedup *dedup, int n_slots, void *dev_mem, size_t bytes, void *stream) {
    if (!dedup || !dedup_args_ok(n_slots) || !dev_mem || ((uintptr_t)dev_mem & 255)) return XQ_ERR_ARG;
    const DdLayout l = make_dd_layout((size_t)n_slots);
    if (bytes < l.total) return XQ_ERR_WORKSPACE;
    memset(dedup, 0, sizeof(*dedup));
    dedup->n_slots = n_slots;
    dedup->table_size = dedup_table_size(n_slots);
    for (int i = 0; i < DD_N; ++i) dedup->p[i] = (char *)dev_mem + l.off[i];
    hipStream_t s = (hipStream_t)stream;
    XQ_TRY(hipMemsetD32Async((hipDeviceptr_t)dev_mem, DD_EMPTY, (size_t)dedup->table_size, s));   // every bucket empty
    XQ_TRY(hipMemsetAsync((char *)dev_mem + l.off[DD_KEYS], 0, l.total - l.off[DD_KEYS], s));
    return XQ_OK;
}

int xq_engine_compact_unique(const xq_evdedup *dedup, const xq_engine *eng, const float *dev_nn_input, void *stream) {
    if (!dedup_engine_ok(dedup, eng) || !dev_nn_input) return XQ_ERR_ARG;
    const Dev E = make_dev(eng);
    hipStream_t s = (hipStream_t)stream;
    const int G = eng->cfg.n_games;
    const int rc = launch_dedup(E, make_dddev(dedup), nullptr, E.req, dev_nn_input, G, (int32_t *)eng->p[P_PK_N],
                                (int32_t *)eng->p[P_PK_ROWS], s);
    if (rc != XQ_OK) return rc;
    return gather_packed_rows(eng, dev_nn_input, G, s);
}

int xq_engine_expand_dedup(const xq_evdedup *dedup, const xq_engine *eng, const float *dev_packed_logits, const float *dev_packed_value,
                           void *stream) {
    if (!dedup_engine_ok(dedup, eng) || !dev_packed_logits || !dev_packed_value || (((uintptr_t)dev_packed_logits) & 7))
        return XQ_ERR_ARG;
    const int G = eng->cfg.n_games;
    float *slot_logits = (float *)eng->p[P_PK_LOGITS], *slot_value = (float *)eng->p[P_PK_VALUE];
    hipLaunchKernelGGL(k_scatter_dedup, dim3((G + 3) / 4), dim3(256), 0, (hipStream_t)stream, make_dev(eng), make_dddev(dedup),
                       dev_packed_logits, dev_packed_value, slot_logits, slot_value);
    const int rc = launch_status();
    if (rc != XQ_OK) return rc;
    return xq_engine_expand_legal(eng, slot_logits, slot_value, stream);
}

int xq_evdedup_stats_read(const xq_evdedup *dedup, xq_evdedup_stats *host_out, void *stream) {
    if (!dedup_ok(dedup) || !host_out) return XQ_ERR_ARG;
    const size_t n = (size_t)dedup->n_slots * DDS_N;
    unsigned long long *h = (unsigned long long *)malloc(n * sizeof(unsigned long long));
    if (!h) return XQ_ERR_ARG;
    int rc = xq::check(hipMemcpyAsync(h, dedup->p[DD_STATS], n * sizeof(unsigned long long), hipMemcpyDeviceToHost,
                                      (hipStream_t)stream));
    if (rc == XQ_OK) rc = xq::check(hipStreamSynchronize((hipStream_t)stream));
    if (rc == XQ_OK) {
        unsigned long long sum[DDS_N] = {0};
        for (size_t i = 0; i < n; ++i) sum[i % DDS_N] += h[i];
        memset(host_out, 0, sizeof(*host_out));
        host_out->requests = sum[DDS_REQUESTS]; host_out->merged = sum[DDS_MERGED];
        host_out->collisions = sum[DDS_COLLISIONS]; host_out->mismatches = sum[DDS_MISMATCHES];
    }
    free(h);
    return rc;
}

int xq_evdedup_bucket_host(const uint32_t *key12, int table_size) {
    if (!key12 || table_size <= 0 || (table_size & (table_size - 1))) return XQ_ERR_ARG;
    return (int)(evkey_hash(key12) & (uint32_t)(table_size - 1));
}

int xq_dedup_rows_batch(const float *dev_x, const int32_t *dev_counts, const int32_t *dev_live_flags, int n, const xq_evdedup *dedup,
                        int32_t *dev_rep_out, int32_t *dev_rows_out, int32_t *dev_n_out, void *stream) {
    if (n < 0) return XQ_ERR_ARG;
    if (!dedup_ok(dedup) || n > dedup->n_slots || !dev_n_out) return XQ_ERR_ARG;
    if (n > 0 && (!dev_x || !dev_counts || !dev_live_flags || !dev_rep_out || !dev_rows_out)) return XQ_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    if (n == 0) return xq::check(hipMemsetAsync(dev_n_out, 0, 4, s));
    Dev E;
    memset(&E, 0, sizeof(E));
    E.cfg.n_games = n;
    E.stats = (unsigned long long *)dedup->p[DD_SINK];
    DdDev D = make_dddev(dedup);
    D.rep = dev_rep_out;
    return launch_dedup(E, D, dev_live_flags, dev_counts, dev_x, n, dev_n_out, dev_rows_out, s);
}

}  // extern "C"
