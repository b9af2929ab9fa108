// xq_evcache.hip -- the evaluation cache of the packed self-play step (map: xq_engine.hip).
//
// Evaluation cache (xq_evcache_*, opt-in): per slot K entries in W-way sets (W = min(4, K)) holding the legal-move logits and
// value the network returned for a position.  A request's output depends only on its 15 input planes (board + side to move;
// the ordered legal moves are a function of them) and each evaluator kernel's arithmetic for a row is independent of its
// batch position, so a cached row is bit-identical to a recomputed one.  Private to a slot: no sharing, no atomics.
//
//   key   : the 12 words of xq_evkey.cuh (90 squares x 4 bits and the side to move), injective over k_select's planes.
//   set   : a hash of the key picks the set; a hit needs all 12 key words, the current generation and the count to match.
//   stamp : the slot's probe clock at insert / last hit; the victim is an entry of an older generation, else the oldest stamp
//           (lowest way on ties).
#include "xq_engine_state.cuh"
#include "xq_evkey.cuh"

#pragma clang fp contract(off)

namespace {

enum Ec : int { EC_GEN = 0, EC_CLOCK, EC_HIT, EC_SKEY, EC_STATS, EC_EGEN, EC_STAMP, EC_COUNT, EC_VALUE, EC_KEY, EC_LOGITS, EC_N };
enum EcSt : int { ECS_PROBES = 0, ECS_HITS, ECS_INSERTS, ECS_EVICTIONS, ECS_MISMATCHES, ECS_N = 8 };

struct EvDev {
    int K, W, sets;
    uint32_t *gen;                    // the current generation (device word: no host value is recorded into a graph)
    uint32_t *clock;                  // [G] probes of the slot so far
    int32_t *hit;                     // [G] 1: this step's request was answered by the cache
    uint32_t *skey;                   // [G][12] the key probed this step (commit's input)
    unsigned long long *stats;        // [G][ECS_N]
    uint32_t *egen, *stamp;           // [G K]
    int32_t *count;                   // [G K]
    float *value;                     // [G K]
    uint32_t *key;                    // [G K][12]
    float *logits;                    // [G K][XQ_MAXM]
};

EvDev make_evdev(const xq_evcache *c) {
    EvDev d;
    d.K = c->entries; d.W = c->ways; d.sets = c->sets;
    d.gen = (uint32_t *)c->p[EC_GEN]; d.clock = (uint32_t *)c->p[EC_CLOCK]; d.hit = (int32_t *)c->p[EC_HIT];
    d.skey = (uint32_t *)c->p[EC_SKEY]; d.stats = (unsigned long long *)c->p[EC_STATS];
    d.egen = (uint32_t *)c->p[EC_EGEN]; d.stamp = (uint32_t *)c->p[EC_STAMP]; d.count = (int32_t *)c->p[EC_COUNT];
    d.value = (float *)c->p[EC_VALUE]; d.key = (uint32_t *)c->p[EC_KEY]; d.logits = (float *)c->p[EC_LOGITS];
    return d;
}

// Probe: one wave per slot, four per workgroup; slots that are not waiting exit.  Lane w < W tests way w of the key's set.
// A hit writes the entry's logits / value into the slot-ordered hand-back rows k_expand reads (as k_scatter_rows does for
// evaluated rows) and refreshes its stamp; every probe records its key for k_evcache_commit.
__global__ __launch_bounds__(256) void k_evcache_probe(Dev E, EvDev C, const float *__restrict__ nn_in,
                                                       float *__restrict__ slot_logits, float *__restrict__ slot_value) {
    const int slot = blockIdx.x * 4 + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (slot >= E.cfg.n_games) return;
    const int ph = E.gi[(size_t)slot * GI_N + GI_PHASE];
    if (ph != PH_WAIT_ROOT && ph != PH_WAIT_LEAF) return;
    uint32_t key[EC_KEYW];
    wave_evkey(nn_in + (size_t)slot * XQ_STATE_FLOATS, key);
    const int count = E.req[slot];
    const uint32_t gen = *C.gen, clock = C.clock[slot] + 1u;
    const size_t e0 = (size_t)slot * C.K + (size_t)(evkey_hash(key) & (uint32_t)(C.sets - 1)) * C.W;
    bool kmatch = false, same = false;
    if (lane < C.W) {
        const size_t e = e0 + lane;
        kmatch = C.egen[e] == gen && key_eq(C.key + e * EC_KEYW, key);
        same = kmatch && C.count[e] == count;
    }
    const unsigned long long km = __ballot(kmatch), sm = __ballot(same);
    const int way = sm ? __ffsll((long long)sm) - 1 : -1;
    if (way >= 0) {
        const size_t e = e0 + way;
        ((float2 *)(slot_logits + (size_t)slot * XQ_MAXM))[lane] = ((const float2 *)(C.logits + e * XQ_MAXM))[lane];
        if (lane == 0) { slot_value[slot] = C.value[e]; C.stamp[e] = clock; }
    }
    if (lane == 0) {
        uint4 *sk = (uint4 *)(C.skey + (size_t)slot * EC_KEYW);
        sk[0] = make_uint4(key[0], key[1], key[2], key[3]);
        sk[1] = make_uint4(key[4], key[5], key[6], key[7]);
        sk[2] = make_uint4(key[8], key[9], key[10], key[11]);
        C.hit[slot] = way >= 0 ? 1 : 0;
        C.clock[slot] = clock;
        unsigned long long *st = C.stats + (size_t)slot * ECS_N;
        st[ECS_PROBES] += 1;
        st[ECS_HITS] += way >= 0 ? 1 : 0;
        st[ECS_MISMATCHES] += (way < 0 && km) ? 1 : 0;     // key and generation match, count differs: never expected
    }
}

// Stable compaction of the misses (xq_engine_compact_misses): k_compact with the predicate "waiting and not a hit".
__global__ __launch_bounds__(CPT) void k_compact_misses(Dev E, const int32_t *__restrict__ hit, int32_t *__restrict__ n_live,
                                                        int32_t *__restrict__ rows) {
    block_compact(E, E.cfg.n_games, [&](int s) { return slot_waits(E, s) && hit[s] == 0; }, n_live, rows);
}

// Commit: one wave per evaluated (packed) row r < n_live; the row's slot inserts the key it probed with this step.  One
// insert per slot and step, so the victim choice is deterministic without atomics.
__global__ __launch_bounds__(256) void k_evcache_commit(EvDev C, int G, const int32_t *__restrict__ n_live,
                                                        const int32_t *__restrict__ rows, const int32_t *__restrict__ counts,
                                                        const float *__restrict__ logits, const float *__restrict__ value) {
    const int r = blockIdx.x * 4 + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= G || r >= *n_live) return;
    const int slot = rows[r];
    const uint4 *sk = (const uint4 *)(C.skey + (size_t)slot * EC_KEYW);
    const uint4 k0 = sk[0], k1 = sk[1], k2 = sk[2];
    const uint32_t key[EC_KEYW] = {k0.x, k0.y, k0.z, k0.w, k1.x, k1.y, k1.z, k1.w, k2.x, k2.y, k2.z, k2.w};
    const uint32_t gen = *C.gen, clock = C.clock[slot];
    const size_t e0 = (size_t)slot * C.K + (size_t)(evkey_hash(key) & (uint32_t)(C.sets - 1)) * C.W;
    int victim = 0;
    bool evict = true;
    uint32_t oldest = 0xFFFFFFFFu;
    for (int w = 0; w < C.W; ++w) {
        const size_t e = e0 + w;
        if (C.egen[e] != gen) { victim = w; evict = false; break; }
        const uint32_t st = C.stamp[e];
        if (st < oldest) { oldest = st; victim = w; }
    }
    const size_t e = e0 + victim;
    ((float2 *)(C.logits + e * XQ_MAXM))[lane] = ((const float2 *)(logits + (size_t)r * XQ_MAXM))[lane];
    if (lane == 0) {
        uint4 *ek = (uint4 *)(C.key + e * EC_KEYW);
        ek[0] = k0; ek[1] = k1; ek[2] = k2;
        C.value[e] = value[r];
        C.count[e] = counts[r];
        C.egen[e] = gen;
        C.stamp[e] = clock;
        unsigned long long *st = C.stats + (size_t)slot * ECS_N;
        st[ECS_INSERTS] += 1;
        st[ECS_EVICTIONS] += evict ? 1 : 0;
    }
}

// Invalidation: a new generation; entries of older ones never hit and are the first victims.
__global__ void k_evcache_invalidate(uint32_t *gen) {
    if (threadIdx.x == 0) *gen += 1u;
}

struct EcLayout {
    size_t off[EC_N];
    size_t total;
};

bool evcache_args_ok(long long n_slots, long long k) { return n_slots > 0 && k > 0 && (k & (k - 1)) == 0 && k <= (1 << 20); }

EcLayout make_ec_layout(size_t G, size_t K) {
    EcLayout l;
    memset(&l, 0, sizeof(l));
    const size_t GK = G * K;
    size_t o = 0;
    auto put = [&](int id, size_t bytes) { l.off[id] = o; o = align_up(o + bytes); };
    put(EC_GEN, 4);
    put(EC_CLOCK, G * 4);
    put(EC_HIT, G * 4);
    put(EC_SKEY, G * EC_KEYW * 4);
    put(EC_STATS, G * ECS_N * 8);
    put(EC_EGEN, GK * 4);            // everything up to here is zeroed by xq_evcache_init
    put(EC_STAMP, GK * 4);
    put(EC_COUNT, GK * 4);
    put(EC_VALUE, GK * 4);
    put(EC_KEY, GK * EC_KEYW * 4);
    put(EC_LOGITS, GK * XQ_MAXM * 4);
    l.total = o;
    return l;
}

bool evcache_ok(const xq_evcache *c) {
    return c && evcache_args_ok(c->n_slots, c->entries) && c->ways > 0 && c->sets > 0 && c->ways * c->sets == c->entries &&
           c->p[EC_GEN] && c->p[EC_LOGITS];
}

}  // namespace

extern "C" {

size_t xq_evcache_bytes(int n_slots, int entries_per_slot) {
    if (!evcache_args_ok(n_slots, entries_per_slot)) return 0;
    return make_ec_layout((size_t)n_slots, (size_t)entries_per_slot).total;
}

int xq_evcache_init(xq_evcache *cache, int n_slots, int entries_per_slot, void *dev_mem, size_t bytes, void *stream) {
    if (!cache || !evcache_args_ok(n_slots, entries_per_slot) || !dev_mem || ((uintptr_t)dev_mem & 255)) return XQ_ERR_ARG;
    const EcLayout l = make_ec_layout((size_t)n_slots, (size_t)entries_per_slot);
    if (bytes < l.total) return XQ_ERR_WORKSPACE;
    memset(cache, 0, sizeof(*cache));
    cache->n_slots = n_slots;
    cache->entries = entries_per_slot;
    cache->ways = entries_per_slot < 4 ? entries_per_slot : 4;
    cache->sets = entries_per_slot / cache->ways;
    for (int i = 0; i < EC_N; ++i) cache->p[i] = (char *)dev_mem + l.off[i];
    hipStream_t s = (hipStream_t)stream;
    XQ_TRY(hipMemsetAsync(dev_mem, 0, l.off[EC_COUNT], s));   // generation 0, clocks, flags, counters, entry generations, stamps
    hipLaunchKernelGGL(k_evcache_invalidate, dim3(1), dim3(64), 0, s, (uint32_t *)cache->p[EC_GEN]);   // generation 1
    return launch_status();
}

int xq_evcache_hit_flags(const xq_evcache *cache, const int32_t **dev_hit) {
    if (!evcache_ok(cache) || !dev_hit) return XQ_ERR_ARG;
    *dev_hit = (const int32_t *)cache->p[EC_HIT];
    return XQ_OK;
}

int xq_evcache_probe(const xq_evcache *cache, const xq_engine *eng, const float *dev_nn_input, void *stream) {
    if (!eng || leaves_of(eng) > 1) return XQ_ERR_ARG;            // the cache serves one request row per slot
    if (!evcache_ok(cache) || !dev_nn_input || eng->cfg.n_games <= 0 || cache->n_slots != eng->cfg.n_games)
        return XQ_ERR_ARG;
    const int G = eng->cfg.n_games;
    hipLaunchKernelGGL(k_evcache_probe, dim3((G + 3) / 4), dim3(256), 0, (hipStream_t)stream, make_dev(eng), make_evdev(cache),
                       dev_nn_input, (float *)eng->p[P_PK_LOGITS], (float *)eng->p[P_PK_VALUE]);
    return launch_status();
}

int xq_engine_compact_misses(const xq_engine *eng, const float *dev_nn_input, const int32_t *dev_hit_flags, void *stream) {
    if (!eng || !dev_nn_input || !dev_hit_flags || eng->cfg.n_games <= 0 || leaves_of(eng) > 1) return XQ_ERR_ARG;
    if (mirror_of(eng)) return XQ_ERR_ARG;            // a hit would return whichever orientation was evaluated first
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_compact_misses, dim3(1), dim3(CPT), 0, s, make_dev(eng), dev_hit_flags, (int32_t *)eng->p[P_PK_N],
                       (int32_t *)eng->p[P_PK_ROWS]);
    int rc = launch_status();
    if (rc != XQ_OK) return rc;
    return gather_packed_rows(eng, dev_nn_input, eng->cfg.n_games, s);
}

int xq_evcache_commit(const xq_evcache *cache, const xq_engine *eng, const float *dev_packed_logits,
                      const float *dev_packed_value, void *stream) {
    if (!evcache_ok(cache) || !eng || leaves_of(eng) > 1 || !dev_packed_logits || !dev_packed_value || eng->cfg.n_games <= 0 ||
        cache->n_slots != eng->cfg.n_games || (((uintptr_t)dev_packed_logits) & 7))
        return XQ_ERR_ARG;
    const int G = eng->cfg.n_games;
    hipLaunchKernelGGL(k_evcache_commit, dim3((G + 3) / 4), dim3(256), 0, (hipStream_t)stream, make_evdev(cache), G,
                       (const int32_t *)eng->p[P_PK_N], (const int32_t *)eng->p[P_PK_ROWS], (const int32_t *)eng->p[P_PK_COUNTS],
                       dev_packed_logits, dev_packed_value);
    return launch_status();
}

int xq_evcache_invalidate(const xq_evcache *cache, void *stream) {
    if (!evcache_ok(cache)) return XQ_ERR_ARG;
    hipLaunchKernelGGL(k_evcache_invalidate, dim3(1), dim3(64), 0, (hipStream_t)stream, (uint32_t *)cache->p[EC_GEN]);
    return launch_status();
}

int xq_evcache_stats_read(const xq_evcache *cache, xq_evcache_stats *host_out, void *stream) {
    if (!evcache_ok(cache) || !host_out) return XQ_ERR_ARG;
    const size_t n = (size_t)cache->n_slots * ECS_N;
    unsigned long long *h = (unsigned long long *)malloc(n * sizeof(unsigned long long));
    if (!h) return XQ_ERR_ARG;
    int rc = xq::check(hipMemcpyAsync(h, cache->p[EC_STATS], n * sizeof(unsigned long long), hipMemcpyDeviceToHost,
                                      (hipStream_t)stream));
    if (rc == XQ_OK) rc = xq::check(hipStreamSynchronize((hipStream_t)stream));
    if (rc == XQ_OK) {
        unsigned long long sum[ECS_N] = {0};
        for (size_t i = 0; i < n; ++i) sum[i % ECS_N] += h[i];
        memset(host_out, 0, sizeof(*host_out));
        host_out->probes = sum[ECS_PROBES]; host_out->hits = sum[ECS_HITS]; host_out->inserts = sum[ECS_INSERTS];
        host_out->evictions = sum[ECS_EVICTIONS]; host_out->mismatches = sum[ECS_MISMATCHES];
    }
    free(h);
    return rc;
}

int xq_evcache_key_host(const float *host_planes, uint32_t *host_out12) {
    if (!host_planes || !host_out12) return XQ_ERR_ARG;
    for (int w = 0; w < EC_KEYW; ++w) host_out12[w] = 0;
    for (int sq = 0; sq < 90; ++sq) host_out12[sq >> 3] |= evkey_nibble(host_planes, sq) << (4 * (sq & 7));
    host_out12[90 >> 3] |= evkey_side(host_planes) << (4 * (90 & 7));
    return XQ_OK;
}

}  // extern "C"
