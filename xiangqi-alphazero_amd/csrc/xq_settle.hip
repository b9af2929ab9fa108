// xq_settle.hip -- the settled-move cutoff of the decided searches (map: xq_engine.hip).
//
// Settled-move cutoff (xq_engine_settle, opt-in): a search whose move is played at temperature 0 -- an arena game's, or a
// search-only engine's under MCTS.get_action(temperature=0) -- is decided by the FIRST MAXIMUM of the root's visit counts in move
// order (slot_arena_move; np.argmax over the visits).  k_settle, launched ahead of the select kernel, ends such a search as soon
// as the simulations that are left cannot move that maximum.  A slot in PH_SEARCH with sims_done < budget = S is settled when
//
//   nch == 1                          the move is forced, or
//   n1 - n2 > budget - sims_done      n1 the largest child visit count, n2 the second largest counted with multiplicity: a tie for
//                                     first has lead 0.  Strict: at lead == remaining the runner-up can still tie, and with a lower
//                                     index it would then be the first maximum.
//
// One simulation adds one visit to one root child, so after the remaining r simulations every other child stands at most at
// n2 + r < n1 and the leader at no less than n1: the first maximum stays where it is.  The rule is exact -- no move changes.
//
// A settled slot: an arena engine (manual_moves = 2) gets gi[GI_SIMS] = budget, and the select kernel that follows in the same step
// takes its own sims_done >= budget branch (slot_arena_move; the next root request resets the word); a search-only engine
// (manual_moves = 1) gets gi[GI_PHASE] = PH_HOLD and keeps GI_SIMS, so read_root's sims_done tells what was really run.
//
// One wavefront per slot, WAVES_PER_WG slots per workgroup.  A wave whose slot is not searching exits after one load -- at arena
// scale almost all of them, the slots wait for an evaluation.  The others load the child counts, at most two per lane
// (XQ_MAXM = 128), and reduce them with shuffles and two ballots.  No LDS, no scratch, no atomics; lane 0 alone stores.  Its own
// kernel for the reason k_start_pool is one: the select instances have no register to spare, and so no existing kernel's
// arguments or code change.
//
// Counters: caller-owned uint64[n_games][2], row s written by slot s's wave only -- [0] searches settled, [1] simulations not run.
#include "xq_engine_state.cuh"

namespace {

constexpr int WAVES_PER_WG = 4;

// the maximum of v over the wave, wave-uniform
__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off));
    return __builtin_amdgcn_readfirstlane(v);
}

__global__ __launch_bounds__(64 * WAVES_PER_WG) void k_settle(Dev E, unsigned long long *__restrict__ counters) {
    const int slot = blockIdx.x * WAVES_PER_WG + (int)(threadIdx.x >> 6);
    if (slot >= E.cfg.n_games) return;
    const int lane = threadIdx.x & 63;
    int32_t *gi = E.gi + (size_t)slot * GI_N;
    if (__builtin_amdgcn_readfirstlane(gi[GI_PHASE]) != PH_SEARCH) return;
    const int budget = E.cfg.num_simulations;
    const int sims_done = __builtin_amdgcn_readfirstlane(gi[GI_SIMS]);
    if (sims_done >= budget) return;                                // the select kernel ends this search by itself
    const size_t nb = (size_t)slot * E.node_cap;
    const int nch = __builtin_amdgcn_readfirstlane((int)(E.tM[nb] & XQ_CNT_MASK));
    const int first = __builtin_amdgcn_readfirstlane(E.tC[nb]);
    if (nch < 1 || nch > XQ_MAXM || first < 0 || first > E.node_cap - nch) return;   // never expected: a searched root is expanded
    bool settled = nch == 1;
    if (!settled) {
        const int32_t *n = E.tN + nb + first;
        const int a = lane < nch ? n[lane] : -1;                    // counts are >= 0: -1 never leads and never ties
        int b = -1;
        if (nch > 64) b = lane + 64 < nch ? n[lane + 64] : -1;      // wave-uniform: the second load only where there is one
        const int n1 = wave_max(max(a, b));
        const int leaders = __popcll(__ballot(a == n1)) + __popcll(__ballot(b == n1));
        int n2 = n1;                                                // a tie for first: the runner-up stands level
        if (leaders == 1) n2 = wave_max(max(a == n1 ? -1 : a, b == n1 ? -1 : b));
        settled = n1 - n2 > budget - sims_done;
    }
    if (!settled) return;
    if (lane == 0) {
        if (E.cfg.manual_moves == 2) gi[GI_SIMS] = budget;
        else gi[GI_PHASE] = PH_HOLD;
        counters[(size_t)slot * 2] += 1ull;
        counters[(size_t)slot * 2 + 1] += (unsigned long long)(budget - sims_done);
    }
}

}  // namespace

extern "C" {

int xq_engine_settle(const xq_engine *eng, unsigned long long *dev_counters, void *stream) {
    if (!eng || !dev_counters || eng->cfg.n_games <= 0 || eng->cfg.num_simulations <= 0 || !eng->p[P_GI] || !eng->p[P_TN]) return XQ_ERR_ARG;
    if (eng->cfg.manual_moves != 1 && eng->cfg.manual_moves != 2) return XQ_ERR_ARG;    // self-play: the counts are the target
    if (leaves_of(eng) > 1) return XQ_ERR_ARG;                      // leaf batching: pending descents are no part of N yet
    if (solver_of(eng)) return XQ_ERR_ARG;                          // rule 5 plays the first maximum of adjusted counts, not of N
    if (gumbel_of(eng) || cap_of(eng) || forced_of(eng) || reuse_of(eng)) return XQ_ERR_ARG;
    hipLaunchKernelGGL(k_settle, dim3((eng->cfg.n_games + WAVES_PER_WG - 1) / WAVES_PER_WG), dim3(64 * WAVES_PER_WG), 0,
                       (hipStream_t)stream, make_dev(eng), dev_counters);
    return launch_status();
}

}  // extern "C"
