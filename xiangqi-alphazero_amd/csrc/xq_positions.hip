// xq_positions.hip -- is a board a position the rules code can safely run on?  (include/xq_hip.h, xq_positions_check_batch)
// One 64-lane wavefront per position, four positions per 256-thread workgroup, the board in LDS carved per wave, no workgroup
// barrier (xq_rules.cuh), no atomics, no scratch.  Lane l owns squares l and l + 64; counts are popcounts of ballots.
#include "xq_tools.cuh"

#pragma clang fp contract(off)

using namespace xq;

namespace {

struct PosLds {
    __attribute__((aligned(16))) int8_t board[XQ_BS];
    MoveGenLds mg;
    uint16_t moves[XQ_MAXM];
};

// a piece of colour `colour` (1 red, -1 black) and kind 2 .. 7 on (r, c): may it ever stand there?  Black is red mirrored.
__device__ __forceinline__ bool may_stand(int kind, int colour, int r, int c) {
    const int rr = colour == 1 ? r : 9 - r;           // the row as red sees it
    if (kind == 2) return (rr == 1 && c == 4) || ((rr == 0 || rr == 2) && (c == 3 || c == 5));
    if (kind == 3) return ((rr == 0 || rr == 4) && (c == 2 || c == 6)) || (rr == 2 && (c == 0 || c == 4 || c == 8));
    if (kind == 7) return rr >= 5 || (rr >= 3 && (c & 1) == 0);
    return true;
}

__global__ __launch_bounds__(64 * WPW) void k_positions_check(const int8_t *__restrict__ boards, const int8_t *__restrict__ side, int n,
                                                              uint8_t *__restrict__ status) {
    __shared__ PosLds Ls[WPW];
    XQ_WAVE_ITEM(n)
    PosLds &L = Ls[wv];
    const int lane = lane_id();
    wave_load_board(boards + (size_t)i * 90, L.board);
    wave_sync();
    const int sd = __builtin_amdgcn_readfirstlane((int)side[i]);
    const bool has1 = lane + 64 < 90;
    const int sq1 = has1 ? lane + 64 : 0;
    const int p0 = L.board[lane], p1 = has1 ? L.board[sq1] : 0;
    auto count = [&](int v) { return __popcll(__ballot(p0 == v)) + __popcll(__ballot(p1 == v)); };
    int st = 0;
    // bit 1: a square outside -7 .. 7, a side outside {1, -1}
    if (__ballot(p0 < -7 || p0 > 7 || p1 < -7 || p1 > 7) != 0ull || (sd != 1 && sd != -1)) st |= 1;
    // bit 2: exactly one king of each colour, inside its palace
    {
        auto out_of_palace = [](int p, int sq) {
            if (p != 1 && p != -1) return false;
            const int r = sq / 9, c = sq % 9;
            return c < 3 || c > 5 || (p == 1 ? r > 2 : r < 7);
        };
        if (count(1) != 1 || count(-1) != 1 || __ballot(out_of_palace(p0, lane) || out_of_palace(p1, sq1)) != 0ull) st |= 2;
    }
    if (st) {                                          // the rules code is not run on such a board: the later bits stay 0
        if (lane == 0) status[i] = (uint8_t)st;
        return;
    }
    // bit 4: a piece where it can never stand, or more of a kind than a set has
    {
        auto misplaced = [](int p, int sq) {
            const int kind = p < 0 ? -p : p;
            return kind >= 2 && !may_stand(kind, p > 0 ? 1 : -1, sq / 9, sq % 9);
        };
        bool bad = __ballot(misplaced(p0, lane) || misplaced(p1, sq1)) != 0ull;
#pragma unroll
        for (int kind = 2; kind <= 7; ++kind) {
            const int most = kind == 7 ? 5 : 2;
            bad = bad || count(kind) > most || count(-kind) > most;
        }
        if (bad) st |= 4;
    }
    // bit 8: the side not to move is in check (facing kings included: the ray scan meets the other king first)
    if (wave_in_check(L.board, -sd)) st |= 8;
    // bit 16: the side to move has no legal move
    int ovf = 0;
    if (wave_movegen(L.board, sd, L.mg, L.moves, &ovf) == 0) st |= 16;
    if (lane == 0) status[i] = (uint8_t)st;
}

}  // namespace

extern "C" {

int xq_positions_check_batch(const int8_t *dev_boards, const int8_t *dev_side, int n, uint8_t *dev_status, void *stream) {
    if (n < 0 || (n > 0 && (!dev_boards || !dev_side || !dev_status))) return XQ_ERR_ARG;
    if (n == 0) return XQ_OK;
    hipLaunchKernelGGL(k_positions_check, dim3((n + WPW - 1) / WPW), dim3(64 * WPW), 0, (hipStream_t)stream, dev_boards, dev_side, n,
                       dev_status);
    return launch_status();
}

}  // extern "C"
