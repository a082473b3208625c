// exchange_plan.h -- the send/receive collectives of a sharded server (piehip_rccl.cpp: piehip_rccl_scatter_query,
// piehip_rccl_exchange_accumulators, piehip_gather_results; DESIGN.md section 6 "Query slices across processes"): who sends what to
// whom, from where, to where, and in which order the transfers of a rank are posted inside its one group call -- the one place that
// knows the transfers and the rule of the ranks' ranges.  Nothing of HIP or RCCL in here, so that
// tests/exchange_plan_check.cpp can carry the plan out with memcpy, match every send with its receive and run every rank's list over
// channels without any buffering.
//
// Rank r of G holds the units [u_lo_r, u_hi_r) (the rule of piehip_query_slice; unit u = h L + l is limb l of inner hash function h)
// and runs the product chain of the bin layers [bin_lo_r, bin_hi_r) (the rule of piehip_rccl_bin_slice).  Nobody exchanges a range:
// every rank derives every rank's from (K, L, b, G).
//
//   scatter   the root holds the whole queries.  It lays every unit's pieces into a staging area in unit order, per query
//             idx[K L][E][2][N] and minus[K L][2][N]; the units of a rank are then one contiguous range of each.  Per query and
//             receiver: one transfer of the index slice [u_n][E][2][N], one of the minus slice [u_n][2][N], straight into the
//             receiver's slice inputs.  A rank without units takes no part; the root's own units are a device copy.
//   exchange  rank s has acc_slice[b][nq][u_n_s][2][N] of its units for ALL bin layers; rank d needs the rows [bin_lo_d, bin_hi_d)
//             of everybody's.  b is outermost, so that is one contiguous block per (s, d).  d receives it into a staging buffer
//             at offset bin_n_d nq 2N u_lo_s: block after block in unit order, each [bin_n_d][nq][u_n_s][2][N].  Its own rows never
//             leave acc_slice.  A transfer with u_n_s = 0 or bin_n_d = 0 does not exist, on either side.
//   gather    rank r has the result rows [bin_n_r][nq][ncomp][rl][N] of its bin layers: ncomp components on rl limbs each, 2 and L
//             unless a setting of the handles says otherwise (plan_row_words; the ranks have agreed on it: piehip_rccl_agree_rows).
//             The root posts one receive per peer with layers, in ascending rank, straight into the rows at bin_lo_r of its list
//             [b][nq][ncomp][rl][N]; such a peer posts one send of its result buffer.  A rank without layers posts nothing; the root's
//             own rows are a device copy outside the plan.
//
// Posting order.  A rank walks its peers in ascending rank; towards a higher-ranked peer it posts its send first and then its
// receive, towards a lower-ranked peer its receive first and then its send.  RCCL does not care about the order inside a group; a
// transport that executes a group's operations one after the other with blocking sends does.  Write every transfer as the pair
// (lower rank, higher rank) it connects, the lower rank's send before the higher rank's: the order above posts every rank's transfers
// in ascending order of that one total order, and both ends of a transfer agree on its place in it.  The least transfer not yet
// completed is therefore next on both of its ranks, so it can complete: no rank ever waits for ever, even where a send only
// completes once its receive has been reached.  In the scatter all transfers leave one rank, which walks the receivers in
// ascending rank and the queries in order; every receiver posts its own in that same order.  In the gather every transfer has the
// root at one end and each peer has one: the root's ascending walk over its peers is ascending in that total order.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace piehip {

struct ExchangeShape {
    uint32_t K, L, b, nq, N, E;   // (E: ciphertexts per unit of the index matrix; the scatter's sizes only)
    // a result ciphertext as the gather moves it: components, and limbs per component (0: all L)
    uint32_t ncomp = 2, row_limbs = 0;
};

// [lo, hi) of `total` things for rank r of G: contiguous, sizes differ by at most one (piehip_query_slice, piehip_rccl_bin_slice)
inline void plan_range(uint32_t total, int G, int r, uint32_t *lo, uint32_t *hi)
{
    *lo = (uint32_t)((uint64_t)total * (uint64_t)r / (uint64_t)G);
    *hi = (uint32_t)((uint64_t)total * ((uint64_t)r + 1) / (uint64_t)G);
}
inline void plan_unit_range(const ExchangeShape &s, int G, int r, uint32_t *lo, uint32_t *hi) { plan_range(s.K * s.L, G, r, lo, hi); }
inline void plan_bin_range(const ExchangeShape &s, int G, int r, uint32_t *lo, uint32_t *hi) { plan_range(s.b, G, r, lo, hi); }

// what a transfer's offset counts from
enum PlanBuffer {
    PLAN_STAGE_INDEX,   // the root's staging area of query q, idx[K L][E][2][N]
    PLAN_STAGE_MINUS,   // ... minus[K L][2][N]
    PLAN_OWN_INDEX,     // the rank's own index slice of query q, [u_n][E][2][N]
    PLAN_OWN_MINUS,     // ... minus slice [u_n][2][N]
    PLAN_ACC_SLICE,     // the rank's acc_slice[b][nq][u_n][2][N]
    PLAN_ACC_STAGE,     // the rank's staging buffer of received blocks, bin_n nq 2N K L words
    PLAN_RESULT_ROWS,   // the result rows of this rank, [bin_n][nq][ncomp][rl][N]
    PLAN_GATHERED       // the gathered list at the root, [b][nq][ncomp][rl][N]
};

// one transfer as one of its two ranks sees it; offsets and sizes in words
struct PlanTransfer {
    bool send;
    int peer;
    PlanBuffer buf;
    uint32_t q;      // the query (scatter; 0 in the exchange and the gather)
    size_t off, words;
};

// words of the exchange's staging buffer on a rank with bin_n bin layers
inline size_t plan_acc_stage_words(const ExchangeShape &s, uint32_t bin_n) { return (size_t)bin_n * s.nq * 2 * s.N * s.K * s.L; }

// the transfers rank r posts in piehip_rccl_scatter_query, in posting order
inline std::vector<PlanTransfer> scatter_plan(const ExchangeShape &s, int G, int r, int root)
{
    std::vector<PlanTransfer> out;
    const size_t mw = 2 * (size_t)s.N, iw = mw * s.E;   // words per unit: minus slice, index slice
    for (int d = 0; d < G; d++) {
        if (d == root || (r != root && d != r)) continue;
        uint32_t lo, hi;
        plan_unit_range(s, G, d, &lo, &hi);
        if (hi == lo) continue;
        for (uint32_t q = 0; q < s.nq; q++) {
            if (r == root) {
                out.push_back({true, d, PLAN_STAGE_INDEX, q, lo * iw, (hi - lo) * iw});
                out.push_back({true, d, PLAN_STAGE_MINUS, q, lo * mw, (hi - lo) * mw});
            } else {
                out.push_back({false, root, PLAN_OWN_INDEX, q, 0, (hi - lo) * iw});
                out.push_back({false, root, PLAN_OWN_MINUS, q, 0, (hi - lo) * mw});
            }
        }
    }
    return out;
}

// the transfers rank r posts in piehip_rccl_exchange_accumulators, in posting order
inline std::vector<PlanTransfer> exchange_plan(const ExchangeShape &s, int G, int r)
{
    std::vector<PlanTransfer> out;
    uint32_t u_lo, u_hi, bin_lo, bin_hi;
    plan_unit_range(s, G, r, &u_lo, &u_hi);
    plan_bin_range(s, G, r, &bin_lo, &bin_hi);
    const size_t un = u_hi - u_lo, bn = bin_hi - bin_lo, row = (size_t)s.nq * 2 * s.N;   // words per bin layer and unit
    for (int p = 0; p < G; p++) {
        if (p == r) continue;
        uint32_t pu_lo, pu_hi, pb_lo, pb_hi;
        plan_unit_range(s, G, p, &pu_lo, &pu_hi);
        plan_bin_range(s, G, p, &pb_lo, &pb_hi);
        const size_t pun = pu_hi - pu_lo, pbn = pb_hi - pb_lo;
        const PlanTransfer snd = {true, p, PLAN_ACC_SLICE, 0, pb_lo * row * un, pbn * row * un};
        const PlanTransfer rcv = {false, p, PLAN_ACC_STAGE, 0, bn * row * pu_lo, bn * row * pun};
        const PlanTransfer first = p > r ? snd : rcv, second = p > r ? rcv : snd;
        if (first.words) out.push_back(first);
        if (second.words) out.push_back(second);
    }
    return out;
}

// words of one bin layer's result rows: its nq result ciphertexts of ncomp components on rl limbs
static inline size_t plan_row_words(const ExchangeShape &s) { return (size_t)s.nq * s.ncomp * (s.row_limbs ? s.row_limbs : s.L) * s.N; }

// the transfers rank r posts in piehip_gather_results, in posting order (static: the library's dynamic symbol table stays as it was)
static inline std::vector<PlanTransfer> gather_plan(const ExchangeShape &s, int G, int r, int root)
{
    std::vector<PlanTransfer> out;
    const size_t row = plan_row_words(s);
    for (int p = 0; p < G; p++) {
        if (p == root || (r != root && p != r)) continue;
        uint32_t lo, hi;
        plan_bin_range(s, G, p, &lo, &hi);
        if (hi == lo) continue;
        out.push_back(r == root ? PlanTransfer{false, p, PLAN_GATHERED, 0, lo * row, (hi - lo) * row}
                                : PlanTransfer{true, root, PLAN_RESULT_ROWS, 0, 0, (hi - lo) * row});
    }
    return out;
}

// One entry per unit of the table the placement launch reads (kernels.hpp, PlaceSource): where the chain side of rank r finds unit u
// after the exchange.  own: in its own acc_slice, whose rows start at bin layer 0; otherwise in the staging buffer at `off`, whose rows
// start at the rank's first layer.  u_lo, u_n: the unit range of the block.
struct PlanUnitSource {
    bool own;
    size_t off;
    uint32_t u_lo, u_n;
};
inline PlanUnitSource plan_unit_source(const ExchangeShape &s, int G, int r, uint32_t u)
{
    uint32_t bin_lo, bin_hi;
    plan_bin_range(s, G, r, &bin_lo, &bin_hi);
    for (int p = 0; p < G; p++) {
        uint32_t lo, hi;
        plan_unit_range(s, G, p, &lo, &hi);
        if (u < lo || u >= hi) continue;
        if (p == r) return {true, 0, lo, hi - lo};
        return {false, (size_t)(bin_hi - bin_lo) * s.nq * 2 * s.N * lo, lo, hi - lo};
    }
    return {false, 0, 0, 0};
}

}  // namespace piehip
