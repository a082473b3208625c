// The plan of the scatter and the exchange of query slices across ranks and of the final gather of the results (csrc/exchange_plan.h, the
// only include of the library here), on the CPU, for every G in 1..9, every root and five shapes (K, L, b, nq) that include G > K L and G > b:
//   (a) the unit and bin ranges tile [0, K L) and [0, b); they are printed ("range ..." lines) for tests/test_exchange_plan.py, which
//       compares them with piehip_query_slice and piehip_rccl_bin_slice of the built library;
//   (b) every send has exactly one matching receive of the same size, and a transfer with u_n_s = 0 or bin_n_d = 0 is on neither side
//       (the gather: a rank without bin layers posts nothing, nobody posts anything towards it);
//   (c) every rank executes its list strictly in order over channels WITHOUT any buffering -- a send completes only when the peer's
//       next operation is the matching receive -- and every rank finishes: the scatter, the exchange, the gather, the exchange behind
//       the scatter and the gather behind both;
//   (d) the plan carried out with memcpy between buffers of exactly the stated sizes (the sanitizers this is also built with see a
//       block outside either) on arrays whose words encode (row, query, unit, component, n): every word of every destination's
//       [rows][nq][K L][2][N] is written exactly once, with the right value; the scatter likewise for every receiver's slice inputs,
//       the gather for the root's [b][nq][2][L][N], where the root's own rows are copied in place of the device copy.
// `exchange_plan_check naive` posts all sends first, then all receives, for G = 2 and reports that simulation (c) then deadlocks:
// the check can fail.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../nested_hashing_psi_amd/csrc/exchange_plan.h"

using namespace piehip;
typedef uint64_t u64;
typedef uint32_t u32;

static const u64 UNTOUCHED = ~(u64)0;
typedef std::vector<std::vector<PlanTransfer>> Lists;   // per rank, in posting order

// (c): true when every rank reaches the end of its list
static bool completes(const Lists &lists)
{
    const int G = (int)lists.size();
    std::vector<size_t> at(G, 0);
    for (bool moved = true; moved;) {
        moved = false;
        for (int r = 0; r < G; r++) {
            if (at[r] == lists[r].size()) continue;
            const PlanTransfer &t = lists[r][at[r]];
            if (!t.send || at[t.peer] == lists[t.peer].size()) continue;
            const PlanTransfer &o = lists[t.peer][at[t.peer]];
            if (o.send || o.peer != r) continue;   // the peer is not at the matching receive: the send stays blocked
            if (o.words != t.words) return printf("rank %d sends %zu words, rank %d receives %zu\n", r, t.words, t.peer, o.words), false;
            at[r]++, at[t.peer]++, moved = true;
        }
    }
    for (int r = 0; r < G; r++)
        if (at[r] != lists[r].size()) return false;
    return true;
}

// (b): the k-th send of s to d is the k-th receive of d from s, same size; nothing of zero words; returns the number of transfers or -1
static long matched(const Lists &lists)
{
    const int G = (int)lists.size();
    long n = 0;
    for (int s = 0; s < G; s++)
        for (int d = 0; d < G; d++) {
            std::vector<size_t> snd, rcv;
            for (const PlanTransfer &t : lists[s])
                if (t.send && t.peer == d) snd.push_back(t.words);
            for (const PlanTransfer &t : lists[d])
                if (!t.send && t.peer == s) rcv.push_back(t.words);
            if (snd != rcv) return printf("sends of %d to %d and receives of %d from %d differ\n", s, d, d, s), -1;
            if (s == d && !snd.empty()) return printf("rank %d sends to itself\n", s), -1;
            for (size_t w : snd)
                if (!w) return printf("empty transfer %d -> %d\n", s, d), -1;
            n += (long)snd.size();
        }
    return n;
}

// the receive of `d` that matches send number k (among those to d) of s
static const PlanTransfer *receive_of(const Lists &lists, int s, int d, size_t k)
{
    for (const PlanTransfer &t : lists[d])
        if (!t.send && t.peer == s && !k--) return &t;
    return nullptr;
}

static u64 acc_word(const ExchangeShape &sh, u32 beta, u32 q, u32 u, u32 c, u32 n)
{
    return 1 + ((((u64)beta * sh.nq + q) * sh.K * sh.L + u) * 2 + c) * sh.N + n;
}
static u64 query_word(const ExchangeShape &sh, int piece, u32 q, u32 u, size_t w)   // w: word within the unit's [cts][2][N]
{
    return 1 + (((u64)q * 2 + piece) * sh.K * sh.L + u) * ((u64)sh.E * 2 * sh.N) + w;
}

static int check_exchange(const ExchangeShape &sh, int G)
{
    const u32 KL = sh.K * sh.L, N = sh.N;
    Lists lists(G);
    std::vector<u32> u_lo(G), u_hi(G), b_lo(G), b_hi(G);
    for (int r = 0; r < G; r++) {
        lists[r] = exchange_plan(sh, G, r);
        plan_unit_range(sh, G, r, &u_lo[r], &u_hi[r]);
        plan_bin_range(sh, G, r, &b_lo[r], &b_hi[r]);
    }
    long want = 0;
    for (int s = 0; s < G; s++)
        for (int d = 0; d < G; d++) want += s != d && u_hi[s] > u_lo[s] && b_hi[d] > b_lo[d];
    if (matched(lists) != want) return printf("exchange: %ld transfers expected\n", want), 1;
    if (!completes(lists)) return printf("exchange: a rank never finishes its list\n"), 1;
    // (d)
    std::vector<std::vector<u64>> acc(G), stage(G);
    std::vector<std::vector<int>> written(G);
    for (int r = 0; r < G; r++) {
        const u32 un = u_hi[r] - u_lo[r];
        acc[r].resize((size_t)sh.b * sh.nq * un * 2 * N);
        for (u32 beta = 0; beta < sh.b; beta++)
            for (u32 q = 0; q < sh.nq; q++)
                for (u32 u = 0; u < un; u++)
                    for (u32 c = 0; c < 2; c++)
                        for (u32 n = 0; n < N; n++) acc[r][((((size_t)beta * sh.nq + q) * un + u) * 2 + c) * N + n] = acc_word(sh, beta, q, u_lo[r] + u, c, n);
        stage[r].assign(plan_acc_stage_words(sh, b_hi[r] - b_lo[r]), UNTOUCHED);
        written[r].assign(stage[r].size(), 0);
    }
    for (int s = 0; s < G; s++) {
        std::vector<size_t> k(G, 0);
        for (const PlanTransfer &t : lists[s]) {
            if (!t.send) continue;
            const PlanTransfer *o = receive_of(lists, s, t.peer, k[t.peer]++);
            if (!o || t.buf != PLAN_ACC_SLICE || o->buf != PLAN_ACC_STAGE) return printf("exchange: wrong buffer\n"), 1;
            if (t.off + t.words > acc[s].size() || o->off + o->words > stage[t.peer].size()) return printf("exchange: block out of bounds\n"), 1;
            memcpy(stage[t.peer].data() + o->off, acc[s].data() + t.off, t.words * sizeof(u64));
            for (size_t w = 0; w < t.words; w++) written[t.peer][o->off + w]++;
        }
    }
    for (int d = 0; d < G; d++) {
        const u32 bn = b_hi[d] - b_lo[d];
        std::vector<int> placed((size_t)bn * sh.nq * KL * 2 * N, 0);
        for (u32 u = 0; u < KL; u++) {
            const PlanUnitSource us = plan_unit_source(sh, G, d, u);
            if (!us.u_n || u < us.u_lo || u >= us.u_lo + us.u_n) return printf("exchange: unit %u has no source on rank %d\n", u, d), 1;
            const std::vector<u64> &buf = us.own ? acc[d] : stage[d];
            const size_t row0 = us.own ? (size_t)b_lo[d] * sh.nq : 0;
            for (u32 row = 0; row < bn * sh.nq; row++)
                for (u32 c = 0; c < 2; c++)
                    for (u32 n = 0; n < N; n++) {
                        const size_t at = us.off + (((row0 + row) * us.u_n + (u - us.u_lo)) * 2 + c) * N + n;
                        if (at >= buf.size()) return printf("exchange: placement reads out of bounds\n"), 1;
                        if (!us.own && written[d][at] != 1) return printf("exchange: a staged word was written %d times\n", written[d][at]), 1;
                        if (buf[at] != acc_word(sh, b_lo[d] + row / sh.nq, row % sh.nq, u, c, n)) return printf("exchange: wrong word\n"), 1;
                        placed[(((size_t)row * KL + u) * 2 + c) * N + n]++;
                    }
        }
        for (int p : placed)
            if (p != 1) return printf("exchange: a destination word was written %d times\n", p), 1;
        // nothing lands in the staging buffer where the rank's own units would be, and nothing twice
        size_t total = 0;
        for (int w : written[d]) total += (size_t)w;
        if (total != (size_t)bn * sh.nq * 2 * N * (KL - (u_hi[d] - u_lo[d]))) return printf("exchange: staged words\n"), 1;
    }
    return 0;
}

static int check_scatter(const ExchangeShape &sh, int G, int root)
{
    const u32 KL = sh.K * sh.L;
    const size_t cw[2] = {(size_t)sh.E * 2 * sh.N, 2 * (size_t)sh.N};   // words per unit: index slice, minus slice
    Lists lists(G), both(G);
    long want = 0;
    for (int r = 0; r < G; r++) {
        lists[r] = scatter_plan(sh, G, r, root);
        both[r] = lists[r];
        const std::vector<PlanTransfer> x = exchange_plan(sh, G, r);
        both[r].insert(both[r].end(), x.begin(), x.end());
        u32 lo, hi;
        plan_unit_range(sh, G, r, &lo, &hi);
        want += r != root && hi > lo ? 2 * sh.nq : 0;
    }
    if (matched(lists) != want) return printf("scatter: %ld transfers expected\n", want), 1;
    if (!completes(lists)) return printf("scatter: a rank never finishes its list\n"), 1;
    if (!completes(both)) return printf("scatter, then exchange: a rank never finishes its list\n"), 1;
    // (d): the root's staging area per query and piece, [K L][cts][2][N]
    std::vector<u64> stage[2];
    for (int p = 0; p < 2; p++) {
        stage[p].resize((size_t)sh.nq * KL * cw[p]);
        for (u32 q = 0; q < sh.nq; q++)
            for (u32 u = 0; u < KL; u++)
                for (size_t w = 0; w < cw[p]; w++) stage[p][((size_t)q * KL + u) * cw[p] + w] = query_word(sh, p, q, u, w);
    }
    for (int d = 0; d < G; d++) {
        if (d == root) continue;
        u32 lo, hi;
        plan_unit_range(sh, G, d, &lo, &hi);
        std::vector<u64> own[2];
        for (int p = 0; p < 2; p++) own[p].assign((size_t)sh.nq * (hi - lo) * cw[p], UNTOUCHED);
        size_t k = 0;
        for (const PlanTransfer &t : lists[root]) {
            if (!t.send || t.peer != d) continue;
            const PlanTransfer *o = receive_of(lists, root, d, k++);
            const int p = t.buf == PLAN_STAGE_INDEX ? 0 : 1;
            if (!o || (t.buf != PLAN_STAGE_INDEX && t.buf != PLAN_STAGE_MINUS) || o->buf != (p ? PLAN_OWN_MINUS : PLAN_OWN_INDEX) || o->q != t.q)
                return printf("scatter: wrong buffer or query\n"), 1;
            if (t.off + t.words > (size_t)KL * cw[p] || o->off + o->words > (size_t)(hi - lo) * cw[p]) return printf("scatter: out of bounds\n"), 1;
            u64 *dst = own[p].data() + (size_t)t.q * (hi - lo) * cw[p] + o->off;
            for (size_t w = 0; w < t.words; w++)
                if (dst[w] != UNTOUCHED) return printf("scatter: a word written twice\n"), 1;
            memcpy(dst, stage[p].data() + (size_t)t.q * KL * cw[p] + t.off, t.words * sizeof(u64));
        }
        for (int p = 0; p < 2; p++)
            for (u32 q = 0; q < sh.nq; q++)
                for (u32 u = lo; u < hi; u++)
                    for (size_t w = 0; w < cw[p]; w++)
                        if (own[p][((size_t)q * (hi - lo) + (u - lo)) * cw[p] + w] != query_word(sh, p, q, u, w)) return printf("scatter: wrong word\n"), 1;
    }
    return 0;
}

static int check_gather(const ExchangeShape &sh, int G, int root)
{
    const size_t row = (size_t)sh.nq * 2 * sh.L * sh.N;   // words per bin layer; word w of layer beta holds 1 + beta row + w
    Lists lists(G), all(G);
    std::vector<u32> b_lo(G), b_hi(G);
    long want = 0;
    for (int r = 0; r < G; r++) {
        lists[r] = gather_plan(sh, G, r, root);
        for (const std::vector<PlanTransfer> &x : {scatter_plan(sh, G, r, root), exchange_plan(sh, G, r), lists[r]}) all[r].insert(all[r].end(), x.begin(), x.end());
        plan_bin_range(sh, G, r, &b_lo[r], &b_hi[r]);
        want += r != root && b_hi[r] > b_lo[r];
    }
    if (matched(lists) != want) return printf("gather: %ld transfers expected\n", want), 1;
    if (!completes(lists)) return printf("gather: a rank never finishes its list\n"), 1;
    if (!completes(all)) return printf("scatter, exchange, then gather: a rank never finishes its list\n"), 1;
    // (d)
    std::vector<u64> gathered((size_t)sh.b * row, UNTOUCHED);
    std::vector<int> written(gathered.size(), 0);
    for (int s = 0; s < G; s++) {
        std::vector<u64> rows((size_t)(b_hi[s] - b_lo[s]) * row);   // the rank's result buffer, exactly its bin layers
        for (size_t w = 0; w < rows.size(); w++) rows[w] = 1 + (size_t)b_lo[s] * row + w;
        PlanTransfer own = {true, root, PLAN_RESULT_ROWS, 0, 0, rows.size()}, own_at = {false, s, PLAN_GATHERED, 0, (size_t)b_lo[s] * row, rows.size()};
        const PlanTransfer *t = &own, *o = &own_at;   // the root's own rows: the device copy's stand-in
        if (s != root && lists[s].size() != (rows.empty() ? 0u : 1u)) return printf("gather: rank %d posts %zu transfers\n", s, lists[s].size()), 1;
        if (rows.empty()) continue;
        if (s != root) {
            t = &lists[s][0], o = receive_of(lists, s, root, 0);
            if (!t->send || t->peer != root || t->buf != PLAN_RESULT_ROWS || !o || o->buf != PLAN_GATHERED) return printf("gather: wrong transfer or buffer\n"), 1;
        }
        if (t->off + t->words > rows.size() || o->off + o->words > gathered.size() || o->words != t->words) return printf("gather: block out of bounds\n"), 1;
        memcpy(gathered.data() + o->off, rows.data() + t->off, t->words * sizeof(u64));
        for (size_t w = 0; w < t->words; w++) written[o->off + w]++;
    }
    for (size_t w = 0; w < gathered.size(); w++)
        if (written[w] != 1 || gathered[w] != 1 + w) return printf("gather: word %zu written %d times or wrong\n", w, written[w]), 1;
    return 0;
}

// all sends, then all receives: what the posting order is there to avoid
static std::vector<PlanTransfer> naive_order(const std::vector<PlanTransfer> &plan)
{
    std::vector<PlanTransfer> out;
    for (int pass = 0; pass < 2; pass++)
        for (const PlanTransfer &t : plan)
            if (t.send == (pass == 0)) out.push_back(t);
    return out;
}

int main(int argc, char **argv)
{
    static const u32 shapes[5][4] = {{2, 2, 3, 1}, {2, 4, 14, 3}, {3, 2, 2, 2}, {2, 2, 5, 2}, {3, 3, 2, 1}};   // K, L, b, nq
    const u32 N = 4, E = 3;
    if (argc > 1 && !strcmp(argv[1], "naive")) {
        for (const u32 *s : shapes) {
            const ExchangeShape sh = {s[0], s[1], s[2], s[3], N, E};
            Lists lists(2);
            for (int r = 0; r < 2; r++) lists[r] = naive_order(exchange_plan(sh, 2, r));
            if (matched(lists) != 2) return printf("naive order: two transfers expected\n"), 1;
            if (completes(lists)) return printf("naive order completes: simulation (c) cannot fail\n"), 1;
        }
        printf("naive order deadlocks\n");
        return 0;
    }
    size_t cases = 0;
    for (const u32 *s : shapes) {
        const ExchangeShape sh = {s[0], s[1], s[2], s[3], N, E};
        for (int G = 1; G <= 9; G++) {
            u32 u_next = 0, b_next = 0;
            for (int r = 0; r < G; r++) {   // (a)
                u32 u_lo, u_hi, b_lo, b_hi;
                plan_unit_range(sh, G, r, &u_lo, &u_hi);
                plan_bin_range(sh, G, r, &b_lo, &b_hi);
                if (u_lo != u_next || u_hi < u_lo || b_lo != b_next || b_hi < b_lo) return printf("FAILED: the ranges do not tile (G %d rank %d)\n", G, r), 1;
                u_next = u_hi, b_next = b_hi;
                printf("range %d %u %u %u %d %u %u %u %u\n", G, sh.K, sh.L, sh.b, r, u_lo, u_hi, b_lo, b_hi);
            }
            if (u_next != sh.K * sh.L || b_next != sh.b) return printf("FAILED: the ranges do not cover (G %d)\n", G), 1;
            if (check_exchange(sh, G)) return printf("FAILED: K %u L %u b %u nq %u G %d\n", sh.K, sh.L, sh.b, sh.nq, G), 1;
            for (int root = 0; root < G; root++, cases++)
                if (check_scatter(sh, G, root) || check_gather(sh, G, root)) return printf("FAILED: K %u L %u b %u nq %u G %d root %d\n", sh.K, sh.L, sh.b, sh.nq, G, root), 1;
        }
    }
    printf("exchange plan ok: %zu cases\n", cases);
    return 0;
}
