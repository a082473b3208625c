// The plan of piehip_gather_results for result rows of any shape (csrc/exchange_plan.h, the only include of the library here), on the
// CPU: a result ciphertext of ncomp components on rl limbs, (ncomp, rl) in {(2, L), (2, 1), (3, L), (3, 2)} with L = 3, for G = 1..5,
// every root, b in {1, 4, 5, 14} and nq in {1, 3}:
//   (a) both ends of a transfer name the same word count, and every peer with bin layers has exactly one transfer with the root;
//   (b) the plan carried out with memcpy between buffers of exactly the stated sizes (the sanitizers this is also built with see a
//       block outside either): every word of the root's [b][nq][ncomp][rl][N] is written exactly once, and it is the word of the rank
//       that owns its layer -- words encode (owner, position in the owner's buffer); the root's own rows are copied in place of the
//       device copy;
//   (c) the default-initialised trailing members (ncomp = 2, row_limbs = 0: all L) give today's plan -- row words nq 2 L N, written
//       out here as the plan had it before rows had a shape -- transfer for transfer, and so does naming (2, L) outright.
// `gather_rows_plan_check wrong` lets one rank plan with another row shape than the root and reports that (a) then fails: the check
// can fail.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../nested_hashing_psi_amd/csrc/exchange_plan.h"

using namespace piehip;
typedef uint64_t u64;
typedef uint32_t u32;

static const u32 L = 3, N = 8, K = 2, E = 3;

static bool same_transfer(const PlanTransfer &a, const PlanTransfer &b)
{
    return a.send == b.send && a.peer == b.peer && a.buf == b.buf && a.q == b.q && a.off == b.off && a.words == b.words;
}

// today's plan: the gather as it was before ExchangeShape had a row shape
static std::vector<PlanTransfer> default_plan(u32 b, u32 nq, int G, int r, int root)
{
    std::vector<PlanTransfer> out;
    const size_t row = (size_t)nq * 2 * L * N;
    for (int p = 0; p < G; p++) {
        if (p == root || (r != root && p != r)) continue;
        u32 lo, hi;
        plan_range(b, G, p, &lo, &hi);
        if (hi == lo) continue;
        out.push_back(r == root ? PlanTransfer{false, p, PLAN_GATHERED, 0, lo * row, (hi - lo) * row}
                                : PlanTransfer{true, root, PLAN_RESULT_ROWS, 0, 0, (hi - lo) * row});
    }
    return out;
}

// shape_of(r): the shape rank r plans with (all the same unless the check is being shown to fail)
template <typename ShapeOf>
static int check(ShapeOf shape_of, int G, int root)
{
    const ExchangeShape sh = shape_of(root);
    const u32 rl = sh.row_limbs ? sh.row_limbs : sh.L;
    const size_t row = (size_t)sh.nq * sh.ncomp * rl * sh.N;
    if (plan_row_words(sh) != row) return printf("row words %zu, expected %zu\n", plan_row_words(sh), row), 1;
    std::vector<std::vector<PlanTransfer>> lists(G);
    for (int r = 0; r < G; r++) lists[r] = gather_plan(shape_of(r), G, r, root);
    std::vector<u64> gathered((size_t)sh.b * row, ~(u64)0);
    std::vector<int> written(gathered.size(), 0);
    size_t next_recv = 0;   // the root's receives come in ascending rank of the peers that have layers
    for (int s = 0; s < G; s++) {
        u32 lo, hi;
        plan_bin_range(sh, G, s, &lo, &hi);
        std::vector<u64> rows((size_t)(hi - lo) * row);   // the rank's result buffer: exactly its layers
        for (size_t w = 0; w < rows.size(); w++) rows[w] = ((u64)(s + 1) << 40) | w;
        if (s == root) {   // the device copy's stand-in
            if (!rows.empty()) memcpy(gathered.data() + (size_t)lo * row, rows.data(), rows.size() * sizeof(u64));
            for (size_t w = 0; w < rows.size(); w++) written[(size_t)lo * row + w]++;
            continue;
        }
        if (lists[s].size() != (rows.empty() ? 0u : 1u)) return printf("rank %d posts %zu transfers\n", s, lists[s].size()), 1;
        if (rows.empty()) continue;
        if (next_recv >= lists[root].size()) return printf("the root has no receive for rank %d\n", s), 1;
        const PlanTransfer &snd = lists[s][0], &rcv = lists[root][next_recv++];
        if (!snd.send || snd.peer != root || snd.buf != PLAN_RESULT_ROWS || rcv.send || rcv.peer != s || rcv.buf != PLAN_GATHERED)
            return printf("rank %d: wrong transfer, peer or buffer\n", s), 1;
        if (snd.words != rcv.words) return printf("rank %d sends %zu words, the root receives %zu\n", s, snd.words, rcv.words), 1;
        if (snd.off + snd.words > rows.size() || rcv.off + rcv.words > gathered.size()) return printf("rank %d: block out of bounds\n", s), 1;
        memcpy(gathered.data() + rcv.off, rows.data() + snd.off, snd.words * sizeof(u64));
        for (size_t w = 0; w < snd.words; w++) written[rcv.off + w]++;
    }
    if (next_recv != lists[root].size()) return printf("the root posts %zu receives, %zu have a sender\n", lists[root].size(), next_recv), 1;
    for (u32 beta = 0; beta < sh.b; beta++) {   // layer beta belongs to the rank whose range holds it
        int owner = -1;
        u32 olo = 0;
        for (int r = 0; r < G; r++) {
            u32 lo, hi;
            plan_bin_range(sh, G, r, &lo, &hi);
            if (beta >= lo && beta < hi) owner = r, olo = lo;
        }
        for (size_t w = 0; w < row; w++) {
            const size_t at = (size_t)beta * row + w;
            if (written[at] != 1 || gathered[at] != (((u64)(owner + 1) << 40) | ((size_t)(beta - olo) * row + w)))
                return printf("layer %u word %zu: written %d times or not rank %d's\n", beta, w, written[at], owner), 1;
        }
    }
    return 0;
}

int main(int argc, char **argv)
{
    const bool wrong = argc > 1 && !strcmp(argv[1], "wrong");
    const u32 rows[4][2] = {{2, L}, {2, 1}, {3, L}, {3, 2}}, bs[] = {1, 4, 5, 14}, nqs[] = {1, 3};
    if (wrong) {   // rank 1 of 2 kept all limbs, the root kept one: both ends no longer name one size
        auto shape_of = [&](int r) { return ExchangeShape{K, L, 5, 1, N, E, 2, r == 1 ? L : 1u}; };
        const int rc = check(shape_of, 2, 0);
        printf(rc ? "gather rows plan: ranks with different row shapes are caught\n" : "gather rows plan: NOT caught\n");
        return rc ? 0 : 1;
    }
    size_t cases = 0;
    for (u32 b : bs)
        for (u32 nq : nqs)
            for (int G = 1; G <= 5; G++)
                for (int root = 0; root < G; root++) {
                    for (const u32 *row : rows) {
                        const ExchangeShape sh = {K, L, b, nq, N, E, row[0], row[1]};
                        if (check([&](int) { return sh; }, G, root))
                            return printf("FAILED: ncomp %u limbs %u b %u nq %u G %d root %d\n", row[0], row[1], b, nq, G, root), 1;
                        cases++;
                    }
                    // (c)
                    const ExchangeShape dflt = {K, L, b, nq, N, E}, named = {K, L, b, nq, N, E, 2, L};
                    if (dflt.ncomp != 2 || dflt.row_limbs != 0) return printf("FAILED: the default shape is not (2, all limbs)\n"), 1;
                    for (int r = 0; r < G; r++) {
                        const std::vector<PlanTransfer> was = default_plan(b, nq, G, r, root), is = gather_plan(dflt, G, r, root), is2 = gather_plan(named, G, r, root);
                        bool eq = was.size() == is.size() && was.size() == is2.size();
                        for (size_t i = 0; eq && i < was.size(); i++) eq = same_transfer(was[i], is[i]) && same_transfer(was[i], is2[i]);
                        if (!eq) return printf("FAILED: the default shape's plan moved (b %u nq %u G %d root %d rank %d)\n", b, nq, G, root, r), 1;
                    }
                }
    printf("gather rows plan ok: %zu cases\n", cases);
    return 0;
}
