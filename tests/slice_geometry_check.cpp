// The copies that bring a slice input up (csrc/slice_geometry.h, the only include of the library here) against the definition of a
// slice, on the CPU: unit u of a handle's range [u_lo, u_hi) takes limb u % L of inner hash function u / L -- of the index matrix
// [K][E][halves][L][N] its E ciphertexts, of the minus element [halves][L][N] the one -- both halves of a ciphertext, or the c0 half
// alone when the piece is seeded.  The owned copy is [u_n][cts][2][N] either way; a seeded piece's c1 rows are not written.
//
// For every shape, every contiguous unit range (the empty ones too), both pieces, both source layouts, seeded and not: a whole query of
// distinct words, the planned copies performed row by row with memcpy between buffers of exactly the stated sizes (the sanitizers
// this is built with see a row outside either), and the outcome compared word for word.  Every destination row is written once.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../nested_hashing_psi_amd/csrc/slice_geometry.h"

using namespace piehip;
typedef uint64_t u64;
typedef uint32_t u32;

static const u64 UNTOUCHED = ~(u64)0;

static int check(u32 N, u32 L, u32 K, u32 E, SlicePiece piece, SliceLayout layout, bool seeded, u32 u_lo, u32 u_hi)
{
    const u32 cts = piece == SLICE_INDEX ? E : 1, halves = seeded ? 1 : 2, un = u_hi - u_lo;
    const u32 hfs = piece == SLICE_INDEX ? K : 1;   // one minus element for every inner hash function
    // the whole piece [hfs][cts][halves][L][N]: distinct words
    std::vector<u64> whole((size_t)hfs * cts * halves * L * N);
    for (size_t i = 0; i < whole.size(); i++) whole[i] = 1000 + i;
    auto word = [&](u32 u, u32 j, u32 c, u32 n) {
        const u32 h = piece == SLICE_INDEX ? u / L : 0;
        return whole[((((size_t)h * cts + j) * halves + c) * L + u % L) * N + n];
    };
    // the slice by the definition, as the owned copy holds it and as a caller cuts it
    std::vector<u64> want((size_t)un * cts * 2 * N, UNTOUCHED), cut((size_t)un * cts * halves * N);
    for (u32 u = u_lo; u < u_hi; u++)
        for (u32 j = 0; j < cts; j++)
            for (u32 c = 0; c < halves; c++)
                for (u32 n = 0; n < N; n++) {
                    want[((((size_t)(u - u_lo) * cts + j) * 2) + c) * N + n] = word(u, j, c, n);
                    cut[((((size_t)(u - u_lo) * cts + j) * halves) + c) * N + n] = word(u, j, c, n);
                }
    const std::vector<u64> &src = layout == SLICE_CUT ? cut : whole;
    std::vector<u64> got((size_t)un * cts * 2 * N, UNTOUCHED);
    std::vector<int> written((size_t)un * cts * 2, 0);
    const u32 copies = layout == SLICE_WHOLE ? un : 1;
    for (u32 c = 0; c < copies; c++) {
        const SliceCopy g = slice_copy(piece, layout, seeded, N, L, E, u_lo, u_hi, c);
        if (g.rows != (layout == SLICE_WHOLE ? 1 : un) * cts * halves) return printf("rows of copy %u: %u\n", c, g.rows), 1;
        for (u32 r = 0; r < g.rows; r++) {
            const size_t d = g.dst_off + r * g.dst_pitch, s = g.src_off + r * g.src_pitch;
            if (d % N || d + N > got.size() || s + N > src.size()) return printf("copy %u row %u out of bounds\n", c, r), 1;
            memcpy(got.data() + d, src.data() + s, N * sizeof(u64));
            written[d / N]++;
        }
    }
    for (size_t r = 0; r < written.size(); r++)
        if (written[r] != (r % 2 < halves ? 1 : 0)) return printf("row %zu written %d times\n", r, written[r]), 1;
    if (got != want) return printf("the slice differs from its definition\n"), 1;
    return 0;
}

int main()
{
    static const u32 shapes[3][3] = {{2, 2, 3}, {4, 2, 3}, {3, 3, 1}};   // L, K, E
    const u32 N = 8;
    size_t cases = 0;
    for (const u32 *sh : shapes) {
        const u32 L = sh[0], K = sh[1], E = sh[2];
        for (u32 u_lo = 0; u_lo <= K * L; u_lo++)
            for (u32 u_hi = u_lo; u_hi <= K * L; u_hi++)
                for (int piece = 0; piece < SLICE_PIECES; piece++)
                    for (int layout = 0; layout < 2; layout++)
                        for (int seeded = 0; seeded < 2; seeded++, cases++)
                            if (check(N, L, K, E, (SlicePiece)piece, layout ? SLICE_WHOLE : SLICE_CUT, seeded != 0, u_lo, u_hi)) {
                                printf("FAILED: L %u K %u E %u units [%u, %u) %s, %s, %s\n", L, K, E, u_lo, u_hi, piece ? "minus" : "index",
                                       layout ? "whole query" : "slice", seeded ? "seeded" : "unseeded");
                                return 1;
                            }
    }
    printf("slice geometry ok: %zu cases\n", cases);
    return 0;
}
