// slice_geometry.h -- how a slice input comes up from host memory (piehip_slice.cpp, set_piece): the strided copies that cut a handle's
// units [u_lo, u_hi) out of the source and lay them into the owned device copy [u_n][cts][2][N].  Nothing of HIP in here, so that
// tests/slice_geometry_check.cpp can perform the same copies with memcpy and compare with the definition of a slice.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace piehip {

// the two pieces of a query: the index matrix, E ciphertexts per unit, and the minus element, one
enum SlicePiece { SLICE_INDEX = 0, SLICE_MINUS = 1, SLICE_PIECES = 2 };
// the source: already cut, [u_n][cts][halves][N], or the whole query, [K][cts][halves][L][N] (the minus element: [halves][L][N]);
// halves = 2 (c0, c1), or 1 for a seeded piece, whose c1 rows are expanded on the device
enum SliceLayout { SLICE_CUT, SLICE_WHOLE };

// one copy of `rows` rows of N words; offsets and pitches in words
struct SliceCopy {
    size_t src_off, src_pitch, dst_off, dst_pitch;
    uint32_t rows;
};

// copy number c of a setter: SLICE_CUT has one copy, SLICE_WHOLE one per unit, u = u_lo + c (limb u % L of inner hash function u / L)
inline SliceCopy slice_copy(SlicePiece piece, SliceLayout layout, bool seeded, uint32_t N, uint32_t L, uint32_t E, uint32_t u_lo,
                            uint32_t u_hi, uint32_t c)
{
    const uint32_t cts = piece == SLICE_INDEX ? E : 1, halves = seeded ? 1 : 2, u = u_lo + c;
    const size_t dst_pitch = seeded ? 2 * (size_t)N : N;   // seeded: the c0 rows of ciphertexts that follow each other
    if (layout == SLICE_CUT) return {0, N, 0, dst_pitch, (u_hi - u_lo) * cts * halves};
    const size_t hf = piece == SLICE_INDEX ? (size_t)(u / L) * cts * halves * L : 0;   // every inner hash function reads the one minus element
    return {(hf + u % L) * N, (size_t)L * N, (size_t)c * cts * 2 * N, dst_pitch, cts * halves};
}

}  // namespace piehip
