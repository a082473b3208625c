// kernels_seed.hip -- expansion of seeded ciphertexts: the uniform half a[L][N] of a secret-key ciphertext (c0, c1 = a), or of an
// EvalMult key row, regenerated on the device from a 32-byte seed (include/piehip.h, "Seeded ciphertexts").
//
// Format (a wire format: the client's expansion and this one must agree bit for bit).  For limb l of the chain and chunk c of ten
// coefficients,
//     out = SHAKE128("PIEHIP-A" || seed[32] || u32le(l) || u32le(c)).digest(160)       (FIPS 202)
//     a[l][10 c + t] = (128-bit little-endian word t of out) mod q_l,   t = 0..9,  10 c + t < N
// in the ABI's EVALUATION word order (no transform, no permutation).  The 48-byte message plus padding fits one 168-byte SHAKE128
// block and 160 output bytes fit one squeeze, so every chunk is ONE Keccak-f[1600] and every thread computes its chunk alone: no
// LDS, no cross-lane traffic.  Reducing 128 bits modulo a prime below 2^61 leaves a statistical distance below 2^-67 per
// coefficient (FIPS 186's "extra random bits" method), so there is no rejection loop either.
#include "kernels.hpp"

namespace piehip {

static const u32 SEED_TPB = 256;

// 64-bit lanes as two 32-bit halves: v_alignbit_b32 for the rotates (two per 64-bit rotate, none for rotates by 0 or 32),
// v_bfi_b32 for chi (one per 32-bit half, plus one xor).
struct Lane {
    u32 lo, hi;
};

// a ^ b ^ c: gfx950 has no v_xor3_b32 (gfx10+), but hipcc folds three-input logic into gfx950's v_bitop3_b32
__device__ __forceinline__ u32 xor3(u32 a, u32 b, u32 c) { return a ^ b ^ c; }
// (m & x) | (~m & y): hipcc selects v_bfi_b32 for this pattern (checked with tools/isa_count.py)
__device__ __forceinline__ u32 bfi(u32 m, u32 x, u32 y) { return (m & x) | (~m & y); }
template <int N>
__device__ __forceinline__ Lane rotl(Lane x)
{
    constexpr int n = N & 63;
    if constexpr (n == 0) return x;
    else if constexpr (n == 32) return Lane{x.hi, x.lo};
    else if constexpr (n < 32) return Lane{__builtin_amdgcn_alignbit(x.lo, x.hi, 32 - n), __builtin_amdgcn_alignbit(x.hi, x.lo, 32 - n)};
    else return Lane{__builtin_amdgcn_alignbit(x.hi, x.lo, 64 - n), __builtin_amdgcn_alignbit(x.lo, x.hi, 64 - n)};
}

__constant__ const u64 KECCAK_RC[24] = {
    0x0000000000000001ULL, 0x0000000000008082ULL, 0x800000000000808AULL, 0x8000000080008000ULL, 0x000000000000808BULL,
    0x0000000080000001ULL, 0x8000000080008081ULL, 0x8000000000008009ULL, 0x000000000000008AULL, 0x0000000000000088ULL,
    0x0000000080008009ULL, 0x000000008000000AULL, 0x000000008000808BULL, 0x800000000000008BULL, 0x8000000000008089ULL,
    0x8000000000008003ULL, 0x8000000000008002ULL, 0x8000000000000080ULL, 0x000000000000800AULL, 0x800000008000000AULL,
    0x8000000080008081ULL, 0x8000000000008080ULL, 0x0000000080000001ULL, 0x8000000080008008ULL};

// rho offsets by lane index x + 5 y, and pi: lane x + 5 y moves to y + 5 ((2 x + 3 y) mod 5)
#define KECCAK_RHO_PI(X, Y, R) B[(Y) + 5 * ((2 * (X) + 3 * (Y)) % 5)] = rotl<R>(A[(X) + 5 * (Y)])

// Keccak-f[1600] on 25 lanes, all 24 rounds unrolled (every index is a constant: the state stays in 50 VGPRs)
__device__ __forceinline__ void keccak_f1600(Lane A[25])
{
#pragma unroll
    for (int round = 0; round < 24; round++) {
        Lane C[5], D[5], B[25];
#pragma unroll
        for (int x = 0; x < 5; x++) {
            C[x].lo = xor3(xor3(A[x].lo, A[x + 5].lo, A[x + 10].lo), A[x + 15].lo, A[x + 20].lo);
            C[x].hi = xor3(xor3(A[x].hi, A[x + 5].hi, A[x + 10].hi), A[x + 15].hi, A[x + 20].hi);
        }
#pragma unroll
        for (int x = 0; x < 5; x++) {
            const Lane r = rotl<1>(C[(x + 1) % 5]);
            D[x].lo = C[(x + 4) % 5].lo ^ r.lo;
            D[x].hi = C[(x + 4) % 5].hi ^ r.hi;
        }
#pragma unroll
        for (int i = 0; i < 25; i++) {
            A[i].lo ^= D[i % 5].lo;
            A[i].hi ^= D[i % 5].hi;
        }
        KECCAK_RHO_PI(0, 0, 0);
        KECCAK_RHO_PI(1, 0, 1);
        KECCAK_RHO_PI(2, 0, 62);
        KECCAK_RHO_PI(3, 0, 28);
        KECCAK_RHO_PI(4, 0, 27);
        KECCAK_RHO_PI(0, 1, 36);
        KECCAK_RHO_PI(1, 1, 44);
        KECCAK_RHO_PI(2, 1, 6);
        KECCAK_RHO_PI(3, 1, 55);
        KECCAK_RHO_PI(4, 1, 20);
        KECCAK_RHO_PI(0, 2, 3);
        KECCAK_RHO_PI(1, 2, 10);
        KECCAK_RHO_PI(2, 2, 43);
        KECCAK_RHO_PI(3, 2, 25);
        KECCAK_RHO_PI(4, 2, 39);
        KECCAK_RHO_PI(0, 3, 41);
        KECCAK_RHO_PI(1, 3, 45);
        KECCAK_RHO_PI(2, 3, 15);
        KECCAK_RHO_PI(3, 3, 21);
        KECCAK_RHO_PI(4, 3, 8);
        KECCAK_RHO_PI(0, 4, 18);
        KECCAK_RHO_PI(1, 4, 2);
        KECCAK_RHO_PI(2, 4, 61);
        KECCAK_RHO_PI(3, 4, 56);
        KECCAK_RHO_PI(4, 4, 14);
        // chi: a ^ (~b & c) = b ? a : a ^ c
#pragma unroll
        for (int y = 0; y < 5; y++)
#pragma unroll
            for (int x = 0; x < 5; x++) {
                const Lane a = B[x + 5 * y], b = B[(x + 1) % 5 + 5 * y], c = B[(x + 2) % 5 + 5 * y];
                A[x + 5 * y].lo = bfi(b.lo, a.lo, a.lo ^ c.lo);
                A[x + 5 * y].hi = bfi(b.hi, a.hi, a.hi ^ c.hi);
            }
        A[0].lo ^= (u32)KECCAK_RC[round];
        A[0].hi ^= (u32)(KECCAK_RC[round] >> 32);
    }
}
#undef KECCAK_RHO_PI

// One chunk: the permutation of the chunk's message and its ten words reduced mod q_l into dst[0 .. 9], as far as they lie below N
// (the last chunk of a row is partial), dst = job.dst + row + n0.  Both kernels below are this function behind their own indexing
// and job type; job and l are uniform over the workgroup.
template <class Job>
__device__ __forceinline__ void expand_chunk(const DevConsts *__restrict__ dc, const Job &job, u32 l, u32 c, size_t row, u32 n0, u32 N)
{
    const Mod m = dc->mod[l];
    Lane A[25];
#pragma unroll
    for (int i = 0; i < 25; i++) A[i] = Lane{0, 0};
    A[0] = Lane{0x48454950u, 0x412D5049u};  // "PIEHIP-A", little-endian
#pragma unroll
    for (int i = 0; i < 4; i++) A[1 + i] = Lane{job.seed[2 * i], job.seed[2 * i + 1]};
    A[5] = Lane{l, c};
    A[6].lo = 0x1Fu;           // SHAKE domain bits + first pad bit, at byte 48
    A[20].hi = 0x80000000u;    // last pad bit, at byte 167 (end of the 168-byte rate)
    keccak_f1600(A);
    u64 *dst = job.dst + row + n0;
#pragma unroll
    for (int t = 0; t < 10; t++) {
        const Lane lo = A[2 * t], hi = A[2 * t + 1];
        if (n0 + t < N) dst[t] = barrett128(((u64)hi.hi << 32) | hi.lo, ((u64)lo.hi << 32) | lo.lo, m);  // the last chunk is partial
    }
}

// one thread per (job, limb, chunk of ten coefficients); grid (chunks / SEED_TPB, L, jobs).  The job (seed and destination) is
// uniform over the workgroup: scalar loads.
__global__ void __launch_bounds__(SEED_TPB) expand_uniform_kernel(const DevConsts *__restrict__ dc, u32 N, const SeedJob *__restrict__ jobs)
{
    const u32 c = blockIdx.x * SEED_TPB + threadIdx.x;
    const u32 n0 = c * 10;
    if (n0 >= N) return;
    const u32 l = blockIdx.y;
    const SeedJob &job = jobs[blockIdx.z];
    expand_chunk(dc, job, l, c, (size_t)l * N, n0, N);
}

// Limb-selective expansion (query slices: a slice holds one-limb rows): one thread per (job, chunk); grid (chunks / SEED_TPB, jobs).
// Job j writes limb job.limb of its seed's polynomial -- the words expand_uniform_kernel writes into row job.limb -- into the ONE
// row dst[N].  What follows the row is not this polynomial's next limb (in a slice: the c0 row of the next ciphertext), so the
// partial last chunk's bound in expand_chunk is what keeps live data intact.  The job -- seed, destination, limb and with it the
// limb's reduction constants -- is uniform over the workgroup: scalar loads.
__global__ void __launch_bounds__(SEED_TPB) expand_uniform_limb_kernel(const DevConsts *__restrict__ dc, u32 N, const SeedLimbJob *__restrict__ jobs)
{
    const u32 c = blockIdx.x * SEED_TPB + threadIdx.x;
    const u32 n0 = c * 10;
    if (n0 >= N) return;
    const SeedLimbJob &job = jobs[blockIdx.y];
    expand_chunk(dc, job, job.limb, c, 0, n0, N);
}

void launch_expand_uniform(const DevConsts *dc, u32 N, u32 L, const SeedJob *jobs, u32 njobs, hipStream_t st)
{
    const u32 chunks = (N + 9) / 10;
    for (u32 j0 = 0; j0 < njobs; j0 += SEED_MAX_JOBS_PER_LAUNCH) {
        const u32 nj = std::min(njobs - j0, SEED_MAX_JOBS_PER_LAUNCH);
        hipLaunchKernelGGL(expand_uniform_kernel, dim3((chunks + SEED_TPB - 1) / SEED_TPB, L, nj), dim3(SEED_TPB), 0, st, dc, N, jobs + j0);
    }
}

void launch_expand_uniform_limb(const DevConsts *dc, u32 N, const SeedLimbJob *jobs, u32 njobs, hipStream_t st)
{
    const u32 chunks = (N + 9) / 10;
    for (u32 j0 = 0; j0 < njobs; j0 += SEED_MAX_JOBS_PER_LAUNCH) {
        const u32 nj = std::min(njobs - j0, SEED_MAX_JOBS_PER_LAUNCH);
        hipLaunchKernelGGL(expand_uniform_limb_kernel, dim3((chunks + SEED_TPB - 1) / SEED_TPB, nj), dim3(SEED_TPB), 0, st, dc, N, jobs + j0);
    }
}

}  // namespace piehip
