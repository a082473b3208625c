// piehip_client.cpp -- client-side harness (the client role of src/Client/FHE/BatchedFHEPSIClient.cpp): key generation, packed
// encryption, decryption.  Not part of the server hot path; it produces the hot path's inputs and reads its outputs.
#include "piehip_ctx.hpp"

#include <thread>

using namespace piehip;

namespace {
// xoshiro256** seeded through splitmix64, rejection sampling on the smallest covering mask
struct HostRng {
    u64 s[4];
    explicit HostRng(u64 seed)
    {
        for (int i = 0; i < 4; i++) {
            seed += 0x9E3779B97F4A7C15ULL;
            u64 z = seed;
            z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
            z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
            s[i] = z ^ (z >> 31);
        }
    }
    static u64 rotl(u64 x, int k) { return (x << k) | (x >> (64 - k)); }
    u64 next()
    {
        const u64 result = rotl(s[1] * 5, 7) * 9, t = s[1] << 17;
        s[2] ^= s[0];
        s[3] ^= s[1];
        s[1] ^= s[2];
        s[0] ^= s[3];
        s[2] ^= t;
        s[3] = rotl(s[3], 45);
        return result;
    }
    u64 below(u64 bound)
    {
        u64 mask = bound - 1;
        mask |= mask >> 1;
        mask |= mask >> 2;
        mask |= mask >> 4;
        mask |= mask >> 8;
        mask |= mask >> 16;
        mask |= mask >> 32;
        for (;;) {
            const u64 v = next() & mask;
            if (v < bound) return v;
        }
    }
};
void sample_uniform(HostRng &r, const HostParams &hp, u64 *a)  // [L][N], independent per limb
{
    for (u32 i = 0; i < hp.L; i++)
        for (u32 j = 0; j < hp.N; j++) a[(size_t)i * hp.N + j] = r.below(hp.moduli[i]);
}
void sample_error(HostRng &r, u32 N, int32_t *e)  // centred binomial, variance 10
{
    for (u32 j = 0; j < N; j++) {
        const u64 x = r.next();
        e[j] = __builtin_popcountll(x & 0xFFFFF) - __builtin_popcountll((x >> 20) & 0xFFFFF);
    }
}
}  // namespace

extern "C" {

int piehip_client_keygen(piehip_handle h, uint64_t seed, uint64_t *sk)
{
    NEED(h);
    if (!sk) return fail(PIEHIP_EINVAL, "null sk");
    HIPCHK(hipSetDevice(h->device));
    const u32 N = h->hp.N, L = h->hp.L;
    HostRng r(seed);
    std::vector<u64> host((size_t)L * N);
    for (u32 j = 0; j < N; j++) {
        const int v = (int)r.below(3) - 1;
        for (u32 i = 0; i < L; i++) host[(size_t)i * N + j] = v >= 0 ? (u64)v : h->hp.moduli[i] - 1;
    }
    Tmp tmp;
    TMPGET(d, (size_t)L * N);
    HIPCHK(hipMemcpy(d, host.data(), host.size() * sizeof(u64), hipMemcpyHostToDevice));
    launch_ntt(h->plan, d, L, 0, L, false, h->stream);
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(sk, d, host.size() * sizeof(u64), hipMemcpyDeviceToHost));
    return PIEHIP_OK;
}

// BV key-switching key from s_from to sk (oracle: ks_keygen): row i = (e_i - a_i s + [j == i] s_from, a_i).
// g == 0: s_from = s^2 (EvalMultKeyGen); otherwise s_from = s(X^g) (EvalAtIndexKeyGen / EvalSumKeyGen).
// a_seeds == null: every a_i is sampled on the host from `seed` (before its e_i) and out is the key [L][2][L][N]; otherwise a_i is
// the expansion of a_seeds[i] (kernels_seed.hip), `seed` draws the e_i only, and out is the first components [L][L][N].
static int client_ks_keygen(piehip_ctx *h, const uint64_t *sk, uint32_t g, uint64_t seed, const uint8_t *a_seeds, uint64_t *out)
{
    HIPCHK(hipSetDevice(h->device));
    const u32 N = h->hp.N, L = h->hp.L;
    const size_t LN = h->LN();
    HostRng r(seed);
    std::vector<u64> ks((size_t)L * 2 * LN), e((size_t)L * LN);
    std::vector<int32_t> ev(N);
    for (u32 i = 0; i < L; i++) {
        if (!a_seeds) sample_uniform(r, h->hp, &ks[((size_t)i * 2 + 1) * LN]);
        sample_error(r, N, ev.data());
        for (u32 l = 0; l < L; l++)
            for (u32 j = 0; j < N; j++) e[(size_t)i * LN + (size_t)l * N + j] = ev[j] >= 0 ? (u64)ev[j] : h->hp.moduli[l] - (u64)(-ev[j]);
    }
    Tmp tmp;
    TMPGET(d_ks, ks.size());
    TMPGET(d_e, e.size());
    TMPGET(d_sk, LN);
    TMPGET(d_s2, LN);
    TMPGET(d_mapw, (N + 1) / 2 + 1);
    if (a_seeds) {
        std::vector<SeedJob> jobs(L);
        for (u32 i = 0; i < L; i++) jobs[i] = seed_job(d_ks + ((size_t)i * 2 + 1) * LN, a_seeds + (size_t)i * 32);
        int rc = expand_seeded_sync(h, jobs);
        if (rc) return rc;
    } else {
        HIPCHK(hipMemcpy(d_ks, ks.data(), ks.size() * sizeof(u64), hipMemcpyHostToDevice));
    }
    HIPCHK(hipMemcpy(d_e, e.data(), e.size() * sizeof(u64), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_sk, sk, LN * sizeof(u64), hipMemcpyHostToDevice));
    launch_ntt(h->plan, d_e, L * L, 0, L, false, h->stream);
    if (g) {
        std::vector<u32> map = h->hp.automorph_map(g);
        HIPCHK(hipMemcpy(d_mapw, map.data(), sizeof(u32) * N, hipMemcpyHostToDevice));
        launch_permute(N, d_sk, (const u32 *)d_mapw, d_s2, L, h->stream);
    } else {
        launch_square(h->d_dc, N, L, d_sk, d_s2, h->stream);
    }
    launch_ks_finish(h->d_dc, N, L, d_e, d_sk, d_s2, d_ks, h->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->stream));
    if (!a_seeds) {
        HIPCHK(hipMemcpy(out, d_ks, ks.size() * sizeof(u64), hipMemcpyDeviceToHost));
    } else {
        for (u32 i = 0; i < L; i++) HIPCHK(hipMemcpy(out + (size_t)i * LN, d_ks + (size_t)i * 2 * LN, LN * sizeof(u64), hipMemcpyDeviceToHost));
    }
    return PIEHIP_OK;
}

int piehip_client_relin_keygen(piehip_handle h, const uint64_t *sk, uint64_t seed, uint64_t *evk)
{
    NEED(h);
    if (!sk || !evk) return fail(PIEHIP_EINVAL, "null operand");
    return client_ks_keygen(h, sk, 0, seed, nullptr, evk);
}

int piehip_client_relin_keygen_seeded(piehip_handle h, const uint64_t *sk, uint64_t seed, const uint8_t *a_seeds, uint64_t *evk0)
{
    if (!h) return fail(PIEHIP_EINVAL, "null handle");
    if (!sk || !a_seeds || !evk0) return fail(PIEHIP_EINVAL, "null operand");
    NEED(h);
    return client_ks_keygen(h, sk, 0, seed, a_seeds, evk0);
}

int piehip_rotation_galois(piehip_handle h, int32_t index, uint32_t *g)
{
    NEED_RO(h);
    if (!g) return fail(PIEHIP_EINVAL, "null out");
    const u32 N = h->hp.N;
    const u64 m2 = 2ULL * N;
    u64 base = 5;
    if (index < 0) base = powmod(5, N / 2 - 1, m2);  // 5 has order N/2 modulo 2N
    const u64 k = (u64)(index < 0 ? -(int64_t)index : (int64_t)index);
    *g = (u32)powmod(base, k % (N / 2 ? N / 2 : 1), m2);
    return PIEHIP_OK;
}

int piehip_client_rot_keygen(piehip_handle h, const uint64_t *sk, int32_t index, uint64_t seed, uint64_t *rk)
{
    NEED(h);
    if (!sk || !rk) return fail(PIEHIP_EINVAL, "null operand");
    uint32_t g = 1;
    int rc = piehip_rotation_galois(h, index, &g);
    if (rc) return rc;
    if (g == 1) return fail(PIEHIP_EINVAL, "rotation index is a multiple of the row length");
    return client_ks_keygen(h, sk, g, seed, nullptr, rk);
}

// a_seeds == null: every ciphertext draws a (uniform), then e, from seeds[c] on the host and out is [nct][2][L][N]; otherwise a is
// the expansion of a_seeds[c] (kernels_seed.hip), seeds[c] draws e only, and out is the c0 halves [nct][L][N]
static int client_encrypt(piehip_ctx *h, const uint64_t *sk, const int64_t *slots, uint32_t nct, uint32_t B, const uint64_t *seeds,
                          const uint8_t *a_seeds, uint64_t *out)
{
    if (B > h->hp.N) return fail(PIEHIP_EINVAL, "batch size exceeds the ring dimension");
    HIPCHK(hipSetDevice(h->device));
    const u32 N = h->hp.N, L = h->hp.L, M = h->hp.M;
    const size_t LN = h->LN();
    const u64 t = h->hp.t;
    for (size_t i = 0; i < (size_t)nct * B; i++) {
        const u64 v = (u64)slots[i], mag = slots[i] < 0 ? 0 - v : v;  // unsigned: INT64_MIN has no signed negation
        if (mag >= t) return fail(PIEHIP_EINVAL, "slot value out of range for the plaintext modulus");
    }
    // host staging, not zero-filled (the sampling threads touch their own parts): a[nct][L][N] and e[nct][N]
    std::unique_ptr<u64[]> a_host(a_seeds ? nullptr : new u64[(size_t)nct * LN]);
    std::unique_ptr<int32_t[]> ev(new int32_t[(size_t)nct * N]);
    {
        // every ciphertext has its own seed and draws a (uniform), then e, as a sequential client would: the ciphertexts are
        // independent, so host threads share them out (2.4 M rejection-sampled words for the 29 ciphertexts of a C3 query)
        auto sample = [&](u32 c0, u32 c1) {
            for (u32 c = c0; c < c1; c++) {
                HostRng r(seeds[c]);
                if (!a_seeds) sample_uniform(r, h->hp, &a_host[(size_t)c * LN]);
                sample_error(r, N, &ev[(size_t)c * N]);
            }
        };
        const u32 hw = std::thread::hardware_concurrency();
        const u32 nth = std::max(1u, std::min(std::min(nct, hw ? hw : 1u), 16u));
        std::vector<std::thread> pool;
        for (u32 i = 1; i < nth; i++) pool.emplace_back(sample, (u32)((u64)nct * i / nth), (u32)((u64)nct * (i + 1) / nth));
        sample(0, nct / nth);
        for (auto &th : pool) th.join();
    }
    const size_t ct_words = (size_t)nct * 2 * LN;
    Tmp tmp(h);
    TMPGET(d_out, ct_words);
    TMPGET(d_sk, LN);
    TMPGET(d_slotsw, (size_t)nct * B);
    TMPGET(d_u, (size_t)nct * N);
    TMPGET(d_em, (size_t)nct * LN);
    TMPGET(d_evw, ((size_t)nct * N + 1) / 2 + 1);
    TMPGET(d_a, (size_t)nct * LN);
    if (a_seeds) {
        std::vector<SeedJob> jobs(nct);
        for (u32 c = 0; c < nct; c++) jobs[c] = seed_job(d_a + (size_t)c * LN, a_seeds + (size_t)c * 32);
        int rc = expand_seeded_sync(h, jobs);
        if (rc) return rc;
    } else {
        HIPCHK(hipMemcpy(d_a, a_host.get(), (size_t)nct * LN * sizeof(u64), hipMemcpyHostToDevice));  // enc_finish puts it into the c1 halves
    }
    HIPCHK(hipMemcpy(d_sk, sk, LN * sizeof(u64), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_slotsw, slots, sizeof(int64_t) * (size_t)nct * B, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_evw, ev.get(), sizeof(int32_t) * (size_t)nct * N, hipMemcpyHostToDevice));
    launch_encode_scatter(h->d_dc, N, M, (const int64_t *)d_slotsw, B, h->d_inv_pos, d_u, nct, h->stream);
    launch_ntt(h->plan, d_u, nct, M, 1, true, h->stream);  // coefficients mod t
    launch_enc_message(h->d_dc, N, L, M, d_u, (const int32_t *)d_evw, d_em, nct, h->stream);
    launch_ntt(h->plan, d_em, nct * L, 0, L, false, h->stream);
    launch_enc_finish(h->d_dc, N, L, d_em, d_sk, d_a, d_out, nct, h->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->stream));
    if (!a_seeds) {
        HIPCHK(hipMemcpy(out, d_out, ct_words * sizeof(u64), hipMemcpyDeviceToHost));
    } else {
        for (u32 c = 0; c < nct; c++) HIPCHK(hipMemcpy(out + (size_t)c * LN, d_out + (size_t)c * 2 * LN, LN * sizeof(u64), hipMemcpyDeviceToHost));
    }
    return PIEHIP_OK;
}

int piehip_client_encrypt(piehip_handle h, const uint64_t *sk, const int64_t *slots, uint32_t nct, uint32_t B,
                          const uint64_t *seeds, uint64_t *out)
{
    NEED(h);
    if (!sk || !slots || !seeds || !out || !nct) return fail(PIEHIP_EINVAL, "null operand");
    return client_encrypt(h, sk, slots, nct, B, seeds, nullptr, out);
}

int piehip_client_encrypt_seeded(piehip_handle h, const uint64_t *sk, const int64_t *slots, uint32_t nct, uint32_t B,
                                 const uint64_t *noise_seeds, const uint8_t *a_seeds, uint64_t *c0)
{
    if (!h) return fail(PIEHIP_EINVAL, "null handle");
    if (!sk || !slots || !noise_seeds || !a_seeds || !c0 || !nct) return fail(PIEHIP_EINVAL, "null operand");
    NEED(h);
    return client_encrypt(h, sk, slots, nct, B, noise_seeds, a_seeds, c0);
}

// the device side of decryption, arguments checked by the caller.  max_dist == null: slots alone, as piehip_client_decrypt(_deg2)
// always ran it.  Otherwise the rounding kernel is the one that keeps the fraction sums: max_dist[nct] comes back with them, and
// with B == 0 the transform mod t and the gather are left out (slots is not touched)
static int decrypt_on_device(piehip_ctx *h, Tmp &tmp, const uint64_t *sk, const uint64_t *ct, uint32_t nct, uint32_t B, int64_t *slots,
                             u32 ncomp, uint64_t *max_dist)
{
    HIPCHK(hipSetDevice(h->device));
    const u32 N = h->hp.N, L = h->hp.L, M = h->hp.M;
    const size_t LN = h->LN();
    TMPGET(d_ct, (size_t)nct * ncomp * LN);
    TMPGET(d_sk, LN);
    TMPGET(d_x, (size_t)nct * LN);
    TMPGET(d_u, (size_t)nct * N);
    TMPGET(d_slotsw, (size_t)nct * B);
    TMPGET(d_posw, (N + 1) / 2 + 1);
    HIPCHK(hipMemcpy(d_ct, ct, (size_t)nct * ncomp * LN * sizeof(u64), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_sk, sk, LN * sizeof(u64), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_posw, h->hp.slot_pos.data(), sizeof(u32) * N, hipMemcpyHostToDevice));
    u64 *d_md = nullptr;
    if (max_dist) {
        d_md = tmp.get(nct);
        if (!d_md) return fail(PIEHIP_ENOMEM, "hipMalloc failed (scratch)");
    }
    launch_dec_dot(h->d_dc, N, L, d_ct, d_sk, d_x, nct, h->stream, ncomp);
    launch_ntt(h->plan, d_x, nct * L, 0, L, true, h->stream);
    if (max_dist) {
        // scratch is recycled: the block maxima land in zeroes, set on the stream the kernel runs on
        HIPCHK(hipMemsetAsync(d_md, 0, (size_t)nct * sizeof(u64), h->stream));
        launch_dec_round_budget(h->d_dc, N, L, M, d_x, B ? d_u : nullptr, d_md, nct, h->stream);
    } else {
        launch_dec_round(h->d_dc, N, L, M, d_x, d_u, nct, h->stream);
    }
    if (B || !max_dist) {
        launch_ntt(h->plan, d_u, nct, M, 1, false, h->stream);
        launch_decode_gather(h->d_dc, N, M, d_u, (const u32 *)d_posw, B, (int64_t *)d_slotsw, nct, h->stream);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->stream));
    if (B || !max_dist) HIPCHK(hipMemcpy(slots, d_slotsw, sizeof(int64_t) * (size_t)nct * B, hipMemcpyDeviceToHost));
    if (max_dist) HIPCHK(hipMemcpy(max_dist, d_md, (size_t)nct * sizeof(u64), hipMemcpyDeviceToHost));
    return PIEHIP_OK;
}

// ncomp components per ciphertext: 2, or 3 for rows of a product that was not relinearised (piehip_client_decrypt_deg2)
static int client_decrypt(piehip_handle h, const uint64_t *sk, const uint64_t *ct, uint32_t nct, uint32_t B, int64_t *slots, u32 ncomp)
{
    NEED(h);
    if (!sk || !ct || !slots || !nct) return fail(PIEHIP_EINVAL, "null operand");
    if (B > h->hp.N) return fail(PIEHIP_EINVAL, "batch size exceeds the ring dimension");
    Tmp tmp;
    return decrypt_on_device(h, tmp, sk, ct, nct, B, slots, ncomp, nullptr);
}

int piehip_client_decrypt(piehip_handle h, const uint64_t *sk, const uint64_t *ct, uint32_t nct, uint32_t B, int64_t *slots)
{
    return client_decrypt(h, sk, ct, nct, B, slots, 2);
}
int piehip_client_decrypt_deg2(piehip_handle h, const uint64_t *sk, const uint64_t *ct, uint32_t nct, uint32_t B, int64_t *slots)
{
    return client_decrypt(h, sk, ct, nct, B, slots, 3);
}

int piehip_budget_from_distance(uint64_t max_dist)
{
    if (!max_dist) return 58;
    const int budget = 59 - (64 - __builtin_clzll(max_dist));  // 59 - bit length
    return budget < 0 ? 0 : (budget > 58 ? 58 : budget);
}

int piehip_client_decrypt_budget(piehip_handle h, const uint64_t *sk, const uint64_t *ct, uint32_t nct, uint32_t ncomp, uint32_t B,
                                 int64_t *slots, int32_t *budget, uint64_t *max_dist)
{
    if (!h) return fail(PIEHIP_EINVAL, "null handle");
    if (!sk || !ct || !budget || !nct) return fail(PIEHIP_EINVAL, "null operand");
    if (ncomp != 2 && ncomp != 3) return fail(PIEHIP_EINVAL, "a ciphertext has 2 or 3 components");
    if (B > h->hp.N) return fail(PIEHIP_EINVAL, "batch size exceeds the ring dimension");
    if (B && !slots) return fail(PIEHIP_EINVAL, "null slots");
    NEED(h);
    std::vector<u64> md(nct);
    {
        Tmp tmp(h);
        int rc = decrypt_on_device(h, tmp, sk, ct, nct, B, slots, ncomp, md.data());
        if (rc) return rc;
    }
    for (u32 c = 0; c < nct; c++) budget[c] = piehip_budget_from_distance(md[c]);
    if (max_dist) std::copy(md.begin(), md.end(), max_dist);
    return PIEHIP_OK;
}

}  // extern "C"
