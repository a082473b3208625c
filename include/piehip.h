/*
 * piehip.h -- C ABI of libpiehip.so: the MI355X (gfx950) implementation of the server-side
 * batched-FHE private-indexed-equality evaluation of SAP/nested-hashing-psi.
 *
 * Drop-in boundary.  The reference operator is the concrete class
 *     class BatchedFHEHIPPIE            src/Common/Crypto/PrivateIndexedEqualityCheck/BatchedFHEHIPPIE.hpp:18-49
 * constructed at src/Server/FHE/BatchedFHEPSIServer.cpp:86 and driven at :101-103,108 in the order
 * setMinusCompareElement, setIndex, run, getResultList.  Every arithmetic instruction of run()
 * (BatchedFHEHIPPIE.cpp:88-129) is an OpenFHE call on lbcrypto::Ciphertext<DCRTPoly> /
 * lbcrypto::Plaintext objects; a DCRTPoly is L contiguous uint64_t[N] limbs ("towers") in
 * EVALUATION format, so the ABI below sees only such limb arrays: plain pointers and sizes, no
 * OpenFHE, no torch types.  INTEGRATION.md shows the binding a maintainer adds on the reference side.
 *
 * Conventions
 *   - every array is uint64_t, C-contiguous, limb-major [..][limb][N], residues canonical in
 *     [0, modulus); ciphertext/plaintext/key polynomials are in EVALUATION (NTT, bit-reversed) format,
 *     exactly as OpenFHE stores them after Encrypt / MakePackedPlaintext+SetFormat(EVALUATION).
 *   - every function returns 0 on success or a negative PIEHIP_E* code and never throws;
 *     piehip_last_error() gives the text (thread-local).  The C++ facade converts codes back into
 *     the exception types the reference throws (BatchedFHEHIPPIE.cpp:13-21: std::invalid_argument).
 *   - a handle is not thread-safe: one host thread per handle, as the reference uses one
 *     BatchedFHEHIPPIE per server process (BatchedFHEPSIServer.hpp:23).
 *   - host pointers are copied on load/set; *_device variants take pointers to HBM the caller owns
 *     (they must stay valid until the next run() has completed).
 */
#ifndef PIEHIP_H
#define PIEHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PIEHIP_OK 0
#define PIEHIP_EINVAL (-1)   /* bad argument (reference: std::invalid_argument) */
#define PIEHIP_ESTATE (-2)   /* call order violated (run before keys/DB/inputs are set) */
#define PIEHIP_EHIP (-3)     /* HIP runtime error (no device, allocation, launch) */
#define PIEHIP_ENOMEM (-4)

typedef struct piehip_ctx *piehip_handle;

/* 100 = rounds 1-4; 101 (round 5) adds piehip_profile_read_n, piehip_set/get_transform_slots, piehip_upload_turn_wait,
 * piehip_set_host_path_timing / piehip_host_path_times, piehip_rccl_wait / _abort / _agree; nothing of 100 changed its signature or
 * its meaning (piehip_profile_read keeps writing the twelve kernel classes of version 100).  102 adds the seeded ciphertexts
 * ("Seeded ciphertexts" below); nothing of 101 changed.  The result limbs ("Result limbs" below: piehip_mod_reduce, piehip_set / get_result_limbs,
 * three more kernel classes, PIEHIP_NKERNELS 14 -> 17) were added without a new number: look the symbols up; nothing of 102 changed
 * (piehip_profile_read_n writes min(n, PIEHIP_NKERNELS) entries, so a caller built with 14 keeps its 14).  The result relinearisation
 * ("Result relinearisation" below: piehip_set / get_result_relin, piehip_get_result_components, piehip_client_decrypt_deg2, one more
 * kernel class, PIEHIP_NKERNELS 17 -> 18) likewise: no new number, nothing of 102 changed. */
int piehip_version(void);
const char *piehip_last_error(void);

/* Default RNS chain: the largest primes < 2^60 that are 1 mod 2N, descending -- L for Q, then L+1
 * more for the auxiliary basis P of the HPS multiplication (what GenCryptoContext derives for the
 * reference at src/Client/FHE/BatchedFHEPSIClient.cpp:72-78). */
int piehip_default_moduli(uint32_t N, uint32_t L, uint64_t *q /*[L]*/, uint64_t *p /*[L+1]*/);

/* Replaces the CryptoContext reference held at BatchedFHEHIPPIE.hpp:21 (cryptoContext member):
 * ring dimension N, L primes q (basis Q), L+1 primes p (basis P; NULL,NULL = default chain),
 * plaintext modulus t (GetPlaintextModulus, BatchedFHEHIPPIE.cpp:43).
 * device: HIP device ordinal; stream: a hipStream_t to enqueue on, or NULL for a private stream. */
int piehip_create(piehip_handle *out, uint32_t N, uint32_t L, uint64_t t, const uint64_t *q, const uint64_t *p,
                  int device, void *stream);
int piehip_destroy(piehip_handle h);

/* parameter read-back (moduli: q_0..q_{L-1}, p_0..p_L, t = 2L+2 entries) */
int piehip_get_moduli(piehip_handle h, uint64_t *out);
int piehip_get_root(piehip_handle h, uint32_t mod_index, uint64_t *psi);
int piehip_get_twiddles(piehip_handle h, uint32_t mod_index, uint64_t *fwd /*[N]*/, uint64_t *inv /*[N]*/);
int piehip_get_slot_positions(piehip_handle h, uint32_t *pos /*[N]*/);

/* Replaces the EvalMult key the context holds after DeserializeEvalMultKey
 * (src/Server/FHE/BatchedFHEPSIServer.cpp:49): BV key, one digit per RNS limb,
 * evk[L digits][2 (b,a)][L limbs][N]. */
int piehip_load_relin_key(piehip_handle h, const uint64_t *evk);

/* Replaces the constructor's packed database (BatchedFHEHIPPIE.cpp:37-82):
 *   pts   [K][b][E][L][N]  vectorizedHCT      (BatchedFHEHIPPIE.hpp:23), EVALUATION format
 *   masks [b][L][N]        preCalcRandomMask  (BatchedFHEHIPPIE.hpp:27)
 * b is the number of bin layers THIS handle evaluates (a shard of the reference's eachBinSize). */
int piehip_load_db(piehip_handle h, uint32_t K, uint32_t b, uint32_t E, const uint64_t *pts, const uint64_t *masks);
/* Same, from raw slot values: the device performs MakePackedPlaintext (BatchedFHEHIPPIE.cpp:68,81):
 *   slots [K][b][E][B] int64 (negative = t-|v|), mask_slots [b][B]; B <= N slots used. */
int piehip_load_db_slots(piehip_handle h, uint32_t K, uint32_t b, uint32_t E, uint32_t B, const int64_t *slots,
                         const int64_t *mask_slots);

/* The server's whole offline phase on the device (src/Server/FHE/BatchedFHEPSIServer.cpp:75-90):
 * HierarchicalCuckooHashTable::insertAll (HierarchicalCuckooHashTable.cpp:55-72: k outer tabulation hashes into e
 * positions, each a blocked Cuckoo table K x b x E with inner hash ids k..k+K-1) followed by the BatchedFHEHIPPIE
 * constructor (BatchedFHEHIPPIE.cpp:23-82: bin-layer shuffle, gather into K*b*E packed plaintexts of B = k*e slots,
 * b mask plaintexts).  items[n]: non-zero values < t (0 is the empty-cell sentinel, CuckooHashTable.cpp:89-90).
 * hash_seed seeds TabulationHashing (TabulationHashing.cpp:16-36: std::mt19937 + uniform_int_distribution<uint64_t>);
 * the reference seeds evictions, shuffle and masks from std::random_device -- here they are explicit.
 * Errors: PIEHIP_EINVAL for bad sizes / items >= t, PIEHIP_EHASH when an insertion fails
 * (the reference throws runtime_error("(Blocked) Cuckoo hashing error"), CuckooHashTable.cpp:113). */
#define PIEHIP_EHASH (-5)
int piehip_build_db(piehip_handle h, const uint64_t *items, size_t n, uint32_t k, uint32_t e, uint32_t K, uint32_t b,
                    uint32_t E, uint64_t hash_seed, uint64_t evict_seed, uint64_t shuffle_seed, uint64_t mask_seed);
/* Sharded server: the same offline phase, but this handle keeps -- gathers, encodes, evaluates -- only the bin
 * layers [bin_lo, bin_hi) of the b the table has.  The table itself is built and shuffled whole, so handles given the same
 * seeds hold slices of one and the same database, and the masks of layer beta are those the unsharded call draws for it. */
int piehip_build_db_bins(piehip_handle h, const uint64_t *items, size_t n, uint32_t k, uint32_t e, uint32_t K, uint32_t b,
                         uint32_t E, uint64_t hash_seed, uint64_t evict_seed, uint64_t shuffle_seed, uint64_t mask_seed,
                         uint32_t bin_lo, uint32_t bin_hi);
/* Allocates, ahead of the offline phase, everything piehip_build_db(_bins) of this shape and a query need (database, run
 * workspace, hash table, hashing / packing scratch, input buffers), so that the timed phases do not call hipMalloc.  The
 * reference server knows these sizes when it is constructed (HashTableParameter, BatchedFHEPSIServer.hpp:24).  Optional. */
int piehip_reserve(piehip_handle h, size_t n, uint32_t k, uint32_t e, uint32_t K, uint32_t b, uint32_t E, uint32_t bin_lo,
                   uint32_t bin_hi);
/* Only the BatchedFHEHIPPIE constructor (BatchedFHEHIPPIE.cpp:23-82) on the device, for a hash table the caller
 * built itself (the reference's HierarchicalCuckooHashTable): tbl[k][e][K][b][E] = hierarchicalCuckooTable[i][p]
 * .cuckooTable[h][bin][j]; shuffles the bin layers, gathers, draws the masks and encodes. */
int piehip_load_db_table(piehip_handle h, const uint64_t *tbl, uint32_t k, uint32_t e, uint32_t K, uint32_t b, uint32_t E,
                         uint64_t shuffle_seed, uint64_t mask_seed);
int piehip_load_db_table_bins(piehip_handle h, const uint64_t *tbl, uint32_t k, uint32_t e, uint32_t K, uint32_t b, uint32_t E,
                              uint64_t shuffle_seed, uint64_t mask_seed, uint32_t bin_lo, uint32_t bin_hi);
/* the table built by piehip_build_db, after the bin shuffle: tbl[k][e][K][b][E] (hierarchicalCuckooTable[i][p].cuckooTable) */
int piehip_get_hash_table(piehip_handle h, uint64_t *tbl);
/* TabulationHashing::hashWithIndicator for n inputs (host-side; no device needed) */
int piehip_tabulation_hash(uint64_t hash_seed, uint32_t nfun, uint32_t hf, const uint64_t *x, size_t n, uint64_t *out);
/* the client's Cuckoo table (client harness; host-side): k single-layer tables of e positions, hash functions 0..k-1 of the
 * nfun-function family, items inserted in order with the reference's eviction walk (BatchedFHEPSIClient.cpp:97-99,109;
 * CuckooHashTable.cpp:72-114).  table[k][e], 0 = empty.  PIEHIP_EHASH when an insertion fails after 1000 retries. */
int piehip_client_cuckoo_table(uint64_t hash_seed, uint32_t nfun, uint32_t k, uint32_t e, const uint64_t *items, size_t n,
                               uint64_t *table);

/* setIndex (BatchedFHEHIPPIE.hpp:40-43): idx[K][E][2][L][N];
 * setMinusCompareElement (BatchedFHEHIPPIE.hpp:45-48): minus[2][L][N]. */
int piehip_set_index(piehip_handle h, const uint64_t *idx);
int piehip_set_minus(piehip_handle h, const uint64_t *minus);
/* the same for inputs that already live in HBM (no copy is taken).  The arrays must have been written on the stream
 * given to piehip_create, or be complete, at the time of the call; call again whenever their contents change, so that
 * the next run() waits for the writer (see "Stream order" below). */
int piehip_set_index_device(piehip_handle h, const void *d_idx);
int piehip_set_minus_device(piehip_handle h, const void *d_minus);

/* run() (BatchedFHEHIPPIE.cpp:88-129): enqueue the whole evaluation on the handle's stream.
 * Asynchronous; piehip_sync() or piehip_get_results() waits for it.
 * K = 1 (a database loaded with piehip_load_db / _slots; the hashing entry points refuse it as CuckooHashTable.cpp:39-42 does):
 * multipliedResult is the inner product itself (.cpp:117-120), so run() is stage A and the mask multiply (.cpp:126); no key needed. */
int piehip_run(piehip_handle h);
/* the same, with the result ciphertexts written straight into caller-owned HBM d_results[b][2][L][N] (e.g. the RCCL
 * gather buffer; d_results[b][nq][2][L][N] for a query batch) instead of the handle's result buffer */
int piehip_run_into(piehip_handle h, void *d_results);
/* The online phase in one call, as the reference server times it (BatchedFHEPSIServer.cpp:98-108): setMinusCompareElement +
 * setIndex + run + getResultList with the query in HOST memory.  The index matrix is uploaded one inner hash function (row of
 * E ciphertexts) at a time on a copy queue, stage A of row h starts as soon as that row has landed, and each queue group's
 * slice of the result list is downloaded as soon as the group is done.  Synchronous: results (may be NULL) are complete on
 * return.  Fastest with piehip_host_buffers' pinned arrays (a deserialiser writes the towers straight into them); any host
 * pointers work. */
int piehip_run_host(piehip_handle h, const uint64_t *idx /*[K][E][2][L][N]*/, const uint64_t *minus /*[2][L][N]*/,
                    uint64_t *results /*[b][2][L][N]*/);
/* The same in two halves, for a server that keeps several queries in flight (one handle per query slot, see
 * piehip_attach_database): _async returns once the uploads, the evaluation and the downloads are queued -- with page-locked
 * arrays (piehip_host_buffers) nothing in it waits for the device -- and _wait blocks until `results` is complete.  While
 * slot A evaluates, slot B's query crosses PCIe: the path is bound by the 29 MiB upload per query, not by upload + run +
 * download.  The arrays must stay valid and unchanged until _wait returns.
 * A handle with a batch of nq queries (piehip_set_query_batch) takes idx[nq][K][E][2][L][N], minus[nq][2][L][N] and writes
 * results[b][nq][2][L][N]. */
int piehip_run_host_async(piehip_handle h, const uint64_t *idx, const uint64_t *minus, uint64_t *results);
int piehip_run_host_wait(piehip_handle h);
/* page-locked staging arrays owned by the handle (valid until the database shape or the batch size changes, or the handle is
 * destroyed).  _q: the staging of query q of a batch -- every query has its own index matrix and minus element; `results` is the
 * one result array of the handle, [b][nq][2][L][N] (the nq result ciphertexts of a bin layer are adjacent), for every q. */
int piehip_host_buffers(piehip_handle h, uint64_t **idx, uint64_t **minus, uint64_t **results);
int piehip_host_buffers_q(piehip_handle h, uint32_t q, uint64_t **idx, uint64_t **minus, uint64_t **results);
/* piehip_run_host_async piece by piece, for a server that receives the query message by message -- one message per ciphertext,
 * the minus element first (BatchedFHEPSIServer.cpp:94-95,114-141): every piece starts its upload as soon as the deserialiser has
 * written it (into the page-locked arrays above, or any host memory that stays valid until piehip_run_host_wait), so the 29 MiB of
 * a C3 query cross PCIe while the remaining messages are still arriving, i.e. before the reference's timer starts (.cpp:98-99).
 *   piehip_stage_minus(_q)      the minus element [2][L][N] (of query q of the batch; pieces of different queries in any order)
 *   piehip_stage_index_row(_q)  row `row` (one inner hash function) of the index matrix, [E][2][L][N]
 *   piehip_stage_index_ct_q     one ciphertext (row, j) of the index matrix, [2][L][N] -- one message of the reference's receive loop
 *                               (.cpp:124-141): when the timer starts (.cpp:98) at most the last message's megabyte is still on
 *                               its way, not the last row's fourteen
 *   piehip_run_staged           setMinusCompareElement + setIndex + run + getResultList on the staged pieces: stage A of row h waits
 *                               for row h of every query of the batch only; results ([b][nq][2][L][N], may be NULL) are complete
 *                               after piehip_run_host_wait.
 *   piehip_stage_reset          drops a partial staging sequence (a receive failed between two pieces): the next piece begins a
 *                               new one.  Staging a piece again before the run simply replaces it.
 * PIEHIP_ESTATE when a piece is missing.  piehip_run_host_async is exactly: stage_minus, stage_index_row for every row, run_staged.
 * Queries of one device go up one after the other, in the order they were staged: the first piece of a staging sequence waits
 * (on the host) until the pieces other handles staged before it have left host memory -- uploads that share the link finish
 * together and the slots fall into lock-step (piehip_host.cpp). */
int piehip_stage_minus(piehip_handle h, const uint64_t *minus);
int piehip_stage_index_row(piehip_handle h, uint32_t row, const uint64_t *row_data);
int piehip_stage_minus_q(piehip_handle h, uint32_t q, const uint64_t *minus);
int piehip_stage_index_row_q(piehip_handle h, uint32_t q, uint32_t row, const uint64_t *row_data);
int piehip_stage_index_ct_q(piehip_handle h, uint32_t q, uint32_t row, uint32_t j, const uint64_t *ct);
int piehip_stage_reset(piehip_handle h);
int piehip_run_staged(piehip_handle h, uint64_t *results);
/* how long this handle's staging sequences waited (on the host) for their turn on the device's link: the last one, all of them,
 * and how many waited at all.  A wait that reaches 5 s returns PIEHIP_EHIP from the staging call instead of going on silently. */
int piehip_upload_turn_wait(piehip_handle h, double *last_ms, double *total_ms, uint64_t *waits);
/* measurement: with timing on, every host-memory query records three events on the handle's stream (first staged piece, uploads
 * handed over, results down); after piehip_run_host_wait piehip_host_path_times gives the last query's upload time and the rest
 * (evaluation + the result list's way down) -- which side of a slow query is slow */
int piehip_set_host_path_timing(piehip_handle h, int on);
int piehip_host_path_times(piehip_handle h, double *upload_ms, double *rest_ms);
/* Stream order.  run() works on the handle's own queues (piehip_set_run_streams); it waits for the handle's stream
 * where it must (new inputs; the result buffer), and the handle's stream waits for the run in the next call of any
 * other entry point -- piehip_join() does only that, piehip_sync() also blocks the host.  Work queued on the handle's
 * stream after such a call sees the results; consecutive run() calls pipeline. */
int piehip_join(piehip_handle h);
int piehip_sync(piehip_handle h);
/* run() spreads the (independent) bin layers over up to n HIP streams of the handle so that the partial workgroup rounds of
 * one group's launches are filled by another group's; n = 1 serialises everything on the handle's stream (per-kernel
 * timing), 0 = the default (2).  The results are complete on the handle's stream either way. */
int piehip_set_run_streams(piehip_handle h, uint32_t n);
/* The transforms are persistent grids that fill every workgroup slot of the device (two per CU) for 60-100 us at a time, with the
 * CU's whole register file.  A sharded server's RCCL kernels (broadcast of the next query, gather of the previous results) need
 * CUs during exactly those launches: n > 0 caps the transforms' grids at n workgroups (n < 2 x CUs leaves (2 x CUs - n) / 2 CUs
 * free; results are bit-identical for every n), 0 = the default, every slot.  Applies to this handle's later runs. */
int piehip_set_transform_slots(piehip_handle h, uint32_t n);
int piehip_get_transform_slots(piehip_handle h, uint32_t *n /* the cap, 0 = none */, uint32_t *device_slots /* 2 x CUs */);
/* How the context's kernels reduce sums of variable x variable products, decided once from the moduli at creation:
 *   0  128-bit accumulators, two-word Barrett (some modulus outside (2^59, 2^60))
 *   1  30-bit column accumulators, one-word Barrett (every Q and P modulus in (2^59, 2^60))
 *   2  column accumulators folded with d (every Q and P modulus is 2^60 - d with d < 2^27: the default chains) in the base
 *      conversions, scale-and-round and the fused tensor product, and butterflies that reduce by the same fold in the
 *      16-coefficient transforms of Q and P limbs; results are the same residues either way */
int piehip_get_reduction(piehip_handle h, uint32_t *kind);
/* The same for the level context of Lc limbs (Chain limbs: a level has a plan of its own, decided from the moduli it keeps, so a
 * level of a Barrett parent folds where the parent's only wide-d moduli are among those it drops).  Lc = L is the handle's own
 * plan; PIEHIP_ESTATE for a level that no piehip_set_chain_schedule of this handle has named yet. */
int piehip_get_level_reduction(piehip_handle h, uint32_t Lc, uint32_t *kind);
/* on != 0: run() / run_into() replay one captured hipGraph (all launches of both queue groups, forked from and joined back to
 * the handle's stream) instead of enqueueing ~26 launches; re-captured when the input arrays, the result buffer or the queue
 * count change.  Amortises the launch path when a handle evaluates few bin layers (one rank's share of a sharded server);
 * consecutive runs then do not overlap each other.  Off by default. */
int piehip_set_graph(piehip_handle h, int on);
/* A further query slot on the same database.  `h` (same device, same parameters) takes `owner`'s relinearisation key, packed
 * database and masks by reference -- nothing is copied -- and gets a run() workspace of its own, so that queries set and
 * run on the two handles (each on its own stream) overlap: one query's plaintext-ciphertext stage is HBM-bound while the
 * other's transforms are ALU-bound.  The reference operator evaluates one query at a time (BatchedFHEHIPPIE.cpp:88-129);
 * this is how a server with several clients keeps the GPU full.  While handles are attached, `owner` refuses (PIEHIP_ESTATE)
 * to be destroyed, to load or build a database of any shape, to reload its key and to attach itself elsewhere: the attached
 * handles read those buffers on streams of their own.  Loading a database into `h` itself returns it to a private copy
 * (load_relin_key is refused while attached). */
int piehip_attach_database(piehip_handle h, piehip_handle owner);
/* Query batches: one run() evaluates nq (1 .. 8) queries -- each with its own index matrix and minus element -- against the
 * handle's database.  The reference operator takes one query per run() (BatchedFHEHIPPIE.hpp:40-48, .cpp:88-129); a server
 * with several clients waiting hands them over together: stage A then reads every database plaintext once for the batch
 * instead of once per query (the database is 3/4 of that stage's traffic), and every later launch carries nq times as many
 * ciphertexts.  Each query's results are bit-identical to its own run().
 *   piehip_set_query_batch   sizes the workspace for nq queries per run() (default 1; may be called before or after the database
 *                            is loaded; synchronises the handle's stream)
 *   piehip_set_*_q           inputs of query q < nq (q = 0: the plain setters above)
 *   results                  piehip_run / piehip_run_into / piehip_get_results then use rows [b][nq][2][L][N]: the nq result
 *                            ciphertexts of a bin layer are adjacent
 *   piehip_load_relin_key_q  the EvalMult key of query q's client (BatchedFHEPSIServer.cpp:45-49: every client sends its own);
 *                            queries without one use the handle's key.  Sized by the batch: load again after piehip_set_query_batch.
 *                            A handle without a batch has query 0 only: its key, once loaded, is the one run() relinearises with
 * The host-memory path takes batches too: piehip_host_buffers_q / piehip_stage_*_q / piehip_run_staged / piehip_run_host* below.
 * Only the captured graph (piehip_set_graph) is limited to one query per run(). */
int piehip_set_query_batch(piehip_handle h, uint32_t nq);
int piehip_get_query_batch(piehip_handle h, uint32_t *nq);
int piehip_load_relin_key_q(piehip_handle h, uint32_t q, const uint64_t *evk /*[L][2][L][N]*/);
int piehip_set_index_q(piehip_handle h, uint32_t q, const uint64_t *idx /*[K][E][2][L][N]*/);
int piehip_set_minus_q(piehip_handle h, uint32_t q, const uint64_t *minus /*[2][L][N]*/);
int piehip_set_index_device_q(piehip_handle h, uint32_t q, const void *d_idx);
int piehip_set_minus_device_q(piehip_handle h, uint32_t q, const void *d_minus);
/* getResultList (BatchedFHEHIPPIE.hpp:35-38): out[b][2][L][N] (out[b][nq][2][L][N] for a query batch) */
int piehip_get_results(piehip_handle h, uint64_t *out);
/* device address of the result buffer [b][2][L][N] ([b][nq][2][L][N] for a query batch; valid until the database shape or the
 * batch size changes); for the RCCL gather */
int piehip_results_device(piehip_handle h, void **d_out);
/* enqueue a device-to-device copy of the results into caller-owned HBM (e.g. the RCCL gather buffer) */
int piehip_copy_results_device(piehip_handle h, void *d_dst);

/* ---- sharded server: one process per GPU, RCCL over xGMI ---------------------------------------------
 * The outer loop of run() over bin layers (BatchedFHEHIPPIE.cpp:91) has independent iterations: rank r of G evaluates the
 * bin layers [b r / G, b (r + 1) / G) of the same table (piehip_build_db_bins / piehip_load_db_table_bins with the same seeds)
 * and holds the EvalMult key(s).  Two exchanges per query, both queued on the handle's stream:
 *   piehip_rccl_broadcast_query  in: the query reaches the server on ONE rank -- the process that holds the client's socket
 *                                (BatchedFHEPSIServer.cpp:94-95,114-141).  That rank stages it (piehip_stage_*); then EVERY rank
 *                                calls this, and every rank's input buffers hold the query (all queries of a batch).
 *   piehip_gather_results        out: the only exchange of the evaluation itself.  After piehip_run on every rank, each rank's
 *                                result rows travel to `root` (the rank that answers the client: sendResult, .cpp:143-152) --
 *                                exact sizes, one transfer per rank, each over its own xGMI link.  d_out on the root:
 *                                [b_total][nq][ncomp][rl][N] in bin order, caller-owned HBM; ignored elsewhere.  ncomp and rl are
 *                                the handle's piehip_get_result_components and min(piehip_get_result_limbs, piehip_get_chain_limbs)
 *                                (the former alone for K = 1): 2 and L unless a setting says otherwise.  b_total counts what the
 *                                ranks share out: TILED layers on a tiled database (piehip_set_layer_tiling).  Rows of any other
 *                                shape than [2][L][N] travel only after piehip_rccl_agree_rows (below): PIEHIP_ESTATE otherwise.
 * RCCL is bound at run time (the copy already in the process, else /opt/rocm's): a one-GPU deployment never loads it.
 *   piehip_rccl_unique_id   ncclGetUniqueId: 128 bytes made on one rank and handed to the others by the caller's own means
 *   piehip_rccl_init        ncclCommInitRank on the handle's device (collective over the nranks processes); the handle owns it
 *   piehip_rccl_attach      or: a communicator (ncclComm_t) the caller made with the process's RCCL; not destroyed here
 *   piehip_rccl_bin_slice   the bin layers of rank `rank` (what the rank's database must be built for)
 *   piehip_rccl_broadcast   any device buffer from root to all (set-up traffic: key, seeds) */
#define PIEHIP_RCCL_ID_BYTES 128
int piehip_rccl_unique_id(void *id /*[PIEHIP_RCCL_ID_BYTES]*/);
int piehip_rccl_init(piehip_handle h, const void *id, int nranks, int rank);
int piehip_rccl_attach(piehip_handle h, void *nccl_comm, int nranks, int rank);
int piehip_rccl_destroy(piehip_handle h);
int piehip_rccl_bin_slice(uint32_t b_total, int nranks, int rank, uint32_t *bin_lo, uint32_t *bin_hi);
int piehip_rccl_broadcast(piehip_handle h, int root, void *d_buf, size_t bytes);
int piehip_rccl_broadcast_query(piehip_handle h, int root);
int piehip_gather_results(piehip_handle h, uint32_t b_total, int root, void *d_out);
/* the same, with the gathered list brought down to host memory on the root: *results (root only; NULL elsewhere) is a page-locked
 * array [b_total][nq][ncomp][rl][N] owned by the handle, complete after piehip_sync -- what sendResult (.cpp:143-152) reads */
int piehip_gather_results_host(piehip_handle h, uint32_t b_total, int root, uint64_t **results);
/* Nobody waits for the other ranks without a bound.  A collective completes when EVERY rank has queued its side; a rank that
 * never does (it died; it returned an error from one of the calls above before anything was queued) would leave its peers'
 * streams blocked for ever.  The reference ends the process on any error (BatchedFHEHIPPIE.cpp:15,20); a sharded server does the
 * same for the whole group:
 *   piehip_rccl_wait    piehip_sync with a time-out (milliseconds): polls the handle's stream and the communicator's asynchronous
 *                       error state; when the time is up or RCCL reports a failed peer it aborts the communicator (ncclCommAbort
 *                       releases the blocked stream) and returns PIEHIP_EHIP -- the handle has no communicator afterwards
 *                       (a communicator given with piehip_rccl_attach is only dropped: aborting it is its owner's business)
 *   piehip_rccl_abort   the same on purpose: a rank on its way out tears its side down, its peers' waits end at once
 *   piehip_rccl_agree   *all_ok = (every rank passed ok != 0): one all-reduced word + piehip_rccl_wait; called at the end of a phase
 *                       (database built, key loaded) so that a failure on one rank ends the session on all of them BEFORE anybody
 *                       enters a collective the failed rank will not join.  Not part of the per-query path.
 *   piehip_rccl_agree_rows   the same mechanism for the shape of a result row.  Collective: every rank contributes (ncomp, rl, nq)
 *                       as its handle stands; *same = 1 on every rank if and only if all ranks gave equal triples (one min-reduction
 *                       over the values and their negations + piehip_rccl_wait).  On same = 1 the handle remembers the triple, and
 *                       piehip_gather_results(_host) moves rows of that shape.  Every call that can change the triple forgets it:
 *                       piehip_set_result_limbs, _set_result_relin, _set_chain_limbs, _set_chain_schedule, _set_query_batch, every
 *                       database load or build, piehip_rccl_init / _attach / _abort.  A gather on a handle whose rows are not
 *                       [2][L][N] and whose triple is not the remembered one returns PIEHIP_ESTATE before anything is queued: a rank
 *                       that forgot to agree fails on its own and never posts a transfer of the wrong size.  Handles at the default
 *                       shape need no agreement.  Not part of the per-query path. */
/* Query slices across the ranks ("Query slices" below; the plan of both calls and of the gather: csrc/exchange_plan.h).  Rank r of G is a query-sliced
 * handle with the units of piehip_query_slice(K, L, G, r) and the bin layers of piehip_rccl_bin_slice(b, G, r); no rank needs the
 * whole query, and no rank but the root ever holds it.  Per batch of queries, every rank calls, in this order: piehip_rccl_scatter_query,
 * piehip_run_slice, piehip_rccl_exchange_accumulators, piehip_run_chain, piehip_gather_results(_host), piehip_rccl_wait.
 *   piehip_rccl_scatter_query          (BatchedFHEPSIServer.cpp:114-141, the query's way in; BatchedFHEHIPPIE.hpp:40-48) the root cuts every
 *                                      rank's slices out of its piehip_slice_host_buffers_q arrays -- one strided copy per unit and piece
 *                                      into a device staging area in unit order -- and sends each rank the contiguous ranges of its units:
 *                                      per query the index slice [u_n][E][2][N] and the minus slice [u_n][2][N], straight into the
 *                                      receiver's owned slice inputs, which the next piehip_run_slice reads (a pending expansion of such a
 *                                      piece is cancelled, as by any unseeded setter).  The root's own units are a device copy; a rank
 *                                      without units takes no part.  All nq queries in ONE group call on the handle's stream; the host
 *                                      arrays must stay unchanged until the next piehip_sync or piehip_rccl_wait.
 *   piehip_rccl_exchange_accumulators  (BatchedFHEHIPPIE.cpp:117: the accumulators as the chain reads them) after piehip_run_slice: rank s
 *                                      sends rank d the rows [bin_lo_d, bin_hi_d) of its acc_slice, one contiguous block; d receives it
 *                                      into a staging buffer (allocated at the first exchange of a shape and kept).  One group call on the
 *                                      handle's stream; then ONE placement launch puts every unit 0 .. K L - 1 -- the received blocks and
 *                                      the handle's own rows -- into the chain side, behind the queues of the handle's last run_chain, as
 *                                      piehip_put_accumulators does for one source.  All units count as put: piehip_run_chain follows.
 * Both refuse before anything is queued, and a refused call changes nothing: PIEHIP_ESTATE without a communicator, on an unsliced handle,
 * when a unit has already been put in this round (exchange), when the root has not asked for its host arrays (scatter); PIEHIP_EINVAL for
 * a null handle, a root outside the communicator, and unit or bin ranges that are not the rule's for (nranks, rank) -- the peers' ranges
 * are derived, not exchanged.  piehip_gather_results(_host) serves a sliced handle after piehip_run_chain as it serves any other,
 * a rank without bin layers included. */
int piehip_rccl_scatter_query(piehip_handle h, int root);
int piehip_rccl_exchange_accumulators(piehip_handle h);
int piehip_rccl_wait(piehip_handle h, uint32_t timeout_ms);
int piehip_rccl_abort(piehip_handle h);
int piehip_rccl_agree(piehip_handle h, int ok, int *all_ok, uint32_t timeout_ms);
int piehip_rccl_agree_rows(piehip_handle h, uint32_t timeout_ms, int *same);

/* ---- the OpenFHE primitives under run(), exposed one by one for kernel-level parity tests ------
 * (host buffers in, host buffers out; synchronous) */
/* DCRTPoly::SetFormat on nlimbs limbs [nlimbs][N]; limb i uses modulus mod_base + (i % mod_count) */
int piehip_ntt(piehip_handle h, uint64_t *limbs, uint32_t nlimbs, uint32_t mod_base, uint32_t mod_count, int inverse);
/* EvalAdd(ct,ct) BatchedFHEHIPPIE.cpp:112,116 / EvalMult(ct,pt) :108,113,126 */
int piehip_eval_add(piehip_handle h, const uint64_t *x, const uint64_t *y, uint64_t *out);
int piehip_eval_mult_plain(piehip_handle h, const uint64_t *x, const uint64_t *pt, uint64_t *out);
/* EvalMult(ct,ct) BatchedFHEHIPPIE.cpp:123 (HPS P-over-Q tensor + BV relinearisation with the loaded
 * key); nct independent pairs x[nct][2][L][N], y[nct][2][L][N] -> out[nct][2][L][N].
 * relin=0 returns the 3-component tensor result out[nct][3][L][N] instead. */
int piehip_eval_mult(piehip_handle h, const uint64_t *x, const uint64_t *y, uint32_t nct, int relin, uint64_t *out);
/* EvalAtIndex-style rotation (reference call sites FHEHIPPIE.cpp:71,74 via EvalInnerProduct/EvalMerge;
 * NOT on the batched path): automorphism X -> X^g then key switch with rk[L][2][L][N] */
int piehip_eval_automorph(piehip_handle h, const uint64_t *x, uint32_t g, const uint64_t *rk, uint64_t *out);
/* MakePackedPlaintext for npt plaintexts: slots[npt][B] -> out[npt][L][N] EVALUATION format */
int piehip_encode(piehip_handle h, const int64_t *slots, uint32_t npt, uint32_t B, uint64_t *out);
/* base conversions of the HPS multiplication on npoly polynomials (COEFFICIENT format):
 * which = 0: Q -> QP centred extension        in[npoly][L][N]    -> out[npoly][2L+1][N]
 * which = 1: scale by P/Q into P, extend to QP in[npoly][L][N]    -> out[npoly][2L+1][N]
 * which = 2: scale by t/P from QP into Q      in[npoly][2L+1][N] -> out[npoly][L][N] */
int piehip_base_convert(piehip_handle h, int which, const uint64_t *in, uint32_t npoly, uint64_t *out);

/* ---- result limbs: result ciphertexts leave the device on a prefix of the prime chain ------------------------------------------
 * After the last multiplication a result ciphertext is only ever decrypted, and it decrypts as well on fewer RNS limbs (what SEAL
 * does before it serialises a result, and OpenFHE's Compress; the reference calls neither): a C3 result (4 x 60-bit primes, 33-bit t)
 * is 3.5 MiB per query on one limb instead of 14 MiB on four.
 * The operation, in exact integers.  A component is a polynomial with coefficients c in [0, Q), held as residues.  The limbs
 * l = L - 1, L - 2, .., keep are dropped one after the other; each drop is
 *     r = c mod q_l, centred (r = v if v <= (q_l - 1) / 2 else v - q_l);   c <- (c - r) / q_l   (exact),
 * i.e. c_i <- (c_i - r) q_l^-1 mod q_i for i < l, coefficient by coefficient in COEFFICIENT format, both components alike.  Input and
 * output cross the ABI in EVALUATION format; the output is [2][keep][N], canonical, under q_0 .. q_{keep-1}, and decrypts as a plain
 * BFV ciphertext of the context (N, keep, t, q[:keep]) with the first `keep` limbs of the secret key.  A drop adds at most
 * t (1 + N) / (2 q_0) to the invariant noise.  Integer arithmetic only: every schedule gives the same bits.  The library does not
 * check noise: piehip_client_decrypt_budget (client-side harness, below) measures what a reduced row has left.
 *   piehip_mod_reduce        the operation on nct ciphertexts in host memory; synchronous.  keep == L copies the input.
 *   piehip_set_result_limbs  run() ends with the reduction of its result list to `keep` limbs (default L: nothing is added, no
 *                            launch, buffer or byte differs).  With keep < L every queue group of a run() is followed, on its own
 *                            queue, by an inverse transform of its result rows, the limb-drop kernel and a forward transform of the
 *                            kept limbs, and everything that hands results out uses rows of 2 keep N words: piehip_run,
 *                            piehip_run_into (d_results[b][nq][2][keep][N]), piehip_get_results, piehip_results_device,
 *                            piehip_copy_results_device, piehip_run_staged, piehip_run_host(_async / _wait / _seeded*) and the
 *                            page-locked result array of piehip_host_buffers(_q), which is sized by the setting at the time of the
 *                            call (ask again after changing it).  Per handle: a query slot (piehip_attach_database) has its own
 *                            setting.  Any K.  In a host-results run a queue group's download follows that group's reduction; the
 *                            next group is released (see piehip_run_host) in front of the group's limb-drop kernel, when the group
 *                            has that kernel and the forward transform of the kept limbs left.
 *   piehip_get_result_limbs  the setting.
 * PIEHIP_EINVAL: keep == 0 or keep > L.  PIEHIP_ESTATE: keep < L on a handle with piehip_set_graph(1), and piehip_set_graph(1) on a
 * handle with keep < L (the captured graph stays one plain query per run()).  piehip_gather_results(_host) gathers the rows of a
 * handle with keep < L once the ranks have compared their row shapes (piehip_rccl_agree_rows, after the setting; PIEHIP_ESTATE
 * until then): both ends of a transfer then name one size.  piehip_fhepie_* ignores the setting. */
int piehip_mod_reduce(piehip_handle h, const uint64_t *in /*[nct][2][L][N]*/, uint32_t nct, uint32_t keep,
                      uint64_t *out /*[nct][2][keep][N]*/);
int piehip_set_result_limbs(piehip_handle h, uint32_t keep);
int piehip_get_result_limbs(piehip_handle h, uint32_t *keep);

/* ---- result relinearisation: run() without the last key switch -------------------------------------------------------------------
 * run() ends every bin layer with EvalMult(ct, ct) and the mask multiply (BatchedFHEHIPPIE.cpp:123,126), and the result is only ever
 * decrypted.  A three-component ciphertext (d0, d1, d2) decrypts as d0 + d1 s + d2 s^2, so the relinearisation of that last product
 * does nothing for the client: the reference pays for it because OpenFHE's EvalMult relinearises by default.  Leaving it out saves the
 * key switch of the last product (the L^2 digit transforms, the digit array, the key-switch MAC and every key word it reads), and a
 * database with K = 2 inner hash functions then needs no EvalMult key at all.  The price is a third component in every result row.
 *   piehip_set_result_relin  on = 1 (the default): no launch, buffer, byte or refusal differs.  on = 0 with a database of K >= 2: the
 *                            product chain relinearises the products h = 1 .. K - 2 as before, the LAST product (h = K - 1) is left as
 *                            its three-component tensor result and the mask multiplies all three components.  A result row is
 *                            [3][keep][N]: components d0, d1, d2, EVALUATION format, standard order, canonical residues, and
 *                            everything that hands results out uses rows of 3 keep N words: piehip_run, piehip_run_into
 *                            (d_results[b][nq][3][keep][N]), piehip_get_results, piehip_results_device (the buffer may move when
 *                            the setting changes: ask again), piehip_copy_results_device, piehip_run_staged,
 *                            piehip_run_host(_async / _wait / _seeded*) and the page-locked result array of
 *                            piehip_host_buffers(_q), which is sized by the setting at the time of the call (ask again after
 *                            changing it).  K = 1: there is no product, the setting has no effect, rows keep two components.
 *                            Per handle: a query slot (piehip_attach_database) has its own setting.
 *   piehip_get_result_relin  the setting.
 *   piehip_get_result_components  2 or 3: the components of a result row as the handle stands (setting and loaded K).
 * The exact bits.  Component c of row (beta, q) is mask_beta (.) T[c], where T = (x0 y0, x0 y1 + x1 y0, x1 y1) scaled by t/Q and rounded
 * -- the tensor result piehip_eval_mult(relin = 0) returns -- of X, the chain's value in front of the last product (the h = 0
 * accumulator at K = 2, the relinearised product of the earlier accumulators at K >= 3), and Y, the last accumulator.  Integer
 * arithmetic only: every schedule and route gives the same bits.
 * Keys.  With on = 0 and K = 2, piehip_run* needs NO EvalMult key (loading one is harmless).  K >= 3 needs keys as before, and
 * per-query keys (piehip_load_relin_key_q) work as before.
 * Result limbs.  The setting composes with piehip_set_result_limbs: the limb drop runs over rows * 3 polynomials; its definition is
 * per polynomial and unchanged.  Noise: a drop rounds every coefficient of component c by e_c, |e_c| <= 1/2, and the decryption
 * sees e_0 + e_1 s + e_2 s^2.  The first two terms are the two-component drop's, at most (1 + N) / 2 for a ternary s.  The third is at
 * most ||s^2||_1 / 2, and ||s^2||_1 can reach N^2: in the worst case over all ternary s a drop adds t (1 + N + N^2) / (2 q_0) to the
 * invariant noise, which at C3's parameters (N = 2^14, 33-bit t, q_0 ~ 2^60) is no bound at all.  For the uniform ternary s the client
 * draws, a coefficient of s^2 is a sum of N products of variance 4/9, a coefficient of e_2 s^2 a sum of N independent terms of
 * variance (1/12)(4/9) N each: standard deviation N / sqrt(27), and |e_2 s^2| <= 6 N / sqrt(27) < 1.2 N in every coefficient except
 * with probability below 2^-27 N.  With that probability a drop adds at most t (1 + N + 2.4 N) / (2 q_0): a high-probability bound,
 * not a worst-case one (INTEGRATION.md section 5 has the measured budgets).  The library does not check noise:
 * piehip_client_decrypt_budget with ncomp = 3 measures what a three-component row has left.
 * PIEHIP_ESTATE: on = 0 on a handle with piehip_set_graph(1), and piehip_set_graph(1) on a handle with on = 0 (the captured graph
 * stays the reference's run()); on = 0 on a query-sliced handle (piehip_load_db*_sliced), and a sliced load on a handle with on = 0.
 * piehip_gather_results(_host) gathers three-component rows under the condition of keep < L: after piehip_rccl_agree_rows, and
 * PIEHIP_ESTATE until then.  piehip_fhepie_* ignores the setting.
 *   piehip_client_decrypt_deg2  Decrypt + GetPackedValue of three-component rows ct[nct][3][L][N] -> slots[nct][B] (centred):
 *                            c0 + c1 s + c2 s^2 on the handle's chain (rows reduced to keep < L limbs decrypt on a context of the
 *                            chain q[:keep] with the first keep limbs of the key, as two-component ones do). */
int piehip_set_result_relin(piehip_handle h, int on);
int piehip_get_result_relin(piehip_handle h, int *on);
int piehip_get_result_components(piehip_handle h, uint32_t *ncomp);
int piehip_client_decrypt_deg2(piehip_handle h, const uint64_t *sk, const uint64_t *ct /*[nct][3][L][N]*/, uint32_t nct, uint32_t B,
                               int64_t *slots);

/* ---- chain limbs: the product chain of run() on a prefix of the RNS prime chain -----------------------------
 * Everything of run() behind stage A -- the inverse transforms of the accumulators, both base conversions, the tensor product,
 * scale-and-round, the digit transforms and the key-switch MAC -- costs between L and L^2 per row, and a stage-A accumulator (a sum of
 * ciphertext x plaintext products) has most of its noise budget left.  The limb drop of "Result limbs" can therefore move to the FRONT
 * of the chain: modulus switching between levels, as SEAL and OpenFHE users know it.  Opt-in, per handle, off by default.
 *   piehip_set_chain_limbs   1 <= Lc <= L; Lc = L (the default): no launch, buffer or byte differs.  With Lc < L and a database of
 *                            K >= 2, run() is, in exact integers:
 *                            1. stage A as ever, on all L limbs: the accumulators are bit-identical;
 *                            2. the limb drop: every accumulator ciphertext is reduced to its first Lc limbs by the limb drop of
 *                               "Result limbs" -- the same formula, both components, the limbs L - 1 .. Lc one after the other with
 *                               centred rounding: what piehip_mod_reduce(.., keep = Lc) computes;
 *                            3. the product chain and the mask multiply (BatchedFHEHIPPIE.cpp:117-126) exactly as run() performs them
 *                               on the LEVEL CONTEXT (N, Lc, t, q[:Lc], p[:Lc + 1]) -- every product, the intermediate ones of K >= 3
 *                               included -- with the EvalMult key evk[i][c][j] restricted to i, j < Lc (the BV key's digit factor is
 *                               [i = j] limb by limb, so the prefix is a valid key modulo Q' = q_0 .. q_{Lc-1}) and the masks
 *                               restricted to their first Lc limbs;
 *                            4. result rows [b][nq][ncomp][min(keep, Lc)][N]: with keep < Lc (piehip_set_result_limbs) the result
 *                               reduction follows inside the level context, from Lc limbs down to keep; ncomp follows
 *                               piehip_set_result_relin as ever (degree-2 results at a lower level work; K = 2 still needs no key).
 *                            K = 1 has no product: the setting is accepted and changes nothing (rows of `keep` limbs).
 *                            Every entry point that hands results out sizes its rows by min(keep, Lc): piehip_run, piehip_run_into,
 *                            piehip_get_results, piehip_results_device, piehip_copy_results_device, piehip_run_staged,
 *                            piehip_run_host(_async / _wait / _seeded*) and the page-locked result array of piehip_host_buffers(_q),
 *                            which is sized by the settings at the time of the call (ask again after changing one).
 *                            Per handle: a query slot (piehip_attach_database) has its own setting.  Works with query batches and
 *                            per-query keys, seeded queries (stage A is untouched), one and two queues, the host-results stagger.
 *   piehip_get_chain_limbs   the setting (with a chain schedule, below: the limb count of the last product that runs).
 * Choosing Lc.  The library does not check noise (piehip_client_decrypt_budget measures it on the result rows).  The budget after the
 * drop is min(budget, log2 Q' - log2 t - log2(N + 1) - 1) bits, and the chain then costs what it costs on any context of Lc limbs.  Budgets in bits as the CPU oracle reports them (its readout
 * saturates at 57-58), K = 2, fresh queries (tests/test_chain_limbs.py):
 *     parameters                                   full chain   chain limbs L-1        then keep = 2 / 1   chain limbs L-2
 *     N = 16384, L = 4, t = 4296540161, E = 14     57           40, same plaintext     40 / 20             0, WRONG plaintext
 *     N = 4096,  L = 3, t = 65537,      E = 6      57           14, same plaintext     -  / 14             0, WRONG plaintext
 *     N = 2048,  L = 3, t = 4296540161, E = 3      29           0,  WRONG plaintext
 * The L-2 column and the third row do NOT decrypt: the setting is the caller's responsibility.
 * PIEHIP_EINVAL: Lc = 0 or Lc > L.  PIEHIP_ESTATE (the handle stays usable): Lc < L on a handle with piehip_set_graph(1), and
 * piehip_set_graph(1) on a handle with Lc < L; Lc < L on a query-sliced handle, and a sliced load on a handle with Lc < L;
 * piehip_gather_results(_host) on a handle whose rows have fewer than L limbs by this setting, until the ranks have agreed on the
 * row shape (piehip_rccl_agree_rows).  piehip_fhepie_* ignores the setting.  Added without a new version number:
 * look the symbols up; nothing of 102 changed. */
int piehip_set_chain_limbs(piehip_handle h, uint32_t Lc);
int piehip_get_chain_limbs(piehip_handle h, uint32_t *Lc);
/* Chain schedule: a limb count per product.  The products of a chain of K >= 3 do not need the same number of limbs -- the last one
 * has the least noise budget left to protect -- so the drop can also sit BETWEEN the products.
 *   piehip_set_chain_schedule   Lc[0] >= Lc[1] >= .. >= Lc[n-1], every entry in [1, L], 1 <= n <= 7.  Product hf (1-based, hf < K) runs
 *                               on l_hf = Lc[min(hf, n) - 1] limbs; l_last is the level of the last product that runs.  In exact integers:
 *                               1. stage A on all L limbs;
 *                               2. x = drop(acc[0], L -> l_1);
 *                               3. for hf = 1 .. K - 1: where l_hf is below the level of x, x = mod_reduce(x, l_hf) on the level
 *                                  context of l_{hf-1} limbs; y = mod_reduce(acc[hf], l_hf) on the handle's context; x = the product
 *                                  of x and y on the level context of l_hf limbs, with the key evk[:l_hf, :, :l_hf] (without the last
 *                                  relinearisation, piehip_set_result_relin(0), the last product is the tensor product alone);
 *                               4. the mask multiply with the masks' first l_last limbs; rows [b][nq][ncomp][min(keep, l_last)][N].
 *                               mod_reduce is piehip_mod_reduce's formula.  piehip_set_chain_limbs(h, x) is the schedule {x}; entries
 *                               behind the last product that runs change nothing; K = 1 is accepted and changes nothing.
 *   piehip_get_chain_schedule   the schedule as it was set (n entries; PIEHIP_EINVAL when cap < n).  piehip_get_chain_limbs answers
 *                               l_last, and every entry point that sizes result rows means l_last.
 * Per handle, like chain limbs: a query slot has its own schedule.  Everything chain limbs works with, a schedule works with.
 * Choosing a schedule.  The library checks no noise.  Budgets in bits as the CPU oracle reports them, K = 3, b = 1, fresh queries
 * (tests/test_chain_schedule.py prints them); (l_1, l_2): product 1 on l_1 limbs, product 2 and the mask multiply on l_2:
 *     N = 16384, L = 4, t = 4296540161, E = 14   (4,4) 38 | (4,3) 38 | (3,3), (3,2), (4,2): 0, WRONG plaintext
 *     N = 32768, L = 6, t = 4296540161, E = 30   (6,6) 56 | (6,5) 56 | (5,5) 56 | (5,4) 57 | (6,4) 57 | (4,4) 53 | (4,3) 38 | (5,3) 39 |
 *                                                (6,3) 39 | (3,3): 0, WRONG plaintext
 *     N = 4096,  L = 4, t = 65537,      E = 4    (4,4) 57 | (4,3) 57 | (3,3) 48 | (3,2) 14 | (4,2) 14 | (2,2): 0, WRONG plaintext
 * On the first row no uniform setting below L decrypts and (4,3) keeps the full run's 38 bits; on the second the lowest uniform
 * setting is (4,4) and (4,3) still leaves 38 bits.  Every other entry named here has the full run's plaintext.
 * Rule of thumb: give the last product one limb fewer than the lowest uniform setting that still decrypts, and every product before it
 * that setting; check the budget of the real parameters on a client before relying on it: piehip_client_decrypt_budget reads it from
 * the result rows, and nested_hashing_psi_amd/schedule.py (choose_chain_schedule) runs every candidate schedule and picks by it.
 * PIEHIP_EINVAL: n = 0 or n > 7, an entry of 0 or above L, an increasing pair.  PIEHIP_ESTATE: every refusal of chain limbs above,
 * whenever any entry is below L.  piehip_fhepie_* ignores the setting.  Added without a new version number: look the symbols up. */
int piehip_set_chain_schedule(piehip_handle h, const uint32_t *Lc /*[n]*/, uint32_t n);
int piehip_get_chain_schedule(piehip_handle h, uint32_t *Lc /*[cap]*/, uint32_t cap, uint32_t *n);

/* ---- layer tiling: several bin layers in one ciphertext's slots --------------------------------------------
 * run() time, database bytes, result bytes and the client's decryption work are linear in the bin-layer count b, and a packed plaintext
 * uses B = k e of the ring's N slots.  run() is slot-wise from the first multiply to the mask, so when B <= N / 2, R = floor(N / B) bin
 * layers fit side by side in one plaintext: the client repeats its B query slots R times, one "tiled layer" evaluates R bin layers, and
 * b becomes b' = ceil(b / R) everywhere.  With slot s = i e + p as ever and R >= 1, R B <= N, the tiled database is a re-arrangement of
 * what the loaders gather, after the same shuffle and with the same mask draw:
 *   database slots   slots'[h][g][j][r B + s] = slots[h][g R + r][j][s] for g R + r < b, else 0; slots at R B and above are 0
 *   mask slots       mask'[g][r B + s] = mask(layer g R + r, slot s) by the rule of the untiled draw; the layer index runs on past b
 *                    in the last tiled layer (the draw of b' R layers on B slots, read as [b'][R B])
 *   client vectors   the client tiles every plaintext vector: index'[h][j][r B + s] = index[h][j][s], and the minus vector likewise
 *   results          row g, slot r B + s, is bin layer g R + r, slot s; blocks with g R + r >= b are to be ignored.  They are never
 *                    zero: the accumulator there is -x != 0 in an occupied slot and +1 in a dummy slot, times a mask in [1, t - 1],
 *                    and t is prime
 * The handle then holds an ordinary database of b' layers on R B slots: run() and everything behind it are untouched.
 *   piehip_set_layer_tiling   per handle, R >= 1, default 1 (no launch, buffer, byte or refusal differs).  Read by the NEXT
 *                             piehip_build_db(_bins), piehip_load_db_table(_bins) and piehip_reserve: they size and build for b' layers,
 *                             and bin_lo / bin_hi count tiled layers.  piehip_get_hash_table still returns the untiled [k][e][K][b][E].
 *                             piehip_load_db and piehip_load_db_slots ignore the setting (their callers tile by hand), and a handle
 *                             attached to another's database takes what that database is.
 *   piehip_get_layer_tiling   the setting
 *   piehip_layer_tiling       host only, no handle: the balanced choice for a shape.  Rmax = floor(N / (k e));
 *                             b_tiled = ceil(b / min(Rmax, b)); R = ceil(b / b_tiled): the fewest tiled layers, filled evenly.
 * PIEHIP_EINVAL: R = 0; from the build, load or reserve when R k e > N (the handle keeps its previous database and stays usable);
 * piehip_layer_tiling when k e > N.  PIEHIP_ESTATE: piehip_load_db_table_sliced and piehip_build_db_sliced while R > 1 (query slices
 * of a tiled database are not built).  Added without a new version number: look the symbols up. */
int piehip_set_layer_tiling(piehip_handle h, uint32_t R);
int piehip_get_layer_tiling(piehip_handle h, uint32_t *R);
int piehip_layer_tiling(uint32_t N, uint32_t k, uint32_t e, uint32_t b, uint32_t *R, uint32_t *b_tiled);   /* host only, no handle */

/* ---- query slices: stage A sharded by inner hash function and limb --------------------------------------
 * The reference evaluates, per bin layer, K inner products over E index ciphertexts (BatchedFHEHIPPIE.cpp:96-116) and then multiplies
 * the K accumulators together (.cpp:117-126).  Every RNS limb of an inner product depends on that limb of its operands only, so the
 * first half shards by what the QUERY is made of.  A unit u = h L + l, 0 <= u < K L, is limb l = u % L (modulus q_l) of inner hash
 * function h = u / L.  A query-sliced handle has two sides:
 *   the slice side (.cpp:96-116)   a contiguous unit range [u_lo, u_hi), u_n = u_hi - u_lo: those limbs of the packed database for ALL
 *                                  b bin layers ([u_n][b][E][N] words, 1 / (K L) of the database per unit), those limbs of every
 *                                  query's index ciphertexts and minus element, and -- piehip_run_slice -- those limbs of every
 *                                  accumulator, acc_slice[b][nq][u_n][2][N] (EVALUATION format, canonical residues)
 *   the chain side (.cpp:117-126)  the bin layers [bin_lo, bin_hi) of b, as a piehip_load_db_table_bins handle has them: their masks, a
 *                                  run() workspace, the EvalMult key(s).  piehip_put_accumulators(_from) places the limbs that arrive
 *                                  from the slice sides; piehip_run_chain runs everything of run() behind stage A.
 * G handles whose unit ranges tile [0, K L) and whose bin ranges tile [0, b) evaluate a query together; each is sent u_n / (K L) of it.
 * The results are, word for word, those of piehip_run on unsliced handles.  Either range may be empty (a handle that only computes
 * units, or only runs chains; G > K L and G > b are legal).
 *   piehip_query_slice            (.cpp:96-116; host only) the units of rank `rank` of nranks: [K L rank / nranks, K L (rank + 1) / nranks),
 *                                 the rule of piehip_rccl_bin_slice
 *   piehip_load_db_table_sliced   (.cpp:45-82 for the slice side, the masks of :77-81 for the chain side) the table is shuffled whole with
 *                                 shuffle_seed -- the database of piehip_load_db_table with the same seeds -- and the handle gathers and
 *                                 encodes only its units' limbs (the forward transform runs for those limbs only); the masks of its bin
 *                                 layers are the ones the unsharded call draws.  Refuses K = 1 as every hashing entry point does.
 *                                 Synchronous, on the handle's stream.
 *   piehip_build_db_sliced        (.cpp:45-82, with the table's construction at :45-66 on the device) piehip_build_db_bins' offline phase for a
 *                                 sliced handle: the server set is hashed and the whole table shuffled in HBM, where it stays -- no round
 *                                 trip through host memory -- and then encoded as piehip_load_db_table_sliced encodes its table: the units'
 *                                 limbs, the masks of the chain side's layers.  The same seeds give slices of the one database that
 *                                 piehip_build_db makes.  K = 1 refused; PIEHIP_EHASH when the Cuckoo insertion fails.  Synchronous.
 *   piehip_load_db_sliced         the same from arrays: pts_slice[u_n][b][E][N] (unit u: limb u % L of pts[u / L][.][.] of piehip_load_db),
 *                                 masks[bin_hi - bin_lo][L][N].  Any K >= 1.  Synchronous.
 *   piehip_get_query_slice        the four bounds of a sliced handle
 *   piehip_set_index_slice_q      (.hpp:40-43) query q's index slice, host memory: idx_slice[u_n][E][2][N]; synchronous
 *   piehip_set_minus_slice_q      (.hpp:45-48) ... minus slice [u_n][2][N]: limb u % L of the minus element for every unit
 *   piehip_set_*_slice_from_q     the same cut out of the WHOLE input in host memory (idx[K][E][2][L][N], minus[2][L][N]): one strided
 *                                 copy per unit; only the handle's units cross the link
 *   piehip_set_index_slice_seeded_q   seeded slice inputs ("Seeded ciphertexts"): only the c0 rows cross the link, c0_slice[u_n][E][N] (unit u:
 *   piehip_set_minus_slice_seeded_q   limb u % L of the c0 halves of inner hash function u / L) and [u_n][N], into the c0 rows of the owned
 *                                 slice copy.  `seeds` is always the WHOLE query's table, [K][E][32] for the index matrix and [32] for the
 *                                 minus element: the handle picks the rows of its own units.  Synchronous, as their unseeded siblings;
 *                                 the seeds are remembered.  The next piehip_run_slice queues ONE limb-selective expansion launch
 *                                 (kernels_seed.hip), on the handle's stream in front of stage A, for every piece of the batch that was
 *                                 set seeded since the last piehip_run_slice: row c1 of unit u is limb u % L of the seed's polynomial,
 *                                 bit for bit.  A piece that is not set again is not expanded again (its c1 is still there).  Setting a
 *                                 piece through any unseeded or device-pointer setter cancels its pending expansion: an expansion never
 *                                 writes over an unseeded input (the contract of the host-memory path)
 *   piehip_set_*_slice_seeded_from_q  the same cut out of the WHOLE c0 arrays in host memory (c0idx[K][E][L][N], c0minus[L][N]): one strided
 *                                 copy per unit.  Per query a handle receives (E + 1) N 8 bytes per unit: half of the unseeded bytes
 *   piehip_slice_host_buffers_q   (.hpp:40-48: where setIndex / setMinusCompareElement find their arguments) page-locked arrays for the WHOLE
 *                                 query q, idx[K][E][2][L][N] and minus[2][L][N], owned by the sliced handle and allocated at the first call
 *                                 that asks for them (a null out-pointer allocates nothing): where the rank that holds the client's channel
 *                                 writes a query for piehip_rccl_scatter_query
 *   piehip_set_*_slice_device_q   arrays in HBM, no copy taken; ordered as piehip_set_index_device is (written on the handle's stream, or complete)
 *                                 piehip_set_query_batch sizes everything for nq queries, as on any handle
 *   piehip_run_slice              (.cpp:96-116) stage A of the handle's units, all b layers, all nq queries, into the handle's acc_slice: one
 *                                 launch per group of one to four queries.  Asynchronous, on the handle's stream (not behind the queues of
 *                                 an earlier piehip_run_chain: it touches none of their buffers)
 *   piehip_slice_accumulators_device   device address of acc_slice (valid until the slice or the batch size changes)
 *   piehip_get_slice_accumulators acc_slice to host memory (tests); synchronous
 *   piehip_put_accumulators       (.cpp:117: the accumulators as the chain reads them) rows [bin_lo, bin_hi) of d_src[b][nq][u_hi - u_lo][2][N]
 *                                 -- units [u_lo, u_hi) of ALL b layers, 16-byte aligned, readable by h's device -- into h's accumulators.
 *                                 One launch on h's stream, behind the queues of h's last run_chain; the caller orders the writer of d_src
 *                                 before it.  Where the context hands operand X of the first product to the chain in lane order (batches
 *                                 on rings from 8192), the units of inner hash function 0 land where the unsliced stage A puts them.
 *   piehip_put_accumulators_from  the same from a sliced handle `src` of this process (its acc_slice and unit range): h's stream waits for
 *                                 what src's stream holds at the call (its piehip_run_slice), and src's stream waits for the placement
 *                                 before anything queued on it later.  Same device, or another with peer access enabled
 *   piehip_run_chain(_into)       (.cpp:117-126) everything of run() behind stage A for the handle's bin layers -- transforms, product chain,
 *                                 key switch with the mask multiply (K = 1: the mask multiply), the result-limb reduction, both queues,
 *                                 per-query keys -- with the result rows, result buffer and stream order of piehip_run(_into) on a
 *                                 piehip_load_db_table_bins(bin_lo, bin_hi) handle.  No bin layers: nothing is launched
 * PIEHIP_ESTATE: piehip_run_chain unless every unit 0 .. K L - 1 has been put since the last piehip_run_chain or batch-size change; a put
 * whose range overlaps one already put in this round; piehip_run_slice without its slice inputs; piehip_run(_into / _staged / _host*) and
 * piehip_set_graph(1) on a sliced handle; piehip_attach_database to or from one; the slice calls on an unsliced handle.  PIEHIP_EINVAL:
 * ranges outside [0, K L] or [0, b], u_lo > u_hi, bin_lo > bin_hi.  The slice setters: null input or seeds and q >= nq are PIEHIP_EINVAL, an
 * unsliced handle PIEHIP_ESTATE, all before anything reaches the device; on a handle without units they return PIEHIP_OK and do nothing.
 * A refused call changes nothing.  Loading a whole database
 * (piehip_load_db*, piehip_build_db*) makes the handle an unsliced one again. */
int piehip_query_slice(uint32_t K, uint32_t L, int nranks, int rank, uint32_t *u_lo, uint32_t *u_hi);
int piehip_load_db_table_sliced(piehip_handle h, const uint64_t *tbl, uint32_t k, uint32_t e, uint32_t K, uint32_t b, uint32_t E,
                                uint64_t shuffle_seed, uint64_t mask_seed, uint32_t u_lo, uint32_t u_hi, uint32_t bin_lo, uint32_t bin_hi);
int piehip_build_db_sliced(piehip_handle h, const uint64_t *items, size_t n, uint32_t k, uint32_t e, uint32_t K, uint32_t b, uint32_t E,
                           uint64_t hash_seed, uint64_t evict_seed, uint64_t shuffle_seed, uint64_t mask_seed, uint32_t u_lo, uint32_t u_hi,
                           uint32_t bin_lo, uint32_t bin_hi);
int piehip_load_db_sliced(piehip_handle h, uint32_t K, uint32_t b, uint32_t E, uint32_t u_lo, uint32_t u_hi,
                          const uint64_t *pts_slice /*[u_n][b][E][N]*/, uint32_t bin_lo, uint32_t bin_hi, const uint64_t *masks /*[bin_n][L][N]*/);
int piehip_get_query_slice(piehip_handle h, uint32_t *u_lo, uint32_t *u_hi, uint32_t *bin_lo, uint32_t *bin_hi);
int piehip_set_index_slice_q(piehip_handle h, uint32_t q, const uint64_t *idx_slice /*[u_n][E][2][N]*/);
int piehip_set_minus_slice_q(piehip_handle h, uint32_t q, const uint64_t *minus_slice /*[u_n][2][N]*/);
int piehip_set_index_slice_from_q(piehip_handle h, uint32_t q, const uint64_t *idx /*[K][E][2][L][N]*/);
int piehip_set_minus_slice_from_q(piehip_handle h, uint32_t q, const uint64_t *minus /*[2][L][N]*/);
int piehip_set_index_slice_seeded_q(piehip_handle h, uint32_t q, const uint64_t *c0_slice /*[u_n][E][N]*/, const uint8_t *seeds /*[K][E][32]*/);
int piehip_set_minus_slice_seeded_q(piehip_handle h, uint32_t q, const uint64_t *c0_slice /*[u_n][N]*/, const uint8_t *seed /*[32]*/);
int piehip_set_index_slice_seeded_from_q(piehip_handle h, uint32_t q, const uint64_t *c0idx /*[K][E][L][N]*/, const uint8_t *seeds /*[K][E][32]*/);
int piehip_set_minus_slice_seeded_from_q(piehip_handle h, uint32_t q, const uint64_t *c0minus /*[L][N]*/, const uint8_t *seed /*[32]*/);
int piehip_slice_host_buffers_q(piehip_handle h, uint32_t q, uint64_t **idx /*[K][E][2][L][N]*/, uint64_t **minus /*[2][L][N]*/);
int piehip_set_index_slice_device_q(piehip_handle h, uint32_t q, const void *d_idx_slice);
int piehip_set_minus_slice_device_q(piehip_handle h, uint32_t q, const void *d_minus_slice);
int piehip_run_slice(piehip_handle h);
int piehip_slice_accumulators_device(piehip_handle h, void **d_acc_slice);
int piehip_get_slice_accumulators(piehip_handle h, uint64_t *out /*[b][nq][u_n][2][N]*/);
int piehip_put_accumulators(piehip_handle h, uint32_t u_lo, uint32_t u_hi, const void *d_src /*[b][nq][u_hi - u_lo][2][N]*/);
int piehip_put_accumulators_from(piehip_handle h, piehip_handle src);
int piehip_run_chain(piehip_handle h);
int piehip_run_chain_into(piehip_handle h, void *d_results);

/* ---- FHEHIPPIE: the rotation-based sibling operator ---------------------------------
 * Reference: src/Common/Crypto/PrivateIndexedEqualityCheck/FHEHIPPIE.{hpp,cpp}; one operator per client slot
 * (FHEHIPPIECollection, PIECollection.hpp); `npie` operators are evaluated as one batch here.
 * An operator holds a flat blocked Cuckoo table T[K][b][E] with b == E (FHEHIPPIE.cpp:13-16), packs row (hf, bin)
 * as the E table cells followed by a 1 (FHEHIPPIE.cpp:41-51), and evaluates per hash function
 *   EvalMult(EvalMerge_bin(EvalInnerProduct(index[hf], row[hf][bin], b)), mask[hf])        (FHEHIPPIE.cpp:61-77)
 * where EvalInnerProduct = EvalMult(ct, pt) + ceil(log2 b) rotate-by-2^r-and-add steps and EvalMerge masks
 * slot 0 of ciphertext i and rotates it by -i [OFHE-UNVERIFIED: OpenFHE is not part of the reference tree]. */
/* Galois element 5^index mod 2N of the row rotation by `index` (negative = to the right) */
int piehip_rotation_galois(piehip_handle h, int32_t index, uint32_t *g);
/* rotation keys (EvalSumKeyGen / EvalRotateKeyGen products, SimpleFHEPSIClient.cpp:80-89), BV layout as the
 * relinearisation key: keys[nkeys][L][2][L][N], indices[nkeys] signed rotation amounts.  run() needs
 * 2^r (r < ceil(log2 b)) and -1 .. -(b-1). */
int piehip_load_rotation_keys(piehip_handle h, uint32_t nkeys, const int32_t *indices, const uint64_t *keys);
/* constructor packing (FHEHIPPIE.cpp:23-59) for npie operators: slots[npie][K][b][E+1] (already in the bin
 * order the caller's permutation vector chose), masks[npie][K][b] in [1, t-1]; encoded on the device.
 * PIEHIP_EINVAL if b != E (the reference's invalid_argument). */
int piehip_fhepie_load_table(piehip_handle h, uint32_t npie, uint32_t K, uint32_t b, uint32_t E, const int64_t *slots,
                             const int64_t *masks);
/* setIndex (FHEHIPPIE.hpp:45-48): idx[npie][K][2][L][N] */
int piehip_fhepie_set_index(piehip_handle h, const uint64_t *idx);
/* run() (FHEHIPPIE.cpp:61-77), synchronous; getResultList (FHEHIPPIE.hpp:40-43): out[npie][K][2][L][N] in hash
 * function order (the caller applies its result permutation) */
int piehip_fhepie_run(piehip_handle h);
int piehip_fhepie_get_results(piehip_handle h, uint64_t *out);

/* ---- client-side harness -----------------------------------------------------------------------------
 * Not part of the server hot path: the client role of src/Client/FHE/BatchedFHEPSIClient.cpp, needed to
 * produce the hot path's inputs, to read its outputs and to measure the end-to-end PSI wall-clock
 * (SURVEY.md 8f-1).  Deterministic samplers (xoshiro256** streams seeded per call) run on the host, the
 * polynomial arithmetic on the device.  BFV conventions: secret key uniform ternary; noise centred
 * binomial (sigma 3.16); fresh ciphertext (c0, c1) = (-a s + e + round(Q m / t), a); all in EVALUATION format. */
/* KeyGen (BatchedFHEPSIClient.cpp:88): sk[L][N] */
int piehip_client_keygen(piehip_handle h, uint64_t seed, uint64_t *sk);
/* EvalMultKeyGen (BatchedFHEPSIClient.cpp:91): BV key, evk[L][2][L][N] */
int piehip_client_relin_keygen(piehip_handle h, const uint64_t *sk, uint64_t seed, uint64_t *evk);
/* EvalSumKeyGen / EvalRotateKeyGen (SimpleFHEPSIClient.cpp:80-89): BV key from s(X^g) to s for the row rotation
 * by `index`, rk[L][2][L][N] */
int piehip_client_rot_keygen(piehip_handle h, const uint64_t *sk, int32_t index, uint64_t seed, uint64_t *rk);
/* MakePackedPlaintext + Encrypt(secretKey, .) (BatchedFHEPSIClient.cpp:155-156,161-168) of nct slot vectors
 * slots[nct][B]; seeds[nct] one sampler seed per ciphertext; out[nct][2][L][N] */
int piehip_client_encrypt(piehip_handle h, const uint64_t *sk, const int64_t *slots, uint32_t nct, uint32_t B,
                          const uint64_t *seeds, uint64_t *out);
/* Decrypt + GetPackedValue (BatchedFHEPSIClient.cpp:249-265): ct[nct][2][L][N] -> slots[nct][B] (centred) */
int piehip_client_decrypt(piehip_handle h, const uint64_t *sk, const uint64_t *ct, uint32_t nct, uint32_t B, int64_t *slots);
/* Decryption that also measures the invariant noise budget: what a client runs before it relies on piehip_set_result_limbs,
 * piehip_set_result_relin, piehip_set_chain_limbs or piehip_set_chain_schedule, none of which checks noise.
 * Definition.  Decryption rounds t x / Q coefficient by coefficient, x = c0 + c1 s (+ c2 s^2) in COEFFICIENT format; the device forms
 * the fractional part of t x / Q as fsum, the sum over the limbs of the 60-bit truncated fractions of t y_i / q_i (y_i the CRT digits
 * of x).  For coefficient n of ciphertext c:  f = fsum mod 2^60,  d(c, n) = min(f, 2^60 - f),  and
 *     max_dist[c] = max of d(c, n) over ALL N coefficients, whatever B is
 * -- the largest distance of t x / Q from an integer, in units of 2^-60: decryption is right while it stays below 2^59.
 *   piehip_budget_from_distance  the readout, in bits: 58 for max_dist = 0, otherwise 59 - bitlength(max_dist) clamped to [0, 58], i.e.
 *                                floor(-log2(2 max_dist / 2^60)).  Host arithmetic, no handle.  It is the CPU oracle's readout word
 *                                for word, and like it saturates at 57-58: every limb's fraction is truncated below 2^-60, so a
 *                                noiseless ciphertext of several limbs may read a few units away from 0.
 *   piehip_client_decrypt_budget ct[nct][ncomp][L][N], ncomp = 2 or 3 -> budget[c] = piehip_budget_from_distance(max_dist[c]);
 *                                max_dist[nct] itself where the pointer is not null; slots[nct][B] bit-identical to
 *                                piehip_client_decrypt (ncomp = 2) and piehip_client_decrypt_deg2 (ncomp = 3).  B = 0 (slots may then
 *                                be null): the budgets alone, without the transform mod t and the gather.  Any context: rows reduced
 *                                to keep < L limbs are measured on a context of the chain q[:keep] with the first keep limbs of the key,
 *                                as they are decrypted.
 * A budget of 0 means that some coefficient is at least a quarter away from an integer: the plaintext is not to be trusted.  The number
 * is a MEASUREMENT on one ciphertext under one key, not a worst-case bound: leave a margin for other queries, databases and keys.
 * PIEHIP_EINVAL, before anything reaches the device (budget, max_dist and slots are not written): a null handle, sk, ct or budget;
 * nct = 0; ncomp outside {2, 3}; B > N; null slots with B > 0.  Added without a new version number: look the symbols up. */
int piehip_client_decrypt_budget(piehip_handle h, const uint64_t *sk, const uint64_t *ct /*[nct][ncomp][L][N]*/,
                                 uint32_t nct, uint32_t ncomp /*2 or 3*/, uint32_t B,
                                 int64_t *slots /*[nct][B]; null iff B == 0*/,
                                 int32_t *budget /*[nct]*/, uint64_t *max_dist /*[nct], may be null*/);
int piehip_budget_from_distance(uint64_t max_dist);   /* host only, no handle */

/* ---- seeded ciphertexts: the client uploads c0, the device regenerates c1 ---------------------------------------------------
 * A secret-key ciphertext (c0, c1) = (-a s + e + round(Q m / t), a) -- how the reference client encrypts every query ciphertext
 * (BatchedFHEPSIClient.cpp:156,166) and builds its EvalMult key (:91) -- carries a uniform polynomial a that does not depend on the
 * message.  Sent as a 32-byte seed instead, it halves the query: a C3 query is 14.5 MiB of c0 instead of 29 MiB.
 * Format (a wire format; both sides must agree bit for bit).  A seed stands for a[L][N] in the EVALUATION word order of this ABI (the
 * array piehip_client_encrypt puts into the c1 half; no transform, no permutation).  For limb l (index into the handle's chain
 * q_0..q_{L-1}) and chunk c (0 <= c < ceil(N / 10)):
 *     msg = "PIEHIP-A" || seed[32] || u32le(l) || u32le(c)                   48 bytes
 *     out = SHAKE128(msg), first 160 bytes                                    FIPS 202: one Keccak-f[1600]
 *     a[l][10 c + t] = (bytes 16 t .. 16 t + 15 of out, little-endian) mod q_l,   t = 0..9, 10 c + t < N
 * (128 bits reduced modulo a prime < 2^61: statistical distance < 2^-67 per coefficient, no rejection.)
 *   seeded ciphertext     c0[L][N] + seed[32]
 *   seeded EvalMult key   evk0[L][L][N] (the first component of each of the L rows) + seeds[L][32], one per row
 * SECURITY: seeds must be distinct and drawn from a CSPRNG (32 fresh random bytes per ciphertext / key row).  A repeated seed repeats
 * a, and two ciphertexts with the same a and the same key give away the difference of their messages and noise.  Seeding is sound for
 * SECRET-KEY encryption only (what the reference client does); a public-key ciphertext's c1 is not uniform and cannot be seeded.
 *   piehip_expand_uniform          n seeds -> out[n][L][N] (host memory); synchronous
 *   piehip_expand_uniform_device   the same into caller-owned HBM d_out[n][L][N]; complete on return
 *   piehip_stage_*_seeded_q        the seeded forms of piehip_stage_minus_q / _index_row_q / _index_ct_q: c0 only ([L][N];
 *                                  a row is c0[E][L][N] + seeds[E][32]) goes up into the c0 half of the piece's slot, and the seed is
 *                                  kept.  Order, batches and piehip_stage_reset follow the unseeded calls; seeded and unseeded pieces
 *                                  mix freely in one staging sequence, and staging a piece again in either form replaces it (an
 *                                  unseeded restage is never overwritten by an expansion).  piehip_run_staged queues ONE expansion
 *                                  launch for every seeded piece of the batch, behind the pieces' uploads, in front of the
 *                                  evaluation: the next handle's upload runs while it expands.
 *   piehip_run_host_seeded(_async) exactly: piehip_stage_minus_seeded_q and piehip_stage_index_row_seeded_q for every query and row,
 *                                  then piehip_run_staged; piehip_run_host_wait waits for it.  c0idx[nq][K][E][L][N],
 *                                  idx_seeds[nq][K][E][32], c0minus[nq][L][N], minus_seeds[nq][32], results as piehip_run_host.
 *                                  The page-locked arrays of piehip_host_buffers_q hold the c0 layouts (half of their size):
 *                                  c0idx in `idx`, c0minus in `minus`.
 *   piehip_load_relin_key_seeded(_q)   piehip_load_relin_key(_q) from evk0[L][L][N] + seeds[L][32]
 *   piehip_client_encrypt_seeded   piehip_client_encrypt with a = expand(a_seeds[c]) and the noise drawn from noise_seeds[c];
 *                                  writes c0[nct][L][N]
 *   piehip_client_relin_keygen_seeded  piehip_client_relin_keygen with a_i = expand(a_seeds[i]), the noise drawn from `seed`;
 *                                  writes evk0[L][L][N]
 * Null seeds and positions outside the index matrix or the batch are PIEHIP_EINVAL before anything reaches the device.
 * A sharded server's piehip_rccl_broadcast_query refuses (PIEHIP_ESTATE) a staged query with seeded pieces. */
int piehip_expand_uniform(piehip_handle h, const uint8_t *seeds /*[n][32]*/, uint32_t n, uint64_t *out /*[n][L][N]*/);
int piehip_expand_uniform_device(piehip_handle h, const uint8_t *seeds /*[n][32]*/, uint32_t n, void *d_out /*[n][L][N]*/);
int piehip_stage_minus_seeded_q(piehip_handle h, uint32_t q, const uint64_t *c0 /*[L][N]*/, const uint8_t *seed /*[32]*/);
int piehip_stage_index_row_seeded_q(piehip_handle h, uint32_t q, uint32_t row, const uint64_t *c0 /*[E][L][N]*/,
                                    const uint8_t *seeds /*[E][32]*/);
int piehip_stage_index_ct_seeded_q(piehip_handle h, uint32_t q, uint32_t row, uint32_t j, const uint64_t *c0 /*[L][N]*/,
                                   const uint8_t *seed /*[32]*/);
int piehip_run_host_seeded_async(piehip_handle h, const uint64_t *c0idx, const uint8_t *idx_seeds, const uint64_t *c0minus,
                                 const uint8_t *minus_seeds, uint64_t *results);
int piehip_run_host_seeded(piehip_handle h, const uint64_t *c0idx, const uint8_t *idx_seeds, const uint64_t *c0minus,
                           const uint8_t *minus_seeds, uint64_t *results);
int piehip_load_relin_key_seeded(piehip_handle h, const uint64_t *evk0 /*[L][L][N]*/, const uint8_t *seeds /*[L][32]*/);
int piehip_load_relin_key_seeded_q(piehip_handle h, uint32_t q, const uint64_t *evk0, const uint8_t *seeds);
int piehip_client_encrypt_seeded(piehip_handle h, const uint64_t *sk, const int64_t *slots, uint32_t nct, uint32_t B,
                                 const uint64_t *noise_seeds /*[nct]*/, const uint8_t *a_seeds /*[nct][32]*/,
                                 uint64_t *c0 /*[nct][L][N]*/);
int piehip_client_relin_keygen_seeded(piehip_handle h, const uint64_t *sk, uint64_t seed, const uint8_t *a_seeds /*[L][32]*/,
                                      uint64_t *evk0 /*[L][L][N]*/);

/* ---- measurement ------------------------------------------------------------------------------
 * With profiling on, run() brackets every kernel launch with HIP events on the handle's stream.
 * piehip_profile_read returns, per kernel class, the launch count, total milliseconds, and the
 * algorithmic bytes (SURVEY.md 8d formulas) of the last run. */
#define PIEHIP_NKERNELS 18
enum {
    PIEHIP_K_STAGE_A = 0,   /* fused ct x pt multiply-accumulate + minus add  (A3+A4)          */
    PIEHIP_K_NTT_FWD = 1,   /* forward negacyclic NTT                          (A1)             */
    PIEHIP_K_NTT_INV = 2,   /* inverse negacyclic NTT                          (A1)             */
    PIEHIP_K_EXPAND = 3,    /* Q->QP extension and P/Q scaling                 (A6)             */
    PIEHIP_K_TENSOR = 4,    /* tensor product over QP                          (A5 step 4)      */
    PIEHIP_K_SCALE = 5,     /* scale-and-round by t/P                          (A6)             */
    PIEHIP_K_DIGITS = 6,    /* BV digit decomposition                          (A7)             */
    PIEHIP_K_RELIN = 7,     /* key-switch multiply-accumulate (+ mask multiply) (A7, A3)        */
    PIEHIP_K_MASK = 8,      /* final ct x pt mask multiply when not fused                       */
    PIEHIP_K_ENCODE = 9,    /* packed encoding                                 (A2)             */
    PIEHIP_K_AUTOMORPH = 10,/* automorphism permutation                        (A9)             */
    PIEHIP_K_OTHER = 11,
    PIEHIP_K_EVENT_PAIR = 12,/* no launch: the two events of a bracket back to back -- what the bracket itself reads on this stream */
    PIEHIP_K_TENSOR_NTT_INV = 13,/* tensor product formed in the load phase of the inverse NTT that follows it: one launch in place of
                                  * a PIEHIP_K_TENSOR and a PIEHIP_K_NTT_INV launch (bytes: the tensor product's, 8N * 7M per row).
                                  * A class of its own: it does a product's arithmetic, so it is not a transform for a roofline */
    PIEHIP_K_RESULT_NTT_INV = 14,/* result limbs: inverse transform of the result rows, standard order in and out (bytes 16 N per limb) */
    PIEHIP_K_LIMB_DROP = 15,     /* result limbs: the coefficient-wise limb-drop kernel (bytes: 8 N (L + keep) per polynomial)       */
    PIEHIP_K_DEG2_FINISH = 17,   /* result relinearisation off: own-limb terms + mask multiply of the last product's three components
                                  * (bytes: 8 N per limb: 3 in, 4 operands, 1 mask, 3 out) */
    PIEHIP_K_RESULT_NTT_FWD = 16 /* result limbs: forward transform of the kept limbs.  Classes of their own: the reduction's cost is
                                  * read off these three, and the transforms of the multiplication chain keep their roofline class   */
};
/* times `iters` back-to-back NTT launches over nlimbs random limbs (moduli cycle over mod_count from 0);
 * flags: bit 0 = inverse transform, bit 1 = EVALUATION side in the library's internal lane order.
 * Returns the average milliseconds per launch.  Used by bench tooling to sweep batch sizes. */
int piehip_bench_ntt(piehip_handle h, uint32_t nlimbs, uint32_t mod_count, int flags, uint32_t iters, double *ms_per_launch);
int piehip_set_profiling(piehip_handle h, int on);
/* piehip_profile_read_n fills the first min(n, PIEHIP_NKERNELS) entries of the caller's arrays: pass the length the caller was
 * BUILT with, so that a library with more classes never writes past them (piehip_version() >= 101).
 * piehip_profile_read is the entry point of version 100 and keeps that version's contract: exactly PIEHIP_NKERNELS_V100 = 12
 * entries, the kernel classes only.  Class 12 (PIEHIP_K_EVENT_PAIR) is not a kernel -- it is what an event bracket reads with
 * nothing between its two events -- and must not be added to a sum of kernel times. */
#define PIEHIP_NKERNELS_V100 12
int piehip_profile_read_n(piehip_handle h, uint32_t n, uint32_t *launches /*[n]*/, double *ms /*[n]*/, double *alg_bytes /*[n]*/);
int piehip_profile_read(piehip_handle h, uint32_t *launches /*[12]*/, double *ms /*[12]*/, double *alg_bytes /*[12]*/);
const char *piehip_kernel_name(int k);

#ifdef __cplusplus
}
#endif
#endif
