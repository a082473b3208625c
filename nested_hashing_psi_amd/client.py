"""Client-side harness: the role of the reference's BatchedFHEPSIClient
(src/Client/FHE/BatchedFHEPSIClient.cpp), enough to drive the server hot path with real inputs, read
its outputs and measure the end-to-end PSI wall-clock.  Harness, not the product:
the product is the server path.  Hashing of the (small) client set runs on the host; BFV key
generation, encryption and decryption run on the device through the C ABI (piehip_client_*).
"""
import ctypes as C
import hashlib
import secrets

import numpy as np

from ._lib import i32p, i64p, lib, u8p, u64p
from .pie import _check, _u64, tabulation_hash


def _out(shape, dtype):
    """output buffer for a device-to-host copy, pages touched here: a calloc'ed (np.zeros) array is faulted in page by
    page inside the copy, ~25 ms for the 30 MiB of one query's ciphertexts"""
    a = np.empty(shape, dtype=dtype)
    a.fill(0)
    return a


def harness_seeds(base, n, tag):
    """n 32-byte seeds of seeded ciphertexts / key rows, as an [n][32] uint8 array.  base=None: from the OS CSPRNG, as real use
    must (seeds distinct and unpredictable: include/piehip.h).  An integer base derives them reproducibly -- SHA-256 of
    (tag, base, i) -- for tests and benchmarks only: a client whose seeds can be guessed or repeat gives its queries away."""
    if base is None:
        return np.frombuffer(secrets.token_bytes(32 * n), dtype=np.uint8).reshape(n, 32).copy()
    out = np.empty((n, 32), dtype=np.uint8)
    for i in range(n):
        out[i] = np.frombuffer(hashlib.sha256(b"piehip-harness-seed|%s|%d|%d" % (tag.encode(), int(base), i)).digest(), dtype=np.uint8)
    return out


PLAINTEXT_MODULI = {16: 65537, 32: 4296540161, 40: 1099579260929, 48: 281474981953537}


def select_parameters(bitSize, eachCuckooTableSize):
    """The reference client's scheme parameters (BatchedFHEPSIClient.cpp:22-57,72-78): plaintext modulus by item bit size
    (ValueError as the reference's invalid_argument otherwise), multiplicative depth 3 / 5 / 10 by inner table size, ring
    dimension 16384.  The number of 60-bit primes OpenFHE derives from the depth is not in the reference tree
    [OFHE-UNVERIFIED]: depth 3 with the 33-bit modulus is the 4-prime chain BASELINE.json names; deeper settings take one
    prime per level plus one."""
    if bitSize not in PLAINTEXT_MODULI:
        raise ValueError("Error: FHE can only support bit sizes 16 or 32.")
    depth = 3 if eachCuckooTableSize < 500 else (5 if eachCuckooTableSize < 5000 else 10)
    return dict(N=16384, t=PLAINTEXT_MODULI[bitSize], depth=depth, L=depth + 1)


class BatchedFHEPSIClient:
    """Mirror of BatchedFHEPSIClient (BatchedFHEPSIClient.cpp:14-193): runSetUpPhase, runOfflinePhase,
    the online-phase result extraction.  No TCP: the caller moves the arrays.

    layerTiling=R: the client of a server whose database packs R bin layers per plaintext (include/piehip.h "Layer tiling").  Every
    query vector is its k*e slots repeated R times; the server answers with ceil(b / R) ciphertexts whose block r of k*e slots is
    bin layer g*R + r, and the blocks behind the last bin layer are ignored."""

    def __init__(self, cryptoContext, numberOfSimpleHashFunctions, eachSimpleTableSize, numberOfCuckooHashFunctions,
                 eachCuckooTableSize, maxItemsPerPosition, hashSeed=987654321, layerTiling=1):
        self.cc = cryptoContext
        self.k, self.e = numberOfSimpleHashFunctions, eachSimpleTableSize
        self.K, self.E, self.b = numberOfCuckooHashFunctions, eachCuckooTableSize, maxItemsPerPosition
        self.hashSeed = hashSeed
        self.B = self.k * self.e
        self.R = int(layerTiling)
        if self.R < 1 or self.R * self.B > self.cc.N:
            raise ValueError("layerTiling: between 1 and N // (k*e) bin layers per ciphertext")

    # -- setup (BatchedFHEPSIClient.cpp:88-91): KeyGen + EvalMultKeyGen
    def runSetUpPhase(self, keySeed=11, evalKeySeed=12):
        cc = self.cc
        self.sk = _out((cc.L, cc.N), np.uint64)
        _check(lib().piehip_client_keygen(cc._h, keySeed, self.sk.ctypes.data_as(u64p)))
        self.evalMultKey = _out((cc.L, 2, cc.L, cc.N), np.uint64)
        _check(lib().piehip_client_relin_keygen(cc._h, self.sk.ctypes.data_as(u64p), evalKeySeed,
                                                self.evalMultKey.ctypes.data_as(u64p)))
        return self.evalMultKey

    # -- the same with a seeded EvalMult key: evk0[L][L][N] + one seed per row (include/piehip.h "Seeded ciphertexts").
    #    aSeedBase: harness_seeds (None = CSPRNG)
    def runSetUpPhaseSeeded(self, keySeed=11, evalKeySeed=12, aSeedBase=None):
        cc = self.cc
        self.sk = _out((cc.L, cc.N), np.uint64)
        _check(lib().piehip_client_keygen(cc._h, keySeed, self.sk.ctypes.data_as(u64p)))
        self.evalMultKeySeeds = harness_seeds(aSeedBase, cc.L, "evk")
        self.evalMultKey0 = _out((cc.L, cc.L, cc.N), np.uint64)
        _check(lib().piehip_client_relin_keygen_seeded(cc._h, self.sk.ctypes.data_as(u64p), evalKeySeed,
                                                       self.evalMultKeySeeds.ctypes.data_as(u8p), self.evalMultKey0.ctypes.data_as(u64p)))
        return self.evalMultKey0, self.evalMultKeySeeds

    # -- EvalSumKeyGen + EvalRotateKeyGen of the rotation-based sibling (SimpleFHEPSIClient.cpp:80-89): keys for the
    #    rotations 2^r (r < ceil(log2 b)) and -1 .. -(b-1) that FHEHIPPIE::run needs
    def rotationKeyGen(self, nbins, seedBase=50):
        cc = self.cc
        R = 0
        while (1 << R) < nbins:
            R += 1
        rots = [1 << r for r in range(R)] + [-i for i in range(1, nbins)]
        keys = {}
        for i, r in enumerate(rots):
            rk = _out((cc.L, 2, cc.L, cc.N), np.uint64)
            _check(lib().piehip_client_rot_keygen(cc._h, self.sk.ctypes.data_as(u64p), r, seedBase + i, rk.ctypes.data_as(u64p)))
            keys[r] = rk
        return keys

    # -- client Cuckoo table: CuckooHashTable(hash, e, k, startingHashId 0, stash 0, multi, 1 layer)
    #    (BatchedFHEPSIClient.cpp:97-99, insertAll at :109; insert at CuckooHashTable.cpp:72-114)
    def _hash_client_set(self, items):
        items = np.ascontiguousarray(items, dtype=np.uint64)
        table = np.zeros((self.k, self.e), dtype=np.uint64)
        _check(lib().piehip_client_cuckoo_table(self.hashSeed, self.k + self.K, self.k, self.e, items.ctypes.data_as(u64p), len(items),
                                                table.ctypes.data_as(u64p)))
        return table

    # -- offline (BatchedFHEPSIClient.cpp:107-169): index matrix + minus vector, secret-key encrypted
    def runOfflinePhase(self, clientSet, encSeedBase=100):
        K, E = self.K, self.E
        vecs = self._query_vectors(clientSet)
        seeds = np.array([encSeedBase - 1] + [encSeedBase + i for i in range(K * E)], dtype=np.uint64)
        cts = self._encrypt(vecs, seeds)
        self.encryptedMinusElements = cts[0]
        self.batchedEncryptedIndexMatrix = cts[1:].reshape(K, E, 2, self.cc.L, self.cc.N)
        return self.encryptedMinusElements, self.batchedEncryptedIndexMatrix

    def _query_vectors(self, clientSet):
        """the plaintext vectors of one query, [1 + K*E][R*B]: the minus vector (dummy slot: +1, all-zero index column, :128-131),
        then the index matrix; each is its B slots repeated R times.  plainIndex / plainMinus keep the B slots"""
        self.clientTable = self._hash_client_set(clientSet)
        k, e, K, E, B = self.k, self.e, self.K, self.E, self.B
        flat = self.clientTable.reshape(-1)
        index = np.zeros((K, E, B), dtype=np.int64)
        minus = np.ones(B, dtype=np.int64)
        occ = np.nonzero(flat)[0]
        if len(occ):
            minus[occ] = -flat[occ].astype(np.int64)
            for hf in range(K):
                hi = tabulation_hash(self.hashSeed, k + K, k + hf, flat[occ]) % np.uint64(E)
                index[hf, hi.astype(np.int64), occ] = 1
        self.plainIndex, self.plainMinus = index, minus
        return np.tile(np.concatenate([minus.reshape(1, B), index.reshape(K * E, B)]), (1, self.R))

    # -- the offline phase with seeded ciphertexts: c0 halves + one 32-byte seed per ciphertext; the server expands the c1 halves.
    #    Returns (minus c0 [L][N], minus seed [32], index c0 [K][E][L][N], index seeds [K][E][32]).  encSeedBase draws the noise as in
    #    runOfflinePhase; aSeedBase: harness_seeds (None = CSPRNG)
    def runOfflinePhaseSeeded(self, clientSet, encSeedBase=100, aSeedBase=None):
        K, E, cc = self.K, self.E, self.cc
        vecs = np.ascontiguousarray(self._query_vectors(clientSet), dtype=np.int64)
        n = vecs.shape[0]
        noise = np.array([encSeedBase - 1] + [encSeedBase + i for i in range(K * E)], dtype=np.uint64)
        aseeds = harness_seeds(aSeedBase, n, "query")
        c0 = _out((n, cc.L, cc.N), np.uint64)
        _check(lib().piehip_client_encrypt_seeded(cc._h, self.sk.ctypes.data_as(u64p), vecs.ctypes.data_as(i64p), n, vecs.shape[1],
                                                  noise.ctypes.data_as(u64p), aseeds.ctypes.data_as(u8p), c0.ctypes.data_as(u64p)))
        return c0[0], aseeds[0].copy(), c0[1:].reshape(K, E, cc.L, cc.N), aseeds[1:].reshape(K, E, 32).copy()

    def _encrypt(self, vecs, seeds):
        cc = self.cc
        v = np.ascontiguousarray(vecs, dtype=np.int64)
        out = _out((v.shape[0], 2, cc.L, cc.N), np.uint64)
        s = np.ascontiguousarray(seeds, dtype=np.uint64)
        _check(lib().piehip_client_encrypt(cc._h, self.sk.ctypes.data_as(u64p), v.ctypes.data_as(i64p), v.shape[0], v.shape[1],
                                           s.ctypes.data_as(u64p), out.ctypes.data_as(u64p)))
        return out

    def _reduced_context(self, limbs):
        """the context (N, limbs, t, q[:limbs]) that decrypts results the server reduced to `limbs` limbs (setResultLimbs), made
        once per limb count and kept.  A context wants an auxiliary basis too: the next limbs + 1 primes of this context's chain
        (decryption never touches them)."""
        cache = self.__dict__.setdefault("_reduced", {})
        if limbs not in cache:
            cc = self.cc
            chain = [int(v) for v in cc.moduli[:cc.M]]
            cache[limbs] = type(cc)(cc.N, limbs, cc.t, chain[:limbs], chain[limbs:2 * limbs + 1])
        return cache[limbs]

    def _decrypt_operands(self, cts, limbs):
        """(array, its pointer, handle, key) of a decryption on `limbs` limbs"""
        cc = self.cc
        a, ap = _u64(cts)
        limbs = cc.L if limbs is None else int(limbs)
        if not 1 <= limbs <= cc.L:
            raise ValueError("limbs must be between 1 and L")
        if a.ndim != 4 or a.shape[1] not in (2, 3) or a.shape[2:] != (limbs, cc.N):
            raise ValueError("ciphertexts must be [n][2][%d][N] (or [n][3][%d][N]: not relinearised)" % (limbs, limbs))
        h, sk = cc._h, self.sk
        if limbs < cc.L:
            h, sk = self._reduced_context(limbs)._h, np.ascontiguousarray(self.sk[:limbs])
        return a, ap, h, sk

    def decrypt(self, cts, nslots=None, limbs=None, budget=False):
        """cts [n][2][L][N] -> slots [n][nslots].  limbs = keep < L: cts [n][2][keep][N] as a server with setResultLimbs(keep)
        returns them, decrypted in the reduced context with the first `keep` limbs of the secret key.  Three-component rows
        [n][3][..][N] (a server with setResultRelin(False)) are recognised by their shape and decrypt as c0 + c1 s + c2 s^2.
        budget=True: (slots, budgets), budgets [n] int32 the invariant noise budget of every ciphertext in bits
        (piehip_client_decrypt_budget: measured on these ciphertexts under this key, not a bound)."""
        a, ap, h, sk = self._decrypt_operands(cts, limbs)
        n = a.shape[0]
        nslots = nslots or self.R * self.B
        out = _out((n, nslots), np.int64)
        if budget:
            bud = _out((n,), np.int32)
            _check(lib().piehip_client_decrypt_budget(h, sk.ctypes.data_as(u64p), ap, n, a.shape[1], nslots, out.ctypes.data_as(i64p),
                                                      bud.ctypes.data_as(i32p), None))
            return out, bud
        dec = lib().piehip_client_decrypt_deg2 if a.shape[1] == 3 else lib().piehip_client_decrypt
        _check(dec(h, sk.ctypes.data_as(u64p), ap, n, nslots, out.ctypes.data_as(i64p)))
        return out

    def noiseBudget(self, cts, limbs=None):
        """the smallest invariant noise budget among the ciphertexts, in bits; nothing is decoded (the B = 0 form of
        piehip_client_decrypt_budget).  0: some ciphertext is not to be trusted"""
        a, ap, h, sk = self._decrypt_operands(cts, limbs)
        n = a.shape[0]
        bud = _out((n,), np.int32)
        _check(lib().piehip_client_decrypt_budget(h, sk.ctypes.data_as(u64p), ap, n, a.shape[1], 0, None, bud.ctypes.data_as(i32p), None))
        return int(bud.min())

    # -- online (BatchedFHEPSIClient.cpp:176-192): zero slot in any of the b results <=> item in the intersection
    def extractIntersection(self, resultList, limbs=None):
        dec = self.decrypt(resultList, limbs=limbs)
        if self.R > 1:   # row g, block r is bin layer g*R + r; the blocks behind layer b - 1 are not bin layers
            dec = dec.reshape(dec.shape[0] * self.R, self.B)[:self.b]
        self.batchedDecryptedResult = dec
        flat = self.clientTable.reshape(-1)
        hit = (self.batchedDecryptedResult == 0).any(axis=0)
        return flat[hit].copy()
