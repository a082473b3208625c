"""The client kernels (kernels_client.hip, piehip_client.cpp: key generation, encryption, decryption) on crafted phases, messages and
keys, bit for bit against the oracle.

The other GPU tests decrypt honest ciphertexts, whose phase sits dozens of bits from a rounding tie, and encrypt honest 0/1 index
vectors.  Here decryption gets the phases of coeff_columns.decrypt_families planted in ciphertexts -- CRT digits at their extremes,
values a few units of 2^-60 from a tie of round(t x/Q), the wrap t -> 0 and the steps around t/2 -- and encryption gets messages whose
[Q m]_t sits on every branch of the message term.  tests/test_client_columns.py shows on the CPU that these inputs are where claimed,
holds the oracle to exact arithmetic on them, and restates the samplers; what is imported from there is checked there.

Small ring (N = 64): every chain of tests/param_chains.py at L = 1, 2, 3, 7 and every plaintext modulus the chain allows, one context
per case (the `small` fixture; pytest runs a context's tests together).  Then one case per route of ntt_plan_decide at the rings of
tests/test_gpu_result_limbs.py::LARGE and below, and the reduced contexts of setResultLimbs.  No tolerance and no skip.
"""
import numpy as np
import pytest

from oracle import exact as ex
from tests import coeff_columns as ccol
from tests.param_chains import T16, T32
from tests.test_client_columns import CASES, N, key_noise, key_sources, make_oracle, sampled_rows, seeded_c0
from tests.test_result_limbs import reduced_oracle

pytestmark = pytest.mark.gpu

INT64_MIN = -(1 << 63)


# ---- the C ABI of the client, called directly --------------------------------------------------------------------------------------
def _api():
    from nested_hashing_psi_amd._lib import i64p, lib, u8p, u64p
    return lib(), u64p, i64p, u8p


def _ok(rc):
    from nested_hashing_psi_amd.pie import _check
    _check(rc)


def dev_keygen(cc, seed):
    L_, u64p, _, _ = _api()
    sk = np.zeros((cc.L, cc.N), dtype=np.uint64)
    _ok(L_.piehip_client_keygen(cc._h, seed, sk.ctypes.data_as(u64p)))
    return sk


def dev_ks_keygen(cc, sk, seed, index=None):
    """the relinearisation key, or the rotation key of `index`"""
    L_, u64p, _, _ = _api()
    key = np.zeros((cc.L, 2, cc.L, cc.N), dtype=np.uint64)
    if index is None:
        _ok(L_.piehip_client_relin_keygen(cc._h, sk.ctypes.data_as(u64p), seed, key.ctypes.data_as(u64p)))
    else:
        _ok(L_.piehip_client_rot_keygen(cc._h, sk.ctypes.data_as(u64p), index, seed, key.ctypes.data_as(u64p)))
    return key


def dev_relin_keygen_seeded(cc, sk, seed, a_seeds):
    L_, u64p, _, u8p = _api()
    evk0 = np.zeros((cc.L, cc.L, cc.N), dtype=np.uint64)
    _ok(L_.piehip_client_relin_keygen_seeded(cc._h, sk.ctypes.data_as(u64p), seed, a_seeds.ctypes.data_as(u8p), evk0.ctypes.data_as(u64p)))
    return evk0


def dev_encrypt_rc(cc, sk, slots, seeds):
    """piehip_client_encrypt on slots [nct][B]: (return code, ciphertexts [nct][2][L][N])"""
    L_, u64p, i64p, _ = _api()
    s = np.ascontiguousarray(slots, dtype=np.int64)
    sd = np.ascontiguousarray(seeds, dtype=np.uint64)
    assert s.ndim == 2 and sd.shape == (s.shape[0],)
    out = np.zeros((s.shape[0], 2, cc.L, cc.N), dtype=np.uint64)
    rc = L_.piehip_client_encrypt(cc._h, sk.ctypes.data_as(u64p), s.ctypes.data_as(i64p), s.shape[0], s.shape[1], sd.ctypes.data_as(u64p),
                                  out.ctypes.data_as(u64p))
    return rc, out


def dev_encrypt(cc, sk, slots, seeds):
    rc, out = dev_encrypt_rc(cc, sk, slots, seeds)
    _ok(rc)
    return out


def dev_encrypt_seeded(cc, sk, slots, noise_seeds, a_seeds):
    """the c0 halves [nct][L][N]"""
    L_, u64p, i64p, u8p = _api()
    s = np.ascontiguousarray(slots, dtype=np.int64)
    sd = np.ascontiguousarray(noise_seeds, dtype=np.uint64)
    assert s.ndim == 2 and sd.shape == (s.shape[0],) and a_seeds.shape == (s.shape[0], 32)
    c0 = np.zeros((s.shape[0], cc.L, cc.N), dtype=np.uint64)
    _ok(L_.piehip_client_encrypt_seeded(cc._h, sk.ctypes.data_as(u64p), s.ctypes.data_as(i64p), s.shape[0], s.shape[1], sd.ctypes.data_as(u64p),
                                        a_seeds.ctypes.data_as(u8p), c0.ctypes.data_as(u64p)))
    return c0


def dev_decrypt(cc, sk, cts, B):
    """cts [nct][2 or 3][L][N] as ONE batch -> slots [nct][B]"""
    L_, u64p, i64p, _ = _api()
    a = np.ascontiguousarray(cts, dtype=np.uint64)
    assert a.ndim == 4 and a.shape[1] in (2, 3) and a.shape[2:] == (cc.L, cc.N)
    out = np.zeros((a.shape[0], B), dtype=np.int64)
    fn = L_.piehip_client_decrypt_deg2 if a.shape[1] == 3 else L_.piehip_client_decrypt
    _ok(fn(cc._h, sk.ctypes.data_as(u64p), a.ctypes.data_as(u64p), a.shape[0], B, out.ctypes.data_as(i64p)))
    return out


def want_slots(o, sk, cts, B):
    return np.stack([o.decode(o.decrypt(sk, ct)[0], B) for ct in cts])


def a_seeds_of(n, tag):
    from nested_hashing_psi_amd.client import harness_seeds
    return harness_seeds(tag, n, "client-columns")


def _context(pie, o):
    cc = pie.PieContext(o.N, o.L, o.t, o.q, o.p)
    assert (cc.moduli == o.moduli).all()
    return cc


@pytest.fixture(scope="module", params=[pytest.param(p.values, id=p.id) for p in CASES])
def small(request, ob, pie_mod):
    """(oracle, device context) of one small-ring case; made once for the tests below"""
    L, chain, t = request.param
    o = make_oracle(ob, L, chain, t)
    cc = _context(pie_mod, o)
    yield o, cc
    cc.close()


def worst_key(o):
    """not a key anyone samples, but the ABI takes any residues: every residue q_i - 1 (the polynomial -1) drives the products of
    dec_dot_kernel to their largest"""
    return np.stack([np.full(o.N, int(q) - 1, dtype=np.uint64) for q in o.q])


# ---- small ring: decryption of planted phases ------------------------------------------------------------------------------------
def planted_batches(o, polys, sk, rng):
    """[(key, ciphertexts [n][2 or 3][L][N])]: the phases `polys` with c1 = 0 and with c1 uniform under sk (one batch), with three
    components (c1, c2 uniform and c1 = 0, c2 uniform), and both again under worst_key"""
    qs, _ = ccol.moduli(o)

    def u():
        return ccol.uniform_poly(qs, o.N, rng)
    zero = np.zeros((o.L, o.N), dtype=np.uint64)
    wk = worst_key(o)
    return [(sk, np.stack([ccol.phase_ct(o, X) for X in polys] + [ccol.phase_ct(o, X, sk, u()) for X in polys])),
            (sk, np.stack([ccol.phase_ct(o, X, sk, u(), u()) for X in polys] + [ccol.phase_ct(o, X, sk, zero, u()) for X in polys])),
            (wk, np.stack([ccol.phase_ct(o, X, wk, u()) for X in polys] + [ccol.phase_ct(o, X) for X in polys])),
            (wk, np.stack([ccol.phase_ct(o, X, wk, u(), u()) for X in polys] + [ccol.phase_ct(o, X, wk, zero, u()) for X in polys]))]


def test_decrypt_planted_phases(small):
    """dec_dot_kernel (two and three components), the inverse transform, dec_round_kernel and decode_gather_kernel on every column of
    decrypt_families, in as many polynomials as the columns need, each batch decrypted in one call; B = N reads every coefficient"""
    o, cc = small
    qs, _ = ccol.moduli(o)
    rng = np.random.default_rng(o.L + o.t % 1000)
    fam = ccol.decrypt_families(o)
    cols = [c for v in fam.values() for c in v]
    polys = ccol.columns_polys(cols, qs, N)
    sk = o.keygen(41 + o.L)
    batches = planted_batches(o, polys, sk, rng)
    coeff = np.stack([o.decrypt(sk, ccol.phase_ct(o, X))[0] for X in polys])
    for key, cts in batches:                            # every form holds the same phases
        assert cts.shape[0] == 2 * len(polys)
        assert (np.stack([o.decrypt(key, ct)[0] for ct in cts]) == np.concatenate([coeff, coeff])).all()
    for B in (1, 7, N // 2, N):
        for b, (key, cts) in enumerate(batches):
            got = dev_decrypt(cc, key, cts, B)
            bad = np.argwhere(got != want_slots(o, key, cts, B))
            assert not len(bad), "batch %d, B = %d: %d slots differ, first (ciphertext, slot) = %r" % (b, B, len(bad), tuple(bad[0]))
    print("L=%d t=2^%d q=%s: %d columns (%s) in %d polynomial(s), 4 forms x 4 slot counts"
          % (o.L, o.t.bit_length() - 1, [q.bit_length() for q in qs], len(cols), ", ".join("%s %d" % (k, len(v)) for k, v in fam.items()), len(polys)))


# ---- small ring: encryption of crafted messages ------------------------------------------------------------------------------------
def edge_slot_rows(t):
    """{B: slot rows [n][B]} holding +-(t - 1)/2, +-1, 0 and +-(t - 1): seven values, all in the one slot of B = 1, in the seven of
    B = 7 (and rotated by three), cycled over B = N (and negated, shifted by one)"""
    h = (t - 1) // 2
    v = [h, -h, 1, -1, 0, t - 1, -(t - 1)]
    return {1: np.array(v, dtype=np.int64).reshape(7, 1),
            7: np.array([v, v[3:] + v[:3]], dtype=np.int64),
            N: np.array([[v[i % 7] for i in range(N)], [-v[(i + 1) % 7] for i in range(N)]], dtype=np.int64)}


def test_encrypt_crafted_messages(small):
    """encode_scatter_kernel, the transform mod t, enc_message_kernel and enc_finish_kernel: messages with [Q m]_t on every branch of
    the message term (slots over all N positions) and slot vectors at the edges of the slot range, B = 1, 7, N.  The seeded form takes
    its second component from expand_uniform and draws the error first; the device then decrypts what it encrypted"""
    o, cc = small
    qs, _ = ccol.moduli(o)
    sk = o.keygen(43 + o.L)
    rows = edge_slot_rows(o.t)
    rows[N] = np.concatenate([o.decode(ccol.enc_message_coeffs(o, N), N).reshape(1, N), rows[N]])
    for B, slots in rows.items():
        n = slots.shape[0]
        seeds = np.arange(500 + 10 * B, 500 + 10 * B + n, dtype=np.uint64)
        got = dev_encrypt(cc, sk, slots, seeds)
        for c in range(n):
            assert (got[c] == o.encrypt_slots(sk, slots[c], int(seeds[c]))).all(), "B = %d, ciphertext %d" % (B, c)
        aseeds = a_seeds_of(n, B)
        a = cc.expand_uniform(aseeds)
        c0 = dev_encrypt_seeded(cc, sk, slots, seeds, aseeds)
        for c in range(n):
            e = sampled_rows(o, int(seeds[c]), uniform=False)[0][1]
            assert (c0[c] == seeded_c0(o, sk, slots[c], a[c], e)).all(), "seeded, B = %d, ciphertext %d" % (B, c)
        if ex.prod(qs) >= 64 * o.t:
            want = np.where(np.abs(slots) == o.t - 1, -np.sign(slots), slots)          # +-(t - 1) is -+1 (mod t)
            assert (dev_decrypt(cc, sk, got, B) == want).all(), "B = %d: the device does not decrypt its own ciphertexts" % B
            assert (dev_decrypt(cc, sk, np.stack([c0, a], axis=1), B) == want).all(), "B = %d, seeded" % B


# ---- small ring: keys ----------------------------------------------------------------------------------------------------------------
def test_keys(small):
    """piehip_client_keygen, ks_finish_kernel behind square_kernel (relinearisation) and behind the permuted secret (rotations 1, -1, 2,
    N/4) equal the oracle's; the seeded relinearisation key has the structure tests/test_client_columns.py holds the oracle's keys to,
    with a_i = expand_uniform(seed_i) and the error polynomials drawn one after the other"""
    o, cc = small
    sk = o.keygen(45 + o.L)
    assert (dev_keygen(cc, 45 + o.L) == sk).all()
    for s in (sk, worst_key(o)):
        assert (dev_ks_keygen(cc, s, 46) == o.relin_keygen(s, 46)).all()
    for index in (1, -1, 2, N // 4):
        g = o.rot_index(index)
        assert cc.rotation_galois(index) == g
        assert (dev_ks_keygen(cc, sk, 47 + index, index=index) == o.rot_keygen(sk, g, 47 + index)).all(), "rotation %d" % index
    aseeds = a_seeds_of(o.L, 9)
    a = cc.expand_uniform(aseeds)
    evk0 = dev_relin_keygen_seeded(cc, sk, 48, aseeds)
    es = key_noise(o, sk, evk0, key_sources(o, sk)["relin"][1], a=a)
    assert es == [e for _, e in sampled_rows(o, 48, rows=o.L, uniform=False)]


# ---- small ring: encoding --------------------------------------------------------------------------------------------------------------
def test_encode_edge_coefficients(small):
    """piehip_encode (encode_scatter_kernel, the transform mod t, encode_lift_kernel): plaintexts whose COEFFICIENTS cycle through 0, 1,
    (t - 1)/2, (t + 1)/2, t - 1 -- the lift changes sign between the middle two -- each value at every position in one of five vectors"""
    o, cc = small
    t = o.t
    v = [0, 1, (t - 1) // 2, (t + 1) // 2, t - 1]
    slots = np.stack([o.decode(np.array([v[(n + r) % 5] for n in range(N)], dtype=np.uint64), N) for r in range(5)])
    for r in range(5):
        assert [int(c) for c in o.encode(slots[r])[0]] == [v[(n + r) % 5] for n in range(N)]
    assert (cc.MakePackedPlaintext(slots) == np.stack([o.encode_eval(s) for s in slots])).all()


# ---- small ring: refusals --------------------------------------------------------------------------------------------------------------
def test_encrypt_refuses_out_of_range_slots(small, pie_mod):
    """a slot of t, of -t and of INT64_MIN (which has no negation) is PIEHIP_EINVAL wherever it stands; +-(t - 1) are slots; and the
    handle encrypts and decrypts afterwards"""
    o, cc = small
    t = o.t
    sk = o.keygen(49 + o.L)
    seeds = np.array([601, 602], dtype=np.uint64)
    for bad in (t, -t, INT64_MIN, 1 << 62, -(1 << 62)):
        for where in ((0, 0), (1, 6)):
            slots = np.zeros((2, 7), dtype=np.int64)
            slots[where] = bad
            rc, _ = dev_encrypt_rc(cc, sk, slots, seeds)
            assert rc == pie_mod.EINVAL, "slot value %d at %r: return code %d" % (bad, where, rc)
    slots = np.array([[t - 1, -(t - 1), 0, 1, -1, 2, -2], [0, 0, 0, 0, 0, 0, -(t - 1)]], dtype=np.int64)
    rc, got = dev_encrypt_rc(cc, sk, slots, seeds)
    assert rc == 0
    for c in range(2):
        assert (got[c] == o.encrypt_slots(sk, slots[c], int(seeds[c]))).all()
    assert (dev_decrypt(cc, sk, got, 7) == want_slots(o, sk, got, 7)).all()


# ---- ciphertext counts: how the host shares the sampling out -----------------------------------------------------------------------
@pytest.mark.parametrize("nct", [1, 2, 17, 33])
def test_ciphertext_counts(ob, pie_mod, nct):
    """the host samples a and e of the ciphertexts in up to 16 threads, ciphertexts nct i/nth .. nct (i + 1)/nth each: counts that do
    not divide evenly, every ciphertext under its own seed"""
    o = make_oracle(ob, 2, None, T32)
    cc = _context(pie_mod, o)
    rng = np.random.default_rng(nct)
    sk = o.keygen(51)
    slots = rng.integers(-(o.t - 1), o.t, (nct, 7), dtype=np.int64)
    seeds = np.arange(700, 700 + nct, dtype=np.uint64)
    got = dev_encrypt(cc, sk, slots, seeds)
    aseeds = a_seeds_of(nct, 11)
    a = cc.expand_uniform(aseeds)
    c0 = dev_encrypt_seeded(cc, sk, slots, seeds, aseeds)
    cc.close()
    for c in range(nct):
        assert (got[c] == o.encrypt_slots(sk, slots[c], int(seeds[c]))).all(), "ciphertext %d of %d" % (c, nct)
        e = sampled_rows(o, int(seeds[c]), uniform=False)[0][1]
        assert (c0[c] == seeded_c0(o, sk, slots[c], a[c], e)).all(), "seeded ciphertext %d of %d" % (c, nct)


# ---- one case per transform route ------------------------------------------------------------------------------------------------------
ROUTE_CASES = [(256, 1, None, T32), (1024, 3, None, T32), (2048, 6, None, T32), (4096, 2, None, T16), (8192, 3, 1 << 58, T32),
               (16384, 4, None, T32), (16384, 7, 1 << 50, T32), (32768, 6, None, T32), (32768, 4, 1 << 61, T32), (65536, 2, 1 << 61, T32)]


@pytest.mark.parametrize("n,L,chain,t", [pytest.param(n, L, c, t, id="%d-%d-%s-t%d" % (n, L, "default" if c is None else "below2^%d" % (c.bit_length() - 1),
                                                                                 t.bit_length() - 1)) for n, L, c, t in ROUTE_CASES])
def test_routes(ob, pie_mod, n, L, chain, t):
    """every route of ntt_plan_decide under the client kernels, and their grids of 256-thread blocks partial (N = 64 above), exact and
    many: two ciphertexts decrypted together -- the families of decrypt_families tiled over a polynomial as its phase, and an honest
    product -- two encryptions of the crafted messages, and the relinearisation key"""
    o = make_oracle(ob, L, chain, t, n)
    qs, _ = ccol.moduli(o)
    rng = np.random.default_rng(n + L)
    sk = o.keygen(53)
    evk = o.relin_keygen(sk, 54)
    slots = np.stack([o.decode(ccol.enc_message_coeffs(o, n), n), o.decode(np.roll(ccol.enc_message_coeffs(o, n), 4), n)])
    seeds = np.array([801, 802], dtype=np.uint64)
    enc = np.stack([o.encrypt_slots(sk, slots[c], int(seeds[c])) for c in range(2)])
    cts = np.stack([ccol.phase_ct(o, ccol.tile(ccol.decrypt_families(o), n, rng)), o.mul(enc[0], enc[1], evk)])
    cc = _context(pie_mod, o)
    got_dec = {B: dev_decrypt(cc, sk, cts, B) for B in (7, n)}
    got_enc = dev_encrypt(cc, sk, slots, seeds)
    got_evk = dev_ks_keygen(cc, sk, 54)
    cc.close()
    for B, got in got_dec.items():
        bad = np.argwhere(got != want_slots(o, sk, cts, B))
        assert not len(bad), "B = %d: %d slots differ, first (ciphertext, slot) = %r" % (B, len(bad), tuple(bad[0]))
    assert (got_enc == enc).all()
    assert (got_evk == evk).all()


# ---- reduced contexts ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("keep", [1, 2])
def test_decrypt_in_a_reduced_context(ob, pie_mod, keep):
    """BatchedFHEPSIClient.decrypt(..., limbs=keep): results a server reduced to `keep` limbs are decrypted in the context (N, keep, t,
    q[:keep]) with the first limbs of the key; the phases are planted over those limbs"""
    from nested_hashing_psi_amd.client import BatchedFHEPSIClient
    o = make_oracle(ob, 4, None, T32)
    ro = reduced_oracle(ob, o, keep)
    qs, _ = ccol.moduli(ro)
    assert qs == ccol.moduli(o)[0][:keep]
    rng = np.random.default_rng(keep)
    fam = ccol.decrypt_families(ro)
    polys = ccol.columns_polys([c for v in fam.values() for c in v], qs, N)
    cc = _context(pie_mod, o)
    cl = BatchedFHEPSIClient(cc, 1, N, 1, 1, 1)
    cl.sk = o.keygen(55)
    sk = np.ascontiguousarray(cl.sk[:keep])
    assert (sk == ro.keygen(55)).all()
    for key, cts in planted_batches(ro, polys, sk, rng)[:2]:
        for B in (7, N):
            assert (cl.decrypt(cts, nslots=B, limbs=keep) == want_slots(ro, key, cts, B)).all(), "%d components, B = %d" % (cts.shape[1], B)
    cc.close()
