"""The client's side of the protocol on crafted inputs (tests/coeff_columns.py): that the builders deliver what they claim, and the C
oracle's decryption, encryption and key generation against exact arithmetic (oracle/exact.py) and against their definitions.

Decryption rounds round(t x/Q) mod t with a sum of L truncated 60-bit fractions, as the base conversions do; the zone in which it may
leave exact rounding, by one step, is the 2n + 2 units around a tie that the header of tests/test_coeff_columns.py derives, with n = L.
The columns here are the phases x themselves: a ciphertext (c0, 0) has the phase INTT(c0) under every key.
tests/test_gpu_client_columns.py holds the device to the oracle on the same columns, bit for bit.
"""
import numpy as np
import pytest

from oracle import exact as ex
from tests import coeff_columns as ccol
from tests import param_chains as pc
from tests.param_chains import T16, T32, T40, T48
from tests.hashing_model import Rng
from tests.test_coeff_columns import CHAINS, N, _chain_id

LS = (1, 2, 3, 7)
TS = (T16, T32, T40, T48)
NOISE = 20          # the error sampler is popcount(20 bits) - popcount(20 bits)


def narrowest_q_bits(chain, L):
    """bit length of the narrowest modulus of Q (tests/param_chains.py)"""
    if chain == "q_narrow_p_wide":
        return 36
    if chain == "q0_wide" and L > 1:
        return 45
    return chain.bit_length() - 1 if isinstance(chain, int) else 60


def chain_allows(chain, L, t):
    """a context wants every q_i above t (piehip_create refuses the others): t below the smallest value of the narrowest width"""
    return t < 1 << (narrowest_q_bits(chain, L) - 1)


# barrett_edges holds two special primes in Q: it has no chain of one limb
SHAPES = [(L, chain) for chain in CHAINS for L in LS if not (L == 1 and chain == "barrett_edges")]
CASES = [pytest.param(L, chain, t, id="L%d-%s-t%d" % (L, _chain_id(chain), t.bit_length() - 1))
         for L, chain in SHAPES for t in TS if chain_allows(chain, L, t)]
LEFT_OUT = [(L, chain, t) for L, chain in SHAPES for t in TS if not chain_allows(chain, L, t)]


def make_oracle(ob, L, chain, t, n=N):
    if chain is None:
        return ob.Oracle(n, L, t)
    q, p = pc.uniform_chain(n, L, chain) if isinstance(chain, int) else pc.named_chain(n, L, chain)
    return ob.Oracle(n, L, t, q, p)


def test_cases_leave_out_only_what_a_context_refuses(ob):
    """the (chain, t) pairs that CASES leaves out hold a modulus q_i <= t, the pairs it keeps hold none"""
    assert sorted({(_chain_id(c), t) for _, c, t in LEFT_OUT}) == sorted([("q0_wide", T48), ("q_narrow_p_wide", T40), ("q_narrow_p_wide", T48)])
    for L, chain, t in LEFT_OUT:
        assert min(ccol.moduli(make_oracle(ob, L, chain, t))[0]) <= t
    for L, chain in SHAPES:
        qs = ccol.moduli(make_oracle(ob, L, chain, T16))[0]
        assert min(qs).bit_length() == narrowest_q_bits(chain, L)
        for t in TS:
            assert chain_allows(chain, L, t) == (min(qs) > t)


# ---- the builders ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,chain,t", CASES)
def test_decrypt_ties_sit_where_stated(ob, L, chain, t):
    """t x/Q of tie column k is |k| units of 2^-60 from a half-integer, to within one unit and one integer step (as
    tests/test_coeff_columns.py::test_ties_sit_where_stated asserts for the other tie families)"""
    from fractions import Fraction
    o = make_oracle(ob, L, chain, t)
    qs, _ = ccol.moduli(o)
    Q = ex.prod(qs)
    fam = ccol.ties_decrypt(o)
    ks = ccol.tie_ks(L)
    assert set(fam) == set(ks) | {"floor", "floor+1", "x=0", "x=1", "x=-1"}
    step = Fraction(1 << 60, Q)
    tol = 1 + step
    if L > 1:           # Q >= 2^71: a step is far below a unit, and u = floor(Q 2^-60) >= 2^11 is a unit to within 1/u
        u = ccol.tie_unit(Q)
        assert tol < 2 and u >= 1 << 11 and abs(u * step - 1) < Fraction(1, u)
    for k in ks:
        dist = ccol.tie_distance(t * fam[k], Q)
        assert abs(dist - abs(k) * ccol.tie_unit(Q) * step) < tol, "k = %d: %.3f units" % (k, float(dist))
    for lab in ("floor", "floor+1"):
        assert ccol.tie_distance(t * fam[lab], Q) < tol
    assert (t * fam["floor"] % Q, t * fam["floor+1"] % Q) == ((Q - 1) // 2, (Q + 1) // 2)
    assert (fam["x=0"], fam["x=1"], fam["x=-1"]) == (0, 1, Q - 1)
    assert all(0 <= x < Q for x in fam.values())


@pytest.mark.parametrize("L,chain,t", CASES)
def test_message_edges_are_the_steps_of_the_rounding(ob, L, chain, t):
    """every pair rounds exactly to m - 1 and m; m = t is the wrap to message 0, and the pairs at (t - 1)/2 and (t + 1)/2 are the
    coefficients between which the centred value changes sign"""
    o = make_oracle(ob, L, chain, t)
    Q = ex.prod(ccol.moduli(o)[0])
    edges = ccol.message_edges(o)
    ms = ccol.message_edge_values(t)
    assert ms == [1, (t - 1) // 2, (t + 1) // 2, t - 1, t] and len(edges) == 2 * len(ms)
    for m in ms:
        lo, hi = edges[(m, "below")], edges[(m, "at")]
        assert 0 <= lo < hi < Q and hi == lo + 1
        assert ex.rnd_div(t * lo, Q) == m - 1 and ex.rnd_div(t * hi, Q) == m
    assert ex.rnd_div(t * edges[(t, "at")], Q) % t == 0
    fam = ccol.decrypt_families(o)
    assert list(fam) == ["digits", "windows", "ties_decrypt", "message_edges"] and fam.moduli == tuple(ccol.moduli(o)[0])
    assert fam["message_edges"] == [ccol.reduce_col(x, fam.moduli) for x in edges.values()]
    assert fam["digits"] == ccol.digit_extremes(fam.moduli) and fam["windows"] == ccol.lift_windows(fam.moduli)


@pytest.mark.parametrize("L,chain,t", CASES)
def test_message_coeffs_reach_every_branch(ob, L, chain, t):
    """[Q m_n]_t is the intended rr, every rr of message_rrs appears, and the slot vector o.decode(coeff, N) encodes back to coeff"""
    o = make_oracle(ob, L, chain, t)
    Q = ex.prod(ccol.moduli(o)[0])
    coeff = ccol.enc_message_coeffs(o, N)
    rrs = ccol.message_rrs(t)
    h = (t - 1) // 2
    assert rrs == [0, 1, 2, h - 1, h, h + 1, h + 2, t - 2, t - 1] and N >= len(rrs)
    assert [Q * int(m) % t for m in coeff] == [rrs[n % len(rrs)] for n in range(N)]
    slots = o.decode(coeff, N)
    assert (np.abs(slots) <= h).all()
    assert (o.encode(slots)[0] == coeff).all()


def test_phase_ct_has_the_phase(ob):
    """c0 + c1 s (+ c2 s^2) of phase_ct's ciphertext is NTT(X), for c1 = 0 under any key and for uniform c1, c2 under a sampled one"""
    o = make_oracle(ob, 3, "q0_wide", T32)
    qs, _ = ccol.moduli(o)
    rng = np.random.default_rng(3)
    X = ccol.uniform_poly(qs, N, rng)
    sk = o.keygen(5)
    c1, c2 = ccol.uniform_poly(qs, N, rng), ccol.uniform_poly(qs, N, rng)
    want = ccol.ntt_q(o, X)
    ct = ccol.phase_ct(o, X)
    assert ct.shape == (2, 3, N) and (ct[0] == want).all() and (ct[1] == 0).all()
    ct = ccol.phase_ct(o, X, sk, c1)
    assert ct.shape == (2, 3, N) and (ct[1] == c1).all()
    s2 = ccol.mulmod_rows(sk, sk, qs)
    for i, q in enumerate(qs):
        assert [(int(a) + int(b) * int(s)) % q for a, b, s in zip(ct[0, i], c1[i], sk[i])] == [int(v) for v in want[i]]
    ct = ccol.phase_ct(o, X, sk, c1, c2)
    assert ct.shape == (3, 3, N) and (ct[1] == c1).all() and (ct[2] == c2).all()
    for i, q in enumerate(qs):
        got = [(int(a) + int(b) * int(s) + int(c) * int(ss)) % q for a, b, c, s, ss in zip(ct[0, i], c1[i], c2[i], sk[i], s2[i])]
        assert got == [int(v) for v in want[i]]
    polys = ccol.columns_polys(ccol.cols_of(X)[:N] + ccol.cols_of(X)[:5], qs, N)
    assert polys.shape == (2, 3, N) and (polys[0] == X).all() and (polys[1][:, :5] == X[:, :5]).all() and (polys[1][:, 5:] == 0).all()


# ---- the oracle's decryption against exact rounding ---------------------------------------------------------------------------------
def in_zone(o, x):
    Q = ex.prod(ccol.moduli(o)[0])
    return ccol.tie_distance(o.t * x, Q) <= 2 * o.L + 2


def decrypt_columns(o):
    """every column of decrypt_families(o) planted as a phase (c1 = 0) and decrypted by the oracle.  Asserts the contract and returns
    {family: (columns, columns in the zone, columns on which the oracle differs from exact rounding)}"""
    qs, _ = ccol.moduli(o)
    Q, t = ex.prod(qs), o.t
    fam = ccol.decrypt_families(o)
    sk = np.zeros((o.L, o.N), dtype=np.uint64)        # c1 = 0: the key does not enter
    counts = {}
    for name, cols in fam.items():
        got = []
        for poly in ccol.columns_polys(cols, qs, o.N):
            got += [int(v) for v in o.decrypt(sk, ccol.phase_ct(o, poly))[0]]
        zone = differ = 0
        for col, g in zip(cols, got):
            x = ex.crt(col, qs)
            want = ex.rnd_div(t * x, Q) % t
            if in_zone(o, x):
                zone += 1
                assert g in (want, (want + 1) % t, (want - 1) % t), "%s column %r: %d is not within a step of %d" % (name, col, g, want)
            else:
                assert g == want, "%s column %r differs outside the zone: %d, exact %d" % (name, col, g, want)
            differ += g != want
        counts[name] = (len(cols), zone, differ)
    # conditions on the families, not measurements: only the ties and the message edges may lie in the zone
    assert counts["digits"][1] == 0 and counts["windows"][1] == 0
    plain = ccol.ties_decrypt(o)
    assert not any(in_zone(o, plain[lab]) for lab in ("x=0", "x=1", "x=-1"))
    return counts


def _line(counts):
    return ", ".join("%s %d/%d/%d" % ((name,) + c) for name, c in counts.items())


@pytest.mark.parametrize("L,chain,t", CASES)
def test_decrypt_against_exact(ob, L, chain, t):
    """o.decrypt equals round(t x/Q) mod t outside the zone of 2L + 2 units around a tie, and is within one step (mod t) inside it"""
    counts = decrypt_columns(make_oracle(ob, L, chain, t))
    tot = [sum(c[i] for c in counts.values()) for i in range(3)]
    print("L=%d %s t=2^%d: %d columns, %d in the zone, the oracle differs from exact on %d  (family columns/zone/differ: %s)"
          % (L, _chain_id(chain), t.bit_length() - 1, tot[0], tot[1], tot[2], _line(counts)))


def test_decrypt_families_reach_the_zone(ob):
    """on the 60-bit chain with L = 7 -- up to fourteen units of truncation -- the oracle's decryption leaves exact rounding on some
    column: these are the columns a device kernel has to reproduce bit for bit"""
    counts = decrypt_columns(make_oracle(ob, 7, None, T32))
    assert sum(c[2] for c in counts.values()) > 0, "none of the columns differs: %s" % _line(counts)


# ---- the oracle's encryption against its definition ---------------------------------------------------------------------------------
def sampled_rows(o, seed, rows=1, uniform=True):
    """what one generator seeded with `seed` hands out, row after row: the uniform polynomial a [L][N] (rejection sampling, limb by
    limb; None where the caller supplies a: seeded ciphertexts and key rows) and then the error polynomial e [N].  A restatement of
    the samplers in Python (tests/hashing_model.Rng is the generator): returns [(a, e)] * rows"""
    qs, _ = ccol.moduli(o)
    r = Rng(seed)
    out = []
    for _ in range(rows):
        a = np.array([[r.below(q) for _ in range(o.N)] for q in qs], dtype=np.uint64) if uniform else None
        xs = [r.next() for _ in range(o.N)]
        out.append((a, [bin(x & 0xFFFFF).count("1") - bin((x >> 20) & 0xFFFFF).count("1") for x in xs]))
    return out


def message_term(Q, t, m):
    """round(Q m/t) = (Q m - [Q m]_t)/t with [.]_t centred"""
    rr = Q * m % t
    if 2 * rr > t:
        rr -= t
    assert (Q * m - rr) % t == 0
    return (Q * m - rr) // t


@pytest.mark.parametrize("L,chain,t", CASES)
def test_encrypt_against_definition(ob, L, chain, t):
    """for every coefficient of a crafted message, the phase of o.encrypt's ciphertext is round(Q m/t) + e (mod Q) with |e| <= 20;
    encrypting the slot vector gives the same ciphertext; and it decrypts to the message wherever Q >= 64 t"""
    o = make_oracle(ob, L, chain, t)
    qs, _ = ccol.moduli(o)
    Q = ex.prod(qs)
    coeff = ccol.enc_message_coeffs(o, N)
    sk = o.keygen(11 + L)
    ct = o.encrypt(sk, coeff, 77 + L)
    # phase: c0 + c1 s, with Python integers limb by limb
    ev = np.stack([np.array([(int(a) + int(b) * int(s)) % q for a, b, s in zip(ct[0, i], ct[1, i], sk[i])], dtype=np.uint64) for i, q in enumerate(qs)])
    es = []
    for n, col in enumerate(ccol.cols_of(ccol.intt_q(o, ev))):
        e = ex.centered(ex.crt(col, qs) - message_term(Q, t, int(coeff[n])), Q)
        assert abs(e) <= NOISE, "coefficient %d (rr = %d): e = %d" % (n, Q * int(coeff[n]) % t, e)
        es.append(e)
    assert min(es) < 0 < max(es)                                       # noise of both signs met the terms
    a, e = sampled_rows(o, 77 + L)[0]
    assert (ct[1] == a).all() and es == e                              # ... and it is the seed's: a first, then e
    assert (ct == o.encrypt_slots(sk, o.decode(coeff, N), 77 + L)).all()
    if Q >= 64 * t:
        assert (o.decrypt(sk, ct)[0] == coeff).all()


def seeded_c0(o, sk, slots, a, e):
    """the c0 half of the secret-key encryption of `slots` with second component a and error polynomial e: NTT(e + round(Q m/t)) - a s,
    with Python integers around the oracle's encoding and transforms"""
    qs, _ = ccol.moduli(o)
    Q = ex.prod(qs)
    coeff = o.encode(slots)[0]
    x = [message_term(Q, o.t, int(m)) + ev for m, ev in zip(coeff, e)]
    em = ccol.ntt_q(o, np.array([[v % q for v in x] for q in qs], dtype=np.uint64))
    return ccol.phase_ct(o, ccol.intt_q(o, em), sk, a)[0]


@pytest.mark.parametrize("L,chain,t", [(1, None, T48), (3, "q0_wide", T32), (7, 1 << 61, T16)])
def test_seeded_c0_restates_the_encryption(ob, L, chain, t):
    """seeded_c0, which tests/test_gpu_client_columns.py holds seeded ciphertexts to, gives the oracle's c0 when handed the oracle's own
    a and e"""
    o = make_oracle(ob, L, chain, t)
    sk = o.keygen(3)
    slots = o.decode(ccol.enc_message_coeffs(o, N), N)
    ct = o.encrypt_slots(sk, slots, 9)
    a, e = sampled_rows(o, 9)[0]
    assert (seeded_c0(o, sk, slots, a, e) == ct[0]).all()
    assert (seeded_c0(o, sk, slots, a, [v + (n == 5) for n, v in enumerate(e)]) != ct[0]).any()


def test_encrypt_cannot_decrypt_without_room(ob):
    """Q >= 64 t above is a condition of the scheme, not slack of the test: on a 50-bit chain of one limb with a 48-bit plaintext
    modulus Q/2t is about 2, below the noise, and decryption must fail"""
    o = make_oracle(ob, 1, 1 << 50, T48)
    assert ex.prod(ccol.moduli(o)[0]) < 64 * T48
    coeff = ccol.enc_message_coeffs(o, N)
    sk = o.keygen(12)
    assert (o.decrypt(sk, o.encrypt(sk, coeff, 78))[0] != coeff).any()


# ---- key-switching keys against their definition ------------------------------------------------------------------------------------
def key_noise(o, sk, key, s_from, a=None):
    """the small polynomials e_i of a key [L][2][L][N] (or of first components [L][L][N] with the second components `a`): asserts that
    INTT_j(b_i + a_i s - [i == j] s_from) has all coefficients in [-20, 20] and is the same polynomial in every limb j; returns [L][N]"""
    qs, _ = ccol.moduli(o)
    L = len(qs)
    out = []
    for i in range(L):
        b, ai = (key[i, 0], key[i, 1]) if a is None else (key[i], a[i])
        v = np.stack([np.array([(int(x) + int(y) * int(s) - (int(f) if i == j else 0)) % q for x, y, s, f in zip(b[j], ai[j], sk[j], s_from[j])],
                               dtype=np.uint64) for j, q in enumerate(qs)])
        e = [[ex.centered(int(c), q) for c in row] for row, q in zip(ccol.intt_q(o, v), qs)]
        assert all(abs(c) <= NOISE for row in e for c in row), "row %d: |e| up to %d" % (i, max(abs(c) for row in e for c in row))
        assert all(row == e[0] for row in e), "row %d: the limbs hold different polynomials" % i
        out.append(e[0])
    return out


def key_sources(o, sk):
    """{name: (galois element or 0, s_from in EVALUATION form)}: s^2, s(X^5), s(X^(2N - 1))"""
    qs, _ = ccol.moduli(o)
    s = ccol.intt_q(o, sk)
    src = {"relin": (0, ccol.mulmod_rows(sk, sk, qs))}
    for g in (5, 2 * o.N - 1):
        src["rot%d" % g] = (g, ccol.ntt_q(o, ccol.sigma(s, g, qs)))
    return src


@pytest.mark.parametrize("L,chain,t", CASES)
def test_keys_against_definition(ob, L, chain, t):
    """o.relin_keygen and o.rot_keygen (g = 5 and 2N - 1): row i is (e_i - a_i s + [limb == i] s_from, a_i) with e_i small and the same
    in every limb; s_from = s^2, or s(X^g) by coeff_columns.sigma on the coefficient form of s.  The secret itself is ternary"""
    o = make_oracle(ob, L, chain, t)
    qs, _ = ccol.moduli(o)
    sk = o.keygen(21 + L)
    s = [[ex.centered(int(c), q) for c in row] for row, q in zip(ccol.intt_q(o, sk), qs)]
    assert all(row == s[0] for row in s) and set(s[0]) == {-1, 0, 1}
    for name, (g, s_from) in key_sources(o, sk).items():
        key = o.rot_keygen(sk, g, 31 + L) if g else o.relin_keygen(sk, 31 + L)
        es = key_noise(o, sk, key, s_from)
        assert len({tuple(e) for e in es}) == L, "%s: rows share their noise" % name
        assert all(min(e) < 0 < max(e) for e in es)
        for i, (a, e) in enumerate(sampled_rows(o, 31 + L, rows=L)):   # one generator for the whole key: a_0, e_0, a_1, e_1, ..
            assert (key[i, 1] == a).all() and es[i] == e
