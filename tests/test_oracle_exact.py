"""C oracle (tier ii, RNS-native) against exact big-integer mathematics (tier i, oracle/exact.py).

The reference holds no numeric vectors for this path (tests/TestBatchedFHEPIE.cpp:139-149 prints
"Matches"), so the oracle is pinned against the mathematical definition of each routine instead.
"""
import numpy as np
import pytest

from oracle import exact as ex
from tests import param_chains as pc

T16 = 65537
T32 = 4296540161  # 2^32 + 2^20 + 2^19 + 1, reference BatchedFHEPSIClient.cpp:29


def cols(arr):
    return [tuple(int(v) for v in arr[:, n]) for n in range(arr.shape[1])]


@pytest.mark.parametrize("N", [1024, 4096, 16384, 32768])
def test_prime_chain_and_roots(ob, N):
    L = 2
    q, p = ob.default_moduli(N, L)
    chain = ex.prime_chain(N, 2 * L + 1)
    assert [int(x) for x in q] + [int(x) for x in p] == chain
    for c in chain:
        assert c < (1 << 60) and c % (2 * N) == 1 and ex.is_prime(c)
    if N <= 4096:  # the O(N) minimal-root scan in pure Python
        o = ob.Oracle(N, L, T16)
        for mi in range(2 * L + 1):
            assert o.psi(mi) == ex.min_primitive_root(chain[mi], N)
        assert o.psi(2 * L + 1) == ex.min_primitive_root(T16, N)


@pytest.mark.parametrize("t", [65537, 4296540161, 1099579260929, 281474981953537])
def test_reference_plaintext_moduli_are_ntt_friendly(ob, t):
    # BatchedFHEPSIClient.cpp:23-38 -- all four must be prime and 1 mod 2N for N = 16384
    assert ex.is_prime(t) and ob.lib().po_is_prime(t) and t % (2 * 16384) == 1


@pytest.mark.parametrize("N,L", [(64, 2), (4096, 2), (16384, 4)])
def test_ntt_matches_evaluation_definition(ob, N, L):
    o = ob.Oracle(N, L, T16 if N <= 4096 else T32)
    rng = np.random.default_rng(N)
    logN = N.bit_length() - 1
    for mi in (0, L, 2 * L, 2 * L + 1):
        q = int(o.moduli[mi])
        a = rng.integers(0, q, N, dtype=np.uint64)
        f = o.ntt(mi, a)
        assert (o.intt(mi, f) == a).all()
        for p in ([0, 1, 2, N // 2, N - 1] if N > 64 else range(N)):
            assert int(f[p]) == ex.ntt_eval_point(a, o.psi(mi), q, p, logN)
    # edge inputs: zeros, all q-1, a delta
    q = int(o.moduli[0])
    z = np.zeros(N, dtype=np.uint64)
    assert (o.ntt(0, z) == 0).all()
    m1 = np.full(N, q - 1, dtype=np.uint64)
    assert (o.intt(0, o.ntt(0, m1)) == m1).all()
    d = z.copy()
    d[0] = 1
    assert (o.ntt(0, d) == 1).all()


def test_twiddle_tables(ob):
    N, L = 256, 2
    o = ob.Oracle(N, L, T16)
    fwd, inv = o.twiddles(0)
    q, psi = int(o.q[0]), o.psi(0)
    for k in range(1, N):
        w = pow(psi, ex.bitrev(k, 8), q)
        assert int(fwd[k]) == w and int(inv[k]) == pow(w, -1, q)


def _chain(N, L, chain):
    """None: the default chain; an int: the uniform chain below it; a str: a named chain of tests/param_chains.py"""
    if chain is None:
        return None, None
    if isinstance(chain, int):
        return pc.uniform_chain(N, L, chain)
    return pc.named_chain(N, L, chain)


def _cases(rows):
    """parameter rows (N, L, t, chain); the ids of the default-chain rows stay N-L-t"""
    def cid(N, L, t, chain):
        tail = "" if chain is None else "-" + (chain if isinstance(chain, str) else "below2^%d" % (chain.bit_length() - 1))
        return "%d-%d-%d%s" % (N, L, t, tail)
    return [pytest.param(*r, id=cid(*r)) for r in rows]


@pytest.mark.parametrize("N,L,t,chain", _cases([(64, 1, T16, None), (64, 2, T16, None), (256, 3, T32, None), (128, 4, T32, None),
                                                (64, 6, T32, None),
                                                (64, 7, T32, None), (128, 7, T16, None), (64, 7, T32, 1 << 61), (64, 7, T32, 1 << 50)]
                                               + [(64, L, T32, name) for name in pc.NAMED for L in (2, 4, 7)]
                                               + [(128, 3, T16, name) for name in pc.NAMED]))
def test_base_conversions_exact(ob, N, L, t, chain):
    """the oracle's three base conversions against big-integer arithmetic; up to L = 7 (MAX_L) and on the mixed-width chains"""
    q, p = _chain(N, L, chain)
    o = ob.Oracle(N, L, t, q, p)
    if q is not None:
        assert (o.q == q).all() and (o.p == p).all()
    qs = [int(x) for x in o.q]
    ps = [int(x) for x in o.p]
    rng = np.random.default_rng(1000 * N + L)
    xq = np.stack([rng.integers(0, q, N, dtype=np.uint64) for q in qs])
    # force edge columns: 0, Q-1 (= -1), 1, and values a safe 2^-40 away from the +-Q/2 wrap.
    # (Inputs within ~2^-57 (relative) of a rounding tie are the documented domain where the
    # 60-bit fixed-point rounding term may differ from exact rounding -- as OpenFHE's float
    # formulation does; tests/test_coeff_columns.py generates them and bounds the difference.)
    Q = ex.prod(qs)
    for n, val in enumerate([0, Q - 1, Q // 2 - (Q >> 40), Q // 2 + (Q >> 40), 1]):
        for i, q in enumerate(qs):
            xq[i, n] = val % q
    got = o.expand_q_to_qp(xq)
    want = ex.expand_q_to_qp(cols(xq), qs, ps)
    assert cols(got) == want
    got = o.scale_pq_expand(xq)
    want = ex.scale_pq_expand(cols(xq), qs, ps)
    assert cols(got) == want
    mods = qs + ps
    xqp = np.stack([rng.integers(0, m, N, dtype=np.uint64) for m in mods])
    QP = Q * ex.prod(ps)
    for n, val in enumerate([0, QP - 1, QP // 2 - (QP >> 40), QP // 2 + (QP >> 40), 1]):
        for i, m in enumerate(mods):
            xqp[i, n] = val % m
    got = o.scale_round_tp(xqp)
    want = ex.scale_round_tp(cols(xqp), qs, ps, t)
    assert cols(got) == want


def _coeff_ints(o, ct_eval, qs):
    """EVALUATION ct [c][L][N] -> per component list of CRT-reconstructed coefficients in [0,Q)"""
    out = []
    for comp in ct_eval:
        limbs = np.stack([o.intt(i, comp[i]) for i in range(len(qs))])
        out.append([ex.crt(col, qs) for col in cols(limbs)])
    return out


@pytest.mark.parametrize("N,L,t", [(64, 2, T16), (1024, 2, T16), (512, 3, T32), (4096, 2, T16)])
def test_tensor_product_exact(ob, N, L, t):
    """po_mul_tensor == round(t/P * (a (x) round(P/Q b)))  computed with big integers mod QP"""
    o = ob.Oracle(N, L, t)
    qs = [int(x) for x in o.q]
    ps = [int(x) for x in o.p]
    Q, P = ex.prod(qs), ex.prod(ps)
    QP = Q * P
    rng = np.random.default_rng(7 * N + L)
    sk = o.keygen(5)
    lim = 150 if t == T16 else 1000  # keep |x*y| < t/2
    x = rng.integers(-lim, lim, N // 2)
    y = rng.integers(-lim, lim, N // 2)
    cx, cy = o.encrypt_slots(sk, x, 1), o.encrypt_slots(sk, y, 2)
    got = o.mul_tensor(cx, cy)
    a = [[ex.centered(v, Q) % QP for v in comp] for comp in _coeff_ints(o, cx, qs)]
    b = [[ex.centered(ex.rnd_div(P * ex.centered(v, Q), Q), P) % QP for v in comp] for comp in _coeff_ints(o, cy, qs)]
    d0 = ex.negacyclic_mul_mod(a[0], b[0], QP)
    d1 = [(u + v) % QP for u, v in zip(ex.negacyclic_mul_mod(a[0], b[1], QP), ex.negacyclic_mul_mod(a[1], b[0], QP))]
    d2 = ex.negacyclic_mul_mod(a[1], b[1], QP)
    want = [[ex.rnd_div(t * ex.centered(v, QP), P) % Q for v in d] for d in (d0, d1, d2)]
    assert _coeff_ints(o, got, qs) == want
    # and it decrypts (3-component) to the slot-wise product
    dec, budget = o.decrypt_slots(sk, got, N // 2)
    assert (dec == x * y).all() and budget > 0


@pytest.mark.parametrize("N,L,t,chain", _cases([(64, 2, T16, None), (1024, 3, T32, None), (64, 7, T16, None), (256, 7, T32, None),
                                                (64, 3, T16, "q0_wide"), (256, 7, T16, "q0_wide"), (64, 3, T16, "q_narrow_p_wide")]))
def test_decrypt_and_relin_against_exact(ob, N, L, t, chain):
    """decryption and relinearisation against exact arithmetic; q0_wide lifts the digit of its 60-bit q_0 into 45-bit
    moduli (q_i >= 2 q_j: the Barrett branch of the digit lift)"""
    q, p = _chain(N, L, chain)
    o = ob.Oracle(N, L, t, q, p)
    qs = [int(x) for x in o.q]
    rng = np.random.default_rng(3)
    sk = o.keygen(5)
    evk = o.relin_keygen(sk, 6)
    s_coeff = o.intt(0, sk[0])
    q0 = qs[0]
    s = [int(v) if int(v) <= 1 else int(v) - q0 for v in s_coeff]
    assert set(s) <= {-1, 0, 1}
    x = rng.integers(-150, 150, N)
    y = rng.integers(-150, 150, N)
    cx, cy = o.encrypt_slots(sk, x, 1), o.encrypt_slots(sk, y, 2)
    for ct in (cx, o.mul_tensor(cx, cy), o.mul(cx, cy, evk)):
        m_exact, worst = ex.decrypt_exact(_coeff_ints(o, ct, qs), s, qs, t)
        m_oracle, budget = o.decrypt(sk, ct)
        assert [int(v) for v in m_oracle] == m_exact
        assert worst < 0.5
        # the fixed-point budget estimate agrees with the exact noise to within a bit -- or, for a ciphertext quieter than
        # the L ulps (of 2^-60) the per-limb fractions may lose, reads the best budget an L-limb sum can show
        import math
        exact_budget = min(58, int(math.floor(-math.log2(2 * worst)))) if worst > 0 else 58
        floor_L = 59 - L.bit_length()
        assert abs(budget - exact_budget) <= 1 or (budget == floor_L and exact_budget > floor_L)
    dec, _ = o.decrypt_slots(sk, o.mul(cx, cy, evk), N)
    assert (dec == x * y).all()


@pytest.mark.parametrize("chain", [None, 1 << 61], ids=["60-bit", "61-bit"])
@pytest.mark.parametrize("pattern", ["all_q_minus_1", "near_max"])
def test_pie_run_long_sum_against_exact(ob, chain, pattern):
    """run() with K = 1 is stage A plus the mask multiply, every step element-wise mod q in evaluation form: the oracle's
    E = 581 inner products (one mulmod + addmod per term) against Python integers, with every index and database word q - 1
    or in [q - 2^24, q) -- the reference side of tests/test_gpu_long_sums.py at its longest sum"""
    N, L, K, E, b = 16, 2, 1, 581, 2
    q, p = _chain(N, L, chain)
    o = ob.Oracle(N, L, T16, q, p)
    qs = [int(x) for x in o.q]
    rng = np.random.default_rng(581 + len(pattern))

    def words(shape):
        a = np.zeros(tuple(shape) + (L, N), dtype=np.uint64)
        for i, qi in enumerate(qs):
            off = 0 if pattern == "all_q_minus_1" else rng.integers(0, 1 << 24, tuple(shape) + (N,), dtype=np.uint64)
            a[..., i, :] = np.uint64(qi - 1) - off
        return a

    def rand(shape):
        a = np.zeros(tuple(shape) + (L, N), dtype=np.uint64)
        for i, qi in enumerate(qs):
            a[..., i, :] = rng.integers(0, qi, tuple(shape) + (N,), dtype=np.uint64)
        return a

    idx, db = words((K, E, 2)), words((K, b, E))
    minus, masks, evk = rand((2,)), rand((b,)), rand((L, 2))
    got = o.pie_run(idx, minus, db, masks, evk)
    io, do, mo, ko = idx.astype(object), db.astype(object), minus.astype(object), masks.astype(object)
    for bn in range(b):
        for c in range(2):
            for i, qi in enumerate(qs):
                acc = sum(io[0, j, c, i] * do[0, bn, j, i] for j in range(E))     # exact, ~2^131 before the one reduction
                want = [int(v) for v in (acc + mo[c, i]) * ko[bn, i] % qi]
                assert [int(v) for v in got[bn, c, i]] == want, "bin %d, component %d, limb %d" % (bn, c, i)


# ---- the rotation path: Galois elements, the automorphism and its key switch ---------------------------------------------
@pytest.mark.parametrize("N", [8, 16, 64, 4096, 65536])
def test_rot_index_is_a_power_of_five(ob, N):
    """po_rot_index(r) = 5^r mod 2N for r > 0 and 5^-|r| for r < 0 (EvalAtIndex: r > 0 rotates the rows left); every multiple
    of the row length N/2 (5 has order N/2 mod 2N) is the identity"""
    o = ob.Oracle(N, 1, T32)
    m2, h = 2 * N, N // 2
    inv5 = pow(5, -1, m2)
    for r in sorted({1, 2, h - 1}):
        assert o.rot_index(r) == pow(5, r, m2)
        assert o.rot_index(-r) == pow(inv5, r, m2)
        assert o.rot_index(r) * o.rot_index(-r) % m2 == 1
    for r in (h, -h, 2 * h, -3 * h):
        assert o.rot_index(r) == 1
    assert len({pow(5, r, m2) for r in range(h)}) == h


def sigma(a, g, M):
    """sigma_g: a(X) -> a(X^g) mod (X^N + 1, M), coefficient lists"""
    N = len(a)
    out = [0] * N
    for i, v in enumerate(a):
        k = i * g % (2 * N)
        if k < N:
            out[k] = (out[k] + v) % M
        else:
            out[k - N] = (out[k - N] - v) % M
    return out


@pytest.mark.parametrize("chain", [None, "q0_wide", "q_narrow_p_wide"], ids=["60-bit", "q0_wide", "q_narrow_p_wide"])
@pytest.mark.parametrize("N,L", [(64, 2), (64, 7), (256, 7), (1024, 3)])
def test_automorph_against_exact(ob, N, L, chain):
    """po_automorph(c, g, po_rot_keygen(s, g)) decrypts exactly to sigma_g of the message polynomial, and its phase c0 + c1 s is
    sigma_g of c's phase plus the BV key-switch noise sum_i d_i e_i: |d_i| <= q_i / 2 (centred digits), |e_i| <= 20 (the centred
    binomial of 2 x 20 bits), so every coefficient is at most N sum_i 10 q_i.  A key of the wrong secret or Galois element leaves
    noise of size Q.  g: 5, 5^-1 (rotations by +-1), 25 (by 2) and 2N - 1 (the row swap)"""
    t = T16
    q, p = _chain(N, L, chain)
    o = ob.Oracle(N, L, t, q, p)
    qs = [int(x) for x in o.q]
    Q = ex.prod(qs)
    sk = o.keygen(5)
    s = [int(v) if int(v) <= 1 else int(v) - qs[0] for v in o.intt(0, sk[0])]
    assert set(s) <= {-1, 0, 1}
    sQ = [v % Q for v in s]
    rng = np.random.default_rng(N + L)
    x = rng.integers(-(t // 2), t // 2 + 1, N)
    m = [int(v) for v in o.encode(x)[0]]
    c = o.encrypt(sk, m, 9)
    c0, c1 = _coeff_ints(o, c, qs)
    phase = [(u + v) % Q for u, v in zip(c0, ex.negacyclic_mul_mod(c1, sQ, Q))]
    bound = N * sum(10 * qi for qi in qs)
    for n, g in enumerate([5, pow(5, -1, 2 * N), 25, 2 * N - 1]):
        rk = o.rot_keygen(sk, g, 40 + n)
        out = o.automorph(c, g, rk)
        d0, d1 = _coeff_ints(o, out, qs)
        got, worst = ex.decrypt_exact([d0, d1], s, qs, t)
        assert got == sigma(m, g, t), "g = %d" % g
        assert worst < 0.5
        ph = [(u + v) % Q for u, v in zip(d0, ex.negacyclic_mul_mod(d1, sQ, Q))]
        noise = max(abs(ex.centered(u - v, Q)) for u, v in zip(ph, sigma(phase, g, Q)))
        assert noise <= bound, "g = %d: key-switch noise 2^%.1f above the bound 2^%.1f" % (g, np.log2(noise), np.log2(bound))
