"""Result limbs: the exact definition of the limb drop (include/piehip.h "Result limbs"), pinned, and what it does to a ciphertext.

The oracle has no such function, so the definition lives here as a short function over Python integers, built on the oracle's
transforms.  tests/test_gpu_result_limbs.py compares the library against it bit for bit.

A component is a polynomial with coefficients c in [0, Q), held as residues.  The limbs l = L - 1 .. keep are dropped one after
the other:  r = c mod q_l centred;  c <- (c - r) / q_l (exact), i.e. c_i <- (c_i - r) q_l^-1 mod q_i for i < l.
"""
import numpy as np
import pytest

from tests.param_chains import T16, named_chain


def drop_limbs_coeff(c, q, keep):
    """c: list of L object arrays (Python ints), the residues of COEFFICIENT-format polynomials mod q[0..L-1]; returns the `keep`
    residue arrays after dropping the limbs L - 1 .. keep"""
    c = [np.array(v, dtype=object) for v in c]
    q = [int(v) for v in q]
    for l in range(len(q) - 1, keep - 1, -1):
        v = c[l]
        r = np.where(v > (q[l] - 1) // 2, v - q[l], v)          # q_l is odd: no ties
        for i in range(l):
            c[i] = (c[i] - r) * pow(q[l], -1, q[i]) % q[i]
    return c[:keep]


def mod_reduce_exact(o, ct, keep):
    """the definition on ciphertexts ct[..][2][L][N] in EVALUATION format under the oracle o's chain: [..][2][keep][N]"""
    ct = np.asarray(ct, dtype=np.uint64)
    L, N = o.L, o.N
    assert ct.shape[-2:] == (L, N) and 1 <= keep <= L
    flat = ct.reshape(-1, L, N)
    out = np.zeros((flat.shape[0], keep, N), dtype=np.uint64)
    for k, poly in enumerate(flat):
        c = drop_limbs_coeff([o.intt(l, poly[l]).astype(object) for l in range(L)], o.q, keep)
        for i in range(keep):
            out[k, i] = o.ntt(i, c[i].astype(np.uint64))
    return out.reshape(ct.shape[:-2] + (keep, N))


def reduced_oracle(ob, o, keep):
    """the oracle context (N, keep, t, q[:keep]); po_create wants an auxiliary basis too: the next keep + 1 primes of the chain"""
    chain = [int(v) for v in o.moduli[:o.M]]
    return ob.Oracle(o.N, keep, o.t, np.array(chain[:keep], dtype=np.uint64), np.array(chain[keep:2 * keep + 1], dtype=np.uint64))


def _crt(res, q):
    Q = 1
    for m in q:
        Q *= m
    x = 0
    for r, m in zip(res, q):
        Qi = Q // m
        x += int(r) * Qi * pow(Qi, -1, m)
    return x % Q, Q


def test_residue_form_is_the_integer_definition():
    """the pin: on whole integers c in [0, Q), with exact division, against the residue form used everywhere else -- random
    coefficients and the edges of the centred rounding (dropped residues 0, (q-1)/2, (q+1)/2, q-1; kept residues 0 and q-1)"""
    rng = np.random.default_rng(5)
    for q in ([1152921504606830593, 1152921504606748673, 1152921504606683137, 1152921504606584833],
              [(1 << 61) - 1, 1125899906826241, 288230376151130113],     # 61-, 50- and 58-bit moduli (odd, coprime: all the pin needs)
              [1125899906826241, (1 << 61) - 1]):
        L = len(q)
        cols = [[int(rng.integers(0, m)) for m in q] for _ in range(40)]
        for edge in (0, 1, 2, 3):
            for kept in (0, 1):
                cols.append([(0 if kept == 0 else m - 1) if i == 0 else (0, (m - 1) // 2, (m + 1) // 2, m - 1)[edge]
                             for i, m in enumerate(q)])
        res = [np.array([col[i] for col in cols], dtype=object) for i in range(L)]
        for keep in range(1, L):
            got = drop_limbs_coeff(res, q, keep)
            for n, col in enumerate(cols):
                c, Q = _crt(col, q)
                for l in range(L - 1, keep - 1, -1):
                    v = c % q[l]
                    r = v if v <= (q[l] - 1) // 2 else v - q[l]
                    assert (c - r) % q[l] == 0
                    c = (c - r) // q[l]
                    Q //= q[l]
                    c %= Q                                     # a number modulo q_0 .. q_{l-1} from here on
                assert [int(got[i][n]) for i in range(keep)] == [c % q[i] for i in range(keep)]


def test_keep_all_limbs_is_the_identity(ob):
    o = ob.Oracle(64, 3, T16)
    rng = np.random.default_rng(1)
    ct = np.stack([rng.integers(0, int(m), 64, dtype=np.uint64) for m in o.q] * 2).reshape(2, 3, 64)
    assert (mod_reduce_exact(o, ct, 3) == ct).all()


def _product(o, sk, evk):
    xs, ys = [1, 2, 3, -4, 0, 77], [5, -6, 7, 8, 9, 0]
    prod = o.mul(o.encrypt_slots(sk, xs, 5), o.encrypt_slots(sk, ys, 6), evk)
    return prod, [x * y for x, y in zip(xs, ys)]


@pytest.mark.parametrize("L,chain", [(4, None), (3, "q0_wide")])
def test_reduced_product_decrypts_on_the_shorter_chain(ob, L, chain):
    """after a ct x ct product with relinearisation every keep < L decrypts, in the context (N, keep, t, q[:keep]) with sk[:keep],
    to the slots of the full ciphertext, with noise budget left"""
    N, t = 4096, T16
    q, p = (None, None) if chain is None else named_chain(N, L, chain)
    o = ob.Oracle(N, L, t, q, p)
    sk = o.keygen(3)
    evk = o.relin_keygen(sk, 4)
    prod, want = _product(o, sk, evk)
    full, budget = o.decrypt_slots(sk, prod, len(want))
    assert list(full) == want and budget >= 1
    for keep in range(1, L):
        red = mod_reduce_exact(o, prod, keep)
        assert red.shape == (2, keep, N)
        assert all((red[:, i] < o.q[i]).all() for i in range(keep))
        ok = reduced_oracle(ob, o, keep)
        assert (ok.q == o.q[:keep]).all()
        got, bud = ok.decrypt_slots(np.ascontiguousarray(sk[:keep]), red, len(want))
        print("N=%d L=%d chain=%s keep=%d: budget %d bits (full ciphertext: %d)" % (N, L, chain, keep, bud, budget))
        assert list(got) == want
        assert bud >= 1
