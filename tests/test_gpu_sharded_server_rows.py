"""The C++ servers with the settings that change the shape of a result row (tests/rows_server_main.cpp): the sharded server
(host/ShardedBatchedFHEPSIServer.hpp: resultLimbs, chainLimbs, resultRelin) as 2 and 3 processes on one GPU over the stand-in transport
of tests/fake_rccl, which each process loads from the path it is given, and host/BatchedFHEPSIServer.hpp with setResultRelin(false).

This process is the client, with a session of its own that reads the component count and the limb count of every result message from
its header (host/WireFraming.hpp: reserved = 0 or 2 -> two components, 3 -> three).  The shape is KAT-0's (k = 2, e = 1, K = 2, b = 20,
100 server items) at N = 4096, L = 3, t = 65537 with E = 6, where include/piehip.h's table gives 14 bits of budget for keep = 1 and for
chain limbs 2.  Every test asserts a positive noise budget on the rows it received BEFORE the intersection, so that a wrong plaintext
cannot pass as a parameter problem, and compares every row bit for bit with the definitions (exact_rows of
tests/test_gpu_gather_rows.py) for the test seeds 1, 2, 3.
"""
import os
import socket
import struct
import subprocess

import numpy as np
import pytest

from tests import slice_ranks_util as sr
from tests.slice_ranks_util import T16
from tests.test_gpu_gather_rows import exact_rows

pytestmark = pytest.mark.gpu
N, L, T, k, e, K, E, b, NS = 4096, 3, T16, 2, 1, 2, 6, 20, 100
MAGIC = 0x48454950


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    fake, exes = sr.build_programs(tmp_path_factory.mktemp("rows_server"), ["rows_server_main"])
    return fake, exes["rows_server_main"]


@pytest.fixture(scope="module")
def table(ob):
    """the server set, and the database and masks every server here builds from it (the default hash seed, the test secrets 1, 2, 3)"""
    rng = np.random.default_rng(41)
    items = np.unique(rng.integers(1, T, NS + 64, dtype=np.uint64))
    rng.shuffle(items)
    server, others = items[:NS].copy(), items[NS:]
    o = ob.Oracle(N, L, T)
    tbl = ob.hct_build(ob.Tabulation(987654321, k + K), server, k, e, K, b, E, evict_seed=1)
    ob.hct_shuffle_bins(tbl, 2)
    slots = ob.pack_db(tbl)
    mask_slots = ob.masks(T, b, k * e, 3)
    db = np.stack([o.encode_eval(slots[h, bn, j]) for h in range(K) for bn in range(b) for j in range(E)]).reshape(K, b, E, L, N)
    masks = np.stack([o.encode_eval(mask_slots[bn]) for bn in range(b)])
    return o, server, others, db, masks


class Client:
    """one client's side of a session, message by message"""

    def __init__(self, sock, pie, cc, key_seed=11):
        from nested_hashing_psi_amd.client import BatchedFHEPSIClient
        self.s, self.cc = sock, cc
        self.cl = BatchedFHEPSIClient(cc, k, e, K, E, b)
        self.evk = self.cl.runSetUpPhase(keySeed=key_seed, evalKeySeed=key_seed + 1)

    def send(self, payload):
        self.s.sendall(struct.pack("i", len(payload)) + payload)

    def recv(self):
        def exactly(n):
            buf = bytearray()
            while len(buf) < n:
                chunk = self.s.recv(min(1 << 20, n - len(buf)))
                if not chunk:
                    raise ConnectionError("server closed the channel")
                buf += chunk
            return bytes(buf)
        return exactly(struct.unpack("i", exactly(4))[0])

    def setup(self, with_key=True):
        moduli = np.zeros(15, dtype=np.uint64)
        moduli[:2 * L + 1] = self.cc.moduli[:2 * L + 1]
        self.send(struct.pack("IIQ", N, L, T) + moduli.tobytes())
        self.send(b"")
        self.send(np.ascontiguousarray(self.evk, dtype=np.uint64).tobytes() if with_key else b"")

    def barrier(self):
        assert self.recv() == b""

    def query(self, clientset):
        self.minus_ct, self.idx_ct = self.cl.runOfflinePhase(clientset)
        ct_msg = lambda ct: struct.pack("IIIIQ", MAGIC, 1, L, N, 0) + np.ascontiguousarray(ct, dtype=np.uint64).tobytes()
        self.send(ct_msg(self.minus_ct))
        for h in range(K):
            for j in range(E):
                self.send(ct_msg(self.idx_ct[h, j]))

    def results(self):
        """-> rows [b][ncomp][limbs][N], the shape read from the headers"""
        res, shape = [], None
        for _ in range(b):
            m = self.recv()
            magic, count, limbs, n, reserved = struct.unpack("IIIIQ", m[:24])
            assert magic == MAGIC and count == 1 and n == N and reserved in (0, 2, 3) and 1 <= limbs <= L
            ncomp = 3 if reserved == 3 else 2
            assert len(m) == 24 + ncomp * limbs * N * 8
            assert shape in (None, (ncomp, limbs))
            shape = (ncomp, limbs)
            res.append(np.frombuffer(m[24:], dtype=np.uint64).reshape(ncomp, limbs, N))
        return np.stack(res)


def _start(built, G, setfile, settings, slices=False):
    """G ranks of the sharded server, rank r with settings[r] -> (the client's socket, the processes)"""
    fake, exe = built
    a, bsock = socket.socketpair()
    sides = [socket.socketpair() for _ in range(G - 1)]
    env = dict(os.environ, PIEHIP_TEST_SEEDS="1,2,3", PIEHIP_TEST_TIMEOUT_MS="20000")
    tail = [str(setfile)] + [str(v) for v in (k, e, K, E, b)]
    extra = ["slices"] if slices else []
    side0 = ",".join(str(s[0].fileno()) for s in sides) or "-"
    procs = [subprocess.Popen([exe, fake, "0", str(G), "0", str(bsock.fileno()), side0] + tail + [settings[0]] + extra,
                              pass_fds=[bsock.fileno()] + [s[0].fileno() for s in sides], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE)]
    for r in range(1, G):
        procs.append(subprocess.Popen([exe, fake, str(r), str(G), "0", "-1", str(sides[r - 1][1].fileno())] + tail + [settings[r]] + extra,
                                      pass_fds=[sides[r - 1][1].fileno()], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE))
    bsock.close()
    for s in sides:
        s[0].close()
        s[1].close()
    return a, procs


def _clientset(server, others, ninter=1):
    return np.concatenate([server[:ninter], others[:k * e - ninter]]).astype(np.uint64)


def _check_rows(ob, table, c, rows, setting, with_key, ninter=1):
    o, server, others, db, masks = table
    ncomp, rl = rows.shape[1:3]
    # the budget first: rows that do not decrypt are a parameter problem, rows that decrypt to something else are a bug
    assert c.cl.noiseBudget(rows, limbs=rl if rl < L else None) > 0
    found = c.cl.extractIntersection(rows, limbs=rl if rl < L else None)
    assert sorted(int(v) for v in found) == sorted(int(v) for v in server[:ninter])
    idx = np.ascontiguousarray(c.idx_ct, dtype=np.uint64).reshape(K, E, 2, L, N)
    minus = np.ascontiguousarray(c.minus_ct, dtype=np.uint64).reshape(2, L, N)
    evk = np.ascontiguousarray(c.evk, dtype=np.uint64).reshape(L, 2, L, N) if with_key else None
    want = exact_rows(ob, o, idx, minus, db, masks, evk, setting)
    assert want.shape == rows.shape, (want.shape, rows.shape)
    assert (rows == want).all(), "bin layers %s differ from the definition" % [i for i in range(b) if not (rows[i] == want[i]).all()]


# (G, setting, the client sends a key, (components, limbs) of a result message)
@pytest.mark.parametrize("G,setting,with_key,shape", [
    (2, "1:1:0", True, (2, 1)),        # resultLimbs = 1
    (3, "0:1:2", True, (2, 2)),        # chainLimbs = 2; 6 + 7 + 7 layers
    (3, "0:0:0", False, (3, 3)),       # resultRelin = false and an EMPTY key message, forwarded to the workers like any other
    (2, "1:0:2", True, (3, 1)),        # all three together, and a key that does arrive is loaded as ever
])
def test_sharded_server_sends_shaped_rows(ob, pie_mod, built, table, tmp_path, G, setting, with_key, shape):
    o, server, others, db, masks = table
    setfile = tmp_path / "server_set.bin"
    server.astype(np.uint64).tofile(setfile)
    a, procs = _start(built, G, setfile, [setting] * G)
    cc = pie_mod.PieContext(N, L, T)
    try:
        c = Client(a, pie_mod, cc)
        try:
            c.setup(with_key)
            c.barrier()
            c.barrier()
            c.query(_clientset(server, others))
            rows = c.results()
        except Exception:
            for p in procs:
                p.kill()
            raise AssertionError("session failed: %s" % [x[2] for x in sr.wait_all(procs)])
        for r, (rc, so, se) in enumerate(sr.wait_all(procs)):
            assert rc == 0, "server rank %d: %s" % (r, se)
        assert rows.shape == (b,) + shape + (N,)
        _check_rows(ob, table, c, rows, setting, with_key)
    finally:
        a.close()
        cc.close()


@pytest.mark.parametrize("what", ["different", "slices", "empty key"])
def test_sharded_server_refuses_on_every_rank(pie_mod, built, table, tmp_path, what):
    """ranks started with different resultLimbs; a setting together with querySlices; an empty key message with relinearisation on:
    std::invalid_argument on every rank, the client's channel closed, nobody left waiting"""
    o, server, others, db, masks = table
    setfile = tmp_path / "server_set.bin"
    server.astype(np.uint64).tofile(setfile)
    G = 3
    settings = ["1:1:0", "1:1:0", "2:1:0"] if what == "different" else ["1:1:0"] * G
    a, procs = _start(built, G, setfile, settings, slices=what == "slices")
    cc = pie_mod.PieContext(N, L, T)
    try:
        c = Client(a, pie_mod, cc)
        with pytest.raises((ConnectionError, BrokenPipeError, ConnectionResetError)):
            c.setup(with_key=what != "empty key")
            c.barrier()
            c.barrier()
            raise AssertionError("the session went on: %s" % what)
        outs = sr.wait_all(procs, timeout=60)
        for r, (rc, so, se) in enumerate(outs):
            assert rc == 1 and se.startswith("invalid_argument: "), "rank %d: %d %s" % (r, rc, se)
        text = {"different": "resultLimbs", "slices": "querySlices", "empty key": "empty EvalMult key"}[what]
        assert all(text in x[2] for x in outs), outs
    finally:
        a.close()
        cc.close()


@pytest.mark.parametrize("nclients,keys", [(1, (False,)), (3, (True, False, True))])
def test_batched_server_without_the_last_relinearisation(ob, pie_mod, built, table, tmp_path, nclients, keys):
    """host/BatchedFHEPSIServer.hpp, setResultRelin(false), K = 2: one client that sends no key, and three clients in one batch of whom
    only two send one -- every client gets three-component rows, bit for bit the definition's under no key at all"""
    o, server, others, db, masks = table
    fake, exe = built
    setfile = tmp_path / "server_set.bin"
    server.astype(np.uint64).tofile(setfile)
    pairs = [socket.socketpair() for _ in range(nclients)]
    env = dict(os.environ, PIEHIP_TEST_SEEDS="1,2,3")
    fds = [p[1].fileno() for p in pairs]
    proc = subprocess.Popen([exe, "-", "0", "0", "0", ",".join(str(v) for v in fds), "-", str(setfile)] + [str(v) for v in (k, e, K, E, b)] + ["0:0:0"],
                            pass_fds=fds, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    for p in pairs:
        p[1].close()
    cc = pie_mod.PieContext(N, L, T)
    try:
        clients = [Client(pairs[i][0], pie_mod, cc, key_seed=11 + 10 * i) for i in range(nclients)]
        try:
            for c, with_key in zip(clients, keys):
                c.setup(with_key)
            for _ in range(2):
                for c in clients:
                    c.barrier()
            sets = [np.concatenate([server[i:i + 1], others[i:i + 1]]).astype(np.uint64) for i in range(nclients)]
            rows = []
            for c, s in zip(clients, sets):
                c.query(s)
            for c in clients:
                rows.append(c.results())
        except Exception:
            proc.kill()
            raise AssertionError("session failed: %s" % proc.communicate()[1].decode())
        so, se = proc.communicate(timeout=60)
        assert proc.returncode == 0, se.decode()
        for i, c in enumerate(clients):
            assert rows[i].shape == (b, 3, L, N)
            assert c.cl.noiseBudget(rows[i]) > 0
            assert [int(v) for v in c.cl.extractIntersection(rows[i])] == [int(server[i])]
            idx = np.ascontiguousarray(c.idx_ct, dtype=np.uint64).reshape(K, E, 2, L, N)
            minus = np.ascontiguousarray(c.minus_ct, dtype=np.uint64).reshape(2, L, N)
            assert (rows[i] == exact_rows(ob, o, idx, minus, db, masks, None, "0:0:0")).all(), "client %d" % i
    finally:
        for p in pairs:
            p[0].close()
        cc.close()


def test_batched_server_refuses_an_empty_key_when_it_relinearises(pie_mod, built, table, tmp_path):
    o, server, others, db, masks = table
    fake, exe = built
    setfile = tmp_path / "server_set.bin"
    server.astype(np.uint64).tofile(setfile)
    a, bsock = socket.socketpair()
    proc = subprocess.Popen([exe, "-", "0", "0", "0", str(bsock.fileno()), "-", str(setfile)] + [str(v) for v in (k, e, K, E, b)] + ["0:1:0"],
                            pass_fds=[bsock.fileno()], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    bsock.close()
    cc = pie_mod.PieContext(N, L, T)
    try:
        c = Client(a, pie_mod, cc)
        with pytest.raises((ConnectionError, BrokenPipeError, ConnectionResetError)):
            c.setup(with_key=False)
            c.barrier()
        so, se = proc.communicate(timeout=60)
        assert proc.returncode == 1 and se.decode().startswith("invalid_argument: empty EvalMult key"), se
    finally:
        a.close()
        cc.close()
