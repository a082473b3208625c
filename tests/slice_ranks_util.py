"""What the tests of query slices across processes share (tests/test_gpu_slice_ranks.py, tests/test_gpu_sliced_server.py): building the
test-only transport (tests/fake_rccl) and the native programs into a temporary directory, starting the ranks, the client's side of a
server session, and the comparison of result ciphertexts with the oracle.  The programs are handed the transport's path as their
first argument and load it themselves: no process started here has its loader environment touched."""
import os
import socket
import struct
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "nested_hashing_psi_amd")
T16, T32 = 65537, 4296540161


def build_programs(d, names):
    """-> (path of the transport library, {name: executable})"""
    fake = str(d / "librccl.so.1")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-shared", "-fPIC", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-o", fake,
                           os.path.join(ROOT, "tests", "fake_rccl", "fake_rccl.cpp"), "-Wl,-soname,librccl.so.1", "-L/opt/rocm/lib",
                           "-Wl,-rpath,/opt/rocm/lib", "-lamdhip64", "-lpthread"])
    exes = {}
    for name in names:
        exes[name] = str(d / name)
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-o", exes[name], os.path.join(ROOT, "tests", name + ".cpp"), "-L" + LIBDIR,
                               "-lpiehip", "-Wl,-rpath," + LIBDIR, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-ldl"])
    return fake, exes


def rand_limbs(rng, q, shape, N):
    out = np.zeros(shape + (len(q), N), dtype=np.uint64)
    for i, qi in enumerate(q):
        out[..., i, :] = rng.integers(0, int(qi), shape + (N,), dtype=np.uint64)
    return out


def wait_all(procs, timeout=150):
    """[(return code, stdout, stderr)]; everybody is killed when one of them does not end in time"""
    outs = []
    for p in procs:
        try:
            so, se = p.communicate(timeout=timeout)
        except subprocess.TimeoutExpired:
            for pp in procs:
                pp.kill()
            raise
        outs.append((p.returncode, so.decode(), se.decode()))
    return outs


def client_session(a, cl, cc, N, L, t, K, E, b, clientset):
    """the client of one session over socket `a` (the framing of host/WireFraming.hpp) -> (evk, minus_ct, idx_ct, results [b][2][L][N])"""
    def send(payload):
        a.sendall(struct.pack("i", len(payload)) + payload)

    def recv():
        hdr = b""
        while len(hdr) < 4:
            chunk = a.recv(4 - len(hdr))
            if not chunk:
                raise ConnectionError("server closed the channel")
            hdr += chunk
        n, = struct.unpack("i", hdr)
        buf = bytearray()
        while len(buf) < n:
            chunk = a.recv(min(1 << 20, n - len(buf)))
            if not chunk:
                raise ConnectionError("server closed the channel")
            buf += chunk
        return bytes(buf)

    def ct_msg(ct):
        return struct.pack("IIIIQ", 0x48454950, 1, L, N, 0) + np.ascontiguousarray(ct, dtype=np.uint64).tobytes()

    evk = cl.runSetUpPhase()
    moduli = np.zeros(15, dtype=np.uint64)
    moduli[:2 * L + 1] = cc.moduli[:2 * L + 1]
    send(struct.pack("IIQ", N, L, t) + moduli.tobytes())
    send(b"")
    send(np.ascontiguousarray(evk, dtype=np.uint64).tobytes())
    assert recv() == b""
    minus_ct, idx_ct = cl.runOfflinePhase(clientset)
    assert recv() == b""
    send(ct_msg(minus_ct))
    for h in range(K):
        for j in range(E):
            send(ct_msg(idx_ct[h, j]))
    res = []
    for _ in range(b):
        m = recv()
        assert struct.unpack("IIIIQ", m[:24]) == (0x48454950, 1, L, N, 0)
        res.append(np.frombuffer(m[24:], dtype=np.uint64).reshape(2, L, N))
    return evk, minus_ct, idx_ct, np.stack(res)


def start_servers(exe, fake, G, setfile, k, e, K, E, b):
    """G server processes (rank 0 holds the client's channel) -> (the client's socket, the processes)"""
    a, bsock = socket.socketpair()
    sides = [socket.socketpair() for _ in range(G - 1)]
    env = dict(os.environ, PIEHIP_TEST_SEEDS="1,2,3", PIEHIP_TEST_TIMEOUT_MS="20000")
    side0 = ",".join(str(s[0].fileno()) for s in sides) or "-"
    tail = [str(setfile), str(k), str(e), str(K), str(E), str(b)]
    procs = [subprocess.Popen([exe, fake, "0", str(G), "0", str(bsock.fileno()), side0] + tail,
                              pass_fds=[bsock.fileno()] + [s[0].fileno() for s in sides], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE)]
    for r in range(1, G):
        procs.append(subprocess.Popen([exe, fake, str(r), str(G), "0", "-1", str(sides[r - 1][1].fileno())] + tail,
                                      pass_fds=[sides[r - 1][1].fileno()], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE))
    bsock.close()
    for s in sides:
        s[0].close()
        s[1].close()
    return a, procs


def layers_differing_from_oracle(ob, N, L, t, server, k, e, K, E, b, idx_ct, minus_ct, evk, res):
    """the bin layers whose result ciphertext is not the oracle's, bit for bit: the same table (the server's default hash seed, the
    test secrets 1, 2, 3 of PIEHIP_TEST_SEEDS)"""
    import concurrent.futures
    o = ob.Oracle(N, L, t)
    tab = ob.Tabulation(987654321, k + K)
    tbl = ob.hct_build(tab, server, k, e, K, b, E, evict_seed=1)
    ob.hct_shuffle_bins(tbl, 2)
    slots = ob.pack_db(tbl)
    mask_slots = ob.masks(t, b, k * e, 3)
    idx = np.ascontiguousarray(idx_ct, dtype=np.uint64).reshape(K, E, 2, L, N)
    minus = np.ascontiguousarray(minus_ct, dtype=np.uint64).reshape(2, L, N)
    evk = np.ascontiguousarray(evk, dtype=np.uint64).reshape(L, 2, L, N)

    def layer_ok(bn):
        db = np.stack([o.encode_eval(slots[h, bn, j]) for h in range(K) for j in range(E)]).reshape(K, 1, E, L, N)
        return bool((res[bn] == o.pie_run(idx, minus, db, o.encode_eval(mask_slots[bn])[None], evk)[0]).all())
    with concurrent.futures.ThreadPoolExecutor(max_workers=8) as pool:
        ok = list(pool.map(layer_ok, range(b)))
    return [i for i, v in enumerate(ok) if not v]
