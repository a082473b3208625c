"""The folded column reduction on the device, word for word against its model (tests/fold_reduce.py): tests/fold_reduce_check, a
program of its own that compiles the product's definitions -- colacc_fold<false>, colacc_fold<true> (csrc/stage_a_common.h) and
colacc_fold_to_4q (csrc/ntt16_kernel.h) -- and runs them on the columns it is given, one launch per modulus.

  d        tests/test_fold_reduce.py's: 1, the nine of the default chain at N = 16384, the largest at N = 32768, 2^27 - 1
  columns  the crafted ones at z < 2^123 and at z < 2^124 (the W124 sites take the same block) and one wave of random ones per width
The lazy words must equal the model's r itself (the same representative, not only the same residue), the canonical ones z mod q.
One run of the program, as a fresh child process."""
import os
import subprocess

import numpy as np
import pytest

from tests import fold_reduce as fr
from tests.param_chains import uniform

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nested_hashing_psi_amd", "csrc")
EXE = os.path.join(CSRC, "build", "fold_reduce_check")


def _cases(d):
    out = []
    for bits in (123, 124):
        out += [c for _, c in fr.crafted(d, bits)]
        out += fr.random_columns(fr.rng_for(d, bits), bits, 64)
    return out


def test_fold_blocks_match_the_model_on_the_device(tmp_path):
    c3 = [(1 << 60) - q for q in uniform(16384, 9)]
    ds = fr.check_ds(c3, max((1 << 60) - q for q in uniform(32768, 13)))
    cases = [_cases(d) for d in ds]
    n = len(cases[0])
    assert all(len(c) == n for c in cases)
    src, dst = str(tmp_path / "in.u64"), str(tmp_path / "out.u64")
    np.array(cases, dtype=np.uint64).tofile(src)
    subprocess.check_call(["make", "-j8", "-C", CSRC, "build/fold_reduce_check"], stdout=subprocess.DEVNULL)
    r = subprocess.run([EXE, src, dst, str(n)] + [str(d) for d in ds], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       universal_newlines=True, timeout=120)
    assert r.returncode == 0, "status %d\n%s" % (r.returncode, r.stdout[-4000:])
    got = np.fromfile(dst, dtype=np.uint64).reshape(len(ds), n, 3)
    bad = []
    for k, d in enumerate(ds):
        q = (1 << 60) - d
        for i, c in enumerate(cases[k]):
            lazy, canon = fr.fold_lazy(*c, d), fr.value(*c) % q
            assert fr.fold_canon(*c, d) == canon and lazy < 4 * q
            g = [int(v) for v in got[k, i]]
            if g != [lazy, canon, lazy]:
                bad.append((d, c, g, [lazy, canon, lazy]))
    assert not bad, bad[:4]
