"""The device arithmetic on the GPU, operation by operation, at its edges.

Every op of include/hd_mathcheck.h runs over its table (tests/math_cases.py,
proven on the host build by tests/test_math_cases.py) in blocks of 64 and 256
threads and at n = 1, 63, 64, 65, 200 and the whole table, so that one-lane,
63-lane, full and mixed wavefronts all occur (the inversion tables are laid
out by wavefront for modinv30's early exit).  The reference is Python
integers and oracle.point_add (math_cases.check); everything is exact.  For
the raw field ops the device limbs must also equal the host build's word for
word: both run the same integer algorithm, so a difference is code
generation."""
import ctypes

import numpy as np
import pytest

import math_cases as mc

pytestmark = pytest.mark.gpu

_host_cache = {}


def run_device(lib, op, inp, block):
    code = mc.OPS[op]
    iw, ow = ctypes.c_uint32(), ctypes.c_uint32()
    assert lib.hd_mathcheck_words(code, ctypes.byref(iw), ctypes.byref(ow)) == 0
    inp = np.ascontiguousarray(inp, dtype=np.uint32)
    assert inp.shape[1] == iw.value
    out = np.full((len(inp), ow.value), 0xA5A5A5A5, np.uint32)
    rc = lib.hd_mathcheck(0, code, len(inp), block, inp.ctypes.data, out.ctypes.data)
    if rc == -3:   # a device error: nothing more is started on this GPU
        pytest.exit(f"hd_mathcheck {op}: device error", returncode=3)
    assert rc == 0, (op, rc)
    return out


@pytest.fixture(scope="module")
def lib(gpu):
    from hyperdrive_amd import _lib
    return _lib.load()


def sizes(total):
    return sorted({n for n in (1, 63, 64, 65, 200, total) if n <= total})


@pytest.mark.parametrize("block", [64, 256])
@pytest.mark.parametrize("op", sorted(mc.OPS, key=mc.OPS.get))
def test_op_against_python_integers(lib, hostmath, op, block):
    inp = mc.table(op)
    if op not in _host_cache:
        _host_cache[op] = hostmath.mathcheck(mc.OPS[op], inp)
    host = _host_cache[op]
    for n in sizes(len(inp)):
        out = run_device(lib, op, inp[:n], block)
        mc.check(op, inp[:n], out)
        if op in mc.FE_OPS:
            bad = np.nonzero((out != host[:n]).any(axis=1))[0]
            assert len(bad) == 0, f"{op} n={n} block={block}: device limbs differ from the host build's at rows " \
                                  f"{bad[:8].tolist()}: {out[bad[0]].tolist()} != {host[bad[0]].tolist()}"
