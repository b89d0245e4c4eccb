"""The single-operation tables of tests/math_cases.py through the host build of
the device headers (the CPU twin of tests/test_gpu_devmath.py): proves the
tables and their Python references right before a GPU sees them, and shows,
with Python models, that the rows named for a rare branch or a special
wavefront are what they are named."""
import os

import numpy as np
import pytest

import math_cases as mc


@pytest.mark.parametrize("op", sorted(mc.OPS, key=mc.OPS.get))
def test_table_on_host_build(hostmath, op):
    inp = mc.table(op)
    out = hostmath.mathcheck(mc.OPS[op], inp)
    mc.check(op, inp, out)


def test_row_words_match_the_library_header(hostmath):
    import ctypes
    for op, code in mc.OPS.items():
        iw, ow = ctypes.c_uint32(), ctypes.c_uint32()
        assert hostmath.L.hdh_mathcheck_words(code, ctypes.byref(iw), ctypes.byref(ow)) == 0
        assert mc.table(op).shape[1] == iw.value, op
    assert hostmath.L.hdh_mathcheck_words(99, ctypes.byref(iw), ctypes.byref(ow)) == -1


def test_device_entry_checks_its_arguments_before_any_device_work():
    """hd_mathcheck rejects a bad n, block size, op or pointer without touching a GPU (none is needed here),
    and its row sizes are the host harness's"""
    import ctypes

    from hyperdrive_amd import _lib, build
    if not os.path.exists(build.LIB):
        build.build()
    lib = _lib.load()
    inp = mc.table("fe_mul")[:4]
    out = np.zeros((4, 9), np.uint32)
    i, o = inp.ctypes.data, out.ctypes.data
    assert lib.hd_mathcheck(0, 0, 0, 64, i, o) == -1
    assert lib.hd_mathcheck(0, 0, 65537, 64, i, o) == -1
    assert lib.hd_mathcheck(0, 0, 4, 128, i, o) == -1
    assert lib.hd_mathcheck(0, 17, 4, 64, i, o) == -1
    assert lib.hd_mathcheck(0, 0, 4, 64, None, o) == -1
    assert lib.hd_mathcheck(0, 0, 4, 64, i, None) == -1
    assert lib.hd_mathcheck_words(48, None, None) == -1
    for op, code in mc.OPS.items():
        iw, ow = ctypes.c_uint32(), ctypes.c_uint32()
        assert lib.hd_mathcheck_words(code, ctypes.byref(iw), ctypes.byref(ow)) == 0
        assert iw.value == mc.table(op).shape[1], op


def test_raw_field_rows_equal_hdh_fe_raw(hostmath):
    """the rows are the same arithmetic as the older raw-limb entry (tests/test_field_bounds.py)"""
    from test_field_bounds import raw
    for op, code in (("fe_mul", 0), ("fe_sqr", 1), ("fe_norm_weak", 2), ("fe_normalize", 3)):
        inp = mc.table(op)[:80]
        out = hostmath.mathcheck(mc.OPS[op], inp)
        for i, o in zip(inp, out):
            a = [int(x) for x in i[:9]]
            b = [int(x) for x in i[9:18]] if len(i) > 9 else None
            assert raw(hostmath, code, a, b) == [int(x) for x in o]


def test_checks_are_live(hostmath):
    """a wrong word fails its check: every op's first output row, one bit flipped"""
    for op in mc.OPS:
        inp = mc.table(op)[:1]
        out = hostmath.mathcheck(mc.OPS[op], inp).copy()
        out[0, 0] ^= 1
        with pytest.raises(AssertionError):
            mc.check(op, inp, out)


def test_sc_reduce_branch_rows():
    """the rows named for sc_reduce's two last branches take them (the three folds restated in Python), the
    rows just below do not, and random 512-bit values take neither"""
    for t in mc.REDUCE_CY:
        r, cy, ge = mc.sc_reduce_model(t)
        assert cy and not ge and r == t % mc.N and t >> 256
    for t in mc.REDUCE_GE:
        r, cy, ge = mc.sc_reduce_model(t)
        assert ge and not cy and r == t % mc.N
    assert sum(1 for t in mc.REDUCE_GE if t >> 256) >= 3          # reached through both earlier folds too
    for t in (mc._reduce_preimage(2 ** 256 - mc.C - 1), mc._reduce_preimage(mc.N - 1)):
        assert mc.sc_reduce_model(t) == (t % mc.N, False, False)
    taken = [mc.sc_reduce_model(t)[1:] for t in mc.reduce512_values()[-200:]]
    assert not any(cy or ge for cy, ge in taken)
    tab = {mc.unwords(r) for r in mc.table("sc_reduce512")}
    assert set(mc.REDUCE_CY + mc.REDUCE_GE) <= tab


def test_normalisation_branch_rows(hostmath):
    """fe_normalize's subtraction runs for p, p + 1 and 2^256 - 1 through the comparison with p, and for
    FE_TOP_OVERFLOW through the top limb (fe_normalize restated in Python says which); the host build agrees
    with the restatement on the whole table; sc_from_be_reduce's subtraction runs for n, n + 1, 2^256 - 1"""
    tab = [[int(x) for x in r] for r in mc.table("fe_normalize")]
    out = hostmath.mathcheck(mc.OPS["fe_normalize"], mc.table("fe_normalize"))
    took = {0: 0, 1: 0, 2: 0}
    for r, o in zip(tab, out):
        n, ge = mc.fe_normalize_model(r)
        assert n == [int(x) for x in o]
        took[ge] += 1
    assert took[0] > 100 and took[1] >= 2 and took[2] >= 3, took
    for v in (mc.P, mc.P + 1, 2 ** 256 - 1):
        assert mc.limbs(v) in tab and mc.fe_normalize_model(mc.limbs(v))[1] == 2
    for r in mc.FE_TOP_OVERFLOW:
        assert r in tab and mc.fe_normalize_model(r)[1] == 1
    assert [mc.LOOSE_MAX] * 9 in tab and all(mc.limbs(v) in tab for v in mc.FE_LOOSE_VALUES)
    tab = {mc.unwords(r) for r in mc.table("sc_from_be_reduce")}
    assert {mc.N, mc.N + 1, 2 ** 256 - 1} <= tab


@pytest.mark.parametrize("m", [mc.N, mc.P], ids=["n", "p"])
def test_inversion_wavefronts_are_as_named(m):
    rows, batches = mc.modinv_rows(m)
    assert all(b <= 17 for b in batches[0:64]) and max(batches[0:64]) == 17
    assert all(b == 18 for b in batches[64:128])
    assert all((b <= 17) == (k % 2 == 0) for k, b in enumerate(batches[128:192]))
    assert rows[192:256] == [0] * 64
    assert all(mc.divstep_count(x, m) <= 590 for x in rows)
    name = "sc_inv_divsteps" if m == mc.N else "fe_inv_divsteps"
    conv = mc.unwords if m == mc.N else mc.val
    assert [conv(r) for r in mc.table(name)[:256]] == rows[:256]


def test_divstep_model_matches_the_inverse():
    """the model's rule is the inversion's: run to g = 0 it leaves f = +-1 (the gcd)"""
    for m in (mc.N, mc.P):
        for x in mc.modinv_edges(m)[:20]:
            f, g, zeta = m, x, -1
            while g:
                if g & 1:
                    if zeta < 0:
                        zeta, f, g = -zeta - 2, g, (g - f) >> 1
                    else:
                        zeta, g = zeta - 1, (g + f) >> 1
                else:
                    zeta, g = zeta - 1, g >> 1
            assert f in (1, -1)


def test_chain_rows_are_as_named():
    rows = mc.chain_cases()
    assert all(not sk for r in rows[:64] for _, _, sk in r)
    models = [mc.chain_model(r) for r in rows]
    assert sum(1 for s, d, _ in models if d) >= 2 * (mc.CHAIN_LEN - 1)      # + and - at every step
    assert any(not s for s, _, _ in models)                                  # a sum that never starts
    assert any(r[0][2] and s and not d for r, (s, d, _) in zip(rows, models))   # a sum that starts late
    # both signs occur: a doubling (the true sum is finite) and a cancellation (it is infinity)
    assert any(d and w is not None for _, d, w in models) and any(d and w is None for _, d, w in models)
