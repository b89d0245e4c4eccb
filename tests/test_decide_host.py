"""hd_decide without a GPU: argument checks, the ctypes mirror of hd_decide_out
against gcc on the header, and the propose restatement (tests/propose_cases.py,
the yardstick of tests/test_gpu_decide.py) against hand-worked cases of
process_test.go's propose specs."""
import ctypes
import os
import shutil
import subprocess

import pytest

import propose_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from hyperdrive_amd import _lib, build
    if not os.path.exists(build.LIB):
        build.build()
    return _lib, _lib.load(build.LIB)


def test_null_arguments_are_rejected_without_a_gpu():
    L, lib = _lib()
    out, cin, b = L.HdDecideOut(), L.HdDecideIn(), L.HdBatch()
    v = (ctypes.c_uint8 * 4)()
    assert lib.hd_decide(None, None, None, None, None) == L.HD_EINVAL
    assert lib.hd_decide(None, ctypes.byref(b), v, ctypes.byref(cin), ctypes.byref(out)) == L.HD_EINVAL
    assert lib.hd_decide_device_bitmap(None, ctypes.byref(b), v, ctypes.byref(cin), ctypes.byref(out),
                                       None) == L.HD_EINVAL
    # a NULL `out` (and an `out` without arrays) is refused before the context is touched
    ctx = ctypes.c_void_p(1)
    assert lib.hd_decide(ctx, ctypes.byref(b), v, ctypes.byref(cin), None) == L.HD_EINVAL
    assert lib.hd_decide(ctx, ctypes.byref(b), v, ctypes.byref(cin), ctypes.byref(out)) == L.HD_EINVAL
    assert lib.hd_decide(ctx, ctypes.byref(b), v, None, ctypes.byref(out)) == L.HD_EINVAL
    assert lib.hd_decide_device_bitmap(ctx, ctypes.byref(b), v, ctypes.byref(cin), None, None) == L.HD_EINVAL
    assert lib.hd_abi_version() == 2


def test_decide_struct_layouts_match_the_header(tmp_path):
    L, _ = _lib()
    if not shutil.which("gcc"):
        pytest.fail("gcc absent")
    structs = {"hd_decide_out": L.HdDecideOut, "hd_decide_in": L.HdDecideIn}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "hd_verify.h"', "int main(void) {"]
    for cname, py in structs.items():
        lines.append(f'printf("{cname} size %zu\\n", sizeof({cname}));')
        for fname, _t in py._fields_:
            lines.append(f'printf("{cname} {fname} %zu\\n", offsetof({cname}, {fname}));')
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = {}
    for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines():
        c, f, v = line.split()
        got[(c, f)] = int(v)
    for cname, py in structs.items():
        assert got[(cname, "size")] == ctypes.sizeof(py), cname
        for fname, _t in py._fields_:
            assert got[(cname, fname)] == getattr(py, fname).offset, (cname, fname)
    assert L.HdDecideOut.ROW_FIELDS == list(PC.ROW_FIELDS)


def test_python_face():
    import hyperdrive_amd as hd
    from hyperdrive_amd import quorum, verify
    assert hd.DecideResult is verify.DecideResult
    assert verify.DECISION_KEYS == PC.BIT_KEYS
    assert "481" in quorum.__doc__


# ---- the yardstick itself -------------------------------------------------
def _sig(k):
    import hd_pyoracle as O
    return O.sha256(b"p" + bytes([k]))


def _batch(msgs):
    import hd_pyoracle as O
    b = O.Batch()
    for t, h, r, vr, value, frm in msgs:
        b.append(t, h, r, vr, value, frm, bytes(65))
    return b


def test_restatement_scheduled_proposer_and_out_of_turn(oracle):
    """process_test.go:1090-1120 / 4046: a propose from another signatory than
    the scheduled one is not inserted and is caught as out of turn; the
    scheduled proposer's is logged (592-640)."""
    O = oracle
    sched = [_sig(k) for k in range(4)]
    v = O.canonical_value(1, 0)
    b = _batch([(O.PROPOSE, 1, 0, -1, v, sched[0]),       # turn of (1 + 0) % 4 = 1: out of turn
                (O.PROPOSE, 1, 0, -1, v, sched[1]),
                (O.PROPOSE, 1, 2, -1, v, sched[3])])      # (1 + 2) % 4 = 3
    w = PC.restate(b, [O.VALID] * 3, 1, sched)
    assert w.pclass == [4, 0, 0]
    assert w.proposes == {(1, 0): 1, (1, 2): 2}
    assert [(x["height"], x["round"], x["rep"], x["propose"]) for x in w.rows] == [(1, 0, 1, 1), (1, 2, 2, 2)]
    # no scheduler: the first one is logged, the second is its double (Equal compares From)
    w = PC.restate(b, [O.VALID] * 3, 1, None)
    assert w.pclass == [0, 2, 0]


def test_restatement_double_and_identical_propose(oracle):
    """process_test.go:3807: two different proposes of one round -> the second
    is caught; an identical copy is dropped without a catch (process.go:788-795)."""
    O = oracle
    s = _sig(0)
    v, v2 = O.canonical_value(1, 0), O.canonical_value(1, 1)
    b = _batch([(O.PROPOSE, 1, 0, -1, v, s), (O.PROPOSE, 1, 0, -1, v, s), (O.PROPOSE, 1, 0, -1, v2, s),
                (O.PROPOSE, 1, 0, 0, v, s)])
    w = PC.restate(b, [O.VALID] * 4, 1)
    assert w.pclass == [0, 1, 2, 2]
    assert w.proposes == {(1, 0): 0}


def test_restatement_invalid_round_nil_value_and_validator(oracle):
    """process_test.go:770-802 (round -1 is ignored), 804-862 (a nil propose
    is logged as invalid: no trace entry), 732-768 (the validator rejects)."""
    O = oracle
    s = _sig(0)
    v = O.canonical_value(1, 0)
    b = _batch([(O.PROPOSE, 1, -1, -1, v, s), (O.PROPOSE, 1, 0, -1, O.NIL_VALUE, s), (O.PROPOSE, 1, 1, -1, v, s),
                (O.PROPOSE, 1, 2, -1, v, s)])
    w = PC.restate(b, [O.VALID] * 4, 0, None, value_ok=[1, 1, 0, 1])
    assert w.pclass == [3, 0, 0, 0]
    assert [(x["round"], x["flags"], x["trace"]) for x in w.rows] == [(0, 1, 0), (1, 1, 0), (2, 7, 1)]
    assert [x["bits"] >> 4 & 1 for x in w.rows] == [0, 0, 1]          # skip with f = 0: f + 1 = 1


def test_restatement_f_unique_signatories_with_a_propose(oracle):
    """process_test.go:3510-3607: one propose and f prevotes from f unique
    signatories do not skip; 3379-3508: f votes and a propose from an f+1-th
    signatory do (process.go:751, 813-816)."""
    O = oracle
    f = 3
    v = O.canonical_value(1, 5)
    votes = [(O.PREVOTE, 1, 5, -1, v, _sig(k)) for k in range(f)]
    w = PC.restate(_batch(votes + [(O.PROPOSE, 1, 5, -1, v, _sig(0))]), [O.VALID] * (f + 1), f)
    assert (w.row(1, 5)["trace"], w.row(1, 5)["flags"], w.decisions[(1, 5)]["skip"]) == (f, 3, False)
    w = PC.restate(_batch(votes + [(O.PROPOSE, 1, 5, -1, v, _sig(9))]), [O.VALID] * (f + 1), f)
    assert (w.row(1, 5)["trace"], w.row(1, 5)["flags"], w.decisions[(1, 5)]["skip"]) == (f + 1, 7, True)


def test_restatement_valid_round_counts(oracle):
    """process_test.go:1170-1540: 2f+1 prevotes for the propose's value in its
    valid round (process.go:486-494)."""
    O = oracle
    f = 1
    v = O.canonical_value(1, 1)
    pv = [(O.PREVOTE, 1, 1, -1, v, _sig(k)) for k in range(2 * f + 1)]
    w = PC.restate(_batch(pv + [(O.PROPOSE, 1, 3, 1, v, _sig(0))]), [O.VALID] * (2 * f + 2), f)
    x = w.row(1, 3)
    assert (x["pv_validround"], x["bits"] >> 7, x["prevotes"], x["rep"]) == (2 * f + 1, 1, 0, 2 * f + 1)
    w = PC.restate(_batch(pv[:2 * f] + [(O.PROPOSE, 1, 3, 1, v, _sig(0))]), [O.VALID] * (2 * f + 1), f)
    assert (w.row(1, 3)["pv_validround"], w.row(1, 3)["bits"] >> 7) == (2 * f, 0)


def test_restatement_turn_uses_uint64_arithmetic(oracle):
    O = oracle
    sched = [_sig(k) for k in range(7)]
    h = 2**63 - 1
    assert PC.scheduled(sched, h, 5) == sched[(h + 5) % 7]
    assert PC.scheduled(sched, 3, 2**63 - 1) == sched[(3 + 2**63 - 1) % 7]
