"""tests/evidence_cases.py pinned against hand-worked batches (no GPU, no
library call): the rows of each kind of record, a logged message that sits in
an earlier insert, a resent vote with other signature bytes, an out-of-turn
propose.  Also the binding's side of the new calls: their names in
``_lib.SIGNATURES`` and the layout of the two new structs."""
import ctypes
import os
import shutil
import subprocess

import pytest

import catch_cases as CC
import evidence_cases as EC
import hd_pyoracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = 5
NEVER = EC.NEVER
sig = lambda k: O.sha256(b"g" + bytes([k]))
V, W = O.canonical_value(H, 0), O.canonical_value(H, 1)
SCHED = [sig(k) for k in range(4)]                                     # (5 + 0) % 4 = 1: sig(1) proposes round 0


def _batch(msgs, tag=b"e"):
    ob = O.Batch()
    for m in msgs:
        ob.append(*m, bytes(65))
    return EC.unique_sigs(ob, tag)


def _each_kind():
    s = sig(0)
    return [
        (O.PREVOTE, H, 0, -1, V, s),              # 0 logged
        (O.PRECOMMIT, H, 0, -1, V, s),            # 1 logged
        (O.PROPOSE, H, 0, -1, V, sig(1)),         # 2 in turn: logged
        (O.PREVOTE, H, 0, -1, W, s),              # 3 double prevote, against 0
        (O.PRECOMMIT, H, 0, -1, W, s),            # 4 double precommit, against 1
        (O.PREVOTE, H, 0, -1, V, s),              # 5 equal to 0: silent
        (O.PROPOSE, H, 0, 0, W, sig(1)),          # 6 double propose, against 2
        (O.PROPOSE, H, 0, -1, V, sig(2)),         # 7 out of turn
        (O.PRECOMMIT, H, 0, -1, O.NIL_VALUE, s),  # 8 double precommit again, against 1
    ]


def test_a_row_is_the_whole_message():
    ob = _batch(_each_kind())
    r = EC.row(ob, 6)
    assert len(r) == EC.ROW_BYTES == 154
    assert r[0] == O.PROPOSE and r[1:9] == (5).to_bytes(8, "little") and r[9:17] == bytes(8)
    assert r[17:25] == bytes(8) and EC.row(ob, 7)[17:25] == b"\xff" * 8        # valid_round 0 and -1
    assert r[25:57] == W and r[57:89] == sig(1) and r[89:] == ob.sig[6] == EC.sig_of(b"e", 6)
    assert len({bytes(s) for s in ob.sig}) == len(ob)                          # unique to each message
    assert EC.sig_of(b"e", 1) != EC.sig_of(b"f", 1)


def test_one_of_each_kind_in_one_insert():
    ob = _batch(_each_kind())
    m = EC.Kept(H, 1, SCHED)
    exp, recs, ev = m.push(ob, [O.VALID] * len(ob))
    assert recs == [(3, CC.DOUBLE_PREVOTE, 0), (4, CC.DOUBLE_PRECOMMIT, 1), (6, CC.DOUBLE_PROPOSE, 2),
                    (7, CC.OUT_OF_TURN, NEVER), (8, CC.DOUBLE_PRECOMMIT, 1)]
    r = lambda i: EC.row(ob, i)
    assert ev == [(r(3), r(0)), (r(4), r(1)), (r(6), r(2)), (r(7), EC.ZERO_ROW), (r(8), r(1))]
    assert exp.logpos == [0, 1, 2] + [NEVER] * 6 and m.kept == [r(0), r(1), r(2)] and m.kept_ok == [1, 1, 1]


def test_the_logged_message_sits_in_an_earlier_insert():
    msgs = _each_kind()
    a, b = _batch(msgs[:2], b"a"), _batch(msgs[2:], b"b")
    m = EC.Kept(H, 1, SCHED)
    _, recs, ev = m.push(a, [O.VALID] * 2)
    assert recs == [] and ev == [] and m.entries == 2
    exp, recs, ev = m.push(b, [O.VALID] * 7)
    # base 2: message i of b is 2 + i; 0 and 1 are log positions of the first insert, the propose is b's own
    assert recs == [(3, CC.DOUBLE_PREVOTE, 0), (4, CC.DOUBLE_PRECOMMIT, 1), (6, CC.DOUBLE_PROPOSE, 2),
                    (7, CC.OUT_OF_TURN, NEVER), (8, CC.DOUBLE_PRECOMMIT, 1)]
    assert ev == [(EC.row(b, 1), EC.row(a, 0)), (EC.row(b, 2), EC.row(a, 1)), (EC.row(b, 4), EC.row(b, 0)),
                  (EC.row(b, 5), EC.ZERO_ROW), (EC.row(b, 6), EC.row(a, 1))]
    assert ev[0][1][89:] == EC.sig_of(b"a", 0) and ev[2][1][89:] == EC.sig_of(b"b", 0)
    assert m.kept == [EC.row(a, 0), EC.row(a, 1), EC.row(b, 0)]
    # the same messages again: caught again, against the retained entries only, nothing kept
    again = _batch(msgs[2:], b"c")
    exp, recs, ev = m.push(again, [O.VALID] * 7)
    assert exp.kept == 0 and [a_ for _, _, a_ in recs] == [0, 1, 2, NEVER, 1]
    assert ev[2] == (EC.row(again, 4), EC.row(b, 0))


def test_a_resent_vote_keeps_the_first_signature():
    s = sig(0)
    first = _batch([(O.PREVOTE, H, 0, -1, V, s)], b"1")
    resent = _batch([(O.PREVOTE, H, 0, -1, V, s), (O.PREVOTE, H, 0, -1, W, s)], b"2")
    assert EC.row(first, 0)[:89] == EC.row(resent, 0)[:89] and EC.row(first, 0)[89:] != EC.row(resent, 0)[89:]
    m = EC.Kept(H, 1)
    m.push(first, [O.VALID])
    exp, recs, ev = m.push(resent, [O.VALID] * 2)
    assert exp.dup == [1, 2] and exp.logpos == [NEVER, NEVER] and recs == [(2, CC.DOUBLE_PREVOTE, 0)]
    assert ev == [(EC.row(resent, 1), EC.row(first, 0))] and m.kept == [EC.row(first, 0)]
    # both copies in one insert: the logged message is the batch's first
    m = EC.Kept(H, 1)
    one = _batch([(O.PREVOTE, H, 0, -1, V, s), (O.PREVOTE, H, 0, -1, V, s), (O.PREVOTE, H, 0, -1, W, s)], b"3")
    exp, recs, ev = m.push(one, [O.VALID] * 3)
    assert recs == [(2, CC.DOUBLE_PREVOTE, 0)] and ev == [(EC.row(one, 2), EC.row(one, 0))]
    assert m.kept == [EC.row(one, 0)]


def test_value_ok_and_messages_that_are_not_candidates():
    s = sig(0)
    ob = _batch([(O.PROPOSE, H, 0, -1, V, sig(1)), (O.PREVOTE, H + 1, 0, -1, V, s), (O.PREVOTE, H, 0, -1, V, s),
                 (O.PREVOTE, H, 1, -1, V, s)])
    m = EC.Kept(H, 1, SCHED)
    exp, recs, ev = m.push(ob, [O.VALID, O.VALID, O.BAD_RS, O.VALID], [0, 1, 1, 1])
    assert exp.logpos == [0, NEVER, NEVER, 1] and m.kept == [EC.row(ob, 0), EC.row(ob, 3)] and m.kept_ok == [0, 1]
    assert recs == [] and ev == []


def test_the_binding_declares_the_new_calls():
    from hyperdrive_amd import _lib
    for name in ("hd_log_keep_signatures", "hd_log_read", "hd_log_insert_evidence",
                 "hd_log_insert_evidence_device_bitmap"):
        assert name in _lib.SIGNATURES, name
    assert _lib.SIGNATURES["hd_log_insert_evidence"][1][-1]._type_ is _lib.HdEvidenceOut
    assert _lib.SIGNATURES["hd_log_read"][1][-1]._type_ is _lib.HdLogRows
    import hyperdrive_amd as hd
    assert issubclass(hd.EvidenceLogInsertResult, hd.CaughtLogInsertResult)


def test_struct_layouts_match_the_header(tmp_path):
    """hd_log_rows and hd_evidence_out as the C compiler lays them out (gcc on include/hd_log.h)."""
    from hyperdrive_amd import _lib
    if not shutil.which("gcc"):
        pytest.skip("gcc absent")
    structs = {"hd_log_rows": _lib.HdLogRows, "hd_evidence_out": _lib.HdEvidenceOut, "hd_log_info": _lib.HdLogInfo}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "hd_log.h"', "int main(void) {"]
    for cname, py in structs.items():
        lines.append(f'printf("{cname} size %zu\\n", sizeof({cname}));')
        for fname, _ in py._fields_:
            lines.append(f'printf("{cname} {fname} %zu\\n", offsetof({cname}, {fname}));')
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = {}
    for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n"):
        if line:
            parts = line.split()
            got[(parts[0], parts[1])] = int(parts[2])
    for cname, py in structs.items():
        assert got[(cname, "size")] == ctypes.sizeof(py), cname
        for fname, _ in py._fields_:
            assert got[(cname, fname)] == getattr(py, fname).offset, (cname, fname)
