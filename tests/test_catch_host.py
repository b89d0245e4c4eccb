"""tests/catch_cases.py pinned on the CPU, and the catch list's ABI.

The yardstick is compared with the existing restatement (``propose_cases.restate``:
a record exactly where dup == 2 or pclass is 2 or 4, against the logged message
of the same key) on the seeded mixes tests/test_gpu_catch.py runs, whose record
counts are asserted here because that file's coverage claims rest on them; then
with hand-worked batches, one per kind.  The ABI tests need the built library
but no GPU."""
import ctypes
import os
import subprocess
from collections import Counter

import pytest

import catch_cases as CC
import hd_pyoracle as O
import log_cases as LC
import propose_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEVER = CC.NEVER
H = 5


# (mix, total records, dup 2, pclass 2, pclass 4)
MIXES = [
    (lambda: CC.mix_3000(True), 1897, 1828, 48, 21),
    (lambda: CC.mix_3000(False), 1893, 1822, 71, 0),
    (CC.mix_40, 4, 3, 0, 1),
    (CC.mix_5000, 3360, 2744, 429, 187),
]


@pytest.mark.parametrize("case", range(len(MIXES)))
def test_yardstick_against_the_restatement(case):
    make, total, n_dup2, n_pc2, n_pc4 = MIXES[case]
    sigs, sched, ob, verdicts, value_ok = make()
    recs = CC.records(ob, verdicts, sched)
    want = PC.restate(ob, verdicts, 3, sched, value_ok)
    n = len(ob)
    assert [i for i, _, _ in recs] == [i for i in range(n) if want.dup[i] == 2 or want.pclass[i] in (2, 4)]
    kinds = Counter(k for _, k, _ in recs)
    assert (len(recs), kinds[1] + kinds[2], kinds[3], kinds[4]) == (total, n_dup2, n_pc2, n_pc4)
    for i, k, a in recs:
        if k == CC.OUT_OF_TURN:
            assert a == NEVER and want.pclass[i] == 4
            continue
        assert a < i and (ob.height[a], ob.round[a]) == (ob.height[i], ob.round[i])
        if k == CC.DOUBLE_PROPOSE:
            assert want.pclass[i] == 2 and want.pclass[a] == 0 and ob.mtype[a] == ob.mtype[i] == O.PROPOSE
            assert not PC.propose_equal(ob, i, a)
            assert a == want.proposes[(ob.height[i], ob.round[i])]
        else:
            assert want.dup[i] == 2 and want.dup[a] == 0
            assert ob.mtype[a] == ob.mtype[i] == (O.PREVOTE if k == CC.DOUBLE_PREVOTE else O.PRECOMMIT)
            assert ob.frm[a] == ob.frm[i] and ob.value[a] != ob.value[i]


def test_stream_records_name_kept_messages():
    """The 40-message stream at every cut: every `against` of the second insert
    resolves through the position map (a KeyError would be the finding), some
    cut puts one below base, and the two inserts' lists together are the
    one-shot list under the index map."""
    sigs, sched, ob, verdicts, value_ok = CC.mix_40()
    whole = CC.records(ob, verdicts, sched)
    below = 0
    for c in range(1, 40):
        st = CC.Stream(H, 2, sched)
        e1, r1 = st.push(*LC.cut(ob, verdicts, value_ok, 0, c))
        e2, r2 = st.push(*LC.cut(ob, verdicts, value_ok, c, 40))
        assert e1.base == 0 and r1 == [x for x in whole if x[0] < c]
        assert [i - e2.base + c for i, _, _ in r2] == [i for i, _, _ in whole if i >= c]
        for (i, k, a), (wi, wk, wa) in zip(r2, [x for x in whole if x[0] >= c]):
            assert k == wk and i >= e2.base
            if wa == NEVER:
                assert a == NEVER
            elif wa < c:
                assert a == e1.logpos[wa] < e2.base
                below += 1
            else:
                assert a == e2.base + (wa - c)
    assert below > 0


# ---- hand-worked batches ---------------------------------------------------------------
def _sig(k):
    return O.sha256(b"c" + bytes([k]))


V, W = O.canonical_value(H, 0), O.canonical_value(H, 1)


def _batch(msgs):
    ob = O.Batch()
    for m in msgs:
        ob.append(*m, bytes(65))
    return ob


def test_double_prevote_by_hand():
    ob = _batch([
        (O.PREVOTE, H, 0, -1, V, _sig(0)),        # 0 logged
        (O.PREVOTE, H, 0, -1, V, _sig(1)),        # 1 logged
        (O.PREVOTE, H, 0, -1, V, _sig(0)),        # 2 the same again: dropped silently
        (O.PREVOTE, H, 0, -1, W, _sig(0)),        # 3 double, against 0
        (O.PREVOTE, H, 1, -1, W, _sig(0)),        # 4 another round: logged
        (O.PRECOMMIT, H, 0, -1, W, _sig(0)),      # 5 another type: logged
        (O.PREVOTE, H, 0, -1, O.NIL_VALUE, _sig(1)),   # 6 double, against 1
        (O.PREVOTE, H, 0, -1, W, _sig(0)),        # 7 double again, still against 0
    ])
    assert CC.records(ob, [O.VALID] * 8) == [(3, 1, 0), (6, 1, 1), (7, 1, 0)]


def test_double_precommit_by_hand():
    ob = _batch([
        (O.PRECOMMIT, H, 2, -1, V, _sig(3)),      # 0 logged
        (O.PREVOTE, H, 2, -1, W, _sig(3)),        # 1 a prevote: its own log
        (O.PRECOMMIT, H, 2, -1, W, _sig(3)),      # 2 double, against 0
        (O.PRECOMMIT, H + 1, 2, -1, W, _sig(3)),  # 3 another height: logged
        (O.PRECOMMIT, H + 1, 2, -1, V, _sig(3)),  # 4 double, against 3
        (O.PRECOMMIT, H, 2, -1, V, _sig(3)),      # 5 equal to 0: silent
        (O.PRECOMMIT, H, 2, -1, V, _sig(4)),      # 6 logged
    ])
    assert CC.records(ob, [O.VALID] * 7) == [(2, 2, 0), (4, 2, 3)]


def test_double_propose_by_hand():
    ob = _batch([
        (O.PROPOSE, H, 0, -1, V, _sig(1)),        # 0 logged
        (O.PROPOSE, H, 0, -1, V, _sig(1)),        # 1 Equal: silent
        (O.PROPOSE, H, 0, -1, W, _sig(1)),        # 2 another value: double, against 0
        (O.PROPOSE, H, 0, 0, V, _sig(1)),         # 3 another valid round: double
        (O.PROPOSE, H, 0, -1, V, _sig(2)),        # 4 another From (no schedule): double
        (O.PROPOSE, H, 1, -1, W, _sig(2)),        # 5 another round: logged
        (O.PROPOSE, H, -1, -1, W, _sig(2)),       # 6 round <= InvalidRound: no candidate
        (O.PROPOSE, H, 1, -1, V, _sig(2)),        # 7 double, against 5
        (O.PREVOTE, H, 0, -1, W, _sig(1)),        # 8 a vote
    ])
    assert CC.records(ob, [O.VALID] * 9) == [(2, 3, 0), (3, 3, 0), (4, 3, 0), (7, 3, 5)]


def test_out_of_turn_propose_by_hand():
    sched = [_sig(k) for k in range(4)]           # (5 + 0) % 4 = 1, (5 + 1) % 4 = 2
    ob = _batch([
        (O.PROPOSE, H, 0, -1, V, _sig(2)),        # 0 out of turn
        (O.PROPOSE, H, 0, -1, V, _sig(1)),        # 1 in turn: logged
        (O.PROPOSE, H, 0, -1, W, _sig(2)),        # 2 out of turn: the schedule is checked before the log
        (O.PROPOSE, H, 0, -1, W, _sig(1)),        # 3 in turn, another value: double, against 1
        (O.PROPOSE, H, 1, -1, V, _sig(1)),        # 4 out of turn at round 1
        (O.PROPOSE, 0, 0, -1, V, _sig(3)),        # 5 height <= 0 under a schedule: no candidate, no record
        (O.PROPOSE, H, 1, -1, V, _sig(2)),        # 6 in turn: logged
    ])
    assert CC.records(ob, [O.VALID] * 7, sched) == [(0, 4, NEVER), (2, 4, NEVER), (3, 3, 1), (4, 4, NEVER)]
    assert CC.named(CC.records(ob, [O.VALID] * 7, sched))[2] == (3, "double_propose", 1)
    # without a schedule nobody is out of turn: 0 and 4 are logged and the others of their rounds conflict
    # with them (1 by its From alone); 5 is the logged propose of (0, 0)
    assert CC.records(ob, [O.VALID] * 7) == [(1, 3, 0), (2, 3, 0), (3, 3, 0), (6, 3, 4)]


def test_logged_vote_follows_an_invalid_copy():
    """The first message of the key is not VALID, so the second one is the
    logged vote and the conflict names it, not the invalid copy."""
    ob = _batch([
        (O.PREVOTE, H, 0, -1, W, _sig(0)),        # 0 not VALID: never reaches the insert
        (O.PREVOTE, H, 0, -1, V, _sig(1)),        # 1 logged
        (O.PREVOTE, H, 0, -1, V, _sig(0)),        # 2 logged: the first VALID vote of its key
        (O.PREVOTE, H, 0, -1, W, _sig(0)),        # 3 double, against 2
        (O.PREVOTE, H, 0, -1, W, _sig(1)),        # 4 not VALID
        (O.PREVOTE, H, 0, -1, O.NIL_VALUE, _sig(0)),   # 5 double, against 2
    ])
    verdicts = [O.BAD_RS, O.VALID, O.VALID, O.VALID, O.BAD_RS, O.VALID]
    assert CC.records(ob, verdicts) == [(3, 1, 2), (5, 1, 2)]


# ---- ABI ---------------------------------------------------------------------------------
CATCH_SYMBOLS = ("hd_decide_catch", "hd_decide_catch_device_bitmap", "hd_log_insert_catch",
                 "hd_log_insert_catch_device_bitmap")


def _lib_path():
    from hyperdrive_amd import build
    if not os.path.exists(build.LIB):
        build.build()
    return build.LIB


def test_library_exports_the_catch_entries():
    out = subprocess.run(["nm", "-D", "--defined-only", _lib_path()], capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert set(CATCH_SYMBOLS) <= exported
    from hyperdrive_amd import _lib
    assert set(CATCH_SYMBOLS) <= set(_lib.SIGNATURES)


def test_catch_out_layout_matches_the_header(tmp_path):
    import shutil
    from hyperdrive_amd import _lib
    if not shutil.which("gcc"):
        pytest.skip("gcc absent")
    fields = [f for f, _ in _lib.HdCatchOut._fields_]
    assert fields == ["cap", "n", "index", "against", "kind"]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "hd_log.h"', "int main(void) {",
             'printf("size %zu\\n", sizeof(hd_catch_out));']
    lines += [f'printf("{f} %zu\\n", offsetof(hd_catch_out, {f}));' for f in fields]
    lines += ['printf("kinds %d %d %d %d\\n", HD_CATCH_DOUBLE_PREVOTE, HD_CATCH_DOUBLE_PRECOMMIT, '
              'HD_CATCH_DOUBLE_PROPOSE, HD_CATCH_OUT_OF_TURN);', "return 0; }"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = dict(line.split(" ", 1) for line in
               subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["size"]) == ctypes.sizeof(_lib.HdCatchOut)
    for f in fields:
        assert int(got[f]) == getattr(_lib.HdCatchOut, f).offset, f
    assert got["kinds"].split() == [str(k) for k in sorted(CC.NAMES)]
    from hyperdrive_amd import verify
    assert verify.CATCH_NAMES == CC.NAMES


def test_null_arguments_without_a_device():
    """HD_EINVAL before any device work: no context exists here."""
    from hyperdrive_amd import _lib
    lib = _lib.load(_lib_path())
    assert lib.hd_abi_version() == 2
    c = _lib.HdCatchOut(0, 7, None, None, None)
    assert lib.hd_decide_catch(None, None, None, None, None, None, None) == _lib.HD_EINVAL
    assert lib.hd_decide_catch(None, None, None, None, None, None, ctypes.byref(c)) == _lib.HD_EINVAL
    assert lib.hd_decide_catch_device_bitmap(None, None, None, None, None, None, None, None) == _lib.HD_EINVAL
    assert lib.hd_decide_catch_device_bitmap(None, None, None, None, None, None, ctypes.byref(c),
                                             None) == _lib.HD_EINVAL
    assert lib.hd_log_insert_catch(None, None, None, None, None, None, None, None) == _lib.HD_EINVAL
    assert lib.hd_log_insert_catch(None, None, None, None, None, None, None, ctypes.byref(c)) == _lib.HD_EINVAL
    assert lib.hd_log_insert_catch_device_bitmap(None, None, None, None, None, None, None, None,
                                                 None) == _lib.HD_EINVAL
    assert lib.hd_log_insert_catch_device_bitmap(None, None, None, None, None, None, None, ctypes.byref(c),
                                                 None) == _lib.HD_EINVAL
    assert c.n == 7                                # rejected before anything was written
