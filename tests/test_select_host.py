"""hd_log_select (include/hd_log.h) on the host: the model of
tests/select_cases.py pinned on hand-worked logs, the binding, and the
kernel's own predicate and rank arithmetic.

hyperdrive_amd/csrc/hd_logselect.h is plain C++; the stand-alone program
tests/native/hd_logselect_check.cpp compiles the text k_log_sel_count and
k_log_sel_emit compile, under ASan + UBSan, and replays the two passes lane by
lane -- blocks of 256, wavefronts of 64, ballot prefixes -- over the match
patterns the GPU test builds its logs from.  The positions it stores must be the
model's, with a flag table of exactly L entries and an output of exactly
min(limit, cap) slots, so a read behind the log or a store behind cap is the
sanitizer's to catch."""
import ctypes
import os
import random
import shutil
import subprocess

import pytest

import evidence_cases as EC
import select_cases as SC

H = 5


@pytest.fixture(scope="module")
def prog():
    return SC.build_check(sanitize=True)


# ---- the model, by hand -----------------------------------------------------------------
def _hand_log(O):
    """Nine entries of height 5.  v, w: two values; a, b, c: three senders.
         0 propose   r0 v  a      3 precommit r0 v a     6 prevote   r1 w a
         1 prevote   r0 v  a      4 precommit r0 v b     7 precommit r1 w c
         2 prevote   r0 w  b      5 prevote   r0 v c     8 propose   r1 w b"""
    v, w = O.canonical_value(H, 0), O.canonical_value(H, 1)
    a, b, c = (SC.sender(k) for k in range(3))
    msgs = [(O.PROPOSE, 0, v, a), (O.PREVOTE, 0, v, a), (O.PREVOTE, 0, w, b), (O.PRECOMMIT, 0, v, a),
            (O.PRECOMMIT, 0, v, b), (O.PREVOTE, 0, v, c), (O.PREVOTE, 1, w, a), (O.PRECOMMIT, 1, w, c),
            (O.PROPOSE, 1, w, b)]
    ob = O.Batch()
    for t, r, val, frm in msgs:
        ob.append(t, H, r, -1, val, frm, bytes(65))
    ob = EC.unique_sigs(ob)
    return [EC.row(ob, i) for i in range(len(ob))], v, w, (a, b, c)


def test_model_on_a_hand_worked_log(oracle):
    kept, v, w, (a, b, c) = _hand_log(oracle)
    P, V, C = SC.PROPOSE, SC.PREVOTE, SC.PRECOMMIT
    sel = lambda *x, **k: SC.select(kept, *x, **k)
    assert sel(V, 0) == ([1, 2, 5], 3)                                  # PrevoteLogs[0]
    assert sel(C, 0) == ([3, 4], 2)                                     # PrecommitLogs[0]
    assert sel(P, 1) == ([8], 1) and sel(P, 2) == ([], 0)               # ProposeLogs[1], [2]
    assert sel(V, 0, sender=b) == ([2], 1)                              # PrevoteLogs[0][b]
    assert sel(V, 0, sender=SC.sender(9)) == ([], 0)
    assert sel(C, None, value=v) == ([3, 4], 2)                         # the precommits for v
    assert sel((V, C), None, value=w) == ([2, 6, 7], 3)
    assert sel((P, V, C)) == (list(range(9)), 9)
    assert sel((V, C), (0, 1), sender=a) == ([1, 3, 6], 3)
    assert sel((V, C), (1, 0)) == ([], 0)                               # lo > hi
    assert sel((V, C), value=w, sender=c, round=1) == ([7], 1)          # every field together
    # a propose with a vote's value stays out of a votes-only mask
    assert 0 not in sel((V, C), 0, value=v)[0] and sel((P, V, C), 0, value=v)[0][0] == 0
    # limit keeps the first k and the total; the range is inclusive at both ends and clipped to the log
    assert sel(V, 0, limit=2) == ([1, 2], 3) and sel(V, 0, limit=1) == ([1], 3) and sel(V, 0, limit=7) == ([1, 2, 5], 3)
    assert sel(V, 0, first=2) == ([2, 5], 2) and sel(V, 0, upto=4) == ([1, 2], 2) and sel(V, 0, upto=5) == ([1, 2, 5], 3)
    assert sel(V, 0, first=2, upto=2) == ([2], 1) and sel(V, 0, first=3, upto=2) == ([], 0)
    assert sel(V, 0, upto=100) == ([1, 2, 5], 3) and sel(V, 0, first=9) == ([], 0) and sel(V, 0, upto=-1) == ([], 0)
    assert sel(C, None, value=v, upto=3, limit=2) == ([3], 1)           # a certificate one message early


def test_model_of_flag_tables():
    f = [q in (1, 2, 5, 6) for q in range(9)]
    assert SC.select_flags(f, 0, 9, 0) == ([1, 2, 5, 6], 4)
    assert SC.select_flags(f, 2, 6, 0) == ([2, 5], 2) and SC.select_flags(f, 2, 99, 3) == ([2, 5, 6], 3)
    assert SC.select_flags(f, 0, 9, 1) == ([1], 4) and SC.select_flags(f, 9, 9, 0) == ([], 0)
    assert SC.select_flags([], 0, 5, 0) == ([], 0)


def test_patterns_cover_the_edges():
    for L in SC.SIZES:
        p = SC.patterns(L)
        assert all(len(f) == L for f in p.values())
        assert sum(p["every"]) == L and sum(p["none"]) == 0
        assert sum(p["first"]) == sum(p["last"]) == (1 if L else 0)
        assert sum(p["lanes_63_64"]) == min(max(L - 63, 0), 2) and sum(p["positions_255_256"]) == min(max(L - 255, 0), 2)
    assert {0, 1, 63, 64, 65, 255, 256, 257, 513, 1025} == set(SC.SIZES)


@pytest.mark.parametrize("mode", ["value", "from", "type", "round"])
def test_pattern_logs_match_their_pattern(oracle, mode):
    """pattern_log gives every entry a key of its own (so all are logged) and the query of its mode
    matches exactly the flagged entries."""
    O = oracle
    v, w, special = O.canonical_value(H, 0), O.canonical_value(H, 1), SC.sender(99)
    for L in (1, 65, 257):
        for name, flags in SC.patterns(L).items():
            ob = SC.pattern_log(O, H, flags, mode, v, w, special)
            assert len({(ob.mtype[i], ob.round[i], ob.frm[i]) for i in range(L)}) == L
            kept = [EC.row(ob, i) for i in range(L)]
            pos, total = SC.select(kept, **SC.pattern_query(mode, L, w, special))
            assert pos == [q for q in range(L) if flags[q]] and total == len(pos), (mode, L, name)


# ---- the binding ------------------------------------------------------------------------
def test_binding_of_the_select():
    from hyperdrive_amd import _lib, quorum
    from hyperdrive_amd.verify import DecideLog, DeviceSelection, LogSelection
    for name in ("hd_log_select", "hd_log_select_device"):
        assert name in _lib.SIGNATURES
    assert ctypes.sizeof(_lib.HdLogFilter) == 104 and ctypes.sizeof(_lib.HdLogSelected) == 8
    assert [n for n, _ in _lib.HdLogFilter._fields_] == ["round_lo", "round_hi", "type_mask", "flags", "pos_lo",
                                                         "pos_hi", "limit", "reserved", "value32", "from32"]
    assert (_lib.HD_LOG_SEL_VALUE, _lib.HD_LOG_SEL_FROM) == (1, 2)
    for m in ("select", "count", "select_device", "proposal", "votes", "vote_of", "certificate"):
        assert callable(getattr(DecideLog, m)), m
    assert callable(quorum.check_certificate) and LogSelection and DeviceSelection


def test_struct_layouts_match_the_header(tmp_path):
    """hd_log_filter and hd_log_selected as the C compiler lays them out"""
    from hyperdrive_amd import _lib
    assert shutil.which("gcc"), "gcc is needed for the layout check"
    structs = {"hd_log_filter": _lib.HdLogFilter, "hd_log_selected": _lib.HdLogSelected}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "hd_log.h"', "int main(void) {"]
    for cname, py in structs.items():
        lines.append(f'printf("{cname} size %zu\\n", sizeof({cname}));')
        lines += [f'printf("{cname} {f} %zu\\n", offsetof({cname}, {f}));' for f, _ in py._fields_]
    lines.append('printf("flags %u %u\\n", HD_LOG_SEL_VALUE, HD_LOG_SEL_FROM);')
    lines.append("return 0; }")
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", os.path.join(SC.ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = {}
    for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n"):
        if line:
            a, b, c = line.split()
            got[(a, b)] = int(c)
    for cname, py in structs.items():
        assert got[(cname, "size")] == ctypes.sizeof(py), cname
        for f, _ in py._fields_:
            assert got[(cname, f)] == getattr(py, f).offset, (cname, f)
    assert got[("flags", "1")] == 2


def test_filter_arguments_of_the_python_face():
    """DecideLog._filter without a library: the ranges, the masks and the 32-byte checks"""
    from hyperdrive_amd.verify import DecideLog
    f = DecideLog._filter(None, ("prevote", 3), None, None, None, 0, None, 0)
    assert (f.type_mask, f.round_lo, f.round_hi, f.flags) == (0b1100, SC.I64_MIN, SC.I64_MAX, 0)
    assert (f.pos_lo, f.pos_hi, f.limit, f.reserved) == (0, 0xFFFFFFFF, 0, 0)
    f = DecideLog._filter(None, 1, (2, 9), b"\x01" * 32, b"\x02" * 32, 4, 7, 5)
    assert (f.type_mask, f.round_lo, f.round_hi, f.flags, f.pos_lo, f.pos_hi, f.limit) == (2, 2, 9, 3, 4, 8, 5)
    assert bytes(f.value32) == b"\x01" * 32 and bytes(f.from32) == b"\x02" * 32
    assert DecideLog._filter(None, 2, -4, None, None, 0, -1, 0).pos_hi == 0
    for bad in (dict(types=4), dict(types="vote"), dict(types=2, value=b"x"), dict(types=2, sender=bytes(31)),
                dict(types=2, first=-1), dict(types=2, limit=-1)):
        a = dict(types=2, round=None, value=None, sender=None, first=0, upto=None, limit=0)
        a.update(bad)
        with pytest.raises(ValueError):
            DecideLog._filter(None, **a)


# ---- the kernel's predicate -------------------------------------------------------------
def test_filter_validation(prog):
    cases = [(m, f, r) for m in (0, 1, 2, 4, 8, 6, 12, 14, 15, 16, 0x10E, 0x80000000) for f in (0, 1, 2, 3, 4, 7)
             for r in (0, 1)]
    want = [m != 0 and m & ~0xE == 0 and f & ~3 == 0 and r == 0 for m, f, r in cases]
    assert SC.run_filter(prog, cases) == want and sum(want) == 6 * 4            # six masks x four flag sets


def test_match_against_the_model(prog, oracle):
    """log_match == the model's predicate, near misses included: a value or From that differs in its
    first or its last byte only, round - 1 and round + 1, the int64 extremes, a propose with a vote's
    value under a votes-only mask."""
    O = oracle
    v, a = O.canonical_value(H, 0), SC.sender(0)
    flip = lambda x, k: x[:k] + bytes([x[k] ^ 1]) + x[k + 1:]
    rng = random.Random(5)
    entries = [(t, r, val, frm) for t in (0, 1, 2, 3, 4, 31, 32, 33, 255)
               for r, val, frm in ((7, v, a), (6, v, a), (8, v, a))]
    entries += [(2, 7, val, frm) for val in (flip(v, 0), flip(v, 31), flip(v, 15), flip(v, 16), bytes(32))
                for frm in (a, flip(a, 0), flip(a, 31))]
    entries += [(3, r, v, a) for r in (SC.I64_MIN, SC.I64_MIN + 1, -1, 0, SC.I64_MAX - 1, SC.I64_MAX)]
    filters = []
    for mask in (2, 4, 8, 6, 12, 14):
        for fl in (0, 1, 2, 3):
            for rlo, rhi in ((7, 7), (6, 8), (8, 6), (SC.I64_MIN, SC.I64_MAX), (SC.I64_MAX, SC.I64_MAX),
                             (SC.I64_MIN, SC.I64_MIN), (SC.I64_MIN, -1), (0, SC.I64_MAX)):
                filters.append((mask, fl, rlo, rhi, v, a))
    cases = [(f, e) for f in filters for e in entries]
    rng.shuffle(cases)
    got = SC.run_match(prog, cases)
    hits = 0
    for ((mask, fl, rlo, rhi, fv, ff), (t, r, ev, ef)), g in zip(cases, got):
        row = bytes([t]) + SC.struct.pack("<qqq", H, r, -1) + ev + ef + bytes(65)
        types = [k for k in range(1, 4) if mask >> k & 1]
        want = SC.matches(row, types, rlo, rhi, fv if fl & 1 else None, ff if fl & 2 else None)
        assert g == want, (mask, fl, rlo, rhi, t, r)
        hits += want
    assert 100 < hits < len(cases) // 2
    # the named near misses, one by one
    vote_filter = (12, 3, 7, 7, v, a)
    named = [(2, 7, v, a), (2, 7, flip(v, 31), a), (2, 7, flip(v, 0), a), (2, 7, v, flip(a, 31)), (2, 7, v, flip(a, 0)),
             (2, 6, v, a), (2, 8, v, a), (1, 7, v, a)]
    assert SC.run_match(prog, [(vote_filter, e) for e in named]) == [True] + [False] * 7


# ---- the kernel's rank arithmetic -------------------------------------------------------
def _same_rank(prog, cases):
    got = SC.run_rank(prog, cases)
    for (flags, lo, hi, limit, cap), (pos, total, n) in zip(cases, got):
        want, wtotal = SC.select_flags(flags, lo, hi, limit)
        assert (total, n) == (wtotal, len(want)), (len(flags), lo, hi, limit, cap)
        assert pos == want[:cap], (len(flags), lo, hi, limit, cap)          # nothing at or beyond cap
    return got


@pytest.mark.parametrize("L", SC.SIZES)
def test_rank_over_the_patterns(prog, L):
    """every pattern of every size: whole log, room for all"""
    _same_rank(prog, [(f, 0, 0xFFFFFFFF, 0, L) for f in SC.patterns(L).values()]
               + [(f, 0, L, 0, L + 3) for f in SC.patterns(L).values()])


def test_rank_with_limits(prog):
    """limit inside a wavefront, at a wavefront boundary, at a block boundary, 1, >= total"""
    cases = []
    for L in (65, 257, 513, 1025):
        for name in ("every", "random", "every_64th"):
            f = SC.patterns(L)[name]
            total = sum(f)
            for limit in (1, 3, 63, 64, 65, 255, 256, 257, total - 1, total, total + 1, 0xFFFFFFFF):
                if limit > 0:
                    cases.append((f, 0, L, limit, L))
    got = _same_rank(prog, cases)
    assert len({t for _, t, _ in got}) > 4


def test_rank_with_position_ranges(prog):
    """pos_lo / pos_hi mid-wavefront and at block edges, pos_hi clipped, pos_lo >= L"""
    cases = []
    for L in (257, 1025):
        for name in ("every", "random"):
            f = SC.patterns(L)[name]
            for lo in (0, 1, 37, 63, 64, 255, 256, 257, L - 1, L, L + 1, 0xFFFFFFFF):
                for hi in (0, 38, 64, 256, 257, L - 1, L, L + 1, 0xFFFFFFFF):
                    for limit in (0, 5):
                        cases.append((f, lo, hi, limit, L))
    got = _same_rank(prog, cases)
    assert any(t == 0 for _, t, _ in got) and any(t > 256 for _, t, _ in got)


def test_rank_with_small_caps(prog):
    """cap below the matches: total and n name the need, the first cap slots are filled, no other"""
    cases = []
    for L in (64, 257, 1025):
        for name in ("every", "random"):
            f = SC.patterns(L)[name]
            for cap in (0, 1, 63, 64, 65, 256, sum(f) - 1, sum(f)):
                for limit in (0, 2, 300):
                    cases.append((f, 0, L, limit, max(cap, 0)))
    _same_rank(prog, cases)


def test_rank_past_256_blocks(prog):
    """65,536 + 300 positions: a block's offset sums more counts than the block has threads"""
    L = 65536 + 300
    rng = random.Random(3)
    sparse = [q % 2003 == 17 for q in range(L)]
    tail = [q >= L - 200 and q % 3 == 0 for q in range(L)]
    dense = [rng.random() < 0.5 for _ in range(L)]
    _same_rank(prog, [(sparse, 0, L, 0, L), (tail, 0, L, 3, 3), (tail, 65536, L + 9, 0, 100), (dense, 0, L, 0, L),
                      (dense, 255, L - 1, 40000, 40000), ([True] * L, 0, L, 0, L)])
