"""The yardstick of hd_log (include/hd_log.h) and a pure-Python model of the
retained log.

``Stream`` is the yardstick: it joins every batch inserted so far and runs
``when_cases.replay`` and ``propose_cases.restate`` over the concatenation
(messages of another height get a verdict that is not VALID), then states the
result in the joined coordinates of the call: a stream index becomes the log
position of a message kept by an earlier insert, or ``base + i`` for message i
of the current batch.

``Model`` is the design under test, restated in Python: it keeps the list of
kept messages and replays ``retained + batch`` at every insert, keeping the
messages ``restate`` marks as logged.  tests/test_log_host.py shows the two
agree on seeded streams, that every index the yardstick reports names a kept
message, and that the replay logs every retained entry again; nothing here
calls the library."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import hd_pyoracle as O
import propose_cases as PC
import when_cases as WC

NEVER = WC.NEVER
ROW_FIELDS = PC.ROW_FIELDS


@dataclass
class Expect:
    """One insert's outputs, as plain lists (joined coordinates)."""
    base: int
    kept: int
    rows: List[Dict[str, int]]          # propose_cases.ROW_FIELDS per row
    when: List[List[int]]
    exact_until: List[int]
    pclass: List[int]                   # this batch's messages
    dup: List[int]
    logpos: List[int]
    firings: List[Tuple[int, int, int, str]]
    new_firings: List[Tuple[int, int, int, str]]
    relogged: int


def masked(ob, verdicts, height: int) -> List[int]:
    """The verdicts with every message of another height made not VALID
    (process.go:759, 824, 861: the inserts reject another height first)."""
    return [v if ob.height[i] == height else O.BAD_RS for i, v in enumerate(verdicts)]


def _extend(dst, src) -> None:
    for i in range(len(src)):
        dst.append(src.mtype[i], src.height[i], src.round[i], src.valid_round[i], src.value[i], src.frm[i], src.sig[i])


def _decide(ob, verdicts, f, schedule, value_ok, index):
    """restate + replay over ob with every index passed through `index`."""
    want = PC.restate(ob, verdicts, f, schedule, value_ok)
    logs = WC.replay(ob, verdicts, f, schedule, value_ok)
    ix = lambda v, none: none if v == none else index(v)
    rows, when, until = [], [], []
    for x in want.rows:
        y = dict(x)
        y["rep"] = index(x["rep"])
        y["propose"] = ix(x["propose"], PC.NO_PROPOSE)
        rows.append(y)
        lg = logs[(x["height"], x["round"])]
        assert lg.first == x["rep"]
        when.append([ix(w, NEVER) for w in lg.when])
        until.append(ix(lg.exact_until, NEVER))
    assert len(logs) == len(rows)
    fir = [(index(i), h, r, k) for i, h, r, k in WC.firings(logs)]
    return want, rows, when, until, fir


class Stream:
    """The yardstick: one-shot decide over the concatenation."""

    def __init__(self, height: int, f: int, schedule=None):
        self.height, self.f, self.schedule = height, f, schedule
        self.ob = O.Batch()
        self.verdicts: List[int] = []
        self.value_ok: List[int] = []
        self.pos: Dict[int, int] = {}       # stream index -> log position
        self.entries = 0

    def peek(self, ob, verdicts, value_ok=None) -> Tuple[Expect, Dict[int, int]]:
        """What inserting (ob, verdicts, value_ok) must return, and the log
        positions it would add; the stream is unchanged."""
        s0, base, n = len(self.ob), self.entries, len(ob)
        full = O.Batch()
        _extend(full, self.ob)
        _extend(full, ob)
        fv = self.verdicts + masked(ob, verdicts, self.height)
        fok = self.value_ok + ([1] * n if value_ok is None else [1 if x else 0 for x in value_ok])
        add: Dict[int, int] = {}

        def index(i):                       # total where it is used: a KeyError is a finding
            return self.pos[i] if i < s0 else base + (i - s0)

        want, rows, when, until, fir = _decide(full, fv, self.f, self.schedule, fok, index)
        for i in range(s0, s0 + n):
            if want.dup[i] == 0 or want.pclass[i] == 0:
                add[i] = base + len(add)
        relogged = sum(1 for i in range(s0) if want.dup[i] == 0 or want.pclass[i] == 0)
        assert relogged == base and all((i in self.pos) == (want.dup[i] == 0 or want.pclass[i] == 0)
                                        for i in range(s0))
        exp = Expect(base, len(add), rows, when, until, want.pclass[s0:], want.dup[s0:],
                     [add.get(i, NEVER) for i in range(s0, s0 + n)], fir,
                     [(i - base, h, r, k) for i, h, r, k in fir if i >= base], relogged)
        return exp, add

    def push(self, ob, verdicts, value_ok=None) -> Expect:
        exp, add = self.peek(ob, verdicts, value_ok)
        n = len(ob)
        _extend(self.ob, ob)
        self.verdicts += masked(ob, verdicts, self.height)
        self.value_ok += [1] * n if value_ok is None else [1 if x else 0 for x in value_ok]
        self.pos.update(add)
        self.entries += len(add)
        return exp


class Model:
    """The retained log in Python: kept messages only, replayed at every insert."""

    def __init__(self, height: int, f: int, schedule=None):
        self.height, self.f, self.schedule = height, f, schedule
        self.kept = O.Batch()
        self.kept_ok: List[int] = []

    def insert(self, ob, verdicts, value_ok=None) -> Expect:
        base, n = len(self.kept), len(ob)
        joined = O.Batch()
        _extend(joined, self.kept)
        _extend(joined, ob)
        jv = [O.VALID] * base + masked(ob, verdicts, self.height)
        jok = self.kept_ok + ([1] * n if value_ok is None else [1 if x else 0 for x in value_ok])
        want, rows, when, until, fir = _decide(joined, jv, self.f, self.schedule, jok, lambda i: i)
        logged = lambda i: want.dup[i] == 0 or want.pclass[i] == 0
        relogged = sum(1 for i in range(base) if logged(i))
        logpos, k = [], 0
        for i in range(base, base + n):
            if logged(i):
                logpos.append(base + k)
                k += 1
                self.kept.append(joined.mtype[i], joined.height[i], joined.round[i], joined.valid_round[i],
                                 joined.value[i], joined.frm[i], joined.sig[i])
                self.kept_ok.append(jok[i])
            else:
                logpos.append(NEVER)
        return Expect(base, k, rows, when, until, want.pclass[base:], want.dup[base:], logpos, fir,
                      [(i - base, h, r, kk) for i, h, r, kk in fir if i >= base], relogged)


def cut(ob, verdicts, value_ok, lo: int, hi: int):
    """Messages lo..hi-1 as (oracle batch, verdicts, value_ok)."""
    part = O.Batch()
    for i in range(lo, hi):
        part.append(ob.mtype[i], ob.height[i], ob.round[i], ob.valid_round[i], ob.value[i], ob.frm[i], ob.sig[i])
    return part, verdicts[lo:hi], None if value_ok is None else value_ok[lo:hi]


def same_insert(res, exp: Expect) -> None:
    """res: a hyperdrive_amd LogInsertResult.  Everything, exactly."""
    assert (res.base, res.kept) == (exp.base, exp.kept), ((res.base, res.kept), (exp.base, exp.kept))
    assert res.relogged == res.base == exp.relogged
    assert len(res) == len(exp.rows), (len(res), len(exp.rows))
    for k in ROW_FIELDS:
        assert getattr(res, k).tolist() == [x[k] for x in exp.rows], k
    assert res.when.shape == (len(res), 8) and res.when.tolist() == exp.when
    assert res.exact_until.tolist() == exp.exact_until
    assert res.pclass.tolist() == exp.pclass
    assert res.dup.tolist() == exp.dup
    assert res.logpos.tolist() == exp.logpos
    assert res.firings == exp.firings
    assert res.new_firings == exp.new_firings
