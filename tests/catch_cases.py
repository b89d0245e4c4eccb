"""The yardstick of the catch list (hd_catch_out, include/hd_verify.h): a
sequential replay that appends a record wherever the reference's Process calls
its Catcher.

The batch is walked once in order with two dicts, as the reference's inserts
keep them per height: the vote logs, keyed (h, r, type, From) -> the index of
the logged vote (PrevoteLogs / PrecommitLogs, process/process.go:824-843 and
861-880), and the propose log, keyed (h, r) -> the index of the logged propose
(ProposeLogs, process.go:759-795).  Nothing here calls the library, and nothing
comes from ``propose_cases.restate`` or ``oracle.tally``: tests/test_catch_host.py
compares this file with those on seeded mixes and pins it against hand-worked
batches.

``Stream`` states the records of one insert into an hd_log in the call's joined
coordinates, through the position map of the ``log_cases.Stream`` it wraps."""
from __future__ import annotations

import random
from typing import Dict, List, Sequence, Tuple

import hd_pyoracle as O
import log_cases as LC
import when_cases as WC

NEVER = 0xFFFFFFFF
DOUBLE_PREVOTE, DOUBLE_PRECOMMIT, DOUBLE_PROPOSE, OUT_OF_TURN = 1, 2, 3, 4
NAMES = {DOUBLE_PREVOTE: "double_prevote", DOUBLE_PRECOMMIT: "double_precommit", DOUBLE_PROPOSE: "double_propose",
         OUT_OF_TURN: "out_of_turn_propose"}
U64 = 1 << 64
H = 5

Record = Tuple[int, int, int]      # (index, kind, against)


def _proposer(schedule: Sequence[bytes], h: int, r: int) -> bytes:
    """scheduler/scheduler.go:52: signatories[(uint64(height) + uint64(round)) % n]."""
    return schedule[((h % U64) + (r % U64)) % U64 % len(schedule)]


def records(b, verdicts, schedule=None) -> List[Record]:
    """The Catcher calls of inserting b's VALID messages one at a time, each
    height into a Process at that height: (index, kind, against) in call order."""
    votes: Dict[Tuple[int, int, int, bytes], int] = {}
    proposes: Dict[Tuple[int, int], int] = {}
    out: List[Record] = []
    for i in range(len(b)):
        if verdicts[i] != O.VALID:
            continue
        t, h, r = b.mtype[i], b.height[i], b.round[i]
        if t in (O.PREVOTE, O.PRECOMMIT):
            key = (h, r, t, b.frm[i])
            if key in votes:                                   # process.go:831-843, 868-880
                e = votes[key]
                if b.value[i] != b.value[e]:                   # !Equal: the key's fields are the same already
                    out.append((i, DOUBLE_PREVOTE if t == O.PREVOTE else DOUBLE_PRECOMMIT, e))
                continue
            votes[key] = i                                     # 846, 883
        elif t == O.PROPOSE:
            if r <= O.INVALID_ROUND:                           # 763
                continue
            if schedule is not None:                           # 770
                if h <= 0:                                     # no Process runs at such a height: no candidate
                    continue
                if _proposer(schedule, h, r) != b.frm[i]:      # 771-779
                    out.append((i, OUT_OF_TURN, NEVER))
                    continue
            if (h, r) in proposes:                             # 788-794
                e = proposes[(h, r)]
                equal = (b.valid_round[i] == b.valid_round[e] and b.value[i] == b.value[e]
                         and b.frm[i] == b.frm[e])             # message.go:83-89, height and round being the key
                if not equal:
                    out.append((i, DOUBLE_PROPOSE, e))
                continue
            proposes[(h, r)] = i                               # 804, 811
    return out


def named(recs: Sequence[Record]) -> List[Tuple[int, str, int]]:
    """The records as a result's ``caught`` states them."""
    return [(i, NAMES[k], a) for i, k, a in recs]


def same_caught(res, recs: Sequence[Record]) -> None:
    """res: a result of a call made with catch=True.  The list, exactly."""
    assert res.caught_index.tolist() == [i for i, _, _ in recs]
    assert res.caught_kind.tolist() == [k for _, k, _ in recs]
    assert res.caught_against.tolist() == [a for _, _, a in recs]
    assert res.caught == named(recs)


class Stream:
    """A log_cases.Stream that also states each insert's catch list: the
    records of the whole stream so far whose offender is a message of the
    batch being inserted, in the insert's joined coordinates."""

    def __init__(self, height: int, f: int, schedule=None):
        self.ys = LC.Stream(height, f, schedule)

    @property
    def entries(self) -> int:
        return self.ys.entries

    def peek_caught(self, ob, verdicts) -> List[Record]:
        ys = self.ys
        s0, base = len(ys.ob), ys.entries
        full = O.Batch()
        LC._extend(full, ys.ob)
        LC._extend(full, ob)
        fv = ys.verdicts + LC.masked(ob, verdicts, ys.height)
        out = []
        for i, k, a in records(full, fv, ys.schedule):
            if i < s0:
                continue
            if a != NEVER:                                     # a logged message outside the map is a finding
                a = ys.pos[a] if a < s0 else base + (a - s0)
            out.append((base + (i - s0), k, a))
        return out

    def push(self, ob, verdicts, value_ok=None):
        """(log_cases.Expect, records) of this insert; the stream moves on."""
        recs = self.peek_caught(ob, verdicts)
        return self.ys.push(ob, verdicts, value_ok), recs


# ---- the seeded mixes of tests/test_catch_host.py and tests/test_gpu_catch.py ----------------
# each returns (signatories, schedule or None, oracle batch, verdicts, value_ok)
def mix_3000(with_schedule: bool):
    """The 3,000-message mix of tests/test_gpu_log.py's big_mix; without a
    schedule the mix is generated without one too."""
    sigs = [O.sha256(b"b" + bytes([k])) for k in range(40)]
    vals = [O.canonical_value(H, k) for k in range(3)] + [O.NIL_VALUE]
    sched = sigs if with_schedule else None
    ob, verdicts, value_ok = WC.mix(random.Random(42), 3000, [H], [0, 1, 2, 3], sigs, vals, 1 / 40, sched, p_bad=0.05)
    return sigs, sched, ob, verdicts, value_ok


def mix_40():
    """The stream of tests/test_gpu_log.py::test_every_cut_of_a_small_stream."""
    sigs = [O.sha256(b"a" + bytes([k])) for k in range(7)]
    vals = [O.canonical_value(H, k) for k in range(2)] + [O.NIL_VALUE]
    ob, verdicts, value_ok = WC.mix(random.Random(41), 40, [H], [-1, 0, 1, 2], sigs, vals, 1 / 8, sigs,
                                    valid_rounds=(-1, 0, 1, 2))
    return sigs, sigs, ob, verdicts, value_ok


def mix_5000():
    sigs = [O.sha256(b"j" + bytes([k])) for k in range(12)]
    vals = [O.canonical_value(H, k) for k in range(2)] + [O.NIL_VALUE]
    ob, verdicts, value_ok = WC.mix(random.Random(46), 5000, [H], [0, 1], sigs, vals, 1 / 8, sigs, p_bad=0.02)
    return sigs, sigs, ob, verdicts, value_ok
