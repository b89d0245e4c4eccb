"""The yardstick of the evidence rows (hd_evidence_out) and of hd_log_read
(include/hd_log.h): a Python model of exactly the host bookkeeping those calls
replace.

Before the log kept whole messages, a caller that wanted the two messages of a
catch record kept a second copy of the log on the host: a list of whole
messages indexed by log position, appended to after every insert from that
insert's ``logpos`` ("A height's logs across flushes").  ``Kept``
is that list.  It wraps a ``catch_cases.Stream`` -- the records and the insert's
other outputs come from there -- and turns every record into (offender row,
against row): ``against < base`` is looked up in the list, anything from ``base``
on is a message of the batch being inserted, and HD_WHEN_NEVER (an out-of-turn
propose) is a row of zero bytes.

A row is the whole message, 154 bytes: type, height, round, valid_round (little
endian int64), value, From, signature.  Every message of the cases here carries
65 signature bytes unique to it (``unique_sigs``), so a row gathered from the
wrong place cannot compare equal.  Nothing here calls the library;
tests/test_evidence_host.py pins the model against hand-worked batches."""
from __future__ import annotations

import struct
from typing import List, Sequence, Tuple

import catch_cases as CC
import hd_pyoracle as O

NEVER = CC.NEVER
ROW_BYTES = 1 + 8 + 8 + 8 + 32 + 32 + 65
ZERO_ROW = bytes(ROW_BYTES)


def sig_of(tag: bytes, k: int) -> bytes:
    """65 bytes that no other (tag, k) has."""
    s = tag + struct.pack(">I", k)
    return O.sha256(b"r" + s) + O.sha256(b"s" + s) + bytes([k % 4])


def unique_sigs(ob, tag: bytes = b"e"):
    """ob with message i signed sig_of(tag, i): the fields decide reads are unchanged."""
    out = O.Batch()
    for i in range(len(ob)):
        out.append(ob.mtype[i], ob.height[i], ob.round[i], ob.valid_round[i], ob.value[i], ob.frm[i], sig_of(tag, i))
    return out


def row(ob, i: int) -> bytes:
    """Message i of an oracle batch as its 154 bytes."""
    return (bytes([ob.mtype[i]]) + struct.pack("<qqq", ob.height[i], ob.round[i], ob.valid_round[i]) + ob.value[i]
            + ob.frm[i] + ob.sig[i])


def rows(b) -> List[bytes]:
    """The rows of a hyperdrive_amd Batch (a result's evidence_offender / evidence_against, DecideLog.read)."""
    out = []
    for i in range(len(b)):
        out.append(bytes([int(b.type[i])]) + struct.pack("<qqq", int(b.height[i]), int(b.round[i]),
                                                          int(b.valid_round[i]))
                   + b.value[i].tobytes() + b.frm[i].tobytes() + b.sig[i].tobytes())
    return out


Evidence = List[Tuple[bytes, bytes]]       # (offender row, against row) per record


class Kept:
    """The host copy of the log by position, and each insert's evidence from it."""

    def __init__(self, height: int, f: int, schedule=None):
        self.cs = CC.Stream(height, f, schedule)
        self.kept: List[bytes] = []        # whole messages by log position
        self.kept_ok: List[int] = []       # their value_ok bytes

    @property
    def entries(self) -> int:
        return len(self.kept)

    def peek(self, ob, verdicts) -> Tuple[List[CC.Record], Evidence]:
        """The records and evidence an insert of (ob, verdicts) must return; nothing moves."""
        base = len(self.kept)
        recs = self.cs.peek_caught(ob, verdicts)

        def message(q: int) -> bytes:
            if q == NEVER:
                return ZERO_ROW
            return self.kept[q] if q < base else row(ob, q - base)

        return recs, [(message(i), message(a)) for i, _, a in recs]

    def push(self, ob, verdicts, value_ok=None):
        """(log_cases.Expect, records, evidence) of this insert; the list grows by the insert's logpos."""
        recs, ev = self.peek(ob, verdicts)
        exp, recs2 = self.cs.push(ob, verdicts, value_ok)
        assert recs2 == recs
        for i, p in enumerate(exp.logpos):
            if p != NEVER:
                assert p == len(self.kept)             # positions are handed out in order
                self.kept.append(row(ob, i))
                self.kept_ok.append(1 if value_ok is None or value_ok[i] else 0)
        assert len(self.kept) == self.cs.entries
        return exp, recs, ev


def same_evidence(res, ev: Sequence[Tuple[bytes, bytes]]) -> None:
    """res: a result of an insert made with catch=True, evidence=True.  Every byte of every row."""
    got_o, got_a = rows(res.evidence_offender), rows(res.evidence_against)
    assert len(got_o) == len(got_a) == len(ev) == len(res.caught_index), (len(got_o), len(got_a), len(ev))
    for k, (o, a) in enumerate(ev):
        assert got_o[k] == o, ("offender", k)
        assert got_a[k] == a, ("against", k)
