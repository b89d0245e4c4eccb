"""A pure-Python restatement of the reference's propose log (insertPropose,
process/process.go:758-819) over a whole batch, and of the per-round rows
hd_decide returns (include/hd_verify.h).  It is the yardstick of
tests/test_gpu_decide.py; tests/test_decide_host.py pins it against
hand-worked cases of process_test.go's propose specs.

The vote side comes from ``oracle.tally`` (process.go:823-892) and the
predicates from ``oracle.decide_round``; nothing here calls the library."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import hd_pyoracle as O

NO_PROPOSE = 0xFFFFFFFF
ROW_FIELDS = ("height", "round", "rep", "propose", "prevotes", "precommits", "trace", "pv_value", "pc_value",
              "pv_nil", "pv_validround", "flags", "bits")
BIT_KEYS = ("timeout_prevote", "precommit_nil", "timeout_precommit_reached", "timeout_precommit_exact", "skip",
            "precommit_value", "commit", "prevote_validround")
U64 = 1 << 64


@dataclass
class Restated:
    rows: List[Dict[str, int]]                   # in the batch order of each round's first message
    decisions: Dict[Tuple[int, int], Dict[str, bool]]
    proposes: Dict[Tuple[int, int], int]         # (h, r) -> batch index of the logged propose
    pclass: List[int]
    dup: List[int]
    tally: "O.Tally"

    def row(self, h: int, r: int) -> Optional[Dict[str, int]]:
        for x in self.rows:
            if (x["height"], x["round"]) == (h, r):
                return x
        return None


def scheduled(schedule: Sequence[bytes], h: int, r: int) -> bytes:
    """scheduler/scheduler.go:52: signatories[(uint64(height) + uint64(round)) % n]."""
    return schedule[((h % U64) + (r % U64)) % U64 % len(schedule)]


def propose_equal(b, i: int, j: int) -> bool:
    """process/message.go:83-89 (the signature is not compared)."""
    return (b.height[i] == b.height[j] and b.round[i] == b.round[j] and b.valid_round[i] == b.valid_round[j]
            and b.value[i] == b.value[j] and b.frm[i] == b.frm[j])


def propose_log(b, verdicts, schedule=None):
    """insertPropose applied per height to every VALID propose in batch order:
    ({(h, r): logged index}, pclass)."""
    log: Dict[Tuple[int, int], int] = {}
    pclass = [3] * len(b)
    for i in range(len(b)):
        if b.mtype[i] != O.PROPOSE or verdicts[i] != O.VALID:
            continue
        h, r = b.height[i], b.round[i]
        if r <= O.INVALID_ROUND:                          # process.go:763
            continue
        if schedule is not None:                          # process.go:770
            if h <= 0:
                continue
            if scheduled(schedule, h, r) != b.frm[i]:     # process.go:771-780
                pclass[i] = 4
                continue
        if (h, r) in log:                                 # process.go:788-795
            pclass[i] = 1 if propose_equal(b, i, log[(h, r)]) else 2
            continue
        log[(h, r)] = i                                   # process.go:804, 811
        pclass[i] = 0
    return log, pclass


def restate(b, verdicts, f: int, schedule=None, value_ok=None) -> Restated:
    t = O.tally(b, verdicts)
    log, pclass = propose_log(b, verdicts, schedule)
    signers: Dict[Tuple[int, int], set] = {}      # TraceLogs[r] restricted to votes
    first: Dict[Tuple[int, int], int] = {}
    for i in range(len(b)):
        key = (b.height[i], b.round[i])
        if t.dup[i] == 0:
            signers.setdefault(key, set()).add(b.frm[i])
        if t.dup[i] != 3 or pclass[i] == 0:
            first.setdefault(key, i)
    rows, decisions = [], {}
    for key, rep in sorted(first.items(), key=lambda kv: kv[1]):
        h, r = key
        p = log.get(key)
        pvalue, pvalid, vr, new = None, False, O.INVALID_ROUND, False
        if p is not None:
            pvalue, vr = b.value[p], b.valid_round[p]
            pvalid = pvalue != O.NIL_VALUE and (value_ok is None or bool(value_ok[p]))   # process.go:803
            new = pvalid and b.frm[p] not in signers.get(key, set())                     # process.go:813-816
        d = O.decide_round(t, h, r, f, pvalue, pvalid, vr, new)
        decisions[key] = d
        cnt = lambda rr, ty: t.count.get((h, rr, ty, pvalue), 0) if p is not None else 0
        rows.append({
            "height": h, "round": r, "rep": rep, "propose": NO_PROPOSE if p is None else p,
            "prevotes": t.distinct.get((h, r, O.PREVOTE), 0), "precommits": t.distinct.get((h, r, O.PRECOMMIT), 0),
            "trace": len(signers.get(key, ())) + (1 if new else 0),                      # process.go:751
            "pv_value": cnt(r, O.PREVOTE), "pc_value": cnt(r, O.PRECOMMIT),
            "pv_nil": t.count.get((h, r, O.PREVOTE, O.NIL_VALUE), 0),
            "pv_validround": cnt(vr, O.PREVOTE) if vr > O.INVALID_ROUND else 0,
            "flags": (0 if p is None else 1) | (2 if pvalid else 0) | (4 if new else 0),
            "bits": sum(1 << k for k, name in enumerate(BIT_KEYS) if d[name]),
        })
    return Restated(rows, decisions, log, pclass, t.dup, t)


def same_as(res, want: Restated) -> None:
    """res: a hyperdrive_amd DecideResult.  Rows, order, bits, pclass and dup, all exact."""
    assert len(res) == len(want.rows), (len(res), len(want.rows))
    for k in ROW_FIELDS:
        assert getattr(res, k).tolist() == [x[k] for x in want.rows], k
    assert res.pclass.tolist() == want.pclass
    assert res.dup.tolist() == want.dup
    assert res.decisions == want.decisions
    assert res.proposes == want.proposes
