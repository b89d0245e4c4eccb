"""Host-side mirror of the batch-verify boundary.

In the reference the authentication of a Propose/Prevote/Precommit is a
precondition the caller must establish before ``Replica.Propose/Prevote/
Precommit`` (replica/replica.go:153-181; mq/mq.go:85-101 "assumes that the
sender has already been authenticated"), and membership is the
``procsAllowed`` filter at consume time (mq/mq.go:49-51).  This module is the
Python face of the C ABI that takes over both for a whole batch:

    v = Verifier(device=0)
    v.set_signatories(signatories)          # replica.go:69-72 / 136-144
    res = v.verify_batch(batch)             # per-message verdicts
    t = v.tally(batch, res.verdict)         # first-wins logs + 2f+1 counts

Per-message failures are verdicts (never exceptions); exceptions are raised
only for invalid arguments and device failures, like the reference's
``fmt.Errorf`` returns in process/message.go:61-77.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from ._lib import HDError, HdBatch, HdTallyOut

# verdicts (include/hd_verify.h)
VALID = 0
BAD_RECID = 1
BAD_RS = 2
NO_POINT = 3
INFINITY = 4
SIGNATORY_MISMATCH = 5
NOT_ADMITTED = 6
BAD_TYPE = 7
NOT_AUTHENTIC = 8     # authenticate_batch_device only (include/hd_verify.h)
VERDICT_NAMES = ["VALID", "BAD_RECID", "BAD_RS", "NO_POINT", "INFINITY", "SIGNATORY_MISMATCH",
                 "NOT_ADMITTED", "BAD_TYPE", "NOT_AUTHENTIC"]

PROPOSE, PREVOTE, PRECOMMIT = 1, 2, 3

# statuses of import_keys (include/hd_verify.h HD_KEY_*)
KEY_IMPORTED, KEY_KNOWN, KEY_NOT_ADMITTED, KEY_NO_SLOT, KEY_BAD_POINT = 0, 1, 2, 3, 4


def _ptr(a: Optional[np.ndarray]):
    if a is None:
        return None
    assert a.flags["C_CONTIGUOUS"], "arrays must be C-contiguous"
    return a.ctypes.data


def set_change_info(lib, ctx, check) -> dict:
    """hd_ctx_set_change_info of a context handle, as a dict of its fields"""
    info = _lib.HdSetChangeInfo()
    check(lib.hd_ctx_set_change_info(ctx, ctypes.byref(info)), "hd_ctx_set_change_info")
    return {name: int(getattr(info, name)) for name, _ in info._fields_}


@dataclass
class Batch:
    """Structure-of-arrays batch in host memory (hd_batch)."""
    type: np.ndarray          # uint8[n]
    height: np.ndarray        # int64[n]
    round: np.ndarray         # int64[n]
    valid_round: Optional[np.ndarray]  # int64[n] or None
    value: np.ndarray         # uint8[n, 32]
    frm: np.ndarray           # uint8[n, 32]
    sig: np.ndarray           # uint8[n, 65]

    def __post_init__(self):
        n = len(self.type)
        self.type = np.ascontiguousarray(self.type, dtype=np.uint8)
        self.height = np.ascontiguousarray(self.height, dtype=np.int64)
        self.round = np.ascontiguousarray(self.round, dtype=np.int64)
        if self.valid_round is not None:
            self.valid_round = np.ascontiguousarray(self.valid_round, dtype=np.int64)
        self.value = np.ascontiguousarray(self.value, dtype=np.uint8).reshape(n, 32)
        self.frm = np.ascontiguousarray(self.frm, dtype=np.uint8).reshape(n, 32)
        self.sig = np.ascontiguousarray(self.sig, dtype=np.uint8).reshape(n, 65)
        for name in ("height", "round"):
            if len(getattr(self, name)) != n:
                raise ValueError(f"{name} has {len(getattr(self, name))} entries, expected {n}")
        if self.valid_round is not None and len(self.valid_round) != n:
            raise ValueError("valid_round length mismatch")

    def __len__(self) -> int:
        return len(self.type)

    @classmethod
    def _wrap(cls, mtype, height, round_, valid_round, value, frm, sig) -> "Batch":
        """Fields the library just wrote (contiguous, right dtypes and shapes):
        no conversion pass (the per-flush result of the mq consume)."""
        b = object.__new__(cls)
        b.type, b.height, b.round, b.valid_round, b.value, b.frm, b.sig = (mtype, height, round_, valid_round, value,
                                                                           frm, sig)
        return b

    @classmethod
    def from_lists(cls, mtype, height, round_, valid_round, value, frm, sig) -> "Batch":
        n = len(mtype)
        return cls(np.array(mtype, np.uint8), np.array(height, np.int64), np.array(round_, np.int64),
                   np.array(valid_round, np.int64) if valid_round is not None else None,
                   np.frombuffer(b"".join(value), np.uint8).reshape(n, 32).copy() if n else np.zeros((0, 32), np.uint8),
                   np.frombuffer(b"".join(frm), np.uint8).reshape(n, 32).copy() if n else np.zeros((0, 32), np.uint8),
                   np.frombuffer(b"".join(sig), np.uint8).reshape(n, 65).copy() if n else np.zeros((0, 65), np.uint8))

    def c_struct(self) -> HdBatch:
        return HdBatch(len(self), _ptr(self.type), _ptr(self.height), _ptr(self.round), _ptr(self.valid_round),
                       _ptr(self.value), _ptr(self.frm), _ptr(self.sig))


@dataclass
class CompactBatch:
    """The PCIe-lean host batch (hd_batch_compact): From and value as 16-bit
    indices into the signatory array of the context (then escape rows) and
    into a per-batch value dictionary."""
    type: np.ndarray          # uint8[n]
    height: np.ndarray        # int64[n]
    round: np.ndarray         # int64[n]
    valid_round: Optional[np.ndarray]
    from_idx: np.ndarray      # uint16[n]
    value_idx: np.ndarray     # uint16[n]
    sig: np.ndarray           # uint8[n, 65]
    escape: np.ndarray        # uint8[n_escape, 32]
    values: np.ndarray        # uint8[n_values, 32]

    def __len__(self):
        return len(self.type)

    @staticmethod
    def from_batch(b: "Batch", signatories) -> "CompactBatch":
        """Index form of a Batch against the signatory array the context was
        given (the first row of a repeated signatory is used; Froms outside
        it become escape rows, values the batch's dictionary)."""
        sig = np.ascontiguousarray(_as_rows(signatories, 32))
        n, ns = len(b), len(sig)
        key = lambda rows: rows.view(np.dtype((np.void, 32))).ravel()
        skeys = key(sig)
        order = np.argsort(skeys, kind="stable")
        fk = key(b.frm)
        pos = np.searchsorted(skeys[order], fk)
        pos = np.minimum(pos, max(ns - 1, 0))
        hit = (skeys[order][pos] == fk) if ns else np.zeros(n, bool)
        from_idx = np.zeros(n, np.int64)
        from_idx[hit] = order[pos[hit]]
        esc_rows, esc_inv = np.unique(fk[~hit], return_inverse=True)
        from_idx[~hit] = ns + esc_inv.ravel()
        vals, vinv = np.unique(key(b.value), return_inverse=True)
        if ns + len(esc_rows) > 65536 or len(vals) > 65536:
            raise ValueError("more than 65536 From rows or values: split the batch")
        return CompactBatch(b.type, b.height, b.round, b.valid_round, from_idx.astype(np.uint16),
                            vinv.ravel().astype(np.uint16), b.sig,
                            np.frombuffer(esc_rows.tobytes(), np.uint8).reshape(-1, 32).copy(),
                            np.frombuffer(vals.tobytes(), np.uint8).reshape(-1, 32).copy())

    def c_struct(self):
        from ._lib import HdBatchCompact
        return HdBatchCompact(len(self), _ptr(self.type), _ptr(self.height), _ptr(self.round), _ptr(self.valid_round),
                              _ptr(self.from_idx), _ptr(self.value_idx), _ptr(self.sig), len(self.escape),
                              _ptr(self.escape) if len(self.escape) else None, len(self.values), _ptr(self.values))


@dataclass
class VerifyResult:
    verdict: np.ndarray       # uint8[n]
    recovered: np.ndarray     # uint8[n, 32]
    valid_bitmap: np.ndarray  # uint32[ceil(n/32)]


@dataclass
class TallyResult:
    """First-wins vote logs summarised per (h, r) and per (h, r, type, value)."""
    count: Dict[Tuple[int, int, int, bytes], int]
    distinct: Dict[Tuple[int, int, int], int]
    distinct_any: Dict[Tuple[int, int], int]
    dup: np.ndarray           # uint8[n]: 0 logged, 1 identical dup, 2 double vote, 3 not a candidate


DECISION_KEYS = ("timeout_prevote", "precommit_nil", "timeout_precommit_reached", "timeout_precommit_exact", "skip",
                 "precommit_value", "commit", "prevote_validround")   # bit order of hd_decide_out.bits
NO_PROPOSE = 0xFFFFFFFF


@dataclass
class DecideResult:
    """One row per (h, r) of a batch (hd_decide_out): the log lengths, the
    logged propose, the counts for its value and the eight predicate bits,
    computed on the device.  Rows are in the batch order of each round's first
    vote candidate or logged propose."""
    height: np.ndarray         # int64[rows]
    round: np.ndarray          # int64[rows]
    rep: np.ndarray            # uint32[rows]
    propose: np.ndarray        # uint32[rows], NO_PROPOSE without a logged propose
    prevotes: np.ndarray
    precommits: np.ndarray
    trace: np.ndarray
    pv_value: np.ndarray
    pc_value: np.ndarray
    pv_nil: np.ndarray
    pv_validround: np.ndarray
    flags: np.ndarray          # uint8[rows]: 1 propose logged, 2 it is valid, 4 its signer was new to the trace
    bits: np.ndarray           # uint8[rows]: DECISION_KEYS, bit k = key k
    pclass: np.ndarray         # uint8[n]: 0 logged, 1 equal copy, 2 double propose, 3 no candidate, 4 out of turn
    dup: np.ndarray            # uint8[n]: as TallyResult.dup

    def __len__(self) -> int:
        return len(self.height)

    @property
    def decisions(self) -> Dict[Tuple[int, int], Dict[str, bool]]:
        """{(h, r): the dict quorum.decide returns}."""
        return {(int(h), int(r)): {k: bool((int(b) >> j) & 1) for j, k in enumerate(DECISION_KEYS)}
                for h, r, b in zip(self.height, self.round, self.bits)}

    @property
    def proposes(self) -> Dict[Tuple[int, int], int]:
        """{(h, r): batch index of the logged propose}."""
        return {(int(h), int(r)): int(p) for h, r, p in zip(self.height, self.round, self.propose)
                if int(p) != NO_PROPOSE}


WHEN_NEVER = 0xFFFFFFFF


@dataclass
class OrderedDecideResult(DecideResult):
    """A DecideResult plus, per row and predicate, the batch index at which the
    predicate first holds when the batch is inserted one message at a time
    (hd_decide_order, include/hd_verify.h)."""
    when: np.ndarray = None          # uint32[rows, 8], WHEN_NEVER where the predicate never holds
    exact_until: np.ndarray = None   # uint32[rows]: timeout_precommit_exact holds on [when[:, 3], exact_until)

    @property
    def firings(self) -> List[Tuple[int, int, int, str]]:
        """(batch index, height, round, DECISION_KEYS name) of every predicate
        that ever holds, sorted by batch index, then bit: the order in which
        to feed the automaton."""
        rows, ks = np.nonzero(self.when != WHEN_NEVER)
        out = [(int(self.when[j, k]), int(k), int(self.height[j]), int(self.round[j])) for j, k in zip(rows, ks)]
        out.sort(key=lambda x: (x[0], x[1]))
        return [(i, h, r, DECISION_KEYS[k]) for i, k, h, r in out]


@dataclass
class LogInsertResult(OrderedDecideResult):
    """One :meth:`DecideLog.insert`: the OrderedDecideResult of the whole
    stream so far, in joined coordinates -- an index below ``base`` is a log
    position (an earlier insert's ``logpos``), an index at or above it is
    message ``index - base`` of this batch.  pclass / dup / logpos have one
    entry per message of this batch."""
    base: int = 0                    # entries before this insert
    kept: int = 0                    # entries this insert added
    logpos: np.ndarray = None        # uint32[n]: the message's log position, WHEN_NEVER when it was not kept
    relogged: int = 0                # retained entries the replay logged again: always == base

    @property
    def new_firings(self) -> List[Tuple[int, int, int, str]]:
        """The firings of this insert: (index into this batch, height, round,
        name) of every predicate that first held at one of its messages."""
        return [(i - self.base, h, r, k) for i, h, r, k in self.firings if i >= self.base]


# kinds of a catch record (include/hd_verify.h HD_CATCH_*)
CATCH_NAMES = {1: "double_prevote", 2: "double_precommit", 3: "double_propose", 4: "out_of_turn_propose"}


class _Caught:
    """The catch list of a decide or insert made with ``catch=True``
    (hd_catch_out): one record per double vote, double propose and out-of-turn
    propose, in ascending index."""

    @property
    def caught(self) -> List[Tuple[int, str, int]]:
        """(index, name, against): the offender, the CATCH_NAMES name of its
        kind and the logged message it contradicts (WHEN_NEVER for an
        out-of-turn propose): the arguments of the reference's Catcher calls,
        in the order of those calls."""
        return [(int(i), CATCH_NAMES[int(k)], int(a))
                for i, k, a in zip(self.caught_index, self.caught_kind, self.caught_against)]


@dataclass
class CaughtDecideResult(DecideResult, _Caught):
    caught_index: np.ndarray = None      # uint32[records], ascending
    caught_against: np.ndarray = None    # uint32[records]
    caught_kind: np.ndarray = None       # uint8[records]


@dataclass
class CaughtOrderedDecideResult(OrderedDecideResult, _Caught):
    caught_index: np.ndarray = None
    caught_against: np.ndarray = None
    caught_kind: np.ndarray = None


@dataclass
class CaughtLogInsertResult(LogInsertResult, _Caught):
    """index and against are joined coordinates, as every index of a
    LogInsertResult: index - base is the message of this batch; against below
    base is a log position."""
    caught_index: np.ndarray = None
    caught_against: np.ndarray = None
    caught_kind: np.ndarray = None


@dataclass
class EvidenceLogInsertResult(CaughtLogInsertResult):
    """A CaughtLogInsertResult with the whole messages of every record
    (hd_evidence_out): row k of ``evidence_offender`` and row k of
    ``evidence_against`` are the two messages of ``caught[k]``, as the
    reference's Catcher takes them.  The against row of an out-of-turn propose
    is all zero bytes.  On a log that keeps no signatures both ``sig`` arrays
    are zero."""
    evidence_offender: Batch = None
    evidence_against: Batch = None
    evidence_offender_value_ok: np.ndarray = None   # uint8[records]
    evidence_against_value_ok: np.ndarray = None


def _rows_struct(n: int, sig: bool):
    """An hd_log_rows with room for n rows, and its arrays."""
    from ._lib import HdLogRows
    m = max(n, 1)
    a = {"type": np.zeros(m, np.uint8), "height": np.zeros(m, np.int64), "round": np.zeros(m, np.int64),
         "valid_round": np.zeros(m, np.int64), "value32": np.zeros((m, 32), np.uint8),
         "from32": np.zeros((m, 32), np.uint8), "value_ok": np.zeros(m, np.uint8), "sig65": np.zeros((m, 65), np.uint8)}
    r = HdLogRows(n, 0, _ptr(a["type"]), _ptr(a["height"]), _ptr(a["round"]), _ptr(a["valid_round"]),
                  _ptr(a["value32"]), _ptr(a["from32"]), _ptr(a["value_ok"]), _ptr(a["sig65"]) if sig else None)
    return r, a


def _rows_batch(n: int, a) -> Tuple[Batch, np.ndarray]:
    """The first n rows of _rows_struct's arrays as (Batch, value_ok)."""
    return (Batch._wrap(a["type"][:n].copy(), a["height"][:n].copy(), a["round"][:n].copy(),
                        a["valid_round"][:n].copy(), a["value32"][:n].copy(), a["from32"][:n].copy(),
                        a["sig65"][:n].copy()), a["value_ok"][:n].copy())


def _catch_struct(n: int):
    """An hd_catch_out with room for every message of a batch of n."""
    from ._lib import HdCatchOut
    arrs = {"index": np.zeros(max(n, 1), np.uint32), "against": np.zeros(max(n, 1), np.uint32),
            "kind": np.zeros(max(n, 1), np.uint8)}
    c = HdCatchOut(n, 0, _ptr(arrs["index"]), _ptr(arrs["against"]), _ptr(arrs["kind"]))
    return c, arrs


def _caught_fields(c, arrs) -> Dict[str, np.ndarray]:
    return {"caught_" + k: arrs[k][: c.n].copy() for k in ("index", "against", "kind")}


class _DeviceBytes:
    """n bytes at a device address, where insert_device takes a tensor."""
    __slots__ = ("ptr", "n")

    def __init__(self, ptr: int, n: int):
        self.ptr, self.n = ptr, n

    def data_ptr(self) -> int:
        return self.ptr

    def numel(self) -> int:
        return self.n


class DecideLog:
    """A height's vote and propose logs kept on the device across inserts
    (include/hd_log.h): every insert returns what decide_ordered would return
    for all the batches inserted since the last reset, joined."""

    def __init__(self, v: "Verifier", height: int, f: int, schedule=None, max_entries: int = 0,
                 keep_signatures: bool = False):
        self._v = v
        self._lib = v._lib
        h = ctypes.c_void_p()
        v._check(self._lib.hd_log_create(v.handle, ctypes.byref(h)), "hd_log_create")
        self._log = h
        self._close_rank = 0          # closed before its Verifier
        _lib.track(self)
        self.max_entries = int(max_entries)
        self.f = int(f)
        self._sched = None
        self._rows = 0                # rows of the last insert: the next has at most this many more than its batch
        self._sel_cap = 256           # rows a select without a limit brings room for; HD_ECAP names the need
        self.keep_signatures = bool(keep_signatures)
        if keep_signatures:
            v._check(self._lib.hd_log_keep_signatures(h, 1), "hd_log_keep_signatures")
        self.reset(height, f, schedule)

    def close(self):
        if getattr(self, "_log", None):
            self._lib.hd_log_destroy(self._log)
            self._log = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def handle(self):
        return self._log

    def reset(self, height: int, f: Optional[int] = None, schedule=None) -> None:
        """Empties the log and sets its height; f and schedule: None keeps the
        current one."""
        if f is not None:
            self.f = int(f)
        if schedule is not None:
            sched = _as_rows(schedule, 32)
            if len(sched) == 0:
                raise ValueError("an empty schedule (pass None for no turn check)")
            self._sched = sched
        s = self._sched
        self._v._check(self._lib.hd_log_reset(self._log, int(height), self.f, _ptr(s), len(s) if s is not None else 0,
                                              self.max_entries), "hd_log_reset")
        self._rows = 0

    def _len(self) -> Tuple[int, int]:
        h, e = ctypes.c_int64(), ctypes.c_uint32()
        self._v._check(self._lib.hd_log_len(self._log, ctypes.byref(h), ctypes.byref(e)), "hd_log_len")
        return h.value, e.value

    @property
    def height(self) -> int:
        return self._len()[0]

    @property
    def entries(self) -> int:
        return self._len()[1]

    def _outputs(self, n: int):
        from ._lib import HdLogInfo
        cap = self._rows + n
        o, a = Verifier._decide_struct(n, cap)
        w, when, until = Verifier._order_struct(cap)
        logpos = np.full(max(n, 1), WHEN_NEVER, np.uint32)
        info = HdLogInfo(0, 0, 0, _ptr(logpos))
        return o, a, w, when, until, logpos, info

    def _result(self, n, o, a, when, until, logpos, info, caught=None, evidence=None) -> LogInsertResult:
        self._rows = o.n
        rows = {k: a[k][: o.n].copy() for k in type(o).ROW_FIELDS}
        cls, extra = (CaughtLogInsertResult, _caught_fields(*caught)) if caught else (LogInsertResult, {})
        if evidence:
            ev, oa, aa = evidence
            cls = EvidenceLogInsertResult
            extra["evidence_offender"], extra["evidence_offender_value_ok"] = _rows_batch(ev.offender.n, oa)
            extra["evidence_against"], extra["evidence_against_value_ok"] = _rows_batch(ev.against.n, aa)
        return cls(pclass=a["pclass"][:n].copy(), dup=a["dup"][:n].copy(), when=when[: o.n].copy(),
                   exact_until=until[: o.n].copy(), base=info.base, kept=info.kept,
                   logpos=logpos[:n].copy(), relogged=info.relogged, **rows, **extra)

    def _evidence_struct(self, n: int):
        from ._lib import HdEvidenceOut
        off, oa = _rows_struct(n, self.keep_signatures)
        ag, aa = _rows_struct(n, self.keep_signatures)
        return HdEvidenceOut(off, ag), oa, aa

    def read(self, positions=None, first: int = 0, n: Optional[int] = None) -> Tuple[Batch, np.ndarray]:
        """hd_log_read: the entries ``positions`` (any order, repeats allowed),
        or entries first .. first + n - 1 (n None: to the log's end), as
        (Batch, value_ok bytes).  The signatures are read on a log that keeps
        them and are zero otherwise."""
        pos = None
        if positions is not None:
            pos = np.ascontiguousarray(positions, dtype=np.uint32)
            n = len(pos)
        elif n is None:
            n = max(self.entries - first, 0)
        r, a = _rows_struct(n, self.keep_signatures)
        self._v._check(self._lib.hd_log_read(self._log, _ptr(pos), int(first), n, ctypes.byref(r)), "hd_log_read")
        return _rows_batch(r.n, a)

    def insert(self, batch: Batch, verdict: np.ndarray, value_ok=None, catch: bool = False,
               evidence: bool = False) -> LogInsertResult:
        """hd_log_insert of a host batch with its verdicts (and value_ok, one
        byte per message, as :meth:`Verifier.decide`).  catch: also return the
        catch list of this batch (a CaughtLogInsertResult; hd_log_insert_catch).
        evidence (with catch): also both whole messages of every record (an
        EvidenceLogInsertResult; hd_log_insert_evidence)."""
        if evidence and not catch:
            raise ValueError("evidence=True needs catch=True")
        n = len(batch)
        verdict = np.ascontiguousarray(verdict, dtype=np.uint8)
        if len(verdict) != n:
            raise ValueError("verdict length mismatch")
        vok = np.ascontiguousarray(value_ok, dtype=np.uint8) if value_ok is not None else None
        if vok is not None and len(vok) != n:
            raise ValueError("value_ok length mismatch")
        o, a, w, when, until, logpos, info = self._outputs(n)
        cb = batch.c_struct()
        if evidence:
            c, ca = _catch_struct(n)
            ev, oa, aa = self._evidence_struct(n)
            self._v._check(self._lib.hd_log_insert_evidence(self._log, ctypes.byref(cb), _ptr(verdict), _ptr(vok),
                                                            ctypes.byref(o), ctypes.byref(w), ctypes.byref(info),
                                                            ctypes.byref(c), ctypes.byref(ev)),
                           "hd_log_insert_evidence")
            return self._result(n, o, a, when, until, logpos, info, (c, ca), (ev, oa, aa))
        if catch:
            c, ca = _catch_struct(n)
            self._v._check(self._lib.hd_log_insert_catch(self._log, ctypes.byref(cb), _ptr(verdict), _ptr(vok),
                                                         ctypes.byref(o), ctypes.byref(w), ctypes.byref(info),
                                                         ctypes.byref(c)), "hd_log_insert_catch")
            return self._result(n, o, a, when, until, logpos, info, (c, ca))
        self._v._check(self._lib.hd_log_insert(self._log, ctypes.byref(cb), _ptr(verdict), _ptr(vok), ctypes.byref(o),
                                               ctypes.byref(w), ctypes.byref(info)), "hd_log_insert")
        return self._result(n, o, a, when, until, logpos, info)

    def insert_device(self, dbatch: HdBatch, d_bitmap: int, value_ok=None, stream: Optional[int] = None,
                      catch: bool = False, evidence: bool = False) -> LogInsertResult:
        """hd_log_insert_device_bitmap over a device batch and the valid bitmap
        of verify_batch_device (bit i is message i of `dbatch`).  value_ok: a
        torch uint8 tensor on the device, the device address of n bytes (an
        int: mq.Taken.d_value_ok), or a host array, which is uploaded first.
        catch, evidence: as :meth:`insert`."""
        import torch
        if evidence and not catch:
            raise ValueError("evidence=True needs catch=True")
        n = dbatch.n
        vok = value_ok
        if isinstance(vok, int):
            vok = _DeviceBytes(vok, n)
        if vok is not None and not isinstance(vok, (torch.Tensor, _DeviceBytes)):
            vok = torch.from_numpy(np.ascontiguousarray(vok, dtype=np.uint8)).cuda()
            torch.cuda.current_stream().synchronize()
        if vok is not None and vok.numel() != n:
            raise ValueError("value_ok length mismatch")
        o, a, w, when, until, logpos, info = self._outputs(n)
        if evidence:
            c, ca = _catch_struct(n)
            ev, oa, aa = self._evidence_struct(n)
            self._v._check(self._lib.hd_log_insert_evidence_device_bitmap(
                self._log, ctypes.byref(dbatch), d_bitmap, vok.data_ptr() if vok is not None else None,
                ctypes.byref(o), ctypes.byref(w), ctypes.byref(info), ctypes.byref(c), ctypes.byref(ev), stream),
                "hd_log_insert_evidence_device_bitmap")
            return self._result(n, o, a, when, until, logpos, info, (c, ca), (ev, oa, aa))
        if catch:
            c, ca = _catch_struct(n)
            self._v._check(self._lib.hd_log_insert_catch_device_bitmap(
                self._log, ctypes.byref(dbatch), d_bitmap, vok.data_ptr() if vok is not None else None,
                ctypes.byref(o), ctypes.byref(w), ctypes.byref(info), ctypes.byref(c), stream),
                "hd_log_insert_catch_device_bitmap")
            return self._result(n, o, a, when, until, logpos, info, (c, ca))
        self._v._check(self._lib.hd_log_insert_device_bitmap(self._log, ctypes.byref(dbatch), d_bitmap,
                                                             vok.data_ptr() if vok is not None else None,
                                                             ctypes.byref(o), ctypes.byref(w), ctypes.byref(info),
                                                             stream), "hd_log_insert_device_bitmap")
        return self._result(n, o, a, when, until, logpos, info)

    # ---- keyed reads (hd_log_select) ---------------------------------------
    def _filter(self, types, round, value, sender, first, upto, limit):
        from ._lib import HD_LOG_SEL_FROM, HD_LOG_SEL_VALUE, HdLogFilter
        f = HdLogFilter()
        f.type_mask = _type_mask(types)
        if round is None:
            f.round_lo, f.round_hi = -(1 << 63), (1 << 63) - 1
        elif isinstance(round, (tuple, list)):
            f.round_lo, f.round_hi = int(round[0]), int(round[1])
        else:
            f.round_lo = f.round_hi = int(round)
        for name, flag, v in (("value32", HD_LOG_SEL_VALUE, value), ("from32", HD_LOG_SEL_FROM, sender)):
            if v is not None:
                raw = bytes(v) if not isinstance(v, np.ndarray) else v.tobytes()
                if len(raw) != 32:
                    raise ValueError(f"{name} needs 32 bytes")
                f.flags |= flag
                ctypes.memmove(getattr(f, name), raw, 32)
        if first < 0 or limit < 0 or (upto is not None and upto < -1):
            raise ValueError("first, upto and limit are log positions and a count")
        f.pos_lo = int(first)
        f.pos_hi = 0xFFFFFFFF if upto is None else min(int(upto) + 1, 0xFFFFFFFF)
        f.limit = int(limit)
        return f

    def select(self, types, round=None, value=None, sender=None, first: int = 0, upto: Optional[int] = None,
               limit: int = 0, rows: bool = True) -> "LogSelection":
        """hd_log_select: the logged entries of ``types`` (PROPOSE / PREVOTE /
        PRECOMMIT, their names, or several of them) in arrival order, narrowed
        by ``round`` (r, or (lo, hi) inclusive), ``value`` and ``sender`` (32
        bytes each) and to the log positions ``first`` .. ``upto``, both
        inclusive (upto None: to the log's end).  ``limit`` = k returns the
        first k matches; ``total`` counts them all either way.  rows=False
        returns the positions alone."""
        from ._lib import HD_ECAP, HdLogSelected
        f = self._filter(types, round, value, sender, first, upto, limit)
        sel = HdLogSelected()
        cap = int(limit) if limit else self._sel_cap
        while True:
            pos = np.zeros(max(cap, 1), np.uint32)
            r, a = _rows_struct(cap, self.keep_signatures) if rows else (None, None)
            rc = self._lib.hd_log_select(self._log, ctypes.byref(f), _ptr(pos), cap,
                                         ctypes.byref(r) if rows else None, ctypes.byref(sel))
            if rc != HD_ECAP or sel.n <= cap:
                break
            cap = sel.n                                    # the need: the same call with room succeeds
        self._v._check(rc, "hd_log_select")
        if not limit:
            self._sel_cap = max(256, sel.n + sel.n // 4)
        batch, ok = _rows_batch(sel.n, a) if rows else (None, None)
        return LogSelection(pos[: sel.n].copy(), int(sel.total), batch, ok)

    def count(self, types, round=None, value=None, sender=None, first: int = 0, upto: Optional[int] = None) -> int:
        """The count-only form of :meth:`select`: how many entries match.
        Nothing but the counts comes down."""
        from ._lib import HdLogSelected
        f = self._filter(types, round, value, sender, first, upto, 0)
        sel = HdLogSelected()
        self._v._check(self._lib.hd_log_select(self._log, ctypes.byref(f), None, 0, None, ctypes.byref(sel)),
                       "hd_log_select")
        return int(sel.total)

    def select_device(self, types, round=None, value=None, sender=None, first: int = 0, upto: Optional[int] = None,
                      limit: int = 0, cap: Optional[int] = None, stream=None) -> "DeviceSelection":
        """hd_log_select_device: the same selection left on the device as a
        DeviceBatch (signatures on a log that keeps them, zero otherwise) with
        its value_ok bytes and log positions, ready for codec.marshal_device,
        verify_batch_device and the *_device calls.  ``cap``: rows to allocate
        (default: ``limit``, or the count of a count-only call made first).
        ``stream``: a torch stream (default: the work stream)."""
        import torch
        from ._lib import HdLogSelected
        from .device import DeviceBatch, work_stream
        f = self._filter(types, round, value, sender, first, upto, limit)
        if cap is None:
            cap = int(limit) if limit else self.count(types, round, value, sender, first, upto)
        ws = stream or work_stream()
        with torch.cuda.stream(ws):
            db = DeviceBatch.empty(cap)
            if not self.keep_signatures:
                db.sig.zero_()
            vok = torch.empty(cap, dtype=torch.uint8, device="cuda")
            pos = torch.empty(cap, dtype=torch.int32, device="cuda")
        co = db.c_out()
        if not self.keep_signatures:
            co.sig65 = None
        co.adv_class = None
        sel = HdLogSelected()
        self._v._check(self._lib.hd_log_select_device(self._log, ctypes.byref(f), ctypes.byref(co), vok.data_ptr(),
                                                      pos.data_ptr(), cap, ctypes.byref(sel), ws.cuda_stream),
                       "hd_log_select_device")
        n = sel.n
        return DeviceSelection(db.rows(0, n), vok[:n], pos[:n], n, int(sel.total))

    def proposal(self, round: int) -> Optional["LogSelection"]:
        """``ProposeLogs[round]`` as a selection of one row, ``value_ok[0]``
        being ``ProposeIsValid[round]``; None when the round has no logged
        propose."""
        s = self.select(PROPOSE, round, limit=1)
        return s if len(s) else None

    def votes(self, kind, round: int) -> "LogSelection":
        """``PrevoteLogs[round]`` / ``PrecommitLogs[round]`` in arrival order."""
        return self.select(_vote_kind(kind), round)

    def vote_of(self, kind, round: int, sender) -> Optional["LogSelection"]:
        """``PrevoteLogs[round][sender]`` / ``PrecommitLogs[round][sender]`` as
        a selection of one row, or None."""
        s = self.select(_vote_kind(kind), round, sender=sender, limit=1)
        return s if len(s) else None

    def certificate(self, kind, round: int, value, upto: Optional[int] = None) -> Optional["LogSelection"]:
        """The first 2f+1 logged votes of ``kind`` for ``value`` in ``round``
        at log positions <= ``upto`` (None: the whole log): the signed votes
        behind a firing of commit or prevote_validround, for a peer to check
        with quorum.check_certificate.  None when there are fewer.

        ``upto`` is a log position.  A ``when`` of an insert's result that is
        below that insert's ``base`` already is one; a ``when`` at or above
        ``base`` is a batch index, and the message's position is
        ``result.logpos[when - result.base]`` (the message at which a count
        rule fires is a logged vote, so it has one)."""
        q = 2 * self.f + 1
        s = self.select(_vote_kind(kind), round, value=value, upto=upto, limit=q)
        return s if len(s) == q else None


@dataclass
class LogSelection:
    """What DecideLog.select returns: ``positions`` (uint32, ascending), the
    rows as a Batch with their ``value_ok`` bytes (None with rows=False), and
    ``total``, the matches there are whatever ``limit`` was."""
    positions: np.ndarray
    total: int
    batch: Optional[Batch]
    value_ok: Optional[np.ndarray]

    def __len__(self) -> int:
        return len(self.positions)


@dataclass
class DeviceSelection:
    """What DecideLog.select_device returns: ``n`` rows on the device."""
    batch: "object"          # device.DeviceBatch of n rows
    value_ok: "object"       # torch uint8[n]
    positions: "object"      # torch int32[n]
    n: int
    total: int


# statuses of check_certificates (include/hd_cert.h HD_CERT_*)
CERT_OK, CERT_SHORT, CERT_BAD_SIGNATURE, CERT_WRONG_FIELD, CERT_REPEATED_SENDER = 0, 1, 2, 3, 4
CERT_NOT_MEMBER = 5   # check_certificates_sets only: authentic, but From is outside the certificate's set
CERT_NAMES = ["OK", "SHORT", "BAD_SIGNATURE", "WRONG_FIELD", "REPEATED_SENDER", "NOT_MEMBER"]


@dataclass
class CertSpec:
    """One certificate to check (hd_cert): messages [first, first + count) of
    a batch must be VALID votes of ``kind`` ("prevote" / "precommit", or the
    type) for ``value`` at (height, round), from pairwise distinct
    signatories, at least ``quorum`` (2f+1) of them.  ``set``: the id of the
    signatory set (SignatorySets.add) the certificate falls under, read by
    check_certificates_sets when it is given no ``set_of``."""
    first: int
    count: int
    kind: object
    height: int
    round: int
    value: bytes
    quorum: int
    set: Optional[int] = None


@dataclass
class CertCheck:
    """What check_certificates returns, one entry per certificate: ``status``
    (CERT_*), ``good`` (distinct signatories among the clean messages) and
    ``first_bad`` (batch index of the lowest offending message, 0xFFFFFFFF:
    none), all uint32; ``verdict`` (uint8 per message of the batch) when
    asked for."""
    status: np.ndarray
    good: np.ndarray
    first_bad: np.ndarray
    verdict: Optional[np.ndarray] = None

    def __len__(self) -> int:
        return len(self.status)

    @property
    def ok(self) -> List[bool]:
        return [int(s) == CERT_OK for s in self.status]


def cert_rows(certs):
    """The hd_cert rows of a list of CertSpec, as a ctypes array.  Every call
    that takes ``certs`` also takes such an array as it stands, so a caller
    that checks the same segments again builds the rows once."""
    if isinstance(certs, ctypes.Array):
        return certs
    rows = (_lib.HdCert * len(certs))()
    for row, c in zip(rows, certs):
        value = bytes(c.value)
        if len(value) != 32:
            raise ValueError("a certificate's value has 32 bytes")
        row.first, row.count, row.quorum, row.type = int(c.first), int(c.count), int(c.quorum), _vote_kind(c.kind)
        row.height, row.round = int(c.height), int(c.round)
        ctypes.memmove(row.value32, value, 32)
    return rows


def cert_sets(certs, set_of, k: int) -> np.ndarray:
    """The set id of every certificate as uint32[k]: ``set_of``, or each
    CertSpec's ``set``."""
    if set_of is None:
        if isinstance(certs, ctypes.Array) or any(c.set is None for c in certs):
            raise ValueError("set_of, or a set in every CertSpec")
        set_of = [c.set for c in certs]
    ids = np.ascontiguousarray(set_of, np.int64)
    if ids.shape != (k,) or (k and (ids.min() < 0 or ids.max() > 0xFFFFFFFF)):
        raise ValueError("one set id per certificate")
    return ids.astype(np.uint32)


class SignatorySets:
    """Signatory sets resident on the device, apart from the verifier's
    admitted set (include/hd_sigsets.h): ``add`` at each ResetHeight a peer
    learns of, then check_certificates_sets decides every certificate under
    the set it names.  Nothing here touches set_signatories' set."""

    def __init__(self, v: "Verifier"):
        self._v = v
        self._lib = v._lib
        h = ctypes.c_void_p()
        v._check(self._lib.hd_sigsets_create(v.handle, ctypes.byref(h)), "hd_sigsets_create")
        self._sets = h
        self._close_rank = 0          # closed before its Verifier (either order is allowed)
        _lib.track(self)

    def close(self):
        if getattr(self, "_sets", None):
            self._lib.hd_sigsets_destroy(self._sets)
            self._sets = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def handle(self):
        return self._sets

    def _check(self, rc: int, where: str):
        if rc != 0:
            raise HDError(rc, where)

    def add(self, signatories) -> int:
        """hd_sigsets_add: one more set (n x 32 bytes, any order, duplicates
        allowed, n = 0 allowed); returns its id.  Earlier ids stay valid."""
        arr = _as_rows(signatories, 32)
        sid = ctypes.c_uint32()
        self._check(self._lib.hd_sigsets_add(self._sets, _ptr(arr) if len(arr) else None, len(arr), ctypes.byref(sid)),
                    "hd_sigsets_add")
        return int(sid.value)

    def clear(self) -> None:
        self._check(self._lib.hd_sigsets_clear(self._sets), "hd_sigsets_clear")

    def info(self, set_id: int) -> Tuple[int, int]:
        """(rows given to add, distinct rows) of a set"""
        r, d = ctypes.c_uint32(), ctypes.c_uint32()
        self._check(self._lib.hd_sigsets_info(self._sets, int(set_id), ctypes.byref(r), ctypes.byref(d)),
                    "hd_sigsets_info")
        return int(r.value), int(d.value)


def _cert_check(res, k: int, verdict=None) -> CertCheck:
    a = np.frombuffer(res, np.uint32).reshape(-1, 4)[:k]
    return CertCheck(a[:, 0].copy(), a[:, 1].copy(), a[:, 2].copy(), verdict)


_TYPE_NAMES = {"propose": PROPOSE, "prevote": PREVOTE, "precommit": PRECOMMIT}


def _type_mask(types) -> int:
    if isinstance(types, (int, np.integer, str)):
        types = (types,)
    mask = 0
    for t in types:
        t = _TYPE_NAMES.get(t) if isinstance(t, str) else int(t)
        if t not in (PROPOSE, PREVOTE, PRECOMMIT):
            raise ValueError(f"bad message type {t}")
        mask |= 1 << t
    return mask


def _vote_kind(kind) -> int:
    t = _TYPE_NAMES.get(kind, kind) if isinstance(kind, str) else int(kind)
    if t not in (PREVOTE, PRECOMMIT):
        raise ValueError(f"{kind!r} is not a vote kind")
    return t


class Verifier:
    """One context per caller thread (the reference's Process is
    single-goroutine, process/process.go:100-101)."""

    def __init__(self, device: int = 0, compressed=True):
        """compressed: the pubkey encoding of id.NewSignatory -- True / 1 SEC1
        compressed (33 B, default), False / 0 SEC1 uncompressed (65 B),
        2 raw X || Y (64 B), 3 X.Bytes() || Y.Bytes() (Go minimal encodings,
        <= 64 B) (include/hd_verify.h HD_PUBKEY_*)."""
        self._lib = _lib.load()
        h = ctypes.c_void_p()
        rc = self._lib.hd_ctx_create(device, ctypes.byref(h))
        if rc != 0:
            raise HDError(rc, "hd_ctx_create")
        self._ctx = h
        self._close_rank = 1          # closed after the queues / tables that use it
        _lib.track(self)
        self.device = device
        self._check(self._lib.hd_ctx_set_pubkey_format(self._ctx, int(compressed)), "set_pubkey_format")
        self.n_signatories = 0

    def _check(self, rc: int, where: str):
        if rc != 0:
            detail = self._lib.hd_ctx_last_error(self._ctx).decode() if self._ctx else ""
            raise HDError(rc, where, detail)

    def close(self):
        if getattr(self, "_ctx", None):
            self._lib.hd_ctx_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def handle(self):
        return self._ctx

    def set_signatories(self, signatories) -> None:
        """hd_set_signatories.  Known keys of signatories that stay admitted
        are still known on return, also when the new set size makes the
        context pick another key-table width (their tables are rebuilt inside
        the call); a forced ``key_width`` that differs from the current one, a
        pubkey format change and a set change that fails forget every key.
        ``last_set_change()`` says what happened."""
        arr = _as_rows(signatories, 32)
        self._check(self._lib.hd_set_signatories(self._ctx, _ptr(arr), len(arr)), "hd_set_signatories")
        self.n_signatories = len(arr)

    def last_set_change(self) -> dict:
        """hd_ctx_set_change_info: what the last set_signatories did to the
        known keys -- ``width_before`` / ``width_after`` (table widths in
        bits), ``kept`` (left READY in place), ``carried`` (rebuilt at another
        width or after a failed allocation), ``dropped`` (lost: the signatory
        left the set, or no slot).  All zero before the first set change or
        with the fast path off."""
        return set_change_info(self._lib, self._ctx, self._check)

    def set_pubkey_format(self, fmt) -> None:
        """hd_ctx_set_pubkey_format (values as ``compressed`` of the
        constructor); a change drops every known key, imported ones included."""
        self._check(self._lib.hd_ctx_set_pubkey_format(self._ctx, int(fmt)), "hd_ctx_set_pubkey_format")

    def import_keys(self, keys) -> Tuple[np.ndarray, np.ndarray]:
        """hd_import_keys: public keys (rows of 64 bytes, X || Y big-endian) of
        admitted signatories, so that their messages take the known-key check
        from the first batch on.  Returns (status uint8[n] of KEY_*, signer
        int32[n]: the row of the signatory array, -1 for a key that is not
        admitted or not a curve point).  The keys are not trusted: each is
        hashed in the context's pubkey format and looked up in the admitted
        set."""
        arr = _as_rows(keys, 64)
        n = len(arr)
        status = np.zeros(n, np.uint8)
        signer = np.full(n, -1, np.int32)
        self._check(self._lib.hd_import_keys(self._ctx, _ptr(arr), n, _ptr(status), _ptr(signer)), "hd_import_keys")
        return status, signer

    def export_keys(self) -> Tuple[np.ndarray, np.ndarray]:
        """hd_export_keys: (keys uint8[n, 64], known bool[n]) for the n rows of
        the signatory array last given to set_signatories; a row whose key is
        not known yet is zero."""
        cap, n = self.n_signatories, ctypes.c_uint32()
        while True:
            keys = np.zeros((cap, 64), np.uint8)
            known = np.zeros(cap, np.uint8)
            rc = self._lib.hd_export_keys(self._ctx, _ptr(keys), _ptr(known), cap, ctypes.byref(n))
            if rc != -4 or n.value <= cap:   # HD_ECAP: the set is larger than this object last saw
                break
            cap = n.value
        self._check(rc, "hd_export_keys")
        return keys[: n.value], known[: n.value].astype(bool)

    # include/hd_verify.h HD_VAR_*: kernel variants of this context
    VARIANTS = {"verify_waves": 0, "sum_waves": 1, "split_k": 4, "recover_g": 5, "key_width": 7, "wave_prio": 8,
                "sum_cap": 9, "foreign_keys": 10, "slow_lift": 11, "dedup": 12, "lean_inv": 13, "sum_chain": 14,
                "pre_share": 15}

    def set_variant(self, name: str, value: int) -> None:
        """Select a compiled kernel variant (A/B, variant tests); see
        include/hd_verify.h HD_VAR_* for the keys and values."""
        self._check(self._lib.hd_ctx_set_variant(self._ctx, self.VARIANTS[name], int(value)), "hd_ctx_set_variant")

    def variant(self, name: str) -> int:
        v = ctypes.c_int()
        self._check(self._lib.hd_ctx_get_variant(self._ctx, self.VARIANTS[name], ctypes.byref(v)), "hd_ctx_get_variant")
        return v.value

    def set_fastpath(self, enable: bool) -> None:
        """Known-key fast path on/off (include/hd_verify.h hd_ctx_set_fastpath)."""
        self._check(self._lib.hd_ctx_set_fastpath(self._ctx, 1 if enable else 0), "hd_ctx_set_fastpath")

    def profile(self, enable: bool) -> None:
        """Record HIP events around every verify call and its k_fast_sums
        launch (include/hd_verify.h hd_ctx_profile)."""
        self._check(self._lib.hd_ctx_profile(self._ctx, 1 if enable else 0), "hd_ctx_profile")

    def profile_read(self):
        """(calls, verify ms summed, k_fast_sums launches, their ms summed)
        since the last read."""
        c, s = ctypes.c_uint32(), ctypes.c_uint32()
        vm, sm = ctypes.c_double(), ctypes.c_double()
        self._check(self._lib.hd_ctx_profile_read(self._ctx, ctypes.byref(c), ctypes.byref(vm), ctypes.byref(s),
                                                  ctypes.byref(sm)), "hd_ctx_profile_read")
        return c.value, vm.value, s.value, sm.value

    def fastpath_stats(self) -> Tuple[int, int]:
        """(signatories with built key tables, messages of the last verify
        call that took the full recovery)."""
        k, f = ctypes.c_uint32(), ctypes.c_uint32()
        self._check(self._lib.hd_ctx_fastpath_stats(self._ctx, ctypes.byref(k), ctypes.byref(f)),
                    "hd_ctx_fastpath_stats")
        return int(k.value), int(f.value)

    def foreign_stats(self, checks: bool = False):
        """(foreign-key slots with built tables, slotless Froms promoted so far
        into a colder foreign key's slot[, eviction checks so far])."""
        r, e, c = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
        self._check(self._lib.hd_ctx_foreign_stats(self._ctx, ctypes.byref(r), ctypes.byref(e), ctypes.byref(c)),
                    "hd_ctx_foreign_stats")
        return (int(r.value), int(e.value), int(c.value)) if checks else (int(r.value), int(e.value))

    def dedup_stats(self) -> Tuple[int, int]:
        """(messages that entered the known-key check, those of them served as
        exact repeats of an earlier message of their call), cumulative since
        the context was created (include/hd_verify.h hd_ctx_dedup_stats)."""
        c, r = ctypes.c_uint64(), ctypes.c_uint64()
        self._check(self._lib.hd_ctx_dedup_stats(self._ctx, ctypes.byref(c), ctypes.byref(r)), "hd_ctx_dedup_stats")
        return int(c.value), int(r.value)

    def preimage_stats(self) -> Tuple[int, int]:
        """(typed messages of the calls that shared preimages, the distinct
        preimages those calls hashed), cumulative since the context was
        created (include/hd_verify.h hd_ctx_preimage_stats)."""
        t, d = ctypes.c_uint64(), ctypes.c_uint64()
        self._check(self._lib.hd_ctx_preimage_stats(self._ctx, ctypes.byref(t), ctypes.byref(d)),
                    "hd_ctx_preimage_stats")
        return int(t.value), int(d.value)

    def overlap_stats(self) -> Tuple[int, int, int]:
        """(calls with a capped k_fast_sums, calls with the lean inversion
        kernels, calls whose sums waited for the previous call's), cumulative
        (include/hd_verify.h hd_ctx_overlap_stats)."""
        c, l, w = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
        self._check(self._lib.hd_ctx_overlap_stats(self._ctx, ctypes.byref(c), ctypes.byref(l), ctypes.byref(w)),
                    "hd_ctx_overlap_stats")
        return int(c.value), int(l.value), int(w.value)

    def inv_levels(self, set: int = -1) -> int:
        """Levels of the lean inversions (1 or 2); `set` 1 or 2 changes it for
        the calls that follow (include/hd_verify.h hd_ctx_inv_levels)."""
        got = self._lib.hd_ctx_inv_levels(self._ctx, set)
        if got not in (1, 2):
            self._check(got if got < 0 else -1, "hd_ctx_inv_levels")
        return got

    def inv_stats(self) -> Tuple[int, int]:
        """(lean calls that launched the two-level inversions, lean calls that
        launched the one-level kernels), cumulative
        (include/hd_verify.h hd_ctx_inv_stats)."""
        out = (ctypes.c_uint64 * 2)()
        self._check(self._lib.hd_ctx_inv_stats(self._ctx, out), "hd_ctx_inv_stats")
        return int(out[0]), int(out[1])

    def fastpath_geometry(self) -> Tuple[int, int, int]:
        """(G table windows, per-key table windows, messages sharing one
        inversion) of the known-key check as this context runs it."""
        g, k, m = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        self._check(self._lib.hd_ctx_fastpath_geometry(self._ctx, ctypes.byref(g), ctypes.byref(k), ctypes.byref(m)),
                    "hd_ctx_fastpath_geometry")
        return int(g.value), int(k.value), int(m.value)

    def known_keys(self) -> int:
        return self.fastpath_stats()[0]

    def verify_batch(self, batch: Batch, recovered: bool = True) -> VerifyResult:
        n = len(batch)
        verdict = np.zeros(n, np.uint8)
        rec = np.zeros((n, 32), np.uint8)
        bitmap = np.zeros((n + 31) // 32, np.uint32)
        cb = batch.c_struct()
        self._check(self._lib.hd_verify_batch(self._ctx, ctypes.byref(cb), _ptr(verdict),
                                              _ptr(rec) if recovered else None, _ptr(bitmap)), "hd_verify_batch")
        return VerifyResult(verdict, rec, bitmap)

    def submit(self, batch: Batch, verdict: np.ndarray, recovered: Optional[np.ndarray] = None,
               bitmap: Optional[np.ndarray] = None) -> int:
        """Asynchronous host-buffer verification (hd_verify_submit): returns a
        ticket; the outputs land in the given arrays by wait(ticket).  The
        batch arrays and the outputs must stay alive (and the inputs
        unchanged) until then; pinned arrays (torch pin_memory / pinned_empty)
        move by DMA without a staging copy."""
        cb = batch.c_struct()
        t = ctypes.c_uint64()
        self._check(self._lib.hd_verify_submit(self._ctx, ctypes.byref(cb), _ptr(verdict), _ptr(recovered),
                                               _ptr(bitmap), ctypes.byref(t)), "hd_verify_submit")
        return t.value

    def submit_compact(self, batch: CompactBatch, verdict: np.ndarray, recovered: Optional[np.ndarray] = None,
                       bitmap: Optional[np.ndarray] = None) -> int:
        """hd_verify_submit_compact: as submit, with From and value as indices
        (CompactBatch.from_batch); the outputs are the expanded batch's."""
        cb = batch.c_struct()
        t = ctypes.c_uint64()
        self._check(self._lib.hd_verify_submit_compact(self._ctx, ctypes.byref(cb), _ptr(verdict), _ptr(recovered),
                                                       _ptr(bitmap), ctypes.byref(t)), "hd_verify_submit_compact")
        return t.value

    def wait(self, ticket: int) -> None:
        self._check(self._lib.hd_verify_wait(self._ctx, int(ticket)), "hd_verify_wait")

    def verify_batch_device(self, dbatch: HdBatch, d_verdict: int, d_recovered: Optional[int] = None,
                            d_signer: Optional[int] = None, d_bitmap: Optional[int] = None,
                            stream: Optional[int] = None) -> None:
        """Device-resident variant: every pointer is a device address."""
        self._check(self._lib.hd_verify_batch_device(self._ctx, ctypes.byref(dbatch), d_verdict, d_recovered,
                                                     d_signer, d_bitmap, stream), "hd_verify_batch_device")

    def authenticate_batch_device(self, dbatch: HdBatch, d_verdict: int, stream: Optional[int] = None) -> None:
        """Verdicts for the replica ingress (hd_authenticate_batch_device):
        VALID and NOT_ADMITTED exactly as verify_batch_device; a message whose
        From has a known key that does not verify its signature is final as
        NOT_AUTHENTIC, without the recovery that would classify it (the
        reference drops every unauthenticated message, process/process.go:95-98)."""
        self._check(self._lib.hd_authenticate_batch_device(self._ctx, ctypes.byref(dbatch), d_verdict, stream),
                    "hd_authenticate_batch_device")

    # ---- certificates ---------------------------------------------------
    def check_certificates(self, batch: Batch, certs, verdict: bool = False) -> CertCheck:
        """hd_check_certificates: one upload of ``batch``, its verification
        against this verifier's signatory set, and the check of every
        certificate of ``certs`` (CertSpec segments of the batch, or their
        cert_rows) in one launch behind
        it; one synchronisation.  ``verdict=True`` also returns the
        per-message verdicts, which say why a BAD_SIGNATURE message failed."""
        rows = cert_rows(certs)
        k = len(rows)
        res = (_lib.HdCertResult * max(k, 1))()
        vd = np.zeros(len(batch), np.uint8) if verdict else None
        cb = batch.c_struct()
        self._check(self._lib.hd_check_certificates(self._ctx, ctypes.byref(cb), rows, k, res, _ptr(vd)),
                    "hd_check_certificates")
        return _cert_check(res, k, vd)

    def check_certificates_device(self, dbatch: HdBatch, d_bitmap: int, d_signer: int, n_signers: int,
                                  certs, stream: Optional[int] = None) -> CertCheck:
        """hd_check_certificates_device: the batch, the valid bitmap and the
        signer indices are the device outputs of verify_batch_device;
        ``n_signers`` is the size of the signatory set that verified them.
        Queued on ``stream`` behind the verification, which is synchronised
        once."""
        rows = cert_rows(certs)
        k = len(rows)
        res = (_lib.HdCertResult * max(k, 1))()
        self._check(self._lib.hd_check_certificates_device(self._ctx, ctypes.byref(dbatch), d_bitmap, d_signer,
                                                           int(n_signers), rows, k, res, stream),
                    "hd_check_certificates_device")
        return _cert_check(res, k)

    def open_sets(self) -> SignatorySets:
        """An empty collection of signatory sets on this context (hd_sigsets)."""
        return SignatorySets(self)

    def check_certificates_sets(self, batch: Batch, certs, sets: SignatorySets, set_of=None,
                                verdict: bool = False) -> CertCheck:
        """hd_check_certificates_sets: as check_certificates, with certificate
        k decided under set ``set_of[k]`` of ``sets`` (or its CertSpec's
        ``set``) instead of this verifier's signatory set, which the call
        leaves alone.  A message whose signature is its From's but whose From
        is outside the certificate's set makes the status CERT_NOT_MEMBER."""
        rows = cert_rows(certs)
        k = len(rows)
        ids = cert_sets(certs, set_of, k)
        res = (_lib.HdCertResult * max(k, 1))()
        vd = np.zeros(len(batch), np.uint8) if verdict else None
        cb = batch.c_struct()
        self._check(self._lib.hd_check_certificates_sets(self._ctx, sets.handle, ctypes.byref(cb), rows, _ptr(ids), k,
                                                         res, _ptr(vd)), "hd_check_certificates_sets")
        return _cert_check(res, k, vd)

    def check_certificates_sets_device(self, dbatch: HdBatch, d_verdict: int, certs, sets: SignatorySets,
                                       set_of=None, stream: Optional[int] = None) -> CertCheck:
        """hd_check_certificates_sets_device: the batch on the device (type,
        height, round, value and From are read) and the verdict bytes
        verify_batch_device or authenticate_batch_device wrote for it.  Queued
        on ``stream`` behind the verification, which is synchronised once."""
        rows = cert_rows(certs)
        k = len(rows)
        ids = cert_sets(certs, set_of, k)
        res = (_lib.HdCertResult * max(k, 1))()
        self._check(self._lib.hd_check_certificates_sets_device(self._ctx, sets.handle, ctypes.byref(dbatch), d_verdict,
                                                                rows, _ptr(ids), k, res, stream),
                    "hd_check_certificates_sets_device")
        return _cert_check(res, k)

    @staticmethod
    def cert_plan(n_signers: int, k: int) -> dict:
        """hd_cert_plan_info: where the check keeps its per-signer table and
        the grid it launches (diagnostics)."""
        p = _lib.HdCertPlan()
        rc = _lib.load().hd_cert_plan_info(int(n_signers), int(k), ctypes.byref(p))
        if rc != 0:
            raise HDError(rc, "hd_cert_plan_info")
        return {name: int(getattr(p, name)) for name, _ in p._fields_}

    # ---- tally -------------------------------------------------------
    @staticmethod
    def _tally_struct(n: int, pinned: bool = False):
        """Output arrays for n messages.  pinned: page-locked host memory (torch
        pin_memory), so the library's device-to-host copies are plain DMA on
        the tally's stream instead of staged pageable copies."""
        keep = []

        def mk(dtype):
            if not pinned:
                return np.zeros(max(n, 1), dtype)
            import torch
            tdt = {np.int64: torch.int64, np.uint8: torch.uint8, np.uint32: torch.int32}[dtype]
            t = torch.zeros(max(n, 1), dtype=tdt, pin_memory=True)
            keep.append(t)
            return t.numpy().view(dtype)

        arrs = dict(
            count_height=mk(np.int64), count_round=mk(np.int64), count_type=mk(np.uint8), count_rep=mk(np.uint32),
            count_n=mk(np.uint32), hr_height=mk(np.int64), hr_round=mk(np.int64), hr_prevotes=mk(np.uint32),
            hr_precommits=mk(np.uint32), hr_any=mk(np.uint32), dup=mk(np.uint8), hr_rep=mk(np.uint32))
        if keep:
            arrs["_pinned"] = keep
        t = HdTallyOut()
        t.cap_counts = n
        t.cap_hr = n
        for k, a in arrs.items():
            if not k.startswith("_"):
                setattr(t, k, _ptr(a))
        return t, arrs

    @staticmethod
    def _tally_result(batch: Batch, t: HdTallyOut, a) -> TallyResult:
        count = {}
        for k in range(t.n_counts):
            rep = int(a["count_rep"][k])
            count[(int(a["count_height"][k]), int(a["count_round"][k]), int(a["count_type"][k]),
                   batch.value[rep].tobytes())] = int(a["count_n"][k])
        distinct, distinct_any = {}, {}
        for k in range(t.n_hr):
            h, r = int(a["hr_height"][k]), int(a["hr_round"][k])
            if a["hr_prevotes"][k]:
                distinct[(h, r, PREVOTE)] = int(a["hr_prevotes"][k])
            if a["hr_precommits"][k]:
                distinct[(h, r, PRECOMMIT)] = int(a["hr_precommits"][k])
            distinct_any[(h, r)] = int(a["hr_any"][k])
        return TallyResult(count, distinct, distinct_any, a["dup"][: len(batch)].copy())

    def tally(self, batch: Batch, verdict: np.ndarray) -> TallyResult:
        n = len(batch)
        verdict = np.ascontiguousarray(verdict, dtype=np.uint8)
        t, a = self._tally_struct(n)
        cb = batch.c_struct()
        self._check(self._lib.hd_tally(self._ctx, ctypes.byref(cb), _ptr(verdict), ctypes.byref(t)), "hd_tally")
        return self._tally_result(batch, t, a)

    def process_batch(self, batch: Batch) -> Tuple[VerifyResult, TallyResult]:
        n = len(batch)
        verdict = np.zeros(n, np.uint8)
        rec = np.zeros((n, 32), np.uint8)
        bitmap = np.zeros((n + 31) // 32, np.uint32)
        t, a = self._tally_struct(n)
        cb = batch.c_struct()
        self._check(self._lib.hd_process_batch(self._ctx, ctypes.byref(cb), _ptr(verdict), _ptr(rec), _ptr(bitmap),
                                               ctypes.byref(t)), "hd_process_batch")
        return VerifyResult(verdict, rec, bitmap), self._tally_result(batch, t, a)

    # ---- decide ------------------------------------------------------
    @staticmethod
    def _decide_struct(n: int, cap: Optional[int] = None):
        from ._lib import HdDecideOut
        cap = n if cap is None else cap
        dt = {"height": np.int64, "round": np.int64, "flags": np.uint8, "bits": np.uint8}
        arrs = {k: np.zeros(max(cap, 1), dt.get(k, np.uint32)) for k in HdDecideOut.ROW_FIELDS}
        arrs["pclass"] = np.zeros(max(n, 1), np.uint8)
        arrs["dup"] = np.zeros(max(n, 1), np.uint8)
        o = HdDecideOut()
        o.cap = cap
        for k, a in arrs.items():
            setattr(o, k, _ptr(a))
        return o, arrs

    @staticmethod
    def _decide_result(n: int, o, a, caught=None) -> DecideResult:
        rows = {k: a[k][: o.n].copy() for k in type(o).ROW_FIELDS}
        cls, extra = (CaughtDecideResult, _caught_fields(*caught)) if caught else (DecideResult, {})
        return cls(pclass=a["pclass"][:n].copy(), dup=a["dup"][:n].copy(), **rows, **extra)

    def decide(self, batch: Batch, verdict: np.ndarray, f: int, schedule=None, value_ok=None,
               catch: bool = False) -> DecideResult:
        """hd_decide: the vote logs of :meth:`tally`, the propose log of
        process.go:758-819 and every round's eight predicates, on the device.
        schedule: the round-robin order of signatories (rows of 32 bytes) or
        None for no turn check; value_ok: one byte per message standing in for
        validator.Valid on a propose's value (None: every non-nil value is
        valid); catch: also return the catch list (a CaughtDecideResult with
        ``caught``; hd_decide_catch)."""
        from ._lib import HdDecideIn
        n = len(batch)
        verdict = np.ascontiguousarray(verdict, dtype=np.uint8)
        if len(verdict) != n:
            raise ValueError("verdict length mismatch")
        sched = _as_rows(schedule, 32) if schedule is not None else None
        if sched is not None and len(sched) == 0:
            raise ValueError("an empty schedule (pass None for no turn check)")
        vok = np.ascontiguousarray(value_ok, dtype=np.uint8) if value_ok is not None else None
        if vok is not None and len(vok) != n:
            raise ValueError("value_ok length mismatch")
        o, a = self._decide_struct(n)
        cin = HdDecideIn(int(f), len(sched) if sched is not None else 0, _ptr(sched), _ptr(vok))
        cb = batch.c_struct()
        if catch:
            c, ca = _catch_struct(n)
            self._check(self._lib.hd_decide_catch(self._ctx, ctypes.byref(cb), _ptr(verdict), ctypes.byref(cin),
                                                  ctypes.byref(o), None, ctypes.byref(c)), "hd_decide_catch")
            return self._decide_result(n, o, a, (c, ca))
        self._check(self._lib.hd_decide(self._ctx, ctypes.byref(cb), _ptr(verdict), ctypes.byref(cin),
                                        ctypes.byref(o)), "hd_decide")
        return self._decide_result(n, o, a)

    def decide_device(self, dbatch: HdBatch, d_bitmap: int, f: int, schedule=None, value_ok=None,
                      stream: Optional[int] = None, catch: bool = False) -> DecideResult:
        """hd_decide_device_bitmap over a device batch and the valid bitmap of
        verify_batch_device.  schedule / value_ok: torch tensors on the device
        (uint8 [n_sched, 32] / [n]), or host arrays, which are uploaded first."""
        import torch
        from ._lib import HdDecideIn
        n = dbatch.n

        def dev(x, width):
            if x is None or isinstance(x, torch.Tensor):
                return x
            arr = _as_rows(x, width) if width > 1 else np.ascontiguousarray(x, dtype=np.uint8)
            t = torch.from_numpy(arr).cuda()
            torch.cuda.current_stream().synchronize()
            return t

        sched, vok = dev(schedule, 32), dev(value_ok, 1)
        if sched is not None and sched.numel() == 0:
            raise ValueError("an empty schedule (pass None for no turn check)")
        if vok is not None and vok.numel() != n:
            raise ValueError("value_ok length mismatch")
        o, a = self._decide_struct(n)
        cin = HdDecideIn(int(f), sched.numel() // 32 if sched is not None else 0,
                         sched.data_ptr() if sched is not None else None,
                         vok.data_ptr() if vok is not None else None)
        if catch:
            c, ca = _catch_struct(n)
            self._check(self._lib.hd_decide_catch_device_bitmap(self._ctx, ctypes.byref(dbatch), d_bitmap,
                                                                ctypes.byref(cin), ctypes.byref(o), None,
                                                                ctypes.byref(c), stream),
                        "hd_decide_catch_device_bitmap")
            return self._decide_result(n, o, a, (c, ca))
        self._check(self._lib.hd_decide_device_bitmap(self._ctx, ctypes.byref(dbatch), d_bitmap, ctypes.byref(cin),
                                                      ctypes.byref(o), stream), "hd_decide_device_bitmap")
        return self._decide_result(n, o, a)

    # ---- decide, ordered ---------------------------------------------
    @staticmethod
    def _order_struct(cap: int):
        from ._lib import HdDecideOrder
        when = np.full((max(cap, 1), 8), WHEN_NEVER, np.uint32)
        until = np.full(max(cap, 1), WHEN_NEVER, np.uint32)
        w = HdDecideOrder()
        w.cap = cap
        w.when = _ptr(when)
        w.exact_until = _ptr(until)
        return w, when, until

    @staticmethod
    def _ordered_result(n: int, o, a, when, until, caught=None) -> OrderedDecideResult:
        rows = {k: a[k][: o.n].copy() for k in type(o).ROW_FIELDS}
        cls, extra = (CaughtOrderedDecideResult, _caught_fields(*caught)) if caught else (OrderedDecideResult, {})
        return cls(pclass=a["pclass"][:n].copy(), dup=a["dup"][:n].copy(), when=when[: o.n].copy(),
                   exact_until=until[: o.n].copy(), **rows, **extra)

    def decide_ordered(self, batch: Batch, verdict: np.ndarray, f: int, schedule=None,
                       value_ok=None, catch: bool = False) -> OrderedDecideResult:
        """hd_decide_ordered: :meth:`decide` plus the batch index at which each
        round's predicates first hold in batch order (``when``,
        ``exact_until``, ``firings``).  Arguments as :meth:`decide`."""
        from ._lib import HdDecideIn
        n = len(batch)
        verdict = np.ascontiguousarray(verdict, dtype=np.uint8)
        if len(verdict) != n:
            raise ValueError("verdict length mismatch")
        sched = _as_rows(schedule, 32) if schedule is not None else None
        if sched is not None and len(sched) == 0:
            raise ValueError("an empty schedule (pass None for no turn check)")
        vok = np.ascontiguousarray(value_ok, dtype=np.uint8) if value_ok is not None else None
        if vok is not None and len(vok) != n:
            raise ValueError("value_ok length mismatch")
        o, a = self._decide_struct(n)
        w, when, until = self._order_struct(n)
        cin = HdDecideIn(int(f), len(sched) if sched is not None else 0, _ptr(sched), _ptr(vok))
        cb = batch.c_struct()
        if catch:
            c, ca = _catch_struct(n)
            self._check(self._lib.hd_decide_catch(self._ctx, ctypes.byref(cb), _ptr(verdict), ctypes.byref(cin),
                                                  ctypes.byref(o), ctypes.byref(w), ctypes.byref(c)),
                        "hd_decide_catch")
            return self._ordered_result(n, o, a, when, until, (c, ca))
        self._check(self._lib.hd_decide_ordered(self._ctx, ctypes.byref(cb), _ptr(verdict), ctypes.byref(cin),
                                                ctypes.byref(o), ctypes.byref(w)), "hd_decide_ordered")
        return self._ordered_result(n, o, a, when, until)

    def decide_ordered_device(self, dbatch: HdBatch, d_bitmap: int, f: int, schedule=None, value_ok=None,
                              stream: Optional[int] = None, catch: bool = False) -> OrderedDecideResult:
        """hd_decide_ordered_device_bitmap; arguments as :meth:`decide_device`."""
        import torch
        from ._lib import HdDecideIn
        n = dbatch.n

        def dev(x, width):
            if x is None or isinstance(x, torch.Tensor):
                return x
            arr = _as_rows(x, width) if width > 1 else np.ascontiguousarray(x, dtype=np.uint8)
            t = torch.from_numpy(arr).cuda()
            torch.cuda.current_stream().synchronize()
            return t

        sched, vok = dev(schedule, 32), dev(value_ok, 1)
        if sched is not None and sched.numel() == 0:
            raise ValueError("an empty schedule (pass None for no turn check)")
        if vok is not None and vok.numel() != n:
            raise ValueError("value_ok length mismatch")
        o, a = self._decide_struct(n)
        w, when, until = self._order_struct(n)
        cin = HdDecideIn(int(f), sched.numel() // 32 if sched is not None else 0,
                         sched.data_ptr() if sched is not None else None,
                         vok.data_ptr() if vok is not None else None)
        if catch:
            c, ca = _catch_struct(n)
            self._check(self._lib.hd_decide_catch_device_bitmap(self._ctx, ctypes.byref(dbatch), d_bitmap,
                                                                ctypes.byref(cin), ctypes.byref(o), ctypes.byref(w),
                                                                ctypes.byref(c), stream),
                        "hd_decide_catch_device_bitmap")
            return self._ordered_result(n, o, a, when, until, (c, ca))
        self._check(self._lib.hd_decide_ordered_device_bitmap(self._ctx, ctypes.byref(dbatch), d_bitmap,
                                                              ctypes.byref(cin), ctypes.byref(o), ctypes.byref(w),
                                                              stream), "hd_decide_ordered_device_bitmap")
        return self._ordered_result(n, o, a, when, until)

    # ---- decide across calls -----------------------------------------
    def open_log(self, height: int, f: int, schedule=None, max_entries: int = 0,
                 keep_signatures: bool = False) -> DecideLog:
        """A device-resident log of one height on this context (hd_log):
        ``log.insert(batch, verdict)`` after ``log.insert(...)`` returns what
        :meth:`decide_ordered` would return for the batches joined.
        max_entries: the most entries the log may hold (0: no limit).
        keep_signatures: each entry also keeps its 65 signature bytes, so
        ``log.read`` and ``insert(..., catch=True, evidence=True)`` return
        whole messages.  The log's inserts and this verifier's tallies and
        decides go on one stream."""
        return DecideLog(self, height, f, schedule, max_entries, keep_signatures)

    # ---- synthetic workload ------------------------------------------
    def gen_keys(self, S: int) -> Tuple[np.ndarray, np.ndarray]:
        sigs = np.zeros((S, 32), np.uint8)
        foreign = np.zeros((16, 32), np.uint8)
        self._check(self._lib.hd_gen_keys(self._ctx, S, _ptr(sigs), _ptr(foreign)), "hd_gen_keys")
        return sigs, foreign


def _as_rows(x, width: int) -> np.ndarray:
    if isinstance(x, np.ndarray):
        arr = np.ascontiguousarray(x, dtype=np.uint8).reshape(-1, width)
    else:
        x = list(x)
        for s in x:
            if len(s) != width:
                raise ValueError(f"expected {width}-byte entries")
        arr = np.frombuffer(b"".join(x), np.uint8).reshape(-1, width).copy() if x else np.zeros((0, width), np.uint8)
    return arr


def probe_valu(device: int = 0, op: int = 1, iters: int = 2000) -> float:
    """Measured lane-ops/s of one VALU instruction class (include/hd_probe.h)."""
    lib = _lib.load()
    out = ctypes.c_double()
    rc = lib.hd_probe_valu(device, op, iters, ctypes.byref(out))
    if rc != 0:
        raise HDError(rc, "hd_probe_valu")
    return out.value
