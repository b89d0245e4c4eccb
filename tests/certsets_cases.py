"""The yardstick of hd_check_certificates_sets (include/hd_cert.h, second half;
include/hd_sigsets.h): a Python model of the segmented check under several
signatory sets, the synthetic cases the host and the GPU test share, and the
driver of the host replay (tests/native/hd_certsets_check.cpp).

The model walks each segment in index order, as the header states the
semantics: a message is *not authentic* (verdict byte neither VALID nor
NOT_ADMITTED), else *not a member* (its From is no entry of the certificate's
set), else *wrong* (type, height, round or value differs), else a *repeat* (a
lower clean message of the segment has its From), else it counts.  Nothing here
calls the library; tests/test_certsets_host.py pins the model on hand-worked
segments.  adm_hash and adm_index_slots are restated from
hyperdrive_amd/csrc/hd_verify_msg.h only to construct inputs (entries that
collide, entries whose probe wraps)."""
from __future__ import annotations

import hashlib
import os
import shutil
import struct
import subprocess
from dataclasses import dataclass, field
from typing import Dict, List, Sequence, Tuple

from cert_cases import FIRST, LENGTHS, NEVER, PRECOMMIT, PREVOTE, Cert, value

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, SHORT, BAD_SIGNATURE, WRONG_FIELD, REPEATED_SENDER, NOT_MEMBER = 0, 1, 2, 3, 4, 5
VALID, BAD_RS, NOT_ADMITTED = 0, 2, 6
AUTHENTIC = (VALID, NOT_ADMITTED)
H, R, V = 7, 3, value(0)   # height != round: a compare that reads the wrong column shows


# ---- the model ------------------------------------------------------------------
def check_sets(certs: Sequence[Cert], set_of, sets, types, heights, rounds, values, froms,
               verdicts) -> List[Tuple[int, int, int]]:
    """(status, good, first_bad) per certificate"""
    out = []
    for c, sid in zip(certs, set_of):
        members = set(sets[sid])
        seen, good, bad, cls = set(), 0, NEVER, OK
        for i in range(c.first, c.first + c.count):
            if verdicts[i] not in AUTHENTIC:
                k = BAD_SIGNATURE
            elif froms[i] not in members:
                k = NOT_MEMBER
            elif (types[i], heights[i], rounds[i], values[i]) != (c.type, c.height, c.round, c.value):
                k = WRONG_FIELD
            elif froms[i] in seen:
                k = REPEATED_SENDER
            else:
                seen.add(froms[i])
                good += 1
                continue
            if bad == NEVER:
                bad, cls = i, k
        out.append((SHORT if c.count < c.quorum else cls, good, bad))
    return out


# ---- the index, restated to construct inputs ----------------------------------------
M64 = (1 << 64) - 1


def adm_hash(row: bytes) -> int:
    k0, k1, k2, k3 = struct.unpack(">4I", row[:16])
    x = (k0 << 32 | k1) ^ (((k2 << 32 | k3) * 0x9E3779B97F4A7C15) & M64)
    x ^= x >> 31
    x = (x * 0xBF58476D1CE4E5B9) & M64
    x ^= x >> 29
    return x & 0xFFFFFFFF


def adm_index_slots(n: int) -> int:
    c = 16
    while c < 4 * n:
        c <<= 1
    return c


_SIGS: Dict[Tuple[int, int], bytes] = {}


def sig(family: int, j: int) -> bytes:
    """signatory j of a family of pairwise distinct 32-byte rows (families are disjoint)"""
    key = (family, j)
    if key not in _SIGS:
        _SIGS[key] = hashlib.sha256(b"sigset %d %d" % key).digest()
    return _SIGS[key]


def family(f: int, n: int) -> List[bytes]:
    return [sig(f, j) for j in range(n)]


def rows_hashing_to(slot: int, slots: int, how_many: int, seed: int) -> List[bytes]:
    """distinct rows whose adm_hash lands on `slot` of `slots`, found by search"""
    out, j = [], 0
    while len(out) < how_many:
        row = hashlib.sha256(b"wrap %d %d" % (seed, j)).digest()
        if adm_hash(row) & (slots - 1) == slot:
            out.append(row)
        j += 1
    return out


# ---- synthetic cases --------------------------------------------------------------
@dataclass
class SCase:
    """Sets as given to add (any order, duplicates allowed), a batch as columns, and the certificates
    over it with the set each names."""
    sets: List[List[bytes]]
    type: List[int] = field(default_factory=list)
    height: List[int] = field(default_factory=list)
    round: List[int] = field(default_factory=list)
    value: List[bytes] = field(default_factory=list)
    verdict: List[int] = field(default_factory=list)
    frm: List[bytes] = field(default_factory=list)
    certs: List[Cert] = field(default_factory=list)
    set_of: List[int] = field(default_factory=list)
    _ordered: Dict[int, tuple] = field(default_factory=dict, repr=False)

    @property
    def n(self) -> int:
        return len(self.type)

    def ordered(self, sid: int) -> List[bytes]:
        """the set's sorted distinct rows (kept until the set's list is replaced)"""
        rows = self.sets[sid]
        hit = self._ordered.get(sid)
        if hit is None or hit[0] is not rows or hit[1] != len(rows):
            hit = self._ordered[sid] = (rows, len(rows), sorted(set(rows)))
        return hit[2]

    def pick(self, sid: int, j: int) -> bytes:
        """logical signer j of a set: even j from the bottom of its sorted rows, odd j from the top, so
        that the lowest and the highest entry are reached; distinct while j < the distinct count"""
        rows = self.ordered(sid)
        return rows[(j // 2 if j % 2 == 0 else len(rows) - 1 - j // 2) % len(rows)]

    def msg(self, frm: bytes, t=PRECOMMIT, h=H, r=R, v=V, verdict=None) -> int:
        self.type.append(t)
        self.height.append(h)
        self.round.append(r)
        self.value.append(v)
        # both authentic bytes in turn: NOT_ADMITTED says nothing about the certificate's set
        self.verdict.append((VALID, NOT_ADMITTED)[self.n % 2] if verdict is None else verdict)
        self.frm.append(frm)
        return self.n - 1

    def pad(self, sid: int, k: int) -> None:
        """k messages that would be clean in any segment here, from the signers the segments use: a
        read outside [first, first + count) shows up as a repeat or a wrong count"""
        for j in range(k):
            self.msg(self.pick(sid, j))

    def seg(self, sid: int, count: int, quorum=None, t=PRECOMMIT, h=H, r=R, v=V, shift: int = 0) -> int:
        """count clean messages from logical signers shift .. shift + count - 1 of set sid, and their
        certificate under that set; returns the segment's first index"""
        first = self.n
        for j in range(count):
            self.msg(self.pick(sid, shift + j), t, h, r, v)
        self.cert(first, count, sid, quorum, t, h, r, v)
        return first

    def cert(self, first, count, sid, quorum=None, t=PRECOMMIT, h=H, r=R, v=V) -> None:
        self.certs.append(Cert(first, count, max(count, 1) if quorum is None else quorum, t, h, r, v))
        self.set_of.append(sid)

    def expected(self):
        return check_sets(self.certs, self.set_of, self.sets, self.type, self.height, self.round, self.value,
                          self.frm, self.verdict)


OUTSIDER = 99   # a family no set is built from


def offend(c: SCase, i: int, kind: str, against: int = None) -> None:
    if kind == "notauth":
        c.verdict[i] = BAD_RS
    elif kind == "nonmember":
        c.frm[i] = sig(OUTSIDER, i)
    elif kind == "type":
        c.type[i] = PREVOTE
    elif kind == "height":
        c.height[i] = R      # the certificate's round, so only a compare of the height column sees it
    elif kind == "round":
        c.round[i] = H
    elif kind == "value":
        c.value[i] = V[:31] + bytes([V[31] ^ 1])
    elif kind == "repeat":
        c.frm[i] = c.frm[against]
    else:
        raise ValueError(kind)


KINDS = ["notauth", "nonmember", "type", "height", "round", "value", "repeat"]
STATUS_OF = {"notauth": BAD_SIGNATURE, "nonmember": NOT_MEMBER, "repeat": REPEATED_SENDER}   # else WRONG_FIELD


def lengths_case(L: int) -> SCase:
    c = SCase([family(0, 8000)])
    c.pad(0, FIRST)
    c.seg(0, L)
    c.pad(0, 5)
    return c


def two_sets_case(count: int = 70, j: int = 41) -> SCase:
    """one message range under set 0 (all of its signers) and under set 1 (all but message j's)"""
    full = family(1, 200)
    c = SCase([full, []])
    c.pad(0, FIRST)
    first = c.seg(0, count)
    c.sets[1] = [s for s in full if s != c.frm[first + j]]
    c.cert(first, count, 1)
    c.pad(0, 3)
    return c


def precedence_case(n_members: int = 300) -> SCase:
    c = SCase([family(2, n_members)])
    c.pad(0, FIRST)
    # every class at once on one message, then every pair: the first class in the header's order decides
    first = c.seg(0, 60)
    for kind in ("notauth", "nonmember", "value"):
        offend(c, first + 30, kind)
    for a, b in (("notauth", "nonmember"), ("notauth", "value"), ("nonmember", "round"), ("notauth", "repeat"),
                 ("nonmember", "repeat"), ("height", "repeat")):
        first = c.seg(0, 60)
        offend(c, first + 30, "repeat" if b == "repeat" else a, first + 4)   # the repeat first: the other kind may
        offend(c, first + 30, a if b == "repeat" else b, first + 4)          # replace the From it copied
    # two offenders of different classes: the lower index decides, whatever the classes
    for lo in KINDS:
        for hi in KINDS:
            if lo != hi:
                first = c.seg(0, 40)
                offend(c, first + 10, lo, first + 2)
                offend(c, first + 20, hi, first + 3)
    # SHORT wins over every class, and good / first_bad are still filled
    for kind in KINDS:
        first = c.seg(0, 10, quorum=11)
        offend(c, first + 4, kind, first + 1)
    # count >= quorum decides SHORT, not good
    first = c.seg(0, 10, quorum=10)
    offend(c, first + 4, "nonmember")
    # a non-member or not authentic "first occurrence" never makes a later message a repeat
    first = c.seg(0, 60)
    offend(c, first + 5, "nonmember")
    c.frm[first + 40] = c.frm[first + 5]           # the same outsider again: not a member again, never a repeat
    first = c.seg(0, 60)
    offend(c, first + 40, "repeat", first + 5)     # 40 has 5's From ...
    offend(c, first + 5, "notauth")                # ... but 5 is not authentic: 40 counts, 5 is the offender
    first = c.seg(0, 60)
    offend(c, first + 40, "repeat", first + 5)
    offend(c, first + 5, "value")                  # ... 5 is wrong: 40 counts
    # a repeat whose first occurrence lies 300 messages earlier: past what a lane keeps of its own
    first = c.seg(0, 1300, shift=0) if n_members >= 1300 else c.seg(0, min(n_members, 290))
    offend(c, first + (1290 if n_members >= 1300 else 280), "repeat", first + 50)
    c.pad(0, 3)
    return c


def verdict_bytes_case() -> SCase:
    """every HD_VERDICT_* value on an otherwise clean member: only 0 and 6 are authentic"""
    c = SCase([family(3, 40)])
    c.pad(0, FIRST)
    for v in range(9):
        first = c.seg(0, 7)
        c.verdict[first + 3] = v
    c.pad(0, 2)
    return c


def index_edges_case() -> SCase:
    """the hashed index at its edges: one probe chain of entries that share their first 16 bytes, a probe
    that wraps past the last slot, a From equal to an entry in its first 31 bytes only, and sets of 0,
    1, duplicate rows and 4n an exact power of two"""
    prefix = hashlib.sha256(b"prefix").digest()[:16]
    chain = [prefix + hashlib.sha256(b"suffix %d" % j).digest()[:16] for j in range(24)]
    last16 = rows_hashing_to(15, 16, 4, 1)            # a set of <= 4 rows has 16 slots
    wrap = last16[:3] + [sig(4, 0)]
    assert adm_index_slots(len(wrap)) == 16
    last64 = rows_hashing_to(63, 64, 6, 2)            # 16 rows: 4 * 16 = 64 slots exactly
    pow2 = last64[:5] + family(5, 11)
    assert adm_index_slots(len(pow2)) == 64 == 4 * len(pow2)
    dup = family(6, 9)
    dup = dup + dup[2:6] + dup[:1]                      # 14 rows, 9 distinct
    c = SCase([chain, wrap, [], [sig(7, 0)], dup, pow2])
    c.pad(0, FIRST)
    # 0: every entry of the chain, then a stranger with the chain's first 16 bytes
    c.seg(0, len(chain))
    first = c.seg(0, len(chain))
    c.frm[first + 9] = prefix + hashlib.sha256(b"stranger").digest()[:16]
    # 1: the three rows on slot 15 spill to slots 0 and 1; a stranger on slot 15 walks the whole chain
    c.seg(1, 4)
    first = c.seg(1, 4)
    c.frm[first + 2] = last16[3]
    # a From that equals an entry in its first 31 bytes only, in each of these sets
    for sid in (0, 1, 5):
        first = c.seg(sid, 4)
        f = c.frm[first + 1]
        c.frm[first + 1] = f[:31] + bytes([f[31] ^ 1])
    # 2: the empty set -- every authentic message is outside it; an empty segment under it is SHORT
    first = c.n
    for j in range(5):
        c.msg(c.pick(0, j))
    c.cert(first, 5, 2)
    c.cert(first, 0, 2, quorum=1)
    c.verdict[first + 1] = BAD_RS
    c.cert(first + 1, 3, 2)
    # 3: one entry -- alone it is a quorum of 1; twice it repeats
    first = c.seg(3, 1)
    c.msg(c.pick(3, 0))
    c.cert(first, 2, 3)
    # 4: duplicate rows -- every distinct row once, then one more
    c.seg(4, 9)
    first = c.seg(4, 9)
    offend(c, first + 8, "repeat", first)
    # 5: 4n a power of two, five rows on the last slot
    c.seg(5, 16)
    first = c.seg(5, 16)
    c.frm[first + 7] = last64[5]
    c.pad(0, 3)
    return c


def set_sizes_case(threshold: int, scratch: bool) -> SCase:
    """sets of 1, 4, threshold and threshold + 1 distinct entries in one object; the call names the two
    small ones and the threshold (LDS placement) or all four (scratch placement); the expectations of
    the certificates both calls have are the same"""
    c = SCase([family(10, 1), family(11, 4), family(12, threshold), family(13, threshold + 1)])
    c.pad(2, FIRST)
    for sid in (0, 1, 2) + ((3,) if scratch else ()):
        m = len(c.sets[sid])
        c.seg(sid, min(m, 70))                         # the lowest and the highest entry, and their neighbours
        first = c.seg(sid, min(m, 70))
        if m > 1:
            offend(c, first + min(m, 70) - 1, "repeat", first)   # the lowest entry twice
        first = c.seg(sid, min(m, 70))
        offend(c, first, "nonmember")
        # the same messages under another set of the call (the families are disjoint): all strangers
        c.cert(first, min(m, 70), (sid + 1) % 3)
    c.pad(2, 3)
    return c


def alternating_case(K: int = 3000) -> SCase:
    """K certificates of 5 messages that alternate between two sets of different sizes, adjoining and
    every third one overlapping its neighbour: a block meets both sets in turn on one table"""
    a, b = family(20, 7), family(21, 300)
    c = SCase([a, b + a[:2]])                            # the sets share two rows
    c.pad(0, FIRST)
    for k in range(K):
        sid = k % 2
        first = c.seg(sid, 5, quorum=5, h=H + k % 4, shift=k % 6)
        if k % 10 == 3:
            offend(c, first + 1 + (k // 10) % 3, KINDS[(k // 10) % len(KINDS)], first)
        if k % 3 == 2:                                   # the previous segment's messages under this one's set
            c.cert(first - 5, 10, sid, quorum=5, h=H + k % 4)
    c.pad(1, 3)
    return c


def small_cases() -> Dict[str, SCase]:
    """the cases that run at one size"""
    return {"two_sets": two_sets_case(), "precedence": precedence_case(1400), "verdict_bytes": verdict_bytes_case(),
            "index_edges": index_edges_case()}


# ---- the host program -------------------------------------------------------------
def build_check(sanitize=True):
    """compile tests/native/hd_certsets_check.cpp; sanitize: ASan + UBSan"""
    assert shutil.which("g++"), "g++ is needed for the host check of hd_sigsets.h"
    out = os.path.join(ROOT, "tests", "native", "_build", "hd_certsets_check" + ("_san" if sanitize else ""))
    src = os.path.join(ROOT, "tests", "native", "hd_certsets_check.cpp")
    deps = [src] + [os.path.join(ROOT, "include", f) for f in ("hd_cert.h", "hd_sigsets.h", "hd_verify.h")]
    csrc = os.path.join(ROOT, "hyperdrive_amd", "csrc")
    deps += [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]
    if os.path.exists(out) and all(os.path.getmtime(d) <= os.path.getmtime(out) for d in deps):
        return out
    os.makedirs(os.path.dirname(out), exist_ok=True)
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wno-unused-function", *san, "-o", out, src], check=True)
    return out


def _run(prog, text: str) -> List[List[str]]:
    r = subprocess.run([prog], input=text, capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    return [ln.split() for ln in r.stdout.split("\n") if ln]


def _ids(items) -> Dict[bytes, int]:
    ids: Dict[bytes, int] = {}
    for x in items:
        ids.setdefault(x, len(ids))
    return ids


def run_replay(prog, case: SCase, lds_limit: int, order: int) -> List[Tuple[int, int, int]]:
    """the kernel's sweeps replayed lane by lane over `case` (order: 0 ascending, 1 descending, 2
    scattered lane order); per certificate (status, good, first_bad)"""
    vals = _ids(list(case.value) + [c.value for c in case.certs])
    froms = _ids(case.frm)
    lines = [f"case {case.n} {len(case.sets)} {len(case.certs)} {len(vals)} {len(froms)} {lds_limit} {order}"]
    for s in case.sets:
        lines.append(str(len(s)))
        lines += [row.hex() for row in s]
    lines += [v.hex() for v in vals]
    lines += [f.hex() for f in froms]
    lines += [f"{case.type[i]} {case.height[i]} {case.round[i]} {vals[case.value[i]]} {case.verdict[i]} "
              f"{froms[case.frm[i]]}" for i in range(case.n)]
    lines += [f"{c.first} {c.count} {c.quorum} {c.type} {c.height} {c.round} {vals[c.value]} {sid}"
              for c, sid in zip(case.certs, case.set_of)]
    rows = _run(prog, "\n".join(lines) + "\n")
    assert len(rows) == len(case.certs) and all(r[0] == "c" for r in rows)
    return [(int(r[1]), int(r[2]), int(r[3])) for r in rows]


def run_build(prog, rows: Sequence[bytes], probes: Sequence[bytes]):
    """sigset_build over `rows`: (slots, the sorted distinct rows, the index each input row is found at,
    the index each probe is found at or -1)"""
    text = "\n".join([f"build {len(rows)} {len(probes)}"] + [r.hex() for r in rows] + [p.hex() for p in probes])
    out = _run(prog, text + "\n")
    assert out[0][0] == "b"
    m, slots = int(out[0][1]), int(out[0][2])
    body = out[1:]
    assert [r[0] for r in body] == ["r"] * m + ["i"] * len(rows) + ["q"] * len(probes)
    return (slots, [bytes.fromhex(r[1]) for r in body[:m]], [int(r[1]) for r in body[m:m + len(rows)]],
            [int(r[1]) for r in body[m + len(rows):]])


def run_place(prog, rows_used: int, slots_used: int, n_sets: int, m: int, slots: int):
    """sigset_place: None when refused, else (word_off, slot_off, mask, n)"""
    (row,) = _run(prog, f"place {rows_used} {slots_used} {n_sets} {m} {slots}\n")
    assert row[0] == "l"
    return tuple(int(x) for x in row[2:]) if row[1] == "1" else None
