"""The yardstick of hd_check_certificates (include/hd_cert.h): a Python model of
the segmented check, the synthetic cases the host and the GPU test share, and
the driver of the host replay (tests/native/hd_certcheck_check.cpp).

The model walks each segment in index order, as the header states the
semantics: a message is *not valid* (bitmap bit clear, or signer outside
[0, n_signers)), else *wrong* (type, height, round or value differs), else a
*repeat* (a lower clean message of the segment has its signer), else it counts.
Nothing here calls the library; tests/test_cert_host.py pins the model on
hand-worked segments."""
from __future__ import annotations

import os
import shutil
import subprocess
from dataclasses import dataclass, field
from typing import Dict, List, NamedTuple, Sequence, Tuple

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PREVOTE, PRECOMMIT = 2, 3
OK, SHORT, BAD_SIGNATURE, WRONG_FIELD, REPEATED_SENDER = 0, 1, 2, 3, 4
NEVER = 0xFFFFFFFF
LENGTHS = [0, 1, 63, 64, 65, 255, 256, 257, 1025]
FIRST = 33   # every synthetic segment starts inside a bitmap word


class Cert(NamedTuple):
    first: int
    count: int
    quorum: int
    type: int
    height: int
    round: int
    value: bytes


# ---- the model ------------------------------------------------------------------
def check(certs: Sequence[Cert], types, heights, rounds, values, valid_bits, signers,
          n_signers: int) -> List[Tuple[int, int, int]]:
    """(status, good, first_bad) per certificate"""
    out = []
    for c in certs:
        seen, good, bad, cls = set(), 0, NEVER, OK
        for i in range(c.first, c.first + c.count):
            if not valid_bits[i] or not 0 <= signers[i] < n_signers:
                k = BAD_SIGNATURE
            elif (types[i], heights[i], rounds[i], values[i]) != (c.type, c.height, c.round, c.value):
                k = WRONG_FIELD
            elif signers[i] in seen:
                k = REPEATED_SENDER
            else:
                seen.add(signers[i])
                good += 1
                continue
            if bad == NEVER:
                bad, cls = i, k
        out.append((SHORT if c.count < c.quorum else cls, good, bad))
    return out


# ---- synthetic cases --------------------------------------------------------------
def value(k: int) -> bytes:
    return bytes((37 * k + 11 * j + 1) & 0xFF for j in range(32))


H, R, V = 7, 3, value(0)   # height != round: a compare that reads the wrong column shows


@dataclass
class Case:
    """A batch as columns, and the certificates over it."""
    n_signers: int
    type: List[int] = field(default_factory=list)
    height: List[int] = field(default_factory=list)
    round: List[int] = field(default_factory=list)
    value: List[bytes] = field(default_factory=list)
    valid: List[int] = field(default_factory=list)
    signer: List[int] = field(default_factory=list)
    certs: List[Cert] = field(default_factory=list)

    @property
    def n(self) -> int:
        return len(self.type)

    def sig(self, j: int) -> int:
        """logical signer j -> a table index: even j from the bottom of the table, odd j from its top,
        so that entry n_signers - 1 is used; distinct while j < n_signers"""
        return (j // 2 if j % 2 == 0 else self.n_signers - 1 - j // 2) % max(self.n_signers, 1)

    def msg(self, j: int, t=PRECOMMIT, h=H, r=R, v=V, valid=1) -> int:
        self.type.append(t)
        self.height.append(h)
        self.round.append(r)
        self.value.append(v)
        self.valid.append(valid)
        self.signer.append(self.sig(j))
        return self.n - 1

    def pad(self, k: int) -> None:
        """k messages that would be clean in any segment here, from the signers the segments use: a
        read outside [first, first + count) shows up as a repeat or a wrong count"""
        for j in range(k):
            self.msg(j)

    def seg(self, count: int, quorum=None, t=PRECOMMIT, h=H, r=R, v=V, shift: int = 0) -> int:
        """count clean messages from logical signers shift .. shift + count - 1, and their certificate;
        returns the segment's first index"""
        first = self.n
        for j in range(count):
            self.msg(shift + j, t, h, r, v)
        self.certs.append(Cert(first, count, max(count, 1) if quorum is None else quorum, t, h, r, v))
        return first

    def expected(self):
        return check(self.certs, self.type, self.height, self.round, self.value, self.valid, self.signer,
                     self.n_signers)


def lengths_case(L: int, n_signers: int) -> Case:
    c = Case(n_signers)
    c.pad(FIRST)
    c.seg(L)
    c.pad(5)
    return c


def adjoining_case(n_signers: int) -> Case:
    """two adjoining segments: the last signer of the first is the first signer of the second"""
    c = Case(n_signers)
    c.pad(FIRST)
    c.seg(70)
    c.seg(70, shift=69)
    assert c.signer[FIRST + 69] == c.signer[FIRST + 70]
    return c


def overlap_case(n_signers: int) -> Case:
    """two certificates over one range with different values, and one across both halves of it"""
    c = Case(n_signers)
    c.pad(FIRST)
    first = c.seg(90)
    c.certs.append(Cert(first, 90, 90, PRECOMMIT, H, R, value(1)))
    c.certs.append(Cert(first + 20, 40, 40, PRECOMMIT, H, R, V))
    c.certs.reverse()   # any order
    return c


def _offend(c: Case, i: int, kind: str, against: int = None) -> None:
    if kind == "notvalid":
        c.valid[i] = 0
    elif kind == "type":
        c.type[i] = PREVOTE
    elif kind == "height":
        c.height[i] = R      # the certificate's round, so only a compare of the height column sees it
    elif kind == "round":
        c.round[i] = H
    elif kind == "value":
        c.value[i] = V[:31] + bytes([V[31] ^ 1])   # the last byte only
    elif kind == "value0":
        c.value[i] = bytes([V[0] ^ 0x80]) + V[1:]   # the first byte only
    elif kind == "repeat":
        c.signer[i] = c.signer[against]
    else:
        raise ValueError(kind)


KINDS = ["notvalid", "type", "height", "round", "value", "value0", "repeat"]


def positions_case(n_signers: int, length: int = 130) -> Case:
    """each class at the first index, the last index and indices 63 and 64 of a segment of its own
    (a repeat cannot sit at the first index: it sits at the second, repeating the first)"""
    c = Case(n_signers)
    c.pad(FIRST)
    for kind in KINDS:
        for pos in (0, length - 1, 63, 64):
            first = c.seg(length)
            if kind == "repeat":
                pos = max(pos, 1)
                _offend(c, first + pos, kind, first + pos - 1)
            else:
                _offend(c, first + pos, kind)
    c.pad(3)
    return c


def precedence_case(n_signers: int) -> Case:
    c = Case(n_signers)
    c.pad(FIRST)
    # two offenders of different classes: the lower decides
    for lo, hi in (("value", "notvalid"), ("notvalid", "round"), ("repeat", "notvalid"), ("height", "repeat")):
        first = c.seg(60)
        _offend(c, first + 10, lo, first + 2)
        _offend(c, first + 20, hi, first + 3)
    # not valid and wrong at once: not valid
    first = c.seg(60)
    _offend(c, first + 30, "notvalid")
    _offend(c, first + 30, "value")
    # a repeat whose first occurrence lies 300 messages earlier
    first = c.seg(400)
    _offend(c, first + 350, "repeat", first + 50)
    # a "first occurrence" that is not clean never makes a later message a repeat
    for kind in ("value", "notvalid"):
        first = c.seg(60)
        _offend(c, first + 40, "repeat", first + 5)   # 40 has 5's signer ...
        _offend(c, first + 5, kind)                   # ... but 5 is not clean: 40 counts, 5 is the offender
    # the not-clean message is the later one: the earlier one counts, the later is classed by its own fault
    first = c.seg(60)
    _offend(c, first + 40, "repeat", first + 5)
    _offend(c, first + 40, "round")
    # three messages of one signer: the two later ones are repeats, the lowest of them is named
    first = c.seg(200)
    _offend(c, first + 150, "repeat", first + 9)
    _offend(c, first + 77, "repeat", first + 9)
    # count >= quorum decides SHORT, not good: an offender leaves good below quorum, still its own class
    first = c.seg(10, quorum=10)
    _offend(c, first + 4, "notvalid")
    # SHORT wins over every class, and good / first_bad are still filled
    first = c.seg(10, quorum=11)
    _offend(c, first + 4, "value")
    return c


def signer_filter_case(n_signers: int) -> Case:
    """signer -1, n_signers and far outside on a set bit: BAD_SIGNATURE, no table access"""
    c = Case(n_signers)
    c.pad(FIRST)
    for bad in (-1, n_signers, n_signers + 1, -(1 << 31), (1 << 31) - 1):
        first = c.seg(min(66, n_signers))
        c.signer[first + min(64, n_signers - 1)] = bad
    return c


def small_table_case() -> Case:
    """n_signers 4: every segment holds at most four distinct signers"""
    c = Case(4)
    c.pad(FIRST)
    c.seg(4)
    c.seg(3, quorum=3, shift=1)
    first = c.seg(4)
    _offend(c, first + 3, "repeat", first)
    first = c.seg(4)
    c.signer[first + 2] = 4
    c.seg(0, quorum=1)
    return c


def many_small_case(n_signers: int, K: int = 5000) -> Case:
    """K certificates of 3 messages, every tenth with one offender of a rotating kind"""
    c = Case(n_signers)
    c.pad(FIRST)
    for k in range(K):
        first = c.seg(3, quorum=3, h=H + k % 5, shift=k % 7)
        if k % 10 == 0:
            _offend(c, first + 1 + (k // 10) % 2, KINDS[(k // 10) % len(KINDS)], first)
    return c


def large_case(n_signers: int, count: int = 100000) -> Case:
    """one certificate of `count` messages.  With n_signers >= count every signer is distinct but one,
    which repeats once; with fewer signatories than messages the signers go round (i mod n_signers),
    so message n_signers is the first repeat and good is n_signers."""
    c = Case(n_signers)
    c.pad(FIRST)
    first = c.n
    for j in range(count):
        c.msg(j % n_signers)
    c.certs.append(Cert(first, count, 1, PRECOMMIT, H, R, V))
    if n_signers >= count:
        _offend(c, first + 90001, "repeat", first + 17)
    c.pad(2)
    return c


def table_cases(n_signers: int) -> Dict[str, Case]:
    """the cases run at every table placement"""
    return {"adjoining": adjoining_case(n_signers), "overlap": overlap_case(n_signers),
            "positions": positions_case(n_signers), "precedence": precedence_case(n_signers),
            "signer_filter": signer_filter_case(n_signers)}


# ---- the host program -------------------------------------------------------------
def build_check(sanitize=True):
    """compile tests/native/hd_certcheck_check.cpp; sanitize: ASan + UBSan"""
    assert shutil.which("g++"), "g++ is needed for the host check of hd_certcheck.h"
    out = os.path.join(ROOT, "tests", "native", "_build", "hd_certcheck_check" + ("_san" if sanitize else ""))
    src = os.path.join(ROOT, "tests", "native", "hd_certcheck_check.cpp")
    deps = [src, os.path.join(ROOT, "include", "hd_cert.h"), os.path.join(ROOT, "include", "hd_verify.h")]
    deps += [os.path.join(ROOT, "hyperdrive_amd", "csrc", f) for f in ("hd_certcheck.h", "hd_common.h")]
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


def run_replay(prog, case: Case, lds_limit: int, order: int) -> List[Tuple[int, int, int]]:
    """the kernel's sweeps replayed lane by lane over `case` (order: 0 ascending, 1 descending, 2
    scattered lane order); per certificate (status, good, first_bad)"""
    vals: Dict[bytes, int] = {}
    for v in list(case.value) + [c.value for c in case.certs]:
        vals.setdefault(v, len(vals))
    lines = [f"case {case.n} {case.n_signers} {len(case.certs)} {len(vals)} {lds_limit} {order}"]
    lines += [v.hex() for v in vals]
    lines += [f"{case.type[i]} {case.height[i]} {case.round[i]} {vals[case.value[i]]} {case.valid[i]} {case.signer[i]}"
              for i in range(case.n)]
    lines += [f"{c.first} {c.count} {c.quorum} {c.type} {c.height} {c.round} {vals[c.value]}" for c in case.certs]
    rows = _run(prog, "\n".join(lines) + "\n")
    assert len(rows) == len(case.certs) and all(r[0] == "c" for r in rows)
    return [(int(r[1]), int(r[2]), int(r[3])) for r in rows]


def run_plan(prog, n_signers: int, K: int, lds_limit: int) -> dict:
    (row,) = _run(prog, f"plan {n_signers} {K} {lds_limit}\n")
    assert row[0] == "p"
    keys = ["in_lds", "blocks", "lds_bytes", "lds_entries", "slice_bytes", "scratch_bytes", "guide_limit", "own",
            "grid_lds", "grid_scratch", "scratch_cap"]
    return dict(zip(keys, (int(x) for x in row[1:])))


def run_row_ok(prog, rows) -> List[bool]:
    """rows: [(first, count, quorum, type, r0, r1, r2, n)] -> cert_row_ok"""
    out = _run(prog, "".join("rowok %d %d %d %d %d %d %d %d\n" % tuple(r) for r in rows))
    return [r[1] == "1" for r in out]
