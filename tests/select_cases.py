"""The yardstick of hd_log_select (include/hd_log.h): a Python model of the
keyed read and the logs both tests of it use.

The model filters the ``kept`` list of ``evidence_cases.Kept`` -- the 154-byte
rows by log position, each with signature bytes of its own -- with the same
predicate, position range and limit as the call: the entries of the asked types
whose round lies in the range and whose value and From equal the asked ones, in
ascending position, the first ``limit`` of them.  Nothing here calls the
library; tests/test_select_host.py pins the model on hand-worked logs and runs
the kernel's rank arithmetic (hyperdrive_amd/csrc/hd_logselect.h) on the host
against it, over the same match patterns the GPU test builds its logs from."""
from __future__ import annotations

import os
import random
import shutil
import struct
import subprocess
from typing import List, Optional, Sequence, Tuple

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROPOSE, PREVOTE, PRECOMMIT = 1, 2, 3
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 513, 1025]


# ---- the model ----------------------------------------------------------------
def fields(row: bytes):
    """(type, height, round, valid_round, value, From, signature) of a 154-byte row"""
    assert len(row) == 154
    h, r, vr = struct.unpack("<qqq", row[1:25])
    return row[0], h, r, vr, row[25:57], row[57:89], row[89:]


def matches(row: bytes, types: Sequence[int], round_lo: int, round_hi: int, value: Optional[bytes],
            sender: Optional[bytes]) -> bool:
    t, _, r, _, v, frm, _ = fields(row)
    return (t in types and round_lo <= r <= round_hi and (value is None or v == value)
            and (sender is None or frm == sender))


def select(kept: Sequence[bytes], types, round=None, value=None, sender=None, first: int = 0,
           upto: Optional[int] = None, limit: int = 0) -> Tuple[List[int], int]:
    """(positions returned, total): the arguments of DecideLog.select -- ``round`` None, r or (lo, hi);
    positions first .. upto, both inclusive."""
    types = (types,) if isinstance(types, int) else tuple(types)
    lo, hi = (I64_MIN, I64_MAX) if round is None else (round if isinstance(round, tuple) else (round, round))
    end = len(kept) if upto is None else min(upto + 1, len(kept))
    pos = [q for q in range(first, end) if matches(kept[q], types, lo, hi, value, sender)]
    return (pos[:limit] if limit else pos), len(pos)


def select_flags(flags: Sequence[bool], pos_lo: int, pos_hi: int, limit: int) -> Tuple[List[int], int]:
    """the same over a table of match bits and the C range [pos_lo, pos_hi)"""
    pos = [q for q in range(pos_lo, min(pos_hi, len(flags))) if flags[q]]
    return (pos[:limit] if limit else pos), len(pos)


# ---- match patterns -----------------------------------------------------------
def patterns(L: int):
    """name -> L match bits: the tables at which rank and bounds can go wrong.  A pattern that needs a
    position the log does not have keeps what fits (lanes 63 and 64 of a log of 64 entries: lane 63)."""
    rng = random.Random(1000 + L)
    at = lambda ps: [q in ps for q in range(L)]
    return {
        "none": [False] * L,
        "every": [True] * L,
        "first": at({0}),
        "last": at({L - 1}),
        "lanes_63_64": at({63, 64}),
        "positions_255_256": at({255, 256}),
        "every_64th": [q % 64 == 0 for q in range(L)],
        "random": [rng.random() < 0.3 for _ in range(L)],
    }


# ---- logs -----------------------------------------------------------------------
def sender(k: int) -> bytes:
    import hd_pyoracle as O
    return O.sha256(b"hd-select-sender" + struct.pack(">I", k))


def pattern_log(O, height: int, flags: Sequence[bool], mode: str, v: bytes, w: bytes, special: bytes):
    """An oracle batch of len(flags) votes that are all logged, from 4 senders over many rounds (8 entries
    a round: 4 senders x prevote, precommit), with entry q matching exactly when flags[q]:
      mode "value":  a matching entry carries value w, every other v     (filter: value = w)
      mode "from":   a matching entry is signed by `special`, in a round of its own, 10,000 + q
                     (filter: sender = special)
      mode "type":   a matching entry is a precommit, every other a prevote; each in a round of its
                     own (filter: types = precommit)
      mode "round":  a matching entry lies in rounds 5,000 .. 5,000 + L, every other below
                     (filter: round = (5000, 5000 + L))"""
    import evidence_cases as EC
    ob = O.Batch()
    for q, m in enumerate(flags):
        t, r, val, frm = (PREVOTE if q % 2 == 0 else PRECOMMIT), q // 8, v, sender(q // 2 % 4)
        if mode == "value":
            val = w if m else v
        elif mode == "from":
            if m:
                frm, r = special, 10000 + q
        elif mode == "type":
            t, r = (PRECOMMIT if m else PREVOTE), q
        elif mode == "round":
            if m:
                r = 5000 + q // 8
        else:
            raise ValueError(mode)
        ob.append(t, height, r, -1, val, frm, bytes(65))
    return EC.unique_sigs(ob, b"p" + mode.encode())


def pattern_query(mode: str, L: int, w: bytes, special: bytes) -> dict:
    """the select arguments that match exactly the flagged entries of pattern_log"""
    return {"value": dict(types=(PREVOTE, PRECOMMIT), value=w),
            "from": dict(types=(PREVOTE, PRECOMMIT), sender=special),
            "type": dict(types=PRECOMMIT),
            "round": dict(types=(PREVOTE, PRECOMMIT), round=(5000, 5000 + L))}[mode]


# ---- the host program ---------------------------------------------------------
def build_check(sanitize=True):
    """compile tests/native/hd_logselect_check.cpp; sanitize: ASan + UBSan"""
    assert shutil.which("g++"), "g++ is needed for the host check of hd_logselect.h"
    out = os.path.join(ROOT, "tests", "native", "_build", "hd_logselect_check" + ("_san" if sanitize else ""))
    src = os.path.join(ROOT, "tests", "native", "hd_logselect_check.cpp")
    deps = [src, os.path.join(ROOT, "include", "hd_log.h"), os.path.join(ROOT, "include", "hd_verify.h")]
    deps += [os.path.join(ROOT, "hyperdrive_amd", "csrc", f) for f in ("hd_logselect.h", "hd_common.h")]
    if os.path.exists(out) and all(os.path.getmtime(d) <= os.path.getmtime(out) for d in deps):
        return out
    os.makedirs(os.path.dirname(out), exist_ok=True)
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wno-unused-function", *san, "-o", out, src], check=True)
    return out


def _run(prog, lines: List[str], tag: str) -> List[List[str]]:
    r = subprocess.run([prog], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    rows = [ln.split() for ln in r.stdout.split("\n") if ln]
    assert len(rows) == len(lines) and all(row[0] == tag for row in rows)
    return [row[1:] for row in rows]


def run_rank(prog, cases) -> List[Tuple[List[int], int, int]]:
    """cases: [(flags, pos_lo, pos_hi, limit, cap)]; per case (positions stored, total, n) of the replay"""
    lines = []
    for flags, lo, hi, limit, cap in cases:
        bits = "".join("1" if m else "0" for m in flags) or "-"
        lines.append(f"rank {len(flags)} {lo} {hi} {limit} {cap} {bits}")
    return [([int(t) for t in row[2:]], int(row[0]), int(row[1])) for row in _run(prog, lines, "r")]


def run_match(prog, cases) -> List[bool]:
    """cases: [((type_mask, flags, round_lo, round_hi, value, from), (type, round, value, from))]"""
    lines = []
    for (mask, fl, rlo, rhi, fv, ff), (t, r, ev, ef) in cases:
        lines.append(f"match {mask} {fl} {rlo} {rhi} {fv.hex()} {ff.hex()} {t} {r} {ev.hex()} {ef.hex()}")
    return [row[0] == "1" for row in _run(prog, lines, "m")]


def run_filter(prog, cases) -> List[bool]:
    """cases: [(type_mask, flags, reserved)] -> log_filter_ok"""
    return [row[0] == "1" for row in _run(prog, [f"filter {m} {f} {r}" for m, f, r in cases], "f")]
