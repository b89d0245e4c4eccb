"""Cases of the consume into device memory (include/hd_mq.h
hd_mq_consume_device), shared by the host test (test_mqtake_host.py) and the
GPU test (test_gpu_mq_device.py).

Two things live here, and neither calls the library:

* the locate of a delivered row's sender: a model written from the contract
  ("row k belongs to the k-th delivered message in sender order"),
  independent of hyperdrive_amd/csrc/hd_mqtake.h, and the driver of the
  stand-alone host program tests/native/hd_mqtake_check.cpp;

* the scenario table of the GPU test, built from seeds.  ``check`` asserts
  with oracle/mq_oracle.py alone that each scenario meets the condition it is
  named for (the delivered count, removed > delivered, where the proposes
  sit), so a scenario cannot silently stop covering its edge."""
import functools
import hashlib
import os
import shutil
import subprocess

import numpy as np

from mq_oracle import MessageQueue as OracleMQ

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROPOSE, PREVOTE, PRECOMMIT = 1, 2, 3
H = 7                       # the height every scenario consumes first
LATER = (H + 1, H + 3)      # and the later heights consumed after it


# ---- the locate ---------------------------------------------------------------
def offsets(counts):
    """the plan's off[]: delivered rows of the senders before each sender"""
    off, t = [], 0
    for c in counts:
        off.append(t)
        t += c
    return off


def locate_model(counts, k):
    """the sender of delivered row k: rows are laid out sender by sender"""
    return [s for s, c in enumerate(counts) for _ in range(c)][k]


def edge_rows(counts):
    """the first and the last row of every sender that delivers"""
    ks = []
    for o, c in zip(offsets(counts), counts):
        if c:
            ks += [o, o + c - 1]
    return sorted(set(ks))


def build_check(sanitize=True):
    """compile tests/native/hd_mqtake_check.cpp; sanitize: ASan + UBSan"""
    assert shutil.which("g++"), "g++ is needed for the host check of hd_mqtake.h"
    out = os.path.join(ROOT, "tests", "native", "_build", "hd_mqtake_check" + ("_san" if sanitize else ""))
    src = os.path.join(ROOT, "tests", "native", "hd_mqtake_check.cpp")
    deps = [src] + [os.path.join(ROOT, "hyperdrive_amd", "csrc", f) for f in ("hd_mqtake.h", "hd_common.h")]
    if os.path.exists(out) and all(os.path.getmtime(d) <= os.path.getmtime(out) for d in deps):
        return out
    os.makedirs(os.path.dirname(out), exist_ok=True)
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wno-unused-function", *san, "-o", out, src], check=True)
    return out


def run_check(prog, cases):
    """cases: [(counts, rows)]; returns per case the senders the host program located"""
    lines = []
    for counts, ks in cases:
        lines.append(f"case {len(counts)} {len(ks)}")
        lines.append(" ".join(str(o) for o in offsets(counts)))
        lines.append(" ".join(str(k) for k in ks))
    r = subprocess.run([prog], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    rows = [ln.split() for ln in r.stdout.split("\n") if ln]
    assert len(rows) == len(cases) and all(row[0] == "s" for row in rows)
    return [[int(t) for t in row[1:]] for row in rows]


# ---- scenarios ----------------------------------------------------------------
def sender(name, k):
    """a From: 32 bytes that sort in no relation to k"""
    return hashlib.sha256(b"hd-mq-device" + name.encode() + int(k).to_bytes(4, "big")).digest()


class Scenario:
    """batches: [[row, ...], ...] in arrival order, a row being the oracle's
    message (height, round, type, valid_round, value32, from32, sig65);
    vr_null: the batches go in without a valid_round column (rows hold -1);
    allowed: procsAllowed as a list of Froms, or None for the admitted set,
    which is then `admitted`; expect: the conditions `check` asserts."""

    def __init__(self, name, capacity, batches, allowed, admitted, vr_null, expect):
        self.name, self.capacity, self.batches = name, capacity, batches
        self.allowed, self.admitted, self.vr_null, self.expect = allowed, admitted, vr_null, expect

    def allowed_set(self):
        return set(self.admitted if self.allowed is None else self.allowed)

    def oracle(self):
        q = OracleMQ(self.capacity)
        for rows in self.batches:
            for m in rows:
                q.insert(m[5], m)
        return q


def sender_ids(q):
    """From -> sender-queue id (creation order)"""
    return {frm: k for k, frm in enumerate(q.queues)}


def _order(rng, n_allowed, n_other):
    """creation order, True = allowed: not-allowed senders first and last, a
    run of two in the middle, the rest anywhere"""
    order = [True] * n_allowed
    left = n_other
    if left >= 4 and n_allowed >= 2:
        mid = n_allowed // 2
        order[mid:mid] = [False, False]
        left -= 2
    for _ in range(max(left - 2, 0)):
        order.insert(int(rng.integers(0, len(order) + 1)), False)
    if left >= 1:
        order.insert(0, False)
    if left >= 2:
        order.append(False)
    return order


def _split(rng, total, parts):
    """total rows over `parts` senders; with three or more, the last gets none
    (the not-allowed run in the middle then lies between two that deliver)"""
    if parts == 0:
        return []
    w = rng.random(parts) + 0.05
    if parts >= 3:
        w[parts - 1] = 0.0
    c = np.floor(w / w.sum() * total).astype(int)
    c[int(np.argmax(w))] += total - int(c.sum())
    return [int(x) for x in c]


def _make(name, seed, n_deliver=0, n_allowed=0, n_other=0, proposes="any", vr_null=False, admitted=False,
          one_each=0, capacity=8192):
    rng = np.random.default_rng(seed)
    blob = lambda k: rng.integers(0, 256, k, dtype=np.uint8).tobytes()
    typ = lambda: int(rng.integers(1, 4)) if proposes == "any" else int(rng.integers(2, 4))
    vr = lambda: -1 if vr_null else int(rng.integers(-1, 3))
    row = lambda h, r, frm: [int(h), int(r), typ(), vr(), blob(32), frm, blob(65)]
    if one_each:                                   # one message per sender, every third sender not allowed
        order = [k % 3 != 1 for k in range(one_each)]
        froms = [sender(name, k) for k in range(one_each)]
        rows = [row(H, rng.integers(0, 3), f) for f in froms]
        batches = [rows[: one_each // 2], rows[one_each // 2:]]
        n_deliver = sum(order)
    else:
        order = _order(rng, n_allowed, n_other)
        froms = [sender(name, k) for k in range(len(order))]
        first = [row(H + 1, 0, f) for f in froms]  # arrival order of these = creation order
        rest = []
        counts = iter(_split(rng, n_deliver, n_allowed))
        for ok, f in zip(order, froms):
            below = next(counts) if ok else int(rng.integers(1, 6))   # removed, and delivered when allowed
            rest += [row(rng.choice([H - 2, H - 1, H]), rng.integers(0, 4), f) for _ in range(below)]
            rest += [row(rng.choice([H + 1, H + 2, H + 3]), rng.integers(0, 3), f)
                     for _ in range(int(rng.integers(1, 4)))]
        rest = [rest[i] for i in rng.permutation(len(rest))]
        cut = int(rng.integers(0, len(rest) + 1))
        batches = [first + rest[:cut], rest[cut:]] if froms else []
    allowed = [f for ok, f in zip(order, froms) if ok]
    sc = Scenario(name, capacity, batches, None if admitted else allowed, allowed if admitted else None, vr_null,
                  dict(deliver=n_deliver, senders=len(order), more_removed=not all(order), proposes=proposes))
    # the proposes go where the scenario's name says, by the oracle's order
    if proposes in ("first", "last", "two"):
        _, out = sc.oracle().consume(H, sc.allowed_set())
        got = [m for _, m in out]
        if proposes == "two":
            at_h = [m for m in got if m[0] == H]
            pair = next((a, b) for i, a in enumerate(at_h) for b in at_h[i + 1:] if a[1] == b[1] and a[5] != b[5])
            for m in pair:
                m[2] = PROPOSE
        else:
            got[0 if proposes == "first" else -1][2] = PROPOSE
    sc.batches = [[tuple(m) for m in rows] for rows in sc.batches]
    return sc


TABLE = [
    ("empty", dict()),
    ("none_allowed", dict(n_other=3)),
    ("d1", dict(n_deliver=1, n_allowed=3, n_other=4)),
    ("d63", dict(n_deliver=63, n_allowed=3, n_other=4)),
    ("d64", dict(n_deliver=64, n_allowed=3, n_other=4)),
    ("d65", dict(n_deliver=65, n_allowed=3, n_other=4)),
    ("d255", dict(n_deliver=255, n_allowed=3, n_other=4)),
    ("d257", dict(n_deliver=257, n_allowed=3, n_other=4)),
    ("d4097", dict(n_deliver=4097, n_allowed=24, n_other=13)),    # past HD_MQ_STAGE_ROWS
    ("one_sender", dict(n_deliver=65, n_allowed=1)),
    ("three_senders", dict(n_deliver=130, n_allowed=3)),
    ("s1025", dict(one_each=1025)),                                 # the twin's multi-block host path
    ("vr_null", dict(n_deliver=70, n_allowed=3, n_other=4, vr_null=True)),
    ("p_none", dict(n_deliver=130, n_allowed=3, n_other=4, proposes="none")),
    ("p_first", dict(n_deliver=130, n_allowed=3, n_other=4, proposes="first")),
    ("p_last", dict(n_deliver=130, n_allowed=3, n_other=4, proposes="last")),
    ("p_two", dict(n_deliver=130, n_allowed=3, n_other=4, proposes="two")),
    ("window", dict(n_deliver=90, n_allowed=5, n_other=4, admitted=True)),
]
NAMES = [name for name, _ in TABLE]
DELIVERY = [n for n in NAMES if n != "window"]            # case 1 of the GPU test
PROPOSES = ["p_none", "p_first", "p_last", "p_two", "d257"]


@functools.lru_cache(maxsize=None)
def scenario(name):
    k = NAMES.index(name)
    return _make(name, 1000 + k, **TABLE[k][1])


def run_oracle(sc, heights=(H,) + LATER):
    """[(removed, [(sender id, row)], messages left)] for a consume of each
    height in turn, with the scenario's procsAllowed"""
    q = sc.oracle()
    ids = sender_ids(q)
    out = []
    for h in heights:
        n, got = q.consume(h, sc.allowed_set())
        out.append((n, [(ids[s], m) for s, m in got], len(q)))
    return out


def check(sc):
    """the scenario covers the edge it is named for (mq_oracle alone)"""
    e = sc.expect
    q = sc.oracle()
    assert len(q.queues) == e["senders"]
    total = len(q)
    (removed, got, left), *later = run_oracle(sc)
    assert len(got) == e["deliver"], (sc.name, len(got), e["deliver"])
    assert left == total - removed
    if e["more_removed"]:
        assert removed > len(got), sc.name                    # procsAllowed dropped messages
    else:
        assert removed == len(got)
    if got:
        assert len(got) < 60 or sc.name == "s1025" or min(m[0] for _, m in got) < H   # heights below h too
        ids = [s for s, _ in got]
        assert ids == sorted(ids)                               # sender queues in creation order
    if e["senders"] and sc.name != "s1025":
        assert sum(n for n, _, _ in later) > 0                 # something is left for the later consumes
    if e["more_removed"] and e["deliver"]:
        # offsets repeat: some sender between two delivering ones delivers nothing
        ids = sorted({s for s, _ in got})
        assert any(b - a > 1 for a, b in zip(ids, ids[1:])) or e["deliver"] == 1
    where = [k for k, (_, m) in enumerate(got) if m[2] == PROPOSE]
    if e["proposes"] == "none":
        assert where == []
    elif e["proposes"] == "first":
        assert where == [0]
    elif e["proposes"] == "last":
        assert where == [len(got) - 1]
    elif e["proposes"] == "two":
        a, b = where
        assert got[a][1][:2] == got[b][1][:2] and got[a][0] != got[b][0]    # one round, two senders
    if sc.vr_null:
        assert all(m[3] == -1 for rows in sc.batches for m in rows)
    return removed, got
