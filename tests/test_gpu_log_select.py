"""hd_log_select and hd_log_select_device (include/hd_log.h; DecideLog.select,
count, select_device, proposal, votes, vote_of, certificate and
quorum.check_certificate) against the model of tests/select_cases.py, which
filters the host copy of the log (evidence_cases.Kept) with the same predicate,
range and limit.  Every comparison is exact, on the positions and on all 154
bytes of a row; every message carries signature bytes of its own, so a row
gathered from the wrong place cannot compare equal.  Verdicts are passed
directly except in the certificate case, which needs real signatures.
tests/test_select_host.py pins the model and runs the kernels' rank arithmetic
on the host over the same match patterns."""
import ctypes
import struct

import numpy as np
import pytest

import catch_cases as CC
import evidence_cases as EC
import log_cases as LC
import select_cases as SC
from util import to_np

pytestmark = pytest.mark.gpu

H = 5
P, V, C = SC.PROPOSE, SC.PREVOTE, SC.PRECOMMIT
VOTES = (V, C)


@pytest.fixture(scope="module")
def verifier(gpu, oracle):
    v = gpu.Verifier(0)
    v.set_signatories(_rows([oracle.sha256(b"g" + bytes([k])) for k in range(6)]))   # the senders here: outside it
    yield v
    v.close()


def _rows(sigs):
    return np.frombuffer(b"".join(sigs), np.uint8).reshape(len(sigs), 32).copy()


def _batch(O, msgs, tag=b"s"):
    ob = O.Batch()
    for m in msgs:
        ob.append(*m, bytes(65))
    return EC.unique_sigs(ob, tag)


class Pair:
    """A library log that keeps signatures and the model fed side by side, every insert with evidence
    (as tests/test_gpu_log_evidence.py feeds its pairs)."""

    def __init__(self, verifier, O, height, f, keep=True, max_entries=0):
        self.O = O
        self.log = verifier.open_log(height, f, None, max_entries=max_entries, keep_signatures=keep)
        self.ys = EC.Kept(height, f, None)

    def put(self, ob, value_ok=None):
        verdicts = [self.O.VALID] * len(ob)
        res = self.log.insert(to_np(ob), np.array(verdicts, np.uint8),
                              None if value_ok is None else np.array(value_ok, np.uint8), catch=True, evidence=True)
        exp, recs, ev = self.ys.push(ob, verdicts, value_ok)
        LC.same_insert(res, exp)
        CC.same_caught(res, recs)
        EC.same_evidence(res, ev)
        assert self.log.entries == self.ys.entries == res.base + res.kept
        return res

    def same_log(self):
        b, ok = self.log.read()
        assert EC.rows(b) == self.ys.kept and ok.tolist() == self.ys.kept_ok

    def same(self, types, **q):
        """log.select(types, **q) == the model's, positions and whole rows; the count-only form and the
        positions-only form agree"""
        sel = self.log.select(types, **q)
        same_selection(sel, self.ys.kept, self.ys.kept_ok, *SC.select(self.ys.kept, types, **q))
        bare = self.log.select(types, rows=False, **q)
        assert bare.positions.tolist() == sel.positions.tolist() and bare.total == sel.total and bare.batch is None
        q.pop("limit", None)
        assert self.log.count(types, **q) == sel.total
        return sel

    def reset(self, height):
        self.log.reset(height)
        self.ys = EC.Kept(height, self.ys.cs.ys.f, None)

    def close(self):
        self.log.close()


def same_selection(sel, kept, kept_ok, want_pos, want_total):
    assert sel.positions.tolist() == want_pos, (sel.positions.tolist()[:8], want_pos[:8])
    assert sel.total == want_total and len(sel) == len(want_pos)
    assert EC.rows(sel.batch) == [kept[q] for q in want_pos]
    assert sel.value_ok.tolist() == [kept_ok[q] for q in want_pos]


@pytest.fixture
def pair(verifier, oracle):
    made = []

    def make(height=H, f=1, keep=True, max_entries=0):
        made.append(Pair(verifier, oracle, height, f, keep, max_entries))
        return made[-1]

    yield make
    for p in made:
        p.close()


def _values(O):
    return O.canonical_value(H, 0), O.canonical_value(H, 1), SC.sender(99)


def _pattern_pair(p, O, flags, mode):
    """p reset and holding pattern_log(flags, mode); the query that matches the flagged entries"""
    v, w, special = _values(O)
    p.reset(H)
    L = len(flags)
    ob = SC.pattern_log(O, H, flags, mode, v, w, special)
    res = p.put(ob, value_ok=[q % 5 != 0 for q in range(L)])
    assert res.kept == L == p.log.entries
    return SC.pattern_query(mode, L, w, special)


def _raw_select(log, flt, cap, rows=True, sig=True, pos=True, rows_cap=None):
    """hd_log_select through the C ABI: (rc, hd_log_selected, positions, hd_log_rows, its arrays)"""
    from hyperdrive_amd import _lib
    from hyperdrive_amd.verify import _rows_struct
    r, a = _rows_struct(cap if rows_cap is None else rows_cap, sig)
    p = np.full(max(cap, 1) + 4, 0xDEADBEEF, np.uint32)                # four guard words behind cap
    sel = _lib.HdLogSelected(77, 77)
    rc = _lib.load().hd_log_select(log.handle, ctypes.byref(flt) if flt is not None else None,
                                   p.ctypes.data if pos else None, cap, ctypes.byref(r) if rows else None,
                                   ctypes.byref(sel))
    return rc, sel, p, r, a


def _filter(log, types, **q):
    a = dict(round=None, value=None, sender=None, first=0, upto=None, limit=0)
    a.update(q)
    return log._filter(types, **a)


# ---- 1. log sizes around wavefront and block boundaries ---------------------------------
@pytest.mark.parametrize("L", SC.SIZES)
def test_sizes_and_patterns(verifier, oracle, pair, L):
    """Every pattern of select_cases.patterns -- no match, every entry, position 0 alone, position L - 1
    alone, lanes 63 and 64, positions 255 and 256, every 64th, seeded random -- as a log whose entries'
    values say which ones match; the random pattern also by From, by type and by round."""
    p = pair()
    for name, flags in SC.patterns(L).items():
        for mode in (("value", "from", "type", "round") if name == "random" else ("value",)):
            q = _pattern_pair(p, oracle, flags, mode)
            types = q.pop("types")
            sel = p.same(types, **q)
            assert sel.positions.tolist() == [k for k in range(L) if flags[k]], (name, mode)
    # every entry, whatever its key
    assert p.same((P, V, C)).total == L


# ---- 2. each filter field alone, all together, near misses ------------------------------
def test_filter_fields_and_near_misses(verifier, oracle, pair):
    O = oracle
    v, w, _ = _values(O)
    a, b = SC.sender(0), SC.sender(1)
    flip = lambda x, k: x[:k] + bytes([x[k] ^ 1]) + x[k + 1:]
    msgs = [(V, H, 7, -1, v, a),                                       # 0: the entry every query below is after
            (V, H, 7, -1, flip(v, 31), b), (V, H, 7, -1, flip(v, 0), SC.sender(2)),
            (V, H, 7, -1, v, flip(a, 31)), (V, H, 7, -1, v, flip(a, 0)),
            (V, H, 6, -1, v, a), (V, H, 8, -1, v, a),                  # round - 1, round + 1
            (P, H, 7, -1, v, a),                                       # 7: a propose with the vote's value and From
            (C, H, 7, -1, v, a), (C, H, 7, -1, w, b),
            (V, H, SC.I64_MAX, -1, v, a), (V, H, SC.I64_MIN, -1, v, a),
            (C, H, SC.I64_MAX - 1, -1, v, a), (C, H, SC.I64_MIN + 1, -1, v, a), (V, H, -1, -1, v, a), (V, H, 0, -1, v, a)]
    ob = _batch(O, msgs)
    p = pair()
    res = p.log.insert(to_np(ob), np.zeros(len(ob), np.uint8))
    assert res.kept == len(ob) and res.logpos.tolist() == list(range(len(ob)))
    p.ys.kept = [EC.row(ob, i) for i in range(len(ob))]
    p.ys.kept_ok = [1] * len(ob)
    p.same_log()
    # all fields together: the one entry, none of its near misses
    assert p.same(V, round=7, value=v, sender=a).positions.tolist() == [0]
    assert p.same(VOTES, round=7, value=v, sender=a).positions.tolist() == [0, 8]      # not the propose at 7
    assert p.same((P, V, C), round=7, value=v, sender=a).positions.tolist() == [0, 7, 8]
    # each field alone
    assert p.same(P).positions.tolist() == [7]
    assert p.same(C).positions.tolist() == [8, 9, 12, 13]
    assert p.same(VOTES, round=7).positions.tolist() == [0, 1, 2, 3, 4, 8, 9]
    assert p.same(VOTES, value=v).positions.tolist() == [0, 3, 4, 5, 6, 8, 10, 11, 12, 13, 14, 15]
    assert p.same(VOTES, sender=a).positions.tolist() == [0, 5, 6, 8, 10, 11, 12, 13, 14, 15]
    for near in (flip(v, 31), flip(v, 0)):
        assert len(p.same(VOTES, value=near)) == 1
    for near in (flip(a, 31), flip(a, 0)):
        assert len(p.same(VOTES, sender=near)) == 1
    assert p.same(VOTES, value=flip(v, 15)).total == 0
    # rounds: the neighbours, ranges, the int64 extremes
    assert p.same(V, round=6).positions.tolist() == [5] and p.same(V, round=8).positions.tolist() == [6]
    assert p.same(V, round=(6, 8), sender=a).positions.tolist() == [0, 5, 6]
    assert p.same(VOTES, round=(8, 6)).total == 0
    assert p.same(VOTES, round=SC.I64_MAX).positions.tolist() == [10]
    assert p.same(VOTES, round=SC.I64_MIN).positions.tolist() == [11]
    assert p.same(VOTES, round=(SC.I64_MIN + 1, SC.I64_MAX - 1)).total == 13
    assert p.same(VOTES, round=(SC.I64_MIN, -1)).positions.tolist() == [11, 13, 14]
    assert p.same(VOTES, round=(SC.I64_MAX - 1, SC.I64_MAX)).positions.tolist() == [10, 12]
    assert p.same((P, V, C)).total == len(ob)


# ---- 3. limit, 4. pos_lo / pos_hi -------------------------------------------------------
def test_limits_and_position_ranges(verifier, oracle, pair):
    O = oracle
    L = 1025
    p = pair()
    for name in ("every", "random"):
        flags = SC.patterns(L)[name]
        q = _pattern_pair(p, O, flags, "value")
        types = q.pop("types")
        total = sum(flags)
        # the cut inside a wavefront, at a wavefront boundary, at a block boundary; 1; at and past the total
        for limit in (1, 3, 63, 64, 65, 128, 255, 256, 257, total - 1, total, total + 1, 100000):
            sel = p.same(types, limit=limit, **q)
            assert sel.total == total and len(sel) == min(limit, total)
        # ranges mid-wavefront and at block edges; upto beyond the log is clipped; first at or past L is empty
        for first in (0, 37, 64, 255, 256, 257, 1024):
            for upto in (36, 63, 255, 256, 1023, 1024, 5000, None):
                p.same(types, first=first, upto=upto, **q)
                p.same(types, first=first, upto=upto, limit=5, **q)
        for first in (L, L + 1, 0xFFFFFFFF):
            assert p.same(types, first=first, **q).total == 0
        assert p.same(types, upto=-1, **q).total == 0


# ---- 5. more than 256 blocks ------------------------------------------------------------
def test_more_than_256_blocks(verifier, oracle):
    """65,836 votes of 2,000 senders outside the admitted set: message k is from sender k mod 2,000, a
    prevote or a precommit of round k div 4,000; the last 36 carry another value.  Every key is its own,
    so every message is kept in order and the expected rows are the batch's."""
    from hyperdrive_amd.verify import Batch
    O = oracle
    n, S = 65536 + 300, 2000
    v, w, _ = _values(O)
    senders = [SC.sender(1000 + k) for k in range(S)]
    k = np.arange(n)
    typ = np.where((k // S) % 2 == 0, V, C).astype(np.uint8)
    rnd = (k // (2 * S)).astype(np.int64)
    value = np.frombuffer(b"".join(w if q >= 65800 else v for q in range(n)), np.uint8).reshape(n, 32)
    frm = np.frombuffer(b"".join(senders[q % S] for q in range(n)), np.uint8).reshape(n, 32)
    sig = np.frombuffer(b"".join(EC.sig_of(b"big", q) for q in range(n)), np.uint8).reshape(n, 65)
    nb = Batch(typ, np.full(n, H, np.int64), rnd, np.full(n, -1, np.int64), value, frm, sig)
    kept = EC.rows(nb)
    ok = [1] * n
    log = verifier.open_log(H, 1, None, keep_signatures=True)
    try:
        res = log.insert(nb, np.zeros(n, np.uint8))
        assert res.kept == n == log.entries and res.logpos[-1] == n - 1
        # one sender's votes: a match in block 256, behind 256 counts
        s = senders[1700]
        sel = log.select(VOTES, sender=s)
        same_selection(sel, kept, ok, *SC.select(kept, VOTES, sender=s))
        assert sel.total == 33 and sel.positions[-1] == 65700
        # one round's precommits: 2,000 consecutive matches
        sel = log.select(C, round=5)
        same_selection(sel, kept, ok, *SC.select(kept, C, round=5))
        assert sel.positions.tolist() == list(range(22000, 24000))
        # limit 3, the matches beginning in the last block
        sel = log.select(VOTES, value=w, limit=3)
        same_selection(sel, kept, ok, [65800, 65801, 65802], 36)
        assert log.count(VOTES, value=w) == 36 and log.count(VOTES) == n
        assert log.count(VOTES, round=16, first=65536) == 300
    finally:
        log.close()


# ---- 6. capacity ------------------------------------------------------------------------
def test_capacity(verifier, oracle, pair):
    import torch
    from hyperdrive_amd import _lib
    O = oracle
    L = 300
    p = pair()
    q = _pattern_pair(p, O, [True] * L, "value")
    kept = p.ys.kept
    flt = _filter(p.log, VOTES)
    # host form: one short is HD_ECAP with the need, nothing written; the same call with room succeeds
    for cap in (1, 64, 256, L - 1):
        rc, sel, pos, r, a = _raw_select(p.log, flt, cap)
        assert (rc, sel.total, sel.n, r.n) == (_lib.HD_ECAP, L, L, 0), cap
        assert (pos == 0xDEADBEEF).all() and not a["from32"].any()
    rc, sel, pos, r, a = _raw_select(p.log, flt, L)
    assert (rc, sel.total, sel.n, r.n) == (_lib.HD_OK, L, L, L)
    assert pos[:L].tolist() == list(range(L)) and (pos[L:] == 0xDEADBEEF).all()
    flt3 = _filter(p.log, VOTES, limit=3)                              # limit <= cap < total: no error
    rc, sel, pos, r, a = _raw_select(p.log, flt3, 3)
    assert (rc, sel.total, sel.n, pos[:3].tolist()) == (_lib.HD_OK, L, 3, [0, 1, 2]) and (pos[3:] == 0xDEADBEEF).all()
    rc, sel, pos, r, a = _raw_select(p.log, flt3, 2)
    assert (rc, sel.total, sel.n) == (_lib.HD_ECAP, L, 3)
    # positions alone, rows alone
    rc, sel, pos, r, a = _raw_select(p.log, flt, L, rows=False)
    assert rc == _lib.HD_OK and pos[:L].tolist() == list(range(L))
    rc, sel, pos, r, a = _raw_select(p.log, flt, L, pos=False)
    assert (rc, r.n) == (_lib.HD_OK, L) and a["sig65"][L - 1].tobytes() == kept[L - 1][89:]
    # the count-only form: NULL outputs, cap 0
    rc, sel, pos, r, a = _raw_select(p.log, flt, 0, rows=False, pos=False)
    assert (rc, sel.total, sel.n) == (_lib.HD_OK, L, L)
    rc, sel, pos, r, a = _raw_select(p.log, flt3, 0, rows=False, pos=False)
    assert (rc, sel.total, sel.n) == (_lib.HD_OK, L, 3)
    # device form: guard rows behind cap, filled with a pattern, are intact after HD_ECAP and after success
    lib = _lib.load()
    G = 8
    for cap, want_rc in ((40, _lib.HD_ECAP), (255, _lib.HD_ECAP), (L, _lib.HD_OK)):
        cols = _device_columns(cap + G)
        rc, sel = _raw_select_device(lib, p.log, flt, cols, cap)
        torch.cuda.synchronize()
        assert (rc, sel.total, sel.n) == (want_rc, L, L), cap
        for name, t in cols.items():
            assert (t[cap:] == 0xA5 if t.dtype == torch.uint8 else t[cap:] == GUARD[t.dtype]).all(), (cap, name)
        if rc == _lib.HD_OK:
            assert _device_rows(cols, L) == kept and cols["pos"][:L].tolist() == list(range(L))
    p.same_log()


GUARD = {}


def _device_columns(rows):
    """device columns of `rows` rows, every byte 0xA5"""
    import torch
    GUARD.update({torch.int64: struct.unpack("<q", b"\xA5" * 8)[0], torch.int32: struct.unpack("<i", b"\xA5" * 4)[0]})
    u8 = lambda *shape: torch.full(shape, 0xA5, dtype=torch.uint8, device="cuda")
    i64 = lambda: torch.full((rows,), GUARD[torch.int64], dtype=torch.int64, device="cuda")
    cols = {"type": u8(rows), "height": i64(), "round": i64(), "valid_round": i64(), "value": u8(rows, 32),
            "frm": u8(rows, 32), "sig": u8(rows, 65), "value_ok": u8(rows),
            "pos": torch.full((rows,), GUARD[torch.int32], dtype=torch.int32, device="cuda")}
    torch.cuda.synchronize()
    return cols


def _raw_select_device(lib, log, flt, cols, cap, valid_round=True, sig=True, value_ok=True, pos=True, stream=None):
    from hyperdrive_amd import _lib
    ptr = lambda k, on=True: cols[k].data_ptr() if on else None
    out = _lib.HdBatchOut(ptr("type"), ptr("height"), ptr("round"), ptr("valid_round", valid_round), ptr("value"),
                          ptr("frm"), ptr("sig", sig), None)
    sel = _lib.HdLogSelected(77, 77)
    rc = lib.hd_log_select_device(log.handle, ctypes.byref(flt), ctypes.byref(out), ptr("value_ok", value_ok),
                                  ptr("pos", pos), cap, ctypes.byref(sel), stream)
    return rc, sel


def _device_rows(cols, n):
    from hyperdrive_amd.verify import Batch
    c = lambda k: cols[k][:n].cpu().numpy()
    return EC.rows(Batch(c("type"), c("height"), c("round"), c("valid_round"), c("value"), c("frm"), c("sig")))


# ---- 7. the log is unchanged and scratch is never read ------------------------------------
def test_log_unchanged_and_scratch_unread(verifier, oracle, pair):
    from hyperdrive_amd import _lib
    O = oracle
    v, w, _ = _values(O)
    p = pair(max_entries=70)
    first = _batch(O, [(V if k % 2 else C, H, k // 8, -1, v, SC.sender(k // 2 % 4)) for k in range(60)], b"a")
    p.put(first)
    assert p.same(VOTES).total == 60 and p.same(C, round=(2, 5), limit=7).total == 16
    # fed on after the selects, the pair still equals the model: a double vote against entry 3, new votes
    more = _batch(O, [(V, H, 0, -1, w, SC.sender(1))] + [(V, H, 20 + k, -1, w, SC.sender(5)) for k in range(6)], b"b")
    res = p.put(more)
    assert res.caught == [(60, "double_prevote", 3)] and p.log.entries == 66
    p.same_log()
    assert p.same(V, value=w).positions.tolist() == list(range(60, 66))
    # an insert refused for max_entries leaves its rows behind L in the buffer: they are never selected
    refused = _batch(O, [(C, H, 40 + k, -1, w, SC.sender(6)) for k in range(9)], b"c")
    with pytest.raises(_lib.HDError) as e:
        p.log.insert(to_np(refused), np.zeros(9, np.uint8))
    assert e.value.code == _lib.HD_ECAP and p.log.entries == 66
    assert p.same((P, V, C)).total == 66 and p.same(C, value=w).total == 0
    assert p.same(VOTES, upto=5000).positions.tolist() == list(range(66))
    p.same_log()
    p.put(_batch(O, [(C, H, 40, -1, w, SC.sender(6))], b"d"))            # and it still takes what fits
    assert p.same(C, value=w).positions.tolist() == [66]
    # after a reset: zero matches, the old rows out of reach
    p.reset(H + 1)
    assert p.same((P, V, C)).total == 0 and p.same(VOTES, upto=66).total == 0
    nxt = _batch(O, [(V, H + 1, 0, -1, w, SC.sender(0))], b"e")
    p.put(nxt)
    assert p.same((P, V, C)).positions.tolist() == [0]


# ---- 8. ordering after an insert on a caller's stream -------------------------------------
def test_select_follows_an_insert_on_a_caller_s_stream(verifier, oracle, pair):
    import torch
    from hyperdrive_amd.device import DeviceBatch, work_stream
    O = oracle
    v, w, _ = _values(O)
    p = pair()
    n = 3000
    ob = _batch(O, [(V if k % 2 else C, H, k // 8, -1, w if k % 7 == 0 else v, SC.sender(k // 2 % 4)) for k in range(n)])
    exp, recs, ev = p.ys.push(ob, [O.VALID] * n)
    db = DeviceBatch.from_host(to_np(ob))
    bitmap = torch.full(((n + 31) // 32,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ws = work_stream()
    res = p.log.insert_device(db.c_struct(), bitmap.data_ptr(), stream=ws.cuda_stream)
    sel = p.log.select(VOTES, value=w)                                 # at once: the commit is still on ws
    LC.same_insert(res, exp)
    same_selection(sel, p.ys.kept, p.ys.kept_ok, *SC.select(p.ys.kept, VOTES, value=w))
    assert sel.total == len(range(0, n, 7))
    # and the device form on another stream of the caller's, behind a commit on the context's stream
    more = _batch(O, [(V, H, 900 + k, -1, w, SC.sender(9)) for k in range(500)], b"m")
    p.put(more)
    other = torch.cuda.Stream()
    ds = p.log.select_device(V, sender=SC.sender(9), stream=other)
    assert ds.n == ds.total == 500 and EC.rows(ds.batch.to_host()) == p.ys.kept[n:]
    assert ds.positions.cpu().tolist() == list(range(n, n + 500))


# ---- 9. the device form -------------------------------------------------------------------
def test_device_form(verifier, oracle, pair):
    import torch
    from hyperdrive_amd import _lib
    from hyperdrive_amd.codec import marshal_device, unmarshal_device
    O = oracle
    lib = _lib.load()
    p = pair()
    L = 700
    flags = SC.patterns(L)["random"]
    q = _pattern_pair(p, O, flags, "value")
    types = q.pop("types")
    host = p.same(types, **q)
    # the columns, read back, equal the host form's rows
    ds = p.log.select_device(types, **q)
    assert (ds.n, ds.total) == (len(host), host.total) and ds.n > 150
    assert EC.rows(ds.batch.to_host()) == EC.rows(host.batch)
    assert ds.value_ok.cpu().tolist() == host.value_ok.tolist()
    assert ds.positions.cpu().tolist() == host.positions.tolist()
    lim = p.log.select_device(types, limit=65, **q)
    assert (lim.n, lim.total) == (65, host.total) and EC.rows(lim.batch.to_host()) == EC.rows(host.batch)[:65]
    none = p.log.select_device(P)
    assert (none.n, none.total) == (0, 0)
    # valid_round, sig65, value_ok and the positions each NULL: that column is untouched, the rest is written
    flt = p.log._filter(types, None, q["value"], None, 0, None, 0)
    for off in ("valid_round", "sig", "value_ok", "pos"):
        cols = _device_columns(ds.n)
        rc, sel = _raw_select_device(lib, p.log, flt, cols, ds.n, **{off: False})
        torch.cuda.synchronize()
        assert (rc, sel.n) == (_lib.HD_OK, ds.n)
        guard = cols[off] == (0xA5 if cols[off].dtype == torch.uint8 else GUARD[cols[off].dtype])
        assert guard.all(), off
        for name in ("type", "height", "round", "value", "frm"):
            assert torch.equal(cols[name], getattr(ds.batch, name)), (off, name)
    # one round's precommits -> the wire -> back: byte for byte the selection
    r = 40
    pre = p.log.select_device(C, round=r)
    want = p.same(C, round=r)
    assert pre.n == len(want) > 0
    buf = marshal_device(verifier, C, pre.batch, with_sig=True)
    back, status = unmarshal_device(verifier, C, buf, pre.n, with_sig=True)
    assert not status.cpu().numpy().any()
    assert EC.rows(back.to_host()) == EC.rows(want.batch) == [p.ys.kept[k] for k in want.positions.tolist()]
    # a log that keeps no signatures: zero signatures in the host rows, HD_EINVAL for sig65
    bare = pair(keep=False)
    ob = SC.pattern_log(O, H, flags, "value", *_values(O))
    bare.log.insert(to_np(ob), np.zeros(L, np.uint8))
    sel = bare.log.select(types, **q)
    assert sel.positions.tolist() == host.positions.tolist() and not sel.batch.sig.any()
    assert [x[:89] for x in EC.rows(sel.batch)] == [x[:89] for x in EC.rows(host.batch)]
    dsel = bare.log.select_device(types, **q)
    assert not dsel.batch.sig.cpu().numpy().any() and EC.rows(dsel.batch.to_host()) == EC.rows(sel.batch)
    bflt = bare.log._filter(types, None, q["value"], None, 0, None, 0)
    assert _raw_select(bare.log, bflt, L, sig=True)[0] == _lib.HD_EINVAL
    assert _raw_select_device(lib, bare.log, bflt, _device_columns(L), L)[0] == _lib.HD_EINVAL
    assert _raw_select_device(lib, bare.log, bflt, _device_columns(L), L, sig=False)[0] == _lib.HD_OK


# ---- 10. a certificate end to end, with real signatures -------------------------------------
def test_certificate_end_to_end(gpu, oracle):
    from hyperdrive_amd import quorum
    from hyperdrive_amd.verify import Batch
    O = oracle
    keys = O.KeyCache()
    S, f, r = 7, 2, 3
    sigs = O.admitted_set(S, keys)
    v, w = O.canonical_value(H, 0), O.canonical_value(H, 1)

    def signed(t, rnd, value, who):
        return (t, H, rnd, -1, value, sigs[who], O.sign(keys.sk(who), O.message_digest(t, H, rnd, -1, value)))

    def batch(msgs):
        ob = O.Batch()
        for m in msgs:
            ob.append(*m)
        return to_np(ob)

    # flush 1: the propose, a precommit for another value, three precommits for v; flush 2: a prevote, the
    # fourth and fifth precommit for v -- commit fires at the fifth -- and a sixth behind it
    flushes = [[signed(P, r, v, 0), signed(C, r, w, 6), signed(C, r, v, 0), signed(C, r, v, 1), signed(C, r, v, 2)],
               [signed(V, r, v, 3), signed(C, r, v, 3), signed(C, r, v, 4), signed(C, r, v, 5)]]
    a, b = gpu.Verifier(0), gpu.Verifier(0)
    log = None
    try:
        a.set_signatories(_rows(sigs))
        b.set_signatories(_rows(sigs))
        log = a.open_log(H, f, None, keep_signatures=True)
        results = []
        for msgs in flushes:
            nb = batch(msgs)
            vd = a.verify_batch(nb).verdict
            assert vd.tolist() == [O.VALID] * len(msgs)
            results.append(log.insert(nb, vd))
        assert not [x for x in results[0].new_firings if x[3] == "commit"]
        (i, h, rr, _), = [x for x in results[1].new_firings if x[3] == "commit"]
        assert (i, h, rr) == (2, H, r)
        fired = int(results[1].logpos[i])                              # a batch index -> the log position
        assert fired == results[1].base + i == 7
        cert = log.certificate("precommit", r, v, upto=fired)
        assert len(cert) == 2 * f + 1 == 5 and cert.positions.tolist() == [2, 3, 4, 6, 7]
        assert all(q <= fired for q in cert.positions.tolist()) and cert.total == 5
        assert log.certificate("precommit", r, v, upto=fired - 1) is None          # one message before the firing
        assert log.certificate("precommit", r, w) is None and log.certificate("prevote", r, v) is None
        assert log.certificate("precommit", r, v).positions.tolist() == [2, 3, 4, 6, 7]   # the first 2f+1 of six
        # the reference's lookups
        pr = log.proposal(r)
        assert pr.positions.tolist() == [0] and pr.value_ok.tolist() == [1] and pr.batch.value[0].tobytes() == v
        assert log.proposal(r + 1) is None
        assert log.votes("precommit", r).positions.tolist() == [1, 2, 3, 4, 6, 7, 8]
        assert log.votes("prevote", r).positions.tolist() == [5] and len(log.votes(V, r + 1)) == 0
        assert log.vote_of("precommit", r, sigs[6]).batch.value[0].tobytes() == w
        assert log.vote_of("precommit", r, sigs[3]).positions.tolist() == [6]
        assert log.vote_of("prevote", r, sigs[0]) is None
        # the receiving side, a fresh verifier with the same set
        cb = cert.batch
        assert quorum.check_certificate(b, cb, H, r, "precommit", v, f) is True
        assert quorum.check_certificate(b, cb, H, r, C, v, f) is True
        take = lambda ix: Batch(cb.type[ix], cb.height[ix], cb.round[ix], cb.valid_round[ix], cb.value[ix], cb.frm[ix],
                                cb.sig[ix])
        assert quorum.check_certificate(b, take([0, 1, 2, 3]), H, r, "precommit", v, f) is False   # one row dropped
        assert quorum.check_certificate(b, take([0, 1, 2, 3, 3]), H, r, "precommit", v, f) is False   # one twice
        bad = take([0, 1, 2, 3, 4])
        bad.sig[2, 40] ^= 1                                            # one signature byte
        assert quorum.check_certificate(b, bad, H, r, "precommit", v, f) is False
        for args in ((H + 1, r, "precommit", v), (H, r + 1, "precommit", v), (H, r, "prevote", v), (H, r, "precommit", w)):
            assert quorum.check_certificate(b, cb, *args, f) is False
        assert quorum.check_certificate(b, cb, H, r, "precommit", v, 3) is False   # 2f+1 = 7 > 5
    finally:
        if log is not None:
            log.close()
        a.close()
        b.close()


# ---- 11. argument errors ------------------------------------------------------------------
def test_argument_errors(verifier, oracle, pair):
    from hyperdrive_amd import _lib
    O = oracle
    lib = _lib.load()
    p = pair()
    q = _pattern_pair(p, O, [True] * 100, "value")
    good = _filter(p.log, VOTES)
    EINVAL = _lib.HD_EINVAL

    def refused(flt=good, cap=100, **k):
        rc, sel, pos, r, a = _raw_select(p.log, flt, cap, **k)
        assert rc == EINVAL and (pos == 0xDEADBEEF).all() and r.n == 0, (rc, cap, k)

    def changed(**k):
        flt = _filter(p.log, VOTES)
        for name, val in k.items():
            setattr(flt, name, val)
        return flt

    for mask in (0, 1, 16, 0xE | 1, 0xE | 16, 0x80000004):
        refused(changed(type_mask=mask))
    for flags in (4, 7, 0x80000000):
        refused(changed(flags=flags))
    refused(changed(reserved=1))
    refused(rows_cap=99)                                               # rows->cap < cap
    refused(None)                                                      # a NULL filter
    sel = _lib.HdLogSelected()
    assert lib.hd_log_select(None, ctypes.byref(good), None, 0, None, ctypes.byref(sel)) == EINVAL
    assert lib.hd_log_select(p.log.handle, ctypes.byref(good), None, 0, None, None) == EINVAL
    rc, sel, pos, r, a = _raw_select(p.log, good, 100)
    r.height = None                                                    # rows without one of its arrays
    assert lib.hd_log_select(p.log.handle, ctypes.byref(good), None, 100, ctypes.byref(r), ctypes.byref(sel)) == EINVAL
    # the device form refuses the same, and columns it cannot write
    cols = _device_columns(100)
    assert _raw_select_device(lib, p.log, changed(type_mask=0), cols, 100)[0] == EINVAL
    assert _raw_select_device(lib, p.log, changed(flags=8), cols, 100)[0] == EINVAL
    assert _raw_select_device(lib, p.log, changed(reserved=2), cols, 100)[0] == EINVAL
    assert lib.hd_log_select_device(None, ctypes.byref(good), None, None, None, 0, ctypes.byref(sel), None) == EINVAL
    assert lib.hd_log_select_device(p.log.handle, None, None, None, None, 0, ctypes.byref(sel), None) == EINVAL
    assert lib.hd_log_select_device(p.log.handle, ctypes.byref(good), None, None, None, 0, None, None) == EINVAL
    assert lib.hd_log_select_device(p.log.handle, ctypes.byref(good), None, None, None, 5, ctypes.byref(sel),
                                    None) == EINVAL                    # rows asked for, no columns
    import torch
    torch.cuda.synchronize()
    for name, t in cols.items():
        assert (t == (0xA5 if t.dtype == torch.uint8 else GUARD[t.dtype])).all(), name
    # the device form's count-only call, and the log and a following select as before
    assert lib.hd_log_select_device(p.log.handle, ctypes.byref(good), None, None, None, 0, ctypes.byref(sel),
                                    None) == _lib.HD_OK
    assert (sel.total, sel.n) == (100, 100)
    assert p.log.entries == 100
    p.same_log()
    assert p.same(VOTES).total == 100
    with pytest.raises(ValueError):
        p.log.select("vote")
    with pytest.raises(ValueError):
        p.log.votes("propose", 0)
