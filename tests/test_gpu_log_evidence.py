"""Whole messages in hd_log (include/hd_log.h): signatures kept on request
(hd_log_keep_signatures), entries read back (hd_log_read) and both messages of
every catch record returned with it (hd_log_insert_evidence and its device
form; ``evidence=True`` on DecideLog.insert* and Ingress.flush_decide), against
the model of tests/evidence_cases.py -- the host copy of the log these calls
replace.  Every comparison is exact, all 154 bytes of a row; every message
carries signature bytes of its own, so a row gathered from the wrong place
cannot compare equal.  Verdicts are passed directly except in the device-entry
and ingress cases.  tests/test_evidence_host.py pins the model."""
import ctypes
import random

import numpy as np
import pytest

import catch_cases as CC
import evidence_cases as EC
import log_cases as LC
import when_cases as WC
from util import to_np

pytestmark = pytest.mark.gpu

NEVER = CC.NEVER
H = 5


@pytest.fixture(scope="module")
def verifier(gpu):
    v = gpu.Verifier(0)
    yield v
    v.close()


def _rows(sigs):
    return np.frombuffer(b"".join(sigs), np.uint8).reshape(len(sigs), 32).copy()


def _batch(O, msgs, tag=b"e"):
    ob = O.Batch()
    for m in msgs:
        ob.append(*m, bytes(65))
    return EC.unique_sigs(ob, tag)


class Pair:
    """A library log that keeps signatures and the model fed side by side, every insert with evidence."""

    def __init__(self, verifier, O, height, f, schedule=None, keep=True):
        self.O = O
        self.log = verifier.open_log(height, f, _rows(schedule) if schedule is not None else None,
                                     keep_signatures=keep)
        self.ys = EC.Kept(height, f, schedule)

    def put(self, ob, verdicts=None, value_ok=None):
        verdicts = [self.O.VALID] * len(ob) if verdicts is None else verdicts
        res = self.log.insert(to_np(ob), np.array(verdicts, np.uint8),
                              None if value_ok is None else np.array(value_ok, np.uint8), catch=True, evidence=True)
        exp, recs, ev = self.ys.push(ob, verdicts, value_ok)
        LC.same_insert(res, exp)
        CC.same_caught(res, recs)
        EC.same_evidence(res, ev)
        assert self.log.entries == self.ys.entries == res.base + res.kept
        return res

    def same_log(self):
        """hd_log_read of everything == the model's list."""
        b, ok = self.log.read()
        assert EC.rows(b) == self.ys.kept and ok.tolist() == self.ys.kept_ok
        return b, ok

    def reset(self, height):
        self.log.reset(height)
        self.ys = EC.Kept(height, self.ys.cs.ys.f, self.ys.cs.ys.schedule)

    def close(self):
        self.log.close()


@pytest.fixture
def pair(verifier, oracle):
    made = []

    def make(height, f, schedule=None, keep=True):
        made.append(Pair(verifier, oracle, height, f, schedule, keep))
        return made[-1]

    yield make
    for p in made:
        p.close()


def _sig(O):
    return lambda k: O.sha256(b"g" + bytes([k]))


def _setup(verifier, O):
    sig = _sig(O)
    verifier.set_signatories(_rows([sig(k) for k in range(6)]))       # 6..: outside the set (hashed log path)
    return sig, O.canonical_value(H, 0), O.canonical_value(H, 1)


def _raw_evidence(log, nb, vd, vok=None, cap=None, sig=True, batch_sig=True):
    """hd_log_insert_evidence through the C ABI: (rc, catch struct, catch arrays, evidence struct, its arrays, out)."""
    from hyperdrive_amd import _lib
    from hyperdrive_amd.verify import _catch_struct, _rows_struct
    lib = _lib.load()
    n = len(nb)
    o, a, w, when, until, logpos, info = log._outputs(n)
    c, ca = _catch_struct(n)
    if cap is not None:
        c.cap = cap
    off, oa = _rows_struct(n, sig)
    ag, aa = _rows_struct(n, sig)
    ev = _lib.HdEvidenceOut(off, ag)
    cb = nb.c_struct()
    if not batch_sig:
        cb.sig65 = None
    rc = lib.hd_log_insert_evidence(log.handle, ctypes.byref(cb), vd.ctypes.data,
                                    vok.ctypes.data if vok is not None else None, ctypes.byref(o), ctypes.byref(w),
                                    ctypes.byref(info), ctypes.byref(c), ctypes.byref(ev))
    return rc, c, ca, ev, (oa, aa), o


def _raw_rows(ev, arrs):
    from hyperdrive_amd.verify import _rows_batch
    return (EC.rows(_rows_batch(ev.offender.n, arrs[0])[0]), EC.rows(_rows_batch(ev.against.n, arrs[1])[0]))


def _raw_read(log, pos, first, n, sig=True, cap=None):
    from hyperdrive_amd import _lib
    from hyperdrive_amd.verify import _rows_struct
    r, a = _rows_struct(n if cap is None else cap, sig)
    p = np.ascontiguousarray(pos, np.uint32) if pos is not None else None
    rc = _lib.load().hd_log_read(log.handle, p.ctypes.data if p is not None else None, first, n, ctypes.byref(r))
    return rc, r, a


# ---- 1. every cut of a small stream -----------------------------------------------------
def _small_stream(O):
    """catch_cases.mix_40 (a double prevote, two double precommits, an out-of-turn propose) with two
    conflicting in-turn proposes of a round the mix does not use put in at 5 and 25: 42 messages, four kinds."""
    sigs, sched, ob, verdicts, value_ok = CC.mix_40()
    out, vd, vok = O.Batch(), [], []
    turn = sched[(H + 3) % len(sched)]
    for i in range(len(ob)):
        if i in (5, 25):
            out.append(O.PROPOSE, H, 3, -1, O.canonical_value(H, 0 if i == 5 else 1), turn, bytes(65))
            vd.append(O.VALID)
            vok.append(1)
        out.append(ob.mtype[i], ob.height[i], ob.round[i], ob.valid_round[i], ob.value[i], ob.frm[i], ob.sig[i])
        vd.append(verdicts[i])
        vok.append(value_ok[i])
    return sigs, sched, EC.unique_sigs(out), vd, vok


def test_every_cut_of_a_small_stream(verifier, oracle, pair):
    sigs, sched, ob, verdicts, value_ok = _small_stream(oracle)
    n = len(ob)
    assert n == 42 and {k for _, k, _ in CC.records(ob, verdicts, sched)} == {1, 2, 3, 4}
    verifier.set_signatories(_rows(sigs[:5]))
    p = pair(H, 2, sched)
    below = above = 0
    for c in range(1, n):
        p.reset(H)
        a = p.put(*LC.cut(ob, verdicts, value_ok, 0, c))
        b = p.put(*LC.cut(ob, verdicts, value_ok, c, n))
        assert len(a.caught) + len(b.caught) == 5
        below += sum(1 for _, _, x in b.caught if x < b.base)
        above += sum(1 for _, _, x in b.caught if b.base <= x != NEVER)
        if c in (1, 20, 41):
            p.same_log()
    assert below > 0 and above > 0


# ---- 2. wave and block edges of the gather ----------------------------------------------
@pytest.mark.parametrize("count", [0, 1, 63, 64, 65, 255, 256, 257])
def test_record_counts_at_the_gather_s_edges(verifier, oracle, pair, count):
    """One insert with exactly `count` records on a fresh log (which stages 256 records of evidence: 257
    take the second copy).  Even records contradict an entry of an earlier insert, odd ones a message of
    this batch."""
    O = oracle
    sig, v, w = _setup(verifier, O)
    p = pair(H, 1)
    p.put(_batch(O, [(O.PREVOTE, H, 0, -1, v, sig(7)), (O.PREVOTE, H, 0, -1, v, sig(0))], b"a"))
    msgs = [(O.PREVOTE, H, 0, -1, v, sig(8))] + [(O.PREVOTE, H, 0, -1, w, sig(0 if k % 2 == 0 else 8))
                                                  for k in range(count)]
    ob = _batch(O, msgs, b"b")
    recs, _ = p.ys.peek(ob, [O.VALID] * len(ob))
    assert len(recs) == count
    assert [a for _, _, a in recs] == [1 if k % 2 == 0 else 2 for k in range(count)]
    res = p.put(ob)
    assert len(res.caught) == count and len(res.evidence_offender) == len(res.evidence_against) == count
    p.same_log()


# ---- 3. past the catch list's staged capacity -------------------------------------------
def test_past_the_staged_capacity_and_the_list_s_own(gpu, oracle):
    """A fresh context stages 1,024 catch records and a fresh log 256 records of evidence: 1,897 take
    both overflow paths.  Then the list at exactly its need and one short of it."""
    from hyperdrive_amd import _lib
    O = oracle
    sigs, sched, ob, verdicts, value_ok = CC.mix_3000(True)
    ob = EC.unique_sigs(ob)
    model = EC.Kept(H, 13, sched)
    recs, ev = model.peek(ob, verdicts)
    need = len(recs)
    assert need == 1897 > 1024
    nb, vd, vok = to_np(ob), np.array(verdicts, np.uint8), np.array(value_ok, np.uint8)
    v = gpu.Verifier(0)
    logs = []
    try:
        v.set_signatories(_rows(sigs[:20]))                            # signers 20..39 take the hashed table
        logs = [v.open_log(H, 13, _rows(sched), keep_signatures=True) for _ in range(2)]
        first = logs[0].insert(nb, vd, vok, catch=True, evidence=True)
        CC.same_caught(first, recs)
        EC.same_evidence(first, ev)
        want = (EC.rows(first.evidence_offender), EC.rows(first.evidence_against))
        # one short: HD_ECAP with the need, the log unchanged; then exactly the need
        rc, c, ca, e, arrs, o = _raw_evidence(logs[1], nb, vd, vok, cap=need - 1)
        assert (rc, c.n, logs[1].entries) == (_lib.HD_ECAP, need, 0)
        assert (e.offender.n, e.against.n) == (0, 0)
        rc, c, ca, e, arrs, o = _raw_evidence(logs[1], nb, vd, vok, cap=need)
        assert (rc, c.n, e.offender.n, e.against.n) == (_lib.HD_OK, need, need, need)
        assert ca["index"][:need].tolist() == first.caught_index.tolist()
        assert _raw_rows(e, arrs) == want
        assert logs[1].entries == logs[0].entries == first.kept
    finally:
        for lg in logs:
            lg.close()
        v.close()


def test_evidence_rows_need_the_list_s_capacity(verifier, oracle, pair):
    from hyperdrive_amd import _lib
    from hyperdrive_amd.verify import _catch_struct, _rows_struct
    O = oracle
    sig, v, w = _setup(verifier, O)
    p = pair(H, 1)
    p.put(_batch(O, [(O.PREVOTE, H, 0, -1, v, sig(0))], b"a"))
    ob = _batch(O, [(O.PREVOTE, H, 0, -1, w, sig(0))] * 3, b"b")
    nb, vd = to_np(ob), np.zeros(3, np.uint8)
    lib = _lib.load()
    o, a, w_, when, until, logpos, info = p.log._outputs(3)
    c, ca = _catch_struct(3)
    off, oa = _rows_struct(3, True)
    ag, aa = _rows_struct(2, True)                                    # one row short of caught->cap
    e = _lib.HdEvidenceOut(off, ag)
    cb = nb.c_struct()
    args = (p.log.handle, ctypes.byref(cb), vd.ctypes.data, None, ctypes.byref(o), ctypes.byref(w_),
            ctypes.byref(info))
    assert lib.hd_log_insert_evidence(*args, ctypes.byref(c), ctypes.byref(e)) == _lib.HD_EINVAL
    assert lib.hd_log_insert_evidence(*args, ctypes.byref(c), None) == _lib.HD_EINVAL
    assert lib.hd_log_insert_evidence(*args, None, ctypes.byref(e)) == _lib.HD_EINVAL
    assert p.log.entries == 1
    with pytest.raises(ValueError):
        p.log.insert(nb, vd, evidence=True)                           # evidence without catch
    assert len(p.put(ob).caught) == 3


# ---- 4. first-wins signature ------------------------------------------------------------
def test_the_first_copy_s_signature_wins(verifier, oracle, pair):
    O = oracle
    sig, v, w = _setup(verifier, O)
    for signer in (0, 9):                                              # dense cell, hashed table
        s = sig(signer)
        p = pair(H, 1)
        first = _batch(O, [(O.PREVOTE, H, 0, -1, v, s)], b"1")
        resent = _batch(O, [(O.PREVOTE, H, 0, -1, v, s), (O.PREVOTE, H, 0, -1, w, s)], b"2")
        p.put(first)
        res = p.put(resent)
        assert res.dup.tolist() == [1, 2] and res.kept == 0 and res.caught == [(2, "double_prevote", 0)]
        assert res.evidence_against.sig[0].tobytes() == first.sig[0] != resent.sig[0]
        assert res.evidence_offender.sig[0].tobytes() == resent.sig[1]
        b, _ = p.log.read()
        assert len(b) == 1 and b.sig[0].tobytes() == first.sig[0]
        # both copies in one insert
        p.reset(H)
        one = _batch(O, [(O.PREVOTE, H, 0, -1, v, s), (O.PREVOTE, H, 0, -1, v, s), (O.PREVOTE, H, 0, -1, w, s)], b"3")
        res = p.put(one)
        assert res.evidence_against.sig[0].tobytes() == one.sig[0]
        assert p.log.read()[0].sig[0].tobytes() == one.sig[0]


# ---- 5. alignment -------------------------------------------------------------------------
def _device_batch(nb, sig_offset):
    """nb on the device with its sig65 base `sig_offset` bytes past a 16-byte boundary."""
    import torch
    from hyperdrive_amd._lib import HdBatch
    from hyperdrive_amd.device import DeviceBatch
    db = DeviceBatch.from_host(nb)
    n = len(nb)
    buf = torch.zeros(65 * n + 32, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    buf[sig_offset: sig_offset + 65 * n] = torch.from_numpy(nb.sig.reshape(-1)).cuda()
    cs = db.c_struct()
    cs.sig65 = buf.data_ptr() + sig_offset
    bitmap = torch.full(((n + 31) // 32,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    return cs, bitmap, (db, buf)


@pytest.mark.parametrize("offset", [1, 4, 8])
def test_misaligned_signatures_in_the_device_form(verifier, oracle, pair, offset):
    """Offenders at messages 4..7 and the messages they contradict at 0..3: 65 i mod 4 takes every value
    on both sides, over a base that is itself `offset` bytes off."""
    from hyperdrive_amd.device import work_stream
    O = oracle
    sig, v, w = _setup(verifier, O)
    msgs = [(O.PREVOTE, H, 0, -1, v, sig(k)) for k in range(4)] + [(O.PREVOTE, H, 0, -1, w, sig(k)) for k in range(4)]
    ob = _batch(O, msgs)
    p = pair(H, 1)
    exp, recs, ev = p.ys.push(ob, [O.VALID] * 8)
    assert [(i, a) for i, _, a in recs] == [(4, 0), (5, 1), (6, 2), (7, 3)]
    cs, bitmap, hold = _device_batch(to_np(ob), offset)
    res = p.log.insert_device(cs, bitmap.data_ptr(), stream=work_stream().cuda_stream, catch=True, evidence=True)
    LC.same_insert(res, exp)
    CC.same_caught(res, recs)
    EC.same_evidence(res, ev)
    p.same_log()
    # the second insert's logged messages are retained entries, read from the log's own column
    again = _batch(O, msgs[4:], b"f")
    exp, recs, ev = p.ys.push(again, [O.VALID] * 4)
    cs, bitmap, hold = _device_batch(to_np(again), offset)
    res = p.log.insert_device(cs, bitmap.data_ptr(), stream=work_stream().cuda_stream, catch=True, evidence=True)
    CC.same_caught(res, recs)
    EC.same_evidence(res, ev)
    assert [a for _, _, a in res.caught] == [0, 1, 2, 3]


# ---- 6. regrow while holding signatures -------------------------------------------------
def test_regrow_while_holding_signatures(verifier, oracle, pair):
    """The columns are sized max(need * 1.25, 4096) rows.  The first insert joins 0 + 3,500 rows: capacity
    4,375, and all 3,500 are kept.  The second joins 3,500 + 2,000 = 5,500 > 4,375: the columns are
    allocated again (6,875 rows) and the first 3,500 rows, signatures included, are carried over."""
    O = oracle
    sig, v, w = _setup(verifier, O)
    signer = lambda k: O.sha256(b"s" + k.to_bytes(2, "big"))           # none admitted
    p = pair(H, 1)
    a = p.put(_batch(O, [(O.PREVOTE, H, 0, -1, v, signer(k)) for k in range(3500)], b"a"))
    assert a.kept == 3500
    b = p.put(_batch(O, [(O.PRECOMMIT, H, 0, -1, v, signer(k)) for k in range(1999)]
                     + [(O.PREVOTE, H, 0, -1, w, signer(3499))], b"b"))
    assert (b.base, b.kept) == (3500, 1999) and b.caught == [(5499, "double_prevote", 3499)]
    assert p.log.entries == 5499
    p.same_log()


# ---- 7. read ----------------------------------------------------------------------------
def test_read_cases(verifier, oracle, pair):
    from hyperdrive_amd import _lib
    O = oracle
    sig, v, w = _setup(verifier, O)
    signer = lambda k: O.sha256(b"t" + k.to_bytes(2, "big"))
    p = pair(H, 1, [sig(k) for k in range(4)])
    # an empty log: n = 0 is fine, any position is not
    b, ok = p.log.read()
    assert len(b) == 0 and len(ok) == 0
    assert _raw_read(p.log, None, 0, 0)[0] == _lib.HD_OK
    assert _raw_read(p.log, None, 0, 1)[0] == _lib.HD_EINVAL
    # 130 entries, a propose among them; every fifth value_ok byte is 0
    msgs = [(O.PREVOTE if k % 2 else O.PRECOMMIT, H, k % 3, -1, v, signer(k)) for k in range(129)]
    msgs.insert(7, (O.PROPOSE, H, 0, -1, w, sig(1)))                  # (5 + 0) % 4 = 1: in turn
    ob = _batch(O, msgs)
    p.put(ob, value_ok=[k % 5 != 0 for k in range(130)])
    L = p.log.entries
    assert L == 130
    whole, whole_ok = p.same_log()
    assert whole.valid_round.tolist() == [-1] * 130 and whole_ok.tolist()[:6] == [0, 1, 1, 1, 1, 0]
    rng = random.Random(7)
    for n in (1, 64, 65, L):
        pos = [rng.randrange(L) for _ in range(n)]
        pos[-1] = pos[0]                                               # a repeat
        b, ok = p.log.read(positions=pos)
        assert EC.rows(b) == [p.ys.kept[q] for q in pos] and ok.tolist() == [p.ys.kept_ok[q] for q in pos]
        b, ok = p.log.read(first=L - n, n=n)                           # a range that ends at the log's end
        assert EC.rows(b) == p.ys.kept[L - n:] and ok.tolist() == p.ys.kept_ok[L - n:]
    assert EC.rows(p.log.read(first=3)[0]) == p.ys.kept[3:]
    # without signatures: the fields only
    rc, r, a = _raw_read(p.log, [5, 129], 0, 2, sig=False)
    assert (rc, r.n) == (_lib.HD_OK, 2) and not a["sig65"].any()
    assert a["from32"][:2].tobytes() == ob.frm[5] + ob.frm[129]
    # errors, each before any device work and with the log unchanged
    for pos, first, n, cap in (([L], 0, 1, None), ([0, L, 1], 0, 3, None), (None, L, 1, None), (None, L - 1, 2, None),
                               (None, 0, 4, 3), (None, 0xFFFFFFFF, 2, None)):
        rc, r, a = _raw_read(p.log, pos, first, n, cap=cap)
        assert (rc, r.n) == (_lib.HD_EINVAL, 0), (pos, first, n, cap)
    lib = _lib.load()
    assert lib.hd_log_read(p.log.handle, None, 0, 1, None) == _lib.HD_EINVAL
    rc, r, a = _raw_read(p.log, None, 0, 1)
    r.height = None
    assert lib.hd_log_read(p.log.handle, None, 0, 1, ctypes.byref(r)) == _lib.HD_EINVAL
    assert _raw_read(p.log, None, L, 0)[0] == _lib.HD_OK               # nothing, at the end
    p.same_log()
    p.put(_batch(O, msgs[:4], b"x"))                                   # and the log still inserts: all four are resent
    assert p.log.entries == L
    # a log that keeps no signatures: sig65 is refused, the fields are read
    q = pair(H, 1, [sig(k) for k in range(4)], keep=False)
    q.log.insert(to_np(ob), np.zeros(130, np.uint8))
    assert _raw_read(q.log, None, 0, 2, sig=True)[0] == _lib.HD_EINVAL
    b, ok = q.log.read()
    assert q.log.entries == len(b) == 130 and not b.sig.any()
    assert [x[:89] for x in EC.rows(b)] == [EC.row(ob, i)[:89] for i in range(130)]


# ---- 8. snapshot / restore --------------------------------------------------------------
def test_snapshot_and_restore(verifier, oracle, pair):
    O = oracle
    sigs, sched, ob, verdicts, value_ok = CC.mix_3000(True)
    ob = EC.unique_sigs(ob)
    verifier.set_signatories(_rows(sigs[:20]))
    a = pair(H, 13, sched)
    a.put(*LC.cut(ob, verdicts, value_ok, 0, 700))
    a.put(*LC.cut(ob, verdicts, value_ok, 700, 1500))
    snap, snap_ok = a.same_log()
    L = len(snap)
    assert L == a.log.entries > 200 and 0 in snap_ok.tolist()
    report = a.log.insert(to_np(O.Batch()), np.zeros(0, np.uint8))     # n = 0: the log as it stands
    b = verifier.open_log(H, 13, _rows(sched), keep_signatures=True)
    try:
        res = b.insert(snap, np.zeros(L, np.uint8), snap_ok)
        assert (res.base, res.kept) == (0, L) and res.logpos.tolist() == list(range(L))
        assert len(res) == len(report) > 0
        for k in list(LC.ROW_FIELDS) + ["when", "exact_until"]:
            assert getattr(res, k).tolist() == getattr(report, k).tolist(), k
        again, again_ok = b.read()
        assert EC.rows(again) == EC.rows(snap) and again_ok.tolist() == snap_ok.tolist()
        # both go on alike
        part, pv, pok = LC.cut(ob, verdicts, value_ok, 1500, 2200)
        ra = a.put(part, pv, pok)
        rb = b.insert(to_np(part), np.array(pv, np.uint8), np.array(pok, np.uint8), catch=True, evidence=True)
        assert rb.caught == ra.caught and len(ra.caught) > 100
        assert EC.rows(rb.evidence_against) == EC.rows(ra.evidence_against)
        assert rb.when.tolist() == ra.when.tolist() and rb.logpos.tolist() == ra.logpos.tolist()
    finally:
        b.close()


# ---- 9. the setting and reset -----------------------------------------------------------
def test_setting_and_reset(verifier, oracle, pair):
    from hyperdrive_amd import _lib
    lib = _lib.load()
    O = oracle
    sig, v, w = _setup(verifier, O)
    p = pair(H, 1)
    ob = _batch(O, [(O.PREVOTE, H, 0, -1, v, sig(k)) for k in range(3)])
    nb, vd = to_np(ob), np.zeros(3, np.uint8)
    # an insert without signatures on a log that keeps them
    rc, c, ca, e, arrs, o = _raw_evidence(p.log, nb, vd, batch_sig=False)
    assert rc == _lib.HD_EINVAL and p.log.entries == 0
    cb = nb.c_struct()
    cb.sig65 = None
    o, a, w_, when, until, logpos, info = p.log._outputs(3)
    assert lib.hd_log_insert(p.log.handle, ctypes.byref(cb), vd.ctypes.data, None, ctypes.byref(o), ctypes.byref(w_),
                             ctypes.byref(info)) == _lib.HD_EINVAL
    assert p.log.entries == 0
    assert lib.hd_log_keep_signatures(p.log.handle, 1) == _lib.HD_OK   # empty: allowed, and already on
    p.put(ob)
    for on in (0, 1):
        assert lib.hd_log_keep_signatures(p.log.handle, on) == _lib.HD_EINVAL
    assert lib.hd_log_keep_signatures(None, 1) == _lib.HD_EINVAL
    p.same_log()
    p.reset(H + 1)
    assert p.log.entries == 0 and p.log.height == H + 1
    assert _raw_read(p.log, [0], 0, 1)[0] == _lib.HD_EINVAL            # the old rows are out of reach
    assert _raw_read(p.log, None, 0, 1)[0] == _lib.HD_EINVAL
    o, a, w_, when, until, logpos, info = p.log._outputs(3)
    assert lib.hd_log_insert(p.log.handle, ctypes.byref(cb), vd.ctypes.data, None, ctypes.byref(o), ctypes.byref(w_),
                             ctypes.byref(info)) == _lib.HD_EINVAL     # the setting still holds
    nxt = _batch(O, [(O.PREVOTE, H + 1, 0, -1, w, sig(k)) for k in range(2)], b"n")
    p.put(nxt)
    b, _ = p.same_log()
    assert len(b) == 2 and b.sig[1].tobytes() == nxt.sig[1]
    # switched off on the emptied log: inserts need no signatures again and none can be read
    p.log.reset(H + 2)
    assert lib.hd_log_keep_signatures(p.log.handle, 0) == _lib.HD_OK
    o, a, w_, when, until, logpos, info = p.log._outputs(3)
    assert lib.hd_log_insert(p.log.handle, ctypes.byref(cb), vd.ctypes.data, None, ctypes.byref(o), ctypes.byref(w_),
                             ctypes.byref(info)) == _lib.HD_OK
    assert _raw_read(p.log, None, 0, 1, sig=True)[0] == _lib.HD_EINVAL
    assert _raw_read(p.log, None, 0, 1, sig=False)[0] == _lib.HD_EINVAL   # the batch is of height 5: nothing kept
    assert p.log.entries == 0


# ---- 10. a log that never opted in ------------------------------------------------------
def test_opt_out_is_unchanged(verifier, oracle, pair):
    from hyperdrive_amd import _lib
    O = oracle
    sigs, sched, ob, verdicts, value_ok = CC.mix_40()
    verifier.set_signatories(_rows(sigs[:5]))
    log = verifier.open_log(H, 2, _rows(sched))
    try:
        assert log.keep_signatures is False
        ys, cs = LC.Stream(H, 2, sched), CC.Stream(H, 2, sched)
        for lo, hi in ((0, 13), (13, 40)):
            part, pv, pok = LC.cut(ob, verdicts, value_ok, lo, hi)
            exp = ys.peek(part, pv, pok)[0]
            nb = to_np(part)
            nb.sig = None                                              # and no signature array at all
            res = log.insert(nb, np.array(pv, np.uint8), np.array(pok, np.uint8), catch=True)
            assert type(res).__name__ == "CaughtLogInsertResult"
            LC.same_insert(res, exp)
            CC.same_caught(res, cs.push(part, pv, pok)[1])
            ys.push(part, pv, pok)
        plain = log.insert(to_np(ob), np.array(verdicts, np.uint8), np.array(value_ok, np.uint8))
        assert type(plain).__name__ == "LogInsertResult" and plain.kept == 0
        LC.same_insert(plain, ys.push(ob, verdicts, value_ok))
        # evidence on such a log: the fields, no signatures; asking for them is refused
        uo = EC.unique_sigs(ob)
        res = log.insert(to_np(uo), np.array(verdicts, np.uint8), np.array(value_ok, np.uint8), catch=True,
                         evidence=True)
        assert len(res.caught) == 4 and not res.evidence_offender.sig.any() and not res.evidence_against.sig.any()
        assert [x[:89] for x in EC.rows(res.evidence_offender)] == [EC.row(uo, i - res.base)[:89]
                                                                   for i in res.caught_index.tolist()]
        rc, c, ca, e, arrs, o = _raw_evidence(log, to_np(uo), np.array(verdicts, np.uint8), sig=True)
        assert rc == _lib.HD_EINVAL
    finally:
        log.close()


# ---- 11. the device form in four slices -------------------------------------------------
def test_device_form_in_four_slices(verifier, oracle):
    """As tests/test_gpu_catch.py::test_device_entries feeds a log: a generated, verified batch in four
    slices through the device form, beside the same slices through the host form."""
    import torch
    from hyperdrive_amd import quorum
    from hyperdrive_amd.device import generate, work_stream
    S, n, m = 100, 4096, 1024
    ks = verifier.gen_keys(S)
    verifier.set_signatories(ks[0])
    db, _, _ = generate(verifier, 1, n, S, 10, keys=ks)
    ws = work_stream()
    with torch.cuda.stream(ws):
        verdict = torch.empty(n, dtype=torch.uint8, device="cuda")
        bitmap = torch.zeros((n + 31) // 32, dtype=torch.int32, device="cuda")
    cs = db.c_struct()
    verifier.verify_batch_device(cs, verdict.data_ptr(), None, None, bitmap.data_ptr(), ws.cuda_stream)
    ws.synchronize()
    f = quorum.thresholds(S)[0]
    hb, hv = db.to_host(), verdict.cpu().numpy()
    dev, host = (verifier.open_log(1, f, ks[0], keep_signatures=True) for _ in range(2))
    try:
        got = below = 0
        for k in range(n // m):
            lo = k * m
            rd = dev.insert_device(db.rows(lo, m).c_struct(), bitmap.data_ptr() + 4 * (lo // 32),
                                   stream=ws.cuda_stream, catch=True, evidence=True)
            part = db.rows(lo, m).to_host()
            rh = host.insert(part, hv[lo: lo + m], catch=True, evidence=True)
            assert rd.caught == rh.caught and rd.logpos.tolist() == rh.logpos.tolist()
            assert EC.rows(rd.evidence_offender) == EC.rows(rh.evidence_offender)
            assert EC.rows(rd.evidence_against) == EC.rows(rh.evidence_against)
            # the offender rows are this slice's messages, signatures included
            src = EC.rows(part)
            assert EC.rows(rd.evidence_offender) == [src[i - rd.base] for i in rd.caught_index.tolist()]
            got += len(rd.caught)
            below += sum(1 for _, kd, a in rd.caught if a < rd.base)
        assert got > 20 and below > 0, (got, below)
        # the commit of the last device insert ran on the caller's stream: the read waits for it
        assert EC.rows(dev.read()[0]) == EC.rows(host.read()[0]) and dev.entries == host.entries > 0
    finally:
        dev.close()
        host.close()


# ---- 12. end to end through the ingress -------------------------------------------------
def test_ingress_evidence_is_signed_proof(verifier, oracle):
    """Really signed wire messages: a double prevote across two flushes and a double propose.  Both
    messages of each record come back whole: the oracle recovers the returned From from the returned
    signature over the returned fields."""
    import surge_codec as SC
    import torch
    from hyperdrive_amd.ingress import Ingress
    O = oracle
    keys = O.KeyCache()
    S = 4
    sigs = O.admitted_set(S, keys)
    verifier.set_signatories(_rows(sigs))
    v, w = O.canonical_value(H, 0), O.canonical_value(H, 1)

    def signed(t, r, vr, value, who):
        return (t, H, r, vr, value, sigs[who], O.sign(keys.sk(who), O.message_digest(t, H, r, vr, value)))

    turn = lambda r: (H + r) % S                                       # scheduler.go:52 over sigs
    flushes = [[signed(O.PREVOTE, 0, -1, v, 2), signed(O.PROPOSE, 0, -1, v, turn(0))],
               [signed(O.PREVOTE, 0, -1, w, 2),                        # double prevote, against flush 1
                signed(O.PROPOSE, 1, -1, v, turn(1)), signed(O.PROPOSE, 1, 0, w, turn(1))]]   # double propose
    ing = Ingress(verifier, height=H)
    try:
        ing.open_log(_rows(sigs), keep_signatures=True)
        out = []
        for msgs in flushes:
            for t in (O.PROPOSE, O.PREVOTE):
                ms = [m for m in msgs if m[0] == t]
                buf = SC.marshal_array(t, [m[1] for m in ms], [m[2] for m in ms], [m[3] for m in ms],
                                       [m[4] for m in ms], [m[5] for m in ms], [m[6] for m in ms])
                vd = ing.push_wire(t, torch.frombuffer(bytearray(buf), dtype=torch.uint8).cuda(), len(ms))
                assert vd.cpu().tolist() == [O.VALID] * len(ms)
            res, dec = ing.flush_decide(catch=True, evidence=True)
            assert len(res.consumed) == len(msgs)
            out.append(dec)
        assert out[0].caught == [] and out[0].kept == 2
        d = out[1]
        assert sorted(k for _, k, _ in d.caught) == ["double_prevote", "double_propose"]
        assert sorted(a < d.base for _, _, a in d.caught) == [False, True]
        sent = {m[6] for msgs in flushes for m in msgs}
        for side in (d.evidence_offender, d.evidence_against):
            assert len(side) == 2
            for i in range(2):
                t, r, vr = int(side.type[i]), int(side.round[i]), int(side.valid_round[i])
                frm, sg = side.frm[i].tobytes(), side.sig[i].tobytes()
                assert sg in sent
                assert O.verify_message(t, int(side.height[i]), r, vr, side.value[i].tobytes(), frm, sg,
                                        set(sigs)) == (O.VALID, frm)
        for k in range(2):                                             # a pair contradicts: same sender, other content
            assert d.evidence_offender.frm[k].tobytes() == d.evidence_against.frm[k].tobytes()
            assert d.evidence_offender.value[k].tobytes() != d.evidence_against.value[k].tobytes()
    finally:
        ing.close()
