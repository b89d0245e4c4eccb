"""The catch list (hd_catch_out: hd_decide_catch, hd_log_insert_catch and their
device forms; ``catch=True`` on Verifier.decide*, DecideLog.insert* and
Ingress.flush_decide) against the yardstick of tests/catch_cases.py: every
list is exact -- indices, kinds and the logged message each offence
contradicts, in batch order, in a log's joined coordinates.  Verdicts are
passed directly and the signatures are 65 zero bytes, as in
tests/test_gpu_log.py; only the device-entry and ingress cases verify generated
batches first.  tests/test_catch_host.py pins the yardstick and the record
counts the coverage claims below rest on."""
import ctypes
import random

import numpy as np
import pytest

import catch_cases as CC
import log_cases as LC
import propose_cases as PC
import when_cases as WC
from util import from_np, to_np

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


def _batch(O, msgs):
    ob = O.Batch()
    for m in msgs:
        ob.append(*m, bytes(65))
    return ob


class Pair:
    """A library log and the yardstick fed side by side, every insert catching."""

    def __init__(self, verifier, O, height, f, schedule=None, max_entries=0):
        self.O = O
        self.log = verifier.open_log(height, f, _rows(schedule) if schedule is not None else None, max_entries)
        self.ys = CC.Stream(height, f, schedule)

    def put(self, msgs, verdicts=None, value_ok=None):
        ob = msgs if hasattr(msgs, "mtype") else _batch(self.O, msgs)
        verdicts = [self.O.VALID] * len(ob) if verdicts is None else verdicts
        res = self.log.insert(to_np(ob), np.array(verdicts, np.uint8),
                              None if value_ok is None else np.array(value_ok, np.uint8), catch=True)
        exp, recs = self.ys.push(ob, verdicts, value_ok)
        LC.same_insert(res, exp)
        CC.same_caught(res, recs)
        assert self.log.entries == self.ys.entries == res.base + res.kept
        assert all(i >= res.base for i in res.caught_index.tolist())
        return res

    def reset(self, height):
        self.log.reset(height)
        self.ys = CC.Stream(height, self.ys.ys.f, self.ys.ys.schedule)

    def close(self):
        self.log.close()


@pytest.fixture
def pair(verifier, oracle):
    made = []

    def make(height, f, schedule=None, max_entries=0):
        made.append(Pair(verifier, oracle, height, f, schedule, max_entries))
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


def _raw_decide(verifier, ob, verdicts, f, sched=None, ordered=False, catch_cap=None, out_cap=None, classes=True,
                null_arrays=False):
    """hd_decide_catch through the C ABI: (rc, out, arrays, when, until, catch struct, catch arrays)."""
    from hyperdrive_amd import _lib
    from hyperdrive_amd.verify import _catch_struct
    lib = _lib.load()
    n = len(ob)
    nb, v = to_np(ob), np.array(verdicts, np.uint8)
    o, a = verifier._decide_struct(n)
    w, when, until = verifier._order_struct(n)
    c, ca = _catch_struct(n)
    if catch_cap is not None:
        c.cap = catch_cap
    if null_arrays:
        c.index = c.against = c.kind = None
    if out_cap is not None:
        o.cap = out_cap
    if not classes:
        o.dup = o.pclass = None
    rows = _rows(sched) if sched is not None else None
    cin = _lib.HdDecideIn(f, len(sched) if sched is not None else 0, rows.ctypes.data if rows is not None else None,
                          None)
    cb = nb.c_struct()
    rc = lib.hd_decide_catch(verifier.handle, ctypes.byref(cb), v.ctypes.data, ctypes.byref(cin), ctypes.byref(o),
                             ctypes.byref(w) if ordered else None, ctypes.byref(c))
    return rc, o, a, when, until, c, ca


def _list(c, ca):
    return list(zip(ca["index"][: c.n].tolist(), ca["kind"][: c.n].tolist(), ca["against"][: c.n].tolist()))


# ---- 1. each kind by hand, both log paths ---------------------------------------------
@pytest.mark.parametrize("signer", [0, 9])
def test_each_kind_by_hand(verifier, oracle, pair, signer):
    """signer 0 is admitted (dense log cells), 9 is not (the hashed table D)."""
    O = oracle
    sig, v, w = _setup(verifier, O)
    sched = [sig(k) for k in range(4)]                                 # (5 + 0) % 4 = 1
    s = sig(signer)
    msgs = [
        (O.PREVOTE, H, 0, -1, v, s),              # 0 logged
        (O.PRECOMMIT, H, 0, -1, v, s),            # 1 logged
        (O.PROPOSE, H, 0, -1, v, sig(1)),         # 2 in turn: logged
        (O.PREVOTE, H, 0, -1, w, s),              # 3 double prevote, against 0
        (O.PRECOMMIT, H, 0, -1, w, s),            # 4 double precommit, against 1
        (O.PREVOTE, H, 0, -1, v, s),              # 5 equal to 0: silent
        (O.PROPOSE, H, 0, -1, w, sig(1)),         # 6 double propose, against 2
        (O.PROPOSE, H, 0, -1, v, sig(2)),         # 7 out of turn
        (O.PROPOSE, H, 0, -1, v, sig(1)),         # 8 Equal to 2: silent
        (O.PRECOMMIT, H, 0, -1, O.NIL_VALUE, s),  # 9 double precommit again, against 1
    ]
    want = [(3, 1, 0), (4, 2, 1), (6, 3, 2), (7, 4, NEVER), (9, 2, 1)]
    ob = _batch(O, msgs)
    assert CC.records(ob, [O.VALID] * 10, sched) == want
    for call in (verifier.decide, verifier.decide_ordered):
        res = call(to_np(ob), np.zeros(10, np.uint8), 1, schedule=_rows(sched), catch=True)
        CC.same_caught(res, want)
        assert res.dup.tolist() == [0, 0, 3, 2, 2, 1, 3, 3, 3, 2] and res.pclass.tolist() == [3, 3, 0, 3, 3, 3, 2, 4, 1, 3]
    assert res.caught[3] == (7, "out_of_turn_propose", NEVER)
    # the same stream in two inserts: the logged messages are log positions below base
    p = pair(H, 1, sched)
    a = p.put(msgs[:3])
    assert a.caught == [] and a.logpos.tolist() == [0, 1, 2]
    b = p.put(msgs[3:])
    assert b.base == 3 and b.caught == [(3, "double_prevote", 0), (4, "double_precommit", 1), (6, "double_propose", 2),
                                        (7, "out_of_turn_propose", NEVER), (9, "double_precommit", 1)]
    c = p.put(msgs[3:])                           # inserted again: caught again, nothing kept
    assert c.base == 3 and c.kept == 0 and c.caught == b.caught


# ---- 2. overflow, then staged -----------------------------------------------------------
@pytest.mark.parametrize("with_schedule", [True, False])
def test_overflow_then_staged(gpu, oracle, with_schedule):
    """A fresh context stages 1,024 records: the mix's 1,897 (1,893) take the
    overflow columns; the same call again is staged whole."""
    sigs, sched, ob, verdicts, value_ok = CC.mix_3000(with_schedule)
    recs = CC.records(ob, verdicts, sched)
    assert len(recs) == (1897 if with_schedule else 1893)
    nb, vd, vok = to_np(ob), np.array(verdicts, np.uint8), np.array(value_ok, np.uint8)
    v = gpu.Verifier(0)
    try:
        v.set_signatories(_rows(sigs[:20]))                            # signers 20..39 take the hashed table
        rows = _rows(sched) if sched is not None else None
        first = v.decide_ordered(nb, vd, 13, schedule=rows, value_ok=vok, catch=True)
        CC.same_caught(first, recs)
        again = v.decide_ordered(nb, vd, 13, schedule=rows, value_ok=vok, catch=True)
        CC.same_caught(again, recs)
        PC.same_as(again, PC.restate(ob, verdicts, 13, sched, value_ok))
        CC.same_caught(v.decide(nb, vd, 13, schedule=rows, value_ok=vok, catch=True), recs)
    finally:
        v.close()


# ---- 3. block and wavefront borders -----------------------------------------------------
def test_borders_of_words_wavefronts_and_blocks(verifier, oracle):
    O = oracle
    sig, v, w = _setup(verifier, O)
    n, at = 4200, (63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4199)
    signer = lambda k: O.sha256(b"s" + k.to_bytes(2, "big"))           # none admitted
    msgs = [(O.PREVOTE, H, 0, -1, v, signer(k)) for k in range(n)]
    for k in at:
        msgs[k] = (O.PREVOTE, H, 0, -1, w, signer(0))
    ob = _batch(O, msgs)
    want = [(k, 1, 0) for k in at]
    assert CC.records(ob, [O.VALID] * n) == want
    CC.same_caught(verifier.decide(to_np(ob), np.zeros(n, np.uint8), 1, catch=True), want)


@pytest.mark.parametrize("signer", [0, 9])
def test_one_logged_vote_and_699_conflicts(verifier, oracle, signer):
    O = oracle
    sig, v, w = _setup(verifier, O)
    ob = _batch(O, [(O.PREVOTE, H, 0, -1, v, sig(signer))] + [(O.PREVOTE, H, 0, -1, w, sig(signer))] * 699)
    want = [(k, 1, 0) for k in range(1, 700)]
    assert CC.records(ob, [O.VALID] * 700) == want
    CC.same_caught(verifier.decide_ordered(to_np(ob), np.zeros(700, np.uint8), 1, catch=True), want)


# ---- 4. nothing to report ---------------------------------------------------------------
def test_nothing_to_report(verifier, oracle):
    from hyperdrive_amd import _lib
    O = oracle
    sig, v, w = _setup(verifier, O)
    ob = _batch(O, [(O.PREVOTE if k % 2 else O.PRECOMMIT, H, k % 3, -1, v, O.sha256(b"h" + bytes([k // 2])))
                    for k in range(500)])
    assert CC.records(ob, [O.VALID] * 500) == []
    res = verifier.decide(to_np(ob), np.zeros(500, np.uint8), 1, catch=True)
    assert res.caught == [] and len(res.caught_index) == 0 and not res.dup.any()
    rc, o, a, when, until, c, ca = _raw_decide(verifier, ob, [O.VALID] * 500, 1, catch_cap=0, null_arrays=True)
    assert (rc, c.n, o.n) == (_lib.HD_OK, 0, 3)
    # an empty batch
    rc, o, a, when, until, c, ca = _raw_decide(verifier, O.Batch(), [], 1)
    assert (rc, c.n, o.n) == (_lib.HD_OK, 0, 0)
    assert verifier.decide(to_np(O.Batch()), np.zeros(0, np.uint8), 1, catch=True).caught == []


# ---- 5. capacity ------------------------------------------------------------------------
def test_capacity(verifier, oracle, pair):
    from hyperdrive_amd import _lib
    from hyperdrive_amd.verify import _catch_struct
    lib = _lib.load()
    O = oracle
    sigs, sched, ob, verdicts, value_ok = CC.mix_40()
    verifier.set_signatories(_rows(sigs[:5]))
    recs = CC.records(ob, verdicts, sched)
    rows = len(PC.restate(ob, verdicts, 2, sched, None).rows)
    assert len(recs) == 4 and rows >= 2
    rc, o, a, when, until, c, ca = _raw_decide(verifier, ob, verdicts, 2, sched, catch_cap=3)
    assert (rc, c.n, o.n) == (_lib.HD_ECAP, 4, rows)
    rc, o, a, when, until, c, ca = _raw_decide(verifier, ob, verdicts, 2, sched, catch_cap=3, out_cap=rows - 1)
    assert (rc, c.n, o.n) == (_lib.HD_ECAP, 4, rows)                   # both needs
    rc, o, a, when, until, c, ca = _raw_decide(verifier, ob, verdicts, 2, sched, catch_cap=0, null_arrays=True)
    assert (rc, c.n) == (_lib.HD_ECAP, 4)                              # count only
    rc, o, a, when, until, c, ca = _raw_decide(verifier, ob, verdicts, 2, sched, catch_cap=4)
    assert rc == _lib.HD_OK and _list(c, ca) == recs
    # cap > 0 with a NULL array: HD_EINVAL before any device work
    rc, o, a, when, until, c, ca = _raw_decide(verifier, ob, verdicts, 2, sched, catch_cap=4, null_arrays=True)
    assert rc == _lib.HD_EINVAL
    # on a log: the refused insert leaves the log as it was, and the same insert with room succeeds
    p = pair(H, 2, sched)
    p.put(*LC.cut(ob, verdicts, value_ok, 0, 10))
    entries = p.log.entries
    part, pv, _ = LC.cut(ob, verdicts, value_ok, 10, 40)
    need = len(p.ys.peek_caught(part, pv))
    assert need >= 2
    nb, vd = to_np(part), np.array(pv, np.uint8)
    cb = nb.c_struct()
    for short_rows in (False, True):
        o, a, w_, when, until, logpos, info = p.log._outputs(30)
        c, ca = _catch_struct(30)
        c.cap = need - 1
        if short_rows:
            o.cap = 1
        rc = lib.hd_log_insert_catch(p.log.handle, ctypes.byref(cb), vd.ctypes.data, None, ctypes.byref(o),
                                     ctypes.byref(w_), ctypes.byref(info), ctypes.byref(c))
        assert (rc, c.n, p.log.entries) == (_lib.HD_ECAP, need, entries)
        assert o.n >= 2
    o, a, w_, when, until, logpos, info = p.log._outputs(30)
    assert lib.hd_log_insert_catch(p.log.handle, ctypes.byref(cb), vd.ctypes.data, None, ctypes.byref(o),
                                   ctypes.byref(w_), ctypes.byref(info), None) == _lib.HD_EINVAL
    assert p.log.entries == entries
    p.put(part, pv)                                                    # the full answer


def test_log_without_class_arrays(verifier, oracle, pair):
    """hd_log_insert_catch with out->dup, out->pclass or both NULL: the list,
    the rows and the class array that is taken are what the full call gives."""
    from hyperdrive_amd import _lib
    from hyperdrive_amd.verify import _catch_struct
    lib = _lib.load()
    sigs, sched, ob, verdicts, value_ok = CC.mix_40()
    verifier.set_signatories(_rows(sigs[:5]))
    part, pv, _ = LC.cut(ob, verdicts, value_ok, 10, 40)
    nb, vd = to_np(part), np.array(pv, np.uint8)
    cb = nb.c_struct()
    for no_dup, no_pclass in ((True, True), (True, False), (False, True)):
        p = pair(H, 2, sched)
        p.put(*LC.cut(ob, verdicts, value_ok, 0, 10))
        exp, recs = p.ys.push(part, pv)
        o, a, w_, when, until, logpos, info = p.log._outputs(30)
        c, ca = _catch_struct(30)
        if no_dup:
            o.dup = None
        if no_pclass:
            o.pclass = None
        rc = lib.hd_log_insert_catch(p.log.handle, ctypes.byref(cb), vd.ctypes.data, None, ctypes.byref(o),
                                     ctypes.byref(w_), ctypes.byref(info), ctypes.byref(c))
        assert rc == _lib.HD_OK and _list(c, ca) == recs and len(recs) == 4
        assert (info.base, info.kept, o.n) == (exp.base, exp.kept, len(exp.rows)) and logpos[:30].tolist() == exp.logpos
        assert when[: o.n].tolist() == exp.when
        assert a["dup"][:30].tolist() == ([0] * 30 if no_dup else exp.dup)
        assert a["pclass"][:30].tolist() == ([0] * 30 if no_pclass else exp.pclass)
        p.put([])                                                      # the log and the yardstick still agree


# ---- 6. the same outputs with and without the list --------------------------------------
def test_same_outputs_with_and_without_the_list(verifier, oracle):
    from hyperdrive_amd import _lib
    O = oracle
    sigs, sched, ob, verdicts, value_ok = CC.mix_5000()
    verifier.set_signatories(_rows(sigs[:6]))
    nb, vd = to_np(ob), np.array(verdicts, np.uint8)
    recs = CC.records(ob, verdicts, sched)
    fields = list(PC.ROW_FIELDS) + ["dup", "pclass"]
    plain = verifier.decide(nb, vd, 3, schedule=_rows(sched))
    listed = verifier.decide(nb, vd, 3, schedule=_rows(sched), catch=True)
    assert type(plain).__name__ == "DecideResult" and not hasattr(plain, "caught")
    for k in fields:
        assert getattr(plain, k).tolist() == getattr(listed, k).tolist(), k
    CC.same_caught(listed, recs)
    plain = verifier.decide_ordered(nb, vd, 3, schedule=_rows(sched))
    listed = verifier.decide_ordered(nb, vd, 3, schedule=_rows(sched), catch=True)
    for k in fields + ["when", "exact_until"]:
        assert getattr(plain, k).tolist() == getattr(listed, k).tolist(), k
    CC.same_caught(listed, recs)
    assert (plain.when != NEVER).sum() > 4
    # neither class array: the list and the rows are unchanged
    for ordered in (False, True):
        rc, o, a, when, until, c, ca = _raw_decide(verifier, ob, verdicts, 3, sched, ordered=ordered, classes=False)
        assert rc == _lib.HD_OK and _list(c, ca) == recs and o.n == len(plain)
        assert not a["dup"].any() and not a["pclass"].any()            # not written
        rc2, o2, a2, when2, until2, c2, ca2 = _raw_decide(verifier, ob, verdicts, 3, sched, ordered=ordered)
        for k in PC.ROW_FIELDS:
            assert a[k][: o.n].tolist() == a2[k][: o2.n].tolist() == getattr(plain, k).tolist(), k
        assert a2["dup"][:5000].tolist() == plain.dup.tolist() and a2["pclass"][:5000].tolist() == plain.pclass.tolist()
        if ordered:
            assert when[: o.n].tolist() == plain.when.tolist() and until[: o.n].tolist() == plain.exact_until.tolist()


# ---- 7. a log, every cut ----------------------------------------------------------------
def test_log_every_cut(verifier, oracle, pair):
    sigs, sched, ob, verdicts, value_ok = CC.mix_40()
    verifier.set_signatories(_rows(sigs[:5]))
    p = pair(H, 2, sched)
    below = total = 0
    for c in range(1, 40):
        p.reset(H)
        a = p.put(*LC.cut(ob, verdicts, value_ok, 0, c))
        b = p.put(*LC.cut(ob, verdicts, value_ok, c, 40))
        total = len(a.caught) + len(b.caught)
        below += sum(1 for _, _, x in b.caught if x < b.base)
        assert total == 4
    assert below > 0


# ---- 8. a log, pieces -------------------------------------------------------------------
PIECES = (1, 63, 64, 65, 255, 257, 700)


@pytest.mark.parametrize("f,with_schedule", [(13, True), (3, False)])
def test_log_pieces(verifier, oracle, pair, f, with_schedule):
    sigs, sched, ob, verdicts, value_ok = CC.mix_3000(with_schedule)
    verifier.set_signatories(_rows(sigs[:20]))                        # signers 20..39 take the hashed table
    p = pair(H, f, sched)
    lo, k, caught, below = 0, 0, 0, 0
    while lo < len(ob):
        hi = min(lo + PIECES[k % len(PIECES)], len(ob))
        res = p.put(*LC.cut(ob, verdicts, value_ok, lo, hi))
        caught += len(res.caught)
        below += sum(1 for _, _, x in res.caught if x < res.base)
        if k == 4:                                                     # the same 255 messages again
            again = p.put(*LC.cut(ob, verdicts, value_ok, lo, hi))
            assert again.kept == 0 and len(res.caught) > 0
            assert {(i - res.base, kd) for i, kd, _ in res.caught} <= {(i - again.base, kd) for i, kd, _ in again.caught}
            assert all(x < again.base for _, kd, x in again.caught if kd != "out_of_turn_propose")
        lo, k = hi, k + 1
    assert caught == (1897 if with_schedule else 1893) and below > 1000


# ---- 9. the device entries --------------------------------------------------------------
def test_device_entries(verifier, oracle):
    import torch
    from hyperdrive_amd import quorum
    from hyperdrive_amd.device import generate, work_stream
    O = oracle
    S, n, m = 100, 8192, 2048
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
    sched = [bytes(r) for r in ks[0]]
    recs = CC.records(from_np(hb), hv.tolist(), sched)
    kinds = sorted({k for _, k, _ in recs})
    assert len(recs) > 50 and len(kinds) >= 2, (len(recs), kinds)
    whole = verifier.decide_ordered_device(cs, bitmap.data_ptr(), f, schedule=ks[0], stream=ws.cuda_stream, catch=True)
    host = verifier.decide_ordered(hb, hv, f, schedule=ks[0], catch=True)
    CC.same_caught(whole, recs)
    CC.same_caught(host, recs)
    CC.same_caught(verifier.decide_device(cs, bitmap.data_ptr(), f, schedule=ks[0], stream=ws.cuda_stream, catch=True),
                   recs)
    assert whole.dup.tolist() == host.dup.tolist() and whole.when.tolist() == host.when.tolist()
    # four slices into a log: the whole batch's records under the index map of the log positions
    log = verifier.open_log(1, f, ks[0])
    try:
        pos = np.full(n, NEVER, np.uint32)
        got = 0
        for k in range(n // m):
            lo = k * m
            part = db.rows(lo, m).c_struct()
            res = log.insert_device(part, bitmap.data_ptr() + 4 * (lo // 32), stream=ws.cuda_stream, catch=True)
            pos[lo: lo + m] = res.logpos
            ix = lambda i: NEVER if i == NEVER else (int(pos[i]) if i < lo else res.base + (i - lo))
            CC.same_caught(res, [(res.base + (i - lo), kd, ix(a)) for i, kd, a in recs if lo <= i < lo + m])
            assert NEVER not in [a for _, kd, a in res.caught if kd != "out_of_turn_propose"]
            got += len(res.caught)
        assert got == len(recs)
    finally:
        log.close()


# ---- 10. ingress -------------------------------------------------------------------------
def test_ingress_flush_decide_catch(verifier, oracle):
    import torch
    from hyperdrive_amd.device import DeviceBatch, generate
    from hyperdrive_amd.ingress import Ingress
    O = oracle
    S, n = 20, 2 * 20 * 6                                              # six heights of 40 votes
    db, sigs, _ = generate(verifier, 0, n, S, adv_pct=10, start=0)
    verifier.set_signatories(sigs)
    H0 = int(db.height.min().item())
    perm = torch.from_numpy(np.random.default_rng(8).permutation(n)).cuda()
    half = lambda idx: DeviceBatch(int(idx.numel()), *(getattr(db, k)[idx].contiguous()
                                                        for k in ("type", "height", "round", "valid_round", "value",
                                                                  "frm", "sig")))
    ing = Ingress(verifier, height=H0)
    try:
        ing.open_log()
        ys = [CC.Stream(H0, S // 3)]

        def flush():
            res, dec = ing.flush_decide(catch=True)
            ob = from_np(res.consumed)
            exp, recs = ys[0].push(ob, [O.VALID] * len(ob))
            LC.same_insert(dec, exp)
            CC.same_caught(dec, recs)
            return res, dec

        ing.push_device(half(perm[: n // 2]))
        r1, d1 = flush()
        ing.push_device(half(perm[n // 2:]))
        r2, d2 = flush()                                               # the same height again: the log carries over
        assert d2.base == d1.kept > 0
        assert ing.reset_height(H0 + 1, sigs[: S - 3])
        ys[0] = CC.Stream(H0 + 1, (S - 3) // 3)
        r3, d3 = flush()
        ing.advance_height(H0 + 2)
        ys[0] = CC.Stream(H0 + 2, (S - 3) // 3)
        r4, d4 = flush()
        assert d3.base == 0 and d4.base == 0 and d4.kept > 10
        caught = [len(d.caught) for d in (d1, d2, d3, d4)]
        assert sum(caught) > 0, caught
    finally:
        ing.close()


# ---- 11. a shared context ------------------------------------------------------------------
def test_shares_the_context(verifier, oracle, pair):
    """A tally, a decide without the list and a second log between catching
    inserts: every call keeps its own exact result, so the tables are clean
    after the catch passes."""
    O = oracle
    rng = random.Random(44)
    sigs = [O.sha256(b"i" + bytes([k])) for k in range(30)]
    vals = [O.canonical_value(H, k) for k in range(2)] + [O.NIL_VALUE]
    verifier.set_signatories(_rows(sigs[:15]))
    ob, verdicts, value_ok = WC.mix(rng, 1200, [H], list(range(4)), sigs, vals, 1 / 8)
    other, overd, ook = WC.mix(rng, 900, [1, 2, 3], list(range(5)), sigs, vals, 1 / 8)
    nb, ov = to_np(other), np.array(overd, np.uint8)
    p, q = pair(H, 3), pair(H, 9, sigs)
    a = p.put(*LC.cut(ob, verdicts, value_ok, 0, 500))
    tal, ot = verifier.tally(nb, ov), O.tally(other, overd)
    assert (tal.count, tal.distinct, tal.dup.tolist()) == (ot.count, ot.distinct, ot.dup)
    q.put(*LC.cut(ob, verdicts, value_ok, 600, 900))                   # a second log on the context
    PC.same_as(verifier.decide(nb, ov, 3, value_ok=np.array(ook, np.uint8)), PC.restate(other, overd, 3, None, ook))
    b = p.put(*LC.cut(ob, verdicts, value_ok, 500, 1200))
    res = verifier.decide_ordered(nb, ov, 3, value_ok=np.array(ook, np.uint8), catch=True)
    WC.same_when(res, WC.replay(other, overd, 3, None, ook))
    CC.same_caught(res, CC.records(other, overd))
    q.put(*LC.cut(ob, verdicts, value_ok, 0, 600))
    tal = verifier.tally(nb, ov)
    assert (tal.count, tal.distinct, tal.dup.tolist()) == (ot.count, ot.distinct, ot.dup)
    p.put(*LC.cut(ob, verdicts, value_ok, 0, 100))
    assert len(a.caught) > 20 and len(b.caught) > 20 and len(res.caught) > 20
