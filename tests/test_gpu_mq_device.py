"""The consume into device memory (include/hd_mq.h hd_mq_consume_device;
MessageQueue.consume_device, mq.Taken, Ingress.flush_decide_device).

Yardsticks: oracle/mq_oracle.py ``consume(allowed=...)`` for the delivery,
tests/log_cases.py ``Stream`` for the insert results, and a twin queue or
Ingress on the existing host path, fed identically, as a second opinion.
Every comparison is exact.  The queue-only scenarios come from
tests/mq_device_cases.py, whose table the CPU suite checks against the oracle
(tests/test_mqtake_host.py); their messages go in through insert_device, which
takes any bytes as a signature.  The Ingress cases generate and verify signed
messages as test_gpu_log.py's ingress case does."""
import ctypes

import numpy as np
import pytest

from hyperdrive_amd._lib import HDError

import log_cases as LC
import mq_device_cases as C
import propose_cases as PC
from util import from_np

pytestmark = pytest.mark.gpu

EINVAL, ECAP = -1, -4


@pytest.fixture(scope="module")
def verifier(gpu):
    v = gpu.Verifier(0)
    yield v
    v.close()


# ---- helpers ---------------------------------------------------------------------------
def _insert(q, rows, vr_null):
    import torch
    n = len(rows)
    col = lambda k, dt: np.array([m[k] for m in rows], dt)
    blob = lambda k, w: np.frombuffer(b"".join(m[k] for m in rows), np.uint8).reshape(n, w).copy()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    cols = [t(col(2, np.uint8)), t(col(0, np.int64)), t(col(1, np.int64)), t(col(3, np.int64)), t(blob(4, 32)),
            t(blob(5, 32)), t(blob(6, 65))]
    if not vr_null:
        from hyperdrive_amd.device import DeviceBatch
        q.insert_device(DeviceBatch(n, *cols))
        return
    # a batch without a valid_round column: the C entry point directly
    from hyperdrive_amd._lib import HdBatch
    torch.cuda.synchronize()
    cs = HdBatch(n, cols[0].data_ptr(), cols[1].data_ptr(), cols[2].data_ptr(), None, cols[4].data_ptr(),
                 cols[5].data_ptr(), cols[6].data_ptr())
    q._check(q._lib.hd_mq_insert_device(q._q, ctypes.byref(cs), None, None), "hd_mq_insert_device")


def _allowed(sc):
    """procsAllowed as the queue takes it: rows of 32 bytes, or None for the admitted set"""
    if sc.allowed is None:
        return None
    return np.frombuffer(b"".join(sc.allowed), np.uint8).reshape(len(sc.allowed), 32).copy()


def _filled(gpu, verifier, sc, count=2):
    from hyperdrive_amd.mq import MessageQueue
    qs = [MessageQueue(verifier, sc.capacity) for _ in range(count)]
    for q in qs:
        for rows in sc.batches:
            _insert(q, rows, sc.vr_null)
    return qs


def _rows(b):
    return [(int(b.height[i]), int(b.round[i]), int(b.type[i]), int(b.valid_round[i]), b.value[i].tobytes(),
             b.frm[i].tobytes(), b.sig[i].tobytes()) for i in range(len(b))]


def _same_delivery(got_batch, got_senders, want):
    """every column and the sender ids against the oracle's [(sender id, row)]"""
    assert len(got_batch) == len(want)
    assert np.asarray(got_senders).tolist() == [s for s, _ in want]
    rows, exp = _rows(got_batch), [m for _, m in want]
    for k in range(7):                      # height, round, type, valid_round, value, From, 65 signature bytes
        assert [r[k] for r in rows] == [m[k] for m in exp], k


def _bitmap_words(n):
    return [(1 << min(32, n - 32 * w)) - 1 for w in range((n + 31) // 32)]


def _device_state(taken):
    vok, bitmap, snd = taken.tensors()
    return vok.cpu().numpy(), (bitmap.cpu().numpy().astype(np.int64) & 0xFFFFFFFF).tolist(), snd.cpu().numpy()


# ---- 1. the delivery equals the oracle's and the host path's ------------------------------
@pytest.mark.parametrize("name", C.DELIVERY)
def test_delivery_equals_the_oracle_and_the_host_path(gpu, verifier, name):
    sc = C.scenario(name)
    want = C.run_oracle(sc)
    q, twin = _filled(gpu, verifier, sc)
    try:
        removed, got, left = want[0]
        taken = q.consume_device(C.H, _allowed(sc))
        b, snd = twin.consume(C.H, _allowed(sc))
        assert (taken.n, taken.removed, q.last_removed) == (len(got), removed, removed)
        assert (len(b), twin.last_removed) == (len(got), removed)
        assert len(q) == len(twin) == left and q.senders == twin.senders == sc.expect["senders"]
        tb, ts = taken.read()
        _same_delivery(tb, ts, got)
        _same_delivery(b, snd, got)
        assert taken.batch.n == taken.n == len(taken)
        if taken.n:
            vok, bitmap, dsnd = _device_state(taken)
            assert vok.tolist() == [1] * taken.n and bitmap == _bitmap_words(taken.n)
            assert dsnd.tolist() == [s for s, _ in got]
        if sc.vr_null:
            assert len(got) > 0 and (tb.valid_round == -1).all()
        # the heads were committed right: the later heights come out equal on the host path
        for h, (rem, later, left) in zip(C.LATER, want[1:]):
            b1, s1 = q.consume(h, _allowed(sc))
            b2, s2 = twin.consume(h, _allowed(sc))
            _same_delivery(b1, s1, later)
            _same_delivery(b2, s2, later)
            assert q.last_removed == twin.last_removed == rem and len(q) == len(twin) == left
    finally:
        q.close()
        twin.close()


# ---- 2. read by index ------------------------------------------------------------------
def test_read_by_index(gpu, verifier):
    sc = C.scenario("d257")
    (_, got, _), *_ = C.run_oracle(sc)
    q, = _filled(gpu, verifier, sc, 1)
    try:
        taken = q.consume_device(C.H, _allowed(sc))
        n = taken.n
        assert n == 257
        rng = np.random.default_rng(5)
        for idx in (np.arange(n)[::-1], np.array([0, 0, n - 1, 5, n - 1, 0, 256, 255]), rng.integers(0, n, 600),
                    np.array([n - 1]), np.zeros(0, np.uint32)):
            b, s = taken.read(idx)
            _same_delivery(b, s, [got[int(i)] for i in idx])
        for first, m in ((0, n), (0, 1), (1, 255), (255, 2), (256, 1), (n, 0), (100, None)):
            b, s = taken.read(first=first, n=m)
            _same_delivery(b, s, got[first: n if m is None else first + m])
        for bad in (dict(idx=[n]), dict(idx=[0, 1, 0xFFFFFFFF]), dict(first=n, n=1), dict(first=n + 1, n=0),
                    dict(first=1, n=n), dict(first=0xFFFFFFFF, n=2)):
            with pytest.raises(HDError) as e:
                taken.read(**bad)
            assert e.value.code == EINVAL
        b, s = taken.read()                                    # a refused read changes nothing
        _same_delivery(b, s, got)
    finally:
        q.close()


# ---- 3. the prefetch window ------------------------------------------------------------
def test_a_staged_prefetch_window_is_committed_first(gpu, verifier):
    sc = C.scenario("window")
    heights = (C.H, C.H + 1, C.H + 2, C.H + 3)
    want = C.run_oracle(sc, heights)
    assert all(len(got) > 0 for _, got, _ in want[:3])
    verifier.set_signatories(np.frombuffer(b"".join(sc.admitted), np.uint8).reshape(-1, 32).copy())
    q, twin = _filled(gpu, verifier, sc)
    try:
        b, s = q.consume(C.H)                                  # admitted-set mode: stages the next heights
        _same_delivery(b, s, want[0][1])
        _same_delivery(*twin.consume(C.H), want[0][1])
        assert len(q) == len(twin) == want[0][2]
        taken = q.consume_device(C.H + 1)                      # must see the window's consumes committed
        b2, s2 = twin.consume(C.H + 1)
        _same_delivery(*taken.read(), want[1][1])
        _same_delivery(b2, s2, want[1][1])
        assert (taken.removed, twin.last_removed) == (want[1][0], want[1][0])
        assert len(q) == len(twin) == want[1][2]
        for k in (2, 3):
            _same_delivery(*q.consume(heights[k]), want[k][1])
            _same_delivery(*twin.consume(heights[k]), want[k][1])
            assert q.last_removed == twin.last_removed == want[k][0] and len(q) == len(twin) == want[k][2]
    finally:
        q.close()
        twin.close()


# ---- 4. the view's lifetime as specified -------------------------------------------------
def test_two_device_consumes_in_a_row(gpu, verifier):
    sc = C.scenario("p_two")
    first, second, _ = C.run_oracle(sc)
    q, = _filled(gpu, verifier, sc, 1)
    try:
        t1 = q.consume_device(C.H, _allowed(sc))
        assert len(t1.proposes) == 2
        t1.set_value_ok([1, 0])
        t2 = q.consume_device(C.LATER[0], _allowed(sc))
        assert (t2.n, t2.removed) == (len(second[1]), second[0]) and t2.n > 0 and len(q) == second[2]
        _same_delivery(*t2.read(), second[1])
        vok, bitmap, dsnd = _device_state(t2)
        assert vok.tolist() == [1] * t2.n and bitmap == _bitmap_words(t2.n)
        assert len(t2.proposes) == 0                           # the later heights hold votes only
        with pytest.raises(HDError) as e:
            t1.set_value_ok([1, 0])                            # the first delivery's count: it has ended
        assert e.value.code == EINVAL
        t2.set_value_ok([])
        # a call that changes the queue ends the delivery
        q.drop_below(0)
        for call in (t2.read, lambda: t2.set_value_ok([])):
            with pytest.raises(HDError) as e:
                call()
            assert e.value.code == EINVAL
    finally:
        q.close()


# ---- 5. propose rows -------------------------------------------------------------------
@pytest.mark.parametrize("name", C.PROPOSES)
def test_propose_rows(gpu, verifier, name):
    sc = C.scenario(name)
    (_, got, _), *_ = C.run_oracle(sc)
    where = [k for k, (_, m) in enumerate(got) if m[2] == C.PROPOSE]
    q, = _filled(gpu, verifier, sc, 1)
    try:
        taken = q.consume_device(C.H, _allowed(sc))
        p = taken.proposes
        assert p.index.tolist() == where and len(p) == len(where)
        b, s = taken.read(p.index)
        assert p.sender.tolist() == s.tolist() == [got[k][0] for k in where]
        assert (p.type == C.PROPOSE).all() and (b.type == C.PROPOSE).all()
        for key in ("height", "round", "valid_round", "value", "frm"):
            assert getattr(p, key).tolist() == getattr(b, key).tolist(), key
        ok = np.array([k % 2 for k in range(len(where))], np.uint8)         # zeros at every other propose
        taken.set_value_ok(ok)
        want = np.ones(taken.n, np.uint8)
        want[[where[k] for k in range(len(where)) if ok[k] == 0]] = 0
        assert _device_state(taken)[0].tolist() == want.tolist()
        taken.set_value_ok(1 - ok)                                            # and a second answer replaces the first
        want = np.ones(taken.n, np.uint8)
        want[[where[k] for k in range(len(where)) if ok[k] == 1]] = 0
        assert _device_state(taken)[0].tolist() == want.tolist()
        with pytest.raises(HDError) as e:
            taken.set_value_ok(np.ones(len(where) + 1, np.uint8))
        assert e.value.code == EINVAL
    finally:
        q.close()


# ---- 6. flush_decide_device against flush_decide -----------------------------------------
def _same_batch(a, b):
    for key in ("type", "height", "round", "valid_round", "value", "frm", "sig"):
        assert getattr(a, key).tolist() == getattr(b, key).tolist(), key


def _ingress_run(verifier, O, full, reject):
    """test_gpu_log.py's ingress scenario on twin Ingresses, with the two
    rounds' proposes of the first height added: 20 signatories, six heights,
    two pushes of one height, a reset_height to a smaller set and an
    advance_height.  Returns the device path's results per flush."""
    import torch
    from hyperdrive_amd.device import DeviceBatch, generate
    from hyperdrive_amd.ingress import Ingress
    S, n = 20, 2 * 20 * 6
    ks = verifier.gen_keys(S)
    votes, sigs, _ = generate(verifier, 0, n, S, adv_pct=10, start=0, keys=ks)
    rounds, _, _ = generate(verifier, 1, 2 * (1 + 2 * S), S, adv_pct=0, start=0, keys=ks)   # height 1: rounds 0, 1
    verifier.set_signatories(sigs)
    keys = ("type", "height", "round", "valid_round", "value", "frm", "sig")
    db = DeviceBatch(votes.n + rounds.n, *(torch.cat([getattr(votes, k), getattr(rounds, k)]).contiguous()
                                           for k in keys))
    H0 = int(db.height.min().item())
    perm = torch.from_numpy(np.random.default_rng(8).permutation(db.n)).cuda()
    half = lambda idx: DeviceBatch(int(idx.numel()), *(getattr(db, k)[idx].contiguous() for k in keys))
    bad = bytes(O.canonical_value(H0, 0)) if reject else None
    rows32 = lambda a: [bytes(r) for r in np.asarray(a)]
    dev_ok = (lambda p: np.array([v != bad for v in rows32(p.value)], np.uint8)) if reject else None
    host_ok = (lambda b: np.array([not (t == C.PROPOSE and v == bad) for t, v in zip(b.type, rows32(b.value))],
                                  np.uint8)) if reject else None
    dev, twin = Ingress(verifier, height=H0), Ingress(verifier, height=H0)
    out, proposes = [], 0
    try:
        for ing in (dev, twin):
            ing.open_log(keep_signatures=full)
        ys = [LC.Stream(H0, S // 3)]

        def flush():
            nonlocal proposes
            taken, dd = dev.flush_decide_device(value_ok=dev_ok, catch=full, evidence=full)
            res, dh = twin.flush_decide(value_ok=host_ok, catch=full, evidence=full)
            assert (taken.n, taken.removed) == (len(res.consumed), res.removed) and taken.n == len(dd.dup)
            _same_batch(taken.read()[0], res.consumed)
            assert taken.read()[1].tolist() == res.senders.tolist()
            assert taken.proposes.index.tolist() == res.proposes.tolist()
            proposes += len(res.proposes)
            ob = from_np(res.consumed)
            vok = None if not reject else host_ok(res.consumed).tolist()
            LC.same_insert(dd, ys[0].push(ob, [O.VALID] * len(ob), vok))
            assert (dd.base, dd.kept, dd.relogged) == (dh.base, dh.kept, dh.relogged)
            for key in PC.ROW_FIELDS:
                assert getattr(dd, key).tolist() == getattr(dh, key).tolist(), key
            for key in ("when", "exact_until", "logpos", "dup", "pclass"):
                assert getattr(dd, key).tolist() == getattr(dh, key).tolist(), key
            assert dev.log.entries == twin.log.entries == dd.base + dd.kept
            if full:
                assert dd.caught == dh.caught
                _same_batch(dd.evidence_offender, dh.evidence_offender)
                _same_batch(dd.evidence_against, dh.evidence_against)
                assert dd.evidence_offender_value_ok.tolist() == dh.evidence_offender_value_ok.tolist()
                assert dd.evidence_against_value_ok.tolist() == dh.evidence_against_value_ok.tolist()
            out.append(dd)
            return dd

        for ing in (dev, twin):
            ing.push_device(half(perm[: db.n // 2]))
        d1 = flush()
        for ing in (dev, twin):
            ing.push_device(half(perm[db.n // 2:]))
        d2 = flush()                                             # the same height again: the log carries over
        assert d2.base == d1.kept > 0 and d1.new_firings != [] and proposes == 2
        if full:
            assert len(d1.caught) + len(d2.caught) > 0 and d2.evidence_offender.sig.any()
        for ing in (dev, twin):
            assert ing.reset_height(H0 + 1, sigs[: S - 3])       # ResetHeight with a smaller set
        assert (dev.log.height, dev.log.entries, dev.log.f) == (H0 + 1, 0, (S - 3) // 3)
        ys[0] = LC.Stream(H0 + 1, (S - 3) // 3)
        d3 = flush()
        assert d3.base == 0 and d3.kept > 10
        for ing in (dev, twin):
            ing.advance_height(H0 + 2)
        ys[0] = LC.Stream(H0 + 2, (S - 3) // 3)
        d4 = flush()
        assert d4.base == 0 and d4.kept > 10
        d5 = flush()                                             # nothing buffered at the height: an empty delivery
        assert (d5.base, d5.kept, len(d5.dup)) == (d4.kept, 0, 0) and d5.firings == d4.firings
    finally:
        dev.close()
        twin.close()
    return out


@pytest.fixture(scope="module")
def plain_run(verifier, oracle):
    return _ingress_run(verifier, oracle, full=False, reject=False)


def test_flush_decide_device_equals_flush_decide(plain_run):
    assert len(plain_run) == 5


def test_flush_decide_device_with_catch_and_evidence(verifier, oracle):
    _ingress_run(verifier, oracle, full=True, reject=False)


def test_flush_decide_device_with_a_rejected_value(verifier, oracle, plain_run):
    got = _ingress_run(verifier, oracle, full=False, reject=True)
    # (inside the run: equal to the twin, which was given the per-message bytes, and to the yardstick)
    state = lambda run: [(d.trace.tolist(), d.bits.tolist()) for d in run]
    assert state(got)[:2] != state(plain_run)[:2]               # the rejected propose is not traced as valid
    assert state(got)[2:] == state(plain_run)[2:]               # the other heights hold no propose


# ---- 7. a failing insert keeps the view ---------------------------------------------------
def test_a_failing_insert_keeps_the_view(gpu, verifier, oracle):
    sc = C.scenario("p_two")
    q, = _filled(gpu, verifier, sc, 1)
    log = verifier.open_log(C.H, 1)
    try:
        taken = q.consume_device(C.H, _allowed(sc))
        ob = from_np(taken.read()[0])
        o, a, w, when, until, logpos, info = log._outputs(taken.n)
        o.cap = 0                                                # no room for a single row
        rc = log._lib.hd_log_insert_device_bitmap(log._log, ctypes.byref(taken.batch), taken.d_bitmap,
                                                  taken.d_value_ok, ctypes.byref(o), ctypes.byref(w),
                                                  ctypes.byref(info), None)
        assert rc == ECAP and o.n > 0 and log.entries == 0
        res = log.insert_device(taken.batch, taken.d_bitmap, taken.d_value_ok)
        LC.same_insert(res, LC.Stream(C.H, 1).push(ob, [oracle.VALID] * len(ob)))
        assert res.kept > 0 and log.entries == res.kept
        _same_delivery(*taken.read(), C.run_oracle(sc)[0][1])   # the view is still the delivery
    finally:
        log.close()
        q.close()
