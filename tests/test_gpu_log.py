"""hd_log (include/hd_log.h; Verifier.open_log, DecideLog, Ingress.flush_decide)
against the yardstick of tests/log_cases.py: after every insert the library's
rows, when, exact_until, pclass, dup, logpos, base, kept, relogged and
new_firings equal the one-shot decide of everything inserted so far, in the
call's joined coordinates.  Verdicts are passed directly and the signatures are
65 zero bytes, as in tests/test_gpu_decide_ordered.py; only the device-entry
and ingress cases verify generated batches first."""
import ctypes
import random

import numpy as np
import pytest

import log_cases as LC
import propose_cases as PC
import when_cases as WC
from util import from_np, to_np

pytestmark = pytest.mark.gpu

NEVER = LC.NEVER
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
    """A library log and the yardstick fed side by side."""

    def __init__(self, verifier, O, height, f, schedule=None, max_entries=0):
        self.O = O
        self.log = verifier.open_log(height, f, _rows(schedule) if schedule is not None else None, max_entries)
        self.ys = LC.Stream(height, f, schedule)

    def put(self, msgs, verdicts=None, value_ok=None):
        ob = msgs if hasattr(msgs, "mtype") else _batch(self.O, msgs)
        verdicts = [self.O.VALID] * len(ob) if verdicts is None else verdicts
        res = self.log.insert(to_np(ob), np.array(verdicts, np.uint8),
                              None if value_ok is None else np.array(value_ok, np.uint8))
        LC.same_insert(res, self.ys.push(ob, verdicts, value_ok))
        assert self.log.entries == self.ys.entries == res.base + res.kept
        return res

    def reset(self, height, f=None, schedule=None):
        self.log.reset(height, f, _rows(schedule) if schedule is not None else None)
        self.ys = LC.Stream(height, self.ys.f if f is None else f, self.ys.schedule if schedule is None else schedule)
        assert (self.log.height, self.log.entries) == (height, 0)

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


def _when(res, r):
    hit = [j for j in range(len(res)) if int(res.round[j]) == r]
    assert len(hit) == 1, (r, hit)
    return res.when[hit[0]].tolist(), int(res.exact_until[hit[0]]), int(res.bits[hit[0]])


# ---- 1. every cut of a small stream ------------------------------------------------
def test_every_cut_of_a_small_stream(verifier, oracle, pair):
    O = oracle
    rng = random.Random(41)
    sigs = [O.sha256(b"a" + bytes([k])) for k in range(7)]
    vals = [O.canonical_value(H, k) for k in range(2)] + [O.NIL_VALUE]
    verifier.set_signatories(_rows(sigs[:5]))
    ob, verdicts, value_ok = WC.mix(rng, 40, [H], [-1, 0, 1, 2], sigs, vals, 1 / 8, sigs, valid_rounds=(-1, 0, 1, 2))
    p = pair(H, 2, sigs)
    fired = set()
    for c in range(1, 40):
        p.reset(H)
        p.put(*LC.cut(ob, verdicts, value_ok, 0, c))
        fired |= {k for _, _, _, k in p.put(*LC.cut(ob, verdicts, value_ok, c, 40)).new_firings}
    p.reset(H)
    for i in range(40):
        res = p.put(*LC.cut(ob, verdicts, value_ok, i, i + 1))
    whole = verifier.decide_ordered(to_np(ob), np.array(verdicts, np.uint8), 2, schedule=_rows(sigs),
                                    value_ok=np.array(value_ok, np.uint8))
    assert res.bits.tolist() == whole.bits.tolist() and res.trace.tolist() == whole.trace.tolist()
    assert len(fired) >= 2 and res.base + res.kept == int(((whole.dup == 0) | (whole.pclass == 0)).sum())


# ---- 2. block and wavefront boundaries ---------------------------------------------
PIECES = (1, 63, 64, 65, 255, 257, 700)


@pytest.fixture(scope="module")
def big_mix(oracle):
    O = oracle
    rng = random.Random(42)
    sigs = [O.sha256(b"b" + bytes([k])) for k in range(40)]
    vals = [O.canonical_value(H, k) for k in range(3)] + [O.NIL_VALUE]
    ob, verdicts, value_ok = WC.mix(rng, 3000, [H], [0, 1, 2, 3], sigs, vals, 1 / 40, sigs, p_bad=0.05)
    verdicts[0] = O.VALID
    if ob.mtype[0] == O.PROPOSE:                                      # the first piece (one message) is a vote: kept
        ob.mtype[0], ob.valid_round[0] = O.PREVOTE, -1
    return sigs, ob, verdicts, value_ok


@pytest.mark.parametrize("f,with_schedule", [(13, True), (3, False)])
def test_block_and_wavefront_boundaries(verifier, oracle, pair, big_mix, f, with_schedule):
    sigs, ob, verdicts, value_ok = big_mix
    verifier.set_signatories(_rows(sigs[:20]))                        # signers 20..39 take the hashed table
    p = pair(H, f, sigs if with_schedule else None)
    lo, k, seen, fired = 0, 0, [], set()
    while lo < len(ob):
        hi = min(lo + PIECES[k % len(PIECES)], len(ob))
        res = p.put(*LC.cut(ob, verdicts, value_ok, lo, hi))
        seen.append((res.base, res.kept, hi - lo))
        fired |= {x for _, _, _, x in res.new_firings}
        if k == 4:                                                     # the same 255 messages again: nothing is kept
            again = p.put(*LC.cut(ob, verdicts, value_ok, lo, hi))
            assert again.kept == 0 and (again.logpos == NEVER).all() and again.new_firings == []
            assert not (again.dup == 0).any() and not (again.pclass == 0).any()
        lo, k = hi, k + 1
    assert seen[0][1:] == (1, 1)                                       # a piece that keeps everything
    assert sum(1 for b, _, _ in seen if b % 32) >= len(seen) - 3 and any(b // 256 != (b + kk) // 256 for b, kk, _ in seen)
    assert len(fired) >= 4, fired


# ---- 3. hand-worked crossings between calls ----------------------------------------
def _sig(O):
    return lambda k: O.sha256(b"g" + bytes([k]))


def _setup(verifier, O):
    sig = _sig(O)
    verifier.set_signatories(_rows([sig(k) for k in range(6)]))       # 6..: outside the set (hashed log path)
    return sig, O.canonical_value(H, 0), O.canonical_value(H, 1)


@pytest.mark.parametrize("signer", [0, 9])
def test_double_vote_across_calls(verifier, oracle, pair, signer):
    O = oracle
    sig, v, w = _setup(verifier, O)
    p = pair(H, 1)
    a = p.put([(O.PRECOMMIT, H, 0, -1, v, sig(signer))])
    assert (a.base, a.kept, a.dup.tolist(), a.logpos.tolist()) == (0, 1, [0], [0])
    b = p.put([(O.PRECOMMIT, H, 0, -1, v, sig(signer)), (O.PRECOMMIT, H, 0, -1, w, sig(signer)),
               (O.PREVOTE, H, 0, -1, w, sig(signer))])
    assert (b.base, b.kept, b.dup.tolist(), b.logpos.tolist()) == (1, 1, [1, 2, 0], [NEVER, NEVER, 1])
    assert b.precommits.tolist() == [1] and b.prevotes.tolist() == [1] and b.rep.tolist() == [0]


def test_double_propose_across_calls(verifier, oracle, pair):
    O = oracle
    sig, v, w = _setup(verifier, O)
    p = pair(H, 1)
    a = p.put([(O.PROPOSE, H, 0, -1, v, sig(1))])
    assert (a.kept, a.pclass.tolist(), a.dup.tolist(), a.propose.tolist()) == (1, [0], [3], [0])
    b = p.put([(O.PROPOSE, H, 0, -1, v, sig(1)), (O.PROPOSE, H, 0, -1, w, sig(1)), (O.PROPOSE, H, 0, 0, v, sig(1))])
    assert (b.base, b.kept, b.pclass.tolist(), b.propose.tolist()) == (1, 0, [1, 2, 2], [0])


def test_out_of_turn_propose_across_calls(verifier, oracle, pair):
    O = oracle
    sig, v, w = _setup(verifier, O)
    sched = [sig(k) for k in range(4)]                                 # (5 + 0) % 4 = 1, (5 + 1) % 4 = 2
    p = pair(H, 1, sched)
    p.put([(O.PROPOSE, H, 0, -1, v, sig(1))])
    b = p.put([(O.PROPOSE, H, 0, -1, v, sig(2)), (O.PROPOSE, H, 1, -1, v, sig(1)), (O.PROPOSE, H, 1, -1, w, sig(2))])
    assert (b.pclass.tolist(), b.kept, b.logpos.tolist()) == ([4, 4, 0], 1, [NEVER, NEVER, 1])


def test_quorum_completes_in_the_second_call(verifier, oracle, pair):
    """f = 2: 2f prevotes in call 1 and the (2f+1)-th in call 2."""
    O = oracle
    sig, v, w = _setup(verifier, O)
    p = pair(H, 2)
    a = p.put([(O.PREVOTE, H, 0, -1, v, sig(k)) for k in (0, 7, 1, 8)])
    assert _when(a, 0)[0][0] == NEVER and a.new_firings == [(2, H, 0, "skip")]
    b = p.put([(O.PREVOTE, H, 0, -1, v, sig(7)), (O.PREVOTE, H, 1, -1, v, sig(2)), (O.PREVOTE, H, 0, -1, w, sig(2))])
    assert b.base == 4 and _when(b, 0)[0][0] == b.base + 2 and _when(b, 0)[0][4] == 2
    assert b.new_firings == [(2, H, 0, "timeout_prevote")]
    c = p.put([])
    assert _when(c, 0)[0][0] == 5 == int(b.logpos[2]) and c.new_firings == []


def test_quorum_before_its_propose(verifier, oracle, pair):
    O = oracle
    sig, v, w = _setup(verifier, O)
    p = pair(H, 1)
    a = p.put([(O.PREVOTE, H, 0, -1, v, sig(k)) for k in (0, 7, 1)] + [(O.PRECOMMIT, H, 0, -1, v, sig(k)) for k in (0, 7, 1)])
    assert _when(a, 0)[0][5:7] == [NEVER, NEVER]
    p.put([(O.PREVOTE, H, 1, -1, w, sig(3))])
    c = p.put([(O.PREVOTE, H, 0, -1, v, sig(0)), (O.PROPOSE, H, 0, -1, v, sig(4))])
    w0 = _when(c, 0)[0]
    assert c.base == 7 and w0[5] == w0[6] == c.base + 1 and w0[0] == 2 and w0[2] == 5
    assert c.new_firings == [(1, H, 0, "precommit_value"), (1, H, 0, "commit")]


def test_valid_round_prevotes_from_an_earlier_call(verifier, oracle, pair):
    O = oracle
    sig, v, w = _setup(verifier, O)
    p = pair(H, 1)
    p.put([(O.PREVOTE, H, 0, -1, v, sig(k)) for k in (0, 7, 1)])
    b = p.put([(O.PREVOTE, H, 2, -1, v, sig(0)), (O.PROPOSE, H, 1, 0, v, sig(8))])
    assert _when(b, 1)[0][7] == b.base + 1 == 4 and (1, H, 1, "prevote_validround") in b.new_firings
    # the other order: the propose first, the valid round's quorum in a later call
    p.reset(H)
    p.put([(O.PROPOSE, H, 1, 0, v, sig(8)), (O.PREVOTE, H, 0, -1, v, sig(0))])
    c = p.put([(O.PREVOTE, H, 0, -1, v, sig(7)), (O.PREVOTE, H, 0, -1, v, sig(1))])
    assert _when(c, 1)[0][7] == c.base + 1 == 3


def test_exact_window_across_calls(verifier, oracle, pair):
    O = oracle
    sig, v, w = _setup(verifier, O)
    p = pair(H, 1)
    a = p.put([(O.PRECOMMIT, H, 0, -1, v, sig(k)) for k in (0, 7, 1)])
    wa, ua, ba = _when(a, 0)
    assert (wa[2], wa[3], ua, (ba >> 3) & 1) == (2, 2, NEVER, 1)
    b = p.put([(O.PRECOMMIT, H, 0, -1, w, sig(7)), (O.PRECOMMIT, H, 0, -1, v, sig(8))])
    wb, ub, bb = _when(b, 0)
    assert (wb[2], wb[3], ub, (bb >> 3) & 1) == (2, 2, b.base + 1, 0) and b.new_firings == []


@pytest.mark.parametrize("proposer", [2, 9])
def test_proposer_trace_entry_across_calls(verifier, oracle, pair, proposer):
    """f = 2 (three entries): the proposer's entry is its propose of call 1, so
    its vote of call 2 adds none."""
    O = oracle
    sig, v, w = _setup(verifier, O)
    p = pair(H, 2)
    a = p.put([(O.PROPOSE, H, 0, -1, v, sig(proposer)), (O.PREVOTE, H, 0, -1, v, sig(0))])
    assert _when(a, 0)[0][4] == NEVER
    b = p.put([(O.PREVOTE, H, 0, -1, v, sig(proposer)), (O.PRECOMMIT, H, 0, -1, v, sig(proposer)),
               (O.PREVOTE, H, 0, -1, v, sig(7))])
    assert b.base == 2 and b.kept == 3 and _when(b, 0)[0][4] == b.base + 2 and b.trace.tolist() == [3]


# ---- 4. heights ----------------------------------------------------------------------
def test_other_heights_stay_out(verifier, oracle, pair):
    O = oracle
    sig, v, w = _setup(verifier, O)
    p = pair(H, 1)
    a = p.put([(O.PREVOTE, H + 1, 0, -1, v, sig(0)), (O.PROPOSE, H - 1, 0, -1, v, sig(1)), (O.PREVOTE, H, 0, -1, v, sig(0)),
               (O.PROPOSE, H + 1, 0, -1, v, sig(1)), (O.PRECOMMIT, 0, 0, -1, v, sig(0))])
    assert (a.dup.tolist(), a.pclass.tolist()) == ([3, 3, 0, 3, 3], [3] * 5)
    assert (a.kept, a.logpos.tolist(), a.height.tolist()) == (1, [NEVER, NEVER, 0, NEVER, NEVER], [H])
    b = p.put([(O.PREVOTE, H + 1, 0, -1, v, sig(0))])
    assert (b.kept, len(b)) == (0, 1)


def test_reset_empties_the_log(verifier, oracle, pair):
    O = oracle
    sig, v, w = _setup(verifier, O)
    p = pair(H, 1)
    msgs = [(O.PREVOTE, H, 0, -1, v, sig(0)), (O.PREVOTE, H + 1, 0, -1, v, sig(0)), (O.PREVOTE, H + 1, 0, -1, v, sig(7))]
    a = p.put(msgs)
    assert (a.kept, a.dup.tolist()) == (1, [0, 3, 3])
    assert p.put(msgs).dup.tolist() == [1, 3, 3]
    p.reset(H + 1)
    b = p.put(msgs)
    assert (b.base, b.kept, b.dup.tolist(), b.height.tolist()) == (0, 2, [3, 0, 0], [H + 1])
    p.reset(H + 2, f=0)
    c = p.put([(O.PREVOTE, H + 2, 0, -1, v, sig(0))])
    assert c.new_firings == [(0, H + 2, 0, "timeout_prevote"), (0, H + 2, 0, "skip")]


def test_reset_with_a_new_schedule(verifier, oracle, pair):
    O = oracle
    sig, v, w = _setup(verifier, O)
    sched = [sig(k) for k in range(4)]
    p = pair(H, 1, sched)
    msgs = [(O.PROPOSE, H, 0, -1, v, sig(1)), (O.PROPOSE, H, 0, -1, v, sig(2))]
    assert p.put(msgs).pclass.tolist() == [0, 4]
    p.reset(H, schedule=sched[::-1])                                   # (5 + 0) % 4 = 1 is sig(2) now
    assert p.put(msgs).pclass.tolist() == [4, 0]
    p.reset(H, schedule=sched + sched[:1])                             # five entries: (5 + 0) % 5 = 0
    assert p.put(msgs + [(O.PROPOSE, H, 0, -1, v, sig(0))]).pclass.tolist() == [4, 4, 0]


# ---- 5. limits and errors ------------------------------------------------------------
def _raw(p, ob, verdicts, cap=None, with_classes=True):
    """hd_log_insert through the C ABI: (rc, out struct, arrays, when, until, logpos, info)."""
    from hyperdrive_amd import _lib
    lib = _lib.load()
    nb, v = to_np(ob), np.array(verdicts, np.uint8)
    o, a, w, when, until, logpos, info = p.log._outputs(len(ob))
    if cap is not None:
        o.cap = cap
    if not with_classes:
        o.dup = o.pclass = info.logpos = None
    cb = nb.c_struct()
    rc = lib.hd_log_insert(p.log.handle, ctypes.byref(cb), v.ctypes.data if len(v) else None, None, ctypes.byref(o),
                           ctypes.byref(w), ctypes.byref(info))
    return rc, o, a, when, until, logpos, info


def test_max_entries(verifier, oracle, pair):
    from hyperdrive_amd import _lib
    O = oracle
    sig, v, w = _setup(verifier, O)
    p = pair(H, 1, max_entries=5)
    p.put([(O.PREVOTE, H, 0, -1, v, sig(k)) for k in range(4)])
    over = _batch(O, [(O.PRECOMMIT, H, 0, -1, v, sig(k)) for k in (0, 0, 1, 7)])
    rc, o, a, when, until, logpos, info = _raw(p, over, [O.VALID] * 4)
    assert rc == _lib.HD_ECAP and (info.base, info.kept, info.relogged) == (4, 3, 4) and p.log.entries == 4
    with pytest.raises(_lib.HDError) as e:
        p.log.insert(to_np(over), np.zeros(4, np.uint8))
    assert e.value.code == _lib.HD_ECAP and p.log.entries == 4
    res = p.put([(O.PRECOMMIT, H, 0, -1, v, sig(0)), (O.PRECOMMIT, H, 0, -1, w, sig(0))])
    assert (res.base, res.kept, p.log.entries) == (4, 1, 5)
    res = p.put([(O.PRECOMMIT, H, 0, -1, v, sig(0))])                 # full, and nothing to add: fine
    assert res.kept == 0


def test_row_capacity_and_null_arguments(verifier, oracle, pair):
    from hyperdrive_amd import _lib
    lib = _lib.load()
    O = oracle
    sig, v, w = _setup(verifier, O)
    p = pair(H, 1)
    p.put([(O.PREVOTE, H, 0, -1, v, sig(0))])
    more = _batch(O, [(O.PREVOTE, H, 1, -1, v, sig(0)), (O.PREVOTE, H, 2, -1, v, sig(0))])
    rc, o, *_ = _raw(p, more, [O.VALID] * 2, cap=2)
    assert rc == _lib.HD_ECAP and o.n == 3 and p.log.entries == 1
    # NULL arguments: HD_EINVAL before any device work
    nb = to_np(more)
    cb, vd = nb.c_struct(), np.zeros(2, np.uint8)
    o, a, w_, when, until, logpos, info = p.log._outputs(2)
    args = [p.log.handle, ctypes.byref(cb), vd.ctypes.data, None, ctypes.byref(o), ctypes.byref(w_), ctypes.byref(info)]
    for k in (0, 1, 2, 4, 5, 6):
        bad = list(args)
        bad[k] = None
        assert lib.hd_log_insert(*bad) == _lib.HD_EINVAL, k
    o.bits = None
    assert lib.hd_log_insert(*args) == _lib.HD_EINVAL
    o, a, w_, when, until, logpos, info = p.log._outputs(2)
    w_.cap = o.cap - 1
    assert lib.hd_log_insert(p.log.handle, ctypes.byref(cb), vd.ctypes.data, None, ctypes.byref(o), ctypes.byref(w_),
                             ctypes.byref(info)) == _lib.HD_EINVAL
    w_.cap = o.cap
    assert lib.hd_log_insert_device_bitmap(p.log.handle, ctypes.byref(cb), None, None, ctypes.byref(o),
                                           ctypes.byref(w_), ctypes.byref(info), None) == _lib.HD_EINVAL
    assert lib.hd_log_create(None, None) == _lib.HD_EINVAL and lib.hd_log_destroy(None) == _lib.HD_EINVAL
    assert lib.hd_log_reset(None, 1, 1, None, 0, 0) == _lib.HD_EINVAL
    assert lib.hd_log_reset(p.log.handle, 1, 1, vd.ctypes.data, 0, 0) == _lib.HD_EINVAL
    assert lib.hd_log_len(None, None, None) == _lib.HD_EINVAL and lib.hd_log_len(p.log.handle, None, None) == 0
    assert p.log.entries == 1 and p.log.height == H
    res = p.put(more)                                                  # the log is as it was
    assert (res.base, res.kept, len(res)) == (1, 2, 3)


def test_empty_batches_and_null_outputs(verifier, oracle, pair):
    O = oracle
    sig, v, w = _setup(verifier, O)
    p = pair(H, 0)
    res = p.put([])
    assert (len(res), res.base, res.kept, res.when.shape, res.firings) == (0, 0, 0, (0, 8), [])
    res = p.put([(O.PREVOTE, H, 0, -1, v, sig(0))], [O.BAD_RS])
    assert (len(res), res.kept, res.dup.tolist()) == (0, 0, [3])
    first = p.put([(O.PREVOTE, H, 0, -1, v, sig(0)), (O.PROPOSE, H, 0, -1, v, sig(7))])
    again = p.put([])
    assert (again.base, again.kept, len(again.logpos)) == (2, 0, 0)
    assert again.when.tolist() == first.when.tolist() and again.bits.tolist() == first.bits.tolist()
    # dup / pclass / logpos NULL
    ob = _batch(O, [(O.PREVOTE, H, 0, -1, v, sig(0)), (O.PREVOTE, H, 0, -1, v, sig(1))])
    exp = p.ys.push(ob, [O.VALID] * 2)
    rc, o, a, when, until, logpos, info = _raw(p, ob, [O.VALID] * 2, with_classes=False)
    assert rc == 0 and (info.base, info.kept, info.relogged, o.n) == (2, 1, 2, 1)
    assert when[: o.n].tolist() == exp.when and (logpos == NEVER).all() and not a["dup"].any()
    p.put([])


# ---- 6. growth and sharing -----------------------------------------------------------
def test_growth_keeps_the_entries(gpu, oracle):
    """A fresh context and log: 10 messages, then 5,000 -- every buffer grows
    and the ten retained entries move with them."""
    O = oracle
    rng = random.Random(43)
    sigs = [O.sha256(b"h" + bytes([k])) for k in range(40)]
    vals = [O.canonical_value(H, k) for k in range(2)] + [O.NIL_VALUE]
    ob, verdicts, value_ok = WC.mix(rng, 5010, [H], [0, 1, 2, 3], sigs, vals, 1 / 50, None, p_bad=0.02)
    v = gpu.Verifier(0)
    try:
        v.set_signatories(_rows(sigs[:20]))
        p = Pair(v, O, H, 13)
        a = p.put(*LC.cut(ob, verdicts, value_ok, 0, 10))
        b = p.put(*LC.cut(ob, verdicts, value_ok, 10, 5010))
        assert a.kept >= 8 and b.base == a.kept and b.kept > 200 and (b.rep < b.base).any()
        p.close()
    finally:
        v.close()


def test_shares_the_context_with_tally_and_decide(verifier, oracle, pair):
    O = oracle
    rng = random.Random(44)
    sigs = [O.sha256(b"i" + bytes([k])) for k in range(30)]
    vals = [O.canonical_value(H, k) for k in range(2)] + [O.NIL_VALUE]
    verifier.set_signatories(_rows(sigs[:15]))
    ob, verdicts, value_ok = WC.mix(rng, 1200, [H], list(range(4)), sigs, vals, 1 / 8)
    other, overd, ook = WC.mix(rng, 900, [1, 2, 3], list(range(5)), sigs, vals, 1 / 8)
    nb, ov = to_np(other), np.array(overd, np.uint8)
    p, q = pair(H, 3), pair(H, 9, sigs)
    p.put(*LC.cut(ob, verdicts, value_ok, 0, 500))
    tal, ot = verifier.tally(nb, ov), O.tally(other, overd)
    assert (tal.count, tal.distinct, tal.dup.tolist()) == (ot.count, ot.distinct, ot.dup)
    q.put(*LC.cut(ob, verdicts, value_ok, 600, 900))                   # a second log on the context
    PC.same_as(verifier.decide(nb, ov, 3, value_ok=np.array(ook, np.uint8)), PC.restate(other, overd, 3, None, ook))
    p.put(*LC.cut(ob, verdicts, value_ok, 500, 1200))
    verifier.set_signatories(_rows(sigs[10:]))                         # a set change between inserts
    q.put(*LC.cut(ob, verdicts, value_ok, 0, 600))
    res = verifier.decide_ordered(nb, ov, 3, value_ok=np.array(ook, np.uint8))
    WC.same_when(res, WC.replay(other, overd, 3, None, ook))
    p.put(*LC.cut(ob, verdicts, value_ok, 0, 100))
    q.put(*LC.cut(ob, verdicts, value_ok, 900, 1200))


def test_no_signatory_set(gpu, oracle):
    """S = 0: every signer takes the hashed table."""
    O = oracle
    rng = random.Random(45)
    sigs = [O.sha256(b"j" + bytes([k])) for k in range(12)]
    vals = [O.canonical_value(H, 0), O.NIL_VALUE]
    ob, verdicts, value_ok = WC.mix(rng, 400, [H], [0, 1], sigs, vals, 1 / 8, sigs)
    v = gpu.Verifier(0)
    try:
        p = Pair(v, O, H, 3, sigs)
        for lo, hi in ((0, 70), (70, 71), (71, 400)):
            p.put(*LC.cut(ob, verdicts, value_ok, lo, hi))
        p.close()
    finally:
        v.close()


# ---- 7. the device entry ---------------------------------------------------------------
def test_device_entry_in_four_slices(verifier, oracle):
    import torch
    from hyperdrive_amd import quorum
    from hyperdrive_amd.device import generate, work_stream
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
    assert (db.height == 1).all().item()
    f = quorum.thresholds(S)[0]
    whole = verifier.decide_ordered_device(cs, bitmap.data_ptr(), f, schedule=ks[0], stream=ws.cuda_stream)
    logged = (whole.dup == 0) | (whole.pclass == 0)
    log = verifier.open_log(1, f, ks[0])
    try:
        pos = np.full(n, NEVER, np.uint32)
        for k in range(n // m):
            part = db.rows(k * m, m).c_struct()
            res = log.insert_device(part, bitmap.data_ptr() + 4 * (k * m // 32), stream=ws.cuda_stream)
            sl = slice(k * m, (k + 1) * m)
            assert (res.base, res.kept, res.relogged) == (int(logged[: k * m].sum()), int(logged[sl].sum()), res.base)
            assert res.dup.tolist() == whole.dup[sl].tolist() and res.pclass.tolist() == whole.pclass[sl].tolist()
            pos[sl] = res.logpos
            assert ((res.logpos != NEVER) == logged[sl]).all()
        assert log.entries == int(logged.sum()) and pos[logged].tolist() == list(range(log.entries))
        # the last insert is the whole batch's answer under the index map
        base, lo = res.base, n - m
        ix = np.vectorize(lambda i: NEVER if i == NEVER else (int(pos[i]) if i < lo else base + (i - lo)), otypes=[np.uint32])
        for key in PC.ROW_FIELDS:
            want = getattr(whole, key)
            assert getattr(res, key).tolist() == (ix(want) if key in ("rep", "propose") else want).tolist(), key
        assert res.when.tolist() == ix(whole.when).tolist() and res.exact_until.tolist() == ix(whole.exact_until).tolist()
        assert len(res) >= 40 and (res.when != NEVER).sum() > 100
        assert res.new_firings == [(i - lo, h, r, name) for i, h, r, name in whole.firings if i >= lo]
    finally:
        log.close()


# ---- 8. ingress ------------------------------------------------------------------------
def test_ingress_flush_decide(verifier, oracle):
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
        log = ing.open_log()
        assert (log.height, log.f, ing.f) == (H0, S // 3, S // 3)
        ys = LC.Stream(H0, S // 3)

        def flush():
            res, dec = ing.flush_decide()
            ob = from_np(res.consumed)
            LC.same_insert(dec, ys.push(ob, [O.VALID] * len(ob)))
            assert len(res.consumed) == len(dec.dup) and (res.consumed.height == ing.height).all()
            return res, dec

        ing.push_device(half(perm[: n // 2]))
        r1, d1 = flush()
        ing.push_device(half(perm[n // 2:]))
        r2, d2 = flush()                                               # the same height again: the log carries over
        assert len(r1.consumed) > 5 and len(r2.consumed) > 5 and d2.base == d1.kept > 0
        assert d1.new_firings != [] and len(d2.firings) >= len(d1.firings)
        assert ing.reset_height(H0 + 1, sigs[: S - 3])                 # ResetHeight with a smaller set: f = 5
        assert (log.height, log.entries, log.f) == (H0 + 1, 0, (S - 3) // 3)
        ys = LC.Stream(H0 + 1, (S - 3) // 3)
        r3, d3 = flush()
        assert d3.base == 0 and d3.kept > 10
        ing.advance_height(H0 + 2)
        assert (log.height, log.entries) == (H0 + 2, 0)
        ys = LC.Stream(H0 + 2, (S - 3) // 3)
        r4, d4 = flush()
        assert d4.base == 0 and d4.kept > 10
    finally:
        ing.close()
