"""hd_decide_ordered / hd_decide_ordered_device_bitmap (through the Python face
and the C ABI) against the sequential replay of tests/when_cases.py and the
restatement of tests/propose_cases.py.  Verdicts are passed directly and the
signatures are 65 zero bytes, as in tests/test_gpu_decide.py; only the
device-entry case verifies a generated batch first."""
import ctypes
import random

import numpy as np
import pytest

import propose_cases as PC
import when_cases as WC
from util import from_np, to_np

pytestmark = pytest.mark.gpu

NEVER = WC.NEVER
MONOTONE = (0, 1, 2, 4, 5, 6, 7)


@pytest.fixture(scope="module")
def verifier(gpu):
    v = gpu.Verifier(0)
    yield v
    v.close()


def _rows(sigs):
    return np.frombuffer(b"".join(sigs), np.uint8).reshape(len(sigs), 32).copy()


def _args(ob, verdicts, schedule, value_ok):
    return (to_np(ob), np.array(verdicts, np.uint8)), dict(
        schedule=_rows(schedule) if schedule is not None else None,
        value_ok=np.array(value_ok, np.uint8) if value_ok is not None else None)


def _ordered(verifier, ob, verdicts, f, schedule=None, value_ok=None):
    a, kw = _args(ob, verdicts, schedule, value_ok)
    return verifier.decide_ordered(*a, f, **kw)


def _bits_agree(res):
    """The monotone bits are `when != NEVER`; bit 3 is the open window."""
    for j in range(len(res)):
        bits = int(res.bits[j])
        for k in MONOTONE:
            assert bool((bits >> k) & 1) == (int(res.when[j, k]) != NEVER), (j, k)
        assert bool((bits >> 3) & 1) == (int(res.when[j, 3]) != NEVER and int(res.exact_until[j]) == NEVER), j
        assert int(res.when[j, 3]) == int(res.when[j, 2])
        if int(res.exact_until[j]) != NEVER:
            assert int(res.when[j, 3]) < int(res.exact_until[j])


def _check(verifier, ob, verdicts, f, schedule=None, value_ok=None):
    """decide_ordered == the restatement (rows) and the replay (when), exactly."""
    res = _ordered(verifier, ob, verdicts, f, schedule, value_ok)
    PC.same_as(res, PC.restate(ob, verdicts, f, schedule, value_ok))
    logs = WC.replay(ob, verdicts, f, schedule, value_ok)
    WC.same_when(res, logs)
    _bits_agree(res)
    return res, logs


def _same_rows(a, b):
    for k in PC.ROW_FIELDS + ("pclass", "dup"):
        x, y = getattr(a, k), getattr(b, k)
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), k


def _when(res, h, r):
    hit = [j for j in range(len(res)) if (int(res.height[j]), int(res.round[j])) == (h, r)]
    assert len(hit) == 1, (h, r, hit)
    return res.when[hit[0]].tolist(), int(res.exact_until[hit[0]])


# ---- 1. random mixes, and 6. agreement with decide -----------------------------
@pytest.mark.parametrize("with_schedule", [True, False])
def test_dense_mix(verifier, oracle, with_schedule):
    O = oracle
    rng = random.Random(15)
    sigs = [O.sha256(b"d" + bytes([k])) for k in range(70)]
    vals = [O.canonical_value(1, k) for k in range(3)] + [O.NIL_VALUE]
    verifier.set_signatories(_rows(sigs[:35]))                    # signers 35..69 take the hashed table
    sched = sigs if with_schedule else None
    ob, verdicts, value_ok = WC.mix(rng, 6000, [1, 2, 3], [-1, 0, 1, 2, 3], sigs, vals, 1 / 40, sched)
    for f in (70 // 3, 5):
        res, logs = _check(verifier, ob, verdicts, f, sched, value_ok)
        a, kw = _args(ob, verdicts, sched, value_ok)
        _same_rows(res, verifier.decide(*a, f, **kw))
    fired = {k for x in logs.values() for k in range(8) if x.when[k] != NEVER}
    assert fired == set(range(8)) and any(x.exact_until != NEVER for x in logs.values())
    assert {2} <= set(res.dup.tolist()) and len(res.proposes) >= 6


def test_sparse_mix(verifier, oracle):
    """300 rounds over 4,000 messages: a wavefront's lanes do not share a round."""
    O = oracle
    rng = random.Random(16)
    sigs = [O.sha256(b"s" + bytes([k])) for k in range(40)]
    vals = [O.canonical_value(2, k) for k in range(2)] + [O.NIL_VALUE]
    verifier.set_signatories(_rows(sigs[:20]))
    ob, verdicts, value_ok = WC.mix(rng, 4000, list(range(1, 31)), list(range(10)), sigs, vals, 1 / 10,
                                    valid_rounds=(-1, 0, 1, 2, 3, 7))
    for f in (1, 0):
        res, logs = _check(verifier, ob, verdicts, f, None, value_ok)
        a, kw = _args(ob, verdicts, None, value_ok)
        _same_rows(res, verifier.decide(*a, f, **kw))
    assert len(res) > 290 and len(res.firings) > 600


# ---- 2. thresholds at wavefront boundaries ---------------------------------------
def _two_rounds(O, rng, sigs):
    """Round (1, 0): a prevote and a precommit of every signer, shuffled, with
    round (1, 1)'s votes between them.  Message 0 belongs to round (1, 0)."""
    v = O.canonical_value(1, 0)
    a = [(t, 1, 0, -1, v, s) for s in sigs for t in (O.PREVOTE, O.PRECOMMIT)]
    b = [(t, 1, 1, -1, rng.choice([v, O.NIL_VALUE]), s) for s in sigs[::3] for t in (O.PREVOTE, O.PRECOMMIT)]
    rng.shuffle(a)
    rest = a[1:] + b
    rng.shuffle(rest)
    return [a[0]] + rest


def _batch(O, msgs):
    ob = O.Batch()
    for m in msgs:
        ob.append(*m, bytes(65))
    return ob


@pytest.mark.parametrize("f", [0, 31, 32, 62, 63, 64, 128])
def test_thresholds_at_wave_boundaries(verifier, oracle, f):
    """2f+1 in {1, 63, 65, 129} and f+1 in {1, 63, 64, 65, 129}: the crossing
    item is the last of a 64-item chunk, the first of the next, or inside."""
    O = oracle
    rng = random.Random(200 + f)
    sigs = [O.sha256(b"w" + bytes([k])) for k in range(140)]
    verifier.set_signatories(_rows(sigs[:100]))                   # 40 signers outside the admitted set
    msgs = _two_rounds(O, rng, sigs)
    ob = _batch(O, msgs)
    ok = [O.VALID] * len(ob)
    res, logs = _check(verifier, ob, ok, f)
    x = logs[(1, 0)]
    if f == 0:                                                    # the crossing vote is the first message
        assert x.when[4] == 0 and 0 in (x.when[0], x.when[2])
    assert x.when[4] != NEVER and (x.when[2] != NEVER) == (2 * f + 1 <= 140)
    # the crossing vote is the last message of the batch
    for k in (0, 2, 4):
        if x.when[k] != NEVER:
            cut = _batch(O, msgs[: x.when[k] + 1])
            res, _ = _check(verifier, cut, [O.VALID] * len(cut), f)
            assert _when(res, 1, 0)[0][k] == len(cut) - 1
    # the crossing precommit directly after a double vote of the same signer
    c = x.when[2]
    if c != NEVER:
        s = ob.frm[c]
        v2 = O.canonical_value(7, 7)
        extra = [(O.PREVOTE, 1, 0, -1, ob.value[c], s), (O.PREVOTE, 1, 0, -1, v2, s)]
        ob2 = _batch(O, msgs[:c] + extra + msgs[c:])
        res, logs2 = _check(verifier, ob2, [O.VALID] * len(ob2), f)
        assert int(res.dup[c + 1]) == 2 and _when(res, 1, 0)[0][2] == c + 2 == logs2[(1, 0)].when[2]


# ---- 3. the propose's place ------------------------------------------------------
def _place_setup(verifier, O):
    sig = lambda k: O.sha256(b"p" + bytes([k]))
    verifier.set_signatories(_rows([sig(k) for k in range(6)]))   # 6..: outside the set (hashed log path)
    return sig, O.canonical_value(3, 1)


@pytest.mark.parametrize("place", ["before", "between", "after"])
def test_propose_place(verifier, oracle, place):
    """f = 2: five prevotes and five precommits of round (3, 1) and five
    prevotes of the valid round (3, 0), all for the propose's value; the
    propose before all of them, after the fifth prevote but before the fifth
    precommit and the valid round's fifth prevote, or after all of them."""
    O = oracle
    sig, v = _place_setup(verifier, O)
    other = O.canonical_value(3, 2)
    votes = []
    for k in range(5):
        votes += [(O.PREVOTE, 3, 1, -1, v, sig(k + 3)), (O.PRECOMMIT, 3, 1, -1, v, sig(k + 3)),
                  (O.PREVOTE, 3, 0, -1, v, sig(k + 3)), (O.PREVOTE, 3, 1, -1, other, sig(k + 10))]
    propose = (O.PROPOSE, 3, 1, 0, v, sig(20))
    pos = {"before": 0, "between": 4 * 4 + 1, "after": len(votes)}[place]
    msgs = votes[:pos] + [propose] + votes[pos:]
    ob = _batch(O, msgs)
    res, logs = _check(verifier, ob, [O.VALID] * len(ob), 2)
    w, _ = _when(res, 3, 1)
    idx = lambda m: msgs.index(m)
    fifth = lambda t, r: idx((t, 3, r, -1, v, sig(7)))
    assert w[5] == max(pos, fifth(O.PREVOTE, 1))
    assert w[6] == max(pos, fifth(O.PRECOMMIT, 1))
    assert w[7] == max(pos, fifth(O.PREVOTE, 0))
    assert res.proposes[(3, 1)] == pos


@pytest.mark.parametrize("case", ["own_round", "empty_round", "later_crossing", "below"])
def test_valid_round_place(verifier, oracle, case):
    O = oracle
    sig, v = _place_setup(verifier, O)
    f = 2
    msgs = []
    vr = {"own_round": 1, "empty_round": 4}.get(case, 0)
    n_vr = 4 if case == "below" else 5
    if case != "later_crossing":
        msgs += [(O.PREVOTE, 3, 0, -1, v, sig(k + 4)) for k in range(n_vr)]
    msgs += [(O.PREVOTE, 3, 1, -1, v, sig(k + 4)) for k in range(5)]
    msgs.append((O.PROPOSE, 3, 1, vr, v, sig(1)))
    msgs.append((O.PRECOMMIT, 3, 1, -1, v, sig(2)))
    last_of_round = len(msgs) - 1
    if case == "later_crossing":                                   # after every message of round (3, 1)
        msgs += [(O.PREVOTE, 9, 0, -1, v, sig(k + 4)) for k in range(5)]     # another height: must not count
        msgs += [(O.PREVOTE, 3, 0, -1, v, sig(k + 4)) for k in range(5)]
    ob = _batch(O, msgs)
    res, logs = _check(verifier, ob, [O.VALID] * len(ob), f)
    w, _ = _when(res, 3, 1)
    p = res.proposes[(3, 1)]
    if case == "own_round":
        assert w[7] == w[5] == p
    elif case in ("empty_round", "below"):
        assert w[7] == NEVER and w[5] == p
    else:
        assert w[7] == len(ob) - 1 > last_of_round


@pytest.mark.parametrize("case", ["new", "new_last", "voted_dense", "voted_hashed", "votes_later_dense",
                                  "votes_later_hashed", "invalid"])
def test_proposer_trace_entry(verifier, oracle, case):
    """f = 2 (three entries).  The proposer is new to the trace, already voted
    (its log in a dense cell or in the hashed table), votes only after its
    propose, or its propose is invalid."""
    O = oracle
    sig, v = _place_setup(verifier, O)
    dense, hashed = 2, 9
    proposer = {"voted_dense": dense, "votes_later_dense": dense, "voted_hashed": hashed,
                "votes_later_hashed": hashed}.get(case, 30)
    own = [(O.PRECOMMIT, 3, 1, -1, v, sig(proposer)), (O.PREVOTE, 3, 1, -1, v, sig(proposer))]
    propose = (O.PROPOSE, 3, 1, -1, O.NIL_VALUE if case == "invalid" else v, sig(proposer))
    a, b, c = [(O.PREVOTE, 3, 1, -1, v, sig(k)) for k in (0, 7, 1)]
    if case == "new":
        msgs, want = [a, propose, b, c], 2
    elif case == "new_last":
        msgs, want = [a, b, propose, c], 2
    elif case in ("voted_dense", "voted_hashed"):
        msgs, want = [own[0], a, propose, own[1], b], 4
    elif case in ("votes_later_dense", "votes_later_hashed"):
        msgs, want = [propose, own[0], own[1], a, b], 4
    else:
        msgs, want = [a, propose, b, c], 3
    ob = _batch(O, msgs)
    res, logs = _check(verifier, ob, [O.VALID] * len(ob), 2)
    assert _when(res, 3, 1)[0][4] == want


# ---- 4. the exact window -----------------------------------------------------------
@pytest.mark.parametrize("f", [3, 0])
@pytest.mark.parametrize("extra", [-1, 0, 1, 4])
def test_exact_window(verifier, oracle, f, extra):
    """Precommit logs of 2f, 2f+1, 2f+2 and 2f+5 signers."""
    O = oracle
    sig = lambda k: O.sha256(b"x" + bytes([k]))
    verifier.set_signatories(_rows([sig(k) for k in range(5)]))
    v = O.canonical_value(1, 0)
    n_pc = 2 * f + 1 + extra
    msgs = []
    for k in range(n_pc):
        msgs.append((O.PRECOMMIT, 1, 0, -1, v, sig(k)))
        msgs.append((O.PREVOTE, 1, 1, -1, v, sig(k)))             # another round between them
        if k % 3 == 0:
            msgs.append((O.PRECOMMIT, 1, 0, -1, O.NIL_VALUE, sig(k)))   # a double vote: not logged
    msgs.append((O.PREVOTE, 1, 0, -1, v, sig(0)))                 # the row exists with no precommit at all
    ob = _batch(O, msgs)
    res, logs = _check(verifier, ob, [O.VALID] * len(ob), f)
    w, until = _when(res, 1, 0)
    a, kw = _args(ob, [O.VALID] * len(ob), None, None)
    bit3 = verifier.decide(*a, f, **kw).decisions[(1, 0)]["timeout_precommit_exact"]
    nth = lambda k: msgs.index((O.PRECOMMIT, 1, 0, -1, v, sig(k - 1)))
    if extra < 0:
        assert (w[2], w[3], until, bit3) == (NEVER, NEVER, NEVER, False)
    elif extra == 0:
        assert (w[2], w[3], until, bit3) == (nth(2 * f + 1), nth(2 * f + 1), NEVER, True)
    else:
        assert (w[2], w[3], until, bit3) == (nth(2 * f + 1), nth(2 * f + 1), nth(2 * f + 2), False)


# ---- 5. edge sizes -------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_edge_sizes(verifier, oracle, n):
    O = oracle
    sigs = [O.sha256(b"e" + bytes([k])) for k in range(6)]
    vals = [O.canonical_value(1, 0), O.NIL_VALUE]
    verifier.set_signatories(_rows(sigs[:3]))
    for seed in range(3):
        rng = random.Random(100 * n + seed)
        ob, verdicts, value_ok = WC.mix(rng, n, [1, 2], [0, 1], sigs, vals, 1 / 4, None, 0.05, valid_rounds=(-1, 0, 1))
        for f in (0, 1):
            _check(verifier, ob, verdicts, f, None, value_ok)
        # thresholds above the batch size, up to the largest f
        for f in (n, 2**31 - 1, 2**31, 2**32 - 1):
            res, _ = _check(verifier, ob, verdicts, f, None, value_ok)
            assert (res.when == NEVER).all() and (res.exact_until == NEVER).all() and res.firings == []
    # the last message alone is a candidate
    ob = O.Batch()
    for i in range(n):
        ob.append(O.PROPOSE, 1, 0, 0, vals[0], sigs[0], bytes(65))
    res, _ = _check(verifier, ob, [O.BAD_RS] * (n - 1) + [O.VALID], 0)
    assert len(res) == 1 and res.when[0].tolist() == [NEVER] * 4 + [n - 1] + [NEVER] * 3
    assert res.firings == [(n - 1, 1, 0, "skip")]


def test_empty_candidate_batch(verifier, oracle):
    O = oracle
    ob = O.Batch()
    for t in (1, 2, 3, 1):
        ob.append(t, 1, 0, -1, bytes(32), O.sha256(b"x"), bytes(65))
    res, _ = _check(verifier, ob, [O.BAD_RS, O.NOT_ADMITTED, O.BAD_RS, O.NO_POINT], 1)
    assert len(res) == 0 and res.when.shape == (0, 8) and res.firings == []


# ---- 7. the tables stay clean --------------------------------------------------------
def test_tables_stay_clean(verifier, oracle):
    from hyperdrive_amd import _lib
    O = oracle
    rng = random.Random(19)
    sigs = [O.sha256(b"c" + bytes([k])) for k in range(30)]
    vals = [O.canonical_value(1, k) for k in range(2)] + [O.NIL_VALUE]
    verifier.set_signatories(_rows(sigs[:15]))
    ob, verdicts, value_ok = WC.mix(rng, 3000, [1, 2, 3, 4], list(range(6)), sigs, vals, 1 / 8)
    first, logs = _check(verifier, ob, verdicts, 3, None, value_ok)
    nb, v = to_np(ob), np.array(verdicts, np.uint8)
    tal = verifier.tally(nb, v)
    ot = O.tally(ob, verdicts)
    assert (tal.count, tal.distinct, tal.distinct_any, tal.dup.tolist()) == (ot.count, ot.distinct, ot.distinct_any,
                                                                            ot.dup)
    PC.same_as(verifier.decide(nb, v, 3, value_ok=np.array(value_ok, np.uint8)),
               PC.restate(ob, verdicts, 3, None, value_ok))
    again, _ = _check(verifier, ob, verdicts, 3, None, value_ok)
    _same_rows(again, first)
    assert again.when.tobytes() == first.when.tobytes() and again.exact_until.tobytes() == first.exact_until.tobytes()
    # a capacity below the row count: HD_ECAP with the need, and the next calls are right
    lib = _lib.load()
    o, a = verifier._decide_struct(len(ob), cap=len(first) - 1)
    w, when, until = verifier._order_struct(len(first) - 1)
    cin = _lib.HdDecideIn(3, 0, None, None)
    cb = nb.c_struct()
    rc = lib.hd_decide_ordered(verifier.handle, ctypes.byref(cb), v.ctypes.data, ctypes.byref(cin), ctypes.byref(o),
                               ctypes.byref(w))
    assert rc == _lib.HD_ECAP and o.n == len(first)
    _check(verifier, ob, verdicts, 3)
    # fewer `when` rows than decide rows: HD_EINVAL before any device work
    o, a = verifier._decide_struct(len(ob), cap=len(first))
    w, when, until = verifier._order_struct(len(first) - 1)
    o.n = 12345
    rc = lib.hd_decide_ordered(verifier.handle, ctypes.byref(cb), v.ctypes.data, ctypes.byref(cin), ctypes.byref(o),
                               ctypes.byref(w))
    assert rc == _lib.HD_EINVAL and o.n == 12345 and (when == NEVER).all()
    w.cap = len(first)
    w.when = None
    assert lib.hd_decide_ordered(verifier.handle, ctypes.byref(cb), v.ctypes.data, ctypes.byref(cin), ctypes.byref(o),
                                 ctypes.byref(w)) == _lib.HD_EINVAL
    assert lib.hd_decide_ordered(verifier.handle, ctypes.byref(cb), v.ctypes.data, ctypes.byref(cin), ctypes.byref(o),
                                 None) == _lib.HD_EINVAL
    tal = verifier.tally(nb, v)
    assert (tal.count, tal.dup.tolist()) == (ot.count, ot.dup)
    _check(verifier, ob, verdicts, 3, None, value_ok)


# ---- 8. more rounds than staged --------------------------------------------------------
def test_more_rounds_than_staged(gpu, oracle):
    """A fresh context stages 1,024 rows: a batch of 1,500 rounds takes the
    overflow columns -- `when` and `exact_until` with them -- and the next
    call the grown stage."""
    O = oracle
    v = gpu.Verifier(0)
    try:
        ob = O.Batch()
        val = O.canonical_value(1, 0)
        for k in range(1500):
            t = (O.PROPOSE, O.PREVOTE, O.PRECOMMIT)[k % 3]
            ob.append(t, 1 + k // 50, k % 50, -1, val, O.sha256(b"o" + bytes([k % 7])), bytes(65))
        for k in range(1500):                                      # a second vote in every round
            ob.append(O.PRECOMMIT, 1 + k // 50, k % 50, -1, val, O.sha256(b"o" + bytes([7 + k % 5])), bytes(65))
        for _ in range(2):
            res, logs = _check(v, ob, [O.VALID] * len(ob), 0)
            assert len(res) == 1500 and len(res.firings) > 3000
            assert (res.exact_until[1024:] != NEVER).sum() > 100 and (res.when[1024:, 4] < 1500).all()
    finally:
        v.close()


# ---- 9. the device entry on generated data ---------------------------------------------
@pytest.mark.parametrize("adv", [0, 30])
def test_device_entry_on_generated_rounds(verifier, oracle, adv):
    import torch
    from hyperdrive_amd import quorum
    from hyperdrive_amd.device import generate, work_stream
    O = oracle
    S, n = 100, 32 * 201
    ks = verifier.gen_keys(S)
    verifier.set_signatories(ks[0])
    db, _, _ = generate(verifier, 1, n, S, adv, keys=ks)
    ws = work_stream()
    with torch.cuda.stream(ws):
        verdict = torch.empty(n, dtype=torch.uint8, device="cuda")
        bitmap = torch.zeros((n + 31) // 32, dtype=torch.int32, device="cuda")
    cs = db.c_struct()
    verifier.verify_batch_device(cs, verdict.data_ptr(), None, None, bitmap.data_ptr(), ws.cuda_stream)
    ws.synchronize()
    f = quorum.thresholds(S)[0]
    res = verifier.decide_ordered_device(cs, bitmap.data_ptr(), f, schedule=ks[0], stream=ws.cuda_stream)
    hb = db.to_host()
    verdicts = verdict.cpu().numpy().tolist()
    sched = [ks[0][k].tobytes() for k in range(S)]
    ob = from_np(hb)
    PC.same_as(res, PC.restate(ob, verdicts, f, sched))
    WC.same_when(res, WC.replay(ob, verdicts, f, sched))
    _bits_agree(res)
    _same_rows(res, verifier.decide_device(cs, bitmap.data_ptr(), f, schedule=ks[0], stream=ws.cuda_stream))
    if adv == 0:
        assert len(res) == 32 and (res.when[:, [0, 2, 3, 4]] != NEVER).all()   # 100 signers' votes per type
        assert (res.exact_until != NEVER).all()
