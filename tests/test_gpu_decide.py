"""hd_decide / hd_decide_device_bitmap (through the Python face and the C ABI)
against the oracle's tally and predicates and the restatement of insertPropose
(tests/propose_cases.py; process/process.go:758-819).  Every case passes its
verdicts directly and carries 65 zero bytes as signatures: no crypto runs,
except in the device-entry case, which verifies a generated batch first."""
import ctypes
import random

import numpy as np
import pytest

import propose_cases as PC
from tally_cases import _sig, scenarios
from util import from_np, to_np

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def verifier(gpu):
    v = gpu.Verifier(0)
    yield v
    v.close()


def _rows(sigs):
    return np.frombuffer(b"".join(sigs), np.uint8).reshape(len(sigs), 32).copy()


def _decide(verifier, ob, verdicts, f, schedule=None, value_ok=None):
    return verifier.decide(to_np(ob), np.array(verdicts, np.uint8), f,
                           schedule=_rows(schedule) if schedule is not None else None,
                           value_ok=np.array(value_ok, np.uint8) if value_ok is not None else None)


def _check(verifier, oracle, ob, verdicts, f, schedule=None, value_ok=None):
    """decide == the restatement, exactly; returns (result, restatement)."""
    res = _decide(verifier, ob, verdicts, f, schedule, value_ok)
    want = PC.restate(ob, verdicts, f, schedule, value_ok)
    PC.same_as(res, want)
    return res, want


def _row(res, h, r):
    hit = [k for k in range(len(res)) if (int(res.height[k]), int(res.round[k])) == (h, r)]
    assert len(hit) == 1, (h, r, hit)
    return {name: int(getattr(res, name)[hit[0]]) for name in PC.ROW_FIELDS}


def _with(ob, pos, msg):
    """A copy of the oracle batch with msg inserted before position pos."""
    import hd_pyoracle as O
    out = O.Batch()
    for i in range(len(ob) + 1):
        if i == pos:
            out.append(*msg)
        if i < len(ob):
            out.append(ob.mtype[i], ob.height[i], ob.round[i], ob.valid_round[i], ob.value[i], ob.frm[i], ob.sig[i])
    return out


# ---- 1. the threshold scenarios with a propose added ------------------------
@pytest.mark.parametrize("sc", scenarios(), ids=lambda s: s.name)
def test_scenarios_with_a_propose(verifier, oracle, sc):
    """Signers 0..39 are admitted (dense log cells), the rest take the hashed
    table.  The propose comes from signer 0, who votes in every expected round,
    so the scenarios' own `skip` expectations hold."""
    O = oracle
    verifier.set_signatories(_rows([_sig(k) for k in range(40)]))
    rng = random.Random(sc.name)
    _check(verifier, O, sc.b, sc.verdicts(), sc.f)          # no propose at all
    for h, r, pvalue, pvalid, want in sc.expect:
        variants = [(pvalue, None)] if pvalid else [(O.NIL_VALUE, None), (pvalue, 0)]
        for value, ok in variants:
            pos = rng.randrange(len(sc.b) + 1)
            ob = _with(sc.b, pos, (O.PROPOSE, h, r, -1, value, _sig(0), bytes(65)))
            verdicts = [O.VALID] * len(ob)
            value_ok = None
            if ok is not None:
                value_ok = [1] * len(ob)
                value_ok[pos] = ok
            res, _ = _check(verifier, O, ob, verdicts, sc.f, None, value_ok)
            ot = O.tally(ob, verdicts)
            voted = {ob.frm[i] for i in range(len(ob))
                     if ot.dup[i] == 0 and (ob.height[i], ob.round[i]) == (h, r)}
            d = O.decide_round(ot, h, r, sc.f, value, pvalid, -1, pvalid and _sig(0) not in voted)
            row = _row(res, h, r)
            assert row["bits"] == sum(1 << k for k, name in enumerate(PC.BIT_KEYS) if d[name])
            assert res.decisions[(h, r)] == d
            for k, v in want.items():
                assert res.decisions[(h, r)][k] == v, (sc.name, k)
            assert row["propose"] == pos and res.proposes[(h, r)] == pos
            assert row["prevotes"] == ot.distinct.get((h, r, O.PREVOTE), 0)
            assert row["precommits"] == ot.distinct.get((h, r, O.PRECOMMIT), 0)
            assert row["pv_value"] == ot.count.get((h, r, O.PREVOTE, value), 0)
            assert row["pc_value"] == ot.count.get((h, r, O.PRECOMMIT, value), 0)
            assert row["pv_nil"] == ot.count.get((h, r, O.PREVOTE, O.NIL_VALUE), 0)


# ---- 2. the propose log classes ---------------------------------------------
def _class_batch(O, sched):
    v, v2 = O.canonical_value(3, 2), O.canonical_value(3, 9)
    big = 2**63 - 1
    turn = lambda h, r: sched[((h % 2**64) + (r % 2**64)) % 2**64 % len(sched)]
    ob = O.Batch()
    P = O.PROPOSE
    ob.append(P, 3, 2, -1, v, sched[0], bytes(65))              # 0 out of turn (turn is 5)
    ob.append(P, 3, 2, -1, v, sched[5], bytes(65))              # 1 not VALID
    ob.append(P, 3, 2, -1, v, sched[5], bytes(65))              # 2 logged
    ob.append(P, 3, 2, -1, v, sched[5], b"\x07" * 65)           # 3 identical but for the signature
    ob.append(P, 3, 2, -1, v2, sched[5], bytes(65))             # 4 another value
    ob.append(P, 3, 2, 1, v, sched[5], bytes(65))               # 5 another valid_round
    ob.append(O.PREVOTE, 3, 2, -1, v, sched[1], bytes(65))      # 6
    ob.append(P, 3, 3, -1, O.NIL_VALUE, sched[6], bytes(65))    # 7 nil: logged, invalid, not traced
    ob.append(P, 3, -1, -1, v, sched[2], bytes(65))             # 8 round -1
    ob.append(P, 0, 0, -1, v, sched[0], bytes(65))              # 9 height 0 under a schedule
    ob.append(P, -3, 3, -1, v, sched[0], bytes(65))             # 10 height -3
    ob.append(P, big, 5, -1, v, turn(big, 5), bytes(65))        # 11 uint64 turn: logged
    ob.append(P, big, 6, -1, v, turn(big, 5), bytes(65))        # 12 the neighbour's turn: out of turn
    verdicts = [O.VALID] * len(ob)
    verdicts[1] = O.BAD_RS
    return ob, verdicts


def test_propose_log_classes(verifier, oracle):
    O = oracle
    sched = [O.sha256(b"sched" + bytes([k])) for k in range(7)]
    verifier.set_signatories(_rows(sched))
    ob, verdicts = _class_batch(O, sched)
    assert (2**63 - 1 + 5) % 7 != (2**63 - 1 + 6) % 7
    res, want = _check(verifier, O, ob, verdicts, 1, sched)
    assert res.pclass.tolist() == [4, 3, 0, 1, 2, 2, 3, 0, 3, 3, 3, 0, 4]
    assert res.proposes == {(3, 2): 2, (3, 3): 7, (2**63 - 1, 5): 11}
    assert (_row(res, 3, 3)["flags"], _row(res, 3, 3)["trace"]) == (1, 0)
    assert (_row(res, 3, 2)["flags"], _row(res, 3, 2)["trace"], _row(res, 3, 2)["rep"]) == (7, 2, 2)
    # without a schedule the first VALID propose of a round is the logged one
    res, want = _check(verifier, O, ob, verdicts, 1, None)
    assert res.pclass.tolist() == [0, 3, 2, 2, 2, 2, 3, 0, 3, 0, 0, 0, 0]
    assert res.proposes[(3, 2)] == 0 and res.proposes[(0, 0)] == 9 and res.proposes[(-3, 3)] == 10


# ---- 3. the trace boundary ----------------------------------------------------
@pytest.mark.parametrize("case", ["new", "voted_dense", "voted_hashed", "nil_new", "propose_only_f0"])
def test_trace_boundary(verifier, oracle, case):
    O = oracle
    f = 4
    sig = lambda k: O.sha256(b"t" + bytes([k]))
    verifier.set_signatories(_rows([sig(k) for k in range(10)]))     # signer 15 is outside the set
    v = O.canonical_value(1, 2)
    ob = O.Batch()
    voters = [0, 1, 2, 15]
    if case != "propose_only_f0":
        for j, k in enumerate(voters):
            ob.append(O.PREVOTE if j % 2 else O.PRECOMMIT, 1, 2, -1, v, sig(k), bytes(65))
    frm, value = {"new": (sig(20), v), "voted_dense": (sig(0), v), "voted_hashed": (sig(15), v),
                  "nil_new": (sig(20), O.NIL_VALUE), "propose_only_f0": (sig(20), v)}[case]
    ob.append(O.PROPOSE, 1, 2, -1, value, frm, bytes(65))
    if case == "propose_only_f0":
        f = 0
    res, _ = _check(verifier, O, ob, [O.VALID] * len(ob), f)
    row = _row(res, 1, 2)
    skip = res.decisions[(1, 2)]["skip"]
    if case == "new":
        assert (skip, row["trace"], row["flags"]) == (True, f + 1, 7)
    elif case in ("voted_dense", "voted_hashed"):
        assert (skip, row["trace"], row["flags"]) == (False, f, 3)
    elif case == "nil_new":
        assert (skip, row["trace"], row["flags"]) == (False, f, 1)
    else:
        assert len(res) == 1 and (skip, row["trace"], row["flags"], row["rep"], row["prevotes"]) == (True, 1, 7, 0, 0)


# ---- 4. the valid round -------------------------------------------------------
@pytest.mark.parametrize("case", ["2f1", "2f", "empty_round", "own_round", "later_round", "other_height"])
def test_valid_round(verifier, oracle, case):
    O = oracle
    f, h = 2, 4
    sig = lambda k: O.sha256(b"vr" + bytes([k]))
    verifier.set_signatories(_rows([sig(k) for k in range(3)]))       # both log paths
    v = O.canonical_value(h, 1)
    ob = O.Batch()
    n_pv = 2 * f if case in ("2f", "other_height") else 2 * f + 1
    for k in range(n_pv):
        ob.append(O.PREVOTE, h, 1, -1, v, sig(k), bytes(65))
    if case == "other_height":                                         # must not leak into height h
        for k in range(2 * f + 1):
            ob.append(O.PREVOTE, h + 1, 1, -1, v, sig(k), bytes(65))
    if case in ("own_round", "later_round"):                           # votes at (h, 3) and (h, 5) as well
        for k in range(2 * f + 1):
            ob.append(O.PREVOTE, h, 3, -1, v, sig(k), bytes(65))
            ob.append(O.PREVOTE, h, 5, -1, v, sig(k), bytes(65))
    vr = {"empty_round": 2, "own_round": 3, "later_round": 5}.get(case, 1)
    ob.append(O.PROPOSE, h, 3, vr, v, sig(9), bytes(65))
    verdicts = [O.VALID] * len(ob)
    res, _ = _check(verifier, O, ob, verdicts, f)
    row = _row(res, h, 3)
    ot = O.tally(ob, verdicts)
    d = O.decide_round(ot, h, 3, f, v, True, vr, True)
    assert res.decisions[(h, 3)] == d
    if case == "2f1":
        assert (row["pv_validround"], row["bits"] >> 7, row["prevotes"], row["rep"]) == (2 * f + 1, 1, 0, len(ob) - 1)
    elif case in ("2f", "other_height"):
        assert (row["pv_validround"], row["bits"] >> 7) == (2 * f, 0)
    elif case == "empty_round":
        assert (row["pv_validround"], row["bits"] >> 7) == (0, 0)
    else:
        assert (row["pv_validround"], row["bits"] >> 7) == (2 * f + 1, 1) and d["prevote_validround"]


# ---- 5. random mixes ----------------------------------------------------------
def _mix(O, rng, n, heights, rounds, sigs, vals, p_propose, sched=None, p_bad=0.1):
    ob = O.Batch()
    proposes = []
    for _ in range(n):
        h, r = rng.choice(heights), rng.choice(rounds)
        if rng.random() < p_propose:
            frm = rng.choice(sigs)
            if sched is not None and h > 0 and rng.random() < 0.7:
                frm = PC.scheduled(sched, h, r)
            msg = (O.PROPOSE, h, r, rng.choice([-1, 0, 1, 2, 3]), rng.choice(vals), frm)
            if proposes and rng.random() < 0.25:      # an earlier propose again, under another signature
                msg = rng.choice(proposes)
            proposes.append(msg)
            ob.append(*msg, bytes([rng.randrange(256)]) * 65)
        else:
            ob.append(rng.choice([O.PREVOTE, O.PRECOMMIT]), h, r, -1, rng.choice(vals), rng.choice(sigs), bytes(65))
    verdicts = [O.VALID if rng.random() >= p_bad else O.BAD_RS for _ in range(n)]
    value_ok = [1 if rng.random() < 0.8 else 0 for _ in range(n)]
    return ob, verdicts, value_ok


@pytest.mark.parametrize("with_schedule", [True, False])
def test_dense_mix(verifier, oracle, with_schedule):
    O = oracle
    rng = random.Random(5)
    sigs = [O.sha256(b"d" + bytes([k])) for k in range(70)]
    vals = [O.canonical_value(1, k) for k in range(3)] + [O.NIL_VALUE]
    verifier.set_signatories(_rows(sigs[:35]))
    sched = sigs if with_schedule else None
    ob, verdicts, value_ok = _mix(O, rng, 6000, [1, 2, 3], [-1, 0, 1, 2, 3], sigs, vals, 1 / 40, sched)
    res, want = _check(verifier, O, ob, verdicts, 70 // 3, sched, value_ok)
    assert len(want.proposes) >= 6 and set(want.pclass) >= ({0, 1, 2, 3, 4} if with_schedule else {0, 1, 2, 3})


def test_sparse_mix(verifier, oracle):
    """300 rounds over 4,000 messages: a wavefront's lanes do not share a round."""
    O = oracle
    rng = random.Random(6)
    sigs = [O.sha256(b"s" + bytes([k])) for k in range(40)]
    vals = [O.canonical_value(2, k) for k in range(2)] + [O.NIL_VALUE]
    verifier.set_signatories(_rows(sigs[:20]))
    ob, verdicts, value_ok = _mix(O, rng, 4000, list(range(1, 31)), list(range(10)), sigs, vals, 1 / 10)
    res, want = _check(verifier, O, ob, verdicts, 1, None, value_ok)
    assert len(res) > 290 and len(set(res.bits.tolist())) > 2


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_edge_sizes(verifier, oracle, n):
    O = oracle
    sigs = [O.sha256(b"e" + bytes([k])) for k in range(6)]
    vals = [O.canonical_value(1, 0), O.NIL_VALUE]
    verifier.set_signatories(_rows(sigs[:3]))
    for seed in range(3):
        rng = random.Random(100 * n + seed)
        ob, verdicts, value_ok = _mix(O, rng, n, [1, 2], [0, 1], sigs, vals, 1 / 4, None, 0.05)
        _check(verifier, O, ob, verdicts, 1, None, value_ok)
    # the last message alone is a candidate
    ob = O.Batch()
    for i in range(n):
        ob.append(O.PROPOSE, 1, 0, -1, vals[0], sigs[0], bytes(65))
    res, _ = _check(verifier, O, ob, [O.BAD_RS] * (n - 1) + [O.VALID], 0)
    assert len(res) == 1 and int(res.rep[0]) == n - 1 and res.proposes == {(1, 0): n - 1}


def test_empty_batch(verifier, oracle):
    O = oracle
    ob = O.Batch()
    for t in (1, 2, 3, 1):
        ob.append(t, 1, 0, -1, bytes(32), O.sha256(b"x"), bytes(65))
    res, _ = _check(verifier, O, ob, [O.BAD_RS, O.NOT_ADMITTED, O.BAD_RS, O.NO_POINT], 1)
    assert len(res) == 0 and res.pclass.tolist() == [3] * 4 and res.dup.tolist() == [3] * 4


# ---- 6. the tables stay clean -------------------------------------------------
def _equal(a, b):
    for k in PC.ROW_FIELDS + ("pclass", "dup"):
        assert getattr(a, k).tolist() == getattr(b, k).tolist(), k


def test_tables_stay_clean(verifier, oracle):
    from hyperdrive_amd import _lib
    O = oracle
    rng = random.Random(9)
    sigs = [O.sha256(b"c" + bytes([k])) for k in range(30)]
    vals = [O.canonical_value(1, k) for k in range(2)] + [O.NIL_VALUE]
    verifier.set_signatories(_rows(sigs[:15]))
    ob, verdicts, value_ok = _mix(O, rng, 3000, [1, 2, 3, 4], list(range(6)), sigs, vals, 1 / 8)
    first, want = _check(verifier, O, ob, verdicts, 3, None, value_ok)
    tal = verifier.tally(to_np(ob), np.array(verdicts, np.uint8))
    ot = O.tally(ob, verdicts)
    assert (tal.count, tal.distinct, tal.distinct_any, tal.dup.tolist()) == (ot.count, ot.distinct, ot.distinct_any,
                                                                            ot.dup)
    _equal(_decide(verifier, ob, verdicts, 3, None, value_ok), first)
    # a capacity below the row count: HD_ECAP with the need, and the next call is right
    lib = _lib.load()
    nb = to_np(ob)
    o, a = verifier._decide_struct(len(ob), cap=len(first) - 1)
    cin = _lib.HdDecideIn(3, 0, None, None)
    cb = nb.c_struct()
    v = np.array(verdicts, np.uint8)
    rc = lib.hd_decide(verifier.handle, ctypes.byref(cb), v.ctypes.data, ctypes.byref(cin), ctypes.byref(o))
    assert rc == _lib.HD_ECAP and o.n == len(first)
    PC.same_as(_decide(verifier, ob, verdicts, 3), PC.restate(ob, verdicts, 3))
    tal = verifier.tally(nb, v)
    assert (tal.count, tal.dup.tolist()) == (ot.count, ot.dup)


def test_more_rounds_than_staged(gpu, oracle):
    """A fresh context stages 1,024 rows: a batch of 1,500 rounds takes the
    overflow columns, the next call the grown stage; both equal the restatement."""
    O = oracle
    v = gpu.Verifier(0)
    try:
        ob = O.Batch()
        val = O.canonical_value(1, 0)
        for k in range(1500):
            t = O.PROPOSE if k % 3 == 0 else O.PREVOTE
            ob.append(t, 1 + k // 50, k % 50, -1, val, O.sha256(b"o" + bytes([k % 7])), bytes(65))
        for _ in range(2):
            res, _w = _check(v, O, ob, [O.VALID] * len(ob), 0)
            assert len(res) == 1500
    finally:
        v.close()


# ---- 6b. one plan for tally and decide, across table capacities ---------------
def _capacity_sequence(hd, O):
    """Tally, decide and decide_ordered share one table plan on a context's
    buffers.  300 messages take tables of 1,024 slots and 3,000 take 8,192, so
    every step below meets tables the previous step left at the other capacity
    (or, from step 3 on, an allocation that is larger than the step needs).
    Each result equals the oracle / restatement / replay and the same call on a
    fresh context."""
    import when_cases as WC
    rng = random.Random(11)
    sigs = [O.sha256(b"p" + bytes([k])) for k in range(30)]
    vals = [O.canonical_value(1, k) for k in range(2)] + [O.NIL_VALUE]
    f = 3
    small = _mix(O, rng, 300, [1, 2], list(range(4)), sigs, vals, 1 / 8)
    big = _mix(O, rng, 3000, [1, 2, 3, 4], list(range(6)), sigs, vals, 1 / 8)

    def tally(v, mix):
        ob, verdicts, _ = mix
        tal = v.tally(to_np(ob), np.array(verdicts, np.uint8))
        return (tal.count, tal.distinct, tal.distinct_any, tal.dup.tolist())

    def tally_want(mix):
        ot = O.tally(mix[0], mix[1])
        return lambda got: got == (ot.count, ot.distinct, ot.distinct_any, ot.dup)

    def decide(v, mix):
        ob, verdicts, value_ok = mix
        res = _decide(v, ob, verdicts, f, None, value_ok)
        return tuple(getattr(res, k).tobytes() for k in PC.ROW_FIELDS + ("pclass", "dup")), res

    def decide_want(mix):
        want = PC.restate(mix[0], mix[1], f, None, mix[2])
        return lambda got: PC.same_as(got[1], want) is None

    def ordered(v, mix):
        ob, verdicts, value_ok = mix
        res = v.decide_ordered(to_np(ob), np.array(verdicts, np.uint8), f, value_ok=np.array(value_ok, np.uint8))
        rows = tuple(getattr(res, k).tobytes() for k in PC.ROW_FIELDS + ("pclass", "dup"))
        return rows + (res.when.tobytes(), res.exact_until.tobytes()), res

    def ordered_want(mix):
        want, logs = PC.restate(mix[0], mix[1], f, None, mix[2]), WC.replay(mix[0], mix[1], f, None, mix[2])
        return lambda got: PC.same_as(got[1], want) is None and WC.same_when(got[1], logs) is None

    steps = [(tally, tally_want, small), (decide, decide_want, big), (tally, tally_want, small),
             (ordered, ordered_want, big), (decide, decide_want, small), (tally, tally_want, big)]
    shared = hd.Verifier(0)
    try:
        shared.set_signatories(_rows(sigs[:15]))
        for k, (call, want, mix) in enumerate(steps):
            got = call(shared, mix)
            assert want(mix)(got), k
            fresh = hd.Verifier(0)
            try:
                fresh.set_signatories(_rows(sigs[:15]))
                alone = call(fresh, mix)
            finally:
                fresh.close()
            same = got == alone if call is tally else got[0] == alone[0]
            assert same, k
    finally:
        shared.close()


def test_plan_shared_across_capacities(gpu, oracle):
    _capacity_sequence(gpu, oracle)


def test_plan_shared_across_capacities_checked():
    """The same sequence with HD_TALLY_CHECK=1: every tally call then also
    asserts the table invariants and that the emit left the tables clean.  The
    variable is set for a fresh child process, so that nothing else in this
    process runs under it."""
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    code = ("import sys; sys.path[:0] = %r; import hd_pyoracle as O, hyperdrive_amd as hd, test_gpu_decide as T; "
            "T._capacity_sequence(hd, O); print('sequence ok')" % [here, root, os.path.join(root, "oracle")])
    r = subprocess.run([sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", code],
                       env=dict(os.environ, HD_TALLY_CHECK="1"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "sequence ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


# ---- 7. the device entry on generated data ------------------------------------
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
    res = verifier.decide_device(cs, bitmap.data_ptr(), f, schedule=ks[0], stream=ws.cuda_stream)
    hb = db.to_host()
    verdicts = verdict.cpu().numpy()
    sched = [ks[0][k].tobytes() for k in range(S)]
    PC.same_as(res, PC.restate(from_np(hb), verdicts.tolist(), f, sched))
    if adv == 0:
        assert (verdicts == 0).all()
        _equal(verifier.decide(hb, verdicts, f, schedule=ks[0]), res)
        assert sorted(res.proposes) == [(1, r) for r in range(32)]
        assert all(int(hb.type[p]) == 1 for p in res.proposes.values())
