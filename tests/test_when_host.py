"""tests/when_cases.py -- the sequential replay that hd_decide_ordered is
checked against -- pinned without a GPU:

- hand-worked batches: a propose after and before its 2f+1 prevotes, the window
  of the precommit equality, a valid-round trigger that is a prevote of the
  earlier round, the proposer's trace entry;
- the host vote table (hyperdrive_amd.votes.VoteLog.insert_batch, f set): on
  single-height, propose-free batches its per-message crossing events are the
  replay's when[0] / when[2] / when[4];
- the prefix property against propose_cases.restate: when[k] = i means bit k
  is set on the batch cut after message i and clear on the batch cut before
  it; for the monotone bits NEVER means the whole batch leaves the bit clear."""
import random

import numpy as np
import pytest

import hd_pyoracle as O
import propose_cases as PC
import when_cases as WC
from util import to_np

NEVER = WC.NEVER
PV, PC_, PR = O.PREVOTE, O.PRECOMMIT, O.PROPOSE


def _sig(k):
    return O.sha256(b"w" + bytes([k]))


def _batch(msgs):
    ob = O.Batch()
    for t, h, r, vr, value, k in msgs:
        ob.append(t, h, r, vr, value, _sig(k), bytes(65))
    return ob


def _replay(msgs, f, **kw):
    ob = _batch(msgs)
    return WC.replay(ob, [O.VALID] * len(ob), f, **kw)


V = O.canonical_value(1, 1)
V2 = O.canonical_value(1, 2)


def test_propose_after_its_prevotes():
    # f = 1: prevotes 0, 1, 2 for V, the propose at 3
    logs = _replay([(PV, 1, 0, -1, V, 0), (PV, 1, 0, -1, V, 1), (PV, 1, 0, -1, V, 2), (PR, 1, 0, -1, V, 9)], 1)
    x = logs[(1, 0)]
    assert x.when == [2, NEVER, NEVER, NEVER, 1, 3, NEVER, NEVER] and x.exact_until == NEVER and x.first == 0


def test_propose_before_its_prevotes():
    # the propose first; a prevote for another value and a repeated vote do not count
    logs = _replay([(PR, 1, 0, -1, V, 9), (PV, 1, 0, -1, V, 0), (PV, 1, 0, -1, V2, 1), (PV, 1, 0, -1, V, 0),
                    (PV, 1, 0, -1, V, 2), (PV, 1, 0, -1, V, 3)], 1)
    x = logs[(1, 0)]
    # timeout_prevote at the third logged prevote (index 4); the third for V at 5;
    # skip (f+1 = 2 trace entries): the proposer at 0 and signer 0 at 1
    assert x.when == [4, NEVER, NEVER, NEVER, 1, 5, NEVER, NEVER] and x.first == 0


def test_exact_window():
    # f = 1: precommits 0..4 of five signers, a double vote between them
    msgs = [(PC_, 1, 0, -1, V, 0), (PC_, 1, 0, -1, V, 1), (PC_, 1, 0, -1, V2, 1), (PC_, 1, 0, -1, V, 2),
            (PV, 1, 0, -1, V, 7), (PC_, 1, 0, -1, V, 3), (PC_, 1, 0, -1, V, 4)]
    x = _replay(msgs, 1)[(1, 0)]
    assert (x.when[2], x.when[3], x.exact_until) == (3, 3, 5)
    # exactly 2f+1: the window never closes
    x = _replay(msgs[:5], 1)[(1, 0)]
    assert (x.when[2], x.when[3], x.exact_until) == (3, 3, NEVER)
    # 2f: never
    x = _replay(msgs[:3], 1)[(1, 0)]
    assert (x.when[2], x.when[3], x.exact_until) == (NEVER, NEVER, NEVER)
    # f = 0: the first precommit opens the window, the second closes it
    x = _replay(msgs, 0)[(1, 0)]
    assert (x.when[2], x.when[3], x.exact_until) == (0, 0, 1)


def test_valid_round_trigger_is_a_prevote_of_the_earlier_round():
    # the propose of round 3 names round 1; round 1's third prevote for V comes last
    msgs = [(PV, 1, 1, -1, V, 0), (PV, 1, 1, -1, V, 1), (PR, 1, 3, 1, V, 9), (PV, 1, 3, -1, V, 0),
            (PV, 1, 1, -1, V2, 2), (PV, 2, 1, -1, V, 3), (PV, 1, 1, -1, V, 3)]
    logs = _replay(msgs, 1)
    assert logs[(1, 3)].when[7] == 6 and logs[(1, 3)].first == 2
    assert logs[(1, 1)].when == [4, NEVER, NEVER, NEVER, 1, NEVER, NEVER, NEVER]
    # the crossing before the propose: the propose is the trigger
    logs = _replay(msgs[:2] + [msgs[6], msgs[2]], 1)
    assert logs[(1, 3)].when[7] == 3
    # an invalid (nil) propose still carries its valid round, but no value rules and no trace entry
    logs = _replay([(PV, 1, 1, -1, O.NIL_VALUE, 0), (PR, 1, 3, 1, O.NIL_VALUE, 9)], 0)
    assert logs[(1, 3)].when == [NEVER, NEVER, NEVER, NEVER, NEVER, NEVER, NEVER, 1]


def test_proposer_trace_entry():
    # f = 1 (two entries): the proposer's own later votes are no new entry
    logs = _replay([(PR, 1, 0, -1, V, 5), (PV, 1, 0, -1, V, 5), (PC_, 1, 0, -1, V, 5), (PC_, 1, 0, -1, V, 6)], 1)
    assert logs[(1, 0)].when[4] == 3
    # the proposer voted first: the propose is no new entry
    logs = _replay([(PV, 1, 0, -1, V, 5), (PR, 1, 0, -1, V, 5), (PV, 1, 0, -1, V, 6)], 1)
    assert logs[(1, 0)].when[4] == 2
    # an unacceptable value: logged, not traced
    ob = _batch([(PV, 1, 0, -1, V, 6), (PR, 1, 0, -1, V, 5), (PV, 1, 0, -1, V, 7)])
    logs = WC.replay(ob, [O.VALID] * 3, 1, value_ok=[1, 0, 1])
    assert logs[(1, 0)].when[4] == 2 and logs[(1, 0)].propose == 1
    logs = WC.replay(ob, [O.VALID] * 3, 1)
    assert logs[(1, 0)].when[4] == 1


def test_firings_order():
    logs = _replay([(PV, 1, 0, -1, V, 0), (PC_, 1, 1, -1, V, 0), (PR, 1, 0, -1, V, 0)], 0)
    assert WC.firings(logs) == [(0, 1, 0, "timeout_prevote"), (0, 1, 0, "skip"),
                                (1, 1, 1, "timeout_precommit_reached"), (1, 1, 1, "timeout_precommit_exact"),
                                (1, 1, 1, "skip"), (2, 1, 0, "precommit_value")]


# ---- the host vote table's crossing events ------------------------------------
@pytest.mark.parametrize("seed", range(3))
def test_votelog_events_are_the_replay(seed):
    from hyperdrive_amd import votes as VL
    rng = random.Random(40 + seed)
    f = 2 + seed
    sigs = [_sig(k) for k in range(3 * f + 4)]
    vals = [V, V2, O.NIL_VALUE]
    ob, verdicts, _ = WC.mix(rng, 600, [5], [0, 1, 2], sigs, vals, 0.0)
    logs = WC.replay(ob, verdicts, f)
    v = VL.VoteLog(5)
    v.set_f(f)
    v.insert_batch(to_np(ob), np.array(verdicts, np.uint8))
    ev = v.last_events
    v.close()
    seen = {k: {} for k in (VL.EV_PREVOTE_2F1, VL.EV_PRECOMMIT_2F1, VL.EV_TRACE_F1)}
    for i in range(len(ob)):
        for bit in seen:
            if int(ev[i]) & bit:
                assert ob.round[i] not in seen[bit], "one crossing per round and rule"
                seen[bit][ob.round[i]] = i
    for (h, r), x in logs.items():
        assert seen[VL.EV_PREVOTE_2F1].get(r, NEVER) == x.when[0]
        assert seen[VL.EV_PRECOMMIT_2F1].get(r, NEVER) == x.when[2] == x.when[3]
        assert seen[VL.EV_TRACE_F1].get(r, NEVER) == x.when[4]
    assert any(x.when[2] != NEVER and x.exact_until != NEVER for x in logs.values())


# ---- the prefix property ------------------------------------------------------
def _cut(ob, n):
    out = O.Batch()
    for i in range(n):
        out.append(ob.mtype[i], ob.height[i], ob.round[i], ob.valid_round[i], ob.value[i], ob.frm[i], ob.sig[i])
    return out


def _bit(want, key, k):
    row = want.row(*key)
    return bool(row is not None and (row["bits"] >> k) & 1)


@pytest.mark.parametrize("seed,with_schedule", [(0, False), (1, True), (2, False)])
def test_prefix_property(seed, with_schedule):
    rng = random.Random(70 + seed)
    sigs = [_sig(k) for k in range(9)]
    vals = [V, V2, O.NIL_VALUE]
    sched = sigs if with_schedule else None
    f = 1 + seed % 2
    ob, verdicts, value_ok = WC.mix(rng, 300, [1, 2], [0, 1, 2], sigs, vals, 1 / 12, sched, valid_rounds=(-1, 0, 1, 2))
    logs = WC.replay(ob, verdicts, f, sched, value_ok)
    cuts = {}

    def restated(n):
        if n not in cuts:
            cuts[n] = PC.restate(_cut(ob, n), verdicts[:n], f, sched, value_ok[:n])
        return cuts[n]

    whole = restated(len(ob))
    assert sorted(logs) == sorted((x["height"], x["round"]) for x in whole.rows)
    fired = set()
    for key, x in logs.items():
        assert x.first == whole.row(*key)["rep"]
        for k in range(8):
            i = x.when[k]
            if i == NEVER:
                if k != 3:
                    assert not _bit(whole, key, k), (key, k)
                continue
            fired.add(k)
            assert _bit(restated(i + 1), key, k) and not _bit(restated(i), key, k), (key, k, i)
        if x.exact_until != NEVER:
            u = x.exact_until
            assert x.when[3] < u
            assert _bit(restated(u), key, 3) and not _bit(restated(u + 1), key, 3), key
        assert _bit(whole, key, 3) == (x.when[3] != NEVER and x.exact_until == NEVER)
    assert fired >= ({0, 2, 3, 4} if with_schedule else {0, 2, 3, 4, 5, 7}), fired   # most proposes are out of turn
