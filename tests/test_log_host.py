"""tests/log_cases.py pinned on the CPU: the retained-log model (kept messages
only, replayed at every insert) equals the one-shot yardstick over the
concatenation of everything inserted, under the index map "log position if
kept earlier, else base + i".  No library call; these make the expected values
of tests/test_gpu_log.py trustworthy."""
import random

import pytest

import hd_pyoracle as O
import log_cases as LC
import when_cases as WC

NEVER = LC.NEVER


def _stream(seed, n=None):
    rng = random.Random(seed)
    S = rng.choice([4, 7, 10])
    sigs = [O.sha256(b"L" + bytes([seed % 251, k])) for k in range(S)]
    vals = [O.canonical_value(5, k) for k in range(rng.choice([1, 2, 3]))] + [O.NIL_VALUE]
    sched = sigs if rng.random() < 0.5 else None
    heights = [5] if rng.random() < 0.5 else [5, 5, 5, 6, 4]
    n = n or rng.randrange(20, 90)
    ob, verdicts, value_ok = WC.mix(rng, n, heights, [-1, 0, 1, 2], sigs, vals, 1 / 6, sched,
                                    valid_rounds=(-1, 0, 1, 2))
    f = rng.choice([0, 1, (S - 1) // 3])
    cuts = sorted({0, n} | {rng.randrange(n + 1) for _ in range(rng.randrange(1, 7))})
    if rng.random() < 0.3:
        cuts = sorted(cuts + [cuts[len(cuts) // 2]])          # an empty piece
    return rng, ob, verdicts, value_ok if rng.random() < 0.7 else None, sched, f, cuts


@pytest.mark.parametrize("block", range(10))
def test_model_equals_the_concatenation(block):
    """300 seeded streams cut at random points."""
    fired = set()
    for seed in range(30 * block, 30 * block + 30):
        rng, ob, verdicts, value_ok, sched, f, cuts = _stream(seed)
        ys, md = LC.Stream(5, f, sched), LC.Model(5, f, sched)
        for lo, hi in zip(cuts, cuts[1:]):
            part = LC.cut(ob, verdicts, value_ok, lo, hi)
            want = ys.push(*part)              # raises KeyError if an index names a message that was not kept
            got = md.insert(*part)
            assert got == want, (seed, lo, hi)
            assert got.relogged == got.base == want.relogged
            assert got.kept == sum(1 for p in got.logpos if p != NEVER)
            fired |= {k for _, _, _, k in want.new_firings}
        assert len(md.kept) == ys.entries
        # the last insert's answer is the one-shot answer of the whole stream, up to the index map
        whole = LC.Stream(5, f, sched).push(ob, verdicts, value_ok)
        strip = lambda rows: [{k: v for k, v in x.items() if k not in ("rep", "propose")} for x in rows]
        assert strip(whole.rows) == strip(want.rows)
        assert [[w == NEVER for w in r] for r in whole.when] == [[w == NEVER for w in r] for r in want.when]
    assert len(fired) >= 5, fired


def test_every_reported_index_names_a_kept_message():
    """when / exact_until / rep / propose only ever name logged messages."""
    for seed in range(60):
        rng, ob, verdicts, value_ok, sched, f, _ = _stream(1000 + seed)
        e = LC.Stream(5, f, sched).push(ob, verdicts, value_ok)
        kept = {i for i, p in enumerate(e.logpos) if p != NEVER}
        named = {x["rep"] for x in e.rows} | {x["propose"] for x in e.rows if x["propose"] != NEVER}
        named |= {w for r in e.when for w in r if w != NEVER} | {u for u in e.exact_until if u != NEVER}
        assert named <= kept, (seed, sorted(named - kept))
        # on an empty log the positions are 0, 1, 2, ... in arrival order
        assert [p for p in e.logpos if p != NEVER] == list(range(e.kept))


def test_hand_worked_crossing_between_inserts():
    """f = 1: two prevotes in the first insert, the third (the 2f+1-th) in the
    second, behind a repeat and a conflicting copy of the first."""
    s = [O.sha256(bytes([k])) for k in range(4)]
    v, w = O.canonical_value(5, 0), O.canonical_value(5, 1)
    mk = lambda msgs: (lambda b: ([b.append(*m, bytes(65)) for m in msgs], b)[1])(O.Batch())
    for cls in (LC.Stream, LC.Model):
        lg = cls(5, 1)
        put = lg.push if cls is LC.Stream else lg.insert
        a = put(mk([(O.PREVOTE, 5, 0, -1, v, s[0]), (O.PREVOTE, 6, 0, -1, v, s[3]), (O.PREVOTE, 5, 0, -1, v, s[1])]),
                [O.VALID] * 3)
        assert (a.base, a.kept, a.logpos, a.dup) == (0, 2, [0, NEVER, 1], [0, 3, 0])
        assert a.when == [[NEVER] * 4 + [2] + [NEVER] * 3] and a.new_firings == [(2, 5, 0, "skip")]
        b = put(mk([(O.PREVOTE, 5, 0, -1, v, s[0]), (O.PREVOTE, 5, 0, -1, w, s[0]), (O.PREVOTE, 5, 0, -1, w, s[2])]),
                [O.VALID] * 3)
        assert (b.base, b.kept, b.logpos, b.dup) == (2, 1, [NEVER, NEVER, 2], [1, 2, 0])
        assert b.when == [[4, NEVER, NEVER, NEVER, 1, NEVER, NEVER, NEVER]]      # base + 2, and the old skip
        assert b.new_firings == [(2, 5, 0, "timeout_prevote")] and b.rows[0]["rep"] == 0
        c = put(O.Batch(), [])
        assert (c.base, c.kept, c.new_firings) == (3, 0, [])
        assert c.when == [[2, NEVER, NEVER, NEVER, 1, NEVER, NEVER, NEVER]]      # both are log positions now
