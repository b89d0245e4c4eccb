"""The slot plan of a set change that re-tiers the key tables
(hyperdrive_amd/csrc/hd_keycarry.h) on the host.

The header is plain C++; the stand-alone program
tests/native/hd_keycarry_check.cpp runs it under ASan + UBSan, and its
adm_slot, carry list and counts must equal the model of key_carry_cases.py,
which is written from the contract: known keys (LEARNED or READY, outside the
foreign block) of signatories that stay take slots first, in sorted order, the
rest follow in sorted order, slot 0 is never assigned, and a known key without
a place is counted as dropped."""
import random

import pytest

import key_carry_cases as C

E, CL, L, R = C.EMPTY, C.CLAIMED, C.LEARNED, C.READY


@pytest.fixture(scope="module")
def prog():
    return C.build_check(sanitize=True)


def _old(sigs, states=None, first=1):
    """a snapshot of `sigs` in slots first, first + 1, ... and the state array
    (slot 0 and any gap below `first` EMPTY); every key READY unless given"""
    states = [R] * len(sigs) if states is None else states
    return [(s, first + k) for k, s in enumerate(sigs)], [E] * first + list(states)


def _check(prog, cases):
    got = C.run_check(prog, cases)
    want = [C.model(*c) for c in cases]
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"case {k}: got {g}, want {w}"
        adm = [s for s in g[0] if s >= 0]
        assert 0 not in adm and len(set(adm)) == len(adm)            # slot 0 is G's; no slot twice
        assert all(s < max(cases[k][5], 1) for s in adm)             # below max_slots
        assert g[2] == 1 + len(adm)                                    # slots count up from 1
    return got


def test_binding_of_the_set_change_info():
    # (the library itself is not loaded here)
    import ctypes
    from hyperdrive_amd import _lib
    assert "hd_ctx_set_change_info" in _lib.SIGNATURES
    assert [n for n, _ in _lib.HdSetChangeInfo._fields_] == ["width_before", "width_after", "kept", "carried", "dropped"]
    assert ctypes.sizeof(_lib.HdSetChangeInfo) == 20
    from hyperdrive_amd.verify import Verifier
    from hyperdrive_amd.multi import MultiVerifier
    assert callable(Verifier.last_set_change) and callable(MultiVerifier.last_set_change)


def test_identical_permuted_disjoint_and_overlapping_sets(prog):
    sigs = [C.sig(k) for k in range(12)]
    new = sorted(sigs)
    shuffled = sigs[:]
    random.Random(5).shuffle(shuffled)
    others = sorted(C.sig(100 + k) for k in range(12))
    overlap = sorted(sigs[:7] + [C.sig(200 + k) for k in range(6)])
    cases = [(*_old(sigs), 0, 0, new, 64), (*_old(shuffled), 0, 0, new, 64), (*_old(sigs), 0, 0, others, 64),
             (*_old(sigs), 0, 0, overlap, 64)]
    same, perm, disjoint, part = _check(prog, cases)
    assert (same[3], same[4]) == (12, 0) and sorted(same[0]) == list(range(1, 13))
    # a snapshot in another row order carries the same keys into the same slots
    assert perm[0] == same[0]
    assert [sigs[r] for r, _ in same[1]] == [shuffled[r] for r, _ in perm[1]] == new
    assert (disjoint[3], disjoint[4], disjoint[1]) == (0, 12, [])
    assert (part[3], part[4]) == (7, 5)
    kept = sorted(sigs[:7])
    assert [overlap[k] for k in range(13) if part[0][k] in range(1, 8)] == kept      # carried first, sorted
    assert sorted(part[0]) == list(range(1, 14))


def test_only_learned_and_ready_are_carried(prog):
    sigs = sorted(C.sig(k) for k in range(8))
    states = [E, CL, L, R, E, CL, L, R]
    (got,) = _check(prog, [(*_old(sigs, states), 0, 0, sigs, 64)])
    assert [sigs[r] for r, _ in got[1]] == [sigs[k] for k in (2, 3, 6, 7)]
    assert (got[3], got[4], got[5], got[6]) == (4, 0, 4, 4)
    # a state word that is none of the four is no key either
    (odd,) = _check(prog, [(*_old(sigs[:2], [7, 0xFFFFFFFF]), 0, 0, sigs, 64)])
    assert odd[3] == 0


def test_foreign_block_and_out_of_range_slots_are_never_carried(prog):
    sigs = sorted(C.sig(k) for k in range(6))
    snap, states = _old(sigs)                       # slots 1..6, all READY
    (got,) = _check(prog, [(snap, states, 3, 5, sigs, 64)])
    assert [r for r, _ in got[1]] == [0, 1, 4, 5]   # slots 3 and 4 are the foreign block's
    # a row in slot 0 (G's) and rows past the state array hold no key
    snap2 = [(sigs[0], 0), (sigs[1], 7), (sigs[2], 0xFFFFFFFF), (sigs[3], 2)]
    (edge,) = _check(prog, [(snap2, states, 0, 0, sigs, 64)])
    assert edge[1] == [(3, 1)] and edge[5] == 1


def test_fewer_slots_than_signatories(prog):
    """max_slots below the set size: the carried keys, though last in sorted
    order, take the slots; below even the carried count: the rest is dropped
    and counted."""
    new = sorted(C.sig(k) for k in range(50))
    last4 = new[-4:]
    snap, states = _old(last4)
    full, tight, two, none = _check(prog, [(snap, states, 0, 0, new, 39), (snap, states, 0, 0, new, 5),
                                          (snap, states, 0, 0, new, 3), (snap, states, 0, 0, new, 1)])
    assert full[0][-4:] == [1, 2, 3, 4] and full[0][:34] == list(range(5, 39)) and full[0][34:46] == [-1] * 12
    assert (full[3], full[4], full[2]) == (4, 0, 39)
    assert tight[0][-4:] == [1, 2, 3, 4] and set(tight[0][:-4]) == {-1}
    assert two[0][-4:] == [1, 2, -1, -1] and (two[3], two[4]) == (2, 2)
    assert set(none[0]) == {-1} and (none[3], none[4], none[2]) == (0, 4, 1)


@pytest.mark.parametrize("m", [0, 1, 1000])
def test_set_sizes(prog, m):
    new = sorted(C.sig(k) for k in range(m))
    half = new[::2]
    random.Random(m).shuffle(half)
    gone = [C.sig(5000 + k) for k in range(3)]
    snap, states = _old(half + gone)
    (got,) = _check(prog, [(snap, states, 0, 0, new, 1 << 20)])
    assert (got[3], got[4]) == (len(half), 3)
    assert sorted(s for s in got[0]) == list(range(1, m + 1))
    # and from nothing known: slots in sorted order, as a first mapping gives them
    (cold,) = _check(prog, [([], [], 0, 0, new, 1 << 20)])
    assert cold[0] == list(range(1, m + 1)) and cold[1] == []


def test_plan_follows_the_snapshot_not_the_live_map(prog):
    """The hazard of a failed attempt: it gave slots of departed signatories
    (states still READY, the departed keys) to new ones.  The plan is a
    function of the snapshot alone: the new signatories carry nothing, the
    ones that stayed carry their own rows, whatever the live map says by
    then -- and a plan wrongly fed that live map WOULD carry the departed
    keys for the new signatories, which is what the snapshot rule prevents."""
    old = sorted(C.sig(k) for k in range(30))
    snap, states = _old(old)
    stay, gone = old[:25], old[25:]
    fresh = [C.sig(900 + k) for k in range(7)]
    new = sorted(stay + fresh)
    # the failed attempt's live map: the five freed slots went to new signatories
    live = [(s, slot) for s, slot in snap if s in stay] + [(fresh[k], dict(snap)[gone[k]]) for k in range(5)]
    from_snap, from_live = _check(prog, [(snap, states, 0, 0, new, 64), (live, states, 0, 0, new, 64)])
    assert (from_snap[3], from_snap[4]) == (25, 5)
    assert sorted(snap[r][0] for r, _ in from_snap[1]) == stay
    slot_new = dict(zip(new, from_snap[0]))
    assert all(slot_new[s] > 25 for s in fresh)            # after every carried key
    assert from_live[3] == 30                               # the wrong source: five foreign keys carried
    # the same snapshot gives the same plan however the live map was shuffled
    again, = _check(prog, [(list(reversed(snap)), states, 0, 0, new, 64)])
    assert again[0] == from_snap[0]
