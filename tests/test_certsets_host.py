"""hd_check_certificates_sets and hd_sigsets without a GPU: the model of
tests/certsets_cases.py pinned on hand-worked segments; the set builder
(hyperdrive_amd/csrc/hd_sigsets.h sigset_build, sigset_place) against Python;
and the kernel's arithmetic replayed lane by lane under ASan + UBSan by
tests/native/hd_certsets_check.cpp -- a stand-alone program, run as a
subprocess -- over the synthetic cases the GPU test runs, on both table
placements and in three lane orders: the results must equal the model's
whatever the order."""
import ctypes

import pytest

import certsets_cases as SC
from certsets_cases import (BAD_RS, BAD_SIGNATURE, NOT_ADMITTED, NOT_MEMBER, OK, REPEATED_SENDER, SHORT, VALID,
                            WRONG_FIELD)
from cert_cases import NEVER, PRECOMMIT, PREVOTE, Cert, value

GUIDE_LDS = 160 * 1024   # what one CDNA4 workgroup may allocate
THRESHOLD = (GUIDE_LDS - 256) // 4   # cert_lds_entries(GUIDE_LDS); test_cert_host.py pins the formula


@pytest.fixture(scope="module")
def prog():
    return SC.build_check(sanitize=True)


# ---- 1. the model, on hand-worked segments ----------------------------------------------
A, B = value(1), value(2)
a, b, c, d, e, x = (bytes([k]) * 32 for k in (1, 2, 3, 4, 5, 9))
SETS = [[a, b, c, d], [c, b, a, e, e], []]   # x is in none; set 1 has a duplicate row


def _hand():
    """eight messages from a b c a x d e b; message 2 has verdict BAD_RS, message 5 value B, message 6
    verdict NOT_ADMITTED (authentic), every other VALID and (PRECOMMIT, 5, 2, A)"""
    types = [PRECOMMIT] * 8
    heights = [5] * 8
    rounds = [2] * 8
    values = [A, A, A, A, A, B, A, A]
    froms = [a, b, c, a, x, d, e, b]
    verdicts = [VALID, VALID, BAD_RS, VALID, VALID, VALID, NOT_ADMITTED, VALID]
    return types, heights, rounds, values, froms, verdicts


def _one(first, count, sid, quorum=1, t=PRECOMMIT, h=5, r=2, v=A):
    (res,) = SC.check_sets([Cert(first, count, quorum, t, h, r, v)], [sid], SETS, *_hand())
    return res


def test_model_each_status():
    assert _one(0, 2, 0, 2) == (OK, 2, NEVER)
    assert _one(0, 2, 0, 3) == (SHORT, 2, NEVER)
    assert _one(0, 0, 0) == (SHORT, 0, NEVER)                  # the empty segment
    assert _one(1, 2, 0) == (BAD_SIGNATURE, 1, 2)              # verdict BAD_RS
    assert _one(3, 2, 0) == (NOT_MEMBER, 1, 4)                 # x is in no set
    assert _one(5, 1, 0) == (WRONG_FIELD, 0, 5)                # the value
    assert _one(0, 4, 0, v=A)[0] == BAD_SIGNATURE              # message 2 before the repeat at 3
    assert _one(3, 1, 0, t=PREVOTE) == (WRONG_FIELD, 0, 3)
    assert _one(6, 1, 1) == (OK, 1, NEVER)                     # NOT_ADMITTED is authentic; e is in set 1
    assert _one(6, 1, 0) == (NOT_MEMBER, 0, 6)                 # ... and in set 1 only
    assert _one(5, 1, 1, v=B) == (NOT_MEMBER, 0, 5)            # d is in set 0 only
    assert _one(0, 2, 2) == (NOT_MEMBER, 0, 0)                 # the empty set
    assert _one(2, 1, 2) == (BAD_SIGNATURE, 0, 2)              # ... not authentic comes first


def test_model_precedence_and_repeats():
    types, heights, rounds, values, froms, verdicts = _hand()
    verdicts[2] = VALID
    run = lambda sid, first=0, count=8, **kw: SC.check_sets(
        [Cert(first, count, kw.get("quorum", 1), PRECOMMIT, 5, 2, kw.get("v", A))], [sid], SETS, types, heights,
        rounds, values, froms, verdicts)[0]
    # set 0: a b c count, message 3 repeats a, x is outside, d is wrong, e is outside, b repeats
    assert run(0) == (REPEATED_SENDER, 3, 3)
    assert run(0, quorum=9) == (SHORT, 3, 3)
    # set 1: d is not a member (that comes before its wrong value), e counts
    assert run(1) == (REPEATED_SENDER, 4, 3)
    assert run(1, first=4, count=4) == (NOT_MEMBER, 2, 4)
    assert run(1, first=5, count=3) == (NOT_MEMBER, 2, 5)
    # a non-member "first occurrence" never makes a later message a repeat: x twice is NOT_MEMBER twice
    froms[6] = x
    assert run(0, first=4, count=3) == (NOT_MEMBER, 0, 4)
    # a wrong "first occurrence" neither: message 5 (d, value B) then d again with value A counts
    froms[6] = d
    assert run(0, first=5, count=2) == (WRONG_FIELD, 1, 5)
    # not authentic, non-member and wrong at once is not authentic; non-member and wrong is non-member
    verdicts[5], froms[5] = BAD_RS, x
    assert run(0, first=5, count=1) == (BAD_SIGNATURE, 0, 5)
    verdicts[5] = NOT_ADMITTED
    assert run(0, first=5, count=1) == (NOT_MEMBER, 0, 5)


def test_cases_say_what_they_mean():
    """the builders produce the outcomes their names promise (the model decides)"""
    for L in SC.LENGTHS:
        (res,) = SC.lengths_case(L).expected()
        assert res == ((OK if L else SHORT), L, NEVER)
    two = SC.two_sets_case(70, 41)
    assert two.expected() == [(OK, 70, NEVER), (NOT_MEMBER, 69, SC.FIRST + 41)]
    pre = SC.precedence_case(1400)
    ex = pre.expected()
    assert [r[0] for r in ex[:7]] == [BAD_SIGNATURE, BAD_SIGNATURE, BAD_SIGNATURE, NOT_MEMBER, BAD_SIGNATURE,
                                      NOT_MEMBER, WRONG_FIELD]
    k = 7
    for lo in SC.KINDS:
        for hi in SC.KINDS:
            if lo != hi:
                assert ex[k][0] == SC.STATUS_OF.get(lo, WRONG_FIELD) and ex[k][2] == pre.certs[k].first + 10, (lo, hi)
                assert ex[k][1] == 38
                k += 1
    assert [r[0] for r in ex[k:k + 7]] == [SHORT] * 7 and all(r[1] == 9 and r[2] != NEVER for r in ex[k:k + 7])
    k += 7
    assert ex[k] == (NOT_MEMBER, 9, pre.certs[k].first + 4)
    assert ex[k + 1] == (NOT_MEMBER, 58, pre.certs[k + 1].first + 5)
    assert ex[k + 2] == (BAD_SIGNATURE, 59, pre.certs[k + 2].first + 5)        # message 40 counts
    assert ex[k + 3] == (WRONG_FIELD, 59, pre.certs[k + 3].first + 5)
    assert ex[k + 4] == (REPEATED_SENDER, 1299, pre.certs[k + 4].first + 1290) and len(ex) == k + 5
    vb = SC.verdict_bytes_case().expected()
    assert [r[0] for r in vb] == [OK if v in (VALID, NOT_ADMITTED) else BAD_SIGNATURE for v in range(9)]
    edges = SC.index_edges_case()
    assert [r[0] for r in edges.expected()] == [OK, NOT_MEMBER, OK, NOT_MEMBER, NOT_MEMBER, NOT_MEMBER, NOT_MEMBER,
                                                NOT_MEMBER, SHORT, BAD_SIGNATURE, OK, REPEATED_SENDER, OK,
                                                REPEATED_SENDER, OK, NOT_MEMBER]
    # the edges are what they claim: one chain of equal hashes, rows on the last slot, 4n a power of two
    assert len({SC.adm_hash(r) for r in edges.sets[0]}) == 1 and len(set(edges.sets[0])) == 24
    assert sum(SC.adm_hash(r) & 15 == 15 for r in edges.sets[1]) >= 3
    assert len(edges.sets[4]) == 14 and len(set(edges.sets[4])) == 9
    assert 4 * len(edges.sets[5]) == SC.adm_index_slots(len(edges.sets[5])) == 64
    assert sum(SC.adm_hash(r) & 63 == 63 for r in edges.sets[5]) >= 5
    for scratch in (False, True):
        sz = SC.set_sizes_case(THRESHOLD, scratch)
        assert [len(s) for s in sz.sets] == [1, 4, THRESHOLD, THRESHOLD + 1]
        assert max(len(sz.sets[s]) for s in sz.set_of) == THRESHOLD + (1 if scratch else 0)
        for s in set(sz.set_of):   # the lowest and the highest entry of every named set are reached
            rows = sz.ordered(s)
            assert rows[0] in sz.frm and rows[-1] in sz.frm
    assert SC.set_sizes_case(THRESHOLD, True).expected()[:12] == SC.set_sizes_case(THRESHOLD, False).expected()
    alt = SC.alternating_case(300)
    st = [r[0] for r in alt.expected()]
    assert len(st) == 400 and st.count(OK) > 150 and {NOT_MEMBER, WRONG_FIELD, REPEATED_SENDER, BAD_SIGNATURE} <= set(st)


# ---- 2. the set builder -----------------------------------------------------------------
@pytest.mark.parametrize("name", ["chain", "wrap", "empty", "one", "dup", "pow2", "big"])
def test_builder(prog, name):
    edges = SC.index_edges_case()
    rows = dict(chain=edges.sets[0], wrap=edges.sets[1], empty=[], one=edges.sets[3], dup=edges.sets[4],
                pow2=edges.sets[5], big=list(reversed(SC.family(30, 3000))) + SC.family(30, 50))[name]
    near = [r[:31] + bytes([r[31] ^ 1]) for r in rows[:40]] + [bytes([r[0] ^ 0x80]) + r[1:] for r in rows[:40]]
    slots = SC.adm_index_slots(len(set(rows)))
    probes = near + SC.family(31, 40) + SC.rows_hashing_to(slots - 1, slots, 3, 7) + [bytes(32), b"\xff" * 32]
    probes = [p for p in probes if p not in set(rows)]
    got_slots, ordered, found, probed = SC.run_build(prog, rows, probes)
    want = sorted(set(rows))
    assert got_slots == slots and ordered == want            # sorted, unique
    assert found == [want.index(r) for r in rows]             # every entry, duplicates too, at its index
    assert probed == [-1] * len(probes)                       # every constructed non-member


def test_placement_and_limits(prog):
    MAX_ROWS, MAX_SETS = 1 << 27, 1 << 20
    assert SC.run_place(prog, 0, 0, 0, 0, 16) == (0, 0, 15, 0)
    assert SC.run_place(prog, 10, 64, 1, 7, 32) == (80, 64, 31, 7)          # word offset: 8 words a row
    assert SC.run_place(prog, MAX_ROWS - 5, 1 << 30, 3, 5, 32) == (8 * (MAX_ROWS - 5), 1 << 30, 31, 5)
    assert SC.run_place(prog, MAX_ROWS - 5, 1 << 30, 3, 6, 32) is None     # one row too many
    assert SC.run_place(prog, 0, 0, MAX_SETS - 1, 1, 16) is not None
    assert SC.run_place(prog, 0, 0, MAX_SETS, 1, 16) is None               # one set too many
    assert SC.run_place(prog, 0, (1 << 32) - 16, 1, 1, 16) is None         # the slot offsets stay within 32 bits


# ---- 3. the replay ----------------------------------------------------------------------
def _replay_all(prog, case, limits=(GUIDE_LDS, 0), orders=(0, 1, 2)):
    want = case.expected()
    for lim in limits:
        for order in orders:
            got = SC.run_replay(prog, case, lim, order)
            diff = [(k, g, w) for k, (g, w) in enumerate(zip(got, want)) if g != w]
            assert not diff and len(got) == len(want), (lim, order, diff[:5])


@pytest.mark.parametrize("L", SC.LENGTHS)
def test_replay_lengths(prog, L):
    _replay_all(prog, SC.lengths_case(L))


@pytest.mark.parametrize("name", ["two_sets", "precedence", "verdict_bytes", "index_edges"])
def test_replay_small_cases(prog, name):
    _replay_all(prog, SC.small_cases()[name])


@pytest.mark.parametrize("scratch", [False, True])
def test_replay_set_sizes(prog, scratch):
    """the placement follows the largest set the call names: the threshold keeps the table in LDS, one
    entry more moves the whole call to scratch; limit 0 puts either call in scratch"""
    _replay_all(prog, SC.set_sizes_case(THRESHOLD, scratch), orders=(0, 2))


@pytest.mark.parametrize("limit", [GUIDE_LDS, 0])
def test_replay_alternating(prog, limit):
    """4,000 certificates that alternate between two sets: more than either grid cap, so a block meets
    both sets in turn on one table and the restore between them is what keeps the later ones right"""
    _replay_all(prog, SC.alternating_case(), limits=(limit,), orders=(0, 2))


# ---- 4. the binding ---------------------------------------------------------------------
def test_binding():
    from hyperdrive_amd import _lib, quorum, verify
    for name in ("hd_check_certificates_sets", "hd_check_certificates_sets_device", "hd_sigsets_create",
                 "hd_sigsets_destroy", "hd_sigsets_add", "hd_sigsets_clear", "hd_sigsets_info"):
        assert name in _lib.SIGNATURES
    assert (_lib.HD_CERT_NOT_MEMBER, verify.CERT_NOT_MEMBER, verify.CERT_NAMES[5]) == (NOT_MEMBER, NOT_MEMBER, "NOT_MEMBER")
    spec = verify.CertSpec(3, 5, "precommit", 7, -1, A, 5)
    assert spec.set is None and verify.CertSpec(3, 5, "precommit", 7, -1, A, 5, set=2).set == 2
    assert verify.cert_sets([spec, spec], [4, 0], 2).tolist() == [4, 0]
    assert verify.cert_sets([verify.CertSpec(0, 1, 3, 1, 1, A, 1, 6)], None, 1).tolist() == [6]
    assert verify.cert_sets([], None, 0).dtype.itemsize == 4
    for bad in (lambda: verify.cert_sets([spec], None, 1), lambda: verify.cert_sets([spec], [1, 2], 1),
                lambda: verify.cert_sets([spec], [-1], 1), lambda: verify.cert_sets(verify.cert_rows([spec]), None, 1)):
        with pytest.raises(ValueError):
            bad()
    assert callable(quorum.check_certificates_sets) and callable(verify.Verifier.open_sets)
    assert callable(verify.Verifier.check_certificates_sets) and callable(verify.Verifier.check_certificates_sets_device)
    import inspect
    sig = inspect.signature(quorum.check_certificates_wire)
    assert sig.parameters["sets"].default is None and sig.parameters["set_of"].default is None


def test_null_arguments():
    """the entry points refuse NULL arguments before any device work"""
    from hyperdrive_amd import _lib
    lib = _lib.load()
    E = _lib.HD_EINVAL
    out = ctypes.c_void_p()
    sid = ctypes.c_uint32()
    assert lib.hd_sigsets_create(None, ctypes.byref(out)) == E
    assert lib.hd_sigsets_destroy(None) == E and lib.hd_sigsets_clear(None) == E
    assert lib.hd_sigsets_add(None, None, 0, ctypes.byref(sid)) == E
    assert lib.hd_sigsets_info(None, 0, None, None) == E
    assert lib.hd_check_certificates_sets(None, None, None, None, None, 0, None, None) == E
    assert lib.hd_check_certificates_sets_device(None, None, None, None, None, None, 0, None, None) == E
    assert lib.hd_abi_version() == 2
