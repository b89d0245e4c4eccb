"""hd_check_certificates without a GPU: the model of tests/cert_cases.py pinned
on hand-worked segments; the plan function at its edges; and the kernel's
arithmetic (hyperdrive_amd/csrc/hd_certcheck.h) replayed lane by lane under
ASan + UBSan by tests/native/hd_certcheck_check.cpp over the synthetic cases
the GPU test runs, on both table placements and in three lane orders -- the
results must equal the model's whatever the order."""
import ctypes

import pytest

import cert_cases as CC
from cert_cases import BAD_SIGNATURE, NEVER, OK, PRECOMMIT, PREVOTE, REPEATED_SENDER, SHORT, WRONG_FIELD, Cert

GUIDE_LDS = 160 * 1024   # what one CDNA4 workgroup may allocate


@pytest.fixture(scope="module")
def prog():
    return CC.build_check(sanitize=True)


# ---- 1. the model, on hand-worked segments ----------------------------------------------
A, B = CC.value(1), CC.value(2)


def _hand():
    """nine messages: signers 0 1 2 3 1 4 5 6 2; message 3 has a clear bit, message 5 value B,
    message 6 round 9, message 7 signer 7 = n_signers (outside), every other (PRECOMMIT, 5, 2, A)"""
    types = [PRECOMMIT] * 9
    heights = [5] * 9
    rounds = [2, 2, 2, 2, 2, 2, 9, 2, 2]
    values = [A, A, A, A, A, B, A, A, A]
    valid = [1, 1, 1, 0, 1, 1, 1, 1, 1]
    signers = [0, 1, 2, 3, 1, 4, 5, 7, 2]
    return types, heights, rounds, values, valid, signers, 7


def _one(first, count, quorum=1, t=PRECOMMIT, h=5, r=2, v=A):
    (res,) = CC.check([Cert(first, count, quorum, t, h, r, v)], *_hand())
    return res


def test_model_each_status():
    assert _one(0, 3, 3) == (OK, 3, NEVER)
    assert _one(0, 3, 4) == (SHORT, 3, NEVER)
    assert _one(0, 0, 1) == (SHORT, 0, NEVER)                  # the empty segment
    assert _one(2, 2) == (BAD_SIGNATURE, 1, 3)                 # the clear bit
    assert _one(7, 2) == (BAD_SIGNATURE, 1, 7)                 # signer == n_signers on a set bit
    assert _one(4, 2) == (WRONG_FIELD, 1, 5)                   # the value
    assert _one(6, 1) == (WRONG_FIELD, 0, 6)                   # the round
    assert _one(0, 3, t=PREVOTE) == (WRONG_FIELD, 0, 0)        # the type
    assert _one(0, 3, h=2) == (WRONG_FIELD, 0, 0)              # the height (2 is the messages' round)
    assert _one(1, 4) == (BAD_SIGNATURE, 2, 3)
    assert _one(0, 3, v=B) == (WRONG_FIELD, 0, 0)


def test_model_precedence():
    # messages 0..4: 3 is not valid, 4 repeats 1: the lower offender decides
    assert _one(0, 5) == (BAD_SIGNATURE, 3, 3)
    # messages 4..8 with value A: 4 counts (its first occurrence, message 1, is outside), 5 is wrong, 6 wrong,
    # 7 not valid, 8 counts
    assert _one(4, 5) == (WRONG_FIELD, 2, 5)
    # the whole batch: the repeat at 4 and at 8 never decide, 3 does; good = signers 0 1 2
    assert _one(0, 9) == (BAD_SIGNATURE, 3, 3)
    # asked for value B: message 5 is the only clean one; message 0 decides
    assert _one(0, 9, v=B) == (WRONG_FIELD, 1, 0)
    # SHORT wins over every class, good and first_bad are filled all the same
    assert _one(0, 9, quorum=10) == (SHORT, 3, 3)
    # a repeat is the lowest offender: 1 2 | 3 is outside -> messages 1, 2, then 4 repeats 1
    types, heights, rounds, values, valid, signers, ns = _hand()
    valid[3] = 1
    assert CC.check([Cert(0, 5, 1, PRECOMMIT, 5, 2, A)], types, heights, rounds, values, valid, signers, ns) == \
        [(REPEATED_SENDER, 4, 4)]
    # a not-clean "first occurrence" never makes a later message a repeat: message 1 gets value B, so
    # message 4 (same signer) counts and message 1 is the offender
    values[1] = B
    assert CC.check([Cert(0, 5, 1, PRECOMMIT, 5, 2, A)], types, heights, rounds, values, valid, signers, ns) == \
        [(WRONG_FIELD, 4, 1)]
    # not valid and wrong at once is not valid
    valid[1] = 0
    assert CC.check([Cert(0, 5, 1, PRECOMMIT, 5, 2, A)], types, heights, rounds, values, valid, signers, ns) == \
        [(BAD_SIGNATURE, 4, 1)]


def test_model_overlap_and_order():
    cs = [Cert(4, 5, 1, PRECOMMIT, 5, 2, A), Cert(0, 3, 3, PRECOMMIT, 5, 2, A), Cert(0, 3, 3, PRECOMMIT, 5, 2, B)]
    assert CC.check(cs, *_hand()) == [(WRONG_FIELD, 2, 5), (OK, 3, NEVER), (WRONG_FIELD, 0, 0)]


def test_cases_say_what_they_mean():
    """the builders produce the outcomes their names promise (the model decides)"""
    for L in CC.LENGTHS:
        (res,) = CC.lengths_case(L, L + 3).expected()
        assert res == ((OK if L else SHORT), L, NEVER)
    assert [r[0] for r in CC.adjoining_case(200).expected()] == [OK, OK]
    c = CC.overlap_case(200)
    assert c.expected() == [(OK, 40, NEVER), (WRONG_FIELD, 0, CC.FIRST), (OK, 90, NEVER)]
    pos = CC.positions_case(500).expected()
    want = {"notvalid": BAD_SIGNATURE, "repeat": REPEATED_SENDER}
    for k, kind in enumerate(CC.KINDS):
        for q, at in enumerate((0, 129, 63, 64)):
            first = CC.FIRST + 130 * (4 * k + q)
            at = max(at, 1) if kind == "repeat" else at
            assert pos[4 * k + q] == (want.get(kind, WRONG_FIELD), 129, first + at), (kind, at)
    pre = CC.precedence_case(500)
    assert [r[0] for r in pre.expected()] == [
        WRONG_FIELD, BAD_SIGNATURE, REPEATED_SENDER, WRONG_FIELD, BAD_SIGNATURE, REPEATED_SENDER, WRONG_FIELD,
        BAD_SIGNATURE, WRONG_FIELD, REPEATED_SENDER, BAD_SIGNATURE, SHORT]
    far = pre.expected()[5]
    assert far[1] == 399 and far[2] == pre.certs[5].first + 350
    assert pre.expected()[6][1] == 59 and pre.expected()[6][2] == pre.certs[6].first + 5   # message 40 counts
    assert pre.expected()[9][2] == pre.certs[9].first + 77
    assert all(r[0] == BAD_SIGNATURE and r[1] == 65 for r in CC.signer_filter_case(300).expected())
    small = CC.small_table_case().expected()
    assert [r[0] for r in small] == [OK, OK, REPEATED_SENDER, BAD_SIGNATURE, SHORT]
    many = CC.many_small_case(16, 200).expected()
    assert [k for k, r in enumerate(many) if r[0] != OK] == list(range(0, 200, 10))
    big = CC.large_case(100000, 100000)
    assert big.expected() == [(REPEATED_SENDER, 99999, CC.FIRST + 90001)]
    assert CC.large_case(8000, 20000).expected() == [(REPEATED_SENDER, 8000, CC.FIRST + 8000)]


# ---- 2. the plan ------------------------------------------------------------------------
def test_plan_edges(prog):
    base = CC.run_plan(prog, 1, 1, GUIDE_LDS)
    assert base["guide_limit"] == GUIDE_LDS, "the limit is CDNA4's 160 KiB per workgroup"
    thr = base["lds_entries"]
    assert thr == (GUIDE_LDS - base["own"]) // 4 and 4 * thr + base["own"] <= GUIDE_LDS
    cap = max(base["grid_lds"], base["grid_scratch"])
    for ns in (0, 1, thr, thr + 1, 1 << 20):
        for K in (0, 1, 7, cap, cap + 1, 5000, 1 << 20):
            p = CC.run_plan(prog, ns, K, GUIDE_LDS)
            assert p["in_lds"] == (1 if ns <= thr else 0), (ns, K)
            assert (p["blocks"] == 0) == (K == 0) and p["blocks"] <= K
            assert p["scratch_bytes"] == p["blocks"] * p["slice_bytes"]
            if p["in_lds"]:
                assert p["slice_bytes"] == 0 and p["blocks"] == min(K, p["grid_lds"])
                assert 4 * ns <= p["lds_bytes"] <= GUIDE_LDS - p["own"] + 12 and p["lds_bytes"] % 16 == 0
            else:
                assert p["lds_bytes"] == 0 and p["slice_bytes"] == 4 * ns
                assert p["blocks"] <= p["grid_scratch"]
                assert p["scratch_bytes"] <= max(p["scratch_cap"], p["slice_bytes"])   # bounded: the cap, or one slice
    # a device that allows less moves the threshold with it
    small = CC.run_plan(prog, 16000, 3, 64 * 1024)
    assert small["lds_entries"] == (64 * 1024 - base["own"]) // 4 and small["in_lds"] == 1
    assert CC.run_plan(prog, 16384, 3, 64 * 1024)["in_lds"] == 0
    assert CC.run_plan(prog, 5, 3, 0)["in_lds"] == 0


def test_row_checks(prog):
    rows = [(0, 5, 5, 3, 0, 0, 0, 5), (1, 5, 5, 3, 0, 0, 0, 5), (0, 0, 1, 2, 0, 0, 0, 0), (0, 5, 0, 3, 0, 0, 0, 5),
            (0, 5, 5, 1, 0, 0, 0, 5), (0, 5, 5, 4, 0, 0, 0, 5), (0, 5, 5, 0, 0, 0, 0, 5), (0, 5, 5, 3, 1, 0, 0, 5),
            (0, 5, 5, 3, 0, 1, 0, 5), (0, 5, 5, 3, 0, 0, 1, 5), (0xFFFFFFFF, 2, 1, 3, 0, 0, 0, 0xFFFFFFFF),
            (0xFFFFFFFF, 0, 1, 3, 0, 0, 0, 0xFFFFFFFF), (5, 0, 1, 3, 0, 0, 0, 5), (6, 0, 1, 3, 0, 0, 0, 5)]
    assert CC.run_row_ok(prog, rows) == [True, False, True, False, False, False, False, False, False, False, False,
                                         True, True, False]


# ---- 3. the replay ----------------------------------------------------------------------
def _replay_all(prog, case, limits=(GUIDE_LDS,), orders=(0, 1, 2)):
    want = case.expected()
    for lim in limits:
        for order in orders:
            assert CC.run_replay(prog, case, lim, order) == want, (lim, order)


@pytest.mark.parametrize("L", CC.LENGTHS)
def test_replay_lengths(prog, L):
    _replay_all(prog, CC.lengths_case(L, max(L, 1) + 3), limits=(GUIDE_LDS, 0))


@pytest.mark.parametrize("n_signers", [4, "threshold", "threshold+1", 20000])
def test_replay_table_cases(prog, n_signers):
    thr = CC.run_plan(prog, 1, 1, GUIDE_LDS)["lds_entries"]
    ns = {"threshold": thr, "threshold+1": thr + 1}.get(n_signers, n_signers)
    for name, case in CC.table_cases(ns).items():
        assert CC.run_plan(prog, ns, len(case.certs), GUIDE_LDS)["in_lds"] == (1 if ns <= thr else 0)
        _replay_all(prog, case)
    # the same cases at 600 signatories on both placements (limit 0: every table is scratch)
    if n_signers == 4:
        _replay_all(prog, CC.small_table_case(), limits=(GUIDE_LDS, 0))
        for name, case in CC.table_cases(600).items():
            _replay_all(prog, case, limits=(0,))


@pytest.mark.parametrize("limit", [GUIDE_LDS, 0])
def test_replay_many_small(prog, limit):
    """5,000 certificates of 3: more than either grid cap, so blocks take several certificates and the
    restore between them is what keeps the later ones right"""
    case = CC.many_small_case(16)
    assert len(case.certs) > CC.run_plan(prog, 16, len(case.certs), limit)["blocks"]
    _replay_all(prog, case, limits=(limit,), orders=(0, 2))


def test_replay_large(prog):
    _replay_all(prog, CC.large_case(100000), orders=(1, 2))          # scratch: 100,000 signatories
    _replay_all(prog, CC.large_case(8000), orders=(2,))              # LDS: 8,000, the signers go round


# ---- 4. the binding ---------------------------------------------------------------------
def test_binding():
    from hyperdrive_amd import _lib, quorum, verify
    for name in ("hd_check_certificates", "hd_check_certificates_device", "hd_cert_plan_info"):
        assert name in _lib.SIGNATURES
    assert ctypes.sizeof(_lib.HdCert) == 64 and ctypes.sizeof(_lib.HdCertResult) == 16
    assert _lib.HdCert.height.offset == 16 and _lib.HdCert.value32.offset == 32 and _lib.HdCert.type.offset == 12
    rows = verify.cert_rows([verify.CertSpec(3, 5, "precommit", 7, -1, A, 5), verify.CertSpec(0, 0, 2, 1, 2, B, 1)])
    assert (rows[0].first, rows[0].count, rows[0].quorum, rows[0].type, rows[0].height, rows[0].round) == \
        (3, 5, 5, 3, 7, -1)
    assert bytes(rows[0].value32) == A and rows[1].type == 2 and bytes(rows[0].reserved) == bytes(3)
    assert len(rows) == 2 and verify.cert_rows(rows) is rows and len(verify.cert_rows([])) == 0
    with pytest.raises(ValueError):
        verify.cert_rows([verify.CertSpec(0, 1, "propose", 1, 1, A, 1)])
    with pytest.raises(ValueError):
        verify.cert_rows([verify.CertSpec(0, 1, 3, 1, 1, A[:31], 1)])
    assert callable(quorum.check_certificates) and callable(quorum.check_certificates_wire)
    assert (verify.CERT_OK, verify.CERT_SHORT, verify.CERT_BAD_SIGNATURE, verify.CERT_WRONG_FIELD,
            verify.CERT_REPEATED_SENDER) == (OK, SHORT, BAD_SIGNATURE, WRONG_FIELD, REPEATED_SENDER)


def test_plan_info_and_null_arguments():
    """hd_cert_plan_info is the header's plan function (CDNA4's limit, or the visible device's where that is lower), and the entry
    points refuse NULL arguments before any device work"""
    from hyperdrive_amd import _lib, verify
    lib = _lib.load()
    p = verify.Verifier.cert_plan(1000, 5000)
    assert p["in_lds"] == 1 and p["lds_bytes"] == 4000 and p["blocks"] == 2048 and p["scratch_bytes"] == 0
    thr = p["lds_entries"]
    q = verify.Verifier.cert_plan(thr + 1, 5000)
    assert q["in_lds"] == 0 and q["scratch_bytes"] == q["blocks"] * q["slice_bytes"] and q["blocks"] > 0
    assert lib.hd_cert_plan_info(1, 1, None) == _lib.HD_EINVAL
    assert lib.hd_check_certificates(None, None, None, 0, None, None) == _lib.HD_EINVAL
    assert lib.hd_check_certificates_device(None, None, None, None, 0, None, 0, None, None) == _lib.HD_EINVAL
