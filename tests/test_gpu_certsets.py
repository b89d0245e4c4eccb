"""hd_check_certificates_sets[_device] and hd_sigsets (include/hd_cert.h,
include/hd_sigsets.h; Verifier.open_sets, Verifier.check_certificates_sets[_device],
quorum.check_certificates_sets, quorum.check_certificates_wire(..., sets=...))
against the model of tests/certsets_cases.py, row for row.

The synthetic tests call the device form with torch tensors for the columns,
the From rows and synthetic verdict bytes: no signatures.  The messages around
every segment would be clean in it and come from its signers, so a read outside
[first, first + count) changes a count or names a repeat.  The agreement test
translates every tests/cert_cases.py scenario of tests/test_gpu_cert.py (signer
index -> a From of one set, bitmap bit -> verdict VALID / BAD_RS) and compares
with hd_check_certificates_device itself.  The chain test signs with the Python
oracle under two signatory sets, cuts a certificate per set from a DecideLog,
puts both on the wire from the device and checks them in one call on a second
verifier whose own admitted set is one, the other, or neither.
tests/test_certsets_host.py pins the model and replays the kernel's arithmetic
on the host over the same cases."""
import ctypes
import struct

import numpy as np
import pytest

import cert_cases as CC
import certsets_cases as SC
from util import to_np

pytestmark = pytest.mark.gpu

P, V, C = 1, 2, 3


@pytest.fixture(scope="module")
def verifier(gpu):
    v = gpu.Verifier(0)
    yield v
    v.close()


@pytest.fixture(scope="module")
def threshold(gpu):
    """the largest distinct count whose table lives in LDS on this device, from the plan"""
    p = gpu.Verifier.cert_plan(1, 1)
    assert p["in_lds"] == 1 and p["lds_entries"] >= 8000
    return p["lds_entries"]


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def _rows32(rows):
    return np.frombuffer(b"".join(rows), np.uint8).reshape(len(rows), 32).copy() if rows else np.zeros((0, 32), np.uint8)


class Dev:
    """the columns of a case on the device: type, height, round, value, From and verdict bytes"""

    def __init__(self, types, heights, rounds, values, froms, verdicts):
        import torch
        from hyperdrive_amd._lib import HdBatch
        n = len(types)
        self.type = _t(np.array(types, np.uint8))
        self.height = _t(np.array(heights, np.int64))
        self.round = _t(np.array(rounds, np.int64))
        self.value = _t(_rows32(values))
        self.frm = _t(_rows32(froms))
        self.verdict = _t(np.array(verdicts, np.uint8))
        torch.cuda.synchronize()
        self.batch = HdBatch(n, self.type.data_ptr(), self.height.data_ptr(), self.round.data_ptr(), None,
                             self.value.data_ptr(), self.frm.data_ptr(), None)


def specs(certs, set_of=None):
    from hyperdrive_amd.verify import CertSpec
    return [CertSpec(c.first, c.count, c.type, c.height, c.round, c.value, c.quorum,
                     None if set_of is None else set_of[k]) for k, c in enumerate(certs)]


def rows(res):
    return list(zip(res.status.tolist(), res.good.tolist(), res.first_bad.tolist()))


def open_sets(v, case):
    ss = v.open_sets()
    for k, s in enumerate(case.sets):
        assert ss.add(s) == k
        assert ss.info(k) == (len(s), len(set(s)))
    return ss


def run(v, case, ss=None, dev=None, by_spec=False):
    """the case through check_certificates_sets_device; the result equals the model exactly"""
    own = ss is None
    ss = ss or open_sets(v, case)
    try:
        d = dev or Dev(case.type, case.height, case.round, case.value, case.frm, case.verdict)
        if by_spec:   # the set in every CertSpec
            res = v.check_certificates_sets_device(d.batch, d.verdict.data_ptr(), specs(case.certs, case.set_of), ss)
        else:
            res = v.check_certificates_sets_device(d.batch, d.verdict.data_ptr(), specs(case.certs), ss, case.set_of)
        got, want = rows(res), case.expected()
        assert len(got) == len(want)
        diff = [(k, g, w) for k, (g, w) in enumerate(zip(got, want)) if g != w]
        assert not diff, diff[:5]
        return d
    finally:
        if own:
            ss.close()


def named_max(case):
    return max(len(set(case.sets[s])) for s in case.set_of)


# ---- parity with the model --------------------------------------------------------------
@pytest.mark.parametrize("L", SC.LENGTHS)
def test_segment_lengths(verifier, L):
    run(verifier, SC.lengths_case(L))


@pytest.mark.parametrize("name", ["two_sets", "precedence", "verdict_bytes", "index_edges"])
def test_small_cases(verifier, name):
    run(verifier, SC.small_cases()[name], by_spec=name == "two_sets")


@pytest.mark.parametrize("placement", ["lds", "scratch"])
def test_set_sizes_in_one_call(gpu, verifier, threshold, placement):
    """sets of 1, 4, threshold and threshold + 1 entries in one object: a call that names the first three
    keeps the table in LDS, one that names all four moves it to scratch; same expectations"""
    case = SC.set_sizes_case(threshold, placement == "scratch")
    assert gpu.Verifier.cert_plan(named_max(case), len(case.certs))["in_lds"] == (placement == "lds")
    run(verifier, case)


def test_alternating_sets(gpu, verifier):
    """4,000 small certificates alternating between two sets: more than the grid, both sets on one table"""
    case = SC.alternating_case()
    assert gpu.Verifier.cert_plan(named_max(case), len(case.certs))["blocks"] < len(case.certs)
    run(verifier, case)


# ---- agreement with hd_check_certificates_device ------------------------------------------
FAMILY = 50   # signer index j of a cert_cases scenario -> sig(FAMILY, j)


def _agree(v, case):
    """the scenario through the existing check (its bitmap and signer) and, translated, through the
    sets form: the same good and first_bad, the same status once NOT_MEMBER reads BAD_SIGNATURE"""
    from hyperdrive_amd.verify import CertSpec
    ns, n = case.n_signers, case.n
    froms = [SC.sig(FAMILY, s) if 0 <= s < ns else SC.sig(SC.OUTSIDER, i) for i, s in enumerate(case.signer)]
    verdicts = [SC.VALID if ok else SC.BAD_RS for ok in case.valid]
    d = Dev(case.type, case.height, case.round, case.value, froms, verdicts)
    bits = np.zeros((n + 31) // 32 * 32, np.uint8)
    bits[:n] = case.valid
    bitmap = _t(np.packbits(bits, bitorder="little").view(np.uint32).view(np.int32).copy())
    signer = _t(np.array(case.signer, np.int32))
    import torch
    torch.cuda.synchronize()
    certs = [CertSpec(c.first, c.count, c.type, c.height, c.round, c.value, c.quorum) for c in case.certs]
    ref = rows(v.check_certificates_device(d.batch, bitmap.data_ptr(), signer.data_ptr(), ns, certs))
    assert ref == case.expected()
    with v.open_sets() as ss:
        sid = ss.add(SC.family(FAMILY, ns))
        got = rows(v.check_certificates_sets_device(d.batch, d.verdict.data_ptr(), certs, ss, [sid] * len(certs)))
    got = [(CC.BAD_SIGNATURE if st == SC.NOT_MEMBER else st, good, bad) for st, good, bad in got]
    diff = [(k, g, w) for k, (g, w) in enumerate(zip(got, ref)) if g != w]
    assert not diff and len(got) == len(ref), diff[:5]


def test_agrees_on_lengths_and_small_table(verifier):
    for L in CC.LENGTHS:
        _agree(verifier, CC.lengths_case(L, max(L, 1) + 3))
    _agree(verifier, CC.small_table_case())


@pytest.mark.parametrize("n_signers", [4, 300, "threshold", "threshold+1", 20000])
def test_agrees_on_table_cases(verifier, threshold, n_signers):
    ns = {"threshold": threshold, "threshold+1": threshold + 1}.get(n_signers, n_signers)
    for name, case in CC.table_cases(ns).items():
        _agree(verifier, case)


@pytest.mark.parametrize("placement", ["lds", "scratch"])
def test_agrees_on_many_small(verifier, threshold, placement):
    _agree(verifier, CC.many_small_case(16 if placement == "lds" else threshold + 1))


@pytest.mark.parametrize("n_signers", [100000, 8000])
def test_agrees_on_one_large_certificate(verifier, n_signers):
    _agree(verifier, CC.large_case(n_signers))


# ---- reuse ------------------------------------------------------------------------------
def test_reuse(gpu, threshold):
    """a scratch-placement call, an add, the same call again: identical.  A table left dirty by the
    first call shows up as a repeat in the second, and the ids given before the add still name their sets"""
    v = gpu.Verifier(0)
    try:
        case = SC.set_sizes_case(threshold, True)
        ss = open_sets(v, case)
        d = run(v, case, ss)
        extra = SC.family(40, 33) + case.sets[2][:5]
        assert ss.add(extra) == 4 and ss.info(4) == (38, 38)
        run(v, case, ss, d)
        # the new set works beside the old ones, on the LDS placement of the same context
        small = SC.SCase(case.sets + [extra])
        small.pad(4, CC.FIRST)
        small.seg(4, 38)
        first = small.seg(1, 4)
        small.cert(first, 4, 4)
        run(v, small, ss)
        run(v, case, ss, d)
        ss.clear()
        assert ss.add(case.sets[1]) == 0 and ss.info(0) == (4, 4)   # ids count up from 0 again
        with pytest.raises(gpu.verify.HDError):
            ss.info(1)
        ss.close()
    finally:
        v.close()


# ---- errors -----------------------------------------------------------------------------
def test_errors(gpu, verifier):
    """each HD_EINVAL comes back with `results` untouched; K = 0 is HD_OK"""
    import torch
    from hyperdrive_amd import _lib
    from hyperdrive_amd.verify import cert_rows
    lib = _lib.load()
    case = SC.lengths_case(65)
    d = Dev(case.type, case.height, case.round, case.value, case.frm, case.verdict)
    n = case.n
    ss = open_sets(verifier, case)
    other = gpu.Verifier(0)
    foreign = open_sets(other, case)
    one = specs(case.certs)
    EINVAL = _lib.HD_EINVAL
    untouched = b"\xAB" * 64

    def call(rows_, ids, k, batch=None, sets=ss, verdict=True, results=True, ctx=True):
        res = (_lib.HdCertResult * 4)()
        ctypes.memset(res, 0xAB, ctypes.sizeof(res))
        b = batch if batch is not None else d.batch
        set_of = None if ids is None else (ctypes.c_uint32 * max(len(ids), 1))(*ids)
        rc = lib.hd_check_certificates_sets_device(verifier.handle if ctx else None, sets.handle if sets else None,
                                                   ctypes.byref(b), d.verdict.data_ptr() if verdict else None, rows_,
                                                   set_of, k, res if results else None, None)
        return rc, bytes(res)

    try:
        good = cert_rows(one)
        rc, raw = call(good, [0], 1)
        assert rc == 0 and raw[:16] != untouched[:16] and raw[16:] == untouched[16:]   # one row written, no more
        assert np.frombuffer(raw[:12], np.uint32).tolist() == [SC.OK, 65, SC.NEVER]
        assert call(good, [0], 0) == (0, untouched)
        assert call(None, None, 0) == (0, untouched)
        assert call(None, [0], 1) == (EINVAL, untouched)
        assert call(good, None, 1) == (EINVAL, untouched)
        assert call(good, [0], 1, results=False)[0] == EINVAL
        assert call(good, [0], 1, ctx=False) == (EINVAL, untouched)
        assert call(good, [0], 1, sets=None) == (EINVAL, untouched)
        assert call(good, [0], 1, verdict=False) == (EINVAL, untouched)
        # a set id the object does not hold; the sets of another context (also with K = 0 there is nothing to do)
        two = cert_rows(one + one)
        assert call(two, [0, 1], 2) == (EINVAL, untouched)
        assert call(two, [0, 0xFFFFFFFF], 2) == (EINVAL, untouched)
        assert call(good, [0], 1, sets=foreign) == (EINVAL, untouched)
        # a NULL From column; a From or a value column that is not 16-byte aligned
        H = _lib.HdBatch
        cols = (d.type.data_ptr(), d.height.data_ptr(), d.round.data_ptr(), None, d.value.data_ptr(), d.frm.data_ptr(), None)
        assert call(good, [0], 1, batch=H(n, *cols[:5], None, None)) == (EINVAL, untouched)
        pad = torch.zeros(32 * n + 32, dtype=torch.uint8, device="cuda")
        pad[8:8 + 32 * n] = d.frm.reshape(-1)
        torch.cuda.synchronize()
        assert pad.data_ptr() % 16 == 0
        assert call(good, [0], 1, batch=H(n, *cols[:5], pad.data_ptr() + 8, None)) == (EINVAL, untouched)
        assert call(good, [0], 1, batch=H(n, *cols[:4], pad.data_ptr() + 4, cols[5], None)) == (EINVAL, untouched)

        def bad(**change):
            r = cert_rows(one + one)   # two rows: the second one is the bad one
            for name, val in change.items():
                if name == "reserved":
                    r[1].reserved[val] = 1
                else:
                    setattr(r[1], name, val)
            assert call(r, [0, 0], 2) == (EINVAL, untouched), change

        bad(count=n - CC.FIRST + 1)            # first + count = n + 1
        bad(first=n, count=1)
        bad(first=0xFFFFFFFF, count=2)         # first + count wraps in 32 bits
        bad(quorum=0)
        for t in (0, 1, 4, 255):
            bad(type=t)
        for k in range(3):
            bad(reserved=k)
        # the Python face: an empty list of certificates; a CertSpec without a set and no set_of
        out = verifier.check_certificates_sets_device(d.batch, d.verdict.data_ptr(), [], ss)
        assert len(out) == 0 and out.ok == []
        with pytest.raises(ValueError):
            verifier.check_certificates_sets_device(d.batch, d.verdict.data_ptr(), one, ss)
        # add: NULL rows with n > 0, a NULL id; info: an unknown id
        sid = ctypes.c_uint32(7)
        assert lib.hd_sigsets_add(ss.handle, None, 3, ctypes.byref(sid)) == EINVAL and sid.value == 7
        assert lib.hd_sigsets_add(ss.handle, None, 0, None) == EINVAL
        assert lib.hd_sigsets_info(ss.handle, 1, None, None) == EINVAL
        assert lib.hd_sigsets_info(ss.handle, 0, None, None) == 0
    finally:
        foreign.close()
        other.close()
        ss.close()


def test_lifetime(gpu):
    """sets destroyed after their context, and before it; each after a check that used them"""
    case = SC.two_sets_case()
    for sets_first in (True, False):
        v = gpu.Verifier(0)
        ss = open_sets(v, case)
        run(v, case, ss)
        if sets_first:
            ss.close()
            v.close()
        else:
            v.close()
            ss.close()


# ---- the chain ----------------------------------------------------------------------------
RND, H0 = 3, 11
EPOCHS = [dict(who=list(range(0, 7)), f=2), dict(who=list(range(3, 13)), f=3)]   # 7 and 10 signatories
DISJOINT = list(range(40, 47))


def _wire(b):
    """the surge records of a batch of votes with signatures (include/hd_codec.h), in Python"""
    return b"".join(struct.pack(">qq", int(b.height[i]), int(b.round[i])) + b.value[i].tobytes() + b.frm[i].tobytes()
                    + b.sig[i].tobytes() for i in range(len(b)))


def _join(parts):
    from hyperdrive_amd.verify import Batch
    cat = lambda f: np.concatenate([getattr(p, f) for p in parts])
    return Batch(cat("type"), cat("height"), cat("round"), cat("valid_round"), cat("value"), cat("frm"), cat("sig"))


@pytest.fixture(scope="module")
def chain(gpu, oracle):
    """the sender: one height per epoch, each under its own signatory set, fed to a DecideLog until commit
    fires; the certificate behind the firing selected on the device and marshalled there"""
    from hyperdrive_amd import codec
    O = oracle
    keys = O.KeyCache()
    a = gpu.Verifier(0)
    a.set_variant("key_width", 13)
    parts, wires, values, sets = [], [], [], []

    def signed(t, h, r, value, who, vr=-1):
        return (t, h, r, vr, value, keys.signatory(who), O.sign(keys.sk(who), O.message_digest(t, h, r, vr, value)))

    try:
        for e, ep in enumerate(EPOCHS):
            who, f = ep["who"], ep["f"]
            S, Q, h = len(who), 2 * ep["f"] + 1, H0 + e
            sigs = [keys.signatory(w) for w in who]
            sets.append(sigs)
            a.set_signatories(_rows32(sigs))
            v = O.canonical_value(h, 0)
            values.append(v)
            ob = O.Batch()
            for m in [signed(P, h, RND, v, who[0])] + [signed(V, h, RND, v, who[k]) for k in range(Q)] + \
                    [signed(C, h, RND, v, who[(k + h) % S]) for k in range(Q + 1)]:
                ob.append(*m)
            nb = to_np(ob)
            vd = a.verify_batch(nb).verdict
            assert vd.tolist() == [O.VALID] * len(ob)
            log = a.open_log(h, f, None, keep_signatures=True)
            try:
                res = log.insert(nb, vd)
                (i, hh, rr, _), = [x for x in res.new_firings if x[3] == "commit"]
                assert (hh, rr) == (h, RND) and i == 1 + Q + Q - 1          # the 2f+1-th precommit
                fired = int(res.logpos[i])
                cert = log.certificate("precommit", RND, v, upto=fired)
                assert len(cert) == Q
                sel = log.select_device(C, RND, value=v, upto=fired, limit=Q)
                assert sel.n == Q
                raw = codec.marshal_device(a, C, sel.batch, with_sig=True).cpu().numpy().tobytes()
                assert raw == _wire(cert.batch)                             # the device's bytes are the codec's
                parts.append(cert.batch)
                wires.append(raw)
            finally:
                log.close()
    finally:
        a.close()
    return dict(O=O, keys=keys, sets=sets, parts=parts, wires=wires, values=values)


def test_chain(gpu, chain):
    """sender -> wire -> receiver: both certificates, each under its own set and under the other's, in
    one check_certificates_wire(..., sets=...) call -- with the receiver's admitted set equal to epoch
    0's, to epoch 1's and disjoint from both.  The three runs agree with the model and so with each
    other, and none of them touches the admitted set."""
    from hyperdrive_amd import quorum
    from hyperdrive_amd.verify import CertSpec
    O, keys, parts = chain["O"], chain["keys"], chain["parts"]
    Q = [2 * ep["f"] + 1 for ep in EPOCHS]
    batch = _join(parts)
    firsts = [0, len(parts[0])]
    # (certificate, set): each under its own set, then under the other's with that set's quorum
    pairs = [(0, 0), (1, 1), (0, 1), (1, 0)]
    certs = [CertSpec(firsts[c], len(parts[c]), "precommit", H0 + c, RND, chain["values"][c], Q[s], s) for c, s in pairs]
    wire = b"".join(chain["wires"])
    assert wire == _wire(batch)

    def model(b_):
        froms = [b_.frm[i].tobytes() for i in range(len(b_))]
        return SC.check_sets([CC.Cert(c.first, c.count, c.quorum, C, c.height, c.round, c.value) for c in certs],
                             [s for _, s in pairs], chain["sets"], b_.type.tolist(), b_.height.tolist(),
                             b_.round.tolist(), [b_.value[i].tobytes() for i in range(len(b_))], froms,
                             [SC.VALID] * len(b_))   # every signature is its From's

    want = model(batch)
    # epoch 1's signers (k + 12) % 10 = 2 .. 8 of who 3 .. 12 are who 5 .. 11: who 7 at index 2 is the
    # first outside epoch 0's set; epoch 0's five messages are fewer than epoch 1's quorum of seven
    assert want[0] == (SC.OK, Q[0], SC.NEVER) and want[1] == (SC.OK, Q[1], SC.NEVER)
    assert want[2][0] == SC.SHORT and want[3] == (SC.NOT_MEMBER, 2, firsts[1] + 2)
    tampered = _join(parts)
    tampered.sig[2, 40] ^= 1
    want_tampered = list(want)
    want_tampered[0] = (SC.BAD_SIGNATURE, Q[0] - 1, 2)
    want_tampered[2] = (SC.SHORT, want[2][1] - 1, 2)   # message 2 (who 6) is in both sets: it counted in both

    b = gpu.Verifier(0)
    try:
        b.set_variant("key_width", 13)
        ss = b.open_sets()
        assert [ss.add(s) for s in chain["sets"]] == [0, 1]
        seen = []
        for admitted in (EPOCHS[0]["who"], EPOCHS[1]["who"], DISJOINT):
            b.set_signatories(_rows32([keys.signatory(w) for w in admitted]))
            b.verify_batch(batch)      # the admitted signers' keys are learned here, before the count is taken
            before = (b.last_set_change(), b.known_keys())
            for _ in range(2):         # the second pass runs on whatever keys the first one left
                res = quorum.check_certificates_wire(b, "precommit", wire, certs, sets=ss)
                assert rows(res) == want and res.ok == [True, True, False, False]
                host = b.check_certificates_sets(batch, certs, ss, verdict=True)
                assert rows(host) == want and set(host.verdict.tolist()) <= {SC.VALID, SC.NOT_ADMITTED}
                assert quorum.check_certificates_sets(b, batch, certs, ss) == [True, True, False, False]
            bad = quorum.check_certificates_wire(b, "precommit", _wire(tampered), certs, sets=ss)
            assert rows(bad) == want_tampered
            host = b.check_certificates_sets(tampered, certs, ss, verdict=True)
            assert rows(host) == want_tampered and host.verdict[2] not in (SC.VALID, SC.NOT_ADMITTED)
            assert (b.last_set_change(), b.known_keys()) == before          # the admitted set is untouched
            assert b.n_signatories == len(admitted)
            seen.append(rows(res))
        assert seen[0] == seen[1] == seen[2]
        # without sets the wire form is what it was: everything under the admitted (disjoint) set
        plain = quorum.check_certificates_wire(b, "precommit", wire, certs[:2])
        assert [r[0] for r in rows(plain)] == [CC.BAD_SIGNATURE, CC.BAD_SIGNATURE]
        ss.close()
    finally:
        b.close()
