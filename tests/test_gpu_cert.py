"""hd_check_certificates and hd_check_certificates_device (include/hd_cert.h;
Verifier.check_certificates[_device], quorum.check_certificates[_wire]) against
the model of tests/cert_cases.py, row for row.

The synthetic tests call the device form with torch tensors for the columns,
the bitmap and the signer indices: no signatures and no signatory set.  The
messages around every segment would be clean in it and come from its signers,
so a read outside [first, first + count) changes a count or names a repeat.
The chain tests sign with the Python oracle, cut certificates from a DecideLog,
put them on the wire from the device and check them on a second verifier.
tests/test_cert_host.py pins the model and replays the kernel's arithmetic on
the host over the same cases.

"One large certificate" is run in two forms, since 100,000 messages cannot come
from 8,000 signatories with only one of them repeating: 100,000 messages from
100,000 signatories of which exactly one repeats (the scratch placement), and
100,000 messages over 8,000 signatories going round (the LDS placement: good
is 8,000 and message 8,000 is the first repeat)."""
import ctypes
import struct

import numpy as np
import pytest

import cert_cases as CC
from util import from_np, to_np

pytestmark = pytest.mark.gpu

P, V, C = 1, 2, 3


@pytest.fixture(scope="module")
def verifier(gpu):
    v = gpu.Verifier(0)
    yield v
    v.close()


@pytest.fixture(scope="module")
def threshold(gpu):
    """the largest n_signers whose table lives in LDS on this device, from the plan"""
    p = gpu.Verifier.cert_plan(1, 1)
    assert p["in_lds"] == 1 and p["lds_entries"] >= 8000
    assert gpu.Verifier.cert_plan(p["lds_entries"], 3)["in_lds"] == 1
    assert gpu.Verifier.cert_plan(p["lds_entries"] + 1, 3)["in_lds"] == 0
    return p["lds_entries"]


class Dev:
    """a Case on the device: the columns, the bitmap and the signer indices as torch tensors"""

    def __init__(self, case):
        import torch
        from hyperdrive_amd._lib import HdBatch
        n = case.n
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda")
        self.type = t(np.array(case.type, np.uint8))
        self.height = t(np.array(case.height, np.int64))
        self.round = t(np.array(case.round, np.int64))
        self.value = t(np.frombuffer(b"".join(case.value), np.uint8).reshape(n, 32).copy())
        bits = np.zeros((n + 31) // 32 * 32, np.uint8)
        bits[:n] = case.valid
        self.bitmap = t(np.packbits(bits, bitorder="little").view(np.uint32).view(np.int32).copy())
        self.signer = t(np.array(case.signer, np.int32))
        torch.cuda.synchronize()
        self.batch = HdBatch(n, self.type.data_ptr(), self.height.data_ptr(), self.round.data_ptr(), None,
                             self.value.data_ptr(), None, None)
        self.specs = specs(case)
        self.n_signers = case.n_signers


def specs(case):
    from hyperdrive_amd.verify import CertSpec
    return [CertSpec(c.first, c.count, c.type, c.height, c.round, c.value, c.quorum) for c in case.certs]


def rows(res):
    return list(zip(res.status.tolist(), res.good.tolist(), res.first_bad.tolist()))


def run(v, case, dev=None, prebuilt=False):
    from hyperdrive_amd.verify import cert_rows
    d = dev or Dev(case)
    certs = cert_rows(d.specs) if prebuilt else d.specs      # the rows built once, or the list of CertSpec
    res = v.check_certificates_device(d.batch, d.bitmap.data_ptr(), d.signer.data_ptr(), d.n_signers, certs)
    got, want = rows(res), case.expected()
    assert len(got) == len(want)
    diff = [(k, g, w) for k, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not diff, diff[:5]
    return d


# ---- the synthetic cases ------------------------------------------------------------------
@pytest.mark.parametrize("L", CC.LENGTHS)
def test_segment_lengths(verifier, L):
    run(verifier, CC.lengths_case(L, max(L, 1) + 3))


def test_small_table(verifier):
    run(verifier, CC.small_table_case())


@pytest.mark.parametrize("n_signers", [4, "threshold", "threshold+1", 20000])
def test_table_placements(gpu, verifier, threshold, n_signers):
    """adjoining and overlapping segments, every class at the first, the last and indices 63 and 64, the
    precedence rules and the signer filter, with the table in LDS (4, the threshold) and in the
    context's scratch (the threshold + 1); the signers reach entry n_signers - 1.  Where 20,000 falls
    is the plan's to say: in LDS on a device whose workgroups may allocate CDNA4's 160 KiB (threshold
    40,896), in scratch where the device reports 64 KiB; test_one_large_certificate[100000] is on the
    scratch placement either way"""
    ns = {"threshold": threshold, "threshold+1": threshold + 1}.get(n_signers, n_signers)
    for name, case in CC.table_cases(ns).items():
        assert gpu.Verifier.cert_plan(ns, len(case.certs))["in_lds"] == (1 if ns <= threshold else 0)
        run(verifier, case)


@pytest.mark.parametrize("placement", ["lds", "scratch"])
def test_many_small_certificates(gpu, verifier, threshold, placement):
    """5,000 certificates of 3 messages, every tenth with one offender: more certificates than blocks"""
    ns = 16 if placement == "lds" else threshold + 1
    case = CC.many_small_case(ns)
    plan = gpu.Verifier.cert_plan(ns, len(case.certs))
    assert plan["in_lds"] == (placement == "lds") and plan["blocks"] < len(case.certs)
    run(verifier, case)


def test_reuse(gpu, threshold):
    """the same case twice, then another, on one context and on both placements: a table left dirty by
    a call shows up as a repeat in the next"""
    v = gpu.Verifier(0)
    try:
        for ns in (300, threshold + 1):
            a, b = CC.precedence_case(ns), CC.positions_case(ns)
            da = run(v, a)
            run(v, a, da, prebuilt=True)
            run(v, b)
            run(v, a, da)
    finally:
        v.close()


@pytest.mark.parametrize("n_signers", [100000, 8000])
def test_one_large_certificate(gpu, verifier, threshold, n_signers):
    case = CC.large_case(n_signers)
    assert gpu.Verifier.cert_plan(n_signers, 1)["in_lds"] == (1 if n_signers <= threshold else 0)
    (want,) = case.expected()
    assert want[0] == CC.REPEATED_SENDER and want[1] == (99999 if n_signers == 100000 else 8000)
    run(verifier, case)


def test_errors(verifier):
    """each HD_EINVAL comes back with `results` untouched; K = 0 is HD_OK"""
    from hyperdrive_amd import _lib
    from hyperdrive_amd.verify import cert_rows
    lib = _lib.load()
    case = CC.lengths_case(65, 80)
    d = Dev(case)
    n = case.n

    def call(rows_, k, batch=None, bitmap=True, signer=True, results=True, ctx=True):
        res = (_lib.HdCertResult * 4)()
        ctypes.memset(res, 0xAB, ctypes.sizeof(res))
        b = batch if batch is not None else d.batch
        rc = lib.hd_check_certificates_device(verifier.handle if ctx else None, ctypes.byref(b),
                                              d.bitmap.data_ptr() if bitmap else None,
                                              d.signer.data_ptr() if signer else None, d.n_signers, rows_, k,
                                              res if results else None, None)
        return rc, bytes(res)

    untouched = b"\xAB" * 64
    good = cert_rows(d.specs)
    rc, raw = call(good, 1)
    assert rc == 0 and raw[:16] != untouched[:16] and raw[16:] == untouched[16:]   # one row written, no more
    assert call(good, 0) == (0, untouched)
    assert call(None, 0) == (0, untouched)
    EINVAL = _lib.HD_EINVAL
    assert call(None, 1) == (EINVAL, untouched)
    assert call(good, 1, results=False)[0] == EINVAL
    assert call(good, 1, ctx=False) == (EINVAL, untouched)
    assert call(good, 1, bitmap=False) == (EINVAL, untouched)
    assert call(good, 1, signer=False) == (EINVAL, untouched)
    nb = _lib.HdBatch(n, None, d.height.data_ptr(), d.round.data_ptr(), None, d.value.data_ptr(), None, None)
    assert call(good, 1, batch=nb) == (EINVAL, untouched)

    def bad(**change):
        r = cert_rows(d.specs + d.specs)   # two rows: the second one is the bad one
        for name, val in change.items():
            if name == "reserved":
                r[1].reserved[val] = 1
            else:
                setattr(r[1], name, val)
        assert call(r, 2) == (EINVAL, untouched), change

    bad(count=n - CC.FIRST + 1)            # first + count = n + 1
    bad(first=n, count=1)
    bad(first=0xFFFFFFFF, count=2)         # first + count wraps in 32 bits
    bad(quorum=0)
    for t in (0, 1, 4, 255):
        bad(type=t)
    for k in range(3):
        bad(reserved=k)
    r = cert_rows(d.specs + d.specs)
    r[1].first, r[1].count = n, 0          # the empty segment at the very end is allowed
    rc, raw = call(r, 2)
    res = np.frombuffer(raw, np.uint32).reshape(4, 4)
    assert rc == 0 and res[1].tolist()[:3] == [CC.SHORT, 0, CC.NEVER] and res[0].tolist()[:3] == [CC.OK, 65, CC.NEVER]
    # the Python face: an empty list of certificates
    out = verifier.check_certificates_device(d.batch, d.bitmap.data_ptr(), d.signer.data_ptr(), d.n_signers, [])
    assert len(out) == 0 and out.ok == []


# ---- the chain ----------------------------------------------------------------------------
S, F, RND, H0 = 7, 2, 3, 11
Q = 2 * F + 1


def _wire(b):
    """the surge records of a batch of votes with signatures (include/hd_codec.h), in Python"""
    return b"".join(struct.pack(">qq", int(b.height[i]), int(b.round[i])) + b.value[i].tobytes() + b.frm[i].tobytes()
                    + b.sig[i].tobytes() for i in range(len(b)))


def _take(b, ix):
    from hyperdrive_amd.verify import Batch
    ix = list(ix)
    return Batch(b.type[ix], b.height[ix], b.round[ix], b.valid_round[ix], b.value[ix], b.frm[ix], b.sig[ix])


def _join(parts):
    from hyperdrive_amd.verify import Batch
    cat = lambda f: np.concatenate([getattr(p, f) for p in parts])
    return Batch(cat("type"), cat("height"), cat("round"), cat("valid_round"), cat("value"), cat("frm"), cat("sig"))


@pytest.fixture(scope="module")
def chain(gpu, oracle):
    """the sender: three heights fed to a DecideLog until commit fires, the certificate behind each firing
    selected on the device and marshalled there; (host batches per height, the wire bytes, the values)"""
    from hyperdrive_amd import codec
    O = oracle
    keys = O.KeyCache()
    sigs = O.admitted_set(S, keys)
    a = gpu.Verifier(0)
    a.set_variant("key_width", 13)
    a.set_signatories(np.frombuffer(b"".join(sigs), np.uint8).reshape(S, 32).copy())
    parts, wires, values = [], [], []

    def signed(t, h, r, value, who, vr=-1):
        return (t, h, r, vr, value, keys.signatory(who), O.sign(keys.sk(who), O.message_digest(t, h, r, vr, value)))

    try:
        for h in range(H0, H0 + 3):
            v = O.canonical_value(h, 0)
            values.append(v)
            ob = O.Batch()
            for m in [signed(P, h, RND, v, 0)] + [signed(V, h, RND, v, k) for k in range(Q)] + \
                    [signed(C, h, RND, v, (k + h) % S) for k in range(Q + 1)]:
                ob.append(*m)
            nb = to_np(ob)
            vd = a.verify_batch(nb).verdict
            assert vd.tolist() == [O.VALID] * len(ob)
            log = a.open_log(h, F, None, keep_signatures=True)
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
    return dict(O=O, keys=keys, sigs=sigs, parts=parts, wires=wires, values=values, signed=signed)


def _scenarios(ch):
    """name -> the three certificates' batches, the middle one tampered with"""
    O, keys, signed = ch["O"], ch["keys"], ch["signed"]
    h, v = H0 + 1, ch["values"][1]
    mid = ch["parts"][1]

    def with_row(k, msg):
        ob = from_np(mid)
        for name, x in zip(("mtype", "height", "round", "valid_round", "value", "frm", "sig"), msg):
            getattr(ob, name)[k] = x
        return to_np(ob)

    flipped = _take(mid, range(Q))
    flipped.sig[2, 40] ^= 1
    out = {
        "untouched": mid,
        "signature_byte": flipped,
        "not_admitted": with_row(1, signed(C, h, RND, v, S + 3)),
        "neighbour_copy": _take(mid, [0, 1, 2, 2, 4]),
        "other_round": with_row(3, signed(C, h, RND + 1, v, (3 + h) % S)),
        "dropped": _take(mid, [0, 1, 2, 4]),
    }
    return {name: [ch["parts"][0], m, ch["parts"][2]] for name, m in out.items()}


WANT_MID = {"untouched": (CC.OK, Q, None), "signature_byte": (CC.BAD_SIGNATURE, Q - 1, 2),
            "not_admitted": (CC.BAD_SIGNATURE, Q - 1, 1), "neighbour_copy": (CC.REPEATED_SENDER, Q - 1, 3),
            "other_round": (CC.WRONG_FIELD, Q - 1, 3), "dropped": (CC.SHORT, Q - 1, None)}


def test_chain(gpu, chain):
    """sender -> wire -> receiver: three certificates in one call, on the wire form and on the host form,
    twice each (the first pass of a fresh receiver is the full recovery, later ones the known-key check),
    against the model fed with the oracle's verdicts and against quorum.check_certificate per certificate"""
    from hyperdrive_amd import quorum
    from hyperdrive_amd.verify import CertSpec
    O, sigs = chain["O"], chain["sigs"]
    index = {s: k for k, s in enumerate(sigs)}
    b = gpu.Verifier(0)
    try:
        b.set_variant("key_width", 13)
        b.set_signatories(np.frombuffer(b"".join(sigs), np.uint8).reshape(S, 32).copy())
        for name, parts in _scenarios(chain).items():
            batch = _join(parts)
            firsts = np.cumsum([0] + [len(p) for p in parts])
            certs = [CertSpec(int(firsts[k]), len(parts[k]), "precommit", H0 + k, RND, chain["values"][k], Q)
                     for k in range(3)]
            ob = from_np(batch)
            verdicts, _ = O.verify_batch(ob, sigs)
            model = CC.check([CC.Cert(c.first, c.count, c.quorum, C, c.height, c.round, c.value) for c in certs],
                             ob.mtype, ob.height, ob.round, ob.value, [x == O.VALID for x in verdicts],
                             [index.get(f, -1) for f in ob.frm], S)
            st, good, at = WANT_MID[name]
            assert model == [(CC.OK, Q, CC.NEVER), (st, good, CC.NEVER if at is None else int(firsts[1]) + at),
                             (CC.OK, Q, CC.NEVER)], name
            strict = [quorum.check_certificate(b, parts[k], H0 + k, RND, "precommit", chain["values"][k], F)
                      for k in range(3)]
            assert strict == [True, name == "untouched", True], name
            wire = _wire(batch)
            if name == "untouched":
                assert wire == b"".join(chain["wires"])
            for _ in range(2):
                res = quorum.check_certificates_wire(b, "precommit", wire, certs)
                assert rows(res) == model and res.ok == strict, (name, rows(res))
                host = b.check_certificates(batch, certs, verdict=True)
                assert rows(host) == model and host.verdict.tolist() == verdicts, (name, rows(host))
                assert quorum.check_certificates(b, batch, certs) == strict
            if name == "untouched":
                assert b.known_keys() > 0   # from here on the known-key check feeds the check
    finally:
        b.close()


def test_wire_truncated(gpu, chain):
    """a buffer that ends inside its last record: that record decodes to zero bytes with unmarshal status
    1, verifies as not VALID, and is the certificate's offender"""
    from hyperdrive_amd import quorum
    from hyperdrive_amd.verify import CertSpec
    sigs = chain["sigs"]
    b = gpu.Verifier(0)
    try:
        b.set_variant("key_width", 13)
        b.set_signatories(np.frombuffer(b"".join(sigs), np.uint8).reshape(S, 32).copy())
        wire = chain["wires"][0]
        cert = [CertSpec(0, Q, "precommit", H0, RND, chain["values"][0], Q)]
        assert rows(quorum.check_certificates_wire(b, C, wire, cert)) == [(CC.OK, Q, CC.NEVER)]
        assert rows(quorum.check_certificates_wire(b, C, wire[:-7], cert)) == [(CC.BAD_SIGNATURE, Q - 1, Q - 1)]
        assert rows(quorum.check_certificates_wire(b, C, b"", [CertSpec(0, 0, C, H0, RND, bytes(32), 1)])) == \
            [(CC.SHORT, 0, CC.NEVER)]
    finally:
        b.close()
