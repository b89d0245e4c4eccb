"""Signatures at the arithmetic's edges through the product kernels.

The generator's messages and its 13 adversarial classes steer verdicts, not
operand values: every scalar and field operand they give the kernels is
uniformly random.  The rows here choose the operands (s, m, r, the known-key
check's u1 and u2, the full recovery's join) under known keys and solve for
the digest, which is supplied (hd_verify_batch_digest_device), in the way of
test_gpu_verify.py's _zero_digit_rows:

1. s in {1, 2, n-1, n-2, (n-1)/2, (n+1)/2, 2^255, c = 2^256 - n};
2. m = 0 (a zero digest, and the digest n), n-1, and the digests 2^256 - 1
   and n + 5, which sc_from_be_reduce must reduce;
3. r = 1 and the largest r < n whose x lifts; the signer is whatever the
   oracle recovers, and that signatory is admitted;
4. v & 2, x = r + n: r = 2, 4, 6 (the lift succeeds: VALID), r = p - n - 1,
   and r = p - n (NO_POINT by the range check);
5. a known-key sum that meets its own partial sum: u1 = c d (the first key
   window doubles) and u1 = -c d (it cancels) with u2's window-0 digit c,
   for c = 1 and 5: k_fast_sums ends with ZZ = 0 and marks the row for the
   full recovery, and the inversion kernels must treat it as a leaf 1 or
   the whole lane's batch inverse is zero;
6. the full recovery's join doubling: m = -s k, so that u1 G = u2 R.

Every row has a twin with a mismatching (admitted) From.  The rows are spread
evenly through about 540 honest, distinct messages of the library generator
whose digests come from hd_digest_batch_device, so that every inversion lane
holds crafted rows and honest ones.  Three passes per context -- the full
recovery (no key known yet), the known-key check, the known-key check again --
compare verdict, recovered signatory, signer index and bitmap with
oracle.recover (crafted rows) and the C oracle (filler).  On passes 2 and 3
the fallback count is what the construction implies: the rows that pass the
signature's range checks and then fail the check, i.e. the mismatching twins,
the four collision rows, and the honest rows whose verdict is not VALID.
"""
import random

import numpy as np
import pytest

from test_dedup import _host, _launch

S = 4            # the filler's signatories
N_FILL = 540
LIFT_RS = (2, 4, 6)


def _sig(r, s, v):
    return r.to_bytes(32, "big") + s.to_bytes(32, "big") + bytes([v])


def _nonce_point(O, k):
    R = O.point_mul(k, O.G)
    return R[0] % O.N, (R[1] & 1) | (2 if R[0] >= O.N else 0)


def build_rows(O):
    """[(what, signer or None, sig, digest, collision)]: signer None means `whoever the oracle recovers`"""
    keys = O.KeyCache()
    rng = random.Random(2026)
    n, p = O.N, O.P
    c = 2 ** 256 - n
    rows = []
    j = 0

    def key():
        nonlocal j
        j += 1
        return j % S, keys.sk(j % S)

    def rand_k():
        return rng.randrange(1, n)

    for s in (1, 2, n - 1, n - 2, (n - 1) // 2, (n + 1) // 2, 2 ** 255, c):            # 1: s, k chosen
        signer, d = key()
        k = rand_k()
        r, v = _nonce_point(O, k)
        m = (s * k - r * d) % n
        rows.append((f"s={s:#x}", signer, _sig(r, s, v), m.to_bytes(32, "big"), False))
    for m, dg in ((0, 0), (0, n), (n - 1, n - 1), (c - 1, 2 ** 256 - 1), (5, n + 5)):  # 2: m, k chosen
        signer, d = key()
        k = rand_k()
        r, v = _nonce_point(O, k)
        s = (m + r * d) * pow(k, -1, n) % n
        assert s and dg % n == m
        rows.append((f"digest={dg:#x}", signer, _sig(r, s, v), dg.to_bytes(32, "big"), False))
    top = n - 1
    while O.lift_x(top, 1) is None:
        top -= 1
    for r, v in ((1, 0), (top, 1)):                                                   # 3: r chosen
        rows.append((f"r={r:#x}", None, _sig(r, rand_k(), v), rng.randbytes(32), False))
    for i, r in enumerate(LIFT_RS + (p - n - 1, p - n)):                              # 4: x = r + n
        rows.append((f"r={r:#x} v&2", None, _sig(r, rand_k(), 2 | (i & 1)), rng.randbytes(32), False))
    for cc in (1, 5):                                                                 # 5: u1 = +-c d
        for sign in (1, -1):
            signer, d = key()
            u2 = (rng.randrange(1, 2 ** 230) << 22) | cc
            u1 = sign * cc * d % n
            k = (u1 + u2 * d) % n
            r, v = _nonce_point(O, k)
            s = r * pow(u2, -1, n) % n
            m = u1 * s % n
            rows.append((f"u1={'+' if sign > 0 else '-'}{cc}d", signer, _sig(r, s, v), m.to_bytes(32, "big"), True))
    signer, d = key()                                                                 # 6: m = -s k
    k = rand_k()
    r, v = _nonce_point(O, k)
    s = r * d * pow(2 * k, -1, n) % n
    m = -s * k % n
    rows.append(("m=-sk", signer, _sig(r, s, v), m.to_bytes(32, "big"), False))
    return rows, keys


class Crafted:
    """the crafted rows with their twins, the admitted set and what the oracle says of each"""

    def __init__(self, O):
        rows, keys = build_rows(O)
        self.admitted = [keys.signatory(k) for k in range(S)]
        recovered = []
        for what, signer, sig, dg, coll in rows:
            verdict, Q = O.recover(dg, sig)
            recovered.append(O.signatory_of_pub(Q, True) if verdict == O.VALID else None)
            if signer is None and recovered[-1] is not None and recovered[-1] not in self.admitted:
                self.admitted.append(recovered[-1])
        assert len(self.admitted) - S <= 16
        self.what, self.frm, self.sig, self.digest = [], [], [], []
        self.verdict, self.rec, self.signer, self.leaves = [], [], [], []
        self.collision = []
        for t, ((what, signer, sig, dg, coll), got) in enumerate(zip(rows, recovered)):
            honest = keys.signatory(signer) if signer is not None else got if got is not None else self.admitted[1]
            other = self.admitted[(self.admitted.index(honest) + 1 + t % (S - 1)) % S]
            assert other != honest
            for frm in (honest, other):
                verdict, _ = O.recover(dg, sig)
                if verdict == O.VALID:
                    verdict = O.VALID if got == frm else O.SIGNATORY_MISMATCH
                r, s, v = int.from_bytes(sig[:32], "big"), int.from_bytes(sig[32:64], "big"), sig[64]
                in_range = v < 4 and 0 < r < O.N and 0 < s < O.N and (not (v & 2) or r < O.P - O.N)
                self.what.append(what + ("" if frm == honest else " (twin)"))
                self.frm.append(frm)
                self.sig.append(sig)
                self.digest.append(dg)
                self.verdict.append(verdict)
                self.rec.append(got if got is not None else bytes(32))
                self.signer.append(self.admitted.index(frm) if verdict == O.VALID else -1)
                self.collision.append(coll and frm == honest)
                # leaves the known-key check for the full recovery: in range, and the check cannot say VALID
                self.leaves.append(in_range and (verdict != O.VALID or (coll and frm == honest)))
        self.n = len(self.what)


@pytest.fixture(scope="module")
def crafted(oracle):
    return Crafted(oracle)


# ---- no GPU: the rows are what they are named ----------------------------------
def test_rows_are_what_they_claim(oracle, crafted):
    O, c = oracle, crafted
    by = {w: k for k, w in enumerate(c.what)}
    honest = [k for k, w in enumerate(c.what) if not w.endswith("(twin)")]
    # every row under a known key is VALID for its signer, SIGNATORY_MISMATCH for the twin
    for k in honest:
        if not c.what[k].startswith("r="):
            assert c.verdict[k] == O.VALID and c.verdict[k + 1] == O.SIGNATORY_MISMATCH, c.what[k]
    for r in LIFT_RS:                                    # the x = r + n lift ends VALID
        k = by[f"r={r:#x} v&2"]
        assert c.verdict[k] == O.VALID and c.sig[k][64] & 2 and O.lift_x(r + O.N, c.sig[k][64] & 1) is not None
    assert c.verdict[by[f"r={O.P - O.N:#x} v&2"]] == O.NO_POINT
    assert c.verdict[by["r=0x1"]] in (O.VALID, O.NO_POINT)
    top = int.from_bytes(c.sig[[k for k in honest if c.what[k].startswith("r=") and "v&2" not in c.what[k]][1]][:32],
                         "big")
    assert O.lift_x(top, 1) is not None and all(O.lift_x(x, 1) is None for x in range(top + 1, O.N))
    # the collisions: u1 G = +-c P and the first key digit is c, at every table width
    keys = O.KeyCache()
    for k in honest:
        if not c.collision[k]:
            continue
        sig, m = c.sig[k], int.from_bytes(c.digest[k], "big") % O.N
        r, s = int.from_bytes(sig[:32], "big"), int.from_bytes(sig[32:64], "big")
        u1, u2 = m * pow(s, -1, O.N) % O.N, r * pow(s, -1, O.N) % O.N
        d = keys.sk(c.admitted.index(c.frm[k]))
        cc = int(c.what[k][4])
        assert u1 in (cc * d % O.N, -cc * d % O.N) and u2 & (2 ** 22 - 1) == cc
    k = by["m=-sk"]                                      # the join: u1 G = u2 R in the full recovery
    sig, m = c.sig[k], int.from_bytes(c.digest[k], "big")
    r, s = int.from_bytes(sig[:32], "big"), int.from_bytes(sig[32:64], "big")
    R = O.lift_x(r, sig[64] & 1)
    assert O.point_mul(-m * pow(r, -1, O.N) % O.N, O.G) == O.point_mul(s * pow(r, -1, O.N) % O.N, R)
    # the fallback count of passes 2 and 3: the twins in range, the four collisions, the honest non-VALID rows
    twins = sum(1 for k in honest if c.leaves[k + 1])
    assert twins == len(honest) - 1                      # all but r = p - n, which the range check decides
    other = sum(1 for k in honest if c.leaves[k] and not c.collision[k])
    assert sum(c.collision) == 4 and sum(c.leaves) == twins + 4 + other
    assert other == sum(1 for k in honest if c.verdict[k] != O.VALID) - 1
    # 24 twins, 4 collisions, and r = p - n - 1 (in range, but x = p - 1 is on no point)
    assert (twins, other, sum(c.leaves)) == (24, 1, 29)


# ---- GPU -------------------------------------------------------------------------
class _Mixed:
    """the crafted rows spread through the filler, on the device, with digests and expectations"""

    def __init__(self, gpu, oracle, coracle, crafted):
        import torch
        from hyperdrive_amd.device import DeviceBatch, generate
        from hyperdrive_amd.digest import SHA256, digest_device
        from hyperdrive_amd.verify import Batch
        c = crafted
        v = gpu.Verifier(0)
        try:
            ks = v.gen_keys(S)
            assert [bytes(x) for x in ks[0]] == c.admitted[:S]
            self.admitted = np.frombuffer(b"".join(c.admitted), np.uint8).reshape(-1, 32).copy()
            fill_db = generate(v, 0, N_FILL, S, 0, keys=ks)[0]
            fb = fill_db.to_host()
            n = N_FILL + c.n
            self.pos = np.array([(2 * k + 1) * n // (2 * c.n) for k in range(c.n)], np.int64)   # evenly spread
            assert len(set(self.pos.tolist())) == c.n and np.diff(self.pos).max() < 64
            self.fill = np.setdiff1d(np.arange(n), self.pos)
            rng = random.Random(7)

            def mix(filler, made, dtype, width=None):
                a = np.zeros((n,) if width is None else (n, width), dtype)
                a[self.fill] = filler
                a[self.pos] = made
                return a
            u8 = lambda rows, w: np.frombuffer(b"".join(rows), np.uint8).reshape(-1, w)   # noqa: E731
            b = Batch(mix(fb.type, 2, np.uint8), mix(fb.height, 10_000 + np.arange(c.n), np.int64),
                      mix(fb.round, 0, np.int64), mix(fb.valid_round, -1, np.int64),
                      mix(fb.value, u8([rng.randbytes(32) for _ in range(c.n)], 32), np.uint8, 32),
                      mix(fb.frm, u8(c.frm, 32), np.uint8, 32), mix(fb.sig, u8(c.sig, 65), np.uint8, 65))
            self.n = n
            self.db = DeviceBatch.from_host(b)
            self.fill_db = fill_db
            self.digest = digest_device(v, SHA256, self.db).clone()
            self.digest[torch.from_numpy(self.pos).cuda()] = torch.from_numpy(u8(c.digest, 32).copy()).cuda()
            torch.cuda.synchronize()
        finally:
            v.close()
        cv, crec = coracle.verify(fb, self.admitted, True, threads=8)
        assert (cv == 0).all()
        adm = [bytes(x) for x in self.admitted]
        self.verdict = mix(cv, np.array(c.verdict, np.uint8), np.uint8)
        self.rec = mix(crec, u8(c.rec, 32), np.uint8, 32)
        self.signer = mix(np.array([adm.index(bytes(f)) for f in fb.frm], np.int32), np.array(c.signer, np.int32),
                          np.int32)
        self.fallbacks = sum(c.leaves)

    def check(self, out, what):
        got = _host(out)
        bad = np.nonzero(got["verdict"] != self.verdict)[0]
        assert len(bad) == 0, (what, "verdict", bad.tolist(), got["verdict"][bad].tolist(), self.verdict[bad].tolist())
        assert got["rec"].tobytes() == self.rec.tobytes(), (what, "recovered signatory")
        assert got["signer"].tolist() == self.signer.tolist(), (what, "signer index")
        bits = np.unpackbits(got["bitmap"].view(np.uint8), bitorder="little")[:self.n]
        assert (bits == (self.verdict == 0)).all(), (what, "bitmap")


@pytest.fixture(scope="module")
def mixed(gpu, oracle, coracle, crafted):
    return _Mixed(gpu, oracle, coracle, crafted)


CONTEXTS = {"defaults": {}, "split_k16": {"split_k": 16}, "key_width13": {"key_width": 13},
            "key_width16": {"key_width": 16},
            "overlap": {"sum_waves": 3, "key_width": 13, "foreign_keys": 0, "sum_cap": 1, "sum_chain": 1, "lean_inv": 1}}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CONTEXTS))
def test_edge_signatures_through_the_product_kernels(gpu, mixed, crafted, name):
    from hyperdrive_amd.device import work_stream
    ws = work_stream()
    v = gpu.Verifier(0)
    try:
        for key, value in CONTEXTS[name].items():
            v.set_variant(key, value)
        v.set_signatories(mixed.admitted)

        def honest_call():   # synchronised; after the first the leftover estimate is 0, the second takes the path
            for _ in range(2):
                out = _launch(v, mixed.fill_db, "verify", None, ws)
                ws.synchronize()
                assert (_host(out)["verdict"] == 0).all()
        for rnd in range(3):
            if name == "overlap" and rnd > 0:
                honest_call()
            before = v.overlap_stats()
            out = _launch(v, mixed.db, "digest", mixed.digest, ws)
            ws.synchronize()
            mixed.check(out, (name, rnd))
            if rnd == 0:
                assert v.known_keys() == len(mixed.admitted)      # every admitted key signed a VALID row
                continue
            # the rows that leave the check: mismatching twins in range, collisions, honest non-VALID rows
            assert v.fastpath_stats()[1] == mixed.fallbacks, (name, rnd)
            if name == "overlap":   # the measured call ran capped and lean: not the register forms
                capped, lean, _ = (a - b for a, b in zip(v.overlap_stats(), before))
                assert (capped, lean) == (1, 1), (capped, lean)
    except RuntimeError as e:   # a device error (HDError, torch): nothing more is started on this GPU
        pytest.exit(f"{name}: {e}", returncode=3)
    finally:
        v.close()
