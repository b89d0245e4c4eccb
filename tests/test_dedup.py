"""Repeats in the known-key check (HD_VAR_DEDUP; hd_dedup.h).

A vote whose height, round, value, From and 65 signature bytes equal an
earlier live vote's of the same call is checked once.  Every case here runs
its batch twice through the known-key check of a context with dedup on (keys
taught beforehand, 13-bit tables) and compares verdict, recovered signatory,
signer index and valid bitmap bit for bit with the same calls on a context
with dedup 0, and a sample of up to 512 messages with the C oracle.  The
counters (hd_ctx_dedup_stats) are checked against the number of repeats
computed here with numpy: votes that enter the check minus distinct rows among
them.  More repeats than that would be a wrong merge; the generator batches
must reach 99 % of it (the rest: the probe cutoff at table load <= 1/4).
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, N_GEN = 100, 8231     # 8231: a multiple of neither 64 nor 200, a partial last wave
SECP_N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
P_MINUS_N = 0x14551231950B75FC4402DA1722FC9BAEE


# ---- host check of the predicate and the hash (no GPU) ---------------------
def test_dedup_header_host_check_sanitized():
    """hd_dedup.h's equality predicate, hash, loads at the arrays' ends and
    table sizing, in a stand-alone program under ASan + UBSan.  (A missing
    compiler fails the test: this is the only host coverage of the two.)"""
    assert shutil.which("g++"), "g++ is needed for the host check of hd_dedup.h"
    out = os.path.join(ROOT, "tests", "native", "_build", "hd_dedup_check")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unused-function",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", out,
                    os.path.join(ROOT, "tests", "native", "hd_dedup_check.cpp")], check=True)
    r = subprocess.run([out], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout, r.stderr[-2000:])


def test_dedup_variant_and_binding():
    # (the library itself is not loaded here: the GPU cases below load it after torch)
    from hyperdrive_amd import _lib
    from hyperdrive_amd.verify import Verifier
    assert Verifier.VARIANTS["dedup"] == 12
    assert "hd_ctx_dedup_stats" in _lib.SIGNATURES


# ---- batches ----------------------------------------------------------------
def _take(b, idx):
    from hyperdrive_amd.verify import Batch
    idx = np.asarray(idx, np.int64)
    return Batch(b.type[idx].copy(), b.height[idx].copy(), b.round[idx].copy(), b.valid_round[idx].copy(),
                 b.value[idx].copy(), b.frm[idx].copy(), b.sig[idx].copy())


def _enters(b, admitted):
    """Messages that enter the known-key check once every admitted key is
    known: a valid type, an admitted From, and a signature that passes the
    range checks (v < 4, 0 < r, s < n, r + n < p when v & 2)."""
    adm = {x.tobytes() for x in admitted}
    out = np.zeros(len(b), bool)
    for i in range(len(b)):
        if not 1 <= int(b.type[i]) <= 3 or b.frm[i].tobytes() not in adm:
            continue
        sig = b.sig[i].tobytes()
        r, s, v = int.from_bytes(sig[:32], "big"), int.from_bytes(sig[32:64], "big"), sig[64]
        out[i] = v < 4 and 0 < r < SECP_N and 0 < s < SECP_N and (not (v & 2) or r < P_MINUS_N)
    return out


def _expected(b, admitted, digest=None):
    """(messages entering the check, repeats among its votes)"""
    n = len(b)
    live = _enters(b, admitted)
    votes = live & (b.type != 1)
    if digest is None:
        head = [b.height.view(np.uint8).reshape(n, 8), b.round.view(np.uint8).reshape(n, 8), b.value]
    else:
        head = [digest]
    rows = np.concatenate(head + [b.frm, b.sig], axis=1)[votes]
    distinct = len(np.unique(rows, axis=0)) if len(rows) else 0
    return int(live.sum()), int(votes.sum()) - distinct


class _World:
    """Two contexts over one admitted set, keys taught, dedup on and off."""

    def __init__(self, gpu):
        from hyperdrive_amd.device import generate
        self.v = {}
        for dd in (1, 0):
            v = gpu.Verifier(0)
            v.set_variant("key_width", 13)
            v.set_variant("foreign_keys", 0)
            v.set_variant("dedup", dd)
            self.v[dd] = v
        self.keys = self.v[1].gen_keys(S)
        self.sigs = self.keys[0]
        for v in self.v.values():
            v.set_signatories(self.sigs)
        db, _, _ = generate(self.v[1], 0, N_GEN, S, 0, keys=self.keys)
        self.honest = db.to_host()
        db, _, _ = generate(self.v[1], 0, N_GEN, S, 30, keys=self.keys)
        self.adv = db.to_host()
        for v in self.v.values():                  # one VALID message per signatory teaches its key
            res = v.verify_batch(self.honest)
            assert (res.verdict == 0).all()
            assert v.known_keys() == S
            assert v.dedup_stats() == (0, 0)       # nothing entered the check yet
        i0 = 0
        assert self.honest.type[i0] == 2
        self.i0 = i0

    def close(self):
        for v in self.v.values():
            v.close()


@pytest.fixture(scope="module")
def world(gpu):
    w = _World(gpu)
    yield w
    w.close()


def _launch(v, db, mode, digest, stream):
    import torch
    from hyperdrive_amd.digest import verify_digest_device
    n = db.n
    out = dict(verdict=torch.full((n,), 255, dtype=torch.uint8, device="cuda"),
               rec=torch.full((n, 32), 7, dtype=torch.uint8, device="cuda"),
               signer=torch.full((n,), -7, dtype=torch.int32, device="cuda"),
               bitmap=torch.full(((n + 31) // 32,), -1, dtype=torch.int32, device="cuda"))
    stream.wait_stream(torch.cuda.current_stream())
    if mode == "auth":
        v.authenticate_batch_device(db.c_struct(), out["verdict"].data_ptr(), stream.cuda_stream)
        out = dict(verdict=out["verdict"])
    elif mode == "digest":
        verify_digest_device(v, db, digest, out["verdict"].data_ptr(), out["rec"].data_ptr(),
                             out["signer"].data_ptr(), out["bitmap"].data_ptr(), stream=stream)
    else:
        v.verify_batch_device(db.c_struct(), out["verdict"].data_ptr(), out["rec"].data_ptr(),
                              out["signer"].data_ptr(), out["bitmap"].data_ptr(), stream.cuda_stream)
    return out


def _host(out):
    return {k: t.cpu().numpy() for k, t in out.items()}


def _check(world, coracle, b, mode="verify", lower=None, repeats_exact=None):
    """Runs b twice on both contexts; returns the dedup-on outputs."""
    import torch
    from hyperdrive_amd.device import DeviceBatch, work_stream
    from hyperdrive_amd.digest import SHA256, digest_device
    ws = work_stream()
    n = len(b)
    db = DeviceBatch.from_host(b)
    digest = hd = None
    if mode == "digest":
        digest = digest_device(world.v[1], SHA256, db)
        hd = digest.cpu().numpy()
    torch.cuda.synchronize()
    checked, repeats = _expected(b, world.sigs, hd)
    got = {}
    for dd in (1, 0):
        v = world.v[dd]
        for rnd in range(2):
            c0, r0 = v.dedup_stats()
            out = _launch(v, db, mode, digest, ws)
            ws.synchronize()
            c1, r1 = v.dedup_stats()
            print(f"n {n} mode {mode} dedup {dd} pass {rnd}: checked {c1 - c0} (expected {checked}), "
                  f"repeats {r1 - r0} (expected {repeats})")
            assert c1 - c0 == checked, (dd, rnd)
            if dd == 0:
                assert r1 - r0 == 0, rnd
            else:
                assert r1 - r0 <= repeats, (rnd, "a wrong merge")
                if lower is not None:
                    assert r1 - r0 >= lower * repeats, rnd
                if repeats_exact is not None:
                    assert r1 - r0 == repeats_exact, rnd
            h = _host(out)
            if (dd, 0) in got:
                for k in h:
                    assert h[k].tobytes() == got[(dd, 0)][k].tobytes(), (dd, k, "second pass differs")
            got[(dd, rnd)] = h
    on, off = got[(1, 1)], got[(0, 1)]
    for k in off:
        assert on[k].tobytes() == off[k].tobytes(), k
    # the C oracle on a sample
    pick = np.unique(np.linspace(0, n - 1, min(n, 512)).astype(np.int64))
    cv, crec = coracle.verify(_take(b, pick), world.sigs, True, threads=8)
    if mode == "auth":
        va = on["verdict"][pick]
        exact = np.isin(cv, (0, 6))
        assert (va[exact] == cv[exact]).all() and ((va == cv) | (va == 8)).all()
    else:
        assert on["verdict"][pick].tolist() == cv.tolist()
        assert on["rec"][pick].tobytes() == crec.tobytes()
        bits = np.unpackbits(on["bitmap"].view(np.uint8), bitorder="little")[:n]
        assert (bits == (on["verdict"] == 0)).all()
    return on


# ---- cases ------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("which", ["honest", "adv30"])
def test_generator_batches(world, coracle, which):
    """The library generator's C2 batch (40 % repeats), honest and 30 %
    adversarial: outputs equal, at least 99 % of the repeats found."""
    b = world.honest if which == "honest" else world.adv
    _, repeats = _expected(b, world.sigs)
    assert repeats > 0.2 * len(b)
    _check(world, coracle, b, lower=0.99)


@pytest.mark.gpu
def test_one_message_4096_times(world, coracle):
    """One vote repeated 4,096 times with alternating types: one slot, so the
    inversion kernels run with T at its minimum."""
    b = _take(world.honest, [world.i0] * 4096)
    b.type[:] = 2 + (np.arange(4096) & 1)
    on = _check(world, coracle, b, repeats_exact=4095)
    assert (on["verdict"] == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63])
def test_small_batches(world, coracle, n):
    # 63: the Prevote / Precommit pairs of 31 signatories and one single vote
    idx = [world.i0] if n == 1 else list(range(32)) + list(range(100, 131))
    b = _take(world.honest, idx)
    on = _check(world, coracle, b, lower=1.0)
    assert (on["verdict"] == 0).all()


@pytest.mark.gpu
def test_near_repeats_are_not_merged(world, coracle):
    """Copies of a vote that differ from it in exactly one byte of height,
    round, value32, from32, r, s or v (first and last byte of each), and a
    copy under another admitted From: no repeat may be found.  The one-byte
    from32 copies are no longer admitted Froms, so they never reach the
    table; on the device the table's From compare is exercised by the copy
    under another admitted From only (every From byte: the host check)."""
    fields = [("height", 8), ("round", 8), ("value", 32), ("frm", 32), ("r", 32), ("s", 32), ("v", 1)]
    muts = [(f, k) for f, w in fields for k in sorted({0, w - 1})]
    b = _take(world.honest, [world.i0] * (1 + len(muts) + 1))
    for j, (f, k) in enumerate(muts, start=1):
        if f in ("height", "round"):
            getattr(b, f).view(np.uint8).reshape(-1, 8)[j, k] ^= 1
        elif f in ("value", "frm"):
            getattr(b, f)[j, k] ^= 1
        else:
            b.sig[j, {"r": 0, "s": 32, "v": 64}[f] + k] ^= 1
    b.frm[-1] = world.sigs[(np.flatnonzero((world.sigs == b.frm[0]).all(axis=1))[0] + 1) % S]
    b.type[:] = 2 + (np.arange(len(b)) & 1)
    assert _expected(b, world.sigs)[1] == 0
    on = _check(world, coracle, b, repeats_exact=0)
    assert on["verdict"][0] == 0 and (on["verdict"][1:] != 0).all()


@pytest.mark.gpu
def test_propose_is_not_merged_with_a_vote(world, coracle):
    """A Propose and votes with equal height, round, value, From and
    signature: the votes merge, the Propose (another preimage) does not."""
    b = _take(world.honest, [world.i0] * 4)
    b.type[:] = [1, 2, 1, 3]
    on = _check(world, coracle, b, repeats_exact=1)
    assert on["verdict"].tolist()[1::2] == [0, 0] and 0 not in on["verdict"].tolist()[0::2]


@pytest.mark.gpu
def test_collision_flood_hits_the_probe_cutoff(world, coracle):
    """2,048 votes that agree on every word the hash reads (signature and
    From) and differ in height: all distinct, all on one probe sequence, so
    all but the first few give up at the cutoff.  Only the upper bound on the
    repeats applies."""
    b = _take(world.honest, [world.i0] * 2048)
    b.height[:] += np.arange(2048)
    on = _check(world, coracle, b, repeats_exact=0)
    assert on["verdict"][0] == 0 and (on["verdict"][1:] == 5).all()


@pytest.mark.gpu
def test_repeats_of_fallback_and_early_verdict_messages(world, coracle):
    """Repeats of a vote that ends in the full recovery (a signatory
    mismatch: another admitted From's key) and of votes with an early verdict
    (s = 0: BAD_RS; v = 2 with r + n >= p: NO_POINT): every copy gets the
    verdict of the dedup-off run.  The early-verdict copies never enter the
    table (their code is final in k_fast_prep), which is what the counters
    assert: only the 5 mismatch copies count as repeats."""
    b = _take(world.honest, [world.i0] * 18)
    b.type[:] = 2 + (np.arange(18) & 1)
    other = world.sigs[(np.flatnonzero((world.sigs == b.frm[0]).all(axis=1))[0] + 1) % S]
    b.frm[0:6] = other                            # mismatch, through the check and the recovery
    b.sig[6:12, 32:64] = 0                        # s = 0
    b.sig[12:18, 64] = 2                          # r + n >= p for a random r
    on = _check(world, coracle, b, repeats_exact=5)
    assert on["verdict"].tolist() == [5] * 6 + [2] * 6 + [3] * 6


@pytest.mark.gpu
def test_repeat_in_another_block(world, coracle):
    """A repeat 4,096 messages after its first copy (another block and wave)."""
    b = _take(world.honest, list(range(4097)))
    for f in ("height", "round", "value", "frm", "sig"):
        getattr(b, f)[4096] = getattr(b, f)[0]
    b.type[4096] = 3
    _, repeats = _expected(b, world.sigs)
    on = _check(world, coracle, b, lower=0.99)
    assert repeats > 1000 and (on["verdict"] == 0).all()


@pytest.mark.gpu
def test_authenticate_batch_device(world, coracle):
    _check(world, coracle, world.adv, mode="auth", lower=0.99)


@pytest.mark.gpu
def test_variant_values_and_null_arguments(world):
    from hyperdrive_amd import _lib
    lib = _lib.load()
    assert lib.hd_ctx_dedup_stats(None, None, None) == _lib.HD_EINVAL
    assert lib.hd_ctx_dedup_stats(world.v[1].handle, None, None) == 0
    assert world.v[1].variant("dedup") == 1 and world.v[0].variant("dedup") == 0
    assert lib.hd_ctx_set_variant(world.v[0].handle, 12, 2) == _lib.HD_EINVAL


@pytest.mark.gpu
def test_digest_in_call(world, coracle):
    """hd_verify_batch_digest_device keys the repeats on the digest row."""
    _check(world, coracle, world.adv, mode="digest", lower=0.99)


@pytest.mark.gpu
def test_three_calls_in_flight(world, coracle):
    """Three calls on three streams with nothing between them (the
    benchmark's shape), each on its own scratch set and repeat table."""
    import torch
    from hyperdrive_amd.device import DeviceBatch, generate, verify_streams
    streams = verify_streams(None, 3)
    dbs = [generate(world.v[1], 0, N_GEN, S, 0, start=k * N_GEN, keys=world.keys)[0] for k in range(3)]
    hbs = [db.to_host() for db in dbs]
    exp = [_expected(hb, world.sigs) for hb in hbs]
    torch.cuda.synchronize()
    res = {}
    for dd in (1, 0):
        v = world.v[dd]
        c0, r0 = v.dedup_stats()
        outs = [_launch(v, db, "verify", None, st) for db, st in zip(dbs, streams)]
        torch.cuda.synchronize()
        c1, r1 = v.dedup_stats()
        print(f"three streams dedup {dd}: checked {c1 - c0} (expected {sum(e[0] for e in exp)}), "
              f"repeats {r1 - r0} (expected {sum(e[1] for e in exp)})")
        assert c1 - c0 == sum(e[0] for e in exp)
        if dd:
            assert 0.99 * sum(e[1] for e in exp) <= r1 - r0 <= sum(e[1] for e in exp)
        else:
            assert r1 - r0 == 0
        res[dd] = [_host(o) for o in outs]
    for on, off, hb in zip(res[1], res[0], hbs):
        for k in off:
            assert on[k].tobytes() == off[k].tobytes(), k
        pick = np.arange(0, N_GEN, 17)[:512]
        cv, crec = coracle.verify(_take(hb, pick), world.sigs, True, threads=8)
        assert on["verdict"][pick].tolist() == cv.tolist() and on["rec"][pick].tobytes() == crec.tobytes()
