"""Shared preimages in the known-key check (HD_VAR_PRE_SHARE; hd_dedup.h,
DESIGN.md §4 "preimages").

A call without caller digests hashes each distinct preimage once.  Every case
here runs its batch through the known-key check of one context (keys taught
beforehand, 13-bit tables) with pre_share 1 and then 0 and compares verdict,
recovered signatory, signer index and valid bitmap byte for byte between the
two and with the C oracle (signer: From's index for a VALID message, else -1;
bitmap: the VALID messages).

A wrong shared digest would not show in the outputs of a VALID message: its
known-key check fails and the full recovery, which hashes for itself, still
returns VALID.  So every case also compares the number of messages that took
the full recovery (fastpath_stats) between the two settings; the validly
signed cases assert that it is 0.  The counters (hd_ctx_preimage_stats) are
checked against the distinct preimages counted here with numpy.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, N_GEN = 100, 8231     # 8231: a multiple of neither 64 nor 200, a partial last wave
DD_PROBES = 8            # hd_dedup.h HD_DD_PROBES
M32 = 0xFFFFFFFF


# ---- host checks (no GPU) ---------------------------------------------------
def test_preimage_header_host_check_sanitized():
    """hd_dedup.h's preimage key, predicate, hash (with the near misses) and
    pid encoding, in a stand-alone program under ASan + UBSan."""
    assert shutil.which("g++"), "g++ is needed for the host check of hd_dedup.h"
    out = os.path.join(ROOT, "tests", "native", "_build", "hd_preimage_check")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unused-function",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", out,
                    os.path.join(ROOT, "tests", "native", "hd_preimage_check.cpp")], check=True)
    r = subprocess.run([out], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout, r.stderr[-2000:])


def test_pre_share_variant_and_binding():
    # (the library itself is not loaded here: the GPU cases below load it after torch)
    from hyperdrive_amd import _lib
    from hyperdrive_amd.verify import Verifier
    assert Verifier.VARIANTS["pre_share"] == 15
    assert "hd_ctx_preimage_stats" in _lib.SIGNATURES


# ---- host copies of hd_dedup.h ----------------------------------------------
def _pre_hash(is_propose, valid_round, height, rnd, value):
    """dd_pre_hash"""
    hh, rr, vr = height & (2 ** 64 - 1), rnd & (2 ** 64 - 1), valid_round & (2 ** 64 - 1)
    v0, v7 = int.from_bytes(value[0:4], "big"), int.from_bytes(value[28:32], "big")
    h = ((hh & M32) * 0x9E3779B1) & M32
    h = ((h ^ (hh >> 32)) * 0x85EBCA6B) & M32
    h = ((h ^ (h >> 15) ^ (rr & M32)) * 0xC2B2AE35) & M32
    h = ((h ^ (rr >> 32)) * 0x27D4EB2F) & M32
    h = ((h ^ (h >> 13) ^ v0) * 0x165667B1) & M32
    h = ((h ^ v7) * 0x9E3779B1) & M32
    h = ((h ^ (h >> 14) ^ int(is_propose) ^ ((vr << 1) & M32)) * 0x85EBCA6B) & M32
    return h ^ (h >> 16)


def _table_words(n):
    """dd_table_words"""
    w = 1024
    while w < 4 * n and w < 0x80000000:
        w <<= 1
    return w


# ---- batches ----------------------------------------------------------------
def _take(b, idx):
    from hyperdrive_amd.verify import Batch
    idx = np.asarray(idx, np.int64)
    return Batch(b.type[idx].copy(), b.height[idx].copy(), b.round[idx].copy(), b.valid_round[idx].copy(),
                 b.value[idx].copy(), b.frm[idx].copy(), b.sig[idx].copy())


def _preimages(b):
    """(typed messages, distinct preimages among them)"""
    n = len(b)
    typed = (b.type >= 1) & (b.type <= 3)
    prop = b.type == 1
    vr = np.ascontiguousarray(np.where(prop, b.valid_round, 0).astype(np.int64))
    b8 = lambda a: np.ascontiguousarray(a).view(np.uint8).reshape(n, 8)
    rows = np.concatenate([prop.astype(np.uint8)[:, None], b8(vr), b8(b.height), b8(b.round), b.value], axis=1)[typed]
    return int(typed.sum()), (len(np.unique(rows, axis=0)) if len(rows) else 0)


def _signed(oracle, world, msgs):
    """A validly signed batch of (type, height, round, valid_round, value, signer)."""
    from hyperdrive_amd.verify import Batch
    n = len(msgs)
    b = Batch(np.zeros(n, np.uint8), np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64),
              np.zeros((n, 32), np.uint8), np.zeros((n, 32), np.uint8), np.zeros((n, 65), np.uint8))
    for i, (t, h, r, vr, value, k) in enumerate(msgs):
        b.type[i], b.height[i], b.round[i], b.valid_round[i] = t, h, r, vr
        b.value[i] = np.frombuffer(value, np.uint8)
        b.frm[i] = world.sigs[k]
        b.sig[i] = np.frombuffer(oracle.sign(oracle.signer_sk(k), oracle.message_digest(t, h, r, vr, value)), np.uint8)
    return b


class _World:
    """One context, keys taught; the generator's honest and adversarial batch."""

    def __init__(self, gpu):
        from hyperdrive_amd.device import generate
        v = gpu.Verifier(0)
        v.set_variant("key_width", 13)
        v.set_variant("foreign_keys", 0)
        self.v = v
        self.keys = v.gen_keys(S)
        self.sigs = self.keys[0]
        v.set_signatories(self.sigs)
        db, _, _ = generate(v, 0, N_GEN, S, 0, keys=self.keys)
        self.honest = db.to_host()
        db, _, _ = generate(v, 0, N_GEN, S, 30, keys=self.keys)
        self.adv = db.to_host()
        res = v.verify_batch(self.honest)          # one VALID message per signatory teaches its key
        assert (res.verdict == 0).all()
        assert v.known_keys() == S
        self.index = {s.tobytes(): k for k, s in enumerate(self.sigs)}

    def close(self):
        self.v.close()


@pytest.fixture(scope="module")
def world(gpu):
    w = _World(gpu)
    yield w
    w.close()


def _launch(v, db, digest, stream):
    import torch
    from hyperdrive_amd.digest import verify_digest_device
    n = db.n
    out = dict(verdict=torch.full((n,), 255, dtype=torch.uint8, device="cuda"),
               rec=torch.full((n, 32), 7, dtype=torch.uint8, device="cuda"),
               signer=torch.full((n,), -7, dtype=torch.int32, device="cuda"),
               bitmap=torch.full(((n + 31) // 32,), -1, dtype=torch.int32, device="cuda"))
    stream.wait_stream(torch.cuda.current_stream())
    if digest is not None:
        verify_digest_device(v, db, digest, out["verdict"].data_ptr(), out["rec"].data_ptr(),
                             out["signer"].data_ptr(), out["bitmap"].data_ptr(), stream=stream)
    else:
        v.verify_batch_device(db.c_struct(), out["verdict"].data_ptr(), out["rec"].data_ptr(),
                              out["signer"].data_ptr(), out["bitmap"].data_ptr(), stream.cuda_stream)
    return out


def _host(out):
    return {k: t.cpu().numpy() for k, t in out.items()}


def _against_oracle(world, coracle, b, got):
    """verdict, recovered signatory, signer and bitmap of a call against the C
    oracle (every message up to 1,024, else 512 spread over the batch)."""
    n = len(b)
    pick = np.arange(n) if n <= 1024 else np.unique(np.linspace(0, n - 1, 512).astype(np.int64))
    cv, crec = coracle.verify(_take(b, pick), world.sigs, True, threads=8)
    assert got["verdict"][pick].tolist() == cv.tolist()
    assert got["rec"][pick].tobytes() == crec.tobytes()
    want = [world.index[b.frm[i].tobytes()] if c == 0 else -1 for i, c in zip(pick, cv)]
    assert got["signer"][pick].tolist() == want
    bits = np.unpackbits(got["bitmap"].view(np.uint8), bitorder="little")[:n]
    assert (bits == (got["verdict"] == 0)).all()


def _check(world, coracle, b, distinct=None, digest_mode=False, fallback=None):
    """Runs b with pre_share 1, then 0; returns the pre_share 1 outputs.
    distinct: the ids expected (default: the distinct preimages of b)."""
    import torch
    from hyperdrive_amd.device import DeviceBatch, work_stream
    from hyperdrive_amd.digest import SHA256, digest_device
    ws = work_stream()
    v = world.v
    db = DeviceBatch.from_host(b)
    digest = digest_device(v, SHA256, db) if digest_mode else None
    torch.cuda.synchronize()
    typed, uniq = _preimages(b)
    if distinct is None:
        distinct = uniq
    got, fell = {}, {}
    try:
        for ps in (1, 0):
            v.set_variant("pre_share", ps)
            t0, d0 = v.preimage_stats()
            out = _launch(v, db, digest, ws)
            ws.synchronize()
            t1, d1 = v.preimage_stats()
            fell[ps] = v.fastpath_stats()[1]
            print(f"n {len(b)} pre_share {ps}: typed {t1 - t0} (of {typed}), distinct {d1 - d0} (expected {distinct}), "
                  f"full recoveries {fell[ps]}")
            if ps == 1 and not digest_mode:
                assert (t1 - t0, d1 - d0) == (typed, distinct)
            else:
                assert (t1 - t0, d1 - d0) == (0, 0)
            got[ps] = _host(out)
    finally:
        v.set_variant("pre_share", 1)
    for k in got[0]:
        assert got[1][k].tobytes() == got[0][k].tobytes(), k
    assert fell[1] == fell[0]
    if fallback is not None:
        assert fell[1] == fallback
    _against_oracle(world, coracle, b, got[1])
    return got[1]


# ---- cases ------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_wave_and_block_edges(world, coracle, n):
    on = _check(world, coracle, _take(world.honest, range(n)), fallback=0)
    assert (on["verdict"] == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["honest", "adv30"])
def test_generator_batches(world, coracle, which):
    """The library generator's C2 batch, honest and 30 % adversarial: 200
    messages per height, so far fewer preimages than messages."""
    b = world.honest if which == "honest" else world.adv
    typed, uniq = _preimages(b)
    assert uniq < 0.2 * typed
    on = _check(world, coracle, b, fallback=0 if which == "honest" else None)
    if which == "honest":
        assert (on["verdict"] == 0).all()


@pytest.mark.gpu
def test_all_messages_share_one_preimage(world, coracle):
    """4,096 votes of 100 signers over one preimage: one id, one hash."""
    h = world.honest
    first = np.flatnonzero(h.height == h.height[0])
    same = first[(h.value[first] == h.value[first[0]]).all(axis=1)]
    assert len(np.unique(h.frm[same], axis=0)) > S // 2 and set(h.type[same].tolist()) == {2, 3}
    b = _take(h, np.resize(same, 4096))
    on = _check(world, coracle, b, distinct=1, fallback=0)
    assert (on["verdict"] == 0).all()


@pytest.mark.gpu
def test_every_message_has_its_own_preimage(world, coracle):
    """One validly signed vote per height (1,031 heights, signers in turn):
    as many ids as messages, more than one block of k_pre_hash."""
    from hyperdrive_amd.device import generate
    n = 1031
    db, _, _ = generate(world.v, 0, n * 2 * S, S, 0, keys=world.keys)
    k = np.arange(n)
    b = _take(db.to_host(), k * 2 * S + k % S)
    assert len(np.unique(b.height)) == n
    on = _check(world, coracle, b, distinct=n, fallback=0)
    assert (on["verdict"] == 0).all()


@pytest.mark.gpu
def test_near_misses_do_not_share(world, coracle, oracle):
    """Validly signed messages whose preimages differ in one respect only:
    the last value byte, the high word of height, the high word of round,
    propose against vote, a propose's valid_round.  A wrong share gives a
    message another's digest: its check fails and it takes the full recovery."""
    va, vb = bytes(range(32)), bytes(range(31)) + b"\xfe"
    H, R = 77, 3
    msgs = [(2, H, R, -1, va, 0), (3, H, R, -1, va, 1),            # the base preimage, twice
            (2, H, R, -1, vb, 2),                                  # last value byte
            (2, H + (1 << 32), R, -1, va, 3), (3, H + (5 << 32), R, -1, va, 4),   # height, high word
            (2, H, R + (1 << 32), -1, va, 5), (3, H, R + (1 << 40), -1, va, 6),   # round, high word
            (1, H, R, -1, va, 7), (1, H, R, 0, va, 8), (1, H, R, 2, va, 9),       # proposes: valid_round
            (1, H, R, 2, va, 10),                                  # ... and one that does share
            (1, H, R, 2 + (1 << 32), va, 11)]                      # valid_round, high word
    b = _signed(oracle, world, msgs)
    assert _preimages(b) == (12, 10)
    on = _check(world, coracle, b, distinct=10, fallback=0)
    assert (on["verdict"] == 0).all()


@pytest.mark.gpu
def test_collision_flood_hits_the_probe_cutoff(world, coracle):
    """13 distinct preimages on one probe sequence of the preimage table
    (heights searched with the host copy of dd_pre_hash), three votes each.
    Whichever 8 claim the sequence's slots get one id each; the messages of
    the other 5 find neither a free slot nor an equal claimant within the
    cutoff and count on their own: 8 + 5 * 3 ids, whatever the order."""
    F, copies = 13, 3
    base = _take(world.honest, [0])
    mask = _table_words(F * copies) - 1
    value, rnd = base.value[0].tobytes(), int(base.round[0])
    target = _pre_hash(False, 0, 1 << 20, rnd, value) & mask
    heights = [h for h in range(1 << 20, (1 << 20) + 200000) if _pre_hash(False, 0, h, rnd, value) & mask == target][:F]
    assert len(heights) == F > DD_PROBES
    signers = np.flatnonzero(world.honest.height == world.honest.height[0])[:copies]
    b = _take(world.honest, np.tile(signers, F))
    b.height[:] = np.repeat(heights, copies)
    b.value[:] = base.value[0]
    assert _preimages(b) == (F * copies, F)
    want = DD_PROBES + (F - DD_PROBES) * copies
    on = _check(world, coracle, b, distinct=want)
    assert (on["verdict"] != 0).all()          # (signed for another height: the full recovery's verdict)


@pytest.mark.gpu
def test_bad_types_between_sharers(world, coracle):
    """Messages with a type outside 1..3 between messages that share: no id,
    BAD_TYPE, and their neighbours' digests are untouched."""
    b = _take(world.honest, range(130))
    b.type[[0, 10, 11, 64, 129]] = [0, 4, 255, 0, 9]
    assert _preimages(b)[0] == 125
    on = _check(world, coracle, b, fallback=0)
    assert int((on["verdict"] == 0).sum()) == 125


@pytest.mark.gpu
def test_three_calls_in_flight(world, coracle):
    """Three calls on three streams with nothing between them (the
    benchmark's shape), each on its own scratch set and tables."""
    import torch
    from hyperdrive_amd.device import generate, verify_streams
    v = world.v
    streams = verify_streams(None, 3)
    dbs = [generate(v, 0, N_GEN, S, 0, start=k * N_GEN, keys=world.keys)[0] for k in range(3)]
    hbs = [db.to_host() for db in dbs]
    exp = [_preimages(hb) for hb in hbs]
    torch.cuda.synchronize()
    res = {}
    try:
        for ps in (1, 0):
            v.set_variant("pre_share", ps)
            t0, d0 = v.preimage_stats()
            outs = [_launch(v, db, None, st) for db, st in zip(dbs, streams)]
            torch.cuda.synchronize()
            t1, d1 = v.preimage_stats()
            print(f"three streams pre_share {ps}: typed {t1 - t0}, distinct {d1 - d0} (expected {sum(e[1] for e in exp)})")
            assert (t1 - t0, d1 - d0) == ((sum(e[0] for e in exp), sum(e[1] for e in exp)) if ps else (0, 0))
            res[ps] = [_host(o) for o in outs]
    finally:
        v.set_variant("pre_share", 1)
    for on, off, hb in zip(res[1], res[0], hbs):
        for k in off:
            assert on[k].tobytes() == off[k].tobytes(), k
        assert (on["verdict"] == 0).all()
        _against_oracle(world, coracle, hb, on)


@pytest.mark.gpu
def test_digest_in_call_is_unaffected(world, coracle):
    """A call with caller-supplied digests shares nothing and counts nothing."""
    _check(world, coracle, world.adv, digest_mode=True)


@pytest.mark.gpu
def test_variant_values_and_null_arguments(world):
    from hyperdrive_amd import _lib
    lib = _lib.load()
    v = world.v
    assert lib.hd_ctx_preimage_stats(None, None, None) == _lib.HD_EINVAL
    assert lib.hd_ctx_preimage_stats(v.handle, None, None) == 0
    assert v.variant("pre_share") == 1
    with pytest.raises(_lib.HDError):
        v.set_variant("pre_share", 2)
    assert lib.hd_ctx_set_variant(v.handle, 15, 2) == _lib.HD_EINVAL
    assert lib.hd_ctx_set_variant(v.handle, 15, -1) == _lib.HD_EINVAL
    assert v.variant("pre_share") == 1
