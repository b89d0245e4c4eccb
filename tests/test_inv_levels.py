"""The lean inversions in two levels (hd_ctx_inv_levels; hd_inv2.h,
hd_fastverify.hip).

With inv_levels 2 each lean inversion kernel runs as three kernels (up, mid,
down) and one divstep inversion serves K * K2 slots; what a call returns is
unchanged.  Every GPU case here forces the overlap path at small sizes as
test_sums_overlap does (sum_waves 3, sum_cap, sum_chain, lean_inv 1), for
split_k 8 and 16, and compares verdict, recovered signatory, signer index and
valid bitmap byte for byte between three contexts: inv_levels 2, inv_levels 1
(the one-level lean kernels) and lean_inv 0 (the register forms); the
adversarial case also against the C oracle on a 512-message sample.  Each
case asserts from hd_ctx_inv_stats which form its call launched.

As in test_sums_overlap, a call that follows one with many leftovers runs off
the overlap path, so every case first makes honest, synchronised calls.
"""
import ctypes
import os
import re

import numpy as np
import pytest

from test_dedup import _host, _launch, _take

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, N_ADV, N_TEACH = 100, 8231, 1024
FORMS = ("two", "one", "reg")
# form -> what one call adds to hd_ctx_inv_stats
ADDS = {"two": (1, 0), "one": (0, 1), "reg": (0, 0)}


# ---- no GPU -----------------------------------------------------------------
def test_binding_and_header():
    """Both calls are bound and documented, and the switch is no variant key."""
    from hyperdrive_amd import _lib
    from hyperdrive_amd.verify import Verifier
    text = open(os.path.join(ROOT, "include", "hd_verify.h")).read()
    for name in ("hd_ctx_inv_levels", "hd_ctx_inv_stats"):
        assert name in _lib.SIGNATURES
        assert re.search(r"\bint %s\(hd_ctx\* ctx, " % name, text)
    assert "HD_INV_LEVELS" in text
    assert not any("inv_levels" in k for k in Verifier.VARIANTS)
    assert "HD_VAR_INV" not in text
    lib = _lib.load()
    out = (ctypes.c_uint64 * 2)()
    assert lib.hd_ctx_inv_levels(None, -1) == _lib.HD_EINVAL
    assert lib.hd_ctx_inv_stats(None, out) == _lib.HD_EINVAL


# ---- contexts and batches ---------------------------------------------------
def _context(gpu, k, form):
    v = gpu.Verifier(0)
    v.set_variant("key_width", 13)
    v.set_variant("foreign_keys", 0)
    v.set_variant("sum_waves", 3)
    v.set_variant("sum_cap", 1)
    v.set_variant("sum_chain", 1)
    v.set_variant("lean_inv", 0 if form == "reg" else 1)
    v.set_variant("split_k", k)
    assert v.inv_levels(2 if form == "two" else 1) == (2 if form == "two" else 1)
    return v


class _World:
    def __init__(self, gpu):
        import torch
        from hyperdrive_amd.device import DeviceBatch, generate, verify_streams
        self.gpu = gpu
        self.v = {(k, f): _context(gpu, k, f) for k in (8, 16) for f in FORMS}
        first = self.v[(8, "reg")]
        self.keys = first.gen_keys(S)
        self.sigs = self.keys[0]
        n_max = 16 * 16 * 64 + 1
        self.honest = generate(first, 0, n_max, S, 0, keys=self.keys)[0].to_host()
        self.adv = generate(first, 0, N_ADV, S, 30, start=n_max, keys=self.keys)[0].to_host()
        self.teach = _take(self.honest, np.arange(N_TEACH))
        self.d_teach = DeviceBatch.from_host(self.teach)
        self.streams = verify_streams(None, 3)
        for v in self.v.values():
            self.teach_keys(v)
        torch.cuda.synchronize()

    def teach_keys(self, v):
        v.set_signatories(self.sigs)
        res = v.verify_batch(self.teach)   # a VALID message of every signatory teaches its key
        assert (res.verdict == 0).all()
        assert v.known_keys() == S

    def alone(self, v, db, stream=0):
        st = self.streams[stream]
        out = _launch(v, db, "verify", None, st)
        st.synchronize()
        return _host(out)

    def settle(self, v):
        """Two honest, synchronised calls: after the first the leftover figure
        the path rule reads is 0, so the calls that follow take the overlap
        path for as long as only honest calls precede them."""
        self.alone(v, self.d_teach, 2)
        self.alone(v, self.d_teach, 2)

    def close(self):
        for v in self.v.values():
            v.close()


@pytest.fixture(scope="module")
def world(gpu):
    w = _World(gpu)
    yield w
    w.close()


class _Form:
    """Asserts from hd_ctx_inv_stats and hd_ctx_overlap_stats that the `calls`
    calls made inside the block launched the form the context stands for."""

    def __init__(self, v, form, calls=1):
        self.v, self.form, self.calls = v, form, calls

    def __enter__(self):
        self.inv, self.over = self.v.inv_stats(), self.v.overlap_stats()
        return self

    def __exit__(self, *exc):
        if exc[0] is None:
            inv = tuple(a - b for a, b in zip(self.v.inv_stats(), self.inv))
            capped, lean, _ = (a - b for a, b in zip(self.v.overlap_stats(), self.over))
            assert inv == tuple(self.calls * x for x in ADDS[self.form]), (self.form, inv)
            assert capped == self.calls and lean == (0 if self.form == "reg" else self.calls), (self.form, capped, lean)


def _three_forms(world, k, db, dedup):
    """db alone on the three contexts of split_k k; asserts the three equal
    byte for byte and returns the two-level outputs with each context's
    (checked, repeats) of the call."""
    got, stats = {}, {}
    for f in FORMS:
        v = world.v[(k, f)]
        v.set_variant("dedup", dedup)
        world.settle(v)
        d0 = v.dedup_stats()
        with _Form(v, f):
            got[f] = world.alone(v, db)
        d1 = v.dedup_stats()
        stats[f] = (d1[0] - d0[0], d1[1] - d0[1])
    for f in ("one", "reg"):
        for key in got[f]:
            assert got["two"][key].tobytes() == got[f][key].tobytes(), (k, f, key)
    assert stats["two"] == stats["one"] == stats["reg"], stats
    bits = np.unpackbits(got["two"]["bitmap"].view(np.uint8), bitorder="little")[:db.n]
    assert (bits == (got["two"]["verdict"] == 0)).all()
    return got["two"], stats["two"]


# ---- cases ------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("k", [8, 16])
@pytest.mark.parametrize("size", ["64", "64K", "64K+1", "1024K+1"])
def test_honest_every_message_a_slot(world, k, size):
    """dedup 0: every live message takes a slot, nc == n exactly.  One wave
    at level 1; full lanes; one slot in a second round; and 1024 K + 1, the
    first size with a second wave at level 2 (K2 = 16)."""
    from hyperdrive_amd.device import DeviceBatch
    n = {"64": 64, "64K": 64 * k, "64K+1": 64 * k + 1, "1024K+1": 1024 * k + 1}[size]
    out, (checked, repeats) = _three_forms(world, k, DeviceBatch.from_host(_take(world.honest, np.arange(n))), 0)
    assert (out["verdict"] == 0).all()
    assert (checked, repeats) == (n, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [8, 16])
def test_adversarial_with_repeats(world, coracle, k):
    """30 % adversarial, dedup 1: repeats, early verdicts, leftovers, and sums
    that end at infinity (dead slots for the Z pass)."""
    from hyperdrive_amd.device import DeviceBatch
    out, (checked, repeats) = _three_forms(world, k, DeviceBatch.from_host(world.adv), 1)
    assert 0 < repeats < checked < N_ADV
    assert (out["verdict"] == 0).any() and (out["verdict"] != 0).any()
    pick = np.unique(np.linspace(0, N_ADV - 1, 512).astype(np.int64))
    cv, crec = coracle.verify(_take(world.adv, pick), world.sigs, True, threads=8)
    assert out["verdict"][pick].tolist() == cv.tolist()
    assert out["rec"][pick].tobytes() == crec.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("k", [8, 16])
def test_one_message_4096_times(world, k):
    """All repeats: one slot, nc == 1, one live lane at each level."""
    from hyperdrive_amd.device import DeviceBatch
    assert world.honest.type[0] == 2
    b = _take(world.honest, [0] * 4096)
    b.type[:] = 2 + (np.arange(4096) & 1)
    out, (checked, repeats) = _three_forms(world, k, DeviceBatch.from_host(b), 1)
    assert (checked, repeats) == (4096, 4095)
    assert (out["verdict"] == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("k", [8, 16])
def test_first_call_on_a_fresh_context(world, k):
    """No key is known yet: nothing takes a slot (nc == 0, T == 0), every
    message goes to the full recovery, and the two-level kernels were
    launched all the same."""
    v = _context(world.gpu, k, "two")
    try:
        v.set_signatories(world.sigs)
        assert v.known_keys() == 0
        d0 = v.dedup_stats()
        with _Form(v, "two"):
            got = world.alone(v, world.d_teach)
        assert v.dedup_stats() == d0   # nothing entered the known-key check
    finally:
        v.close()
    ref = world.v[(k, "reg")]
    world.settle(ref)
    want = world.alone(ref, world.d_teach)
    for key in want:
        assert got[key].tobytes() == want[key].tobytes(), key
    assert (got["verdict"] == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("k", [8, 16])
def test_three_calls_in_flight(world, k):
    """Three calls on three streams, one scratch set and so one pair of root
    rows each; every call's outputs equal that call made alone on the
    register forms."""
    import torch
    from hyperdrive_amd.device import DeviceBatch
    cuts = ((0, 5000), (5000, 10001), (10001, 15100))
    dbs = [DeviceBatch.from_host(_take(world.honest, np.arange(a, b))) for a, b in cuts]
    ref = world.v[(k, "reg")]
    ref.set_variant("dedup", 0)
    world.settle(ref)
    want = [world.alone(ref, d) for d in dbs]
    v = world.v[(k, "two")]
    v.set_variant("dedup", 0)
    world.settle(v)
    with _Form(v, "two", 3):
        outs = [_launch(v, d, "verify", None, st) for d, st in zip(dbs, world.streams)]
        torch.cuda.synchronize()
    for o, w in zip(outs, want):
        h = _host(o)
        for key in w:
            assert h[key].tobytes() == w[key].tobytes(), key
        assert (h["verdict"] == 0).all()


@pytest.mark.gpu
def test_switch_round_trip(world):
    from hyperdrive_amd import _lib
    lib = _lib.load()
    v = world.v[(8, "two")]
    assert v.inv_levels() == 2
    for bad in (0, 3, -2):
        assert lib.hd_ctx_inv_levels(v.handle, bad) == _lib.HD_EINVAL
    assert v.inv_levels(1) == 1 and v.inv_levels() == 1
    assert v.inv_levels(2) == 2 and v.inv_levels() == 2
