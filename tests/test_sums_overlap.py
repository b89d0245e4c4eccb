"""One call's short kernels beside another call's sums (HD_VAR_SUM_CAP,
HD_VAR_SUM_CHAIN, HD_VAR_LEAN_INV; hd_fastverify.hip, DESIGN.md §4 and §5
round 12).

The three variants change where and in which form kernels run, never what a
call returns.  Every GPU case here forces the 3-wave sums (HD_VAR_SUM_WAVES 3:
a small batch picks the 4-wave form, which is neither capped nor chained) and
compares verdict, recovered signatory, signer index and valid bitmap byte for
byte with a context that has all three off, a 512-message sample with the C
oracle, and the repeat and preimage counters of both contexts.  Batches: the
library generator at n = 8,231 with 100 signatories, keys taught beforehand,
13-bit tables.

A call that follows one with many leftovers (a 30 %-adversarial call, a call
that taught keys) runs without the three whatever the variants say, and the
rule reads a figure the device writes.  So every case first makes an honest,
synchronised call, keeps adversarial batches to the last call of a burst, and
asserts from hd_ctx_overlap_stats how many of its calls ran capped, lean and
chained: a case cannot pass on the path without them.
"""
import ctypes
import os
import re

import numpy as np
import pytest

from test_dedup import _host, _launch, _take

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, N_GEN = 100, 8231
# (sum_cap, sum_chain, lean_inv)
COMBOS = {"off": (0, 0, 0), "cap": (1, 0, 0), "chain": (0, 1, 0), "both": (1, 1, 0), "lean": (1, 1, 1)}
ON = [c for c in COMBOS if c != "off"]


# ---- no GPU -----------------------------------------------------------------
def test_variant_keys_and_header():
    """The three keys are the header's, distinct from every other key, below
    HD_VAR__COUNT, and named in the Python binding; a NULL context is
    rejected for them like for any key."""
    from hyperdrive_amd.verify import Verifier
    text = open(os.path.join(ROOT, "include", "hd_verify.h")).read()
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (HD_VAR_\w+) (\d+)", text)}
    assert defs["HD_VAR_SUM_CAP"] == Verifier.VARIANTS["sum_cap"] == 9
    assert defs["HD_VAR_LEAN_INV"] == Verifier.VARIANTS["lean_inv"] == 13
    assert defs["HD_VAR_SUM_CHAIN"] == Verifier.VARIANTS["sum_chain"] == 14
    keys = [v for k, v in defs.items() if k != "HD_VAR__COUNT"]
    assert len(set(keys)) == len(keys) and max(keys) < defs["HD_VAR__COUNT"]
    assert sorted(Verifier.VARIANTS.values()) == sorted(keys)
    # The round trip through hd_ctx_set_variant / hd_ctx_get_variant needs a
    # context, and a context needs a device (hd_ctx_create makes its stream):
    # where one can be created the trip is made here, otherwise only the NULL
    # context's rejection is checked and the trip is
    # test_variant_round_trip_and_rejected_values' (GPU).
    from hyperdrive_amd import _lib
    lib = _lib.load()
    ctx = ctypes.c_void_p()
    made = lib.hd_ctx_create(0, ctypes.byref(ctx)) == 0
    got = ctypes.c_int(-7)
    for key in (9, 13, 14):
        assert lib.hd_ctx_set_variant(None, key, 1) == _lib.HD_EINVAL
        assert lib.hd_ctx_get_variant(None, key, ctypes.byref(got)) == _lib.HD_EINVAL
        if made:
            for value in (0, 1):
                assert lib.hd_ctx_set_variant(ctx, key, value) == 0
                assert lib.hd_ctx_get_variant(ctx, key, ctypes.byref(got)) == 0 and got.value == value
            for bad in (-1, 2):
                assert lib.hd_ctx_set_variant(ctx, key, bad) == _lib.HD_EINVAL
            assert lib.hd_ctx_get_variant(ctx, key, ctypes.byref(got)) == 0 and got.value == 1
    if made:
        assert lib.hd_ctx_destroy(ctx) == 0
    # the keys that existed before keep their numbers
    # (key 2, the sums' prefetch depth, is retired: its number is not reused)
    assert {k: Verifier.VARIANTS[k] for k in ("verify_waves", "sum_waves", "split_k", "recover_g", "key_width",
                                              "wave_prio", "foreign_keys", "slow_lift", "dedup", "pre_share")} == \
        {"verify_waves": 0, "sum_waves": 1, "split_k": 4, "recover_g": 5, "key_width": 7, "wave_prio": 8,
         "foreign_keys": 10, "slow_lift": 11, "dedup": 12, "pre_share": 15}
    assert 2 not in Verifier.VARIANTS.values()


# ---- contexts and batches -----------------------------------------------------
def _context(gpu, combo):
    cap, chain, lean = COMBOS[combo]
    v = gpu.Verifier(0)
    v.set_variant("key_width", 13)
    v.set_variant("foreign_keys", 0)
    v.set_variant("sum_waves", 3)
    v.set_variant("sum_cap", cap)
    v.set_variant("sum_chain", chain)
    v.set_variant("lean_inv", lean)
    return v


def _teach(v, sigs, honest):
    v.set_signatories(sigs)
    res = v.verify_batch(honest)   # one VALID message per signatory teaches its key
    assert (res.verdict == 0).all()
    assert v.known_keys() == S
    # (every message of that call was left to the full recovery: the cases
    # below make an honest call first, see _settle)


class _World:
    def __init__(self, gpu, coracle):
        import torch
        from hyperdrive_amd.device import generate, verify_streams
        self.v = {c: _context(gpu, c) for c in COMBOS}
        self.edge = {c: _context(gpu, c) for c in ("both", "lean")}   # the edge cases' own contexts
        off = self.v["off"]
        self.keys = off.gen_keys(S)
        self.sigs = self.keys[0]
        # seven distinct device batches: 0 honest, 1 30 % adversarial, 2.. honest
        self.db = [generate(off, 0, N_GEN, S, 30 if k == 1 else 0, start=k * N_GEN, keys=self.keys)[0]
                   for k in range(7)]
        self.hb = [d.to_host() for d in self.db]
        for v in list(self.v.values()) + list(self.edge.values()):
            _teach(v, self.sigs, self.hb[0])
        self.streams = verify_streams(None, 3)
        torch.cuda.synchronize()
        # the reference: each batch alone on the context with everything off,
        # checked against the C oracle on a 512-message sample
        self.pick = np.unique(np.linspace(0, N_GEN - 1, 512).astype(np.int64))
        self.ref, self.oracle = [], []
        for d, h in zip(self.db, self.hb):
            out = self.alone(off, d)
            cv, crec = coracle.verify(_take(h, self.pick), self.sigs, True, threads=8)
            assert out["verdict"][self.pick].tolist() == cv.tolist()
            assert out["rec"][self.pick].tobytes() == crec.tobytes()
            self.ref.append(out)
            self.oracle.append((cv, crec))

    def alone(self, v, db, mode="verify", digest=None, stream=None):
        st = self.streams[0] if stream is None else stream
        out = _launch(v, db, mode, digest, st)
        st.synchronize()
        return _host(out)

    def close(self):
        for v in list(self.v.values()) + list(self.edge.values()):
            v.close()


@pytest.fixture(scope="module")
def world(gpu, coracle):
    w = _World(gpu, coracle)
    yield w
    w.close()


def _same(got, want, what):
    for k in want:
        assert got[k].tobytes() == want[k].tobytes(), (what, k)


def _same_as_ref(world, k, got, what):
    _same(got, world.ref[k], what)
    cv, crec = world.oracle[k]
    assert got["verdict"][world.pick].tolist() == cv.tolist(), what
    assert got["rec"][world.pick].tobytes() == crec.tobytes(), what
    bits = np.unpackbits(got["bitmap"].view(np.uint8), bitorder="little")[:len(got["verdict"])]
    assert (bits == (got["verdict"] == 0)).all(), what


class _Path:
    """Asserts which path the calls made inside the block took, from the
    context's overlap counters (hd_ctx_overlap_stats): `calls` calls on the
    variants' path, `waits` of them behind the previous call's sums."""

    def __init__(self, v, combo, calls, waits):
        self.v, self.combo, self.calls, self.waits = v, combo, calls, waits

    def __enter__(self):
        self.before = self.v.overlap_stats()
        return self

    def __exit__(self, *exc):
        if exc[0] is None:
            cap, chain, lean = COMBOS[self.combo]
            got = tuple(x - y for x, y in zip(self.v.overlap_stats(), self.before))
            assert got == (cap * self.calls, lean * self.calls, chain * self.waits), (self.combo, got)


def _settle(world, v, stream=2):
    """Two honest, synchronised calls: after the first the leftover estimate
    the library's path rule reads is 0, so the second takes the variants'
    path and records its sums, and so do the calls that follow for as long
    as only honest calls precede them."""
    world.alone(v, world.db[0], stream=world.streams[stream])
    return world.alone(v, world.db[0], stream=world.streams[stream])


# ---- outputs against the parent path -----------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("combo", ON)
@pytest.mark.parametrize("which", ["honest", "adv30"])
def test_outputs_equal_the_path_with_all_off(world, which, combo):
    k = 0 if which == "honest" else 1
    stats = {}
    for c in (combo, "off"):
        v = world.v[c]
        d0, p0 = v.dedup_stats(), v.preimage_stats()
        for rnd in range(2):
            _settle(world, v)
            with _Path(v, c, 1, 1):   # on the variants' path, behind the settling call's sums
                got = world.alone(v, world.db[k], stream=world.streams[rnd])
            _same_as_ref(world, k, got, (c, which, rnd))
        d1, p1 = v.dedup_stats(), v.preimage_stats()
        stats[c] = (d1[0] - d0[0], d1[1] - d0[1], p1[0] - p0[0], p1[1] - p0[1])
    print(f"{combo} {which}: checked, repeats, typed, distinct preimages {stats[combo]} (all off {stats['off']})")
    assert stats[combo] == stats["off"] and stats[combo][0] > 0 and stats[combo][2] > 0


HONEST = (0, 2, 3, 4, 5, 6)


@pytest.mark.gpu
@pytest.mark.parametrize("combo", ON)
def test_six_calls_over_three_streams(world, combo):
    """Six distinct honest batches with nothing between the calls: every
    scratch set is used twice, and each call's sums waits for the previous
    call's on another stream, so the chain crosses every pair of streams in
    both directions.  Each call's outputs equal that call made alone."""
    import torch
    v = world.v[combo]
    _settle(world, v)
    d0, p0 = v.dedup_stats(), v.preimage_stats()
    with _Path(v, combo, 6, 6):   # (the first call waits for the settling call's sums on stream 2)
        outs = [_launch(v, world.db[k], "verify", None, world.streams[j % 3]) for j, k in enumerate(HONEST)]
        torch.cuda.synchronize()
    d1, p1 = v.dedup_stats(), v.preimage_stats()
    for k, o in zip(HONEST, outs):
        _same_as_ref(world, k, _host(o), (combo, k))
    off = world.v["off"]
    e0, q0 = off.dedup_stats(), off.preimage_stats()
    for k in HONEST:
        world.alone(off, world.db[k])
    e1, q1 = off.dedup_stats(), off.preimage_stats()
    assert (d1[0] - d0[0], d1[1] - d0[1]) == (e1[0] - e0[0], e1[1] - e0[1])
    assert (p1[0] - p0[0], p1[1] - p0[1]) == (q1[0] - q0[0], q1[1] - q0[1])


# ---- the cap alone ------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n", [257, 1023, 8231])
def test_cap_only(world, n):
    """Whole blocks plus a partial one: a reservation that made the launch
    fail, or moved the kernel's digit array, would show here."""
    from hyperdrive_amd.device import DeviceBatch
    db = DeviceBatch.from_host(_take(world.hb[1], np.arange(n)))
    want = world.alone(world.v["off"], db)
    v = world.v["cap"]
    _settle(world, v)
    with _Path(v, "cap", 1, 0):   # the sums was launched with the reservation
        got = world.alone(v, db)
    _same(got, want, n)
    for k in ("verdict", "rec", "signer"):   # a prefix of batch 1: the same messages, the same outputs
        assert got[k].tobytes() == world.ref[1][k][:n].tobytes(), (n, k)
    assert (want["verdict"] == 0).any() and (want["verdict"] != 0).any()


# ---- the chain's edge cases -----------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("combo", ["both", "lean"])
def test_chain_after_a_call_without_an_admitted_set(world, combo):
    """A call with no admitted set launches no sums; the next call, on
    another stream, takes the variants' path and waits for nothing."""
    v = world.edge[combo]
    s0, s1, s2 = world.streams
    _same_as_ref(world, 0, _settle(world, v, 0), "before")
    v.set_signatories(np.zeros((0, 32), np.uint8))
    with _Path(v, combo, 0, 0):
        none = _launch(v, world.db[0], "verify", None, s1)
        s1.synchronize()
    v.set_signatories(world.sigs)
    with _Path(v, combo, 1, 0):
        a = _launch(v, world.db[2], "verify", None, s2)
        s2.synchronize()
    assert (_host(none)["verdict"] == 6).all()   # HD_VERDICT_NOT_ADMITTED
    _same_as_ref(world, 2, _host(a), "after")
    _teach(v, world.sigs, world.hb[0])
    _settle(world, v)
    with _Path(v, combo, 1, 1):   # and the chain goes on from there
        _same_as_ref(world, 3, world.alone(v, world.db[3], stream=s0), "after, second")


@pytest.mark.gpu
@pytest.mark.parametrize("combo", ["both", "lean"])
def test_chain_after_an_invalid_call(world, combo):
    """HD_EINVAL before the call reaches the check: the chain's state is
    untouched, and the next call waits for the sums of the last call that
    launched one (a wait on earlier work, harmless)."""
    from hyperdrive_amd import _lib
    lib = _lib.load()
    v = world.edge[combo]
    s0, s1, s2 = world.streams
    _settle(world, v)
    with _Path(v, combo, 2, 1):   # `first` on the settling call's stream; `after` waits for `first`
        first = _launch(v, world.db[0], "verify", None, s2)
        cs = world.db[1].c_struct()
        assert lib.hd_verify_batch_device(v.handle, ctypes.byref(cs), None, None, None, None,
                                          s1.cuda_stream) == _lib.HD_EINVAL
        after = _launch(v, world.db[1], "verify", None, s0)
        for st in world.streams:
            st.synchronize()
    _same_as_ref(world, 0, _host(first), "before")
    _same_as_ref(world, 1, _host(after), "after")


@pytest.mark.gpu
@pytest.mark.parametrize("combo", ["both", "lean"])
def test_chain_two_calls_on_one_stream(world, combo):
    """Streams 0 0 1 1 0 after a settling call on stream 2: the second call
    of each pair does not wait, the other three do."""
    v = world.edge[combo]
    s0, s1, _ = world.streams
    _settle(world, v)
    plan = ((0, s0), (2, s0), (3, s1), (4, s1), (5, s0))
    with _Path(v, combo, 5, 3):
        outs = [_launch(v, world.db[k], "verify", None, st) for k, st in plan]
        for st in world.streams:
            st.synchronize()
    for (k, _), o in zip(plan, outs):
        _same_as_ref(world, k, _host(o), k)


@pytest.mark.gpu
@pytest.mark.parametrize("combo", ["both", "lean"])
def test_chain_across_set_signatories(world, combo):
    v = world.edge[combo]
    s0, s1, s2 = world.streams
    _settle(world, v)
    with _Path(v, combo, 3, 3):
        a = _launch(v, world.db[0], "verify", None, s0)
        v.set_signatories(world.sigs)   # waits for a; the record of a's sums stays valid
        b = _launch(v, world.db[2], "verify", None, s1)
        c = _launch(v, world.db[1], "verify", None, s2)
        for st in world.streams:
            st.synchronize()
    for k, o in ((0, a), (2, b), (1, c)):
        _same_as_ref(world, k, _host(o), k)


@pytest.mark.gpu
@pytest.mark.parametrize("combo", ["both", "lean"])
def test_chain_with_caller_digests(world, combo):
    """A call with caller digests (k_fast_prep<false>, no preimage kernels)
    between two calls without, each on its own stream."""
    import torch
    from hyperdrive_amd.digest import SHA256, digest_device
    v, off = world.edge[combo], world.v["off"]
    s0, s1, s2 = world.streams
    digest = digest_device(off, SHA256, world.db[2])
    torch.cuda.synchronize()
    want = world.alone(off, world.db[2], mode="digest", digest=digest)
    _settle(world, v)
    with _Path(v, combo, 3, 3):
        a = _launch(v, world.db[0], "verify", None, s0)
        b = _launch(v, world.db[2], "digest", digest, s1)
        c = _launch(v, world.db[1], "verify", None, s2)
        for st in world.streams:
            st.synchronize()
    _same_as_ref(world, 0, _host(a), "before")
    _same(_host(b), want, "digest call")
    _same_as_ref(world, 1, _host(c), "after")


@pytest.mark.gpu
def test_leftovers_and_authentication_keep_the_path_without(world):
    """The library's rule: a call that follows one with more than 1 / 128 of
    its messages left over, and every authentication call, runs without the
    three variants."""
    v = world.v["lean"]
    _settle(world, v)
    with _Path(v, "lean", 1, 1):
        world.alone(v, world.db[1], stream=world.streams[0])   # 30 % adversarial: decided before it ran
    with _Path(v, "lean", 0, 0):
        _same_as_ref(world, 0, world.alone(v, world.db[0], stream=world.streams[1]), "after adversarial")
    with _Path(v, "lean", 1, 0):   # nothing chained before it: the call above recorded no sums
        world.alone(v, world.db[0], stream=world.streams[2])
    with _Path(v, "lean", 0, 0):
        out = _launch(v, world.db[0], "auth", None, world.streams[0])
        world.streams[0].synchronize()
    assert (_host(out)["verdict"] == 0).all()


@pytest.mark.gpu
def test_variant_round_trip_and_rejected_values(world):
    from hyperdrive_amd import _lib
    lib = _lib.load()
    v = world.v["off"]
    for name, key in (("sum_cap", 9), ("lean_inv", 13), ("sum_chain", 14)):
        assert v.variant(name) == 0
        v.set_variant(name, 1)
        assert v.variant(name) == 1
        for bad in (-1, 2, 3):
            assert lib.hd_ctx_set_variant(v.handle, key, bad) == _lib.HD_EINVAL
        assert v.variant(name) == 1
        v.set_variant(name, 0)
        assert v.variant(name) == 0
        assert lib.hd_ctx_set_variant(None, key, 1) == _lib.HD_EINVAL
    for gone in (3, 6):   # keys of variants removed earlier
        assert lib.hd_ctx_set_variant(v.handle, gone, 0) == _lib.HD_EINVAL
    assert lib.hd_ctx_set_variant(v.handle, 16, 0) == _lib.HD_EINVAL
    for c, (cap, chain, lean) in COMBOS.items():
        w = world.v[c]
        assert (w.variant("sum_cap"), w.variant("sum_chain"), w.variant("lean_inv")) == (cap, chain, lean)
        assert w.variant("sum_waves") == 3
