"""A set change that re-tiers the key tables keeps the known keys (fb_map in
hd_fbtables.hip, the plan of hd_keycarry.h, k_key_gather / k_key_carry in
hd_keyimport.hip), on the GPU.

Width arithmetic the cases rest on (fb_pick_width, fb_slot_bytes):
a slot costs 64 B per table entry, 72 B per window base and key, 8 B of state
and pointer --
    20-bit: 64 * 6,356,992 + 72 * 14 + 8 = 4.068e8 B, picked when 4.068e8 (m + 1) <= budget
    16-bit: 64 *   557,056 + 72 * 17 + 8 = 3.565e7 B, picked when 3.565e7 (m + 1 + F) <= budget,
            F = the foreign_keys variant (16 by default)
    13-bit: 64 *    78,336 + 72 * 21 + 8 = 5.015e6 B, otherwise.
The 16 <-> 13 decision reads the context's own budget only, not what other
contexts of the process hold, so the cases sit on that boundary.
HD_FB_MAX_BYTES = 2e9: m = 4 fails the 20-bit rule (2.03e9), and 3.565e7 (m + 17)
<= 2e9 holds up to m = 39: 4 <= m <= 39 takes 16 bits (16 key windows), m >= 40
takes 13 bits (20 key windows).  HD_FB_MAX_BYTES = 2e8 with foreign_keys 0:
m = 4 takes 16 bits (1.78e8), m = 50 takes 13 bits with floor(2e8 / 5.015e6) =
39 slots, slot 0 reserved: 38 signatories get one.  Every case asserts its
pick through fastpath_geometry()[1] before it relies on it.

The reference of every output is a context with the fast path off."""
import ctypes
import random

import numpy as np
import pytest

import fb_table_ref as R

pytestmark = pytest.mark.gpu

N = 4001                 # a partial last wave
READY = 3
VALID, NOT_ADMITTED, NOT_AUTHENTIC = 0, 6, 8
W16, W13 = 16, 20        # key windows of the 16-bit and the 13-bit tables


def _run(v, db, n):
    """[verdict, signer, recovered, bitmap] of one verify_batch_device call"""
    import torch
    from hyperdrive_amd.device import work_stream
    ws = work_stream()
    outs = [torch.empty(n, dtype=torch.uint8, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda"),
            torch.empty((n, 32), dtype=torch.uint8, device="cuda"),
            torch.zeros((n + 31) // 32, dtype=torch.int32, device="cuda")]
    v.verify_batch_device(db.c_struct(), outs[0].data_ptr(), outs[2].data_ptr(), outs[1].data_ptr(),
                          outs[3].data_ptr(), ws.cuda_stream)
    ws.synchronize()
    return outs


def _auth(v, db, n):
    """verdict bytes of one authenticate_batch_device call"""
    import torch
    from hyperdrive_amd.device import work_stream
    ws = work_stream()
    out = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
    v.authenticate_batch_device(db.c_struct(), out.data_ptr(), ws.cuda_stream)
    ws.synchronize()
    return out.cpu().numpy()


def _same(a, b):
    import torch
    return all(torch.equal(x, y) for x, y in zip(a, b))


def _rows(a):
    return [bytes(r) for r in np.asarray(a)]


def _export(v, sigs):
    """{signatory: key64} of the known rows of export_keys, the unknown rows
    checked to be all zero; sigs: the array last given to set_signatories"""
    keys, known = v.export_keys()
    assert len(keys) == len(sigs)
    assert not keys[~known].any()
    return {s: bytes(k) for s, k, kn in zip(_rows(sigs), keys, known) if kn}


def _info(v):
    i = v.last_set_change()
    return i["width_before"], i["width_after"], i["kept"], i["carried"], i["dropped"]


def _ref(sigs, db, n, fmt=True):
    """the full recovery's outputs for one admitted set and batch"""
    from hyperdrive_amd.verify import Verifier
    slow = Verifier(0, compressed=fmt)
    try:
        slow.set_fastpath(False)
        slow.set_signatories(sigs)
        return _run(slow, db, n)
    finally:
        slow.close()


_narrow = {}


def _narrowing_world():
    """Shared by cases 1, 3 and 6, computed once and left unchanged: 60 keys;
    the new set (the 30 old signatories in shuffled caller order, then the 30
    new ones); a batch of the 30 old signers and one of all 60; the full
    recovery's outputs for both against the new set, and for the old batch
    against the old set."""
    if not _narrow:
        from hyperdrive_amd.device import generate
        from hyperdrive_amd.verify import Verifier
        g = Verifier(0)
        try:
            sigs, foreign = g.gen_keys(60)
            old = sigs[:30].copy()
            order = list(range(30))
            random.Random(16).shuffle(order)
            new = np.concatenate([old[order], sigs[30:]])
            db_old, _, _ = generate(g, 0, N, 30, 10, keys=(old, foreign), start=1613)
            db_all, _, _ = generate(g, 0, N, 60, 10, keys=(sigs, foreign), start=1316)
        finally:
            g.close()
        _narrow.update(old=old, new=new, db_old=db_old, db_all=db_all, ref_old_at_old=_ref(old, db_old, N),
                       ref_old=_ref(new, db_old, N), ref_all=_ref(new, db_all, N))
    return _narrow


def _learn_30_then_narrow(v, w):
    """case 1's steps up to the set change: 30 keys learned at 16 bits with
    two verify calls, exported, then the set of 60 (13 bits)"""
    v.set_signatories(w["old"])
    assert v.fastpath_geometry()[1] == W16
    for _ in range(2):
        assert _same(w["ref_old_at_old"], _run(v, w["db_old"], N))
    assert v.known_keys() == 30
    before = _export(v, w["old"])
    assert sorted(before) == sorted(_rows(w["old"]))
    v.set_signatories(w["new"])
    assert v.fastpath_geometry()[1] == W13
    return before


# ---- 1: narrowing ---------------------------------------------------------------
def test_narrowing_keeps_the_known_keys(gpu, monkeypatch):
    """16 -> 13 bits (30 -> 60 signatories at a 2e9 budget).  Without the carry
    the first known_keys() after the set change is 0: the re-tier freed every
    table and forgot every key."""
    from hyperdrive_amd.verify import Verifier
    monkeypatch.setenv("HD_FB_MAX_BYTES", str(2e9))
    w = _narrowing_world()
    v = Verifier(0)
    try:
        before = _learn_30_then_narrow(v, w)
        # no verify call in between
        assert v.known_keys() == 30
        assert _export(v, w["new"]) == before          # exactly the 30 old ones, with their keys
        assert _info(v) == (16, 13, 0, 30, 0)
        # the old signers' batch: the known-key path from the first call on
        assert _same(w["ref_old"], _run(v, w["db_old"], N))
        fallback, invalid = v.fastpath_stats()[1], int((w["ref_old"][0] != VALID).sum())
        print(f"first call after the carry: fallback {fallback} of {N} (non-VALID {invalid})")
        assert fallback <= invalid
        for _ in range(2):
            assert _same(w["ref_all"], _run(v, w["db_all"], N))
        assert v.known_keys() == 60
        # an unchanged width leaves everything in place
        v.set_signatories(w["new"][::-1].copy())
        assert _info(v) == (13, 13, 60, 0, 0) and v.known_keys() == 60
    finally:
        v.close()


# ---- 2: widening ----------------------------------------------------------------
def _table(v, which, first, count):
    from hyperdrive_amd import _lib
    lib = _lib.load()
    out = np.full(64 * max(count, 1), 0xA5, np.uint8)
    width, state = ctypes.c_int(-1), ctypes.c_uint32(99)
    key = np.zeros(64, np.uint8)
    rc = lib.hd_fb_table_read(v.handle, which, first, count, out.ctypes.data, ctypes.byref(width), ctypes.byref(state),
                              key.ctypes.data)
    assert rc == 0, (which, first, count, rc)
    return out.tobytes()[:64 * count], width.value, state.value, key.tobytes()


@pytest.mark.parametrize("fmt", [True, 3])
def test_widening_rebuilds_the_tables(gpu, monkeypatch, fmt):
    """13 -> 16 bits (60 -> every second signatory in sorted order).  The
    carried keys' 16-bit tables equal those of a context that learned the same
    30 keys at 16 bits: two of them whole (557,056 entries), the others at the
    edge set of fb_table_ref (the builder walk's starts, joins and ends)."""
    from hyperdrive_amd.device import generate
    from hyperdrive_amd.verify import Verifier
    monkeypatch.setenv("HD_FB_MAX_BYTES", str(2e9))
    A, B = Verifier(0, compressed=fmt), Verifier(0, compressed=fmt)
    try:
        sigs, foreign = A.gen_keys(60)
        db, _, _ = generate(A, 0, N, 60, 10, keys=(sigs, foreign), start=1361)
        in_order = sorted(_rows(sigs))[::2]
        half = np.frombuffer(b"".join(in_order), np.uint8).reshape(30, 32).copy()
        ref60, ref30 = _ref(sigs, db, N, fmt), _ref(half, db, N, fmt)
        A.set_signatories(sigs)
        assert A.fastpath_geometry()[1] == W13
        for _ in range(2):
            assert _same(ref60, _run(A, db, N))
        assert A.known_keys() == 60
        before = _export(A, sigs)
        A.set_signatories(half)
        assert A.fastpath_geometry()[1] == W16
        assert A.known_keys() == 30                      # at once
        assert _info(A) == (13, 16, 0, 30, 30)
        assert _export(A, half) == {s: before[s] for s in _rows(half)}
        # B learns the same 30 keys at 16 bits
        B.set_signatories(half)
        assert B.fastpath_geometry()[1] == W16
        for _ in range(2):
            assert _same(ref30, _run(B, db, N))
        assert B.known_keys() == 30
        nwin, n, topbits, tab = R.geometry(16)
        assert tab == 557056
        rng = random.Random(1316)
        for which in range(30):                          # (sorted index: the same signatory in A and B)
            _, wa, sa, ka = _table(A, which, 0, 0)
            _, wb, sb, kb = _table(B, which, 0, 0)
            assert (wa, sa) == (wb, sb) == (16, READY), which
            key = before[in_order[which]]                # X || Y big-endian; a table entry is little-endian
            assert ka == kb == key[:32][::-1] + key[32:][::-1], which
            if which in (0, 29):
                assert _table(A, which, 0, tab)[0] == _table(B, which, 0, tab)[0], f"table {which} differs"
                continue
            for j in range(nwin):
                for first, count in R.runs_of(R.edge_set(16, j, rng)):
                    ta = _table(A, which, j * n + first - 1, count)[0]
                    tb = _table(B, which, j * n + first - 1, count)[0]
                    assert ta == tb, f"table {which} window {j} entries {first}..{first + count - 1} differ"
        assert _same(ref30, _run(A, db, N))
    finally:
        A.close()
        B.close()


# ---- 3: authenticate after a carry ----------------------------------------------
def test_authenticate_after_a_carry(gpu, monkeypatch):
    """hd_authenticate_batch_device trusts a known key: a wrong carried key
    would make honest messages NOT_AUTHENTIC.  Right after case 1's set change
    every row the reference calls VALID or NOT_ADMITTED has that verdict, and
    the rows of the 30 old signers equal those of a context warmed by verify
    calls at the same set.  (Rows of the 30 new signers that are not VALID
    differ in that first call by design: without a known key they take the
    full recovery, which names their class instead of NOT_AUTHENTIC.)  The
    first call learns the new signers' keys; the second call's output equals
    the warmed context's whole."""
    from hyperdrive_amd.verify import Verifier
    monkeypatch.setenv("HD_FB_MAX_BYTES", str(2e9))
    w = _narrowing_world()
    v, warm = Verifier(0), Verifier(0)
    try:
        warm.set_signatories(w["new"])
        assert warm.fastpath_geometry()[1] == W13
        for _ in range(2):
            assert _same(w["ref_all"], _run(warm, w["db_all"], N))
        assert warm.known_keys() == 60
        want = _auth(warm, w["db_all"], N)
        _learn_30_then_narrow(v, w)
        assert v.known_keys() == 30
        got = _auth(v, w["db_all"], N)
        ref = w["ref_all"][0].cpu().numpy()
        final = (ref == VALID) | (ref == NOT_ADMITTED)
        assert final.sum() > N // 2
        bad = np.flatnonzero(final & (got != ref))
        assert not len(bad), f"rows {bad[:8]}: {got[bad[:8]]} for the reference's {ref[bad[:8]]}"
        assert not (got[~final] == VALID).any() and not (got[~final] == NOT_ADMITTED).any()
        old = set(_rows(w["old"]))
        from_old = np.array([f in old for f in _rows(w["db_all"].to_host().frm)])
        assert from_old.sum() > N // 4 and np.array_equal(got[from_old], want[from_old])
        assert (want == NOT_AUTHENTIC).sum() > 0 and not (got[final] == NOT_AUTHENTIC).any()
        assert np.array_equal(_auth(v, w["db_all"], N), want)
    finally:
        v.close()
        warm.close()


# ---- 4: the retry with replaced signatories (the hazard) ------------------------
def test_failed_grow_carries_from_the_snapshot(gpu, monkeypatch):
    """30 keys at 16 bits fill 1 + 30 + 16 = 47 slots: six chunks of 8, 48
    slots with tables.  The new set drops 5 and adds 7: the freed 5 slots and 2
    more, 49 slots, one more chunk -- which HD_FB_FAIL_WIDTH refuses at 16
    bits.  That failed attempt has handed the 5 freed slots, states still READY
    with the departed keys, to new signatories; the retry at 13 bits must carry
    from the snapshot taken before it: 25 keys, each its own signatory's, and
    nothing for the 7 new ones."""
    from hyperdrive_amd.device import generate
    from hyperdrive_amd.verify import Verifier
    monkeypatch.setenv("HD_FB_MAX_BYTES", str(2e9))
    v = Verifier(0)
    try:
        sigs, foreign = v.gen_keys(37)
        old = sigs[:30].copy()
        new = np.concatenate([sigs[:25], sigs[30:]])
        db_old, _, _ = generate(v, 0, N, 30, 10, keys=(old, foreign), start=2516)
        db_all, _, _ = generate(v, 0, N, 37, 10, keys=(sigs, foreign), start=2513)
        ref_old, ref = _ref(old, db_old, N), _ref(new, db_all, N)
        v.set_signatories(old)
        assert v.fastpath_geometry()[1] == W16
        for _ in range(2):
            assert _same(ref_old, _run(v, db_old, N))
        assert v.known_keys() == 30
        before = _export(v, old)
        monkeypatch.setenv("HD_FB_FAIL_WIDTH", "16")
        v.set_signatories(new)
        monkeypatch.delenv("HD_FB_FAIL_WIDTH")
        assert v.fastpath_geometry()[1] == W13
        assert v.known_keys() == 25
        assert _export(v, new) == {s: before[s] for s in _rows(sigs[:25])}     # the 7 new: unknown, all zero
        assert _info(v) == (16, 13, 0, 25, 5)
        got = _auth(v, db_all, N)
        r = ref[0].cpu().numpy()
        final = (r == VALID) | (r == NOT_ADMITTED)
        assert (r == VALID).sum() > N // 2 and (r == NOT_ADMITTED).sum() > N // 20    # signers 25..29 left
        bad = np.flatnonzero(final & (got != r))
        assert not len(bad), f"rows {bad[:8]}: {got[bad[:8]]} for the reference's {r[bad[:8]]}"
        assert not (got[~final] == VALID).any() and not (got[~final] == NOT_ADMITTED).any()
        for _ in range(2):
            assert _same(ref, _run(v, db_all, N))
        assert v.known_keys() == 32
    finally:
        v.close()


# ---- 5: slot priority -----------------------------------------------------------
def test_carried_keys_take_slots_first(gpu, monkeypatch):
    """2e8 bytes, no foreign block: the last four signatories, in sorted order,
    of a set of 50 are learned as a set of their own (16 bits); the set of 50
    takes 13 bits with 38 slots for signatories.  In sorted order alone the
    four would get none; carried keys take slots first."""
    from hyperdrive_amd.device import generate
    from hyperdrive_amd.verify import Verifier
    monkeypatch.setenv("HD_FB_MAX_BYTES", str(2e8))
    v = Verifier(0)
    try:
        v.set_variant("foreign_keys", 0)
        sigs, foreign = v.gen_keys(50)
        db, _, _ = generate(v, 0, N, 50, 10, keys=(sigs, foreign), start=5038)
        last4 = np.frombuffer(b"".join(sorted(_rows(sigs))[-4:]), np.uint8).reshape(4, 32).copy()
        ref4, ref50 = _ref(last4, db, N), _ref(sigs, db, N)
        v.set_signatories(last4)
        assert v.fastpath_geometry()[1] == W16
        for _ in range(2):
            assert _same(ref4, _run(v, db, N))
        assert v.known_keys() == 4
        before = _export(v, last4)
        v.set_signatories(sigs)
        assert v.fastpath_geometry()[1] == W13
        assert v.known_keys() == 4                       # at once
        assert _info(v) == (16, 13, 0, 4, 0)
        assert _export(v, sigs) == before
        for _ in range(2):
            assert _same(ref50, _run(v, db, N))
        assert v.known_keys() == 38
    finally:
        v.close()


# ---- 6: hd_multi ----------------------------------------------------------------
def test_multi_set_change_carries_on_every_context(gpu, monkeypatch):
    from hyperdrive_amd.multi import MultiVerifier
    monkeypatch.setenv("HD_FB_MAX_BYTES", str(2e9))
    w = _narrowing_world()
    hb_old, hb_all = w["db_old"].to_host(), w["db_all"].to_host()
    m = MultiVerifier([0, 0])

    def check(hb, ref):
        res, _ = m.process_batch(hb, tally=False)
        assert np.array_equal(res.verdict, ref[0].cpu().numpy())
        assert np.array_equal(res.recovered, ref[2].cpu().numpy())
        assert np.array_equal(res.valid_bitmap, ref[3].cpu().numpy().view(np.uint32))

    try:
        m.set_signatories(w["old"])
        for _ in range(2):
            check(hb_old, w["ref_old_at_old"])
        assert [m.fastpath_stats(k)[0] for k in (0, 1)] == [30, 30]
        keys, known = m.export_keys()
        assert known.all()
        before = dict(zip(_rows(w["old"]), _rows(keys)))
        m.set_signatories(w["new"])
        assert [m.fastpath_stats(k)[0] for k in (0, 1)] == [30, 30]
        for k in (0, 1):
            i = m.last_set_change(k)
            assert (i["width_before"], i["width_after"], i["kept"], i["carried"], i["dropped"]) == (16, 13, 0, 30, 0)
        keys, known = m.export_keys()
        assert {s: k for s, k, kn in zip(_rows(w["new"]), _rows(keys), known) if kn} == before
        check(hb_old, w["ref_old"])
        for _ in range(2):
            check(hb_all, w["ref_all"])
        assert [m.fastpath_stats(k)[0] for k in (0, 1)] == [60, 60]
    finally:
        m.close()
