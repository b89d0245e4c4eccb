"""The fixed-base tables the device builds for itself (k_fb_bases / k_fb_runs,
hd_fbtables.hip), read back entry by entry through hd_fb_table_read and
compared with Python integers (tests/fb_table_ref.py), all 64 bytes of every
entry, no tolerance.

The verify tests see a table only through the entries their messages happen
to read (11 of the G table's 8.4e7, 12 to 20 of a key table's, at uniformly
random digits); the entries the builder's walk treats specially are
essentially never among them.  These tests read exactly those: per window
the edge set of fb_table_ref.edge_set (the walk's start, the joins of its
blocks of 32 and its segments of 512, the window's last entries, random d),
on the G table and on per-key tables of every width, with enough keys to
cross the table chunks (8 slots) and, at 22 bits, to send builder lanes into
a second grid-stride pass over their z-ratio scratch."""
import ctypes
import random
import time

import numpy as np
import pytest

import fb_table_ref as R
from util import to_np

pytestmark = pytest.mark.gpu

READY = 3
HD_EINVAL = -1


def _read(v, which, first, count, fill=0xA5):
    """(rc, entries' bytes, width, state, key64) of hd_fb_table_read; the
    output buffer is pre-filled, so a call that copies nothing shows"""
    from hyperdrive_amd import _lib
    lib = _lib.load()
    out = np.full(64 * max(count, 1), fill, np.uint8)
    width, state = ctypes.c_int(-1), ctypes.c_uint32(99)
    key = np.zeros(64, np.uint8)
    rc = lib.hd_fb_table_read(v.handle, which, first, count, out.ctypes.data, ctypes.byref(width),
                              ctypes.byref(state), key.ctypes.data)
    return rc, out.tobytes()[:64 * count], width.value, state.value, key.tobytes()


def _honest(O, keys, idxs):
    """one honest prevote per signer: the full recovery learns each key"""
    b = O.Batch()
    val = O.canonical_value(1, 0)
    dg = O.message_digest(O.PREVOTE, 1, 0, O.INVALID_ROUND, val)
    for k in idxs:
        b.append(O.PREVOTE, 1, 0, O.INVALID_ROUND, val, keys.signatory(k), O.sign(keys.sk(k), dg))
    return b


def _verify_all_valid(O, v, keys, idxs):
    res = v.verify_batch(to_np(_honest(O, keys, idxs)))
    assert res.verdict.tolist() == [O.VALID] * len(idxs)


def _context(gpu, O, keys, width, idxs):
    """(verifier, key indices in the sorted admitted order)"""
    v = gpu.Verifier(0)
    v.set_variant("key_width", width)
    v.set_signatories(np.frombuffer(b"".join(keys.signatory(k) for k in idxs), np.uint8).reshape(len(idxs), 32))
    return v, sorted(idxs, key=keys.signatory)


_pub_cache = {}


def _pub(O, keys, k):
    if k not in _pub_cache:
        _pub_cache[k] = O.pubkey_of(keys.sk(k))
    return _pub_cache[k]


def _check_table(v, which, pub, width, seed, full=False):
    """Compares the edge set (or, full, every entry) of every window of one
    table with the reference; returns (entries compared, the bytes read)."""
    rc, _, w, state, key = _read(v, which, 0, 0)
    assert rc == 0 and state == READY, (which, rc, state)
    assert w == width, (which, w)
    assert key == R.pack(pub), f"table {which}: the slot's key is not the expected public key"
    nwin, n, topbits, tab = R.geometry(w)
    rng = random.Random(seed)
    bases = R.window_bases(pub, w)
    seen, compared, bad = {}, 0, []
    for j in range(nwin):
        dmax = R.window_dmax(w, j)
        ds = range(1, dmax + 1) if full else R.edge_set(w, j, rng)
        runs = R.runs_of(ds)
        if j == nwin - 1:
            assert runs[-1][0] + runs[-1][1] - 1 == 1 << topbits   # the top window's last entry is in
        want = R.expected_runs(bases[j], runs)
        for first, count in runs:
            rc, got, _, _, _ = _read(v, which, j * n + first - 1, count)
            assert rc == 0, (which, j, first, count, rc)
            seen[(j, first)] = got
            compared += count
            if got != want[first]:
                bad += [(j, first + k) for k in range(count) if got[64 * k:64 * k + 64] != want[first][64 * k:64 * k + 64]]
    assert not bad, f"table {which} (W = {w}): {len(bad)} of {compared} entries differ, first (window, d): {bad[:12]}"
    return compared, seen


def test_g_table_edges(gpu, oracle):
    """The shared G table (24-bit windows in the product build): the edge set
    on all 11 windows, the top window's 65,536th entry included."""
    O = oracle
    t0 = time.perf_counter()
    v = gpu.Verifier(0)
    try:
        rc, _, w, state, key = _read(v, -1, 0, 0)
        assert rc == 0 and state == READY and key == R.pack(O.G)
        nwin, n, topbits, tab = R.geometry(w)
        compared, seen = _check_table(v, -1, O.G, w, seed=24)
        assert compared >= 300 * nwin
        if w == 24:
            assert nwin == 11 and (10, 65536 - 65) in seen and len(seen[(10, 65536 - 65)]) == 64 * 66
        # the very last entry of the table, alone: 2^16 2^240 G = 2^256 G
        rc, last, _, _, _ = _read(v, -1, tab - 1, 1)
        assert rc == 0 and last == R.pack(O.point_mul(pow(2, 256, O.N), O.G))
        # accessor errors: a range past the table, an index without a slot
        assert _read(v, -1, tab, 1)[0] == HD_EINVAL
        assert _read(v, -1, tab - 1, 2)[0] == HD_EINVAL
        assert _read(v, -1, 1 << 40, 1)[0] == HD_EINVAL
        assert _read(v, 0, 0, 0)[0] == HD_EINVAL          # no admitted set yet
        assert _read(v, -2, 0, 0)[0] == HD_EINVAL
    finally:
        v.close()
    print(f"fb tables: G W={w} {compared} entries {time.perf_counter() - t0:.2f} s")


def test_key_tables_13bit_whole_tables_across_chunks(gpu, oracle, keys):
    """13-bit windows, 10 keys: the slots cross the 8-slot chunk boundary of
    fb_grow_slots (a fresh context hands slots 1.. out in sorted order: sorted
    index 0 sits in the first chunk, 9 in the second).  Those two tables are
    compared whole (78,336 entries each), the other eight at the edge set."""
    O = oracle
    t0 = time.perf_counter()
    idxs = list(range(10))
    v, order = _context(gpu, O, keys, 13, idxs)
    try:
        _verify_all_valid(O, v, keys, idxs)
        t1 = time.perf_counter()
        total = 0
        for which, k in enumerate(order):
            full = which in (0, 9)
            c, _ = _check_table(v, which, _pub(O, keys, k), 13, seed=1300 + which, full=full)
            assert c == 78336 if full else c >= 20 * 100
            total += c
        # accessor errors on a key table
        tab = R.geometry(13)[3]
        assert _read(v, 0, tab - 1, 1)[0] == 0
        assert _read(v, 0, tab, 1)[0] == HD_EINVAL and _read(v, 0, tab - 5, 6)[0] == HD_EINVAL
        assert _read(v, 10, 0, 0)[0] == HD_EINVAL          # ten admitted: no index 10
    finally:
        v.close()
    print(f"fb tables: W=13 10 keys {total} entries, learn {t1 - t0:.2f} s, check {time.perf_counter() - t1:.2f} s")


def test_key_tables_16bit_two_builds(gpu, oracle, keys):
    """16-bit windows, 10 keys, built by two calls: the first carries
    messages of five signers only -- their tables are READY and right, the
    other five slots report their state and copy nothing.  The second call
    carries everyone: every table holds its edge set, and the first five
    read back byte for byte what they held before the second build."""
    O = oracle
    t0 = time.perf_counter()
    idxs = list(range(10))
    v, order = _context(gpu, O, keys, 16, idxs)
    try:
        first_half = order[0::2]
        _verify_all_valid(O, v, keys, first_half)
        before = {}
        for which, k in enumerate(order):
            if k in first_half:
                _, before[which] = _check_table(v, which, _pub(O, keys, k), 16, seed=1600 + which)
            else:
                rc, got, w, state, key = _read(v, which, 0, 4)
                assert rc == 0 and w == 16 and state != READY and state == 0, (which, rc, state)
                assert got == bytes([0xA5]) * 256 and key == bytes(64)
        _verify_all_valid(O, v, keys, idxs)
        total = 0
        for which, k in enumerate(order):
            c, seen = _check_table(v, which, _pub(O, keys, k), 16, seed=1600 + which)
            total += c
            if which in before:
                assert seen == before[which], f"table {which} changed in a build that was not its own"
    finally:
        v.close()
    print(f"fb tables: W=16 10 keys two builds {total} entries {time.perf_counter() - t0:.2f} s")


def test_key_tables_20bit(gpu, oracle, keys):
    """20-bit windows, 4 keys: the edge set on every key."""
    O = oracle
    t0 = time.perf_counter()
    idxs = list(range(4))
    v, order = _context(gpu, O, keys, 20, idxs)
    try:
        _verify_all_valid(O, v, keys, idxs)
        t1 = time.perf_counter()
        total = sum(_check_table(v, which, _pub(O, keys, k), 20, seed=2000 + which)[0]
                    for which, k in enumerate(order))
    finally:
        v.close()
    print(f"fb tables: W=20 4 keys {total} entries, learn {t1 - t0:.2f} s, check {time.perf_counter() - t1:.2f} s")


def test_key_tables_22bit_second_grid_stride_pass(gpu, oracle, keys):
    """22-bit windows with more segments than builder threads: a base has
    11 x 4096 + 32 segments, k_fb_runs runs 4 x CU count x 256 threads, so
    with S + 2 keys (S the smallest count whose segments exceed the threads;
    6 at 256 CUs) lanes take a second grid-stride pass and reuse their
    z-ratio scratch.  k_fb_list orders the slots by an atomic, so any key may
    be the one reached in the second pass: every key gets the edge set."""
    import torch
    O = oracle
    t0 = time.perf_counter()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    threads = 4 * cus * 256
    nwin, n, topbits, tab = R.geometry(22)
    seg_per_base = (nwin - 1) * (n // R.SEG) + (1 << topbits) // R.SEG
    assert seg_per_base == 11 * 4096 + 32
    S = threads // seg_per_base + 1
    assert S * seg_per_base > threads >= (S - 1) * seg_per_base
    nkeys = S + 2
    assert nkeys * seg_per_base > threads, "no second grid-stride pass: the case would prove nothing"
    idxs = list(range(nkeys))
    v, order = _context(gpu, O, keys, 22, idxs)
    try:
        _verify_all_valid(O, v, keys, idxs)   # one call: one build over all the keys
        t1 = time.perf_counter()
        total = sum(_check_table(v, which, _pub(O, keys, k), 22, seed=2200 + which)[0]
                    for which, k in enumerate(order))
    finally:
        v.close()
    print(f"fb tables: W=22 {cus} CUs {nkeys} keys {total} entries, learn {t1 - t0:.2f} s, "
          f"check {time.perf_counter() - t1:.2f} s")


def test_rekeying_leaves_no_stale_table(gpu, oracle, keys):
    """set_signatories with ten other keys on the same context and width, one
    call: every slot's key is then a new key and its table is that key's --
    no table of the old set survives under a new key."""
    O = oracle
    t0 = time.perf_counter()
    old, new = list(range(10)), list(range(10, 20))
    v, order = _context(gpu, O, keys, 13, old)
    try:
        _verify_all_valid(O, v, keys, old)
        old_keys = set()
        for which, k in enumerate(order):
            rc, _, _, state, key = _read(v, which, 0, 0)
            assert rc == 0 and state == READY and key == R.pack(_pub(O, keys, k))
            old_keys.add(key)
        v.set_signatories(np.frombuffer(b"".join(keys.signatory(k) for k in new), np.uint8).reshape(10, 32))
        order2 = sorted(new, key=keys.signatory)
        for which in range(10):                            # re-mapped: nothing READY, no key, nothing copied
            rc, got, _, state, key = _read(v, which, 0, 1)
            assert rc == 0 and state == 0 and key == bytes(64) and got == bytes([0xA5]) * 64
        _verify_all_valid(O, v, keys, new)
        total = 0
        for which, k in enumerate(order2):
            c, _ = _check_table(v, which, _pub(O, keys, k), 13, seed=1350 + which)
            assert _read(v, which, 0, 0)[4] not in old_keys
            total += c
    finally:
        v.close()
    print(f"fb tables: W=13 re-keyed 10 keys {total} entries {time.perf_counter() - t0:.2f} s")
