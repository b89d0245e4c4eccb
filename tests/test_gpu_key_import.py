"""hd_import_keys / hd_export_keys on the GPU (hd_keyimport.hip).

An import may change no output: a context that imported its keys must give,
from its first call on, what a context that learned them gives and what the
full recovery alone gives -- verdicts, recovered signatories, signers, bitmap
-- with tables equal byte for byte.  What it buys is the first call's path:
its fallback count is bounded by the non-VALID messages, the bound
test_fast_path_equals_full_recovery puts on its SECOND pass (without an
import the first pass falls back for every typed message).

Tables are forced to 13-bit windows (5 MB per key) through HD_FB_PW, as
test_key_table_widths_equal_full_recovery forces a width, except in the one
test at the default width."""
import ctypes

import numpy as np
import pytest

import fb_table_ref as R
import key_import_cases as C

pytestmark = pytest.mark.gpu

S, N = 10, 5003          # ten keys cross the 8-slot table chunk; 5,003: a partial last wave
READY = 3


@pytest.fixture(autouse=True)
def _width13(request, monkeypatch):
    if request.node.name != "test_oracle_keys_at_the_default_width":
        monkeypatch.setenv("HD_FB_PW", "13")


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


def _same(a, b):
    import torch
    return all(torch.equal(x, y) for x, y in zip(a, b))


_worlds = {}


def _world(fmt, s=S):
    """Per pubkey format, computed once and left unchanged: the keys, the
    batch, the full recovery's outputs, and what context A -- which learned
    its keys from a first verify call -- knows and exports."""
    if (fmt, s) not in _worlds:
        from hyperdrive_amd.device import generate
        from hyperdrive_amd.verify import Verifier
        A, slow = Verifier(0, compressed=fmt), Verifier(0, compressed=fmt)
        try:
            slow.set_fastpath(False)
            ks = A.gen_keys(s)
            db, _, _ = generate(A, 0, N, s, 30, keys=ks, start=4242)
            A.set_signatories(ks[0])
            slow.set_signatories(ks[0])
            ref = _run(slow, db, N)
            assert A.known_keys() == 0
            assert _same(ref, _run(A, db, N))
            keys, known = A.export_keys()
            assert known.all() and A.known_keys() == s     # every signer has a VALID message
            _worlds[(fmt, s)] = dict(ks=ks, db=db, ref=ref, keys=keys, known_keys=A.known_keys(),
                                     fallback_first=A.fastpath_stats()[1], n_invalid=int((ref[0] != 0).sum()))
        finally:
            A.close()
            slow.close()
    return _worlds[(fmt, s)]


def _read(v, which, count):
    """(entries' bytes, width, state, key64) of hd_fb_table_read from entry 0"""
    from hyperdrive_amd import _lib
    lib = _lib.load()
    out = np.full(64 * max(count, 1), 0xA5, np.uint8)
    width, state = ctypes.c_int(-1), ctypes.c_uint32(99)
    key = np.zeros(64, np.uint8)
    rc = lib.hd_fb_table_read(v.handle, which, 0, count, out.ctypes.data, ctypes.byref(width), ctypes.byref(state),
                              key.ctypes.data)
    assert rc == 0
    return out.tobytes()[:64 * count], width.value, state.value, key.tobytes()


def _first_call_is_warm(B, w):
    """B's first verify call: the full recovery's outputs, on the known-key path"""
    assert _same(w["ref"], _run(B, w["db"], N))
    fallback = B.fastpath_stats()[1]
    print(f"first call: fallback {fallback} of {N} (non-VALID {w['n_invalid']}; a cold first call: {w['fallback_first']})")
    assert fallback <= w["n_invalid"]


# ---- 1: import equals learning ----------------------------------------------
@pytest.mark.parametrize("fmt", C.FORMATS)
def test_import_equals_learning(gpu, fmt):
    from hyperdrive_amd.verify import Verifier
    w = _world(fmt)
    assert w["fallback_first"] >= N - int((w["ref"][0] == 7).sum())     # A started cold
    B = Verifier(0, compressed=fmt)
    try:
        B.set_signatories(w["ks"][0])
        status, signer = B.import_keys(w["keys"])
        assert B.known_keys() == w["known_keys"] == S
        assert status.tolist() == [C.IMPORTED] * S
        assert signer.tolist() == list(range(S))
        _first_call_is_warm(B, w)
        keys, known = B.export_keys()
        assert known.all() and np.array_equal(keys, w["keys"])
    finally:
        B.close()


# ---- 2: tables byte for byte -------------------------------------------------
def test_imported_tables_equal_learned_tables(gpu):
    from hyperdrive_amd.verify import Verifier
    w = _world(1)
    tab = R.geometry(13)[3]
    A, B = Verifier(0), Verifier(0)
    try:
        for v in (A, B):
            v.set_signatories(w["ks"][0])
        _run(A, w["db"], N)                      # A learns
        B.import_keys(w["keys"])                 # B is told
        for which in range(S):
            ta, wa, sa, ka = _read(A, which, tab)
            tb, wb, sb, kb = _read(B, which, tab)
            assert (wa, sa) == (wb, sb) == (13, READY), which
            assert ka == kb and ka != bytes(64), which
            assert ta == tb, f"table {which} differs"
    finally:
        A.close()
        B.close()


# ---- 3: statuses on the device ----------------------------------------------
def _status_rows(n):
    """n rows, honest and bad interleaved (every wave holds both); past 34
    rows the keys repeat"""
    honest = [C.enc(*C.pub(i)) for i in range(6)] + [C.enc(*C.pub(C.SIGNER_X0)), C.enc(*C.pub(C.SIGNER_Y0)),
                                                      C.enc(*C.pub_both())]
    bad = [r for _, r in C.bad_rows(0)] + [C.enc(*C.pub(7))]      # signer 7: a valid key, not admitted
    return honest, [honest[(k // 2) % len(honest)] if k % 2 == 0 else bad[(k // 2) % len(bad)] for k in range(n)]


@pytest.mark.parametrize("fmt", C.FORMATS)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 200])
def test_statuses_equal_the_host_program(gpu, n, fmt):
    from hyperdrive_amd.verify import Verifier
    honest, rows = _status_rows(n)
    sigs = [C.sig_of(int.from_bytes(h[:32], "big"), int.from_bytes(h[32:], "big"), fmt) for h in honest]
    want = C.run_check(C.build_check(sanitize=False), [(fmt, sigs, True, rows)])
    assert want == [C.expect(r, fmt, sigs) for r in rows]
    if n >= 63:
        assert {s for s, _ in want} == {C.IMPORTED, C.NOT_ADMITTED, C.BAD_POINT}
    v = Verifier(0, compressed=fmt)
    try:
        v.set_signatories(sigs)
        status, signer = v.import_keys(rows)
        assert list(zip(status.tolist(), signer.tolist())) == want
        distinct = len({r for r, (s, _) in zip(rows, want) if s == C.IMPORTED})
        assert v.known_keys() == distinct
        count = R.geometry(13)[3] if fmt == 1 else 0
        before = [_read(v, which, count) for which in range(len(sigs))]
        status2, signer2 = v.import_keys(rows)
        assert status2.tolist() == [C.KNOWN if s == C.IMPORTED else s for s, _ in want]
        assert signer2.tolist() == signer.tolist()
        assert v.known_keys() == distinct
        assert [_read(v, which, count) for which in range(len(sigs))] == before
    finally:
        v.close()


def test_argument_errors(gpu):
    from hyperdrive_amd import _lib
    from hyperdrive_amd.verify import Verifier
    lib = _lib.load()
    v = Verifier(0)
    try:
        st = np.zeros(1, np.uint8)
        key = np.zeros(64, np.uint8)
        n = ctypes.c_uint32(77)
        assert lib.hd_import_keys(v.handle, None, 1, st.ctypes.data, None) == -1
        assert lib.hd_import_keys(v.handle, key.ctypes.data, 1, None, None) == -1
        assert lib.hd_import_keys(v.handle, None, 0, None, None) == 0
        assert lib.hd_export_keys(v.handle, None, None, 0, ctypes.byref(n)) == 0 and n.value == 0
        v.set_signatories(_world(1)["ks"][0])
        assert lib.hd_export_keys(v.handle, None, None, S - 1, ctypes.byref(n)) == -4 and n.value == S
        assert lib.hd_abi_version() == 2
    finally:
        v.close()


# ---- 4: keys from the oracle, default width ----------------------------------
def test_oracle_keys_at_the_default_width(gpu):
    """The public keys derived in Python from the generator's seeds, not taken
    from an export, at the width the context picks itself."""
    from hyperdrive_amd.verify import Verifier
    s = 7
    w = _world(1, s)
    B = Verifier(0)
    try:
        B.set_signatories(w["ks"][0])
        status, signer = B.import_keys([C.enc(*C.pub(i)) for i in range(s)])
        assert status.tolist() == [C.IMPORTED] * s and signer.tolist() == list(range(s))
        assert B.known_keys() == s
        assert B.variant("key_width") == 0                   # the width is the context's own pick
        _first_call_is_warm(B, w)
    finally:
        B.close()


# ---- 5: the authenticate path ------------------------------------------------
def test_authenticate_after_import(gpu):
    import torch
    from hyperdrive_amd.device import work_stream
    from hyperdrive_amd.verify import Verifier
    w = _world(1)
    B, W = Verifier(0), Verifier(0)
    try:
        outs = []
        for v in (B, W):
            v.set_signatories(w["ks"][0])
        B.import_keys(w["keys"])
        _run(W, w["db"], N)                      # W is warmed by a verify call
        ws = work_stream()
        for v in (B, W):
            out = torch.full((N,), 255, dtype=torch.uint8, device="cuda")
            v.authenticate_batch_device(w["db"].c_struct(), out.data_ptr(), ws.cuda_stream)
            ws.synchronize()
            outs.append(out.cpu().numpy())
        ref = w["ref"][0].cpu().numpy()
        auth = np.isin(ref, (0, 6))
        assert auth.sum() > N // 2 and (ref == 6).sum() > 0
        for got in outs:
            assert (got[auth] == ref[auth]).all()          # honest rows: VALID / NOT_ADMITTED, never NOT_AUTHENTIC
            assert not np.isin(got[~auth], (0, 6)).any()
        assert (outs[0][auth] == outs[1][auth]).all()
        assert B.fastpath_stats()[1] <= w["n_invalid"]
    finally:
        B.close()
        W.close()


# ---- 6: state changes ----------------------------------------------------------
def test_partial_import_set_change_and_format_change(gpu):
    from hyperdrive_amd.verify import Verifier
    w = _world(1)
    sigs = w["ks"][0]
    v = Verifier(0)
    try:
        v.set_signatories(sigs)
        status, signer = v.import_keys(w["keys"][:5])
        assert status.tolist() == [C.IMPORTED] * 5 and signer.tolist() == [0, 1, 2, 3, 4]
        keys, known = v.export_keys()
        assert known.tolist() == [True] * 5 + [False] * 5
        assert np.array_equal(keys[:5], w["keys"][:5]) and not keys[5:].any()
        assert _same(w["ref"], _run(v, w["db"], N))          # the other five are learned
        keys, known = v.export_keys()
        assert known.all() and np.array_equal(keys, w["keys"])
        # a reordered set with a duplicate entry, one signatory gone and a stranger
        order = [9, 3, 3, 0, 7, 1, 8, 2, 6, 4]
        re = np.concatenate([sigs[order], np.frombuffer(C.filler(0), np.uint8).reshape(1, 32)])
        v.set_signatories(re)
        assert v.known_keys() == 9                           # kept, READY: imported and learned alike
        keys, known = v.export_keys()
        assert known.tolist() == [True] * 10 + [False]
        assert np.array_equal(keys[:10], w["keys"][order]) and not keys[10].any()
        status, signer = v.import_keys(w["keys"])
        assert status.tolist() == [C.KNOWN] * 5 + [C.NOT_ADMITTED] + [C.KNOWN] * 4
        assert signer.tolist() == [3, 5, 7, 1, 9, -1, 8, 4, 6, 0]
        # another pubkey format: every key is dropped; the same raw keys import again
        v.set_pubkey_format(2)
        keys, known = v.export_keys()
        assert not known.any() and not keys.any() and v.known_keys() == 0
        w2 = _world(2)
        v.set_signatories(w2["ks"][0])
        status, signer = v.import_keys(w["keys"])
        assert status.tolist() == [C.IMPORTED] * S and signer.tolist() == list(range(S))
        assert np.array_equal(w2["keys"], w["keys"])         # one key pair per signer, whatever the format
        _first_call_is_warm(v, w2)
    finally:
        v.close()


def test_no_slot_when_the_mapping_failed_or_the_fast_path_is_off(gpu, monkeypatch):
    from hyperdrive_amd import _lib
    from hyperdrive_amd.verify import Verifier
    w = _world(1)
    failed, off = Verifier(0), Verifier(0)
    try:
        monkeypatch.setenv("HD_FB_FAIL_WIDTH", "13")
        failed.set_variant("key_width", 13)                  # a forced width is not retried narrower
        with pytest.raises(_lib.HDError):
            failed.set_signatories(w["ks"][0])
        monkeypatch.delenv("HD_FB_FAIL_WIDTH")
        off.set_signatories(w["ks"][0])
        off.set_fastpath(False)
        for v in (failed, off):
            status, signer = v.import_keys(w["keys"])
            assert status.tolist() == [C.NO_SLOT] * S and signer.tolist() == list(range(S))
            assert v.known_keys() == 0
            assert _same(w["ref"], _run(v, w["db"], N))
    finally:
        failed.close()
        off.close()


def test_ingress_reset_height_imports(gpu):
    from hyperdrive_amd.ingress import Ingress
    from hyperdrive_amd.verify import Verifier
    w = _world(1)
    v = Verifier(0)
    try:
        ing = Ingress(v, height=1)
        assert ing.reset_height(2, w["ks"][0], keys=w["keys"])
        assert v.known_keys() == S
        keys, known = ing.export_keys()
        assert known.all() and np.array_equal(keys, w["keys"])
    finally:
        v.close()


# ---- 7: hd_multi ---------------------------------------------------------------
def test_multi_import(gpu):
    from hyperdrive_amd.multi import MultiVerifier
    w = _world(1)
    hb = w["db"].to_host()
    m = MultiVerifier([0, 0])
    try:
        m.set_signatories(w["ks"][0])
        status, signer = m.import_keys(w["keys"])
        assert status.tolist() == [C.IMPORTED] * S and signer.tolist() == list(range(S))
        assert [m.fastpath_stats(k)[0] for k in (0, 1)] == [S, S]
        res, _ = m.process_batch(hb, tally=False)
        ref = w["ref"]
        assert np.array_equal(res.verdict, ref[0].cpu().numpy())
        assert np.array_equal(res.recovered, ref[2].cpu().numpy())
        assert np.array_equal(res.valid_bitmap, ref[3].cpu().numpy().view(np.uint32))
        for k in (0, 1):
            assert m.fastpath_stats(k)[1] <= w["n_invalid"]
        keys, known = m.export_keys()
        assert known.all() and np.array_equal(keys, w["keys"])
    finally:
        m.close()
