"""hd_import_keys' row check (hyperdrive_amd/csrc/hd_keyimport.h) on the host.

The header compiles for the device and the host; here the stand-alone program
tests/native/hd_keyimport_check.cpp runs it as plain C++ under ASan + UBSan,
and every row's status and signer must equal the model of key_import_cases.py,
whose keys and signatories come from the Python oracle (point_mul, the
signatory derivation of all four pubkey formats)."""
import pytest

import hd_pyoracle as O
import key_import_cases as C


@pytest.fixture(scope="module")
def prog():
    return C.build_check(sanitize=True)


def _check(prog, groups):
    got = C.run_check(prog, groups)
    want = [C.expect(row, fmt, sigs, slots) for fmt, sigs, slots, rows in groups for row in rows]
    names = [(fmt, len(sigs), k) for fmt, sigs, slots, rows in groups for k in range(len(rows))]
    bad = [(nm, g, w) for nm, g, w in zip(names, got, want) if g != w]
    assert not bad, f"(format, set size, row): got, want: {bad[:8]}"
    return got


def test_bindings_and_constants():
    # (the library itself is not loaded here)
    from hyperdrive_amd import _lib, verify
    for name in ("hd_import_keys", "hd_export_keys", "hd_multi_import_keys", "hd_multi_export_keys"):
        assert name in _lib.SIGNATURES
    assert (verify.KEY_IMPORTED, verify.KEY_KNOWN, verify.KEY_NOT_ADMITTED, verify.KEY_NO_SLOT,
            verify.KEY_BAD_POINT) == (C.IMPORTED, C.KNOWN, C.NOT_ADMITTED, C.NO_SLOT, C.BAD_POINT)


def test_leading_zero_keys_are_what_they_claim():
    """the searched keys have the leading zero bytes the cases rely on"""
    (x, y), (u, v), (a, b) = C.pub(C.SIGNER_Y0), C.pub(C.SIGNER_X0), C.pub_both()
    assert x >> 248 and not y >> 248
    assert not u >> 248 and v >> 248
    assert not a >> 248 and not b >> 248


@pytest.mark.parametrize("fmt", C.FORMATS)
def test_honest_and_leading_zero_keys(prog, fmt):
    """An honest key, and keys whose X, whose Y and both of whose coordinates
    have a leading zero byte (XY_STRIPPED then hashes 63 or 62 bytes), in each
    format: IMPORTED with the signatory's row; NO_SLOT without a slot map."""
    pubs = [C.pub(0), C.pub(1), C.pub(C.SIGNER_X0), C.pub(C.SIGNER_Y0), C.pub_both()]
    sigs = [O.signatory_of_pub(q, fmt) for q in pubs]
    rows = [C.enc(*q) for q in pubs]
    got = _check(prog, [(fmt, sigs, True, rows), (fmt, sigs, False, rows)])
    assert got == [(C.IMPORTED, k) for k in range(5)] + [(C.NO_SLOT, k) for k in range(5)]


@pytest.mark.parametrize("fmt", C.FORMATS)
def test_bad_rows(prog, fmt):
    """(X, p - Y) is a valid point and another signatory: NOT_ADMITTED.
    (X, Y + 1), (0, 0), X = p, X = 2^256 - 1, Y = p: BAD_POINT."""
    sigs = [O.signatory_of_pub(C.pub(0), fmt), O.signatory_of_pub(C.pub(1), fmt)]
    bad = C.bad_rows(0)
    got = _check(prog, [(fmt, sigs, True, [r for _, r in bad])])
    assert got[0] == (C.NOT_ADMITTED, -1)
    assert got[1:] == [(C.BAD_POINT, -1)] * (len(bad) - 1)


@pytest.mark.parametrize("fmt", C.FORMATS)
def test_admitted_hash_of_an_off_curve_pair_is_bad_point(prog, fmt):
    """The admitted set holds SHA-256 of the encoding of an off-curve pair
    (for the compressed format that is the honest signatory itself: (X, Y + 2)
    encodes as (X, Y) does).  The pair must be BAD_POINT, never IMPORTED --
    the case that fails when the curve check is dropped."""
    x, y = C.pub(0)
    groups = []
    for dy in (1, 2):
        sigs = [C.filler(0), C.sig_of(x, y + dy, fmt), C.filler(1)]
        groups.append((fmt, sigs, True, [C.enc(x, y + dy)]))
    assert C.sig_of(x, y + 2, 1) == O.signatory_of_pub((x, y), 1)
    assert _check(prog, groups) == [(C.BAD_POINT, -1)] * 2


@pytest.mark.parametrize("size", [1, 2, 1024, 1025])
def test_admitted_set_sizes(prog, size):
    """Sets of 1, 2, 1,024 and 1,025 entries with the key's signatory first,
    last and absent; and entered twice, where the signer is the first row."""
    q, fmt = C.pub(2), 1
    s, row = O.signatory_of_pub(q, fmt), C.enc(*C.pub(2))
    fill = [C.filler(k) for k in range(size)]
    first, last, absent = [s] + fill[1:], fill[:-1] + [s], fill
    twice = [fill[0], s] + fill[2:] + [s]
    got = _check(prog, [(fmt, sigs, True, [row]) for sigs in (first, last, absent, twice)])
    assert got == [(C.IMPORTED, 0), (C.IMPORTED, size - 1), (C.NOT_ADMITTED, -1), (C.IMPORTED, 1)]


def test_empty_set(prog):
    assert _check(prog, [(1, [], True, [C.enc(*C.pub(0))])]) == [(C.NOT_ADMITTED, -1)]
