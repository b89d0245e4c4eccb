"""tests/fb_table_ref.py (the Python-integer reference of the device-built
tables) against the oracle's affine point_mul, and the edge set's content: the
reference of the GPU table test must itself be right.  No GPU."""
import random

import fb_table_ref as R


def test_runs_equal_point_mul(oracle):
    O = oracle
    rng = random.Random(3)
    B = O.pubkey_of(O.signer_sk(7))
    for w in (13, 24):
        nwin, n, topbits, tab = R.geometry(w)
        bases = R.window_bases(B, w)
        for j in (0, 1, nwin - 1):
            assert bases[j] == O.point_mul(pow(2, w * j, O.N), B)
            dmax = R.window_dmax(w, j)
            runs = [(1, 3), (dmax - 1, 2), (rng.randrange(2, dmax - 40), 35)]
            got = R.expected_runs(bases[j], runs)
            for first, count in runs:
                for k in (0, count - 1):
                    want = O.point_mul((first + k) * pow(2, w * j, O.N) % O.N, B)
                    assert got[first][64 * k:64 * k + 64] == R.pack(want), (w, j, first + k)


def test_geometry_matches_the_documented_tables():
    assert R.geometry(13) == (20, 4096, 9, 78336)
    assert R.geometry(16) == (16, 32768, 16, 15 * 32768 + 65536)
    assert R.geometry(20) == (13, 1 << 19, 16, 12 * (1 << 19) + 65536)
    assert R.geometry(22) == (12, 1 << 21, 14, 11 * (1 << 21) + (1 << 14))
    assert R.geometry(24) == (11, 1 << 23, 16, 10 * (1 << 23) + 65536)


def test_edge_digit_scalars_have_their_digits(oracle):
    from math_cases import fb_digits_ref
    rng = random.Random(2)
    for w in (13, 16, 20, 22, 24):
        nwin, n, topbits, _ = R.geometry(w)
        single = R.edge_digit_scalars(w, rng)
        assert len(single) == 14
        for u, want, top in single + R.combined_digit_scalars(w, rng):
            assert 0 < u < oracle.N
            R.assert_digits(u, w, want, top, fb_digits_ref)
            ds = fb_digits_ref(u, w)
            assert sum(d << (w * j) for j, d in enumerate(ds)) == u
        tops = [fb_digits_ref(u, w)[-1] for u, _, top in single if top]
        assert tops == [1 << topbits, (1 << topbits) - 1]
        flat = {(j, d) for _, want, _ in single for j, d in want.items()}
        assert {d for _, d in flat} == {-n, n, 1, 2, 32, 33, 512, 513}
        assert {j for j, d in flat if d == -n} == {0, (nwin - 1) // 2, nwin - 2}
        assert {j for j, d in flat if d == n} == {1, (nwin - 1) // 2, nwin - 2}


def test_edge_set_holds_the_structural_entries():
    rng = random.Random(1)
    for w in (13, 16, 20, 22, 24):
        nwin = R.geometry(w)[0]
        for j in (0, nwin - 1):
            ds = R.edge_set(w, j, rng)
            dmax = R.window_dmax(w, j)
            assert ds == sorted(set(ds)) and ds[0] == 1 and ds[-1] == dmax
            for d in (1, 2, 32, 33, 64, 65, 512, 513, 544, 545, dmax - 1, dmax):
                assert d in ds or d > dmax, (w, j, d)
            if dmax > R.SEG:
                mid = 1 + R.SEG * (dmax // R.SEG // 2)
                assert {mid - 1, mid, mid + 31, mid + 32} <= set(ds)
            assert 32 <= len(ds) <= 66 + 68 + 66 + 3 * 69 + 32
