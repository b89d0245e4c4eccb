"""The fixed-base tables in Python integers: what entry (j, d) of a base must
be, and which entries the table tests look at (tests/test_gpu_fb_tables.py).

Entry (j, d) of base B is the affine point d 2^(W j) B at index j N + d - 1,
N = 2^(W-1); the top window holds d <= 2^TOPBITS (hd_fixedbase.h FbL<W>).
Nothing here uses the device headers: Jacobian coordinates over Python
integers, one batched inversion per run of entries, checked against the
oracle's affine point_mul in tests/test_fb_table_ref.py."""
import hd_pyoracle as O

P = O.P
SEG = 512   # k_fb_runs: segments of 512 multiples, walked in blocks of 32
RUN = 32


def geometry(w):
    """(NWIN, N, TOPBITS, TAB) of FbL<w>"""
    nwin = (256 + w - 1) // w
    n = 1 << (w - 1)
    topbits = 256 - w * (nwin - 1)
    return nwin, n, topbits, (nwin - 1) * n + (1 << topbits)


def window_dmax(w, j):
    nwin, n, topbits, _ = geometry(w)
    return (1 << topbits) if j == nwin - 1 else n


def jac_dbl(a):
    X, Y, Z = a
    if Z == 0:
        return a
    A = X * X % P
    B = Y * Y % P
    C = B * B % P
    D = 2 * ((X + B) * (X + B) - A - C) % P
    E = 3 * A % P
    X3 = (E * E - 2 * D) % P
    return X3, (E * (D - X3) - 8 * C) % P, 2 * Y * Z % P


def jac_add_affine(a, b):
    X1, Y1, Z1 = a
    x2, y2 = b
    if Z1 == 0:
        return x2, y2, 1
    ZZ = Z1 * Z1 % P
    H = (x2 * ZZ - X1) % P
    r = (y2 * Z1 % P * ZZ - Y1) % P
    if H == 0:
        return jac_dbl(a) if r == 0 else (0, 1, 0)
    HH = H * H % P
    HHH = H * HH % P
    V = X1 * HH % P
    X3 = (r * r - HHH - 2 * V) % P
    return X3, (r * (V - X3) - Y1 * HHH) % P, Z1 * H % P


def jac_mul_small(d, b):
    """d b for d >= 1, double-and-add from the top bit"""
    a = (b[0], b[1], 1)
    for bit in bin(d)[3:]:
        a = jac_dbl(a)
        if bit == "1":
            a = jac_add_affine(a, b)
    return a


def to_affine(pts):
    """Jacobian points (none at infinity) to affine, one inversion for all"""
    pre, acc = [], 1
    for (_, _, Z) in pts:
        assert Z % P != 0, "a table entry at infinity"
        pre.append(acc)
        acc = acc * Z % P
    inv = pow(acc, -1, P)
    out = [None] * len(pts)
    for k in range(len(pts) - 1, -1, -1):
        X, Y, Z = pts[k]
        zi = inv * pre[k] % P
        inv = inv * Z % P
        z2 = zi * zi % P
        out[k] = (X * z2 % P, Y * z2 % P * zi % P)
    return out


def window_bases(b, w):
    """2^(w j) b for every window j, affine"""
    nwin = geometry(w)[0]
    out = [b]
    for _ in range(nwin - 1):
        a = (out[-1][0], out[-1][1], 1)
        for _ in range(w):
            a = jac_dbl(a)
        out.append(to_affine([a])[0])
    return out


def pack(pt):
    """a table entry's 64 bytes: x, y as 8 little-endian words each"""
    return pt[0].to_bytes(32, "little") + pt[1].to_bytes(32, "little")


def runs_of(ds):
    """sorted distinct d -> [(first, count)] of contiguous runs"""
    out = []
    for d in sorted(set(ds)):
        if out and out[-1][0] + out[-1][1] == d:
            out[-1][1] += 1
        else:
            out.append([d, 1])
    return [(a, c) for a, c in out]


def expected_runs(bj, runs):
    """{first: bytes of the run's entries} for runs [(first, count)] of
    multiples of the window base bj: one small multiplication for a run's
    first point, then additions; one inversion for all runs together"""
    pts = []
    for first, count in runs:
        a = jac_mul_small(first, bj)
        pts.append(a)
        for _ in range(count - 1):
            a = jac_add_affine(a, bj)
            pts.append(a)
    aff = to_affine(pts)
    out, k = {}, 0
    for first, count in runs:
        out[first] = b"".join(pack(p) for p in aff[k:k + count])
        k += count
    return out


def digit_scalar(w, want, rng, top=None):
    """A scalar 0 < u < n whose window digits at width w (fb_digit) are
    want[j] in the windows j < NWIN - 1 it names and, with top = "max" /
    "max-1", 2^TOPBITS / 2^TOPBITS - 1 in the top window; the other bits are
    random.  Digit patterns (Booth: the window's bits plus the bit below,
    minus 2^w when the window's top bit is set):
      -2^(w-1): the window's top bit set, its other bits and the bit below clear
      +2^(w-1): the top bit clear, the other bits and the bit below set
      small d:  the window's bits = d, the bit below clear
      top max:  bits w (NWIN-1) - 1 .. 255 set, bit 200 cleared (keeps u < n)
      top max-1: the same with bit w (NWIN-1) - 1 cleared
    The caller asserts the digits (math_cases.fb_digits_ref) before use."""
    nwin, n, topbits, _ = geometry(w)
    tb = w * (nwin - 1)
    u = rng.getrandbits(250)
    if top:
        u |= ((1 << 256) - 1) ^ ((1 << (tb - 1)) - 1)
        u &= ~(1 << 200)
        if top == "max-1":
            u &= ~(1 << (tb - 1))
    for j in sorted(want):
        d = want[j]
        assert 0 <= j < nwin - 1
        field, below = ((1 << (w - 1)), 0) if d == -n else (n - 1, 1) if d == n else (d, 0)
        assert 0 <= field < (1 << w)
        u &= ~(((1 << w) - 1) << (w * j))
        u |= field << (w * j)
        if j > 0:
            u = (u & ~(1 << (w * j - 1))) | (below << (w * j - 1))
    assert 0 < u < O.N
    return u


def edge_digit_scalars(w, rng):
    """[(scalar, {window: digit}, top)]: the digits of the table entries that
    random scalars essentially never read -- -2^(w-1) in window 0, the middle
    window and window NWIN-2; +2^(w-1) in windows 1, middle and NWIN-2; the
    top window's maximum and maximum - 1; 1, 2, 32, 33, 512 and 513 (the
    builder's direct write, its doubling, block joins, a segment join)"""
    nwin, n, topbits, _ = geometry(w)
    mid = (nwin - 1) // 2
    cases = [({j: -n}, None) for j in (0, mid, nwin - 2)] + [({j: n}, None) for j in (1, mid, nwin - 2)]
    cases += [({}, "max"), ({}, "max-1")]
    cases += [({2 + k: d}, None) for k, d in enumerate((1, 2, 32, 33, 512, 513))]
    return [(digit_scalar(w, want, rng, top), want, top) for want, top in cases]


def combined_digit_scalars(w, rng):
    """The same digits packed into two scalars (for signatures whose key is
    fitted to the scalar, one table per scalar): the negative extremes, the
    top maximum and 1, 2, 32 in one; the positive extremes, the top
    maximum - 1 and 33, 512, 513 in the other."""
    nwin, n, topbits, _ = geometry(w)
    mid = (nwin - 1) // 2
    assert mid >= 5 and mid + 1 < nwin - 3
    a = {0: -n, mid: -n, nwin - 2: -n, 2: 1, 3: 2, 4: 32}
    b = {1: n, mid: n, nwin - 2: n, 2: 33, 3: 512, mid + 1: 513}
    return [(digit_scalar(w, a, rng, "max"), a, "max"), (digit_scalar(w, b, rng, "max-1"), b, "max-1")]


def assert_digits(u, w, want, top, fb_digits_ref):
    nwin, n, topbits, _ = geometry(w)
    ds = fb_digits_ref(u, w)
    for j, d in want.items():
        assert ds[j] == d, (w, j, d, ds[j])
    if top:
        assert ds[-1] == (1 << topbits) - (0 if top == "max" else 1), (w, top, ds[-1])


def edge_set(w, j, rng):
    """The d of window j that the table tests compare: where the builder's
    walk starts, joins its blocks of 32 and its segments of 512, and ends.
    [1, 66]: d = 1 written directly, d = 2 the doubling, two block joins;
    [479, 546]: the end of segment 0, the restart at 513 and a block join;
    the last 66 entries of the window (2^(W-1), or 2^TOPBITS at the top);
    d0 - 34 .. d0 + 34 around two random segment starts d0 = 1 + 512 s and
    around the middle one; 32 random d.  Clipped to the window."""
    dmax = window_dmax(w, j)
    nseg = dmax // SEG
    ds = set(range(1, 67)) | set(range(479, 547)) | set(range(dmax - 65, dmax + 1))
    starts = [nseg // 2] + ([rng.randrange(1, nseg) for _ in range(2)] if nseg > 1 else [])
    for s in starts:
        d0 = 1 + SEG * s
        ds |= set(range(d0 - 34, d0 + 35))
    ds |= {rng.randrange(1, dmax + 1) for _ in range(32)}
    return sorted(d for d in ds if 1 <= d <= dmax)
