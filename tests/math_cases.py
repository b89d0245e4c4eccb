"""One table of single-operation cases for the device arithmetic, run on both
builds: the host build of the headers (tests/test_math_cases.py) and the
gfx950 kernels of hd_mathcheck.hip (tests/test_gpu_devmath.py).

Pure Python.  ``table(op)`` gives an op's input rows (uint32 words, the row
layouts of include/hd_mathcheck.h) and ``check(op, inp, out)`` compares output
rows with Python integers and ``oracle.point_add``: limb values are taken
mod p, Jacobian / XYZZ outputs are made affine here, Z = 0 (mod p) is
infinity, and the output's limb class is asserted where the source promises
one.  Everything is exact.

Rare branches and special wavefronts, and the rows that take them
(test_math_cases.py shows each with the models below, on the CPU):

* fe_normalize's ``ge`` branch (``fe_normalize_model`` restates the function
  and says which half of the test held): p, p + 1 and 2^256 - 1 through the
  comparison with p (p is the case with both low limbs equal to p's), and
  ``FE_TOP_OVERFLOW`` through the top limb; 2^256 + 0x1000003D0, 2p - 1 and
  [0xFFFFFFF7] * 9 fold at weight 2^256 first and end below p.
* sc_from_be_reduce's subtraction: n, n + 1, 2^256 - 1.
* sc_reduce's two last branches (``sc_reduce_model`` restates the three folds
  and reports which were taken; ``REDUCE_CY`` / ``REDUCE_GE`` are built
  backwards from the branch condition, see ``_reduce_preimage``):
  - ``if (cy)``: the third fold wraps past 2^256.  m2 = 2^257 - 1 (m2[8] = 1,
    low half all ones), and m2 = 2^256 + (2^256 - c) (the smallest low half
    that wraps for m2[8] = 1), each unfolded twice to a 512-bit t.
  - final ``sc_ge_n``: the third fold lands in [n, 2^256).  r = n, n + 1,
    2^256 - 1 reached with non-zero upper halves at both earlier folds, and
    the plain 256-bit values n, n + 1, 2^256 - 1 (upper half zero).
* modinv30's early exit (device only).  ``divstep_batches`` is a Python model
  of divsteps30: the number of 30-divstep batches after which g = 0.  Rows of
  the two inversion tables, by wavefront of 64 rows: 0-63 all finish in 17
  batches (the wavefront leaves after 17), 64-127 all need 18, 128-191
  alternate 17 / 18, 192-255 are zero (g = 0 from the start: leaves at the
  first vote); n = 1 and n = 63 run a one-lane and a 63-lane wavefront of the
  first kind, n = 65 a one-lane wavefront of the second.  A CPU search of a
  minute per modulus found no input above 540 divsteps (the maximum was 534,
  ``DIVSTEP_SEARCH``); the two inputs that reached the maximum are rows.
* the sum chain (HD_MC_GXZ_CHAIN): rows 0-63 have six non-zero digits (a
  wavefront that never takes the repair branch); later rows have zero digits,
  sums that start late, a sum that never starts, and partial sums equal to
  + / - the next point, which must end with ZZ = 0.
"""
from __future__ import annotations

import functools
import random

import numpy as np

import hd_pyoracle as oracle

P = oracle.P
N = oracle.N
C = 2 ** 256 - N
M256 = 2 ** 256 - 1
M29 = (1 << 29) - 1
M24 = (1 << 24) - 1
T = [M29, M29, M29 + (1 << 17)] + [M29] * 5 + [M24]
PL = [0x1FFFFC2F, 0x1FFFFFF7] + [M29] * 6 + [M24]          # p's limbs
LOOSE_MAX = 0xFFFFFFF7                                       # fe_norm_weak's input bound
R261 = 2 ** 261

OPS = {
    "fe_mul": 0, "fe_sqr": 1, "fe_norm_weak": 2, "fe_normalize": 3, "fe_add": 4, "fe_sub2": 5, "fe_neg": 6,
    "fe_mul_int": 7, "fe_inv": 8, "fe_inv_divsteps": 9, "fe_sqrt": 10, "fe_flags": 11, "fe_sqr_sqr": 12,
    "fe_sqr_mul_a": 13, "fe_sqr_mul_b": 14, "fe_mul_alias": 15, "fe_sqr_n88": 16,
    "sc_mul": 20, "sc_sqr": 21, "sc_neg": 22, "sc_add": 23, "sc_inv": 24, "sc_inv_divsteps": 25,
    "sc_from_be_reduce": 26, "sc_reduce512": 27, "sc_split_lambda": 28, "sm_mul": 29, "sm_chain": 30,
    "booth": 31, "booth160": 32, "fb_digits": 33,
    "gej_dbl": 40, "gej_add_ge": 41, "gej_add": 42, "gej_add_ge_nx": 43, "gej_add_ge_z1": 44,
    "gxz_add_ge_nx": 45, "gxz_add_ge_z1": 46, "gxz_chain": 47,
}
# the raw field ops: device limbs must equal the host build's word for word
FE_OPS = [k for k, v in OPS.items() if v <= 16]
CHAIN_LEN = 6
SM_CHAIN_LEN = 4


# ------------------------------------------------------------------ limbs
def limbs(v: int):
    """canonical layout of a value < 2^261: 8 limbs of 29 bits and the rest"""
    return [(v >> (29 * i)) & M29 for i in range(8)] + [v >> 232]


def val(l) -> int:
    return sum(int(x) << (29 * i) for i, x in enumerate(l))


def words(v: int, n: int = 8):
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(n)]


def unwords(w) -> int:
    return sum(int(x) << (32 * i) for i, x in enumerate(w))


def in_class(l, k: int) -> bool:
    return all(int(x) <= k * t for x, t in zip(l, T))


def is_canonical(l) -> bool:
    return all(int(x) <= M29 for x in l[:8]) and int(l[8]) <= M24 and val(l) < P


def lneg(l):
    """fe_neg's own output for tight limbs: 2p - a limb by limb (2T)"""
    return [2 * p - int(x) for p, x in zip(PL, l)]


def ladd_p(l, k: int):
    """the same value with k p added limb by limb (a loose form)"""
    return [int(x) + k * p for x, p in zip(l, PL)]


FE_CONSTANTS = [0, 1, 2, 3, 977, 0x1000003D1]
FE_LOOSE_VALUES = [P, P + 1, 2 ** 256 - 1, 2 ** 256 + 0x1000003D0, 2 * P - 1, 2 ** 256 + 5]
# tests/test_devmath.py's field edge values
FE_VALUES = [0, 1, 2, 3, P - 1, P - 2, 2 ** 32, 2 ** 32 - 1, 2 ** 255, P - 2 ** 32, 0x1000003D1,
             2 ** 256 - 2 ** 32 - 978, 2 ** 224 - 1, (1 << 256) - 1 - (1 << 32) - 977 - 5, 977]


def _limb_patterns(mx):
    """limb vectors at the edges of a class with per-limb maxima mx"""
    out = []
    for i in range(9):                                   # each limb alone at its maximum
        out.append([mx[j] if j == i else 0 for j in range(9)])
    out.append(mx[:8] + [0])                             # top limb zero
    out.append([mx[j] if j % 2 == 0 else 0 for j in range(9)])   # alternating 0 and max
    out.append([mx[j] if j % 2 == 1 else 0 for j in range(9)])
    out.append(list(mx))
    return out


@functools.lru_cache(None)
def fe_class(k: int, seed: int = 0, nrand: int = 24):
    """edge and random limb vectors within the class k T"""
    out = []
    for kk in (1, 2, 3, 7):
        if kk <= k:
            out += _limb_patterns([kk * t for t in T])
    out += [limbs(v) for v in FE_CONSTANTS + FE_VALUES]
    out += [limbs(v) for v in FE_LOOSE_VALUES]
    out += [PL, [2 * x for x in PL]]
    rng = random.Random(1000 + 10 * k + seed)
    out += [limbs(rng.randrange(P)) for _ in range(nrand)]
    out += [limbs((P - rng.randrange(2 ** 40)) % P) for _ in range(6)] + [limbs(rng.randrange(2 ** 40)) for _ in range(6)]
    out += [[rng.randrange(k * t + 1) for t in T] for _ in range(nrand)]
    seen, uniq = set(), []
    for l in out:
        if in_class(l, k) and tuple(l) not in seen:
            seen.add(tuple(l))
            uniq.append(list(l))
    return uniq


@functools.lru_cache(None)
def fe_loose():
    """limb vectors up to fe_norm_weak's bound (tests/test_field_bounds.py's list and the classes)"""
    out = [[LOOSE_MAX] * 9] + _limb_patterns([LOOSE_MAX] * 9) + FE_TOP_OVERFLOW + fe_class(7)
    rng = random.Random(22)
    out += [[rng.randrange(LOOSE_MAX + 1) for _ in range(9)] for _ in range(200)]
    return out


def fe_normalize_model(l):
    """hd_field.h fe_normalize restated on Python integers: (canonical limbs, which half of the `ge` test
    held: 0 neither, 1 the top limb ran over 2^24, 2 the comparison with p)"""
    n = [int(x) for x in l]
    c = 0
    for i in range(8):                                   # fe_norm_weak
        t = n[i] + c
        n[i], c = t & M29, t >> 29
    t8 = n[8] + c
    n[8], u = t8 & M24, t8 >> 24
    x = u * 977 + n[0]
    n[0] = x & M29
    y = (x >> 29) + (u << 3) + n[1]
    n[1] = y & M29
    n[2] += y >> 29
    c = 0
    for i in range(2, 8):                                # the second carry pass
        t = n[i] + c
        n[i], c = t & M29, t >> 29
    n[8] += c
    ge = 1 if n[8] >> 24 else 2 if val(n) >= P else 0
    if ge:
        n = limbs(val(n) - P)
    return n, ge


# rows that reach the top-limb half of fe_normalize's test: the fold's carry into limb 2 runs to the top
FE_TOP_OVERFLOW = [[0, M29] + [M29] * 6 + [2 ** 25 - 1], [M29] * 8 + [2 ** 25 - 1]]


def _pairs(A, B, extra=()):
    """every a with a rotating b, every b with a rotating a, plus the listed pairs"""
    out = [(a, B[(3 * i + 1) % len(B)]) for i, a in enumerate(A)]
    out += [(A[(5 * i + 2) % len(A)], b) for i, b in enumerate(B)]
    return out + list(extra)


def _mul_pairs():
    out = []
    for ka, kb in ((1, 7), (7, 1), (2, 3), (3, 2), (1, 1)):
        out += _pairs(fe_class(ka), fe_class(kb), [([ka * t for t in T], [kb * t for t in T])])
    return out


# ---------------------------------------------------------------- scalars
SC_VALUES = [0, 1, 2, N - 1, N - 2, N // 2, N // 2 + 1, C, C - 1, C + 1, 2 ** 128 + 1, 2 ** 128 - 1, 2 ** 128,
             2 ** 255, 2 ** 32 - 1, 2 ** 32, 2 ** 64 - 1, 2 ** 224 - 1]
SC_REDUCE_VALUES = [N, N + 1, 2 ** 256 - 1, N + 5, N - 1, 0]


def modinv_edges(m: int):
    """tests/test_modinv.py's edge list"""
    edge = [1, 2, 3, m - 1, m - 2, (m - 1) // 2, (m + 1) // 2, 2 ** 255 % m, 2 ** 128, 2 ** 128 - 1,
            (1 << 256) - 1 - (1 << 128), 0x5555555555555555555555555555555555555555555555555555555555555555 % m]
    edge += [(1 << k) % m for k in range(0, 256, 7)] + [(m - (1 << k)) % m for k in range(0, 256, 11)]
    return [e for e in edge if e]


@functools.lru_cache(None)
def sc_values(seed: int = 0, nrand: int = 40):
    rng = random.Random(13 + seed)
    return SC_VALUES + [rng.randrange(N) for _ in range(nrand)]


def sc_reduce_model(t: int):
    """hd_field.h sc_reduce restated: (result, the `if (cy)` branch taken, the final sc_ge_n branch taken)"""
    assert 0 <= t < 2 ** 512
    m = (t & M256) + (t >> 256) * C            # stage 1: 13 words
    assert m < 2 ** 416
    m2 = (m & M256) + (m >> 256) * C           # stage 2: 9 words
    assert m2 < 2 ** 288
    r = (m2 & M256) + (m2 >> 256) * C          # stage 3: 8 words and a carry
    cy = r >> 256
    o = r & M256
    if cy:
        o = (o + C) & M256
    ge = o >= N
    if ge:
        o -= N
    return o, bool(cy), ge


def _reduce_preimage(m2: int) -> int:
    """a 512-bit t whose second fold gives m2 (m2 < 2^260): unfold twice, each time giving the upper half
    as much as it can take so that both earlier folds carry weight"""
    def unfold(v, hi_max):
        hi = min(v // C, hi_max)
        lo = v - hi * C
        assert 0 <= lo < 2 ** 256
        return (hi << 256) | lo
    # m = m_hi 2^256 + m_lo with m_lo + m_hi c = m2; m_hi < c keeps m below c 2^256, which a 512-bit t can reach
    m = unfold(m2, C - 1)
    return unfold(m, 2 ** 256 - 1)


REDUCE_CY = [_reduce_preimage(2 ** 257 - 1), _reduce_preimage(2 ** 256 + (2 ** 256 - C)),
             _reduce_preimage(2 ** 256 + 2 ** 256 - 1 - 12345)]
REDUCE_GE = [_reduce_preimage(N), _reduce_preimage(N + 1), _reduce_preimage(2 ** 256 - 1), N, N + 1, 2 ** 256 - 1]


@functools.lru_cache(None)
def reduce512_values():
    rng = random.Random(27)
    out = REDUCE_CY + REDUCE_GE + [0, 1, N - 1, 2 ** 512 - 1, (2 ** 256 - 1) << 256, N * N, (N - 1) * (N - 1),
                                   N * N - 1, N << 256, (N << 256) - 1, C << 256, 2 ** 511, 2 ** 256, 2 ** 384]
    out += [_reduce_preimage(2 ** 256 - C - 1), _reduce_preimage(N - 1)]      # just below each branch
    out += [rng.randrange(2 ** 512) for _ in range(200)]
    return out


# --------------------------------------------------- divstep batch counts
def divstep_count(x: int, m: int) -> int:
    """divsteps (hd_modinv.h divsteps30's rule, on whole integers) until g = 0, from f = m, g = x"""
    f, g, zeta, k = m, x, -1, 0
    while g:
        if g & 1:
            if zeta < 0:
                zeta, f, g = -zeta - 2, g, (g - f) >> 1
            else:
                zeta, g = zeta - 1, (g + f) >> 1
        else:
            zeta, g = zeta - 1, g >> 1
        k += 1
    return k


def divstep_batches(x: int, m: int) -> int:
    return (divstep_count(x, m) + 29) // 30


# A one-off search with divstep_count, one minute per modulus (589,124 random inputs mod n, 600,431 mod p):
# mean 516.9 divsteps, 5.2 % of the inputs done within 17 batches (510 divsteps) and all the others within 18;
# the maximum was 534 for both moduli, so no input above 540 was found.  (maximum, an input reaching it):
DIVSTEP_SEARCH = {
    N: [(534, 0xa4d171f31c46ff7fc3903ca5dad76ab82113579d397c64a92705a3cea2e711a3)],
    P: [(534, 0xd5c9bac0c4a2d3ce361691281c1be1463f823dc32802e660a84d6e2af43ef0d4)],
}


@functools.lru_cache(None)
def modinv_rows(m: int):
    """(rows, batches per row); the first four wavefronts are as named in the module docstring"""
    rng = random.Random(0xD1 + (m & 0xFF))
    fast, slow = [], []
    for e in modinv_edges(m):
        (fast if divstep_batches(e, m) <= 17 else slow).append(e)
    while len(fast) < 96 or len(slow) < 96:
        x = rng.randrange(1, m)
        b = divstep_batches(x, m)
        if b <= 17 and len(fast) < 96:
            fast.append(x)
        elif b > 17 and len(slow) < 96:
            slow.append(x)
    rows = fast[:64] + slow[:64]
    rows += [fast[64 + i // 2] if i % 2 == 0 else slow[64 + i // 2] for i in range(64)]
    rows += [0] * 64
    rows += modinv_edges(m) + [x for _, x in DIVSTEP_SEARCH.get(m, [])]
    rows += [rng.randrange(1, m) for _ in range(100)]
    return rows, [divstep_batches(x, m) if x else 0 for x in rows[:256]]


# ---------------------------------------------------------------- digits
def booth_ref(k: int, w: int, j: int) -> int:
    x = ((k << 1) >> (w * j)) & ((1 << (w + 1)) - 1)
    return (x >> 1) + (x & 1) - ((x >> w) << w)


def window_patterns(w: int):
    """scalars whose w-bit windows are all ones, all zero, and alternate between the two"""
    even = sum(((1 << w) - 1) << (w * j) for j in range(0, 256 // w + 2, 2)) & M256
    return [0, M256, even, M256 ^ even]


BOOTH_WIDTHS = (4, 8, 12, 13, 16, 20, 22, 24)
# tests/test_devmath.py's Booth scalars
BOOTH_VALUES = [0, 1, N - 1, 2 ** 255, 2 ** 256 - 1 - 2 ** 200]


@functools.lru_cache(None)
def booth_values():
    rng = random.Random(14)
    out = list(BOOTH_VALUES)
    for w in BOOTH_WIDTHS:
        out += window_patterns(w)
    return out + SC_VALUES + [rng.randrange(N) for _ in range(100)]


@functools.lru_cache(None)
def booth160_values():
    """signed values of at most 129 bits, as sc_split_lambda produces them (k, or n - k for a negative)"""
    rng = random.Random(15)
    mags = [0, 1, 2, 2 ** 128 - 1, 2 ** 128, 2 ** 128 + 1, 2 ** 129 - 1, 2 ** 127, 7, 8, 9, 2 ** 64 - 1]
    for w in (4, 12):
        mags += [x & (2 ** 129 - 1) for x in window_patterns(w)]
    mags += [rng.randrange(2 ** 128) for _ in range(60)]
    return [x for a in mags for x in (a, (N - a) % N)]


# ---------------------------------------------------------------- points
G = oracle.G


def jac(pt, z: int):
    """(x z^2, y z^3, z) as canonical limbs; None -> infinity in gej_set_inf's form"""
    if pt is None:
        return limbs(0) + limbs(1) + limbs(0)
    return limbs(pt[0] * z * z % P) + limbs(pt[1] * z * z * z % P) + limbs(z % P)


def aff(pt, neg: bool = False):
    """affine limbs; neg: the y of -pt... as fe_neg leaves it (2T), pt itself being the positive point"""
    y = limbs(pt[1])
    return limbs(pt[0]) + (lneg(y) if neg else y)


def from_jac(w):
    x, y, z = val(w[0:9]) % P, val(w[9:18]) % P, val(w[18:27]) % P
    if z == 0:
        return None
    zi = pow(z, -1, P)
    return (x * zi * zi % P, y * zi * zi * zi % P)


def from_xyzz(w):
    x, y, zz, zzz = (val(w[9 * i:9 * i + 9]) % P for i in range(4))
    if zz == 0:
        return None
    assert pow(zz, 3, P) == zzz * zzz % P, "ZZ^3 != ZZZ^2"
    return (x * pow(zz, -1, P) % P, y * pow(zzz, -1, P) % P)


@functools.lru_cache(None)
def point_pool():
    rng = random.Random(40)
    pts = [G, oracle.point_neg(G), oracle.point_mul(2, G), oracle.point_mul(N - 2, G)]
    while len(pts) < 10:                                  # coordinates with long runs of one-bits
        x = (P - 1 - rng.randrange(1 << 20)) if rng.random() < 0.5 else (2 ** 255 - 1 - rng.randrange(1 << 20))
        R = oracle.lift_x(x % P, rng.randrange(2))
        if R is not None:
            pts.append(R)
    pts += [oracle.point_mul(rng.randrange(1, N), G) for _ in range(24)]
    return pts


ZS = [1, 2, P - 1, 2 ** 255, 0x1000003D1, 3 ** 150 % P, 5 ** 100 % P]


@functools.lru_cache(None)
def point_cases():
    """(a, za, b, zb, b negated): a, b affine points or None (infinity), the Jacobian forms scaled by za, zb;
    `b negated`: b's y goes in as the 2T negation of (-b)'s y"""
    pts = point_pool()
    rng = random.Random(41)
    out = []
    for i, a in enumerate(pts):
        za, zb = ZS[i % len(ZS)], ZS[(i + 3) % len(ZS)]
        b = pts[(i + 7) % len(pts)]
        out += [(a, za, b, zb, False), (a, za, b, zb, True),
                (a, za, a, zb, False), (a, za, a, zb, True),                       # b = a: the doubling
                (a, za, oracle.point_neg(a), zb, False), (a, za, oracle.point_neg(a), zb, True),   # b = -a
                (None, za, b, zb, False), (None, za, b, zb, True)]                 # a infinite (b is finite
                                                                                   # by every addition's contract)
    for _ in range(40):
        a, b = rng.choice(pts[10:]), rng.choice(pts[10:])
        out.append((a, rng.randrange(1, P), b, rng.randrange(1, P), rng.random() < 0.5))
    return out


def _b_aff(b, negated):
    return aff(oracle.point_neg(b), True) if negated else aff(b)


def _b_jac(b, zb, negated):
    if b is None or not negated:
        return jac(b, zb)
    w = jac(oracle.point_neg(b), zb)
    return w[0:9] + lneg(w[9:18]) + w[18:27]


@functools.lru_cache(None)
def chain_cases():
    """rows of the sum chain: CHAIN_LEN x (point, neg, skip); the first 64 have no zero digit"""
    pts = point_pool()[10:]
    rng = random.Random(47)

    def dense():
        return [(p, rng.randrange(2), 0) for p in rng.sample(pts, CHAIN_LEN)]
    rows = [dense() for _ in range(64)]
    skips = [(0, 0, 1, 0, 0, 0), (0, 1, 0, 0, 0, 0), (1, 0, 0, 0, 0, 0), (1, 1, 0, 0, 0, 0), (1, 1, 1, 0, 0, 0),
             (1, 1, 1, 1, 1, 0), (1, 1, 1, 1, 1, 1), (0, 1, 1, 1, 1, 1), (0, 0, 0, 0, 0, 1), (1, 0, 1, 0, 1, 0),
             (0, 1, 0, 1, 0, 1), (0, 0, 0, 1, 1, 0)]
    for s in skips:
        for _ in range(2):
            rows.append([(p, ng, sk) for (p, ng, _), sk in zip(dense(), s)])
    # a partial sum equal to +- the next point, at each step and behind a late start
    for pos in range(1, CHAIN_LEN):
        for sign in (1, -1):
            for lead_skip in (0, 1):
                if lead_skip and pos < 2:
                    continue
                r = dense()
                if lead_skip:
                    r[0] = (r[0][0], r[0][1], 1)
                acc = None
                for p, ng, sk in r[:pos]:
                    if not sk:
                        acc = oracle.point_add(acc, oracle.point_neg(p) if ng else p)
                nxt = acc if sign > 0 else oracle.point_neg(acc)
                ng = rng.randrange(2)
                r[pos] = (oracle.point_neg(nxt) if ng else nxt, ng, 0)
                rows.append(r)
    rows += [dense() for _ in range(30)]
    return rows


def chain_model(row):
    """(started, degenerate, sum): degenerate once an addition met + / - its own partial sum"""
    acc, started, degenerate = None, False, False
    for p, ng, sk in row:
        if sk:
            continue
        q = oracle.point_neg(p) if ng else p
        if not started:
            acc, started = q, True
            continue
        if acc is not None and acc[0] == q[0]:
            degenerate = True
        acc = oracle.point_add(acc, q)
    return started, degenerate, acc


# ------------------------------------------------------------------ tables
def _arr(rows):
    a = np.array(rows, dtype=np.uint64)
    assert a.ndim == 2 and a.max() <= 0xFFFFFFFF
    return np.ascontiguousarray(a.astype(np.uint32))


@functools.lru_cache(None)
def table(op: str) -> np.ndarray:
    """the input rows of op (fewer than 4096)"""
    t = _table(op)
    assert 1 <= len(t) < 4096, (op, len(t))
    return t


def _table(op: str) -> np.ndarray:
    if op in ("fe_mul", "fe_mul_alias"):
        return _arr([a + b for a, b in _mul_pairs()])
    if op in ("fe_sqr", "fe_sqr_sqr", "fe_sqr_mul_a"):
        return _arr(fe_class(2, nrand=150))
    if op == "fe_sqr_mul_b":
        return _arr([a + b for a, b in _pairs(fe_class(2), fe_class(7), [([2 * t for t in T], [7 * t for t in T])])])
    if op in ("fe_norm_weak", "fe_normalize"):
        return _arr(fe_loose())
    if op == "fe_add":
        return _arr([a + b for a, b in _pairs(fe_class(3), fe_class(3)) + _pairs(fe_class(1), fe_class(6))])
    if op == "fe_sub2":
        B = [b for b in fe_class(2) if all(x <= 2 * p for x, p in zip(b, PL))]
        return _arr([a + b for a, b in _pairs(fe_class(3), B, [(fe_class(3)[0], [2 * p for p in PL])])])
    if op == "fe_neg":
        return _arr([a for a in fe_class(2) if all(x <= 2 * p for x, p in zip(a, PL))])
    if op == "fe_mul_int":
        rows = []
        for ka, ks in ((1, (0, 1, 2, 3, 4, 7)), (2, (2, 3)), (3, (2,)), (7, (1,))):
            for k in ks:
                rows += [a + [k] for a in fe_class(ka)]
        return _arr(rows)
    if op in ("fe_inv", "fe_sqrt", "fe_sqr_n88"):
        return _arr(fe_class(1, nrand=100))
    if op == "fe_inv_divsteps":
        return _arr([limbs(x) for x in modinv_rows(P)[0]] + fe_class(2))
    if op == "fe_flags":
        A = fe_class(3)
        rows = [a + b for a, b in _pairs(A, fe_class(1))]
        for b in fe_class(1):                              # equal values in different forms
            rows += [b + b, ladd_p(b, 1) + b, ladd_p(b, 2) + b]
            rows += [ladd_p(limbs((val(b) + 1) % P), 1) + b]
        return _arr(rows)
    if op in ("sc_mul", "sc_add", "sm_mul"):
        A = sc_values() + (SC_REDUCE_VALUES if op == "sc_mul" else [])    # sc_mul alone takes operands >= n
        return _arr([words(a) + words(b) for a, b in _pairs(A, A) + [(N - 1, N - 1), (N - 1, 1), (C, C), (0, 0)]])
    if op in ("sc_sqr", "sc_neg", "sc_split_lambda"):
        return _arr([words(a) for a in sc_values(nrand=200)])
    if op == "sc_inv":
        return _arr([words(a) for a in sc_values(nrand=60) + modinv_edges(N)[:40]])
    if op == "sc_inv_divsteps":
        return _arr([words(x) for x in modinv_rows(N)[0]])
    if op == "sc_from_be_reduce":
        return _arr([words(a) for a in SC_REDUCE_VALUES + sc_values(nrand=100)
                     + [random.Random(26).randrange(2 ** 256) for _ in range(100)]])
    if op == "sc_reduce512":
        return _arr([words(t, 16) for t in reduce512_values()])
    if op == "sm_chain":
        rng = random.Random(30)
        V = sc_values()
        rows = [[V[(i + 5 * k) % len(V)] for k in range(1 + SM_CHAIN_LEN)] for i in range(len(V))]
        rows += [[N - 1] * 5, [1] * 5, [0] * 5] + [[rng.randrange(N) for _ in range(5)] for _ in range(100)]
        return _arr([sum((words(v) for v in r), []) for r in rows])
    if op in ("booth", "fb_digits"):
        return _arr([words(k) for k in booth_values()])
    if op == "booth160":
        return _arr([words(k) for k in booth160_values()])
    if op == "gej_dbl":
        rows = [jac(a, za) for a, za, _, _, _ in point_cases()]
        return _arr(rows + [limbs(5) + limbs(7) + limbs(0)])            # infinity with stale X, Y
    if op == "gej_add_ge":
        return _arr([jac(a, za) + _b_aff(b, ng) for a, za, b, _, ng in point_cases() if b is not None])
    if op == "gej_add":
        return _arr([jac(a, za) + _b_jac(b, zb, ng) for a, za, b, zb, ng in point_cases()])
    if op == "gej_add_ge_nx":
        return _arr([jac(a, za) + _b_aff(b, ng) for a, za, b, _, ng in point_cases()
                     if a is not None and b is not None])
    if op in ("gej_add_ge_z1", "gxz_add_ge_z1"):
        return _arr([aff(a) + _b_aff(b, ng) for a, _, b, _, ng in point_cases() if a is not None and b is not None])
    if op == "gxz_add_ge_nx":
        rows = []
        for i, (a, za, b, _, ng) in enumerate(point_cases()):
            if a is None or b is None:
                continue
            zz, zzz = za * za % P, za * za * za % P
            x, y = limbs(a[0] * zz % P), limbs(a[1] * zzz % P)
            if i % 2:                                                   # the loop's loose classes: X 5T, Y 3T
                x, y = ladd_p(x, 4), ladd_p(y, 2)
            rows.append(x + y + limbs(zz) + limbs(zzz) + _b_aff(b, ng))
        return _arr(rows)
    if op == "gxz_chain":
        return _arr([sum((aff(p) + [ng, sk] for p, ng, sk in row), []) for row in chain_cases()])
    raise KeyError(op)


# ------------------------------------------------------------------ checks
LAMBDA = 0x5363AD4CC05C30E0A5261C028812645A122E22EA20816678DF02967C1B23BD72


def _signed(x: int) -> int:
    return x - N if x > N // 2 else x


def check(op: str, inp: np.ndarray, out: np.ndarray) -> None:
    """asserts every output row of op against Python integers"""
    assert len(inp) == len(out)
    chk = _CHECKS[op]
    for k in range(len(inp)):
        i = [int(x) for x in inp[k]]
        o = [int(x) for x in out[k]]
        try:
            chk(i, o)
        except AssertionError as e:
            raise AssertionError(f"{op} row {k}: in {[hex(x) for x in i]} out {[hex(x) for x in o]}: {e}") from None


def _fe_tight(want):
    def f(i, o):
        assert val(o) % P == want(i) % P, "value"
        assert in_class(o, 1), "output not tight"
    return f


def _a(i):
    return val(i[0:9])


def _b(i):
    return val(i[9:18])


def _chk_normalize(i, o):
    assert val(o) == _a(i) % P and is_canonical(o)


def _chk_add(i, o):
    assert o == [x + y for x, y in zip(i[0:9], i[9:18])] and val(o) % P == (_a(i) + _b(i)) % P


def _chk_sub2(i, o):
    assert o == [x + 2 * p - y for x, y, p in zip(i[0:9], i[9:18], PL)] and val(o) % P == (_a(i) - _b(i)) % P


def _chk_neg(i, o):
    assert o == lneg(i[0:9]) and val(o) % P == -_a(i) % P and all(x <= 2 * p for x, p in zip(o, PL))


def _chk_mul_int(i, o):
    assert o == [x * i[9] for x in i[0:9]] and val(o) % P == _a(i) * i[9] % P


def _chk_inv_divsteps(i, o):
    a = _a(i) % P
    assert val(o) == (pow(a, -1, P) if a else 0) and is_canonical(o)


def _chk_sqrt(i, o):
    a = _a(i) % P
    assert val(o[0:9]) % P == pow(a, (P + 1) // 4, P) and in_class(o[0:9], 1)
    assert o[9] == (1 if pow(a, (P - 1) // 2, P) in (0, 1) else 0), "flag"


def _chk_flags(i, o):
    a, b = _a(i) % P, _b(i) % P
    assert o == [int(a == 0), a & 1, int(a == b)]


def _sc(want):
    def f(i, o):
        assert unwords(o) == want(i)
    return f


def _u(i, k=0):
    return unwords(i[8 * k:8 * k + 8])


def _chk_split(i, o):
    k, k1, k2 = _u(i) % N, unwords(o[0:8]), unwords(o[8:16])
    assert k1 < N and k2 < N and (k1 + k2 * LAMBDA) % N == k
    assert abs(_signed(k1)) < 2 ** 128 and abs(_signed(k2)) < 2 ** 128, "half too long"


def _chk_sm_mul(i, o):
    want = _u(i) * _u(i, 1) * pow(R261, -1, N) % N
    assert unwords(o[0:8]) == want
    raw = o[8:17]
    assert all(x <= M29 for x in raw[:8]) and val(raw) < 2 * N and val(raw) % N == want


def _chk_sm_chain(i, o):
    want = _u(i)
    for t in range(SM_CHAIN_LEN):
        want = want * _u(i, 1 + t) * pow(R261, -1, N) % N
    assert unwords(o) == want


def _s32(x):
    return x - (1 << 32) if x >> 31 else x


def _chk_booth(i, o):
    k = _u(i)
    for w, nw, off in ((4, 65, 0), (8, 33, 65)):
        ds = [_s32(x) for x in o[off:off + nw]]
        assert ds == [booth_ref(k, w, j) for j in range(nw)]
        assert all(abs(d) <= 2 ** (w - 1) for d in ds) and sum(d << (w * j) for j, d in enumerate(ds)) == k


def _chk_booth160(i, o):
    k = _u(i)
    neg = k > N // 2
    mag = (N - k) if neg else k
    assert o[0] == int(neg) and unwords(o[1:6]) == mag & (2 ** 160 - 1)
    for w, nw, off in ((4, 33, 6), (12, 11, 39)):
        ds = [_s32(x) for x in o[off:off + nw]]
        assert ds == [(-1 if neg else 1) * booth_ref(mag, w, j) for j in range(nw)]
        assert sum(d << (w * j) for j, d in enumerate(ds)) == (-mag if neg else mag)


def fb_digits_ref(k: int, w: int):
    nw = (256 + w - 1) // w
    ds = [booth_ref(k, w, j) for j in range(nw - 1)]
    x = ((k << 1) >> (w * (nw - 1))) & ((1 << (w + 1)) - 1)
    return ds + [(x >> 1) + (x & 1)]                       # top window: unsigned, takes the Booth carry


def _chk_fb_digits(i, o):
    k = _u(i)
    wg = o[0]
    assert wg in (12, 24), wg
    off = 1
    for w in (13, 16, 20, 22, wg):
        nw = (256 + w - 1) // w
        ds = [_s32(x) for x in o[off:off + nw]]
        assert ds == fb_digits_ref(k, w), w
        assert sum(d << (w * j) for j, d in enumerate(ds)) == k
        assert all(abs(d) <= 2 ** (w - 1) for d in ds[:-1]) and 0 <= ds[-1] <= 2 ** (256 - w * (nw - 1))
        off += nw
    assert not any(o[off:])


def _jac_tight(o):
    assert all(in_class(o[9 * c:9 * c + 9], 1) for c in range(3)), "coordinates not tight"


def _chk_gej_dbl(i, o):
    a = from_jac(i)
    assert from_jac(o) == oracle.point_add(a, a)
    _jac_tight(o)


def _aff_in(w):
    return (val(w[0:9]) % P, val(w[9:18]) % P)


def _chk_gej_add_ge(i, o):
    assert from_jac(o) == oracle.point_add(from_jac(i[0:27]), _aff_in(i[27:45]))
    _jac_tight(o)


def _chk_gej_add(i, o):
    assert from_jac(o) == oracle.point_add(from_jac(i[0:27]), from_jac(i[27:54]))
    _jac_tight(o)


def _nx(a, b, got):
    """the additions with no exceptional cases: a = +-b must give Z = 0 (ZZ = 0), else the sum"""
    if a[0] == b[0]:
        assert got is None, "a = +-b must end with Z = 0"
    else:
        assert got == oracle.point_add(a, b)


def _chk_gej_add_ge_nx(i, o):
    _nx(from_jac(i[0:27]), _aff_in(i[27:45]), from_jac(o))
    _jac_tight(o)


def _chk_gej_add_ge_z1(i, o):
    _nx(_aff_in(i[0:18]), _aff_in(i[18:36]), from_jac(o))
    _jac_tight(o)


def _xyzz_class(o):
    assert in_class(o[0:9], 5) and in_class(o[9:18], 3) and in_class(o[18:27], 1) and in_class(o[27:36], 1), \
        "XYZZ limb classes (5T, 3T, T, T)"


def _chk_gxz_add_ge_nx(i, o):
    _nx(from_xyzz(i[0:36]), _aff_in(i[36:54]), from_xyzz(o))
    _xyzz_class(o)


def _chk_gxz_add_ge_z1(i, o):
    _nx(_aff_in(i[0:18]), _aff_in(i[18:36]), from_xyzz(o))
    _xyzz_class(o)


def _chk_gxz_chain(i, o):
    row = [(_aff_in(i[20 * k:20 * k + 18]), i[20 * k + 18], i[20 * k + 19]) for k in range(CHAIN_LEN)]
    started, degenerate, want = chain_model(row)
    assert o[27] == int(started), "started"
    if not started:
        return
    xn, yn, t = (val(o[9 * c:9 * c + 9]) % P for c in range(3))
    assert all(in_class(o[9 * c:9 * c + 9], 1) for c in range(3))
    if degenerate or want is None:
        assert o[28] == 1 and t == 0, "a degenerate sum must end with ZZ = 0"
        return
    assert o[28] == 0 and t != 0
    ti = pow(t, -1, P)
    assert (xn * ti % P, yn * ti % P) == want


_CHECKS = {
    "fe_mul": _fe_tight(lambda i: _a(i) * _b(i)),
    "fe_mul_alias": _fe_tight(lambda i: _a(i) * _b(i)),
    "fe_sqr": _fe_tight(lambda i: _a(i) ** 2),
    "fe_norm_weak": _fe_tight(_a),
    "fe_normalize": _chk_normalize,
    "fe_add": _chk_add,
    "fe_sub2": _chk_sub2,
    "fe_neg": _chk_neg,
    "fe_mul_int": _chk_mul_int,
    "fe_inv": _fe_tight(lambda i: pow(_a(i) % P, P - 2, P)),
    "fe_inv_divsteps": _chk_inv_divsteps,
    "fe_sqrt": _chk_sqrt,
    "fe_flags": _chk_flags,
    "fe_sqr_sqr": _fe_tight(lambda i: _a(i) ** 4),
    "fe_sqr_mul_a": _fe_tight(lambda i: _a(i) ** 3),
    "fe_sqr_mul_b": _fe_tight(lambda i: _a(i) ** 2 * _b(i)),
    "fe_sqr_n88": _fe_tight(lambda i: pow(_a(i) % P, 2 ** 88, P)),
    "sc_mul": _sc(lambda i: _u(i) * _u(i, 1) % N),
    "sc_sqr": _sc(lambda i: _u(i) ** 2 % N),
    "sc_neg": _sc(lambda i: -_u(i) % N),
    "sc_add": _sc(lambda i: (_u(i) + _u(i, 1)) % N),
    "sc_inv": _sc(lambda i: pow(_u(i), N - 2, N)),
    "sc_inv_divsteps": _sc(lambda i: pow(_u(i), -1, N) if _u(i) else 0),
    "sc_from_be_reduce": _sc(lambda i: _u(i) % N),
    "sc_reduce512": _sc(lambda i: unwords(i) % N),
    "sc_split_lambda": _chk_split,
    "sm_mul": _chk_sm_mul,
    "sm_chain": _chk_sm_chain,
    "booth": _chk_booth,
    "booth160": _chk_booth160,
    "fb_digits": _chk_fb_digits,
    "gej_dbl": _chk_gej_dbl,
    "gej_add_ge": _chk_gej_add_ge,
    "gej_add": _chk_gej_add,
    "gej_add_ge_nx": _chk_gej_add_ge_nx,
    "gej_add_ge_z1": _chk_gej_add_ge_z1,
    "gxz_add_ge_nx": _chk_gxz_add_ge_nx,
    "gxz_add_ge_z1": _chk_gxz_add_ge_z1,
    "gxz_chain": _chk_gxz_chain,
}
