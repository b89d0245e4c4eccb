"""Cases of hd_import_keys, shared by the host test (test_key_import_host.py)
and the GPU test (test_gpu_key_import.py): keys from the Python oracle, the
status and signer every row must get (a model written from the header's
contract, independent of hd_keyimport.h), and the driver of the stand-alone
host program tests/native/hd_keyimport_check.cpp."""
import hashlib
import os
import shutil
import subprocess

import hd_pyoracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMPORTED, KNOWN, NOT_ADMITTED, NO_SLOT, BAD_POINT = 0, 1, 2, 3, 4
FORMATS = (0, 1, 2, 3)   # uncompressed, compressed, raw X || Y, X.Bytes() || Y.Bytes()

# Keys with a leading zero byte: in Y (signer 58), in X (signer 560) -- the
# signers tests/golden/make_golden.py found -- and in both: K_BOTH G, the
# first multiple of G with that property (found by adding G 55,958 times).
SIGNER_Y0, SIGNER_X0, K_BOTH = 58, 560, 55959

_pub = {}


def pub(i):
    """public key of the generator's signer i"""
    if i not in _pub:
        _pub[i] = O.pubkey_of(O.signer_sk(i))
    return _pub[i]


def pub_both():
    if "both" not in _pub:
        _pub["both"] = O.point_mul(K_BOTH, O.G)
    return _pub["both"]


def enc(x, y):
    """a row of hd_import_keys: X || Y, 32 bytes big-endian each"""
    return x.to_bytes(32, "big") + y.to_bytes(32, "big")


def sig_of(x, y, fmt):
    """SHA-256 of the encoding of (x, y) in pubkey format fmt, on the curve or not"""
    return O.sha256(O.pubkey_bytes((x, y), fmt))


def expect(key, fmt, sigs, slots=True):
    """(status, signer) of one row against the signatory array `sigs` (caller
    order) on a context whose slots are all empty"""
    x, y = int.from_bytes(key[:32], "big"), int.from_bytes(key[32:], "big")
    if x >= O.P or y >= O.P or (y * y - x * x * x - 7) % O.P:
        return BAD_POINT, -1
    s = sig_of(x, y, fmt)
    if s not in sigs:
        return NOT_ADMITTED, -1
    return (IMPORTED if slots else NO_SLOT), sigs.index(s)


def bad_rows(i=0):
    """(name, row) of the rows that are no key of an admitted signatory,
    derived from signer i's key; every one is BAD_POINT except the negated
    point, which is a valid key of another signatory"""
    x, y = pub(i)
    assert y + 2 < O.P
    return [("negated", enc(x, O.P - y)), ("y+1", enc(x, y + 1)), ("zero", enc(0, 0)), ("x=p", enc(O.P, y)),
            ("x=2^256-1", enc(2 ** 256 - 1, y)), ("y=p", enc(x, O.P)),
            # same X, same parity of Y: the compressed encoding is the honest key's
            ("y+2", enc(x, y + 2))]


def filler(k):
    """a signatory no key of these tests hashes to"""
    return hashlib.sha256(b"hd-key-import-filler" + k.to_bytes(4, "big")).digest()


def build_check(sanitize=True):
    """compile tests/native/hd_keyimport_check.cpp; sanitize: ASan + UBSan"""
    assert shutil.which("g++"), "g++ is needed for the host check of hd_keyimport.h"
    out = os.path.join(ROOT, "tests", "native", "_build", "hd_keyimport_check" + ("_san" if sanitize else ""))
    src = os.path.join(ROOT, "tests", "native", "hd_keyimport_check.cpp")
    deps = [src] + [os.path.join(ROOT, "hyperdrive_amd", "csrc", f)
                    for f in os.listdir(os.path.join(ROOT, "hyperdrive_amd", "csrc")) if f.endswith(".h")]
    if os.path.exists(out) and all(os.path.getmtime(d) <= os.path.getmtime(out) for d in deps):
        return out
    os.makedirs(os.path.dirname(out), exist_ok=True)
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wno-unused-function", *san, "-o", out, src], check=True)
    return out


def run_check(prog, groups):
    """groups: [(fmt, sigs, slots, [row, ...])]; returns [(status, signer)] of
    every row, in order, from one run of the host program"""
    lines, total = [], 0
    for fmt, sigs, slots, rows in groups:
        lines.append(f"set {fmt} {len(sigs)} {1 if slots else 0}")
        lines += [s.hex() for s in sigs]
        lines += ["key " + r.hex() for r in rows]
        total += len(rows)
    r = subprocess.run([prog], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    out = [tuple(int(t) for t in ln.split()) for ln in r.stdout.split("\n") if ln]
    assert len(out) == total
    return out
