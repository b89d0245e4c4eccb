"""Cases of the key carry (a set change that re-tiers the key tables keeps the
known keys), shared by the host test (test_key_carry_host.py) and the GPU test
(test_gpu_key_carry.py): a model of the slot plan written from the issue's
contract, independent of hyperdrive_amd/csrc/hd_keycarry.h, and the driver of
the stand-alone host program tests/native/hd_keycarry_check.cpp."""
import hashlib
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMPTY, CLAIMED, LEARNED, READY = 0, 1, 2, 3


def sig(k):
    """a signatory: 32 bytes that sort in no relation to k"""
    return hashlib.sha256(b"hd-key-carry" + int(k).to_bytes(4, "big")).digest()


def model(snap, states, f0, f1, new_sorted, max_slots):
    """The plan a re-tier must make.  snap: [(signatory, old slot)] as it stood
    at the entry of the set change; states: the old slots' states; [f0, f1):
    the foreign block; new_sorted: the new set, sorted and distinct.

    A row's key is known when its slot is in [1, len(states)), outside the
    foreign block, and LEARNED or READY.  New slots count up from 1 and end
    below max_slots: first the signatories of the new set whose key is known,
    in sorted order, then the others in sorted order.  Returns (adm_slot per
    sorted index or -1, [(row, new slot)] by sorted index, used, carried,
    dropped, known, staying)."""
    assert list(new_sorted) == sorted(set(new_sorted))
    index = {s: k for k, s in enumerate(new_sorted)}
    row_of, known, dropped = {}, 0, 0
    for r, (s, slot) in enumerate(snap):
        if not 1 <= slot < len(states) or f0 <= slot < f1 or states[slot] not in (LEARNED, READY):
            continue
        known += 1
        if s in index and s not in row_of:
            row_of[s] = r
        else:
            dropped += 1
    staying = sum(1 for r, (s, slot) in enumerate(snap)
                  if 1 <= slot < len(states) and not f0 <= slot < f1 and states[slot] in (LEARNED, READY) and s in index)
    adm, carry, nxt = [-1] * len(new_sorted), [], 1
    for first in (True, False):
        for k, s in enumerate(new_sorted):
            if (s in row_of) != first:
                continue
            if nxt < max_slots:
                adm[k] = nxt
                if first:
                    carry.append((row_of[s], nxt))
                nxt += 1
            elif first:
                dropped += 1
    return adm, carry, nxt, len(carry), dropped, known, staying


def build_check(sanitize=True):
    """compile tests/native/hd_keycarry_check.cpp; sanitize: ASan + UBSan"""
    assert shutil.which("g++"), "g++ is needed for the host check of hd_keycarry.h"
    out = os.path.join(ROOT, "tests", "native", "_build", "hd_keycarry_check" + ("_san" if sanitize else ""))
    src = os.path.join(ROOT, "tests", "native", "hd_keycarry_check.cpp")
    deps = [src] + [os.path.join(ROOT, "hyperdrive_amd", "csrc", f)
                    for f in os.listdir(os.path.join(ROOT, "hyperdrive_amd", "csrc")) if f.endswith(".h")]
    if os.path.exists(out) and all(os.path.getmtime(d) <= os.path.getmtime(out) for d in deps):
        return out
    os.makedirs(os.path.dirname(out), exist_ok=True)
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wno-unused-function", *san, "-o", out, src], check=True)
    return out


def run_check(prog, cases):
    """cases: [(snap, states, f0, f1, new_sorted, max_slots)]; returns, per
    case and in the shape model() returns, what the host program planned"""
    lines = []
    for snap, states, f0, f1, new_sorted, max_slots in cases:
        lines.append(f"case {len(snap)} {len(states)} {f0} {f1} {len(new_sorted)} {max_slots}")
        lines += [f"{s.hex()} {slot}" for s, slot in snap]
        lines += [str(v) for v in states]
        lines += [s.hex() for s in new_sorted]
    r = subprocess.run([prog], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    out, rows = [], [ln.split() for ln in r.stdout.split("\n") if ln]
    assert len(rows) == 4 * len(cases)
    for k in range(len(cases)):
        plan, adm, carry, count = rows[4 * k: 4 * k + 4]
        assert (plan[0], adm[0], carry[0], count[0]) == ("plan", "adm", "carry", "count")
        used, carried, dropped = (int(t) for t in plan[1:])
        known, staying = (int(t) for t in count[1:])
        out.append(([int(t) for t in adm[1:]], [tuple(int(x) for x in t.split(":")) for t in carry[1:]],
                    used, carried, dropped, known, staying))
    return out
