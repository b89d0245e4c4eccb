"""The two-level lean inversions on the host (hyperdrive_amd/csrc/hd_inv2.h).

tests/native/hd_inv2_check.cpp runs the up, mid and down passes the gfx950
kernels run, lane by lane over plain arrays, for the scalars mod n and the
field mod p, K in {8, 16} x K2 in {8, 16}, N in {1, 64 K, 64 K + 1,
64 K K2 + 1}, with random live masks, whole level-1 lanes dead, whole level-2
lanes dead, one live entry and none, and compares every live entry with a
direct inversion of that entry.  The program is stand-alone and built with
ASan + UBSan: its rows have the library's sizes, so an index past one fails.
"""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_inv2_host_check_sanitized():
    assert shutil.which("g++"), "g++ is needed for the host check of hd_inv2.h"
    out = os.path.join(ROOT, "tests", "native", "_build", "hd_inv2_check")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unused-function",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", out,
                    os.path.join(ROOT, "tests", "native", "hd_inv2_check.cpp")], check=True)
    r = subprocess.run([out], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout, r.stderr[-2000:])
