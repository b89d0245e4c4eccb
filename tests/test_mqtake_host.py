"""The consume into device memory (include/hd_mq.h hd_mq_consume_device) on
the host: the locate of a delivered row's sender, the binding, and the
scenario table of the GPU test.

The locate (hyperdrive_amd/csrc/hd_mqtake.h) is plain C++; the stand-alone
program tests/native/hd_mqtake_check.cpp runs the text k_mq_take_rows
compiles under ASan + UBSan, and the sender it names for a row must equal the
model of mq_device_cases.py, which lays the rows out sender by sender.  A
sender that delivers nothing shares its offset with the next one, so the
cases put such senders first, last and in runs in the middle."""
import random

import pytest

import mq_device_cases as C


@pytest.fixture(scope="module")
def prog():
    return C.build_check(sanitize=True)


def _check(prog, tables, rows=None):
    """every row (or `rows`) of every table of per-sender counts"""
    cases = [(c, list(range(sum(c))) if rows is None else rows(c)) for c in tables]
    got = C.run_check(prog, cases)
    for (counts, ks), g in zip(cases, got):
        assert g == [C.locate_model(counts, k) for k in ks], counts[:40]
        assert all(counts[s] > 0 for s in g)                     # the located sender delivers
    return got


def test_binding_of_the_device_consume():
    # (the library itself is not loaded here)
    import ctypes
    from hyperdrive_amd import _lib
    for name in ("hd_mq_consume_device", "hd_mq_taken_value_ok", "hd_mq_taken_read"):
        assert name in _lib.SIGNATURES
    assert ctypes.sizeof(_lib.HdMqPropose) == 96
    assert [n for n, _ in _lib.HdMqPropose._fields_] == ["index", "sender", "height", "round", "valid_round",
                                                         "value32", "from32"]
    assert [n for n, _ in _lib.HdMqTaken._fields_] == ["n", "removed", "batch", "d_sender", "d_valid_bitmap",
                                                       "d_value_ok", "n_proposes", "proposes"]
    assert _lib.HdMqTaken.batch.offset == 8 and dict(_lib.HdMqTaken._fields_)["batch"] is _lib.HdBatch
    from hyperdrive_amd.ingress import Ingress
    from hyperdrive_amd.mq import MessageQueue, Taken
    assert callable(MessageQueue.consume_device) and callable(Ingress.flush_decide_device)
    assert callable(Taken.set_value_ok) and callable(Taken.read)


def test_struct_layouts_match_the_header(tmp_path):
    """hd_mq_propose and hd_mq_taken as the C compiler lays them out"""
    import ctypes
    import os
    import shutil
    import subprocess
    from hyperdrive_amd import _lib
    assert shutil.which("gcc"), "gcc is needed for the layout check"
    structs = {"hd_mq_propose": _lib.HdMqPropose, "hd_mq_taken": _lib.HdMqTaken}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "hd_mq.h"', "int main(void) {"]
    for cname, py in structs.items():
        lines.append(f'printf("{cname} size %zu\\n", sizeof({cname}));')
        lines += [f'printf("{cname} {f} %zu\\n", offsetof({cname}, {f}));' for f, _ in py._fields_]
    lines.append("return 0; }")
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", os.path.join(C.ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = {}
    for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n"):
        if line:
            a, b, c = line.split()
            got[(a, b)] = int(c)
    for cname, py in structs.items():
        assert got[(cname, "size")] == ctypes.sizeof(py), cname
        for f, _ in py._fields_:
            assert got[(cname, f)] == getattr(py, f).offset, (cname, f)
    assert got[("hd_mq_propose", "size")] == 96


def test_one_sender(prog):
    _check(prog, [[1], [2], [64], [1000]])


def test_first_and_last_sender_deliver_nothing(prog):
    _check(prog, [[0, 5], [5, 0], [0, 5, 0], [0, 0, 3, 4, 0, 0], [0, 1, 0], [0, 0, 0, 1]])


def test_runs_of_senders_that_deliver_nothing(prog):
    _check(prog, [[3, 0, 2], [3, 0, 0, 0, 2], [1, 0, 1, 0, 0, 1, 0, 0, 0, 1], [2, 0, 0, 7, 0, 1, 0, 0, 0, 0, 0, 0, 4],
                  [0, 4, 0, 0, 4, 0]])
    rng = random.Random(11)
    _check(prog, [[rng.choice([0, 0, 0, 1, 2, 9]) for _ in range(rng.randrange(1, 70))] + [1] for _ in range(200)])


def test_every_sender_delivers_one_row(prog):
    got = _check(prog, [[1] * n for n in (1, 2, 3, 63, 64, 65, 1024)])
    assert got[-1] == list(range(1024))


def test_1025_senders(prog):
    rng = random.Random(12)
    ones = [1] * 1025
    thirds = [0 if k % 3 == 1 else 1 for k in range(1025)]         # the GPU scenario s1025
    mixed = [rng.choice([0, 0, 1, 3, 1000]) for _ in range(1024)] + [2]
    sparse = [0] * 1025
    sparse[0], sparse[511], sparse[512], sparse[1024] = 1, 2, 3, 1
    _check(prog, [ones, thirds, sparse])
    got, = _check(prog, [mixed], rows=C.edge_rows)                  # every run's first and last row
    assert len(got) > 700 and got[-1] == 1024


def test_first_and_last_row_of_every_run(prog):
    rng = random.Random(13)
    tables = [[rng.choice([0, 1, 2, 255, 256, 257, 4097]) for _ in range(rng.randrange(1, 40))] + [1]
              for _ in range(60)]
    _check(prog, tables, rows=C.edge_rows)
    # and the rows next to the edges
    near = lambda c: sorted({k for e in C.edge_rows(c) for k in (e - 1, e, e + 1) if 0 <= k < sum(c)})
    _check(prog, tables[:20], rows=near)


@pytest.mark.parametrize("name", C.NAMES)
def test_scenario_covers_its_edge(name):
    sc = C.scenario(name)
    removed, got = C.check(sc)
    assert sc.expect["deliver"] == len(got)


def test_scenario_table_covers_the_issue():
    counts = {C.scenario(n).expect["deliver"] for n in C.DELIVERY}
    assert {0, 1, 63, 64, 65, 255, 257, 4097} <= counts
    assert {C.scenario(n).expect["senders"] for n in ("one_sender", "three_senders", "s1025")} == {1, 3, 1025}
    assert C.scenario("empty").batches == [] and C.scenario("none_allowed").expect["more_removed"]
    assert C.scenario("window").allowed is None and len(C.scenario("window").admitted) == 5
