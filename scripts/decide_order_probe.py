"""What the ordered decide costs over the plain one, and the host replay it
replaces.

On one GPU, in one process, for the C2 shape (kind 0: 1,048,576 votes, 100
signatories) and the C3 shape (kind 1: 128,064 messages, 1,000 signatories, 64
rounds), after the batch is verified on the device:

  tally            hd_tally_device_bitmap
  decide           hd_decide_device_bitmap
  decide_ordered   hd_decide_ordered_device_bitmap
  host_replay      hd_votes_reset + hd_votes_insert_batch (f set, crossing
                   events on) over the batch's VALID votes, height by height,
                   through the raw C calls on slices built beforehand: the
                   host way to the order of the crossings

The three device calls are warmed up and then ALTERNATED, each call between two
events on its stream (kernels and the download; the call ends in a stream
synchronise) and inside a host clock.  One JSON line per shape with medians,
minima and the 10th / 90th percentiles in milliseconds.  With HD_LIB naming an
older build only the entry points it has are run, so two builds can be
compared by running the script once per build in one job.

    python scripts/decide_order_probe.py [--shapes c2,c3] [--reps 50]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {"c3": (1, 128064, 1000), "c2": (0, 1 << 20, 100)}


def stats(ts):
    a = np.sort(np.array(ts))
    return {"median_ms": round(float(np.median(a)), 4), "min_ms": round(float(a[0]), 4),
            "p10_ms": round(float(a[len(a) // 10]), 4), "p90_ms": round(float(a[(9 * len(a)) // 10]), 4),
            "reps": len(a)}


def host_replay(lib, hb, verdicts, f, reps):
    """ms per replay of the whole batch through the host vote table."""
    from hyperdrive_amd.verify import Batch
    from hyperdrive_amd.votes import VoteLog
    n = len(hb)
    cuts = [0] + (np.flatnonzero(np.diff(hb.height)) + 1).tolist() + [n]
    parts = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        sl = Batch(*(np.ascontiguousarray(x[a:b]) if x is not None else None
                     for x in (hb.type, hb.height, hb.round, hb.valid_round, hb.value, hb.frm, hb.sig)))
        parts.append((int(hb.height[a]), sl, sl.c_struct(), np.ascontiguousarray(verdicts[a:b])))
    most = max(len(p[1]) for p in parts)
    st, dbl, ev = np.zeros(most, np.uint8), np.zeros(most, np.uint32), np.zeros(most, np.uint8)
    ins = ctypes.c_uint32()
    v = VoteLog(parts[0][0])
    v.set_f(f)
    ts, inserted = [], 0
    for _ in range(reps + 1):
        inserted = 0
        t0 = time.perf_counter()
        for h, _sl, cs, vd in parts:
            lib.hd_votes_reset(v._v, h)
            rc = lib.hd_votes_insert_batch(v._v, ctypes.byref(cs), vd.ctypes.data, st.ctypes.data, dbl.ctypes.data,
                                           ev.ctypes.data, ctypes.byref(ins))
            assert rc == 0, rc
            inserted += ins.value
        ts.append((time.perf_counter() - t0) * 1e3)
    v.close()
    return stats(ts[1:]), len(parts), inserted


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="c2,c3")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=5, help="0: skip the host replay")
    ap.add_argument("--label", default=os.environ.get("HD_LIB", "tree"))
    a = ap.parse_args()

    import torch
    from hyperdrive_amd import _lib, quorum
    from hyperdrive_amd.device import generate, work_stream
    from hyperdrive_amd.verify import Verifier
    if not torch.cuda.is_available():
        raise SystemExit("decide_order_probe: no GPU visible (nothing is measured on the CPU)")
    lib = _lib.load()
    for shape in a.shapes.split(","):
        kind, n, S = SHAPES[shape]
        v = Verifier(0)
        ks = v.gen_keys(S)
        v.set_signatories(ks[0])
        db, _, _ = generate(v, kind, n, S, 0, keys=ks)
        ws = work_stream()
        with torch.cuda.stream(ws):
            verdict = torch.empty(n, dtype=torch.uint8, device="cuda")
            bitmap = torch.zeros((n + 31) // 32, dtype=torch.int32, device="cuda")
        cs, s = db.c_struct(), ws.cuda_stream
        for _ in range(2):
            v.verify_batch_device(cs, verdict.data_ptr(), None, None, bitmap.data_ptr(), s)
        ws.synchronize()
        f = quorum.thresholds(S)[0]
        sched = torch.from_numpy(np.ascontiguousarray(ks[0])).cuda()
        torch.cuda.synchronize()
        cin = _lib.HdDecideIn(f, S, sched.data_ptr(), None)
        t, _ta = v._tally_struct(n)
        o, _oa = v._decide_struct(n)
        calls = {}

        def tally():
            assert lib.hd_tally_device_bitmap(v.handle, ctypes.byref(cs), bitmap.data_ptr(), ctypes.byref(t), s) == 0

        def decide():
            assert lib.hd_decide_device_bitmap(v.handle, ctypes.byref(cs), bitmap.data_ptr(), ctypes.byref(cin),
                                               ctypes.byref(o), s) == 0

        calls["tally"] = tally
        if hasattr(lib, "hd_decide_device_bitmap"):
            calls["decide"] = decide
        if hasattr(lib, "hd_decide_ordered_device_bitmap"):
            w, when, until = v._order_struct(n)

            def decide_ordered():
                assert lib.hd_decide_ordered_device_bitmap(v.handle, ctypes.byref(cs), bitmap.data_ptr(),
                                                           ctypes.byref(cin), ctypes.byref(o), ctypes.byref(w), s) == 0

            calls["decide_ordered"] = decide_ordered
        for fn in calls.values():
            for _ in range(a.warm):
                fn()
        dev = {k: [] for k in calls}
        host = {k: [] for k in calls}
        for _ in range(a.reps):
            for k, fn in calls.items():                  # alternated: one call of each per repetition
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0 = time.perf_counter()
                e0.record(ws)
                fn()
                e1.record(ws)
                e1.synchronize()
                host[k].append((time.perf_counter() - t0) * 1e3)
                dev[k].append(e0.elapsed_time(e1))
        out = {"label": a.label, "shape": shape, "n": n, "S": S, "f": f, "rows": int(o.n)}
        for k in calls:
            out[k] = {"device": stats(dev[k]), "host": stats(host[k])}
        if "decide_ordered" in calls:
            out["ordered_minus_decide_ms"] = round(out["decide_ordered"]["device"]["median_ms"]
                                                   - out["decide"]["device"]["median_ms"], 4)
            out["fired"] = int((when[: o.n] != 0xFFFFFFFF).sum())
            if a.host_reps > 0:
                hb = db.to_host()
                rep, heights, inserted = host_replay(lib, hb, verdict.cpu().numpy(), f, a.host_reps)
                out["host_replay"] = dict(rep, heights=heights, inserted=inserted)
        print(json.dumps(out), flush=True)
        v.close()


if __name__ == "__main__":
    main()
