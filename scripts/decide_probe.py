"""What hd_decide_device_bitmap costs next to the tally it extends.

On one GPU, for the C3 shape (kind 1: 128,064 messages, 1,000 signatories, 64
rounds) or the C2 shape (kind 0: 1M votes, 100 signatories), after the batch is
verified on the device:

  tally     hd_tally_device_bitmap into preallocated arrays
  decide    hd_decide_device_bitmap into preallocated arrays
  host_way  hd_tally_device_bitmap + Verifier._tally_result + quorum.decide
            over every round: the same answer without hd_decide

Each is a host clock around calls that end in a stream synchronise, warmed up,
repeated; median, min and the 10th / 90th percentiles are printed as one JSON
line.  With HD_LIB naming an older build (no hd_decide) only tally and
host_way run, so two builds can be alternated in one job.

    python scripts/decide_probe.py --shape c3 [--reps 40] [--only decide]
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
    a = np.sort(np.array(ts)) * 1e3
    return {"median_ms": round(float(np.median(a)), 4), "min_ms": round(float(a[0]), 4),
            "p10_ms": round(float(a[len(a) // 10]), 4), "p90_ms": round(float(a[(9 * len(a)) // 10]), 4),
            "reps": len(a)}


def timed(fn, warm, reps):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return stats(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=sorted(SHAPES), default="c3")
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--only", choices=["tally", "decide", "host_way"], default=None)
    ap.add_argument("--label", default=os.environ.get("HD_LIB", "tree"))
    a = ap.parse_args()

    import torch
    from hyperdrive_amd import _lib, quorum
    from hyperdrive_amd.device import generate, work_stream
    from hyperdrive_amd.verify import Verifier
    if not torch.cuda.is_available():
        raise SystemExit("decide_probe: no GPU visible (nothing is measured on the CPU)")
    lib = _lib.load()
    kind, n, S = SHAPES[a.shape]
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
    hb = db.to_host()
    f = quorum.thresholds(S)[0]
    out = {"label": a.label, "shape": a.shape, "n": n, "S": S, "f": f}

    t, ta = v._tally_struct(n)

    def tally():
        rc = lib.hd_tally_device_bitmap(v.handle, ctypes.byref(cs), bitmap.data_ptr(), ctypes.byref(t), s)
        assert rc == 0, rc

    def host_way():
        tally()
        tal = v._tally_result(hb, t, ta)
        return {(h, r): quorum.decide(tal, h, r, f, hb.value[0].tobytes(), True) for (h, r) in tal.distinct_any}

    want = (a.only,) if a.only else ("tally", "decide", "host_way")
    if "tally" in want:
        out["tally"] = timed(tally, a.warm, a.reps)
        out["tally_download_bytes"] = int(lib.hd_tally_stage_bytes(v.handle, n, 1))
        out["tally_rows"] = [int(t.n_hr), int(t.n_counts)]
    if "decide" in want and hasattr(lib, "hd_decide_device_bitmap"):
        sched = torch.from_numpy(np.ascontiguousarray(ks[0])).cuda()
        torch.cuda.synchronize()
        o, oa = v._decide_struct(n)
        cin = _lib.HdDecideIn(f, S, sched.data_ptr(), None)

        def decide():
            rc = lib.hd_decide_device_bitmap(v.handle, ctypes.byref(cs), bitmap.data_ptr(), ctypes.byref(cin),
                                             ctypes.byref(o), s)
            assert rc == 0, rc

        out["decide"] = timed(decide, a.warm, a.reps)
        rows = int(o.n)
        staged = max(1024, rows + rows // 4)          # the stage's row capacity once the guess has settled
        out["decide_rows"] = rows
        out["decide_download_bytes"] = 64 + 2 * ((n + 63) // 64 * 64) + 54 * staged + 64
        out["decide_python"] = timed(lambda: v.decide_device(cs, bitmap.data_ptr(), f, schedule=sched,
                                                             stream=s).decisions, 2, max(5, a.reps // 4))
    if "host_way" in want:
        out["host_way"] = timed(host_way, 2, max(5, a.reps // 4))
        out["host_way_rounds"] = len(host_way())
    print(json.dumps(out))
    v.close()


if __name__ == "__main__":
    main()
