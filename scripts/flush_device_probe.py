"""What a flush into the retained log costs with the delivery kept on the
device (Ingress.flush_decide_device) next to the host path
(Ingress.flush_decide), at three deliveries:

  c5   160 messages: one height of 80 signatories' prevotes and precommits
  c3   8,004 messages: one height of 1,000 signatories, four rounds
  c2   100 senders x 1,000 rows: 500 heights of 100 signatories consumed in one
       flush, the largest delivery of a queue at the default capacity

On one GPU, in one process.  The messages are generated (and signed) on the
device once and go into the queue through MessageQueue.insert_device before
every repetition, unverified: a flush does not look at signatures.  Two
Ingresses, one per path, take turns repetition by repetition; each
repetition refills its queue, empties its log and its vote table, and times

  flush_decide          the Python call, host clock (consume to host arrays,
                        host vote table, upload, hd_log_insert)
  flush_decide_device   the Python call, host clock (hd_mq_consume_device,
                        hd_log_insert_device_bitmap)
  consume / insert      the two halves of each path alone, host clock around
                        each Python call

Both paths run on the context's own stream and every call ends synchronised
with it, so the host clock around a call covers its device work; the
context's stream has no handle a caller could record events on.  Medians with
p10 and p90, in milliseconds, as one JSON line.  With HD_LIB naming an older
build only flush_decide and its halves are run, so two builds can be compared
by running the script once per build in one job.

    python scripts/flush_device_probe.py [--reps 20] [--warm 3] [--only c5,c3,c2]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {"c5": (0, 160, 80), "c3": (1, 8004, 1000), "c2": (0, 100000, 100)}    # generator kind, messages, signatories


def stats(xs):
    q = lambda p: round(float(np.percentile(xs, p)), 4)
    return {"med": q(50), "p10": q(10), "p90": q(90)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--only", default="c5,c3,c2")
    ap.add_argument("--label", default=os.environ.get("HD_LIB", "tree"))
    a = ap.parse_args()

    import torch
    from hyperdrive_amd import _lib
    from hyperdrive_amd.device import generate
    from hyperdrive_amd.ingress import Ingress
    from hyperdrive_amd.verify import Verifier
    if not torch.cuda.is_available():
        raise SystemExit("flush_device_probe: no GPU visible (nothing is measured on the CPU)")
    lib = _lib.load()
    device_path = hasattr(lib, "hd_mq_consume_device")
    out = {"label": a.label, "reps": a.reps, "device_path": device_path}
    for name in a.only.split(","):
        kind, n, S = SHAPES[name]
        v = Verifier(0)
        ks = v.gen_keys(S)
        v.set_signatories(ks[0])
        db, _, _ = generate(v, kind, n, S, 0, keys=ks)
        h = int(db.height.max().item())
        paths = ["host", "device"] if device_path else ["host"]
        ing = {p: Ingress(v, height=h, max_capacity=1000) for p in paths}
        for i in ing.values():
            i.open_log()
        t = {k: [] for k in ("flush_decide", "flush_decide_device", "host_consume", "host_insert", "device_consume",
                             "device_insert")}
        delivered = {}

        def refill(i):
            i.mq.insert_device(db)
            i.log.reset(h)
            i.votes.reset(h)

        def clock(fn):
            t0 = time.perf_counter()
            r = fn()
            return r, (time.perf_counter() - t0) * 1e3

        for rep in range(a.warm + a.reps):
            keep = rep >= a.warm
            for p in paths:                       # the whole call, the paths taking turns
                i = ing[p]
                refill(i)
                (res, dec), ms = clock(i.flush_decide if p == "host" else i.flush_decide_device)
                delivered[p] = (len(res.consumed) if p == "host" else res.n, dec.kept)
                if keep:
                    t["flush_decide" if p == "host" else "flush_decide_device"].append(ms)
            for p in paths:                       # and its two halves
                i = ing[p]
                refill(i)
                if p == "host":
                    res, c_ms = clock(i.flush)
                    b = res.consumed
                    _, i_ms = clock(lambda: i.log.insert(b, np.zeros(len(b), np.uint8), None))
                else:
                    tk, c_ms = clock(lambda: i.mq.consume_device(h))
                    _, i_ms = clock(lambda: i.log.insert_device(tk.batch, tk.d_bitmap, tk.d_value_ok))
                if keep:
                    t[p + "_consume"].append(c_ms)
                    t[p + "_insert"].append(i_ms)
        assert len(set(delivered.values())) == 1 and delivered["host"][0] == n, delivered
        out[name] = {"delivered": n, "kept": delivered["host"][1], "senders": S,
                     **{k: stats(x) for k, x in t.items() if x}}
        for i in ing.values():
            i.close()
        v.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
