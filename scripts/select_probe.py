"""What a keyed read of the retained log (hd_log_select) costs, next to what it
replaces: hd_log_read of the whole log and a numpy filter on the host
(DESIGN §5).

On one GPU, in one process: the C3 shape restricted to one height (kind 1:
height 1, 1,000 signatories, f = 333, `--rounds` rounds of 1 propose + 1,000
prevotes + 1,000 precommits), generated and verified on the device and inserted
into a log that keeps signatures: 4 rounds are 8,004 entries, 50 rounds 100,050.
Three questions are asked of it, each as the count-only form, as a select with
whole rows, and as read-everything-and-filter:

  precommits   one round's precommits for one value     (about 2f+1 .. 1,000 rows)
  vote_of      one sender's precommit of that round     (1 row)
  first_q      the first 2f+1 of `precommits` (limit)   (667 rows)

The arms alternate inside every repetition, so a drift of the machine touches
all of them alike.  Host wall clock around each Python call (every call ends
synchronised); medians with p10 and p90, in microseconds, as one JSON line.
With HD_LIB naming an older build only the arms it has are run (the read
arms), so the read can be compared between two builds in one job.

    python scripts/select_probe.py [--rounds 4] [--reps 30] [--warm 3]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def stats(xs):
    a = np.asarray(xs) * 1e6
    return {"median": round(float(np.median(a)), 1), "p10": round(float(np.percentile(a, 10)), 1),
            "p90": round(float(np.percentile(a, 90)), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--signers", type=int, default=1000)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--label", default=os.environ.get("HD_LIB", "tree"))
    a = ap.parse_args()

    import torch
    from hyperdrive_amd import _lib, quorum
    from hyperdrive_amd.device import generate, work_stream
    from hyperdrive_amd.verify import PRECOMMIT, Verifier
    if not torch.cuda.is_available():
        raise SystemExit("select_probe: no GPU visible (nothing is measured on the CPU)")
    lib = _lib.load()
    S = a.signers
    n = a.rounds * (2 * S + 1)
    v = Verifier(0)
    ks = v.gen_keys(S)
    v.set_signatories(ks[0])
    db, _, _ = generate(v, 1, n, S, 0, keys=ks)
    ws = work_stream()
    with torch.cuda.stream(ws):
        verdict = torch.empty(n, dtype=torch.uint8, device="cuda")
        bitmap = torch.zeros((n + 31) // 32, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    v.verify_batch_device(db.c_struct(), verdict.data_ptr(), None, None, bitmap.data_ptr(), ws.cuda_stream)
    ws.synchronize()
    f = quorum.thresholds(S)[0]
    q = 2 * f + 1
    log = v.open_log(1, f, ks[0], keep_signatures=True)
    res = log.insert_device(db.c_struct(), bitmap.data_ptr(), stream=ws.cuda_stream)
    L = log.entries
    out = {"label": a.label, "messages": n, "entries": L, "kept": res.kept, "S": S, "f": f, "rounds": a.rounds}

    # the questions, from the log itself: the middle round, the value most of its precommits carry
    whole, _ = log.read()
    r0 = int(np.median(whole.round))
    pc = (whole.type == PRECOMMIT) & (whole.round == r0)
    vals, cnt = np.unique(whole.value[pc], axis=0, return_counts=True)
    val = vals[int(np.argmax(cnt))].tobytes()
    who = whole.frm[np.nonzero(pc)[0][len(np.nonzero(pc)[0]) // 2]].tobytes()
    val_a, who_a = np.frombuffer(val, np.uint8), np.frombuffer(who, np.uint8)

    def host_filter(kind):
        b, ok = log.read()
        m = (b.type == PRECOMMIT) & (b.round == r0)
        m &= (b.frm == who_a).all(1) if kind == "vote_of" else (b.value == val_a).all(1)
        pos = np.nonzero(m)[0]
        if kind == "first_q":
            pos = pos[:q]
        return pos, b.sig[pos], b.frm[pos], b.value[pos]

    want = {k: host_filter(k)[0].tolist() for k in ("precommits", "vote_of", "first_q")}
    out["rows"] = {k: len(p) for k, p in want.items()}
    arms = {"read_filter_" + k: (lambda k=k: host_filter(k)) for k in want}
    if hasattr(lib, "hd_log_select"):
        arms.update({
            "count_precommits": lambda: log.count(PRECOMMIT, r0, value=val),
            "select_precommits": lambda: log.select(PRECOMMIT, r0, value=val),
            "count_vote_of": lambda: log.count(PRECOMMIT, r0, sender=who),
            "select_vote_of": lambda: log.select(PRECOMMIT, r0, sender=who, limit=1),
            "positions_first_q": lambda: log.select(PRECOMMIT, r0, value=val, limit=q, rows=False),
            "select_first_q": lambda: log.select(PRECOMMIT, r0, value=val, limit=q),
        })
        assert log.select(PRECOMMIT, r0, value=val).positions.tolist() == want["precommits"]
        assert log.select(PRECOMMIT, r0, sender=who, limit=1).positions.tolist() == want["vote_of"]
        assert log.select(PRECOMMIT, r0, value=val, limit=q).positions.tolist() == want["first_q"]
        assert log.count(PRECOMMIT, r0, value=val) == len(want["precommits"])
    times = {k: [] for k in arms}
    for rep in range(a.warm + a.reps):
        for k, fn in arms.items():
            t0 = time.perf_counter()
            fn()
            dt = time.perf_counter() - t0
            if rep >= a.warm:
                times[k].append(dt)
    out["us"] = {k: stats(t) for k, t in times.items()}
    print(json.dumps(out), flush=True)
    log.close()
    v.close()


if __name__ == "__main__":
    main()
