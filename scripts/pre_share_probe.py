"""Shared preimages (pre_share): counters of one C2
call, and the cost of the two extra passes when nothing shares.

    python scripts/pre_share_probe.py [--n 1048576] [--calls 20]

Part 1: one 1M C2 call (the benchmark's batch) after the keys are learned;
prints hd_ctx_preimage_stats and hd_ctx_dedup_stats of that call.
Part 2: a batch in which every message has its own preimage and a valid
signature: message k is the generator's message k * 2S + k % S (one vote per
height, signers in turn), gathered on the device from the generator's
workload chunk by chunk.  The verify call is timed with pre_share 1 and 0 in
turn on one context; prints every time, the medians and their difference.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def timed(v, db, verdict, ws, torch):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(ws)
    v.verify_batch_device(db.c_struct(), verdict.data_ptr(), None, None, None, ws.cuda_stream)
    e1.record(ws)
    e1.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--calls", type=int, default=20)
    a = ap.parse_args()
    import torch
    import hyperdrive_amd as hd
    from hyperdrive_amd.device import DeviceBatch, generate, work_stream
    N, S = a.n, 100
    v = hd.Verifier(0)
    keys = v.gen_keys(S)
    v.set_signatories(keys[0])
    ws = work_stream()
    verdict = torch.empty(N, dtype=torch.uint8, device="cuda")

    # part 1: the C2 call's counters
    db, _, _ = generate(v, 0, N, S, 0, keys=keys)
    timed(v, db, verdict, ws, torch)                    # learns the keys
    timed(v, db, verdict, ws, torch)
    t0, d0 = v.preimage_stats()
    c0, r0 = v.dedup_stats()
    ms = timed(v, db, verdict, ws, torch)
    t1, d1 = v.preimage_stats()
    c1, r1 = v.dedup_stats()
    print(json.dumps({"part": "c2 counters", "n": N, "typed": t1 - t0, "distinct": d1 - d0,
                      "distinct_share": round((d1 - d0) / max(t1 - t0, 1), 4), "checked": c1 - c0,
                      "repeats": r1 - r0, "call_ms": round(ms, 3), "valid": int((verdict == 0).sum())}), flush=True)

    # part 2: every message its own preimage
    out = DeviceBatch.empty(N, "cuda")
    fields = ("type", "height", "round", "valid_round", "value", "frm", "sig")
    got, start, chunk = 0, 0, 1 << 20
    idx = torch.arange(chunk, device="cuda", dtype=torch.int64)
    while got < N:
        cb, _, _ = generate(v, 0, chunk, S, 0, start=start, keys=keys)
        g = idx + start
        take = torch.nonzero(g % (2 * S) == (g // (2 * S)) % S).flatten()[: N - got]
        for f in fields:
            getattr(out, f)[got: got + len(take)] = getattr(cb, f)[take]
        got += len(take)
        start += chunk
    torch.cuda.synchronize()
    assert len(torch.unique(out.height)) == N
    res = {1: [], 0: []}
    timed(v, out, verdict, ws, torch)
    assert int((verdict == 0).sum()) == N, "the all-distinct batch must be validly signed"
    for k in range(2 * a.calls + 2):
        ps = 1 - (k & 1)
        v.set_variant("pre_share", ps)
        t0, d0 = v.preimage_stats()
        ms = timed(v, out, verdict, ws, torch)
        t1, d1 = v.preimage_stats()
        assert (t1 - t0, d1 - d0) == ((N, N) if ps else (0, 0)), (ps, t1 - t0, d1 - d0)
        if k >= 2:
            res[ps].append(round(ms, 4))
    med = {ps: sorted(x)[len(x) // 2] for ps, x in res.items()}
    print(json.dumps({"part": "all distinct", "n": N, "ms_pre_share_1": res[1], "ms_pre_share_0": res[0],
                      "median_1": med[1], "median_0": med[0],
                      "cost_pct": round(100 * (med[1] - med[0]) / med[0], 2),
                      "fallback_last_call": v.fastpath_stats()[1], "valid": int((verdict == 0).sum())}), flush=True)
    v.close()


if __name__ == "__main__":
    main()
