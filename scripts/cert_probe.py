"""What checking many quorum certificates costs (hd_check_certificates_device),
next to the only way there was before it: quorum.check_certificate once per
certificate (DESIGN §5 "Certificates").

On one GPU, in one process.  The votes come from the generator's rounds shape
(kind 1: height 1, `--signers` signatories, one round = 1 propose + S prevotes
+ S precommits, 90 % of them for the round's canonical value), generated on the
device.  A certificate is `--votes` precommits of one round for its canonical
value, gathered on the device into one batch of `--certs` x `--votes` messages
(1,000 x 667 by default; `--certs 5000 --votes 3` is the other shape).  The
signatories' keys are learned by a first context, exported and imported into
the measured one, so every verification is the known-key check.

Arms, alternated inside every repetition:

  verify+check   hd_verify_batch_device, then hd_check_certificates_device on
                 the same stream: HIP events before the first and after the
                 second (which returns synchronised)
  check          the second call alone, its hd_cert rows built beforehand
                 (verify.cert_rows): HIP events around it
  check_specs    the same from the list of CertSpec: the Python loop that
                 fills the rows is inside the events
  verify         hd_verify_batch_device alone, for the difference
  host_loop      quorum.check_certificate per certificate on host slices of
                 the same batch: host clock (every call ends synchronised);
                 skipped with --no-host (the kernel-trace run)

Medians of `--reps` after `--warm`, with p10 and p90, in microseconds, as one JSON line.  Every
arm's answers are compared once before anything is timed.

    python scripts/cert_probe.py [--certs 1000] [--votes 667] [--signers 1000] [--reps 20] [--warm 3]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def stats(xs, scale):
    a = np.asarray(xs) * scale
    return {"median": round(float(np.median(a)), 1), "p10": round(float(np.percentile(a, 10)), 1),
            "p90": round(float(np.percentile(a, 90)), 1)}


def rows_of(res):
    return res.status.tolist(), res.good.tolist(), res.first_bad.tolist()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--certs", type=int, default=1000)
    ap.add_argument("--votes", type=int, default=667)
    ap.add_argument("--signers", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()

    import torch
    from hyperdrive_amd import quorum
    from hyperdrive_amd.device import DeviceBatch, generate, work_stream
    from hyperdrive_amd.verify import PRECOMMIT, CertSpec, Verifier, cert_rows
    if not torch.cuda.is_available():
        raise SystemExit("cert_probe: no GPU visible (nothing is measured on the CPU)")
    S, K, q = a.signers, a.certs, a.votes
    f = quorum.thresholds(S)[0]
    rounds = min(K, 1000)
    per_round = S // q if q <= S else 0
    if per_round * rounds < K:
        raise SystemExit("cert_probe: too many certificates for 1,000 rounds of this signatory set")

    # the workload, and a first context that learns the keys
    teacher = Verifier(0)
    ks = teacher.gen_keys(S)
    teacher.set_signatories(ks[0])
    n_all = rounds * (2 * S + 1)
    src, _, _ = generate(teacher, 1, n_all, S, 0, keys=ks)
    ws = work_stream()
    with torch.cuda.stream(ws):
        vd = torch.empty(n_all, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    teacher.verify_batch_device(src.c_struct(), vd.data_ptr(), None, None, None, ws.cuda_stream)
    ws.synchronize()
    assert int(vd.max()) == 0, "the generated votes are VALID"
    keys, known = teacher.export_keys()
    teacher.close()

    # certificate k: the (k // rounds)-th run of q precommits for the canonical value of round k % rounds
    h_type, h_round = src.type.cpu().numpy(), src.round.cpu().numpy()
    h_value = src.value.cpu().numpy()
    index, specs = [], []
    for r in range(rounds):
        lo = r * (2 * S + 1)
        blk = slice(lo, lo + 2 * S + 1)
        canon = h_value[lo]                                   # the round's propose carries the canonical value
        ok = (h_type[blk] == PRECOMMIT) & (h_value[blk] == canon).all(1)
        pos = lo + np.nonzero(ok)[0]
        for j in range((K - r + rounds - 1) // rounds):
            assert len(pos) >= (j + 1) * q, "a round with too few precommits for its canonical value"
            index.append((r + j * rounds, pos[j * q:(j + 1) * q], int(h_round[lo]), canon.tobytes()))
    index.sort(key=lambda t: t[0])
    gather = torch.from_numpy(np.concatenate([t[1] for t in index]).astype(np.int64)).to("cuda")
    n = K * q
    db = DeviceBatch(n, src.type[gather], src.height[gather], src.round[gather], src.valid_round[gather],
                     src.value[gather].contiguous(), src.frm[gather].contiguous(), src.sig[gather].contiguous())
    specs = [CertSpec(k * q, q, PRECOMMIT, 1, t[2], t[3], q) for k, t in enumerate(index)]
    torch.cuda.synchronize()
    del src

    v = Verifier(0)
    v.set_signatories(ks[0])
    status, _ = v.import_keys(keys[known])
    with torch.cuda.stream(ws):
        verdict = torch.empty(n, dtype=torch.uint8, device="cuda")
        signer = torch.empty(n, dtype=torch.int32, device="cuda")
        bitmap = torch.zeros((n + 31) // 32, dtype=torch.int32, device="cuda")
    cs = db.c_struct()
    s = ws.cuda_stream

    def verify():
        v.verify_batch_device(cs, verdict.data_ptr(), None, signer.data_ptr(), bitmap.data_ptr(), s)

    rows = cert_rows(specs)

    def check(certs=rows):
        return v.check_certificates_device(cs, bitmap.data_ptr(), signer.data_ptr(), S, certs, s)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(ws)
        fn()
        e1.record(ws)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3

    verify()
    res = check()
    assert rows_of(check(specs)) == rows_of(res)
    assert res.ok == [True] * K and res.good.tolist() == [q] * K, "every certificate is OK"
    known_keys, fallback = v.fastpath_stats()
    plan = Verifier.cert_plan(S, K)
    out = {"certs": K, "votes": q, "messages": n, "S": S, "f": f, "imported": int((status <= 1).sum()),
           "known_keys": known_keys, "last_fallback": fallback, "plan": plan}

    arms = {"verify+check": lambda: timed(lambda: (verify(), check())), "check": lambda: timed(check),
            "check_specs": lambda: timed(lambda: check(specs)),
            "verify": lambda: timed(verify)}
    if not a.no_host:
        host = db.to_host()
        from hyperdrive_amd.verify import Batch
        cut = [Batch(host.type[k * q:(k + 1) * q], host.height[k * q:(k + 1) * q], host.round[k * q:(k + 1) * q],
                     host.valid_round[k * q:(k + 1) * q], host.value[k * q:(k + 1) * q], host.frm[k * q:(k + 1) * q],
                     host.sig[k * q:(k + 1) * q]) for k in range(K)]
        fq = (q - 1) // 2

        def host_loop():
            t0 = time.perf_counter()
            oks = [quorum.check_certificate(v, cut[k], 1, c.round, PRECOMMIT, c.value, fq) for k, c in enumerate(specs)]
            dt = time.perf_counter() - t0
            assert all(oks)
            return dt
        arms["host_loop"] = host_loop
    times = {k: [] for k in arms}
    for rep in range(a.warm + a.reps):
        for k, fn in arms.items():
            dt = fn()
            if rep >= a.warm:
                times[k].append(dt)
    out["us"] = {k: stats(t, 1e6) for k, t in times.items()}
    print(json.dumps(out), flush=True)
    v.close()


if __name__ == "__main__":
    main()
