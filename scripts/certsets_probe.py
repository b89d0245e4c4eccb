"""What checking certificates under several signatory sets costs
(hd_check_certificates_sets_device), next to the only way there was before it:
group the certificates by set and, per group, hd_set_signatories on the live
context, then hd_verify_batch_device and hd_check_certificates_device (DESIGN §5
"Certificates under several sets").

On one GPU, in one process.  The votes come from the generator's rounds shape
(kind 1: height 1, `--sets` x `--signers` signatories, one round = 1 propose + S
prevotes + S precommits, 90 % of them for the round's canonical value),
generated on the device.  Signatory set g is signatories g * signers ..
(g + 1) * signers - 1.  A certificate is `--votes` precommits of one round for
its canonical value from the signers of one set, gathered on the device into
one batch of `--certs` x `--votes` messages, the certificates of a set next to
each other.  The measured context's own admitted set is `--signers` rows that
signed nothing: every signer lies outside it, so the verification is the full
recovery or the foreign-key block, never the per-key tables.

Arms, alternated inside every repetition (the admitted set is put back before
`sets` and `check` run; that is not timed):

  sets      hd_verify_batch_device for the verdicts of the whole batch, then
            hd_check_certificates_sets_device: host clock, the call returns
            synchronised
  check     the second call alone over ready verdicts: HIP events around it
  grouped   per set: hd_set_signatories, hd_verify_batch_device on that group's
            messages, hd_check_certificates_device: host clock over all groups
            (hd_set_signatories blocks; each check returns synchronised)

Medians of `--reps` after `--warm`, with p10 and p90, in microseconds, as one
JSON line.  Every arm's answers are compared once before anything is timed.

    python scripts/certsets_probe.py [--certs 1000] [--votes 667] [--sets 4] [--signers 1000] [--reps 7] [--warm 2]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--certs", type=int, default=1000)
    ap.add_argument("--votes", type=int, default=667)
    ap.add_argument("--sets", type=int, default=4)
    ap.add_argument("--signers", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warm", type=int, default=2)
    a = ap.parse_args()

    import torch
    from hyperdrive_amd.device import DeviceBatch, generate, work_stream
    from hyperdrive_amd.verify import PRECOMMIT, CertSpec, Verifier, cert_rows
    if not torch.cuda.is_available():
        raise SystemExit("certsets_probe: no GPU visible (nothing is measured on the CPU)")
    G, Sg, K, q = a.sets, a.signers, a.certs, a.votes
    S = G * Sg
    if K % G:
        raise SystemExit("certsets_probe: --certs is a multiple of --sets")
    rounds = K // G   # one certificate per set and round

    maker = Verifier(0)
    ks = maker.gen_keys(S)
    maker.set_signatories(ks[0])
    src, _, _ = generate(maker, 1, rounds * (2 * S + 1), S, 0, keys=ks)
    torch.cuda.synchronize()
    maker.close()
    sets = [ks[0][g * Sg:(g + 1) * Sg].copy() for g in range(G)]

    # certificate (g, r): the first q precommits of round r for its canonical value from set g's signers
    h_type, h_round = src.type.cpu().numpy(), src.round.cpu().numpy()
    h_value, h_from = src.value.cpu().numpy(), src.frm.cpu().numpy()
    owner = {ks[0][j].tobytes(): j // Sg for j in range(S)}
    picks = [[] for _ in range(G)]
    for r in range(rounds):
        lo = r * (2 * S + 1)
        canon = h_value[lo]                                   # the round's propose carries the canonical value
        ok = (h_type[lo:lo + 2 * S + 1] == PRECOMMIT) & (h_value[lo:lo + 2 * S + 1] == canon).all(1)
        pos = lo + np.nonzero(ok)[0]
        of = np.array([owner[h_from[p].tobytes()] for p in pos])
        for g in range(G):
            mine = pos[of == g]
            assert len(mine) >= q, "a round with too few precommits of one set for its canonical value"
            picks[g].append((mine[:q], int(h_round[lo]), canon.tobytes()))
    order = [(g, t) for g in range(G) for t in picks[g]]      # the certificates of a set next to each other
    gather = torch.from_numpy(np.concatenate([t[0] for _, t in order]).astype(np.int64)).to("cuda")
    n = K * q

    def cut(ix):
        return DeviceBatch(len(ix), src.type[ix], src.height[ix], src.round[ix], src.valid_round[ix],
                           src.value[ix].contiguous(), src.frm[ix].contiguous(), src.sig[ix].contiguous())

    db = cut(gather)
    per = rounds * q                                           # messages of one set's group
    groups = [cut(gather[g * per:(g + 1) * per]) for g in range(G)]
    specs = [CertSpec(k * q, q, PRECOMMIT, 1, t[1], t[2], q, g) for k, (g, t) in enumerate(order)]
    group_rows = [cert_rows([CertSpec(k * q, q, PRECOMMIT, 1, t[1], t[2], q) for k, t in enumerate(picks[g])])
                  for g in range(G)]
    torch.cuda.synchronize()
    del src
    print("workload ready: %d messages" % n, file=sys.stderr, flush=True)

    v = Verifier(0)
    outside = np.random.default_rng(5).integers(0, 256, (Sg, 32), dtype=np.uint8)
    v.set_signatories(outside)
    ss = v.open_sets()
    assert [ss.add(s) for s in sets] == list(range(G))
    ws = work_stream()
    with torch.cuda.stream(ws):
        verdict = torch.empty(n, dtype=torch.uint8, device="cuda")
        signer = torch.empty(per, dtype=torch.int32, device="cuda")
        bitmap = torch.zeros((per + 31) // 32, dtype=torch.int32, device="cuda")
    ws.synchronize()
    cs, s = db.c_struct(), ws.cuda_stream
    rows, set_of = cert_rows(specs), [g for g, _ in order]

    def check():
        return v.check_certificates_sets_device(cs, verdict.data_ptr(), rows, ss, set_of, s)

    def arm_sets():
        t0 = time.perf_counter()
        v.verify_batch_device(cs, verdict.data_ptr(), None, None, None, s)
        res = check()
        return time.perf_counter() - t0, res

    def arm_check():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(ws)
        res = check()
        e1.record(ws)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3, res

    def arm_grouped():
        out = []
        t0 = time.perf_counter()
        for g in range(G):
            v.set_signatories(sets[g])
            v.verify_batch_device(groups[g].c_struct(), verdict.data_ptr(), None, signer.data_ptr(), bitmap.data_ptr(), s)
            out.append(v.check_certificates_device(groups[g].c_struct(), bitmap.data_ptr(), signer.data_ptr(), Sg,
                                                   group_rows[g], s))
        return time.perf_counter() - t0, out

    _, res = arm_sets()
    assert res.ok == [True] * K and res.good.tolist() == [q] * K, "every certificate is OK under its set"
    assert int(verdict.max()) == 6 and int(verdict.min()) == 6, "every signer is outside the admitted set"
    _, parts = arm_grouped()
    assert all(p.ok == [True] * rounds for p in parts)
    v.set_signatories(outside)
    out = {"certs": K, "votes": q, "messages": n, "sets": G, "signers_per_set": Sg,
           "plan": Verifier.cert_plan(Sg, K), "foreign": list(v.foreign_stats())}

    times = {"sets": [], "check": [], "grouped": []}
    for rep in range(a.warm + a.reps):
        dts = [arm_sets()[0], arm_check()[0], arm_grouped()[0]]
        v.set_signatories(outside)
        print("rep %d: %s" % (rep, " ".join("%.0f" % (1e6 * dt) for dt in dts)), file=sys.stderr, flush=True)
        if rep >= a.warm:
            for k, dt in zip(times, dts):
                times[k].append(dt)
    out["us"] = {k: stats(t, 1e6) for k, t in times.items()}
    print(json.dumps(out), flush=True)
    ss.close()
    v.close()


if __name__ == "__main__":
    main()
