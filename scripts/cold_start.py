"""What importing the signatories' public keys buys at a cold start
(hd_import_keys).  C2's shape: 100 signatories, 1M honest votes,
the table width the context picks itself.  One arm per process, one JSON line
each, so that every step runs under its own timeout:

    timeout -k 10 300 python scripts/cold_start.py --arm cold
    timeout -k 10 300 python scripts/cold_start.py --arm import
    timeout -k 10 300 python scripts/cold_start.py --arm retier

cold    set_signatories -> the first verify_batch_device (full recovery of every
        message, key learning, table build), then three steady-state calls.
        Needs nothing of this change: with HD_LIB naming another build of the
        library (the parent commit's) it measures that build.
import  a donor context learns the keys and exports them; a fresh context then
        times set_signatories, import_keys alone, the first verify call after
        the import, and three steady-state calls.
retier  a set change across a table-width boundary: a context learns 29
        signatories (the pick is printed; 22-bit tables at the default budget)
        and three steady-state calls are timed; set_signatories to those 29 plus
        one more (20 bits) is timed, then the first verify call after it with
        its fallback count, then three steady-state calls.  With HD_LIB naming
        the parent commit's build it measures what a crossing cost before the
        keys were carried over it.

Times are host wall clock around a call and the synchronisation of its stream.
The first call of a context also allocates its per-call scratch (63 words per
message and the fallback lists), in either arm; `second_s` shows a call
without that."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

N, S = 1 << 20, 100
S_RETIER = 29   # the largest set the default budget gives 22-bit tables; one more takes 20 bits


def retier(a):
    import torch
    import hyperdrive_amd as hd
    from hyperdrive_amd.device import generate, work_stream
    ws = work_stream()
    verdict = torch.empty(N, dtype=torch.uint8, device="cuda")
    out = {"arm": a.arm, "n": N, "signatories": [S_RETIER, S_RETIER + 1], "lib": os.environ.get("HD_LIB", "in-tree")}

    def timed(f):
        torch.cuda.synchronize()
        t = time.perf_counter()
        f()
        ws.synchronize()
        return round(time.perf_counter() - t, 5)

    v = hd.Verifier(0)
    sigs, foreign = v.gen_keys(S_RETIER + 1)
    db, _, _ = generate(v, 0, N, S_RETIER + 1, 0, keys=(sigs, foreign))
    cb = db.c_struct()
    verify = lambda: v.verify_batch_device(cb, verdict.data_ptr(), None, None, None, ws.cuda_stream)
    out["set_signatories_before_s"] = timed(lambda: v.set_signatories(sigs[:S_RETIER]))
    out["key_windows_before"] = v.fastpath_geometry()[1]
    out["learn_s"] = [timed(verify) for _ in range(2)]
    out["known_before"] = v.known_keys()
    out["steady_before_s"] = [timed(verify) for _ in range(3)]
    out["steady_before_fallback"] = v.fastpath_stats()[1]   # the one signer that is not admitted yet
    out["set_change_s"] = timed(lambda: v.set_signatories(sigs))
    out["key_windows_after"] = v.fastpath_geometry()[1]
    if hasattr(v._lib, "hd_ctx_set_change_info"):
        out["set_change"] = v.last_set_change()
    out["known_after_set_change"] = v.known_keys()
    out["first_batch_s"] = timed(verify)
    out["first_batch_fallback"] = v.fastpath_stats()[1]
    out["first_batch_valid"] = int((verdict == 0).sum().item())
    out["messages_of_new_signer"] = len(range(S_RETIER, N, S_RETIER + 1))
    out["steady_s"] = [timed(verify) for _ in range(3)]
    out["steady_fallback"] = v.fastpath_stats()[1]
    out["known_end"] = v.known_keys()
    v.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arm", choices=["cold", "import", "retier"], required=True)
    a = ap.parse_args()
    if a.arm == "retier":
        return retier(a)
    import torch
    import hyperdrive_amd as hd
    from hyperdrive_amd.device import generate, work_stream
    ws = work_stream()
    verdict = torch.empty(N, dtype=torch.uint8, device="cuda")
    out = {"arm": a.arm, "n": N, "signatories": S, "lib": os.environ.get("HD_LIB", "in-tree")}

    def timed(f):
        torch.cuda.synchronize()
        t = time.perf_counter()
        f()
        ws.synchronize()
        return round(time.perf_counter() - t, 5)

    donor = hd.Verifier(0)
    sigs, foreign = donor.gen_keys(S)
    db, _, _ = generate(donor, 0, N, S, 0, keys=(sigs, foreign))
    cb = db.c_struct()
    verify = lambda v: v.verify_batch_device(cb, verdict.data_ptr(), None, None, None, ws.cuda_stream)
    keys = None
    if a.arm == "import":
        # 13-bit tables (0.5 GB): with the default width the donor frees 41 GB
        # right before the timed context allocates as much, and that context's
        # set_signatories then took 1.45 s instead of 4 ms
        donor.set_variant("key_width", 13)
        donor.set_signatories(sigs)
        verify(donor)
        ws.synchronize()
        keys, known = donor.export_keys()
        assert known.all()
    donor.close()

    v = hd.Verifier(0)
    out["set_signatories_s"] = timed(lambda: v.set_signatories(sigs))
    if keys is not None:
        out["import_keys_s"] = timed(lambda: v.import_keys(keys))
        out["known_after_import"] = v.known_keys()
    out["first_batch_s"] = timed(lambda: verify(v))
    out["first_batch_fallback"] = v.fastpath_stats()[1]
    out["first_batch_valid"] = int((verdict == 0).sum().item())
    out["second_s"] = timed(lambda: verify(v))
    out["steady_s"] = [timed(lambda: verify(v)) for _ in range(3)]
    out["key_windows"] = v.fastpath_geometry()[1]
    v.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
