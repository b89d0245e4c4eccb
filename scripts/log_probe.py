"""What an insert into the retained log (hd_log) costs as the log grows, next to
the one-batch ordered decide and the host vote table.

On one GPU, in one process: the C3 shape restricted to one height (kind 1:
height 1, 1,000 signatories, f = 333, four rounds of 1 propose + 1,000 prevotes
+ 1,000 precommits = 8,004 distinct messages).  A stream of 128,000 messages
is drawn from those with repetition, in random order, verified on the device
and fed as 16 pieces of 8,000.  Per piece, after warm-up:

  insert           hd_log_insert_device_bitmap of the piece into a log holding
                   the pieces before it (`base` entries)
  decide_ordered   hd_decide_ordered_device_bitmap of the piece alone
  host_votes       hd_votes_insert_batch of the piece into a host table holding
                   the pieces before it (votes only: it knows no proposes)

With --catch the insert is timed twice more (hd_log_insert_catch_device_bitmap):

  insert_catch           the same insert plus the catch list
  insert_catch_noclass   the same with out->dup and out->pclass NULL: what a
                         replica that wants only the list pays, against
                         `insert` with both arrays

With --evidence (and --catch) once more, with both whole messages of every
record (hd_log_insert_evidence_device_bitmap):

  insert_evidence        insert_catch plus the evidence rows

--keep-sigs makes the log keep signatures (hd_log_keep_signatures), so every
figure above is that of a log holding whole messages.  Where the build has
hd_log_read, the whole log is read back at the end:

  read                   hd_log_read of every entry (host wall time: the call
                         runs on the context's stream and ends synchronised)

--adv P draws the stream from a batch with P % adversarial messages, so that
there is something to catch (0, the default, repeats messages but never
conflicts); --only-insert leaves out decide_ordered and host_votes.

Each device call sits between two events on its stream (kernels and the
download; the call ends in a stream synchronise).  A repetition resets the log
and feeds the 16 pieces in order, so every piece is timed at the same `base`
each time.  One JSON line with per-piece medians in milliseconds.  With HD_LIB
naming an older build only the entry points it has are run, so two builds can
be compared by running the script once per build in one job.

    python scripts/log_probe.py [--reps 20] [--pieces 16] [--piece 8000] [--catch] [--adv 0] [--only-insert]
                                 [--keep-sigs] [--evidence]
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


def med(rows):
    return [round(float(np.median(r)), 4) for r in rows]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--pieces", type=int, default=16)
    ap.add_argument("--piece", type=int, default=8000, help="messages per piece (a multiple of 32)")
    ap.add_argument("--signers", type=int, default=1000)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--label", default=os.environ.get("HD_LIB", "tree"))
    ap.add_argument("--catch", action="store_true", help="also time the insert with the catch list")
    ap.add_argument("--adv", type=int, default=0, help="adversarial messages in the source batch, per cent")
    ap.add_argument("--only-insert", action="store_true", help="leave out decide_ordered and host_votes")
    ap.add_argument("--keep-sigs", action="store_true", help="the log keeps signatures (hd_log_keep_signatures)")
    ap.add_argument("--evidence", action="store_true", help="with --catch: also time the insert with evidence")
    a = ap.parse_args()
    if a.piece % 32:
        raise SystemExit("log_probe: --piece must be a multiple of 32 (the bitmap is sliced by words)")

    import torch
    from hyperdrive_amd import _lib, quorum
    from hyperdrive_amd.device import DeviceBatch, generate, work_stream
    from hyperdrive_amd.verify import Batch, Verifier
    from hyperdrive_amd.votes import VoteLog
    if not torch.cuda.is_available():
        raise SystemExit("log_probe: no GPU visible (nothing is measured on the CPU)")
    lib = _lib.load()
    S, P, m = a.signers, a.pieces, a.piece
    distinct, n = a.rounds * (2 * S + 1), a.pieces * a.piece
    v = Verifier(0)
    ks = v.gen_keys(S)
    v.set_signatories(ks[0])
    src, _, _ = generate(v, 1, distinct, S, a.adv, keys=ks)
    pick = torch.from_numpy(np.random.default_rng(1).integers(0, distinct, n)).cuda()
    db = DeviceBatch(n, *(getattr(src, k)[pick].contiguous() for k in ("type", "height", "round", "valid_round",
                                                                       "value", "frm", "sig")))
    ws = work_stream()
    with torch.cuda.stream(ws):
        verdict = torch.empty(n, dtype=torch.uint8, device="cuda")
        bitmap = torch.zeros((n + 31) // 32, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    s = ws.cuda_stream
    for _ in range(2):
        v.verify_batch_device(db.c_struct(), verdict.data_ptr(), None, None, bitmap.data_ptr(), s)
    ws.synchronize()
    assert a.adv or int((verdict == 0).sum().item()) == n
    f = quorum.thresholds(S)[0]
    sched = torch.from_numpy(np.ascontiguousarray(ks[0])).cuda()
    torch.cuda.synchronize()
    parts = [(db.rows(k * m, m).c_struct(), bitmap.data_ptr() + 4 * (k * m // 32)) for k in range(P)]
    out = {"label": a.label, "n": n, "piece": m, "S": S, "f": f, "rounds": a.rounds, "distinct": distinct}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record(ws)
        fn()
        e1.record(ws)
        e1.synchronize()
        return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3

    # the piece alone through the one-batch ordered decide
    if hasattr(lib, "hd_decide_ordered_device_bitmap") and not a.only_insert:
        cin = _lib.HdDecideIn(f, S, sched.data_ptr(), None)
        o, _oa = v._decide_struct(m)
        w, _when, _until = v._order_struct(m)
        dev = [[] for _ in range(P)]
        for rep in range(a.warm + a.reps):
            for k, (cs, bm) in enumerate(parts):
                def call():
                    assert lib.hd_decide_ordered_device_bitmap(v.handle, ctypes.byref(cs), bm, ctypes.byref(cin),
                                                               ctypes.byref(o), ctypes.byref(w), s) == 0
                d, _ = timed(call)
                if rep >= a.warm:
                    dev[k].append(d)
        out["decide_ordered_ms"] = med(dev)

    # the retained log
    if hasattr(lib, "hd_log_insert_device_bitmap"):
        if a.keep_sigs and not hasattr(lib, "hd_log_keep_signatures"):
            raise SystemExit("log_probe: --keep-sigs needs a build with hd_log_keep_signatures")
        log = v.open_log(1, f, ks[0], keep_signatures=a.keep_sigs)
        out["keep_sigs"] = a.keep_sigs
        o2, _oa2 = v._decide_struct(m, distinct + m)            # rows: at most one per distinct message
        w2, _w2, _u2 = v._order_struct(distinct + m)
        logpos = np.zeros(m, np.uint32)
        info = _lib.HdLogInfo(0, 0, 0, logpos.ctypes.data)
        dev, host, base, kept, rows = [[] for _ in range(P)], [[] for _ in range(P)], [0] * P, [0] * P, [0] * P
        for rep in range(a.warm + a.reps):
            log.reset(1)
            for k, (cs, bm) in enumerate(parts):
                def call():
                    rc = lib.hd_log_insert_device_bitmap(log.handle, ctypes.byref(cs), bm, None, ctypes.byref(o2),
                                                         ctypes.byref(w2), ctypes.byref(info), s)
                    assert rc == 0, rc
                d, h = timed(call)
                assert info.relogged == info.base
                base[k], kept[k], rows[k] = info.base, info.kept, o2.n
                if rep >= a.warm:
                    dev[k].append(d)
                    host[k].append(h)
        out.update(base=base, kept=kept, rows=rows, insert_ms=med(dev), insert_host_ms=med(host),
                   entries=log.entries)
        # the same inserts with the catch list, with and without the class arrays
        if a.catch and hasattr(lib, "hd_log_insert_catch_device_bitmap"):
            from hyperdrive_amd.verify import _catch_struct
            c, _ca = _catch_struct(m)
            o3, _oa3 = v._decide_struct(m, distinct + m)
            o3.dup = o3.pclass = None
            for key, oo in (("insert_catch_ms", o2), ("insert_catch_noclass_ms", o3)):
                dev, caught = [[] for _ in range(P)], [0] * P
                for rep in range(a.warm + a.reps):
                    log.reset(1)
                    for k, (cs, bm) in enumerate(parts):
                        def call():
                            rc = lib.hd_log_insert_catch_device_bitmap(log.handle, ctypes.byref(cs), bm, None,
                                                                       ctypes.byref(oo), ctypes.byref(w2),
                                                                       ctypes.byref(info), ctypes.byref(c), s)
                            assert rc == 0, rc
                        d, _ = timed(call)
                        assert info.relogged == info.base
                        caught[k] = c.n
                        if rep >= a.warm:
                            dev[k].append(d)
                out[key] = med(dev)
                assert out.setdefault("caught", caught) == caught   # the same records either way
            if a.evidence and hasattr(lib, "hd_log_insert_evidence_device_bitmap"):
                e, _eo, _ea = log._evidence_struct(m)
                dev = [[] for _ in range(P)]
                for rep in range(a.warm + a.reps):
                    log.reset(1)
                    for k, (cs, bm) in enumerate(parts):
                        def call():
                            rc = lib.hd_log_insert_evidence_device_bitmap(log.handle, ctypes.byref(cs), bm, None,
                                                                          ctypes.byref(o2), ctypes.byref(w2),
                                                                          ctypes.byref(info), ctypes.byref(c),
                                                                          ctypes.byref(e), s)
                            assert rc == 0, rc
                        d, _ = timed(call)
                        assert e.offender.n == e.against.n == c.n == out["caught"][k]
                        if rep >= a.warm:
                            dev[k].append(d)
                out["insert_evidence_ms"] = med(dev)
        if hasattr(lib, "hd_log_read"):   # every loop above leaves the log full
            from hyperdrive_amd.verify import _rows_struct
            L = log.entries
            r, _ra = _rows_struct(L, a.keep_sigs)
            wall = []
            for rep in range(a.warm + a.reps):
                t0 = time.perf_counter()
                rc = lib.hd_log_read(log.handle, None, 0, L, ctypes.byref(r))
                wall.append((time.perf_counter() - t0) * 1e3)
                assert rc == 0 and r.n == L, rc
            out.update(read_entries=L, read_ms=round(float(np.median(wall[a.warm:])), 4))
        log.close()

    if not a.only_insert:
        # the host vote table, accumulating like the log
        hb = db.to_host()
        vd = verdict.cpu().numpy()
        hparts = []
        for k in range(P):
            sl = Batch(*(np.ascontiguousarray(x[k * m:(k + 1) * m]) for x in (hb.type, hb.height, hb.round, hb.valid_round,
                                                                              hb.value, hb.frm, hb.sig)))
            hparts.append((sl, sl.c_struct(), np.ascontiguousarray(vd[k * m:(k + 1) * m])))
        st, dbl, ev = np.zeros(m, np.uint8), np.zeros(m, np.uint32), np.zeros(m, np.uint8)
        ins = ctypes.c_uint32()
        vl = VoteLog(1)
        vl.set_f(f)
        hv = [[] for _ in range(P)]
        for rep in range(1 + min(a.reps, 5)):
            lib.hd_votes_reset(vl._v, 1)
            for k, (_sl, cs, pv) in enumerate(hparts):
                t0 = time.perf_counter()
                rc = lib.hd_votes_insert_batch(vl._v, ctypes.byref(cs), pv.ctypes.data, st.ctypes.data, dbl.ctypes.data,
                                               ev.ctypes.data, ctypes.byref(ins))
                t1 = time.perf_counter()
                assert rc == 0, rc
                if rep:
                    hv[k].append((t1 - t0) * 1e3)
        vl.close()
        out["host_votes_ms"] = med(hv)
    print(json.dumps(out), flush=True)
    v.close()


if __name__ == "__main__":
    main()
