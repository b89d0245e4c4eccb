"""Host-side quorum predicates over a batch tally.

The GPU tally (hd_tally) produces, per (height, round), the sizes of the
first-wins vote logs and the per-value counts; these functions apply the exact
comparisons of the reference's rules to them.  The automaton's step / once-flag
gating (process.go's ``CurrentStep`` checks and ``OnceFlag``) is sequential
control flow and stays with the caller.  So does the guard of process.go:481
(``propose.ValidRound >= CurrentRound`` returns): ``prevote_validround`` is
computed for any ``propose_valid_round > -1``, the propose's own round and
later ones included, and the caller applies ``valid_round < CurrentRound``.

``Verifier.decide`` (hd_decide) evaluates the same eight predicates on the
device for every round of a batch, with the propose taken from the batch's own
propose log (process.go:758-819); its ``decisions`` are these dicts.
``Verifier.decide_ordered`` (hd_decide_ordered) adds the batch index at which
each predicate first holds in batch order, for every height of the batch and
for proposes too: the per-message crossing that is otherwise only available
from the host vote table (hd_votes' events, one height at a time).
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

PREVOTE, PRECOMMIT = 2, 3
INVALID_ROUND = -1
NIL_VALUE = bytes(32)


def thresholds(n_signatories: int) -> Tuple[int, int, int]:
    """f = len(signatories) / 3 (integer division, replica/replica.go:54, 138);
    returns (f, 2f+1, f+1)."""
    f = n_signatories // 3
    return f, 2 * f + 1, f + 1


def decide(tally, height: int, round_: int, f: int, propose_value: Optional[bytes] = None,
           propose_valid: bool = False, propose_valid_round: int = INVALID_ROUND,
           propose_signer_new: bool = False) -> Dict[str, bool]:
    """Predicates for one (height, round) given a tally with ``count``,
    ``distinct`` and ``distinct_any`` maps.

    - timeout_prevote   L34 ``len(PrevoteLogs[r]) >= 2f+1``         process.go:534
    - precommit_nil     L44 #prevotes for NilValue >= 2f+1          process.go:626-632
    - timeout_precommit_reached  L47: the log reached 2f+1 at some insert of
      the batch (``>=``: true iff the equality ``len == 2f+1`` held at the
      crossing insert; the per-insert crossing is hd_votes' EV_PRECOMMIT_2F1,
      or ``when[3]`` / ``exact_until`` of ``Verifier.decide_ordered``)
                                                                    process.go:658
    - timeout_precommit_exact  L47 as StartRound evaluates it on entering the
      round: ``len(PrecommitLogs[r]) == 2f+1`` exactly (more than 2f+1
      buffered precommits never fire it)                   process.go:310, 658
    - skip              L55 |TraceLogs[r]| >= f+1 (votes + valid propose signer) process.go:751
    - precommit_value   L36 #prevotes for propose.Value >= 2f+1     process.go:574-582
    - commit            L49 #precommits for propose.Value >= 2f+1   process.go:696-702
    - prevote_validround L28 #prevotes in validRound for propose.Value >= 2f+1  process.go:486-494
    """
    q = 2 * f + 1
    count = tally.count
    pv = lambda v: count.get((height, round_, PREVOTE, v), 0)
    pc = lambda v: count.get((height, round_, PRECOMMIT, v), 0)
    out = {
        "timeout_prevote": tally.distinct.get((height, round_, PREVOTE), 0) >= q,
        "precommit_nil": pv(NIL_VALUE) >= q,
        "timeout_precommit_reached": tally.distinct.get((height, round_, PRECOMMIT), 0) >= q,
        "timeout_precommit_exact": tally.distinct.get((height, round_, PRECOMMIT), 0) == q,
        "skip": tally.distinct_any.get((height, round_), 0) + (1 if propose_signer_new else 0) >= f + 1,
        "precommit_value": False,
        "commit": False,
        "prevote_validround": False,
    }
    if propose_value is not None and propose_valid:
        out["precommit_value"] = pv(propose_value) >= q
        out["commit"] = pc(propose_value) >= q
    if propose_value is not None and propose_valid_round > INVALID_ROUND:
        out["prevote_validround"] = count.get((height, propose_valid_round, PREVOTE, propose_value), 0) >= q
    return out


def check_certificate(verifier, batch, height: int, round_: int, kind, value: bytes, f: int) -> bool:
    """The receiving side of ``DecideLog.certificate``: are these messages
    2f+1 signed votes of ``kind`` ("prevote" / "precommit", or the type) for
    ``value`` at (height, round)?  The signatures are verified on the device
    against ``verifier``'s signatory set (verify_batch); then, on the host:
    every verdict is VALID, every message has the asked type, height, round
    and value, the Froms are pairwise distinct, and there are at least 2f+1."""
    mtype = {"prevote": PREVOTE, "precommit": PRECOMMIT}.get(kind, kind)
    if mtype not in (PREVOTE, PRECOMMIT):
        raise ValueError(f"{kind!r} is not a vote kind")
    value = bytes(value)
    n = len(batch)
    if n < 2 * f + 1:
        return False
    verdict = verifier.verify_batch(batch, recovered=False).verdict
    if any(int(v) != 0 for v in verdict):                              # VALID
        return False
    for i in range(n):
        if (int(batch.type[i]), int(batch.height[i]), int(batch.round[i])) != (mtype, height, round_):
            return False
        if batch.value[i].tobytes() != value:
            return False
    return len({batch.frm[i].tobytes() for i in range(n)}) == n


def check_certificates(verifier, batch, certs) -> list:
    """Many certificates in one call (``Verifier.check_certificates``,
    hd_check_certificates): ``certs`` are ``verify.CertSpec`` segments of
    ``batch``.  One upload, one verification and one check launch for all of
    them; entry k is True exactly when certificate k is at least ``quorum``
    VALID votes of its kind for its value at its (height, round), from
    pairwise distinct signatories, and nothing else -- what
    :func:`check_certificate` answers for that segment alone."""
    return verifier.check_certificates(batch, certs).ok


def check_certificates_sets(verifier, batch, certs, sets, set_of=None) -> list:
    """The same under several signatory sets
    (``Verifier.check_certificates_sets``, hd_check_certificates_sets):
    certificate k is decided under set ``set_of[k]`` of ``sets`` (a
    ``verify.SignatorySets``; ``set_of=None`` reads each CertSpec's ``set``),
    not under the verifier's own set, which stays as it is.  Entry k is True
    exactly when certificate k is at least ``quorum`` authentic votes of its
    kind for its value at its (height, round), from pairwise distinct members
    of its set, and nothing else."""
    return verifier.check_certificates_sets(batch, certs, sets, set_of).ok


def check_certificates_wire(verifier, kind, buf, certs, sets=None, set_of=None):
    """The same for certificates as they arrive: ``buf`` holds the records
    ``codec.marshal_device(..., with_sig=True)`` (hd_marshal_batch_device)
    produced for votes of one ``kind``, any number of certificates back to
    back; ``certs`` name their segments by record index.  Upload ->
    hd_unmarshal_batch_device -> hd_verify_batch_device ->
    hd_check_certificates_device are queued on one stream, which is
    synchronised once.  Returns the ``verify.CertCheck`` (``.ok`` is the list
    of bool).  A record the buffer ends before decodes to zero bytes (unmarshal
    status 1): its zero signature verifies as BAD_RS, so it is *not valid* to
    the check.

    With ``sets`` (a ``verify.SignatorySets``) certificate k is decided under
    set ``set_of[k]`` of it (``set_of=None``: each CertSpec's ``set``): upload
    -> unmarshal -> hd_verify_batch_device for the verdicts ->
    hd_check_certificates_sets_device, again on one stream with one
    synchronisation, and the verifier's own set decides nothing."""
    import numpy as np
    import torch
    from . import codec
    from .device import DeviceBatch, work_stream
    from .verify import _vote_kind
    mtype = _vote_kind(kind)
    raw = buf if isinstance(buf, torch.Tensor) else torch.from_numpy(np.frombuffer(bytes(buf), np.uint8).copy())
    rec = codec.record_size(mtype, True)
    n = (raw.numel() + rec - 1) // rec
    ws = work_stream()
    with torch.cuda.stream(ws):
        d_buf = torch.zeros(max(raw.numel(), 16), dtype=torch.uint8, device="cuda")
        d_buf[: raw.numel()].copy_(raw, non_blocking=True)
        db = DeviceBatch.empty(n)
        d_verdict = torch.empty(max(n, 1), dtype=torch.uint8, device="cuda")
        d_signer = torch.empty(max(n, 1), dtype=torch.int32, device="cuda")
        d_bitmap = torch.zeros((n + 31) // 32 + 1, dtype=torch.int32, device="cuda")
    if n:
        codec.unmarshal_device(verifier, mtype, d_buf[: raw.numel()], n, with_sig=True, stream=ws, sync=False, out=db)
    if sets is not None:
        if n:
            verifier.verify_batch_device(db.c_struct(), d_verdict.data_ptr(), None, None, None, ws.cuda_stream)
        return verifier.check_certificates_sets_device(db.c_struct(), d_verdict.data_ptr(), certs, sets, set_of,
                                                       ws.cuda_stream)
    if n:
        verifier.verify_batch_device(db.c_struct(), d_verdict.data_ptr(), None, d_signer.data_ptr(),
                                     d_bitmap.data_ptr(), ws.cuda_stream)
    return verifier.check_certificates_device(db.c_struct(), d_bitmap.data_ptr(), d_signer.data_ptr(),
                                              verifier.n_signatories, certs, ws.cuda_stream)


def decide_votes(votes, round_: int, f: int, propose_value: Optional[bytes] = None, propose_valid: bool = False,
                 propose_valid_round: int = INVALID_ROUND) -> Dict[str, bool]:
    """The same predicates as :func:`decide`, for the current height of an
    incremental :class:`hyperdrive_amd.votes.VoteLog` (include/hd_votes.h):
    every value is one O(1) lookup where process.go runs its O(n) loops.  A
    valid propose's signer is already in the log's trace (trace_propose)."""
    q = 2 * f + 1
    out = {
        "timeout_prevote": votes.len(PREVOTE, round_) >= q,                 # process.go:534
        "precommit_nil": votes.count(PREVOTE, round_, NIL_VALUE) >= q,     # 626-632
        "timeout_precommit_reached": votes.len(PRECOMMIT, round_) >= q,    # 658 (crossed at some insert)
        "timeout_precommit_exact": votes.len(PRECOMMIT, round_) == q,      # 310 + 658 (StartRound's ==)
        "skip": votes.trace_len(round_) >= f + 1,                          # 751
        "precommit_value": False,
        "commit": False,
        "prevote_validround": False,
    }
    if propose_value is not None and propose_valid:
        out["precommit_value"] = votes.count(PREVOTE, round_, propose_value) >= q     # 574-582
        out["commit"] = votes.count(PRECOMMIT, round_, propose_value) >= q            # 696-702
    if propose_value is not None and propose_valid_round > INVALID_ROUND:
        out["prevote_validround"] = votes.count(PREVOTE, propose_valid_round, propose_value) >= q  # 486-494
    return out
