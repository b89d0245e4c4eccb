"""hyperdrive_amd -- MI355X-native batch authentication + 2f+1 tally for
hyperdrive consensus messages (tuanggolt/hyperdrive's data-parallel hot path).

The compute lives in ``_lib/libhdverify.so`` (HIP, gfx950) behind the C ABI of
``include/hd_verify.h``; this package is its host-side face.
"""
from .verify import (BAD_RECID, BAD_RS, BAD_TYPE, CATCH_NAMES, INFINITY, NO_POINT, NOT_ADMITTED, NOT_AUTHENTIC,
                     SIGNATORY_MISMATCH, VALID, WHEN_NEVER, Batch, CertCheck, CertSpec, CaughtDecideResult, CaughtLogInsertResult,
                     CaughtOrderedDecideResult, DecideLog, DecideResult, EvidenceLogInsertResult, LogInsertResult,
                     OrderedDecideResult, SignatorySets,
                     TallyResult, Verifier, VerifyResult, probe_valu)

__all__ = ["Batch", "Verifier", "VerifyResult", "TallyResult", "DecideResult", "OrderedDecideResult", "DecideLog",
           "LogInsertResult", "CaughtDecideResult", "CaughtOrderedDecideResult", "CaughtLogInsertResult",
           "EvidenceLogInsertResult", "CertSpec", "CertCheck", "SignatorySets", "CATCH_NAMES", "WHEN_NEVER", "probe_valu", "VALID", "BAD_RECID", "BAD_RS",
           "NO_POINT", "INFINITY", "SIGNATORY_MISMATCH", "NOT_ADMITTED", "BAD_TYPE", "NOT_AUTHENTIC"]
