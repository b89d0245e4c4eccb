"""The known-key check's per-call plan and the variant table (hd_fastplan.h),
through the host build (tests/native/hd_host_check.cpp): no GPU.

Every expected value is written out from the rules as include/hd_verify.h and
DESIGN.md state them; the defaults are literals, not read back from the table."""
from __future__ import annotations

import itertools

import pytest

NONE = 0xFFFFFFFF
KEY = {"verify_waves": 0, "sum_waves": 1, "split_k": 4, "recover_g": 5, "key_width": 7,
       "wave_prio": 8, "sum_cap": 9, "foreign_keys": 10, "slow_lift": 11, "dedup": 12, "lean_inv": 13,
       "sum_chain": 14, "pre_share": 15}
DEFAULTS = {"verify_waves": 3, "sum_waves": 0, "split_k": -1, "recover_g": 0, "key_width": 0,
            "wave_prio": 0, "sum_cap": 1, "foreign_keys": 16, "slow_lift": 1, "dedup": 1, "lean_inv": 1,
            "sum_chain": 1, "pre_share": 1}
# removed (3, 6 in round 5; 2, the sums' prefetch depth, once depth 2 had lost every A/B): key -> the value get
# still returns
REMOVED = {2: 1, 3: 0, 6: 2}
SWITCHES = ("recover_g", "sum_cap", "slow_lift", "dedup", "lean_inv", "sum_chain", "pre_share")


def plan(hostmath, n, est=(NONE, NONE, NONE, NONE), n_cu=256, auth=False, caller_digests=False, **variants):
    var = [0] * 16
    for name, v in DEFAULTS.items():
        var[KEY[name]] = v
    for k, v in REMOVED.items():
        var[k] = v
    for name, v in variants.items():
        var[KEY[name]] = v
    return hostmath.fb_plan(var, n_cu, n, auth, caller_digests, est)


def test_keys_match_the_python_names():
    from hyperdrive_amd.verify import Verifier
    assert Verifier.VARIANTS == KEY


def test_messages_per_inversion(hostmath):
    k = lambda n, e2=NONE, e3=NONE, **kw: plan(hostmath, n, (NONE, NONE, e2, e3), **kw)["k"]
    assert k(2 ** 19 - 1) == 8 and k(2 ** 19) == 16
    assert k(2 ** 20, 1, 2) == 16                      # 2^19 lanes
    assert k(2 ** 20, 2 ** 19 - 1, 2 ** 20) == 8       # 2^19 - 1 lanes
    # estimates that say nothing: lanes = n
    for e2, e3 in ((0, 2), (3, 2), (NONE, 2), (1, NONE)):
        assert k(2 ** 19, e2, e3) == 16, (e2, e3)
        assert k(2 ** 19 - 1, e2, e3) == 8, (e2, e3)
    assert k(2 ** 20, split_k=8) == 8 and k(1, split_k=16) == 16
    assert k(2 ** 20, 1, 2 ** 20, split_k=16) == 16 and k(2 ** 20, split_k=-1) == 16


def test_sums_waves(hostmath):
    w = lambda n, **kw: plan(hostmath, n, **kw)["waves"]
    assert w(393215) == 4 and w(393216) == 3           # 2 * 3 * 4 * 64 * 256
    assert w(1535, n_cu=0) == 4 and w(1536, n_cu=0) == 3
    assert w(1535, n_cu=1) == 4 and w(1536, n_cu=1) == 3
    for forced in (2, 3, 4):
        assert w(393215, sum_waves=forced) == forced and w(393216, sum_waves=forced) == forced


def test_overlap(hostmath):
    n = 393216
    p = lambda e0=NONE, **kw: plan(hostmath, n, (e0, NONE, NONE, NONE), **kw)
    assert p(3072)["overlap"] == 1 and p(3073)["overlap"] == 0 and p(NONE)["overlap"] == 1
    assert p(0)["overlap"] == 1
    assert p(auth=True)["overlap"] == 0
    assert p(sum_waves=4)["overlap"] == 0
    two = p(sum_waves=2)
    assert two["overlap"] == 1 and two["capped"] == 0 and two["lean"] == 1 and two["chain"] == 1
    assert plan(hostmath, n - 1)["overlap"] == 0       # the 4-wave sums of a small batch


def test_capped_lean_chain_follow_their_variants_on_the_overlap_path(hostmath):
    n = 393216
    for cap, lean, chain in itertools.product((0, 1), repeat=3):
        on = plan(hostmath, n, sum_cap=cap, lean_inv=lean, sum_chain=chain)
        assert (on["overlap"], on["capped"], on["lean"], on["chain"]) == (1, cap, lean, chain)
    off = plan(hostmath, n, (3073, NONE, NONE, NONE), sum_cap=1, lean_inv=1, sum_chain=1)
    assert (off["overlap"], off["capped"], off["lean"], off["chain"]) == (0, 0, 0, 0)
    off = plan(hostmath, n, auth=True)
    assert (off["overlap"], off["capped"], off["lean"], off["chain"]) == (0, 0, 0, 0)


# (waves asked for, the retired key 2's fixed value, the form: k_fast_sums' WAVES and the prefetch depth that
# form has -- 0 for the 4-wave form, which loads its points when used, else 1)
@pytest.mark.parametrize("waves,pf,form", [(2, 1, (2, 1)), (3, 1, (3, 1)), (4, 1, (4, 0))])
def test_sums_form(hostmath, waves, pf, form):
    assert hostmath.variant(2, pf)[:2] == (pf, False)   # get reads 1, set rejects even that
    p = plan(hostmath, 393216, sum_waves=waves)
    assert p["waves"] == waves and (p["sums_waves"], p["sums_pf"]) == form
    assert p["capped"] == (1 if waves == 3 else 0)
    # the rule's own choice of 4 and of 3 waves takes the same forms
    auto = plan(hostmath, 393215 if waves == 4 else 393216)
    if waves != 2:
        assert auto["waves"] == waves and (auto["sums_waves"], auto["sums_pf"]) == form
    # whatever key 2 of a variant vector holds, the plan is the same
    var = [3, waves, 2, 0, -1, 0, 2, 0, 0, 1, 16, 1, 1, 1, 1, 1]
    assert hostmath.fb_plan(var, 256, 393216, False, False, (NONE,) * 4) == p


def test_share_dedup_lift(hostmath):
    n = 2 ** 20
    for share in (0, 1):
        assert plan(hostmath, n, pre_share=share)["share"] == share
        assert plan(hostmath, n, pre_share=share, caller_digests=True)["share"] == 0
    for dedup in (0, 1):
        assert plan(hostmath, n, dedup=dedup)["dedup"] == dedup
    est = (13108, 2 ** 20, NONE, NONE)   # 65 blocks by [0], all 1024 by [1]
    with_lift, without = plan(hostmath, n, est, slow_lift=1), plan(hostmath, n, est, slow_lift=0)
    assert (with_lift["lift"], with_lift["lift_blocks"], with_lift["slow_blocks"]) == (1, 65, 1024)
    assert (without["lift"], without["lift_blocks"], without["slow_blocks"]) == (0, 65, 65)


def test_fallback_grids(hostmath):
    for e in (0, 1, 1000, 2 ** 20, NONE - 1, NONE):
        p = plan(hostmath, 1000, (e, e, NONE, NONE))
        assert (p["full"], p["lift_blocks"], p["slow_blocks"]) == (4, 4, 4), e
    for e, want in ((0, 64), (13107, 64), (13108, 65), (2 ** 20, 1024), (NONE, 1024)):
        p = plan(hostmath, 2 ** 20, (e, e, NONE, NONE))
        assert (p["full"], p["lift_blocks"], p["slow_blocks"]) == (1024, want, want), e
    # full is capped by four blocks per CU, and by one block where n_cu is 0
    assert plan(hostmath, 2 ** 20, n_cu=8)["full"] == 32
    assert plan(hostmath, 2 ** 20, n_cu=0)["full"] == 4
    assert plan(hostmath, 1)["full"] == 1 and plan(hostmath, 257)["full"] == 2


def test_variant_defaults(hostmath):
    for name, want in DEFAULTS.items():
        assert hostmath.variant(KEY[name], 0)[0] == want, name
    for key, fixed in REMOVED.items():
        assert hostmath.variant(key, 0)[0] == fixed
    assert hostmath.variant(-1, 0) is None and hostmath.variant(16, 0) is None


def test_variant_accepted_values(hostmath):
    ok = lambda name, v: hostmath.variant(KEY[name], v)[1]
    accepted = lambda name, lo, hi: [v for v in range(lo, hi + 1) if ok(name, v)]
    for key in REMOVED:
        assert not any(hostmath.variant(key, v)[1] for v in range(-2, 70))
    assert accepted("verify_waves", -2, 8) == [2, 3, 4]
    assert accepted("sum_waves", -2, 8) == [0, 2, 3, 4]
    assert [v for v in range(-2, 9) if hostmath.variant(2, v)[1]] == []   # the prefetch depth: retired
    assert accepted("split_k", -3, 40) == [-1, 8, 16]
    assert accepted("wave_prio", -2, 8) == [0, 1, 2, 3]
    assert accepted("foreign_keys", -2, 70) == list(range(0, 65))
    for name in SWITCHES:
        assert accepted(name, -2, 4) == [0, 1], name
    widths = hostmath.variant(KEY["key_width"], 0)[2]
    assert widths[1:] == [20, 22, 13] and len(set(widths)) == 4   # (the host build narrows HD_FB_W)
    assert accepted("key_width", -2, 70) == sorted([0] + widths)
