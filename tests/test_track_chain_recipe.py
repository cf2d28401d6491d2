"""CPU partner of tests/test_track_chain_gpu.py: the cases of tests/track_chain_ref.py are LIVE.  A grid on which the estimator finds no
model everywhere would compare identities on the GPU; here the reference side of every case is held to what the recipe promises, on the
oracle alone: the live group (outlier share <= 0.3, at least 63 kept pairs, no lens) finds the generating motion, the model minima refuse
and accept where they must, the lens cases drop pairs on both sides."""
import numpy as np
import pytest

from tests import track_chain_ref as T


def _ref(oracle, c):
    prev, matched, status, _ = c.arrays
    return T.reference(oracle, prev, matched, status, c.n, c.und(oracle, c.n), c.region, c.threshold, c.full)


def test_the_case_list_covers_what_it_must():
    live = [c for c in T.CASES if c.live]
    assert 200 >= len(T.CASES) >= 120 and len(live) >= 40
    for n in T.N_EDGES:
        assert any(c.n == n for c in T.CASES), n
        assert any(c.kept == n for c in T.CASES), f"no case keeps exactly {n} pairs"
    for name, values, get in [("region", T.REGIONS, lambda c: c.region), ("motion", T.MOTIONS, lambda c: c.motion), ("share", T.SHARES, lambda c: c.share),
                              ("threshold", T.THRESHOLDS, lambda c: c.threshold), ("pattern", T.PATTERNS, lambda c: c.pattern), ("model", [True, False], lambda c: c.full)]:
        for v in values:
            assert any(get(c) == v for c in T.CASES), (name, v)
    # the live group spans every region x motion x model
    assert {(c.region, c.motion, c.full) for c in live} == {(r, m, f) for r in T.REGIONS for m in T.MOTIONS for f in (True, False)}


@pytest.mark.parametrize("case", [c for c in T.CASES if c.live], ids=lambda c: c.id)
def test_live_cases_find_the_generating_motion(oracle, case):
    c = case
    prev, matched, status, clean = c.arrays
    ref = _ref(oracle, c)
    assert ref["oracle_rc"] >= 0, c
    clean_kept = int(np.count_nonzero(clean & (status != 0)))
    assert ref["oracle_rc"] * 2 >= clean_kept, (c, ref["oracle_rc"], clean_kept)
    w, h = c.region
    corners = np.array([[0, 0], [w, 0], [w, h], [0, h]], np.float64)
    err = np.abs(T.apply_h(ref["H"], corners) - T.apply_h(T.motion_matrix(c.motion, c.region, c.full), corners)).max()
    assert err <= 2.0 * w / 480.0, (c, err)


def test_model_minima_refuse_and_accept(oracle):
    seen = set()
    for c in T.CASES:
        if not (c.sub.startswith("min") or c.sub.startswith("exact")):
            continue
        ref = _ref(oracle, c)
        need = 4 if c.full else 2
        assert ref["m"] == c.kept
        assert (ref["oracle_rc"] >= 0) == (c.kept >= need), (c, ref["oracle_rc"])
        seen.add((c.full, c.kept))
    assert {(True, 3), (True, 4), (False, 1), (False, 2)} <= seen


def test_lens_cases_drop_pairs_on_both_sides(oracle):
    prev_only = matched_only = models = total = 0
    for c in T.CASES:
        if c.lens is None:
            continue
        und = c.und(oracle, c.n)
        a, b = T.inside_region(und[:c.n], c.region), T.inside_region(und[c.n:], c.region)
        ref = _ref(oracle, c)
        if c.lens == "all_dropped":
            assert ref["m"] == 0 and ref["oracle_rc"] < 0 and (~a).any() and (~b).any(), c
            continue
        total += 1
        prev_only += int(np.count_nonzero(~a & b)); matched_only += int(np.count_nonzero(a & ~b))
        if c.n >= 63:
            assert 0 < np.count_nonzero(a & b) < c.n, (c, np.count_nonzero(a & b))      # the rule fires, and not for every pair
            models += ref["oracle_rc"] >= 0
    assert prev_only > 0 and matched_only > 0
    assert models * 2 >= sum(1 for c in T.CASES if c.lens == "on" and c.n >= 63)      # most lens cases estimate a motion, not "no model"
