"""The tracking chain in the variants the stabilization filter launches, through lvk_hip_track_chain -- the diagnostics entry over the SAME
launcher lvk_hip_stab::track uses (csrc/track_chain.hip): fast_filter inside the RANSAC's first kernel (k_ransac_hypotheses<true, true>) or as
k_match_compact in front of the staged / global-memory estimator, the point count from the host or clamped from a device word, the model
choice from the host or from a device word, completion by stream synchronisation or by the host signal word, lens-corrected pairs with the
drop rule, and the flow kernel in its chained form (points from pinned host memory, LENS on, device count).

Reference: tests/track_chain_ref.py (swap-erase + lens drop rule + oracle.find_homography + oracle.pyrlk).  Bar: bit-exact -- H as uint64, the
pairs as uint32 in swap-erase order, mask, return code, counts, mirrors, und; every byte no kernel should write still holds the fill value.
Every variant is held to the same reference on the same input, so every variant equals every other.  tests/test_track_chain_recipe.py shows
on the CPU that the cases are live (the estimator finds the generating motion where the recipe says it must)."""
import numpy as np
import pytest

from tests import track_chain_ref as T
from tests.test_oracle_imgproc import _smooth_scene

pytestmark = pytest.mark.gpu

FILL, GUARD = 0xA5, 64
INT_MAX = 2 ** 31 - 1

# compaction - count - model - completion; every value of every axis, and the pairs of them the product runs together
#   asfilter: fused up to 2048 points, k_match_compact beyond (what lvk_hip_stab::track decides); separate: k_match_compact for any n
#   nhost: host n; nword: device word == bound; nbelow: device word below the launch bound; nabove: word above the bound (clamped); nzero: word 0
#   mhost: host flag; mword: device word (host flag agrees); mwins: device word, host flag says the opposite
#   (the word must win in the fused kernels as well as in the separate ones, on a count that is not zero)
VARIANTS = ["asfilter-nhost-mhost-sync", "separate-nhost-mhost-signal", "asfilter-nword-mwins-signal", "separate-nbelow-mwins-sync",
            "asfilter-nbelow-mword-signal", "asfilter-nabove-mhost-sync", "separate-nabove-mword-signal", "asfilter-nzero-mwins-sync",
            "separate-nzero-mhost-signal"]

_ref_cache = {}


def _gpu(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _filled(a):
    return bool((np.ascontiguousarray(a).view(np.uint8) == FILL).all())


def _bound_above(n):
    return T.N_EDGES[T.N_EDGES.index(n) + 1]


def _reference(oracle, c, n_eff):
    key = (c.id, n_eff)
    if key not in _ref_cache:
        prev, matched, status, _ = c.arrays
        und = c.und(oracle, n_eff)
        _ref_cache[key] = (T.reference(oracle, prev, matched, status, n_eff, und, c.region, c.threshold, c.full), und)
    return _ref_cache[key]


def _check_chain(out, ref, nb, n_eff, label, signal):
    m = ref["m"]
    assert out["count_dev"] == m and out["count_host"] == m, (label, out["count_dev"], out["count_host"], m)
    assert out["rc"] == ref["rc"], (label, out["rc"], ref["rc"])
    assert np.array_equal(out["H"].view(np.uint64), ref["H"].view(np.uint64)), (label, np.abs(out["H"] - ref["H"]).max())
    assert np.array_equal(out["mask"][:m], ref["mask"]), label
    assert _filled(out["mask"][m:]), label
    for k, want in enumerate((ref["p1"], ref["p2"])):
        assert np.array_equal(out["pairs_dev"][k, :m].view(np.uint32), np.ascontiguousarray(want).view(np.uint32).reshape(m, 2)), (label, "pairs", k)
        assert _filled(out["pairs_dev"][k, m:]), (label, "pairs tail", k)
    assert np.array_equal(out["mirror_matched"][:n_eff].view(np.uint32), np.ascontiguousarray(ref["mirror_matched"]).view(np.uint32).reshape(n_eff, 2)), label
    assert np.array_equal(out["mirror_status"][:n_eff], ref["mirror_status"]), label
    assert _filled(out["mirror_matched"][n_eff:]) and _filled(out["mirror_status"][n_eff:]), label
    if signal:
        assert out["signalled"] == 1, (label, "results were not taken from the host signal word")


def _run_variant(ctx, oracle, c, variant):
    compaction, count, model, completion = variant.split("-")
    prev, matched, status, _ = c.arrays
    n = c.n
    nb = _bound_above(n) if count == "nbelow" else n
    n_word = {"nhost": None, "nword": n, "nbelow": n, "nabove": n + 1 if n % 2 else INT_MAX, "nzero": 0}[count]
    n_eff = 0 if count == "nzero" else n
    if nb > n:
        # what lies between the count and the launch bound is not part of the input: plausible pairs, flagged as tracked, that must be ignored
        rng = np.random.default_rng(n)
        pad = nb - n
        prev = np.concatenate([prev, rng.uniform(0, c.region[0], (pad, 2)).astype(np.float32)])
        matched = np.concatenate([matched, rng.uniform(0, c.region[0], (pad, 2)).astype(np.float32)])
        status = np.concatenate([status, np.ones(pad, np.uint8)])
    ref, und = _reference(oracle, c, n_eff)
    full, full_word = {"mhost": (c.full, None), "mword": (c.full, int(c.full)), "mwins": (not c.full, int(c.full))}[model]
    out = ctx.track_chain(prev, matched, status, und=und, threshold=c.threshold, region=c.region, full=full, full_word=full_word, n_word=n_word,
                          separate_compact=compaction == "separate", host_signal=completion == "signal")
    _check_chain(out, ref, nb, n_eff, (c, variant), completion == "signal")
    return out


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("n", T.N_EDGES)
def test_chain_from_a_flow_result(ctx, oracle, n, variant):
    """Every case of the recipe with this n (all kept, m on the edge below, fast_filter's patterns, the model minima, lens on, every pair
    dropped, the live breadth cases) through one variant, against the composed reference."""
    if variant.split("-")[1] == "nbelow" and n == T.N_EDGES[-1]:
        n = 4095                # no launch bound above 4096 exists: a count below the bound sees 4096 as the BOUND of the n = 4095 cases
        assert _bound_above(n) == 4096
    n_cases = [c for c in T.CASES if c.n == n]
    assert len(n_cases) >= 5
    for c in n_cases:
        _run_variant(ctx, oracle, c, variant)


def test_model_minima_on_the_device(ctx, oracle):
    """A homography refuses 3 pairs and takes 4, a similarity refuses 1 and takes 2 -- in the fused and in the separate kernels, the model from the word."""
    seen = set()
    for c in T.CASES:
        if c.sub.startswith("min") or c.sub.startswith("exact"):
            for variant in ("asfilter-nhost-mhost-sync", "separate-nword-mwins-signal"):
                out = _run_variant(ctx, oracle, c, variant)
                assert (out["rc"] >= 0) == (c.kept >= (4 if c.full else 2)), (c, variant, out["rc"])
                assert out["rc"] >= 0 or (out["rc"] == T.NO_MODEL and np.array_equal(out["H"], np.eye(3)))
                seen.add((c.full, c.kept, out["rc"] >= 0))
    assert {(True, 3, False), (True, 4, True), (False, 1, False), (False, 2, True)} <= seen


def test_live_cases_find_the_motion_on_the_device(ctx, oracle):
    """The liveness conditions of tests/test_track_chain_recipe.py hold for what the GPU returned (not only for the oracle's side)."""
    for c in [c for c in T.CASES if c.live][::5]:
        out = _run_variant(ctx, oracle, c, "asfilter-nword-mwins-signal")
        w, h = c.region
        corners = np.array([[0, 0], [w, 0], [w, h], [0, h]], np.float64)
        err = np.abs(T.apply_h(out["H"], corners) - T.apply_h(T.motion_matrix(c.motion, c.region, c.full), corners)).max()
        assert out["rc"] >= 0 and err <= 2.0 * w / 480.0, (c, out["rc"], err)


@pytest.mark.parametrize("variant", ["asfilter-nword-mwins-signal", "separate-nbelow-mwins-sync"])
def test_chain_is_deterministic_across_calls_and_contexts(ctx, oracle, variant):
    import livevisionkit_amd as lvk
    other = lvk.Context(0)
    try:
        for c in [c for c in T.CASES if c.n in (257, 2047, 2049) and c.sub in ("kept", "lens", "dense", "sparse", "value255", "even", "odd")]:
            a, b, o = _run_variant(ctx, oracle, c, variant), _run_variant(ctx, oracle, c, variant), _run_variant(other, oracle, c, variant)
            for k in ("H", "mask", "pairs_dev", "mirror_matched", "mirror_status"):
                assert a[k].tobytes() == b[k].tobytes() == o[k].tobytes(), (c, k)
            assert (a["rc"], a["count_dev"], a["count_host"]) == (b["rc"], b["count_dev"], b["count_host"]) == (o["rc"], o["count_dev"], o["count_host"])
    finally:
        other.close()


# ---- the chain from two images: the flow kernel in its chained form ---------------------------------------------------------------------------
FLOW_GEOMETRY = {"270x480-w11": (270, 480, (11, 11), 3, (1.3, -0.7), 600), "256x256-w11": (256, 256, (11, 11), 3, (0.8, -1.1), 257),
                 "90x120-w7x9": (90, 120, (7, 9), 2, (0.8, -1.1), 150), "135x240-w15": (135, 240, (15, 15), 3, (-0.6, 0.9), 64)}
# the count: host n; a word equal to / below the bound; a word ABOVE the bound (clamped -- the bound + 17 keeps even an unclamped `und` offset
# inside the guard entries); a word of 0
FLOW_COUNTS = ["nhost", "nword", "nbelow", "nabove", "nzero"]


def _run_flow(ctx, oracle, geometry, lens, count, separate=False, signal=True, full=True):
    rows, cols, win, lv, shift, nb = FLOW_GEOMETRY[geometry]
    prev_img = _smooth_scene(rows, cols, 0, 0); next_img = _smooth_scene(rows, cols, shift[0], shift[1])
    rng = np.random.default_rng(rows + nb)
    pts = np.c_[rng.uniform(-5, cols + 5, nb), rng.uniform(-5, rows + 5, nb)].astype(np.float32)      # near and outside the border as well
    n_word = {"nhost": None, "nword": nb, "nbelow": nb - nb // 3, "nabove": nb + 17, "nzero": 0}[count]
    n_eff = nb if n_word is None else min(n_word, nb)
    region = (cols, rows)
    want_next, want_status = oracle.pyrlk(prev_img, next_img, pts[:n_eff], win=win, max_level=lv) if n_eff else (np.zeros((0, 2), np.float32), np.zeros(0, np.uint8))
    und = None
    if lens:
        und = oracle.lens_undistort_points(T.lens_profile(region), rows * T.LENS_SCALE, cols * T.LENS_SCALE, float(T.LENS_SCALE), float(T.LENS_SCALE),
                                           np.concatenate([pts[:n_eff], want_next]))
    ref = T.reference(oracle, pts, want_next, want_status, n_eff, und, region, 3.0, full)
    out = ctx.track_chain(pts, images=(_gpu(prev_img), _gpu(next_img)), win=win, max_level=lv,
                          lens=(T.lens_profile(region), rows * T.LENS_SCALE, cols * T.LENS_SCALE, T.LENS_SCALE, T.LENS_SCALE) if lens else None,
                          threshold=3.0, region=region, full=full if count == "nbelow" else not full, full_word=int(full), n_word=n_word, separate_compact=separate, host_signal=signal)      # (host flag and word disagree: the word wins)
    label = (geometry, lens, count, separate)
    # the flow kernel's own outputs: the first n_eff entries are the tracker's, everything else -- the entries of the workgroups beyond the
    # device count, the guard entries in front and behind -- is untouched
    nxt, st, fu = out["next_pts"], out["flow_status"], out["flow_und"]
    assert np.array_equal(st[GUARD:GUARD + n_eff], want_status), label
    assert np.array_equal(nxt[GUARD:GUARD + n_eff].view(np.uint32), want_next.view(np.uint32).reshape(n_eff, 2)), label
    assert _filled(nxt[:GUARD]) and _filled(nxt[GUARD + n_eff:]) and _filled(st[:GUARD]) and _filled(st[GUARD + n_eff:]), label
    if lens:
        assert np.array_equal(fu[GUARD:GUARD + 2 * n_eff].view(np.uint32), und.view(np.uint32).reshape(2 * n_eff, 2)), label
        assert _filled(fu[:GUARD]) and _filled(fu[GUARD + 2 * n_eff:]), label
    else:
        assert _filled(fu), label
    _check_chain(out, ref, nb, n_eff, label, signal)
    return out, ref


@pytest.mark.parametrize("count", FLOW_COUNTS)
@pytest.mark.parametrize("lens", [False, True], ids=["raw", "lens"])
@pytest.mark.parametrize("geometry", list(FLOW_GEOMETRY))
def test_chain_from_images(ctx, oracle, geometry, lens, count):
    out, ref = _run_flow(ctx, oracle, geometry, lens, count, separate=count in ("nbelow", "nzero"), signal=count != "nhost", full=geometry != "90x120-w7x9")
    if count != "nzero" and not lens:
        assert ref["m"] > 30 and ref["oracle_rc"] >= 4, (geometry, ref["m"], ref["oracle_rc"])      # a real flow result and a real model


def test_flow_lens_count_word_above_the_bound_regression(ctx, oracle):
    """The flow kernel's LENS form took the device word unclamped: a word above the launch bound moved the matched half of `und` behind the
    2 n entries of the buffer (pyrlk.hip `la.und[n + pt]`), while k_match_compact / the fused hypotheses kernel read it at the clamped count.
    The guard entries behind `und` stay untouched, the corrected pairs are the ones the compaction reads."""
    for separate in (False, True):
        out, ref = _run_flow(ctx, oracle, "270x480-w11", True, "nabove", separate=separate)
        assert ref["m"] > 30 and out["rc"] == ref["rc"]
