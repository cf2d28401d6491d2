"""What tests/test_track_chain_gpu.py and its CPU partner share: the input recipe of the tracking chain's cases and the reference the
chain is held against, composed from pieces the suite already trusts -- the reference's back-to-front swap-erase, the lens drop rule on
oracle.lens_undistort_points, oracle.find_homography (the frozen estimator specification) and oracle.pyrlk."""
import functools

import numpy as np

# wave (64), block (256 / 512 / 1024) and LDS_POINTS / LVK_COMPACT_RANSAC_MAX (2048) multiples, both sides of each; the model minima 2 and 4
N_EDGES = [2, 3, 4, 5, 8, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096]
REGIONS = [(480, 270), (256, 256), (3840, 2160)]
MOTIONS = ["identity", "translation", "rotzoom", "perspective"]
SHARES = [0.0, 0.3, 0.6, 1.0]
THRESHOLDS = [0.5, 3.0, 20.0]
PATTERNS = ["all", "none", "even", "odd", "dense", "sparse", "tail_holes", "front_holes", "value255"]
NO_MODEL = -12            # lvk_hip_track_chain: no model (too few pairs included)
# a strong barrel profile (frame = 4 x the tracking size): corrected positions near the border leave the tracking region
LENS_SCALE = 4


def lens_profile(region):
    w, h = region[0] * LENS_SCALE, region[1] * LENS_SCALE
    return (0.8 * w, 0.8 * w, w / 2 + 3, h / 2 - 2, -0.22, 0.05, 1e-3, -2e-3, 0.01)


def swap_erase(arrays, keep):
    """fast_filter (Functions/Container.tpp:97-121): back to front, swap a dropped element with the last kept one."""
    arrays = [a.copy() for a in arrays]
    m = len(keep)
    for k in range(len(keep) - 1, -1, -1):
        if not keep[k]:
            m -= 1
            for a in arrays:
                a[[k, m]] = a[[m, k]]
    return [a[:m] for a in arrays]


def apply_h(H, p):
    q = np.c_[p, np.ones(len(p))] @ H.T
    return q[:, :2] / q[:, 2:]


def motion_matrix(name, region, full):
    """The generating motion, in what the chosen model can express: the suite's mild perspective (test_global_motion_bit_exact) keeps its last
    row for the homography and is reduced to its similarity part (mean scale, mean rotation) for the 4-dof model."""
    w, h = region
    s = w / 480.0
    if name == "identity":
        return np.eye(3)
    if name == "translation":
        return np.array([[1, 0, 3.1 * s], [0, 1, -2.2 * s], [0, 0, 1.0]])
    if name == "rotzoom":
        a, b = 1.1 * np.cos(np.deg2rad(5)), 1.1 * np.sin(np.deg2rad(5))
        cx, cy = w / 2, h / 2
        return np.array([[a, -b, cx - (a * cx - b * cy)], [b, a, cy - (b * cx + a * cy)], [0, 0, 1.0]])
    if full:
        return np.array([[1.01, 0.012, 3.1 * s], [-0.011, 0.995, -2.2 * s], [2e-5 / s, -1e-5 / s, 1.0]])
    a, b = (1.01 + 0.995) / 2, (-0.011 - 0.012) / 2
    return np.array([[a, -b, 3.1 * s], [b, a, -2.2 * s], [0, 0, 1.0]])


def status_pattern(name, n, rng):
    i = np.arange(n)
    if name == "all":
        return np.ones(n, np.uint8)
    if name == "none":
        return np.zeros(n, np.uint8)
    if name == "even":
        return (i % 2).astype(np.uint8)
    if name == "odd":
        return ((i + 1) % 2).astype(np.uint8)
    if name == "dense":
        return (rng.random(n) < 0.9).astype(np.uint8)
    if name == "sparse":
        return (rng.random(n) < 0.3).astype(np.uint8)
    if name == "tail_holes":
        return (i < n // 3).astype(np.uint8)
    if name == "front_holes":
        return (i >= n // 3).astype(np.uint8)
    if name == "value255":
        return (rng.random(n) < 0.5).astype(np.uint8) * 255
    assert name.startswith("keep"), name            # keep<m>: exactly m pairs kept, anywhere
    st = np.zeros(n, np.uint8)
    st[rng.choice(n, int(name[4:]), replace=False)] = 1
    return st


class Case:
    """One input of the chain: a flow result (prev, matched, status[, und]) of n points, a region, a threshold, a model."""

    def __init__(self, n, sub, region, motion, share, threshold, full, pattern, lens=None, seed=0):
        self.n, self.sub, self.region, self.motion, self.share, self.threshold, self.full, self.pattern, self.lens, self.seed = \
            n, sub, region, motion, share, threshold, full, pattern, lens, seed
        self.id = f"n{n}-{sub}"

    def __repr__(self):
        return (f"Case(n={self.n}, {self.sub}, region={self.region}, {self.motion}, share={self.share}, thr={self.threshold}, "
                f"{'homography' if self.full else 'similarity'}, {self.pattern}, lens={self.lens}, seed={self.seed})")

    @functools.cached_property
    def arrays(self):
        """prev, matched (float32 n x 2), status (uint8 n), clean (bool n: the pairs that follow the generating motion)."""
        n, (w, h) = self.n, self.region
        rng = np.random.default_rng([self.seed, n, w, MOTIONS.index(self.motion), int(self.share * 10), int(self.full)])
        s = w / 480.0
        prev = np.c_[rng.uniform(0, w, n), rng.uniform(0, h, n)].astype(np.float32)
        matched = apply_h(motion_matrix(self.motion, self.region, self.full), prev) + rng.normal(0, 0.2, prev.shape)
        out = np.zeros(n, bool)
        out[rng.permutation(n)[:int(round(self.share * n))]] = True
        matched[out] += rng.uniform(-40 * s, 40 * s, (int(out.sum()), 2))
        status = status_pattern(self.pattern, n, rng)
        return prev, matched.astype(np.float32), status, ~out

    def und(self, oracle, n_eff):
        """Lens-corrected (previous | matched) positions of the first n_eff pairs, as the flow kernel's LENS form lays them out; None without lens."""
        if self.lens is None:
            return None
        prev, matched, _, _ = self.arrays
        w, h = self.region
        und = oracle.lens_undistort_points(lens_profile(self.region), h * LENS_SCALE, w * LENS_SCALE, float(LENS_SCALE), float(LENS_SCALE),
                                           np.concatenate([prev[:n_eff], matched[:n_eff]]))
        if self.lens == "all_dropped" and n_eff:
            # the degenerate case: every pair has one end outside the region -- alternately the previous and the matched position
            und = und.copy()
            und[np.arange(0, n_eff, 2), 0] = np.float32(-0.25)
            und[n_eff + np.arange(1, n_eff, 2), 1] = np.float32(h)
        return und

    @property
    def live(self):
        """The cases that must find the generating motion (the liveness conditions); everything else may find no model."""
        return self.lens is None and self.share <= 0.3 and self.kept >= 63

    @functools.cached_property
    def kept(self):
        return int(np.count_nonzero(self.arrays[2]))


def inside_region(p, region):
    """The drop rule of the fused lens mode (k_match_compact): binary32 comparisons, NaN is outside."""
    w, h = np.float32(region[0]), np.float32(region[1])
    with np.errstate(invalid="ignore"):
        return (p[:, 0] >= np.float32(0)) & (p[:, 0] < w) & (p[:, 1] >= np.float32(0)) & (p[:, 1] < h)


def reference(oracle, prev, matched, status, n_eff, und, region, threshold, full):
    """What the chain must leave behind for the first n_eff points of a flow result: compacted pairs in swap-erase order, the estimator's
    result on them under lvk_hip_track_chain's return convention, and the host mirrors."""
    prev, matched, status = prev[:n_eff], matched[:n_eff], status[:n_eff]
    keep = status != 0
    a, b = prev, matched
    if und is not None:
        a, b = und[:n_eff], und[n_eff:2 * n_eff]
        keep = keep & inside_region(a, region) & inside_region(b, region)
    p1, p2 = swap_erase([a, b], keep)
    rc, H, mask = oracle.find_homography(p1.reshape(-1, 2), p2.reshape(-1, 2), threshold, region=region, partial=not full)
    return dict(p1=p1, p2=p2, m=len(p1), rc=rc if rc >= 0 else NO_MODEL, oracle_rc=rc, H=H, mask=mask,
                mirror_matched=matched, mirror_status=np.where(keep, status, 0).astype(np.uint8))


def _cases():
    cases = []
    for k, n in enumerate(N_EDGES):
        lower = [e for e in N_EDGES if e < n]
        pick = lambda seq, j: seq[(k + j) % len(seq)]
        full = k % 2 == 0
        # (a) every pair kept, the live shares: m = n on the edge
        cases.append(Case(n, "kept", pick(REGIONS, 0), pick(MOTIONS, 0), pick(SHARES[:2], 0), pick(THRESHOLDS, 0), full, "all"))
        # (b) the other model, holes anywhere, m on the edge below n; the shares that may lose the model
        m_edge = lower[-1] if lower else n
        cases.append(Case(n, f"m{m_edge}", pick(REGIONS, 1), pick(MOTIONS, 1), pick(SHARES, 2), pick(THRESHOLDS, 1), not full, f"keep{m_edge}"))
        # (c) fast_filter's patterns, the third region / threshold
        cases.append(Case(n, pick(PATTERNS, 0), pick(REGIONS, 2), pick(MOTIONS, 2), pick(SHARES, 1), pick(THRESHOLDS, 2), full, pick(PATTERNS, 0)))
        cases.append(Case(n, pick(PATTERNS, 4), pick(REGIONS, 0), pick(MOTIONS, 3), pick(SHARES[:2], 1), pick(THRESHOLDS, 0), not full, pick(PATTERNS, 4)))
        # (d) the model minima: a homography refuses 3 pairs and takes 4, a similarity refuses 1 and takes 2 (clean pairs)
        need, fm = pick([(3, True), (4, True), (1, False), (2, False)], 0)
        if n >= need:
            cases.append(Case(n, f"min{need}{'h' if fm else 's'}", pick(REGIONS, 1), pick(MOTIONS, 1), 0.0, 3.0, fm, f"keep{need}"))
        # (e) lens on: the motion between corrected positions, pairs dropped on either side; now and then every pair dropped
        cases.append(Case(n, "lens", pick(REGIONS[:2], 0), pick(MOTIONS, 2), pick(SHARES[:3], 0), 3.0, full, pick(["all", "dense", "value255"], 0), lens="on"))
        if k % 4 == 1:
            cases.append(Case(n, "lens_all_dropped", REGIONS[0], "translation", 0.0, 3.0, not full, "all", lens="all_dropped"))
    # the model minima at the smallest n, both ways for both models
    for n, need, fm in [(3, 3, True), (4, 4, True), (4, 3, True), (2, 2, False), (2, 1, False), (5, 4, True)]:
        cases.append(Case(n, f"exact{need}{'h' if fm else 's'}", REGIONS[0], "rotzoom", 0.0, 3.0, fm, f"keep{need}", seed=1))
    # every motion x region x model x live share at a mid-size n (the live group's breadth)
    j = 0
    for region in REGIONS:
        for motion in MOTIONS:
            for full in (True, False):
                n = [63, 257, 1025, 2049][j % 4]
                cases.append(Case(n, f"live-{motion}-{region[0]}-{'h' if full else 's'}", region, motion, SHARES[j % 2], THRESHOLDS[j % 3], full, "dense", seed=2))
                j += 1
    ids = [c.id for c in cases]
    assert len(ids) == len(set(ids)), "case ids must be unique"
    return cases


CASES = _cases()
