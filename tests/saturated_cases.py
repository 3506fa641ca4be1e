"""Saturated content for the block-search kernels (host and GPU tests): frames near 0 against frames near 255, where every
hand-derived value range of csrc/bbme_sea.hip, bbme_sea_mse.hip, bbme_walk16.hip, bbme_kernels.hip, bbme_fast.hip and
bbme_mfma.hip is tight ("Value ranges at saturated content").

The families are deterministic functions of (H, W, bs, seed) that return (prev, cur); ``stack`` turns a pair into the three
frames [prev, cur, prev], i.e. the pair in both directions at frame distance 1.  The NumPy restatement of the block costs
(``candidate_costs`` and friends) is int64 throughout and shares no code with the oracles it cross-checks; the ``cost``
hook exists for the mutation checks of tests/test_saturated_cases_host.py, which also holds the families to the extremes
they claim.  Nothing here imports device code."""
import numpy as np

FAMILIES = ("opposite", "near_max", "half_split", "cell_pan", "bits")

# near_max: prev is 0, cur is 255 except that one pixel in NEAR_MAX_STEP (on average) is 252, 253 or 254.  Seed and
# density were found once with search_near_max() below; test_saturated_cases_host.py holds them to what they must give
# at every bs 16 shape (a unique winner in at least half of the blocks under both norms, a winner that is not the first
# candidate in scan order in a block with a full window).
NEAR_MAX_SEED = 7
NEAR_MAX_STEP = 16

# MSE at bs > 16 sums in NumPy's float32 pairwise order.  (seed, step) of the near_max case, one per (bs, procedure), at
# which the float32-order field differs from the integer-order field at F32_SW on the (3 bs + 1) x (4 bs + 3) frame:
# found once with search_f32_cases() below.
F32_SW = 7
F32_BLOCK_SIZES = (20, 24, 28, 32)
F32_CASES = {
    (20, 0): (4, 24), (20, 1): (0, 24), (20, 2): (6, 24), (20, 3): (9, 24),
    (24, 0): (3, 24), (24, 1): (4, 24), (24, 2): (0, 24), (24, 3): (0, 24),
    (28, 0): (1, 24), (28, 1): (0, 24), (28, 2): (2, 24), (28, 3): (1, 24),
    (32, 0): (6, 24), (32, 1): (9, 24), (32, 2): (2, 24), (32, 3): (0, 24),
}


# ---------------------------------------------------------------------------
# content families
# ---------------------------------------------------------------------------
def _rng(H, W, bs, seed, salt):
    return np.random.default_rng([H, W, bs, seed, salt])


def opposite(H, W, bs=16, seed=0):
    """0 against 255: every candidate of every block ties at 255 bs^2 / 65025 bs^2, the first in scan order wins."""
    return np.zeros((H, W), np.uint8), np.full((H, W), 255, np.uint8)


def near_max(H, W, bs=16, seed=NEAR_MAX_SEED, step=NEAR_MAX_STEP):
    """0 against 255 with one pixel in `step` lowered to 252 .. 254: the costs sit within a few hundred units of the maximum
    and differ in their lowest bits, so a truncated, shifted or saturated cost picks another vector."""
    rng = _rng(H, W, bs, seed, 1)
    cur = np.full((H, W), 255, np.uint8)
    low = rng.integers(0, step, (H, W)) == 0
    cur[low] = rng.integers(252, 255, (H, W), dtype=np.uint8)[low]
    return np.zeros((H, W), np.uint8), cur


def half_split(H, W, bs=16, seed=0, axis=1):
    """prev: the first half of every bs-wide column band is 0, the second half 255; cur is the inverse.  axis 0 splits the
    bs-high row bands top / bottom instead.  The zero vector meets the maximum, a shift by bs / 2 along the axis matches
    exactly, and in between the quadrant sums of one candidate differ from the anchor's by +bs^2/4 * 255 and -bs^2/4 * 255."""
    n = W if axis == 1 else H
    line = ((np.arange(n) % bs) >= bs // 2).astype(np.uint8) * 255
    prev = np.broadcast_to(line[None, :] if axis == 1 else line[:, None], (H, W)).copy()
    return prev, (255 - prev).astype(np.uint8)


def cell_pan_vector(bs):
    """(dx, dy) of cell_pan: offsets up to bs - 1 lie inside the window at every sw; neither is a multiple of 4."""
    return (3, 1) if bs >= 4 else (1, 1)


def cell_pan(H, W, bs=16, seed=0):
    """Every bs x bs cell of a plane (the blocks of prev are whole cells) is 0 or 255 at random; cur is prev panned by
    cell_pan_vector(bs): an exact match (cost 0) beside candidates at the maximum."""
    dx, dy = cell_pan_vector(bs)
    rng = _rng(H, W, bs, seed, 2)
    cells = rng.integers(0, 2, (H // bs + 3, W // bs + 3)).astype(np.uint8) * 255
    canvas = np.kron(cells, np.ones((bs, bs), np.uint8))
    prev = np.ascontiguousarray(canvas[bs:bs + H, bs:bs + W])
    cur = np.ascontiguousarray(canvas[bs - dy:bs - dy + H, bs - dx:bs - dx + W])    # cur[y + dy, x + dx] == prev[y, x]
    return prev, cur


def bits(H, W, bs=16, seed=0):
    """Independent per-pixel 0 / 255 in both frames: block costs near half of the maximum."""
    rng = _rng(H, W, bs, seed, 3)
    return ((rng.integers(0, 2, (H, W)) * 255).astype(np.uint8), (rng.integers(0, 2, (H, W)) * 255).astype(np.uint8))


def half_split_rows(H, W, bs=16, seed=0):
    return half_split(H, W, bs, seed, axis=0)


BUILDERS = {"opposite": opposite, "near_max": near_max, "half_split": half_split, "half_split_rows": half_split_rows,
            "cell_pan": cell_pan, "bits": bits}
VARIANTS = ("opposite", "near_max", "half_split", "half_split_rows", "cell_pan", "bits")     # half_split has two variants


def variants_of(family):
    return ("half_split", "half_split_rows") if family == "half_split" else (family,)


def pair(variant, H, W, bs=16, seed=0):
    prev, cur = BUILDERS[variant](H, W, bs, seed) if variant != "near_max" else near_max(H, W, bs)
    return np.ascontiguousarray(prev), np.ascontiguousarray(cur)


def stack(variant, H, W, bs=16, seed=0):
    """uint8[3, H, W]: [prev, cur, prev] -- the pair in both directions at frame distance 1, prev against prev at 2."""
    prev, cur = pair(variant, H, W, bs, seed)
    return np.stack([prev, cur, prev])


# ---------------------------------------------------------------------------
# case lists
# ---------------------------------------------------------------------------
# bs 16: the smallest frames in which one block has a full window (sw <= 16: block (1, 2) of 3 x 5; sw <= 32: block (2, 3) of
# 5 x 7) while the others touch every edge and corner; the ragged sizes leave rows and columns beyond the last block
BS16_SHAPES = {0: ((48, 80), (50, 83)), 8: ((48, 80), (50, 83)), 16: ((48, 80), (50, 83)),
               24: ((80, 112), (81, 115)), 32: ((80, 112), (81, 115))}
BS16_SWS = (0, 8, 16, 24, 32)
BS16_DISTANCES = (1, 2)
WALK16_SWS = (4, 16, 32)                          # three-step / 2-D log: FITS at 4 and 16, not at 32
WALK16_SHAPES = {4: ((48, 80), (50, 83)), 16: ((48, 80), (50, 83)), 32: ((80, 112), (81, 115))}

# other block sizes on (3 bs + 1) x (4 bs + 3): k_walkq (MAE at all of WALKQ_SIZES, MSE up to 12), k_walk<G> at 6 and 10,
# k_exh_generic for the exhaustive search of all of them; MSE above 16 takes the float32-order kernels (F32_CASES)
WALKQ_SIZES = (4, 8, 12, 20, 24, 28, 32)
WALK_SIZES = (6, 10)
OTHER_SWS = (7, 2)
DENSE_SHAPE = (33, 33)                            # the smallest gme_begin accepts: level 1 holds a 16 x 16 block and one row / column more


def other_shape(bs):
    return 3 * bs + 1, 4 * bs + 3


def full_window_block(H, W, bs, sw):
    """(block row, block column) of the block nearest the centre whose offsets -sw .. sw all lie inside the frame, or None.
    (The window is asymmetric, -sw .. sw + bs - 1; the offsets past sw leave the small frames of the lists above in every
    block.)"""
    nbr, nbc = H // bs, W // bs
    ok = [(abs(2 * r - nbr + 1) + abs(2 * c - nbc + 1), r, c) for r in range(nbr) for c in range(nbc)
          if r * bs - sw >= 0 and c * bs - sw >= 0 and r * bs + sw + bs <= H and c * bs + sw + bs <= W]
    return min(ok)[1:] if ok else None


# ---------------------------------------------------------------------------
# block costs in NumPy int64
# ---------------------------------------------------------------------------
def sad(d):
    return np.abs(d).sum(axis=(-2, -1))


def ssd(d):
    return (d * d).sum(axis=(-2, -1))


def candidate_costs(prev, cur, bs, sw, r, c, cost):
    """(costs int64[n], offsets int64[n, 2] as (wc, wr)) of the valid candidates of block (r, c) in the scan order of the
    exhaustive search: column offset outermost, both from -sw to sw + bs - 1; `cost` maps the int64 differences
    [..., bs, bs] to one number per candidate."""
    H, W = prev.shape
    r0, c0 = r * bs, c * bs
    anchor = prev[r0:r0 + bs, c0:c0 + bs].astype(np.int64)
    t0, t1 = max(r0 - sw, 0), min(r0 + sw + bs - 1, H - bs)
    l0, l1 = max(c0 - sw, 0), min(c0 + sw + bs - 1, W - bs)
    region = cur[t0:t1 + bs, l0:l1 + bs].astype(np.int64)
    win = np.lib.stride_tricks.sliding_window_view(region, (bs, bs))       # [top, left, bs, bs]
    costs = np.asarray(cost(win - anchor), dtype=np.int64).T                # [left, top]: the column offset is outermost
    wc, wr = np.meshgrid(np.arange(l0, l1 + 1) - c0, np.arange(t0, t1 + 1) - r0, indexing="ij")
    return costs.ravel(), np.stack([wc.ravel(), wr.ravel()], -1)


def exhaustive_field(prev, cur, bs, sw, cost):
    """int32[H // bs, W // bs, 2] of the exhaustive search: the first minimum in scan order."""
    H, W = prev.shape
    mf = np.zeros((H // bs, W // bs, 2), np.int32)
    for r in range(H // bs):
        for c in range(W // bs):
            costs, offs = candidate_costs(prev, cur, bs, sw, r, c, cost)
            mf[r, c] = offs[int(np.argmin(costs))]
    return mf


def norm_cost(pnorm):
    return ssd if pnorm else sad


def quadrant_differences(prev, cur, bs, sw, r, c):
    """int64[n, 4]: the four (bs / 2)^2 quadrant sums of every valid candidate minus the anchor's."""
    h = bs // 2

    def quads(d):
        return np.stack([d[..., :h, :h].sum((-2, -1)), d[..., :h, h:].sum((-2, -1)),
                         d[..., h:, :h].sum((-2, -1)), d[..., h:, h:].sum((-2, -1))], -1)
    H, W = prev.shape
    r0, c0 = r * bs, c * bs
    anchor = prev[r0:r0 + bs, c0:c0 + bs].astype(np.int64)
    t0, t1 = max(r0 - sw, 0), min(r0 + sw + bs - 1, H - bs)
    l0, l1 = max(c0 - sw, 0), min(c0 + sw + bs - 1, W - bs)
    win = np.lib.stride_tricks.sliding_window_view(cur[t0:t1 + bs, l0:l1 + bs].astype(np.int64), (bs, bs))
    return (quads(win) - quads(anchor)).reshape(-1, 4)


# ---------------------------------------------------------------------------
# the searches that chose the constants above (run by hand, and by the host test on the committed values)
# ---------------------------------------------------------------------------
def near_max_report(seed, step):
    """[(H, W, sw, pnorm, unique share, first-is-not-winner in a full-window block)] over the bs 16 shapes."""
    out = []
    for sw in BS16_SWS:
        for H, W in BS16_SHAPES[sw]:
            prev, cur = near_max(H, W, 16, seed, step)
            for pnorm in (0, 1):
                unique = 0
                for r in range(H // 16):
                    for c in range(W // 16):
                        costs, _ = candidate_costs(prev, cur, 16, sw, r, c, norm_cost(pnorm))
                        s = np.sort(costs)
                        unique += len(s) == 1 or s[0] < s[1]
                fw = full_window_block(H, W, 16, sw)
                costs, _ = candidate_costs(prev, cur, 16, sw, fw[0], fw[1], norm_cost(pnorm))
                out.append((H, W, sw, pnorm, unique / ((H // 16) * (W // 16)), int(np.argmin(costs)) != 0))
    return out


def search_near_max(seeds=range(8), steps=(24, 16, 12)):
    """The first (seed, step) at which every bs 16 shape, at each of its windows and under both norms, has a unique winner in
    at least half of its blocks and a winner that is not the first candidate of its full-window block."""
    for step in steps:
        for seed in seeds:
            if all(u >= 0.5 and nf for (_, _, _, _, u, nf) in near_max_report(seed, step)):
                return seed, step
    return None


def f32_pair(bs, procedure):
    seed, step = F32_CASES[(bs, procedure)]
    H, W = other_shape(bs)
    return near_max(H, W, bs, seed, step)


def search_f32_cases(bbme, seeds=range(16), steps=(24, 12, 40, 150, 8, 80)):
    """{(bs, procedure): (seed, step)} with `bbme(prev, cur, bs, sw, procedure, pnorm, allow_inexact)` (the C oracle's)."""
    found = {}
    for bs in F32_BLOCK_SIZES:
        H, W = other_shape(bs)
        for proc in range(4):
            for step in steps:
                for seed in seeds:
                    prev, cur = near_max(H, W, bs, seed, step)
                    if not np.array_equal(bbme(prev, cur, bs, F32_SW, proc, 1, 0), bbme(prev, cur, bs, F32_SW, proc, 1, 1)):
                        found[(bs, proc)] = (seed, step)
                        break
                if (bs, proc) in found:
                    break
    return found
