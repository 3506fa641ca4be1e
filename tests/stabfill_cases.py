"""Shared inputs of the full-frame stabilization tests (stabilize.warp_fill / gme_seq_warp_fill): seeded
candidate lists and warps with the coverage the device comparison needs, the degenerate candidates, the host references (computed
once per case) and the prototype scene of "what it achieves".  No GPU needed."""
import functools

import numpy as np

from test_gpu_stabilize import degenerate_warps, random_warps

SHAPES = ((37, 53), (41, 131), (240, 320))       # W and H no multiples of 4; rows shorter and longer than a workgroup's 256 columns
CANDIDATES = (1, 3, 17)
N_FRAMES = 8
WORKGROUP_COLS = 256
# chosen on the CPU (test_stabfill_host.py::test_case_coverage holds them to the coverage condition)
SEEDS = {((37, 53), 1): 0, ((37, 53), 3): 0, ((37, 53), 17): 2, ((41, 131), 1): 0, ((41, 131), 3): 0, ((41, 131), 17): 73,
         ((240, 320), 1): 0, ((240, 320), 3): 0, ((240, 320), 17): 93}
DEGENERATE_SHAPE = (41, 53)


def build(shape, n, seed):
    """(frames uint8[N, H, W], sources int32[N, n], warps float64[N, n, 8]).  Candidate 0: a random frame under a slight
    zoom-in that stays inside (frame 0: every row is candidate 0's), a near warp (frames 1, 2) or a far one (half the output
    samples outside it).  Later candidates: random frames, in no temporal order, under far warps.  So that late candidates
    get to win, each is absent (-1) with probability 1/2 (n <= 3) or 9/10 (beyond), and then candidate j is put back in
    frame 3 + (j - 1) % (N - 3).  With n >= 3, frame 1 lists candidate 0's frame a second time and frame 2 has a -1 between
    two frames."""
    H, W = shape
    rng = np.random.default_rng([seed, H, W, n])
    frames = rng.integers(0, 256, size=(N_FRAMES, H, W), dtype=np.uint8)
    sources = rng.integers(0, N_FRAMES, size=(N_FRAMES, n)).astype(np.int32)
    warps = random_warps(rng, N_FRAMES * n, H, W, far=True).reshape(N_FRAMES, n, 8)
    warps[0, 0] = [0.9, 0, 0.05 * (W - 1) + 0.3, 0, 0.9, 0.05 * (H - 1) + 0.4, 0, 0]
    warps[1:3, 0] = random_warps(rng, 2, H, W)
    if n > 1:
        absent = rng.random((N_FRAMES, n - 1)) < (0.5 if n <= 3 else 0.9)
        if n > 3:
            for j in range(1, n):
                absent[3 + (j - 1) % (N_FRAMES - 3), j - 1] = False
        sources[:, 1:][absent] = -1
    if n >= 3:
        sources[1, 1] = sources[1, 0]
        sources[2, 1] = -1
        sources[2, 2] = (sources[2, 0] + 3) % N_FRAMES
    return frames, sources, warps


@functools.lru_cache(maxsize=None)
def case(shape, n):
    """The inputs of one (shape, n) and the host results in the three border / fill modes:
    dict(frames, sources, warps, want={(border, fill): stabilize.warp_fill's tuple}).  Read-only."""
    import stabilize
    frames, sources, warps = build(shape, n, SEEDS[(shape, n)])
    want = {(b, f): stabilize.warp_fill(frames, sources, warps, b, f) for b, f in MODES}
    for a in (frames, sources, warps) + tuple(x for w in want.values() for x in w):
        a.setflags(write=False)
    return {"frames": frames, "sources": sources, "warps": warps, "want": want}


MODES = (("constant", 0), ("constant", 201), ("replicate", 0))


def coverage(source, n):
    """What the host ``source`` map of a case reaches: the set of winning j, whether 255 occurs, whether some output row is
    won by candidate 0 alone, and whether some wave (one row of one workgroup: 256 columns) has lanes (four pixels each)
    that were resolved at different j."""
    wins = set(np.unique(source).tolist())
    row_of_zero = bool(np.any(np.all(source == 0, axis=2)))
    mixed = False
    W = source.shape[2]
    for c0 in range(0, W, WORKGROUP_COLS):
        seg = source[:, :, c0:c0 + WORKGROUP_COLS]
        pad = (-seg.shape[2]) % 4
        lanes = np.pad(seg, ((0, 0), (0, 0), (0, pad)), constant_values=255).reshape(seg.shape[0], seg.shape[1], -1, 4)
        last = np.where(lanes == 255, -1, lanes.astype(np.int64)).max(axis=3)        # the j at which the lane stopped taking part
        took = last >= 0
        hi = np.where(took, last, -1).max(axis=2)
        lo = np.where(took, last, 1 << 30).min(axis=2)
        mixed = mixed or bool(np.any((hi > lo) & (lo < (1 << 30))))
    return {"wins": wins - {255}, "none": 255 in wins, "row_of_zero": row_of_zero, "mixed_wave": mixed, "all": set(range(n))}


def degenerate_case():
    """(frames, sources int32[N, 12], warps, names) on DEGENERATE_SHAPE: candidate 0 a far random warp of frame t, candidates
    1 .. 11 the degenerate warps of test_gpu_stabilize.py (sorted by name) on other frames, rotated by t so that each of
    them comes first behind candidate 0 in some frame."""
    H, W = DEGENERATE_SHAPE
    table = degenerate_warps(H, W)
    names = sorted(table)
    N = len(names)
    rng = np.random.default_rng(53)
    frames = rng.integers(0, 256, size=(N, H, W), dtype=np.uint8)
    sources = np.empty((N, N + 1), np.int32)
    warps = np.empty((N, N + 1, 8))
    warps[:, 0] = random_warps(rng, N, H, W, far=True)
    for t in range(N):
        sources[t, 0] = t
        for j in range(N):
            k = (t + j) % N
            sources[t, 1 + j] = (t + 1 + j) % N
            warps[t, 1 + j] = np.asarray(table[names[k]][0], np.float64)
    return frames, sources, warps, names, table


# ---- the prototype's scene (what it achieves) ------------------------------------------------------------------------------
SCENE = {"frames": 24, "H": 96, "W": 128, "radius": 8, "canvas_seed": 7}


@functools.lru_cache(maxsize=None)
def scene():
    """synth.canvas(7) under test_stabilize_host.camera_path, 24 frames of 96 x 128 -> dict(G, frames, h): the true poses, the
    rendered frames and the true pair warps."""
    import stabilize
    from test_direct_host import warp_canvas
    from test_stabilize_host import camera_path, pair_warps
    n, H, W = SCENE["frames"], SCENE["H"], SCENE["W"]
    G = camera_path(n, H, W)
    frames = np.stack([warp_canvas(stabilize.params(G[t]), H, W, seed=SCENE["canvas_seed"])[1] for t in range(n)])
    return {"G": G, "frames": frames, "h": pair_warps(G)}
