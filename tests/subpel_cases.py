"""Frames with a known quarter-pel shift, for the sub-pel tests (host and GPU).

A smooth texture (a few dozen random low-frequency waves) is built at four times the resolution; ``previous`` is its 4 x 4 box
average and ``current`` the box average of the same texture displaced by (sx, sy) hi-res pixels, i.e. quarter pixels: what lies
at (x, y) in ``previous`` lies at (x + sx / 4, y + sy / 4) in ``current`` exactly, before the rounding to 8 bits."""
import numpy as np

SHIFTS = ((5, -3), (-6, 2), (1, 1), (9, 7), (0, 0))             # quarter units (column, row)
RAMP = 24                                                        # hi-res pixels of the fade
MARGIN = 16                                                      # hi-res pixels around the frame: |shift| stays below it


def texture(height, width, border, seed=7, waves=40):
    """float64[height, width] in [0, 255]: random waves with periods of 24 hi-res pixels and more around mid grey, faded to
    flat grey over RAMP hi-res pixels towards a flat band of ``border`` hi-res pixels along the edges."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:height, 0:width].astype(np.float64)
    t = np.zeros((height, width))
    for _ in range(waves):
        fx, fy = rng.uniform(-1.0, 1.0, 2) * (2.0 * np.pi / 24.0)
        t += rng.uniform(0.3, 1.0) * np.sin(fx * x + fy * y + rng.uniform(0.0, 2.0 * np.pi))
    t *= 127.0 / np.abs(t).max()
    edge = np.minimum(np.minimum(x, width - 1 - x), np.minimum(y, height - 1 - y))
    fade = np.clip((edge - border) / RAMP, 0.0, 1.0)
    return 128.0 + t * (0.5 - 0.5 * np.cos(np.pi * fade))


def _box(hi, top, left, H, W):
    v = hi[top:top + 4 * H, left:left + 4 * W].reshape(H, 4, W, 4).mean(axis=(1, 3))
    return np.floor(v + 0.5).astype(np.uint8)


def shifted_pair(H, W, shift, block_size, seed=7):
    """(previous, current) uint8[H, W] with ``current`` displaced by ``shift`` = (sx, sy) quarter pixels.  The outermost ring
    of blocks and the three pixels next to it are flat in both frames: a block whose displaced origin leaves the frame stays a
    copy under either compensation (whole under the quarter-pel rule, pixel by pixel under the integer one), and on a flat
    block a copy costs nothing, so the squared errors compare what the vectors do, not what the frame edge does."""
    sx, sy = shift
    assert max(abs(sx), abs(sy)) <= MARGIN - 4
    hi = texture(4 * H + 2 * MARGIN, 4 * W + 2 * MARGIN, MARGIN + 4 * (block_size + 3), seed)
    return _box(hi, MARGIN, MARGIN, H, W), _box(hi, MARGIN - sy, MARGIN - sx, H, W)


def interior_hits(qfield, shift):
    """Share of the blocks outside the outermost ring whose vector is exactly ``shift``."""
    inner = qfield[1:-1, 1:-1].reshape(-1, 2)
    return float(np.mean(np.all(inner == np.asarray(shift), axis=1)))
