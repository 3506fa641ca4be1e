"""Frames and measures shared by the hierarchical-search tests (host and GPU)."""
import numpy as np

import subpel_cases
from frame_kernel_cases import np_pyrdown

SHIFTS = ((13, -9), (-18, 7), (3, 2), (0, 0))                    # pixels (column, row)
EDGE = 20                                                        # pixels a block keeps from every frame edge to count as interior


def pair(H, W, shift, margin=40, seed=7):
    """(previous, current) uint8[H, W]: crops of one smooth texture with texture up to the edges; what lies at (x, y) in
    ``previous`` lies at (x + sx, y + sy) in ``current``."""
    sx, sy = shift
    assert max(abs(sx), abs(sy)) <= margin
    t = np.floor(subpel_cases.texture(H + 2 * margin, W + 2 * margin, 0, seed) + 0.5).astype(np.uint8)
    return (np.ascontiguousarray(t[margin:margin + H, margin:margin + W]),
            np.ascontiguousarray(t[margin - sy:margin - sy + H, margin - sx:margin - sx + W]))


def pyramid(frame):
    """[level0, level1, level2] of a frame by the NumPy restatement of the pyramid kernel."""
    l1 = np_pyrdown(frame)
    return [np_pyrdown(l1), l1, frame]


def interior_hits(field, shift, block_size, shape=None):
    """Share of the blocks at least EDGE pixels from every frame edge whose vector equals ``shift``; ``shape`` = (H, W) of the
    frame where it is no multiple of the block size."""
    Hb, Wb = field.shape[:2]
    H, W = shape if shape is not None else (Hb * block_size, Wb * block_size)
    i, j = np.mgrid[0:Hb, 0:Wb]
    inner = ((i * block_size >= EDGE) & (j * block_size >= EDGE) & (H - (i + 1) * block_size >= EDGE) &
             (W - (j + 1) * block_size >= EDGE))
    assert inner.any()
    return float(np.mean(np.all(field[inner] == np.asarray(shift), axis=1)))


def level_shapes(H, W):
    """{level: (H_l, W_l)} of the pyramid of an H x W frame."""
    h1, w1 = (H + 1) // 2, (W + 1) // 2
    return {0: ((h1 + 1) // 2, (w1 + 1) // 2), 1: (h1, w1), 2: (H, W)}


def clamped_blocks(fields, level_shapes, block_size):
    """Blocks, summed over the levels below the first, whose doubled parent vector the clamp changed."""
    n = 0
    for l in sorted(fields)[1:]:
        Hl, Wl = level_shapes[l]
        b = block_size >> (2 - l)
        raw = 2 * fields[l - 1].astype(np.int64)
        Hb, Wb = raw.shape[:2]
        i, j = np.mgrid[0:Hb, 0:Wb]
        cx = np.clip(raw[:, :, 0], -j * b, Wl - b - j * b)
        cy = np.clip(raw[:, :, 1], -i * b, Hl - b - i * b)
        n += int(np.sum((cx != raw[:, :, 0]) | (cy != raw[:, :, 1])))
    return n
