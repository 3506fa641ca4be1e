"""Case lists for the frame-plumbing kernels of csrc/gme_kernels.hip (host and GPU tests): k_pyrdown_lds, k_pyrdown,
k_pyrdown_edge16, k_pyrdown_edge, k_compensate16, k_compensate, k_sse and k_repack.

Every list is built deterministically so that it lands on the exact values at which those kernels change path; the pure-Python
mirrors ``pyr_path`` and ``comp_paths`` say which path a case reaches, and tests/test_frame_kernel_cases_host.py fails when a
list misses one.  The NumPy restatements (``np_pyrdown``, ``np_compensate``, ``np_sse``) are int64 throughout and share no
code with the oracles they cross-check.  Nothing here imports device code."""
import collections

import numpy as np

# ---------------------------------------------------------------------------
# pyramid
# ---------------------------------------------------------------------------
PYR_T, PYR_ROWS, PYR_APRON = 8, 19, 4           # csrc/gme_kernels.hip: output rows per workgroup, source rows staged, apron

LDS_WIDTHS = (8, 16, 24, 40, 56, 72, 248, 264)                  # W % 16 is 0 and 8; 248 / 264 straddle one 256-item staging pass
LDS_WIDE = (2032, 2040)                                         # 2040: the last width the launcher accepts
# source heights: dH odd and even, dH % 8 in {0, 1, 7} (13 and 29 supply the 7), sH < 4 (the looping reflect101), dH = 9 and 17
# (a last workgroup with one row), dH = 3, 7, 15 (an odd dH on the last row pair of a workgroup)
LDS_HEIGHTS = (1, 2, 3, 4, 5, 13, 15, 16, 17, 29, 31, 33)
LDS_WIDE_HEIGHTS = (1, 3, 13, 16, 17, 19)                       # at most 19 rows at the wide widths
FALLBACK_WIDE = ((9, 2048), (5, 3456))                          # 2048: the first width past pyr_quads < 256; 3456 is also past the
                                                                # 64 KB of LDS (19 rows, from 3448 on): k_pyrdown + k_pyrdown_edge16
MOD8_4_WIDTHS = (12, 20, 36)                                    # W % 8 == 4: 20 and 36 take k_pyrdown_edge16, 12 is narrower than its
                                                                # 16-byte chunk and takes the per-pixel k_pyrdown_edge
EDGE_WIDTHS = (3, 5, 7, 13, 15, 17, 18, 19)                     # dW < 4 (3, 5), pyr_interior_end clamps to 4 (up to 15)
FALLBACK_HEIGHTS = (1, 4, 9, 17)

CONTENTS = ("noise", "zeros", "full", "checker", "border")


def pyr_shapes():
    """(H, W) of every single-plane pyramid case."""
    shapes = [(H, W) for W in LDS_WIDTHS for H in LDS_HEIGHTS]
    shapes += [(H, W) for W in LDS_WIDE for H in LDS_WIDE_HEIGHTS]
    shapes += list(FALLBACK_WIDE)
    shapes += [(H, W) for W in MOD8_4_WIDTHS + EDGE_WIDTHS for H in FALLBACK_HEIGHTS]
    return shapes


# a Sequence of PYR_BATCH frames per shape (gme_begin is valid for each: level 1 holds a 16 x 16 block, level 0 a 2 x 2 one):
# three whose levels 2 -> 1 take k_pyrdown_lds (W % 16 of 0 and 8, dH of 17 and 18 = a partly empty last workgroup) and one
# that takes k_pyrdown + k_pyrdown_edge
PYR_BATCH = 5
PYR_BATCH_SHAPES = ((33, 80), (35, 264), (34, 2040), (33, 90))


def content(kind, H, W, seed=0):
    """uint8[H, W] of one of CONTENTS."""
    if kind == "noise":
        return np.random.default_rng([H, W, seed]).integers(0, 256, (H, W), dtype=np.uint8)
    if kind == "zeros":
        return np.zeros((H, W), np.uint8)
    if kind == "full":                           # (a + 128) >> 8 at the top of the range: 255 * 256 + 128
        return np.full((H, W), 255, np.uint8)
    if kind == "checker":
        y, x = np.mgrid[0:H, 0:W]
        return (((x + y) & 1) * 255).astype(np.uint8)
    if kind == "border":                         # a one-pixel 255 frame on 0: only the reflected taps tell the kernels apart
        f = np.zeros((H, W), np.uint8)
        f[0, :] = f[-1, :] = 255
        f[:, 0] = f[:, -1] = 255
        return f
    raise KeyError(kind)


def _round_up(v, m):
    return (v + m - 1) // m * m


def pyr_lds_geometry(W):
    """(admitted, per_row, quads) of the LDS-tiled form for source width W: the predicate of launch_pyrdown
    (csrc/gme_kernels.hip, "LDS-tiled form", the `if (src.W % 8 == 0 && ...` above the k_pyrdown_lds launch), with the
    plane pitch every entry point uses (W rounded up to 64 bytes, plane_shape in csrc/gme_internal.h)."""
    pitch = _round_up(W, 64)
    lpitch = (PYR_APRON + W + 2 + 7) & ~7
    lds = PYR_ROWS * lpitch
    per_row, quads = (W + 15) // 16, ((W + 1) // 2) // 4
    ok = (W % 8 == 0 and W >= 8 and pitch % 16 == 0 and lds <= 64 * 1024 and PYR_ROWS * per_row < 4096 and per_row < 256 and
          (PYR_T // 2) * quads < 4096 and quads < 256)
    return ok, per_row, quads


def pyr_interior_end(sW, dW):
    """pyr_interior_end of csrc/gme_kernels.hip (C division truncates towards zero)."""
    e = min(int((sW - 12) / 2) + 4, dW) & ~3
    return 4 if e < 4 else e


def pyr_path(H, W, force_generic=False):
    """Names of the kernels launch_pyrdown (csrc/gme_kernels.hip) starts for an H x W source plane, restating its dispatch:
    the LDS predicate (pyr_lds_geometry) unless GME_FORCE_GENERIC is set, else k_pyrdown when `interior_quads > 0`, and
    k_pyrdown_edge16 under `src.W >= 16 && src.W % 4 == 0 && !GME_FORCE_GENERIC`, k_pyrdown_edge otherwise."""
    if pyr_lds_geometry(W)[0] and not force_generic:
        return ("k_pyrdown_lds",)
    dW = (W + 1) // 2
    names = []
    if (pyr_interior_end(W, dW) - 4) // 4 > 0:
        names.append("k_pyrdown")
    names.append("k_pyrdown_edge16" if W >= 16 and W % 4 == 0 and not force_generic else "k_pyrdown_edge")
    return tuple(names)


def _reflect_index(idx, n):
    """BORDER_REFLECT_101 of an index array in closed form (period 2 (n - 1)); n == 1 maps everything to 0."""
    if n == 1:
        return np.zeros_like(idx)
    period = 2 * (n - 1)
    m = np.mod(idx, period)
    return np.where(m >= n, period - m, m)


def np_pyrdown(src, rounding=128):
    """cv2.pyrDown as the kernels state it: separable 1-4-6-4-1, BORDER_REFLECT_101, (a + 128) >> 8, in int64.
    `rounding` exists for the mutation check of the host test only."""
    s = np.asarray(src).astype(np.int64)
    H, W = s.shape
    taps = (1, 4, 6, 4, 1)
    xs, ys = 2 * np.arange((W + 1) // 2), 2 * np.arange((H + 1) // 2)
    hp = sum(t * s[:, _reflect_index(xs + d - 2, W)] for d, t in enumerate(taps))
    vp = sum(t * hp[_reflect_index(ys + d - 2, H), :] for d, t in enumerate(taps))
    return ((vp + rounding) >> 8).astype(np.uint8)


# ---------------------------------------------------------------------------
# compensation
# ---------------------------------------------------------------------------
COMP_SHAPES = (
    (64, 96, 16), (96, 160, 32),      # k_compensate16
    (80, 160, 32),                    # two block rows on a height 32 does not divide: the kernels' bs = H // rows is 40, k_compensate
    (64, 90, 16),                     # k_compensate, quad path, W % 4 != 0 in the last quad
    (70, 90, 16),                     # four block rows on 70 rows: the kernels' bs is 17, per-pixel path
    (60, 84, 12), (66, 90, 6),        # 12: quad path, 6: per-pixel path
    (45, 50, 5),                      # per-pixel path
    (50, 96, 16),                     # H % bs != 0: rows beyond the field
)
# shapes whose nominal block size is not the one the kernels use (bs = H // rows, rows = H // nominal)
COMP_BS_CHANGES = {(80, 160, 32): 40, (70, 90, 16): 17}
EXTREMES = (32767, -32767, 32768, -32768, 2 ** 31 - 1, -(2 ** 31 - 1), -2 ** 31)
TAIL_BOUNDS = (-1, 0, "W-2", "W-1", "W")          # source column of the first pixel of the last, partial quad (W % 4 != 0)


def kernel_bs(H, rows):
    """The block size of the kernels and of motion.compensate_frame: the height only."""
    return H // rows


def sx_bounds(W):
    """Source columns at which a run changes path: sx in {-16, -15, -1, W - 1, W} for the 16-pixel runs, {-4, -3} for the
    4-pixel ones, and a run that ends on W - s for s = 0 .. 3 (every byte shift next to the right edge; s = 0 is
    sx + 16 == W / sx + 4 == W, s > 0 reads the fifth dword / the second dword up to the row's last byte)."""
    return [-16, -15, -4, -3, -1, W - 1, W] + [W - 16 - s for s in range(4)] + [W - 4 - s for s in range(4)]


def sy_bounds(H):
    return [-1, 0, H - 1, H]


def _background(h, w):
    """Small vectors of every residue mod 4 in x: interior runs take all four byte shifts."""
    i, j = np.mgrid[0:h, 0:w]
    return np.stack([(3 * i + 5 * j) % 9 - 4, (5 * i + 3 * j) % 7 - 3], -1).astype(np.int32)


def comp_fields(H, W, bs):
    """[(name, int32[rows, columns, 2])] for one (H, W, bs): one field per boundary value of each family.  Positions are those
    the kernels see: k = H // (H // bs) pixels per block (kernel_bs), which is not bs for the shapes of COMP_BS_CHANGES.

    sx=B       the first run of the first block column and of the last block column inside the frame reads from column B
               (every block row, d1 = 0)
    last=s     that last block column moves by s = 0 .. 3: its last run ends on W - s when k divides W
    sy=B       row 0 of the first block row and the last row of the last block row read from row B (every block column)
    extreme    vectors of +-32767, +-32768, +-(2^31 - 1), -2^31: nothing lies inside any frame
    cols-1     one block column fewer than W // bs: columns beyond the field
    rows-1     one block row and column fewer: the kernels' block size grows, rows and columns beyond the field
    wide-sx=B  only where W // bs blocks of k pixels end before W: one block column more, which covers the rest of the row (the
               partial quad of a W % 4 != 0 included); its first run reads from column B
    tail-sx=B  the same wide field, only where W % 4 != 0: the first pixel of the last, partial quad reads from column B"""
    h, w = H // bs, W // bs
    k = kernel_bs(H, h)
    jl = min(w, -(-W // k)) - 1                  # the last block column with a pixel inside the frame
    fields = []
    for B in sx_bounds(W):
        mf = _background(h, w)
        mf[:, 0] = (0 - B, 0)
        mf[:, jl] = (jl * k - B, 0)
        fields.append(("sx=%d" % B, mf))
    for s in range(4):
        mf = _background(h, w)
        mf[:, jl] = (s, 0)
        fields.append(("last=%d" % s, mf))
    for B in sy_bounds(H):
        mf = _background(h, w)
        mf[0, :, 1] = 0 - B
        mf[h - 1, :, 1] = (h * k - 1) - B
        fields.append(("sy=%d" % B, mf))
    ext = np.array([EXTREMES[n % len(EXTREMES)] for n in range(h * w * 2)], np.int64).astype(np.int32).reshape(h, w, 2)
    fields.append(("extreme", ext))
    fields.append(("cols-1", _background(h, w)[:, :-1].copy()))
    fields.append(("rows-1", _background(h, w)[:-1, :-1].copy()))
    if w * k < W:
        for B in sx_bounds(W):
            mf = _background(h, w + 1)
            mf[:, w] = (w * k - B, 0)
            fields.append(("wide-sx=%d" % B, mf))
        if W % 4:
            xt = W - W % 4
            for name in TAIL_BOUNDS:
                B = {"W-2": W - 2, "W-1": W - 1, "W": W}.get(name, name)
                mf = _background(h, w + 1)
                mf[:, xt // k] = (xt - B, 0)
                fields.append(("tail-sx=%s" % name, mf))
    return fields


def comp_cases():
    """[(id, H, W, bs, mf)] over COMP_SHAPES x comp_fields."""
    return [("%dx%d-bs%d-%s" % (H, W, bs, name), H, W, bs, mf) for (H, W, bs) in COMP_SHAPES for name, mf in comp_fields(H, W, bs)]


def comp_frame(H, W):
    return content("noise", H, W, seed=1)


def comp_kernel(H, W, rows, force_generic=False):
    """The kernel launch_compensate (csrc/gme_kernels.hip) picks: `(H / h) % 16 == 0 && W % 16 == 0` plus alignment
    conditions that every public entry meets (pitch = W rounded up to 64, 256-byte plane strides), unless GME_FORCE_GENERIC."""
    return "k_compensate16" if kernel_bs(H, rows) % 16 == 0 and W % 16 == 0 and not force_generic else "k_compensate"


COMP_CLASSES16 = ("inside0", "inside1", "inside2", "inside3", "straddle_left", "straddle_right", "keep_row", "keep_col", "beyond")
COMP_CLASSES = COMP_CLASSES16 + ("pixel_bs", "pixel_tail")

Run = collections.namedtuple("Run", "kernel cls x y i j sx sy")


def comp_runs(H, W, mf, force_generic=False):
    """Every thread run of one compensation as the kernels see it: a run is the 16 pixels (k_compensate16) or the 4 pixels
    (k_compensate) one thread handles in one row, at block (i, j) = (y // k, x // k), k = H // rows.  sx, sy are the source of
    its first pixel, or None where the block lies beyond the field."""
    mf = np.asarray(mf)
    h, w = mf.shape[:2]
    k = kernel_bs(H, h)
    kernel = comp_kernel(H, W, h, force_generic)
    run = 16 if kernel == "k_compensate16" else 4
    for y in range(H):
        for x in range(0, W, run):
            i, j = y // k, x // k
            sx = sy = None
            if i < h and j < w:
                sx, sy = x - int(mf[i, j, 0]), y - int(mf[i, j, 1])
            if run == 4 and k % 4 != 0:
                cls = "pixel_bs"
            elif run == 4 and x + 4 > W:
                cls = "pixel_tail"
            elif sx is None:
                cls = "beyond"
            elif sy < 0 or sy >= H:
                cls = "keep_row"
            elif sx >= 0 and sx + run <= W:
                cls = "inside%d" % (sx & 3)
            elif sx <= -run or sx >= W:
                cls = "keep_col"
            else:
                cls = "straddle_left" if sx < 0 else "straddle_right"
            yield Run(kernel, cls, x, y, i, j, sx, sy)


def comp_paths(H, W, bs, mf, force_generic=False):
    """Counter of (kernel, class) over the thread runs (comp_runs) of one compensation.  Classes: inside0 .. inside3 (source run
    inside the frame, byte shift sx & 3), straddle_left / straddle_right (part of the run leaves the frame), keep_row (source row
    outside), keep_col (every source column outside), beyond (block row or column beyond the field), and k_compensate's per-pixel
    branch: pixel_bs (a block size that is no multiple of 4: every run) and pixel_tail (the last, partial quad of a width that is
    no multiple of 4, beside quads that gather).  `bs` is the caller's nominal block size: the field must have H // bs rows, or
    one fewer; the classes follow the kernels' H // rows."""
    rows = np.asarray(mf).shape[0]
    assert rows in (H // bs, H // bs - 1), (H, bs, rows)
    return collections.Counter((r.kernel, r.cls) for r in comp_runs(H, W, mf, force_generic))


def np_compensate(frame, mf, right_edge=0):
    """The per-pixel rule of motion.compensate_frame in int64: out[a, b] = frame[a - d1, b - d0] of the block (a // bs, b // bs),
    bs = H // rows, where the block lies in the field and the source inside the frame; the pixel is kept otherwise.
    `right_edge` exists for the mutation check of the host test only (1: the frame's last column counts as outside)."""
    frame = np.asarray(frame)
    mf = np.asarray(mf).astype(np.int64)
    H, W = frame.shape
    h, w = mf.shape[:2]
    bs = H // h
    a, b = np.mgrid[0:H, 0:W].astype(np.int64)
    i, j = a // bs, b // bs
    covered = (i < h) & (j < w)
    ic, jc = np.minimum(i, h - 1), np.minimum(j, w - 1)
    sa, sb = a - mf[ic, jc, 1], b - mf[ic, jc, 0]
    take = covered & (sa >= 0) & (sa < H) & (sb >= 0) & (sb < W - right_edge)
    out = frame.copy()
    out[take] = frame[sa[take], sb[take]]
    return out


def np_sse(a, b):
    d = np.asarray(a).astype(np.int64) - np.asarray(b).astype(np.int64)
    return int((d * d).sum())


# batched form: one pure translation per pair, d0 / d1 for every block (affine parameters [d0, 0, 0, d1, 0, 0])
def seq_translations(H, W):
    """(d0, d1) per pair: block columns land on the boundaries of sx_bounds / sy_bounds for some run of every row."""
    xs = [-16, -15, -1, W - 16, W - 1, W]
    ys = [-1, H - 1, H]
    return [(d0, 0) for d0 in xs] + [(0, d1) for d1 in ys] + [(-15, -1), (W - 1, H - 1)]


COMP_SEQ_SHAPES = ((64, 96, 16), (96, 160, 32), (64, 90, 16), (66, 90, 6))

# ---------------------------------------------------------------------------
# squared error
# ---------------------------------------------------------------------------
SSE_SATURATED = ((32, 256), (33, 257), (480, 720))              # 32 x 256: exactly one k_compensate* tile
SSE_NOISE = ((1, 1), (3, 65), (5, 64))


def sse_pairs():
    """[(id, a, b)]: 0 against 255 and 255 against 0 at SSE_SATURATED, noise against noise at SSE_NOISE."""
    out = []
    for H, W in SSE_SATURATED:
        lo, hi = content("zeros", H, W), content("full", H, W)
        out += [("%dx%d-0v255" % (H, W), lo, hi), ("%dx%d-255v0" % (H, W), hi, lo)]
    for H, W in SSE_NOISE:
        out.append(("%dx%d-noise" % (H, W), content("noise", H, W, 2), content("noise", H, W, 3)))
    return out


# ---------------------------------------------------------------------------
# repack
# ---------------------------------------------------------------------------
REPACK_WIDTHS = (15, 16, 17, 48, 720, 722)      # 16, 48, 720: the 16-byte path; none is a multiple of the 64-byte pitch
REPACK_STREAMED = ((48, 48), (48, 50))          # (H, W) for bbme_streamed: one 16-byte width, one byte-path width
