"""The case lists of tests/frame_kernel_cases.py, checked without a GPU: they reach every kernel and every branch they are
meant to reach, the multiply-shift index division of k_pyrdown_lds is exact over everything its launcher admits, and the C
oracle the GPU tests compare against equals an independent NumPy int64 restatement on every case."""
import collections

import numpy as np
import pytest

import frame_kernel_cases as fk
from helpers import c_oracle


# ---------------------------------------------------------------------------
# branch coverage: a condition on the inputs
# ---------------------------------------------------------------------------
def test_pyramid_shapes_reach_every_kernel():
    shapes = fk.pyr_shapes()
    assert len(set(shapes)) == len(shapes)
    reached = collections.Counter(k for H, W in shapes for k in fk.pyr_path(H, W))
    assert set(reached) == {"k_pyrdown_lds", "k_pyrdown", "k_pyrdown_edge16", "k_pyrdown_edge"}, reached
    # the forced fallback of every LDS shape runs the two generic kernels
    forced = collections.Counter(k for H, W in shapes if fk.pyr_path(H, W) == ("k_pyrdown_lds",)
                                 for k in fk.pyr_path(H, W, force_generic=True))
    assert set(forced) == {"k_pyrdown", "k_pyrdown_edge"}, forced


def test_pyramid_shapes_sit_on_the_launcher_limits():
    path = fk.pyr_path
    for W in fk.LDS_WIDTHS + fk.LDS_WIDE:
        assert path(1, W) == ("k_pyrdown_lds",), W
    assert {W % 16 for W in fk.LDS_WIDTHS} == {0, 8} and {W % 16 for W in fk.LDS_WIDE} == {0, 8}
    # 2040 is the last width of the LDS form; 2048 and 3456 take the two-launch fallback
    assert path(9, 2040) == ("k_pyrdown_lds",) and all(not fk.pyr_lds_geometry(W)[0] for W in range(2041, 8200))
    assert path(9, 2048) == path(5, 3456) == ("k_pyrdown", "k_pyrdown_edge16")
    assert path(9, 20) == path(9, 36) == ("k_pyrdown", "k_pyrdown_edge16")
    assert path(9, 12) == ("k_pyrdown_edge",)                  # W % 4 == 0 but narrower than one 16-byte chunk
    for W in fk.EDGE_WIDTHS:
        assert "k_pyrdown_edge" in path(9, W) and "k_pyrdown_lds" not in path(9, W), W
    assert any((W + 1) // 2 < 4 for W in fk.EDGE_WIDTHS)
    assert any(int((W - 12) / 2) + 4 < 4 and fk.pyr_interior_end(W, (W + 1) // 2) == 4 for W in fk.EDGE_WIDTHS)
    # heights: the looping reflect101, dH % 8 in {0, 1, 7}, odd and even dH, a last workgroup that is partly empty
    dH = [(H + 1) // 2 for H in fk.LDS_HEIGHTS]
    assert {1, 2, 3} <= set(fk.LDS_HEIGHTS) and {0, 1, 7} <= {d % fk.PYR_T for d in dH}
    assert any(d % 2 for d in dH) and any(d % 2 == 0 for d in dH) and any(d > fk.PYR_T and d % fk.PYR_T for d in dH)
    assert max(fk.LDS_WIDE_HEIGHTS) <= 19
    # batched shapes: gme_begin is valid (a 16 x 16 block fits level 1, with a row and a column to spare for the diamond search)
    lds = [s for s in fk.PYR_BATCH_SHAPES if path(*s) == ("k_pyrdown_lds",)]
    assert len(lds) == 3 and len(fk.PYR_BATCH_SHAPES) == 4
    assert all((H + 1) // 2 > 16 and (W + 1) // 2 > 16 for H, W in fk.PYR_BATCH_SHAPES)


@pytest.fixture(scope="module")
def comp_classes():
    """Counter of (kernel, class) over every compensation case, default dispatch and forced generic."""
    total = {False: collections.Counter(), True: collections.Counter()}
    per_case = {}
    for cid, H, W, bs, mf in fk.comp_cases():
        for forced in (False, True):
            c = fk.comp_paths(H, W, bs, mf, force_generic=forced)
            total[forced] += c
            per_case[(cid, forced)] = c
    return total, per_case


def test_compensation_cases_reach_every_branch(comp_classes):
    total, per_case = comp_classes
    default = total[False]
    for cls in fk.COMP_CLASSES16:
        assert default[("k_compensate16", cls)] > 0, cls
    for cls in fk.COMP_CLASSES:
        assert default[("k_compensate", cls)] > 0, cls
    for cls in fk.COMP_CLASSES16 + ("pixel_bs",):              # forced: pixel_tail needs W % 4 != 0, which is k_compensate anyway
        assert total[True][("k_compensate", cls)] > 0, cls
    assert not any(k == "k_compensate16" for k, _ in total[True])
    # the per-shape promises of COMP_SHAPES: the block size the kernels use, the kernel, the branch
    for H, W, bs in fk.COMP_SHAPES:
        assert fk.kernel_bs(H, H // bs) == fk.COMP_BS_CHANGES.get((H, W, bs), bs), (H, W, bs)
    assert set(fk.COMP_BS_CHANGES) <= set(fk.COMP_SHAPES)
    kernel = lambda H, W, bs: fk.comp_kernel(H, W, H // bs)
    assert kernel(64, 96, 16) == kernel(96, 160, 32) == kernel(50, 96, 16) == "k_compensate16"
    assert all(kernel(*s) == "k_compensate" for s in ((80, 160, 32), (64, 90, 16), (70, 90, 16), (60, 84, 12), (66, 90, 6), (45, 50, 5)))
    only = lambda cid: {cls for (_, cls) in per_case[(cid, False)]}
    gathers = {"inside0", "inside1", "inside2", "inside3", "straddle_left", "straddle_right"}
    assert only("66x90-bs6-sx=-1") == only("45x50-bs5-sx=-1") == only("70x90-bs16-sx=-1") == {"pixel_bs"}
    assert only("64x96-bs16-rows-1") == {"pixel_bs"}           # three block rows on 64 rows: bs = 21
    assert not {"pixel_bs", "pixel_tail"} & only("60x84-bs12-sx=-1") and gathers & only("80x160-bs32-sx=-1")
    # the partial last quad of W % 4 != 0 goes per pixel while its neighbours gather: in every field of 64 x 90, and with
    # a vector of its own in the wide fields
    for cid, H, W, bs, mf in fk.comp_cases():
        if (H, W, bs) == (64, 90, 16) and not cid.endswith(("extreme", "rows-1")):
            assert "pixel_tail" in only(cid) and "pixel_bs" not in only(cid) and gathers & only(cid), cid
    for name in fk.TAIL_BOUNDS:
        mf = dict(fk.comp_fields(64, 90, 16))["tail-sx=%s" % name]
        tails = [r for r in fk.comp_runs(64, 90, mf) if r.cls == "pixel_tail"]
        B = {"W-2": 88, "W-1": 89, "W": 90}.get(name, name)
        assert len(tails) == 64 and all(r.x == 88 and r.sx == B for r in tails), name
    assert "beyond" in only("50x96-bs16-sx=-1") and "beyond" in only("64x96-bs16-cols-1")
    assert only("64x96-bs16-extreme") <= {"keep_row", "keep_col"}


def _pixel_sources(H, W, mf):
    """{(block column, source column)} and {(block row, source row)} over the pixels of the frame, with the kernels' block size."""
    k = fk.kernel_bs(H, mf.shape[0])
    cols = {(x // k, x - int(mf[0, x // k, 0])) for x in range(W) if x // k < mf.shape[1]}
    rows = {(y // k, y - int(mf[y // k, 0, 1])) for y in range(H) if y // k < mf.shape[0]}
    return cols, rows


def test_compensation_cases_hit_the_listed_boundaries():
    """Each boundary value is the source of a pixel -- and, where threads gather runs, of a thread run -- in the first and in the
    last block column (row) that the kernels read, found from the kernels' own block size H // rows."""
    for H, W, bs in fk.COMP_SHAPES:
        fields = dict(fk.comp_fields(H, W, bs))
        k = fk.kernel_bs(H, H // bs)
        assert {-16, -15, -1, W - 1, W, W - 16, W - 4} <= set(fk.sx_bounds(W))
        for B in fk.sx_bounds(W):
            mf = fields["sx=%d" % B]
            cols, _ = _pixel_sources(H, W, mf)
            last = max(j for j, _ in cols)
            assert last * k < W and (last + 1 == mf.shape[1] or (last + 1) * k >= W)
            assert (0, B) in cols and (last, B) in cols, (H, W, bs, B)
            for forced in (False, True):
                runs = list(fk.comp_runs(H, W, mf, forced))
                if runs[0].cls != "pixel_bs":
                    seen = {(r.j, r.sx) for r in runs if r.sy is not None and 0 <= r.sy < H}
                    assert (0, B) in seen and (last, B) in seen, (H, W, bs, B, forced)
            if "wide-sx=%d" % B in fields:
                wide = fields["wide-sx=%d" % B]
                assert wide.shape[1] == mf.shape[1] + 1 and (mf.shape[1], B) in _pixel_sources(H, W, wide)[0], (H, W, bs, B)
        for B in fk.sy_bounds(H):
            _, rows = _pixel_sources(H, W, fields["sy=%d" % B])
            assert (0, B) in rows and (H // bs - 1, B) in rows, (H, W, bs, B)
        cols = [_pixel_sources(H, W, fields["last=%d" % s])[0] for s in range(4)]
        last = max(j for j, _ in cols[0])
        assert all((last, last * k - s) in cols[s] for s in range(4))
        ext = fields["extreme"]
        assert ext.dtype == np.int32 and set(ext[..., 0].ravel()) | set(ext[..., 1].ravel()) == set(fk.EXTREMES)
        assert fields["cols-1"].shape == (H // bs, W // bs - 1, 2) and fields["rows-1"].shape == (H // bs - 1, W // bs - 1, 2)
    assert any(n.startswith("wide-") for n, _ in fk.comp_fields(64, 90, 16)) and not any(n.startswith("wide-") for n, _ in fk.comp_fields(64, 96, 16))
    # a 16-pixel run that ends exactly on W with each byte shift next to it, in the last block column of a k_compensate16 shape
    c = collections.Counter()
    for s in range(4):
        runs = [r for r in fk.comp_runs(64, 96, dict(fk.comp_fields(64, 96, 16))["last=%d" % s]) if r.x == 80]
        assert all(r.sx + 16 == 96 - s for r in runs)
        c.update(r.cls for r in runs)
    assert all(c["inside%d" % n] > 0 for n in range(4))


def test_batched_translations_land_on_the_boundaries():
    for H, W, bs in fk.COMP_SEQ_SHAPES:
        tr = fk.seq_translations(H, W)
        assert {d0 for d0, _ in tr} >= {-16, -15, -1, W - 16, W - 1, W} and {d1 for _, d1 in tr} >= {-1, H - 1, H}
    kinds = {fk.comp_kernel(H, W, H // bs) for H, W, bs in fk.COMP_SEQ_SHAPES}
    assert kinds == {"k_compensate16", "k_compensate"}


def test_sse_and_repack_lists():
    ids = [p[0] for p in fk.sse_pairs()]
    assert len(ids) == 9 and "32x256-0v255" in ids and "480x720-255v0" in ids and "1x1-noise" in ids
    # the largest tile sum of k_compensate* (256 x 32 pixels of 255^2) fits the 32-bit partial sums
    assert 256 * 32 * 255 ** 2 < 2 ** 32
    assert {W % 16 == 0 for W in fk.REPACK_WIDTHS} == {True, False} and all(W % 64 for W in fk.REPACK_WIDTHS)
    assert [W % 16 == 0 for _, W in fk.REPACK_STREAMED] == [True, False]


# ---------------------------------------------------------------------------
# the multiply-shift division of k_pyrdown_lds
# ---------------------------------------------------------------------------
def test_multiply_shift_division_is_exact_where_the_launcher_admits_it():
    """r = (it * (2^20 / d + 1)) >> 20 must equal it / d, and the product must fit 32 bits (__umul24 returns the low 32), for
    d = per_row over the staging items (a thread computes the row of base + 256 u, u < 4, before it tests it < total) and for
    d = quads over the (row pair, quad) items.  The predicate's own `per_row < 256` would not be enough -- the division
    fails at d = 255 -- but `pyr_quads < 256` keeps the width below 2048, so per_row stays at or below 128."""
    admitted = [W for W in range(1, 8200) if fk.pyr_lds_geometry(W)[0]]
    assert admitted[0] == 8 and admitted[-1] == 2040
    rows = sorted({fk.pyr_lds_geometry(W)[1] for W in admitted})
    quads = sorted({fk.pyr_lds_geometry(W)[2] for W in admitted})
    assert rows[-1] == 128 and quads[-1] == 255
    for d in rows:
        magic = 2 ** 20 // d + 1
        it = np.arange(fk.PYR_ROWS * d + 768, dtype=np.int64)
        assert it[-1] < 2 ** 24 and magic < 2 ** 24 and int(it[-1]) * magic < 2 ** 32, d
        assert np.array_equal((it * magic) >> 20, it // d), d
    for d in quads:
        magic = 2 ** 20 // d + 1
        it = np.arange((fk.PYR_T // 2) * d, dtype=np.int64)
        assert magic < 2 ** 24 and int(it[-1]) * magic < 2 ** 32, d
        assert np.array_equal((it * magic) >> 20, it // d), d
    # why the quads bound matters: an in-range staging item of a 255-segment row would get the wrong row
    it = np.arange(fk.PYR_ROWS * 255, dtype=np.int64)
    assert not np.array_equal((it * (2 ** 20 // 255 + 1)) >> 20, it // 255)


# ---------------------------------------------------------------------------
# the C oracle against the NumPy restatements
# ---------------------------------------------------------------------------
def test_oracle_pyrdown_equals_numpy_on_every_case():
    co = c_oracle()
    mutated = 0
    for H, W in fk.pyr_shapes() + list(fk.PYR_BATCH_SHAPES):
        for kind in fk.CONTENTS:
            f = fk.content(kind, H, W)
            l1 = co.pyrdown(f)
            assert l1.shape == ((H + 1) // 2, (W + 1) // 2)
            assert np.array_equal(l1, fk.np_pyrdown(f)), (H, W, kind)
            assert np.array_equal(co.pyrdown(l1), fk.np_pyrdown(l1)), (H, W, kind, "level 0")
            mutated += not np.array_equal(l1, fk.np_pyrdown(f, rounding=127))
    assert mutated > 0            # the cases tell (a + 127) >> 8 from (a + 128) >> 8
    assert np.array_equal(fk.np_pyrdown(fk.content("full", 5, 8)), np.full((3, 4), 255, np.uint8))


def test_oracle_compensate_and_sse_equal_numpy_on_every_case():
    co = c_oracle()
    mutated = 0
    for cid, H, W, bs, mf in fk.comp_cases():
        f = fk.comp_frame(H, W)
        want = fk.np_compensate(f, mf)
        assert np.array_equal(co.compensate(f, mf), want), cid
        mutated += not np.array_equal(want, fk.np_compensate(f, mf, right_edge=1))
        if cid.endswith("extreme"):
            assert np.array_equal(want, f), cid
    assert mutated > 0            # the cases tell sb < W from sb < W - 1
    for H, W, bs in fk.COMP_SEQ_SHAPES:
        f, cur = fk.comp_frame(H, W), fk.content("noise", H, W, seed=4)
        for d0, d1 in fk.seq_translations(H, W):
            mf = np.tile(np.array([d0, d1], np.int32), (H // bs, W // bs, 1))
            want = fk.np_compensate(f, mf)
            assert np.array_equal(co.compensate(f, mf), want), (H, W, bs, d0, d1)
            assert co.sse(cur, want) == fk.np_sse(cur, want)
    for sid, a, b in fk.sse_pairs():
        assert co.sse(a, b) == fk.np_sse(a, b), sid
        if "v" in sid:
            assert co.sse(a, b) == 255 ** 2 * a.size, sid
