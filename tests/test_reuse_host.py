"""The cases of tests/reuse_cases.py, checked without a device: the steps cover every gme_seq_* call the header declares, every
step's result grows and shrinks along the schedule, the expectations of two different demands are never the same arrays (a
stale buffer cannot pass for a fresh result), and the block-matching fields are those of both oracles."""
import numpy as np

import lifetime_cases as lc
import reuse_cases as rc
from helpers import c_oracle, np_oracle


def test_every_declared_call_is_driven_or_exempt():
    """Every gme_seq_* declaration of include/gme_hip.h is driven by a step or stands in reuse_cases.EXEMPT with its reason.  A
    pass added to the header fails here until it joins."""
    decl = lc.header_declarations()
    assert len(decl) > 40 and "gme_seq_denoise" in decl and "gme_seq_create" in decl, sorted(decl)
    driven = {c for s in rc.STEPS.values() for c in s.calls}
    assert driven <= set(decl), sorted(driven - set(decl))
    assert set(rc.EXEMPT) <= set(decl), sorted(set(rc.EXEMPT) - set(decl))
    for name, reason in rc.EXEMPT.items():
        assert reason and name not in driven, name
    assert sorted(set(decl) - driven - set(rc.EXEMPT)) == []
    # the passes the suite had never asked one sequence for at two sizes
    for name in ("hier", "vbs", "compensate_vbs", "bipred", "predict_bipred", "gmc", "predict_gmc", "prop", "interp", "obmc", "denoise",
                 "warp_frames", "read_warped_range", "frame_sse", "warp_fill", "gme_begin_fit2", "gme_fit2", "gme_device_solve",
                 "gme_device_solve2", "refine_projective", "compensate_projective", "bbme_streamed"):
        assert "gme_seq_" + name in driven, name


def test_steps_groups_and_events_are_consistent():
    assert all(s in rc.STEPS for g in rc.GROUPS.values() for s in g)
    assert {s for g in rc.GROUPS.values() for s in g} == set(rc.STEPS)              # every step runs in some group
    assert set(rc.SPLIT_LIBRARY) | set(rc.SPLIT_WRAPPER) <= set(rc.GROUPS) and set(rc.NO_SPLIT) <= set(rc.STEPS)
    split = {s for g in rc.SPLIT_LIBRARY + rc.SPLIT_WRAPPER for s in rc.GROUPS[g]}
    assert not split & set(rc.NO_SPLIT) and split | set(rc.NO_SPLIT) == set(rc.STEPS)      # every other step also runs in split-phase mode
    writers = {s.name for s in rc.STEPS.values() if s.planes is not None}
    assert writers == {s.name for s in rc.STEPS.values() if set(s.events) & set(lc.COMP_WRITERS)}
    for s in rc.STEPS.values():
        assert set(s.events) <= set(lc.EVENTS), s.name
        assert {lc.EVENTS[e] for e in s.events} <= set(s.calls) | {"gme_seq_compensate", "gme_seq_compensate2", "gme_seq_gme_begin_fit"}, s.name


def test_schedule():
    """At least five demands over three distinct ones; the frame counts, distances and block sizes change; the stack changes once;
    one adjacent pair has equal shapes and different searches."""
    assert len(rc.SCHEDULE) >= 5 and len(set(rc.SCHEDULE)) >= 3 and len(rc.STACKS) == len(rc.SCHEDULE)
    assert len({d.v for d in set(rc.SCHEDULE)}) == len(set(rc.SCHEDULE)) and all(0 <= d.v < 4 for d in rc.SCHEDULE)
    for field in ("n", "fd", "bs", "sw", "proc", "norm"):
        assert len({getattr(d, field) for d in rc.SCHEDULE}) > 1, field
    assert sum(a != b for a, b in zip(rc.STACKS, rc.STACKS[1:])) == 1
    i, j = rc.EQUAL_SHAPES
    a, b = rc.SCHEDULE[i], rc.SCHEDULE[j]
    assert j == i + 1 and rc.STACKS[i] == rc.STACKS[j] and (a.n, a.fd, a.bs) == (b.n, b.fd, b.bs) and rc.search(a) != rc.search(b)
    assert rc.PLAN[a.name] != rc.PLAN[b.name] and set(rc.PLAN) >= {d.name for d in rc.SCHEDULE}
    # at block size 16 under MSE both kinds of box-sum table occur: the matrix-core kernel's and the elimination kernel's
    mse16 = {rc.PLAN[d.name] for d in rc.SCHEDULE if (d.bs, d.proc, d.norm) == (16, rc.EXHAUSTIVE, rc.MSE)}
    assert {"k_exh_mfma16", "k_exh_sea16_mse"} <= mse16
    assert (rc.S7.n, rc.S7.bs, rc.S7.norm) == (rc.M.n, rc.M.bs, rc.M.norm) and rc.PLAN["S7"] != rc.PLAN["M"]      # both kinds at one frame count
    assert rc.stack("A").shape == rc.stack("B").shape == (rc.N, rc.H, rc.W) and rc.W % 64 != 0
    assert not np.array_equal(rc.stack("A"), rc.stack("B"))
    for d in rc.SCHEDULE:
        assert 2 * d.fd + 1 <= d.n <= rc.N and rc.H % d.bs == 0 and rc.W % d.bs == 0, d
        for mode in rc.DENOISE_MODES:
            a = rc.denoise_args(d, mode)
            assert 2 * a[5] * a[0] + 1 <= d.n, (d, mode)


def test_rise_and_fall():
    """The element count of every step's result strictly rises and strictly falls along the schedule."""
    for step in rc.STEPS:
        e = [rc.elements(rc.expected(step, i)) for i in range(len(rc.SCHEDULE))]
        assert all(n > 0 for n in e), (step, e)
        assert any(b > a for a, b in zip(e, e[1:])) and any(b < a for a, b in zip(e, e[1:])), (step, e)


def test_discrimination():
    """The expectations of a step at two different entries of the schedule differ in shape or bytes, and at the pair of equal
    shapes in bytes."""
    assert rc.discrimination_failures() == []
    i, j = rc.EQUAL_SHAPES
    for step in rc.STEPS:
        a, b = rc.expected(step, i), rc.expected(step, j)
        assert rc.same_shapes(a, b), step
        assert not rc.same_result(a, b), step
    # the caller-given parameters differ too, so that a kept parameter block cannot pass either
    for make in (rc.affine_rows, rc.order2_rows, rc.frame_warps, rc.camera_field, lambda d: rc.named_warps(d, rc.pairs(d)),
                 lambda d: rc.usable_warps(d, rc.pairs(d)), lambda d: rc.fill_candidates(d)[1]):
        assert not np.array_equal(make(rc.SCHEDULE[i]), make(rc.SCHEDULE[j]))


def test_the_solves_are_not_vacuous():
    """The host path solves every pair of the affine estimate at every demand; the second-order one everywhere but where level 1
    is too small for its model, and there it solves none (the device must flag them all)."""
    for i, d in enumerate(rc.SCHEDULE):
        assert all(r is not None for r in rc.expected("solve", i)["pairs"]), d
        solved = [r is not None for r in rc.expected("solve2", i)["pairs"]]
        assert all(solved) or (not any(solved) and rc.MODEL_OF[d.name] == "quadratic" and d.bs == 16), (d, solved)
    assert any(all(r is not None for r in rc.expected("solve2", i)["pairs"]) for i in range(len(rc.SCHEDULE)))
    # wherever the host solves every pair, some pair is clear of rounding ties: there the device may not flag it
    for step, clear in (("solve", rc.clear_solve), ("solve2", rc.clear_solve2)):
        for i, d in enumerate(rc.SCHEDULE):
            rows = rc.expected(step, i)["pairs"]
            if all(r is not None for r in rows):
                assert any(clear(r, d) for r in rows), (step, d)


def test_fields_equal_both_oracles():
    """The expected block-matching fields of one demand, and one backward search of a composite pass, by the C and the NumPy oracle."""
    co, o = c_oracle(), np_oracle()
    d = rc.L
    frames = rc.stack("A")[:d.n]
    want = rc.expected("bbme", 1)["mv"]
    assert want.shape == (rc.pairs(d), rc.H // d.bs, rc.W // d.bs, 2) and want.any()
    for k in range(rc.pairs(d)):
        args = (frames[k], frames[k + d.fd], d.bs, d.sw, d.proc, d.norm)
        assert np.array_equal(want[k], co.bbme(*args)) and np.array_equal(want[k], np.asarray(o.get_motion_field(*args))), k
    # a backward search of the composite passes (the target as the previous frame), under MSE at block size 16
    d = rc.S
    frames = rc.stack("A")[:d.n]
    f0 = rc.expected("bipred", 0)["f0"]
    assert f0.shape[0] == d.n - 2 * d.fd
    args = (frames[d.fd], frames[0], d.bs, d.sw, d.proc, d.norm)
    assert np.array_equal(f0[0], co.bbme(*args)) and np.array_equal(f0[0], np.asarray(o.get_motion_field(*args)))
