"""The lifetime table of tests/lifetime_cases.py, checked without a device: it covers every reader and every event the header
declares, it has an entry for every pair, every sentence it is taken from stands in the header, and its inputs tell a stale
result from a fresh one."""
import numpy as np

import lifetime_cases as lc


def test_every_declared_call_is_in_the_matrix():
    """A gme_seq_read_*, gme_seq_compensate* or gme_seq_predict_* declaration is a reader of the table; a gme_seq_* call that takes
    no output pointer is an event; anything else of that kind stands in lifetime_cases.EXCEPTIONS with its reason.  A family added
    to the header fails here until it joins the matrix."""
    decl = lc.header_declarations()
    assert len(decl) > 40 and "gme_seq_read_prop" in decl and "gme_seq_create" in decl, sorted(decl)
    read_by = {c for _, calls in lc.READERS.values() for c in calls}
    made_by = set(lc.EVENTS.values())
    assert read_by <= set(decl) and made_by <= set(decl) and set(lc.EXCEPTIONS) <= set(decl), "the table names calls the header does not declare"
    for name, reason in lc.EXCEPTIONS.items():
        assert reason and name not in read_by and name not in made_by, name
    missing = []
    for name, (_, params) in decl.items():
        if name in lc.EXCEPTIONS:
            continue
        if name.startswith(("gme_seq_read_", "gme_seq_compensate", "gme_seq_predict_")) and name not in read_by:
            missing.append(("reader", name))
        if not lc.has_output_pointer(params) and name not in made_by:
            missing.append(("event", name))
    assert not missing, missing
    # the readers and events the lifetime rules were written for
    for name in ("gme_seq_gme_read_stage", "gme_seq_gme_fit"):
        assert name in read_by
    for name in ("gme_seq_bbme_streamed", "gme_seq_gme_begin_fit", "gme_seq_warp_frames", "gme_seq_moving_masks") + tuple(
            "gme_seq_" + w for w in lc.COMP_WRITERS):
        assert name in made_by
    assert not lc.has_output_pointer(["gme_seq *seq", "const double *h"]) and lc.has_output_pointer(["gme_seq *seq", "int64_t *sse_out"])


def test_table_is_total():
    assert set(lc.TABLE) == {(e, r) for e in lc.EVENTS for r in lc.READERS} and len(lc.TABLE) == len(lc.EVENTS) * len(lc.READERS)
    assert set(lc.TABLE.values()) == {lc.REFUSES, lc.UNCHANGED, lc.FRESH}
    families = {fam for fam, _ in lc.READERS.values()}
    assert families == set(lc.RULES), families ^ set(lc.RULES)
    for fam, rule in lc.RULES.items():
        assert set(rule) <= set(lc.EVENTS), (fam, set(rule) - set(lc.EVENTS))
    assert set(lc.FRAME_EVENTS) <= set(lc.EVENTS) and set(lc.COMP_WRITERS) <= set(lc.EVENTS) and set(lc.COMP_WRITERS) <= set(lc.READERS)


def test_table_holds_the_decisions_of_the_header():
    """The three rules of "Result lifetimes" and the cells the fixes were made for."""
    for e in lc.FRAME_EVENTS:
        assert lc.TABLE[e, "read_mv"] == (lc.FRESH if e == "bbme_streamed" else lc.UNCHANGED), e
        for r in ("read_qmv", "compensate_qpel", "read_hier[1]", "read_hier[2]", "read_vbs", "compensate_vbs", "read_prop", "read_bipred",
                  "predict_bipred", "read_gmc", "predict_gmc", "read_stage", "gme_fit"):
            assert lc.TABLE[e, r] == lc.REFUSES, (e, r)
        for r in ("read_warped_range", "read_mosaic", "read_masks_range", "read_compensated[first]", "read_compensated[last]"):
            assert lc.TABLE[e, r] == lc.UNCHANGED, (e, r)
    for r in ("read_qmv", "read_vbs", "read_hier[2]", "read_prop"):
        assert [lc.TABLE[e, r] for e in ("bipred", "gmc", "gme_begin_fit", "warp_frames")] == [lc.UNCHANGED] * 4, r
    assert lc.TABLE["predict_bipred", "read_compensated[last]"] == lc.REFUSES
    assert lc.TABLE["predict_bipred", "read_compensated_range[all]"] == lc.REFUSES
    assert lc.TABLE["predict_gmc", "read_compensated[last]"] == lc.FRESH
    assert lc.TABLE["prop", "read_hier[1]"] == lc.REFUSES and lc.TABLE["hier", "read_prop"] == lc.REFUSES


def test_quoted_sentences_stand_in_the_header():
    text = lc.header_text()
    assert len(lc.QUOTES) >= 19
    for q in lc.QUOTES:
        assert q in text, q


def test_discrimination():
    """On every stack an event uploads, every family's host result differs from the one on stack A, and any two writers of the
    compensated planes leave different planes: a stale read cannot pass as a fresh one.  A condition on the inputs (the seed of
    stack B: lifetime_cases.find_seed_b), not a tolerance."""
    assert lc.discrimination_failures() == []
    a = lc.stack("A")
    for name in lc.CHANGED_STACKS:
        f = lc.stack(name)
        assert f.shape == a.shape == (lc.N, lc.H, lc.W) and f.dtype == np.uint8 and not np.array_equal(f, a)
    assert np.array_equal(lc.stack("A+B[slot]")[lc.SLOT], lc.stack("B")[lc.SLOT])
    assert all(np.array_equal(lc.stack("A+B[slot]")[k], a[k]) for k in range(lc.N) if k != lc.SLOT)
    # the two argument sets of a call give different results on stack A: "fresh" after an event differs from "unchanged"
    mv = lc.host_bbme(a, lc.ARGS["bbme"][0])
    for name, fn in (("bbme", lambda v: (lc.host_bbme(a, lc.ARGS["bbme"][v]),)),
                     ("hier", lambda v: lc.host_hier(a, lc.ARGS["hier"][v])[1]),
                     ("prop", lambda v: lc.host_prop(a, mv, lc.ARGS["prop"][v], v)),
                     ("subpel", lambda v: lc.host_subpel(a, mv, lc.ARGS["subpel"][v])),
                     ("vbs", lambda v: lc.host_vbs(a, mv, lc.ARGS["vbs"][v])),
                     ("bipred", lambda v: lc.host_bipred(a, lc.ARGS["bipred"][v])),
                     ("gmc", lambda v: lc.host_gmc(a, lc.ARGS["gmc"][v], v)),
                     ("begin_fit", lambda v: tuple(lc.host_staged(a, lc.ARGS["begin_fit"][v])[k] for k in ("gt1", "gt2", "sums1"))),
                     ("compensate", lambda v: lc.host_compensate(a, 1, v)), ("compensate2", lambda v: lc.host_compensate(a, 2, v)),
                     ("compensate_projective", lambda v: lc.host_compensate_projective(a, v)),
                     ("warp_frames", lambda v: lc.host_warp(a, v)), ("mosaic", lambda v: lc.host_mosaic(a, v)),
                     ("moving_masks", lambda v: lc.host_masks(a, *lc.host_mosaic(a, 0), 0, v))):
        assert not lc.same_arrays(fn(0), fn(1)), name


def test_shorter_sequence_is_told_apart():
    """gme_seq_set_frames(4): every family's result has one pair (target, frame) fewer, so its shape alone differs."""
    short = lc.stack("A")[:lc.N_SHORT]
    assert len(lc.host_bbme(short, lc.ARGS["bbme"][0])) == lc.N_SHORT - lc.FD
    assert len(lc.host_bipred(short, lc.ARGS["bipred"][0])[0]) == lc.N_SHORT - 2 * lc.FD
    assert len(lc.host_compensate(short, 1, 0)[0]) == lc.N_SHORT - lc.FD < lc.N - lc.FD
