"""The result lifetimes of a resident sequence on the device against the table of tests/lifetime_cases.py (include/gme_hip.h,
"Result lifetimes"): one sequence is brought to the full state (every producer has run, every reader equals its host
definition), one event is applied, and every reader must refuse, return the bytes it returned before, or equal the host
definition on what the sequence now holds, as the table says.  Then every producer runs again, so that no refusal leaves a family
stuck.  Needs an MI355X."""
import numpy as np
import pytest

import lifetime_cases as lc

pytestmark = pytest.mark.gpu

LAST = lc.N - lc.FD - 1                                          # the last compensated plane the sequence has room for
COMP_PROBES = ("read_compensated[first]", "read_compensated[last]", "read_compensated_range[written]", "read_compensated_range[all]")
WRITERS = lc.COMP_WRITERS                                        # as readers they run last, gme_seq_predict_bipred at the very end
PLAIN = tuple(r for r in lc.READERS if r not in WRITERS)         # the readers that write nothing, the probes among them
REFUSED = ("refused",)


@pytest.fixture(scope="module")
def native():
    import _gme_native
    ctx = _gme_native.default_context()
    assert "gfx950" in ctx.info()["name"]
    return _gme_native


def same(got, want):
    if len(got) != len(want):
        return False
    for g, w in zip(got, want):
        g, w = np.asarray(g), np.asarray(w)
        if g.shape != w.shape:
            return False
        if w.dtype.kind == "f":
            if g.dtype != w.dtype or np.ascontiguousarray(g).tobytes() != np.ascontiguousarray(w).tobytes():
                return False
        elif not np.array_equal(g, w):
            return False
    return True


class Rig:
    """One sequence and what the host definitions say it holds: ``frames`` / ``n`` the frames on the device and how many are in
    use, ``mv`` its motion field, ``want[reader]`` the arrays a reader returns where it does not refuse."""

    def __init__(self, native, split=False):
        self.native, self.split = native, split
        self.frames, self.n = lc.stack("A"), lc.N
        self.seq = native.Sequence.from_frames(native.default_context(), self.frames)
        self.mv, self.want, self.comp, self.sprite = None, {}, None, None
        self.fail, self.where = [], "build"

    def close(self):
        if self.split:
            self.seq.set_split_phase(False)
        self.seq.close()

    def cur(self):
        return self.frames[:self.n]

    def pairs(self):
        return self.n - lc.FD

    def wait(self):
        if self.split:
            self.seq.wait()

    def note(self, what, *detail):
        self.fail.append("%s: %s %s" % (self.where, what, " ".join(str(d) for d in detail)))

    # ---- producers (v 0: the full state, v 1: as an event) ----------------------------------------------------------------------
    def bbme(self, v):
        a = lc.ARGS["bbme"][v]
        self.seq.bbme(*a)
        self.mv = lc.host_bbme(self.cur(), a)
        self.want["read_mv"] = (self.mv,)

    def bbme_streamed(self, v):
        a = lc.ARGS["bbme"][v]
        self.frames = lc.stack("B")
        out = np.array(self.seq.bbme_streamed(self.frames, *a, chunk_frames=2))
        self.mv = lc.host_bbme(self.cur(), a)
        self.want["read_mv"] = (self.mv,)
        if not same((out,), (self.mv,)):
            self.note("bbme_streamed", "its own result differs from the C oracle")

    def hier(self, v):
        a = lc.ARGS["hier"][v]
        self.seq.hier(*a)
        fields, costs = lc.host_hier(self.cur(), a)
        self.mv = fields[1]
        self.want.update({"read_mv": (self.mv,), "read_hier[1]": (fields[0], costs[0]), "read_hier[2]": (fields[1], costs[1])})

    def prop(self, v):
        a = lc.ARGS["prop"][v]
        self.seq.prop(*a, lc.prop_camera(v, self.pairs()))
        res = lc.host_prop(self.cur(), self.mv, a, v)
        self.mv = res[0]
        self.want.update({"read_mv": (self.mv,), "read_prop": res})

    def subpel(self, v):
        a = lc.ARGS["subpel"][v]
        self.seq.subpel(*a)
        q, cost, planes, sse = lc.host_subpel(self.cur(), self.mv, a)
        self.want.update({"read_qmv": (q, cost), "compensate_qpel": (sse, planes)})

    def vbs(self, v):
        a = lc.ARGS["vbs"][v]
        self.seq.vbs(*a)
        leaf, dmap, cost, planes, sse = lc.host_vbs(self.cur(), self.mv, a)
        self.want.update({"read_vbs": (leaf, dmap, cost), "compensate_vbs": (sse, planes)})

    def bipred(self, v):
        a = lc.ARGS["bipred"][v]
        self.seq.bipred(*a)
        r = lc.host_bipred(self.cur(), a)
        self.want.update({"read_bipred": r[:7], "predict_bipred": (r[8], r[7])})

    def gmc(self, v):
        a = lc.ARGS["gmc"][v]
        self.seq.gmc(a[0], lc.named_warps(lc.GMC_WARPS[v], self.pairs()), *a[1:])
        r = lc.host_gmc(self.cur(), a, v)
        self.want.update({"read_gmc": r[:5], "predict_gmc": (r[6], r[5])})

    def gme_begin_fit(self, v):
        a = lc.ARGS["begin_fit"][v]
        p0, sums1 = self.seq.gme_begin_fit(*a)
        self.wait()
        st = lc.host_staged(self.cur(), a)
        if not same((p0, sums1), (st["p0"], st["sums1"])):
            self.note("gme_begin_fit", "its own result differs from the C oracle")
        self.want["read_stage"] = (st["dense"], st["gt1"], st["model1"], st["mask1"], st["thr1"])
        self.want["gme_fit"] = (st["sums2"], st["gt2"], st["model2"], st["mask2"], st["thr2"])

    def warp_frames(self, v):
        border, fill = lc.ARGS["warp_frames"][v]
        valid = self.seq.warp_frames(0, lc.frame_warps(v, self.n), border, fill)
        warped, want_valid = lc.host_warp(self.cur(), v)
        if not same((valid,), (want_valid,)):
            self.note("warp_frames", "its own counts differ from stabilize.warp_frames")
        self.want["read_warped_range"] = (warped[lc.RANGE[0]:lc.RANGE[0] + lc.RANGE[1]],)

    def mosaic(self, v):
        pl = lc.mosaic_plan(v)
        self.seq.mosaic(0, pl["G"], np.asarray(pl["flags"]) == 0, pl["ox"], pl["oy"], pl["Hc"], pl["Wc"], lc.ARGS["mosaic"][v][0], True)
        sprite, count = lc.host_mosaic(self.cur(), v)
        self.sprite = (sprite, count, v)
        self.want["read_mosaic"] = (sprite, count)

    def moving_masks(self, v):
        sprite, count, plan_v = self.sprite
        pl = lc.mosaic_plan(plan_v)
        threshold, min_count = lc.ARGS["moving_masks"][v]
        known, moving = self.seq.moving_masks(0, pl["A"], np.asarray(pl["flags"]) == 0, pl["ox"], pl["oy"], threshold, min_count)
        masks, want_known, want_moving = lc.host_masks(self.cur(), sprite, count, plan_v, v)
        if not same((known, moving), (want_known, want_moving)):
            self.note("moving_masks", "its own counts differ from mosaic.moving_masks")
        self.want["read_masks_range"] = (masks[lc.RANGE[0]:lc.RANGE[0] + lc.RANGE[1]],)

    # ---- the writers of the compensated planes -> (sse, planes), as readers (v 0) and as events (v 1) -------------------------------
    def frames_want(self, reader, v=0):
        """What the readers that depend on nothing but the frames return."""
        if reader == "read_frame":
            return (self.frames,)
        planes, sse = {"compensate": lambda: lc.host_compensate(self.cur(), 1, v), "compensate2": lambda: lc.host_compensate(self.cur(), 2, v),
                       "compensate_projective": lambda: lc.host_compensate_projective(self.cur(), v)}[reader]()
        return (sse, planes)

    def write(self, writer, v=0):
        seq, P = self.seq, self.pairs()
        if writer == "compensate":
            sse = seq.compensate(lc.FD, lc.BS, lc.comp_params(v, P))
        elif writer == "compensate2":
            sse = seq.compensate2(lc.FD, lc.BS, lc.comp2_params(v, P))
        elif writer == "compensate_projective":
            sse = seq.compensate_projective(lc.FD, lc.named_warps(lc.PROJ_WARPS[v], P))
        elif writer == "compensate_qpel":
            sse = seq.compensate_qpel(lc.FD, lc.BS)
        elif writer == "compensate_vbs":
            sse = seq.compensate_vbs(lc.FD, lc.BS)
        elif writer == "predict_bipred":
            sse = seq.predict_bipred()
        else:
            sse = seq.predict_gmc()
        self.wait()
        sse = np.array(sse)
        want = self.frames_want(writer, v) if lc.READERS[writer][0] == "frames" else self.want[writer]
        self.comp = want[1]                                       # the planes the sequence holds now, by the host definitions
        return sse, seq.read_compensated_range(0, len(sse))

    def comp_want(self, probe):
        """What a probe of the compensated planes returns after the last writer, None where it refuses."""
        planes = self.comp
        if probe == "read_compensated[first]":
            return (planes[0],)
        if probe == "read_compensated_range[written]":
            return (planes,)
        if len(planes) <= LAST:
            return None
        return (planes[LAST],) if probe == "read_compensated[last]" else (planes[:LAST + 1],)

    # ---- readers -> a tuple of arrays -----------------------------------------------------------------------------------------------
    def call(self, reader):
        seq = self.seq
        if reader in WRITERS:
            return self.write(reader)
        if reader == "read_frame":
            return (np.stack([seq.read_frame(k) for k in range(lc.N)]),)
        if reader == "read_mv":
            return (seq.read_mv(),)
        if reader.startswith("read_hier["):
            return seq.read_hier(int(reader[-2]))
        if reader in ("read_qmv", "read_vbs", "read_bipred", "read_gmc", "read_prop", "read_mosaic"):
            return getattr(seq, reader)()
        if reader == "read_stage":
            rows = [(seq.gme_read_stage(0, p)["gt"], seq.gme_read_stage(1, p)) for p in range(seq._gme[2])]
            return (np.stack([d for d, _ in rows]),) + tuple(np.stack([np.asarray(st[k]) for _, st in rows]) for k in ("gt", "model", "mask", "thr"))
        if reader == "gme_fit":
            P = seq._gme[2]
            sums = seq.gme_fit(lc.FIT_LEVEL, lc.fit_params(P), lc.FIT_FRACTION)
            self.wait()
            sums = np.array(sums)
            rows = [seq.gme_read_stage(lc.FIT_LEVEL, p) for p in range(P)]
            return (sums,) + tuple(np.stack([np.asarray(st[k]) for st in rows]) for k in ("gt", "model", "mask", "thr"))
        if reader == "read_compensated[first]":
            return (seq.read_compensated(0),)
        if reader == "read_compensated[last]":
            return (seq.read_compensated(LAST),)
        if reader == "read_compensated_range[written]":
            return (seq.read_compensated_range(0, len(self.comp)),)
        if reader == "read_compensated_range[all]":
            return (seq.read_compensated_range(0, LAST + 1),)
        if reader == "read_warped_range":
            return (seq.read_warped_range(*lc.RANGE),)
        if reader == "read_masks_range":
            return (seq.read_masks_range(*lc.RANGE),)
        raise KeyError(reader)

    def read(self, reader):
        """("ok", arrays), ("refused",) for GmeError carrying the state error, ("error", text) for anything else."""
        try:
            return ("ok",) + tuple(self.call(reader))
        except self.native.GmeError as e:
            return REFUSED if "(code %d)" % self.native.ERR_STATE in str(e) else ("error", repr(e))
        except (IndexError, AssertionError, MemoryError) as e:
            return ("error", repr(e))

    def expect(self, reader, want):
        """``want``: the arrays, or None for a refusal."""
        got = self.read(reader)
        if want is None:
            if got != REFUSED:
                self.note(reader, "should refuse with the state error, but gave", got[0], got[1] if got[0] == "error" else "")
        elif got[0] != "ok" or not same(got[1:], want):
            self.note(reader, "should equal its host definition, but", "differs" if got[0] == "ok" else got)

    def fresh(self, reader):
        if reader in COMP_PROBES:
            return self.comp_want(reader)
        return self.frames_want(reader) if lc.READERS[reader][0] == "frames" else self.want[reader]

    # ---- the full state ---------------------------------------------------------------------------------------------------------------
    def build(self, tail):
        """Every producer on the frames in use, every reader against its host definition.  ``tail``: the block-matching call that
        runs last ("hier" or "prop"); the other one's result ends there."""
        for producer, readers in (("warp_frames", ("read_warped_range",)), ("mosaic", ("read_mosaic",)), ("moving_masks", ("read_masks_range",)),
                                  ("gme_begin_fit", ("read_stage", "gme_fit")), ("bipred", ("read_bipred",)), ("gmc", ("read_gmc",)),
                                  ("bbme", ("read_mv",))):
            getattr(self, producer)(0)
            for r in readers:
                self.expect(r, self.want[r])
        first = "prop" if tail == "hier" else "hier"
        for producer in (first, tail):
            getattr(self, producer)(0)
            for r in ("read_mv",) + (("read_prop",) if producer == "prop" else ("read_hier[1]", "read_hier[2]")):
                self.expect(r, self.want[r])
        for r in (("read_prop",) if first == "prop" else ("read_hier[1]", "read_hier[2]")):
            self.expect(r, None)
        self.subpel(0)
        self.expect("read_qmv", self.want["read_qmv"])
        self.vbs(0)
        self.expect("read_vbs", self.want["read_vbs"])
        self.expect("read_frame", self.fresh("read_frame"))
        for w in WRITERS:
            self.expect(w, self.fresh(w))
            for probe in COMP_PROBES:
                self.expect(probe, self.comp_want(probe))
        return first

    def snapshot(self):
        before = {r: self.read(r) for r in PLAIN + WRITERS}
        before.update({r: self.read(r) for r in COMP_PROBES})      # behind the last writer among the readers
        return before

    def check(self, event, reader, before):
        what = lc.TABLE[event, reader]
        if what == lc.REFUSES:
            self.expect(reader, None)
        elif what == lc.FRESH:
            self.expect(reader, self.fresh(reader))
        else:
            got = self.read(reader)
            if got[0] != before[reader][0] or (got[0] == "ok" and not same(got[1:], before[reader][1:])) or got[0] == "error":
                self.note(reader, "should be unchanged (%s before), but is" % before[reader][0], got[0] if got[0] != "ok" else "other bytes")

    # ---- events -------------------------------------------------------------------------------------------------------------------
    def apply(self, event):
        seq = self.seq
        if event == "upload_all":
            self.frames = lc.stack("B")
            seq.upload(0, self.frames)
        elif event == "upload_one":
            self.frames = lc.stack("A+B[slot]")
            seq.upload(lc.SLOT, self.frames[lc.SLOT:lc.SLOT + 1])
        elif event == "synth":
            self.frames = lc.stack("synth")
            seq.synth(lc.SYNTH_SEED, lc.SYNTH_T0)
        elif event == "invalidate_pyramids":
            seq.invalidate_pyramids()
        elif event in ("set_frames_4", "set_frames_4_and_back"):
            seq.set_frames(lc.N_SHORT)
            self.n = lc.N_SHORT
            if event == "set_frames_4_and_back":
                seq.set_frames(lc.N)
                self.n = lc.N
        elif event in WRITERS:
            got = self.write(event, 1)
            want = self.frames_want(event, 1) if lc.READERS[event][0] == "frames" else self.want[event]
            if not same(got, want):
                self.note(event, "its own result differs from its host definition")
        else:
            getattr(self, event)(1)
        self.wait()
        if event in lc.FRAME_EVENTS:
            assert (self.frames is lc.stack(lc.FRAME_EVENTS[event][0]) or event.startswith("set_frames")) and self.n == lc.FRAME_EVENTS[event][1]


def run_event(native, event, split=False):
    failures = []
    for tail in ("hier", "prop"):
        rig = Rig(native)
        rig.where = "%s, %s last, the full state" % (event, tail)
        ended = rig.build(tail)
        rig.where = "%s, %s last, before" % (event, tail)
        before = rig.snapshot()
        # the full state: everything readable but the block-matching result that `tail` ended and, behind predict_bipred, the last plane
        for r, got in before.items():
            refused = (lc.READERS[r][0] == ended) or (lc.READERS[r][0] == "comp_last")
            if (got == REFUSED) != refused or got[0] == "error":
                rig.note(r, "is", got[0], "in the full state")
        if split:
            native._check(rig.seq.lib.gme_seq_set_split_phase(rig.seq.handle, 1), rig.seq.lib)       # the library's switch alone: the
            rig.split = True                                      # wrappers keep plain buffers and let the blocking calls through
        rig.where = "%s, %s last" % (event, tail)
        rig.apply(event)
        for r in PLAIN + WRITERS:
            rig.check(event, r, before)
        # after the walk: the readers wrote the compensated planes; everything else is where the table put it
        rig.where = "%s, %s last, after the walk" % (event, tail)
        for r in PLAIN:
            if r in COMP_PROBES:
                rig.expect(r, rig.comp_want(r))
            else:
                rig.check(event, r, before)
        # no family is stuck: every producer again, on what the sequence holds now
        rig.where = "%s, %s last, producers again" % (event, tail)
        rig.build(tail)
        if split:
            native._check(rig.seq.lib.gme_seq_set_split_phase(rig.seq.handle, 0), rig.seq.lib)
            rig.split = False
        failures += rig.fail
        rig.close()
    assert not failures, "%d cells:\n%s" % (len(failures), "\n".join(failures))


@pytest.mark.parametrize("event", tuple(lc.EVENTS))
def test_event(native, event):
    run_event(native, event)


def test_split_phase(native):
    """The events that bring new frame data with the library in split-phase mode: gme_seq_upload only queues its copies there, and
    the producers behind it block "also in split-phase mode"."""
    for event in lc.FRAME_EVENTS:
        run_event(native, event, split=True)


@pytest.mark.parametrize("n", (lc.N, lc.N_SHORT))
@pytest.mark.parametrize("writer", WRITERS)
def test_compensated_planes_written(native, writer, n):
    """A sequence on which nothing has compensated yet refuses every read; after its first writer it serves the planes that writer
    wrote and refuses the others (under gme_seq_set_frames(4) every writer leaves the last plane out, gme_seq_predict_bipred
    two); a second writer ends the planes of the first."""
    rig = Rig(native)
    rig.where = "%s on a fresh sequence of %d" % (writer, n)
    for probe in COMP_PROBES[:2] + COMP_PROBES[3:]:
        rig.expect(probe, None)
    if n != lc.N:
        rig.seq.set_frames(n)
        rig.n = n
    for producer in {"compensate_qpel": ("bbme", "subpel"), "compensate_vbs": ("bbme", "vbs"), "predict_bipred": ("bipred",),
                     "predict_gmc": ("gmc",)}.get(writer, ()):
        getattr(rig, producer)(0)
    rig.expect(writer, rig.fresh(writer))
    count = len(rig.comp)
    assert count == (n - 2 * lc.FD if writer == "predict_bipred" else n - lc.FD)
    for probe in COMP_PROBES:
        rig.expect(probe, rig.comp_want(probe))
    for first, cnt in ((0, count + 1), (count, 1), (count - 1, 2)):
        if first + cnt <= LAST + 1:
            rig.where = "%s on a fresh sequence of %d, range (%d, %d)" % (writer, n, first, cnt)
            try:
                rig.seq.read_compensated_range(first, cnt)
                rig.note("read_compensated_range", "served a plane nobody wrote")
            except native.GmeError as e:
                if "(code %d)" % native.ERR_STATE not in str(e):
                    rig.note("read_compensated_range", repr(e))
    # a second writer ends the first one's planes
    if writer != "predict_bipred" and n == lc.N:
        rig.where = "predict_bipred behind %s" % writer
        rig.bipred(0)
        rig.expect("predict_bipred", rig.want["predict_bipred"])
        for probe in COMP_PROBES:
            rig.expect(probe, rig.comp_want(probe))
    fail = rig.fail
    rig.close()
    assert not fail, "\n".join(fail)


def test_bipred_at_frame_distance_2(native):
    """gme_seq_bipred at frame distance 2 has one target on five frames: gme_seq_predict_bipred writes one plane and every other
    one refuses; under gme_seq_set_frames(4) the result ends, and the call itself has too few frames (GME_ERR_ARG)."""
    rig = Rig(native)
    rig.where = "bipred at frame distance 2"
    rig.gmc(0)
    rig.expect("predict_gmc", rig.want["predict_gmc"])             # four planes, which the next writer ends
    rig.bipred(2)
    assert len(rig.want["read_bipred"][0]) == lc.N - 4 == 1
    rig.expect("read_bipred", rig.want["read_bipred"])
    rig.expect("predict_bipred", rig.want["predict_bipred"])
    for probe in COMP_PROBES:
        rig.expect(probe, rig.comp_want(probe))
    try:
        rig.seq.read_compensated(1)
        rig.note("read_compensated(1)", "served a plane nobody wrote")
    except native.GmeError as e:
        assert "(code %d)" % native.ERR_STATE in str(e)
    rig.seq.set_frames(lc.N_SHORT)
    rig.n = lc.N_SHORT
    rig.expect("read_bipred", None)
    rig.expect("predict_bipred", None)
    rig.expect("read_compensated[first]", rig.comp_want("read_compensated[first]"))      # the plane stays readable
    with pytest.raises(IndexError):
        rig.seq.bipred(*lc.ARGS["bipred"][2])
    fail = rig.fail
    rig.close()
    assert not fail, "\n".join(fail)
