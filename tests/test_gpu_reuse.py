"""One long-lived Sequence through every pass at changing sizes (tests/reuse_cases.py): the steps run along a schedule of demands
that makes every device buffer of the sequence grow, shrink in use and serve another family in between, in three orders, and
after every step every array is compared with what the definitions give for that demand -- never with another sequence.  Where
the lifetime rules of include/gme_hip.h end a result, its reader must refuse with the state error, and serve where they do not;
of the compensated planes exactly those of the last writer are served.
Once per order the second stack is uploaded between two demands.  Successful calls only.  Needs an MI355X."""
import pytest

import lifetime_cases as lc
import reuse_cases as rc

pytestmark = pytest.mark.gpu

ORDERS = ("family", "round_robin", "reversed")
# family -> the probe of its reader: one pair (target) with every output NULL, which the header allows
PROBES = {
    "qmv": ("gme_seq_read_qmv", (0, 1, None, None)),
    "hier": ("gme_seq_read_hier", (2, 0, 1, None, None)),
    "vbs": ("gme_seq_read_vbs", (0, 1, None, None, None)),
    "bipred": ("gme_seq_read_bipred", (0, 1, None, None, None, None, None, None, None)),
    "gmc": ("gme_seq_read_gmc", (0, 1, None, None, None, None, None)),
    "prop": ("gme_seq_read_prop", (0, 1, None, None, None)),
    "staged": ("gme_seq_gme_read_stage", (1, 0, None, None, None, None)),
}
# lifetime_cases names its events after its own frame counts; the rules are those of any upload and any change of the count
UPLOAD, SET_FRAMES = "upload_all", "set_frames_4"


@pytest.fixture(scope="module")
def native():
    import _gme_native
    ctx = _gme_native.default_context()
    assert "gfx950" in ctx.info()["name"]
    return _gme_native


@pytest.fixture(scope="module")
def expectations():
    """Every expectation once, before the first sequence exists (reuse_cases caches them per step, demand and stack)."""
    for step in rc.STEPS:
        for i in range(len(rc.SCHEDULE)):
            rc.expected(step, i)
    return rc.expected


class Rig:
    """One sequence, the stack and frame count it holds, and which result families the lifetime rules leave readable."""

    def __init__(self, native, split=None):
        """``split``: None, "library" (the library's switch alone: the wrappers keep ordinary buffers and let the blocking calls
        through) or "wrapper" (Sequence.set_split_phase: the results arrive in the wrapper's page-locked buffers)."""
        self.native, self.ctx = native, native.default_context()
        self.stack, self.n = "A", rc.N
        self.seq = native.Sequence.from_frames(self.ctx, rc.stack("A"))
        self.valid = {family: False for family in PROBES}          # before any producer every reader refuses
        self.planes = 0                                            # compensated planes of the last writer
        self.split = split
        self.switch(True)
        self.plans = {}

    def switch(self, on):
        if self.split == "wrapper":
            self.seq.set_split_phase(on)
        elif self.split == "library":
            self.native._check(self.seq.lib.gme_seq_set_split_phase(self.seq.handle, int(on)), self.seq.lib)

    def close(self):
        self.switch(False)
        self.seq.close()

    def plane(self, index):
        """True where gme_seq_read_compensated serves plane ``index``, False where it refuses with the state error."""
        try:
            self.seq.read_compensated(index)
            return True
        except self.native.GmeError as e:
            assert "(code %d)" % self.native.ERR_STATE in str(e), e
            return False

    def wait(self):
        if self.split:
            self.seq.wait()

    def event(self, name):
        for family in self.valid:
            rule = lc.RULES[family].get(name)
            if rule == lc.REFUSES:
                self.valid[family] = False
            elif rule == lc.FRESH:
                self.valid[family] = True

    def demand(self, d, stack):
        """The stack and the frame count of a demand: an upload of all frames and gme_seq_set_frames where they change."""
        if stack != self.stack:
            self.stack = stack
            self.seq.upload(0, rc.stack(stack))
            self.wait()
            self.event(UPLOAD)
        if d.n != self.n:
            self.seq.set_frames(d.n)
            self.n = d.n
            self.event(SET_FRAMES)

    def step(self, name, d, stack):
        """One step at a demand on a stack: every array against the definitions, every family's reader served or refused as the
        lifetime rules say, the compensated planes of the last writer served and the next one refused, and after gme_seq_bbme
        the kernel the demand is named for."""
        self.demand(d, stack)
        s = rc.STEPS[name]
        where = (name, d.name, stack)
        if name == "bbme_streamed":
            got = s.run(self.seq, d, self.wait, rc.stack(stack))
        else:
            got = s.run(self.seq, d, self.wait)
        if name == "bbme":
            self.plans[d.name] = self.ctx.last_bbme_info()["plan"]
        rc.compare(name, got, rc.expected_for(name, d, stack), where, d)
        for e in s.events:
            self.event(e)
        lib = self.seq.lib
        for family, (call, args) in PROBES.items():
            got_rc = getattr(lib, call)(self.seq.handle, *args)
            assert got_rc == (0 if self.valid[family] else self.native.ERR_STATE), where + (call, "readable" if self.valid[family] else "ended", got_rc)
        # "each call writes planes 0 .. its own count - 1 and ends the planes of the call before it": whatever an earlier, larger
        # writer left behind the last writer's planes is refused, and before any writer plane 0 is
        if s.planes is not None:
            self.planes = s.planes(d)
        assert self.planes == 0 or self.plane(self.planes - 1), where + ("plane", self.planes - 1, "of the last writer is refused")
        for beyond in range(self.planes, rc.N):
            assert not self.plane(beyond), where + ("plane", beyond, "is served, the last writer wrote", self.planes)
        if name == "bbme":
            assert self.plans[d.name].startswith(rc.PLAN[d.name]), (where, self.plans[d.name])


def walk(order, steps):
    """[(step, schedule index)] in the order asked for."""
    entries = range(len(rc.SCHEDULE))
    if order == "family":
        return [(s, i) for s in steps for i in entries]
    if order == "round_robin":
        return [(s, i) for i in entries for s in steps]
    return [(s, i) for i in entries for s in reversed(steps)]


def run(native, order, group, split=None):
    rig = Rig(native, split)
    try:
        for name, index in walk(order, rc.GROUPS[group]):
            rig.step(name, rc.SCHEDULE[index], rc.STACKS[index])
    finally:
        rig.close()


@pytest.mark.parametrize("group", tuple(rc.GROUPS))
@pytest.mark.parametrize("order", ORDERS)
def test_reuse(native, expectations, order, group):
    run(native, order, group)


@pytest.mark.parametrize("group", rc.SPLIT_LIBRARY)
def test_reuse_split_phase(native, expectations, group):
    """The round-robin order with the library in split-phase mode: the staged calls, the compensations, the device solves and the
    upload only queue their work there, every other call of these groups blocks "also in split-phase mode"."""
    run(native, "round_robin", group, split="library")


@pytest.mark.parametrize("group", rc.SPLIT_WRAPPER)
def test_reuse_split_phase_page_locked(native, expectations, group):
    """... through Sequence.set_split_phase(True): the queued calls hand back the wrapper's page-locked buffers, reused from one
    demand to the next, which the library fills from the device while the caller is elsewhere."""
    run(native, "round_robin", group, split="wrapper")


def test_both_box_sum_tables_on_one_sequence(native):
    """Block size 16 under MSE at one frame count, so that nothing but the search itself asks for another table: the matrix-core
    kernel's signed table (S7) and the elimination kernel's plain one (M) each behind the other, behind the backward searches of
    gme_seq_gmc and gme_seq_bipred that index the same table by frame, and behind an upload that changes the frames under a table
    of the kind the next search wants."""
    rig = Rig(native)
    try:
        for name, d, stack in (("bbme", rc.S7, "A"), ("bbme", rc.M, "A"), ("gmc", rc.S7, "A"), ("bipred", rc.M, "A"), ("bipred", rc.M, "B"),
                               ("bbme", rc.M, "B"), ("bbme", rc.S7, "B"), ("gmc", rc.S7, "A"), ("bbme", rc.S7, "A"), ("denoise_r1", rc.M, "A"),
                               ("denoise_r1", rc.M, "B"), ("denoise_r2", rc.S7, "B")):
            assert d.n == rc.N
            rig.step(name, d, stack)
        assert rig.plans["S7"].startswith("k_exh_mfma16") and rig.plans["M"].startswith("k_exh_sea16_mse"), rig.plans
    finally:
        rig.close()
