"""The staged estimate (roadmap.stages) under each of its drivers, on a recording stand-in for a device sequence: the
blocking helper, ShardedSequence's round robin over split-phase lanes and StreamEstimator's poll loop must issue the same
stage calls per lane, in the order the overlap of one lane's host solves with the other lanes' kernels depends on."""
import types

import numpy as np
import pytest

_X, _Y = (a.ravel().astype(np.float64) for a in np.meshgrid(np.arange(6), np.arange(5)))


def _canned_sums(order, pairs, level):
    """Normal-equation sums of a well-posed fit (30 points), different per level -> float64[pairs, 15 or 27]."""
    import roadmap
    dx = 1.0 + 0.1 * _X - 0.05 * _Y + 0.01 * level * _X * _Y
    dy = -2.0 + 0.02 * _X * _Y + 0.03 * level * _Y
    phi = [np.ones_like(_X), _X, _Y] if order == 1 else [np.ones_like(_X), _X, _Y, _X * _X, _X * _Y, _Y * _Y]
    phi = np.stack(phi)
    if order == 1:
        head = (phi @ phi.T).ravel()
    else:
        head = [np.sum(_X ** p * _Y ** q) for p, q in sorted(roadmap._MOMENT, key=roadmap._MOMENT.get)]
    return np.tile(np.concatenate([head, phi @ dx, phi @ dy]), (pairs, 1))


class _Ctx:
    def __init__(self, log, name):
        self.log, self.name = log, name

    def sync(self):
        self.log.append((self.name, "sync"))

    def close(self):
        pass


class _Seq:
    """Records every call; the stage calls return canned sums (``singular`` lanes: all-zero sums)."""

    def __init__(self, log, name, n_frames, singular=False, flags=0):
        self.log, self.name, self.N, self.singular, self.flags = log, name, n_frames, singular, flags
        self._split = False

    def _rec(self, *what):
        self.log.append((self.name,) + what)

    def _begin_fit(self, order, frame_distance, bbme_block_size, outlier_fraction, procedure, search_window):
        self._rec("begin_fit", order, frame_distance, bbme_block_size, outlier_fraction, procedure, search_window)
        pairs = self.N - frame_distance
        sums = _canned_sums(order, pairs, 1)
        return np.zeros((pairs, 6), np.float32), sums * 0 if self.singular else sums

    def _fit(self, order, level, params_in, outlier_fraction):
        self._rec("fit", order, level, tuple(np.asarray(params_in).ravel()), outlier_fraction)
        return _canned_sums(order, len(params_in), level)

    def _compensate(self, order, frame_distance, block_size, params):
        self._rec("compensate", order, frame_distance, block_size, tuple(np.asarray(params).ravel()))
        return np.arange(len(params), dtype=np.int64) + 7

    def gme_device_solve(self, frame_distance, bbme_block_size, outlier_fraction, procedure=3, search_window=2):
        self._rec("device_solve", frame_distance)
        pairs = self.N - frame_distance
        return np.ones((pairs, 6)), np.full(pairs, 5, np.int64), np.full(pairs, self.flags, np.int32)

    def set_split_phase(self, on=True):
        self._rec("split", bool(on))
        self._split = bool(on)

    def wait(self):
        self._rec("wait")

    def poll(self):
        return True

    def set_frames(self, n_frames):
        self.N = n_frames

    def upload(self, first, frames):
        self._rec("upload", len(frames))

    def close(self):
        pass


STAGES = ("begin_fit", "fit", "compensate", "device_solve")


def _stage_calls(log, name):
    return [e[1:] for e in log if e[0] == name and e[1] in STAGES]


def _sharded(log, lanes, interleave, fd=1, **seq_kw):
    """A ShardedSequence over stand-in lanes of the given pair counts (no device)."""
    import sequence
    sh = sequence.ShardedSequence.__new__(sequence.ShardedSequence)
    sh.ctx, sh.H, sh.W, sh.fd, sh.interleave, sh._pool, sh.lanes = None, 48, 64, fd, interleave, None, []
    lo = 0
    for j, n in enumerate(lanes):
        name = "lane%d" % j
        sh.lanes.append(sequence._Lane(_Ctx(log, name), _Seq(log, name, n + fd, **seq_kw.get(name, {})), lo, lo + n))
        lo += n
    return sh


@pytest.mark.parametrize("model", ["affine", "similarity", "quadratic"])
def test_drivers_issue_the_same_stage_calls(model):
    import roadmap
    import sequence
    pairs = 4
    want_log = []
    want_p, want_sse = roadmap.estimate_blocking(_Seq(want_log, "lane", pairs + 1), 1, model, 3, 2, compensate=True)
    want = _stage_calls(want_log, "lane")
    order = roadmap.normalize_model(model)[1]
    assert [c[:2] for c in want] == [("begin_fit", order), ("fit", order), ("compensate", order)]
    assert want_p.shape == (pairs, 12 if order == 2 else 6) and list(want_sse) == [7, 8, 9, 10]
    assert np.array_equal(roadmap.estimate_sequence(_Seq([], "x", pairs + 1), 1, model), want_p)

    for interleave in (False, True):
        log = []
        sh = _sharded(log, [pairs] * 3, interleave)
        try:
            got_p, got_psnr = sh.estimate_and_compensate(model=model)
            assert np.array_equal(sh.estimate(model=model), np.concatenate([want_p] * 3))
        finally:
            sh.close()
        assert np.array_equal(got_p, np.concatenate([want_p] * 3))
        assert np.array_equal(got_psnr, sequence.psnr_from_sse(np.tile(want_sse, 3), 48, 64, False))
        for j in range(3):
            assert _stage_calls(log, "lane%d" % j) == want + want[:2], (interleave, j)

    # streamed: one chunk per lane, each covering `pairs` pairs
    log = []
    est = sequence.StreamEstimator.__new__(sequence.StreamEstimator)
    est.H, est.W, est.fd, est.chunk_pairs, est.min_chunk, est.procedure, est.search_window = 48, 64, 1, pairs, pairs, 3, 2
    est.cap = pairs + 1
    est.lanes = [types.SimpleNamespace(ctx=_Ctx(log, "lane%d" % j), seq=_Seq(log, "lane%d" % j, pairs + 1), host=None,
                                       comp_host=None, chain=None, steps=0) for j in range(2)]
    for lane in est.lanes:
        lane.seq._split = True
    frames = np.zeros((2 * pairs + 1, 48, 64), np.uint8)
    got_p, got_psnr = est.run(frames, model=model, exact_psnr=False)
    assert np.array_equal(got_p, np.concatenate([want_p] * 2))
    assert np.array_equal(got_psnr, sequence.psnr_from_sse(np.tile(want_sse, 2), 48, 64, False))
    for j in range(2):
        calls = [e[1:] for e in log if e[0] == "lane%d" % j]
        assert calls[:2] == [("upload", pairs + 1), ("wait",)], calls       # nothing queued behind the upload before it arrived
        assert _stage_calls(log, "lane%d" % j) == want, j
        assert calls[-1] == ("sync",)


def test_round_robin_queues_every_lane_before_the_first_wait():
    log = []
    sh = _sharded(log, [3, 2, 3], interleave=True)
    sh.estimate_and_compensate()
    sh.close()
    kinds = [(e[0], e[1]) for e in log if e[1] != "split"]
    lanes = ["lane0", "lane1", "lane2"]
    want = [(n, "begin_fit") for n in lanes]
    for stage in ("fit", "compensate"):
        for n in lanes:
            want += [(n, "wait"), (n, stage)]                # each lane's next stage right after its own solve
    for n in lanes:
        want += [(n, "wait"), (n, "sync")]
    assert kinds == want
    assert all(not lane.seq._split for lane in sh.lanes)


def test_split_phase_is_off_again_when_a_solve_raises():
    import roadmap
    log = []
    sh = _sharded(log, [3, 3, 3], interleave=True, lane1={"singular": True})
    with pytest.raises(np.linalg.LinAlgError):
        sh.estimate_and_compensate()
    assert all(not lane.seq._split for lane in sh.lanes)
    assert [e[0] for e in log if e[1] == "begin_fit"] == ["lane0", "lane1", "lane2"]
    split = _Seq([], "s", 4)
    split.set_split_phase(True)
    with pytest.raises(RuntimeError, match="needs blocking calls"):
        roadmap.estimate_blocking(split, 1)
    sh.close()


@pytest.mark.parametrize("flagged", [False, True])
def test_device_solve_falls_back_to_the_stages_on_a_flag(monkeypatch, flagged):
    monkeypatch.setenv("GME_DEVICE_SOLVE", "1")
    log = []
    sh = _sharded(log, [2, 2], interleave=False, lane1={"flags": int(flagged)})
    params, _ = sh.estimate_and_compensate()
    sh.close()
    for n in ("lane0", "lane1"):
        kinds = [c[0] for c in _stage_calls(log, n)]
        assert kinds == (["device_solve", "begin_fit", "fit", "compensate"] if flagged else ["device_solve"]), n
    assert np.array_equal(params, np.ones((4, 6))) != flagged
    assert all(not lane.seq._split for lane in sh.lanes)
    # a first-order model other than affine has no device solve
    log.clear()
    sh = _sharded(log, [2], interleave=False)
    sh.estimate_and_compensate(model="translation")
    assert [c[0] for c in _stage_calls(log, "lane0")] == ["begin_fit", "fit", "compensate"]
    sh.close()
