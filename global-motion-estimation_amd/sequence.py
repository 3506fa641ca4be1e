"""Whole-sequence (batch) form of the hot path and its multi-GPU sharding.

The reference processes a video as independent frame pairs (results.py:41-59): pair ``p``
is ``(frames[p], frames[p + fd])`` and no state is carried between pairs.  That is the
only parallel axis the path has, so:

* on one GPU the frames stay resident in HBM (``_gme_native.Sequence``) and every
  kernel launch covers all pairs of the shard;
* across GPUs (one process per GPU) contiguous pair ranges are dealt to the ranks, each
  rank needs its pairs' frames plus ``fd`` halo frames, and the only exchange is one
  all-gather of the per-pair ``float64[6]`` parameter vectors (48 B per pair) at the end
  -- RCCL over xGMI through the library's own communicator (gme_comm_*, gme_shard_gather).
"""
import ctypes
import os
import stat
import time
import types

import numpy as np

import _gme_native as _native
import motion
import roadmap


def shard_range(n_pairs, rank, world):
    """Contiguous pair range [start, stop) of `rank`."""
    if not 0 <= rank < world:
        raise ValueError("rank %d outside world of %d" % (rank, world))
    return (rank * n_pairs) // world, ((rank + 1) * n_pairs) // world


def shard_frames(n_pairs, frame_distance, rank, world):
    """(first_frame, n_frames) a rank must hold: its pairs plus the `fd` halo."""
    start, stop = shard_range(n_pairs, rank, world)
    if stop == start:
        return start, 0
    return start, (stop - start) + frame_distance


# ---- the library's own RCCL communicator (gme_comm_*, include/gme_hip.h): no torch involved -------------
class CommUnavailable(RuntimeError):
    """Raised by comm_init on EVERY rank of the launch when at least one rank cannot bring the RCCL
    communicator up (no librccl, no id, ncclCommInitRank failed): the ranks can then take the same
    fallback, or all exit; none is left waiting inside a collective."""


def _process_start_time():
    """Wall-clock time this process was started (the ranks of one launch start within a second or so of
    each other; files older than that belong to an earlier launch)."""
    try:
        with open("/proc/self/stat") as f:
            ticks = int(f.read().rsplit(")", 1)[1].split()[19])          # field 22: starttime in clock ticks since boot
        with open("/proc/uptime") as f:
            up = float(f.read().split()[0])
        return time.time() - (up - ticks / os.sysconf("SC_CLK_TCK"))
    except Exception:                                                      # noqa: BLE001
        return _IMPORT_TIME


_IMPORT_TIME = time.time()
_STALE_SLACK_S = 60.0        # ranks of one launch may start (and publish) this much apart; an earlier launch's files are older


def _rendezvous_base():
    """Path prefix of this launch's rendezvous files.  GME_COMM_ID_FILE names it outright; otherwise it lives in
    a directory only this user can enter (0700, checked) and is keyed by MASTER_PORT and the pid of the ranks'
    common parent (torch.distributed.run's agent, or the test's spawner)."""
    explicit = os.environ.get("GME_COMM_ID_FILE")
    if explicit:
        return explicit
    d = os.path.join(os.environ.get("GME_COMM_DIR", "/tmp"), "gme_rccl_%d" % os.getuid())
    try:
        os.mkdir(d, 0o700)
    except FileExistsError:
        pass
    st = os.lstat(d)
    if not stat.S_ISDIR(st.st_mode) or st.st_uid != os.getuid() or (st.st_mode & 0o077):
        raise PermissionError("%s is not a private directory of uid %d (mode %o, owner %d)" % (d, os.getuid(), st.st_mode & 0o7777, st.st_uid))
    try:                                         # day-old leftovers of earlier launches (ack files, crashed attempts)
        for name in os.listdir(d):
            path = os.path.join(d, name)
            st1 = os.lstat(path)
            if stat.S_ISREG(st1.st_mode) and st1.st_uid == os.getuid() and st1.st_mtime < time.time() - 86400:
                os.unlink(path)
    except OSError:
        pass
    return os.path.join(d, "%s_%d" % (os.environ.get("MASTER_PORT", "0"), os.getppid()))


class Rendezvous:
    """File-based exchange of small blobs between the ranks of one launch on one node: publish(key, blob) writes
    <base>.<key>.<rank> atomically (0600, O_EXCL | O_NOFOLLOW); collect(key) returns every rank's blob once all are
    there.  A file is accepted only if it is a regular file of this user and not older than this process (minus a few
    minute of start-up skew): what an earlier launch with the same port and parent left behind is never read."""

    _attempts = {}               # base -> rendezvous objects this process has made for it (ranks make them collectively)

    def __init__(self, rank, world, timeout_s=180.0, base=None):
        self.rank, self.world, self.timeout_s = int(rank), int(world), float(timeout_s)
        self.base = base or _rendezvous_base()
        self.not_before = _process_start_time() - _STALE_SLACK_S
        self._mine = []
        # Attempt nonce: a second bring-up in the same processes, or a worker group restarted by the same
        # torchrun agent (same port, same parent pid), must never read the first attempt's files -- a stale "no:" marker
        # or, worse, a stale ncclUniqueId (ranks entering ncclCommInitRank with different ids hang for good).  Every
        # rank of a launch makes its rendezvous objects in the same order, so the counter agrees across ranks.
        n = Rendezvous._attempts.get(self.base, 0)
        Rendezvous._attempts[self.base] = n + 1
        self.attempt = "a%s_%d" % (os.environ.get("TORCHELASTIC_RESTART_COUNT", "0"), n)

    def _path(self, key, rank):
        return "%s.%s.%s.%d" % (self.base, self.attempt, key, rank)

    def publish(self, key, blob):
        path = self._path(key, self.rank)
        tmp = "%s.tmp%d" % (path, os.getpid())
        for stale in (tmp, path):
            try:
                os.unlink(stale)
            except FileNotFoundError:
                pass
        fd = os.open(tmp, os.O_WRONLY | os.O_CREAT | os.O_EXCL | getattr(os, "O_NOFOLLOW", 0), 0o600)
        with os.fdopen(fd, "wb") as f:
            f.write(blob)
        os.replace(tmp, path)                    # atomic: readers see nothing or everything
        self._mine.append(path)

    def _read(self, key, rank):
        try:
            fd = os.open(self._path(key, rank), os.O_RDONLY | getattr(os, "O_NOFOLLOW", 0))
        except (FileNotFoundError, OSError):
            return None
        with os.fdopen(fd, "rb") as f:
            st = os.fstat(f.fileno())
            if not stat.S_ISREG(st.st_mode) or st.st_uid != os.getuid() or st.st_mtime < self.not_before:
                return None
            return f.read()

    def collect(self, key, ranks=None):
        ranks = list(range(self.world)) if ranks is None else list(ranks)
        got, t0 = {}, time.time()
        while True:
            for r in ranks:
                if r not in got:
                    blob = self._read(key, r)
                    if blob is not None:
                        got[r] = blob
            if len(got) == len(ranks):
                return [got[r] for r in ranks]
            if time.time() - t0 > self.timeout_s:
                missing = [r for r in ranks if r not in got]
                raise TimeoutError("rank %d: no '%s' from rank(s) %s at %s.* after %.0f s" % (self.rank, key, missing, self.base, self.timeout_s))
            time.sleep(0.01)

    def agree(self, key, ok, payload=b""):
        """Every rank says ok / not ok (with a payload or a reason); returns all payloads if every rank was ok,
        raises CommUnavailable on EVERY rank otherwise."""
        self.publish(key, (b"ok:" if ok else b"no:") + payload)
        blobs = self.collect(key)
        bad = ["rank %d: %s" % (r, b[3:].decode("utf-8", "replace")) for r, b in enumerate(blobs) if not b.startswith(b"ok:")]
        if bad:
            self.fail(key, "%s failed on %d of %d ranks (%s)" % (key, len(bad), self.world, "; ".join(bad)))
        return [b[3:] for b in blobs]

    def fail(self, key, message):
        """Raise CommUnavailable(message) -- called with the same verdict on every rank.  One more round first says that
        every rank has READ every file; then each rank removes its own.  The 4-byte ack files themselves stay (a rank
        that is done may exit before the slowest rank has read its ack; the attempt nonce keeps a later bring-up away
        from them, and _rendezvous_base sweeps day-old files out of the private directory)."""
        try:
            self.publish("ack_" + key, b"read")
            self.collect("ack_" + key)
            self._mine = [p for p in self._mine if ".ack_" not in os.path.basename(p)]
            self.cleanup()
        except TimeoutError:
            pass
        raise CommUnavailable(message)

    def cleanup(self):
        """Remove this rank's own files (call only once every rank is known to have read them)."""
        for path in self._mine:
            try:
                os.unlink(path)
            except OSError:
                pass
        self._mine = []


def comm_exchange_id(make_id, rank, world, timeout_s=180.0, rdv=None):
    """Rank 0 calls make_id() -> bytes and publishes them; every rank returns the same bytes.  If rank 0 cannot
    make one it says so through the same file and the others stop waiting at once."""
    rdv = rdv or Rendezvous(rank, world, timeout_s)
    if rank == 0:
        try:
            blob = make_id()
        except Exception:
            rdv.publish("id", b"FAILED")
            raise
        rdv.publish("id", blob)
        return blob
    blob = rdv.collect("id", [0])[0]
    if blob == b"FAILED":
        raise RuntimeError("rank 0 could not create an RCCL id")
    return blob


def collective_init(rdv, probe, make_id, init, destroy, device_tag=None):
    """The agreement around ncclCommInitRank, which cannot time out: (1) every rank loads RCCL (`probe`) and rank 0
    makes the id; all ranks learn whether all could, and nobody enters the collective otherwise; (2) every rank runs
    `init(id)`; all ranks learn whether all succeeded, and those that did `destroy()` their communicator
    otherwise.  Either every rank returns, or every rank raises CommUnavailable -- PROVIDED every rank that passed
    phase 1 really enters ncclCommInitRank in `init`: a rank whose `init` fails before the collective (device lost
    between probe and init, out of memory) leaves its peers inside a call that cannot time out, and only the
    launcher's own timeout ends the launch.  Everything that can fail locally therefore belongs in `probe`
    (comm_init: gme_comm_probe loads RCCL AND binds the context's device; the payload carries the device's PCI bus id
    and phase 1 refuses two ranks on one device, which RCCL would only refuse inside the collective)."""
    blob, err, tag = b"", None, b""
    try:
        probe()
        if device_tag is not None:
            tag = device_tag()
        if rdv.rank == 0:
            blob = make_id()
    except Exception as e:                        # noqa: BLE001 -- reported to every rank below
        err = e
    payload = len(tag).to_bytes(2, "little") + tag + blob
    blobs = rdv.agree("probe", err is None, payload if err is None else repr(err).encode())
    tags = [b[2:2 + int.from_bytes(b[:2], "little")] for b in blobs]
    shared = sorted({t for t in tags if t and tags.count(t) > 1})
    if shared and not os.environ.get("GME_COMM_ALLOW_SHARED_DEVICE"):
        # every rank sees the same tags, so every rank raises -- before anybody is inside ncclCommInitRank
        rdv.fail("probe", "probe: ranks share a device (%s): RCCL wants one device per rank" % ", ".join(
            "%s on ranks %s" % (t.decode("utf-8", "replace"), [r for r, x in enumerate(tags) if x == t]) for t in shared))
    uid = blobs[0][2 + len(tags[0]):]
    err = None
    try:
        init(uid)
    except Exception as e:                        # noqa: BLE001
        err = e
    try:
        rdv.agree("init", err is None, b"" if err is None else repr(err).encode())
    except CommUnavailable:
        if err is None:
            destroy()
        raise


def comm_init(ctx, rank, world, timeout_s=180.0):
    """Collective: give `ctx` an RCCL communicator spanning the `world` ranks of this node.  Raises
    CommUnavailable on every rank if any rank cannot (see collective_init)."""
    lib = ctx.lib

    def probe():
        _native._check(lib.gme_comm_probe(), lib)

    def make_id():
        buf = ctypes.create_string_buffer(128)
        _native._check(lib.gme_comm_unique_id(buf), lib)
        return buf.raw

    def init(blob):
        _native._check(lib.gme_comm_init(ctx.handle, blob, rank, world), lib)

    def device_tag():
        buf = ctypes.create_string_buffer(64)
        _native._check(lib.gme_device_bus_id(ctx.handle, buf, 64), lib)     # also binds the device: fails HERE, not in init
        return buf.value

    if world == 1:
        probe()
        init(make_id())
        comm_barrier(ctx)
        return
    rdv = Rendezvous(rank, world, timeout_s)
    collective_init(rdv, probe, make_id, init, lambda: comm_destroy(ctx), device_tag)
    comm_barrier(ctx)                            # every rank has read every file once this returns
    rdv.cleanup()


def comm_info(ctx):
    """(rank, world) as RCCL itself reports them for the context's communicator (ncclCommUserRank / ncclCommCount)."""
    r, n = ctypes.c_int(-1), ctypes.c_int(-1)
    _native._check(ctx.lib.gme_comm_info(ctx.handle, ctypes.byref(r), ctypes.byref(n)), ctx.lib)
    return r.value, n.value


def comm_destroy(ctx):
    _native._check(ctx.lib.gme_comm_destroy(ctx.handle), ctx.lib)


def comm_max(ctx, value):
    v = np.array([float(value)], dtype=np.float64)
    _native._check(ctx.lib.gme_comm_allreduce_max(ctx.handle, v.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), 1), ctx.lib)
    return float(v[0])


def comm_barrier(ctx):
    comm_max(ctx, 0.0)


def pad_and_trim(n_pairs, world):
    """(rows of the largest shard, [(start, stop)] per rank): the fixed block size of the all-gather
    and how to cut the padding off again."""
    sizes = [shard_range(n_pairs, r, world) for r in range(world)]
    return max(1, max(b - a for a, b in sizes)), sizes


def gather_parameters_rccl(ctx, local, n_pairs, rank, world):
    """gather_parameters over the library's RCCL communicator (gme_shard_gather)."""
    local = np.ascontiguousarray(local, dtype=np.float64)
    k = local.shape[1] if local.ndim == 2 else 6
    longest, sizes = pad_and_trim(n_pairs, world)
    out = np.empty((world, longest, k), dtype=np.float64)
    dp = ctypes.POINTER(ctypes.c_double)
    _native._check(ctx.lib.gme_shard_gather(ctx.handle, local.ctypes.data_as(dp), len(local), k, longest, out.ctypes.data_as(dp)),
                   ctx.lib)
    return np.concatenate([out[r, :b - a] for r, (a, b) in enumerate(sizes)], axis=0)


def psnr_from_sse(sse, height, width, exact=True):
    """utils.PSNR (utils.py:100-116) from sums of squared error: -1 where the frames are equal,
    else the real part of the reference's complex 20 log10(255 / sqrt(mse)).

    ``exact`` evaluates it per pair with cmath like the reference (results.py writes
    ``str(value)`` into psnr_records.json, so the last bit shows); the vectorised NumPy form
    differs from it by at most 2e-14 dB and is what the batch hot path uses."""
    mse = np.asarray(sse, dtype=np.float64) / (height * width)
    out = np.full(len(mse), -1.0)
    if exact:
        from cmath import log10, sqrt
        for k, m in enumerate(mse):
            if m != 0:
                out[k] = (20 * log10(255.0 / sqrt(m))).real
        return out
    nz = mse != 0
    out[nz] = 20.0 * np.log10(255.0 / np.sqrt(mse[nz]))
    return out


def lane_ranges(n_local_pairs, streams):
    """The local pair ranges [lo, hi) of a shard's lanes: ``streams`` contiguous pieces, at most one per pair, at least one."""
    k = max(1, min(int(streams), n_local_pairs))
    return [shard_range(n_local_pairs, j, k) for j in range(k)]


def stabilized_owners(n_frames, rank, world, streams=1):
    """The global frames [a, b) whose stabilized form each lane of ``rank`` reads out (ShardedSequence.read_stabilized):
    lane j owns the frames of its pairs, [lo, hi); the last lane of the last rank also owns frame N-1.  Frame distance 1."""
    n_pairs = max(0, int(n_frames) - 1)
    start, stop = shard_range(n_pairs, rank, world)
    if stop == start:
        return []
    out = [(start + lo, start + hi) for lo, hi in lane_ranges(stop - start, streams)]
    if rank == world - 1:
        out[-1] = (out[-1][0], out[-1][1] + 1)
    return out


class _Lane:
    """One stream's part of a shard: its own context (HIP stream) and resident frames."""

    def __init__(self, ctx, seq, lo, hi):
        self.ctx, self.seq, self.lo, self.hi = ctx, seq, lo, hi    # local pair range [lo, hi)


class ShardedSequence:
    """This rank's slice of a video: frames in HBM, pair-level results on demand.

    ``streams`` > 1 cuts the slice once more into that many contiguous pair ranges, each with
    its own context (= HIP stream) on the same GPU and driven by its own host thread.  The
    staged estimate (roadmap.stages) has the host solve 3x3 systems between device
    stages; with several streams one range's solves and launch latencies are covered by the
    other ranges' kernels.  Results do not depend on ``streams``.

    ``interleave=True`` drives the ranges from ONE host thread instead, through the split-phase calls
    of the C ABI (gme_seq_set_split_phase / gme_seq_wait): stage s of every range is queued, then each
    range's result is awaited and solved in turn while the other ranges' kernels run.  No host threads
    contend for the interpreter or the BLAS; estimate() and estimate_and_compensate() use it.
    """

    def __init__(self, height, width, n_frames, frame_distance=1, rank=0, world=1, ctx=None, streams=1, interleave=False):
        self.ctx = ctx or _native.default_context()
        self.interleave = bool(interleave)
        self.H, self.W, self.fd = int(height), int(width), int(frame_distance)
        self.n_frames_total = int(n_frames)
        self.n_pairs_total = max(0, self.n_frames_total - self.fd)
        self.rank, self.world = rank, world
        self.pair_start, self.pair_stop = shard_range(self.n_pairs_total, rank, world)
        self.first_frame, n_local = shard_frames(self.n_pairs_total, self.fd, rank, world)
        self.lanes = []
        n_loc = self.pair_stop - self.pair_start
        ranges = lane_ranges(n_loc, streams)
        k = len(ranges)
        for j, (lo, hi) in enumerate(ranges if n_local else []):
            c = self.ctx if j == 0 else _native.Context(self.ctx.device)
            n_fr = (hi - lo) + self.fd if k > 1 else max(n_local, self.fd + 1)
            self.lanes.append(_Lane(c, _native.Sequence(c, n_fr, self.H, self.W), lo, hi))
        self.seq = self.lanes[0].seq if len(self.lanes) == 1 else None     # single-stream shards: the sequence itself
        self._pool = None
        self._stabilized = None       # the frames of the last stabilize(neighbours >= 1), which keeps nothing on the device

    @property
    def n_pairs(self):
        return self.pair_stop - self.pair_start

    def _each(self, fn):
        """fn(lane) for every lane, one host thread per lane; results in lane order."""
        if len(self.lanes) <= 1:
            return [fn(lane) for lane in self.lanes]
        if self._pool is None:
            from concurrent.futures import ThreadPoolExecutor
            self._pool = ThreadPoolExecutor(len(self.lanes))
        return list(self._pool.map(fn, self.lanes))

    def _lane_of(self, pair):
        for lane in self.lanes:
            if lane.lo <= pair < lane.hi:
                return lane, pair - lane.lo
        raise IndexError("pair %d is not in this shard" % pair)

    def close(self):
        if self._pool is not None:
            self._pool.shutdown()
            self._pool = None
        for lane in self.lanes:
            lane.seq.close()
            if lane.ctx is not self.ctx:
                lane.ctx.close()
        self.lanes, self.seq = [], None

    def sync(self):
        for lane in self.lanes:
            lane.ctx.sync()

    def invalidate(self):
        """Mark everything derived from the frames stale (new video in the same buffers)."""
        for lane in self.lanes:
            lane.seq.invalidate_pyramids()

    def load(self, frames):
        """`frames` is the WHOLE video (uint8[N, H, W] or a list); only this rank's slice is uploaded:
        one copy per lane (its frames back to back), the lanes' copies in their own host threads so that
        one lane's upload runs beside another lane's kernels."""
        def run(lane):
            g0 = self.first_frame + lane.lo
            n = max(0, min(lane.seq.N, len(frames) - g0))
            if n == 0:
                return
            if isinstance(frames, np.ndarray) and frames.ndim == 3 and frames.dtype == np.uint8:
                lane.seq.upload(0, frames[g0:g0 + n])
            else:
                lane.seq.upload(0, np.stack([np.asarray(f, dtype=np.uint8) for f in frames[g0:g0 + n]]))
        self._each(run)

    def synth(self, seed, t0=0):
        """Generate this rank's slice of the synthetic sequence `seed` (video frame k = time t0 + k) on its own GPU."""
        for lane in self.lanes:
            lane.seq.synth(seed, t0 + self.first_frame + lane.lo)

    def motion_fields(self, block_size, search_window, procedure, pnorm):
        """bbme.get_motion_field for every local pair -> int32[P_local, h, w, 2]."""
        if not self.lanes:
            return np.zeros((0, int(self.H / block_size), int(self.W / block_size), 2), np.int32)

        def run(lane):
            lane.seq.bbme(self.fd, block_size, search_window, procedure, pnorm)
            return lane.seq.read_mv(0, lane.hi - lane.lo)
        return np.concatenate(self._each(run), axis=0)

    def motion_fields_subpel(self, block_size, search_window, procedure, pnorm, levels=2, compensate=False):
        """motion_fields refined to half (levels 1) or quarter pixels (2) on the device (subpel.py) for
        every local pair -> (qfield int32[P_local, h, w, 2] in quarter pixels, cost int64[P_local, h, w]) and, with
        ``compensate``, sse int64[P_local] of the quarter-pel compensation against the current frames (the frames: lane
        sequences' read_compensated_range)."""
        levels = _native._subpel_levels(levels)
        h, w = int(self.H / block_size), int(self.W / block_size)
        if not self.lanes:
            empty = (np.zeros((0, h, w, 2), np.int32), np.zeros((0, h, w), np.int64))
            return empty + (np.zeros(0, np.int64),) if compensate else empty

        def run(lane):
            n = lane.hi - lane.lo
            lane.seq.bbme(self.fd, block_size, search_window, procedure, pnorm)
            lane.seq.subpel(self.fd, block_size, pnorm, levels)
            q, cost = lane.seq.read_qmv(0, n)
            return (q, cost, lane.seq.compensate_qpel(self.fd, block_size)[:n]) if compensate else (q, cost)
        return tuple(np.concatenate(part, axis=0) for part in zip(*self._each(run)))

    def motion_fields_hier(self, block_size, coarse_window, radius, pnorm, frame_distance, levels=3):
        """hier.search for every local pair -> (field int32[P_local, h, w, 2] in full-resolution pixels,
        cost int64[P_local, h, w]).  ``frame_distance`` is the one the sequence was sharded for.  Each lane's level-2 field
        stays its sequence's motion field, so the quarter-pel calls of the lane sequences refine it."""
        block_size, coarse_window, radius, pnorm, levels = _native._hier_args(block_size, coarse_window, radius, pnorm, levels)
        if int(frame_distance) != self.fd:
            raise ValueError("frame_distance %d, but the sequence is sharded for %d" % (int(frame_distance), self.fd))
        if not self.lanes:
            h, w = self.H // block_size, self.W // block_size
            return np.zeros((0, h, w, 2), np.int32), np.zeros((0, h, w), np.int64)

        def run(lane):
            lane.seq.hier(self.fd, block_size, coarse_window, radius, pnorm, levels)
            return lane.seq.read_hier(2, 0, lane.hi - lane.lo)
        return tuple(np.concatenate(part, axis=0) for part in zip(*self._each(run)))

    def motion_fields_vbs(self, block_size, search_window, procedure, pnorm, depth=2, radius=1, penalty=None, hier=False,
                          compensate=False):
        """The search, then vbs.tree on its field for every local pair, per lane -> (leaf
        int32[P_local, h << depth, w << depth, 2], depth uint8[P_local, h << depth, w << depth], cost int64[P_local, h, w]) and,
        with ``compensate``, sse int64[P_local] of the leaf-field compensation against the current frames.  The search is
        bbme(block_size, search_window, procedure, pnorm) or, with ``hier``, the hierarchical one at three levels with
        search_window as its coarse window and radius 1.  ``penalty`` None: vbs.default_penalty."""
        import vbs
        penalty = vbs.default_penalty(block_size, pnorm) if penalty is None else penalty
        block_size, depth, radius, pnorm, penalty = _native._vbs_args(block_size, depth, radius, pnorm, penalty)
        h, w = self.H // block_size, self.W // block_size
        if not self.lanes:
            empty = (np.zeros((0, h << depth, w << depth, 2), np.int32), np.zeros((0, h << depth, w << depth), np.uint8),
                     np.zeros((0, h, w), np.int64))
            return empty + (np.zeros(0, np.int64),) if compensate else empty

        def run(lane):
            n = lane.hi - lane.lo
            if hier:
                lane.seq.hier(self.fd, block_size, search_window, 1, pnorm, 3)
            else:
                lane.seq.bbme(self.fd, block_size, search_window, procedure, pnorm)
            lane.seq.vbs(self.fd, block_size, depth, radius, pnorm, penalty)
            out = lane.seq.read_vbs(0, n)
            return out + (lane.seq.compensate_vbs(self.fd, block_size)[:n],) if compensate else out
        return tuple(np.concatenate(part, axis=0) for part in zip(*self._each(run)))

    def motion_fields_prop(self, block_size, search_window, procedure, pnorm, rounds=2, steps=1, temporal=True, g=None, hier=False):
        """The search, then propagate.search on its field for every local pair, per lane -> (field
        int32[P_local, h, w, 2], cost int64[P_local, h, w], source uint8[P_local, h, w]).  The search is bbme(block_size,
        search_window, procedure, pnorm) or, with ``hier``, the hierarchical one at three levels with search_window as its coarse
        window and radius 1.  ``g`` is the camera field int32[P_local, h, w, 2] or None.  With ``temporal`` a pair also scores
        the prior field of the pair before it -- where that pair lies in the same lane: the first pair of every shard and of every
        lane has no temporal prior, so a sharded run equals the single-sequence one only with ``temporal`` off.  Each lane's
        propagated field becomes its sequence's motion field."""
        block_size, pnorm, rounds, steps = _native._prop_args(block_size, pnorm, rounds, steps)
        h, w = self.H // block_size, self.W // block_size
        if g is not None:
            g = _native._prop_field(g, "g", (self.lanes[-1].hi if self.lanes else 0, h, w))
        if not self.lanes:
            return np.zeros((0, h, w, 2), np.int32), np.zeros((0, h, w), np.int64), np.zeros((0, h, w), np.uint8)

        def run(lane):
            n = lane.hi - lane.lo
            if hier:
                lane.seq.hier(self.fd, block_size, search_window, 1, pnorm, 3)
            else:
                lane.seq.bbme(self.fd, block_size, search_window, procedure, pnorm)
            own = None
            if g is not None:                   # the lane's sequence may hold more pairs than the lane covers
                own = np.zeros((lane.seq.N - self.fd, h, w, 2), np.int32)
                own[:n] = g[lane.lo:lane.hi]
            lane.seq.prop(self.fd, block_size, pnorm, rounds, steps, temporal, own)
            return lane.seq.read_prop(0, n)
        return tuple(np.concatenate(part, axis=0) for part in zip(*self._each(run)))

    def estimate(self, procedure=3, search_window=2, model=None):
        """motion.global_motion_estimation for every local pair -> float64[P_local, 6].  ``model``: one of roadmap.MODELS
        (roadmap.stages per lane); the second-order models return float64[P_local, 12]."""
        model, _, width = roadmap.normalize_model(model)
        if not self.lanes:
            return np.zeros((0, width))
        return self._join(self._stages(procedure, search_window, model, False))[0]

    def _psnr(self, sse, exact=True):
        return psnr_from_sse(sse, self.H, self.W, exact)

    def compensate(self, params):
        """results.py:52-59,109 for every local pair -> PSNR(current, compensated) as float64[P_local]."""
        if not self.lanes:
            return np.zeros(0)
        params = np.asarray(params, dtype=np.float64)
        sse = self._each(lambda lane: lane.seq.compensate(self.fd, int(motion.BBME_BLOCK_SIZE),
                                                          params[lane.lo:lane.hi])[:lane.hi - lane.lo])
        return self._psnr(np.concatenate(sse))

    def estimate_and_compensate(self, procedure=3, search_window=2, exact_psnr=False, model=None):
        """estimate() then compensate() per stream without a join in between -> (params[P,6], psnr[P]).

        ``model``: one of roadmap.MODELS (None or "affine": the reference's path).  The others run the staged calls of their
        order with roadmap.solve_model / roadmap.project; the second-order models return params[P, 12].

        Under GME_DEVICE_SOLVE=1 the affine and second-order models try the device solve first (_device_solved)."""
        model, order, width = roadmap.normalize_model(model)
        if not self.lanes:
            return np.zeros((0, width)), np.zeros(0)
        if os.environ.get("GME_DEVICE_SOLVE") == "1" and (model == "affine" or order == 2):
            got = self._device_solved(procedure, search_window, exact_psnr, model=model)
            if got is not None:
                return got
        return self._join(self._stages(procedure, search_window, model, True), exact_psnr)

    def _device_solved(self, procedure, search_window, exact_psnr=False, model="affine"):
        """estimate_and_compensate() with the solves on the device (roadmap.device_stages, round robin): one call and one
        wait per lane -> (params, psnr), or None when the library flags a pair (near a rounding tie, singular or
        ill-conditioned) and the caller must run the host path.  Both orders keep one contract (gme_seq_gme_device_solve and
        gme_seq_gme_device_solve2 in the header): each parameter within 1e-10 max(1, S) of the host path's, scaled by its
        term's largest factor over the field; model fields, masks, compensated frames and PSNR bit-equal to it."""
        parts = self._round_robin(lambda lane: roadmap.device_stages(lane.seq, self.fd, model, procedure, search_window))
        if any(np.any(f[:lane.hi - lane.lo]) for lane, (_, _, f) in zip(self.lanes, parts)):
            return None
        return self._join(parts, exact_psnr)

    def _stages(self, procedure, search_window, model, compensate):
        """roadmap.stages on every lane -> [(params, sse or None)] in lane order: driven round robin from one host thread
        (``interleave`` and several lanes), else with blocking calls, one host thread per lane."""
        if self.interleave and len(self.lanes) > 1:
            return self._round_robin(lambda lane: roadmap.stages(lane.seq, self.fd, model, procedure, search_window, compensate))
        return self._each(lambda lane: roadmap.estimate_blocking(lane.seq, self.fd, model, procedure, search_window, compensate))

    def _round_robin(self, chain):
        """``chain(lane)`` (roadmap.stages) of every lane driven from ONE host thread through the split-phase calls
        (gme_seq_set_split_phase / gme_seq_wait) -> what each chain returns, in lane order.  Stage s is queued on every lane
        before the first wait; each lane in turn is then awaited, solved and its stage s + 1 queued, so one lane's host
        solves run while the other lanes' kernels do."""
        lanes = self.lanes
        for lane in lanes:
            lane.seq.set_split_phase(True)
        try:
            chains = [chain(lane) for lane in lanes]
            for c in chains:
                next(c)
            out, left = [None] * len(lanes), list(range(len(lanes)))
            while left:
                for k in list(left):
                    lanes[k].seq.wait()
                    try:
                        next(chains[k])                   # the lane's solve, and its next stage queued
                    except StopIteration as done:
                        out[k] = done.value
                        left.remove(k)
                        lanes[k].ctx.sync()       # drains the stream and reports a walk that overran its guard
        finally:
            for lane in lanes:
                lane.seq.set_split_phase(False)   # the other methods of the class use the blocking calls
        return out

    def _join(self, parts, exact_psnr=False):
        """Per-lane (params, sse or None, ...) -> (params[P_local, k], psnr[P_local] or None)."""
        n = [lane.hi - lane.lo for lane in self.lanes]
        params = np.concatenate([part[0][:m] for part, m in zip(parts, n)], axis=0)
        if parts[0][1] is None:
            return params, None
        return params, self._psnr(np.concatenate([part[1][:m] for part, m in zip(parts, n)]), exact_psnr)

    def estimate_projective(self, procedure=3, search_window=2, outlier_fraction=0.1, max_iters=10, exact_psnr=False):
        """Direct projective refinement of every local pair from its indirect affine estimate, and the
        dense compensation under the result -> (h float64[P_local, 8], flags int32[P_local], psnr float64[P_local]).  One
        host thread per lane; the rows gather like any other (gather, k = 8)."""
        if not self.lanes:
            return np.zeros((0, 8)), np.zeros(0, np.int32), np.zeros(0)

        def run(lane):
            n = lane.hi - lane.lo
            h, flags = roadmap.refine_sequence(lane.seq, self.fd, None, outlier_fraction, max_iters, procedure, search_window)
            return h[:n], flags[:n], lane.seq.compensate_projective(self.fd, h)[:n]
        parts = self._each(run)
        return (np.concatenate([h for h, _, _ in parts], axis=0), np.concatenate([f for _, f, _ in parts]),
                self._psnr(np.concatenate([e for _, _, e in parts]), exact_psnr))

    def read_compensated(self, pair):
        lane, k = self._lane_of(pair)
        return lane.seq.read_compensated(k)

    def _pair_warps(self, estimator, procedure, search_window, outlier_fraction, max_iters):
        """This shard's pair warps (frame distance 1) as projective parameters -> (h float64[P_local, 8], flags
        int32[P_local]), each lane estimating its own pairs: "projective" the direct refinement, "affine" the indirect
        estimate written as a projective warp.  The first half of stabilize() and mosaic()."""
        bs = int(motion.BBME_BLOCK_SIZE)

        def estimate(lane):
            n = lane.hi - lane.lo
            if estimator == "affine":
                h = roadmap.affine_to_projective(motion.estimate_sequence(lane.seq, 1, procedure, search_window), bs)
                return h[:n], np.zeros(n, np.int32)
            h, flags = roadmap.refine_sequence(lane.seq, 1, None, outlier_fraction, max_iters, procedure, search_window)
            return h[:n], flags[:n]
        parts = self._each(estimate)
        h_loc = np.concatenate([h for h, _ in parts], axis=0) if parts else np.zeros((0, 8))
        f_loc = np.concatenate([f for _, f in parts]) if parts else np.zeros(0, np.int32)
        return h_loc, f_loc

    # ---- video stabilization (stabilize.py, gme_stab.hip)
    def stabilize(self, estimator="projective", radius=15, sigma=None, crop="auto", max_crop=0.25, border="constant", fill=0,
                  procedure=3, search_window=2, outlier_fraction=0.1, max_iters=10, neighbours=0):
        """Stabilize the whole video from its estimated camera path -> result dict (stabilize.stabilize).  Each lane estimates
        its pairs; the pair warps are all-gathered (gather, k = 8), so every rank and lane computes the same path, crop and
        corrections in host float64; each lane then warps all of its resident frames lo .. hi (the frame shared at a lane
        boundary twice, identically) and the consecutive-frame squared errors of its pairs.  read_stabilized reads the
        frames.  Results do not depend on ``streams``.  With ``neighbours`` K >= 1 the border of frame t is filled from frames
        t-1, t+1, .. t-K, t+K (stabilize.fill_candidates, gme_seq_warp_fill), which reads frames across lane boundaries: one
        rank, one lane; the call returns the frames and read_stabilized serves them from host memory."""
        import stabilize as stab
        neighbours = int(neighbours)
        if neighbours and (self.world > 1 or len(self.lanes) > 1):
            raise ValueError("stabilize with neighbours needs the whole video in one sequence: world %d, streams %d (a border is "
                             "filled from frames of other shards; use world = 1 and streams = 1)" % (self.world, len(self.lanes)))
        if self.fd != 1:
            raise ValueError("stabilize needs frame_distance 1 (this sequence has %d)" % self.fd)
        if estimator not in stab.ESTIMATORS:
            raise ValueError("estimator %r (choose from %r)" % (estimator, stab.ESTIMATORS))
        bid = stab.border_id(border)
        if not 0 <= int(fill) <= 255:
            raise ValueError("fill %d outside 0 .. 255" % fill)
        h_loc, f_loc = self._pair_warps(estimator, procedure, search_window, outlier_fraction, max_iters)
        h = self.gather(h_loc)
        out = stab.plan(h, self.H, self.W, radius, sigma, crop, max_crop, neighbours)
        Wt = out["W"]
        self._stabilized = None
        if neighbours:
            n = self.n_pairs_total
            self._stabilized, _, valid, filled, sse = self.seq.warp_fill(0, out["sources"], out["fill_warps"], bid, int(fill))
            out.update(h=h, pair_flags=f_loc, estimator=estimator, valid=valid, filled=filled,
                       unfilled=self.H * self.W - valid - filled, itf_before=stab.itf(self.seq.frame_sse(0, 0, n), self.H, self.W),
                       itf_after=stab.itf(sse, self.H, self.W))
            return out

        def warp(lane):
            n = lane.hi - lane.lo
            g0 = self.first_frame + lane.lo
            valid = lane.seq.warp_frames(0, Wt[g0:g0 + n + 1], bid, int(fill))
            return np.stack([lane.seq.frame_sse(0, 0, n).astype(np.float64), lane.seq.frame_sse(1, 0, n).astype(np.float64),
                             valid[:n].astype(np.float64), valid[1:n + 1].astype(np.float64)], axis=1)
        rows = self._each(warp)
        local = np.concatenate(rows, axis=0) if rows else np.zeros((0, 4))
        rows = self.gather(np.concatenate([f_loc.astype(np.float64)[:, None], local], axis=1).reshape(-1, 5))
        out.update(h=h, pair_flags=rows[:, 0].astype(np.int32), estimator=estimator,
                   valid=np.concatenate([rows[:, 3], rows[-1:, 4]]).astype(np.int64),
                   itf_before=stab.itf(rows[:, 1].astype(np.int64), self.H, self.W),
                   itf_after=stab.itf(rows[:, 2].astype(np.int64), self.H, self.W))
        return out

    def _owner(self, frame):
        owners = stabilized_owners(self.n_frames_total, self.rank, self.world, len(self.lanes))
        for lane, (a, b) in zip(self.lanes, owners):
            if a <= frame < b:
                return lane, frame - self.first_frame - lane.lo, b - frame
        raise IndexError("frame %d is not read out by this rank" % frame)

    def read_stabilized(self, frame):
        """Stabilized frame ``frame`` (global index) from the lane that owns it (stabilized_owners) -> uint8[H, W]."""
        if self._stabilized is not None:
            return self._stabilized[frame].copy()
        lane, k, _ = self._owner(frame)
        return lane.seq.read_warped_range(k, 1)[0]

    def read_stabilized_range(self, first, count):
        """Stabilized frames first .. first+count-1, all owned by this rank -> uint8[count, H, W]."""
        if self._stabilized is not None:
            if not 0 <= first <= first + count <= len(self._stabilized):
                raise IndexError("frames [%d, %d) outside [0, %d)" % (first, first + count, len(self._stabilized)))
            return self._stabilized[first:first + count].copy()
        out = np.empty((int(count), self.H, self.W), np.uint8)
        k = 0
        while k < count:
            lane, j, left = self._owner(first + k)
            n = min(count - k, left)
            out[k:k + n] = lane.seq.read_warped_range(j, n)
            k += n
        return out

    # ---- background mosaic and moving-object masks (mosaic.py, gme_mosaic.hip)
    def mosaic(self, estimator="projective", anchor=0, threshold=16, min_count=3, fill=0, masks=True, max_canvas_pixels=None,
               h=None, cull=True, procedure=3, search_window=2, outlier_fraction=0.1, max_iters=10):
        """The background sprite of the whole video on the canvas of its camera path and, with ``masks``, the moving-object
        mask of every frame -> result dict (mosaic.mosaic); read_mosaic and read_masks_range read them.  The pair warps are
        estimated as stabilize() does, or taken from ``h`` (float64[P, 8]) where the path is known.  One rank, one lane: a
        median does not combine across shards of frames."""
        import mosaic as mos
        import stabilize as stab
        if self.world > 1 or len(self.lanes) > 1:
            raise ValueError("mosaic needs the whole video in one sequence: world %d, streams %d (a median does not combine "
                             "across shards of frames; use world = 1 and streams = 1)" % (self.world, len(self.lanes)))
        if self.fd != 1:
            raise ValueError("mosaic needs frame_distance 1 (this sequence has %d)" % self.fd)
        if estimator not in stab.ESTIMATORS:
            raise ValueError("estimator %r (choose from %r)" % (estimator, stab.ESTIMATORS))
        if not 0 <= int(fill) <= 255:
            raise ValueError("fill %d outside 0 .. 255" % fill)
        if not 0 <= int(threshold) <= 255:
            raise ValueError("threshold %d outside 0 .. 255" % threshold)
        if int(min_count) < 1:
            raise ValueError("min_count %d < 1" % min_count)
        if h is None:
            h, pair_flags = self._pair_warps(estimator, procedure, search_window, outlier_fraction, max_iters)
        else:
            h = np.asarray(h, dtype=np.float64).reshape(self.n_pairs_total, 8)
            pair_flags, estimator = np.zeros(len(h), np.int32), "given"
        out = mos.plan(h, self.H, self.W, anchor, max_canvas_pixels)
        usable = out["flags"] == 0
        self.seq.mosaic(0, out["G"], usable, out["ox"], out["oy"], out["Hc"], out["Wc"], int(fill), cull)
        out.update(h=h, pair_flags=pair_flags, estimator=estimator, threshold=int(threshold), min_count=int(min_count))
        if masks:
            out["known"], out["moving"] = self.seq.moving_masks(0, out["A"], usable, out["ox"], out["oy"], int(threshold),
                                                                int(min_count))
        return out

    def read_mosaic(self):
        """(sprite uint8[Hc, Wc], count uint16[Hc, Wc]) of the last mosaic()."""
        return self.seq.read_mosaic()

    def read_masks_range(self, first, count):
        """Moving-object masks (0 / 1) of frames first .. first+count-1 -> uint8[count, H, W]."""
        return self.seq.read_masks_range(first, count)

    def gather(self, local_rows):
        """All-gather of this shard's per-pair rows (float64[P_local, k]) -> float64[P_total, k] on every rank, over the
        context's RCCL communicator (comm_init first); the identity on a single rank."""
        if self.world == 1:
            return np.ascontiguousarray(local_rows, dtype=np.float64)
        return gather_parameters_rccl(self.ctx, local_rows, self.n_pairs_total, self.rank, self.world)

    def unpad(self, gathered):
        """float64[world, n_max, k] blocks of a fixed-size all-gather -> float64[P_total, k]."""
        _, sizes = pad_and_trim(self.n_pairs_total, self.world)
        return np.concatenate([gathered[r, :b - a] for r, (a, b) in enumerate(sizes)], axis=0)


class StreamEstimator:
    """results.py:41-59,109 for videos that still live in HOST memory: ``run(frames)`` -> (params float64[P, 6], psnr float64[P]).

    A video is cut into chunks of at most ``chunk_pairs`` pairs (plus the ``fd`` halo frames; see schedule()); ``streams`` lanes -- each its own
    context, HIP stream and (chunk_pairs + fd)-frame device sequence, allocated once here and reused by every run() --
    take the chunks in turn.  Everything a lane does is split-phase (gme_seq_set_split_phase): the upload of its chunk
    (on the device's shared upload stream), pyramids + dense field, level fits, compensation are queued and ONE host
    thread serves whichever lane has its result (gme_seq_poll), doing its projection / 3x3 solves (motion.py:191-207,
    262-282) and queueing its next stage.  While one lane's frames cross the link the other lanes' kernels run, so a
    video larger than HBM streams through at link speed.

    ``frames``: uint8[N, H, W] (page-locked memory from _gme_native.pinned_empty crosses at link speed and never holds
    the host thread) or a list of 2-D uint8 arrays (gathered chunk by chunk into a page-locked buffer per lane).
    ``compensated``: optional uint8[P, H, W] array that receives every compensated frame (results.py:59 writes them out).
    Results equal the resident path bit for bit (tests/test_gpu_round3.py)."""

    def __init__(self, height, width, frame_distance=1, chunk_pairs=512, streams=2, ctx=None, procedure=3, search_window=2,
                 min_chunk=64):
        self.H, self.W, self.fd = int(height), int(width), int(frame_distance)
        self.chunk_pairs = max(1, int(chunk_pairs))
        self.min_chunk = max(1, min(int(min_chunk), self.chunk_pairs))
        self.cap = self.chunk_pairs + self.fd                    # frames a lane holds
        self.procedure, self.search_window = procedure, search_window
        self.ctx = ctx or _native.default_context()
        self.lanes = []
        try:
            for j in range(max(1, int(streams))):
                c = self.ctx if j == 0 else _native.Context(self.ctx.device)
                seq = _native.Sequence(c, self.cap, self.H, self.W)
                seq.set_split_phase(True)
                self.lanes.append(types.SimpleNamespace(ctx=c, seq=seq, host=None, comp_host=None, chain=None, steps=0))
        except BaseException:
            self.close(check=False)
            raise

    def close(self, check=True):
        """Release the lanes' device objects; with ``check`` a walk that overran its guard is reported (gme_sync)."""
        lanes, self.lanes = self.lanes, []
        err = None
        for lane in lanes:
            try:
                lane.seq.set_split_phase(False)
                if check:
                    lane.ctx.sync()
            except Exception as e:                                   # noqa: BLE001 -- release everything, then report
                err = err or e
            finally:
                lane.seq.close()
                if lane.ctx is not self.ctx:
                    lane.ctx.close()
        if err is not None and check:
            raise err

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close(check=exc[0] is None)

    def schedule(self, n_pairs):
        """Chunks [(first pair, end pair)] of a video of `n_pairs` pairs: as large as a lane holds while much is left (each
        chunk costs the host three round trips whatever its size), shrinking towards the end -- a quarter of what is left per
        lane, at least `min_chunk` -- because the estimate of the LAST chunk is the one stretch no upload hides (traced:
        with equal chunks of 1024 pairs the link idles 2.5 of 15.9 ms behind the last copy, with equal chunks of 128 the
        host's round trips leave gaps between the copies)."""
        out, p0 = [], 0
        while p0 < n_pairs:
            left = n_pairs - p0
            c = min(self.chunk_pairs, max(self.min_chunk, -(-left // (2 * max(1, len(self.lanes))))), left)
            out.append((p0, p0 + c))
            p0 += c
        return out

    def run(self, frames, compensated=None, exact_psnr=True, on_chunk=None, model=None):
        """``on_chunk(p0, p1, comp, params, psnr)`` is called as each chunk finishes (chunks of different lanes may finish out
        of order) with its compensated frames uint8[p1 - p0, H, W] (one read for the chunk; the array is reused by the next
        chunk of the same lane), parameters and PSNR: what results.py writes per pair, without a whole-video array on the host.

        ``model``: one of roadmap.MODELS (None: the reference's affine path, as without the argument).  The second-order
        models (roadmap.SECOND_ORDER) run the order-2 stages and return params float64[P, 12]."""
        fd, H, W, cap = self.fd, self.H, self.W, self.cap
        P = max(0, len(frames) - fd)
        model, _, width = roadmap.normalize_model(model)
        params_out, sse_out = np.zeros((P, width)), np.zeros(P, dtype=np.int64)
        if P == 0:
            return params_out, np.zeros(0)
        if tuple(np.asarray(frames[0]).shape) != (H, W):
            raise ValueError("frames of %r do not fit this estimator's %r" % (np.asarray(frames[0]).shape, (H, W)))
        chunks = self.schedule(P)
        stacked = isinstance(frames, np.ndarray) and frames.ndim == 3 and frames.dtype == np.uint8 and frames.flags.c_contiguous

        def chunk(lane, p0, p1):
            """One chunk on one lane, a stage chain like roadmap.stages: the upload, the staged estimate, the results."""
            n = p1 - p0 + fd
            if stacked:
                src = frames[p0:p0 + n]
            else:
                if lane.host is None:
                    lane.host = _native.pinned_empty((cap, H, W))
                for k in range(n):
                    lane.host[k] = frames[p0 + k]
                src = lane.host[:n]
            lane.seq.set_frames(n)               # the stages cover this chunk's pairs only; buffers stay sized for `cap`
            lane.seq.upload(0, src)              # queued; `src` stays alive (lane.host / the caller's array)
            # Nothing else is queued on the lane yet: a kernel launch behind a cross-stream wait on a copy holds the calling
            # thread until that copy is done (measured: one gme_begin_fit call of 7.6 ms, the upload of two chunks), and the
            # one host thread must stay free for the other lanes.  The stages follow once the upload's event has arrived.
            yield
            params, sse = yield from roadmap.stages(lane.seq, fd, model, self.procedure, self.search_window, compensate=True)
            params_out[p0:p1] = params
            sse_out[p0:p1] = sse
            if compensated is not None:
                lane.seq.read_compensated_range(0, p1 - p0, compensated[p0:p1])      # one wait for the chunk, not one per pair
            if on_chunk is not None:
                if compensated is not None:
                    comp = compensated[p0:p1]
                else:
                    if lane.comp_host is None:
                        lane.comp_host = np.empty((cap, H, W), np.uint8)
                    comp = lane.seq.read_compensated_range(0, p1 - p0, lane.comp_host[:p1 - p0])
                on_chunk(p0, p1, comp, params, psnr_from_sse(sse, H, W, exact_psnr))

        def start(lane, p0_p1):
            lane.chain, lane.steps = chunk(lane, *p0_p1), 1
            next(lane.chain)

        todo = list(reversed(chunks))
        busy = []
        for lane in self.lanes:
            if todo:
                start(lane, todo.pop())
                busy.append(lane)
        while busy:
            # serve whichever lane has its result: a lane that waits for its frames must not hold up one whose sums are
            # back; the lanes furthest along go first, so that their next chunk's upload is queued as early as possible
            progressed = False
            for lane in sorted(busy, key=lambda l: -l.steps):
                if lane.seq.poll():
                    progressed = True
                    lane.seq.wait()
                    try:
                        next(lane.chain)         # the lane's solve, and its next stage queued
                        lane.steps += 1
                    except StopIteration:        # the chunk is finished
                        if todo:
                            start(lane, todo.pop())
                        else:
                            busy.remove(lane)
            if not progressed:
                time.sleep(2e-5)                 # nothing ready: look again shortly (blocking on ONE lane's event would sit out
                                                 # another lane's result: traced, a lane idled 3.5 ms behind its finished upload)
        for lane in self.lanes:
            lane.ctx.sync()                      # drains the lane and reports a walk that overran its guard
        return params_out, psnr_from_sse(sse_out, H, W, exact_psnr)


def estimate_stream(frames, frame_distance=1, chunk_pairs=512, streams=2, ctx=None, compensated=None, procedure=3, on_chunk=None,
                    search_window=2, exact_psnr=True, min_chunk=64, model=None):
    """One-shot StreamEstimator: allocate the lanes, run `frames` through them, release them
    -> (params float64[P, 6], psnr float64[P]); params float64[P, 12] for a second-order ``model`` (StreamEstimator.run).
    Setting the lanes up costs a few milliseconds each; callers with several videos of one size keep a StreamEstimator."""
    n_frames = len(frames)
    P = max(0, n_frames - int(frame_distance))
    if P == 0:
        return np.zeros((0, roadmap.normalize_model(model)[2])), np.zeros(0)
    H, W = np.asarray(frames[0]).shape
    chunk_pairs = max(1, min(int(chunk_pairs), P))
    n_chunks = (P + chunk_pairs - 1) // chunk_pairs
    with StreamEstimator(H, W, frame_distance, chunk_pairs, max(1, min(int(streams), n_chunks)), ctx, procedure, search_window,
                         min_chunk=min_chunk) as est:
        return est.run(frames, compensated=compensated, exact_psnr=exact_psnr, on_chunk=on_chunk, model=model)
