"""The host definition of the vector propagation search (propagate.py): argument rules, monotone costs, the Jacobi wavefront,
camera and temporal candidates, the refinement, ties, hostile vectors, camera_field, the source coverage of the noise cases and
the ABI.  No GPU."""
import os

import numpy as np
import pytest

import direct
import gmc_cases
import prop_cases as pc
import propagate
from vbs import _cost

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_check_args():
    assert propagate.check_args(16, 0, 2, 1) == (16, 0, 2, 1)
    assert propagate.check_args(4, 1, 1, 0) == (4, 1, 1, 0)
    assert propagate.check_args(64, 1, 4, 4) == (64, 1, 4, 4)
    for bad in ((3, 0, 1, 0), (65, 0, 1, 0), (0, 0, 1, 0), (16, 2, 1, 0), (16, -1, 1, 0), (16, 0, 0, 0), (16, 0, 5, 0), (16, 0, 1, -1),
                (16, 0, 1, 5)):
        with pytest.raises(ValueError):
            propagate.check_args(*bad)
    z = np.zeros((16, 32), np.uint8)
    f = np.zeros((1, 2, 2), np.int32)
    with pytest.raises(ValueError):
        propagate.search(z, z, f, 16, 2, 1, 0)
    for name in ("f", "t", "g"):
        fields = dict(f=f, t=None, g=None)
        fields[name] = np.zeros((2, 2, 2), np.int32)
        with pytest.raises(ValueError):
            propagate.search(z, z, fields["f"], 16, 0, 1, 0, fields["t"], fields["g"])
    with pytest.raises(TypeError):
        propagate.search(z, z.astype(np.int16), f, 16, 0, 1, 0)
    assert 64 * 64 * 255 * 255 < 1 << 31                          # the largest sum
    # a field with more than two components per block is taken by its first two
    wide = np.concatenate([f, np.full((1, 2, 1), 7, np.int32)], axis=2)
    for a, b in zip(propagate.search(z, z, wide, 16, 0, 1, 0), propagate.search(z, z, f, 16, 0, 1, 0)):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("pnorm", (0, 1))
def test_monotone_costs(pnorm):
    """Own is a candidate: the cost of round r is at most that of round r - 1 per block; the final cost is at most the cost at
    the zero vector and at most the cost at f where f is available."""
    case = pc.NOISE[3]
    (H, W), bs = case
    previous, current, f, t, g = pc.noise_pair(case)
    zero = propagate.prior_cost(previous, current, np.zeros_like(f), bs, pnorm)
    own = propagate.prior_cost(previous, current, f, bs, pnorm)
    assert np.all(zero >= 0) and np.any(own < 0) and np.any(own >= 0)
    for steps in (0, 1):
        last = None
        for rounds in (1, 2, 3, 4):
            mf, cost, source = pc.noise_result(case, pnorm, rounds, steps, True, True) if (rounds, steps) in pc.ROUNDS_STEPS else \
                propagate.search(previous, current, f, bs, pnorm, rounds, steps, t, g)
            assert mf.dtype == np.int32 and cost.dtype == np.int64 and source.dtype == np.uint8
            assert np.all(cost >= 0) and np.all(cost <= zero) and np.all(cost[own >= 0] <= own[own >= 0])
            assert np.array_equal(cost, propagate.prior_cost(previous, current, mf, bs, pnorm))      # the cost is the vector's
            if last is not None:
                assert np.all(cost <= last)
            last = cost


@pytest.mark.parametrize("pnorm", (0, 1))
def test_wavefront(pnorm):
    """A zero prior with one block that carries the pan's vector, no refinement: after r rounds the blocks that carry it are
    exactly those reached in r steps of the 8-neighbourhood through blocks where it is available.  An in-place update would run
    ahead of the front."""
    ok = pc.available_mask(pc.PAN_SHAPE, pc.PAN_BLOCK, pc.PAN_MOVE)
    assert ok[pc.PAN_START] and not ok.all()
    sizes = []
    for rounds in (1, 2, 3, 4):
        mf, cost, source = pc.wavefront_result(pnorm, rounds)
        carries = np.all(mf == pc.PAN_MOVE, axis=-1)
        want = pc.reached(ok, pc.PAN_START, rounds)
        assert np.array_equal(carries, want), (rounds, carries, want)
        assert np.all(mf[~carries] == 0)
        assert not np.any(source & propagate.MOVED)
        sizes.append(int(carries.sum()))
    assert sizes[0] < sizes[1] < sizes[2] == int(ok.sum()), sizes  # the front needs three rounds to cover the grid


@pytest.mark.parametrize("pnorm", (0, 1))
@pytest.mark.parametrize("which, cls", (("g", propagate.CAMERA), ("t", propagate.TEMPORAL)))
def test_inherited_field(pnorm, which, cls):
    """A zero prior and the pan's vector everywhere in the camera (temporal) field, one round, no refinement: every block where
    the vector is available takes it with source 3 (2), the others keep zero with source 0."""
    ok = pc.available_mask(pc.PAN_SHAPE, pc.PAN_BLOCK, pc.PAN_MOVE)
    mf, cost, source = pc.inherit_result(pnorm, which)
    assert np.all(mf[ok] == pc.PAN_MOVE) and np.all(source[ok] == cls)
    assert np.all(mf[~ok] == 0) and np.all(source[~ok] == propagate.OWN)


@pytest.mark.parametrize("pnorm", (0, 1))
@pytest.mark.parametrize("off", pc.REFINE_OFFSETS)
def test_refinement(pnorm, off):
    """A prior one pixel off the pan everywhere, one round: with one step every block where both vectors are available ends at
    the pan's vector with source OWN | MOVED; with no step none moves."""
    previous, current = pc.pan_scene()
    v = (pc.PAN_MOVE[0] + off[0], pc.PAN_MOVE[1] + off[1])
    both = pc.available_mask(pc.PAN_SHAPE, pc.PAN_BLOCK, pc.PAN_MOVE) & pc.available_mask(pc.PAN_SHAPE, pc.PAN_BLOCK, v)
    assert both.any()
    mf, cost, source = propagate.search(previous, current, pc.constant_field(v), pc.PAN_BLOCK, pnorm, 1, 1)
    assert np.all(mf[both] == pc.PAN_MOVE) and np.all(source[both] == (propagate.OWN | propagate.MOVED)), (mf, source)
    mf, cost, source = propagate.search(previous, current, pc.constant_field(v), pc.PAN_BLOCK, pnorm, 1, 0)
    assert not np.any(source & propagate.MOVED) and np.all(mf[both] == v)


@pytest.mark.parametrize("pnorm", (0, 1))
def test_ties(pnorm):
    """Constant frames: every block keeps its own vector with source 0 and no MOVED; a block whose own vector is unavailable
    takes its first available candidate in list order."""
    previous, current = pc.ties_frames()
    for bs in (8, 16):
        f, t, g = pc.ties_fields(bs)
        own = pc.available_mask(previous.shape, bs, (0, 0)) & False
        for i in range(f.shape[0]):
            for j in range(f.shape[1]):
                own[i, j] = propagate.available(37, 53, i * bs, j * bs, bs, int(f[i, j, 0]), int(f[i, j, 1]))
        assert not own[0, 0] and own.any()
        mf, cost, source = propagate.search(previous, current, f, bs, pnorm, 1, 2, t, g)
        assert np.all(mf[own] == f[own]) and np.all(source[own] == propagate.OWN)
        assert not np.any(source & propagate.MOVED)
        assert np.all(cost == bs * bs * (7 if pnorm == 0 else 49))
        # block (0, 0): its own vector points outside, it has no upper or left neighbour; the first candidate is its right neighbour
        assert tuple(mf[0, 0]) == (1, 2) and source[0, 0] == propagate.SPATIAL
        # without any available neighbour, temporal or camera vector, zero is what is left
        lone = np.full_like(f, -40)
        mf, cost, source = propagate.search(previous, current, lone, bs, pnorm, 1, 0, lone, lone)
        assert np.all(mf == 0) and np.all(source == propagate.ZERO)
        # ... and temporal comes before camera
        mf, cost, source = propagate.search(previous, current, lone, bs, pnorm, 1, 0, np.ones_like(f), np.ones_like(f) * 2)
        inner = pc.available_mask(previous.shape, bs, (1, 1))
        assert np.all(mf[inner] == 1) and np.all(source[inner] == propagate.TEMPORAL)
        mf, cost, source = propagate.search(previous, current, lone, bs, pnorm, 1, 0, None, np.ones_like(f) * 2)
        inner = pc.available_mask(previous.shape, bs, (2, 2))
        assert np.all(mf[inner] == 2) and np.all(source[inner] == propagate.CAMERA)


def test_hostile_input():
    """Vectors of +-2^30 in f, t and g are unavailable and no error."""
    case = pc.NOISE[0]
    (H, W), bs = case
    previous, current, f, t, g = pc.noise_pair(case)
    big = 1 << 30
    hostile = []
    for k, a in enumerate((f, t, g)):
        a = a.copy()
        a[0, 0] = (big, -big)
        a[1, k] = (-big, 3)
        a[2, 2 + k] = (2, big)
        hostile.append(a)
    assert not propagate.available(H, W, 0, 0, bs, big, 0) and not propagate.available(H, W, 0, 0, bs, 0, -big)
    assert not propagate.available(1 << 20, 1 << 20, 0, 0, bs, (1 << 14) + 1, 0)            # the magnitude alone
    assert propagate.available(1 << 20, 1 << 20, 0, 0, bs, 1 << 14, 1 << 14)
    for pnorm in (0, 1):
        mf, cost, source = propagate.search(previous, current, hostile[0], bs, pnorm, 2, 1, hostile[1], hostile[2])
        assert np.all(np.abs(mf) <= pc.FIELD_REACH + 2 * 1 + 1) and np.all(cost >= 0)
        assert np.array_equal(cost, propagate.prior_cost(previous, current, mf, bs, pnorm))
    assert propagate.prior_cost(previous, current, hostile[0], bs, 0)[0, 0] == -1


def test_camera_field():
    H, W, bs = 70, 101, 16
    assert np.all(propagate.camera_field(direct.IDENTITY, H, W, bs) == 0)
    # a pixel of `current` samples `previous` at (u - 3, v + 2): the content of `previous` lies at (+3, -2) in `current`
    h = gmc_cases.warp_of("integer", H, W)
    g = propagate.camera_field(h, H, W, bs)
    assert g.dtype == np.int32 and g.shape == (H // bs, W // bs, 2)
    assert np.all(g == (-int(h[2]), -int(h[5]))) and np.all(g == (3, -2))
    for bs2 in (4, 12, 64):
        assert np.all(propagate.camera_field(h, H, W, bs2) == (3, -2))
    for name in ("unusable", "nan"):
        assert propagate.camera_field(gmc_cases.warp_of(name, H, W), H, W, bs) is None
    singular = np.array([1.0, 1.0, 0.0, 1.0, 1.0, 0.0, 0.0, 0.0])
    assert propagate.camera_field(singular, H, W, bs) is None
    far = np.array([1.0, 0.0, -float(1 << 15), 0.0, 1.0, 0.0, 0.0, 0.0])                      # a component beyond 2^14
    assert propagate.camera_field(far, H, W, bs) is None
    # half-pixel translations round half up, as floor(x + 0.5) does
    half = np.array([1.0, 0.0, -2.5, 0.0, 1.0, 2.5, 0.0, 0.0])
    assert np.all(propagate.camera_field(half, H, W, bs) == (3, -2))
    # `current` samples `previous` 1.3 times as far from the centre: a centre c of `previous` lands at c / 1.3 (no value below
    # lies within 0.04 of a rounding tie)
    z = gmc_cases.rotation_zoom(H, W, 0.0, 1.0 / 1.3)
    g = propagate.camera_field(z, H, W, bs)
    cx = (np.arange(W // bs) * bs + (bs - 1) / 2.0) - (W - 1) / 2.0
    want = np.floor((1.0 / 1.3 - 1.0) * cx + 0.5)
    assert np.array_equal(g[0, :, 0], want.astype(np.int32)), (g[0, :, 0], want)


def test_summary():
    f = np.zeros((2, 2, 2), np.int32)
    mf = f.copy()
    mf[0, 1] = (1, 0)
    source = np.array([[0, 1 | 8], [3, 4]], np.uint8)
    s = propagate.summary(f, np.array([[10, 20], [-1, 30]]), mf, np.array([[10, 5], [7, 30]]), source, 400, 100, 4, 4)
    assert s["changed_share"] == 0.25 and s["moved_share"] == 0.25
    assert s["source_share"] == {"own": 0.25, "spatial": 0.25, "temporal": 0.0, "camera": 0.25, "zero": 0.25}
    assert s["mean_cost_prior"] == 20.0 and s["mean_cost_prop"] == 13.0
    assert s["psnr_prop"] > s["psnr_prior"] > 0


@pytest.mark.parametrize("case", pc.NOISE)
def test_noise_sources(case):
    """The noise cases of the GPU test hold every class and the MOVED flag (prop_cases.SEED), and candidates that are not
    available."""
    (H, W), bs = case
    previous, current, f, t, g = pc.noise_pair(case)
    res = [pc.noise_result(case, pnorm, r, s, True, True) for pnorm in (0, 1) for r, s in pc.ROUNDS_STEPS]
    assert pc.sources_seen(res) == pc.ALL_SOURCES, pc.sources_seen(res)
    assert any(np.any(propagate.prior_cost(previous, current, a, bs, 0) < 0) for a in (f, t, g))
    # one block restated apart from propagate._block: the candidates by hand, first strict minimum
    mf, cost, source = propagate.search(previous, current, f, bs, 0, 1, 0, t, g)
    i, j = f.shape[0] - 1, f.shape[1] - 1
    cands = [(0, f[i, j])] + [(1, f[i + di, j + dj]) for di, dj in ((-1, -1), (-1, 0), (0, -1)) if i + di >= 0 and j + dj >= 0]
    cands += [(2, t[i, j]), (3, g[i, j]), (4, (0, 0))]
    best = None
    for cls, v in cands:
        vx, vy = int(v[0]), int(v[1])
        if abs(vx) > 1 << 14 or abs(vy) > 1 << 14 or j * bs + vx < 0 or i * bs + vy < 0 or j * bs + vx + bs > W or i * bs + vy + bs > H:
            continue
        c = _cost(previous, current, i * bs, j * bs, bs, vx, vy, 0)
        if best is None or c < best[0]:
            best = (c, vx, vy, cls)
    assert (int(cost[i, j]), int(mf[i, j, 0]), int(mf[i, j, 1]), int(source[i, j])) == best


def test_abi_declares_the_prop_entries():
    import _gme_native
    lib = _gme_native.load_library()
    header = open(os.path.join(REPO, "include", "gme_hip.h")).read()
    for name in ("gme_prop_u8", "gme_seq_prop", "gme_seq_read_prop"):
        assert name in _gme_native.exported_symbols() and hasattr(lib, name) and name + "(" in header
