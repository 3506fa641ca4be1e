"""CPU-side checks of the second-order device solve (k_solve_model2, gme_solve_model2_sums, gme_seq_gme_device_solve2): the
compiler's resources of the new kernel, the C ABI's model ids, and ShardedSequence's model argument."""
import os
import re
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_solve_kernel_neither_spills_nor_uses_scratch():
    """The 8 x 9 augmented system with runtime pivot rows is the textbook case of a private array the compiler puts in
    scratch; the kernel keeps it in LDS."""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import resource_table
    rows = [r for r in resource_table.kernels() if r["name"] == "k_solve_model2"]
    assert rows, "no resource remarks for k_solve_model2 (make -C global-motion-estimation_amd/csrc)"
    for r in rows:
        assert r["vgpr_spill"] == 0 and r["scratch"] == 0, r


def test_header_declares_the_model_solve_and_the_model_ids():
    import _gme_native
    import roadmap
    header = open(os.path.join(REPO, "include", "gme_hip.h")).read()
    declared = set(re.findall(r"GME_API [^;(]*?\b(gme_\w+)\s*\(", header))
    assert {"gme_solve_model2_sums", "gme_seq_gme_device_solve2"} <= declared
    lib = _gme_native.load_library()
    assert hasattr(lib, "gme_solve_model2_sums") and hasattr(lib, "gme_seq_gme_device_solve2")
    ids = {m.group(1): int(m.group(2)) for m in re.finditer(r"\bGME_MODEL_(\w+)\s*=\s*(\d+)", header)}
    assert ids == {m.upper(): roadmap.MODELS.index(m) for m in roadmap.SECOND_ORDER}
    assert _gme_native.MODEL_IDS == {m: roadmap.MODELS.index(m) for m in roadmap.SECOND_ORDER}
    assert _gme_native.model_id("quadratic") == 5 and _gme_native.model_id(2) == 2      # ints go to the library's check
    with pytest.raises(ValueError):
        _gme_native.model_id("affine")                                                   # no order-2 device solve for it


class _NoDevice:
    """Stands in for a context: a shard without pairs never creates a sequence, so nothing may call into it."""

    def __getattr__(self, name):
        raise AssertionError("the device was touched (%s)" % name)


def test_sharded_sequence_checks_the_model_before_the_device():
    import roadmap
    import sequence
    shard = sequence.ShardedSequence(240, 320, 1, ctx=_NoDevice())        # one frame: no pair, no lane
    assert shard.lanes == []
    for call in (shard.estimate_and_compensate, shard.estimate):
        with pytest.raises(ValueError, match="unknown motion model"):
            call(model="projective")
    for model in roadmap.MODELS:
        width = 12 if model in roadmap.SECOND_ORDER else 6
        params, psnr = shard.estimate_and_compensate(model=model)
        assert params.shape == (0, width) and psnr.shape == (0,)
        assert shard.estimate(model=model).shape == (0, width)
    assert shard.estimate_and_compensate()[0].shape == (0, 6) and shard.estimate().shape == (0, 6)
