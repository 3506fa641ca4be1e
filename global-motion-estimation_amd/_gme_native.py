"""ctypes binding of libgme_hip.so (include/gme_hip.h) -- the only way the Python
surface reaches the GPU.  No PyTorch, no fallback: if the library or a gfx950 device
is missing every call raises.

Build the library with ``python -c "import __graft_entry__ as g; g.build()"`` or
``make -C global-motion-estimation_amd/csrc``.
"""
import ctypes
import os
import threading
import weakref

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libgme_hip.so")

GME_OK, ERR_ARG, ERR_GEOMETRY, ERR_HIP, ERR_STATE, ERR_NOMEM = 0, -1, -3, -4, -5, -6
# GME_MODEL_* of include/gme_hip.h: the second-order models by their index in roadmap.MODELS
MODEL_IDS = {"bilinear": 3, "pseudo_perspective": 4, "quadratic": 5}


def model_id(model):
    """A second-order model name (roadmap.SECOND_ORDER) -> its GME_MODEL_* id; an int passes through (the library checks it)."""
    if isinstance(model, str):
        if model not in MODEL_IDS:
            raise ValueError("no device solve for motion model %r (choose from %r)" % (model, tuple(MODEL_IDS)))
        return MODEL_IDS[model]
    return int(model)


class GmeError(RuntimeError):
    """HIP/runtime failure inside libgme_hip.so."""


_c_u8p = ctypes.POINTER(ctypes.c_uint8)
_c_i16p = ctypes.POINTER(ctypes.c_int16)
_c_u16p = ctypes.POINTER(ctypes.c_uint16)
_c_i32p = ctypes.POINTER(ctypes.c_int32)
_c_i64p = ctypes.POINTER(ctypes.c_int64)
_c_f32p = ctypes.POINTER(ctypes.c_float)
_c_f64p = ctypes.POINTER(ctypes.c_double)
_vp = ctypes.c_void_p
_i = ctypes.c_int

_SIGNATURES = {
    "gme_last_error": (ctypes.c_char_p, []),
    "gme_device_count": (_i, []),
    "gme_create": (_vp, [_i]),
    "gme_destroy": (None, [_vp]),
    "gme_sync": (_i, [_vp]),
    "gme_stream": (_vp, [_vp]),
    "gme_device_info": (_i, [_vp, ctypes.c_char_p, _i, ctypes.POINTER(_i), ctypes.POINTER(_i)]),
    "gme_device_bus_id": (_i, [_vp, ctypes.c_char_p, _i]),
    "gme_last_bbme_info": (_i, [_vp, ctypes.c_char_p, _i, _c_i64p, _c_i64p, _c_i64p]),
    "gme_last_bbme_listed": (_i, [_vp, _c_i64p]),
    "gme_timer_start": (_i, [_vp]),
    "gme_timer_stop": (_i, [_vp, _c_f32p]),
    "gme_bbme_u8": (_i, [_vp, _c_u8p, _c_u8p, _i, _i, _i, _i, _i, _i, _i, _c_i32p]),
    "gme_pyrdown_u8": (_i, [_vp, _c_u8p, _i, _i, _i, _c_u8p]),
    "gme_affine_field": (_i, [_vp, _c_f64p, _i, _i, _c_i16p]),
    "gme_compensate_u8": (_i, [_vp, _c_u8p, _i, _i, _i, _c_i32p, _i, _i, _c_u8p]),
    "gme_sse_u8": (_i, [_vp, _c_u8p, _c_u8p, _i, _i, _i, _i, _c_i64p]),
    "gme_seq_create": (_vp, [_vp, _i, _i, _i]),
    "gme_seq_destroy": (None, [_vp]),
    "gme_seq_upload": (_i, [_vp, _i, _i, _c_u8p, _i, ctypes.c_int64]),
    "gme_seq_set_frames": (_i, [_vp, _i]),
    "gme_seq_synth": (_i, [_vp, ctypes.c_uint64, _i]),
    "gme_seq_read_frame": (_i, [_vp, _i, _i, _c_u8p]),
    "gme_seq_invalidate": (_i, [_vp]),
    "gme_seq_bbme": (_i, [_vp, _i, _i, _i, _i, _i]),
    "gme_seq_read_mv": (_i, [_vp, _i, _i, _c_i32p]),
    "gme_seq_bbme_streamed": (_i, [_vp, _c_u8p, _i, ctypes.c_int64, _i, _i, _i, _i, _i, _i, _i, _c_i32p]),
    "gme_host_alloc": (_vp, [ctypes.c_size_t]),
    "gme_host_free": (None, [_vp]),
    "gme_comm_probe": (_i, []),
    "gme_comm_info": (_i, [_vp, ctypes.POINTER(_i), ctypes.POINTER(_i)]),
    "gme_seq_mv_summary": (_i, [_vp, _c_f64p]),
    "gme_seq_mv_summary_gather": (_i, [_vp, _i, _c_f64p]),
    "gme_comm_unique_id": (_i, [ctypes.c_char_p]),
    "gme_comm_init": (_i, [_vp, ctypes.c_char_p, _i, _i]),
    "gme_comm_destroy": (_i, [_vp]),
    "gme_shard_gather": (_i, [_vp, _c_f64p, _i, _i, _i, _c_f64p]),
    "gme_comm_allreduce_max": (_i, [_vp, _c_f64p, _i]),
    "gme_seq_gme_begin": (_i, [_vp, _i, _i, _i, _i, _c_f32p]),
    "gme_seq_gme_fit": (_i, [_vp, _i, _c_f64p, ctypes.c_double, _c_f64p]),
    "gme_seq_gme_begin_fit": (_i, [_vp, _i, _i, _i, _i, ctypes.c_double, _c_f32p, _c_f64p]),
    "gme_seq_gme_read_stage": (_i, [_vp, _i, _i, _c_i32p, _c_i16p, _c_u8p, _c_i64p]),
    "gme_seq_compensate": (_i, [_vp, _i, _i, _c_f64p, _c_i64p]),
    "gme_model2_field": (_i, [_vp, _c_f64p, _i, _i, _c_i16p]),
    "gme_seq_gme_begin_fit2": (_i, [_vp, _i, _i, _i, _i, ctypes.c_double, _c_f32p, _c_f64p]),
    "gme_seq_gme_fit2": (_i, [_vp, _i, _c_f64p, ctypes.c_double, _c_f64p]),
    "gme_seq_compensate2": (_i, [_vp, _i, _i, _c_f64p, _c_i64p]),
    "gme_solve_fit_sums": (_i, [_vp, _c_f64p, _i, _i, _i, _i, _c_f64p, _c_i32p]),
    "gme_seq_gme_device_solve": (_i, [_vp, _i, _i, _i, _i, ctypes.c_double, _c_f64p, _c_i64p, _c_i32p]),
    "gme_solve_model2_sums": (_i, [_vp, _i, _c_f64p, _i, _i, _i, _i, _c_f64p, _c_i32p]),
    "gme_seq_gme_device_solve2": (_i, [_vp, _i, _i, _i, _i, _i, ctypes.c_double, _c_f64p, _c_i64p, _c_i32p]),
    "gme_seq_direct_eval": (_i, [_vp, _i, _i, _c_f64p, ctypes.c_double, _c_f64p, _c_i64p, _c_f64p, _c_f64p]),
    "gme_seq_refine_projective": (_i, [_vp, _i, _c_f64p, ctypes.c_double, _i, _c_f64p, _c_i32p]),
    "gme_seq_compensate_projective": (_i, [_vp, _i, _c_f64p, _c_i64p]),
    "gme_seq_read_compensated": (_i, [_vp, _i, _c_u8p]),
    "gme_seq_read_compensated_range": (_i, [_vp, _i, _i, _c_u8p]),
    "gme_seq_warp_frames": (_i, [_vp, _i, _i, _c_f64p, _i, _i, _c_i64p]),
    "gme_seq_read_warped_range": (_i, [_vp, _i, _i, _c_u8p]),
    "gme_seq_frame_sse": (_i, [_vp, _i, _i, _i, _c_i64p]),
    "gme_seq_warp_fill": (_i, [_vp, _i, _i, _i, _c_i32p, _c_f64p, _i, _i, _c_u8p, _c_u8p, _c_i64p, _c_i64p, _c_i64p]),
    "gme_seq_mosaic": (_i, [_vp, _i, _i, _c_f64p, _c_u8p, _i, _i, _i, _i, _i, _i]),
    "gme_seq_read_mosaic": (_i, [_vp, _c_u8p, _c_u16p]),
    "gme_seq_moving_masks": (_i, [_vp, _i, _i, _c_f64p, _c_u8p, _i, _i, _i, _i, _c_i64p, _c_i64p]),
    "gme_seq_read_masks_range": (_i, [_vp, _i, _i, _c_u8p]),
    "gme_subpel_u8": (_i, [_vp, _c_u8p, _c_u8p, _i, _i, _i, _i, _i, _i, _c_i32p, _c_i32p, _c_i64p]),
    "gme_seq_subpel": (_i, [_vp, _i, _i, _i, _i]),
    "gme_seq_read_qmv": (_i, [_vp, _i, _i, _c_i32p, _c_i64p]),
    "gme_seq_compensate_qpel": (_i, [_vp, _i, _i, _c_i64p]),
    "gme_hier_u8": (_i, [_vp, _c_u8p, _c_u8p, _i, _i, _i, _i, _i, _i, _i, _i, _c_i32p, _c_i64p]),
    "gme_seq_hier": (_i, [_vp, _i, _i, _i, _i, _i, _i]),
    "gme_seq_read_hier": (_i, [_vp, _i, _i, _i, _c_i32p, _c_i64p]),
    "gme_vbs_u8": (_i, [_vp, _c_u8p, _c_u8p, _i, _i, _i, _i, _i, _i, _i, _i, _c_i32p, _c_i32p, _c_u8p, _c_i64p]),
    "gme_seq_vbs": (_i, [_vp, _i, _i, _i, _i, _i, _i]),
    "gme_seq_read_vbs": (_i, [_vp, _i, _i, _c_i32p, _c_u8p, _c_i64p]),
    "gme_seq_compensate_vbs": (_i, [_vp, _i, _i, _c_i64p]),
    "gme_bipred_u8": (_i, [_vp, _c_u8p, _c_u8p, _c_u8p, _i, _i, _i, _i, _i, _i, _i, _i, _c_i32p, _c_i32p, _c_u8p, _c_i32p, _c_i32p, _c_i64p,
                           _c_i64p, _c_u8p, _c_i64p]),
    "gme_seq_bipred": (_i, [_vp, _i, _i, _i, _i, _i, _i, _i, _i]),
    "gme_seq_read_bipred": (_i, [_vp, _i, _i, _c_i32p, _c_i32p, _c_u8p, _c_i32p, _c_i32p, _c_i64p, _c_i64p]),
    "gme_seq_predict_bipred": (_i, [_vp, _c_i64p]),
    "gme_gmc_u8": (_i, [_vp, _c_u8p, _c_u8p, _i, _i, _i, _i, _i, _i, _c_f64p, _c_i32p, _c_u8p, _c_i64p, _c_i64p, _c_u8p, _c_i64p]),
    "gme_seq_gmc": (_i, [_vp, _i, _i, _i, _i, _i, _i, _c_f64p]),
    "gme_seq_read_gmc": (_i, [_vp, _i, _i, _c_i32p, _c_u8p, _c_i64p, _c_i64p, _c_u8p]),
    "gme_seq_predict_gmc": (_i, [_vp, _c_i64p]),
    "gme_prop_u8": (_i, [_vp, _c_u8p, _c_u8p, _i, _i, _i, _i, _i, _i, _i, _c_i32p, _c_i32p, _c_i32p, _c_i32p, _c_i64p, _c_u8p]),
    "gme_seq_prop": (_i, [_vp, _i, _i, _i, _i, _i, _i, _c_i32p]),
    "gme_seq_read_prop": (_i, [_vp, _i, _i, _c_i32p, _c_i64p, _c_u8p]),
    "gme_interp_u8": (_i, [_vp, _c_u8p, _c_u8p, _c_u8p, _i, _i, _i, _i, _i, _i, _i, _c_i32p, _c_i64p, _c_i64p, _c_u8p, _c_i64p]),
    "gme_seq_interp": (_i, [_vp, _i, _i, _i, _i, _i, _i, _i, _c_i32p, _c_i64p, _c_i64p, _c_u8p, _c_i64p]),
    "gme_retime_u8": (_i, [_vp, _c_u8p, _c_u8p, _c_u8p, _i, _i, _i, _i, _i, _i, _i, _i, _i, _c_i32p, _c_i64p, _c_i64p, _c_u8p, _c_i64p]),
    "gme_retime_clip_u8": (_i, [_vp, _c_u8p, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _c_u8p, _c_i32p, _c_i64p, _c_i64p]),
    "gme_obmc_u8": (_i, [_vp, _c_u8p, _c_u8p, _i, _i, _i, _i, _c_i32p, _i, _c_u8p, _c_i64p]),
    "gme_seq_obmc": (_i, [_vp, _i, _i, _i, _i, _i, _c_u8p, _c_i64p]),
    "gme_denoise_u8": (_i, [_vp, _c_u8p, ctypes.POINTER(_c_u8p), ctypes.POINTER(_c_i32p), _i, _i, _i, _i, _i, _i, _i, _c_u8p, _c_u8p,
                            _c_i64p]),
    "gme_seq_denoise": (_i, [_vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _c_u8p, _c_i64p]),
    "gme_seq_set_split_phase": (_i, [_vp, _i]),
    "gme_seq_wait": (_i, [_vp]),
    "gme_seq_poll": (_i, [_vp]),
}

_lib = None
_lib_lock = threading.Lock()


def exported_symbols():
    """Names include/gme_hip.h declares (used by the CPU-side symbol test)."""
    return sorted(_SIGNATURES)


def load_library():
    """dlopen libgme_hip.so and attach signatures; never touches a device."""
    global _lib
    with _lib_lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise GmeError(
                "libgme_hip.so is not built (%s). Build it with `make -C %s`; this package has no "
                "CPU fallback." % (LIB_PATH, os.path.join(_HERE, "csrc")))
        # multi-process use (one rank per GPU, RCCL over xGMI): the host driver of this pool only supports dmabuf IPC, and
        # the runtime reads the switch when the first HIP call initialises it -- i.e. after this point.  A value the
        # launcher exported wins.
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        lib = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _lib = lib
        return lib


def _raise(rc, lib):
    msg = (lib.gme_last_error() or b"").decode("utf-8", "replace")
    if rc == ERR_ARG:
        raise IndexError(msg)            # bbme.py:27,60 raise IndexError on bad table indices
    if rc == ERR_GEOMETRY:
        raise AssertionError(msg)        # bbme.py:59
    if rc == ERR_NOMEM:
        raise MemoryError(msg)
    raise GmeError("libgme_hip: %s (code %d)" % (msg, rc))


def _check(rc, lib):
    if rc != GME_OK:
        _raise(rc, lib)


def as_frame(a, name="frame"):
    """2-D C-contiguous uint8 view/copy of `a` (the reference feeds grayscale uint8, utils.py:26-28)."""
    a = np.asarray(a)
    if a.ndim != 2:
        raise ValueError("%s must be a 2-D grayscale image, got shape %r" % (name, a.shape))
    if a.dtype != np.uint8:
        raise TypeError("%s must be uint8 (got %s): the device kernels are integer-exact on 8-bit luma" % (name, a.dtype))
    if a.strides[1] != 1 or a.strides[0] < a.shape[1]:
        a = np.ascontiguousarray(a)
    return a


def _p(a, t):
    return a.ctypes.data_as(t)


def _block_size(bs):
    """The reference divides the frame shape by the block size first (bbme.py:23-25, motion.py:303):
    a zero block size is a ZeroDivisionError there, before anything else is looked at."""
    bs = int(bs)
    if bs == 0:
        raise ZeroDivisionError("division by zero")
    return bs


class _Pinned:
    """Owner of one gme_host_alloc block; frees it when the last array view goes away."""

    def __init__(self, lib, nbytes):
        self.lib, self.ptr = lib, lib.gme_host_alloc(nbytes)
        if not self.ptr:
            raise MemoryError((lib.gme_last_error() or b"").decode())

    def __del__(self):
        try:
            if self.ptr:
                self.lib.gme_host_free(self.ptr)
                self.ptr = None
        except Exception:
            pass


def pinned_empty(shape, dtype=np.uint8):
    """np.empty in page-locked host memory (gme_host_alloc): frame loaders that decode into it let
    uploads run at link speed and overlap the kernels (Sequence.bbme_streamed, ShardedSequence.load)."""
    lib = load_library()
    dtype = np.dtype(dtype)
    n = int(np.prod(shape)) * dtype.itemsize
    owner = _Pinned(lib, max(n, 1))
    buf = (ctypes.c_uint8 * max(n, 1)).from_address(owner.ptr)
    buf._gme_owner = owner                     # the array's .base chain keeps `buf`, which keeps the block
    return np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)


class Context:
    """One device + one HIP stream (gme_ctx)."""

    def __init__(self, device=None):
        self.lib = load_library()
        if device is None:
            device = int(os.environ.get("GME_DEVICE", os.environ.get("LOCAL_RANK", "0")))
            n = self.lib.gme_device_count()
            if n > 0:
                device %= n
        self.device = device
        self._sequences = weakref.WeakSet()
        self.handle = self.lib.gme_create(device)
        if not self.handle:
            raise GmeError("cannot open HIP device %d: %s" % (device, self.lib.gme_last_error().decode()))

    def close(self):
        if getattr(self, "handle", None):
            for seq in list(self._sequences):      # sequences hold device memory of this context
                seq.close()
            self.lib.gme_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- misc
    def sync(self):
        _check(self.lib.gme_sync(self.handle), self.lib)

    def info(self):
        name = ctypes.create_string_buffer(128)
        cu, clk = _i(0), _i(0)
        _check(self.lib.gme_device_info(self.handle, name, 128, ctypes.byref(cu), ctypes.byref(clk)), self.lib)
        return {"name": name.value.decode(), "cu_count": cu.value, "clock_khz": clk.value}

    def last_bbme_info(self):
        """{'plan': kernel / tile shape / schedule of the last block-matching call,
        'patches': candidate patches its elimination bound saw, 'surviving': those scored exactly,
        'listed': those each block's first upper bound left (what a single evaluation round would have scored),
        'redo_tiles': tiles handed to the brute-force redo kernel}."""
        plan = ctypes.create_string_buffer(192)
        n, k, r, l = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
        _check(self.lib.gme_last_bbme_info(self.handle, plan, 192, ctypes.byref(n), ctypes.byref(k), ctypes.byref(r)), self.lib)
        _check(self.lib.gme_last_bbme_listed(self.handle, ctypes.byref(l)), self.lib)
        return {"plan": plan.value.decode(), "patches": n.value, "surviving": k.value, "listed": l.value, "redo_tiles": r.value}

    def solve_fit_sums(self, sums, h, w, project=False):
        """gme_solve_fit_sums: float64[P, 15] normal-equation sums -> (params float64[P, 6], flags int32[P])."""
        sums = np.ascontiguousarray(np.asarray(sums, dtype=np.float64).reshape(-1, 15))
        params = np.empty((len(sums), 6), np.float64)
        flags = np.empty(len(sums), np.int32)
        _check(self.lib.gme_solve_fit_sums(self.handle, _p(sums, _c_f64p), len(sums), int(bool(project)), int(h), int(w),
                                           _p(params, _c_f64p), _p(flags, _c_i32p)), self.lib)
        return params, flags

    def solve_model2_sums(self, sums, model, h, w, project=False):
        """gme_solve_model2_sums: float64[P, 27] order-2 sums of a second-order `model` (name or GME_MODEL_* id)
        -> (params float64[P, 12], flags int32[P]); the tie check runs on the h x w field."""
        sums = np.ascontiguousarray(np.asarray(sums, dtype=np.float64).reshape(-1, 27))
        params = np.empty((len(sums), 12), np.float64)
        flags = np.empty(len(sums), np.int32)
        _check(self.lib.gme_solve_model2_sums(self.handle, model_id(model), _p(sums, _c_f64p), len(sums), int(bool(project)), int(h),
                                              int(w), _p(params, _c_f64p), _p(flags, _c_i32p)), self.lib)
        return params, flags

    def timer_start(self):
        _check(self.lib.gme_timer_start(self.handle), self.lib)

    def timer_stop(self):
        ms = ctypes.c_float(0)
        _check(self.lib.gme_timer_stop(self.handle, ctypes.byref(ms)), self.lib)
        return ms.value

    # ---- single-pair calls
    def bbme(self, prev, cur, block_size, search_window, procedure, pnorm):
        prev, cur = as_frame(prev, "previous"), as_frame(cur, "current")
        if prev.shape != cur.shape:
            raise AssertionError("previous and current differ in shape (bbme.py:59)")
        H, W = prev.shape
        block_size = _block_size(block_size)
        if cur.strides[0] != prev.strides[0]:
            cur = np.ascontiguousarray(cur)
            prev = np.ascontiguousarray(prev)
        mf = np.zeros((int(H / block_size), int(W / block_size), 2), dtype=np.int32)
        _check(self.lib.gme_bbme_u8(self.handle, _p(prev, _c_u8p), _p(cur, _c_u8p), H, W, prev.strides[0],
                                    block_size, search_window, procedure, pnorm, _p(mf, _c_i32p)), self.lib)
        return mf

    def pyrdown(self, img):
        img = as_frame(img, "image")
        H, W = img.shape
        out = np.empty(((H + 1) // 2, (W + 1) // 2), dtype=np.uint8)
        _check(self.lib.gme_pyrdown_u8(self.handle, _p(img, _c_u8p), H, W, img.strides[0], _p(out, _c_u8p)), self.lib)
        return out

    def affine_field(self, params, h, w):
        p = np.ascontiguousarray(np.asarray(params).astype(np.float64).reshape(6))
        out = np.zeros((h, w, 2), dtype=np.int16)
        _check(self.lib.gme_affine_field(self.handle, _p(p, _c_f64p), h, w, _p(out, _c_i16p)), self.lib)
        return out

    def model2_field(self, params, h, w):
        """The second-order field of params float64[12] (roadmap.py) -> int16[h, w, 2]."""
        p = np.ascontiguousarray(np.asarray(params).astype(np.float64).reshape(12))
        out = np.zeros((h, w, 2), dtype=np.int16)
        _check(self.lib.gme_model2_field(self.handle, _p(p, _c_f64p), h, w, _p(out, _c_i16p)), self.lib)
        return out

    def compensate(self, frame, mf):
        frame = as_frame(frame)
        mf32 = np.ascontiguousarray(np.asarray(mf)[:, :, :2].astype(np.int32))
        H, W = frame.shape
        out = np.empty((H, W), dtype=np.uint8)
        _check(self.lib.gme_compensate_u8(self.handle, _p(frame, _c_u8p), H, W, frame.strides[0], _p(mf32, _c_i32p),
                                          mf32.shape[0], mf32.shape[1], _p(out, _c_u8p)), self.lib)
        return out

    def sse(self, a, b):
        a, b = as_frame(a, "original"), as_frame(b, "noisy")
        if a.shape != b.shape:
            raise ValueError("operands could not be broadcast together with shapes %r %r" % (a.shape, b.shape))
        v = ctypes.c_int64(0)
        _check(self.lib.gme_sse_u8(self.handle, _p(a, _c_u8p), _p(b, _c_u8p), a.shape[0], a.shape[1], a.strides[0],
                                   b.strides[0], ctypes.byref(v)), self.lib)
        return v.value


    def subpel(self, prev, cur, mf, block_size, pnorm, levels=2):
        """Quarter-pel refinement of the integer field mf int32[H // bs, W // bs, 2] of one pair (gme_subpel_u8, subpel.refine)
        -> (qfield int32[h, w, 2] in quarter pixels, cost int64[h, w])."""
        prev, cur = as_frame(prev, "previous"), as_frame(cur, "current")
        if prev.shape != cur.shape:
            raise AssertionError("previous and current differ in shape (bbme.py:59)")
        levels = _subpel_levels(levels)
        H, W = prev.shape
        block_size = _block_size(block_size)
        if cur.strides[0] != prev.strides[0]:
            cur, prev = np.ascontiguousarray(cur), np.ascontiguousarray(prev)
        h, w = int(H / block_size), int(W / block_size)
        mf32 = np.ascontiguousarray(np.asarray(mf)[:, :, :2].astype(np.int32))
        if mf32.shape != (h, w, 2):
            raise ValueError("the field of a %d x %d frame at block size %d is %r, not %r" % (H, W, block_size, (h, w, 2), mf32.shape))
        q, cost = np.zeros((h, w, 2), np.int32), np.zeros((h, w), np.int64)
        _check(self.lib.gme_subpel_u8(self.handle, _p(prev, _c_u8p), _p(cur, _c_u8p), H, W, prev.strides[0], block_size, int(pnorm),
                                      levels, _p(mf32, _c_i32p), _p(q, _c_i32p), _p(cost, _c_i64p)), self.lib)
        return q, cost

    def hier(self, prev, cur, block_size=16, coarse_window=8, radius=1, pnorm=0, levels=3):
        """Hierarchical block matching of one pair (gme_hier_u8, hier.search on the device's own pyramids) -> (field
        int32[h, w, 2] in full-resolution pixels, cost int64[h, w])."""
        prev, cur = as_frame(prev, "previous"), as_frame(cur, "current")
        if prev.shape != cur.shape:
            raise AssertionError("previous and current differ in shape (bbme.py:59)")
        block_size, coarse_window, radius, pnorm, levels = _hier_args(block_size, coarse_window, radius, pnorm, levels)
        H, W = prev.shape
        if cur.strides[0] != prev.strides[0]:
            cur, prev = np.ascontiguousarray(cur), np.ascontiguousarray(prev)
        h, w = H // block_size, W // block_size
        mf, cost = np.zeros((h, w, 2), np.int32), np.zeros((h, w), np.int64)
        _check(self.lib.gme_hier_u8(self.handle, _p(prev, _c_u8p), _p(cur, _c_u8p), H, W, prev.strides[0], block_size, coarse_window,
                                    radius, pnorm, levels, _p(mf, _c_i32p), _p(cost, _c_i64p)), self.lib)
        return mf, cost

    def vbs(self, prev, cur, mf, block_size, depth=2, radius=1, pnorm=0, penalty=0):
        """The variable-block-size tree of one pair on the integer field mf int32[H // bs, W // bs, 2] (gme_vbs_u8, vbs.tree) ->
        (leaf int32[h << depth, w << depth, 2], depth uint8[h << depth, w << depth], cost int64[h, w])."""
        prev, cur = as_frame(prev, "previous"), as_frame(cur, "current")
        if prev.shape != cur.shape:
            raise AssertionError("previous and current differ in shape (bbme.py:59)")
        block_size, depth, radius, pnorm, penalty = _vbs_args(block_size, depth, radius, pnorm, penalty)
        H, W = prev.shape
        if cur.strides[0] != prev.strides[0]:
            cur, prev = np.ascontiguousarray(cur), np.ascontiguousarray(prev)
        h, w = H // block_size, W // block_size
        mf32 = np.ascontiguousarray(np.asarray(mf)[:, :, :2].astype(np.int32))
        if mf32.shape != (h, w, 2):
            raise ValueError("the field of a %d x %d frame at block size %d is %r, not %r" % (H, W, block_size, (h, w, 2), mf32.shape))
        leaf = np.zeros((h << depth, w << depth, 2), np.int32)
        dmap, cost = np.zeros((h << depth, w << depth), np.uint8), np.zeros((h, w), np.int64)
        _check(self.lib.gme_vbs_u8(self.handle, _p(prev, _c_u8p), _p(cur, _c_u8p), H, W, prev.strides[0], block_size, depth, radius,
                                   pnorm, penalty, _p(mf32, _c_i32p), _p(leaf, _c_i32p), _p(dmap, _c_u8p), _p(cost, _c_i64p)), self.lib)
        return leaf, dmap, cost

    def bipred(self, past, mid, next, f0, f1, block_size, radius=1, rounds=1, pnorm=0, penalty=0):
        """Bidirectional prediction of ``mid`` on the integer fields f0 (into ``past``) and f1 (into ``next``), int32[H // bs,
        W // bs, 2] (gme_bipred_u8, bipred.decide and bipred.predict) -> (mode uint8[h, w], v0 int32[h, w, 2], v1 int32[h, w, 2],
        cost int64[h, w], costs int64[h, w, 3], predicted uint8[H, W], sse int)."""
        frames = [as_frame(a, name) for a, name in ((past, "past"), (mid, "mid"), (next, "next"))]
        if any(a.shape != frames[1].shape for a in frames):
            raise AssertionError("past, mid and next differ in shape (bbme.py:59)")
        block_size, radius, rounds, pnorm, penalty = _bipred_args(block_size, radius, rounds, pnorm, penalty)
        H, W = frames[1].shape
        if any(a.strides[0] != frames[1].strides[0] for a in frames):
            frames = [np.ascontiguousarray(a) for a in frames]
        h, w = H // block_size, W // block_size
        fields = [np.ascontiguousarray(np.asarray(f)[:, :, :2].astype(np.int32)) for f in (f0, f1)]
        for f in fields:
            if f.shape != (h, w, 2):
                raise ValueError("the field of a %d x %d frame at block size %d is %r, not %r" % (H, W, block_size, (h, w, 2), f.shape))
        mode, v0, v1 = np.zeros((h, w), np.uint8), np.zeros((h, w, 2), np.int32), np.zeros((h, w, 2), np.int32)
        cost, costs, pred = np.zeros((h, w), np.int64), np.zeros((h, w, 3), np.int64), np.empty((H, W), np.uint8)
        sse = ctypes.c_int64(0)
        _check(self.lib.gme_bipred_u8(self.handle, _p(frames[0], _c_u8p), _p(frames[1], _c_u8p), _p(frames[2], _c_u8p), H, W,
                                      frames[1].strides[0], block_size, radius, rounds, pnorm, penalty, _p(fields[0], _c_i32p),
                                      _p(fields[1], _c_i32p), _p(mode, _c_u8p), _p(v0, _c_i32p), _p(v1, _c_i32p), _p(cost, _c_i64p),
                                      _p(costs, _c_i64p), _p(pred, _c_u8p), ctypes.byref(sse)), self.lib)
        return mode, v0, v1, cost, costs, pred, sse.value

    def gmc(self, ref, cur, h, f, block_size, pnorm=0, penalty=0):
        """Global motion compensation of ``cur`` from ``ref`` under the warp h float64[8] on the integer field f int32[H // bs,
        W // bs, 2] (gme_gmc_u8, gmc.decide and gmc.predict) -> (mode uint8[h, w], cost int64[h, w], costs int64[h, w, 2],
        predicted uint8[H, W], sse int)."""
        frames = [as_frame(a, name) for a, name in ((ref, "ref"), (cur, "cur"))]
        if frames[0].shape != frames[1].shape:
            raise AssertionError("ref and cur differ in shape (bbme.py:59)")
        block_size, pnorm, penalty = _gmc_args(block_size, pnorm, penalty)
        H, W = frames[1].shape
        if frames[0].strides[0] != frames[1].strides[0]:
            frames = [np.ascontiguousarray(a) for a in frames]
        hb, wb = H // block_size, W // block_size
        warp = np.ascontiguousarray(np.asarray(h, dtype=np.float64).reshape(8))
        field = np.ascontiguousarray(np.asarray(f)[:, :, :2].astype(np.int32))
        if field.shape != (hb, wb, 2):
            raise ValueError("the field of a %d x %d frame at block size %d is %r, not %r" % (H, W, block_size, (hb, wb, 2), field.shape))
        mode, cost, costs = np.zeros((hb, wb), np.uint8), np.zeros((hb, wb), np.int64), np.zeros((hb, wb, 2), np.int64)
        pred = np.empty((H, W), np.uint8)
        sse = ctypes.c_int64(0)
        _check(self.lib.gme_gmc_u8(self.handle, _p(frames[0], _c_u8p), _p(frames[1], _c_u8p), H, W, frames[1].strides[0], block_size, pnorm,
                                   penalty, _p(warp, _c_f64p), _p(field, _c_i32p), _p(mode, _c_u8p), _p(cost, _c_i64p),
                                   _p(costs, _c_i64p), _p(pred, _c_u8p), ctypes.byref(sse)), self.lib)
        return mode, cost, costs, pred, sse.value

    def prop(self, prev, cur, f, block_size, pnorm=0, rounds=2, steps=1, t=None, g=None):
        """Vector propagation of one pair on the prior field f int32[H // bs, W // bs, 2], with the previous pair's field ``t`` and
        the camera field ``g`` of the same shape where given (gme_prop_u8, propagate.search) -> (mf int32[h, w, 2], cost
        int64[h, w], source uint8[h, w])."""
        prev, cur = as_frame(prev, "previous"), as_frame(cur, "current")
        if prev.shape != cur.shape:
            raise AssertionError("previous and current differ in shape (bbme.py:59)")
        block_size, pnorm, rounds, steps = _prop_args(block_size, pnorm, rounds, steps)
        H, W = prev.shape
        if cur.strides[0] != prev.strides[0]:
            cur, prev = np.ascontiguousarray(cur), np.ascontiguousarray(prev)
        h, w = H // block_size, W // block_size
        fields = [None if a is None else _prop_field(a, name, (h, w)) for a, name in ((f, "f"), (t, "t"), (g, "g"))]
        if fields[0] is None:
            raise ValueError("f is the prior field, int32[%d, %d, 2]" % (h, w))
        mf, cost, source = np.zeros((h, w, 2), np.int32), np.zeros((h, w), np.int64), np.zeros((h, w), np.uint8)
        _check(self.lib.gme_prop_u8(self.handle, _p(prev, _c_u8p), _p(cur, _c_u8p), H, W, prev.strides[0], block_size, pnorm, rounds, steps,
                                    *[None if a is None else _p(a, _c_i32p) for a in fields], _p(mf, _c_i32p), _p(cost, _c_i64p),
                                    _p(source, _c_u8p)), self.lib)
        return mf, cost, source

    def interp(self, past, next, block_size, search_window=8, pnorm=0, bias=0, truth=None):
        """The frame halfway between ``past`` and ``next`` (gme_interp_u8, interp.search and interp.interpolate) -> (mv int32[h, w,
        2], cost int64[h, w], dist int64[h, w], frame uint8[H, W], sse int): ``sse`` is the squared error against ``truth``, the true
        middle frame, or -1 without one."""
        frames = [as_frame(a, name) for a, name in ((past, "past"), (next, "next")) + (() if truth is None else ((truth, "truth"),))]
        if any(a.shape != frames[0].shape for a in frames):
            raise AssertionError("the frames differ in shape (bbme.py:59)")
        H, W = frames[0].shape
        block_size, search_window, pnorm, bias = _interp_args(block_size, search_window, pnorm, bias, H, W)
        if any(a.strides[0] != frames[0].strides[0] for a in frames):
            frames = [np.ascontiguousarray(a) for a in frames]
        h, w = H // block_size, W // block_size
        mv, cost, dist = np.zeros((h, w, 2), np.int32), np.zeros((h, w), np.int64), np.zeros((h, w), np.int64)
        made = np.empty((H, W), np.uint8)
        sse = ctypes.c_int64(0)
        _check(self.lib.gme_interp_u8(self.handle, _p(frames[0], _c_u8p), _p(frames[1], _c_u8p),
                                      None if truth is None else _p(frames[2], _c_u8p), H, W, frames[0].strides[0], block_size,
                                      search_window, pnorm, bias, _p(mv, _c_i32p), _p(cost, _c_i64p), _p(dist, _c_i64p), _p(made, _c_u8p),
                                      ctypes.byref(sse)), self.lib)
        return mv, cost, dist, made, sse.value

    def retime(self, past, next, block_size, search_window=16, pnorm=0, bias=0, n=1, d=2, truth=None):
        """The frame at phase n / d between ``past`` and ``next`` (gme_retime_u8, retime.search and retime.interpolate) -> (mv
        int32[h, w, 2], cost int64[h, w], dist int64[h, w], frame uint8[H, W], sse int): ``sse`` is the squared error against
        ``truth``, the true frame at that time, or -1 without one."""
        import retime
        frames = [as_frame(a, name) for a, name in ((past, "past"), (next, "next")) + (() if truth is None else ((truth, "truth"),))]
        if any(a.shape != frames[0].shape for a in frames):
            raise AssertionError("the frames differ in shape (bbme.py:59)")
        H, W = frames[0].shape
        block_size, search_window, pnorm, bias = retime.check_args(block_size, search_window, pnorm, bias)
        retime.check_shape(H, W, block_size)
        n, d = retime.check_phase(n, d)
        if any(a.strides[0] != frames[0].strides[0] for a in frames):
            frames = [np.ascontiguousarray(a) for a in frames]
        h, w = H // block_size, W // block_size
        mv, cost, dist = np.zeros((h, w, 2), np.int32), np.zeros((h, w), np.int64), np.zeros((h, w), np.int64)
        made = np.empty((H, W), np.uint8)
        sse = ctypes.c_int64(0)
        _check(self.lib.gme_retime_u8(self.handle, _p(frames[0], _c_u8p), _p(frames[1], _c_u8p),
                                      None if truth is None else _p(frames[2], _c_u8p), H, W, frames[0].strides[0], block_size,
                                      search_window, pnorm, bias, n, d, _p(mv, _c_i32p), _p(cost, _c_i64p), _p(dist, _c_i64p),
                                      _p(made, _c_u8p), ctypes.byref(sse)), self.lib)
        return mv, cost, dist, made, sse.value

    def retime_clip(self, frames, block_size, search_window=16, pnorm=0, bias=0, step=(1, 2), first=0, count=None):
        """The outputs first .. first + count - 1 (default: all from ``first``) of retime.schedule for the clip ``frames`` uint8[N,
        H, W] at the step (num, den) input frames per output (gme_retime_clip_u8) -> (frames uint8[count, H, W], mv int32[count, h,
        w, 2], cost int64[count, h, w], dist int64[count, h, w]); a copy comes with zero vectors and costs.  A range outside the
        schedule is an IndexError."""
        import retime
        frames = np.ascontiguousarray(frames)
        if frames.ndim != 3 or frames.dtype != np.uint8 or len(frames) < 1:
            raise TypeError("frames must be uint8[N, H, W], N >= 1")
        N, H, W = frames.shape
        block_size, search_window, pnorm, bias = retime.check_args(block_size, search_window, pnorm, bias)
        retime.check_shape(H, W, block_size)
        num, den = int(step[0]), int(step[1])
        M = len(retime.schedule(N, num, den))
        first = int(first)
        count = M - first if count is None else int(count)
        if first < 0 or count < 0 or first + count > M:
            raise IndexError("outputs [%d, %d) outside [0, %d)" % (first, first + count, M))
        h, w = H // block_size, W // block_size
        made = np.empty((count, H, W), np.uint8)
        mv, cost, dist = np.zeros((count, h, w, 2), np.int32), np.zeros((count, h, w), np.int64), np.zeros((count, h, w), np.int64)
        _check(self.lib.gme_retime_clip_u8(self.handle, _p(frames, _c_u8p), N, H, W, W, block_size, search_window, pnorm, bias, num, den,
                                           first, count, _p(made, _c_u8p), _p(mv, _c_i32p), _p(cost, _c_i64p), _p(dist, _c_i64p)),
               self.lib)
        return made, mv, cost, dist

    def obmc(self, prev, field, block_size, quarter=True, cur=None):
        """``prev`` compensated by the block field with overlapped blocks (gme_obmc_u8, obmc.compensate) -> (frame uint8[H, W],
        sse int): ``field`` int32[H // B, W // B, 2] in quarter pixels, or with ``quarter`` false in whole pixels (components within
        +-2**29); ``sse`` is the squared error against ``cur``, or -1 without one."""
        import obmc
        frames = [as_frame(prev, "prev")] + ([] if cur is None else [as_frame(cur, "cur")])
        if any(a.shape != frames[0].shape for a in frames):
            raise AssertionError("the frames differ in shape (bbme.py:59)")
        H, W = frames[0].shape
        block_size = obmc.check_block_size(block_size)
        obmc.check_shape(H, W, block_size)
        field = _obmc_field(field, H, W, block_size, quarter)
        if any(a.strides[0] != frames[0].strides[0] for a in frames):
            frames = [np.ascontiguousarray(a) for a in frames]
        made = np.empty((H, W), np.uint8)
        sse = ctypes.c_int64(0)
        _check(self.lib.gme_obmc_u8(self.handle, _p(frames[0], _c_u8p), None if cur is None else _p(frames[1], _c_u8p), H, W,
                                    frames[0].strides[0], block_size, _p(field, _c_i32p), 1 if quarter else 4, _p(made, _c_u8p),
                                    ctypes.byref(sse)), self.lib)
        return made, sse.value


    def denoise(self, cur, refs, fields, block_size, quarter=False, strength=24, truth=None):
        """``cur`` filtered with the overlapped predictions of it from ``refs`` (gme_denoise_u8, denoise.frame) -> (frame
        uint8[H, W], sse int): ``fields[r]`` int32[H // B, W // B, 2] says where the blocks of ``cur`` are found in ``refs[r]``, in
        whole pixels (components within +-2**29) or with ``quarter`` in quarter pixels; ``sse`` is the squared error against
        ``truth``, or -1 without one.  The default strength is a convention of the tool, not a tuned value."""
        import denoise
        import obmc
        refs, fields = list(refs), list(fields)
        R, strength = denoise.check_args(len(refs), strength)
        if len(fields) != R:
            raise ValueError("%d references, %d fields" % (R, len(fields)))
        frames = [as_frame(cur, "cur")] + [as_frame(a, "ref") for a in refs] + ([] if truth is None else [as_frame(truth, "truth")])
        if any(a.shape != frames[0].shape for a in frames):
            raise AssertionError("the frames differ in shape (bbme.py:59)")
        H, W = frames[0].shape
        block_size = obmc.check_block_size(block_size)
        obmc.check_shape(H, W, block_size)
        fields = [_obmc_field(f, H, W, block_size, quarter) for f in fields]
        if any(a.strides[0] != frames[0].strides[0] for a in frames):
            frames = [np.ascontiguousarray(a) for a in frames]
        ref_ptrs = (_c_u8p * R)(*[_p(a, _c_u8p) for a in frames[1:1 + R]])
        field_ptrs = (_c_i32p * R)(*[_p(f, _c_i32p) for f in fields])
        made = np.empty((H, W), np.uint8)
        sse = ctypes.c_int64(0)
        _check(self.lib.gme_denoise_u8(self.handle, _p(frames[0], _c_u8p), ref_ptrs, field_ptrs, R, H, W, frames[0].strides[0], block_size,
                                       1 if quarter else 4, strength, None if truth is None else _p(frames[-1], _c_u8p), _p(made, _c_u8p),
                                       ctypes.byref(sse)), self.lib)
        return made, sse.value


def _obmc_field(field, H, W, block_size, quarter):
    """obmc.check_field and the range of an integer field: ValueError before the library is asked -> contiguous int32."""
    import obmc
    field = obmc.check_field(field, H, W, block_size)
    limit = (1 << 31) - 1 if quarter else obmc.MAX_INTEGER_VECTOR
    if field.size and (int(field.min()) < (-limit - 1 if quarter else -limit) or int(field.max()) > limit):
        raise ValueError("a vector component beyond %s" % ("int32" if quarter else "+-2**29 whole pixels"))
    return np.ascontiguousarray(field, dtype=np.int32)


def _interp_args(block_size, search_window, pnorm, bias, H, W):
    """interp.check_args and interp.check_shape: the definition's argument rules, ValueError before the library is asked."""
    import interp
    args = interp.check_args(block_size, search_window, pnorm, bias)
    interp.check_shape(H, W, args[0])
    return args


def _prop_args(block_size, pnorm, rounds, steps):
    """propagate.check_args: the definition's argument rules, ValueError before the library is asked."""
    import propagate
    return propagate.check_args(block_size, pnorm, rounds, steps)


def _prop_field(a, name, grid):
    """A field of vector propagation as contiguous int32[..., 2] of the block grid ``grid`` (the leading axes), or ValueError."""
    a = np.asarray(a)
    if a.ndim != len(grid) + 1 or a.shape[:-1] != tuple(grid) or a.shape[-1] < 2:
        raise ValueError("%s is %r, not %r" % (name, a.shape, tuple(grid) + (2,)))
    return np.ascontiguousarray(a[..., :2].astype(np.int32))


def _gmc_args(block_size, pnorm, penalty):
    """gmc.check_args: the definition's argument rules, ValueError before the library is asked."""
    import gmc
    return gmc.check_args(block_size, pnorm, penalty)


def _bipred_args(block_size, radius, rounds, pnorm, penalty):
    """bipred.check_args: the definition's argument rules, ValueError before the library is asked."""
    import bipred
    return bipred.check_args(block_size, radius, rounds, pnorm, penalty)


def _vbs_args(block_size, depth, radius, pnorm, penalty):
    """vbs.check_args: the definition's argument rules, ValueError before the library is asked."""
    import vbs
    return vbs.check_args(block_size, depth, radius, pnorm, penalty)


def _hier_args(block_size, coarse_window, radius, pnorm, levels):
    """hier.check_args: the definition's argument rules, ValueError before the library is asked."""
    import hier
    return hier.check_args(block_size, coarse_window, radius, pnorm, levels)


def _subpel_levels(levels):
    levels = int(levels)
    if levels not in (0, 1, 2):
        raise ValueError("levels %d (0: integer, 1: half-pel, 2: quarter-pel)" % levels)
    return levels


class Sequence:
    """N frames resident in HBM (gme_seq) and the per-pair results computed from them."""

    def __init__(self, ctx, n_frames, height, width):
        self.ctx, self.lib = ctx, ctx.lib
        self.N, self.H, self.W = int(n_frames), int(height), int(width)
        self.N_cap = self.N                      # frames the device buffers hold; N = frames in use (set_frames)
        self.handle = self.lib.gme_seq_create(ctx.handle, self.N, self.H, self.W)
        if not self.handle:
            raise GmeError("gme_seq_create failed: %s" % self.lib.gme_last_error().decode())
        ctx._sequences.add(self)
        self._gme = None

    @classmethod
    def from_frames(cls, ctx, frames):
        frames = [as_frame(f) for f in frames] if not isinstance(frames, np.ndarray) else frames
        if isinstance(frames, np.ndarray):
            if frames.ndim != 3 or frames.dtype != np.uint8:
                raise TypeError("frames must be uint8[N, H, W]")
            frames = np.ascontiguousarray(frames)
            seq = cls(ctx, frames.shape[0], frames.shape[1], frames.shape[2])
            seq.upload(0, frames)
            return seq
        seq = cls(ctx, len(frames), *frames[0].shape)
        for k, f in enumerate(frames):
            if f.shape != frames[0].shape:
                raise ValueError("all frames of a sequence must share one shape")
            seq.upload(k, np.ascontiguousarray(f)[None])
        return seq

    def close(self):
        if getattr(self, "handle", None):
            if getattr(self.ctx, "handle", None):  # the context may already be gone at interpreter exit
                self.lib.gme_seq_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def upload(self, first, frames):
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
        n, H, W = frames.shape
        if (H, W) != (self.H, self.W):
            raise ValueError("frame shape %r does not match the sequence %r" % ((H, W), (self.H, self.W)))
        _check(self.lib.gme_seq_upload(self.handle, first, n, _p(frames, _c_u8p), W, H * W), self.lib)

    def set_frames(self, n_frames):
        """Use only the first `n_frames` frames from now on (1 <= n_frames <= N_cap): every stage call covers the pairs of
        frames [0, n_frames); the device buffers stay sized for N_cap.  Ends a staged GME run; a change of the count is new
        frame data to every result the sequence keeps (include/gme_hip.h, "Result lifetimes")."""
        _check(self.lib.gme_seq_set_frames(self.handle, int(n_frames)), self.lib)
        self.N = int(n_frames)

    def synth(self, seed, t0=0):
        _check(self.lib.gme_seq_synth(self.handle, seed, t0), self.lib)

    def invalidate_pyramids(self):
        """Force the next gme_begin to rebuild pyramid levels 1 and 0 (done automatically after
        upload/synth; bench.py uses it so that every timed step pays for its pyramids)."""
        _check(self.lib.gme_seq_invalidate(self.handle), self.lib)

    def level_shape(self, level):
        h, w = self.H, self.W
        for _ in range(2 - level):
            h, w = (h + 1) // 2, (w + 1) // 2
        return h, w

    def read_frame(self, index, level=2):
        out = np.empty(self.level_shape(level), dtype=np.uint8)
        _check(self.lib.gme_seq_read_frame(self.handle, level, index, _p(out, _c_u8p)), self.lib)
        return out

    # ---- BBME over all pairs
    def bbme(self, frame_distance, block_size, search_window, procedure, pnorm):
        block_size = _block_size(block_size)
        _check(self.lib.gme_seq_bbme(self.handle, frame_distance, block_size, search_window, procedure, pnorm), self.lib)
        self._mv_shape = (self.N - frame_distance, int(self.H / block_size), int(self.W / block_size), 2)

    def bbme_streamed(self, frames, frame_distance, block_size, search_window, procedure, pnorm, chunk_frames=128):
        """bbme() for frames that still live in host memory (uint8[n, H, W], n <= N): chunked upload on a
        copy stream overlapped with the search of the previous chunk -> int32[n - fd, h, w, 2].

        The array returned is a page-locked buffer that belongs to the sequence and is OVERWRITTEN by the next
        bbme_streamed() call on it: copy it if it has to outlive that call ("Host frames, streamed")."""
        block_size = _block_size(block_size)
        frames = np.asarray(frames)
        if frames.ndim != 3 or frames.dtype != np.uint8 or frames.shape[1:] != (self.H, self.W):
            raise TypeError("frames must be uint8[n, %d, %d]" % (self.H, self.W))
        if frames.strides[2] != 1 or frames.strides[1] < self.W or frames.strides[0] < frames.strides[1] * self.H:
            frames = np.ascontiguousarray(frames)
        n = frames.shape[0]
        shape = (max(n - frame_distance, 0), int(self.H / block_size), int(self.W / block_size), 2)
        # page-locked result (the read-backs never hold the calling thread), kept with the sequence: pinning
        # 22 MB takes several milliseconds, more than the search of 2048 pairs.  The array returned is this
        # buffer: copy it if it has to outlive the next bbme_streamed() call on the same sequence.
        out = getattr(self, "_stream_out", None)
        if out is None or out.shape != shape:
            try:
                out = pinned_empty(shape, np.int32) if shape[0] else np.empty(shape, np.int32)
            except MemoryError:
                out = np.empty(shape, dtype=np.int32)
            self._stream_out = out
        _check(self.lib.gme_seq_bbme_streamed(self.handle, _p(frames, _c_u8p), frames.strides[1], frames.strides[0], n,
                                              frame_distance, block_size, search_window, procedure, pnorm, int(chunk_frames),
                                              _p(out, _c_i32p)), self.lib)
        self._mv_shape = out.shape
        return out

    def read_mv(self, first=0, count=None):
        pairs = self._mv_shape[0]
        count = pairs - first if count is None else count
        out = np.empty((count,) + self._mv_shape[1:], dtype=np.int32)
        if out.size:
            _check(self.lib.gme_seq_read_mv(self.handle, first, count, _p(out, _c_i32p)), self.lib)
        return out

    def mv_summary(self):
        """Per-pair summary rows of the last bbme() field -> float64[P, 6] = modal vector x, y (over [-64, 64)^2),
        its block count, sum of x, sum of y, checksum (include/gme_hip.h: gme_seq_mv_summary)."""
        out = np.empty((self._mv_shape[0], 6), dtype=np.float64)
        _check(self.lib.gme_seq_mv_summary(self.handle, _p(out, _c_f64p)), self.lib)
        return out

    def mv_summary_gather(self, n_max, world, slot=0):
        """mv_summary() of every rank, all-gathered device to device over the context's RCCL communicator
        -> float64[world, n_max, 6] (each rank's block zero-padded to n_max rows).  In split-phase mode the array
        is filled once wait() returns; `slot` picks one of several page-locked result buffers so that a caller
        can queue the next step while it still reads the previous one."""
        out = self._buffer("gathered%d" % slot, (int(world), int(n_max), 6), np.float64, by_frames=False)
        _check(self.lib.gme_seq_mv_summary_gather(self.handle, int(n_max), _p(out, _c_f64p)), self.lib)
        return out

    # ---- GME stages
    # -- split-phase calls (gme_seq_set_split_phase): gme_begin / gme_fit / compensate queue their work and hand back
    #    page-locked arrays that are filled once wait() returns; one host thread can then drive several sequences
    def set_split_phase(self, on=True):
        """Split-phase mode: upload / gme_begin / gme_fit / compensate / mv_summary_gather return once queued.  The arrays
        they hand back are page-locked buffers owned by the sequence, one per call kind, REUSED by the next call of that
        kind and valid only after wait(); the blocking helpers (motion.estimate_sequence) refuse a sequence in this mode."""
        _check(self.lib.gme_seq_set_split_phase(self.handle, int(bool(on))), self.lib)
        self._split = bool(on)                   # the page-locked buffers stay with the sequence for the next time

    def wait(self):
        _check(self.lib.gme_seq_wait(self.handle), self.lib)

    def poll(self):
        """True when wait() would return at once (the last split-phase result has arrived)."""
        rc = self.lib.gme_seq_poll(self.handle)
        if rc < 0:
            _raise(rc, self.lib)
        return rc == 1

    def _buffer(self, name, shape, dtype, by_frames=True):
        """Result / argument array of a staged call: ordinary memory, or (split-phase) one page-locked block per
        name and shape kept with the sequence -- the copy engine writes it while the caller is elsewhere."""
        if not getattr(self, "_split", False):
            return np.empty(shape, dtype=dtype)
        pin = self.__dict__.setdefault("_pin", {})
        shape = tuple(shape)
        a = pin.get(name)
        if a is None or a.shape[1:] != shape[1:] or a.shape[0] < shape[0] or a.dtype != np.dtype(dtype):
            # one block per name, sized for the sequence's full frame count: set_frames() changes the rows in use,
            # pinning memory anew for every chunk length would cost more than the chunk
            full = (max(shape[0], self.N_cap) if by_frames else shape[0],) + shape[1:]
            try:
                a = pinned_empty(full, dtype) if int(np.prod(full)) else np.empty(full, dtype=dtype)
            except MemoryError:                  # no page-locked memory left: the copies still work, they just hold the caller
                a = np.empty(full, dtype=dtype)
            pin[name] = a
        return a[:shape[0]]

    def gme_begin(self, frame_distance, bbme_block_size, procedure=3, search_window=2):
        pairs = self.N - frame_distance
        bbme_block_size = _block_size(bbme_block_size)
        p0 = self._buffer("p0", (max(pairs, 0), 6), np.float32)
        _check(self.lib.gme_seq_gme_begin(self.handle, frame_distance, bbme_block_size, procedure, search_window,
                                          _p(p0, _c_f32p)), self.lib)
        self._gme = (frame_distance, bbme_block_size, pairs)
        return p0

    # Model orders: 1 = affine (params float64[P, 6], sums float64[P, 15] = F (9) | Sx (3) | Sy (3)); 2 = the second-order
    # models of roadmap.py (params float64[P, 12], sums float64[P, 27] = moments (15) | Sx (6) | Sy (6)).  Each order has
    # its own C entry points and its own reused buffers (split-phase callers hold the returned arrays).
    _ORDER = {1: (6, 15, ""), 2: (12, 27, "2")}          # order -> (parameters, sums, entry-point suffix)

    def _begin_fit(self, order, frame_distance, bbme_block_size, outlier_fraction, procedure, search_window):
        n_sums, suffix = self._ORDER[order][1:]
        pairs = self.N - frame_distance
        bbme_block_size = _block_size(bbme_block_size)
        p0 = self._buffer("p0", (max(pairs, 0), 6), np.float32)
        sums = self._buffer("sums%d_1" % order, (max(pairs, 0), n_sums), np.float64)
        _check(getattr(self.lib, "gme_seq_gme_begin_fit" + suffix)(self.handle, frame_distance, bbme_block_size, procedure,
                                                                   search_window, float(outlier_fraction), _p(p0, _c_f32p),
                                                                   _p(sums, _c_f64p)), self.lib)
        self._gme = (frame_distance, bbme_block_size, pairs)
        return p0, sums

    def _fit(self, order, level, params_in, outlier_fraction):
        n_params, n_sums, suffix = self._ORDER[order]
        pairs = self._gme[2] if level >= 0 else self._mv_shape[0]
        p = self._buffer("fit%d_in%d" % (order, level), (pairs, n_params), np.float64)
        p[...] = np.asarray(params_in, dtype=np.float64).reshape(pairs, n_params)
        sums = self._buffer("sums%d_%d" % (order, level), (pairs, n_sums), np.float64)
        _check(getattr(self.lib, "gme_seq_gme_fit" + suffix)(self.handle, level, _p(p, _c_f64p), float(outlier_fraction),
                                                             _p(sums, _c_f64p)), self.lib)
        return sums

    def _compensate(self, order, frame_distance, block_size, params):
        n_params, _, suffix = self._ORDER[order]
        pairs = self.N - frame_distance
        block_size = _block_size(block_size)
        p = self._buffer("comp%d_in" % order, (pairs, n_params), np.float64)
        p[...] = np.asarray(params, dtype=np.float64).reshape(pairs, n_params)
        sse = self._buffer("sse", (pairs,), np.int64)
        _check(getattr(self.lib, "gme_seq_compensate" + suffix)(self.handle, frame_distance, block_size, _p(p, _c_f64p),
                                                                _p(sse, _c_i64p)), self.lib)
        return sse

    def gme_begin_fit(self, frame_distance, bbme_block_size, outlier_fraction, procedure=3, search_window=2):
        """gme_begin + projection of the first parameters + gme_fit(level 1) without the trip to the host in between
        -> (first parameters float32[P, 6], level-1 sums float64[P, 15]); the level-2 search is queued behind."""
        return self._begin_fit(1, frame_distance, bbme_block_size, outlier_fraction, procedure, search_window)

    def gme_fit(self, level, params_in, outlier_fraction):
        """-> sums float64[P, 15] = F (9) | Sx (3) | Sy (3).  level -1 fits the field of the
        last bbme() call against the full-resolution frame size."""
        return self._fit(1, level, params_in, outlier_fraction)

    def gme_begin_fit2(self, frame_distance, bbme_block_size, outlier_fraction, procedure=3, search_window=2):
        """gme_begin_fit with the order-2 sums -> (first parameters float32[P, 6], level-1 sums float64[P, 27])."""
        return self._begin_fit(2, frame_distance, bbme_block_size, outlier_fraction, procedure, search_window)

    def gme_fit2(self, level, params_in, outlier_fraction):
        """gme_fit for params float64[P, 12] -> sums float64[P, 27] = moments (15) | Sx (6) | Sy (6)."""
        return self._fit(2, level, params_in, outlier_fraction)

    def compensate2(self, frame_distance, block_size, params):
        """compensate() with the order-2 field of params float64[P, 12] -> sse int64[P]."""
        return self._compensate(2, frame_distance, block_size, params)

    def stage_shape(self, level):
        if level < 0:
            return self._mv_shape[1:3]
        h, w = self.level_shape(level)
        bs = 2 if level == 0 else self._gme[1]
        return int(h / bs), int(w / bs)

    def gme_read_stage(self, level, pair):
        h, w = self.stage_shape(level)
        gt = np.empty((h, w, 2), dtype=np.int32)
        model = np.empty((h, w, 2), dtype=np.int16)
        mask = np.empty((h, w), dtype=np.uint8)
        thr = ctypes.c_int64(0)
        _check(self.lib.gme_seq_gme_read_stage(self.handle, level, pair, _p(gt, _c_i32p), _p(model, _c_i16p),
                                               _p(mask, _c_u8p), ctypes.byref(thr)), self.lib)
        if level == 0:
            return {"gt": gt}
        return {"gt": gt, "model": model, "mask": mask.astype(bool), "thr": thr.value}

    # ---- compensation + squared error
    def compensate(self, frame_distance, block_size, params):
        """Compensated frames of the affine params float64[P, 6] -> sse int64[P]."""
        return self._compensate(1, frame_distance, block_size, params)

    def gme_device_solve(self, frame_distance, bbme_block_size, outlier_fraction, procedure=3, search_window=2):
        """The whole estimate + compensation with the 3x3 solves on the device (gme_seq_gme_device_solve): one round trip
        -> (params float64[P, 6], sse int64[P], flags int32[P]); pairs with a non-zero flag must be redone by the staged calls."""
        pairs = self.N - frame_distance
        bbme_block_size = _block_size(bbme_block_size)
        params = self._buffer("dev_params", (max(pairs, 0), 6), np.float64)
        sse = self._buffer("dev_sse", (max(pairs, 0),), np.int64)
        flags = self._buffer("dev_flags", (max(pairs, 0),), np.int32)
        _check(self.lib.gme_seq_gme_device_solve(self.handle, frame_distance, bbme_block_size, procedure, search_window,
                                                 float(outlier_fraction), _p(params, _c_f64p), _p(sse, _c_i64p), _p(flags, _c_i32p)), self.lib)
        self._gme = (frame_distance, bbme_block_size, pairs)
        return params, sse, flags

    def gme_device_solve2(self, model, frame_distance, bbme_block_size, outlier_fraction, procedure=3, search_window=2):
        """gme_device_solve for a second-order `model` (gme_seq_gme_device_solve2) -> (params float64[P, 12], sse int64[P],
        flags int32[P]); pairs with a non-zero flag must be redone by the staged order-2 calls."""
        mid = model_id(model)
        pairs = self.N - frame_distance
        bbme_block_size = _block_size(bbme_block_size)
        params = self._buffer("dev2_params", (max(pairs, 0), 12), np.float64)
        sse = self._buffer("dev_sse", (max(pairs, 0),), np.int64)
        flags = self._buffer("dev_flags", (max(pairs, 0),), np.int32)
        _check(self.lib.gme_seq_gme_device_solve2(self.handle, mid, frame_distance, bbme_block_size, procedure, search_window,
                                                  float(outlier_fraction), _p(params, _c_f64p), _p(sse, _c_i64p),
                                                  _p(flags, _c_i32p)), self.lib)
        self._gme = (frame_distance, bbme_block_size, pairs)
        return params, sse, flags

    # ---- direct projective refinement (gme_direct.hip, direct.py)
    def _projective(self, frame_distance, params):
        if getattr(self, "_split", False):
            raise RuntimeError("the projective calls are blocking: the sequence is in split-phase mode")
        pairs = self.N - int(frame_distance)
        if pairs < 0:
            raise IndexError("frame_distance %d needs at least %d frames" % (frame_distance, frame_distance + 1))
        return pairs, np.ascontiguousarray(np.asarray(params, dtype=np.float64).reshape(pairs, 8))

    def direct_eval(self, frame_distance, level, params, outlier_fraction=0.1):
        """One evaluation per pair at params float64[P, 8] in level-`level` coordinates with a fresh threshold
        (gme_seq_direct_eval) -> dict(threshold float64[P], counts int64[P, 2] = n_valid, n_in, cost float64[P],
        sums float64[P, 44] = JtJ upper triangle | Jte)."""
        pairs, p = self._projective(frame_distance, params)
        out = {"threshold": np.zeros(pairs), "counts": np.zeros((pairs, 2), np.int64), "cost": np.zeros(pairs),
               "sums": np.zeros((pairs, 44))}
        _check(self.lib.gme_seq_direct_eval(self.handle, int(frame_distance), int(level), _p(p, _c_f64p), float(outlier_fraction),
                                            _p(out["threshold"], _c_f64p), _p(out["counts"], _c_i64p), _p(out["cost"], _c_f64p),
                                            _p(out["sums"], _c_f64p)), self.lib)
        return out

    def refine_projective(self, frame_distance, init, outlier_fraction=0.1, max_iters=10):
        """Direct projective refinement of every pair from init float64[P, 8] (full resolution; gme_seq_refine_projective)
        -> (params float64[P, 8], flags int32[P])."""
        pairs, p = self._projective(frame_distance, init)
        params = np.zeros((pairs, 8))
        flags = np.zeros(pairs, np.int32)
        _check(self.lib.gme_seq_refine_projective(self.handle, int(frame_distance), _p(p, _c_f64p), float(outlier_fraction),
                                                  int(max_iters), _p(params, _c_f64p), _p(flags, _c_i32p)), self.lib)
        return params, flags

    def compensate_projective(self, frame_distance, params):
        """Dense compensation under params float64[P, 8] (gme_seq_compensate_projective) -> sse int64[P]; the frames are
        read with read_compensated(_range)."""
        pairs, p = self._projective(frame_distance, params)
        sse = np.zeros(pairs, np.int64)
        _check(self.lib.gme_seq_compensate_projective(self.handle, int(frame_distance), _p(p, _c_f64p), _p(sse, _c_i64p)), self.lib)
        return sse

    def read_compensated(self, pair):
        """Compensated frame `pair` of the last compensating or predicting call; a pair that call did not write is a GmeError."""
        out = np.empty((self.H, self.W), dtype=np.uint8)
        _check(self.lib.gme_seq_read_compensated(self.handle, pair, _p(out, _c_u8p)), self.lib)
        return out

    def read_compensated_range(self, first, count, out=None):
        """Compensated frames of pairs first .. first+count-1 -> uint8[count, H, W] with one wait (into `out` if given)."""
        if out is None:
            out = np.empty((count, self.H, self.W), dtype=np.uint8)
        if out.shape != (count, self.H, self.W) or out.dtype != np.uint8 or not out.flags.c_contiguous:
            raise ValueError("out must be a contiguous uint8[%d, %d, %d]" % (count, self.H, self.W))
        _check(self.lib.gme_seq_read_compensated_range(self.handle, int(first), int(count), _p(out, _c_u8p)), self.lib)
        return out

    # ---- video stabilization (gme_stab.hip, stabilize.py)
    def warp_frames(self, first, warps, border=0, fill=0):
        """Frames first .. first+count-1 warped by warps float64[count, 8] (gme_seq_warp_frames; border 0 constant `fill`,
        1 replicate) into the sequence's warped frames -> valid int64[count], the in-frame samples per frame."""
        if getattr(self, "_split", False):
            raise RuntimeError("the stabilization calls are blocking: the sequence is in split-phase mode")
        w = np.ascontiguousarray(np.asarray(warps, dtype=np.float64).reshape(-1, 8))
        valid = np.zeros(len(w), np.int64)
        _check(self.lib.gme_seq_warp_frames(self.handle, int(first), len(w), _p(w, _c_f64p), int(border), int(fill),
                                            _p(valid, _c_i64p)), self.lib)
        return valid

    def read_warped_range(self, first, count):
        """Warped frames first .. first+count-1 -> uint8[count, H, W] with one wait."""
        out = np.empty((int(count), self.H, self.W), dtype=np.uint8)
        _check(self.lib.gme_seq_read_warped_range(self.handle, int(first), int(count), _p(out, _c_u8p)), self.lib)
        return out

    def frame_sse(self, warped, first, count):
        """sum (f[first+k+1] - f[first+k])^2 for k < count, of the resident (warped=0) or warped (1) frames -> int64[count]."""
        sse = np.zeros(int(count), np.int64)
        _check(self.lib.gme_seq_frame_sse(self.handle, int(warped), int(first), int(count), _p(sse, _c_i64p)), self.lib)
        return sse

    def warp_fill(self, first, sources, warps, border=0, fill=0, want_source=False):
        """Output frames first .. first+count-1, each pixel from the first of its frame's candidates (sources int32[count, n]
        absolute frame indices or -1, warps float64[count, n, 8], n in 1 .. 17) whose sample point lies in its frame, the border
        rule on candidate 0 elsewhere (gme_seq_warp_fill, stabilize.warp_fill) -> (frames uint8[count, H, W], source
        uint8[count, H, W] or None, valid int64[count], filled int64[count], sse int64[count - 1]).  One blocking call, also in
        split-phase mode, that keeps nothing and leaves everything the sequence holds as it was."""
        src = np.ascontiguousarray(sources, dtype=np.int32)
        if src.ndim != 2:
            raise ValueError("sources must be int32[count, n], not of shape %r" % (src.shape,))
        count, n = src.shape
        w = np.ascontiguousarray(np.asarray(warps, dtype=np.float64).reshape(count, n, 8))
        frames = np.empty((count, self.H, self.W), np.uint8)
        who = np.empty((count, self.H, self.W), np.uint8) if want_source else None
        valid, filled = np.zeros(max(count, 1), np.int64), np.zeros(max(count, 1), np.int64)
        sse = np.zeros(max(count - 1, 1), np.int64)
        _check(self.lib.gme_seq_warp_fill(self.handle, int(first), count, n, _p(src, _c_i32p), _p(w, _c_f64p), int(border), int(fill),
                                          _p(frames, _c_u8p), None if who is None else _p(who, _c_u8p), _p(valid, _c_i64p),
                                          _p(filled, _c_i64p), _p(sse, _c_i64p)), self.lib)
        return frames, who, valid[:count], filled[:count], sse[:max(count - 1, 0)]

    # ---- background mosaic and moving-object masks (gme_mosaic.hip, mosaic.py)
    def _blocking(self, what):
        if getattr(self, "_split", False):
            raise RuntimeError("the %s calls are blocking: the sequence is in split-phase mode" % what)

    def mosaic(self, first, inv_warps, usable, ox, oy, Hc, Wc, fill=0, cull=True):
        """The background sprite of frames first .. first+count-1 under inv_warps float64[count, 8] on the Hc x Wc canvas with
        origin (ox, oy) (gme_seq_mosaic; ``usable`` uint8[count] or None), kept in the sequence: read_mosaic reads it."""
        self._blocking("mosaic")
        g = np.ascontiguousarray(np.asarray(inv_warps, dtype=np.float64).reshape(-1, 8))
        use = None if usable is None else np.ascontiguousarray(np.asarray(usable).reshape(len(g)) != 0, dtype=np.uint8)
        self._mosaic_shape = None
        _check(self.lib.gme_seq_mosaic(self.handle, int(first), len(g), _p(g, _c_f64p), None if use is None else _p(use, _c_u8p),
                                       int(ox), int(oy), int(Hc), int(Wc), int(fill), int(bool(cull))), self.lib)
        self._mosaic_shape = (int(Hc), int(Wc))

    def read_mosaic(self):
        """(sprite uint8[Hc, Wc], count uint16[Hc, Wc]) of the last mosaic()."""
        shape = getattr(self, "_mosaic_shape", None) or (1, 1)     # without a mosaic the library refuses before it writes
        sprite, count = np.empty(shape, np.uint8), np.empty(shape, np.uint16)
        _check(self.lib.gme_seq_read_mosaic(self.handle, _p(sprite, _c_u8p), _p(count, _c_u16p)), self.lib)
        return sprite, count

    def moving_masks(self, first, warps, usable, ox, oy, threshold=16, min_count=3):
        """Masks of frames first .. first+count-1 against the sequence's mosaic under warps float64[count, 8]
        (gme_seq_moving_masks) -> (known int64[count], moving int64[count]); read_masks_range reads the masks."""
        self._blocking("mosaic")
        a = np.ascontiguousarray(np.asarray(warps, dtype=np.float64).reshape(-1, 8))
        use = None if usable is None else np.ascontiguousarray(np.asarray(usable).reshape(len(a)) != 0, dtype=np.uint8)
        known, moving = np.zeros(len(a), np.int64), np.zeros(len(a), np.int64)
        _check(self.lib.gme_seq_moving_masks(self.handle, int(first), len(a), _p(a, _c_f64p), None if use is None else _p(use, _c_u8p),
                                             int(ox), int(oy), int(threshold), int(min_count), _p(known, _c_i64p),
                                             _p(moving, _c_i64p)), self.lib)
        return known, moving

    def read_masks_range(self, first, count):
        """Masks (0 / 1) of frames first .. first+count-1 -> uint8[count, H, W] with one wait."""
        out = np.empty((int(count), self.H, self.W), dtype=np.uint8)
        _check(self.lib.gme_seq_read_masks_range(self.handle, int(first), int(count), _p(out, _c_u8p)), self.lib)
        return out

    # ---- quarter-pel block matching (bbme_subpel.hip, subpel.py)
    def subpel(self, frame_distance, block_size, pnorm, levels=2):
        """Refine the field of the last bbme() (same frame distance and block size) to half (levels 1) or quarter pixels (2)
        on the device (gme_seq_subpel); read_qmv reads the result, compensate_qpel compensates with it."""
        self._blocking("sub-pel")
        _check(self.lib.gme_seq_subpel(self.handle, int(frame_distance), _block_size(block_size), int(pnorm), _subpel_levels(levels)),
               self.lib)

    def read_qmv(self, first=0, count=None):
        """(qfield int32[count, h, w, 2] in quarter pixels, cost int64[count, h, w]) of pairs first .. first+count-1 of the
        last subpel()."""
        shape = getattr(self, "_mv_shape", (0, 0, 0, 2))
        count = shape[0] - first if count is None else count
        q, cost = np.empty((max(count, 0),) + tuple(shape[1:]), np.int32), np.empty((max(count, 0),) + tuple(shape[1:3]), np.int64)
        _check(self.lib.gme_seq_read_qmv(self.handle, int(first), int(count), _p(q, _c_i32p), _p(cost, _c_i64p)), self.lib)
        return q, cost

    def compensate_qpel(self, frame_distance, block_size):
        """Compensated frames of the refined field (gme_seq_compensate_qpel, subpel.compensate) -> sse int64[P] against the
        current frames; read_compensated(_range) reads the frames."""
        self._blocking("sub-pel")
        sse = np.zeros(max(getattr(self, "_mv_shape", (0,))[0], 1), np.int64)
        _check(self.lib.gme_seq_compensate_qpel(self.handle, int(frame_distance), _block_size(block_size), _p(sse, _c_i64p)), self.lib)
        return sse[:getattr(self, "_mv_shape", (0,))[0]]

    # ---- hierarchical block matching (bbme_hier.hip, hier.py)
    def hier(self, frame_distance, block_size=16, coarse_window=8, radius=1, pnorm=0, levels=3):
        """hier.search for every pair on the device (gme_seq_hier).  The level-2 field becomes the sequence's motion field:
        read_mv, subpel, read_qmv and compensate_qpel work on it as after bbme(); read_hier reads any level with its costs."""
        self._blocking("hierarchical search")
        block_size, coarse_window, radius, pnorm, levels = _hier_args(block_size, coarse_window, radius, pnorm, levels)
        _check(self.lib.gme_seq_hier(self.handle, int(frame_distance), block_size, coarse_window, radius, pnorm, levels), self.lib)
        self._mv_shape = (self.N - int(frame_distance), self.H // block_size, self.W // block_size, 2)

    def read_hier(self, level=2, first=0, count=None):
        """(field int32[count, h, w, 2], cost int64[count, h, w]) of pairs first .. first+count-1 at pyramid level ``level`` of
        the last hier(); a level it did not use is an IndexError."""
        shape = getattr(self, "_mv_shape", (0, 0, 0, 2))
        count = shape[0] - first if count is None else count
        mf, cost = np.empty((max(count, 0),) + tuple(shape[1:]), np.int32), np.empty((max(count, 0),) + tuple(shape[1:3]), np.int64)
        _check(self.lib.gme_seq_read_hier(self.handle, int(level), int(first), int(count), _p(mf, _c_i32p), _p(cost, _c_i64p)), self.lib)
        return mf, cost

    # ---- variable-block-size motion (bbme_vbs.hip, vbs.py)
    def vbs(self, frame_distance, block_size=16, depth=2, radius=1, pnorm=0, penalty=0):
        """vbs.tree on the field of the last bbme() or hier() (same frame distance and block size) for every pair on the device
        (gme_seq_vbs).  The motion field stays what it was; read_vbs reads the result, compensate_vbs compensates with it."""
        self._blocking("variable-block-size tree")
        block_size, depth, radius, pnorm, penalty = _vbs_args(block_size, depth, radius, pnorm, penalty)
        _check(self.lib.gme_seq_vbs(self.handle, int(frame_distance), block_size, depth, radius, pnorm, penalty), self.lib)
        self._vbs_depth = depth

    def read_vbs(self, first=0, count=None):
        """(leaf int32[count, h << D, w << D, 2], depth uint8[count, h << D, w << D], cost int64[count, h, w]) of pairs
        first .. first+count-1 of the last vbs()."""
        shape, D = getattr(self, "_mv_shape", (0, 0, 0, 2)), getattr(self, "_vbs_depth", 0)
        count = shape[0] - first if count is None else count
        grid = (max(count, 0), shape[1] << D, shape[2] << D)
        leaf, dmap = np.empty(grid + (2,), np.int32), np.empty(grid, np.uint8)
        cost = np.empty((max(count, 0),) + tuple(shape[1:3]), np.int64)
        _check(self.lib.gme_seq_read_vbs(self.handle, int(first), int(count), _p(leaf, _c_i32p), _p(dmap, _c_u8p), _p(cost, _c_i64p)),
               self.lib)
        return leaf, dmap, cost

    def compensate_vbs(self, frame_distance, block_size):
        """Compensated frames of the leaf field (gme_seq_compensate_vbs, subpel.compensate_integer at the leaf size) -> sse
        int64[P] against the current frames; read_compensated(_range) reads the frames."""
        self._blocking("variable-block-size tree")
        sse = np.zeros(max(getattr(self, "_mv_shape", (0,))[0], 1), np.int64)
        _check(self.lib.gme_seq_compensate_vbs(self.handle, int(frame_distance), _block_size(block_size), _p(sse, _c_i64p)), self.lib)
        return sse[:getattr(self, "_mv_shape", (0,))[0]]

    # ---- bidirectional block prediction (bbme_bipred.hip, bipred.py)
    def bipred(self, frame_distance, block_size=16, search_window=16, procedure=0, pnorm=0, radius=1, rounds=1, penalty=0):
        """bipred.decide for the targets t = fd .. N-1-fd on the device (gme_seq_bipred): both searches from every target (into
        frame t-fd and into frame t+fd, the arguments of bbme()) and the decision.  The motion field and what was derived from it
        stay what they were; read_bipred reads the result, predict_bipred predicts with it."""
        self._blocking("bidirectional prediction")
        block_size, radius, rounds, pnorm, penalty = _bipred_args(block_size, radius, rounds, pnorm, penalty)
        fd = int(frame_distance)
        _check(self.lib.gme_seq_bipred(self.handle, fd, block_size, int(search_window), int(procedure), pnorm, radius, rounds, penalty),
               self.lib)
        self._bipred_shape = (self.N - 2 * fd, self.H // block_size, self.W // block_size)

    def read_bipred(self, first=0, count=None):
        """(f0, f1 int32[count, h, w, 2], mode uint8[count, h, w], v0, v1 int32[count, h, w, 2], cost int64[count, h, w], costs
        int64[count, h, w, 3]) of targets first .. first+count-1 of the last bipred()."""
        shape = getattr(self, "_bipred_shape", None) or (0, 0, 0)
        count = shape[0] - first if count is None else count
        grid = (max(count, 0),) + tuple(shape[1:])
        f0, f1, v0, v1 = (np.empty(grid + (2,), np.int32) for _ in range(4))
        mode, cost, costs = np.empty(grid, np.uint8), np.empty(grid, np.int64), np.empty(grid + (3,), np.int64)
        _check(self.lib.gme_seq_read_bipred(self.handle, int(first), int(count), _p(f0, _c_i32p), _p(f1, _c_i32p), _p(mode, _c_u8p),
                                            _p(v0, _c_i32p), _p(v1, _c_i32p), _p(cost, _c_i64p), _p(costs, _c_i64p)), self.lib)
        return f0, f1, mode, v0, v1, cost, costs

    def predict_bipred(self):
        """The predicted frames of the last bipred() (gme_seq_predict_bipred, bipred.predict) -> sse int64[T] against the target
        frames; read_compensated_range(0, T) reads the frames."""
        self._blocking("bidirectional prediction")
        T = (getattr(self, "_bipred_shape", None) or (0,))[0]
        sse = np.zeros(max(T, 1), np.int64)
        _check(self.lib.gme_seq_predict_bipred(self.handle, _p(sse, _c_i64p)), self.lib)
        return sse[:T]

    # ---- global motion compensation (bbme_gmc.hip, gmc.py)
    def gmc(self, frame_distance, h, block_size=16, search_window=16, procedure=0, pnorm=0, penalty=0):
        """gmc.decide for the pairs k = 0 .. N-1-fd on the device (gme_seq_gmc): frame k+fd is predicted from frame k under the
        warp h[k] (float64[P, 8], the pairs of refine_projective); the search (frame k+fd looked for in frame k, the arguments of
        bbme()) and the decision.  The motion field and what was derived from it stay what they were; read_gmc reads the result,
        predict_gmc predicts with it."""
        self._blocking("global motion compensation")
        block_size, pnorm, penalty = _gmc_args(block_size, pnorm, penalty)
        fd = int(frame_distance)
        pairs = self.N - fd
        if pairs < 0:
            raise IndexError("frame_distance %d needs at least %d frames" % (fd, fd + 1))
        warps = np.ascontiguousarray(np.asarray(h, dtype=np.float64).reshape(pairs, 8))
        _check(self.lib.gme_seq_gmc(self.handle, fd, block_size, int(search_window), int(procedure), pnorm, penalty, _p(warps, _c_f64p)),
               self.lib)
        self._gmc_shape = (pairs, self.H // block_size, self.W // block_size)

    def read_gmc(self, first=0, count=None):
        """(f int32[count, h, w, 2], mode uint8[count, h, w], cost int64[count, h, w], costs int64[count, h, w, 2], usable
        uint8[count]) of pairs first .. first+count-1 of the last gmc()."""
        shape = getattr(self, "_gmc_shape", None) or (0, 0, 0)
        count = shape[0] - first if count is None else count
        grid = (max(count, 0),) + tuple(shape[1:])
        f, mode, cost, costs = np.empty(grid + (2,), np.int32), np.empty(grid, np.uint8), np.empty(grid, np.int64), np.empty(grid + (2,), np.int64)
        usable = np.empty(max(count, 0), np.uint8)
        _check(self.lib.gme_seq_read_gmc(self.handle, int(first), int(count), _p(f, _c_i32p), _p(mode, _c_u8p), _p(cost, _c_i64p),
                                         _p(costs, _c_i64p), _p(usable, _c_u8p)), self.lib)
        return f, mode, cost, costs, usable

    def predict_gmc(self):
        """The predicted frames of the last gmc() (gme_seq_predict_gmc, gmc.predict) -> sse int64[P] against the frames they
        predict; read_compensated_range(0, P) reads the frames."""
        self._blocking("global motion compensation")
        P = (getattr(self, "_gmc_shape", None) or (0,))[0]
        sse = np.zeros(max(P, 1), np.int64)
        _check(self.lib.gme_seq_predict_gmc(self.handle, _p(sse, _c_i64p)), self.lib)
        return sse[:P]

    # ---- vector propagation search (bbme_prop.hip, propagate.py)
    def prop(self, frame_distance, block_size=16, pnorm=0, rounds=2, steps=1, temporal=True, g=None):
        """propagate.search on the field of the last bbme(), hier() or prop() (same frame distance and block size) for every pair
        on the device (gme_seq_prop).  With ``temporal``, pair k >= 1 also scores the prior field of pair k - 1; ``g`` is the camera
        field int32[P, h, w, 2] or None.  The result becomes the sequence's motion field: read_mv, subpel, vbs and a further prop()
        work on it; read_prop reads it with its costs and sources."""
        self._blocking("vector propagation")
        block_size, pnorm, rounds, steps = _prop_args(block_size, pnorm, rounds, steps)
        if g is not None:
            g = _prop_field(g, "g", tuple(getattr(self, "_mv_shape", (0, 0, 0, 2))[:3]))
        _check(self.lib.gme_seq_prop(self.handle, int(frame_distance), block_size, pnorm, rounds, steps, int(bool(temporal)),
                                     None if g is None else _p(g, _c_i32p)), self.lib)

    def read_prop(self, first=0, count=None):
        """(mf int32[count, h, w, 2], cost int64[count, h, w], source uint8[count, h, w]) of pairs first .. first+count-1 of the
        last prop()."""
        shape = getattr(self, "_mv_shape", (0, 0, 0, 2))
        count = shape[0] - first if count is None else count
        grid = (max(count, 0),) + tuple(shape[1:3])
        mf, cost, source = np.empty(grid + (2,), np.int32), np.empty(grid, np.int64), np.empty(grid, np.uint8)
        _check(self.lib.gme_seq_read_prop(self.handle, int(first), int(count), _p(mf, _c_i32p), _p(cost, _c_i64p), _p(source, _c_u8p)),
               self.lib)
        return mf, cost, source

    # ---- motion-compensated frame interpolation (bbme_interp.hip, interp.py)
    def interp(self, frame_distance, block_size=16, search_window=8, pnorm=0, bias=0, first=0, count=None):
        """The frames halfway between frame k and frame k + fd for the pairs k = first .. first+count-1 (gme_seq_interp,
        interp.search and interp.interpolate) -> (mv int32[count, h, w, 2], cost int64[count, h, w], dist int64[count, h, w], frames
        uint8[count, H, W], sse int64[count]): ``sse`` is the squared error against frame k + fd / 2 for an even fd, -1 for an odd
        one.  One blocking call, also in split-phase mode, that keeps nothing and leaves everything the sequence holds as it was.
        Too few frames for the distance or a range outside the pairs is an IndexError."""
        fd = int(frame_distance)
        block_size, search_window, pnorm, bias = _interp_args(block_size, search_window, pnorm, bias, self.H, self.W)
        first = int(first)
        count = self.N - fd - first if count is None else int(count)
        n = max(count, 0)                      # a refused range writes nothing
        grid = (n, self.H // block_size, self.W // block_size)
        mv, cost, dist = np.zeros(grid + (2,), np.int32), np.zeros(grid, np.int64), np.zeros(grid, np.int64)
        frames, sse = np.empty((n, self.H, self.W), np.uint8), np.zeros(max(n, 1), np.int64)
        _check(self.lib.gme_seq_interp(self.handle, fd, block_size, search_window, pnorm, bias, first, count, _p(mv, _c_i32p),
                                       _p(cost, _c_i64p), _p(dist, _c_i64p), _p(frames, _c_u8p), _p(sse, _c_i64p)), self.lib)
        return mv, cost, dist, frames, sse[:n]

    # ---- overlapped block motion compensation (bbme_obmc.hip, obmc.py)
    def obmc(self, frame_distance, block_size, quarter=False, first=0, count=None):
        """Frame k compensated with overlapped blocks for the pairs k = first .. first+count-1 (gme_seq_obmc, obmc.compensate) ->
        (frames uint8[count, H, W], sse int64[count]) by the sequence's motion field, or with ``quarter`` by its quarter-pel field;
        ``sse`` is the squared error against frame k + fd.  One blocking call, also in split-phase mode, that keeps nothing and
        leaves everything the sequence holds as it was.  A range outside the field's pairs is an IndexError."""
        import obmc
        fd = int(frame_distance)
        block_size = obmc.check_block_size(block_size)
        obmc.check_shape(self.H, self.W, block_size)
        first = int(first)
        count = self.N - fd - first if count is None else int(count)
        n = max(count, 0)                      # a refused range writes nothing
        frames, sse = np.empty((n, self.H, self.W), np.uint8), np.zeros(max(n, 1), np.int64)
        _check(self.lib.gme_seq_obmc(self.handle, fd, block_size, 1 if quarter else 4, first, count, _p(frames, _c_u8p),
                                     _p(sse, _c_i64p)), self.lib)
        return frames, sse[:n]


    # ---- motion-compensated temporal denoising (bbme_denoise.hip, denoise.py)
    def denoise(self, frame_distance, block_size=16, search_window=8, procedure=0, pnorm=0, radius=1, levels=0, strength=24, first=0,
                count=None):
        """The interior targets t = radius fd + first + k, k < count, each filtered with its 2 radius references t -+ d fd
        (gme_seq_denoise, denoise.frame over searches from the target) -> (frames uint8[count, H, W], change int64[count]);
        ``change`` is the squared difference between the filtered frame and the target.  One blocking call, also in split-phase
        mode, that keeps nothing and leaves everything the sequence holds as it was.  A range outside the interior targets is an
        IndexError.  The default strength is a convention of the tool, not a tuned value."""
        import denoise
        import obmc
        fd, radius = int(frame_distance), denoise.check_radius(radius)
        _, strength = denoise.check_args(2 * radius, strength)
        block_size = obmc.check_block_size(block_size)
        obmc.check_shape(self.H, self.W, block_size)
        first = int(first)
        count = self.N - 2 * radius * fd - first if count is None else int(count)
        n = max(count, 0)                      # a refused range writes nothing
        frames, change = np.empty((n, self.H, self.W), np.uint8), np.zeros(max(n, 1), np.int64)
        _check(self.lib.gme_seq_denoise(self.handle, fd, block_size, int(search_window), int(procedure), int(pnorm), radius, int(levels),
                                        strength, first, count, _p(frames, _c_u8p), _p(change, _c_i64p)), self.lib)
        return frames, change[:n]


_default = None
_default_lock = threading.Lock()


def default_context():
    """Process-wide context used by the module-level functions of bbme/motion/utils."""
    global _default
    with _default_lock:
        if _default is None:
            _default = Context()
        return _default
