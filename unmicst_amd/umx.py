"""ctypes binding of libumx.so (include/umx.h) -- the thin shim between Python and the HIP engine.

There is deliberately no fallback: if the shared library is missing or no gfx950 device is present the calls
raise, they never route to a CPU path.
"""
from __future__ import annotations

import ctypes
import math
import os
from typing import List, Optional

import numpy as np

from . import build as _build
from .model import HParams

UMX_OK = 0
PREC_DEFAULT, PREC_F32, PREC_F16X3, PREC_F16X3_F6 = 0, 1, 2, 3      # enum umx_precision
PRECISIONS = {"default": PREC_DEFAULT, "f32": PREC_F32, "f16x3": PREC_F16X3, "f16f6": PREC_F16X3_F6}
ERR_INVALID, ERR_HIP = 1, 4   # UMX_ERR_INVALID, UMX_ERR_HIP
ERR_RANGE = 6   # UMX_ERR_RANGE
ERR_GUARD = 7   # UMX_ERR_GUARD (debug guard mode, UMX_DEBUG_GUARD: a red zone round a device buffer was written)
MODE_ACCUMULATE, MODE_REPLACE = 0, 1
STITCH_FP16_COMPAT, STITCH_FP32 = 0, 1

# every symbol include/umx.h declares (checked by tests/test_abi.py)
EXPORTS = [
    "umx_device_count", "umx_device_mem_info", "umx_create", "umx_create_opts", "umx_precision_of", "umx_destroy", "umx_last_error", "umx_set_stream", "umx_synchronize",
    "umx_forward_tiles", "umx_forward_tiles_dev", "umx_tile_grid", "umx_infer_image", "umx_infer_image_dev",
    "umx_infer_image_raw", "umx_infer_image_raw_range", "umx_plane_range", "umx_infer_image_raw_scaled", "umx_infer_image_raw_outlier", "umx_infer_image_raw_submit", "umx_infer_image_wait", "umx_tiff_lzw_decode",
    "umx_tiff_packbits_decode", "umx_shard_unique_id", "umx_shard_init", "umx_shard_init_transport", "umx_shard_fini", "umx_shard_plan",
    "umx_infer_image_sharded_dev", "umx_infer_image_sharded_raw", "umx_infer_image_sharded_raw_submit",
    "umx_band_tiles_dev", "umx_stitch_dev", "umx_profile_enable", "umx_profile_read", "umx_prof_entry_size", "umx_test_double_to_half", "umx_test_double_to_half_dev",
    "umx_test_gauss_weights", "umx_test_resize_dev", "umx_test_rescale_dev", "umx_test_plane_range_dev", "umx_test_half_to_u8_dev",
    "umx_describe", "umx_describe_graph", "umx_plan_check", "umx_test_infer_plan", "umx_test_wgrad_plan", "umx_test_train_plan", "umx_test_step_plan", "umx_test_slide_plan", "umx_test_band_plan", "umx_test_mx_pack_e2m3", "umx_version",
    "umx_label_options_check", "umx_labeler_create", "umx_labeler_destroy", "umx_labeler_last_error", "umx_labeler_run",
    "umx_labeler_run_dev", "umx_labeler_objects", "umx_labeler_last_ms",
    "umx_label_measure_check", "umx_labeler_measure", "umx_labeler_measure_dev", "umx_labeler_measure_last_ms",
    "umx_label_split_check", "umx_labeler_run_split", "umx_labeler_run_split_dev",
    "umx_label_flood_check", "umx_labeler_run_flood", "umx_labeler_run_flood_dev",
    "umx_label_hmax_check", "umx_labeler_run_hmax", "umx_labeler_run_hmax_dev",
    "umx_label_shape_check", "umx_labeler_shape", "umx_labeler_shape_dev", "umx_labeler_shape_last_ms",
    "umx_label_contact_check", "umx_labeler_contacts", "umx_labeler_contacts_dev", "umx_labeler_contacts_last_ms",
    "umx_labeler_contacts_last_stats",
    "umx_label_hull_check", "umx_labeler_hull", "umx_labeler_hull_dev", "umx_labeler_hull_last_ms",
    "umx_label_relabel_check", "umx_label_relabel_map", "umx_labeler_relabel", "umx_labeler_relabel_dev", "umx_labeler_relabel_last_ms",
]

# the label mask's limits and the geometry of its kernels (the UMX_LABEL_* macros of include/umx.h; tests/test_label_cpu.py compares)
LABEL_MAX_CLASSES, LABEL_MAX_MIN_AREA = 16, 65536
LABEL_STRIP_ROWS, LABEL_THREADS, LABEL_SCAN_BLOCK = 32, 1024, 2048
# the growth: its largest radius, the tile a workgroup owns and the halo it loads round it (= the levels one launch advances)
LABEL_MAX_GROW, LABEL_GROW_TILE, LABEL_GROW_HALO = 255, 64, 8
# the split at the necks: its largest depth, core area and regrow bound (the UMX_SPLIT_* enumerators; tests/test_label_split_cpu.py compares)
SPLIT_MAX_DEPTH, SPLIT_MAX_CORE_AREA, SPLIT_MAX_REGROW = 8, 65536, 255
# the level flood: its largest and its default level step, the steps of one launch (the UMX_FLOOD_* enumerators; tests/test_label_flood_cpu.py compares)
FLOOD_MAX_STEP, FLOOD_DEFAULT_STEP, FLOOD_LAUNCH_STEPS = 256, 16, 8
# the h-maxima seeds: the largest height, the steps of one reconstruction launch, the launches one reconstruction may take (the
# UMX_HMAX_* enumerators; tests/test_label_hmax_cpu.py compares)
HMAX_MAX_HEIGHT, HMAX_LAUNCH_STEPS, HMAX_MAX_LAUNCHES = 255, 64, 2048


class UmxError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__("libumx error %d: %s" % (code, msg))
        self.code = code


class _HP(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in
                ("graph", "imSize", "nChannels", "nClasses", "nOut0", "nLayers", "ks", "nExtraConvs", "featMapsFact")]


class _Options(ctypes.Structure):
    _fields_ = [("device_ordinal", ctypes.c_int32), ("max_batch", ctypes.c_int32), ("precision", ctypes.c_int32),
                ("act_shift", ctypes.c_int32), ("lanes", ctypes.c_int32), ("reserved", ctypes.c_int32 * 11)]


class ProfEntry(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char * 48), ("kernel", ctypes.c_char * 64), ("launches", ctypes.c_int64),
                ("total_ms", ctypes.c_double), ("flops", ctypes.c_double), ("bytes", ctypes.c_double),
                ("exec_flops", ctypes.c_double), ("launches_seen", ctypes.c_int64), ("xcd_order", ctypes.c_int32),
                ("reserved", ctypes.c_int32)]


class _LabelGrow(ctypes.Structure):
    _fields_ = [("grow_radius", ctypes.c_int32), ("grow_classes", ctypes.c_uint32)]


class _LabelTail(ctypes.Union):
    """the six words after min_area as the header names them (two growth words, four reserved ones) and, as before the growth
    existed, as six words by index: reserved[0] and [1] are grow_radius and grow_classes, reserved[2..5] the header's reserved[0..3]"""
    _anonymous_ = ("grow",)
    _fields_ = [("grow", _LabelGrow), ("reserved", ctypes.c_int32 * 6)]


class _LabelOptions(ctypes.Structure):
    """umx_label_options: 32 bytes"""
    _anonymous_ = ("tail",)
    _fields_ = [("cls", ctypes.c_int32), ("min_area", ctypes.c_int32), ("tail", _LabelTail)]


class _LabelSplitOptions(ctypes.Structure):
    """umx_label_split_options: 64 bytes"""
    _fields_ = [("base", _LabelOptions), ("depth", ctypes.c_int32), ("core_min_area", ctypes.c_int32), ("regrow", ctypes.c_int32),
                ("reserved", ctypes.c_int32 * 5)]


class _LabelSplitCounts(ctypes.Structure):
    """umx_label_split_counts: 32 bytes"""
    _fields_ = [(n, ctypes.c_int64) for n in ("n_objects", "n_before", "n_cored", "unreached")]


class _LabelFloodOptions(ctypes.Structure):
    """umx_label_flood_options: 96 bytes"""
    _fields_ = [("split", _LabelSplitOptions), ("relief_plane", ctypes.c_int32), ("invert", ctypes.c_int32), ("level_step", ctypes.c_int32),
                ("reserved", ctypes.c_int32 * 5)]


class _LabelFloodCounts(ctypes.Structure):
    """umx_label_flood_counts: 64 bytes"""
    _fields_ = [(n, ctypes.c_int64) for n in ("n_objects", "n_before", "n_cored", "unreached", "levels_claimed", "claimed", "launches",
                                              "reserved")]


class _LabelHmaxOptions(ctypes.Structure):
    """umx_label_hmax_options: 128 bytes"""
    _fields_ = [("flood", _LabelFloodOptions), ("seed_plane", ctypes.c_int32), ("seed_invert", ctypes.c_int32), ("height", ctypes.c_int32),
                ("reserved", ctypes.c_int32 * 5)]


class _LabelHmaxCounts(ctypes.Structure):
    """umx_label_hmax_counts: 96 bytes"""
    _fields_ = [("flood", _LabelFloodCounts), ("seed_pixels", ctypes.c_int64), ("recon_launches", ctypes.c_int64 * 2), ("reserved", ctypes.c_int64)]


class LabelObject(ctypes.Structure):
    """umx_label_object: 40 bytes"""
    _fields_ = [(n, ctypes.c_int32) for n in ("area", "y0", "x0", "y1", "x1", "reserved")] + [("sum_y", ctypes.c_int64), ("sum_x", ctypes.c_int64)]


# the same record as a numpy dtype: what Labeler.run returns its table in
LABEL_OBJECT_DTYPE = np.dtype([(n, "<i4") for n in ("area", "y0", "x0", "y1", "x1", "reserved")] + [("sum_y", "<i8"), ("sum_x", "<i8")])


# umx_label_measure (32 bytes): what Labeler.measure returns, [C, N]; mean and std are measure_mean_std's
LABEL_MEASURE_DTYPE = np.dtype([("sum", "<u8"), ("sum_sq", "<u8"), ("min", "<u4"), ("max", "<u4"), ("count", "<u4"), ("reserved", "<u4")])
MEASURE_U8, MEASURE_U16 = 1, 2                                 # UMX_MEASURE_*
LABEL_MEASURE_GROUP, LABEL_MAX_MEASURE_PLANES = 4, 1024
_MEASURE_DTYPES = {np.dtype(np.uint8): MEASURE_U8, np.dtype(np.uint16): MEASURE_U16}


class LabelShape(ctypes.Structure):
    """umx_label_shape: 64 bytes"""
    _fields_ = [(n, ctypes.c_int64) for n in ("sum_y", "sum_x", "sum_yy", "sum_xy", "sum_xx")] + \
               [(n, ctypes.c_uint32) for n in ("q1", "q2", "qd", "q3", "q4", "reserved")]


# the same record as a numpy dtype: what Labeler.shape returns, [N]; the descriptors are shape_descriptors'
LABEL_SHAPE_DTYPE = np.dtype([(n, "<i8") for n in ("sum_y", "sum_x", "sum_yy", "sum_xy", "sum_xx")] +
                             [(n, "<u4") for n in ("q1", "q2", "qd", "q3", "q4", "reserved")])
SHAPE_MAX_SIDE = 65536                                         # UMX_SHAPE_MAX_SIDE


class LabelContact(ctypes.Structure):
    """umx_label_contact: 16 bytes"""
    _fields_ = [("a", ctypes.c_int32), ("b", ctypes.c_int32), ("edges", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class _LabelContactStats(ctypes.Structure):
    """umx_label_contact_stats: 32 bytes"""
    _fields_ = [("table_capacity", ctypes.c_int64), ("reruns", ctypes.c_int64), ("longest_row", ctypes.c_int64),
                ("ordered_by", ctypes.c_int32), ("reserved", ctypes.c_int32)]


# the same record as a numpy dtype: what Labeler.contacts returns, [M], sorted by (a, b)
LABEL_CONTACT_DTYPE = np.dtype([("a", "<i4"), ("b", "<i4"), ("edges", "<u4"), ("reserved", "<u4")])
# the UMX_CONTACT_* macros of include/umx.h (tests/test_label_contacts_cpu.py compares)
CONTACT_MAX_REACH, CONTACT_TABLE_MIN, CONTACT_TABLE_MAX, CONTACT_PROBE_MAX, CONTACT_DEVICE_SORT_MAX = 255, 65536, 268435456, 1024, 1024
CONTACT_ORDER_NONE, CONTACT_ORDER_DEVICE, CONTACT_ORDER_HOST = 0, 1, 2


class LabelHull(ctypes.Structure):
    """umx_label_hull: 32 bytes"""
    _fields_ = [("area2", ctypes.c_int64), ("feret_max_sq", ctypes.c_int64), ("first", ctypes.c_int64), ("n_vertices", ctypes.c_int32),
                ("rows", ctypes.c_int32)]


class LabelHullVertex(ctypes.Structure):
    """umx_label_hull_vertex: 8 bytes"""
    _fields_ = [("y", ctypes.c_int32), ("x", ctypes.c_int32)]


# the same records as numpy dtypes: what Labeler.hull returns, [N] and [V]; the descriptors are hull_descriptors'
LABEL_HULL_DTYPE = np.dtype([("area2", "<i8"), ("feret_max_sq", "<i8"), ("first", "<i8"), ("n_vertices", "<i4"), ("rows", "<i4")])
LABEL_HULL_VERTEX_DTYPE = np.dtype([("y", "<i4"), ("x", "<i4")])
HULL_MAX_SIDE, HULL_MAX_ROWS = 65536, 268435456                # UMX_HULL_* (tests/test_label_hull_cpu.py compares)
RELABEL_MAX_PAIRS = 268435456                                  # UMX_RELABEL_MAX_PAIRS (tests/test_label_relabel_cpu.py compares)


_SEND_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p)
_GATHER_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p)
_GROUP_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p)


class ShardTransport(ctypes.Structure):
    """umx_shard_transport (include/umx.h): the inter-rank operations of umx_infer_image_sharded_dev as a table of callbacks."""
    _fields_ = [("user", ctypes.c_void_p), ("send", _SEND_FN), ("recv", _SEND_FN), ("all_gather", _GATHER_FN),
                ("group_start", _GROUP_FN), ("group_end", _GROUP_FN)]


_lib = None
hip_runtime = None      # path of the libamdhip64 libumx was bound to (set by load())


def _torch_hip_runtime() -> Optional[str]:
    """Path of the libamdhip64 PyTorch bundles, WITHOUT importing torch (find_spec only locates the package)."""
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        return None
    if spec is None or not spec.origin:
        return None
    cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    return cand if os.path.exists(cand) else None


def _bind_hip_runtime() -> str:
    """Make exactly one HIP runtime (libamdhip64) global in this process before libumx is dlopen'ed.

    libumx.so is linked without a HIP runtime dependency.  PyTorch wheels bundle their own libamdhip64 +
    libhsa-runtime64; a second copy (e.g. /opt/rocm's) initialised in the same process leaves one of the two
    without a GPU.  Policy (UMX_HIP_RUNTIME = auto | torch | system, default auto):
      auto    PyTorch's copy whenever a PyTorch with a bundled runtime is INSTALLED (located with find_spec and dlopen'ed
              directly: torch itself is not imported, so the choice does not depend on import order and costs nothing) --
              a later `import torch` in the process (sharding.py, the trainer's helpers, the oracles) then finds the very
              runtime libumx already uses; the system ROCm runtime otherwise.
      system  the system ROCm runtime.  The per-file command-line tools ask for it (driver.main: they never import torch, and
              the system runtime initialises 0.1 s faster); mixing it with a later `import torch` is refused by
              require_torch_runtime().
      torch   import torch first (as rounds 1-4 did under the tests), then bind its copy.
    """
    import sys
    mode = os.environ.get("UMX_HIP_RUNTIME", "auto")
    if mode not in ("auto", "torch", "system"):
        raise ValueError("UMX_HIP_RUNTIME must be auto, torch or system (got %r)" % mode)
    if mode == "torch":
        import torch  # noqa: F401  (loads its bundled libamdhip64.so)
    if mode in ("auto", "torch"):
        cand = _torch_hip_runtime()
        if cand is not None:
            ctypes.CDLL(cand, mode=ctypes.RTLD_GLOBAL)
            return cand
        if "torch" in sys.modules and mode == "torch":
            raise OSError("UMX_HIP_RUNTIME=torch: this PyTorch bundles no libamdhip64")
    for cand in (os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"), "libamdhip64.so.7",
                 "libamdhip64.so"):
        try:
            ctypes.CDLL(cand, mode=ctypes.RTLD_GLOBAL)
            return cand
        except OSError:
            continue
    raise OSError("no HIP runtime (libamdhip64) found; libumx has no CPU fallback")


def require_torch_runtime(who: str) -> None:
    """Called by the torch-facing helpers (unmicst_amd/sharding.py, bench.py) before they hand torch tensors to libumx:
    refuses to run when libumx is bound to another HIP runtime than the one PyTorch brings -- two runtimes in one process and
    one of them loses the GPU (the symptom is hipErrorNoDevice or a hang far from the cause)."""
    load()
    want = _torch_hip_runtime()
    if want is not None and hip_runtime is not None and os.path.realpath(want) != os.path.realpath(hip_runtime):
        raise RuntimeError("%s needs libumx and PyTorch on ONE HIP runtime, but libumx is bound to %s and PyTorch brings %s "
                           "(UMX_HIP_RUNTIME=%s): leave UMX_HIP_RUNTIME unset (auto) in processes that import torch"
                           % (who, hip_runtime, want, os.environ.get("UMX_HIP_RUNTIME", "auto")))


def load(path: Optional[str] = None):
    """dlopen libumx.so (built in-tree by unmicst_amd.build); raises if it is missing."""
    global _lib, hip_runtime
    if _lib is not None:
        return _lib
    path = path or os.environ.get("UMX_LIB") or _build.lib_path()   # UMX_LIB: an alternative build (kernel experiments)
    if not os.path.exists(path):
        raise FileNotFoundError("%s not found: run `python -c 'import __graft_entry__ as g; g.build()'` "
                                "(libumx has no CPU fallback)" % path)
    hip_runtime = _bind_hip_runtime()
    L = ctypes.CDLL(path)
    c_int, c_void_p, c_double = ctypes.c_int, ctypes.c_void_p, ctypes.c_double
    ip = ctypes.POINTER(c_int)
    L.umx_device_count.restype = c_int
    L.umx_device_mem_info.restype = c_int
    L.umx_device_mem_info.argtypes = [c_int, ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_size_t)]
    L.umx_create.restype = c_int
    L.umx_create.argtypes = [ctypes.POINTER(_HP), c_void_p, ctypes.c_size_t, c_int, c_int, ctypes.POINTER(c_void_p)]
    L.umx_create_opts.restype = c_int
    L.umx_create_opts.argtypes = [ctypes.POINTER(_HP), c_void_p, ctypes.c_size_t, ctypes.POINTER(_Options),
                                  ctypes.POINTER(c_void_p)]
    L.umx_precision_of.restype = c_int
    L.umx_precision_of.argtypes = [c_void_p]
    L.umx_destroy.restype = None
    L.umx_destroy.argtypes = [c_void_p]
    L.umx_last_error.restype = ctypes.c_char_p
    L.umx_last_error.argtypes = [c_void_p]
    L.umx_set_stream.argtypes = [c_void_p, c_void_p]
    L.umx_synchronize.argtypes = [c_void_p]
    L.umx_forward_tiles.argtypes = [c_void_p, c_void_p, c_int, c_void_p]
    L.umx_forward_tiles_dev.argtypes = [c_void_p, c_void_p, c_int, c_void_p]
    L.umx_tile_grid.argtypes = [c_void_p, c_int, c_int, ip, ip, ip, ip]
    L.umx_infer_image.argtypes = [c_void_p, c_void_p, c_int, c_int, c_int, c_double, c_double, c_int, c_int, c_void_p]
    L.umx_infer_image_dev.argtypes = L.umx_infer_image.argtypes
    L.umx_infer_image_raw_outlier.restype = c_int
    L.umx_infer_image_raw_outlier.argtypes = [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_double, c_double, c_double, c_double,
                                              c_int, c_void_p]
    L.umx_infer_image_raw_scaled.restype = c_int
    L.umx_infer_image_raw_scaled.argtypes = [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_double, c_int, c_double, c_double,
                                             c_int, c_void_p]
    L.umx_infer_image_raw_submit.restype = c_int
    L.umx_infer_image_raw_submit.argtypes = [c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, c_double, c_double,
                                             c_int, c_void_p]
    L.umx_infer_image_wait.restype = c_int
    L.umx_infer_image_wait.argtypes = [c_void_p, c_int]
    L.umx_shard_unique_id.restype = c_int
    L.umx_shard_unique_id.argtypes = [c_void_p]
    L.umx_shard_init.restype = c_int
    L.umx_shard_init.argtypes = [c_void_p, c_void_p, c_int, c_int]
    L.umx_shard_fini.restype = c_int
    L.umx_shard_fini.argtypes = [c_void_p]
    L.umx_shard_init_transport.restype = c_int
    L.umx_shard_init_transport.argtypes = [c_void_p, ctypes.POINTER(ShardTransport), c_int, c_int]
    L.umx_shard_plan.restype = c_int
    L.umx_shard_plan.argtypes = [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int] + [c_void_p] * 9
    L.umx_infer_image_sharded_dev.restype = c_int
    L.umx_infer_image_sharded_dev.argtypes = [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_double, c_double, c_int,
                                              c_int, c_int, c_void_p]
    L.umx_infer_image_sharded_raw_submit.restype = c_int
    L.umx_infer_image_sharded_raw_submit.argtypes = [c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p,
                                                     c_double, c_double, c_int, c_int, c_void_p, c_void_p]
    L.umx_infer_image_sharded_raw.restype = c_int
    L.umx_infer_image_sharded_raw.argtypes = [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p,
                                              c_double, c_double, c_int, c_int, c_void_p, c_void_p]
    for fn in (L.umx_tiff_lzw_decode, L.umx_tiff_packbits_decode):
        fn.restype = ctypes.c_longlong
        fn.argtypes = [c_void_p, ctypes.c_size_t, c_void_p, ctypes.c_size_t]
    L.umx_infer_image_raw.restype = c_int
    L.umx_infer_image_raw.argtypes = [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_double, c_double, c_int,
                                      c_void_p]
    L.umx_plane_range.restype = c_int
    L.umx_plane_range.argtypes = [c_void_p, c_int, ctypes.c_size_t, c_void_p]
    L.umx_infer_image_raw_range.restype = c_int
    L.umx_infer_image_raw_range.argtypes = [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_double, c_double, c_int,
                                            c_void_p]
    L.umx_band_tiles_dev.argtypes = [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_double, c_double,
                                     c_int, c_int, c_void_p]
    L.umx_stitch_dev.argtypes = [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p]
    L.umx_profile_enable.argtypes = [c_void_p, c_int]
    L.umx_profile_read.argtypes = [c_void_p, ctypes.POINTER(ProfEntry), c_int, ip]
    L.umx_test_double_to_half.restype = None
    L.umx_test_double_to_half.argtypes = [c_void_p, c_void_p, ctypes.c_size_t]
    L.umx_describe.argtypes = [ctypes.POINTER(_HP), ip, ctypes.POINTER(c_double), ctypes.POINTER(c_double)]
    L.umx_describe_graph.argtypes = [ctypes.POINTER(_HP), ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t)]
    L.umx_describe_graph.restype = c_int
    L.umx_version.restype = ctypes.c_char_p
    L.umx_label_options_check.restype = c_int
    L.umx_label_options_check.argtypes = [ctypes.POINTER(_LabelOptions), c_int, c_int, c_int, ctypes.c_char_p, ctypes.c_size_t]
    L.umx_labeler_create.restype = c_int
    L.umx_labeler_create.argtypes = [c_int, ctypes.POINTER(c_void_p)]
    L.umx_labeler_destroy.restype = None
    L.umx_labeler_destroy.argtypes = [c_void_p]
    L.umx_labeler_last_error.restype = ctypes.c_char_p
    L.umx_labeler_last_error.argtypes = [c_void_p]
    for fn in (L.umx_labeler_run, L.umx_labeler_run_dev):
        fn.restype = c_int
        fn.argtypes = [c_void_p, c_void_p, c_int, c_int, c_int, ctypes.POINTER(_LabelOptions), c_void_p, ctypes.POINTER(ctypes.c_int64)]
    L.umx_label_split_check.restype = c_int
    L.umx_label_split_check.argtypes = [ctypes.POINTER(_LabelSplitOptions), c_int, c_int, c_int, ctypes.c_char_p, ctypes.c_size_t]
    for fn in (L.umx_labeler_run_split, L.umx_labeler_run_split_dev):
        fn.restype = c_int
        fn.argtypes = [c_void_p, c_void_p, c_int, c_int, c_int, ctypes.POINTER(_LabelSplitOptions), c_void_p, ctypes.POINTER(_LabelSplitCounts)]
    L.umx_label_flood_check.restype = c_int
    L.umx_label_flood_check.argtypes = [ctypes.POINTER(_LabelFloodOptions), c_int, c_int, c_int, ctypes.c_char_p, ctypes.c_size_t]
    L.umx_label_hmax_check.restype = c_int
    L.umx_label_hmax_check.argtypes = [ctypes.POINTER(_LabelHmaxOptions), c_int, c_int, c_int, ctypes.c_char_p, ctypes.c_size_t]
    for fn in (L.umx_labeler_run_hmax, L.umx_labeler_run_hmax_dev):
        fn.restype = c_int
        fn.argtypes = [c_void_p, c_void_p, c_int, c_int, c_int, ctypes.POINTER(_LabelHmaxOptions), c_void_p, ctypes.POINTER(_LabelHmaxCounts)]
    for fn in (L.umx_labeler_run_flood, L.umx_labeler_run_flood_dev):
        fn.restype = c_int
        fn.argtypes = [c_void_p, c_void_p, c_int, c_int, c_int, ctypes.POINTER(_LabelFloodOptions), c_void_p, ctypes.POINTER(_LabelFloodCounts)]
    L.umx_labeler_objects.restype = c_int
    L.umx_labeler_objects.argtypes = [c_void_p, c_void_p, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)]
    L.umx_labeler_last_ms.restype = c_int
    L.umx_labeler_last_ms.argtypes = [c_void_p] + [ctypes.POINTER(c_double)] * 3
    L.umx_label_measure_check.restype = c_int
    L.umx_label_measure_check.argtypes = [c_int, c_int, c_int, c_int, ctypes.c_int64, ctypes.c_char_p, ctypes.c_size_t]
    L.umx_labeler_measure.restype = c_int
    L.umx_labeler_measure.argtypes = [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)]
    L.umx_labeler_measure_dev.restype = c_int
    L.umx_labeler_measure_dev.argtypes = [c_void_p, c_void_p, ctypes.c_int64, c_void_p, c_int, c_int, c_int, c_int, c_void_p, ctypes.c_int64]
    L.umx_labeler_measure_last_ms.restype = c_int
    L.umx_labeler_measure_last_ms.argtypes = [c_void_p] + [ctypes.POINTER(c_double)] * 3
    L.umx_label_shape_check.restype = c_int
    L.umx_label_shape_check.argtypes = [c_int, c_int, ctypes.c_int64, ctypes.c_char_p, ctypes.c_size_t]
    L.umx_labeler_shape.restype = c_int
    L.umx_labeler_shape.argtypes = [c_void_p, c_int, c_int, c_void_p, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)]
    L.umx_labeler_shape_dev.restype = c_int
    L.umx_labeler_shape_dev.argtypes = [c_void_p, c_void_p, ctypes.c_int64, c_int, c_int, c_void_p, ctypes.c_int64]
    L.umx_labeler_shape_last_ms.restype = c_int
    L.umx_labeler_shape_last_ms.argtypes = [c_void_p] + [ctypes.POINTER(c_double)] * 2
    L.umx_label_contact_check.restype = c_int
    L.umx_label_contact_check.argtypes = [c_int, c_int, ctypes.c_int64, c_int, ctypes.c_char_p, ctypes.c_size_t]
    L.umx_labeler_contacts.restype = c_int
    L.umx_labeler_contacts.argtypes = [c_void_p, c_int, c_int, c_int, c_void_p, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)]
    L.umx_labeler_contacts_dev.restype = c_int
    L.umx_labeler_contacts_dev.argtypes = [c_void_p, c_void_p, ctypes.c_int64, c_int, c_int, c_int, c_void_p, ctypes.c_int64,
                                           ctypes.POINTER(ctypes.c_int64)]
    L.umx_labeler_contacts_last_ms.restype = c_int
    L.umx_labeler_contacts_last_ms.argtypes = [c_void_p] + [ctypes.POINTER(c_double)] * 2
    L.umx_labeler_contacts_last_stats.restype = c_int
    L.umx_labeler_contacts_last_stats.argtypes = [c_void_p, ctypes.POINTER(_LabelContactStats)]
    L.umx_label_hull_check.restype = c_int
    L.umx_label_hull_check.argtypes = [c_int, c_int, ctypes.c_int64, ctypes.c_char_p, ctypes.c_size_t]
    L.umx_labeler_hull.restype = c_int
    L.umx_labeler_hull.argtypes = [c_void_p, c_int, c_int, c_void_p, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64), c_void_p, ctypes.c_int64,
                                   ctypes.POINTER(ctypes.c_int64)]
    L.umx_labeler_hull_dev.restype = c_int
    L.umx_labeler_hull_dev.argtypes = [c_void_p, c_void_p, ctypes.c_int64, c_int, c_int, c_void_p, ctypes.c_int64, c_void_p, ctypes.c_int64,
                                       ctypes.POINTER(ctypes.c_int64)]
    L.umx_labeler_hull_last_ms.restype = c_int
    L.umx_labeler_hull_last_ms.argtypes = [c_void_p] + [ctypes.POINTER(c_double)] * 2
    L.umx_label_relabel_check.restype = c_int
    L.umx_label_relabel_check.argtypes = [c_int, c_int, ctypes.c_int64, ctypes.c_int64, ctypes.c_char_p, ctypes.c_size_t]
    L.umx_label_relabel_map.restype = c_int
    L.umx_label_relabel_map.argtypes = [ctypes.c_int64, c_void_p, c_void_p, ctypes.c_int64, c_void_p, ctypes.POINTER(ctypes.c_int64),
                                        ctypes.c_char_p, ctypes.c_size_t]
    L.umx_labeler_relabel.restype = c_int
    L.umx_labeler_relabel.argtypes = [c_void_p, c_int, c_int, c_void_p, ctypes.c_int64, c_void_p, ctypes.c_int64, c_void_p, c_void_p,
                                      ctypes.POINTER(ctypes.c_int64)]
    L.umx_labeler_relabel_dev.restype = c_int
    L.umx_labeler_relabel_dev.argtypes = [c_void_p, c_void_p, ctypes.c_int64, c_int, c_int, c_void_p, c_void_p, ctypes.c_int64, c_void_p,
                                          c_void_p, ctypes.POINTER(ctypes.c_int64)]
    L.umx_labeler_relabel_last_ms.restype = c_int
    L.umx_labeler_relabel_last_ms.argtypes = [c_void_p] + [ctypes.POINTER(c_double)] * 3
    L.umx_prof_entry_size.restype = c_int
    if L.umx_prof_entry_size() != ctypes.sizeof(ProfEntry):
        raise RuntimeError("libumx (%s) lays umx_prof_entry out in %d bytes, this binding in %d: mixed builds" % (
            L.umx_version().decode(), L.umx_prof_entry_size(), ctypes.sizeof(ProfEntry)))
    for name in ("umx_set_stream", "umx_synchronize", "umx_forward_tiles", "umx_forward_tiles_dev", "umx_tile_grid",
                 "umx_infer_image", "umx_infer_image_dev", "umx_band_tiles_dev", "umx_stitch_dev",
                 "umx_profile_enable", "umx_profile_read", "umx_describe"):
        getattr(L, name).restype = c_int
    _lib = L
    return L


def plane_range(raw: np.ndarray):
    """(min, max) of a contiguous uint8 / uint16 array by umx_plane_range (one pass, host threads; no GPU involved)."""
    a = np.ascontiguousarray(raw)
    if a.dtype not in (np.uint8, np.uint16) or a.size == 0:
        raise TypeError("plane_range takes non-empty uint8 / uint16 arrays")
    a = a.astype(a.dtype.newbyteorder("="), copy=False)
    out = np.zeros(2, np.uint32)
    rc = load().umx_plane_range(a.ctypes.data, a.dtype.itemsize * 8, a.size, out.ctypes.data)
    if rc != 0:
        raise UmxError(rc, "umx_plane_range")
    return int(out[0]), int(out[1])


def _hp_struct(hp: HParams) -> _HP:
    return _HP(hp.graph, hp.imSize, hp.nChannels, hp.nClasses, hp.nOut0, hp.nLayers, hp.ks, hp.nExtraConvs,
               hp.featMapsFact)


def device_count() -> int:
    return int(load().umx_device_count())


def device_mem_info(device: int):
    """(free_bytes, total_bytes) of one device -- the quantity toolbox/GPUselect.py reads through NVML."""
    f, t = ctypes.c_size_t(), ctypes.c_size_t()
    rc = load().umx_device_mem_info(int(device), ctypes.byref(f), ctypes.byref(t))
    if rc:
        raise UmxError(rc, load().umx_last_error(None).decode())
    return f.value, t.value


def pick_device_most_free_memory() -> int:
    """HIP analogue of GPUselect.pick_gpu_lowest_memory (reference toolbox/GPUselect.py:4-22)."""
    n = device_count()
    if n < 1:
        raise UmxError(3, "no HIP device available (libumx has no CPU fallback)")
    return max(range(n), key=lambda d: device_mem_info(d)[0])


def describe(hp: HParams) -> dict:
    n, f, e = ctypes.c_int(), ctypes.c_double(), ctypes.c_double()
    h = _hp_struct(hp)
    rc = load().umx_describe(ctypes.byref(h), ctypes.byref(n), ctypes.byref(f), ctypes.byref(e))
    if rc:
        raise UmxError(rc, load().umx_last_error(None).decode())
    return {"launches": n.value, "flops_per_tile": f.value, "executed_flops_per_tile": e.value}


def describe_graph(hp: HParams) -> dict:
    """The library's wiring of a model (buffers, launch list, constants): see umx_describe_graph in include/umx.h.  Host only."""
    import json
    h = _hp_struct(hp)
    need = ctypes.c_size_t()
    rc = load().umx_describe_graph(ctypes.byref(h), None, 0, ctypes.byref(need))
    if rc:
        raise UmxError(rc, load().umx_last_error(None).decode())
    buf = ctypes.create_string_buffer(need.value)
    rc = load().umx_describe_graph(ctypes.byref(h), buf, need.value, ctypes.byref(need))
    if rc:
        raise UmxError(rc, load().umx_last_error(None).decode())
    return json.loads(buf.value.decode())


def plan_check(hp: HParams) -> str:
    """umx_plan_check: "" if the split-precision planner takes every layer of this model, else the first refused layer and why.  Host only."""
    h = _hp_struct(hp)
    L = load()
    L.umx_plan_check.restype = ctypes.c_int
    L.umx_plan_check.argtypes = [ctypes.c_void_p]
    rc = L.umx_plan_check(ctypes.byref(h))
    return "" if rc == 0 else L.umx_last_error(None).decode()


def wgrad_plan(B: int, H: int, Cxt: int, Cx: int, Cg: int, slabs, f32_route: bool, planes: bool, XCs: int = 0, GCs: int = 0) -> str:
    """umx_test_wgrad_plan: the weight-gradient plan and kernel selection of one layer as a line of text; slabs = [(dy, dx, master tap,
    channel offset)].  Host only."""
    L = load()
    cols = [(ctypes.c_int * len(slabs))(*[int(s[k]) for s in slabs]) for k in range(4)]
    buf = ctypes.create_string_buffer(1024)
    L.umx_test_wgrad_plan.restype = ctypes.c_int
    L.umx_test_wgrad_plan.argtypes = [ctypes.c_int] * 6 + [ctypes.c_void_p] * 4 + [ctypes.c_int] * 4 + [ctypes.c_char_p, ctypes.c_size_t]
    _check(L, L.umx_test_wgrad_plan(B, H, Cxt, Cx, Cg, len(slabs), *cols, int(f32_route), int(planes), XCs, GCs, buf, len(buf)))
    return buf.value.decode()


def train_plan(hp, batch: int, blob, conv_f32: bool = False, no_ksplit: bool = False):
    """umx_test_train_plan: the host pass of the trainer's build for these hyper-parameters, batch and initial parameters, as one line
    per forward / input-gradient convolution in build order (its UMX_DEBUG_PLAN text, groups, direct, weight shift, descriptor and
    reference counts, K-split scratch, digest of what the upload would send).  Host only."""
    import numpy as np
    L = load()
    blob = np.ascontiguousarray(blob, dtype=np.float32)
    hps = _hp_struct(hp)
    fn = L.umx_test_train_plan
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p,
                   ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t)]
    buf = ctypes.create_string_buffer(1 << 16)
    need = ctypes.c_size_t(0)
    args = (ctypes.byref(hps), batch, int(conv_f32), int(no_ksplit), blob.ctypes.data, blob.size)
    rc = fn(*args, buf, len(buf), ctypes.byref(need))
    if rc and need.value > len(buf):
        buf = ctypes.create_string_buffer(need.value)
        rc = fn(*args, buf, len(buf), ctypes.byref(need))
    _check(L, rc)
    return buf.value.decode().splitlines()


def step_plan(hp, batch: int, blob, conv_f32: bool = False, no_ksplit: bool = False, reg: bool = True):
    """umx_test_step_plan: the stream schedule of the v2 training step after the same host pass, one line per step in host enqueue
    order: "op site stream; wait e..; record e..; r buf..; w buf..".  Host only."""
    blob = np.ascontiguousarray(blob, dtype=np.float32)
    hps = _hp_struct(hp)
    return _plan_text(load().umx_test_step_plan, [ctypes.c_void_p] + [ctypes.c_int] * 4 + [ctypes.c_void_p, ctypes.c_size_t],
                      (ctypes.byref(hps), batch, int(conv_f32), int(no_ksplit), int(reg), blob.ctypes.data, blob.size), cap=1 << 16)


def _plan_text(fn, argtypes, args, cap=1 << 14):
    """a host-only test entry that writes text into (buffer, capacity, needed): its lines"""
    fn.restype = ctypes.c_int
    fn.argtypes = argtypes + [ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t)]
    buf = ctypes.create_string_buffer(cap)
    need = ctypes.c_size_t(0)
    rc = fn(*args, buf, len(buf), ctypes.byref(need))
    if rc and need.value > len(buf):
        buf = ctypes.create_string_buffer(need.value)
        rc = fn(*args, buf, len(buf), ctypes.byref(need))
    _check(load(), rc)
    return buf.value.decode().splitlines()


def infer_plan(hp, f6: bool, act_shift: int, blob, nt: str = "", override: str = "", stamps: str = "", threads: int = 0, batches=()):
    """umx_test_infer_plan: the split-precision plan of a model under the planner's switches (given here, not through the environment), one
    line per launch but the head: its UMX_DEBUG_PLAN text, kernel, destination layout, nt16, wshift, digest of what the upload would
    send, and "n:<workgroup order>/<tiles per XCD>" for every batch n.  A model the planner refuses raises UmxError.  Host only."""
    blob = np.ascontiguousarray(blob, dtype=np.float32)
    hps = _hp_struct(hp)
    bt = (ctypes.c_int * len(batches))(*[int(b) for b in batches])
    return _plan_text(load().umx_test_infer_plan,
                      [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t] + [ctypes.c_char_p] * 3 + [ctypes.c_int, ctypes.c_void_p, ctypes.c_int],
                      (ctypes.byref(hps), int(f6), act_shift, blob.ctypes.data, blob.size, nt.encode(), override.encode(), stamps.encode(), threads, bt, len(batches)),
                      cap=1 << 17)   # (a second call would plan the model again)


def slide_plan(hp, H: int, W: int, max_batch: int, C_img: int, src_bits: int = 0, rescale: bool = False, has_range: bool = False,
               sync_call: bool = True, host_range_ok: bool = True, raw_gather: bool = False, stitch: int = 0, out_u8: bool = False,
               tile_flops: float = 0.0):
    """umx_test_slide_plan: the schedule of a whole-slide call on one GPU -- a header line, then one line per step.  Host only."""
    hps = _hp_struct(hp)
    return _plan_text(load().umx_test_slide_plan, [ctypes.c_void_p] + [ctypes.c_int] * 12 + [ctypes.c_double],
                      (ctypes.byref(hps), H, W, max_batch, C_img, src_bits, int(rescale), int(has_range), int(sync_call), int(host_range_ok),
                       int(raw_gather), stitch, int(out_u8), float(tile_flops)))


def band_plan(hp, H: int, W: int, world: int, rank: int, nslabs: int, max_batch: int, band_row0: int, band_rows: int, stitch: int = 0,
              u8: bool = False, staged: bool = False, own_stream: bool = False):
    """umx_test_band_plan: the schedule of one rank's band of a sharded slide -- a header line, then one line per launch group and per
    slab.  Host only."""
    hps = _hp_struct(hp)
    return _plan_text(load().umx_test_band_plan, [ctypes.c_void_p] + [ctypes.c_int] * 12,
                      (ctypes.byref(hps), H, W, world, rank, nslabs, max_batch, band_row0, band_rows, stitch, int(u8), int(staged), int(own_stream)))


def auto_batch(hp: HParams, arena_bytes: float = 12 * 2 ** 30) -> int:
    """Tiles per launch group for a model: enough pixels per launch to fill the chip at the deep, small layers (a 64 x 64-pixel
    tile is 4 x 4 pixels at the solo model's bottom: 256 tiles are 160 workgroups on 512 slots) -- 2^24 pixels per group, i.e.
    256 / 1024 / 4096 tiles of 256 / 128 / 64 pixels -- capped so that the activation arena stays within `arena_bytes`.
    Measured on MI355X (profiles/r03/batch_sweep.txt): solo 64-px tiles +12 %, duo 128-px tiles +22 % over groups of 256."""
    g = describe_graph(hp)
    per_tile = sum(b["size"] ** 2 * ((b["channels"] + 7) // 8 * 8) * 4 for b in g["buffers"])
    by_pixels = max(int(hp.batchSize), min(4096, (1 << 24) // (hp.imSize * hp.imSize)))
    cap = max(1, int(arena_bytes // max(per_tile, 1)))
    cap = 1 << (cap.bit_length() - 1)                      # power of two below the cap
    return max(1, min(by_pixels, max(cap, int(hp.batchSize))))


def double_to_half(x: np.ndarray) -> np.ndarray:
    x = np.ascontiguousarray(x, np.float64)
    out = np.empty(x.shape, np.uint16)
    load().umx_test_double_to_half(x.ctypes.data, out.ctypes.data, x.size)
    return out.view(np.float16)


def double_to_half_dev(x: np.ndarray) -> np.ndarray:
    """umx_test_double_to_half_dev: the DEVICE routine of the stitch kernel (needs a GPU)."""
    x = np.ascontiguousarray(x, np.float64)
    out = np.empty(x.shape, np.uint16)
    L = load()
    L.umx_test_double_to_half_dev.restype = ctypes.c_int
    L.umx_test_double_to_half_dev.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
    rc = L.umx_test_double_to_half_dev(x.ctypes.data, out.ctypes.data, x.size)
    if rc:
        raise UmxError(rc, L.umx_last_error(None).decode())
    return out.view(np.float16)


def _check(L, rc: int) -> None:
    if rc:
        raise UmxError(rc, L.umx_last_error(None).decode())


def gauss_weights(sigma: float) -> np.ndarray:
    """umx_test_gauss_weights: the resize's anti-aliasing weights of one axis, [0] = centre tap .. [radius].  Host only."""
    L = load()
    out = np.empty(4096, np.float64)
    L.umx_test_gauss_weights.restype = ctypes.c_int
    L.umx_test_gauss_weights.argtypes = [ctypes.c_double, ctypes.c_void_p, ctypes.c_int]
    radius = L.umx_test_gauss_weights(float(sigma), out.ctypes.data, out.size)
    if radius < 0:
        raise ValueError("no resize weights for sigma %r" % (sigma,))
    return out[:radius + 1].copy()


def resize_dev(src: np.ndarray, h: int, w: int):
    """umx_test_resize_dev: one resize of a float64 plane to (h, w) on the device -> (float64 plane, uint8 plane, the plane after
    the Gaussian)."""
    src = np.ascontiguousarray(src, np.float64)
    H, W = src.shape
    out, out8, filt = np.empty((h, w), np.float64), np.empty((h, w), np.uint8), np.empty((H, W), np.float64)
    L = load()
    L.umx_test_resize_dev.restype = ctypes.c_int
    L.umx_test_resize_dev.argtypes = [ctypes.c_void_p] + [ctypes.c_int] * 4 + [ctypes.c_void_p] * 3
    _check(L, L.umx_test_resize_dev(src.ctypes.data, H, W, h, w, out.ctypes.data, out8.ctypes.data, filt.ctypes.data))
    return out, out8, filt


def rescale_dev(plane: np.ndarray, outlier: float = -1.0):
    """umx_test_rescale_dev: (rescaled plane, (min, limit)); limit = max, or np.percentile(plane, outlier) for outlier >= 0."""
    plane = np.ascontiguousarray(plane, np.float64)
    out, rng = np.empty(plane.shape, np.float64), np.empty(2, np.float64)
    L = load()
    L.umx_test_rescale_dev.restype = ctypes.c_int
    L.umx_test_rescale_dev.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p]
    _check(L, L.umx_test_rescale_dev(plane.ctypes.data, plane.size, float(outlier), out.ctypes.data, rng.ctypes.data))
    return out, rng


def plane_range_dev(planes, offsets, nslabs) -> np.ndarray:
    """umx_test_plane_range_dev: the device range search on a list of 1-D uint8 / uint16 planes (one dtype), each at its own
    element offset from an aligned address and over its own number of slabs -> [len(planes), 2] (min, max)."""
    dtype = planes[0].dtype
    assert dtype in (np.uint8, np.uint16) and all(p.dtype == dtype and p.ndim == 1 for p in planes)
    raw = np.ascontiguousarray(planes[0] if len(planes) == 1 else np.concatenate(planes))
    n = np.array([p.size for p in planes], np.uintp)
    off, ns = np.ascontiguousarray(offsets, np.uintp), np.ascontiguousarray(nslabs, np.int32)
    assert off.shape == ns.shape == n.shape
    out = np.empty((len(planes), 2), np.uint32)
    L = load()
    L.umx_test_plane_range_dev.restype = ctypes.c_int
    L.umx_test_plane_range_dev.argtypes = [ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 3 + [ctypes.c_int, ctypes.c_void_p]
    _check(L, L.umx_test_plane_range_dev(raw.ctypes.data, 8 * dtype.itemsize, n.ctypes.data, off.ctypes.data, ns.ctypes.data,
                                         len(planes), out.ctypes.data))
    return out


def half_to_u8_dev(pm: np.ndarray):
    """umx_test_half_to_u8_dev: the drivers' uint8 cast of float16 probabilities -> (uint8, the float64 u8 / 255 plane)."""
    pm = np.ascontiguousarray(pm, np.float16)
    out8, outf = np.empty(pm.shape, np.uint8), np.empty(pm.shape, np.float64)
    L = load()
    L.umx_test_half_to_u8_dev.restype = ctypes.c_int
    L.umx_test_half_to_u8_dev.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]
    _check(L, L.umx_test_half_to_u8_dev(pm.ctypes.data, pm.size, out8.ctypes.data, outf.ctypes.data))
    return out8, outf


def tiff_decode(kind: str, buf: bytes, nbytes: int) -> bytes:
    """Decode one TIFF strip / tile: kind "lzw" (compression 5) or "packbits" (32773) -> exactly ``nbytes`` bytes
    (zero-filled if the stream is short)."""
    L = load()
    out = ctypes.create_string_buffer(nbytes)
    fn = {"lzw": L.umx_tiff_lzw_decode, "packbits": L.umx_tiff_packbits_decode}[kind]
    n = fn(buf, len(buf), out, nbytes)
    if n < 0:
        raise ValueError("malformed %s stream in TIFF strip" % kind)
    return out.raw


def shard_plan(hp: HParams, H: int, W: int, rank: int, world: int, nslabs: int = 2, slab: int = 0) -> dict:
    """umx_shard_plan: band / slab geometry of one rank (needs no device)."""
    L = load()
    v = [ctypes.c_int() for _ in range(9)]
    h = _hp_struct(hp)
    rc = L.umx_shard_plan(ctypes.byref(h), H, W, int(rank), int(world), int(nslabs), int(slab), *[ctypes.byref(x) for x in v])
    if rc:
        raise UmxError(rc, L.umx_last_error(None).decode())
    names = ("patch_row0", "patch_row1", "need_row0", "need_row1", "own_row0", "own_row1", "slab_row0", "slab_row1", "nslabs")
    return {n: x.value for n, x in zip(names, v)}


def grow_class_word(K: int, cls: int, grow: int, grow_classes=None) -> int:
    """The grow_classes word of umx_label_options: bit k per class index of ``grow_classes``; None with grow > 0: every class except
    0 and the label class; 0 without a growth and without classes."""
    if grow_classes is None:
        return sum(1 << k for k in range(1, K) if k != cls) if grow else 0
    word = 0
    for k in grow_classes:
        if not 0 <= int(k) < 32:
            raise ValueError("grow class %d: classes are 0..%d" % (int(k), K - 1))
        word |= 1 << int(k)
    return word


def _label_options(K: int, cls: Optional[int], min_area: int, grow: int, grow_classes) -> "_LabelOptions":
    o = _LabelOptions(K - 1 if cls is None else int(cls), int(min_area))
    o.grow_radius = int(grow)
    o.grow_classes = grow_class_word(K, o.cls, o.grow_radius, grow_classes)
    return o


def label_options_check(K: int, H: int, W: int, cls: int, min_area: int = 1, reserved=None, grow: int = 0, grow_classes=None) -> str:
    """umx_label_options_check: "" if a label mask of K planes of H x W for class ``cls``, ``min_area`` and the growth is accepted,
    else the reason.  ``reserved``: the six words after min_area by index (the first two are the growth's).  Host only."""
    o = _label_options(K, cls, min_area, grow, grow_classes)
    for j, v in enumerate(reserved or ()):
        o.reserved[j] = int(v)
    buf = ctypes.create_string_buffer(256)
    rc = load().umx_label_options_check(ctypes.byref(o), int(K), int(H), int(W), buf, len(buf))
    return "" if rc == 0 else buf.value.decode()


def _label_split_options(base: "_LabelOptions", split: int, split_core: int, split_regrow: int) -> "_LabelSplitOptions":
    o = _LabelSplitOptions()
    o.base = base
    o.depth, o.core_min_area, o.regrow = int(split), int(split_core), int(split_regrow)
    return o


def label_split_check(K: int, H: int, W: int, cls: int, min_area: int = 1, grow: int = 0, grow_classes=None, split: int = 1,
                      split_core: int = 1, split_regrow: int = 255, base_reserved=None, reserved=None, null: bool = False) -> str:
    """umx_label_split_check: "" if a split run of K planes of H x W is accepted, else the reason.  ``base_reserved``: the six words after
    min_area of the base by index, as label_options_check's ``reserved``; ``reserved``: the split's own five.  ``null``: a NULL record.
    Host only."""
    o = _label_split_options(_label_options(K, cls, min_area, grow, grow_classes), split, split_core, split_regrow)
    for j, v in enumerate(base_reserved or ()):
        o.base.reserved[j] = int(v)
    for j, v in enumerate(reserved or ()):
        o.reserved[j] = int(v)
    buf = ctypes.create_string_buffer(256)
    rc = load().umx_label_split_check(None if null else ctypes.byref(o), int(K), int(H), int(W), buf, len(buf))
    return "" if rc == 0 else buf.value.decode()


def _label_flood_options(split: "_LabelSplitOptions", flood: int, flood_step: int, flood_invert) -> "_LabelFloodOptions":
    o = _LabelFloodOptions()
    o.split = split
    o.relief_plane, o.level_step = int(flood), int(flood_step)
    o.invert = int(flood_invert)                                   # (True and False are 1 and 0)
    return o


def label_flood_check(K: int, H: int, W: int, cls: int, min_area: int = 1, grow: int = 0, grow_classes=None, split: int = 1,
                      split_core: int = 1, split_regrow: int = 255, flood: int = 0, flood_step: int = FLOOD_DEFAULT_STEP, flood_invert=False,
                      base_reserved=None, split_reserved=None, reserved=None, null: bool = False) -> str:
    """umx_label_flood_check: "" if a flood run of K planes of H x W is accepted, else the reason.  ``base_reserved`` and
    ``split_reserved``: as label_split_check's ``base_reserved`` and ``reserved``; ``reserved``: the flood's own five words.  ``null``:
    a NULL record.  Host only."""
    so = _label_split_options(_label_options(K, cls, min_area, grow, grow_classes), split, split_core, split_regrow)
    for j, v in enumerate(base_reserved or ()):
        so.base.reserved[j] = int(v)
    for j, v in enumerate(split_reserved or ()):
        so.reserved[j] = int(v)
    o = _label_flood_options(so, flood, flood_step, flood_invert)
    for j, v in enumerate(reserved or ()):
        o.reserved[j] = int(v)
    buf = ctypes.create_string_buffer(256)
    rc = load().umx_label_flood_check(None if null else ctypes.byref(o), int(K), int(H), int(W), buf, len(buf))
    return "" if rc == 0 else buf.value.decode()


def _label_hmax_options(base: "_LabelOptions", hmax: int, hmax_plane: Optional[int], hmax_invert, hmax_core: int, flood: Optional[int],
                        flood_step: int, flood_invert) -> "_LabelHmaxOptions":
    """the record of an h-maxima run: the split's depth is not used (1 is sent), its regrow is the flood's 255; without ``flood`` the
    regrow is by distance -- one level (step 256) on the plane of the class itself; ``hmax_plane`` None is that plane too"""
    so = _label_split_options(base, 1, hmax_core, SPLIT_MAX_REGROW)
    o = _LabelHmaxOptions()
    if flood is None:
        o.flood = _label_flood_options(so, base.cls, FLOOD_MAX_STEP, False)
    else:
        o.flood = _label_flood_options(so, flood, flood_step, flood_invert)
    o.seed_plane = base.cls if hmax_plane is None else int(hmax_plane)
    o.seed_invert = int(hmax_invert)
    o.height = int(hmax)
    return o


def label_hmax_check(K: int, H: int, W: int, cls: int, min_area: int = 1, grow: int = 0, grow_classes=None, hmax: int = 1,
                     hmax_plane: Optional[int] = None, hmax_invert=False, hmax_core: int = 1, flood: Optional[int] = None,
                     flood_step: int = FLOOD_DEFAULT_STEP, flood_invert=False, depth: int = 1, base_reserved=None, split_reserved=None,
                     flood_reserved=None, reserved=None, null: bool = False) -> str:
    """umx_label_hmax_check: "" if an h-maxima run of K planes of H x W is accepted, else the reason.  ``depth``: the split record's
    depth, which must pass the split's check and is otherwise not used.  ``base_reserved``, ``split_reserved`` and ``flood_reserved``:
    the reserved words of the inner records as label_flood_check names them; ``reserved``: the h-maxima's own five words.  ``null``: a
    NULL record.  Host only."""
    o = _label_hmax_options(_label_options(K, cls, min_area, grow, grow_classes), hmax, hmax_plane, hmax_invert, hmax_core, flood, flood_step,
                            flood_invert)
    o.flood.split.depth = int(depth)
    for j, v in enumerate(base_reserved or ()):
        o.flood.split.base.reserved[j] = int(v)
    for j, v in enumerate(split_reserved or ()):
        o.flood.split.reserved[j] = int(v)
    for j, v in enumerate(flood_reserved or ()):
        o.flood.reserved[j] = int(v)
    for j, v in enumerate(reserved or ()):
        o.reserved[j] = int(v)
    buf = ctypes.create_string_buffer(256)
    rc = load().umx_label_hmax_check(None if null else ctypes.byref(o), int(K), int(H), int(W), buf, len(buf))
    return "" if rc == 0 else buf.value.decode()


def label_measure_check(dtype: int, C: int, H: int, W: int, n_objects: int = 0) -> str:
    """umx_label_measure_check: "" if a measurement of C planes of H x W of that dtype code against n_objects labels is accepted, else
    the reason.  Host only."""
    buf = ctypes.create_string_buffer(256)
    rc = load().umx_label_measure_check(int(dtype), int(C), int(H), int(W), int(n_objects), buf, len(buf))
    return "" if rc == 0 else buf.value.decode()


def measure_mean_std(records: np.ndarray):
    """(mean, std) in float64 of LABEL_MEASURE_DTYPE records, as include/umx.h states them: mean = sum / count, std =
    sqrt(max(sum_sq / count - mean * mean, 0)); both nan where count is 0.  A constant object has std 0 exactly: every pixel v gives
    sum = count v and sum_sq = count v^2; count v <= 2^31 * 65535 < 2^53 is exact, so mean is v and mean * mean is the integer v^2
    exactly, sum_sq / count rounds to the same v^2, and the difference is 0."""
    count = records["count"].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = records["sum"].astype(np.float64) / count
        std = np.sqrt(np.maximum(records["sum_sq"].astype(np.float64) / count - mean * mean, 0.0))
    return mean, std


def label_shape_check(H: int, W: int, n_objects: int = 0) -> str:
    """umx_label_shape_check: "" if the shapes of n_objects labels on H x W are accepted, else the reason.  Host only."""
    buf = ctypes.create_string_buffer(256)
    rc = load().umx_label_shape_check(int(H), int(W), int(n_objects), buf, len(buf))
    return "" if rc == 0 else buf.value.decode()


SHAPE_DESCRIPTORS = ("area", "perimeter_edges", "perimeter", "euler", "holes", "mu_yy", "mu_xx", "mu_yx", "major_axis_length",
                     "minor_axis_length", "eccentricity", "orientation")


def shape_descriptors(records: np.ndarray) -> dict:
    """Step 18 of DESIGN.md section 8.1, stated here once: LABEL_SHAPE_DTYPE records [N] -> {name: array [N]} for SHAPE_DESCRIPTORS.
    int64: area = (q1 + 2 q2 + 2 qd + 3 q3 + 4 q4) / 4, perimeter_edges = q1 + q2 + 2 qd + q3, euler = (q1 - q3 + 2 qd) / 4 (both
    divisions are exact), holes = 1 - euler.  float64, with A = area: the numerators A sum_yy - sum_y^2, A sum_xx - sum_x^2 and
    A sum_xy - sum_y sum_x are formed exactly (Python integers: they pass 2^64) and each divided once by A * A -- one correctly
    rounded division -- to mu_yy, mu_xx, mu_yx; then l1, l2 = (mu_yy + mu_xx) / 2 +- sqrt(((mu_yy - mu_xx) / 2)^2 + mu_yx^2),
    major = 4 sqrt(l1), minor = 4 sqrt(max(l2, 0)), eccentricity = sqrt(1 - l2 / l1) (0 when l1 == 0), orientation =
    0.5 atan2(2 mu_yx, mu_yy - mu_xx): the angle of the major axis from the row axis, 0 for an isotropic object; perimeter =
    q2 + (q1 + q3 + 2 qd) / sqrt(2), the bit-quad estimate.  A record of area 0 (a label no pixel carries) has nan in the moment
    columns.  These are the project's reading of the usual regionprops conventions; nothing is pinned to scikit-image."""
    rec = np.asarray(records)
    q1, q2, qd, q3, q4 = (rec[n].astype(np.int64) for n in ("q1", "q2", "qd", "q3", "q4"))
    four = q1 + 2 * q2 + 2 * qd + 3 * q3 + 4 * q4
    e4 = q1 - q3 + 2 * qd
    if (four % 4).any() or (e4 % 4).any():
        raise ValueError("window counts that are no object's: 4 * area or 4 * euler is not a multiple of 4")
    area, euler = four // 4, e4 // 4
    out = {"area": area, "perimeter_edges": q1 + q2 + 2 * qd + q3, "euler": euler, "holes": 1 - euler,
           "perimeter": q2.astype(np.float64) + (q1 + q3 + 2 * qd).astype(np.float64) / np.sqrt(2.0)}
    mu = np.full((3, len(rec)), np.nan)
    for j in np.flatnonzero(area > 0):
        A, sy, sx = int(area[j]), int(rec["sum_y"][j]), int(rec["sum_x"][j])
        mu[0, j] = (A * int(rec["sum_yy"][j]) - sy * sy) / (A * A)
        mu[1, j] = (A * int(rec["sum_xx"][j]) - sx * sx) / (A * A)
        mu[2, j] = (A * int(rec["sum_xy"][j]) - sy * sx) / (A * A)
    myy, mxx, myx = mu
    half, root = (myy + mxx) / 2.0, np.sqrt(((myy - mxx) / 2.0) ** 2 + myx * myx)
    l1, l2 = half + root, half - root
    with np.errstate(divide="ignore", invalid="ignore"):
        ecc = np.where(l1 == 0.0, 0.0, np.sqrt(1.0 - l2 / l1))
    out.update({"mu_yy": myy, "mu_xx": mxx, "mu_yx": myx, "major_axis_length": 4.0 * np.sqrt(l1),
                "minor_axis_length": 4.0 * np.sqrt(np.maximum(l2, 0.0)), "eccentricity": ecc,
                "orientation": 0.5 * np.arctan2(2.0 * myx, myy - mxx)})
    return out


def label_contact_check(H: int, W: int, n_objects: int = 0, reach: int = 0) -> str:
    """umx_label_contact_check: "" if the contacts of n_objects labels on H x W at this reach are accepted, else the reason.  Host only."""
    buf = ctypes.create_string_buffer(256)
    rc = load().umx_label_contact_check(int(H), int(W), int(n_objects), int(reach), buf, len(buf))
    return "" if rc == 0 else buf.value.decode()


def contact_degrees(records: np.ndarray, N: int):
    """Step 24 of DESIGN.md section 8.1, stated here once: LABEL_CONTACT_DTYPE records [M] of labels 1..N -> (degree, shared_edges),
    both int64 [N]: entry j - 1 is the number of contacts label j takes part in and the sum of their edges.  With the shape table's
    perimeter_edges, shared_edges / perimeter_edges is the share of an object's outline that is in contact."""
    rec = np.asarray(records)
    a, b = rec["a"].astype(np.int64), rec["b"].astype(np.int64)
    if len(rec) and (a.min() < 1 or b.max() > N or (a >= b).any()):
        raise ValueError("records that are no contact list of %d labels: 1 <= a < b <= N does not hold" % N)
    both = np.concatenate([a, b]) - 1
    degree = np.bincount(both, minlength=int(N)).astype(np.int64)
    shared = np.zeros(int(N), np.int64)
    np.add.at(shared, both, np.tile(rec["edges"].astype(np.int64), 2))
    return degree, shared


def label_hull_check(H: int, W: int, n_objects: int = 0) -> str:
    """umx_label_hull_check: "" if the hulls of n_objects labels on H x W are accepted, else the reason.  Host only."""
    buf = ctypes.create_string_buffer(256)
    rc = load().umx_label_hull_check(int(H), int(W), int(n_objects), buf, len(buf))
    return "" if rc == 0 else buf.value.decode()


HULL_DESCRIPTORS = ("hull_area", "solidity", "feret_max", "feret_min", "hull_perimeter", "n_vertices")


def hull_feret_min_sq(y, x):
    """The square of the least width of one hull as an exact rational (numerator, denominator) of Python integers: the minimum over
    the hull's edges e of max_k cross(e, v_k - e_0)^2 / |e|^2.  y, x: the hull's vertices in list order, at least 3.  The largest
    cross product of an edge is taken in int64 (it is at most 2^33); the squares and the comparison of two edges' quotients -- by
    cross-multiplication -- are Python integers."""
    y, x = np.asarray(y, np.int64), np.asarray(x, np.int64)
    n = len(y)
    ey, ex = np.roll(y, -1) - y, np.roll(x, -1) - x
    best = None
    step = max(1, (1 << 20) // n)                               # edges per round: bounds the n x step temporaries
    for i0 in range(0, n, step):
        s = slice(i0, i0 + step)
        cross = ex[s, None] * (y[None, :] - y[s, None]) - ey[s, None] * (x[None, :] - x[s, None])
        widest = np.abs(cross).max(axis=1)
        for c, dy, dx in zip(widest.tolist(), ey[s].tolist(), ex[s].tolist()):
            num, den = c * c, dy * dy + dx * dx
            if best is None or num * best[1] < best[0] * den:
                best = (num, den)
    return best


def hull_descriptors(records: np.ndarray, vertices: np.ndarray, area) -> dict:
    """Step 28 of DESIGN.md section 8.1, stated here once: LABEL_HULL_DTYPE records [N], LABEL_HULL_VERTEX_DTYPE vertices [V] and the
    objects' pixel counts [N] (the label table's or the shape table's area) -> {name: array [N]} for HULL_DESCRIPTORS, float64 but
    n_vertices (int64).  hull_area = area2 / 2; solidity = area / hull_area, at most 1 and 1 exactly for a full rectangle; feret_max
    = sqrt(feret_max_sq); feret_min = the least width of the hull, the minimum over its edges e of max_k cross(e, v_k)^2 / |e|^2
    chosen exactly (hull_feret_min_sq) and rounded once, by one division and one sqrt; hull_perimeter = the sum of hypot over the
    edges, added in list order.  A label no pixel carries (n_vertices 0) has 0 in every column."""
    rec, verts = np.asarray(records), np.asarray(vertices)
    N = len(rec)
    area = np.asarray(area).astype(np.float64)
    if area.shape != (N,):
        raise ValueError("area has shape %s for %d records" % (area.shape, N))
    n = rec["n_vertices"].astype(np.int64)
    first = rec["first"].astype(np.int64)
    if N and (not np.array_equal(first, np.cumsum(n) - n) or int(n.sum()) != len(verts) or ((n != 0) & (n < 4)).any()):
        raise ValueError("records and vertices that are no hull table: first is not the running sum of n_vertices over %d vertices" % len(verts))
    hull_area = rec["area2"].astype(np.float64) / 2.0
    out = {"hull_area": hull_area, "solidity": np.zeros(N), "feret_max": np.sqrt(rec["feret_max_sq"].astype(np.float64)),
           "feret_min": np.zeros(N), "hull_perimeter": np.zeros(N), "n_vertices": n}
    present = n > 0
    out["solidity"][present] = area[present] / hull_area[present]
    vy, vx = verts["y"].astype(np.int64), verts["x"].astype(np.int64)
    for j in np.flatnonzero(present):
        y, x = vy[first[j]:first[j] + n[j]], vx[first[j]:first[j] + n[j]]
        num, den = hull_feret_min_sq(y, x)
        out["feret_min"][j] = math.sqrt(num / den)
        edges = np.hypot((np.roll(y, -1) - y).astype(np.float64), (np.roll(x, -1) - x).astype(np.float64))
        out["hull_perimeter"][j] = np.cumsum(edges)[-1]        # (cumsum adds in order; np.sum adds pairwise)
    return out


def label_relabel_check(H: int, W: int, n_objects: int = 0, n_pairs: int = 0) -> str:
    """umx_label_relabel_check: "" if a relabel of n_objects labels on H x W with n_pairs pairs is accepted, else the reason.  Host only."""
    buf = ctypes.create_string_buffer(256)
    rc = load().umx_label_relabel_check(int(H), int(W), int(n_objects), int(n_pairs), buf, len(buf))
    return "" if rc == 0 else buf.value.decode()


def _relabel_args(n_objects: int, keep, pairs):
    """keep (None, or n_objects values: nonzero keeps) and pairs (None, or [M, 2] labels) as the contiguous uint8 and int32 arrays the
    library reads, either None when not given; what cannot be such arguments raises UmxError(ERR_INVALID) as the library would"""
    if keep is not None:
        keep = np.ascontiguousarray(np.asarray(keep) != 0, np.uint8).ravel()
        if keep.size != int(n_objects):
            raise UmxError(ERR_INVALID, "keep has %d entries: %d objects need as many" % (keep.size, int(n_objects)))
    if pairs is not None:
        p = np.asarray(pairs)
        if p.size and (p.ndim != 2 or p.shape[1] != 2):
            raise UmxError(ERR_INVALID, "pairs must be [M, 2] labels, not %s" % (p.shape,))
        p = p.reshape(-1, 2)
        if p.size and (p.dtype.kind not in "iu" or p.min() < -2 ** 31 or p.max() > 2 ** 31 - 1):
            raise UmxError(ERR_INVALID, "pairs must be integers that fit an int32")
        pairs = np.ascontiguousarray(p, np.int32)
    return keep, pairs


def relabel_map(n_objects: int, keep=None, pairs=None):
    """umx_label_relabel_map, steps 29 and 30 of DESIGN.md section 8.1 on the host (no device): -> (map int32 [n_objects + 1], N').
    keep: None (all) or n_objects values, nonzero keeps label j at keep[j - 1]; pairs: None or [M, 2] labels to merge.  map[j] is
    the new number of label j, 0 for a dropped one; the kept classes are numbered in order of their least member.  A pair outside
    1..n_objects, or one that names a dropped label, raises UmxError with the pair's index."""
    why = label_relabel_check(1, 1, n_objects, 0 if pairs is None else len(pairs))   # (before the map is sized from the arguments)
    if why:
        raise UmxError(ERR_INVALID, why)
    keep, pairs = _relabel_args(n_objects, keep, pairs)
    out = np.zeros(int(n_objects) + 1, np.int32)
    n = ctypes.c_int64(-1)
    buf = ctypes.create_string_buffer(256)
    rc = load().umx_label_relabel_map(int(n_objects), None if keep is None else keep.ctypes.data, None if pairs is None else pairs.ctypes.data,
                                      0 if pairs is None else len(pairs), out.ctypes.data, ctypes.byref(n), buf, len(buf))
    if rc:
        raise UmxError(rc, buf.value.decode())
    return out, int(n.value)


def relabel_objects(objects: np.ndarray, map: np.ndarray) -> np.ndarray:
    """Step 32 of DESIGN.md section 8.1 on the host, for callers of relabel_ptr: LABEL_OBJECT_DTYPE records [N] and a map [N + 1] of
    relabel_map -> the records [N'] of the new labels: area, sum_y and sum_x added, y0 and x0 by minimum, y1 and x1 by maximum over
    the members.  A new label whose members have no pixel has the empty record (area 0, y0 = x0 = 2^31 - 1, y1 = x1 = -1)."""
    objects, m = np.asarray(objects), np.asarray(map).astype(np.int64)
    if objects.dtype != LABEL_OBJECT_DTYPE or m.ndim != 1 or len(m) != len(objects) + 1 or m[0] != 0 or (len(m) > 1 and m.min() < 0):
        raise ValueError("objects must be LABEL_OBJECT_DTYPE [N] and map the N + 1 words of relabel_map")
    n_new = int(m.max())
    out = np.zeros(n_new, LABEL_OBJECT_DTYPE)
    out["y0"] = out["x0"] = 2 ** 31 - 1
    out["y1"] = out["x1"] = -1
    to = m[1:] - 1
    live = (to >= 0) & (objects["area"] > 0)
    to, src = to[live], objects[live]
    for name in ("area", "sum_y", "sum_x"):
        np.add.at(out[name], to, src[name])
    for name in ("y0", "x0"):
        np.minimum.at(out[name], to, src[name])
    for name in ("y1", "x1"):
        np.maximum.at(out[name], to, src[name])
    return out


class Labeler:
    """One umx_labeler: the label mask (include/umx.h) of uint8 probability stacks on one MI355X.  It needs no
    model; its device buffers grow on demand and are kept between runs."""

    def __init__(self, device: int = 0):
        self._L = load()
        self._lb = ctypes.c_void_p()
        rc = self._L.umx_labeler_create(int(device), ctypes.byref(self._lb))
        if rc:
            raise UmxError(rc, self._L.umx_labeler_last_error(None).decode())
        self.device = device
        self._split_counts = None
        self._flood_counts = None
        self._hmax_counts = None
        self._last_shape = (1, 1)                                  # H, W of the last run: what shape() names when not told
        self._contacts_room = 1024                                 # records the next contacts call offers: the last list's length
        self._contacts_reruns_before = 0                           # reruns of a first pass that was offered too little room
        self._hull_room = (1024, 16384)                            # records and vertices the next hull call offers: the last call's

    def close(self) -> None:
        if getattr(self, "_lb", None) and self._lb.value:
            self._L.umx_labeler_destroy(self._lb)
            self._lb = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, rc: int) -> None:
        if rc:
            raise UmxError(rc, self._L.umx_labeler_last_error(self._lb).decode())

    def objects(self) -> np.ndarray:
        """The table of the last run: a structured array (LABEL_OBJECT_DTYPE), one record per kept object in label order."""
        n = ctypes.c_int64()
        self._check(self._L.umx_labeler_objects(self._lb, None, 0, ctypes.byref(n)))
        out = np.zeros(n.value, LABEL_OBJECT_DTYPE)
        if n.value:
            self._check(self._L.umx_labeler_objects(self._lb, out.ctypes.data, n.value, ctypes.byref(n)))
        return out

    def last_ms(self):
        """(upload, kernel, download) milliseconds of the last run, by HIP events on the labeler's stream."""
        v = [ctypes.c_double() for _ in range(3)]
        self._check(self._L.umx_labeler_last_ms(self._lb, *[ctypes.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def split_counts(self) -> dict:
        """n_objects (N), n_before (N0), n_cored and unreached of the last run with split > 0 of this Labeler; None before one, and
        after a later run without a split.  A refused run (ERR_INVALID) leaves these and the two below as they were."""
        return self._split_counts

    def flood_counts(self) -> dict:
        """The counts of the last run with a flood of this Labeler: the four of split_counts(), levels_claimed (levels at which a pixel
        was claimed), claimed (pixels claimed in all) and launches (informative); None before one, and after a later run without."""
        return self._flood_counts

    def hmax_counts(self) -> dict:
        """The counts of the last run with h-maxima seeds of this Labeler: the seven of flood_counts(), seed_pixels (|E|) and
        recon_launches (a pair, informative); None before one, and after a later run without."""
        return self._hmax_counts

    def _run_any(self, planes_ptr, dev: bool, K: int, H: int, W: int, o: "_LabelOptions", labels_ptr, split: int, split_core: int,
                 split_regrow: int, flood: Optional[int] = None, flood_step: int = FLOOD_DEFAULT_STEP, flood_invert=False,
                 hmax: Optional[int] = None, hmax_plane: Optional[int] = None, hmax_invert=False, hmax_core: int = 1) -> int:
        """the entry of today when split is 0, else the split's, or the flood's when ``flood`` names a plane; the h-maxima's when
        ``hmax`` names a height; -> N.  A refused call (ERR_INVALID) has touched nothing: the counts of the run before stand too."""
        if hmax is not None and split:
            raise ValueError("hmax and split both place the seeds: give one of them")
        before = tuple(getattr(self, name, None) for name in ("_split_counts", "_flood_counts", "_hmax_counts"))
        try:
            return self._run_counted(planes_ptr, dev, K, H, W, o, labels_ptr, split, split_core, split_regrow, flood, flood_step, flood_invert,
                                     hmax, hmax_plane, hmax_invert, hmax_core)
        except UmxError as e:
            if e.code == ERR_INVALID:
                self._split_counts, self._flood_counts, self._hmax_counts = before
            raise

    def _run_counted(self, planes_ptr, dev, K, H, W, o, labels_ptr, split, split_core, split_regrow, flood, flood_step, flood_invert, hmax,
                     hmax_plane, hmax_invert, hmax_core) -> int:
        """_run_any's call; the three counts are those of this call, None where it has none or fails"""
        planes_ptr, labels_ptr = ctypes.c_void_p(planes_ptr), ctypes.c_void_p(labels_ptr or None)
        if hmax is not None:
            ho = _label_hmax_options(o, hmax, hmax_plane, hmax_invert, hmax_core, flood, flood_step, flood_invert)
            hc = _LabelHmaxCounts()
            fn = self._L.umx_labeler_run_hmax_dev if dev else self._L.umx_labeler_run_hmax
            self._split_counts = self._flood_counts = self._hmax_counts = None
            self._check(fn(self._lb, planes_ptr, K, H, W, ctypes.byref(ho), labels_ptr, ctypes.byref(hc)))
            self._flood_counts = {name: int(getattr(hc.flood, name)) for name, _ in _LabelFloodCounts._fields_ if name != "reserved"}
            self._split_counts = {name: self._flood_counts[name] for name, _ in _LabelSplitCounts._fields_}
            self._hmax_counts = dict(self._flood_counts, seed_pixels=int(hc.seed_pixels), recon_launches=tuple(int(v) for v in hc.recon_launches))
            return int(hc.flood.n_objects)
        self._split_counts = None
        self._flood_counts = None
        self._hmax_counts = None
        if flood is not None:                                      # (without a split the library refuses the depth of 0)
            fo = _label_flood_options(_label_split_options(o, split, split_core, split_regrow), flood, flood_step, flood_invert)
            fc = _LabelFloodCounts()
            fn = self._L.umx_labeler_run_flood_dev if dev else self._L.umx_labeler_run_flood
            self._check(fn(self._lb, planes_ptr, K, H, W, ctypes.byref(fo), labels_ptr, ctypes.byref(fc)))
            self._flood_counts = {name: int(getattr(fc, name)) for name, _ in _LabelFloodCounts._fields_ if name != "reserved"}
            self._split_counts = {name: self._flood_counts[name] for name, _ in _LabelSplitCounts._fields_}
            return int(fc.n_objects)
        if not split:
            n = ctypes.c_int64()
            fn = self._L.umx_labeler_run_dev if dev else self._L.umx_labeler_run
            self._check(fn(self._lb, planes_ptr, K, H, W, ctypes.byref(o), labels_ptr, ctypes.byref(n)))
            return n.value
        so = _label_split_options(o, split, split_core, split_regrow)
        c = _LabelSplitCounts()
        fn = self._L.umx_labeler_run_split_dev if dev else self._L.umx_labeler_run_split
        self._check(fn(self._lb, planes_ptr, K, H, W, ctypes.byref(so), labels_ptr, ctypes.byref(c)))
        self._split_counts = {name: int(getattr(c, name)) for name, _ in _LabelSplitCounts._fields_}
        return int(c.n_objects)

    def run(self, planes: np.ndarray, cls: Optional[int] = None, min_area: int = 1, want_labels: bool = True, grow: int = 0,
            grow_classes=None, split: int = 0, split_core: int = 1, split_regrow: int = 255, flood: Optional[int] = None,
            flood_step: int = FLOOD_DEFAULT_STEP, flood_invert: bool = False, hmax: Optional[int] = None, hmax_plane: Optional[int] = None,
            hmax_invert: bool = False, hmax_core: int = 1):
        """planes uint8 [K, H, W] in the model's class order -> (labels int32 [H, W], objects); ``cls`` None: the last class.
        want_labels False: labels is None (only the count and the table come down).  grow R > 0: the kept objects grow R levels
        over the pixels whose class is in ``grow_classes`` (an iterable of class indices; None: every class but 0 and ``cls``).
        split D > 0: the kept objects are split at their necks first (erosion cores of depth D and area >= ``split_core``, regrown
        at most ``split_regrow`` levels inside their objects); split_counts() has the counts.
        split 0 is the call of before.
        flood P (with split > 0): the cores are regrown by the level flood on the relief planes[P] (255 - planes[P] with
        ``flood_invert``) in levels of ``flood_step`` (a power of two, 1..256) instead of by distance, so a neck is cut along the
        relief's ridge (steps 19 to 21; split_regrow must stay 255); flood_counts() has the counts.  None is the call of before.
        hmax h (1..255, without split): the seeds are the extended maxima of the h-maxima transform of planes[``hmax_plane``]
        (255 - that with ``hmax_invert``; None: the plane of ``cls``) inside the kept objects -- a peak seeds an object of its own
        iff it stands more than h above the saddle to a higher one -- with components of fewer than ``hmax_core`` pixels seeding
        nothing (steps 33 to 36); they are regrown by the flood of ``flood`` / ``flood_step`` / ``flood_invert``, or by distance
        without ``flood``; hmax_counts() has the counts.  hmax together with split is a ValueError.  None is the call of before."""
        planes = np.ascontiguousarray(planes)
        if planes.dtype != np.uint8 or planes.ndim != 3:
            raise TypeError("planes must be uint8 [K, H, W]")
        K, H, W = planes.shape
        o = _label_options(K, cls, min_area, grow, grow_classes)
        labels = np.empty((H, W), np.int32) if want_labels else None
        n = self._run_any(planes.ctypes.data, False, K, H, W, o, labels.ctypes.data if want_labels else None, split, split_core, split_regrow,
                          flood, flood_step, flood_invert, hmax, hmax_plane, hmax_invert, hmax_core)
        if want_labels:
            self._last_shape = (H, W)                              # (of the resident labels: a refused run above has left them)
        objs = self.objects()
        assert len(objs) == n
        return labels, objs

    def run_ptr(self, planes_ptr: int, K: int, H: int, W: int, labels_ptr: int = 0, cls: Optional[int] = None, min_area: int = 1,
                grow: int = 0, grow_classes=None, split: int = 0, split_core: int = 1, split_regrow: int = 255,
                flood: Optional[int] = None, flood_step: int = FLOOD_DEFAULT_STEP, flood_invert: bool = False, hmax: Optional[int] = None,
                hmax_plane: Optional[int] = None, hmax_invert: bool = False, hmax_core: int = 1) -> np.ndarray:
        """umx_labeler_run_dev on DEVICE addresses (e.g. torch.Tensor.data_ptr()): uint8 [K, H, W] in, int32 [H, W] out (0: no label
        plane) -> objects.  The planes must be complete; the call returns with the labels complete.  grow, grow_classes and the
        split's three, the flood's three and the h-maxima's four: as run."""
        o = _label_options(int(K), cls, min_area, grow, grow_classes)
        self._run_any(planes_ptr, True, int(K), int(H), int(W), o, labels_ptr, split, split_core, split_regrow, flood, flood_step, flood_invert,
                      hmax, hmax_plane, hmax_invert, hmax_core)
        return self.objects()

    def measure(self, planes: np.ndarray) -> np.ndarray:
        """umx_labeler_measure: uint8 / uint16 planes [C, H, W] (or one plane [H, W]) against the labels the last run(want_labels=True)
        left on the device -> LABEL_MEASURE_DTYPE [C, N], record [c, j - 1] of plane c and label j."""
        planes = np.ascontiguousarray(planes)
        if planes.ndim == 2:
            planes = planes[None]
        if planes.dtype not in _MEASURE_DTYPES or planes.ndim != 3:
            raise TypeError("planes must be uint8 or uint16 [C, H, W] or [H, W], not %s %s" % (planes.dtype, planes.shape))
        code = _MEASURE_DTYPES[planes.dtype]
        C, H, W = planes.shape
        n = ctypes.c_int64()
        self._check(self._L.umx_labeler_measure(self._lb, None, code, C, H, W, None, 0, ctypes.byref(n)))
        out = np.zeros((C, n.value), LABEL_MEASURE_DTYPE)
        self._check(self._L.umx_labeler_measure(self._lb, planes.ctypes.data, code, C, H, W, out.ctypes.data, out.size, ctypes.byref(n)))
        return out

    def measure_ptr(self, labels_ptr: int, n_objects: int, planes_ptr: int, dtype, C: int, H: int, W: int) -> np.ndarray:
        """umx_labeler_measure_dev on DEVICE addresses (e.g. torch.Tensor.data_ptr()): int32 [H, W] labels with objects 1..n_objects
        and planes [C, H, W] of ``dtype`` (np.uint8 / np.uint16, or a UMX_MEASURE_* code), both complete -> LABEL_MEASURE_DTYPE
        [C, n_objects].  Needs no prior run."""
        code = dtype if isinstance(dtype, int) else _MEASURE_DTYPES.get(np.dtype(dtype), 0)
        why = label_measure_check(code, C, H, W, n_objects)        # (before any buffer is sized from the arguments)
        if why:
            raise UmxError(ERR_INVALID, why)
        out = np.zeros((int(C), int(n_objects)), LABEL_MEASURE_DTYPE)
        self._check(self._L.umx_labeler_measure_dev(self._lb, ctypes.c_void_p(labels_ptr), int(n_objects), ctypes.c_void_p(planes_ptr), code,
                                                    int(C), int(H), int(W), out.ctypes.data, out.size))
        return out

    def measure_last_ms(self):
        """(upload, kernel, download) milliseconds of the last measurement, summed over its groups of planes."""
        v = [ctypes.c_double() for _ in range(3)]
        self._check(self._L.umx_labeler_measure_last_ms(self._lb, *[ctypes.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def shape(self, H: Optional[int] = None, W: Optional[int] = None) -> np.ndarray:
        """umx_labeler_shape: the shapes of the labels the last run(want_labels=True) left on the device -- plain, grown or split --
        -> LABEL_SHAPE_DTYPE [N], record j - 1 of label j; shape_descriptors turns them into axes, perimeter and holes.  H, W: the
        size the caller believes the labels have (refused when it is not theirs); None: that of the last run of this Labeler."""
        H, W = (self._last_shape[0] if H is None else H), (self._last_shape[1] if W is None else W)
        n = ctypes.c_int64()
        self._check(self._L.umx_labeler_shape(self._lb, int(H), int(W), None, 0, ctypes.byref(n)))
        out = np.zeros(n.value, LABEL_SHAPE_DTYPE)
        self._check(self._L.umx_labeler_shape(self._lb, int(H), int(W), out.ctypes.data, out.size, ctypes.byref(n)))
        return out

    def shape_ptr(self, labels_ptr: int, n_objects: int, H: int, W: int) -> np.ndarray:
        """umx_labeler_shape_dev on a DEVICE address (e.g. torch.Tensor.data_ptr()): int32 [H, W] labels with objects 1..n_objects,
        complete -> LABEL_SHAPE_DTYPE [n_objects].  Needs no prior run."""
        why = label_shape_check(H, W, n_objects)                   # (before any buffer is sized from the arguments)
        if why:
            raise UmxError(ERR_INVALID, why)
        out = np.zeros(int(n_objects), LABEL_SHAPE_DTYPE)
        self._check(self._L.umx_labeler_shape_dev(self._lb, ctypes.c_void_p(labels_ptr), int(n_objects), int(H), int(W), out.ctypes.data,
                                                  out.size))
        return out

    def shape_last_ms(self):
        """(kernel, download) milliseconds of the last shape call."""
        v = [ctypes.c_double() for _ in range(2)]
        self._check(self._L.umx_labeler_shape_last_ms(self._lb, *[ctypes.byref(x) for x in v]))
        return tuple(x.value for x in v)


    def _contacts(self, call) -> np.ndarray:
        """call(out_ptr, cap, m_ref) -> rc.  The length of the list is known only after the pass over the plane: the call offers room
        for as many records as the last list had and, when the library refuses that as too little, once more what it asked for
        (contacts_stats() then counts the reruns of both passes; contacts_last_ms() is the second one's)."""
        m = ctypes.c_int64(-1)
        out = np.zeros(self._contacts_room, LABEL_CONTACT_DTYPE)
        self._contacts_reruns_before = 0
        rc = call(out.ctypes.data, out.size, ctypes.byref(m))
        if rc == ERR_INVALID and m.value > out.size:
            self._contacts_reruns_before = self.contacts_stats()["reruns"]
            out = np.zeros(m.value, LABEL_CONTACT_DTYPE)
            rc = call(out.ctypes.data, out.size, ctypes.byref(m))
        self._check(rc)
        self._contacts_room = max(1024, int(m.value))
        return out[:m.value].copy()

    def contacts(self, reach: int = 0, H: Optional[int] = None, W: Optional[int] = None) -> np.ndarray:
        """umx_labeler_contacts: which objects of the labels the last run(want_labels=True) left on the device -- plain, grown, split
        or flooded -- touch: LABEL_CONTACT_DTYPE [M] sorted by (a, b), a < b, ``edges`` the pixel edges they share (4-neighbours).
        reach R > 0: on a scratch copy grown R levels over every unlabelled pixel, so that objects up to about 2 R apart with
        nothing between them count as neighbours; the resident labels are untouched.  H, W: as shape()."""
        H, W = (self._last_shape[0] if H is None else H), (self._last_shape[1] if W is None else W)
        return self._contacts(lambda out, cap, m: self._L.umx_labeler_contacts(self._lb, int(H), int(W), int(reach), out, cap, m))

    def contacts_ptr(self, labels_ptr: int, n_objects: int, H: int, W: int, reach: int = 0) -> np.ndarray:
        """umx_labeler_contacts_dev on a DEVICE address (e.g. torch.Tensor.data_ptr()): int32 [H, W] labels with objects 1..n_objects,
        complete and only read -> LABEL_CONTACT_DTYPE [M].  Needs no prior run."""
        why = label_contact_check(H, W, n_objects, reach)          # (before any buffer is sized from the arguments)
        if why:
            raise UmxError(ERR_INVALID, why)
        return self._contacts(lambda out, cap, m: self._L.umx_labeler_contacts_dev(self._lb, ctypes.c_void_p(labels_ptr), int(n_objects),
                                                                                     int(H), int(W), int(reach), out, cap, m))

    def contacts_last_ms(self):
        """(kernel, download) milliseconds of the last contacts call."""
        v = [ctypes.c_double() for _ in range(2)]
        self._check(self._L.umx_labeler_contacts_last_ms(self._lb, *[ctypes.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def contacts_stats(self) -> dict:
        """umx_labeler_contacts_last_stats: table_capacity (entries), reruns (passes repeated with the table doubled), longest_row
        (the most contacts (a, .) of one label a) and ordered_by ("device", "host", or "none" for an empty list) of the last call."""
        st = _LabelContactStats()
        self._check(self._L.umx_labeler_contacts_last_stats(self._lb, ctypes.byref(st)))
        return {"table_capacity": int(st.table_capacity), "reruns": int(st.reruns) + self._contacts_reruns_before, "longest_row": int(st.longest_row),
                "ordered_by": {CONTACT_ORDER_NONE: "none", CONTACT_ORDER_DEVICE: "device", CONTACT_ORDER_HOST: "host"}[st.ordered_by]}

    def _hull(self, call, n_known=None):
        """call(out_ptr, cap, n_ref, verts_ptr, vcap, v_ref) -> rc.  The number of vertices is known only after the passes over the
        plane, the number of records of hull() only to the library: the call offers the room of the last call and, when the library
        refuses that as too little, what it asked for (too few records are refused before the device works; hull_last_ms() is the
        last call's)."""
        n, v = ctypes.c_int64(-1), ctypes.c_int64(-1)
        rec = np.zeros(self._hull_room[0] if n_known is None else int(n_known), LABEL_HULL_DTYPE)
        verts = np.zeros(self._hull_room[1], LABEL_HULL_VERTEX_DTYPE)
        for _ in range(3):
            n.value, v.value = -1, -1
            rc = call(rec.ctypes.data if rec.size else None, rec.size, ctypes.byref(n), verts.ctypes.data if verts.size else None, verts.size,
                      ctypes.byref(v))
            if rc == ERR_INVALID and n.value > rec.size:
                rec = np.zeros(n.value, LABEL_HULL_DTYPE)
            elif rc == ERR_INVALID and v.value > verts.size:
                verts = np.zeros(v.value, LABEL_HULL_VERTEX_DTYPE)
            else:
                break
        self._check(rc)
        N = int(n_known) if n_known is not None else int(n.value)
        self._hull_room = (max(1024, N), max(16384, int(v.value)))
        return rec[:N].copy(), verts[:v.value].copy()

    def hull(self, H: Optional[int] = None, W: Optional[int] = None):
        """umx_labeler_hull: the convex hulls of the labels the last run(want_labels=True) left on the device -- plain, grown, split
        or flooded -- -> (LABEL_HULL_DTYPE [N], LABEL_HULL_VERTEX_DTYPE [V]): record j - 1 of label j, whose vertices are
        vertices[first : first + n_vertices], corners of the pixel squares, from the top-left one along the top edge.
        hull_descriptors turns them into solidity and the Feret diameters.  H, W: as shape()."""
        H, W = (self._last_shape[0] if H is None else H), (self._last_shape[1] if W is None else W)
        return self._hull(lambda out, cap, n, verts, vcap, v: self._L.umx_labeler_hull(self._lb, int(H), int(W), out, cap, n, verts, vcap, v))

    def hull_ptr(self, labels_ptr: int, n_objects: int, H: int, W: int):
        """umx_labeler_hull_dev on a DEVICE address (e.g. torch.Tensor.data_ptr()): int32 [H, W] labels with objects 1..n_objects,
        complete and only read -> (LABEL_HULL_DTYPE [n_objects], LABEL_HULL_VERTEX_DTYPE [V]).  Needs no prior run."""
        why = label_hull_check(H, W, n_objects)                    # (before any buffer is sized from the arguments)
        if why:
            raise UmxError(ERR_INVALID, why)
        return self._hull(lambda out, cap, n, verts, vcap, v: self._L.umx_labeler_hull_dev(self._lb, ctypes.c_void_p(labels_ptr), int(n_objects),
                                                                                             int(H), int(W), out, cap, verts, vcap, v),
                          n_known=n_objects)

    def hull_last_ms(self):
        """(kernel, download) milliseconds of the last hull call."""
        v = [ctypes.c_double() for _ in range(2)]
        self._check(self._L.umx_labeler_hull_last_ms(self._lb, *[ctypes.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def relabel(self, keep=None, pairs=None, want_labels: bool = True, H: Optional[int] = None, W: Optional[int] = None):
        """umx_labeler_relabel: drops and merges objects of the labels the last run(want_labels=True) left on the device and renumbers
        the rest 1..N'  -> (labels int32 [H, W] or None, objects [N'], map int32 [N + 1]).
        keep: None (all) or one value per object, nonzero keeps it; pairs: None or [M, 2] labels to merge (their closure is merged;
        a pair that names a dropped label is refused).  The labels and the table on the device are edited in place: objects(),
        measure(), shape(), contacts() and hull() afterwards see the new ones.  A refused call has changed nothing.  H, W: as shape()."""
        H, W = (self._last_shape[0] if H is None else H), (self._last_shape[1] if W is None else W)
        n = ctypes.c_int64()
        self._check(self._L.umx_labeler_objects(self._lb, None, 0, ctypes.byref(n)))
        keep, pairs = _relabel_args(n.value if keep is None else len(np.asarray(keep).ravel()), keep, pairs)
        why = label_relabel_check(H, W, 0, 0 if pairs is None else len(pairs))   # (before any buffer is sized from the arguments)
        if why:
            raise UmxError(ERR_INVALID, why)
        labels = np.empty((int(H), int(W)), np.int32) if want_labels else None
        map_ = np.zeros(n.value + 1, np.int32)
        n_new = ctypes.c_int64(-1)
        self._check(self._L.umx_labeler_relabel(self._lb, int(H), int(W), None if keep is None else keep.ctypes.data,
                                                0 if keep is None else keep.size, None if pairs is None else pairs.ctypes.data,
                                                0 if pairs is None else len(pairs), labels.ctypes.data if want_labels else None,
                                                map_.ctypes.data, ctypes.byref(n_new)))
        objs = self.objects()
        assert len(objs) == n_new.value
        return labels, objs, map_

    def relabel_ptr(self, labels_ptr: int, n_objects: int, H: int, W: int, keep=None, pairs=None, out_ptr: Optional[int] = None):
        """umx_labeler_relabel_dev on DEVICE addresses (e.g. torch.Tensor.data_ptr()): int32 [H, W] labels with objects 1..n_objects,
        complete, remapped into the int32 [H, W] plane at out_ptr (None: in place) -> (map int32 [n_objects + 1], N').  A value
        outside 0..n_objects comes out 0.  No table: relabel_objects remaps the caller's.  Needs no prior run and leaves the resident
        labels alone."""
        why = label_relabel_check(H, W, n_objects, 0 if pairs is None else len(pairs))   # (before any buffer is sized from the arguments)
        if why:
            raise UmxError(ERR_INVALID, why)
        keep, pairs = _relabel_args(n_objects, keep, pairs)
        map_ = np.zeros(int(n_objects) + 1, np.int32)
        n_new = ctypes.c_int64(-1)
        self._check(self._L.umx_labeler_relabel_dev(self._lb, ctypes.c_void_p(labels_ptr), int(n_objects), int(H), int(W),
                                                    None if keep is None else keep.ctypes.data, None if pairs is None else pairs.ctypes.data,
                                                    0 if pairs is None else len(pairs), ctypes.c_void_p(labels_ptr if out_ptr is None else out_ptr),
                                                    map_.ctypes.data, ctypes.byref(n_new)))
        return map_, int(n_new.value)

    def relabel_last_ms(self):
        """(upload, kernel, download) milliseconds of the last relabel call."""
        v = [ctypes.c_double() for _ in range(3)]
        self._check(self._L.umx_labeler_relabel_last_ms(self._lb, *[ctypes.byref(x) for x in v]))
        return tuple(x.value for x in v)


class Engine:
    """One umx_ctx: a model resident on one MI355X."""

    def __init__(self, hp: HParams, blob: np.ndarray, device: int = 0, max_batch: int = 32,
                 precision="default", act_shift: int = -1, lanes: int = 0):
        """precision: "default" (f16x3 unless UMX_PRECISION=f32), "f32" (exact fp32 MFMA) or "f16x3" (three binary16
        MFMA products per fp32 product, fp32 accumulation) -- both hold the 1e-4 tolerance.
        lanes: 0 = library default, 1 or 2 activation-buffer sets / streams the tile batches alternate between."""
        self._L = load()
        self.hp = hp
        self._ctx = ctypes.c_void_p()
        blob = np.ascontiguousarray(blob, dtype="<f4")
        h = _hp_struct(hp)
        o = _Options(int(device), int(max_batch), PRECISIONS.get(precision, precision), int(act_shift), int(lanes))
        rc = self._L.umx_create_opts(ctypes.byref(h), blob.ctypes.data, blob.size, ctypes.byref(o),
                                     ctypes.byref(self._ctx))
        if rc:
            raise UmxError(rc, self._L.umx_last_error(None).decode())
        self.device = device
        self.max_batch = max_batch
        self.precision = {PREC_F32: "f32", PREC_F16X3: "f16x3", PREC_F16X3_F6: "f16f6"}[self._L.umx_precision_of(self._ctx)]
        self.note = ""
        if precision == "default" and self.precision == "f32":   # the planner of the fast kernels refused the model: say so
            import warnings
            self.note = self._L.umx_last_error(self._ctx).decode()
            if self.note.startswith("note:"):   # (not when UMX_PRECISION=f32 asked for it)
                warnings.warn(self.note, RuntimeWarning, stacklevel=2)

    # -- lifetime
    def close(self) -> None:
        if getattr(self, "_ctx", None) and self._ctx.value:
            self._L.umx_destroy(self._ctx)
            self._ctx = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, rc: int) -> None:
        if rc:
            raise UmxError(rc, self._L.umx_last_error(self._ctx).decode())

    # -- plumbing
    # -- multi-GPU inside the library (RCCL over xGMI): see include/umx.h
    @staticmethod
    def shard_unique_id() -> bytes:
        buf = ctypes.create_string_buffer(128)
        rc = load().umx_shard_unique_id(buf)
        if rc:
            raise UmxError(rc, load().umx_last_error(None).decode())
        return buf.raw

    def shard_init(self, unique_id: bytes, rank: int, world: int) -> None:
        self._check(self._L.umx_shard_init(self._ctx, ctypes.create_string_buffer(unique_id, 128), int(rank), int(world)))

    def shard_fini(self) -> None:
        """umx_shard_fini: drop the communicator / transport (after a failure: ncclCommAbort instead of ncclCommDestroy)."""
        self._check(self._L.umx_shard_fini(self._ctx))

    def shard_init_transport(self, send, recv, all_gather, rank: int, world: int, group_start=None, group_end=None) -> None:
        """umx_shard_init_transport with Python callables: send(dev_ptr, nbytes, peer, stream), recv(dev_ptr, nbytes, peer, stream),
        all_gather(send_ptr, recv_ptr, nbytes_per_rank, stream), group_start() / group_end(); an exception = failure."""
        def guard(fn):
            def call(user, *a):
                try:
                    fn(*a)
                    return 0
                except Exception:   # noqa: BLE001  (nothing may propagate through the C frames)
                    import traceback
                    traceback.print_exc()
                    return 1
            return call
        t = ShardTransport(None, _SEND_FN(guard(send)), _SEND_FN(guard(recv)), _GATHER_FN(guard(all_gather)),
                           _GROUP_FN(guard(group_start)) if group_start else _GROUP_FN(), _GROUP_FN(guard(group_end)) if group_end else _GROUP_FN())
        self._transport = t   # (the callbacks must outlive the context's use of them)
        self._check(self._L.umx_shard_init_transport(self._ctx, ctypes.byref(t), int(rank), int(world)))

    def shard_plan(self, H: int, W: int, rank: int, world: int, nslabs: int = 2, slab: int = 0) -> dict:
        return shard_plan(self.hp, H, W, rank, world, nslabs, slab)

    def infer_image_sharded_dev(self, band_ptr: int, C: int, H: int, W: int, band_row0: int, band_rows: int, mean: float,
                                std: float, mode: int, stitch: int, nslabs: int, out_full_ptr: int) -> None:
        self._check(self._L.umx_infer_image_sharded_dev(self._ctx, ctypes.c_void_p(band_ptr), C, H, W, int(band_row0),
                                                        int(band_rows), float(mean), float(std), int(mode), int(stitch),
                                                        int(nslabs), ctypes.c_void_p(out_full_ptr)))

    def infer_image_sharded_raw_submit(self, slot: int, band_ptr: int, bits: int, C: int, H: int, W: int, band_row0: int,
                                       band_rows: int, value_range, mean: float, std: float, mode: int, nslabs: int,
                                       own_out_ptr: int = 0, out_full_ptr: int = 0) -> None:
        """umx_infer_image_sharded_raw_submit: this rank's raw rows (host pointer) in, uint8 planes out -- the rank's own rows to
        ``own_out_ptr`` (host, [K, own rows, W]) and the gathered stack to ``out_full_ptr`` (device, [K, H, W]); 0 = none / the
        library's buffer.  ``value_range``: None, or per plane (min, max) of the WHOLE plane (the drivers' rescale).
        ``infer_image_wait(slot)`` completes the call."""
        rng = None
        if value_range is not None:
            rng = (ctypes.c_uint32 * (2 * C))(*[int(v) for pair in value_range for v in pair])
        self._check(self._L.umx_infer_image_sharded_raw_submit(
            self._ctx, int(slot), ctypes.c_void_p(band_ptr), int(bits), C, H, W, int(band_row0), int(band_rows), rng, float(mean),
            float(std), int(mode), int(nslabs), ctypes.c_void_p(own_out_ptr or None), ctypes.c_void_p(out_full_ptr or None)))

    def infer_image_sharded_raw(self, band: np.ndarray, H: int, W: int, band_row0: int, value_range, mean: float, std: float,
                                mode: int = MODE_ACCUMULATE, nslabs: int = 2, own_rows: int = 0, out_full_ptr: int = 0):
        """Synchronous form on a numpy band [C, rows, W] (or [rows, W]) of uint8 / uint16: returns this rank's own rows as uint8
        [K, own_rows, W] (``own_rows`` from shard_plan: own_row1 - own_row0)."""
        b = np.ascontiguousarray(band)
        if b.ndim == 2:
            b = b[None]
        if b.dtype not in (np.uint8, np.uint16):
            raise TypeError("raw planes must be uint8 or uint16")
        out = np.empty((self.hp.nClasses, int(own_rows), W), dtype=np.uint8)
        self.infer_image_sharded_raw_submit(0, b.ctypes.data, 8 * b.dtype.itemsize, b.shape[0], H, W, band_row0, b.shape[1], value_range,
                                            mean, std, mode, nslabs, out.ctypes.data if out.size else 0, out_full_ptr)
        self.infer_image_wait(0)
        return out

    def set_stream(self, hip_stream) -> None:
        """Run the engine's launches on the caller's HIP stream (a non-zero hipStream_t handle, e.g.
        ``torch.cuda.Stream().cuda_stream``); ``None`` restores the engine's own stream.  The legacy default stream
        (handle 0 -- what ``torch.cuda.current_stream()`` is unless a ``torch.cuda.stream`` context is active) is
        refused: the C ABI reads NULL as "own stream", and that stream is non-blocking, so engine work would NOT be
        ordered against the caller's default-stream work."""
        if hip_stream is None:
            hip_stream = 0
        elif int(hip_stream) == 0:
            raise ValueError("set_stream(0): the legacy default stream cannot be shared with the engine; run the caller's "
                             "work under a dedicated torch.cuda.Stream and pass its cuda_stream handle (None = own stream)")
        self._check(self._L.umx_set_stream(self._ctx, ctypes.c_void_p(int(hip_stream))))

    def synchronize(self) -> None:
        self._check(self._L.umx_synchronize(self._ctx))

    def tile_grid(self, H: int, W: int):
        a, b, c, d = (ctypes.c_int() for _ in range(4))
        self._check(self._L.umx_tile_grid(self._ctx, H, W, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c),
                                          ctypes.byref(d)))
        return a.value, b.value, c.value, d.value

    # -- host-pointer API
    def forward_tiles(self, tiles: np.ndarray) -> np.ndarray:
        """== Session.run(UNet2D.nn, {tfData: tiles, tfTraining: 0}) (reference UnMicst1-5.py:704)."""
        hp = self.hp
        tiles = np.ascontiguousarray(tiles, dtype=np.float32)
        if tiles.ndim != 4 or tiles.shape[1:] != (hp.imSize, hp.imSize, hp.nChannels):
            raise ValueError("tiles must be [n,%d,%d,%d]" % (hp.imSize, hp.imSize, hp.nChannels))
        out = np.empty((tiles.shape[0], hp.imSize, hp.imSize, hp.nClasses), np.float32)
        self._check(self._L.umx_forward_tiles(self._ctx, tiles.ctypes.data, tiles.shape[0], out.ctypes.data))
        return out

    def infer_image(self, image: np.ndarray, mean: float, std: float, mode: int = MODE_ACCUMULATE,
                    stitch: int = STITCH_FP16_COMPAT) -> np.ndarray:
        """All-class whole-image inference: image float64 (H,W) or (C,H,W) -> [K,H,W] float16 / float32."""
        image = np.ascontiguousarray(image, dtype=np.float64)
        if image.ndim == 2:
            image = image[None]
        if image.ndim != 3:
            raise ValueError("image must be (H,W) or (C,H,W)")
        C, H, W = image.shape
        out = np.empty((self.hp.nClasses, H, W), np.float32 if stitch == STITCH_FP32 else np.float16)
        self._check(self._L.umx_infer_image(self._ctx, image.ctypes.data, C, H, W, float(mean), float(std), int(mode),
                                            int(stitch), out.ctypes.data))
        return out

    def infer_image_ptr(self, image_ptr: int, C: int, H: int, W: int, mean: float, std: float, out_ptr: int,
                        mode: int = MODE_ACCUMULATE, stitch: int = STITCH_FP16_COMPAT) -> None:
        """umx_infer_image on raw HOST addresses (e.g. pinned buffers: the slab-wise uploads / downloads are then true DMA
        under the tile kernels): float64 [C,H,W] in, [K,H,W] float16 / float32 out."""
        self._check(self._L.umx_infer_image(self._ctx, ctypes.c_void_p(image_ptr), C, H, W, float(mean), float(std),
                                            int(mode), int(stitch), ctypes.c_void_p(out_ptr)))

    def infer_image_raw_range_ptr(self, raw_ptr: int, bits: int, C: int, H: int, W: int, value_range, mean: float, std: float,
                                  out_ptr: int, mode: int = MODE_ACCUMULATE) -> None:
        """umx_infer_image_raw_range on raw HOST addresses (rescale implied; value_range: per plane (min, max))."""
        rng = np.ascontiguousarray(np.asarray(value_range, dtype=np.uint32).reshape(C, 2))
        self._check(self._L.umx_infer_image_raw_range(self._ctx, ctypes.c_void_p(raw_ptr), int(bits), C, H, W, rng.ctypes.data,
                                                      float(mean), float(std), int(mode), ctypes.c_void_p(out_ptr)))

    def infer_image_raw_ptr(self, raw_ptr: int, bits: int, C: int, H: int, W: int, rescale: bool, mean: float, std: float,
                            out_ptr: int, mode: int = MODE_ACCUMULATE) -> None:
        """umx_infer_image_raw on raw HOST addresses: uint8 / uint16 [C,H,W] in, uint8 [K,H,W] out."""
        self._check(self._L.umx_infer_image_raw(self._ctx, ctypes.c_void_p(raw_ptr), int(bits), C, H, W, int(bool(rescale)),
                                                float(mean), float(std), int(mode), ctypes.c_void_p(out_ptr)))

    def infer_image_raw_submit(self, slot: int, raw_ptr: int, bits: int, C: int, H: int, W: int, rescale: bool, mean: float,
                               std: float, out_ptr: int, mode: int = MODE_ACCUMULATE) -> None:
        """Enqueue one slide on `slot` (0 / 1) and return; pair with infer_image_wait(slot).  HOST addresses."""
        self._check(self._L.umx_infer_image_raw_submit(self._ctx, int(slot), ctypes.c_void_p(raw_ptr), int(bits), C, H, W,
                                                       int(bool(rescale)), float(mean), float(std), int(mode),
                                                       ctypes.c_void_p(out_ptr)))

    def infer_image_wait(self, slot: int) -> None:
        self._check(self._L.umx_infer_image_wait(self._ctx, int(slot)))

    def infer_image_raw(self, raw: np.ndarray, rescale: bool, mean: float, std: float,
                        mode: int = MODE_ACCUMULATE, value_range=None) -> np.ndarray:
        """Driver fast path at scalingFactor 1: raw uint8/uint16 (H,W) or (C,H,W) -> uint8 [K,H,W] (see include/umx.h).
        value_range (with rescale): per plane (min, max) of the raw samples, as the reader found them (umx_infer_image_raw_range:
        the upload then overlaps the tile kernels in this synchronous call too)."""
        raw = np.ascontiguousarray(raw)
        if raw.dtype not in (np.uint8, np.uint16):
            raise TypeError("raw planes must be uint8 or uint16")
        if raw.ndim == 2:
            raw = raw[None]
        if raw.ndim != 3:
            raise ValueError("raw must be (H,W) or (C,H,W)")
        C, H, W = raw.shape
        raw = raw.astype(raw.dtype.newbyteorder("="), copy=False)
        out = np.empty((self.hp.nClasses, H, W), np.uint8)
        if rescale and value_range is not None:
            rng = np.ascontiguousarray(np.asarray(value_range, dtype=np.uint32).reshape(C, 2))
            self._check(self._L.umx_infer_image_raw_range(self._ctx, raw.ctypes.data, raw.dtype.itemsize * 8, C, H, W, rng.ctypes.data,
                                                          float(mean), float(std), int(mode), out.ctypes.data))
            return out
        self._check(self._L.umx_infer_image_raw(self._ctx, raw.ctypes.data, raw.dtype.itemsize * 8, C, H, W,
                                                1 if rescale else 0, float(mean), float(std), int(mode), out.ctypes.data))
        return out

    def infer_image_raw_scaled(self, raw: np.ndarray, scaling: float, rescale: bool, mean: float, std: float,
                               mode: int = MODE_ACCUMULATE) -> np.ndarray:
        """The drivers' recipe at --scalingFactor != 1 on the device: raw uint8/uint16 (H,W) or (C,H,W) -> uint8 [K,H,W]."""
        raw = np.ascontiguousarray(raw)
        if raw.dtype not in (np.uint8, np.uint16):
            raise TypeError("raw planes must be uint8 or uint16")
        if raw.ndim == 2:
            raw = raw[None]
        C, H, W = raw.shape
        raw = raw.astype(raw.dtype.newbyteorder("="), copy=False)
        out = np.empty((self.hp.nClasses, H, W), np.uint8)
        self._check(self._L.umx_infer_image_raw_scaled(self._ctx, raw.ctypes.data, raw.dtype.itemsize * 8, C, H, W,
                                                       float(scaling), 1 if rescale else 0, float(mean), float(std), int(mode),
                                                       out.ctypes.data))
        return out

    def infer_image_raw_outlier(self, raw: np.ndarray, scaling: float, outlier: float, mean: float, std: float,
                                mode: int = MODE_ACCUMULATE) -> np.ndarray:
        """The drivers' recipe with --outlier on the device (any --scalingFactor): intensities rescaled to
        (min, np.percentile(resized plane, outlier)) -> (0, 0.983); raw uint8/uint16 (H,W) or (C,H,W) -> uint8 [K,H,W]."""
        raw = np.ascontiguousarray(raw)
        if raw.dtype not in (np.uint8, np.uint16):
            raise TypeError("raw planes must be uint8 or uint16")
        if raw.ndim == 2:
            raw = raw[None]
        C, H, W = raw.shape
        raw = raw.astype(raw.dtype.newbyteorder("="), copy=False)
        out = np.empty((self.hp.nClasses, H, W), np.uint8)
        self._check(self._L.umx_infer_image_raw_outlier(self._ctx, raw.ctypes.data, raw.dtype.itemsize * 8, C, H, W,
                                                        float(scaling), float(outlier), float(mean), float(std), int(mode),
                                                        out.ctypes.data))
        return out

    # -- device-pointer API (pointers are plain ints, e.g. torch.Tensor.data_ptr())
    def forward_tiles_dev(self, tiles_ptr: int, n: int, probs_ptr: int) -> None:
        self._check(self._L.umx_forward_tiles_dev(self._ctx, ctypes.c_void_p(tiles_ptr), n, ctypes.c_void_p(probs_ptr)))

    def infer_image_dev(self, image_ptr: int, C: int, H: int, W: int, mean: float, std: float, mode: int, stitch: int,
                        out_ptr: int) -> None:
        self._check(self._L.umx_infer_image_dev(self._ctx, ctypes.c_void_p(image_ptr), C, H, W, float(mean),
                                                float(std), mode, stitch, ctypes.c_void_p(out_ptr)))

    def band_tiles_dev(self, image_ptr: int, C: int, H: int, W: int, band_row0: int, band_rows: int, mean: float,
                       std: float, pr0: int, pr1: int, probs_ptr: int) -> None:
        self._check(self._L.umx_band_tiles_dev(self._ctx, ctypes.c_void_p(image_ptr), C, H, W, band_row0, band_rows,
                                               float(mean), float(std), pr0, pr1, ctypes.c_void_p(probs_ptr)))

    def stitch_dev(self, probs_ptr: int, tpr0: int, tpr1: int, H: int, W: int, mode: int, stitch: int, y0: int,
                   y1: int, out_ptr: int) -> None:
        self._check(self._L.umx_stitch_dev(self._ctx, ctypes.c_void_p(probs_ptr), tpr0, tpr1, H, W, mode, stitch, y0,
                                           y1, ctypes.c_void_p(out_ptr)))

    # -- profiling
    def profile_enable(self, on) -> None:
        """False / 0: off; True / 1: two HIP events around every launch; N >= 2: around every N-th launch of each site."""
        self._check(self._L.umx_profile_enable(self._ctx, int(on)))

    def profile_read(self) -> List[dict]:
        n = ctypes.c_int()
        arr = (ProfEntry * 256)()
        self._check(self._L.umx_profile_read(self._ctx, arr, 256, ctypes.byref(n)))
        out = []
        for i in range(min(n.value, 256)):
            e = arr[i]
            out.append({"name": e.name.decode(), "kernel": e.kernel.decode(), "launches": int(e.launches),
                        "total_ms": float(e.total_ms), "flops": float(e.flops), "bytes": float(e.bytes),
                        "exec_flops": float(e.exec_flops), "seen": int(e.launches_seen), "xcd_order": int(e.xcd_order)})
        return out
