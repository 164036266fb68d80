"""ctypes binding of the training step of libumx (include/umx_train.h) and the host-side mirror of the reference's
training regimes.

``Trainer.step(batchData, batchLabels, batchWeights)`` is one ``sess.run([optOp, loss], feed_dict=...)`` of the
reference's loop (UnMicst1-5.py:483-484, UnMicst2.py:471-472); ``solo_options`` / ``duo_options`` carry the constants
those scripts hard-code (optimiser, learning-rate schedule, regularisers, dropout rates, the probability clip).  The legacy
graph of the shipped checkpoints trains with ``legacy_options`` (UnMicst.py:270-279: Momentum, unweighted loss -- ``weights``
may be None -- no dropout, no regulariser).  The trained parameters come back in the blob layout ``umx.Engine`` loads
(``Trainer.blob()``), so train -> infer needs no conversion.  No CPU fallback: without libumx and a gfx950 device every call raises.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass, fields
from typing import Optional

import numpy as np

from . import umx as _umx
from .model import GRAPH_LEGACY, GRAPH_V2, HParams

OPT_ADAM, OPT_MOMENTUM = 0, 1
REG_NONE, REG_L1, REG_L2 = 0, 1, 2
TV_PARAMS, TV_GRADS, TV_SLOT_M, TV_SLOT_V = 0, 1, 2, 3

# every symbol include/umx_train.h declares (checked by tests/test_abi.py)
EXPORTS = [
    "umx_train_options_solo", "umx_train_options_duo", "umx_train_options_legacy", "umx_trainer_create", "umx_trainer_destroy",
    "umx_trainer_last_error", "umx_train_step", "umx_train_step_dev", "umx_trainer_loss", "umx_trainer_read",
    "umx_trainer_probs", "umx_trainer_read_tensor", "umx_trainer_eval", "umx_trainer_step_count", "umx_trainer_batch", "umx_trainer_flops_per_image",
    "umx_trainer_profile", "umx_test_trainer_serial", "umx_trainset_create", "umx_trainset_set", "umx_trainset_destroy", "umx_train_step_sampled",
    "umx_trainer_assemble", "umx_trainer_evaluate", "umx_guard_scan", "umx_augment_table_check", "umx_trainset_set_augment",
    "umx_train_step_augmented", "umx_trainer_assemble_augmented", "umx_warp_desc_check", "umx_train_step_warped",
    "umx_trainer_assemble_warped", "umx_trainer_init", "umx_elastic_desc_check", "umx_train_step_elastic",
    "umx_trainer_assemble_elastic", "umx_border_options_check", "umx_trainset_border_weights", "umx_trainset_border_planes",
    "umx_object_options_check", "umx_trainer_evaluate_objects", "umx_trainer_object_counts",
]


class _TrainOptions(ctypes.Structure):
    _fields_ = [("device_ordinal", ctypes.c_int32), ("batch", ctypes.c_int32), ("optimizer", ctypes.c_int32),
                ("decay_steps", ctypes.c_int32), ("lr0", ctypes.c_float), ("decay_rate", ctypes.c_float),
                ("momentum", ctypes.c_float), ("beta1", ctypes.c_float), ("beta2", ctypes.c_float),
                ("adam_eps", ctypes.c_float), ("reg_kind", ctypes.c_int32), ("reg_down", ctypes.c_float),
                ("reg_bottom", ctypes.c_float), ("reg_up", ctypes.c_float), ("reg_top", ctypes.c_float),
                ("clip_eps", ctypes.c_float), ("drop_down_step", ctypes.c_float), ("drop_bottom", ctypes.c_float),
                ("drop_up0", ctypes.c_float), ("drop_up_step", ctypes.c_float), ("bn_momentum", ctypes.c_float),
                ("seed", ctypes.c_uint64), ("reserved", ctypes.c_int32 * 8)]


class _InitOptions(ctypes.Structure):
    """``umx_init_options`` (include/umx_train.h)."""
    _fields_ = [("seed", ctypes.c_uint64), ("std_dev0", ctypes.c_float), ("reserved", ctypes.c_int32 * 5)]


# the reference's stdDev0 where a model directory has no hp.data: its own UNet2D.setup(...) example (UnMicstCyto2.py:689)
DEFAULT_STD_DEV0 = 0.007


@dataclass
class TrainOptions:
    """Field-for-field ``umx_train_options``; the defaults are the solo script's (UnMicst1-5.py:84,139,362-378)."""
    optimizer: int = OPT_ADAM
    lr0: float = 5e-5
    decay_steps: int = 5000
    decay_rate: float = 0.98
    momentum: float = 0.9
    beta1: float = 0.9
    beta2: float = 0.999
    adam_eps: float = 1e-8
    reg_kind: int = REG_L1
    reg_down: float = 8e-5
    reg_bottom: float = 8e-5
    reg_up: float = 8e-5
    reg_top: float = 8e-5
    clip_eps: float = 1e-7
    drop_down_step: float = 0.0
    drop_bottom: float = 0.35
    drop_up0: float = 0.0
    drop_up_step: float = 0.0
    bn_momentum: float = 0.99
    seed: int = 1234


class LabelWeightsC(ctypes.Structure):
    """``umx_label_weights`` (include/umx_train.h)."""
    _fields_ = [("weighted", ctypes.c_int32), ("class_weight", ctypes.c_float * 8), ("intersect_weight", ctypes.c_float * 8),
                ("reserved", ctypes.c_int32 * 7)]


# ``umx_sample_desc`` (include/umx_train.h): one image of a batch drawn from a training set, 32 bytes
SAMPLE_DESC = np.dtype([("index", "<i4"), ("page", "<i4"), ("y0", "<i4"), ("x0", "<i4"), ("transform", "<i4"),
                        ("brightness", "<f4"), ("contrast", "<f4"), ("reserved", "<i4")])

# ``umx_augment_desc``: the blur level and saturation gain of one image, parallel to its SAMPLE_DESC
AUGMENT_DESC = np.dtype([("blur_level", "<i4"), ("gain", "<f4")])
AUGMENT_MAX_LEVELS, AUGMENT_MAX_RADIUS = 16, 12

# ``umx_warp_desc``: rotation and zoom of one image, parallel to its SAMPLE_DESC; (sy, sx) = M (y - c, x - c) + the crop's centre
WARP_DESC = np.dtype([("m", "<f4", (4,))])

# ``umx_elastic_desc``: the displacement lattice of one image, parallel to its SAMPLE_DESC, 304 bytes; n = 0 (no deformation) or 4..6
# lattice points per axis, d[0] / d[1] the row / column displacements in pixels (zero outside the n x n block)
ELASTIC_MAX_GRID, ELASTIC_MAX_DISP = 6, 32.0
ELASTIC_DESC = np.dtype([("n", "<i4"), ("reserved", "<i4", (3,)), ("d", "<f4", (2, ELASTIC_MAX_GRID, ELASTIC_MAX_GRID))])

# the arrays parallel to SAMPLE_DESC in the order the entries take them, as Trainer's messages name them
_PARALLEL_DESCS = ((AUGMENT_DESC, "augmentation", "AUGMENT_DESC"), (WARP_DESC, "warp", "WARP_DESC"), (ELASTIC_DESC, "elastic", "ELASTIC_DESC"))


class AugmentTableC(ctypes.Structure):
    """``umx_augment_table`` (include/umx_train.h)."""
    _fields_ = [("mean", ctypes.c_float), ("std", ctypes.c_float), ("n_levels", ctypes.c_int32),
                ("radius", ctypes.c_int32 * AUGMENT_MAX_LEVELS), ("taps", (ctypes.c_float * (AUGMENT_MAX_RADIUS + 1)) * AUGMENT_MAX_LEVELS),
                ("reserved", ctypes.c_int32 * 5)]


# ``umx_border_options``: the computed border weight map of a sample ("Border weight maps")
BORDER_MAX_SIGMA, BORDER_CONNECTIVITY = 8.0, 4


class BorderOptionsC(ctypes.Structure):
    """``umx_border_options`` (include/umx_train.h)."""
    _fields_ = [("object_code", ctypes.c_int32), ("sigma", ctypes.c_float), ("reserved", ctypes.c_int32 * 6)]


# ``umx_object_options``: the object score of the validation pass ("Object score")
OBJECT_COUNTS, OBJECT_MAX_MIN_AREA = 8, 65536
OBJECT_COUNT_NAMES = ("truth", "predicted", "matched", "matched75", "merged", "split")


class ObjectOptionsC(ctypes.Structure):
    """``umx_object_options`` (include/umx_train.h)."""
    _fields_ = [("object_code", ctypes.c_int32), ("min_area", ctypes.c_int32), ("reserved", ctypes.c_int32 * 6)]


def object_f1(matched: int, truth: int, predicted: int) -> float:
    """``2 matched / (truth + predicted)``; NaN when there is no object on either side."""
    return 2.0 * matched / (truth + predicted) if truth + predicted else float("nan")


def solo_options(**kw) -> TrainOptions:
    return TrainOptions(**kw)


def duo_options(**kw) -> TrainOptions:
    """UnMicst2.py:82,114,123,137,158,203,211,357-371."""
    base = dict(lr0=6e-5, decay_steps=4000, decay_rate=0.99, reg_kind=REG_L2, reg_down=0.01, reg_bottom=0.01,
                reg_up=0.005, reg_top=0.005, clip_eps=0.0, drop_down_step=0.05, drop_bottom=0.3, drop_up0=0.25,
                drop_up_step=0.05)
    base.update(kw)
    return TrainOptions(**base)


def legacy_options(**kw) -> TrainOptions:
    """UnMicst.py:270-279 (train() of the legacy graph): MomentumOptimizer(0.01 * 0.95^floor(step/1000), 0.9), the
    unweighted, unclipped cross-entropy, no regulariser, no dropout."""
    base = dict(optimizer=OPT_MOMENTUM, lr0=0.01, decay_steps=1000, decay_rate=0.95, momentum=0.9, reg_kind=REG_NONE,
                reg_down=0.0, reg_bottom=0.0, reg_up=0.0, reg_top=0.0, clip_eps=0.0, drop_bottom=0.0)
    base.update(kw)
    return TrainOptions(**base)


def _legacy_refusal(opts: TrainOptions) -> Optional[str]:
    if opts.reg_kind != REG_NONE or any(getattr(opts, k) != 0.0 for k in ("drop_down_step", "drop_bottom", "drop_up0", "drop_up_step")):
        return ("the legacy graph has no dropout and no regulariser: train it with legacy_options() "
                "(reference UnMicst.py:270-279)")
    return None


def _bind(L):
    if getattr(L, "_umx_train_bound", False):
        return L
    c_int, c_void_p = ctypes.c_int, ctypes.c_void_p
    dp = ctypes.POINTER(ctypes.c_double)
    L.umx_train_options_solo.restype = None
    L.umx_train_options_solo.argtypes = [ctypes.POINTER(_TrainOptions)]
    L.umx_train_options_duo.restype = None
    L.umx_train_options_duo.argtypes = [ctypes.POINTER(_TrainOptions)]
    L.umx_train_options_legacy.restype = None
    L.umx_train_options_legacy.argtypes = [ctypes.POINTER(_TrainOptions)]
    L.umx_trainer_create.restype = c_int
    L.umx_trainer_create.argtypes = [ctypes.POINTER(_umx._HP), c_void_p, ctypes.c_size_t, ctypes.POINTER(_TrainOptions),
                                     ctypes.POINTER(c_void_p)]
    L.umx_trainer_destroy.restype = None
    L.umx_trainer_destroy.argtypes = [c_void_p]
    L.umx_trainer_init.restype = c_int
    L.umx_trainer_init.argtypes = [c_void_p, ctypes.POINTER(_InitOptions)]
    L.umx_trainer_last_error.restype = ctypes.c_char_p
    L.umx_trainer_last_error.argtypes = [c_void_p]
    L.umx_train_step.restype = c_int
    L.umx_train_step.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_int, dp]
    L.umx_train_step_dev.restype = c_int
    L.umx_train_step_dev.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_int]
    L.umx_trainer_loss.restype = c_int
    L.umx_trainer_loss.argtypes = [c_void_p, dp]
    L.umx_trainer_read.restype = c_int
    L.umx_trainer_read.argtypes = [c_void_p, c_int, c_void_p, ctypes.c_size_t]
    L.umx_trainer_probs.restype = c_int
    L.umx_trainer_probs.argtypes = [c_void_p, c_void_p]
    L.umx_trainer_read_tensor.restype = c_int
    L.umx_trainer_read_tensor.argtypes = [c_void_p, ctypes.c_char_p, c_void_p, ctypes.POINTER(ctypes.c_size_t)]
    L.umx_trainer_eval.restype = c_int
    L.umx_trainer_eval.argtypes = [c_void_p, c_void_p, c_void_p]
    L.umx_trainer_step_count.restype = ctypes.c_int64
    L.umx_trainer_step_count.argtypes = [c_void_p]
    L.umx_trainer_batch.restype = c_int
    L.umx_trainer_batch.argtypes = [c_void_p]
    L.umx_trainer_flops_per_image.restype = ctypes.c_double
    L.umx_trainer_flops_per_image.argtypes = [c_void_p]
    L.umx_trainer_profile.restype = c_int
    L.umx_trainer_profile.argtypes = [c_void_p, c_int, dp, dp, dp, ctypes.POINTER(c_int)]
    L.umx_test_trainer_serial.restype = c_int
    L.umx_test_trainer_serial.argtypes = [c_void_p, c_int]
    # the device-resident training set (unmicst_amd/trainset.py)
    L.umx_trainset_create.restype = c_int
    L.umx_trainset_create.argtypes = [c_void_p, c_int, c_int, c_int, ctypes.POINTER(LabelWeightsC), ctypes.POINTER(c_void_p)]
    L.umx_trainset_set.restype = c_int
    L.umx_trainset_set.argtypes = [c_void_p, c_int, c_void_p, c_void_p, c_void_p]
    L.umx_trainset_destroy.restype = None
    L.umx_trainset_destroy.argtypes = [c_void_p]
    L.umx_train_step_sampled.restype = c_int
    L.umx_train_step_sampled.argtypes = [c_void_p, c_void_p, c_void_p, c_int]
    L.umx_trainer_assemble.restype = c_int
    L.umx_trainer_assemble.argtypes = [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p]
    L.umx_trainer_evaluate.restype = c_int
    L.umx_trainer_evaluate.argtypes = [c_void_p, c_void_p, c_void_p, c_int, ctypes.POINTER(ctypes.c_int64), dp]
    # computed defocus / saturation (umx_augment_table, umx_augment_desc)
    L.umx_augment_table_check.restype = c_int
    L.umx_augment_table_check.argtypes = [ctypes.POINTER(AugmentTableC), ctypes.c_char_p, ctypes.c_size_t]
    L.umx_trainset_set_augment.restype = c_int
    L.umx_trainset_set_augment.argtypes = [c_void_p, ctypes.POINTER(AugmentTableC)]
    L.umx_train_step_augmented.restype = c_int
    L.umx_train_step_augmented.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_int]
    L.umx_trainer_assemble_augmented.restype = c_int
    L.umx_trainer_assemble_augmented.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p]
    # rotation and zoom (umx_warp_desc)
    L.umx_warp_desc_check.restype = c_int
    L.umx_warp_desc_check.argtypes = [c_void_p, c_int, ctypes.c_char_p, ctypes.c_size_t]
    L.umx_train_step_warped.restype = c_int
    L.umx_train_step_warped.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int]
    L.umx_trainer_assemble_warped.restype = c_int
    L.umx_trainer_assemble_warped.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p]
    # elastic deformation (umx_elastic_desc)
    L.umx_elastic_desc_check.restype = c_int
    L.umx_elastic_desc_check.argtypes = [c_void_p, c_int, ctypes.c_char_p, ctypes.c_size_t]
    L.umx_train_step_elastic.restype = c_int
    L.umx_train_step_elastic.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int]
    L.umx_trainer_assemble_elastic.restype = c_int
    L.umx_trainer_assemble_elastic.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p]
    # border weight maps (umx_border_options)
    L.umx_border_options_check.restype = c_int
    L.umx_border_options_check.argtypes = [ctypes.POINTER(BorderOptionsC), c_int, ctypes.c_char_p, ctypes.c_size_t]
    L.umx_trainset_border_weights.restype = c_int
    L.umx_trainset_border_weights.argtypes = [c_void_p, c_int, ctypes.POINTER(BorderOptionsC)]
    L.umx_trainset_border_planes.restype = c_int
    L.umx_trainset_border_planes.argtypes = [c_void_p, c_int, ctypes.POINTER(BorderOptionsC), c_void_p, c_void_p, c_void_p, c_void_p]
    # object score (umx_object_options)
    L.umx_object_options_check.restype = c_int
    L.umx_object_options_check.argtypes = [ctypes.POINTER(ObjectOptionsC), c_int, ctypes.c_char_p, ctypes.c_size_t]
    L.umx_trainer_evaluate_objects.restype = c_int
    L.umx_trainer_evaluate_objects.argtypes = [c_void_p, c_void_p, c_void_p, c_int, ctypes.POINTER(ObjectOptionsC),
                                               ctypes.POINTER(ctypes.c_int64), dp, ctypes.POINTER(ctypes.c_int64), c_void_p, c_void_p]
    L.umx_trainer_object_counts.restype = c_int
    L.umx_trainer_object_counts.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_int, ctypes.POINTER(ObjectOptionsC), c_void_p,
                                            c_void_p, c_void_p]
    # debug guard mode (UMX_DEBUG_GUARD): the host scan of one red zone
    L.umx_guard_scan.restype = c_int
    L.umx_guard_scan.argtypes = [c_void_p, ctypes.c_size_t, c_int, ctypes.c_size_t, c_int, ctypes.c_char_p, ctypes.c_char_p,
                                 ctypes.c_size_t]
    L._umx_train_bound = True
    return L


def native_options(kind: str) -> TrainOptions:
    """The presets as libumx fills them (umx_train_options_solo/_duo/_legacy) -- tests compare them with the dataclasses."""
    L = _bind(_umx.load())
    o = _TrainOptions()
    fill = {"solo": L.umx_train_options_solo, "legacy": L.umx_train_options_legacy}.get(kind, L.umx_train_options_duo)
    fill(ctypes.byref(o))
    return TrainOptions(**{f.name: getattr(o, f.name) for f in fields(TrainOptions)})


class Trainer:
    def __init__(self, hp: HParams, blob: np.ndarray, opts: Optional[TrainOptions] = None, batch: int = 0,
                 device: int = 0):
        self.opts = opts or TrainOptions()
        if hp.graph == GRAPH_LEGACY:
            if not 0 <= hp.nExtraConvs <= 2:
                raise ValueError("the training step covers the legacy graph with nExtraConvs 0..2")
            why = _legacy_refusal(self.opts)
            if why:
                raise ValueError(why)
        elif hp.graph != GRAPH_V2 or hp.nExtraConvs != 0:
            raise ValueError("the training step covers the v2 graph with nExtraConvs == 0")
        self._lib = _bind(_umx.load())
        self.hp = hp
        o = _TrainOptions()
        for f in fields(TrainOptions):
            setattr(o, f.name, getattr(self.opts, f.name))
        o.device_ordinal = int(device)
        o.batch = int(batch) if batch else int(hp.batchSize)
        blob = np.ascontiguousarray(blob, dtype=np.float32)
        self.nparams = int(blob.size)
        h = ctypes.c_void_p()
        hps = _umx._hp_struct(hp)
        rc = self._lib.umx_trainer_create(ctypes.byref(hps), blob.ctypes.data, blob.size, ctypes.byref(o), ctypes.byref(h))
        if rc != _umx.UMX_OK:
            raise _umx.UmxError(rc, (self._lib.umx_trainer_last_error(None) or b"").decode())
        self._h = h
        self.batch = int(self._lib.umx_trainer_batch(h))
        self.device = int(device)

    @classmethod
    def from_scratch(cls, hp: HParams, opts: Optional[TrainOptions], init_seed: int, std_dev0: float, batch: int = 0,
                     device: int = 0) -> "Trainer":
        """A trainer whose variables are the graph's initial state (``tf.global_variables_initializer()``):
        created from a zero blob of the graph's length, then initialised on the device (``init``)."""
        from .model import tensor_specs
        n = sum(int(np.prod(shape)) for _, shape in tensor_specs(hp))
        tr = cls(hp, np.zeros(n, np.float32), opts, batch=batch, device=device)
        try:
            tr.init(init_seed, std_dev0)
        except Exception:
            tr.close()
            raise
        return tr

    def init(self, seed: int, std_dev0: float):
        """Replace the variables by the initial state of (seed, std_dev0) (umx_trainer_init): truncated-normal filters, BN at its
        identity; gradients and optimiser slots zeroed, step counter 0.  The dropout stream (``TrainOptions.seed``) is not touched."""
        o = _InitOptions()
        o.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        o.std_dev0 = float(std_dev0)
        self._check(self._lib.umx_trainer_init(self._h, ctypes.byref(o)))

    # ------------------------------------------------------------------------------------------
    def _check(self, rc):
        if rc != _umx.UMX_OK:
            raise _umx.UmxError(rc, (self._lib.umx_trainer_last_error(self._h) or b"").decode())

    def close(self):
        if getattr(self, "_h", None):
            for ts in list(getattr(self, "_sets", ())):   # a training set lives in this trainer's memory: it goes first
                ts.close()
            self._lib.umx_trainer_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _batch_arrays(self, data, labels, weights):
        hp, B = self.hp, self.batch
        if weights is None and hp.graph != GRAPH_LEGACY:
            raise ValueError("weights=None (the unweighted loss) is the legacy graph's; the v2 loss needs weights")
        d = np.ascontiguousarray(data, dtype=np.float32)
        y = np.ascontiguousarray(labels, dtype=np.float32)
        w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float32)
        if d.shape != (B, hp.imSize, hp.imSize, hp.nChannels):
            raise ValueError("data must be %r, got %r" % ((B, hp.imSize, hp.imSize, hp.nChannels), d.shape))
        if y.shape != (B, hp.imSize, hp.imSize, hp.nClasses) or (w is not None and w.shape != y.shape):
            raise ValueError("labels / weights must be %r" % ((B, hp.imSize, hp.imSize, hp.nClasses),))
        return d, y, w

    def step(self, data, labels, weights=None, apply_update: bool = True):
        """-> (loss, data term, regularisation loss) of this batch; parameters updated unless apply_update is False.
        weights None (legacy graph only): the unweighted loss of UnMicst.py:276."""
        d, y, w = self._batch_arrays(data, labels, weights)
        out = (ctypes.c_double * 3)()
        self._check(self._lib.umx_train_step(self._h, d.ctypes.data, y.ctypes.data, None if w is None else w.ctypes.data,
                                             int(apply_update), out))
        return float(out[0]), float(out[1]), float(out[2])

    def step_dev(self, data_ptr: int, labels_ptr: int, weights_ptr: Optional[int], apply_update: bool = True):
        """Device pointers (e.g. torch tensors' data_ptr()); only enqueues -- call loss() to synchronise.  weights_ptr None or 0:
        the unweighted loss (legacy graph only)."""
        if not weights_ptr and self.hp.graph != GRAPH_LEGACY:
            raise ValueError("weights_ptr is required for the v2 graph")
        self._check(self._lib.umx_train_step_dev(self._h, ctypes.c_void_p(data_ptr), ctypes.c_void_p(labels_ptr),
                                                 ctypes.c_void_p(weights_ptr), int(apply_update)))

    def loss(self):
        out = (ctypes.c_double * 3)()
        self._check(self._lib.umx_trainer_loss(self._h, out))
        return float(out[0]), float(out[1]), float(out[2])

    def _read(self, which: int) -> np.ndarray:
        out = np.empty(self.nparams, np.float32)
        self._check(self._lib.umx_trainer_read(self._h, which, out.ctypes.data, out.size))
        return out

    def blob(self) -> np.ndarray:
        """Current variables (incl. BN moving statistics) in the weight-blob layout of umx.Engine."""
        return self._read(TV_PARAMS)

    def grads(self) -> np.ndarray:
        return self._read(TV_GRADS)

    def slots(self):
        return self._read(TV_SLOT_M), self._read(TV_SLOT_V)

    def read_tensor(self, name: str) -> np.ndarray:
        """A tensor of the last step's forward pass as a flat float32 array (umx_trainer_read_tensor: "ld0.z", "ld0.stat", "lu1.us",
        "ds2", ...; NHWC order)."""
        n = ctypes.c_size_t(0)
        self._check(self._lib.umx_trainer_read_tensor(self._h, name.encode(), None, ctypes.byref(n)))
        out = np.empty(n.value, dtype=np.float32)
        self._check(self._lib.umx_trainer_read_tensor(self._h, name.encode(), out.ctypes.data, ctypes.byref(n)))
        return out

    def probs(self) -> np.ndarray:
        hp = self.hp
        out = np.empty((self.batch, hp.imSize, hp.imSize, hp.nClasses), np.float32)
        self._check(self._lib.umx_trainer_probs(self._h, out.ctypes.data))
        return out

    def eval(self, data) -> np.ndarray:
        """Inference-mode forward of one batch with the current variables (``tfTraining: 0``) -> probabilities."""
        hp = self.hp
        d = np.ascontiguousarray(data, dtype=np.float32)
        if d.shape != (self.batch, hp.imSize, hp.imSize, hp.nChannels):
            raise ValueError("data must be %r, got %r" % ((self.batch, hp.imSize, hp.imSize, hp.nChannels), d.shape))
        out = np.empty((self.batch, hp.imSize, hp.imSize, hp.nClasses), np.float32)
        self._check(self._lib.umx_trainer_eval(self._h, d.ctypes.data, out.ctypes.data))
        return out

    # ---- the device-resident training set (unmicst_amd/trainset.py) ----------------------------
    def _descs(self, desc, n_max: int):
        d = np.ascontiguousarray(desc, dtype=SAMPLE_DESC)
        if d.ndim != 1 or not 1 <= d.size <= n_max:
            raise ValueError("expected 1..%d descriptors (a 1-d SAMPLE_DESC array), got shape %r" % (n_max, d.shape))
        return d

    def _set_batch(self, desc, parallel=(), step=None):
        """The arrays of one training-set entry: the descriptors, then ``parallel``, the entry's own arrays in the order AUGMENT_DESC,
        WARP_DESC, ELASTIC_DESC, one row per descriptor.  The last of them is the one the entry is named for; one in front of it may be
        None, and None stays None.  ``step``: the method's name where it takes exactly B descriptors."""
        d = self._descs(desc, self.batch)
        if step and d.size != self.batch:
            raise ValueError("%s takes exactly %d descriptors, got %d" % (step, self.batch, d.size))
        arrays = [d]
        for k, (rows, (dtype, what, name)) in enumerate(zip(parallel, _PARALLEL_DESCS)):
            if rows is None and k + 1 < len(parallel):
                arrays.append(None)
                continue
            a = np.ascontiguousarray(rows, dtype=dtype)
            if a.shape != (d.size,):
                raise ValueError("expected %d %s descriptors (a 1-d %s array), got shape %r" % (d.size, what, name, a.shape))
            arrays.append(a)
        return arrays

    def _batch_outputs(self, ts, n: int):
        hp, P = self.hp, self.hp.imSize
        data = np.empty((n, P, P, hp.nChannels), np.float32)
        labels = np.empty((n, P, P, hp.nClasses), np.float32)
        weights = np.empty((n, P, P, hp.nClasses), np.float32) if ts.weighted else None
        return data, labels, weights

    def _set_call(self, symbol: str, ts, *args):
        """The C entry ``symbol`` on (trainer, set, args): an array goes as its address, None as NULL."""
        self._check(getattr(self._lib, symbol)(self._h, ts._handle(), *(a.ctypes.data if isinstance(a, np.ndarray) else a for a in args)))

    def _assemble_call(self, symbol: str, ts, arrays):
        out = self._batch_outputs(ts, arrays[0].size)
        self._set_call(symbol, ts, *arrays, arrays[0].size, *out)
        return out

    def step_sampled(self, ts, desc, apply_update: bool = True):
        """One step on the batch that B descriptors draw from the training set ``ts`` (assembled on the device); only enqueues
        -- call loss() to synchronise and read the loss."""
        self._set_call("umx_train_step_sampled", ts, *self._set_batch(desc, (), "step_sampled"), int(apply_update))

    def assemble(self, ts, desc):
        """The batch that n <= B descriptors assemble, copied to the host: (data [n,P,P,C], labels [n,P,P,K], weights or None)."""
        return self._assemble_call("umx_trainer_assemble", ts, self._set_batch(desc))

    def step_augmented(self, ts, desc, aug, apply_update: bool = True):
        """``step_sampled`` with a blur level and a saturation gain per image (``aug``: B AUGMENT_DESC rows; the set needs a table,
        ``TrainSet.set_augment``).  Only enqueues."""
        self._set_call("umx_train_step_augmented", ts, *self._set_batch(desc, (aug,), "step_augmented"), int(apply_update))

    def assemble_augmented(self, ts, desc, aug):
        """``assemble`` with a blur level and a saturation gain per image."""
        return self._assemble_call("umx_trainer_assemble_augmented", ts, self._set_batch(desc, (aug,)))

    def step_warped(self, ts, desc, aug, warp, apply_update: bool = True):
        """``step_augmented`` with a rotation / zoom matrix per image (``warp``: B WARP_DESC rows, ``trainset.warp_matrix``).  ``aug``
        None: no blur and gain 1 for every image, and the set needs no table.  Only enqueues."""
        self._set_call("umx_train_step_warped", ts, *self._set_batch(desc, (aug, warp), "step_warped"), int(apply_update))

    def assemble_warped(self, ts, desc, aug, warp):
        """``assemble_augmented`` with a rotation / zoom matrix per image; ``aug`` may be None."""
        return self._assemble_call("umx_trainer_assemble_warped", ts, self._set_batch(desc, (aug, warp)))

    def step_elastic(self, ts, desc, aug, warp, elastic, apply_update: bool = True):
        """``step_warped`` with a displacement lattice per image (``elastic``: B ELASTIC_DESC rows, ``trainset.elastic_lattice``).
        ``aug`` None: no blur and gain 1; ``warp`` None: no rotation or zoom.  Only enqueues."""
        self._set_call("umx_train_step_elastic", ts, *self._set_batch(desc, (aug, warp, elastic), "step_elastic"), int(apply_update))

    def assemble_elastic(self, ts, desc, aug, warp, elastic):
        """``assemble_warped`` with a displacement lattice per image; ``aug`` and ``warp`` may be None."""
        return self._assemble_call("umx_trainer_assemble_elastic", ts, self._set_batch(desc, (aug, warp, elastic)))

    def evaluate(self, ts, descs, objects=None) -> dict:
        """The validation pass over any number of descriptors, B at a time (eval mode: moving statistics, no dropout):
        {"per_class_error": 1 - correct / labelled per class (nan for a class with no pixel; UnMicst1-5.py:386-397),
         "loss": mean -log p[label] over labelled pixels, "loss_sum": its sum, "counts": int64 [2, K] = correct | labelled}.
        ``objects`` (a ``trainset.ObjectOptions``): the object pass runs on the same forward (umx_trainer_evaluate_objects) and the
        result gains "objects": {"truth", "predicted", "matched", "matched75", "merged", "split"} summed over all chunks, and "f1" =
        2 matched / (truth + predicted) (nan without objects).  The other entries are what they are without it."""
        d = np.ascontiguousarray(descs, dtype=SAMPLE_DESC).reshape(-1)
        if d.size == 0:
            raise ValueError("no descriptors to evaluate")
        K = self.hp.nClasses
        total = np.zeros(2 * K, np.int64)
        loss_sum = 0.0
        part = np.zeros(2 * K, np.int64)
        ls = ctypes.c_double()
        i64p = ctypes.POINTER(ctypes.c_int64)
        oc = None if objects is None else objects.c_struct(K)
        obj_total, obj_part = np.zeros(OBJECT_COUNTS, np.int64), np.zeros(OBJECT_COUNTS, np.int64)
        for b0 in range(0, d.size, self.batch):
            chunk = np.ascontiguousarray(d[b0:b0 + self.batch])
            if oc is None:
                self._check(self._lib.umx_trainer_evaluate(self._h, ts._handle(), chunk.ctypes.data, chunk.size,
                                                           part.ctypes.data_as(i64p), ctypes.byref(ls)))
            else:
                self._check(self._lib.umx_trainer_evaluate_objects(self._h, ts._handle(), chunk.ctypes.data, chunk.size, ctypes.byref(oc),
                                                                   part.ctypes.data_as(i64p), ctypes.byref(ls),
                                                                   obj_part.ctypes.data_as(i64p), None, None))
                obj_total += obj_part
            total += part
            loss_sum += ls.value
        counts = total.reshape(2, K)
        with np.errstate(invalid="ignore", divide="ignore"):
            err = 1.0 - counts[0] / counts[1].astype(np.float64)
        n_lab = int(counts[1].sum())
        out = {"per_class_error": err, "loss": loss_sum / n_lab if n_lab else float("nan"), "loss_sum": loss_sum,
               "counts": counts}
        if oc is not None:
            o = {name: int(v) for name, v in zip(OBJECT_COUNT_NAMES, obj_total)}
            o["f1"] = object_f1(o["matched"], o["truth"], o["predicted"])
            out["objects"] = o
        return out

    def evaluate_objects(self, ts, desc, objects):
        """One chunk of n <= B descriptors through umx_trainer_evaluate_objects, with the planes: (counts int64 [2, K], loss_sum,
        objects int64 [8], truth_codes uint8 [n, P, P], pred_codes uint8 [n, P, P]).  Diagnostics and tests."""
        d = self._descs(desc, self.batch)
        K, P = self.hp.nClasses, self.hp.imSize
        oc = objects.c_struct(K)
        counts, obj = np.zeros(2 * K, np.int64), np.zeros(OBJECT_COUNTS, np.int64)
        ls = ctypes.c_double()
        truth, pred = np.empty((d.size, P, P), np.uint8), np.empty((d.size, P, P), np.uint8)
        i64p = ctypes.POINTER(ctypes.c_int64)
        self._check(self._lib.umx_trainer_evaluate_objects(self._h, ts._handle(), d.ctypes.data, d.size, ctypes.byref(oc),
                                                           counts.ctypes.data_as(i64p), ctypes.byref(ls), obj.ctypes.data_as(i64p),
                                                           truth.ctypes.data, pred.ctypes.data))
        return counts.reshape(2, K), ls.value, obj, truth, pred

    def object_counts(self, ts, truth, pred, options, labels: bool = False):
        """The object pass on n <= B pairs of class-code planes (uint8 [n, P, P]) given by the host (umx_trainer_object_counts): int64
        [n, 8] = truth, predicted, matched, matched75, merged, split, 0, 0 per image; with ``labels`` also the two int32 label planes
        [n, P, P] (1 + y * P + x of the component's first pixel, 0 off the objects)."""
        P = self.hp.imSize
        t = np.ascontiguousarray(truth, dtype=np.uint8)
        p = np.ascontiguousarray(pred, dtype=np.uint8)
        if t.ndim != 3 or t.shape[1:] != (P, P) or p.shape != t.shape or not 1 <= t.shape[0] <= self.batch:
            raise ValueError("truth and pred must both be [n, %d, %d] with 1 <= n <= %d, got %r and %r" % (P, P, self.batch, t.shape, p.shape))
        n = t.shape[0]
        oc = options.c_struct(self.hp.nClasses)
        per = np.zeros((n, OBJECT_COUNTS), np.int64)
        tl = np.empty((n, P, P), np.int32) if labels else None
        pl = np.empty((n, P, P), np.int32) if labels else None
        self._check(self._lib.umx_trainer_object_counts(self._h, ts._handle(), t.ctypes.data, p.ctypes.data, n, ctypes.byref(oc),
                                                        per.ctypes.data, None if tl is None else tl.ctypes.data,
                                                        None if pl is None else pl.ctypes.data))
        return (per, tl, pl) if labels else per

    @property
    def step_count(self) -> int:
        return int(self._lib.umx_trainer_step_count(self._h))

    @property
    def flops_per_image(self) -> float:
        return float(self._lib.umx_trainer_flops_per_image(self._h))

    def test_serial(self, on: bool = True) -> None:
        """umx_test_trainer_serial: the v2 step enqueues its whole schedule on the main stream, in plan order, without events."""
        self._check(self._lib.umx_test_trainer_serial(self._h, int(on)))

    def profile(self, enable: bool = True) -> dict:
        f, b, o = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        n = ctypes.c_int()
        self._check(self._lib.umx_trainer_profile(self._h, int(enable), ctypes.byref(f), ctypes.byref(b), ctypes.byref(o),
                                                  ctypes.byref(n)))
        return {"forward_ms": f.value, "backward_ms": b.value, "update_ms": o.value, "steps": n.value}
