"""A training set that lives in device memory, the sampler that draws batches from it, and the reader of the reference's
published annotation layout.

Layout (interface only; reference readers UnMicst1-5.py:295-312, UnMicst2.py:293-309, UnMicst.py:236-243), one triple per
sample ``i`` of a directory:

* ``I%05d_Img.tif``: ``n_pages x n_channels`` pages, page ``aug + n_pages * channel`` -- the extra pages are the "real
  augmentation" z-planes;
* ``I%05d_Ant.tif``: class codes, ``k + 1`` = class ``k`` (0 = unlabelled);
* ``I%05d_wt.tif``: the contour-intersection weight map (optional here: a missing one counts as 0, or -- ``upload(..., border=...)``,
  ``TrainSet.border_weights`` -- is computed on the device from the annotation).

``TrainSet`` uploads the normalised planes once (``umx_trainset_create`` / ``_set``); ``Sampler`` draws the 32-byte descriptors
(``trainer.SAMPLE_DESC``) of each batch; ``Trainer.step_sampled`` / ``assemble`` / ``evaluate`` build the batch on the device
(DESIGN.md section 9.2).  The labels and weights follow the reference's recipe: ``labels[k] = (code == k + 1)`` and
``weights[k] = intersect_weight[k] * W + class_weight[k]``.

Computed defocus and saturation (the stand-in for the re-imaged pages of the published sets when a user has one in-focus plane
per sample): ``AugmentTable.from_sigmas`` makes the Gaussian levels, ``TrainSet.set_augment`` attaches them, ``Sampler.next_augmented``
draws a blur level and a saturation gain per image and ``Trainer.step_augmented`` applies them on the device.

Rotation and zoom: ``warp_matrix`` makes the 2 x 2 matrix of an angle and a magnification, ``Sampler.next_warped`` draws one per
image (``rotate_prob``, ``zoom_prob``, ``zoom_range``) and ``Trainer.step_warped`` resamples data, labels and weights on the device.

Elastic deformation: ``elastic_lattice`` lays clipped normal draws into the displacement lattice of ``trainer.ELASTIC_DESC``,
``Sampler.next_elastic`` draws one per image (``elastic_prob``, ``elastic_sigma``, ``elastic_grid``) and ``Trainer.step_elastic``
adds its cubic B-spline displacement to the source coordinate of that one resampling.

Border weight maps, for sets annotated without a ``_wt.tif`` (the reference reads that file and never makes it): ``BorderOptions`` names
the objects' class and a sigma, ``TrainSet.border_weights`` replaces the stored map of a sample by U-Net's border term
``exp(-(d1 + d2)^2 / (2 sigma^2))`` of its annotation's 4-connected objects (``umx_trainset_border_weights``; DESIGN.md section 9.2,
"Border weight maps" -- a reading of the published maps, not something the reference pins), ``TrainSet.border_planes`` returns the
labels, both squared distances and the map of one sample.

Object score of the validation pass: ``ObjectOptions`` names the objects' class and a least area, ``Trainer.evaluate(ts, descs,
objects=...)`` then also counts annotated and predicted 4-connected objects, the pairs with IoU > 1/2 and > 3/4, merges and splits, on
the device (``umx_trainer_evaluate_objects``; DESIGN.md section 9.2, "Object score" -- this project's own definition), and
``Trainer.object_counts`` runs the same pass on planes the host supplies.
"""
from __future__ import annotations

import ctypes
import os
import re
from dataclasses import dataclass
from typing import List, Optional, Tuple

import numpy as np

from . import imtools, tiffio
from .trainer import (AUGMENT_DESC, AUGMENT_MAX_LEVELS, AUGMENT_MAX_RADIUS, BORDER_MAX_SIGMA, ELASTIC_DESC, ELASTIC_MAX_DISP,
                      ELASTIC_MAX_GRID, OBJECT_MAX_MIN_AREA, SAMPLE_DESC, WARP_DESC, AugmentTableC, BorderOptionsC, LabelWeightsC,
                      ObjectOptionsC)


@dataclass(frozen=True)
class LabelWeights:
    """``umx_label_weights``: weighted=False is the unweighted loss (legacy graph only)."""
    weighted: bool
    class_weight: Tuple[float, ...] = ()
    intersect_weight: Tuple[float, ...] = ()

    def c_struct(self) -> LabelWeightsC:
        lw = LabelWeightsC()
        lw.weighted = int(bool(self.weighted))
        for k, v in enumerate(self.class_weight):
            lw.class_weight[k] = float(v)
        for k, v in enumerate(self.intersect_weight):
            lw.intersect_weight[k] = float(v)
        return lw


UNWEIGHTED = LabelWeights(False)

# The reference's constants per trainer (bgWeight, contourWeight, nucleiWeight, intersectWeight and the jitter maxima):
#   solo    UnMicst1-5.py:276-281 (weights), :464-477 (maxBrig = datasetStDev, maxCont = 0.1 datasetStDev)
#   duo     UnMicst2.py:273-278, :453-463
#   legacy  UnMicst.py:236-243, :343-350 -- labels only (an unweighted loss) and no jitter
LABEL_WEIGHTS = {
    "solo": LabelWeights(True, (1.0, 2.0, 7.0), (0.0, 15.0, 0.0)),
    "duo": LabelWeights(True, (1.0, 2.0, 5.0), (0.0, 10.0, 0.0)),
    "legacy": UNWEIGHTED,
}


def default_jitter(kind: str, std: float) -> Tuple[float, float]:
    """(max_brightness, max_contrast) of a trainer kind, in the normalised domain: the reference adds ``maxBrig = 1 * datasetStDev``
    and scales by ``1 +- 0.1 * datasetStDev`` after normalising (UnMicst1-5.py:464-477, UnMicst2.py:453-463); the legacy trainer
    has no jitter."""
    if kind == "legacy":
        return 0.0, 0.0
    return 1.0 * float(std), 0.1 * float(std)


def gaussian_taps(sigma: float) -> np.ndarray:
    """The one-sided taps ``w[0..R]`` (float32) of a Gaussian of ``sigma`` pixels, by scipy.ndimage's rule with truncate = 3:
    ``R = int(3 sigma + 0.5)``, ``exp(-0.5 (t / sigma)^2)`` normalised over ``-R..R`` in float64, then rounded (not renormalised)."""
    sigma = float(sigma)
    if not (np.isfinite(sigma) and sigma > 0.0):
        raise ValueError("a blur sigma must be finite and > 0, got %r" % sigma)
    R = int(3.0 * sigma + 0.5)
    if R > AUGMENT_MAX_RADIUS:
        raise ValueError("sigma %g gives radius %d; the kernel takes radii up to %d (sigma <= 4)" % (sigma, R, AUGMENT_MAX_RADIUS))
    t = np.arange(-R, R + 1, dtype=np.float64)
    w = np.exp(-0.5 * (t / sigma) ** 2)
    w /= w.sum()
    return w[R:].astype(np.float32)


def warp_matrix(angle_deg: float, zoom: float) -> np.ndarray:
    """``umx_warp_desc.m``: ``(1 / zoom) * [[cos t, -sin t], [sin t, cos t]]`` in float64, rounded to float32 -- the source step per
    output step, so ``zoom > 1`` magnifies.  An angle of 0 at zoom 1 is the exact identity ("no warp")."""
    angle_deg, zoom = float(angle_deg), float(zoom)
    if not (np.isfinite(angle_deg) and np.isfinite(zoom) and zoom > 0.0):
        raise ValueError("a warp needs a finite angle and a finite zoom > 0, got %r, %r" % (angle_deg, zoom))
    t = np.deg2rad(np.float64(angle_deg))
    c, s = np.cos(t) / zoom, np.sin(t) / zoom
    return (np.array([c, -s, s, c], np.float64) + 0.0).astype(np.float32)   # (+ 0.0: no -0.0)


def elastic_lattice(z, sigma: float, n: int) -> np.ndarray:
    """``umx_elastic_desc.d``: ``float32(sigma * clip(z, -2, 2))`` for ``2 n n`` standard normal draws ``z`` (row displacements first),
    laid into the ``n x n`` corner of the 2 x 6 x 6 block; the rest is zero.  ``n`` = lattice points per axis, 4..6."""
    sigma, n = float(sigma), int(n)
    if not 4 <= n <= ELASTIC_MAX_GRID:
        raise ValueError("a lattice has 4..%d points per axis, got %d" % (ELASTIC_MAX_GRID, n))
    if not (np.isfinite(sigma) and 0.0 <= sigma and 2.0 * sigma <= ELASTIC_MAX_DISP):
        raise ValueError("an elastic sigma is finite, >= 0 and at most %g, got %r" % (ELASTIC_MAX_DISP / 2.0, sigma))
    z = np.asarray(z, np.float64)
    if z.size != 2 * n * n or not np.isfinite(z).all():
        raise ValueError("a %d x %d lattice takes %d finite draws, got shape %r" % (n, n, 2 * n * n, z.shape))
    d = np.zeros((2, ELASTIC_MAX_GRID, ELASTIC_MAX_GRID), np.float32)
    d[:, :n, :n] = (sigma * np.clip(z.reshape(2, n, n), -2.0, 2.0) + 0.0).astype(np.float32)   # (+ 0.0: no -0.0)
    return d


@dataclass(frozen=True)
class AugmentTable:
    """``umx_augment_table``: ``taps[l]`` are the one-sided taps of blur level ``l`` (level 0: no blur), ``mean`` / ``std`` the set's
    normalisation (the saturation ceiling is ``(1 - mean) / std``)."""
    mean: float
    std: float
    taps: Tuple[np.ndarray, ...]

    @classmethod
    def from_sigmas(cls, sigmas, mean: float, std: float) -> "AugmentTable":
        """Level 0 = no blur, level ``i + 1`` = a Gaussian of ``sigmas[i]`` pixels."""
        sigmas = list(sigmas)
        if len(sigmas) + 1 > AUGMENT_MAX_LEVELS:
            raise ValueError("a table holds %d blur levels besides 'none', got %d sigmas" % (AUGMENT_MAX_LEVELS - 1, len(sigmas)))
        if not (np.isfinite(mean) and np.isfinite(std) and std > 0):
            raise ValueError("mean must be finite and std finite and > 0")
        return cls(float(mean), float(std), (np.ones(1, np.float32),) + tuple(gaussian_taps(s) for s in sigmas))

    @property
    def n_levels(self) -> int:
        return len(self.taps)

    @property
    def radius(self) -> Tuple[int, ...]:
        return tuple(len(w) - 1 for w in self.taps)

    def c_struct(self) -> AugmentTableC:
        t = AugmentTableC()
        t.mean, t.std, t.n_levels = self.mean, self.std, self.n_levels
        for l, w in enumerate(self.taps):
            t.radius[l] = len(w) - 1
            for k, v in enumerate(w):
                t.taps[l][k] = float(v)
        return t


@dataclass(frozen=True)
class BorderOptions:
    """``umx_border_options``: ``sigma`` in pixels, ``0 < sigma <= 8`` (the map is cut at ``radius = ceil(4 sigma)`` pixels);
    ``object_class`` the 0-based class of the objects, None = the last class (nuclei in the reference's sets)."""
    sigma: float = 5.0
    object_class: Optional[int] = None

    def __post_init__(self):
        sigma = float(np.float32(self.sigma))
        if not 0.0 < sigma <= BORDER_MAX_SIGMA:   # (a NaN fails the chain)
            raise ValueError("a border sigma is above 0 and at most %g, got %r" % (BORDER_MAX_SIGMA, self.sigma))
        if self.object_class is not None and (int(self.object_class) != self.object_class or self.object_class < 0):
            raise ValueError("object_class is a 0-based class index or None, got %r" % (self.object_class,))

    @property
    def radius(self) -> int:
        return int(np.ceil(4.0 * np.float64(np.float32(self.sigma))))

    def object_code(self, n_classes: int) -> int:
        """The annotation code of the objects: class + 1."""
        k = n_classes - 1 if self.object_class is None else int(self.object_class)
        if not 0 <= k < n_classes:
            raise ValueError("object_class %d: the model has classes 0..%d" % (k, n_classes - 1))
        return k + 1

    def c_struct(self, n_classes: int) -> BorderOptionsC:
        o = BorderOptionsC()
        o.object_code, o.sigma = self.object_code(n_classes), float(self.sigma)
        return o


@dataclass(frozen=True)
class ObjectOptions:
    """``umx_object_options``: ``object_class`` the 0-based class of the objects, None = the last class (nuclei in the reference's sets);
    ``min_area`` in pixels, 1..65536: predicted objects below it are dropped before anything is counted."""
    object_class: Optional[int] = None
    min_area: int = 1

    def __post_init__(self):
        if self.object_class is not None and (int(self.object_class) != self.object_class or self.object_class < 0):
            raise ValueError("object_class is a 0-based class index or None, got %r" % (self.object_class,))
        whole = isinstance(self.min_area, (int, np.integer)) or (isinstance(self.min_area, float) and self.min_area.is_integer())
        if not whole or not 1 <= self.min_area <= OBJECT_MAX_MIN_AREA:
            raise ValueError("min_area is 1..%d pixels, got %r" % (OBJECT_MAX_MIN_AREA, self.min_area))

    def object_code(self, n_classes: int) -> int:
        """The class code of the objects: class + 1."""
        k = n_classes - 1 if self.object_class is None else int(self.object_class)
        if not 0 <= k < n_classes:
            raise ValueError("object_class %d: the model has classes 0..%d" % (k, n_classes - 1))
        return k + 1

    def c_struct(self, n_classes: int) -> ObjectOptionsC:
        o = ObjectOptionsC()
        o.object_code, o.min_area = self.object_code(n_classes), int(self.min_area)
        return o


class TrainSet:
    """``n_samples`` samples of ``size x size`` pixels with ``nChannels x n_pages`` normalised planes each, one annotation plane and
    (weighted sets) one weight map, in the device memory of ``trainer``.  Close it (or the trainer) to free that memory."""

    def __init__(self, trainer, n_samples: int, n_pages: int, size: int, label_weights: LabelWeights):
        self.trainer = trainer
        self.n_samples, self.n_pages, self.size = int(n_samples), int(n_pages), int(size)
        self.label_weights = label_weights
        self.weighted = bool(label_weights.weighted)
        lib = trainer._lib
        lw = label_weights.c_struct()
        h = ctypes.c_void_p()
        trainer._check(lib.umx_trainset_create(trainer._h, self.n_samples, self.n_pages, self.size, ctypes.byref(lw), ctypes.byref(h)))
        self._h = h
        self._lib = lib
        self.border_computed = 0          # samples whose weight map ``upload`` computed on the device
        if not hasattr(trainer, "_sets"):
            import weakref
            trainer._sets = weakref.WeakSet()
        trainer._sets.add(self)

    def _handle(self):
        if not getattr(self, "_h", None):
            raise ValueError("the training set is closed")
        return self._h

    def set(self, i: int, planes, annotation, weight_map=None) -> None:
        """Upload sample ``i``: planes [nChannels][n_pages][size][size] (normalised, float32), annotation [size][size] class codes
        (uint8), weight_map [size][size] or None (= 0; ignored by an unweighted set)."""
        hp, S = self.trainer.hp, self.size
        p = np.ascontiguousarray(planes, dtype=np.float32)
        if p.shape != (hp.nChannels, self.n_pages, S, S):
            raise ValueError("planes must be %r, got %r" % ((hp.nChannels, self.n_pages, S, S), p.shape))
        a = np.asarray(annotation)
        if a.shape != (S, S):
            raise ValueError("annotation must be %r, got %r" % ((S, S), a.shape))
        if a.dtype != np.uint8:
            if a.size and (a.min() < 0 or a.max() > 255):
                raise ValueError("annotation codes must be 0..255")
            a = a.astype(np.uint8)
        a = np.ascontiguousarray(a)
        w = None
        if weight_map is not None:
            w = np.ascontiguousarray(weight_map, dtype=np.float32)
            if w.shape != (S, S):
                raise ValueError("weight_map must be %r, got %r" % ((S, S), w.shape))
        self.trainer._check(self._lib.umx_trainset_set(self._handle(), int(i), p.ctypes.data, a.ctypes.data,
                                                       None if w is None else w.ctypes.data))

    def set_augment(self, table: AugmentTable) -> None:
        """Attach (or replace) the blur levels and the normalisation that ``Trainer.step_augmented`` / ``assemble_augmented`` use."""
        c = table.c_struct()
        self.trainer._check(self._lib.umx_trainset_set_augment(self._handle(), ctypes.byref(c)))
        self.augment = table

    def border_weights(self, options: BorderOptions, index: Optional[int] = None) -> None:
        """Replace the stored weight map of sample ``index`` (None: of every sample) by the border map computed from its annotation
        (weighted sets only)."""
        o = options.c_struct(self.trainer.hp.nClasses)
        self.trainer._check(self._lib.umx_trainset_border_weights(self._handle(), -1 if index is None else int(index), ctypes.byref(o)))

    def border_planes(self, index: int, options: BorderOptions):
        """Diagnostics: ``(labels, d1sq, d2sq, wmap)`` of sample ``index``, int32 / int32 / int32 / float32 [size][size], recomputed by
        the kernels of ``border_weights``; the stored map stays."""
        S = self.size
        o = options.c_struct(self.trainer.hp.nClasses)
        labels, d1sq, d2sq = (np.empty((S, S), np.int32) for _ in range(3))
        wmap = np.empty((S, S), np.float32)
        self.trainer._check(self._lib.umx_trainset_border_planes(self._handle(), int(index), ctypes.byref(o), labels.ctypes.data,
                                                                 d1sq.ctypes.data, d2sq.ctypes.data, wmap.ctypes.data))
        return labels, d1sq, d2sq, wmap

    @classmethod
    def from_arrays(cls, trainer, planes, annotations, weight_maps=None, label_weights: LabelWeights = UNWEIGHTED) -> "TrainSet":
        """planes [N][C][pages][S][S], annotations [N][S][S], weight_maps: None or a sequence of [S][S] arrays / None."""
        planes = np.asarray(planes)
        if planes.ndim != 5:
            raise ValueError("planes must be [N][C][pages][S][S], got shape %r" % (planes.shape,))
        n, _, pages, S, _ = planes.shape
        ts = cls(trainer, n, pages, S, label_weights)
        try:
            for i in range(n):
                ts.set(i, planes[i], annotations[i], None if weight_maps is None else weight_maps[i])
        except BaseException:
            ts.close()
            raise
        return ts

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.umx_trainset_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


@dataclass
class Dataset:
    """What ``read_dataset_dir`` returns: planes [N][C][pages][S][S] float32, annotations [N][S][S] uint8, weight maps (float32 or
    None per sample)."""
    planes: np.ndarray
    annotations: np.ndarray
    weight_maps: List[Optional[np.ndarray]]

    @property
    def n_samples(self) -> int:
        return int(self.planes.shape[0])

    @property
    def size(self) -> int:
        return int(self.planes.shape[-1])


_IMG = re.compile(r"^I(\d{5})_Img\.tif$")


def dataset_indices(path: str) -> List[int]:
    """The sample numbers of a dataset directory (``I%05d_Img.tif`` files), sorted."""
    if not os.path.isdir(path):
        raise FileNotFoundError("%s is not a directory" % path)
    return sorted(int(m.group(1)) for m in (_IMG.match(f) for f in os.listdir(path)) if m)


def read_dataset_dir(path: str, n_pages: int, n_channels: int, mean: float, std: float) -> Dataset:
    """Read every sample of the published layout and normalise it as the reference does, in float64, rounded once to float32:
    ``(im2double(page) - mean) / std`` for page ``aug + n_pages * channel`` (UnMicst1-5.py:297-301).  Annotations keep their
    codes; a missing ``_wt.tif`` gives None."""
    idx = dataset_indices(path)
    if not idx:
        raise FileNotFoundError("%s holds no I%%05d_Img.tif samples" % path)
    planes, anns, wmaps = [], [], []
    size = None
    for i in idx:
        img = os.path.join(path, "I%05d_Img.tif" % i)
        have = tiffio.num_pages(img)
        if have != n_pages * n_channels:
            raise ValueError("%s has %d pages, expected %d (%d pages x %d channels)" % (img, have, n_pages * n_channels, n_pages,
                                                                                         n_channels))
        p = np.empty((n_channels, n_pages), dtype=object)
        for c in range(n_channels):
            for a in range(n_pages):
                im = imtools.im2double(tiffio.imread(img, key=a + n_pages * c))
                p[c, a] = ((np.asarray(im, np.float64) - float(mean)) / float(std)).astype(np.float32)
        shape = p[0, 0].shape
        if len(shape) != 2 or shape[0] != shape[1]:
            raise ValueError("%s: samples must be square, got %r" % (img, shape))
        if size is None:
            size = shape[0]
        if shape[0] != size or any(q.shape != shape for q in p.flat):
            raise ValueError("%s: every sample and page must be %d x %d" % (img, size, size))
        planes.append(np.stack([np.stack(list(p[c])) for c in range(n_channels)]))
        ant = tiffio.imread(os.path.join(path, "I%05d_Ant.tif" % i))
        if ant.shape != shape:
            raise ValueError("I%05d_Ant.tif is %r, the image %r" % (i, ant.shape, shape))
        if ant.dtype != np.uint8:
            if ant.min() < 0 or ant.max() > 255:
                raise ValueError("I%05d_Ant.tif: class codes must be 0..255" % i)
            ant = ant.astype(np.uint8)
        anns.append(ant)
        wt = os.path.join(path, "I%05d_wt.tif" % i)
        if os.path.exists(wt):
            w = tiffio.imread(wt)
            if w.shape != shape:
                raise ValueError("I%05d_wt.tif is %r, the image %r" % (i, w.shape, shape))
            wmaps.append(np.asarray(w, np.float32))
        else:
            wmaps.append(None)
    return Dataset(np.stack(planes), np.stack(anns), wmaps)


class Sampler:
    """Descriptor stream of a training run: every sample once per epoch in an order reshuffled each epoch, then per image a
    uniform augmentation page, a uniform crop origin, optionally one of the 8 dihedral transforms, and the reference's jitter
    (``brightness = max_brightness * (+-1) * U[0,1)``, ``contrast = 1 + max_contrast * (+-1) * U[0,1)``, UnMicst1-5.py:473-474).
    All draws come from ``numpy.random.Generator(PCG64(seed))`` in a fixed order, so a seed fixes the stream.

    Blur and saturation (off by default; then nothing extra is drawn): with ``blur_prob`` an image gets a blur level uniform over
    ``1..blur_levels - 1`` (``blur_levels`` = the levels of the set's table, level 0 included), with ``saturate_prob`` a gain
    ``1 + (max_gain - 1) U[0,1)``.  When either probability is positive, four draws follow every image's contrast draw -- blur coin,
    level, saturation coin, gain -- whatever the coins say, so one image's outcome never shifts the next one's draws.

    Rotation and zoom (off by default; then nothing extra is drawn): with ``rotate_prob`` an image is rotated by ``360 U[0,1)`` degrees,
    with ``zoom_prob`` magnified by ``lo (hi / lo)^U[0,1)``, ``(lo, hi) = zoom_range`` (log-uniform).  When either probability is
    positive, four more draws follow the image's previous ones (after the gain draw when blur / saturation are on, else after the
    contrast draw) -- rotation coin, angle, zoom coin, zoom -- again whatever the coins say.

    Elastic deformation (off by default; then nothing extra is drawn): with ``elastic_prob`` an image gets a lattice of
    ``n = elastic_grid + 3`` points per axis (``elastic_grid`` = 1..3 spline cells across the crop) whose displacements are
    ``elastic_sigma`` pixels times standard normal draws clipped at +-2 (``elastic_lattice``).  When ``elastic_prob`` is positive, two
    draws follow the image's previous ones -- the coin, then ``standard_normal(2 n n)`` -- whatever the coin says."""

    def __init__(self, seed: int, n_samples: int, batch: int, size: int, P: int, n_pages: int, max_brightness: float = 0.0,
                 max_contrast: float = 0.0, transforms: bool = False, blur_levels: int = 1, blur_prob: float = 0.0,
                 saturate_prob: float = 0.0, max_gain: float = 1.0, rotate_prob: float = 0.0, zoom_prob: float = 0.0,
                 zoom_range: Tuple[float, float] = (1.0, 1.0), elastic_prob: float = 0.0, elastic_sigma: float = 0.0,
                 elastic_grid: int = 2):
        if n_samples < 1 or batch < 1 or n_pages < 1 or size < P:
            raise ValueError("a sampler needs samples, a batch, pages and size >= P")
        if not (0.0 <= blur_prob <= 1.0 and 0.0 <= saturate_prob <= 1.0):
            raise ValueError("blur_prob and saturate_prob are probabilities")
        if not 1 <= blur_levels <= AUGMENT_MAX_LEVELS or (blur_prob > 0 and blur_levels < 2):
            raise ValueError("blur_levels counts the table's levels (1..%d); blurring needs one besides level 0" % AUGMENT_MAX_LEVELS)
        if not (np.isfinite(max_gain) and max_gain >= 1.0):
            raise ValueError("max_gain must be finite and >= 1")
        if not (0.0 <= rotate_prob <= 1.0 and 0.0 <= zoom_prob <= 1.0):
            raise ValueError("rotate_prob and zoom_prob are probabilities")
        lo, hi = (float(v) for v in zoom_range)
        if not 0.5 <= lo <= 1.0 <= hi <= 2.0:   # (no anti-aliased minification: the floor of 0.5)
            raise ValueError("zoom_range must satisfy 0.5 <= lo <= 1 <= hi <= 2, got %r" % ((lo, hi),))
        if not 0.0 <= elastic_prob <= 1.0:
            raise ValueError("elastic_prob is a probability")
        if int(elastic_grid) != elastic_grid or not 1 <= elastic_grid <= ELASTIC_MAX_GRID - 3:
            raise ValueError("elastic_grid counts the spline cells across the crop, 1..%d, got %r" % (ELASTIC_MAX_GRID - 3, elastic_grid))
        if not (np.isfinite(elastic_sigma) and 0.0 <= elastic_sigma and 2.0 * elastic_sigma <= ELASTIC_MAX_DISP):
            raise ValueError("elastic_sigma must be finite, >= 0 and at most %g" % (ELASTIC_MAX_DISP / 2.0))
        if elastic_prob > 0 and not elastic_sigma > 0:
            raise ValueError("an elastic deformation needs elastic_sigma > 0")
        self.elastic_prob, self.elastic_sigma, self.elastic_grid = float(elastic_prob), float(elastic_sigma), int(elastic_grid)
        self.rotate_prob, self.zoom_prob, self.zoom_range = float(rotate_prob), float(zoom_prob), (lo, hi)
        self.blur_levels, self.blur_prob = int(blur_levels), float(blur_prob)
        self.saturate_prob, self.max_gain = float(saturate_prob), float(max_gain)
        self.rng = np.random.Generator(np.random.PCG64(seed))
        self.n_samples, self.batch, self.size, self.P, self.n_pages = int(n_samples), int(batch), int(size), int(P), int(n_pages)
        self.max_brightness, self.max_contrast = float(max_brightness), float(max_contrast)
        self.transforms = bool(transforms)
        self.epoch = 0
        self._perm = self.rng.permutation(self.n_samples)
        self._pos = 0

    def _next_index(self) -> int:
        if self._pos == self.n_samples:
            self.epoch += 1
            self._perm = self.rng.permutation(self.n_samples)
            self._pos = 0
        i = int(self._perm[self._pos])
        self._pos += 1
        return i

    @property
    def augmenting(self) -> bool:
        return self.blur_prob > 0.0 or self.saturate_prob > 0.0

    @property
    def warping(self) -> bool:
        return self.rotate_prob > 0.0 or self.zoom_prob > 0.0

    def next(self) -> np.ndarray:
        """The next batch: ``batch`` descriptors (a SAMPLE_DESC array)."""
        return self.next_warped()[0]

    def next_augmented(self) -> Tuple[np.ndarray, np.ndarray]:
        """The next batch: ``batch`` descriptors and their blur level / gain (a SAMPLE_DESC and an AUGMENT_DESC array)."""
        return self.next_warped()[:2]

    @property
    def deforming(self) -> bool:
        return self.elastic_prob > 0.0

    def next_warped(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """The next batch: ``batch`` descriptors, their blur level / gain and their rotation / zoom matrix (a SAMPLE_DESC, an
        AUGMENT_DESC and a WARP_DESC array)."""
        return self.next_elastic()[:3]

    def next_elastic(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """The next batch: ``batch`` descriptors, their blur level / gain, their rotation / zoom matrix and their displacement lattice (a
        SAMPLE_DESC, an AUGMENT_DESC, a WARP_DESC and an ELASTIC_DESC array)."""
        d = np.zeros(self.batch, SAMPLE_DESC)
        a = np.zeros(self.batch, AUGMENT_DESC)
        a["gain"] = 1.0
        w = np.zeros(self.batch, WARP_DESC)
        w["m"] = (1.0, 0.0, 0.0, 1.0)
        e = np.zeros(self.batch, ELASTIC_DESC)
        n_lat = self.elastic_grid + 3
        lo, hi = self.zoom_range
        r = self.rng
        span = self.size - self.P + 1
        for j in range(self.batch):
            d["index"][j] = self._next_index()
            d["page"][j] = r.integers(self.n_pages)
            d["y0"][j] = r.integers(span)
            d["x0"][j] = r.integers(span)
            d["transform"][j] = r.integers(8) if self.transforms else 0
            sb = -1.0 if r.random() < 0.5 else 1.0
            d["brightness"][j] = self.max_brightness * sb * r.random() + 0.0   # (+ 0.0: no -0.0 when there is no jitter)
            sc = -1.0 if r.random() < 0.5 else 1.0
            d["contrast"][j] = 1.0 + self.max_contrast * sc * r.random()
            if self.augmenting:
                blur = r.random() < self.blur_prob
                level = 1 + int(r.integers(max(self.blur_levels - 1, 1)))
                sat = r.random() < self.saturate_prob
                gain = 1.0 + (self.max_gain - 1.0) * r.random()
                a["blur_level"][j] = level if blur else 0
                a["gain"][j] = gain if sat else 1.0
            if self.warping:
                rot = r.random() < self.rotate_prob
                angle = 360.0 * r.random()
                zoomed = r.random() < self.zoom_prob
                zoom = lo * (hi / lo) ** r.random()
                w["m"][j] = warp_matrix(angle if rot else 0.0, zoom if zoomed else 1.0)
            if self.deforming:
                deformed = r.random() < self.elastic_prob
                z = r.standard_normal(2 * n_lat * n_lat)
                if deformed:
                    e["n"][j] = n_lat
                    e["d"][j] = elastic_lattice(z, self.elastic_sigma, n_lat)
        return d, a, w, e

    def __iter__(self):
        while True:
            yield self.next()

    def validation_descriptors(self) -> np.ndarray:
        return validation_descriptors(self.n_samples, self.size, self.P)


def crop_origins(size: int, P: int) -> List[int]:
    """Origins of the P-crops that cover 0..size-1: every P pixels, the last one flush with the far edge."""
    o = list(range(0, size - P + 1, P))
    if o[-1] != size - P:
        o.append(size - P)
    return o


def validation_descriptors(n_samples: int, size: int, P: int) -> np.ndarray:
    """Every sample once, covered by P-crops (page 0, no transform, no jitter)."""
    org = crop_origins(size, P)
    d = np.zeros(n_samples * len(org) ** 2, SAMPLE_DESC)
    k = 0
    for i in range(n_samples):
        for y in org:
            for x in org:
                d[k] = (i, 0, y, x, 0, 0.0, 1.0, 0)
                k += 1
    return d


def upload(trainer, ds: Dataset, label_weights: LabelWeights, border: Optional[BorderOptions] = None) -> TrainSet:
    """A ``Dataset`` into the device memory of ``trainer``.  ``border``: the weight map of exactly those samples that bring none
    (``weight_maps[i] is None``) is computed on the device; ``TrainSet.border_computed`` counts them."""
    if border is not None:
        if not label_weights.weighted:
            raise ValueError("a border weight map needs a weighted set: the legacy loss takes no weights")
        border.object_code(trainer.hp.nClasses)
    ts = TrainSet.from_arrays(trainer, ds.planes, ds.annotations, ds.weight_maps, label_weights)
    if border is not None:
        try:
            maps = [None] * ts.n_samples if ds.weight_maps is None else ds.weight_maps
            missing = [i for i, w in enumerate(maps) if w is None]
            if len(missing) == ts.n_samples:
                ts.border_weights(border)
            else:
                for i in missing:
                    ts.border_weights(border, i)
            ts.border_computed = len(missing)
        except BaseException:
            ts.close()
            raise
    return ts


def graph_kind(hp) -> str:
    """Which of the reference's trainers a model's graph belongs to: legacy (UnMicst.py), solo (1 channel, UnMicst1-5.py) or
    duo (2 channels, UnMicst2.py)."""
    from .model import GRAPH_LEGACY
    if hp.graph == GRAPH_LEGACY:
        return "legacy"
    return "solo" if hp.nChannels == 1 else "duo"


__all__ = ["LabelWeights", "UNWEIGHTED", "LABEL_WEIGHTS", "default_jitter", "BorderOptions", "ObjectOptions", "TrainSet", "Dataset", "dataset_indices",
           "read_dataset_dir", "Sampler", "gaussian_taps", "AugmentTable", "AUGMENT_DESC", "warp_matrix", "WARP_DESC", "elastic_lattice", "ELASTIC_DESC", "crop_origins", "validation_descriptors", "upload", "graph_kind", "SAMPLE_DESC"]
