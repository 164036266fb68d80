"""Fine-tune a model on an annotated training set, or train one from the initial state:

    python -m unmicst_amd.finetune --model NAME|DIR --train DIR --valid DIR --out DIR [--steps N] [--batch B] [--pages A]
                                   [--eval-every E] [--seed S] [--lr0 LR] [--transforms] [--device D]
                                   [--blur-sigmas 0.75,1.5,3] [--blur-prob P] [--saturate-prob P] [--max-gain G]
                                   [--rotate-prob P] [--zoom-prob P] [--zoom-range LO,HI]
                                   [--elastic-sigma PX] [--elastic-prob P] [--elastic-grid G]
                                   [--border-sigma PX [--border-class K]]
                                   [--object-score [--object-class K] [--object-min-area A] [--select pixel|object]]
                                   [--from-scratch [--init-seed S] [--std-dev0 V] [--mean M --std S]]

``--train`` / ``--valid`` hold the reference's published layout (``I%05d_Img.tif`` / ``_Ant.tif`` / ``_wt.tif``, see
unmicst_amd/trainset.py).  Both sets are uploaded to the device once; each step draws its batch with ``Sampler`` and trains with
``Trainer.step_sampled`` under the reference trainer's regime for the model's graph (legacy / solo / duo options, label weights
and jitter).  Every ``--eval-every`` steps the whole validation set is evaluated on the device; the checkpoint with the lowest mean
per-class pixel error (or, with ``--select object``, the highest object F1) is written to ``<out>/umx_model.npz`` with the base model's normalisation mean / std, so
``UnMicst.py --model <out>`` runs on it, and every evaluation is one line of ``<out>/finetune_log.jsonl``.

Computed defocus and saturation, for sets with one in-focus plane per sample (the published sets carry re-imaged defocused and
saturated planes as extra pages instead): ``--blur-sigmas`` lists the Gaussian blur levels in pixels and ``--blur-prob`` is the chance
that an image gets one of them; ``--saturate-prob`` is the chance that an image is amplified by a gain drawn from
``[1, --max-gain)`` on the im2double scale and clipped at 1.  Both are applied on the device while the batch is built
(``Trainer.step_augmented``); validation stays unaugmented.  When any of the four flags is given, the settings are the first line of
the log.

Rotation and zoom, the geometry a small set of ``imSize``-wide samples cannot get from crops and the 8 dihedral transforms:
``--rotate-prob`` is the chance that an image is rotated about its crop's centre by an angle uniform over the full turn,
``--zoom-prob`` (0.5 when ``--zoom-range`` is given) the chance that it is magnified by a factor drawn log-uniformly from
``--zoom-range LO,HI`` (``0.5 <= LO <= 1 <= HI <= 2``).  Data is resampled bilinearly and mirrored at the sample's edges; labels and
weight maps take the nearest source pixel (``Trainer.step_warped``).  Validation stays unwarped.  When one of the three flags is given,
the log's first line carries the settings as its ``"warp"`` object (next to ``"augment"`` when both are on).

Elastic deformation, the one augmentation here that changes a nucleus's shape: ``--elastic-sigma PX`` is the standard deviation of the
displacement vectors on a lattice of ``--elastic-grid G`` (1..3, default 2) spline cells across the tile, drawn on the host and clipped
at two sigmas; ``--elastic-prob`` (0.5 when a sigma is given) is the chance that an image gets one.  A uniform cubic B-spline spreads
the lattice over the crop on the device, and the displacement is added to the source coordinate of the rotation / zoom resampling, so
data is still interpolated once and labels and weight maps still take the nearest source pixel (``Trainer.step_elastic``).  A sigma of
``(imSize - 1) / (8 G)`` or more is refused: below it the deformation cannot fold the image over itself.  Validation stays undeformed.
When one of the three flags is given, the log's first line carries the settings as its ``"elastic"`` object (after ``"init"``,
``"augment"`` and ``"warp"``).

Border weight maps, for sets annotated without ``_wt.tif`` files (without them, and without this flag, the contour-intersection term of
the weighted loss is 0 for those samples): ``--border-sigma PX`` (``0 < PX <= 8``; U-Net's own choice is 5) computes the map of every
sample of either set that brings none, on the device, as ``exp(-(d1 + d2)^2 / (2 PX^2))`` with ``d1`` / ``d2`` the distances to the nearest
and the second nearest 4-connected object of class ``--border-class K`` (0-based; default: the last class, nuclei), cut at
``ceil(4 PX)`` pixels.  That is U-Net's border term (Ronneberger et al. 2015) and this project's reading of the published maps: the
reference never makes them ("Border weight maps").  A sample with a ``_wt.tif`` keeps it.  The legacy graph's
loss takes no weights, so the flag is refused there.  With the flag the log's first line carries the ``"border"`` object (after
``"elastic"``): sigma, class, radius and ``"computed": [n_train, n_valid]``, the samples whose map was computed.

Object score, for users who count objects: the pixel error cannot see whether touching nuclei come apart (two of them merged through a
three-pixel bridge cost three pixels).  ``--object-score`` adds an object pass to every evaluation, on the device and on the same forward
pass (``umx_trainer_evaluate_objects``; DESIGN.md section 9.2, "Object score" -- this project's own definition, the reference has only the
pixel error): per validation crop, the 4-connected objects of class ``--object-class K`` (0-based; default: the last class, nuclei) in the
annotation and in the arg-max prediction -- predicted ones below ``--object-min-area A`` pixels (default 1) dropped -- are paired by
overlap; every evaluation line of the log gains ``"objects"``: ``truth``, ``predicted``, ``matched`` (IoU > 1/2), ``matched75`` (IoU > 3/4),
``merged``, ``split`` and ``f1 = 2 matched / (truth + predicted)`` (``null`` when there is no object on either side).  ``--select object``
keeps the checkpoint with the highest F1 instead of the lowest mean per-class pixel error (an F1 that is not a number never replaces a
kept checkpoint; ties keep the earlier step); ``--select pixel`` is the default.  With ``--object-score`` the log's first line carries the
``"objects"`` settings object (after ``"border"``): class, min_area and select.  Without it the log and the saved model are byte for
byte what they were.

``--from-scratch`` starts from the graph's initial state instead of the model's weights (the reference's
``train(..., restoreVariables=False)``: ``tf.global_variables_initializer()``, made on the device by ``Trainer.from_scratch``; DESIGN.md
section 9.3).  ``--model`` then supplies hyper-parameters only: a directory without weights (the shipped ``nucleiDAPI1-5`` /
``nucleiDAPILAMIN`` stand-ins) is accepted, and the weights of one that has them are not read.  ``--init-seed`` (default: ``--seed``)
seeds the initial state, ``--std-dev0`` overrides the reference's ``stdDev0`` (default: the directory's ``hp.data``, else 0.007), and
``--mean`` / ``--std`` (both or neither) set the new model's normalisation instead of the model directory's scalars.  The log's first
line then starts with the ``"init"`` object: seed, std_dev0, mean and std of the run (and ``"weights_not_read": true`` when the
model directory has weights).

The run is a function of its arguments: the same seed gives the same descriptor stream, the same steps and the same files.
There is no CPU fallback.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys

import numpy as np

from . import model, trainer, trainset, umx

LOG_NAME = "finetune_log.jsonl"


class Refusal(Exception):
    """An input the command does not take (reported before any device work)."""


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="python -m unmicst_amd.finetune", description=__doc__.split("\n\n")[0])
    p.add_argument("--model", required=True, help="model name under models/ (UMX_MODELS_DIR) or a model directory")
    p.add_argument("--train", required=True, help="training set directory (I%%05d_Img.tif / _Ant.tif / _wt.tif)")
    p.add_argument("--valid", required=True, help="validation set directory, same layout")
    p.add_argument("--out", required=True, help="output model directory (umx_model.npz + finetune_log.jsonl)")
    p.add_argument("--steps", type=int, default=1000)
    p.add_argument("--batch", type=int, default=0, help="images per step (0: the model's batchSize)")
    p.add_argument("--pages", type=int, default=1, help="augmentation pages per channel in the _Img.tif files")
    p.add_argument("--eval-every", type=int, default=100)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--lr0", type=float, default=None, help="initial learning rate (default: the graph's trainer)")
    p.add_argument("--transforms", action="store_true", help="draw one of the 8 dihedral transforms per image")
    p.add_argument("--device", type=int, default=0)
    p.add_argument("--blur-sigmas", default=None, help="blur levels: comma-separated Gaussian sigmas in pixels, each in (0, 4]")
    p.add_argument("--blur-prob", type=float, default=None, help="chance that an image is blurred (default 0.5 with --blur-sigmas)")
    p.add_argument("--saturate-prob", type=float, default=None, help="chance that an image is amplified and clipped (default 0)")
    p.add_argument("--max-gain", type=float, default=None, help="gains are drawn from [1, G) (default 2 with --saturate-prob)")
    p.add_argument("--rotate-prob", type=float, default=None, help="chance that an image is rotated by a uniform angle (default 0)")
    p.add_argument("--zoom-prob", type=float, default=None, help="chance that an image is magnified (default 0.5 with --zoom-range)")
    p.add_argument("--zoom-range", default=None, help="LO,HI: magnifications are drawn log-uniformly, 0.5 <= LO <= 1 <= HI <= 2")
    p.add_argument("--elastic-sigma", type=float, default=None, help="standard deviation of a lattice displacement in pixels, > 0")
    p.add_argument("--elastic-prob", type=float, default=None, help="chance that an image is deformed (default 0.5 with --elastic-sigma)")
    p.add_argument("--elastic-grid", type=int, default=None, help="spline cells across the tile, 1..3 (default 2)")
    p.add_argument("--border-sigma", type=float, default=None,
                   help="compute the weight map of samples without _wt.tif: sigma of the border term in pixels, in (0, 8]")
    p.add_argument("--border-class", type=int, default=None, help="0-based class of the objects (default: the last class); needs --border-sigma")
    p.add_argument("--object-score", action="store_true", help="add the object-level score to every evaluation")
    p.add_argument("--object-class", type=int, default=None, help="0-based class of the objects (default: the last class); needs --object-score")
    p.add_argument("--object-min-area", type=int, default=None,
                   help="predicted objects below this many pixels are dropped, 1..%d (default 1); needs --object-score" % trainer.OBJECT_MAX_MIN_AREA)
    p.add_argument("--select", choices=("pixel", "object"), default=None,
                   help="keep the checkpoint with the lowest mean per-class pixel error (default) or the highest object F1 (needs --object-score)")
    p.add_argument("--from-scratch", action="store_true", help="start from the graph's initial state, not from the model's weights")
    p.add_argument("--init-seed", type=int, default=None, help="seed of the initial state (default: --seed); needs --from-scratch")
    p.add_argument("--std-dev0", type=float, default=None,
                   help="the reference's stdDev0 (default: the model directory's hp.data, else %g); needs --from-scratch" % trainer.DEFAULT_STD_DEV0)
    p.add_argument("--mean", type=float, default=None, help="normalisation mean of the new model (with --std); needs --from-scratch")
    p.add_argument("--std", type=float, default=None, help="normalisation std of the new model (with --mean); needs --from-scratch")
    return p


def init_settings(args, model_path=None):
    """The from-scratch flags -> None without --from-scratch, else {"seed", "std_dev0", "mean", "std"}.  ``model_path`` supplies what
    the flags leave open (hp.data's stdDev0, the directory's mean / std); without it those stay None and only the flags are checked.
    Raises Refusal."""
    flags = (("--init-seed", "init_seed"), ("--std-dev0", "std_dev0"), ("--mean", "mean"), ("--std", "std"))
    if not getattr(args, "from_scratch", False):
        for flag, key in flags:
            if getattr(args, key, None) is not None:
                raise Refusal("%s needs --from-scratch" % flag)
        return None
    if args.std_dev0 is not None and not (math.isfinite(args.std_dev0) and args.std_dev0 > 0):
        raise Refusal("--std-dev0 %r: a standard deviation is finite and > 0" % args.std_dev0)
    if (args.mean is None) != (args.std is None):
        raise Refusal("--mean and --std go together: got only %s" % ("--mean" if args.std is None else "--std"))
    if args.std is not None and not (math.isfinite(args.std) and args.std > 0):
        raise Refusal("--std %r: a standard deviation is finite and > 0" % args.std)
    if args.mean is not None and not math.isfinite(args.mean):
        raise Refusal("--mean %r is not finite" % args.mean)
    out = {"seed": int(args.seed if args.init_seed is None else args.init_seed), "std_dev0": args.std_dev0, "mean": args.mean,
           "std": args.std}
    if model_path is not None:
        _, mean, std, sd0 = model.load_hparams_dir(model_path)
        if out["std_dev0"] is None:
            out["std_dev0"] = trainer.DEFAULT_STD_DEV0 if sd0 is None else sd0
        if out["mean"] is None:
            out["mean"], out["std"] = mean, std
    return {k: (v if v is None or k == "seed" else float(v)) for k, v in out.items()}


def has_weights(model_path: str) -> bool:
    """Whether load_model_dir would find weights in this directory (the converted blob or the reference's checkpoint shard)."""
    return any(os.path.exists(os.path.join(model_path, n)) for n in (model.CONVERTED_NAME, "model.ckpt.data-00000-of-00001"))


def warp_settings(args):
    """The three warp flags -> None when none is given, else {"rotate_prob", "zoom_prob", "zoom_range"}.  Raises Refusal."""
    given = [getattr(args, k, None) for k in ("rotate_prob", "zoom_prob", "zoom_range")]
    if all(v is None for v in given):
        return None
    zr = None
    if args.zoom_range is not None:
        try:
            zr = [float(v) for v in args.zoom_range.split(",")]
        except ValueError:
            zr = []
        if len(zr) != 2:
            raise Refusal("--zoom-range %r: expected LO,HI" % args.zoom_range)
        if not 0.5 <= zr[0] <= 1.0 <= zr[1] <= 2.0:   # (a NaN fails the chain)
            raise Refusal("--zoom-range %r: 0.5 <= LO <= 1 <= HI <= 2" % args.zoom_range)
    rot_prob = 0.0 if args.rotate_prob is None else args.rotate_prob
    zoom_prob = (0.5 if zr else 0.0) if args.zoom_prob is None else args.zoom_prob
    for name, v in (("--rotate-prob", rot_prob), ("--zoom-prob", zoom_prob)):
        if not 0.0 <= v <= 1.0:
            raise Refusal("%s %r is not a probability" % (name, v))
    if zoom_prob > 0 and zr is None:
        raise Refusal("--zoom-prob needs --zoom-range")
    return {"rotate_prob": float(rot_prob), "zoom_prob": float(zoom_prob), "zoom_range": zr or [1.0, 1.0]}


def elastic_settings(args, im_size=None):
    """The three elastic flags -> None when none is given, else {"prob", "sigma", "grid"}.  ``im_size`` (the model's tile) adds the
    bounds that depend on it; without it only the flags are checked.  Raises Refusal."""
    given = [getattr(args, k, None) for k in ("elastic_sigma", "elastic_prob", "elastic_grid")]
    if all(v is None for v in given):
        return None
    sigma = args.elastic_sigma
    if sigma is not None and not (math.isfinite(sigma) and sigma > 0):
        raise Refusal("--elastic-sigma %r: a standard deviation is finite and > 0" % sigma)
    prob = (0.5 if sigma is not None else 0.0) if args.elastic_prob is None else args.elastic_prob
    if not 0.0 <= prob <= 1.0:   # (a NaN fails both comparisons)
        raise Refusal("--elastic-prob %r is not a probability" % prob)
    if prob > 0 and sigma is None:
        raise Refusal("--elastic-prob needs --elastic-sigma")
    grid = 2 if args.elastic_grid is None else args.elastic_grid
    if not 1 <= grid <= trainer.ELASTIC_MAX_GRID - 3:
        raise Refusal("--elastic-grid %r: 1..%d spline cells across the tile" % (grid, trainer.ELASTIC_MAX_GRID - 3))
    sigma = 0.0 if sigma is None else float(sigma)
    if im_size is not None and sigma > 0:
        # lattice values are clipped at 2 sigma, so a partial derivative of the displacement is at most g = 4 sigma / h with
        # h = (P - 1) / G; the map is invertible for certain while 1 - 2 g > 0
        bound = (im_size - 1) / (8.0 * grid)
        if sigma >= bound:
            raise Refusal("--elastic-sigma %g: with %d cell(s) across a %d-pixel tile a sigma of %g or more may fold the image over itself"
                          % (sigma, grid, im_size, bound))
        if 2.0 * sigma > trainer.ELASTIC_MAX_DISP:
            raise Refusal("--elastic-sigma %g: displacements are clipped at 2 sigma, which must stay within %g pixels"
                          % (sigma, trainer.ELASTIC_MAX_DISP))
    return {"prob": float(prob), "sigma": sigma, "grid": int(grid)}


def border_settings(args, hp=None):
    """The two border flags -> None when neither is given, else {"sigma", "class", "radius"}.  ``hp`` (the model's hyper-parameters)
    adds the checks that depend on the graph and resolves the default class; without it only the flags are checked and a class left
    open stays None.  Raises Refusal."""
    sigma, cls = getattr(args, "border_sigma", None), getattr(args, "border_class", None)
    if sigma is None and cls is None:
        return None
    if sigma is None:
        raise Refusal("--border-class needs --border-sigma")
    if not 0.0 < sigma <= trainer.BORDER_MAX_SIGMA:   # (a NaN fails the chain)
        raise Refusal("--border-sigma %r: a sigma is above 0 and at most %g pixels" % (sigma, trainer.BORDER_MAX_SIGMA))
    if cls is not None and cls < 0:
        raise Refusal("--border-class %r: classes are 0-based" % cls)
    if hp is not None:
        if cls is not None and cls >= hp.nClasses:
            raise Refusal("--border-class %d: the model has classes 0..%d" % (cls, hp.nClasses - 1))
        if not trainset.LABEL_WEIGHTS[trainset.graph_kind(hp)].weighted:
            raise Refusal("--border-sigma: the legacy loss takes no weights, so a weight map would never be read")
        if cls is None:
            cls = hp.nClasses - 1
    opts = trainset.BorderOptions(float(sigma), cls)
    return {"sigma": float(sigma), "class": None if cls is None else int(cls), "radius": opts.radius}


def object_settings(args, hp=None):
    """The four object-score flags -> None without --object-score, else {"class", "min_area", "select"}.  ``hp`` (the model's
    hyper-parameters) adds the check that depends on the model and resolves the default class; without it only the flags are checked and
    a class left open stays None.  Raises Refusal."""
    cls, area, select = (getattr(args, k, None) for k in ("object_class", "object_min_area", "select"))
    if not getattr(args, "object_score", False):
        for flag, v in (("--object-class", cls), ("--object-min-area", area)):
            if v is not None:
                raise Refusal("%s needs --object-score" % flag)
        if select == "object":
            raise Refusal("--select object needs --object-score")
        return None
    if cls is not None and cls < 0:
        raise Refusal("--object-class %r: classes are 0-based" % cls)
    area = 1 if area is None else area
    if not 1 <= area <= trainer.OBJECT_MAX_MIN_AREA:
        raise Refusal("--object-min-area %r: an area is 1..%d pixels" % (area, trainer.OBJECT_MAX_MIN_AREA))
    if hp is not None:
        if cls is not None and cls >= hp.nClasses:
            raise Refusal("--object-class %d: the model has classes 0..%d" % (cls, hp.nClasses - 1))
        if cls is None:
            cls = hp.nClasses - 1
    return {"class": None if cls is None else int(cls), "min_area": int(area), "select": select or "pixel"}


def better_f1(f1: float, kept) -> bool:
    """Whether an evaluation with this F1 replaces the kept one (``kept`` = its F1, or None when nothing is kept yet: the first
    evaluation is always kept, so that the run leaves a model).  An F1 that is not a number never replaces a kept checkpoint; an equal
    one keeps the earlier step."""
    if kept is None:
        return True
    if math.isnan(f1):
        return False
    return math.isnan(kept) or f1 > kept


def augment_settings(args):
    """The four augmentation flags -> None when none is given, else {"blur_sigmas", "blur_prob", "saturate_prob", "max_gain"}.
    Raises Refusal."""
    given = [getattr(args, k, None) for k in ("blur_sigmas", "blur_prob", "saturate_prob", "max_gain")]
    if all(v is None for v in given):
        return None
    sigmas = []
    if args.blur_sigmas is not None:
        try:
            sigmas = [float(v) for v in args.blur_sigmas.split(",")]
        except ValueError:
            raise Refusal("--blur-sigmas %r: expected comma-separated numbers" % args.blur_sigmas)
    if len(sigmas) > trainer.AUGMENT_MAX_LEVELS - 1:
        raise Refusal("--blur-sigmas: at most %d levels" % (trainer.AUGMENT_MAX_LEVELS - 1))
    for v in sigmas:
        try:
            trainset.gaussian_taps(v)
        except ValueError as e:
            raise Refusal("--blur-sigmas: %s" % e)
    blur_prob = (0.5 if sigmas else 0.0) if args.blur_prob is None else args.blur_prob
    sat_prob = 0.0 if args.saturate_prob is None else args.saturate_prob
    max_gain = (2.0 if sat_prob > 0 else 1.0) if args.max_gain is None else args.max_gain
    for name, v in (("--blur-prob", blur_prob), ("--saturate-prob", sat_prob)):
        if not 0.0 <= v <= 1.0:   # (a NaN fails both comparisons)
            raise Refusal("%s %r is not a probability" % (name, v))
    if blur_prob > 0 and not sigmas:
        raise Refusal("--blur-prob needs --blur-sigmas")
    if not (math.isfinite(max_gain) and max_gain >= 1.0):
        raise Refusal("--max-gain %r: a gain is finite and >= 1" % max_gain)
    return {"blur_sigmas": sigmas, "blur_prob": float(blur_prob), "saturate_prob": float(sat_prob), "max_gain": float(max_gain)}


def resolve_model(name: str) -> str:
    """As the drivers do (driver.run): a directory as given, else <repository>/models/<name> (UMX_MODELS_DIR overrides)."""
    if os.path.isdir(name):
        return name
    from .driver import models_root
    return os.path.join(models_root(os.path.dirname(os.path.dirname(os.path.realpath(__file__)))), name)


def options_for(kind: str, seed: int, lr0=None) -> trainer.TrainOptions:
    make = {"legacy": trainer.legacy_options, "solo": trainer.solo_options, "duo": trainer.duo_options}[kind]
    kw = {"seed": int(seed)}
    if lr0 is not None:
        kw["lr0"] = float(lr0)
    return make(**kw)


def prepare(args):
    """Everything that needs no device: the model, both sets read and checked.  Raises Refusal."""
    if args.steps < 1 or args.eval_every < 1 or args.pages < 1 or args.batch < 0:
        raise Refusal("--steps, --eval-every and --pages must be positive, --batch non-negative")
    augment_settings(args)
    warp_settings(args)
    elastic_settings(args)
    border_settings(args)
    object_settings(args)
    scratch = init_settings(args) is not None
    path = resolve_model(args.model)
    if not os.path.isdir(path):
        raise Refusal("model %s: no such directory (%s)" % (args.model, path))
    for what, d in (("--train", args.train), ("--valid", args.valid)):
        if not os.path.isdir(d):
            raise Refusal("%s %s: no such directory" % (what, d))
        if not trainset.dataset_indices(d):
            raise Refusal("%s %s holds no I%%05d_Img.tif samples" % (what, d))
    if scratch:
        # hyper-parameters only: the artefacts carry no blob, and the normalisation the new model is trained with
        try:
            hp0 = model.load_hparams_dir(path)[0]
            init = init_settings(args, path)
        except (FileNotFoundError, KeyError) as e:
            raise Refusal("model %s has no hyper-parameters to start from: %s" % (args.model, e))
        art = model.ModelArtefacts(hp0, None, init["mean"], init["std"])
    else:
        try:
            art = model.load_model_dir(path)
        except FileNotFoundError as e:
            raise Refusal("model %s has no weights to fine-tune: %s" % (args.model, e))
    hp = art.hp
    elastic_settings(args, hp.imSize)
    border_settings(args, hp)
    object_settings(args, hp)
    sets = []
    for what, d in (("--train", args.train), ("--valid", args.valid)):
        try:
            ds = trainset.read_dataset_dir(d, args.pages, hp.nChannels, art.mean, art.std)
        except ValueError as e:
            raise Refusal("%s: %s (the model takes %d channel(s), --pages is %d)" % (what, e, hp.nChannels, args.pages))
        if ds.size < hp.imSize:
            raise Refusal("%s: samples are %d x %d, smaller than the model's %d x %d tile" % (what, ds.size, ds.size, hp.imSize,
                                                                                         hp.imSize))
        sets.append(ds)
    return art, sets[0], sets[1]


def run(args) -> int:
    art, train_ds, valid_ds = prepare(args)
    aug = augment_settings(args)
    warp = warp_settings(args)
    hp = art.hp
    elastic = elastic_settings(args, hp.imSize)
    border = border_settings(args, hp)
    objects = object_settings(args, hp)
    oopts = None if objects is None else trainset.ObjectOptions(objects["class"], objects["min_area"])
    by_f1 = objects is not None and objects["select"] == "object"
    kind = trainset.graph_kind(hp)
    lw = trainset.LABEL_WEIGHTS[kind]
    init = init_settings(args, resolve_model(args.model))
    if init is None:
        tr = trainer.Trainer(hp, art.blob, options_for(kind, args.seed, args.lr0), batch=args.batch, device=args.device)
    else:
        if has_weights(resolve_model(args.model)):
            init["weights_not_read"] = True
            print("--from-scratch: the weights of model %s are not read (it supplies the hyper-parameters only)" % args.model, flush=True)
        tr = trainer.Trainer.from_scratch(hp, options_for(kind, args.seed, args.lr0), init["seed"], init["std_dev0"], batch=args.batch,
                                          device=args.device)
    try:
        bopts = None if border is None else trainset.BorderOptions(border["sigma"], border["class"])
        ts = trainset.upload(tr, train_ds, lw, border=bopts)
        vs = trainset.upload(tr, valid_ds, lw, border=bopts)
        if border is not None:
            border["computed"] = [ts.border_computed, vs.border_computed]
        mb, mc = trainset.default_jitter(kind, art.std)
        akw = {}
        if aug is not None:
            ts.set_augment(trainset.AugmentTable.from_sigmas(aug["blur_sigmas"], art.mean, art.std))
            akw = dict(blur_levels=len(aug["blur_sigmas"]) + 1, blur_prob=aug["blur_prob"], saturate_prob=aug["saturate_prob"],
                       max_gain=aug["max_gain"])
        if warp is not None:
            akw.update(rotate_prob=warp["rotate_prob"], zoom_prob=warp["zoom_prob"], zoom_range=tuple(warp["zoom_range"]))
        if elastic is not None:
            akw.update(elastic_prob=elastic["prob"], elastic_sigma=elastic["sigma"], elastic_grid=elastic["grid"])
        sampler = trainset.Sampler(args.seed, train_ds.n_samples, tr.batch, train_ds.size, hp.imSize, args.pages, mb, mc,
                                   transforms=args.transforms, **akw)
        vdesc = trainset.validation_descriptors(valid_ds.n_samples, valid_ds.size, hp.imSize)
        os.makedirs(args.out, exist_ok=True)
        log_path = os.path.join(args.out, LOG_NAME)
        best = None
        train_loss = None
        with open(log_path, "w") as log:
            settings = {k: v for k, v in (("init", init), ("augment", aug), ("warp", warp), ("elastic", elastic), ("border", border),
                                          ("objects", objects)) if v is not None}
            if settings:
                log.write(json.dumps(settings) + "\n")
            for step in range(args.steps + 1):
                if step % args.eval_every == 0 or step == args.steps:
                    ev = tr.evaluate(vs, vdesc) if oopts is None else tr.evaluate(vs, vdesc, objects=oopts)
                    err = [None if math.isnan(e) else float(e) for e in ev["per_class_error"]]
                    seen = [e for e in err if e is not None]
                    mean_err = float(np.mean(seen)) if seen else float("nan")
                    rec = {"step": step, "train_loss": train_loss, "loss": ev["loss"], "per_class_error": err, "mean_error": mean_err,
                           "labelled": [int(v) for v in ev["counts"][1]]}
                    f1 = float("nan")
                    if oopts is not None:
                        f1 = ev["objects"]["f1"]
                        rec["objects"] = dict(ev["objects"], f1=None if math.isnan(f1) else f1)
                    log.write(json.dumps(rec) + "\n")
                    log.flush()
                    print("step %d: validation loss %.6g, per-class error %s" % (step, ev["loss"], err), flush=True)
                    if oopts is not None:
                        print("step %d: objects %s" % (step, json.dumps(rec["objects"])), flush=True)
                    keep = better_f1(f1, None if best is None else best[0]) if by_f1 else best is None or mean_err < best[0]
                    if keep:
                        best = (f1 if by_f1 else mean_err, step)
                        model.save_converted(model.ModelArtefacts(hp, tr.blob(), art.mean, art.std), args.out)
                if step == args.steps:
                    break
                if elastic is not None:
                    d, a, w, e = sampler.next_elastic()
                    tr.step_elastic(ts, d, None if aug is None else a, None if warp is None else w, e)
                elif warp is not None:
                    d, a, w = sampler.next_warped()
                    tr.step_warped(ts, d, None if aug is None else a, w)
                elif aug is None:
                    tr.step_sampled(ts, sampler.next())
                else:
                    tr.step_augmented(ts, *sampler.next_augmented())
                if (step + 1) % args.eval_every == 0 or step + 1 == args.steps:
                    train_loss = tr.loss()[0]
        print("best %s %.6g at step %d -> %s" % ("object F1" if by_f1 else "mean per-class error", best[0], best[1],
                                                 os.path.join(args.out, model.CONVERTED_NAME)))
    finally:
        tr.close()
    return 0


def main(argv=None) -> int:
    args = build_parser().parse_args(argv)
    try:
        return run(args)
    except Refusal as e:
        print("finetune: error: %s" % e, file=sys.stderr)
        return 2
    except umx.UmxError as e:
        print("finetune: error: %s" % e, file=sys.stderr)
        return 1


if __name__ == "__main__":
    sys.exit(main())
