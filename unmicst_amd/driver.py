"""One command-line driver for every UnMicst tool.

The reference ships the same ``__main__`` block five times with small per-tool differences (UnMicst1-5.py:713-876 solo,
UnMicst2.py:692-835 duo, UnMicst.py:544-678 legacy, UnMicstCyto2.py:679-827).  Here the differences are data
(``TOOLS``) and the flow is written once: read page(s) -> resize -> intensity rescale -> ONE pass of the HIP engine for
all classes -> uint8 recipe -> BigTIFF pages with the reference's names and page order.

Kept identical on purpose (file-level parity): argparse surfaces; 0-based channels in the scripts / 1-based in the
wrapper; the file-type switch on the text after the first dot (solo: after the last dots, with the ``ome.`` special
case); float32 input cast to uint16; the solo quirk that the network sees the *un-rescaled* image (``cells = I`` is
bound before the rescale, UnMicst1-5.py:816-821) while legacy/duo/cyto feed the rescaled one; uint8 truncation twice
(UnMicst1-5.py:848-854); ``_Probabilities_`` pages in reversed class order; ``qc/<stem>_Preview_`` = [contours, raw/max];
default output directory ``<parent of parent>/probability_maps``.

Not kept: ``.czi`` / ``.nd2`` (proprietary readers absent: NotImplementedError, which is what the reference raises for
types it cannot read, UnMicst1-5.py:806); the NVML device probe (replaced by umx_device_mem_info).
"""
from __future__ import annotations

import argparse
import os
import sys
import time
from dataclasses import dataclass

import numpy as np

from . import imtools, tiffio
from .unet2d import UNet2D


@dataclass(frozen=True)
class ToolSpec:
    script: str              # reference script this spec mirrors
    default_model: str
    graph: object            # model.GRAPH_* or None (detect)
    multi_channel: bool      # --channel nargs='+' (solo, duo) vs a single int (legacy, cyto)
    n_inputs: int            # image planes fed to the network (duo: 2)
    split_last: bool         # solo derives stem/type from the LAST dots; the others split at the first dot
    tiff_types: tuple        # extensions read as OME/BigTIFF pages
    infer_rescaled: bool     # False: solo's `cells = I` quirk
    cast_float32: bool
    has_verbose: bool
    qc_dir: bool             # Preview goes to <out>/qc
    suffix_plus_one: bool    # file-name suffix is channel+1 (cyto writes the raw 0-based channel)


TOOLS = {
    "unmicst-solo": ToolSpec("UnMicst1-5.py", "nucleiDAPI1-5", 1, True, 1, True, ("ome.tif", "ome.tiff", "btf"), False,
                             True, True, True, True),
    "unmicst-duo": ToolSpec("UnMicst2.py", "nucleiDAPILAMIN", 1, True, 2, False, ("ome.tif", "ome.tiff", "btf"), True,
                            True, True, True, True),
    "unmicst-legacy": ToolSpec("UnMicst.py", "nucleiDAPI", 0, False, 1, False, ("ome.tif", "ome.tiff", "btf"), True,
                               True, True, True, True),
    "UnMicstCyto2": ToolSpec("UnMicstCyto2.py", "nucleiDAPI", 1, False, 1, False, ("ome.tif", "btf"), True, False,
                             False, False, False),
}


def build_parser(spec: ToolSpec) -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog=spec.script)
    p.add_argument("imagePath", help="path to the .tif file")
    p.add_argument("--model", help="type of model. For example, nuclei vs cytoplasm", default=spec.default_model)
    p.add_argument("--outputPath", help="output path of probability map")
    if spec.multi_channel:
        p.add_argument("--channel", help="channel to perform inference on", nargs="+", default=[0])
    else:
        p.add_argument("--channel", help="channel to perform inference on", type=int, default=0)
    p.add_argument("--classOrder", help="background, contours, foreground", type=int, nargs="+", default=-1)
    p.add_argument("--mean", help="mean intensity of input image. Use -1 to use model", type=float, default=-1)
    p.add_argument("--std", help="mean standard deviation of input image. Use -1 to use model", type=float, default=-1)
    p.add_argument("--scalingFactor", help="factor by which to increase/decrease image size by", type=float, default=1)
    p.add_argument("--stackOutput", help="save probability maps as separate files", action="store_true")
    p.add_argument("--GPU", help="explicitly select GPU", type=int, default=-1)
    p.add_argument("--outlier", help="map percentile intensity to max when rescaling intensity values. "
                                     "Max intensity as default", type=float, default=-1)
    if spec.has_verbose:
        p.add_argument("--verbose", help="display error messages for debugging", action="store_true")
    # the one flag the reference does not have: the reference runs the whole slide once PER CLASS
    # (UnMicst1-5.py:845-863); here one pass yields every class.  For A/B timing this switch takes the reference's shape:
    # host-side pre-processing, then one full pass of the engine per class written.  Same bytes in the files.
    p.add_argument("--compat-per-class", dest="compat_per_class", action="store_true",
                   help="A/B timing only: one full inference pass per output class, like the reference (same output bytes)")
    # three more the reference does not have: the nuclei themselves ("Label mask").  From the uint8 planes
    # this run writes -- whatever --classOrder says about their pages -- the 4-connected objects of one class, labelled on the device:
    # <stem>_Labels_<suffix>.tif (one int32 page) and <stem>_Objects_<suffix>.csv next to the probability files.
    p.add_argument("--labelMask", dest="labelMask", action="store_true",
                   help="also write a label mask of the nuclei (int32 TIFF) and their table (CSV)")
    p.add_argument("--labelClass", dest="labelClass", type=int, default=None,
                   help="class whose objects are labelled, 0-based in the MODEL's class order (not --classOrder's); default: the last")
    p.add_argument("--labelMinArea", dest="labelMinArea", type=int, default=None,
                   help="objects of fewer pixels are dropped from the label mask (default 1)")
    # the labelled objects are the nuclei without their rims (the contour class keeps touching nuclei apart and is every nucleus' outer
    # ring): --labelGrow R grows them back, R pixels at most, over the pixels of --labelGrowClasses
    p.add_argument("--labelGrow", dest="labelGrow", type=int, default=None,
                   help="grow the labelled objects R pixels (1..255) into the classes of --labelGrowClasses; a shared rim is cut "
                        "where two objects meet (default: no growth)")
    p.add_argument("--labelGrowClasses", dest="labelGrowClasses", type=int, nargs="+", default=None,
                   help="classes the objects grow over, 0-based in the MODEL's class order; default: every class but 0 and --labelClass")
    # touching nuclei that the contour class did not keep apart are one object: --labelSplit D cuts an object at its necks (erosion
    # cores of depth D, regrown inside the object), before any --labelGrow
    p.add_argument("--labelSplit", dest="labelSplit", type=int, default=None, metavar="D",
                   help="split the labelled objects at necks of up to 2 D pixels (D 1..8): erosion cores of depth D, regrown inside "
                        "their object (the project's own definition)")
    p.add_argument("--labelSplitCore", dest="labelSplitCore", type=int, default=None, metavar="C",
                   help="erosion cores of fewer pixels seed no object (1..65536, default 1)")
    p.add_argument("--labelSplitRegrow", dest="labelSplitRegrow", type=int, default=None, metavar="L",
                   help="levels the cores grow back inside their object (1..255, default 255)")
    # the regrow cuts a neck on the midline between its cores; --labelFlood P regrows the cores by a level flood on probability plane
    # P instead, so the cut follows that plane's ridge
    p.add_argument("--labelFlood", dest="labelFlood", type=int, default=None, metavar="PLANE",
                   help="with --labelSplit: regrow the cores by a level flood on this probability plane (0-based in the MODEL's class "
                        "order, e.g. the contour class), cutting touching nuclei along its ridge")
    p.add_argument("--labelFloodStep", dest="labelFloodStep", type=int, default=None, metavar="Q",
                   help="the flood rises in levels of Q grey values: a power of two, 1..256 (default 16)")
    p.add_argument("--labelFloodInvert", dest="labelFloodInvert", action="store_true",
                   help="flood on 255 - plane (for a plane that is high inside the nuclei, e.g. --labelClass itself)")
    # erosion cores see geometry alone; --labelHmax H places the seeds by the probability's own peaks instead: the extended maxima of
    # the h-maxima transform of a plane inside the objects, regrown by --labelFlood or by distance
    p.add_argument("--labelHmax", dest="labelHmax", type=int, default=None, metavar="H",
                   help="split the labelled objects by h-maxima seeds instead of --labelSplit: a peak of the seed plane seeds an object "
                        "of its own iff it stands more than H grey values (1..255) above the saddle to a higher one")
    p.add_argument("--labelHmaxPlane", dest="labelHmaxPlane", type=int, default=None, metavar="PLANE",
                   help="with --labelHmax: the probability plane the peaks are taken from (0-based in the MODEL's class order; "
                        "default: --labelClass)")
    p.add_argument("--labelHmaxInvert", dest="labelHmaxInvert", action="store_true",
                   help="with --labelHmax: take the peaks of 255 - plane (the basins of e.g. the contour plane)")
    p.add_argument("--labelHmaxCore", dest="labelHmaxCore", type=int, default=None, metavar="C",
                   help="with --labelHmax: seed components of fewer pixels seed no object (1..65536, default 1)")
    # how bright every labelled object is in the image's own pages: <stem>_Intensities_<suffix>.csv
    p.add_argument("--labelMeasure", dest="labelMeasure", type=int, nargs="*", default=None, metavar="PAGE",
                   help="also write mean, std, min and max of every labelled object in the probability planes and in these pages of "
                        "the input file, 0-based as --channel counts them (no value: every page)")
    # what shape every labelled object has: <stem>_Shapes_<suffix>.csv
    p.add_argument("--labelShape", dest="labelShape", action="store_true",
                   help="also write perimeter, holes, major and minor axis, eccentricity, orientation and extent of every labelled "
                        "object (the grown or split ones with --labelGrow / --labelSplit)")
    # which labelled objects touch: <stem>_Neighbors_<suffix>.csv
    p.add_argument("--labelNeighbors", dest="labelNeighbors", action="store_true",
                   help="also write which labelled objects (the grown or split ones with --labelGrow / --labelSplit) touch, and along "
                        "how many pixel edges")
    p.add_argument("--labelNeighborsReach", dest="labelNeighborsReach", type=int, default=None, metavar="R",
                   help="with --labelNeighbors: objects also count as neighbours when fronts grown R pixels (0..255, default 0) from them "
                        "over the unlabelled pixels meet; the label mask itself is not changed")
    # the convex hull of every labelled object: <stem>_Hulls_<suffix>.csv
    p.add_argument("--labelHull", dest="labelHull", action="store_true",
                   help="also write convex-hull area, solidity, largest and least Feret diameter and hull perimeter of every labelled "
                        "object (the grown or split ones with --labelGrow / --labelSplit)")
    p.add_argument("--labelHullVertices", dest="labelHullVertices", action="store_true",
                   help="with --labelHull: also write the hulls' vertices, corners of the pixel squares (<stem>_HullVertices_<suffix>.csv)")
    # acting on the tables: objects are merged, then dropped, and the rest renumbered on the
    # device before any file is written, so the Labels page and every table are those of the final objects
    p.add_argument("--labelKeep", dest="labelKeep", nargs="+", default=None, metavar="RULE",
                   help="keep only the labelled objects for which every RULE holds and renumber them; a RULE is NAME OP VALUE without "
                        "spaces, OP one of >= <= > < == !=, NAME one of area, border (1 when the object's box touches the image border) "
                        "or a column of the Shapes, Hulls or Intensities file (e.g. 'area>=30' 'border==0' 'pm2_mean>=128')")
    p.add_argument("--labelMerge", dest="labelMerge", type=float, default=None, metavar="F",
                   help="merge touching objects whose shared edges are at least F (0 < F <= 1) of the smaller one's perimeter edges: "
                        "takes back the cuts of --labelSplit / --labelFlood through a body; applied before --labelKeep")
    return p


def check_label_args(parser: argparse.ArgumentParser, args) -> None:
    """The refusals of the label flags that need no model (parser.error: exit status 2, like any bad flag)."""
    if not args.labelMask:
        for flag, v in (("--labelClass", args.labelClass), ("--labelMinArea", args.labelMinArea), ("--labelGrow", args.labelGrow),
                        ("--labelGrowClasses", args.labelGrowClasses), ("--labelMeasure", args.labelMeasure),
                        ("--labelSplit", args.labelSplit), ("--labelSplitCore", args.labelSplitCore),
                        ("--labelSplitRegrow", args.labelSplitRegrow), ("--labelShape", args.labelShape or None),
                        ("--labelFlood", args.labelFlood), ("--labelFloodStep", args.labelFloodStep),
                        ("--labelFloodInvert", args.labelFloodInvert or None), ("--labelHmax", args.labelHmax),
                        ("--labelHmaxPlane", args.labelHmaxPlane), ("--labelHmaxInvert", args.labelHmaxInvert or None),
                        ("--labelHmaxCore", args.labelHmaxCore), ("--labelNeighbors", args.labelNeighbors or None),
                        ("--labelNeighborsReach", args.labelNeighborsReach), ("--labelHull", args.labelHull or None),
                        ("--labelHullVertices", args.labelHullVertices or None), ("--labelKeep", args.labelKeep),
                        ("--labelMerge", args.labelMerge)):
            if v is not None:
                parser.error("%s needs --labelMask" % flag)
        return
    if args.labelClass is not None and args.labelClass < 0:
        parser.error("--labelClass %d: classes are numbered from 0" % args.labelClass)
    if args.labelMinArea is not None and not 1 <= args.labelMinArea <= 65536:
        parser.error("--labelMinArea %d: it must be 1..65536 pixels" % args.labelMinArea)
    if args.labelGrowClasses is not None and args.labelGrow is None:
        parser.error("--labelGrowClasses needs --labelGrow")
    if args.labelGrow is not None and not 1 <= args.labelGrow <= 255:
        parser.error("--labelGrow %d: it must be 1..255 pixels" % args.labelGrow)
    for flag, v in (("--labelSplitCore", args.labelSplitCore), ("--labelSplitRegrow", args.labelSplitRegrow)):
        if v is not None and args.labelSplit is None:
            parser.error("%s needs --labelSplit" % flag)
    if args.labelSplit is not None and not 1 <= args.labelSplit <= 8:
        parser.error("--labelSplit %d: it must be 1..8 pixels" % args.labelSplit)
    if args.labelSplitCore is not None and not 1 <= args.labelSplitCore <= 65536:
        parser.error("--labelSplitCore %d: it must be 1..65536 pixels" % args.labelSplitCore)
    if args.labelSplitRegrow is not None and not 1 <= args.labelSplitRegrow <= 255:
        parser.error("--labelSplitRegrow %d: it must be 1..255 levels" % args.labelSplitRegrow)
    for flag, v in (("--labelSplit", args.labelSplit), ("--labelSplitCore", args.labelSplitCore), ("--labelSplitRegrow", args.labelSplitRegrow)):
        if v is not None and args.labelHmax is not None:
            parser.error("--labelHmax places the seeds itself: it excludes %s" % flag)
    for flag, v in (("--labelHmaxPlane", args.labelHmaxPlane), ("--labelHmaxInvert", args.labelHmaxInvert or None),
                    ("--labelHmaxCore", args.labelHmaxCore)):
        if v is not None and args.labelHmax is None:
            parser.error("%s needs --labelHmax" % flag)
    if args.labelHmax is not None and not 1 <= args.labelHmax <= 255:
        parser.error("--labelHmax %d: it must be 1..255 grey values" % args.labelHmax)
    if args.labelHmaxPlane is not None and not 0 <= args.labelHmaxPlane < 16:
        parser.error("--labelHmaxPlane %d: planes are numbered 0..15 at the most" % args.labelHmaxPlane)
    if args.labelHmaxCore is not None and not 1 <= args.labelHmaxCore <= 65536:
        parser.error("--labelHmaxCore %d: it must be 1..65536 pixels" % args.labelHmaxCore)
    if args.labelFlood is not None and args.labelSplit is None and args.labelHmax is None:
        parser.error("--labelFlood needs --labelSplit")
    for flag, v in (("--labelFloodStep", args.labelFloodStep), ("--labelFloodInvert", args.labelFloodInvert or None)):
        if v is not None and args.labelFlood is None:
            parser.error("%s needs --labelFlood" % flag)
    if args.labelFlood is not None and not 0 <= args.labelFlood < 16:
        parser.error("--labelFlood %d: planes are numbered 0..15 at the most" % args.labelFlood)
    if args.labelFlood is not None and args.labelSplitRegrow not in (None, 255):
        parser.error("--labelSplitRegrow %d: the flood's steps have no bound, with --labelFlood it must be 255" % args.labelSplitRegrow)
    if args.labelFloodStep is not None and args.labelFloodStep not in (1, 2, 4, 8, 16, 32, 64, 128, 256):
        parser.error("--labelFloodStep %d: it must be a power of two, 1..256" % args.labelFloodStep)
    if args.labelNeighborsReach is not None and not args.labelNeighbors:
        parser.error("--labelNeighborsReach needs --labelNeighbors")
    if args.labelNeighborsReach is not None and not 0 <= args.labelNeighborsReach <= 255:
        parser.error("--labelNeighborsReach %d: it must be 0..255 pixels" % args.labelNeighborsReach)
    if args.labelHullVertices and not args.labelHull:
        parser.error("--labelHullVertices needs --labelHull")
    if args.labelMerge is not None and not 0.0 < args.labelMerge <= 1.0:     # (nan fails both)
        parser.error("--labelMerge %r: it must be a fraction above 0 and at most 1" % args.labelMerge)
    for rule in args.labelKeep or ():
        try:
            parse_keep_rule(rule)
        except ValueError as e:
            parser.error("--labelKeep %s" % e)
    for k in args.labelGrowClasses or ():
        if k < 0:
            parser.error("--labelGrowClasses %d: classes are numbered from 0" % k)
    for page in args.labelMeasure or ():
        if page < 0:
            parser.error("--labelMeasure %d: pages are numbered from 0" % page)


def label_grow_classes(parser: argparse.ArgumentParser, args, n_classes: int):
    """The class set of the growth once the model's class count is known (None without --labelGrow); its refusals."""
    if args.labelGrow is None:
        return None
    if args.labelGrowClasses is not None:
        for k in args.labelGrowClasses:
            if k >= n_classes:
                parser.error("--labelGrowClasses %d: the model has classes 0..%d" % (k, n_classes - 1))
        return sorted(set(args.labelGrowClasses))
    cls = n_classes - 1 if args.labelClass is None else args.labelClass
    classes = [k for k in range(1, n_classes) if k != cls]
    if not classes:
        parser.error("--labelGrow: a model of %d classes leaves no class to grow over besides 0 and the labelled one; name them "
                     "with --labelGrowClasses" % n_classes)
    return classes


KEEP_OPS = {">=": np.greater_equal, "<=": np.less_equal, ">": np.greater, "<": np.less, "==": np.equal, "!=": np.not_equal}
MEASURE_COLUMNS = ("mean", "std", "min", "max")


def parse_keep_rule(text: str):
    """'NAME OP VALUE' without spaces -> (name, op, value float, table): table is "objects" (area, border), "shape", "hull", or
    ("pm", k) / ("ch", p) for a column of the Intensities file.  ValueError with the reason for anything else.  Whether the model has
    plane k and the file page p is the caller's check (keep_rule_refusal)."""
    import re
    m = re.fullmatch(r"([A-Za-z_][A-Za-z0-9_]*)(>=|<=|==|!=|>|<)(\S+)", text)
    if not m:
        raise ValueError("%r: a rule is NAME OP VALUE without spaces, OP one of >= <= > < == !=" % text)
    name, op, number = m.groups()
    try:
        value = float(number)
    except ValueError:
        value = float("nan")
    if value != value or value in (float("inf"), float("-inf")):
        raise ValueError("%r: %r is no number" % (text, number))
    if name in ("area", "border"):
        return name, op, value, "objects"
    if name in SHAPE_COLUMNS[1:]:
        return name, op, value, "shape"
    if name in HULL_COLUMNS[1:]:
        return name, op, value, "hull"
    im = re.fullmatch(r"(pm|ch)(\d+)_(%s)" % "|".join(MEASURE_COLUMNS), name)
    if im:
        return name, op, value, (im.group(1), int(im.group(2)))
    raise ValueError("%r: %r is neither area, border nor a column of the Shapes, Hulls or Intensities file" % (text, name))


def keep_rule_refusal(rules, n_classes: int, n_pages) -> str:
    """"" when every parsed rule names a plane the model has (pm<k>) and a page the file has (ch<p>; n_pages None: the file is no
    TIFF whose pages can be measured), else the reason"""
    for name, _, _, table in rules:
        if isinstance(table, tuple) and table[0] == "pm" and table[1] >= n_classes:
            return "%s: the model has planes 0..%d" % (name, n_classes - 1)
        if isinstance(table, tuple) and table[0] == "ch" and (n_pages is None or table[1] >= n_pages):
            return "%s: only pages of a TIFF are measured" % name if n_pages is None else "%s: the file has pages 0..%d" % (name, n_pages - 1)
    return ""


def object_columns(objects, shape) -> dict:
    """the columns a rule reads from the object table alone: area, and border = 1 where the inclusive box touches the image border"""
    H, W = shape
    border = (objects["y0"] == 0) | (objects["x0"] == 0) | (objects["y1"] == H - 1) | (objects["x1"] == W - 1)
    return {"area": objects["area"], "border": border.astype(np.int64)}


def shape_columns(objects, records) -> dict:
    """SHAPE_COLUMNS[1:] -> arrays [N]: umx.shape_descriptors of the records, and extent = area / the area of the table's bounding
    box, one float64 division.  The area the window counts give must be the table's."""
    from . import umx as _umx
    d = _umx.shape_descriptors(records)
    if not np.array_equal(d["area"], objects["area"]):
        raise AssertionError("the shapes counted other pixels than the label table")
    box = (objects["y1"].astype(np.int64) - objects["y0"] + 1) * (objects["x1"].astype(np.int64) - objects["x0"] + 1)
    cols = {n: d[n] for n in SHAPE_COLUMNS[1:-1]}
    cols["extent"] = d["area"].astype(np.float64) / box.astype(np.float64)
    return cols


def hull_columns(objects, records, vertices) -> dict:
    """HULL_COLUMNS[1:] -> arrays [N]: umx.hull_descriptors of the records with the table's areas.  Every object of the table must have
    a hull and no hull fewer pixels' worth of area than the object."""
    from . import umx as _umx
    if len(records) != len(objects) or (records["n_vertices"] < 4).any() or (2 * objects["area"].astype(np.int64) > records["area2"]).any():
        raise AssertionError("the hulls are not those of the label table's objects")
    d = _umx.hull_descriptors(records, vertices, objects["area"])
    return {n: d[n] for n in HULL_COLUMNS[1:]}


def intensity_columns(objects, planes) -> dict:
    """<prefix>_mean, _std, _min, _max -> arrays [N] for planes [(prefix, records umx.LABEL_MEASURE_DTYPE [N])]: what
    write_intensities_csv prints from.  Every plane's count must be the table's area."""
    from . import umx as _umx
    cols = {}
    for prefix, records in planes:
        if not np.array_equal(records["count"], objects["area"]):
            raise AssertionError("the measurement of %s counted other pixels than the label table" % prefix)
        mean, std = _umx.measure_mean_std(records)
        cols.update({prefix + "_mean": mean, prefix + "_std": std, prefix + "_min": records["min"], prefix + "_max": records["max"]})
    return cols


def keep_mask(rules, columns: dict) -> np.ndarray:
    """uint8 [N]: 1 where every rule (name, op, value, ...) holds on its column, compared in float64 on the values the CSV writers
    print from, before formatting (a nan holds only under !=)"""
    n = len(next(iter(columns.values())))
    keep = np.ones(n, bool)
    for name, op, value, *_ in rules:
        keep &= KEEP_OPS[op](np.asarray(columns[name]).astype(np.float64), np.float64(value))
    return keep.astype(np.uint8)


def merge_pairs(contacts, perimeter_edges, fraction: float) -> np.ndarray:
    """int32 [M, 2]: the contacts (umx.LABEL_CONTACT_DTYPE, reach 0) whose shared edges are >= fraction * the lesser of the two
    objects' perimeter edges, compared in float64"""
    pe = np.asarray(perimeter_edges).astype(np.float64)
    a, b = contacts["a"].astype(np.int64), contacts["b"].astype(np.int64)
    take = contacts["edges"].astype(np.float64) >= np.float64(fraction) * np.minimum(pe[a - 1], pe[b - 1])
    return np.stack([a[take], b[take]], axis=1).astype(np.int32).reshape(-1, 2)


def write_objects_csv(path: str, objects) -> None:
    """label,area,y0,x0,y1,x1,centroid_y,centroid_x -- one line per kept object, label order; centroid = sum / area in float64."""
    with open(path, "w") as f:
        f.write("label,area,y0,x0,y1,x1,centroid_y,centroid_x\n")
        area = objects["area"].astype(np.float64)
        cols = [range(1, len(objects) + 1)] + [objects[n].tolist() for n in ("area", "y0", "x0", "y1", "x1")]
        cols += [(objects["sum_y"] / area).tolist(), (objects["sum_x"] / area).tolist()]   # (sums below 2^53: exact in float64)
        f.writelines("%d,%d,%d,%d,%d,%d,%.6f,%.6f\n" % row for row in zip(*cols))


def write_intensities_csv(path: str, objects, planes) -> None:
    """label,area, then <prefix>_mean,_std,_min,_max per measured plane -- one line per object, label order, the floats written the way
    write_objects_csv writes centroids.  planes: [(prefix, records umx.LABEL_MEASURE_DTYPE [N])]; every plane's count must be the
    table's area."""
    c = intensity_columns(objects, planes)
    cols = [range(1, len(objects) + 1), objects["area"].tolist()]
    for prefix, _ in planes:
        cols += [c[prefix + "_" + n].tolist() for n in MEASURE_COLUMNS]
    fmt = "%d,%d" + ",%.6f,%.6f,%d,%d" * len(planes) + "\n"
    with open(path, "w") as f:
        f.write(",".join(["label,area"] + [prefix + "_" + n for prefix, _ in planes for n in ("mean", "std", "min", "max")]) + "\n")
        f.writelines(fmt % row for row in zip(*cols))


SHAPE_COLUMNS = ("label", "area", "perimeter_edges", "perimeter", "euler", "holes", "major_axis_length", "minor_axis_length",
                 "eccentricity", "orientation", "extent")


def write_shapes_csv(path: str, objects, records) -> None:
    """SHAPE_COLUMNS -- one line per object, label order.  records: umx.LABEL_SHAPE_DTYPE [N], turned into the columns by
    umx.shape_descriptors alone; extent = area / the area of the table's bounding box, one float64 division.  The area the window
    counts give must be the table's.  Unlike the centroids and the intensities, whose six decimals say all there is to say about a
    mean of integers, these floats are written with repr: the shortest digits that read back to the same float64."""
    d = shape_columns(objects, records)
    cols = [range(1, len(objects) + 1)] + [d[n].tolist() for n in SHAPE_COLUMNS[1:]]
    with open(path, "w") as f:
        f.write(",".join(SHAPE_COLUMNS) + "\n")
        f.writelines("%d,%d,%d,%r,%d,%d,%r,%r,%r,%r,%r\n" % row for row in zip(*cols))


NEIGHBOR_COLUMNS = ("label_a", "label_b", "shared_edges")


def write_neighbors_csv(path: str, contacts) -> None:
    """NEIGHBOR_COLUMNS -- one line per contact of umx.LABEL_CONTACT_DTYPE records [M], in their order: (label_a, label_b) ascending,
    label_a < label_b."""
    with open(path, "w") as f:
        f.write(",".join(NEIGHBOR_COLUMNS) + "\n")
        f.writelines("%d,%d,%d\n" % row for row in zip(contacts["a"].tolist(), contacts["b"].tolist(), contacts["edges"].tolist()))


HULL_COLUMNS = ("label", "hull_area", "solidity", "feret_max", "feret_min", "hull_perimeter", "n_vertices")
HULL_VERTEX_COLUMNS = ("label", "index", "y", "x")


def write_hulls_csv(path: str, objects, records, vertices) -> None:
    """HULL_COLUMNS -- one line per object, label order.  records, vertices: umx.LABEL_HULL_DTYPE [N] and umx.LABEL_HULL_VERTEX_DTYPE
    [V], turned into the columns by umx.hull_descriptors alone with the table's areas.  Every object of the table must have a hull
    and no hull fewer pixels' worth of area than the object.  The floats are written with repr, as in the Shapes file."""
    d = hull_columns(objects, records, vertices)
    cols = [range(1, len(objects) + 1)] + [d[n].tolist() for n in HULL_COLUMNS[1:]]
    with open(path, "w") as f:
        f.write(",".join(HULL_COLUMNS) + "\n")
        f.writelines("%d,%r,%r,%r,%r,%r,%d\n" % row for row in zip(*cols))


def write_hull_vertices_csv(path: str, records, vertices) -> None:
    """HULL_VERTEX_COLUMNS -- one line per hull vertex, label order and inside a label the list's order (index from 0): corners of
    the pixel squares, 0 <= y <= H and 0 <= x <= W."""
    label = np.repeat(np.arange(1, len(records) + 1), records["n_vertices"])
    index = np.arange(len(vertices)) - np.repeat(records["first"], records["n_vertices"])
    with open(path, "w") as f:
        f.write(",".join(HULL_VERTEX_COLUMNS) + "\n")
        f.writelines("%d,%d,%d,%d\n" % row for row in zip(label.tolist(), index.tolist(), vertices["y"].tolist(), vertices["x"].tolist()))


def measure_pages(labeler, path: str, pages, shape) -> list:
    """[("ch<p>", records [N])] of the pages of the TIFF against the labeler's resident labels.  One page is held at a time: page
    i + 1 is read on a thread while page i is uploaded and measured.  A page that cannot be measured raises before anything is written."""
    from concurrent.futures import ThreadPoolExecutor
    out = []
    if not pages:
        return out
    with ThreadPoolExecutor(1) as pool:
        job = pool.submit(tiffio.imread, path, int(pages[0]))
        for i, page in enumerate(pages):
            plane = job.result()
            job = pool.submit(tiffio.imread, path, int(pages[i + 1])) if i + 1 < len(pages) else None
            if plane.dtype not in (np.uint8, np.uint16):
                raise ValueError("--labelMeasure: page %d of %s is %s; only uint8 and uint16 pages are measured" % (page, path, plane.dtype))
            if tuple(plane.shape) != tuple(shape):
                raise ValueError("--labelMeasure: page %d of %s is %s and the label mask %s" % (page, path, plane.shape, tuple(shape)))
            out.append(("ch%d" % page, labeler.measure(plane)[0]))
    return out


def models_root(script_dir: str) -> str:
    """``<script dir>/models`` like the reference (UnMicst1-5.py:744), overridable with UMX_MODELS_DIR."""
    return os.environ.get("UMX_MODELS_DIR") or os.path.join(script_dir, "models")


def split_name(file_name: str, spec: ToolSpec):
    """-> (stem, type) the way the tool's reference script derives them."""
    if spec.split_last:
        parts = file_name.split(os.extsep)
        if len(parts) < 2:
            raise NotImplementedError("Input filename has no extension")
        if parts[-2] == "ome":
            return os.extsep.join(parts[:-2]), os.extsep.join(parts[-2:])
        return os.extsep.join(parts[:-1]), parts[-1]
    parts = file_name.split(os.extsep, 1)
    if len(parts) < 2:
        raise NotImplementedError("Input filename has no extension")
    return parts[0], parts[1]


def read_plane(path: str, file_type: str, channel: int, spec: ToolSpec) -> np.ndarray:
    if file_type in spec.tiff_types or file_type == "tif":
        I = tiffio.imread(path, key=int(channel))
    else:
        raise NotImplementedError("Don't know how to read image with extension .%s" % file_type)
    if spec.cast_float32 and I.dtype == np.float32:
        I = np.uint16(I)
    return I


def preprocess(I: np.ndarray, scaling: float, outlier: float):
    """resize by --scalingFactor, then rescale intensities to (0, 0.983) -> (resized float image, rescaled image)."""
    hsize = int(float(I.shape[0]) * float(scaling))
    vsize = int(float(I.shape[1]) * float(scaling))
    R = imtools.resize(I, (hsize, vsize))
    max_limit = np.max(R) if outlier == -1 else np.percentile(R, outlier)
    S = imtools.im2double(imtools.rescale_intensity(R, (np.min(R), max_limit), (0, 0.983)))
    return R, S


class _Stages:
    """UMX_CLI_TIMING=1: one JSON line on stderr with the seconds each stage of the run took (tools/cli_walltime.py reads it)."""

    def __init__(self):
        self.on = bool(os.environ.get("UMX_CLI_TIMING"))
        self.t = time.perf_counter()
        self.stages = []
        self.notes = {}
        t0 = float(os.environ.get("UMX_CLI_T0", "0") or 0)
        if self.on and t0:
            self.stages.append(("interpreter_start_and_imports", time.time() - t0))

    def mark(self, name):
        if self.on:
            now = time.perf_counter()
            self.stages.append((name, now - self.t))
            self.t = now

    def note(self, name, value):
        """a value that goes into the report next to the stages' seconds"""
        if self.on:
            self.notes[name] = value

    def report(self):
        if self.on:
            import json
            import resource
            t0 = float(os.environ.get("UMX_CLI_T0", "0") or 0)
            d = {k: round(v, 4) for k, v in self.stages}
            d.update(self.notes)
            if t0:
                d["since_parent_spawned"] = round(time.time() - t0, 4)
            d["user_cpu_s"] = round(resource.getrusage(resource.RUSAGE_SELF).ru_utime, 3)
            print("umx-cli-timing " + json.dumps(d), file=sys.stderr)


def plane_range(raw: np.ndarray):
    """(min, max) of a plane in one pass on host threads (umx_plane_range): the reference's np.min / np.max over the page
    (UnMicst1-5.py:817-821), 2 x 70 ms in numpy for a 16384 x 16384 uint16 page.  The fast path hands the pair to the engine
    (umx_infer_image_raw_range: the upload then overlaps the inference) and reuses the maximum for the preview page."""
    a = np.asarray(raw)
    if a.dtype in (np.uint8, np.uint16) and a.size >= (1 << 20):
        from . import umx as _umx
        return _umx.plane_range(a)
    return int(a.min()), int(a.max())


def preview_u8(raw: np.ndarray, top_value=None) -> np.ndarray:
    """np.uint8(255 * (im2double(raw) / max)) (reference UnMicst1-5.py:809-810,861): a function of the raw value alone, so it is
    evaluated once per possible value with the same float64 operations and looked up -- four float64 passes over a 16384 x
    16384 plane (2.1 GB each) were 1.5 s of the tool's 3 s."""
    if raw.dtype in (np.uint8, np.uint16) and raw.size > (1 << 16):
        top = imtools.im2double(np.asarray(raw.max() if top_value is None else top_value, dtype=raw.dtype))
        vals = imtools.im2double(np.arange(np.iinfo(raw.dtype).max + 1, dtype=raw.dtype))
        return np.uint8(255 * (vals / top))[raw]
    rawI = imtools.im2double(raw)
    return np.uint8(255 * (rawI / np.max(rawI)))


def run(tool: str, argv=None, script_dir: str = None) -> int:
    spec = TOOLS[tool]
    st = _Stages()
    parser = build_parser(spec)
    args = parser.parse_args(argv)
    check_label_args(parser, args)
    script_dir = script_dir or os.path.dirname(os.path.dirname(os.path.realpath(__file__)))
    model_path = args.model if os.path.isdir(args.model) else os.path.join(models_root(script_dir), args.model)

    def channel_list():
        ch = [int(c) for c in args.channel] if spec.multi_channel else [int(args.channel)]
        return ([ch[0], ch[0]] if len(ch) == 1 else ch[:2]) if spec.n_inputs == 2 else [ch[0]]

    label_art = None
    if args.labelMask:
        from . import model as _model
        label_art = _model.load_model_dir(model_path, None, synthetic_if_missing=os.environ.get("UMX_SYNTHETIC_WEIGHTS", "0") not in ("", "0"))
        if args.labelClass is not None and args.labelClass >= label_art.hp.nClasses:
            parser.error("--labelClass %d: the model has classes 0..%d" % (args.labelClass, label_art.hp.nClasses - 1))
        grow_classes = label_grow_classes(parser, args, label_art.hp.nClasses)
        if args.labelFlood is not None and args.labelFlood >= label_art.hp.nClasses:
            parser.error("--labelFlood %d: the model has planes 0..%d" % (args.labelFlood, label_art.hp.nClasses - 1))
        if args.labelHmaxPlane is not None and args.labelHmaxPlane >= label_art.hp.nClasses:
            parser.error("--labelHmaxPlane %d: the model has planes 0..%d" % (args.labelHmaxPlane, label_art.hp.nClasses - 1))
    measure_pages_arg = None
    if args.labelMeasure is not None:
        ftype = split_name(os.path.basename(args.imagePath), spec)[1]
        if not (ftype in spec.tiff_types or ftype == "tif"):     # (what read_plane would say after the set-up)
            raise NotImplementedError("Don't know how to read image with extension .%s" % ftype)
        n_pages = tiffio.num_pages(args.imagePath)
        measure_pages_arg = list(args.labelMeasure) or list(range(n_pages))
        for page in measure_pages_arg:
            if page >= n_pages:
                parser.error("--labelMeasure %d: the file has pages 0..%d" % (page, n_pages - 1))
    keep_rules = [parse_keep_rule(rule) for rule in args.labelKeep or ()]
    if keep_rules:
        ftype = split_name(os.path.basename(args.imagePath), spec)[1]
        pages_known = any(isinstance(r[3], tuple) and r[3][0] == "ch" for r in keep_rules) and (ftype in spec.tiff_types or ftype == "tif")
        why = keep_rule_refusal(keep_rules, label_art.hp.nClasses, tiffio.num_pages(args.imagePath) if pages_known else None)
        if why:
            parser.error("--labelKeep " + why)

    # the page(s) are read on a thread while the engine is set up (model load, planning, weight packing: 0.2 - 0.6 s against
    # 0.18 s of file reading for a 16384 x 16384 page; both release the GIL).  An error of the read surfaces where the reference
    # reads, after the set-up.
    from concurrent.futures import ThreadPoolExecutor
    _pool = ThreadPoolExecutor(1)
    _ftype = split_name(os.path.basename(args.imagePath), spec)[1]
    _pages = _pool.submit(lambda: [read_plane(args.imagePath, _ftype, ch, spec) for ch in channel_list()])
    if args.GPU == -1:
        print("automatically choosing GPU")
    try:
        if args.labelMask:   # (the class count comes from the model: its directory is read first, the engine set up after the check)
            UNet2D.setupWithArtefacts(label_art, args.GPU, args.mean, args.std)
        else:
            UNet2D.singleImageInferenceSetup(model_path, args.GPU, args.mean, args.std, graph=None)
    except BaseException:
        _pool.shutdown(wait=True)
        raise
    print("Using GPU " + str(UNet2D.Engine.device))
    st.mark("setup")
    reuse_before = UNet2D.reuse_pass
    try:
        n_class = UNet2D.hp["nClasses"]
        image_path = args.imagePath
        channels = [int(c) for c in args.channel] if spec.multi_channel else [int(args.channel)]
        first = channels[0]
        if spec.n_inputs == 2:
            channels = [first, first] if len(channels) == 1 else channels[:2]
            print("Using channels %d and %d" % (channels[0] + 1, channels[1] + 1))
        else:
            channels = [first]
            if spec.multi_channel:
                print("Using channel " + str(first + 1))
        parent = os.path.dirname(os.path.dirname(image_path))
        stem, file_type = split_name(os.path.basename(image_path), spec)

        top_value = None                      # max of the preview plane where the fast path has found it already
        try:
            raws = _pages.result()
        finally:
            _pool.shutdown(wait=True)
        raw = raws[-1]                        # the reference keeps the last plane read for the preview (rawI)
        raw_shape = raw.shape[:2]
        class_order = range(n_class) if args.classOrder == -1 else args.classOrder
        st.mark("read")

        out_dir = args.outputPath if args.outputPath else parent + "//probability_maps"
        os.makedirs(out_dir, exist_ok=True)
        qc_dir = out_dir + "//qc" if spec.qc_dir else out_dir
        if spec.qc_dir:
            os.makedirs(qc_dir, exist_ok=True)
        suffix = str(first + 1) if spec.suffix_plus_one else str(first)

        # fast path: the whole pre/post-processing -- im2double, both resizes at --scalingFactor != 1, min/max (or the
        # --outlier percentile, exact by radix selection) + rescale, the double uint8 cast -- runs on the GPU next to the
        # inference (umx_infer_image_raw / _raw_scaled / _raw_outlier): no float64 upload / float16 download.
        fast = (all(r.dtype in (np.uint8, np.uint16) for r in raws)
                and len({(r.shape, r.dtype) for r in raws}) == 1 and not os.environ.get("UMX_NO_RAW_PATH")
                and not args.compat_per_class)
        if args.compat_per_class:
            UNet2D.reuse_pass = False            # every singleImageInference below is a whole pass (UnMicst1-5.py:848,867,872)
        preview_job = None
        if fast:
            stack_raw = np.stack(raws) if spec.n_inputs == 2 else raws[0]
            # the preview page (a table look-up over the raw plane, 0.1 s for 16384 x 16384) on a thread under the engine call
            if raw.size > (1 << 22):
                _pool2 = ThreadPoolExecutor(1)
                preview_job = _pool2.submit(lambda: preview_u8(raw, plane_range(raw)[1]))
                _pool2.shutdown(wait=False)
            if args.outlier != -1 and spec.infer_rescaled:   # (a tool that feeds the un-rescaled plane ignores the limit)
                u8_planes = UNet2D.singleImageInferenceRawOutlier(stack_raw, args.scalingFactor, args.outlier, "accumulate")
            elif float(args.scalingFactor) == 1.0:
                # (the page's extrema from the host pass the reference makes too: the engine then starts on the first rows while
                # the rest of the page is still crossing the bus)
                ranges = [plane_range(r) for r in raws] if spec.infer_rescaled else None
                if ranges:
                    top_value = ranges[-1][1]
                u8_planes = UNet2D.singleImageInferenceRaw(stack_raw, spec.infer_rescaled, "accumulate", value_range=ranges)
            else:   # both resizes (skimage defaults) run on the device too
                u8_planes = UNet2D.singleImageInferenceRawScaled(stack_raw, args.scalingFactor, spec.infer_rescaled, "accumulate")

            def plane_u8(k):
                return u8_planes[k]
            st.mark("engine")
        else:
            planes_in = []
            for r in raws:
                resized, rescaled = preprocess(r, args.scalingFactor, args.outlier)
                planes_in.append(rescaled if spec.infer_rescaled else resized)
            cells = np.stack(planes_in) if spec.n_inputs == 2 else planes_in[0]

            def plane_u8(k):
                return imtools.to_uint8_via_resize(UNet2D.singleImageInference(cells, "accumulate", k), raw_shape)

        if args.stackOutput:
            stack = out_dir + "//" + stem + "_Probabilities_" + suffix + ".tif"
            preview = qc_dir + "//" + stem + "_Preview_" + suffix + ".tif"
            for page, k in enumerate(class_order[::-1]):   # reversed "to align with ilastik" (UnMicst1-5.py:848)
                pm = plane_u8(k)
                tiffio.imsave(stack, pm, append=page > 0)
                if page == 1:
                    tiffio.imsave(preview, pm, append=False)
                    tiffio.imsave(preview, preview_job.result() if preview_job else preview_u8(raw, top_value), append=True)
        else:
            cont = out_dir + "//" + stem + "_ContoursPM_" + suffix + ".tif"
            tiffio.imsave(cont, plane_u8(class_order[1]), append=False)
            tiffio.imsave(cont, preview_job.result() if preview_job else preview_u8(raw, top_value), append=True)
            tiffio.imsave(out_dir + "//" + stem + "_NucleiPM_" + suffix + ".tif", plane_u8(class_order[2]), append=False)
        st.mark("write")
        if args.labelMask:
            from . import umx as _umx
            stack_u8 = u8_planes if fast else np.stack([plane_u8(k) for k in range(n_class)])
            with _umx.Labeler(UNet2D.Engine.device) as labeler:
                labels, objects = labeler.run(stack_u8, args.labelClass, 1 if args.labelMinArea is None else args.labelMinArea,
                                              grow=args.labelGrow or 0, grow_classes=grow_classes, split=args.labelSplit or 0,
                                              split_core=args.labelSplitCore or 1, split_regrow=args.labelSplitRegrow or 255,
                                              flood=args.labelFlood, flood_step=args.labelFloodStep or _umx.FLOOD_DEFAULT_STEP,
                                              flood_invert=args.labelFloodInvert, hmax=args.labelHmax, hmax_plane=args.labelHmaxPlane,
                                              hmax_invert=args.labelHmaxInvert, hmax_core=args.labelHmaxCore or 1)
                if args.labelMerge is not None or keep_rules:
                    # merge, then drop, on the device: every file below is written from the final resident labels
                    st.mark("label")
                    n0 = len(objects)
                    if args.labelMerge is not None:
                        perimeter_edges = _umx.shape_descriptors(labeler.shape())["perimeter_edges"]
                        pairs = merge_pairs(labeler.contacts(reach=0), perimeter_edges, args.labelMerge)
                        labels, objects, _ = labeler.relabel(pairs=pairs, want_labels=not keep_rules)
                    merged = n0 - len(objects)
                    if keep_rules:
                        tables = {r[3] for r in keep_rules}
                        columns = object_columns(objects, stack_u8.shape[1:])
                        if "shape" in tables:
                            columns.update(shape_columns(objects, labeler.shape()))
                        if "hull" in tables:
                            columns.update(hull_columns(objects, *labeler.hull()))
                        if any(isinstance(t, tuple) and t[0] == "pm" for t in tables):
                            pm = labeler.measure(stack_u8)
                            columns.update(intensity_columns(objects, [("pm%d" % k, pm[k]) for k in range(len(pm))]))
                        pages = sorted(t[1] for t in tables if isinstance(t, tuple) and t[0] == "ch")
                        columns.update(intensity_columns(objects, measure_pages(labeler, image_path, pages, stack_u8.shape[1:])))
                        labels, objects, _ = labeler.relabel(keep=keep_mask(keep_rules, columns))
                    dropped = n0 - merged - len(objects)
                    print("Label relabel: %d objects from %d (%d dropped, %d merged away)" % (len(objects), n0, dropped, merged))
                    st.note("label_relabel", {"n_objects": len(objects), "n_before": n0, "dropped": dropped, "merged_away": merged})
                    st.mark("relabel")
                tiffio.imsave(out_dir + "//" + stem + "_Labels_" + suffix + ".tif", labels, append=False)
                write_objects_csv(out_dir + "//" + stem + "_Objects_" + suffix + ".csv", objects)
                st.mark("label_write" if args.labelMerge is not None or keep_rules else "label")
                if args.labelSplit:
                    c = labeler.split_counts()
                    print("Label split: %d objects from %d (%d with a core), %d pixels unreached"
                          % (c["n_objects"], c["n_before"], c["n_cored"], c["unreached"]))
                    st.note("label_split", c)
                if args.labelHmax is not None:
                    c = labeler.hmax_counts()
                    print("Label hmax: %d seed pixels, %d objects from %d (%d with a core), reconstructions in %d and %d launches"
                          % ((c["seed_pixels"], c["n_objects"], c["n_before"], c["n_cored"]) + tuple(c["recon_launches"])))
                    st.note("label_hmax", c)
                if args.labelFlood is not None:
                    c = labeler.flood_counts()
                    print("Label flood: %d pixels claimed at %d levels in %d launches, %d pixels unreached"
                          % (c["claimed"], c["levels_claimed"], c["launches"], c["unreached"]))
                    st.note("label_flood", c)
                if measure_pages_arg is not None:
                    # the labels (the grown ones with --labelGrow) are still on the device: the planes the labeler just used, then
                    # the file's pages one at a time; the file is written only when every page has been measured
                    pm = labeler.measure(stack_u8)
                    measured = [("pm%d" % k, pm[k]) for k in range(len(pm))]
                    measured += measure_pages(labeler, image_path, measure_pages_arg, labels.shape)
                    write_intensities_csv(out_dir + "//" + stem + "_Intensities_" + suffix + ".csv", objects, measured)
                    st.mark("measure")
                if args.labelShape:
                    write_shapes_csv(out_dir + "//" + stem + "_Shapes_" + suffix + ".csv", objects, labeler.shape())
                    st.mark("shape")
                if args.labelNeighbors:
                    contacts = labeler.contacts(reach=args.labelNeighborsReach or 0)
                    write_neighbors_csv(out_dir + "//" + stem + "_Neighbors_" + suffix + ".csv", contacts)
                    degree = _umx.contact_degrees(contacts, len(objects))[0]
                    print("Label neighbors: %d contacts, largest degree %d" % (len(contacts), int(degree.max()) if len(degree) else 0))
                    st.note("label_neighbors", dict(labeler.contacts_stats(), contacts=len(contacts)))
                    st.mark("neighbors")
                if args.labelHull:
                    hulls, hull_vertices = labeler.hull()
                    write_hulls_csv(out_dir + "//" + stem + "_Hulls_" + suffix + ".csv", objects, hulls, hull_vertices)
                    if args.labelHullVertices:
                        write_hull_vertices_csv(out_dir + "//" + stem + "_HullVertices_" + suffix + ".csv", hulls, hull_vertices)
                    st.mark("hull")
    finally:
        if args.compat_per_class:
            UNet2D.reuse_pass = reuse_before
        UNet2D.singleImageInferenceCleanup()
        st.mark("cleanup")
        st.report()
    return 0


def main(tool: str, script_file: str) -> None:
    # the per-file tools never import torch: they take the system ROCm runtime (umx._bind_hip_runtime: `system`; in every other
    # process libumx binds the runtime an installed PyTorch bundles, so that a later `import torch` shares it)
    os.environ.setdefault("UMX_HIP_RUNTIME", "system")
    rc = run(tool, None, os.path.dirname(os.path.realpath(script_file)))
    # every output file is written and closed, the engine destroyed: what is left is interpreter finalisation and the unloading of the
    # HIP runtime, 0.2 s of a 0.9 s tool.  UMX_NO_FAST_EXIT=1 leaves through sys.exit as usual.
    if os.environ.get("UMX_NO_FAST_EXIT"):
        sys.exit(rc)
    sys.stdout.flush()
    sys.stderr.flush()
    os._exit(rc)
