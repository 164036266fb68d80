"""CPU checks of the label mask's contacts: the numpy restatement against an edge-by-edge
loop and against lists known on paper, the record's size, the host-only limits of umx_label_contact_check, the UMX_CONTACT_ macros,
umx.contact_degrees, the Neighbors file, the drivers' two refusals, and the host arithmetic of the library (limits, first table,
ordering of a scattered list) as a stand-alone program under the host sanitizers.  No kernel runs here:
tests/test_gpu_label_contacts.py holds the device to the restatement."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import helpers
import label_contact_ref as ref
from unmicst_amd import build, driver, model, umx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    build.build()
    return umx.load()


def test_restatement_against_the_edge_loop():
    for name, labels, N, known in ref.hand_made():
        got = ref.contacts(labels, N)
        assert ref.as_tuples(got) == ref.contacts_slow(labels, N) == known, name
        assert got.dtype == ref.RECORD and not got["reserved"].any()
    seen = 0
    for H, W in ((1, 1), (1, 9), (2, 65), (3, 7), (4, 140), (5, 30), (9, 64)):
        labels, N = ref.mosaic(H, W)
        got = ref.as_tuples(ref.contacts(labels, N))
        assert got == ref.contacts_slow(labels, N), (H, W)
        assert got == sorted(got) and all(1 <= a < b <= N and n >= 1 for a, b, n in got)
        seen += len(got)
    assert seen > 200
    labels, N = ref.mosaic(4, 140)
    assert ref.has_long_border(labels) and (1, 2, ref.LONG) in ref.as_tuples(ref.contacts(labels[:2], N))


def test_restatement_of_the_reach():
    """two blocks 5 apart: fronts of R levels meet iff 2 R >= 5, along the blocks' common height; a third object between them takes
    both contacts; R = 0 is the plain list; the labels are not changed"""
    lab = np.zeros((8, 16), np.int32)
    lab[2:6, 1:4] = 1
    lab[2:6, 9:12] = 2
    before = lab.copy()
    assert len(ref.contacts(lab, 2, 0)) == 0 and len(ref.contacts(lab, 2, 2)) == 0
    got = ref.as_tuples(ref.contacts(lab, 2, 3))
    assert len(got) == 1 and got[0][:2] == (1, 2) and got[0][2] >= 4
    lab[2:6, 6] = 3
    assert [t[:2] for t in ref.as_tuples(ref.contacts(lab, 3, 3))] == [(1, 3), (2, 3)]
    lab[2:6, 6] = 0
    assert np.array_equal(lab, before)
    S = ref.reached(lab, 2, 3)
    assert np.array_equal(S[lab > 0], lab[lab > 0]) and (S > 0).sum() > (lab > 0).sum()
    bad = lab.copy()
    bad[0, 0] = 7                                                # outside 1..N: domain like any 0
    assert np.array_equal(ref.reached(bad, 2, 3), S)


def test_limits(lib):
    ok = umx.label_contact_check
    assert ok(1, 1) == "" and ok(1, 2 ** 31 - 1, 2 ** 31 - 1, 255) == "" and ok(46340, 46340, 0, 0) == "" and ok(2 ** 31 - 1, 1) == ""
    assert "at least 1" in ok(0, 5) and "at least 1" in ok(5, 0) and "at least 1" in ok(-1, 5)
    assert "flat pixel index" in ok(2, 2 ** 30) and "flat pixel index" in ok(46341, 46341) and "flat pixel index" in ok(65536, 65536)
    assert ok(1, 70000) == ""                                    # (no bound on a side: nothing here squares a coordinate)
    assert "n_objects" in ok(4, 4, -1) and "n_objects" in ok(4, 4, 2 ** 31) and ok(4, 4, 2 ** 31 - 1) == ""
    assert "reach" in ok(4, 4, 1, -1) and "reach" in ok(4, 4, 1, 256) and ok(4, 4, 1, 255) == "" and ok(4, 4, 1, 0) == ""
    assert lib.umx_label_contact_check(0, 0, 0, 0, None, 0) == umx.ERR_INVALID and lib.umx_label_contact_check(1, 1, 0, 0, None, 0) == 0
    buf = ctypes.create_string_buffer(8)
    assert lib.umx_label_contact_check(0, 0, 0, 0, buf, 8) == umx.ERR_INVALID and len(buf.value) == 7


def test_binding_mirrors_the_header(lib):
    header = open(os.path.join(ROOT, "include", "umx.h")).read()
    assert umx.LABEL_CONTACT_DTYPE == ref.RECORD and umx.LABEL_CONTACT_DTYPE.itemsize == 16 and ctypes.sizeof(umx.LabelContact) == 16
    body = re.search(r"typedef struct umx_label_contact \{(.*?)\} umx_label_contact;\s*/\* 16 bytes \*/", header, re.S).group(1)
    fields = [(t, n.strip()) for t, decl in re.findall(r"(u?int\d+_t) ([\w, ]+);", body) for n in decl.split(",")]
    assert tuple(n for _, n in fields) == umx.LABEL_CONTACT_DTYPE.names == tuple(n for n, _ in umx.LabelContact._fields_)
    ctype = {"int32_t": ctypes.c_int32, "uint32_t": ctypes.c_uint32, "int64_t": ctypes.c_int64}

    class Record(ctypes.Structure):                              # the header's record, field by field
        _fields_ = [(n, ctype[t]) for t, n in fields]
    assert ctypes.sizeof(Record) == 16
    for name, _ in Record._fields_:
        assert getattr(Record, name).offset == umx.LABEL_CONTACT_DTYPE.fields[name][1] == getattr(umx.LabelContact, name).offset, name
    body = re.search(r"typedef struct umx_label_contact_stats \{(.*?)\} umx_label_contact_stats;\s*/\* 32 bytes \*/", header, re.S).group(1)
    fields = [(t, n.strip()) for t, decl in re.findall(r"(u?int\d+_t) ([\w, ]+);", body) for n in decl.split(",")]
    assert [(n, ctype[t]) for t, n in fields] == umx._LabelContactStats._fields_ and ctypes.sizeof(umx._LabelContactStats) == 32
    macros = {k: int(v) for k, v in re.findall(r"#define (UMX_CONTACT_\w+) (\d+)", header)}
    assert macros == {"UMX_CONTACT_MAX_REACH": umx.CONTACT_MAX_REACH, "UMX_CONTACT_TABLE_MIN": umx.CONTACT_TABLE_MIN,
                      "UMX_CONTACT_TABLE_MAX": umx.CONTACT_TABLE_MAX, "UMX_CONTACT_PROBE_MAX": umx.CONTACT_PROBE_MAX,
                      "UMX_CONTACT_DEVICE_SORT_MAX": umx.CONTACT_DEVICE_SORT_MAX, "UMX_CONTACT_ORDER_NONE": umx.CONTACT_ORDER_NONE,
                      "UMX_CONTACT_ORDER_DEVICE": umx.CONTACT_ORDER_DEVICE, "UMX_CONTACT_ORDER_HOST": umx.CONTACT_ORDER_HOST}
    assert set(re.findall(r"UMX_CONTACT_\w+", header)) == set(macros)                 # no enumerator, no stray name
    assert umx.CONTACT_MAX_REACH == 255 == umx.LABEL_MAX_GROW and umx.CONTACT_TABLE_MIN & (umx.CONTACT_TABLE_MIN - 1) == 0
    assert umx.CONTACT_TABLE_MAX & (umx.CONTACT_TABLE_MAX - 1) == 0 and umx.CONTACT_PROBE_MAX <= umx.CONTACT_TABLE_MIN < umx.CONTACT_TABLE_MAX
    raw = ctypes.CDLL(build.lib_path())
    for name in ("umx_label_contact_check", "umx_labeler_contacts", "umx_labeler_contacts_dev", "umx_labeler_contacts_last_ms",
                 "umx_labeler_contacts_last_stats"):
        assert hasattr(raw, name) and name in umx.EXPORTS


def test_contact_degrees():
    rec = np.array([(1, 2, 3, 0), (1, 4, 5, 0), (2, 4, 1, 0), (4, 6, 2, 0)], umx.LABEL_CONTACT_DTYPE)
    degree, shared = umx.contact_degrees(rec, 6)
    assert degree.tolist() == [2, 2, 0, 3, 0, 1] and shared.tolist() == [8, 4, 0, 8, 0, 2]
    assert degree.dtype == shared.dtype == np.int64 and degree.sum() == 2 * len(rec) and shared.sum() == 2 * int(rec["edges"].sum())
    degree, shared = umx.contact_degrees(rec[:0], 3)
    assert degree.tolist() == [0, 0, 0] == shared.tolist()
    assert [len(v) for v in umx.contact_degrees(rec[:0], 0)] == [0, 0]
    big = np.array([(1, 2, 2 ** 32 - 1, 0), (1, 3, 2 ** 32 - 1, 0)], umx.LABEL_CONTACT_DTYPE)
    assert umx.contact_degrees(big, 3)[1].tolist() == [2 ** 33 - 2, 2 ** 32 - 1, 2 ** 32 - 1]
    for bad in ([(0, 2, 1, 0)], [(2, 2, 1, 0)], [(3, 2, 1, 0)], [(1, 7, 1, 0)]):
        with pytest.raises(ValueError):
            umx.contact_degrees(np.array(bad, umx.LABEL_CONTACT_DTYPE), 6)
    name, labels, N, known = [c for c in ref.hand_made() if c[0] == "enclosed"][0]
    degree, shared = umx.contact_degrees(ref.contacts(labels, N), N)
    assert degree.tolist() == [1, 1] and shared.tolist() == [12, 12]  # the inner object's whole outline (12 edges) is in contact


def test_neighbors_csv(tmp_path):
    labels, N = ref.mosaic(9, 65)
    rec = ref.contacts(labels, N)
    p = str(tmp_path / "n.csv")
    driver.write_neighbors_csv(p, rec)
    lines = open(p).read().splitlines()
    assert lines[0] == "label_a,label_b,shared_edges" == ",".join(driver.NEIGHBOR_COLUMNS) and len(lines) == len(rec) + 1 > 50
    assert [tuple(int(v) for v in line.split(",")) for line in lines[1:]] == ref.as_tuples(rec)
    driver.write_neighbors_csv(p, rec[:0])
    assert open(p).read() == "label_a,label_b,shared_edges\n"


def test_driver_refusals(tmp_path, monkeypatch, capsys):
    hp, blob, mean, std = helpers.load_nuclei_dapi()
    models = tmp_path / "models"
    model.save_converted(model.ModelArtefacts(hp, blob, mean, std), str(models / "nucleiDAPI"))
    monkeypatch.setenv("UMX_MODELS_DIR", str(models))

    def no_engine(*a, **k):
        raise AssertionError("the engine was set up before the label flags were checked")
    monkeypatch.setattr(umx, "Engine", no_engine)
    from unmicst_amd import tiffio
    os.makedirs(tmp_path / "x" / "registration")
    img = str(tmp_path / "x" / "registration" / "one.tif")
    tiffio.imsave(img, np.zeros((5, 7), np.uint16))
    for tool in driver.TOOLS:
        for flags, word in ((["--labelNeighbors"], "--labelNeighbors needs --labelMask"),
                            (["--labelNeighborsReach", "3"], "--labelNeighborsReach needs --labelMask"),
                            (["--labelMask", "--labelNeighborsReach", "3"], "--labelNeighborsReach needs --labelNeighbors"),
                            (["--labelMask", "--labelNeighbors", "--labelNeighborsReach", "256"], "0..255"),
                            (["--labelMask", "--labelNeighbors", "--labelNeighborsReach", "-1"], "0..255")):
            with pytest.raises(SystemExit) as e:
                driver.run(tool, [img, "--model", "nucleiDAPI"] + flags)
            assert e.value.code == 2
            assert word in capsys.readouterr().err, (tool, flags)


def test_host_arithmetic_under_the_sanitizers(tmp_path):
    """tools/contact_host_check.cpp -- the limits, the first table's size and the ordering of a scattered list, all of
    unmicst_amd/csrc/umx_contact_host.h -- built as a stand-alone program with ASan and UBSan on the host compiler, and run"""
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "contact_host_check")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        os.path.join(ROOT, "tools", "contact_host_check.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "contact-host-ok" in r.stdout, (r.stdout[-1000:], r.stderr[-2000:])
