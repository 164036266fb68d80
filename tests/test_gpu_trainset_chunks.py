"""GPU test of the chunking of a batch's assembly (unmicst_amd/csrc/umx_trainset.hip: enqueue_assemble, enqueue_batch): a launch
carries at most 64 plain descriptors, 16 blurred or warped images or 8 elastic images, and a batch of 72 images of all four kinds,
interleaved, makes every one of them flush a full chunk and go on into the next.  Every entry is bit-equal to its restatement
(tests/trainset_*_ref.py) on that batch, and a step on it is the host-fed step on the restated arrays."""
import numpy as np
import pytest

import helpers
import trainset_augment_ref as aref
import trainset_elastic_ref as eref
import trainset_ref as ref
import trainset_warp_ref as wref
from trainset_cases import MEAN, STD, _augs, _descs, _elastics, _random_set, _same_bits, _warps
from unmicst_amd import model, trainer, trainset

pytestmark = pytest.mark.gpu

HP = helpers.small_hps()["v2_duo_like"]                  # P = 32, C = 2, K = 3
LW3 = trainset.LabelWeights(True, (1.0, 2.0, 7.0), (0.0, 15.0, 0.25))
GAINS = (1.0, 1.5, 4.0)
IDENTITY = (1.0, 0.0, 0.0, 1.0)
B, N, PAGES, S = 72, 3, 2, 49
DESC_CHUNK, AUG_CHUNK, ELASTIC_CHUNK = 64, 16, 8         # kDescChunk, kAugChunk, kElasticChunk of umx_internal.h


def _rows():
    """Row i has kind i % 4: 0 plain, 1 blur / gain only, 2 warped, 3 elastic."""
    span = S - HP.imSize + 1
    rng = np.random.default_rng(72)
    rows, augs, warps, lats = [], [], [], []
    for i in range(B):
        kind = i % 4
        rows.append((i % N, i % PAGES, (5 * i) % span, (11 * i) % span, i % 8, 0.1, 1.02))
        augs.append(((i // 4) % 4, GAINS[i % 3]) if kind else (0, 1.0))
        warps.append(trainset.warp_matrix(30 + i, 1.25) if kind >= 2 and i % 8 != 3 else IDENTITY)
        n = 4 + i % 3
        lats.append((n, trainset.elastic_lattice(rng.standard_normal(2 * n * n), 2.5, n)) if kind == 3 else None)
    return rows, augs, warps, lats


def _kinds(augs, warps, lats):
    """How many images enqueue_batch sends to the (blur / gain only, warped, elastic) chunks, and how many it never touches again;
    augs / warps / lats None: the entry without that array."""
    blur = warped = elastic = plain = 0
    for i in range(B):
        if lats is not None and lats[i] is not None:
            elastic += 1
        elif warps is not None and not wref.is_identity(warps[i]):
            warped += 1
        elif augs is not None and tuple(augs[i]) != (0, 1.0):
            blur += 1
        else:
            plain += 1
    return blur, warped, elastic, plain


@pytest.fixture(scope="module")
def rig():
    planes, ann, wmaps = _random_set(HP, N, PAGES, S, 13)
    assert wmaps[1] is None and all(w is not None for w in (wmaps[0], wmaps[2]))
    table = trainset.AugmentTable.from_sigmas((0.75, 1.5, 4.0), MEAN, STD)
    blob, opts = model.random_blob(HP, seed=5), trainer.duo_options()
    a, b = trainer.Trainer(HP, blob, opts, batch=B), trainer.Trainer(HP, blob, opts, batch=B)
    ts = trainset.TrainSet.from_arrays(a, planes, ann, wmaps, LW3)
    ts.set_augment(table)
    rows, augs, warps, lats = _rows()
    yield dict(a=a, b=b, ts=ts, set=(planes, ann, wmaps), table=table, d=_descs(rows), g=_augs(augs), w=_warps(warps), e=_elastics(lats))
    a.close()
    b.close()


def test_the_batch_crosses_every_chunk_limit():
    _, augs, warps, lats = _rows()
    blur, warped, elastic, plain = _kinds(augs, warps, lats)
    assert (blur, warped, elastic, plain) == (17, 18, 18, 19)
    assert blur > AUG_CHUNK and warped > AUG_CHUNK and elastic > 2 * ELASTIC_CHUNK and B > DESC_CHUNK and plain >= 1
    # the entries with fewer arrays: the images whose array is missing fall to the chunk before
    assert _kinds(augs, warps, None)[1] > AUG_CHUNK and _kinds(augs, None, None)[0] > 3 * AUG_CHUNK
    kinds = [i % 4 for i in range(B)]
    assert kinds[:8] == [0, 1, 2, 3, 0, 1, 2, 3]                          # interleaved: every chunk fills while the others are part full


def _weights():
    return LW3.class_weight, LW3.intersect_weight


@pytest.mark.parametrize("n", [B, B - 2], ids=["all_rows", "n_lt_B"])
def test_assemble_elastic_across_chunks(rig, n):
    planes, ann, wmaps = rig["set"]
    d, g, w, e = (rig[k][:n] for k in "dgwe")
    got = rig["a"].assemble_elastic(rig["ts"], d, g, w, e)
    assert got[0].shape == (n, HP.imSize, HP.imSize, HP.nChannels)
    want = eref.assemble_elastic(planes, ann, wmaps, d, g, w, e, rig["table"], HP.imSize, HP.nClasses, *_weights())
    _same_bits(got, want, ("assemble_elastic", n))


@pytest.mark.parametrize("n", [B, B - 2], ids=["all_rows", "n_lt_B"])
def test_assemble_warped_across_chunks(rig, n):
    planes, ann, wmaps = rig["set"]
    d, g, w = (rig[k][:n] for k in "dgw")
    got = rig["a"].assemble_warped(rig["ts"], d, g, w)
    want = wref.assemble_warped(planes, ann, wmaps, d, g, w, rig["table"], HP.imSize, HP.nClasses, *_weights())
    _same_bits(got, want, ("assemble_warped", n))


def test_assemble_augmented_across_chunks(rig):
    planes, ann, wmaps = rig["set"]
    got = rig["a"].assemble_augmented(rig["ts"], rig["d"], rig["g"])
    want = aref.assemble_augmented(planes, ann, wmaps, rig["d"], rig["g"], rig["table"], HP.imSize, HP.nClasses, *_weights())
    _same_bits(got, want, "assemble_augmented")


def test_assemble_plain_second_chunk(rig):
    planes, ann, wmaps = rig["set"]
    got = rig["a"].assemble(rig["ts"], rig["d"])
    want = ref.assemble(planes, ann, wmaps, rig["d"], HP.imSize, HP.nClasses, *_weights())
    _same_bits(got, want, "assemble")


def test_step_elastic_across_chunks_is_the_host_fed_step(rig):
    planes, ann, wmaps = rig["set"]
    a, b = rig["a"], rig["b"]
    d, g, w, e = (rig[k] for k in "dgwe")
    a.step_elastic(rig["ts"], d, g, w, e)
    la = a.loss()
    data, labels, weights = eref.assemble_elastic(planes, ann, wmaps, d, g, w, e, rig["table"], HP.imSize, HP.nClasses, *_weights())
    lb = b.step(data, labels, weights)
    assert la == lb
    assert a.grads().tobytes() == b.grads().tobytes()
    assert a.blob().tobytes() == b.blob().tobytes()
    assert a.step_count == b.step_count == 1
