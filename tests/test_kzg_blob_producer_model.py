"""The host model of the producers from the evaluation form (tests/kzg_blob_producer_model.py) on its own, without a GPU, against statements
that do not share its route: the inverse transform undoes om.blob_evaluations (a recursive forward transform) for the two golden blobs;
for a blob that is nobody's pubdata, Horner's rule on its coefficients equals the barycentric eval_poly on its elements, off the domain and
ON it; the direct sum agrees with the full transform; and the compositions reproduce tests/golden/eip4844_proofs_kat.json."""
import json
import random

import pytest

from tests import kzg_blob_producer_model as pr
from tests import kzg_blob_verify_model as bm
from tests import kzg_model as km
from tests import kzg_open_model as om

R = km.R


def horner(coeffs, x):
    v = 0
    for a in reversed(coeffs):
        v = (v * x + a) % R
    return v


@pytest.fixture(scope="module")
def golden():
    """[(blob, record, evaluation form)] of the two blobs of eip4844_kat.json"""
    return [(blob, rec, om.blob_evaluations(blob)) for blob, rec in om.kat_blobs()]


@pytest.mark.parametrize("case", [0, 1])
def test_coefficients_undo_blob_evaluations(golden, case):
    blob, _, ev = golden[case]
    assert pr.coefficients(bm.elements_of(ev)) == om.blob_coefficients(blob)
    assert pr.coefficient_rows(ev) == b"".join(e.to_bytes(32, "little") for e in km.blob_elements(blob)[::-1])


def test_horner_on_the_coefficients_equals_eval_poly_on_a_full_range_blob():
    rng = random.Random(2901)
    elements = [rng.randrange(R) for _ in range(4096)]
    assert max(elements) >> 248  # not a blob of 31-byte elements
    coeffs = pr.coefficients(elements)
    for z in (rng.randrange(R), 0, pow(om.OMEGA, om.brp12(255), R)):
        assert horner(coeffs, z) == bm.eval_poly(elements, z), z
    assert horner(coeffs, pow(om.OMEGA, om.brp12(255), R)) == elements[255]
    for k in (0, 1, 2047, 4095):  # the sum as it stands
        assert pr.coefficient(elements, k) == coeffs[k], k
    evals = b"".join(f.to_bytes(32, "big") for f in elements)
    z = rng.randrange(R)
    assert pr.open_blobs(evals, z, proof=False)[1] == bm.eval_poly(elements, z)


@pytest.mark.parametrize("case", [0, 1])
def test_the_compositions_reproduce_the_golden_proofs(golden, case):
    kat = json.load(open(om.KAT_FILE))["cases"][case]
    _, rec, ev = golden[case]
    assert pr.commit_blobs(ev) == rec["commitment"]
    proof, y = pr.open_blobs(ev, int.from_bytes(rec["evaluation_point"], "big"))
    assert proof.hex() == kat["opening_proof"] and y.to_bytes(32, "big") == rec["opening_value"]
    proof, z, y = pr.prove_blobs(ev, rec["commitment"])
    assert proof.hex() == kat["blob_proof"] and z == int(kat["blob_challenge"], 16) and y == int(kat["blob_value"], 16)
