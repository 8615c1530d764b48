"""The host model of the blob check (tests/kzg_blob_verify_model.py) on its own, without a GPU, against statements that do not share its
route: the barycentric eval_poly on a blob's evaluation form equals Horner's rule on the blob's coefficients, off the domain and ON it; it
reproduces blob_value at blob_challenge of tests/golden/eip4844_proofs_kat.json; and on a setup whose tau is known the constructed claim
holds while the same proof with one changed blob byte does not."""
import json
import random

import pytest

from tests import kzg_blob_verify_model as bm
from tests import kzg_model as km
from tests import kzg_open_model as om

TAU = 0x4844
R = km.R


def horner(coeffs, x):
    v = 0
    for a in reversed(coeffs):
        v = (v * x + a) % R
    return v


@pytest.fixture(scope="module")
def blob():
    return random.Random(20).randbytes(km.BLOB_BYTES)


@pytest.fixture(scope="module")
def evals(blob):
    return om.blob_evaluations(blob)


def test_eval_poly_equals_horner_on_the_coefficients_off_and_on_the_domain(blob, evals):
    coeffs, elements = om.blob_coefficients(blob), bm.elements_of(evals)
    points = [random.Random(21).randrange(R), 0] + [pow(om.OMEGA, om.brp12(i), R) for i in (0, 1, 255, 256, 4095)]
    assert points[2] == 1 and points[3] == R - 1
    for z in points:
        assert bm.eval_poly(elements, z) == horner(coeffs, z), z
    for k, i in enumerate((0, 1, 255, 256, 4095)):  # on the domain the value is the element itself
        assert bm.eval_poly(elements, points[2 + k]) == elements[i]


@pytest.mark.parametrize("case", [0, 1])
def test_eval_poly_reproduces_the_golden_blob_value_at_the_blob_challenge(case):
    kat = json.load(open(om.KAT_FILE))["cases"][case]
    blob, record = om.kat_blobs()[case]
    ev = om.blob_evaluations(blob)
    z = om.blob_challenge(ev, record["commitment"])
    assert z == int(kat["blob_challenge"], 16)
    assert bm.eval_poly(bm.elements_of(ev), z) == int(kat["blob_value"], 16)


def test_a_constructed_claim_holds_and_one_changed_blob_byte_breaks_it(evals):
    c, q = bm.true_claim_by_tau(evals, TAU)
    assert c == horner(om.blob_coefficients(random.Random(20).randbytes(km.BLOB_BYTES)), TAU)  # the commitment of the blob's polynomial
    verdict, z, y = bm.verify_proof_poly_by_tau(evals, c, q, TAU)
    assert verdict == 1 and y == bm.eval_poly(bm.elements_of(evals), z)
    assert bm.verify_proof_poly_by_tau(evals, c, (q + 1) % R, TAU)[0] == 0
    for at in (31, 32 * 4095 + 31):  # the last byte of an element: it stays below r
        changed = bytearray(evals)
        changed[at] ^= 1
        verdict, z2, _ = bm.verify_proof_poly_by_tau(bytes(changed), c, q, TAU)
        assert verdict == 0 and z2 != z
    # a blob that is nobody's evaluation form on purpose has its true claim too
    other = b"".join(random.Random(22).randrange(R).to_bytes(32, "big") for _ in range(4096))
    c2, q2 = bm.true_claim_by_tau(other, TAU)
    assert bm.verify_proof_poly_by_tau(other, c2, q2, TAU)[0] == 1 and bm.verify_proof_poly_by_tau(other, c, q, TAU)[0] == 0
