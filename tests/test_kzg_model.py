"""The host model of the EIP-4844 blob witness (tests/kzg_model.py) checked on its own, without a GPU: it reproduces the known answers of
tests/golden/eip4844_kat.json (the zero blob's versioned hash is the publicly known one of the empty blob's commitment), reads the
trusted-setup fixture as the monomial powers of tau, and its bucket multi-scalar multiplication equals naive double-and-add."""
import hashlib
import json
import os
import random

import pytest

from tests import kzg_model as km

G = (0x17F1D3A73197D7942695638C4FA9AC0FC3688C4F9774B905A14E3A3F171BAC586C55E83FF97A1AEFFB3AF00ADB22C6BB,
     0x08B3F481E3AAA0F1A09E30ED741D8AE4FCF5E095D5D00AF600DB18CB2C04B3EDD03CC744A2888AE40CAA232946C5E7E1)


def test_fixture_is_the_ceremony_output():
    raw = km.load_setup_bytes()
    assert len(raw) == 196608
    assert hashlib.sha256(raw).hexdigest() == "08797579f6cfd5788eddc1a215d64dcfabd04acbcaf2953fb2c1afb830f43315"
    assert raw[:48].hex().startswith("97f1d3a7") and raw[:48].hex().endswith("c6bb")


def test_first_setup_point_is_the_generator_and_lies_in_the_subgroup():
    assert km.decompress(km.load_setup_bytes()[:48]) == G
    assert (G[1] ** 2 - G[0] ** 3 - km.B) % km.P == 0
    assert km.compress(G) == km.load_setup_bytes()[:48] and km.compress(km.INF) == bytes([0xC0]) + bytes(47)


@pytest.mark.parametrize("case", [0, 1])
def test_model_reproduces_the_known_answers(case):
    kat = json.load(open(os.path.join(km.GOLDEN, "eip4844_kat.json")))["cases"][case]
    blob = bytes(km.BLOB_BYTES) if case == 0 else km.pattern_blob()
    got = km.eip4844_witness(blob)
    for field, value in got.items():
        assert value.hex() == kat[field], field


def test_unit_coefficient_commits_to_its_setup_point():
    raw = km.load_setup_bytes()
    assert km.commit([0, 1, 0, 0]) == raw[48:96]


def test_bucket_method_equals_double_and_add():
    rng = random.Random(5)
    scalars = [rng.randrange(1 << 247, 1 << 248) for _ in range(5)]
    points = km.load_setup()[:5]
    assert km.msm(scalars, points) == km.msm_naive(scalars, points)
    assert km.msm([0, 0], points[:2]) is km.INF
    assert km.msm([km.R - 1], points[:1]) == km.neg(points[0])
