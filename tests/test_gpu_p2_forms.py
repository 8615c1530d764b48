"""The Poseidon2 forms of csrc/poseidon2.cuh piece by piece: tests/csrc_gpu/p2_forms_test.hip compares wp_reduce, the three round-constant
additions, one external and one internal layer of the lane form, Coop, Coop2 and Coop4, Coop::pow7_pair, and the whole permutations
p2::permute, permute_lat, Coop::permute, Coop2::permute and coop_flattened (all 130 stored values) with the definition written in the
program (`unsigned __int128 % p`, the layers as matrices from include/zkw_poseidon2_params.h), and the host forms with the same. A host
word model of the device steps counts the inputs that take each wrap; the conditions asserted here are conditions on those inputs. The
CPU test runs --host-only (inputs, coverage, host forms, no HIP call); the two GPU tests run the modes "layers" and "perms"."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
LAYER_STATES = 16 + 16 * 12 * 2 + (1 << 12)  # uniform edge states, one edge word in one position (rest 0 / all ones), seeded states
ROUND_CONSTANTS = 30 * 12


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("p2_forms") / "p2_forms_test")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "csrc_gpu", "p2_forms_test.hip"), "-o", out])
    return out


def _run(exe, mode):
    r = subprocess.run([exe, mode], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    last = lines[-1].split()
    assert last[0] == "ok" and last[2] == mode.lstrip("-"), r.stdout[-2000:]
    cover = {}
    for line in lines:
        w = line.split()
        if w[0] == "cover":
            cover[w[1]] = {k: int(v, 0) for k, v in (kv.split("=") for kv in w[2:])}
    return int(last[1]), cover


def _assert_layer_coverage(c):
    wp = c["wp_reduce"]
    assert wp["n"] >= 1 << 14
    assert wp["cc"] == 0b0111  # (c, c2) = (0,0), (1,0), (0,1); (1,1) cannot occur for L, H < 2^63
    assert wp["lt47"] >= 1 << 12 and wp["cc47"] == 0b0111  # the callers' range
    rc = c["add_rc"]
    assert rc["consts"] == ROUND_CONSTANTS + 2 and rc["n"] >= 256 * rc["consts"] and rc["w"] == 0b11
    ly = c["layers"]
    assert ly["n"] == LAYER_STATES
    assert ly["row_ext_wrap"] >= 1 and ly["row_int_wrap"] >= 1  # the final v_cndmask wrap of Coop::external / Coop::internal
    assert ly["lane_ext_c2"] >= 1 and ly["lane_int_c2"] >= 1    # wp_reduce's second wrap inside the lane form's layers
    assert c["pow7_pair"]["n"] >= 1 << 12


def test_p2_forms_inputs_cover_every_wrap(exe):
    _, c = _run(exe, "--host-only")
    _assert_layer_coverage(c)
    assert c["perms"]["n"] == 1 << 14


@pytest.mark.gpu
def test_p2_layers_and_pieces_equal_the_definition(exe):
    total, c = _run(exe, "layers")
    _assert_layer_coverage(c)
    states = -(-LAYER_STATES // 256) * 256  # padded to whole blocks
    # wp_reduce pairs, three additions per (x, constant), eight layers (the row form's with its four idle lanes), pow7_pair
    assert total == c["wp_reduce"]["n"] + 3 * c["add_rc"]["n"] + states * (6 * 12 + 2 * 16) + c["pow7_pair"]["n"]


@pytest.mark.gpu
def test_p2_permutation_forms_equal_the_plain_reference(exe):
    total, c = _run(exe, "perms")
    n = c["perms"]["n"]
    assert n == 1 << 14
    # lane form, permute_lat, Coop2: 12 words; Coop: 16 lanes; coop_flattened: 130 slots + 12 results
    assert total == n * (3 * 12 + 16 + 142)
