"""Host model of the verification of EIP-7594 cell proofs in plain Python integers, on top of tests/kzg_cells_model.py and
tests/kzg_pairing_model.py. It pins zkw_kzg_verify_cells and zkw_kzg_commit_cells (tests/test_gpu_kzg_cell_verify.py); the model itself is
pinned by tests/test_kzg_cell_verify_model.py.

Cell k holds p at the 64 roots of X^64 - c_k, c_k = w128^brp7(k), in the order h_k w64^brp6(t), h_k = W^brp7(k), w64 = W^128. I_k is the
polynomial of degree below 64 through them: p = q_k (X^64 - c_k) + I_k, and with pi = [q_k(tau)] G1 the claim (C, k, cell, pi) holds when
    e(C - [I_k(tau)] G1 + [c_k] pi, -G2) e(pi, [tau^64] G2) = 1.
`interpolant` goes the kernels' way (an inverse transform of the cell over w64, then the coset's shift undone); `interpolant_by_remainder`
reduces the blob's polynomial modulo X^64 - c_k and shares nothing with it. A polynomial is a list of coefficients, LOWEST first."""
from tests import kzg_cells_model as cm
from tests import kzg_model as km
from tests import kzg_open_model as om
from tests import kzg_pairing_model as pm

R = km.R
CELL = cm.CELL
W64 = pow(cm.W, 128, R)


def cell_shift(k):
    """h_k: the cell's points are h_k times the 64th roots of unity"""
    return pow(cm.W, cm.brp(k, 7), R)


def cell_elements(cell):
    assert len(cell) == 32 * CELL
    return [int.from_bytes(cell[32 * t:32 * t + 32], "big") for t in range(CELL)]


def interpolant(k, cell):
    """I_k from the 2 048 bytes of cell k: v[brp6(t)] = element t is the transform over w64 of b_i = I_k[i] h_k^i"""
    e = cell_elements(cell)
    assert all(x < R for x in e)
    v = [e[cm.brp(m, 6)] for m in range(CELL)]
    inv = pow(CELL, -1, R)
    b = [x * inv % R for x in om._ntt(v, pow(W64, -1, R))]
    back = pow(cell_shift(k), -1, R)
    return [x * pow(back, i, R) % R for i, x in enumerate(b)]


def interpolant_by_remainder(coeffs, k):
    """p mod (X^64 - c_k): I_k[i] = sum_j c_k^j p[i + 64 j]"""
    c = cm.cell_constant(k)
    out = [0] * CELL
    for i in range(CELL):
        acc = 0
        for j in range(len(coeffs) // CELL - 1, -1, -1):
            acc = (acc * c + coeffs[i + CELL * j]) % R
        out[i] = acc
    return out


def g1_of(scalar):
    """[scalar] G1, affine (None: infinity)"""
    return km.mul_naive(scalar % R, pm.g1_gen())


def tau64_g2(tau):
    """[tau^64] G2 of a setup whose tau is known, as a point and as the 96 bytes a verifier is created from"""
    q = pm.g2_mul(pow(tau, 64, R), pm.G2_GEN)
    return q, pm.g2_compress(q)


def interpolant_commitment(k, cell, points=None, tau=None):
    """[I_k(tau)] G1, affine: over the setup's first 64 points (`points`; None: the golden setup), or, when the setup's tau is known,
    by one multiplication of the generator"""
    coeffs = interpolant(k, cell)
    if tau is not None:
        return g1_of(cm.evaluate(coeffs, tau))
    points = km.load_setup() if points is None else points
    return km.msm(coeffs, points[:CELL])


def verify_cell(commitment, k, cell, proof, tau64_g2, points=None, tau=None):
    """the pairing check of one claim on decompressed points (None: infinity); `points` and `tau` as for interpolant_commitment"""
    i_k = interpolant_commitment(k, cell, points, tau)
    p1 = km.add(km.add(commitment, km.neg(i_k)), km.mul_naive(cm.cell_constant(k), proof))
    return pm.pairing_product_is_one([(p1, pm.g2_neg(pm.G2_GEN)), (proof, tau64_g2)])
