"""Host model of the EIP-7594 cells and cell proofs of a blob in plain Python integers, on top of tests/kzg_model.py and
tests/kzg_open_model.py. It pins zkw_kzg_cells_blobs, zkw_kzg_cell_proofs_blobs and zkw_eip4844_cell_proofs (tests/test_gpu_kzg_cells.py);
the model itself is pinned by tests/test_kzg_cells_model.py against statements that do not share its route.

A polynomial is a list of 4 096 coefficients, LOWEST first. W = 7^((r - 1) / 8192), W^2 = OMEGA. Extended evaluation e[j] = p(W^brp13(j)),
j < 8192; cell k = e[64 k .. 64 k + 63], whose points are the 64 roots of X^64 - c_k, c_k = w128^brp7(k), w128 = OMEGA^32. The proof of
cell k is [q_k(tau)] G1 for q_k = p div (X^64 - c_k); nothing here runs FK20 — `fk20_scalars` restates it over the scalars of a known-tau
setup only so that the index arithmetic of the device's route can be checked on the host."""
from tests import kzg_model as km
from tests import kzg_open_model as om

R = km.R
N = 4096
CELLS = 128
CELL = 64
OMEGA = om.OMEGA
W = pow(7, (R - 1) // 8192, R)
W128 = pow(OMEGA, 32, R)


def brp(i, bits):
    return int(format(i, "0%db" % bits)[::-1], 2) if bits else 0


def cell_constant(k):
    return pow(W128, brp(k, 7), R)


def cell_points(k):
    """the 64 points of cell k, in the cell's order"""
    return [pow(W, brp(CELL * k + t, 13), R) for t in range(CELL)]


def extended_evaluations(coeffs):
    """e[j] = p(W^brp13(j)): the blob's own evaluation form, then the transform of the coefficients scaled by W^i"""
    assert len(coeffs) == N
    lower = om._ntt(list(coeffs), OMEGA)
    upper = om._ntt([c * pow(W, i, R) % R for i, c in enumerate(coeffs)], OMEGA)
    return [lower[om.brp12(i)] for i in range(N)] + [upper[om.brp12(i)] for i in range(N)]


def cells(coeffs):
    """the 128 cells, 2 048 bytes each"""
    e = extended_evaluations(coeffs)
    return [b"".join(v.to_bytes(32, "big") for v in e[CELL * k:CELL * k + CELL]) for k in range(CELLS)]


def quotient_by_cell(coeffs, k):
    """q_k lowest first (4 032 coefficients): p = q_k (X^64 - c_k) + remainder, by synthetic division from the top down"""
    c = cell_constant(k)
    q = [0] * (N - CELL)
    for i in range(N - CELL - 1, -1, -1):
        q[i] = (coeffs[i + CELL] + (c * q[i + CELL] if i + CELL < N - CELL else 0)) % R
    return q


def quotients(coeffs):
    return [quotient_by_cell(coeffs, k) for k in range(CELLS)]


def evaluate(coeffs, x):
    v = 0
    for a in reversed(coeffs):
        v = (v * x + a) % R
    return v


def cell_proof_by_tau(coeffs, k, tau):
    """compress([q_k(tau)] G1) on a known-tau setup: q_k(tau) in Fr, one multiplication of the generator, no commitment"""
    g = km.decompress(km.load_setup_bytes()[:48], check_subgroup=False)
    return km.compress(km.mul_naive(evaluate(quotient_by_cell(coeffs, k), tau), g))


def fk20_scalars(coeffs, tau):
    """[q_k(tau) for k] by the device's route with every group element replaced by its scalar (S[k] = tau^k): the Toeplitz vectors, the
    circular products in the transformed domain, the dropped upper half, the last transform and the bit reversal"""
    s = [pow(tau, k, R) for k in range(N)]
    inv = pow(128, -1, R)
    hh = [0] * 128
    for i in range(CELL):
        x = [s[N - CELL - 1 - i - CELL * m] for m in range(63)] + [0] * 65
        t = [coeffs[N - 1 - i]] + [0] * 65 + [coeffs[127 - i + CELL * m] for m in range(62)]
        xf, cf = om._ntt(x, W128), om._ntt(t, W128)
        hh = [(a + c * b) % R for a, b, c in zip(hh, xf, cf)]
    h = [v * inv % R for v in om._ntt(hh, pow(W128, -1, R))]
    p = om._ntt(h[:64] + [0] * 64, W128)
    return [p[brp(k, 7)] for k in range(CELLS)]
