"""Host model of the KZG producers that start from a blob in EVALUATION form (compute_commitment, compute_proof and compute_proof_poly,
kzg/src/lib.rs:188-191, 218-256, 285-288 of the reference, as its own two tests call them) in plain Python integers, on top of
tests/kzg_model.py and tests/kzg_open_model.py. It pins zkw_kzg_blob_coefficients, zkw_kzg_commit_blobs, zkw_kzg_open_blobs and
zkw_eip4844_prove_blobs (tests/test_gpu_kzg_blob_producers.py); the model itself is pinned by tests/test_kzg_blob_producer_model.py.

A blob in evaluation form is 4 096 x 32 big-endian bytes, element i = f_i = p(w^brp12(i)). The way back to the monomial form the setup is
kept in is the inverse transform
    a_k = 4096^-1 sum_i f_i w^(-brp12(i) k)
written here twice, neither time through om._ntt: `coefficient` is that sum as it stands, for one k; `coefficients` is the whole transform,
iterative, decimation in time on the blob's own order (which IS the bit-reversed order such a transform starts from) with powers of
w^-1. The producers are compositions: the commitment of the coefficients, the quotient of Horner's walk on them, the reference's challenge."""
from tests import kzg_blob_verify_model as bm
from tests import kzg_model as km
from tests import kzg_open_model as om

R = km.R
N = km.N_POINTS
OMEGA_INV = pow(om.OMEGA, R - 2, R)
N_INV = pow(N, R - 2, R)


def coefficient(elements, k):
    """a_k by the direct sum over the 4 096 elements"""
    assert len(elements) == N
    return N_INV * sum(f * pow(OMEGA_INV, om.brp12(i) * k % N, R) for i, f in enumerate(elements) if f) % R


def coefficients(elements):
    """[a_0 .. a_4095], lowest first (zkw_kzg_commit's order), of the polynomial whose evaluation form is `elements`"""
    assert len(elements) == N and all(0 <= f < R for f in elements)
    a = list(elements)
    width = 2
    while width <= N:
        step = pow(OMEGA_INV, N // width, R)  # a primitive width-th root of unity, inverted
        for start in range(0, N, width):
            t = 1
            for j in range(width // 2):
                u, v = a[start + j], a[start + j + width // 2] * t % R
                a[start + j], a[start + j + width // 2] = (u + v) % R, (u - v) % R
                t = t * step % R
        width *= 2
    return [x * N_INV % R for x in a]


def coefficient_rows(evals):
    """what zkw_kzg_blob_coefficients writes for one blob: 4 096 rows of 32 little-endian bytes"""
    return b"".join(c.to_bytes(32, "little") for c in coefficients(bm.elements_of(evals)))


def commit_blobs(evals, points=None):
    """compute_commitment: the 48 compressed bytes"""
    return km.commit(coefficients(bm.elements_of(evals)), points)


def open_blobs(evals, z, points=None, proof=True):
    """compute_proof: (proof, y) at the point z, on the domain or off it; proof=False leaves the commitment of the quotient out (None)"""
    assert 0 <= z < R
    q, y = om.quotient(coefficients(bm.elements_of(evals)), z)
    return (km.commit(q, points) if proof else None), y


def prove_blobs(evals, commitment, points=None, proof=True):
    """compute_proof_poly: (proof, z, y) with z = compute_challenge(blob, commitment); the commitment's bytes are hashed as they are"""
    z = om.blob_challenge(evals, commitment)
    q, y = open_blobs(evals, z, points, proof)
    return q, z, y
