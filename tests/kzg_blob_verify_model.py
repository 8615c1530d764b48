"""Host model of the blob check a consumer of a sidecar runs (verify_proof_poly with eval_poly, kzg/src/lib.rs:292-301, 327-358 of the
reference) in plain Python integers, on top of tests/kzg_open_model.py. It pins zkw_kzg_evaluate_blobs and zkw_eip4844_verify_blobs
(tests/test_gpu_kzg_blob_verify.py); the model itself is pinned by tests/test_kzg_blob_verify_model.py against Horner's rule on the
blob's coefficients and against tests/golden/eip4844_proofs_kat.json.

A blob in evaluation form is 4 096 x 32 big-endian bytes, element i = p(w^brp12(i)) (om.blob_evaluations). The barycentric formula
    y = (z^4096 - 1) / 4096 * sum_i f_i w_i / (z - w_i)            (y = f_i if z = w_i)
is walked the way lib.rs:327-358 walks it: one modular inverse per element, nothing batched. (On the domain the reference goes on to
multiply f_i by z^4096 - 1 = 0; the value of the polynomial there is f_i, and that is what this library returns.)"""
from tests import kzg_model as km
from tests import kzg_open_model as om

R = km.R
N = km.N_POINTS


def elements_of(evals):
    assert len(evals) == 32 * N
    return [int.from_bytes(evals[32 * i:32 * i + 32], "big") for i in range(N)]


_ROOTS = None


def roots_brp():
    """roots_of_unity_brp: w^brp12(i)"""
    global _ROOTS
    if _ROOTS is None:
        _ROOTS = [pow(om.OMEGA, om.brp12(i), R) for i in range(N)]
    return _ROOTS


def eval_poly(elements, z):
    """p(z) for the polynomial whose evaluation form is `elements` (4 096 integers below r)"""
    assert len(elements) == N and 0 <= z < R and all(0 <= f < R for f in elements)
    roots = roots_brp()
    inverse_width = pow(N, -1, R)
    if z in roots:
        return elements[roots.index(z)]
    res = 0
    for el, root in zip(elements, roots):
        el = el * root % R
        z_1 = (z - root) % R
        el = el * pow(z_1, -1, R) % R
        res = (res + el) % R
    z_1 = (pow(z, N, R) - 1) % R
    res = res * z_1 % R
    return res * inverse_width % R


def g1_of(k):
    """compress([k] G1)"""
    return km.compress(km.mul_naive(k % R, km.decompress(km.load_setup_bytes()[:48], check_subgroup=False)))


def verify_proof_poly_by_tau(evals, c, q, tau):
    """(verdict, z, y) for the blob `evals` (131 072 bytes), the commitment [c] G1 and the proof [q] G1 on a setup whose tau is known:
    z = compute_challenge(blob, commitment), y = eval_poly(blob, z), and e(C - [y] G1, G2) = e(proof, [tau - z] G2) says
    c - y = q (tau - z) mod r"""
    z = om.blob_challenge(evals, g1_of(c))
    y = eval_poly(elements_of(evals), z)
    return int((c - y) % R == q * (tau - z) % R), z, y


def true_claim_by_tau(evals, tau):
    """(c, q) of the one true claim about ANY evaluation-form blob, without multi-scalar work: c = p(tau), q = (c - y) / (tau - z)"""
    c = eval_poly(elements_of(evals), tau)
    z = om.blob_challenge(evals, g1_of(c))
    y = eval_poly(elements_of(evals), z)
    return c, (c - y) * pow((tau - z) % R, -1, R) % R
