"""Host model of the two KZG proofs of an EIP-4844 blob (compute_proof, compute_proof_poly and compute_challenge, kzg/src/lib.rs:218-256,
285-288, 360-383 of the reference) in plain Python integers, on top of tests/kzg_model.py. It pins zkw_kzg_open and zkw_eip4844_prove
(tests/test_gpu_kzg_open.py); the model itself is pinned by tests/test_kzg_open_model.py against statements that do not share its route
and by tests/golden/eip4844_proofs_kat.json, which `python -m tests.kzg_open_model` writes.

A polynomial is a list of coefficients, LOWEST first (zkw_kzg_commit's order). The proof of p(z) = y is the commitment of
q(X) = (p(X) - y) / (X - z) (synthetic division: the intermediate values of Horner's walk). The blob's polynomial is the one the witness
commits to (element i = the coefficient of X^(4095 - i)); its evaluation form is element i = p(w^brp12(i))."""
import hashlib
import json
import os

from tests import kzg_model as km

_read = open  # (the builtin: this module's `open` is the KZG opening)
R = km.R
N = km.N_POINTS
OMEGA = 39033254847818212395286706435128746857159659164139250548781411570340225835782  # 7^((r - 1) / 4096) mod r (lib.rs:39-47)
DOMAIN = b"FSBLOBVERIFY_V1_"
KAT_FILE = os.path.join(km.GOLDEN, "eip4844_proofs_kat.json")
FIELDS = ("opening_proof", "blob_proof", "blob_challenge", "blob_value")


def brp12(i):
    return int(format(i, "012b")[::-1], 2)


def quotient(coeffs, z):
    """(q, y): p(X) - y = q(X) (X - z), q lowest first"""
    v, walk = 0, []
    for a in reversed(coeffs):
        v = (v * z + a) % R
        walk.append(v)
    return walk[-2::-1] if len(walk) > 1 else [], v


def open(coeffs, z, points=None):  # noqa: A001 (the issue's name for it)
    """(proof, y): the 48 compressed bytes of [q(tau)] G1 and y = p(z)"""
    assert 0 <= z < R
    q, y = quotient(coeffs, z)
    return km.commit(q, points), y


def _ntt(a, w):
    """[sum_k a[k] w^(j k) for j], len(a) a power of two, w a primitive len(a)-th root (decimation in time, recursive)"""
    n = len(a)
    if n == 1:
        return list(a)
    even, odd = _ntt(a[0::2], w * w % R), _ntt(a[1::2], w * w % R)
    out, t = [0] * n, 1
    for j in range(n // 2):
        o = odd[j] * t % R
        out[j], out[j + n // 2] = (even[j] + o) % R, (even[j] - o) % R
        t = t * w % R
    return out


def blob_coefficients(blob):
    return km.blob_elements(blob)[::-1]


def blob_evaluations(blob):
    """the sidecar's blob: 4 096 x 32 big-endian bytes, element i = p(w^brp12(i))"""
    natural = _ntt(blob_coefficients(blob), OMEGA)
    return b"".join(natural[brp12(i)].to_bytes(32, "big") for i in range(N))


def blob_challenge(evals, commitment):
    assert len(evals) == 32 * N and len(commitment) == 48
    return int.from_bytes(hashlib.sha256(DOMAIN + N.to_bytes(16, "big") + evals + commitment).digest(), "big") % R


def eip4844_prove(blob, record, points=None, proofs=True):
    """the four fields of zkw_eip4844_proof_record and the evaluation form, from a blob and its witness record (bytes by field name).
    proofs=False leaves the two commitments out (None): the caller has another way to them"""
    coeffs = blob_coefficients(blob)
    z = int.from_bytes(record["evaluation_point"], "big")
    q, y = quotient(coeffs, z)
    assert y.to_bytes(32, "big") == record["opening_value"]
    evals = blob_evaluations(blob)
    c = blob_challenge(evals, record["commitment"])
    qc, v = quotient(coeffs, c)
    return {"opening_proof": km.commit(q, points) if proofs else None, "blob_proof": km.commit(qc, points) if proofs else None,
            "blob_challenge": c.to_bytes(32, "big"), "blob_value": v.to_bytes(32, "big"), "blob_evaluations": evals}


def known_tau_setup(tau, n):
    """S[k] = [tau^k] G1 for a tau that is no secret, S[k + 1] = [tau] S[k] from the generator (the golden setup's first 48 bytes)"""
    pts = [km.decompress(km.load_setup_bytes()[:48], check_subgroup=False)]
    for _ in range(n - 1):
        pts.append(km.mul_naive(tau, pts[-1]))
    return pts


def proof_by_tau(coeffs, x, tau):
    """compress([(p(tau) - p(x)) / (tau - x)] G1): the proof on a known-tau setup WITHOUT synthetic division (tau != x)"""
    def ev(at):
        v = 0
        for a in reversed(coeffs):
            v = (v * at + a) % R
        return v
    k = (ev(tau) - ev(x)) * pow((tau - x) % R, R - 2, R) % R
    return km.compress(km.mul_naive(k, km.decompress(km.load_setup_bytes()[:48], check_subgroup=False)))


def kat_blobs():
    """the two blobs of tests/golden/eip4844_kat.json with their witness records"""
    kat = json.load(_read(os.path.join(km.GOLDEN, "eip4844_kat.json")))["cases"]
    return [(blob, {f: bytes.fromhex(v) for f, v in case.items() if f != "blob"}) for blob, case in zip((bytes(km.BLOB_BYTES), km.pattern_blob()), kat)]


def kat_case(blob, record):
    got = eip4844_prove(blob, record)
    out = {f: got[f].hex() for f in FIELDS}
    out["blob_evaluations_sha256"] = hashlib.sha256(got["blob_evaluations"]).hexdigest()
    return out


if __name__ == "__main__":
    names = ("zero", "pattern: byte[j] = (167 j + 13) & 0xff")
    doc = {"source": "pure-Python model tests/kzg_open_model.py (python -m tests.kzg_open_model) on tests/golden/kzg_trusted_setup_g1.bin, for the blobs and "
                     "records of eip4844_kat.json; blob_evaluations_sha256 is the SHA-256 of the 131 072 bytes of the evaluation form",
           "cases": [dict(blob=name, **kat_case(blob, rec)) for name, (blob, rec) in zip(names, kat_blobs())]}
    with _read(KAT_FILE, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc, indent=1))
