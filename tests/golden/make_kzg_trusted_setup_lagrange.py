#!/usr/bin/env python3
"""Regenerates kzg_trusted_setup_g1_lagrange.bin from kzg_trusted_setup_g1.bin (`python tests/golden/make_kzg_trusted_setup_lagrange.py`,
about 75 s; a script, not a test).

The ceremony's setup in the Lagrange basis, in the order the reference keeps it (`lagrange_setup_brp` of KzgSettings::new,
kzg/src/lib.rs:91-141): entry i = L[brp12(i)], L[u] = [l_u(tau)] G1 = (1 / 4096) sum_k w^(-u k) S[k], w = 7^((r - 1) / 4096), 48 compressed
bytes each. Computed by a plain radix-2 inverse transform (decimation in frequency, which leaves the bit-reversed order by itself) over
the arithmetic of tests/kzg_model.py, one double-and-add product per butterfly. Entry 0 is the first `g1_lagrange` point of the public
setup file (c-kzg's trusted_setup.txt). Data only."""
import hashlib
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import kzg_model as km  # noqa: E402

SHA256 = "000be46bb434946e041c7bc9757175591eb07bcdaff641ea6eca2552618dc39d"
OUT = os.path.join(HERE, "kzg_trusted_setup_g1_lagrange.bin")


def jmul(k, p):
    acc = km.J_INF
    for bit in bin(k)[2:] if k else "":
        acc = km.jdbl(acc)
        if bit == "1":
            acc = km.jadd(acc, p)
    return acc


def lagrange_brp(points):
    """[L[brp(i)] for i], L the inverse transform of `points` (affine, a power of two of them), affine"""
    n = len(points)
    w_inv = pow(pow(7, (km.R - 1) // n, km.R), -1, km.R)
    x = [km.to_jac(p) for p in points]
    half = n // 2
    while half:
        step = pow(w_inv, n // (2 * half), km.R)
        for start in range(0, n, 2 * half):
            tw = 1
            for j in range(half):
                u, v = x[start + j], x[start + j + half]
                x[start + j] = km.jadd(u, v)
                d = km.jadd(u, (v[0], (km.P - v[1]) % km.P, v[2]))
                x[start + j + half] = d if tw == 1 else jmul(tw, d)
                tw = tw * step % km.R
        half //= 2
    n_inv = pow(n, -1, km.R)
    return [km.to_affine(jmul(n_inv, p)) for p in x]


if __name__ == "__main__":
    raw = b"".join(km.compress(p) for p in lagrange_brp(km.load_setup()))
    digest = hashlib.sha256(raw).hexdigest()
    assert len(raw) == 4096 * 48 and digest == SHA256, digest
    open(OUT, "wb").write(raw)
    print("ok", len(raw))
