"""Host model of the EIP-4844 blob witness (generate_eip4844_witness, src/utils.rs:119-231 of the reference; kzg/src/lib.rs) in plain
Python integers: BLS12-381 G1 decompression / compression, Jacobian arithmetic, a bucket MSM and the witness function. It pins
zkw_kzg_commit and zkw_eip4844_witness (tests/test_gpu_kzg.py) the way storage_witness_model.py pins the witness trees; the model itself
is pinned by tests/test_kzg_model.py against tests/golden/eip4844_kat.json.

A blob is 4 096 x 31 bytes; element i is the little-endian integer of its i-th 31 bytes; p(X) = sum_i e_i X^(4095 - i); the commitment is
sum_i e_i S[4095 - i] over the monomial setup S[k] = [tau^k] G1 (tests/golden/kzg_trusted_setup_g1.bin)."""
import hashlib
import os

from era_zkevm_test_harness_amd.secp256k1 import keccak256

P = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
B = 4
N_POINTS = 4096
BLOB_BYTES = N_POINTS * 31
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SETUP_FILE = os.path.join(GOLDEN, "kzg_trusted_setup_g1.bin")
INF = None  # the point at infinity (affine form); Jacobian: Z == 0


class BadPoint(ValueError):
    pass


def sqrt_fq(a):
    """a root of a (p = 3 mod 4), or None"""
    y = pow(a, (P + 1) // 4, P)
    return y if y * y % P == a % P else None


def decompress(b, check_subgroup=True):
    """48 bytes -> affine (x, y) or INF; BadPoint on every encoding zkw_kzg_settings_create refuses"""
    assert len(b) == 48
    if not b[0] & 0x80:
        raise BadPoint("bit 7 clear (not a compressed point)")
    if b[0] & 0x40:
        if b[0] != 0xC0 or any(b[1:]):
            raise BadPoint("infinity flag with other bits set")
        return INF
    x = int.from_bytes(bytes([b[0] & 0x1F]) + b[1:], "big")
    if x >= P:
        raise BadPoint("x >= p")
    y = sqrt_fq((x * x * x + B) % P)
    if y is None:
        raise BadPoint("x has no y on the curve")
    if (y > P - y) != bool(b[0] & 0x20):
        y = P - y
    if check_subgroup and mul_naive(R, (x, y)) is not INF:
        raise BadPoint("not in the order-r subgroup")
    return (x, y)


def compress(pt):
    if pt is INF:
        return bytes([0xC0]) + bytes(47)
    x, y = pt
    out = bytearray(x.to_bytes(48, "big"))
    out[0] |= 0x80 | (0x20 if y > P - y else 0)
    return bytes(out)


# ---- Jacobian arithmetic (X, Y, Z); Z == 0 is infinity ----
J_INF = (1, 1, 0)


def jdbl(p):
    X, Y, Z = p
    if Z == 0 or Y == 0:
        return J_INF
    a, b = X * X % P, Y * Y % P
    c = b * b % P
    d = 2 * ((X + b) * (X + b) - a - c) % P
    e = 3 * a % P
    x3 = (e * e - 2 * d) % P
    return (x3, (e * (d - x3) - 8 * c) % P, 2 * Y * Z % P)


def jadd(p, q):
    X1, Y1, Z1 = p
    X2, Y2, Z2 = q
    if Z1 == 0:
        return q
    if Z2 == 0:
        return p
    z1z1, z2z2 = Z1 * Z1 % P, Z2 * Z2 % P
    u1, u2 = X1 * z2z2 % P, X2 * z1z1 % P
    s1, s2 = Y1 * Z2 * z2z2 % P, Y2 * Z1 * z1z1 % P
    if u1 == u2:
        return jdbl(p) if s1 == s2 else J_INF
    h, r = (u2 - u1) % P, (s2 - s1) % P
    h2 = h * h % P
    h3, v = h * h2 % P, u1 * h2 % P
    x3 = (r * r - h3 - 2 * v) % P
    return (x3, (r * (v - x3) - s1 * h3) % P, Z1 * Z2 * h % P)


def to_jac(pt):
    return J_INF if pt is INF else (pt[0], pt[1], 1)


def to_affine(p):
    X, Y, Z = p
    if Z == 0:
        return INF
    zi = pow(Z, P - 2, P)
    return (X * zi * zi % P, Y * zi * zi * zi % P)


def neg(pt):
    return INF if pt is INF else (pt[0], (P - pt[1]) % P)


def add(a, b):
    return to_affine(jadd(to_jac(a), to_jac(b)))


def mul_naive(k, pt):
    """double-and-add, most significant bit first"""
    acc = J_INF
    base = to_jac(pt)
    for bit in bin(k)[2:] if k else "":
        acc = jdbl(acc)
        if bit == "1":
            acc = jadd(acc, base)
    return to_affine(acc)


def msm_naive(scalars, points):
    acc = J_INF
    for k, pt in zip(scalars, points):
        acc = jadd(acc, to_jac(mul_naive(k, pt)))
    return to_affine(acc)


def msm(scalars, points, window=8):
    """bucket method: per window, digit d of scalar i sends point i into bucket d; sum_d d B_d by the running sum; windows by Horner"""
    nbits = max([s.bit_length() for s in scalars] + [1])
    pts = [to_jac(p) for p in points]
    acc = J_INF
    for w in reversed(range((nbits + window - 1) // window)):
        for _ in range(window):
            acc = jdbl(acc)
        buckets = [J_INF] * (1 << window)
        for s, p in zip(scalars, pts):
            d = (s >> (w * window)) & ((1 << window) - 1)
            if d:
                buckets[d] = jadd(buckets[d], p)
        run, tot = J_INF, J_INF
        for d in range((1 << window) - 1, 0, -1):
            run = jadd(run, buckets[d])
            tot = jadd(tot, run)
        acc = jadd(acc, tot)
    return to_affine(acc)


def load_setup_bytes():
    raw = open(SETUP_FILE, "rb").read()
    assert len(raw) == N_POINTS * 48
    return raw


_SETUP = None


def load_setup():
    """the 4 096 points S[k] = [tau^k] G1, decompressed (the subgroup check is the device's and test_kzg_model's business: ~2 s without it)"""
    global _SETUP
    if _SETUP is None:
        raw = load_setup_bytes()
        _SETUP = [decompress(raw[48 * k:48 * k + 48], check_subgroup=False) for k in range(N_POINTS)]
    return _SETUP


def commit(coeffs, points=None):
    """compress(sum_i coeffs[i] S[i])"""
    points = load_setup() if points is None else points
    assert len(coeffs) <= len(points) and all(0 <= c < R for c in coeffs)
    return compress(msm(list(coeffs), points[:len(coeffs)]))


def blob_elements(blob):
    assert len(blob) == BLOB_BYTES
    return [int.from_bytes(blob[31 * i:31 * i + 31], "little") for i in range(N_POINTS)]


def eip4844_witness(blob, points=None):
    e = blob_elements(blob)
    linear_hash = keccak256(bytes(blob))
    commitment = commit(e[::-1], points)  # coefficient of X^k is e[4095 - k]
    versioned_hash = b"\x01" + hashlib.sha256(commitment).digest()[1:]
    z_bytes = keccak256(linear_hash + versioned_hash)[16:32]
    z = int.from_bytes(z_bytes, "big")
    y = 0
    for ei in e:  # Horner: element 0 is the highest coefficient
        y = (y * z + ei) % R
    y_bytes = y.to_bytes(32, "big")
    return {"linear_hash": linear_hash, "versioned_hash": versioned_hash, "output_hash": keccak256(versioned_hash + z_bytes + y_bytes),
            "evaluation_point": z_bytes, "opening_value": y_bytes, "commitment": commitment}


def pattern_blob():
    return bytes((167 * j + 13) & 0xFF for j in range(BLOB_BYTES))
