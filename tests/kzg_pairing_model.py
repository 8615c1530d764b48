"""Host model of the BLS12-381 pairing and of KZG proof verification (verify_kzg_proof, kzg/src/lib.rs:259-282 of the reference) in plain
Python integers, on top of tests/kzg_model.py. It pins csrc/bls12_381_pairing.cuh (tests/test_gpu_bls_pairing.py) and zkw_kzg_verify /
zkw_eip4844_verify (tests/test_gpu_kzg_verify.py); the model itself is pinned by tests/test_kzg_pairing_model.py against the ceremony's
[tau] G2 (tests/golden/kzg_trusted_setup_g2.bin), which no model of this tree produced.

The tower and the basis are the device's: Fq2 = Fq[u] / (u^2 + 1), a pair (c0, c1); Fq12 = six Fq2 coefficients of w^k, w^6 = xi = 1 + u.
G2 is the order-r subgroup of the twist y^2 = x^3 + 4 xi over Fq2; (x, y) of the twist is (x / w^2, y / w^3) on the curve over Fq12, so
the line through T with slope lam, taken at P = (xP, yP) of G1 and scaled by w^3 (an element of Fq4, which the final exponentiation
sends to 1), is
    (lam xT - yT)  -  lam xP w^2  +  yP w^3
— three coefficients out of six. The Miller loop walks |x| = 0xd201000000010000 (63 doublings, 5 additions: 68 lines) and conjugates at
the end, since x is negative. The final exponentiation raises to FINAL_EXP_MULTIPLE = 3 times (p^12 - 1) / r:
    3 (p^4 - p^2 + 1) / r = (x - 1)^2 (x + p) (x^2 + p^2 - 1) + 3
and p^4 - p^2 + 1 = 1 mod 3, so the cube is one exactly when the pairing is.

verify_kzg_proof here is the reference's form, with [tau] G2 - [z] G2 computed in G2; the device moves [z] into G1 (all of its
run-time scalar multiplications are there), so the two reach a verdict by different routes.

`python -m tests.kzg_pairing_model` prints the constants of the device header (Montgomery form, 32-bit words, lowest first)."""
import os

from tests import kzg_model as km

P, R = km.P, km.R
X_ABS = 0xD201000000010000  # the curve's parameter is -X_ABS
FINAL_EXP_MULTIPLE = 3
G2_FILE = os.path.join(km.GOLDEN, "kzg_trusted_setup_g2.bin")
INF = None

# ---- Fq2 -------------------------------------------------------------------------------------------------------------------------------
F2_ZERO, F2_ONE, XI = (0, 0), (1, 0), (1, 1)


def f2_add(a, b):
    return ((a[0] + b[0]) % P, (a[1] + b[1]) % P)


def f2_sub(a, b):
    return ((a[0] - b[0]) % P, (a[1] - b[1]) % P)


def f2_neg(a):
    return (-a[0] % P, -a[1] % P)


def f2_conj(a):
    return (a[0], -a[1] % P)


def f2_mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def f2_sqr(a):
    return f2_mul(a, a)


def f2_scale(a, s):
    return (a[0] * s % P, a[1] * s % P)


def f2_mul_xi(a):
    return ((a[0] - a[1]) % P, (a[0] + a[1]) % P)


def f2_inv(a):
    """0 -> 0, as the device's Fermat inversion"""
    n = pow((a[0] * a[0] + a[1] * a[1]) % P, P - 2, P)
    return (a[0] * n % P, -a[1] * n % P)


def f2_pow(a, e):
    r = F2_ONE
    for bit in bin(e)[2:] if e else "":
        r = f2_sqr(r)
        if bit == "1":
            r = f2_mul(r, a)
    return r


def f2_sqrt(a):
    """a root of a, or None (p = 3 mod 4: Adj and Rodriguez-Henriquez, algorithm 9). The device walks the same steps, so the two agree
    on WHICH root"""
    a1 = f2_pow(a, (P - 3) // 4)
    alpha = f2_mul(f2_sqr(a1), a)
    if f2_mul(f2_conj(alpha), alpha) == (P - 1, 0):
        return None
    x0 = f2_mul(a1, a)
    if alpha == (P - 1, 0):
        x = (-x0[1] % P, x0[0])  # u x0
    else:
        x = f2_mul(f2_pow(f2_add(F2_ONE, alpha), (P - 1) // 2), x0)
    return x if f2_sqr(x) == (a[0] % P, a[1] % P) else None


def f2_is_larger(y):
    """the compressed form's sign: y above -y, comparing c1 first and c0 when c1 is zero"""
    return y[1] > P - y[1] if y[1] else y[0] > P - y[0]


# ---- Fq12: [a_0 .. a_5], the coefficients of w^k ---------------------------------------------------------------------------------------
F12_ONE = [F2_ONE] + [F2_ZERO] * 5
GAMMA1 = [f2_pow(XI, k * (P - 1) // 6) for k in range(6)]          # w^(k (p - 1))
GAMMA2 = [f2_mul(g, f2_conj(g)) for g in GAMMA1]                    # w^(k (p^2 - 1)): in Fq
assert all(g[1] == 0 for g in GAMMA2)


def f12_mul(a, b):
    out = []
    for k in range(6):
        lo, hi = F2_ZERO, F2_ZERO
        for i in range(6):
            t = f2_mul(a[i], b[(k - i) % 6])
            if i > k:
                hi = f2_add(hi, t)  # i + j = k + 6: the w^6 = xi wrap
            else:
                lo = f2_add(lo, t)
        out.append(f2_add(lo, f2_mul_xi(hi)))
    return out


def f12_sqr(a):
    return f12_mul(a, a)


def f12_mul_line(a, l0, l2, l3):
    """a times l0 + l2 w^2 + l3 w^3 (l3 in Fq: an integer)"""
    out = []
    for k in range(6):
        t = f2_mul(a[k], l0)
        t2 = f2_mul(a[(k - 2) % 6], l2)
        t3 = f2_scale(a[(k - 3) % 6], l3)
        t = f2_add(t, f2_mul_xi(t2) if k < 2 else t2)
        out.append(f2_add(t, f2_mul_xi(t3) if k < 3 else t3))
    return out


def f12_conj(a):
    """the p^6 map: w -> -w"""
    return [f2_neg(c) if k & 1 else c for k, c in enumerate(a)]


def f12_frob(a, n=1):
    """the p^n map, n in {1, 2, 3, 6}"""
    if n == 1:
        return [f2_mul(f2_conj(c), GAMMA1[k]) for k, c in enumerate(a)]
    if n == 2:
        return [f2_scale(c, GAMMA2[k][0]) for k, c in enumerate(a)]
    if n == 3:
        return f12_frob(f12_frob(a, 2), 1)
    assert n == 6
    return f12_conj(a)


def f12_inv(a):
    """a conj(a) lies in Fq6 (odd coefficients zero); an element s of Fq6 times s^(p^2) s^(p^4) lies in Fq2: one Fq inversion in all"""
    ac = f12_conj(a)
    s = f12_mul(a, ac)
    t = f12_mul(f12_frob(s, 2), f12_frob(f12_frob(s, 2), 2))
    n = f12_mul(s, t)
    assert all(c == F2_ZERO for c in n[1:])
    ni = f2_inv(n[0])
    return [f2_mul(c, ni) for c in f12_mul(ac, t)]


def f12_pow(a, e):
    r = F12_ONE
    for bit in bin(e)[2:] if e else "":
        r = f12_sqr(r)
        if bit == "1":
            r = f12_mul(r, a)
    return r


# ---- G2: affine points (x, y) of the twist, x and y in Fq2; INF = None -------------------------------------------------------------------
B2 = (4, 4)  # 4 xi
G2_GEN = ((0x024AA2B2F08F0A91260805272DC51051C6E47AD4FA403B02B4510B647AE3D1770BAC0326A805BBEFD48056C8C121BDB8,
           0x13E02B6052719F607DACD3A088274F65596BD0D09920B61AB5DA61BBDC7F5049334CF11213945D57E5AC7D055D042B7E),
          (0x0CE5D527727D6E118CC9CDC6DA2E351AADFD9BAA8CBDD3A76D429A695160D12C923AC9CC3BACA289E193548608B82801,
           0x0606C4A02EA734CC32ACD2B02BC28B99CB3E287E85A763AF267492AB572E99AB3F370D275CEC1DA1AAA9075FF05F79BE))


def g2_on_twist(q):
    return q is INF or f2_sqr(q[1]) == f2_add(f2_mul(f2_sqr(q[0]), q[0]), B2)


def g2_neg(q):
    return INF if q is INF else (q[0], f2_neg(q[1]))


def g2_dbl_line(t):
    """(2 T, lam, lam xT - yT)"""
    lam = f2_mul(f2_scale(f2_sqr(t[0]), 3), f2_inv(f2_scale(t[1], 2)))
    x3 = f2_sub(f2_sqr(lam), f2_scale(t[0], 2))
    return (x3, f2_sub(f2_mul(lam, f2_sub(t[0], x3)), t[1])), lam, f2_sub(f2_mul(lam, t[0]), t[1])


def g2_add_line(t, q):
    """(T + Q, lam, lam xT - yT), T != +-Q"""
    lam = f2_mul(f2_sub(t[1], q[1]), f2_inv(f2_sub(t[0], q[0])))
    x3 = f2_sub(f2_sub(f2_sqr(lam), t[0]), q[0])
    return (x3, f2_sub(f2_mul(lam, f2_sub(t[0], x3)), t[1])), lam, f2_sub(f2_mul(lam, t[0]), t[1])


def g2_add(a, b):
    if a is INF:
        return b
    if b is INF:
        return a
    if a[0] == b[0]:
        if a[1] != b[1] or a[1] == F2_ZERO:
            return INF
        return g2_dbl_line(a)[0]
    return g2_add_line(a, b)[0]


def g2_mul(k, q):
    acc = INF
    for bit in bin(k)[2:] if k else "":
        acc = g2_add(acc, acc)
        if bit == "1":
            acc = g2_add(acc, q)
    return acc


PSI_X = f2_inv(f2_pow(XI, (P - 1) // 3))
PSI_Y = f2_inv(f2_pow(XI, (P - 1) // 2))


def g2_psi(q):
    """the untwist-Frobenius-twist endomorphism; on G2 it is multiplication by p = x mod r"""
    return INF if q is INF else (f2_mul(f2_conj(q[0]), PSI_X), f2_mul(f2_conj(q[1]), PSI_Y))


def g2_in_subgroup(q):
    return g2_mul(R, q) is INF


def g2_compress(q):
    """96 bytes: x.c1 then x.c0, big-endian; the flags of G1's form in the first byte"""
    if q is INF:
        return bytes([0xC0]) + bytes(95)
    out = bytearray(q[0][1].to_bytes(48, "big") + q[0][0].to_bytes(48, "big"))
    out[0] |= 0x80 | (0x20 if f2_is_larger(q[1]) else 0)
    return bytes(out)


def g2_decompress(b, check_subgroup=True):
    """96 bytes -> (x, y) or INF; km.BadPoint on every encoding zkw_kzg_verifier_create refuses (infinity itself is the caller's)"""
    assert len(b) == 96
    if not b[0] & 0x80:
        raise km.BadPoint("bit 7 clear (not a compressed point)")
    if b[0] & 0x40:
        if b[0] != 0xC0 or any(b[1:]):
            raise km.BadPoint("infinity flag with other bits set")
        return INF
    x = (int.from_bytes(b[48:], "big"), int.from_bytes(bytes([b[0] & 0x1F]) + b[1:48], "big"))
    if x[0] >= P or x[1] >= P:
        raise km.BadPoint("a coordinate >= p")
    y = f2_sqrt(f2_add(f2_mul(f2_sqr(x), x), B2))
    if y is None:
        raise km.BadPoint("x has no y on the twist")
    if f2_is_larger(y) != bool(b[0] & 0x20):
        y = f2_neg(y)
    if check_subgroup and not g2_in_subgroup((x, y)):
        raise km.BadPoint("not in the order-r subgroup")
    return (x, y)


def outside_g2():
    """(test vectors) a twist point outside the order-r subgroup: the cofactor is huge, so the first x = (k, 0) with a root serves"""
    k = 1
    while True:
        y = f2_sqrt(f2_add((k ** 3 % P, 0), B2))
        if y is not None:
            return ((k, 0), y)
        k += 1


def no_root_g2():
    """(test vectors) 96 bytes whose x = (k, 0) has no y on the twist"""
    k = 1
    while f2_sqrt(f2_add((k ** 3 % P, 0), B2)) is not None:
        k += 1
    return bytes([0x80]) + bytes(47) + k.to_bytes(48, "big")


def load_tau_g2_bytes():
    raw = open(G2_FILE, "rb").read()
    assert len(raw) == 96
    return raw


# ---- the pairing -----------------------------------------------------------------------------------------------------------------------
def g2_lines(q):
    """the 68 (lam, lam xT - yT) of the Miller loop over |x|, and [|x|] Q"""
    t, out = q, []
    for bit in bin(X_ABS)[3:]:
        t, lam, c = g2_dbl_line(t)
        out.append((lam, c))
        if bit == "1":
            t, lam, c = g2_add_line(t, q)
            out.append((lam, c))
    return out, t


def miller_loop(pairs):
    """the product of the Miller functions of (P in G1, Q in G2) pairs on one accumulator; a pair with a point at infinity contributes 1"""
    pairs = [(p, g2_lines(q)[0]) for p, q in pairs if p is not INF and q is not INF]
    f, k = F12_ONE, 0
    for bit in bin(X_ABS)[3:]:
        f = f12_sqr(f)
        for (xp, yp), lines in pairs:
            lam, c = lines[k]
            f = f12_mul_line(f, c, f2_neg(f2_scale(lam, xp)), yp)
        k += 1
        if bit == "1":
            for (xp, yp), lines in pairs:
                lam, c = lines[k]
                f = f12_mul_line(f, c, f2_neg(f2_scale(lam, xp)), yp)
            k += 1
    return f12_conj(f)


def _pow_x(a):
    """a^x for a in the cyclotomic subgroup (where the inverse is the conjugate)"""
    return f12_conj(f12_pow(a, X_ABS))


def final_exp(f):
    """f^(3 (p^12 - 1) / r)"""
    t = f12_mul(f12_conj(f), f12_inv(f))        # p^6 - 1
    t = f12_mul(f12_frob(t, 2), t)              # p^2 + 1
    a = f12_mul(_pow_x(t), f12_conj(t))         # x - 1
    a = f12_mul(_pow_x(a), f12_conj(a))         # (x - 1)^2
    b = f12_mul(_pow_x(a), f12_frob(a, 1))      # x + p
    c = f12_mul(f12_mul(_pow_x(_pow_x(b)), f12_frob(b, 2)), f12_conj(b))  # x^2 + p^2 - 1
    return f12_mul(c, f12_mul(f12_sqr(t), t))


def pairing(p, q):
    """e(P, Q)^3"""
    return final_exp(miller_loop([(p, q)]))


def pairing_product_is_one(pairs):
    return final_exp(miller_loop(pairs)) == F12_ONE


def g1_gen():
    return km.decompress(km.load_setup_bytes()[:48], check_subgroup=False)


def verify_kzg_proof(commitment, z, y, proof, tau_g2):
    """lib.rs:259-282: e(C - [y] G1, -G2) e(proof, [tau] G2 - [z] G2) == 1, points decompressed"""
    x_minus_z = g2_add(tau_g2, g2_neg(g2_mul(z, G2_GEN)))
    p_minus_y = km.add(commitment, km.neg(km.mul_naive(y, g1_gen())))
    return pairing_product_is_one([(p_minus_y, g2_neg(G2_GEN)), (proof, x_minus_z)])


# ---- the device header's constants -----------------------------------------------------------------------------------------------------
def mont_words(a):
    v = a * (1 << 384) % P
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(12)]


def _c_fq(a):
    return "{{" + ", ".join("0x%08xu" % w for w in mont_words(a)) + "}}"


def _c_words(v, n):
    return "{" + ", ".join("0x%08xu" % ((v >> (32 * i)) & 0xFFFFFFFF) for i in range(n)) + "}"


if __name__ == "__main__":
    print("// w^(k (p - 1)), k < 6: (c0, c1)")
    for g in GAMMA1:
        print("    {%s, %s}," % (_c_fq(g[0]), _c_fq(g[1])))
    print("// w^(k (p^2 - 1)), k < 6: in Fq")
    for g in GAMMA2:
        print("    %s," % _c_fq(g[0]))
    print("// psi: 1 / xi^((p - 1) / 3), 1 / xi^((p - 1) / 2)")
    for g in (PSI_X, PSI_Y):
        print("    {%s, %s}," % (_c_fq(g[0]), _c_fq(g[1])))
    print("// (p - 3) / 4:", _c_words((P - 3) // 4, 12))
    print("// (p - 1) / 2:", _c_words((P - 1) // 2, 12))
    print("// -G2 compressed:", ", ".join("0x%02x" % b for b in g2_compress(g2_neg(G2_GEN))))
