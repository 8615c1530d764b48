"""Host model of the setup in the Lagrange basis (zkw_kzg_settings_to_lagrange; KzgSettings::new, kzg/src/lib.rs:91-141 of the reference),
for a tau that is no secret. It shares nothing with the kernels' route: no transform of points at all.

The Lagrange polynomial of w^j on the domain of the n-th roots of unity (w = 7^((r - 1) / n)) is l_j(X) = w^j (X^n - 1) / (n (X - w^j)), so
the SCALARS l_j(tau) come in closed form, and L[j] = [l_j(tau)] G1 is one fixed-base product each. Where tau is on the domain, tau = w^i,
the closed form is 0 / 0 at j = i: there l_j(tau) is 1 at j = i and 0 elsewhere. The products run over a byte-window table of the
generator (2^(8 w) d G for 32 windows and d < 256): a sum of at most 32 table entries per scalar over tests/kzg_model.py's jadd."""
from tests import kzg_model as km

R = km.R


def root(n):
    return pow(7, (R - 1) // n, R)


def brp(i, bits):
    return int(format(i, "0%db" % bits)[::-1], 2) if bits else 0


def lagrange_scalars(tau, n):
    """[l_j(tau) for j < n], n a power of two"""
    w = root(n)
    tau %= R
    top = (pow(tau, n, R) - 1) % R
    if top == 0:  # tau is on the domain
        out, wj = [], 1
        for _ in range(n):
            out.append(1 if wj == tau else 0)
            wj = wj * w % R
        assert sum(out) == 1
        return out
    top = top * pow(n, -1, R) % R
    out, wj = [], 1
    for _ in range(n):
        out.append(wj * top % R * pow((tau - wj) % R, -1, R) % R)
        wj = wj * w % R
    return out


def inverse_transform(values):
    """(1 / n) sum_k w^(-j k) values[k] for every j, by the definition's recursion (radix 2) on scalars"""
    n = len(values)

    def rec(x, wi):
        if len(x) == 1:
            return x
        even, odd = rec(x[0::2], wi * wi % R), rec(x[1::2], wi * wi % R)
        out, t = [0] * len(x), 1
        for j in range(len(x) // 2):
            out[j] = (even[j] + t * odd[j]) % R
            out[j + len(x) // 2] = (even[j] - t * odd[j]) % R
            t = t * wi % R
        return out

    n_inv = pow(n, -1, R)
    return [v * n_inv % R for v in rec(list(values), pow(root(n), -1, R))]


def forward_transform(values):
    """sum_k w^(j k) values[k] for every j (scalars)"""
    n = len(values)
    back = inverse_transform(values)  # (1 / n) sum_k w^(-j k) v[k]
    return [back[(-j) % n] * n % R for j in range(n)]


_TABLE = None


def _table():
    """_TABLE[w][d] = [2^(8 w) d] G (Jacobian), d < 256"""
    global _TABLE
    if _TABLE is None:
        base = km.to_jac(km.decompress(km.load_setup_bytes()[:48], check_subgroup=False))
        _TABLE = []
        for _ in range(32):
            row = [km.J_INF]
            for _d in range(255):
                row.append(km.jadd(row[-1], base))
            _TABLE.append(row)
            base = km.jadd(row[-1], base)  # 256 base
    return _TABLE


def generator_times(k):
    """[k] G, Jacobian"""
    table, acc = _table(), km.J_INF
    k %= R
    for w in range(32):
        d = (k >> (8 * w)) & 0xFF
        if d:
            acc = km.jadd(acc, table[w][d])
    return acc


def generator_points(scalars):
    """compress([k] G) for every k, concatenated"""
    return b"".join(km.compress(km.to_affine(generator_times(k))) for k in scalars)


def lagrange_setup_brp(tau, n):
    """the n x 48 bytes a handle holds after to_lagrange of S[k] = [tau^k] G1: entry i = [l_brp(i)(tau)] G1"""
    bits = n.bit_length() - 1
    sc = lagrange_scalars(tau, n)
    return generator_points([sc[brp(i, bits)] for i in range(n)])
