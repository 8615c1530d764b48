"""Host model of EIP-7594 recovery (recover_cells_and_kzg_proofs of the consensus specs) in plain Python integers, on top of
tests/kzg_cells_model.py. It pins zkw_kzg_recover_cells_blobs (tests/test_gpu_kzg_recover.py); the model itself is pinned by
tests/test_kzg_recover_model.py.

`recover` is the model. It shares nothing with the device's route: P = sum_(m < 64) X^m g_m(X^64); the 64 points of cell k are
x0 zeta^brp6(t), x0 = W^brp7(k), zeta = W^128 (x0^64 = c_k), so the cell's values are the 64-point transform of y_m = x0^m g_m(c_k), one
inverse transform per supplied cell gives the g_m(c_k), and each g_m (degree below 64) is the Lagrange interpolant through the 64
constants c_k of the FIRST 64 supplied cells. Every further supplied cell must equal kzg_cells_model.cells of the result, else the set lies
on no polynomial of degree below 4 096 (`Inconsistent`).

`vanishing_route` restates, stage by stage and index by index, what csrc/kzg_recover_kernels.cuh does (the vanishing polynomial of the
missing cells over a coset), so that its index arithmetic is checked on the host before a kernel runs."""
from tests import kzg_cells_model as cm
from tests import kzg_open_model as om

R = cm.R
N = cm.N
CELLS = cm.CELLS
CELL = cm.CELL
W = cm.W
W128 = cm.W128
OMEGA = cm.OMEGA
SHIFT = 7  # s: any s with s^8192 != 1 keeps Z(X) = z(X^64) away from zero on the coset s w^i
ABSENT = 0xFF


class Inconsistent(ValueError):
    """the supplied cells do not lie on one polynomial of degree below 4 096"""


def check_indices(cell_indices):
    idx = list(cell_indices)
    assert CELL <= len(idx) <= CELLS and all(0 <= k < CELLS for k in idx) and all(a < b for a, b in zip(idx, idx[1:])), idx
    return idx


def cell_elements(cell):
    assert len(cell) == 32 * CELL
    v = [int.from_bytes(cell[32 * t:32 * t + 32], "big") for t in range(CELL)]
    assert all(x < R for x in v)
    return v


def _lagrange_basis(xs):
    """[L_k lowest first]: L_k(xs[j]) = (j == k), by dividing the master polynomial prod (Y - x) by (Y - x_k)"""
    master = [1]
    for x in xs:
        master = [((master[i - 1] if i else 0) - x * (master[i] if i < len(master) else 0)) % R for i in range(len(master) + 1)]
    out = []
    for x in xs:
        q, carry = [0] * len(xs), 0
        for i in range(len(xs), 0, -1):  # synthetic division, top down
            carry = (master[i] + carry * x) % R
            q[i - 1] = carry
        scale = pow(cm.evaluate(q, x), R - 2, R)
        out.append([c * scale % R for c in q])
    return out


def recover(cell_indices, cells):
    """the 4 096 coefficients, lowest first, of the polynomial of degree below 4 096 through the supplied cells (bytes, in the list's
    order)"""
    idx = check_indices(cell_indices)
    assert len(cells) == len(idx)
    zeta_inv, inv64 = pow(W, R - 1 - 128, R), pow(CELL, R - 2, R)
    g_at = []  # per supplied cell of the first 64: [g_m(c_k) for m]
    for k, cell in zip(idx[:CELL], cells):
        v = cell_elements(cell)
        y = om._ntt([v[cm.brp(j, 6)] for j in range(CELL)], zeta_inv)  # v in the order of the exponent of zeta
        x0_inv = pow(W, R - 1 - cm.brp(k, 7), R)
        g_at.append([y[m] * inv64 % R * pow(x0_inv, m, R) % R for m in range(CELL)])
    basis = _lagrange_basis([cm.cell_constant(k) for k in idx[:CELL]])
    coeffs = [0] * N
    for m in range(CELL):
        for d in range(CELL):  # coefficient d of g_m is the coefficient of X^(m + 64 d)
            coeffs[m + CELL * d] = sum(g_at[j][m] * basis[j][d] for j in range(CELL)) % R
    if len(idx) > CELL:
        full = cm.cells(coeffs)
        if any(full[k] != bytes(cell) for k, cell in zip(idx[CELL:], cells[CELL:])):
            raise Inconsistent("the supplied cells lie on no polynomial of degree below 4096")
    return coeffs


def recover_cells(cell_indices, cells):
    """(the 128 cells, the coefficients)"""
    coeffs = recover(cell_indices, cells)
    return cm.cells(coeffs), coeffs


def evaluation_form(coeffs):
    """the blob in evaluation form: cells 0..63"""
    return b"".join(cm.cells(coeffs)[:CELL])


# ---- the device's route, restated -----------------------------------------------------------------------------------------------------------
def slot_table(cell_indices):
    """slot[k] = the position of cell k in the list, ABSENT for a missing cell: the kernels' 128-byte argument"""
    slot = [ABSENT] * CELLS
    for i, k in enumerate(check_indices(cell_indices)):
        slot[k] = i
    return slot


def _dif(x, root):
    """the stages of k_kzg_blob_ntt on len(x) = 2^b points: natural order in, x[i'] = sum_k x[k] root^(k brp_b(i')) out"""
    n, s = len(x), 0
    half = n // 2
    while half:
        for b in range(n // 2):
            j = b & (half - 1)
            i0 = ((b // half) * 2 * half) | j
            u, v = x[i0], x[i0 + half]
            x[i0], x[i0 + half] = (u + v) % R, (u - v) * pow(root, j << s, R) % R
        half //= 2
        s += 1
    return x


def _dif_undo(x, tw):
    """the stages of k_kzg_blob_intt on 4 096 points with the table tw[j] = w^j, j < 2048: bit-reversed order in, natural order out, times
    4 096. w^-e = -w^(2048 - e): the table read backwards with add and sub exchanged, entry 0 with them as they are"""
    for s in range(11, -1, -1):
        half = 2048 >> s
        for b in range(2048):
            j = b & (half - 1)
            i0 = ((b >> (11 - s)) << (12 - s)) | j
            u, m = x[i0], x[i0 + half] * tw[(2048 - (j << s)) & 2047] % R
            with_, without = (u + m) % R, (u - m) % R
            x[i0], x[i0 + half] = (with_, without) if j == 0 else (without, with_)
    return x


def vanishing_values(slot):
    """k_kzg_recover_vanish: (zc, zinv); zc[k] = z(c_k), the factor of cell k (zero exactly on the missing cells); zinv[u] =
    1 / z(s^64 w128^(2 u)), u < 64, the 64 values Z takes on the coset s w^i"""
    z = [1] + [0] * (CELLS - 1)
    for k in range(CELLS):
        if slot[k] == ABSENT:
            c = cm.cell_constant(k)
            z = [((z[m - 1] if m else 0) - c * z[m]) % R for m in range(CELLS)]
    assert not any(z[CELL + 1:])
    zc = _dif(list(z), W128)  # position k holds z(w128^brp7(k)) = z(c_k)
    s64 = pow(SHIFT, CELL, R)
    on_coset = _dif([c * pow(s64, m, R) % R for m, c in enumerate(z)], W128)  # position q < 64: z(s^64 w128^brp7(q)), brp7(q) = 2 brp6(q)
    zinv = [0] * CELL
    for q in range(CELL):
        zinv[cm.brp(q, 6)] = pow(on_coset[q], R - 2, R)
    return zc, zinv


def vanishing_route(cell_indices, cells):
    """the coefficients by the kernels' route; no consistency check here (the device compares the recomputed cells)"""
    slot = slot_table(cell_indices)
    zc, zinv = vanishing_values(slot)
    tw = [pow(OMEGA, j, R) for j in range(2048)]
    wpow = [pow(W, k, R) for k in range(N)]
    elements = [cell_elements(c) for c in cells]
    # k_kzg_recover_halves: half h holds positions 4096 h + i of E Z, the point of position i is W^h w^brp12(i)
    halves = []
    for h in range(2):
        x = [0] * N
        for i in range(N):
            k = CELL * h + (i >> 6)
            if slot[k] != ABSENT:
                x[i] = elements[slot[k]][i & 63] * zc[k] % R
        x = _dif_undo(x, tw)  # 4096 times the coefficients
        if h:  # b_i = b'_i W^-i, W^-i = -W^(4096 - i) for i >= 1: k_kzg_cell_wpow's table backwards, the sign changed
            x = [x[0]] + [(R - x[i] * wpow[N - i] % R) % R for i in range(1, N)]
        halves.append(x)
    a, b = halves
    # k_kzg_recover_quotient: F = D mod (X^4096 - s^4096); the factors 1 / 2 and 1 / 4096 (twice: the halves' transform and this one's)
    c = pow(SHIFT, N, R)
    inv = pow(2 * N * N, R - 2, R)
    fold_a, fold_b = (1 + c) * inv % R, (1 - c) * inv % R
    x = _dif([(a[i] * fold_a + b[i] * fold_b) % R * pow(SHIFT, i, R) % R for i in range(N)], OMEGA)
    x = [x[i] * zinv[cm.brp(i >> 6, 6)] % R for i in range(N)]  # position i' holds F(s w^brp12(i')), and brp12(i') mod 64 = brp6(i' >> 6)
    x = _dif_undo(x, tw)
    s_inv = pow(SHIFT, R - 2, R)
    return [x[i] * pow(s_inv, i, R) % R for i in range(N)]


def device_constants():
    """name -> value of the constants csrc/kzg_recover_kernels.cuh carries in Montgomery form"""
    c, inv = pow(SHIFT, N, R), pow(2 * N * N, R - 2, R)
    return {"kzg_recover_s_inv": pow(SHIFT, R - 2, R), "kzg_recover_fold_a": (1 + c) * inv % R, "kzg_recover_fold_b": (1 - c) * inv % R}


def montgomery_words(v):
    m = v * (1 << 256) % R
    return [(m >> (32 * i)) & 0xFFFFFFFF for i in range(8)]
