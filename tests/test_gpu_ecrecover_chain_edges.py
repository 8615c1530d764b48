"""GPU: the ECRecover circuit (type 7) at the edges of its accumulator chain — requests WITHOUT a witness, and scalars at the ends of the chain.

The circuit's additions are incomplete (affine, x1 != x2), made safe against accidents by the public offset point
O = hash_point(b"zkw ecrecover accumulator offset"): the accumulator starts at O, takes 256 double-and-add steps over the bits of u2 = s / r
(top bit first; the addition of R is evaluated at EVERY step and selected by the bit), then subtracts byte C of u1 = h / r times 2^(8C) G for
every non-zero byte, then adds -2^256 O. With j the value of the top t bits of u2 the accumulator after step t's doubling is
2^t O + (j >> 1 << 1) R, so anyone can publish a signature whose chain meets x1 == x2: such a request still recovers a valid address, but the
circuit has no witness for it and zkw_ecrecover_synthesize refuses it (ERR_CHECK_FAILED, naming the request). Everything here is constructed
in Python integers from secp256k1.py alone: hash_point is restated and checked against the offset point the spec holds, and `_first_meeting`
walks the chain with the affine addition to say where a request meets x1 == x2 (or that it never does).

Why a refused cycle cannot write outside its buffers (read from the code before these tests ran on a GPU). On the fast path the refusal is
indirect: ecl::jmadd leaves Z == 0 (h == 0 in Z3 = Z1 h), every later point of the chain keeps Z == 0 (jdbl: Z3 = 2 Y Z; jmadd: Z3 = Z h),
k_ec_affine flags those points and writes nothing for them, so the `out` states of their segments stay as the scratch held them (an earlier
call's values, or whatever the allocation held); where the bit of the step is clear the chain never adds, all points are written, and the
refusal comes from the segment's own H_DIV (b == 0). Either way status is raised by atomicMax and read after the last kernel, and:
  - k_ec_chain: PRE's MAIN items have a witness for every 128 input bytes (out-of-range r / s are replaced by the substitute signature, 1 / r is
    taken of the replaced value), and lane 0 returns before the chain otherwise; so the globals are written when the chain reads them: the bits
    of u2 are masked `& 1`, and the index into S.fixed comes from the bytes of u1 — the byte split of the canonical 16-bit limbs ec_to_limbs16
    wrote, each <= 255 — so ((8 C + limb) * 256 + byte) * 2 + 1 stays below the table's 256 * 256 * 2 words;
  - ec_eval_items_of (k_ec_segments, k_ec_leaves): tape reads and writes go to positions the spec names (base + constant); the only
    value-derived index is the lookup's table index `a`, refused when a > 255 (Xor8: b too) before it is used; ec_get_vec refuses values above
    32 bits, H_DIV refuses b == 0 and inverts a reduced non-zero value modulo a prime (the binary Euclid ends), the MUL row's loops have constant
    bounds; an item that fails ends its list, later items of the list keep stale values — values, never positions;
  - k_ec_prepare masks the key bytes `& 0xFF`; k_ec_stream stores what it reads at (column, row) pairs of the spec, and its Xor8 keys at a slot
    fixed by (instance, cycle, row); k_ec_hist bins keys `& 32767` after selecting a half by `>> 15` of a 16-bit key, and its FixedBaseMul
    counts read the byte cell of a FIX row — a copy of the same u1 byte global (< 256) — and fifteen constant-zero padding slots.
So a refused request costs its call, nothing else; the trace slots are not claimed and the next call overwrites tape and trace. Capacity 2 and
2^18 rows, like tests/test_gpu_ecrecover_circuit.py."""
import os
import re

import numpy as np
import pytest

from era_zkevm_test_harness_amd import secp256k1 as ec
from era_zkevm_test_harness_amd import synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_ROWS = 1 << 18
CAP = 2
N, P = ec.N, ec.P


def _hash_point(tag):
    """tools/gen_ecrecover_circuit.py hash_point, restated: try-and-increment on keccak256(tag || counter), the even root"""
    ctr = 0
    while True:
        x = int.from_bytes(ec.keccak256(tag + ctr.to_bytes(4, "big")), "big") % P
        pt = ec.lift_x(x, 0)
        if pt is not None:
            return pt
        ctr += 1


O = _hash_point(b"zkw ecrecover accumulator offset")
O_END = ec.neg(ec.mul(pow(2, 256, N), O))  # what POST adds: -2^256 O
H_ANY = 0x456E9AEA5E197A1F1AF7A3E85A3212FA4049A3BA34C2289B4C860FC0B0C64EF3


def _first_meeting(h, v, r, s):
    """where the circuit's chain meets x1 == x2 for a request with 0 < r, s < n and r on the curve: ("daa", step) / ("fix", byte) / ("post", 0)
    with "equal" or "opposite" for the two points, or None — by the affine addition of secp256k1.py"""
    R = ec.lift_x(r, v)
    ri = pow(r, -1, N)
    u2, u1 = s * ri % N, h * ri % N
    acc = O

    def meets(q):
        return None if acc[0] != q[0] else "equal" if acc[1] == q[1] else "opposite"

    for k in range(256):
        acc = ec.add(acc, acc)
        if meets(R):  # (evaluated whatever the bit)
            return ("daa", k), meets(R)
        if (u2 >> (255 - k)) & 1:
            acc = ec.add(acc, R)
    for c in range(32):
        b = (u1 >> (8 * c)) & 0xFF
        if b:
            t = ec.neg(ec.mul(b << (8 * c), ec.G))
            if meets(t):
                return ("fix", c), meets(t)
            acc = ec.add(acc, t)
    return (("post", 0), meets(O_END)) if meets(O_END) else None


def _request(R, u2, u1=None, h=H_ANY):
    """(h, v, r, s) with s / r = u2 and, when u1 is given, h / r = u1"""
    r, v = R[0], R[1] & 1
    s = u2 * r % N
    if u1 is not None:
        h = u1 * r % N
    assert 0 < r < N and 0 < s < N and ec.lift_x(r, v) == R
    assert s * pow(r, -1, N) % N == u2 and (u1 is None or h * pow(r, -1, N) % N == u1)
    return h, v, r, s


def _crafted():
    """name -> (request, where its chain meets x1 == x2)"""
    out = {}
    two_o = ec.add(O, O)
    u2 = (1 << 255) + 0x1234567
    out["a_first_step_equal"] = _request(two_o, u2), (("daa", 0), "equal")
    out["b_first_step_opposite"] = _request(ec.neg(two_o), u2), (("daa", 0), "opposite")
    # deep in the chain: before the addition of step t - 1 the accumulator is 2^t O + (j - 1) R; R = 2^t / (2 - j) O makes it R itself
    t = 200
    u2 = (0xB5C0FBCFEC4D3B2F9E3779B97F4A7C15F39CC0605CEDC8341082276BF3A27251 | 1 << (256 - t)) % N
    j = u2 >> (256 - t)
    assert j & 1 and u2 < N
    out["c_deep_in_the_chain"] = _request(ec.mul((1 << t) * pow(2 - j, -1, N) % N, O), u2), (("daa", t - 1), "equal")
    # table stage: u1 = b, one non-zero byte; after the 256 steps the accumulator is 2^256 O + u2 R = +- b G
    b, u2 = 0xA7, 0x6A09E667F3BCC908BB67AE8584CAA73B3C6EF372FE94F82BA54FF53A5F1D36F1
    d = ec.add(ec.mul(b, ec.G), O_END)  # b G - 2^256 O
    out["d_table_opposite"] = _request(ec.mul(pow(u2, -1, N), d), u2, u1=b), (("fix", 0), "opposite")
    d = ec.add(ec.neg(ec.mul(b, ec.G)), O_END)
    out["e_table_equal"] = _request(ec.mul(pow(u2, -1, N), d), u2, u1=b), (("fix", 0), "equal")
    # the addition of a step is evaluated whatever the bit: a clear top bit of u2 does not save R = 2 O. The chain kernel never adds here: the
    # refusal comes from the segment's own division
    out["f_first_step_bit_clear"] = _request(two_o, 0x1234567), (("daa", 0), "equal")
    return out


CRAFTED = _crafted()


def test_offset_point_restated_equals_the_spec():
    """the constructions above stand on it: the 16-bit limbs of O in the generated spec"""
    text = open(os.path.join(ROOT, "include", "zkw_ecrecover_ec_spec.h")).read()
    bigs = [int(x) for x in re.findall(r"\d+", re.search(r"#define EC_BIG_INIT \{([^}]*)\}", text).group(1))]
    ox, oy = (int(re.search(rf"#define EC_BIG_{n} (\d+)", text).group(1)) for n in ("OX", "OY"))
    val = lambda k: sum(limb << (16 * i) for i, limb in enumerate(bigs[16 * k:16 * k + 16]))  # noqa: E731
    assert (val(ox), val(oy)) == O and (O[1] ** 2 - O[0] ** 3 - 7) % P == 0


@pytest.mark.parametrize("name", sorted(CRAFTED))
def test_crafted_request_is_a_valid_signature_without_a_witness(oracle, name):
    """no GPU: the precompile recovers an address (the signature is fine, it is the circuit's addition that is incomplete), the chain meets
    x1 == x2 where the construction says, and the oracle's own evaluator reports no witness"""
    crafted, where = CRAFTED[name]
    ok, addr = ec.ecrecover(*crafted)
    assert ok == 1 and 0 < addr < 1 << 160
    assert _first_meeting(*crafted) == where
    with pytest.raises(RuntimeError, match="no witness"):
        oracle.ec_eval_cycle(oracle.ec_inputs(*crafted))


@pytest.fixture(scope="module")
def ctx():
    from era_zkevm_test_harness_amd import native

    c = native.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def trace(ctx):
    from era_zkevm_test_harness_amd import native

    t = native.Trace(ctx, N_ROWS, 3, n_cols=native.EK_COLS)
    yield t
    t.free()


def _witness(ctx, oracle, requests, seed):
    """a witness (library and oracle) whose requests are the given (h, v, r, s), written values as the precompile computes them"""
    from era_zkevm_test_harness_amd import native

    req, mq = synthetic.precompile_trace(2, len(requests), seed=seed)
    for k, c in enumerate(requests):
        for j, val in enumerate(tuple(c) + ec.ecrecover(*c)):
            mq["value"][6 * k + j] = np.frombuffer(int(val).to_bytes(32, "little"), "<u4")
    tails = oracle.queue_push_chain_log(oracle.encode_log_queries(req))[1]
    mem_in = np.zeros(1, native.QUEUE_STATE12)
    return ctx._precompile(2, req, tails, mq, CAP, mem_in), oracle.precompile_build(2, req, tails, mq, CAP, mem_in)


def _requests_of(mq, n):
    return [tuple(int.from_bytes(np.ascontiguousarray(mq["value"][6 * k + j]).tobytes(), "little") for j in range(4)) for k in range(n)]


@pytest.fixture(scope="module")
def valid(ctx, oracle):
    """four valid requests (two instances), the oracle's traces of them computed once: the call that follows every refusal"""
    _req, mq = synthetic.precompile_trace(2, 4, seed=3)
    requests = _requests_of(mq, 4)
    w, o = _witness(ctx, oracle, requests, seed=3)
    assert w.num_instances == 2
    exp = [oracle.ecrecover_synthesize(o, i, CAP, N_ROWS) for i in range(2)]
    yield requests, w, exp
    w.free()


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CRAFTED))
def test_request_without_a_witness_is_refused_and_the_next_call_is_exact(ctx, oracle, trace, valid, name):
    from era_zkevm_test_harness_amd import native

    crafted, _where = CRAFTED[name]
    with pytest.raises(RuntimeError, match="no witness"):  # the oracle's own evaluator (the rest of the construction: the CPU test above)
        oracle.ec_eval_cycle(oracle.ec_inputs(*crafted))
    requests, w_valid, exp = valid
    assert all(_first_meeting(*c) is None for c in requests if ec.ecrecover(*c)[0])
    # the crafted request as cycle 1 of instance 1; with another crafted one before it the kernels keep the highest flagged request
    batch = list(requests)
    batch[3] = crafted
    if name.startswith("b_"):
        batch[1] = CRAFTED["a_first_step_equal"][0]
    w, _o = _witness(ctx, oracle, batch, seed=3)
    with pytest.raises(native.ZkwError) as ei:
        ctx.synthesize_ecrecover(w, trace, 0, 2, 0)
    assert ei.value.code == native.ERR_CHECK_FAILED
    assert "request 3 (instance 1 of the call) has no witness" in str(ei.value), str(ei.value)
    w.free()
    # the same context and trace, a call of valid requests: cell for cell the oracle's, and satisfied
    ctx.synthesize_ecrecover(w_valid, trace, 0, 2, 0)
    for i in range(2):
        got = trace.get(i)
        assert np.array_equal(got, exp[i]), np.argwhere(got != exp[i])[:4]
        assert ctx.check_if_satisfied_ecrecover(trace, i, CAP) == (0, (0, 0, 0))


@pytest.mark.gpu
def test_scalars_at_the_chain_edges(ctx, oracle, trace):
    """valid requests whose scalars sit at the ends of the chain: u2 = 1 (255 doublings before the only addition), n - 1, 2^255 (one addition, at
    the first step); u1 with every byte non-zero (32 table additions) and with only byte 31 non-zero. Trace == oracle cell for cell, the address
    the trace writes == secp256k1.ecrecover"""
    R = ec.mul(0x1F2E3D4C5B6A79880796A5B4C3D2E1F00F1E2D3C4B5A69788796A5B4C3D2E1F0 % N, ec.G)
    u_any = 0x243F6A8885A308D313198A2E03707344A4093822299F31D0082EFA98EC4E6C89 % N
    all_bytes = int.from_bytes(bytes(range(1, 33)), "little")
    scalars = [(1, u_any), (N - 1, u_any), (1 << 255, u_any), (u_any, all_bytes), (u_any, 0xC3 << 248)]
    assert all(0 < u2 < N and 0 < u1 < N for u2, u1 in scalars) and all((all_bytes >> (8 * c)) & 0xFF for c in range(32))
    requests = [_request(R, u2, u1=u1) for u2, u1 in scalars]
    want = [ec.ecrecover(*c) for c in requests]
    assert all(ok == 1 for ok, _a in want) and all(_first_meeting(*c) is None for c in requests)
    w, o = _witness(ctx, oracle, requests, seed=17)
    ni = w.num_instances
    assert ni == 3
    ctx.synthesize_ecrecover(w, trace, 0, ni, 0)
    for i in range(ni):
        got = trace.get(i)
        exp = oracle.ecrecover_synthesize(o, i, CAP, N_ROWS)
        assert np.array_equal(got, exp), np.argwhere(got != exp)[:4]
        assert ctx.check_if_satisfied_ecrecover(trace, i, CAP) == (0, (0, 0, 0))
        for c in range(min(CAP, len(requests) - CAP * i)):  # the value bytes of the cycle's two writes (queue section)
            okc = [got[oracle.nlq_cell(7, CAP, c, 5, -1, 0, 6 + b)] for b in range(32)]
            adc = [got[oracle.nlq_cell(7, CAP, c, 6, -1, 0, 6 + b)] for b in range(32)]
            assert (int.from_bytes(bytes(int(b) for b in okc), "little"), int.from_bytes(bytes(int(b) for b in adc), "little")) == want[CAP * i + c]
    w.free()
