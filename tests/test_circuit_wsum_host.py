"""Weighted-sum nodes (sgfhe_circuit_create_w, include/sgfhe_hip.h) without a device: the
planner's validation through ctypes, a sgfhe_circuit_create3 plan restated in the CSR form, Circuit.sum_node against
the mod-4 formula, xor / gf2_matvec / crc16_ccitt against numpy and binascii, the planner with circuit_plain_bits under
ASan / UBSan (tests/native/circuit_wsum_sanitized.cpp), and a sum-node circuit on the C oracle at Params(64)."""

import binascii
import ctypes
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

import wsum_ref as WR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID_ARG = -1
NONE = 0x7FFFFFFE
FALSE = 0x7FFFFFFF
NOT = 0x80000000


def _p(x):
    return None if x is None else x.ctypes.data_as(ctypes.c_void_p)


def _create_w(L, n_inputs, nodes, outs, oshift, group, start=None, shifts=True):
    """nodes: [(kind, [(weight, ref, shift), ...])]."""
    kind = np.array([k for k, _ in nodes], dtype=np.uint32)
    st = np.cumsum([0] + [len(t) for _, t in nodes]).astype(np.uint32) if start is None else np.array(start, dtype=np.uint32)
    tw = np.array([w for _, t in nodes for w, _, _ in t], dtype=np.int32)
    tr = np.array([r for _, t in nodes for _, r, _ in t], dtype=np.uint32)
    ts = np.array([d for _, t in nodes for _, _, d in t], dtype=np.int32) if shifts else None
    o = np.array(outs, dtype=np.uint32)
    os_ = None if oshift is None else np.array(oshift, dtype=np.int32)
    h = ctypes.c_void_p(0xDEAD)
    rc = L.sgfhe_circuit_create_w(n_inputs, _p(kind), _p(st), _p(tr), _p(ts), _p(tw), len(nodes), _p(o), _p(os_), len(o),
                                  group, ctypes.byref(h))
    return rc, h


def _info(L, h):
    info = (ctypes.c_uint64 * 4)()
    assert L.sgfhe_circuit_info(h, info) == 0
    return list(info)


def test_create_w_validation(S):
    L = S.lib()
    assert "sgfhe_circuit_create_w" in S.EXPORTED_SYMBOLS
    assert L.sgfhe_abi_version() == 7          # functions are only added
    hdr = open(os.path.join(ROOT, "include", "sgfhe_hip.h")).read()
    assert "#define SGFHE_CIRCUIT_MAX_TERMS 64u" in hdr
    # 2 inputs; node 0 classic (0, 1), node 1 = 2 AND(0) + in0 - ~XOR(0): wires 2..4 and 5..7
    def good(w=1, ref=0, d=0, kind0=0, w0=1, extra0=()):
        return [(kind0, [(w0, 0, 0), (1, 1, 0)] + list(extra0)), (1, [(2, 2, 0), (w, ref, d), (-1, NOT | 4, 0)])]
    outs = [5, NOT | 7, 0]

    def refused(nodes, outputs=outs, oshift=None, group=8, **kw):
        rc, h = _create_w(L, 2, nodes, outputs, oshift, group, **kw)
        assert rc == ERR_INVALID_ARG and h.value is None, (nodes, outputs, oshift, group, kw)

    for w in (0, 3, -3, 2 ** 31 - 1, -2 ** 31):
        refused(good(w=w))
    refused([(0, [(1, 0, 0), (1, 1, 0)]), (1, [])])                                   # a sum node with 0 terms
    refused([(0, [(1, 0, 0), (1, 1, 0)]), (1, [(2, 0, 0)] * 65)])                      # ... with 65
    refused(good(), start=[0, 5, 2])                                                   # decreasing node_start
    refused(good(), start=[1, 2, 5])                                                   # node_start[0] != 0
    refused(good(extra0=[(1, 0, 0)]))                                                  # a classic node with three terms
    refused([(0, [(1, 0, 0)]), (1, [(2, 0, 0)])])                                      # ... with one
    refused(good(w0=2))                                                                # ... with a weight of 2
    refused(good(w0=-1))
    refused([(2, [(1, 0, 0), (1, 1, 0)]), (1, [(2, 0, 0)])])                           # node_kind above 1
    refused(good(ref=NONE))                                                            # NONE as a term
    refused(good(ref=NOT | NONE))
    refused(good(ref=5))                                                               # a term naming its own node
    refused(good(ref=8))                                                               # ... no wire at all
    refused([(1, [(1, 0, 0), (1, 5, 0)]), (1, [(2, 0, 0)])])                           # ... a later node
    refused(good(), outputs=[5, NONE, 0])
    for d in (8, -8, 2 ** 31 - 1, -2 ** 31):                                           # |shift| >= group
        refused(good(d=d))
        refused(good(), oshift=[0, d, 0])
    refused(good(d=1), group=1)                                                        # group = 1 admits no shift but 0
    refused(good(), group=0)
    refused(good(), outputs=[])
    assert L.sgfhe_circuit_create_w(2, None, None, None, None, None, 0, None, None, 0, 1, None) == ERR_INVALID_ARG
    # accepted: 64 terms of the largest weights and shifts, one term, NULL shifts, constants with a shift
    wide = [(0, [(1, 0, 0), (1, 1, 0)]),
            (1, [((-2, 2)[i % 2], (2, 3, 4, 0, 1, NOT | FALSE)[i % 6], (7, -7)[i % 2]) for i in range(64)])]
    for nodes, group, kw in ((good(), 1, {}), (good(d=7), 8, {}), (good(d=-7), 8, {}), (good(), 8, dict(shifts=False)),
                             (wide, 8, {}), (good(w=-2, ref=NOT | FALSE, d=3), 4, {})):
        rc, h = _create_w(L, 2, nodes, outs, None, group, **kw)
        assert rc == 0 and h.value, (nodes, group)
        assert _info(L, h)[:3] == [2, 2, 1]
        g = ctypes.c_uint32(0)
        assert L.sgfhe_circuit_group(h, ctypes.byref(g)) == 0 and g.value == group
        L.sgfhe_circuit_destroy(h)
    rc, h = _create_w(L, 2, [(1, [(1, 0, 0)]), (1, [(2, 3, 0)])], [5], None, 1)       # refresh, then a one-term parity
    assert rc == 0 and _info(L, h)[:3] == [2, 2, 1]
    L.sgfhe_circuit_destroy(h)


def test_create3_plan_restated_through_create_w(S):
    """The arrays of a sgfhe_circuit_create3 plan in the CSR form -- classic nodes stay classic, three-input nodes
    become three unit-weight terms: the same sgfhe_circuit_info and group."""
    L = S.lib()
    rng = np.random.default_rng(11)
    for n_gates, group in ((1, 1), (9, 1), (40, 1), (25, 8)):
        def shift():
            return int(rng.integers(-(group - 1), group))

        def ref(g):
            return (FALSE if rng.integers(9) == 0 else int(rng.integers(3 + 3 * g))) | (NOT if rng.integers(2) else 0)
        gates = [(ref(g), ref(g), NONE if rng.integers(3) == 0 else ref(g)) for g in range(n_gates)]
        gsh = [(shift(), shift(), shift()) for _ in range(n_gates)]
        outs = [3 + 3 * n_gates - 1, NOT | 1, FALSE, 3 + int(rng.integers(3 * n_gates))]
        osh = [shift() for _ in outs]
        g3 = np.array(gates, dtype=np.uint32)
        s3 = np.array(gsh, dtype=np.int32)
        o = np.array(outs, dtype=np.uint32)
        os_ = np.array(osh, dtype=np.int32)
        h0 = ctypes.c_void_p()
        assert L.sgfhe_circuit_create3(3, _p(g3), _p(s3), n_gates, _p(o), _p(os_), len(outs), group, ctypes.byref(h0)) == 0
        nodes = [(int(z != NONE), [(1, r, d) for r, d in zip(gate, sh) if r != NONE]) for gate, sh, z in
                 ((gate, sh, gate[2]) for gate, sh in zip(gates, gsh))]
        rc, h1 = _create_w(L, 3, nodes, outs, osh, group)
        assert rc == 0 and _info(L, h1) == _info(L, h0)
        grp = ctypes.c_uint32()
        assert L.sgfhe_circuit_group(h1, ctypes.byref(grp)) == 0 and grp.value == group
        L.sgfhe_circuit_destroy(h1)
        L.sgfhe_circuit_destroy(h0)


@pytest.mark.parametrize("k", [1, 2, 3])
def test_evaluate_plain_is_the_mod4_formula(S, k):
    """Every weight tuple in {-2, -1, 1, 2}^k over all input patterns x all NOT patterns: HI = s in {2, 3},
    MID = s in {1, 2}, LOW = s mod 2 with s = the sum of w x mod 4, worked out here in plain integers."""
    bits = np.array(list(itertools.product([0, 1], repeat=k)), dtype=bool).T              # [k][2^k]
    for weights in itertools.product([-2, -1, 1, 2], repeat=k):
        c = S.Circuit(k)
        outs = []
        for pat in range(2 ** k):
            outs.extend(c.sum_node([(w, ~x if pat >> i & 1 else x) for i, (w, x) in enumerate(zip(weights, c.inputs))]))
        c.output(*outs)
        got = c.evaluate_plain(bits)
        for pat in range(2 ** k):
            for t in range(2 ** k):
                s = sum(w * (int(bits[i, t]) ^ (pat >> i & 1)) for i, w in enumerate(weights)) % 4
                assert tuple(got[3 * pat:3 * pat + 3, t]) == (s in (2, 3), s in (1, 2), s % 2 == 1), (weights, pat, t)
        assert c.info()["nodes"] == 2 ** k and c.schedule() == [list(range(2 ** k))]
        # the entry point: create_w only when create3 cannot say it
        assert c.has_wsum == (not (k in (2, 3) and set(weights) == {1}))
    # TRUE with weight c adds c: 2 TRUE + x has HI = 1 and LOW = x
    d = S.Circuit(1)
    d.output(*d.sum_node([(2, S.Circuit.TRUE), (1, d.inputs[0])]))
    assert np.array_equal(d.evaluate_plain([[0, 1]]), [[1, 1], [1, 0], [0, 1]])


def test_sum_node_of_unit_weights_is_gate3_in_the_model(S):
    c = S.Circuit(3, group=4)
    x, y, z = c.inputs
    ins = (x, ~y.lane(1), z.lane(-3))
    c.output(*(c.gate3(*ins) + c.sum_node([(1, w) for w in ins]) + c.sum_node([(1, x), (1, y)]) + c.gate(x, y)))
    assert not c.has_wsum and not c._wide(1) and c.kind(0) == "gate3" and c.kind(1) == "sum" and c.kind(3) == "classic"
    bits = np.random.default_rng(5).integers(0, 2, size=(3, 24)).astype(bool)
    got = c.evaluate_plain(bits)
    assert np.array_equal(got[0:3], got[3:6]) and np.array_equal(got[6:9], got[9:12])
    assert c.info() == dict(levels=1, nodes=4, widest=4, slots=15)
    with pytest.raises(ValueError):
        c.sum_node([])
    with pytest.raises(ValueError):
        c.sum_node([(2, x)] * 65)
    with pytest.raises(ValueError):
        c.sum_node([(3, x)])


def test_xor_of_1_to_16_wires(S):
    rng = np.random.default_rng(17)
    bits = rng.integers(0, 2, size=(16, 50)).astype(bool)
    for k in range(1, 17):
        c = S.Circuit(16)
        pick = [c.inputs[j] for j in rng.permutation(16)[:k]]
        neg = [~w if rng.integers(2) else w for w in pick]
        c.output(c.xor(*pick), c.xor(*neg))
        assert c.n_gates == 2 and c.info()["levels"] == 1
        want = np.bitwise_xor.reduce([bits[w.id] for w in pick])
        flips = sum(w.negated for w in neg) % 2
        got = c.evaluate_plain(bits)
        assert np.array_equal(got[0], want) and np.array_equal(got[1], want ^ bool(flips)), k
    assert S.Circuit(1).xor() == S.Circuit.FALSE


def test_gf2_matvec_against_numpy(S):
    rng = np.random.default_rng(19)
    for rows, cols in ((1, 1), (8, 8), (5, 13), (16, 64)):
        M = rng.integers(0, 2, size=(rows, cols))
        M[rows // 2] = 0                                    # an empty row: the constant FALSE
        if cols > 2:
            M[:, 2] = 0                                     # an unused input: no refresh for it
        x = rng.integers(0, 2, size=(cols, 33))
        want = (M @ x) % 2
        for refresh in (False, True):
            c = S.gf2_matvec(M, refresh_inputs=refresh)
            used = int(M.any(axis=0).sum())
            live_rows = int(M.any(axis=1).sum())
            assert c.n_gates == live_rows + (used if refresh else 0)
            assert c.info()["levels"] == ((2 if refresh else 1) if live_rows else 0)
            assert np.array_equal(c.evaluate_plain(x.astype(bool)), want.astype(bool))
    with pytest.raises(ValueError):
        S.gf2_matvec(np.ones((1, 65), dtype=int))
    with pytest.raises(ValueError):
        S.gf2_matvec([[0, 2]])


def test_crc16_ccitt_against_binascii(S):
    rng = np.random.default_rng(23)
    nbits = 32
    msgs = [bytes(4), b"\xff" * 4] + [bytes(rng.integers(0, 256, size=4).astype(np.uint8)) for _ in range(40)]
    bits = np.array([[m[j // 8] >> (7 - j % 8) & 1 for m in msgs] for j in range(nbits)], dtype=bool)
    want = [binascii.crc_hqx(m, 0) for m in msgs]
    for refresh, nodes in ((False, 16), (True, 48)):
        c = S.crc16_ccitt(nbits, refresh_inputs=refresh)
        assert c.n_inputs == 32 and c.n_outputs == 16 and c.n_gates == nodes and c.info()["nodes"] == nodes
        assert c.has_wsum and max(len(g) for g in c.gates) <= 64
        out = c.evaluate_plain(bits).astype(np.int64)
        assert list((out << np.arange(16)[:, None]).sum(axis=0)) == want
    assert S.crc16_ccitt(nbits).n_gates == 48                # refresh_inputs defaults to True


def test_wsum_planner_under_asan_and_ubsan(tmp_path):
    """tests/native/circuit_wsum_sanitized.cpp: circuit_plain_bits of plans with sum nodes of fan-in 1 to 64 and
    shifted terms against a per-instance evaluation at (G, instances) = (1, 5), (8, 72), (64, 192); the node table and its image;
    refused inputs return without allocating.  A child process of its own; the same program without the sanitizers
    compares as many bits."""
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    src = os.path.join(ROOT, "tests", "native", "circuit_wsum_sanitized.cpp")
    inc = os.path.join(ROOT, "sgfhe.jl_amd", "csrc")
    exe = str(tmp_path / "circuit_wsum_sanitized")
    b = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", "-I", inc, src, "-o", exe],
                       capture_output=True, text=True, timeout=300)
    if b.returncode != 0 and "sanitize" in b.stderr and "cannot find" in b.stderr:
        pytest.skip("the sanitizer runtimes are not installed: " + b.stderr[-300:])
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    env.pop("LD_PRELOAD", None)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    tag, compared = r.stdout.split()
    assert tag == "ok" and int(compared) > 50000
    exe2 = str(tmp_path / "circuit_wsum_plain")
    subprocess.run([gxx, "-std=c++17", "-O2", "-I", inc, src, "-o", exe2], check=True, timeout=300)
    r2 = subprocess.run([exe2], capture_output=True, text=True, timeout=300)
    assert r2.returncode == 0 and r2.stdout == r.stdout


def test_sum_nodes_on_the_c_oracle_p64(S, oc):
    """Eight inputs refreshed, their 8-term parity, and a 2x + y + z node on refreshed x and gate rows y, z, through
    replay_levels on the C oracle at Params(64), 64 instances: every output decrypts to evaluate_plain, and every node's
    input-sum error, measured with the secret key, is below Dr/2 = 128."""
    from sgfhe_jl_amd import circuit as C
    params = S.Params(64)
    o = oc.Oracle.from_params(params)
    sk = o.private_key(401)
    bkey = o.bootstrap_key(sk, 402)
    c = S.Circuit(8)
    fresh = [c.refresh(w) for w in c.inputs]
    parity = c.xor(*fresh)
    and_, or_, _ = c.gate(c.inputs[0], c.inputs[1])
    mixed = c.sum_node([(2, fresh[2]), (1, and_), (1, ~or_)])
    c.output(parity, ~parity, *mixed)
    assert c.has_wsum and c.info() == dict(levels=2, nodes=11, widest=9, slots=c.info()["slots"])
    inst = 64
    bits = np.random.default_rng(403).integers(0, 2, size=(8, inst)).astype(bool)
    bits[:, :4] = [[0, 1, 0, 1]] * 2 + [[0, 0, 1, 1]] + [[0] * 4] * 5      # s = 2x + y + z over 0 .. 3 and beyond
    a, b = o.lwe_encrypt_bits(sk, bits.reshape(-1).astype(np.uint8), 404)
    inputs = np.concatenate([a, b[:, None]], axis=1).reshape(8, inst, params.n + 1)
    boot = lambda call, a1, b1, a2, b2: o.bootstrap_batch(bkey, a1, b1, a2, b2)
    worst = WR.input_sum_errors(S, params, sk, c, inputs, bits, boot)
    print("largest input-sum error per node:", worst, "against Dr/2 =", params.Dr // 2)
    assert len(worst) == c.n_gates and max(worst.values()) < params.Dr // 2, worst
    out = C.replay_levels(c, inputs, params.r, boot)
    plain = c.evaluate_plain(bits)
    assert np.array_equal(plain[0], np.bitwise_xor.reduce(bits)) and 0 < plain[0].sum() < inst
    x, y, z = bits[2], bits[0] & bits[1], ~(bits[0] | bits[1])
    assert all(np.array_equal(p, q) for p, q in zip(plain[2:], WR.sum_node_model((2, 1, 1), (x, y, z))))
    dec = S.host.decrypt_lwe(params, sk, out[..., :params.n], out[..., params.n]).reshape(out.shape[:-1])
    assert np.array_equal(dec, plain)
