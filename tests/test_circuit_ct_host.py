"""sgfhe_circuit_run_ct (include/sgfhe_hip.h) without a device: the export and its
declaration, and the host composition `circuit.replay_ct` that the GPU tests and tools/circuit_bench.py compare
the device run with -- the block / bit -> instance mapping, the grouping of the pack calls, the call numbers,
and the split of both ciphertext lengths against the C host plumbing."""

import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_export_declaration_and_null_ctx(S):
    L = S.lib()
    assert "sgfhe_circuit_run_ct" in S.EXPORTED_SYMBOLS and hasattr(L, "sgfhe_circuit_run_ct")
    hdr = open(os.path.join(ROOT, "include", "sgfhe_hip.h")).read()
    m = re.search(r"int32_t\s+sgfhe_circuit_run_ct\s*\(([^)]*)\)\s*;", hdr)
    assert m, "the header does not declare sgfhe_circuit_run_ct"
    assert len(m.group(1).split(",")) == 9
    assert len(L.sgfhe_circuit_run_ct.argtypes) == 9
    assert L.sgfhe_abi_version() == 7          # functions are only added
    c = S.Circuit(1)
    c.output(c.inputs[0])
    buf = np.zeros(64, dtype=np.uint64)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    assert L.sgfhe_circuit_run_ct(None, c.handle(), 1, p, p, 64, p, p, None) == -1


class _P:
    """The fields of Params the composition reads (n = 2048 without building that parameter set)."""

    def __init__(self, n):
        self.n, self.r, self.m = n, 16 * n, 8 * n


def _standins(n, m, log):
    def boot(call, a1, b1, a2, b2):
        log.append(("boot", call, len(b1)))
        out = np.zeros((len(b1), 3, n + 1), dtype=np.uint64)
        out[:, 0] = np.concatenate([a1, b1[:, None]], axis=1)                   # "AND" = x
        out[:, 1] = np.concatenate([a2, b2[:, None]], axis=1)                   # "OR"  = y
        out[:, 2, :n], out[:, 2, n] = a1 + a2, b1 + b2                          # "XOR" = x + y
        return out

    def pack(call, a, b):
        assert a.shape == (len(b), n, n) and b.shape == (len(b), n)
        log.append(("pack", call, len(b)))
        w = np.zeros((len(b), m), dtype=np.uint64)
        v = np.zeros((len(b), m), dtype=np.uint64)
        w[:, :n], w[:, n] = a[:, :, 0], call           # word 0 of every LWE of the group, and the call
        v[:, :n], v[:, n] = b, np.arange(len(b))       # the b words, and the index within the call
        return w, v
    return boot, pack


def test_replay_ct_mapping_and_split_both_lengths(S):
    from sgfhe_jl_amd import circuit as C
    params = S.Params(64)
    n, m, r = params.n, params.m, params.r
    rng = np.random.default_rng(5)
    c = S.Circuit(2)
    x, y = c.inputs
    g = c.gate(x, y)
    c.output(x, ~y, g[2])
    blocks = 3
    for N in (n, m):
        a = rng.integers(0, r, size=(2, blocks, N), dtype=np.uint64)
        a[0, 0, 0] = 0                                              # -0 mod r
        b = rng.integers(0, r, size=(2, blocks, N), dtype=np.uint64)
        log = []
        boot, pack = _standins(n, m, log)
        (w, v), lwe = C.replay_ct(c, a, b, params, boot, pack)
        assert lwe.shape == (3, blocks * n, n + 1) and w.shape == v.shape == (3, blocks, m)
        # instance block * n + i is bit i of the block's ciphertext: the C split, both lengths
        for i in range(2):
            for t in range(blocks):
                la, lb = S.host.split_ciphertext(params, a[i, t], b[i, t])
                want = np.concatenate([la, lb[:, None]], axis=1)
                got = lwe[i, t * n:(t + 1) * n]
                assert np.array_equal(got if i == 0 else C.lwe_not(got, r), want), (N, i, t)
                # and the reference's extract, bit by bit (1-based)
                assert np.array_equal(want[5, :n], S.extract(a[i, t], 6, n) & np.uint64(r - 1))
        assert np.array_equal(lwe[2, :, n], (b[0, :, :n] + b[1, :, :n]).reshape(-1))
        # one level of blocks * n rows, then one pack call of all 9 ciphertexts (cpc = 128), numbered after it
        assert log == [("boot", 0, blocks * n), ("pack", 1, 9)]
        # ciphertext q = output * blocks + block holds the n LWEs of that output over the block
        assert np.array_equal(v[:, :, :n].reshape(3, blocks * n), lwe[:, :, n])
        assert np.array_equal(w[:, :, :n].reshape(3, blocks * n), lwe[:, :, 0])
        assert np.array_equal(v[:, :, n].reshape(-1), np.arange(9))


def test_replay_ct_pack_call_grouping(S):
    from sgfhe_jl_amd import circuit as C
    assert C.pack_calls(64) == 128 and C.pack_calls(1024) == 8 and C.pack_calls(2048) == 4
    assert C.pack_calls(16384) == 1
    # n = 64: 70 outputs x 2 blocks = 140 ciphertexts = calls of 128 and 12, after the two levels' calls
    params = S.Params(64)
    n, m = params.n, params.m
    c = S.Circuit(2)
    x, y = c.inputs
    g1 = c.gate(x, y)
    g2 = c.gate(g1[0], ~g1[2])
    c.output(*([g2[0], g2[1], ~g2[2], x, S.Circuit.TRUE] * 14))
    rng = np.random.default_rng(6)
    a = rng.integers(0, params.r, size=(2, 2, n), dtype=np.uint64)
    b = rng.integers(0, params.r, size=(2, 2, n), dtype=np.uint64)
    log = []
    (w, v), lwe = C.replay_ct(c, a, b, params, *_standins(n, m, log))
    assert log == [("boot", 0, 2 * n), ("boot", 1, 2 * n), ("pack", 2, 128), ("pack", 3, 12)]
    q = np.arange(140)
    assert np.array_equal(w.reshape(140, m)[:, n], 2 + q // 128)
    assert np.array_equal(v.reshape(140, m)[:, n], q % 128)
    # n = 2048: 4 ciphertexts per call; 3 outputs x 3 blocks = calls of 4, 4 and 1
    p2 = _P(2048)
    c2 = S.Circuit(1)
    c2.output(c2.inputs[0], ~c2.inputs[0], S.Circuit.FALSE)
    a = rng.integers(0, p2.r, size=(1, 3, p2.n), dtype=np.uint64)
    b = rng.integers(0, p2.r, size=(1, 3, p2.n), dtype=np.uint64)
    log = []
    (w, v), lwe = C.replay_ct(c2, a, b, p2, *_standins(p2.n, p2.m, log))
    assert log == [("pack", 0, 4), ("pack", 1, 4), ("pack", 2, 1)]      # no level: the pack calls start at 0
    assert np.array_equal(lwe[2], np.zeros_like(lwe[2]))
    assert np.array_equal(v[0, :, :p2.n], b[0])


def test_evaluate_circuit_ct_checks_its_inputs(S):
    params = S.Params(64)
    c = S.Circuit(2)
    c.output(*c.gate(*c.inputs))
    z = np.zeros(params.n, dtype=np.uint64)
    pc = S.PackedCiphertext(params, S.RLWE(z, z))
    ct = S.Ciphertext(params, S.RLWE(np.zeros(params.m, dtype=np.uint64), np.zeros(params.m, dtype=np.uint64)))

    class Key:
        pass
    k = Key()
    k.params = params
    with pytest.raises(ValueError):
        S.evaluate_circuit_ct(k, None, c, [[pc]])                       # one row per input
    with pytest.raises(ValueError):
        S.evaluate_circuit_ct(k, None, c, [[pc, pc], [pc]])             # ragged
    with pytest.raises(TypeError):
        S.evaluate_circuit_ct(k, None, c, [[pc], [ct]])                 # one kind
