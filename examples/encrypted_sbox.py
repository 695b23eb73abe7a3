"""A 3-bit S-box on encrypted bits with ONE bootstrap per output bit.  A gate bootstrap separates four phases, so only
threshold functions of a sum of wires come out of it; a LUT node (Circuit.lut, sgfhe_circuit_create_lut) sums its three
inputs at the codewords Dr/4, Dr/2 and Dr -- eight phases in one half period -- and evaluates ANY 8-entry truth table.
The S-box is given as a table; its three output bits are three LUT nodes on the fanned inputs (Circuit.fan brings a wire
to all three scales in one bootstrap).  Fresh encryptions are refreshed first: the inputs of a LUT node must be
bootstrapped wires (the noise rule in include/sgfhe_hip.h).  The count is printed beside that of the same S-box from
two-input gates -- each output bit as a multiplexer on x2 of two functions of (x0, x1).
Run on a GPU box:  python examples/encrypted_sbox.py [blocks]
RLWE ciphertexts in and out (evaluate_circuit_ct): ciphertext i holds bit i of n = 1024 S-box inputs per block."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SBOX = (0, 1, 3, 6, 7, 4, 5, 2)       # a 3-bit permutation: SBOX[x0 + 2 x1 + 4 x2]


def truth_table(bit):
    """The 8-entry table of output bit `bit`: bit s of it is that bit of SBOX[s]."""
    return sum(((SBOX[s] >> bit) & 1) << s for s in range(8))


def lut_sbox(S):
    c = S.Circuit(3)
    f = [c.fan(c.refresh(w)) for w in c.inputs]
    c.output(*[c.lut(truth_table(k), f[0][2], f[1][1], f[2][0])[0] for k in range(3)])
    return c


def two_input(c, table4, x0, x1):
    """Any function of two bits (bit x0 + 2 x1 of table4) from at most one gate and NOTs."""
    T, F = c.TRUE, c.FALSE
    for neg in (False, True):
        t = table4 ^ 0xF if neg else table4
        inv = (lambda w: ~w) if neg else (lambda w: w)
        if t == 0x0:
            return inv(F)
        if t == 0xA:
            return inv(x0)
        if t == 0xC:
            return inv(x1)
        if t == 0x6:
            return inv(c.gate(x0, x1)[2])
        for a0 in (False, True):
            for a1 in (False, True):     # AND of the two literals
                if t == sum(((((s & 1) ^ a0) & ((s >> 1) ^ a1)) & 1) << s for s in range(4)):
                    return inv(c.gate(~x0 if a0 else x0, ~x1 if a1 else x1)[0])
    raise AssertionError(table4)


def gate_sbox(S):
    c = S.Circuit(3)
    x0, x1, x2 = c.inputs
    outs = []
    for k in range(3):
        t = truth_table(k)
        lo, hi = two_input(c, t & 0xF, x0, x1), two_input(c, t >> 4, x0, x1)
        outs.append(c.gate(c.gate(~x2, lo)[0], c.gate(x2, hi)[0])[1])
    c.output(*outs)
    return c


def main(blocks=1):
    import sgfhe_jl_amd as S
    rng = np.random.default_rng()
    params = S.Params(1024)
    n = params.n
    key = S.PrivateKey(params, rng)
    bkey = S.BootstrapKey(rng, key)
    inst = blocks * n
    x = rng.integers(0, 8, size=inst)
    x[:8] = np.arange(8)
    plain = np.stack([(x >> i) & 1 for i in range(3)]).astype(bool)
    cts = [[S.encrypt(key, rng, plain[i, t * n:(t + 1) * n]) for t in range(blocks)] for i in range(3)]
    want = np.array(SBOX)[x]
    for name, circ in (("LUT nodes", lut_sbox(S)), ("two-input gates", gate_sbox(S))):
        assert np.array_equal(circ.evaluate_plain(plain), np.stack([(want >> k) & 1 for k in range(3)]).astype(bool))
        info = circ.info()
        t0 = time.time()
        outs = S.evaluate_circuit_ct(bkey, None, circ, cts)
        dt = time.time() - t0
        got = sum(np.concatenate([S.decrypt(key, ct) for ct in row]).astype(np.int64) << k for k, row in enumerate(outs))
        assert np.array_equal(got, want), "wrong S-box outputs (%s)" % name
        print("3-bit S-box of %d encrypted inputs at Params(1024) from %s: %d levels, %d bootstraps per input (+ %d in the "
              "pack stage), %.2f s; all %d outputs equal the table"
              % (inst, name, info["levels"], info["nodes"], circ.n_outputs, dt, inst))


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 1)
