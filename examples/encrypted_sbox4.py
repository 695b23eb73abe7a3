"""The 4-bit S-box of PRESENT on encrypted bits through a LUT family.  A LUT node evaluates any function of THREE bits
in one bootstrap; a function of four is a multiplexer on x3 of its two cofactors on (x0, x1, x2) (circuit.shannon).  The
S-box has four output bits, so eight cofactors -- and all eight read the same three fanned wires.  The k-loop of a LUT
bootstrap does not depend on the table: Circuit.lut_multi (sgfhe_circuit_create_lut_multi) evaluates all eight on ONE
bootstrap's accumulator, each further table costing one more extraction.  The count and the time are printed beside the
same circuit with one LUT node per cofactor.  Fresh encryptions are refreshed first: the inputs of a LUT node must be
bootstrapped wires (the noise rule in include/sgfhe_hip.h).
Run on a GPU box:  python examples/encrypted_sbox4.py [blocks]
RLWE ciphertexts in and out (evaluate_circuit_ct): ciphertext i holds bit i of n = 1024 S-box inputs per block."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SBOX = (0xC, 5, 6, 0xB, 9, 0, 0xA, 0xD, 3, 0xE, 0xF, 8, 4, 7, 1, 2)       # PRESENT: SBOX[x0 + 2 x1 + 4 x2 + 8 x3]


def truth_table(bit):
    """The 16-entry table of output bit `bit`: bit s of it is that bit of SBOX[s]."""
    return sum(((SBOX[s] >> bit) & 1) << s for s in range(16))


def sbox_circuit(S, family):
    c = S.Circuit(4)
    c.output(*S.shannon(c, [truth_table(k) for k in range(4)], c.inputs, refresh=True, family=family))
    return c


def main(blocks=1):
    import sgfhe_jl_amd as S
    rng = np.random.default_rng()
    params = S.Params(1024)
    n = params.n
    key = S.PrivateKey(params, rng)
    bkey = S.BootstrapKey(rng, key)
    inst = blocks * n
    x = rng.integers(0, 16, size=inst)
    x[:16] = np.arange(16)
    plain = np.stack([(x >> i) & 1 for i in range(4)]).astype(bool)
    cts = [[S.encrypt(key, rng, plain[i, t * n:(t + 1) * n]) for t in range(blocks)] for i in range(4)]
    want = np.array(SBOX)[x]
    for name, circ in (("one LUT family", sbox_circuit(S, True)), ("one LUT node per table", sbox_circuit(S, False))):
        assert np.array_equal(circ.evaluate_plain(plain), np.stack([(want >> k) & 1 for k in range(4)]).astype(bool))
        info = circ.info()
        S.evaluate_circuit_ct(bkey, None, circ, cts)           # (buffers and the plan's tables: not timed)
        t0 = time.time()
        outs = S.evaluate_circuit_ct(bkey, None, circ, cts)
        dt = time.time() - t0
        got = sum(np.concatenate([S.decrypt(key, ct) for ct in row]).astype(np.int64) << k for k, row in enumerate(outs))
        assert np.array_equal(got, want), "wrong S-box outputs (%s)" % name
        print("PRESENT S-box of %d encrypted inputs at Params(1024), %s: %d levels, %d bootstraps per input (+ %d in the "
              "pack stage), %.2f s; all %d outputs equal the table"
              % (inst, name, info["levels"], info["nodes"], circ.n_outputs, dt, inst))


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 1)
