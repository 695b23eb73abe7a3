"""Add two encrypted 16-bit numbers over many independent instances with one circuit run
(sgfhe_circuit_run): a ripple-carry adder of 3 nodes per bit -- (a, b) -> AND, XOR; (p, c) -> AND, XOR;
(g, t) -> OR -- evaluated level by level on the device, every level one wide bootstrap call.
Run on a GPU box:  python examples/encrypted_adder.py [bits] [instances]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def adder_circuit(S, bits):
    """Inputs x_0 .. x_{bits-1}, y_0 .. y_{bits-1} (least significant first); outputs the bits + 1 bits of
    the sum.  Bit 0 takes the constant FALSE as its carry in."""
    c = S.Circuit(2 * bits)
    carry = S.Circuit.FALSE
    outs = []
    for i in range(bits):
        g, _, p = c.gate(c.inputs[i], c.inputs[bits + i])       # generate, propagate
        t, _, s = c.gate(p, carry)
        outs.append(s)
        _, carry, _ = c.gate(g, t)
    c.output(*outs, carry)
    return c


def encrypt_bits(S, key, rng, bits):
    """EncryptedBits of a flat bool array, n at a time through one RLWE encryption each."""
    n = key.params.n
    out = []
    for i in range(0, len(bits), n):
        chunk = np.zeros(n, dtype=bool)
        chunk[:len(bits[i:i + n])] = bits[i:i + n]
        out.extend(S.split_ciphertext(S.encrypt(key, rng, chunk))[:len(bits[i:i + n])])
    return out


def main(bits=16, instances=256):
    import sgfhe_jl_amd as S
    rng = np.random.default_rng()
    params = S.Params(1024)
    key = S.PrivateKey(params, rng)
    bkey = S.BootstrapKey(rng, key)
    xs = rng.integers(0, 1 << bits, size=instances)
    ys = rng.integers(0, 1 << bits, size=instances)
    plain = np.array([(xs >> i) & 1 for i in range(bits)] + [(ys >> i) & 1 for i in range(bits)], dtype=bool)
    enc = encrypt_bits(S, key, rng, plain.reshape(-1))
    inputs = [enc[i * instances:(i + 1) * instances] for i in range(2 * bits)]
    circ = adder_circuit(S, bits)
    info = circ.info()
    t0 = time.time()
    outs = S.evaluate_circuit(bkey, None, circ, inputs)
    dt = time.time() - t0
    sums = np.zeros(instances, dtype=np.int64)
    for i, row in enumerate(outs):
        sums += np.array([S.decrypt(key, e) for e in row], dtype=np.int64) << i
    assert np.array_equal(sums, xs + ys), "wrong sums"
    print("%d-bit adder x %d instances: %d levels, %d gates, %.2f s (%.0f gates/s); all %d sums correct"
          % (bits, instances, info["levels"], info["nodes"] * instances, dt, info["nodes"] * instances / dt, instances))


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 16, int(sys.argv[2]) if len(sys.argv) > 2 else 256)
