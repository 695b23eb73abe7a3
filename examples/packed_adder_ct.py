"""Add 16-bit numbers that sit SIDE BY SIDE in one ciphertext each (sgfhe_circuit_create_lanes): a ciphertext of n
bits holds n / 16 numbers, LSB first, and circuit.packed_adder(16) -- a Kogge-Stone adder whose carries move between
bits of the same ciphertext through lane-shifted wire references -- adds two such ciphertexts word by word in one
evaluate_circuit_ct call.  2 ciphertexts go in per block, 2 come out: the sums, and the carries (bit 15 of every word
is its carry-out).  examples/encrypted_adder_ct.py is the bit-sliced form of the same work: one ciphertext per bit
position, n additions at once, 32 ciphertexts in and 17 out.
Run on a GPU box:  python examples/packed_adder_ct.py [n] [blocks] [--direct]
--direct packs the two outputs straight from the gates' LWEs over Z_Q (SGFHE_CIRCUIT_PACK_DIRECT): both are unshifted
gate wires, so no refresh bootstraps are left."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WIDTH = 16


def main(n=64, blocks=1, direct=False):
    import sgfhe_jl_amd as S
    rng = np.random.default_rng()
    params = S.Params(n)
    key = S.PrivateKey(params, rng)
    bkey = S.BootstrapKey(rng, key)
    words = blocks * n // WIDTH                  # additions in the run
    xs = rng.integers(0, 1 << WIDTH, size=words)
    ys = rng.integers(0, 1 << WIDTH, size=words)
    lanes = np.arange(WIDTH)
    plain = [((v[:, None] >> lanes) & 1).astype(bool).reshape(blocks, n) for v in (xs, ys)]
    cts = [[S.encrypt(key, rng, p[t]) for t in range(blocks)] for p in plain]
    circ = S.packed_adder(WIDTH)
    info = circ.info()
    t0 = time.time()
    sum_cts, carry_cts = S.evaluate_circuit_ct(bkey, None, circ, cts, direct=direct)
    dt = time.time() - t0
    sums = np.concatenate([S.decrypt(key, ct) for ct in sum_cts]).astype(np.int64).reshape(words, WIDTH)
    carry = np.concatenate([S.decrypt(key, ct) for ct in carry_cts]).astype(np.int64).reshape(words, WIDTH)
    total = (sums << lanes).sum(axis=1) + (carry[:, WIDTH - 1] << WIDTH)
    assert np.array_equal(total, xs + ys), "wrong sums"
    boots = (info["nodes"] + (0 if direct else circ.n_outputs)) * blocks * n
    print("%d-bit packed adder at Params(%d), %d ciphertexts in, %d out, %d additions: %d levels, %d bootstraps "
          "(gates + pack) = %.1f per addition, %.2f s; all %d sums correct"
          % (WIDTH, n, 2 * blocks, circ.n_outputs * blocks, words, info["levels"], boots, boots / words, dt, words))
    return dt, boots, words


if __name__ == "__main__":
    a = [int(v) for v in sys.argv[1:] if v != "--direct"]
    main(*a[:2], direct="--direct" in sys.argv[1:])
