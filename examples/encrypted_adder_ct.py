"""Add two encrypted 16-bit numbers with RLWE ciphertexts in and out (sgfhe_circuit_run_ct): the reference's
flow  encrypt -> split_ciphertext -> gates -> pack_encrypted_bits -> decrypt  with the split and the pack done on
the device inside one circuit run.  A ciphertext holds n bits, so it is one wire of the adder over n instances:
bit i of x for n different x.  32 ciphertexts go in, 17 come out.
Run on a GPU box:  python examples/encrypted_adder_ct.py [bits] [n] [blocks] [--direct]
--direct packs the sums straight from the gates' LWEs over Z_Q (SGFHE_CIRCUIT_PACK_DIRECT): no refresh bootstraps."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from encrypted_adder import adder_circuit  # noqa: E402


def main(bits=16, n=64, blocks=1, direct=False):
    import sgfhe_jl_amd as S
    rng = np.random.default_rng()
    params = S.Params(n)
    key = S.PrivateKey(params, rng)
    bkey = S.BootstrapKey(rng, key)
    inst = blocks * n
    xs = rng.integers(0, 1 << bits, size=inst)
    ys = rng.integers(0, 1 << bits, size=inst)
    plain = np.array([(xs >> i) & 1 for i in range(bits)] + [(ys >> i) & 1 for i in range(bits)], dtype=bool)
    cts = [[S.encrypt(key, rng, plain[i, t * n:(t + 1) * n]) for t in range(blocks)] for i in range(2 * bits)]
    circ = adder_circuit(S, bits)
    info = circ.info()
    t0 = time.time()
    outs = S.evaluate_circuit_ct(bkey, None, circ, cts, direct=direct)
    dt = time.time() - t0
    sums = np.zeros(inst, dtype=np.int64)
    for i, row in enumerate(outs):
        sums += np.concatenate([S.decrypt(key, ct) for ct in row]).astype(np.int64) << i
    assert np.array_equal(sums, xs + ys), "wrong sums"
    boots = (info["nodes"] + (0 if direct else circ.n_outputs)) * inst    # (every sum bit is a gate wire)
    print("%d-bit adder at Params(%d), %d ciphertexts in, %d out, %d instances: %d levels, %d bootstraps "
          "(gates + pack), %.2f s; all %d sums correct"
          % (bits, n, 2 * bits * blocks, circ.n_outputs * blocks, inst, info["levels"], boots, dt, inst))


if __name__ == "__main__":
    a = [int(v) for v in sys.argv[1:] if v != "--direct"]
    main(*a[:3], direct="--direct" in sys.argv[1:])
