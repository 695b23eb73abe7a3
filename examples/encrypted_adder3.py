"""The 16-bit adder of examples/encrypted_adder.py from full adders of ONE bootstrap each (Circuit.full_adder,
sgfhe_circuit_create3): a three-input node bootstraps on (x + y, carry) and yields the carry MAJ as its AND row and
the sum bit XOR3 = x + y + carry - 2 MAJ without a bootstrap.  ripple_adder(16) is 16 nodes in 16 levels against
the 48 nodes and 32 levels of the two-input adder; both run here on the same inputs and both counts are printed.
Run on a GPU box:  python examples/encrypted_adder3.py [bits] [instances]
                   python examples/encrypted_adder3.py --ct [--lift] [bits] [blocks]
--ct: RLWE ciphertexts in and out (evaluate_circuit_ct; a block is n = 1024 additions).  The inputs are first passed
through an identity circuit, so that the adder gets packed Ciphertexts with the small error of a circuit's outputs,
not fresh encryptions.  --lift packs every output without a refresh bootstrap (SGFHE_CIRCUIT_PACK_LIFT): the sum bits
are XOR3 wires, which are lifted from Z_r and carry the errors of their inputs on -- hence the clean inputs -- and the
run is the 16 n level bootstraps alone instead of 33 n."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main(bits=16, instances=256):
    import sgfhe_jl_amd as S
    from encrypted_adder import adder_circuit, encrypt_bits
    rng = np.random.default_rng()
    params = S.Params(1024)
    key = S.PrivateKey(params, rng)
    bkey = S.BootstrapKey(rng, key)
    xs = rng.integers(0, 1 << bits, size=instances)
    ys = rng.integers(0, 1 << bits, size=instances)
    plain = np.array([(xs >> i) & 1 for i in range(bits)] + [(ys >> i) & 1 for i in range(bits)], dtype=bool)
    enc = encrypt_bits(S, key, rng, plain.reshape(-1))
    inputs = [enc[i * instances:(i + 1) * instances] for i in range(2 * bits)]
    for name, circ in (("two-input nodes (3 per bit)", adder_circuit(S, bits)),
                       ("full adders (1 per bit)", S.ripple_adder(bits))):
        info = circ.info()
        t0 = time.time()
        outs = S.evaluate_circuit(bkey, None, circ, inputs)
        dt = time.time() - t0
        sums = np.zeros(instances, dtype=np.int64)
        for i, row in enumerate(outs):
            sums += np.array([S.decrypt(key, e) for e in row], dtype=np.int64) << i
        assert np.array_equal(sums, xs + ys), "wrong sums"
        print("%d-bit adder x %d instances, %s: %d levels, %d bootstraps per instance, %d in all, %.2f s; all %d sums "
              "correct" % (bits, instances, name, info["levels"], info["nodes"], info["nodes"] * instances, dt, instances))


def main_ct(bits=16, blocks=1, lift=False):
    import sgfhe_jl_amd as S
    rng = np.random.default_rng()
    params = S.Params(1024)
    n = params.n
    key = S.PrivateKey(params, rng)
    bkey = S.BootstrapKey(rng, key)
    inst = blocks * n
    xs = rng.integers(0, 1 << bits, size=inst)
    ys = rng.integers(0, 1 << bits, size=inst)
    plain = np.array([(xs >> i) & 1 for i in range(bits)] + [(ys >> i) & 1 for i in range(bits)], dtype=bool)
    fresh = [[S.encrypt(key, rng, plain[i, t * n:(t + 1) * n]) for t in range(blocks)] for i in range(2 * bits)]
    ident = S.Circuit(2 * bits)
    ident.output(*ident.inputs)
    cts = S.evaluate_circuit_ct(bkey, None, ident, fresh)       # what an earlier circuit would hand on
    circ = S.ripple_adder(bits)
    info = circ.info()
    t0 = time.time()
    outs = S.evaluate_circuit_ct(bkey, None, circ, cts, lift=lift)
    dt = time.time() - t0
    sums = np.zeros(inst, dtype=np.int64)
    for i, row in enumerate(outs):
        sums += np.concatenate([S.decrypt(key, ct) for ct in row]).astype(np.int64) << i
    assert np.array_equal(sums, xs + ys), "wrong sums"
    boots = (info["nodes"] + (0 if lift else circ.n_outputs)) * inst
    print("%d-bit adder of full adders at Params(1024), %d ciphertexts in, %d out, %d instances, %s: %d levels, "
          "%d bootstraps (gates + pack), %.2f s; all %d sums correct"
          % (bits, 2 * bits * blocks, circ.n_outputs * blocks, inst, "outputs lifted" if lift else "outputs refreshed",
             info["levels"], boots, dt, inst))


if __name__ == "__main__":
    if "--ct" in sys.argv[1:]:
        a = [int(v) for v in sys.argv[1:] if not v.startswith("--")]
        main_ct(*a[:2], lift="--lift" in sys.argv[1:])
        sys.exit(0)
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 16, int(sys.argv[2]) if len(sys.argv) > 2 else 256)
