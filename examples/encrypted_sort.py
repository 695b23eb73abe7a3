"""Sort encrypted numbers that sit SIDE BY SIDE in their ciphertexts (sgfhe_circuit_create_routed): the numbers are
bit-sliced over `width` wires and every G consecutive lanes hold G numbers, which circuit.bitonic_sort(width, G) sorts
ascending -- each compare-exchange of the network reaches its partner lane t ^ k through a lane route, which costs no
bootstrap, so the only bootstraps are the comparators' MAJ chains and one LUT mux per bit and stage.
Run on a GPU box:  python examples/encrypted_sort.py [n] [width] [G] [groups | blocks] [--ct] [--masked]
Default: the LWE form, `groups` groups of G encrypted numbers (evaluate_circuit).  --ct: the ciphertext form -- `width`
ciphertexts of n bits per block go in (n / G groups each), `width` come out (evaluate_circuit_ct: split, sort and pack in
one queued run; the outputs are LUT wires, refreshed by the pack stage).  --masked: the comparators' chains carry lane
masks (sgfhe_circuit_create_masked) and bootstrap only the G / 2 lanes whose decision the swap reads: the same result in
fewer rows."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(n=64, width=3, G=8, count=2, ct=False, masked=False):
    import sgfhe_jl_amd as S
    from encrypted_adder import encrypt_bits
    rng = np.random.default_rng()
    params = S.Params(n)
    key = S.PrivateKey(params, rng)
    bkey = S.BootstrapKey(rng, key)
    circ = S.bitonic_sort(width, G, masked=masked)
    info = circ.info()
    inst = count * n if ct else count * G
    vals = rng.integers(0, 1 << width, size=inst)
    bits = [((vals >> i) & 1).astype(bool) for i in range(width)]
    if ct:
        cts = [[S.encrypt(key, rng, b.reshape(count, n)[t]) for t in range(count)] for b in bits]
        t0 = time.time()
        outs = S.evaluate_circuit_ct(bkey, None, circ, cts)
        dt = time.time() - t0
        dec = [np.concatenate([S.decrypt(key, c) for c in row]) for row in outs]
    else:
        enc = [encrypt_bits(S, key, rng, b) for b in bits]
        t0 = time.time()
        outs = S.evaluate_circuit(bkey, None, circ, enc)
        dt = time.time() - t0
        dec = [np.array([S.decrypt(key, e) for e in row]) for row in outs]
    got = sum(np.asarray(d).astype(np.int64) << i for i, d in enumerate(dec))
    want = np.sort(vals.reshape(-1, G), axis=1).reshape(-1)
    assert np.array_equal(got, want), "not sorted"
    boots = circ.rows_per_group() * (inst // G) + (width if ct else 0) * inst
    print("bitonic sort of %d groups of %d %d-bit numbers at Params(%d), %s form: %d nodes in %d levels, %d route tables, "
          "%d bootstraps = %.1f per number, %.2f s; every group sorted"
          % (inst // G, G, width, n, "ciphertext" if ct else "LWE", info["nodes"], info["levels"], len(circ.route_tables),
             boots, boots / inst, dt))
    return dt, boots, inst


if __name__ == "__main__":
    a = [int(v) for v in sys.argv[1:] if not v.startswith("--")]
    main(*a[:4], ct="--ct" in sys.argv[1:], masked="--masked" in sys.argv[1:])
