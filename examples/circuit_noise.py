"""How much decryption margin does a circuit leave?  The 16-bit adder of examples/encrypted_adder.py over a few
hundred instances with the noise probe (sgfhe_circuit_run_probe): the LWE error of EVERY wire -- read or not --
against the secret key, reduced on the device; per level the worst max |e| against Dr/4 and the wrong count.
Then one gate bootstrap left un-reduced over Z_Q, probed with sgfhe_lwe_noise (raw=True).
A diagnostic (the secret key goes to the library), as the reference's examples/errors.jl and depth.jl are.
Run on a GPU box:  python examples/circuit_noise.py [bits] [instances] [n]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from encrypted_adder import adder_circuit, encrypt_bits


def main(bits=16, instances=256, n=1024):
    import sgfhe_jl_amd as S
    rng = np.random.default_rng()
    params = S.Params(n)
    key = S.PrivateKey(params, rng)
    bkey = S.BootstrapKey(rng, key)
    xs = rng.integers(0, 1 << bits, size=instances)
    ys = rng.integers(0, 1 << bits, size=instances)
    plain = np.array([(xs >> i) & 1 for i in range(bits)] + [(ys >> i) & 1 for i in range(bits)], dtype=bool)
    enc = encrypt_bits(S, key, rng, plain.reshape(-1))
    inputs = [enc[i * instances:(i + 1) * instances] for i in range(2 * bits)]
    circ = adder_circuit(S, bits)
    outs, stats = S.probe_circuit(bkey, key, None, circ, inputs, plain)
    sums = np.zeros(instances, dtype=np.int64)
    for i, row in enumerate(outs):
        sums += np.array([S.decrypt(key, e) for e in row], dtype=np.int64) << i
    assert np.array_equal(sums, xs + ys), "wrong sums"
    report = S.noise_report(circ, stats)
    print("%d-bit adder x %d instances at Params(%d): %d wires measured, Dr/4 = %d"
          % (bits, instances, n, len(report), params.Dr // 4))
    for level in range(circ.info()["levels"] + 1):
        rows = [d for d in report if d["level"] == level]
        worst = rows[0]                                   # the report is sorted by max |e|
        print("  level %2d%s: %3d wires, worst max |e| %4d (%.2f of Dr/4; %s of %s), rms %.1f, wrong %d, past the margin %d"
              % (level, " (inputs)" if level == 0 else "", len(rows), worst["max_abs"],
                 worst["max_abs"] / (params.Dr // 4), worst["kind"],
                 "input %d" % worst["wire"] if worst["node"] is None else "node %d" % worst["node"],
                 max(d["rms"] for d in rows), sum(d["wrong"] for d in rows), sum(d["margin"] for d in rows)))
    assert all(d["wrong"] == 0 for d in report)
    # one call left over Z_Q (what sgfhe_pack_lwe_modq takes): the error against the codewords 0 and 2 DQ_tilde
    e1, e2 = enc[:instances], enc[bits * instances:(bits + 1) * instances]
    a = lambda es: np.stack([e.lwe.a for e in es])
    b = lambda es: np.array([e.lwe.b for e in es], dtype=np.uint64)
    raw = bkey.engine.bootstrap_batch(a(e1), b(e1), a(e2), b(e2), raw=True)
    x, y = plain[0], plain[bits]
    q = bkey.engine.lwe_noise(key.key, raw, np.stack([x & y, x | y, x ^ y], axis=1).reshape(-1), raw=True)
    print("un-reduced gate outputs over Z_Q: %d rows, max |e| = 2^%.1f against DQ_tilde = 2^%.1f, %d past it"
          % (q.rows, np.log2(max(q.max_abs, 1)), np.log2(params.DQ_tilde), q.wrong))


if __name__ == "__main__":
    main(*[int(v) for v in sys.argv[1:4]])
