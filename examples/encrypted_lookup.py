"""A table lookup where every instance has its OWN public table.  Instance t holds a public table T_t of 16 entries of
4 bits and an encrypted 4-bit index x_t; the result is the encrypted entry T_t[x_t].  A LUT node evaluates any function of
three bits in one bootstrap, and the k-loop of that bootstrap does not depend on the table -- so the table may be
run-time DATA that differs from instance to instance (Circuit(planes=...), sgfhe_circuit_create_data): a run brings
`data`, uint8 [planes][instances], and a data node of plane p has the truth table data[p][t] at instance t.
circuit.lookup builds the Shannon expansion with such tables: the 2 cofactors of each of the 4 output bits on
(x0, x1, x2) are 8 data tables on ONE bootstrap (a LUT family), a multiplexer on x3 per output bit follows, and
circuit.lookup_data lays the tables out as planes.  Public per-instance data costs no rows and no input positions.
Run on a GPU box:  python examples/encrypted_lookup.py [instances] [--ct] [--threshold]
  (default)     the LWE form: `instances` (at most n = 1024, default 256) encrypted indices, bit by bit
  --ct          RLWE ciphertexts in and out (evaluate_circuit_ct): ciphertext i holds bit i of n = 1024 indices
  --threshold   "x_t >= c_t" for an encrypted 8-bit x_t and a public threshold c_t of its own at every instance, as a
                chain of 8 data nodes: bit i is the node (carry, FALSE, x_i) whose table is "x_i AND carry" where bit i of
                c_t is set and "x_i OR carry" where it is not.
Fresh encryptions are refreshed first: the inputs of a LUT node must be bootstrapped wires (the noise rule in
include/sgfhe_hip.h)."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

GE_AND, GE_OR = 0xA0, 0xFA      # tables on s = carry + 4 x (position 1 is the constant): x AND carry, x OR carry


def lookup_circuit(S):
    c = S.Circuit(4, planes=8)
    c.output(*S.lookup(c, c.inputs, count=4, refresh=True))
    return c


def threshold_circuit(S, width=8):
    """x >= c, LSB first: carry_-1 = TRUE (equal so far), carry_i = x_i > c_i, or x_i == c_i and carry_(i-1)."""
    c = S.Circuit(width, planes=width)
    carry = (S.Circuit.TRUE,) * 3
    for i in range(width):
        carry = c.lut_data(i, carry[2], S.Circuit.FALSE, c.refresh(c.inputs[i]))
    c.output(carry[0])
    return c


def main(instances=256, ct=False, threshold=False):
    import sgfhe_jl_amd as S
    rng = np.random.default_rng()
    params = S.Params(1024)
    n = params.n
    inst = n if ct else instances
    if not 1 <= inst <= n:
        raise SystemExit("1 .. %d instances" % n)
    key = S.PrivateKey(params, rng)
    bkey = S.BootstrapKey(rng, key)
    if threshold:
        width = 8
        circ = threshold_circuit(S, width)
        x = rng.integers(0, 1 << width, size=inst)
        thr = rng.integers(0, 1 << width, size=inst)
        thr[:3] = (x[:3] + np.array([0, 1, -1]))[:inst]          # equal, just above, just below
        thr = np.clip(thr, 0, (1 << width) - 1)
        data = np.where((thr[None, :] >> np.arange(width)[:, None]) & 1, GE_AND, GE_OR).astype(np.uint8)
        want = (x >= thr)[None, :]
        what = "x >= c_t for %d encrypted 8-bit values, a public threshold per instance" % inst
    else:
        width = 4
        circ = lookup_circuit(S)
        x = rng.integers(0, 16, size=inst)
        x[:min(16, inst)] = np.arange(min(16, inst))
        entries = rng.integers(0, 16, size=(inst, 16))            # T_t[s]
        tables = [[sum(((int(entries[t][s]) >> f) & 1) << s for s in range(16)) for t in range(inst)] for f in range(4)]
        data = S.lookup_data(tables, 4)                           # [8 planes][instances]
        value = entries[np.arange(inst), x]
        want = np.stack([(value >> f) & 1 for f in range(4)]).astype(bool)
        what = "T_t[x_t] for %d encrypted 4-bit indices, a public 16 x 4-bit table per instance" % inst
    plain = np.stack([(x >> i) & 1 for i in range(width)]).astype(bool)
    assert np.array_equal(circ.evaluate_plain(plain, data), want)
    full = np.zeros((width, n), dtype=bool)
    full[:, :inst] = plain
    cts = [S.encrypt(key, rng, full[i]) for i in range(width)]
    info = circ.info()
    if ct:
        run = lambda: S.evaluate_circuit_ct(bkey, None, circ, [[c] for c in cts], data=data)
        run()                                                     # (buffers and the plan's tables: not timed)
        t0 = time.time()
        outs = run()
        dt = time.time() - t0
        got = np.stack([S.decrypt(key, row[0]) for row in outs])
    else:
        inputs = [S.split_ciphertext(c)[:inst] for c in cts]
        run = lambda: S.evaluate_circuit(bkey, None, circ, inputs, data=data)
        run()
        t0 = time.time()
        outs = run()
        dt = time.time() - t0
        got = np.array([[S.decrypt(key, e) for e in row] for row in outs])
    assert np.array_equal(got, want), "wrong results"
    print("%s at Params(1024), %s form: %d planes of data, %d levels, %d bootstraps per instance%s, %.2f s; all %d results "
          "are right" % (what, "ciphertext" if ct else "LWE", circ.planes, info["levels"], info["nodes"],
                         " (+ %d in the pack stage)" % circ.n_outputs if ct else "", dt, inst))


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    main(int(args[0]) if args else 256, ct="--ct" in sys.argv, threshold="--threshold" in sys.argv)
