"""Two circuits back to back on one engine with the LWEs never leaving the device (Engine.circuit_run_device,
sgfhe_circuit_run_device): is z >= x + y, for encrypted 4-bit x, y, z over many instances.
  run A   the adder of examples/encrypted_adder.py: x + y as four sum wires and a carry
  glue    a public NOT of all five wires, as torch operations on the device (a -> -a, b -> Dr - b mod r)
  run B   a comparator: the carry out of z + ~sum + 1 says z >= sum, and AND ~carry says the sum fitted in four bits
Both runs and the torch kernels between them are queued on ONE torch stream, which is passed to the engine as
hip_stream: everything is in stream order, the host waits once, at the end, and decrypts once.  The same computation
through the host form (Engine.circuit_run, numpy glue) is printed beside it: the same bytes.
Run on a GPU box:  python examples/chained_circuits.py [instances] [n]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

BITS = 4


def comparator_circuit(S):
    """Inputs u_0 .. u_3, v_0 .. v_3, w: [u + v + 1 >= 16] AND w, four full adders and a gate."""
    c = S.Circuit(2 * BITS + 1)
    carry = S.Circuit.TRUE
    for i in range(BITS):
        _, carry = c.full_adder(c.inputs[i], c.inputs[BITS + i], carry)
    c.output(c.gate(carry, c.inputs[2 * BITS])[0])
    return c


def main(instances=256, n=1024):
    import torch
    import sgfhe_jl_amd as S
    from sgfhe_jl_amd.circuit import lwe_not
    from encrypted_adder import adder_circuit, encrypt_bits
    rng = np.random.default_rng()
    params = S.Params(n)
    r, Dr = params.r, params.r // 4
    key = S.PrivateKey(params, rng)
    bkey = S.BootstrapKey(rng, key)
    eng = bkey.engine
    xs, ys, zs = (rng.integers(0, 1 << BITS, size=instances) for _ in range(3))
    plain = np.array([(v >> i) & 1 for v in (xs, ys, zs) for i in range(BITS)], dtype=bool)
    enc = encrypt_bits(S, key, rng, plain.reshape(-1))
    adder, comp = adder_circuit(S, BITS), comparator_circuit(S)
    wires = np.array([[np.append(e.lwe.a, e.lwe.b) for e in enc[i * instances:(i + 1) * instances]]
                      for i in range(3 * BITS)], dtype=np.uint64)                       # [12][instances][n + 1]
    xy, z = np.ascontiguousarray(wires[:2 * BITS]), np.ascontiguousarray(wires[2 * BITS:])

    def decrypt(row):
        return np.array([S.decrypt(key, S.EncryptedBit(S.LWE(w[:n], w[n]))) for w in row], dtype=bool)

    with eng.lock:
        eng.set_random_flatten(False)
        # ---- the device-resident chain: nothing between the upload and the download touches the host
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            d_xy = torch.from_numpy(xy.view(np.int64)).cuda()
            d_z = torch.from_numpy(z.view(np.int64)).cuda()
            t0 = time.time()
            sums = eng.circuit_run_device(adder, d_xy, hip_stream=st)                   # [5][instances][n + 1]
            neg = torch.cat([(r - sums[:, :, :n]) % r, (Dr - sums[:, :, n:]) % r], dim=2)     # NOT of every wire
            d_in = torch.cat([d_z, neg]).contiguous()                                   # z, ~sum bits, ~carry
            flag = eng.circuit_run_device(comp, d_in, hip_stream=st)
            queued = time.time() - t0
        st.synchronize()
        dt_dev = time.time() - t0
        dev = flag.cpu().numpy().view(np.uint64)
        # ---- the host form: every LWE comes down and goes up again between the runs
        t0 = time.time()
        h_sums = eng.circuit_run(adder, xy)
        h_flag = eng.circuit_run(comp, np.concatenate([z, lwe_not(h_sums, r)]))
        dt_host = time.time() - t0
    got, want = decrypt(dev[0]), zs >= xs + ys
    assert np.array_equal(got, want), "wrong flags"
    assert np.array_equal(dev, h_flag), "the device-resident chain and the host form differ"
    print("z >= x + y over %d instances at Params(%d): %d + %d bootstraps per instance" %
          (instances, n, adder.info()["nodes"], comp.info()["nodes"]))
    print("  device-resident: queued in %.1f ms, done in %.2f s; %d of %d flags true, all correct" %
          (queued * 1e3, dt_dev, int(got.sum()), instances))
    print("  host form:       done in %.2f s; the same bytes" % dt_host)


if __name__ == "__main__":
    main(*(int(v) for v in sys.argv[1:3]))
