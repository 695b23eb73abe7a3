"""Weighted-sum nodes at Params(1024): what fan-in does a parity node carry?

  python tools/wsum_noise.py [--instances 256] [--fan-in 8,16,32]
      the noise probe (probe_circuit) of a circuit that refreshes 32 fresh encryptions and takes the parity of the
      first 8, 16 and 32 refreshed wires in one sum node each: max |e| of the inputs, of the refreshed wires, and of
      every parity node's HI and LOW wire -- LOW = U - 2 HI carries the error of the doubled sum -- against Dr/2.
  python tools/wsum_noise.py --trace [--dir DIR]
      examples/encrypted_crc.py --direct (one block) in a child process under `rocprofv3 --kernel-trace --stats`: the
      share of k_circ_gather in the kernel time of the run."""

import argparse
import csv
import glob
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))


def probe(args):
    import sgfhe_jl_amd as S
    from encrypted_adder import encrypt_bits
    fans = [int(v) for v in args.fan_in.split(",")]
    width, inst = max(fans), args.instances
    rng = np.random.default_rng(args.seed)
    params = S.Params(1024)
    key = S.PrivateKey(params, rng)
    bkey = S.BootstrapKey(rng, key)
    c = S.Circuit(width)
    fresh = [c.refresh(w) for w in c.inputs]
    nodes = [c.sum_node([(2, w) for w in fresh[:k]]) for k in fans]
    c.output(*[w for node in nodes for w in (node[0], node[2])])
    bits = rng.integers(0, 2, size=(width, inst)).astype(bool)
    enc = encrypt_bits(S, key, rng, bits.reshape(-1))
    outs, stats = S.probe_circuit(bkey, key, None, c, [enc[i * inst:(i + 1) * inst] for i in range(width)], bits)
    dec = np.array([[S.decrypt(key, e) for e in row] for row in outs], dtype=bool)
    plain = c.evaluate_plain(bits)
    print("Params(1024), %d instances, Dr/2 = %d; decryption %s"
          % (inst, params.Dr // 2, "correct" if np.array_equal(dec, plain) else "WRONG"))
    print("  inputs (split encrypt): max |e| %d" % max(stats[i].max_abs for i in range(width)))
    mids = [stats[width + 3 * g + 1] for g in range(width)]
    print("  refreshed wires (MID of one term of weight 1): max |e| %d, rms %.1f, wrong %d"
          % (max(s.max_abs for s in mids), max((s.sum_sq / s.rows) ** 0.5 for s in mids), sum(s.wrong for s in mids)))
    for k, node in zip(fans, nodes):
        hi, low = stats[node[0].id], stats[node[2].id]
        print("  parity of %2d refreshed wires: HI max |e| %d (wrong %d); LOW max |e| %d, rms %.1f (wrong %d) = %.3f of Dr/2"
              % (k, hi.max_abs, hi.wrong, low.max_abs, (low.sum_sq / low.rows) ** 0.5, low.wrong,
                 low.max_abs / (params.Dr // 2)))


def trace(args):
    d = os.path.abspath(args.dir)
    os.makedirs(d, exist_ok=True)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "crc", "--", sys.executable,
           os.path.join(ROOT, "examples", "encrypted_crc.py"), "--direct", "1"]
    rc = subprocess.call(cmd)
    if rc:
        sys.exit("rocprofv3 run failed: %d" % rc)
    stats = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
    if not stats:
        sys.exit("no kernel_stats.csv under %s" % d)
    rows = list(csv.DictReader(open(stats[0])))
    tot = sum(float(r["TotalDurationNs"]) for r in rows)
    print("kernel time under rocprofv3: %.3f s in %d kernels" % (tot * 1e-9, len(rows)))
    for r in sorted(rows, key=lambda r: -float(r["TotalDurationNs"])):
        ns = float(r["TotalDurationNs"])
        if "k_circ" in r["Name"] or ns > 0.01 * tot:
            print("  %-60s calls %7s  total %10.3f ms  avg %9.1f us  %6.3f %%"
                  % (r["Name"][:60], r["Calls"], ns * 1e-6, float(r["AverageNs"]) * 1e-3, 100 * ns / tot))
    g = sum(float(r["TotalDurationNs"]) for r in rows if "k_circ_gather" in r["Name"])
    print("k_circ_gather: %.3f ms = %.4f %% of the kernel time" % (g * 1e-6, 100 * g / tot))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", type=int, default=256)
    ap.add_argument("--fan-in", default="8,16,32")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--dir", default="circuit_trace")
    args = ap.parse_args()
    trace(args) if args.trace else probe(args)


if __name__ == "__main__":
    main()
