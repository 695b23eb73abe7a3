"""Gate circuits on the device (sgfhe_circuit_run) against the same levels replayed through
Engine.bootstrap_batch on host arrays, at Params(1024), deterministic flatten.

  python tools/circuit_bench.py [--configs 16x256,16x1024,32x256,32x1024] [--reps 1]
      wall time of ripple-carry adders (examples/encrypted_adder.py: 3 nodes per bit) over many instances:
      gates/s of one circuit_run against the per-level replay, the two alternating in one process (the
      order swaps every repetition), with the rows of every level; both paths must give the same bytes.
  python tools/circuit_bench.py --trace [--configs 16x1024] [--dir DIR]
      the same circuit run in a child process under `rocprofv3 --kernel-trace --stats`: the share of the
      gather, scatter and collect kernels in the kernel time of the run.

Inputs are uniform words of [0, r): a bootstrap's time does not depend on what it encrypts."""

import argparse
import csv
import glob
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))


def configs(spec):
    return [tuple(int(v) for v in c.split("x")) for c in spec.split(",")]


def wall(args):
    import sgfhe_jl_amd as S
    import encrypted_adder
    from sgfhe_jl_amd import circuit as C
    params = S.Params(1024)
    eng = S.Engine(params)
    rng = np.random.default_rng(1)
    eng.generate_key(rng.integers(0, 2, size=params.n).astype(np.uint64), 2)
    print("build %s, Params(1024), deterministic flatten, call rows %d" % (eng.build_id(), C.CALL_ROWS))
    warm = encrypted_adder.adder_circuit(S, 2)
    eng.circuit_run(warm, rng.integers(0, params.r, size=(4, 64, params.n + 1), dtype=np.uint64))
    for bits, inst in configs(args.configs):
        c = encrypted_adder.adder_circuit(S, bits)
        info = c.info()
        sched = c.schedule()
        gates = info["nodes"] * inst
        inputs = rng.integers(0, params.r, size=(2 * bits, inst, params.n + 1), dtype=np.uint64)
        rows = [len(l) * inst for l in sched]
        print("\n%d-bit adder x %d instances: %d levels, %d nodes per instance, %d gates per run, %d slots; "
              "rows per level %s" % (bits, inst, info["levels"], info["nodes"], gates, info["slots"],
                                     " ".join(str(r) for r in rows)))
        for rep in range(args.reps):
            res = {}
            order = ("circuit", "replay") if rep % 2 == 0 else ("replay", "circuit")
            for what in order:
                t0 = time.perf_counter()
                if what == "circuit":
                    out = eng.circuit_run(c, inputs)
                else:
                    out = C.replay_levels(c, inputs, params.r,
                                          lambda call, a1, b1, a2, b2: eng.bootstrap_batch(a1, b1, a2, b2))
                res[what] = (time.perf_counter() - t0, out)
            same = np.array_equal(res["circuit"][1], res["replay"][1])
            tc, tr = res["circuit"][0], res["replay"][0]
            print("  rep %d (%s first): circuit_run %.3f s = %.0f gates/s | replayed levels %.3f s = %.0f gates/s | "
                  "ratio %.3f | same bytes: %s" % (rep, order[0], tc, gates / tc, tr, gates / tr, tr / tc, same))
            if not same:
                sys.exit("circuit_run and the replayed levels differ")
    eng.close()


def trace(args):
    d = os.path.abspath(args.dir)
    os.makedirs(d, exist_ok=True)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "circ", "--", sys.executable,
           os.path.abspath(__file__), "--configs", args.configs, "--reps", "1", "--circuit-only"]
    rc = subprocess.call(cmd)
    if rc:
        sys.exit("rocprofv3 run failed: %d" % rc)
    stats = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
    if not stats:
        sys.exit("no kernel_stats.csv under %s" % d)
    rows = list(csv.DictReader(open(stats[0])))
    tot = sum(float(r["TotalDurationNs"]) for r in rows)
    print("kernel time under rocprofv3 (%s): %.3f s in %d kernels" % (args.configs, tot * 1e-9, len(rows)))
    circ = 0.0
    for r in sorted(rows, key=lambda r: -float(r["TotalDurationNs"])):
        ns = float(r["TotalDurationNs"])
        if "k_circ" in r["Name"]:
            circ += ns
        print("  %-60s calls %7s  total %10.3f ms  avg %9.1f us  %6.3f %%"
              % (r["Name"][:60], r["Calls"], ns * 1e-6, float(r["AverageNs"]) * 1e-3, 100 * ns / tot))
    print("gather + scatter + collect: %.3f ms = %.3f %% of the kernel time" % (circ * 1e-6, 100 * circ / tot))


def circuit_only(args):
    import sgfhe_jl_amd as S
    import encrypted_adder
    params = S.Params(1024)
    eng = S.Engine(params)
    rng = np.random.default_rng(1)
    eng.generate_key(rng.integers(0, 2, size=params.n).astype(np.uint64), 2)
    for bits, inst in configs(args.configs):
        c = encrypted_adder.adder_circuit(S, bits)
        eng.circuit_run(c, rng.integers(0, params.r, size=(2 * bits, inst, params.n + 1), dtype=np.uint64))
    print("build", eng.build_id())
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default=None, help="bits x instances, comma-separated")
    ap.add_argument("--reps", type=int, default=1)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--circuit-only", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--dir", default="circuit_trace", help="where rocprofv3 writes its files")
    args = ap.parse_args()
    if args.configs is None:
        args.configs = "16x1024" if args.trace else "16x256,16x1024,32x256,32x1024"
    if args.circuit_only:
        circuit_only(args)
    elif args.trace:
        trace(args)
    else:
        wall(args)


if __name__ == "__main__":
    main()
