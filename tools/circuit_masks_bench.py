"""Lane masks: what the rows saved are worth in time (sgfhe_circuit_create_masked; profiles/r26_circuit_masks.txt).

  python tools/circuit_masks_bench.py [--params 512,1024] [--groups 128] [--reps 3]
      bitonic_sort(4, 8) and packed_equal(16), each masked against the same circuit without masks (the sort with every
      comparator on all lanes; the equality as a tree of AND nodes on all lanes), in one process on one keyed ctx: rows a
      group, level calls, best wall time of `reps` circuit_run calls after a warm-up.  The inputs are random words of
      Z_r: a bootstrap costs the same whatever it rotates by.  The rows are asserted; the times are printed.
  python tools/circuit_masks_bench.py --trace [--dir DIR] [--params 1024]
      the masked plans alone in a child process under `rocprofv3 --kernel-trace --stats`: the share of k_circ_mask_fill
      (and of the other circuit kernels) in the kernel time of the run."""

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


def equal_tree(S, width):
    """packed_equal(width) without masks: the XNOR node, then every stage of the reduction on all lanes."""
    c = S.Circuit(2, group=width)
    acc, k = ~c.gate(*c.inputs)[2], 1
    while k < width:
        acc = c.gate(acc, acc.lane(k))[0]
        k *= 2
    c.output(acc)
    return c


def cases(S):
    return [("bitonic_sort(4, 8)", S.bitonic_sort(4, 8), S.bitonic_sort(4, 8, masked=True)),
            ("packed_equal(16)", equal_tree(S, 16), S.packed_equal(16))]


def engine(S, n, seed=1):
    eng = S.Engine(S.Params(n))
    eng.generate_key(np.random.default_rng(seed).integers(0, 2, size=n).astype(np.uint64), 2)
    return eng


def timed(eng, c, inputs, reps):
    eng.circuit_run(c, inputs)
    best = None
    for _ in range(reps):
        t0 = time.perf_counter()
        eng.circuit_run(c, inputs)
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best


def measure(args):
    import sgfhe_jl_amd as S
    for n in [int(v) for v in args.params.split(",")]:
        eng = engine(S, n)
        params = eng.params
        rng = np.random.default_rng(2)
        for name, plain, masked in cases(S):
            G, inst = plain.group, args.groups * plain.group
            inputs = rng.integers(0, params.r, size=(plain.n_inputs, inst, n + 1), dtype=np.uint64)
            line = []
            for c in (plain, masked):
                rows = c.rows_per_group()
                calls = eng.debug_circuit_script_calls(c, inst)
                assert sum(r for r, _ in calls) == rows * args.groups
                line.append((rows, len(calls), timed(eng, c, inputs, args.reps)))
            assert plain.info() == {k: v for k, v in masked.info().items() if k != "rows_per_group"}
            (r0, c0, t0), (r1, c1, t1) = line
            print("Params(%d) %-19s %d groups of %d: rows a group %d -> %d (%.3f), calls %d -> %d, %.3f s -> %.3f s (%.3f), "
                  "%.3f -> %.3f ms a row" % (n, name, args.groups, G, r0, r1, r1 / r0, c0, c1, t0, t1, t1 / t0,
                                             1e3 * t0 / (r0 * args.groups), 1e3 * t1 / (r1 * args.groups)))
        eng.close()


def child(args):
    import sgfhe_jl_amd as S
    n = int(args.params.split(",")[0])
    eng = engine(S, n)
    rng = np.random.default_rng(2)
    for name, plain, masked in cases(S):
        inst = args.groups * masked.group
        eng.circuit_run(masked, rng.integers(0, eng.params.r, size=(masked.n_inputs, inst, n + 1), dtype=np.uint64))
    eng.close()


def trace(args):
    d = os.path.abspath(args.dir)
    os.makedirs(d, exist_ok=True)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "masks", "--", sys.executable,
           os.path.abspath(__file__), "--child", "--params", args.params.split(",")[0], "--groups", str(args.groups)]
    rc = subprocess.call(cmd)
    if rc:
        sys.exit("rocprofv3 run failed: %d" % rc)
    stats = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
    if not stats:
        sys.exit("no kernel_stats.csv under %s" % d)
    rows = list(csv.DictReader(open(stats[0])))
    tot = sum(float(r["TotalDurationNs"]) for r in rows)
    print("Params(%s), the two masked plans over %d groups: kernel time under rocprofv3 %.3f s in %d kernels"
          % (args.params.split(",")[0], args.groups, tot * 1e-9, len(rows)))
    for r in sorted(rows, key=lambda r: -float(r["TotalDurationNs"])):
        ns = float(r["TotalDurationNs"])
        if "k_circ" in r["Name"]:
            print("  %-40s calls %7s  total %10.3f ms  avg %9.1f us  %7.4f %%"
                  % (r["Name"][:40], r["Calls"], ns * 1e-6, float(r["AverageNs"]) * 1e-3, 100 * ns / tot))
    f = sum(float(r["TotalDurationNs"]) for r in rows if "k_circ_mask_fill" in r["Name"])
    print("k_circ_mask_fill: %.3f ms = %.4f %% of the kernel time" % (f * 1e-6, 100 * f / tot))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--params", default="512,1024")
    ap.add_argument("--groups", type=int, default=128)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--dir", default=os.path.join(ROOT, "circuit_trace"))
    args = ap.parse_args()
    if args.child:
        child(args)
    elif args.trace:
        trace(args)
    else:
        measure(args)


if __name__ == "__main__":
    main()
