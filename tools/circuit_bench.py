"""Gate circuits on the device (sgfhe_circuit_run) against the same levels replayed through
Engine.bootstrap_batch on host arrays, at Params(1024), deterministic flatten.

  python tools/circuit_bench.py [--configs 16x256,16x1024,32x256,32x1024] [--reps 1]
      wall time of ripple-carry adders (examples/encrypted_adder.py: 3 nodes per bit) over many instances:
      gates/s of one circuit_run against the per-level replay, the two alternating in one process (the
      order swaps every repetition), with the rows of every level; both paths must give the same bytes.
  python tools/circuit_bench.py --trace [--configs 16x1024] [--dir DIR]
      the same circuit run in a child process under `rocprofv3 --kernel-trace --stats`: the share of the
      gather, scatter and collect kernels in the kernel time of the run.

  python tools/circuit_bench.py --ct [--configs 16x1] [--reps 3]
      ciphertexts in and out (bits x blocks; a block is n = 1024 instances): (A) one circuit_run_ct -- split and
      pack on the device -- against (B) what a caller composes from host arrays without it: host split
      (sgfhe_host_split_ciphertext), circuit_run, pack_encrypted_bits in groups of 8 ciphertexts.  The two
      alternate in one process on two ctxs that share one key (the order swaps every round); the bytes must be
      equal; prints both times per round, their spread, and the bytes each moves over PCIe each way.
  python tools/circuit_bench.py --ct --direct [--configs 16x1] [--reps 3]
      (A) as above against (D) the same run with SGFHE_CIRCUIT_PACK_DIRECT -- the outputs packed from the gates' LWEs
      over Z_Q, without the n refresh bootstraps per output ciphertext -- alternating on one ctx; the LWE outputs
      must be the same bytes; prints both times per round and the bootstraps each runs.
  python tools/circuit_bench.py --probe [--configs 16x1024] [--reps 3]
      (R) circuit_run against (P) circuit_probe -- the same run with the noise probe of every wire -- alternating on
      one ctx (the order swaps every round); the outputs must be the same bytes; prints both times per round and
      the worst record of the probed run.  --run-only: (R) alone, the same rounds (what an older build can run).
  python tools/circuit_bench.py --gate3 [--configs 16x1024] [--reps 3]
      (T) the adder of 3 two-input nodes per bit against (F) ripple_adder -- one three-input node, one bootstrap, per
      bit (sgfhe_circuit_create3) -- alternating on one ctx (the order swaps every round), on valid encryptions; both
      must decrypt to the integer sums; prints both times per round and the bootstraps each runs.  Then, in a run of
      its own, the noise probe of (F): the worst max |e| per wire kind and the largest error of the sum of a node's
      three inputs.
  python tools/circuit_bench.py --ct --gate3 --lift [--configs 16x1] [--reps 3]
      ripple_adder (one full adder per bit: every sum bit an XOR3 wire) with ciphertexts in and out: (A) refreshed,
      (D) SGFHE_CIRCUIT_PACK_DIRECT -- only the carry-out is a gate row -- and (L) SGFHE_CIRCUIT_PACK_LIFT -- no
      bootstrap in the pack stage -- interleaved on one ctx (the order rotates every round), on valid encryptions
      (|e| <= Dr/16); the LWE outputs must be the same bytes and all three must decrypt to the sums; prints the times
      beside the bootstraps each runs, and the worst packed phase error of each.
  python tools/circuit_bench.py --ct --trace [--configs 16x1] [--dir DIR]
      run (A) alone in a child process under `rocprofv3 --kernel-trace --stats`: the share of k_circ_split.
  python tools/circuit_bench.py --device [--configs 16x1024] [--reps 3]
      ripple_adder: (H) the host form, circuit_run on numpy arrays, against (D) the device-resident form,
      circuit_run_device on torch tensors, timed from the call to the end of sync(), with the time the call itself
      takes (the queueing); alternating on one ctx (the order swaps every round); the bytes must be equal.

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


def wall_ct(args):
    import sgfhe_jl_amd as S
    import encrypted_adder
    from sgfhe_jl_amd import circuit as C
    params = S.Params(1024)
    n, m = params.n, params.m
    eng_a = S.Engine(params)
    rng = np.random.default_rng(1)
    eng_a.generate_key(rng.integers(0, 2, size=n).astype(np.uint64), 2)
    eng_b = eng_a.clone()
    cpc = C.pack_calls(n)
    print("build %s, Params(1024), deterministic flatten, call rows %d, %d ciphertexts per pack call"
          % (eng_a.build_id(), C.CALL_ROWS, cpc))
    warm = encrypted_adder.adder_circuit(S, 2)
    wa = rng.integers(0, params.r, size=(4, 1, n), dtype=np.uint64)
    for e in (eng_a, eng_b):
        e.circuit_run_ct(warm, wa, wa)

    def composed(c, a, b):
        inputs = np.zeros((c.n_inputs, a.shape[1] * n, n + 1), dtype=np.uint64)
        for i in range(a.shape[0]):
            for t in range(a.shape[1]):
                la, lb = S.host.split_ciphertext(params, a[i, t], b[i, t])
                inputs[i, t * n:(t + 1) * n, :n], inputs[i, t * n:(t + 1) * n, n] = la, lb
        lwe = eng_b.circuit_run(c, inputs)
        g = lwe.reshape(-1, n, n + 1)
        w = np.zeros((len(g), m), dtype=np.uint64)
        v = np.zeros((len(g), m), dtype=np.uint64)
        for q0 in range(0, len(g), cpc):
            w[q0:q0 + cpc], v[q0:q0 + cpc] = eng_b.pack_encrypted_bits(g[q0:q0 + cpc, :, :n], g[q0:q0 + cpc, :, n])
        return w.reshape(c.n_outputs, -1, m), v.reshape(c.n_outputs, -1, m)

    for bits, blocks in configs(args.configs):
        c = encrypted_adder.adder_circuit(S, bits)
        info = c.info()
        inst = blocks * n
        boots = (info["nodes"] + c.n_outputs) * inst
        a = rng.integers(0, params.r, size=(2 * bits, blocks, n), dtype=np.uint64)
        b = rng.integers(0, params.r, size=(2 * bits, blocks, n), dtype=np.uint64)
        lwe_in, lwe_out = c.n_inputs * inst * (n + 1) * 8, c.n_outputs * inst * (n + 1) * 8
        ct_in, ct_out = 2 * c.n_inputs * blocks * n * 8, 2 * c.n_outputs * blocks * m * 8
        print("\n%d-bit adder x %d block(s) = %d instances: %d levels, %d nodes per instance, %d outputs, "
              "%d bootstraps per run (gates + pack)" % (bits, blocks, inst, info["levels"], info["nodes"], c.n_outputs, boots))
        print("  PCIe bytes  (A) up %d  down %d  |  (B) up %d (LWE inputs %d + LWEs again for the pack %d)  "
              "down %d (LWE outputs %d + ciphertexts %d)" % (ct_in, ct_out, lwe_in + lwe_out, lwe_in, lwe_out,
                                                            lwe_out + ct_out, lwe_out, ct_out))
        ta, tb = [], []
        for rep in range(args.reps):
            res = {}
            order = ("A", "B") if rep % 2 == 0 else ("B", "A")
            for what in order:
                t0 = time.perf_counter()
                out = eng_a.circuit_run_ct(c, a, b) if what == "A" else composed(c, a, b)
                res[what] = (time.perf_counter() - t0, out)
            same = all(np.array_equal(x, y) for x, y in zip(res["A"][1], res["B"][1]))
            ta.append(res["A"][0])
            tb.append(res["B"][0])
            print("  round %d (%s first): (A) circuit_run_ct %.3f s = %.0f bootstraps/s | (B) composed from host arrays "
                  "%.3f s = %.0f bootstraps/s | B / A %.4f | same bytes: %s"
                  % (rep, order[0], ta[-1], boots / ta[-1], tb[-1], boots / tb[-1], tb[-1] / ta[-1], same))
            if not same:
                sys.exit("circuit_run_ct and the composition differ")
        print("  (A) mean %.3f s, spread %.3f s | (B) mean %.3f s, spread %.3f s | mean B - mean A = %+.3f s"
              % (np.mean(ta), max(ta) - min(ta), np.mean(tb), max(tb) - min(tb), np.mean(tb) - np.mean(ta)))
    eng_b.close()
    eng_a.close()


def wall_direct(args):
    import sgfhe_jl_amd as S
    import encrypted_adder
    from sgfhe_jl_amd import circuit as C
    params = S.Params(1024)
    n = params.n
    eng = S.Engine(params)
    rng = np.random.default_rng(1)
    eng.generate_key(rng.integers(0, 2, size=n).astype(np.uint64), 2)
    print("build %s, Params(1024), deterministic flatten, call rows %d, %d ciphertexts per pack group"
          % (eng.build_id(), C.CALL_ROWS, C.pack_calls(n)))
    warm = encrypted_adder.adder_circuit(S, 2)
    wa = rng.integers(0, params.r, size=(4, 1, n), dtype=np.uint64)
    for d in (False, True):
        eng.circuit_run_ct(warm, wa, wa, direct=d)
    for bits, blocks in configs(args.configs):
        c = encrypted_adder.adder_circuit(S, bits)
        info = c.info()
        inst = blocks * n
        refreshed = sum(1 for ref in c.outputs if (ref & 0x7FFFFFFF) < c.n_inputs or (ref & 0x7FFFFFFF) == C.FALSE_ID)
        boots = {"A": (info["nodes"] + c.n_outputs) * inst, "D": (info["nodes"] + refreshed) * inst}
        a = rng.integers(0, params.r, size=(2 * bits, blocks, n), dtype=np.uint64)
        b = rng.integers(0, params.r, size=(2 * bits, blocks, n), dtype=np.uint64)
        print("\n%d-bit adder x %d block(s) = %d instances: %d levels, %d nodes per instance, %d outputs (%d refreshed "
              "in the direct run); bootstraps per run: (A) %d, (D) %d; raw output table %.0f MB"
              % (bits, blocks, inst, info["levels"], info["nodes"], c.n_outputs, refreshed, boots["A"], boots["D"],
                 c.n_outputs * blocks * n * (n + 1) * 16 / 1e6))
        t = {"A": [], "D": []}
        for rep in range(args.reps):
            res = {}
            order = ("A", "D") if rep % 2 == 0 else ("D", "A")
            for what in order:
                t0 = time.perf_counter()
                out = eng.circuit_run_ct(c, a, b, packed=True, lwe=True, direct=what == "D")
                res[what] = (time.perf_counter() - t0, out)
                t[what].append(res[what][0])
            same = np.array_equal(res["A"][1][1], res["D"][1][1])
            print("  round %d (%s first): (A) refreshed %.3f s = %.0f bootstraps/s | (D) direct %.3f s = %.0f bootstraps/s | "
                  "D / A %.4f | same LWE outputs: %s"
                  % (rep, order[0], t["A"][-1], boots["A"] / t["A"][-1], t["D"][-1], boots["D"] / t["D"][-1],
                     t["D"][-1] / t["A"][-1], same))
            if not same:
                sys.exit("the LWE outputs of the direct run differ")
        print("  (A) mean %.3f s, spread %.3f s | (D) mean %.3f s, spread %.3f s | mean D / mean A = %.4f, by bootstrap "
              "counts %.4f" % (np.mean(t["A"]), max(t["A"]) - min(t["A"]), np.mean(t["D"]), max(t["D"]) - min(t["D"]),
                               np.mean(t["D"]) / np.mean(t["A"]), boots["D"] / boots["A"]))
    eng.close()


def wall_probe(args):
    import sgfhe_jl_amd as S
    import encrypted_adder
    from sgfhe_jl_amd import circuit as C
    params = S.Params(1024)
    n = params.n
    eng = S.Engine(params)
    rng = np.random.default_rng(1)
    sk = rng.integers(0, 2, size=n).astype(np.uint64)
    eng.generate_key(sk, 2)
    print("build %s, Params(1024), deterministic flatten, call rows %d" % (eng.build_id(), C.CALL_ROWS))
    warm = encrypted_adder.adder_circuit(S, 2)
    wi = rng.integers(0, params.r, size=(4, 64, n + 1), dtype=np.uint64)
    eng.circuit_run(warm, wi)
    if not args.run_only:
        eng.circuit_probe(warm, wi, sk, np.zeros((4, 64), dtype=np.uint8))
    for bits, inst in configs(args.configs):
        c = encrypted_adder.adder_circuit(S, bits)
        info = c.info()
        gates = info["nodes"] * inst
        # valid encryptions (uniform a, b = <a, s> + bit Dr + small e), so that the records mean something
        plain = rng.integers(0, 2, size=(2 * bits, inst)).astype(np.uint8)
        inputs = rng.integers(0, params.r, size=(2 * bits, inst, n + 1), dtype=np.uint64)
        dot = (inputs[:, :, :n] * sk[None, None, :]).sum(axis=2, dtype=np.uint64)
        e = rng.integers(-(params.Dr // 16), params.Dr // 16 + 1, size=plain.shape)
        inputs[:, :, n] = (dot.astype(np.int64) + plain.astype(np.int64) * params.Dr + e) % params.r
        print("\n%d-bit adder x %d instances: %d levels, %d nodes per instance, %d gates per run; the probe reads "
              "%.1f MB of result rows and %.1f MB of inputs"
              % (bits, inst, info["levels"], info["nodes"], gates, gates * 3 * (n + 1) * 8 / 1e6,
                 2 * bits * inst * (n + 1) * 8 / 1e6))
        t = {"R": [], "P": []}
        for rep in range(args.reps):
            res = {}
            order = ("R",) if args.run_only else ("R", "P") if rep % 2 == 0 else ("P", "R")
            for what in order:
                t0 = time.perf_counter()
                out = eng.circuit_run(c, inputs) if what == "R" else eng.circuit_probe(c, inputs, sk, plain)
                res[what] = (time.perf_counter() - t0, out)
                t[what].append(res[what][0])
            if args.run_only:
                print("  round %d: (R) circuit_run %.3f s = %.0f gates/s" % (rep, t["R"][-1], gates / t["R"][-1]))
                continue
            same = np.array_equal(res["R"][1], res["P"][1][0])
            print("  round %d (%s first): (R) circuit_run %.3f s = %.0f gates/s | (P) circuit_probe %.3f s = %.0f gates/s | "
                  "P / R %.4f | same outputs: %s"
                  % (rep, order[0], t["R"][-1], gates / t["R"][-1], t["P"][-1], gates / t["P"][-1],
                     t["P"][-1] / t["R"][-1], same))
            if not same:
                sys.exit("the outputs of the probed run differ")
        print("  (R) mean %.3f s, spread %.3f s" % (np.mean(t["R"]), max(t["R"]) - min(t["R"])))
        if not args.run_only:
            print("  (P) mean %.3f s, spread %.3f s | mean P / mean R = %.4f"
                  % (np.mean(t["P"]), max(t["P"]) - min(t["P"]), np.mean(t["P"]) / np.mean(t["R"])))
            rep = C.noise_report(c, res["P"][1][1])
            print("  records: %d wires, wrong rows %d, worst max |e| %d on wire %d (%s of node %s, level %d) against "
                  "Dr/4 = %d" % (len(rep), sum(d["wrong"] for d in rep), rep[0]["max_abs"], rep[0]["wire"], rep[0]["kind"],
                                 rep[0]["node"], rep[0]["level"], params.Dr // 4))
    eng.close()


def wall_gate3(args):
    import sgfhe_jl_amd as S
    import encrypted_adder
    from sgfhe_jl_amd import circuit as C
    params = S.Params(1024)
    n, r, Dr = params.n, params.r, params.Dr
    eng = S.Engine(params)
    rng = np.random.default_rng(1)
    sk = rng.integers(0, 2, size=n).astype(np.uint64)
    eng.generate_key(sk, 2)
    print("build %s, Params(1024), deterministic flatten, call rows %d" % (eng.build_id(), C.CALL_ROWS))
    wi = rng.integers(0, r, size=(4, 64, n + 1), dtype=np.uint64)
    for warm in (encrypted_adder.adder_circuit(S, 2), C.ripple_adder(2)):
        eng.circuit_run(warm, wi)
    eng.circuit_probe(C.ripple_adder(2), wi, sk, np.zeros((4, 64), dtype=np.uint8))

    def phase_error(lwe, bits):   # centred error of LWEs [..., n + 1] that encrypt the integers `bits` (times Dr)
        ph = lwe[..., n] - (lwe[..., :n] * sk).sum(axis=-1, dtype=np.uint64)
        e = (ph.astype(np.int64) - bits.astype(np.int64) * Dr) % r
        return np.where(e > r // 2, e - r, e)

    for bits, inst in configs(args.configs):
        circ = {"T": encrypted_adder.adder_circuit(S, bits), "F": C.ripple_adder(bits)}
        info = {k: c.info() for k, c in circ.items()}
        boots = {k: info[k]["nodes"] * inst for k in circ}
        # valid encryptions (uniform a, b = <a, s> + bit Dr + e, |e| <= Dr/16), so that the sums decrypt
        xs, ys = rng.integers(0, 1 << bits, size=inst), rng.integers(0, 1 << bits, size=inst)
        plain = np.array([(xs >> i) & 1 for i in range(bits)] + [(ys >> i) & 1 for i in range(bits)], dtype=np.uint8)
        inputs = rng.integers(0, r, size=(2 * bits, inst, n + 1), dtype=np.uint64)
        dot = (inputs[:, :, :n] * sk[None, None, :]).sum(axis=2, dtype=np.uint64)
        e = rng.integers(-(Dr // 16), Dr // 16 + 1, size=plain.shape)
        inputs[:, :, n] = (dot.astype(np.int64) + plain.astype(np.int64) * Dr + e) % r
        print("\n%d-bit adder x %d instances: (T) two-input nodes: %d levels, %d nodes per instance, %d bootstraps | "
              "(F) full adders: %d levels, %d nodes per instance, %d bootstraps | F / T by bootstrap counts %.4f"
              % (bits, inst, info["T"]["levels"], info["T"]["nodes"], boots["T"], info["F"]["levels"], info["F"]["nodes"],
                 boots["F"], boots["F"] / boots["T"]))
        t = {"T": [], "F": []}
        for rep in range(args.reps):
            order = ("T", "F") if rep % 2 == 0 else ("F", "T")
            for what in order:
                t0 = time.perf_counter()
                out = eng.circuit_run(circ[what], inputs)
                t[what].append(time.perf_counter() - t0)
                dec = ((phase_error(out, np.zeros(out.shape[:2], np.int64)) + Dr // 2) % r) // Dr
                if not np.array_equal((dec << np.arange(bits + 1)[:, None]).sum(axis=0), xs + ys):
                    sys.exit("(%s) does not decrypt to the sums" % what)
            print("  round %d (%s first): (T) %.3f s = %.0f bootstraps/s | (F) %.3f s = %.0f bootstraps/s | F / T %.4f | "
                  "both decrypt to x + y" % (rep, order[0], t["T"][-1], boots["T"] / t["T"][-1], t["F"][-1],
                                             boots["F"] / t["F"][-1], t["F"][-1] / t["T"][-1]))
        print("  (T) mean %.3f s, spread %.3f s | (F) mean %.3f s, spread %.3f s | mean F / mean T = %.4f, by bootstrap "
              "counts %.4f" % (np.mean(t["T"]), max(t["T"]) - min(t["T"]), np.mean(t["F"]), max(t["F"]) - min(t["F"]),
                               np.mean(t["F"]) / np.mean(t["T"]), boots["F"] / boots["T"]))
        # the probe of (F), a run of its own; its outputs are every sum bit and every carry, so that the error of the
        # sum of each node's inputs can be taken on the host from the LWEs the node read
        f = C.ripple_adder(bits)
        carries = [C.Wire(f.n_inputs + 3 * g) for g in range(bits)]
        f.output(*([C.Wire(f.n_inputs + 3 * g + 2) for g in range(bits)] + carries))
        out, stats = eng.circuit_probe(f, inputs, sk, plain)
        recs = C.noise_report(f, stats)
        print("  probe of (F): %d wires, wrong rows %d; against Dr/4 = %d and Dr/2 = %d:"
              % (len(recs), sum(d["wrong"] for d in recs), Dr // 4, Dr // 2))
        for kind in ("input", "MAJ", "ONE_OR_TWO", "XOR3"):
            worst = max((d for d in recs if d["kind"] == kind), key=lambda d: d["max_abs"])
            print("    %-10s worst max |e| %5d (wire %d, level %d), rms there %.1f"
                  % (kind, worst["max_abs"], worst["wire"], worst["level"], worst["rms"]))
        carry_bits = np.zeros(inst, dtype=np.int64)
        carry_lwe = np.zeros((inst, n + 1), dtype=np.uint64)
        worst_sum = 0
        for g in range(bits):
            total = (inputs[g] + inputs[bits + g] + carry_lwe) & np.uint64(r - 1)
            s = plain[g].astype(np.int64) + plain[bits + g] + carry_bits
            worst_sum = max(worst_sum, int(np.abs(phase_error(total, s)).max()))
            carry_bits, carry_lwe = s >> 1, out[bits + g]
        print("    largest error of the sum of a node's three inputs: %d against Dr/2 = %d" % (worst_sum, Dr // 2))
    eng.close()


def wall_lift(args):
    import sgfhe_jl_amd as S
    from sgfhe_jl_amd import circuit as C
    params = S.Params(1024)
    n, r, Dr = params.n, params.r, params.Dr
    eng = S.Engine(params)
    rng = np.random.default_rng(1)
    sk = rng.integers(0, 2, size=n).astype(np.uint64)
    eng.generate_key(sk, 2)
    print("build %s, Params(1024), deterministic flatten, call rows %d, %d ciphertexts per pack group"
          % (eng.build_id(), C.CALL_ROWS, C.pack_calls(n)))
    kw = {"A": {}, "D": {"direct": True}, "L": {"lift": True}}
    names = {"A": "refreshed", "D": "direct", "L": "lift"}
    wa = rng.integers(0, r, size=(4, 1, n), dtype=np.uint64)
    for k in "ADL":
        eng.circuit_run_ct(C.ripple_adder(2), wa, wa, **kw[k])

    def errors(a, b, bits):   # centred error of every message coefficient of RLWEs [..., N] against bits [..., n]
        lwe = C.split_ciphertext_array(a, b, n, r)
        ph = lwe[..., n] - (lwe[..., :n] * sk).sum(axis=-1, dtype=np.uint64)
        e = (ph.astype(np.int64) - bits.astype(np.int64) * Dr) % r
        return np.where(e > r // 2, e - r, e)

    for bits, blocks in configs(args.configs):
        c = C.ripple_adder(bits)
        info = c.info()
        inst = blocks * n
        level = info["nodes"] * inst
        boots = {"A": level + c.n_outputs * inst, "D": level + bits * inst, "L": level}   # (the sum bits are XOR3 wires)
        # valid encryptions: a uniform, b = a s + bit Dr + e with |e| <= Dr/16 on the message coefficients
        xs, ys = rng.integers(0, 1 << bits, size=inst), rng.integers(0, 1 << bits, size=inst)
        plain = np.array([(xs >> i) & 1 for i in range(bits)] + [(ys >> i) & 1 for i in range(bits)],
                         dtype=np.int64).reshape(2 * bits, blocks, n)
        a = rng.integers(0, r, size=(2 * bits, blocks, n), dtype=np.uint64)
        e0 = rng.integers(-(Dr // 16), Dr // 16 + 1, size=plain.shape)
        b = ((errors(a, np.zeros_like(a), np.zeros_like(plain)) * -1 + plain * Dr + e0) % r).astype(np.uint64)
        want = np.array([((xs + ys) >> i) & 1 for i in range(bits + 1)], dtype=np.int64).reshape(bits + 1, blocks, n)
        print("\n%d-bit ripple adder x %d block(s) = %d instances: %d levels, %d nodes per instance, %d outputs (%d XOR3 "
              "wires); bootstraps per run: (A) %d, (D) %d, (L) %d; raw output table %.0f MB"
              % (bits, blocks, inst, info["levels"], info["nodes"], c.n_outputs, bits, boots["A"], boots["D"], boots["L"],
                 c.n_outputs * blocks * n * (n + 1) * 16 / 1e6))
        t = {k: [] for k in "ADL"}
        worst = {}
        for rep in range(args.reps):
            res = {}
            order = "ADL"[rep % 3:] + "ADL"[:rep % 3]
            for what in order:
                t0 = time.perf_counter()
                res[what] = eng.circuit_run_ct(c, a, b, packed=True, lwe=True, **kw[what])
                t[what].append(time.perf_counter() - t0)
            same = all(np.array_equal(res["A"][1], res[k][1]) for k in "DL")
            print("  round %d (order %s): " % (rep, order) +
                  " | ".join("(%s) %s %.3f s, %d bootstraps = %.0f bootstraps/s"
                             % (k, names[k], t[k][-1], boots[k], boots[k] / t[k][-1]) for k in "ADL") +
                  " | L / A %.4f, L / D %.4f | same LWE outputs: %s"
                  % (t["L"][-1] / t["A"][-1], t["L"][-1] / t["D"][-1], same))
            if not same:
                sys.exit("the LWE outputs of the three runs differ")
            for k in "ADL":
                err = np.abs(errors(res[k][0][0], res[k][0][1], want))
                if err.max() >= Dr // 2:
                    sys.exit("(%s) does not decrypt to the sums" % k)
                worst[k] = (int(err[:bits].max()), int(err[bits].max()))
        mean = {k: np.mean(t[k]) for k in "ADL"}
        print("  " + " | ".join("(%s) mean %.3f s, spread %.3f s" % (k, mean[k], max(t[k]) - min(t[k])) for k in "ADL"))
        print("  mean L / mean A = %.4f, by bootstrap counts %.4f | mean L / mean D = %.4f, by bootstrap counts %.4f"
              % (mean["L"] / mean["A"], boots["L"] / boots["A"], mean["L"] / mean["D"], boots["L"] / boots["D"]))
        print("  seconds per 1000 bootstraps: " + ", ".join("(%s) %.4f" % (k, 1e3 * mean[k] / boots[k]) for k in "ADL") +
              "; L minus its share of A's rate: %+.3f s" % (mean["L"] - mean["A"] * boots["L"] / boots["A"]))
        print("  worst packed phase error against Dr/2 = %d (all decrypt to x + y): " % (Dr // 2) +
              ", ".join("(%s) %s: sum bits %d, carry-out %d" % (k, names[k], worst[k][0], worst[k][1]) for k in "ADL"))
    eng.close()


def wall_device(args):
    import torch
    import sgfhe_jl_amd as S
    params = S.Params(1024)
    eng = S.Engine(params)
    rng = np.random.default_rng(1)
    eng.generate_key(rng.integers(0, 2, size=params.n).astype(np.uint64), 2)
    print("build %s, Params(1024), deterministic flatten" % eng.build_id())
    for bits, inst in configs(args.configs):
        c = S.ripple_adder(bits)
        info = c.info()
        x = rng.integers(0, params.r, size=(2 * bits, inst, params.n + 1), dtype=np.uint64)
        xt = torch.from_numpy(x.view(np.int64)).cuda()
        out = torch.empty((c.n_outputs, inst, params.n + 1), dtype=torch.int64, device=xt.device)
        torch.cuda.synchronize()
        eng.circuit_run(c, x[:, :64])                # both forms once: buffers, kernels, pinned pages
        eng.circuit_run_device(c, xt, out=out)
        eng.sync()
        print("\nripple_adder(%d) x %d instances: %d levels, %d bootstraps per run; %.1f MB of inputs, %.1f MB of outputs"
              % (bits, inst, info["levels"], info["nodes"] * inst, x.nbytes / 1e6, out.numel() * 8 / 1e6))
        th, td = [], []
        for rep in range(args.reps):
            order = ("host", "device") if rep % 2 == 0 else ("device", "host")
            for what in order:
                t0 = time.perf_counter()
                if what == "host":
                    h = eng.circuit_run(c, x)
                    th.append(time.perf_counter() - t0)
                else:
                    eng.circuit_run_device(c, xt, out=out)
                    tq = time.perf_counter() - t0
                    eng.sync()
                    td.append(time.perf_counter() - t0)
            same = np.array_equal(out.cpu().numpy().view(np.uint64), h)
            print("  round %d (%s first): (H) host form %.3f s | (D) device form %.3f s, of which the call %.1f ms | "
                  "D / H %.4f | same bytes: %s" % (rep, order[0], th[-1], td[-1], tq * 1e3, td[-1] / th[-1], same))
            if not same:
                sys.exit("the host form and the device-resident form differ")
        print("  (H) min %.3f max %.3f spread %.1f %% | (D) min %.3f max %.3f spread %.1f %% | D / H of the medians %.4f"
              % (min(th), max(th), 100 * (max(th) - min(th)) / min(th), min(td), max(td),
                 100 * (max(td) - min(td)) / min(td), float(np.median(td) / np.median(th))))
    eng.close()


def ct_only(args):
    import sgfhe_jl_amd as S
    import encrypted_adder
    params = S.Params(1024)
    eng = S.Engine(params)
    rng = np.random.default_rng(1)
    eng.generate_key(rng.integers(0, 2, size=params.n).astype(np.uint64), 2)
    for bits, blocks in configs(args.configs):
        c = encrypted_adder.adder_circuit(S, bits)
        a = rng.integers(0, params.r, size=(2 * bits, blocks, params.n), dtype=np.uint64)
        eng.circuit_run_ct(c, a, a)
    print("build", eng.build_id())
    eng.close()


def trace(args):
    d = os.path.abspath(args.dir)
    os.makedirs(d, exist_ok=True)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "circ", "--", sys.executable,
           os.path.abspath(__file__), "--configs", args.configs, "--reps", "1",
           "--ct-only" if args.ct else "--circuit-only"]
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
    print("gather + scatter + collect%s: %.3f ms = %.3f %% of the kernel time"
          % (" + split" if args.ct else "", circ * 1e-6, 100 * circ / tot))
    if args.ct:
        split = sum(float(r["TotalDurationNs"]) for r in rows if "k_circ_split" in r["Name"])
        print("k_circ_split: %.3f ms = %.4f %% of the kernel time" % (split * 1e-6, 100 * split / tot))


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
    ap.add_argument("--ct", action="store_true", help="ciphertexts in and out: circuit_run_ct against the composition")
    ap.add_argument("--direct", action="store_true", help="with --ct: the refreshed run against SGFHE_CIRCUIT_PACK_DIRECT")
    ap.add_argument("--probe", action="store_true", help="circuit_run against circuit_probe (the noise probe of every wire)")
    ap.add_argument("--gate3", action="store_true", help="the adder of two-input nodes against ripple_adder (full adders)")
    ap.add_argument("--lift", action="store_true",
                    help="with --ct --gate3: ripple_adder refreshed, direct and with SGFHE_CIRCUIT_PACK_LIFT")
    ap.add_argument("--device", action="store_true", help="ripple_adder: circuit_run against circuit_run_device")
    ap.add_argument("--run-only", action="store_true", help="with --probe: circuit_run alone, the same rounds")
    ap.add_argument("--circuit-only", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--ct-only", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--dir", default="circuit_trace", help="where rocprofv3 writes its files")
    args = ap.parse_args()
    if args.configs is None:
        args.configs = "16x1" if args.ct or args.ct_only else "16x1024" if args.trace or args.probe or args.gate3 or args.device else \
            "16x256,16x1024,32x256,32x1024"
    if (args.ct or args.probe or args.gate3 or args.device) and not args.trace and args.reps == 1:
        args.reps = 3
    if args.circuit_only:
        circuit_only(args)
    elif args.ct_only:
        ct_only(args)
    elif args.device:
        wall_device(args)
    elif args.trace:
        trace(args)
    elif args.lift:
        if not (args.ct and args.gate3):
            sys.exit("--lift goes with --ct --gate3")
        wall_lift(args)
    elif args.gate3:
        wall_gate3(args)
    elif args.probe:
        wall_probe(args)
    elif args.ct and args.direct:
        wall_direct(args)
    elif args.ct:
        wall_ct(args)
    else:
        wall(args)


if __name__ == "__main__":
    main()
