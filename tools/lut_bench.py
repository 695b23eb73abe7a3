"""LUT bootstraps (sgfhe_bootstrap_lut_batch) at Params(1024): their noise and their rate.

  python tools/lut_bench.py --noise [--instances 256]
      Three input bits per instance, encrypted with |e| <= Dr/16, refreshed (AND with TRUE, one gate bootstrap), fanned
      to all three scales (table 0xF0 on the wire alone), then LUT bootstraps two levels deep -- level 1 reads the
      fanned inputs, level 2 reads level-1 results at the scale of its position -- composed on the host from the
      primitive's rows (a LUT input is the sum of three rows mod r).  Prints max |e| of the rows at each scale, and the
      worst |e0 + e1 + e2| of a LUT input against Dr/8, in both flatten modes; every row must decrypt to the plain
      evaluation.  Then the same circuit as LUT nodes (Circuit.refresh, fan, lut) through the noise probe
      (sgfhe_circuit_run_probe): max |e| of the wires at each scale, each against its own codeword.
  python tools/lut_bench.py --rate [--batch 4096] [--reps 3]
      sgfhe_bootstrap_lut_batch beside sgfhe_bootstrap_batch at the same batch on one ctx, alternating (the order swaps
      every round): the k-loop is the same, the difference is k_final_lut against k_final and the staging of one input
      instead of two.
  python tools/lut_bench.py --tables 1 8 64 256 [--batch 4096] [--reps 3]
      LUT families: sgfhe_bootstrap_lut_multi_batch with T tables per row beside sgfhe_bootstrap_lut_batch at the same
      batch on one ctx, alternating as --rate does.  The k-loop is the same; the difference is k_final_lut_multi, which
      writes T times the rows, and their way to the host.  The batch is cut (to a multiple of 8) where the result of the
      family call would exceed --max-gib.
  python tools/lut_bench.py --family-noise [--instances 256]
      The circuit of --noise with each level as LUT families (Circuit.lut_multi) through the noise probe: max |e| of the
      family wires that have a slot, two levels deep, in both flatten modes.
"""

import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TABLES1 = (0x96, 0xE8, 0xCA, 0x10, 0x6B, 0xD4)      # level 1: XOR3, MAJ, MUX, one minterm, two S-box bits
TABLES2 = (0xCA, 0x96, 0x2D)


def phases(params, sk, rows):
    rows = rows.reshape(-1, params.n + 1).astype(np.int64)
    return (rows[:, -1] - rows[:, :-1] @ sk.astype(np.int64)) % params.r


def errors(params, sk, rows, bits, scale):
    """Centred error of rows against bit * (Dr >> scale)."""
    r = params.r
    e = (phases(params, sk, rows) - bits.reshape(-1).astype(np.int64) * ((r // 4) >> scale)) % r
    return np.where(e > r // 2, e - r, e)


def encrypt(params, sk, bits, emax, rng):
    n, r = params.n, params.r
    a = rng.integers(0, r, size=(bits.size, n), dtype=np.uint64)
    e = rng.integers(-emax, emax + 1, size=bits.size)
    b = ((a.astype(np.int64) @ sk.astype(np.int64)) + bits.reshape(-1).astype(np.int64) * (r // 4) + e) % r
    return np.concatenate([a, b.astype(np.uint64)[:, None]], axis=1)


def noise(args):
    import sgfhe_jl_amd as S
    params = S.Params(1024)
    n, r, Dr = params.n, params.r, params.r // 4
    inst = args.instances
    rng = np.random.default_rng(11)
    sk = rng.integers(0, 2, size=n).astype(np.uint64)
    eng = S.Engine(params)
    eng.generate_key(sk, 12)
    print("build %s, Params(1024): Dr = %d, Dr/8 = %d, %d instances" % (eng.build_id(), Dr, Dr // 8, inst))
    bits = rng.integers(0, 2, size=(3, inst))
    fresh = encrypt(params, sk, bits, Dr // 16, rng).reshape(3, inst, n + 1)

    def lut(tables, x0, x1, x2, want_in):
        """One LUT bootstrap per (table, instance): x_i [inst][n + 1] at scale 2 - i (None: the constant FALSE).
        Returns rows [tables][inst][3][n + 1] and the worst input-sum error."""
        u = np.zeros((inst, n + 1), dtype=np.uint64)
        for x in (x0, x1, x2):
            if x is not None:
                u = (u + x) % np.uint64(r)
        s = want_in[0] + 2 * want_in[1] + 4 * want_in[2]
        e = (phases(params, sk, u) - s * (Dr // 4)) % r
        e = np.where(e > r // 2, e - r, e)
        a = np.tile(u[:, :n], (len(tables), 1))
        b = np.tile(u[:, n], len(tables))
        t = np.repeat(np.array(tables, dtype=np.uint8), inst)
        out = eng.bootstrap_lut_batch(a, b, t).reshape(len(tables), inst, 3, n + 1)
        plain = np.stack([(tb >> s) & 1 for tb in tables])
        return out, plain, int(np.abs(e).max())

    for rnd in (False, True):
        eng.set_random_flatten(rnd, 13)
        # refresh: AND with the trivial TRUE (0, Dr)
        x = fresh.reshape(-1, n + 1)
        ref = eng.bootstrap_batch(np.zeros_like(x[:, :n]), np.full(len(x), Dr, dtype=np.uint64), x[:, :n], x[:, n])
        refreshed = ref[:, 0].reshape(3, inst, n + 1)
        worst = {0: 0, 1: 0, 2: 0}
        report = []
        e_ref = int(np.abs(errors(params, sk, refreshed, bits, 0)).max())
        zero = np.zeros(inst, dtype=np.int64)
        fans, sum_fan = [], 0
        for i in range(3):     # fan(x) = lut(0xF0, FALSE, FALSE, x)
            out, plain, es = lut((0xF0,), None, None, refreshed[i], (zero, zero, bits[i]))
            assert np.array_equal(plain[0], bits[i])
            fans.append(out[0])
            sum_fan = max(sum_fan, es)
        def measure(rows, plain, name):
            for k in range(3):
                e = errors(params, sk, rows[..., k, :], plain, k)
                C = Dr >> k
                assert np.all(np.abs(e) < C // 2), "%s: a row at scale %d decrypts wrongly" % (name, k)
                worst[k] = max(worst[k], int(np.abs(e).max()))
                report.append("%s scale %d (C = %d): max |e| %d" % (name, k, C, int(np.abs(e).max())))
        for i in range(3):
            measure(fans[i], bits[i], "fan")
        l1, p1, sum1 = lut(TABLES1, fans[0][:, 2], fans[1][:, 1], fans[2][:, 0], (bits[0], bits[1], bits[2]))
        measure(l1, p1, "level 1")
        # level 2: position i reads a level-1 node at scale 2 - i
        l2, p2, sum2 = lut(TABLES2, l1[0][:, 2], l1[1][:, 1], l1[2][:, 0], (p1[0], p1[1], p1[2]))
        measure(l2, p2, "level 2")
        l2b, p2b, sum2b = lut(TABLES2, l1[3][:, 2], l1[4][:, 1], l1[5][:, 0], (p1[3], p1[4], p1[5]))
        measure(l2b, p2b, "level 2")
        print("\n%s flatten: refreshed inputs max |e| %d of Dr = %d" % ("randomised" if rnd else "deterministic", e_ref, Dr))
        for line in sorted(set(report)):
            print("  " + line)
        print("  worst max |e| per scale: %d of %d, %d of %d, %d of %d"
              % (worst[0], Dr, worst[1], Dr // 2, worst[2], Dr // 4))
        print("  worst |e0 + e1 + e2| of a LUT input: fan %d, level 1 %d, level 2 %d, against Dr/8 = %d"
              % (sum_fan, sum1, max(sum2, sum2b), Dr // 8))
        # the same circuit as LUT nodes, through the probe
        from sgfhe_jl_amd import circuit as C
        c = S.Circuit(3)
        f = [c.fan(c.refresh(w)) for w in c.inputs]
        n1 = [c.lut(t, f[0][2], f[1][1], f[2][0]) for t in TABLES1]
        n2 = [c.lut(t, n1[0][2], n1[1][1], n1[2][0]) for t in TABLES2] + \
             [c.lut(t, n1[3][2], n1[4][1], n1[5][0]) for t in TABLES2]
        c.output(*[w[0] for w in n2])
        eng.set_random_flatten(rnd, 13)
        out, stats = eng.circuit_probe(c, fresh, sk, bits.astype(np.uint8))
        assert np.all(np.abs(errors(params, sk, out, c.evaluate_plain(bits), 0)) < Dr // 2)
        rep = C.noise_report(c, stats)
        assert all(d["wrong"] == 0 for d in rep)
        by = {}
        for d in rep:
            by[d["kind"]] = max(by.get(d["kind"], 0), d["max_abs"])
        print("  probe of the circuit (%d nodes, %d levels): max |e| %s; rows past a quarter of their codeword: %d"
              % (c.info()["nodes"], c.info()["levels"],
                 ", ".join("%s %d" % (k, by[k]) for k in ("input", "MID", "F", "F_HALF", "F_QUARTER")),
                 sum(d["margin"] for d in rep if d["kind"] != "input")))
    eng.close()


def rate(args):
    import sgfhe_jl_amd as S
    params = S.Params(1024)
    n, r = params.n, params.r
    rng = np.random.default_rng(21)
    eng = S.Engine(params)
    eng.generate_key(rng.integers(0, 2, size=n).astype(np.uint64), 22)
    B = args.batch
    a1 = rng.integers(0, r, size=(B, n), dtype=np.uint64)
    a2 = rng.integers(0, r, size=(B, n), dtype=np.uint64)
    b1 = rng.integers(0, r, size=B, dtype=np.uint64)
    b2 = rng.integers(0, r, size=B, dtype=np.uint64)
    t = rng.integers(0, 256, size=B).astype(np.uint8)
    print("build %s, Params(1024), deterministic flatten, batch %d" % (eng.build_id(), B))
    eng.bootstrap_batch(a1[:256], b1[:256], a2[:256], b2[:256])
    eng.bootstrap_lut_batch(a1[:256], b1[:256], t[:256])
    for rep in range(args.reps):
        res = {}
        for what in (("gate", "lut") if rep % 2 == 0 else ("lut", "gate")):
            t0 = time.perf_counter()
            if what == "gate":
                eng.bootstrap_batch(a1, b1, a2, b2)
            else:
                eng.bootstrap_lut_batch(a1, b1, t)
            res[what] = time.perf_counter() - t0
        print("  rep %d: bootstrap_batch %.3f s = %.0f /s | bootstrap_lut_batch %.3f s = %.0f /s | ratio %.3f"
              % (rep, res["gate"], B / res["gate"], res["lut"], B / res["lut"], res["lut"] / res["gate"]))
    eng.close()


def tables_rate(args):
    import sgfhe_jl_amd as S
    params = S.Params(1024)
    n, r = params.n, params.r
    rng = np.random.default_rng(21)
    eng = S.Engine(params)
    eng.generate_key(rng.integers(0, 2, size=n).astype(np.uint64), 22)
    print("build %s, Params(1024), deterministic flatten" % eng.build_id())
    for T in args.tables:
        fit = int(args.max_gib * 2 ** 30) // (T * 3 * (n + 1) * 8)
        B = min(args.batch, max(8, fit // 8 * 8))
        a = rng.integers(0, r, size=(B, n), dtype=np.uint64)
        b = rng.integers(0, r, size=B, dtype=np.uint64)
        t = rng.integers(0, 256, size=(B, T)).astype(np.uint8)
        eng.bootstrap_lut_batch(a[:256], b[:256], t[:256, 0])
        eng.bootstrap_lut_multi_batch(a[:256], b[:256], t[:256])
        for rep in range(args.reps):
            res = {}
            for what in (("single", "multi") if rep % 2 == 0 else ("multi", "single")):
                t0 = time.perf_counter()
                if what == "single":
                    eng.bootstrap_lut_batch(a, b, t[:, 0])
                else:
                    eng.bootstrap_lut_multi_batch(a, b, t)
                res[what] = time.perf_counter() - t0
            print("  T = %3d, batch %4d, rep %d: bootstrap_lut_batch %.3f s = %.0f /s | bootstrap_lut_multi_batch %.3f s = "
                  "%.0f rows/s = %.0f tables/s | time ratio %.3f"
                  % (T, B, rep, res["single"], B / res["single"], res["multi"], B / res["multi"], B * T / res["multi"],
                     res["multi"] / res["single"]))
    eng.close()


def family_noise(args):
    import sgfhe_jl_amd as S
    from sgfhe_jl_amd import circuit as C
    params = S.Params(1024)
    n, Dr = params.n, params.r // 4
    inst = args.instances
    rng = np.random.default_rng(11)
    sk = rng.integers(0, 2, size=n).astype(np.uint64)
    eng = S.Engine(params)
    eng.generate_key(sk, 12)
    bits = rng.integers(0, 2, size=(3, inst))
    fresh = encrypt(params, sk, bits, Dr // 16, rng).reshape(3, inst, n + 1)
    c = S.Circuit(3)
    f = [c.fan(c.refresh(w)) for w in c.inputs]
    n1 = c.lut_multi(TABLES1, f[0][2], f[1][1], f[2][0])
    n2 = c.lut_multi(TABLES2, n1[0][2], n1[1][1], n1[2][0]) + c.lut_multi(TABLES2, n1[3][2], n1[4][1], n1[5][0])
    c.output(*[w[0] for w in n2])
    print("build %s, Params(1024): Dr = %d, %d instances; %d bootstraps per instance in %d levels (%d with one LUT node "
          "per table)" % (eng.build_id(), Dr, inst, c.info()["nodes"], c.info()["levels"],
                          c.info()["nodes"] + len(TABLES1) - 1 + 2 * (len(TABLES2) - 1)))
    for rnd in (False, True):
        eng.set_random_flatten(rnd, 13)
        out, stats = eng.circuit_probe(c, fresh, sk, bits.astype(np.uint8))
        assert np.all(np.abs(errors(params, sk, out, c.evaluate_plain(bits), 0)) < Dr // 2)
        rep = C.noise_report(c, stats)
        assert all(d["wrong"] == 0 for d in rep)
        by = {}
        for d in rep:
            if d["node"] is not None and c.kind(d["node"]) == "sibling":
                key = (d["level"], d["kind"])
                by[key] = max(by.get(key, 0), d["max_abs"])
        print("  %s flatten, sibling wires with a slot: %s; rows past a quarter of their codeword: %d"
              % ("randomised" if rnd else "deterministic",
                 ", ".join("level %d %s %d" % (k[0], k[1], v) for k, v in sorted(by.items())),
                 sum(d["margin"] for d in rep if d["kind"] != "input")))
    eng.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--noise", action="store_true")
    ap.add_argument("--rate", action="store_true")
    ap.add_argument("--instances", type=int, default=256)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--tables", type=int, nargs="+")
    ap.add_argument("--max-gib", type=float, default=2.0)
    ap.add_argument("--family-noise", action="store_true")
    args = ap.parse_args()
    if args.noise:
        noise(args)
    if args.rate:
        rate(args)
    if args.tables:
        tables_rate(args)
    if args.family_noise:
        family_noise(args)
    if not (args.noise or args.rate or args.tables or args.family_noise):
        ap.error("--noise, --rate, --tables or --family-noise")


if __name__ == "__main__":
    main()
