"""Stepped run against the host loop (profiles/r19_circuit_steps.txt, RESULTS.md): serial_adder over `steps` steps at
Params(1024) as ONE sgfhe_circuit_run_steps, against the same steps as a host loop of sgfhe_circuit_run on the step plan
with the carry pulled down and pushed up again each step -- the only form a stateful circuit had before registers.  Both
on one ctx, the same key and inputs, deterministic flatten; the outputs must be the same bytes.  Prints wall times of
`reps` repetitions of each after one warm-up, the bytes each moves up and down, and the wire-table sizes beside
ripple_adder(steps)'s.
Run on a GPU box:  python tools/steps_bench.py [instances] [steps] [reps]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(inst=1024, steps=16, reps=3):
    import sgfhe_jl_amd as S
    params = S.Params(1024)
    n, r = params.n, params.r
    rng = np.random.default_rng(19)
    sk = rng.integers(0, 2, size=n, dtype=np.uint64)
    eng = S.Engine(params)
    eng.generate_key(sk, 22)
    x, y = rng.integers(0, 1 << steps, size=inst), rng.integers(0, 1 << steps, size=inst)
    bits = np.array([[(x >> i) & 1, (y >> i) & 1] for i in range(steps)], dtype=np.uint64)
    stream = np.zeros((steps, 2, inst, n + 1), dtype=np.uint64)
    stream[..., :n] = rng.integers(0, r, size=stream.shape[:3] + (n,), dtype=np.uint64)
    e = rng.integers(-(r // 64), r // 64 + 1, size=bits.shape).astype(np.int64).astype(np.uint64)
    stream[..., n] = (stream[..., :n] @ sk + bits * np.uint64(params.Dr) + e) & np.uint64(r - 1)
    c = S.serial_adder()
    sp = c.step_plan()
    zero = np.zeros((1, inst, n + 1), dtype=np.uint64)

    def stepped():
        return eng.circuit_run_steps(c, None, stream)

    def host_loop():
        state, outs = zero, []
        for s in range(steps):
            res = eng.circuit_run(sp, np.concatenate([state, stream[s]]))
            outs.append(res[:1])
            state = res[1:]
        return np.stack(outs), state

    results, times = {}, {}
    for name, fn in (("host loop", host_loop), ("stepped", stepped), ("host loop again", host_loop), ("stepped again", stepped)):
        fn()
        t = []
        for _ in range(reps):
            t0 = time.perf_counter()
            results[name] = fn()
            t.append(time.perf_counter() - t0)
        times[name] = t
    for name in results:
        assert np.array_equal(results[name][0], results["stepped"][0]) and np.array_equal(results[name][1], results["stepped"][1])
    out, end = results["stepped"]
    phase = lambda lwe: ((lwe[..., n] - lwe[..., :n] @ sk + np.uint64(params.Dr // 2)) & np.uint64(r - 1)) // np.uint64(params.Dr)
    total = sum(phase(out[i, 0]).astype(np.int64) << i for i in range(steps)) + (phase(end[0]).astype(np.int64) << steps)
    assert np.array_equal(total, x + y), "wrong sums"
    row = (n + 1) * 8
    print("serial_adder, Params(1024), %d instances, %d steps, %d bootstraps per run; build %s"
          % (inst, steps, inst * steps, eng.build_id()))
    for name, t in times.items():
        print("  %-16s %s s   (min %.4f, spread %.4f)" % (name, " ".join("%.4f" % v for v in t), min(t), max(t) - min(t)))
    a, b = min(times["stepped"] + times["stepped again"]), min(times["host loop"] + times["host loop again"])
    print("  stepped / host loop (best of each): %.4f" % (a / b))
    print("  bytes up:   stepped %d (2 stream inputs a step), host loop %d (carry + 2 inputs a step)"
          % (steps * 2 * inst * row, steps * 3 * inst * row))
    print("  bytes down: stepped %d (1 output a step + the carry once), host loop %d (output + carry a step)"
          % ((steps + 1) * inst * row, steps * 2 * inst * row))
    rp = S.ripple_adder(steps)
    print("  wire table: serial_adder %d slots = %d bytes, state buffer %d bytes; ripple_adder(%d) %d slots = %d bytes, "
          "%d bytes of inputs uploaded at once"
          % (c.info()["slots"], c.info()["slots"] * inst * row, inst * row, steps, rp.info()["slots"],
             rp.info()["slots"] * inst * row, 2 * steps * inst * row))
    print("  the sums of all %d instances are right; stepped run and host loop give the same bytes" % inst)
    eng.close()


if __name__ == "__main__":
    a = [int(v) for v in sys.argv[1:]]
    main(*a)
