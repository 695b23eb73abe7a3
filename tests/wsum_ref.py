"""Helpers of the weighted-sum node tests (test_circuit_wsum_host.py, test_gpu_wsum.py): the mod-4 model of a sum
node stated on its own, and the error of every node's INPUT SUM measured with the secret key from a level-by-level
replay -- the condition of the noise rule in include/sgfhe_hip.h, checked before anything is compared."""

import numpy as np

import noise_ref as NR


def sum_node_model(weights, values):
    """weights [k], values [k][instances] (0/1) -> (HI, MID, LOW) from s = sum of w x mod 4."""
    s = sum(int(w) * np.asarray(v).astype(np.int64) for w, v in zip(weights, values)) % 4
    return (s == 2) | (s == 3), (s == 1) | (s == 2), (s & 1) == 1


def with_term_outputs(S, c, keep_outputs=False):
    """A circuit with the nodes of `c` whose outputs are (the outputs of `c`, when asked, and then) the references of
    every term of every node, and the list [(node, weight)] beside those term outputs."""
    d = S.Circuit(c.n_inputs, group=c.group)
    d.gates, d.gate_shifts, d.gate_weights = list(c.gates), list(c.gate_shifts), dict(c.gate_weights)
    terms = [(g, w, S.Wire(ref, sh)) for g in range(c.n_gates)
             for w, ref, sh in zip(c.weights(g), c.gates[g], c.gate_shifts[g])]
    own = [S.Wire(ref, sh) for ref, sh in zip(c.outputs, c.output_shifts)] if keep_outputs else []
    d.output(*(own + [wire for _, _, wire in terms]))
    return d, [(g, w) for g, w, _ in terms]


def sum_errors(params, sk, n_gates, terms, lwes, plain):
    """{node: largest |error| of the sum of w X over its terms} for EVERY node, from the LWEs [terms][instances][n + 1]
    and plaintext bits [terms][instances] of the term outputs of with_term_outputs; the error is against
    (sum of w x) Dr mod r, centred."""
    lwes, plain = np.asarray(lwes).astype(np.int64), np.asarray(plain).astype(np.int64)
    worst = {}
    for g in range(n_gates):
        idx = [i for i, (h, _) in enumerate(terms) if h == g]
        total = sum(terms[i][1] * lwes[i] for i in idx) % params.r
        s = sum(terms[i][1] * plain[i] for i in idx)
        ph = NR.phases_zr(params, sk, total.astype(np.uint64)).astype(np.int64)
        e = (ph - s * params.Dr) % params.r
        e = np.where(e > params.r // 2, e - params.r, e)
        worst[g] = int(np.abs(e).max())
    assert sorted(worst) == list(range(n_gates))
    return worst


def input_sum_errors(S, params, sk, c, inputs, bits, boot):
    """sum_errors of `c` from replay_levels driven by `boot`."""
    from sgfhe_jl_amd import circuit as C
    d, terms = with_term_outputs(S, c)
    return sum_errors(params, sk, c.n_gates, terms, C.replay_levels(d, inputs, params.r, boot), d.evaluate_plain(bits))
