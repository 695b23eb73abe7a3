"""TEST INFRASTRUCTURE: the LUT extraction of sgfhe_bootstrap_lut_batch in Python integers (include/sgfhe_hip.h).

A LUT row enters the bootstrap at phase s Dr/4 + e, s = x0 + 2 x1 + 4 x2 and |e| < Dr/8, with the accumulator
started at A0 = DQ_tilde >> 2.  After the k-loop, P(acc, c) is A0 T(c + phase) with T the antiperiodic extension of the
test polynomial (+1 on [0, Dr), 0 at Dr, -1 on (Dr, 2 Dr), then negated), so the coefficient at
c(j) = 3 Dr - (2 j - 1) Dr/8 is the step "+A0 for s >= j, -A0 for s < j", and a truth table is a +-1 combination of
the steps at its transitions.  rows_from_acc is the one reference every GPU comparison uses.
"""

import numpy as np


def sigma(table, s):
    """+1 where bit s of the table is set, else -1; sigma(8) = -sigma(0) (the antiperiodic continuation)."""
    if s == 8:
        return -sigma(table, 0)
    return 1 if (table >> s) & 1 else -1


def transitions(table):
    """The j in 1..8 at which sigma changes: an odd number, at most 7."""
    return [j for j in range(1, 9) if sigma(table, j) != sigma(table, j - 1)]


def coefficient(params, j):
    """c(j) = (3 Dr - (2 j - 1) Dr/8) mod 2 m."""
    Dr = params.r // 4
    return (3 * Dr - (2 * j - 1) * (Dr // 8)) % (2 * params.m)


def kappas(table):
    """kappa_i = -sigma(0) (-1)^i for the i-th transition."""
    return [-sigma(table, 0) * (-1) ** i for i in range(len(transitions(table)))]


def ideal_step(j, s):
    """T(c(j) + s Dr/4) in units of Dr/8: the sign an error-free accumulator shows at c(j) for input sum s (any
    integer: the phases run on antiperiodically past s = 7)."""
    u = (24 - (2 * j - 1) + 2 * s) % 32
    assert u % 8 != 0          # never on a zero of the test polynomial
    return 1 if (u < 8 or u > 24) else -1


def ideal_combination(table, s):
    """(phase of the base LWE) / A0 - 1 for an error-free accumulator: sigma(s mod 8) (-1)^(s div 8)."""
    return sum(k * ideal_step(j, s) for k, j in zip(kappas(table), transitions(table)))


def _P(poly, i, m, Q):
    """P(p, i): p[i] for i < m, -p[i - m] mod Q otherwise, i taken mod 2 m."""
    i %= 2 * m
    return poly[i] if i < m else (Q - poly[i - m]) % Q


def modred(x, params):
    """ModRed of k_final: round(x r / Q), halves up, mod r (fhe.jl:616-618, rescale utils.jl:78-92)."""
    q, rem = divmod(x * params.r, params.Q)
    if rem >= params.Q // 2 + (params.Q & 1):
        q += 1
    return q % params.r


def base_lwe(params, acc_a, acc_b, table):
    """(alpha[0..n), beta) of one row: lists of Python ints mod Q."""
    n, m, Q = params.n, params.m, params.Q
    A0 = params.DQ_tilde >> 2
    js, ks = transitions(table), kappas(table)
    assert len(js) % 2 == 1 and len(js) <= 7
    alpha = [sum(k * _P(acc_a, coefficient(params, j) - e, m, Q) for k, j in zip(ks, js)) % Q for e in range(n)]
    beta = (A0 + sum(k * _P(acc_b, coefficient(params, j), m, Q) for k, j in zip(ks, js))) % Q
    return alpha, beta


def rows_from_acc(params, acc, tables, raw=False):
    """acc [batch][2][m][2] uint64 ({lo, hi} residues of acc_a, acc_b after the k-loop at amplitude A0), tables
    [batch] -> [batch][3][n + 1] uint64 over Z_r, or [batch][3][n + 1][2] residues mod Q with raw: rows 0, 1, 2 carry
    the table's bit at the codewords Dr, Dr/2 and Dr/4 (4, 2 and 1 times the base LWE)."""
    n, Q = params.n, params.Q
    acc = np.asarray(acc, dtype=np.uint64)
    batch = acc.shape[0]
    assert acc.shape == (batch, 2, params.m, 2) and len(tables) == batch
    out = np.zeros((batch, 3, n + 1, 2) if raw else (batch, 3, n + 1), dtype=np.uint64)
    for t in range(batch):
        pa = [int(lo) | (int(hi) << 64) for lo, hi in acc[t, 0]]
        pb = [int(lo) | (int(hi) << 64) for lo, hi in acc[t, 1]]
        alpha, beta = base_lwe(params, pa, pb, int(tables[t]))
        words = alpha + [beta]
        for k in range(3):
            for e, w in enumerate(words):
                v = (w << (2 - k)) % Q
                if raw:
                    out[t, k, e, 0] = v & 0xFFFFFFFFFFFFFFFF
                    out[t, k, e, 1] = v >> 64
                else:
                    out[t, k, e] = modred(v, params)
    return out


def low_oracle(oc, params):
    """The oracle of the same parameter set whose bootstrap starts at A0 = DQ_tilde >> 2."""
    return oc.Oracle(params.n, params.r, params.m, params.Q, params.B, params.DQ_tilde >> 2)


def rows_at(params, sk, s, e, rng):
    """LWE rows over Z_r made from the secret key: row t has phase s[t] Dr/4 + e[t] exactly, a uniform."""
    n, r = params.n, params.r
    s = np.asarray(s, dtype=np.int64)
    e = np.asarray(e, dtype=np.int64)
    a = rng.integers(0, r, size=(len(s), n), dtype=np.uint64)
    skb = (np.asarray(sk, dtype=np.uint64) & np.uint64(1)).astype(np.int64)
    dot = (a.astype(np.int64) @ skb) % r
    b = ((dot + s * (r // 16) + e) % r).astype(np.uint64)
    return a, b


def phase_errors(params, sk, rows, bits, scale):
    """Centred error of rows [..][n + 1] over Z_r against bit * (Dr >> scale)."""
    r = params.r
    rows = np.asarray(rows, dtype=np.uint64).reshape(-1, params.n + 1).astype(np.int64)
    skb = (np.asarray(sk, dtype=np.uint64) & np.uint64(1)).astype(np.int64)
    ph = (rows[:, -1] - rows[:, :-1] @ skb) % r
    C = (r // 4) >> scale
    e = (ph - np.asarray(bits, dtype=np.int64).reshape(-1) * C) % r
    return np.where(e > r // 2, e - r, e)


def decrypt_scaled(params, sk, rows, scale):
    """The bit of rows at codeword C = Dr >> scale: phase nearer to C than to 0 (the rule of decrypt(::EncryptedBit)
    at scale 0: ((phase + Dr/2) mod r) div Dr, where quotients 2 and 3 are wrong and returned as they are)."""
    r = params.r
    rows = np.asarray(rows, dtype=np.uint64).reshape(-1, params.n + 1).astype(np.int64)
    skb = (np.asarray(sk, dtype=np.uint64) & np.uint64(1)).astype(np.int64)
    ph = (rows[:, -1] - rows[:, :-1] @ skb) % r
    C = (r // 4) >> scale
    return ((ph + C // 2) % r) // C


def oracle_boots(o, lo, bkey, params, key, raw=False):
    """(boot, boot_lut) of circuit.replay_levels on the two C oracles -- `o` the standard one, `lo` the low-amplitude
    one of the same parameter set -- through the NTT-domain key, which serves both.  key = None: deterministic; else
    the seed of the draw stream: row t of call `call` draws as bootstrap t of that call, LUT rows at their own indices
    within the call.  raw: un-reduced rows (replay_ct_direct)."""
    khat = o.key_transform(bkey)

    def boot(call, a1, b1, a2, b2):
        return o.bootstrap_batch(khat, a1, b1, a2, b2, raw=raw, opt=True, rnd=(key, call) if key else None)

    def boot_lut(call, a, b, tables, idx):
        z = np.zeros_like(a), np.zeros_like(b)
        _, acc = lo.bootstrap_batch(khat, a, b, z[0], z[1], want_acc=True, opt=True,
                                    rnd=(key, call, np.asarray(idx, dtype=np.uint32)) if key else None)
        return rows_from_acc(params, acc, tables, raw=raw)

    return boot, boot_lut


def lut_input_sum_errors(S, params, sk, c, inputs, bits, boot, boot_lut):
    """{LUT node: largest |error| of X0 + X1 + X2 against s Dr/4, s = x0 + 2 x1 + 4 x2} for every live LUT node of
    `c`, from circuit.replay_levels driven by (boot, boot_lut): the condition of the noise rule in include/sgfhe_hip.h,
    checked before anything is compared.  The sums are what replay_levels hands to boot_lut; their plaintext comes from
    the circuit whose outputs are the terms of the LUT nodes (evaluated in clear only: a term may have any scale)."""
    from sgfhe_jl_amd import circuit as C
    inst = np.asarray(inputs).shape[1]
    r = params.r
    luts = [g for g in range(c.n_gates) if c.kind(g) == "lut"]
    d = S.Circuit(c.n_inputs, group=c.group)
    d.gates, d.gate_shifts = list(c.gates), list(c.gate_shifts)
    d.gate_weights, d.gate_tables = dict(c.gate_weights), dict(c.gate_tables)
    d.outputs = [ref for g in luts for ref in c.gates[g]]
    d.output_shifts = [sh for g in luts for sh in c.gate_shifts[g]]
    plain = d.evaluate_plain(bits).astype(np.int64).reshape(len(luts), 3, inst)
    s_of = {g: plain[i, 0] + 2 * plain[i, 1] + 4 * plain[i, 2] for i, g in enumerate(luts)}
    calls = []                                  # (nodes of the level, first row of the call), in call order
    for nodes in c.schedule():
        calls += [(nodes, r0) for r0 in range(0, len(nodes) * inst, C.CALL_ROWS)]
    worst = {}

    def recording(call, a, b, tables, idx):
        nodes, r0 = calls[call]
        rows = np.concatenate([a, np.asarray(b).reshape(-1, 1)], axis=1)
        skb = (np.asarray(sk, dtype=np.uint64) & np.uint64(1)).astype(np.int64)
        ph = (rows[:, -1].astype(np.int64) - rows[:, :-1].astype(np.int64) @ skb) % r
        for t, R in enumerate(r0 + np.asarray(idx)):
            g = nodes[R // inst]
            e = (int(ph[t]) - int(s_of[g][R % inst]) * (r // 16)) % r
            worst[g] = max(worst.get(g, 0), min(e, r - e))
        return boot_lut(call, a, b, tables, idx)

    C.replay_levels(c, inputs, r, boot, recording)
    return worst
