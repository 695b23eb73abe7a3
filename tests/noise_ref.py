"""The records of the noise probe (sgfhe_lwe_noise, sgfhe_circuit_run_probe; include/sgfhe_hip.h) restated on the
host: numpy for rows over Z_r, Python integers for rows over Z_Q.  Records are tuples of Python ints in the field
order of engine.NoiseStats / NoiseStatsQ, so a test compares them for equality."""

import numpy as np


def phases_zr(params, sk, rows):
    """rows [count][n + 1] uint64 (a then b) -> phase = b - sum a_i s_i mod r, uint64 [count]."""
    rows = np.asarray(rows, dtype=np.uint64).reshape(-1, params.n + 1)
    s = (np.asarray(sk, dtype=np.uint64) & np.uint64(1))
    dot = (rows[:, :params.n] * s[None, :]).sum(axis=1, dtype=np.uint64)     # wraps mod 2^64; r divides 2^64
    return (rows[:, params.n] - dot) & np.uint64(params.r - 1)


def errors_zr(params, sk, rows, expected):
    """The centred error of every row, in (-r/2, r/2], as int64 [count]."""
    r, Dr = params.r, params.r // 4
    d = (phases_zr(params, sk, rows).astype(np.int64) - np.asarray(expected, dtype=np.int64).reshape(-1) * Dr) % r
    return np.where(d > r // 2, d - r, d)


def wrong_zr(params, sk, rows, expected):
    """Per row: ((phase + Dr/2) mod r) div Dr != expected, the rule of decrypt(::EncryptedBit) (src/fhe.jl:504-507)."""
    r, Dr = params.r, params.r // 4
    q = ((phases_zr(params, sk, rows).astype(np.int64) + Dr // 2) % r) // Dr
    return q != np.asarray(expected, dtype=np.int64).reshape(-1)


def record_zr(params, sk, rows, expected):
    """(rows, wrong, max |e|, sum e, sum e^2, rows with |e| >= Dr/4)."""
    expected = np.asarray(expected).reshape(-1)
    if expected.size == 0:
        return (0, 0, 0, 0, 0, 0)
    e = [int(x) for x in errors_zr(params, sk, rows, expected)]
    Dr = params.r // 4
    return (len(e), int(wrong_zr(params, sk, rows, expected).sum()), max(abs(x) for x in e), sum(e),
            sum(x * x for x in e), sum(abs(x) >= Dr // 4 for x in e))


def _ints128(x):
    x = np.asarray(x, dtype=np.uint64)
    return [int(lo) | (int(hi) << 64) for lo, hi in x.reshape(-1, 2)]


def errors_zq(params, sk, rows, expected):
    """rows [count][n + 1][2] uint64 residues mod Q -> the centred error of every row against the codewords 0 and
    2 DQ_tilde, in (-Q/2, Q/2], as Python ints."""
    n, Q = params.n, params.Q
    rows = np.asarray(rows, dtype=np.uint64).reshape(-1, n + 1, 2)
    s = [int(v) & 1 for v in np.asarray(sk).reshape(-1)]
    out = []
    for row, bit in zip(rows, np.asarray(expected).reshape(-1)):
        v = _ints128(row)
        phase = (v[n] - sum(a for a, k in zip(v[:n], s) if k)) % Q
        d = (phase - int(bit) * 2 * params.DQ_tilde) % Q
        out.append(d - Q if 2 * d > Q else d)
    return out


def record_zq(params, sk, rows, expected):
    """(rows, rows with |e| >= DQ_tilde, max |e|, sum |e|)."""
    e = errors_zq(params, sk, rows, expected)
    if not e:
        return (0, 0, 0, 0)
    return (len(e), sum(abs(x) >= params.DQ_tilde for x in e), max(abs(x) for x in e), sum(abs(x) for x in e))


def handmade_zr(params, sk, rng, errors, bits):
    """One row per (e, bit): uniform a, b = sum a_i s_i + bit Dr + e mod r."""
    n, r = params.n, params.r
    a = rng.integers(0, r, size=(len(errors), n), dtype=np.uint64)
    s = np.asarray(sk, dtype=np.uint64) & np.uint64(1)
    dot = (a * s[None, :]).sum(axis=1, dtype=np.uint64)
    b = (dot.astype(np.int64) + np.asarray(bits, dtype=np.int64) * (r // 4) + np.asarray(errors, dtype=np.int64)) % r
    return np.concatenate([a, b.astype(np.uint64)[:, None]], axis=1)


def boundary_errors(params):
    """The errors a test places by hand: 0, +-1, Dr/4 - 1, Dr/4, Dr/2 - 1, Dr/2, r/2 (and the negatives of the inner
    ones)."""
    Dr, r = params.r // 4, params.r
    return [0, 1, -1, Dr // 4 - 1, Dr // 4, -(Dr // 4), Dr // 2 - 1, -(Dr // 2 - 1), Dr // 2, -(Dr // 2), r // 2]
