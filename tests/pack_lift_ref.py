"""What the tests of the lifted pack stage share (tests/test_pack_lift_host.py, tests/test_gpu_pack_lift.py): the circuit
whose outputs take every path of the stage under SGFHE_CIRCUIT_PACK_LIFT, and input ciphertexts crafted with a chosen
error bound."""

import numpy as np


def lift_circuit(S, width=3):
    """ripple_adder(width) -- sum bits are XOR3 wires (lifted), the carry-out a MAJ wire (direct) -- extended with an
    input, a negated input, TRUE and a negated XOR3 wire (all lifted).  Returns (circuit, lifted): lifted[o] tells
    whether output o is lifted."""
    c = S.ripple_adder(width)
    outs = [S.Wire(ref) for ref in c.outputs]
    c.output(*(outs + [c.inputs[0], ~c.inputs[width + 1], S.Circuit.TRUE, ~outs[1]]))
    return c, [True] * width + [False] + [True] * 4


def craft_cts(S, params, sk, bits, seed, N=None, bound=None):
    """bits [n_inputs][blocks][n] -> RLWE (a, b), each [n_inputs][blocks][N] (N = n or m): a uniform over Z_r and
    b = a s + bit Dr + e with e uniform in [-bound, bound] (default Dr / 16) on the n message coefficients -- the LWE
    split_ciphertext extracts for bit i has exactly the error e_i.  Not encrypt_private, whose rounding of b alone
    costs Dr / 8."""
    from sgfhe_jl_amd.scheme import split_ciphertext_array
    n, r = params.n, params.r
    N = n if N is None else N
    bound = params.Dr // 16 if bound is None else bound
    rng = np.random.default_rng(seed)
    bits = np.asarray(bits, dtype=np.uint64)
    a = rng.integers(0, r, size=bits.shape[:2] + (N,), dtype=np.uint64)
    b = rng.integers(0, r, size=bits.shape[:2] + (N,), dtype=np.uint64)      # (the coefficients past n are not read)
    rows = split_ciphertext_array(a, np.zeros_like(a), n, r)[..., :n]        # [..., bit][j]: the LWE's a
    s = np.asarray(sk, dtype=np.uint64) & np.uint64(1)
    e = rng.integers(-bound, bound + 1, size=bits.shape).astype(np.int64).astype(np.uint64)
    b[..., :n] = (rows @ s + bits * np.uint64(params.Dr) + e) & np.uint64(r - 1)
    return a, b


def lwe_errors(params, sk, lwe, bits):
    """Centred Z_r errors of LWEs [..., n + 1] against their plaintext bits [...]."""
    n, r = params.n, params.r
    lwe = np.asarray(lwe, dtype=np.uint64)
    s = np.asarray(sk, dtype=np.uint64) & np.uint64(1)
    d = (lwe[..., n] - lwe[..., :n] @ s - np.asarray(bits, dtype=np.uint64) * np.uint64(params.Dr)) & np.uint64(r - 1)
    d = d.astype(np.int64)
    return np.where(d > r // 2, d - r, d)


def widen_cts(a, b, m, seed):
    """RLWE (a, b) [..., n] -> the Ciphertext form [..., m] that split_ciphertext takes to the SAME LWEs: a[d] stays
    for 0 <= d < n and -a[n + d] moves to -a[m + d] for -n < d < 0; the coefficients in between, and b past n, are
    never read and get random words.  One oracle reference then serves N = n and N = m."""
    n = a.shape[-1]
    rng = np.random.default_rng(seed)
    hi = int(max(a.max(), b.max())) + 1
    am = rng.integers(0, hi, size=a.shape[:-1] + (m,), dtype=np.uint64)
    bm = rng.integers(0, hi, size=a.shape[:-1] + (m,), dtype=np.uint64)
    am[..., :n] = a
    am[..., m - n + 1:] = a[..., 1:]
    bm[..., :n] = b
    return am, bm
