"""The numpy mirrors the circuit paths are compared with -- lift_words, modred_words and lwe_not_modq of
sgfhe_jl_amd/circuit.py, which emulate 128 bits in two uint64 and take a quotient from doubles -- against Python integers
at every modulus of tests/ring_cases.py and of Params(64), (1024) and (2048): a Q below 2^24, one just below 2^64, one
of 93 bits, a composite one.  No GPU."""

import types

import numpy as np
import pytest

import lut_ref as LR
import ring_cases as RC


def _moduli():
    import sgfhe_jl_amd as S
    return RC.moduli(S)


MODULI = _moduli()


def _words(vals):
    out = np.zeros((len(vals), 2), dtype=np.uint64)
    out[:, 0] = [v & 0xFFFFFFFFFFFFFFFF for v in vals]
    out[:, 1] = [v >> 64 for v in vals]
    return out


def _ints(arr):
    return [int(lo) | (int(hi) << 64) for lo, hi in np.asarray(arr, dtype=np.uint64).reshape(-1, 2)]


@pytest.mark.parametrize("name", list(MODULI))
def test_lift_words_every_word(name):
    """floor((x Q + r/2) / r) for EVERY x in [0, r); the result is a residue, and ModRed takes it back to x."""
    from sgfhe_jl_amd import circuit as C
    Q, r, _ = MODULI[name]
    x = np.arange(r, dtype=np.uint64)
    got = _ints(C.lift_words(x, Q, r))
    assert got == [(i * Q + r // 2) // r for i in range(r)]
    assert max(got) < Q
    assert np.array_equal(C.modred_words(_words(got), Q, r), x)


@pytest.mark.parametrize("name", list(MODULI))
def test_modred_words_at_every_rounding_threshold(name):
    """Against lut_ref.modred on the lifted words, on 0, Q - 1 and ceil(Q/2) +- 1, and on the residues on either side of
    every threshold ceil((2 k + 1) Q / (2 r)), k < r: the last residue that rounds to k and the first that rounds to
    k + 1 (mod r)."""
    from sgfhe_jl_amd import circuit as C
    Q, r, _ = MODULI[name]
    p = types.SimpleNamespace(Q=Q, r=r)
    thr = [-((-(2 * k + 1) * Q) // (2 * r)) for k in range(r)]
    assert 0 < thr[0] and thr[-1] < Q and all(a < b for a, b in zip(thr, thr[1:]))
    half = (Q + 1) // 2
    vals = [(i * Q + r // 2) // r for i in range(r)] + [0, Q - 1, half - 1, half, half + 1]
    vals += [t - 1 for t in thr] + thr
    got = [int(v) for v in C.modred_words(_words(vals), Q, r)]
    assert got == [LR.modred(v, p) for v in vals]
    assert got[:r] == list(range(r))
    assert got[r + 5:2 * r + 5] == list(range(r))                      # below threshold k: still k
    assert got[2 * r + 5:] == [(k + 1) % r for k in range(r)]          # at it: k + 1, the last one wraps to 0


def _not_rows(Q, DQ):
    """Rows of 5 words (a then b) that hold 0, 1, Q - 1, 2 DQ_tilde and 2 DQ_tilde +- 1 (mod Q), each in a and in b."""
    one = 2 * DQ
    vals = [0, 1, Q - 1, one % Q, (one + 1) % Q, (one - 1) % Q, Q // 2, Q // 2 + 1]
    rows = []
    for i, b in enumerate(vals):
        rows.append([vals[(i + j) % len(vals)] for j in range(1, 5)] + [b])
    return rows


def _check_not(Q, DQ):
    from sgfhe_jl_amd import circuit as C
    rows = _not_rows(Q, DQ)
    x = _words([v for row in rows for v in row]).reshape(len(rows), 5, 2)
    got = _ints(C.lwe_not_modq(x, Q, DQ))
    want = [((Q - v) % Q if j < 4 else (2 * DQ - v) % Q) for row in rows for j, v in enumerate(row)]
    assert got == want
    assert max(got) < Q


@pytest.mark.parametrize("name", list(MODULI))
def test_lwe_not_modq(name):
    Q, _, DQ = MODULI[name]
    _check_not(Q, DQ)


@pytest.mark.parametrize("name", list(MODULI))
def test_lwe_not_modq_with_the_codeword_past_q(name):
    """The ctx accepts any DQ_tilde < Q: at DQ_tilde = floor(Q/2) + 1 the codeword 2 DQ_tilde wraps, and NOT subtracts
    from its residue (the device kernels reduce it too: tests/test_gpu_rings.py)."""
    Q = MODULI[name][0]
    DQ = Q // 2 + 1
    assert 2 * DQ >= Q
    _check_not(Q, DQ)
    _check_not(Q, Q - 1)
