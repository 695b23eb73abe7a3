"""The host side of the noise probe: the restatement of its records (tests/noise_ref.py)
against decrypt(::EncryptedBit) and against rows with hand-placed errors, and the plaintext wire evaluation of
csrc/circuit.h (circuit_plain_bits) against Circuit.evaluate_plain, driven through a stand-alone program under
AddressSanitizer / UndefinedBehaviorSanitizer.  No GPU."""

import os
import shutil
import subprocess

import numpy as np
import pytest

import noise_ref as NR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FALSE, NOT = 0x7FFFFFFF, 0x80000000


def test_wrong_is_zero_exactly_when_decryption_matches(S, oc):
    """Params(64), rows from the oracle -- fresh encryptions and the three gates of 16 bootstraps -- and uniform
    rows: per row, the record's `wrong` against sgfhe_host_decrypt_lwe, for the right and for the flipped bit.
    A uniform row may round to quotient 2 or 3, where the reference's convert(Bool, .) throws and the host
    decryption keeps bit 0 of the quotient: the record counts such a row as wrong whatever the bit."""
    params = S.Params(64)
    n = params.n
    o = oc.Oracle.from_params(params)
    sk = o.private_key(5)
    bkey = o.bootstrap_key(sk, 6)
    bits = np.random.default_rng(7).integers(0, 2, size=32).astype(np.uint8)
    a, b = o.lwe_encrypt_bits(sk, bits, 8)
    fresh = np.concatenate([a, b[:, None]], axis=1)
    res = o.bootstrap_batch(bkey, a[:16], b[:16], a[16:], b[16:])
    x, y = bits[:16], bits[16:]
    gates = np.concatenate([res[:, g] for g in range(3)])
    gate_bits = np.concatenate([x & y, x | y, x ^ y])
    uniform = np.random.default_rng(9).integers(0, params.r, size=(64, n + 1), dtype=np.uint64)
    rows = np.concatenate([fresh, gates, uniform])
    expected = np.concatenate([bits, gate_bits, np.zeros(64, dtype=np.uint8)])
    dec = S.host.decrypt_lwe(params, sk, rows[:, :n], rows[:, n])
    assert np.array_equal(dec[:80], expected[:80])                      # the oracle's rows decrypt
    assert 0 < dec[80:].sum() < 64                                      # the uniform ones to both values
    quot = ((NR.phases_zr(params, sk, rows).astype(np.int64) + params.Dr // 2) % params.r) // params.Dr
    assert quot[:80].max() <= 1 and quot[80:].max() >= 2
    for flip in (0, 1):
        exp = expected ^ flip
        for i in range(len(rows)):
            rec = NR.record_zr(params, sk, rows[i:i + 1], exp[i:i + 1])
            assert rec[0] == 1 and (rec[1] == 0) == (quot[i] <= 1 and dec[i] == exp[i]), (i, flip, rec)
        assert NR.record_zr(params, sk, rows, exp)[1] == int(((dec != exp) | (quot >= 2)).sum())
    rec = NR.record_zr(params, sk, rows[:80], expected[:80])
    assert rec[:2] == (80, 0) and rec[2] < params.Dr // 2 and rec[5] == 0


def test_records_of_hand_placed_errors(S, oc):
    """e = 0, +-1, Dr/4 - 1, +-Dr/4, +-(Dr/2 - 1), +-Dr/2, r/2 on both bits: every field from first principles."""
    params = S.Params(64)
    r, Dr = params.r, params.r // 4
    sk = oc.Oracle.from_params(params).private_key(11)
    errs = NR.boundary_errors(params)
    assert errs == [0, 1, -1, Dr // 4 - 1, Dr // 4, -Dr // 4, Dr // 2 - 1, -(Dr // 2 - 1), Dr // 2, -Dr // 2, r // 2]
    # decryption rounds phase + Dr/2 down to a multiple of Dr: e in [-Dr/2, Dr/2) keeps the bit
    wrong = [e >= Dr // 2 or e < -Dr // 2 for e in errs]
    assert wrong == [False] * 8 + [True, False, True]
    margin = [abs(e) >= Dr // 4 for e in errs]
    for bit in (0, 1):
        rows = NR.handmade_zr(params, sk, np.random.default_rng(12 + bit), errs, [bit] * len(errs))
        assert [int(v) for v in NR.errors_zr(params, sk, rows, [bit] * len(errs))] == errs
        dec = S.host.decrypt_lwe(params, sk, rows[:, :params.n], rows[:, params.n])
        # (e = r/2 rounds to quotient bit + 2: wrong by the rule, while the host decryption keeps bit 0 of it)
        assert [bool(d != bit) for d in dec[:-1]] == wrong[:-1] and dec[-1] == bit
        for i, e in enumerate(errs):
            assert NR.record_zr(params, sk, rows[i:i + 1], [bit]) == (1, int(wrong[i]), abs(e), e, e * e, int(margin[i]))
        assert NR.record_zr(params, sk, rows, [bit] * len(errs)) == \
            (len(errs), sum(wrong), r // 2, sum(errs), sum(e * e for e in errs), sum(margin))
    assert NR.record_zr(params, sk, np.zeros((0, params.n + 1), np.uint64), []) == (0, 0, 0, 0, 0, 0)


def test_zq_record_of_hand_placed_errors(S, oc):
    """Over Z_Q: rows built with chosen errors against the codewords 0 and 2 DQ_tilde."""
    params = S.Params(64)
    n, Q, DQ = params.n, params.Q, params.DQ_tilde
    sk = oc.Oracle.from_params(params).private_key(13)
    rng = np.random.default_rng(14)
    errs = [0, 1, -1, DQ - 1, DQ, -DQ, Q // 2, -(Q // 2)]
    bits = [0, 1, 0, 1, 0, 1, 0, 1]
    rows = np.zeros((len(errs), n + 1, 2), dtype=np.uint64)
    for i, (e, bit) in enumerate(zip(errs, bits)):
        a = [int(rng.integers(0, 1 << 62)) * int(rng.integers(0, 1 << 31)) % Q for _ in range(n)]
        b = (sum(v for v, k in zip(a, sk) if int(k) & 1) + bit * 2 * DQ + e) % Q
        for j, v in enumerate(a + [b]):
            rows[i, j] = (v & (2 ** 64 - 1), v >> 64)
    assert NR.errors_zq(params, sk, rows, bits) == errs
    assert NR.record_zq(params, sk, rows, bits) == (8, 4, Q // 2, sum(abs(e) for e in errs))
    assert NR.record_zq(params, sk, rows[3:4], bits[3:4]) == (1, 0, DQ - 1, DQ - 1)
    assert NR.record_zq(params, sk, rows[4:5], bits[4:5]) == (1, 1, DQ, DQ)


def _probe_circuit(S):
    """NOT on inputs and gate wires, both constants, a pruned node, a wire read twice, an unread input."""
    c = S.Circuit(4)
    x, y, z, _u = c.inputs
    a0, o0, x0 = c.gate(x, ~y)
    a1, o1, x1 = c.gate(z, S.Circuit.TRUE)
    a2, o2, x2 = c.gate(a0, ~o1)
    c.gate(x0, S.Circuit.FALSE)                 # pruned: no output depends on it
    a3, o3, x3 = c.gate(x2, ~x0)
    a4, o4, x4 = c.gate(x0, x0)                 # one wire on both inputs (and read a second time)
    c.output(x3, ~a2, o4, y)
    return c


def _all_wires_circuit(S, c):
    """The same nodes with every input and every wire of every LIVE node as an output: the same pruning, levels
    and rows, and every wire comes out."""
    live = sorted(g for nodes in c.schedule() for g in nodes)
    d = S.Circuit(c.n_inputs)
    for x, y in c.gates:
        d.gate(S.Wire(x), S.Wire(y))
    wires = list(range(c.n_inputs)) + [c.n_inputs + 3 * g + w for g in live for w in range(3)]
    d.output(*[S.Wire(w) for w in wires])
    assert d.schedule() == c.schedule()
    return d, wires


@pytest.mark.parametrize("instances", [1, 64, 70, 130])
def test_plain_wire_bits_under_asan_and_ubsan(S, tmp_path, instances):
    """circuit_plain_bits against Circuit.evaluate_plain, through tests/native/circuit_bits_sanitized.cpp."""
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    src = os.path.join(ROOT, "tests", "native", "circuit_bits_sanitized.cpp")
    inc = os.path.join(ROOT, "sgfhe.jl_amd", "csrc")
    exe = str(tmp_path / "circuit_bits_sanitized")
    b = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", "-I", inc, src, "-o", exe],
                       capture_output=True, text=True, timeout=300)
    if b.returncode != 0 and "sanitize" in b.stderr and "cannot find" in b.stderr:
        pytest.skip("the sanitizer runtimes are not installed: " + b.stderr[-300:])
    assert b.returncode == 0, b.stderr[-3000:]
    c = _probe_circuit(S)
    bits = np.random.default_rng(instances).integers(0, 2, size=(c.n_inputs, instances)).astype(np.uint8)
    text = "%d %d %d %d\n" % (c.n_inputs, c.n_gates, c.n_outputs, instances)
    text += "".join("%d %d\n" % g for g in c.gates) + " ".join(str(o) for o in c.outputs) + "\n"
    text += "".join("".join(str(v) for v in row) + "\n" for row in bits)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    got = {int(line.split()[0]): line.split()[1] for line in r.stdout.strip().splitlines()}
    d, wires = _all_wires_circuit(S, c)
    plain = d.evaluate_plain(bits)
    assert sorted(got) == wires                                   # the pruned node's wires have no row
    assert c.n_inputs + 3 * 3 not in got
    for w, row in zip(wires, plain):
        assert got[w] == "".join(str(int(v)) for v in row), w
