"""LUT bootstraps and LUT nodes (sgfhe_bootstrap_lut_batch, sgfhe_circuit_create_lut; include/sgfhe_hip.h, DESIGN.md
section 11) without a device: the exports and their declarations, the combinatorics of `lut_ref` over all 256 tables,
`lut_ref.rows_from_acc` on the accumulators of the low-amplitude C oracle decrypting to the table entry at all three
scales in both flatten modes; the planner's validation through ctypes, Circuit.lut / fan against the table, the second
callback of replay_levels, and the planner with circuit_plain_bits under ASan / UBSan
(tests/native/circuit_lut_sanitized.cpp)."""

import os
import re

import numpy as np

import lut_ref as LR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TABLES = (0x00, 0xFF, 0x96, 0xE8, 0xCA, 0xF0, 0x10, 0xAA, 0x01, 0x80, 0x55, 0x7F)


def test_export_and_declaration(S):
    L = S.lib()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sgfhe_hip.h")).read(), flags=re.S)
    name, arity = "sgfhe_bootstrap_lut_batch", 7
    assert name in S.EXPORTED_SYMBOLS and hasattr(L, name)
    m = re.search(r"int32_t\s+%s\s*\(([^)]*)\)\s*;" % name, hdr)
    assert m, "the header does not declare %s" % name
    assert len(m.group(1).split(",")) == arity
    assert len(getattr(L, name).argtypes) == arity
    assert L.sgfhe_abi_version() == 7          # an entry point is only added
    assert L.sgfhe_bootstrap_lut_batch(None, None, None, None, 1, None, 0) == -1


def test_every_table_is_a_combination_of_steps():
    """All 256 tables, s in 0..15: the combination of ideal steps is sigma(s mod 8) (-1)^(s div 8); the transitions are
    an odd number, at most 7; 0x10 has them at j = 4 and 5 (and 8)."""
    for table in range(256):
        js = LR.transitions(table)
        assert len(js) % 2 == 1 and len(js) <= 7
        assert len(LR.kappas(table)) == len(js)
        for s in range(16):
            assert LR.ideal_combination(table, s) == LR.sigma(table, s % 8) * (-1) ** (s // 8), (table, s)
    assert LR.transitions(0x10) == [4, 5, 8]
    assert LR.transitions(0x00) == [8] and LR.transitions(0xFF) == [8]
    assert len(LR.transitions(0x55)) == 7 and len(LR.transitions(0xAA)) == 7


def test_coefficients_fold_and_wrap(S):
    """c(j) at Params(64) and Params(1024): j <= 4 lies in the negated half, j = 4 folds to Dr/8 < n, so c(4) - e runs
    below 0 for a words."""
    for n in (64, 1024):
        p = S.Params(n)
        Dr, m = p.r // 4, p.m
        cs = [LR.coefficient(p, j) for j in range(1, 9)]
        assert cs == [3 * Dr - (2 * j - 1) * Dr // 8 for j in range(1, 9)]
        assert all(c >= m for c in cs[:4]) and all(c < m for c in cs[4:])
        assert cs[3] - m == Dr // 8 and cs[3] - m < p.n


def _rows(params, sk, seed):
    """All 8 sums with the errors 0, +-(Dr/8 - 1) and a few between, every table of TABLES on every sum."""
    Dr = params.r // 4
    lim = Dr // 8 - 1
    errs = (0, lim, -lim, 1, -1, lim // 2, -(lim // 3))
    s, e, t = [], [], []
    k = 0
    for table in TABLES:
        for sv in range(8):
            s.append(sv)
            e.append(errs[k % len(errs)])
            t.append(table)
            k += 1
    a, b = LR.rows_at(params, sk, s, e, np.random.default_rng(seed))
    return a, b, np.array(s), np.array(t, dtype=np.uint8)


def test_rows_from_acc_on_the_low_amplitude_oracle(S, oc):
    """Params(64), both flatten modes: every scale decrypts to the table entry, the raw rows reduce to the reduced rows,
    and the Z_r error stays within a few units of the codeword Dr = 256."""
    params = S.Params(64)
    o = oc.Oracle.from_params(params)
    lo = LR.low_oracle(oc, params)
    sk = o.private_key(31)
    bkey = o.bootstrap_key(sk, 32)
    a, b, s, tables = _rows(params, sk, 33)
    z = np.zeros_like(a), np.zeros_like(b)
    want = np.array([(int(t) >> int(sv)) & 1 for t, sv in zip(tables, s)])
    for rnd in (None, (77, 0)):
        _, acc = lo.bootstrap_batch(bkey, a, b, z[0], z[1], want_acc=True, rnd=rnd)
        rows = LR.rows_from_acc(params, acc, tables)
        raw = LR.rows_from_acc(params, acc, tables, raw=True)
        for k in range(3):
            assert np.array_equal(LR.decrypt_scaled(params, sk, rows[:, k], k), want), (rnd, k)
            # the CPU experiment behind the header's noise rule recorded at most 5 of Dr = 256 here (other rows, another
            # key); 9 adds twice the standard deviation of ModRed's rounding over the key's ~n/2 words, sqrt(33 / 12)
            # = 1.7.  A scaled row's error does not grow with its scale
            assert np.abs(LR.phase_errors(params, sk, rows[:, k], want, k)).max() <= 9, (rnd, k)
        vals = [int(lo_) | (int(hi) << 64) for lo_, hi in raw.reshape(-1, 2)]
        assert all(v < params.Q for v in vals)
        assert [LR.modred(v, params) for v in vals] == [int(x) for x in rows.reshape(-1)]


# ---- LUT nodes in circuits (sgfhe_circuit_create_lut) ------------------------------------------------------------

import ctypes
import shutil
import subprocess

import pytest

ERR_INVALID_ARG = -1
FALSE = 0x7FFFFFFF
NOT = 0x80000000


def _p(x):
    return None if x is None else x.ctypes.data_as(ctypes.c_void_p)


def _arrays(nodes, outs):
    """nodes: [(kind, table, [(weight, ref, shift), ...])]."""
    kind = np.array([k for k, _, _ in nodes], dtype=np.uint32)
    table = np.array([t for _, t, _ in nodes], dtype=np.uint32)
    st = np.cumsum([0] + [len(t) for _, _, t in nodes]).astype(np.uint32)
    tw = np.array([w for _, _, t in nodes for w, _, _ in t], dtype=np.int32)
    tr = np.array([r for _, _, t in nodes for _, r, _ in t], dtype=np.uint32)
    ts = np.array([d for _, _, t in nodes for _, _, d in t], dtype=np.int32)
    return kind, st, tr, ts, tw, table, np.array(outs, dtype=np.uint32)


def _create_lut(L, n_inputs, nodes, outs, group=1, table=True):
    kind, st, tr, ts, tw, tb, o = _arrays(nodes, outs)
    h = ctypes.c_void_p(0xDEAD)
    rc = L.sgfhe_circuit_create_lut(n_inputs, _p(kind), _p(st), _p(tr), _p(ts), _p(tw), _p(tb) if table else None,
                                    len(nodes), _p(o), None, len(o), group, ctypes.byref(h))
    return rc, h


def _create_w(L, n_inputs, nodes, outs, group=1):
    kind, st, tr, ts, tw, _, o = _arrays(nodes, outs)
    h = ctypes.c_void_p(0xDEAD)
    rc = L.sgfhe_circuit_create_w(n_inputs, _p(kind), _p(st), _p(tr), _p(ts), _p(tw), len(nodes), _p(o), None, len(o),
                                  group, ctypes.byref(h))
    return rc, h


def _info(L, h):
    info = (ctypes.c_uint64 * 4)()
    assert L.sgfhe_circuit_info(h, info) == 0
    return list(info)


def test_create_lut_validation(S):
    """Every violation of the scale rule, a table of 256 and a LUT node without exactly three unit-weight terms are
    SGFHE_ERR_INVALID_ARG with *out NULL; sgfhe_circuit_create_w keeps rejecting kind 2."""
    L = S.lib()
    name, arity = "sgfhe_circuit_create_lut", 13
    assert name in S.EXPORTED_SYMBOLS and len(getattr(L, name).argtypes) == arity
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sgfhe_hip.h")).read(), flags=re.S)
    m = re.search(r"int32_t\s+%s\s*\(([^)]*)\)\s*;" % name, hdr)
    assert m and len(m.group(1).split(",")) == arity
    # 3 inputs; node 0 = fan(in 0): wires 3, 4, 5 at scales 0, 1, 2; node 1 = lut(5, ~4, 3): wires 6, 7, 8
    def good(r0=5, r1=NOT | 4, r2=3, table=0xCA, w=(1, 1, 1), kind1=2, fan0=FALSE, extra=()):
        return [(2, 0xF0, [(1, fan0, 0), (1, FALSE, 0), (1, 0, 0)]),
                (kind1, table, [(w[0], r0, 0), (w[1], r1, 0), (w[2], r2, 0)] + list(extra))]
    outs = [6, NOT | 3, 1]
    rc, h = _create_lut(L, 3, good(), outs)
    assert rc == 0 and _info(L, h)[:3] == [2, 2, 1]
    L.sgfhe_circuit_destroy(h)

    def refused(nodes, outputs=outs, **kw):
        rc, h = _create_lut(L, 3, nodes, outputs, **kw)
        assert rc == ERR_INVALID_ARG and h.value is None, (nodes, outputs, kw)

    for bad in (dict(r0=4), dict(r0=3), dict(r0=1), dict(r0=NOT | 2),          # position 0 reads scale 1, 0, inputs
                dict(r1=5), dict(r1=3), dict(r1=NOT | 0),                        # position 1 reads scale 2, 0, an input
                dict(r2=4), dict(r2=NOT | 5),                                    # position 2 reads scale 1, 2
                dict(fan0=0), dict(fan0=NOT | 1),                                # a fan reading an input at position 0
                dict(table=256), dict(table=2 ** 32 - 1),
                dict(w=(2, 1, 1)), dict(w=(1, -1, 1)), dict(w=(1, 1, 0)),
                dict(kind1=3), dict(extra=[(1, FALSE, 0)]),                      # kind above 2; four terms
                dict(r0=6), dict(r2=9)):                                         # its own node; no wire at all
        refused(good(**bad))
    refused([good()[0], (2, 0xCA, [(1, 5, 0), (1, 4, 0)])])                     # a LUT node of two terms
    refused(good(), outputs=[7])                                                 # an output of scale 1
    refused(good(), outputs=[6, NOT | 8])                                        # ... of scale 2
    refused(good() + [(0, 0, [(1, 6, 0), (1, 7, 0)])])                           # a classic node reading scale 1
    refused(good() + [(1, 0, [(2, 6, 0), (1, 8, 0)])])                           # a sum node reading scale 2
    refused(good(), table=False)                                                 # NULL node_table
    rc, h = _create_lut(L, 3, good() + [(0, 0, [(1, 6, 0), (1, NOT | 3, 0)]), (1, 0, [(2, 6, 0), (1, 9, 0)])], [12, 6])
    assert rc == 0 and _info(L, h)[:3] == [4, 4, 1]
    L.sgfhe_circuit_destroy(h)
    rc, h = _create_w(L, 3, good(), outs)                                        # kind 2 through sgfhe_circuit_create_w
    assert rc == ERR_INVALID_ARG and h.value is None


def test_plan_without_lut_nodes_is_the_create_w_plan(S):
    """The same arrays through both entries: the same info (levels, nodes, widest, slots) and group, and the same
    bytes from a run are checked on the device; table by table under the sanitizers (circuit_lut_sanitized.cpp)."""
    L = S.lib()
    from sgfhe_jl_amd import circuit as C
    c = C.crc16_ccitt(16)
    nodes = [(0 if c.kind(g) == "classic" else 1, 0x12345, list(zip(c.weights(g), c.gates[g], c.gate_shifts[g])))
             for g in range(c.n_gates)]
    rc, h = _create_lut(L, c.n_inputs, nodes, c.outputs)
    rc2, h2 = _create_w(L, c.n_inputs, nodes, c.outputs)
    assert rc == 0 and rc2 == 0 and _info(L, h) == _info(L, h2) == [c.info()[k] for k in ("levels", "nodes", "widest", "slots")]
    L.sgfhe_circuit_destroy(h)
    L.sgfhe_circuit_destroy(h2)


def _mixed_circuit(S):
    c = S.Circuit(3, group=2)
    rx, ry, rz = (c.refresh(w) for w in c.inputs)
    fx, fy, fz = c.fan(rx), c.fan(ry), c.fan(rz)
    mux = c.lut(0xCA, fx[2], ~fy[1].lane(1), fz[0])
    g = c.gate(rx, ~ry)
    s = c.sum_node([(2, g[0]), (1, mux[0]), (-1, rz)])
    t = c.lut(0x2D, mux[2].lane(-1), S.Circuit.TRUE, s[1])
    dead = c.lut(0xFF, fx[2], fy[1], fz[0])                    # pruned
    c.output(t[0], ~mux[0], s[2], g[2].lane(1))
    return c, dead


def test_circuit_lut_python_model(S):
    """Circuit.lut / fan: the scale rule raises ValueError; kind, schedule and info agree with the C plan; evaluate_plain
    is bit s of the table."""
    c, dead = _mixed_circuit(S)
    assert c.has_lut and [c.kind(g) for g in range(c.n_gates)] == ["sum"] * 3 + ["lut"] * 4 + ["classic", "sum", "lut", "lut"]
    sched = c.schedule()
    info = c.info()
    assert info["levels"] == len(sched) == 5 and info["nodes"] == sum(len(l) for l in sched) == c.n_gates - 1
    assert info["widest"] == max(len(l) for l in sched) and (dead[0].id - 3) // 3 not in [g for l in sched for g in l]
    fx = S.Wire(3 + 3 * 3), S.Wire(3 + 3 * 3 + 1), S.Wire(3 + 3 * 3 + 2)
    assert [c.scale(w) for w in fx] == [0, 1, 2] and c.scale(S.Circuit.TRUE) is None and c.scale(c.inputs[0]) == 0
    for bad in (lambda: c.lut(1, fx[0], fx[1], fx[0]), lambda: c.lut(1, fx[2], fx[2], fx[0]),
                lambda: c.lut(1, fx[2], fx[1], fx[1]), lambda: c.gate(fx[1], fx[0]), lambda: c.gate3(fx[0], fx[0], fx[2]),
                lambda: c.sum_node([(1, fx[1])]), lambda: c.xor(fx[0], fx[2]), lambda: c.output(fx[1]),
                lambda: c.lut(256, fx[2], fx[1], fx[0]), lambda: c.lut(-1, fx[2], fx[1], fx[0]), lambda: c.fan(fx[1])):
        with pytest.raises(ValueError):
            bad()
    c, _ = _mixed_circuit(S)                                   # (the refused calls above appended nothing that is live)
    bits = np.random.default_rng(5).integers(0, 2, size=(3, 8)).astype(bool)
    x, y, z = bits
    from sgfhe_jl_amd.circuit import lane_shift
    mux = np.where(x, ~lane_shift(y, 1, 2), z)                 # 0xCA: x0 ? x1 : x2, x1 = ~(y shifted, FALSE outside)
    g_and, g_xor = x & ~y, x ^ ~y
    sv = (2 * g_and.astype(int) + mux.astype(int) - z.astype(int)) % 4
    s_mid, s_low = (sv == 1) | (sv == 2), sv % 2 == 1
    idx = lane_shift(mux, -1, 2).astype(int) + 2 + 4 * s_mid.astype(int)
    t = ((0x2D >> idx) & 1).astype(bool)
    assert np.array_equal(c.evaluate_plain(bits), np.stack([t, ~mux, s_low, lane_shift(g_xor, 1, 2)]))
    f = S.Circuit(1)
    f.output(f.fan(f.inputs[0])[0])
    assert np.array_equal(f.evaluate_plain([[0, 1]]), [[False, True]]) and f.gate_tables == {0: 0xF0}


def test_replay_levels_hands_lut_rows_to_the_second_callback(S):
    """The LUT rows of a call, their tables and their indices within the call; `boot` sees every row of a mixed call
    and is not called for a call of LUT rows only."""
    from sgfhe_jl_amd import circuit as C
    c = S.Circuit(2)
    x, y = c.inputs
    fx = c.fan(x)
    g = c.gate(x, y)
    fy = c.fan(y)
    m = c.lut(0x96, fx[2], ~fy[1], g[0])
    c.output(m[0])
    n, r, inst = 4, 64, 3
    inputs = np.random.default_rng(6).integers(0, r, size=(2, inst, n + 1), dtype=np.uint64)
    log = []

    def boot(call, a1, b1, a2, b2):
        log.append(("boot", call, len(b1)))
        return np.zeros((len(b1), 3, n + 1), dtype=np.uint64)

    def boot_lut(call, a, b, tables, idx):
        log.append(("lut", call, list(tables), list(idx)))
        out = np.zeros((len(b), 3, n + 1), dtype=np.uint64)
        out[:, :, :n] = a[:, None, :]
        out[:, :, n] = b[:, None]
        return out

    out = C.replay_levels(c, inputs, r, boot, boot_lut)
    assert log == [("boot", 0, 9), ("lut", 0, [0xF0] * 3 + [0xF0] * 3, [0, 1, 2, 6, 7, 8]), ("lut", 1, [0x96] * 3, [0, 1, 2])]
    # the stand-in returns its input sum on all three wires: level 2 saw x + (Dr/2 - y) + 0, b word included
    want = (inputs[0] - inputs[1]) % r
    want[:, n] = (want[:, n] + r // 8) % r
    assert np.array_equal(out[0], want)


def test_lut_planner_under_asan_and_ubsan(tmp_path):
    """tests/native/circuit_lut_sanitized.cpp: random mixed circuits under the scale rule, circuit_plain_bits against a
    per-instance evaluation, the kind words, the plan without LUT nodes against the sgfhe_circuit_create_w plan, and
    the refused inputs without an allocation.  A child process of its own; the same program without the sanitizers
    compares as many bits."""
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    src = os.path.join(ROOT, "tests", "native", "circuit_lut_sanitized.cpp")
    inc = os.path.join(ROOT, "sgfhe.jl_amd", "csrc")
    exe = str(tmp_path / "circuit_lut_sanitized")
    b = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", "-I", inc, src, "-o", exe],
                       capture_output=True, text=True, timeout=300)
    if b.returncode != 0 and "sanitize" in b.stderr and "cannot find" in b.stderr:
        pytest.skip("the sanitizer runtimes are not installed: " + b.stderr[-300:])
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    env.pop("LD_PRELOAD", None)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    tag, compared = r.stdout.split()
    assert tag == "ok" and int(compared) > 50000
    exe2 = str(tmp_path / "circuit_lut_plain")
    subprocess.run([gxx, "-std=c++17", "-O2", "-I", inc, src, "-o", exe2], check=True, timeout=300)
    r2 = subprocess.run([exe2], capture_output=True, text=True, timeout=300)
    assert r2.returncode == 0 and r2.stdout == r.stdout
