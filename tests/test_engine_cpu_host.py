"""The engine built for the CPU, every kernel under AddressSanitizer and UBSan.  No GPU.

csrc/engine.hip and its kernel headers compile unchanged as host C++ against the HIP stand-in of tests/native/hipcpu
(hipMalloc is an exact malloc, dynamic LDS an exact heap block, the threads of a block OS threads, buffer resources
range-checked and counted, readfirstlane checked for uniformity) and are driven through the C ABI by
tests/native/engine_cpu_driver.cpp.  tests/engine_cpu.py puts a running sanitized driver where the ctypes library stands,
so the calls below are made by Engine and Circuit themselves, and -- where a GPU test of the same thing exists -- by that
test's own function on its own cases and references (tests/test_gpu_rings.py, test_gpu_kloop_step.py,
test_gpu_entry_exit.py), on the rings of tests/ring_cases.py.  For every session:

  * the sanitized run ends clean (any report aborts it; LeakSanitizer runs at its exit, after every ctx is destroyed),
  * every result equals its reference, word for word, while the run goes,
  * the same call list run again, sanitized with device memory pre-filled with 0xA5 instead of 0x00, gives the same
    bytes: nothing depends on device memory (or dynamic LDS) that nothing wrote,
  * and so does the plain -O2 build.

The last test holds the kernels the driver launched to the list of __global__ functions in kernels.h; OMITTED names the
ones no session reaches, with the reason.
"""

import contextlib
import os
import re

import numpy as np
import pytest

import engine_cpu as EC
import ring_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAUNCHED = {}
SESSIONS = []


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    d = tmp_path_factory.mktemp("engine_cpu")
    exes = {}
    for tag, flags in (("san", EC.SAN_FLAGS), ("plain", EC.PLAIN_FLAGS)):
        exes[tag] = str(d / ("engine_cpu_" + tag))
        why = EC.build(exes[tag], flags)
        if why:
            pytest.skip(why)
    return exes["san"], exes["plain"], d


@contextlib.contextmanager
def session(S, drivers, name):
    """The binding's library is a sanitized driver for the length of the block; at its end the three-run comparison."""
    ses = EC.Session(drivers[0], drivers[1], drivers[2], name)
    before, S._lib._lib = S._lib._lib, ses
    try:
        yield ses
        for k, v in ses.finish().items():
            LAUNCHED[k] = LAUNCHED.get(k, 0) + v
        SESSIONS.append(name)
    finally:
        S._lib._lib = before
        if ses.proc.poll() is None:
            ses.proc.kill()


def _getter(make):
    made = {}

    def get(name, *a):
        if name not in made:
            made[name] = make(name, *a)
        return made[name]
    get.made = made
    return get


# ---- the marshalling itself ------------------------------------------------------------------------------------------------

def test_argument_records_of_the_session():
    """Session._arg without a driver: what each kind of argument the binding passes becomes in the call list, and that
    anything else is refused."""
    import ctypes
    import struct
    ses = EC.Session.__new__(EC.Session)
    ses.live, ses.known, ses._next_id = {}, {}, 1
    rec = lambda a, name="sgfhe_x", last=False: ses._arg(name, a, last)
    assert rec(None) == (b"\x02", None) and rec(ctypes.c_void_p(None)) == (b"\x02", None)
    assert rec(7) == (struct.pack("<Bq", 0, 7), None) and rec(True)[0] == struct.pack("<Bq", 0, 1)
    assert rec(ctypes.c_size_t(9))[0] == struct.pack("<Bq", 0, 9)
    data, sink = rec(b"abc")
    assert data == struct.pack("<BQ", 1, 3) + b"abc" and sink(b"xyz") is None
    arr = np.arange(6, dtype=np.uint32).reshape(2, 3)
    data, sink = rec(arr.ctypes.data_as(ctypes.c_void_p))
    assert data == struct.pack("<BQ", 1, 24) + arr.tobytes()
    sink(np.full(6, 5, dtype=np.uint32).tobytes())
    assert (arr == 5).all()                                          # a returned buffer lands in the caller's array
    with pytest.raises(AssertionError):
        rec(arr.T.ctypes.data_as(ctypes.c_void_p))                   # not contiguous: no size to go by
    n = ctypes.c_size_t(4)
    data, sink = rec(ctypes.byref(n))
    assert data == struct.pack("<BQ", 1, 8) + struct.pack("<Q", 4)
    sink(struct.pack("<Q", 11))
    assert n.value == 11
    buf = ctypes.create_string_buffer(5)
    assert rec(buf)[0] == struct.pack("<BQ", 1, 5) + bytes(5)
    h = ctypes.c_void_p()
    assert rec(ctypes.byref(h), "sgfhe_ctx_create_ex", True) == (struct.pack("<BI", 4, 1), None) and ses.live == {1: "ctx"}
    assert rec(h) == (struct.pack("<BI", 3, 1), None) and rec(h.value) == (struct.pack("<BI", 3, 1), None)
    c = ctypes.c_void_p()
    assert rec(ctypes.byref(c), "sgfhe_circuit_create3", True)[0] == struct.pack("<BI", 4, 2) and ses.live[2] == "circuit"
    assert rec(h.value + 1)[0][0] == 0                               # no handle: a plain integer
    with pytest.raises(AssertionError):
        rec(ctypes.c_void_p(arr.ctypes.data))                        # a bare pointer nobody named
    ses.register(arr, device=True)
    assert rec(ctypes.c_void_p(arr.ctypes.data))[0] == struct.pack("<BQ", 5, 24) + arr.tobytes()
    assert rec(arr.ctypes.data)[0][0] == 5
    ses.known.clear()
    with pytest.raises(AssertionError):
        rec(3.5)


# ---- a. whole bootstraps against the C oracle ----------------------------------------------------------------------------

BATCHES = (1, 7, 8, 9, 17)


def _rows(p, rng, batch):
    a = rng.integers(0, p.r, size=(2, batch, p.n)).astype(np.uint64)
    b = rng.integers(0, p.r, size=(2, batch)).astype(np.uint64)
    return a[0], b[0], a[1], b[1]


@pytest.mark.parametrize("name", RC.NAMES)
def test_bootstraps_equal_the_oracle(S, oc, drivers, name):
    """Both key routes (the oracle's key uploaded, in limb pairs on `composite`; the key generated on the device from
    the oracle's seed), both flatten modes, 1, 7, 8, 9 and 17 gates, reduced and un-reduced; then the throughput form
    alone (set_small_batch_max(0)) and chunks of 8 on one lane and on two, a ragged last chunk on each."""
    import test_gpu_rings as TR
    with session(S, drivers, "bootstraps-" + name):
        case = TR.Case(S, oc, name)
        p, rg = case.params, case.rg
        seed = TR.SK_SEED[name] + 1
        gen = S.Engine(p)
        gen.generate_key(case.sk, seed, noise=rg.noise)
        rng = np.random.default_rng(900 + p.n)
        rows = {batch: _rows(p, rng, batch) for batch in BATCHES + (19,)}

        def want(batch, rnd, raw):
            return case.o.bootstrap_batch(case.khat, *rows[batch], raw=raw, opt=True, rnd=(RC.KEY32, 0) if rnd else None)

        for eng in (case.eng, gen):
            for rnd in RC.MODES:
                assert RC.set_mode(S, eng, rg, rnd)
                for batch in BATCHES:
                    for raw in (False, True):
                        RC.set_mode(S, eng, rg, rnd)                      # the call counter starts again
                        got = eng.bootstrap_batch(*rows[batch], raw=raw)
                        assert np.array_equal(got, want(batch, rnd, raw)), (name, rnd, batch, raw)
                for knobs in (dict(small=0), dict(chunk=8, lanes=1), dict(chunk=8, lanes=2)):
                    eng.set_small_batch_max(knobs.get("small", 24))
                    eng.set_lanes(knobs.get("lanes", 2))
                    eng.set_chunk(knobs.get("chunk", 0))
                    RC.set_mode(S, eng, rg, rnd)
                    batch = 19 if "chunk" in knobs else 9
                    assert np.array_equal(eng.bootstrap_batch(*rows[batch]), want(batch, rnd, False)), (name, rnd, knobs)
                eng.set_small_batch_max(24)
                eng.set_lanes(2)
                eng.set_chunk(0)
            eng.set_random_flatten(False)
        gen.close()
        case.close()


# ---- b. every k-loop form, one step each ------------------------------------------------------------------------------------

KLOOP_OBSERVED = set()         # kernel names the steps of this file reported (the GPU file's own set stays its own)


@contextlib.contextmanager
def _observed_here(TK):
    """TK.OBSERVED is this file's set for the length of the block, so that steps a GPU run made do not count here."""
    theirs, TK.OBSERVED = TK.OBSERVED, KLOOP_OBSERVED
    try:
        yield
    finally:
        TK.OBSERVED = theirs


@pytest.mark.parametrize("name", RC.NAMES)
def test_kloop_steps_on_the_small_rings(S, drivers, name):
    """tests/test_gpu_kloop_step.py's test_small_rings, both modes: the latency pair, the small form, k_extprod, every CRT
    kind of the five rings, each held to the kernel pair its form table names."""
    import test_gpu_kloop_step as TK
    with _observed_here(TK), session(S, drivers, "kloop-" + name):
        get = _getter(lambda n, params=None: TK.Ctx(S, params() if params else RC.ring(S, n).params))
        for rnd in RC.MODES:
            TK.test_small_rings(get, name, rnd)
        for c in get.made.values():
            c.eng.close()


# (ring, randomised, gate counts) of test_gpu_kloop_step.BIG_CASES that run here: one case of every kernel pair the small
# rings do not reach.  Sanitized live run + the two replays, 8 cores: p512 28-35 s, p1024 see RESULTS.md, p2048 16-86 s.
# Left out for time, their kernel pairs all covered by a case that stays: the second p512 case of each mode ((12, 13):
# the fused kernel's cap), p1024 (1, 7, 12), (25,) and randomised (10, 11), and every `two-limb` case.
QUARTER_CASES = [("p512", False, (1, 6, 7)), ("p512", True, (1, 6, 7)), ("p1024", False, (13,)), ("p1024", True, (1, 7)),
                 ("p2048", False, (1, 7)), ("p2048", True, (1,))]


@pytest.mark.parametrize("name,rnd,counts", QUARTER_CASES,
                         ids=["%s-%s-%s" % (n, RC.MODE_IDS[r], "+".join(map(str, cs))) for n, r, cs in QUARTER_CASES])
def test_kloop_steps_on_the_quarter_rings(S, drivers, name, rnd, counts):
    """tests/test_gpu_kloop_step.py's test_quarter_rings at m = 4096, 8192 and 16384, one step each: k_fwd_quarter,
    k_inv_quarter, k_ext_quarter, k_crt_lean1q, the 87-bit k_crt_lean and the WIDE forms under the sanitizers."""
    import test_gpu_kloop_step as TK
    assert (name, rnd, counts) in TK.BIG_CASES
    with _observed_here(TK), session(S, drivers, "kloop-%s-%d-%s" % (name, rnd, "+".join(map(str, counts)))):
        get = _getter(lambda n, params=None: TK.Ctx(S, params() if params else RC.ring(S, n).params))
        TK.test_quarter_rings(S, get, name, rnd, counts)
        for c in get.made.values():
            c.eng.close()


def test_every_kloop_kernel_pair_was_reported():
    """As the GPU file ends: the union of the kernel pairs the steps above reported covers the k-loop's list."""
    import test_gpu_kloop_step as TK
    need = {"kloop-" + n for n in RC.NAMES} | {"kloop-%s-%d-%s" % (n, r, "+".join(map(str, cs))) for n, r, cs in QUARTER_CASES}
    if not need <= set(SESSIONS):
        pytest.skip("not every k-loop session of this file ran before this test")
    with _observed_here(TK):
        TK.test_every_kloop_kernel_was_observed()


# ---- c. the entry and the exit of a chunk ---------------------------------------------------------------------------------

@pytest.mark.parametrize("name", RC.NAMES)
def test_chunk_entry_and_exit(S, drivers, name):
    """tests/test_gpu_entry_exit.py on its rows (tests/exit_cases.py): classic rows, LUT rows, the family of 256 tables,
    the entry; both modes; the RNS2 form on `composite`."""
    import test_gpu_entry_exit as TE
    with session(S, drivers, "entry-exit-" + name):
        get = _getter(lambda n: TE.Ctx(S, n))
        for rnd in RC.MODES:
            TE.test_classic_rows(get, name, rnd)
            TE.test_lut_rows(get, name, rnd)
            TE.test_entry(get, name, rnd)
        for c in get.made.values():
            c.eng.close()


# ---- d. circuits, the LUT primitive, the lift and the noise probe ----------------------------------------------------------------

# (one session per ring: minutes each under the sanitizers, most of it in the 256-thread blocks of the glue and probe
# kernels; RESULTS.md has the figures)
@pytest.mark.parametrize("name", RC.NAMES)
def test_circuits_lut_lift_and_probe(S, oc, drivers, name):
    """tests/test_gpu_rings.py on one ring: the lift of every word, the LUT primitive on all 256 tables, the mixed circuit
    in the LWE form and in the ciphertext form (plain, PACK_DIRECT, PACK_DIRECT | PACK_LIFT), sgfhe_lwe_noise over Z_r and
    Z_Q with the stride form, and sgfhe_circuit_run_probe on every wire."""
    import test_gpu_rings as TR
    with session(S, drivers, "rings-" + name):
        case = TR.Case(S, oc, name)
        TR.test_lwe_lift_every_word(case)
        TR.test_lwe_noise_primitive(case)
        for rnd in RC.MODES:
            TR.test_lut_primitive(case, rnd)
            TR.test_mixed_circuit_lwe_form(case, rnd)
            TR.test_mixed_circuit_ciphertext_form(case, rnd)
            TR.test_circuit_probe_every_wire(case, rnd)
        case.close()


def test_scripted_circuit_runs(S, drivers):
    """tests/test_gpu_circuit_script.py on the cases of tests/circuit_script_cases.py, through sgfhe_debug_circuit_script
    on ctxs without a key: every reference form through one gather, sum nodes, LUT NOT and data planes, the scatter, a
    level across two calls with routes over the boundary, un-reduced calls on `tiny` and `wide`, a raw call split inside
    a node, the lift of every kind of output, the split with N = n and N = m, and three steps with registers at every
    scale under an emit mask."""
    import test_gpu_circuit_script as TS
    with session(S, drivers, "scripted"):
        try:
            for G in (1, 6):
                TS.test_every_reference_form_through_one_gather(S, G)
            for mode in ("lwe", "direct"):
                TS.test_sum_nodes_at_the_ends_of_the_sum_and_low_with_a_borrow(S, mode)
            TS.test_lut_not_at_every_codeword_and_every_table_of_a_plane(S)
            TS.test_scatter_leaves_unread_and_pruned_rows_out_and_moves_nothing_else(S)
            TS.test_a_level_wider_than_a_call_with_routes_across_the_boundary(S)
            for ring in ("tiny", "wide"):
                TS.test_unreduced_calls_at_the_ends_of_zq_and_the_ties_of_modred(S, ring)
            TS.test_a_raw_call_split_inside_a_producing_node(S)
            TS.test_lift_of_every_kind_of_output_equals_the_integer_lift(S)
            for big in (False, True):
                TS.test_split_reads_the_negative_side_where_it_should(S, big)
            TS.test_three_steps_with_registers_at_every_scale(S)
        finally:
            TS.teardown_module(TS)      # its ctxs belong to this session


@pytest.mark.parametrize("name", RC.NAMES)
def test_data_planes(S, oc, drivers, name):
    """tests/test_gpu_circuit_data.py's test_other_ring_kinds: a run with data planes on every ring, both modes."""
    import test_gpu_circuit_data as TD
    with session(S, drivers, "data-" + name):
        for rnd in RC.MODES:
            TD.test_other_ring_kinds(S, oc, name, rnd)


# ---- e. the rest of the ABI that launches anything ----------------------------------------------------------------------------

def test_transforms_conversions_and_the_product(S, oc, drivers):
    """sgfhe_debug_ntt forward and back on every prime of m = 64 and 128 (the round trip is the identity),
    sgfhe_rns2_convert both ways at 1 and 257 elements, sgfhe_release_host_staging between two calls, and a clone that
    runs after its parent is destroyed."""
    import bigint_oracle as BO
    import test_gpu_rings as TR
    with session(S, drivers, "abi-rest"):
        rng = np.random.default_rng(77)
        for name in ("limb64", "m128"):
            eng = S.Engine(RC.ring(S, name).params)
            m = eng.params.m
            for i, q in enumerate(eng.primes()):
                x = rng.integers(0, q, size=m).astype(np.uint32)
                assert np.array_equal(eng.debug_ntt(i, eng.debug_ntt(i, x), inverse=True), x), (name, i)
            eng.close()
        case = TR.Case(S, oc, "composite")
        B, Bp = case.rg.rns2
        for count in (1, 257):
            vals = [int(v) for v in rng.integers(0, 1 << 62, size=count)]
            vals = [(v * v) % case.params.Q for v in vals]
            canon = np.array([[v & (2**64 - 1), v >> 64] for v in vals], dtype=np.uint64)
            pairs = case.eng.rns2_convert(canon, B, Bp, True)
            assert [tuple(int(x) for x in pr) for pr in pairs] == [tuple(BO.rns2_from_int(v, B, Bp)) for v in vals]
            assert np.array_equal(case.eng.rns2_convert(pairs, B, Bp, False), canon)
        case.close()
        case = TR.Case(S, oc, "m128")
        p = case.params
        assert case.mode(False)
        rows = _rows(p, rng, 3)
        want = case.o.bootstrap_batch(case.khat, *rows, opt=True)
        assert np.array_equal(case.eng.bootstrap_batch(*rows), want)
        case.eng.release_host_staging()
        assert np.array_equal(case.eng.bootstrap_batch(*rows), want)
        clone = case.eng.clone()
        case.close()
        assert np.array_equal(clone.bootstrap_batch(*rows), want)
        clone.close()


def test_ntt_every_size_and_the_external_product(S, oc, drivers):
    """tests/test_gpu_parity.py: sgfhe_debug_ntt at every logm 6..14 forward (against the numpy model) and back, and
    sgfhe_external_product against the oracle with the gadget matrix and with a random one (k_flatten_canon)."""
    import test_gpu_parity as TP
    with session(S, drivers, "ntt-extprod"):
        for logm in range(6, 15):
            TP.test_ntt_matches_model(S, logm)
        for gadget in (True, False):
            TP.test_external_product(S, oc, gadget)


def test_key_export_import_and_a_device_call(S, oc, drivers):
    """The device-form key exported into a hipMalloc block of exactly sgfhe_bkey_device_form_bytes and imported into a
    second ctx, which then bootstraps to the oracle's rows; sgfhe_bootstrap_batch_device on pointers the stand-in
    allocated; sgfhe_pack_encrypted_bits against the oracle at one ciphertext."""
    import test_gpu_rings as TR
    with session(S, drivers, "export-import") as ses:
        case = TR.Case(S, oc, "m128")
        p = case.params
        assert case.mode(False)
        rng = np.random.default_rng(78)
        rows = _rows(p, rng, 3)
        want = case.o.bootstrap_batch(case.khat, *rows, opt=True)
        blob = np.zeros(case.eng.key_device_form_bytes(), dtype=np.uint8)
        case.eng.export_key_device_form(ses.register(blob, device=True))
        assert blob.any()
        other = S.Engine(p)
        other.import_key_device_form(blob.ctypes.data)
        assert np.array_equal(other.bootstrap_batch(*rows), want)
        out = np.zeros((3, 3, p.n + 1), dtype=np.uint64)
        dev = [ses.register(np.ascontiguousarray(x), device=True) for x in rows] + [ses.register(out, device=True)]
        other.bootstrap_batch_device(dev[0], dev[1], dev[2], dev[3], 3, dev[4])
        other.sync()
        assert np.array_equal(out, want)
        a, b = _rows(p, rng, p.n)[:2]
        w, v = case.eng.pack_encrypted_bits(a.reshape(1, p.n, p.n), b.reshape(1, p.n))
        ow, ov = case.o.pack_encrypted_bits(case.bkey, a, b)
        assert np.array_equal(w[0], ow) and np.array_equal(v[0], ov)
        other.close()
        case.close()


def test_cmux_hook(S, drivers):
    """tests/test_gpu_kloop_step.py's test_equals_the_cmux_hook on `m128`: sgfhe_debug_cmux (k_flatten_canon -> k_extprod
    -> the CRT kernel) against one k-loop step on the same operands, itself held to the reference in Python integers."""
    import test_gpu_kloop_step as TK
    with _observed_here(TK), session(S, drivers, "cmux"):
        get = _getter(lambda n, params=None: TK.Ctx(S, params() if params else RC.ring(S, n).params))
        TK.test_equals_the_cmux_hook(S, get, "m128")
        for c in get.made.values():
            c.eng.close()


def test_pack_and_lift_at_counts_of_1_and_n_plus_1(S, oc, drivers):
    """`tiny` (n = 8), counts 1 and n + 1: sgfhe_lwe_lift_modq against floor((x Q + r/2) / r) in Python integers,
    sgfhe_pack_lwe_modq on un-reduced oracle rows against the big-integer tail (pack_direct_ref.FastTail), and
    sgfhe_pack_encrypted_bits against the C oracle."""
    import pack_direct_ref as R
    import test_gpu_rings as TR
    with session(S, drivers, "pack-lift-counts"):
        case = TR.Case(S, oc, "tiny")
        p, n = case.params, case.params.n
        assert case.mode(False)
        rng = np.random.default_rng(79)
        fast = R.FastTail(case.bp, case.bk)
        for count in (1, n + 1):
            x = rng.integers(0, p.r, size=(count, n + 1)).astype(np.uint64)
            x[0, :2] = (0, p.r - 1)
            got = case.eng.lwe_lift(x)
            want = [(int(v) * p.Q + p.r // 2) // p.r for v in x.reshape(-1)]
            assert [int(lo) | (int(hi) << 64) for lo, hi in got.reshape(-1, 2)] == want, count
            rows = _rows(p, rng, count * n)
            raw = case.o.bootstrap_batch(case.khat, *rows, raw=True, opt=True)
            lwe = np.ascontiguousarray(raw[:, 0].reshape(count, n, n + 1, 2))
            w, v = case.eng.pack_lwe_modq(lwe)
            for ct in range(count):
                ow, ov = fast(lwe[ct], seed=None, ct=ct, call=0)
                assert np.array_equal(w[ct], ow) and np.array_equal(v[ct], ov), (count, ct)
            a, b = rows[0].reshape(count, n, n), rows[1].reshape(count, n)
            w, v = case.eng.pack_encrypted_bits(a, b)
            for ct in range(count):
                ow, ov = case.o.pack_encrypted_bits(case.bkey, a[ct], b[ct])
                assert np.array_equal(w[ct], ow) and np.array_equal(v[ct], ov), (count, ct)
        case.close()


def test_device_resident_circuit_entries(S, oc, drivers):
    """One call of each of sgfhe_circuit_run_device, _run_ct_device, _run_steps_device and _run_steps_ct_device on
    `tiny`, every pointer a block the stand-in allocated: the bytes of the host entry of the same form on the same
    inputs (whose results the ring sessions hold to the oracle).  Their ordering guarantees are about real streams and
    are out of this harness's reach."""
    import pack_lift_ref as PL
    import run_error_cases as RE
    import test_gpu_rings as TR
    with session(S, drivers, "device-entries") as ses:
        case = TR.Case(S, oc, "tiny")
        p, n, eng = case.params, case.params.n, case.eng
        assert case.mode(False)
        plans = RE.make_plans(S)
        plain, regs = plans["plain"], plans["regs"]
        rng = np.random.default_rng(80)
        dev = lambda arr: ses.register(arr, device=True)
        inst, blocks, steps = 5, 1, 2
        import noise_ref as NR
        bits = rng.integers(0, 2, size=2 * inst).astype(bool)
        x = np.ascontiguousarray(NR.handmade_zr(p, case.sk, rng, np.zeros(bits.size, dtype=np.int64), bits)
                                 .reshape(2, inst, n + 1), dtype=np.uint64)
        # LWE form, one-shot
        want = eng.circuit_run(plain, x)
        out = np.zeros_like(want)
        assert ses.sgfhe_circuit_run_device(eng._h, plain.handle(), inst, dev(x), None, dev(out), None) == 0
        eng.sync()
        assert np.array_equal(out, want)
        # LWE form, stepped: [steps][stream inputs][instances][n + 1]
        xs = np.ascontiguousarray(x.reshape(steps, 1, inst, n + 1))
        want, want_st = eng.circuit_run_steps(regs, None, xs)
        out, st = np.zeros_like(want), np.zeros_like(want_st)
        assert ses.sgfhe_circuit_run_steps_device(eng._h, regs.handle(), inst, steps, None, dev(xs), None, None, dev(out),
                                                  dev(st), None) == 0
        eng.sync()
        assert np.array_equal(out, want) and np.array_equal(st, want_st)
        # ciphertext form, one-shot: [n_inputs][blocks][N = n]
        cbits = rng.integers(0, 2, size=(2, blocks, n)).astype(bool)
        a, b = (np.ascontiguousarray(t, dtype=np.uint64) for t in PL.craft_cts(S, p, case.sk, cbits, 2424))
        (ww, wv), wl = eng.circuit_run_ct(plain, a, b, packed=True, lwe=True)
        w, v, lwe = np.zeros_like(ww), np.zeros_like(wv), np.zeros_like(wl)
        assert ses.sgfhe_circuit_run_ct_device(eng._h, plain.handle(), blocks, dev(a), dev(b), a.shape[2], None, dev(w),
                                               dev(v), dev(lwe), 0, None) == 0
        eng.sync()
        assert np.array_equal(w, ww) and np.array_equal(v, wv) and np.array_equal(lwe, wl)
        # ciphertext form, stepped: [steps][stream inputs][blocks][N]
        ta, tb = (np.ascontiguousarray(t).reshape(steps, 1, blocks, a.shape[2]) for t in (a, b))
        ((ww, wv), wl), want_st = eng.circuit_run_steps_ct(regs, None, None, ta, tb, packed=True, lwe=True)
        w, v, lwe, st = np.zeros_like(ww), np.zeros_like(wv), np.zeros_like(wl), np.zeros_like(want_st)
        assert ses.sgfhe_circuit_run_steps_ct_device(eng._h, regs.handle(), blocks, steps, None, None, dev(ta), dev(tb),
                                                     a.shape[2], None, None, dev(w), dev(v), dev(lwe), dev(st), 0, None) == 0
        eng.sync()
        assert np.array_equal(w, ww) and np.array_equal(v, wv) and np.array_equal(lwe, wl) and np.array_equal(st, want_st)
        del plans, plain, regs
        case.close()


def _device_call(RE):
    """run_error_cases.Call with numpy arrays where it makes tensors on a GPU: the same shapes, dtypes and fill."""
    class DeviceCall(RE.Call):
        def __init__(self, entry, case, params):
            E = RE.ENTRIES[entry]
            RE.ENTRIES[entry] = E._replace(device=False)       # (Call.__init__ reads the flag only to pick torch)
            try:
                super().__init__(entry, case, params)
            finally:
                RE.ENTRIES[entry] = E
            self.E = E
    return DeviceCall


def test_refusals_match_the_record(S, oc, drivers):
    """Every case of tests/run_error_cases.py against tests/golden/circuit_run_errors.json: code and message, nothing
    written.  The cases of the device-resident entries hand in blocks the stand-in allocated where the GPU test hands
    in tensors (`_DeviceCall`)."""
    import json
    import run_error_cases as RE
    with open(os.path.join(ROOT, "tests", "golden", "circuit_run_errors.json")) as fh:
        golden = json.load(fh)["cases"]
    with session(S, drivers, "refusals") as ses:
        params = S.Params(RE.N)
        sk = oc.Oracle.from_params(params).private_key(2411)
        keyed, bare = S.Engine(params), S.Engine(params)
        keyed.generate_key(sk, 2412)
        plans = RE.make_plans(S)
        ran = 0
        for entry, case in RE.CASES:
            device = RE.ENTRIES[entry].device
            call = (_device_call(RE) if device else RE.Call)(entry, case, params)
            for a, arr in call.arrays.items():
                ses.register(arr, device=device and a != "emit")
            eng = keyed if case.key else bare
            code, msg = call.run(ses, eng._h, plans[case.plan].handle())
            assert [code, msg if code else ""] == golden[RE.case_id(entry, case)], (entry, case.name)
            zeroed = ("stats",) if code == 0 and RE.ENTRIES[entry].probe else ()
            assert call.untouched(zeroed), (entry, case.name)
            ses.known.clear()
            ran += 1
        assert ran == len(RE.CASES)
        del plans
        keyed.close()
        bare.close()


# ---- what ran ----------------------------------------------------------------------------------------------------------

# kernels of kernels.h that no session above launches, each with its reason
OMITTED = {}


def _expected_sessions():
    per_ring = ("bootstraps-", "kloop-", "entry-exit-", "data-")
    return ({pre + n for pre in per_ring for n in RC.NAMES} | {"rings-" + n for n in RC.NAMES} |
            {"kloop-%s-%d-%s" % (n, r, "+".join(map(str, cs))) for n, r, cs in QUARTER_CASES} |
            {"scripted", "abi-rest", "ntt-extprod", "export-import", "refusals", "cmux", "pack-lift-counts", "device-entries"})


def test_every_kernel_was_launched():
    """The stand-in counts launches by kernel name: all __global__ functions of kernels.h but the OMITTED ones.  The
    verdict needs every session of this file to have ended well; under a selection of tests it is skipped."""
    if set(SESSIONS) != _expected_sessions():
        pytest.skip("not every session of this file ran before this test: %s"
                    % sorted(_expected_sessions() - set(SESSIONS)))
    with open(os.path.join(ROOT, "sgfhe.jl_amd", "csrc", "kernels.h")) as fh:
        text = fh.read()
    kernels = set(re.findall(r"__global__ void __launch_bounds__\([^\n]*\)\s*\n?\s*(k_\w+)\(", text))
    assert len(kernels) == text.count("__global__"), "the pattern no longer finds every kernel"
    assert set(OMITTED) <= kernels
    missing = kernels - set(LAUNCHED) - set(OMITTED)
    assert not missing, "never launched: %s" % sorted(missing)
