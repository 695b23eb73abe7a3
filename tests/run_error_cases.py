"""TEST INFRASTRUCTURE: the arguments a circuit run refuses (or takes as an empty run), once, for every run entry of the
C ABI (tests/golden/make_run_errors.py records them, tests/test_gpu_circuit_errors.py and
tests/test_circuit_request_host.py hold the library and csrc/circuit.h's circuit_request_check to the record).

A case is a run of one entry on a small plan at Params(64) that differs from a correct run -- 8 instances or 1 block,
1 step, flags 0, N = n, every pointer the plan needs given, a ctx with a key -- in one named defect, or in two where the
pair pins which check comes first.  The checks, in the order every entry makes them:
flag bits; NULL circuit, input or output pointers and the state pair; a plan with registers in a one-shot entry; a
register of scale 1 or 2 in a stepped ciphertext entry; a plan with planes in an entry without `data`; NULL data; the
probe's pointers; the out_w / out_v pairing and one output form; N; no key; the pack bound (which no valid parameter set
misses: tests/test_circuit_request_host.py alone has that case); an empty run, which returns OK; the addressing limits;
the lane group.  Every case ends before any device work: no case's arrays need to be as large as its count says.

Arguments are named as csrc/circuit.h's CircuitRequest names them: `count` is instances or blocks, `out` the LWE
outputs (out_lwe of the ciphertext entries), `state_out` the registers after the last step (state_lwe there).
"""

import collections

N = 64                      # Params(64)
BASE = {False: 8, True: 1}   # count of the correct run, by `ct`: instances, blocks
CAP = 64                    # instances every array of a case is allocated for (>= any count below 2^31 a case passes)

Entry = collections.namedtuple("Entry", "ct stepped probe device data flags args")
_LWE, _CT = ("circ", "count", "in"), ("circ", "count", "in_a", "in_b", "N")
_STEPS = ("circ", "count", "steps", "state_in", "in", "data", "emit", "out", "state_out")
_STEPS_CT = ("circ", "count", "steps", "state_a", "state_b", "in_a", "in_b", "N", "data", "emit", "out_w", "out_v", "out",
             "state_out", "flags")
_PROBE, _WV = ("sk", "in_bits", "stats"), ("out_w", "out_v", "out")


def _entry(args, ct=False, stepped=False, probe=False, device=False):
    return Entry(ct, stepped, probe, device, "data" in args, "flags" in args, args + (("stream",) if device else ()))


# the arguments of every entry behind the ctx, in the order of include/sgfhe_hip.h
ENTRIES = {
    "sgfhe_circuit_run": _entry(_LWE + ("out",)),
    "sgfhe_circuit_run_data": _entry(_LWE + ("data", "out")),
    "sgfhe_circuit_run_probe": _entry(_LWE + ("out",) + _PROBE, probe=True),
    "sgfhe_circuit_run_probe_data": _entry(_LWE + ("data", "out") + _PROBE, probe=True),
    "sgfhe_circuit_run_ct": _entry(_CT + _WV, ct=True),
    "sgfhe_circuit_run_ct_ex": _entry(_CT + _WV + ("flags",), ct=True),
    "sgfhe_circuit_run_ct_data": _entry(_CT + ("data",) + _WV + ("flags",), ct=True),
    "sgfhe_circuit_run_steps": _entry(_STEPS, stepped=True),
    "sgfhe_circuit_run_steps_ct": _entry(_STEPS_CT, ct=True, stepped=True),
    "sgfhe_circuit_run_device": _entry(_LWE + ("data", "out"), device=True),
    "sgfhe_circuit_run_ct_device": _entry(_CT + ("data",) + _WV + ("flags",), ct=True, device=True),
    "sgfhe_circuit_run_steps_device": _entry(_STEPS, stepped=True, device=True),
    "sgfhe_circuit_run_steps_ct_device": _entry(_STEPS_CT, ct=True, stepped=True, device=True),
}
SCALARS = ("count", "steps", "N", "flags")
OUTPUTS = ("out", "out_w", "out_v", "state_out", "stats")
OPTIONAL = ("state_in", "state_a", "state_b", "emit")   # NULL in the correct run

# `expect`: "refused" (a code below 0) or "empty" (SGFHE_OK, nothing done).  `null` / `given`: the pointers a case takes
# away from, or adds to, the correct run's.  `N`: "n" or "n+1".
Case = collections.namedtuple("Case", "name plan key count steps N flags null given expect")


def make_plans(S):
    """The plans of the cases, by name, as circuit.Circuit: one to three nodes each."""
    C = S.Circuit

    def one_gate(**kw):
        c = C(2, **kw)
        c.output(c.gate(*c.inputs)[0])
        return c
    plans = {"plain": one_gate(), "group8": one_gate(group=8), "group48": one_gate(group=48)}
    c = C(2, registers=1)                     # one register of scale 0, one stream input
    g = c.gate(c.registers[0], c.stream_inputs[0])
    c.output(g[0])
    c.next_state(g[2])
    plans["regs"] = c
    c = C(2, registers=1, reg_scales=[1])     # a register of scale 1, read and fed by a LUT node
    f = c.lut(0x96, C.FALSE, c.registers[0], c.stream_inputs[0])
    c.output(f[0])
    c.next_state(f[1])
    plans["regs1"] = c
    c = C(2, planes=1)                        # a classic node, then a LUT node whose table is plane 0
    g = c.gate(*c.inputs)
    c.output(c.lut_data(0, C.FALSE, C.FALSE, g[0])[0])
    plans["planes"] = c
    c = C(2)                                  # three nodes in one level: widest = 3
    x, y = c.inputs
    c.output(c.gate(x, y)[0], c.gate(x, ~y)[0], c.gate(~x, y)[0])
    plans["wide"] = c
    return plans


# what the host program reads of a plan (tests/native/circuit_request_sanitized.cpp builds the same)
PLAN_FACTS = {   # n_inputs, n_regs, n_planes, group, widest, n_outputs, n_gates
    "plain": (2, 0, 0, 1, 1, 1, 1), "group8": (2, 0, 0, 8, 1, 1, 1), "group48": (2, 0, 0, 48, 1, 1, 1),
    "regs": (2, 1, 0, 1, 1, 1, 1), "regs1": (2, 1, 0, 1, 1, 1, 1), "planes": (2, 0, 1, 1, 1, 1, 2),
    "wide": (2, 0, 0, 1, 3, 3, 3),
}


def cases_of(entry):
    """The cases of one entry, in the order of the checks."""
    E = ENTRIES[entry]
    per = N if E.ct else 1   # instances per count
    out = []

    def add(name, expect="refused", plan="plain", key=True, count=None, steps=1, N="n", flags=0, null=(), given=()):
        null = tuple(a for a in null if a in E.args)
        out.append(Case(name, plan, key, BASE[E.ct] if count is None else count, steps, N, flags, null, given, expect))

    no_output = ("out", "out_w", "out_v", "state_out") if E.ct or E.stepped else ("out",)
    if E.flags:
        add("flag_bit_4", flags=4)
        add("lift_alone", flags=2)
    add("null_circuit", null=("circ",))
    for a in (("in_a", "in_b") if E.ct else ("in",)):
        add("null_" + a, null=(a,))
    add("no_output", null=no_output)
    if E.ct and E.stepped:
        add("state_a_without_b", given=("state_a",))
    if not E.stepped:
        add("registers_plan", plan="regs")
    if E.ct and E.stepped:
        add("scale_1_register", plan="regs1")
    if not E.stepped and not E.data:
        add("planes_plan", plan="planes")
    if E.data:
        add("null_data", plan="planes", null=("data",))
    if E.probe:
        for a in ("sk", "in_bits", "stats"):
            add("null_" + a, null=(a,))
    if E.ct:
        add("out_w_without_v", null=("out_v",))
        add("bad_N", N="n+1")
    add("no_key", key=False)
    add("count_0", count=0, expect="empty")
    if E.stepped:
        add("steps_0", steps=0, expect="empty")
    add("instances_2^31", count=2**31 // per)
    add("widest_overflow", plan="wide", count=0x60000000 // per)      # 3 * 0x60000000 > 2^32 - 1
    if E.ct:
        add("group_48", plan="group48")
    else:
        add("group_8_of_20", plan="group8", count=20)
    # two defects: the earlier check's message
    if E.flags:
        add("flags_and_null_circuit", flags=4, null=("circ",))
    if E.data:
        add("null_data_and_no_key", plan="planes", null=("data",), key=False)
    if E.ct:
        add("bad_N_and_no_key", N="n+1", key=False)
    add("no_key_and_count_0", key=False, count=0)
    if E.ct:
        add("too_many_and_group", plan="group48", count=2**31 // per)
        add("out_w_without_v_and_bad_N", null=("out_v",), N="n+1")
    else:
        add("too_many_and_group", plan="group8", count=2**31 + 4)
    return out


CASES = [(entry, case) for entry in ENTRIES for case in cases_of(entry)]


def case_id(entry, case):
    return "%s %s" % (entry, case.name)


def shapes(entry, case):
    """name -> (shape, is uint8) of every pointer argument of the entry, for the plan of `case`: each large enough for a
    run over CAP instances (one block) and one step, whatever the case's count says ("m": the ring degree)."""
    E = ENTRIES[entry]
    n_inputs, n_regs, n_planes, _group, _widest, n_outputs, n_gates = PLAN_FACTS[case.plan]
    lwe =lambda k: ((max(k, 1), CAP, N + 1), False)
    ct = lambda k: ((max(k, 1), 1, "m"), False)
    every = {
        "in": lwe(n_inputs), "in_a": ct(n_inputs), "in_b": ct(n_inputs), "out": lwe(n_outputs),
        "out_w": ct(n_outputs), "out_v": ct(n_outputs), "state_in": lwe(n_regs), "state_a": ct(n_regs),
        "state_b": ct(n_regs), "state_out": lwe(n_regs), "data": ((max(n_planes, 1), CAP), True), "emit": ((1,), True),
        "sk": ((N,), False), "in_bits": ((n_inputs, CAP), True), "stats": ((n_inputs + 3 * n_gates, 8), False),
    }
    return {a: every[a] for a in E.args if a in every}


SENTINEL = 0xA5A5A5A5A5A5A5A5


class Call:
    """One case made into the arguments of its entry.  `arrays`: name -> the array behind each pointer handed in (numpy,
    or a torch tensor on the device for a device entry; `emit` is host memory in both).  run(L, ctx, handle) makes the
    call once and returns (code, message); untouched() says whether every output array still holds the sentinel
    (`zeroed`: names expected to hold zeros instead)."""

    def __init__(self, entry, case, params):
        import numpy as np
        self.entry, self.case, self.E = entry, case, ENTRIES[entry]
        self.params = params
        self.arrays = {}
        for a, (shape, small) in shapes(entry, case).items():
            if a in case.null or (a in OPTIONAL and a not in case.given):
                continue
            if a == "data" and not PLAN_FACTS[case.plan][2]:
                continue                                  # a plan without planes takes no data
            shape = tuple(params.m if d == "m" else d for d in shape)
            arr = np.full(shape, SENTINEL if a in OUTPUTS else 1, dtype=np.uint8 if small else np.uint64)
            if self.E.device and a != "emit":
                import torch
                arr = torch.from_numpy(arr.view(np.int64) if not small else arr).cuda()
            self.arrays[a] = arr
        if self.E.device:
            import torch
            torch.cuda.synchronize()

    def _pointer(self, a):
        import ctypes
        arr = self.arrays.get(a)
        if arr is None:
            return None
        return ctypes.c_void_p(arr.data_ptr() if hasattr(arr, "data_ptr") else arr.ctypes.data)

    def args(self, handle):
        c, p = self.case, self.params
        scalar = {"count": c.count, "steps": c.steps, "N": p.n + (c.N == "n+1"), "flags": c.flags}
        out = []
        for a in self.E.args:
            if a == "circ":
                out.append(None if "circ" in c.null else handle)
            elif a == "stream":
                out.append(None)
            elif a in scalar:
                out.append(scalar[a])
            else:
                out.append(self._pointer(a))
        return out

    def run(self, L, ctx, handle):
        code = getattr(L, self.entry)(ctx, *self.args(handle))
        return int(code), L.sgfhe_last_error_string(ctx).decode()

    def host(self, a):
        import numpy as np
        arr = self.arrays[a]
        if hasattr(arr, "data_ptr"):
            import torch
            torch.cuda.synchronize()
            arr = arr.cpu().numpy()
            if arr.dtype == np.int64:
                arr = arr.view(np.uint64)
        return arr

    def untouched(self, zeroed=()):
        for a in self.arrays:
            if a in OUTPUTS:
                want = 0 if a in zeroed else SENTINEL
                if not (self.host(a) == want).all():
                    return False
        return True
