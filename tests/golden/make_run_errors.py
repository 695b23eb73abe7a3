"""Recorder of tests/golden/circuit_run_errors.json: what every run entry of the C ABI answers to the cases of
tests/run_error_cases.py -- (entry, case) -> [code, sgfhe_last_error_string] -- on a GPU, through ctypes and nothing but
the ABI.  The fixture is the behaviour of the commit it was recorded at (named in the file, with the library's build id)
and is what later commits are held to: it is not made again from the code under test.

    python tests/golden/make_run_errors.py [--out FILE]

Each case runs once, under a time limit, and the recorder stops at the first case that is neither refused nor empty as
the case list says it must be: every case ends before any device work, so none may queue a run."""

import argparse
import faulthandler
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

import run_error_cases as RC  # noqa: E402

CASE_LIMIT_S = 60


def check_plans(plans):
    """The plans are what the case list says of them (the counts of the addressing cases rest on `widest` and `group`)."""
    for name, c in plans.items():
        n_inputs, n_regs, n_planes, group, widest, n_outputs, n_gates = RC.PLAN_FACTS[name]
        assert (c.n_inputs, c.n_regs, c.planes, c.group, c.n_outputs, c.n_gates) == \
            (n_inputs, n_regs, n_planes, group, n_outputs, n_gates), name
        assert c.info()["widest"] == widest, name


def engines(S):
    """(params, a ctx with a key, a ctx without one) at Params(64)."""
    params = S.Params(RC.N)
    keyed, bare = S.Engine(params), S.Engine(params)
    keyed.generate_key(np.random.default_rng(2401).integers(0, 2, size=params.n).astype(np.uint64), 2402)
    return params, keyed, bare


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "circuit_run_errors.json"))
    ap.add_argument("--commit", default=None, help="the commit recorded at (default: git rev-parse HEAD)")
    args = ap.parse_args()
    import sgfhe_jl_amd as S
    L = S.lib()
    params, keyed, bare = engines(S)
    plans = RC.make_plans(S)
    check_plans(plans)
    commit = args.commit or subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True,
                                           text=True).stdout.strip()
    record = {"commit": commit or None, "build_id": L.sgfhe_build_id().decode(), "abi": int(L.sgfhe_abi_version()),
              "cases": {}}
    status = 0
    for entry, case in RC.CASES:
        call = RC.Call(entry, case, params)
        eng = keyed if case.key else bare
        faulthandler.dump_traceback_later(CASE_LIMIT_S, exit=True)
        code, msg = call.run(L, eng._h, plans[case.plan].handle())
        faulthandler.cancel_dump_traceback_later()
        print("%-40s %-28s %3d %s" % (entry, case.name, code, msg if code else ""), flush=True)
        if (code < 0) != (case.expect == "refused") or code > 0:
            print("STOP: the case list expects this case to be %s" % case.expect, flush=True)
            status = 1
            break
        record["cases"][RC.case_id(entry, case)] = [code, msg if code else ""]
    with open(args.out, "w") as fh:
        json.dump(record, fh, indent=1, sort_keys=True)
        fh.write("\n")
    keyed.close()
    bare.close()
    print("%d of %d cases recorded -> %s" % (len(record["cases"]), len(RC.CASES), args.out))
    return status


if __name__ == "__main__":
    sys.exit(main())
