"""Static VALU instruction counts of the k-loop CRT kernels, from the gfx950 assembly hipcc produces
for the current sources: k_crt_lean<5, 3, true> (crt_lean87_one, Params(1024)) against the generic
k_crt_lean<5, 3>, per thread (four coefficients) and per coefficient, with the instruction mix; and,
for the whole library, the kernel count and every kernel that uses scratch.
usage: python tools/crt_valu.py  -> JSON on stdout (the compile takes about a minute)"""
import collections
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sgfhe.jl_amd", "csrc")
KERNELS = {"k_crt_lean<5, 3, true>": "_ZN5sgfhe10k_crt_leanILi5ELi3ELb1EEEvPKjPmPKNS_7CrtLeanEjj",
           "k_crt_lean<5, 3>": "_ZN5sgfhe10k_crt_leanILi5ELi3ELb0EEEvPKjPmPKNS_7CrtLeanEjj"}


def main():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "engine.s")
        subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S",
                               "-o", out, os.path.join(CSRC, "engine.hip")], stderr=subprocess.DEVNULL)
        asm = open(out).read()
    res = {}
    for name, sym in KERNELS.items():
        m = re.search(r"^%s:.*?\n(.*?)\n\.Lfunc_end" % re.escape(sym), asm, re.S | re.M)
        if not m:
            raise SystemExit("kernel %s not found in the assembly" % name)
        ops = [l.split()[0] for l in m.group(1).splitlines() if l.strip().startswith("v_")]
        mix = collections.Counter(o.replace("_e32", "").replace("_e64", "") for o in ops)
        res[name] = {"valu_per_thread": len(ops), "valu_per_coefficient": len(ops) / 4,
                     "mix": dict(mix.most_common())}
    kern = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M)
    scratch = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)(?:(?!\.end_amdhsa_kernel).)*?"
                         r"\.amdhsa_private_segment_fixed_size\s+([1-9]\d*)", asm, re.M | re.S)
    res["kernels"] = len(kern)
    res["kernels_with_scratch"] = [k for k, _ in scratch]
    json.dump(res, sys.stdout, indent=1)
    print()


if __name__ == "__main__":
    main()
