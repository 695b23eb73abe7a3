"""Every constant the kernels read (csrc/constants.h: check_params, plan_bases, derive_basis, prime_tables, key_factors,
rns2_const) without a device: a stand-alone program prints them under ASan / UBSan (tests/native/constants_sanitized.cpp)
and every field is compared, exactly, with Python big integers -- rns_model.Consts / CrtLean, test_crt_lean87_model, and
the exact bounds the header's double-precision sizing rules stand for."""

import math
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import rns_model as RM
import test_crt_lean87_model as L87

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM_INCLUDE = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")
M32 = (1 << 32) - 1
NPR_MAX, ALPHA_MAX = RM.NPR_MAX, 6 * RM.NPR_MAX + 2

# (row, key) pairs of the record that are printed in decimal; everything else is hex
DEC = {"case": {"det_only"}, "plan": {"logm", "npr", "rnd_width_ok", "nb", "rnd_ok", "npr_max"},
       "basis": {"basis", "mode", "npr", "lean_rnd_ok", "pack_G", "pack_G_rnd"}, "crt": {"npr", "logr"},
       "lean": {"nl", "a", "t2", "sB", "p87"},
       "pk": {"pk", "p", "sR", "sRr", "hoff", "r1", "r2", "r3", "qmodp", "kappaR", "minvR", "npr", "nulls"}}
REFUSALS = {   # request -> (code, message) of sgfhe_ctx_create_ex today, in the order it checks
    "check 3 64 128 8 10001 200 5": (-2, "ell must be 2 (fhe.jl:576)"),
    "check 2 32 64 8 10001 200 5": (-2, "m must be a power of two in [2^6, 2^14]"),
    "check 2 32768 65536 8 10001 200 5": (-2, "m must be a power of two in [2^6, 2^14]"),
    "check 2 96 192 8 10001 200 5": (-2, "m must be a power of two in [2^6, 2^14]"),
    "check 2 64 64 8 10001 200 5": (-1, "r must equal 2 m (fhe.jl:62)"),
    "check 2 64 128 0 10001 200 5": (-1, "n must be a power of two in [1, m / 4] (fhe.jl:45-46; extract, fhe.jl:585-590)"),
    "check 2 64 128 32 10001 200 5": (-1, "n must be a power of two in [1, m / 4] (fhe.jl:45-46; extract, fhe.jl:585-590)"),
    "check 2 64 128 12 10001 200 5": (-1, "n must be a power of two in [1, m / 4] (fhe.jl:45-46; extract, fhe.jl:585-590)"),
    "check 2 64 128 8 2 200 1": (-2, "Q must be in [3, 2^94)"),
    "check 2 64 128 8 %x %x 5" % (1 << 94, 1 << 46): (-2, "Q must be in [3, 2^94)"),
    "check 2 64 128 8 3 1 1": (-2, "B must be in [2, 2^47)"),
    "check 2 64 128 8 10001 %x 5" % (1 << 47): (-2, "B must be in [2, 2^47)"),
    "check 2 64 128 8 10001 ff 5": (-1, "B^2 must be >= Q"),
    "check 2 64 128 8 10001 200 10001": (-1, "DQ_tilde must be < Q"),
    # (ell is checked first, DQ_tilde last)
    "check 3 32 64 0 2 1 5": (-2, "ell must be 2 (fhe.jl:576)"),
    "check 2 64 128 16 3 2 2": None,          # the smallest set it accepts
    "check 2 16384 32768 4096 %x %x 0" % (((1 << 47) - 1) ** 2, (1 << 47) - 1): None,     # the largest
}


# ---- the program -------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    """(sanitized, plain) builds of tests/native/constants_sanitized.cpp."""
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    if not os.path.exists(os.path.join(ROCM_INCLUDE, "hip", "hip_vector_types.h")):
        pytest.skip("no <hip/hip_vector_types.h> under " + ROCM_INCLUDE)
    tmp = tmp_path_factory.mktemp("constants")
    src = os.path.join(ROOT, "tests", "native", "constants_sanitized.cpp")
    inc = ["-D__HIP_PLATFORM_AMD__", "-I", ROCM_INCLUDE, "-I", os.path.join(ROOT, "sgfhe.jl_amd", "csrc")]
    exe = str(tmp / "constants_sanitized")
    # (the sanitizer runtimes are linked into the program, so that it starts in any environment: a dynamic ASan runtime
    #  refuses to start behind a library the environment preloads)
    b = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-static-libasan", "-static-libubsan", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror"]
                       + inc + [src, "-o", exe], capture_output=True, text=True, timeout=300)
    if b.returncode != 0 and "sanitize" in b.stderr and "cannot find" in b.stderr:
        pytest.skip("the sanitizer runtimes are not installed: " + b.stderr[-300:])
    assert b.returncode == 0, b.stderr[-3000:]
    exe2 = str(tmp / "constants_plain")
    subprocess.run([gxx, "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror"] + inc + [src, "-o", exe2], check=True, timeout=300)
    return exe, exe2, tmp


def run(programs, requests):
    """The sanitized program's output lines for the requests; the plain build must print the same."""
    exe, exe2, _ = programs
    text = "".join(r + "\n" for r in requests)
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=300)   # (the environment as it is)
    assert r.returncode == 0, (r.stdout[-1500:] + r.stderr)[-3000:]
    r2 = subprocess.run([exe2], input=text, capture_output=True, text=True, timeout=300)
    assert r2.returncode == 0 and r2.stdout == r.stdout, "the plain build prints something else"
    lines = r.stdout.splitlines()
    assert re.fullmatch(r"ok %d" % len(requests), lines[-1]), lines[-1]
    return lines[:-1]


def parse(lines):
    """[case record]: {"case", "refusal" | "plan", "primes", "basis": {b: {...rows, "pk": [...]}}, "keyfactors", "tables"}."""
    out = []
    for line in lines:
        tok = line.split()
        row, rest = tok[0], tok[1:]
        if row == "refusal":
            out[-1]["refusal"] = (int(rest[0]), " ".join(rest[1:]))
        elif row in DEC:
            if row == "case":
                rest = ["name", rest[0]] + rest[1:]
            if row in ("basis", "pk"):
                rest = [row] + rest
            d, keys = {}, iter(rest)
            for k in keys:
                v = [next(keys)]
                if row == "plan" and k in ("npr", "have"):
                    v.append(next(keys))
                v = [x if k == "name" else int(x, 10 if k in DEC[row] else 16) for x in v]
                d[k] = v if len(v) > 1 else v[0]
            if row == "case":
                out.append({"case": d, "basis": {}})
            elif row == "plan":
                out[-1]["plan"] = d
            elif row == "basis":
                cur = out[-1]["basis"][d["basis"]] = {"head": d, "pk": []}
            elif row == "pk":
                cur["pk"].append(d)
            else:
                cur[row] = d
        elif row == "keyfactors":
            out[-1][row] = [int(x) for x in rest]
        elif row == "tables":
            out[-1][row] = int(rest[0], 16)
        elif row == "primes":
            out[-1][row] = [int(x, 16) for x in rest]
        else:
            cur[row] = [int(x, 16) for x in rest]
    return out


# ---- the views of exact values -----------------------------------------------------------------------------------------

def dbits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def fbits(x):
    return int(np.float32(x).view(np.uint32))


def limbs32(v, n):
    return [(v >> (32 * i)) & M32 for i in range(n)]


def limbs29(v):
    return [(v >> (29 * k)) & ((1 << 29) - 1) for k in range(4)]


def pad(xs, n):
    return list(xs) + [0] * (n - len(xs))


# ---- one case against the model ----------------------------------------------------------------------------------------

def expected_plan(logm, Q, B, det_only):
    det, have_det, mbq = RM.fewest_primes(logm, B, Q, False)
    rnd, have_rnd, _ = RM.fewest_primes(logm, B, Q, True)
    width_ok = 2.0 * math.log2(RM.u128_dbl(B)) + 2.0 - math.log2(RM.u128_dbl(Q)) < 50.0
    nb = 2 if (not det_only and width_ok and rnd > det) else 1
    return dict(logm=logm, npr=[det, rnd], have=[dbits(have_det), dbits(have_rnd)], mbq=dbits(mbq), rnd_width_ok=int(width_ok),
                nb=nb, rnd_ok=int(width_ok and rnd != 0 and (nb == 2 or rnd == det)), npr_max=rnd if nb == 2 else det)


def check_basis(rec, n, m, Q, B, DQt, mode, npr, where):
    logm = m.bit_length() - 1
    C = RM.Consts(n, m, Q, B, DQt, tables=False, npr=npr)
    prod = C.Mrns
    H, crt = rec["head"], rec["crt"]
    assert (H["mode"], H["npr"]) == (mode, npr), where
    # the exact bounds the double-precision sizing rules stand for
    assert (20 if mode else 5) * m * B * Q < prod, where
    for G, scale in ((H["pack_G"], 1), (H["pack_G_rnd"], 4)):
        fits = lambda g: 10 * scale * g * m * B * Q < 8 * prod          # g m B Q / 2 (x 4) < 0.4 prod
        if G:
            assert G & (G - 1) == 0 and G <= n and fits(G), (where, G)
            # maximal under the rule: the next power of two is above n, or the rule's margin of 0.001 in log2 refuses it
            assert G == n or not fits(2 * G) or 10 * scale * 2 * G * m * B * Q * 1000 > 8 * prod * 999, (where, G)
        else:
            assert not fits(1) or 10 * scale * m * B * Q * 1000 > 8 * prod * 999, where
    assert H["pack_G"] == RM.pack_group(n, logm, B, Q, False, sized_for=bool(mode)), where
    assert H["pack_G_rnd"] == RM.pack_group(n, logm, B, Q, True, sized_for=bool(mode)), where
    # CrtConst
    assert (crt["Q"], crt["B"], crt["npr"], crt["logr"]) == (Q, B, npr, logm + 1), where
    assert crt["offneg"] == (Q - C.off) % Q and crt["offneg_rnd"] == (Q - C.off_rnd) % Q, where
    assert crt["xmax"] == C.xmax and crt["DQ"] == C.DQ and crt["DQL"] == DQt >> 2, where
    assert crt["halfQ"] == Q // 2 and crt["roundthr"] == Q // 2 + (Q & 1), where
    want = [C.digits_of(a) for a in (0, C.DQ, (Q - C.DQ) % Q, DQt >> 2, (Q - (DQt >> 2)) % Q)]
    assert rec["dig"] == [x for d in want for x in d], where
    assert rec["c"] == pad(C.c, NPR_MAX) and rec["T"] == pad(C.T, ALPHA_MAX), where
    assert rec["c32"] == [w for c in pad(C.c, NPR_MAX) for w in limbs32(c, 3)], where
    assert rec["T32"] == [w for t in pad(C.T, ALPHA_MAX) for w in limbs32(t, 4)], where
    assert rec["Q32"] == limbs32(Q, 3), where
    assert rec["cd"] == pad([dbits(RM.u128_dbl(c)) for c in C.c], NPR_MAX), where
    assert rec["Td"] == pad([dbits(RM.u128_dbl(t)) for t in C.T], ALPHA_MAX), where
    assert crt["Bd"] == dbits(float(B)) and crt["invB"] == dbits(1.0 / float(B)), where
    assert crt["invQ"] == dbits(1.0 / RM.u128_dbl(Q)), where
    assert rec["invp"] == pad([fbits(np.float32(1.0) / np.float32(p)) for p in C.primes], NPR_MAX), where
    # PrimeK
    assert len(rec["pk"]) == npr
    for i, (got, P) in enumerate(zip(rec["pk"], C.pk)):
        for k in ("p", "pinv", "sR", "sRr", "hoff", "r1", "r2", "r3", "qmodp", "kappaR", "minvR"):
            assert got[k] == P[k], (where, i, k)
        assert got["invp"] == fbits(np.float32(1.0) / np.float32(P["p"])) and got["npr"] == npr and got["nulls"] == 1
    # CrtLean
    L = RM.CrtLean(C)
    K = rec["lean"]
    nq, nb = Q.bit_length(), B.bit_length()
    NL = max(2, -(-nq // 29))
    a = 29 * (NL - 1) - (nq - 29)
    assert L.ok == (nb >= 13 and NL <= 4 and nq >= 30 and 0 <= a <= 28), where      # the engine's rule, spelled out
    if not L.ok:
        assert all(v == 0 for v in K.values()) and H["lean_rnd_ok"] == 0, where
        assert not any(rec[k][i] for k in ("lean.c", "lean.w", "lean.cMn", "lean.Qw", "lean.cR") for i in range(len(rec[k])))
        return C, None
    assert (K["nl"], K["a"], K["t2"], K["sB"], K["hoff"]) == (L.NL, L.a, L.t2, L.sB, L.hoff) and L.NL == NL, where
    assert rec["lean.c"] == [w for c in pad(C.c, NPR_MAX) for w in limbs29(c)], where
    assert [x[:L.NL] for x in (limbs29(c) for c in C.c)] == L.c and limbs29(L.cRv)[:L.NL] == L.cR, where
    assert rec["lean.w"] == pad(L.w, NPR_MAX) and rec["lean.cMn"] == pad(L.cMn, 4) and rec["lean.cR"] == pad(L.cR, 4), where
    assert rec["lean.Qw"] == limbs32(Q, 3), where
    assert (K["B0"], K["B1"], K["Bw0"], K["Bw1"]) == (L.B0, L.B1, B & M32, B >> 32), where
    assert K["mq0"] | K["mq1"] << 32 == L.mq and K["mb0"] | K["mb1"] << 32 == L.mb, where
    assert K["xm2lo"] | K["xm2hi"] << 32 == 2 * C.xmax, where
    # k_crt_lean_rnd: the two conditions of the comment in derive_basis
    assert H["lean_rnd_ok"] == int((NL >= 3 or 7 * B < 1 << 32 or B >> 29 == 0) and B * B <= Q << 27), where
    if L87.accepts(C):
        F = L87.Lean87(C)
        assert K["p87"] == 1 and K["mqw0"] | K["mqw1"] << 32 == F.mq and K["mbw0"] | K["mbw1"] << 32 == F.mb, where
    else:
        assert (K["p87"], K["mqw0"], K["mqw1"], K["mbw0"], K["mbw1"]) == (0, 0, 0, 0, 0), where
    return C, L


def check_tables(path, m, primes, where):
    """One prime after another: [f | v | fp | vp], the quarter block, psi^e R, the head words."""
    raw = np.fromfile(path, dtype=np.int32).astype(np.int64)
    assert raw.size == len(primes) * (10 * m + 8), where
    ms = m // 4
    for i, p in enumerate(primes):
        blk = raw[i * (10 * m + 8):(i + 1) * (10 * m + 8)]
        f, v, fp, vp = (blk[k * m:(k + 1) * m] for k in range(4))
        twq, pw, head = blk[4 * m:8 * m], blk[8 * m:10 * m], blk[10 * m:]
        T = RM.prime_tables(p, m)
        for got, key in ((f, "twf"), (v, "twi"), (fp, "twfp"), (vp, "twip")):
            assert np.array_equal(got, T[key]), (where, i, key)
        # the quarter form: entry mm' + i' of quarter q = big entry 4 mm' + q mm' + i'; fp / vp zero below 2
        # (tests/test_rns_model.py _quarter_tables)
        jj = np.arange(1, ms)
        mmq = 1 << (np.floor(np.log2(jj)).astype(np.int64))
        for q in range(4):
            J = 4 * mmq + q * mmq + (jj - mmq)
            for k, big in enumerate((f, v, fp, vp)):
                want = np.zeros(ms, dtype=np.int64)
                want[1:] = big[J]
                if k >= 2:
                    want[:2] = 0
                assert np.array_equal(twq[q * m + k * ms:q * m + (k + 1) * ms], want), (where, i, q, k)
        R1, want, x = (1 << 32) % p, np.zeros(2 * m, dtype=np.int64), 1
        for e in range(2 * m):
            want[e] = x
            x = x * T["psi"] % p
        want = want * R1 % p
        want = np.where(want > (p - 1) // 2, want - p, want)
        assert np.array_equal(pw, want), (where, i, "pw")
        assert list(head) == [f[1], f[2], f[3], fp[2], fp[3], v[1], v[2], v[3]], (where, i, "head")


def check_case(rec, n, m, Q, B, DQt, det_only, tables=None, ring=None):
    where = rec["case"]["name"]
    logm = m.bit_length() - 1
    assert "refusal" not in rec, (where, rec.get("refusal"))
    plan = expected_plan(logm, Q, B, det_only)
    assert rec["plan"] == plan, (where, rec["plan"], plan)
    assert rec["primes"] == RM.rns_primes(), where
    assert sorted(rec["basis"]) == list(range(plan["nb"])), where
    lean = {}
    for b in rec["basis"]:
        mode = 1 if (plan["nb"] == 2 and b == 1) else 0
        _, lean[b] = check_basis(rec["basis"][b], n, m, Q, B, DQt, mode, plan["npr"][mode], "%s basis %d" % (where, b))
    if plan["rnd_ok"] and plan["nb"] == 1:      # one basis for both modes: it covers the randomised bound too
        assert 20 * m * B * Q < math.prod(RM.rns_primes()[:plan["npr"][0]]), where
    if plan["nb"] == 2:
        small, big = RM.rns_primes()[:plan["npr"][0]], RM.rns_primes()[:plan["npr"][1]]
        extra = math.prod(big[len(small):])
        assert rec["keyfactors"] == pad([RM.centre((1 << 32) * extra, p) for p in small], NPR_MAX), where
    else:
        assert "keyfactors" not in rec, where
    if tables:
        check_tables(tables, m, RM.rns_primes()[:plan["npr_max"]], where)
    if ring is not None:        # tests/ring_cases.py: what Engine.kernel_names() must report fixes npr and the limbs
        for rnd in ((False,) if det_only and not plan["rnd_ok"] else (False, True)):
            H = rec["basis"][plan["nb"] - 1 if rnd else 0]
            name, args = re.fullmatch(r"(\w+)<(.*)>", ring.kernels[rnd][1]).groups()
            args = [x.strip() for x in args.split(",")]
            if name.startswith("k_crt_lean"):
                assert (H["head"]["npr"], H["lean"]["nl"]) == (int(args[0]), int(args[1])), (where, rnd)
                assert not rnd or H["head"]["lean_rnd_ok"] == 1, where
            else:
                assert H["lean"]["nl"] == 0 or (rnd and not H["head"]["lean_rnd_ok"]), (where, rnd)


# ---- the cases ---------------------------------------------------------------------------------------------------------

def named_cases():
    """[(name, (n, m, Q, B, DQ_tilde), ring | None)]: the parameter sets of bench.make_params, the rings of
    tests/ring_cases.py, and the edge pairs of test_crt_lean87_model._cases."""
    import bench
    import ring_cases as RC
    import sgfhe_jl_amd as S
    out = []
    for name in ("params64", "params512", "params1024", "params2048", "synth64", "rns2"):
        p = bench.make_params(S, name)
        out.append((name, (p.n, p.m, p.Q, p.B, p.DQ_tilde), None))
    for name in RC.NAMES:
        rg = RC.ring(S, name)
        p = rg.params
        out.append((name, (p.n, p.m, p.Q, p.B, p.DQ_tilde), rg))
    out += [(name, args, None) for name, args in L87._cases() if name.startswith("edge")]
    assert len(out) == 17
    return out


def sweep_cases():
    """m = 64: every bits(Q) from 2 to 93 at Q = 2^(k-1) + 1 and 2^k - 1, each with B at ceil(sqrt(Q)), 2^46 and
    2^47 - 1 (where B^2 >= Q allows); m = 16384 with the largest Q and B, where the most primes are taken."""
    out = []
    for k in range(2, 94):
        for Q in ((1 << (k - 1)) + 1, (1 << k) - 1):
            root = math.isqrt(Q - 1) + 1
            for B in sorted(B for B in {max(root, 2), 1 << 46, (1 << 47) - 1} if B * B >= Q):
                out.append(("sweep_q%d_%x_%x" % (k, Q, B), (16, 64, Q, B, Q // 8)))
    for Q in (((1 << 47) - 1) ** 2, (1 << 93) + 1, (1 << 94) - (1 << 70), (1 << 92) - 1):     # (B < 2^47 and B^2 >= Q)
        for B in sorted(B for B in {(1 << 47) - 1, 1 << 46, math.isqrt(Q - 1) + 1} if B * B >= Q):
            out.append(("sweep_m16384_%x_%x" % (Q, B), (4096, 16384, Q, B, Q - 1)))
    return out


def request(name, args, det_only, tables):
    """(three edge pairs of test_crt_lean87_model have B^2 < Q: ctx creation refuses them, test_key_factors_rns2_and_refusals
    says so; their constants are derived all the same, as that model test derives them)"""
    n, m, Q, B, DQt = args
    return ("case" if B * B >= Q else "unchecked") + " %s %d %d %x %x %x %d %s" % (name, n, m, Q, B, DQt, det_only, tables)


def test_named_parameter_sets_with_tables(programs):
    cases = named_cases()
    tmp = programs[2]
    reqs, paths = [], []
    for name, args, _ in cases:
        for det_only in (0, 1):
            paths.append(str(tmp / ("%s_%d.tables" % (name, det_only))))
            reqs.append(request(name, args, det_only, paths[-1]))
    recs = parse(run(programs, reqs))
    assert len(recs) == len(reqs)
    seen = {}
    for k, rec in enumerate(recs):
        name, args, ring = cases[k // 2]
        check_case(rec, *args, det_only=k % 2, tables=paths[k], ring=ring)
        seen[(name, k % 2)] = rec
    # what tests/ring_cases.py says in prose
    assert seen[("tiny", 0)]["basis"][0]["lean"]["nl"] == 0
    assert [seen[("limb64", 0)]["basis"][b]["head"]["npr"] for b in (0, 1)] == [4, 5]
    assert seen[("wide", 0)]["plan"]["npr"] == [6, 6] and seen[("wide", 0)]["basis"][0]["lean"]["nl"] == 4
    # Params(1024): five primes against six, and the deterministic-only ctx keeps the five
    assert seen[("params1024", 0)]["plan"]["npr"] == [5, 6] and seen[("params1024", 0)]["plan"]["nb"] == 2
    assert seen[("params1024", 1)]["plan"]["nb"] == 1 and seen[("params1024", 1)]["plan"]["rnd_ok"] == 0
    assert {name for (name, d), r in seen.items() if d == 0 and r["basis"][0]["lean"]["p87"]} == \
        {"params1024", "rns2"} | {"edge%d" % i for i in range(6)}


def test_sweep_of_moduli(programs):
    cases = sweep_cases()
    reqs = [request(name, args, det_only, "-") for name, args in cases for det_only in (0, 1)]
    recs = parse(run(programs, reqs))
    assert len(recs) == len(reqs)
    for k, rec in enumerate(recs):
        check_case(rec, *cases[k // 2][1], det_only=k % 2)
    nprs = {tuple(r["plan"]["npr"]) for r in recs}
    # 20 m B Q < 2^4.33 2^14 2^47 2^94 = 2^159.33 takes six primes of 29 bits and never the seventh candidate
    assert max(b for _, b in nprs) == 6 and min(a for a, _ in nprs) == 2
    assert any(r["basis"][0]["lean"]["nl"] == 0 for r in recs) and {r["basis"][0]["lean"]["nl"] for r in recs} >= {2, 3, 4}


def test_key_factors_rns2_and_refusals(programs):
    import bench
    import ring_cases as RC
    import sgfhe_jl_amd as S
    pairs = [bench.rns2_moduli(S), RC.ring(S, "composite").rns2]
    rns2 = ["rns2 %x %x %x" % (m1 * m2, m1, m2) for m1, m2 in pairs] + ["rns2 %x %x %x" % (m1 * m2, m2, m1) for m1, m2 in pairs]
    bad = {"rns2 %x %x %x" % (pairs[0][0] * pairs[0][1] + 2, pairs[0][0], pairs[0][1]): (-1, "m1 * m2 != Q"),
           "rns2 %x %x %x" % (1 << 48, 1 << 47, 2): (-2, "RNS2 limb moduli must be in [2, 2^47)"),
           "rns2 %x %x %x" % (1 << 48, 1, 1 << 48): (-2, "RNS2 limb moduli must be in [2, 2^47)"),
           "rns2 %x %x %x" % (49, 7, 7): (-1, "RNS2 limb moduli must be distinct primes"),
           "rns2 %x %x %x" % (15 * 7, 15, 7): (-1, "RNS2 limb moduli must be distinct primes")}
    refusals = dict(REFUSALS)
    for name, (n, m, Q, B, DQt), _ in named_cases():
        if B * B < Q:
            assert name in ("edge0", "edge3", "edge4")
            refusals["check 2 %d %d %d %x %x %x" % (m, 2 * m, n, Q, B, DQt)] = (-1, "B^2 must be >= Q")
    reqs = rns2 + list(bad) + list(refusals)
    lines = run(programs, reqs)
    assert len(lines) == len(reqs)
    for (m1, m2), line in zip(pairs + [(b, a) for a, b in pairs], lines):
        d = dict(zip(line.split()[1::2], (int(x, 16) for x in line.split()[2::2])))
        assert line.startswith("rns2 ") and (d["m1"], d["m2"]) == (m1, m2), line
        assert d["i21"] < m1 and d["i21"] * m2 % m1 == 1 and d["i12"] < m2 and d["i12"] * m1 % m2 == 1, line
        assert (d["inv1"], d["inv2"]) == (dbits(1.0 / float(m1)), dbits(1.0 / float(m2))), line
    for (req, want), line in zip(list(bad.items()) + list(refusals.items()), lines[len(rns2):]):
        if want is None:
            m = int(req.split()[2])
            assert line == "accepted %d" % (m.bit_length() - 1), (req, line)
        else:
            assert line == "refusal %d %s" % want, (req, line)
