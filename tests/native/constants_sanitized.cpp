// The constants of csrc/constants.h -- check_params, plan_bases, derive_basis, prime_tables, key_factors, rns2_const --
// under AddressSanitizer and UndefinedBehaviorSanitizer on the CPU (tests/test_constants_host.py, which compares every
// field printed here with Python big integers).  A stand-alone program; it reads one request per line from stdin:
//   case <name> <n> <m> <Q> <B> <DQ_tilde> <det_only> <tables>
//       Q, B and DQ_tilde in hex.  <tables> is "-" (no tables), "+" (compute them and print their hash) or a file name:
//       the tables of every prime of the larger basis go there as raw int32, per prime
//       [f | v | fp | vp] (4 m), the quarter block (4 m), psi^e R (2 m) and the eight head words.
//       Prints the plan, every basis (CrtConst, CrtLean and each PrimeK, big values in hex, doubles and floats as
//       their IEEE bits) and, with two bases, the KeyFactors -- or the refusal.
//   unchecked <the same fields>
//       The same without check_params first, for a power of two m and Q >= 3, B >= 2 within the widths: the edge pairs of
//       tests/test_crt_lean87_model.py with B^2 < Q, which ctx creation refuses and the arithmetic does not depend on.
//   check <ell> <m> <r> <n> <Q> <B> <DQ_tilde>          check_params alone: "accepted <logm>" or the refusal
//   rns2 <Q> <m1> <m2>                                  rns2_const: the record or the refusal (all in hex)
// Ends with "ok <cases>".
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>

#include "constants.h"

using namespace sgfhe;

static u128 parse_hex(const char *s) {
    u128 v = 0;
    for (; *s; s++) {
        const int d = *s >= '0' && *s <= '9' ? *s - '0' : *s >= 'a' && *s <= 'f' ? *s - 'a' + 10 : -1;
        if (d < 0 || (v >> 124)) { fprintf(stderr, "bad hex\n"); exit(2); }
        v = (v << 4) | (unsigned)d;
    }
    return v;
}
static std::string hex(u128 v) {
    char buf[40];
    if (v >> 64) snprintf(buf, sizeof buf, "%llx%016llx", (unsigned long long)(v >> 64), (unsigned long long)v);
    else snprintf(buf, sizeof buf, "%llx", (unsigned long long)v);
    return buf;
}
static unsigned long long bits(double d) { unsigned long long u; memcpy(&u, &d, 8); return u; }
static unsigned bits(float f) { unsigned u; memcpy(&u, &f, 4); return u; }
static void words(u128 v, uint64_t w[2]) { w[0] = (uint64_t)v; w[1] = (uint64_t)(v >> 64); }
static void refusal(const Refusal &r) { printf("refusal %d %s\n", r.code, r.msg); }

#define ROW_U128(name, arr, n) do { printf(" " name); for (int i_ = 0; i_ < (int)(n); i_++) printf(" %s", hex(arr[i_]).c_str()); printf("\n"); } while (0)
#define ROW_U32(name, arr, n) do { printf(" " name); for (int i_ = 0; i_ < (int)(n); i_++) printf(" %x", (unsigned)(arr)[i_]); printf("\n"); } while (0)

static void print_basis(int b, int mode, const BasisConst &K, uint32_t npr) {
    const CrtConst &c = K.crt;
    printf("basis %d mode %d npr %u lean_rnd_ok %d pack_G %u pack_G_rnd %u\n", b, mode, npr, (int)K.lean_rnd_ok, K.pack_G,
           K.pack_G_rnd);
    printf(" crt Q %s B %s offneg %s offneg_rnd %s xmax %llx DQ %s halfQ %s roundthr %s invQ %llx invB %llx Bd %llx npr %u "
           "logr %u DQL %s\n", hex(c.Q).c_str(), hex(c.B).c_str(), hex(c.offneg).c_str(), hex(c.offneg_rnd).c_str(),
           (unsigned long long)c.xmax, hex(c.DQ).c_str(), hex(c.halfQ).c_str(), hex(c.roundthr).c_str(), bits(c.invQ),
           bits(c.invB), bits(c.Bd), c.npr, c.logr, hex(c.DQL).c_str());
    const ulonglong2 *dg[5] = {&c.dig0, &c.digP, &c.digN, &c.digPL, &c.digNL};
    printf(" dig");
    for (const ulonglong2 *d : dg) printf(" %llx %llx", (unsigned long long)d->x, (unsigned long long)d->y);
    printf("\n");
    ROW_U128("c", c.c, NPR_MAX);            // (all NPR_MAX / CRT_ALPHA_MAX entries: those past npr must be zero)
    ROW_U128("T", c.T, CRT_ALPHA_MAX);
    ROW_U32("c32", &c.c32[0][0], NPR_MAX * 3);
    ROW_U32("Q32", c.Q32, 3);
    ROW_U32("T32", &c.T32[0][0], CRT_ALPHA_MAX * 4);
    printf(" cd"); for (int i = 0; i < NPR_MAX; i++) printf(" %llx", bits(c.cd[i])); printf("\n");
    printf(" Td"); for (int i = 0; i < CRT_ALPHA_MAX; i++) printf(" %llx", bits(c.Td[i])); printf("\n");
    printf(" invp"); for (int i = 0; i < NPR_MAX; i++) printf(" %x", bits(c.invp[i])); printf("\n");
    const CrtLean &L = K.lean;
    printf(" lean nl %u hoff %x B0 %x B1 %x Bw0 %x Bw1 %x mq0 %x mq1 %x mb0 %x mb1 %x a %u t2 %u sB %u xm2lo %x xm2hi %x "
           "p87 %u mqw0 %x mqw1 %x mbw0 %x mbw1 %x\n", L.nl, L.hoff, L.B0, L.B1, L.Bw0, L.Bw1, L.mq0, L.mq1, L.mb0, L.mb1,
           L.a, L.t2, L.sB, L.xm2lo, L.xm2hi, L.p87, L.mqw0, L.mqw1, L.mbw0, L.mbw1);
    ROW_U32("lean.c", &L.c[0][0], NPR_MAX * 4);
    ROW_U32("lean.w", L.w, NPR_MAX);
    ROW_U32("lean.cMn", L.cMn, 4);
    ROW_U32("lean.Qw", L.Qw, 3);
    ROW_U32("lean.cR", L.cR, 4);
    for (uint32_t i = 0; i < npr; i++) {
        const PrimeK &P = K.pk[i];
        const bool nulls = !P.twf && !P.twi && !P.twq && !P.pw && !P.f1 && !P.f2 && !P.f3 && !P.fp2 && !P.fp3 && !P.v1 &&
                           !P.v2 && !P.v3;
        printf(" pk %u p %d pinv %x sR %d sRr %d hoff %u r1 %d r2 %d r3 %d qmodp %d kappaR %d minvR %d invp %x npr %u "
               "nulls %d\n", i, P.p, P.pinv, P.sR, P.sRr, P.hoff, P.r1, P.r2, P.r3, P.qmodp, P.kappaR, P.minvR,
               bits(P.invp), P.npr, (int)nulls);
    }
}

static unsigned long long n_cases = 0;

static void run_case(char **f, bool checked) {
    sgfhe_params p;
    memset(&p, 0, sizeof p);
    p.n = strtoull(f[2], nullptr, 10);
    p.m = strtoull(f[3], nullptr, 10);
    p.r = 2 * p.m;
    p.ell = 2;
    const u128 Q = parse_hex(f[4]), B = parse_hex(f[5]), DQ = parse_hex(f[6]);
    words(Q, p.Q);
    words(B, p.B);
    words(DQ, p.DQ_tilde);
    const bool det_only = atoi(f[7]) != 0;
    const char *tables = f[8];
    printf("case %s det_only %d\n", f[1], (int)det_only);
    n_cases++;
    int logm = 0;
    Refusal r;
    if (checked) {
        if ((r = check_params(p, &logm))) { refusal(r); return; }
    } else {
        while ((1ull << logm) < p.m) logm++;
    }
    BasisPlan plan;
    if ((r = plan_bases(logm, Q, B, det_only, &plan))) { refusal(r); return; }
    printf("plan logm %d npr %u %u have %llx %llx mbq %llx rnd_width_ok %d nb %d rnd_ok %d npr_max %u\n", logm, plan.npr[0],
           plan.npr[1], bits(plan.log_have[0]), bits(plan.log_have[1]), bits(plan.log_mbq), (int)plan.rnd_width_ok, plan.nb,
           (int)plan.rnd_ok, plan.npr_max);
    ROW_U32("primes", plan.primes, NPR_MAX);
    // the larger basis first, as the engine takes them
    for (int b = plan.nb - 1; b >= 0; b--) {
        const int mode = plan.mode_of(b);
        BasisConst K;
        derive_basis(logm, (uint32_t)p.n, Q, B, DQ, plan.primes, plan.npr[mode], plan.log_have[mode], plan.log_mbq, &K);
        print_basis(b, mode, K, plan.npr[mode]);
    }
    if (plan.nb == 2) {
        const KeyFactors fac = key_factors(plan.primes, plan.npr[0], plan.npr[1]);
        printf("keyfactors");
        for (int i = 0; i < NPR_MAX; i++) printf(" %d", fac.f[i]);
        printf("\n");
    }
    if (strcmp(tables, "-")) {
        FILE *out = strcmp(tables, "+") ? fopen(tables, "wb") : nullptr;
        if (strcmp(tables, "+") && !out) { fprintf(stderr, "cannot write %s\n", tables); exit(2); }
        uint64_t h = 0xcbf29ce484222325ull;
        PrimeTables T;
        for (uint32_t i = 0; i < plan.npr_max; i++) {
            if ((r = prime_tables(plan.primes[i], logm, &T))) { refusal(r); break; }
            const std::vector<int32_t> head(T.head, T.head + 8);
            const std::vector<int32_t> *parts[4] = {&T.tw, &T.twq, &T.pw, &head};
            for (const std::vector<int32_t> *v : parts) {
                for (int32_t x : *v) { h ^= (uint32_t)x; h *= 0x100000001b3ull; }
                if (out && fwrite(v->data(), 4, v->size(), out) != v->size()) { fprintf(stderr, "short write\n"); exit(2); }
            }
        }
        if (out) fclose(out);
        printf("tables %llx\n", (unsigned long long)h);
    }
}

int main() {
    static char line[4096];
    while (fgets(line, sizeof line, stdin)) {
        char *f[16];
        int nf = 0;
        for (char *t = strtok(line, " \t\r\n"); t && nf < 16; t = strtok(nullptr, " \t\r\n")) f[nf++] = t;
        if (!nf) continue;
        if ((!strcmp(f[0], "case") || !strcmp(f[0], "unchecked")) && nf == 9) {
            run_case(f, f[0][0] == 'c');
        } else if (!strcmp(f[0], "check") && nf == 8) {
            sgfhe_params p;
            memset(&p, 0, sizeof p);
            p.ell = strtoull(f[1], nullptr, 10);
            p.m = strtoull(f[2], nullptr, 10);
            p.r = strtoull(f[3], nullptr, 10);
            p.n = strtoull(f[4], nullptr, 10);
            words(parse_hex(f[5]), p.Q);
            words(parse_hex(f[6]), p.B);
            words(parse_hex(f[7]), p.DQ_tilde);
            int logm = -1;
            const Refusal r = check_params(p, &logm);
            if (r) refusal(r);
            else printf("accepted %d\n", logm);
            n_cases++;
        } else if (!strcmp(f[0], "rns2") && nf == 4) {
            Rns2Const rc;
            memset(&rc, 0, sizeof rc);
            const Refusal r = rns2_const(parse_hex(f[1]), (uint64_t)parse_hex(f[2]), (uint64_t)parse_hex(f[3]), &rc);
            if (r) refusal(r);
            else printf("rns2 m1 %llx m2 %llx i21 %llx i12 %llx inv1 %llx inv2 %llx\n", (unsigned long long)rc.m1,
                        (unsigned long long)rc.m2, (unsigned long long)rc.i21, (unsigned long long)rc.i12, bits(rc.inv1),
                        bits(rc.inv2));
            n_cases++;
        } else {
            fprintf(stderr, "bad request: %s\n", f[0]);
            return 2;
        }
    }
    printf("ok %llu\n", n_cases);
    return 0;
}
