// Every constant the kernels read, as plain data, and its derivation on the host (DESIGN.md sections 3 and 11): the
// RNS primes and how many each flatten mode takes, the CRT / flatten constants (CrtConst, CrtLean), the per-prime
// records (PrimeK), the twiddle tables of a prime, the pack group sizes, the factors of key_derive, the idempotents of
// the RNS2Number form, and the parameter check of sgfhe_ctx_create_ex.  Pure functions of values: no ctx, no device
// call, no environment.  A refusal is a code and a message (Refusal), which the engine hands to fail().
// engine.hip allocates, uploads and sets the device pointers; tests/rns_model.py restates the same rules in Python big
// integers, and tests/test_constants_host.py holds the two together field by field.
// Plain C++ (ulonglong2 is that of <hip/hip_vector_types.h>, which needs no HIP runtime):
// tests/native/constants_sanitized.cpp drives this header under ASan / UBSan on the CPU.
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include <hip/hip_vector_types.h>

#include "../../include/sgfhe_hip.h"

namespace sgfhe {

typedef unsigned __int128 u128;

constexpr int NPR_MAX = 7;  // at most this many RNS primes (p_i < 2^29); a ctx uses the fewest whose
                            // product covers 5 m B Q (4 at Params(64), 5 at Params(512/1024))

struct PrimeK {
    int32_t p;        // prime, < 2^29
    uint32_t pinv;    // p^-1 mod 2^32
    int32_t sR;       // -(s R^-1) mod p, centred (digit offset s of utils.jl:162-166, R = 2^32)
    int32_t sRr;      // the same for the randomised flatten: offset s + xmax (utils.jl:198-241)
    uint32_t hoff;    // offset added to the output residue: (p-1)/2 for the last prime, else 0
    int32_t r1, r2, r3;  // R, R^2, R^3 mod p, centred
    int32_t qmodp;    // Q mod p, centred
    int32_t kappaR;   // key scale kappa * R mod p (centred), kappa = R^2 m^-1 (M/p)^-1 mod p
    int32_t minvR;    // m^-1 * R mod p, centred (debug inverse NTT scaling)
    float invp;       // 1 / p
    const int32_t *twf;  // forward twiddles psi^bitrev(i) * R mod p (Montgomery form, centred)
    const int32_t *twi;  // inverse twiddles psi^-bitrev(i) * R mod p
    uint32_t npr;     // number of primes of the ctx (the same in every record)
    // quarter form of the latency kernels (k_fwd_quarter / k_inv_quarter / k_crt_lean1q):
    int32_t f1, f2, f3, fp2, fp3;   // forward twiddles of the first two stages: twf[1..3], and the products twf[2 m + 2], [2 m + 3]
    int32_t v1, v2, v3;             // inverse twiddles of the last two stages: twi[1..3]
    const int32_t *twq;  // twiddle tables of the four quarter transforms: block q = [f_q | v_q | fp_q | vp_q], m / 4 words each
    const int32_t *pw;   // psi^e * R mod p, centred, e in [0, 2 m): (x^j - 1) in the NTT domain is psi^(j (2 brv(s) + 1)) - 1 at slot s
};

constexpr int CRT_ALPHA_MAX = 6 * NPR_MAX + 2;  // entries of the alpha-indexed CRT correction table

// CRT / flatten constants, resident in device memory.
struct CrtConst {
    u128 Q, B;
    u128 c[NPR_MAX];     // (M / p_i) mod Q
    u128 T[CRT_ALPHA_MAX];   // (-alpha * M - H') mod Q,  H' = (M / p_last) * (p_last - 1) / 2;
                             // alpha < 6 npr + 1: the residues are non-negative representatives
                             // below 5.7 p (6.2 p for the last prime), not canonical ones
    u128 offneg;         // (Q - off) mod Q, off = (1 + B) s mod Q
    u128 offneg_rnd;     // the same with s + xmax in place of s (randomised flatten)
    uint64_t xmax;       // v_i uniform in [-xmax, xmax], xmax = 3 (B / 2) (utils.jl:210-214)
    u128 DQ;             // DQ_tilde mod Q
    u128 halfQ;          // Q / 2 (centred lift of key residues)
    u128 roundthr;       // Q / 2 + (Q odd)        (utils.jl:84)
    double invQ, invB;
    // 32-bit limb / double views of the same constants for k_crt_acc's 96-bit arithmetic
    uint32_t c32[NPR_MAX][3];
    uint32_t Q32[3];
    alignas(16) uint32_t T32[CRT_ALPHA_MAX][4];
    double cd[NPR_MAX], Td[CRT_ALPHA_MAX], Bd;
    float invp[NPR_MAX];
    uint32_t npr;        // number of primes in use
    uint32_t logr;
    ulonglong2 dig0, digP, digN;  // (lo, hi) digits of x' for acc = 0, DQ_tilde, Q - DQ_tilde
    // LUT rows (sgfhe_bootstrap_lut_batch) start at a quarter of the amplitude
    u128 DQL;                     // A0 = DQ_tilde >> 2
    ulonglong2 digPL, digNL;      // digits of x' for acc = A0, Q - A0
};

// The constants of k_crt_lean (kernels.h, where the kernel's arithmetic is described).
struct CrtLean {
    uint32_t c[NPR_MAX][4];   // (M / p_i) mod Q in 29-bit limbs
    uint32_t w[NPR_MAX];      // floor(2^58 / p_i)
    uint32_t cMn[4];          // (-M) mod Q in 29-bit limbs
    uint32_t hoff;            // (p_last - 1) / 2, the offset k_extprod adds to the last prime's residue
    uint32_t Qw[3];           // Q in 32-bit words
    uint32_t B0, B1;          // B = B0 + B1 2^29
    uint32_t Bw0, Bw1;        // B in 32-bit words
    uint32_t mq0, mq1;        // floor(2^(t + 72) / Q)
    uint32_t mb0, mb1;        // floor(2^(bits(B) + 51) / B)
    uint32_t a;               // top limb sum << a, the next >> 29 - a, the next >> 58 - a
    uint32_t t2, sB;          // x >> t2;  final shift of the digit estimate
    uint32_t nl;              // limbs in use (2, 3 or 4); 0 = parameter set outside this kernel's bounds
    uint32_t cR[4];           // randomised flatten: (-2 xmax (1 + B)) mod Q in 29-bit limbs
    uint32_t xm2lo, xm2hi;    //   2 xmax
    uint32_t p87;             // 1: crt_lean87_one applies (five primes, Q of 87 bits, B of 44 bits)
    uint32_t mqw0, mqw1;      //   floor(2^122 / Q)
    uint32_t mbw0, mbw1;      //   floor(2^96 / B)
};

// k_key_derive: one constant per prime of the smaller basis (key_factors below).
struct KeyFactors {
    int32_t f[NPR_MAX];
};

// k_rns2_to_canon / k_canon_to_rns2 (rns2_const below).
struct Rns2Const {
    uint64_t m1, m2;   // limb moduli, distinct primes below 2^47
    uint64_t i21, i12; // m2^-1 mod m1, m1^-1 mod m2
    double inv1, inv2; // 1 / m1, 1 / m2
};

// A refusal of one of the functions below: an SGFHE_ERR_* code and the message of sgfhe_last_error_string.
struct Refusal {
    int32_t code = SGFHE_OK;
    const char *msg = "";
    explicit operator bool() const { return code != SGFHE_OK; }
};

// ---------------------------------------------------------------- host number theory (word size)

inline uint32_t mulmod32(uint32_t a, uint32_t b, uint32_t p) { return (uint32_t)((uint64_t)a * b % p); }
inline uint32_t powmod32(uint32_t a, uint64_t e, uint32_t p) {
    uint32_t r = 1 % p;
    a %= p;
    while (e) {
        if (e & 1) r = mulmod32(r, a, p);
        a = mulmod32(a, a, p);
        e >>= 1;
    }
    return r;
}
inline bool is_prime32(uint32_t x) {
    if (x < 2) return false;
    for (uint32_t q : {2u, 3u, 5u, 7u, 11u, 13u}) {
        if (x % q == 0) return x == q;
    }
    uint32_t d = x - 1;
    int s = 0;
    while (!(d & 1)) { d >>= 1; s++; }
    for (uint32_t a : {2u, 3u, 5u, 7u}) {  // deterministic below 3,215,031,751
        uint32_t y = powmod32(a, d, x);
        if (y == 1 || y == x - 1) continue;
        bool comp = true;
        for (int i = 0; i < s - 1; i++) {
            y = mulmod32(y, y, x);
            if (y == x - 1) { comp = false; break; }
        }
        if (comp) return false;
    }
    return true;
}
inline uint32_t bitrev(uint32_t x, int bits) {
    uint32_t r = 0;
    for (int i = 0; i < bits; i++) { r = (r << 1) | (x & 1); x >>= 1; }
    return r;
}
inline u128 ld128(const uint64_t *w) { return ((u128)w[1] << 64) | w[0]; }
inline int32_t centre32(uint32_t x, uint32_t p) { return x > (p - 1) / 2 ? (int32_t)x - (int32_t)p : (int32_t)x; }
inline double u128_dbl(u128 x) { return (double)(uint64_t)(x >> 64) * 18446744073709551616.0 + (double)(uint64_t)x; }
inline double u128_log2(u128 x) { return log2(u128_dbl(x)); }

// ---------------------------------------------------------------- the parameter check of sgfhe_ctx_create_ex

// What the engine implements of the reference's parameter sets; *logm = log2 m where nothing is refused.
inline Refusal check_params(const sgfhe_params &p, int *logm) {
    const uint64_t m = p.m;
    if (p.ell != 2) return {SGFHE_ERR_UNSUPPORTED, "ell must be 2 (fhe.jl:576)"};
    if (m < 64 || m > 16384 || (m & (m - 1)))
        return {SGFHE_ERR_UNSUPPORTED, "m must be a power of two in [2^6, 2^14]"};
    if (p.r != 2 * m) return {SGFHE_ERR_INVALID_ARG, "r must equal 2 m (fhe.jl:62)"};
    if (p.n == 0 || p.n > m / 4 || (p.n & (p.n - 1)))
        return {SGFHE_ERR_INVALID_ARG, "n must be a power of two in [1, m / 4] (fhe.jl:45-46; extract, fhe.jl:585-590)"};
    const u128 Q = ld128(p.Q), B = ld128(p.B);
    if (Q < 3 || (Q >> 94)) return {SGFHE_ERR_UNSUPPORTED, "Q must be in [3, 2^94)"};
    if (B < 2 || (B >> 47)) return {SGFHE_ERR_UNSUPPORTED, "B must be in [2, 2^47)"};
    // B^2 >= Q (utils.jl:145); B < 2^47 so B*B fits 128 bits
    if (B * B < Q) return {SGFHE_ERR_INVALID_ARG, "B^2 must be >= Q"};
    if (ld128(p.DQ_tilde) >= Q) return {SGFHE_ERR_INVALID_ARG, "DQ_tilde must be < Q"};
    *logm = 0;
    while ((1ull << *logm) < m) ++*logm;
    return {};
}

// ---------------------------------------------------------------- the basis plan

// Which primes a ctx uses.  Index 0 is the deterministic flatten, index 1 the randomised one.
struct BasisPlan {
    uint32_t primes[NPR_MAX];   // the candidates, largest first; a basis takes the first npr[mode] of them
    uint32_t npr[2];            // primes the mode's exactness bound takes (0: more than the candidates cover)
    double log_have[2];         // log2 of their product, as the sizing rule summed it
    double log_mbq;             // log2(m B Q), likewise
    bool rnd_width_ok;          // the randomised flatten's reductions are exact for these B and Q
    int nb;                     // bases of the ctx: 2 where the randomised mode takes one prime more
    bool rnd_ok;                // the ctx has the randomised mode
    uint32_t npr_max;           // primes of the larger basis
    int mode_of(int b) const { return b == nb - 1 && nb == 2 ? 1 : 0; }   // the mode whose sizing basis b has
};

// RNS primes: the largest primes below 2^29 with p = 1 mod 2^15 (2 m | p - 1 for every
// supported m), as many as the exactness bound needs.  The exact integer the CRT has to
// recover is D = (x^j - 1) sum_row u_row (*) C_row with |u| <= B / 2 (deterministic flatten,
// utils.jl:155-189) and the key lifted to |C| <= Q / 2, so |D| <= 2 m B Q; k_crt_acc needs
// |D| <= 0.4 M_rns, i.e. 5 m B Q <= M_rns.  The randomised flatten (|u| <= 2 B,
// utils.jl:198-241) needs a factor 4 more.  Where that takes one more prime (Params(1024): six
// against five) the ctx gets a basis per mode (sgfhe_ctx::Basis), unless it was created with
// SGFHE_CTX_DETERMINISTIC_ONLY.
inline Refusal plan_bases(int logm, u128 Q, u128 B, bool det_only, BasisPlan *out) {
    BasisPlan &P = *out;
    memset(&P, 0, sizeof P);
    {
        int found = 0;
        for (uint64_t kk = ((1ull << 29) - 1) >> 15; kk > 0 && found < NPR_MAX; kk--) {
            uint32_t cand = (uint32_t)((kk << 15) + 1);
            if (cand < (1u << 29) && is_prime32(cand)) P.primes[found++] = cand;
        }
        if (found < NPR_MAX) return {SGFHE_ERR_UNSUPPORTED, "could not find RNS primes"};
    }
    P.log_mbq = logm + u128_log2(B) + u128_log2(Q);
    const double log_need = log2(5.0) + P.log_mbq + 0.001;
    auto fewest = [&](double target, double *have) {
        uint32_t npr = 0;
        double lh = 0;
        while (npr < NPR_MAX && (npr < 2 || lh < target)) lh += log2((double)P.primes[npr++]);
        *have = lh;
        return lh >= target ? npr : 0u;
    };
    P.npr[0] = fewest(log_need, &P.log_have[0]);
    if (!P.npr[0]) return {SGFHE_ERR_UNSUPPORTED, "5 m B Q exceeds the product of the RNS primes"};
    // |u| <= 2 B in the randomised mode: the exactness bound needs 4 x more head-room.  Its reductions
    // (random_digits, acc_from_digits, crt_reduce) divide values up to about 4 B^2 by Q with a
    // double-precision quotient estimate, exact while the quotient stays below 2^50.
    // (stored digits reach 4 B: above 2^48 they take the third plane of the digit record,
    // MODE_WIDE; B < 2^47 is checked at ctx creation)
    P.rnd_width_ok = 2.0 * u128_log2(B) + 2.0 - u128_log2(Q) < 50.0;
    P.npr[1] = fewest(log_need + 2.0, &P.log_have[1]);
    P.nb = (!det_only && P.rnd_width_ok && P.npr[1] > P.npr[0]) ? 2 : 1;
    P.rnd_ok = P.rnd_width_ok && P.npr[1] != 0 && (P.nb == 2 || P.npr[1] == P.npr[0]);
    P.npr_max = P.nb == 2 ? P.npr[1] : P.npr[0];
    return {};
}

// ---------------------------------------------------------------- one basis

// Everything that depends on which primes are in use, but for the twiddle tables: CRT / flatten constants and the
// per-prime records.  The pointer fields of the records (twf, twi, twq, pw) and the head words they copy from the
// tables (f1 ... v3) are null / zero here: the engine sets them once the tables are on the device.
struct BasisConst {
    CrtConst crt;
    CrtLean lean;               // nl = 0: this parameter set keeps k_crt_acc
    PrimeK pk[NPR_MAX];
    bool lean_rnd_ok;           // k_crt_lean_rnd's width bounds hold for this parameter set
    uint32_t pack_G, pack_G_rnd;  // key slices per exact-accumulation group of the packing path
                                  // (deterministic / randomised flatten; 0 = not available)
};

// primes[0 .. npr), log_have and log_mbq as plan_bases gives them for the mode the basis is sized for.
inline void derive_basis(int logm, uint32_t n, u128 Q, u128 B, u128 DQ_tilde, const uint32_t *primes, uint32_t npr,
                         double log_have, double log_mbq, BasisConst *out) {
    memset(out, 0, sizeof *out);   // (padding included: the records go to the device byte for byte)
    const uint32_t M = 1u << logm;
    const int NPR = (int)npr;  // the loops below run over the primes in use

    // Packing (fhe.jl:683-687): G slices of two digit polynomials each are summed exactly before a
    // CRT: |sum| <= G m B Q / 2 (four times that with the randomised flatten) must stay below
    // 0.4 M_rns.
    {
        auto group = [&](double lg) {
            uint32_t G = 0;
            if (lg >= 0) { G = 1; while (G < n && (double)(31 - __builtin_clz(2 * G)) <= lg) G *= 2; }
            return G;
        };
        const double lg = log_have + log2(0.8) - log_mbq - 0.001;
        out->pack_G = group(lg);
        out->pack_G_rnd = group(lg - 2.0);
    }

    // flatten constants (utils.jl:162-169); randomised flatten: v_i in [-xmax, xmax], digits shifted by
    // s + xmax (utils.jl:204-216)
    const u128 s = (B & 1) ? (B - 1) / 2 : B / 2 - 1;
    const u128 xmax = (B & 1) ? (B - 1) / 2 * 3 : B / 2 * 3;
    const u128 off = (((1 + B) % Q) * (s % Q)) % Q;  // (1+B) < 2^63, s < 2^62
    auto digits_of = [&](u128 acc) {
        u128 x = (acc + off) % Q;
        return make_ulonglong2((uint64_t)(x % B), (uint64_t)(x / B));
    };

    CrtConst &cc = out->crt;
    cc.Q = Q;
    cc.B = B;
    cc.offneg = (Q - off) % Q;
    cc.xmax = (uint64_t)xmax;
    cc.offneg_rnd = (Q - (((1 + B) % Q) * ((s + xmax) % Q)) % Q) % Q;
    cc.DQ = DQ_tilde % Q;
    cc.halfQ = Q / 2;
    cc.roundthr = Q / 2 + (Q & 1);
    cc.invQ = 1.0 / u128_dbl(Q);
    cc.invB = 1.0 / u128_dbl(B);
    cc.logr = logm + 1;
    cc.dig0 = digits_of(0);
    cc.digP = digits_of(cc.DQ);
    cc.digN = digits_of((Q - cc.DQ) % Q);
    cc.DQL = DQ_tilde >> 2;   // LUT rows: A0 (DQ_tilde < Q is checked at ctx creation)
    cc.digPL = digits_of(cc.DQL);
    cc.digNL = digits_of((Q - cc.DQL) % Q);
    u128 cM = 1 % Q;
    for (int i = 0; i < NPR; i++) cM = (cM * primes[i]) % Q;  // < 2^94 * 2^29
    for (int i = 0; i < NPR; i++) {
        u128 ci = 1 % Q;
        for (int j = 0; j < NPR; j++)
            if (j != i) ci = (ci * primes[j]) % Q;
        cc.c[i] = ci;
        cc.invp[i] = 1.0f / (float)primes[i];
    }
    const uint32_t plast = primes[NPR - 1];
    const u128 cH = (cc.c[NPR - 1] * ((plast - 1) / 2)) % Q;
    for (int a = 0; a < 6 * NPR + 2; a++) cc.T[a] = (Q - (((u128)a * cM) % Q + cH) % Q) % Q;
    auto limbs = [](u128 v, uint32_t *w, int nw) {
        for (int i = 0; i < nw; i++) w[i] = (uint32_t)(v >> (32 * i));
    };
    for (int i = 0; i < NPR; i++) { limbs(cc.c[i], cc.c32[i], 3); cc.cd[i] = u128_dbl(cc.c[i]); }
    for (int a = 0; a < 6 * NPR + 2; a++) { limbs(cc.T[a], cc.T32[a], 4); cc.Td[a] = u128_dbl(cc.T[a]); }
    limbs(Q, cc.Q32, 3);
    cc.Bd = u128_dbl(B);
    cc.npr = npr;

    {   // k_crt_lean (kernels.h; tests/rns_model.py::CrtLean derives the same values)
        CrtLean &K = out->lean;
        int nq = 0, nb = 0;
        while (nq < 128 && (Q >> nq)) nq++;
        while (nb < 64 && (B >> nb)) nb++;
        int NL = (nq + 28) / 29;
        if (NL < 2) NL = 2;
        const int t = nq - 29, a = 29 * (NL - 1) - t;
        if (nb >= 13 && NL <= 4 && nq >= 30 && a >= 0 && a <= 28) {
            auto lim = [&](u128 v, uint32_t *w) {
                for (int k = 0; k < 4; k++) w[k] = (uint32_t)((v >> (29 * k)) & 0x1FFFFFFFu);
            };
            for (int i = 0; i < NPR; i++) {
                lim(cc.c[i], K.c[i]);
                K.w[i] = (uint32_t)((1ull << 58) / primes[i]);
            }
            lim((Q - cM % Q) % Q, K.cMn);
            K.hoff = (plast - 1) / 2;
            limbs(Q, K.Qw, 3);
            K.B0 = (uint32_t)(B & 0x1FFFFFFFu);
            K.B1 = (uint32_t)(B >> 29);
            K.Bw0 = (uint32_t)B;
            K.Bw1 = (uint32_t)(B >> 32);
            // floor(2^(t + 72) / Q) < 2^44: long division, 2^(t + 72) has up to 138 bits
            {
                u128 rem = 0, quo = 0;
                for (int bit = t + 72; bit >= 0; bit--) {
                    rem = (rem << 1) | (bit == t + 72 ? 1 : 0);
                    quo <<= 1;
                    if (rem >= Q) { rem -= Q; quo |= 1; }
                }
                K.mq0 = (uint32_t)quo;
                K.mq1 = (uint32_t)(quo >> 32);
            }
            {   // floor(2^(nb + 51) / B) <= 2^52
                const u128 quo = ((u128)1 << (nb + 51)) / B;
                K.mb0 = (uint32_t)quo;
                K.mb1 = (uint32_t)(quo >> 32);
            }
            K.a = (uint32_t)a;
            K.t2 = (uint32_t)(nq > 63 ? nq - 63 : 0);
            K.sB = (uint32_t)(nb + 51 - (int)K.t2 - 64);
            K.nl = (uint32_t)NL;
            // randomised flatten: 2 xmax and (-2 xmax (1 + B)) mod Q  (2 xmax (1 + B) < 3.1 B^2 < 2^96)
            const u128 xm2 = (u128)2 * cc.xmax;
            lim((Q - (xm2 * (1 + B)) % Q) % Q, K.cR);
            K.xm2lo = (uint32_t)xm2;
            K.xm2hi = (uint32_t)(xm2 >> 32);
            // k_crt_lean_rnd adds the draws to the old stored digits: its hi operand reaches
            // Q / B + 6 B <= 7 B.  With two limbs (Q < 2^58) the term h1 B1 2^61 of hi B has no limb
            // sum to go to (crt_lean_one drops it), so the kernel is taken only where that term is
            // zero; and 6 B^2 has to stay far below the 2^34 Q of the residue sum for the quotient
            // estimate's width (tests/rns_model.py CrtLean.digits asserts both).  Reference
            // parameter sets have three limbs and B ~ sqrt(Q); others fall back to k_crt_acc.
            out->lean_rnd_ok = (NL >= 3 || ((7 * B) >> 32) == 0 || K.B1 == 0) && B * B <= (Q << 27);
            // crt_lean87_one: five primes, Q of 87 bits, B of 44 bits (Params(1024)); its register
            // widths and quotient estimates hold for every such Q and B
            // (tests/test_crt_lean87_model.py)
            if (NPR == 5 && nq == 87 && nb == 44) {
                const u128 mq = ((u128)1 << 122) / Q, mb = ((u128)1 << 96) / B;
                K.mqw0 = (uint32_t)mq;
                K.mqw1 = (uint32_t)(mq >> 32);
                K.mbw0 = (uint32_t)mb;
                K.mbw1 = (uint32_t)(mb >> 32);
                K.p87 = 1;
            }
        }
    }

    // per-prime constants (all residues centred: |.| <= (p - 1) / 2)
    for (int i = 0; i < NPR; i++) {
        const uint32_t p = primes[i];
        PrimeK &P = out->pk[i];
        P.p = (int32_t)p;
        uint32_t inv = p;  // Newton: p^-1 mod 2^32
        for (int it = 0; it < 5; it++) inv *= 2u - p * inv;
        P.pinv = inv;
        const uint32_t R1 = (uint32_t)((1ull << 32) % p);
        const uint32_t Rinv = powmod32(R1, p - 2, p);
        const uint32_t R2 = mulmod32(R1, R1, p);
        P.r1 = centre32(R1, p);
        P.r2 = centre32(R2, p);
        P.r3 = centre32(mulmod32(R2, R1, p), p);
        P.sR = centre32((p - mulmod32((uint32_t)(s % p), Rinv, p)) % p, p);
        P.sRr = centre32((p - mulmod32((uint32_t)((s + xmax) % p), Rinv, p)) % p, p);
        P.hoff = (i == NPR - 1) ? (p - 1) / 2 : 0;
        P.qmodp = centre32((uint32_t)(Q % p), p);
        uint32_t Mi = 1;  // (M_rns / p_i) mod p_i
        for (int j = 0; j < NPR; j++)
            if (j != i) Mi = mulmod32(Mi, primes[j] % p, p);
        const uint32_t ei = powmod32(Mi, p - 2, p);
        const uint32_t minv = powmod32(M % p, p - 2, p);
        const uint32_t kappa = mulmod32(mulmod32(R2, minv, p), ei, p);
        P.kappaR = centre32(mulmod32(kappa, R1, p), p);
        P.minvR = centre32(mulmod32(minv, R1, p), p);
        P.invp = 1.0f / (float)p;
        P.npr = npr;
    }
}

// ---------------------------------------------------------------- one prime's tables

// The twiddle tables of a prime (all residues centred, Montgomery form), as they lie on the device.
struct PrimeTables {
    // four tables of m entries [f | v | fp | vp]: forward twiddles, inverse twiddles, and the product twiddles
    // of the radix-4 steps of each (ntt.h fwd_step4): twp[j] = +-tw[j >> 1] tw[j], minus for odd j
    std::vector<int32_t> tw;
    // quarter form of the latency kernels: four blocks [f_q | v_q | fp_q | vp_q] of m / 4 words (empty below m = 16)
    std::vector<int32_t> twq;
    std::vector<int32_t> pw;    // psi^e R mod p, e in [0, 2 m)
    int32_t head[8];            // f[1..3], fp[2], fp[3], v[1..3] (PrimeK::f1 ... v3)
};

inline Refusal prime_tables(uint32_t p, int logm, PrimeTables *out) {
    const uint32_t M = 1u << logm;
    uint32_t psi = 0;
    for (uint32_t x = 2; x < 2000 && !psi; x++) {
        uint32_t g = powmod32(x, (p - 1) / (2 * M), p);
        if (powmod32(g, M, p) == p - 1) psi = g;
    }
    if (!psi) return {SGFHE_ERR_UNSUPPORTED, "no primitive 2m-th root of unity"};
    const uint32_t ipsi = powmod32(psi, p - 2, p);
    out->tw.assign((size_t)4 * M, 0);
    int32_t *f = out->tw.data(), *v = f + M, *fp = f + 2 * M, *vp = f + 3 * M;
    const uint32_t R1m = (uint32_t)((1ull << 32) % p);
    std::vector<uint32_t> pf(M), pv(M);   // plain values in table order
    uint32_t pw = 1, ipw = 1;
    for (uint32_t t = 0; t < M; t++) {
        const uint32_t br = bitrev(t, logm);
        pf[br] = pw;
        pv[br] = ipw;
        f[br] = centre32(mulmod32(pw, R1m, p), p);   // Montgomery form
        v[br] = centre32(mulmod32(ipw, R1m, p), p);
        pw = mulmod32(pw, psi, p);
        ipw = mulmod32(ipw, ipsi, p);
    }
    fp[0] = fp[1] = vp[0] = vp[1] = 0;
    for (uint32_t j = 2; j < M; j++) {
        const uint32_t a = mulmod32(mulmod32(pf[j >> 1], pf[j], p), R1m, p);
        const uint32_t b = mulmod32(mulmod32(pv[j >> 1], pv[j], p), R1m, p);
        fp[j] = centre32((j & 1) ? (p - a) % p : a, p);
        vp[j] = centre32((j & 1) ? (p - b) % p : b, p);
    }
    // quarter form of the latency kernels: after the first two Cooley-Tukey stages quarter q of the
    // array runs on the sub-tree of the twiddle table rooted at entry 4 + q, so its tables are a
    // re-indexing of the big ones: entry mm' + i' (mm' a power of two, i' < mm') = big entry
    // 4 mm' + q mm' + i'; the same for the inverse and for both product tables
    out->twq.clear();
    if (M >= 16) {
        const uint32_t MS = M / 4;
        out->twq.assign((size_t)4 * M, 0);
        for (uint32_t q = 0; q < 4; q++)
            for (uint32_t jj = 1; jj < MS; jj++) {
                const uint32_t mmq = 1u << (31 - __builtin_clz(jj)), J = 4 * mmq + q * mmq + (jj - mmq);
                int32_t *blk = out->twq.data() + (size_t)q * M;
                blk[jj] = f[J];
                blk[MS + jj] = v[J];
                blk[2 * MS + jj] = jj >= 2 ? fp[J] : 0;
                blk[3 * MS + jj] = jj >= 2 ? vp[J] : 0;
            }
    }
    {   // psi^e R mod p, centred
        out->pw.resize((size_t)2 * M);
        uint32_t pe = 1;
        for (uint32_t e = 0; e < 2 * M; e++) { out->pw[e] = centre32(mulmod32(pe, R1m, p), p); pe = mulmod32(pe, psi, p); }
    }
    const int32_t head[8] = {f[1], M > 2 ? f[2] : 0, M > 2 ? f[3] : 0, M > 2 ? fp[2] : 0, M > 2 ? fp[3] : 0,
                             v[1], M > 2 ? v[2] : 0, M > 2 ? v[3] : 0};
    memcpy(out->head, head, sizeof head);
    return {};
}

// ---------------------------------------------------------------- key_derive, RNS2

// The key of a ctx's smaller basis from the key of its larger one (kernels.h k_key_derive): per prime of the smaller
// basis the product of the larger one's extra primes, in Montgomery form, centred.
inline KeyFactors key_factors(const uint32_t *primes, uint32_t nps, uint32_t npb) {
    KeyFactors fac = {};
    for (uint32_t i = 0; i < nps; i++) {
        const uint32_t p = primes[i];
        uint32_t f = (uint32_t)((1ull << 32) % p);                   // R: Montgomery form
        for (uint32_t j = nps; j < npb; j++) f = mulmod32(f, primes[j] % p, p);
        fac.f[i] = centre32(f, p);
    }
    return fac;
}

// CRT of rns.jl:32-40: c1 = m2^(m1-1) mod Q = m2 (m2^-1 mod m1), c2 = m1 (m1^-1 mod m2)
// (Fermat idempotents, m1 and m2 prime)
inline Refusal rns2_const(u128 Q, uint64_t m1, uint64_t m2, Rns2Const *out) {
    if ((u128)m1 * m2 != Q) return {SGFHE_ERR_INVALID_ARG, "m1 * m2 != Q"};
    if (m1 >= (1ull << 47) || m2 >= (1ull << 47) || m1 < 2 || m2 < 2)
        return {SGFHE_ERR_UNSUPPORTED, "RNS2 limb moduli must be in [2, 2^47)"};
    auto powmod64 = [](uint64_t a, uint64_t e, uint64_t md) {
        u128 r = 1, b = a % md;
        while (e) { if (e & 1) r = r * b % md; b = b * b % md; e >>= 1; }
        return (uint64_t)r;
    };
    Rns2Const rc;
    rc.m1 = m1;
    rc.m2 = m2;
    rc.i21 = powmod64(m2 % m1, m1 - 2, m1);
    rc.i12 = powmod64(m1 % m2, m2 - 2, m2);
    if ((u128)(m2 % m1) * rc.i21 % m1 != 1 || (u128)(m1 % m2) * rc.i12 % m2 != 1)
        return {SGFHE_ERR_INVALID_ARG, "RNS2 limb moduli must be distinct primes"};
    rc.inv1 = 1.0 / (double)m1;
    rc.inv2 = 1.0 / (double)m2;
    *out = rc;
    return {};
}

}  // namespace sgfhe
