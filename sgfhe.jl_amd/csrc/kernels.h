// HIP kernels of the gate-bootstrap engine (gfx950).  Hot path of nucypher/SGFHE.jl:
// _bootstrap_internal / external_product / flatten / reduce_modulus
// (/root/reference/src/fhe.jl:519-621, src/utils.jl:78-189), restructured as in DESIGN.md:
//
//   acc <- acc + (x^j - 1) * sum_row u_row (*) C_k[row]          (CMux form of fhe.jl:580-581)
//
// State per bootstrap: the *flattened* accumulators, i.e. for every coefficient of (a, b) the
// two base-B digits (lo, hi) of x' = (acc + off) mod Q with off = (1 + B) s (utils.jl:162-181).
// Per iteration k two kernels run over a chunk of bootstraps in lock-step:
//   k_extprod  one workgroup per (bootstrap, RNS prime): digits -> 4 forward NTTs -> 8 pointwise
//              multiply-accumulates against the NTT-domain key slice -> 2 inverse NTTs ->
//              negacyclic rotate-and-subtract (x^j - 1) -> residues y mod p_i
//   k_crt_acc  per coefficient: CRT of the residues to the exact integer, reduce mod Q, add to
//              the accumulator, flatten again (divide by B).
#pragma once

#include "ntt.h"
#include "constants.h"

namespace sgfhe {

constexpr int LOGE = 4;  // points per thread (2^LOGE) in every NTT of the engine

__device__ __forceinline__ Mod mod_of(const PrimeK &P) { return Mod{P.p, -P.p, P.pinv}; }

// The npr PrimeK records live in device memory and are indexed by the (wave-uniform) prime
// index of the workgroup.
typedef const PrimeK *__restrict__ PrimeSet;

// A call's optional per-row LUT descriptor (bootstrap_device): one word per row of the call, LUT_ROW | truth table for
// a LUT row, 0 for a row of the classic path.
constexpr uint32_t LUT_ROW = 0x100u;

enum : uint32_t {
    MODE_PLAIN = 1u,  // k_extprod: no (x^j - 1) factor (external_product debug hook)
    MODE_NOACC = 2u,  // k_crt_acc: do not add the previous accumulator
    MODE_CANON = 4u,  // k_crt_acc: write canonical residues instead of digits
    MODE_RANDOM = 16u,// randomised flatten (rng != nothing, utils.jl:198-241): digits e_i hold
                      // u_i + s + xmax, u_i in (-2B, 2B]
    MODE_WIDE = 32u   // with MODE_RANDOM and B >= 2^46: stored digits reach 4 B >= 2^48, bits 48..55
                      // live in the record's third plane (Params(2048): B = 35 * 2^41)
};

// ---- small 128-bit helpers -----------------------------------------------------------------

__device__ __forceinline__ double u128_to_double(u128 x) {
    return (double)(uint64_t)(x >> 64) * 18446744073709551616.0 + (double)(uint64_t)x;
}
__device__ __forceinline__ u128 mul_u64_u128(uint64_t a, u128 b) {
    // a * b mod 2^128
    return (u128)a * (uint64_t)b + (((u128)(a * (uint64_t)(b >> 64))) << 64);
}
// x mod d for x < 2^127, d < 2^94, quotient < 2^62; inv = 1.0 / d.
__device__ __forceinline__ u128 mod_wide(u128 x, u128 d, double inv, uint64_t *quot) {
    uint64_t q = (uint64_t)(u128_to_double(x) * inv);
    u128 r = x - mul_u64_u128(q, d);
#pragma unroll 1
    while ((__int128)r < 0) { r += d; q--; }
#pragma unroll 1
    while (r >= d) { r -= d; q++; }
    if (quot) *quot = q;
    return r;
}

// ---- digit planes ---------------------------------------------------------------------------------
// Per (bootstrap, c) a record of 16 m bytes (the size of the canonical residues it replaces):
//   [lo words: digit 0 | digit 1] 2 m x uint32      bits 0..31 of the digits
//   [hi words: digit 0 | digit 1] 2 m x uint16      bits 32..47          (12 m bytes in use)
//   [top bytes: digit 0 | digit 1] 2 m x uint8      bits 48..55, MODE_WIDE only (14 m bytes in use)
// digit 0 = lo, digit 1 = hi of x' for acc_a (c = 0) and acc_b (c = 1); every stored digit is
// below 2^48 (B < 2^46 is checked at ctx creation; the randomised mode stores up to 4 B).  Plane
// p = 2 c + digit is the p-th row of u = [a_lo, a_hi, b_lo, b_hi] (fhe.jl:524-526) and multiplies
// key row p.  6 bytes per digit instead of 8: the CRT kernel is bound by these bytes.
// Byte offsets inside a chunk's buffers fit 32 bits (chunk <= 8192, buffers below 4 GB): a uniform
// base plus a 32-bit byte offset takes the SGPR-base addressing mode, with no 64-bit address
// arithmetic on the vector ALU.
template <class T>
__device__ __forceinline__ T ld_off(const void *base, uint32_t byte_off) {
    return *reinterpret_cast<const T *>(reinterpret_cast<const char *>(base) + byte_off);
}
template <class T>
__device__ __forceinline__ void st_off(void *base, uint32_t byte_off, T v) {
    *reinterpret_cast<T *>(reinterpret_cast<char *>(base) + byte_off) = v;
}
// Buffer-descriptor addressing (MI355X guide, T8 / T20): the 128-bit resource lives in SGPRs, a
// load or store takes a 32-bit per-lane byte offset (VGPR), a wave-uniform byte offset (SGPR,
// formed on the scalar ALU) and a 12-bit immediate -- no 64-bit address arithmetic on the vector
// ALU, which is what bounds k_extprod.  Everything that builds a descriptor or an soffset must be
// provably wave-uniform (kernel arguments, blockIdx, loop counters), or hipcc wraps the access in
// a waterfall loop.  Accesses beyond `bytes` read 0 / are dropped by the hardware range check.
typedef __amdgpu_buffer_rsrc_t BufRsrc;
__device__ __forceinline__ BufRsrc make_rsrc(const void *base, uint32_t bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(base), (short)0, (int)bytes, 0x00020000);
}
__device__ __forceinline__ uint32_t buf_ld_u32(BufRsrc r, uint32_t voff, uint32_t soff) {
    return (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(r, (int)voff, (int)soff, 0);
}
__device__ __forceinline__ uint32_t buf_ld_u16(BufRsrc r, uint32_t voff, uint32_t soff) {
    return (uint16_t)__builtin_amdgcn_raw_buffer_load_b16(r, (int)voff, (int)soff, 0);
}
__device__ __forceinline__ uint32_t buf_ld_u8(BufRsrc r, uint32_t voff, uint32_t soff) {
    return (uint8_t)__builtin_amdgcn_raw_buffer_load_b8(r, (int)voff, (int)soff, 0);
}
__device__ __forceinline__ int4 buf_ld_i4(BufRsrc r, uint32_t voff, uint32_t soff) {
    typedef unsigned int v4u __attribute__((ext_vector_type(4)));
    const v4u v = __builtin_amdgcn_raw_buffer_load_b128(r, (int)voff, (int)soff, 0);
    return make_int4((int)v.x, (int)v.y, (int)v.z, (int)v.w);
}
// Cache policy of the residue stores (aux bits: 1 = sc0, 2 = nt, 16 = sc1), measured in the
// pipeline (profiles/r02_exp_plain_vs_nt_stores_final.txt, r02_exp_store_policy.txt): non-temporal
// 1863, plain 1893 (the Infinity Cache keeps up to 256 MB of written data for the next kernel's
// reads, and a non-temporal store writes more slowly: tools/ubench_mall.hip, 4.0 against
// 5.9 TB/s); on another box plain 1922, sc0 1924, sc1 1936, sc0 sc1 1935, sc0 nt 1903.  sc1
// (write-through) it is.
constexpr int YRES_AUX = 16;
__device__ __forceinline__ void buf_st_u32(BufRsrc r, uint32_t voff, uint32_t soff, uint32_t v) {
    __builtin_amdgcn_raw_buffer_store_b32(v, r, (int)voff, (int)soff, YRES_AUX);
}

__device__ __forceinline__ const uint32_t *digit_lo_plane(const uint64_t *dig, size_t bc, uint32_t M) {
    return reinterpret_cast<const uint32_t *>(dig + bc * 2 * M);
}
__device__ __forceinline__ const uint16_t *digit_hi_plane(const uint64_t *dig, size_t bc, uint32_t M) {
    return reinterpret_cast<const uint16_t *>(dig + bc * 2 * M + M);
}
__device__ __forceinline__ ulonglong2 load_digits(const uint64_t *__restrict__ dig, size_t bc,
                                                  uint32_t i, uint32_t M, bool wide = false) {
    const uint32_t rec = (uint32_t)bc * 16u * M;           // byte offset of the record
    const uint32_t lo = rec + 4u * i, hi = rec + 8u * M + 2u * i;
    ulonglong2 d = make_ulonglong2(
        ld_off<uint32_t>(dig, lo) | ((uint64_t)ld_off<uint16_t>(dig, hi) << 32),
        ld_off<uint32_t>(dig, lo + 4u * M) | ((uint64_t)ld_off<uint16_t>(dig, hi + 2u * M) << 32));
    if (wide) {
        const uint32_t top = rec + 12u * M + i;
        d.x |= (uint64_t)ld_off<uint8_t>(dig, top) << 48;
        d.y |= (uint64_t)ld_off<uint8_t>(dig, top + M) << 48;
    }
    return d;
}
__device__ __forceinline__ void store_digits(uint64_t *__restrict__ dig, size_t bc, uint32_t i,
                                             uint32_t M, uint64_t lo, uint64_t hi, bool wide = false) {
    const uint32_t rec = (uint32_t)bc * 16u * M;
    const uint32_t ol = rec + 4u * i, oh = rec + 8u * M + 2u * i;
    st_off<uint32_t>(dig, ol, (uint32_t)lo);
    st_off<uint32_t>(dig, ol + 4u * M, (uint32_t)hi);
    st_off<uint16_t>(dig, oh, (uint16_t)(lo >> 32));
    st_off<uint16_t>(dig, oh + 2u * M, (uint16_t)(hi >> 32));
    if (wide) {
        const uint32_t top = rec + 12u * M + i;
        st_off<uint8_t>(dig, top, (uint8_t)(lo >> 48));
        st_off<uint8_t>(dig, top + M, (uint8_t)(hi >> 48));
    }
}

// ---- randomised flatten (utils.jl:198-241) ----------------------------------------------------------
// The draws come from a ChaCha counter stream (the RFC 8439 block function with RND_ROUNDS = 8
// rounds: "ChaCha8") keyed with the caller's 32 bytes, so the digit perturbations are
// cryptographically strong when the key is.  (Rounds 1-3 used Philox4x32-10 keyed by 64 bits: a
// statistical generator.)  Functional parity only: the reference draws from the caller's Julia
// rng, whose stream cannot be reproduced here.
// The draw for a digit pair is addressed by a counter that does not depend on how a batch is cut
// into chunks or scheduled: the 128 bits of coefficient x are words 4 (x mod 4) .. + 3 of the block
// whose state words 12 .. 15 are
//   (x div 4   with x = coefficient index (c << log2 m) + i of the accumulator pair (c = 0: a, 1: b),
//    y: 0 for the initial accumulators, k + 1 after k-loop iteration k
//       (pack_encrypted_bits' flatten of as_i: 2^31 | i),
//    z: index of the bootstrap within the call (of the ciphertext, for packing),
//    w: number of the call since sgfhe_set_random_flatten),
// so a thread of k_crt_lean_rnd (four adjacent coefficients) computes exactly one block.
// oracle/bigint_oracle.py restates the same stream, so the randomised mode is bit-comparable with
// the oracle.
// The round count fixes the stream, and with it every randomised result (and the oracle's restatement).
constexpr int RND_ROUNDS = 8;
struct ChaChaKey {
    uint32_t k[8];
};
// ChaCha block function (RFC 8439 section 2.3 with ROUNDS rounds): state words 12 .. 15 = c12 .. c15
template <int ROUNDS>
__device__ __forceinline__ void chacha_block(const ChaChaKey &key, uint32_t c12, uint32_t c13,
                                             uint32_t c14, uint32_t c15, uint32_t (&out)[16]) {
    static_assert(ROUNDS % 2 == 0, "double rounds");
    const uint32_t s[16] = {0x61707865u, 0x3320646eu, 0x79622d32u, 0x6b206574u,
                            key.k[0], key.k[1], key.k[2], key.k[3],
                            key.k[4], key.k[5], key.k[6], key.k[7], c12, c13, c14, c15};
    uint32_t x[16];
#pragma unroll
    for (int i = 0; i < 16; i++) x[i] = s[i];
#define SGFHE_QR(a, b, c, d)                                                             \
    x[a] += x[b]; x[d] = __builtin_rotateleft32(x[d] ^ x[a], 16);                        \
    x[c] += x[d]; x[b] = __builtin_rotateleft32(x[b] ^ x[c], 12);                        \
    x[a] += x[b]; x[d] = __builtin_rotateleft32(x[d] ^ x[a], 8);                         \
    x[c] += x[d]; x[b] = __builtin_rotateleft32(x[b] ^ x[c], 7);
#pragma unroll
    for (int r = 0; r < ROUNDS / 2; r++) {
        SGFHE_QR(0, 4, 8, 12) SGFHE_QR(1, 5, 9, 13) SGFHE_QR(2, 6, 10, 14) SGFHE_QR(3, 7, 11, 15)
        SGFHE_QR(0, 5, 10, 15) SGFHE_QR(1, 6, 11, 12) SGFHE_QR(2, 7, 8, 13) SGFHE_QR(3, 4, 9, 14)
    }
#undef SGFHE_QR
#pragma unroll
    for (int i = 0; i < 16; i++) out[i] = x[i] + s[i];
}
// A call gathered from several callers (engine.hip Coalescer, round 5): every row of the batch draws from the
// stream of the ctx it came in on -- that ctx's key, call number and the row's index in ITS call -- so that each
// caller gets the bytes its call gives alone.  One record per row of the combined call, in device memory.
struct RndRow {
    ChaChaKey key;
    uint32_t call, boot;
};
struct RndArgs {
    ChaChaKey key;         // 32-byte key of the draw stream
    uint32_t call, chunk;  // per-call counter, index of the chunk's first bootstrap in the call
    const RndRow *rows;    // gathered call: the stream of every row of the call (kernels instantiated with ROWS); else null
};
// The stream of bootstrap `row` of the chunk: key, its index in its call (counter word z), its call number (w).
// ROWS = false leaves the key in the kernel arguments (scalar registers), as before the table existed.
template <bool ROWS>
__device__ __forceinline__ void rnd_stream(const RndArgs &ra, uint32_t row, ChaChaKey &key, uint32_t &cz, uint32_t &cw) {
    if constexpr (ROWS) {
        const RndRow r = ra.rows[ra.chunk + row];
        key = r.key; cz = r.boot; cw = r.call;
    } else {
        key = ra.key; cz = ra.chunk + row; cw = ra.call;
    }
}
// the 128 bits of one coefficient (ctr.x = its index): a quarter of its quad's block
__device__ __forceinline__ uint4 rnd128(const ChaChaKey &key, uint4 ctr) {
    uint32_t w[16];
    chacha_block<RND_ROUNDS>(key, ctr.x >> 2, ctr.y, ctr.z, ctr.w, w);
    const uint32_t q = ctr.x & 3u;
    return make_uint4(q == 0 ? w[0] : q == 1 ? w[4] : q == 2 ? w[8] : w[12],
                      q == 0 ? w[1] : q == 1 ? w[5] : q == 2 ? w[9] : w[13],
                      q == 0 ? w[2] : q == 1 ? w[6] : q == 2 ? w[10] : w[14],
                      q == 0 ? w[3] : q == 1 ? w[7] : q == 2 ? w[11] : w[15]);
}
// Digits of the randomised flatten of acc, given xn = (acc + (s + xmax)(1 + B)) mod Q:
//   r_i = v_i + xmax uniform in [0, 2 xmax];  x2 = (xn - r_0 - r_1 B) mod Q = a' of utils.jl:179
//   for the shifted value;  (lo, hi) = divmod(x2, B);  e_i = (lo, hi) + r_i  ( = u_i + s + xmax ).
__device__ __forceinline__ ulonglong2 random_digits(u128 xn, const CrtConst *CC, const ChaChaKey &key,
                                                    uint4 ctr) {
    const uint4 rv = rnd128(key, ctr);
    const uint64_t span = 2 * CC->xmax + 1;
    const uint64_t r0 = (uint64_t)(((u128)(((uint64_t)rv.y << 32) | rv.x) * span) >> 64);
    const uint64_t r1 = (uint64_t)(((u128)(((uint64_t)rv.w << 32) | rv.z) * span) >> 64);
    const u128 B = CC->B, Q = CC->Q;
    const u128 tsub = mod_wide((u128)r1 * (uint64_t)B + r0, Q, CC->invQ, nullptr);
    const u128 x2 = xn >= tsub ? xn - tsub : xn + Q - tsub;
    uint64_t hi;
    const u128 lo = mod_wide(x2, B, CC->invB, &hi);
    return make_ulonglong2((uint64_t)lo + r0, hi + r1);
}

// ---- digit -> residue ------------------------------------------------------------------------
// (e - s) * R^-1 mod p for a stored digit e < 2^48: |REDC(e)| <= 2^16 + p / 2, plus the centred
// constant -(s R^-1): |result| <= p + 2^16.
__device__ __forceinline__ int32_t digit_reduce(uint64_t e, const Mod &md, int32_t sR) {
    return sredc((int64_t)e, md) + sR;
}

// ---- steps the product kernels share ---------------------------------------------------------------
// (tests/rns_model.py restates each of them once, too)
// Offset of the residues handed to the CRT kernels.  |+-v - z| < 2.7 p: + 3 p makes a non-negative
// representative below 5.7 p (no reduction at all: the CRT kernels take any such residues); + (p - 1) / 2
// for the last prime, folded into the same wave-uniform constant.
__device__ __forceinline__ uint32_t handover_offset(const PrimeK &P) { return 3u * (uint32_t)P.p + P.hoff; }

// Products of one transformed key row (E points per thread, slot order) with the row's two key polynomials,
// kp and kp + M: two int4 key loads, two smont per point, two int4 stores per group of four  -> zpart
template <int M, int E>
__device__ __forceinline__ void key_row_products(const int32_t (&x)[1][E], const int32_t *kp, int32_t *zp,
                                                 const Mod &md) {
#pragma unroll
    for (int h = 0; h < E / 4; h++) {
        const int4 a = reinterpret_cast<const int4 *>(kp)[h];
        const int4 bq = reinterpret_cast<const int4 *>(kp + M)[h];
        const int32_t ka[4] = {a.x, a.y, a.z, a.w};
        const int32_t kb[4] = {bq.x, bq.y, bq.z, bq.w};
        int32_t r0[4], r1[4];
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const int32_t u = x[0][4 * h + t];
            r0[t] = smont(u, ka[t], md);  // |.| < 0.74 * 2^29
            r1[t] = smont(u, kb[t], md);
        }
        reinterpret_cast<int4 *>(zp)[h] = make_int4(r0[0], r0[1], r0[2], r0[3]);
        reinterpret_cast<int4 *>(zp + M)[h] = make_int4(r1[0], r1[1], r1[2], r1[3]);
    }
}
// Sum over the four key rows of group h (four slots) of the partial products in zpart: < 2.99 * 2^29
template <int M>
__device__ __forceinline__ void zpart_sum4(const int32_t *zp, int h, int32_t (&acc)[4]) {
    acc[0] = acc[1] = acc[2] = acc[3] = 0;
#pragma unroll
    for (int ph = 0; ph < 4; ph++) {
        const int4 v = reinterpret_cast<const int4 *>(zp + (size_t)ph * 2 * M)[h];
        acc[0] += v.x; acc[1] += v.y; acc[2] += v.z; acc[3] += v.w;
    }
}

// Radix-4 head of a quarter transform: quarter q of the first two Cooley-Tukey stages.  With X0..X3 the
// coefficients i, i + m/4, i + m/2, i + 3m/4 of a digit plane (dl, dh: its low and high words),
//   u = f1 X2;  q < 2: (X0 + u) +- (f2 X1 + fp2 X3);  q >= 2: (X0 - u) +- (f3 X1 + fp3 X3)
// (the arithmetic of ntt.h fwd_step4), reduced to [0, p].
struct QuarterHead {
    uint32_t q;
    int32_t wB, wP;
    __device__ __forceinline__ QuarterHead(uint32_t q_, const PrimeK &P)
        : q(q_), wB((q_ & 2) ? P.f3 : P.f2), wP((q_ & 2) ? P.fp3 : P.fp2) {}
    template <int MS>
    __device__ __forceinline__ int32_t point(const uint32_t *dl, const uint16_t *dh, uint32_t i, const PrimeK &P,
                                             const Mod &md, int32_t sRd) const {
        int32_t X[4];
#pragma unroll
        for (int t = 0; t < 4; t++)
            X[t] = digit_reduce(dl[i + t * MS] | ((uint64_t)dh[i + t * MS] << 32), md, sRd);   // |.| <= p + 2^16
        const int32_t u = smont(X[2], P.f1, md);                                              // < 0.57 * 2^29
        const int32_t a = (q & 2) ? X[0] - u : X[0] + u;
        const int32_t w = sredc((int64_t)X[1] * wB + (int64_t)X[3] * wP, md);                   // < 0.63 * 2^29
        return sred_floor((q & 1) ? a - w : a + w, md);                                       // [0, p]
    }
};

// Rotation factors of the E slots s = q m/4 + E t + e of thread t of quarter q: slot s holds the value at
// psi^(2 brv(s) + 1), so (x^j - 1) is psi^(j (2 brv(s) + 1) mod 2m) - 1 there.  A gather from the table of
// psi powers: the callers request it first.
template <int LOGM, int E>
__device__ __forceinline__ void rot_factors(int32_t (&dfac)[E], const PrimeK &P, uint32_t j, uint32_t q, int t) {
    constexpr uint32_t M = 1u << LOGM;
#pragma unroll
    for (int e = 0; e < E; e++) {
        const uint32_t sl = q * (M / 4) + (uint32_t)(E * t + e);
        const uint32_t br = __brev(sl) >> (32 - LOGM);
        dfac[e] = P.pw[(j * (2u * br + 1u)) & (2u * M - 1u)];
    }
}
// (psi^e - 1) R mod p from two centred residues: in (-p, p), centred again for the product's bound
__device__ __forceinline__ int32_t rot_centre(int32_t dfac, const PrimeK &P, const Mod &md) {
    return scentre(dfac - P.r1, md);
}

// The last two Gentleman-Sande stages of the quarter form, for coefficient i of (bootstrap, c) = bc, on the
// four partial values Y_0..Y_3 at i mod m/4 of every prime --
//   C0 = Y0 + Y1, C1 = v2 (Y0 - Y1), C2 = Y2 + Y3, C3 = v3 (Y2 - Y3);
//   coefficient in quarter 0: C0 + C2;  1: C1 + C3;  2: v1 (C0 - C2);  3: v1 (C1 - C3)
// (only the one this coefficient needs; the quarter is the same for a whole workgroup) -- then the residue in
// the form k_extprod hands over: non-negative, below 4.6 p.
template <int NP>
__device__ __forceinline__ void quarter_residues(const int32_t *__restrict__ ypart, PrimeSet PS, uint32_t bc,
                                                 uint32_t i, uint32_t logm, uint32_t (&y)[NP]) {
    const uint32_t MS = (1u << logm) >> 2, jq = i & (MS - 1), qq = i >> (logm - 2);
#pragma unroll
    for (int q = 0; q < NP; q++) {
        const PrimeK P = PS[q];
        const Mod md = mod_of(P);
        const int32_t *yp = ypart + (((size_t)bc * NP + q) * 4) * MS + jq;
        int32_t r;
        if (qq & 1u) {          // C1, C3
            const int32_t c1 = smont(yp[0] - yp[MS], P.v2, md), c3 = smont(yp[2 * MS] - yp[3 * MS], P.v3, md);
            r = (qq & 2u) ? smont(c1 - c3, P.v1, md) : c1 + c3;             // < 0.75 / < 1.5 * 2^29
        } else {                // C0, C2
            const int32_t c0 = sred(yp[0] + yp[MS], md), c2 = sred(yp[2 * MS] + yp[3 * MS], md);   // sums < 2.8: reduced to 0.51
            r = (qq & 2u) ? smont(c0 - c2, P.v1, md) : c0 + c2;             // < 0.75 / < 1.03 * 2^29
        }
        y[q] = (uint32_t)r + handover_offset(P);
    }
}

// ---- k_extprod ----------------------------------------------------------------------------------
// grid = chunk * NPR workgroups of T = m / 16 threads; chunk is a multiple of 8.  Workgroups are
// dealt round-robin to the 8 XCDs (blocks g and g + 8 share an XCD, MI355X_MICROARCH.md), so
// the NPR prime-workgroups of one bootstrap are given the same g mod 8: they re-read the same
// digits and hit in that XCD's L2.  At m = 8192 a workgroup is 512 threads, at most 128 VGPRs and
// 64 KiB of LDS (32 KiB NTT exchange buffer + 32 KiB thread-private accumulator of the second
// product polynomial): two workgroups share a CU, so one computes butterflies while the other
// sits in an LDS exchange, a barrier or a load.
//   dig    [chunk][2][2][m]     digit planes (see above)
//   keyk   [NPR][4][2][m]       NTT-domain key slice of iteration k (slot order, scaled by kappa,
//                               centred residues as int32)
//   yres   [chunk][2][NPR][m]   output residues y_i = (M/p_i)^-1 * D mod p_i (+ hoff): non-negative
//                               representatives below 5.7 p_i (6.2 p_i for the last prime)
//   ua     [chunk][n]           j = u.a[k] of every bootstrap (fhe.jl:566,580)
// The four digit polynomials u = [a_lo, a_hi, b_lo, b_hi] (fhe.jl:524-526) go through the forward
// NTT one at a time (phase = key row); the two product polynomials through the inverse NTT one at
// a time.  The running NTT-domain sum z_0 lives in registers, z_1 in LDS.
constexpr int EXT_WAVES = 4;  // waves per SIMD of __launch_bounds__ where a workgroup has 4 or more waves
// Digit loads of a phase in groups (round 5, profiles/r05_exp_wide.txt).  The WIDE instantiations have three loads
// per digit -- 48 values in flight beside the 32 accumulator registers -- and hipcc spilled five accumulator pairs
// around the phase loop (44-52 bytes of scratch per lane, rounds 3-4): Params(2048) with the randomised flatten ran
// at 297 bootstraps/s with the spills and runs at 345 without them (+16 %, same call).  The digits of a phase are
// requested in SPLIT groups, each reduced before the next is requested (a scheduling barrier between the groups
// bounds the values in flight): 2 groups remove the scratch at m = 8192 / 16384, 4 at m = 4096 too; a 32-bit
// column-0 accumulator instead (106-125 VGPRs, no scratch either) measured 339.
constexpr int wide_split(int logm) { return logm >= 13 ? 2 : 4; }
// The two-plane (deterministic) kernels are not split: 2 groups would give k_extprod<13, 4, false> 12 bytes of
// scratch, and leave the radix-4 steps at m = 4096 / 16384 spilling 8-32 bytes (RESULTS.md, round 5).
constexpr int DET_SPLIT = 0;
// LE: points per thread (2^LE); 16 wherever that leaves a full wavefront, 8 for m <= 512 (8 measured
// slower at m = 4096 and 8192 too: profiles/r02_exp_p512_points.txt, r04_exp_mid_le3.txt)
constexpr int EXT_LE3_MAX = 9;   // largest log2(m) with 8 points per thread
// WIDE: the digit planes carry a third plane (bits 48..55; MODE_WIDE): a separate instantiation, so
// that the deterministic kernel is textually what it was.
template <int LOGM, int LE, bool WIDE = false>
__global__ void __launch_bounds__((NttGeom<LOGM, LE>::T), (NttGeom<LOGM, LE>::T >= 256 ? EXT_WAVES : 1))
k_extprod(const uint64_t *__restrict__ dig, const int32_t *__restrict__ keyk,
          uint32_t *__restrict__ yres, const uint32_t *__restrict__ ua, PrimeSet PS, uint32_t k,
          uint32_t n, uint32_t mode) {
    using G = NttGeom<LOGM, LE>;
    constexpr int M = G::M, T = G::T, E = G::E;
    SGFHE_DYN_LDS(uint32_t, lds);
    int32_t *const z1 = reinterpret_cast<int32_t *>(lds) + M + threadIdx.x;  // z1[e * T]: private to the thread, conflict-free

    const int tid = threadIdx.x;
    const uint32_t g = blockIdx.x;
    const uint32_t slot = g >> 3;
    const uint32_t npr = PS[0].npr;
    const uint32_t b = (slot / npr) * 8 + (g & 7);
    const uint32_t pi = slot % npr;
    const PrimeK P = PS[pi];
    const Mod md = mod_of(P);
    // Buffer descriptors over this launch's digit planes, key slice and residues (all below 4 GiB:
    // checked when the chunk size is set).  Built from kernel arguments and gridDim only.
    const uint32_t cpad = gridDim.x / npr;  // bootstraps of the (padded) chunk
    const BufRsrc rdig = make_rsrc(dig, cpad * 32u * (uint32_t)M);
    const BufRsrc rkey = make_rsrc(keyk, npr * 32u * (uint32_t)M);
#ifdef SGFHE_ABL_NO_YRES  // timing-only build: zero records, the range check drops every residue store
    const BufRsrc ryres = make_rsrc(yres, 0u);
#else
    const BufRsrc ryres = make_rsrc(yres, cpad * npr * 8u * (uint32_t)M);
#endif

    const int32_t sRd = (mode & MODE_RANDOM) ? P.sRr : P.sR;  // digit offset of the flatten mode
    constexpr int SPLIT = E == 16 ? (WIDE ? wide_split(LOGM) : DET_SPLIT) : 0;
    // the 64-bit NTT-domain sum of column 0 over the four phases (|.| < 1.98 * 2^60)
    int64_t acc0[E];
#pragma unroll
    for (int e = 0; e < E; e++) { acc0[e] = 0; z1[e * T] = 0; }
    // A real loop (not unrolled): one copy of the forward NTT in the instruction stream, and the
    // loads of a later phase cannot be hoisted over the registers of an earlier one.
#pragma unroll 1
    for (int ph = 0; ph < 4; ph++) {
        // The thread index is made opaque per iteration: otherwise the ~60 loop-invariant LDS /
        // twiddle addresses derived from it are hoisted out of the loop and spilled.
        const int tid = (int)threadIdx.x + (int)opaque_zero();
        // 1. digits -> residues (flatten_poly, utils.jl:253-264, lifted to signed integers)
        int32_t x[1][E];
        // Buffer loads: the lane supplies one 32-bit offset per plane (4 tid / 2 tid); record,
        // plane and coefficient stride go into the scalar offset (SALU) -- no vector instruction
        // is spent on addresses (the flat form cost 23 per phase).
        const uint32_t srec = (b * 2u + (uint32_t)(ph >> 1)) * 16u * (uint32_t)M;  // byte offset of the record
        const uint32_t slo = srec + (uint32_t)(ph & 1) * 4u * (uint32_t)M;
        const uint32_t shi = srec + 8u * (uint32_t)M + (uint32_t)(ph & 1) * 2u * (uint32_t)M;
        const uint32_t vlo = 4u * (uint32_t)tid, vhi = 2u * (uint32_t)tid;
#pragma unroll
        for (int e = 0; e < E; e++) {
#ifdef SGFHE_ABL_NO_DIG
            x[0][e] = digit_reduce((uint64_t)(tid + e) * 0x9E3779B97F4Aull, md, sRd);  // timing-only build
#else
            // (the part of the stride below 4096 goes into the instruction's immediate offset)
            const uint32_t OL = (uint32_t)(4 * T * e), OH = (uint32_t)(2 * T * e);  // constants after unrolling
            const uint32_t lo = buf_ld_u32(rdig, vlo + (OL & 4095u), slo + (OL & ~4095u));
            uint32_t hi = buf_ld_u16(rdig, vhi + (OH & 4095u), shi + (OH & ~4095u));
            if constexpr (WIDE)
                hi |= buf_ld_u8(rdig, (uint32_t)tid + ((uint32_t)(T * e) & 4095u),
                                srec + 12u * (uint32_t)M + (uint32_t)(ph & 1) * (uint32_t)M + ((uint32_t)(T * e) & ~4095u)) << 16;
            x[0][e] = digit_reduce(lo | ((uint64_t)hi << 32), md, sRd);
#endif
            if constexpr (SPLIT > 1)    // next group of digit loads only after this group's reductions
                if ((e + 1) % (E / SPLIT) == 0 && e + 1 < E) __builtin_amdgcn_sched_barrier(0);
        }
        // the exchange buffer is reused: every wave must have finished the previous phase's loads
        SGFHE_SYNC();

        // 2. forward NTT of u[ph].  The key slice rows of this phase (from L2: every bootstrap of
        //    the launch reads the same slice) are requested after the transform.  Requesting them
        //    before its last pass keeps 32 more registers live through that pass: at the
        //    128-register budget hipcc then spills or shuffles the accumulators, and the kernel is
        //    slower (profiles/r02_exp_buffer_addressing.txt).
        const uint32_t skey = (pi * 8u + (uint32_t)ph * 2u) * 4u * (uint32_t)M;  // byte offset of key row ph, column 0
        const uint32_t vkey = 4u * (uint32_t)E * (uint32_t)tid;
        int4 ka4[E / 4], kb4[E / 4];
        ntt_forward<LOGM, 1, LE>(x, lds, P.twf, tid, md);
#pragma unroll
        for (int h = 0; h < E / 4; h++) {
#ifdef SGFHE_ABL_NO_KEY
            ka4[h] = make_int4(tid, h, ph, 7), kb4[h] = make_int4(h, tid, 5, ph);  // timing-only
#else
            ka4[h] = buf_ld_i4(rkey, vkey + 16u * (uint32_t)h, skey);
            kb4[h] = buf_ld_i4(rkey, vkey + 16u * (uint32_t)h, skey + 4u * (uint32_t)M);
#endif
        }

        // 3. pointwise: z_c += U * K[ph][c]   (fhe.jl:527-528 in the NTT domain), |U| < 3.95 * 2^29,
        //    |K| <= p / 2
        //    column 0: 64-bit multiply-accumulate (one v_mad_i64_i32 per product), reduced once after
        //              the loop.  (Montgomery-reduced per phase into 16 registers instead of 32:
        //              104 VGPRs and no spills, but 2 more multiplies per product; measured 230.8
        //              against 225.1 us per launch, profiles/r02_acc32_* vs r02_v1_*.)
        //    column 1: Montgomery-reduced (|.| < 0.75 * 2^29) and added to the LDS accumulator
        const Mod &mdp = md;
#pragma unroll
        for (int h = 0; h < E / 4; h++) {
            const int4 a = ka4[h], bq = kb4[h];
            const int32_t ka[4] = {a.x, a.y, a.z, a.w};
            const int32_t kb[4] = {bq.x, bq.y, bq.z, bq.w};
#pragma unroll
            for (int t = 0; t < 4; t++) {
                const int e = 4 * h + t;
                const int32_t u = x[0][e];
                acc0[e] += (int64_t)u * ka[t];
                int32_t *zp = reinterpret_cast<int32_t *>(lds) + M + e * T + tid;
                *zp += smont(u, kb[t], mdp);
            }
        }
    }
    // 4. inverse NTT of both columns at once (same twiddles, one set of exchanges; the second
    //    exchange buffer is the LDS area that held z_1):
    //    P_c = (M/p)^-1 * sum_row u_row (*) C_row[c]  mod p
    int32_t z[2][E];
    // With 16 points per thread the first inverse pass takes column 0 as the Montgomery step
    // leaves it (|.| < 1.49 * 2^29) and reduces six more of its sums instead (ntt.h inv_red_mask).
    // (the radix-4 inverse reduces column 0 on entry like column 1)
    constexpr bool WIDE0 = !inv_r4(LOGM) && LE == 4 && NttGeom<LOGM, LE>::SLAST_INV >= 0 &&
                           !(NttGeom<LOGM, LE>::RHO == 0 && NttGeom<LOGM, LE>::STOP == 0);
#pragma unroll
    for (int e = 0; e < E; e++) {
        const int32_t r0 = sredc(acc0[e], md);   // |REDC| < 1.49 * 2^29
        z[0][e] = WIDE0 ? r0 : sred(r0, md);
        z[1][e] = sred(z1[e * T], md);           // four phases: < 2.99 * 2^29
    }
    SGFHE_SYNC();  // every thread has taken its z_1 out of the buffer the exchanges now reuse
    ntt_inverse<LOGM, 2, LE, WIDE0>(z, lds, P.twi, tid, md);  // |z| < 1.4 * 2^29

    // Output addressing as for the digit loads: scalar offsets per column and coefficient, one
    // 32-bit lane offset.
    const uint32_t sy0 = (b * 2u * npr + pi) * 4u * (uint32_t)M;
    const uint32_t sy1 = sy0 + npr * 4u * (uint32_t)M;
    const uint32_t vout = 4u * (uint32_t)tid;
    // 5. y = x^j P - P  (mul_by_xj_minus_one, fhe.jl:554-556, applied to the product)
    if (mode & MODE_PLAIN) {
#pragma unroll
        for (int c = 0; c < 2; c++)
#pragma unroll
            for (int e = 0; e < E; e++)
                buf_st_u32(ryres, vout + ((uint32_t)(4 * T * e) & 4095u),
                              (c ? sy1 : sy0) + ((uint32_t)(4 * T * e) & ~4095u),
                              condsub(sfull(z[c][e], md) + P.hoff, (uint32_t)P.p));
        return;
    }
    const uint32_t j = ua[(size_t)b * n + k];
    const uint32_t yoff = handover_offset(P);
    // The transform's swizzled layout is kept for this exchange.  Its j-shifted reads collide where
    // the run of 64 source indices crosses a swizzle boundary (2.6 % of the kernel's LDS cycles,
    // profiles/r03_v10_counters.json).  A plain layout (word i of polynomial c at c m + i) has no
    // conflict for any j but needs one more workgroup barrier, and measured the same at m = 8192
    // (2108 against 2110 bootstraps/s, same call) and 2.3-2.4 % slower at m = 4096 and 16384
    // (profiles/r04_exp_epilogue.txt): LDS bandwidth is not what this kernel waits for.
    lds_store<LOGM, 2, LE, G::STOP>(z, lds, tid);
    SGFHE_SYNC();
    // Source index of output coefficient i = tid + T e is s_e = (i - j) mod 2m = s_0 + T e:
    // the swizzled low part is computed once per thread.
    {
        constexpr uint32_t LOWMASK = (1u << G::STOP) - 1u;
        const uint32_t s0 = ((uint32_t)tid - j) & (2 * M - 1);
        const uint32_t lowswz = swz<LE>(s0 & LOWMASK);
        const uint32_t h0 = s0 >> G::STOP;
#pragma unroll
        for (int e = 0; e < E; e++) {
            const uint32_t he = h0 + e;
            const uint32_t hipart = (he & (E - 1)) << G::STOP;
            // swz is XOR-linear; for m = 8192 the e bits lie above every bit it reads
            const uint32_t addr = hipart ^ lowswz ^ (G::STOP >= 9 ? 0u : swz_bits<LE>(hipart));
            // x^m = -1: the source is negated when bit LE of he is set.  -v = (v ^ -1) + 1, so
            // with smask = 0 / -1 the output is (v ^ smask) + (yoff - smask - z): one subtract and
            // one xor-add per residue, the per-e constants shared by both columns.
            const uint32_t smask = 0u - ((he >> LE) & 1u);
            const uint32_t yoe = yoff - smask;
#pragma unroll
            for (int c = 0; c < 2; c++) {
                const uint32_t v = lds[c * M + addr];
                const uint32_t y = (v ^ smask) + (yoe - (uint32_t)z[c][e]);
                buf_st_u32(ryres, vout + ((uint32_t)(4 * T * e) & 4095u),
                              (c ? sy1 : sy0) + ((uint32_t)(4 * T * e) & ~4095u), y);
            }
        }
    }
}

// ---- k_crt_acc --------------------------------------------------------------------------------
// One thread per (bootstrap, c, coefficient).  With y'_i = (D + H') (M/p_i)^-1 mod p_i:
//   D + H' = sum_i y'_i (M/p_i) - alpha M,  alpha = floor(sum_i y'_i / p_i)
// and |D| <= 0.4 M (5 m B Q <= M is checked at ctx creation) puts the fractional part of the sum
// within 0.5 +- 0.4, so alpha is exact in float (the estimate is off by < 10^-6).  The identity
// holds for any non-negative representatives y'_i = y_i + t p_i (alpha grows by t): k_extprod
// hands over residues below 5.7 p_i (6.2 p_i for the last prime), so alpha < 6 npr + 1.  Then x'_new = (x'_old + D) mod Q and the new digits are
// (x'_new mod B, x'_new / B)  (flatten, utils.jl:155-189).
//
// Arithmetic: S = sum_i y'_i c_i + T[alpha] + x'_old < 2^35 Q.  Its quotient by Q is estimated in
// double precision (error < 1), the remainder is formed modulo 2^96 in three 32-bit limbs
// (v_mad_u64_u32 chains) and corrected by at most one +-Q; same scheme for the division by B.
struct U96 {
    uint32_t w0, w1, w2;
};
__device__ __forceinline__ void mad96(U96 &a, uint32_t y, const uint32_t (&c)[3]) {
    const uint64_t p0 = (uint64_t)y * c[0] + a.w0;
    const uint64_t p1 = (uint64_t)y * c[1] + a.w1 + (p0 >> 32);
    a.w0 = (uint32_t)p0;
    a.w1 = (uint32_t)p1;
    a.w2 = y * c[2] + a.w2 + (uint32_t)(p1 >> 32);
}
// S = sum_i y_i c_i + T[alpha] (+ hi B + lo of the previous digits) reduced modulo Q: the
// canonical residue of x'_new (or of D when there is no previous accumulator), as three limbs.
template <int NP>
__device__ __forceinline__ U96 crt_reduce(const uint32_t (&y)[NP], const CrtConst *__restrict__ CC,
                                          bool have_old, ulonglong2 d) {
    float f = 0.f;
    double Sd = 0.0;
#pragma unroll
    for (int q = 0; q < NP; q++) {
        f += (float)y[q] * CC->invp[q];
#ifndef SGFHE_ABL_CRT_NOSD  // (timing-only build without the double-precision sum: wrong results)
        Sd += (double)y[q] * CC->cd[q];
#endif
    }
    const int alpha = (int)f;
    const uint4 tv = *reinterpret_cast<const uint4 *>(CC->T32[alpha]);
    U96 a = {tv.x, tv.y, tv.z};
    Sd += CC->Td[alpha];
#pragma unroll
    for (int q = 0; q < NP; q++) mad96(a, y[q], CC->c32[q]);
    if (have_old) {  // x'_old = hi B + lo
        const uint64_t B = (uint64_t)CC->B;
        const uint32_t h0 = (uint32_t)d.y, h1 = (uint32_t)(d.y >> 32);
        const uint32_t b0 = (uint32_t)B, b1 = (uint32_t)(B >> 32);
        const uint64_t p0 = (uint64_t)h0 * b0 + a.w0 + (uint32_t)d.x;
        const uint64_t p1 = (uint64_t)h0 * b1 + (uint64_t)h1 * b0 + a.w1 + (uint32_t)(d.x >> 32) + (p0 >> 32);
        a.w0 = (uint32_t)p0;
        a.w1 = (uint32_t)p1;
        a.w2 += h1 * b1 + (uint32_t)(p1 >> 32);
#ifndef SGFHE_ABL_CRT_NOSD
        Sd += (double)d.y * CC->Bd + (double)d.x;
#endif
    }
    // subtract q1 Q, q1 = floor(S / Q) +- 1
    {
        const uint64_t q1 = (uint64_t)(Sd * CC->invQ);
        const uint32_t qa = (uint32_t)q1, qb = (uint32_t)(q1 >> 32);
        const uint64_t m0 = (uint64_t)qa * CC->Q32[0];
        const uint64_t m1 = (uint64_t)qa * CC->Q32[1] + (uint64_t)qb * CC->Q32[0] + (m0 >> 32);
        const uint32_t m2 = qa * CC->Q32[2] + qb * CC->Q32[1] + (uint32_t)(m1 >> 32);
        const uint64_t r0 = (uint64_t)a.w0 - (uint32_t)m0;
        const uint64_t r1 = (uint64_t)a.w1 - (uint32_t)m1 - ((r0 >> 32) & 1u);
        a.w2 = a.w2 - m2 - (uint32_t)((r1 >> 32) & 1u);
        a.w0 = (uint32_t)r0;
        a.w1 = (uint32_t)r1;
    }
    // the remainder is in (-Q, 2Q) modulo 2^96: one correction
    {
        const uint64_t Qlo = ((uint64_t)CC->Q32[1] << 32) | CC->Q32[0];
        const uint32_t Qhi = CC->Q32[2];
        uint64_t lo = ((uint64_t)a.w1 << 32) | a.w0;
        uint32_t hi = a.w2;
        if ((int32_t)hi < 0) {  // negative: add Q
            const uint64_t nlo = lo + Qlo;
            hi = hi + Qhi + (nlo < lo);
            lo = nlo;
        } else if (hi > Qhi || (hi == Qhi && lo >= Qlo)) {
            const uint64_t nlo = lo - Qlo;
            hi = hi - Qhi - (lo < Qlo);
            lo = nlo;
        }
        a.w0 = (uint32_t)lo;
        a.w1 = (uint32_t)(lo >> 32);
        a.w2 = hi;
    }
    return a;
}
// Residues of coefficient i of (bootstrap, c) = bc, yres[bc][q][i] for q < NP.  ABLATE: the caller is one
// whose loads the timing-only build SGFHE_ABL_NO_YRES removes (wrong results).
template <int NP, bool ABLATE = false>
__device__ __forceinline__ void load_residues(const uint32_t *__restrict__ yres, uint32_t bc, uint32_t i,
                                              uint32_t logm, uint32_t (&y)[NP]) {
    const uint32_t yo = 4u * ((bc * NP << logm) + i);  // byte offset
#pragma unroll
    for (int q = 0; q < NP; q++) {
#ifdef SGFHE_ABL_NO_YRES
        if constexpr (ABLATE) { y[q] = (((bc << logm) + i) * 2654435761u + (uint32_t)q * 40503u) >> 3; continue; }
#endif
        y[q] = ld_off<uint32_t>(yres, yo + ((uint32_t)(4 * q) << logm));
    }
}
// The same for the four adjacent coefficients i .. i + 3 (i a multiple of 4), 16 bytes per prime.
// The residues are read exactly once: non-temporal loads keep them from displacing what the other
// lane's k_extprod re-reads from the caches (key slice, digit planes).  Same call, two lanes of
// 256 (profiles/r03_exp_cache_policy.txt): 2076 against 2016 bootstraps/s, +3.0 %, and +2.9 % on
// a second box; the old digits loaded the same way as well: +2.2 % (they are in the caches, the
// external product of this chunk has just read them), so those stay plain loads.
// ABLATE: as above, for the timing-only build SGFHE_ABL_NO_YLOAD.
template <int NP, bool ABLATE = false>
__device__ __forceinline__ void load_residues4(const uint32_t *__restrict__ yres, uint32_t bc, uint32_t i,
                                               uint32_t logm, uint4 (&yv)[NP]) {
    typedef unsigned int v4u __attribute__((ext_vector_type(4)));
    const uint32_t yo = 4u * ((bc * NP << logm) + i);
#pragma unroll
    for (int q = 0; q < NP; q++) {
#ifdef SGFHE_ABL_NO_YLOAD
        if constexpr (ABLATE) { yv[q] = make_uint4((((bc << logm) + i) >> 2) + q, yo, i + 7u * q, bc); continue; }
#endif
        const v4u t = __builtin_nontemporal_load(reinterpret_cast<const v4u *>(
            reinterpret_cast<const char *>(yres) + yo + ((uint32_t)(4 * q) << logm)));
        yv[q] = make_uint4(t.x, t.y, t.z, t.w);
    }
}
// coefficient j of the four
template <int NP>
__device__ __forceinline__ void residues_of(const uint4 (&yv)[NP], int j, uint32_t (&y)[NP]) {
#pragma unroll
    for (int q = 0; q < NP; q++) y[q] = j == 0 ? yv[q].x : j == 1 ? yv[q].y : j == 2 ? yv[q].z : yv[q].w;
}

template <int NP, bool ROWS = false>
__global__ void __launch_bounds__(256)
k_crt_acc(const uint32_t *__restrict__ yres, uint64_t *__restrict__ dig,
          const CrtConst *__restrict__ CC, uint32_t total, uint32_t logm, uint32_t mode,
          RndArgs ra, uint32_t iter) {
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const uint32_t M = 1u << logm;
    const uint32_t i = t & (M - 1);
    const uint32_t bc = t >> logm;
    uint32_t y[NP];
    load_residues<NP, true>(yres, bc, i, logm, y);
    const bool have_old = !(mode & MODE_NOACC);
    const bool wide = (mode & MODE_WIDE) != 0;
    const ulonglong2 d = have_old ? load_digits(dig, bc, i, M, wide) : make_ulonglong2(0, 0);
#ifdef SGFHE_ABL_CRT_MEMONLY  // timing-only build: every load and store, no arithmetic (wrong results)
    {
        uint32_t acc = 0;
#pragma unroll
        for (int q = 0; q < NP; q++) acc ^= y[q];
        store_digits(dig, bc, i, M, d.x ^ acc, d.y + acc);
        return;
    }
#endif
    const U96 a = crt_reduce(y, CC, have_old, d);
    const uint64_t xlo = ((uint64_t)a.w1 << 32) | a.w0;
    if (mode & MODE_CANON) {  // canonical residues, interleaved {lo, hi} words
        reinterpret_cast<ulonglong2 *>(dig)[t] = make_ulonglong2(xlo, (uint64_t)a.w2);
        return;
    }
    if (mode & MODE_RANDOM) {
        ChaChaKey key;
        uint32_t cz, cw;
        rnd_stream<ROWS>(ra, bc >> 1, key, cz, cw);
        const uint4 ctr = make_uint4(((bc & 1u) << logm) + i, iter, cz, cw);
        const ulonglong2 e = random_digits(((u128)a.w2 << 64) | xlo, CC, key, ctr);
        store_digits(dig, bc, i, M, e.x, e.y, wide);
        return;
    }
    // digits: hi = x' / B (double estimate +- 1), lo = x' - hi B (exact modulo 2^64)
    const uint64_t B = (uint64_t)CC->B;
    const double xd = (double)a.w2 * 18446744073709551616.0 + (double)xlo;
    uint64_t hq = (uint64_t)(xd * CC->invB);
    int64_t lo = (int64_t)(xlo - hq * B);
    if (lo < 0) { lo += (int64_t)B; hq--; }
    else if ((uint64_t)lo >= B) { lo -= (int64_t)B; hq++; }
    store_digits(dig, bc, i, M, (uint64_t)lo, hq);
}

// The k-loop's own case (deterministic flatten, previous accumulator present) with two adjacent
// coefficients per thread: 8-byte residue and digit-word loads / stores and 4-byte loads / stores
// of the 16-bit high words -- half the memory instructions for the same bytes.  Same arithmetic.
template <int NP>
__global__ void __launch_bounds__(256)
k_crt_acc2(const uint32_t *__restrict__ yres, uint64_t *__restrict__ dig,
           const CrtConst *__restrict__ CC, uint32_t pairs, uint32_t logm) {
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= pairs) return;
    const uint32_t M = 1u << logm;
    const uint32_t i = (2u * t) & (M - 1);  // even
    const uint32_t bc = (2u * t) >> logm;
    const uint32_t yo = 4u * ((bc * NP << logm) + i);
    uint2 yv[NP];
#pragma unroll
    for (int q = 0; q < NP; q++) yv[q] = ld_off<uint2>(yres, yo + ((uint32_t)(4 * q) << logm));
    const uint32_t rec = bc * 16u * M;
    const uint32_t ol = rec + 4u * i, oh = rec + 8u * M + 2u * i;
    const uint2 l0 = ld_off<uint2>(dig, ol), l1 = ld_off<uint2>(dig, ol + 4u * M);
    const uint32_t h0 = ld_off<uint32_t>(dig, oh), h1 = ld_off<uint32_t>(dig, oh + 2u * M);
#ifdef SGFHE_ABL_CRT_MEMONLY  // timing-only build: every load and store, no arithmetic (wrong results)
    {
        uint32_t ax = 0, ay = 0;
#pragma unroll
        for (int q = 0; q < NP; q++) { ax ^= yv[q].x; ay += yv[q].y; }
        st_off<uint2>(dig, ol, make_uint2(l0.x ^ ax, l0.y + ay));
        st_off<uint2>(dig, ol + 4u * M, make_uint2(l1.x + ay, l1.y ^ ax));
        st_off<uint32_t>(dig, oh, h0 ^ ax);
        st_off<uint32_t>(dig, oh + 2u * M, h1 + ay);
        return;
    }
#endif
    const uint64_t B = (uint64_t)CC->B;
    uint32_t olo[2][2], ohi[2][2];  // [digit][coefficient]
#pragma unroll
    for (int j = 0; j < 2; j++) {
        uint32_t y[NP];
#pragma unroll
        for (int q = 0; q < NP; q++) y[q] = j ? yv[q].y : yv[q].x;
        const uint32_t hw0 = j ? (h0 >> 16) : (h0 & 0xFFFFu), hw1 = j ? (h1 >> 16) : (h1 & 0xFFFFu);
        const ulonglong2 d = make_ulonglong2((j ? l0.y : l0.x) | ((uint64_t)hw0 << 32),
                                             (j ? l1.y : l1.x) | ((uint64_t)hw1 << 32));
        const U96 a = crt_reduce(y, CC, true, d);
        const uint64_t xlo = ((uint64_t)a.w1 << 32) | a.w0;
        const double xd = (double)a.w2 * 18446744073709551616.0 + (double)xlo;
        uint64_t hq = (uint64_t)(xd * CC->invB);
        int64_t lo = (int64_t)(xlo - hq * B);
        if (lo < 0) { lo += (int64_t)B; hq--; }
        else if ((uint64_t)lo >= B) { lo -= (int64_t)B; hq++; }
        olo[0][j] = (uint32_t)lo; ohi[0][j] = (uint32_t)((uint64_t)lo >> 32);
        olo[1][j] = (uint32_t)hq; ohi[1][j] = (uint32_t)(hq >> 32);
    }
    st_off<uint2>(dig, ol, make_uint2(olo[0][0], olo[0][1]));
    st_off<uint2>(dig, ol + 4u * M, make_uint2(olo[1][0], olo[1][1]));
    st_off<uint32_t>(dig, oh, (ohi[0][0] & 0xFFFFu) | (ohi[0][1] << 16));
    st_off<uint32_t>(dig, oh + 2u * M, (ohi[1][0] & 0xFFFFu) | (ohi[1][1] << 16));
}

// ---- k_crt_lean: the k-loop's CRT + accumulate + flatten in integer arithmetic ---------------------
// Same function as k_crt_acc2 (deterministic flatten, previous accumulator present) at less than
// half the vector instructions: the kernel is HBM-bound on its own, but on the second lane it runs
// beside the other chunk's k_extprod, which is bound by vector-ALU issue -- there every instruction
// of this kernel is paid in full (profiles/r03_exp_crt_ceiling.txt).  No floating point, no table:
//   alpha = (sum_i y_i w_i) >> 58,  w_i = floor(2^58 / p_i)           (5 multiply-adds)
//   S = sum_i y'_i c_i + alpha (-M mod Q) + hi_old B + lo_old  <  2^34.5 Q,  y'_i = y_i except
//     y'_last = y_last - (p_last - 1) / 2: that takes H' = (M / p_last) (p_last - 1) / 2 out again
//     as NL sums L_k over 29-bit limbs of the constants: every product is below 2^61, so a limb sum
//     is one chain of v_mad_u64_u32 with no carry handling (S = sum_k L_k 2^(29 k))
//   q = ((S >> t) mq) >> 72 with mq = floor(2^(t + 72) / Q) < 2^44, t = bits(Q) - 29, S >> t taken
//     from the top three limb sums: q is floor(S / Q) or one less
//   x = S - q Q modulo 2^96, in [0, 2 Q): one conditional subtraction
//   hq = ((x >> t2) mb) >> (bits(B) + 51 - t2), mb = floor(2^(bits(B) + 51) / B) <= 2^52:
//     floor(x / B) or one less;  lo = x - hq B modulo 2^64, in [0, 2 B): one conditional subtraction.
// tests/rns_model.py::CrtLean restates this with every intermediate checked against its register
// width and both estimates checked against the exact quotients.
// Four adjacent coefficients per thread: 16-byte residue and digit-word accesses, 8-byte accesses
// of the 16-bit high words.
// (struct CrtLean, the constants: constants.h)

// (x m) >> 64 for x < 2^63.5 and m = m1 2^32 + m0 with m1 <= 2^20
__device__ __forceinline__ uint64_t mulhi64_lean(uint64_t x, uint32_t m0, uint32_t m1) {
    const uint32_t x0 = (uint32_t)x, x1 = (uint32_t)(x >> 32);
    const uint64_t t1 = (uint64_t)x0 * m1 + __umulhi(x0, m0);
    const uint64_t t2 = (uint64_t)x1 * m0 + t1;
    return (uint64_t)x1 * m1 + (t2 >> 32);
}

template <int NP, int NL, bool RND = false>
__device__ __forceinline__ void crt_lean_one(const uint32_t (&y)[NP], uint64_t lo_o, uint64_t hi_o,
                                             const CrtLean *__restrict__ K, uint64_t &lo_n,
                                             uint64_t &hi_n) {
    // alpha
    uint64_t acc = 0;
#pragma unroll
    for (int q = 0; q < NP; q++) acc += (uint64_t)y[q] * K->w[q];
    const uint32_t alpha = (uint32_t)(acc >> 58);
    // limb sums
    const uint32_t ylast = y[NP - 1] - K->hoff;   // >= 0: the residue proper is non-negative
    uint64_t L[NL];
#pragma unroll
    for (int k = 0; k < NL; k++) {
        uint64_t l = k == 0 ? lo_o : 0;
#pragma unroll
        for (int q = 0; q < NP; q++) l += (uint64_t)(q == NP - 1 ? ylast : y[q]) * K->c[q][k];
        L[k] = l + (uint64_t)alpha * K->cMn[k];
        if constexpr (RND) L[k] += K->cR[k];
    }
    {   // + hi_old B
        const uint32_t h0 = (uint32_t)hi_o, h1 = (uint32_t)(hi_o >> 32);
        L[0] += (uint64_t)h0 * K->B0;
        L[1] += (uint64_t)h0 * K->B1;
        L[1] += ((uint64_t)h1 * K->B0) << 3;
        if constexpr (NL >= 3) L[2] += ((uint64_t)h1 * K->B1) << 3;
    }
    // quotient by Q
    const uint32_t a = K->a;
    uint64_t X = (L[NL - 1] << a) + (L[NL - 2] >> (29 - a));
    if constexpr (NL >= 3) X += L[NL - 3] >> (58 - a);
    const uint64_t q1 = mulhi64_lean(X, K->mq0, K->mq1) >> 8;
    // S modulo 2^96
    uint64_t slo = L[0];
    uint32_t shi = 0;
    {
        const uint64_t v = L[1] << 29;
        slo += v;
        shi += (uint32_t)(L[1] >> 35) + (slo < v);
    }
    if constexpr (NL >= 3) {
        const uint64_t v = L[2] << 58;
        slo += v;
        shi += (uint32_t)(L[2] >> 6) + (slo < v);
    }
    if constexpr (NL >= 4) shi += (uint32_t)L[3] << 23;
    // x = S - q1 Q modulo 2^96
    uint64_t xlo;
    uint32_t xhi;
    {
        const uint32_t qa = (uint32_t)q1, qb = (uint32_t)(q1 >> 32);
        const uint64_t m0 = (uint64_t)qa * K->Qw[0];
        const uint64_t m1 = (uint64_t)qa * K->Qw[1] + (m0 >> 32) + (uint64_t)qb * K->Qw[0];  // modulo 2^64
        const uint32_t m2 = qa * K->Qw[2] + qb * K->Qw[1] + (uint32_t)(m1 >> 32);
        const uint64_t mlo = (m1 << 32) | (uint32_t)m0;
        xlo = slo - mlo;
        xhi = shi - m2 - (slo < mlo);
    }
    {   // in [0, 2 Q): subtract Q when that does not borrow
        const uint64_t Qlo = ((uint64_t)K->Qw[1] << 32) | K->Qw[0];
        const uint64_t dlo = xlo - Qlo;
        const uint32_t bor = xlo < Qlo;
        const uint32_t dhi = xhi - K->Qw[2] - bor;
        const bool below = xhi < K->Qw[2] || (xhi == K->Qw[2] && bor);   // x < Q
        xlo = below ? xlo : dlo;
        xhi = below ? xhi : dhi;
    }
    // digits
    const uint32_t t2 = K->t2;
    const uint64_t X2 = t2 ? ((xlo >> t2) | ((uint64_t)xhi << (64 - t2))) : xlo;
    uint64_t hq = mulhi64_lean(X2, K->mb0, K->mb1) >> K->sB;
    const uint64_t Bv = ((uint64_t)K->Bw1 << 32) | K->Bw0;
    uint64_t lo = xlo - hq * Bv;   // modulo 2^64: in [0, 2 B)
    if (lo >= Bv) { lo -= Bv; hq += 1; }
    lo_n = lo;
    hi_n = hq;
}

// crt_lean_one at five primes, Q of 87 bits and B of 44 bits (Params(1024)).  There the three 29-bit
// limbs cover Q exactly (a = 0, t2 + sB = 31), so every shift of the recombination is a constant and
// both quotients are read from 32-bit words: no 64-bit shift, no 64-bit compare.
//   limb sums as crt_lean_one, hi_old B as h0 B0 + h0 B1 2^29 + h1 (8 B0) 2^29 + h1 (8 B1) 2^58
//   U = L0 + lo(L1) 2^29,  X = L2 + 8 hi(L1):  S = U + 2^58 X exactly, U and X below 2^64
//   q = (X mq) >> 64 with mq = floor(2^122 / Q) <= 2^36:  floor(S / Q) or one less
//   x = S - q Q modulo 2^96 in 32-bit words, in [0, 2 Q): minus Q unless that borrows
//   hq = ((x >> 32) mb) >> 64 with mb = floor(2^96 / B) <= 2^53:  floor(x / B) or one less
//   lo = x - hq B modulo 2^64, in [0, 2 B): minus B, and hq + 1, unless that borrows.
// The two corrections are subtract-with-borrow chains whose borrow-out selects.  Same digits as
// crt_lean_one; tests/test_crt_lean87_model.py restates it with every register width checked and
// both estimates checked against the exact quotients.
__device__ __forceinline__ uint32_t sub_borrow(uint32_t a, uint32_t b, uint32_t bin, uint32_t &bout) {
    uint32_t r;
    bout = __builtin_sub_overflow(a, b, &r);
    bout |= __builtin_sub_overflow(r, bin, &r);
    return r;
}

// (x m) >> 64 for x < 2^64 and m = m1 2^32 + m0 with m1 < 2^24, less than one below the exact value:
// mulhi64_lean with its three multiply-adds in this order (left to itself the compiler reassociates
// them into four instructions and a move).  m0 and m1 are wave-uniform (SGPRs).
__device__ __forceinline__ uint64_t mad_u64_u32_vs(uint32_t a, uint32_t b, uint64_t c) {
#ifdef SGFHE_HOST_KERNELS
    return (uint64_t)a * b + c;
#else
    uint64_t r, cy;
    asm("v_mad_u64_u32 %0, %1, %2, %3, %4" : "=v"(r), "=s"(cy) : "v"(a), "s"(b), "v"(c));
    return r;
#endif
}
__device__ __forceinline__ uint64_t mulhi64_87(uint64_t x, uint32_t m0, uint32_t m1) {
    const uint32_t x0 = (uint32_t)x, x1 = (uint32_t)(x >> 32);
    const uint64_t t1 = mad_u64_u32_vs(x0, m1, __umulhi(x0, m0));
    const uint64_t t2 = mad_u64_u32_vs(x1, m0, t1);
    return mad_u64_u32_vs(x1, m1, t2 >> 32);
}

// Q and B in 32-bit words as vector registers (one copy per thread, not one per use): the borrow
// chains take them as their second operand, which has to be a VGPR.
struct Lean87W {
    uint32_t Q0, Q1, Q2, B0, B1;
};

template <int NP>
__device__ __forceinline__ void crt_lean87_one(const uint32_t (&y)[NP], uint64_t lo_o, uint32_t h0,
                                               uint32_t h1, const CrtLean *__restrict__ K, const Lean87W &W,
                                               uint64_t &lo_n, uint64_t &hi_n) {
    uint64_t acc = 0;
#pragma unroll
    for (int q = 0; q < NP; q++) acc += (uint64_t)y[q] * K->w[q];
    const uint32_t alpha = (uint32_t)(acc >> 32) >> 26;
    const uint32_t ylast = y[NP - 1] - K->hoff;
    uint64_t L0 = lo_o + (uint64_t)h0 * K->B0;
    uint64_t L1 = (uint64_t)h0 * K->B1 + (uint64_t)h1 * (K->B0 << 3);
    uint64_t L2 = (uint64_t)h1 * (K->B1 << 3);
#pragma unroll
    for (int q = 0; q < NP; q++) {
        const uint32_t yq = q == NP - 1 ? ylast : y[q];
        L0 += (uint64_t)yq * K->c[q][0];
        L1 += (uint64_t)yq * K->c[q][1];
        L2 += (uint64_t)yq * K->c[q][2];
    }
    L0 += (uint64_t)alpha * K->cMn[0];
    L1 += (uint64_t)alpha * K->cMn[1];
    L2 += (uint64_t)alpha * K->cMn[2];
    // (the multipliers 2^29 and 8 are hidden from the optimiser, which would otherwise turn these two
    // multiply-adds into 64-bit shifts, masks and adds)
    uint32_t m29 = 1u << 29, m3 = 8;
    SGFHE_HIDE("+s"(m29), "+s"(m3));
    const uint64_t U = (uint64_t)(uint32_t)L1 * m29 + L0;
    const uint64_t X = (uint64_t)(uint32_t)(L1 >> 32) * m3 + L2;
    // quotient by Q and q Q modulo 2^96
    const uint64_t q = mulhi64_87(X, K->mqw0, K->mqw1);
    const uint32_t qa = (uint32_t)q, qb = (uint32_t)(q >> 32);
    const uint64_t p0 = (uint64_t)qa * K->Qw[0];
    const uint64_t p1 = (uint64_t)qa * K->Qw[1] + (p0 >> 32);
    const uint32_t p2 = (uint32_t)(p1 >> 32) + qa * K->Qw[2] + qb * K->Qw[1];
    const uint64_t p12 = ((((uint64_t)p2 << 32) | (uint32_t)p1)) + (uint64_t)qb * K->Qw[0];
    // x = S - q Q:  S = U + 2^58 X in words (U.lo, U.hi + (X << 26) mod 2^64)
    const uint64_t s12 = (U >> 32) + (X << 26);
    uint32_t br;
    uint32_t x0 = sub_borrow((uint32_t)U, (uint32_t)p0, 0, br);
    uint32_t x1 = sub_borrow((uint32_t)s12, (uint32_t)p12, br, br);
    uint32_t x2 = (uint32_t)(s12 >> 32) - (uint32_t)(p12 >> 32) - br;
    {   // in [0, 2 Q): subtract Q when that does not borrow
        uint32_t b;
        const uint32_t d0 = sub_borrow(x0, W.Q0, 0, b);
        const uint32_t d1 = sub_borrow(x1, W.Q1, b, b);
        const uint32_t d2 = sub_borrow(x2, W.Q2, b, b);
        x0 = b ? x0 : d0;
        x1 = b ? x1 : d1;
        x2 = b ? x2 : d2;
    }
    // digits
    uint64_t hq = mulhi64_87(((uint64_t)x2 << 32) | x1, K->mbw0, K->mbw1);
    const uint32_t g0 = (uint32_t)hq, g1 = (uint32_t)(hq >> 32);
    const uint64_t pb = (uint64_t)g0 * K->Bw0;
    const uint32_t pbh = (uint32_t)(pb >> 32) + g0 * K->Bw1 + g1 * K->Bw0;
    uint32_t b;
    uint32_t lo0 = sub_borrow(x0, (uint32_t)pb, 0, b);
    uint32_t lo1 = x1 - pbh - b;
    {   // in [0, 2 B): subtract B when that does not borrow
        const uint32_t d0 = sub_borrow(lo0, W.B0, 0, b);
        const uint32_t d1 = sub_borrow(lo1, W.B1, b, b);
        lo0 = b ? lo0 : d0;
        lo1 = b ? lo1 : d1;
        hq += 1u - b;
    }
    lo_n = ((uint64_t)lo1 << 32) | lo0;
    hi_n = hq;
}

template <int NP, int NL, bool P87 = false>
__global__ void __launch_bounds__(256)
k_crt_lean(const uint32_t *__restrict__ yres, uint64_t *__restrict__ dig,
           const CrtLean *__restrict__ K, uint32_t quads, uint32_t logm) {
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= quads) return;
    const uint32_t M = 1u << logm;
    const uint32_t i = (4u * t) & (M - 1);  // multiple of 4
    const uint32_t bc = (4u * t) >> logm;
    uint4 yv[NP];
    load_residues4<NP, true>(yres, bc, i, logm, yv);
    const uint32_t rec = bc * 16u * M;
    const uint32_t ol = rec + 4u * i, oh = rec + 8u * M + 2u * i;
    const uint4 l0 = ld_off<uint4>(dig, ol), l1 = ld_off<uint4>(dig, ol + 4u * M);
    const uint2 h0 = ld_off<uint2>(dig, oh), h1 = ld_off<uint2>(dig, oh + 2u * M);
    const uint32_t l0w[4] = {l0.x, l0.y, l0.z, l0.w}, l1w[4] = {l1.x, l1.y, l1.z, l1.w};
    const uint32_t h0w[4] = {h0.x & 0xFFFFu, h0.x >> 16, h0.y & 0xFFFFu, h0.y >> 16};
    const uint32_t h1w[4] = {h1.x & 0xFFFFu, h1.x >> 16, h1.y & 0xFFFFu, h1.y >> 16};
    Lean87W W{};
    if constexpr (P87) {
        W = Lean87W{K->Qw[0], K->Qw[1], K->Qw[2], K->Bw0, K->Bw1};
        SGFHE_HIDE("+v"(W.Q0), "+v"(W.Q1), "+v"(W.Q2), "+v"(W.B0), "+v"(W.B1));
    }
    uint64_t nlo[4], nhi[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        uint32_t y[NP];
        residues_of(yv, j, y);
        if constexpr (P87)
            crt_lean87_one<NP>(y, l0w[j] | ((uint64_t)h0w[j] << 32), l1w[j], h1w[j], K, W, nlo[j], nhi[j]);
        else
            crt_lean_one<NP, NL>(y, l0w[j] | ((uint64_t)h0w[j] << 32), l1w[j] | ((uint64_t)h1w[j] << 32), K,
                                 nlo[j], nhi[j]);
    }
    st_off<uint4>(dig, ol, make_uint4((uint32_t)nlo[0], (uint32_t)nlo[1], (uint32_t)nlo[2], (uint32_t)nlo[3]));
    st_off<uint4>(dig, ol + 4u * M,
                  make_uint4((uint32_t)nhi[0], (uint32_t)nhi[1], (uint32_t)nhi[2], (uint32_t)nhi[3]));
    st_off<uint2>(dig, oh, make_uint2((uint32_t)(nlo[0] >> 32) | ((uint32_t)(nlo[1] >> 32) << 16),
                                      (uint32_t)(nlo[2] >> 32) | ((uint32_t)(nlo[3] >> 32) << 16)));
    st_off<uint2>(dig, oh + 2u * M, make_uint2((uint32_t)(nhi[0] >> 32) | ((uint32_t)(nhi[1] >> 32) << 16),
                                               (uint32_t)(nhi[2] >> 32) | ((uint32_t)(nhi[3] >> 32) << 16)));
}

// The same with ONE coefficient per thread, for the latency form of the k-loop (a call of a few gates):
// there the kernel is a dependent link of the launch chain, one wave per SIMD, and what counts is the
// length of a thread's instruction stream (117 instead of 468), not the width of its memory accesses.
template <int NP, int NL>
__global__ void __launch_bounds__(256)
k_crt_lean1(const uint32_t *__restrict__ yres, uint64_t *__restrict__ dig,
            const CrtLean *__restrict__ K, uint32_t total, uint32_t logm) {
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const uint32_t M = 1u << logm;
    const uint32_t i = t & (M - 1);
    const uint32_t bc = t >> logm;
    uint32_t y[NP];
    load_residues<NP>(yres, bc, i, logm, y);
    const ulonglong2 d = load_digits(dig, bc, i, M);
    uint64_t lo, hi;
    crt_lean_one<NP, NL>(y, d.x, d.y, K, lo, hi);
    store_digits(dig, bc, i, M, lo, hi);
}

// The randomised flatten (utils.jl:198-241; random_digits above) through the same limb sums.  With
// r_i the draws in [0, 2 xmax] and (e_lo, e_hi) the old stored digits, the value to flatten is
//   x2 = (x_old + D - r_0 - r_1 B) mod Q,   x_old == e_hi B + e_lo  (mod Q),
// so the draws enter as 2 xmax - r_i >= 0 added to the old digits, the constant
// cR = (-2 xmax (1 + B)) mod Q puts the shift back, and the one quotient step of crt_lean_one gives
// x2 directly -- no reduction of r_1 B + r_0, no second quotient.  New stored digits: those of x2
// plus r_i.  Same stream addressing as k_crt_acc (random_digits), bit-identical output (tests: the oracle; the
// register widths: tests/rns_model.py CrtLean.digits_random).
template <int NP, int NL, bool WIDE, bool ROWS = false>
__global__ void __launch_bounds__(256)
k_crt_lean_rnd(const uint32_t *__restrict__ yres, uint64_t *__restrict__ dig,
               const CrtLean *__restrict__ K, uint32_t quads, uint32_t logm, RndArgs ra, uint32_t iter) {
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= quads) return;
    const uint32_t M = 1u << logm;
    const uint32_t i = (4u * t) & (M - 1);  // multiple of 4
    const uint32_t bc = (4u * t) >> logm;
    uint4 yv[NP];
    load_residues4<NP>(yres, bc, i, logm, yv);
    const uint32_t rec = bc * 16u * M;
    const uint32_t ol = rec + 4u * i, oh = rec + 8u * M + 2u * i, ot = rec + 12u * M + i;
    const uint4 l0 = ld_off<uint4>(dig, ol), l1 = ld_off<uint4>(dig, ol + 4u * M);
    const uint2 h0 = ld_off<uint2>(dig, oh), h1 = ld_off<uint2>(dig, oh + 2u * M);
    uint32_t t0 = 0, t1 = 0;   // third plane: bits 48..55 of the four stored digits
    if constexpr (WIDE) { t0 = ld_off<uint32_t>(dig, ot); t1 = ld_off<uint32_t>(dig, ot + M); }
    const uint32_t l0w[4] = {l0.x, l0.y, l0.z, l0.w}, l1w[4] = {l1.x, l1.y, l1.z, l1.w};
    const uint32_t h0w[4] = {h0.x & 0xFFFFu, h0.x >> 16, h0.y & 0xFFFFu, h0.y >> 16};
    const uint32_t h1w[4] = {h1.x & 0xFFFFu, h1.x >> 16, h1.y & 0xFFFFu, h1.y >> 16};
    const uint64_t xm2 = ((uint64_t)K->xm2hi << 32) | K->xm2lo, span = xm2 + 1;
    const uint32_t cx = ((bc & 1u) << logm) + i;
    ChaChaKey key;
    uint32_t cz, cw;
    rnd_stream<ROWS>(ra, bc >> 1, key, cz, cw);
    uint32_t rw[16];   // the draws of the thread's four coefficients: one block of the stream
    chacha_block<RND_ROUNDS>(key, cx >> 2, iter, cz, cw, rw);
    uint64_t nlo[4], nhi[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        uint32_t y[NP];
        residues_of(yv, j, y);
        const uint64_t r0 = __umul64hi(((uint64_t)rw[4 * j + 1] << 32) | rw[4 * j], span);
        const uint64_t r1 = __umul64hi(((uint64_t)rw[4 * j + 3] << 32) | rw[4 * j + 2], span);
        uint32_t hw0 = h0w[j], hw1 = h1w[j];
        if constexpr (WIDE) {
            hw0 |= ((t0 >> (8 * j)) & 0xFFu) << 16;
            hw1 |= ((t1 >> (8 * j)) & 0xFFu) << 16;
        }
        const uint64_t e_lo = l0w[j] | ((uint64_t)hw0 << 32), e_hi = l1w[j] | ((uint64_t)hw1 << 32);
        crt_lean_one<NP, NL, true>(y, e_lo + (xm2 - r0), e_hi + (xm2 - r1), K, nlo[j], nhi[j]);
        nlo[j] += r0;
        nhi[j] += r1;
    }
    st_off<uint4>(dig, ol, make_uint4((uint32_t)nlo[0], (uint32_t)nlo[1], (uint32_t)nlo[2], (uint32_t)nlo[3]));
    st_off<uint4>(dig, ol + 4u * M,
                  make_uint4((uint32_t)nhi[0], (uint32_t)nhi[1], (uint32_t)nhi[2], (uint32_t)nhi[3]));
    st_off<uint2>(dig, oh, make_uint2(((uint32_t)(nlo[0] >> 32) & 0xFFFFu) | ((uint32_t)(nlo[1] >> 32) << 16),
                                      ((uint32_t)(nlo[2] >> 32) & 0xFFFFu) | ((uint32_t)(nlo[3] >> 32) << 16)));
    st_off<uint2>(dig, oh + 2u * M, make_uint2(((uint32_t)(nhi[0] >> 32) & 0xFFFFu) | ((uint32_t)(nhi[1] >> 32) << 16),
                                               ((uint32_t)(nhi[2] >> 32) & 0xFFFFu) | ((uint32_t)(nhi[3] >> 32) << 16)));
    if constexpr (WIDE) {
        uint32_t w0 = 0, w1 = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            w0 |= ((uint32_t)(nlo[j] >> 48) & 0xFFu) << (8 * j);
            w1 |= ((uint32_t)(nhi[j] >> 48) & 0xFFu) << (8 * j);
        }
        st_off<uint32_t>(dig, ot, w0);
        st_off<uint32_t>(dig, ot + M, w1);
    }
}

// The randomised flatten with ONE coefficient per thread, for the latency form (a call of a few gates): every
// thread computes the ChaCha block of its quad of coefficients -- four times the block function across the
// launch, which an otherwise idle device does not notice -- and uses its own four words of it, so a thread's
// instruction stream is one block and one CRT instead of one block and four.  Same stream addressing, same
// digits as k_crt_lean_rnd.  QUARTER: residues from the partial values of the quarter kernels.  Not for the
// three-plane digit records (B >= 2^46).
template <int NP, int NL, bool QUARTER, bool ROWS = false>
__global__ void __launch_bounds__(256)
k_crt_lean_rnd1(const uint32_t *__restrict__ yres, uint64_t *__restrict__ dig,
                const CrtLean *__restrict__ K, uint32_t total, uint32_t logm, RndArgs ra, uint32_t iter,
                const PrimeK *__restrict__ PS) {
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const uint32_t M = 1u << logm;
    const uint32_t i = t & (M - 1);
    const uint32_t bc = t >> logm;
    uint32_t y[NP];
    if constexpr (QUARTER)
        quarter_residues<NP>(reinterpret_cast<const int32_t *>(yres), PS, bc, i, logm, y);
    else
        load_residues<NP>(yres, bc, i, logm, y);
    const ulonglong2 d = load_digits(dig, bc, i, M);
    const uint64_t xm2 = ((uint64_t)K->xm2hi << 32) | K->xm2lo, span = xm2 + 1;
    const uint32_t cx = ((bc & 1u) << logm) + i;
    ChaChaKey key;
    uint32_t cz, cw;
    rnd_stream<ROWS>(ra, bc >> 1, key, cz, cw);
    uint32_t rw[16];
    chacha_block<RND_ROUNDS>(key, cx >> 2, iter, cz, cw, rw);
    const uint32_t sel = cx & 3u;   // this coefficient's four words of the block
    const uint32_t w0 = sel == 0 ? rw[0] : sel == 1 ? rw[4] : sel == 2 ? rw[8] : rw[12];
    const uint32_t w1 = sel == 0 ? rw[1] : sel == 1 ? rw[5] : sel == 2 ? rw[9] : rw[13];
    const uint32_t w2 = sel == 0 ? rw[2] : sel == 1 ? rw[6] : sel == 2 ? rw[10] : rw[14];
    const uint32_t w3 = sel == 0 ? rw[3] : sel == 1 ? rw[7] : sel == 2 ? rw[11] : rw[15];
    const uint64_t r0 = __umul64hi(((uint64_t)w1 << 32) | w0, span);
    const uint64_t r1 = __umul64hi(((uint64_t)w3 << 32) | w2, span);
    uint64_t lo, hi;
    crt_lean_one<NP, NL, true>(y, d.x + (xm2 - r0), d.y + (xm2 - r1), K, lo, hi);
    store_digits(dig, bc, i, M, lo + r0, hi + r1);
}

// ---- small-batch ("latency") form of the external product --------------------------------------
// A call with a handful of gates leaves most of the 256 CUs idle while one workgroup per
// (bootstrap, prime) walks through 4 forward and 2 inverse transforms.  Here the same work is cut
// into 4 + 2 independent workgroups per (bootstrap, prime), three launches per iteration:
//   k_fwd_phase   (bootstrap, prime, key row ph)  digit plane -> forward NTT -> products with the
//                 two key polynomials of that row, |.| < 0.74 * 2^29        -> zpart
//   k_inv_column  (bootstrap, prime, column c)    sum of the four partial products -> inverse NTT
//                 -> (x^j - 1) rotation -> residues                         -> yres
//   k_crt_acc     as before.
//   zpart [chunk][npr][4][2][m]   slot order (the order of the key slices)
// Both run with 8 points per thread where that fits a workgroup (LE = 3: twice the threads on
// each transform); the slot order of a transform does not depend on the points per thread.
template <int LOGM, int LE, bool WIDE = false>
__global__ void __launch_bounds__((NttGeom<LOGM, LE>::T), (NttGeom<LOGM, LE>::T >= 256 ? 4 : 1))
k_fwd_phase(const uint64_t *__restrict__ dig, const int32_t *__restrict__ keyk,
            int32_t *__restrict__ zpart, PrimeSet PS, uint32_t mode) {
    using G = NttGeom<LOGM, LE>;
    constexpr int M = G::M, T = G::T, E = G::E;
    SGFHE_DYN_LDS(uint32_t, lds);
    const int tid = threadIdx.x;
    const uint32_t npr = PS[0].npr;
    const uint32_t ph = blockIdx.x & 3u;
    const uint32_t pi = (blockIdx.x >> 2) % npr;
    const uint32_t b = (blockIdx.x >> 2) / npr;
    const PrimeK P = PS[pi];
    const Mod md = mod_of(P);
    const int32_t sRd = (mode & MODE_RANDOM) ? P.sRr : P.sR;

    int32_t x[1][E];
    const uint32_t *dl = digit_lo_plane(dig, (size_t)b * 2 + (ph >> 1), M) + (ph & 1) * M;
    const uint16_t *dh = digit_hi_plane(dig, (size_t)b * 2 + (ph >> 1), M) + (ph & 1) * M;
    const uint8_t *dt = reinterpret_cast<const uint8_t *>(dig + ((size_t)b * 2 + (ph >> 1)) * 2 * M) + 12 * M + (ph & 1) * M;
#pragma unroll
    for (int e = 0; e < E; e++) {
        uint64_t d = dl[tid + T * e] | ((uint64_t)dh[tid + T * e] << 32);
        if constexpr (WIDE) d |= (uint64_t)dt[tid + T * e] << 48;
        x[0][e] = digit_reduce(d, md, sRd);
    }
    ntt_forward<LOGM, 1, LE>(x, lds, P.twf, tid, md);

    const int32_t *kp = keyk + ((size_t)pi * 8 + ph * 2) * M + E * tid;
    int32_t *zp = zpart + ((((size_t)b * npr + pi) * 4 + ph) * 2) * M + E * tid;
    key_row_products<M, E>(x, kp, zp, md);
}

template <int LOGM, int LE>
__global__ void __launch_bounds__((NttGeom<LOGM, LE>::T), (NttGeom<LOGM, LE>::T >= 256 ? 4 : 1))
k_inv_column(const int32_t *__restrict__ zpart, uint32_t *__restrict__ yres,
             const uint32_t *__restrict__ ua, PrimeSet PS, uint32_t k, uint32_t n) {
    using G = NttGeom<LOGM, LE>;
    constexpr int M = G::M, T = G::T, E = G::E;
    SGFHE_DYN_LDS(uint32_t, lds);
    const int tid = threadIdx.x;
    const uint32_t npr = PS[0].npr;
    const uint32_t c = blockIdx.x & 1u;
    const uint32_t pi = (blockIdx.x >> 1) % npr;
    const uint32_t b = (blockIdx.x >> 1) / npr;
    const PrimeK P = PS[pi];
    const Mod md = mod_of(P);

    int32_t z[1][E];
    const int32_t *zp = zpart + ((((size_t)b * npr + pi) * 4) * 2 + c) * M + E * tid;
#pragma unroll
    for (int h = 0; h < E / 4; h++) {
        int32_t acc[4];
        zpart_sum4<M>(zp, h, acc);
#pragma unroll
        for (int t = 0; t < 4; t++) z[0][4 * h + t] = sred(acc[t], md);
    }
    ntt_inverse<LOGM, 1, LE>(z, lds, P.twi, tid, md);

    // y = x^j P - P
    uint32_t *yb = yres + (((size_t)b * 2 + c) * npr + pi) * M;
    const uint32_t j = ua[(size_t)b * n + k];
    const uint32_t yoff = handover_offset(P);
    lds_store<LOGM, 1, LE, G::STOP>(z, lds, tid);  // own addresses: the thread's last loads
    SGFHE_SYNC();
    constexpr uint32_t LOWMASK = (1u << G::STOP) - 1u;
    const uint32_t s0 = ((uint32_t)tid - j) & (2 * M - 1);
    const uint32_t lowswz = swz<LE>(s0 & LOWMASK);
    const uint32_t h0 = s0 >> G::STOP;
#pragma unroll
    for (int e = 0; e < E; e++) {
        const uint32_t he = h0 + e;
        const uint32_t hipart = (he & (E - 1)) << G::STOP;
        const uint32_t addr = hipart ^ lowswz ^ (G::STOP >= 9 ? 0u : swz_bits<LE>(hipart));
        const int32_t v = (int32_t)lds[addr];
        const int32_t vs = (he & E) ? -v : v;  // x^m = -1
        yb[tid + T * e] = (uint32_t)(vs - z[0][e]) + yoff;
    }
}

// ---- quarter form of the latency kernels (round 4) ------------------------------------------------------
// A call of a few gates is a dependent chain of 3 n launches, each a handful of workgroups on an
// otherwise idle device: what counts is the length of one workgroup's work.  Here each transform of
// m points is cut across four workgroups of m / 32 threads:
//   k_fwd_quarter  (bootstrap, prime, key row, quarter q): reads all four quarters of the digit plane,
//                  forms quarter q of the first two Cooley-Tukey stages (one radix-4 combination per
//                  point: the arithmetic of ntt.h fwd_step4), runs the remaining log2(m) - 2 stages as
//                  an (m / 4)-point transform on the twiddle sub-tree of that quarter (tables twq), and
//                  multiplies with its quarter of the two key polynomials             -> zpart (unchanged layout)
//   k_inv_quarter  (bootstrap, prime, column, quarter q): sums the four partial products of its slots,
//                  applies (x^j - 1) in the NTT domain -- slot s holds the value at psi^(2 brv(s) + 1), so
//                  the factor is psi^(j (2 brv(s) + 1)) - 1, from a table of psi powers -- and runs the first
//                  log2(m) - 2 Gentleman-Sande stages on its quarter                   -> ypart[...][q][m / 4]
//   k_crt_lean1q   one thread per coefficient: the last two inverse stages (a radix-4 combination of the
//                  four partial values per prime, only the output this coefficient needs), then the CRT /
//                  accumulate / flatten of k_crt_lean1.
// No rotation epilogue, no LDS exchange for it, a quarter of the butterflies per workgroup.  Deterministic
// flatten, m >= 4096, up to `split_max` gates (engine.hip); same residues, same digits, same bytes.
template <int LOGM, int LE>
__global__ void __launch_bounds__((NttGeom<LOGM - 2, LE>::T))
k_fwd_quarter(const uint64_t *__restrict__ dig, const int32_t *__restrict__ keyk,
              int32_t *__restrict__ zpart, PrimeSet PS, uint32_t mode) {
    constexpr int LS = LOGM - 2;
    using G = NttGeom<LS, LE>;
    constexpr int M = 1 << LOGM, MS = G::M, T = G::T, E = G::E;
    SGFHE_DYN_LDS(uint32_t, lds);
    const int tid = threadIdx.x;
    const uint32_t npr = PS[0].npr;
    const uint32_t q = blockIdx.x & 3u, ph = (blockIdx.x >> 2) & 3u;
    const uint32_t pi = (blockIdx.x >> 4) % npr, b = (blockIdx.x >> 4) / npr;
    const PrimeK P = PS[pi];
    const Mod md = mod_of(P);
    const int32_t sRd = (mode & MODE_RANDOM) ? P.sRr : P.sR;   // digit offset of the flatten mode
    const uint32_t *dl = digit_lo_plane(dig, (size_t)b * 2 + (ph >> 1), M) + (ph & 1) * M;
    const uint16_t *dh = digit_hi_plane(dig, (size_t)b * 2 + (ph >> 1), M) + (ph & 1) * M;
    const QuarterHead head(q, P);
    int32_t x[1][E];
#pragma unroll
    for (int e = 0; e < E; e++) x[0][e] = head.point<MS>(dl, dh, (uint32_t)tid + (uint32_t)(T * e), P, md, sRd);
    ntt_forward<LS, 1, LE>(x, lds, P.twq + (size_t)q * M, tid, md);
    const int32_t *kp = keyk + ((size_t)pi * 8 + ph * 2) * M + q * MS + E * tid;
    int32_t *zp = zpart + ((((size_t)b * npr + pi) * 4 + ph) * 2) * M + q * MS + E * tid;
    key_row_products<M, E>(x, kp, zp, md);
}

template <int LOGM, int LE>
__global__ void __launch_bounds__((NttGeom<LOGM - 2, LE>::T))
k_inv_quarter(const int32_t *__restrict__ zpart, int32_t *__restrict__ ypart,
              const uint32_t *__restrict__ ua, PrimeSet PS, uint32_t k, uint32_t n) {
    constexpr int LS = LOGM - 2;
    using G = NttGeom<LS, LE>;
    constexpr int M = 1 << LOGM, MS = G::M, T = G::T, E = G::E;
    SGFHE_DYN_LDS(uint32_t, lds);
    const int tid = threadIdx.x;
    const uint32_t npr = PS[0].npr;
    const uint32_t q = blockIdx.x & 3u, c = (blockIdx.x >> 2) & 1u;
    const uint32_t pi = (blockIdx.x >> 3) % npr, b = (blockIdx.x >> 3) / npr;
    const PrimeK P = PS[pi];
    const Mod md = mod_of(P);
    const uint32_t j = ua[(size_t)b * n + k];
    int32_t dfac[E];   // requested first
    rot_factors<LOGM>(dfac, P, j, q, tid);
    int32_t z[1][E];
    const int32_t *zp = zpart + ((((size_t)b * npr + pi) * 4) * 2 + c) * M + q * MS + E * tid;
#pragma unroll
    for (int h = 0; h < E / 4; h++) {
        int32_t acc[4];
        zpart_sum4<M>(zp, h, acc);
#pragma unroll
        for (int t = 0; t < 4; t++)
            z[0][4 * h + t] = smont(acc[t], rot_centre(dfac[4 * h + t], P, md), md);   // < 0.19 + 0.5 = 0.69 * 2^29
    }
    ntt_inverse<LS, 1, LE>(z, lds, P.twq + (size_t)q * M + MS, tid, md);   // natural order inside the quarter, |.| < 1.4 * 2^29
    int32_t *yb = ypart + ((((size_t)b * 2 + c) * npr + pi) * 4 + q) * MS;
#pragma unroll
    for (int e = 0; e < E; e++) yb[tid + T * e] = z[0][e];
}

// k_fwd_quarter and k_inv_quarter in one launch (round 4, second step): a quarter of the slots is closed
// under everything between the radix-4 head of the forward transforms and the radix-4 tail of the inverse
// ones, so one workgroup per (bootstrap, prime, quarter) can go from digit planes to partial products
// without a hand-over through memory -- one dependent launch less per iteration of the chain.  Two groups
// of m / 32 threads: group g transforms key rows 2 g and 2 g + 1 side by side (the two digits of one
// accumulator polynomial), forms its share of both product columns with 64-bit multiply-adds,
//   w_c = REDC(u_2g K[2g][c] + u_2g+1 K[2g+1][c]),   |.| < (2 * 3.95 * 2^29 * 2^28) / 2^32 + p / 2 < 0.99 * 2^29,
// keeps w_g, hands w_(1-g) to the other group through LDS, and runs the inverse quarter of column g on
// (w_g + w'_g) (psi^(j (2 brv(s) + 1)) - 1): |sum| < 1.98 * 2^29, after the Montgomery product < 0.63 * 2^29.
// Same residues modulo every prime as the two-launch form, hence the same digits.
//   lds: [group][2][m/4] transform exchange, then [2][m/4] hand-over  (6 m/4 words)
template <int LOGM, int LE>
__global__ void __launch_bounds__((2 * NttGeom<LOGM - 2, LE>::T))
k_ext_quarter(const uint64_t *__restrict__ dig, const int32_t *__restrict__ keyk, int32_t *__restrict__ ypart,
              const uint32_t *__restrict__ ua, PrimeSet PS, uint32_t mode, uint32_t k, uint32_t n) {
    constexpr int LS = LOGM - 2;
    using G = NttGeom<LS, LE>;
    constexpr int M = 1 << LOGM, MS = G::M, T = G::T, E = G::E;
    SGFHE_DYN_LDS(uint32_t, lds);
    const uint32_t g = (uint32_t)threadIdx.x / (uint32_t)T;          // key rows 2 g, 2 g + 1; product column g
    const int tl = (int)((uint32_t)threadIdx.x & (uint32_t)(T - 1));
    const uint32_t npr = PS[0].npr;
    const uint32_t q = blockIdx.x & 3u;
    const uint32_t pi = (blockIdx.x >> 2) % npr, b = (blockIdx.x >> 2) / npr;
    const PrimeK P = PS[pi];
    const Mod md = mod_of(P);
    const int32_t sRd = (mode & MODE_RANDOM) ? P.sRr : P.sR;
    uint32_t *const glds = lds + (size_t)g * 2 * MS;
    int32_t *const hand = reinterpret_cast<int32_t *>(lds) + 4 * MS;

    // requested first: the rotation factors of column g's slots (a gather behind the load of j) and the key
    const uint32_t j = ua[(size_t)b * n + k];
    int32_t dfac[E];
    rot_factors<LOGM>(dfac, P, j, q, tl);
    int4 kk[2][2][E / 4];                                           // [row of the pair][column][..]
    {
        const int32_t *kp = keyk + ((size_t)pi * 8 + g * 4) * M + q * MS + E * tl;
#pragma unroll
        for (int r = 0; r < 2; r++)
#pragma unroll
            for (int c = 0; c < 2; c++)
#pragma unroll
                for (int h = 0; h < E / 4; h++) kk[r][c][h] = reinterpret_cast<const int4 *>(kp + (size_t)(r * 2 + c) * M)[h];
    }
    const QuarterHead head(q, P);   // of both rows
    int32_t x[2][E];
#pragma unroll
    for (int r = 0; r < 2; r++) {
        const uint32_t *dl = digit_lo_plane(dig, (size_t)b * 2 + g, M) + r * M;
        const uint16_t *dh = digit_hi_plane(dig, (size_t)b * 2 + g, M) + r * M;
#pragma unroll
        for (int e = 0; e < E; e++) x[r][e] = head.point<MS>(dl, dh, (uint32_t)tl + (uint32_t)(T * e), P, md, sRd);
    }
    ntt_forward<LS, 2, LE>(x, glds, P.twq + (size_t)q * M, tl, md);
    // products of the pair, both columns; the other group's column goes to the hand-over area
    int32_t own[E];
#pragma unroll
    for (int h = 0; h < E / 4; h++) {
        int32_t w[2][4];
#pragma unroll
        for (int c = 0; c < 2; c++) {
            const int4 a4 = kk[0][c][h], b4 = kk[1][c][h];
            const int32_t ka[4] = {a4.x, a4.y, a4.z, a4.w}, kb[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
            for (int t = 0; t < 4; t++)
                w[c][t] = sredc((int64_t)x[0][4 * h + t] * ka[t] + (int64_t)x[1][4 * h + t] * kb[t], md);
        }
        const int4 w0 = make_int4(w[0][0], w[0][1], w[0][2], w[0][3]), w1 = make_int4(w[1][0], w[1][1], w[1][2], w[1][3]);
        const int4 keep = g ? w1 : w0, give = g ? w0 : w1;
        own[4 * h] = keep.x; own[4 * h + 1] = keep.y; own[4 * h + 2] = keep.z; own[4 * h + 3] = keep.w;
        reinterpret_cast<int4 *>(hand + (size_t)(1u - g) * MS + E * tl)[h] = give;
    }
    SGFHE_SYNC();   // hand-over written; every wave is through its forward exchanges
    int32_t z[1][E];
#pragma unroll
    for (int h = 0; h < E / 4; h++) {
        const int4 o = reinterpret_cast<const int4 *>(hand + (size_t)g * MS + E * tl)[h];
        const int32_t ov[4] = {o.x, o.y, o.z, o.w};
#pragma unroll
        for (int t = 0; t < 4; t++)
            z[0][4 * h + t] = smont(own[4 * h + t] + ov[t], rot_centre(dfac[4 * h + t], P, md), md);
    }
    ntt_inverse<LS, 1, LE>(z, glds, P.twq + (size_t)q * M + MS, tl, md);
    int32_t *yb = ypart + ((((size_t)b * 2 + g) * npr + pi) * 4 + q) * MS;
#pragma unroll
    for (int e = 0; e < E; e++) yb[tl + T * e] = z[0][e];
}

// One thread per coefficient: quarter_residues (the last two inverse stages), then crt_lean_one.
template <int NP, int NL>
__global__ void __launch_bounds__(256)
k_crt_lean1q(const int32_t *__restrict__ ypart, uint64_t *__restrict__ dig, PrimeSet PS,
             const CrtLean *__restrict__ K, uint32_t total, uint32_t logm) {
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const uint32_t M = 1u << logm;
    const uint32_t i = t & (M - 1);
    const uint32_t bc = t >> logm;
    uint32_t y[NP];
    quarter_residues<NP>(ypart, PS, bc, i, logm, y);
    const ulonglong2 d = load_digits(dig, bc, i, M);
    uint64_t lo, hi;
    crt_lean_one<NP, NL>(y, d.x, d.y, K, lo, hi);
    store_digits(dig, bc, i, M, lo, hi);
}

// ---- k_init -------------------------------------------------------------------------------------
// u = lwe1 + lwe2 (fhe.jl:566); a = 0 (fhe.jl:570); b = x^(-u.b) t DQ_tilde (fhe.jl:572-573) with
// t = initial_poly (fhe.jl:535-548): +1 on [0, Dr), 0 at Dr, -1 on (Dr, m).  Every coefficient of
// b is 0, +DQ_tilde or -DQ_tilde, so the three possible digit pairs are precomputed.
// One thread per (bootstrap of the padded chunk, coefficient).
template <bool ROWS = false>
__global__ void __launch_bounds__(256)
k_init(const uint64_t *__restrict__ a1, const uint64_t *__restrict__ b1,
       const uint64_t *__restrict__ a2, const uint64_t *__restrict__ b2,
       uint64_t *__restrict__ dig, uint32_t *__restrict__ ua, const CrtConst *__restrict__ CC,
       uint32_t nvalid, uint32_t chunk, uint32_t n, uint32_t logm, uint32_t mode, RndArgs ra,
       const uint32_t *__restrict__ lut = nullptr) {
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    const uint32_t M = 1u << logm;
    if (t >= chunk * M) return;
    const uint32_t i = t & (M - 1);
    const uint32_t b = t >> logm;
    const uint32_t rmask = 2 * M - 1;  // r = 2 m
    const bool valid = b < nvalid;
    // a LUT row of the chunk (lut: the descriptor from this chunk's first row on, or nullptr) starts at amplitude A0
    const bool low = lut && valid && (lut[b] & LUT_ROW);
    if (i < n) ua[(size_t)b * n + i] =
        valid ? (uint32_t)((a1[(size_t)b * n + i] + a2[(size_t)b * n + i]) & rmask) : 0u;
    int tv = 0;
    if (valid) {
        const uint32_t ub = (uint32_t)((b1[b] + b2[b]) & rmask);
        const uint32_t Dr = M / 2;  // r / 4
        const uint32_t src = (i + ub) & rmask;
        const uint32_t s = src & (M - 1);
        tv = s < Dr ? 1 : (s == Dr ? 0 : -1);
        if (src & M) tv = -tv;
    }
    if (mode & MODE_RANDOM) {  // flatten(rng, .) of a = 0 and of b in {0, +-DQ_tilde}
        const u128 Q = CC->Q;
        const u128 offr = CC->offneg_rnd ? Q - CC->offneg_rnd : 0;
        const u128 amp = low ? CC->DQL : CC->DQ;
        u128 xb = offr + (tv > 0 ? amp : (tv < 0 ? Q - amp : 0));
        if (xb >= Q) xb -= Q;
        ChaChaKey key;
        uint32_t cz, cw;
        rnd_stream<ROWS>(ra, b, key, cz, cw);
        const ulonglong2 ea = random_digits(offr, CC, key, make_uint4(i, 0u, cz, cw));
        const ulonglong2 eb = random_digits(xb, CC, key, make_uint4(M + i, 0u, cz, cw));
        store_digits(dig, (size_t)b * 2 + 0, i, M, ea.x, ea.y, (mode & MODE_WIDE) != 0);
        store_digits(dig, (size_t)b * 2 + 1, i, M, eb.x, eb.y, (mode & MODE_WIDE) != 0);
        return;
    }
    store_digits(dig, (size_t)b * 2 + 0, i, M, CC->dig0.x, CC->dig0.y);
    ulonglong2 d = CC->dig0;
    if (valid) d = tv > 0 ? (low ? CC->digPL : CC->digP) : (tv < 0 ? (low ? CC->digNL : CC->digN) : CC->dig0);
    store_digits(dig, (size_t)b * 2 + 1, i, M, d.x, d.y);
}

// ---- k_final ------------------------------------------------------------------------------------
// LWE extraction (fhe.jl:585-592, extract :237-244 in its i >= n branch) and ModRed
// (fhe.jl:616-618,644-648; rescale utils.jl:78-92).  One thread per (bootstrap, t in [0, n]).
__device__ __forceinline__ u128 acc_from_digits(ulonglong2 d, const CrtConst *CC,
                                                uint32_t mode = 0) {
    if (mode & MODE_RANDOM)  // digits up to 4 B: reduce properly
        return mod_wide((u128)d.y * (uint64_t)CC->B + d.x + CC->offneg_rnd, CC->Q, CC->invQ, nullptr);
    u128 x = (u128)d.y * (uint64_t)CC->B + d.x + CC->offneg;
    if (x >= CC->Q) x -= CC->Q;
    return x;
}
__device__ __forceinline__ uint64_t modred(u128 x, const CrtConst *CC) {
    const u128 num = x << CC->logr;  // x * r
    uint64_t q;
    const u128 rem = mod_wide(num, CC->Q, CC->invQ, &q);
    if (rem >= CC->roundthr) {
        q += 1;
        if (q == (1ull << CC->logr)) q = 0;
    }
    return q;
}
__global__ void __launch_bounds__(256)
k_final(const uint64_t *__restrict__ dig, uint64_t *__restrict__ out,
        const CrtConst *__restrict__ CC, uint32_t nvalid, uint32_t n, uint32_t logm, uint32_t raw,
        uint32_t mode) {
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= nvalid * (n + 1)) return;
    const uint32_t M = 1u << logm;
    const uint32_t b = t / (n + 1), e = t % (n + 1);
    const size_t ba = (size_t)b * 2 + 0, bb = (size_t)b * 2 + 1;
    const u128 Q = CC->Q;
    const bool wide = (mode & MODE_WIDE) != 0;
    u128 va, vo;
    if (e < n) {
        va = acc_from_digits(load_digits(dig, ba, 3 * M / 4 - e, M, wide), CC, mode);
        const u128 w = acc_from_digits(load_digits(dig, ba, M / 4 - e, M, wide), CC, mode);
        vo = w ? Q - w : 0;
    } else {
        va = CC->DQ + acc_from_digits(load_digits(dig, bb, 3 * M / 4, M, wide), CC, mode);
        if (va >= Q) va -= Q;
        const u128 w = acc_from_digits(load_digits(dig, bb, M / 4, M, wide), CC, mode);
        vo = CC->DQ >= w ? CC->DQ - w : CC->DQ + Q - w;
    }
    const u128 vx = vo >= va ? vo - va : vo + Q - va;
    const size_t stride = n + 1;
    if (raw) {
        ulonglong2 *o = reinterpret_cast<ulonglong2 *>(out) + (size_t)b * 3 * stride + e;
        o[0] = make_ulonglong2((uint64_t)va, (uint64_t)(va >> 64));
        o[stride] = make_ulonglong2((uint64_t)vo, (uint64_t)(vo >> 64));
        o[2 * stride] = make_ulonglong2((uint64_t)vx, (uint64_t)(vx >> 64));
    } else {
        uint64_t *o = out + (size_t)b * 3 * stride + e;
        o[0] = modred(va, CC);
        o[stride] = modred(vo, CC);
        o[2 * stride] = modred(vx, CC);
    }
}

// ---- k_final_lut --------------------------------------------------------------------------------
// The extraction of a LUT row (sgfhe_bootstrap_lut_batch, include/sgfhe_hip.h): the accumulator started at A0, so
// P(acc, c) = A0 T(c + phase) with T the antiperiodic test polynomial, and the coefficient at
// c(j) = 3 Dr - (2 j - 1) Dr/8 is the step "+A0 for s >= j, -A0 below" of the input sum s = phase / (Dr/4).  The truth
// table is the +-1 combination of the steps at its transitions (sigma(j) != sigma(j - 1), j in 1..8, sigma(8) =
// -sigma(0)): base = A0 [b word only] + sum_i kappa_i P(acc, c(j_i) - e), kappa_i = -sigma(0) (-1)^i, and the three
// rows are 4, 2 and 1 times the base: the table's bit at the codewords Dr, Dr/2, Dr/4.
// One thread per (row of the chunk, word e in [0, n]) computes the base once and writes the three rows; rows of the
// chunk that are not LUT rows are left alone (k_final has written them).  The table decode is uniform over a row;
// consecutive threads read consecutive (descending) coefficients.  c(j) - e is taken mod 2 m: c(j) >= m for j <= 4
// (the negated half), and c(4) - m = Dr/8 < n, so the index does wrap below 0 into the other half, negating again.
// P(acc, c(j) - e) of one thread, j in 1..8: the coefficient index with its wrap, and the negation that goes with it.
__device__ __forceinline__ u128 lut_coeff(const uint64_t *__restrict__ dig, size_t bc, uint32_t shift, uint32_t j,
                                          uint32_t M, bool wide, const CrtConst *CC, uint32_t mode) {
    const uint32_t c = 3 * (M / 2) - (2 * j - 1) * (M / 16);          // below 3 m / 2
    uint32_t idx = (c + 2 * M - shift) & (2 * M - 1);
    const bool neg = idx >= M;
    if (neg) idx -= M;
    const u128 w = acc_from_digits(load_digits(dig, bc, idx, M, wide), CC, mode);
    return neg && w ? CC->Q - w : w;
}

// bit j of the result marks a transition of the table at j in 1..8 (sigma(8) = -sigma(0))
__device__ __forceinline__ uint32_t lut_edges(uint32_t table) {
    const uint32_t ext = (table & 0xFFu) | ((~table & 1u) << 8);   // bit j is sigma(j) for j in 0..8
    return (ext ^ (ext << 1)) & 0x1FEu;
}

// The base LWE word of one table: A0 on the b word only, then kappa_i coeff(j_i) over the table's transitions, folded
// after every add.  coeff(j) is P(acc, c(j) - e): k_final_lut loads it, k_final_lut_multi has it in a register.
template <class F>
__device__ __forceinline__ u128 lut_base(uint32_t table, bool bword, const CrtConst *CC, F coeff) {
    const u128 Q = CC->Q;
    const uint32_t edge = lut_edges(table);
    bool minus = (table & 1u) != 0;      // kappa_0 = -sigma(0)
    u128 v = bword ? CC->DQL : (u128)0;
#pragma unroll
    for (uint32_t j = 1; j <= 8; j++) {
        if (!((edge >> j) & 1u)) continue;
        u128 w = coeff(j);
        if (minus) w = w ? Q - w : 0;
        v += w;
        if (v >= Q) v -= Q;
        minus = !minus;
    }
    return v;
}

// The three scaled rows of a base word v: 4 v, 2 v and v mod Q at `o`, `o + stride`, `o + 2 stride` -- 16-byte
// residues when raw (`o` then counts residues), through ModRed otherwise.
__device__ __forceinline__ void lut_store_rows(uint64_t *__restrict__ o, size_t stride, u128 v, uint32_t raw,
                                               const CrtConst *CC) {
    const u128 Q = CC->Q;
    u128 v2 = v + v;
    if (v2 >= Q) v2 -= Q;
    u128 v4 = v2 + v2;
    if (v4 >= Q) v4 -= Q;
    if (raw) {
        ulonglong2 *o2 = reinterpret_cast<ulonglong2 *>(o);
        o2[0] = make_ulonglong2((uint64_t)v4, (uint64_t)(v4 >> 64));
        o2[stride] = make_ulonglong2((uint64_t)v2, (uint64_t)(v2 >> 64));
        o2[2 * stride] = make_ulonglong2((uint64_t)v, (uint64_t)(v >> 64));
    } else {
        o[0] = modred(v4, CC);
        o[stride] = modred(v2, CC);
        o[2 * stride] = modred(v, CC);
    }
}

__global__ void __launch_bounds__(256)
k_final_lut(const uint64_t *__restrict__ dig, uint64_t *__restrict__ out, const CrtConst *__restrict__ CC,
            const uint32_t *__restrict__ lut, uint32_t nvalid, uint32_t n, uint32_t logm, uint32_t raw, uint32_t mode) {
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= nvalid * (n + 1)) return;
    const uint32_t M = 1u << logm;
    const uint32_t b = t / (n + 1), e = t % (n + 1);
    const uint32_t word = lut[b];
    if (!(word & LUT_ROW)) return;
    const bool wide = (mode & MODE_WIDE) != 0;
    const size_t bc = (size_t)b * 2 + (e < n ? 0 : 1);
    const uint32_t shift = e < n ? e : 0u;
    const u128 v = lut_base(word, e == n, CC,
                            [&](uint32_t j) { return lut_coeff(dig, bc, shift, j, M, wide, CC, mode); });
    const size_t stride = n + 1;
    lut_store_rows(out + ((size_t)b * 3 * stride + e) * (raw ? 2 : 1), stride, v, raw, CC);
}

// (slot references of the circuit tables, described with the gate circuits below)
constexpr uint32_t CIRC_REF_FALSE = 0x7FFFFFFFu, CIRC_REF_NOT = 0x80000000u, CIRC_SLOT_NONE = 0xFFFFFFFFu;
// A table that is run-time data (sgfhe_circuit_create_data, circuit.h CIRC_DATA): bit 24 of a LUT node's kind word, whose
// bits 8..23 then hold the plane, and of a family entry, whose low 16 bits then hold it.  The table of instance `inst`
// is the byte data[plane * instances + inst] of the run's planes.
constexpr uint32_t CIRC_TABLE_DATA = 0x01000000u;

// ---- k_final_lut_multi --------------------------------------------------------------------------
// A LUT family: several truth tables on the accumulator of one row.  The k-loop does not know the table; a further
// table costs one more +-1 combination of the same eight coefficients.
// One thread per (row of the chunk, word e in [0, n]), as k_final_lut.  The thread reconstructs P(acc, c(j) - e) once
// for every j that is a transition of some table of its row (lut_coeff: the index wrap and the double negation are
// k_final_lut's), keeps the eight values in registers -- the loops over j are unrolled, so the array is never indexed
// at run time -- and then forms lut_base and the three scaled rows table by table: the bytes of k_final_lut for that
// table.  The table list is uniform over a row, and for every table consecutive threads store consecutive words:
// coalesced 8-byte stores, or 16-byte ones when raw.  The kernel is bound by those stores, 3 words a table and thread.
// The primitive (sgfhe_bootstrap_lut_multi_batch, CIRC = false): the row's tables are tables[row][0 .. n_tables), and
// the rows go to out [row][n_tables][3][n + 1], both from the chunk's first row on.
// A level call of a circuit (sgfhe_circuit_create_lut_multi, CIRC = true): chunk row b is row R = row0 + b of its
// level, node node0 + R / instances of the plan at instance R % instances (circ_row: a plan with lane masks decodes
// the row through its pairs); the live siblings of that node are the
// entries start[node] .. start[node + 1] of {table, slot of wire +0, +1, +2} (CircuitPlan::fam_entry), and wire w goes
// to its slot of the wire table `out` ([slot][instances][n + 1]) -- as the ModRed word, in an un-reduced call too;
// a wire nothing reads has no slot (CIRC_SLOT_NONE) and is not formed.  The node's own table leaves through k_final_lut.
// An entry may name a plane instead of a table (CIRC_TABLE_DATA): the thread resolves it with one byte load at its
// instance, uniform over the row, before the entry's table is used at all (lut_fam_table).
// The rows of a level call of a plan with lane masks (sgfhe_circuit_create_masked): the level's (node, lane) pairs --
// `node` the rank in the level -- with per = instances / group; row R of the level is pair R / per at group R % per,
// instance (R % per) * group + lane.  `node` NULL: a plan without masks, rank R / instances at instance R % instances.
// The two entries are 4-byte loads at an address that is uniform over a row, and per-lane loads for the reason written
// at circ_ref_word: a wave may straddle two rows, so they are not wave-uniform broadcasts.
struct CircPairs {
    const uint32_t *node = nullptr, *lane = nullptr;
    uint32_t per = 0, group = 0;
};
// row R of a level -> (rank of its node in the level, instance)
__device__ __forceinline__ void circ_row(const CircPairs &X, uint32_t R, uint32_t instances, uint32_t &rank,
                                         uint32_t &inst) {
    if (!X.node) {
        rank = R / instances, inst = R % instances;
        return;
    }
    const uint32_t p = R / X.per;
    rank = X.node[p];
    inst = (R % X.per) * X.group + X.lane[p];
}

struct LutTables {
    const uint8_t *tables;            // the primitive
    uint32_t n_tables;
    const uint32_t *start, *entry;    // a level call
    uint32_t node0, row0, instances;
    const uint8_t *data;              // a level call of a plan with planes: [n_planes][instances]
    CircPairs pairs;                  // a level call of a plan with lane masks (an unmasked leader: all its lanes)
};
__device__ __forceinline__ uint32_t lut_fam_table(const LutTables &T, uint32_t i, uint32_t inst) {
    const uint32_t w = T.entry[4 * i];
    return w & CIRC_TABLE_DATA ? T.data[(size_t)(w & 0xFFFFu) * T.instances + inst] : w;
}
__device__ __forceinline__ void lut_coeffs(u128 (&P)[8], uint32_t need, const uint64_t *__restrict__ dig, size_t bc,
                                           uint32_t shift, uint32_t M, bool wide, const CrtConst *CC, uint32_t mode) {
#pragma unroll
    for (uint32_t j = 1; j <= 8; j++)
        P[j - 1] = (need >> j) & 1u ? lut_coeff(dig, bc, shift, j, M, wide, CC, mode) : (u128)0;
}
template <bool CIRC>
__global__ void __launch_bounds__(256)
k_final_lut_multi(const uint64_t *__restrict__ dig, uint64_t *__restrict__ out, const CrtConst *__restrict__ CC,
                  LutTables T, uint32_t nvalid, uint32_t n, uint32_t logm, uint32_t raw, uint32_t mode) {
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= nvalid * (n + 1)) return;
    const uint32_t M = 1u << logm;
    const uint32_t b = t / (n + 1), e = t % (n + 1);
    const bool wide = (mode & MODE_WIDE) != 0;
    const size_t bc = (size_t)b * 2 + (e < n ? 0 : 1);
    const uint32_t shift = e < n ? e : 0u;
    const size_t stride = n + 1;
    uint32_t need = 0;                   // bit j: some table of the row has a transition at j
    u128 P[8];
    if constexpr (CIRC) {
        uint32_t rank, inst;
        circ_row(T.pairs, T.row0 + b, T.instances, rank, inst);
        const uint32_t node = T.node0 + rank;
        const uint32_t s0 = T.start[node], s1 = T.start[node + 1];
        if (s0 == s1) return;
        for (uint32_t i = s0; i < s1; i++) need |= lut_edges(lut_fam_table(T, i, inst));
        lut_coeffs(P, need, dig, bc, shift, M, wide, CC, mode);
        const u128 Q = CC->Q;
        for (uint32_t i = s0; i < s1; i++) {
            u128 v = lut_base(lut_fam_table(T, i, inst), e == n, CC, [&](uint32_t j) { return P[j - 1]; });
#pragma unroll
            for (int w = 2; w >= 0; w--) {   // wire +2 is the base word, +1 twice and +0 four times it
                const uint32_t slot = T.entry[4 * i + 1 + w];
                if (slot != CIRC_SLOT_NONE) out[((size_t)slot * T.instances + inst) * stride + e] = modred(v, CC);
                v += v;
                if (v >= Q) v -= Q;
            }
        }
    } else {
        const uint8_t *tab = T.tables + (size_t)b * T.n_tables;
        for (uint32_t i = 0; i < T.n_tables; i++) need |= lut_edges(tab[i]);
        lut_coeffs(P, need, dig, bc, shift, M, wide, CC, mode);
        uint64_t *o = out + (((size_t)b * T.n_tables) * 3 * stride + e) * (raw ? 2 : 1);
        for (uint32_t i = 0; i < T.n_tables; i++, o += 3 * stride * (raw ? 2 : 1)) {
            const u128 v = lut_base(tab[i], e == n, CC, [&](uint32_t j) { return P[j - 1]; });
            lut_store_rows(o, stride, v, raw, CC);
        }
    }
}

// ---- gate circuits (sgfhe_circuit_run, csrc/circuit.h) ---------------------------------------------
// Memory-bound copies of rows of n + 1 uint64 words (a[0..n) then b) between the wire table
// ([slot][instances][n + 1]) and the staging of one bootstrap call, one thread per word: consecutive
// threads touch consecutive words of a row, so loads and stores are coalesced 8-byte accesses (rows
// are not 16-byte aligned).  Row R of a level is node rank R / instances, instance R % instances -- or, in a plan
// with lane masks, what circ_row makes of the level's pairs (`X`, the last parameter of every kernel that decodes a row).
// A slot reference is a slot number, or CIRC_FALSE (the trivial LWE (0, 0)), plus CIRC_NOT:
// NOT w = enc_trivial(true) - w (fhe.jl:221-223,669-670), a -> -a mod r, b -> (Dr - b) mod r.

// `one`: the codeword of the wire, b of its trivial TRUE -- Dr = r / 4 everywhere but at positions 0 and 1 of a LUT node,
// which read wires at Dr/4 and Dr/2.
__device__ __forceinline__ uint64_t circ_word(const uint64_t *__restrict__ wires, uint32_t ref, size_t inst_row,
                                              uint32_t e, uint32_t n, uint64_t r, uint64_t one) {
    // inst_row = slot * instances + instance (not read for the constant)
    const uint64_t v = (ref & ~CIRC_REF_NOT) == CIRC_REF_FALSE ? 0ull : wires[inst_row * (n + 1) + e];
    if (!(ref & CIRC_REF_NOT)) return v;
    return ((e < n ? 0ull : one) + r - v) & (r - 1);
}

// A lane-shifted reference (sgfhe_circuit_create_lanes): instances form consecutive groups of `group`, and the
// reference reads row inst + d of its slot where the lane (inst % group) + d stays inside the group, the constant
// FALSE elsewhere (NOT applied afterwards, so a negated reference fills with TRUE).  The lane sum is signed and 64 bits
// wide -- d < 0 must not wrap -- and the test is uniform over a row, so a wave diverges only where it straddles rows.
// instances is a multiple of group (checked before a run is queued): row inst + d is inside the slot.
// A routed reference (sgfhe_circuit_create_routed; `rho` its table of `group` entries, NULL for none, and then d is 0)
// reads lane rho[inst % group] of its own group in place of lane + d: the constant where the entry is negative (the
// planner admits -1 and [0, group) only), row inst - inst % group + rho[..] otherwise.  The entry is one 4-byte load
// at an address that is uniform over a row, as the group test is; the source row stays a coalesced 8-byte access.
// It is a per-lane load on purpose: rows are n + 1 words, so a wave may straddle two rows and the entry is uniform over
// a row, not over a wave -- broadcasting the first lane's entry would read the wrong lane past the row's end.  The lanes
// of a row hit one cache line.
// One list of references of a plan on the device -- the terms of the node table, the outputs, the registers' next
// states: reference i is the slot reference ref[i] at the lane shift shift[i], or through the table of its route index
// route[i] -- k >= 1 is table k - 1 of `routes` [n_routes][group], 0 none; `route` and `routes` are both NULL in a plan
// without route tables.
struct CircRefs {
    const uint32_t *ref;
    const int32_t *shift;
    const uint32_t *route;
    const int32_t *routes;
    uint32_t group;
};

// word e of reference i of `refs` at instance `inst`; `one` is the codeword NOT is taken at
__device__ __forceinline__ uint64_t circ_ref_word(const uint64_t *__restrict__ wires, const CircRefs &refs, size_t i,
                                                  uint32_t instances, uint32_t inst, uint32_t e, uint32_t n, uint64_t r,
                                                  uint64_t one) {
    uint32_t ref = refs.ref[i];
    const int32_t d = refs.shift[i];
    const uint32_t k = refs.route ? refs.route[i] : 0u;
    const int32_t *rho = k ? refs.routes + (size_t)(k - 1) * refs.group : nullptr;
    const uint32_t own = inst % refs.group;
    const int64_t lane = rho ? (int64_t)rho[own] : (int64_t)own + d;
    if (lane < 0 || lane >= (int64_t)refs.group) ref = CIRC_REF_FALSE | (ref & CIRC_REF_NOT);
    const size_t src = (size_t)((int64_t)(inst - own) + lane);   // (not read for the constant)
    return circ_word(wires, ref, (size_t)(ref & ~CIRC_REF_NOT) * instances + src, e, n, r, one);
}

// The node table of a plan on the device (CircuitPlan::node_kind ..): one CSR over the live nodes and the pack stage's
// pseudo-level, node k's terms term_start[k] .. term_start[k + 1] of `terms` and `weight`.
struct CircNodes {
    const uint32_t *kind, *start;
    const int32_t *weight;
    CircRefs terms;
};

// The staged inputs of one call, a1 / a2 [rows][n], b1 / b2 [rows]: rows row0 .. row0 + rows of the level whose first
// node is `node0` of the table.  A classic node (kind 0) writes (a1, a2) = (X, Y), its two terms.  A sum node writes
// a1 = U = the sum of w X over its terms mod r and a2 = 0 -- the bootstrap adds its two inputs first, so (U, 0) gives
// what (X + Y, Z) gives: the rotation is by the phase of the sum, the AND row of three unit weights is MAJ(X, Y, Z), the
// OR row "one or two true", and LOW = U - 2 HI over Z_r needs no bootstrap (k_circ_xor3).  One thread per word of a row
// and BOTH outputs; the node decode and the term range are uniform over a row, every load is a coalesced 8-byte access
// along a (shifted) source row.  The sum runs in wrapping uint64 arithmetic with a signed multiply (w in {-2, -1, 1, 2})
// and is reduced with one mask: r is a power of two (at most 2^15), so 2^64 is a multiple of it, and 64 terms of weight
// 2 stay far below 2^64 anyway.  A plan without lane groups has group 1 and no shift but 0.
// A LUT node (kind 2, its table in bits 8..15 of the kind word; sgfhe_circuit_create_lut) writes a1 = U = X0 + X1 + X2
// and a2 = 0 as a sum node of unit weights does, but position i reads a wire at the codeword Dr >> (2 - i), so NOT at
// position i is b -> (Dr >> (2 - i)) - b.  `lutw` (NULL for a call without LUT nodes): the call's LUT descriptor, one
// word per row, LUT_ROW | table for the rows of a LUT node and 0 for the others (bootstrap_device's LutDesc).  The
// table of a data LUT node (CIRC_TABLE_DATA) is the byte of its plane at the row's own instance, data[plane * instances +
// inst]: one load, by the thread that writes the word.
__global__ void __launch_bounds__(256)
k_circ_gather(const uint64_t *__restrict__ wires, CircNodes nodes, uint32_t node0, uint64_t *__restrict__ a1,
              uint64_t *__restrict__ b1, uint64_t *__restrict__ a2, uint64_t *__restrict__ b2, uint32_t row0,
              uint32_t rows, uint32_t instances, uint32_t n, uint64_t r, uint32_t *__restrict__ lutw = nullptr,
              const uint8_t *__restrict__ data = nullptr, CircPairs X = {}) {
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= rows * (n + 1)) return;
    const uint32_t lr = t / (n + 1), e = t % (n + 1), R = row0 + lr;
    uint32_t rank, inst;
    circ_row(X, R, instances, rank, inst);
    const uint32_t k = node0 + rank;
    auto read = [&](uint32_t i, uint64_t one) -> uint64_t {
        return circ_ref_word(wires, nodes.terms, i, instances, inst, e, n, r, one);
    };
    const uint32_t t0 = nodes.start[k], t1 = nodes.start[k + 1];
    const uint32_t kw = nodes.kind[k], kd = kw & 0xFFu;
    uint64_t u = 0, v = 0;
    if (kd == 0) {
        u = read(t0, r / 4);
        v = read(t0 + 1, r / 4);
    } else if (kd == 2) {
        u = (read(t0, r / 16) + read(t0 + 1, r / 8) + read(t0 + 2, r / 4)) & (r - 1);
    } else {
        for (uint32_t i = t0; i < t1; i++) u += (uint64_t)((int64_t)nodes.weight[i] * (int64_t)read(i, r / 4));
        u &= r - 1;
    }
    if (e < n) {
        a1[(size_t)lr * n + e] = u;
        a2[(size_t)lr * n + e] = v;
    } else {
        b1[lr] = u;
        b2[lr] = v;
        if (lutw) {
            uint32_t tb = (kw >> 8) & 0xFFu;
            if (kw & CIRC_TABLE_DATA) tb = data[(size_t)((kw >> 8) & 0xFFFFu) * instances + inst];
            lutw[lr] = kd == 2 ? LUT_ROW | tb : 0u;
        }
    }
}

// LOW of the sum nodes of a call (XOR3 of a three-input node; node_kind [nodes] of the level marks them), after its
// k-loop and before anything reads its result rows
// [rows][3][n + 1]: row 2 = a1 + a2 - 2 row 0 mod r, word by word, b included -- a1 + a2 is the sum U as the bootstrap
// consumed it (the staging is not written between the gather and here), row 0 the reduced HI.  The rows of classic
// nodes are left alone.  One thread per word, as the gather.
__global__ void __launch_bounds__(256)
k_circ_xor3(uint64_t *__restrict__ res, const uint32_t *__restrict__ node_kind, const uint64_t *__restrict__ a1,
            const uint64_t *__restrict__ b1, const uint64_t *__restrict__ a2, const uint64_t *__restrict__ b2,
            uint32_t row0, uint32_t rows, uint32_t instances, uint32_t n, uint64_t r, CircPairs X = {}) {
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= rows * (n + 1)) return;
    const uint32_t lr = t / (n + 1), e = t % (n + 1);
    uint32_t rank, inst;
    circ_row(X, row0 + lr, instances, rank, inst);
    if ((node_kind[rank] & 0xFFu) != 1) return;   // a sum node's rows only
    const uint64_t s = e < n ? a1[(size_t)lr * n + e] + a2[(size_t)lr * n + e] : b1[lr] + b2[lr];
    uint64_t *o = res + (size_t)lr * 3 * (n + 1) + e;
    o[2 * (size_t)(n + 1)] = (s - 2 * o[0]) & (r - 1);
}

// The same after k_circ_scatter_raw, for a call whose rows stay un-reduced (16-byte residues over Z_Q): the XOR3 words
// over Z_r go straight into the wire's slot, over the ModRed of the meaningless XOR row the scatter put there, with
// row 0 reduced by the device function of k_final -- the words the reduced call gives.  The raw rows are not touched
// (an output naming an XOR3 wire is refreshed or lifted, never direct).  One workgroup per row, as k_circ_scatter_raw.
__global__ void __launch_bounds__(256)
k_circ_xor3_raw(const ulonglong2 *__restrict__ res, const uint32_t *__restrict__ node_kind,
                const uint32_t *__restrict__ out_slot, uint64_t *__restrict__ wires, const uint64_t *__restrict__ a1,
                const uint64_t *__restrict__ b1, const uint64_t *__restrict__ a2, const uint64_t *__restrict__ b2,
                const CrtConst *__restrict__ CC, uint32_t row0, uint32_t instances, uint32_t n, uint64_t r,
                CircPairs X = {}) {
    const uint32_t lr = blockIdx.x, R = row0 + lr;
    uint32_t rank, inst;   // (uniform over the workgroup)
    circ_row(X, R, instances, rank, inst);
    if ((node_kind[rank] & 0xFFu) != 1) return;   // a sum node's rows only
    const uint32_t slot = out_slot[3 * rank + 2];
    if (slot == CIRC_SLOT_NONE) return;
    const size_t stride = n + 1;
    const ulonglong2 *src = res + (size_t)lr * 3 * stride;
    uint64_t *dst = wires + ((size_t)slot * instances + inst) * stride;
    for (uint32_t e = threadIdx.x; e <= n; e += 256) {
        const ulonglong2 v = src[e];
        const uint64_t s = e < n ? a1[(size_t)lr * n + e] + a2[(size_t)lr * n + e] : b1[lr] + b2[lr];
        dst[e] = (s - 2 * modred(((u128)v.y << 64) | v.x, CC)) & (r - 1);
    }
}

// bootstrap output [rows][3][n + 1] -> the slots of the gate outputs something reads
__global__ void __launch_bounds__(256)
k_circ_scatter(const uint64_t *__restrict__ res, const uint32_t *__restrict__ out_slot, uint64_t *__restrict__ wires,
               uint32_t row0, uint32_t rows, uint32_t instances, uint32_t n, CircPairs X = {}) {
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    const uint32_t w3 = 3 * (n + 1);
    if (t >= rows * w3) return;
    const uint32_t lr = t / w3, rem = t % w3, g = rem / (n + 1), e = rem % (n + 1), R = row0 + lr;
    uint32_t rank, inst;
    circ_row(X, R, instances, rank, inst);
    const uint32_t slot = out_slot[3 * rank + g];
    if (slot == CIRC_SLOT_NONE) return;
    wires[((size_t)slot * instances + inst) * (n + 1) + e] = res[t];
}

// The scatter of a level call whose k-loop left its rows un-reduced ([rows][3][n + 1] 16-byte residues over
// Z_Q: SGFHE_CIRCUIT_PACK_DIRECT, a call that produces a wire some packed output names).  One workgroup per
// (row, blockIdx.y); the threads run along the n + 1 axis, so the loads are coalesced 16-byte accesses and the
// row decode is per workgroup, not per thread.
//   blockIdx.y == 0 (launches with_wires = 1; a call with more jobs than a grid holds takes further launches
//                    without): ModRed (the device function of k_final: the same words) of the gate outputs something
//                    reads into their slots of the wire table, as k_circ_scatter does with reduced rows;
//   blockIdx.y == with_wires + j: job j = {output o, rank of the producing node in its level, gate | CIRC_REF_NOT}:
//                    the rows of that node copied as they are into rawout [o][instances][n + 1].  NOT over Z_Q
//                    is enc_trivial(true) - w with true = (0, 2 DQ_tilde): a -> -a, b -> 2 DQ_tilde - b mod Q.
__global__ void __launch_bounds__(256)
k_circ_scatter_raw(const ulonglong2 *__restrict__ res, const uint32_t *__restrict__ out_slot,
                   uint64_t *__restrict__ wires, const uint32_t *__restrict__ jobs, ulonglong2 *__restrict__ rawout,
                   const CrtConst *__restrict__ CC, uint32_t row0, uint32_t instances, uint32_t n, uint32_t with_wires,
                   CircPairs X = {}) {
    const uint32_t lr = blockIdx.x, R = row0 + lr;
    uint32_t rank, inst;   // (uniform over the workgroup; both halves below read them)
    circ_row(X, R, instances, rank, inst);
    const size_t stride = n + 1;
    if (with_wires && blockIdx.y == 0) {
        for (uint32_t g = 0; g < 3; g++) {
            const uint32_t slot = out_slot[3 * rank + g];
            if (slot == CIRC_SLOT_NONE) continue;
            const ulonglong2 *src = res + ((size_t)lr * 3 + g) * stride;
            uint64_t *dst = wires + ((size_t)slot * instances + inst) * stride;
            for (uint32_t e = threadIdx.x; e <= n; e += 256) {
                const ulonglong2 v = src[e];
                dst[e] = modred(((u128)v.y << 64) | v.x, CC);
            }
        }
        return;
    }
    const uint32_t *job = jobs + 3 * (size_t)(blockIdx.y - with_wires);
    if (job[1] != rank) return;
    const uint32_t neg = job[2] & CIRC_REF_NOT, g = job[2] & 3u;
    const ulonglong2 *src = res + ((size_t)lr * 3 + g) * stride;
    ulonglong2 *dst = rawout + ((size_t)job[0] * instances + inst) * stride;
    const u128 Q = CC->Q;
    u128 one = 2 * CC->DQ;   // reduced as k_lwe_noise_q reduces it: the ctx accepts any DQ_tilde < Q
    if (one >= Q) one -= Q;
    for (uint32_t e = threadIdx.x; e <= n; e += 256) {
        ulonglong2 v = src[e];
        if (neg) {
            const u128 x = ((u128)v.y << 64) | v.x;
            const u128 y = e < n ? (x ? Q - x : 0) : (one >= x ? one - x : one + Q - x);
            v = make_ulonglong2((uint64_t)y, (uint64_t)(y >> 64));
        }
        dst[e] = v;
    }
}

// gate 0 (AND) of an un-reduced bootstrap output [rows][3][n + 1] -> compact rows [rows][n + 1] (the refreshed
// ciphertexts of a direct pack group on their way into the raw output table); one workgroup per row
__global__ void __launch_bounds__(256)
k_circ_raw_and(const ulonglong2 *__restrict__ res, ulonglong2 *__restrict__ dst, uint32_t n) {
    const size_t stride = n + 1;
    const ulonglong2 *src = res + (size_t)blockIdx.x * 3 * stride;
    ulonglong2 *d = dst + (size_t)blockIdx.x * stride;
    for (uint32_t e = threadIdx.x; e <= n; e += 256) d[e] = src[e];
}

// ---- lift to Z_Q (sgfhe_lwe_lift_modq, SGFHE_CIRCUIT_PACK_LIFT) ----------------------------------------------------
// L(x) = floor((x Q + r/2) / r), r = 2^logr: the exact scaling of a word of Z_r to a canonical residue of Z_Q.  It
// maps a wrap of r to a wrap of Q and the codeword Dr to Q/4 (2 DQ_tilde to within 1), and adds at most 1/2 of
// rounding per word; the error of the LWE is carried on, scaled, not cleaned.  x < r <= 2^15 and Q < 2^94: the
// product is below 2^109, and the result below Q because x <= r - 1.
__device__ __forceinline__ ulonglong2 lift_word(uint64_t x, const CrtConst *CC) {
    const u128 y = ((u128)x * CC->Q + (1ull << (CC->logr - 1))) >> CC->logr;
    return make_ulonglong2((uint64_t)y, (uint64_t)(y >> 64));
}

// The lifted ciphertexts of a pack group (SGFHE_CIRCUIT_PACK_LIFT): rows row0 .. row0 + rows of the pack stage's
// pseudo-level, whose node o is (TRUE, output o) -- row R = q n + bit is output R / instances at instance R % instances
// -- read from the wire table as that level's gather reads its second input (`outs` [n_outputs]; NOT, the constant
// and the lane shift or route applied over Z_r), lifted word by word into row R of the raw output table
// [q][n][n + 1].  Thread-to-word map of the gathers: coalesced 8-byte loads along a source row, 16-byte stores
// (raw rows are 16-byte aligned), the row decode uniform over a row.
__global__ void __launch_bounds__(256)
k_circ_lift(const uint64_t *__restrict__ wires, CircRefs outs, ulonglong2 *__restrict__ rawout,
            const CrtConst *__restrict__ CC, uint32_t row0, uint32_t rows, uint32_t instances, uint32_t n, uint64_t r) {
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= rows * (n + 1)) return;
    const uint32_t lr = t / (n + 1), e = t % (n + 1), R = row0 + lr;
    const uint32_t o = R / instances, inst = R % instances;
    const uint64_t v = circ_ref_word(wires, outs, o, instances, inst, e, n, r, r / 4);
    rawout[(size_t)R * (n + 1) + e] = lift_word(v, CC);
}

// sgfhe_lwe_lift_modq: the same device function on plain rows, `total` words (grid-stride: the array may hold more
// than 2^32 words)
__global__ void __launch_bounds__(256)
k_lwe_lift(const uint64_t *__restrict__ in, ulonglong2 *__restrict__ out, const CrtConst *__restrict__ CC, size_t total) {
    for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (size_t)gridDim.x * 256)
        out[t] = lift_word(in[t], CC);
}

// the circuit's outputs [n_outputs][instances][n + 1], NOT, the constant and the lane shift or route of `outs`
// [n_outputs] applied (grid-stride: the array may hold more than 2^32 words)
__global__ void __launch_bounds__(256)
k_circ_collect(const uint64_t *__restrict__ wires, CircRefs outs, uint64_t *__restrict__ out, size_t total,
               uint32_t instances, uint32_t n, uint64_t r) {
    const size_t per_out = (size_t)instances * (n + 1);
    for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (size_t)gridDim.x * 256) {
        const size_t o = t / per_out, w = t % per_out;
        const uint32_t inst = (uint32_t)(w / (n + 1)), e = (uint32_t)(w % (n + 1));
        out[t] = circ_ref_word(wires, outs, o, instances, inst, e, n, r, r / 4);
    }
}

// ---- registers of a stepped run (sgfhe_circuit_run_steps) ------------------------------------------------------------
// The state buffer [n_regs][instances][n + 1] is the canonical value of the registers between steps; the wire table
// only holds a copy for the length of a step.  Both kernels are memory-bound copies in the thread-to-word map of
// k_circ_collect: one word per thread and step of the grid-stride loop, consecutive threads consecutive words of a row
// (coalesced 8-byte accesses), the register decode uniform over a row.

// Start of a step: register i's rows into its slot of the wire table (reg_slot = the first n_regs entries of the
// plan's input_slot; a register nothing reads has no slot).  One launch for all registers.
__global__ void __launch_bounds__(256)
k_circ_state_load(const uint64_t *__restrict__ state, const uint32_t *__restrict__ reg_slot,
                  uint64_t *__restrict__ wires, size_t total, uint32_t instances, uint32_t n) {
    const size_t per_reg = (size_t)instances * (n + 1);
    for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (size_t)gridDim.x * 256) {
        const size_t i = t / per_reg, w = t % per_reg;
        const uint32_t slot = reg_slot[i];
        if (slot != CIRC_SLOT_NONE) wires[(size_t)slot * per_reg + w] = state[t];
    }
}

// End of a step: the next-state gather.  Register i takes reference i of `nexts` -- NOT, the constant and the shift
// or route as k_circ_collect applies them to an output, with the codeword of NOT and of the TRUE fill
// Dr >> next_scale[i], the register's scale.  It reads the wire table and writes the state buffer, never the same
// words: a swap, a rotation, a register holding itself or reading a stream input need no ordering between threads.
__global__ void __launch_bounds__(256)
k_circ_next(const uint64_t *__restrict__ wires, CircRefs nexts, const uint32_t *__restrict__ next_scale,
            uint64_t *__restrict__ state, size_t total, uint32_t instances, uint32_t n, uint64_t r) {
    const size_t per_reg = (size_t)instances * (n + 1);
    for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (size_t)gridDim.x * 256) {
        const size_t i = t / per_reg, w = t % per_reg;
        const uint32_t inst = (uint32_t)(w / (n + 1)), e = (uint32_t)(w % (n + 1));
        state[t] = circ_ref_word(wires, nexts, i, instances, inst, e, n, r, (r / 4) >> next_scale[i]);
    }
}

// split_ciphertext (fhe.jl:287-290, extract :237-244) of the input ciphertexts of sgfhe_circuit_run_ct, straight
// into the wire table.  ct_a / ct_b [n_inputs][blocks][N] (N = n or m); bit i of (input, block) becomes the row of
// instance block * n + i in the input's slot: word j < n is a[i - j] for j <= i and -a[N - (j - i)] mod r beyond,
// word n is b[i] -- with ext[d] = a[d] (d >= 0), -a[N + d] (d < 0), word j is ext[i - j].
// Bound by its stores (n + 1 words written per coefficient read).  A workgroup writes CIRC_SPLIT_ROWS consecutive
// rows of one ciphertext, which are contiguous in the table: it stages the n + CIRC_SPLIT_ROWS - 1 values of ext
// those rows read in LDS once (negated where d < 0), then every thread stores one word per step, consecutive
// threads consecutive words (coalesced 8-byte stores; rows of n + 1 words are not 16-byte aligned).
// grid = n_inputs * blocks * ceil(n / CIRC_SPLIT_ROWS); dynamic LDS (n + CIRC_SPLIT_ROWS - 1) * 8 bytes.
constexpr uint32_t CIRC_SPLIT_ROWS = 16;

__global__ void __launch_bounds__(256)
k_circ_split(const uint64_t *__restrict__ ct_a, const uint64_t *__restrict__ ct_b,
             const uint32_t *__restrict__ in_slot, uint64_t *__restrict__ wires, uint32_t blocks, uint32_t N,
             uint32_t n, uint64_t r) {
    SGFHE_DYN_LDS(uint64_t, split_ext);
    const uint32_t tiles = (n + CIRC_SPLIT_ROWS - 1) / CIRC_SPLIT_ROWS;
    const uint32_t tile = blockIdx.x % tiles, q = blockIdx.x / tiles;   // q = input * blocks + block
    const uint32_t input = q / blocks, block = q % blocks;
    const uint32_t slot = in_slot[input];
    if (slot == CIRC_SLOT_NONE) return;   // nothing reads this input (uniform over the workgroup)
    const uint32_t i0 = tile * CIRC_SPLIT_ROWS;
    const uint32_t rows = n - i0 < CIRC_SPLIT_ROWS ? n - i0 : CIRC_SPLIT_ROWS;
    const uint64_t *a = ct_a + (size_t)q * N, *b = ct_b + (size_t)q * N;
    // split_ext[k] = ext[i0 - (n - 1) + k], k < n + rows - 1: d runs from i0 - n + 1 to i0 + rows - 1 <= n - 1 < N
    for (uint32_t k = threadIdx.x; k < n + rows - 1; k += 256) {
        const int32_t d = (int32_t)(i0 + k) - (int32_t)(n - 1);
        split_ext[k] = d >= 0 ? a[d] : (r - a[N - (uint32_t)(-d)]) & (r - 1);
    }
    __syncthreads();
    const uint32_t row = n + 1, total = rows * row;
    uint64_t *dst = wires + ((size_t)slot * blocks * n + (size_t)block * n + i0) * row;
    uint32_t lr = threadIdx.x / row, e = threadIdx.x % row;
    for (uint32_t w = threadIdx.x; w < total; w += 256) {
        // word e of row i0 + lr: ext[i0 + lr - e] = split_ext[lr + n - 1 - e]
        dst[w] = e < n ? split_ext[lr + n - 1 - e] : b[i0 + lr];
        e += 256;
        while (e >= row) { e -= row; lr++; }
    }
}

// ---- noise probe (sgfhe_lwe_noise, sgfhe_circuit_run_probe) -----------------------------------------
// The error of LWE rows against the secret key, reduced to integer statistics per wire.  A diagnostic: the
// key bits are on the device only for the length of the call.
// One wave64 per row: lane l adds the words l, l + 64, ... of a whose key bit is set (coalesced 8-byte loads;
// rows are not 16-byte aligned), the wave sums by shuffles, and every lane then holds the row's phase.  The n
// key bits are a bit mask in LDS, loaded once per workgroup: bit l of word j is s[64 j + l], so a wave reads one
// word per step (a broadcast) and each lane its own bit.  A workgroup of NOISE_WAVES waves covers NOISE_ROWS
// consecutive instances of ONE wire (wave w takes instances w, w + NOISE_WAVES, ... of the tile), sums its
// rows' statistics in LDS and issues one 64-bit atomic per statistic into the wire's record: integer sums and a
// maximum, so the record does not depend on the launch geometry or on the order of arrival.
// Geometry, shared by both kernels: row R = node * instances + instance of a level (sgfhe_circuit_run's
// numbering); a launch covers the rows [row0, row0 + rows) of a call, whose LWEs are at lwe + (R - row0) *
// row_stride + gate * gate_stride words; blockIdx.x = node_in_launch * tiles + tile, the tile's instances start
// at inst0 + tile * NOISE_ROWS, blockIdx.y = gate; the wire's record and its row of the bit table are
// wire0 + node_in_launch * gridDim.y + gate.  A tile never leaves its node; rows of the node outside the call
// are skipped.  The primitive is one node of `count` instances, one gate.
// bits: [wire][bit_words] uint64, instance t at bit t & 63 of word t / 64 (circuit_plain_bits of circuit.h).
constexpr uint32_t NOISE_WAVES = 4, NOISE_ROWS = 16, NOISE_MASK_WORDS = 64;   // n <= 4096 (sgfhe_ctx_create)

struct NoiseGeom {
    size_t row_stride, gate_stride;   // in words of the row type
    uint32_t wire0, node0, row0, rows, instances, inst0, tiles, bit_words, n;
    const uint32_t *kind;             // the node kinds of the launch, by node_in_launch (device; NULL: no LUT node) --
                                      // gate g of a LUT node is measured against its own codeword Dr >> g
    uint32_t scale;                   // added to that scale: the launch over one wire of a LUT sibling, from its slot
};

__device__ __forceinline__ void noise_load_mask(uint64_t *smask, const uint64_t *__restrict__ keymask, uint32_t n) {
    const uint32_t words = (n + 63) / 64;
    if (threadIdx.x < words) smask[threadIdx.x] = keymask[threadIdx.x];
    __syncthreads();
}
// local row (R - row0) of instance i of this workgroup's node, or -1 when the call does not hold it
__device__ __forceinline__ int64_t noise_row(const NoiseGeom &G, uint32_t node, uint32_t i) {
    if (i >= G.instances) return -1;
    const uint64_t R = (uint64_t)(G.node0 + node) * G.instances + i;
    return R >= G.row0 && R < (uint64_t)G.row0 + G.rows ? (int64_t)(R - G.row0) : -1;
}
__device__ __forceinline__ uint64_t wave_sum64(uint64_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// Rows over Z_r (r = 2^logr, Dr = r / 4): phase = b - sum a_i s_i, e = centred (phase - bit * Dr) in (-r/2, r/2].
// stats[wire][8] = {rows, rows that decrypt wrongly ((phase + Dr/2) mod r div Dr != bit, fhe.jl:504-507), max |e|,
// sum e (two's complement), sum e^2, rows with |e| >= Dr/4, 0, 0}.
__global__ void __launch_bounds__(64 * NOISE_WAVES)
k_lwe_noise(const uint64_t *__restrict__ lwe, const uint64_t *__restrict__ keymask, const uint64_t *__restrict__ bits,
            unsigned long long *__restrict__ stats, NoiseGeom G, uint32_t logr) {
    __shared__ uint64_t smask[NOISE_MASK_WORDS];
    __shared__ uint64_t part[NOISE_WAVES][6];
    noise_load_mask(smask, keymask, G.n);
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t node = blockIdx.x / G.tiles, tile = blockIdx.x % G.tiles;
    const uint32_t wire = G.wire0 + node * gridDim.y + blockIdx.y;
    const uint64_t rmask = (1ull << logr) - 1, Dr = 1ull << (logr - 2);
    // the wire's codeword C = Dr >> scale (uniform over the workgroup): scale 0 but for wires +1, +2 of a LUT node
    const uint32_t scale = G.scale + (G.kind && (G.kind[node] & 0xFFu) == 2 ? blockIdx.y : 0u);
    const uint64_t C = Dr >> scale;
    const uint64_t *wbits = bits + (size_t)wire * G.bit_words;
    uint64_t cnt = 0, wrong = 0, emax = 0, esum = 0, esq = 0, margin = 0;
    for (uint32_t t = wave; t < NOISE_ROWS; t += NOISE_WAVES) {
        const uint32_t i = G.inst0 + tile * NOISE_ROWS + t;
        const int64_t lr = noise_row(G, node, i);   // (uniform over the wave)
        if (lr < 0) continue;
        const uint64_t *row = lwe + (size_t)lr * G.row_stride + (size_t)blockIdx.y * G.gate_stride;
        uint64_t s = 0;
#pragma unroll 4
        for (uint32_t w = lane, j = 0; w < G.n; w += 64, j++) {
            const uint64_t a = row[w];
            s += (smask[j] >> lane) & 1 ? a : 0ull;
        }
        s = wave_sum64(s);
        const uint64_t bit = (wbits[i >> 6] >> (i & 63)) & 1;
        const uint64_t phase = (row[G.n] - s) & rmask;
        const uint64_t d = (phase - bit * C) & rmask;
        const int64_t e = d > (rmask >> 1) + 1 ? (int64_t)d - (int64_t)(rmask + 1) : (int64_t)d;
        const uint64_t ae = e < 0 ? (uint64_t)(-e) : (uint64_t)e;
        cnt++;
        wrong += scale ? ae >= C / 2 : (((phase + Dr / 2) & rmask) >> (logr - 2)) != bit;
        emax = ae > emax ? ae : emax;
        esum += (uint64_t)e;
        esq += ae * ae;
        margin += ae >= C / 4;
    }
    if (lane == 0) {
        part[wave][0] = cnt, part[wave][1] = wrong, part[wave][2] = emax;
        part[wave][3] = esum, part[wave][4] = esq, part[wave][5] = margin;
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        const uint32_t k = threadIdx.x;
        uint64_t v = part[0][k], held = part[0][0];
        for (uint32_t w = 1; w < NOISE_WAVES; w++) {
            v = k == 2 ? (part[w][k] > v ? part[w][k] : v) : v + part[w][k];
            held += part[w][0];
        }
        unsigned long long *rec = stats + (size_t)wire * 8;
        if (held) {   // a tile outside the call adds nothing
            if (k == 2) atomicMax(rec + k, (unsigned long long)v);
            else atomicAdd(rec + k, (unsigned long long)v);
        }
    }
}

// Rows over Z_Q ([n + 1] 16-byte canonical residues, a RAW_MODQ result): the lanes' sums stay below n Q < 2^106,
// are added as 128-bit values and reduced mod Q once per row (mod_wide).  The codewords are 0 and 2 DQ_tilde
// (enc_trivial(true) over Z_Q): e = centred (phase - bit * 2 DQ_tilde) in (-Q/2, Q/2].  There is no 128-bit atomic:
// every workgroup walks its tiles in a grid-stride loop and writes one partial record
// partial[blockIdx.x][8] = {rows, rows with |e| >= DQ_tilde, max |e| lo, hi, sum |e| lo, hi, 0, 0}; the host folds them.
__global__ void __launch_bounds__(64 * NOISE_WAVES)
k_lwe_noise_q(const ulonglong2 *__restrict__ lwe, const uint64_t *__restrict__ keymask,
              const uint64_t *__restrict__ bits, unsigned long long *__restrict__ partial,
              const CrtConst *__restrict__ CC, NoiseGeom G) {
    __shared__ uint64_t smask[NOISE_MASK_WORDS];
    __shared__ uint64_t part[NOISE_WAVES][6];
    noise_load_mask(smask, keymask, G.n);
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const u128 Q = CC->Q, DQ = CC->DQ;
    u128 one = 2 * DQ;
    if (one >= Q) one -= Q;
    uint64_t cnt = 0, wrong = 0;
    u128 emax = 0, esum = 0;
    for (uint32_t tile = blockIdx.x; tile < G.tiles; tile += gridDim.x)
        for (uint32_t t = wave; t < NOISE_ROWS; t += NOISE_WAVES) {
            const uint32_t i = G.inst0 + tile * NOISE_ROWS + t;
            const int64_t lr = noise_row(G, 0, i);   // (uniform over the wave)
            if (lr < 0) continue;
            const ulonglong2 *row = lwe + (size_t)lr * G.row_stride;
            u128 s = 0;
#pragma unroll 4
            for (uint32_t w = lane, j = 0; w < G.n; w += 64, j++) {
                const ulonglong2 a = row[w];
                if ((smask[j] >> lane) & 1) s += ((u128)a.y << 64) | a.x;
            }
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) {
                const uint64_t lo = __shfl_xor((uint64_t)s, d, 64), hi = __shfl_xor((uint64_t)(s >> 64), d, 64);
                s += ((u128)hi << 64) | lo;
            }
            s = mod_wide(s, Q, CC->invQ, nullptr);
            const ulonglong2 bv = row[G.n];
            const u128 b = ((u128)bv.y << 64) | bv.x;
            const u128 phase = b >= s ? b - s : b + Q - s;
            const bool bit = (bits[i >> 6] >> (i & 63)) & 1;
            const u128 code = bit ? one : 0;
            const u128 d = phase >= code ? phase - code : phase + Q - code;
            const u128 ae = d > (Q >> 1) ? Q - d : d;
            cnt++;
            wrong += ae >= DQ;
            emax = ae > emax ? ae : emax;
            esum += ae;
        }
    if (lane == 0) {
        part[wave][0] = cnt, part[wave][1] = wrong;
        part[wave][2] = (uint64_t)emax, part[wave][3] = (uint64_t)(emax >> 64);
        part[wave][4] = (uint64_t)esum, part[wave][5] = (uint64_t)(esum >> 64);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (uint32_t w = 1; w < NOISE_WAVES; w++) {
            cnt += part[w][0], wrong += part[w][1];
            const u128 m = ((u128)part[w][3] << 64) | part[w][2];
            emax = m > emax ? m : emax;
            esum += ((u128)part[w][5] << 64) | part[w][4];
        }
        unsigned long long *rec = partial + (size_t)blockIdx.x * 8;
        rec[0] = cnt, rec[1] = wrong;
        rec[2] = (uint64_t)emax, rec[3] = (uint64_t)(emax >> 64);
        rec[4] = (uint64_t)esum, rec[5] = (uint64_t)(esum >> 64);
        rec[6] = 0, rec[7] = 0;
    }
}

// digits -> canonical accumulators (debug hook)
__global__ void __launch_bounds__(256)
k_dump_acc(const uint64_t *__restrict__ dig, ulonglong2 *__restrict__ out,
           const CrtConst *__restrict__ CC, uint32_t total, uint32_t logm, uint32_t mode) {
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const uint32_t M = 1u << logm;
    const u128 x = acc_from_digits(load_digits(dig, t >> logm, t & (M - 1), M, (mode & MODE_WIDE) != 0), CC, mode);
    out[t] = make_ulonglong2((uint64_t)x, (uint64_t)(x >> 64));
}

// stored digit planes -> [bootstrap][c][digit][m] uint64 (debug hook): e_i = u_i + s, or
// u_i + s + xmax in the randomised mode, u the reference's flatten result as a signed integer
__global__ void __launch_bounds__(256)
k_dump_digits(const uint64_t *__restrict__ dig, uint64_t *__restrict__ out, uint32_t total,
              uint32_t logm, uint32_t mode) {
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const uint32_t M = 1u << logm, bc = t >> logm, i = t & (M - 1);
    const ulonglong2 d = load_digits(dig, bc, i, M, (mode & MODE_WIDE) != 0);
    out[((size_t)bc * 2 + 0) * M + i] = d.x;
    out[((size_t)bc * 2 + 1) * M + i] = d.y;
}

// [bootstrap][c][digit][m] uint64 -> stored digit planes, the inverse of k_dump_digits (debug hook:
// sgfhe_debug_kloop_step, which has checked that every value is one a flatten stores)
__global__ void __launch_bounds__(256)
k_load_digits(const uint64_t *__restrict__ in, uint64_t *__restrict__ dig, uint32_t total,
              uint32_t logm, uint32_t mode) {
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const uint32_t M = 1u << logm, bc = t >> logm, i = t & (M - 1);
    store_digits(dig, bc, i, M, in[((size_t)bc * 2 + 0) * M + i], in[((size_t)bc * 2 + 1) * M + i],
                 (mode & MODE_WIDE) != 0);
}

// canonical residues -> digits of x' = (v + off) mod Q  (flatten, utils.jl:155-189)
__global__ void __launch_bounds__(256)
k_flatten_canon(const ulonglong2 *__restrict__ in, uint64_t *__restrict__ dig,
                const CrtConst *__restrict__ CC, uint32_t total, uint32_t logm) {
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const uint32_t M = 1u << logm;
    const ulonglong2 v = in[t];
    u128 x = (((u128)v.y << 64) | v.x) + (CC->Q - CC->offneg);
    if (x >= CC->Q) x -= CC->Q;
    if (x >= CC->Q) x -= CC->Q;
    uint64_t hi;
    const u128 lo = mod_wide(x, CC->B, CC->invB, &hi);
    store_digits(dig, t >> logm, t & (M - 1), M, (uint64_t)lo, hi);
}

// ==================================================================================================
// Packing LWEs into an RLWE ciphertext: pack_encrypted_bits / shortened_external_product
// (src/fhe.jl:632-641,660-696), second caller of the hot path.
//   1. n bootstraps (trivial encryption of 1, bit_i), AND branch, un-reduced      (k-loop above)
//   2. k_pack_flatten: as_i = polynomial of the i-th LWE coefficients (fhe.jl:675-677), flattened
//   3. k_shortprod:   for a group of slices i: sum_i flatten(as_i) * C_i[2:4, :]  in the NTT domain
//                     (exact integers stay below 0.4 M for `G` slices per group), inverse NTT
//   4. k_pack_finish: CRT of every group, sum mod Q, w = ModRed(-W), v = ModRed(b - V)
// ==================================================================================================

// raw: the un-reduced LWE of bit j of ciphertext ci is the n + 1 16-byte residues at row
// (ci * n + j) * rstride -- rstride = 3 (n + 1) for a RAW_MODQ bootstrap output [count * n][3][n + 1],
// of which only gate 0 (AND) is read, and n + 1 for a compact [count * n][n + 1] source
// (sgfhe_pack_lwe_modq).  pdig: [count][n slices][2 digits][len] uint64 with len = n coefficients for the
// deterministic flatten (the zero padding of as_i, fhe.jl:675-677, has the constant digits of 0)
// and len = m for the randomised one (flatten_poly draws for every coefficient of the resized
// polynomial, utils.jl:253-264).
__global__ void __launch_bounds__(256)
k_pack_flatten(const ulonglong2 *__restrict__ raw, uint64_t *__restrict__ pdig,
               const CrtConst *__restrict__ CC, uint32_t count, uint32_t n, uint32_t logm,
               uint32_t mode, RndArgs ra, uint32_t rstride) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t len = (mode & MODE_RANDOM) ? (1u << logm) : n;
    if (t >= (size_t)count * n * len) return;
    const uint32_t j = (uint32_t)(t % len);         // bit index = coefficient index of as_i
    const uint32_t i = (uint32_t)((t / len) % n);   // LWE coefficient index = slice
    const uint32_t ci = (uint32_t)(t / ((size_t)n * len));
    const u128 Q = CC->Q;
    u128 x = 0;
    if (j < n) {
        const ulonglong2 v = raw[((size_t)ci * n + j) * rstride + i];
        x = ((u128)v.y << 64) | v.x;
    }
    uint64_t *d = pdig + (((size_t)ci * n + i) * 2) * len + j;
    if (mode & MODE_RANDOM) {
        x += CC->offneg_rnd ? Q - CC->offneg_rnd : 0;   // + (s + xmax)(1 + B)
        if (x >= Q) x -= Q;
        const ulonglong2 e = random_digits(x, CC, ra.key, make_uint4(j, 0x80000000u | i, ci, ra.call));
        d[0] = e.x;
        d[len] = e.y;
        return;
    }
    x += Q - CC->offneg;   // + off
    if (x >= Q) x -= Q;
    uint64_t hi;
    const u128 lo = mod_wide(x, CC->B, CC->invB, &hi);
    d[0] = (uint64_t)lo;
    d[len] = hi;
}

// grid = count * groups * NPR workgroups of T threads.  Workgroup (ci, g, pi) runs the 2 G phases
// (slice i in the group, digit) through the forward NTT and accumulates both product columns
// lazily (mod 2p; z0 in registers, z1 in LDS), then two inverse NTTs.
//   yg [count][groups][2][NPR][m] residues (+ hoff), in [0, p]
template <int LOGM>
__global__ void __launch_bounds__((NttGeom<LOGM, LOGE>::T), (NttGeom<LOGM, LOGE>::T >= 256 ? 4 : 1))
k_shortprod(const uint64_t *__restrict__ pdig, const int32_t *__restrict__ keyhat,
            uint32_t *__restrict__ yg, PrimeSet PS, const CrtConst *__restrict__ CC, uint32_t n,
            uint32_t G, uint32_t groups, uint32_t mode) {
    using GE = NttGeom<LOGM, LOGE>;
    constexpr int M = GE::M, T = GE::T, E = GE::E;
    SGFHE_DYN_LDS(uint32_t, lds);
    int32_t *const ldsi = reinterpret_cast<int32_t *>(lds);
    const uint32_t npr = PS[0].npr;
    const uint32_t pi = blockIdx.x % npr;
    const uint32_t g = (blockIdx.x / npr) % groups;
    const uint32_t ci = blockIdx.x / (npr * groups);
    const PrimeK P = PS[pi];
    const Mod md = mod_of(P);
    const int32_t sRd = (mode & MODE_RANDOM) ? P.sRr : P.sR;
    // residues of the digits of a zero coefficient (x' = off): the zero padding of as_i
    // (deterministic flatten of 0; the randomised mode draws for the padding too: k_pack_flatten
    // writes all m coefficients there)
    const int32_t zlo = digit_reduce(CC->dig0.x, md, P.sR), zhi = digit_reduce(CC->dig0.y, md, P.sR);
    const uint32_t len = (mode & MODE_RANDOM) ? (uint32_t)M : n;  // stored coefficients per digit polynomial

    int32_t z0[1][E];
#pragma unroll
    for (int e = 0; e < E; e++) { z0[0][e] = 0; ldsi[M + e * T + threadIdx.x] = 0; }
#pragma unroll 1
    for (uint32_t ph = 0; ph < 2 * G; ph++) {
        const int tid = (int)threadIdx.x + (int)opaque_zero();
        const uint32_t i = g * G + (ph >> 1), digit = ph & 1;
        int32_t x[1][E];
        const uint64_t *d = pdig + (((size_t)ci * n + i) * 2 + digit) * len;
#pragma unroll
        for (int e = 0; e < E; e++) {
            const uint32_t idx = tid + T * e;
            x[0][e] = idx < len ? digit_reduce(d[idx], md, sRd) : (digit ? zhi : zlo);
        }
        SGFHE_SYNC();
        ntt_forward<LOGM, 1, LOGE>(x, lds, P.twf, tid, md);
        // key rows l + 1 .. 2 l of slice i (fhe.jl:638-639): polynomials (2 + digit) * 2 + c
        const int32_t *kp = keyhat + (((size_t)i * npr + pi) * 8 + (2 + digit) * 2) * M + E * tid;
#pragma unroll
        for (int h = 0; h < E / 4; h++) {
            const int4 a = reinterpret_cast<const int4 *>(kp)[h];
            const int4 bq = reinterpret_cast<const int4 *>(kp + M)[h];
            const int32_t ka[4] = {a.x, a.y, a.z, a.w};
            const int32_t kb[4] = {bq.x, bq.y, bq.z, bq.w};
#pragma unroll
            for (int t = 0; t < 4; t++) {
                const int e = 4 * h + t;
                const int32_t u = x[0][e];
                z0[0][e] = sred(z0[0][e] + smont(u, ka[t], md), md);  // stays below 0.52 * 2^29
                int32_t *zp = ldsi + M + e * T + tid;
                *zp = sred(*zp + smont(u, kb[t], md), md);
            }
        }
    }
    const int tid = threadIdx.x;
    uint32_t *yb = yg + (((size_t)ci * groups + g) * 2 * npr + pi) * M;
#pragma unroll
    for (int c = 0; c < 2; c++) {
        if (c > 0) {
#pragma unroll
            for (int e = 0; e < E; e++) z0[0][e] = ldsi[M + e * T + tid];
            SGFHE_SYNC();
        }
        ntt_inverse<LOGM, 1, LOGE>(z0, lds, P.twi, tid, md);
#pragma unroll
        for (int e = 0; e < E; e++)
            yb[(size_t)c * npr * M + tid + T * e] = condsub(sfull(z0[0][e], md) + P.hoff, (uint32_t)P.p);
    }
}

// One thread per (ciphertext, coefficient k < m): W = sum_g CRT(y_g column 0), V likewise
// (fhe.jl:686-687); w = ModRed(-W), v = ModRed(b_k - V) (fhe.jl:689-693), b_k = the un-reduced
// LWE constant of bit k for k < n and 0 beyond (resize, fhe.jl:678).  raw / rstride as in k_pack_flatten.
template <int NP>
__global__ void __launch_bounds__(256)
k_pack_finish(const uint32_t *__restrict__ yg, const ulonglong2 *__restrict__ raw,
              uint64_t *__restrict__ out_w, uint64_t *__restrict__ out_v,
              const CrtConst *__restrict__ CC, uint32_t count, uint32_t n, uint32_t logm,
              uint32_t groups, uint32_t rstride) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t M = 1u << logm;
    if (t >= (size_t)count * M) return;
    const uint32_t kk = (uint32_t)(t & (M - 1));
    const uint32_t ci = (uint32_t)(t >> logm);
    const u128 Q = CC->Q;
    u128 acc[2] = {0, 0};
    for (uint32_t g = 0; g < groups; g++) {
#pragma unroll
        for (int c = 0; c < 2; c++) {
            const uint32_t *yp = yg + ((((size_t)ci * groups + g) * 2 + c) * NP) * M + kk;
            uint32_t y[NP];
#pragma unroll
            for (int q = 0; q < NP; q++) y[q] = yp[(size_t)q * M];
            const U96 a = crt_reduce(y, CC, false, make_ulonglong2(0, 0));
            acc[c] += ((u128)a.w2 << 64) | ((uint64_t)a.w1 << 32) | a.w0;
            if (acc[c] >= Q) acc[c] -= Q;
        }
    }
    const u128 w1 = acc[0] ? Q - acc[0] : 0;
    u128 bk = 0;
    if (kk < n) {
        const ulonglong2 v = raw[((size_t)ci * n + kk) * rstride + n];
        bk = ((u128)v.y << 64) | v.x;
    }
    const u128 v1 = bk >= acc[1] ? bk - acc[1] : bk + Q - acc[1];
    out_w[t] = modred(w1, CC);
    out_v[t] = modred(v1, CC);
}

// ==================================================================================================
// Bootstrap-key generation on the device: BootstrapKey(rng, sk) (src/fhe.jl:181-201), SURVEY.md 8f
// row N2.  Randomness: ChaCha20 (RFC 8439 block function) keyed with the caller's 32-byte seed,
// one stream per (domain, key row), nonce = (domain, k * 4 + row, 0), block counter from 0:
//   domain 1  the uniform polynomial a_row: coefficient i = words 4 (i mod 4) .. + 3 of block i / 4,
//             lo = w0 | w1 << 32, hi = w2 | w3 << 32, value (hi 2^64 + lo) mod Q   (fhe.jl:193)
//   domain 2  the noise e_row: coefficient i = words 2 (i mod 8), + 1 of block i / 8,
//             d = w0 | w1 << 32, value d mod (2 noise + 1) - noise                   (fhe.jl:194)
// The streams are counter-addressed, so every thread computes its own block; the oracle's
// generator (oracle/sgfhe_oracle.c, oracle/bigint_oracle.py) reads the same streams and produces
// the same key from the same seed.
// Per batch of rows:  k_keygen_draw -> k_polymul_s (a (*) s, exact, per prime) -> k_crt_acc (CANON)
// -> k_keygen_finish (b = a (*) s + e, + s_k G on the constant terms) -> k_key_transform.
// ==================================================================================================

__device__ __forceinline__ void chacha20_block(const ChaChaKey &key, uint32_t counter, uint32_t n0,
                                               uint32_t n1, uint32_t n2, uint32_t (&out)[16]) {
    chacha_block<20>(key, counter, n0, n1, n2, out);
}
// (hi 2^64 + lo) mod Q for 2^16 <= Q < 2^94: long division in base 2^32 (quotients < 2^32 are
// exact through the double-precision estimate of mod_wide)
__device__ __forceinline__ u128 mod128(uint64_t hi, uint64_t lo, const CrtConst *CC) {
    const u128 Q = CC->Q;
    u128 r = mod_wide((u128)(hi >> 32), Q, CC->invQ, nullptr);
    r = mod_wide((r << 32) | (uint32_t)hi, Q, CC->invQ, nullptr);
    r = mod_wide((r << 32) | (uint32_t)(lo >> 32), Q, CC->invQ, nullptr);
    return mod_wide((r << 32) | (uint32_t)lo, Q, CC->invQ, nullptr);
}
// rows [row0, row0 + R) (row = k * 4 + gadget row): canonical a into acan[r][m], noise into e[r][m].
// One thread per 64-byte block of the a stream (four coefficients); every second thread also takes
// one block of the e stream (eight coefficients).
__global__ void __launch_bounds__(256)
k_keygen_draw(ulonglong2 *__restrict__ acan, int32_t *__restrict__ e,
              const CrtConst *__restrict__ CC, ChaChaKey key, uint32_t noise, uint32_t row0,
              uint32_t R, uint32_t logm) {
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    const uint32_t M = 1u << logm, bpr = M >> 2;  // a-stream blocks per row
    if (t >= R * bpr) return;
    const uint32_t blk = t & (bpr - 1), r = t / bpr;
    uint32_t w[16];
    chacha20_block(key, blk, 1u, row0 + r, 0u, w);
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const uint64_t lo = ((uint64_t)w[4 * q + 1] << 32) | w[4 * q];
        const uint64_t hi = ((uint64_t)w[4 * q + 3] << 32) | w[4 * q + 2];
        const u128 a = mod128(hi, lo, CC);
        acan[(size_t)r * M + 4 * blk + q] = make_ulonglong2((uint64_t)a, (uint64_t)(a >> 64));
    }
    if (blk & 1u) return;
    chacha20_block(key, blk >> 1, 2u, row0 + r, 0u, w);
    const uint64_t span = 2 * (uint64_t)noise + 1;
#pragma unroll
    for (int q = 0; q < 8; q++) {
        const uint64_t d = (((uint64_t)w[2 * q + 1] << 32) | w[2 * q]) % span;
        e[(size_t)r * M + 4 * blk + q] = (int32_t)d - (int32_t)noise;
    }
}

// Residue mod p of a canonical value C < 2^96 given as three 32-bit limbs, lifted to the centred
// representative of C mod Q first when `lift` (C > Q / 2 -> C - Q): |result| < 3.5 * 2^29.
__device__ __forceinline__ int32_t limbs_mod_p(ulonglong2 v, bool lift, const PrimeK &P, const Mod &md) {
    const uint32_t c0 = (uint32_t)v.x, c1 = (uint32_t)(v.x >> 32), c2 = (uint32_t)v.y;
    int32_t r = smontu(c0, P.r1, md) + smontu(c1, P.r2, md) + smontu(c2, P.r3, md);  // each |.| < p
    if (lift) r -= P.qmodp;
    return r;
}

// shat[pi][slot] = NTT(s)[slot] * m^-1 * (M/p)^-1 * R mod p, centred  (s = the secret key, zero padded)
template <int LOGM>
__global__ void __launch_bounds__((NttGeom<LOGM, LOGE>::T))
k_shat(const uint64_t *__restrict__ sk, int32_t *__restrict__ shat, PrimeSet PS, uint32_t n) {
    using G = NttGeom<LOGM, LOGE>;
    constexpr int M = G::M, T = G::T, E = G::E;
    SGFHE_DYN_LDS(uint32_t, lds);
    const int tid = threadIdx.x;
    const uint32_t pi = blockIdx.x;
    const PrimeK P = PS[pi];
    const Mod md = mod_of(P);
    int32_t x[1][E];
#pragma unroll
    for (int e = 0; e < E; e++) {
        const uint32_t idx = tid + T * e;
        x[0][e] = idx < n ? (int32_t)(sk[idx] & 1) : 0;
    }
    ntt_forward<LOGM, 1, LOGE>(x, lds, P.twf, tid, md);
    // kappaR = R^2 m^-1 (M/p)^-1 * R: smont(x, kappaR) = x R^2 m^-1 e; one more Montgomery step
    // with 1 brings it down to x R m^-1 e
#pragma unroll
    for (int e = 0; e < E; e++) {
        int32_t u = smont(x[0][e], P.kappaR, md);
        u = smont(u, 1, md);
        shat[(size_t)pi * M + E * tid + e] = scentre(u, md);
    }
}

// y[r][pi][m] = (M/p)^-1 * (a_r (*) s) mod p (+ hoff), a lifted to (-Q/2, Q/2]
template <int LOGM>
__global__ void __launch_bounds__((NttGeom<LOGM, LOGE>::T))
k_polymul_s(const ulonglong2 *__restrict__ acan, const int32_t *__restrict__ shat,
            uint32_t *__restrict__ y, PrimeSet PS, const CrtConst *__restrict__ CC) {
    using G = NttGeom<LOGM, LOGE>;
    constexpr int M = G::M, T = G::T, E = G::E;
    SGFHE_DYN_LDS(uint32_t, lds);
    const int tid = threadIdx.x;
    const uint32_t npr = PS[0].npr;
    const uint32_t r = blockIdx.x / npr, pi = blockIdx.x % npr;
    const PrimeK P = PS[pi];
    const Mod md = mod_of(P);
    const u128 halfQ = CC->halfQ;
    int32_t x[1][E];
#pragma unroll
    for (int e = 0; e < E; e++) {
        const ulonglong2 v = acan[(size_t)r * M + tid + T * e];
        const u128 C = ((u128)v.y << 64) | v.x;
        x[0][e] = sred(limbs_mod_p(v, C > halfQ, P, md), md);
    }
    ntt_forward<LOGM, 1, LOGE>(x, lds, P.twf, tid, md);
#pragma unroll
    for (int e = 0; e < E; e++)  // |x| < 3.95 * 2^29, |shat| <= p / 2: |product R^-1| < 0.75 * 2^29
        x[0][e] = smont(x[0][e], shat[(size_t)pi * M + E * tid + e], md);
    __syncthreads();
    ntt_inverse<LOGM, 1, LOGE>(x, lds, P.twi, tid, md);
#pragma unroll
    for (int e = 0; e < E; e++)
        y[((size_t)r * npr + pi) * M + tid + T * e] = condsub(sfull(x[0][e], md) + P.hoff, (uint32_t)P.p);
}

// canon[(r * 2 + col)][m]: col 0 = a_r + s_k G[row][0], col 1 = a_r (*) s + e_r + s_k G[row][1]
// (constant-term adds, fhe.jl:195-196); prod holds the canonical a_r (*) s.
__global__ void __launch_bounds__(256)
k_keygen_finish(const ulonglong2 *__restrict__ acan, const ulonglong2 *__restrict__ prod,
                const int32_t *__restrict__ e, const uint64_t *__restrict__ sk,
                ulonglong2 *__restrict__ canon, const CrtConst *__restrict__ CC, uint32_t row0,
                uint32_t R, uint32_t logm) {
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    const uint32_t M = 1u << logm;
    if (t >= R * M) return;
    const uint32_t i = t & (M - 1), r = t >> logm;
    const uint32_t grow = (row0 + r) & 3, kk = (row0 + r) >> 2;
    const u128 Q = CC->Q;
    u128 a = ((u128)acan[t].y << 64) | acan[t].x;
    u128 b = ((u128)prod[t].y << 64) | prod[t].x;
    const int32_t ev = e[t];
    b += ev >= 0 ? (u128)(uint32_t)ev : Q - (u128)(uint32_t)(-ev);
    if (b >= Q) b -= Q;
    if (i == 0 && (sk[kk] & 1)) {  // G = [1 0; B 0; 0 1; 0 B] (fhe.jl:119-122)
        const u128 g = (grow & 1) ? CC->B % Q : (u128)1;
        if (grow < 2) { a += g; if (a >= Q) a -= Q; }
        else { b += g; if (b >= Q) b -= Q; }
    }
    canon[((size_t)r * 2 + 0) * M + i] = make_ulonglong2((uint64_t)a, (uint64_t)(a >> 64));
    canon[((size_t)r * 2 + 1) * M + i] = make_ulonglong2((uint64_t)b, (uint64_t)(b >> 64));
}

// ---- k_key_transform ------------------------------------------------------------------------------
// BootstrapKey.key (fhe.jl:176-201) canonical residues -> device form: centred lift to
// (-Q/2, Q/2], residue mod p_i, scaled by kappa_i, forward NTT, slot order.
//   canon  [npolys][m] 16-byte residues (polys in [k][row][col] order)
//   keyhat [k][NPR][row*2+col][m]
template <int LOGM>
__global__ void __launch_bounds__((NttGeom<LOGM, LOGE>::T))
k_key_transform(const ulonglong2 *__restrict__ canon, int32_t *__restrict__ keyhat, PrimeSet PS,
                const CrtConst *__restrict__ CC, uint32_t poly0, uint32_t *__restrict__ bad) {
    using G = NttGeom<LOGM, LOGE>;
    constexpr int M = G::M, T = G::T, E = G::E;
    SGFHE_DYN_LDS(uint32_t, lds);
    const int tid = threadIdx.x;
    const uint32_t npr = PS[0].npr;
    const uint32_t pl = blockIdx.x / npr;  // polynomial within this staging batch
    const uint32_t pi = blockIdx.x % npr;
    const PrimeK P = PS[pi];
    const Mod md = mod_of(P);
    const u128 halfQ = CC->halfQ;
    int32_t x[1][E];
#pragma unroll
    for (int e = 0; e < E; e++) {
        const ulonglong2 v = canon[(size_t)pl * M + tid + T * e];
        const u128 C = ((u128)v.y << 64) | v.x;
        if (C >= CC->Q) *bad = 1u;  // not a canonical residue: reported by the upload call
        x[0][e] = smont(limbs_mod_p(v, C > halfQ, P, md), P.kappaR, md);  // |.| < 0.72 * 2^29
    }
    ntt_forward<LOGM, 1, LOGE>(x, lds, P.twf, tid, md);
    const uint32_t pg = poly0 + pl;  // global polynomial index = k * 8 + row * 2 + col
    int32_t *dst = keyhat + (((size_t)(pg >> 3) * npr + pi) * 8 + (pg & 7)) * M + E * tid;
#pragma unroll
    for (int h = 0; h < E / 4; h++) {
        int32_t o[4];
#pragma unroll
        for (int t = 0; t < 4; t++) o[t] = scentre(sred(sred_floor(x[0][4 * h + t], md), md), md);  // [-(p-1)/2, (p-1)/2]
        reinterpret_cast<int4 *>(dst)[h] = make_int4(o[0], o[1], o[2], o[3]);
    }
}

// ---- k_key_derive -------------------------------------------------------------------------------------
// The key of a ctx's smaller basis (primes 0 .. nps-1, deterministic flatten) from the key of its larger
// one (primes 0 .. npb-1, randomised flatten): the device form is scaled by (M_rns / p_i)^-1 mod p_i,
// and M_big = M_small * (the extra primes), so keyhat_small = keyhat_big * (product of the extra primes)
// mod p_i -- one constant per prime, no transform.  fac.f[i] = that constant in Montgomery form, centred.
// The result is the centred canonical residue, i.e. byte for byte what k_key_transform writes for the
// smaller basis.  One thread per element of the smaller key: keyhat[k][prime][row * 2 + col][slot].
// (struct KeyFactors: constants.h, where key_factors derives it)
__global__ void __launch_bounds__(256)
k_key_derive(const int32_t *__restrict__ big, int32_t *__restrict__ small, PrimeSet PS, KeyFactors fac,
             uint32_t npb, uint32_t nps, uint32_t logm, size_t total) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const size_t per_prime = (size_t)8 << logm;                 // 8 polynomials of m slots
    const size_t e = t % per_prime;
    const uint32_t i = (uint32_t)((t / per_prime) % nps);
    const size_t k = t / (per_prime * nps);
    const PrimeK P = PS[i];
    const Mod md = mod_of(P);
    const int32_t v = big[(k * npb + i) * per_prime + e];
    small[t] = scentre(sred(smont(v, fac.f[i], md), md), md);
}

// ---- RNS2Number boundary conversions (src/rns.jl, BASELINE.json config 4) --------------------------
// The reference's two-modulus residue type holds a coefficient of Z_Q, Q = m1 m2, as
// (v1, v2) = (x mod m1, x mod m2) (rns.jl:16-18) and converts back with the Fermat idempotents
// c1 = m2^(m1-1), c2 = m1^(m2-1) mod Q: x = (v1 c1 + v2 c2) mod Q (rns.jl:32-40).  With
// c1 = m2 (m2^-1 mod m1) and c2 = m1 (m1^-1 mod m2) that is
//   x = ((v1 i21) mod m1) m2 + ((v2 i12) mod m2) m1,  minus Q if >= Q.
// Both kernels work in place on 16-byte elements ({v1, v2} <-> {x lo, x hi}).
// (struct Rns2Const: constants.h, where rns2_const derives it)
__global__ void __launch_bounds__(256)
k_rns2_to_canon(ulonglong2 *__restrict__ buf, size_t count, Rns2Const rc,
                const CrtConst *__restrict__ CC, uint32_t *__restrict__ bad) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= count) return;
    const ulonglong2 v = buf[t];
    if (v.x >= rc.m1 || v.y >= rc.m2) { *bad = 1u; return; }  // not an RNS2Number of these moduli
    const u128 h1 = mod_wide((u128)v.x * rc.i21, (u128)rc.m1, rc.inv1, nullptr);
    const u128 h2 = mod_wide((u128)v.y * rc.i12, (u128)rc.m2, rc.inv2, nullptr);
    u128 x = h1 * rc.m2 + h2 * rc.m1;
    if (x >= CC->Q) x -= CC->Q;
    buf[t] = make_ulonglong2((uint64_t)x, (uint64_t)(x >> 64));
}
__global__ void __launch_bounds__(256)
k_canon_to_rns2(ulonglong2 *__restrict__ buf, size_t count, Rns2Const rc) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= count) return;
    const ulonglong2 v = buf[t];
    const u128 x = ((u128)v.y << 64) | v.x;  // < Q = m1 m2: both quotients are below 2^47
    buf[t] = make_ulonglong2((uint64_t)mod_wide(x, (u128)rc.m1, rc.inv1, nullptr),
                             (uint64_t)mod_wide(x, (u128)rc.m2, rc.inv2, nullptr));
}

// ---- k_debug_ntt ----------------------------------------------------------------------------------
template <int LOGM>
__global__ void __launch_bounds__((NttGeom<LOGM, LOGE>::T))
k_debug_ntt(const uint32_t *__restrict__ in, uint32_t *__restrict__ out, PrimeSet PS, uint32_t pi,
            uint32_t inverse) {
    using G = NttGeom<LOGM, LOGE>;
    constexpr int T = G::T, E = G::E;
    SGFHE_DYN_LDS(uint32_t, lds);
    const int tid = threadIdx.x;
    const PrimeK P = PS[pi];
    const Mod md = mod_of(P);
    int32_t x[1][E];
    if (!inverse) {
#pragma unroll
        for (int e = 0; e < E; e++) x[0][e] = (int32_t)in[tid + T * e];  // [0, p)
        ntt_forward<LOGM, 1, LOGE>(x, lds, P.twf, tid, md);
#pragma unroll
        for (int e = 0; e < E; e++) out[E * tid + e] = sfull(sred_floor(x[0][e], md), md);
    } else {
#pragma unroll
        for (int e = 0; e < E; e++) x[0][e] = sred((int32_t)in[E * tid + e], md);
        ntt_inverse<LOGM, 1, LOGE>(x, lds, P.twi, tid, md);
#pragma unroll
        for (int e = 0; e < E; e++) out[tid + T * e] = scanon(smont(x[0][e], P.minvR, md), md);
    }
}

}  // namespace sgfhe
