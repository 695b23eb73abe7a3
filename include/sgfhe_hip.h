/*
 * sgfhe_hip.h -- C ABI of libsgfhe_hip.so, the MI355X (gfx950) gate-bootstrap engine.
 *
 * Drop-in boundary for the hot path of nucypher/SGFHE.jl (paths relative to /root/reference):
 * the reference has no FFI of its own (pure Julia); each entry point
 * below names the Julia function or data structure whose work it takes over, and
 * INTEGRATION.md shows the `ccall` stub a maintainer adds on the Julia side.
 *
 * Conventions
 *   - every function returns an int32 status: 0 = OK, negative = sgfhe_status error
 *   - no exception crosses the boundary; sgfhe_last_error_string() explains the last failure
 *   - the caller owns every buffer it passes; the library owns device memory behind the handle
 *   - a ctx is bound to one device; any number of ctxs may share a device.  Every entry point
 *     that takes a ctx locks it for the duration of the call, so a ctx may be shared by host
 *     threads (calls on one ctx are serialised; calls on different ctxs run concurrently).
 *     That includes the asynchronous entry point sgfhe_bootstrap_batch_device: the work of
 *     successive calls on one ctx is ordered on the device in the order the calls were made,
 *     whatever stream each call names (each call's first kernel waits, on the device, for the
 *     previous call's last one: the ctx owns the work buffers every call uses), so two threads
 *     or two streams sharing a ctx get the bytes of the same calls made one after the other
 *     (the reference call is pure, src/fhe.jl:608-621).  Callers that want their calls to OVERLAP on
 *     the device -- Julia tasks each running bootstrap(bkey, ...) on one key -- take one clone of the
 *     ctx each (sgfhe_ctx_clone, ABI revision 7): clones share the device key and constants and own
 *     their work buffers and streams
 *   - residues mod Q cross the boundary as canonical representatives in [0, Q), little-endian
 *     `limbs` x uint64 each, limbs = 2 (16 bytes, the reference's UInt128 storage width) unless
 *     stated otherwise; LWE words over Z_r are one uint64 each, exactly the memory of
 *     `Vector{ModUInt{UInt64, r}}` (src/fhe.jl:206-209)
 */
#ifndef SGFHE_HIP_H
#define SGFHE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sgfhe_ctx sgfhe_ctx;

typedef enum {
    SGFHE_OK = 0,
    SGFHE_ERR_INVALID_ARG = -1,   /* NULL pointer, size mismatch, malformed parameter set */
    SGFHE_ERR_UNSUPPORTED = -2,   /* parameter set outside what the engine implements */
    SGFHE_ERR_NO_DEVICE = -3,     /* no usable gfx950 device / HIP runtime failure at start-up */
    SGFHE_ERR_HIP = -4,           /* a HIP runtime call failed (see last_error_string) */
    SGFHE_ERR_NO_KEY = -5,        /* bootstrap requested before a bootstrap key was uploaded */
    SGFHE_ERR_OOM = -6            /* host or device allocation failed */
} sgfhe_status;

/*
 * Scheme parameters: the fields of `Params` (src/fhe.jl:27-41) that the hot path reads.
 * Params(n) (src/fhe.jl:43-97) fixes r = 16 n, m = r / 2, ell = 2 (src/fhe.jl:576),
 * B = 35 r^2 n, DQ_tilde = Q / 8; synthetic sets (BASELINE.json configs 3 / 4) choose their own
 * Q and B with the same structure.  Q need not be prime: the engine computes the exact integer
 * negacyclic product in a residue number system of word-size NTT primes and reduces mod Q.
 */
typedef struct {
    uint64_t n;           /* LWE dimension (polynomial length of the small ring) */
    uint64_t r;           /* LWE modulus, power of two, r = 2 m */
    uint64_t m;           /* bootstrap polynomial length, power of two, 2^6 .. 2^14 */
    uint64_t ell;         /* gadget decomposition length; must be 2 */
    uint64_t Q[2];        /* bootstrap modulus, Q < 2^94 */
    uint64_t B[2];        /* gadget base, B^2 >= Q, B < 2^47 */
    uint64_t DQ_tilde[2]; /* Q / 8 for Params(n) */
} sgfhe_params;

/* flags of sgfhe_bootstrap_batch* */
#define SGFHE_FLAG_RAW_MODQ 1u /* return _bootstrap_internal's LWEs over Z_Q (fhe.jl:559-595) as
                                  16-byte residues instead of ModRed words (fhe.jl:616-618) */
#define SGFHE_FLAG_RAW_RNS2 2u /* with RAW_MODQ: every residue leaves as the RNS2Number limb pair
                                  (x mod m1, x mod m2) (src/rns.jl:16-18) of the moduli given to
                                  sgfhe_bkey_upload_rns2, instead of {lo, hi} of x */

/* Library / build information: "sgfhe_hip <version> gfx950". */
const char *sgfhe_version(void);
/* Revision of this header the library was built against.  A binding compares it with the
 * SGFHE_ABI_VERSION it was written for and refuses a stale library (julia/SGFHEHip.jl __init__,
 * sgfhe.jl_amd/_lib.py).  Bumped whenever a signature, a struct layout, a flag value or the
 * meaning of an argument changes. */
#define SGFHE_ABI_VERSION 7u
uint32_t sgfhe_abi_version(void);
/* Identity of the kernel sources the library was compiled from: the first 16 hex digits of the
 * SHA-256 over csrc/{*.h, *.hip} (in file-name order), followed by "+<flags>" when the build used
 * extra -D flags (timing-only ablation builds).  bench.py quotes profile counters only when they
 * were collected on a library with the same id. */
const char *sgfhe_build_id(void);

/* Create an engine for one parameter set on HIP device `device`.
 * Replaces: the type-level set-up Julia does when `Params(n)` fixes MgModUInt{LargeType, Q}
 * (src/fhe.jl:71-85,102-104) -- here: RNS primes, twiddle tables, CRT and flatten constants. */
int32_t sgfhe_ctx_create(const sgfhe_params *p, int device, sgfhe_ctx **out);
/* The same with creation flags.
 * Both flatten modes of the reference (`rng = nothing` and `rng::AbstractRNG` of bootstrap /
 * pack_encrypted_bits, src/utils.jl:155-189 and :198-241) are available on every ctx.  The digits
 * of the randomised one are four times larger, and at Params(1024) that takes a sixth 29-bit RNS
 * prime: such a ctx keeps a basis per mode (ABI revision 6) -- the key in both forms (1.34 + 1.61 GB
 * at Params(1024); the five-prime form is derived from the six-prime one on the device), constants
 * for both -- so the deterministic mode runs on five primes whatever the ctx may be asked later, and
 * sgfhe_set_random_flatten switches.  The other Params(n) need one basis for both.
 *   SGFHE_CTX_DETERMINISTIC_ONLY  the smaller basis only (no second key form): on such a ctx
 *       sgfhe_set_random_flatten(enable = 1) fails with SGFHE_ERR_UNSUPPORTED where the randomised
 *       mode would need the extra prime.  Its key blob is the smaller basis's.
 *   SGFHE_CTX_RANDOM_FLATTEN      accepted and without effect (up to ABI revision 5 it asked for the
 *       larger basis, which then also served the deterministic mode, about 20 % slower). */
#define SGFHE_CTX_RANDOM_FLATTEN 1u
#define SGFHE_CTX_DETERMINISTIC_ONLY 2u
int32_t sgfhe_ctx_create_ex(const sgfhe_params *p, int device, uint32_t flags, sgfhe_ctx **out);
/*
 * A second ctx on the same device, parameter set and KEY, for an independent caller (ABI revision 7).
 * The reference call is pure (src/fhe.jl:608-621): any number of Julia tasks may run
 * bootstrap(bkey, ...) on one BootstrapKey side by side.  Calls on ONE ctx are serialised and ordered
 * on the device, because the ctx owns the work buffers every call uses; a clone is what gives a second
 * caller its own: it SHARES with `ctx` everything a bootstrap only reads -- the device key in every
 * form (1.34 + 1.61 GB at Params(1024): not copied), twiddle tables, per-prime and CRT constants -- and
 * OWNS its lanes' work buffers (allocated by its first call, sized by its largest), streams, events,
 * host staging, flatten mode (deterministic to begin with; its own ChaCha key and call counter), error
 * string and lock.  The scheduling knobs (sgfhe_set_chunk / _lanes / _small_batch_max) are inherited as
 * they stand.  Calls on different clones are independent -- each gives the bytes the same call gives on
 * `ctx` -- and small host-pointer calls made at the same time are gathered into one launch chain
 * (sgfhe_set_coalesce below), which is how eight callers get 5.8 (Params(1024)) to 6.7 (Params(512)) times one
 * caller's rate.
 * `ctx` must hold a key (SGFHE_ERR_NO_KEY otherwise).  While a key is shared -- by `ctx` and at least
 * one clone, or by clones alone -- it is read-only: sgfhe_bkey_upload / _upload_rns2 / _generate /
 * _import_device_form on any of the sharers fail with SGFHE_ERR_INVALID_ARG (export is allowed).  The
 * shared memory is freed with the last ctx that holds it, so `ctx` and its clones may be destroyed in
 * any order; every one of them is destroyed with sgfhe_ctx_destroy.
 * As with sgfhe_ctx_create, *out is set even when the call fails after allocating it (read the error,
 * then destroy it).
 */
int32_t sgfhe_ctx_clone(sgfhe_ctx *ctx, sgfhe_ctx **out);
/*
 * Gathering of small calls across the ctxs that share a key (ABI revision 7).  Separate launch chains overlap only so
 * far on this device (four hardware queues: 1.8 x one caller's rate at two callers, 3 x at four and beyond), while ONE
 * chain of g gates costs little more than a chain of one (Params(1024): 15 ms for 1 gate, 21 ms for 8, 27 ms for 16).
 * So sgfhe_bootstrap_batch calls of at most `req_max` gates (default 32) made at the same time on ctxs that share a
 * key -- a ctx and its clones, each driven by its own host thread -- are run as ONE call: the caller that finds no combined call in flight takes
 * every request waiting (up to `gates_max` gates, default 256), runs them as one batch on its own ctx and hands each
 * caller its rows; callers arriving meanwhile form the next round, whose leader waits up to `window_us` (default 300)
 * for as many callers as the last two rounds had.  A caller on its own never waits, and a ctx without clones is not
 * affected at all.  A row of the result does not depend on the rows beside it, so every caller gets the bytes its
 * call gives alone -- with the randomised flatten too: every row of a gathered call draws from the stream of the ctx
 * it came in on (that ctx's key, the number of its call, the row's index in its call), and deterministic and
 * randomised requests form separate rounds.  So do SGFHE_FLAG_RAW_RNS2 requests of ctxs whose RNS2 limb moduli differ
 * (a clone inherits them; sgfhe_rns2_convert sets them on one ctx): each gets its own (v1, v2) order, and a ctx without
 * moduli its own SGFHE_ERR_INVALID_ARG, whoever calls beside it.  The asynchronous entry point (sgfhe_bootstrap_batch_device) and
 * sgfhe_pack_encrypted_bits are never gathered.
 * The setting belongs to the shared key: it applies to every ctx that shares it.  enable = 0 switches gathering off
 * (SGFHE_COALESCE=0 in the environment does the same at ctx creation); the other arguments are then ignored.
 * sgfhe_coalesce_stats: stats[4] = {combined calls run, requests served, gates, most requests in one call}.
 */
int32_t sgfhe_set_coalesce(sgfhe_ctx *ctx, int enable, uint32_t req_max, uint32_t gates_max, uint32_t window_us);
int32_t sgfhe_coalesce_stats(sgfhe_ctx *ctx, uint64_t *stats, int reset);
int32_t sgfhe_ctx_destroy(sgfhe_ctx *ctx);
const char *sgfhe_last_error_string(const sgfhe_ctx *ctx);

/* Batch-scheduling knobs.  chunk: bootstraps that move through the k-loop in lock-step
 * (rounded up to a multiple of 8; a chunk's buffers must stay below 4 GiB).  0 = automatic: a size
 * near the Infinity Cache budget (256 per lane at Params(1024)), and with two lanes a batch above
 * 48 gates is cut into an even number of equal chunks, so that both lanes carry the same load.
 * lanes: 2 (default) runs pairs of chunks on two HIP streams, so that the memory-bound CRT kernel
 * of one chunk runs beside the arithmetic-bound external product of the other (+2 ... 5 % at
 * Params(1024), profiles/r03_exp_lanes_sweep.txt); 1 runs the chunks of a batch one after the
 * other, with twice the default chunk.  Every setting gives bit-identical results, in both
 * flatten modes. */
int32_t sgfhe_set_chunk(sgfhe_ctx *ctx, uint32_t chunk);
/* Chunks of at most this many bootstraps (default 24, 16 at m = 16384; 0 = never, at most 256) run the k-loop in
 * its small-batch form: 6 workgroups per (bootstrap, RNS prime) and three launches per iteration
 * instead of 1 and two, which shortens the serial chain a single bootstrap() call waits for.
 * Same results bit for bit. */
int32_t sgfhe_set_small_batch_max(sgfhe_ctx *ctx, uint32_t max_bootstraps);
int32_t sgfhe_set_lanes(sgfhe_ctx *ctx, uint32_t lanes);

/*
 * Flatten mode of the external product.  enable = 0 (default): deterministic flatten, the
 * `rng = nothing` branch (src/utils.jl:155-189), bit-exact with the reference.  enable = 1:
 * randomised flatten, the `rng::AbstractRNG` branch (src/utils.jl:198-241): every digit gets a
 * uniform v in [-3B/2, 3B/2] drawn from a ChaCha counter stream (the RFC 8439 block function with
 * 8 rounds, "ChaCha8") keyed with `key32`; digits lie in (-2B, 2B].  The draw of a coefficient is
 * addressed by (coefficient, iteration, index of the bootstrap in the call, number of the call
 * since this function): results do not depend on chunk size, lanes or the small-batch threshold,
 * and oracle/bigint_oracle.py reproduces them bit for bit.  They decrypt like the reference's
 * but are not bit-comparable with it (the stream of the caller's Julia rng cannot be reproduced:
 * a host draws the 32 key bytes from that rng instead, julia/SGFHEHip.jl).  Applies to later
 * bootstrap / pack calls, on every ctx not created with SGFHE_CTX_DETERMINISTIC_ONLY (see
 * sgfhe_ctx_create_ex; a ctx with a basis per mode switches to the other one, queued work is not
 * affected).  Every Params(n) the reference can build is covered, n = 64 ... 2048
 * (B up to 2^47: above 2^46 the stored digits take a third plane of the digit record).
 * sgfhe_set_random_flatten_key takes the full 32-byte key (the reference draws every v_i from the
 * caller's rng, src/utils.jl:229: with a key from a cryptographic source the perturbations are
 * cryptographically strong); sgfhe_set_random_flatten is the short form for tests and benchmarks,
 * key = `seed` as 32 little-endian bytes (64 bits of entropy).  (ABI revisions up to 4 drew from
 * Philox4x32-10 keyed by 64 bits.)
 */
int32_t sgfhe_set_random_flatten(sgfhe_ctx *ctx, int enable, uint64_t seed);
int32_t sgfhe_set_random_flatten_key(sgfhe_ctx *ctx, int enable, const uint8_t *key32);

/*
 * Upload a bootstrap key.  `canonical` (host memory) holds value.(p.coeffs) of
 * `BootstrapKey.key` (src/fhe.jl:176-201) in index order [k in 0..n)[row in 0..4)[col in 0..2)
 * [coef in 0..m), each residue 2 x uint64 little-endian; n_words = n * 8 * m * 2.
 * One-time: converts to the device form (per-prime forward NTT, Montgomery-scaled).
 */
int32_t sgfhe_bkey_upload(sgfhe_ctx *ctx, const uint64_t *canonical, size_t n_words);

/*
 * Same for a key held as RNS2Number{UInt64, M1, M2} pairs (src/rns.jl:8-24; type_Q of
 * Scheme2, src/fhe2.jl:76): each coefficient is (v1, v2) = (x mod m1, x mod m2).  The boundary
 * conversion is the CRT of src/rns.jl:32-40, done on the device; requires m1 * m2 == Q, both
 * prime and below 2^47.  A limb outside [0, m_i) is SGFHE_ERR_INVALID_ARG.
 */
int32_t sgfhe_bkey_upload_rns2(sgfhe_ctx *ctx, const uint64_t *pairs, size_t n_words, uint64_t m1,
                               uint64_t m2);
/* The two conversions of src/rns.jl on `count` coefficients (host pointers, run on the device):
 * to_pairs = 0: (v1, v2) -> canonical x = (v1 c1 + v2 c2) mod (m1 m2) (rns.jl:32-40);
 * to_pairs = 1: canonical x -> (x mod m1, x mod m2) (rns.jl:16-18).  m1 m2 must equal Q. */
int32_t sgfhe_rns2_convert(sgfhe_ctx *ctx, int to_pairs, const uint64_t *in, size_t count,
                           uint64_t m1, uint64_t m2, uint64_t *out);

/*
 * BootstrapKey(rng, sk) (src/fhe.jl:181-201) generated on the device, directly in device form:
 * for every k and gadget row a uniform a_row in [0, Q)^m, noise e_row in [-noise, noise]^m
 * (the reference uses noise = n, src/fhe.jl:194), b_row = a_row * s + e_row, plus s_k G on the
 * constant terms.  sk: n words, bit 0 of each is the key bit (PrivateKey.key, src/fhe.jl:130-138).
 * Randomness: ChaCha20 (RFC 8439) keyed with the 32-byte `seed`, separate counter-addressed
 * streams for the uniform polynomials and for the noise of every key row (layout in
 * csrc/kernels.h).  The key's entropy is the seed's: pass 32 bytes from a cryptographic generator.
 */
int32_t sgfhe_bkey_generate(sgfhe_ctx *ctx, const uint64_t *sk, size_t n_sk, const uint8_t *seed,
                            uint32_t noise);

/* Device-form key blob (for the one-time RCCL broadcast rank 0 -> peers). */
int32_t sgfhe_bkey_device_form_bytes(const sgfhe_ctx *ctx, size_t *bytes);
int32_t sgfhe_bkey_export_device_form(sgfhe_ctx *ctx, void *dst_device);
int32_t sgfhe_bkey_import_device_form(sgfhe_ctx *ctx, const void *src_device);

/*
 * bootstrap(bkey, nothing, enc_bit1, enc_bit2) (src/fhe.jl:608-621) over a batch.
 *   a1, a2 : [batch][n] uint64 in [0, r)   (EncryptedBit.lwe.a, src/fhe.jl:206-209,272-274)
 *   b1, b2 : [batch]    uint64 in [0, r)   (EncryptedBit.lwe.b)
 *   out    : [batch][3][n + 1] uint64: a[0..n) then b; gate order AND, OR, XOR
 *            (with SGFHE_FLAG_RAW_MODQ: [batch][3][n + 1][2], residues mod Q)
 * Deterministic flatten (rng = nothing, src/utils.jl:155-189) unless sgfhe_set_random_flatten[_key]
 * selected the other.  Host pointers; synchronous.  The arrays travel chunk by chunk through
 * page-locked staging buffers the ctx keeps (up to 1 GiB each; sgfhe_release_host_staging frees
 * them): a chunk's inputs go up while the chunks before it compute and its results come down while
 * the chunks after it compute, so a large batch runs at the rate of device-resident buffers
 * (larger arrays, and SGFHE_HOST_PIN=0 in the environment, are copied directly before and after).
 * A caller in a loop should keep its `out` buffer: releasing a multi-megabyte
 * array between calls (munmap) can stall the next call's kernels by tens of milliseconds.
 * SGFHE_DEBUG_IO=1 in the environment prints the phases of every call to stderr.
 */
int32_t sgfhe_bootstrap_batch(sgfhe_ctx *ctx, const uint64_t *a1, const uint64_t *b1,
                              const uint64_t *a2, const uint64_t *b2, size_t batch, uint64_t *out,
                              uint32_t flags);

/* Same with every buffer resident in device memory; asynchronous.  `stream` (a hipStream_t) is the
 * stream the call's work is queued on, NULL = the ctx's own: `out` is complete when that stream
 * reaches the end of the call's work (ordinary stream order for whatever the caller queues next on
 * it), and the inputs must stay valid until then.  Calls on one ctx do not overlap on the device:
 * a call's work starts after the work of every earlier call on this ctx, on any stream, has
 * finished (see the conventions above).  sgfhe_sync waits on the host for all work queued on the
 * ctx. */
int32_t sgfhe_bootstrap_batch_device(sgfhe_ctx *ctx, const uint64_t *a1, const uint64_t *b1,
                                     const uint64_t *a2, const uint64_t *b2, size_t batch,
                                     uint64_t *out, uint32_t flags, void *stream);
int32_t sgfhe_sync(sgfhe_ctx *ctx);
/* Frees the staging buffers sgfhe_bootstrap_batch keeps on the ctx (device and page-locked host
 * memory, sized by the largest batch seen), the wire table and call staging of sgfhe_circuit_run[_ct], the raw
 * output table of SGFHE_CIRCUIT_PACK_DIRECT, the tables of the noise probe, and the work buffers of the packing path (sgfhe_pack_encrypted_bits,
 * sgfhe_pack_lwe_modq, the pack stage of sgfhe_circuit_run_ct[_ex]); the next call allocates them again. */
int32_t sgfhe_release_host_staging(sgfhe_ctx *ctx);

/*
 * external_product(nothing, a, b, A, Val(B), Val(2)) (src/fhe.jl:519-530), the operation
 * test/internals.test.jl:144-166 checks.  a, b: [m][2]; A: [4][2][m][2] (row-major A[row][col]);
 * a_res, b_res: [m][2].  Host pointers; synchronous.  Parity / debug hook.
 */
int32_t sgfhe_external_product(sgfhe_ctx *ctx, const uint64_t *a, const uint64_t *b,
                               const uint64_t *A, uint64_t *a_res, uint64_t *b_res);

/*
 * One k-loop iteration on caller-chosen operands, exactly as the hot path runs it
 * (src/fhe.jl:580-581): (a, b) <- external_product(nothing, a, b, (x^j - 1) C .+ G, Val(B), Val(2))
 * = (a, b) + (x^j - 1) sum_row flatten(a, b)_row (*) C[row], through k_flatten_canon -> k_extprod
 * (with the rotation) -> k_crt_acc.  a, b: [m][2]; C: [4][2][m][2] canonical residues (one key
 * slice); j in [0, 2 m).  Host pointers; synchronous.  Parity / debug hook: lets a test drive the
 * exact-integer CRT to the bound it is sized for (digits +-B/2, key residues +-Q/2, j = m).
 */
int32_t sgfhe_debug_cmux(sgfhe_ctx *ctx, const uint64_t *a, const uint64_t *b, const uint64_t *C,
                         uint64_t j, uint64_t *a_res, uint64_t *b_res);

/*
 * pack_encrypted_bits(bkey, nothing, enc_bits) (src/fhe.jl:660-696, with
 * shortened_external_product :632-641): `count` groups of n LWEs each -> `count` RLWE
 * ciphertexts over Z_r.
 *   a : [count][n][n] uint64, b : [count][n] uint64   (the n EncryptedBits of every group)
 *   out_w, out_v : [count][m] uint64 in [0, r)         (Ciphertext.rlwe.a / .b coefficients)
 * Runs count * n gate bootstraps (trivial encryption of 1 paired with every bit, AND branch,
 * un-reduced), then the n half-width external products against the key on the device.
 * Flatten mode: the one sgfhe_set_random_flatten selected for this ctx, for the gate bootstraps
 * and for the flatten of every as_i alike (the reference passes the same `rng` to both,
 * src/fhe.jl:673,683-684): deterministic by default.  Host pointers; synchronous.
 */
int32_t sgfhe_pack_encrypted_bits(sgfhe_ctx *ctx, const uint64_t *a, const uint64_t *b,
                                  size_t count, uint64_t *out_w, uint64_t *out_v);
/*
 * The tail of pack_encrypted_bits (src/fhe.jl:675-695) on LWEs that are already over Z_Q: the n half-width
 * external products, the sums and the ModRed, without the n refresh bootstraps of fhe.jl:669-673.  Those turn an
 * LWE over Z_r into _bootstrap_internal's LWE over Z_Q (fhe.jl:585-594); a bit that has just left a gate
 * bootstrap is such an LWE already (sgfhe_bootstrap_batch with SGFHE_FLAG_RAW_MODQ).
 *   lwe          : [count][n][n + 1][2] uint64: for every bit a[0..n) then b, canonical 16-byte residues -- one
 *                  gate's rows of a SGFHE_FLAG_RAW_MODQ result
 *   out_w, out_v : [count][m] uint64 in [0, r)
 * sgfhe_pack_encrypted_bits(a, b) equals this call on the AND rows of
 * sgfhe_bootstrap_batch(a1 = 0, b1 = Dr, a, b, SGFHE_FLAG_RAW_MODQ) in the deterministic mode.  Host pointers;
 * synchronous; upload, tail and download run on the ctx stream.  SGFHE_ERR_NO_KEY as elsewhere; a residue that
 * is not below Q is SGFHE_ERR_INVALID_ARG, before anything is written; SGFHE_ERR_UNSUPPORTED where
 * sgfhe_pack_encrypted_bits returns it.
 * Flatten mode: the ctx's present one.  Randomised: the call takes one call number of the ctx's draw stream,
 * and ciphertext `ct` draws for the flatten of as_i as in sgfhe_pack_encrypted_bits (y = 2^31 | i, z = ct); no
 * bootstrap draws are consumed.
 */
int32_t sgfhe_pack_lwe_modq(sgfhe_ctx *ctx, const uint64_t *lwe, size_t count, uint64_t *out_w, uint64_t *out_v);

/* Parity / debug hook: run the first n_iters iterations of the k-loop (src/fhe.jl:579-582) and
 * return the accumulator pair (a, b) as canonical residues, acc: [batch][2][m][2]. */
int32_t sgfhe_debug_accumulators(sgfhe_ctx *ctx, const uint64_t *a1, const uint64_t *b1,
                                 const uint64_t *a2, const uint64_t *b2, size_t batch,
                                 uint64_t n_iters, uint64_t *acc);

/* Parity / debug hook: the stored digit planes after n_iters iterations, i.e. the flatten result
 * (src/utils.jl:155-241) the next external product will consume: digits [batch][2][2][m] uint64,
 * index order (accumulator c: 0 = a, 1 = b)(digit i)(coefficient).  Stored value e_i = u_i + s
 * with s = B/2 - 1 (even B) or (B - 1)/2 and u_i the reference's i-th flatten output taken as a
 * signed integer, u_i in (-B/2, B/2]; in the randomised mode e_i = u_i + s + xmax,
 * xmax = 3 (B / 2), u_i in (-2B, 2B] (test/internals.test.jl:50-66).  sum_i u_i B^i == acc mod Q. */
int32_t sgfhe_debug_digits(sgfhe_ctx *ctx, const uint64_t *a1, const uint64_t *b1,
                           const uint64_t *a2, const uint64_t *b2, size_t batch, uint64_t n_iters,
                           uint64_t *digits);

/* Parity / debug hook: flatten_poly(nothing, ., Val(B), Val(2)) (src/utils.jl:155-189,253-264) of
 * two polynomials on its own (k_flatten_canon): values [2][m][2] canonical residues ->
 * digits [2][2][m] uint64 in the stored form of sgfhe_debug_digits (e_i = u_i + s).  Host pointers. */
int32_t sgfhe_debug_flatten(sgfhe_ctx *ctx, const uint64_t *values, uint64_t *digits);

/*
 * Parity / debug hook: one k-loop step (external product, then CRT + flatten) from caller-chosen stored digits,
 * through the function every bootstrap call runs per iteration, so the kernels are the ones a real call of `gates`
 * bootstraps takes in the ctx's present flatten mode and knob settings (throughput, small, quarter or fused quarter
 * form).
 *   digits     : [gates][2][2][m] uint64, the stored form of sgfhe_debug_digits (in the randomised mode with the draws)
 *   C          : [4][2][m][2] canonical residues, one key slice, as in sgfhe_debug_cmux
 *   j          : [gates] rotation amounts in [0, 2 m): u.a[k] of every gate
 *   k          : iteration index in [0, n); the randomised flatten draws with tag k + 1, gate b as bootstrap b of one
 *                call of the ctx's draw stream (the call takes one call number, as a bootstrap call does)
 *   digits_out : [gates][2][2][m] uint64, the stored digits of acc + (x^j - 1) sum_row u_row (*) C[row] after the step
 *   ext_name, crt_name : the kernels the step launched, as a kernel trace names them ("a+b" for a pair of launches)
 * Needs no key.  Host pointers; synchronous.  SGFHE_ERR_INVALID_ARG, before anything is queued or a call number taken:
 * a null pointer, gates = 0 or more than one chunk of the ctx, k >= n, a j >= 2 m, a key residue >= Q, or a digit pair
 * that no flatten of the present mode stores: e_lo <= B - 1 + 2 xmax rnd and e_hi <= floor((Q - 1) / B) + 2 xmax rnd
 * (xmax = 3 (B / 2), rnd = 1 in the randomised mode, else 0), and in the deterministic mode e_lo + e_hi B < Q.
 */
int32_t sgfhe_debug_kloop_step(sgfhe_ctx *ctx, const uint64_t *digits, const uint64_t *C, const uint32_t *j,
                               size_t gates, uint32_t k, uint64_t *digits_out, char *ext_name, size_t ext_cap,
                               char *crt_name, size_t crt_cap);

/*
 * Parity / debug hook: the entry of one chunk (k_init) from caller-chosen rows, through the function every bootstrap
 * call runs before its k-loop: the first digits and the rotation amounts the k-loop starts from, in the ctx's present
 * flatten mode.
 *   a1, a2 : [rows][n], b1, b2 : [rows] uint64 over Z_r, as in sgfhe_bootstrap_batch (u = lwe1 + lwe2 mod r)
 *   lut    : NULL, or [rows] uint32 descriptor words as a level call of a circuit carries them: 0 for a row of the
 *            classic path, 0x100 | truth table for a LUT row, which starts at amplitude DQ_tilde >> 2
 *   digits : [rows][2][2][m] uint64, the stored form of sgfhe_debug_digits: a = 0 and b = x^(-u.b) t DQ_tilde flattened
 *            -- what sgfhe_debug_digits returns at n_iters = 0 for the same rows and call number
 *   ua     : [rows][n] uint32, u.a of every row in [0, r)
 * The chunk is padded to a multiple of 8 rows as in a call; the padding rows are not returned.  In the randomised
 * mode row b draws (tag 0) as bootstrap b of one call of the ctx's draw stream, and the entry takes one call number,
 * as a bootstrap call does.  Needs no key.  Host pointers; synchronous.  SGFHE_ERR_INVALID_ARG, before anything is
 * queued or a call number taken: a null pointer (lut excepted), rows = 0 or more than one chunk of the ctx, a
 * descriptor word that is neither 0 nor 0x100 | table, or a word of a LUT row that is not below r (as the LUT
 * entries refuse it; the rows of the classic path are taken mod r, as sgfhe_bootstrap_batch takes them).
 */
int32_t sgfhe_debug_chunk_entry(sgfhe_ctx *ctx, const uint64_t *a1, const uint64_t *b1, const uint64_t *a2,
                                const uint64_t *b2, size_t rows, const uint32_t *lut, uint64_t *digits, uint32_t *ua);

/*
 * Parity / debug hook: the exit of one chunk (k_final, k_final_lut, k_final_lut_multi, the RNS2 conversion) from
 * caller-chosen stored digits, through the function every bootstrap call runs behind its k-loop: the result rows as
 * a real call of that kind leaves them, in the ctx's present flatten mode.
 *   digits   : [rows][2][2][m] uint64, the stored form of sgfhe_debug_digits (in the randomised mode with the draws)
 *   lut      : NULL, or [rows] uint32 descriptor words (0: a row of the classic path, 0x100 | truth table: a LUT row,
 *              as in sgfhe_debug_chunk_entry).  Classic rows leave as those of sgfhe_bootstrap_batch, LUT rows as those
 *              of sgfhe_bootstrap_lut_batch, over what the classic extraction wrote for them; with every row a LUT
 *              row the classic extraction is skipped, as in sgfhe_bootstrap_lut_batch.
 *   tables   : NULL, or [rows][n_tables] truth tables, n_tables in 1..SGFHE_LUT_MAX_TABLES: a LUT family, every row a
 *              LUT row, the rows of sgfhe_bootstrap_lut_multi_batch.  Not together with `lut`; n_tables is read only
 *              with `tables`.
 *   flags    : 0, SGFHE_FLAG_RAW_MODQ, or (no LUT rows, RNS2 moduli set) SGFHE_FLAG_RAW_MODQ | SGFHE_FLAG_RAW_RNS2
 *   out      : [rows][3][n + 1] uint64 (with `tables`: [rows][n_tables][3][n + 1]); x2 words with SGFHE_FLAG_RAW_MODQ
 *   acc      : NULL, or [rows][2][m][2]: the accumulators the digits store, canonical residues, as
 *              sgfhe_debug_accumulators returns them
 * Needs no key and draws nothing: the call takes no call number of the draw stream.  Host pointers; synchronous.
 * SGFHE_ERR_INVALID_ARG, before anything is queued: a null ctx, digits or out; rows = 0 or more than one chunk of the
 * ctx; a digit pair that no flatten of the present mode stores (the rule of sgfhe_debug_kloop_step); `lut` and `tables`
 * together; n_tables outside 1..SGFHE_LUT_MAX_TABLES; a descriptor word that is neither 0 nor 0x100 | table; an
 * unknown flag; SGFHE_FLAG_RAW_RNS2 without SGFHE_FLAG_RAW_MODQ, on a ctx without RNS2 moduli, or with `lut` or `tables`.
 * The wire-table form of a circuit's LUT families (sgfhe_circuit_create_lut_multi) is not reached from here.
 */
int32_t sgfhe_debug_chunk_exit(sgfhe_ctx *ctx, const uint64_t *digits, size_t rows, const uint32_t *lut,
                               const uint8_t *tables, size_t n_tables, uint32_t flags, uint64_t *out, uint64_t *acc);

/* Parity / debug hook: negacyclic NTT of one polynomial modulo RNS prime `prime_index`.
 * in/out: [m] uint32 residues; forward maps natural order to the engine's slot order,
 * inverse maps back (and divides by m).  Host pointers. */
int32_t sgfhe_debug_ntt(sgfhe_ctx *ctx, uint32_t prime_index, int inverse, const uint32_t *in,
                        uint32_t *out);
/* Number of RNS primes and their values (primes[] must hold 8 entries). */
int32_t sgfhe_debug_primes(const sgfhe_ctx *ctx, uint32_t *count, uint32_t *primes);

/*
 * The ciphertext plumbing either side of the path, on the host: no
 * device, no ctx; `p` supplies n, r = 2 m (t = log2 r - 1, Dr = r / 4).  Polynomials over Z_r
 * are arrays of uint64 in [0, r) (the memory of Polynomial{ModUInt{UInt64, r}}), bit arrays are
 * one uint8 per bit, bit matrices [rows][n] row-major.  Every function is pure: the random draws
 * of the reference (src/fhe.jl:315,319) are arguments, so the caller keeps its own generator.
 */
/* deterministic_expand(params, u) (src/fhe.jl:304-307): u[n] seed bits -> a[n] over Z_r.
 * prng_expand (src/utils.jl:63-68) is built on SHAKE-256 here, the primitive the reference names
 * as intended (utils.jl:64); the reference itself seeds a MersenneTwister with hash(seq). */
int32_t sgfhe_host_deterministic_expand(const sgfhe_params *p, const uint8_t *u, uint64_t *a);
/* _encrypt_private(key, rng, message) (src/fhe.jl:310-328) given its draws u[n] (bits) and
 * w[n] in [-Dr/8, Dr/8]: sk[n] key bits (bit 0 of each word), message[n] bits -> RLWE (a, b). */
int32_t sgfhe_host_encrypt_private(const sgfhe_params *p, const uint64_t *sk, const uint8_t *u,
                                   const int64_t *w, const uint8_t *message, uint64_t *a, uint64_t *b);
/* The v of encrypt_optimal(key::PrivateKey, ...) (src/fhe.jl:339-345): b[n] -> v[5][n] bits. */
int32_t sgfhe_host_pack_private(const sgfhe_params *p, const uint64_t *b, uint8_t *v);
/* normalize_ciphertext(::PrivateEncryptedCiphertext) (src/fhe.jl:354-359): (u[n], v[5][n]) -> (a, b). */
int32_t sgfhe_host_normalize_private(const sgfhe_params *p, const uint8_t *u, const uint8_t *v,
                                     uint64_t *a, uint64_t *b);
/* split_ciphertext(ct) (src/fhe.jl:287-290, extract :237-244) of an RLWE with polynomials of
 * length N = n (PackedCiphertext) or N = m (Ciphertext): lwe_a[n][n], lwe_b[n] -- the inputs of
 * sgfhe_bootstrap_batch. */
int32_t sgfhe_host_split_ciphertext(const sgfhe_params *p, const uint64_t *a, const uint64_t *b,
                                    size_t N, uint64_t *lwe_a, uint64_t *lwe_b);
/* decrypt(key, ::EncryptedBit) (src/fhe.jl:504-507) for `count` LWEs: lwe_a[count][n], lwe_b[count]
 * (e.g. one gate of sgfhe_bootstrap_batch's output) -> bits[count]. */
int32_t sgfhe_host_decrypt_lwe(const sgfhe_params *p, const uint64_t *sk, const uint64_t *lwe_a,
                               const uint64_t *lwe_b, size_t count, uint8_t *bits);
/* decrypt(key, ::Union{Ciphertext, PackedCiphertext}) (src/fhe.jl:471-494), N = n or m -> bits[n]. */
int32_t sgfhe_host_decrypt_rlwe(const sgfhe_params *p, const uint64_t *sk, const uint64_t *a,
                                const uint64_t *b, size_t N, uint8_t *bits);

/*
 * The public-key side: PublicKey, _encrypt_public and the
 * space-optimal public ciphertext, on the host.  q is the public-key modulus of Params(n)
 * (find_modulus(2 n, r n), src/fhe.jl:57; q < 2^31), Dq = q / 4 (src/fhe.jl:88).  Polynomials over
 * Z_q are uint64 in [0, q).  Pure functions: the caller passes the reference's draws.
 */
/* PublicKey(rng, sk) (src/fhe.jl:146-168) given its draws k0[n] in [0, q) and the centred noise
 * e[n] in [-e_max, e_max] (e_max the largest integer below Dq / (41 n), :159-160): k1 = k0 s + e.
 * The reference writes `polynomial - e_max` (:161); the noise is centred on every coefficient
 * here (DarkIntegers' Polynomial - scalar rule is not checkable in this build; decryption holds
 * either way). */
int32_t sgfhe_host_public_key(const sgfhe_params *p, uint64_t q, const uint64_t *sk, const uint64_t *k0,
                              const int64_t *e, uint64_t *k1);
/* _encrypt_public(key, rng, message) (src/fhe.jl:386-409) given its draws u[n] in {-1, 0, 1},
 * w1[n] in [-Dq / (41 n), Dq / (41 n)] and w2[n] in [-Dq / 82, Dq / 82]: -> RLWE (a, b) over Z_r,
 * b a multiple of 2^(t - 5). */
int32_t sgfhe_host_encrypt_public(const sgfhe_params *p, uint64_t q, const uint64_t *k0, const uint64_t *k1,
                                  const int8_t *u, const int64_t *w1, const int64_t *w2,
                                  const uint8_t *message, uint64_t *a, uint64_t *b);
/* The bit matrices of encrypt_optimal(key::PublicKey, ...) (src/fhe.jl:420-436):
 * (a[n], b[n]) -> a_bits[t + 1][n], b_bits[6][n]. */
int32_t sgfhe_host_pack_public(const sgfhe_params *p, const uint64_t *a, const uint64_t *b,
                               uint8_t *a_bits, uint8_t *b_bits);
/* normalize_ciphertext(::PublicEncryptedCiphertext) (src/fhe.jl:444-449). */
int32_t sgfhe_host_normalize_public(const sgfhe_params *p, const uint8_t *a_bits, const uint8_t *b_bits,
                                    uint64_t *a, uint64_t *b);

/*
 * Gate circuits, evaluated on the device level by level over many independent instances.
 *
 * Model.  A circuit has `n_inputs` input wires and `n_gates` nodes; every node is one
 * bootstrap(bkey, rng, x, y) (src/fhe.jl:608-621), which yields AND, OR and XOR together.  Wire ids:
 * inputs 0 .. n_inputs - 1; node g produces n_inputs + 3 g + 0 (AND), + 1 (OR), + 2 (XOR).  A wire
 * REFERENCE is a uint32: the wire id, plus SGFHE_CIRCUIT_NOT (bit 31) for its negation; the id
 * SGFHE_CIRCUIT_FALSE is the constant FALSE (the trivial LWE (0, 0)), so FALSE | NOT is TRUE.
 * NOT w = enc_trivial(true) - w with the reference's LWE subtraction (src/fhe.jl:221-223, enc_trivial
 * :669-670): a -> -a mod r, b -> (Dr - b) mod r, Dr = r / 4 -- so NAND, NOR, XNOR, ANDNOT ... cost their
 * one bootstrap and nothing more.  A node's two inputs (gates[g][0], gates[g][1]) name an input wire, the
 * constant or a wire of an EARLIER node: array order is a topological order.  `outputs` lists wire
 * references; they may name inputs, the constant and negated wires.
 *
 * Plan (sgfhe_circuit_create, host only; one plan serves every ctx and clone).  Validation: ids in range,
 * the rule above, n_outputs >= 1, n_inputs, n_gates, n_outputs and n_inputs + 3 n_gates below 2^31 - 1;
 * anything else is SGFHE_ERR_INVALID_ARG, an allocation failure SGFHE_ERR_OOM (*out is then NULL).  Nodes
 * no output depends on are dropped; the others get level = 1 + the largest level of their input nodes
 * (inputs and the constant are level 0).  Every wire something reads gets a slot of a device wire table
 * ([slot][instance][n + 1] words); a slot is reused only after the last level that reads its wire, output
 * wires stay to the end.
 * info[0] levels, [1] nodes evaluated per instance, [2] widest level (nodes), [3] wire slots.
 *
 * Run (sgfhe_circuit_run): in [n_inputs][instances][n + 1], out [n_outputs][instances][n + 1], uint64 in
 * [0, r), a then b (the layout of one gate of sgfhe_bootstrap_batch's output).  Host pointers; synchronous.
 * `in` may be NULL when n_inputs is 0.  instances = 0 does nothing.  The ctx is locked for the whole run and
 * the coalescer is not used.  Row and call numbering -- the contract of the randomised flatten: within a
 * level the nodes are taken in ascending index, row = rank_in_level * instances + instance; a level's rows
 * go to the device in calls of at most SGFHE_CIRCUIT_CALL_ROWS rows, in order, levels in order; every call
 * takes the next call number of the ctx's draw stream (as an sgfhe_bootstrap_batch call does) and a row
 * draws as the bootstrap at its index within its call.  Each call is a gather kernel (the call's inputs from
 * the wire table, NOT and the constant applied), the k-loop of sgfhe_bootstrap_batch_device, and a scatter
 * kernel (the outputs something reads into their slots); no host synchronisation between levels.  The wire
 * table and the per-call staging are kept on the ctx, grown on demand, and freed by
 * sgfhe_release_host_staging and sgfhe_ctx_destroy.  SGFHE_ERR_NO_KEY before a key is uploaded (nothing is
 * written to `out`).
 *
 * Lanes (sgfhe_circuit_create_lanes).  The model above is strictly SIMD: instance t of a node reads instance t of
 * its inputs.  A plan with a LANE GROUP SIZE `group` = G >= 1 partitions the instances into consecutive groups of G
 * -- instance t is lane t mod G of group t div G -- and gives every gate input (gate_shift [n_gates][2]) and every
 * output reference (out_shift [n_outputs]) a signed LANE SHIFT d, |d| < G.  The value of the reference
 * (wire w, NOT, d) at instance t is w at instance t + d where 0 <= (t mod G) + d < G, and the constant FALSE (the
 * trivial LWE (0, 0)) elsewhere; NOT is applied afterwards as above, so a negated reference fills with TRUE.
 * Shifts never cross a group: with G a power of two dividing n, a ciphertext of sgfhe_circuit_run_ct holds n / G
 * independent G-bit words.  A shift costs no bootstrap -- the gather and collect kernels read another row of the
 * same slot -- and changes nothing else: node numbering, pruning, levels, slots, rows, calls and call numbers are
 * those of the same arrays without shifts (a shifted read names a wire of an earlier level, whose rows are all
 * written and whose slot is held until the reading level ends).  A NULL shift array is all 0; a shift on a
 * reference to the constant is accepted and has no effect.  Validation: everything sgfhe_circuit_create checks,
 * group >= 1 and every |d| < group (so group = 1 admits no shift but 0); anything else is SGFHE_ERR_INVALID_ARG
 * with *out NULL.  sgfhe_circuit_create is group = 1 with NULL shifts; sgfhe_circuit_group reports G.
 * Every run entry point takes such a plan.  Before anything is queued or written, SGFHE_ERR_INVALID_ARG when
 * `instances` is not a multiple of G and, in the ciphertext forms, when n is not (a group must not straddle two
 * ciphertexts).  The probe's plaintext evaluation applies the shifts; a wire's record is over its own rows.
 *
 * Three-input nodes (sgfhe_circuit_create3).  gates and gate_shift are [n_gates][3].  gates[g][2] ==
 * SGFHE_CIRCUIT_NONE makes node g the two-input node above (the shift beside it is ignored); a plan whose third
 * references are all NONE is the sgfhe_circuit_create_lanes plan of the same arrays: info, rows, calls, output bytes,
 * and the kernels it runs.  Any other third reference makes g a THREE-INPUT node; that reference is validated like the
 * other two, may name the constant, carry NOT and a lane shift.  NONE anywhere else -- gates[g][0], gates[g][1],
 * outputs, or with the NOT bit -- is SGFHE_ERR_INVALID_ARG (it is no wire id: ids are below 2^31 - 2).
 * With X, Y, Z the three referenced LWEs at one instance (lane shift, constant fill and NOT applied as above), the
 * node is ONE row of its level call -- pruning, levels, slots, row and call numbering and the draws are those of a
 * two-input node -- whose bootstrap inputs are (a1, b1) = X + Y + Z mod r and (a2, b2) = 0; the bootstrap adds its two
 * inputs first, so this is bootstrap(X + Y mod r, Z) byte for byte.  The bootstrap rotates the
 * test polynomial by the phase of the sum of its inputs, here near s Dr, s = x + y + z in {0, 1, 2, 3}: four distinct
 * values mod r = 4 Dr, each Dr/2 from the nearest sign change, as for two inputs.  Wires of the node:
 *   n_inputs + 3 g + 0  MAJ         the AND row: 0, 0, 1, 1 for s = 0 .. 3
 *   n_inputs + 3 g + 1  ONE_OR_TWO  the OR row:  0, 1, 1, 0 (not all equal)
 *   n_inputs + 3 g + 2  XOR3        (X + Y + Z - 2 MAJ) mod r, word by word, b included, MAJ being the reduced row
 *                                   (the words k_final gives): 0, 1, 0, 1.  NOT the bootstrap's XOR row, which means
 *                                   nothing at s = 3.
 * So a full adder (sum = XOR3, carry = MAJ) is one bootstrap.  With the third input FALSE the node is AND, OR, XOR;
 * with TRUE, MAJ is OR and ONE_OR_TWO is NAND.
 * Every run entry point takes such a plan.  Under SGFHE_CIRCUIT_PACK_DIRECT an output naming a MAJ or ONE_OR_TWO wire
 * with shift 0 is DIRECT (NOT over Z_Q as for any gate row); an output naming an XOR3 wire is REFRESHED (LIFTED under
 * SGFHE_CIRCUIT_PACK_LIFT) -- it is no gate row over Z_Q -- and out_lwe keeps the bytes of the flags = 0 run.  The probe's plaintext evaluation knows the
 * three wires; XOR3 wires get Z_r records like any other.
 * Noise -- a MEASURED rule, not a theorem of the scheme.  XOR3 is not bootstrapped: its error is
 * e_X + e_Y + e_Z - 2 e_MAJ, so it carries the errors of the node's inputs on.  A node (two- or three-input) is
 * correct while the error of the SUM of its inputs stays below Dr/2.  A fresh encryption that was SPLIT
 * (sgfhe_host_encrypt_private, then split_ciphertext) has an LWE error of up to Dr/4 - 1, not the Dr/8 of its draws:
 * encrypt_private rounds b -- with zero draws the error is already Dr/8 - 1 -- and the measured worst over a few
 * thousand bits is 63 of Dr = 256 at Params(64), 123 of 512 at Params(128), 1006 of 4096 at Params(1024): 0.24 Dr.
 * Three of those can reach 0.75 Dr, past Dr/2: a node fed by three such encryptions is not covered by a bound, only
 * by the measured distribution;
 * the reference's bound for two gate outputs does not cover three either, and at Params(1024) the evidence is
 * the probe (sgfhe_circuit_run_probe) -- the one recorded figure there is a worst packed phase error of 22 against
 * Dr/2 = 2048 (RESULTS.md).  An XOR3 wire that feeds a node counts with the sum of its own three inputs' errors:
 * feed it together with bootstrapped wires or constants, as the carry chain of a ripple adder does (sum bits are
 * outputs, only MAJ is carried on).
 *
 * Weighted-sum nodes (sgfhe_circuit_create_w).  The rotation depends on the SUM of the bootstrap's inputs only, and
 * its two sign reads on that sum's multiple of Dr mod 4; three terms of weight 1 are one case.  The nodes come as CSR
 * arrays: node g's terms are term_ref / term_shift / term_weight [node_start[g] .. node_start[g + 1]), node_start[0]
 * = 0.  node_kind[g] = 0 is the CLASSIC two-input node above (exactly two terms of weight 1, its XOR wire the
 * bootstrap's own row); node_kind[g] = 1 is a SUM NODE of 1 to SGFHE_CIRCUIT_MAX_TERMS terms, every weight w_i in
 * {-2, -1, 1, 2}.  A term's reference is validated like any node input: an input wire, the constant or a wire of an
 * earlier node, with NOT and a lane shift, both applied before the weight.  With X_i the referenced LWEs at one
 * instance, the node is ONE row of its level call -- pruning, levels, slots, row and call numbering and the draws
 * are those of any node -- whose bootstrap inputs are (a1, b1) = U = sum of w_i X_i mod r, word by word, b included,
 * and (a2, b2) = 0 (the bootstrap adds its two inputs first: (U, 0) gives the words (X + Y, Z) gives when U =
 * X + Y + Z).  TRUE (FALSE | NOT) with weight c adds the constant c Dr.  With s = sum of w_i x_i mod 4 over the
 * plaintext bits, the wires of the node are
 *   n_inputs + 3 g + 0  HI   the AND row: s in {2, 3}
 *   n_inputs + 3 g + 1  MID  the OR row:  s in {1, 2}
 *   n_inputs + 3 g + 2  LOW  (U - 2 HI) mod r, word by word, b included, HI being the reduced row (the words k_final
 *                            gives): s mod 2.  Linear, not bootstrapped -- what XOR3 is for a three-input node.
 * So weights (1, 1, 1) are the three-input node (the same bytes on all three wires; two unit terms are (x, y,
 * FALSE)); all weights 2 give HI = the XOR of all terms, ONE bootstrap for a parity of up to 64 wires -- a doubled
 * wire encodes its bit as 0 or 2 Dr = r / 2, and sums of those are XORs; one term of weight 1 gives MID = a refresh
 * of that wire; 2x + y + z gives HI = s >= 2 and MID = s in {1, 2} for s = 0 .. 3 (s = 4 wraps to 0).
 * Validation: everything sgfhe_circuit_create3 checks, and node_start non-decreasing from 0, node_kind 0 or 1, the
 * term counts and weights above; SGFHE_CIRCUIT_NONE never appears.  Anything else is SGFHE_ERR_INVALID_ARG with
 * *out NULL, and nothing is allocated.  A NULL term_shift is all 0.
 * Every run entry point takes such a plan, and every plan, whichever entry made it, is gathered by the one
 * k_circ_gather (one pass over the node's terms per word).  Under SGFHE_CIRCUIT_PACK_DIRECT an output naming HI or MID with shift 0 is DIRECT; one naming LOW
 * is REFRESHED (LIFTED under SGFHE_CIRCUIT_PACK_LIFT), as XOR3 is.  The probe's plaintext evaluation knows the three
 * wires; the record of a LOW wire is, up to 2 e_HI, the error of the node's input sum.
 * Noise -- a MEASURED rule, as for three inputs.  A node is correct while |sum of w_i e_i| < Dr/2, and LOW carries
 * that error on.  A weight of 2 doubles its wire's error: a split sgfhe_host_encrypt_private bit has an error of up
 * to Dr/4 - 1, which doubled is already at the limit, so weight-2 terms are for gate rows, refreshed wires (MID of
 * a one-term node) and packed outputs, never for fresh encryptions.  Measured on the C oracle at Params(64), 64
 * instances, inputs refreshed first (max |e| = 4): for k = 2 .. 8 the AND row of 2 (X_1 + ... + X_k) decrypts to the
 * parity in every instance, the error of the doubled sum is at most 28 against Dr/2 = 128, the output error at most
 * 6; a node 2x + y + z gives s >= 2 on the AND row and s in {1, 2} on the OR row for all four values of s.
 * At Params(1024) (Dr/2 = 2048), with the probe over 256 instances: refreshed wires have max |e| = 26, and the LOW wire
 * of a parity node of 8, 16 and 32 refreshed wires max |e| = 146, 202 and 256 -- an eighth of the margin at 32 terms,
 * the errors adding like independent ones; CRC-16 of 32-bit messages (examples/encrypted_crc.py --direct, one block)
 * has a worst packed phase error of 33 (RESULTS.md, profiles/r13_circuit_wsum.txt).
 *
 * LUT nodes (sgfhe_circuit_create_lut): any function of three wires in one bootstrap, the node form of
 * sgfhe_bootstrap_lut_batch (its contract and noise rule are with its declaration below).  The arrays are those of
 * sgfhe_circuit_create_w plus node_table[n_gates] (read for LUT nodes only, must be below 256); node_kind[g] = 2 marks
 * a LUT NODE.  sgfhe_circuit_create_w itself keeps rejecting kinds other than 0 and 1.
 * A LUT node has exactly three terms, at positions 0, 1 and 2, all of weight 1.  Every wire has a SCALE: scale 0 is
 * the codeword Dr -- input wires, every wire of a kind-0 or kind-1 node, and wire +0 of a LUT node; wires +1 and +2 of
 * a LUT node have scales 1 and 2, codewords Dr/2 and Dr/4.  Position i of a LUT node must reference the constant or a
 * wire of scale 2 - i; every other reference in the plan -- the terms of the other node kinds and all outputs -- must
 * have scale 0.  Anything else is SGFHE_ERR_INVALID_ARG with *out NULL.  NOT at position i is a -> -a,
 * b -> (Dr >> (2 - i)) - b mod r; lane shifts work as everywhere, filling with FALSE and applying NOT afterwards.
 * The node is one row of its level call -- pruning, levels, slots, row and call numbering and the draws are those of
 * any node -- with bootstrap inputs (a1, b1) = U = X0 + X1 + X2 mod r and (a2, b2) = 0; its three wires are the three
 * rows of sgfhe_bootstrap_lut_batch for node_table[g], with s = x0 + 2 x1 + 4 x2.  A level call may mix all three
 * kinds: LUT rows start at amplitude A0 and leave through the LUT extraction, the other rows take exactly the path
 * they take without LUT nodes.  In an un-reduced call (SGFHE_CIRCUIT_PACK_DIRECT) the LUT rows are the scaled
 * residues, and their ModRed gives the words of the reduced call.  An output naming wire +0 of a LUT node is
 * REFRESHED, or LIFTED under SGFHE_CIRCUIT_PACK_LIFT, as a LOW wire is.  `fan` -- the LUT node (FALSE, FALSE, x) of
 * table 0xF0 -- brings a scale-0 wire to all three scales in one bootstrap.  Every run entry point takes such a plan.
 * The probe's plaintext evaluation knows LUT nodes, and the record of a wire of scale k is taken against its own
 * codeword C = Dr >> k: e is centred against bit C, stats[1] counts |e| >= C/2 and stats[5] counts |e| >= C/4.
 *
 * LUT families (sgfhe_circuit_create_lut_multi): several truth tables on ONE bootstrap, the node form of
 * sgfhe_bootstrap_lut_multi_batch (declared below).  The arrays are those of sgfhe_circuit_create_lut, and
 * node_kind[g] = 3 marks a SIBLING: a further table, node_table[g] (below 256), on the bootstrap of its LEADER, the
 * nearest earlier kind-2 node.  sgfhe_circuit_create_lut and sgfhe_circuit_create_w keep rejecting kind 3.  A sibling
 * has no terms (node_start[g + 1] == node_start[g]), node g - 1 must be of kind 2 or 3, and a leader with its siblings
 * has at most SGFHE_LUT_MAX_TABLES members; anything else is SGFHE_ERR_INVALID_ARG with *out NULL.  Wire numbering stays
 * n_inputs + 3 g + w: a sibling's three wires have scales 0, 1, 2, and the scale rule and the output rule treat it as a
 * LUT node (an output naming its wire +0 is refreshed, or lifted).
 * A sibling is live when an output reaches one of its wires, and a leader is live when an output reaches it or any of
 * its siblings is live; a dead sibling is not extracted.  A sibling has its leader's level and TAKES NO ROW: within a
 * level the live nodes that are no siblings take the ranks in ascending index, row = rank * instances + instance, so
 * rows, calls, call numbers and draws are those of the same arrays with every kind-3 node deleted.  At every instance
 * the three wires of a live sibling are the bytes the leader's three wires would have with node_table[leader] replaced
 * by the sibling's table -- the terms, lane shifts and NOTs are the leader's -- in an un-reduced level call
 * (SGFHE_CIRCUIT_PACK_DIRECT) too, where they reach the wire table as the ModRed words of the reduced call.
 * sgfhe_circuit_info: info[1] and info[2] count BOOTSTRAPS -- the live nodes that take a row --, info[3] counts slots,
 * those of sibling wires included; a plan without siblings reports what it always did.  Every run entry point takes
 * such a plan.  The probe's plaintext evaluation knows siblings; `stats` stays indexed by wire id.  A live sibling's
 * wire is measured, against its own codeword, WHEN IT HAS A SLOT -- when a node or an output reads it -- from the
 * slot's rows of that call.  A sibling wire that nothing reads is never written anywhere and gets an all-zero record,
 * as the wires of dead siblings do: the one place where "every wire of every live node" does not extend.
 *
 * Data planes (sgfhe_circuit_create_data): truth tables that differ from instance to instance.  The arrays are those of
 * sgfhe_circuit_create_lut_multi with two more kinds: node_kind[g] = 4 is a DATA LUT node -- a kind-2 node in every
 * respect (three unit terms at positions 0, 1, 2, the scale rule, wires of scales 0, 1, 2, the output rule) whose
 * node_table[g] is a PLANE index below n_planes, not a table -- and node_kind[g] = 5 a DATA sibling, a kind-3 node whose
 * node_table[g] is a plane index.  A sibling of kind 3 or 5 belongs to the nearest earlier node of kind 2 or 4, node
 * g - 1 of a sibling is of kind 2, 3, 4 or 5, and a family may mix constant and data members, SGFHE_LUT_MAX_TABLES at
 * most.  n_planes is at most SGFHE_CIRCUIT_MAX_PLANES; a plane may be used by several nodes or by none.  A plane index
 * that is not below n_planes, or n_planes above the cap, is SGFHE_ERR_INVALID_ARG with *out NULL and nothing allocated.
 * Every other creator keeps rejecting kinds 4 and 5.  Pruning, liveness, levels, slots, rows, calls, call numbers and
 * sgfhe_circuit_info are those of the same arrays with kind 4 read as 2 and kind 5 as 3; with n_planes = 0 and no node
 * of kind 4 or 5 the plan is the sgfhe_circuit_create_lut_multi plan.  sgfhe_circuit_planes gives n_planes (0 for a plan
 * of any other creator).
 * The run entries sgfhe_circuit_run_data, _run_ct_data and _run_probe_data take `data`, [n_planes][instances] uint8
 * (instances = blocks * n in the ciphertext form, numbered as sgfhe_circuit_run_ct numbers them): at instance t a data
 * node or data sibling of plane p has the truth table data[p][t], bit s its value at s = x0 + 2 x1 + 4 x2 -- at the
 * node's OWN instance, whatever lane shifts its terms carry.  Any byte is a table; `data` is not validated beyond NULL.
 * The planes go up once per run into a buffer kept on the ctx like the wire table (grown on demand, freed by
 * sgfhe_release_host_staging and sgfhe_ctx_destroy); no host synchronisation is added.  The contract: the run is, byte
 * for byte, the run of the constant-table plan with each row evaluated under its own table -- calls, rows, call numbers
 * and every row's draws unchanged, in both flatten modes, reduced and un-reduced, under every flag set of
 * sgfhe_circuit_run_ct_ex.  Row R of a level call of a data leader is the row of sgfhe_bootstrap_lut_batch with
 * table[R] = data[p][R % instances]; a live data sibling's three wires are what the leader's would be under the
 * sibling's byte at that instance.  An output naming wire +0 of a data node or data sibling is refreshed, or lifted
 * under SGFHE_CIRCUIT_PACK_LIFT, as for kinds 2 and 3.  The probe variant evaluates the plaintext circuit with `data`
 * and measures data wires by the rules of LUT and sibling wires (a sibling wire without a slot: an all-zero record).
 * The table does not enter the k-loop, so the noise rule is that of LUT nodes and no new rule is claimed.
 * Errors, before anything is queued or written: SGFHE_ERR_INVALID_ARG for data == NULL when the plan has planes and
 * instances > 0, and for everything the entry without data rejects; SGFHE_ERR_NO_KEY and SGFHE_ERR_OOM as there.  A
 * plan without planes may go through the _data entries with data NULL: that run is the old entry.  sgfhe_circuit_run,
 * _run_ct, _run_ct_ex and _run_probe return SGFHE_ERR_INVALID_ARG for a plan with planes, write nothing and consume no
 * call number.
 *
 * Registers and stepped runs (sgfhe_circuit_create_seq, sgfhe_circuit_run_steps, sgfhe_circuit_run_steps_ct): a
 * SEQUENTIAL circuit is a plan whose first n_regs input wires are REGISTERS, and a stepped run evaluates it `steps`
 * times over the same instances in one queued run; after each step every register takes the value of its next-state
 * reference.  The other n_inputs - n_regs inputs (the STREAM inputs), the data planes and the outputs are per step.
 * Nothing is added to the k-loop: a step's level calls are exactly those of sgfhe_circuit_run_data.
 * The creator takes the arrays of sgfhe_circuit_create_data and
 *   n_regs      : at most n_inputs; register i is input wire i;
 *   next_ref    : [n_regs] wire references, validated like outputs: an input, a register (itself included), the
 *                 constant or any node wire, with or without SGFHE_CIRCUIT_NOT;
 *   next_shift  : [n_regs] lane shifts, NULL = all 0, every |d| below `group`;
 *   reg_scale   : [n_regs], each 0, 1 or 2, NULL = all 0.  For the scale rule register i is a wire of scale
 *                 reg_scale[i] (so a LUT node may read a scale-2 register at position 0 without a fan), and its
 *                 next_ref names the constant or a wire of that same scale.  NOT on a next-state reference of scale k
 *                 is a -> -a, b -> (Dr >> k) - b.  Stream inputs are scale 0.
 * Next-state references count as readers exactly as outputs do -- liveness, levels, slot lifetime (held to the end of
 * the step) -- so a node reached only through next_ref is live, and levels, order, rows and calls are those of the STEP
 * PLAN: the sgfhe_circuit_create_data plan of the same node arrays with outputs = outputs ++ next_ref.  n_outputs >= 1
 * stays.  With n_regs = 0 the plan is the sgfhe_circuit_create_data plan of the same arrays (info, tables, rows, calls).
 * sgfhe_circuit_registers gives n_regs (0 for a plan of any other creator).  Every other run entry (sgfhe_circuit_run,
 * _run_data, _run_ct, _run_ct_ex, _run_ct_data, _run_probe, _run_probe_data) returns SGFHE_ERR_INVALID_ARG for a plan
 * with registers before anything is queued, writes nothing and consumes no call number.
 * sgfhe_circuit_run_steps, the LWE form (host pointers, synchronous, the ctx locked for the whole run):
 *   state_in  : [n_regs][instances][n + 1], the registers before step 0; NULL = every register FALSE (the trivial LWE);
 *   in        : [steps][n_inputs - n_regs][instances][n + 1], the stream inputs of every step;
 *   data      : [steps][n_planes][instances], the planes of every step (NULL for a plan without planes);
 *   emit      : [steps] uint8, nonzero = the step's outputs are wanted; NULL = every step;
 *   out       : [emitted steps][n_outputs][instances][n + 1], the emitted steps in order; rows past them are not written;
 *   state_out : [n_regs][instances][n + 1], the registers after the last step.  At least one of out, state_out.
 * The contract: step s is, byte for byte, sgfhe_circuit_run_data of the step plan on (the registers at the start of step
 * s) ++ in[s] with the planes data[s]; its first n_outputs outputs are the step's outputs and the others the registers
 * at the start of step s + 1.  The level calls of successive steps take consecutive call numbers of the ctx's draw
 * stream.  A step's outputs are taken BEFORE the feedback: an output that names a register shows the value the step
 * started with.  steps = 0 or instances = 0 does nothing and consumes nothing.  A run of a + b steps equals a run of a
 * steps followed by a run of b steps started from the first run's state_out, on the same stream.
 * Host and device memory do not grow with `steps`: the wire table is slots * instances * (n + 1) words as for one run,
 * the registers live between steps in a ctx buffer [n_regs][instances][n + 1] (grown on demand, freed with the other
 * circuit buffers), in[s] and data[s] go up at the start of step s and an emitted step's outputs come down in stream
 * order; the host waits once, at the end.  In a step with emit[s] = 0 nothing is collected or downloaded, but ITS NODES
 * STILL RUN, output-only nodes included: the plan is static, and the call numbers do not depend on `emit`.
 * sgfhe_circuit_run_steps_ct, the ciphertext form (numbering, N and flags as sgfhe_circuit_run_ct_ex):
 *   state_a, state_b : [n_regs][blocks][N], the registers start as the split of these; both NULL = FALSE;
 *   in_a, in_b       : [steps][n_inputs - n_regs][blocks][N], split into the input slots at the start of each step;
 *   out_w, out_v     : [emitted steps][n_outputs][blocks][m]: an emitted step runs the pack stage of
 *                      sgfhe_circuit_run_ct_ex on that step's wire table under `flags`;
 *   out_lwe          : [emitted steps][n_outputs][blocks * n][n + 1], the bytes of the LWE-form stepped run;
 *   state_lwe        : [n_regs][blocks * n][n + 1], the registers after the last step (LWEs: feed them to
 *                      sgfhe_circuit_run_steps, or pack them).  One of (out_w, out_v), out_lwe, state_lwe is needed.
 * Call numbers per step: the step's level calls, then the step's pack calls if it is emitted.  A plan with a register
 * of scale 1 or 2 is refused (SGFHE_ERR_INVALID_ARG, nothing written): a split ciphertext is scale 0 and an LWE cannot
 * be halved.  There is no probe variant of a stepped run.
 * Errors of both, before anything is queued or written: SGFHE_ERR_INVALID_ARG for a NULL plan, NULL stream inputs when
 * the plan has any, NULL data when it has planes (and steps, instances > 0), no output pointer, instances not a
 * multiple of the group, and the size limits of the one-shot entries; SGFHE_ERR_NO_KEY, SGFHE_ERR_OOM as there.
 * Noise rule for registers, MEASURED, NOT PROVED (tests/test_gpu_circuit_steps.py: a serial adder over 64 steps): a
 * register should be fed by a bootstrapped wire -- a gate row, HI / MID of a sum node, a LUT wire -- whose error does
 * not depend on the step.  A LOW / XOR3 wire or a stream input fed back carries its error on and adds to it every step.
 *
 * Lane routes (sgfhe_circuit_create_routed): any public lane map inside a group, at no bootstrap.  The creator takes the
 * arrays of sgfhe_circuit_create_seq and
 *   n_routes   : route tables, at most SGFHE_CIRCUIT_MAX_ROUTES; a table may be used by several references or by none;
 *   routes     : [n_routes][group] int32, each entry a source lane in [0, group) or SGFHE_CIRCUIT_ROUTE_FALSE (-1);
 *   term_route : beside term_shift, NULL = all 0; out_route [n_outputs] and next_route [n_regs] likewise.
 * A route index 0 means none -- the shift applies as before -- and k >= 1 names table k - 1.  The reference (w, NOT,
 * route rho) at instance t, lane l = t mod group, is w at instance t - l + rho[l], and the constant FALSE where rho[l]
 * is SGFHE_CIRCUIT_ROUTE_FALSE; NOT is applied afterwards at the codeword of the position (Dr, Dr/2 or Dr/4 by the scale
 * rule), so a negated reference fills with TRUE exactly as a shift that leaves the group does.  A reference with a
 * route has shift 0; a route on a reference to the constant is dropped, as a shift is.  The table of a data LUT node
 * stays the byte at the node's OWN instance, whatever routes its terms carry.  Numbering, pruning, levels, slots, rows,
 * calls, call numbers and sgfhe_circuit_info do not see routes (a routed read names a wire of an earlier level,
 * whichever instance of it is read), and with n_routes = 0 the plan is the sgfhe_circuit_create_seq plan of the same
 * arrays.  SGFHE_ERR_INVALID_ARG with *out NULL and nothing allocated for: an entry outside [-1, group), a route index
 * above n_routes, a route beside a non-zero shift, n_routes > 0 with routes NULL, n_routes above the cap, and everything
 * sgfhe_circuit_create_seq rejects.  sgfhe_circuit_routes gives n_routes (0 for a plan of any other creator).
 * A routed plan runs through every run entry above that takes its plan otherwise (planes: the _data entries, registers:
 * the _steps entries).  In the ciphertext form an output with a route is REFRESHED, or LIFTED under
 * SGFHE_CIRCUIT_PACK_LIFT, as an output with a non-zero shift is -- even where its table is the identity.  The probe
 * applies the routes in its plaintext bit table; its launches are unchanged.  A route moves whole LWEs and adds no
 * error: no noise rule is added.
 *
 * Lane masks (sgfhe_circuit_create_masked): a node bootstraps only the lanes that are read.  The creator takes the
 * arrays of sgfhe_circuit_create_routed and
 *   n_masks   : mask tables, at most SGFHE_CIRCUIT_MAX_MASKS; a table may be used by several nodes or by none;
 *   masks     : [n_masks][group] uint8, each entry 0 or 1, every table with at least one lane set;
 *   node_mask : [n_gates], NULL = all 0.
 * A mask index 0 means every lane -- the node as before -- and k >= 1 names table k - 1.  A masked node takes a row
 * only at the instances t whose lane t mod group is set.  On the lanes that are off EVERY wire of the node is the
 * constant FALSE -- AND / OR / XOR, HI / MID / LOW, the three scales of a LUT node all read as the trivial LWE (0, 0),
 * all n + 1 words zero -- wherever it is read: by a term, an output, a next state, the lift, the collected LWEs.  NOT
 * on such a reference gives TRUE at the codeword of the reading position, exactly as for a shift that leaves its
 * group.  Numbering, pruning, liveness, levels, slots and sgfhe_circuit_info do not see masks, and with n_masks = 0 the
 * plan is the sgfhe_circuit_create_routed plan of the same arrays.
 * Rows of a masked plan (n_masks > 0; a plan without masks keeps row = rank * instances + instance and every byte, call
 * and call number it has): every level is a list of (node, lane) PAIRS, nodes ascending in the level's order, lanes
 * ascending, an unmasked node contributing all `group` lanes; with per = instances / group, row R of the level is pair
 * R / per at group R mod per, that is instance (R mod per) * group + lane.  Levels are cut into calls of
 * SGFHE_CIRCUIT_CALL_ROWS rows from row 0 as before, and a row draws at its index within its call.
 * SGFHE_ERR_INVALID_ARG with *out NULL and nothing allocated for: an entry other than 0 or 1, a table with no lane set,
 * a mask index above n_masks, n_masks > 0 with masks NULL, n_masks above the cap, a mask on a sibling (kinds 3 and 5),
 * and everything sgfhe_circuit_create_routed rejects; and, with *out NULL and nothing kept, for a masked LUT node that
 * leads a LIVE sibling (the sibling's wires are written inside the bootstrap call, which knows no off lanes).
 * sgfhe_circuit_masks gives n_masks and rows_per_group, the level-call rows one group of `group` instances costs: the
 * sum over the live row-taking nodes of the lanes set (0 and bootstraps * group for a plan of any other creator).
 * A masked plan runs through every run entry that takes its planes, registers and routes, the device-resident forms
 * and sgfhe_debug_circuit_script[_calls] included.  The probe entries refuse it with SGFHE_ERR_UNSUPPORTED and a
 * message, before anything is queued or a call number is taken.  In the ciphertext form an output that names a wire of
 * a masked node is REFRESHED, or LIFTED under SGFHE_CIRCUIT_PACK_LIFT, never direct; outputs of unmasked nodes of the
 * same plan stay direct.  An off lane is the exact trivial LWE and carries no error: no noise rule is added.
 */
typedef struct sgfhe_circuit sgfhe_circuit;
#define SGFHE_CIRCUIT_FALSE 0x7FFFFFFFu
#define SGFHE_CIRCUIT_NONE 0x7FFFFFFEu   /* gates[g][2] of sgfhe_circuit_create3: node g has two inputs */
#define SGFHE_CIRCUIT_NOT 0x80000000u
#define SGFHE_CIRCUIT_CALL_ROWS 8192u
int32_t sgfhe_circuit_create(uint32_t n_inputs, const uint32_t *gates /* [n_gates][2] */, size_t n_gates,
                             const uint32_t *outputs, size_t n_outputs, sgfhe_circuit **out);
int32_t sgfhe_circuit_create_lanes(uint32_t n_inputs, const uint32_t *gates /* [n_gates][2] */,
                                   const int32_t *gate_shift /* [n_gates][2], NULL = all 0 */, size_t n_gates,
                                   const uint32_t *outputs, const int32_t *out_shift /* [n_outputs], NULL = all 0 */,
                                   size_t n_outputs, uint32_t group, sgfhe_circuit **out);
int32_t sgfhe_circuit_create3(uint32_t n_inputs, const uint32_t *gates /* [n_gates][3] */,
                              const int32_t *gate_shift /* [n_gates][3], NULL = all 0 */, size_t n_gates,
                              const uint32_t *outputs, const int32_t *out_shift /* [n_outputs], NULL = all 0 */,
                              size_t n_outputs, uint32_t group, sgfhe_circuit **out);
#define SGFHE_CIRCUIT_MAX_TERMS 64u
int32_t sgfhe_circuit_create_w(uint32_t n_inputs,
                               const uint32_t *node_kind /* [n_gates]: 0 = classic two-input node, 1 = sum node */,
                               const uint32_t *node_start /* [n_gates + 1], CSR into the term arrays, [0] = 0 */,
                               const uint32_t *term_ref, const int32_t *term_shift /* NULL = all 0 */,
                               const int32_t *term_weight, size_t n_gates, const uint32_t *outputs,
                               const int32_t *out_shift /* [n_outputs], NULL = all 0 */, size_t n_outputs,
                               uint32_t group, sgfhe_circuit **out);
int32_t sgfhe_circuit_create_lut(uint32_t n_inputs,
                                 const uint32_t *node_kind /* [n_gates]: 0 classic, 1 sum node, 2 = LUT node */,
                                 const uint32_t *node_start /* [n_gates + 1], CSR into the term arrays, [0] = 0 */,
                                 const uint32_t *term_ref, const int32_t *term_shift /* NULL = all 0 */,
                                 const int32_t *term_weight,
                                 const uint32_t *node_table /* [n_gates]: the truth table of a LUT node, below 256 */,
                                 size_t n_gates, const uint32_t *outputs,
                                 const int32_t *out_shift /* [n_outputs], NULL = all 0 */, size_t n_outputs,
                                 uint32_t group, sgfhe_circuit **out);
int32_t sgfhe_circuit_create_lut_multi(uint32_t n_inputs,
                                       const uint32_t *node_kind /* [n_gates]: 0, 1, 2 as above, 3 = LUT sibling */,
                                       const uint32_t *node_start /* [n_gates + 1], CSR into the term arrays, [0] = 0 */,
                                       const uint32_t *term_ref, const int32_t *term_shift /* NULL = all 0 */,
                                       const int32_t *term_weight,
                                       const uint32_t *node_table /* [n_gates]: read for kinds 2 and 3, below 256 */,
                                       size_t n_gates, const uint32_t *outputs,
                                       const int32_t *out_shift /* [n_outputs], NULL = all 0 */, size_t n_outputs,
                                       uint32_t group, sgfhe_circuit **out);
#define SGFHE_CIRCUIT_MAX_PLANES 65536u
int32_t sgfhe_circuit_create_data(uint32_t n_inputs, uint32_t n_planes,
                                  const uint32_t *node_kind /* [n_gates]: 0 .. 3 as above, 4 = data LUT node, 5 = data sibling */,
                                  const uint32_t *node_start /* [n_gates + 1], CSR into the term arrays, [0] = 0 */,
                                  const uint32_t *term_ref, const int32_t *term_shift /* NULL = all 0 */,
                                  const int32_t *term_weight,
                                  const uint32_t *node_table /* [n_gates]: a table for kinds 2 and 3, a plane for 4 and 5 */,
                                  size_t n_gates, const uint32_t *outputs,
                                  const int32_t *out_shift /* [n_outputs], NULL = all 0 */, size_t n_outputs,
                                  uint32_t group, sgfhe_circuit **out);
int32_t sgfhe_circuit_planes(const sgfhe_circuit *c, uint32_t *n_planes);   /* 0 for every other creator */
int32_t sgfhe_circuit_create_seq(uint32_t n_inputs, uint32_t n_planes,
                                 const uint32_t *node_kind /* [n_gates]: 0 .. 5 as sgfhe_circuit_create_data */,
                                 const uint32_t *node_start /* [n_gates + 1], CSR into the term arrays, [0] = 0 */,
                                 const uint32_t *term_ref, const int32_t *term_shift /* NULL = all 0 */,
                                 const int32_t *term_weight,
                                 const uint32_t *node_table /* [n_gates]: a table for kinds 2 and 3, a plane for 4 and 5 */,
                                 size_t n_gates, const uint32_t *outputs,
                                 const int32_t *out_shift /* [n_outputs], NULL = all 0 */, size_t n_outputs,
                                 uint32_t group, uint32_t n_regs, const uint32_t *next_ref /* [n_regs] */,
                                 const int32_t *next_shift /* [n_regs], NULL = all 0 */,
                                 const uint32_t *reg_scale /* [n_regs]: 0, 1, 2; NULL = all 0 */, sgfhe_circuit **out);
int32_t sgfhe_circuit_registers(const sgfhe_circuit *c, uint32_t *n_regs);   /* 0 for every other creator */
#define SGFHE_CIRCUIT_MAX_ROUTES 65536u
#define SGFHE_CIRCUIT_ROUTE_FALSE (-1)   /* entry of a route table: the constant FALSE at that lane */
int32_t sgfhe_circuit_create_routed(uint32_t n_inputs, uint32_t n_planes,
                                    const uint32_t *node_kind /* [n_gates]: 0 .. 5 as sgfhe_circuit_create_data */,
                                    const uint32_t *node_start /* [n_gates + 1], CSR into the term arrays, [0] = 0 */,
                                    const uint32_t *term_ref, const int32_t *term_shift /* NULL = all 0 */,
                                    const int32_t *term_weight,
                                    const uint32_t *node_table /* [n_gates]: a table for kinds 2 and 3, a plane for 4 and 5 */,
                                    size_t n_gates, const uint32_t *outputs,
                                    const int32_t *out_shift /* [n_outputs], NULL = all 0 */, size_t n_outputs,
                                    uint32_t group, uint32_t n_regs, const uint32_t *next_ref /* [n_regs] */,
                                    const int32_t *next_shift /* [n_regs], NULL = all 0 */,
                                    const uint32_t *reg_scale /* [n_regs]: 0, 1, 2; NULL = all 0 */,
                                    uint32_t n_routes, const int32_t *routes /* [n_routes][group] */,
                                    const uint32_t *term_route /* beside term_shift, NULL = all 0 */,
                                    const uint32_t *out_route /* [n_outputs], NULL = all 0 */,
                                    const uint32_t *next_route /* [n_regs], NULL = all 0 */, sgfhe_circuit **out);
int32_t sgfhe_circuit_routes(const sgfhe_circuit *c, uint32_t *n_routes);   /* 0 for every other creator */
#define SGFHE_CIRCUIT_MAX_MASKS 65536u
int32_t sgfhe_circuit_create_masked(uint32_t n_inputs, uint32_t n_planes,
                                    const uint32_t *node_kind /* [n_gates]: 0 .. 5 as sgfhe_circuit_create_data */,
                                    const uint32_t *node_start /* [n_gates + 1], CSR into the term arrays, [0] = 0 */,
                                    const uint32_t *term_ref, const int32_t *term_shift /* NULL = all 0 */,
                                    const int32_t *term_weight,
                                    const uint32_t *node_table /* [n_gates]: a table for kinds 2 and 3, a plane for 4 and 5 */,
                                    size_t n_gates, const uint32_t *outputs,
                                    const int32_t *out_shift /* [n_outputs], NULL = all 0 */, size_t n_outputs,
                                    uint32_t group, uint32_t n_regs, const uint32_t *next_ref /* [n_regs] */,
                                    const int32_t *next_shift /* [n_regs], NULL = all 0 */,
                                    const uint32_t *reg_scale /* [n_regs]: 0, 1, 2; NULL = all 0 */,
                                    uint32_t n_routes, const int32_t *routes /* [n_routes][group] */,
                                    const uint32_t *term_route /* beside term_shift, NULL = all 0 */,
                                    const uint32_t *out_route /* [n_outputs], NULL = all 0 */,
                                    const uint32_t *next_route /* [n_regs], NULL = all 0 */,
                                    uint32_t n_masks, const uint8_t *masks /* [n_masks][group], 0 or 1 */,
                                    const uint32_t *node_mask /* [n_gates], NULL = all 0 */, sgfhe_circuit **out);
/* n_masks: 0 for every other creator; rows_per_group: level-call rows per group of `group` instances */
int32_t sgfhe_circuit_masks(const sgfhe_circuit *c, uint32_t *n_masks, uint64_t *rows_per_group);
int32_t sgfhe_circuit_group(const sgfhe_circuit *c, uint32_t *group);   /* 1 for sgfhe_circuit_create plans */
int32_t sgfhe_circuit_info(const sgfhe_circuit *c, uint64_t info[4]);
int32_t sgfhe_circuit_destroy(sgfhe_circuit *c);
int32_t sgfhe_circuit_run(sgfhe_ctx *ctx, const sgfhe_circuit *c, size_t instances, const uint64_t *in,
                          uint64_t *out);
/*
 * The same run with RLWE ciphertexts at both ends -- the reference's user flow (docs/src/manual.md:119-121,190-192,
 * test/api.test.jl:86-108): split_ciphertext (src/fhe.jl:287-290) of every input and pack_encrypted_bits
 * (src/fhe.jl:660-696) of every output done on the device inside the one queued run.  A ciphertext of n bits is one
 * wire over n instances:
 *   in_a, in_b   : [n_inputs][blocks][N] uint64 in [0, r), rlwe.a / rlwe.b of one ciphertext per (input, block);
 *                  N = n (PackedCiphertext, what encrypt yields) or N = m (Ciphertext, what packing yields), one N
 *                  per call.  May be NULL when n_inputs is 0.
 *   instances    = blocks * n; instance block * n + i is bit i (0-based) of that block's ciphertext, the LWE
 *                  split_ciphertext(ct)[i + 1] (the bytes of sgfhe_host_split_ciphertext)
 *   out_w, out_v : [n_outputs][blocks][m] uint64 in [0, r): for every (output, block) the Ciphertext
 *                  pack_encrypted_bits makes of that output wire's n LWEs of the block.  Both or neither.
 *   out_lwe      : optional, [n_outputs][blocks * n][n + 1]: exactly what sgfhe_circuit_run returns.
 * At least one of the two output forms must be requested.  Host pointers; synchronous; the ctx is locked for the
 * whole run and the coalescer is not used.  blocks = 0 does nothing.  Before anything is queued or written:
 * SGFHE_ERR_INVALID_ARG for NULL or inconsistent pointers, N neither n nor m, or blocks * n beyond the limits of
 * sgfhe_circuit_run; SGFHE_ERR_NO_KEY; SGFHE_ERR_UNSUPPORTED for packed output where sgfhe_pack_encrypted_bits is
 * unsupported (the exactness bound of the RNS primes).
 * The run: the ciphertexts go up as they are (16 KB each at Params(1024), against 8.4 MB of LWEs); one split
 * kernel writes extract() of every bit of every input something reads into its slot of the wire table; the levels
 * run as in sgfhe_circuit_run; the pack stage takes the ciphertexts q = output * blocks + block in ascending
 * order, max(1, SGFHE_CIRCUIT_CALL_ROWS / n) at a time (8 at Params(1024)), each such call being one
 * sgfhe_pack_encrypted_bits(count = its ciphertexts) whose bootstrap inputs are gathered from the wire table
 * (NOT, constant and pass-through outputs included); (w, v) of all ciphertexts come down in one copy each.  No host
 * synchronisation before the final download.
 * Randomised flatten: the level calls take the next call numbers of the ctx's draw stream as in
 * sgfhe_circuit_run; the pack calls follow, one call number each, in ascending q; within a pack call ciphertext
 * `ct` and bit `j` draw as in sgfhe_pack_encrypted_bits (bootstrap ct * n + j of the call; the flatten of as_i with
 * y = 2^31 | i, z = ct).  out_lwe consumes nothing.  So the whole run equals, on one stream: sgfhe_circuit_run, then
 * sgfhe_pack_encrypted_bits in groups of that many ciphertexts.  A run without out_w consumes the level calls only.
 */
int32_t sgfhe_circuit_run_ct(sgfhe_ctx *ctx, const sgfhe_circuit *c, size_t blocks, const uint64_t *in_a,
                             const uint64_t *in_b, size_t N, uint64_t *out_w, uint64_t *out_v, uint64_t *out_lwe);
/*
 * The same with flags; flags = 0 is sgfhe_circuit_run_ct, unknown bits are SGFHE_ERR_INVALID_ARG.
 *   SGFHE_CIRCUIT_PACK_DIRECT  pack the outputs that name a gate wire straight from the gate's un-reduced LWEs
 *       over Z_Q (sgfhe_pack_lwe_modq), without the n refresh bootstraps per ciphertext.
 * Ciphertext q = output * blocks + block is DIRECT when its output reference names a gate wire with lane shift 0,
 * negated or not, and REFRESHED when it names an input wire or the constant, or carries a non-zero lane shift
 * (sgfhe_circuit_create_lanes: its rows are not the gate's own rows in order) or names the XOR3 wire of a three-input
 * node or the LOW wire of a sum node (sgfhe_circuit_create3, sgfhe_circuit_create_w: linear over Z_r, no gate row).  The levels run with the calls, rows and call
 * numbers of sgfhe_circuit_run_ct, so out_lwe has the bytes of the flags = 0 run in both flatten modes; a level
 * call that produces a wire some direct output names leaves its rows un-reduced, and its scatter kernel writes
 * their ModRed (the words the reduced call gives) into the wire table and the named gate's rows into a raw
 * output table [q][n][n + 1] of 16-byte residues.  NOT over Z_Q is enc_trivial(true) - w: a -> -a,
 * b -> 2 DQ_tilde - b, mod Q.  The raw table is kept on the ctx like the wire table (grown on demand, freed by
 * sgfhe_release_host_staging and sgfhe_ctx_destroy): n_outputs * blocks * n * (n + 1) * 16 bytes -- 16.8 MB
 * per ciphertext at Params(1024), 285 MB per block for the 17 outputs of a 16-bit adder.  An allocation failure
 * is SGFHE_ERR_OOM before any output is written.
 * Pack stage -- the contract of the randomised flatten.  The ciphertexts are taken in ascending q, in groups of
 * max(1, SGFHE_CIRCUIT_CALL_ROWS / n), as in sgfhe_circuit_run_ct.  A group that has refreshed ciphertexts first
 * runs their bootstraps as ONE call (trivial encryption of 1 paired with every bit, AND branch, un-reduced;
 * row = rank * n + j, rank = the ciphertext's position among the group's refreshed ones in ascending q), which
 * takes one call number.  Every group then runs ONE tail (sgfhe_pack_lwe_modq: count = the group's ciphertexts,
 * z = index within the group), which takes one call number.  So a group equals, on one draw stream, an optional
 * sgfhe_bootstrap_batch(SGFHE_FLAG_RAW_MODQ) followed by one sgfhe_pack_lwe_modq.  No host synchronisation
 * before the final download.
 * With out_w NULL the flag changes nothing; blocks = 0 does nothing.
 *   SGFHE_CIRCUIT_PACK_LIFT  pack EVERY output without a refresh bootstrap.  It refines SGFHE_CIRCUIT_PACK_DIRECT and
 *       is given TOGETHER with it (flags = SGFHE_CIRCUIT_PACK_DIRECT | SGFHE_CIRCUIT_PACK_LIFT = 3); bit 1 on its own
 *       was an unknown bit before this flag existed and stays SGFHE_ERR_INVALID_ARG, as do bit 2 and above.  A
 *       ciphertext that is DIRECT above stays DIRECT (its raw gate rows are better than its reduced ones), and every
 *       other ciphertext -- an input wire, the constant, an XOR3 wire, any lane-shifted reference -- is LIFTED instead
 *       of REFRESHED.
 * A LIFTED ciphertext takes its n rows from the wire table as the pack stage's gather reads them (NOT, constant fill
 * and lane shift applied over Z_r), and one kernel per run of consecutive lifted ciphertexts of a group writes
 * sgfhe_lwe_lift_modq of every word into their rows of the raw output table.  Pack stage: the groups of
 * SGFHE_CIRCUIT_PACK_DIRECT, each being ONE tail and nothing else -- no bootstrap runs in the pack stage, and the pack
 * buffers hold no refresh rows.  Randomised flatten: the level calls as in sgfhe_circuit_run_ct, then exactly one call
 * number per group, the tail's, with z = the ciphertext's index within its group; a group equals one
 * sgfhe_pack_lwe_modq on the draw stream.  out_lwe keeps the bytes of the flags = 0 run in both modes; the wire table
 * is not touched.  With out_w NULL the flag changes nothing.  For ripple_adder(16) at Params(1024), one block: 16 n
 * level bootstraps, and 17 n refresh bootstraps with flags = 0, 16 n with PACK_DIRECT (only the carry-out is a gate
 * row), none with PACK_LIFT.
 * Noise -- why this is a flag of its own.  A lifted ciphertext is not bootstrapped.  Its bit error is the wire's Z_r
 * error plus the tail's.  For an XOR3 wire that is e_X + e_Y + e_Z - 2 e_MAJ.  The lift scales an error e over Z_r to
 * e Q / r over Z_Q (plus at most 1/2 per word of rounding) and cleans nothing, so the packed bit decrypts only while
 * the wire's own error plus the tail's stays below Dr/2.  Measure it with sgfhe_lwe_noise(SGFHE_FLAG_RAW_MODQ) on
 * sgfhe_lwe_lift_modq's output, or with the packed phase error after packing.  Measured on the CPU oracles,
 * ripple_adder(3) at Params(64): with inputs of error |e| <= Dr/16 the worst packed phase error of a sum bit is 39
 * and of the carry 6, against Dr/2 = 128; with split fresh encryptions (error up to Dr/4 - 1 each, see the noise
 * rule of three-input nodes above) the sum bits still decrypt but sit at 86 - 108 of 128.  So the flag is meant for inputs
 * that are themselves packed outputs (error about 22 of 2048 at Params(1024), RESULTS.md), or wherever the probe shows
 * room -- not for sums of freshly encrypted bits.  ripple_adder(16) at Params(1024) on inputs of |e| <= Dr/16: worst
 * packed phase error of a sum bit 538 lifted against 26 refreshed, of 2048 (RESULTS.md).
 */
#define SGFHE_CIRCUIT_PACK_DIRECT 1u
#define SGFHE_CIRCUIT_PACK_LIFT 2u
int32_t sgfhe_circuit_run_ct_ex(sgfhe_ctx *ctx, const sgfhe_circuit *c, size_t blocks, const uint64_t *in_a,
                                const uint64_t *in_b, size_t N, uint64_t *out_w, uint64_t *out_v, uint64_t *out_lwe,
                                uint32_t flags);

/*
 * The lift of LWEs from Z_r to Z_Q by exact scaling: out = L(word), L(x) = floor((x Q + r/2) / r), word by word, a and
 * b alike.  L maps a wrap of r to a wrap of Q, the codeword Dr to Q/4 (2 DQ_tilde to within 1) and adds at most 1/2
 * per word of rounding; ModRed of L(x) is x.  It does not clean the error (see SGFHE_CIRCUIT_PACK_LIFT).
 *   lwe [count][n + 1] uint64 in [0, r), a then b; out [count][n + 1][2] canonical 16-byte residues {lo, hi} -- the
 *   input layout of sgfhe_pack_lwe_modq and of sgfhe_lwe_noise(SGFHE_FLAG_RAW_MODQ).
 * Host pointers, synchronous, on the ctx stream; no bootstrap key is needed and the draw stream is not touched.
 * count = 0 does nothing.  A word that is not below r is SGFHE_ERR_INVALID_ARG before anything is queued.
 */
int32_t sgfhe_lwe_lift_modq(sgfhe_ctx *ctx, const uint64_t *lwe, size_t count, uint64_t *out);

/*
 * LUT bootstraps: any function of three bits in one bootstrap.
 *
 * A gate bootstrap separates the four phases 0, Dr, 2 Dr, 3 Dr of a sum of wires at codeword Dr = r/4, and the test
 * polynomial is antiperiodic with period r = 4 Dr, so only threshold functions of the sum come out of it.  Here the
 * three inputs arrive at the codewords Dr/4, Dr/2 and Dr: their sum has phase s Dr/4 + e with s = x0 + 2 x1 + 4 x2 in
 * 0..7, eight phases that fill exactly one half period, and ANY 8-entry truth table is an antiperiodic sign pattern
 * over them -- a +-1 combination of at most seven shifted copies of the step the accumulator holds.  The k-loop is the
 * one of sgfhe_bootstrap_batch; only its two ends differ.
 *
 *   a [batch][n], b [batch]   the rows over Z_r, already the sum X0 + X1 + X2 of the three inputs
 *   table [batch]             bit s of table[t] is the function value of row t at input sum s
 *   out [batch][3][n + 1]     (with SGFHE_FLAG_RAW_MODQ: [batch][3][n + 1][2], residues mod Q)
 *                             row 0 carries f at codeword Dr -- an ordinary wire --, row 1 at Dr/2, row 2 at Dr/4: a
 *                             division is impossible on an LWE and a multiplication is free, so the accumulator starts
 *                             at a quarter of the usual amplitude and the result leaves at x4, x2 and x1.  Any row can
 *                             feed the input position of its scale of a later LUT bootstrap.
 *
 * The contract, with A0 = DQ_tilde >> 2 and sigma(s) = +1 if bit s of the table is set, else -1, for s = 0..7:
 *   1. Init: the accumulator of sgfhe_bootstrap_batch for (a1, b1) = (a, b), (a2, b2) = 0 with A0 in place of DQ_tilde
 *      (in the randomised mode the draws are unchanged).
 *   2. The k-loop as it stands: the accumulators are those of sgfhe_debug_accumulators on a ctx whose
 *      sgfhe_params.DQ_tilde is A0.
 *   3. Extraction.  For a polynomial p of length m and i taken mod 2 m, P(p, i) = p[i] for i < m and -p[i - m] mod Q
 *      otherwise.  Set sigma(8) := -sigma(0); let j_0 < j_1 < ... be the j in 1..8 with sigma(j) != sigma(j - 1) (an
 *      odd number of them, at most 7), c(j) = (3 Dr - (2 j - 1) Dr/8) mod 2 m and kappa_i = -sigma(0) (-1)^i.  The base
 *      LWE over Z_Q is alpha[e] = sum_i kappa_i P(acc_a, c(j_i) - e) for e in 0..n-1 and
 *      beta = A0 + sum_i kappa_i P(acc_b, c(j_i)), all mod Q; its phase is A0 (1 + sigma(s)) when the phase of the
 *      input row is s Dr/4 + e with |e| < Dr/8.  Row k of `out` (k = 0, 1, 2) is 2^(2 - k) (alpha, beta) mod Q, written
 *      as 16-byte residues under SGFHE_FLAG_RAW_MODQ and through ModRed otherwise.
 *
 * Host pointers, synchronous, on the ctx stream; the ctx is locked for the call, and the call is never gathered with
 * other callers'.  The call takes the next call number of the ctx's draw stream, and row t draws as bootstrap t of that
 * call, exactly as in sgfhe_bootstrap_batch_device.  flags is 0 or SGFHE_FLAG_RAW_MODQ; anything else,
 * SGFHE_FLAG_RAW_RNS2 included, is SGFHE_ERR_INVALID_ARG, as are a NULL pointer and a word that is not below r (before
 * anything is queued, nothing written).  batch = 0 does nothing.  SGFHE_ERR_NO_KEY as elsewhere.
 *
 * The noise rule (MEASURED, as the rules of three-input and sum nodes are): a row is correct while the error of its
 * phase against s Dr/4 is below Dr/8 in absolute value -- the test polynomial is 0 exactly on the midpoint, so Dr/8
 * itself is not safe.  The errors of three summed inputs add un-weighted, so |e0 + e1 + e2| < Dr/8; a scaled row's own
 * error is its ModRed rounding, about the size of any bootstrapped wire's, whatever its scale.  The inputs must
 * therefore be bootstrapped rows: a fresh encryption after split is up to Dr/4 - 1 off and the oracle's
 * lwe_encrypt_bits up to Dr/8, and neither may enter, not even at the Dr/4 position.  Measured on the CPU oracles with
 * input errors up to +-(Dr/8 - 1), 16 rows and 18 tables, both flatten modes: every row decrypts at all three scales;
 * the Z_Q error of the combination is at most 8e-4 of the codeword; the Z_r error after ModRed at most 5 of Dr = 256
 * at Params(64) and 9 of Dr = 512 at Params(128).  At Params(1024) (Dr/8 = 512), 256 instances, inputs refreshed, then
 * fanned, then LUT bootstraps two levels deep, both flatten modes: max |e| of the rows 23 of Dr = 4096, 25 of Dr/2 and
 * 27 of Dr/4, the worst |e0 + e1 + e2| of a LUT input 36 -- a fourteenth of Dr/8; no row past a quarter of its
 * codeword (RESULTS.md, profiles/r14_circuit_lut.txt, tools/lut_bench.py).
 */
int32_t sgfhe_bootstrap_lut_batch(sgfhe_ctx *ctx, const uint64_t *a /* [batch][n] */, const uint64_t *b /* [batch] */,
                                  const uint8_t *table /* [batch] */, size_t batch,
                                  uint64_t *out /* [batch][3][n + 1], x2 words with SGFHE_FLAG_RAW_MODQ */, uint32_t flags);

/*
 * LUT families: several truth tables on one bootstrap's accumulator.
 *
 * The k-loop of a LUT bootstrap does not depend on the truth table: the table enters in step 3 of the contract above
 * alone, where it picks which of the eight coefficients P(acc, c(j) - e), j = 1..8, are combined with +-1.  Every
 * further function of the same three inputs therefore costs one more combination of eight values that are already
 * there, and its three output rows.
 *
 *   a [batch][n], b [batch]          as in sgfhe_bootstrap_lut_batch
 *   tables [batch][n_tables]         row t is evaluated under each of tables[t][0 .. n_tables)
 *   out [batch][n_tables][3][n + 1]  (with SGFHE_FLAG_RAW_MODQ: [batch][n_tables][3][n + 1][2], residues mod Q)
 *
 * The contract: out[t][j] is byte for byte out[t] of sgfhe_bootstrap_lut_batch called with table[t] = tables[t][j] at
 * the SAME call number of the same draw stream -- in both flatten modes, reduced and un-reduced, in every chunk, lane
 * and small-batch form.  The call takes ONE call number, and row t draws as bootstrap t of that call; n_tables = 1 is
 * sgfhe_bootstrap_lut_batch.  Each coefficient is reconstructed from the accumulator at most once per output word,
 * whatever the number of tables.
 *
 * Host pointers, synchronous, on the ctx stream; the ctx is locked for the call, and the call is never gathered with
 * other callers'.  Before anything is queued or written, SGFHE_ERR_INVALID_ARG: n_tables outside
 * 1..SGFHE_LUT_MAX_TABLES, flags other than 0 or SGFHE_FLAG_RAW_MODQ, a NULL pointer, a word that is not below r, and
 * batch * n_tables * (n + 1) above 2^31 (the device indexes rows and tables with 32 bits).  batch = 0 does nothing.
 * SGFHE_ERR_NO_KEY and SGFHE_ERR_OOM as elsewhere; nothing is written to `out` then.
 *
 * The noise rule is that of sgfhe_bootstrap_lut_batch, table by table.  The outputs of one row share an accumulator,
 * so their errors are correlated; each of them obeys the rule on its own, which is all that correctness needs.
 */
#define SGFHE_LUT_MAX_TABLES 256u
int32_t sgfhe_bootstrap_lut_multi_batch(sgfhe_ctx *ctx, const uint64_t *a /* [batch][n] */, const uint64_t *b /* [batch] */,
                                        const uint8_t *tables /* [batch][n_tables] */, size_t n_tables, size_t batch,
                                        uint64_t *out /* [batch][n_tables][3][n + 1], x2 words with SGFHE_FLAG_RAW_MODQ */,
                                        uint32_t flags);

/*
 * Noise probe: the LWE error of rows against the SECRET key, reduced on the device to exact integer statistics.
 * DIAGNOSTICS: the secret key crosses this boundary, so both entry points are for parameter studies and tests (what
 * the reference's examples/errors.jl and examples/depth.jl show), never part of a deployment.  The key bits are on
 * the device for the length of the call only.  Every statistic is an integer sum, count or maximum: a record does not
 * depend on launch geometry or summation order.
 *
 * sgfhe_lwe_noise: `count` rows (count < 2^32), host pointers, synchronous; no bootstrap key is needed.
 *   sk               n words, bit 0 of each is the key bit (as in sgfhe_bkey_generate)
 *   lwe              flags = 0: rows over Z_r, [n + 1] uint64, a then b;
 *                    flags = SGFHE_FLAG_RAW_MODQ: rows over Z_Q, [n + 1][2] canonical 16-byte residues, the layout
 *                    of a SGFHE_FLAG_RAW_MODQ result (and of sgfhe_pack_lwe_modq's input).  A residue that is not
 *                    below Q is SGFHE_ERR_INVALID_ARG before anything is queued.
 *   row_stride_words uint64 words from one row to the next, at least the row length (n + 1, or 2 (n + 1) and even over
 *                    Z_Q): 3 (n + 1) probes one gate of a [batch][3][n + 1] result in place
 *   expected[count]  the plaintext bit of every row (bit 0)
 * Z_r.  phase = b - sum a_i s_i mod r; e = the centred representative of phase - expected Dr mod r in (-r/2, r/2],
 * Dr = r / 4.
 *   stats[0] rows
 *   stats[1] rows that decrypt wrongly: ((phase + Dr/2) mod r) div Dr != expected, the rule of decrypt(::EncryptedBit)
 *            (src/fhe.jl:504-507); quotients 2 and 3 count as wrong
 *   stats[2] max |e|
 *   stats[3] sum e, two's-complement int64
 *   stats[4] sum e^2
 *   stats[5] rows with |e| >= Dr/4 (the margin of one input of the next gate)
 *   stats[6], [7] 0
 * Z_Q.  The codewords are 0 and 2 DQ_tilde (enc_trivial(true) = (0, 2 DQ_tilde)); e = the centred representative of
 * phase - expected 2 DQ_tilde mod Q in (-Q/2, Q/2].
 *   stats[0] rows
 *   stats[1] rows with |e| >= DQ_tilde
 *   stats[2], [3] max |e| as lo, hi
 *   stats[4], [5] sum |e| as lo, hi (|e| < 2^93 and count < 2^32: it fits)
 *   stats[6], [7] 0
 * count = 0 gives an all-zero record.  SGFHE_ERR_INVALID_ARG for NULL sk / stats (and lwe / expected when count > 0),
 * other flag bits, a short (or, over Z_Q, odd) stride, count >= 2^32.
 *
 * sgfhe_circuit_run_probe: the run of sgfhe_circuit_run -- same calls, rows and call numbers of the draw stream, `out`
 * has its bytes in both flatten modes -- that also measures every wire.
 *   in_bits [n_inputs][instances] the plaintext bit of every input LWE (may be NULL when n_inputs is 0)
 *   stats   [n_inputs + 3 n_gates][8]: one Z_r record per wire id -- inputs 0 .. n_inputs - 1, then AND, OR, XOR of
 *           node g at n_inputs + 3 g -- over all instances, against the circuit's plaintext evaluation of in_bits.
 *           Every wire of every live node is measured whether something reads it or not (the probe reads each level
 *           call's own result rows, after its last kernel and before the next call reuses them); the wires of pruned
 *           nodes get all-zero records; the constant has none.
 * The plaintext bits go up once per run as a bit table, the records come down once at the end; no host
 * synchronisation is added between levels.  The table of records is kept on the ctx like the wire table (grown on
 * demand, freed by sgfhe_release_host_staging and sgfhe_ctx_destroy).  Errors: those of sgfhe_circuit_run, and
 * SGFHE_ERR_INVALID_ARG for a NULL sk, in_bits or stats (nothing is written to `out`).
 */
int32_t sgfhe_lwe_noise(sgfhe_ctx *ctx, const uint64_t *sk, const uint64_t *lwe, size_t count,
                        size_t row_stride_words, const uint8_t *expected, uint32_t flags, uint64_t stats[8]);
int32_t sgfhe_circuit_run_probe(sgfhe_ctx *ctx, const sgfhe_circuit *c, size_t instances, const uint64_t *in,
                                uint64_t *out, const uint64_t *sk, const uint8_t *in_bits, uint64_t *stats);
/* The run entries of a plan with data planes ("Data planes" above): data [n_planes][instances] uint8. */
int32_t sgfhe_circuit_run_data(sgfhe_ctx *ctx, const sgfhe_circuit *c, size_t instances, const uint64_t *in,
                               const uint8_t *data, uint64_t *out);
int32_t sgfhe_circuit_run_ct_data(sgfhe_ctx *ctx, const sgfhe_circuit *c, size_t blocks, const uint64_t *in_a,
                                  const uint64_t *in_b, size_t N, const uint8_t *data, uint64_t *out_w,
                                  uint64_t *out_v, uint64_t *out_lwe, uint32_t flags);
int32_t sgfhe_circuit_run_probe_data(sgfhe_ctx *ctx, const sgfhe_circuit *c, size_t instances, const uint64_t *in,
                                     const uint8_t *data, uint64_t *out, const uint64_t *sk, const uint8_t *in_bits,
                                     uint64_t *stats);
/* The stepped runs of a plan with registers ("Registers and stepped runs" above). */
int32_t sgfhe_circuit_run_steps(sgfhe_ctx *ctx, const sgfhe_circuit *c, size_t instances, size_t steps,
                                const uint64_t *state_in /* [n_regs][instances][n + 1], NULL = every register FALSE */,
                                const uint64_t *in /* [steps][n_inputs - n_regs][instances][n + 1] */,
                                const uint8_t *data /* [steps][n_planes][instances] */,
                                const uint8_t *emit /* [steps], NULL = every step */,
                                uint64_t *out /* [emitted steps][n_outputs][instances][n + 1] */,
                                uint64_t *state_out /* [n_regs][instances][n + 1], optional */);
int32_t sgfhe_circuit_run_steps_ct(sgfhe_ctx *ctx, const sgfhe_circuit *c, size_t blocks, size_t steps,
                                   const uint64_t *state_a, const uint64_t *state_b /* [n_regs][blocks][N] */,
                                   const uint64_t *in_a, const uint64_t *in_b /* [steps][n_inputs - n_regs][blocks][N] */,
                                   size_t N, const uint8_t *data, const uint8_t *emit, uint64_t *out_w,
                                   uint64_t *out_v /* [emitted steps][n_outputs][blocks][m] */,
                                   uint64_t *out_lwe /* [emitted steps][n_outputs][blocks * n][n + 1] */,
                                   uint64_t *state_lwe /* [n_regs][blocks * n][n + 1], optional */, uint32_t flags);

/*
 * Device-resident runs: every run form with its inputs and outputs in device memory, asynchronous, with the contract
 * of sgfhe_bootstrap_batch_device.  Each entry is the most general host entry of its form -- sgfhe_circuit_run_data,
 * sgfhe_circuit_run_ct_data, sgfhe_circuit_run_steps, sgfhe_circuit_run_steps_ct -- plus a trailing `stream`.  A
 * packed output or a state_out of one run is the input of the next without leaving the device, and public LWE glue
 * between two runs (NOT, select, concatenate) is the caller's own device code on the same stream.
 *
 * Pointers.  Every array is device memory on the ctx's device, in the shape and layout of the host entry, `data`
 * included.  The one exception is `emit`: it steers the host loop, stays a host array and is read before the call
 * returns.  Pointer kinds are not validated (as in sgfhe_bootstrap_batch_device).  `data` may be NULL for a plan
 * without planes; a plan with planes goes through these entries only with `data`, a plan with registers through the
 * _steps entries only.
 *
 * Asynchronous, stream-ordered.  The work is queued on `stream` (a hipStream_t, NULL = the ctx's own), behind
 * everything earlier calls queued on this ctx on any stream, and the call returns when it is queued.  The outputs are
 * complete when that stream reaches the end of the call's work; sgfhe_sync waits for it on the host.  The inputs,
 * `data` and the circuit must stay alive until then (the circuit's tables go up by an asynchronous copy).  The ctx is
 * locked while the call queues.  A run whose ctx buffers are large enough waits for nothing on the host; a run that
 * must regrow one (the wire table, the call staging, the lanes' work buffers ...) first waits for the work queued on
 * the ctx, as a larger sgfhe_bootstrap_batch_device does.
 *
 * Bytes.  Every output word is the word the host entry writes for the same arguments on the same ctx state, in both
 * flatten modes and under every flag set, and the call consumes the same call numbers of the draw stream.
 * instances / blocks / steps = 0 does nothing and consumes nothing.
 *
 * No staging.  The LWE outputs are collected straight into `out` / `out_lwe`, the ciphertexts are split where they
 * are; inputs, state and planes, (w, v) and state_out are device-to-device copies on the run's stream.
 *
 * Aliasing.  No output range may overlap an input range, with one exception: state_out == state_in exactly.  The
 * state is read in full into the ctx's state buffer before anything is written, so a caller may keep one state array
 * and feed a stream chunk by chunk.
 *
 * Errors.  Everything the host entry rejects is rejected with the same code before anything is queued or written and
 * before a call number is taken.  Should queueing fail part way, the entry waits for the stream and returns the
 * error; the outputs are then unspecified.  The probe entries have no device form: they need host tables.
 */
int32_t sgfhe_circuit_run_device(sgfhe_ctx *ctx, const sgfhe_circuit *c, size_t instances, const uint64_t *in,
                                 const uint8_t *data, uint64_t *out, void *stream);
int32_t sgfhe_circuit_run_ct_device(sgfhe_ctx *ctx, const sgfhe_circuit *c, size_t blocks, const uint64_t *in_a,
                                    const uint64_t *in_b, size_t N, const uint8_t *data, uint64_t *out_w,
                                    uint64_t *out_v, uint64_t *out_lwe, uint32_t flags, void *stream);
int32_t sgfhe_circuit_run_steps_device(sgfhe_ctx *ctx, const sgfhe_circuit *c, size_t instances, size_t steps,
                                       const uint64_t *state_in, const uint64_t *in, const uint8_t *data,
                                       const uint8_t *emit /* host */, uint64_t *out, uint64_t *state_out,
                                       void *stream);
int32_t sgfhe_circuit_run_steps_ct_device(sgfhe_ctx *ctx, const sgfhe_circuit *c, size_t blocks, size_t steps,
                                          const uint64_t *state_a, const uint64_t *state_b, const uint64_t *in_a,
                                          const uint64_t *in_b, size_t N, const uint8_t *data,
                                          const uint8_t *emit /* host */, uint64_t *out_w, uint64_t *out_v,
                                          uint64_t *out_lwe, uint64_t *state_lwe, uint32_t flags, void *stream);

/*
 * Parity / debug hook: a circuit run with every bootstrap call and the pack tail replaced by a script, so that the glue
 * kernels of a run (k_circ_split, k_circ_gather, k_circ_xor3[_raw], k_circ_scatter[_raw], k_circ_raw_and, k_circ_lift,
 * k_circ_collect, k_circ_state_load, k_circ_next) work on caller-chosen words.  The run is built and checked as the run
 * entries build and check theirs, and walks the same calls with the same kernels, grids, buffers and job chunks; only
 *   - a level call: the gather runs; the staged rows of the call go to `staged`, and the call's LUT descriptor, if it
 *     carries one, to `lut`; in place of the bootstrap the script's result rows of the call are copied in; the call's
 *     XOR3 and scatter kernels follow;
 *   - the refresh call of a pack group: its gathers run, the staged rows are logged, and scripted un-reduced rows stand
 *     in for the bootstrap; k_circ_raw_and follows in a direct run (a lifted group has no call: k_circ_lift runs);
 *   - the tail: the rows it would read -- gate 0 of the refresh result, or with SGFHE_CIRCUIT_PACK_DIRECT the group's
 *     rows of the raw output table -- go to `tail_in`; no (w, v) is formed.
 *   form     : SGFHE_SCRIPT_CT (the arguments of sgfhe_circuit_run_ct_ex; otherwise those of sgfhe_circuit_run_data) |
 *              SGFHE_SCRIPT_STEPPED (those of sgfhe_circuit_run_steps[_ct]).  The probe and the device forms
 *              (SGFHE_SCRIPT_PROBE, SGFHE_SCRIPT_DEVICE) are refused.
 *   count, steps, N, data, emit, out, state_out, flags : as in the run entry of that form (steps, emit and state_out
 *              are read in the stepped forms, N and flags in the ciphertext forms); `out` is the LWE output
 *   in_a, in_b       : the ciphertext forms' inputs; the LWE forms take `in` as in_a and ignore in_b
 *   state_a, state_b : stepped: the ciphertext forms' first state; the LWE form takes state_in as state_a
 *   results  : the scripted calls' result rows, concatenated in the run's own call order -- per step the level calls,
 *              then the refresh calls of an emitted step's pack groups --, each block compact: [rows][3][n + 1] words
 *              of Z_r, or where the real run leaves the call un-reduced (a level call of a direct run that produces a
 *              direct output; every refresh call) [rows][3][n + 1][2] residues mod Q, {lo, hi}
 *   staged   : log, per scripted call [rows][2][n + 1]: input 1 then input 2 of every row, a then b
 *   lut      : log, per scripted call [rows] uint32: the descriptor words (0x100 | table for a LUT row, 0 for any
 *              other), 0 throughout for a call that carries no descriptor
 *   tail_in  : log [emitted steps][n_outputs * blocks][n][n + 1][2], or NULL: the run has no pack stage (then `out` or
 *              state_out is needed); this is what out_w / out_v are to a run entry
 * sgfhe_debug_circuit_script_calls gives the number of scripted calls of such a run (`pack`: tail_in is given), and
 * for the first `cap` of them the rows and whether they are un-reduced, so that a caller can size its arrays.
 * Needs no key, takes no call number and draws nothing: last_call and the draw stream stay as they were, and the bytes
 * are the same in either flatten mode.  Host pointers; synchronous.  SGFHE_ERR_INVALID_ARG, before anything is queued
 * or written: everything the run entries refuse (but a missing key), in their order and words; NULL results, staged or
 * lut; a scripted word that is not below r; a scripted residue that is not below Q; a plan with a live LUT sibling
 * (sgfhe_circuit_create_lut_multi) -- the sibling's wires are written into the wire table inside the bootstrap call, by
 * k_final_lut_multi from the accumulator, which result rows cannot stand in for.  An empty run (count or steps 0)
 * returns SGFHE_OK and touches nothing.
 */
#define SGFHE_SCRIPT_CT 1u
#define SGFHE_SCRIPT_STEPPED 2u
#define SGFHE_SCRIPT_PROBE 4u
#define SGFHE_SCRIPT_DEVICE 8u
int32_t sgfhe_debug_circuit_script(sgfhe_ctx *ctx, const sgfhe_circuit *circuit, uint32_t form, size_t count, size_t steps,
                                   const uint64_t *state_a, const uint64_t *state_b, const uint64_t *in_a,
                                   const uint64_t *in_b, size_t N, const uint8_t *data, const uint8_t *emit, uint64_t *out,
                                   uint64_t *state_out, uint32_t flags, const uint64_t *results, uint64_t *staged,
                                   uint32_t *lut, uint64_t *tail_in);
int32_t sgfhe_debug_circuit_script_calls(sgfhe_ctx *ctx, const sgfhe_circuit *circuit, uint32_t form, size_t count,
                                         size_t steps, const uint8_t *emit, int pack, uint32_t flags, size_t *n_calls,
                                         uint32_t *rows, uint8_t *raw, size_t cap);

/*
 * Measurement hook for bench.py: HIP-event timings taken on the ctx stream around sampled
 * launches of the two per-iteration kernels since the last reset (stats must hold 8 doubles).
 *   stats[0] = average external-product kernel time (ms)   stats[1] = its sampled launches
 *   stats[2] = average CRT/accumulate kernel time (ms)     stats[3] = its sampled launches
 *   stats[4] = bootstraps per external-product launch (chunk actually used)
 *   stats[5] = average device time of a whole sgfhe_bootstrap_batch_device call (ms), from its
 *              first to its last kernel on both lanes     stats[6] = calls   stats[7] = batch
 * With two lanes the kernels of the lanes overlap: stats[0] and [2] are then durations under
 * co-execution and do not add up to an iteration; stats[5] is the wall time.
 */
int32_t sgfhe_timing_enable(sgfhe_ctx *ctx, int enable);
int32_t sgfhe_timing_read(sgfhe_ctx *ctx, double *stats, int reset);
/* Names of the two k-loop kernels this ctx launches in its present flatten mode, as they appear in
 * a rocprofv3 kernel trace ("k_extprod<13, 4, false>", "k_crt_lean<5, 3>"; parameter sets outside
 * k_crt_lean's bounds give k_crt_acc2 / k_crt_acc), NUL-terminated into the
 * caller's buffers (64 bytes suffice). */
int32_t sgfhe_kernel_names(const sgfhe_ctx *ctx, char *extprod, size_t extprod_cap, char *crt,
                           size_t crt_cap);

#ifdef __cplusplus
}
#endif
#endif
