// Host side of libsgfhe_hip.so: context set-up (RNS primes, twiddle tables, CRT / flatten
// constants), bootstrap-key upload, lock-step batch scheduling, and the C ABI of
// include/sgfhe_hip.h.  Reference citations are relative to /root/reference.
#include "../../include/sgfhe_hip.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <type_traits>
#include <unordered_map>
#include <vector>

#include "kernels.h"
#include "circuit_masks.h"
#include "host_plumbing.h"
#include "coalescer.h"
#include "circuit.h"
#include "chunking.h"

using namespace sgfhe;

// wall clock in milliseconds (the SGFHE_DEBUG_IO phase lines)
static double wall_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// A grow-on-demand buffer that a ctx keeps between calls: device memory, or page-locked host memory
// (PINNED).  grow() never keeps the contents, and is called only when nothing of the ctx is in flight
// (after drain()); a failed allocation leaves the buffer empty and no sticky HIP error behind.
template <typename T, bool PINNED = false>
struct DevBuf {
    T *p = nullptr;
    size_t cap = 0;   // elements
    hipError_t grow(size_t words) {
        if (words <= cap) return hipSuccess;
        release();
        const hipError_t e = PINNED ? hipHostMalloc(&p, words * sizeof(T), hipHostMallocDefault) : hipMalloc(&p, words * sizeof(T));
        if (e != hipSuccess) {
            (void)hipGetLastError();
            p = nullptr;
            return e;
        }
        cap = words;
        return hipSuccess;
    }
    void release() {
        if (p) (void)(PINNED ? hipHostFree(p) : hipFree(p));
        p = nullptr;
        cap = 0;
    }
};
// Call-local device scratch: a DevBuf that frees itself.  An entry declares it BEFORE run_drained, so that it goes
// after run_drained has waited for the stream of a body that failed: no queued work outlives a buffer it uses.
namespace {
template <typename T>
struct Scratch : DevBuf<T> {
    Scratch() = default;
    Scratch(const Scratch &) = delete;
    Scratch &operator=(const Scratch &) = delete;
    ~Scratch() { this->release(); }
};
}  // namespace

// ---------------------------------------------------------------- ctx

// Device memory that a ctx and its clones (sgfhe_ctx_clone) have in common: the per-prime records and
// CRT / flatten constants of every basis, the twiddle tables, and the key in every form -- everything a
// bootstrap only reads.  Each allocation is registered here when it is made and freed when the last ctx
// that holds the block goes, so a clone may outlive the ctx it was taken from.
// (struct Coalescer -- the gathering of small calls across the ctxs that share a key -- is csrc/coalescer.h)
struct SharedDev {
    int device = 0;
    std::mutex mu;
    std::vector<void *> mem;
    Coalescer co;
    std::atomic<unsigned> clones{0};     // clones made of this block so far (their streams are shifted by it)
    void own(void *p) {
        std::lock_guard<std::mutex> g(mu);
        mem.push_back(p);
    }
    ~SharedDev() {
        (void)hipSetDevice(device);
        for (void *p : mem) (void)hipFree(p);
    }
};

// sgfhe_ctx is three groups of members and what is the ctx's own.  sgfhe_ctx_clone assigns the groups; a member
// added to one of them is cloned without another line anywhere.

// What a clone SHARES with the ctx it is taken from and only reads: the parameter set and its geometry, the RNS
// bases with their device constants and key forms, the twiddle tables, and the handle on the shared device memory.
struct CtxShared {
    sgfhe_params par;
    int device = 0;
    int logm = 0;
    uint32_t M = 0, n = 0;
    u128 Q = 0, B = 0;
    // ---- RNS bases ------------------------------------------------------------------------------
    // A ctx has one basis of word-size primes, or two: the deterministic flatten needs 5 m B Q below
    // the product of the primes, the randomised one 20 m B Q, and where that takes one prime more
    // (Params(1024): five against six) the ctx keeps a basis for each mode -- the key in both forms
    // (the form of the smaller basis is the larger one's times a constant per prime, derived on the
    // device), constants for both -- so that `bootstrap(bkey, rng, ...)` works on every ctx and the
    // deterministic mode never pays for the extra prime.  `active` is an index: everything that
    // launches kernels reads basis[active] through cur(); sgfhe_set_random_flatten sets it to the
    // mode's basis, and the key writers to the larger one while they work (key_begin / key_finish).
    struct Basis {
        uint32_t npr = 0;  // RNS primes in use: the fewest whose product covers the exactness bound
        uint32_t primes[NPR_MAX] = {};
        PrimeK *d_primes = nullptr;
        CrtConst *d_crt = nullptr;
        CrtConst h_crt;
        CrtLean *d_lean = nullptr;  // constants of k_crt_lean (nl = 0: this parameter set keeps k_crt_acc)
        CrtLean h_lean;
        bool lean_rnd_ok = false;   // k_crt_lean_rnd's width bounds hold for this parameter set (derive_basis)
        uint32_t pack_G = 1, pack_G_rnd = 0;  // key slices per exact-accumulation group of the packing path
                                              // (deterministic / randomised flatten; 0 = not available)
        int32_t *d_key = nullptr;
        size_t key_bytes = 0;
    } basis[2];
    int nb = 1;                   // bases in use (basis[0]: deterministic mode, basis[nb - 1]: randomised)
    uint32_t npr_max = 0;         // primes of the larger basis: work buffers are sized for it
    uint32_t tw_done = 0;         // primes whose twiddle tables are on the device
    // the read-only device memory of this ctx, shared with its clones (use_count() > 1: the key may not
    // be replaced, sgfhe_ctx_clone)
    std::shared_ptr<SharedDev> shared;
    // device constants
    int32_t *d_tw = nullptr;  // npr * 4 * M entries
    int32_t *d_twq = nullptr; // quarter form of the latency kernels: per prime 4 blocks [f_q | v_q | fp_q | vp_q] of m / 4 words
    int32_t *d_pow = nullptr; //   and psi^e * R mod p, e in [0, 2 m)
    int32_t tw_head[NPR_MAX][8] = {};   // f[1..3], fp[2], fp[3], v[1..3] of every prime (PrimeK::f1 ... v3)
    bool rnd_ok = false;      // the randomised flatten (rng != nothing, utils.jl:198-241) is available on this ctx
    uint32_t create_flags = 0;
};

// The scheduling knobs (sgfhe_set_chunk / _lanes / _small_batch_max and the environment): a clone STARTS with the
// values they have on the ctx it is taken from, and is then set on its own.
struct CtxKnobs {
    uint32_t chunk = 0, lanes = 2;   // work buffers: two lanes, each sized for `cap` bootstraps
    // the quarter form's two transform kernels as one launch (k_ext_quarter) from this many gates per chain, up to
    // what fills the device once (fused_cap below); SGFHE_SMALL_FUSED=0: never, =n: from n gates
    uint32_t fused_min = 7;
    uint32_t split_max = 7;   // calls of at most this many gates take the quarter form (SGFHE_SMALL_SPLIT, 0 = never):
                              // 1 / 2 / 4 / 6 / 8 gates 15.1 / 15.9 / 17.8 / 19.7 / 23.5 ms against 17.9 / 18.6 / 20.3 /
                              // 22.0 / 23.3 with one workgroup per transform (profiles/r04_exp_quarter.txt)
    bool small_padded = false;  // SGFHE_SMALL_PADDED=1: small-batch grids padded to 8 bootstraps as up to round 3 (A/B)
    bool small_lanes = true;    // SGFHE_SMALL_LANES=0: a call of a few gates as one chunk on one stream (A/B)
    uint32_t small_lanes_max = 24;   // ... up to this many gates (SGFHE_SMALL_LANES=<n>)
    uint32_t crt1_max = 0;      // k_crt_lean launches of at most this many coefficients take one per thread
                                // (SGFHE_CRT1_GATES gates' worth: default 8; 0 = never.  Same call, 1 / 2 / 4 / 8
                                // gates: 18.6 / 19.4 / 20.8 / 23.9 ms with four per thread, 17.9 / 18.6 / 20.2 / 23.4
                                // with one, profiles/r04_exp_crt1.txt)
    uint32_t small_max = 24;  // chunks of at most this many bootstraps take the small-batch form
                              // (measured crossover at Params(1024): 24 -> 32.3 vs 40.9 ms, 32 -> 44.0 vs 42.3 ms)
    bool use_pin = true;   // SGFHE_HOST_PIN=0 in the environment: direct copies (A/B measurements)
};

// The state of the key in the shared memory; a clone starts with the state it finds (a ctx without a key is not
// cloned) and, like every sharer, may not change it while the key is shared (key_begin).
struct CtxKeyState {
    bool have_key = false;      // basis[].d_key of every basis in use hold one key
    // RNS2Number form of Z_Q (src/rns.jl): set by sgfhe_bkey_upload_rns2 / sgfhe_rns2_convert
    bool have_rns2 = false;
    Rns2Const rns2;
};

// The ctx's OWN: everything below starts from its initialiser on a clone too -- flatten mode and call counters,
// the active basis, streams, events, work and staging buffers, timing, the error string and the lock.
struct sgfhe_ctx : CtxShared, CtxKnobs, CtxKeyState {
    int active = 0;               // the basis everything reads: cur()
    std::string err;
    // Every C-ABI entry point that takes a ctx holds this lock for the whole call: a ctx may be
    // shared by host threads (their calls are serialised), different ctxs run concurrently.
    mutable std::recursive_mutex mu;
    hipStream_t stream = nullptr;
    hipStream_t stream2 = nullptr;  // second lane: chunk i+1 overlaps its memory-bound k_crt_acc
                                    // with the VALU-bound k_extprod of chunk i
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    // Calls on one ctx are ordered on the device whatever stream each names: every call that queues
    // work first makes its stream wait for ev_done, the end of the previous call's work, and records
    // it again when its own work is queued (the lanes' work buffers, the key and the constants are
    // shared by all calls).  sgfhe_sync and everything that frees or replaces a buffer wait for it on
    // the host.
    hipEvent_t ev_done = nullptr;
    bool pending = false;           // ev_done has been recorded and may not have completed
    // copies of the host-pointer entry point, beside the lanes' kernels: uploads and downloads on
    // streams of their own (on one stream the upload of the next chunks would queue behind the
    // download of the present ones, which waits for their last kernel)
    hipStream_t stream_io = nullptr, stream_io2 = nullptr;
    std::vector<hipEvent_t> ev_pool;   // events of the pipelined host-pointer path (created once, reused)
    uint32_t *d_bad = nullptr;  // set by k_key_transform when a key residue is >= Q
    uint32_t cap = 0;           // bootstraps the lanes' work buffers are sized for
    // randomised flatten (rng != nothing, utils.jl:198-241)
    bool rnd = false;
    ChaChaKey rnd_key = {};   // 32-byte key of the draw stream (sgfhe_set_random_flatten[_key])
    uint32_t rnd_call = 0, last_call = 0;
    int64_t call_fixed = -1;              // the number of the next call, when the coalescer has already assigned it
    const RndRow *gather_rows = nullptr;  // set around a gathered randomised call this ctx leads: d_rows
    DevBuf<RndRow> d_rows;                // per-row draw streams of such a call (device)
    std::vector<RndRow> h_rows;
    struct Lane {
        uint64_t *dig = nullptr;
        uint32_t *yres = nullptr;
        uint32_t *ua = nullptr;
        int32_t *zpart = nullptr;  // small-batch form only: [cap_small][npr][4][2][m]
    } lane[2];
    // staging buffers of the host-pointer entry point (sgfhe_bootstrap_batch: the drop-in signature of
    // fhe.jl:608-610, usually called with one gate): grown on demand and kept, so that a call does
    // not pay a hipMalloc / hipFree pair (hipFree synchronises the device)
    DevBuf<uint64_t> io_in, io_out;
    // ... and their page-locked host mirrors.  hipMemcpyAsync on pageable memory above about 1 MB
    // pins the caller's pages for the copy, a fixed cost of several milliseconds per copy
    // (profiles/r03_latency.txt: 256 gates 155.6 ms through host pointers against 127.6 ms from
    // device buffers, 64 gates 43.6 against 43.4); below PIN_MAX_BYTES per buffer the engine
    // copies through its own pinned buffers instead (one CPU memcpy + one true DMA).
    DevBuf<uint64_t, true> pin_in, pin_out;
    std::vector<uint64_t> co_buf;   // gathered inputs and results of a combined call this ctx leads (Coalescer)
    // device buffers of sgfhe_circuit_run, grown on demand and kept like the I/O staging: the wire table
    // [slot][instance][n + 1], one call's staging [a1 | a2 | b1 | b2 | result rows], the plan's node tables,
    // and the collected outputs
    DevBuf<uint64_t> circ_wires, circ_stage, circ_out;
    DevBuf<uint32_t> circ_tab;
    DevBuf<uint8_t> circ_data;            // the data planes of a run (sgfhe_circuit_run_data): [n_planes][instances]
    // sgfhe_circuit_run_steps: the registers between steps, [n_regs][instances][n + 1]
    DevBuf<uint64_t> circ_state;
    // sgfhe_circuit_run_ct: the uploaded input ciphertexts [a | b], each [n_inputs][blocks][N]
    DevBuf<uint64_t> circ_ct;
    // work buffers of the packing path (pack_tail), shared by sgfhe_pack_encrypted_bits and the pack stage
    // of sgfhe_circuit_run_ct, grown and freed like the circuit buffers: one call's bootstrap inputs
    // [a1 | a2 | b1 | b2], its un-reduced results, the flattened as_i, the group sums, and (w | v)
    DevBuf<uint64_t> pack_lwe, pack_pdig, pack_wv;
    DevBuf<ulonglong2> pack_raw;
    DevBuf<uint32_t> pack_yg;
    // SGFHE_CIRCUIT_PACK_DIRECT: the raw output table [n_outputs * blocks][n][n + 1] of 16-byte residues over Z_Q,
    // the un-reduced LWEs of every output ciphertext on their way into the pack tail
    DevBuf<ulonglong2> circ_raw;
    // noise probe (sgfhe_lwe_noise, sgfhe_circuit_run_probe), grown and freed like the circuit buffers: the per-wire
    // records, the partial records of k_lwe_noise_q, the key mask and the plaintext bit table (noise_layout); and the
    // rows the probe reads that no other buffer holds (the primitive's LWEs, a probed run's unread inputs)
    DevBuf<uint64_t> noise_tab, noise_lwe;
    // timing
    bool timing = false;
    struct EvTriple { hipEvent_t e0, e1, e2; };  // ext = e0 -> e1, crt = e1 -> e2
    std::vector<EvTriple> ev;
    double t_ext = 0, t_crt = 0;
    uint64_t n_ext = 0, n_crt = 0;
    uint32_t last_chunk = 0;
    // whole bootstrap_device calls (fork ... join): the k-loop's wall time on the device when the
    // kernels of two lanes overlap and per-kernel durations no longer add up
    struct EvPair { hipEvent_t e0, e1; uint64_t batch; };
    std::vector<EvPair> ev_call;
    double t_call = 0;
    uint64_t n_call = 0, boots_call = 0;
    // kernels whose dynamic-LDS limit has been raised on this ctx's device (hipFuncSetAttribute is
    // per device; a ctx is bound to one device and used by one host thread)
    uint32_t attr_done = 0;
};
enum : uint32_t { ATTR_EXTPROD = 1u, ATTR_SMALL = 2u, ATTR_SHORTPROD = 4u, ATTR_FUSED = 8u };
// Page-locked mirrors of the host-pointer entry point's staging buffers: per buffer at most this much
// (a batch of 16384 at Params(1024) needs 268 + 403 MB).  Round 3 staged whole buffers and stopped at
// 48 MB, where one CPU memcpy cost what pinning the caller's pages did; the copies are now pipelined
// chunk by chunk beside the kernels (HostPipe), so their size no longer matters.
static constexpr size_t PIN_MAX_BYTES = (size_t)1 << 30;
// SGFHE_PIN_MAX_MB=<n> in the environment lowers the limit (read at every host-pointer call): lets a test
// send a small batch down the direct-copy path that batches above 1 GiB take (tests/test_gpu_round5.py).
static size_t pin_max_bytes() {
    const char *env = getenv("SGFHE_PIN_MAX_MB");
    if (env && *env) {
        const long mb = atol(env);
        if (mb >= 0 && (size_t)mb < (PIN_MAX_BYTES >> 20)) return (size_t)mb << 20;
    }
    return PIN_MAX_BYTES;
}

namespace {

#define SGFHE_LOCK(ctx) std::lock_guard<std::recursive_mutex> lock_((ctx)->mu)
// A synchronous entry point that touches the key, the constants or the lanes' buffers on the ctx
// stream first waits (on the host) for the work of earlier asynchronous calls.
#define SGFHE_QUIESCE(ctx)                                                                        \
    do {                                                                                          \
        int32_t rq_ = drain(ctx);                                                                 \
        if (rq_) return rq_;                                                                      \
    } while (0)

#define HIPCHK(ctx, call)                                                                         \
    do {                                                                                          \
        hipError_t e_ = (call);                                                                   \
        if (e_ != hipSuccess) {                                                                   \
            char buf_[512];                                                                       \
            snprintf(buf_, sizeof buf_, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_),    \
                     __FILE__, __LINE__);                                                         \
            (ctx)->err = buf_;                                                                    \
            return SGFHE_ERR_HIP;                                                                 \
        }                                                                                         \
    } while (0)

int32_t fail(sgfhe_ctx *ctx, int32_t code, const std::string &msg) {
    if (ctx) ctx->err = msg;
    return code;
}

// Start of a call that queues work on `st`: that work begins after everything earlier calls queued.
int32_t fence_begin(sgfhe_ctx *c, hipStream_t st) {
    if (c->pending) HIPCHK(c, hipStreamWaitEvent(st, c->ev_done, 0));
    return SGFHE_OK;
}
// End of such a call: its last work on `st` (the lanes have been joined into it).
int32_t fence_end(sgfhe_ctx *c, hipStream_t st) {
    HIPCHK(c, hipEventRecord(c->ev_done, st));
    c->pending = true;
    return SGFHE_OK;
}
// Host waits for all work queued on the ctx (before buffers are freed or replaced, and in sgfhe_sync).
int32_t drain(sgfhe_ctx *c) {
    if (c->pending) {
        HIPCHK(c, hipEventSynchronize(c->ev_done));
        c->pending = false;
    }
    return SGFHE_OK;
}

// the basis everything reads: basis[active]
sgfhe_ctx::Basis &cur(sgfhe_ctx *c) { return c->basis[c->active]; }
const sgfhe_ctx::Basis &cur(const sgfhe_ctx *c) { return c->basis[c->active]; }
// the basis of the present flatten mode, and the k-loop's mode word in it
int mode_basis(const sgfhe_ctx *c) { return c->rnd ? c->nb - 1 : 0; }
uint32_t flatten_mode(const sgfhe_ctx *c) { return c->rnd ? (MODE_RANDOM | ((c->B >> 46) ? MODE_WIDE : 0u)) : 0u; }
// key slices per exact-accumulation group of the packing path in the present mode (0 = not available)
uint32_t pack_group(const sgfhe_ctx *c) { return c->rnd ? cur(c).pack_G_rnd : cur(c).pack_G; }

// ---- which kernels a launch takes ---------------------------------------------------------------
// Pure functions of the ctx and the launch's own numbers.  The launchers below act on what they
// return and hold no selection of their own; sgfhe_kernel_names formats the same values.

// The quarter form of the latency kernels exists for m >= 4096 where the lean CRT kernel of the flatten mode does
// (both modes; not the three-plane digit records of B >= 2^46, MODE_WIDE).
bool quarter_ok(const sgfhe_ctx *c, uint32_t mode) {
    return c->logm >= 12 && c->split_max &&
           (mode == 0u ? cur(c).h_lean.nl != 0 : (mode == MODE_RANDOM && cur(c).lean_rnd_ok));
}
// Largest chain the fused quarter kernel takes: one workgroup per (gate, prime, quarter), one round of the
// device's 256 compute units (12 gates on five primes, 10 on six); 0 where it does not exist (m < 4096,
// m = 16384, where its workgroup of 1024 threads leaves 128 registers per thread and spills: kernels.h) or
// is switched off.
uint32_t fused_cap(const sgfhe_ctx *c, uint32_t mode) {
    if (!c->fused_min || c->small_padded || (c->logm != 12 && c->logm != 13) || !quarter_ok(c, mode)) return 0;
    return 256u / (cur(c).npr * 4u);
}

// The external product of one chunk of `cb` bootstraps (`cpad`: padded to a multiple of 8).
enum class ExtKind {
    Throughput,   // k_extprod: one workgroup per (bootstrap, prime)
    Small,        // k_fwd_phase + k_inv_column: six
    Quarter,      // k_fwd_quarter + k_inv_quarter: each transform cut across four workgroups
    Fused         // k_ext_quarter: the quarter pair as one launch
};
struct ExtForm {
    ExtKind kind;
    uint32_t cnt;   // gates the grids (the CRT's too) are sized by
    bool quarter() const { return kind == ExtKind::Quarter || kind == ExtKind::Fused; }
};
ExtForm ext_form(const sgfhe_ctx *c, uint32_t mode, uint32_t cb, uint32_t cpad, bool has_zpart) {
    const bool small = cpad <= c->small_max && has_zpart;
    // (the small-batch kernels index bootstraps directly: no padding to a multiple of 8, which is
    // k_extprod's XCD mapping's; a one-gate call then runs one gate's workgroups, not eight's)
    const uint32_t cnt = small && !c->small_padded ? cb : cpad;
    if (small && cnt >= c->fused_min && cnt <= fused_cap(c, mode)) return {ExtKind::Fused, cnt};
    // a few gates, m >= 4096
    if (small && quarter_ok(c, mode) && cnt <= c->split_max) return {ExtKind::Quarter, cnt};
    return {small ? ExtKind::Small : ExtKind::Throughput, cnt};
}

// The CRT of `total` coefficients.
enum class CrtKind { Lean, LeanRnd, Acc2, Acc };   // k_crt_lean*, k_crt_lean_rnd*, k_crt_acc2, k_crt_acc
struct CrtForm {
    CrtKind kind;
    uint32_t np, nl;   // template arguments: primes, and (lean kinds) 29-bit limbs of Q
    bool wide;         // LeanRnd: digit records with a third plane
    bool rows;         // LeanRnd, Acc: a gathered call, every row on the draw stream of the ctx it came in on (RndRow)
    bool p87;          // Lean: the crt_lean87_one instantiation k_crt_lean<5, 3, true>
    bool one;          // lean kinds: one coefficient per thread (k_crt_lean1, k_crt_lean_rnd1), not four
    bool quarter;      // lean kinds: partial residues in, the last two inverse stages inside (k_crt_lean1q, k_crt_lean_rnd1)
    uint32_t per_thread() const { return kind == CrtKind::Acc2 ? 2u : (kind == CrtKind::Acc || one) ? 1u : 4u; }
};
// `quarter`: the chunk's external product took the quarter form (ExtForm::quarter(): the mode's lean kernel exists)
CrtForm crt_form(const sgfhe_ctx *c, uint32_t mode, uint32_t total, bool rows, bool quarter = false) {
    const sgfhe_ctx::Basis &S = cur(c);
    CrtForm f = {CrtKind::Acc, S.npr, S.h_lean.nl, false, false, false, false, quarter};
    if (quarter) {
        f.kind = (mode & MODE_RANDOM) ? CrtKind::LeanRnd : CrtKind::Lean;
        f.one = true;
    } else if (mode == 0u && S.h_lean.nl != 0) {
        // the k-loop's own case (deterministic flatten, accumulator present): the integer-only kernel, four
        // coefficients per thread -- one for a handful of gates (the latency form: four times the threads)
        f.kind = CrtKind::Lean;
        f.one = total <= c->crt1_max;
        f.p87 = !f.one && S.npr == 5 && S.h_lean.p87;
    } else if ((mode & ~MODE_WIDE) == MODE_RANDOM && S.lean_rnd_ok) {
        // the same for the randomised flatten (the k-loop's modes MODE_RANDOM and MODE_RANDOM | MODE_WIDE)
        f.kind = CrtKind::LeanRnd;
        f.wide = (mode & MODE_WIDE) != 0;
        f.one = !f.wide && total <= c->crt1_max;
    } else if (mode == 0u) {
        f.kind = CrtKind::Acc2;   // parameter sets outside the lean kernel's bounds (B < 2^12, Q < 2^30): two per thread
    }                             // every other mode: the general kernel
    f.rows = rows && (f.kind == CrtKind::LeanRnd || f.kind == CrtKind::Acc);
    return f;
}

size_t lds_bytes(int logm, int npoly) { return (size_t)npoly * ((size_t)4 << logm); }
// points per thread of k_extprod: 16, or 8 where 16 would leave half a wavefront idle (m <= 512)
template <int LOGM> constexpr int ext_loge() { return LOGM <= EXT_LE3_MAX ? 3 : LOGE; }
template <int LOGM> constexpr int threads_of() { return NttGeom<LOGM, LOGE>::T; }
// points per thread of k_fwd_phase / k_inv_column: 8 while m / 8 threads fit a workgroup, else the engine's 16
constexpr int small_loge(int logm) { return (logm - 3 <= 10 && logm >= 9) ? 3 : LOGE; }
constexpr int QUARTER_LOGE = 3;   // ... of the quarter kernels

// The kernels of a form as a rocprofv3 kernel trace names them (sgfhe_kernel_names, sgfhe_debug_kloop_step): the
// only place that turns an ExtForm / CrtForm into text.
void ext_form_name(const sgfhe_ctx *c, ExtForm f, uint32_t mode, char *out, size_t cap) {
    const char *wide = (mode & MODE_WIDE) ? "true" : "false";
    const int lm = c->logm, ls = small_loge(lm);
    switch (f.kind) {
    case ExtKind::Throughput: snprintf(out, cap, "k_extprod<%d, %d, %s>", lm, lm <= EXT_LE3_MAX ? 3 : LOGE, wide); break;
    case ExtKind::Small: snprintf(out, cap, "k_fwd_phase<%d, %d, %s>+k_inv_column<%d, %d>", lm, ls, wide, lm, ls); break;
    case ExtKind::Quarter:
        snprintf(out, cap, "k_fwd_quarter<%d, %d>+k_inv_quarter<%d, %d>", lm, QUARTER_LOGE, lm, QUARTER_LOGE);
        break;
    case ExtKind::Fused: snprintf(out, cap, "k_ext_quarter<%d, %d>", lm, QUARTER_LOGE); break;
    }
}
void crt_form_name(CrtForm f, char *out, size_t cap) {
    switch (f.kind) {
    case CrtKind::Lean:
        if (f.quarter) snprintf(out, cap, "k_crt_lean1q<%u, %u>", f.np, f.nl);
        else if (f.one) snprintf(out, cap, "k_crt_lean1<%u, %u>", f.np, f.nl);
        else snprintf(out, cap, f.p87 ? "k_crt_lean<%u, %u, true>" : "k_crt_lean<%u, %u>", f.np, f.nl);
        break;
    case CrtKind::LeanRnd:
        if (f.quarter || f.one) snprintf(out, cap, "k_crt_lean_rnd1<%u, %u, %s>", f.np, f.nl, f.quarter ? "true" : "false");
        else snprintf(out, cap, "k_crt_lean_rnd<%u, %u, %s>", f.np, f.nl, f.wide ? "true" : "false");
        break;
    case CrtKind::Acc2: snprintf(out, cap, "k_crt_acc2<%u>", f.np); break;
    case CrtKind::Acc: snprintf(out, cap, "k_crt_acc<%u>", f.np); break;
    }
}

// ---- one dispatcher per template axis -------------------------------------------------------------
// Each hands the run-time value to a generic lambda as a compile-time constant.  What a lambda
// instantiates is what the library holds: kernels that exist for part of an axis only are kept out
// with `if constexpr` at the launch.

template <class F> int32_t with_logm(sgfhe_ctx *c, F &&f) {
    switch (c->logm) {
#define X(LM) case LM: return f(std::integral_constant<int, LM>{});
        X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14)
#undef X
    }
    return fail(c, SGFHE_ERR_UNSUPPORTED, "unsupported log2(m)");
}
// (the CRT kernels are compiled once per prime count: their residue loops are unrolled)
template <class F> int32_t with_npr(sgfhe_ctx *c, uint32_t npr, F &&f) {
    switch (npr) {
#define X(NP) case NP: return f(std::integral_constant<int, NP>{});
        X(2) X(3) X(4) X(5) X(6) X(7)
#undef X
    }
    return fail(c, SGFHE_ERR_UNSUPPORTED, "unsupported number of RNS primes");
}
template <class F> void with_nl(uint32_t nl, F &&f) {
    switch (nl) {
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 3: f(std::integral_constant<int, 3>{}); break;
    default: f(std::integral_constant<int, 4>{}); break;
    }
}
template <class F> void with_bool(bool b, F &&f) {
    if (b) f(std::true_type{});
    else f(std::false_type{});
}

// ---- launchers --------------------------------------------------------------------------------

int32_t launch_extprod(sgfhe_ctx *c, const sgfhe_ctx::Lane &L, const int32_t *keyk, uint32_t cpad,
                       uint32_t k, uint32_t mode, hipStream_t st) {
    return with_logm(c, [&](auto lm) -> int32_t {
        constexpr int LOGM = decltype(lm)::value, LE = ext_loge<LOGM>();
        const size_t lds = lds_bytes(LOGM, 2);  // exchange buffer + z1 accumulator
        if (!(c->attr_done & ATTR_EXTPROD)) {
            HIPCHK(c, hipFuncSetAttribute((const void *)k_extprod<LOGM, LE, false>,
                                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            HIPCHK(c, hipFuncSetAttribute((const void *)k_extprod<LOGM, LE, true>,
                                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            c->attr_done |= ATTR_EXTPROD;
        }
        with_bool(mode & MODE_WIDE, [&](auto wide) {   // digit planes with a third plane (randomised flatten, B >= 2^46)
            hipLaunchKernelGGL((k_extprod<LOGM, LE, decltype(wide)::value>), dim3(cpad * cur(c).npr),
                               dim3(NttGeom<LOGM, LE>::T), lds, st, L.dig, keyk, L.yres, L.ua, cur(c).d_primes, k,
                               c->n, mode);
        });
        HIPCHK(c, hipGetLastError());
        return SGFHE_OK;
    });
}

int32_t launch_small(sgfhe_ctx *c, const sgfhe_ctx::Lane &L, const int32_t *keyk, uint32_t cnt,
                     uint32_t k, uint32_t mode, hipStream_t st) {
    return with_logm(c, [&](auto lm) -> int32_t {
        constexpr int LOGM = decltype(lm)::value;
        constexpr int LE = small_loge(LOGM);
        constexpr int TH = NttGeom<LOGM, LE>::T;
        const size_t lds = lds_bytes(LOGM, 1);
        if (!(c->attr_done & ATTR_SMALL)) {
            HIPCHK(c, hipFuncSetAttribute((const void *)k_fwd_phase<LOGM, LE, false>,
                                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            HIPCHK(c, hipFuncSetAttribute((const void *)k_fwd_phase<LOGM, LE, true>,
                                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            HIPCHK(c, hipFuncSetAttribute((const void *)k_inv_column<LOGM, LE>,
                                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            c->attr_done |= ATTR_SMALL;
        }
        // (Round 4 measured the per-prime records passed by value in the kernel arguments instead of
        // through this pointer -- one dependent load less at the head of each launch: 24.75 against
        // 24.74 ms per call, no change, profiles/r04_exp_small_args.txt.)
        PrimeSet ps = cur(c).d_primes;
        const uint32_t npr = cur(c).npr;
        with_bool(mode & MODE_WIDE, [&](auto wide) {
            hipLaunchKernelGGL((k_fwd_phase<LOGM, LE, decltype(wide)::value>), dim3(cnt * npr * 4), dim3(TH), lds, st,
                               L.dig, keyk, L.zpart, ps, mode);
        });
        hipLaunchKernelGGL((k_inv_column<LOGM, LE>), dim3(cnt * npr * 2), dim3(TH), lds, st, L.zpart,
                           L.yres, L.ua, ps, k, c->n);
        HIPCHK(c, hipGetLastError());
        return SGFHE_OK;
    });
}

// The quarter form of the two transform kernels (kernels.h k_fwd_quarter / k_inv_quarter), m >= 4096;
// `fused`: both in one launch (kernels.h k_ext_quarter), m = 4096 and 8192.
int32_t launch_quarter(sgfhe_ctx *c, const sgfhe_ctx::Lane &L, const int32_t *keyk, uint32_t cnt, bool fused,
                       uint32_t k, uint32_t mode, hipStream_t st) {
    return with_logm(c, [&](auto lm) -> int32_t {
        constexpr int LOGM = decltype(lm)::value;
        if constexpr (LOGM >= 12) {
            constexpr int LE = QUARTER_LOGE;
            constexpr int TH = NttGeom<LOGM - 2, LE>::T;
            const sgfhe_ctx::Basis &S = cur(c);
            if constexpr (LOGM <= 13) if (fused) {
                const size_t ldsf = (size_t)6 * (sizeof(uint32_t) << (LOGM - 2));
                if (!(c->attr_done & ATTR_FUSED)) {
                    HIPCHK(c, hipFuncSetAttribute((const void *)k_ext_quarter<LOGM, LE>,
                                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsf));
                    c->attr_done |= ATTR_FUSED;
                }
                hipLaunchKernelGGL((k_ext_quarter<LOGM, LE>), dim3(cnt * S.npr * 4), dim3(2 * TH), ldsf, st, L.dig, keyk,
                                   reinterpret_cast<int32_t *>(L.yres), L.ua, S.d_primes, mode, k, c->n);
                HIPCHK(c, hipGetLastError());
                return SGFHE_OK;
            }
            const size_t lds = lds_bytes(LOGM - 2, 1);
            hipLaunchKernelGGL((k_fwd_quarter<LOGM, LE>), dim3(cnt * S.npr * 16), dim3(TH), lds, st, L.dig, keyk,
                               L.zpart, S.d_primes, mode);
            hipLaunchKernelGGL((k_inv_quarter<LOGM, LE>), dim3(cnt * S.npr * 8), dim3(TH), lds, st, L.zpart,
                               reinterpret_cast<int32_t *>(L.yres), L.ua, S.d_primes, k, c->n);
            HIPCHK(c, hipGetLastError());
            return SGFHE_OK;
        } else {
            return fail(c, SGFHE_ERR_UNSUPPORTED, "quarter form needs m >= 4096");
        }
    });
}

// the external product of one chunk in the form the selector chose
int32_t launch_ext(sgfhe_ctx *c, const sgfhe_ctx::Lane &L, const int32_t *keyk, ExtForm f, uint32_t k,
                   uint32_t mode, hipStream_t st) {
    switch (f.kind) {
    case ExtKind::Throughput: return launch_extprod(c, L, keyk, f.cnt, k, mode, st);
    case ExtKind::Small: return launch_small(c, L, keyk, f.cnt, k, mode, st);
    default: return launch_quarter(c, L, keyk, f.cnt, f.kind == ExtKind::Fused, k, mode, st);
    }
}

int32_t launch_shortprod(sgfhe_ctx *c, const uint64_t *pdig, uint32_t *yg, uint32_t count,
                         uint32_t G, uint32_t groups, uint32_t mode, hipStream_t st) {
    return with_logm(c, [&](auto lm) -> int32_t {
        constexpr int LOGM = decltype(lm)::value;
        const sgfhe_ctx::Basis &S = cur(c);
        const size_t lds = lds_bytes(LOGM, 2);
        if (!(c->attr_done & ATTR_SHORTPROD)) {
            HIPCHK(c, hipFuncSetAttribute((const void *)k_shortprod<LOGM>,
                                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            c->attr_done |= ATTR_SHORTPROD;
        }
        hipLaunchKernelGGL(k_shortprod<LOGM>, dim3(count * groups * S.npr), dim3(threads_of<LOGM>()), lds,
                           st, pdig, S.d_key, yg, S.d_primes, S.d_crt, c->n, G, groups, mode);
        HIPCHK(c, hipGetLastError());
        return SGFHE_OK;
    });
}

int32_t launch_keygen_ntt(sgfhe_ctx *c, const uint64_t *d_sk, int32_t *d_shat,
                          const ulonglong2 *d_acan, uint32_t *d_y, uint32_t R, bool shat_pass,
                          hipStream_t st) {
    return with_logm(c, [&](auto lm) -> int32_t {
        constexpr int LOGM = decltype(lm)::value;
        const sgfhe_ctx::Basis &S = cur(c);
        if (shat_pass)
            hipLaunchKernelGGL(k_shat<LOGM>, dim3(S.npr), dim3(threads_of<LOGM>()), lds_bytes(LOGM, 1), st,
                               d_sk, d_shat, S.d_primes, c->n);
        else
            hipLaunchKernelGGL(k_polymul_s<LOGM>, dim3(R * S.npr), dim3(threads_of<LOGM>()),
                               lds_bytes(LOGM, 1), st, d_acan, d_shat, d_y, S.d_primes, S.d_crt);
        HIPCHK(c, hipGetLastError());
        return SGFHE_OK;
    });
}

int32_t launch_keytr(sgfhe_ctx *c, const ulonglong2 *canon, int32_t *keyhat, uint32_t poly0,
                     uint32_t npolys, hipStream_t st) {
    return with_logm(c, [&](auto lm) -> int32_t {
        constexpr int LOGM = decltype(lm)::value;
        hipLaunchKernelGGL(k_key_transform<LOGM>, dim3(npolys * cur(c).npr), dim3(threads_of<LOGM>()),
                           lds_bytes(LOGM, 1), st, canon, keyhat, cur(c).d_primes, cur(c).d_crt, poly0,
                           c->d_bad);
        HIPCHK(c, hipGetLastError());
        return SGFHE_OK;
    });
}

int32_t launch_dbgntt(sgfhe_ctx *c, const uint32_t *in, uint32_t *out, uint32_t pi, int inverse,
                      hipStream_t st) {
    return with_logm(c, [&](auto lm) -> int32_t {
        constexpr int LOGM = decltype(lm)::value;
        hipLaunchKernelGGL(k_debug_ntt<LOGM>, dim3(1), dim3(threads_of<LOGM>()), lds_bytes(LOGM, 1), st,
                           in, out, cur(c).d_primes, pi, (uint32_t)inverse);
        HIPCHK(c, hipGetLastError());
        return SGFHE_OK;
    });
}

// The CRT of `total` coefficients in the form crt_form chooses (`quarter`: after a quarter-form external product).
int32_t launch_crt_raw(sgfhe_ctx *c, const uint32_t *yres, uint64_t *dig, uint32_t total, uint32_t mode,
                       hipStream_t st, RndArgs ra, uint32_t iter, bool quarter = false, CrtForm *used = nullptr) {
    const sgfhe_ctx::Basis &S = cur(c);
    const CrtForm f = crt_form(c, mode, total, ra.rows != nullptr, quarter);
    if (used) *used = f;
    const uint32_t logm = (uint32_t)c->logm, work = total / f.per_thread();
    const dim3 grid((work + 255) / 256), block(256);
    const int32_t rc = with_npr(c, f.np, [&](auto np) -> int32_t {
        constexpr int NP = decltype(np)::value;
        switch (f.kind) {
        case CrtKind::Acc2:
            hipLaunchKernelGGL(k_crt_acc2<NP>, grid, block, 0, st, yres, dig, S.d_crt, work, logm);
            break;
        case CrtKind::Acc:
            with_bool(f.rows, [&](auto rows) {
                hipLaunchKernelGGL((k_crt_acc<NP, decltype(rows)::value>), grid, block, 0, st, yres, dig, S.d_crt, work,
                                   logm, mode, ra, iter);
            });
            break;
        case CrtKind::Lean:
            with_nl(f.nl, [&](auto nl) {
                constexpr int NL = decltype(nl)::value;
                if (f.quarter)
                    hipLaunchKernelGGL((k_crt_lean1q<NP, NL>), grid, block, 0, st, reinterpret_cast<const int32_t *>(yres),
                                       dig, S.d_primes, S.d_lean, work, logm);
                else if (f.one)
                    hipLaunchKernelGGL((k_crt_lean1<NP, NL>), grid, block, 0, st, yres, dig, S.d_lean, work, logm);
                else if (f.p87) {
                    if constexpr (NP == 5 && NL == 3)
                        hipLaunchKernelGGL((k_crt_lean<5, 3, true>), grid, block, 0, st, yres, dig, S.d_lean, work, logm);
                } else
                    hipLaunchKernelGGL((k_crt_lean<NP, NL>), grid, block, 0, st, yres, dig, S.d_lean, work, logm);
            });
            break;
        case CrtKind::LeanRnd:
            with_nl(f.nl, [&](auto nl) {
                with_bool(f.rows, [&](auto rows) {
                    constexpr int NL = decltype(nl)::value;
                    constexpr bool ROWS = decltype(rows)::value;
                    if (f.quarter)
                        hipLaunchKernelGGL((k_crt_lean_rnd1<NP, NL, true, ROWS>), grid, block, 0, st, yres, dig, S.d_lean,
                                           work, logm, ra, iter, S.d_primes);
                    else if (f.one)
                        hipLaunchKernelGGL((k_crt_lean_rnd1<NP, NL, false, ROWS>), grid, block, 0, st, yres, dig, S.d_lean,
                                           work, logm, ra, iter, (const PrimeK *)nullptr);
                    else
                        with_bool(f.wide, [&](auto wide) {   // (k_crt_lean_rnd1 is never WIDE)
                            hipLaunchKernelGGL((k_crt_lean_rnd<NP, NL, decltype(wide)::value, ROWS>), grid, block, 0, st,
                                               yres, dig, S.d_lean, work, logm, ra, iter);
                        });
                });
            });
            break;
        }
        return SGFHE_OK;
    });
    if (rc) return rc;
    HIPCHK(c, hipGetLastError());
    return SGFHE_OK;
}
int32_t launch_crt(sgfhe_ctx *c, const sgfhe_ctx::Lane &L, uint32_t cnt, uint32_t mode, hipStream_t st,
                   RndArgs ra = RndArgs{}, uint32_t iter = 0, bool quarter = false, CrtForm *used = nullptr) {
    return launch_crt_raw(c, L.yres, L.dig, cnt * 2 * c->M, mode, st, ra, iter, quarter, used);
}

// ---- buffers ------------------------------------------------------------------------------------

size_t per_bootstrap_bytes(const sgfhe_ctx *c) {
    return (size_t)2 * c->M * sizeof(ulonglong2) + (size_t)2 * cur(c).npr * c->M * 4 + (size_t)c->n * 4;
}

// what the chunk policy (chunking.h) reads of the ctx, for calls at flatten mode `mode`
ChunkPolicy chunk_policy(const sgfhe_ctx *c, uint32_t mode) {
    return {c->chunk, default_chunk(c->lanes, per_bootstrap_bytes(c)), c->lanes, c->small_max, c->small_lanes,
            c->small_lanes_max, c->logm, fused_cap(c, mode)};
}

void free_lanes(sgfhe_ctx *c) {
    for (auto &L : c->lane) {
        if (L.dig) (void)hipFree(L.dig);
        if (L.yres) (void)hipFree(L.yres);
        if (L.ua) (void)hipFree(L.ua);
        if (L.zpart) (void)hipFree(L.zpart);
        L = sgfhe_ctx::Lane();
    }
    c->cap = 0;
}

int32_t ensure_work(sgfhe_ctx *c, uint32_t cpad) {
    if (cpad <= c->cap) return SGFHE_OK;
    int32_t rcd = drain(c);   // an earlier asynchronous call may still be using the buffers
    if (rcd) return rcd;
    free_lanes(c);
    for (auto &L : c->lane) {
        HIPCHK(c, hipMalloc(&L.dig, (size_t)cpad * 4 * c->M * sizeof(uint64_t)));
        HIPCHK(c, hipMalloc(&L.yres, (size_t)cpad * 2 * c->npr_max * c->M * 4));
        HIPCHK(c, hipMalloc(&L.ua, (size_t)cpad * c->n * 4));
        const uint32_t cs = cpad < c->small_max ? cpad : c->small_max;
        if (cs) HIPCHK(c, hipMalloc(&L.zpart, (size_t)cs * c->npr_max * 8 * c->M * 4));
    }
    c->cap = cpad;
    return SGFHE_OK;
}

// ---- timing events ------------------------------------------------------------------------------

void timing_flush(sgfhe_ctx *c) {
    // (the samples may sit on a caller's stream: wait for the events, not for the ctx stream)
    for (auto &t : c->ev) {
        float ms = 0;
        (void)hipEventSynchronize(t.e2);
        if (hipEventElapsedTime(&ms, t.e0, t.e1) == hipSuccess) { c->t_ext += ms; c->n_ext++; }
        if (hipEventElapsedTime(&ms, t.e1, t.e2) == hipSuccess) { c->t_crt += ms; c->n_crt++; }
        (void)hipEventDestroy(t.e0);
        (void)hipEventDestroy(t.e1);
        (void)hipEventDestroy(t.e2);
    }
    c->ev.clear();
    for (auto &t : c->ev_call) {
        float ms = 0;
        (void)hipEventSynchronize(t.e1);
        if (hipEventElapsedTime(&ms, t.e0, t.e1) == hipSuccess) { c->t_call += ms; c->n_call++; c->boots_call += t.batch; }
        (void)hipEventDestroy(t.e0);
        (void)hipEventDestroy(t.e1);
    }
    c->ev_call.clear();
}

// ---- the k-loop (fhe.jl:579-582) over one chunk, or over two chunks in a pipeline --------------------

// One chunk of the batch on its lane (work buffers + stream).
struct ChunkJob {
    const sgfhe_ctx::Lane *L;
    hipStream_t st;
    uint32_t cb, cpad;  // bootstraps in the chunk, padded to a multiple of 8
    size_t c0;          // index of its first bootstrap in the call
    RndArgs ra;
    bool sampled;       // HIP-event timing samples are taken on this chunk
};

// The forms one step took.
struct StepForms {
    ExtForm ext;
    CrtForm crt;
};
// Iteration k of one job on its stream: the external product with key slice `keyk` in the form ext_form chooses for
// the chunk, then the CRT that form hands its residues to.  `mid`: an event to record between the two (a timing
// sample), `used`: the forms the step took (sgfhe_debug_kloop_step reports them).
int32_t kloop_step(sgfhe_ctx *c, const ChunkJob &J, const int32_t *keyk, uint32_t k, uint32_t mode,
                   hipEvent_t mid = nullptr, StepForms *used = nullptr) {
    const ExtForm form = ext_form(c, mode, J.cb, J.cpad, J.L->zpart != nullptr);
    // (Round 4 also tried warming the next iteration's key slice from a second stream, one iteration
    // ahead, with k_fwd_phase's own workgroup -> XCD mapping: 18.06 / 19.01 / 20.85 ms against 17.94 /
    // 18.80 / 20.24 for 1 / 2 / 4 gates, no gain, profiles/r04_exp_prefetch.txt.)
    int32_t rc = launch_ext(c, *J.L, keyk, form, k, mode, J.st);
    if (rc) return rc;
    if (mid) HIPCHK(c, hipEventRecord(mid, J.st));
    if (used) used->ext = form;
    return launch_crt(c, *J.L, form.cnt, mode, J.st, J.ra, k + 1, form.quarter(), used ? &used->crt : nullptr);
}

// Iteration k of every job: kloop_step, each job on its
// own stream.  (Measured and rejected in round 2: chaining the two streams so that one chunk's
// CRT kernel runs beside the other chunk's external product -- also with the CRT as a
// one-workgroup-per-CU grid-stride "rider" kernel -- costs the external product as much time
// as the CRT takes alone)
int32_t run_iterations(sgfhe_ctx *c, ChunkJob *jobs, int njobs, uint64_t n_iters, uint32_t mode) {
    const size_t slice = (size_t)cur(c).npr * 8 * c->M;
    const int32_t *key = cur(c).d_key;
    for (uint64_t k = 0; k < n_iters; k++) {
        for (int j = 0; j < njobs; j++) {
            const ChunkJob &J = jobs[j];
            const bool sample = c->timing && J.sampled && (k % 64 == 1) && c->ev.size() < 2048;
            hipEvent_t e0 = nullptr, e1 = nullptr, e2 = nullptr;
            if (sample) {
                HIPCHK(c, hipEventCreate(&e0));
                HIPCHK(c, hipEventCreate(&e1));
                HIPCHK(c, hipEventCreate(&e2));
                HIPCHK(c, hipEventRecord(e0, J.st));
            }
            const int32_t rc = kloop_step(c, J, key + k * slice, (uint32_t)k, mode, e1);
            if (rc) return rc;
            if (sample) {
                HIPCHK(c, hipEventRecord(e2, J.st));
                c->ev.push_back({e0, e1, e2});
            }
        }
    }
    return SGFHE_OK;
}

// memcpy between the caller's pageable arrays and the page-locked mirrors.  The copies of the first
// chunk's inputs and of the last chunks' results are the part of a host-pointer call that no kernel
// hides: above 2 MB they are cut across up to four threads (one thread moves 5-8 GB/s).
// Called inside extern "C" entry points: nothing may throw out of it.  std::thread's constructor throws
// std::system_error when the process may not start another thread (EAGAIN: ulimit -u, a container's pid
// limit); the part that thread would have copied, and everything after it, is then copied here.
void host_copy(void *dst, const void *src, size_t bytes) {
    const size_t parts = bytes >= ((size_t)2 << 20) ? (bytes >= ((size_t)8 << 20) ? 4 : 2) : 1;
    if (parts == 1) { memcpy(dst, src, bytes); return; }
    const size_t step = ((bytes / parts) + 4095) & ~(size_t)4095;   // parts 1 .. of `step` bytes; the last takes the rest
    std::thread th[3];
    size_t nth = 0, off = step;
    for (; nth < parts - 1 && off < bytes; off += step) {
        const size_t len = (nth == parts - 2 || bytes - off < step) ? bytes - off : step;
        char *d = static_cast<char *>(dst) + off;
        const char *sr = static_cast<const char *>(src) + off;
        try {
            th[nth] = std::thread([d, sr, len] { memcpy(d, sr, len); });
            nth++;
        } catch (...) {            // no thread to be had: this part and the rest, on the caller's thread
            memcpy(d, sr, bytes - off);
            break;
        }
        if (len == bytes - off) break;
    }
    memcpy(dst, src, step < bytes ? step : bytes);
    for (size_t i = 0; i < nth; i++) th[i].join();
}

// [a1 | a2 | b1 | b2 | res]: the bootstrap inputs of `rows` rows (a: n words, b: one) carved out of `base`, and what
// follows them (the result rows, where the buffer holds them)
struct Staging {
    uint64_t *a1, *a2, *b1, *b2, *res;
    Staging from_row(size_t off, size_t n) const { return {a1 + off * n, a2 + off * n, b1 + off, b2 + off, res}; }
};
Staging staging(uint64_t *base, size_t rows, size_t n) {
    uint64_t *a2 = base + rows * n, *b1 = a2 + rows * n;
    return {base, a2, b1, b1 + rows, b1 + 2 * rows};
}

// The bootstrap inputs of a call or of a chunk as the kernels read them, on the device: a Staging's rows, or four
// arrays of the caller's.
struct BootRows {
    const uint64_t *a1 = nullptr, *a2 = nullptr, *b1 = nullptr, *b2 = nullptr;
    BootRows() = default;
    BootRows(const uint64_t *a1_, const uint64_t *a2_, const uint64_t *b1_, const uint64_t *b2_)
        : a1(a1_), a2(a2_), b1(b1_), b2(b2_) {}
    BootRows(const Staging &S) : a1(S.a1), a2(S.a2), b1(S.b1), b2(S.b2) {}
    BootRows from_row(size_t off, size_t n) const { return {a1 + off * n, a2 + off * n, b1 + off, b2 + off}; }
};

// Host buffers of sgfhe_bootstrap_batch, moved chunk by chunk beside the lanes' kernels (stream_io):
// a chunk's inputs go up while the chunks before it compute, its outputs come down while the chunks
// after it compute, and the CPU copies between the caller's (pageable) arrays and the page-locked
// mirrors happen while the device is busy.  What stays exposed is the first chunk's input (a few MB)
// and the last chunks' output.
struct HostPipe {
    const uint64_t *a1, *b1, *a2, *b2;   // the caller's arrays
    uint64_t *out;                        // the caller's result array
    uint64_t *d_in, *d_out;               // device staging: chunk at row c0 = words [c0 (2 n + 2) ...) laid out
                                          // [a1 rows | a2 rows | b1 | b2]; result rows as in `out`
    uint64_t *p_in, *p_out;               // page-locked mirrors of both, same layouts
    size_t out_row_words;                 // 3 (n + 1), twice that with SGFHE_FLAG_RAW_MODQ
    bool dbg;                             // SGFHE_DEBUG_IO is set (read once per call, bootstrap_host)
};

// One call's run of that pipeline (bootstrap_device): where the rows of every chunk lie on the device, the events of
// the copies, the results on their way to the caller's array, and the SGFHE_DEBUG_IO phase clock.  Without a HostPipe
// (rows and results are the caller's device arrays) every step does nothing.  The only place that knows the
// [a1 | a2 | b1 | b2] layout of the mirrors.
// A host-pointer call that is one group of chunks (a handful of gates up to two chunks' worth) has nothing to overlap
// its copies with: they go on the call's stream itself, in order with the kernels -- one upload before the first
// kernel, one download behind the last -- without the copy streams' events (`single`).
// (Round 4 also measured collecting the results only at the end, all results after the last kernel, and all inputs
// before the first kernel; this pipeline measured best, 1.003 x the device-resident call:
// profiles/r04_exp_io_variants.txt.)
struct PipeRun {
    sgfhe_ctx *const c;
    const HostPipe *const hp;
    const size_t batch, n;
    const bool single, dbg;
    size_t ev_next = 0;   // events of the host pipeline, from the ctx's pool
    struct OutJob { hipEvent_t done; size_t c0; uint32_t cb; };
    std::vector<OutJob> outq;   // result rows on their way to the page-locked mirror
    size_t out_drained = 0;
    double tw0 = 0.0, tw_first = 0.0, tw_wait = 0.0;   // SGFHE_DEBUG_IO=1: wall-clock phases of a pipelined call

    PipeRun(sgfhe_ctx *c_, const HostPipe *hp_, size_t batch_, size_t stride)
        : c(c_), hp(hp_), batch(batch_), n(c_->n), single(hp_ && batch_ <= stride), dbg(hp_ && hp_->dbg) {}

    // rows [c0, c0 + cb) of the caller's a1, a2, b1, b2 into the page-locked mirror, laid out
    // [a1 | a2 | b1 | b2] from word c0 (2 n + 2); returns where they start
    uint64_t *stage_in(size_t c0, size_t cb) const {
        uint64_t *pi = hp->p_in + c0 * (2 * n + 2);
        const Staging P = staging(pi, cb, n);
        host_copy(P.a1, hp->a1 + c0 * n, cb * n * 8);
        host_copy(P.a2, hp->a2 + c0 * n, cb * n * 8);
        memcpy(P.b1, hp->b1 + c0, cb * 8);
        memcpy(P.b2, hp->b2 + c0, cb * 8);
        return pi;
    }
    int32_t next_event(hipEvent_t *e) {
        if (ev_next == c->ev_pool.size()) {
            hipEvent_t ne = nullptr;
            HIPCHK(c, hipEventCreateWithFlags(&ne, hipEventDisableTiming));
            c->ev_pool.push_back(ne);
        }
        *e = c->ev_pool[ev_next++];
        return SGFHE_OK;
    }
    // a single-group call: all its rows up, on `st`
    int32_t upload_call(hipStream_t st) const {
        if (!single) return SGFHE_OK;
        stage_in(0, batch);
        HIPCHK(c, hipMemcpyAsync(hp->d_in, hp->p_in, batch * (2 * n + 2) * 8, hipMemcpyHostToDevice, st));
        return SGFHE_OK;
    }
    // R, the call's device rows, becomes the chunk's: rows J.c0 ... of the call's own arrays or of the whole-call
    // upload, or this chunk's inputs on their way caller's arrays -> page-locked mirror -> device on stream_io,
    // which the chunk's stream then waits for
    int32_t chunk_in(const ChunkJob &J, BootRows &R) {
        if (!hp) { R = R.from_row(J.c0, n); return SGFHE_OK; }
        if (single) { R = BootRows(staging(hp->d_in, batch, n)).from_row(J.c0, n); return SGFHE_OK; }
        if (dbg && J.c0 == 0) tw0 = wall_ms();
        const size_t cb = J.cb;
        uint64_t *pi = stage_in(J.c0, cb), *di = hp->d_in + J.c0 * (2 * n + 2);
        HIPCHK(c, hipMemcpyAsync(di, pi, cb * (2 * n + 2) * 8, hipMemcpyHostToDevice, c->stream_io));
        hipEvent_t ein;
        int32_t rc = next_event(&ein);
        if (rc) return rc;
        HIPCHK(c, hipEventRecord(ein, c->stream_io));
        HIPCHK(c, hipStreamWaitEvent(J.st, ein, 0));
        R = staging(di, cb, n);
        return SGFHE_OK;
    }
    void first_group_queued(size_t g0) {
        if (dbg && g0 == 0) tw_first = wall_ms();
    }
    // this chunk's results: device -> page-locked mirror on stream_io2, behind its last kernel
    // (a single-group call: one download behind the join, finish())
    int32_t chunk_out(const ChunkJob &J) {
        if (!hp || single) return SGFHE_OK;
        hipEvent_t ek, eo;
        int32_t rc;
        if ((rc = next_event(&ek)) || (rc = next_event(&eo))) return rc;
        HIPCHK(c, hipEventRecord(ek, J.st));
        HIPCHK(c, hipStreamWaitEvent(c->stream_io2, ek, 0));
        const size_t w0 = J.c0 * hp->out_row_words;
        HIPCHK(c, hipMemcpyAsync(hp->p_out + w0, hp->d_out + w0, (size_t)J.cb * hp->out_row_words * 8,
                                 hipMemcpyDeviceToHost, c->stream_io2));
        HIPCHK(c, hipEventRecord(eo, c->stream_io2));
        outq.push_back({eo, J.c0, J.cb});
        return SGFHE_OK;
    }
    // the first `upto` results queued: from the page-locked mirror into the caller's array
    int32_t drain_out(size_t upto) {
        for (; out_drained < upto; out_drained++) {
            const OutJob &o = outq[out_drained];
            HIPCHK(c, hipEventSynchronize(o.done));
            host_copy(hp->out + o.c0 * hp->out_row_words, hp->p_out + o.c0 * hp->out_row_words,
                      (size_t)o.cb * hp->out_row_words * 8);
        }
        return SGFHE_OK;
    }
    // with a group of `njobs` chunks queued, collect the results of the groups before it
    int32_t collect_earlier(int njobs) {
        if (!hp || single) return SGFHE_OK;
        const double t = dbg ? wall_ms() : 0.0;
        const int32_t rc = drain_out(outq.size() - (size_t)njobs);
        if (dbg) tw_wait += wall_ms() - t;
        return rc;
    }
    // behind the call's last work on `st`: the single-group download, or the results still on their way
    int32_t finish(hipStream_t st) {
        if (!hp) return SGFHE_OK;
        if (single) {
            HIPCHK(c, hipMemcpyAsync(hp->p_out, hp->d_out, batch * hp->out_row_words * 8, hipMemcpyDeviceToHost, st));
            HIPCHK(c, hipStreamSynchronize(st));
            c->pending = false;
            host_copy(hp->out, hp->p_out, batch * hp->out_row_words * 8);
            return SGFHE_OK;
        }
        const double t1 = dbg ? wall_ms() : 0.0;
        double t2 = 0.0;
        if (dbg && !outq.empty()) {   // the last chunks' kernels are done when their download may start
            (void)hipEventSynchronize(c->ev_done);
            t2 = wall_ms();
        }
        const int32_t rc = drain_out(outq.size());
        if (rc) return rc;
        if (dbg)
            fprintf(stderr, "[sgfhe io] pipelined call of %zu: first chunks staged and queued after %.2f ms, all queued after "
                    "%.2f ms (of which %.2f waiting for earlier results), last kernel done at %.2f, results in the "
                    "caller's array at %.2f\n", batch, tw_first - tw0, t1 - tw0, tw_wait, t2 - tw0, wall_ms() - tw0);
        return SGFHE_OK;
    }
};

// The LUT rows of a call (sgfhe_bootstrap_lut_batch): `rows` is a device array of one word per row of the call,
// LUT_ROW | truth table for a LUT row and 0 for a row of the classic path.  A LUT row starts at amplitude A0 (k_init)
// and leaves through k_final_lut; `all` says that every row is one, so that k_final has nothing to write.
// A LUT family call (sgfhe_bootstrap_lut_multi_batch) sets `tables`, the device array [row][n_tables] of every row's
// tables: every row is a LUT row, `out` is [row][n_tables][3][n + 1], and the rows leave through k_final_lut_multi.
// A level call whose LUT nodes lead live siblings (sgfhe_circuit_create_lut_multi) sets `wires` and the family CSR
// (kernels.h LutTables, with row0 the call's first row of its level): the leaders' rows leave as any LUT row, and
// k_final_lut_multi writes the siblings' wires from the same accumulators straight into the wire table -- per chunk,
// before the next chunk reuses the digits.
struct LutDesc {
    const uint32_t *rows;
    bool all;
    const uint8_t *tables = nullptr;
    uint32_t n_tables = 1;
    uint64_t *wires = nullptr;
    LutTables fam = {};
};

// One call of bootstrap_device.  A call site sets the fields it uses; the others keep what the constructor gives them.
struct BootCall {
    BootRows rows;                   // the inputs on the device (none with `pipe`, which brings them)
    size_t batch = 0;
    uint64_t *out = nullptr;         // device result rows [batch][3][n + 1], of 16-byte residues with SGFHE_FLAG_RAW_MODQ
    uint32_t flags = 0;
    uint64_t n_iters;                // iterations of the k-loop: the ctx's n, fewer for the debug entries
    hipStream_t st;                  // the stream the call is queued on: the ctx's own, or a caller's
    ulonglong2 *acc_out = nullptr;   // debug taps: the accumulators and the digits of every row after the k-loop
    uint64_t *dig_out = nullptr;
    const HostPipe *pipe = nullptr;  // a host-pointer call: inputs and results pipelined beside the kernels
    const LutDesc *lut = nullptr;    // a call with LUT rows
    explicit BootCall(const sgfhe_ctx *c) : n_iters(c->n), st(c->stream) {}
};

// The call number of the draw stream: this ctx's counter -- unless the call was numbered when it was handed
// to the coalescer, or is a gathered call, whose rows carry their own numbers: kernels.h RndRow.
uint32_t next_call_number(sgfhe_ctx *c) {
    if (!c->rnd || c->gather_rows) return 0u;
    if (c->call_fixed >= 0) {
        const uint32_t call = (uint32_t)c->call_fixed;
        c->call_fixed = -1;
        return call;
    }
    return c->rnd_call++;
}

// Chunk entry: accumulators, first digits and rotation amounts of the chunk from its rows R.
int32_t chunk_entry(sgfhe_ctx *c, const ChunkJob &J, const BootRows &R, const LutDesc *lut, uint32_t mode) {
    const uint32_t tot = J.cpad * c->M;
    const uint32_t *jlut = lut ? lut->rows + J.c0 : nullptr;
    with_bool(J.ra.rows != nullptr, [&](auto rows) {
        hipLaunchKernelGGL(k_init<decltype(rows)::value>, dim3((tot + 255) / 256), dim3(256), 0, J.st, R.a1, R.b1, R.a2,
                           R.b2, J.L->dig, J.L->ua, cur(c).d_crt, J.cb, J.cpad, c->n, (uint32_t)c->logm, mode, J.ra, jlut);
    });
    HIPCHK(c, hipGetLastError());
    return SGFHE_OK;
}

// Chunk exit: what leaves the chunk's accumulators behind the k-loop -- the debug taps, then the result rows
// through the kernel their kind takes (LutDesc).
int32_t chunk_exit(sgfhe_ctx *c, const ChunkJob &J, const BootCall &call, uint32_t mode) {
    const uint32_t n = c->n, M = c->M, logm = (uint32_t)c->logm;
    CrtConst *const d_crt = cur(c).d_crt;
    const dim3 block(256);
    if (call.acc_out) {
        const uint32_t t2 = J.cb * 2 * M;
        hipLaunchKernelGGL(k_dump_acc, dim3((t2 + 255) / 256), block, 0, J.st, J.L->dig, call.acc_out + J.c0 * 2 * M,
                           d_crt, t2, logm, mode);
        HIPCHK(c, hipGetLastError());
    }
    if (call.dig_out) {
        const uint32_t t2 = J.cb * 2 * M;
        hipLaunchKernelGGL(k_dump_digits, dim3((t2 + 255) / 256), block, 0, J.st, J.L->dig, call.dig_out + J.c0 * 4 * M,
                           t2, logm, mode);
        HIPCHK(c, hipGetLastError());
    }
    if (!call.out) return SGFHE_OK;
    const LutDesc *lut = call.lut;
    const bool raw = call.flags & SGFHE_FLAG_RAW_MODQ;
    const uint32_t t3 = J.cb * (n + 1), rawk = raw ? 1u : 0u;
    const dim3 grid((t3 + 255) / 256);
    const size_t row_words = (size_t)3 * (n + 1) * (raw ? 2 : 1);
    uint64_t *const out = call.out + J.c0 * row_words;   // the chunk's rows, one result each
    if (!lut || !lut->all)
        hipLaunchKernelGGL(k_final, grid, block, 0, J.st, J.L->dig, out, d_crt, J.cb, n, logm, rawk, mode);
    if (lut && lut->tables) {   // a family call: every table of every row of the chunk, n_tables results to a row
        LutTables T = {};
        T.tables = lut->tables + J.c0 * lut->n_tables;
        T.n_tables = lut->n_tables;
        hipLaunchKernelGGL(k_final_lut_multi<false>, grid, block, 0, J.st, J.L->dig,
                           call.out + J.c0 * lut->n_tables * row_words, d_crt, T, J.cb, n, logm, rawk, mode);
    } else if (lut && lut->wires) {   // the siblings of the chunk's LUT nodes, into the wire table
        LutTables T = lut->fam;
        T.row0 += (uint32_t)J.c0;
        hipLaunchKernelGGL(k_final_lut_multi<true>, grid, block, 0, J.st, J.L->dig, lut->wires, d_crt, T, J.cb, n, logm,
                           0u, mode);
    }
    if (lut && !lut->tables)   // the LUT rows of the chunk, over what k_final wrote for them
        hipLaunchKernelGGL(k_final_lut, grid, block, 0, J.st, J.L->dig, out, d_crt, lut->rows + J.c0, J.cb, n, logm, rawk,
                           mode);
    if (raw && (call.flags & SGFHE_FLAG_RAW_RNS2))  // residues leave as (v1, v2) pairs (rns.jl:16-18)
        hipLaunchKernelGGL(k_canon_to_rns2, dim3((3 * t3 + 255) / 256), block, 0, J.st,
                           reinterpret_cast<ulonglong2 *>(call.out) + J.c0 * 3 * (n + 1), (size_t)3 * t3, c->rns2);
    HIPCHK(c, hipGetLastError());
    return SGFHE_OK;
}

// Every bootstrap goes through here: `call.batch` gate bootstraps, cut into chunks across the lanes (chunking.h),
// queued on call.st.  Reads top to bottom as the stream operations of a call.
int32_t bootstrap_device(sgfhe_ctx *c, const BootCall &call) {
    if (!c->have_key) return fail(c, SGFHE_ERR_NO_KEY, "no bootstrap key uploaded");
    const size_t batch = call.batch;
    const hipStream_t st = call.st;
    const uint32_t mode = flatten_mode(c);
    const CallChunks cut = call_chunks(chunk_policy(c, mode), batch);
    if (call.flags & SGFHE_FLAG_RAW_RNS2) {
        if (!(call.flags & SGFHE_FLAG_RAW_MODQ))
            return fail(c, SGFHE_ERR_INVALID_ARG, "SGFHE_FLAG_RAW_RNS2 needs SGFHE_FLAG_RAW_MODQ");
        if (!c->have_rns2)
            return fail(c, SGFHE_ERR_INVALID_ARG, "SGFHE_FLAG_RAW_RNS2: no RNS2 moduli (upload the key with sgfhe_bkey_upload_rns2)");
    }
    const uint32_t callno = next_call_number(c);
    c->last_call = callno;
    int32_t rc;
    // work buffers for the largest chunk of this call, before anything of it is queued
    if ((rc = ensure_work(c, chunk_rows(cut, batch)))) return rc;
    c->last_chunk = chunk_rows(cut, batch);
    // after everything earlier calls queued on this ctx, whatever their streams
    if ((rc = fence_begin(c, st))) return rc;
    // From here on work is queued: should a later step fail, whatever has been queued still ends in
    // ev_done, so that the next call (or the destructor) waits for it before touching the buffers.
    struct QueuedWork {
        sgfhe_ctx *c;
        hipStream_t st;
        bool closed = false;
        ~QueuedWork() {
            if (closed) return;
            if (c->lanes == 2) {   // the second lane may hold part of it
                if (hipEventRecord(c->ev_join, c->stream2) == hipSuccess) (void)hipStreamWaitEvent(st, c->ev_join, 0);
            }
            if (hipEventRecord(c->ev_done, st) == hipSuccess) c->pending = true;
        }
    } queued{c, st};
    hipEvent_t ecall0 = nullptr, ecall1 = nullptr;
    if (c->timing && c->ev_call.size() < 256) {
        HIPCHK(c, hipEventCreate(&ecall0));
        HIPCHK(c, hipEventCreate(&ecall1));
        HIPCHK(c, hipEventRecord(ecall0, st));
    }
    PipeRun io(c, call.pipe, batch, cut.stride);
    if ((rc = io.upload_call(st))) return rc;
    if (cut.two_lanes) {  // fork: the second lane starts after everything already queued on st
        HIPCHK(c, hipEventRecord(c->ev_fork, st));
        HIPCHK(c, hipStreamWaitEvent(c->stream2, c->ev_fork, 0));
    }
    for (size_t g0 = 0; g0 < batch; g0 += cut.stride) {   // a group: one chunk per lane in use
        ChunkJob jobs[2];
        int njobs = 0;
        for (int li = 0; li < (cut.two_lanes ? 2 : 1); li++) {
            const size_t c0 = g0 + (size_t)li * cut.chunk;
            if (c0 >= batch) break;
            ChunkJob &J = jobs[njobs++];
            J.L = &c->lane[li];
            J.st = li ? c->stream2 : st;
            J.cb = (uint32_t)((batch - c0 < cut.chunk) ? batch - c0 : cut.chunk);
            J.cpad = round_up8(J.cb);
            J.c0 = c0;
            J.ra = RndArgs{c->rnd_key, callno, (uint32_t)c0, c->gather_rows};
            J.sampled = li == 0 && J.cpad == c->last_chunk;
            BootRows R = call.rows;
            if ((rc = io.chunk_in(J, R))) return rc;
            if ((rc = chunk_entry(c, J, R, call.lut, mode))) return rc;
        }
        io.first_group_queued(g0);
        if ((rc = run_iterations(c, jobs, njobs, call.n_iters, mode))) return rc;
        for (int j = 0; j < njobs; j++) {
            if ((rc = chunk_exit(c, jobs[j], call, mode))) return rc;
            if ((rc = io.chunk_out(jobs[j]))) return rc;
        }
        if ((rc = io.collect_earlier(njobs))) return rc;
    }
    if (cut.two_lanes) {  // join
        HIPCHK(c, hipEventRecord(c->ev_join, c->stream2));
        HIPCHK(c, hipStreamWaitEvent(st, c->ev_join, 0));
    }
    if (ecall0) {
        HIPCHK(c, hipEventRecord(ecall1, st));
        c->ev_call.push_back({ecall0, ecall1, (uint64_t)batch});
    }
    if ((rc = fence_end(c, st))) return rc;
    queued.closed = true;
    return io.finish(st);
}

// ---- constants -------------------------------------------------------------------------------------

// The arithmetic of every constant is csrc/constants.h (plan_bases, derive_basis, prime_tables); here they are
// allocated, uploaded and given their device pointers.

// The scheduling knobs of the environment (CtxKnobs), read once at ctx creation.
void read_env_knobs(sgfhe_ctx *c) {
    const char *env = getenv("SGFHE_HOST_PIN");
    c->use_pin = !(env && env[0] == '0');
    env = getenv("SGFHE_SMALL_PADDED");
    c->small_padded = env && env[0] == '1';
    env = getenv("SGFHE_SMALL_LANES");
    if (env) { c->small_lanes = atoi(env) != 0; if (atoi(env) > 1) c->small_lanes_max = (uint32_t)atoi(env); }
    env = getenv("SGFHE_CRT1_GATES");
    c->crt1_max = (uint32_t)(env ? atoi(env) : 8) * 2u * c->M;
    // m = 16384: the latency form ends at 16 gates (20 / 24 gates take 114 / 144 ms in it, 112 / 112 in the
    // throughput form; 12 / 14 gates 86 / 93 against 107; profiles/r04_exp_small_rings_lanes.txt)
    if (c->logm >= 14) { c->small_max = 16; if (c->small_lanes_max > 16) c->small_lanes_max = 16; }
    env = getenv("SGFHE_SMALL_SPLIT");
    if (env) c->split_max = (uint32_t)atoi(env);
    env = getenv("SGFHE_SMALL_FUSED");
    if (env) c->fused_min = (uint32_t)atoi(env);
}

// The twiddle tables of primes[tw_done .. npr) onto the device (a second, smaller basis shares the tables of the first).
int32_t upload_prime_tables(sgfhe_ctx *c, const uint32_t *primes, uint32_t npr) {
    const size_t M = c->M;
    PrimeTables T;
    for (uint32_t i = c->tw_done; i < npr; i++) {
        const Refusal r = prime_tables(primes[i], c->logm, &T);
        if (r) return fail(c, r.code, r.msg);
        HIPCHK(c, hipMemcpy(c->d_tw + 4 * i * M, T.tw.data(), 4 * M * sizeof(int32_t), hipMemcpyHostToDevice));
        if (!T.twq.empty())
            HIPCHK(c, hipMemcpy(c->d_twq + 4 * i * M, T.twq.data(), 4 * M * sizeof(int32_t), hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(c->d_pow + 2 * i * M, T.pw.data(), 2 * M * sizeof(int32_t), hipMemcpyHostToDevice));
        memcpy(c->tw_head[i], T.head, sizeof T.head);
        c->tw_done = i + 1;
    }
    return SGFHE_OK;
}

// One basis of the plan into S (its key comes later): constants and per-prime records, with the records' pointers
// into the tables on the device.
int32_t upload_basis(sgfhe_ctx *c, sgfhe_ctx::Basis &S, const BasisPlan &plan, int mode) {
    const size_t M = c->M;
    const uint32_t npr = plan.npr[mode];
    S.npr = npr;
    for (uint32_t i = 0; i < npr; i++) S.primes[i] = plan.primes[i];
    const int32_t rc = upload_prime_tables(c, S.primes, npr);
    if (rc) return rc;
    BasisConst K;
    derive_basis(c->logm, c->n, c->Q, c->B, ld128(c->par.DQ_tilde), S.primes, npr, plan.log_have[mode], plan.log_mbq, &K);
    memcpy(&S.h_crt, &K.crt, sizeof(CrtConst));     // (byte for byte, padding included: they go to the device)
    memcpy(&S.h_lean, &K.lean, sizeof(CrtLean));
    S.lean_rnd_ok = K.lean_rnd_ok;
    S.pack_G = K.pack_G;
    S.pack_G_rnd = K.pack_G_rnd;
    for (uint32_t i = 0; i < npr; i++) {
        PrimeK &P = K.pk[i];
        const int32_t *h = c->tw_head[i];
        P.twf = c->d_tw + 4 * i * M;
        P.twi = c->d_tw + (4 * i + 1) * M;
        P.f1 = h[0]; P.f2 = h[1]; P.f3 = h[2];
        P.fp2 = h[3]; P.fp3 = h[4];
        P.v1 = h[5]; P.v2 = h[6]; P.v3 = h[7];
        P.twq = c->d_twq + 4 * i * M;
        P.pw = c->d_pow + 2 * i * M;
    }
    HIPCHK(c, hipMalloc(&S.d_primes, npr * sizeof(PrimeK)));
    c->shared->own(S.d_primes);
    HIPCHK(c, hipMemcpy(S.d_primes, K.pk, npr * sizeof(PrimeK), hipMemcpyHostToDevice));
    HIPCHK(c, hipMalloc(&S.d_crt, sizeof(CrtConst)));
    c->shared->own(S.d_crt);
    HIPCHK(c, hipMemcpy(S.d_crt, &S.h_crt, sizeof(CrtConst), hipMemcpyHostToDevice));
    HIPCHK(c, hipMalloc(&S.d_lean, sizeof(CrtLean)));
    c->shared->own(S.d_lean);
    HIPCHK(c, hipMemcpy(S.d_lean, &S.h_lean, sizeof(CrtLean), hipMemcpyHostToDevice));
    return SGFHE_OK;
}

int32_t build_constants(sgfhe_ctx *c) {
    BasisPlan plan;
    const Refusal r = plan_bases(c->logm, c->Q, c->B, (c->create_flags & SGFHE_CTX_DETERMINISTIC_ONLY) != 0, &plan);
    if (r) return fail(c, r.code, r.msg);
    c->nb = plan.nb;
    c->rnd_ok = plan.rnd_ok;
    c->npr_max = plan.npr_max;
    read_env_knobs(c);
    HIPCHK(c, hipMalloc(&c->d_tw, (size_t)c->npr_max * 4 * c->M * sizeof(int32_t)));
    c->shared->own(c->d_tw);
    HIPCHK(c, hipMalloc(&c->d_twq, (size_t)c->npr_max * 4 * c->M * sizeof(int32_t)));
    c->shared->own(c->d_twq);
    HIPCHK(c, hipMalloc(&c->d_pow, (size_t)c->npr_max * 2 * c->M * sizeof(int32_t)));
    c->shared->own(c->d_pow);
    HIPCHK(c, hipMalloc(&c->d_bad, sizeof(uint32_t)));
    HIPCHK(c, hipMemset(c->d_bad, 0, sizeof(uint32_t)));
    // the larger basis first: its pass puts every prime's twiddle tables on the device
    for (int b = c->nb - 1; b >= 0; b--) {
        const int32_t rc = upload_basis(c, c->basis[b], plan, plan.mode_of(b));
        if (rc) return rc;
    }
    c->active = 0;
    return SGFHE_OK;
}

// Key uploads, generation and imports work on the LARGER basis (its key determines the other one): key_basis().
// key_begin makes it the active one for the writer's kernels; key_finish derives the smaller basis's key from it
// and goes back to the basis of the present mode.
// A key that clones share (sgfhe_ctx_clone) is read-only: their calls may be reading it on the device.
int32_t key_begin(sgfhe_ctx *c) {
    if (c->shared.use_count() > 1)
        return fail(c, SGFHE_ERR_INVALID_ARG,
                    "the bootstrap key of this ctx is shared with clones (sgfhe_ctx_clone): destroy them before replacing it");
    c->active = c->nb - 1;
    return SGFHE_OK;
}
sgfhe_ctx::Basis &key_basis(sgfhe_ctx *c) { return c->basis[c->nb - 1]; }
// A key writer calls this once its arguments are accepted, before the first byte of the key changes:
// from here to the end of key_finish the ctx has no key, so a writer that fails part-way (or whose second
// key form cannot be derived) leaves a ctx that refuses to bootstrap instead of one whose two bases hold
// different keys.
void key_dirty(sgfhe_ctx *c) { c->have_key = false; }
int32_t key_alloc(sgfhe_ctx *c, sgfhe_ctx::Basis &S) {
    if (S.d_key) return SGFHE_OK;
    S.key_bytes = (size_t)c->n * S.npr * 8 * c->M * 4;
    HIPCHK(c, hipMalloc(&S.d_key, S.key_bytes));
    c->shared->own(S.d_key);
    return SGFHE_OK;
}
// the smaller basis's key from the larger one's (a ctx with two bases), waited for
int32_t key_derive(sgfhe_ctx *c) {
    const sgfhe_ctx::Basis &Bg = c->basis[1];
    sgfhe_ctx::Basis &Sm = c->basis[0];
    const int32_t rc = key_alloc(c, Sm);
    if (rc) return rc;
    const KeyFactors fac = key_factors(Bg.primes, Sm.npr, Bg.npr);   // (the smaller basis is the first primes of the larger)
    const size_t total = Sm.key_bytes / 4;
    hipLaunchKernelGGL(k_key_derive, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, c->stream,
                       Bg.d_key, Sm.d_key, Sm.d_primes, fac, Bg.npr, Sm.npr, (uint32_t)c->logm, total);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SGFHE_OK;
}
int32_t key_finish(sgfhe_ctx *c, int32_t rc) {
    if (rc == SGFHE_OK && c->nb == 2 && (rc = key_derive(c))) c->have_key = false;
    c->active = mode_basis(c);
    return rc;
}

// Device-form key blob = 64-byte header + payload keyhat[k][prime][row * 2 + col][slot].  The
// header pins everything the payload's meaning depends on, so a blob made for another parameter
// set (or by another arithmetic revision of this library) is refused by the import.
struct KeyBlobHeader {
    char magic[8];         // "SGFHEKEY"
    uint32_t version;      // SGFHE_KEY_BLOB_VERSION: layout + residue form of the payload
    uint32_t n, m, npr;
    uint64_t Q[2];
    uint64_t B;
    uint64_t prime_hash;   // FNV-1a over the RNS primes in use
    uint64_t payload_bytes;
};
static_assert(sizeof(KeyBlobHeader) == 64, "key blob header is 64 bytes");
constexpr uint32_t SGFHE_KEY_BLOB_VERSION = 2;

// (of the larger basis: the blob is its key)
KeyBlobHeader blob_header(sgfhe_ctx *c) {
    const sgfhe_ctx::Basis &S = key_basis(c);
    KeyBlobHeader h;
    memset(&h, 0, sizeof h);
    memcpy(h.magic, "SGFHEKEY", 8);
    h.version = SGFHE_KEY_BLOB_VERSION;
    h.n = c->n;
    h.m = c->M;
    h.npr = S.npr;
    h.Q[0] = (uint64_t)c->Q;
    h.Q[1] = (uint64_t)(c->Q >> 64);
    h.B = (uint64_t)c->B;
    uint64_t f = 0xcbf29ce484222325ull;
    for (uint32_t i = 0; i < S.npr; i++)
        for (int b = 0; b < 4; b++) { f ^= (S.primes[i] >> (8 * b)) & 0xffu; f *= 0x100000001b3ull; }
    h.prime_hash = f;
    h.payload_bytes = (uint64_t)c->n * S.npr * 8 * c->M * 4;
    return h;
}

int32_t create_streams(sgfhe_ctx *c) {
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&c->stream2, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_done, hipEventDisableTiming) != hipSuccess ||
        hipStreamCreateWithFlags(&c->stream_io, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&c->stream_io2, hipStreamNonBlocking) != hipSuccess)
        return fail(c, SGFHE_ERR_HIP, "hipStreamCreate / hipEventCreate failed");
    return SGFHE_OK;
}

}  // namespace

// ==================================================================================================
// C ABI
// ==================================================================================================

extern "C" {

const char *sgfhe_version(void) { return "sgfhe_hip 0.5.0 gfx950"; }

uint32_t sgfhe_abi_version(void) { return SGFHE_ABI_VERSION; }

// The Makefile passes the hash of the kernel sources (and any extra -D flags of an ablation
// build); the marker prefix lets tools find the id in the file without loading it.
#ifndef SGFHE_BUILD_ID
#define SGFHE_BUILD_ID "unknown"
#endif
const char *sgfhe_build_id(void) {
    static const char id[] = "SGFHE_BUILD_ID=" SGFHE_BUILD_ID;
    return id + 15;
}

// The message of the last failed call on this ctx, copied for the calling thread (the ctx may be
// shared): valid until the same thread asks again.
const char *sgfhe_last_error_string(const sgfhe_ctx *ctx) {
    if (!ctx) return "null context";
    static thread_local std::string copy;
    SGFHE_LOCK(ctx);
    copy = ctx->err;
    return copy.c_str();
}

int32_t sgfhe_ctx_create(const sgfhe_params *p, int device, sgfhe_ctx **out) {
    return sgfhe_ctx_create_ex(p, device, 0u, out);
}

int32_t sgfhe_ctx_create_ex(const sgfhe_params *p, int device, uint32_t flags, sgfhe_ctx **out) {
    if (!p || !out) return SGFHE_ERR_INVALID_ARG;
    *out = nullptr;
    if (flags & ~(uint32_t)(SGFHE_CTX_RANDOM_FLATTEN | SGFHE_CTX_DETERMINISTIC_ONLY)) return SGFHE_ERR_INVALID_ARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev)
        return SGFHE_ERR_NO_DEVICE;
    if (hipSetDevice(device) != hipSuccess) return SGFHE_ERR_NO_DEVICE;
    sgfhe_ctx *c = new (std::nothrow) sgfhe_ctx();
    if (!c) return SGFHE_ERR_OOM;
    *out = c;  // returned even on failure so that the caller can read the error string
    c->par = *p;
    c->device = device;
    c->create_flags = flags;
    try {
        c->shared = std::make_shared<SharedDev>();
    } catch (...) {
        return fail(c, SGFHE_ERR_OOM, "out of host memory");
    }
    c->shared->device = device;
    {   // SGFHE_COALESCE=0 in the environment: ctxs sharing a key never gather their calls (A/B measurements)
        const char *env = getenv("SGFHE_COALESCE");
        if (env && env[0] == '0') c->shared->co.enabled = false;
    }
    const Refusal r = check_params(*p, &c->logm);
    if (r) return fail(c, r.code, r.msg);
    c->M = (uint32_t)p->m;
    c->n = (uint32_t)p->n;
    c->Q = ld128(p->Q);
    c->B = ld128(p->B);
    int32_t rc = create_streams(c);
    if (rc) return rc;
    return build_constants(c);
}

int32_t sgfhe_ctx_clone(sgfhe_ctx *src, sgfhe_ctx **out) {
    if (!src || !out) return SGFHE_ERR_INVALID_ARG;
    *out = nullptr;
    SGFHE_LOCK(src);
    if (!src->have_key) return fail(src, SGFHE_ERR_NO_KEY, "ctx_clone: the ctx has no bootstrap key to share");
    if (hipSetDevice(src->device) != hipSuccess) return fail(src, SGFHE_ERR_NO_DEVICE, "ctx_clone: hipSetDevice failed");
    sgfhe_ctx *c = new (std::nothrow) sgfhe_ctx();
    if (!c) return fail(src, SGFHE_ERR_OOM, "out of host memory");
    *out = c;  // returned even on failure so that the caller can read the error string (and destroys it)
    // the groups a clone takes over; its own -- flatten mode (deterministic, call counter 0: active = 0), lanes' work
    // buffers, streams, events, staging, timing, the error string and the lock -- starts as in a new ctx
    static_cast<CtxShared &>(*c) = *src;
    static_cast<CtxKnobs &>(*c) = *src;
    static_cast<CtxKeyState &>(*c) = *src;
    // The runtime deals streams onto its hardware queues (GPU_MAX_HW_QUEUES = 4) in the order they are created, and
    // packets of one hardware queue run in order: with four streams per ctx, the FIRST stream of every ctx -- the
    // one its calls run on -- would sit on the same queue and calls on different clones could never overlap on the
    // device (tools/ubench_streams.hip with UB_EXTRA_STREAMS=3: x1.00 at any number of threads,
    // profiles/r05_concurrent.txt).  A clone therefore shifts its streams by its number among the sharers: a few
    // throw-away streams first, destroyed once its own exist.  (What the gathering of small calls does not cover --
    // calls above its size limit, the asynchronous entry point -- then overlaps as far as the device lets two
    // chains overlap.)
    hipStream_t skip[3] = {nullptr, nullptr, nullptr};
    const unsigned shift = c->shared->clones.fetch_add(1) % 4u + 1u;       // 1, 2, 3, 0, 1, ... (the creator ctx has 0)
    for (unsigned i = 0; i < shift % 4u; i++) (void)hipStreamCreateWithFlags(&skip[i], hipStreamNonBlocking);
    int32_t rc = create_streams(c);
    for (hipStream_t x : skip)
        if (x) (void)hipStreamDestroy(x);
    if (rc) return rc;
    HIPCHK(c, hipMalloc(&c->d_bad, sizeof(uint32_t)));
    HIPCHK(c, hipMemset(c->d_bad, 0, sizeof(uint32_t)));
    return SGFHE_OK;
}

// the buffers of sgfhe_circuit_run[_ct] and of the packing path (the caller has waited for the ctx's work)
static void free_circuit_buffers(sgfhe_ctx *c) {
    c->circ_wires.release();
    c->circ_stage.release();
    c->circ_out.release();
    c->circ_tab.release();
    c->circ_data.release();
    c->circ_state.release();
    c->circ_ct.release();
    c->circ_raw.release();
    c->noise_tab.release();
    c->noise_lwe.release();
    c->pack_lwe.release();
    c->pack_raw.release();
    c->pack_pdig.release();
    c->pack_yg.release();
    c->pack_wv.release();
}
// ... and the staging of the host-pointer entry point
static void free_io_buffers(sgfhe_ctx *c) {
    c->io_in.release();
    c->io_out.release();
    c->pin_in.release();
    c->pin_out.release();
}

// DevBuf::grow for the circuit and pack paths: out of device memory is their caller's error to handle.  A buffer that
// grows is freed first, so the host waits for the ctx's queued work before it does, and only then, as ensure_work does
// (a device-resident run arrives here with earlier runs still in flight; behind run_drained there is nothing to wait for)
extern "C++" template <typename T>
static int32_t circ_grow(sgfhe_ctx *c, DevBuf<T> &buf, size_t words) {
    if (words <= buf.cap) return SGFHE_OK;
    if (const int32_t rc = drain(c)) return rc;
    if (buf.grow(words) == hipSuccess) return SGFHE_OK;
    return fail(c, SGFHE_ERR_OOM, "sgfhe_circuit_run: hipMalloc of " + std::to_string(words * sizeof(T)) +
                                      " bytes failed");
}

// A synchronous entry, after its checks: nothing of an earlier call is in flight when `queued` runs (it may regrow ctx
// buffers, then queues on the ctx stream and waits for it); should it fail, whatever it queued finishes before the
// buffers -- the ctx's, and the entry's own Scratch -- can be touched again.
extern "C++" template <class F>
static int32_t run_drained(sgfhe_ctx *c, F &&queued) {
    (void)hipSetDevice(c->device);
    int32_t rc = drain(c);
    if (rc) return rc;
    if ((rc = queued())) {
        (void)hipStreamSynchronize(c->stream);
        c->pending = false;
    }
    return rc;
}

// An asynchronous entry, after its checks: `queued` queues on `st` behind the ctx's earlier work and returns with its
// own work in flight (fence_begin ... fence_end are its own to place: it may regrow ctx buffers first).  Should it fail
// part way, the host waits for the earlier work and for whatever was queued on `st`, as run_drained does.
extern "C++" template <class F>
static int32_t run_queued(sgfhe_ctx *c, hipStream_t st, F &&queued) {
    (void)hipSetDevice(c->device);
    const int32_t rc = queued();
    if (rc) {
        if (c->pending) (void)hipEventSynchronize(c->ev_done);
        (void)hipStreamSynchronize(st);
        c->pending = false;
    }
    return rc;
}

// DevBuf::grow for call-local scratch (struct Scratch): a failed allocation is the HIP error of the entry
extern "C++" template <typename T>
static int32_t scratch_alloc(sgfhe_ctx *c, Scratch<T> &buf, size_t words) {
    const hipError_t e = buf.grow(words);
    return e == hipSuccess ? SGFHE_OK : fail(c, SGFHE_ERR_HIP, hipGetErrorString(e));
}

// canonical [npolys][m][2 words] in host memory -> NTT-domain key polys poly0.. in keyhat, through a staging buffer
// of at most 64 MiB, each stage waited for (rns2: the words are (v1, v2) limb pairs)
static int32_t key_transform_host(sgfhe_ctx *c, const uint64_t *canon, uint32_t npolys, int32_t *keyhat,
                                  const Rns2Const *rns2 = nullptr) {
    const size_t poly_bytes = (size_t)c->M * 16;
    uint32_t stage_polys = (uint32_t)(((size_t)64 << 20) / poly_bytes);
    if (stage_polys < 8) stage_polys = 8;
    if (stage_polys > npolys) stage_polys = npolys;
    Scratch<ulonglong2> stage;
    return run_drained(c, [&]() -> int32_t {
        int32_t rc = scratch_alloc(c, stage, (size_t)stage_polys * c->M);
        if (rc) return rc;
        for (uint32_t p0 = 0; p0 < npolys; p0 += stage_polys) {
            const uint32_t np = (npolys - p0 < stage_polys) ? npolys - p0 : stage_polys;
            HIPCHK(c, hipMemcpyAsync(stage.p, canon + (size_t)p0 * c->M * 2, (size_t)np * poly_bytes,
                                     hipMemcpyHostToDevice, c->stream));
            if (rns2) {  // (v1, v2) limb pairs -> canonical residues, in place (rns.jl:32-40)
                const size_t cnt = (size_t)np * c->M;
                hipLaunchKernelGGL(k_rns2_to_canon, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0,
                                   c->stream, stage.p, cnt, *rns2, cur(c).d_crt, c->d_bad);
            }
            if ((rc = launch_keytr(c, stage.p, keyhat, p0, np, c->stream))) return rc;
            HIPCHK(c, hipStreamSynchronize(c->stream));
        }
        return SGFHE_OK;
    });
}

int32_t sgfhe_ctx_destroy(sgfhe_ctx *c) {
    if (!c) return SGFHE_OK;
    (void)hipSetDevice(c->device);
    (void)drain(c);   // work of an asynchronous call on a caller's stream
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->stream2) (void)hipStreamSynchronize(c->stream2);
    if (c->stream_io) (void)hipStreamSynchronize(c->stream_io);
    if (c->stream_io2) (void)hipStreamSynchronize(c->stream_io2);
    timing_flush(c);
    free_lanes(c);
    for (hipEvent_t e : c->ev_pool) (void)hipEventDestroy(e);
    if (c->ev_done) (void)hipEventDestroy(c->ev_done);
    if (c->stream_io) (void)hipStreamDestroy(c->stream_io);
    if (c->stream_io2) (void)hipStreamDestroy(c->stream_io2);
    if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
    if (c->ev_join) (void)hipEventDestroy(c->ev_join);
    if (c->stream2) (void)hipStreamDestroy(c->stream2);
    if (c->shared) c->shared->co.forget(c);
    c->shared.reset();   // constants, tables and key: freed with the last ctx that shares them
    free_io_buffers(c);
    free_circuit_buffers(c);
    if (c->d_bad) (void)hipFree(c->d_bad);
    c->d_rows.release();
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
    return SGFHE_OK;
}

int32_t sgfhe_set_chunk(sgfhe_ctx *c, uint32_t chunk) {
    if (!c) return SGFHE_ERR_INVALID_ARG;
    SGFHE_LOCK(c);
    // the kernels index a chunk's planes with 32-bit byte offsets: residues [chunk][2][npr][m] x 4 B
    // and digit records [chunk][2] x 16 m B must stay below 4 GiB
    const uint64_t cap_y = 0xFFFFFFFFull / ((uint64_t)2 * c->npr_max * c->M * 4);
    const uint64_t cap_d = 0xFFFFFFFFull / ((uint64_t)2 * 16 * c->M);
    const uint64_t cap = (cap_y < cap_d ? cap_y : cap_d) & ~7ull;
    if (chunk > cap) return fail(c, SGFHE_ERR_INVALID_ARG, "chunk too large for this ring size");
    c->chunk = chunk ? round_up8(chunk) : 0;
    return SGFHE_OK;
}

static int32_t set_random_flatten(sgfhe_ctx *c, int enable, const ChaChaKey &key) {
    if (enable && !c->rnd_ok)
        return fail(c, SGFHE_ERR_UNSUPPORTED,
                    "randomised flatten: not available on this ctx (created with SGFHE_CTX_DETERMINISTIC_ONLY "
                    "where it needs a prime more, 20 m B Q beyond seven primes, or B^2 > 2^48 Q)");
    c->rnd = enable != 0;
    c->rnd_key = key;
    c->rnd_call = 0;
    c->active = mode_basis(c);   // constants and key form of the mode's basis (queued work keeps its own)
    return SGFHE_OK;
}

int32_t sgfhe_set_random_flatten(sgfhe_ctx *c, int enable, uint64_t seed) {
    if (!c) return SGFHE_ERR_INVALID_ARG;
    SGFHE_LOCK(c);
    ChaChaKey key = {};   // the seed as 32 little-endian bytes
    key.k[0] = (uint32_t)seed;
    key.k[1] = (uint32_t)(seed >> 32);
    return set_random_flatten(c, enable, key);
}

int32_t sgfhe_set_random_flatten_key(sgfhe_ctx *c, int enable, const uint8_t *key32) {
    if (!c || (enable && !key32)) return SGFHE_ERR_INVALID_ARG;
    SGFHE_LOCK(c);
    ChaChaKey key = {};
    if (key32)
        for (int i = 0; i < 8; i++)
            key.k[i] = (uint32_t)key32[4 * i] | ((uint32_t)key32[4 * i + 1] << 8) |
                       ((uint32_t)key32[4 * i + 2] << 16) | ((uint32_t)key32[4 * i + 3] << 24);
    return set_random_flatten(c, enable, key);
}

int32_t sgfhe_set_small_batch_max(sgfhe_ctx *c, uint32_t max_bootstraps) {
    if (!c) return SGFHE_ERR_INVALID_ARG;
    SGFHE_LOCK(c);
    if (max_bootstraps > 256)
        return fail(c, SGFHE_ERR_INVALID_ARG, "small-batch form: at most 256 bootstraps");
    (void)hipSetDevice(c->device);
    (void)drain(c);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->stream2) (void)hipStreamSynchronize(c->stream2);
    free_lanes(c);  // the staging buffer is sized from this value
    c->small_max = max_bootstraps;
    return SGFHE_OK;
}

int32_t sgfhe_set_lanes(sgfhe_ctx *c, uint32_t lanes) {
    if (!c || lanes < 1 || lanes > 2) return SGFHE_ERR_INVALID_ARG;
    SGFHE_LOCK(c);
    c->lanes = lanes;
    return SGFHE_OK;
}

// One key writer (sgfhe_bkey_upload, _upload_rns2, _generate, _import_device_form): the lock; key_begin, which refuses
// a key shared with clones and makes the larger basis the active one (the other basis's key is derived from it);
// nothing of the ctx in flight; `body`; key_finish.  The body checks EVERY argument first, then calls key_alloc and
// key_dirty, then writes: a call refused for its arguments leaves the previous key in place and usable, a call
// that fails after key_dirty a ctx that refuses to bootstrap (SGFHE_ERR_NO_KEY), and it sets have_key at its end.
extern "C++" template <class F>
static int32_t key_write(sgfhe_ctx *c, F &&body) {
    if (!c) return SGFHE_ERR_INVALID_ARG;
    SGFHE_LOCK(c);
    const int32_t rb = key_begin(c);
    if (rb) return rb;
    return key_finish(c, run_drained(c, body));
}

// the arguments are accepted: from here on the ctx has no key until the writer sets have_key
static int32_t key_open(sgfhe_ctx *c) {
    const int32_t rc = key_alloc(c, key_basis(c));
    if (rc == SGFHE_OK) key_dirty(c);
    return rc;
}

// sgfhe_bkey_upload and sgfhe_bkey_upload_rns2 once their arguments are accepted: [n][4][2][m] residues (rns2: limb
// pairs) into the key; a word out of range, found on the device, refuses the key with `bad_msg`
static int32_t key_upload(sgfhe_ctx *c, const uint64_t *words, const Rns2Const *rns2, const char *bad_msg) {
    HIPCHK(c, hipMemset(c->d_bad, 0, sizeof(uint32_t)));
    int32_t rc = key_open(c);
    if (rc) return rc;
    if ((rc = key_transform_host(c, words, c->n * 8, key_basis(c).d_key, rns2))) return rc;
    uint32_t bad = 0;
    HIPCHK(c, hipMemcpy(&bad, c->d_bad, sizeof bad, hipMemcpyDeviceToHost));
    if (bad) return fail(c, SGFHE_ERR_INVALID_ARG, bad_msg);   // (no key: key_dirty)
    c->have_key = true;
    return SGFHE_OK;
}

int32_t sgfhe_bkey_upload(sgfhe_ctx *c, const uint64_t *canonical, size_t n_words) {
    return key_write(c, [&]() -> int32_t {
        if (!canonical) return SGFHE_ERR_INVALID_ARG;
        if (n_words != (size_t)c->n * 8 * c->M * 2) return fail(c, SGFHE_ERR_INVALID_ARG, "bkey_upload: n_words != n*8*m*2");
        return key_upload(c, canonical, nullptr, "bkey_upload: a residue is not in [0, Q)");
    });
}

namespace {
struct KeygenScratch {   // the work buffers of sgfhe_bkey_generate
    Scratch<uint64_t> sk;
    Scratch<int32_t> shat, e;
    Scratch<uint32_t> y;
    Scratch<ulonglong2> acan, prod, canon;
};
}  // namespace

static int32_t keygen_queued(sgfhe_ctx *c, const uint64_t *sk, size_t n_sk, const uint8_t *seed32, uint32_t noise,
                             KeygenScratch &d) {
    if (!sk || !seed32) return SGFHE_ERR_INVALID_ARG;
    if (c->M < 8) return fail(c, SGFHE_ERR_UNSUPPORTED, "bkey_generate needs m >= 8");
    ChaChaKey ck;
    for (int i = 0; i < 8; i++)
        ck.k[i] = (uint32_t)seed32[4 * i] | ((uint32_t)seed32[4 * i + 1] << 8) |
                  ((uint32_t)seed32[4 * i + 2] << 16) | ((uint32_t)seed32[4 * i + 3] << 24);
    if (n_sk != c->n) return fail(c, SGFHE_ERR_INVALID_ARG, "bkey_generate: secret key must hold n bits");
    if (c->Q < ((u128)1 << 16)) return fail(c, SGFHE_ERR_UNSUPPORTED, "bkey_generate needs Q >= 2^16");
    // e in [-noise, noise] is formed in int32 and lifted as Q - |e| (k_keygen_draw / k_keygen_finish)
    if (noise >= (1u << 30) || (u128)noise * 2 >= c->Q)
        return fail(c, SGFHE_ERR_INVALID_ARG, "bkey_generate: noise must be below 2^30 and below Q / 2");
    int32_t rc = key_open(c);
    if (rc) return rc;
    const sgfhe_ctx::Basis &K = key_basis(c);   // (the active one: key_begin)
    const uint32_t M = c->M, rows = c->n * 4;
    uint32_t R = 64;  // rows per batch (16 key slices)
    if (R > rows) R = rows;
    if ((rc = scratch_alloc(c, d.sk, c->n))) return rc;
    if ((rc = scratch_alloc(c, d.shat, (size_t)K.npr * M))) return rc;
    if ((rc = scratch_alloc(c, d.y, (size_t)R * K.npr * M))) return rc;
    if ((rc = scratch_alloc(c, d.acan, (size_t)R * M))) return rc;
    if ((rc = scratch_alloc(c, d.prod, (size_t)R * M))) return rc;
    if ((rc = scratch_alloc(c, d.canon, (size_t)R * 2 * M))) return rc;
    if ((rc = scratch_alloc(c, d.e, (size_t)R * M))) return rc;
    HIPCHK(c, hipMemcpyAsync(d.sk.p, sk, (size_t)c->n * 8, hipMemcpyHostToDevice, c->stream));
    if ((rc = launch_keygen_ntt(c, d.sk.p, d.shat.p, nullptr, nullptr, 0, true, c->stream))) return rc;
    for (uint32_t row0 = 0; row0 < rows; row0 += R) {
        const uint32_t tot = R * M;
        hipLaunchKernelGGL(k_keygen_draw, dim3((tot / 4 + 255) / 256), dim3(256), 0, c->stream,
                           d.acan.p, d.e.p, K.d_crt, ck, noise, row0, R, (uint32_t)c->logm);
        if ((rc = launch_keygen_ntt(c, d.sk.p, d.shat.p, d.acan.p, d.y.p, R, false, c->stream))) return rc;
        // CRT of the exact product, canonical residues into d.prod ([row][m] 16-byte values)
        if ((rc = launch_crt_raw(c, d.y.p, reinterpret_cast<uint64_t *>(d.prod.p), tot, MODE_NOACC | MODE_CANON,
                                 c->stream, RndArgs{}, 0u)))
            return rc;
        hipLaunchKernelGGL(k_keygen_finish, dim3((tot + 255) / 256), dim3(256), 0, c->stream, d.acan.p,
                           d.prod.p, d.e.p, d.sk.p, d.canon.p, K.d_crt, row0, R, (uint32_t)c->logm);
        HIPCHK(c, hipGetLastError());
        if ((rc = launch_keytr(c, d.canon.p, K.d_key, row0 * 2, R * 2, c->stream))) return rc;
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->have_key = true;
    return SGFHE_OK;
}

int32_t sgfhe_bkey_generate(sgfhe_ctx *c, const uint64_t *sk, size_t n_sk, const uint8_t *seed32,
                            uint32_t noise) {
    KeygenScratch d;
    return key_write(c, [&] { return keygen_queued(c, sk, n_sk, seed32, noise, d); });
}

static int32_t rns2_configure(sgfhe_ctx *c, uint64_t m1, uint64_t m2) {
    const Refusal r = rns2_const(c->Q, m1, m2, &c->rns2);
    if (r) return fail(c, r.code, r.msg);
    c->have_rns2 = true;
    return SGFHE_OK;
}

int32_t sgfhe_bkey_upload_rns2(sgfhe_ctx *c, const uint64_t *pairs, size_t n_words, uint64_t m1,
                               uint64_t m2) {
    return key_write(c, [&]() -> int32_t {
        if (!pairs) return SGFHE_ERR_INVALID_ARG;
        if (n_words != (size_t)c->n * 8 * c->M * 2) return fail(c, SGFHE_ERR_INVALID_ARG, "bkey_upload_rns2: bad n_words");
        const int32_t rc = rns2_configure(c, m1, m2);
        if (rc) return rc;
        return key_upload(c, pairs, &c->rns2, "bkey_upload_rns2: a limb is not in [0, m_i)");
    });
}

int32_t sgfhe_rns2_convert(sgfhe_ctx *c, int to_pairs, const uint64_t *in, size_t count, uint64_t m1,
                           uint64_t m2, uint64_t *out) {
    if (!c || !in || !out) return SGFHE_ERR_INVALID_ARG;
    SGFHE_LOCK(c);
    if (count == 0) return SGFHE_OK;
    Scratch<ulonglong2> d;
    uint32_t bad = 0;
    const int32_t rc = run_drained(c, [&]() -> int32_t {
        int32_t r = rns2_configure(c, m1, m2);
        if (r) return r;
        if ((r = scratch_alloc(c, d, count))) return r;
        HIPCHK(c, hipMemsetAsync(c->d_bad, 0, sizeof(uint32_t), c->stream));
        HIPCHK(c, hipMemcpyAsync(d.p, in, count * 16, hipMemcpyHostToDevice, c->stream));
        const dim3 grid((unsigned)((count + 255) / 256));
        if (to_pairs)
            hipLaunchKernelGGL(k_canon_to_rns2, grid, dim3(256), 0, c->stream, d.p, count, c->rns2);
        else
            hipLaunchKernelGGL(k_rns2_to_canon, grid, dim3(256), 0, c->stream, d.p, count, c->rns2,
                               cur(c).d_crt, c->d_bad);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(out, d.p, count * 16, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(&bad, c->d_bad, sizeof bad, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return SGFHE_OK;
    });
    if (rc) return rc;
    // (after the device work, with `out` written: what a refused call leaves there is part of the interface)
    if (to_pairs) {  // canonical inputs must be below Q (checked on the host copy: debug hook)
        for (size_t i = 0; i < count; i++)
            if (ld128(in + 2 * i) >= c->Q) return fail(c, SGFHE_ERR_INVALID_ARG, "rns2_convert: value >= Q");
    } else if (bad) {
        return fail(c, SGFHE_ERR_INVALID_ARG, "rns2_convert: a limb is not in [0, m_i)");
    }
    return SGFHE_OK;
}

int32_t sgfhe_bkey_device_form_bytes(const sgfhe_ctx *c, size_t *bytes) {
    if (!c || !bytes) return SGFHE_ERR_INVALID_ARG;
    SGFHE_LOCK(c);
    *bytes = sizeof(KeyBlobHeader) + (size_t)c->n * c->npr_max * 8 * c->M * 4;   // the larger basis's key
    return SGFHE_OK;
}

int32_t sgfhe_bkey_export_device_form(sgfhe_ctx *c, void *dst) {
    if (!c || !dst) return SGFHE_ERR_INVALID_ARG;
    SGFHE_LOCK(c);
    if (!c->have_key) return fail(c, SGFHE_ERR_NO_KEY, "no bootstrap key uploaded");
    (void)hipSetDevice(c->device);
    SGFHE_QUIESCE(c);
    const sgfhe_ctx::Basis &K = key_basis(c);   // the blob is the key of the larger basis
    const KeyBlobHeader h = blob_header(c);
    HIPCHK(c, hipMemcpy(dst, &h, sizeof h, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpyAsync(static_cast<char *>(dst) + sizeof h, K.d_key, K.key_bytes,
                             hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SGFHE_OK;
}

int32_t sgfhe_bkey_import_device_form(sgfhe_ctx *c, const void *src) {
    return key_write(c, [&]() -> int32_t {
        if (!src) return SGFHE_ERR_INVALID_ARG;
        KeyBlobHeader got;
        HIPCHK(c, hipMemcpy(&got, src, sizeof got, hipMemcpyDeviceToHost));
        const KeyBlobHeader want = blob_header(c);
        if (memcmp(got.magic, want.magic, sizeof want.magic) != 0)
            return fail(c, SGFHE_ERR_INVALID_ARG, "bkey_import: not a device-form key blob (bad magic)");
        if (got.version != want.version)
            return fail(c, SGFHE_ERR_INVALID_ARG, "bkey_import: blob format version differs from this library");
        if (memcmp(&got, &want, sizeof want) != 0)
            return fail(c, SGFHE_ERR_INVALID_ARG,
                        "bkey_import: the blob belongs to another parameter set (n, m, Q, B or RNS primes differ)");
        const int32_t rc = key_open(c);
        if (rc) return rc;
        const sgfhe_ctx::Basis &K = key_basis(c);
        HIPCHK(c, hipMemcpyAsync(K.d_key, static_cast<const char *>(src) + sizeof got, K.key_bytes,
                                 hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        c->have_key = true;
        return SGFHE_OK;
    });
}

int32_t sgfhe_bootstrap_batch_device(sgfhe_ctx *c, const uint64_t *a1, const uint64_t *b1,
                                     const uint64_t *a2, const uint64_t *b2, size_t batch,
                                     uint64_t *out, uint32_t flags, void *stream) {
    if (!c || !a1 || !b1 || !a2 || !b2 || !out) return SGFHE_ERR_INVALID_ARG;
    SGFHE_LOCK(c);
    if (batch == 0) return SGFHE_OK;
    (void)hipSetDevice(c->device);
    // The call's work is queued on the caller's stream (or the ctx's own), behind everything earlier
    // calls queued on this ctx on any stream (fence_begin): calls on one ctx never overlap on the
    // device, so two threads or two streams may share it.
    BootCall call(c);
    call.rows = {a1, a2, b1, b2};
    call.batch = batch, call.out = out, call.flags = flags;
    if (stream) call.st = (hipStream_t)stream;
    return bootstrap_device(c, call);
}

int32_t sgfhe_sync(sgfhe_ctx *c) {
    if (!c) return SGFHE_ERR_INVALID_ARG;
    SGFHE_LOCK(c);
    (void)hipSetDevice(c->device);
    // all work queued on the ctx, whichever streams the calls named (every call ends in ev_done)
    int32_t rc = drain(c);
    if (rc) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SGFHE_OK;
}

static int32_t bootstrap_host(sgfhe_ctx *c, const uint64_t *a1, const uint64_t *b1,
                              const uint64_t *a2, const uint64_t *b2, size_t batch, uint64_t *out,
                              uint32_t flags, uint64_t n_iters, uint64_t *acc, uint64_t *digs = nullptr) {
    (void)hipSetDevice(c->device);
    const size_t n = c->n;
    const size_t out_row = 3 * (n + 1) * ((flags & SGFHE_FLAG_RAW_MODQ) ? 2 : 1);
    const size_t out_words = batch * out_row;
    const size_t acc_words = batch * 2 * (size_t)c->M * 2;
    uint64_t *d_in = nullptr, *d_out = nullptr;
    const size_t dig_words = batch * 4 * (size_t)c->M;
    const size_t in_words = 2 * batch * (n + 1);
    int32_t rc = drain(c);   // the staging buffers may be regrown: nothing of an earlier call may be in flight
    if (rc) return rc;
    HIPCHK(c, c->io_in.grow(in_words));
    if (out) HIPCHK(c, c->io_out.grow(out_words));
    d_in = c->io_in.p;
    if (out) d_out = c->io_out.p;
    const bool dbg = getenv("SGFHE_DEBUG_IO") != nullptr;   // wall-clock phases of the call on stderr
    // The production call (results only): page-locked mirrors of both staging buffers, grown on demand
    // and kept, and the copies pipelined chunk by chunk beside the kernels (HostPipe).  A failed
    // allocation, a buffer above PIN_MAX_BYTES, SGFHE_HOST_PIN=0 and the debug hooks take direct copies
    // of the caller's arrays.
    const size_t pin_max = pin_max_bytes();
    bool pipe = c->use_pin && out && !acc && !digs && in_words * 8 <= pin_max && out_words * 8 <= pin_max;
    auto pin_grow = [&](DevBuf<uint64_t, true> &buf, size_t words, const char *name) {
        if (!pipe || words <= buf.cap) return;
        const hipError_t pe = buf.grow(words);
        if (pe != hipSuccess) pipe = false;
        if (dbg) fprintf(stderr, "[sgfhe io] %s %zu bytes: %s\n", name, words * 8, hipGetErrorString(pe));
    };
    pin_grow(c->pin_in, in_words, "pin_in");
    pin_grow(c->pin_out, out_words, "pin_out");
    const double t0 = wall_ms();
    BootCall call(c);
    call.batch = batch, call.out = d_out, call.flags = flags, call.n_iters = n_iters;
    if (pipe) {
        const HostPipe hp = {a1, b1, a2, b2, out, d_in, d_out, c->pin_in.p, c->pin_out.p, out_row, dbg};
        call.pipe = &hp;
        rc = bootstrap_device(c, call);
        const hipError_t e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess && rc == SGFHE_OK) rc = fail(c, SGFHE_ERR_HIP, hipGetErrorString(e));
        if (rc == SGFHE_OK) c->pending = false;
        if (dbg) fprintf(stderr, "[sgfhe io] batch %zu pipelined: %.2f ms\n", batch, wall_ms() - t0);
        return rc;
    }
    Scratch<ulonglong2> d_acc;   // debug hooks only
    Scratch<uint64_t> d_dig;
    return run_drained(c, [&]() -> int32_t {
        uint64_t *d_a1 = d_in, *d_a2 = d_in + batch * n, *d_b1 = d_in + 2 * batch * n, *d_b2 = d_b1 + batch;
        const size_t a_bytes = batch * n * 8;
        int32_t rq;
        if (acc && (rq = scratch_alloc(c, d_acc, acc_words / 2))) return rq;
        if (digs && (rq = scratch_alloc(c, d_dig, dig_words))) return rq;
        HIPCHK(c, hipMemcpyAsync(d_a1, a1, a_bytes, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(d_a2, a2, a_bytes, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(d_b1, b1, batch * 8, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(d_b2, b2, batch * 8, hipMemcpyHostToDevice, c->stream));
        const double t1 = wall_ms();
        call.rows = {d_a1, d_a2, d_b1, d_b2};
        call.acc_out = d_acc.p, call.dig_out = d_dig.p;
        if ((rq = bootstrap_device(c, call))) return rq;
        const double t2 = wall_ms();
        if (digs) HIPCHK(c, hipMemcpyAsync(digs, d_dig.p, dig_words * 8, hipMemcpyDeviceToHost, c->stream));
        if (out) HIPCHK(c, hipMemcpyAsync(out, d_out, out_words * 8, hipMemcpyDeviceToHost, c->stream));
        if (acc) HIPCHK(c, hipMemcpyAsync(acc, d_acc.p, acc_words * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        c->pending = false;
        if (dbg)
            fprintf(stderr, "[sgfhe io] batch %zu direct copies: copy-in %.2f ms, enqueue %.2f, wait + copy-out %.2f\n",
                    batch, t1 - t0, t2 - t1, wall_ms() - t2);
        return SGFHE_OK;
    });
}

// One request through the coalescer of the ctxs that share this key (csrc/coalescer.h).
static int32_t coalesced_call(sgfhe_ctx *c, const uint64_t *a1, const uint64_t *b1, const uint64_t *a2,
                              const uint64_t *b2, size_t batch, uint64_t *out, uint32_t flags) {
    Coalescer &co = c->shared->co;
    Coalescer::Req me;
    me.owner = c;
    me.a1 = a1; me.b1 = b1; me.a2 = a2; me.b2 = b2;
    me.batch = batch; me.out = out; me.flags = flags;
    if (c->rnd) {               // its draw stream: this ctx's key, and the number this call has on this ctx
        me.rnd = true;
        memcpy(me.key, c->rnd_key.k, sizeof me.key);
        me.call = c->rnd_call++;
        c->last_call = me.call;
    }
    if (flags & SGFHE_FLAG_RAW_RNS2) {      // limb pairs leave by this ctx's moduli: only its like share its round
        me.have_rns2 = c->have_rns2;
        if (c->have_rns2) { me.m1 = c->rns2.m1; me.m2 = c->rns2.m2; }
    }
    std::vector<Coalescer::Req *> take;
    size_t gates = 0, gates_cap = 0;
    const int lead = co.arrive(me, take, gates, &gates_cap);
    if (lead < 0) return fail(c, SGFHE_ERR_OOM, "out of host memory");
    if (lead == 0) {                                // a leader ran it
        if (me.rc) c->err = me.err;
        return me.rc;
    }
    // the combined call, on this ctx (the caller holds its lock)
    int32_t rc;
    const size_t n = c->n;
    const size_t row = 3 * (n + 1) * ((flags & SGFHE_FLAG_RAW_MODQ) ? 2 : 1);
    if (take.size() == 1) {
        if (me.rnd) c->call_fixed = me.call;            // (numbered above)
        rc = bootstrap_host(c, a1, b1, a2, b2, batch, out, flags, c->n, nullptr);
        c->call_fixed = -1;
    } else {
        // (the staging vectors may throw: no exception leaves an entry point of the C ABI)
        auto gathered = [&]() -> int32_t {
            int32_t r = SGFHE_OK;
            if (me.rnd) {   // the draw stream of every row of the combined call, on the device before its first kernel
                (void)hipSetDevice(c->device);
                if ((r = drain(c))) return r;
                // (the kernels draw for the rows that pad a chunk to a multiple of 8 as well: Coalescer::rows_len)
                const size_t nrows = Coalescer::rows_len(gates);
                if (nrows > c->d_rows.cap &&   // (for the largest round the coalescer may gather, at once)
                    c->d_rows.grow(Coalescer::rows_len(gates > gates_cap ? gates : gates_cap)) != hipSuccess)
                    return fail(c, SGFHE_ERR_OOM, "hipMalloc of the gathered call's draw-stream table failed");
                c->h_rows.clear();
                for (const Coalescer::Req *q : take)
                    for (size_t t = 0; t < q->batch; t++) {
                        RndRow row_of;
                        memcpy(row_of.key.k, q->key, sizeof row_of.key.k);
                        row_of.call = q->call;
                        row_of.boot = (uint32_t)t;
                        c->h_rows.push_back(row_of);
                    }
                c->h_rows.resize(nrows, RndRow{});      // the padded rows: zeros, not what an earlier round left
                if (hipMemcpy(c->d_rows.p, c->h_rows.data(), nrows * sizeof(RndRow), hipMemcpyHostToDevice) != hipSuccess)
                    return fail(c, SGFHE_ERR_HIP, "copy of the gathered call's draw-stream table failed");
                c->gather_rows = c->d_rows.p;
            }
            std::vector<uint64_t> &g = c->co_buf;                          // [a1 | a2 | b1 | b2 | out] of all requests
            g.resize(gates * (2 * n + 2 + row));
            uint64_t *ga1 = g.data(), *ga2 = ga1 + gates * n, *gb1 = ga2 + gates * n, *gb2 = gb1 + gates, *gout = gb2 + gates;
            size_t r0 = 0;
            for (const Coalescer::Req *q : take) {
                memcpy(ga1 + r0 * n, q->a1, q->batch * n * 8);
                memcpy(ga2 + r0 * n, q->a2, q->batch * n * 8);
                memcpy(gb1 + r0, q->b1, q->batch * 8);
                memcpy(gb2 + r0, q->b2, q->batch * 8);
                r0 += q->batch;
            }
            if ((r = bootstrap_host(c, ga1, gb1, ga2, gb2, gates, gout, flags, c->n, nullptr))) return r;
            r0 = 0;
            for (const Coalescer::Req *q : take) {
                memcpy(q->out, gout + r0 * row, q->batch * row * 8);
                r0 += q->batch;
            }
            return SGFHE_OK;
        };
        try {
            rc = gathered();
        } catch (...) {
            rc = fail(c, SGFHE_ERR_OOM, "out of host memory");
        }
        c->gather_rows = nullptr;
    }
    co.finish(take, gates, rc, c->err);
    return rc;
}

int32_t sgfhe_bootstrap_batch(sgfhe_ctx *c, const uint64_t *a1, const uint64_t *b1,
                              const uint64_t *a2, const uint64_t *b2, size_t batch, uint64_t *out,
                              uint32_t flags) {
    if (!c || !a1 || !b1 || !a2 || !b2 || !out) return SGFHE_ERR_INVALID_ARG;
    SGFHE_LOCK(c);
    if (batch == 0) return SGFHE_OK;
    // small calls on a key that other ctxs share: gathered with whatever the other callers bring (Coalescer)
    if (c->shared.use_count() > 1 && c->have_key && c->shared->co.wants(batch))
        return coalesced_call(c, a1, b1, a2, b2, batch, out, flags);
    return bootstrap_host(c, a1, b1, a2, b2, batch, out, flags, c->n, nullptr);
}

int32_t sgfhe_set_coalesce(sgfhe_ctx *c, int enable, uint32_t req_max, uint32_t gates_max, uint32_t window_us) {
    if (!c) return SGFHE_ERR_INVALID_ARG;
    SGFHE_LOCK(c);
    if (enable && (req_max == 0 || gates_max < req_max || gates_max > 4096 || window_us > 100000))
        return fail(c, SGFHE_ERR_INVALID_ARG, "set_coalesce: 1 <= req_max <= gates_max <= 4096, window at most 100 ms");
    Coalescer &co = c->shared->co;
    std::lock_guard<std::mutex> lk(co.mu);
    co.enabled = enable != 0;
    if (enable) { co.req_max = req_max; co.gates_max = gates_max; co.window_us = window_us; }
    return SGFHE_OK;
}

int32_t sgfhe_coalesce_stats(sgfhe_ctx *c, uint64_t *stats, int reset) {
    if (!c || !stats) return SGFHE_ERR_INVALID_ARG;
    SGFHE_LOCK(c);
    Coalescer &co = c->shared->co;
    std::lock_guard<std::mutex> lk(co.mu);
    stats[0] = co.n_calls; stats[1] = co.n_reqs; stats[2] = co.n_gates; stats[3] = co.max_reqs;
    if (reset) co.n_calls = co.n_reqs = co.n_gates = co.max_reqs = 0;
    return SGFHE_OK;
}

int32_t sgfhe_debug_accumulators(sgfhe_ctx *c, const uint64_t *a1, const uint64_t *b1,
                                 const uint64_t *a2, const uint64_t *b2, size_t batch,
                                 uint64_t n_iters, uint64_t *acc) {
    if (!c || !a1 || !b1 || !a2 || !b2 || !acc) return SGFHE_ERR_INVALID_ARG;
    SGFHE_LOCK(c);
    if (n_iters > c->n) return fail(c, SGFHE_ERR_INVALID_ARG, "n_iters > n");
    if (batch == 0) return SGFHE_OK;
    return bootstrap_host(c, a1, b1, a2, b2, batch, nullptr, 0, n_iters, acc);
}

int32_t sgfhe_debug_digits(sgfhe_ctx *c, const uint64_t *a1, const uint64_t *b1, const uint64_t *a2,
                           const uint64_t *b2, size_t batch, uint64_t n_iters, uint64_t *digits) {
    if (!c || !a1 || !b1 || !a2 || !b2 || !digits) return SGFHE_ERR_INVALID_ARG;
    SGFHE_LOCK(c);
    if (n_iters > c->n) return fail(c, SGFHE_ERR_INVALID_ARG, "n_iters > n");
    if (batch == 0) return SGFHE_OK;
    return bootstrap_host(c, a1, b1, a2, b2, batch, nullptr, 0, n_iters, nullptr, digits);
}

int32_t sgfhe_debug_flatten(sgfhe_ctx *c, const uint64_t *values, uint64_t *digits) {
    if (!c || !values || !digits) return SGFHE_ERR_INVALID_ARG;
    SGFHE_LOCK(c);
    const uint32_t M = c->M;
    for (uint32_t i = 0; i < 2 * M; i++)
        if (ld128(values + 2 * (size_t)i) >= c->Q)
            return fail(c, SGFHE_ERR_INVALID_ARG, "debug_flatten: a value is not in [0, Q)");
    Scratch<ulonglong2> d_in;
    Scratch<uint64_t> d_out;
    return run_drained(c, [&]() -> int32_t {
        int32_t rc = ensure_work(c, 8);
        if (rc) return rc;
        const sgfhe_ctx::Lane &L = c->lane[0];
        if ((rc = scratch_alloc(c, d_in, (size_t)2 * M))) return rc;
        if ((rc = scratch_alloc(c, d_out, (size_t)4 * M))) return rc;
        HIPCHK(c, hipMemcpyAsync(d_in.p, values, (size_t)2 * M * 16, hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(k_flatten_canon, dim3((2 * M + 255) / 256), dim3(256), 0, c->stream, d_in.p,
                           L.dig, cur(c).d_crt, 2 * M, (uint32_t)c->logm);
        hipLaunchKernelGGL(k_dump_digits, dim3((2 * M + 255) / 256), dim3(256), 0, c->stream, L.dig,
                           d_out.p, 2 * M, (uint32_t)c->logm, 0u);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(digits, d_out.p, (size_t)4 * M * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return SGFHE_OK;
    });
}

// sgfhe_external_product and sgfhe_debug_cmux: one key slice [4][2][m] transformed into scratch, lane 0's digits
// zeroed, (a | b) uploaded and flattened into them; then `middle(L, slice, ab, &src)`, the entry's own launches on
// the ctx stream, which names the two polynomials [2][m] of 16-byte residues that go back as a_res and b_res.
extern "C++" template <class F>
static int32_t one_slice(sgfhe_ctx *c, const uint64_t *a, const uint64_t *b, const uint64_t *slice, uint64_t *a_res,
                         uint64_t *b_res, F &&middle) {
    Scratch<int32_t> d_slice;
    Scratch<ulonglong2> d_ab;
    return run_drained(c, [&]() -> int32_t {
        const uint32_t M = c->M, cpad = 8;
        int32_t rc = ensure_work(c, cpad);
        if (rc) return rc;
        const sgfhe_ctx::Lane &L = c->lane[0];
        if ((rc = scratch_alloc(c, d_slice, (size_t)cur(c).npr * 8 * M))) return rc;
        if ((rc = scratch_alloc(c, d_ab, (size_t)2 * M))) return rc;
        if ((rc = key_transform_host(c, slice, 8, d_slice.p))) return rc;
        HIPCHK(c, hipMemsetAsync(L.dig, 0, (size_t)cpad * 2 * M * 16, c->stream));
        HIPCHK(c, hipMemcpyAsync(d_ab.p, a, (size_t)M * 16, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(d_ab.p + M, b, (size_t)M * 16, hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(k_flatten_canon, dim3((2 * M + 255) / 256), dim3(256), 0, c->stream, d_ab.p,
                           L.dig, cur(c).d_crt, 2 * M, (uint32_t)c->logm);
        const ulonglong2 *src = nullptr;
        if ((rc = middle(L, d_slice.p, d_ab.p, &src))) return rc;
        HIPCHK(c, hipMemcpyAsync(a_res, src, (size_t)M * 16, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(b_res, src + M, (size_t)M * 16, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return SGFHE_OK;
    });
}

int32_t sgfhe_external_product(sgfhe_ctx *c, const uint64_t *a, const uint64_t *b,
                               const uint64_t *A, uint64_t *a_res, uint64_t *b_res) {
    if (!c || !a || !b || !A || !a_res || !b_res) return SGFHE_ERR_INVALID_ARG;
    SGFHE_LOCK(c);
    // A[4][2][m] is exactly one key slice (k = 0)
    return one_slice(c, a, b, A, a_res, b_res,
                     [&](const sgfhe_ctx::Lane &L, const int32_t *d_A, ulonglong2 *, const ulonglong2 **src) -> int32_t {
        int32_t rc = launch_extprod(c, L, d_A, 8, 0, MODE_PLAIN, c->stream);
        if (rc) return rc;
        *src = reinterpret_cast<const ulonglong2 *>(L.dig);     // canonical residues, in place of the digits
        return launch_crt(c, L, 8, MODE_NOACC | MODE_CANON, c->stream);
    });
}

int32_t sgfhe_debug_cmux(sgfhe_ctx *c, const uint64_t *a, const uint64_t *b, const uint64_t *C,
                         uint64_t j, uint64_t *a_res, uint64_t *b_res) {
    if (!c || !a || !b || !C || !a_res || !b_res) return SGFHE_ERR_INVALID_ARG;
    SGFHE_LOCK(c);
    if (j >= 2 * (uint64_t)c->M) return fail(c, SGFHE_ERR_INVALID_ARG, "debug_cmux: j must be in [0, 2 m)");
    const uint32_t jw = (uint32_t)j;
    // C[4][2][m] is one key slice
    return one_slice(c, a, b, C, a_res, b_res,
                     [&](const sgfhe_ctx::Lane &L, const int32_t *d_C, ulonglong2 *d_ab, const ulonglong2 **src) -> int32_t {
        const uint32_t M = c->M;
        HIPCHK(c, hipMemsetAsync(L.ua, 0, (size_t)8 * c->n * 4, c->stream));
        HIPCHK(c, hipMemcpyAsync(L.ua, &jw, 4, hipMemcpyHostToDevice, c->stream));  // u.a[0] of bootstrap 0
        int32_t rc = launch_extprod(c, L, d_C, 8, 0, 0u, c->stream);     // iteration k = 0, with the rotation
        if (rc) return rc;
        if ((rc = launch_crt(c, L, 8, 0u, c->stream))) return rc;        // acc <- acc + D, flattened again
        hipLaunchKernelGGL(k_dump_acc, dim3((2 * M + 255) / 256), dim3(256), 0, c->stream, L.dig, d_ab,
                           cur(c).d_crt, 2 * M, (uint32_t)c->logm, 0u);
        HIPCHK(c, hipGetLastError());
        *src = d_ab;
        return SGFHE_OK;
    });
}

// What a flatten of the ctx's present mode can store as the digit pair (e_lo, e_hi) of one coefficient: x mod B and
// x div B of an x < Q, each plus a draw in [0, 2 xmax] in the randomised mode.
static bool storable_digits(const sgfhe_ctx *c, uint64_t e_lo, uint64_t e_hi) {
    const u128 draw = c->rnd ? 2 * (3 * (c->B / 2)) : 0;
    if (e_lo > c->B - 1 + draw || e_hi > (c->Q - 1) / c->B + draw) return false;
    return c->rnd || e_lo + e_hi * c->B < c->Q;
}

// The chunk the chosen-operand hooks work on (sgfhe_debug_kloop_step, sgfhe_debug_chunk_entry, sgfhe_debug_chunk_exit):
// `cb` rows from row 0 of a call numbered `callno`, on lane 0 and the ctx stream, as bootstrap_device makes the first
// chunk of a call that fits one chunk.
static ChunkJob debug_chunk_job(sgfhe_ctx *c, uint32_t cb, uint32_t callno) {
    ChunkJob J;
    J.L = &c->lane[0];
    J.st = c->stream;
    J.cb = cb;
    J.cpad = round_up8(cb);
    J.c0 = 0;
    J.ra = RndArgs{c->rnd_key, callno, 0u, c->gather_rows};
    J.sampled = false;
    return J;
}

// a per-row LUT descriptor of the hooks: every word 0 (a row of the classic path) or LUT_ROW | truth table
static bool lut_words_ok(const uint32_t *lut, size_t rows) {
    for (size_t b = 0; b < rows; b++)
        if (lut[b] != 0 && (lut[b] & ~0xFFu) != LUT_ROW) return false;
    return true;
}

int32_t sgfhe_debug_kloop_step(sgfhe_ctx *c, const uint64_t *digits, const uint64_t *C, const uint32_t *j, size_t gates,
                               uint32_t k, uint64_t *digits_out, char *ext_name, size_t ext_cap, char *crt_name,
                               size_t crt_cap) {
    if (!c || !digits || !C || !j || !digits_out || !ext_name || !crt_name || !ext_cap || !crt_cap)
        return SGFHE_ERR_INVALID_ARG;
    SGFHE_LOCK(c);
    const uint32_t mode = flatten_mode(c), M = c->M, n = c->n;
    if (gates == 0 || gates > base_chunk(chunk_policy(c, mode)))
        return fail(c, SGFHE_ERR_INVALID_ARG, "debug_kloop_step: between 1 gate and one chunk of the ctx");
    if (k >= n) return fail(c, SGFHE_ERR_INVALID_ARG, "debug_kloop_step: k must be in [0, n)");
    for (size_t b = 0; b < gates; b++)
        if (j[b] >= 2 * M) return fail(c, SGFHE_ERR_INVALID_ARG, "debug_kloop_step: j must be in [0, 2 m)");
    for (size_t bc = 0; bc < gates * 2; bc++)
        for (uint32_t i = 0; i < M; i++)
            if (!storable_digits(c, digits[bc * 2 * M + i], digits[(bc * 2 + 1) * M + i]))
                return fail(c, SGFHE_ERR_INVALID_ARG, "debug_kloop_step: a digit pair no flatten of this mode stores");
    for (uint32_t i = 0; i < 8 * M; i++)
        if (ld128(C + 2 * (size_t)i) >= c->Q)
            return fail(c, SGFHE_ERR_INVALID_ARG, "debug_kloop_step: a key residue is not in [0, Q)");
    const uint32_t cb = (uint32_t)gates, cpad = round_up8(cb), t2 = cb * 2 * M;
    Scratch<int32_t> d_slice;
    Scratch<uint64_t> d_io;
    StepForms used;
    std::vector<uint32_t> ua((size_t)cb * n, 0u);   // ua[b * n + k] = j[b]
    for (uint32_t b = 0; b < cb; b++) ua[(size_t)b * n + k] = j[b];
    int32_t rc = run_drained(c, [&]() -> int32_t {
        int32_t rc = ensure_work(c, cpad);
        if (rc) return rc;
        const sgfhe_ctx::Lane &L = c->lane[0];
        if ((rc = scratch_alloc(c, d_slice, (size_t)cur(c).npr * 8 * M))) return rc;
        if ((rc = scratch_alloc(c, d_io, (size_t)cb * 4 * M))) return rc;
        if ((rc = key_transform_host(c, C, 8, d_slice.p))) return rc;
        // one chunk as chunk_entry leaves it: the gates' digit records (the padding rows zero), u.a[k] of every gate
        HIPCHK(c, hipMemsetAsync(L.dig, 0, (size_t)cpad * 2 * M * 16, c->stream));
        HIPCHK(c, hipMemcpyAsync(d_io.p, digits, (size_t)cb * 4 * M * 8, hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(k_load_digits, dim3((t2 + 255) / 256), dim3(256), 0, c->stream, d_io.p, L.dig, t2,
                           (uint32_t)c->logm, mode);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemsetAsync(L.ua, 0, (size_t)cpad * n * 4, c->stream));
        HIPCHK(c, hipMemcpyAsync(L.ua, ua.data(), ua.size() * 4, hipMemcpyHostToDevice, c->stream));
        const uint32_t callno = next_call_number(c);   // gate b draws as bootstrap b of this call
        c->last_call = callno;
        const ChunkJob J = debug_chunk_job(c, cb, callno);
        if ((rc = kloop_step(c, J, d_slice.p, k, mode, nullptr, &used))) return rc;
        hipLaunchKernelGGL(k_dump_digits, dim3((t2 + 255) / 256), dim3(256), 0, c->stream, L.dig, d_io.p, t2,
                           (uint32_t)c->logm, mode);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(digits_out, d_io.p, (size_t)cb * 4 * M * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return SGFHE_OK;
    });
    if (rc) return rc;
    ext_form_name(c, used.ext, mode, ext_name, ext_cap);
    crt_form_name(used.crt, crt_name, crt_cap);
    return SGFHE_OK;
}

int32_t sgfhe_debug_chunk_entry(sgfhe_ctx *c, const uint64_t *a1, const uint64_t *b1, const uint64_t *a2,
                                const uint64_t *b2, size_t rows, const uint32_t *lut, uint64_t *digits, uint32_t *ua) {
    if (!c || !a1 || !b1 || !a2 || !b2 || !digits || !ua) return SGFHE_ERR_INVALID_ARG;
    SGFHE_LOCK(c);
    const uint32_t mode = flatten_mode(c), M = c->M, n = c->n;
    if (rows == 0 || rows > base_chunk(chunk_policy(c, mode)))
        return fail(c, SGFHE_ERR_INVALID_ARG, "debug_chunk_entry: between 1 row and one chunk of the ctx");
    if (lut) {
        if (!lut_words_ok(lut, rows))
            return fail(c, SGFHE_ERR_INVALID_ARG, "debug_chunk_entry: a descriptor word is 0 or LUT_ROW | table");
        for (size_t b = 0; b < rows; b++) {   // a LUT row: words below r, as the LUT entries ask
            if (!(lut[b] & LUT_ROW)) continue;
            bool ok = b1[b] < c->par.r && b2[b] < c->par.r;
            for (size_t i = b * n; ok && i < (b + 1) * n; i++) ok = a1[i] < c->par.r && a2[i] < c->par.r;
            if (!ok) return fail(c, SGFHE_ERR_INVALID_ARG, "debug_chunk_entry: a word of LUT row " + std::to_string(b) + " is not below r");
        }
    }
    const uint32_t cb = (uint32_t)rows, cpad = round_up8(cb), t2 = cb * 2 * M;
    Scratch<uint64_t> d_in, d_dig;
    Scratch<uint32_t> d_lut;
    return run_drained(c, [&]() -> int32_t {
        int32_t rc = ensure_work(c, cpad);
        if (rc) return rc;
        if ((rc = scratch_alloc(c, d_in, (size_t)2 * cb * (n + 1)))) return rc;
        if ((rc = scratch_alloc(c, d_dig, (size_t)cb * 4 * M))) return rc;
        if (lut && (rc = scratch_alloc(c, d_lut, cb))) return rc;
        const Staging S = staging(d_in.p, cb, n);
        HIPCHK(c, hipMemcpyAsync(S.a1, a1, (size_t)cb * n * 8, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(S.a2, a2, (size_t)cb * n * 8, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(S.b1, b1, (size_t)cb * 8, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(S.b2, b2, (size_t)cb * 8, hipMemcpyHostToDevice, c->stream));
        if (lut) HIPCHK(c, hipMemcpyAsync(d_lut.p, lut, (size_t)cb * 4, hipMemcpyHostToDevice, c->stream));
        const uint32_t callno = next_call_number(c);   // row b draws as bootstrap b of this call
        c->last_call = callno;
        const ChunkJob J = debug_chunk_job(c, cb, callno);
        const LutDesc desc = {d_lut.p, false};
        if ((rc = chunk_entry(c, J, BootRows(S), lut ? &desc : nullptr, mode))) return rc;
        hipLaunchKernelGGL(k_dump_digits, dim3((t2 + 255) / 256), dim3(256), 0, c->stream, J.L->dig, d_dig.p, t2,
                           (uint32_t)c->logm, mode);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(digits, d_dig.p, (size_t)cb * 4 * M * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(ua, J.L->ua, (size_t)cb * n * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return SGFHE_OK;
    });
}

int32_t sgfhe_debug_chunk_exit(sgfhe_ctx *c, const uint64_t *digits, size_t rows, const uint32_t *lut,
                               const uint8_t *tables, size_t n_tables, uint32_t flags, uint64_t *out, uint64_t *acc) {
    if (!c || !digits || !out) return SGFHE_ERR_INVALID_ARG;
    SGFHE_LOCK(c);
    const uint32_t mode = flatten_mode(c), M = c->M, n = c->n;
    if (rows == 0 || rows > base_chunk(chunk_policy(c, mode)))
        return fail(c, SGFHE_ERR_INVALID_ARG, "debug_chunk_exit: between 1 row and one chunk of the ctx");
    if (flags & ~(SGFHE_FLAG_RAW_MODQ | SGFHE_FLAG_RAW_RNS2))
        return fail(c, SGFHE_ERR_INVALID_ARG, "debug_chunk_exit: flags are SGFHE_FLAG_RAW_MODQ and SGFHE_FLAG_RAW_RNS2");
    if (lut && tables)
        return fail(c, SGFHE_ERR_INVALID_ARG, "debug_chunk_exit: a per-row descriptor or a family, not both");
    if (tables && (n_tables < 1 || n_tables > SGFHE_LUT_MAX_TABLES))
        return fail(c, SGFHE_ERR_INVALID_ARG, "debug_chunk_exit: n_tables is 1 to SGFHE_LUT_MAX_TABLES");
    const size_t T = tables ? n_tables : 1;
    if (rows > ((size_t)1 << 31) / (n + 1) / T)   // (row and table counts are 32-bit on the device)
        return fail(c, SGFHE_ERR_INVALID_ARG, "debug_chunk_exit: too many rows");
    if (lut && !lut_words_ok(lut, rows))
        return fail(c, SGFHE_ERR_INVALID_ARG, "debug_chunk_exit: a descriptor word is 0 or LUT_ROW | table");
    if (flags & SGFHE_FLAG_RAW_RNS2) {
        if (!(flags & SGFHE_FLAG_RAW_MODQ))
            return fail(c, SGFHE_ERR_INVALID_ARG, "SGFHE_FLAG_RAW_RNS2 needs SGFHE_FLAG_RAW_MODQ");
        if (!c->have_rns2)
            return fail(c, SGFHE_ERR_INVALID_ARG, "SGFHE_FLAG_RAW_RNS2: no RNS2 moduli (upload the key with sgfhe_bkey_upload_rns2)");
        if (lut || tables)
            return fail(c, SGFHE_ERR_INVALID_ARG, "debug_chunk_exit: no SGFHE_FLAG_RAW_RNS2 with LUT rows");
    }
    for (size_t bc = 0; bc < rows * 2; bc++)
        for (uint32_t i = 0; i < M; i++)
            if (!storable_digits(c, digits[bc * 2 * M + i], digits[(bc * 2 + 1) * M + i]))
                return fail(c, SGFHE_ERR_INVALID_ARG, "debug_chunk_exit: a digit pair no flatten of this mode stores");
    const uint32_t cb = (uint32_t)rows, cpad = round_up8(cb), t2 = cb * 2 * M;
    const size_t out_words = rows * T * 3 * (n + 1) * ((flags & SGFHE_FLAG_RAW_MODQ) ? 2 : 1);
    bool all = lut != nullptr;   // every row a LUT row: k_final has nothing to write (sgfhe_bootstrap_lut_batch)
    for (size_t b = 0; lut && b < rows; b++) all = all && (lut[b] & LUT_ROW);
    Scratch<uint64_t> d_io, d_out;
    Scratch<ulonglong2> d_acc;
    Scratch<uint32_t> d_lut;
    Scratch<uint8_t> d_tab;
    return run_drained(c, [&]() -> int32_t {
        int32_t rc = ensure_work(c, cpad);
        if (rc) return rc;
        if ((rc = scratch_alloc(c, d_io, (size_t)cb * 4 * M))) return rc;
        if ((rc = scratch_alloc(c, d_out, out_words))) return rc;
        if (acc && (rc = scratch_alloc(c, d_acc, (size_t)cb * 2 * M))) return rc;
        if (lut && (rc = scratch_alloc(c, d_lut, cb))) return rc;
        if (tables && (rc = scratch_alloc(c, d_tab, rows * T))) return rc;
        const ChunkJob J = debug_chunk_job(c, cb, 0u);   // the exit draws nothing
        // one chunk as the k-loop leaves it: the rows' digit records (the padding rows zero)
        HIPCHK(c, hipMemsetAsync(J.L->dig, 0, (size_t)cpad * 2 * M * 16, c->stream));
        HIPCHK(c, hipMemcpyAsync(d_io.p, digits, (size_t)cb * 4 * M * 8, hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(k_load_digits, dim3((t2 + 255) / 256), dim3(256), 0, c->stream, d_io.p, J.L->dig, t2,
                           (uint32_t)c->logm, mode);
        HIPCHK(c, hipGetLastError());
        if (lut) HIPCHK(c, hipMemcpyAsync(d_lut.p, lut, (size_t)cb * 4, hipMemcpyHostToDevice, c->stream));
        if (tables) HIPCHK(c, hipMemcpyAsync(d_tab.p, tables, rows * T, hipMemcpyHostToDevice, c->stream));
        LutDesc desc = {d_lut.p, tables ? true : all};
        if (tables) desc.tables = d_tab.p, desc.n_tables = (uint32_t)T;
        BootCall call(c);
        call.batch = rows, call.out = d_out.p, call.flags = flags, call.acc_out = d_acc.p;
        if (lut || tables) call.lut = &desc;
        if ((rc = chunk_exit(c, J, call, mode))) return rc;
        HIPCHK(c, hipMemcpyAsync(out, d_out.p, out_words * 8, hipMemcpyDeviceToHost, c->stream));
        if (acc) HIPCHK(c, hipMemcpyAsync(acc, d_acc.p, (size_t)cb * 2 * M * 16, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return SGFHE_OK;
    });
}

// The pack work buffers of the ctx for calls of at most `count` ciphertexts and `total` ciphertexts of
// (w | v), in the ctx's present flatten mode; before anything is queued (nothing of the ctx in flight).
// `boots` of the call's ciphertexts are bootstrapped first (all of them in pack_encrypted_bits; the refreshed ones
// of a direct pack group); compact = true: pack_raw also holds a compact [count * n][n + 1] source (sgfhe_pack_lwe_modq).
static int32_t pack_grow(sgfhe_ctx *c, size_t count, size_t total, size_t boots, bool compact = false) {
    const size_t n = c->n, M = c->M, nb = boots * n;
    const uint32_t G = pack_group(c);
    const size_t groups = n / G, len = c->rnd ? M : n;
    int32_t rc;
    if ((rc = circ_grow(c, c->pack_lwe, 2 * nb * n + 2 * nb))) return rc;
    if ((rc = circ_grow(c, c->pack_raw, std::max(nb * 3, compact ? count * n : 0) * (n + 1)))) return rc;
    if ((rc = circ_grow(c, c->pack_pdig, count * n * 2 * len))) return rc;
    if ((rc = circ_grow(c, c->pack_yg, count * groups * 2 * cur(c).npr * M))) return rc;
    return circ_grow(c, c->pack_wv, 2 * total * M);
}

// The tail of pack_encrypted_bits (fhe.jl:675-695) on `count` groups of n un-reduced LWEs resident on the device,
// queued on `st`: the flatten of every as_i (drawing as call `call` of the ctx's stream in the randomised mode),
// the half-width external products and the finish into d_w / d_v [count][m].  The LWE of bit j of group ci is
// the n + 1 residues at raw + (ci * n + j) * rstride.  The caller has grown the work buffers and checked pack_G.
static int32_t pack_tail(sgfhe_ctx *c, const ulonglong2 *raw, uint32_t rstride, size_t count, uint64_t *d_w,
                         uint64_t *d_v, uint32_t call, hipStream_t st) {
    const size_t n = c->n, M = c->M;
    // rng != nothing: the flatten of every as_i (all m coefficients of the resized polynomial,
    // utils.jl:253-264) draws from the ctx's ChaCha stream (fhe.jl:683-684)
    const uint32_t mode = c->rnd ? MODE_RANDOM : 0u;
    const sgfhe_ctx::Basis &S = cur(c);
    const uint32_t G = pack_group(c);
    const uint32_t groups = (uint32_t)(n / G);
    const size_t len = c->rnd ? M : n;  // stored coefficients per digit polynomial
    int32_t rc;
    const RndArgs ra = {c->rnd_key, call, 0u, nullptr};
    const size_t tf = count * n * len;
    hipLaunchKernelGGL(k_pack_flatten, dim3((unsigned)((tf + 255) / 256)), dim3(256), 0, st, raw,
                       c->pack_pdig.p, S.d_crt, (uint32_t)count, (uint32_t)n, (uint32_t)c->logm, mode, ra, rstride);
    if ((rc = launch_shortprod(c, c->pack_pdig.p, c->pack_yg.p, (uint32_t)count, G, groups, mode, st))) return rc;
    const size_t tw = count * M;
    if ((rc = with_npr(c, S.npr, [&](auto np) -> int32_t {
            hipLaunchKernelGGL(k_pack_finish<decltype(np)::value>, dim3((unsigned)((tw + 255) / 256)), dim3(256), 0, st,
                               c->pack_yg.p, raw, d_w, d_v, S.d_crt, (uint32_t)count, (uint32_t)n,
                               (uint32_t)c->logm, groups, rstride);
            return SGFHE_OK;
        })))
        return rc;
    HIPCHK(c, hipGetLastError());
    return SGFHE_OK;
}

// Everything sgfhe_pack_encrypted_bits does on the device (run_drained waits for the stream when a step fails):
// pack_encrypted_bits (fhe.jl:660-696) of `count` groups of n LWEs -- the count * n bootstraps of the trivial encryption
// of 1 with the bits, then the tail as the SAME call of the ctx's draw stream (rng != nothing: the reference passes one
// rng to both, fhe.jl:673,683-684)
static int32_t pack_bits_queued(sgfhe_ctx *c, const uint64_t *a, const uint64_t *b, size_t count, uint64_t *out_w,
                                uint64_t *out_v) {
    const size_t n = c->n, M = c->M;
    const size_t nb = count * n;  // bootstraps
    hipStream_t st = c->stream;
    if (!(pack_group(c)))
        return fail(c, SGFHE_ERR_UNSUPPORTED, "pack_encrypted_bits: exactness bound of the RNS primes");
    if (pack_grow(c, count, count, count)) return fail(c, SGFHE_ERR_HIP, hipGetErrorString(hipErrorOutOfMemory));
    // [a1 = 0 | a2 | b1 = Dr | b2]: trivial encryption of 1 paired with every bit (fhe.jl:669-673)
    const Staging S = staging(c->pack_lwe.p, nb, n);
    uint64_t *d_w = c->pack_wv.p, *d_v = d_w + count * M;
    HIPCHK(c, hipMemsetAsync(S.a1, 0, nb * n * 8, st));
    std::vector<uint64_t> ones(nb, c->par.r / 4);
    HIPCHK(c, hipMemcpyAsync(S.b1, ones.data(), nb * 8, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(S.a2, a, nb * n * 8, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(S.b2, b, nb * 8, hipMemcpyHostToDevice, st));
    BootCall call(c);
    call.rows = S, call.batch = nb, call.out = (uint64_t *)c->pack_raw.p, call.flags = SGFHE_FLAG_RAW_MODQ;
    int32_t rc = bootstrap_device(c, call);
    if (rc) return rc;
    if ((rc = pack_tail(c, c->pack_raw.p, 3 * (uint32_t)(n + 1), count, d_w, d_v, c->last_call, st))) return rc;
    HIPCHK(c, hipMemcpyAsync(out_w, d_w, count * M * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(out_v, d_v, count * M * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    return SGFHE_OK;
}

int32_t sgfhe_pack_encrypted_bits(sgfhe_ctx *c, const uint64_t *a, const uint64_t *b, size_t count,
                                  uint64_t *out_w, uint64_t *out_v) {
    if (!c || !a || !b || !out_w || !out_v) return SGFHE_ERR_INVALID_ARG;
    SGFHE_LOCK(c);
    if (count == 0) return SGFHE_OK;
    if (!c->have_key) return fail(c, SGFHE_ERR_NO_KEY, "no bootstrap key uploaded");
    return run_drained(c, [&] { return pack_bits_queued(c, a, b, count, out_w, out_v); });
}

// everything sgfhe_pack_lwe_modq does on the device: `words` residues up, the tail, (w, v) down
static int32_t pack_modq_queued(sgfhe_ctx *c, const uint64_t *lwe, size_t count, size_t words, uint64_t *out_w,
                                uint64_t *out_v) {
    const size_t M = c->M;
    hipStream_t st = c->stream;
    if (!(pack_group(c)))
        return fail(c, SGFHE_ERR_UNSUPPORTED, "pack_encrypted_bits: exactness bound of the RNS primes");
    int32_t rc = pack_grow(c, count, count, 0, true);
    if (rc) return rc;
    const uint32_t call = c->rnd ? c->rnd_call++ : 0u;   // one call of the draw stream: the flatten of every as_i
    c->last_call = call;
    uint64_t *d_w = c->pack_wv.p, *d_v = d_w + count * M;
    HIPCHK(c, hipMemcpyAsync(c->pack_raw.p, lwe, words * 16, hipMemcpyHostToDevice, st));
    if ((rc = pack_tail(c, c->pack_raw.p, (uint32_t)(c->n + 1), count, d_w, d_v, call, st))) return rc;
    HIPCHK(c, hipMemcpyAsync(out_w, d_w, count * M * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(out_v, d_v, count * M * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    return SGFHE_OK;
}

int32_t sgfhe_pack_lwe_modq(sgfhe_ctx *c, const uint64_t *lwe, size_t count, uint64_t *out_w, uint64_t *out_v) {
    if (!c || !lwe || !out_w || !out_v) return SGFHE_ERR_INVALID_ARG;
    SGFHE_LOCK(c);
    if (count == 0) return SGFHE_OK;
    if (!c->have_key) return fail(c, SGFHE_ERR_NO_KEY, "no bootstrap key uploaded");
    const size_t words = count * c->n * (c->n + 1);   // residues
    for (size_t i = 0; i < words; i++)
        if ((((u128)lwe[2 * i + 1] << 64) | lwe[2 * i]) >= c->Q)
            return fail(c, SGFHE_ERR_INVALID_ARG, "sgfhe_pack_lwe_modq: residue " + std::to_string(i) + " is not below Q");
    return run_drained(c, [&] { return pack_modq_queued(c, lwe, count, words, out_w, out_v); });
}

// everything sgfhe_lwe_lift_modq does on the device
// (the pack path's buffers: its LWE staging takes the rows, its un-reduced rows the residues)
static int32_t lwe_lift_queued(sgfhe_ctx *c, const uint64_t *lwe, size_t words, uint64_t *out) {
    hipStream_t st = c->stream;
    int32_t rc;
    if ((rc = circ_grow(c, c->pack_lwe, words))) return rc;
    if ((rc = circ_grow(c, c->pack_raw, words))) return rc;
    HIPCHK(c, hipMemcpyAsync(c->pack_lwe.p, lwe, words * 8, hipMemcpyHostToDevice, st));
    const size_t blocks = std::min<size_t>((words + 255) / 256, (size_t)1 << 20);
    hipLaunchKernelGGL(k_lwe_lift, dim3((uint32_t)blocks), dim3(256), 0, st, c->pack_lwe.p, c->pack_raw.p, cur(c).d_crt,
                       words);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(out, c->pack_raw.p, words * 16, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    return SGFHE_OK;
}

int32_t sgfhe_lwe_lift_modq(sgfhe_ctx *c, const uint64_t *lwe, size_t count, uint64_t *out) {
    if (!c) return SGFHE_ERR_INVALID_ARG;
    SGFHE_LOCK(c);
    if (count == 0) return SGFHE_OK;
    if (!lwe || !out) return fail(c, SGFHE_ERR_INVALID_ARG, "sgfhe_lwe_lift_modq: NULL row or output pointer");
    const size_t row = c->n + 1;
    if (count > ((size_t)1 << 40) / row)   // (the byte counts below stay far inside 64 bits)
        return fail(c, SGFHE_ERR_INVALID_ARG, "sgfhe_lwe_lift_modq: too many rows");
    const size_t words = count * row;
    for (size_t i = 0; i < words; i++)
        if (lwe[i] >= c->par.r)
            return fail(c, SGFHE_ERR_INVALID_ARG, "sgfhe_lwe_lift_modq: word " + std::to_string(i) + " is not below r");
    return run_drained(c, [&] { return lwe_lift_queued(c, lwe, words, out); });
}

// everything sgfhe_bootstrap_lut_batch and sgfhe_bootstrap_lut_multi_batch do on the device; `tables`: the family
// call's [row][n_tables], NULL for the single-table call, whose tables are in the descriptor words
// (the pack path's buffers: its LWE staging takes the rows, zeros for the second input, the descriptor and, behind
//  it, eight to a uint64, the tables; its un-reduced rows the result in either form)
static int32_t bootstrap_lut_queued(sgfhe_ctx *c, const uint64_t *a, const uint64_t *b, const std::vector<uint32_t> &words,
                                    const uint8_t *tables, size_t n_tables, size_t batch, uint64_t *out, uint32_t flags) {
    const size_t n = c->n;
    hipStream_t st = c->stream;
    const bool raw = flags & SGFHE_FLAG_RAW_MODQ;
    const size_t out_words = batch * n_tables * 3 * (n + 1) * (raw ? 2 : 1);
    // [a1 | a2 = 0 | b1 | b2 = 0 | descriptor words, two to a uint64 | tables]
    const size_t desc = 2 * batch * n + 2 * batch, tab = desc + (batch + 1) / 2;
    int32_t rc;
    if ((rc = circ_grow(c, c->pack_lwe, tab + (tables ? (batch * n_tables + 7) / 8 : 0)))) return rc;
    if ((rc = circ_grow(c, c->pack_raw, (out_words + 1) / 2))) return rc;
    const Staging S = staging(c->pack_lwe.p, batch, n);
    uint32_t *d_lut = reinterpret_cast<uint32_t *>(c->pack_lwe.p + desc);
    uint8_t *d_tab = reinterpret_cast<uint8_t *>(c->pack_lwe.p + tab);
    HIPCHK(c, hipMemcpyAsync(S.a1, a, batch * n * 8, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(S.b1, b, batch * 8, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemsetAsync(S.a2, 0, batch * n * 8, st));
    HIPCHK(c, hipMemsetAsync(S.b2, 0, batch * 8, st));
    HIPCHK(c, hipMemcpyAsync(d_lut, words.data(), batch * 4, hipMemcpyHostToDevice, st));
    if (tables) HIPCHK(c, hipMemcpyAsync(d_tab, tables, batch * n_tables, hipMemcpyHostToDevice, st));
    LutDesc lut = {d_lut, true};
    if (tables) lut.tables = d_tab, lut.n_tables = (uint32_t)n_tables;
    uint64_t *d_out = reinterpret_cast<uint64_t *>(c->pack_raw.p);
    BootCall call(c);
    call.rows = S, call.batch = batch, call.out = d_out, call.flags = flags, call.lut = &lut;
    if ((rc = bootstrap_device(c, call))) return rc;
    HIPCHK(c, hipMemcpyAsync(out, d_out, out_words * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    c->pending = false;
    return SGFHE_OK;
}

// What both entries check of a call that has rows, build of it on the host, and run: `name` is the entry's, for the
// error strings.  `family`: `tables` is [row][n_tables] and goes to the device as it is; otherwise it holds one
// table per row, which goes into the row's descriptor word.
static int32_t bootstrap_lut(sgfhe_ctx *c, const std::string &name, const uint64_t *a, const uint64_t *b,
                             const uint8_t *tables, size_t n_tables, bool family, size_t batch, uint64_t *out,
                             uint32_t flags) {
    if (!a || !b || !tables || !out)
        return fail(c, SGFHE_ERR_INVALID_ARG, name + ": NULL row, table or output pointer");
    if (flags & ~SGFHE_FLAG_RAW_MODQ)
        return fail(c, SGFHE_ERR_INVALID_ARG, name + ": flags is 0 or SGFHE_FLAG_RAW_MODQ");
    if (!c->have_key) return fail(c, SGFHE_ERR_NO_KEY, "no bootstrap key uploaded");
    if (batch > ((size_t)1 << 31) / (c->n + 1) / n_tables)   // (row and table counts are 32-bit on the device)
        return fail(c, SGFHE_ERR_INVALID_ARG, name + ": too many rows");
    for (size_t i = 0; i < batch * c->n; i++)
        if (a[i] >= c->par.r)
            return fail(c, SGFHE_ERR_INVALID_ARG, name + ": word " + std::to_string(i) + " of a is not below r");
    for (size_t i = 0; i < batch; i++)
        if (b[i] >= c->par.r)
            return fail(c, SGFHE_ERR_INVALID_ARG, name + ": b of row " + std::to_string(i) + " is not below r");
    std::vector<uint32_t> words;   // the descriptor of k_init: every row is a LUT row
    try {
        words.assign(batch, LUT_ROW);
    } catch (...) {
        return fail(c, SGFHE_ERR_OOM, "out of host memory");
    }
    if (!family)   // ... and carries its table: LUT_ROW | table
        for (size_t t = 0; t < batch; t++) words[t] |= tables[t];
    return run_drained(c, [&] {
        return bootstrap_lut_queued(c, a, b, words, family ? tables : nullptr, n_tables, batch, out, flags);
    });
}

int32_t sgfhe_bootstrap_lut_batch(sgfhe_ctx *c, const uint64_t *a, const uint64_t *b, const uint8_t *table, size_t batch,
                                  uint64_t *out, uint32_t flags) {
    if (!c) return SGFHE_ERR_INVALID_ARG;
    SGFHE_LOCK(c);
    if (batch == 0) return SGFHE_OK;
    return bootstrap_lut(c, "sgfhe_bootstrap_lut_batch", a, b, table, 1, false, batch, out, flags);
}

int32_t sgfhe_bootstrap_lut_multi_batch(sgfhe_ctx *c, const uint64_t *a, const uint64_t *b, const uint8_t *tables,
                                        size_t n_tables, size_t batch, uint64_t *out, uint32_t flags) {
    if (!c) return SGFHE_ERR_INVALID_ARG;
    SGFHE_LOCK(c);
    if (n_tables < 1 || n_tables > SGFHE_LUT_MAX_TABLES)
        return fail(c, SGFHE_ERR_INVALID_ARG, "sgfhe_bootstrap_lut_multi_batch: n_tables is 1 to SGFHE_LUT_MAX_TABLES");
    if (flags & ~SGFHE_FLAG_RAW_MODQ)   // (this entry checks its flags on an empty call too)
        return fail(c, SGFHE_ERR_INVALID_ARG, "sgfhe_bootstrap_lut_multi_batch: flags is 0 or SGFHE_FLAG_RAW_MODQ");
    if (batch == 0) return SGFHE_OK;
    return bootstrap_lut(c, "sgfhe_bootstrap_lut_multi_batch", a, b, tables, n_tables, true, batch, out, flags);
}

int32_t sgfhe_debug_ntt(sgfhe_ctx *c, uint32_t prime_index, int inverse, const uint32_t *in,
                        uint32_t *out) {
    if (!c || !in || !out) return SGFHE_ERR_INVALID_ARG;
    SGFHE_LOCK(c);
    if (prime_index >= cur(c).npr) return SGFHE_ERR_INVALID_ARG;
    Scratch<uint32_t> d;
    return run_drained(c, [&]() -> int32_t {
        const size_t M = c->M;
        int32_t rc = scratch_alloc(c, d, 2 * M);
        if (rc) return rc;
        HIPCHK(c, hipMemcpyAsync(d.p, in, M * 4, hipMemcpyHostToDevice, c->stream));
        if ((rc = launch_dbgntt(c, d.p, d.p + M, prime_index, inverse, c->stream))) return rc;
        HIPCHK(c, hipMemcpyAsync(out, d.p + M, M * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return SGFHE_OK;
    });
}

int32_t sgfhe_debug_primes(const sgfhe_ctx *c, uint32_t *count, uint32_t *primes) {
    if (!c || !count || !primes) return SGFHE_ERR_INVALID_ARG;
    SGFHE_LOCK(c);
    *count = cur(c).npr;
    for (uint32_t i = 0; i < cur(c).npr; i++) primes[i] = cur(c).primes[i];
    return SGFHE_OK;
}

// ---- N3: the ciphertext plumbing either side of the path, on the host (no device, no ctx) ----------

namespace {
// r = 2 m a power of two, n <= m, t = log2(r) - 1, Dr = r / 4
bool host_params_ok(const sgfhe_params *p) {
    return p && p->n >= 1 && p->m >= p->n && p->r == 2 * p->m && (p->r & (p->r - 1)) == 0 && p->r >= 32 &&
           p->r <= (1ull << 32);
}
unsigned host_t(const sgfhe_params *p) {
    unsigned lg = 0;
    while ((1ull << lg) < p->r) lg++;
    return lg - 1;
}
}  // namespace

int32_t sgfhe_host_deterministic_expand(const sgfhe_params *p, const uint8_t *u, uint64_t *a) {
    if (!host_params_ok(p) || !u || !a) return SGFHE_ERR_INVALID_ARG;
    sgfhe_host::prng_expand(u, p->n, host_t(p) + 1, a);
    for (uint64_t i = 0; i < p->n; i++) a[i] &= p->r - 1;
    return SGFHE_OK;
}

int32_t sgfhe_host_encrypt_private(const sgfhe_params *p, const uint64_t *sk, const uint8_t *u,
                                   const int64_t *w, const uint8_t *message, uint64_t *a, uint64_t *b) {
    if (!host_params_ok(p) || !sk || !u || !w || !message || !a || !b) return SGFHE_ERR_INVALID_ARG;
    const uint64_t n = p->n, rmask = p->r - 1, Dr = p->r / 4;
    const int64_t wr = (int64_t)(Dr / 8);
    for (uint64_t i = 0; i < n; i++)
        if (w[i] < -wr || w[i] > wr) return SGFHE_ERR_INVALID_ARG;      // w in -Dr/8 .. Dr/8 (fhe.jl:318-319)
    int32_t rc = sgfhe_host_deterministic_expand(p, u, a);             // fhe.jl:316
    if (rc) return rc;
    std::vector<uint64_t> key(n), as(n);
    for (uint64_t i = 0; i < n; i++) key[i] = sk[i] & 1;
    sgfhe_host::negacyclic_mul(a, key.data(), n, rmask, as.data());
    const unsigned sh = host_t(p) - 4;
    for (uint64_t i = 0; i < n; i++) {
        const uint64_t v = (as[i] + (uint64_t)w[i] + (uint64_t)(message[i] & 1) * Dr) & rmask;   // fhe.jl:322
        b[i] = (v >> sh) << sh;                                          // the highmost 5 bits (fhe.jl:325)
    }
    return SGFHE_OK;
}

int32_t sgfhe_host_pack_private(const sgfhe_params *p, const uint64_t *b, uint8_t *v) {
    if (!host_params_ok(p) || !b || !v) return SGFHE_ERR_INVALID_ARG;
    std::vector<uint64_t> packed(p->n);
    const unsigned sh = host_t(p) - 4;
    for (uint64_t i = 0; i < p->n; i++) packed[i] = b[i] >> sh;        // fhe.jl:342
    sgfhe_host::unpackbits(packed.data(), p->n, 5, v);
    return SGFHE_OK;
}

int32_t sgfhe_host_normalize_private(const sgfhe_params *p, const uint8_t *u, const uint8_t *v,
                                     uint64_t *a, uint64_t *b) {
    if (!host_params_ok(p) || !u || !v || !a || !b) return SGFHE_ERR_INVALID_ARG;
    int32_t rc = sgfhe_host_deterministic_expand(p, u, a);             // fhe.jl:356
    if (rc) return rc;
    sgfhe_host::packbits(v, 5, p->n, b);                               // fhe.jl:357
    const unsigned sh = host_t(p) - 4;
    for (uint64_t i = 0; i < p->n; i++) b[i] = (b[i] << sh) & (p->r - 1);
    return SGFHE_OK;
}

int32_t sgfhe_host_split_ciphertext(const sgfhe_params *p, const uint64_t *a, const uint64_t *b,
                                    size_t N, uint64_t *lwe_a, uint64_t *lwe_b) {
    if (!host_params_ok(p) || !a || !b || !lwe_a || !lwe_b || (N != p->n && N != p->m))
        return SGFHE_ERR_INVALID_ARG;
    const uint64_t n = p->n, rmask = p->r - 1;
    for (uint64_t i = 1; i <= n; i++) {                                 // fhe.jl:288-289
        sgfhe_host::extract(a, N, i, n, rmask, lwe_a + (i - 1) * n);
        lwe_b[i - 1] = b[i - 1] & rmask;
    }
    return SGFHE_OK;
}

int32_t sgfhe_host_decrypt_lwe(const sgfhe_params *p, const uint64_t *sk, const uint64_t *lwe_a,
                               const uint64_t *lwe_b, size_t count, uint8_t *bits) {
    if (!host_params_ok(p) || !sk || !lwe_a || !lwe_b || !bits) return SGFHE_ERR_INVALID_ARG;
    const uint64_t n = p->n, rmask = p->r - 1, Dr = p->r / 4;
    for (size_t t = 0; t < count; t++) {
        uint64_t dot = 0;
        for (uint64_t i = 0; i < n; i++) dot += lwe_a[t * n + i] * (sk[i] & 1);
        const uint64_t b1 = (lwe_b[t] - dot) & rmask;                    // fhe.jl:505
        bits[t] = (uint8_t)((((b1 + Dr / 2) & rmask) / Dr) & 1);         // fhe.jl:506
    }
    return SGFHE_OK;
}

int32_t sgfhe_host_decrypt_rlwe(const sgfhe_params *p, const uint64_t *sk, const uint64_t *a,
                                const uint64_t *b, size_t N, uint8_t *bits) {
    if (!host_params_ok(p) || !sk || !a || !b || !bits || (N != p->n && N != p->m))
        return SGFHE_ERR_INVALID_ARG;
    const uint64_t n = p->n, rmask = p->r - 1, Dr = p->r / 4;
    std::vector<uint64_t> key(N, 0), as(N);                              // resize(key, m) for a Ciphertext (fhe.jl:474-478)
    for (uint64_t i = 0; i < n; i++) key[i] = sk[i] & 1;
    sgfhe_host::negacyclic_mul(a, key.data(), N, rmask, as.data());
    for (uint64_t i = 0; i < n; i++) {                                   // the first n coefficients (fhe.jl:481-482)
        const uint64_t b1 = (b[i] - as[i]) & rmask;
        bits[i] = (uint8_t)((((b1 + Dr / 2) & rmask) / Dr) & 1);         // fhe.jl:491-493
    }
    return SGFHE_OK;
}

// ---- the public-key side (row N4) ------------------------------------------------------------------
static bool host_q_ok(const sgfhe_params *p, uint64_t q) {
    // q = find_modulus(2 n, r n) (fhe.jl:57): odd, 2 n | q - 1, above r n, and small enough for the
    // 64-bit products of rescale (q r < 2^64) and of the short convolution (n q < 2^62)
    return host_params_ok(p) && q > p->r * p->n && q < (1ull << 31) && (q - 1) % (2 * p->n) == 0;
}
static int64_t host_e_max(const sgfhe_params *p, uint64_t q) {
    const uint64_t Dq = q / 4, d = 41 * p->n;                            // fhe.jl:159-160
    return (int64_t)(Dq / d) - (Dq % d == 0 ? 1 : 0);
}

int32_t sgfhe_host_public_key(const sgfhe_params *p, uint64_t q, const uint64_t *sk, const uint64_t *k0,
                              const int64_t *e, uint64_t *k1) {
    if (!sk || !k0 || !e || !k1 || !p || !host_q_ok(p, q)) return SGFHE_ERR_INVALID_ARG;
    const size_t n = p->n;
    const int64_t e_max = host_e_max(p, q);
    std::vector<int8_t> s(n);
    for (size_t i = 0; i < n; i++) {
        if (k0[i] >= q || e[i] < -e_max || e[i] > e_max) return SGFHE_ERR_INVALID_ARG;
        s[i] = (int8_t)(sk[i] & 1);
    }
    std::vector<int64_t> ks(n);
    sgfhe_host::negacyclic_mul_short(k0, s.data(), n, q, ks.data());     // fhe.jl:163-164
    for (size_t i = 0; i < n; i++) {
        const int64_t v = (ks[i] + e[i]) % (int64_t)q;
        k1[i] = (uint64_t)(v < 0 ? v + (int64_t)q : v);
    }
    return SGFHE_OK;
}

int32_t sgfhe_host_encrypt_public(const sgfhe_params *p, uint64_t q, const uint64_t *k0, const uint64_t *k1,
                                  const int8_t *u, const int64_t *w1, const int64_t *w2,
                                  const uint8_t *message, uint64_t *a, uint64_t *b) {
    if (!k0 || !k1 || !u || !w1 || !w2 || !message || !a || !b || !p || !host_q_ok(p, q))
        return SGFHE_ERR_INVALID_ARG;
    const size_t n = p->n;
    const uint64_t r = p->r, Dq = q / 4;
    const int t = (int)host_t(p);                                        // r = 2^(t + 1)
    if (t < 5) return SGFHE_ERR_INVALID_ARG;                             // fhe.jl:404
    const int shift = t - 5;
    const int64_t w1_max = (int64_t)(Dq / (41 * n)), w2_max = (int64_t)(Dq / 82);   // fhe.jl:392,395
    for (size_t i = 0; i < n; i++)
        if (k0[i] >= q || k1[i] >= q || u[i] < -1 || u[i] > 1 || w1[i] < -w1_max || w1[i] > w1_max ||
            w2[i] < -w2_max || w2[i] > w2_max)
            return SGFHE_ERR_INVALID_ARG;
    std::vector<int64_t> k0u(n), k1u(n);
    sgfhe_host::negacyclic_mul_short(k0, u, n, q, k0u.data());           // fhe.jl:399
    sgfhe_host::negacyclic_mul_short(k1, u, n, q, k1u.data());           // fhe.jl:400
    for (size_t i = 0; i < n; i++) {
        int64_t a1 = (k0u[i] + w1[i]) % (int64_t)q;
        if (a1 < 0) a1 += (int64_t)q;
        int64_t a2 = (k1u[i] + w2[i] + (int64_t)((message[i] & 1) * Dq)) % (int64_t)q;
        if (a2 < 0) a2 += (int64_t)q;
        a[i] = sgfhe_host::rescale(r, (uint64_t)a1, q, true);            // fhe.jl:402
        b[i] = (sgfhe_host::rescale(r >> shift, (uint64_t)a2, q, false) << shift) & (r - 1);   // :405-406
    }
    return SGFHE_OK;
}

int32_t sgfhe_host_pack_public(const sgfhe_params *p, const uint64_t *a, const uint64_t *b,
                               uint8_t *a_bits, uint8_t *b_bits) {
    if (!host_params_ok(p) || !a || !b || !a_bits || !b_bits) return SGFHE_ERR_INVALID_ARG;
    const size_t n = p->n;
    const int t = (int)host_t(p);
    if (t < 5) return SGFHE_ERR_INVALID_ARG;
    sgfhe_host::unpackbits(a, n, (size_t)t + 1, a_bits);                 // fhe.jl:429
    std::vector<uint64_t> bp(n);
    for (size_t i = 0; i < n; i++) bp[i] = (b[i] & (p->r - 1)) >> (t - 5);   // fhe.jl:431
    sgfhe_host::unpackbits(bp.data(), n, 6, b_bits);                     // fhe.jl:432
    return SGFHE_OK;
}

int32_t sgfhe_host_normalize_public(const sgfhe_params *p, const uint8_t *a_bits, const uint8_t *b_bits,
                                    uint64_t *a, uint64_t *b) {
    if (!host_params_ok(p) || !a_bits || !b_bits || !a || !b) return SGFHE_ERR_INVALID_ARG;
    const size_t n = p->n;
    const int t = (int)host_t(p);
    if (t < 5) return SGFHE_ERR_INVALID_ARG;
    sgfhe_host::packbits(a_bits, (size_t)t + 1, n, a);                   // fhe.jl:446
    sgfhe_host::packbits(b_bits, 6, n, b);                               // fhe.jl:447
    for (size_t i = 0; i < n; i++) {
        a[i] &= p->r - 1;
        b[i] = (b[i] << (t - 5)) & (p->r - 1);
    }
    return SGFHE_OK;
}

int32_t sgfhe_kernel_names(const sgfhe_ctx *c, char *extprod, size_t extprod_cap, char *crt, size_t crt_cap) {
    if (!c || !extprod || !crt || !extprod_cap || !crt_cap) return SGFHE_ERR_INVALID_ARG;
    SGFHE_LOCK(c);
    // the throughput form at the ctx's present mode: what ext_form / crt_form give a large chunk
    const uint32_t mode = flatten_mode(c);
    ext_form_name(c, ExtForm{ExtKind::Throughput, ~0u}, mode, extprod, extprod_cap);
    CrtForm f = crt_form(c, mode, ~0u, false);
    // (k_crt_lean<5, 3, true>, the crt_lean87_one instantiation, reports as k_crt_lean<5, 3> here: same
    // function, same memory side; sgfhe_debug_kloop_step tells the two apart)
    f.p87 = false;
    crt_form_name(f, crt, crt_cap);
    return SGFHE_OK;
}

int32_t sgfhe_release_host_staging(sgfhe_ctx *c) {
    if (!c) return SGFHE_ERR_INVALID_ARG;
    SGFHE_LOCK(c);
    (void)hipSetDevice(c->device);
    SGFHE_QUIESCE(c);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    free_io_buffers(c);
    free_circuit_buffers(c);
    return SGFHE_OK;
}

int32_t sgfhe_timing_enable(sgfhe_ctx *c, int enable) {
    if (!c) return SGFHE_ERR_INVALID_ARG;
    SGFHE_LOCK(c);
    c->timing = enable != 0;
    return SGFHE_OK;
}

int32_t sgfhe_timing_read(sgfhe_ctx *c, double *stats, int reset) {
    if (!c || !stats) return SGFHE_ERR_INVALID_ARG;
    SGFHE_LOCK(c);
    (void)hipSetDevice(c->device);
    int32_t rcd = drain(c);
    if (rcd) return rcd;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    timing_flush(c);
    stats[0] = c->n_ext ? c->t_ext / (double)c->n_ext : 0.0;
    stats[1] = (double)c->n_ext;
    stats[2] = c->n_crt ? c->t_crt / (double)c->n_crt : 0.0;
    stats[3] = (double)c->n_crt;
    stats[4] = (double)c->last_chunk;
    stats[5] = c->n_call ? c->t_call / (double)c->n_call : 0.0;
    stats[6] = (double)c->n_call;
    stats[7] = c->n_call ? (double)c->boots_call / (double)c->n_call : 0.0;
    if (reset) {
        c->t_ext = c->t_crt = c->t_call = 0;
        c->n_ext = c->n_crt = c->n_call = c->boots_call = 0;
    }
    return SGFHE_OK;
}

// ---- gate circuits (csrc/circuit.h plans) ---------------------------------------

// Every entry fills one CircuitSpec (csrc/circuit.h) from its arrays.  A refused circuit allocates nothing: the planner
// validates before it builds, and into a local
static int32_t circuit_create(const CircuitSpec &S, sgfhe_circuit **out) {
    if (!out) return SGFHE_ERR_INVALID_ARG;
    *out = nullptr;
    CircuitPlan plan;
    const int32_t rc = circuit_plan(S, plan);
    if (rc) return rc;
    sgfhe_circuit *c = new (std::nothrow) sgfhe_circuit();
    if (!c) return SGFHE_ERR_OOM;
    c->plan = std::move(plan);
    *out = c;
    return SGFHE_OK;
}

// what every entry has: the inputs, the nodes, the outputs and the lane group
static CircuitSpec circuit_spec(uint32_t n_inputs, const CircuitNodes &N, size_t n_gates, const uint32_t *outputs,
                                const int32_t *out_shift, size_t n_outputs, uint32_t group) {
    CircuitSpec S;
    S.n_inputs = n_inputs, S.nodes = N, S.n_gates = n_gates;
    S.outputs = outputs, S.out_shift = out_shift, S.n_outputs = n_outputs, S.group = group;
    return S;
}

int32_t sgfhe_circuit_create_lanes(uint32_t n_inputs, const uint32_t *gates, const int32_t *gate_shift, size_t n_gates,
                                   const uint32_t *outputs, const int32_t *out_shift, size_t n_outputs, uint32_t group,
                                   sgfhe_circuit **out) {
    const CircuitNodes N = circuit_nodes_arity(2, gates, gate_shift);
    return circuit_create(circuit_spec(n_inputs, N, n_gates, outputs, out_shift, n_outputs, group), out);
}

int32_t sgfhe_circuit_create3(uint32_t n_inputs, const uint32_t *gates, const int32_t *gate_shift, size_t n_gates,
                              const uint32_t *outputs, const int32_t *out_shift, size_t n_outputs, uint32_t group,
                              sgfhe_circuit **out) {
    const CircuitNodes N = circuit_nodes_arity(3, gates, gate_shift);
    return circuit_create(circuit_spec(n_inputs, N, n_gates, outputs, out_shift, n_outputs, group), out);
}

int32_t sgfhe_circuit_create_w(uint32_t n_inputs, const uint32_t *node_kind, const uint32_t *node_start,
                               const uint32_t *term_ref, const int32_t *term_shift, const int32_t *term_weight,
                               size_t n_gates, const uint32_t *outputs, const int32_t *out_shift, size_t n_outputs,
                               uint32_t group, sgfhe_circuit **out) {
    const CircuitNodes N = circuit_nodes_csr(1, node_kind, node_start, term_ref, term_shift, term_weight);
    return circuit_create(circuit_spec(n_inputs, N, n_gates, outputs, out_shift, n_outputs, group), out);
}

int32_t sgfhe_circuit_create_lut(uint32_t n_inputs, const uint32_t *node_kind, const uint32_t *node_start,
                                 const uint32_t *term_ref, const int32_t *term_shift, const int32_t *term_weight,
                                 const uint32_t *node_table, size_t n_gates, const uint32_t *outputs,
                                 const int32_t *out_shift, size_t n_outputs, uint32_t group, sgfhe_circuit **out) {
    const CircuitNodes N = circuit_nodes_csr(2, node_kind, node_start, term_ref, term_shift, term_weight, node_table);
    return circuit_create(circuit_spec(n_inputs, N, n_gates, outputs, out_shift, n_outputs, group), out);
}

int32_t sgfhe_circuit_create_lut_multi(uint32_t n_inputs, const uint32_t *node_kind, const uint32_t *node_start,
                                       const uint32_t *term_ref, const int32_t *term_shift, const int32_t *term_weight,
                                       const uint32_t *node_table, size_t n_gates, const uint32_t *outputs,
                                       const int32_t *out_shift, size_t n_outputs, uint32_t group, sgfhe_circuit **out) {
    const CircuitNodes N = circuit_nodes_csr(3, node_kind, node_start, term_ref, term_shift, term_weight, node_table);
    return circuit_create(circuit_spec(n_inputs, N, n_gates, outputs, out_shift, n_outputs, group), out);
}

// (sgfhe_circuit_create_data is the routed entry without registers, and sgfhe_circuit_create_seq without routes)
int32_t sgfhe_circuit_create_data(uint32_t n_inputs, uint32_t n_planes, const uint32_t *node_kind,
                                  const uint32_t *node_start, const uint32_t *term_ref, const int32_t *term_shift,
                                  const int32_t *term_weight, const uint32_t *node_table, size_t n_gates,
                                  const uint32_t *outputs, const int32_t *out_shift, size_t n_outputs, uint32_t group,
                                  sgfhe_circuit **out) {
    return sgfhe_circuit_create_routed(n_inputs, n_planes, node_kind, node_start, term_ref, term_shift, term_weight,
                                       node_table, n_gates, outputs, out_shift, n_outputs, group, 0, nullptr, nullptr,
                                       nullptr, 0, nullptr, nullptr, nullptr, nullptr, out);
}

int32_t sgfhe_circuit_create_seq(uint32_t n_inputs, uint32_t n_planes, const uint32_t *node_kind,
                                 const uint32_t *node_start, const uint32_t *term_ref, const int32_t *term_shift,
                                 const int32_t *term_weight, const uint32_t *node_table, size_t n_gates,
                                 const uint32_t *outputs, const int32_t *out_shift, size_t n_outputs, uint32_t group,
                                 uint32_t n_regs, const uint32_t *next_ref, const int32_t *next_shift,
                                 const uint32_t *reg_scale, sgfhe_circuit **out) {
    return sgfhe_circuit_create_routed(n_inputs, n_planes, node_kind, node_start, term_ref, term_shift, term_weight,
                                       node_table, n_gates, outputs, out_shift, n_outputs, group, n_regs, next_ref,
                                       next_shift, reg_scale, 0, nullptr, nullptr, nullptr, nullptr, out);
}

// (... and sgfhe_circuit_create_routed the masked entry without masks)
int32_t sgfhe_circuit_create_routed(uint32_t n_inputs, uint32_t n_planes, const uint32_t *node_kind,
                                    const uint32_t *node_start, const uint32_t *term_ref, const int32_t *term_shift,
                                    const int32_t *term_weight, const uint32_t *node_table, size_t n_gates,
                                    const uint32_t *outputs, const int32_t *out_shift, size_t n_outputs, uint32_t group,
                                    uint32_t n_regs, const uint32_t *next_ref, const int32_t *next_shift,
                                    const uint32_t *reg_scale, uint32_t n_routes, const int32_t *routes,
                                    const uint32_t *term_route, const uint32_t *out_route, const uint32_t *next_route,
                                    sgfhe_circuit **out) {
    return sgfhe_circuit_create_masked(n_inputs, n_planes, node_kind, node_start, term_ref, term_shift, term_weight,
                                       node_table, n_gates, outputs, out_shift, n_outputs, group, n_regs, next_ref,
                                       next_shift, reg_scale, n_routes, routes, term_route, out_route, next_route, 0,
                                       nullptr, nullptr, out);
}

int32_t sgfhe_circuit_create_masked(uint32_t n_inputs, uint32_t n_planes, const uint32_t *node_kind,
                                    const uint32_t *node_start, const uint32_t *term_ref, const int32_t *term_shift,
                                    const int32_t *term_weight, const uint32_t *node_table, size_t n_gates,
                                    const uint32_t *outputs, const int32_t *out_shift, size_t n_outputs, uint32_t group,
                                    uint32_t n_regs, const uint32_t *next_ref, const int32_t *next_shift,
                                    const uint32_t *reg_scale, uint32_t n_routes, const int32_t *routes,
                                    const uint32_t *term_route, const uint32_t *out_route, const uint32_t *next_route,
                                    uint32_t n_masks, const uint8_t *masks, const uint32_t *node_mask,
                                    sgfhe_circuit **out) {
    const CircuitNodes N = circuit_nodes_csr(5, node_kind, node_start, term_ref, term_shift, term_weight, node_table, n_planes);
    CircuitSpec S = circuit_spec(n_inputs, N, n_gates, outputs, out_shift, n_outputs, group);
    S.regs.n_regs = n_regs, S.regs.next_ref = next_ref, S.regs.next_shift = next_shift, S.regs.reg_scale = reg_scale;
    S.routes.n_routes = n_routes, S.routes.routes = routes;
    S.routes.term_route = term_route, S.routes.out_route = out_route, S.routes.next_route = next_route;
    S.masks.n_masks = n_masks, S.masks.masks = masks, S.masks.node_mask = node_mask;
    return circuit_create(S, out);
}

int32_t sgfhe_circuit_masks(const sgfhe_circuit *c, uint32_t *n_masks, uint64_t *rows_per_group) {
    if (!c || !n_masks || !rows_per_group) return SGFHE_ERR_INVALID_ARG;
    *n_masks = c->plan.n_masks;
    *rows_per_group = c->plan.rows_per_group;
    return SGFHE_OK;
}

int32_t sgfhe_circuit_routes(const sgfhe_circuit *c, uint32_t *n_routes) {
    if (!c || !n_routes) return SGFHE_ERR_INVALID_ARG;
    *n_routes = c->plan.n_routes;
    return SGFHE_OK;
}

int32_t sgfhe_circuit_registers(const sgfhe_circuit *c, uint32_t *n_regs) {
    if (!c || !n_regs) return SGFHE_ERR_INVALID_ARG;
    *n_regs = c->plan.n_regs;
    return SGFHE_OK;
}

int32_t sgfhe_circuit_planes(const sgfhe_circuit *c, uint32_t *n_planes) {
    if (!c || !n_planes) return SGFHE_ERR_INVALID_ARG;
    *n_planes = c->plan.n_planes;
    return SGFHE_OK;
}

int32_t sgfhe_circuit_create(uint32_t n_inputs, const uint32_t *gates, size_t n_gates, const uint32_t *outputs,
                             size_t n_outputs, sgfhe_circuit **out) {
    return sgfhe_circuit_create_lanes(n_inputs, gates, nullptr, n_gates, outputs, nullptr, n_outputs, 1u, out);
}

int32_t sgfhe_circuit_group(const sgfhe_circuit *c, uint32_t *group) {
    if (!c || !group) return SGFHE_ERR_INVALID_ARG;
    *group = c->plan.group;
    return SGFHE_OK;
}

int32_t sgfhe_circuit_info(const sgfhe_circuit *c, uint64_t info[4]) {
    if (!c || !info) return SGFHE_ERR_INVALID_ARG;
    info[0] = c->plan.levels;
    info[1] = c->plan.live();
    info[2] = c->plan.widest;
    info[3] = c->plan.slots;
    return SGFHE_OK;
}

int32_t sgfhe_circuit_destroy(sgfhe_circuit *c) {
    delete c;
    return SGFHE_OK;
}

// ---- noise probe: LWE error statistics against the secret key, on the device -------------

static constexpr uint32_t NOISE_Q_GRID = 1024;   // workgroups (partial records) of k_lwe_noise_q

// noise_tab: [wires][8] records | [NOISE_Q_GRID][8] partial records | key mask | [wires][bit_words] plaintext bits
struct NoiseLayout {
    uint64_t *stats, *partial, *mask, *bits;
};
static NoiseLayout noise_layout(sgfhe_ctx *c, size_t wires) {
    uint64_t *p = c->noise_tab.p;
    return {p, p + wires * 8, p + wires * 8 + (size_t)NOISE_Q_GRID * 8, p + wires * 8 + (size_t)NOISE_Q_GRID * 8 + NOISE_MASK_WORDS};
}
static int32_t noise_grow(sgfhe_ctx *c, size_t wires, size_t bit_words, size_t lwe_words) {
    int32_t rc = circ_grow(c, c->noise_tab, wires * 8 + (size_t)NOISE_Q_GRID * 8 + NOISE_MASK_WORDS + wires * bit_words);
    return rc ? rc : circ_grow(c, c->noise_lwe, lwe_words);
}
// host image of [key mask | bit table]: bit l of mask word j is the key bit s[64 j + l] (k_lwe_noise's lane order)
static void noise_key_mask(const sgfhe_ctx *c, const uint64_t *sk, uint64_t *mask) {
    std::fill(mask, mask + NOISE_MASK_WORDS, 0ull);
    for (uint32_t i = 0; i < c->n; i++) mask[i / 64] |= (sk[i] & 1ull) << (i % 64);
}
static uint32_t noise_tiles(uint64_t instances) { return (uint32_t)((instances + NOISE_ROWS - 1) / NOISE_ROWS); }

// The geometries in use (kernels.h, NoiseGeom).  `count` compact rows of n + 1 words, all of one wire, whose record and
// row of the bit table is `wire`; the plain rows of sgfhe_lwe_noise are wire 0 of a table of one row
static NoiseGeom noise_wire_rows(size_t n, uint32_t wire, uint32_t count, size_t bit_words) {
    NoiseGeom G = {};
    G.row_stride = n + 1;
    G.wire0 = wire;
    G.rows = G.instances = count;
    G.tiles = noise_tiles(count);
    G.bit_words = (uint32_t)bit_words;
    G.n = (uint32_t)n;
    return G;
}
// The result rows [rows][3][n + 1] of the level call `C` that starts at row `row0`: C.kb - C.ka + 1 nodes of three wires.
// A call inside one node: tiles over its rows; a call over several nodes: tiles over every node's instances (a tile
// never straddles two nodes; rows outside the call are skipped)
// (`kinds`: the device node kinds from node C.ka on when the call holds a LUT node, whose wires have their own codewords)
static NoiseGeom noise_call_rows(size_t n, uint32_t n_inputs, const CircuitCall &C, uint64_t row0, uint32_t inst,
                                 size_t bit_words, const uint32_t *kinds) {
    const bool one = C.ka == C.kb;
    NoiseGeom G = noise_wire_rows(n, (uint32_t)(n_inputs + 3 * (size_t)C.ka), C.rows, bit_words);
    G.row_stride = 3 * (n + 1);
    G.gate_stride = n + 1;
    G.node0 = C.ka - C.k0;
    G.row0 = (uint32_t)row0;
    G.instances = inst;
    G.inst0 = one ? (uint32_t)(row0 - (uint64_t)G.node0 * inst) : 0u;
    G.tiles = noise_tiles(one ? C.rows : inst);
    G.kind = C.lut ? kinds : nullptr;
    return G;
}
// k_lwe_noise over `nodes` nodes of `gates` wires each, into the records NL.stats
static int32_t launch_lwe_noise(sgfhe_ctx *c, hipStream_t st, const uint64_t *rows, const NoiseLayout &NL,
                                const NoiseGeom &G, uint32_t nodes = 1, uint32_t gates = 1) {
    hipLaunchKernelGGL(k_lwe_noise, dim3(nodes * G.tiles, gates), dim3(64 * NOISE_WAVES), 0, st, rows, NL.mask, NL.bits,
                       (unsigned long long *)NL.stats, G, (uint32_t)cur(c).h_crt.logr);
    HIPCHK(c, hipGetLastError());
    return SGFHE_OK;
}

// One run: what its stages share, and the stages in the order run() queues them on `st`.  Which rows, nodes, jobs and
// ciphertexts a call covers is csrc/circuit.h's (circuit_level_call, circuit_pack_runs, circuit_run_sizes), and so is
// what the caller passed: the stages read the request `q` (CircuitRequest), which circuit_request_check has passed for
// `instances`.  The probe (LWE form only) takes the noise records of every input wire and of every live node's three
// wires from the uploaded inputs and from each level call's own result rows.
struct CircuitRun {
    sgfhe_ctx *c;
    const CircuitPlan &P;
    const CircuitRequest &q;
    const size_t instances;
    uint64_t *const out = q.out;
    const uint8_t *const data = P.n_planes ? q.data : nullptr;   // uploaded with the tables, or -- stepped -- with every step
    // The device-resident form (sgfhe_circuit_run*_device): every array of the caller's (but q.emit) is device
    // memory, the run is queued on the caller's stream between fence_begin and fence_end, and the host waits for
    // nothing.  The host form: the ctx's own stream, drained before the run (run_drained) and waited for at its end.
    const bool device = q.device;
    const hipStream_t st = device && q.stream ? (hipStream_t)q.stream : c->stream;
    const size_t n = c->n, row = n + 1, M = c->M;   // row: words of an LWE
    const uint32_t inst = (uint32_t)instances;
    const uint64_t r = c->par.r;
    // SGFHE_CIRCUIT_PACK_DIRECT: the outputs that name a gate wire are the plan's jobs, and their rows go from the level
    // calls into the raw table.  SGFHE_CIRCUIT_PACK_LIFT: every other ciphertext is lifted from the wire table into the
    // raw table (k_circ_lift), so no group has a refreshed one
    const bool pack = q.packs(), direct = pack && q.direct(), lift = direct && q.lift();
    const CircuitRunSizes sz = circuit_run_sizes(P, instances, n, q.ct ? q.count : 0, pack, direct, lift);
    // (a stepped run splits the registers' ciphertexts and a step's stream ciphertexts in turn through the one buffer)
    const size_t ct_words = q.ct ? (size_t)P.n_inputs * q.count * q.N : 0;
    const size_t probe_rows = q.probe ? circuit_probe_rows(P) : 0, bit_words = circuit_bit_words(instances);
    // the plan's tables on the device (views into circ_tab), and the probe's
    CircNodes nodes = {};
    CircRefs outs = {}, nexts = {};   // the outputs; the registers' next states (a plan with registers)
    const uint32_t *d_out_slot = nullptr, *d_in_slot = nullptr, *d_jobs = nullptr;
    const uint32_t *d_fam_start = nullptr, *d_fam_entry = nullptr;   // (a plan with live siblings)
    const uint32_t *d_next_scale = nullptr, *d_reg_index = nullptr;   // (a plan with registers)
    NoiseLayout NL = {};
    std::vector<CircuitPackRun> runs;   // of the pack group at hand (reserved with the buffers)
    // the probe's host images, which the run's asynchronous copies read and write: [key mask | bit table]; the records
    // by probe row
    std::vector<uint64_t> up, down;
    // a scripted run (sgfhe_debug_circuit_script): where the next scripted call, and the next group's tail rows, lie in
    // the script's arrays -- words of `results`, rows of the two logs, ciphertexts of `tail_in`
    size_t script_words = 0, script_rows = 0, script_cts = 0;

    CircuitRun(sgfhe_ctx *c, const CircuitPlan &P, const CircuitRequest &q, size_t instances)
        : c(c), P(P), q(q), instances(instances) {}

    int32_t grow();
    int32_t upload_tables();
    int32_t upload_ct();
    int32_t upload_lwe();
    int32_t level_call(uint32_t L, uint64_t row0);
    int32_t pack_group(size_t q0);
    int32_t script_call(const Staging &S, size_t rows, bool raw, const uint32_t *lutw, uint64_t *res);
    int32_t script_tail(const ulonglong2 *raw, size_t rstride, size_t cnt);
    // every level L = 1 .. levels in calls of SGFHE_CIRCUIT_CALL_ROWS rows from row 0; then every pack group from
    // ciphertext 0: the walk that numbers a run's calls (csrc/circuit.h)
    int32_t level_calls() {
        for (uint32_t L = 1; L <= P.levels; L++) {
            if (const int32_t rc = mask_fill(L)) return rc;
            for (uint64_t row0 = 0; row0 < P.level_rows(L, instances); row0 += SGFHE_CIRCUIT_CALL_ROWS)
                if (const int32_t rc = level_call(L, row0)) return rc;
        }
        return SGFHE_OK;
    }
    // A plan with lane masks: the pairs of level L on the device (views into circ_tab; none in a plan without masks,
    // whose kernels then decode a row as they always did), and the level's fill -- the off lanes of its masked nodes as
    // zeros, once per level and step, before the level's first call (k_circ_mask_fill says why any place in the level
    // would do)
    CircPairs level_pairs(uint32_t L) const {
        if (!P.masked()) return {};
        const uint32_t *tab = c->circ_tab.p;
        return {tab + P.at.pair_node + P.pair_start[L], tab + P.at.pair_lane + P.pair_start[L], inst / P.group, P.group};
    }
    int32_t mask_fill(uint32_t L) {
        if (!P.masked() || P.off_start[L + 1] == P.off_start[L]) return SGFHE_OK;
        const uint32_t *tab = c->circ_tab.p;
        const uint32_t n_off = P.off_start[L + 1] - P.off_start[L], per = inst / P.group;
        hipLaunchKernelGGL(k_circ_mask_fill, dim3(copy_grid((size_t)n_off * 3 * per * row)), dim3(256), 0, st,
                           c->circ_wires.p, d_out_slot + 3 * (size_t)P.level_start[L], tab + P.at.off_node + P.off_start[L],
                           tab + P.at.off_lane + P.off_start[L], n_off, per, P.group, inst, (uint32_t)n);
        HIPCHK(c, hipGetLastError());
        return SGFHE_OK;
    }
    int32_t pack_groups() {
        for (size_t q0 = 0; q0 < sz.n_ct; q0 += sz.cpc)
            if (const int32_t rc = pack_group(q0)) return rc;
        return SGFHE_OK;
    }
    int32_t fetch(uint64_t *o, uint64_t *w, uint64_t *v);
    int32_t download();
    // The caller's arrays, one helper per direction, so that the stages read the same in both forms: `src` into a ctx
    // buffer, a ctx buffer into `dst`, queued on `st` (host form: from and to host memory; device form: device to device)
    int32_t copy_in(void *d_dst, const void *src, size_t bytes) {
        HIPCHK(c, hipMemcpyAsync(d_dst, src, bytes, device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
        return SGFHE_OK;
    }
    int32_t copy_out(void *dst, const void *d_src, size_t bytes) {
        HIPCHK(c, hipMemcpyAsync(dst, d_src, bytes, device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st));
        return SGFHE_OK;
    }
    // the end of a run that has queued everything: the host form waits for it, the device form leaves it in flight
    int32_t finish() {
        if (device) return fence_end(c, st);
        HIPCHK(c, hipStreamSynchronize(st));
        c->pending = false;
        return SGFHE_OK;
    }
    int32_t run();
    // a stepped run
    int32_t upload_state();
    int32_t upload_step(size_t s);
    int32_t feedback();
    int32_t run_steps();
    int32_t split(const uint64_t *a, const uint64_t *b, uint32_t count, const uint32_t *slot, uint64_t *rows);
    int32_t copy_inputs(uint32_t first, const uint64_t *src);
    size_t state_words() const { return (size_t)P.n_regs * instances * row; }
    static uint32_t copy_grid(size_t total) { return (uint32_t)std::min<size_t>((total + 255) / 256, (size_t)1 << 20); }
    // the gather of one call: rows row0 .. row0 + rows of the level whose first node is `node0` of the plan's node table
    // (a level's first node, or live() for the pack stage's pseudo-level)
    // `lutw`: the call's LUT descriptor, for a level call that holds a LUT node (NULL otherwise)
    // `X`: the level's pairs in a plan with lane masks (level_pairs; the pack stage's pseudo-level has none)
    void gather(uint32_t node0, const Staging &S, size_t row0, size_t rows, uint32_t *lutw, CircPairs X = {}) const {
        hipLaunchKernelGGL(k_circ_gather, dim3(((uint32_t)rows * (uint32_t)row + 255) / 256), dim3(256), 0, st,
                           c->circ_wires.p, nodes, node0, S.a1, S.b1, S.a2, S.b2, (uint32_t)row0, (uint32_t)rows, inst,
                           (uint32_t)n, r, lutw, (const uint8_t *)(data ? c->circ_data.p : nullptr), X);
    }
    // a reference list of the uploaded image, from its offsets (`route` is read only in a plan with route tables)
    CircRefs refs_at(uint32_t ref, uint32_t shift, uint32_t route) const {
        const uint32_t *tab = c->circ_tab.p;
        return {tab + ref, reinterpret_cast<const int32_t *>(tab + shift), P.n_routes ? tab + route : nullptr,
                P.n_routes ? reinterpret_cast<const int32_t *>(tab + P.at.routes) : nullptr, P.group};
    }
    // words of the staging's rows (a direct run's level calls may leave un-reduced rows: 16-byte residues, at an even
    // word offset); the LUT descriptor of a call lies behind them, one 32-bit word per row
    size_t stage_words() const { return (size_t)sz.max_rows * (direct ? 8 : 5) * row; }
    bool has_lut() const { return P.lut_before[P.live()] != 0; }
};

// every buffer before anything is queued (host form: a regrown buffer waits for nothing, drained by the caller; device
// form: circ_grow and ensure_work wait for the ctx's queued work where a buffer grows, and nowhere else), and the
// probe's host images.  The device form stages neither the collected outputs nor the ciphertexts: the kernels write
// and read the caller's arrays in place.
int32_t CircuitRun::grow() {
    int32_t rc;
    if ((rc = circ_grow(c, c->circ_wires, (size_t)P.slots * instances * row))) return rc;
    if ((rc = circ_grow(c, c->circ_stage, stage_words() + (has_lut() ? ((size_t)sz.max_rows + 1) / 2 : 0)))) return rc;
    if (direct && (rc = circ_grow(c, c->circ_raw, sz.n_ct * n * row))) return rc;
    if (out && !device && (rc = circ_grow(c, c->circ_out, (size_t)P.n_outputs * instances * row))) return rc;
    if ((rc = circ_grow(c, c->circ_tab, P.at.words))) return rc;
    if (data && (rc = circ_grow(c, c->circ_data, (size_t)P.n_planes * instances))) return rc;
    if (!device && (rc = circ_grow(c, c->circ_ct, 2 * ct_words))) return rc;
    if (q.stepped && (rc = circ_grow(c, c->circ_state, state_words()))) return rc;
    if (pack && (rc = pack_grow(c, sz.cpc, sz.n_ct, sz.max_ref))) return rc;
    if (q.probe) {
        size_t unread = 0;   // inputs nothing reads have no slot: the probe uploads them for itself
        for (uint32_t i = 0; i < P.n_inputs; i++) unread += P.input_slot[i] == CIRC_NONE;
        if ((rc = noise_grow(c, probe_rows, bit_words, unread * instances * row))) return rc;
        std::vector<uint64_t> table;
        if ((rc = circuit_plain_bits(P, q.in_bits, instances, table, data)))
            return fail(c, rc, "sgfhe_circuit_run_probe: no memory for the plaintext bit table");
        try {
            up.assign(NOISE_MASK_WORDS, 0);
            up.insert(up.end(), table.begin(), table.end());
            down.assign(probe_rows * 8, 0);
        } catch (...) {
            return fail(c, SGFHE_ERR_OOM, "sgfhe_circuit_run_probe: no memory for the plaintext bit table");
        }
        noise_key_mask(c, q.sk, up.data());
        NL = noise_layout(c, probe_rows);
    }
    try {
        runs.reserve(sz.cpc);   // (no pack group allocates)
    } catch (...) {
        return fail(c, SGFHE_ERR_OOM, "sgfhe_circuit_run_ct: no memory for the runs of a pack group");
    }
    if (sz.work_rows) {   // the lanes' work buffers for the largest chunk of any call (bootstrap_device's ensure_work is
                          // then a no-op and never waits on the host between levels)
        if ((rc = ensure_work(c, max_chunk_rows(chunk_policy(c, flatten_mode(c)), sz.work_rows)))) return rc;
    }
    return SGFHE_OK;
}

// the plan's tables (the image outlives the asynchronous copy: it belongs to the circuit), the run's planes (the
// caller's array, as the inputs are), and the probe's
int32_t CircuitRun::upload_tables() {
    HIPCHK(c, hipMemcpyAsync(c->circ_tab.p, P.image.data(), (size_t)P.at.words * 4, hipMemcpyHostToDevice, st));
    if (data && !q.stepped)   // (a stepped run brings planes with every step: upload_step)
        if (const int32_t rc = copy_in(c->circ_data.p, data, (size_t)P.n_planes * instances)) return rc;
    const uint32_t *tab = c->circ_tab.p;
    nodes = {tab + P.at.node_kind, tab + P.at.term_start, reinterpret_cast<const int32_t *>(tab + P.at.term_weight),
             refs_at(P.at.term_ref, P.at.term_shift, P.at.term_route)};
    outs = refs_at(P.at.out_ref, P.at.out_shift, P.at.out_route);
    d_out_slot = tab + P.at.out_slot, d_in_slot = tab + P.at.input_slot, d_jobs = tab + P.at.jobs;
    if (P.siblings()) d_fam_start = tab + P.at.fam_start, d_fam_entry = tab + P.at.fam_entry;
    if (P.n_regs) {
        nexts = refs_at(P.at.next_ref, P.at.next_shift, P.at.next_route);
        d_next_scale = tab + P.at.next_scale, d_reg_index = tab + P.at.reg_index;
    }
    if (q.probe) {   // (mask and bit table are adjacent in noise_tab: one copy)
        HIPCHK(c, hipMemcpyAsync(NL.mask, up.data(), up.size() * 8, hipMemcpyHostToDevice, st));
        if (probe_rows) HIPCHK(c, hipMemsetAsync(NL.stats, 0, probe_rows * 64, st));
    }
    return SGFHE_OK;
}

// ciphertext form: the ciphertexts as they are, and extract() of every bit into the slot of its input wire
int32_t CircuitRun::upload_ct() { return split(q.in_a, q.in_b, P.n_inputs, d_in_slot, c->circ_wires.p); }

// `count` wires of ciphertexts a, b [count][blocks][N] (the caller's) split into the slots slot[0 .. count) (device) of
// `rows` ([slot][instances][n + 1]): uploaded into circ_ct first, or -- device form -- read where they are
int32_t CircuitRun::split(const uint64_t *a, const uint64_t *b, uint32_t count, const uint32_t *slot, uint64_t *rows) {
    if (!count) return SGFHE_OK;
    const size_t words = (size_t)count * q.count * q.N;
    if (!device) {
        int32_t rc;
        if ((rc = copy_in(c->circ_ct.p, a, words * 8))) return rc;
        if ((rc = copy_in(c->circ_ct.p + words, b, words * 8))) return rc;
        a = c->circ_ct.p, b = c->circ_ct.p + words;
    }
    const uint32_t tiles = (uint32_t)((n + CIRC_SPLIT_ROWS - 1) / CIRC_SPLIT_ROWS);
    hipLaunchKernelGGL(k_circ_split, dim3((uint32_t)(count * q.count * tiles)), dim3(256),
                       (n + CIRC_SPLIT_ROWS - 1) * 8, st, a, b, slot, rows,
                       (uint32_t)q.count, (uint32_t)q.N, (uint32_t)n, r);
    HIPCHK(c, hipGetLastError());
    return SGFHE_OK;
}

// LWE form: inputs straight into their slots; runs of consecutive inputs in consecutive slots as one copy
int32_t CircuitRun::copy_inputs(uint32_t first, const uint64_t *src) {   // input wires first .. n_inputs, src[0] the first
    const size_t in_words = instances * row;
    for (uint32_t i = first; i < P.n_inputs;) {
        if (P.input_slot[i] == CIRC_NONE) { i++; continue; }
        uint32_t k = i + 1;
        while (k < P.n_inputs && P.input_slot[k] == P.input_slot[k - 1] + 1) k++;
        if (const int32_t rc = copy_in(c->circ_wires.p + (size_t)P.input_slot[i] * in_words,
                                       src + (size_t)(i - first) * in_words, (size_t)(k - i) * in_words * 8))
            return rc;
        i = k;
    }
    return SGFHE_OK;
}

int32_t CircuitRun::upload_lwe() {
    const size_t in_words = instances * row;
    if (const int32_t rc = copy_inputs(0, q.in)) return rc;
    // the probe of the input wires, from the rows as uploaded (before a level reuses a slot)
    for (uint32_t i = 0, u = 0; q.probe && i < P.n_inputs; i++) {
        const bool own = P.input_slot[i] == CIRC_NONE;
        uint64_t *rows_i = own ? c->noise_lwe.p + (size_t)u++ * in_words : c->circ_wires.p + (size_t)P.input_slot[i] * in_words;
        if (own) HIPCHK(c, hipMemcpyAsync(rows_i, q.in + (size_t)i * in_words, in_words * 8, hipMemcpyHostToDevice, st));
        const int32_t rc = launch_lwe_noise(c, st, rows_i, NL, noise_wire_rows(n, i, inst, bit_words));
        if (rc) return rc;
    }
    return SGFHE_OK;
}

// A scripted call (sgfhe_debug_circuit_script) in place of bootstrap_device: the staged rows of the call -- and its LUT
// descriptor `lutw`, if it carries one -- go to the script's logs, and the script's result rows of the call into `res`,
// reduced words or -- `raw` -- 16-byte residues, as the real call would leave them there
int32_t CircuitRun::script_call(const Staging &S, size_t rows, bool raw, const uint32_t *lutw, uint64_t *res) {
    const CircuitScript &X = *q.script;
    uint64_t *log = X.staged + script_rows * 2 * row;   // [rows][2][n + 1]: (a1, b1), (a2, b2)
    const size_t pitch = 2 * row * 8;
    HIPCHK(c, hipMemcpy2DAsync(log, pitch, S.a1, n * 8, n * 8, rows, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpy2DAsync(log + n, pitch, S.b1, 8, 8, rows, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpy2DAsync(log + row, pitch, S.a2, n * 8, n * 8, rows, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpy2DAsync(log + row + n, pitch, S.b2, 8, 8, rows, hipMemcpyDeviceToHost, st));
    if (lutw) HIPCHK(c, hipMemcpyAsync(X.lut + script_rows, lutw, rows * 4, hipMemcpyDeviceToHost, st));
    const size_t words = rows * 3 * row * (raw ? 2 : 1);
    HIPCHK(c, hipMemcpyAsync(res, X.results + script_words, words * 8, hipMemcpyHostToDevice, st));
    script_rows += rows, script_words += words;
    return SGFHE_OK;
}

// ... and in place of pack_tail: the `cnt` * n rows the tail would read, n + 1 residues each at raw + row * rstride,
// into the script's tail_in
int32_t CircuitRun::script_tail(const ulonglong2 *raw, size_t rstride, size_t cnt) {
    HIPCHK(c, hipMemcpy2DAsync(q.script->tail_in + script_cts * n * row * 2, row * 16, raw, rstride * 16, row * 16, cnt * n,
                               hipMemcpyDeviceToHost, st));
    script_cts += cnt;
    return SGFHE_OK;
}

// One level call: gather, the k-loop of sgfhe_bootstrap_batch_device (the next call number of the ctx's draw stream),
// scatter.  In a direct run, a call that produces a wire some direct output names leaves its rows un-reduced: the
// scatter reduces what the wire table takes (the words k_final writes) and copies the named rows into the raw table.
int32_t CircuitRun::level_call(uint32_t L, uint64_t row0) {
    const CircuitCall C = circuit_level_call(P, L, row0, instances);
    const Staging S = staging(c->circ_stage.p, sz.max_rows, n);
    const uint32_t *out_slot = d_out_slot + 3 * (size_t)C.k0, *kind = nodes.kind + C.k0;
    const uint32_t un = (uint32_t)n, r0 = (uint32_t)row0;
    const bool raw = direct && C.j1 > C.j0;
    const CircPairs X = level_pairs(L);
    // a call that holds a LUT node: its rows start at amplitude A0 and leave through k_final_lut (LutDesc)
    LutDesc lut = {reinterpret_cast<uint32_t *>(c->circ_stage.p + stage_words()), false};
    if (C.fam) {   // ... and the live siblings of its LUT nodes leave through k_final_lut_multi, into the wire table
        lut.wires = c->circ_wires.p;
        lut.fam.start = d_fam_start, lut.fam.entry = d_fam_entry;
        lut.fam.node0 = C.k0, lut.fam.row0 = r0, lut.fam.instances = inst;
        lut.fam.data = data ? c->circ_data.p : nullptr;
        lut.fam.pairs = X;
    }
    gather(C.k0, S, row0, C.rows, C.lut ? const_cast<uint32_t *>(lut.rows) : nullptr, X);
    HIPCHK(c, hipGetLastError());
    BootCall call(c);
    call.rows = S, call.batch = C.rows, call.out = S.res, call.st = st;
    if (raw) call.flags = SGFHE_FLAG_RAW_MODQ;
    if (C.lut) call.lut = &lut;
    int32_t rc = q.script ? script_call(S, C.rows, raw, C.lut ? lut.rows : nullptr, S.res) : bootstrap_device(c, call);
    if (rc) return rc;
    if (raw) {
        const ulonglong2 *res = reinterpret_cast<const ulonglong2 *>(S.res);
        for (size_t j = C.j0; j < C.j1;) {
            const CircuitJobChunk ch = circuit_job_chunk(j, C.j0, C.j1);
            hipLaunchKernelGGL(k_circ_scatter_raw, dim3(C.rows, ch.nj + ch.wires), dim3(256), 0, st, res, out_slot,
                               c->circ_wires.p, d_jobs + 3 * j, c->circ_raw.p, cur(c).d_crt, r0, inst, un, ch.wires, X);
            HIPCHK(c, hipGetLastError());
            j += ch.nj;
        }
        if (C.sum) {   // a sum node's LOW rows, from the staging the bootstrap consumed (after the scatter: over the XOR
                       // row's words in the wire table)
            hipLaunchKernelGGL(k_circ_xor3_raw, dim3(C.rows), dim3(256), 0, st, res, kind, out_slot, c->circ_wires.p,
                               S.a1, S.b1, S.a2, S.b2, cur(c).d_crt, r0, inst, un, r, X);
            HIPCHK(c, hipGetLastError());
        }
        return SGFHE_OK;
    }
    const uint32_t tg = C.rows * (uint32_t)row;
    if (C.sum) {   // (before the scatter and the probe read the result rows)
        hipLaunchKernelGGL(k_circ_xor3, dim3((tg + 255) / 256), dim3(256), 0, st, S.res, kind, S.a1, S.b1, S.a2, S.b2, r0,
                           C.rows, inst, un, r, X);
        HIPCHK(c, hipGetLastError());
    }
    hipLaunchKernelGGL(k_circ_scatter, dim3((3 * tg + 255) / 256), dim3(256), 0, st, S.res, out_slot, c->circ_wires.p, r0,
                       C.rows, inst, un, X);
    HIPCHK(c, hipGetLastError());
    // the probe: the call's own result rows, read or not, before the next call overwrites them (same stream)
    if (!q.probe) return SGFHE_OK;
    rc = launch_lwe_noise(c, st, S.res, NL, noise_call_rows(n, P.n_inputs, C, row0, inst, bit_words, nodes.kind + C.ka),
                          C.kb - C.ka + 1, 3);
    // a sibling has no result rows: the wires of it that have a slot are measured there, over the instances of its
    // leader that this call holds, each against its own codeword
    for (uint32_t k = C.ka; !rc && C.fam && k <= C.kb; k++) {
        const uint64_t lo = std::max<uint64_t>(row0, (uint64_t)(k - C.k0) * inst);
        const uint64_t hi = std::min<uint64_t>(row0 + C.rows, (uint64_t)(k - C.k0 + 1) * inst);
        const uint32_t i0 = (uint32_t)(lo - (uint64_t)(k - C.k0) * inst), cnt = (uint32_t)(hi - lo);
        for (uint32_t i = P.fam_start[k]; !rc && i < P.fam_start[k + 1]; i++)
            for (uint32_t w = 0; !rc && w < 3; w++) {
                const uint32_t slot = P.fam_entry[4 * i + 1 + w];
                if (slot == CIRC_NONE) continue;
                NoiseGeom G = noise_wire_rows(n, (uint32_t)(P.n_inputs + 3 * (P.live() + i) + w), cnt, bit_words);
                G.instances = inst;
                G.inst0 = G.row0 = i0;
                G.scale = w;
                rc = launch_lwe_noise(c, st, c->circ_wires.p + ((size_t)slot * inst + i0) * row, NL, G);
            }
    }
    return rc;
}

// One pack group: ciphertexts q0 .. q0 + cnt are rows q0 * n .. of the "level" whose node o is (TRUE, output o) --
// row = o * instances + block * n + bit -- so the gather of the levels builds their bootstrap inputs.  The group's
// runs (every ciphertext in the plain form, those that are not direct otherwise) are lifted into the raw table -- one
// k_circ_lift per run, straight from the wire table -- or gathered (row = rank among them * n + bit) and bootstrapped
// un-reduced as ONE call.  Then the tail.  Direct: the AND rows join the direct ones in the raw table, and the tail
// over the group's rows of that table is a call of its own, so a group is an optional sgfhe_bootstrap_batch(RAW_MODQ)
// plus one sgfhe_pack_lwe_modq on the draw stream.  Plain: the tail reads gate 0 of the bootstrap's result under the
// bootstrap's own call number, which is one sgfhe_pack_encrypted_bits(count = cnt).
int32_t CircuitRun::pack_group(size_t q0) {
    const size_t cnt = std::min(sz.cpc, sz.n_ct - q0);
    const size_t nb = circuit_pack_runs(P, q.count, q0, cnt, !direct, &runs) * n;
    if (lift) {
        for (const CircuitPackRun &U : runs) {
            const uint32_t rows = (uint32_t)(U.len * n);
            hipLaunchKernelGGL(k_circ_lift, dim3((rows * (uint32_t)row + 255) / 256), dim3(256), 0, st, c->circ_wires.p,
                               outs, c->circ_raw.p, cur(c).d_crt, (uint32_t)(U.q * n), rows, inst, (uint32_t)n, r);
            HIPCHK(c, hipGetLastError());
        }
    } else if (nb) {
        const Staging S = staging(c->pack_lwe.p, nb, n);
        for (const CircuitPackRun &U : runs) {
            gather((uint32_t)P.live(), S.from_row(U.rank * n, n), U.q * n, U.len * n, nullptr);
            HIPCHK(c, hipGetLastError());
        }
        BootCall call(c);
        call.rows = S, call.batch = nb, call.out = (uint64_t *)c->pack_raw.p, call.flags = SGFHE_FLAG_RAW_MODQ, call.st = st;
        const int32_t rc = q.script ? script_call(S, nb, true, nullptr, call.out) : bootstrap_device(c, call);
        if (rc) return rc;
        for (size_t i = 0; direct && i < runs.size(); i++) {
            const CircuitPackRun &U = runs[i];
            hipLaunchKernelGGL(k_circ_raw_and, dim3((uint32_t)(U.len * n)), dim3(256), 0, st,
                               c->pack_raw.p + U.rank * n * 3 * row, c->circ_raw.p + U.q * n * row, (uint32_t)n);
            HIPCHK(c, hipGetLastError());
        }
    }
    if (q.script)   // (no tail: no call number is taken)
        return direct ? script_tail(c->circ_raw.p + q0 * n * row, row, cnt) : script_tail(c->pack_raw.p, 3 * row, cnt);
    uint64_t *d_w = c->pack_wv.p + q0 * M, *d_v = c->pack_wv.p + (sz.n_ct + q0) * M;
    if (!direct) return pack_tail(c, c->pack_raw.p, 3 * (uint32_t)row, cnt, d_w, d_v, c->last_call, st);
    const uint32_t call = c->rnd ? c->rnd_call++ : 0u;
    c->last_call = call;
    return pack_tail(c, c->circ_raw.p + q0 * n * row, (uint32_t)row, cnt, d_w, d_v, call, st);
}

// (w, v) of every ciphertext, the outputs in the LWE form, the probe's records; then the host waits (host form)
int32_t CircuitRun::download() {
    int32_t rc;
    if ((rc = fetch(out, q.out_w, q.out_v))) return rc;
    if (probe_rows)
        HIPCHK(c, hipMemcpyAsync(down.data(), NL.stats, probe_rows * 64, hipMemcpyDeviceToHost, st));
    if ((rc = finish())) return rc;
    if (q.probe) {   // records by wire id; the wires of pruned nodes stay zero
        std::fill(q.stats, q.stats + ((size_t)P.n_inputs + 3 * (size_t)P.n_gates) * 8, 0ull);
        for (size_t w = 0; w < probe_rows; w++)
            std::copy(down.begin() + w * 8, down.begin() + w * 8 + 8, q.stats + (size_t)circuit_probe_wire(P, w) * 8);
    }
    return SGFHE_OK;
}

// the outputs of the wire table as it stands, queued: (w, v) of the packed ciphertexts (a run that packs) and the
// collected LWEs (`o` NULL: not wanted), which the device form collects straight into `o`
int32_t CircuitRun::fetch(uint64_t *o, uint64_t *w, uint64_t *v) {
    int32_t rc;
    if (pack && !q.script) {   // (a scripted run has no tail: nothing wrote (w, v))
        const size_t wv = sz.n_ct * M;
        if ((rc = copy_out(w, c->pack_wv.p, wv * 8))) return rc;
        if ((rc = copy_out(v, c->pack_wv.p + wv, wv * 8))) return rc;
    }
    if (o) {
        const size_t total = (size_t)P.n_outputs * instances * row;
        hipLaunchKernelGGL(k_circ_collect, dim3(copy_grid(total)), dim3(256), 0, st, c->circ_wires.p, outs,
                           device ? o : c->circ_out.p, total, inst, (uint32_t)n, r);
        HIPCHK(c, hipGetLastError());
        if (!device && (rc = copy_out(o, c->circ_out.p, total * 8))) return rc;
    }
    return SGFHE_OK;
}

// ---- a stepped run: the stages around the level calls and pack groups of one step ---------------------------------

// the registers' first values into the state buffer: the caller's LWEs, the split of the caller's ciphertexts, or FALSE
int32_t CircuitRun::upload_state() {
    if (!P.n_regs) return SGFHE_OK;
    if (q.state_a) return split(q.state_a, q.state_b, P.n_regs, d_reg_index, c->circ_state.p);
    if (q.state_in)   // (read in full before anything is written: state_out may be this very array)
        return copy_in(c->circ_state.p, q.state_in, state_words() * 8);
    HIPCHK(c, hipMemsetAsync(c->circ_state.p, 0, state_words() * 8, st));
    return SGFHE_OK;
}

// start of step s: the registers into their slots (one launch), the step's stream inputs into theirs, the step's planes
int32_t CircuitRun::upload_step(size_t s) {
    if (P.n_regs) {
        hipLaunchKernelGGL(k_circ_state_load, dim3(copy_grid(state_words())), dim3(256), 0, st, c->circ_state.p, d_in_slot,
                           c->circ_wires.p, state_words(), inst, (uint32_t)n);
        HIPCHK(c, hipGetLastError());
    }
    int32_t rc;
    if (q.ct) {
        const size_t per = (size_t)P.n_stream() * q.count * q.N;
        rc = split(q.in_a + s * per, q.in_b + s * per, P.n_stream(), d_in_slot + P.n_regs, c->circ_wires.p);
    } else {
        rc = copy_inputs(P.n_regs, q.in + s * (size_t)P.n_stream() * instances * row);
    }
    if (rc) return rc;
    if (data) {
        const size_t per = (size_t)P.n_planes * instances;
        return copy_in(c->circ_data.p, data + s * per, per);
    }
    return SGFHE_OK;
}

// end of a step: every register's next state, from the wire table into the state buffer (one launch)
int32_t CircuitRun::feedback() {
    if (!P.n_regs) return SGFHE_OK;
    hipLaunchKernelGGL(k_circ_next, dim3(copy_grid(state_words())), dim3(256), 0, st, c->circ_wires.p, nexts,
                       d_next_scale, c->circ_state.p, state_words(), inst, (uint32_t)n, r);
    HIPCHK(c, hipGetLastError());
    return SGFHE_OK;
}

// Every step is the run() of the step plan: its level calls, then -- an emitted step -- its pack groups and its
// outputs, taken before the feedback.  Everything is queued on the one stream; the host waits once, at the end (host
// form), or not at all.
int32_t CircuitRun::run_steps() {
    int32_t rc;
    if ((rc = grow())) return rc;
    if (device && (rc = fence_begin(c, st))) return rc;
    if ((rc = upload_tables())) return rc;
    if ((rc = upload_state())) return rc;
    const size_t out_words = (size_t)P.n_outputs * instances * row, wv = sz.n_ct * M;
    for (size_t s = 0, emitted = 0; s < q.steps; s++) {
        if ((rc = upload_step(s))) return rc;
        if ((rc = level_calls())) return rc;
        if (!q.emit || q.emit[s]) {
            if ((rc = pack_groups())) return rc;
            if ((rc = fetch(out ? out + emitted * out_words : nullptr, pack ? q.out_w + emitted * wv : nullptr,
                            pack ? q.out_v + emitted * wv : nullptr)))
                return rc;
            emitted++;
        }
        if ((rc = feedback())) return rc;
    }
    if (q.state_out && P.n_regs && (rc = copy_out(q.state_out, c->circ_state.p, state_words() * 8))) return rc;
    return finish();
}

int32_t CircuitRun::run() {
    int32_t rc;
    if (q.stepped) return run_steps();
    if ((rc = grow())) return rc;
    if (device && (rc = fence_begin(c, st))) return rc;   // (after grow: a buffer that grew has drained the ctx)
    if ((rc = upload_tables())) return rc;
    if ((rc = q.ct ? upload_ct() : upload_lwe())) return rc;
    if ((rc = level_calls())) return rc;
    if ((rc = pack_groups())) return rc;
    return download();
}

// The run of an entry whose checks have passed: the host form behind a drained ctx, waited for; the device form
// (`device`, on `st`: sgfhe_circuit_run*_device) queued behind the ctx's work and left in flight
extern "C++" template <class F>
static int32_t circuit_run_form(sgfhe_ctx *c, bool device, hipStream_t st, F &&body) {
    return device ? run_queued(c, st ? st : c->stream, body) : run_drained(c, body);
}

// What sgfhe_debug_circuit_script checks of the script's memory, behind the request's check and before anything is
// queued: every scripted word below r, every scripted residue below Q.  Then the descriptor log is cleared, so that a
// call without a descriptor reads 0 there.
static int32_t script_check(sgfhe_ctx *c, const CircuitPlan &P, const CircuitRequest &q, size_t instances) {
    std::vector<CircuitScriptCall> calls;
    try {
        circuit_script_calls(P, q, c->n, instances, &calls);
    } catch (...) {
        return fail(c, SGFHE_ERR_OOM, "sgfhe_debug_circuit_script: no memory for the list of calls");
    }
    const uint64_t r = c->par.r, Qlo = c->par.Q[0], Qhi = c->par.Q[1];
    const uint64_t *w = q.script->results;
    size_t rows = 0;
    for (const CircuitScriptCall &C : calls) {
        const size_t words = (size_t)C.rows * 3 * (c->n + 1);
        for (size_t i = 0; i < words; i++)
            if (C.raw ? (w[2 * i + 1] > Qhi || (w[2 * i + 1] == Qhi && w[2 * i] >= Qlo)) : w[i] >= r)
                return fail(c, SGFHE_ERR_INVALID_ARG, C.raw ? "sgfhe_debug_circuit_script: a scripted residue is not below Q"
                                                            : "sgfhe_debug_circuit_script: a scripted word is not below r");
        w += words * (C.raw ? 2 : 1), rows += C.rows;
    }
    std::fill(q.script->lut, q.script->lut + rows, 0u);
    return SGFHE_OK;
}

// Every run entry, the ctx locked: the one check of the request (csrc/circuit.h), then the run in the request's form.
// An empty probe run still clears the caller's records.
static int32_t circuit_run(sgfhe_ctx *c, const sgfhe_circuit *circ, const CircuitRequest &q) {
    const CircuitPlan *P = circ ? &circ->plan : nullptr;
    const CircuitEnv env = {c->n, c->M, c->have_key, pack_group(c) != 0,
                            (uint32_t)((c->n + CIRC_SPLIT_ROWS - 1) / CIRC_SPLIT_ROWS)};
    const CircuitVerdict v = circuit_request_check(P, q, env);
    if (v.what == CircuitVerdict::REFUSED) return fail(c, v.code, v.message);
    if (v.what == CircuitVerdict::EMPTY) {
        if (q.probe) std::fill(q.stats, q.stats + ((size_t)P->n_inputs + 3 * (size_t)P->n_gates) * 8, 0ull);
        return SGFHE_OK;
    }
    if (q.script)
        if (const int32_t rc = script_check(c, *P, q, v.instances)) return rc;
    CircuitRun R(c, *P, q, v.instances);   // (outlives the wait that follows a failed step: the probe's host images)
    return circuit_run_form(c, q.device, (hipStream_t)q.stream, [&] { return R.run(); });
}

// everything sgfhe_lwe_noise queues (run_drained waits for the stream when a step fails)
static int32_t lwe_noise_queued(sgfhe_ctx *c, const uint64_t *lwe, size_t count, size_t stride, bool raw,
                                const std::vector<uint64_t> &up, std::vector<uint64_t> &down) {
    const size_t n = c->n, rowlen = (n + 1) * (raw ? 2 : 1);
    hipStream_t st = c->stream;
    const NoiseLayout NL = noise_layout(c, 1);
    HIPCHK(c, hipMemcpyAsync(NL.mask, up.data(), up.size() * 8, hipMemcpyHostToDevice, st));
    // the rows, compact on the device whatever the caller's stride
    if (stride == rowlen) HIPCHK(c, hipMemcpyAsync(c->noise_lwe.p, lwe, count * rowlen * 8, hipMemcpyHostToDevice, st));
    else HIPCHK(c, hipMemcpy2DAsync(c->noise_lwe.p, rowlen * 8, lwe, stride * 8, rowlen * 8, count, hipMemcpyHostToDevice, st));
    const NoiseGeom G = noise_wire_rows(n, 0, (uint32_t)count, circuit_bit_words(count));
    if (raw) {
        const uint32_t grid = std::min(G.tiles, NOISE_Q_GRID);
        hipLaunchKernelGGL(k_lwe_noise_q, dim3(grid), dim3(64 * NOISE_WAVES), 0, st,
                           reinterpret_cast<const ulonglong2 *>(c->noise_lwe.p), NL.mask, NL.bits,
                           (unsigned long long *)NL.partial, cur(c).d_crt, G);
        HIPCHK(c, hipGetLastError());
        down.assign((size_t)grid * 8, 0);
        HIPCHK(c, hipMemcpyAsync(down.data(), NL.partial, down.size() * 8, hipMemcpyDeviceToHost, st));
    } else {
        HIPCHK(c, hipMemsetAsync(NL.stats, 0, 64, st));
        const int32_t rc = launch_lwe_noise(c, st, c->noise_lwe.p, NL, G);
        if (rc) return rc;
        down.assign(8, 0);
        HIPCHK(c, hipMemcpyAsync(down.data(), NL.stats, 64, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(c, hipStreamSynchronize(st));
    return SGFHE_OK;
}

int32_t sgfhe_lwe_noise(sgfhe_ctx *c, const uint64_t *sk, const uint64_t *lwe, size_t count, size_t row_stride_words,
                        const uint8_t *expected, uint32_t flags, uint64_t stats[8]) {
    if (!c) return SGFHE_ERR_INVALID_ARG;
    SGFHE_LOCK(c);
    if (!sk || !stats || (count && (!lwe || !expected)))
        return fail(c, SGFHE_ERR_INVALID_ARG, "sgfhe_lwe_noise: NULL secret key, row, expected-bit or statistics pointer");
    if (flags & ~SGFHE_FLAG_RAW_MODQ) return fail(c, SGFHE_ERR_INVALID_ARG, "sgfhe_lwe_noise: flags are 0 or SGFHE_FLAG_RAW_MODQ");
    const bool raw = (flags & SGFHE_FLAG_RAW_MODQ) != 0;
    const size_t n = c->n, rowlen = (n + 1) * (raw ? 2 : 1);
    if (row_stride_words < rowlen || (raw && (row_stride_words & 1)))
        return fail(c, SGFHE_ERR_INVALID_ARG, "sgfhe_lwe_noise: row_stride_words below the row length (or odd, for rows over Z_Q)");
    if (count > 0xFFFFFFFFull) return fail(c, SGFHE_ERR_INVALID_ARG, "sgfhe_lwe_noise: count must be below 2^32");
    for (size_t i = 0; raw && i < count; i++)
        for (size_t e = 0; e <= n; e++)
            if (ld128(lwe + i * row_stride_words + 2 * e) >= c->Q)
                return fail(c, SGFHE_ERR_INVALID_ARG, "sgfhe_lwe_noise: residue " + std::to_string(e) + " of row " +
                                                          std::to_string(i) + " is not below Q");
    std::fill(stats, stats + 8, 0ull);
    if (count == 0) return SGFHE_OK;
    std::vector<uint64_t> up, down;   // [key mask | expected bits]; the record or the partial records
    const int32_t rc = run_drained(c, [&]() -> int32_t {
        const size_t bit_words = circuit_bit_words(count);
        const int32_t rg = noise_grow(c, 1, bit_words, count * rowlen);
        if (rg) return rg;
        try {
            up.assign(NOISE_MASK_WORDS + bit_words, 0);
        } catch (...) {
            return fail(c, SGFHE_ERR_OOM, "sgfhe_lwe_noise: no memory for the expected-bit table");
        }
        noise_key_mask(c, sk, up.data());
        for (size_t i = 0; i < count; i++) up[NOISE_MASK_WORDS + i / 64] |= (uint64_t)(expected[i] & 1u) << (i % 64);
        try {
            return lwe_noise_queued(c, lwe, count, row_stride_words, raw, up, down);
        } catch (...) {
            return fail(c, SGFHE_ERR_OOM, "sgfhe_lwe_noise: no memory for the partial records");
        }
    });
    if (rc) return rc;
    if (!raw) {
        std::copy(down.begin(), down.end(), stats);
        return SGFHE_OK;
    }
    u128 emax = 0, esum = 0;   // fold the workgroups' partial records (there is no 128-bit atomic)
    for (size_t g = 0; g < down.size() / 8; g++) {
        const uint64_t *rec = down.data() + g * 8;
        stats[0] += rec[0];
        stats[1] += rec[1];
        emax = std::max(emax, ld128(rec + 2));
        esum += ld128(rec + 4);
    }
    stats[2] = (uint64_t)emax, stats[3] = (uint64_t)(emax >> 64);
    stats[4] = (uint64_t)esum, stats[5] = (uint64_t)(esum >> 64);
    return SGFHE_OK;
}

// ---- the run entries (include/sgfhe_hip.h).  Each fills the request of its form (CircuitRequest, csrc/circuit.h) and
// runs it with the ctx locked -- for the whole run, or while a device entry queues -- so that its call numbers are
// contiguous ---------------------------------------------------------------------------------------------------------

int32_t sgfhe_circuit_run(sgfhe_ctx *c, const sgfhe_circuit *circ, size_t instances, const uint64_t *in,
                          uint64_t *out) {
    if (!c) return SGFHE_ERR_INVALID_ARG;
    SGFHE_LOCK(c);
    CircuitRequest q;
    q.count = instances, q.in = in, q.out = out;
    return circuit_run(c, circ, q);
}

int32_t sgfhe_circuit_run_data(sgfhe_ctx *c, const sgfhe_circuit *circ, size_t instances, const uint64_t *in,
                               const uint8_t *data, uint64_t *out) {
    if (!c) return SGFHE_ERR_INVALID_ARG;
    SGFHE_LOCK(c);
    CircuitRequest q;
    q.with_data = true;
    q.count = instances, q.in = in, q.data = data, q.out = out;
    return circuit_run(c, circ, q);
}

int32_t sgfhe_circuit_run_probe(sgfhe_ctx *c, const sgfhe_circuit *circ, size_t instances, const uint64_t *in,
                                uint64_t *out, const uint64_t *sk, const uint8_t *in_bits, uint64_t *stats) {
    if (!c) return SGFHE_ERR_INVALID_ARG;
    SGFHE_LOCK(c);
    CircuitRequest q;
    q.probe = true;
    q.count = instances, q.in = in, q.out = out;
    q.sk = sk, q.in_bits = in_bits, q.stats = stats;
    return circuit_run(c, circ, q);
}

int32_t sgfhe_circuit_run_probe_data(sgfhe_ctx *c, const sgfhe_circuit *circ, size_t instances, const uint64_t *in,
                                     const uint8_t *data, uint64_t *out, const uint64_t *sk, const uint8_t *in_bits,
                                     uint64_t *stats) {
    if (!c) return SGFHE_ERR_INVALID_ARG;
    SGFHE_LOCK(c);
    CircuitRequest q;
    q.probe = q.with_data = true;
    q.count = instances, q.in = in, q.data = data, q.out = out;
    q.sk = sk, q.in_bits = in_bits, q.stats = stats;
    return circuit_run(c, circ, q);
}

int32_t sgfhe_circuit_run_ct(sgfhe_ctx *c, const sgfhe_circuit *circ, size_t blocks, const uint64_t *in_a,
                             const uint64_t *in_b, size_t N, uint64_t *out_w, uint64_t *out_v, uint64_t *out_lwe) {
    if (!c) return SGFHE_ERR_INVALID_ARG;
    SGFHE_LOCK(c);
    CircuitRequest q;
    q.ct = true;
    q.count = blocks, q.in_a = in_a, q.in_b = in_b, q.N = N;
    q.out_w = out_w, q.out_v = out_v, q.out = out_lwe;
    return circuit_run(c, circ, q);
}

int32_t sgfhe_circuit_run_ct_ex(sgfhe_ctx *c, const sgfhe_circuit *circ, size_t blocks, const uint64_t *in_a,
                                const uint64_t *in_b, size_t N, uint64_t *out_w, uint64_t *out_v, uint64_t *out_lwe,
                                uint32_t flags) {
    if (!c) return SGFHE_ERR_INVALID_ARG;
    SGFHE_LOCK(c);
    CircuitRequest q;
    q.ct = true;
    q.count = blocks, q.in_a = in_a, q.in_b = in_b, q.N = N;
    q.out_w = out_w, q.out_v = out_v, q.out = out_lwe, q.flags = flags;
    return circuit_run(c, circ, q);
}

int32_t sgfhe_circuit_run_ct_data(sgfhe_ctx *c, const sgfhe_circuit *circ, size_t blocks, const uint64_t *in_a,
                                  const uint64_t *in_b, size_t N, const uint8_t *data, uint64_t *out_w, uint64_t *out_v,
                                  uint64_t *out_lwe, uint32_t flags) {
    if (!c) return SGFHE_ERR_INVALID_ARG;
    SGFHE_LOCK(c);
    CircuitRequest q;
    q.ct = q.with_data = true;
    q.count = blocks, q.in_a = in_a, q.in_b = in_b, q.N = N, q.data = data;
    q.out_w = out_w, q.out_v = out_v, q.out = out_lwe, q.flags = flags;
    return circuit_run(c, circ, q);
}

int32_t sgfhe_circuit_run_steps(sgfhe_ctx *c, const sgfhe_circuit *circ, size_t instances, size_t steps,
                                const uint64_t *state_in, const uint64_t *in, const uint8_t *data, const uint8_t *emit,
                                uint64_t *out, uint64_t *state_out) {
    if (!c) return SGFHE_ERR_INVALID_ARG;
    SGFHE_LOCK(c);
    CircuitRequest q;
    q.stepped = q.with_data = true;
    q.count = instances, q.steps = steps, q.state_in = state_in, q.in = in, q.data = data, q.emit = emit;
    q.out = out, q.state_out = state_out;
    return circuit_run(c, circ, q);
}

int32_t sgfhe_circuit_run_steps_ct(sgfhe_ctx *c, const sgfhe_circuit *circ, size_t blocks, size_t steps,
                                   const uint64_t *state_a, const uint64_t *state_b, const uint64_t *in_a,
                                   const uint64_t *in_b, size_t N, const uint8_t *data, const uint8_t *emit,
                                   uint64_t *out_w, uint64_t *out_v, uint64_t *out_lwe, uint64_t *state_lwe,
                                   uint32_t flags) {
    if (!c) return SGFHE_ERR_INVALID_ARG;
    SGFHE_LOCK(c);
    CircuitRequest q;
    q.ct = q.stepped = q.with_data = true;
    q.count = blocks, q.steps = steps, q.state_a = state_a, q.state_b = state_b, q.in_a = in_a, q.in_b = in_b, q.N = N;
    q.data = data, q.emit = emit;
    q.out_w = out_w, q.out_v = out_v, q.out = out_lwe, q.state_out = state_lwe, q.flags = flags;
    return circuit_run(c, circ, q);
}

// device-resident runs: the most general host entry of each form, every array (but `emit`) in device memory, the work
// queued on `stream` and left in flight

int32_t sgfhe_circuit_run_device(sgfhe_ctx *c, const sgfhe_circuit *circ, size_t instances, const uint64_t *in,
                                 const uint8_t *data, uint64_t *out, void *stream) {
    if (!c) return SGFHE_ERR_INVALID_ARG;
    SGFHE_LOCK(c);
    CircuitRequest q;
    q.device = q.with_data = true, q.stream = stream;
    q.count = instances, q.in = in, q.data = data, q.out = out;
    return circuit_run(c, circ, q);
}

int32_t sgfhe_circuit_run_ct_device(sgfhe_ctx *c, const sgfhe_circuit *circ, size_t blocks, const uint64_t *in_a,
                                    const uint64_t *in_b, size_t N, const uint8_t *data, uint64_t *out_w, uint64_t *out_v,
                                    uint64_t *out_lwe, uint32_t flags, void *stream) {
    if (!c) return SGFHE_ERR_INVALID_ARG;
    SGFHE_LOCK(c);
    CircuitRequest q;
    q.ct = q.device = q.with_data = true, q.stream = stream;
    q.count = blocks, q.in_a = in_a, q.in_b = in_b, q.N = N, q.data = data;
    q.out_w = out_w, q.out_v = out_v, q.out = out_lwe, q.flags = flags;
    return circuit_run(c, circ, q);
}

int32_t sgfhe_circuit_run_steps_device(sgfhe_ctx *c, const sgfhe_circuit *circ, size_t instances, size_t steps,
                                       const uint64_t *state_in, const uint64_t *in, const uint8_t *data,
                                       const uint8_t *emit, uint64_t *out, uint64_t *state_out, void *stream) {
    if (!c) return SGFHE_ERR_INVALID_ARG;
    SGFHE_LOCK(c);
    CircuitRequest q;
    q.stepped = q.device = q.with_data = true, q.stream = stream;
    q.count = instances, q.steps = steps, q.state_in = state_in, q.in = in, q.data = data, q.emit = emit;
    q.out = out, q.state_out = state_out;
    return circuit_run(c, circ, q);
}

int32_t sgfhe_circuit_run_steps_ct_device(sgfhe_ctx *c, const sgfhe_circuit *circ, size_t blocks, size_t steps,
                                          const uint64_t *state_a, const uint64_t *state_b, const uint64_t *in_a,
                                          const uint64_t *in_b, size_t N, const uint8_t *data, const uint8_t *emit,
                                          uint64_t *out_w, uint64_t *out_v, uint64_t *out_lwe, uint64_t *state_lwe,
                                          uint32_t flags, void *stream) {
    if (!c) return SGFHE_ERR_INVALID_ARG;
    SGFHE_LOCK(c);
    CircuitRequest q;
    q.ct = q.stepped = q.device = q.with_data = true, q.stream = stream;
    q.count = blocks, q.steps = steps, q.state_a = state_a, q.state_b = state_b, q.in_a = in_a, q.in_b = in_b, q.N = N;
    q.data = data, q.emit = emit;
    q.out_w = out_w, q.out_v = out_v, q.out = out_lwe, q.state_out = state_lwe, q.flags = flags;
    return circuit_run(c, circ, q);
}

// ---- the scripted run (a debug hook): the glue of a run with its calls and its tail replaced by the caller's arrays ----

static bool script_form(uint32_t form, CircuitRequest &q) {
    q.ct = form & SGFHE_SCRIPT_CT, q.stepped = (form & SGFHE_SCRIPT_STEPPED) != 0;
    q.probe = (form & SGFHE_SCRIPT_PROBE) != 0, q.device = (form & SGFHE_SCRIPT_DEVICE) != 0;
    q.with_data = true;
    return !(form & ~(SGFHE_SCRIPT_CT | SGFHE_SCRIPT_STEPPED | SGFHE_SCRIPT_PROBE | SGFHE_SCRIPT_DEVICE));
}

int32_t sgfhe_debug_circuit_script(sgfhe_ctx *c, const sgfhe_circuit *circ, uint32_t form, size_t count, size_t steps,
                                   const uint64_t *state_a, const uint64_t *state_b, const uint64_t *in_a,
                                   const uint64_t *in_b, size_t N, const uint8_t *data, const uint8_t *emit, uint64_t *out,
                                   uint64_t *state_out, uint32_t flags, const uint64_t *results, uint64_t *staged,
                                   uint32_t *lut, uint64_t *tail_in) {
    if (!c) return SGFHE_ERR_INVALID_ARG;
    SGFHE_LOCK(c);
    CircuitRequest q;
    CircuitScript X;
    X.results = results, X.staged = staged, X.lut = lut, X.tail_in = tail_in;
    if (!script_form(form, q)) return fail(c, SGFHE_ERR_INVALID_ARG, "sgfhe_debug_circuit_script: unknown form bits");
    q.script = &X;
    q.count = count, q.data = data, q.out = out;
    if (q.stepped) q.steps = steps, q.emit = emit, q.state_out = state_out;
    if (q.ct) q.in_a = in_a, q.in_b = in_b, q.N = N, q.flags = flags;
    else q.in = in_a;
    if (q.stepped && q.ct) q.state_a = state_a, q.state_b = state_b;
    else if (q.stepped) q.state_in = state_a;
    return circuit_run(c, circ, q);
}

int32_t sgfhe_debug_circuit_script_calls(sgfhe_ctx *c, const sgfhe_circuit *circ, uint32_t form, size_t count, size_t steps,
                                         const uint8_t *emit, int pack, uint32_t flags, size_t *n_calls, uint32_t *rows,
                                         uint8_t *raw, size_t cap) {
    if (!c) return SGFHE_ERR_INVALID_ARG;
    SGFHE_LOCK(c);
    CircuitRequest q;
    CircuitScript X;
    uint64_t some = 0;
    if (pack) X.tail_in = &some;   // (read as a flag only)
    if (!script_form(form, q) || q.probe || q.device || !circ || !n_calls || (cap && (!rows || !raw)))
        return fail(c, SGFHE_ERR_INVALID_ARG, "sgfhe_debug_circuit_script_calls: NULL pointer or a form the hook does not run");
    q.script = &X, q.count = count, q.flags = q.ct ? flags : 0u;
    if (q.stepped) q.steps = steps, q.emit = emit;
    const CircuitPlan &P = circ->plan;
    const uint64_t instances = q.ct ? (uint64_t)count * c->n : count;
    if (count >= 0x80000000u || instances >= 0x80000000u || (uint64_t)P.widest * instances > 0xFFFFFFFFull ||
        (uint64_t)P.n_outputs * instances > 0xFFFFFFFFull)
        return fail(c, SGFHE_ERR_INVALID_ARG, "sgfhe_debug_circuit_script_calls: too many instances for this circuit");
    std::vector<CircuitScriptCall> calls;
    try {
        if (count && q.steps) circuit_script_calls(P, q, c->n, instances, &calls);
    } catch (...) {
        return fail(c, SGFHE_ERR_OOM, "sgfhe_debug_circuit_script_calls: no memory for the list of calls");
    }
    *n_calls = calls.size();
    for (size_t i = 0; i < std::min(cap, calls.size()); i++) rows[i] = calls[i].rows, raw[i] = calls[i].raw;
    return SGFHE_OK;
}

}  // extern "C"
