"""Thin Python handle on one `sgfhe_ctx` of libsgfhe_hip.so (include/sgfhe_hip.h).

Host arrays are numpy; 128-bit residues are uint64 arrays with a trailing axis of 2 ({lo, hi}).
Device-resident entry points take raw device pointers (e.g. `torch.Tensor.data_ptr()`); PyTorch
is only plumbing for device memory and torch.distributed (RCCL), never the compute path.
"""

import collections
import ctypes
import threading

import numpy as np

from . import _lib

FLAG_RAW_MODQ = 1
CIRCUIT_PACK_DIRECT = 1      # SGFHE_CIRCUIT_PACK_DIRECT
CIRCUIT_PACK_LIFT = 2        # SGFHE_CIRCUIT_PACK_LIFT
SCRIPT_CT, SCRIPT_STEPPED, SCRIPT_PROBE, SCRIPT_DEVICE = 1, 2, 4, 8   # SGFHE_SCRIPT_*: forms of sgfhe_debug_circuit_script
FLAG_RAW_RNS2 = 2
LUT_MAX_TABLES = 256         # SGFHE_LUT_MAX_TABLES
CTX_RANDOM_FLATTEN = 1          # accepted, without effect since ABI revision 6
CTX_DETERMINISTIC_ONLY = 2


# The records of the noise probe (sgfhe_lwe_noise, sgfhe_circuit_run_probe), all exact integers.
# Z_r: e = centred (phase - bit Dr); wrong = rows that decrypt wrongly; margin = rows with |e| >= Dr/4.
NoiseStats = collections.namedtuple("NoiseStats", "rows wrong max_abs sum sum_sq margin")
# Z_Q: e = centred (phase - bit 2 DQ_tilde); wrong = rows with |e| >= DQ_tilde.
NoiseStatsQ = collections.namedtuple("NoiseStatsQ", "rows wrong max_abs sum_abs")


def noise_record(words, raw=False):
    """One stats[8] record of the noise probe as a named tuple of Python ints."""
    w = [int(x) for x in words]
    if raw:
        return NoiseStatsQ(w[0], w[1], w[2] | (w[3] << 64), w[4] | (w[5] << 64))
    return NoiseStats(w[0], w[1], w[2], w[3] - (1 << 64) if w[3] >> 63 else w[3], w[4], w[5])


class SgfheError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("sgfhe_hip error %d: %s" % (code, msg))
        self.code = code


def _words(x):
    return (ctypes.c_uint64 * 2)(x & 0xFFFFFFFFFFFFFFFF, (x >> 64) & 0xFFFFFFFFFFFFFFFF)


def _c(arr, dtype=np.uint64):
    a = np.ascontiguousarray(arr, dtype=dtype)
    return a, a.ctypes.data_as(ctypes.c_void_p)


def check_device_tensor(name, t, shape, device, words=True):
    """An argument of the device-resident circuit runs (Engine.circuit_run_device and its kin), checked before any
    library call; needs no engine and no GPU.  `t` must be a torch.Tensor of dtype int64 or uint64 (words=True: LWE
    and ciphertext words) or uint8 (words=False: data planes), C-contiguous, of shape `shape` (an entry None matches
    any length), on the device `device` (an index: cuda:<device>).  ValueError otherwise.  Returns t."""
    import torch
    if not isinstance(t, torch.Tensor):
        raise ValueError("%s: a torch.Tensor is needed, got %s" % (name, type(t).__name__))
    dtypes = (torch.int64, torch.uint64) if words else (torch.uint8,)
    if t.dtype not in dtypes:
        raise ValueError("%s: dtype must be %s, got %s" % (name, " or ".join(str(d) for d in dtypes), t.dtype))
    if not t.is_contiguous():
        raise ValueError("%s: the tensor must be contiguous" % name)
    if t.dim() != len(shape) or any(w is not None and int(w) != int(g) for w, g in zip(shape, t.shape)):
        raise ValueError("%s: shape must be %r, got %r" % (name, tuple(shape), tuple(t.shape)))
    if t.device.type == "cpu":
        raise ValueError("%s: a CPU tensor; the device-resident runs take tensors on cuda:%d" % (name, device))
    if t.device.type != "cuda" or t.device.index != device:
        raise ValueError("%s: the tensor is on %s, the engine on cuda:%d" % (name, t.device, device))
    return t


def _stream_handle(hip_stream):
    """A torch.cuda.Stream, a raw hipStream_t (int) or None (the ctx's own stream) as the C ABI's `void *stream`."""
    if hip_stream is None:
        return ctypes.c_void_p(0)
    return ctypes.c_void_p(int(getattr(hip_stream, "cuda_stream", hip_stream)))


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _hptr(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


# What the ciphertext forms of a circuit run share, host and device-resident alike

def _pack_flags(direct, lift):
    """The flag word of sgfhe_circuit_run_ct_ex and its kin: the C ABI takes the lift bit only with the direct bit."""
    return (CIRCUIT_PACK_DIRECT | (CIRCUIT_PACK_LIFT if lift else 0)) if direct or lift else 0


def _ct_outputs(circuit, p, blocks, packed, lwe, alloc, emitted=None):
    """(w, v, out) of a ciphertext run over `blocks`: w, v [n_outputs][blocks][m] if packed, out [n_outputs][blocks * n]
    [n + 1] if lwe, None otherwise; a stepped run has them per emitted step.  alloc(shape) makes each."""
    lead = () if emitted is None else (emitted,)
    wv = lead + (circuit.n_outputs, blocks, p.m)
    return (alloc(wv) if packed else None, alloc(wv) if packed else None,
            alloc(lead + (circuit.n_outputs, blocks * p.n, p.n + 1)) if lwe else None)


def _ct_result(w, v, out):
    """(w, v), the LWE array, or ((w, v), lwe): whichever of them the caller asked for."""
    if w is not None and out is not None:
        return (w, v), out
    return (w, v) if w is not None else out


def _same_dtype(name, t, like_name, like):
    """An argument of a device-resident run has the dtype of the tensor it goes with."""
    if t.dtype != like.dtype:
        raise ValueError("%s: dtype %s, %s has %s" % (name, t.dtype, like_name, like.dtype))


class Engine:
    """One bootstrap engine (ctx) for one parameter set on one HIP device."""

    def __init__(self, params, device=0, random_flatten=False, deterministic_only=False):
        """Both flatten modes (the `rng` argument of bootstrap / pack_encrypted_bits) are available on
        every engine: where the randomised one needs a prime more (Params(1024): six against five)
        the ctx keeps a basis and a key form per mode and `set_random_flatten` switches between them.
        deterministic_only=True keeps the smaller basis only (SGFHE_CTX_DETERMINISTIC_ONLY: no second
        key form; the randomised mode is then refused where it needs the extra prime).
        random_flatten is accepted for compatibility and has no effect."""
        self.params = params
        self.device = device
        # Held around every C call together with the read of its error string, and by the scheme
        # layer from the choice of the flatten mode to the end of the call that uses it, so that
        # threads sharing an Engine cannot interleave between the two (the C library serialises the
        # individual calls; the pairs are this binding's to keep together).
        self.lock = threading.RLock()
        self._L = _lib.lib()
        sp = _lib.SgfheParams(params.n, params.r, params.m, params.ell, _words(params.Q),
                              _words(params.B), _words(params.DQ_tilde))
        h = ctypes.c_void_p()
        rc = self._L.sgfhe_ctx_create_ex(ctypes.byref(sp), device,
                                         (CTX_RANDOM_FLATTEN if random_flatten else 0) |
                                         (CTX_DETERMINISTIC_ONLY if deterministic_only else 0), ctypes.byref(h))
        self._h = h
        if rc != 0:
            msg = self._L.sgfhe_last_error_string(h).decode() if h else "ctx_create failed"
            if h:
                self._L.sgfhe_ctx_destroy(h)
                self._h = None
            raise SgfheError(rc, msg)

    def clone(self):
        """A second engine on the same device, parameter set and key for an independent caller
        (sgfhe_ctx_clone): shares the device key and constants, owns its work buffers and streams, so
        calls on the clone overlap on the device with calls on this engine (one clone per thread).
        While clones exist the shared key is read-only."""
        h = ctypes.c_void_p()
        with self.lock:
            rc = self._L.sgfhe_ctx_clone(self._h, ctypes.byref(h))
            if rc != 0:
                msg = self._L.sgfhe_last_error_string(h if h else self._h).decode()
                if h:
                    self._L.sgfhe_ctx_destroy(h)
                raise SgfheError(rc, msg)
        other = Engine.__new__(Engine)
        other.params = self.params
        other.device = self.device
        other.lock = threading.RLock()
        other._L = self._L
        other._h = h
        return other

    def set_coalesce(self, enable=True, req_max=32, gates_max=256, window_us=300):
        """Gathering of small bootstrap_batch calls across the engines that share this key (sgfhe_set_coalesce):
        on by default once clones exist; the setting belongs to the shared key."""
        self._call("sgfhe_set_coalesce", int(bool(enable)), req_max, gates_max, window_us)

    def coalesce_stats(self, reset=False):
        st = (ctypes.c_uint64 * 4)()
        self._call("sgfhe_coalesce_stats", st, int(reset))
        return dict(calls=int(st[0]), requests=int(st[1]), gates=int(st[2]), max_requests=int(st[3]))

    def close(self):
        if getattr(self, "_h", None):
            self._L.sgfhe_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _call(self, name, *args):
        with self.lock:
            rc = getattr(self._L, name)(self._h, *args)
            if rc != 0:
                raise SgfheError(rc, self._L.sgfhe_last_error_string(self._h).decode())

    # ---- key ------------------------------------------------------------------------------
    def upload_key(self, canonical):
        """canonical: [n][4][2][m][2] uint64, value.(coeffs) of BootstrapKey.key (fhe.jl:176-201)."""
        p = self.params
        a, ptr = _c(canonical)
        if a.size != p.n * 8 * p.m * 2:
            raise ValueError("bootstrap key must hold n*4*2*m residues of 2 words")
        self._call("sgfhe_bkey_upload", ptr, a.size)

    def upload_key_rns2(self, pairs, m1, m2):
        """pairs: [n][4][2][m][2] uint64 (v1, v2) RNS2Number limbs (src/rns.jl:8-24)."""
        a, ptr = _c(pairs)
        self._call("sgfhe_bkey_upload_rns2", ptr, a.size, m1, m2)

    def rns2_convert(self, values, m1, m2, to_pairs):
        """src/rns.jl on the device: [..., 2] uint64 canonical {lo, hi} -> (x mod m1, x mod m2)
        (to_pairs=True, rns.jl:16-18) or limb pairs -> canonical (to_pairs=False, rns.jl:32-40)."""
        a, ptr = _c(values)
        out = np.zeros_like(a)
        self._call("sgfhe_rns2_convert", int(bool(to_pairs)), ptr, a.size // 2, m1, m2,
                                             out.ctypes.data_as(ctypes.c_void_p))
        return out

    def generate_key(self, sk_bits, seed, noise=None):
        """BootstrapKey(rng, sk) (fhe.jl:181-201) generated on the device from a 32-byte seed
        (ChaCha20 streams); an int is taken as 32 little-endian bytes (tests, benchmarks)."""
        a, ptr = _c(sk_bits)
        if not isinstance(seed, (bytes, bytearray)):
            seed = int(seed).to_bytes(32, "little")
        if len(seed) != 32:
            raise ValueError("key seed must be 32 bytes")
        self._call("sgfhe_bkey_generate", ptr, a.size, bytes(seed),
                                              self.params.n if noise is None else noise)

    def key_device_form_bytes(self):
        n = ctypes.c_size_t()
        self._call("sgfhe_bkey_device_form_bytes", ctypes.byref(n))
        return n.value

    def export_key_device_form(self, dst_device_ptr):
        self._call("sgfhe_bkey_export_device_form", ctypes.c_void_p(dst_device_ptr))

    def import_key_device_form(self, src_device_ptr):
        self._call("sgfhe_bkey_import_device_form", ctypes.c_void_p(src_device_ptr))

    # ---- bootstrap ----------------------------------------------------------------------------
    def set_chunk(self, chunk):
        self._call("sgfhe_set_chunk", chunk)

    def set_lanes(self, lanes):
        self._call("sgfhe_set_lanes", lanes)

    def set_small_batch_max(self, max_bootstraps):
        """Chunks of at most this many bootstraps use the small-batch form of the k-loop (0: never)."""
        self._call("sgfhe_set_small_batch_max", max_bootstraps)

    def set_random_flatten(self, enable, seed=0):
        """rng != nothing branch of flatten (utils.jl:198-241): the draws come from a ChaCha8 counter
        stream keyed with `seed` -- 32 bytes (sgfhe_set_random_flatten_key), or an int taken as 32
        little-endian bytes (tests, benchmarks; the convention of generate_key)."""
        if isinstance(seed, (bytes, bytearray)):
            if len(seed) != 32:
                raise ValueError("random-flatten key: 32 bytes")
            key = bytes(seed)
        else:
            key = (int(seed) % (1 << 256)).to_bytes(32, "little")
        self._call("sgfhe_set_random_flatten_key", int(bool(enable)), key)

    def _lwe_args(self, a1, b1, a2, b2):
        n = self.params.n
        a1, p1 = _c(a1)
        a2, p2 = _c(a2)
        b1, q1 = _c(b1)
        b2, q2 = _c(b2)
        a1 = a1.reshape(-1, n)
        a2 = a2.reshape(-1, n)
        batch = a1.shape[0]
        if a2.shape[0] != batch or b1.size != batch or b2.size != batch:
            raise ValueError("ragged LWE batch")
        keep = (a1, a2, b1, b2)
        return batch, (p1, q1, p2, q2), keep

    def bootstrap_batch(self, a1, b1, a2, b2, raw=False, rns2=False, out=None):
        """bootstrap(bkey, nothing, ., .) (fhe.jl:608-621) over a batch of LWE pairs.
        Returns [batch][3][n+1] uint64 (AND, OR, XOR; a then b), or [batch][3][n+1][2] residues
        mod Q with raw=True (_bootstrap_internal, fhe.jl:559-595): {lo, hi} of the canonical
        value, or with rns2=True the RNS2Number limb pair (v1, v2) (src/rns.jl:16-18).
        `out`: a C-contiguous uint64 array of that shape to write into (a caller in a loop keeps
        its result buffer and its already-touched pages)."""
        batch, (p1, q1, p2, q2), _keep = self._lwe_args(a1, b1, a2, b2)
        n = self.params.n
        raw = raw or rns2
        shape = (batch, 3, n + 1, 2) if raw else (batch, 3, n + 1)
        if out is None:
            out = np.zeros(shape, dtype=np.uint64)
        elif out.shape != shape or out.dtype != np.uint64 or not out.flags["C_CONTIGUOUS"]:
            raise ValueError("bootstrap_batch: out must be a C-contiguous uint64 array of shape %r" % (shape,))
        if batch:
            self._call("sgfhe_bootstrap_batch", p1, q1, p2, q2, batch, out.ctypes.data_as(ctypes.c_void_p),
                (FLAG_RAW_MODQ if raw else 0) | (FLAG_RAW_RNS2 if rns2 else 0))
        return out

    def bootstrap_lut_batch(self, a, b, tables, raw=False):
        """LUT bootstraps (sgfhe_bootstrap_lut_batch): any function of three bits in one bootstrap.  a [batch][n],
        b [batch]: rows over Z_r whose phase is s Dr/4 + e, s = x0 + 2 x1 + 4 x2 the sum of three inputs at the
        codewords Dr/4, Dr/2, Dr and |e| < Dr/8 (bootstrapped inputs only: see the noise rule in
        include/sgfhe_hip.h); tables [batch]: bit s of a row's table is its function value at s.
        Returns [batch][3][n+1] uint64 -- row 0 the result at codeword Dr (an ordinary wire), row 1 at Dr/2, row 2 at
        Dr/4 -- or [batch][3][n+1][2] residues mod Q with raw=True."""
        n = self.params.n
        a, pa = _c(a)
        b, pb = _c(b)
        t, pt = _c(tables, np.uint8)
        a = a.reshape(-1, n)
        batch = a.shape[0]
        if b.size != batch or t.size != batch:
            raise ValueError("bootstrap_lut_batch: a is [batch][n], b and tables are [batch]")
        out = np.zeros((batch, 3, n + 1, 2) if raw else (batch, 3, n + 1), dtype=np.uint64)
        if batch:
            self._call("sgfhe_bootstrap_lut_batch", pa, pb, pt, batch, out.ctypes.data_as(ctypes.c_void_p),
                       FLAG_RAW_MODQ if raw else 0)
        return out

    def bootstrap_lut_multi_batch(self, a, b, tables, raw=False):
        """A LUT family (sgfhe_bootstrap_lut_multi_batch): T truth tables on one bootstrap per row.  a [batch][n],
        b [batch] as in bootstrap_lut_batch; tables [batch][T], T in 1..256.  Returns [batch][T][3][n+1] uint64 (or
        [batch][T][3][n+1][2] residues mod Q with raw=True): [:, j] has the bytes of bootstrap_lut_batch(a, b,
        tables[:, j]) at the same call number of the draw stream, for the cost of one k-loop per row."""
        n = self.params.n
        a, pa = _c(a)
        b, pb = _c(b)
        t, pt = _c(tables, np.uint8)
        a = a.reshape(-1, n)
        batch = a.shape[0]
        if b.size != batch or t.ndim != 2 or t.shape[0] != batch:
            raise ValueError("bootstrap_lut_multi_batch: a is [batch][n], b is [batch], tables is [batch][T]")
        T = t.shape[1]
        if not 1 <= T <= LUT_MAX_TABLES:
            raise ValueError("bootstrap_lut_multi_batch: 1 to %d tables per row" % LUT_MAX_TABLES)
        out = np.zeros((batch, T, 3, n + 1, 2) if raw else (batch, T, 3, n + 1), dtype=np.uint64)
        if batch:
            self._call("sgfhe_bootstrap_lut_multi_batch", pa, pb, pt, T, batch, out.ctypes.data_as(ctypes.c_void_p),
                       FLAG_RAW_MODQ if raw else 0)
        return out

    def bootstrap_batch_device(self, a1_ptr, b1_ptr, a2_ptr, b2_ptr, batch, out_ptr, raw=False,
                               stream=None):
        """Asynchronous, all buffers device-resident (raw pointers)."""
        self._call("sgfhe_bootstrap_batch_device", ctypes.c_void_p(a1_ptr), ctypes.c_void_p(b1_ptr), ctypes.c_void_p(a2_ptr),
            ctypes.c_void_p(b2_ptr), batch, ctypes.c_void_p(out_ptr),
            FLAG_RAW_MODQ if raw else 0, ctypes.c_void_p(stream or 0))

    def sync(self):
        self._call("sgfhe_sync")

    @staticmethod
    def _planes(circuit, data, instances):
        """The data planes of a run as the C ABI takes them: (array or None, pointer or None).  A circuit with planes
        needs data [planes][instances] of uint8; one without takes none (circuit.check_data raises ValueError)."""
        from .circuit import check_data
        d = check_data(circuit, data, instances)
        if d is None:
            return None, None
        d = np.ascontiguousarray(d)
        return d, d.ctypes.data_as(ctypes.c_void_p)

    def circuit_run(self, circuit, inputs, data=None):
        """A gate circuit (circuit.Circuit) over many instances on the device (sgfhe_circuit_run):
        inputs [n_inputs][instances][n+1] uint64 (a then b) -> outputs [n_outputs][instances][n+1].
        A circuit with lane groups (Circuit(group=G)) needs instances to be a multiple of G; in the ciphertext
        form (circuit_run_ct) n must be one, so that no group straddles two ciphertexts.
        data: the planes of a circuit that has any (Circuit(planes=P)): uint8 [planes][instances], the truth table of
        every data node at every instance (sgfhe_circuit_run_data)."""
        n = self.params.n
        a, ptr = _c(inputs)
        if a.ndim != 3 or a.shape[0] != circuit.n_inputs or a.shape[2] != n + 1:
            raise ValueError("circuit_run: inputs must be [n_inputs=%d][instances][n+1=%d]" % (circuit.n_inputs, n + 1))
        d, pd = self._planes(circuit, data, a.shape[1])
        out = np.zeros((circuit.n_outputs, a.shape[1], n + 1), dtype=np.uint64)
        if d is not None:
            self._call("sgfhe_circuit_run_data", circuit.handle(), a.shape[1], ptr, pd, out.ctypes.data_as(ctypes.c_void_p))
        else:
            self._call("sgfhe_circuit_run", circuit.handle(), a.shape[1], ptr, out.ctypes.data_as(ctypes.c_void_p))
        return out

    def circuit_probe(self, circuit, inputs, sk, in_bits, data=None):
        """circuit_run that also measures every wire against the secret key (sgfhe_circuit_run_probe; a
        DIAGNOSTIC: the key crosses the boundary).  sk: n key bits; in_bits [n_inputs][instances]: the plaintext
        bit of every input LWE.  Returns (out, stats): out as circuit_run (the same bytes), stats a list of
        NoiseStats by wire id -- inputs, then AND, OR, XOR of every node; all-zero records for pruned nodes and for the
        wires of a LUT sibling (Circuit.lut_multi) that nothing reads: those are never formed.  data: as circuit_run
        (sgfhe_circuit_run_probe_data)."""
        n = self.params.n
        a, ptr = _c(inputs)
        if a.ndim != 3 or a.shape[0] != circuit.n_inputs or a.shape[2] != n + 1:
            raise ValueError("circuit_probe: inputs must be [n_inputs=%d][instances][n+1=%d]" % (circuit.n_inputs, n + 1))
        sk, psk = _c(sk)
        bits, pbits = _c(in_bits, np.uint8)
        if sk.size != n or bits.size != circuit.n_inputs * a.shape[1]:
            raise ValueError("circuit_probe: sk holds n key bits, in_bits is [n_inputs][instances]")
        d, pd = self._planes(circuit, data, a.shape[1])
        out = np.zeros((circuit.n_outputs, a.shape[1], n + 1), dtype=np.uint64)
        stats = np.zeros((circuit.n_inputs + 3 * circuit.n_gates, 8), dtype=np.uint64)
        if d is not None:
            self._call("sgfhe_circuit_run_probe_data", circuit.handle(), a.shape[1], ptr, pd,
                       out.ctypes.data_as(ctypes.c_void_p), psk, pbits, stats.ctypes.data_as(ctypes.c_void_p))
        else:
            self._call("sgfhe_circuit_run_probe", circuit.handle(), a.shape[1], ptr, out.ctypes.data_as(ctypes.c_void_p),
                       psk, pbits, stats.ctypes.data_as(ctypes.c_void_p))
        return out, [noise_record(rec) for rec in stats]

    def lwe_noise(self, sk, lwe, expected, raw=False, stride=None):
        """The error of LWE rows against the secret key, reduced on the device (sgfhe_lwe_noise; a DIAGNOSTIC: the
        key crosses the boundary; no bootstrap key is needed).  sk: n key bits; expected: one plaintext bit per row.
        lwe: uint64 words -- rows of n + 1 (a then b) over Z_r, or with raw=True rows of [n + 1][2] residues mod Q (a
        bootstrap_batch(raw=True) result).  stride: words from one row to the next (default: the row length);
        3 (n + 1) with lwe = out[:, g] of a [batch][3][n + 1] result probes gate g in place -- pass the flat array
        from the first row on.  Returns NoiseStats (NoiseStatsQ with raw=True)."""
        n = self.params.n
        rowlen = (n + 1) * (2 if raw else 1)
        stride = rowlen if stride is None else int(stride)
        exp, pexp = _c(expected, np.uint8)
        count = exp.size
        arr, parr = _c(lwe)
        sk, psk = _c(sk)
        if sk.size != n:
            raise ValueError("lwe_noise: sk holds n key bits")
        if count and arr.size < (count - 1) * stride + rowlen:
            raise ValueError("lwe_noise: %d rows of stride %d need %d words, got %d"
                             % (count, stride, (count - 1) * stride + rowlen, arr.size))
        st = (ctypes.c_uint64 * 8)()
        self._call("sgfhe_lwe_noise", psk, parr, count, stride, pexp, FLAG_RAW_MODQ if raw else 0, st)
        return noise_record(st, raw)

    def circuit_run_ct(self, circuit, a, b, packed=True, lwe=False, direct=False, lift=False, data=None):
        """A gate circuit with RLWE ciphertexts at both ends (sgfhe_circuit_run_ct): split_ciphertext of the
        inputs and pack_encrypted_bits of the outputs run on the device inside the one run.
        a, b: [n_inputs][blocks][N] uint64, rlwe.a / rlwe.b of one ciphertext per (input, block), N = n
        (PackedCiphertext) or m (Ciphertext); a ciphertext is one wire over n instances.
        packed: return (w, v), each [n_outputs][blocks][m]; lwe: return the LWE array
        [n_outputs][blocks * n][n + 1] of circuit_run.  Both: ((w, v), lwe).
        direct: SGFHE_CIRCUIT_PACK_DIRECT (sgfhe_circuit_run_ct_ex) -- outputs that name a gate wire are packed
        from the gate's LWEs over Z_Q, without the n refresh bootstraps per ciphertext; the packed ciphertexts
        decrypt alike but are other bytes, the LWE outputs are the same bytes.
        lift: SGFHE_CIRCUIT_PACK_DIRECT | SGFHE_CIRCUIT_PACK_LIFT, with or without direct=True (the C ABI takes the
        lift bit only together with the direct bit) -- direct as above, and every other output (an input, the constant, an XOR3
        wire, a lane-shifted reference) is lifted from Z_r (lwe_lift) instead of refreshed: no bootstrap in the pack
        stage, but such an output carries its wire's error on (see the noise rule in include/sgfhe_hip.h).
        data: the planes of a circuit that has any, uint8 [planes][blocks * n] (sgfhe_circuit_run_ct_data)."""
        p = self.params
        a, pa = _c(a)
        b, pb = _c(b)
        if a.ndim != 3 or a.shape != b.shape or a.shape[0] != circuit.n_inputs or a.shape[2] not in (p.n, p.m):
            raise ValueError("circuit_run_ct: a and b must be [n_inputs=%d][blocks][N], N = n = %d or m = %d"
                             % (circuit.n_inputs, p.n, p.m))
        if not packed and not lwe:
            raise ValueError("circuit_run_ct: ask for the packed outputs, the LWE outputs or both")
        blocks = a.shape[1]
        w, v, out = _ct_outputs(circuit, p, blocks, packed, lwe, lambda shape: np.zeros(shape, dtype=np.uint64))
        outs = (_hptr(w), _hptr(v), _hptr(out))
        d, pd = self._planes(circuit, data, blocks * p.n)
        if d is not None:
            self._call("sgfhe_circuit_run_ct_data", circuit.handle(), blocks, pa, pb, a.shape[2], pd, *outs,
                       _pack_flags(direct, lift))
        elif direct or lift:
            self._call("sgfhe_circuit_run_ct_ex", circuit.handle(), blocks, pa, pb, a.shape[2], *outs, _pack_flags(direct, lift))
        else:
            self._call("sgfhe_circuit_run_ct", circuit.handle(), blocks, pa, pb, a.shape[2], *outs)
        return _ct_result(w, v, out)

    @staticmethod
    def _step_args(circuit, data, emit, steps, instances):
        """(planes array, its pointer, emit array, its pointer, emitted steps) of a stepped run."""
        from .circuit import check_step_data
        d = check_step_data(circuit, data, steps, instances)
        pd = None
        if d is not None:
            d = np.ascontiguousarray(d)
            pd = d.ctypes.data_as(ctypes.c_void_p)
        return (d, pd) + Engine._emit_arg(emit, steps)

    @staticmethod
    def _emit_arg(emit, steps):
        """(emit array, its pointer, emitted steps) of a stepped run; emit None: every step."""
        if emit is None:
            return None, None, steps
        e = np.ascontiguousarray(np.asarray(emit).astype(bool).astype(np.uint8))
        if e.shape != (steps,):
            raise ValueError("emit: one flag per step (%d)" % steps)
        return e, e.ctypes.data_as(ctypes.c_void_p), int(e.sum())

    def circuit_run_steps(self, circuit, state, stream, data=None, emit=None):
        """A circuit with registers (Circuit(registers=R)) evaluated `steps` times over the same instances in one queued
        run, the registers fed back on the device (sgfhe_circuit_run_steps).
        state: [registers][instances][n + 1] uint64, or None: every register FALSE; stream:
        [steps][stream inputs][instances][n + 1]; data: uint8 [steps][planes][instances] for a circuit with planes;
        emit: [steps] flags, the steps whose outputs are wanted (None: all).
        Returns (out [emitted steps][n_outputs][instances][n + 1], state [registers][instances][n + 1] after the last
        step).  Step s is, byte for byte, circuit_run of circuit.step_plan() on (state ++ stream[s])."""
        n = self.params.n
        x, px = _c(stream)
        if x.ndim != 4 or x.shape[1] != circuit.n_inputs - circuit.n_regs or x.shape[3] != n + 1:
            raise ValueError("circuit_run_steps: stream must be [steps][stream inputs=%d][instances][n+1=%d]"
                             % (circuit.n_inputs - circuit.n_regs, n + 1))
        steps, inst = x.shape[0], x.shape[2]
        ps = None
        if state is not None:
            state, ps = _c(state)
            if state.shape != (circuit.n_regs, inst, n + 1):
                raise ValueError("circuit_run_steps: state must be [registers=%d][instances=%d][n+1]" % (circuit.n_regs, inst))
        d, pd, e, pe, emitted = self._step_args(circuit, data, emit, steps, inst)
        out = np.zeros((emitted, circuit.n_outputs, inst, n + 1), dtype=np.uint64)
        st = np.zeros((circuit.n_regs, inst, n + 1), dtype=np.uint64)
        self._call("sgfhe_circuit_run_steps", circuit.handle(), inst, steps, ps, px, pd, pe,
                   out.ctypes.data_as(ctypes.c_void_p), st.ctypes.data_as(ctypes.c_void_p))
        return out, st

    def circuit_run_steps_ct(self, circuit, state_a, state_b, a, b, N=None, packed=True, lwe=False, direct=False,
                             lift=False, data=None, emit=None):
        """The stepped run with RLWE ciphertexts at both ends (sgfhe_circuit_run_steps_ct).
        state_a, state_b: [registers][blocks][N] or None (every register FALSE); a, b: [steps][stream inputs][blocks][N],
        N = n or m (given as N when the circuit has no stream input and no state); packed, lwe, direct, lift: as
        circuit_run_ct, per emitted step; data: uint8 [steps][planes][blocks * n]; emit: as circuit_run_steps.
        Registers of scale 0 only.  Returns (outputs, state): outputs (w, v), each [emitted steps][n_outputs][blocks][m],
        the LWE array [emitted steps][n_outputs][blocks * n][n + 1], or ((w, v), lwe), as circuit_run_ct; state
        [registers][blocks * n][n + 1], the registers after the last step as LWEs."""
        p = self.params
        a, pa = _c(a)
        b, pb = _c(b)
        if a.ndim != 4 or a.shape != b.shape or a.shape[1] != circuit.n_inputs - circuit.n_regs or \
                a.shape[3] not in (p.n, p.m) or (N is not None and a.shape[3] != N):
            raise ValueError("circuit_run_steps_ct: a and b must be [steps][stream inputs=%d][blocks][N], N = n = %d or m = %d"
                             % (circuit.n_inputs - circuit.n_regs, p.n, p.m))
        if not packed and not lwe:
            raise ValueError("circuit_run_steps_ct: ask for the packed outputs, the LWE outputs or both")
        steps, blocks, N = a.shape[0], a.shape[2], a.shape[3]
        psa = psb = None
        if state_a is not None:
            state_a, psa = _c(state_a)
            state_b, psb = _c(state_b)
            if state_a.shape != (circuit.n_regs, blocks, N) or state_b.shape != state_a.shape:
                raise ValueError("circuit_run_steps_ct: state_a and state_b must be [registers=%d][blocks=%d][N=%d]"
                                 % (circuit.n_regs, blocks, N))
        d, pd, e, pe, emitted = self._step_args(circuit, data, emit, steps, blocks * p.n)
        w, v, out = _ct_outputs(circuit, p, blocks, packed, lwe, lambda shape: np.zeros(shape, dtype=np.uint64), emitted)
        st = np.zeros((circuit.n_regs, blocks * p.n, p.n + 1), dtype=np.uint64)
        self._call("sgfhe_circuit_run_steps_ct", circuit.handle(), blocks, steps, psa, psb, pa, pb, N, pd, pe, _hptr(w),
                   _hptr(v), _hptr(out), _hptr(st), _pack_flags(direct, lift))
        return _ct_result(w, v, out), st

    # ---- device-resident circuit runs --------------------------------------------------------------
    # The run forms above with every array a torch.Tensor on the engine's device (sgfhe_circuit_run*_device): the same
    # shapes, the same bytes, the same call numbers, nothing copied to or from the host and no host wait.
    #
    # Ordering is the caller's duty.  The work is queued on `hip_stream` -- a torch.cuda.Stream, a raw hipStream_t, or
    # None.  None names the ctx's OWN stream, never torch's default stream.  Torch work on any other stream is not
    # ordered against the run: synchronise before the call (torch.cuda.synchronize(), or the stream that produced the
    # inputs) and call eng.sync() after it, before torch reads the results.  The alternative is to run everything,
    # the torch work included, on one explicit non-default torch.cuda.Stream and to pass it as `hip_stream`: the runs
    # and the torch kernels between them are then in stream order and nothing waits on the host.  Every tensor handed
    # in or returned must outlive the queued work (keep a reference until eng.sync() or a synchronise of the stream).
    # A call waits for nothing, but it launches the whole run from the host, and the hardware queue runs only so far
    # ahead of the device: the call of a long run is paced by it, as bootstrap_batch_device is.

    def _planes_device(self, circuit, data, shape):
        """The planes of a device-resident run: a uint8 tensor of `shape`, or None for a circuit without planes."""
        if not circuit.planes:
            if data is not None:
                raise ValueError("data given for a circuit without data planes")
            return None
        if data is None:
            raise ValueError("a circuit with data planes needs data [planes=%d][instances]" % circuit.planes)
        return check_device_tensor("data", data, shape, self.device, words=False)

    def _empty(self, shape, dtype, hip_stream):
        """An uninitialised result tensor (no fill kernel: it would run on torch's stream, unordered against the run);
        allocated under `hip_stream` where that is a torch stream, so that torch's allocator knows its user."""
        import torch
        dev = torch.device("cuda", self.device)
        if isinstance(hip_stream, torch.cuda.Stream):
            with torch.cuda.stream(hip_stream):
                return torch.empty(shape, dtype=dtype, device=dev)
        return torch.empty(shape, dtype=dtype, device=dev)

    def _result(self, name, t, shape, like, hip_stream):
        """A result tensor of the words' dtype: the caller's `t`, checked, or a new one."""
        if t is None:
            return self._empty(shape, like.dtype, hip_stream)
        check_device_tensor(name, t, shape, self.device)
        if t.dtype != like.dtype:
            raise ValueError("%s: dtype %s, the inputs have %s" % (name, t.dtype, like.dtype))
        return t

    def circuit_run_device(self, circuit, inputs, data=None, out=None, hip_stream=None):
        """circuit_run with the LWEs resident on the device (sgfhe_circuit_run_device), asynchronous: inputs
        [n_inputs][instances][n+1] int64 or uint64 -> out [n_outputs][instances][n+1] of the same dtype (every word is
        below 2^63), the bytes of circuit_run; data uint8 [planes][instances].  out: a tensor to write into (it must
        not overlap the inputs).  Ordering and lifetimes: see the note above -- hip_stream=None is the ctx's own
        stream, never torch's default stream; synchronise before and eng.sync() after, or run everything on one
        explicit torch.cuda.Stream passed as hip_stream; the tensors must outlive the queued work."""
        n = self.params.n
        x = check_device_tensor("inputs", inputs, (circuit.n_inputs, None, n + 1), self.device)
        inst = x.shape[1]
        d = self._planes_device(circuit, data, (circuit.planes, inst))
        out = self._result("out", out, (circuit.n_outputs, inst, n + 1), x, hip_stream)
        if inst:
            self._call("sgfhe_circuit_run_device", circuit.handle(), inst, _ptr(x), _ptr(d), _ptr(out),
                       _stream_handle(hip_stream))
        return out

    def circuit_run_ct_device(self, circuit, a, b, packed=True, lwe=False, direct=False, lift=False, data=None,
                              hip_stream=None):
        """circuit_run_ct with the ciphertexts resident on the device (sgfhe_circuit_run_ct_device), asynchronous:
        a, b [n_inputs][blocks][N] int64 or uint64 tensors, N = n or m; packed, lwe, direct, lift and the results as
        circuit_run_ct, as tensors of the inputs' dtype; data uint8 [planes][blocks * n].  The ciphertexts are split
        where they are, (w, v) is the input of a next run without leaving the device.  Ordering and lifetimes as
        circuit_run_device: hip_stream=None is the ctx's own stream, never torch's default stream; synchronise before
        and eng.sync() after, or one explicit torch.cuda.Stream for everything; the tensors outlive the queued work."""
        p = self.params
        a = check_device_tensor("a", a, (circuit.n_inputs, None, None), self.device)
        if a.shape[2] not in (p.n, p.m):
            raise ValueError("a: shape must be [n_inputs=%d][blocks][N], N = n = %d or m = %d" % (circuit.n_inputs, p.n, p.m))
        b = check_device_tensor("b", b, tuple(a.shape), self.device)
        _same_dtype("b", b, "a", a)
        if not packed and not lwe:
            raise ValueError("circuit_run_ct_device: ask for the packed outputs, the LWE outputs or both")
        blocks = a.shape[1]
        d = self._planes_device(circuit, data, (circuit.planes, blocks * p.n))
        w, v, out = _ct_outputs(circuit, p, blocks, packed, lwe, lambda shape: self._empty(shape, a.dtype, hip_stream))
        if blocks:
            self._call("sgfhe_circuit_run_ct_device", circuit.handle(), blocks, _ptr(a), _ptr(b), a.shape[2], _ptr(d),
                       _ptr(w), _ptr(v), _ptr(out), _pack_flags(direct, lift), _stream_handle(hip_stream))
        return _ct_result(w, v, out)

    def circuit_run_steps_device(self, circuit, state, stream, data=None, emit=None, out=None, state_out=None,
                                 hip_stream=None):
        """circuit_run_steps with state and stream resident on the device (sgfhe_circuit_run_steps_device),
        asynchronous: state [registers][instances][n+1] or None (every register FALSE), stream
        [steps][stream inputs][instances][n+1], int64 or uint64 tensors; data uint8 [steps][planes][instances]; emit a
        HOST sequence of [steps] flags (it steers the host loop).  Returns (out [emitted steps][n_outputs][instances]
        [n+1], state after the last step) as tensors; out / state_out: tensors to write into.  state_out may be `state`
        itself -- the state is read in full before anything is written -- so a caller keeps one state tensor and feeds
        a stream chunk by chunk; no other result may overlap an input.  Ordering and lifetimes as circuit_run_device:
        hip_stream=None is the ctx's own stream, never torch's default stream; synchronise before and eng.sync() after,
        or one explicit torch.cuda.Stream for everything; the tensors outlive the queued work."""
        n = self.params.n
        x = check_device_tensor("stream", stream, (None, circuit.n_inputs - circuit.n_regs, None, n + 1), self.device)
        steps, inst = x.shape[0], x.shape[2]
        if state is not None:
            check_device_tensor("state", state, (circuit.n_regs, inst, n + 1), self.device)
            _same_dtype("state", state, "stream", x)
        d = self._planes_device(circuit, data, (steps, circuit.planes, inst))
        e, pe, emitted = self._emit_arg(emit, steps)
        out = self._result("out", out, (emitted, circuit.n_outputs, inst, n + 1), x, hip_stream)
        state_out = self._result("state_out", state_out, (circuit.n_regs, inst, n + 1), x, hip_stream)
        if steps and inst:
            self._call("sgfhe_circuit_run_steps_device", circuit.handle(), inst, steps, _ptr(state), _ptr(x), _ptr(d), pe,
                       _ptr(out), _ptr(state_out), _stream_handle(hip_stream))
        return out, state_out

    def circuit_run_steps_ct_device(self, circuit, state_a, state_b, a, b, N=None, packed=True, lwe=False, direct=False,
                                    lift=False, data=None, emit=None, hip_stream=None):
        """circuit_run_steps_ct with the ciphertexts resident on the device (sgfhe_circuit_run_steps_ct_device),
        asynchronous: state_a, state_b [registers][blocks][N] or None, a, b [steps][stream inputs][blocks][N], int64 or
        uint64 tensors; everything else, and the results (as tensors), as circuit_run_steps_ct; emit stays a host
        sequence.  Ordering and lifetimes as circuit_run_device: hip_stream=None is the ctx's own stream, never torch's
        default stream; synchronise before and eng.sync() after, or one explicit torch.cuda.Stream for everything; the
        tensors outlive the queued work."""
        p = self.params
        a = check_device_tensor("a", a, (None, circuit.n_inputs - circuit.n_regs, None, None), self.device)
        if a.shape[3] not in (p.n, p.m) or (N is not None and a.shape[3] != N):
            raise ValueError("a: shape must be [steps][stream inputs=%d][blocks][N], N = n = %d or m = %d"
                             % (circuit.n_inputs - circuit.n_regs, p.n, p.m))
        b = check_device_tensor("b", b, tuple(a.shape), self.device)
        _same_dtype("b", b, "a", a)
        if not packed and not lwe:
            raise ValueError("circuit_run_steps_ct_device: ask for the packed outputs, the LWE outputs or both")
        steps, blocks, N = a.shape[0], a.shape[2], a.shape[3]
        if (state_a is None) != (state_b is None):
            raise ValueError("state_a and state_b go together")
        for name, s in (("state_a", state_a), ("state_b", state_b)):
            if s is not None:
                check_device_tensor(name, s, (circuit.n_regs, blocks, N), self.device)
                _same_dtype(name, s, "a", a)
        d = self._planes_device(circuit, data, (steps, circuit.planes, blocks * p.n))
        e, pe, emitted = self._emit_arg(emit, steps)
        w, v, out = _ct_outputs(circuit, p, blocks, packed, lwe, lambda shape: self._empty(shape, a.dtype, hip_stream),
                                emitted)
        st = self._empty((circuit.n_regs, blocks * p.n, p.n + 1), a.dtype, hip_stream)
        if steps and blocks:
            self._call("sgfhe_circuit_run_steps_ct_device", circuit.handle(), blocks, steps, _ptr(state_a), _ptr(state_b),
                       _ptr(a), _ptr(b), N, _ptr(d), pe, _ptr(w), _ptr(v), _ptr(out), _ptr(st), _pack_flags(direct, lift),
                       _stream_handle(hip_stream))
        return _ct_result(w, v, out), st

    def pack_encrypted_bits(self, a, b):
        """pack_encrypted_bits (fhe.jl:660-696) for `count` groups of n LWEs: a [count][n][n],
        b [count][n] -> (w, v), each [count][m] uint64 over Z_r."""
        p = self.params
        a, pa = _c(a)
        b, pb = _c(b)
        if a.size % (p.n * p.n) or b.size * p.n != a.size:
            raise ValueError("pack_encrypted_bits: a is [count][n][n], b is [count][n]")
        count = a.size // (p.n * p.n)
        w = np.zeros((count, p.m), dtype=np.uint64)
        v = np.zeros((count, p.m), dtype=np.uint64)
        self._call("sgfhe_pack_encrypted_bits", pa, pb, count,
                                                    w.ctypes.data_as(ctypes.c_void_p),
                                                    v.ctypes.data_as(ctypes.c_void_p))
        return w, v

    def lwe_lift(self, lwe):
        """LWEs over Z_r lifted to Z_Q by exact scaling, floor((x Q + r/2) / r) word by word (sgfhe_lwe_lift_modq):
        lwe [..., n + 1] uint64, a then b -> [..., n + 1][2] residues {lo, hi}, the input of pack_lwe_modq and of
        lwe_noise(raw=True).  No bootstrap and no key: the error of the LWEs is carried on, not cleaned."""
        n = self.params.n
        lwe, pl = _c(lwe)
        if lwe.ndim < 1 or lwe.shape[-1] != n + 1:
            raise ValueError("lwe_lift: lwe is [...][n + 1]")
        out = np.zeros(lwe.shape + (2,), dtype=np.uint64)
        if lwe.size:
            self._call("sgfhe_lwe_lift_modq", pl, lwe.size // (n + 1), out.ctypes.data_as(ctypes.c_void_p))
        return out

    def pack_lwe_modq(self, lwe):
        """The tail of pack_encrypted_bits (fhe.jl:675-695) on LWEs already over Z_Q (sgfhe_pack_lwe_modq):
        lwe [count][n][n + 1][2] uint64, a then b as 16-byte residues -- one gate's rows of
        bootstrap_batch(raw=True) -- -> (w, v), each [count][m] uint64 over Z_r."""
        p = self.params
        lwe, pl = _c(lwe)
        per = p.n * (p.n + 1) * 2
        if lwe.size % per:
            raise ValueError("pack_lwe_modq: lwe is [count][n][n + 1][2]")
        count = lwe.size // per
        w = np.zeros((count, p.m), dtype=np.uint64)
        v = np.zeros((count, p.m), dtype=np.uint64)
        if count:
            self._call("sgfhe_pack_lwe_modq", pl, count, w.ctypes.data_as(ctypes.c_void_p), v.ctypes.data_as(ctypes.c_void_p))
        return w, v

    # ---- parity / debug hooks ---------------------------------------------------------------
    def external_product(self, a, b, A):
        """external_product(nothing, a, b, A, Val(B), Val(2)) (fhe.jl:519-530)."""
        m = self.params.m
        a, pa = _c(a)
        b, pb = _c(b)
        A, pA = _c(A)
        if a.size != 2 * m or b.size != 2 * m or A.size != 16 * m:
            raise ValueError("external_product: a, b are [m][2]; A is [4][2][m][2]")
        ra = np.zeros((m, 2), dtype=np.uint64)
        rb = np.zeros((m, 2), dtype=np.uint64)
        self._call("sgfhe_external_product", pa, pb, pA,
                                                 ra.ctypes.data_as(ctypes.c_void_p),
                                                 rb.ctypes.data_as(ctypes.c_void_p))
        return ra, rb

    def debug_cmux(self, a, b, C, j):
        """One k-loop iteration on chosen operands (sgfhe_debug_cmux): a, b [m][2], C [4][2][m][2]
        -> (a, b) + (x^j - 1) sum_row flatten(a, b)_row (*) C[row]."""
        m = self.params.m
        a, pa = _c(a)
        b, pb = _c(b)
        C, pC = _c(C)
        if a.size != 2 * m or b.size != 2 * m or C.size != 16 * m:
            raise ValueError("debug_cmux: a, b are [m][2]; C is [4][2][m][2]")
        ra = np.zeros((m, 2), dtype=np.uint64)
        rb = np.zeros((m, 2), dtype=np.uint64)
        self._call("sgfhe_debug_cmux", pa, pb, pC, int(j), ra.ctypes.data_as(ctypes.c_void_p),
                                           rb.ctypes.data_as(ctypes.c_void_p))
        return ra, rb

    def debug_accumulators(self, a1, b1, a2, b2, n_iters):
        batch, (p1, q1, p2, q2), _keep = self._lwe_args(a1, b1, a2, b2)
        acc = np.zeros((batch, 2, self.params.m, 2), dtype=np.uint64)
        if batch:
            self._call("sgfhe_debug_accumulators", p1, q1, p2, q2, batch, n_iters,
                                                       acc.ctypes.data_as(ctypes.c_void_p))
        return acc

    def debug_digits(self, a1, b1, a2, b2, n_iters):
        """Stored digit planes after n_iters iterations: [batch][2][2][m] uint64 (sgfhe_debug_digits)."""
        batch, (p1, q1, p2, q2), _keep = self._lwe_args(a1, b1, a2, b2)
        dig = np.zeros((batch, 2, 2, self.params.m), dtype=np.uint64)
        if batch:
            self._call("sgfhe_debug_digits", p1, q1, p2, q2, batch, n_iters,
                                                 dig.ctypes.data_as(ctypes.c_void_p))
        return dig

    def debug_flatten(self, values):
        """Deterministic flatten_poly of two polynomials: values [2][m][2] uint64 canonical residues
        -> stored digits [2][2][m] (sgfhe_debug_flatten)."""
        m = self.params.m
        a, ptr = _c(values)
        if a.size != 4 * m:
            raise ValueError("debug_flatten: values is [2][m][2]")
        dig = np.zeros((2, 2, m), dtype=np.uint64)
        self._call("sgfhe_debug_flatten", ptr, dig.ctypes.data_as(ctypes.c_void_p))
        return dig

    def debug_kloop_step(self, digits, C, j, k=0):
        """One k-loop step from chosen stored digits, in the form a call of that many gates takes
        (sgfhe_debug_kloop_step): digits [gates][2][2][m] uint64, C [4][2][m][2], j [gates] ->
        (digits after the step, (external-product kernels, CRT kernel))."""
        m = self.params.m
        digits, pd = _c(digits)
        C, pC = _c(C)
        j, pj = _c(j, np.uint32)
        gates = j.size
        if digits.size != gates * 4 * m or C.size != 16 * m:
            raise ValueError("debug_kloop_step: digits is [gates][2][2][m], C is [4][2][m][2], j is [gates]")
        out = np.zeros((gates, 2, 2, m), dtype=np.uint64)
        a, b = ctypes.create_string_buffer(96), ctypes.create_string_buffer(96)
        self._call("sgfhe_debug_kloop_step", pd, pC, pj, gates, int(k), out.ctypes.data_as(ctypes.c_void_p), a, 96, b, 96)
        return out, (a.value.decode(), b.value.decode())

    def debug_chunk_entry(self, a1, b1, a2, b2, lut=None):
        """The entry of one chunk from chosen rows (sgfhe_debug_chunk_entry): a1, a2 [rows][n], b1, b2 [rows] as in
        bootstrap_batch, lut None or [rows] uint32 descriptor words (0, or 0x100 | table for a LUT row) ->
        (stored digits [rows][2][2][m] uint64, u.a [rows][n] uint32) as the k-loop of a call finds them."""
        rows, (p1, q1, p2, q2), _keep = self._lwe_args(a1, b1, a2, b2)
        pl = None
        if lut is not None:
            lut, pl = _c(lut, np.uint32)
            if lut.size != rows:
                raise ValueError("debug_chunk_entry: lut is [rows]")
        dig = np.zeros((rows, 2, 2, self.params.m), dtype=np.uint64)
        ua = np.zeros((rows, self.params.n), dtype=np.uint32)
        self._call("sgfhe_debug_chunk_entry", p1, q1, p2, q2, rows, pl, dig.ctypes.data_as(ctypes.c_void_p),
                   ua.ctypes.data_as(ctypes.c_void_p))
        return dig, ua

    def debug_chunk_exit(self, digits, lut=None, tables=None, raw=False, rns2=False, want_acc=False):
        """The exit of one chunk from chosen stored digits (sgfhe_debug_chunk_exit): digits [rows][2][2][m] uint64;
        lut None or [rows] uint32 descriptor words (0: a classic row, 0x100 | table: a LUT row); tables None or
        [rows][T] uint8, a LUT family.  Returns the rows of a call of that kind -- [rows][3][n+1] uint64, with tables
        [rows][T][3][n+1], a last axis of 2 with raw (residues mod Q) or rns2 (RNS2 limb pairs) -- and with want_acc
        also the accumulators [rows][2][m][2] the digits store."""
        n, m = self.params.n, self.params.m
        digits, pd = _c(digits)
        if digits.size % (4 * m):
            raise ValueError("debug_chunk_exit: digits is [rows][2][2][m]")
        rows = digits.size // (4 * m)
        pl = pt = None
        T = 0
        shape = (rows, 3, n + 1)
        if lut is not None:
            lut, pl = _c(lut, np.uint32)
            if lut.size != rows:
                raise ValueError("debug_chunk_exit: lut is [rows]")
        if tables is not None:
            tables, pt = _c(tables, np.uint8)
            if tables.ndim != 2 or tables.shape[0] != rows:
                raise ValueError("debug_chunk_exit: tables is [rows][T]")
            T = tables.shape[1]
            shape = (rows, T, 3, n + 1)
        raw = raw or rns2
        out = np.zeros(shape + (2,) if raw else shape, dtype=np.uint64)
        acc = np.zeros((rows, 2, m, 2), dtype=np.uint64) if want_acc else None
        self._call("sgfhe_debug_chunk_exit", pd, rows, pl, pt, T, (FLAG_RAW_MODQ if raw else 0) | (FLAG_RAW_RNS2 if rns2 else 0),
                   out.ctypes.data_as(ctypes.c_void_p), acc.ctypes.data_as(ctypes.c_void_p) if want_acc else None)
        return (out, acc) if want_acc else out

    def debug_circuit_script_calls(self, circuit, count, ct=False, steps=None, emit=None, pack=False, direct=False,
                                   lift=False):
        """The scripted calls of a debug_circuit_script run (sgfhe_debug_circuit_script_calls), in the run's call order:
        a list of (rows, un-reduced).  count: instances, or with ct=True blocks; steps: None for a one-shot run."""
        form = (SCRIPT_CT if ct else 0) | (SCRIPT_STEPPED if steps is not None else 0)
        _e, pe, _n = self._emit_arg(emit, steps) if steps is not None else (None, None, 1)
        args = (circuit.handle(), form, count, steps or 0, pe, int(pack), _pack_flags(direct, lift))
        k = ctypes.c_size_t(0)
        self._call("sgfhe_debug_circuit_script_calls", *args, ctypes.byref(k), None, None, 0)
        rows, raw = np.zeros(k.value, dtype=np.uint32), np.zeros(k.value, dtype=np.uint8)
        self._call("sgfhe_debug_circuit_script_calls", *args, ctypes.byref(k), _hptr(rows), _hptr(raw), k.value)
        return [(int(x), bool(y)) for x, y in zip(rows, raw)]

    def debug_circuit_script(self, circuit, results, inputs, state=None, stepped=False, data=None, emit=None, pack=False,
                             direct=False, lift=False, state_in_place=False):
        """A circuit run whose bootstrap calls and pack tail are scripted (sgfhe_debug_circuit_script): the glue kernels
        of a real run on chosen words, without a key.
        inputs: the LWE form's array ([n_inputs][instances][n + 1]; stepped: [steps][stream inputs][instances][n + 1]) or
        a pair (a, b) of the ciphertext form's ([n_inputs][blocks][N]; stepped: [steps][stream inputs][blocks][N]).
        state: stepped: [registers][instances][n + 1], a pair (state_a, state_b), or None.  data, emit: as in the run of
        that form.  pack (ciphertext form): the run has a pack stage; direct, lift: its flags.  state_in_place (LWE form,
        stepped): the registers after the last step are written over `state`, which must then be a C-contiguous uint64
        array: state_out is the very array state_in is.
        results: one array per scripted call, in the order and of the rows of debug_circuit_script_calls: [rows][3][n + 1]
        words of Z_r, or [rows][3][n + 1][2] residues of an un-reduced call.
        Returns a dict: `out` the LWE outputs as the run of that form returns them, `state` (stepped) the registers after
        the last step, `staged` a list of [rows][2][n + 1] per call (input 1, input 2; a then b), `lut` a list of [rows]
        descriptor words per call, `tail_in` [emitted steps][n_outputs * blocks][n][n + 1][2] (pack) or None, `calls`."""
        p = self.params
        n = p.n
        ct = isinstance(inputs, tuple)
        if ct:
            a, pa = _c(inputs[0])
            b, pb = _c(inputs[1])
            if a.shape != b.shape or a.ndim != (4 if stepped else 3):
                raise ValueError("debug_circuit_script: a and b are [n_inputs][blocks][N], with [steps] in front when stepped")
            count, N = a.shape[-2], a.shape[-1]
            inst = count * n
        else:
            a, pa = _c(inputs)
            pb, N = None, 0
            if a.ndim != (4 if stepped else 3) or a.shape[-1] != n + 1:
                raise ValueError("debug_circuit_script: inputs are [n_inputs][instances][n + 1], with [steps] in front when stepped")
            count = inst = a.shape[-2]
        steps = a.shape[0] if stepped else None
        if a.shape[-3] != circuit.n_inputs - (circuit.n_regs if stepped else 0):
            raise ValueError("debug_circuit_script: one input per input wire the caller brings")
        psa = psb = None
        if state is not None:
            if ct:
                sa, psa = _c(state[0])
                sb, psb = _c(state[1])
            else:
                sa, psa = _c(state)
        if stepped:
            d, pd, e, pe, emitted = self._step_args(circuit, data, emit, steps, inst)
        else:
            (d, pd), pe, emitted = self._planes(circuit, data, inst), None, 1
        pack = bool(pack or direct or lift)
        calls = self.debug_circuit_script_calls(circuit, count, ct, steps, emit, pack, direct, lift) if count else []
        if len(results) != len(calls):
            raise ValueError("debug_circuit_script: %d scripted calls, %d result arrays" % (len(calls), len(results)))
        flat = []
        for i, ((rows, raw), res) in enumerate(zip(calls, results)):
            res = np.ascontiguousarray(res, dtype=np.uint64)
            if res.shape != (rows, 3, n + 1) + ((2,) if raw else ()):
                raise ValueError("debug_circuit_script: call %d takes %s, got %s"
                                 % (i, (rows, 3, n + 1) + ((2,) if raw else ()), res.shape))
            flat.append(res.reshape(-1))
        script = np.concatenate(flat) if flat else np.zeros(1, dtype=np.uint64)
        total = sum(rows for rows, _ in calls)
        staged = np.zeros((max(total, 1), 2, n + 1), dtype=np.uint64)
        lut = np.zeros(max(total, 1), dtype=np.uint32)
        n_ct = circuit.n_outputs * count
        tail = np.zeros((emitted, n_ct, n, n + 1, 2), dtype=np.uint64) if pack else None
        out = np.zeros(((emitted,) if stepped else ()) + (circuit.n_outputs, inst, n + 1), dtype=np.uint64)
        st = np.zeros((circuit.n_regs, inst, n + 1), dtype=np.uint64) if stepped else None
        if state_in_place:
            if ct or state is None or sa is not state:
                raise ValueError("debug_circuit_script: state_in_place takes the LWE form's state as a contiguous uint64 array")
            st = sa
        form = (SCRIPT_CT if ct else 0) | (SCRIPT_STEPPED if stepped else 0)
        self._call("sgfhe_debug_circuit_script", circuit.handle(), form, count, steps or 0, psa, psb, pa, pb, N, pd, pe,
                   _hptr(out), _hptr(st), _pack_flags(direct, lift) if ct else 0, _hptr(script), _hptr(staged), _hptr(lut),
                   _hptr(tail))
        cuts = np.cumsum([rows for rows, _ in calls])[:-1] if calls else []
        return {"out": out, "state": st, "staged": np.split(staged[:total], cuts) if calls else [],
                "lut": np.split(lut[:total], cuts) if calls else [], "tail_in": tail, "calls": calls}

    def debug_ntt(self, prime_index, poly, inverse=False):
        x, px = _c(poly, np.uint32)
        out = np.zeros(self.params.m, dtype=np.uint32)
        self._call("sgfhe_debug_ntt", prime_index, int(inverse), px,
                                          out.ctypes.data_as(ctypes.c_void_p))
        return out

    def primes(self):
        cnt = ctypes.c_uint32()
        arr = (ctypes.c_uint32 * 8)()
        self._call("sgfhe_debug_primes", ctypes.byref(cnt), arr)
        return [int(arr[i]) for i in range(cnt.value)]

    # ---- measurement ----------------------------------------------------------------------------
    def timing_enable(self, on=True):
        self._call("sgfhe_timing_enable", int(on))

    def build_id(self):
        """sgfhe_build_id() of the loaded library: hash of the kernel sources it was compiled from
        (+ ablation flags)."""
        return self._L.sgfhe_build_id().decode()

    def kernel_names(self):
        """(external-product kernel, CRT kernel) of the k-loop in the present flatten mode, as a
        rocprofv3 kernel trace names them (sgfhe_kernel_names)."""
        a, b = ctypes.create_string_buffer(64), ctypes.create_string_buffer(64)
        self._call("sgfhe_kernel_names", a, 64, b, 64)
        return a.value.decode(), b.value.decode()

    def release_host_staging(self):
        """Free the device and page-locked staging buffers bootstrap_batch keeps on the ctx."""
        self._call("sgfhe_release_host_staging")

    def timing_read(self, reset=True):
        st = (ctypes.c_double * 8)()
        self._call("sgfhe_timing_read", st, int(reset))
        return dict(extprod_ms=st[0], extprod_samples=int(st[1]), crt_ms=st[2],
                    crt_samples=int(st[3]), chunk=int(st[4]), call_ms=st[5], calls=int(st[6]),
                    call_batch=st[7])
