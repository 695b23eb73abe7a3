"""The four key writers of the C ABI (sgfhe_bkey_upload, _upload_rns2, _generate, _import_device_form) and
sgfhe_ctx_clone, held to what a caller can observe of them: which refusals leave the previous key in place,
which leave a ctx without a key, that the writers replace one another's key on one ctx, and what a clone
starts with.  Keys from the oracle at n = 64: Params(64), and -- where limb pairs need Q = m1 m2 -- the same
ring over the composite modulus of two NTT-friendly primes (the rule of bench.rns2_moduli, src/fhe2.jl:57-58).
Four gates per call: the bytes come from the key, not from the batch."""

import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BITS = np.array([0, 0, 0, 1, 1, 0, 1, 1], dtype=np.uint8)
_CACHE = {}


def _moduli(S):
    import bench
    return bench.rns2_moduli(S, 64)                  # (B, Bp) = (m1, m2), both 1 mod 2 m


def _setup(S, oc, composite):
    """(params, oracle, secret key, canonical key K, the four gates' LWEs, the oracle's bootstrap of them)."""
    if composite not in _CACHE:
        if composite:
            B, Bp = _moduli(S)
            params = S.Params.custom(64, B * Bp, B)
            o = oc.Oracle.from_params(params, rns2=(B, Bp))
        else:
            params = S.Params(64)
            o = oc.Oracle.from_params(params)
        sk = o.private_key(61)
        bkey = o.bootstrap_key(sk, 62)
        a, b = o.lwe_encrypt_bits(sk, BITS, 63)
        gates = (a[0::2], b[0::2], a[1::2], b[1::2])
        _CACHE[composite] = (params, o, sk, bkey, gates, o.bootstrap_batch(bkey, *gates).tobytes())
    return _CACHE[composite]


def _refused(call, code=-1, text=None):
    with pytest.raises(Exception) as ei:
        call()
    assert getattr(ei.value, "code", None) == code, ei.value
    if text is not None:
        assert text in str(ei.value)


def _blob(eng):
    import torch
    blob = torch.empty(eng.key_device_form_bytes(), dtype=torch.uint8, device="cuda:0")
    eng.export_key_device_form(blob.data_ptr())
    return blob


def test_refused_arguments_keep_the_key(S, oc):
    """A writer that refuses its ARGUMENTS (word count, m1 m2 != Q, noise bound, blob header) returns
    SGFHE_ERR_INVALID_ARG before the first byte of the key changes: the same gates give the same bytes."""
    params, o, sk, bkey, gates, want = _setup(S, oc, False)
    eng = S.Engine(params)
    try:
        eng.upload_key(bkey)
        X = eng.bootstrap_batch(*gates).tobytes()
        assert X == want
        blob = _blob(eng)
        bad_blob = blob.clone()
        bad_blob[8] ^= 0x5A                                     # one byte of the header (the format version)
        m1, m2 = _moduli(S)
        assert m1 * m2 != params.Q
        flat = np.ascontiguousarray(bkey)

        def short_upload():                                     # the C check itself: Engine.upload_key refuses earlier
            rc = S.lib().sgfhe_bkey_upload(eng._h, flat.ctypes.data_as(ctypes.c_void_p), flat.size - 2)
            if rc:
                raise S.SgfheError(rc, S.lib().sgfhe_last_error_string(eng._h).decode())
        for call in (short_upload,
                     lambda: eng.upload_key_rns2(bkey, m1, m2),
                     lambda: eng.generate_key(sk, 64, noise=1 << 30),
                     lambda: eng.import_key_device_form(bad_blob.data_ptr())):
            _refused(call)
            assert eng.bootstrap_batch(*gates).tobytes() == X
    finally:
        eng.close()


def test_refused_contents_drop_the_key(S, oc):
    """A writer that finds a bad residue while it transforms the key has already begun to replace it: the call
    returns SGFHE_ERR_INVALID_ARG and the ctx refuses to bootstrap (SGFHE_ERR_NO_KEY) until a key is accepted."""
    params, o, sk, bkey, gates, want = _setup(S, oc, True)
    m1, m2 = _moduli(S)
    eng = S.Engine(params)
    try:
        eng.upload_key(bkey)
        X = eng.bootstrap_batch(*gates).tobytes()
        assert X == want
        pairs = eng.rns2_convert(bkey, m1, m2, to_pairs=True)
        bad = bkey.copy()
        bad[3, 1, 0, 7, 0] = params.Q & 0xFFFFFFFFFFFFFFFF      # == Q: not canonical
        bad[3, 1, 0, 7, 1] = params.Q >> 64
        _refused(lambda: eng.upload_key(bad), text="not in [0, Q)")
        _refused(lambda: eng.bootstrap_batch(*gates), code=-5)
        eng.upload_key(bkey)
        assert eng.bootstrap_batch(*gates).tobytes() == X
        bad = pairs.copy()
        bad[3, 1, 0, 7, 0] = m1                                 # v1 == m1: not a residue
        _refused(lambda: eng.upload_key_rns2(bad, m1, m2))
        _refused(lambda: eng.bootstrap_batch(*gates), code=-5)
        eng.upload_key(bkey)
        assert eng.bootstrap_batch(*gates).tobytes() == X
    finally:
        eng.close()


def test_writers_in_sequence_on_one_ctx(S, oc):
    """Upload, generate, import and the limb-pair upload one after another on one ctx: each replaces the key
    of the one before, and the three forms of K give the same bytes."""
    params, o, sk, bkey, gates, want = _setup(S, oc, True)
    m1, m2 = _moduli(S)
    eng = S.Engine(params)
    try:
        eng.upload_key(bkey)
        X = eng.bootstrap_batch(*gates).tobytes()
        assert X == want
        blob = _blob(eng)
        eng.generate_key(o.private_key(71), 72)
        assert eng.bootstrap_batch(*gates).tobytes() != X
        eng.import_key_device_form(blob.data_ptr())
        assert eng.bootstrap_batch(*gates).tobytes() == X
        pairs = eng.rns2_convert(bkey, m1, m2, to_pairs=True)
        eng.generate_key(o.private_key(71), 72)
        assert eng.bootstrap_batch(*gates).tobytes() != X
        eng.upload_key_rns2(pairs, m1, m2)
        assert eng.bootstrap_batch(*gates).tobytes() == X
    finally:
        eng.close()


def test_clone_starts_clean(S, oc):
    """A clone of a ctx in the randomised mode, after a randomised call and with changed knobs, starts in the
    deterministic mode with call counter 0, and keeps working when the ctx it came from goes first."""
    params, o, sk, bkey, gates, want = _setup(S, oc, False)
    rnd0 = o.bootstrap_batch(bkey, *gates, rnd=(5, 0)).tobytes()
    eng = S.Engine(params)
    cl = None
    try:
        eng.upload_key(bkey)
        eng.set_random_flatten(True, 5)
        assert eng.bootstrap_batch(*gates).tobytes() == rnd0    # the parent's counter now stands at 1
        eng.set_chunk(8)
        eng.set_lanes(1)
        cl = eng.clone()
        got = cl.bootstrap_batch(*gates).tobytes()
        eng.set_random_flatten(False)
        X = eng.bootstrap_batch(*gates).tobytes()
        assert X == want and got == X
        eng.close()                                             # the parent first
        assert cl.bootstrap_batch(*gates).tobytes() == X
        cl.set_random_flatten(True, 5)
        assert cl.bootstrap_batch(*gates).tobytes() == rnd0
    finally:
        eng.close()
        if cl is not None:
            cl.close()
