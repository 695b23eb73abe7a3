"""Bootstrap-key generation on the device (sgfhe_bkey_generate: k_keygen_draw, k_shat, k_polymul_s, k_crt_acc in its
CANON mode, k_keygen_finish, k_key_transform, and k_key_derive on a ctx with two bases) on every ring of
tests/keygen_cases.py: the device-form blob of the generated key against the blob of the C oracle's key uploaded in the
ring's own form, byte for byte, header included -- at m = 64, 128 and 256, with 32, 64 and 128 key rows (less than a
batch of the generator, one batch, two), every noise bound from 0 to the largest accepted, the secret keys of all zeros,
all ones and one bit, and seeds none of whose bytes is zero.  A generated key that is slightly wrong still decrypts, so
everything here is equality of bytes; tests/test_keygen_host.py holds the oracle's key to the big-integer oracle's and
to the definition of the key on the same cases.  A bootstrap call in each flatten mode on the generated key then equals
the oracle's on the oracle's key: on the rings with a basis per mode the blob holds the larger basis only, and the
deterministic call is what reads the key k_key_derive made."""

import numpy as np
import pytest

import bigint_oracle as BO
import keygen_cases as KC
import ring_cases as RC
from conftest import oracle_threads

pytestmark = pytest.mark.gpu

ERR_INVALID_ARG = -1


def _blob(eng):
    import torch
    t = torch.empty(eng.key_device_form_bytes(), dtype=torch.uint8, device="cuda")
    eng.export_key_device_form(t.data_ptr())
    return t.cpu().numpy()


class Case:
    """One ring: the oracle, and two engines for the module -- `up` takes the oracle's keys, `gen` generates."""

    def __init__(self, S, oc, name):
        self.S, self.name = S, name
        self.rg = KC.ring(S, name)
        self.params = self.rg.params
        self.o = RC.oracles(oc, self.rg)[0]
        self.up, self.gen = S.Engine(self.params), S.Engine(self.params)

    def keys(self, case):
        """Both engines keyed for (noise, secret-key kind, seed) -> (secret key, the oracle's key)."""
        noise, kind, seed = case
        sk = KC.secret_key(self.o, self.rg, kind)
        bkey = self.o.bootstrap_key(sk, seed, noise=noise, threads=oracle_threads())   # (the default is every core)
        RC.upload(self.up, self.rg, bkey)
        self.gen.generate_key(sk, seed, noise=noise)
        return sk, bkey

    def close(self):
        self.up.close()
        self.gen.close()


@pytest.fixture(scope="module", params=KC.NAMES)
def case(S, oc, request):
    c = Case(S, oc, request.param)
    yield c
    c.close()


def _assert_same_blob(case, label):
    b1, b2 = _blob(case.up), _blob(case.gen)
    assert b1.shape == b2.shape and b1.size > 64
    bad = np.flatnonzero(b1 != b2)
    assert bad.size == 0, "%s, %s: %d of %d bytes differ, the first at %d" % (case.name, label, bad.size, b1.size, bad[0])


def test_blob_identity(case):
    """The ring's plain case: its own noise, the oracle's secret key, a small seed."""
    plain = KC.cases(case.rg)[0]
    assert plain == (case.rg.noise, "oracle", KC.SEEDS[0])
    case.keys(plain)
    assert case.gen.key_device_form_bytes() == case.up.key_device_form_bytes()
    _assert_same_blob(case, KC.case_id(plain))


def test_bootstrap_in_each_mode_on_the_generated_key(case):
    """Four gates on the generated key in every flatten mode of the ring = the oracle's bootstrap_batch on the oracle's
    key (randomised: call 0 of the stream; set_mode starts the counter again and holds kernel_names() to the table)."""
    S, rg, o, eng = case.S, case.rg, case.o, case.gen
    sk, bkey = case.keys(KC.cases(rg)[0])
    khat = o.key_transform(bkey, threads=oracle_threads())
    bits = np.array([0, 0, 0, 1, 1, 0, 1, 1], dtype=np.uint8)
    a, b = o.lwe_encrypt_bits(sk, bits, 603)
    args = (a[0::2], b[0::2], a[1::2], b[1::2])
    if len(rg.modes) == 2 and case.name in ("limb64", "synth32"):       # a basis per mode: k_key_derive ran
        eng.set_random_flatten(True, RC.KEY32)
        n_rnd = len(eng.primes())
        eng.set_random_flatten(False)
        assert len(eng.primes()) == n_rnd - 1
    try:
        for rnd in rg.modes:
            assert RC.set_mode(S, eng, rg, rnd)
            want = o.bootstrap_batch(khat, *args, opt=True, rnd=(RC.KEY32, 0) if rnd else None)
            assert np.array_equal(eng.bootstrap_batch(*args), want), (case.name, rnd)
            assert RC.set_mode(S, eng, rg, rnd)
            want = o.bootstrap_batch(khat, *args, raw=True, opt=True, rnd=(RC.KEY32, 0) if rnd else None)
            assert np.array_equal(eng.bootstrap_batch(*args, raw=True), want), (case.name, rnd, "raw")
    finally:
        eng.set_random_flatten(False)


def test_edges(case):
    """Blob identities only: at the larger noise bounds nothing decrypts.  m128 (64 rows, exactly one batch) runs every
    noise bound, secret key and seed of the table; every other ring -- limb64 and wide among them, n = 8 with 32 rows,
    and synth32 with two batches -- the largest noise bound, the all-ones secret key (the largest |a (*) s|, a gadget
    term on every row) and the all-zeros one (no gadget term, b = e)."""
    rg = case.rg
    if case.name == "m128":
        edges = KC.cases(rg)[1:]
        assert len(edges) == 9
    else:
        edges = [(KC.noise_max(rg.params.Q), "oracle", KC.SEEDS[0]), (rg.noise, "ones", KC.SEEDS[0]),
                 (rg.noise, "zeros", KC.SEEDS[0])]
        assert all(e in KC.cases(rg) for e in edges)
    for edge in edges:
        case.keys(edge)
        _assert_same_blob(case, KC.case_id(edge))


def test_batches_of_the_generator_are_covered(S):
    """32, 64 and 128 key rows: less than the generator's batch of 64 rows, one batch, two; m = 64, 128, 256."""
    shape = {name: (4 * KC.ring(S, name).params.n, KC.ring(S, name).params.m) for name in KC.NAMES}
    assert {rows for rows, _ in shape.values()} == {32, 64, 128}
    assert {m for _, m in shape.values()} == {64, 128, 256}
    assert shape["m128"] == (64, 128) and shape["synth32"] == (128, 256)


# ---- refusals ------------------------------------------------------------------------------------------------------------

def _random_key(params, seed):
    rng = np.random.default_rng(seed)
    key = np.zeros((params.n, 4, 2, params.m, 2), dtype=np.uint64)
    key[..., 0] = rng.integers(0, params.Q, size=key.shape[:-1], dtype=np.uint64)
    return key


def _refused(S, eng, params, code, **kw):
    """generate_key fails with `code`, and the key the ctx had keeps its bytes and its bootstraps."""
    rng = np.random.default_rng(611)
    args = (rng.integers(0, params.r, size=(3, params.n), dtype=np.uint64), rng.integers(0, params.r, size=3, dtype=np.uint64),
            rng.integers(0, params.r, size=(3, params.n), dtype=np.uint64), rng.integers(0, params.r, size=3, dtype=np.uint64))
    before, out = _blob(eng), eng.bootstrap_batch(*args)
    with pytest.raises(S.SgfheError) as ei:
        eng.generate_key(np.ones(params.n, dtype=np.uint64), KC.SEEDS[1], **kw)
    assert ei.value.code == code
    assert np.array_equal(_blob(eng), before)
    assert np.array_equal(eng.bootstrap_batch(*args), out)


def test_generation_is_refused_below_2_16(S):
    """A ring the ctx accepts (Q = 4481 < 2^16, B^2 >= Q): SGFHE_ERR_UNSUPPORTED at every noise bound, 0 included."""
    n = 8
    Q = BO.find_modulus(16 * n, 1 << 12)
    params = S.Params.custom(n, Q, 127)
    assert 3 <= Q < 1 << 16 and 127 * 127 >= Q
    eng = S.Engine(params)
    try:
        eng.upload_key(_random_key(params, 612))
        for noise in (0, 2, (Q - 1) // 2):
            _refused(S, eng, params, RC.ERR_UNSUPPORTED, noise=noise)
    finally:
        eng.close()


def test_noise_is_refused_at_the_boundary_value(S):
    """2 noise >= Q at noise = (Q + 1) / 2 itself, on the smallest ring the generator accepts; (Q - 1) / 2 is a case of
    the table."""
    rg = KC.ring(S, "q16")
    params = rg.params
    eng = S.Engine(params)
    try:
        eng.upload_key(_random_key(params, 613))
        assert KC.noise_max(params.Q) == (params.Q - 1) // 2
        _refused(S, eng, params, ERR_INVALID_ARG, noise=(params.Q + 1) // 2)
    finally:
        eng.close()
