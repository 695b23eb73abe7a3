"""CRC-16 (CCITT polynomial 0x1021, initial value 0: binascii.crc_hqx(msg, 0)) of encrypted 32-bit messages with ONE
bootstrap per CRC bit.  A CRC is GF(2)-linear: every output bit is the XOR of some message bits, and a weighted-sum
node (Circuit.xor, sgfhe_circuit_create_w) takes the XOR of up to 64 wires in one bootstrap -- a wire doubled over Z_r
encodes its bit as 0 or r / 2, and sums of those are XORs.  crc16_ccitt(32) is 16 such nodes after one refresh per
message bit (a weight of 2 doubles a wire's error, and a fresh encryption is already at the limit): 48 bootstraps per
message against the 202 of the same XORs as trees of two-input nodes, whose count is printed beside.
Run on a GPU box:  python examples/encrypted_crc.py [--direct] [blocks]
RLWE ciphertexts in and out (evaluate_circuit_ct): ciphertext i holds message bit i (bit 7 of byte 0 first) of n = 1024
messages per block, output ciphertext k bit k of their CRCs.  --direct packs the outputs from the gates' own rows
(SGFHE_CIRCUIT_PACK_DIRECT): every output is a gate row, so the pack stage runs no bootstrap at all."""
import binascii
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MESSAGE_BITS = 32


def xor_tree_nodes(M):
    """Two-input nodes of the same map as one XOR tree per row (a row of k ones: k - 1 nodes), inputs used as they are."""
    return int(sum(max(0, int(row.sum()) - 1) for row in np.asarray(M)))


def packed_phase_error(key, ct, bits):
    """Worst |phase - bit Dr| over the n message coefficients of a packed Ciphertext: what decrypt has before it snaps."""
    p = key.params
    w = np.asarray(ct.rlwe.a, dtype=np.uint64).astype(np.int64)
    acc = np.zeros(p.m, dtype=np.int64)
    for i in np.flatnonzero(np.asarray(key.key) & 1):            # the negacyclic product w s, one key bit at a time
        rolled = np.roll(w, i)
        rolled[:i] = -rolled[:i]
        acc += rolled
    d = (np.asarray(ct.rlwe.b, dtype=np.uint64)[:p.n].astype(np.int64) - acc[:p.n] - np.asarray(bits, dtype=np.int64) * p.Dr) % p.r
    return int(np.minimum(d, p.r - d).max())


def main(blocks=1, direct=False):
    import sgfhe_jl_amd as S
    rng = np.random.default_rng()
    params = S.Params(1024)
    n = params.n
    key = S.PrivateKey(params, rng)
    bkey = S.BootstrapKey(rng, key)
    inst = blocks * n
    msgs = rng.integers(0, 256, size=(inst, MESSAGE_BITS // 8)).astype(np.uint8)
    msgs[0], msgs[1] = 0, 255
    plain = np.unpackbits(msgs, axis=1).T.astype(bool)               # [32][inst], bit 7 of byte 0 first
    cts = [[S.encrypt(key, rng, plain[i, t * n:(t + 1) * n]) for t in range(blocks)] for i in range(MESSAGE_BITS)]
    circ = S.crc16_ccitt(MESSAGE_BITS)
    info = circ.info()
    t0 = time.time()
    outs = S.evaluate_circuit_ct(bkey, None, circ, cts, direct=direct)
    dt = time.time() - t0
    want = np.array([binascii.crc_hqx(bytes(m), 0) for m in msgs], dtype=np.int64)
    crcs = np.zeros(inst, dtype=np.int64)
    worst = 0
    for k, row in enumerate(outs):
        crcs += np.concatenate([S.decrypt(key, ct) for ct in row]).astype(np.int64) << k
        worst = max([worst] + [packed_phase_error(key, ct, (want[t * n:(t + 1) * n] >> k) & 1) for t, ct in enumerate(row)])
    assert np.array_equal(crcs, want), "wrong CRCs"
    pack = 0 if direct else circ.n_outputs
    tree = xor_tree_nodes(S.crc16_matrix(MESSAGE_BITS))
    print("CRC-16 of %d encrypted %d-bit messages at Params(1024), %d ciphertexts in, %d out, %s: %d levels, %d sum-node "
          "bootstraps per message (%d refreshes + %d parities) + %d in the pack stage = %d in all, %.2f s; the same XORs "
          "as trees of two-input nodes: %d per message (+ %d) = %d; worst packed phase error %d of Dr/2 = %d; all %d "
          "CRCs equal binascii.crc_hqx"
          % (inst, MESSAGE_BITS, MESSAGE_BITS * blocks, circ.n_outputs * blocks,
             "outputs direct" if direct else "outputs refreshed", info["levels"], info["nodes"], info["nodes"] - 16, 16,
             pack, (info["nodes"] + pack) * inst, dt, tree, pack, (tree + pack) * inst, worst, params.Dr // 2, inst))


if __name__ == "__main__":
    a = [int(v) for v in sys.argv[1:] if not v.startswith("--")]
    main(a[0] if a else 1, direct="--direct" in sys.argv[1:])
