"""CRC-16 (CCITT polynomial 0x1021, initial value 0: binascii.crc_hqx(msg, 0)) of encrypted messages of ANY whole number
of bytes, one byte per step of ONE stepped run.  crc16_stream(8) is a circuit with 16 registers -- the running CRC -- and
8 stream inputs -- the byte's bits: a step refreshes the 8 fresh bits and takes the 16 XORs of gf2_matvec over (state ++
byte), 24 bootstraps, and the 16 parity wires are both the outputs and the next state.  The registers stay on the device
between steps (sgfhe_circuit_run_steps_ct): the plan, the wire table and the call pattern do not depend on the length of
the message, where the unrolled crc16_ccitt(bits) has one input slot per message bit and rows of at most 64 ones.
Run on a GPU box:  python examples/encrypted_crc_stream.py [bytes] [blocks]
RLWE ciphertexts in and out (evaluate_circuit_steps_ct): ciphertext (s, i) holds bit i of byte s (bit 7 first) of n = 1024
messages per block; only the last step's outputs are packed and come down (emit), output ciphertext k holding bit k of the
CRCs.  Every output is a gate row, so direct=True packs them without a bootstrap."""
import binascii
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CHUNK_BITS = 8


def main(n_bytes=6, blocks=1):
    import sgfhe_jl_amd as S
    rng = np.random.default_rng()
    params = S.Params(1024)
    n = params.n
    key = S.PrivateKey(params, rng)
    bkey = S.BootstrapKey(rng, key)
    inst = blocks * n
    msgs = rng.integers(0, 256, size=(inst, n_bytes)).astype(np.uint8)
    msgs[0], msgs[1] = 0, 255
    plain = np.unpackbits(msgs, axis=1).T.astype(bool).reshape(n_bytes, CHUNK_BITS, inst)     # [step][bit][instance]
    cts = [[[S.encrypt(key, rng, plain[s, i, t * n:(t + 1) * n]) for t in range(blocks)] for i in range(CHUNK_BITS)]
           for s in range(n_bytes)]
    circ = S.crc16_stream(CHUNK_BITS)
    info = circ.info()
    emit = [False] * (n_bytes - 1) + [True]
    t0 = time.time()
    outs, _ = S.evaluate_circuit_steps_ct(bkey, None, circ, None, cts, direct=True, emit=emit)
    dt = time.time() - t0
    assert len(outs) == 1
    want = np.array([binascii.crc_hqx(bytes(m), 0) for m in msgs], dtype=np.int64)
    crcs = np.zeros(inst, dtype=np.int64)
    for k, row in enumerate(outs[0]):
        crcs += np.concatenate([S.decrypt(key, ct) for ct in row]).astype(np.int64) << k
    assert np.array_equal(crcs, want), "wrong CRCs"
    print("CRC-16 of %d encrypted messages of %d bytes at Params(1024) as one stepped run of %d steps: %d registers, %d "
          "ciphertexts in per step, %d out after the last; %d levels and %d bootstraps per message and step (%d refreshes "
          "+ 16 parities), %d in all, a wire table of %d slots whatever the length; %.2f s; all %d CRCs equal "
          "binascii.crc_hqx"
          % (inst, n_bytes, n_bytes, circ.n_regs, CHUNK_BITS * blocks, circ.n_outputs * blocks, info["levels"],
             info["nodes"], info["nodes"] - 16, info["nodes"] * n_bytes * inst, info["slots"], dt, inst))


if __name__ == "__main__":
    a = [int(v) for v in sys.argv[1:]]
    main(a[0] if a else 6, a[1] if len(a) > 1 else 1)
