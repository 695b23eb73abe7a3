"""Are two encrypted words equal (sgfhe_circuit_create_masked): the words sit side by side in their ciphertexts, one bit
a lane, `width` lanes a word.  circuit.packed_equal(width) is one XNOR node on every lane and then a reduction over the
lanes of the word with AND (circuit.lane_reduce) whose stage k bootstraps only the lanes that are multiples of 2 k -- the
others are never read -- so a word costs 2 width - 1 bootstraps where a tree on all lanes costs width (1 + log2(width)).
The answer sits at lane 0 of every word, FALSE at the other lanes.
Run on a GPU box:  python examples/encrypted_equal.py [n] [width] [words]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(n=64, width=8, words=6):
    import sgfhe_jl_amd as S
    from encrypted_adder import encrypt_bits
    rng = np.random.default_rng()
    params = S.Params(n)
    key = S.PrivateKey(params, rng)
    bkey = S.BootstrapKey(rng, key)
    circ = S.packed_equal(width)
    x = rng.integers(0, 2, size=(words, width)).astype(bool)
    y = x.copy()
    for w in range(words // 2):                          # half of the words differ, in one bit
        y[2 * w + 1, rng.integers(width)] ^= True
    enc = [encrypt_bits(S, key, rng, v.reshape(-1)) for v in (x, y)]
    t0 = time.time()
    out = S.evaluate_circuit(bkey, None, circ, enc)[0]
    dt = time.time() - t0
    dec = np.array([S.decrypt(key, e) for e in out]).astype(bool).reshape(words, width)
    assert dec[:, 0].tolist() == [bool((p == q).all()) for p, q in zip(x, y)] and not dec[:, 1:].any(), "wrong answer"
    rows = circ.rows_per_group()
    print("equality of %d pairs of %d-bit words at Params(%d): %d nodes in %d levels, %d bootstraps a word (%d on all lanes), "
          "%.2f s; every answer right" % (words, width, n, circ.info()["nodes"], circ.info()["levels"], rows,
                                          width * circ.info()["nodes"], dt))
    return dt, rows * words


if __name__ == "__main__":
    main(*[int(v) for v in sys.argv[1:4]])
