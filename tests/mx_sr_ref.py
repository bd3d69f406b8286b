"""Independent CPU expectation for the stochastic MX quantize (include/ftar.h: ftar_mx_quantize_sr).  Nothing here
calls the library, and nothing here is new arithmetic: element i's product is mx_ref's (the exact widening times
q(s) of i's block, one float32 multiply: sr_ref.product_bits on the elements that share a scale byte) and its
narrowing is sr_ref.sr_cast_words on the word of element i -- words[i], or sr_ref.words(seed, offset + i).  So block
b of a call is sr_ref.sr_cast on that block with r = q(s_b) and offset + 32b, which tests/test_mx_sr_api.py checks.

Arrays travel as unsigned bit patterns (cast_ref.storage), scale bytes as uint8, words as uint32.  The scale bytes
themselves are mx_ref.scales: they do not depend on the rounding."""
import numpy as np

import cast_ref
import mx_ref
import sr_ref


def quantize_words(src_dt, f8, bits, sc, words):
    """What ftar_mx_quantize_sr stores with these scale bytes when element i's word is words[i]."""
    bits = np.asarray(bits).view(cast_ref.storage(src_dt))
    words = np.broadcast_to(np.asarray(words, dtype=np.uint32), bits.shape)
    per = mx_ref._per_element(sc, bits.size)
    out = np.zeros(bits.size, np.uint8)
    for s in np.unique(per):
        m = per == s
        out[m] = sr_ref.sr_cast_words(src_dt, f8, bits[m], mx_ref.q_bits(s), words[m])
    return out


def quantize(src_dt, f8, bits, sc, seed, offset=0):
    """What ftar_mx_quantize_sr stores with these scale bytes (given, or mx_ref.scales() for the compute mode), this
    seed value and this offset."""
    n = np.asarray(bits).size
    return quantize_words(src_dt, f8, bits, sc, sr_ref.words(seed, sr_ref.indices(offset, n)))
