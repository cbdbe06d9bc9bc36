"""Plain-Python restatement of the keyed stereogram noise, written from the definition's text and not from
csrc/chacha.h: the ChaCha block function with a 64-bit counter, the pixel addressing and the seed expansion.  A plain module:
no test lives here."""
import struct

import numpy as np

M32 = 0xffffffff
CONSTANTS = struct.unpack("<4I", b"expand 32-byte k")
MUL, INC = 6364136223846793005, 11634580027462260723


def _rotl(v, n):
    return ((v << n) | (v >> (32 - n))) & M32


def _quarter(s, a, b, c, d):
    s[a] = (s[a] + s[b]) & M32; s[d] = _rotl(s[d] ^ s[a], 16)
    s[c] = (s[c] + s[d]) & M32; s[b] = _rotl(s[b] ^ s[c], 12)
    s[a] = (s[a] + s[b]) & M32; s[d] = _rotl(s[d] ^ s[a], 8)
    s[c] = (s[c] + s[d]) & M32; s[b] = _rotl(s[b] ^ s[c], 7)


def block_words(key: bytes, counter: int, rounds: int = 12):
    """the sixteen u32 words of block `counter`"""
    assert len(key) == 32 and rounds % 2 == 0 and 0 <= counter < 1 << 64
    start = list(CONSTANTS) + list(struct.unpack("<8I", key)) + [counter & M32, counter >> 32, 0, 0]
    s = list(start)
    for _ in range(rounds // 2):
        _quarter(s, 0, 4, 8, 12); _quarter(s, 1, 5, 9, 13); _quarter(s, 2, 6, 10, 14); _quarter(s, 3, 7, 11, 15)
        _quarter(s, 0, 5, 10, 15); _quarter(s, 1, 6, 11, 12); _quarter(s, 2, 7, 8, 13); _quarter(s, 3, 4, 9, 14)
    return [(a + b) & M32 for a, b in zip(s, start)]


def block_bytes(key: bytes, counter: int, rounds: int = 12) -> bytes:
    return struct.pack("<16I", *block_words(key, counter, rounds))


def keystream(key: bytes, nbytes: int, rounds: int = 12) -> bytes:
    return b"".join(block_bytes(key, c, rounds) for c in range((nbytes + 63) // 64))[:nbytes]


def key_from_seed(seed: int) -> bytes:
    state, out = seed & (2**64 - 1), b""
    for _ in range(8):
        state = (state * MUL + INC) % 2**64
        xs = (((state >> 18) ^ state) >> 27) & M32
        rot = state >> 59
        out += struct.pack("<I", ((xs >> rot) | (xs << (32 - rot))) & M32 if rot else xs)
    return out


def noise(key: bytes, out_w: int, out_h: int) -> np.ndarray:
    """u8 [out_h, out_w, 3]: pixel i = y * out_w + x takes word i & 15 of block i >> 4; R, G, B are its three low bytes"""
    pixels = out_w * out_h
    words = []
    for c in range((pixels + 15) // 16):
        words += block_words(key, c)
    w = np.array(words[:pixels], np.uint32)
    rgb = np.stack([w & 255, (w >> 8) & 255, (w >> 16) & 255], axis=-1).astype(np.uint8)
    return rgb.reshape(out_h, out_w, 3)
