"""Key files: sorted canonical keys, optionally with their counts, at any odd k -- the format stated in numpy.

A key is the bit index the whole project uses, canonical(kmer) >> 1, 0 <= key < 2^(2k-1).  Everything is little-endian.

Header, 32 bytes:
     0  8 bytes  magic b"BRXKMERS"
     8  u8       version = 1
     9  u8       k (odd, 5..31)
    10  u8       flags: bit 0 = a count byte per key follows each block's keys; the other bits are 0
    11  u8       floor: 0 in a set file; in a count file the smallest count that was kept (>= 1)
    12  u32      keys per block = 256
    16  u64      n_keys
    24  u64      sum of all keys mod 2^64 (Pcon.fingerprint()[1])

then ceil(n_keys / 256) blocks; block b holds keys [256 b, min(n, 256 b + 256)), m of them, strictly increasing over the
whole file:
    u64                     the block's first key
    u8                      width w (0..61): the bit length of the largest key[i] - key[i-1] - 1 inside the block
    ceil((m-1) * w / 8) B   the m-1 values key[i] - key[i-1] - 1, value j in bits [j*w, (j+1)*w) of the bytes read as a
                            little-endian bit stream (bit 0 = least significant bit of the first byte), padding bits 0
    m bytes                 (flag bit 0) the counts, each in 1..255 and >= floor

The encoding is canonical (minimal w, zero padding, exact block sizes): a file is a function of its contents.  This module
is the expected value of the GPU path (br_amd/csrc/brx_keyfile.hip), as cover.py and abundance.py are for theirs: it needs
no GPU and no library."""
from __future__ import annotations

import struct
from typing import Optional, Tuple

import numpy as np

MAGIC = b"BRXKMERS"
VERSION = 1
BLOCK = 256
HEADER_BYTES = 32
FLAG_COUNTS = 1
MAX_WIDTH = 61
_HEADER = struct.Struct("<8sBBBBIQQ")


def is_keyfile(head_bytes: bytes) -> bool:
    """whether a stream that starts with these bytes (8 are enough) is a key file"""
    return bytes(head_bytes[:8]) == MAGIC


def _bit_length(v: np.ndarray) -> int:
    m = int(v.max()) if v.size else 0
    return m.bit_length()


def _pack_values(vals: np.ndarray, w: int) -> bytes:
    """vals (uint64, each below 2^w) as a little-endian bit stream of w bits per value, zero padded to a byte"""
    if w == 0 or vals.size == 0:
        return b""
    shifts = np.arange(w, dtype=np.uint64)
    bits = ((vals[:, None] >> shifts[None, :]) & np.uint64(1)).astype(np.uint8).reshape(-1)
    return np.packbits(bits, bitorder="little").tobytes()


def _unpack_values(buf: np.ndarray, n: int, w: int) -> np.ndarray:
    if w == 0 or n == 0:
        return np.zeros(n, dtype=np.uint64)
    bits = np.unpackbits(buf, bitorder="little")
    if bits[n * w:].any():
        raise ValueError("key file: padding bits are not zero")
    weights = np.uint64(1) << np.arange(w, dtype=np.uint64)
    return (bits[:n * w].reshape(n, w).astype(np.uint64) * weights[None, :]).sum(axis=1, dtype=np.uint64)


def _check_k(k: int) -> None:
    if not (5 <= k <= 31 and k & 1):
        raise ValueError(f"key file: k={k} (odd k from 5 to 31)")


def encode(k: int, keys, counts=None, floor: int = 0) -> bytes:
    """the key file of `keys` (strictly increasing, each below 2^(2k-1)), with `counts` (1..255 each, >= floor) if given"""
    _check_k(k)
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    n = keys.size
    if n and int(keys[-1]) >= 1 << (2 * k - 1):
        raise ValueError(f"key file: key {int(keys[-1])} is not below 2^{2 * k - 1}")
    if n > 1 and not (keys[1:] > keys[:-1]).all():
        raise ValueError("key file: keys must be strictly increasing")
    flags = 0
    if counts is not None:
        counts = np.ascontiguousarray(counts, dtype=np.uint8)
        if counts.size != n:
            raise ValueError("key file: one count per key")
        if not 1 <= floor <= 255:
            raise ValueError("key file: a count file's floor is 1..255")
        if n and int(counts.min()) < floor:
            raise ValueError("key file: a count below the floor")
        flags = FLAG_COUNTS
    elif floor:
        raise ValueError("key file: a set file's floor is 0")
    total = int(keys.sum(dtype=np.uint64)) if n else 0
    out = [_HEADER.pack(MAGIC, VERSION, k, flags, floor, BLOCK, n, total)]
    for lo in range(0, n, BLOCK):
        blk = keys[lo:lo + BLOCK]
        vals = blk[1:] - blk[:-1] - np.uint64(1)
        w = _bit_length(vals)
        out.append(struct.pack("<QB", int(blk[0]), w))
        out.append(_pack_values(vals, w))
        if counts is not None:
            out.append(counts[lo:lo + BLOCK].tobytes())
    return b"".join(out)


def _header(head: bytes) -> dict:
    if len(head) < HEADER_BYTES:
        if len(head) >= 8 and head[:8] != MAGIC:
            raise ValueError("key file: wrong magic")
        raise ValueError("key file: truncated header")
    magic, version, k, flags, floor, block, n, total = _HEADER.unpack(head[:HEADER_BYTES])
    if magic != MAGIC:
        raise ValueError("key file: wrong magic")
    if version != VERSION:
        raise ValueError(f"key file: version {version} (this reader knows version {VERSION})")
    if block != BLOCK:
        raise ValueError(f"key file: {block} keys per block (must be {BLOCK})")
    _check_k(k)
    if flags & ~FLAG_COUNTS:
        raise ValueError(f"key file: unknown flags {flags:#x}")
    if flags & FLAG_COUNTS:
        if floor < 1:
            raise ValueError("key file: a count file's floor is at least 1")
    elif floor:
        raise ValueError("key file: a set file's floor is 0")
    if n > 1 << (2 * k - 1):
        raise ValueError(f"key file: {n} keys, only {1 << (2 * k - 1)} exist at k={k}")
    return {"version": version, "k": k, "flags": flags, "counts": bool(flags & FLAG_COUNTS), "floor": floor, "block": block,
            "n_keys": n, "key_sum": total}


def peek(f) -> dict:
    """the header of the key file that binary file object `f` is positioned at, as a dict (32 bytes are consumed)"""
    return _header(f.read(HEADER_BYTES))


def decode(data: bytes) -> Tuple[int, np.ndarray, Optional[np.ndarray], int]:
    """(k, keys uint64[n], counts uint8[n] or None, floor) of a key file; ValueError names what is wrong with a bad one"""
    data = bytes(data)
    h = _header(data)
    k, n, with_counts, floor = h["k"], h["n_keys"], h["counts"], h["floor"]
    buf = np.frombuffer(data, dtype=np.uint8)
    limit = 1 << (2 * k - 1)
    keys = np.zeros(n, dtype=np.uint64)
    counts = np.zeros(n, dtype=np.uint8) if with_counts else None
    pos, last = HEADER_BYTES, -1
    for lo in range(0, n, BLOCK):
        m = min(BLOCK, n - lo)
        if pos + 9 > len(data):
            raise ValueError(f"key file: truncated in block {lo // BLOCK}")
        first, w = struct.unpack_from("<QB", data, pos)
        pos += 9
        if w > MAX_WIDTH:
            raise ValueError(f"key file: width {w} in block {lo // BLOCK} (at most {MAX_WIDTH})")
        nb = ((m - 1) * w + 7) // 8
        if pos + nb + (m if with_counts else 0) > len(data):
            raise ValueError(f"key file: truncated in block {lo // BLOCK}")
        vals = _unpack_values(buf[pos:pos + nb], m - 1, w)
        pos += nb
        if first <= last:
            raise ValueError(f"key file: block {lo // BLOCK} does not start above the key before it")
        # the block's last key in python integers (255 values of 61 bits do not fit 64): below the limit, nothing wraps
        span = (int((vals >> np.uint64(32)).sum(dtype=np.uint64)) << 32) + int((vals & np.uint64(0xffffffff)).sum(dtype=np.uint64))
        last = first + span + (m - 1)
        if last >= limit:
            raise ValueError(f"key file: a key of block {lo // BLOCK} is not below 2^{2 * k - 1}")
        if w != _bit_length(vals):
            raise ValueError(f"key file: width {w} of block {lo // BLOCK} is not minimal")
        keys[lo] = first
        keys[lo + 1:lo + m] = np.uint64(first) + np.cumsum(vals + np.uint64(1), dtype=np.uint64)
        if with_counts:
            c = buf[pos:pos + m]
            pos += m
            if int(c.min()) == 0:
                raise ValueError(f"key file: a count of 0 in block {lo // BLOCK}")
            if int(c.min()) < floor:
                raise ValueError(f"key file: a count below the floor {floor} in block {lo // BLOCK}")
            counts[lo:lo + m] = c
    if pos != len(data):
        raise ValueError(f"key file: {len(data) - pos} trailing bytes")
    if (int(keys.sum(dtype=np.uint64)) if n else 0) != h["key_sum"]:
        raise ValueError("key file: the key sum does not match")
    return k, keys, counts, floor
