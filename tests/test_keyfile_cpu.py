"""The key-file format as br_amd/keyfile.py states it in numpy (no GPU, no library): the hand-checkable vectors, the sizes
on the reference's fixture, the canonical form and every refusal."""
import io
import struct

import numpy as np
import pytest

from br_amd import abundance, keyfile

VEC_SET_K5 = "4252584b4d45525301050000000100000300000000000000110000000000000003000000000000000328"
VEC_COUNT_K5 = "4252584b4d4552530105010100010000030000000000000011000000000000000300000000000000032801ff07"
VEC_K31 = "4252584b4d455253011f0000000100000200000000000000ffffffffffffff1f00000000000000003dfeffffffffffff1f"
VEC_EMPTY_K7 = "4252584b4d455253010700000001000000000000000000000000000000000000"


def _u64(*v):
    return np.array(v, dtype=np.uint64)


# ---- the four vectors, both ways ----------------------------------------------------------------------------------------
def test_vector_set_k5():
    data = bytes.fromhex(VEC_SET_K5)
    assert keyfile.encode(5, _u64(3, 4, 10)) == data
    k, keys, counts, floor = keyfile.decode(data)
    assert (k, keys.tolist(), counts, floor) == (5, [3, 4, 10], None, 0)


def test_vector_counts_k5():
    data = bytes.fromhex(VEC_COUNT_K5)
    assert keyfile.encode(5, _u64(3, 4, 10), np.array([1, 255, 7], dtype=np.uint8), floor=1) == data
    k, keys, counts, floor = keyfile.decode(data)
    assert (k, keys.tolist(), counts.tolist(), floor) == (5, [3, 4, 10], [1, 255, 7], 1)


def test_vector_k31_width_61():
    data = bytes.fromhex(VEC_K31)
    assert keyfile.encode(31, _u64(0, 2 ** 61 - 1)) == data
    k, keys, counts, floor = keyfile.decode(data)
    assert (k, keys.tolist(), counts, floor) == (31, [0, 2 ** 61 - 1], None, 0)
    assert data[40] == 61  # a delta of 2^61 - 1 is stored as 2^61 - 2: 61 bits


def test_vector_empty_k7():
    data = bytes.fromhex(VEC_EMPTY_K7)
    assert len(data) == 32
    assert keyfile.encode(7, _u64()) == data
    k, keys, counts, floor = keyfile.decode(data)
    assert (k, keys.size, counts, floor) == (7, 0, None, 0)


def test_peek_and_sniff():
    data = bytes.fromhex(VEC_COUNT_K5)
    h = keyfile.peek(io.BytesIO(data))
    assert (h["k"], h["counts"], h["floor"], h["n_keys"], h["key_sum"], h["block"]) == (5, True, 1, 3, 17, 256)
    assert keyfile.is_keyfile(data[:8]) and keyfile.is_keyfile(data)
    assert not keyfile.is_keyfile(b"\x0b" + bytes(40)) and not keyfile.is_keyfile(b"BRX")


# ---- the sizes on the reference's fixture -------------------------------------------------------------------------------
SIZES = {11: (1064470, 661134, 114187, 123072), 19: (4043870, 1131757, 310894, 105482),
         25: (6637423, 1312190, 461038, 103914), 31: (9512636, 1452465, 609461, 102678)}


@pytest.mark.parametrize("k", sorted(SIZES))
def test_fixture_sizes_and_round_trip(raw_reads, k):
    count_bytes, n_all, set_bytes, n_solid = SIZES[k]
    keys, counts = abundance.count_table([abundance.canonical_hashes(r, k) for r in raw_reads])
    assert keys.size == n_all
    cf = keyfile.encode(k, keys, counts, floor=1)
    assert len(cf) == count_bytes
    k2, keys2, counts2, floor2 = keyfile.decode(cf)
    assert (k2, floor2) == (k, 1) and np.array_equal(keys2, keys) and np.array_equal(counts2, counts)
    solid = keys[counts > 2]
    assert solid.size == n_solid
    sf = keyfile.encode(k, solid)
    assert len(sf) == set_bytes
    k3, keys3, counts3, floor3 = keyfile.decode(sf)
    assert (k3, counts3, floor3) == (k, None, 0) and np.array_equal(keys3, solid)


# ---- canonical form -----------------------------------------------------------------------------------------------------
def _blocks(data, with_counts):
    """[(first, w, value bytes, count bytes)] of a valid file, walked by the format's own rules"""
    n = struct.unpack_from("<Q", data, 16)[0]
    pos, out = 32, []
    for lo in range(0, n, 256):
        m = min(256, n - lo)
        first, w = struct.unpack_from("<QB", data, pos)
        nb = ((m - 1) * w + 7) // 8
        vals = data[pos + 9:pos + 9 + nb]
        pos += 9 + nb
        cnt = data[pos:pos + m] if with_counts else b""
        pos += len(cnt)
        out.append((first, w, vals, cnt))
    assert pos == len(data)
    return out


@pytest.mark.parametrize("n", [1, 255, 256, 257, 512])
def test_block_sizes(n):
    rng = np.random.default_rng(n)
    keys = np.sort(rng.choice(1 << 21, size=n, replace=False).astype(np.uint64))
    counts = rng.integers(1, 256, size=n).astype(np.uint8)
    data = keyfile.encode(11, keys, counts, floor=1)
    blocks = _blocks(data, True)
    assert len(blocks) == (n + 255) // 256
    for b, (first, w, vals, cnt) in enumerate(blocks):
        blk = keys[256 * b:256 * b + 256]
        assert first == int(blk[0]) and cnt == counts[256 * b:256 * b + 256].tobytes()
        d = (blk[1:] - blk[:-1] - np.uint64(1))
        assert w == (int(d.max()).bit_length() if d.size else 0)  # minimal width; 0 for a block of one key
        bits = np.unpackbits(np.frombuffer(vals, dtype=np.uint8), bitorder="little")
        assert not bits[(blk.size - 1) * w:].any()  # zero padding
    k, keys2, counts2, _ = keyfile.decode(data)
    assert np.array_equal(keys2, keys) and np.array_equal(counts2, counts)


def test_consecutive_keys_have_width_0():
    keys = np.arange(1000, 1300, dtype=np.uint64)
    data = keyfile.encode(9, keys)
    assert len(data) == 32 + 2 * 9
    assert [(f, w) for f, w, _, _ in _blocks(data, False)] == [(1000, 0), (1256, 0)]
    assert np.array_equal(keyfile.decode(data)[1], keys)


def test_one_wide_value_sets_the_width_of_its_block_only():
    keys = np.concatenate([np.arange(256, dtype=np.uint64), _u64(256, 2 ** 61 - 1)])
    data = keyfile.encode(31, keys)
    assert [w for _, w, _, _ in _blocks(data, False)] == [0, 61]
    assert np.array_equal(keyfile.decode(data)[1], keys)


def test_encode_refuses_bad_input():
    for bad in (lambda: keyfile.encode(6, _u64(1)), lambda: keyfile.encode(33, _u64(1)), lambda: keyfile.encode(5, _u64(3, 3)),
                lambda: keyfile.encode(5, _u64(4, 3)), lambda: keyfile.encode(5, _u64(512)),
                lambda: keyfile.encode(5, _u64(1), np.array([0], dtype=np.uint8), floor=1),
                lambda: keyfile.encode(5, _u64(1), np.array([2], dtype=np.uint8), floor=3),
                lambda: keyfile.encode(5, _u64(1), floor=1)):
        with pytest.raises(ValueError):
            bad()


# ---- refusals: each file differs from a valid one in exactly that respect -----------------------------------------------
def _valid(with_counts=True):
    rng = np.random.default_rng(5)
    keys = np.sort(rng.choice(1 << 17, size=600, replace=False).astype(np.uint64))
    counts = rng.integers(2, 256, size=600).astype(np.uint8) if with_counts else None
    return keys, counts, bytearray(keyfile.encode(9, keys, counts, floor=2 if with_counts else 0))


def _refused(data, word):
    with pytest.raises(ValueError) as ei:
        keyfile.decode(bytes(data))
    assert word in str(ei.value), str(ei.value)


def test_valid_file_decodes():
    keys, counts, data = _valid()
    k, keys2, counts2, floor = keyfile.decode(bytes(data))
    assert (k, floor) == (9, 2) and np.array_equal(keys, keys2) and np.array_equal(counts, counts2)


def test_refuses_wrong_magic():
    _, _, data = _valid()
    data[0] ^= 1
    _refused(data, "magic")


def test_refuses_wrong_version():
    _, _, data = _valid()
    data[8] = 2
    _refused(data, "version")


def test_refuses_wrong_block_size():
    _, _, data = _valid()
    struct.pack_into("<I", data, 12, 128)
    _refused(data, "per block")


@pytest.mark.parametrize("k", [8, 3, 33])
def test_refuses_even_or_out_of_range_k(k):
    _, _, data = _valid()
    data[9] = k
    _refused(data, "k=")


def test_refuses_key_out_of_range():
    # k = 9: keys below 2^17.  The last block's first key is moved up so that its last key leaves the range; the key sum
    # in the header is made to match, so that nothing else is wrong
    keys, counts, data = _valid()
    blocks = _blocks(bytes(data), True)
    pos = len(data) - (9 + len(blocks[-1][2]) + len(blocks[-1][3]))
    m = 600 - 512
    shift = (1 << 17) - int(keys[-1])
    struct.pack_into("<Q", data, pos, int(keys[512]) + shift)
    struct.pack_into("<Q", data, 24, (int(keys.sum(dtype=np.uint64)) + shift * m) % (1 << 64))
    _refused(data, "not below")


def test_refuses_zero_count_and_count_below_floor():
    _, _, data = _valid()
    low = bytearray(data)
    low[-1] = 1  # floor is 2
    _refused(low, "below the floor")
    data[-1] = 0
    _refused(data, "count of 0")


def test_refuses_wrong_key_sum():
    _, _, data = _valid()
    data[24] ^= 1
    _refused(data, "key sum")


def test_refuses_truncated_stream():
    _, _, data = _valid()
    _refused(data[:-1], "truncated")
    _refused(data[:40], "truncated")
    _refused(data[:20], "truncated")


def test_refuses_trailing_bytes():
    _, _, data = _valid()
    _refused(data + b"\x00", "trailing")


def test_refuses_blocks_out_of_order():
    keys, _, data = _valid(with_counts=False)
    blocks = _blocks(bytes(data), False)
    pos = 32 + 9 + len(blocks[0][2])  # the second block's first key: down to the first block's last key
    shift = int(keys[256]) - int(keys[255])
    struct.pack_into("<Q", data, pos, int(keys[255]))
    struct.pack_into("<Q", data, 24, (int(keys.sum(dtype=np.uint64)) - shift * 256) % (1 << 64))
    _refused(data, "does not start above")


def test_refuses_unknown_flags_and_floor_of_a_set_file():
    _, _, data = _valid(with_counts=False)
    bad = bytearray(data)
    bad[10] = 2
    _refused(bad, "flags")
    data[11] = 1
    _refused(data, "floor")
