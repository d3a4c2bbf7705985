"""Shared by tests/test_index_load_cpu.py and tests/test_gpu_index_load.py: <name>.hd / <name>.dl pairs written byte by byte —
lists no writer of ours lays down but the host reader accepts ("foreign"), and malformed lists spliced into the front of a copy
of golden/db/cars.dl — and the comparison of two loaded indexes word for word.  The yardsticks are these hand-written bytes,
refindex.py and the host reader (sg_index_load_reference), never the device decoder."""
import os
import struct

import numpy as np

import refindex
from index_store_shapes import SHAPES_DESC, type_prefix

FOREIGN_DESC = SHAPES_DESC
FOREIGN_SEGMENTS = 4
SG_E_INVALID = -1


def write_raw_index(hd_path, dl_path, n_indices, descriptors, dl_bytes, type_prefix_from, with_terms=True):
    """descriptors: [(term, indice, size, pos, raw_len)] written as they stand; dl_bytes: the whole .dl"""
    prefix = type_prefix(open(type_prefix_from, "rb").read())
    g = refindex._Gob(memoryview(open(type_prefix_from, "rb").read()))
    g.i = len(prefix)
    g.uint()
    type_id = g.int_()
    body = bytearray(refindex._gob_int(type_id))
    body += refindex._gob_uint(1) + refindex._gob_uint(4) + b"v5.1"
    body += refindex._gob_uint(1) + refindex._gob_uint(n_indices)
    if with_terms:
        body += refindex._gob_uint(1) + refindex._gob_uint(len(descriptors))
        for rec in descriptors:
            f = -1
            for idx, val in enumerate(rec):
                if not val:                                        # gob omits zero values
                    continue
                body += refindex._gob_uint(idx - f) + (refindex._gob_uint(len(val)) + val if idx == 0 else refindex._gob_uint(val))
                f = idx
            body += b"\x00"
    body += b"\x00"
    with open(hd_path, "wb") as fh:
        fh.write(prefix + refindex._gob_uint(len(body)) + bytes(body))
    with open(dl_path, "wb") as fh:
        fh.write(bytes(dl_bytes))


def _varints(deltas):
    return b"".join(refindex._enc_varint(d) for d in deltas)


def skip_blocks(values, sizes):
    """a skip list with blocks of the given numbers of values (0 = an empty block); the last block carries the flag"""
    out, at, first = bytearray(), 0, 0
    for bi, n in enumerate(sizes):
        blk = values[at:at + n]
        at += n
        deltas, prev = [], first
        for j, v in enumerate(blk):
            deltas.append((v - prev) & 0xFFFFFFFF)
            prev = v
            if j == 0:
                first = v
        body = _varints(deltas)
        out += struct.pack("<H", (len(body) + 2) | (0x8000 if bi == len(sizes) - 1 else 0)) + body
    assert at == len(values)
    return bytes(out)


def foreign_lists():
    """-> [(term, indice, raw_len, bytes, expected stored docIDs or None for a descriptor the reader skips)]"""
    out = []
    v = [3 + 5 * i for i in range(100)]
    out.append((b"aaa", 0, 100, skip_blocks(v, (1, 64, 35)), v))
    out.append((b"aab", 1, 2, refindex.encode_vb([5, 0xFFFFFFFF]), [5, 0xFFFFFFFF]))
    runs = struct.pack("<IBHH", 12347, 0x01, 2, 0) + struct.pack("<HHHHH", 2, 10, 299, 65530, 100)   # the second run overshoots 65 535
    out.append((b"aac", 2, 306, runs, [(2 << 16) + x for x in list(range(10, 310)) + list(range(65530, 65536))]))
    out.append((b"aad", 0, 3, b"", None))                          # size == 0
    out.append((b"aae", FOREIGN_SEGMENTS + 95, 1, b"\x07", None))  # indice >= Indices
    v = [11 + 3 * i for i in range(80)]
    out.append((b"aaf", 3, 80, skip_blocks(v, (70, 0, 10)), v))     # a block of more than 64 values, an empty one
    v = [1000 + 7 * i for i in range(66)]
    out.append((b"aag", 1, 66, skip_blocks(v, (0,) * 1100 + (66,)), v))   # 2 200 bytes of empty blocks first: beyond the LDS stage
    arr = [2 * i for i in range(300)]
    arr[5] = arr[4]                                                # an array container that repeats a value: not strictly ascending
    body = struct.pack("<IIHHI", 12346, 1, 7, 299, 16) + struct.pack("<300H", *arr)
    out.append((b"aah", 0, 300, body, [(7 << 16) + x for x in sorted(set(arr))]))
    keys = struct.pack("<IIHHHHII", 12346, 2, 9, 149, 4, 149, 24, 324)   # keys 9, then 4: descending
    body = keys + struct.pack("<150H", *range(150)) + struct.pack("<150H", *range(1, 151))
    out.append((b"aai", 2, 300, body, [(9 << 16) + x for x in range(150)] + [(4 << 16) + x for x in range(1, 151)]))
    full = struct.pack("<IBHH", 12347 | (1 << 16), 0x01, 0, 0) + struct.pack("<HH", 1, 4999)   # a run container, then a bitmap
    words = [0] * 1024
    bits = [3 * i + 1 for i in range(5000)]
    for b in bits:
        words[b >> 6] |= 1 << (b & 63)
    full += struct.pack("<HHH", 1, 0, 65535) + struct.pack("<1024Q", *words)
    out.append((b"aaj", 3, 65536 + 5000, full, list(range(65536)) + [(1 << 16) + b for b in bits]))
    return out


def foreign_files(tmp_path, golden_dir):
    """-> (hd, dl, {(indice, term): stored docIDs})"""
    dl, descs, want = bytearray(), [], {}
    for term, indice, raw, data, stored in foreign_lists():
        descs.append((term, indice, len(data), len(dl), raw))
        dl += data
        if stored is not None:
            want[(indice, term)] = stored
    hd, dlp = str(tmp_path / "foreign.hd"), str(tmp_path / "foreign.dl")
    write_raw_index(hd, dlp, FOREIGN_SEGMENTS, descs, dl, os.path.join(golden_dir, "db", "words_subset.hd"))
    return hd, dlp, want


def no_terms_files(tmp_path, golden_dir):
    hd, dl = str(tmp_path / "noterms.hd"), str(tmp_path / "noterms.dl")
    write_raw_index(hd, dl, FOREIGN_SEGMENTS, [], b"", os.path.join(golden_dir, "db", "words_subset.hd"), with_terms=False)
    return hd, dl


def pair_twice_files(tmp_path, golden_dir):
    """one (term, segment) pair with two lists: the host reader lets the later one win (the first is no longer than it)"""
    first, second, other = refindex.encode_vb([3, 8, 9]), refindex.encode_vb([2, 4, 6, 8, 10]), refindex.encode_vb([1, 7])
    descs = [(b"aaa", 1, len(first), 0, 3), (b"aab", 0, len(other), len(first), 2), (b"aaa", 1, len(second), len(first) + len(other), 5)]
    hd, dl = str(tmp_path / "twice.hd"), str(tmp_path / "twice.dl")
    write_raw_index(hd, dl, FOREIGN_SEGMENTS, descs, first + other + second, os.path.join(golden_dir, "db", "words_subset.hd"))
    return hd, dl, {(1, b"aaa"): (5, [2, 4, 6, 8, 10]), (0, b"aab"): (2, [1, 7])}


def _patched(data, at, fmt, value):
    b = bytearray(data)
    struct.pack_into(fmt, b, at, value)
    return bytes(b)


def malformed_lists():
    """-> {name: (raw_len, bytes)}: each overruns its own end by less than 1 KB at the most"""
    v70 = [9 + 4 * i for i in range(70)]
    skip = refindex.encode_skipping(v70)
    second = struct.unpack_from("<H", skip, 0)[0] & 0x7FFF           # the second block's header
    two_keys = refindex.encode_roaring(list(range(0, 300, 2)) + [(1 << 16) + 3 * i for i in range(150)])
    one_key = refindex.encode_roaring([5 * i for i in range(300)])
    return {
        "varint_runs_off_the_end": (3, b"\x05\x06\x85"),
        "varint_of_six_bytes": (1, b"\x81\x81\x81\x81\x81\x01"),
        "vb_one_value_too_few": (4, refindex.encode_vb([4, 9, 12])),
        "skip_block_past_the_end": (70, _patched(skip, second, "<H", (struct.unpack_from("<H", skip, second)[0] & 0x7FFF) + 300 | 0x8000)),
        "skip_without_last_flag": (70, _patched(skip, second, "<H", struct.unpack_from("<H", skip, second)[0] & 0x7FFF)),
        "roaring_one_container_too_many": (300, _patched(two_keys, 4, "<I", 3)),
        "array_cardinality_past_the_end": (300, _patched(one_key, 10, "<H", 300 + 400 - 1)),
        "unknown_cookie": (300, _patched(one_key, 0, "<I", 12345)),
    }


MALFORMED_TERM = b"zzz"


def malformed_files(tmp_path, golden_dir, name):
    """cars.{hd,dl} with the malformed list `name` (term zzz, segment 0) in front: more than 128 KB of other lists follow it"""
    raw, bad = malformed_lists()[name]
    _, indices, terms = refindex.read_header(os.path.join(golden_dir, "db", "cars.hd"))
    cars = open(os.path.join(golden_dir, "db", "cars.dl"), "rb").read()
    assert len(cars) >= 128 << 10
    descs = [(MALFORMED_TERM, 0, len(bad), 0, raw)] + [(t, i, s, p + len(bad), n) for t, i, s, p, n in terms]
    hd, dl = str(tmp_path / (name + ".hd")), str(tmp_path / (name + ".dl"))
    write_raw_index(hd, dl, indices, descs, bad + cars, os.path.join(golden_dir, "db", "cars.hd"))
    return hd, dl


def load_ex(hd, dl, desc, device):
    """sg_index_load_reference_ex -> NGramIndex without a replica; raises _lib.SuggestHipError"""
    import ctypes as C
    from suggest_amd import NGramIndex, _lib
    from suggest_amd.index import _c_desc, _enc
    d, h = _c_desc(desc), C.c_void_p()
    _lib.check(_lib.lib().sg_index_load_reference_ex(_enc(hd), _enc(dl), C.byref(d), int(device), C.byref(h)))
    return NGramIndex(description=desc, upload=False, _handle=h)


def assert_same_index(a, b):
    """two handles hold the same host CSR: digests, the posting store and the offsets word for word, the counters, every list"""
    assert np.array_equal(a.raw_array("host_seg_off"), b.raw_array("host_seg_off"))
    assert np.array_equal(a.raw_array("host_postings"), b.raw_array("host_postings"))
    assert a.digest() == b.digest()
    sa, sb = a.stats(), b.stats()
    for key in ("n_docs", "n_segments", "n_terms", "n_lists", "n_postings", "n_postings_raw", "posting_bytes"):
        assert sa[key] == sb[key], key
    assert a.lists() == b.lists()
